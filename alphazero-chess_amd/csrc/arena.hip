// arena.hip -- evaluation games in HBM: one lockstep match engine behind two C ABIs.
//   az_arena_*       one match (validation.rs:155-402 evaluate): two players, or one player on both sides
//   az_tournament_*  a round robin's pairings (ratings.rs:10-24): match m = i (i - 1) / 2 + j is
//                    evaluate(&players[i], &players[j])
// A match is G games, its player 1 White in the even games and Black in the odd ones.  Engine game
// t = m * G + g is game g of match m; every game's positions, move list and result live on the device and
// one step plays one ply of every live game of every match:
//   k_match_stage   one wavefront per game: the games in which one player is to move, across all of its
//                   matches, are compacted into rows 0..n-1 (ascending in t); a base-model player's rows get
//                   their planes (plane_value: to_tensor, chess.rs:191-245) and ONE forward of n rows follows
//                   on the engine's stream; an MCTS player's rows are the slots of its one search, whose
//                   improved policy (search_launch_device) stays in device memory
//   k_match_pick    one wavefront per game: arena_pick (arena_dev.h) -- legal moves, the mover's choice (a
//                   policy row under validation.rs:297-308, a uniform entry of the legal-move list, or a
//                   given action) and its validation
//   k_match_commit  one wavefront per game, only if every choice of every match was valid: arena_commit
//   k_match_roots   one wavefront per slot of an MCTS player's search: the same compaction, and slot k's root
//                   records (position history, length, ply) copied from the game's own history in HBM
// The host keeps a mirror of results, sides to move and move lists: a MiniMax player's az_minimax_scores runs
// on the downloaded positions and an external seat's moves are the caller's; both reach the kernels as given
// actions.  With AZ_ARENA_DEVICE_ROOTS=0 an MCTS player's roots are set from the mirror instead
// (az_search_set_roots_from).
// An MCTS player searches with its own settings (az_player_search) on its search's own stream; the searches
// of one ply are launched first and, under AZ_ARENA_OVERLAP, run side by side -- players that name one
// az_net in player order -- before the engine's stream waits for them and goes on to stage / pick / commit.
// The engine is told which ABI it answers for, and only its messages depend on that.
#include <string.h>

#include <string>
#include <vector>

#include "arena_dev.h"

#pragma clang fp contract(off)

// AZ_ARENA_OVERLAP unset: on -- faster in every repeat of every case of profiles/arena_mcts_bench.txt's leg A
// 
#ifndef AZ_ARENA_OVERLAP_DEFAULT
#define AZ_ARENA_OVERLAP_DEFAULT 1
#endif

namespace azi {

struct MatchPlayerDev {
    int kind;
    int row_base;          // the player's first row of pol
};

// device state, passed by value.  io is one block the host reads back per step:
// [0] any bad choice, [1] live games after the ply, then status [T], chosen [T], result [T]
struct MatchDev {
    int T, G, nsm, pad;
    azc::Pos* poshist;     // [T][HMAX]: the position after k moves at [k] (the start at [0])
    int* moves;            // [T][HMAX]
    int* plies;            // [T]
    int* tomove;           // [T] player index of the mover, -1 once the game is over
    int* row;              // [T] row of the game among its mover's games to move
    int* io;
    const int* pair;       // [matches] player 1 | player 2 << 8 (equal: one player on both sides)
    const float* u;        // [T]
    const int* actions;    // [T]
    const float* pol;      // [rows][4096]: policy rows (base model) or improved-policy rows (MCTS) of all players
    MatchPlayerDev pl[AZ_TOURNAMENT_MAX_PLAYERS];
    __device__ __host__ int* status() const { return io + 2; }
    __device__ __host__ int* chosen() const { return io + 2 + T; }
    __device__ __host__ int* result() const { return io + 2 + 2 * T; }
};

// player 1 of the match is White in its even games
__device__ __host__ __forceinline__ int match_mover(int pair, int g, int turn) {
    return ((turn ^ g) & 1) ? (pair >> 8) : (pair & 255);
}

__global__ void __launch_bounds__(64) k_match_reset(MatchDev D, const azc::Pos* __restrict__ start) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= D.T) return;
    const int m = t / D.G, g = t - m * D.G;
    const azc::Pos p = start[g];
    D.poshist[(size_t)t * HMAX] = p;
    D.plies[t] = 0;
    D.tomove[t] = match_mover(D.pair[m], g, p.turn);
    D.row[t] = 0;
    D.result()[t] = azc::ONGOING;
}

// current position of every game, for the MiniMax players
__global__ void __launch_bounds__(64) k_match_positions(MatchDev D, azc::Pos* __restrict__ out) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= D.T) return;
    out[t] = D.poshist[(size_t)t * HMAX + min(D.plies[t], HMAX - 1)];
}

// planes == nullptr (an MCTS player): the rows only
__global__ void __launch_bounds__(64) k_match_stage(MatchDev D, int player, float* __restrict__ planes) {
    // the per-game records were written by vector stores of earlier launches: keep t in a VGPR
    const int t = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (t >= D.T || D.tomove[t] != player) return;
    // row = the lower games with the same mover; only the player's own matches can hold one (the pair
    // table is written once, at create)
    const int mt = t / D.G;
    int row = 0;
    for (int m = 0; m <= mt; m++) {
        const int pr = D.pair[m];
        if ((pr & 255) != player && (pr >> 8) != player) continue;
        const int end = m == mt ? t : (m + 1) * D.G;
        for (int j0 = m * D.G; j0 < end; j0 += 64) {
            const int j = j0 + lane;
            const bool same = j < end && D.tomove[j] == player;
            row += __popcll(__ballot(same));
        }
    }
    if (lane == 0) D.row[t] = row;
    if (!planes) return;
    const azc::Pos p = D.poshist[(size_t)t * HMAX + D.plies[t]];
    float* out = planes + (size_t)row * AZ_PLANES * 64;
    for (int e = lane; e < AZ_PLANES * 64; e += 64) out[e] = azc::plane_value(p, e >> 6, e & 63);
}

// The roots of `player`'s search, set where the games are.  Slot k takes the k-th game (ascending in t) in
// which the player is to move -- k_match_stage's rows -- and a spare slot the first of them: hist[0..plies]
// of the game copied in 16-byte pieces (only the entries that exist), hist_len = plies + 1, ply = plies,
// game id = k.  What az_search_set_roots_from builds from the start position and the move list: match_reset
// stores a finalized start, and arena_commit's leaf_rules leaves the flags and rep_key finalize computes.
static_assert(sizeof(azc::Pos) % 16 == 0, "k_match_roots copies positions as uint4");
__global__ void __launch_bounds__(64) k_match_roots(MatchDev D, int player, SearchRoots R) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= R.slots) return;
    const int M = D.T / D.G;
    int seen = 0, first = -1, hit = -1;                      // wave-uniform: they come from ballots
    for (int m = 0; m < M && hit < 0; m++) {
        const int pr = D.pair[m];
        if ((pr & 255) != player && (pr >> 8) != player) continue;
        const int end = (m + 1) * D.G;
        for (int j0 = m * D.G; j0 < end && hit < 0; j0 += 64) {
            const int j = j0 + lane;
            const bool same = j < end && D.tomove[j] == player;
            const unsigned long long mask = __ballot(same);
            if (!mask) continue;
            if (first < 0) first = j0 + __ffsll((long long)mask) - 1;
            const int c = __popcll(mask);
            if (k < seen + c) {                              // the (k - seen)-th mover of this chunk
                const bool mine = same && __popcll(mask & ((1ull << lane) - 1ull)) == k - seen;
                hit = j0 + __ffsll((long long)__ballot(mine)) - 1;
            }
            seen += c;
        }
    }
    if (first < 0) return;                                   // no game to move: the host launches nothing then
    // the game's records were written by vector stores of earlier launches: keep t in a VGPR
    const int t = vgpr_index(hit >= 0 ? hit : first);
    const int n = min(max(D.plies[t], 0), HMAX - 1) + 1;
    const uint4* src = reinterpret_cast<const uint4*>(D.poshist + (size_t)t * HMAX);
    uint4* dst = reinterpret_cast<uint4*>(R.hist + (size_t)k * HMAX);
    const int pieces = n * (int)(sizeof(azc::Pos) / 16);
    for (int i = lane; i < pieces; i += 64) dst[i] = src[i];
    if (lane == 0) {
        R.hist_len[k] = n;
        R.game_id[k] = k;
        R.ply[k] = n - 1;
        R.active[k] = 1;
    }
}

__global__ void __launch_bounds__(64) k_match_pick(MatchDev D) {
    __shared__ PickShared S;
    const int t = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (t >= D.T) return;
    const int pi = D.tomove[t];
    if (pi < 0) return;
    const azc::Pos p = D.poshist[(size_t)t * HMAX + D.plies[t]];
    const MatchPlayerDev pl = D.pl[pi];
    const float* pol = pl.kind == AZ_PLAYER_BASE || pl.kind == AZ_PLAYER_MCTS
                           ? D.pol + ((size_t)pl.row_base + D.row[t]) * AZ_ACTION_SPACE
                           : nullptr;
    int st;
    const int action = arena_pick(S, p, pl.kind, pol, D.u[t], D.actions[t], D.nsm, lane, &st);
    if (lane == 0) {
        D.chosen()[t] = action;
        D.status()[t] = st;
        if (st != ST_OK) atomicOr(&D.io[0], 1);
    }
}

__global__ void __launch_bounds__(64) k_match_commit(MatchDev D) {
    __shared__ Edge s_ed[MAX_EDGES];
    const int t = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (t >= D.T || load_fresh(&D.io[0]) != 0) return;       // all or nothing, across every match
    if (D.tomove[t] < 0) return;
    const int k = D.plies[t];
    int turn;
    const int res = arena_commit(s_ed, D.poshist + (size_t)t * HMAX, D.moves + (size_t)t * HMAX, k, D.chosen()[t], lane,
                                 &turn);
    if (lane == 0) {
        const int m = t / D.G;
        D.plies[t] = k + 1;
        D.result()[t] = res;
        D.tomove[t] = res != azc::ONGOING ? -1 : match_mover(D.pair[m], t - m * D.G, turn);
        if (res == azc::ONGOING) atomicAdd(&D.io[1], 1);
    }
}

// which ABI a handle answers for: how its messages name the call, a player and a game
enum Abi { ABI_ARENA, ABI_TOURNAMENT };

struct MatchEngine {
    Abi abi = ABI_ARENA;
    int device = 0;
    az_arena_cfg cfg{};
    int P = 0, M = 0, G = 0, T = 0;
    std::vector<az_arena_player> pl;
    std::vector<int> pair;              // [M] as MatchDev::pair
    std::vector<az_search*> search;     // [P], MCTS players only
    std::vector<az_player_search> ss;   // [P] an MCTS player's settings in effect (sims, leaves >= 1, c_puct)
    std::vector<SearchRoots> roots;     // [P] where the search's root records live, and its stream
    std::vector<hipEvent_t> done;       // [P] recorded behind the search's readout
    bool device_roots = true;           // AZ_ARENA_DEVICE_ROOTS: k_match_roots, else the host mirror's move lists
    bool overlap = AZ_ARENA_OVERLAP_DEFAULT != 0;   // AZ_ARENA_OVERLAP: a ply's searches side by side
    std::vector<unsigned long long> evals;   // [P] the search's evaluations when it last ran
    std::vector<int> rows_cap;          // [P] rows of the player's part of d_pol (an MCTS player's slots)
    std::vector<float*> d_planes, d_val;
    bool mcts_one_side = false;         // an MCTS player sits on one side of a match: reset refuses lopsided starts
    hipStream_t st = nullptr;
    MatchDev D{};
    azc::Pos* d_pos = nullptr;          // [T] staging: start positions up, current positions down
    float* d_pol = nullptr; float* d_u = nullptr; int* d_act = nullptr; int* d_pair = nullptr;
    std::vector<void*> bufs;
    // host mirror
    uint64_t seed = 0;
    std::vector<azc::Pos> start;        // [G]
    std::vector<std::vector<int32_t>> hist;   // [T]
    std::vector<int> result, turn;
    std::vector<int> io;
    std::vector<float> hu;
    std::vector<int32_t> hact;
    std::vector<azc::Pos> hpos;
    double num_inferences = 0.0, rows = 0.0;
};

namespace {
std::string fn_name(Abi abi, const char* call) {
    return std::string(abi == ABI_ARENA ? "az_arena_" : "az_tournament_") + call + ": ";
}

// the arena's players are 1 and 2, a tournament's count from 0
std::string player_name(Abi abi, int i) { return "player " + std::to_string(abi == ABI_ARENA ? i + 1 : i); }

std::string game_name(const MatchEngine* e, int t) {
    const std::string game = "game " + std::to_string(t % e->G);
    return e->abi == ABI_ARENA ? game : "match " + std::to_string(t / e->G) + " " + game;
}

int player_ok(Abi abi, const char* call, const az_arena_player* p, int i) {
    const std::string fn = fn_name(abi, call), which = player_name(abi, i);
    if (!p) return fail(fn + "null " + which);
    if (p->kind == AZ_PLAYER_EXTERNAL && abi == ABI_TOURNAMENT)
        return fail(fn + which + " is external; a tournament has no such seat");
    if (p->kind < AZ_PLAYER_MCTS || p->kind > AZ_PLAYER_EXTERNAL) return fail(fn + "bad kind of " + which);
    if (p->kind == AZ_PLAYER_BASE && !p->net) return fail(fn + which + " is a base-model player without a net");
    if (p->kind == AZ_PLAYER_MINIMAX && (p->depth < 1 || p->depth > AZ_MINIMAX_MAX_DEPTH))
        return fail(fn + "MiniMax depth of " + which + " outside 1.." + std::to_string(AZ_MINIMAX_MAX_DEPTH));
    if ((p->kind == AZ_PLAYER_BASE || p->kind == AZ_PLAYER_MCTS) && p->net && !p->net->dev)
        return fail(fn + which + " has a dead net");
    return 0;
}

// an MCTS player's own settings, as given (s may be nullptr: all zero)
int search_ok(Abi abi, const char* call, const az_arena_player* p, const az_player_search* s, int i) {
    if (!s) return 0;
    const std::string fn = fn_name(abi, call), which = player_name(abi, i);
    if (s->reserved != 0) return fail(fn + "reserved of " + which + "'s search settings must be 0");
    if (s->sims < 0) return fail(fn + "sims of " + which + " is negative");
    if (s->sims > 60000) return fail(fn + "sims of " + which + " above 60000");
    if (s->leaves < 0 || s->leaves > LEAVES_MAX)
        return fail(fn + "leaves of " + which + " outside 0.." + std::to_string(LEAVES_MAX));
    if (!(s->c_puct >= 0.0f) || s->c_puct > 3.4028234e38f)
        return fail(fn + "c_puct of " + which + " is negative or not finite");
    if (p->kind != AZ_PLAYER_MCTS) {
        const char* field = s->sims ? "sims" : s->leaves ? "leaves" : s->c_puct != 0.0f ? "c_puct" : nullptr;
        if (field) return fail(fn + which + " is not an MCTS player and has search settings (" + field + ")");
    }
    return 0;
}

template <class T> int dmalloc(MatchEngine* e, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(T);
    AZ_HIP(hipMalloc(&q, bytes < 16 ? 16 : bytes));
    e->bufs.push_back(q);
    *p = (T*)q;
    return 0;
}
}  // namespace

int match_destroy(MatchEngine* e) {
    if (!e) return 0;
    (void)hipSetDevice(e->device);
    if (e->st) (void)hipStreamSynchronize(e->st);
    for (az_search* s : e->search) if (s) az_search_destroy(s);
    for (hipEvent_t ev : e->done) if (ev) (void)hipEventDestroy(ev);
    for (void* p : e->bufs) (void)hipFree(p);
    if (e->st) (void)hipStreamDestroy(e->st);
    delete e;
    return 0;
}

int match_reset(MatchEngine* e, const az_pos* start, uint64_t seed) {
    const std::string fn = fn_name(e->abi, "reset");
    const int G = e->G, T = e->T;
    std::vector<azc::Pos> sp(G, azc::startpos());
    for (int g = 0; start && g < G; g++) {
        azc::Pos p = *reinterpret_cast<const azc::Pos*>(start + g);
        if (const char* why = azc::setup_error(p))
            return fail(fn + "start position of game " + std::to_string(g) + " rejected: " + why);
        bool chk;
        const int n = azc::finalize(p, &chk);
        if (azc::outcome(p, n, chk) != azc::ONGOING)
            return fail(fn + "start position of game " + std::to_string(g) + " is already decided");
        sp[g] = p;
    }
    // in every match player 1 moves in `first` games on the even plies and player 2 in the others: an MCTS
    // player's search holds (games + 1) / 2 roots per match unless it plays both sides
    int first = 0;
    for (int g = 0; g < G; g++) first += ((sp[g].turn ^ g) & 1) == 0;
    const int half = (G + 1) / 2;
    if (e->mcts_one_side && (first > half || G - first > half)) {
        const bool arena = e->abi == ABI_ARENA;
        return fail(fn + "with these start positions one player is to move in " +
                    std::to_string(first > G - first ? first : G - first) + " games" + (arena ? "" : " of a match") +
                    " at once; an MCTS player's search holds " + std::to_string(half) + (arena ? "" : " per match"));
    }
    AZ_HIP(hipSetDevice(e->device));
    for (int i = 0; i < e->P; i++) {
        if (!e->search[i]) continue;
        az_search_stats s0;
        if (az_search_stats_get(e->search[i], &s0)) return -1;
        e->evals[i] = (unsigned long long)s0.evals;
    }
    AZ_HIP(hipMemcpyAsync(e->d_pos, sp.data(), (size_t)G * sizeof(azc::Pos), hipMemcpyHostToDevice, e->st));
    k_match_reset<<<(T + 63) / 64, 64, 0, e->st>>>(e->D, e->d_pos);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipStreamSynchronize(e->st));
    e->seed = seed;
    e->start = sp;
    e->hist.assign(T, std::vector<int32_t>());
    e->result.assign(T, azc::ONGOING);
    e->turn.resize(T);
    for (int t = 0; t < T; t++) e->turn[t] = sp[t % G].turn;
    e->num_inferences = e->rows = 0.0;
    return 0;
}

// players [P] and their search settings [P] (nullptr, or entries that may be nullptr: all zero), checked here,
// before the first device call; pair [M] as MatchDev::pair; call: "create" or "create_with", for the messages
int match_create(Abi abi, const char* call, const az_arena_player* const* players,
                 const az_player_search* const* search, int P, const std::vector<int>& pair, const az_arena_cfg* cfg,
                 int device, MatchEngine** out) {
    const std::string fn = fn_name(abi, call);
    bool mcts = false, own = false;
    for (int i = 0; i < P; i++) {
        if (player_ok(abi, call, players[i], i)) return -1;
        if (search && search_ok(abi, call, players[i], search[i], i)) return -1;
        mcts |= players[i]->kind == AZ_PLAYER_MCTS;
        own |= search && search[i];
    }
    if (cfg->games <= 0) return fail(fn + "games must be positive");
    if (mcts && !own && cfg->sims <= 0) return fail(fn + "an MCTS player needs sims > 0");
    if (own && (cfg->sims < 0 || cfg->sims > 60000)) return fail(fn + "cfg->sims outside 0..60000");
    // the settings in effect: a field left 0 is the handle's, or one leaf
    std::vector<az_player_search> ss(P, az_player_search{0, 0, 0.0f, 0});
    for (int i = 0; i < P; i++) {
        if (players[i]->kind != AZ_PLAYER_MCTS) continue;
        const az_player_search* s = search ? search[i] : nullptr;
        ss[i].sims = s && s->sims ? s->sims : cfg->sims;
        ss[i].leaves = s && s->leaves ? s->leaves : 1;
        ss[i].c_puct = s && s->c_puct != 0.0f ? s->c_puct : cfg->c_puct;
        if (ss[i].sims <= 0)
            return fail(fn + "sims of " + player_name(abi, i) + " is 0: neither its own nor cfg->sims is set");
    }
    for (int i = 0; i < P; i++) {
        const az_arena_player& p = *players[i];
        if (p.net && (p.kind == AZ_PLAYER_BASE || p.kind == AZ_PLAYER_MCTS) && p.net->dev->device != device)
            return fail(fn + (abi == ABI_ARENA ? "a player's net" : "the net of " + player_name(abi, i)) +
                        " is on another device");
    }
    AZ_HIP(hipSetDevice(device));
    MatchEngine* e = new MatchEngine();
    e->abi = abi;
    e->device = device;
    e->cfg = *cfg;
    e->P = P;
    const int M = e->M = (int)pair.size();
    const int G = e->G = cfg->games;
    const int T = e->T = M * G;
    for (int i = 0; i < P; i++) e->pl.push_back(*players[i]);
    e->pair = pair;
    e->search.assign(P, nullptr);
    e->ss = ss;
    e->roots.assign(P, SearchRoots{});
    e->done.assign(P, nullptr);
    if (const char* v = getenv("AZ_ARENA_DEVICE_ROOTS")) e->device_roots = atoi(v) != 0;
    if (const char* v = getenv("AZ_ARENA_OVERLAP")) e->overlap = atoi(v) != 0;
    e->evals.assign(P, 0ull);
    e->rows_cap.assign(P, 0);
    e->d_planes.assign(P, nullptr);
    e->d_val.assign(P, nullptr);
    // per match, with caller-given start positions a base-model player can be to move in all G games; an
    // MCTS player's search holds (G + 1) / 2 roots (match_reset refuses more), G when it plays both sides
    for (int pr : pair) {
        const bool both = (pr & 255) == (pr >> 8);
        for (int side = 0; side < (both ? 1 : 2); side++) {
            const int i = side ? pr >> 8 : pr & 255;
            const int k = e->pl[i].kind;
            e->rows_cap[i] += k == AZ_PLAYER_BASE ? G : k == AZ_PLAYER_MCTS ? (both ? G : (G + 1) / 2) : 0;
            e->mcts_one_side |= k == AZ_PLAYER_MCTS && !both;
        }
    }
    auto build = [&]() -> int {
        AZ_HIP(hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking));
        MatchDev& D = e->D;
        D.T = T;
        D.G = G;
        D.nsm = cfg->num_stochastic_moves;
        if (dmalloc(e, &D.poshist, (size_t)T * HMAX) || dmalloc(e, &D.moves, (size_t)T * HMAX) || dmalloc(e, &D.plies, T) ||
            dmalloc(e, &D.tomove, T) || dmalloc(e, &D.row, T) || dmalloc(e, &D.io, 2 + 3 * (size_t)T) ||
            dmalloc(e, &e->d_pos, T) || dmalloc(e, &e->d_u, T) || dmalloc(e, &e->d_act, T) || dmalloc(e, &e->d_pair, M))
            return -1;
        AZ_HIP(hipMemsetAsync(e->d_act, 0xff, (size_t)T * 4, e->st));
        AZ_HIP(hipMemcpy(e->d_pair, pair.data(), (size_t)M * 4, hipMemcpyHostToDevice));
        D.pair = e->d_pair;
        D.u = e->d_u;
        D.actions = e->d_act;
        size_t total = 0;
        for (int i = 0; i < P; i++) {
            D.pl[i].kind = e->pl[i].kind;
            D.pl[i].row_base = (int)total;
            total += (size_t)e->rows_cap[i];
        }
        if (total > 0x7fffffffull) return fail(fn + "too many policy rows");
        if (dmalloc(e, &e->d_pol, total * AZ_ACTION_SPACE)) return -1;
        D.pol = e->d_pol;
        for (int i = 0; i < P; i++) {
            const az_arena_player& p = e->pl[i];
            if (p.kind == AZ_PLAYER_BASE) {
                if (dmalloc(e, &e->d_planes[i], (size_t)e->rows_cap[i] * AZ_PLANES * 64) ||
                    dmalloc(e, &e->d_val[i], (size_t)e->rows_cap[i]))
                    return -1;
            } else if (p.kind == AZ_PLAYER_MCTS) {
                az_search_cfg sc;
                az_search_default_cfg(&sc);
                sc.games = e->rows_cap[i];
                sc.sims = e->ss[i].sims;
                sc.c_puct = e->ss[i].c_puct;
                sc.leaves = e->ss[i].leaves;
                sc.noise = 0;
                sc.seed = cfg->seed;
                sc.evaluator = p.net ? AZ_EVAL_NET : AZ_EVAL_SYNTHETIC;
                sc.continuous = 0;
                sc.record_evals = 0;
                sc.eval_log_cap = 0;
                sc.cache_capacity = 0;
                if (az_search_create(p.net, &sc, device, &e->search[i])) return -1;
                if (search_roots(e->search[i], &e->roots[i])) return -1;
                AZ_HIP(hipEventCreateWithFlags(&e->done[i], hipEventDisableTiming));
            }
        }
        e->io.resize(2 + 3 * (size_t)T);
        return 0;
    };
    if (build() || match_reset(e, nullptr, cfg->seed)) {
        const std::string why = az_last_error();
        match_destroy(e);
        return fail(why);
    }
    *out = e;
    return 0;
}

// one ply of every live game of every match; actions [T] (may be nullptr): the external seats' moves
int match_step(MatchEngine* e, const float* u, const int32_t* actions, int* live) {
    const std::string fn = fn_name(e->abi, "step");
    const int G = e->G, T = e->T, P = e->P;
    MatchDev& D = e->D;
    AZ_HIP(hipSetDevice(e->device));
    // this ply's movers per player, ascending in t, from the host mirror
    std::vector<std::vector<int>> mv(P);
    int nlive = 0;
    for (int t = 0; t < T; t++)
        if (e->result[t] == azc::ONGOING) { mv[match_mover(e->pair[t / G], t % G, e->turn[t])].push_back(t); nlive++; }
    if (nlive == 0) {
        if (live) *live = 0;
        return 0;
    }
    // what can refuse the step on the host is checked before any search is launched
    for (int i = 0; i < P; i++) {
        if (mv[i].empty()) continue;
        if (e->pl[i].kind == AZ_PLAYER_EXTERNAL && !actions)
            return fail(fn + game_name(e, mv[i][0]) + " has an external mover and actions is NULL");
        if (e->pl[i].kind == AZ_PLAYER_MCTS && (int)mv[i].size() > e->rows_cap[i])
            return fail(fn + "more games to move than the MCTS player's search holds");
    }
    std::vector<float>& hu = e->hu;
    hu.assign(T, 0.0f);
    for (int t = 0; t < T; t++) {
        if (u) { hu[t] = u[t]; continue; }
        uint64_t ctr = 0;
        hu[t] = azc::uniform01(azc::stream_key(e->seed, (uint64_t)(t % G), (uint64_t)e->hist[t].size(), 2), ctr);
    }
    double ninf = 0.0, nrows = 0.0;
    AZ_HIP(hipMemsetAsync(D.io, 0, (2 + 2 * (size_t)T) * 4, e->st));
    AZ_HIP(hipMemcpyAsync(e->d_u, hu.data(), (size_t)T * 4, hipMemcpyHostToDevice, e->st));
    std::vector<int32_t>& hact = e->hact;
    hact.assign(T, -1);
    bool given = false, positions = false;
    std::vector<int> launched;                               // the MCTS players searching this ply, in order
    for (int i = 0; i < P; i++) {
        if (mv[i].empty()) continue;
        const az_arena_player& p = e->pl[i];
        if (p.kind == AZ_PLAYER_EXTERNAL) {
            for (int t : mv[i]) hact[t] = actions[t];
            given = true;
        } else if (p.kind == AZ_PLAYER_MINIMAX) {
            if (!positions) {                                // one download serves every MiniMax player
                k_match_positions<<<(T + 63) / 64, 64, 0, e->st>>>(D, e->d_pos);
                AZ_HIP(hipGetLastError());
                e->hpos.resize(T);
                AZ_HIP(hipMemcpyAsync(e->hpos.data(), e->d_pos, (size_t)T * sizeof(azc::Pos), hipMemcpyDeviceToHost, e->st));
                AZ_HIP(hipStreamSynchronize(e->st));
                positions = true;
            }
            const int n = (int)mv[i].size();
            std::vector<azc::Pos> pos(n);
            for (int k = 0; k < n; k++) pos[k] = e->hpos[mv[i][k]];
            std::vector<int32_t> m((size_t)n * AZ_MAX_MOVES), pr((size_t)n * AZ_MAX_MOVES), sc((size_t)n * AZ_MAX_MOVES), nm(n);
            if (az_minimax_scores(e->device, reinterpret_cast<const az_pos*>(pos.data()), n, p.depth, m.data(), pr.data(),
                                  sc.data(), nm.data(), nullptr))
                return -1;
            for (int k = 0; k < n; k++) {
                const int t = mv[i][k];
                const int b = az_minimax_best(sc.data() + (size_t)k * AZ_MAX_MOVES, nm[k], hu[t]);
                hact[t] = b >= 0 ? m[(size_t)k * AZ_MAX_MOVES + b] : -1;
            }
            AZ_HIP(hipSetDevice(e->device));
            given = true;
        } else if (p.kind == AZ_PLAYER_MCTS) {
            // a fresh noiseless tree per move (MCTree::async_init(.., false)); spare slots repeat the player's
            // first root.  Everything goes to the search's own stream; nothing here waits for it
            az_search* s = e->search[i];
            const int S = e->rows_cap[i], n = (int)mv[i].size();
            // two searches on one az_net stay one after the other, in player order
            if (p.net)
                for (int j : launched)
                    if (e->pl[j].net == p.net) AZ_HIP(hipStreamWaitEvent(e->roots[i].st, e->done[j], 0));
            if (e->device_roots) {
                k_match_roots<<<S, 64, 0, e->roots[i].st>>>(D, i, e->roots[i]);
                AZ_HIP(hipGetLastError());
                if (search_set_roots_device(s)) return -1;
            } else {                                         // from the host copy of the move lists
                std::vector<azc::Pos> st(S);
                std::vector<int32_t> flat, off(S + 1, 0), gid(S), nply(S);
                for (int k = 0; k < S; k++) {
                    const int t = mv[i][k < n ? k : 0];
                    st[k] = e->start[t % G];
                    flat.insert(flat.end(), e->hist[t].begin(), e->hist[t].end());
                    off[k + 1] = (int32_t)flat.size();
                    gid[k] = k;
                    nply[k] = (int32_t)e->hist[t].size();
                }
                flat.push_back(0);
                if (az_search_set_roots_from(s, reinterpret_cast<const az_pos*>(st.data()), flat.data(), off.data(),
                                             gid.data(), nply.data(), 0))
                    return -1;
            }
            if (search_launch_device(s, e->d_pol + (size_t)D.pl[i].row_base * AZ_ACTION_SPACE, e->done[i])) return -1;
            launched.push_back(i);
            if (!e->overlap && search_finish_device(s, nullptr)) return -1;   // one after the other
            AZ_HIP(hipSetDevice(e->device));
            // the forwards it launches: the root batch and one per wave of `leaves` simulations
            ninf += (double)((e->ss[i].sims + e->ss[i].leaves - 1) / e->ss[i].leaves) + 1.0;
        }
    }
    // the engine's stream goes on behind every search of the ply
    for (int i : launched) {
        AZ_HIP(hipStreamWaitEvent(e->st, e->done[i], 0));
        k_match_stage<<<T, 64, 0, e->st>>>(D, i, nullptr);   // the games' slot rows
        AZ_HIP(hipGetLastError());
    }
    // one stage launch and one forward per base-model player, over its games to move in all its matches
    for (int i = 0; i < P; i++) {
        if (mv[i].empty() || e->pl[i].kind != AZ_PLAYER_BASE) continue;
        const int n = (int)mv[i].size();
        if (n > e->rows_cap[i]) return fail(fn + "more games to move than a base player's batch holds");
        k_match_stage<<<T, 64, 0, e->st>>>(D, i, e->d_planes[i]);
        AZ_HIP(hipGetLastError());
        if (az_net_forward_device(e->pl[i].net, e->d_planes[i], n, e->d_pol + (size_t)D.pl[i].row_base * AZ_ACTION_SPACE,
                                  e->d_val[i], e->st))
            return -1;
        AZ_HIP(hipSetDevice(e->device));
        ninf += 1.0;
        nrows += (double)n;
    }
    if (given) AZ_HIP(hipMemcpyAsync(e->d_act, hact.data(), (size_t)T * 4, hipMemcpyHostToDevice, e->st));
    k_match_pick<<<T, 64, 0, e->st>>>(D);
    AZ_HIP(hipGetLastError());
    k_match_commit<<<T, 64, 0, e->st>>>(D);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(e->io.data(), D.io, e->io.size() * 4, hipMemcpyDeviceToHost, e->st));
    AZ_HIP(hipStreamSynchronize(e->st));
    for (int i : launched) {                                 // rows: the searches' evaluations
        unsigned long long ev = 0;
        if (search_finish_device(e->search[i], &ev)) return -1;
        nrows += (double)(ev - e->evals[i]);
        e->evals[i] = ev;
    }
    AZ_HIP(hipSetDevice(e->device));
    const int* status = e->io.data() + 2;
    const int* chosen = e->io.data() + 2 + T;
    const int* result = e->io.data() + 2 + 2 * T;
    if (e->io[0]) {                                          // nothing was committed, in any match
        for (int t = 0; t < T; t++) {
            if (status[t] == ST_NONFINITE) return fail(fn + game_name(e, t) + ": the policy has a non-finite legal entry");
            if (status[t] == ST_ILLEGAL)
                return fail(fn + game_name(e, t) + ": index " + std::to_string(chosen[t]) + " is not a legal move");
        }
        return fail(fn + "a move was refused");
    }
    for (int i = 0; i < P; i++)
        for (int t : mv[i]) {
            e->hist[t].push_back(chosen[t]);
            e->turn[t] ^= 1;
            e->result[t] = result[t];
        }
    e->num_inferences += ninf;
    e->rows += nrows;
    if (live) *live = e->io[1];
    return 0;
}

int match_results(MatchEngine* e, int32_t* result, int32_t* plies) {
    AZ_HIP(hipSetDevice(e->device));
    if (result) AZ_HIP(hipMemcpyAsync(result, e->D.result(), (size_t)e->T * 4, hipMemcpyDeviceToHost, e->st));
    if (plies) AZ_HIP(hipMemcpyAsync(plies, e->D.plies, (size_t)e->T * 4, hipMemcpyDeviceToHost, e->st));
    AZ_HIP(hipStreamSynchronize(e->st));
    return 0;
}

// from the host mirror: no device access
int match_live(MatchEngine* e, int32_t* live) {
    int n = 0;
    for (int t = 0; t < e->T; t++) n += live[t] = e->result[t] == azc::ONGOING ? 1 : 0;
    return n;
}

int match_history(MatchEngine* e, int t, int32_t* moves, int cap) {
    AZ_HIP(hipSetDevice(e->device));
    int n = 0;
    AZ_HIP(hipMemcpyAsync(&n, e->D.plies + t, 4, hipMemcpyDeviceToHost, e->st));
    AZ_HIP(hipStreamSynchronize(e->st));
    const int m = n < cap ? n : cap;
    if (moves && m > 0) {
        AZ_HIP(hipMemcpyAsync(moves, e->D.moves + (size_t)t * HMAX, (size_t)m * 4, hipMemcpyDeviceToHost, e->st));
        AZ_HIP(hipStreamSynchronize(e->st));
    }
    return n;
}

int match_stats(MatchEngine* e, double* num_inferences, double* rows) {
    if (num_inferences) *num_inferences = e->num_inferences;
    if (rows) *rows = e->rows;
    return 0;
}

}  // namespace azi

using namespace azi;

// az_arena and az_tournament are the C names of a MatchEngine
static MatchEngine* engine(az_arena* a) { return reinterpret_cast<MatchEngine*>(a); }
static MatchEngine* engine(az_tournament* t) { return reinterpret_cast<MatchEngine*>(t); }

extern "C" {

// ---------------------------------------------------------------- az_arena_*: one match
int az_arena_choose(const float* policy, int fullmoves, int num_stochastic_moves, float u) {
    if (!policy) return fail("az_arena_choose: null policy");
    if (fullmoves > num_stochastic_moves) {                  // Iterator::max_by: the last of equal maxima
        int best = 0;
        for (int i = 1; i < AZ_ACTION_SPACE; i++) if (!(policy[i] < policy[best])) best = i;
        return best;
    }
    float total = 0.0f;                                      // rand 0.8 WeightedIndex: sequential f32 sums
    for (int i = 0; i < AZ_ACTION_SPACE; i++) total = total + policy[i];
    float x = u * total;
    if (!(x < total)) x = nextafterf(total, 0.0f);
    float cw = 0.0f;
    for (int i = 0; i < AZ_ACTION_SPACE - 1; i++) {
        cw = cw + policy[i];
        if (cw > x) return i;
    }
    return AZ_ACTION_SPACE - 1;
}

static int arena_create(const char* call, const az_arena_player* p1, const az_arena_player* p2,
                        const az_player_search* s1, const az_player_search* s2, const az_arena_cfg* cfg, int device,
                        az_arena** out) {
    const std::string fn = std::string("az_arena_") + call + ": ";
    if (!cfg || !out) return fail(fn + "null argument");
    const az_arena_player* players[2] = {p1, p2};
    const az_player_search* search[2] = {s1, s2};
    const bool same = p1 && p1 == p2;                        // one player on both sides: pair (0, 0), else (0, 1)
    if (same && s2 && s2 != s1) {
        const az_player_search zero{0, 0, 0.0f, 0};
        if (memcmp(s2, s1 ? s1 : &zero, sizeof(zero)) != 0)
            return fail(fn + "one player on both sides, and the search settings of player 2 differ from player 1's");
    }
    MatchEngine* e = nullptr;
    if (match_create(ABI_ARENA, call, players, s1 || s2 ? search : nullptr, same ? 1 : 2, {same ? 0 : 1 << 8}, cfg, device,
                     &e))
        return -1;
    *out = reinterpret_cast<az_arena*>(e);
    return 0;
}

int az_arena_create(const az_arena_player* p1, const az_arena_player* p2, const az_arena_cfg* cfg, int device,
                    az_arena** out) {
    return arena_create("create", p1, p2, nullptr, nullptr, cfg, device, out);
}

int az_arena_create_with(const az_arena_player* p1, const az_arena_player* p2, const az_player_search* s1,
                         const az_player_search* s2, const az_arena_cfg* cfg, int device, az_arena** out) {
    return arena_create("create_with", p1, p2, s1, s2, cfg, device, out);
}

int az_arena_destroy(az_arena* a) { return match_destroy(engine(a)); }

int az_arena_reset(az_arena* a, const az_pos* start, uint64_t seed) {
    if (!a) return fail("az_arena_reset: null arena");
    return match_reset(engine(a), start, seed);
}

int az_arena_step(az_arena* a, const float* u, const int32_t* actions, int* live) {
    if (!a) return fail("az_arena_step: null arena");
    return match_step(engine(a), u, actions, live);
}

int az_arena_results(az_arena* a, int32_t* result, int32_t* plies) {
    if (!a) return fail("az_arena_results: null arena");
    return match_results(engine(a), result, plies);
}

int az_arena_live(az_arena* a, int32_t* live) {
    if (!a || !live) return fail("az_arena_live: null argument");
    return match_live(engine(a), live);
}

int az_arena_history(az_arena* a, int game, int32_t* moves, int cap) {
    if (!a) return fail("az_arena_history: null arena");
    if (game < 0 || game >= engine(a)->G) return fail("az_arena_history: no game " + std::to_string(game));
    return match_history(engine(a), game, moves, cap);
}

int az_arena_stats(az_arena* a, double* num_inferences, double* rows) {
    if (!a) return fail("az_arena_stats: null arena");
    return match_stats(engine(a), num_inferences, rows);
}

// ---------------------------------------------------------------- az_tournament_*: a round robin's matches
int az_tournament_matches(int n_players) {
    if (n_players < 2 || n_players > AZ_TOURNAMENT_MAX_PLAYERS)
        return fail("az_tournament_matches: n_players outside 2.." + std::to_string(AZ_TOURNAMENT_MAX_PLAYERS));
    return n_players * (n_players - 1) / 2;
}

int az_tournament_pair(int n_players, int m, int* p1, int* p2) {
    const int M = az_tournament_matches(n_players);
    if (M < 0) return -1;
    if (!p1 || !p2) return fail("az_tournament_pair: null argument");
    if (m < 0 || m >= M) return fail("az_tournament_pair: no match " + std::to_string(m));
    int i = 1;
    while ((i + 1) * i / 2 <= m) i++;
    *p1 = i;
    *p2 = m - i * (i - 1) / 2;
    return 0;
}

static int tournament_create(const char* call, const az_arena_player* players, const az_player_search* search,
                             int n_players, const az_arena_cfg* cfg, int device, az_tournament** out) {
    const std::string fn = std::string("az_tournament_") + call + ": ";
    if (!players || !cfg || !out) return fail(fn + "null argument");
    const int M = az_tournament_matches(n_players);
    if (M < 0) return fail(fn + "n_players outside 2.." + std::to_string(AZ_TOURNAMENT_MAX_PLAYERS));
    std::vector<const az_arena_player*> pp(n_players);
    std::vector<const az_player_search*> sp(n_players);
    for (int i = 0; i < n_players; i++) {
        pp[i] = players + i;
        sp[i] = search ? search + i : nullptr;
    }
    std::vector<int> pair(M);
    for (int m = 0; m < M; m++) {
        int p1, p2;
        az_tournament_pair(n_players, m, &p1, &p2);
        pair[m] = p1 | (p2 << 8);
    }
    MatchEngine* e = nullptr;
    if (match_create(ABI_TOURNAMENT, call, pp.data(), search ? sp.data() : nullptr, n_players, pair, cfg, device, &e))
        return -1;
    *out = reinterpret_cast<az_tournament*>(e);
    return 0;
}

int az_tournament_create(const az_arena_player* players, int n_players, const az_arena_cfg* cfg, int device,
                         az_tournament** out) {
    return tournament_create("create", players, nullptr, n_players, cfg, device, out);
}

int az_tournament_create_with(const az_arena_player* players, const az_player_search* search, int n_players,
                              const az_arena_cfg* cfg, int device, az_tournament** out) {
    return tournament_create("create_with", players, search, n_players, cfg, device, out);
}

int az_tournament_destroy(az_tournament* t) { return match_destroy(engine(t)); }

int az_tournament_reset(az_tournament* t, const az_pos* start, uint64_t seed) {
    if (!t) return fail("az_tournament_reset: null tournament");
    return match_reset(engine(t), start, seed);
}

int az_tournament_step(az_tournament* t, const float* u, int* live) {
    if (!t) return fail("az_tournament_step: null tournament");
    return match_step(engine(t), u, nullptr, live);
}

int az_tournament_results(az_tournament* t, int32_t* result, int32_t* plies) {
    if (!t) return fail("az_tournament_results: null tournament");
    return match_results(engine(t), result, plies);
}

int az_tournament_live(az_tournament* t, int32_t* live) {
    if (!t || !live) return fail("az_tournament_live: null argument");
    return match_live(engine(t), live);
}

int az_tournament_history(az_tournament* t, int match, int game, int32_t* moves, int cap) {
    if (!t) return fail("az_tournament_history: null tournament");
    MatchEngine* e = engine(t);
    if (match < 0 || match >= e->M) return fail("az_tournament_history: no match " + std::to_string(match));
    if (game < 0 || game >= e->G) return fail("az_tournament_history: no game " + std::to_string(game));
    return match_history(e, match * e->G + game, moves, cap);
}

int az_tournament_stats(az_tournament* t, double* num_inferences, double* rows) {
    if (!t) return fail("az_tournament_stats: null tournament");
    return match_stats(engine(t), num_inferences, rows);
}

}  // extern "C"
