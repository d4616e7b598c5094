// tournament.hip -- a round robin's pairings (ratings.rs:10-24) in one device handle (az_tournament_*).
//
// compute_elo_rankings plays evaluate(&players[i], &players[j]) for every j < i.  Here all those matches
// advance in lockstep: tournament game t = m * G + g is game g of match m, and az_tournament_step plays one
// ply of every live game of every match:
//   k_tour_stage    one wavefront per game: the games in which one player is to move, across all of its
//                   matches, are compacted into rows 0..n-1 (ascending in t); a base-model player's rows get
//                   their planes (plane_value) and ONE forward of n rows follows on the tournament's stream;
//                   an MCTS player's rows are the slots of its one search, whose improved policy
//                   (search_run_device) stays in device memory
//   k_tour_pick     one wavefront per game: arena_pick (arena_dev.h) -- the arena's legal moves, choice rule
//                   and validation, with an MCTS mover's slot row read exactly as a base mover's policy row
//   k_tour_commit   one wavefront per game, only if every choice of every match was valid: arena_commit
// The host keeps what az_arena keeps: the move lists an MCTS player's roots are set from
// (az_search_set_roots_from) and a MiniMax player's az_minimax_scores call on the downloaded positions.
#include <string.h>

#include <string>
#include <vector>

#include "arena_dev.h"

#pragma clang fp contract(off)

namespace azi {

struct TourPlayerDev {
    int kind;
    int row_base;          // the player's first row of pol
    const float* pol;      // [rows][4096]: policy rows (base model) or improved-policy rows (MCTS) of all players
};

// device state, passed by value.  io is one block the host reads back per step:
// [0] any bad choice, [1] live games after the ply, then status [T], chosen [T], result [T]
struct TourDev {
    int T, G, nsm, pad;
    azc::Pos* poshist;     // [T][HMAX]: the position after k moves at [k] (the start at [0])
    int* moves;            // [T][HMAX]
    int* plies;            // [T]
    int* tomove;           // [T] player index of the mover, -1 once the game is over
    int* row;              // [T] row of the game among its mover's games to move
    int* io;
    const int* pair;       // [matches] player 1 | player 2 << 8
    const float* u;        // [T]
    const int* actions;    // [T]
    TourPlayerDev pl[AZ_TOURNAMENT_MAX_PLAYERS];
    __device__ __host__ int* status() const { return io + 2; }
    __device__ __host__ int* chosen() const { return io + 2 + T; }
    __device__ __host__ int* result() const { return io + 2 + 2 * T; }
};

// player 1 of the match is White in its even games (az_arena's rule)
__device__ __forceinline__ int tour_mover(const TourDev& D, int t, int turn) {
    const int m = t / D.G, g = t - m * D.G;
    const int pr = D.pair[m];
    return ((turn ^ g) & 1) ? (pr >> 8) : (pr & 255);
}

__global__ void __launch_bounds__(64) k_tour_reset(TourDev D, const azc::Pos* __restrict__ start) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= D.T) return;
    const azc::Pos p = start[t % D.G];
    D.poshist[(size_t)t * HMAX] = p;
    D.plies[t] = 0;
    D.tomove[t] = tour_mover(D, t, p.turn);
    D.row[t] = 0;
    D.result()[t] = azc::ONGOING;
}

// current position of every game, for the MiniMax players
__global__ void __launch_bounds__(64) k_tour_positions(TourDev D, azc::Pos* __restrict__ out) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= D.T) return;
    out[t] = D.poshist[(size_t)t * HMAX + min(D.plies[t], HMAX - 1)];
}

// planes == nullptr (an MCTS player): the rows only
__global__ void __launch_bounds__(64) k_tour_stage(TourDev D, int player, float* __restrict__ planes) {
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

__global__ void __launch_bounds__(64) k_tour_pick(TourDev D) {
    __shared__ PickShared S;
    const int t = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (t >= D.T) return;
    const int pi = D.tomove[t];
    if (pi < 0) return;
    const azc::Pos p = D.poshist[(size_t)t * HMAX + D.plies[t]];
    const TourPlayerDev pl = D.pl[pi];
    const float* pol = pl.kind == AZ_PLAYER_BASE || pl.kind == AZ_PLAYER_MCTS
                           ? pl.pol + ((size_t)pl.row_base + D.row[t]) * AZ_ACTION_SPACE
                           : nullptr;
    int st;
    const int action = arena_pick(S, p, pl.kind, pol, D.u[t], D.actions[t], D.nsm, lane, &st);
    if (lane == 0) {
        D.chosen()[t] = action;
        D.status()[t] = st;
        if (st != ST_OK) atomicOr(&D.io[0], 1);
    }
}

__global__ void __launch_bounds__(64) k_tour_commit(TourDev D) {
    __shared__ Edge s_ed[MAX_EDGES];
    const int t = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (t >= D.T || load_fresh(&D.io[0]) != 0) return;       // all or nothing, across every match
    if (D.tomove[t] < 0) return;
    const int k = D.plies[t];
    int turn;
    const int res = arena_commit(s_ed, D.poshist + (size_t)t * HMAX, D.moves + (size_t)t * HMAX, k, D.chosen()[t], lane,
                                 &turn);
    if (lane == 0) {
        D.plies[t] = k + 1;
        D.result()[t] = res;
        D.tomove[t] = res != azc::ONGOING ? -1 : tour_mover(D, t, turn);
        if (res == azc::ONGOING) atomicAdd(&D.io[1], 1);
    }
}

}  // namespace azi

using namespace azi;

struct az_tournament {
    int device = 0;
    az_arena_cfg cfg{};
    int P = 0, M = 0, G = 0, T = 0;
    std::vector<az_arena_player> pl;
    std::vector<int> p1, p2;            // [M]
    std::vector<az_search*> search;     // [P], MCTS players only
    std::vector<unsigned long long> evals;   // [P] the search's evaluations when it last ran
    std::vector<int> rows_cap;          // [P] rows of the player's part of d_pol
    std::vector<float*> d_planes, d_val;
    int slots = 0;
    bool mcts = false;
    hipStream_t st = nullptr;
    TourDev D{};
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
int tour_player_ok(const az_arena_player* p, int i) {
    const std::string which = "player " + std::to_string(i);
    if (p->kind == AZ_PLAYER_EXTERNAL) return fail("az_tournament_create: " + which + " is external; a tournament has no such seat");
    if (p->kind < AZ_PLAYER_MCTS || p->kind > AZ_PLAYER_RANDOM) return fail("az_tournament_create: bad kind of " + which);
    if (p->kind == AZ_PLAYER_BASE && !p->net) return fail("az_tournament_create: " + which + " is a base-model player without a net");
    if (p->kind == AZ_PLAYER_MINIMAX && (p->depth < 1 || p->depth > AZ_MINIMAX_MAX_DEPTH))
        return fail("az_tournament_create: MiniMax depth of " + which + " outside 1.." + std::to_string(AZ_MINIMAX_MAX_DEPTH));
    if ((p->kind == AZ_PLAYER_BASE || p->kind == AZ_PLAYER_MCTS) && p->net && !p->net->dev)
        return fail("az_tournament_create: " + which + " has a dead net");
    return 0;
}

template <class T> int dmalloc(az_tournament* a, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(T);
    AZ_HIP(hipMalloc(&q, bytes < 16 ? 16 : bytes));
    a->bufs.push_back(q);
    *p = (T*)q;
    return 0;
}

inline int mover_of(const az_tournament* a, int t) {
    const int m = t / a->G, g = t - m * a->G;
    return ((a->turn[t] ^ g) & 1) ? a->p2[m] : a->p1[m];
}

inline std::string game_name(const az_tournament* a, int t) {
    return "match " + std::to_string(t / a->G) + " game " + std::to_string(t % a->G);
}
}  // namespace

extern "C" {

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

int az_tournament_destroy(az_tournament* a) {
    if (!a) return 0;
    (void)hipSetDevice(a->device);
    if (a->st) (void)hipStreamSynchronize(a->st);
    for (az_search* s : a->search) if (s) az_search_destroy(s);
    for (void* p : a->bufs) (void)hipFree(p);
    if (a->st) (void)hipStreamDestroy(a->st);
    delete a;
    return 0;
}

int az_tournament_create(const az_arena_player* players, int n_players, const az_arena_cfg* cfg, int device,
                         az_tournament** out) {
    if (!players || !cfg || !out) return fail("az_tournament_create: null argument");
    const int M = az_tournament_matches(n_players);
    if (M < 0) return fail("az_tournament_create: n_players outside 2.." + std::to_string(AZ_TOURNAMENT_MAX_PLAYERS));
    const int P = n_players;
    bool mcts = false;
    for (int i = 0; i < P; i++) {
        if (tour_player_ok(players + i, i)) return -1;
        mcts |= players[i].kind == AZ_PLAYER_MCTS;
    }
    if (cfg->games <= 0) return fail("az_tournament_create: games must be positive");
    if (mcts && cfg->sims <= 0) return fail("az_tournament_create: an MCTS player needs sims > 0");
    for (int i = 0; i < P; i++) {
        const az_arena_player& p = players[i];
        if (p.net && (p.kind == AZ_PLAYER_BASE || p.kind == AZ_PLAYER_MCTS) && p.net->dev->device != device)
            return fail("az_tournament_create: the net of player " + std::to_string(i) + " is on another device");
    }
    AZ_HIP(hipSetDevice(device));
    az_tournament* a = new az_tournament();
    a->device = device;
    a->cfg = *cfg;
    a->P = P;
    a->M = M;
    const int G = a->G = cfg->games;
    const int T = a->T = M * G;
    a->pl.assign(players, players + P);
    a->p1.resize(M);
    a->p2.resize(M);
    for (int m = 0; m < M; m++) az_tournament_pair(P, m, &a->p1[m], &a->p2[m]);
    a->slots = (P - 1) * ((G + 1) / 2);
    a->mcts = mcts;
    a->search.assign(P, nullptr);
    a->evals.assign(P, 0ull);
    a->rows_cap.assign(P, 0);
    a->d_planes.assign(P, nullptr);
    a->d_val.assign(P, nullptr);
    auto build = [&]() -> int {
        AZ_HIP(hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking));
        TourDev& D = a->D;
        D.T = T;
        D.G = G;
        D.nsm = cfg->num_stochastic_moves;
        if (dmalloc(a, &D.poshist, (size_t)T * HMAX) || dmalloc(a, &D.moves, (size_t)T * HMAX) || dmalloc(a, &D.plies, T) ||
            dmalloc(a, &D.tomove, T) || dmalloc(a, &D.row, T) || dmalloc(a, &D.io, 2 + 3 * (size_t)T) ||
            dmalloc(a, &a->d_pos, T) || dmalloc(a, &a->d_u, T) || dmalloc(a, &a->d_act, T) || dmalloc(a, &a->d_pair, M))
            return -1;
        AZ_HIP(hipMemsetAsync(a->d_act, 0xff, (size_t)T * 4, a->st));
        std::vector<int> pair(M);
        for (int m = 0; m < M; m++) pair[m] = a->p1[m] | (a->p2[m] << 8);
        AZ_HIP(hipMemcpy(a->d_pair, pair.data(), (size_t)M * 4, hipMemcpyHostToDevice));
        D.pair = a->d_pair;
        D.u = a->d_u;
        D.actions = a->d_act;
        // with caller-given start positions a base-model player can be to move in every game of its
        // P - 1 matches; an MCTS player's search holds `slots` roots (az_tournament_reset refuses more)
        size_t total = 0;
        for (int i = 0; i < P; i++) {
            const int k = a->pl[i].kind;
            a->rows_cap[i] = k == AZ_PLAYER_BASE ? (P - 1) * G : k == AZ_PLAYER_MCTS ? a->slots : 0;
            D.pl[i].kind = k;
            D.pl[i].row_base = (int)total;
            total += (size_t)a->rows_cap[i];
        }
        if (total > 0x7fffffffull) return fail("az_tournament_create: too many policy rows");
        if (dmalloc(a, &a->d_pol, total * AZ_ACTION_SPACE)) return -1;
        for (int i = 0; i < P; i++) {
            const az_arena_player& p = a->pl[i];
            D.pl[i].pol = a->d_pol;
            if (p.kind == AZ_PLAYER_BASE) {
                if (dmalloc(a, &a->d_planes[i], (size_t)a->rows_cap[i] * AZ_PLANES * 64) ||
                    dmalloc(a, &a->d_val[i], (size_t)a->rows_cap[i]))
                    return -1;
            } else if (p.kind == AZ_PLAYER_MCTS) {
                az_search_cfg sc;
                az_search_default_cfg(&sc);
                sc.games = a->slots;
                sc.sims = cfg->sims;
                sc.c_puct = cfg->c_puct;
                sc.noise = 0;
                sc.seed = cfg->seed;
                sc.evaluator = p.net ? AZ_EVAL_NET : AZ_EVAL_SYNTHETIC;
                sc.continuous = 0;
                sc.record_evals = 0;
                sc.eval_log_cap = 0;
                sc.cache_capacity = 0;
                if (az_search_create(p.net, &sc, device, &a->search[i])) return -1;
            }
        }
        a->io.resize(2 + 3 * (size_t)T);
        return 0;
    };
    if (build() || az_tournament_reset(a, nullptr, cfg->seed)) {
        const std::string why = az_last_error();
        az_tournament_destroy(a);
        return fail(why);
    }
    *out = a;
    return 0;
}

int az_tournament_reset(az_tournament* a, const az_pos* start, uint64_t seed) {
    if (!a) return fail("az_tournament_reset: null tournament");
    const int G = a->G, T = a->T;
    std::vector<azc::Pos> sp(G, azc::startpos());
    for (int g = 0; start && g < G; g++) {
        azc::Pos p = *reinterpret_cast<const azc::Pos*>(start + g);
        if (const char* why = azc::setup_error(p))
            return fail("az_tournament_reset: start position of game " + std::to_string(g) + " rejected: " + why);
        bool chk;
        const int n = azc::finalize(p, &chk);
        if (azc::outcome(p, n, chk) != azc::ONGOING)
            return fail("az_tournament_reset: start position of game " + std::to_string(g) + " is already decided");
        sp[g] = p;
    }
    // in every match player 1 moves in `first` games on the even plies and player 2 in the others: an MCTS
    // player's search holds (games + 1) / 2 roots per match (the refusal az_arena_reset makes)
    int first = 0;
    for (int g = 0; g < G; g++) first += ((sp[g].turn ^ g) & 1) == 0;
    const int half = (G + 1) / 2;
    if (a->mcts && (first > half || G - first > half))
        return fail("az_tournament_reset: with these start positions one player is to move in " +
                    std::to_string(first > G - first ? first : G - first) +
                    " games of a match at once; an MCTS player's search holds " + std::to_string(half) + " per match");
    AZ_HIP(hipSetDevice(a->device));
    for (int i = 0; i < a->P; i++) {
        if (!a->search[i]) continue;
        az_search_stats s0;
        if (az_search_stats_get(a->search[i], &s0)) return -1;
        a->evals[i] = (unsigned long long)s0.evals;
    }
    AZ_HIP(hipMemcpyAsync(a->d_pos, sp.data(), (size_t)G * sizeof(azc::Pos), hipMemcpyHostToDevice, a->st));
    k_tour_reset<<<(T + 63) / 64, 64, 0, a->st>>>(a->D, a->d_pos);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipStreamSynchronize(a->st));
    a->seed = seed;
    a->start = sp;
    a->hist.assign(T, std::vector<int32_t>());
    a->result.assign(T, azc::ONGOING);
    a->turn.resize(T);
    for (int t = 0; t < T; t++) a->turn[t] = sp[t % G].turn;
    a->num_inferences = a->rows = 0.0;
    return 0;
}

int az_tournament_step(az_tournament* a, const float* u, int* live) {
    if (!a) return fail("az_tournament_step: null tournament");
    const int G = a->G, T = a->T, P = a->P;
    TourDev& D = a->D;
    AZ_HIP(hipSetDevice(a->device));
    // this ply's movers per player, ascending in t, from the host mirror
    std::vector<std::vector<int>> mv(P);
    int nlive = 0;
    for (int t = 0; t < T; t++)
        if (a->result[t] == azc::ONGOING) { mv[mover_of(a, t)].push_back(t); nlive++; }
    if (nlive == 0) {
        if (live) *live = 0;
        return 0;
    }
    std::vector<float>& hu = a->hu;
    hu.assign(T, 0.0f);
    for (int t = 0; t < T; t++) {
        if (u) { hu[t] = u[t]; continue; }
        uint64_t ctr = 0;
        hu[t] = azc::uniform01(azc::stream_key(a->seed, (uint64_t)(t % G), (uint64_t)a->hist[t].size(), 2), ctr);
    }
    double ninf = 0.0, nrows = 0.0;
    AZ_HIP(hipMemsetAsync(D.io, 0, (2 + 2 * (size_t)T) * 4, a->st));
    AZ_HIP(hipMemcpyAsync(a->d_u, hu.data(), (size_t)T * 4, hipMemcpyHostToDevice, a->st));
    std::vector<int32_t>& hact = a->hact;
    bool given = false, positions = false;
    for (int i = 0; i < P; i++) {
        if (mv[i].empty()) continue;
        const az_arena_player& p = a->pl[i];
        if (p.kind == AZ_PLAYER_MINIMAX) {
            if (!positions) {                                // one download serves every MiniMax player
                k_tour_positions<<<(T + 63) / 64, 64, 0, a->st>>>(D, a->d_pos);
                AZ_HIP(hipGetLastError());
                a->hpos.resize(T);
                AZ_HIP(hipMemcpyAsync(a->hpos.data(), a->d_pos, (size_t)T * sizeof(azc::Pos), hipMemcpyDeviceToHost, a->st));
                AZ_HIP(hipStreamSynchronize(a->st));
                positions = true;
            }
            if (!given) hact.assign(T, -1);
            const int n = (int)mv[i].size();
            std::vector<azc::Pos> pos(n);
            for (int k = 0; k < n; k++) pos[k] = a->hpos[mv[i][k]];
            std::vector<int32_t> m((size_t)n * AZ_MAX_MOVES), pr((size_t)n * AZ_MAX_MOVES), sc((size_t)n * AZ_MAX_MOVES), nm(n);
            if (az_minimax_scores(a->device, reinterpret_cast<const az_pos*>(pos.data()), n, p.depth, m.data(), pr.data(),
                                  sc.data(), nm.data(), nullptr))
                return -1;
            for (int k = 0; k < n; k++) {
                const int t = mv[i][k];
                const int b = az_minimax_best(sc.data() + (size_t)k * AZ_MAX_MOVES, nm[k], hu[t]);
                hact[t] = b >= 0 ? m[(size_t)k * AZ_MAX_MOVES + b] : -1;
            }
            AZ_HIP(hipSetDevice(a->device));
            given = true;
        } else if (p.kind == AZ_PLAYER_MCTS) {
            // a fresh noiseless tree per move (MCTree::async_init(.., false)) through the set-roots path,
            // from the host copy of the move lists; spare slots repeat the player's first root
            az_search* s = a->search[i];
            const int S = a->slots, n = (int)mv[i].size();
            if (n > S) return fail("az_tournament_step: more games to move than the MCTS player's search holds");
            std::vector<azc::Pos> st(S);
            std::vector<int32_t> flat, off(S + 1, 0), gid(S), nply(S);
            for (int k = 0; k < S; k++) {
                const int t = mv[i][k < n ? k : 0];
                st[k] = a->start[t % G];
                flat.insert(flat.end(), a->hist[t].begin(), a->hist[t].end());
                off[k + 1] = (int32_t)flat.size();
                gid[k] = k;
                nply[k] = (int32_t)a->hist[t].size();
            }
            flat.push_back(0);
            if (az_search_set_roots_from(s, reinterpret_cast<const az_pos*>(st.data()), flat.data(), off.data(), gid.data(),
                                         nply.data(), 0))
                return -1;
            unsigned long long ev = 0;
            if (search_run_device(s, a->d_pol + (size_t)D.pl[i].row_base * AZ_ACTION_SPACE, &ev)) return -1;
            AZ_HIP(hipSetDevice(a->device));
            ninf += (double)a->cfg.sims + 1.0;
            nrows += (double)(ev - a->evals[i]);
            a->evals[i] = ev;
            k_tour_stage<<<T, 64, 0, a->st>>>(D, i, nullptr);   // the games' slot rows
            AZ_HIP(hipGetLastError());
        }
    }
    // one stage launch and one forward per base-model player, over its games to move in all its matches
    for (int i = 0; i < P; i++) {
        if (mv[i].empty() || a->pl[i].kind != AZ_PLAYER_BASE) continue;
        const int n = (int)mv[i].size();
        if (n > a->rows_cap[i]) return fail("az_tournament_step: more games to move than a base player's batch holds");
        k_tour_stage<<<T, 64, 0, a->st>>>(D, i, a->d_planes[i]);
        AZ_HIP(hipGetLastError());
        if (az_net_forward_device(a->pl[i].net, a->d_planes[i], n, a->d_pol + (size_t)D.pl[i].row_base * AZ_ACTION_SPACE,
                                  a->d_val[i], a->st))
            return -1;
        AZ_HIP(hipSetDevice(a->device));
        ninf += 1.0;
        nrows += (double)n;
    }
    if (given) AZ_HIP(hipMemcpyAsync(a->d_act, hact.data(), (size_t)T * 4, hipMemcpyHostToDevice, a->st));
    k_tour_pick<<<T, 64, 0, a->st>>>(D);
    AZ_HIP(hipGetLastError());
    k_tour_commit<<<T, 64, 0, a->st>>>(D);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(a->io.data(), D.io, a->io.size() * 4, hipMemcpyDeviceToHost, a->st));
    AZ_HIP(hipStreamSynchronize(a->st));
    const int* status = a->io.data() + 2;
    const int* chosen = a->io.data() + 2 + T;
    const int* result = a->io.data() + 2 + 2 * T;
    if (a->io[0]) {                                          // nothing was committed, in any match
        for (int t = 0; t < T; t++) {
            if (status[t] == ST_NONFINITE)
                return fail("az_tournament_step: " + game_name(a, t) + ": the policy has a non-finite legal entry");
            if (status[t] == ST_ILLEGAL)
                return fail("az_tournament_step: " + game_name(a, t) + ": index " + std::to_string(chosen[t]) +
                            " is not a legal move");
        }
        return fail("az_tournament_step: a move was refused");
    }
    for (int i = 0; i < P; i++)
        for (int t : mv[i]) {
            a->hist[t].push_back(chosen[t]);
            a->turn[t] ^= 1;
            a->result[t] = result[t];
        }
    a->num_inferences += ninf;
    a->rows += nrows;
    if (live) *live = a->io[1];
    return 0;
}

int az_tournament_results(az_tournament* a, int32_t* result, int32_t* plies) {
    if (!a) return fail("az_tournament_results: null tournament");
    const int T = a->T;
    AZ_HIP(hipSetDevice(a->device));
    if (result) AZ_HIP(hipMemcpyAsync(result, a->D.result(), (size_t)T * 4, hipMemcpyDeviceToHost, a->st));
    if (plies) AZ_HIP(hipMemcpyAsync(plies, a->D.plies, (size_t)T * 4, hipMemcpyDeviceToHost, a->st));
    AZ_HIP(hipStreamSynchronize(a->st));
    return 0;
}

int az_tournament_live(az_tournament* a, int32_t* live) {
    if (!a || !live) return fail("az_tournament_live: null argument");
    int n = 0;
    for (int t = 0; t < a->T; t++) n += live[t] = a->result[t] == azc::ONGOING ? 1 : 0;
    return n;
}

int az_tournament_history(az_tournament* a, int match, int game, int32_t* moves, int cap) {
    if (!a) return fail("az_tournament_history: null tournament");
    if (match < 0 || match >= a->M) return fail("az_tournament_history: no match " + std::to_string(match));
    if (game < 0 || game >= a->G) return fail("az_tournament_history: no game " + std::to_string(game));
    const int t = match * a->G + game;
    AZ_HIP(hipSetDevice(a->device));
    int n = 0;
    AZ_HIP(hipMemcpyAsync(&n, a->D.plies + t, 4, hipMemcpyDeviceToHost, a->st));
    AZ_HIP(hipStreamSynchronize(a->st));
    const int m = n < cap ? n : cap;
    if (moves && m > 0) {
        AZ_HIP(hipMemcpyAsync(moves, a->D.moves + (size_t)t * HMAX, (size_t)m * 4, hipMemcpyDeviceToHost, a->st));
        AZ_HIP(hipStreamSynchronize(a->st));
    }
    return n;
}

int az_tournament_stats(az_tournament* a, double* num_inferences, double* rows) {
    if (!a) return fail("az_tournament_stats: null tournament");
    if (num_inferences) *num_inferences = a->num_inferences;
    if (rows) *rows = a->rows;
    return 0;
}

}  // extern "C"
