// arena.hip -- the evaluation arena (validation.rs:155-402) with its games in HBM (az_arena_*).
//
// evaluate() plays G games in lockstep, player 1 White in the even games and Black in the odd ones.
// Here every game's positions, move list and result live on the device and az_arena_step advances
// all live games by one ply:
//   k_arena_stage   one wavefront per game: a base-model player's games to move are compacted into
//                   batch rows (row = number of lower games with the same mover) and their planes are
//                   written through plane_value (to_tensor, chess.rs:191-245); then the net's forward
//                   (az_net_forward_device) runs on the arena's stream
//   k_arena_pick    one wavefront per game: legal moves (gen_legal_wave), the mover's choice -- the
//                   policy row at the legal indices under validation.rs:297-308 (last maximum, or
//                   WeightedIndex with serial f32 sums on one lane in ascending index order), a
//                   uniform entry of the legal-move list, or a given action -- and its validation
//   k_arena_commit  one wavefront per game, only if every choice was valid: play_move (chess.rs:36-63)
//                   -- play, outcome(), repetition against the game's position history, the 50-move
//                   and 200-fullmove limits -- and the appends to the histories
// The bodies of pick and commit are arena_dev.h's arena_pick and arena_commit, which the tournament arena
// (tournament.hip) calls too.
// The host keeps what the composed players need: an MCTS player's games go through the existing
// az_search (fresh noiseless roots from a host copy of the move lists), a MiniMax player's through
// az_minimax_scores on the downloaded positions; both come back as given actions.
#include <string.h>

#include <string>
#include <vector>

#include "arena_dev.h"

#pragma clang fp contract(off)

namespace azi {

// device state, passed by value.  io is one block the host reads back per step:
// [0] any bad choice, [1] live games after the ply, then status [G], chosen [G], result [G]
struct ArenaDev {
    int G, same, kind0, kind1, nsm;
    azc::Pos* poshist;     // [G][HMAX]: the position after k moves at [k] (the start at [0])
    int* moves;            // [G][HMAX]
    int* plies;            // [G]
    int* tomove;           // [G] player slot (0 / 1) of the mover, -1 once the game is over
    int* row;              // [G] batch row of a base-model mover's game
    int* io;
    const float* u;        // [G]
    const int* actions;    // [G]
    const float* pol0; const float* pol1;   // [rows][4096] of the two player slots
    __device__ __host__ int* status() const { return io + 2; }
    __device__ __host__ int* chosen() const { return io + 2 + G; }
    __device__ __host__ int* result() const { return io + 2 + 2 * G; }
};

__global__ void __launch_bounds__(64) k_arena_reset(ArenaDev A, const azc::Pos* __restrict__ start) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= A.G) return;
    const azc::Pos p = start[g];
    A.poshist[(size_t)g * HMAX] = p;
    A.plies[g] = 0;
    A.tomove[g] = A.same ? 0 : ((p.turn ^ g) & 1);
    A.row[g] = 0;
    A.result()[g] = azc::ONGOING;
}

// current position of every game, for the host-composed players
__global__ void __launch_bounds__(64) k_arena_positions(ArenaDev A, azc::Pos* __restrict__ out) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= A.G) return;
    out[g] = A.poshist[(size_t)g * HMAX + min(A.plies[g], HMAX - 1)];
}

__global__ void __launch_bounds__(64) k_arena_stage(ArenaDev A, int slot, float* __restrict__ planes) {
    // the per-game records were written by vector stores of earlier launches: keep g in a VGPR
    const int g = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (g >= A.G || A.tomove[g] != slot) return;
    int row = 0;
    for (int j0 = 0; j0 < g; j0 += 64) {
        const int j = j0 + lane;
        const bool m = j < g && A.tomove[j] == slot;
        row += __popcll(__ballot(m));
    }
    const azc::Pos p = A.poshist[(size_t)g * HMAX + A.plies[g]];
    if (lane == 0) A.row[g] = row;
    float* out = planes + (size_t)row * AZ_PLANES * 64;
    for (int e = lane; e < AZ_PLANES * 64; e += 64) out[e] = azc::plane_value(p, e >> 6, e & 63);
}

__global__ void __launch_bounds__(64) k_arena_pick(ArenaDev A) {
    __shared__ PickShared S;
    const int g = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (g >= A.G) return;
    const int slot = A.tomove[g];
    if (slot < 0) return;
    const azc::Pos p = A.poshist[(size_t)g * HMAX + A.plies[g]];
    const int kind = slot ? A.kind1 : A.kind0;
    const float* pol = kind == AZ_PLAYER_BASE ? (slot ? A.pol1 : A.pol0) + (size_t)A.row[g] * AZ_ACTION_SPACE : nullptr;
    int st;
    const int action = arena_pick(S, p, kind, pol, A.u[g], A.actions[g], A.nsm, lane, &st);
    if (lane == 0) {
        A.chosen()[g] = action;
        A.status()[g] = st;
        if (st != ST_OK) atomicOr(&A.io[0], 1);
    }
}

__global__ void __launch_bounds__(64) k_arena_commit(ArenaDev A) {
    __shared__ Edge s_ed[MAX_EDGES];
    const int g = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (g >= A.G || load_fresh(&A.io[0]) != 0) return;       // all or nothing
    if (A.tomove[g] < 0) return;
    const int k = A.plies[g];
    int turn;
    const int res = arena_commit(s_ed, A.poshist + (size_t)g * HMAX, A.moves + (size_t)g * HMAX, k, A.chosen()[g], lane,
                                 &turn);
    if (lane == 0) {
        A.plies[g] = k + 1;
        A.result()[g] = res;
        A.tomove[g] = res != azc::ONGOING ? -1 : (A.same ? 0 : ((turn ^ g) & 1));
        if (res == azc::ONGOING) atomicAdd(&A.io[1], 1);
    }
}

static int choose_host(const float* policy, int fullmoves, int nsm, float u) {
    if (fullmoves > nsm) {                                   // Iterator::max_by: the last of equal maxima
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

}  // namespace azi

using namespace azi;

struct az_arena {
    int device = 0;
    az_arena_cfg cfg{};
    az_arena_player pl[2]{};
    bool same = false;
    az_search* search[2] = {nullptr, nullptr};
    int slots = 0;
    hipStream_t st = nullptr;
    ArenaDev A{};
    azc::Pos* d_pos = nullptr;          // [G] staging: start positions up, current positions down
    float* d_u = nullptr; int* d_act = nullptr;
    float* d_planes[2] = {nullptr, nullptr}; float* d_pol[2] = {nullptr, nullptr}; float* d_val[2] = {nullptr, nullptr};
    std::vector<void*> bufs;
    // host mirror (what the composed players and the bookkeeping need)
    uint64_t seed = 0;
    std::vector<azc::Pos> start;
    std::vector<std::vector<int32_t>> hist;
    std::vector<int> result, turn, fullmoves;
    std::vector<int> io;
    std::vector<float> improved, hu;
    std::vector<int32_t> hact;
    double num_inferences = 0.0, rows = 0.0;
};

namespace {
int player_ok(const az_arena_player* p, const char* which) {
    if (!p) return fail(std::string("az_arena_create: null ") + which);
    if (p->kind < AZ_PLAYER_MCTS || p->kind > AZ_PLAYER_EXTERNAL) return fail(std::string("az_arena_create: bad kind of ") + which);
    if (p->kind == AZ_PLAYER_BASE && !p->net) return fail(std::string("az_arena_create: ") + which + " is a base-model player without a net");
    if (p->kind == AZ_PLAYER_MINIMAX && (p->depth < 1 || p->depth > AZ_MINIMAX_MAX_DEPTH))
        return fail(std::string("az_arena_create: MiniMax depth of ") + which + " outside 1.." + std::to_string(AZ_MINIMAX_MAX_DEPTH));
    if ((p->kind == AZ_PLAYER_BASE || p->kind == AZ_PLAYER_MCTS) && p->net && !p->net->dev)
        return fail(std::string("az_arena_create: ") + which + " has a dead net");
    return 0;
}

template <class T> int dmalloc(az_arena* a, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(T);
    AZ_HIP(hipMalloc(&q, bytes < 16 ? 16 : bytes));
    a->bufs.push_back(q);
    *p = (T*)q;
    return 0;
}

inline int slot_of(const az_arena* a, int g) { return a->same ? 0 : ((a->turn[g] ^ g) & 1); }
}  // namespace

extern "C" {

int az_arena_choose(const float* policy, int fullmoves, int num_stochastic_moves, float u) {
    if (!policy) return fail("az_arena_choose: null policy");
    return choose_host(policy, fullmoves, num_stochastic_moves, u);
}

int az_arena_destroy(az_arena* a) {
    if (!a) return 0;
    (void)hipSetDevice(a->device);
    if (a->st) (void)hipStreamSynchronize(a->st);
    for (int k = 0; k < 2; k++) if (a->search[k]) az_search_destroy(a->search[k]);
    for (void* p : a->bufs) (void)hipFree(p);
    if (a->st) (void)hipStreamDestroy(a->st);
    delete a;
    return 0;
}

int az_arena_create(const az_arena_player* p1, const az_arena_player* p2, const az_arena_cfg* cfg, int device,
                    az_arena** out) {
    if (!cfg || !out) return fail("az_arena_create: null argument");
    if (player_ok(p1, "player 1") || player_ok(p2, "player 2")) return -1;
    if (cfg->games <= 0) return fail("az_arena_create: games must be positive");
    const bool mcts = p1->kind == AZ_PLAYER_MCTS || p2->kind == AZ_PLAYER_MCTS;
    if (mcts && cfg->sims <= 0) return fail("az_arena_create: an MCTS player needs sims > 0");
    for (const az_arena_player* p : {p1, p2})
        if (p->net && (p->kind == AZ_PLAYER_BASE || p->kind == AZ_PLAYER_MCTS) && p->net->dev->device != device)
            return fail("az_arena_create: a player's net is on another device");
    AZ_HIP(hipSetDevice(device));
    az_arena* a = new az_arena();
    a->device = device;
    a->cfg = *cfg;
    a->pl[0] = *p1;
    a->pl[1] = *p2;
    a->same = p1 == p2;
    const int G = cfg->games;
    a->slots = a->same ? G : (G + 1) / 2;
    auto build = [&]() -> int {
        AZ_HIP(hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking));
        ArenaDev& A = a->A;
        A.G = G;
        A.same = a->same ? 1 : 0;
        A.kind0 = p1->kind;
        A.kind1 = p2->kind;
        A.nsm = cfg->num_stochastic_moves;
        if (dmalloc(a, &A.poshist, (size_t)G * HMAX) || dmalloc(a, &A.moves, (size_t)G * HMAX) || dmalloc(a, &A.plies, G) ||
            dmalloc(a, &A.tomove, G) || dmalloc(a, &A.row, G) || dmalloc(a, &A.io, 2 + 3 * (size_t)G) ||
            dmalloc(a, &a->d_pos, G) || dmalloc(a, &a->d_u, G) || dmalloc(a, &a->d_act, G))
            return -1;
        A.u = a->d_u;
        A.actions = a->d_act;
        for (int k = 0; k < (a->same ? 1 : 2); k++) {
            const az_arena_player& p = a->pl[k];
            if (p.kind == AZ_PLAYER_BASE) {
                // with caller-given start positions one player can be to move in every game
                if (dmalloc(a, &a->d_planes[k], (size_t)G * AZ_PLANES * 64) ||
                    dmalloc(a, &a->d_pol[k], (size_t)G * AZ_ACTION_SPACE) || dmalloc(a, &a->d_val[k], G))
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
                if (az_search_create(p.net, &sc, device, &a->search[k])) return -1;
            }
        }
        A.pol0 = a->d_pol[0];
        A.pol1 = a->same ? a->d_pol[0] : a->d_pol[1];
        a->improved.resize(mcts ? (size_t)a->slots * AZ_ACTION_SPACE : 0);
        a->io.resize(2 + 3 * (size_t)G);
        return 0;
    };
    if (build() || az_arena_reset(a, nullptr, cfg->seed)) {
        const std::string why = az_last_error();
        az_arena_destroy(a);
        return fail(why);
    }
    *out = a;
    return 0;
}

int az_arena_reset(az_arena* a, const az_pos* start, uint64_t seed) {
    if (!a) return fail("az_arena_reset: null arena");
    const int G = a->A.G;
    std::vector<azc::Pos> sp(G, azc::startpos());
    for (int g = 0; start && g < G; g++) {
        azc::Pos p = *reinterpret_cast<const azc::Pos*>(start + g);
        if (const char* why = azc::setup_error(p))
            return fail("az_arena_reset: start position of game " + std::to_string(g) + " rejected: " + why);
        bool chk;
        const int n = azc::finalize(p, &chk);
        if (azc::outcome(p, n, chk) != azc::ONGOING)
            return fail("az_arena_reset: start position of game " + std::to_string(g) + " is already decided");
        sp[g] = p;
    }
    // player 1 moves in `first` games on the even plies and in the others on the odd ones, player 2 the
    // other way round: an MCTS player's search holds (games + 1) / 2 roots unless it plays both sides
    int first = 0;
    for (int g = 0; g < G; g++) first += ((sp[g].turn ^ g) & 1) == 0;
    const bool mcts = a->pl[0].kind == AZ_PLAYER_MCTS || a->pl[1].kind == AZ_PLAYER_MCTS;
    if (mcts && !a->same && (first > a->slots || G - first > a->slots))
        return fail("az_arena_reset: with these start positions one player is to move in " +
                    std::to_string(first > G - first ? first : G - first) + " games at once; an MCTS player's search holds " +
                    std::to_string(a->slots));
    AZ_HIP(hipSetDevice(a->device));
    AZ_HIP(hipMemcpyAsync(a->d_pos, sp.data(), (size_t)G * sizeof(azc::Pos), hipMemcpyHostToDevice, a->st));
    k_arena_reset<<<(G + 63) / 64, 64, 0, a->st>>>(a->A, a->d_pos);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipStreamSynchronize(a->st));
    a->seed = seed;
    a->start = sp;
    a->hist.assign(G, std::vector<int32_t>());
    a->result.assign(G, azc::ONGOING);
    a->turn.resize(G);
    a->fullmoves.resize(G);
    for (int g = 0; g < G; g++) { a->turn[g] = sp[g].turn; a->fullmoves[g] = sp[g].fullmoves; }
    a->num_inferences = a->rows = 0.0;
    return 0;
}

int az_arena_step(az_arena* a, const float* u, const int32_t* actions, int* live) {
    if (!a) return fail("az_arena_step: null arena");
    const int G = a->A.G;
    ArenaDev& A = a->A;
    AZ_HIP(hipSetDevice(a->device));
    // this ply's movers, from the host mirror
    std::vector<int> mv[2];
    for (int g = 0; g < G; g++)
        if (a->result[g] == azc::ONGOING) mv[slot_of(a, g)].push_back(g);
    if (mv[0].empty() && mv[1].empty()) {
        if (live) *live = 0;
        return 0;
    }
    std::vector<float>& hu = a->hu;
    hu.assign(G, 0.0f);
    for (int g = 0; g < G; g++) {
        if (u) { hu[g] = u[g]; continue; }
        uint64_t ctr = 0;
        hu[g] = azc::uniform01(azc::stream_key(a->seed, (uint64_t)g, (uint64_t)a->hist[g].size(), 2), ctr);
    }
    std::vector<int32_t>& hact = a->hact;
    hact.assign(G, -1);
    bool given = false, positions = false;
    double ninf = 0.0, nrows = 0.0;
    for (int k = 0; k < 2; k++) {
        if (mv[k].empty()) continue;
        const az_arena_player& p = a->pl[k];
        if (p.kind == AZ_PLAYER_EXTERNAL) {
            if (!actions)
                return fail("az_arena_step: game " + std::to_string(mv[k][0]) + " has an external mover and actions is NULL");
            for (int g : mv[k]) hact[g] = actions[g];
            given = true;
        } else if (p.kind == AZ_PLAYER_MINIMAX) {
            if (!positions) {
                k_arena_positions<<<(G + 63) / 64, 64, 0, a->st>>>(A, a->d_pos);
                AZ_HIP(hipGetLastError());
                positions = true;
            }
            std::vector<azc::Pos> all(G);
            AZ_HIP(hipMemcpyAsync(all.data(), a->d_pos, (size_t)G * sizeof(azc::Pos), hipMemcpyDeviceToHost, a->st));
            AZ_HIP(hipStreamSynchronize(a->st));
            const int n = (int)mv[k].size();
            std::vector<azc::Pos> pos(n);
            for (int i = 0; i < n; i++) pos[i] = all[mv[k][i]];
            std::vector<int32_t> m((size_t)n * AZ_MAX_MOVES), pr((size_t)n * AZ_MAX_MOVES), sc((size_t)n * AZ_MAX_MOVES), nm(n);
            if (az_minimax_scores(a->device, reinterpret_cast<const az_pos*>(pos.data()), n, p.depth, m.data(), pr.data(),
                                  sc.data(), nm.data(), nullptr))
                return -1;
            for (int i = 0; i < n; i++) {
                const int g = mv[k][i];
                const int b = az_minimax_best(sc.data() + (size_t)i * AZ_MAX_MOVES, nm[i], hu[g]);
                hact[g] = b >= 0 ? m[(size_t)i * AZ_MAX_MOVES + b] : -1;
            }
            AZ_HIP(hipSetDevice(a->device));
            given = true;
        } else if (p.kind == AZ_PLAYER_MCTS) {
            // a fresh noiseless tree per move (MCTree::async_init(.., false)) through the set-roots path,
            // from the host copy of the move lists; spare slots repeat the first game's root
            az_search* s = a->search[k];
            const int S = a->slots, n = (int)mv[k].size();
            if (n > S) return fail("az_arena_step: more games to move than the MCTS player's search holds");
            std::vector<azc::Pos> st(S);
            std::vector<int32_t> flat, off(S + 1, 0), gid(S), nply(S);
            for (int i = 0; i < S; i++) {
                const int g = mv[k][i < n ? i : 0];
                st[i] = a->start[g];
                flat.insert(flat.end(), a->hist[g].begin(), a->hist[g].end());
                off[i + 1] = (int32_t)flat.size();
                gid[i] = i;
                nply[i] = (int32_t)a->hist[g].size();
            }
            flat.push_back(0);
            az_search_stats s0, s1;
            if (az_search_stats_get(s, &s0)) return -1;
            if (az_search_set_roots_from(s, reinterpret_cast<const az_pos*>(st.data()), flat.data(), off.data(), gid.data(),
                                         nply.data(), 0))
                return -1;
            if (az_search_run(s, a->improved.data(), nullptr, nullptr)) return -1;
            if (az_search_stats_get(s, &s1)) return -1;
            for (int i = 0; i < n; i++) {
                const int g = mv[k][i];
                hact[g] = choose_host(a->improved.data() + (size_t)i * AZ_ACTION_SPACE, a->fullmoves[g],
                                      a->cfg.num_stochastic_moves, hu[g]);
            }
            ninf += (double)a->cfg.sims + 1.0;
            nrows += (double)(s1.evals - s0.evals);
            AZ_HIP(hipSetDevice(a->device));
            given = true;
        }
    }
    AZ_HIP(hipMemsetAsync(A.io, 0, (2 + 2 * (size_t)G) * 4, a->st));
    AZ_HIP(hipMemcpyAsync(a->d_u, hu.data(), (size_t)G * 4, hipMemcpyHostToDevice, a->st));
    if (given) AZ_HIP(hipMemcpyAsync(a->d_act, hact.data(), (size_t)G * 4, hipMemcpyHostToDevice, a->st));
    for (int k = 0; k < 2; k++) {
        if (mv[k].empty() || a->pl[k].kind != AZ_PLAYER_BASE) continue;
        const int n = (int)mv[k].size();
        k_arena_stage<<<G, 64, 0, a->st>>>(A, k, a->d_planes[k]);
        AZ_HIP(hipGetLastError());
        if (az_net_forward_device(a->pl[k].net, a->d_planes[k], n, a->d_pol[k], a->d_val[k], a->st)) return -1;
        AZ_HIP(hipSetDevice(a->device));
        ninf += 1.0;
        nrows += (double)n;
    }
    k_arena_pick<<<G, 64, 0, a->st>>>(A);
    AZ_HIP(hipGetLastError());
    k_arena_commit<<<G, 64, 0, a->st>>>(A);
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipMemcpyAsync(a->io.data(), A.io, a->io.size() * 4, hipMemcpyDeviceToHost, a->st));
    AZ_HIP(hipStreamSynchronize(a->st));
    const int* status = a->io.data() + 2;
    const int* chosen = a->io.data() + 2 + G;
    const int* result = a->io.data() + 2 + 2 * G;
    if (a->io[0]) {                                          // nothing was committed
        for (int g = 0; g < G; g++) {
            if (status[g] == ST_NONFINITE)
                return fail("az_arena_step: game " + std::to_string(g) + ": the policy has a non-finite legal entry");
            if (status[g] == ST_ILLEGAL)
                return fail("az_arena_step: game " + std::to_string(g) + ": index " + std::to_string(chosen[g]) +
                            " is not a legal move");
        }
        return fail("az_arena_step: a move was refused");
    }
    for (int k = 0; k < 2; k++)
        for (int g : mv[k]) {
            a->hist[g].push_back(chosen[g]);
            if (a->turn[g] == 1) a->fullmoves[g]++;
            a->turn[g] ^= 1;
            a->result[g] = result[g];
        }
    a->num_inferences += ninf;
    a->rows += nrows;
    if (live) *live = a->io[1];
    return 0;
}

int az_arena_results(az_arena* a, int32_t* result, int32_t* plies) {
    if (!a) return fail("az_arena_results: null arena");
    const int G = a->A.G;
    AZ_HIP(hipSetDevice(a->device));
    if (result) AZ_HIP(hipMemcpyAsync(result, a->A.result(), (size_t)G * 4, hipMemcpyDeviceToHost, a->st));
    if (plies) AZ_HIP(hipMemcpyAsync(plies, a->A.plies, (size_t)G * 4, hipMemcpyDeviceToHost, a->st));
    AZ_HIP(hipStreamSynchronize(a->st));
    return 0;
}

int az_arena_live(az_arena* a, int32_t* live) {
    if (!a || !live) return fail("az_arena_live: null argument");
    int n = 0;
    for (int g = 0; g < a->A.G; g++) n += live[g] = a->result[g] == azc::ONGOING ? 1 : 0;
    return n;
}

int az_arena_history(az_arena* a, int game, int32_t* moves, int cap) {
    if (!a) return fail("az_arena_history: null arena");
    if (game < 0 || game >= a->A.G) return fail("az_arena_history: no game " + std::to_string(game));
    AZ_HIP(hipSetDevice(a->device));
    int n = 0;
    AZ_HIP(hipMemcpyAsync(&n, a->A.plies + game, 4, hipMemcpyDeviceToHost, a->st));
    AZ_HIP(hipStreamSynchronize(a->st));
    const int m = n < cap ? n : cap;
    if (moves && m > 0) {
        AZ_HIP(hipMemcpyAsync(moves, a->A.moves + (size_t)game * HMAX, (size_t)m * 4, hipMemcpyDeviceToHost, a->st));
        AZ_HIP(hipStreamSynchronize(a->st));
    }
    return n;
}

int az_arena_stats(az_arena* a, double* num_inferences, double* rows) {
    if (!a) return fail("az_arena_stats: null arena");
    if (num_inferences) *num_inferences = a->num_inferences;
    if (rows) *rows = a->rows;
    return 0;
}

}  // extern "C"
