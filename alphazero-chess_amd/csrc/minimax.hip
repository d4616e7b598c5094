// minimax.hip -- the arena's MiniMax(n) opponent (chess.rs:248-322): get_best_move's scoring of
// every root move by a full-width negamax over material, for a batch of positions at once.
//
//   az_minimax_scores(device >= 0): the GPU path.  The tree is materialised level by level into a
//     node buffer of bounded size (one wavefront per node: gen_legal_wave, the four promotion roles
//     as separate entries, one child position per lane); below the deepest level that fits, one
//     wavefront per frontier node searches the remaining depth depth-first on an explicit stack in
//     LDS and gives every lane one leaf on the last ply; one backup kernel per materialised level
//     takes max(-child) and sums the call counts.  Levels are kernel launches on one stream.
//   az_minimax_scores(AZ_DEVICE_HOST): the same definition as a recursive negamax over chess.h,
//     threaded over (position, root move); the CPU fallback and the parity reference of the kernels.
//   az_minimax_best: best_moves.choose with a caller-given uniform.
// Everything is integer arithmetic: the two paths agree bit for bit, whatever the buffer size.
#include <limits.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "az_internal.h"
#include "search_dev.h"

namespace azi {

constexpr int MM_MATE = 20000;                              // MATE_SCORE, chess.rs:253
constexpr int MM_STACK = AZ_MINIMAX_MAX_DEPTH - 1;          // plies below a level-1 node that still expand
constexpr long long MM_FRONTIER_DEFAULT = 1ll << 20;        // nodes (about 100 MB of records)
constexpr long long MM_FRONTIER_MIN = AZ_MAX_MOVES, MM_FRONTIER_MAX = 1ll << 24;

// evaluate_material (chess.rs:255-266): side to move minus the other side, kings 0
__host__ __device__ __forceinline__ int mm_material(const azc::Pos& p) {
    using namespace azc;
    const uint64_t us = side_bb(p, p.turn), th = side_bb(p, p.turn ^ 1);
    return 100 * (popc64(p.bb[PAWN] & us) - popc64(p.bb[PAWN] & th)) +
           320 * (popc64(p.bb[KNIGHT] & us) - popc64(p.bb[KNIGHT] & th)) +
           330 * (popc64(p.bb[BISHOP] & us) - popc64(p.bb[BISHOP] & th)) +
           500 * (popc64(p.bb[ROOK] & us) - popc64(p.bb[ROOK] & th)) +
           900 * (popc64(p.bb[QUEEN] & us) - popc64(p.bb[QUEEN] & th));
}
// negamax(pos, 0) (chess.rs:269-281): mate -20000, stalemate / insufficient material 0, else material
__host__ __device__ __forceinline__ int mm_static(const azc::Pos& p) {
    azc::NullSink ns;
    bool chk, lep;
    const int n = azc::gen_legal(p, ns, &chk, &lep);
    if (n == 0) return chk ? -MM_MATE : 0;
    if (azc::insufficient_material(p)) return 0;
    return mm_material(p);
}
// an entry of legal_moves(): move index | promoted role << 12 (0: no promotion; 1 N, 2 B, 3 R, 4 Q)
__host__ __device__ __forceinline__ azc::Pos mm_play(const azc::Pos& p, int ent) {
    const int role = ent >> 12;
    return azc::play_index(p, ent & azc::IDX_MASK, role ? role : (int)azc::QUEEN);
}

// ------------------------------------------------------------------ device
__device__ __forceinline__ int wave_max_i32(int v) {
    v = max(v, dpp_i32<0xB1>(v, v));
    v = max(v, dpp_i32<0x4E>(v, v));
    v = max(v, dpp_i32<0x141>(v, v));
    v = max(v, dpp_i32<0x140>(v, v));
    v = max(v, dpp_i32<0x142, 0xA>(v, v));
    v = max(v, dpp_i32<0x143, 0xC>(v, v));
    return __builtin_amdgcn_readlane(v, 63);
}

// The entry list of p with the lanes of one wavefront (a workgroup of 64): gen_legal_wave's distinct
// indices into `ed`, then every PROMO_FLAG edge as its four roles Q, R, B, N (shakmaty's order) at
// positions from a wave prefix sum.  Returns the entry count (wave-uniform); more than AZ_MAX_MOVES
// entries are flagged in *err, never written.
__device__ __forceinline__ int mm_gen(const azc::Pos& p, Edge* ed, uint16_t* ent, int lane, bool* chk, int* err) {
    bool lep;
    const int ne = gen_legal_wave<1>(p, ed, lane, chk, &lep);
    __syncthreads();
    int total = 0;
    for (int base = 0; base < ne; base += 64) {
        const int i = base + lane;
        const int idx = i < ne ? (int)ed[i].idx : 0;
        const int reps = i < ne ? ((idx & azc::PROMO_FLAG) ? 4 : 1) : 0;
        int sum;
        const int o = total + wave_excl_small(reps, &sum);
        const int mv = idx & azc::IDX_MASK;
        if (reps == 1) {
            if (o < AZ_MAX_MOVES) ent[o] = (uint16_t)mv;
        } else if (reps == 4) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (o + r < AZ_MAX_MOVES) ent[o + r] = (uint16_t)(mv | ((azc::QUEEN - r) << 12));
        }
        total += sum;
    }
    if (total > AZ_MAX_MOVES) {
        if (lane == 0) atomicExch(err, 1);
        total = AZ_MAX_MOVES;
    }
    __syncthreads();
    return total;
}

struct MmTree {                    // node records, [roots + capacity]
    azc::Pos* pos;
    int* score;                    // negamax(node, remaining depth)
    long long* calls;              // negamax() invocations in the node's subtree, the node included
    int* nchild;                   // entries of an expanded node, 0 for a terminal one
    int* child_begin;              // its children are contiguous
    unsigned long long* total;     // entries of the level being counted
    unsigned long long* bump;      // next free node
    int* err;
};

// One wavefront per node of a level that still has depth below it: the terminal rule (chess.rs:269-278
// with depth = rem; a root is expanded whatever its material, chess.rs:298-302) or the entry count.
__global__ void __launch_bounds__(64) k_mm_count(MmTree t, int begin, int count, int rem, int is_root) {
    __shared__ Edge s_ed[AZ_MAX_MOVES];
    __shared__ uint16_t s_ent[AZ_MAX_MOVES];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= count) return;
    const int node = vgpr_index(begin + (int)blockIdx.x);
    const azc::Pos p = t.pos[node];
    bool chk;
    const int n = mm_gen(p, s_ed, s_ent, lane, &chk, t.err);
    const bool over = n == 0 || (!is_root && azc::insufficient_material(p));
    if (lane == 0) {
        t.nchild[node] = over ? 0 : n;
        t.child_begin[node] = 0;
        t.score[node] = n == 0 && chk ? -(MM_MATE + rem) : 0;
        t.calls[node] = 1;
        if (!over) atomicAdd(t.total, (unsigned long long)n);
    }
}

// One wavefront per expanded node: its children, one per lane, at a range taken from the bump
// counter (one integer atomic per wave; no result depends on where a range lands).  limit: the
// buffer's end, checked before anything is written.  Roots also give the caller's moves / promo rows.
__global__ void __launch_bounds__(64) k_mm_expand(MmTree t, int begin, int count, unsigned long long limit,
                                                  int* __restrict__ root_moves, int* __restrict__ root_promo) {
    __shared__ Edge s_ed[AZ_MAX_MOVES];
    __shared__ uint16_t s_ent[AZ_MAX_MOVES];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= count) return;
    const int node = vgpr_index(begin + (int)blockIdx.x);
    if (t.nchild[node] == 0) return;
    const azc::Pos p = t.pos[node];
    bool chk;
    const int n = mm_gen(p, s_ed, s_ent, lane, &chk, t.err);
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(t.bump, (unsigned long long)n);
    base = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    if (n != t.nchild[node] || base + (unsigned long long)n > limit) {
        if (lane == 0) { atomicExch(t.err, 2); t.nchild[node] = 0; }
        return;
    }
    if (lane == 0) t.child_begin[node] = (int)base;
    for (int e = lane; e < n; e += 64) {
        const int ent = s_ent[e];
        t.pos[base + e] = mm_play(p, ent);
        if (root_moves) {
            root_moves[(size_t)node * AZ_MAX_MOVES + e] = ent & azc::IDX_MASK;
            root_promo[(size_t)node * AZ_MAX_MOVES + e] = ent >> 12;
        }
    }
}

// One wavefront per frontier node: negamax(node, rem) depth-first.  Level d of the stack holds the
// position and entry list of the node `d` plies below the frontier node while its children are
// searched one after the other; a node with one ply left gives each lane one child (play, the
// serial generator for the move count and the check flag, the terminal rule, the material sum) and
// takes the wave maximum.  All control flow is wave-uniform.
struct MmLevel {
    uint16_t ent[AZ_MAX_MOVES];
    azc::Pos pos;
    int n, k, best, pad;
};
// Two waves per SIMD: left to itself the compiler takes more than 256 registers for one wave per
// SIMD (128 positions at depth 4: 58.3 ms); held to 256 it spills 20 bytes a lane and runs in
// 40.9 ms; at three waves (168 registers, 448 bytes of scratch) 52.6 ms.  AZ_MM_DFS_WAVES: A/B builds.
#ifndef AZ_MM_DFS_WAVES
#define AZ_MM_DFS_WAVES 2
#endif
__attribute__((amdgpu_waves_per_eu(AZ_MM_DFS_WAVES, AZ_MM_DFS_WAVES)))
__global__ void __launch_bounds__(64) k_mm_dfs(MmTree t, int begin, int count, int rem) {
    __shared__ Edge s_ed[AZ_MAX_MOVES];
    __shared__ MmLevel s_lv[MM_STACK];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= count) return;
    const int node = vgpr_index(begin + (int)blockIdx.x);
    azc::Pos cur = t.pos[node];
    long long calls = 1;
    int result;
    if (rem <= 0) {
        result = mm_static(cur);
    } else {
        int d = 0, ret = 0;
        bool entering = true;
        for (;;) {
            if (entering) {                               // cur = the node at level d, rem - d plies left
                const int left = rem - d;
                MmLevel& lv = s_lv[d];
                bool chk;
                const int n = mm_gen(cur, s_ed, lv.ent, lane, &chk, t.err);
                if (n == 0) {
                    ret = chk ? -(MM_MATE + left) : 0;
                    entering = false;
                } else if (azc::insufficient_material(cur)) {
                    ret = 0;
                    entering = false;
                } else if (left == 1) {
                    int best = INT_MIN;
                    for (int e = lane; e < n; e += 64) best = max(best, -mm_static(mm_play(cur, lv.ent[e])));
                    ret = wave_max_i32(best);
                    calls += n;
                    entering = false;
                } else {
                    if (lane == 0) { lv.pos = cur; lv.n = n; lv.k = 0; lv.best = INT_MIN; }
                    __syncthreads();
                    cur = mm_play(cur, lv.ent[0]);
                    calls++;
                    d++;
                }
            } else {                                      // ret = the value of the node at level d
                if (d == 0) { result = ret; break; }
                d--;
                MmLevel& lv = s_lv[d];
                const int best = max(lv.best, -ret), k = lv.k + 1;
                if (k < lv.n) {
                    __syncthreads();
                    if (lane == 0) { lv.best = best; lv.k = k; }
                    __syncthreads();
                    cur = mm_play(lv.pos, lv.ent[k]);
                    calls++;
                    d++;
                    entering = true;
                } else {
                    ret = best;
                }
            }
        }
    }
    if (lane == 0) {
        t.score[node] = result;
        t.calls[node] = calls;
    }
}

// One thread per node of a materialised level above the frontier: max over its children of -score
__global__ void __launch_bounds__(256) k_mm_backup(MmTree t, int begin, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int node = begin + i, n = t.nchild[node];
    if (n == 0) return;                                   // terminal: k_mm_count wrote its value
    const int c0 = t.child_begin[node];
    int best = INT_MIN;
    long long calls = 1;
    for (int c = c0; c < c0 + n; c++) {
        best = max(best, -t.score[c]);
        calls += t.calls[c];
    }
    t.score[node] = best;
    t.calls[node] = calls;
}

// scores[i][k] = -negamax(child k of root i, depth - 1); nodes[i] = the calls below the root
__global__ void __launch_bounds__(256) k_mm_root_out(MmTree t, int m, int* __restrict__ scores, int* __restrict__ nmoves,
                                                     long long* __restrict__ nodes) {
    if ((int)blockIdx.x >= m) return;
    const int i = vgpr_index((int)blockIdx.x), n = t.nchild[i], c0 = t.child_begin[i];
    for (int k = threadIdx.x; k < n; k += 256) scores[(size_t)i * AZ_MAX_MOVES + k] = -t.score[c0 + k];
    if (threadIdx.x == 0) {
        nmoves[i] = n;
        nodes[i] = t.calls[i] - 1;
    }
}

// ------------------------------------------------------------------ host
struct EntSink {                   // legal_moves() with the four promotion entries (tree.rs:86-89 order: Q R B N)
    uint16_t* ent; int n;
    void put(int e) { if (n < AZ_MAX_MOVES && ent) ent[n] = (uint16_t)e; n++; }
    void operator()(int idx) {
        const int mv = idx & azc::IDX_MASK;
        if (idx & azc::PROMO_FLAG) for (int r = 0; r < 4; r++) put(mv | ((azc::QUEEN - r) << 12));
        else put(mv);
    }
};

static int host_negamax(const azc::Pos& p, int depth, int64_t& calls, bool& overflow) {
    calls++;
    if (depth == 0) return mm_static(p);
    uint16_t ent[AZ_MAX_MOVES];
    EntSink s{ent, 0};
    bool chk, lep;
    azc::gen_legal(p, s, &chk, &lep);
    if (s.n == 0) return chk ? -(MM_MATE + depth) : 0;
    if (azc::insufficient_material(p)) return 0;
    if (s.n > AZ_MAX_MOVES) { overflow = true; s.n = AZ_MAX_MOVES; }
    int best = INT_MIN;
    for (int k = 0; k < s.n; k++) {
        const int v = -host_negamax(mm_play(p, ent[k]), depth - 1, calls, overflow);
        best = v > best ? v : best;
    }
    return best;
}

struct MmRoot { std::vector<uint16_t> ent; };

static int minimax_host(const azc::Pos* pos, int n, int depth, const std::vector<MmRoot>& roots, int32_t* scores,
                        int64_t* nodes) {
    struct Task { int i, k; };
    std::vector<Task> tasks;
    for (int i = 0; i < n; i++)
        for (int k = 0; k < (int)roots[i].ent.size(); k++) tasks.push_back({i, k});
    std::vector<int64_t> calls(tasks.size(), 0);
    std::atomic<size_t> next{0};
    std::atomic<bool> overflow{false};
    auto work = [&]() {
        for (size_t j; (j = next.fetch_add(1)) < tasks.size();) {
            const Task tk = tasks[j];
            bool ov = false;
            const azc::Pos c = mm_play(pos[tk.i], roots[tk.i].ent[tk.k]);
            scores[(size_t)tk.i * AZ_MAX_MOVES + tk.k] = -host_negamax(c, depth - 1, calls[j], ov);
            if (ov) overflow = true;
        }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nthr = std::min<size_t>(std::min<size_t>(16, hw ? hw : 1), tasks.size());
    std::vector<std::thread> pool;
    for (size_t th = 1; th < nthr; th++) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    if (overflow) return fail("az_minimax_scores: a position in the tree lists more than 256 moves");
    if (nodes) {
        for (int i = 0; i < n; i++) nodes[i] = 0;
        for (size_t j = 0; j < tasks.size(); j++) nodes[tasks[j].i] += calls[j];
    }
    return 0;
}

static long long frontier_capacity() {
    long long cap = MM_FRONTIER_DEFAULT;
    if (const char* e = getenv("AZ_MINIMAX_FRONTIER")) {
        char* end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (end != e) cap = v;
    }
    return cap < MM_FRONTIER_MIN ? MM_FRONTIER_MIN : (cap > MM_FRONTIER_MAX ? MM_FRONTIER_MAX : cap);
}

// The GPU path.  h_* are [n][AZ_MAX_MOVES] staging rows the caller copies the valid prefixes from.
static int minimax_device(int device, const azc::Pos* pos, int n, int depth, const std::vector<MmRoot>& roots,
                          int32_t* h_moves, int32_t* h_promo, int32_t* h_scores, int32_t* h_nmoves, int64_t* h_nodes) {
    const long long cap = frontier_capacity();
    // chunks of positions whose own entries (level 1) fit the buffer together
    std::vector<int> chunk_end;
    int max_m = 0;
    for (int i = 0, b = 0; i < n;) {
        long long sum = 0;
        while (i < n && sum + (long long)roots[i].ent.size() <= cap) sum += (long long)roots[i++].ent.size();
        chunk_end.push_back(i);
        max_m = std::max(max_m, i - b);
        b = i;
    }
    AZ_HIP(hipSetDevice(device));
    hipStream_t st;
    AZ_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    std::vector<void*> bufs;
    bool oom = false;
    auto dmal = [&](size_t bytes) -> void* {
        void* p = nullptr;
        if (hipMalloc(&p, bytes < 16 ? 16 : bytes) != hipSuccess) { oom = true; return nullptr; }
        bufs.push_back(p);
        return p;
    };
    const size_t N = (size_t)max_m + (size_t)cap, M = (size_t)max_m;
    MmTree t;
    t.pos = (azc::Pos*)dmal(N * sizeof(azc::Pos));
    t.score = (int*)dmal(N * 4);
    t.calls = (long long*)dmal(N * 8);
    t.nchild = (int*)dmal(N * 4);
    t.child_begin = (int*)dmal(N * 4);
    unsigned long long* ctr = (unsigned long long*)dmal(3 * 8);   // total, bump, err
    t.total = ctr;
    t.bump = ctr + 1;
    t.err = (int*)(ctr + 2);
    int* d_moves = (int*)dmal(M * AZ_MAX_MOVES * 4);
    int* d_promo = (int*)dmal(M * AZ_MAX_MOVES * 4);
    int* d_scores = (int*)dmal(M * AZ_MAX_MOVES * 4);
    int* d_nmoves = (int*)dmal(M * 4);
    long long* d_nodes = (long long*)dmal(M * 8);
    int rc = oom ? fail("az_minimax_scores: hipMalloc failed") : 0;
    auto run = [&]() -> int {
        int b = 0;
        for (int end : chunk_end) {
            const int m = end - b;
            unsigned long long h_ctr[3] = {0, (unsigned long long)m, 0};
            AZ_HIP(hipMemcpyAsync(t.pos, pos + b, (size_t)m * sizeof(azc::Pos), hipMemcpyHostToDevice, st));
            AZ_HIP(hipMemcpyAsync(ctr, h_ctr, sizeof h_ctr, hipMemcpyHostToDevice, st));
            AZ_HIP(hipStreamSynchronize(st));                   // h_ctr is reused below
            const unsigned long long limit = (unsigned long long)m + (unsigned long long)cap;
            // level l = the nodes l plies below the roots, [lbeg[l], lbeg[l] + lcnt[l])
            int lbeg[AZ_MINIMAX_MAX_DEPTH + 1] = {0}, lcnt[AZ_MINIMAX_MAX_DEPTH + 1] = {m};
            unsigned long long used = (unsigned long long)m;
            int L = 0;
            // materialise while the next level fits; a level with no depth below it is only ever the
            // roots' own children (depth 1): deeper leaves are searched one per lane, not one per wave
            while (depth - L >= 1 && (L == 0 || depth - L >= 2) && lcnt[L] > 0) {
                AZ_HIP(hipMemsetAsync(t.total, 0, 8, st));
                k_mm_count<<<lcnt[L], 64, 0, st>>>(t, lbeg[L], lcnt[L], depth - L, L == 0);
                AZ_HIP(hipGetLastError());
                AZ_HIP(hipMemcpyAsync(h_ctr, t.total, 8, hipMemcpyDeviceToHost, st));
                AZ_HIP(hipStreamSynchronize(st));
                const unsigned long long total = h_ctr[0];
                if (used + total > limit) {
                    if (L == 0) return fail("az_minimax_scores: the roots' entries exceed the frontier buffer");
                    break;
                }
                k_mm_expand<<<lcnt[L], 64, 0, st>>>(t, lbeg[L], lcnt[L], limit, L == 0 ? d_moves : nullptr,
                                                    L == 0 ? d_promo : nullptr);
                AZ_HIP(hipGetLastError());
                lbeg[L + 1] = (int)used;
                lcnt[L + 1] = (int)total;
                used += total;
                L++;
            }
            if (lcnt[L] > 0) {
                k_mm_dfs<<<lcnt[L], 64, 0, st>>>(t, lbeg[L], lcnt[L], depth - L);
                AZ_HIP(hipGetLastError());
            }
            for (int l = L - 1; l >= 0; l--) {
                k_mm_backup<<<(lcnt[l] + 255) / 256, 256, 0, st>>>(t, lbeg[l], lcnt[l]);
                AZ_HIP(hipGetLastError());
            }
            k_mm_root_out<<<m, 256, 0, st>>>(t, m, d_scores, d_nmoves, d_nodes);
            AZ_HIP(hipGetLastError());
            const size_t row = (size_t)AZ_MAX_MOVES * 4;
            AZ_HIP(hipMemcpyAsync(h_moves + (size_t)b * AZ_MAX_MOVES, d_moves, m * row, hipMemcpyDeviceToHost, st));
            AZ_HIP(hipMemcpyAsync(h_promo + (size_t)b * AZ_MAX_MOVES, d_promo, m * row, hipMemcpyDeviceToHost, st));
            AZ_HIP(hipMemcpyAsync(h_scores + (size_t)b * AZ_MAX_MOVES, d_scores, m * row, hipMemcpyDeviceToHost, st));
            AZ_HIP(hipMemcpyAsync(h_nmoves + b, d_nmoves, (size_t)m * 4, hipMemcpyDeviceToHost, st));
            AZ_HIP(hipMemcpyAsync(h_nodes + b, d_nodes, (size_t)m * 8, hipMemcpyDeviceToHost, st));
            AZ_HIP(hipMemcpyAsync(h_ctr, ctr, sizeof h_ctr, hipMemcpyDeviceToHost, st));
            AZ_HIP(hipStreamSynchronize(st));
            if ((int)h_ctr[2] == 1) return fail("az_minimax_scores: a position in the tree lists more than 256 moves");
            if ((int)h_ctr[2] != 0) return fail("az_minimax_scores: frontier buffer accounting failed");
            b = end;
        }
        return 0;
    };
    if (!rc) rc = run();
    (void)hipStreamSynchronize(st);
    for (void* p : bufs) (void)hipFree(p);
    (void)hipStreamDestroy(st);
    return rc;
}

}  // namespace azi

using namespace azi;

extern "C" int az_minimax_scores(int device, const az_pos* pos, int n, int depth, int32_t* moves, int32_t* promo,
                                 int32_t* scores, int32_t* nmoves, int64_t* nodes) {
    if (n < 0 || (n > 0 && (!pos || !moves || !promo || !scores || !nmoves)))
        return fail("az_minimax_scores: null argument");
    if (depth < 1 || depth > AZ_MINIMAX_MAX_DEPTH)
        return fail("az_minimax_scores: depth " + std::to_string(depth) + " outside 1.." +
                    std::to_string(AZ_MINIMAX_MAX_DEPTH));
    if (device < AZ_DEVICE_HOST) return fail("az_minimax_scores: bad device");
    if (n == 0) return 0;
    const azc::Pos* P = reinterpret_cast<const azc::Pos*>(pos);
    std::vector<MmRoot> roots(n);
    for (int i = 0; i < n; i++) {
        if (const char* why = azc::setup_error(P[i]))
            return fail("az_minimax_scores: position " + std::to_string(i) + " rejected: " + why);
        uint16_t ent[AZ_MAX_MOVES];
        EntSink s{ent, 0};
        bool chk, lep;
        azc::gen_legal(P[i], s, &chk, &lep);
        if (s.n > AZ_MAX_MOVES)
            return fail("az_minimax_scores: position " + std::to_string(i) + " lists " + std::to_string(s.n) +
                        " moves (more than " + std::to_string(AZ_MAX_MOVES) + ")");
        roots[i].ent.assign(ent, ent + s.n);
    }
    const size_t R = (size_t)n * AZ_MAX_MOVES;
    std::vector<int32_t> h_moves(R, 0), h_promo(R, 0), h_scores(R, 0), h_nmoves(n, 0);
    std::vector<int64_t> h_nodes(n, 0);
    if (device == AZ_DEVICE_HOST) {
        for (int i = 0; i < n; i++) {
            h_nmoves[i] = (int32_t)roots[i].ent.size();
            for (int k = 0; k < h_nmoves[i]; k++) {
                h_moves[(size_t)i * AZ_MAX_MOVES + k] = roots[i].ent[k] & azc::IDX_MASK;
                h_promo[(size_t)i * AZ_MAX_MOVES + k] = roots[i].ent[k] >> 12;
            }
        }
        if (int rc = minimax_host(P, n, depth, roots, h_scores.data(), h_nodes.data())) return rc;
    } else {
        if (int rc = minimax_device(device, P, n, depth, roots, h_moves.data(), h_promo.data(), h_scores.data(),
                                    h_nmoves.data(), h_nodes.data()))
            return rc;
    }
    // outputs are written only now, and only the entries a position has
    for (int i = 0; i < n; i++) {
        const size_t o = (size_t)i * AZ_MAX_MOVES;
        nmoves[i] = h_nmoves[i];
        for (int k = 0; k < h_nmoves[i] && k < AZ_MAX_MOVES; k++) {
            moves[o + k] = h_moves[o + k];
            promo[o + k] = h_promo[o + k];
            scores[o + k] = h_scores[o + k];
        }
        if (nodes) nodes[i] = h_nodes[i];
    }
    return 0;
}

extern "C" int az_minimax_best(const int32_t* scores, int nmoves, float u) {
    if (!scores || nmoves <= 0) return -1;
    int best = scores[0], ties = 0;
    for (int k = 0; k < nmoves; k++) best = scores[k] > best ? scores[k] : best;
    for (int k = 0; k < nmoves; k++) ties += scores[k] == best;
    int pick = (int)(u * (float)ties);                     // floor for u >= 0
    pick = pick < 0 ? 0 : (pick > ties - 1 ? ties - 1 : pick);
    for (int k = 0; k < nmoves; k++)
        if (scores[k] == best && pick-- == 0) return k;
    return -1;
}
