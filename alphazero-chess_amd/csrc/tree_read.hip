// tree_read.hip -- az_search_read_tree / az_search_read_pv: whole search trees and principal variations read
// from the engine's arenas (az_internal.h: Node, Edge, npos per game) as compact CSR records.
//
// A raw copy of the arenas is sized for 218 edges at every node (EMAX); the live part of a tree is a small
// fraction of it.  The export is therefore compacted on the device, one workgroup per listed game:
//   k_tree_count   one wavefront walks the game's nodes in ascending id, 64 a chunk.  A node is kept iff its
//                  parent is kept, its parent's edge has N >= min_visits and its depth is <= max_depth; ids
//                  ascend from parent to child, so one forward pass decides every node (parents of an earlier
//                  chunk are looked up in the table, parents inside the chunk resolved over ballots, as in
//                  search.hip's reroot_keep_subtree).  It writes the game's tables -- a node's ordinal in the
//                  export (-1: left out), its first edge there, which of its parent's edges leads to it -- and
//                  the kept node and edge counts.
//   k_tree_offsets exclusive scan of the counts over the listed games: the CSR offsets.
//   k_tree_write   four wavefronts, a kept node each at a time: the node record, its edges (child ids through
//                  the table, AZ_TREE_CUT where the child was left out) and its position, straight to their
//                  CSR places in the staging buffers.
// The kernels only read the engine's state.  That state was written by other launches, so every load of it
// sits behind a VGPR-held game index (the note above load_fresh in az_internal.h); the tables are global
// scratch written and read back by the one wavefront of k_tree_count: a workgroup-scope fence orders a
// chunk's stores before the next chunk's loads, which go through load_fresh.
#include <algorithm>
#include <string>
#include <vector>

#include "az_internal.h"

namespace azi {

struct TreeRead {
    int* ord = nullptr;        // [G][NMAX] a node's ordinal in the export, -1 = left out
    int* ebeg = nullptr;       // [G][NMAX] ... its edge_begin there
    int* pedge = nullptr;      // [G][NMAX] ... which of its parent's edges leads to it
    int* games = nullptr;      // [cap_n] the listed slots
    int* cnt = nullptr;        // [cap_n][2] kept nodes, kept edges
    long long* off = nullptr;  // [2][cap_n + 1] node offsets, edge offsets
    int cap_n = 0;
};

namespace {

__device__ __forceinline__ int tr_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// a node record whose edge range lies inside the game's arena (anything else is read as a node without edges)
__device__ __forceinline__ int safe_nedges(const Engine& E, const Node& nd) {
    return (size_t)nd.edge_begin + nd.nedges <= (size_t)E.EMAX ? (int)nd.nedges : 0;
}

__global__ void __launch_bounds__(64) k_tree_count(Engine E, const int* games, int min_visits, int max_depth,
                                                   int* t_ord, int* t_ebeg, int* t_pedge, int* cnt) {
    const int k = vgpr_index(blockIdx.x), lane = threadIdx.x;
    const int g = games[k];
    const Node* nodes = E.nodes + (size_t)g * E.NMAX;
    const Edge* edges = E.edges + (size_t)g * E.EMAX;
    int* ord = t_ord + (size_t)g * E.NMAX;
    int* ebeg = t_ebeg + (size_t)g * E.NMAX;
    int* pedge = t_pedge + (size_t)g * E.NMAX;
    const int nc = max(min(E.node_count[g], E.NMAX), 0);
    int nk = 0, ek = 0;
    for (int base = 0; base < nc; base += 64) {
        const int i = base + lane;
        const bool valid = i < nc;
        const Node nd = nodes[valid ? i : 0];
        const int p = nd.parent;
        // which of the parent's edges leads here, and its visits
        int pe = -1, pn = 0;
        if (valid && i > 0 && p >= 0 && p < i) {
            const Node pd = nodes[p];
            const int n = safe_nedges(E, pd);
            for (int j = 0; j < n; j++) {
                if (edges[pd.edge_begin + j].child == i) { pe = j; pn = edges[pd.edge_begin + j].N; break; }
            }
        }
        bool known = true, keep = false;
        if (valid) {
            if (i == 0) keep = true;
            else if (pe < 0 || pn < min_visits || (max_depth >= 0 && (int)nd.depth > max_depth)) keep = false;
            else if (p < base) keep = load_fresh(&ord[p]) >= 0;
            else known = false;                                // the parent is a lower lane of this chunk
        }
        for (;;) {                                             // the lowest unknown lane's parent is known
            const unsigned long long km = __ballot(known), kp = __ballot(keep);
            if (km == ~0ull) break;
            if (!known && ((km >> (p - base)) & 1ull)) { known = true; keep = (kp >> (p - base)) & 1ull; }
        }
        const int n = keep ? safe_nedges(E, nd) : 0;
        const int in = tr_incl_scan(keep ? 1 : 0, lane), ie = tr_incl_scan(n, lane);
        if (valid) {
            ord[i] = keep ? nk + in - 1 : -1;
            ebeg[i] = ek + ie - n;
            pedge[i] = pe;
        }
        nk += __builtin_amdgcn_readlane(in, 63);
        ek += __builtin_amdgcn_readlane(ie, 63);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
    if (lane == 0) { cnt[2 * k] = nk; cnt[2 * k + 1] = ek; }
}

// off[0 .. n] = exclusive scan of the node counts, off[n + 1 .. 2 n + 1] of the edge counts
__global__ void __launch_bounds__(64) k_tree_offsets(const int* cnt, int n, long long* off) {
    const int lane = vgpr_index(threadIdx.x);
    long long tn = 0, te = 0;
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        const int cn = k < n ? cnt[2 * k] : 0, ce = k < n ? cnt[2 * k + 1] : 0;
        const int in = tr_incl_scan(cn, lane), ie = tr_incl_scan(ce, lane);   // a chunk: <= 64 * EMAX < 2^31
        if (k < n) { off[k] = tn + in - cn; off[n + 1 + k] = te + ie - ce; }
        tn += __builtin_amdgcn_readlane(in, 63);
        te += __builtin_amdgcn_readlane(ie, 63);
    }
    if (lane == 0) { off[n] = tn; off[2 * n + 1] = te; }
}

constexpr int WRITE_WAVES = 4;

__global__ void __launch_bounds__(64 * WRITE_WAVES) k_tree_write(Engine E, const int* games, int n_games,
                                                                 const int* t_ord, const int* t_ebeg, const int* t_pedge,
                                                                 const long long* off, az_tree_node* out_nodes,
                                                                 az_tree_edge* out_edges, azc::Pos* out_states) {
    const int k = vgpr_index(blockIdx.x), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = games[k];
    const Node* nodes = E.nodes + (size_t)g * E.NMAX;
    const Edge* edges = E.edges + (size_t)g * E.EMAX;
    const uint32_t* npos = reinterpret_cast<const uint32_t*>(E.npos + (size_t)g * E.NMAX);
    const int* ord = t_ord + (size_t)g * E.NMAX;
    const int* ebeg = t_ebeg + (size_t)g * E.NMAX;
    const int* pedge = t_pedge + (size_t)g * E.NMAX;
    const int nc = max(min(E.node_count[g], E.NMAX), 0);
    const long long n0 = off[k], e0 = off[n_games + 1 + k];
    constexpr int PW = sizeof(azc::Pos) / 4;                   // a position: 20 dwords
    for (int i = wave; i < nc; i += WRITE_WAVES) {
        const int o = ord[i];
        if (o < 0) continue;
        const Node nd = nodes[i];
        const int ne = safe_nedges(E, nd), nb = ebeg[i];
        if (lane == 0) {
            az_tree_node r;
            r.parent = i ? ord[nd.parent] : -1;
            r.parent_edge = i ? pedge[i] : -1;
            r.edge_begin = nb; r.nedges = ne; r.depth = nd.depth; r.nsum = nd.nsum;
            out_nodes[n0 + o] = r;
        }
        if (out_states && lane < PW)
            reinterpret_cast<uint32_t*>(out_states + n0 + o)[lane] = npos[(size_t)i * PW + lane];
        for (int e = lane; e < ne; e += 64) {
            const Edge ed = edges[nd.edge_begin + e];
            az_tree_edge r;
            r.prior = ed.P; r.score = ed.W; r.visits = ed.N;
            r.index = ed.idx & azc::IDX_MASK;
            r.flags = (ed.idx & azc::PROMO_FLAG) ? 1u : 0u;
            int c = ed.child;
            if (c >= 0) {
                c = c < nc ? ord[c] : -1;
                if (c < 0) c = AZ_TREE_CUT;
            }
            r.child = c;
            out_edges[e0 + nb + e] = r;
        }
    }
}

// one wavefront per game: the most visited edge, ties to the larger move index, down the tree
__global__ void __launch_bounds__(64) k_tree_pv(Engine E, int cap, int* moves, int* len, float* q, uint32_t* visits) {
    const int g = vgpr_index(blockIdx.x), lane = threadIdx.x;
    const Node* nodes = E.nodes + (size_t)g * E.NMAX;
    const Edge* edges = E.edges + (size_t)g * E.EMAX;
    const int nc = max(min(E.node_count[g], E.NMAX), 0);
    int node = 0, n = 0;
    float q0 = 0.0f;
    uint32_t v0 = 0;
    while (n < cap && node >= 0 && node < nc) {
        const Node nd = nodes[node];
        const int ne = safe_nedges(E, nd);
        int key = -1, be = 0;                                  // key = N << 12 | index: N first, then the index
        for (int e = lane; e < ne; e += 64) {
            const Edge ed = edges[nd.edge_begin + e];
            const int kk = (int)ed.N << 12 | (ed.idx & azc::IDX_MASK);
            if (kk > key) { key = kk; be = e; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int ok = __shfl_xor(key, o, 64), oe = __shfl_xor(be, o, 64);
            if (ok > key) { key = ok; be = oe; }               // distinct indices: no two keys are equal
        }
        if (key < (1 << 12)) break;                            // no edge, or the best has no visit
        const Edge best = edges[nd.edge_begin + be];
        if (n == 0) { q0 = best.W / (float)best.N; v0 = best.N; }
        if (lane == 0) moves[(size_t)g * cap + n] = key & azc::IDX_MASK;
        n++;
        node = best.child;
    }
    if (lane == 0) {
        if (len) len[g] = n;
        if (q) q[g] = q0;
        if (visits) visits[g] = v0;
    }
}

template <typename T> int tr_alloc(T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc(&q, bytes) != hipSuccess) return fail("az_search_read_tree: hipMalloc failed (" + std::to_string(bytes) + " B)");
    *p = (T*)q;
    return 0;
}

// the per-game tables at the first call, the per-call lists grown to n
int ensure_scratch(const Engine& E, TreeRead** scratch, int n) {
    if (!*scratch) {
        TreeRead* t = new TreeRead;
        const size_t slots = (size_t)E.G * E.NMAX;
        if (tr_alloc(&t->ord, slots) || tr_alloc(&t->ebeg, slots) || tr_alloc(&t->pedge, slots)) {
            tree_read_free(t);
            return -1;
        }
        *scratch = t;
    }
    TreeRead* t = *scratch;
    if (n > t->cap_n || !t->games) {
        (void)hipFree(t->games); (void)hipFree(t->cnt); (void)hipFree(t->off);
        t->games = nullptr; t->cnt = nullptr; t->off = nullptr; t->cap_n = 0;
        const int cap = std::max(n, E.G);
        if (tr_alloc(&t->games, (size_t)cap) || tr_alloc(&t->cnt, 2 * (size_t)cap) || tr_alloc(&t->off, 2 * ((size_t)cap + 1)))
            return -1;
        t->cap_n = cap;
    }
    return 0;
}

}  // namespace

void tree_read_free(TreeRead* t) {
    if (!t) return;
    for (void* p : {(void*)t->ord, (void*)t->ebeg, (void*)t->pedge, (void*)t->games, (void*)t->cnt, (void*)t->off})
        if (p) (void)hipFree(p);
    delete t;
}

int tree_read(const Engine& E, hipStream_t st, TreeRead** scratch, const int32_t* games, int n, int min_visits,
              int max_depth, int64_t* node_off, int64_t* edge_off, az_tree_node* nodes, int64_t node_cap,
              az_tree_edge* edges, int64_t edge_cap, az_pos* states) {
    // every refusal comes before the first write to an output
    if (n < 0) return fail("az_search_read_tree: n = " + std::to_string(n) + " < 0");
    if (min_visits < 0) return fail("az_search_read_tree: min_visits = " + std::to_string(min_visits) + " < 0");
    if (!node_off || !edge_off) return fail("az_search_read_tree: node_off / edge_off are NULL");
    if ((nodes == nullptr) != (edges == nullptr))
        return fail("az_search_read_tree: nodes and edges must both be given, or both be NULL (sizing)");
    std::vector<int> list;
    if (games) {
        list.assign(games, games + n);
        for (int k = 0; k < n; k++)
            if (list[k] < 0 || list[k] >= E.G)
                return fail("az_search_read_tree: games[" + std::to_string(k) + "] = " + std::to_string(list[k]) +
                            " is outside 0.." + std::to_string(E.G - 1));
    } else {
        n = E.G;
        list.resize(n);
        for (int k = 0; k < n; k++) list[k] = k;
    }
    if (n == 0) {
        node_off[0] = 0; edge_off[0] = 0;
        return 0;
    }
    if (ensure_scratch(E, scratch, n)) return -1;
    TreeRead* t = *scratch;
    AZ_HIP(hipMemcpyAsync(t->games, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    k_tree_count<<<n, 64, 0, st>>>(E, t->games, min_visits, max_depth, t->ord, t->ebeg, t->pedge, t->cnt);
    k_tree_offsets<<<1, 64, 0, st>>>(t->cnt, n, t->off);
    AZ_HIP(hipGetLastError());
    std::vector<long long> off(2 * ((size_t)n + 1));
    AZ_HIP(hipMemcpyAsync(off.data(), t->off, off.size() * 8, hipMemcpyDeviceToHost, st));
    AZ_HIP(hipStreamSynchronize(st));
    const long long tn = off[n], te = off[2 * (size_t)n + 1];
    if (nodes) {
        if (node_cap < tn) return fail("az_search_read_tree: node_cap = " + std::to_string(node_cap) + ", the export has " + std::to_string(tn) + " nodes");
        if (edge_cap < te) return fail("az_search_read_tree: edge_cap = " + std::to_string(edge_cap) + ", the export has " + std::to_string(te) + " edges");
        az_tree_node* dn = nullptr; az_tree_edge* de = nullptr; azc::Pos* ds = nullptr;
        int rc = tr_alloc(&dn, (size_t)tn) || tr_alloc(&de, (size_t)te) || (states && tr_alloc(&ds, (size_t)tn)) ? -1 : 0;
        hipError_t e = hipSuccess;
        if (!rc) {
            k_tree_write<<<n, 64 * WRITE_WAVES, 0, st>>>(E, t->games, n, t->ord, t->ebeg, t->pedge, t->off, dn, de, ds);
            e = hipGetLastError();
            // one copy per output array
            if (e == hipSuccess && tn) e = hipMemcpyAsync(nodes, dn, (size_t)tn * sizeof(az_tree_node), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && te) e = hipMemcpyAsync(edges, de, (size_t)te * sizeof(az_tree_edge), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && states && tn) e = hipMemcpyAsync(states, ds, (size_t)tn * sizeof(azc::Pos), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        (void)hipFree(dn); (void)hipFree(de); (void)hipFree(ds);
        if (rc) return rc;
        if (e != hipSuccess) return fail(std::string("az_search_read_tree: ") + hipGetErrorString(e));
    }
    for (int k = 0; k <= n; k++) { node_off[k] = off[k]; edge_off[k] = off[(size_t)n + 1 + k]; }
    return 0;
}

int tree_read_pv(const Engine& E, hipStream_t st, int32_t* moves, int cap, int32_t* len, float* q, uint32_t* visits) {
    if (cap < 0) return fail("az_search_read_pv: cap = " + std::to_string(cap) + " < 0");
    if (!moves && cap > 0) return fail("az_search_read_pv: moves is NULL");
    const int G = E.G;
    int* dm = nullptr; int* dl = nullptr; float* dq = nullptr; uint32_t* dv = nullptr;
    int rc = tr_alloc(&dm, (size_t)G * cap) || tr_alloc(&dl, (size_t)G) || tr_alloc(&dq, (size_t)G) || tr_alloc(&dv, (size_t)G) ? -1 : 0;
    hipError_t e = hipSuccess;
    std::vector<int> hl(G);
    std::vector<int32_t> hm((size_t)G * cap);
    if (!rc) {
        k_tree_pv<<<G, 64, 0, st>>>(E, cap, dm, dl, dq, dv);
        e = hipGetLastError();
        if (e == hipSuccess && cap) e = hipMemcpyAsync(hm.data(), dm, hm.size() * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hl.data(), dl, (size_t)G * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && q) e = hipMemcpyAsync(q, dq, (size_t)G * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && visits) e = hipMemcpyAsync(visits, dv, (size_t)G * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipFree(dm); (void)hipFree(dl); (void)hipFree(dq); (void)hipFree(dv);
    if (rc) return rc;
    if (e != hipSuccess) return fail(std::string("az_search_read_pv: ") + hipGetErrorString(e));
    // only the moves of each PV are the caller's to read: the rest of a row stays as it was
    for (int g = 0; g < G; g++) {
        for (int i = 0; i < hl[g]; i++) moves[(size_t)g * cap + i] = hm[(size_t)g * cap + i];
        if (len) len[g] = hl[g];
    }
    return 0;
}

}  // namespace azi
