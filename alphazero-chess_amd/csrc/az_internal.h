// az_internal.h -- shared definitions of libaz's translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/az.h"
#include "chess.h"

static_assert(sizeof(az_pos) == 80, "az_pos layout");
static_assert(sizeof(azc::Pos) == sizeof(az_pos), "Pos == az_pos");
static_assert(sizeof(az_search_cfg) == 64, "az_search_cfg: leaves sits in the former tail padding");

#ifndef AZ_WINOGRAD_DEFAULT
#define AZ_WINOGRAD_DEFAULT 1
#endif
#ifndef AZ_WINO_SPLIT16_DEFAULT
#define AZ_WINO_SPLIT16_DEFAULT 1
#endif
#ifndef AZ_WINO_DERIVE_DEFAULT
#define AZ_WINO_DERIVE_DEFAULT 1
#endif
#ifndef AZ_WINO_ROWS_DEFAULT
#define AZ_WINO_ROWS_DEFAULT 1
#endif
#ifndef AZ_WINO_VROWS_DEFAULT
#define AZ_WINO_VROWS_DEFAULT 1
#endif
// where the shared-row transform runs (wino.h wino_core_h16, VROWS): 0 waves 0-3 after their last step
// of a chunk, 1 all eight waves inside the steps (A/B: DESIGN.md 5.4)
#ifndef AZ_WINO_VROWS_SCHED
#define AZ_WINO_VROWS_SCHED 0
#endif
// boards per workgroup of the row-direct shared-row tower (wino.h wino_core_b2; C3 A/B: DESIGN.md 5.4)
#ifndef AZ_WINO_BOARDS_DEFAULT
#define AZ_WINO_BOARDS_DEFAULT 2
#endif
// weight ring steps of the row-direct form (wino.h WinoRing; C3 A/B of 2, 3, 4: DESIGN.md 5.4)
#ifndef AZ_WINO_ROWS_PF
#define AZ_WINO_ROWS_PF 4
#endif

namespace azi {

// split-f16 products (wino.h wino_core_h16, net.hip winograd_split16): the activation scale Sa, a
// power of two.  |V| <= 4 |x|, so the layer inputs must stay below 65504 / (4 Sa) = 255.8
// (tools/split16_numerics.py: the scale rule); 511.7 in the row-direct form (wino16_rows below)
constexpr float WINO16_SA = 64.0f;
// AZ_WINO_SPLIT16 is a level: 0 no split-f16 products, 1 (the default) at 256 filters, 2 also at 128
// and 64 filters (measured, not yet the default there: DESIGN.md 5.5)
static inline bool wino16_selected(int level, int filters) {
    return filters == 256 ? level >= 1 : (filters == 128 || filters == 64) && level >= 2;
}

// AZ_WINO_DERIVE (default AZ_WINO_DERIVE_DEFAULT): the split-f16 tower at 256 filters streams 12 of the
// 16 Winograd points' weights and derives row 2 from the other three (wino.h wino_core_h16<F, 12>);
// 0, and 128 / 64 filters at any value, stream all 16
static inline int wino16_streamed(bool derive, int filters) { return derive && filters == 256 ? 12 : 16; }
// AZ_WINO_ROWS (default AZ_WINO_ROWS_DEFAULT): where 12 planes are streamed, the row-direct form
// (wino.h wino_core_h16<256, 12, true>: Winograd across columns, the three tap rows direct, 8
// accumulators per output fragment); 0 the derived-row form (16 accumulators).  AZ_WINO_DERIVE=0
// selects the 16-point kernel whatever AZ_WINO_ROWS says.  Its ring is WINO_ROWS_PF steps deep and its
// weight stream ends in as many zero steps.  |D| <= 2 |x|: the layer inputs must stay below 65504 /
// (2 Sa) = 511.7 (255.8 in the other two forms)
constexpr int WINO_ROWS_PF = AZ_WINO_ROWS_PF;
static_assert(12 % WINO_ROWS_PF == 0 && WINO_ROWS_PF >= 2, "the ring's slots must be compile-time");
static inline bool wino16_rows(bool derive, bool rows, int filters) { return wino16_streamed(derive, filters) == 12 && rows; }
// AZ_WINO_VROWS (default AZ_WINO_VROWS_DEFAULT): in the row-direct form, V holds every D row of the
// padded board once (wino.h wino_vr_*: 10 rows x 4 column points, 20 KB per chunk) instead of the four
// patch rows of every tile (32 KB: rows 2, 3 of a tile are rows 0, 1 of the tile below); the same bits
// reach the same products.  Applies only where wino16_rows holds
static inline bool wino16_vrows(bool rows_form, bool vrows) { return rows_form && vrows; }
// AZ_WINO_BOARDS (1 or 2, default AZ_WINO_BOARDS_DEFAULT): in the shared-row form, 2 evaluates two batch
// rows per workgroup on one weight stream, the residual convs' activations in global memory
// (tower.hip tower32w2_kernel); the persistent per-game kernel stays on one board.  Applies only where
// wino16_vrows holds
static inline int wino16_boards(bool vrows_form, int boards) { return vrows_form && boards == 2 ? 2 : 1; }

void set_error(const std::string& msg);
int fail(const std::string& msg);

#define AZ_HIP(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return ::azi::fail(std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// ---------------- loads of state another launch rewrote ----------------
// A load at a provably wave-uniform address compiles to s_load, which goes through the scalar
// data cache; measured on MI355X (round 2): that cache can still hold the line a previous launch
// of the stream read, so vector stores made in between are not seen (k_expand read stale leaf
// records).  Engine state that launches hand to each other (batch counters, row -> game maps,
// per-game records) is therefore read through vector loads: load_fresh for a single counter,
// vgpr_index for an index that would otherwise make every load behind it scalar.
__device__ __forceinline__ int load_fresh(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int vgpr_index(int i) {
    asm volatile("" : "+v"(i));
    return i;
}

// ---------------- search tree records (HBM, struct-of-arrays per game) ----------------
struct Node {            // 16 B
    uint32_t edge_begin; // first edge (game-relative)
    uint16_t nedges;     // distinct legal move indices
    uint16_t depth;      // root = 0
    uint32_t nsum;       // sum of child visits (tree.rs:121 minus the +1)
    int32_t parent;
};
struct Edge {            // 16 B, one dwordx4 per lane in the select walk
    float P;             // prior (policy[i], noised at roots)
    float W;             // scores[i]
    uint16_t N;          // visits[i]
    uint16_t idx;        // move index | PROMO_FLAG
    int32_t child;       // node id, or CHILD_*
};
static_assert(sizeof(Node) == 16 && sizeof(Edge) == 16, "tree record layout");
enum { CHILD_NONE = -1, CHILD_DRAW = -2, CHILD_WIN = -3 };
enum { LEAF_EVAL = 0, LEAF_DRAW = 1, LEAF_WIN = 2, LEAF_CACHED = 3 };
// leaf-parallel search (Engine::K > 1) only: the leaf ended on the edge an earlier new leaf of the same
// wave (Engine::leaf_src) expands, and takes that leaf's value
enum { LEAF_SHARED = 4 };
constexpr int LEAVES_MAX = 8;      // az_search_cfg.leaves <= 8: one lane per earlier leaf of a wave
constexpr int MAX_EDGES = 224;     // >= 218 legal moves
constexpr int HMAX = 512;          // game history cap (200 fullmoves -> <= 400 plies)

struct StepRec {                   // device -> host self-play record, 1024 B
    int32_t game_id;
    int16_t ply, action, depth, nvis, kind, result;   // kind 0 = step, 1 = game end
    int16_t end_fullmoves, pad;
    int32_t pad2;
    azc::Pos pos;
    uint16_t vis_idx[MAX_EDGES];
    uint16_t vis_n[MAX_EDGES];
    uint8_t tail[1024 - 24 - 80 - 4 * MAX_EDGES];
};
static_assert(sizeof(StepRec) == 1024, "StepRec");

struct Counters {                  // device-side statistics
    unsigned long long sims, evals, terminal, games_finished, moves, depth_sum, select_bytes, cache_hits;
    int batch_count[2];            // rows of simulation step i in [i & 1]; the backup of step i
                                   // reads and clears it (no reset launch, and the fused step
                                   // kernel allocates step i rows while it backs up step i - 1)
    int rec_count;
    int next_game_id;
    int log_count;
    int log_prior_count;
    int overflow;
    int max_remain;                // tree reuse: the most simulations any root re-rooted by the last k_finish
                                   // still needs (the host clears it before the launch and reads it after)
    unsigned long long shared;     // shared leaves of the leaf-parallel search (az_search_leaf_stats)
    // tree reuse (az_search_reuse_stats): re-roots that kept a subtree, the visits and nodes they kept
    unsigned long long reroots, carried_visits, carried_nodes;
};

// everything the tree kernels need, passed by value
struct Engine {
    int G, S, NMAX, EMAX, PMAX;
    float c_puct, dir_alpha, dir_eps;
    int temp_moves, noise, continuous;
    unsigned long long seed;
    Node* nodes;          // [G][NMAX]
    azc::Pos* npos;       // [G][NMAX]
    Edge* edges;          // [G][EMAX]
    uint32_t* child_hdr;  // [G][EMAX]: for an edge whose child is a node, (child's edge_begin << 8) | nedges
    int* node_count; int* edge_count; int* max_depth;
    int* leaf_node; int* leaf_edge; int* leaf_len; int* leaf_kind; int* leaf_row;
    int* path_node; int* path_edge;        // [G][PMAX]
    azc::Pos* hist; int* hist_len;         // [G][HMAX]
    int* game_id; int* ply; int* active;
    int* row_game; int* row_node;          // [G]
    float* value;                          // [G] per batch row
    const float* sqrt_tab;                 // [S + 2]
    Edge* start_edges; int* start_n;       // startpos root template (priors un-noised)
    StepRec* recs; int rec_cap;
    Counters* ctr;
    int* batch_hist;                       // [S] rows evaluated per sim step
    // FEN evaluation cache (tree.rs:214-219): open addressing, CACHE_PROBES linear probes
    int cache_mask;                        // slots - 1 (slots = power of two), -1 = off
    unsigned* c_state;                     // 0 empty, 1 being written, 2 valid
    unsigned long long* c_key;
    azc::Pos* c_pos;
    float* c_value;
    int* c_n;
    float* c_pri;                          // [slots][MAX_EDGES]
    float* cached_value;                   // [G] value of a cache-served leaf
    unsigned long long* g_sims;            // [G] simulations backed up (summed at readout)
    unsigned long long* g_evals;           // [G] network rows of the persistent kernel (summed at readout)
    unsigned long long* g_sel_bytes;       // [G] algorithmic bytes read by k_select
    unsigned long long* trace;             // [G][8] s_memtime phase stamps of k_step (AZ_STEP_TRACE builds only)
    // evaluation log
    int log_cap, log_prior_cap;
    unsigned long long* log_key; float* log_value; int* log_off; int* log_n; int* log_idx; float* log_prior;
    // leaf-parallel search (az_search_cfg.leaves): K leaves per game per simulation step.  With K > 1 the
    // leaf records and cached_value are [G][K], the paths [G][K][PMAX], row_game / row_node / value [G K];
    // K = 1 is the layout above and runs the kernels above
    int K;
    int* leaf_src;                         // [G][K] LEAF_SHARED: the wave's leaf whose value this one takes
    // tree reuse (az_search_set_tree_reuse): k_finish keeps the played move's subtree and a
    // move's search tops the root up to S visits.  reuse = 0 is the search above, bit for bit
    int reuse;
    int* remap;                            // [G][NMAX] k_finish scratch: a node's id after the compaction, -1 = dropped
    uint32_t* remap_eb;                    // [G][NMAX] ... and its edge_begin after it
};

// ---------------- tree read-out (tree_read.hip: az_search_read_tree / az_search_read_pv) ----------------
static_assert(sizeof(az_tree_node) == 24 && sizeof(az_tree_edge) == 24, "tree export record layout");
static_assert(AZ_TREE_UNEXPANDED == CHILD_NONE && AZ_TREE_DRAW == CHILD_DRAW && AZ_TREE_WIN == CHILD_WIN,
              "the export's edge markers are the engine's");
struct TreeRead;          // a search's read-out scratch (device), made by its first tree_read
void tree_read_free(TreeRead* t);
// the work of az_search_read_tree on the trees of E, ordered after what `st` holds; complete on return
int tree_read(const Engine& E, hipStream_t st, TreeRead** scratch, const int32_t* games, int n, int min_visits,
              int max_depth, int64_t* node_off, int64_t* edge_off, az_tree_node* nodes, int64_t node_cap,
              az_tree_edge* edges, int64_t edge_cap, az_pos* states);
int tree_read_pv(const Engine& E, hipStream_t st, int32_t* moves, int cap, int32_t* len, float* q, uint32_t* visits);

// ---------------- network ----------------
struct NetDev {
    int blocks = 0, filters = 0, dtype = 0, device = 0;
    std::vector<void*> conv_w;      // swizzled MFMA fragments per conv (1 + 2*blocks)
    std::vector<float*> conv_b;     // folded bias per conv
    std::vector<size_t> conv_bytes; // allocation size of each conv_w (incl. the 8 zero k-steps of prefetch pad)
    std::vector<void*> wino_w;      // f32 F >= 64: Winograd-transformed residual conv weights (tower32w_kernel)
    std::vector<size_t> wino_bytes;
    bool winograd = AZ_WINOGRAD_DEFAULT != 0;   // tower32w_kernel for f32 F >= 64 nets (env AZ_WINOGRAD=0/1)
    // f32 nets the split16 level selects (wino16_selected): the same weights scaled by Sw (a power of
    // two per conv) and split into f16 hi / lo A-fragments of v_mfma_f32_16x16x32_f16 (wino.h
    // wino_core_h16), and each conv's 1 / (Sa Sw); built instead of wino_w (which then stays empty)
    std::vector<void*> wino16_w;
    std::vector<size_t> wino16_bytes;
    std::vector<float> wino16_us;
    int split16 = AZ_WINO_SPLIT16_DEFAULT;   // split-f16 point GEMMs in tower32w_kernel (env AZ_WINO_SPLIT16=0/1/2)
    bool wino_derive = AZ_WINO_DERIVE_DEFAULT != 0;   // env AZ_WINO_DERIVE=0/1 (wino16_streamed)
    int wino_streamed = 16;         // points per 32-channel group in wino16_w: 16, or 12 with row 2 derived
    bool wino_rows_env = AZ_WINO_ROWS_DEFAULT != 0;   // env AZ_WINO_ROWS=0/1 (wino16_rows)
    bool wino_rows = false;         // wino16_w holds the row-direct stream (winograd_split16_rows)
    bool wino_vrows_env = AZ_WINO_VROWS_DEFAULT != 0;   // env AZ_WINO_VROWS=0/1 (wino16_vrows)
    bool wino_vrows = false;        // the row-direct kernel keeps V in the shared-row layout
    int wino_boards_env = AZ_WINO_BOARDS_DEFAULT;       // env AZ_WINO_BOARDS=1/2 (wino16_boards)
    int wino_boards = 1;            // batch rows per workgroup of tower_forward's kernel
    // global ACT of the two-board tower (wino.h WINO_B2_WG bytes per workgroup): one allocation per stream
    // that launches it (an arena and a search may run one net on two streams), grown on demand under
    // b2_mu, freed with the net
    struct B2Act { void* p = nullptr; int wgs = 0; };
    std::map<hipStream_t, B2Act> b2_act;
    std::mutex b2_mu;
    float* head = nullptr;          // folded head weights (f32)
    void* head_frag = nullptr;      // 1x1 F->40 head conv as bf16 hi/lo MFMA A-fragments (fused tower)
    void* in_pk32 = nullptr;        // f32 Winograd nets: the input conv's weights with channels 16-18 of 4 taps packed per k-step (tower32w)
    size_t in_pk32_bytes = 0;
    void* head_frag32 = nullptr;    // the same conv as f32 A-fragments of v_mfma_f32_16x16x4_f32 (f32 fused tower)
    // AZ_DTYPE_FP8 (tower8.hip): the residual convs back to back as e4m3 A-fragments, their E8M0 scale
    // bytes and their folded biases [2*blocks][F]; conv_w / conv_b / conv_bytes hold the bf16 input conv only
    void* w8 = nullptr; void* w8s = nullptr; float* b8 = nullptr;
    size_t w8_bytes = 0, w8s_bytes = 0;
    size_t head_floats = 0;
    hipStream_t stream = nullptr;
    bool fused = true;              // use tower_forward when supported (AZ_FUSED_TOWER=0 disables)
    // scratch for az_net_forward
    void* x = nullptr; void* h = nullptr; void* planes = nullptr; int scratch_rows = 0;
    float* d_in = nullptr; float* d_pol = nullptr; float* d_val = nullptr; int io_rows = 0;
    // in-place updates (net_update.hip): 0 after net_create, + 1 per update; the searches compare it with
    // the generation their roots were set under.  upd: the device scratch of the update kernels (the flat
    // parameters of the last update among it), allocated by the first update
    int64_t generation = 0;
    struct NetUpdate* upd = nullptr;
};

// offsets inside NetDev::head
struct HeadLayout {
    size_t w40, b40, p2w, p2b, l1w, l1b, l2w, l2b, p2f, total;
    __host__ __device__ static HeadLayout make(int F) {
        HeadLayout L;
        L.w40 = 0;                      // [40][F]: policy_conv_1 (32) then value_conv (8), BN folded
        L.b40 = L.w40 + 40 * (size_t)F;
        L.p2w = L.b40 + 40;             // [64][32]
        L.p2b = L.p2w + 64 * 32;
        L.l1w = L.p2b + 64;             // [512][64]
        L.l1b = L.l1w + 512 * 64;
        L.l2w = L.l1b + 64;             // [64]
        L.l2b = L.l2w + 64;
        L.p2f = L.l2b + 4;              // p2w as MFMA A-fragments [cf 4][lane 64][8] (one 32-byte read per lane)
        L.total = L.p2f + 4 * 64 * 8;
        return L;
    }
};

// search-mode output target of the heads / synthetic evaluator
struct SearchOut {
    const Node* nodes; Edge* edges; int NMAX, EMAX;
    const int* row_game; const int* row_node;
    float* value;
    // eval log (may be disabled: log_cap == 0)
    int log_cap, log_prior_cap;
    unsigned long long* log_key; float* log_value; int* log_off; int* log_n; int* log_idx; float* log_prior;
    Counters* ctr;
    const azc::Pos* npos;
};

int net_create(const az_net_desc* d, const float* w, size_t n, int device, NetDev** out);
void net_destroy(NetDev* n);
// net_update.hip: rewrite every weight buffer of n in place from the flat parameters d_w (device, n's
// device), byte for byte what net_create builds from them; ordered after st, returns when done
int net_update_device(NetDev* n, const float* d_w, size_t count, hipStream_t st);
void net_update_free(NetDev* n);
// planes [rows][64][32] in the net's dtype (device). count may be nullptr (all rows valid).
// ev0/ev1 (optional) bracket the first residual conv launch (timing of one 3x3 FxF conv)
int net_tower(NetDev* n, const void* planes, const int* count, int rows, void* x, void* h, hipStream_t st,
              hipEvent_t ev0, hipEvent_t ev1);
int net_heads_dense(NetDev* n, const void* x, int rows, float* policy, float* value, hipStream_t st);
int net_heads_search(NetDev* n, const void* x, const int* count, int rows, const SearchOut& so, hipStream_t st);
int net_encode_rows(NetDev* n, const azc::Pos* npos, int NMAX, const int* row_game, const int* row_node,
                    const int* count, int rows, void* planes, hipStream_t st);
int synth_eval_rows(const int* count, int rows, const SearchOut& so, hipStream_t st);
int net_planes_from_host_layout(NetDev* n, const float* d_in, int rows, void* planes, hipStream_t st);
// fused tower (tower.hip): input conv + residual tower + heads in one launch (bf16 and f32).
bool tower_supported(const NetDev* n);
bool wino_supported(const NetDev* n);   // f32, F >= 64, Winograd weights built: tower32w_kernel
bool wino_split16(const NetDev* n);     // ... with split-f16 MFMA products (wino16_selected)
// az_wino16_pack (net.hip winograd_split16 on the host): the u16 count, or < 0
int wino16_pack(const float* wf, int F, int streamed, uint16_t* out, size_t cap, float* unscale);
// az_wino16_pack_rows (net.hip winograd_split16_rows): the same for the row-direct stream, F = 256
int wino16_pack_rows(const float* wf, int F, uint16_t* out, size_t cap, float* unscale);
// persistent per-game simulation kernel (tower.hip, k_sims32w): simulation steps [step0, step1) of
// every game, tree steps and Winograd evaluations in one workgroup per game, all backed up at the end
bool sims_persistent_supported(const NetDev* n);
int sims_persistent(const NetDev* n, const Engine& E, const SearchOut& so, int step0, int step1, hipStream_t st);
int tower_forward(NetDev* n, const void* planes, const int* count, int rows, float* pol, float* val,
                  const SearchOut* so, hipStream_t st);
// MX-fp8 tower (tower8.hip): the same launch contract as tower_forward, for AZ_DTYPE_FP8 nets
int tower8_forward(NetDev* n, const void* planes, const int* count, int rows, float* pol, float* val,
                   const SearchOut* so, hipStream_t st);
// one BatchNorm-folded residual conv wf [co][ci][9], quantised by az_mx8_quantize per (co, tap, 32 ci)
// and appended as fragments to the host copies of NetDev::w8 / w8s
void mx8_append_conv(const std::vector<float>& wf, int F, std::vector<uint8_t>* w8, std::vector<uint8_t>* w8s);
size_t act_bytes(int dtype);
double net_flop_per_eval(int blocks, int filters);
double net_tower_flop_per_eval(int blocks, int filters);

}  // namespace azi

struct az_net { azi::NetDev* dev; };

namespace azi {
// search.hip: az_search_run with the improved policy left in device memory, d_improved [games][4096] on
// the search's device -- the simulations of the roots just set, then k_readout.  Complete on return.
// *evals (may be nullptr): the network rows the search has evaluated since it was created
int search_run_device(az_search* s, float* d_improved, unsigned long long* evals);

// The same search in parts, for a caller that sets the roots with a kernel of its own and runs several
// searches side by side (arena.hip).  Where a search's root records live and the stream its work runs on:
struct SearchRoots {
    int slots;                             // az_search_cfg.games
    azc::Pos* hist; int* hist_len;         // [slots][HMAX], [slots]: Engine::hist / hist_len
    int* game_id; int* ply; int* active;   // [slots]
    hipStream_t st;
};
int search_roots(az_search* s, SearchRoots* out);
// after the caller's launches on SearchRoots::st have written every slot's records: what
// az_search_set_roots_from(.., apply_noise = 0) does behind its upload (k_root_setup, the root evaluation,
// k_root_noise(0)), queued on that stream with no host synchronise.  AZ_EVAL_NET / AZ_EVAL_SYNTHETIC only
int search_set_roots_device(az_search* s);
// search_run_device's launches: the simulations, k_readout into d_improved, then `done` recorded on the
// search's stream
int search_launch_device(az_search* s, float* d_improved, hipEvent_t done);
// ... and its read-back of `evals`; waits for the search's stream
int search_finish_device(az_search* s, unsigned long long* evals);
}  // namespace azi
