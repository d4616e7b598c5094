/*
 * az.h -- C-ABI of the MI355X-native alphazero-chess self-play engine (libaz.so).
 *
 * Drop-in boundary for the reference's hot path (AlexandreGac/alphazero-chess @ 2025-08-24).
 * The reference is a single Rust crate with no FFI; each entry point below replaces one
 * item of its module surface (file:line cited) and is what a Rust `extern "C"` block
 * would bind (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions: every function returns int status (0 = ok, <0 = error; message via
 * az_last_error()) unless noted.  Plain pointers and sizes only.  Host buffers are
 * caller-owned; the engine owns all device memory.  A handle is used by one host thread
 * at a time (not re-entrant); one handle per GPU.
 * Squares: a1 = 0 ... h8 = 63 (shakmaty Square order).  Move indices: 0..4095 =
 * plane*64 + rank'*8 + file (chess.rs:73-116), rank' flipped for Black.
 */
#ifndef AZ_H
#define AZ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_ACTION_SPACE 4096   /* parameters.rs:3 */
#define AZ_PLANES 19           /* chess.rs:191-245 */
#define AZ_MAX_MOVES 256

/* Result codes of play (chess.rs:29-34 GameResult, plus -1 = Err("Illegal move")) */
enum { AZ_ONGOING = 0, AZ_DRAW = 1, AZ_WHITE_WINS = 2, AZ_BLACK_WINS = 3, AZ_ILLEGAL = -1 };

/* Packed position (80 bytes) -- the engine's replacement for shakmaty::Chess.
 * bb: P N B R Q K (both colours), white, black.  ep: pseudo-legal en-passant square
 * (shakmaty pseudo_legal_ep_square, chess.rs:218) or 64.  flags bit0: that ep capture is
 * also legal (shakmaty Chess equality uses the legal ep square).  castling bits:
 * 1 = White O-O, 2 = White O-O-O, 4 = Black O-O, 8 = Black O-O-O.
 * rep_key: hash of (board, turn, castling, legal ep) -- the repetition key. */
typedef struct az_pos {
    uint64_t bb[8];
    uint8_t turn, castling, ep, flags;
    uint16_t halfmoves, fullmoves;
    uint64_t rep_key;
} az_pos;

const char* az_last_error(void);
int az_version(void);
int az_device_count(int* n);
int az_device_synchronize(int device);                              /* hipDeviceSynchronize on `device` */

/* ---- rules & codec: chess.rs ---------------------------------------------------- */
int az_pos_startpos(az_pos* out);                                   /* Chess::new, chess.rs:21 */
int az_pos_from_fen(const char* fen, az_pos* out);
int az_pos_to_fen(const az_pos* p, char* buf, int cap);            /* Fen::from_position(.., PseudoLegal) */
uint64_t az_pos_fen_key(const az_pos* p);                           /* cache key, tree.rs:214 */
/* legal move indices in shakmaty legal_moves() order WITH duplicates for
 * under-promotions, exactly MCTree::new's `moves` (tree.rs:86-89). Returns count. */
int az_pos_legal_indices(const az_pos* p, int32_t* out, int cap);
/* index_to_move (chess.rs:118-171) + play_unchecked: returns 1 and writes the child
 * position if the index names a legal move, 0 otherwise. */
int az_pos_play_index(const az_pos* p, int32_t index, az_pos* child);
int az_move_to_index(int from, int to, int turn);                   /* chess.rs:73-116 */
/* outcome(): AZ_ONGOING, AZ_DRAW (stalemate / insufficient material), AZ_WHITE/BLACK_WINS */
int az_pos_outcome(const az_pos* p);
int az_pos_encode(const az_pos* p, float* out);                     /* to_tensor, chess.rs:191-245: 19*64 f32 */

/* GameState = position + repetition multiset (chess.rs:13-27) */
typedef struct az_game az_game;
int az_game_create(az_game** out);                                  /* GameState::new, chess.rs:20 */
int az_game_clone(const az_game* g, az_game** out);
int az_game_destroy(az_game* g);
int az_game_position(const az_game* g, az_pos* out);
int az_game_history(const az_game* g, int32_t* moves, int cap);     /* indices played so far; returns count */
/* play_move(state, index_to_move(index)) (chess.rs:36-63): AZ_ONGOING / AZ_DRAW /
 * AZ_WHITE_WINS / AZ_BLACK_WINS / AZ_ILLEGAL */
int az_game_play(az_game* g, int32_t index);

/* ---- network: agent.rs AlphaZero ------------------------------------------------- */
/* AZ_DTYPE_FP8: the opt-in MX-fp8 mode (OCP MX, e4m3fn elements with one E8M0 scale per 32 channels on
 * the residual convs; 128 or 256 filters, fused tower only; README "Precision"). */
enum { AZ_DTYPE_F32 = 0, AZ_DTYPE_BF16 = 1, AZ_DTYPE_FP8 = 2 };
typedef struct { int blocks, filters, dtype; } az_net_desc;
typedef struct az_net az_net;
/* number of f32 parameters in the flat layout (see DESIGN.md "Weights"): burn module
 * order, conv [out,in,kh,kw], BatchNorm {gamma,beta,running_mean,running_var},
 * Linear weight [d_in,d_out] (burn layout). */
size_t az_net_num_params(int blocks, int filters);
/* AlphaZero::new + load_record (agent.rs:49-110, main.rs:109-116): weights copied to HBM,
 * BatchNorm folded into the convs (inference mode, model.valid()). */
int az_net_create(const az_net_desc* desc, const float* weights, size_t n, int device, az_net** out);
int az_net_destroy(az_net* net);
/* name of the kernel(s) that evaluate this net (fused f32 Winograd / f32 direct / bf16 / MX-fp8 / per-layer) */
int az_net_tower_kernel(az_net* net, char* out, int cap);
/* Winograd points whose weights the split-f16 tower streams per 32 input channels: 16, or 12 where the
 * kernel derives the third row of points from the other three (AZ_WINO_DERIVE, 256 filters); 0 for a
 * net that another kernel evaluates */
int az_net_wino_streamed_points(az_net* net);
/* Winograd-domain accumulators per output fragment of the split-f16 tower: 16 (all 16 points, streamed
 * or derived), or 8 where the kernel is Winograd across columns only and sums the three tap rows
 * directly (AZ_WINO_ROWS, 256 filters, 12 streamed planes); 0 for a net that another kernel evaluates */
int az_net_wino_accumulators(az_net* net);
/* 1 where the row-direct split-f16 tower keeps its transformed input with every row of the padded board
 * stored once (AZ_WINO_VROWS, only where az_net_wino_accumulators is 8), 0 otherwise */
int az_net_wino_v_rows(az_net* net);
/* batch rows per workgroup of the kernel that evaluates this net's batches: 2 where the shared-row tower
 * runs two boards on one weight stream with its activations in global memory (AZ_WINO_BOARDS=2, only
 * where az_net_wino_v_rows is 1), 1 for every other form of the split-f16 tower, 0 for a net that another
 * kernel evaluates */
int az_net_wino_boards(az_net* net);
/* The two-board tower's layout, tabulated from the constants and address functions the kernel uses
 * (wino.h wino_b2_*, wino_vr_*), byte offsets: item[wave][k] = {board, wave-item} of the wave's k-th
 * transform item of a chunk, or -1 past the wave's last item (8 x 8 x 2); act[board][buffer] of the board's X (0) and H (1) within the
 * workgroup's global activations (2 x 2); out[wave][lane][n][q] of the lane's epilogue access (output
 * fragment n, square q of its tile) within a buffer (8 x 64 x 2 x 4, 16 bytes each); vbuf[board][buf] of
 * the V buffers in LDS (2 x 2); zero[k] of the 64 runs of 256 B that are the off-board rows; dims =
 * {buffer bytes, global bytes per workgroup, V buffer bytes, LDS ACT overlay offset, LDS ACT overlay
 * bytes, AUX offset, AUX bytes, total LDS bytes}.  Needs no device. */
int az_wino_boards_layout(int* item, int* act, int* out, int* vbuf, int* zero, int* dims);
/* The shared-row V layout's address functions, tabulated from the formulas the kernel uses (wino.h
 * wino_vr_*), byte offsets: write[q][lane][b] of wave-item q (16 per chunk), point b within a chunk's V
 * buffer (16 x 64 x 4); read[plane][i][b][lane] of patch row i, point b in the hi and the lo plane
 * (2 x 4 x 4 x 64); act[q][lane][j] of the item's read of column j within the layer input (16 x 64 x 4,
 * chunk 0); item[sched][wave][it]
 * the wave-item of transform wave `wave`, or -1 (2 x 8 x 4: sched 0 waves 0-3 x 4 items, 1 eight waves
 * x 2); dims = {plane bytes, buffer bytes, ACT square stride, ACT channel bytes}.  Needs no device. */
int az_wino_vrows_layout(int* write, int* read, int* act, int* item, int* dims);
/* burn NamedMpkFileRecorder<FullPrecisionSettings> model files:
 * load_model (main.rs:109-116) -> flat weights for az_net_create / az_trainer_create, and
 * model.save_file (training.rs:269-270) from flat weights.  out/w hold az_net_num_params floats. */
int az_net_load_mpk(const char* path, int blocks, int filters, float* out, size_t n);
int az_net_save_mpk(const char* path, int blocks, int filters, const float* w, size_t n);
/* AlphaZero::forward (agent.rs:112-144): planes [n,19,8,8] f32 -> policy [n,4096]
 * (softmax) and value [n] (tanh). Host buffers. */
int az_net_forward(az_net* net, const float* planes, int n, float* policy, float* value);
/* Same on device pointers / a caller's hipStream_t (NULL = engine stream). */
int az_net_forward_device(az_net* net, const float* d_planes, int n, float* d_policy, float* d_value,
                          void* stream);
/* model.valid() without leaving the device (training.rs:83): rewrite every weight buffer of an existing
 * net in place -- BatchNorm fold and all packed layouts, by HIP kernels (net_update.hip) -- from flat f32
 * parameters (az_net_num_params layout) that are already in HBM on the net's device.  The buffers keep
 * their addresses and sizes, and the result is byte for byte what az_net_create builds from the same
 * parameters.  The work is ordered after what `stream` holds (NULL = the net's stream); the call returns
 * when the new weights are in place.  n must be the net's parameter count, else an error and no change.
 * No search may be running on the net; a search whose roots were set before the update must set roots
 * (or az_selfplay_reset) again before it runs, or adopt the new weights between two moves
 * (az_search_adopt_net / az_selfplay_adopt_net), which keeps its games. */
int az_net_update_device(az_net* net, const float* d_weights, size_t n, void* stream);
/* the same from host weights: one upload, then the device path (a checkpoint, an arena opponent) */
int az_net_update(az_net* net, const float* weights, size_t n);
/* 0 after az_net_create, + 1 for each successful update */
int64_t az_net_generation(az_net* net);
/* the flat parameters of the last update (the net keeps a device copy from its first update on); an error
 * for a net that was never updated (its creator holds those weights) */
int az_net_get_weights(az_net* net, float* out, size_t n);
/* Test hook: copy one packed weight buffer of the net to the host; returns its size in bytes (out NULL:
 * the size alone), 0 for a buffer this net does not hold, < 0 on error (cap too small).  index = the conv
 * (0 = input conv) for AZ_PACKED_CONV_W / CONV_B, the residual conv (0 .. 2 blocks - 1) for WINO_W /
 * WINO16_W / WINO16_US (the conv's 1 / (Sa Sw), 4 bytes), 0 otherwise. */
enum {
    AZ_PACKED_CONV_W = 0, AZ_PACKED_CONV_B = 1, AZ_PACKED_IN_PK32 = 2, AZ_PACKED_WINO_W = 3, AZ_PACKED_WINO16_W = 4,
    AZ_PACKED_WINO16_US = 5, AZ_PACKED_W8 = 6, AZ_PACKED_W8S = 7, AZ_PACKED_B8 = 8, AZ_PACKED_HEAD = 9,
    AZ_PACKED_HEAD_FRAG = 10, AZ_PACKED_HEAD_FRAG32 = 11, AZ_PACKED_KINDS = 12
};
int az_net_packed_read(az_net* net, int kind, int index, void* out, size_t cap);

/* ---- search: tree.rs MCTree + training.rs self-play driver ------------------------ */
/* AZ_EVAL_NET: the engine's own az_net (fused HIP tower).  AZ_EVAL_SYNTHETIC: the hash evaluator
 * the oracle shares (parity tests).  AZ_EVAL_CALLBACK: a caller-owned evaluator installed with
 * az_search_set_evaluator -- the reference's InferenceRequest / process_batch boundary
 * (training.rs:28-31, 380-422; tree.rs:222-228), e.g. a Rust caller keeping its burn model. */
enum { AZ_EVAL_NET = 0, AZ_EVAL_SYNTHETIC = 1, AZ_EVAL_CALLBACK = 2 };
/* Caller-owned evaluator: called on the calling thread of az_search_set_roots / az_search_run /
 * az_selfplay_* once per simulation step with the n leaf positions that need an evaluation (every
 * game's pending InferenceRequest of that step, in batch-row order).  It fills policy[n * 4096]
 * (AlphaZero::forward's softmax row, agent.rs:128-130: the engine reads it at the legal move
 * indices only) and value[n] (side-to-move view, tanh output).  The rows must be what the
 * reference's forward gives: finite, non-negative, a softmax over the 4096 entries -- the engine
 * takes the legal entries as priors unchecked (PUCT of a NaN prior never wins a selection).
 * Return 0 on success; a non-zero return aborts the search call with an error.  Buffers are
 * engine-owned and valid for the call. */
typedef int (*az_eval_fn)(void* ctx, const az_pos* positions, int n, float* policy, float* value);
typedef struct {
    int games;          /* concurrent games G on this GPU (NUM_EPISODES, parameters.rs:13) */
    int sims;           /* simulations per move (NUM_SIMULATIONS, parameters.rs:32) */
    float c_puct;       /* parameters.rs:34 */
    float dir_alpha;    /* parameters.rs:28.  A row of gamma draws whose f32 sum is 0, or so small that 1/sum
                         * is not finite (dir_alpha < 1 only: every draw underflows through u^(1/alpha), as
                         * 1 in 200 two-move roots do at 0.03), is normalised in the log domain from the same
                         * draws and is a finite distribution; rand_distr yields a NaN row there.  Every other
                         * row is g_i * (1/sum g) as in rand_distr */
    float dir_eps;      /* parameters.rs:29 */
    int temp_moves;     /* TEMPERATURE_ANNEALING, parameters.rs:31 */
    int noise;          /* Dirichlet noise at roots (training.rs:358, tree.rs:243) */
    uint64_t seed;      /* counter-based RNG seed (replaces thread_rng) */
    int evaluator;      /* AZ_EVAL_NET, AZ_EVAL_SYNTHETIC or AZ_EVAL_CALLBACK */
    int continuous;     /* self-play: restart a finished slot with a new game.  Game ids: slots
                           start with ids 0..games-1; new ids are handed out in finishing
                           order, starting at `games`.  Games that end in the same step get
                           consecutive ids in no defined slot order (it can differ from run to
                           run).  A game's content (noise, move choice: the streams keyed by
                           seed, game id, ply) depends on its id only, never on the slot.
                           Restarted slots copy a start-position template evaluated at
                           az_selfplay_reset; az_selfplay_adopt_net evaluates it again after a
                           weight update. */
    int record_evals;   /* keep a log of every evaluation (for replay parity) */
    int eval_log_cap;   /* log capacity in rows */
    int cache_capacity; /* FEN evaluation cache entries (CACHE_CAPACITY, parameters.rs:4; 0 = off):
                           tree.rs:214-219 lookup, training.rs:413 insert.  Changes only how many
                           network rows run, never a result. */
    int leaves;         /* leaf-parallel search: leaves per game per simulation step, K in 1..8 (0 = 1, the
                           default: today's search, bit for bit).  With K > 1 a move's `sims` simulations run
                           in waves of up to K per game: the K leaves of a wave are selected on the same tree,
                           each seeing the earlier ones as visits that lost (virtual loss 1, in the selection
                           only), expanded and evaluated in one batch of up to games * K rows, then backed
                           up in order -- ceil(sims / K) steps a move.  A leaf that ends on the edge an
                           earlier leaf of its wave expands shares that leaf's value (az_search_leaf_stats).
                           Results differ from K = 1 and, with az_selfplay_run_sims, depend on how a move is
                           cut into calls: every call starts a new wave.  Lands in the former tail padding:
                           sizeof(az_search_cfg) stays 64. */
} az_search_cfg;
typedef struct az_search az_search;

int az_search_default_cfg(az_search_cfg* cfg);   /* reference defaults (parameters.rs) */
int az_search_create(az_net* net, const az_search_cfg* cfg, int device, az_search** out);
int az_search_destroy(az_search* s);
/* Install the AZ_EVAL_CALLBACK evaluator (cfg.evaluator must be AZ_EVAL_CALLBACK); replaces
 * process_batch (training.rs:380-422).  Must precede the first az_search_set_roots /
 * az_selfplay_reset. */
int az_search_set_evaluator(az_search* s, az_eval_fn fn, void* ctx);

/* Roots from histories: game g's root = startpos + hist[off[g]..off[g+1]) (move indices),
 * evaluated and optionally noised: MCTree::new(policy, state, apply_noise), tree.rs:84-104.
 * noise_ply[g] (may be NULL = 0) selects the RNG stream (seed, game_id[g], ply).  Abandons a
 * self-play move left in progress by az_selfplay_run_sims (its simulations are discarded). */
int az_search_set_roots(az_search* s, const int32_t* hist, const int32_t* off, const int32_t* game_id,
                        const int32_t* noise_ply, int apply_noise);
/* The same from arbitrary states, MCTree::new(policy, state, apply_noise) with any GameState
 * (tree.rs:84-104): game g's state starts at start[g] (NULL = startpos for every game; its
 * repetition multiset holds start[g] once) and plays hist[off[g]..off[g+1]) through play_move, so
 * the root is the last position and every earlier one counts toward threefold (chess.rs:52-60). */
int az_search_set_roots_from(az_search* s, const az_pos* start, const int32_t* hist, const int32_t* off,
                             const int32_t* game_id, const int32_t* noise_ply, int apply_noise);
/* monte_carlo_tree_search for every game (tree.rs:106-115 / 169-178).  Outputs (any may
 * be NULL): improved policy [G,4096], visits [G,4096], max_subtree_depth [G]. */
int az_search_run(az_search* s, float* improved, uint32_t* visits, int32_t* depth);
/* The current roots' visits / improved policy / max_subtree_depth without running simulations:
 * the reference's public MCTree fields (tree.rs:25-34), e.g. mid-move during az_selfplay_run_sims:
 * after k simulations of a move the outputs are exactly the tree after those k (every one backed
 * up, none counted twice), and reading changes nothing.  A root that no simulation has visited
 * yet (right after az_search_set_roots, az_search_advance or a completed self-play move) reads
 * visits all 0 and depth 0; its improved policy is 0 / 0: NaN at the indices of the root's legal
 * moves and 0 everywhere else (bench.py --dump-outputs reads the roots' legal moves off it). */
int az_search_read_roots(az_search* s, float* improved, uint32_t* visits, int32_t* depth);

/* Whole search trees, read from the device: the reference's public MCTree (tree.rs:25-34: nodes, moves, state,
 * policy, visits, scores at every node) as compact CSR records.
 * az_tree_edge.child is the child node's ordinal within its game, or one of: */
enum {
    AZ_TREE_UNEXPANDED = -1,   /* no simulation has taken the move yet */
    AZ_TREE_DRAW = -2,         /* the move ends the game in a draw */
    AZ_TREE_WIN = -3,          /* the move wins the game for the side that plays it */
    AZ_TREE_CUT = -4           /* the move has a child node that min_visits / max_depth left out */
};
typedef struct {
    int32_t parent;            /* ordinal of the parent node within the game, -1 at the root */
    int32_t parent_edge;       /* which of the parent's edges leads here (0 .. parent.nedges - 1), -1 at the root */
    int32_t edge_begin;        /* the node's edges: [edge_begin, edge_begin + nedges) of the game's edges */
    int32_t nedges;
    int32_t depth;             /* root = 0 */
    uint32_t nsum;             /* visits summed over the node's edges */
} az_tree_node;                /* 24 B */
typedef struct {
    float prior;               /* policy[index] (with the Dirichlet noise at a noised root) */
    float score;               /* scores[index]: the backed-up values' sum; Q = score / visits */
    uint32_t visits;           /* visits[index] */
    int32_t index;             /* the move index, 0..4095 */
    int32_t child;             /* ordinal of the child node within the game, or AZ_TREE_* */
    uint32_t flags;            /* bit 0: the index stands for the four promotion entries of `moves` */
} az_tree_edge;                /* 24 B */
/* The trees of the n slots listed in `games` (NULL: all cfg.games slots in slot order, n is ignored; a slot
 * may repeat and is then exported once per mention).  CSR: game k's nodes are nodes[node_off[k] ..
 * node_off[k+1]) and its edges edges[edge_off[k] .. edge_off[k+1]); node_off and edge_off have n + 1
 * entries; parent, edge_begin and child are relative to the game's own ranges.  Node 0 is the root.  Nodes
 * come in ascending engine id -- creation order, the order the tree-reuse compaction keeps -- so every
 * node's parent has a smaller ordinal.  A node's edges are all of its edges in the order the selection scans
 * them: the distinct move indices by first appearance in legal_moves() order.  states (may be NULL): one
 * az_pos per exported node, in node order, flags and rep_key as the engine holds them.
 * Pruning: a child node is exported only if its parent is, its edge has visits >= min_visits and its depth
 * is <= max_depth (max_depth < 0: no limit).  An edge whose existing child node was left out reads
 * AZ_TREE_CUT, and nothing below it is exported.  min_visits = 0, max_depth = -1 is the whole tree;
 * max_depth = 0 the roots alone with every edge (the reference's root policy / visits / scores / moves).
 * nodes == NULL && edges == NULL fills node_off / edge_off only, for sizing (states is then ignored).
 * Refused with an error, nothing written to any output: a slot outside 0 .. cfg.games - 1, n < 0,
 * min_visits < 0, NULL offsets, node_cap / edge_cap smaller than needed, one of nodes / edges NULL but not
 * the other.
 * May be called wherever az_search_read_roots may, mid-move after az_selfplay_run_sims included: the tree
 * is the tree after the simulations run so far, every one backed up and none counted twice, in every form of
 * the search (both step forms, the persistent kernel, leaves > 1, tree reuse).  Reading changes nothing.
 * An inactive game exports what its arena holds: the tree it had when it went inactive.  The first call
 * allocates the device scratch (12 B per node slot of the arena); a handle that never reads a tree pays
 * nothing. */
int az_search_read_tree(az_search* s, const int32_t* games, int n, int min_visits, int max_depth,
                        int64_t* node_off, int64_t* edge_off,
                        az_tree_node* nodes, int64_t node_cap,
                        az_tree_edge* edges, int64_t edge_cap, az_pos* states);
/* The principal variation of every slot: moves[g * cap .. g * cap + len[g]).  From the root it takes the
 * most visited edge, ties to the larger move index (max_by's last maximum, the rule of self-play's move
 * choice, training.rs:310-317), and descends while that edge has a child node; the last move may sit on an
 * unexpanded or game-ending edge.  It stops before an edge with 0 visits, and at cap.  q[g]: the first
 * move's score / visits in f32 (0 for an empty PV); visits[g]: the first move's visits.  len, q, visits may
 * each be NULL; moves may be NULL only with cap = 0.  Callable wherever az_search_read_tree is. */
int az_search_read_pv(az_search* s, int32_t* moves, int cap, int32_t* len, float* q, uint32_t* visits);

/* traverse_new(action, apply_noise) for every game (tree.rs:239-256) after playing the
 * action on its GameState (training.rs:323-325).  result[g] receives the play_move result:
 *   AZ_ONGOING: the game goes on.  Its root is now the action's child: the child's priors are kept,
 *     its visits and scores are zeroed and every other node is dropped, so the next az_search_run
 *     equals a fresh search of the extended history.  With apply_noise the new root gets Dirichlet
 *     noise from the stream (seed, game_id, ply + 1, 0), ply being the noise ply of the root left
 *     behind (az_search_set_roots' noise_ply; each advance adds one).
 *   AZ_DRAW / AZ_WHITE_WINS / AZ_BLACK_WINS: the move ends the game (mate, stalemate, insufficient
 *     material, threefold repetition, the 50-move or the 200-fullmove limit).
 *   AZ_ILLEGAL: actions[g] is not the index of a legal move of the root (anything outside
 *     0..4095 included), or it is a legal move that no simulation has expanded -- the engine keeps
 *     no child to re-root on (the reference's traverse_new panics there); also the answer for a
 *     game that was inactive already.
 * Every game whose result is not AZ_ONGOING becomes inactive until the next az_search_set_roots:
 * az_search_run runs no simulation for it (none is counted in az_search_stats), az_search_advance
 * ignores its action, and az_search_run / az_search_read_roots keep returning the visits, improved
 * policy and depth its root had when it went inactive. */
int az_search_advance(az_search* s, const int32_t* actions, int apply_noise, int32_t* result);

/* run_all_episodes (training.rs:340-378): reset all G slots to new games from startpos */
int az_selfplay_reset(az_search* s);
/* one move for every active game: sims, improved policy, action choice (training.rs:310-321),
 * play, traverse/record.  *finished = games that ended in this step. */
int az_selfplay_step(az_search* s, int* finished, int* active);
/* The same move in pieces: the next `nsims` simulation steps of every game's current move
 * (async_monte_carlo_tree_search's loop, tree.rs:169-178, cut at any simulation boundary).
 * When the move's sims are complete (*move_done = 1) the action choice, play and re-root of
 * az_selfplay_step follow; until then *finished = 0, *active = -1.  Results are identical to
 * az_selfplay_step. */
int az_selfplay_run_sims(az_search* s, int nsims, int* finished, int* active, int* move_done);

/* EpisodeStep (training.rs:15-20) of finished games, drained in game order. */
typedef struct {
    int32_t game_id;
    int32_t ply;
    int32_t action;
    int32_t search_depth;
    float final_value;         /* training.rs:332-335 */
    int32_t result;            /* AZ_DRAW / AZ_WHITE_WINS / AZ_BLACK_WINS */
    int32_t nvis;              /* improved_policy = visits / sum(visits) over these entries */
    az_pos state;
    uint16_t vis_idx[224];
    uint16_t vis_n[224];
} az_episode_step;
int az_selfplay_drain(az_search* s, az_episode_step* out, int cap);   /* returns count */

/* Adopt the evaluator's current weights in a live search, between moves (after az_net_update* on the
 * search's net, or when a caller-owned evaluator's model changed).  Afterwards every active game is in
 * exactly the state az_search_set_roots would produce from that game's history on the updated evaluator
 * (start position + the moves so far, the game's id, noise_ply = its ply, the same apply_noise): the root
 * is evaluated again, its edges hold the new priors with zero visits and scores, and with noise on the
 * Dirichlet noise comes from the stream (seed, game id, ply, 0) on the new priors.  The repetition
 * history, game id, ply, slot and the steps recorded so far stay; inactive games are not touched (they keep
 * returning the visits they had); the FEN cache is emptied.  With cfg.continuous the start-position
 * template a restarted slot is built from is evaluated again too, so a game that starts after the call
 * equals one played wholly on the new weights.  A game's plies before the call are the old weights', those
 * from the call on equal a fresh search of their history on the new ones; with an evaluator that did not
 * change the call is invisible in every result.  No history is uploaded: the state is rebuilt in HBM.
 * AZ_EVAL_NET: 0 and no work when the net's generation has not moved since the roots were last set or
 * adopted.  AZ_EVAL_CALLBACK / AZ_EVAL_SYNTHETIC: there is no generation, the call always re-evaluates.
 * The rows it evaluates (one per active game, one for the template) are counted in az_search_stats.evals.
 * Refused with an error and no change while a move is in progress (az_selfplay_run_sims).
 * az_selfplay_adopt_net: for handles driven by az_selfplay_*, noise as cfg.noise.
 * az_search_adopt_net: for set_roots / run / advance; the next az_search_run is valid. */
int az_selfplay_adopt_net(az_search* s);
int az_search_adopt_net(az_search* s, int apply_noise);
/* The games now in the slots (logging, checkpoints): per slot the game's id, ply and active flag, read from
 * the device, and the moves it has played so far (the recorded steps of the self-play driver) as CSR --
 * game g's moves are moves[off[g]..off[g+1]), off has games + 1 entries; an inactive slot has none.  Any
 * output may be NULL.  Returns the total move count; with moves == NULL that is all it needs `cap` for,
 * otherwise an error when cap is smaller. */
int az_selfplay_inflight(az_search* s, int32_t* game_id, int32_t* ply, int32_t* active, int32_t* moves, int32_t* off,
                         int cap);

typedef struct {
    int64_t sims;              /* simulations completed */
    int64_t evals;             /* network rows evaluated */
    int64_t terminal_leaves;
    int64_t games_finished;
    int64_t moves;
    int64_t max_depth_sum;     /* sum over moves of max_subtree_depth */
    int64_t cache_hits;        /* expansions served by the FEN cache (CACHE_HITS, training.rs:12) */
    int64_t cache_misses;      /* expansions that needed a network row (CACHE_MISSES) */
    int64_t overflow;          /* expansions refused for want of node/edge arena space (0 by construction) */
    int64_t max_nodes;         /* largest node count of any game's current tree (arena: sims + 2) */
    int64_t max_edges;         /* largest edge count of any game's current tree */
    int64_t node_cap, edge_cap;/* the per-game arena sizes */
} az_search_stats;
int az_search_stats_get(az_search* s, az_search_stats* out);
/* 1 if the untimed simulation steps run through the persistent per-game kernel (k_sims32w: a
 * game's backup / select / expand and its Winograd f32 evaluation in one workgroup, no grid-wide
 * step boundary; chosen when the games fit the device in one round, the net is f32 Winograd (or the
 * bf16 64-filter tower) and
 * the FEN cache is off; env AZ_PERSIST=0/1 forces it), 0 if they run as k_step + the batched
 * tower.  Either way the results are identical (tests/test_gpu_search.py). */
int az_search_persistent(az_search* s);
/* Leaf-parallel search: *leaves = the K in effect (1 for cfg.leaves 0 or 1), *shared_leaves = the
 * simulations whose leaf shared the expansion of an earlier leaf of its wave (always 0 at K = 1), counted
 * like az_search_stats: since creation or the last az_selfplay_reset, which clears every counter.  Either
 * may be NULL.  Beside az_search_stats: sims == evals + cache_hits + terminal_leaves + shared_leaves + the
 * simulations whose selection ended on an edge already known to end the game -- terminal_leaves counts an
 * ended game once, when an expansion finds it, at every K; the later visits of that edge are in `sims`
 * only.  az_search_persistent is 0 at K > 1.  With tree reuse (az_search_set_tree_reuse) the identity
 * holds as it stands: `sims` counts the simulations run (backed up), not cfg.sims per move -- a move on a
 * root that carried c visits runs cfg.sims - c -- and the carried visits are in no counter but
 * az_search_reuse_stats' carried_visits. */
int az_search_leaf_stats(az_search* s, int* leaves, uint64_t* shared_leaves);

/* Tree reuse (opt-in; off: every re-root starts from an empty tree, the reference's traverse_new,
 * tree.rs:239-256, bit for bit).  With on = 1 a re-root on a played move that has a child node -- in
 * az_selfplay_step / az_selfplay_run_sims and in az_search_advance -- keeps that child's subtree: the child
 * becomes the root with its edges' priors, scores, visits and children as they are, every node below it
 * stays, everything else is dropped, depths are rebased (the root's is 0, the reported search depth is the
 * largest rebased depth kept).  Root noise (apply_noise) goes onto the kept priors from the same stream
 * (seed, game id, ply, 0).  A move's search then tops the root up: game g runs cfg.sims - (the root's
 * visits) >= 1 simulations, so its root's visits sum to exactly cfg.sims when the move ends, and the
 * improved policy, the move choice and the EpisodeStep come from those visits as before.  az_search_run
 * likewise runs cfg.sims - visits per game, none for a root already there.  A call runs as many simulation
 * steps as the neediest active game asks; a game that is done takes no leaf, writes no row and moves no
 * counter.  az_selfplay_run_sims sets *move_done when every active root holds cfg.sims visits.  Fresh roots
 * (az_search_set_roots*, az_selfplay_reset, a restarted continuous slot) carry nothing, and az_*_adopt_net
 * discards the carried subtrees: they hold the old weights' evaluations.  The results are a DIFFERENT
 * search from the reference's (its playing strength is not measured); what they are is restated in
 * tests/treereuse_ref.py, which the engine equals bit for bit.
 * Must precede the first az_search_set_roots* / az_selfplay_reset (like az_search_set_evaluator); later,
 * with `on` outside 0 / 1, or with on = 1 on a handle of cfg.leaves > 1, it is an error and nothing
 * changes.  With reuse on az_search_persistent is 0.  The arena's and the tournament's MCTS players keep a
 * fresh tree per ply. */
int az_search_set_tree_reuse(az_search* s, int on);
/* *on = the mode; *reroots = re-roots that kept a subtree, *carried_visits = the sum over them of the new
 * root's visits, *carried_nodes = the sum of the nodes kept (the new root included) -- counted like
 * az_search_stats, since creation or the last az_selfplay_reset.  Any pointer may be NULL. */
int az_search_reuse_stats(az_search* s, int* on, uint64_t* reroots, uint64_t* carried_visits, uint64_t* carried_nodes);

/* Evaluation log (cfg.record_evals): keys[n] (fen keys), values[n], CSR priors at the
 * legal move indices. Pass NULL arrays to query sizes. */
int az_search_eval_log(az_search* s, int64_t* n_rows, int64_t* n_priors, uint64_t* keys, float* values,
                       int32_t* off, int32_t* idx, float* priors);

/* Profiling: device times measured with HIP events on the engine stream while enabled, on
 * every 32nd simulation step (steps 0, 32, 64, ...; every field except select_bytes covers
 * those sampled steps only: sim_steps = sampled steps = select_launches).
 * conv_*: the first residual 3x3 FxF conv of every simulation step (the dominant kernel);
 * conv_flop = algorithmic FLOPs of those launches (rows * 2*64*9*F*F).  tower_*: the whole
 * conv tower.  select_bytes: algorithmic bytes read by the select walk (16 B per edge +
 * 16 B node + 4 B sqrt per level). */
typedef struct {
    double conv_ms;      int64_t conv_launches;  double conv_flop;
    double tower_ms;     double tower_flop;
    double select_ms;    int64_t select_launches; double select_bytes;
    double expand_ms;    double encode_ms;       double heads_ms;    double backup_ms;
    double sim_step_ms;  int64_t sim_steps;      int64_t rows;
} az_timing;
int az_search_timing(az_search* s, az_timing* out, int reset, int enable);


/* ---- training: training.rs train() inner loop ---------------------
 * f32 end to end (the reference's precision).  The trainer owns a device copy of the flat
 * parameters (az_net_num_params layout, BatchNorm running statistics included), the AdamW
 * moments and every activation of a batch of up to max_batch positions. */
typedef struct az_trainer az_trainer;
/* get_cyclical_lr (training.rs:424-441) */
double az_cyclical_lr(int iteration);
/* AlphaZero::new/load_record + AdamWConfig::new().with_grad_clipping(Value(1.0))
 * .with_weight_decay(1e-4).init() (training.rs:48-66) */
int az_trainer_create(int blocks, int filters, const float* weights, size_t n, int max_batch, int device,
                      az_trainer** out);
int az_trainer_destroy(az_trainer* t);
/* forward (training-mode BatchNorm, running statistics updated) + compute_gradients
 * (training.rs:277-292) for one batch: planes [B,19,8,8] (to_tensor), target policy [B,4096],
 * target value [B].  losses (may be NULL) = {policy_loss, value_loss} batch means. */
int az_trainer_compute_grads(az_trainer* t, const float* planes, const float* target_policy,
                             const float* target_value, int batch, float* losses);
/* gradient all-reduce over the trainer's communicator (if any), clip by value 1.0,
 * AdamW step with learning rate lr (optimizer.step, training.rs:186-189) */
int az_trainer_apply(az_trainer* t, double lr);
/* compute_grads + apply: one iteration of training.rs:147-190 */
int az_trainer_step(az_trainer* t, const float* planes, const float* target_policy, const float* target_value,
                    int batch, double lr, float* losses);
/* flat parameters (to build an az_net for self-play, or to save) / last gradients */
int az_trainer_get_params(az_trainer* t, float* out, size_t n);
int az_trainer_get_grads(az_trainer* t, float* out, size_t n);
/* Replace the trainer's flat parameters (az_net_num_params layout, BatchNorm running statistics
 * included).  The AdamW moments, the AdamW step count, the last gradients and every setting (comm,
 * reducer, sharded) stay as they are.  n must be the trainer's parameter count, else an error and
 * no change.  Not a collective: at world > 1 the caller makes the same call on every rank. */
int az_trainer_set_params(az_trainer* t, const float* weights, size_t n);
/* the same from device memory on the trainer's device, ordered after what `stream` holds (NULL: the
 * trainer's stream); returns when the parameters are in place */
int az_trainer_set_params_device(az_trainer* t, const float* d_weights, size_t n, void* stream);
/* new_model = model.clone() (training.rs:132) kept on the device: copy the current parameters into a
 * trainer-owned buffer (allocated at the first call: one more copy of the parameters in HBM, freed with
 * the trainer; if that fails, an error and no change).  A later snapshot overwrites it. */
int az_trainer_snapshot(az_trainer* t);
/* parameters <- the snapshot (the rejected branch of training.rs:231); everything else as
 * az_trainer_set_params leaves it.  An error, and no change, before the first snapshot. */
int az_trainer_restore(az_trainer* t);
/* test hook: the snapshot's contents; an error before the first snapshot */
int az_trainer_get_snapshot(az_trainer* t, float* out, size_t n);
/* optimizer steps applied so far (burn's AdaptiveMomentumWState::time) */
int64_t az_trainer_adamw_steps(az_trainer* t);
/* az_net_update_device from the trainer's device parameters (BatchNorm running statistics included),
 * after everything queued on the trainer's stream: device to device, nothing goes to the host.  The
 * trainer and the net must share the device and the blocks x filters shape. */
int az_net_update_from_trainer(az_net* net, az_trainer* t);
/* introspection for parity tests: the activation each ReLU of the last forward acted on, in
 * forward order -- layer 0 = input block output, 1..2B = residual blocks (h_b, x_b+1 NHWC
 * [B*64][F]), 2B+1 = head convs after BN+ReLU [B*64][64] (columns 0..39), 2B+2 =
 * value_linear_1 output before its ReLU [B][64].  n must equal the tensor's size. */
int az_trainer_relu_output(az_trainer* t, int layer, float* out, size_t n);
/* device time (HIP events on the trainer stream) summed over steps: whole step (compute_grads
 * start to apply end) and the gradient all-reduce; reset = zero the sums after reading */
int az_trainer_timing(az_trainer* t, double* step_ms, double* allreduce_ms, int64_t* steps, int reset);
/* data-parallel training over RCCL (xGMI): rank 0 creates the id (128 bytes, returns its
 * size), every rank passes it to az_trainer_set_comm. */
int az_comm_unique_id(void* out, int cap);
int az_trainer_set_comm(az_trainer* t, const void* unique_id, int rank, int world);
/* The same data-parallel step with the exchange done by the caller on the host (no RCCL: e.g.
 * gloo / MPI between hosts, or a test driving two ranks in one process): at each apply, fn(ctx,
 * buf, n) must replace buf[0..n) (host memory) by its element-wise sum over the `world` ranks --
 * once for the gradients (before clipping; the AdamW step then scales by 1/world) and once for
 * the BatchNorm running statistics (then scaled by 1/world).  Return 0 on success.  Replaces a
 * communicator set by az_trainer_set_comm. */
typedef int (*az_allreduce_fn)(void* ctx, float* buf, size_t n);
int az_trainer_set_host_reducer(az_trainer* t, az_allreduce_fn fn, void* ctx, int rank, int world);
/* Sharded batch (on = 1): each rank's az_trainer_compute_grads batch is its shard of ONE global
 * batch -- the reference's single BATCH_SIZE = 512 step (training.rs:137-159, parameters.rs:17)
 * split over the ranks.  Every training-mode BatchNorm normalises with the statistics of the whole
 * global batch (agent.rs:37,41,115,125,134): each BN's per-rank (sum, squared deviations, rows)
 * are exchanged in the forward and its (sum dz, sum dz*yhat) in the backward, through the
 * communicator or host reducer (a sum all-reduce each: 2 per BatchNorm per step, 43 BNs at
 * 20x256); the loss and the BN backward normalise by the global row count, the summed gradient is
 * applied unscaled, the running statistics (identical on every rank) are not averaged, and the
 * reported losses are global means.  Off (default): each rank trains its own batch with per-rank
 * BatchNorm statistics and the gradients are averaged (global batch = batch x world).  At one rank
 * both modes compute the same step bit for bit. */
int az_trainer_set_sharded(az_trainer* t, int on);
/* the exchanges of the data-parallel steps since the last reset (RCCL all-reduces or host
 * reductions: sharded BatchNorm statistics and backward sums, losses, gradients, running
 * statistics): how many, over how many applied steps, and -- while az_trainer_time_exchanges(t, 1)
 * is on (off by default: the events cost queue time) -- their device time (HIP events around each
 * one on the trainer stream) */
int az_trainer_exchange_stats(az_trainer* t, int64_t* collectives, int64_t* steps, double* exchange_ms, int reset);
int az_trainer_time_exchanges(az_trainer* t, int on);

/* ---- replay buffer: memory.rs ReplayBuffer, host memory ------------ */
typedef struct az_replay az_replay;
int az_replay_create(int capacity, az_replay** out);                /* ReplayBuffer::new, memory.rs:33-38 */
int az_replay_destroy(az_replay* r);
int az_replay_len(const az_replay* r);                              /* memory.rs:103-105 */
/* ReplayBuffer::add (memory.rs:41-79): running mean into an existing FEN entry (returns 0) or
 * a new entry at the FIFO's end, evicting the oldest at capacity (returns 1) */
int az_replay_add(az_replay* r, const az_episode_step* step);
/* az_replay_add of steps[0..n) in order; returns the number of new unique positions (the union of
 * every rank's drained steps, added in rank order, keeps the replicas of one buffer identical) */
int az_replay_add_many(az_replay* r, const az_episode_step* steps, int n);
int az_replay_add_dense(az_replay* r, const az_pos* state, const float* policy, float value);
/* ReplayBuffer::sample (memory.rs:81-101): min(batch, len) distinct entries, uniformly (seeded);
 * writes to_tensor planes [n,19,64], policies [n,4096], values [n], positions (any may be NULL).
 * Returns n. */
int az_replay_sample(az_replay* r, int batch, uint64_t seed, float* planes, float* policy, float* value,
                     az_pos* states);
/* save / load (memory.rs:107-117): bincode 2 standard-config file of the reference's layout */
int az_replay_save(const az_replay* r, const char* path);
int az_replay_load(const char* path, int capacity, az_replay** out);
/* The same buffer with its payload in HBM (device >= 0; AZ_DEVICE_HOST, below: az_replay_create /
 * az_replay_load as they are).  The host keeps the keys (FEN strings), the FIFO order, the visit counts and
 * the key -> slot map; each of `capacity` slots on the device holds an entry's policy [4096] f32, its value
 * and the az_pos rebuilt from its key (what az_replay_sample returns): capacity x 16,468 bytes, allocated
 * here -- if that fails, or `device` is not one az_device_count lists, an error and no handle.  Every
 * az_replay_* call above works on such a handle with results identical to the host buffer's, bit for bit
 * (entries, running means, FIFO order, samples, save file, return values; az_replay_add_many applies the
 * steps before a bad one and then fails): adds upload the compact records (AZ_REPLAY_ADD_CHUNK steps per
 * launch: environment, read per call, default 256, at least 1; no result depends on it) and are complete
 * when the call returns; az_replay_sample gathers on the device and reads back once. */
int az_replay_create_on(int capacity, int device, az_replay** out);
int az_replay_load_on(const char* path, int capacity, int device, az_replay** out);
int az_replay_device(const az_replay* r);                           /* the device, or AZ_DEVICE_HOST */
/* az_replay_sample's draw (the same partial Fisher-Yates, n = min(batch, len)); rows [lo, hi) of it go to
 * device pointers on the buffer's device (any may be NULL), row lo at index 0: planes [hi-lo,19,64], policy
 * [hi-lo,4096] (16-byte aligned), value [hi-lo].  The work is ordered on `stream` (a hipStream_t; NULL = the
 * buffer's own stream, then complete on return).  Returns n.  0 <= lo <= hi <= n, else an error and nothing
 * is written; a host-backed handle is an error. */
int az_replay_sample_rows(az_replay* r, int batch, uint64_t seed, int lo, int hi, float* d_planes, float* d_policy,
                          float* d_value, void* stream);
/* az_trainer_compute_grads / az_trainer_step with the inputs already in HBM on the trainer's device: the
 * uploads become device-to-device copies on the trainer's stream (skipped for the trainer's own input
 * buffers), everything after them is the same, so a step is bit-identical to az_trainer_step on the same
 * data.  The inputs must be complete when the call is made. */
int az_trainer_compute_grads_device(az_trainer* t, const float* d_planes, const float* d_policy, const float* d_value,
                                    int batch, float* losses);
int az_trainer_step_device(az_trainer* t, const float* d_planes, const float* d_policy, const float* d_value, int batch,
                           double lr, float* losses);
/* The same fed by a device-backed buffer: rows [lo, hi) (hi < 0: n) of az_replay_sample_rows' draw are
 * gathered straight into the trainer's inputs on the trainer's stream, then the step runs; *drawn (may be
 * NULL) = n.  Errors, with nothing changed: the buffer is host-backed, on another device than the trainer,
 * or empty; rows outside 0 <= lo < hi <= n; more than the trainer's max_batch rows. */
int az_trainer_compute_grads_replay(az_trainer* t, az_replay* r, int batch, uint64_t seed, int lo, int hi, float* losses,
                                    int* drawn);
int az_trainer_step_replay(az_trainer* t, az_replay* r, int batch, uint64_t seed, int lo, int hi, double lr,
                           float* losses, int* drawn);

/* ---- test hook: the device rules path (parity tests; the engine never calls it) ----------
 * Runs, on the GPU, exactly what a leaf expansion runs (index_to_move + play, chess.rs:118-171 /
 * 42; the wave-parallel legal move generator; outcome(), chess.rs:43-50; the legal-ep flag and
 * repetition key) plus the roots' serial generator and the towers' plane staging (to_tensor,
 * chess.rs:191-245), for n items: item i = parent[i] with action[i] played (action[i] < 0: parent[i]
 * itself; an illegal action is refused on the host).  Outputs (child required, the rest may be NULL):
 * child[n] (flags, rep_key set); moves[n][256] / nmoves[n]: the leaf generator's legal indices in
 * shakmaty order with under-promotion duplicates (MCTree::new's `moves`, tree.rs:86-89);
 * root_moves[n][256] / root_n[n]: the same from the roots' generator; outcome[n] (AZ_ONGOING /
 * AZ_DRAW / AZ_WHITE_WINS / AZ_BLACK_WINS, no repetition); in_check[n]; fen_key[n] (the FEN-cache
 * key, tree.rs:214); planes[n][19][64]. */
int az_rules_probe(int device, const az_pos* parent, const int32_t* action, int n, az_pos* child, int32_t* moves,
                   int32_t* nmoves, int32_t* root_moves, int32_t* root_n, int32_t* outcome, int32_t* in_check,
                   uint64_t* fen_key, float* planes);

/* ---- test hooks: the MX-fp8 mode's arithmetic (the engine never calls az_mx8_conv_probe) -------
 * az_mx8_quantize: the host block quantiser az_net_create applies to the folded residual conv weights
 * of an AZ_DTYPE_FP8 net.  x holds nblocks blocks of 32 consecutive finite f32; block b gets the E8M0
 * byte scales[b] = 127 + clamp(floor(log2 max|x|) - 8, -127, 127) (an all-zero block: 127) and
 * codes[32 b + i] = x / 2^(scales[b] - 127) rounded to nearest even on the e4m3fn grid, saturating at
 * +-448 (a block with a non-finite value: scale 0xFF, codes 0x7F). */
int az_mx8_quantize(const float* x, size_t nblocks, uint8_t* codes, uint8_t* scales);
/* The host packer of the split-f16 Winograd tower's residual conv weights (test hook; no device):
 * folded [filters][filters][3][3], BatchNorm already folded in; filters 64, 128 or 256; streamed 16 or
 * 12.  U = G g G^T in f64, scaled by Sw (the largest power of two <= 2^24 with Sw max|U| <= 32768 over
 * all 16 points), split hi = f16(Sw U), lo = f16(Sw U - hi), as A fragments
 * [ci/32][step][co/16][hi, lo][lane = co%16 + 16 (ci%32/8)][ci%8] and two zero steps at the end.
 * streamed 16: step = point 4 a + b.  streamed 12: row a = 2 is left out (U[2][b] = U[0][b] + U[3][b] -
 * U[1][b]), step = 3 b + (0, 1, 2 for a = 0, 1, 3), and row a = 1 is stored negated.  Returns the number
 * of uint16 the stream holds (out NULL: that alone), < 0 on error; *unscale (may be NULL) =
 * 1 / (64 Sw). */
int az_wino16_pack(const float* folded, int filters, int streamed, uint16_t* out, size_t cap, float* unscale);
/* The same for the row-direct stream (AZ_WINO_ROWS; filters 256 only, anything else is an error):
 * W = g G^T in f64, [k][b] for the 3 tap rows x 4 column points, Sw the largest power of two <= 2^24
 * with Sw max|W| <= 32768 over these 12 values, the same split and A-fragment layout, step = 3 b + k,
 * nothing negated, and as many zero steps at the end as the kernel's weight ring is deep.  Returns the
 * number of uint16 (out NULL: that alone), < 0 on error; *unscale (may be NULL) = 1 / (64 Sw). */
int az_wino16_pack_rows(const float* folded, int filters, uint16_t* out, size_t cap, float* unscale);
/* One residual 3x3 conv layer (filters = 128 or 256) of n boards through the device conv routine and
 * epilogue tower8_kernel uses.  act_codes [n][64][F] / act_scales [n][64][F/32]: the input activation
 * (square = rank'*8 + file, blocks of 32 channels); w_codes [F][F][3][3] / w_scales [F][9][F/32]: the
 * weights (blocks = 32 input channels of one output channel and tap, tap = 3 ky + kx); bias [F] f32, the
 * accumulators' start; residual [n][64][F] bf16 or NULL.  With a residual the layer is a block's second
 * conv, y = relu(acc + residual); without, its first, y = relu(acc).  Outputs (any may be NULL): acc
 * [n][64][F], the raw f32 accumulators; out_bf16 (residual form only), y rounded to bf16;
 * out_codes / out_scales, y block-quantised as az_mx8_quantize does. */
int az_mx8_conv_probe(int device, int filters, int n, const uint8_t* act_codes, const uint8_t* act_scales,
                      const uint8_t* w_codes, const uint8_t* w_scales, const uint16_t* residual, const float* bias,
                      float* acc, uint16_t* out_bf16, uint8_t* out_codes, uint8_t* out_scales);

/* ---- test hook: the random streams' device functions (the engine never calls az_noise_probe) ----
 * One op over n items, with exactly the functions the root noise runs (csrc/detmath.h).  device >= 0: in a
 * kernel; AZ_DEVICE_HOST (below): the same functions as the host compiles them, no GPU needed.
 *   AZ_NOISE_LOGF / AZ_NOISE_EXPF   out[i] = det_logf(x[i]) / det_expf(x[i]), any f32 bit pattern
 *   AZ_NOISE_UNIFORM01 / _OPEN01    out[i][0..m) = the first m draws of the stream key[i] (m in 1..4096)
 *   AZ_NOISE_NORMAL                 out[i] = the first std_normal of the stream key[i]
 *   AZ_NOISE_GAMMA                  out[i] = gamma_sample(shape x[i], key[i])
 *   AZ_NOISE_DIRICHLET              out[i][0..m) = the Dirichlet row (alpha x[i], m components in
 *                                   1..AZ_MAX_MOVES, key[i]) as one game's root noise draws it, the
 *                                   tiny-alpha log-domain rows included (dir_alpha, above); fallback[i]
 *                                   (may be NULL) = 1 where the row was computed that way
 * x and key may be NULL where the op does not read them; m is ignored by the one-output ops; a shape or alpha
 * outside (0, 1e6] is an error, as are more than 2^28 outputs; a refused call writes nothing. */
enum { AZ_NOISE_LOGF = 0, AZ_NOISE_EXPF = 1, AZ_NOISE_UNIFORM01 = 2, AZ_NOISE_OPEN01 = 3, AZ_NOISE_NORMAL = 4,
       AZ_NOISE_GAMMA = 5, AZ_NOISE_DIRICHLET = 6 };
int az_noise_probe(int device, int op, int n, int m, const float* x, const uint64_t* key, float* out,
                   int32_t* fallback);

/* ---- arena opponent: the MiniMax(n) bot, chess.rs:248-322 ---------------------------------- */
#define AZ_DEVICE_HOST (-1)
#define AZ_MINIMAX_MAX_DEPTH 8
/* get_best_move's scoring for n positions at once (chess.rs:268-322). For position i: nmoves[i] = entries of legal_moves()
 * in shakmaty order WITH the four promotion entries; moves[i][k] = move index (queen-promotion index for all four);
 * promo[i][k] = 0 or the promoted role (1 N, 2 B, 3 R, 4 Q); scores[i][k] = -negamax(child, depth-1);
 * nodes[i] (may be NULL) = negamax() invocations for that position (the root's children included, the root not).
 * Arrays are [n][AZ_MAX_MOVES]; only the first nmoves[i] entries of a row are written, and nothing is written when
 * the call fails.  device >= 0: the GPU kernels; AZ_DEVICE_HOST: the same definition on the host (at most 16
 * threads).  depth in 1..AZ_MINIMAX_MAX_DEPTH; a position az_rules_probe would refuse, or one that lists more than
 * AZ_MAX_MOVES entries, is an error.  The GPU path keeps the tree's upper levels in a buffer of
 * AZ_MINIMAX_FRONTIER nodes (environment, read per call; default 1048576, at least 256): no result depends on it. */
int az_minimax_scores(int device, const az_pos* pos, int n, int depth, int32_t* moves, int32_t* promo,
                      int32_t* scores, int32_t* nmoves, int64_t* nodes);
/* best_moves.choose (chess.rs:304-321) with the seeded u in [0,1) standing in for thread_rng: the entry ordinal of the
 * min(floor(u*ties), ties-1)-th entry (the product in float), in list order, among those with the maximal score;
 * -1 if nmoves == 0. */
int az_minimax_best(const int32_t* scores, int nmoves, float u);

/* ---- evaluation arena on the device: validation.rs:155-402 evaluate / play_evaluation_game --------
 * `games` games in lockstep whose positions, position histories (the repetition multisets), move lists
 * and results live in HBM; az_arena_step plays one ply of every live game.  Game g has player 1 as White
 * when g is even and as Black when g is odd.  A move's result is play_move's (chess.rs:36-63): outcome()
 * first, then the position enters the multiset, then a draw at count >= 3, halfmoves >= 100 or
 * fullmoves >= 200. */
enum { AZ_PLAYER_MCTS = 0, AZ_PLAYER_BASE = 1, AZ_PLAYER_MINIMAX = 2, AZ_PLAYER_RANDOM = 3, AZ_PLAYER_EXTERNAL = 4 };
/* net: the MCTS and base-model players' network (NULL for an MCTS player: the synthetic evaluator);
 * depth: a MiniMax player's depth */
typedef struct { int kind; az_net* net; int depth; } az_arena_player;
typedef struct { int games, sims, num_stochastic_moves; float c_puct; uint64_t seed; } az_arena_cfg;
typedef struct az_arena az_arena;
/* p1 == p2 (the same pointer): one player on both sides.  Per mover kind:
 *   BASE      the net's policy row of the current position at the legal move indices, then az_arena_choose's
 *             rule with u[g]; num_inferences += 1 per ply and net, rows += games to move
 *   MCTS      a fresh noiseless tree from the current state with its repetition history
 *             (MCTree::async_init(.., false)), `sims` simulations, the same rule over the improved policy
 *             (the f32 values az_search_read_roots returns; they stay on the device); num_inferences +=
 *             sims + 1.  The arena owns one az_search per MCTS player ((games + 1) / 2 slots, `games` when it
 *             plays both colours, no FEN cache); spare slots repeat the first game's root, and rows counts
 *             their evaluations too
 *   MINIMAX   az_minimax_scores at `depth` on the arena's device, then az_minimax_best(scores, nmoves, u[g])
 *   RANDOM    entry min(floor(u[g] * n), n - 1) (the product in float) of az_pos_legal_indices' list
 *   EXTERNAL  actions[g]: the seat of the reference's Player::Human or any caller-side bot
 * The handle starts reset to the start position with cfg->seed. */
int az_arena_create(const az_arena_player* p1, const az_arena_player* p2, const az_arena_cfg* cfg, int device,
                    az_arena** out);
int az_arena_destroy(az_arena* a);
/* every game back to live with empty histories; start: [games] positions (each ongoing; its repetition
 * multiset holds it once), NULL = the start position.  seed: the engine stream's.  Allocates nothing.
 * With an MCTS player that does not play both sides, start positions that put one player to move in more
 * than (games + 1) / 2 games at once are refused here (its search holds that many roots); nothing changes. */
int az_arena_reset(az_arena* a, const az_pos* start, uint64_t seed);
/* one ply of every live game.  u [games]: game g's uniform in [0,1) for this ply's move choice; NULL: the
 * engine's stream, stream_key(seed, game, ply, 2).  actions [games]: read for games whose mover is
 * AZ_PLAYER_EXTERNAL only (NULL with such a mover is an error).  *live = games still going after the ply.
 * All or nothing: if an action is not a legal move index of its game, or a policy has a non-finite legal
 * entry, the call fails with a message naming the game and no game has advanced. */
int az_arena_step(az_arena* a, const float* u, const int32_t* actions, int* live);
/* result[g]: AZ_ONGOING / AZ_DRAW / AZ_WHITE_WINS / AZ_BLACK_WINS; plies[g]: moves played (either may be NULL) */
int az_arena_results(az_arena* a, int32_t* result, int32_t* plies);
/* live[g] = 1 while game g is going, else 0, as the last az_arena_step (or reset) read it back: no device
 * access.  Returns the number of live games. */
int az_arena_live(az_arena* a, int32_t* live);
/* the move indices of one game (at most cap written); returns the count */
int az_arena_history(az_arena* a, int game, int32_t* moves, int cap);
/* the two values validation.rs:209-254 accumulates, since the last reset */
int az_arena_stats(az_arena* a, double* num_inferences, double* rows);
/* validation.rs:297-308 / 337-350 over a 4096-entry policy (host, no device): fullmoves >
 * num_stochastic_moves picks the LAST maximal index; else rand 0.8 WeightedIndex -- sequential f32
 * cumulative sums, x = u * total (the largest float below total if that is not below it), the first index
 * whose cumulative sum exceeds x, 4095 if none does */
int az_arena_choose(const float* policy, int fullmoves, int num_stochastic_moves, float u);

/* ---- tournament arena: the pairings of a round robin (ratings.rs:10-24) in one device handle ------
 * Every pairing of a pool of players is one az_arena match of cfg->games games; all matches advance in
 * lockstep and each player evaluates all of its games to move at once.  Match m = i (i - 1) / 2 + j for
 * 0 <= j < i < n_players is evaluate(&players[i], &players[j]): players[i] is its player 1.  Tournament
 * game t = m * games + g is game g of match m; player 1 is White in it when g is even.  Every game comes
 * out move for move as az_arena plays it. */
#define AZ_TOURNAMENT_MAX_PLAYERS 16
typedef struct az_tournament az_tournament;
/* n (n - 1) / 2, < 0 outside 2..AZ_TOURNAMENT_MAX_PLAYERS.  No handle, no device. */
int az_tournament_matches(int n_players);
/* *p1 = i, *p2 = j of match m in the order above.  No handle, no device. */
int az_tournament_pair(int n_players, int m, int* p1, int* p2);
/* players [n_players]: MCTS, BASE, MINIMAX and RANDOM (EXTERNAL is refused); two entries naming the same
 * net are two players.  Per mover kind and ply, over all of the player's games to move in all its matches:
 *   BASE      one forward of its games' planes (rows ascending in t), then az_arena_choose's rule on the
 *             device; num_inferences += 1, rows += games to move
 *   MCTS      one search of (n_players - 1) * ((games + 1) / 2) slots (noiseless, no FEN cache, cfg->seed;
 *             spare slots repeat its first root) whose improved policy stays on the device, then the same
 *             rule; num_inferences += sims + 1, rows += the search's evaluations
 *   MINIMAX   one az_minimax_scores call, then az_minimax_best with the game's uniform
 *   RANDOM    as in az_arena
 * Arguments are checked before the first device call.  The handle starts reset with cfg->seed. */
int az_tournament_create(const az_arena_player* players, int n_players, const az_arena_cfg* cfg, int device,
                         az_tournament** out);
int az_tournament_destroy(az_tournament* t);
/* start [games]: start[g] is the start position of game g of EVERY match, NULL = the start position;
 * validated as az_arena_reset does (a rejected or already decided position is an error, and so is, with
 * an MCTS player in the pool, a set that puts one side to move in more than (games + 1) / 2 games of a
 * match); nothing changes on an error. */
int az_tournament_reset(az_tournament* t, const az_pos* start, uint64_t seed);
/* one ply of every live game of every match.  u [matches * games]: u[t] is game t's uniform; NULL: the
 * engine's stream, stream_key(seed, g, ply, 2) with g the game within its match -- the stream of
 * az_arena handles created with the same seed.  *live = games still going.  All or nothing across the
 * tournament: a refused move or a non-finite legal policy entry fails the call with a message naming the
 * match and the game, and no game of any match has advanced. */
int az_tournament_step(az_tournament* t, const float* u, int* live);
/* [matches * games] each, either may be NULL */
int az_tournament_results(az_tournament* t, int32_t* result, int32_t* plies);
/* live [matches * games] from the host mirror: no device access.  Returns the number of live games. */
int az_tournament_live(az_tournament* t, int32_t* live);
int az_tournament_history(az_tournament* t, int match, int game, int32_t* moves, int cap);
/* forwards launched and rows evaluated by the whole tournament since the last reset */
int az_tournament_stats(az_tournament* t, double* num_inferences, double* rows);

/* ---- an MCTS player's own search settings ----------------------------------------------------------
 * A field left 0 takes the handle's az_arena_cfg value (sims, c_puct) or the default (leaves: 1, the
 * reference's search; 2..8: az_search_cfg.leaves).  16 bytes.  The player's az_search is created with its own
 * sims, c_puct and leaves -- its node and edge arenas follow its sims, its slots are what they are without
 * settings -- and a ply it searches adds ceil(sims / leaves) + 1 to num_inferences: the forwards it launches,
 * sims + 1 at one leaf.  rows stays the search's evaluations. */
typedef struct { int sims; int leaves; float c_puct; int reserved; } az_player_search;
/* az_arena_create with s1 / s2 the settings of p1 / p2; either may be NULL (all zero).  Refused, before the
 * first device call and with *out untouched, in a message naming the player and the field: leaves outside
 * 0..8, sims < 0, c_puct < 0 or not finite, reserved != 0, a non-zero field on a player that is not
 * AZ_PLAYER_MCTS, an MCTS player whose sims come out 0 (cfg->sims may be 0 when every MCTS player brings its
 * own), and, with p1 == p2, an s2 that is neither NULL nor equal to *s1.  az_arena_create is this call with
 * NULL, NULL.
 * Environment, read here: AZ_ARENA_DEVICE_ROOTS (unset or 1: an MCTS player's roots are written by a kernel
 * from the arena's own position histories; 0: replayed on the host and uploaded) and AZ_ARENA_OVERLAP (unset
 * or 1: the searches of one ply run side by side on their own streams, players that name one az_net in player
 * order; 0: one after the other).  Every combination plays the same games and reports the same statistics. */
int az_arena_create_with(const az_arena_player* p1, const az_arena_player* p2, const az_player_search* s1,
                         const az_player_search* s2, const az_arena_cfg* cfg, int device, az_arena** out);
/* az_tournament_create with search [n_players] (NULL: all zero): search[i] belongs to players[i].  The same
 * refusals and the same environment; az_tournament_create is this call with NULL. */
int az_tournament_create_with(const az_arena_player* players, const az_player_search* search, int n_players,
                              const az_arena_cfg* cfg, int device, az_tournament** out);

#ifdef __cplusplus
}
#endif
#endif
