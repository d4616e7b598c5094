// wino.h -- the f32 Winograd F(2x2, 3x3) conv of one board, shared by the inference tower
// (tower.hip: tower32w_kernel, k_sims32w) and the training step (train.hip: conv_wino_train_kernel).
#pragma once
#include "az_internal.h"

namespace azi {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

// Packed f32 adds (v_pk_add_f32 / v_pk_fma_f32: two results per VALU issue) with the per-half source
// selects and negations written out.  Left to itself the compiler packed the transforms' adds but
// moved operands into register pairs first (one v_mov per packed add), and VALU issue is what the
// f32 MFMA pipe does not hide.  No memory operands: the waits stay the compiler's.
#define AZ_PK2(name, mods)                                                                    \
    __device__ __forceinline__ f32x2 name(f32x2 a, f32x2 b) {                                 \
        f32x2 r;                                                                              \
        asm("v_pk_add_f32 %0, %1, %2 " mods : "=v"(r) : "v"(a), "v"(b));                      \
        return r;                                                                             \
    }
#define AZ_PK3(name, mods)                                                                    \
    __device__ __forceinline__ f32x2 name(f32x2 a, f32x2 m, f32x2 b) {                        \
        f32x2 r;                                                                              \
        asm("v_pk_fma_f32 %0, %1, %2, %3 " mods : "=v"(r) : "v"(a), "v"(m), "v"(b));          \
        return r;                                                                             \
    }
AZ_PK2(pk_add, "")                                             // (a.x + b.x, a.y + b.y)
AZ_PK2(pk_sub, "neg_lo:[0,1] neg_hi:[0,1]")                    // (a.x - b.x, a.y - b.y)
AZ_PK2(pk_rowa, "op_sel_hi:[1,0] neg_lo:[0,1]")                // (a.x - b.x, a.y + b.x)
AZ_PK2(pk_rowb, "op_sel:[1,0] neg_lo:[0,1] neg_hi:[0,1]")      // (a.y - b.x, a.y - b.y)
AZ_PK2(pk_negx_add, "neg_lo:[1,1]")                            // (-a.x - b.x, a.y + b.y)
AZ_PK2(pk_negx_sub, "neg_lo:[1,0] neg_hi:[0,1]")               // (-a.x + b.x, a.y - b.y)
AZ_PK3(pk_fma_m0_sub, "op_sel_hi:[1,0,1] neg_lo:[0,0,1] neg_hi:[0,0,1]")    // (a.x m.x - b.x, a.y m.x - b.y)
AZ_PK3(pk_sub_m3, "op_sel:[0,1,0] neg_lo:[1,0,0] neg_hi:[1,0,0]")          // (b.x - a.x m.y, b.y - a.y m.y)
AZ_PK3(pk_negx_fma_m0, "op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[0,0,1]")   // (-a.x m.x + b.x, a.y m.x - b.y)
AZ_PK3(pk_negx_sub_m3, "op_sel:[0,1,0] neg_lo:[0,0,1] neg_hi:[1,0,0]")      // (a.x m.y - b.x, -a.y m.y + b.y)

// Phase stamps for the tower trace build (make EXTRA=-DAZ_TOWER_TRACE, tools/tower_trace.c): shader
// clock of one wave at a phase boundary, written by lane 0 through a vector store; `tr` is
// nullptr (no code) in every other build
__device__ __forceinline__ void wino_stamp(unsigned long long* tr, int k) {
#ifdef AZ_TOWER_TRACE
    if (tr) {
        __builtin_amdgcn_sched_barrier(0);
        unsigned long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        __builtin_amdgcn_sched_barrier(0);
        if ((threadIdx.x & 63) == 0) tr[k] = t;
    }
#else
    (void)tr; (void)k;
#endif
}

// zero squares before and after ACT ([64 squares][F/4 + 2 slots]): the transform reads the rows
// above / below the board there
constexpr int WINO_PAD_SQ = 8;

// ====================================================================== f32 Winograd tower
// tower32w_kernel: the same f32 tower with every residual 3x3 conv as Winograd F(2x2, 3x3)
// (Lavin & Gray): the 8x8 board is 16 output tiles of 2x2 whose 4x4 input patches are
// transformed V = B^T d B (16 points xi), the weights were transformed on the host
// U = G g G^T (f64, rounded once to f32), M[xi] = U[xi] V[xi] summed over the input channels is
// 16 GEMMs of F x 16 tiles x F on v_mfma_f32_16x16x4_f32 (exact f32 products), and
// Y = A^T M A.  2.25x fewer MFMAs than the direct conv (16 tiles x 16 points vs 64 squares x 9
// taps).  Numerics: f32 throughout; the transforms' rounding adds ~1.3x the direct f32 error
// (numpy check), checked against the oracle within the f32 tolerance.
// One board per workgroup:
//   ACT [64 squares][F/4 + 2 slots] f32 in LDS -- the layer input, overwritten in place by the
//       output (the block input x stays in the registers of the wave that owns it, as the residual),
//       with WINO_PAD_SQ zero squares before and after it;
//   V   [16 xi][channel quads][16 tiles][4] f32 in CH-channel chunks (double-buffered when the
//       input takes more than one chunk): chunk c+1 is transformed by all waves, one (channel,
//       tile) item per thread, while the MFMAs of chunk c run; one barrier per chunk;
//   weights [F/16 ci groups][16 xi][F/16 co groups][64 lanes][4] f32 per conv, streamed from L2
//       through a register ring of PF steps that carries across layers.
// Step constants (C3 / C2 A/B logs: profiles/r02_ab_wino_s9_knobs_c3.log, r02_ab_wino64_*):
//   WINO_TSPLIT 2  steps between a chunk's patch reads and their transform + V writes (8 -> 2: -2 %)
//   WINO_TSTAG 16  steps by which the second wave of each SIMD pair delays its transform (-0.4 %)
//   WINO_LA 4      B fragments read ahead from V
constexpr int WINO_TSPLIT = 2, WINO_TSTAG = 16, WINO_LA = 4;
// timing-only knob (wrong results): -DAZ_WINO_WFAKE=1 makes every ring step re-read the first two
// steps' weights (L2 / L1 hits), to price the weight stream from L2
#if defined(AZ_WINO_WFAKE) && AZ_WINO_WFAKE
#define WINO_WSTEP(t) ((t) & 1)
#else
#define WINO_WSTEP(t) (t)
#endif

// Per filter count: NWV waves per workgroup, NN 16-channel output fragments per wave, XS points
// per ring step, CH input channels per transform chunk (V buffer = CH KB), PF ring steps of
// weight prefetch.  Every wave owns NN output fragments x all 16 points.
//   F = 256: 8 waves (two per SIMD) x 32 output channels, one point per step (two independent
//            accumulator chains per step), 32-channel chunks;
//   F = 128: 8 waves x 16 channels, two points per step (still two chains: the f32 MFMA's
//            dependent latency exceeds its issue interval);
//   F = 64:  4 waves (one per SIMD) x 16 channels, two points per step, the whole 64-channel input
//            transformed as one chunk (one transform phase and one barrier per conv: C2 A/B -8 %).
template <int F> struct WinoCfg;
template <> struct WinoCfg<256> { static constexpr int NWV = 8, NN = 2, XS = 1, CH = 32, PF = 2; };
template <> struct WinoCfg<128> { static constexpr int NWV = 8, NN = 1, XS = 2, CH = 32, PF = 2; };
template <> struct WinoCfg<64> { static constexpr int NWV = 4, NN = 1, XS = 2, CH = 64, PF = 2; };
// weight ring of the tower: [PF steps][RX][NN] 16-byte fragments; a ring step covers XS points, RX =
// those points (f32 products) or their hi / lo planes, [2 xs + plane] (split-f16 products).
// Split-f16: one point per step where a wave owns two output fragments (F = 256: their two
// accumulator chains interleave), two points per step where it owns one (F = 128, 64: one point's
// hi hi, hi lo, lo hi is a single dependent chain).  There a step is 6 MFMAs of 16 cycles, a third of
// the f32 step, so the ring is 4 steps deep: the same ~400 cycles of MFMA issue ahead of the loads
// ROWS (wino_core_h16's row-direct form, F = 256): 8 accumulators per output fragment instead of 16
// leave room for a ring of WINO_ROWS_PF steps; the 16-point and derived forms keep 2 (with 4 they
// spill 51-73 VGPRs)
template <int F, bool H16, bool ROWS = false> struct WinoRing {
    static constexpr int XS = H16 ? (WinoCfg<F>::NN == 1 ? 2 : 1) : WinoCfg<F>::XS;
    static constexpr int RX = H16 ? 2 * XS : XS;
    static constexpr int PF = ROWS ? WINO_ROWS_PF : H16 && WinoCfg<F>::NN == 1 ? 4 : WinoCfg<F>::PF;
};
// Winograd weight fragment offsets: wave w's lane base (output fragments NN w..) and the byte
// offset of ring step t (16-channel group kl = t / 16, point t % 16) of chunk cg
template <int F> __device__ __forceinline__ int wino_voff(int w, int lane) {
    return (WinoCfg<F>::NN * w * 64 + lane) * 16;
}
template <int F> __device__ __forceinline__ int wino_toff(int cg, int t) {
    constexpr int KPC = WinoCfg<F>::CH / 16, CF = F / 16;
    return ((cg * KPC + t / 16) * 16 + t % 16) * CF * 1024;
}

// split-f16 weights: wave w's lane base (its 2 NN fragments of a step are consecutive: output
// fragment n, plane pl at (2 n + pl) KB); step t = chunk t / 16, point t % 16 at t * (F / 16) * 2 KB
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
template <int F> __device__ __forceinline__ int wino16_voff(int w, int lane) {
    return (2 * WinoCfg<F>::NN * w * 64 + lane) * 16;
}

// The input transform V[buf] <- B^T d B of one chunk, one (channel, tile) item per thread and
// item slot.  Items: wave w covers tile row ty = w & 3 and 16 channels per item: channel
// 16 (w >> 2 + g + it NWV / 4) + (lane & 15) of the chunk, tile (w & 3, lane >> 4) -- a patch read
// then touches 4 tiles of one row x 16 consecutive channels: conflict-free with the ACT row stride
// of 8 banks mod 64.  g = 1 names the item of the wave NWV / 4 waves later (used when one wave
// transforms for two).  In two halves: load issues the patch reads, store transforms and writes V.
// d[it][j] = patch column j as row pairs {rows 0, 1}, {rows 2, 3} (one ds_read2st64_b32 each).
// Element (i, j) of a patch is square (2 ty - 1 + i, 2 tl - 1 + j): rows off the board fall in the
// zero squares before / after ACT (WINO_PAD_SQ), so every row offset is an instruction immediate;
// the off-board columns (tl = 0: j = 0, tl = 3: j = 3) are read at a clamped on-board column (3 / 4:
// keeps the 32-lane groups of each read on distinct banks) and multiplied by 0 in store.
// the input transform's forms (WinoXf::store16)
constexpr int WINO_XF_FULL = 0, WINO_XF_NEG1 = 1, WINO_XF_COLS = 2;

// ---- V with shared rows (the row-direct form at F = 256, AZ_WINO_VROWS).  Rows 2, 3 of a tile's patch
// are rows 0, 1 of the tile below, so the per-tile V holds every D row of board rows 1-6 twice and the
// rows off the board as computed zeros.  Here a chunk's V holds each D row of the padded board once:
// entry (column point b, padded row r = 0..9, channel octet o, tile column tc) = 8 channels of f16,
// 16 B, in a hi plane and a lo plane of 640 entries (VR_PLANE = 10 KB; a buffer 20 KB against 32; the lo
// plane with the tile column ^ 2: wino_vr_lo).  Rows
// 0 and 9 are off the board: zeroed once per board (tower32w_board), never written by an item.
//   entry address  ((2 b + (r & 1)) 5 + (r >> 1)) 256 + (4 (o ^ 2 ((r >> 1) & 1)) + tc) 16
// The B fragment of patch row i, point b of lane (h = lane >> 4, tr = (lane & 15) >> 2, tc = lane & 3) is
// entry (b, 2 tr + i, h, tc), one ds_read_b128 per plane: the eight (h, tr) of a ds_read_b128 lane group
// fall on four distinct octet slots (the XOR by the row pair's parity), 64 banks, one-way.
// Transform items: one lane = one channel x one board row x one tile column; a wave-item q = 0..15 is
// row 1 + (q >> 1), channels 16 (q & 1) + (lane & 15) of the chunk, tile column lane >> 4.  4 ACT reads
// (columns 2 tc - 1 .. 2 tc + 2, clamped as WinoXf::load), the 4 points of xform_cols, 4 x split16, pair
// swap, 4 ds_write_b32 (32 lanes = 2 octets x 2 tile columns x 4 pairs x hi, lo: 32 banks).  The
// arithmetic per entry is xform_cols' and split16's: every stored bit is the per-tile form's.
// The address functions are host-callable: az_wino_vrows_layout tabulates them for tests/.
constexpr int WINO_VR_PLANE = 10240, WINO_VR_BYTES = 2 * WINO_VR_PLANE, WINO_VR_ITEMS = 16;
constexpr int WINO_VR_R16 = (256 / 4 + 2) * 16;                     // ACT square stride at F = 256
// the lo plane's copy of a hi-plane address (its part below 256 B): one plane further, tile column ^ 2 --
// the hi and the lo lane of a channel pair then write 8 banks apart (on one bank the ds_write_b32 was
// 2-way: SQ_LDS_BANK_CONFLICT 1.6x the per-tile form's); uniform within a read
__host__ __device__ constexpr int wino_vr_lo(int a) { return (a ^ 32) + WINO_VR_PLANE; }
__host__ __device__ constexpr int wino_vr_lo_if(int lo, int a) { return lo ? wino_vr_lo(a) : a; }
__host__ __device__ constexpr int wino_vr_item(int wave, int it, int nw) { return wave + nw * it; }   // nw transform waves
__host__ __device__ constexpr int wino_vr_item_row(int q) { return 1 + (q >> 1); }
// write address of (wave-item q, lane, point b) = the item's wave-uniform part + the lane's + b's
__host__ __device__ constexpr int wino_vr_wuni(int q) {
    const int r = wino_vr_item_row(q), rp = (r >> 1) & 1;
    return ((r & 1) * 5 + (r >> 1)) * 256 + (((q & 1) ^ rp) * 2) * 64;
}
__host__ __device__ constexpr int wino_vr_wlane(int lane) {
    return wino_vr_lo_if(lane & 1, ((lane >> 3) & 1) * 64 + (lane >> 4) * 16) + ((lane & 7) >> 1) * 4;
}
__host__ __device__ constexpr int wino_vr_wpoint(int b) { return b * 2560; }
__host__ __device__ constexpr int wino_vr_write(int q, int lane, int b) { return wino_vr_wuni(q) + wino_vr_wlane(lane) + wino_vr_wpoint(b); }
// read address (hi plane; lo: wino_vr_lo of the lane's part) of patch row i, point b: the lane's part for the row pair
// i >> 1 + an immediate
// (the next row pair is one 256-byte run further, and its parity flips the octet slot's bit 1: byte 128)
__host__ __device__ constexpr int wino_vr_rlane(int lane, int i2) {
    const int h = lane >> 4, tr = (lane & 15) >> 2, tc = lane & 3;
    const int a0 = tr * 256 + (4 * (h ^ (2 * (tr & 1))) + tc) * 16;
    return i2 ? (a0 ^ 128) + 256 : a0;
}
__host__ __device__ constexpr int wino_vr_rimm(int i, int b) { return (2 * b + (i & 1)) * 5 * 256; }
__host__ __device__ constexpr int wino_vr_read(int i, int b, int lane) { return wino_vr_rlane(lane, i >> 1) + wino_vr_rimm(i, b); }
// the 32 runs of 256 B that are rows 0 and 9 (k = 16 buffer + 8 plane + 2 b + (0: row 0, 1: row 9)), bytes
// from the first buffer
__host__ __device__ constexpr int wino_vr_zero(int k) {
    return (k >> 4) * WINO_VR_BYTES + ((k >> 3) & 1) * WINO_VR_PLANE + (k & 1 ? (2 * ((k >> 1) & 3) + 1) * 5 + 4 : 2 * ((k >> 1) & 3) * 5) * 256;
}
// the item's ACT reads (bytes from ACT, chunk 0): column j of row r - 1, channel 16 (q & 1) + (lane & 15);
// lane part (column 2 tc), the clamped steps to columns j = 0 and 3, the wave-uniform part
__host__ __device__ constexpr int wino_vr_alane(int lane) { return (lane >> 4) * (2 * WINO_VR_R16) + (lane & 15) * 4; }
__host__ __device__ constexpr int wino_vr_acol(int tc, int j) {
    return j == 0 ? (tc > 0 ? -WINO_VR_R16 : 3 * WINO_VR_R16) : j == 1 ? 0 : j == 2 ? WINO_VR_R16
                                                                  : (tc < 3 ? 2 * WINO_VR_R16 : -2 * WINO_VR_R16);
}
__host__ __device__ constexpr int wino_vr_auni(int q) { return (wino_vr_item_row(q) - 1) * 8 * WINO_VR_R16 + (q & 1) * 64; }
__host__ __device__ constexpr int wino_vr_act(int q, int lane, int j) { return wino_vr_auni(q) + wino_vr_alane(lane) + wino_vr_acol(lane >> 4, j); }
template <int F> struct WinoXf {
    static constexpr int NWV = WinoCfg<F>::NWV, CH = WinoCfg<F>::CH, RS = F / 4 + 2;
    static constexpr int VBYTES = CH * 1024, XST = CH * 64, IT = CH * 16 / (NWV * 64);
    static constexpr int R16 = RS * 16, ROW = 8 * R16;
    typedef f32x2 Patch[IT][4][2];
    char* ldsb;
    int vbase, w, lane, tty, ttx;
    __device__ __forceinline__ WinoXf(char* l, int vb, int w_, int lane_)
        : ldsb(l), vbase(vb), w(w_), lane(lane_), tty(w_ & 3), ttx(lane_ >> 4) {}
    __device__ __forceinline__ int tchan(int it, int g) const { return 16 * ((w >> 2) + g + it * (NWV / 4)) + (lane & 15); }
    __device__ __forceinline__ int vwr(int tch) const {   // + xi * XST
        return (tch >> 2) * 256 + (((4 * tty + ttx) ^ (2 * ((tch >> 2) & 3))) * 16) + (tch & 3) * 4;
    }
    __device__ __forceinline__ void load(int c, Patch& d, int g = 0) const {
        // recomputed per chunk from a laundered index: one loop-invariant register more spilled
        const int tl = vgpr_index(ttx);
        const int pc1 = tl * (2 * R16) + (lane & 15) * 4;
        const int pd0 = tl > 0 ? -R16 : 3 * R16, pd3 = tl < 3 ? 2 * R16 : -2 * R16;
#pragma unroll
        for (int it = 0; it < IT; it++) {
            // tchan(it) - (lane & 15) is wave-uniform
            const int b1 = pc1 + (2 * tty - 1) * ROW + (c * CH + tchan(it, g) - (lane & 15)) * 4;
            const int cb[4] = {b1 + pd0, b1, b1 + R16, b1 + pd3};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const char* p = ldsb + cb[j];
                d[it][j][0] = f32x2{*reinterpret_cast<const float*>(p), *reinterpret_cast<const float*>(p + ROW)};
                d[it][j][1] = f32x2{*reinterpret_cast<const float*>(p + 2 * ROW), *reinterpret_cast<const float*>(p + 3 * ROW)};
            }
        }
    }
    // B^T d B of one channel's patch: d[j] = column j as row pairs {rows 0, 1}, {rows 2, 3};
    // v[k][rp] = (points (2 rp) 4 + k, (2 rp + 1) 4 + k); m = (m0, m3): 0 where patch column 0 / 3
    // is off the board
    static __device__ __forceinline__ void xform(const f32x2 (&d)[4][2], f32x2 m, f32x2 (&v)[4][2]) {
        // rows: A[j] = (tt0, tt1) = (e0 - e2, e1 + e2), B[j] = (-tt2, tt3) = (e1 - e2, e1 - e3)
        f32x2 A[4], B[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            A[j] = pk_rowa(d[j][0], d[j][1]);
            B[j] = pk_rowb(d[j][0], d[j][1]);
        }
        // columns, two rows at a time: v0 = t0 m0 - t2, v1 = t1 + t2, v2 = t2 - t1, v3 = t1 - t3 m3
        // (the same roundings as the scalar form: every multiply is by 1 or 0)
        v[0][0] = pk_fma_m0_sub(A[0], m, A[2]);
        v[1][0] = pk_add(A[1], A[2]);
        v[2][0] = pk_sub(A[2], A[1]);
        v[3][0] = pk_sub_m3(A[3], m, A[1]);
        v[0][1] = pk_negx_fma_m0(B[0], m, B[2]);
        v[1][1] = pk_negx_add(B[1], B[2]);
        v[2][1] = pk_negx_sub(B[2], B[1]);
        v[3][1] = pk_negx_sub_m3(B[3], m, B[1]);
    }
    // d B of one channel's patch, the column pass of xform on the raw rows: v[k][rp] = (D[2 rp][k],
    // D[2 rp + 1][k]), 8 packed operations
    static __device__ __forceinline__ void xform_cols(const f32x2 (&d)[4][2], f32x2 m, f32x2 (&v)[4][2]) {
#pragma unroll
        for (int rp = 0; rp < 2; rp++) {
            v[0][rp] = pk_fma_m0_sub(d[0][rp], m, d[2][rp]);
            v[1][rp] = pk_add(d[1][rp], d[2][rp]);
            v[2][rp] = pk_sub(d[2][rp], d[1][rp]);
            v[3][rp] = pk_sub_m3(d[3][rp], m, d[1][rp]);
        }
    }
    __device__ __forceinline__ void store(int buf, const Patch& d, int g = 0) const {
        const int tl = vgpr_index(ttx);
        const f32x2 m = f32x2{tl > 0 ? 1.0f : 0.0f, tl < 3 ? 1.0f : 0.0f};
#pragma unroll
        for (int it = 0; it < IT; it++) {
            f32x2 v[4][2];   // [column k][row pair]
            xform(d[it], m, v);
            char* vb = ldsb + vbase + buf * VBYTES + vwr(tchan(it, g));
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int rp = 0; rp < 2; rp++) {
                    *reinterpret_cast<float*>(vb + ((2 * rp) * 4 + k) * XST) = v[k][rp].x;
                    *reinterpret_cast<float*>(vb + ((2 * rp + 1) * 4 + k) * XST) = v[k][rp].y;
                }
        }
    }
    // the first NWV / 2 waves transform chunk c into V[buf] for all NWV waves (their own items and
    // those of the waves NWV / 2 later): F = 256 only (IT = 1, NWV = 8)
    template <bool H16 = false, int XF = WINO_XF_FULL> __device__ __forceinline__ void both(int c, int buf) const {
        static_assert(IT == 1 && NWV == 8, "two items per thread of the first half");
        Patch d0, d1;
        load(c, d0, 0);
        if constexpr (H16) {   // one item at a time: the deeper weight ring leaves no room for both patches
            store16<XF>(buf, d0, 0);
            load(c, d1, 1);
            store16<XF>(buf, d1, 1);
        } else {
            load(c, d1, 1);
            store(buf, d0, 0);
            store(buf, d1, 1);
        }
    }
    // ---- split-f16 V (wino_core_h16): the chunk's V as two f16 planes, hi at 0 and lo at VBYTES / 2,
    // each [16 xi][channel octet][16 tile slots][8] f16 (XST16 = 32 CH bytes per point, 1 KB at CH = 32:
    // the B fragment of v_mfma_f32_16x16x32_f16 is one ds_read_b128 per lane, 8 channels of one tile).  The transform
    // stays f32; each value is then scaled by WINO16_SA and split hi = f16(s), lo = f16(s - hi)
    // (round to nearest even: 22 significand bits between them).  A lane owns one channel, its
    // neighbour lane ^ 1 the other channel of the pair: they swap (hi, lo) over DPP, the even lane
    // writes the pair's hi, the odd lane its lo, one ds_write_b32 each.  Tile slot = tile ^ 2 (octet
    // & 3) ^ 4 (lo plane): the 32 lanes of a write (16 channels x 2 tiles, a hi and a lo lane per
    // pair; 32 banks) cover 8 slot values mod 8 x 4 pairs = 32 distinct banks; the B-fragment read
    // is the f32 layout's (quad -> octet), the XOR by 4 uniform within a read: both conflict-free
    // (an XOR by 8 left the hi and lo lanes of a pair on one bank: PMC 22 % of LDS cycles conflicts).
    // A value beyond the f16 range (|V| Sa >= 65520) splits into (inf, -inf): their products sum to
    // NaN, which every ReLU of the split-f16 tower keeps, the heads' included (tower.hip relu_nan).
    // XF = WINO_XF_NEG1 (wino_core_h16 with 12 streamed points): the point row 1 (xi = 4..7) is written
    // negated, to go with the negated weights of that row; exact, and (inf, -inf) stays a NaN-producing
    // pair.  XF = WINO_XF_COLS (the row-direct form): the column transform alone, D = d B (xform_cols),
    // plane 4 i + b = patch row i, column point b; |D| <= 2 |x|.  Scale, split, pair swap and layout
    // are the same.
    static __device__ __forceinline__ unsigned split16(float v) {
        const float s = v * WINO16_SA;
        const _Float16 hi = (_Float16)s;
        const _Float16 lo = (_Float16)(s - (float)hi);
        return (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
    }
    static constexpr int XST16 = CH * 32;
    __device__ __forceinline__ int vwr16(int tch) const {   // + xi * XST16
        const int odd = lane & 1;
        return odd * (VBYTES / 2) + (tch >> 3) * 256 +
               (((4 * tty + ttx) ^ (2 * ((tch >> 3) & 3)) ^ (4 * odd)) * 16) + ((tch & 7) >> 1) * 4;
    }
    template <int XF = WINO_XF_FULL> __device__ __forceinline__ void store16(int buf, const Patch& d, int g = 0) const {
        constexpr bool NEG1 = XF == WINO_XF_NEG1;
        const int tl = vgpr_index(ttx);
        const f32x2 m = f32x2{tl > 0 ? 1.0f : 0.0f, tl < 3 ? 1.0f : 0.0f};
        // v_perm_b32 selectors: even lane (own.hi, other.hi), odd lane (other.lo, own.lo)
        const unsigned sel = (lane & 1) ? 0x03020706u : 0x05040100u;
#pragma unroll
        for (int it = 0; it < IT; it++) {
            f32x2 v[4][2];   // [column k][row pair]
            if constexpr (XF == WINO_XF_COLS) xform_cols(d[it], m, v);
            else xform(d[it], m, v);
            char* vb = ldsb + vbase + buf * VBYTES + vwr16(tchan(it, g));
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int rp = 0; rp < 2; rp++)
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const float pv = e ? v[k][rp].y : v[k][rp].x;
                        const unsigned own = split16(NEG1 && 2 * rp + e == 1 ? -pv : pv);
                        // quad_perm [1, 0, 3, 2]: the other channel of the pair
                        const unsigned oth = (unsigned)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xF, 0xF, true);
                        *reinterpret_cast<unsigned*>(vb + ((2 * rp + e) * 4 + k) * XST16) = __builtin_amdgcn_perm(oth, own, sel);
                    }
        }
    }
    // ---- shared-row items (wino_vr_* above, F = 256): vr_load issues wave-item q's four ACT reads of
    // chunk c, vr_store makes the four points with xform_cols' operations (each multiply by 1 or 0 inside
    // an FMA, the same roundings), splits, swaps within the channel pair and writes them into V[buf]
    // (ln: the lane index laundered by the caller, so that nothing derived from it stays live from chunk
    // to chunk: see load)
    __device__ __forceinline__ void vr_load(int c, int q, float (&e)[4], int ln) const {
        static_assert(F == 256 && R16 == WINO_VR_R16 && CH == 32, "the shared-row layout is the 256-filter tower's");
        const int tl = ln >> 4;
        const char* p = ldsb + wino_vr_alane(ln) + wino_vr_auni(q) + c * CH * 4;
#pragma unroll
        for (int j = 0; j < 4; j++) e[j] = *reinterpret_cast<const float*>(p + wino_vr_acol(tl, j));
    }
    __device__ __forceinline__ void vr_store(int buf, int q, const float (&e)[4], int ln) const {
        const int tl = ln >> 4;
        const float m0 = tl > 0 ? 1.0f : 0.0f, m3 = tl < 3 ? 1.0f : 0.0f;
        const unsigned sel = (ln & 1) ? 0x03020706u : 0x05040100u;
        const float v[4] = {__builtin_fmaf(e[0], m0, -e[2]), e[1] + e[2], e[2] - e[1], __builtin_fmaf(-e[3], m3, e[1])};
        char* vb = ldsb + vbase + buf * WINO_VR_BYTES + wino_vr_wuni(q) + wino_vr_wlane(ln);
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const unsigned own = split16(v[b]);
            const unsigned oth = (unsigned)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xF, 0xF, true);
            *reinterpret_cast<unsigned*>(vb + wino_vr_wpoint(b)) = __builtin_amdgcn_perm(oth, own, sel);
        }
    }
    // chunk c into V[buf] by the first NW waves, WINO_VR_ITEMS / NW wave-items each
    template <int NW> __device__ __forceinline__ void vrows(int c, int buf) const {
        // two items' reads in flight at a time: 8 VGPRs of patch values
        constexpr int NI = WINO_VR_ITEMS / NW;
        static_assert(NI % 2 == 0, "items in pairs");
        const int ln = vgpr_index(lane);
#pragma unroll
        for (int i2 = 0; i2 < NI; i2 += 2) {
            float e[2][4];
            vr_load(c, wino_vr_item(w, i2, NW), e[0], ln);
            vr_load(c, wino_vr_item(w, i2 + 1, NW), e[1], ln);
            vr_store(buf, wino_vr_item(w, i2, NW), e[0], ln);
            vr_store(buf, wino_vr_item(w, i2 + 1, NW), e[1], ln);
        }
    }
};

// DPP row shift within the 16-lane rows: lane l reads lane l - N (SHR) / l + N (SHL); a source
// outside the row reads 0 (bound_ctrl)
template <int CTRL> __device__ __forceinline__ float row_dpp(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_SHL = 0x100, DPP_SHR = 0x110;

// The next conv's input transform straight from a wave's conv outputs (F = 64: each wave's 16
// output channels x all 16 tiles are one quarter of the single 64-channel chunk).  o[q] = the
// lane's 4 channels (quad h of the wave's 16) at square (2 ty + q / 2, 2 tx + q % 2) of tile
// l16 = 4 ty + tx.  A tile's 4x4 patch reaches one square into each neighbouring tile; the
// neighbours' values come over DPP row shifts (tile +-1 = lane +-1, +-4 = lane +-4 within the
// 16-lane row): off-board rows read 0 (outside the row), off-board columns read a finite value
// that the transform multiplies by 0 -- exactly WinoXf::load + store on the same outputs in LDS,
// bit for bit.  Writes the 16 points x 4 channels of the lane's (quad, tile) into V at vdst with
// one ds_write_b128 per point.
// H16: V in the split-f16 layout (WinoXf::store16: two f16 planes, [xi][octet][tile slot][8]).  The
// lane's quad is half h & 1 of octet cq / 2: each value goes through WinoXf::split16, the lane
// groups h and h ^ 1 exchange (the even one gives its lo and takes the other's hi), and per point
// the even group writes the octet's hi, the odd group its lo, one ds_write_b128 each -- the bits
// WinoXf::load + store16 would write.  The 8 lanes a ds_write_b128 services together are 8 tile
// slots distinct mod 8: 32 distinct banks (one ds_write_b64 per lane and plane instead was 2-way:
// its 16 lanes cover 16 slots of 8 bytes; PMC + 1.44 M conflict cycles per launch, 16 % of LDS cycles).
AZ_PK2(pkc_nadd, "neg_lo:[1,1] neg_hi:[1,1]")                 // (-a.x - b.x, -a.y - b.y)
AZ_PK3(pkc_fma_nc, "neg_lo:[0,0,1] neg_hi:[0,0,1]")            // (a.x m.x - c.x, a.y m.y - c.y)
AZ_PK3(pkc_nfma, "neg_lo:[1,0,0] neg_hi:[1,0,0]")              // (-a.x m.x + c.x, -a.y m.y + c.y)
AZ_PK3(pkc_fma, "")                                            // (a.x m.x + c.x, a.y m.y + c.y)
#undef AZ_PK2
#undef AZ_PK3
template <int F, bool H16 = false>
__device__ __forceinline__ void wino_xform_regs(const f32x4 (&o)[4], char* __restrict__ vdst, int w, int lane) {
    static_assert(F == 64 && WinoCfg<F>::NN == 1, "one chunk, one output fragment per wave");
    constexpr int XST = WinoCfg<F>::CH * 64;
    const int l16 = lane & 15, h = lane >> 4, tx = l16 & 3;
    const int cq = w * 4 + h;                                       // channel quad of the chunk
    const float m0 = tx > 0 ? 1.0f : 0.0f, m3 = tx < 3 ? 1.0f : 0.0f;
    const f32x2 m0v = f32x2{m0, m0}, m3v = f32x2{m3, m3};
    f32x4 out[16];
#pragma unroll
    for (int cp = 0; cp < 2; cp++) {   // channel pairs (2 cp, 2 cp + 1), packed in one f32x2
        auto own = [&](int q) { return cp ? f32x2{o[q][2], o[q][3]} : f32x2{o[q][0], o[q][1]}; };
        auto nb = [&](auto dpp, int q) { const f32x2 v = own(q); return f32x2{dpp(v.x), dpp(v.y)}; };
        auto shr1 = [](float x) { return row_dpp<DPP_SHR + 1>(x); };
        auto shr3 = [](float x) { return row_dpp<DPP_SHR + 3>(x); };
        auto shr4 = [](float x) { return row_dpp<DPP_SHR + 4>(x); };
        auto shr5 = [](float x) { return row_dpp<DPP_SHR + 5>(x); };
        auto shl1 = [](float x) { return row_dpp<DPP_SHL + 1>(x); };
        auto shl3 = [](float x) { return row_dpp<DPP_SHL + 3>(x); };
        auto shl4 = [](float x) { return row_dpp<DPP_SHL + 4>(x); };
        auto shl5 = [](float x) { return row_dpp<DPP_SHL + 5>(x); };
        // P[i][j]: patch rows i (square row 2 ty - 1 + i), columns j
        const f32x2 P[4][4] = {
            {nb(shr5, 3), nb(shr4, 2), nb(shr4, 3), nb(shr3, 2)},
            {nb(shr1, 1), own(0), own(1), nb(shl1, 0)},
            {nb(shr1, 3), own(2), own(3), nb(shl1, 2)},
            {nb(shl3, 1), nb(shl4, 0), nb(shl4, 1), nb(shl5, 0)}};
        // rows (as WinoXf::xform): R0 = P0 - P2, R1 = P1 + P2, nR2 = P1 - P2, R3 = P1 - P3
        f32x2 R[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            R[0][j] = pk_sub(P[0][j], P[2][j]);
            R[1][j] = pk_add(P[1][j], P[2][j]);
            R[2][j] = pk_sub(P[1][j], P[2][j]);
            R[3][j] = pk_sub(P[1][j], P[3][j]);
        }
        // columns: the operations of WinoXf::xform per point, two channels per instruction
        f32x2 V[4][4];
        V[0][0] = pkc_fma_nc(R[0][0], m0v, R[0][2]);
        V[0][1] = pk_add(R[0][1], R[0][2]);
        V[0][2] = pk_sub(R[0][2], R[0][1]);
        V[0][3] = pkc_nfma(R[0][3], m3v, R[0][1]);
        V[1][0] = pkc_fma_nc(R[1][0], m0v, R[1][2]);
        V[1][1] = pk_add(R[1][1], R[1][2]);
        V[1][2] = pk_sub(R[1][2], R[1][1]);
        V[1][3] = pkc_nfma(R[1][3], m3v, R[1][1]);
        V[2][0] = pkc_nfma(R[2][0], m0v, R[2][2]);
        V[2][1] = pkc_nadd(R[2][1], R[2][2]);
        V[2][2] = pk_sub(R[2][1], R[2][2]);
        V[2][3] = pkc_fma_nc(R[2][3], m3v, R[2][1]);
        V[3][0] = pkc_fma_nc(R[3][0], m0v, R[3][2]);
        V[3][1] = pk_add(R[3][1], R[3][2]);
        V[3][2] = pk_sub(R[3][2], R[3][1]);
        V[3][3] = pkc_nfma(R[3][3], m3v, R[3][1]);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                out[4 * a + b][2 * cp] = V[a][b].x;
                out[4 * a + b][2 * cp + 1] = V[a][b].y;
            }
    }
    if constexpr (H16) {
        constexpr int XST16 = WinoXf<F>::XST16, PLANE = WinoXf<F>::VBYTES / 2;
        const int oc = cq >> 1, odd = h & 1;
        char* vb = vdst + odd * PLANE + oc * 256 + ((l16 ^ (2 * (oc & 3)) ^ (4 * odd)) * 16);
#pragma unroll
        for (int p = 0; p < 16; p++) {
            unsigned q[4];
#pragma unroll
            for (int e = 0; e < 2; e++) {
                // WinoXf::split16 of the channel pair (2e, 2e + 1), two values per instruction: the
                // packed conversions round to nearest even as the scalar ones, the even channel in the
                // low half
                typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
                const f32x2 s = f32x2{out[p][2 * e], out[p][2 * e + 1]} * WINO16_SA;
                const f16x2 h2 = __builtin_convertvector(s, f16x2);
                const f16x2 l2 = __builtin_convertvector(s - __builtin_convertvector(h2, f32x2), f16x2);
                const unsigned hi = __builtin_bit_cast(unsigned, h2), lo = __builtin_bit_cast(unsigned, l2);
                // v_permlane16_swap_b32: the odd rows of hi change places with the even rows of lo, so an
                // even lane group then holds (its hi, the next group's hi), an odd one (the previous
                // group's lo, its lo): both in channel order
                const auto sw = __builtin_amdgcn_permlane16_swap(hi, lo, false, false);
                q[e] = sw[0];
                q[2 + e] = sw[1];
            }
            *reinterpret_cast<uint4*>(vb + p * XST16) = make_uint4(q[0], q[1], q[2], q[3]);
        }
    } else {
        char* vb = vdst + cq * 256 + ((l16 ^ (2 * (cq & 3))) * 16);
#pragma unroll
        for (int p = 0; p < 16; p++) *reinterpret_cast<f32x4*>(vb + p * XST) = out[p];
    }
}

// wino_core: one Winograd conv of the board whose layer input is in ACT ([64 squares][F/4 + 2
// slots] f32 at ldsb, WINO_PAD_SQ zero squares on either side), V buffers at vbase: every wave's y[n][q] = this wave's outputs (output
// fragment n, tile lane & 15, square (2 ty + q / 2, 2 tx + q % 2), channels co0 + 16 n + 0..3)
// + bias (nullptr: none).  Ends without a workgroup barrier: other waves may still be issuing
// MFMAs on the last V buffer, but every read of ACT and of the other V buffer is done, so the caller
// may overwrite ACT; it must pass a barrier before the next wino_core (which writes V) or before
// reusing V.
// wr: the weight ring; holds this conv's first PF steps on entry and the next conv's (rN) on
// exit, so no layer starts on a cold weight fetch
template <int F>
__device__ __forceinline__ void wino_core(char* __restrict__ ldsb, int vbase,
                                          const __amdgpu_buffer_rsrc_t rW, const __amdgpu_buffer_rsrc_t rN,
                                          const float* __restrict__ bias,
                                          f32x4 (&wr)[WinoCfg<F>::PF][WinoCfg<F>::XS][WinoCfg<F>::NN], int w,
                                          int lane, f32x4 (&y)[WinoCfg<F>::NN][4], bool pre = false,
                                          unsigned long long* tr = nullptr) {
    constexpr int CF = F / 16;
    constexpr int NWV = WinoCfg<F>::NWV, NN = WinoCfg<F>::NN, XS = WinoCfg<F>::XS;
    constexpr int CH = WinoCfg<F>::CH, VBYTES = CH * 1024, XST = CH * 64;   // V buffer, xi stride
    constexpr int IT = CH * 16 / (NWV * 64);                       // transform items per thread per chunk
    // t = (16-channel group kl, point t % 16) pairs of this wave per chunk; a ring step covers XS
    constexpr int NCHUNK = F / CH, KPC = CH / 16, SPC = KPC * 16, SPX = SPC / XS;
    constexpr int PF = WinoCfg<F>::PF, LA = WINO_LA * XS;
    static_assert(NN * 16 * NWV == F && IT * NWV * 64 == CH * 16 && NWV % 4 == 0 && IT >= 1, "Winograd config");
    static_assert(SPX % PF == 0 && SPC % LA == 0 && 16 % XS == 0, "ring slots must be compile-time");
    const int l16 = lane & 15, h = lane >> 4;
    // V[xi][quad cq][tile slot][4]: tile slot = tile ^ 2 (cq & 3).  gfx950 services a ds_read_b128
    // in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32): each group holds quads h and
    // h + 1 of a fragment at complementary tile sets, and the XOR by 2h keeps their 16 slots distinct
    // (64 banks); a ds_write_b32 of the transform (32-lane groups, 32 banks) then covers 8 distinct
    // slot values mod 8, so both are conflict-free (an XOR by 4h, laid out for groups of 16
    // consecutive lanes, made every B-fragment read 2-way: PMC 48 % of LDS cycles were conflicts)
    const int vrd = h * 256 + ((l16 ^ (2 * h)) * 16);               // + xi * XST + k * 1024 (cq = 4k + h, cq & 3 = h)
    const WinoXf<F> xf(ldsb, vbase, w, lane);
    const int co0 = w * 16 * NN + h * 4;
    // (peeling the first chunk so that its MFMAs take C = 0 instead of this zeroing pass made the
    // register allocation spill: 30 VGPRs at F = 256)
    f32x4 acc[16][NN];
#pragma unroll
    for (int x = 0; x < 16; x++)
#pragma unroll
        for (int n = 0; n < NN; n++) {
            if constexpr (F == 256) {   // accumulators in VGPRs: 64-bit moves (the compiler's zeroing was 128 32-bit moves)
                f32x2 z0, z1;
                asm volatile("v_mov_b64 %0, 0" : "=v"(z0));
                asm volatile("v_mov_b64 %0, 0" : "=v"(z1));
                acc[x][n] = f32x4{z0.x, z0.y, z1.x, z1.y};
            } else {                    // F = 64 keeps them in AGPRs, zeroed there directly
                acc[x][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    // weight ring: fragment (16-channel group kc, point xi, co/16 = NN w + n) at ((kc 16 + xi) CF + co/16) KB
    const int voff = wino_voff<F>(w, lane);
    if (!pre) {   // chunk 0 not transformed by the caller
        f32x2 d0[IT][4][2];
        xf.load(0, d0);
        xf.store(0, d0);
        __syncthreads();
    }
    wino_stamp(tr, 1);
    // B fragment of this wave's step t: 16-channel group t / 16 of the chunk, point t % 16
    auto boff = [](int t) { return (t / 16) * 1024 + (t % 16) * XST; };
#pragma unroll 1
    for (int c = 0; c < NCHUNK; c++) {
        f32x2 dn[IT][4][2];
        const int vb = vbase + (c & 1) * VBYTES + vrd;
        const bool more = c + 1 < NCHUNK;
        f32x4 bq[LA];
#pragma unroll
        for (int i = 0; i < LA; i++) bq[i] = *reinterpret_cast<const f32x4*>(ldsb + vb + boff(i));
#pragma unroll
        for (int st = 0; st < SPX; st++) {
            f32x4 B[XS];
#pragma unroll
            for (int xs = 0; xs < XS; xs++) {
                const int t = st * XS + xs;
                B[xs] = bq[t % LA];
                if (t + LA < SPC) bq[t % LA] = *reinterpret_cast<const f32x4*>(ldsb + vb + boff(t + LA));
            }
            f32x4 a[XS][NN];
#pragma unroll
            for (int xs = 0; xs < XS; xs++)
#pragma unroll
                for (int n = 0; n < NN; n++) a[xs][n] = wr[st % PF][xs][n];
            {
                // ring step st + PF: the steps of a conv are linear in the weights; past this
                // conv's last step the refills read the next conv's first steps
                const int cadd = (st + PF) / SPX;
                const bool nxt = cadd > 0 && !more;
                const int tn = c * SPX + st + PF;
                const int to = (nxt ? tn - NCHUNK * SPX : tn) * XS;
                // the step's (wave-uniform) offset rides in the instruction's SGPR offset, the
                // fragment's in the lane offset + immediate: no VALU address arithmetic per load
#pragma unroll
                for (int xs = 0; xs < XS; xs++)
#pragma unroll
                    for (int n = 0; n < NN; n++)
                        wr[st % PF][xs][n] = __builtin_bit_cast(
                            f32x4, __builtin_amdgcn_raw_buffer_load_b128(nxt ? rN : rW, voff + n * 1024,
                                                                         WINO_WSTEP(to + xs) * CF * 1024, 0));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s4 = 0; s4 < 4; s4++)
#pragma unroll
                for (int xs = 0; xs < XS; xs++)
#pragma unroll
                    for (int n = 0; n < NN; n++) {
                        const int x = (st * XS + xs) % 16;
                        acc[x][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[xs][n][s4], B[xs][s4], acc[x][n], 0, 0, 0);
                    }
            __builtin_amdgcn_sched_barrier(0);
            // the next chunk's transform.  F = 256: the first wave of each SIMD pair, which runs ahead
            // of its partner by ~30 % of a chunk, transforms both waves' items after
            // its last step, beside its partner's last MFMAs (C3 A/B: tower -1.1 % against one item
            // per wave at staggered steps); other F: one item per wave, the two waves of a SIMD pair
            // WINO_TSTAG steps apart (a stagger that would not fit in this F's chunk is dropped)
            if (st == 4) wino_stamp(tr, 20 + c);
            if constexpr (F == 256) {
                (void)dn;
                if (st == SPX - 1 && more && w < NWV / 2) xf.both(c + 1, (c + 1) & 1);
            } else {
                constexpr int TSG = (WINO_TSTAG + WINO_TSPLIT) / XS < SPX ? WINO_TSTAG : 0;
                const bool late = TSG > 0 && w >= NWV / 2;
                if (st == 0 && more && !late) xf.load(c + 1, dn);
                if (TSG > 0 && st == TSG / XS && more && late) xf.load(c + 1, dn);
                if (st == WINO_TSPLIT / XS && more && !late) xf.store((c + 1) & 1, dn);
                if (TSG > 0 && st == (TSG + WINO_TSPLIT) / XS && more && late) xf.store((c + 1) & 1, dn);
            }
        }
        wino_stamp(tr, 12 + c);
        // no barrier after the last chunk: the last transform reads of ACT and writes of V were
        // ordered by the previous chunk's barrier, so the waves that finish first start their
        // output transform beside the others' last MFMAs (C3 A/B: tower -0.6 %)
        if (more) __syncthreads();
        wino_stamp(tr, 2 + c);
    }
    // output transform Y = A^T M A per (output fragment n, channel pair), + bias: the two channels
    // of a pair sit in consecutive accumulator registers, so every add is one v_pk_add_f32
#pragma unroll
    for (int n = 0; n < NN; n++) {
        const f32x4 bb = bias ? *reinterpret_cast<const f32x4*>(bias + co0 + n * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < 2; p++) {
            f32x2 m[16];
#pragma unroll
            for (int x = 0; x < 16; x++) m[x] = p ? f32x2{acc[x][n][2], acc[x][n][3]} : f32x2{acc[x][n][0], acc[x][n][1]};
            const f32x2 br = p ? f32x2{bb[2], bb[3]} : f32x2{bb[0], bb[1]};
            f32x2 s0[4], s1[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s0[j] = pk_add(pk_add(m[j], m[4 + j]), m[8 + j]);
                s1[j] = pk_sub(pk_sub(m[4 + j], m[8 + j]), m[12 + j]);
            }
            const f32x2 q0 = pk_add(pk_add(pk_add(s0[0], s0[1]), s0[2]), br);
            const f32x2 q1 = pk_add(pk_sub(pk_sub(s0[1], s0[2]), s0[3]), br);
            const f32x2 q2 = pk_add(pk_add(pk_add(s1[0], s1[1]), s1[2]), br);
            const f32x2 q3 = pk_add(pk_sub(pk_sub(s1[1], s1[2]), s1[3]), br);
            y[n][0][2 * p] = q0.x; y[n][0][2 * p + 1] = q0.y;
            y[n][1][2 * p] = q1.x; y[n][1][2 * p + 1] = q1.y;
            y[n][2][2 * p] = q2.x; y[n][2][2 * p + 1] = q2.y;
            y[n][3][2 * p] = q3.x; y[n][3][2 * p + 1] = q3.y;
        }
    }
}

// ====================================================================== split-f16 point GEMMs
// wino_core_h16: wino_core (any WinoCfg<F>) with the 16 point GEMMs on v_mfma_f32_16x16x32_f16 (16 issue
// cycles for K = 32, against 8 x 32 for the f32 MFMA).  Each f32 factor is scaled by a power of two
// and split into two f16 (11-bit significands), x = hi + lo to 22 bits, and the product is
// hi hi + hi lo + lo hi, accumulated in f32: the dropped lo lo term is below 2^-22 relative, less
// than the rounding of the f32 accumulation (tools/split16_numerics.py).  Same tiling, ACT,
// accumulator / output layout, residual and epilogue as wino_core (the MFMA C/D layout does not
// depend on the input type); differences:
//   V        two f16 planes per chunk (WinoXf::store16), the same 1 KB per channel of the chunk;
//   weights  [32-channel group][xi][co/16][hi, lo][64 lanes][8] f16 (net.hip winograd_split16), lane
//            = co % 16 + 16 (ci % 32 / 8), scaled per conv by Sw: the same 4 bytes per weight;
//   step     XS points x 32 channels (WinoRing<F, true>): per point 2 NN weight fragments (output
//            fragments x hi, lo), 2 B fragments, 3 NN MFMAs.  F = 256: one point, the two output
//            fragments' chains interleaved; F = 128, 64: two points, one chain each.  A chunk is
//            CH / 32 groups of 32 channels x 16 points, in the weights' order (group, point);
//   F = 128  the next chunk's transform one item per wave, the second wave of each SIMD pair half a
//            chunk after the first (wino_core's schedule; its 16-step stagger does not fit in the 8
//            steps of a chunk here);
//   F = 64   the single 64-channel chunk (two groups) in the V buffer the caller chose; the first
//            conv's transform is WinoXf::store16 (4 items per thread), every other conv's was done
//            by the conv before it from registers (wino_xform_regs<F, true>);
//   unscale  the conv's 1 / (Sa Sw), a power of two (exact), folded into the output transform's
//            bias add as one packed FMA.
//   SP = 12  (F = 256, AZ_WINO_DERIVE) 12 of the 16 points' weights are streamed, a chunk is 12 ring
//            steps instead of 16.  G's rows satisfy r1 + r2 = r0 + r3, so U[2][b] = U[0][b] + U[3][b] -
//            U[1][b], and by linearity M[2][b] = (U[0][b] + U[3][b] - U[1][b]) V[2][b].  The steps come
//            in the order [b][a = 0, 1, 3] (net.hip winograd_split16); while the A fragments of (a, b)
//            are in the ring for their own point they are used a second time against V[2][b], into
//            the accumulators of point (2, b): 12 MFMAs per step, in a pipe that the weight stream
//            leaves idle three quarters of the time.  Row 1 of the weights is stored negated and the
//            input transform negates row 1 of V (WinoXf::store16<true>): the own product is unchanged
//            and the derived point's three terms are all additions.
//   ROWS     (F = 256, SP = 12, AZ_WINO_ROWS) Winograd across columns only, a direct 3-tap correlation
//            across rows: W[k][b] = (g G^T)[k][b] for the 3 tap rows, D[i][b] = (d B)[i][b] for the 4 raw
//            patch rows (WinoXf::xform_cols), and the output transform's row sums are accumulated
//            directly: s0[b] = sum_k W[k][b] D[k][b], s1[b] = sum_k W[k][b] D[k + 1][b] -- 8 accumulators
//            per output fragment instead of 16.  The same 12 streamed planes (step 3 b + k, nothing
//            negated), 16 V planes (4 i + b) and 12 MFMAs per step in four chains as the derived form;
//            the input transform loses its row pass, the output transform its first stage, and no
//            product is derived.  The registers that frees hold a deeper ring (WinoRing).
//   VROWS    (ROWS, AZ_WINO_VROWS) V holds every D row of the padded board once (wino_vr_* above: 20 KB per
//            chunk instead of 32) instead of the four patch rows of every tile; the transform is 16 small
//            wave-items per chunk (WinoXf::vrows) and does half the arithmetic and LDS writes.  The B
//            fragment of (patch row i, point b) is entry (b, 2 tr + i, h, tc): the same bits into the same
//            MFMAs.  The phase trace put the tail transform of waves 0-3 on the chunk's
//            critical path -- they request no weights while they transform and are last at every chunk
//            barrier -- so it stays where it was and gets shorter (AZ_WINO_VROWS_SCHED 0); spreading it
//            over all eight waves inside the steps (1) measured slower: it loads the late waves.
template <int F, int SP = 16, bool ROWS = false, bool VROWS = false>
__device__ __forceinline__ void wino_core_h16(char* __restrict__ ldsb, int vbase,
                                              const __amdgpu_buffer_rsrc_t rW, const __amdgpu_buffer_rsrc_t rN,
                                              const float* __restrict__ bias, float unscale,
                                              f32x4 (&wr)[WinoRing<F, true, ROWS>::PF][WinoRing<F, true>::RX][WinoCfg<F>::NN],
                                              int w, int lane, f32x4 (&y)[WinoCfg<F>::NN][4], bool pre = false,
                                              unsigned long long* tr = nullptr) {
    constexpr int CF = F / 16;
    constexpr int NWV = WinoCfg<F>::NWV, NN = WinoCfg<F>::NN, CH = WinoCfg<F>::CH;
    constexpr int PF = WinoRing<F, true, ROWS>::PF, XS = WinoRing<F, true>::XS;
    // t = (32-channel group t / 16, point t % 16) pairs of a chunk; a ring step covers XS
    constexpr bool DER = SP == 12 && !ROWS;
    static_assert(SP == 16 || (SP == 12 && XS == 1 && CH == 32), "12 streamed planes: one per step, one group per chunk");
    static_assert(!ROWS || (SP == 12 && F == 256), "the row-direct form: 256 filters, 12 streamed planes");
    static_assert(!VROWS || ROWS, "shared V rows: the row-direct form only");
    constexpr bool VSTEPS = VROWS && AZ_WINO_VROWS_SCHED == 1;       // the transform inside the steps, all waves
    constexpr int NACC = ROWS ? 8 : 16;
    constexpr int XFORM = ROWS ? WINO_XF_COLS : DER ? WINO_XF_NEG1 : WINO_XF_FULL;
    constexpr int VBYTES = CH * 1024, NCHUNK = F / CH, SPC = (CH / 32) * 16, SPX = SP == 12 ? 12 : SPC / XS;
    constexpr int XST16 = WinoXf<F>::XST16;                          // bytes of a point in a plane
    constexpr int STEPB = CF * 2 * 1024;                             // weight bytes of a (group, point)
    // ring steps of B fragments read ahead.  F = 256: a step lasts ~700 cycles at the weight stream's
    // rate, one is enough, and 2 spilled 12 more VGPRs per block (C3 A/B: tower 13.0-13.3 ms against
    // 13.4-13.7); a two-point step is 96 cycles of MFMA issue, below the LDS latency: 2 (with 1,
    // tower32w_kernel<128> spilled 6 VGPRs in front of the chunk loop; with 2 it needs no scratch)
    constexpr int LA = XS == 1 ? 1 : 2;
    static_assert(CH % 32 == 0 && SPX % PF == 0 && SPX % LA == 0 && 16 % XS == 0, "ring slots must be compile-time");
    const int l16 = lane & 15, h = lane >> 4;
    const int vrd = h * 256 + ((l16 ^ (2 * h)) * 16);                // hi plane; lo: slot ^ 4, + VBYTES / 2
    const int vrl = VBYTES / 2 + h * 256 + ((l16 ^ (2 * h) ^ 4) * 16);
    // shared rows: the lane's part of the read address for patch rows 0, 1 (vrd) and 2, 3 (vrl), hi plane
    const int vr0 = VROWS ? wino_vr_rlane(lane, 0) : vrd, vr1 = VROWS ? wino_vr_rlane(lane, 1) : vrl;   // vr1 = (vr0 ^ 128) + 256
    constexpr int VBUF = VROWS ? WINO_VR_BYTES : VBYTES;             // bytes of a chunk's V buffer
    const WinoXf<F> xf(ldsb, vbase, w, lane);
    const int co0 = w * 16 * NN + h * 4;
    f32x4 acc[NACC][NN];
#pragma unroll
    for (int x = 0; x < NACC; x++)
#pragma unroll
        for (int n = 0; n < NN; n++) {
            if constexpr (F == 256) {   // accumulators in VGPRs: 64-bit moves (see wino_core)
                f32x2 z0, z1;
                asm volatile("v_mov_b64 %0, 0" : "=v"(z0));
                asm volatile("v_mov_b64 %0, 0" : "=v"(z1));
                acc[x][n] = f32x4{z0.x, z0.y, z1.x, z1.y};
            } else {
                acc[x][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    const int voff = wino16_voff<F>(w, lane);
    if (!pre) {   // chunk 0 not transformed by the caller
        if constexpr (VROWS) {
            xf.template vrows<NWV>(0, 0);
        } else {
            typename WinoXf<F>::Patch d0;
            xf.load(0, d0);
            xf.template store16<XFORM>(0, d0);
        }
        __syncthreads();
    }
    wino_stamp(tr, 1);
    // the (group, point) t of step st, point xs: the weights' order.  12 streamed points: column
    // st / 3, row 0, 1, 3
    auto tof = [](int st, int xs) { return DER ? 4 * ((st % 3) + (st % 3) / 2) + st / 3 : st * XS + xs; };
    // B fragment of (group, point) t: octets 4 (t / 16) + h of point t % 16
    auto boff = [](int t) { return (t / 16) * 1024 + (t % 16) * XST16; };
#pragma unroll 1
    for (int c = 0; c < NCHUNK; c++) {
        typename WinoXf<F>::Patch dn;
        const int vb = vbase + (c & 1) * VBUF;
        const bool more = c + 1 < NCHUNK;
        if constexpr (ROWS) {
            // row-direct form.  B fragments: a rolling window of three planes, numbered n = 4 b + i in the
            // order the steps meet them (V point 4 i + b), slot n % 3.  Step (b, k) multiplies planes n0 =
            // 4 b + k and n0 + 1; plane n0 + 2 is read at the top of the step into the slot the previous
            // step freed, and after a column's last products the next column's second plane into the slot
            // just freed: 24 VGPRs, every read at least a step ahead of its use
            (void)dn;
            f16x8 bw[3][2];
            float en[2][4];                                          // VSTEPS: the wave's two items of chunk c + 1
            auto bread = [&](int n) {
                if constexpr (VROWS) {   // patch row n % 4 of point n / 4: entry (b, 2 tr + i, h, tc)
                    const int vl = (n % 4) >> 1 ? vr1 : vr0;
                    const char* p = ldsb + vb + wino_vr_rimm(n % 4, n / 4);
                    bw[n % 3][0] = *reinterpret_cast<const f16x8*>(p + vl);
                    bw[n % 3][1] = *reinterpret_cast<const f16x8*>(p + wino_vr_lo(vl));
                } else {
                    const int pt = 4 * (n % 4) + n / 4;
                    bw[n % 3][0] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrd + pt * XST16);
                    bw[n % 3][1] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrl + pt * XST16);
                }
            };
            bread(0);
            bread(1);
#pragma unroll
            for (int st = 0; st < SPX; st++) {
                const int b = st / 3, n0 = 4 * b + st % 3;
                if (n0 + 2 < 16) bread(n0 + 2);
                f16x8 a[2][NN];
#pragma unroll
                for (int pl = 0; pl < 2; pl++)
#pragma unroll
                    for (int n = 0; n < NN; n++) a[pl][n] = __builtin_bit_cast(f16x8, wr[st % PF][pl][n]);
                {
                    // ring step st + PF; past this conv's last step the refills read the next conv's first
                    const bool nxt = st + PF >= SPX && !more;
                    const int tn = c * SPX + st + PF;
                    const int to = nxt ? tn - NCHUNK * SPX : tn;
#pragma unroll
                    for (int pl = 0; pl < 2; pl++)
#pragma unroll
                        for (int n = 0; n < NN; n++)
                            wr[st % PF][pl][n] = __builtin_bit_cast(
                                f32x4, __builtin_amdgcn_raw_buffer_load_b128(nxt ? rN : rW, voff + (2 * n + pl) * 1024,
                                                                             to * STEPB, 0));
                }
                __builtin_amdgcn_sched_barrier(0);
                // W[k][b] against D[k][b] into s0[b] and against D[k + 1][b] into s1[b]: hi hi, hi lo, lo hi
                // of each, four chains interleaved
#pragma unroll
                for (int term = 0; term < 3; term++)
#pragma unroll
                    for (int pt = 0; pt < 2; pt++)
#pragma unroll
                        for (int n = 0; n < NN; n++) {
                            const f16x8 av = a[term == 2 ? 1 : 0][n];
                            const f16x8 bv = bw[(n0 + pt) % 3][term == 1 ? 1 : 0];
                            acc[4 * pt + b][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc[4 * pt + b][n], 0, 0, 0);
                        }
                __builtin_amdgcn_sched_barrier(0);
                if (st % 3 == 2 && st + 1 < SPX) bread(n0 + 3);
                if (st == 4) wino_stamp(tr, 20 + c);
                // the next chunk's transform: as in wino_core, by the first wave of each SIMD pair; shared rows:
                // the same (AZ_WINO_VROWS_SCHED 0: 4 items per wave), or every wave's two items inside the steps,
                // reads two steps ahead of the transform and writes (1), so that no wave stops requesting
                // weights; V[(c + 1) & 1] is free since the previous chunk's barrier
                if constexpr (VSTEPS) {
                    if (more) {
                        if (st == 1) xf.vr_load(c + 1, wino_vr_item(w, 0, NWV), en[0], vgpr_index(lane));
                        if (st == 3) xf.vr_store((c + 1) & 1, wino_vr_item(w, 0, NWV), en[0], vgpr_index(lane));
                        if (st == 5) xf.vr_load(c + 1, wino_vr_item(w, 1, NWV), en[1], vgpr_index(lane));
                        if (st == 7) xf.vr_store((c + 1) & 1, wino_vr_item(w, 1, NWV), en[1], vgpr_index(lane));
                    }
                } else if constexpr (VROWS) {
                    (void)en;
                    if (st == SPX - 1 && more && w < NWV / 2) {
                        if (c < 4) wino_stamp(tr, 28 + c);   // start of the tail transform (chunks 0-3: the free slots)
                        xf.template vrows<NWV / 2>(c + 1, (c + 1) & 1);
                    }
                } else {
                    (void)en;
                    if (st == SPX - 1 && more && w < NWV / 2) {
                        if (c < 4) wino_stamp(tr, 28 + c);
                        xf.template both<true, XFORM>(c + 1, (c + 1) & 1);
                    }
                }
            }
        } else {
            f16x8 bq[LA][XS][2];
#pragma unroll
            for (int i = 0; i < LA; i++)
#pragma unroll
                for (int xs = 0; xs < XS; xs++) {
                    bq[i][xs][0] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrd + boff(tof(i, xs)));
                    bq[i][xs][1] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrl + boff(tof(i, xs)));
                }
            // 12 streamed points: the B fragments of the derived point (2, b), held for the three steps of
            // column b and refilled for column b + 1 once that column's last products have issued (read
            // inside every step after the own products, in the own point's registers, they spilled 8
            // VGPRs fewer and left the LDS latency exposed once per step: C3 A/B tower 12.63 ms against
            // 12.42)
            f16x8 dq[2];
            if constexpr (DER) {
                dq[0] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrd + boff(8));
                dq[1] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrl + boff(8));
            } else {
                (void)dq;
            }
#pragma unroll
            for (int st = 0; st < SPX; st++) {
                f16x8 bh[XS], bl[XS];
#pragma unroll
                for (int xs = 0; xs < XS; xs++) {
                    bh[xs] = bq[st % LA][xs][0];
                    bl[xs] = bq[st % LA][xs][1];
                    if (st + LA < SPX) {
                        bq[st % LA][xs][0] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrd + boff(tof(st + LA, xs)));
                        bq[st % LA][xs][1] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrl + boff(tof(st + LA, xs)));
                    }
                }
                f16x8 a[XS][2][NN];
#pragma unroll
                for (int xs = 0; xs < XS; xs++)
#pragma unroll
                    for (int pl = 0; pl < 2; pl++)
#pragma unroll
                        for (int n = 0; n < NN; n++) a[xs][pl][n] = __builtin_bit_cast(f16x8, wr[st % PF][2 * xs + pl][n]);
                {
                    // ring step st + PF; past this conv's last step the refills read the next conv's first
                    const bool nxt = st + PF >= SPX && !more;
                    const int tn = c * SPX + st + PF;
                    const int to = (nxt ? tn - NCHUNK * SPX : tn) * XS;
#pragma unroll
                    for (int xs = 0; xs < XS; xs++)
#pragma unroll
                        for (int pl = 0; pl < 2; pl++)
#pragma unroll
                            for (int n = 0; n < NN; n++)
                                wr[st % PF][2 * xs + pl][n] = __builtin_bit_cast(
                                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(nxt ? rN : rW, voff + (2 * n + pl) * 1024,
                                                                                 (to + xs) * STEPB, 0));
                }
                __builtin_amdgcn_sched_barrier(0);
                // hi hi, hi lo, lo hi of each (point, output fragment), the step's two chains interleaved;
                // 12 streamed points: the same A fragments also against V[2][st / 3], into the derived
                // point's accumulators (four chains)
                constexpr int NP = DER ? 2 : 1;
#pragma unroll
                for (int term = 0; term < 3; term++)
#pragma unroll
                    for (int xs = 0; xs < XS; xs++)
#pragma unroll
                        for (int pt = 0; pt < NP; pt++)
#pragma unroll
                            for (int n = 0; n < NN; n++) {
                                const int x = pt ? 8 + st / 3 : tof(st, xs) % 16;
                                const f16x8 av = a[xs][term == 2 ? 1 : 0][n];
                                const f16x8 bv = pt ? dq[term == 1 ? 1 : 0] : (term == 1 ? bl[xs] : bh[xs]);
                                acc[x][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc[x][n], 0, 0, 0);
                            }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (DER) {
                    if (st % 3 == 2 && st + 1 < SPX) {
                        dq[0] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrd + boff(8 + (st + 1) / 3));
                        dq[1] = *reinterpret_cast<const f16x8*>(ldsb + vb + vrl + boff(8 + (st + 1) / 3));
                    }
                }
                if (st == 4 / XS) wino_stamp(tr, 20 + c);
                if constexpr (F == 256) {
                    // the next chunk's transform: as in wino_core, by the first wave of each SIMD pair
                    (void)dn;
                    if (st == SPX - 1 && more && w < NWV / 2) xf.template both<true, XFORM>(c + 1, (c + 1) & 1);
                } else if constexpr (NCHUNK > 1) {
                    constexpr int TSP = WINO_TSPLIT / XS, TSG = SPX / 2;
                    static_assert(TSP >= 1 && TSG + TSP < SPX, "the late waves' transform ends inside the chunk");
                    const bool late = w >= NWV / 2;
                    if (st == 0 && more && !late) xf.load(c + 1, dn);
                    if (st == TSG && more && late) xf.load(c + 1, dn);
                    if (st == TSP && more && !late) xf.store16((c + 1) & 1, dn);
                    if (st == TSG + TSP && more && late) xf.store16((c + 1) & 1, dn);
                } else {
                    (void)dn;
                }
            }
        }
        wino_stamp(tr, 12 + c);
        if (more) __syncthreads();   // (none after the last chunk: see wino_core)
        wino_stamp(tr, 2 + c);
    }
    // output transform Y = A^T M A per (output fragment n, channel pair), x unscale + bias
    const f32x2 us = f32x2{unscale, unscale};
#pragma unroll
    for (int n = 0; n < NN; n++) {
        const f32x4 bb = bias ? *reinterpret_cast<const f32x4*>(bias + co0 + n * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < 2; p++) {
            f32x2 m[NACC];
#pragma unroll
            for (int x = 0; x < NACC; x++) m[x] = p ? f32x2{acc[x][n][2], acc[x][n][3]} : f32x2{acc[x][n][0], acc[x][n][1]};
            const f32x2 br = p ? f32x2{bb[2], bb[3]} : f32x2{bb[0], bb[1]};
            f32x2 s0[4], s1[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if constexpr (ROWS) {   // the row sums were accumulated directly
                    s0[j] = m[j];
                    s1[j] = m[4 + j];
                } else {
                    s0[j] = pk_add(pk_add(m[j], m[4 + j]), m[8 + j]);
                    s1[j] = pk_sub(pk_sub(m[4 + j], m[8 + j]), m[12 + j]);
                }
            }
            const f32x2 q0 = pkc_fma(pk_add(pk_add(s0[0], s0[1]), s0[2]), us, br);
            const f32x2 q1 = pkc_fma(pk_sub(pk_sub(s0[1], s0[2]), s0[3]), us, br);
            const f32x2 q2 = pkc_fma(pk_add(pk_add(s1[0], s1[1]), s1[2]), us, br);
            const f32x2 q3 = pkc_fma(pk_sub(pk_sub(s1[1], s1[2]), s1[3]), us, br);
            y[n][0][2 * p] = q0.x; y[n][0][2 * p + 1] = q0.y;
            y[n][1][2 * p] = q1.x; y[n][1][2 * p + 1] = q1.y;
            y[n][2][2 * p] = q2.x; y[n][2][2 * p + 1] = q2.y;
            y[n][3][2 * p] = q3.x; y[n][3][2 * p + 1] = q3.y;
        }
    }
}

// ====================================================================== two boards per workgroup
// wino_core_b2 (AZ_WINO_BOARDS = 2): the row-direct shared-row form (wino_core_h16<256, 12, true, true>) on two
// boards at once.  Every A fragment the ring delivers feeds both boards' B fragments, so a CU pulls the
// conv's weights from L2 once per pair of boards instead of once per board; per board the products, their
// order and K are the one-board kernel's, so each board's result is bit-equal to it.
//   ACT      lives in global memory (L2-resident): per workgroup and board two buffers X (block input /
//            output) and H (conv 1's output) in ACT's [64 squares][66 slots] f32 layout (WINO_B2_*), read
//            and written through a buffer descriptor of the workgroup's WINO_B2_WG bytes; the wino_vr_a*
//            address functions apply unchanged from the buffer's offset.  LDS holds only V;
//   V        two buffers per board, board nb's buffer `buf` at (2 nb + buf) WINO_VR_BYTES: 80 KB;
//   step     12 MFMAs per board, board 0's then board 1's; each board's four B fragments (planes n0 and
//            n0 + 1, hi and lo: 16 VGPRs) are held for the step at hand, and what the next step needs of
//            them is read as soon as the board's MFMAs have issued, i.e. one board ahead;
//   ring     WINO_B2_PF steps, each slot refilled after the step's MFMAs have read it (no copy);
//   items    the next chunk's transform inside the steps, one item at a time: item k's four global reads at
//            the top of step k, its transform and V writes at the top of step k + 1 -- a step of MFMAs covers
//            the L2 round trip, 4 VGPRs in flight.  The matrix pipe serves the first wave of each SIMD pair
//            first: with the 32 items spread evenly (4 per wave) waves 0-3 ran 3,400 cycles per chunk ahead of
//            their partners and waited 3,800 at every chunk barrier, while a wave alone on its SIMD runs at
//            the loads' latency, not at the pipe's rate; with all 32 on waves 0-3 (8 each) those arrived
//            2,600 cycles late.  They take WINO_B2_XE = 6 each and waves 4-7 two (profiles/boards2_trace.txt).
// The accumulators are returned to the caller (tower.hip conv_wino_b2), whose epilogue reads the residual
// from global ACT once they are dead.
constexpr int WINO_B2_ACT = 64 * WINO_VR_R16;          // one ACT buffer, 67,584 B
constexpr int WINO_B2_BOARD = 2 * WINO_B2_ACT;         // X, then H
constexpr int WINO_B2_WG = 2 * WINO_B2_BOARD;          // 270,336 B of global ACT per workgroup
constexpr int WINO_B2_VBYTES = 4 * WINO_VR_BYTES;      // the four V buffers
#ifndef AZ_WINO_B2_PF
#define AZ_WINO_B2_PF 3
#endif
constexpr int WINO_B2_PF = AZ_WINO_B2_PF;
static_assert(12 % WINO_B2_PF == 0 && WINO_B2_PF >= 2, "the ring's slots must be compile-time");
// byte offset of board nb's buffer (0: X, 1: H) in the workgroup's global ACT, of its V buffer in LDS
__host__ __device__ constexpr int wino_b2_act(int nb, int hbuf) { return nb * WINO_B2_BOARD + hbuf * WINO_B2_ACT; }
__host__ __device__ constexpr int wino_b2_v(int nb, int buf) { return (2 * nb + buf) * WINO_VR_BYTES; }
// the epilogue's access of wave w's lane (conv_wino's out_addr): output fragment n, square q of the lane's tile
// (2 ty + q / 2, 2 tx + q % 2), channels 32 w + 16 n + 4 (lane >> 4) .. + 3, bytes within an ACT buffer
__host__ __device__ constexpr int wino_b2_out(int w, int lane, int n, int q) {
    const int l16 = lane & 15, ty = l16 >> 2, tx = l16 & 3;
    return ((2 * ty + (q >> 1)) * 8 + 2 * tx + (q & 1)) * WINO_VR_R16 + (w * 32 + (lane >> 4) * 4 + n * 16) * 4;
}
// the in-step schedule: a chunk's 32 items g = 16 board + wave-item; each of waves 0-3 takes WINO_B2_XE of
// them (g = w + 4 k), each of waves 4-7 the rest (WINO_B2_XL = 8 - WINO_B2_XE each)
#ifndef AZ_WINO_B2_XE
#define AZ_WINO_B2_XE 6
#endif
constexpr int WINO_B2_XE = AZ_WINO_B2_XE, WINO_B2_XL = 8 - WINO_B2_XE;
static_assert(WINO_B2_XE >= 4 && WINO_B2_XE <= 8, "waves 0-3 take at least their share, at most everything");
__host__ __device__ constexpr int wino_b2_item_count(int w) { return w < 4 ? WINO_B2_XE : WINO_B2_XL; }
__host__ __device__ constexpr int wino_b2_item_g(int w, int k) { return w < 4 ? w + 4 * k : 4 * WINO_B2_XE + (w - 4) + 4 * k; }
__host__ __device__ constexpr int wino_b2_item_board(int w, int k) { return wino_b2_item_g(w, k) >> 4; }
__host__ __device__ constexpr int wino_b2_item_q(int w, int k) { return wino_b2_item_g(w, k) & 15; }

// wave-item q of chunk c from the global ACT buffer at byte offset aoff: the four reads of WinoXf::vr_load
__device__ __forceinline__ void wino_b2_load(const __amdgpu_buffer_rsrc_t rA, int aoff, int c, int q, float (&e)[4], int ln) {
    const int tl = ln >> 4;
    const int p = wino_vr_alane(ln) + wino_vr_auni(q) + c * 128 + aoff;
#pragma unroll
    for (int j = 0; j < 4; j++)
        e[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rA, p + wino_vr_acol(tl, j), 0, 0));
}
// chunk c of both boards into their V buffers `buf` by the first NW waves, every read issued before the
// first transform (for use where the accumulators are dead: 4 x 2 x 16 / NW VGPRs of patch values)
template <int NW>
__device__ __forceinline__ void wino_b2_items(char* __restrict__ ldsv, const __amdgpu_buffer_rsrc_t rA, int hbuf, int c,
                                              int buf, int w, int lane) {
    constexpr int NI = WINO_VR_ITEMS / NW;
    const int ln = vgpr_index(lane);
    float e[2][NI][4];
#pragma unroll
    for (int nb = 0; nb < 2; nb++)
#pragma unroll
        for (int i = 0; i < NI; i++) wino_b2_load(rA, wino_b2_act(nb, hbuf), c, wino_vr_item(w, i, NW), e[nb][i], ln);
#pragma unroll
    for (int nb = 0; nb < 2; nb++) {
        const WinoXf<256> xf(ldsv, wino_b2_v(nb, 0), w, lane);
#pragma unroll
        for (int i = 0; i < NI; i++) xf.vr_store(buf, wino_vr_item(w, i, NW), e[nb][i], ln);
    }
}

// the output transform of the row-direct form for one board's output fragment n: wino_core_h16's, operation
// for operation
__device__ __forceinline__ void wino_rows_out(const f32x4 (&acc)[8][2], const float* __restrict__ bias, float unscale,
                                              int co0, int n, f32x4 (&y)[4]) {
    const f32x2 us = f32x2{unscale, unscale};
    {
        const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + co0 + n * 16);
#pragma unroll
        for (int p = 0; p < 2; p++) {
            f32x2 s0[4], s1[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s0[j] = p ? f32x2{acc[j][n][2], acc[j][n][3]} : f32x2{acc[j][n][0], acc[j][n][1]};
                s1[j] = p ? f32x2{acc[4 + j][n][2], acc[4 + j][n][3]} : f32x2{acc[4 + j][n][0], acc[4 + j][n][1]};
            }
            const f32x2 br = p ? f32x2{bb[2], bb[3]} : f32x2{bb[0], bb[1]};
            const f32x2 q0 = pkc_fma(pk_add(pk_add(s0[0], s0[1]), s0[2]), us, br);
            const f32x2 q1 = pkc_fma(pk_sub(pk_sub(s0[1], s0[2]), s0[3]), us, br);
            const f32x2 q2 = pkc_fma(pk_add(pk_add(s1[0], s1[1]), s1[2]), us, br);
            const f32x2 q3 = pkc_fma(pk_sub(pk_sub(s1[1], s1[2]), s1[3]), us, br);
            y[0][2 * p] = q0.x; y[0][2 * p + 1] = q0.y;
            y[1][2 * p] = q1.x; y[1][2 * p + 1] = q1.y;
            y[2][2 * p] = q2.x; y[2][2 * p + 1] = q2.y;
            y[3][2 * p] = q3.x; y[3][2 * p + 1] = q3.y;
        }
    }
}

// ldsv: the four V buffers; rA: the workgroup's global ACT, hin: the conv's input buffer (0: X, 1: H);
// pre: chunk 0 is in V already (conv_wino_b2's hand-off); acc[nb]: board nb's eight row sums per fragment
__device__ __forceinline__ void wino_core_b2(char* __restrict__ ldsv, const __amdgpu_buffer_rsrc_t rW,
                                             const __amdgpu_buffer_rsrc_t rN, const __amdgpu_buffer_rsrc_t rA, int hin,
                                             f32x4 (&wr)[WINO_B2_PF][2][2], int w, int lane, bool pre,
                                             f32x4 (&acc)[2][8][2], unsigned long long* tr = nullptr) {
    constexpr int F = 256, CF = F / 16, NN = 2, PF = WINO_B2_PF, NCHUNK = 8, SPX = 12, STEPB = CF * 2 * 1024;
    const int vr0 = wino_vr_rlane(lane, 0), vr1 = wino_vr_rlane(lane, 1);
#pragma unroll
    for (int nb = 0; nb < 2; nb++)
#pragma unroll
        for (int x = 0; x < 8; x++)
#pragma unroll
            for (int n = 0; n < NN; n++) {
                f32x2 z0, z1;
                asm volatile("v_mov_b64 %0, 0" : "=v"(z0));
                asm volatile("v_mov_b64 %0, 0" : "=v"(z1));
                acc[nb][x][n] = f32x4{z0.x, z0.y, z1.x, z1.y};
            }
    const int voff = wino16_voff<F>(w, lane);
    if (!pre) {   // chunk 0 not transformed by the caller
        wino_b2_items<8>(ldsv, rA, hin, 0, 0, w, lane);
        __syncthreads();
    }
    wino_stamp(tr, 1);
#pragma unroll 1
    for (int c = 0; c < NCHUNK; c++) {
        const bool more = c + 1 < NCHUNK;
        // planes numbered n = 4 b + i in the order the steps meet them (wino_core_h16), plane n in slot n % 2:
        // step (b, k) multiplies planes n0 = 4 b + k and n0 + 1; the next step of the column keeps n0 + 1 and
        // reads n0 + 2 into the slot n0 leaves, a new column reads both
        f16x8 bw[2][2][2];                                           // [board][slot][hi, lo]
        float en[4];                                                 // the item in flight
        auto bread = [&](int nb, int st) {
            const char* vb = ldsv + wino_b2_v(nb, c & 1);
#pragma unroll
            for (int s = st % 3 == 0 ? 0 : 1; s < 2; s++) {
                const int n = 4 * (st / 3) + st % 3 + s;             // patch row n % 4 of point n / 4
                const int vl = (n % 4) >> 1 ? vr1 : vr0;
                const char* p = vb + wino_vr_rimm(n % 4, n / 4);
                bw[nb][n % 2][0] = *reinterpret_cast<const f16x8*>(p + vl);
                bw[nb][n % 2][1] = *reinterpret_cast<const f16x8*>(p + wino_vr_lo(vl));
            }
        };
        bread(0, 0);
        bread(1, 0);
#pragma unroll
        for (int st = 0; st < SPX; st++) {
            const int b = st / 3;
            // the next chunk's items (waves 0-3): item st - 1 into V[(c + 1) & 1], free since the previous chunk's
            // barrier, then item st's reads -- issued before the step's refill, so that the wait a step later
            // leaves the ring's loads in flight
            if (more) {
                if (st >= 1 && st <= wino_b2_item_count(w)) {
                    const WinoXf<F> xf(ldsv, wino_b2_v(wino_b2_item_board(w, st - 1), 0), w, lane);
                    xf.vr_store((c + 1) & 1, wino_b2_item_q(w, st - 1), en, vgpr_index(lane));
                }
                if (st < wino_b2_item_count(w))
                    wino_b2_load(rA, wino_b2_act(wino_b2_item_board(w, st), hin), c + 1, wino_b2_item_q(w, st), en, vgpr_index(lane));
            }
#pragma unroll
            for (int nb = 0; nb < 2; nb++) {
                __builtin_amdgcn_sched_barrier(0);
                // W[k][b] against D[k][b] into s0[b] and against D[k + 1][b] into s1[b]: hi hi, hi lo, lo hi of
                // each, four chains interleaved (wino_core_h16's order)
#pragma unroll
                for (int term = 0; term < 3; term++)
#pragma unroll
                    for (int pt = 0; pt < 2; pt++)
#pragma unroll
                        for (int n = 0; n < NN; n++) {
                            const f16x8 av = __builtin_bit_cast(f16x8, wr[st % PF][term == 2 ? 1 : 0][n]);
                            const f16x8 bv = bw[nb][(4 * b + st % 3 + pt) % 2][term == 1 ? 1 : 0];
                            acc[nb][4 * pt + b][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc[nb][4 * pt + b][n], 0, 0, 0);
                        }
                __builtin_amdgcn_sched_barrier(0);
                if (nb == 1) {
                    // ring step st + PF into the slot just read; past this conv's last step the next conv's first
                    const bool nxt = st + PF >= SPX && !more;
                    const int tn = c * SPX + st + PF;
                    const int to = nxt ? tn - NCHUNK * SPX : tn;
#pragma unroll
                    for (int pl = 0; pl < 2; pl++)
#pragma unroll
                        for (int n = 0; n < NN; n++)
                            wr[st % PF][pl][n] = __builtin_bit_cast(
                                f32x4, __builtin_amdgcn_raw_buffer_load_b128(nxt ? rN : rW, voff + (2 * n + pl) * 1024,
                                                                             to * STEPB, 0));
                }
                if (st + 1 < SPX) bread(nb, st + 1);
            }
            if (st == 4) wino_stamp(tr, 20 + c);
        }
        wino_stamp(tr, 12 + c);
        if (more) __syncthreads();   // (none after the last chunk: see wino_core)
        wino_stamp(tr, 2 + c);
    }
}

}  // namespace azi
