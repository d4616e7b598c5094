// tower8.hip -- the MX-fp8 inference mode (AZ_DTYPE_FP8): the fused tower of tower.hip with the 2B
// residual convs on the block-scaled e4m3 matrix path, v_mfma_scale_f32_16x16x128_f8f6f4 (f32
// accumulate), the only form that reaches the fp8 peak on gfx950.  OCP MX: e4m3fn elements, one E8M0
// power-of-two scale per 32 consecutive channels -- per (square, 32 channels) for activations, per
// (output channel, tap, 32 input channels) for the BatchNorm-folded weights (quantised once on the host
// by az_mx8_quantize).  The residual stream x stays bf16 in LDS (add in f32); beside it sit the e4m3
// image + scale bytes of x, the next conv's operand, and of a block's inner activation h (e4m3 only).
// The 19->F input conv and the heads are the bf16 tower's code (tower_dev.h), run from the bf16 x.
// A wave owns 32 output channels of every square, so an activation scale block is one wave's epilogue
// output: amax over the 4 lanes (l16 + 16 h) that hold the block, two cross-lane maxima.
//
// Lane maps of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands (cbsz = blgp = 0), established on
// the MI355X with exact integer data by tools/mx8_lane_map.hip (profiles/mx8_lane_map.txt):
//   A: lane L holds 32 bytes (8 VGPRs) of row L % 16; B: lane L holds 32 bytes of column L % 16;
//      byte j of lane group t = L / 16 is K = 64 (j / 16) + 16 t + j % 16: each lane holds TWO 16-element
//      runs, 64 apart (not 32 consecutive K);
//   scales: byte op_sel (0..3) of the lane's scale VGPR, the other bytes are ignored; the scale of lane
//      L applies to row (A) or column (B) L % 16 and to K block g = L / 16, K in [32 g, 32 g + 32), which by
//      the K map is bytes [16 (g / 2), +16) of lane groups 2 (g % 2) and 2 (g % 2) + 1;
//   D: lane l register r = row 4 (l / 16) + r, column l % 16, as every 16x16 MFMA;
//   a NaN scale byte (0xFF) or element (0x7F) makes its row / column of D NaN;
//   v_cvt_pk_fp8_f32 rounds to nearest even with subnormals and does NOT saturate (465 -> 0x7F = NaN),
//      so the quantiser clamps at 448 first.
// A K-step is 128 channels of one tap; lane (l16, h) reads channels [16 h, +16) and [64 + 16 h, +16) of
// them (two ds_read_b128) and the scale byte of block h.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tower_dev.h"

namespace azi {

typedef __attribute__((ext_vector_type(8))) int i32x8;

struct Tower8Args {
    const uint4* w0;          // input conv, bf16 fragments (net.hip swizzle_bf16)
    const float* b0;
    unsigned w0bytes;
    const void* w8;           // residual convs: e4m3 A-fragments [conv][k-step][co/16][lane][32]
    const void* w8s;          // their E8M0 scale bytes [conv][k-step][co/16][lane]
    unsigned w8bytes, w8sbytes;
    const float* b8;          // folded biases [conv][F]
    const float* head;
    const uint4* head_frag;
    int blocks;
};

// workgroup shape and LDS map (bytes).  X: bf16 x, rows of F/8 + 2 slots as the bf16 tower.  X8 / H8:
// e4m3 rows of F codes + F/32 scale bytes, padded to F + 32 bytes.  Z8: the row off-board taps read
// (zero codes, scale bytes 127 = 2^0: 0xFF would be NaN).  ZB: the bf16 input conv's zero slots.  The
// input planes are staged in H8, the heads' scratch lies over X8 and H8.
template <int F> struct Tower8Cfg {
    static constexpr int BPB = TowerCfg<F>::BPB, NCO = 2, NCW = F / 32, NT = NCW * 64;
    static constexpr int RSF = F / 8 + 2, RSI = 32 / 8 + 2, RS8 = F + 32;
    static constexpr int XB = BPB * 64 * RSF * 16, A8 = BPB * 64 * RS8;
    static constexpr int X8 = XB, H8 = XB + A8, Z8 = XB + 2 * A8, ZB = Z8 + 512, TOTAL = ZB + 320;
    static constexpr int KS = 9 * F / 128, CF = F / 16;
    static_assert(XB % 256 == 0 && A8 % 256 == 0, "the bf16 input conv wants 256-byte aligned regions");
    static_assert(BPB * 64 * RSI * 16 <= A8, "input planes are staged in h8");
    static_assert(F + F / 32 <= 512, "zero row");
    static_assert(TOTAL <= 160 * 1024, "LDS");
};

// the E8M0 byte of a block whose largest magnitude has the f32 bits ub (sign cleared): exponent
// floor(log2 amax) - 8, clamped below at -127 (subnormal amax has exponent field 0); amax = 0 -> 2^0;
// a non-finite block -> 0xFF (NaN).  *inv = 1 / scale, exact.
__device__ __forceinline__ int mx8_scale_byte(unsigned ub, float* inv) {
    const int e = (int)(ub >> 23) - 8;
    const int sb = ub == 0u ? 127 : (e < 0 ? 0 : e);
    *inv = __builtin_bit_cast(float, (unsigned)(254 - sb) << 23);
    return ub >= 0x7F800000u ? 0xFF : sb;
}
// 4 values -> 4 e4m3fn codes: v / scale, saturated at 448 (NaN stays NaN), round to nearest even
__device__ __forceinline__ unsigned mx8_pack4(float a, float b, float c, float d, float inv) {
    a *= inv; b *= inv; c *= inv; d *= inv;
    a = a > 448.0f ? 448.0f : a; b = b > 448.0f ? 448.0f : b;
    c = c > 448.0f ? 448.0f : c; d = d > 448.0f ? 448.0f : d;
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    p = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
    return (unsigned)p;
}
__device__ __forceinline__ unsigned abs_bits(float v) { return __builtin_bit_cast(unsigned, v) & 0x7FFFFFFFu; }
__device__ __forceinline__ unsigned umax2(unsigned a, unsigned b) { return a > b ? a : b; }

// this wave's A fragments and scale bytes of k-step kg of the weight stream (all convs back to back;
// past the end the range check of the buffer loads gives zeros)
template <int F>
__device__ __forceinline__ void w8_load(i32x8 (&a)[2], int (&s)[2], const __amdgpu_buffer_rsrc_t rW,
                                        const __amdgpu_buffer_rsrc_t rS, int kg, int cw, int lane) {
    constexpr int CF = F / 16;
#pragma unroll
    for (int n = 0; n < 2; n++) {
        // the whole byte offset rides in voffset: only that is checked against num_records
        const int fr = kg * CF + cw * 2 + n;
        const uint4 lo = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rW, fr * 2048 + lane * 32, 0, 0));
        const uint4 hi = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rW, fr * 2048 + lane * 32 + 16, 0, 0));
        a[n] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        s[n] = (int)__builtin_amdgcn_raw_buffer_load_b8(rS, fr * 64 + lane, 0, 0);
    }
}

// One 3x3 residual conv layer LDS -> LDS on the scaled MFMA.  in_off / out_off: e4m3 images (rows of RS8
// bytes); wave cw computes channels [32 cw, 32 cw + 32) of all BPB boards.  k0: the layer's first k-step
// in the weight stream; wr / ws hold that k-step on entry and the next layer's first on exit.
// RESID: y = relu(conv + bias + x) with x bf16 at x_off, y rounded to bf16 back into x; otherwise
// y = relu(conv + bias).  Either way y (f32) is block-quantised into out_off.  raw (probe only): the
// accumulators of the first nb boards, [board][64][F].
template <int F, bool RESID>
__device__ __forceinline__ void conv8_lds(char* __restrict__ ldsb, int in_off, int out_off, int x_off,
                                          const __amdgpu_buffer_rsrc_t rW, const __amdgpu_buffer_rsrc_t rS, int k0,
                                          const float* __restrict__ bias, i32x8 (&wr)[2], int (&ws)[2], int cw,
                                          int lane, float* __restrict__ raw, int nb) {
    typedef Tower8Cfg<F> C;
    constexpr int MF = C::BPB * 4, NCO = 2, RS8 = C::RS8, NK = F / 128;
    // the lane index laundered per layer: the per-tap LDS addresses are invariant across the tower's
    // block loop, and hoisted out of it they stay live through every layer and spill
    lane = vgpr_index(lane);
    const int h = lane >> 4, l16 = lane & 15;
    f32x4 acc[MF][NCO];
#pragma unroll
    for (int n = 0; n < NCO; n++) {
        const float4 bn = *reinterpret_cast<const float4*>(bias + cw * 32 + n * 16 + h * 4);
#pragma unroll
        for (int m = 0; m < MF; m++) acc[m][n] = f32x4{bn.x, bn.y, bn.z, bn.w};
    }
    const int lr = l16 >> 3, lf = l16 & 7;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int dr = tap / 3 - 1, df = tap % 3 - 1;
        const bool okf = (unsigned)(lf + df) < 8u;
        // row of the shifted square; off-board taps read the zero row (scale 2^0)
        int base[MF];
#pragma unroll
        for (int m = 0; m < MF; m++) {
            const int q = m & 3, bb = m >> 2;
            const bool ok = okf && (unsigned)(2 * q + lr + dr) < 8u;
            base[m] = ok ? in_off + (bb * 64 + q * 16 + l16 + dr * 8 + df) * RS8 : C::Z8;
        }
#pragma unroll
        for (int ks = 0; ks < NK; ks++) {
            i32x8 a[NCO];
            int sa[NCO];
#pragma unroll
            for (int n = 0; n < NCO; n++) { a[n] = wr[n]; sa[n] = ws[n]; }
            w8_load<F>(wr, ws, rW, rS, k0 + tap * NK + ks + 1, cw, lane);
            __builtin_amdgcn_sched_barrier(0);          // keep each k-step's reads with its MFMAs (no spills)
#pragma unroll
            for (int m = 0; m < MF; m++) {
                const char* row = ldsb + base[m];
                const uint4 lo = *reinterpret_cast<const uint4*>(row + ks * 128 + 16 * h);
                const uint4 hi = *reinterpret_cast<const uint4*>(row + ks * 128 + 64 + 16 * h);
                const int sb = *reinterpret_cast<const unsigned char*>(row + F + ks * 4 + h);
                const i32x8 b = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
                for (int n = 0; n < NCO; n++)
                    acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[n], b, acc[m][n], 0, 0, 0, sa[n], 0, sb);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (raw) {
#pragma unroll
        for (int m = 0; m < MF; m++)
            if ((m >> 2) < nb)
#pragma unroll
                for (int n = 0; n < NCO; n++)
                    *reinterpret_cast<f32x4*>(raw + ((size_t)(m >> 2) * 64 + (m & 3) * 16 + l16) * F + cw * 32 + n * 16 + h * 4) = acc[m][n];
    }
    // epilogue.  Lane (l16, h) holds channels 32 cw + 16 n + 4 h + r of square l16 of each fragment: the
    // 32-channel block of that square is spread over the 4 lanes l16 + 16 h'.  `in` and `out` are
    // different buffers, x is read and written by the same lane: no barrier before, one after.
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
#pragma unroll
    for (int m = 0; m < MF; m++) {
        const int row = (m >> 2) * 64 + (m & 3) * 16 + l16;
        float v[8];
#pragma unroll
        for (int n = 0; n < NCO; n++) {
            f32x2 lo = {acc[m][n][0], acc[m][n][1]}, hi = {acc[m][n][2], acc[m][n][3]};
            if constexpr (RESID) {
                const int co = cw * 32 + n * 16 + h * 4;
                uint2* xp = reinterpret_cast<uint2*>(ldsb + x_off + (row * C::RSF + (co >> 3)) * 16 + (co & 7) * 2);
                const uint2 r = *xp;
                lo += f32x2{__builtin_bit_cast(float, r.x << 16), __builtin_bit_cast(float, r.x & 0xFFFF0000u)};
                hi += f32x2{__builtin_bit_cast(float, r.y << 16), __builtin_bit_cast(float, r.y & 0xFFFF0000u)};
                lo[0] = relu_nan<true>(lo[0]); lo[1] = relu_nan<true>(lo[1]);
                hi[0] = relu_nan<true>(hi[0]); hi[1] = relu_nan<true>(hi[1]);
                *xp = make_uint2(__builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf16x2)),
                                 __builtin_bit_cast(unsigned, __builtin_convertvector(hi, bf16x2)));
            } else {
                lo[0] = relu_nan<true>(lo[0]); lo[1] = relu_nan<true>(lo[1]);
                hi[0] = relu_nan<true>(hi[0]); hi[1] = relu_nan<true>(hi[1]);
            }
            v[n * 4 + 0] = lo[0]; v[n * 4 + 1] = lo[1]; v[n * 4 + 2] = hi[0]; v[n * 4 + 3] = hi[1];
        }
        unsigned ub = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) ub = umax2(ub, abs_bits(v[i]));
        ub = umax2(ub, (unsigned)__shfl_xor((int)ub, 16, 64));
        ub = umax2(ub, (unsigned)__shfl_xor((int)ub, 32, 64));
        float inv;
        const int sb = mx8_scale_byte(ub, &inv);
        char* orow = ldsb + out_off + row * RS8;
#pragma unroll
        for (int n = 0; n < NCO; n++)
            *reinterpret_cast<unsigned*>(orow + cw * 32 + n * 16 + h * 4) =
                mx8_pack4(v[n * 4], v[n * 4 + 1], v[n * 4 + 2], v[n * 4 + 3], inv);
        // all 4 lanes of the block store the same byte: a branch here splits the epilogue into basic blocks,
        // and the compiler then sinks each fragment's whole MFMA chain into its block (every weight
        // fragment of the layer live at once: ~2500 spills)
        *reinterpret_cast<unsigned char*>(orow + F + cw) = (unsigned char)sb;
    }
    __syncthreads();
}

// the zero rows of the workgroup (before the first barrier)
template <int F> __device__ __forceinline__ void tower8_zero_rows(char* ldsb, int tid) {
    typedef Tower8Cfg<F> C;
    for (int i = tid; i < 512 / 4; i += C::NT)
        *reinterpret_cast<unsigned*>(ldsb + C::Z8 + i * 4) = (i * 4 >= F && i * 4 < F + F / 32) ? 0x7F7F7F7Fu : 0u;
    for (int i = tid; i < 320 / 4; i += C::NT) *reinterpret_cast<unsigned*>(ldsb + C::ZB + i * 4) = 0u;
}

// boards [row0, row0 + nb) through the MX-fp8 tower, all waves of the workgroup
template <int F, bool SEARCH>
__device__ __forceinline__ void tower8_board(const __bf16* __restrict__ planes, const Tower8Args& ta, int row0, int nb,
                                             float* __restrict__ pol_out, float* __restrict__ val_out,
                                             const SearchOut& so, int tid) {
    typedef Tower8Cfg<F> C;
    constexpr int BPB = C::BPB, NT = C::NT, RSF = C::RSF, RSI = C::RSI, NCO = C::NCO;
    __shared__ __attribute__((aligned(16))) uint4 lds[C::TOTAL / 16];
    char* ldsb = reinterpret_cast<char*>(lds);
    const int lane = tid & 63;
    const int cw = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint4* H = reinterpret_cast<uint4*>(ldsb + C::H8);

    // the input planes [row][64][32] bf16 into h8 with row stride RSI, as tower_board (tower.hip)
    if (planes) {
        const uint4* src = reinterpret_cast<const uint4*>(planes) + (size_t)row0 * 64 * 4;
        for (int c = tid; c < BPB * 64 * 4; c += NT) {
            const int rowi = c >> 2, slot = c & 3;
            H[rowi * RSI + slot] = rowi < nb * 64 ? src[c] : make_uint4(0, 0, 0, 0);
        }
    } else {
        // search mode: to_tensor (chess.rs:191-245) from the leaf's packed position, one thread per square
        for (int rowi = tid; rowi < BPB * 64; rowi += NT) {
            uint4 q[4] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
            if (rowi < nb * 64) {
                const int row = vgpr_index(row0 + (rowi >> 6)), sq = rowi & 63;
                const azc::Pos p = so.npos[(size_t)so.row_game[row] * so.NMAX + so.row_node[row]];
                __bf16 v[32];
#pragma unroll
                for (int c = 0; c < 32; c++) v[c] = (__bf16)(c < 19 ? azc::plane_value(p, c, sq) : 0.0f);
                __builtin_memcpy(q, v, sizeof(v));
            }
#pragma unroll
            for (int k = 0; k < 4; k++) H[rowi * RSI + k] = q[k];
        }
    }
    tower8_zero_rows<F>(ldsb, tid);
    __syncthreads();
    {
        uint4 wr0[RingPF<1>::PF][NCO];
        ring_fill<1, F, NCO>(wr0, ta.w0, cw, lane);
        conv_lds<32, RSI, F, RSF, BPB, NCO, false>(ldsb, lds, C::H8, C::ZB, ta.w0, nullptr, ta.b0, wr0, cw, 0, lane,
                                                   ta.w0bytes, 0u);
    }
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)ta.w8, (short)0, (int)ta.w8bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc((void*)ta.w8s, (short)0, (int)ta.w8sbytes, 0x00020000);
    i32x8 wr[2];
    int ws[2];
    w8_load<F>(wr, ws, rW, rS, 0, cw, lane);
    // the e4m3 image of the input conv's bf16 x: one thread per (square, 32-channel block)
    for (int i = tid; i < BPB * 64 * (F / 32); i += NT) {
        const int row = i / (F / 32), blk = i % (F / 32);
        const uint4* src = reinterpret_cast<const uint4*>(ldsb + (row * RSF + blk * 4) * 16);
        float v[32];
        unsigned ub = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 u = src[k];
            const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                v[k * 8 + 2 * j] = __builtin_bit_cast(float, w[j] << 16);
                v[k * 8 + 2 * j + 1] = __builtin_bit_cast(float, w[j] & 0xFFFF0000u);
            }
        }
#pragma unroll
        for (int k = 0; k < 32; k++) ub = umax2(ub, abs_bits(v[k]));
        float inv;
        const int sb = mx8_scale_byte(ub, &inv);
        char* orow = ldsb + C::X8 + row * C::RS8;
#pragma unroll
        for (int k = 0; k < 8; k++)
            *reinterpret_cast<unsigned*>(orow + blk * 32 + k * 4) = mx8_pack4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3], inv);
        *reinterpret_cast<unsigned char*>(orow + F + blk) = (unsigned char)sb;
    }
    __syncthreads();
    for (int b = 0; b < ta.blocks; b++) {
        conv8_lds<F, false>(ldsb, C::X8, C::H8, 0, rW, rS, (2 * b) * C::KS, ta.b8 + (size_t)(2 * b) * F, wr, ws, cw, lane,
                            nullptr, nb);
        conv8_lds<F, true>(ldsb, C::H8, C::X8, 0, rW, rS, (2 * b + 1) * C::KS, ta.b8 + (size_t)(2 * b + 1) * F, wr, ws, cw,
                           lane, nullptr, nb);
    }
    // heads from the bf16 x: NB boards at a time, scratch over x8 / h8; ReLUs keep NaN
    {
        constexpr int NB = HeadsCfg<F>::NB;
        static_assert(HeadsScratch<NB, NT>::FLOATS * 4 <= 2 * C::A8, "heads scratch must fit over x8 + h8");
        static_assert((16 * NB) % (NT / 64) == 0, "policy tiles must divide over the waves");
        for (int b0 = 0; b0 < BPB && b0 < nb; b0 += NB)
            heads_group<F, RSF, NB, NT, SEARCH, false, true>(ldsb, reinterpret_cast<float*>(ldsb + C::X8), b0, nb, row0,
                                                             tid, ta.head_frag, ta.head, pol_out, val_out, so);
    }
}

template <int F, bool SEARCH>
__global__ void __launch_bounds__(Tower8Cfg<F>::NT)
tower8_kernel(const __bf16* __restrict__ planes, Tower8Args ta, const int* __restrict__ count_ptr, int rows,
              float* __restrict__ pol_out, float* __restrict__ val_out, SearchOut so) {
    constexpr int BPB = Tower8Cfg<F>::BPB;
    const int count = count_ptr ? min(load_fresh(count_ptr), rows) : rows;
    const int row0 = blockIdx.x * BPB;
    if (row0 >= count) return;
    tower8_board<F, SEARCH>(planes, ta, row0, min(BPB, count - row0), pol_out, val_out, so, threadIdx.x);
}

// az_mx8_conv_probe: one residual conv layer of n boards through conv8_lds, operands and results in HBM
struct Mx8Probe {
    const unsigned char* codes;    // [n][64][F]
    const unsigned char* scales;   // [n][64][F/32]
    const unsigned short* resid;   // [n][64][F] bf16 (RESID)
    const void* w8; const void* w8s; unsigned w8bytes, w8sbytes;
    const float* bias;
    float* acc; unsigned short* out_bf16; unsigned char* out_codes; unsigned char* out_scales;
    int n;
};
template <int F, bool RESID>
__global__ void __launch_bounds__(Tower8Cfg<F>::NT) mx8_conv_probe_kernel(Mx8Probe p) {
    typedef Tower8Cfg<F> C;
    constexpr int BPB = C::BPB, NT = C::NT, IN = RESID ? C::H8 : C::X8, OUT = RESID ? C::X8 : C::H8;
    __shared__ __attribute__((aligned(16))) uint4 lds[C::TOTAL / 16];
    char* ldsb = reinterpret_cast<char*>(lds);
    const int tid = threadIdx.x, lane = tid & 63, cw = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * BPB;
    if (row0 >= p.n) return;
    const int nb = min(BPB, p.n - row0);
    for (int c = tid; c < BPB * 64 * (F / 16); c += NT) {
        const int row = c / (F / 16), ch = c % (F / 16);
        *reinterpret_cast<uint4*>(ldsb + IN + row * C::RS8 + ch * 16) =
            row < nb * 64 ? reinterpret_cast<const uint4*>(p.codes)[((size_t)row0 * 64 + row) * (F / 16) + ch] : make_uint4(0, 0, 0, 0);
        if constexpr (RESID)
            for (int k = 0; k < 2; k++)
                *reinterpret_cast<uint4*>(ldsb + (row * C::RSF + ch * 2 + k) * 16) =
                    row < nb * 64 ? reinterpret_cast<const uint4*>(p.resid)[((size_t)row0 * 64 + row) * (F / 8) + ch * 2 + k] : make_uint4(0, 0, 0, 0);
    }
    for (int c = tid; c < BPB * 64 * (F / 32); c += NT) {
        const int row = c / (F / 32), blk = c % (F / 32);
        ldsb[IN + row * C::RS8 + F + blk] = row < nb * 64 ? (char)p.scales[((size_t)row0 * 64 + row) * (F / 32) + blk] : (char)127;
    }
    tower8_zero_rows<F>(ldsb, tid);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)p.w8, (short)0, (int)p.w8bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc((void*)p.w8s, (short)0, (int)p.w8sbytes, 0x00020000);
    i32x8 wr[2];
    int ws[2];
    w8_load<F>(wr, ws, rW, rS, 0, cw, lane);
    conv8_lds<F, RESID>(ldsb, IN, OUT, 0, rW, rS, 0, p.bias, wr, ws, cw, lane,
                        p.acc ? p.acc + (size_t)row0 * 64 * F : nullptr, nb);
    for (int c = tid; c < nb * 64 * (F / 16); c += NT) {
        const int row = c / (F / 16), ch = c % (F / 16);
        if (p.out_codes)
            reinterpret_cast<uint4*>(p.out_codes)[((size_t)row0 * 64 + row) * (F / 16) + ch] =
                *reinterpret_cast<const uint4*>(ldsb + OUT + row * C::RS8 + ch * 16);
        if constexpr (RESID)
            if (p.out_bf16)
                for (int k = 0; k < 2; k++)
                    reinterpret_cast<uint4*>(p.out_bf16)[((size_t)row0 * 64 + row) * (F / 8) + ch * 2 + k] =
                        *reinterpret_cast<const uint4*>(ldsb + (row * C::RSF + ch * 2 + k) * 16);
    }
    if (p.out_scales)
        for (int c = tid; c < nb * 64 * (F / 32); c += NT) {
            const int row = c / (F / 32), blk = c % (F / 32);
            p.out_scales[((size_t)row0 * 64 + row) * (F / 32) + blk] = (unsigned char)ldsb[OUT + row * C::RS8 + F + blk];
        }
}

// ---------------------------------------------------------------------------------- host side
// e4m3fn code of a >= 0 (a <= 448 after saturation), round to nearest even, subnormals kept
static unsigned char e4m3_code(double a) {
    if (!(a <= 448.0)) return std::isnan(a) ? 0x7F : 0x7E;
    if (a == 0.0) return 0;
    int e;
    (void)frexp(a, &e);                                  // a in [2^(e-1), 2^e)
    const int E = e - 1 < -6 ? -6 : e - 1;               // subnormals share the quantum of 2^-6
    const int n = (int)nearbyint(ldexp(a, 3 - E));       // units of 2^(E-3): 0..16, 16 carries into E + 1
    return (unsigned char)(((E + 7) << 3) + n - 8);
}

// A-fragments of one conv: codes [co][tap][ci], scales [co][9][F/32] -> wout [k-step][co/16][lane][32],
// sout [k-step][co/16][lane]; k-step = tap * (F/128) + ks, lane (l16, h): row co = 16 cf + l16, byte j =
// channel 128 ks + 64 (j / 16) + 16 h + j % 16, scale of block 4 ks + h
void mx8_fragments(const uint8_t* codes, const uint8_t* scales, int F, uint8_t* wout, uint8_t* sout) {
    const int NK = F / 128, CF = F / 16;
    for (int kidx = 0; kidx < 9 * NK; kidx++)
        for (int cf = 0; cf < CF; cf++)
            for (int lane = 0; lane < 64; lane++) {
                const int tap = kidx / NK, ks = kidx % NK, co = cf * 16 + (lane & 15), h = lane >> 4;
                const size_t fr = ((size_t)kidx * CF + cf) * 64 + lane;
                for (int j = 0; j < 32; j++)
                    wout[fr * 32 + j] = codes[((size_t)co * 9 + tap) * F + ks * 128 + 64 * (j >> 4) + 16 * h + (j & 15)];
                sout[fr] = scales[((size_t)co * 9 + tap) * (F / 32) + ks * 4 + h];
            }
}

size_t mx8_conv_code_bytes(int F) { return (size_t)9 * (F / 128) * (F / 16) * 64 * 32; }

// one folded residual conv wf [co][ci][9] of an fp8 net, quantised and appended to the weight stream
void mx8_append_conv(const std::vector<float>& wf, int F, std::vector<uint8_t>* w8, std::vector<uint8_t>* w8s) {
    std::vector<float> blk((size_t)F * 9 * F);           // [co][tap][ci]
    for (int co = 0; co < F; co++)
        for (int ci = 0; ci < F; ci++)
            for (int tap = 0; tap < 9; tap++) blk[((size_t)co * 9 + tap) * F + ci] = wf[((size_t)co * F + ci) * 9 + tap];
    std::vector<uint8_t> codes(blk.size()), scales(blk.size() / 32);
    az_mx8_quantize(blk.data(), blk.size() / 32, codes.data(), scales.data());
    const size_t cb = mx8_conv_code_bytes(F), o = w8->size(), os = w8s->size();
    w8->resize(o + cb);
    w8s->resize(os + cb / 32);
    mx8_fragments(codes.data(), scales.data(), F, w8->data() + o, w8s->data() + os);
}

int tower8_forward(NetDev* n, const void* planes, const int* count, int rows, float* pol, float* val,
                   const SearchOut* so, hipStream_t st) {
    if (n->conv_w.empty() || (n->blocks > 0 && (!n->w8 || !n->w8s || !n->b8))) return fail("MX-fp8 tower: weights not built");
    Tower8Args ta;
    memset(&ta, 0, sizeof(ta));
    ta.w0 = reinterpret_cast<const uint4*>(n->conv_w[0]);
    ta.b0 = n->conv_b[0];
    ta.w0bytes = (unsigned)n->conv_bytes[0];
    ta.w8 = n->w8; ta.w8s = n->w8s; ta.w8bytes = (unsigned)n->w8_bytes; ta.w8sbytes = (unsigned)n->w8s_bytes;
    ta.b8 = n->b8;
    ta.head = n->head;
    ta.head_frag = reinterpret_cast<const uint4*>(n->head_frag);
    ta.blocks = n->blocks;
    SearchOut dummy;
    memset(&dummy, 0, sizeof(dummy));
    const SearchOut& s = so ? *so : dummy;
#define AZ_TOWER8(FF)                                                                                            \
    if (n->filters == FF) {                                                                                      \
        const int grid = (rows + Tower8Cfg<FF>::BPB - 1) / Tower8Cfg<FF>::BPB;                                   \
        if (so) tower8_kernel<FF, true><<<grid, Tower8Cfg<FF>::NT, 0, st>>>((const __bf16*)planes, ta, count, rows, pol, val, s); \
        else tower8_kernel<FF, false><<<grid, Tower8Cfg<FF>::NT, 0, st>>>((const __bf16*)planes, ta, count, rows, pol, val, s);  \
        return hipGetLastError() == hipSuccess ? 0 : fail("MX-fp8 tower launch failed");                         \
    }
    AZ_TOWER8(256) AZ_TOWER8(128)
#undef AZ_TOWER8
    return fail("MX-fp8 tower: filters must be 128 or 256");
}

}  // namespace azi

using namespace azi;

extern "C" {

int az_mx8_quantize(const float* x, size_t nblocks, uint8_t* codes, uint8_t* scales) {
    if (!x || !codes || !scales) return fail("null argument");
    for (size_t b = 0; b < nblocks; b++) {
        const float* v = x + b * 32;
        float amax = 0.0f;
        bool finite = true;
        for (int i = 0; i < 32; i++) {
            finite = finite && std::isfinite(v[i]);
            if (fabsf(v[i]) > amax) amax = fabsf(v[i]);
        }
        if (!finite) {                                   // not a block the format holds: NaN scale and elements
            scales[b] = 0xFF;
            memset(codes + b * 32, 0x7F, 32);
            continue;
        }
        int se = 0;
        if (amax > 0.0f) {
            int e;
            (void)frexp((double)amax, &e);               // floor(log2 amax) = e - 1
            se = e - 9 < -127 ? -127 : (e - 9 > 127 ? 127 : e - 9);
        }
        scales[b] = (uint8_t)(se + 127);
        for (int i = 0; i < 32; i++)
            codes[b * 32 + i] = (uint8_t)(e4m3_code(ldexp(fabs((double)v[i]), -se)) | (std::signbit(v[i]) ? 0x80 : 0));
    }
    return 0;
}

int az_mx8_conv_probe(int device, int filters, int n, const uint8_t* act_codes, const uint8_t* act_scales,
                      const uint8_t* w_codes, const uint8_t* w_scales, const uint16_t* residual, const float* bias,
                      float* acc, uint16_t* out_bf16, uint8_t* out_codes, uint8_t* out_scales) {
    const int F = filters;
    if (F != 128 && F != 256) return fail("az_mx8_conv_probe: filters must be 128 or 256");
    if (n <= 0 || !act_codes || !act_scales || !w_codes || !w_scales || !bias) return fail("az_mx8_conv_probe: null argument");
    if (out_bf16 && !residual) return fail("az_mx8_conv_probe: the bf16 output belongs to the residual form (conv2)");
    AZ_HIP(hipSetDevice(device));
    // weights [co][ci][3][3] -> blocks [co][tap][ci] -> fragments
    std::vector<uint8_t> wc((size_t)F * 9 * F), w8(mx8_conv_code_bytes(F)), w8s(w8.size() / 32);
    for (int co = 0; co < F; co++)
        for (int ci = 0; ci < F; ci++)
            for (int tap = 0; tap < 9; tap++) wc[((size_t)co * 9 + tap) * F + ci] = w_codes[((size_t)co * F + ci) * 9 + tap];
    mx8_fragments(wc.data(), w_scales, F, w8.data(), w8s.data());
    const size_t na = (size_t)n * 64 * F;
    struct Buf { void* p = nullptr; ~Buf() { (void)hipFree(p); } };
    Buf d_c, d_s, d_r, d_w, d_ws, d_b, d_acc, d_ob, d_oc, d_os;
    auto up = [](Buf& b, const void* src, size_t bytes) {
        if (hipMalloc(&b.p, bytes) != hipSuccess) return -1;
        return src && hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) != hipSuccess ? -1 : 0;
    };
    if (up(d_c, act_codes, na) || up(d_s, act_scales, na / 32) || up(d_w, w8.data(), w8.size()) ||
        up(d_ws, w8s.data(), w8s.size()) || up(d_b, bias, (size_t)F * 4) || (residual && up(d_r, residual, na * 2)) ||
        up(d_acc, nullptr, na * 4) || up(d_ob, nullptr, na * 2) || up(d_oc, nullptr, na) || up(d_os, nullptr, na / 32))
        return fail("az_mx8_conv_probe: device allocation failed");
    Mx8Probe p;
    p.codes = (const unsigned char*)d_c.p; p.scales = (const unsigned char*)d_s.p; p.resid = (const unsigned short*)d_r.p;
    p.w8 = d_w.p; p.w8s = d_ws.p; p.w8bytes = (unsigned)w8.size(); p.w8sbytes = (unsigned)w8s.size();
    p.bias = (const float*)d_b.p;
    p.acc = (float*)d_acc.p; p.out_bf16 = (unsigned short*)d_ob.p; p.out_codes = (unsigned char*)d_oc.p;
    p.out_scales = (unsigned char*)d_os.p;
    p.n = n;
#define AZ_PROBE8(FF)                                                                                   \
    if (F == FF) {                                                                                      \
        const int grid = (n + Tower8Cfg<FF>::BPB - 1) / Tower8Cfg<FF>::BPB;                             \
        if (residual) mx8_conv_probe_kernel<FF, true><<<grid, Tower8Cfg<FF>::NT>>>(p);                  \
        else mx8_conv_probe_kernel<FF, false><<<grid, Tower8Cfg<FF>::NT>>>(p);                          \
    }
    AZ_PROBE8(256) AZ_PROBE8(128)
#undef AZ_PROBE8
    AZ_HIP(hipGetLastError());
    AZ_HIP(hipDeviceSynchronize());
    if (acc) AZ_HIP(hipMemcpy(acc, d_acc.p, na * 4, hipMemcpyDeviceToHost));
    if (out_bf16) AZ_HIP(hipMemcpy(out_bf16, d_ob.p, na * 2, hipMemcpyDeviceToHost));
    if (out_codes) AZ_HIP(hipMemcpy(out_codes, d_oc.p, na, hipMemcpyDeviceToHost));
    if (out_scales) AZ_HIP(hipMemcpy(out_scales, d_os.p, na / 32, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
