// tower.hip -- fused residual tower + heads (agent.rs:112-144) in ONE launch per batch.
//
// Each workgroup owns BPB boards for the whole forward pass: their activations x and h
// (NHWC bf16, padded 16-B-slot rows: conflict-free ds_read_b128 for every 3x3 tap) stay
// resident in LDS across the input conv, all 2B residual convs and the heads; only the
// weights stream from L2 (MFMA-fragment-swizzled, one dwordx4 per lane per fragment,
// prefetched two K-steps ahead).  Between layers there is a workgroup barrier, no HBM
// round trip and no kernel boundary.  Per layer per wave: 32 output channels x
// (BPB/WB) boards on v_mfma_f32_16x16x32_bf16 (fp32 accumulate), bias + (residual) +
// ReLU fused into an epilogue that writes bf16 back into LDS.
// The heads run from the same LDS image (f32 VALU), in dense mode (policy[4096],
// value) or in search mode (softmax gathered at the new node's legal edges).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "az_internal.h"
#include "search_dev.h"
#include "wino.h"

#include "tower_dev.h"

namespace azi {

// boards [row0, row0 + nb) through the bf16 tower, all waves of the workgroup
template <int F, bool SEARCH>
__device__ __forceinline__ void tower_board(const __bf16* __restrict__ planes, const TowerArgs& ta, int row0, int nb,
                                            float* __restrict__ pol_out, float* __restrict__ val_out,
                                            const SearchOut& so, int tid) {
    constexpr int BPB = TowerCfg<F>::BPB, WB = TowerCfg<F>::WB, BPW = BPB / WB, NCO = TowerCfg<F>::NCO;
    constexpr int NCW = F / (16 * NCO);
    constexpr int NT = NCW * WB * 64;
    constexpr int RSF = F / 8 + 2, RSI = 32 / 8 + 2;
    constexpr int XSZ = BPB * 64 * RSF;               // slots per activation buffer
    constexpr int ZN = 16 + F / 8;
    // h doubles as the heads' scratch: at least that large (small nets with 1 board per workgroup)
    constexpr int HSZ0 = (HeadsScratch<HeadsCfg<F>::NB, NT>::FLOATS * 4 + 15) / 16;
    constexpr int HSZ = ((XSZ > HSZ0 ? XSZ : HSZ0) + 15) / 16 * 16;
    __shared__ __attribute__((aligned(16))) uint4 lds[XSZ + HSZ + ZN];
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = w % NCW, bw = w / NCW;
    uint4* X = lds;
    uint4* H = lds + XSZ;
    const int zero_off = (XSZ + HSZ) * 16;
    const char* ldsb = reinterpret_cast<const char*>(lds);

    // stage the input planes [row][64][32] into H with row stride RSI
    if (planes) {
        const uint4* src = reinterpret_cast<const uint4*>(planes) + (size_t)row0 * 64 * 4;
        for (int c = tid; c < BPB * 64 * 4; c += NT) {
            const int rowi = c >> 2, slot = c & 3;
            H[rowi * RSI + slot] = rowi < nb * 64 ? src[c] : make_uint4(0, 0, 0, 0);
        }
    } else {
        // search mode without a planes buffer: to_tensor (chess.rs:191-245) straight from the
        // leaf's packed position into LDS, one thread per square -- the same per-element
        // conversion as encode_rows_kernel (net.hip), so the rows are bit-identical
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
    for (int c = tid; c < ZN; c += NT) lds[XSZ + HSZ + c] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    {
        uint4 wr0[RingPF<1>::PF][NCO];
        ring_fill<1, F, NCO>(wr0, ta.w[0], cw, lane);
        conv_lds<32, RSI, F, RSF, BPW, NCO, false>(ldsb, X, XSZ * 16, zero_off, ta.w[0], nullptr, ta.b[0], wr0, cw,
                                                   bw, lane, ta.wbytes[0], 0u);
    }
    uint4 wr[RingPF<F / 32>::PF][NCO];
    if (ta.blocks > 0) ring_fill<F / 32, F, NCO>(wr, ta.w[1], cw, lane);
    for (int b = 0; b < ta.blocks; b++) {
        const uint4* after = b + 1 < ta.blocks ? ta.w[3 + 2 * b] : nullptr;
        const unsigned after_bytes = b + 1 < ta.blocks ? ta.wbytes[3 + 2 * b] : 0u;
        conv_lds<F, RSF, F, RSF, BPW, NCO, false>(ldsb, H, 0, zero_off, ta.w[1 + 2 * b], ta.w[2 + 2 * b],
                                                  ta.b[1 + 2 * b], wr, cw, bw, lane, ta.wbytes[1 + 2 * b],
                                                  ta.wbytes[2 + 2 * b]);
        conv_lds<F, RSF, F, RSF, BPW, NCO, true>(ldsb, X, XSZ * 16, zero_off, ta.w[2 + 2 * b], after,
                                                 ta.b[2 + 2 * b], wr, cw, bw, lane, ta.wbytes[2 + 2 * b], after_bytes);
    }
    // heads: NB boards at a time, scratch in H
    {
        constexpr int NB = HeadsCfg<F>::NB;
        static_assert(HeadsScratch<NB, NT>::FLOATS * 4 <= HSZ * 16, "heads scratch must fit in h");
        static_assert((16 * NB) % (NT / 64) == 0, "policy tiles must divide over the waves");
        for (int b0 = 0; b0 < BPB && b0 < nb; b0 += NB)
            heads_group<F, RSF, NB, NT, SEARCH>(ldsb, reinterpret_cast<float*>(H), b0, nb, row0, tid, ta.head_frag,
                                                ta.head, pol_out, val_out, so);
    }
}

template <int F, bool SEARCH>
__global__ void __launch_bounds__((F / (16 * TowerCfg<F>::NCO)) * TowerCfg<F>::WB * 64)
tower_kernel(const __bf16* __restrict__ planes, TowerArgs ta, const int* __restrict__ count_ptr, int rows,
             float* __restrict__ pol_out, float* __restrict__ val_out, SearchOut so) {
    constexpr int BPB = TowerCfg<F>::BPB;
    const int count = count_ptr ? min(load_fresh(count_ptr), rows) : rows;
    const int row0 = blockIdx.x * BPB;
    if (row0 >= count) return;
    tower_board<F, SEARCH>(planes, ta, row0, min(BPB, count - row0), pol_out, val_out, so, threadIdx.x);
}

// ====================================================================== f32 tower
// The reference evaluates in f32 (burn Cuda<f32>, main.rs:15,68; agent.rs:112-144).  This is the
// same fused structure at that precision: activations f32 in LDS, weights f32, every product
// an exact f32 FMA on v_mfma_f32_16x16x4_f32 (64 FLOP/clk/SIMD, the f32 peak, 157.3 TF).
// At 1/16 of the bf16 rate a k-step is long (NCO*MF*4 MFMAs x 32 cycles per wave), so operand
// delivery has ample slack: one board per workgroup (x and h f32 = 2 x 66 KB of LDS at F = 256),
// B fragments double-buffered one k-step ahead, weight fragments two k-steps ahead.
template <int F> struct Tower32Cfg;
template <> struct Tower32Cfg<256> { static constexpr int BPB = 1, WB = 1, NCO = 2; };   // 8 waves, 2 per SIMD
template <> struct Tower32Cfg<128> { static constexpr int BPB = 1, WB = 1, NCO = 2; };
template <> struct Tower32Cfg<64> { static constexpr int BPB = 1, WB = 1, NCO = 1; };
template <> struct Tower32Cfg<32> { static constexpr int BPB = 2, WB = 2, NCO = 1; };
constexpr int T32_PF = 2;  // weight k-steps in flight (register ring)

// One f32 3x3 conv layer LDS -> LDS.  IN: CIN channels (16-channel k-chunks = 4 float4 slots),
// row stride RSI slots; OUT: F channels, row stride RSO.  Wave (cw, bw) computes channels
// [16*NCO*cw, +16*NCO) of boards [bw*BPW, +BPW).  A = weights (16 co x 4 ci), B = activations
// (4 ci x 16 squares): one ds_read_b128 per lane holds 4 consecutive channels and feeds the 4
// MFMAs of a k-chunk (k = 4h + s).  wr: weight ring, holds this layer's first T32_PF k-steps on
// entry, the next layer's (rN) on exit.  The k-step byte offset rides in voffset, so the
// descriptor's num_records bounds every refill.
template <int CIN, int RSI, int F, int RSO, int BPW, int NCO, bool RESID>
__device__ __forceinline__ void conv32_lds(const char* __restrict__ ldsb, char* __restrict__ outb, int in_off,
                                           int zero_off, const __amdgpu_buffer_rsrc_t rW,
                                           const __amdgpu_buffer_rsrc_t rN, const float* __restrict__ bias,
                                           f32x4 (&wr)[T32_PF][NCO], int cw, int bw, int lane) {
    constexpr int NCH = CIN / 16;
    constexpr int CF = F / 16;
    constexpr int MF = BPW * 4;
    constexpr int PF = T32_PF;
    constexpr int KB = CF * 64 * 16;                  // bytes per k-step (all output fragments)
    static_assert(NCH % PF == 0, "ring slots must be compile-time");
    const int h = lane >> 4, l16 = lane & 15;
    f32x4 acc[MF][NCO];
#pragma unroll
    for (int n = 0; n < NCO; n++) {
        const float4 bn = *reinterpret_cast<const float4*>(bias + cw * 16 * NCO + n * 16 + h * 4);
#pragma unroll
        for (int m = 0; m < MF; m++) acc[m][n] = f32x4{bn.x, bn.y, bn.z, bn.w};
    }
    const int voff = ((cw * NCO) * 64 + lane) * 16;
    // per-tap B addresses, branch-free: off-board taps read the zero row at the same slot mod 16
    const int lane_off = ((l16 * RSI) + h) * 16;
    const int lr = l16 >> 3, lf = l16 & 7;
    auto tap_bases = [&](int tap, int* base) {
        const int dr = tap / 3 - 1, df = tap % 3 - 1;
        const bool okf = (unsigned)(lf + df) < 8u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const bool ok = okf && (unsigned)(2 * q + lr + dr) < 8u;
#pragma unroll
            for (int bb = 0; bb < BPW; bb++) {
                const int m = bb * 4 + q;
                const int va = lane_off + (((bw * BPW + bb) * 64 + q * 16 + dr * 8 + df) * RSI) * 16 + in_off;
                base[m] = ok ? va : ((va & 0xF0) | zero_off);
            }
        }
    };
    int bcur[MF], bnx[MF];
    f32x4 bq[MF], bn[MF];
    tap_bases(0, bcur);
#pragma unroll
    for (int m = 0; m < MF; m++) bq[m] = *reinterpret_cast<const f32x4*>(ldsb + bcur[m]);
#pragma unroll 1
    for (int tap = 0; tap < 9; tap++) {
        tap_bases(tap < 8 ? tap + 1 : 8, bnx);
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            // next k-step's B fragments (same tap, next chunk; or the next tap's first chunk) and the
            // weight refill are issued first: a whole k-step of MFMAs covers their latency
#pragma unroll
            for (int m = 0; m < MF; m++)
                bn[m] = *reinterpret_cast<const f32x4*>(ldsb + (c + 1 < NCH ? bcur[m] + (c + 1) * 64 : bnx[m]));
            f32x4 a[NCO];
#pragma unroll
            for (int n = 0; n < NCO; n++) a[n] = wr[c % PF][n];
            // refill the slot with the k-step PF later: this tap, the next tap, or the next layer
            {
                int kidx;
                bool nxt = false;
                if (c + PF < NCH) kidx = tap * NCH + c + PF;
                else if (tap < 8) kidx = (tap + 1) * NCH + c + PF - NCH;
                else { kidx = c + PF - NCH; nxt = true; }
#pragma unroll
                for (int n = 0; n < NCO; n++)
                    wr[c % PF][n] = __builtin_bit_cast(
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(nxt ? rN : rW, voff + n * 1024 + kidx * KB, 0, 0));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s4 = 0; s4 < 4; s4++)
#pragma unroll
                for (int m = 0; m < MF; m++)
#pragma unroll
                    for (int n = 0; n < NCO; n++)
                        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[n][s4], bq[m][s4], acc[m][n], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < MF; m++) bq[m] = bn[m];
        }
#pragma unroll
        for (int m = 0; m < MF; m++) bcur[m] = bnx[m];
    }
    // epilogue: (+ residual) + ReLU, 4 consecutive channels of one square per lane (16-B stores);
    // `in` and `out` are different buffers, the barrier after publishes `out`
#pragma unroll
    for (int n = 0; n < NCO; n++) {
        const int co = cw * 16 * NCO + n * 16 + h * 4;
        char* lane_base = outb + ((bw * BPW * 64 + l16) * RSO + (co >> 2)) * 16;
#pragma unroll
        for (int m = 0; m < MF; m++) {
            f32x4* dst = reinterpret_cast<f32x4*>(lane_base + ((m >> 2) * 64 + (m & 3) * 16) * RSO * 16);
            f32x4 v = acc[m][n];
            if constexpr (RESID) v += *dst;
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = fmaxf(v[r], 0.0f);
            *dst = v;
        }
    }
    __syncthreads();
}

// The f32 input conv of the Winograd tower (19 planes -> F, one board): the weights packed by
// net.hip swizzle_f32_input_packed -- k-steps 0-8: tap k, channels 0-15 (one ds_read_b128 of
// B per square fragment feeds 4 MFMAs, as conv32_lds); k-steps 9-11: MFMA slice s = tap 4 kl + s,
// lane group h = channel 16 + h (one ds_read_b32 per slice and square fragment).  12 k-steps of
// MFMAs instead of conv32_lds's 18 over 32 zero-padded channels.  Input planes at in_off (row
// stride RSI slots, channels 0-31), output F channels at outb (row stride RSO), + bias, ReLU.
// wr holds k-steps [0, T32_PF) on entry; rW covers the 12 k-steps and the 8 zero ones after.
template <int F, int RSI, int RSO, int NCO>
__device__ __forceinline__ void conv32_in_packed(const char* __restrict__ ldsb, char* __restrict__ outb, int in_off,
                                                 int zero_off, const __amdgpu_buffer_rsrc_t rW,
                                                 const float* __restrict__ bias, f32x4 (&wr)[T32_PF][NCO], int cw,
                                                 int lane) {
    constexpr int CF = F / 16, MF = 4, PF = T32_PF, KB = CF * 64 * 16, NK = 12;
    static_assert(NK % PF == 0, "ring slots must be compile-time");
    const int h = lane >> 4, l16 = lane & 15;
    f32x4 acc[MF][NCO];
#pragma unroll
    for (int n = 0; n < NCO; n++) {
        const float4 bn = *reinterpret_cast<const float4*>(bias + cw * 16 * NCO + n * 16 + h * 4);
#pragma unroll
        for (int m = 0; m < MF; m++) acc[m][n] = f32x4{bn.x, bn.y, bn.z, bn.w};
    }
    const int voff = ((cw * NCO) * 64 + lane) * 16;
    const int lr = l16 >> 3, lf = l16 & 7;
    // square fragment m, tap: the lane's square (2 m + lr, lf) shifted by the tap; off-board taps
    // read the zero row (channels 0-15: at the same slot mod 16, conflict-free as conv32_lds)
    auto tap_ok = [&](int tap, int m) {
        const int dr = tap / 3 - 1, df = tap % 3 - 1;
        return (unsigned)(lf + df) < 8u && (unsigned)(2 * m + lr + dr) < 8u;
    };
    auto row_addr = [&](int tap, int m) {   // byte offset of the shifted square's row
        const int dr = tap / 3 - 1, df = tap % 3 - 1;
        return ((l16 + m * 16 + dr * 8 + df) * RSI) * 16 + in_off;
    };
    auto main_addr = [&](int tap, int m) {
        const int va = row_addr(tap, m) + h * 16;
        return tap_ok(tap, m) ? va : ((va & 0xF0) | zero_off);
    };
    auto side_addr = [&](int tap, int m) {  // channel 16 + h
        return tap_ok(tap, m) ? row_addr(tap, m) + 64 + h * 4 : zero_off + 64 + h * 4;
    };
    f32x4 bq[MF];
#pragma unroll
    for (int m = 0; m < MF; m++) bq[m] = *reinterpret_cast<const f32x4*>(ldsb + main_addr(0, m));
#pragma unroll
    for (int k = 0; k < NK; k++) {
        // next k-step's B fragments first: a whole k-step of MFMAs covers their latency
        f32x4 bn[MF];
        if (k + 1 < 9) {
#pragma unroll
            for (int m = 0; m < MF; m++) bn[m] = *reinterpret_cast<const f32x4*>(ldsb + main_addr(k + 1, m));
        } else if (k + 1 < NK) {
            const int kl = k + 1 - 9;
#pragma unroll
            for (int m = 0; m < MF; m++)
#pragma unroll
                for (int s4 = 0; s4 < 4; s4++) {
                    const int tap = 4 * kl + s4;
                    bn[m][s4] = tap < 9 ? *reinterpret_cast<const float*>(ldsb + side_addr(tap, m)) : 0.0f;
                }
        }
        f32x4 a[NCO];
#pragma unroll
        for (int n = 0; n < NCO; n++) a[n] = wr[k % PF][n];
#pragma unroll
        for (int n = 0; n < NCO; n++)
            wr[k % PF][n] = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(rW, voff + n * 1024 + (k + PF) * KB, 0, 0));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s4 = 0; s4 < 4; s4++)
#pragma unroll
            for (int m = 0; m < MF; m++)
#pragma unroll
                for (int n = 0; n < NCO; n++)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[n][s4], bq[m][s4], acc[m][n], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (k + 1 < NK) {
#pragma unroll
            for (int m = 0; m < MF; m++) bq[m] = bn[m];
        }
    }
    // epilogue: + ReLU, 4 consecutive channels of one square per lane; the barrier after publishes it
#pragma unroll
    for (int n = 0; n < NCO; n++) {
        const int co = cw * 16 * NCO + n * 16 + h * 4;
        char* lane_base = outb + (l16 * RSO + (co >> 2)) * 16;
#pragma unroll
        for (int m = 0; m < MF; m++) {
            f32x4 v = acc[m][n];
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = fmaxf(v[r], 0.0f);
            *reinterpret_cast<f32x4*>(lane_base + (m * 16) * RSO * 16) = v;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t t32_rsrc(const uint4* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, (int)bytes, 0x00020000);
}

// input planes [row][64][32] f32 -> H (row stride RSI slots): from a planes buffer, or in search
// mode to_tensor (chess.rs:191-245) from the leaf's packed position, one thread per square
template <int BPB, int RSI, int NT>
__device__ __forceinline__ void stage_planes_f32(uint4* H, const float* __restrict__ planes, const SearchOut& so,
                                                 int row0, int nb, int tid) {
    if (planes) {
        const uint4* src = reinterpret_cast<const uint4*>(planes) + (size_t)row0 * 64 * 8;
        for (int c = tid; c < BPB * 64 * 8; c += NT) {
            const int rowi = c >> 3, slot = c & 7;
            H[rowi * RSI + slot] = rowi < nb * 64 ? src[c] : make_uint4(0, 0, 0, 0);
        }
    } else {
        for (int rowi = tid; rowi < BPB * 64; rowi += NT) {
            float v[32];
#pragma unroll
            for (int c = 0; c < 32; c++) v[c] = 0.0f;
            if (rowi < nb * 64) {
                const int row = vgpr_index(row0 + (rowi >> 6)), sq = rowi & 63;
                const azc::Pos p = so.npos[(size_t)so.row_game[row] * so.NMAX + so.row_node[row]];
#pragma unroll
                for (int c = 0; c < 19; c++) v[c] = azc::plane_value(p, c, sq);
            }
            uint4 q[8];
            __builtin_memcpy(q, v, sizeof(v));
#pragma unroll
            for (int k = 0; k < 8; k++) H[rowi * RSI + k] = q[k];
        }
    }
}

template <int F, bool SEARCH>
__global__ void __launch_bounds__((F / (16 * Tower32Cfg<F>::NCO)) * Tower32Cfg<F>::WB * 64)
tower32_kernel(const float* __restrict__ planes, TowerArgs ta, const int* __restrict__ count_ptr, int rows,
               float* __restrict__ pol_out, float* __restrict__ val_out, SearchOut so) {
    constexpr int BPB = Tower32Cfg<F>::BPB, WB = Tower32Cfg<F>::WB, BPW = BPB / WB, NCO = Tower32Cfg<F>::NCO;
    constexpr int NCW = F / (16 * NCO);
    constexpr int NT = NCW * WB * 64;
    constexpr int RSF = F / 4 + 2, RSI = 32 / 4 + 2;  // f32 rows: F/4 slots + 2 pad (conflict-free b128 reads)
    constexpr int XSZ = BPB * 64 * RSF;
    constexpr int ZN = 16 + F / 4;
    constexpr int NBH = HeadsCfg<F>::NB < BPB ? HeadsCfg<F>::NB : BPB;
    constexpr int HSZ0 = (HeadsScratch<NBH, NT, heads_npart(NT, true)>::FLOATS * 4 + 15) / 16;
    constexpr int HSZ = ((XSZ > HSZ0 ? XSZ : HSZ0) + 15) / 16 * 16;
    static_assert(BPB * 64 * RSI <= HSZ, "input planes must fit in h");
    __shared__ __attribute__((aligned(16))) uint4 lds[XSZ + HSZ + ZN];
    const int count = count_ptr ? min(load_fresh(count_ptr), rows) : rows;
    const int row0 = blockIdx.x * BPB;
    if (row0 >= count) return;
    const int nb = min(BPB, count - row0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = w % NCW, bw = w / NCW;
    uint4* X = lds;
    uint4* H = lds + XSZ;
    const int zero_off = (XSZ + HSZ) * 16;
    const char* ldsb = reinterpret_cast<const char*>(lds);

    stage_planes_f32<BPB, RSI, NT>(H, planes, so, row0, nb, tid);
    for (int c = tid; c < ZN; c += NT) lds[XSZ + HSZ + c] = make_uint4(0, 0, 0, 0);
    __syncthreads();

    f32x4 wr[T32_PF][NCO];
    {
        const __amdgpu_buffer_rsrc_t r0 = t32_rsrc(ta.w[0], ta.wbytes[0]);
        const __amdgpu_buffer_rsrc_t r1 =
            ta.blocks > 0 ? t32_rsrc(ta.w[1], ta.wbytes[1]) : t32_rsrc(ta.w[0] + 18 * (F / 16) * 64, ta.wbytes[0] - 18 * (F / 16) * 1024);
        const int voff = ((cw * NCO) * 64 + lane) * 16;
#pragma unroll
        for (int i = 0; i < T32_PF; i++)
#pragma unroll
            for (int n = 0; n < NCO; n++)
                wr[i][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                         r0, voff + n * 1024 + i * (F / 16) * 1024, 0, 0));
        conv32_lds<32, RSI, F, RSF, BPW, NCO, false>(ldsb, reinterpret_cast<char*>(X), XSZ * 16, zero_off, r0, r1,
                                                     ta.b[0], wr, cw, bw, lane);
    }
    for (int b = 0; b < ta.blocks; b++) {
        const int i1 = 1 + 2 * b, i2 = 2 + 2 * b;
        const __amdgpu_buffer_rsrc_t r1 = t32_rsrc(ta.w[i1], ta.wbytes[i1]);
        const __amdgpu_buffer_rsrc_t r2 = t32_rsrc(ta.w[i2], ta.wbytes[i2]);
        // after the block's second conv the ring prefetches the next block's first conv (or
        // reads this conv's zero pad after the last one)
        const __amdgpu_buffer_rsrc_t r3 =
            b + 1 < ta.blocks ? t32_rsrc(ta.w[i2 + 1], ta.wbytes[i2 + 1])
                              : t32_rsrc(ta.w[i2] + (size_t)9 * (F / 16) * (F / 16) * 64,
                                         ta.wbytes[i2] - 9u * (F / 16) * (F / 16) * 1024);
        conv32_lds<F, RSF, F, RSF, BPW, NCO, false>(ldsb, reinterpret_cast<char*>(H), 0, zero_off, r1, r2,
                                                    ta.b[i1], wr, cw, bw, lane);
        conv32_lds<F, RSF, F, RSF, BPW, NCO, true>(ldsb, reinterpret_cast<char*>(X), XSZ * 16, zero_off, r2, r3,
                                                   ta.b[i2], wr, cw, bw, lane);
    }
    static_assert(HeadsScratch<NBH, NT, heads_npart(NT, true)>::FLOATS * 4 <= HSZ * 16, "heads scratch must fit in h");
    static_assert((16 * NBH) % (NT / 64) == 0, "policy tiles must divide over the waves");
    for (int b0 = 0; b0 < BPB && b0 < nb; b0 += NBH)
        heads_group<F, RSF, NBH, NT, SEARCH, true>(ldsb, reinterpret_cast<float*>(H), b0, nb, row0, tid,
                                                   ta.head_frag32, ta.head, pol_out, val_out, so);
}


// ====================================================================== f32 Winograd tower
// The Winograd conv core is wino.h (shared with the training step).  conv_wino: one residual conv
// of the tower, LDS -> LDS: the core, then + residual (the block input x, kept in the registers of
// the wave that owns those outputs), ReLU, written back over the layer input in ACT.
#ifdef AZ_TOWER_TRACE
// trace build: per-wave phase stamps of the first AZ_TT_WG workgroups of the last launch
// (slot layout in tools/tower_trace.py); read back with az_tower_trace_read
constexpr int AZ_TT_WG = 8, AZ_TT_SLOTS = 2048;
__device__ unsigned long long az_tower_trace_buf[AZ_TT_WG * 8 * AZ_TT_SLOTS];
__device__ __forceinline__ unsigned long long* tt_slot(int w) {
    return blockIdx.x < AZ_TT_WG && w < 8 ? az_tower_trace_buf + (blockIdx.x * 8 + w) * AZ_TT_SLOTS : nullptr;
}
#else
__device__ __forceinline__ unsigned long long* tt_slot(int) { return nullptr; }
#endif

template <int F, bool RESID, bool H16, int SP = 16, bool ROWS = false, bool VROWS = false>
__device__ __forceinline__ void conv_wino(char* __restrict__ ldsb, int vbase,
                                          const __amdgpu_buffer_rsrc_t rW, const __amdgpu_buffer_rsrc_t rN,
                                          const float* __restrict__ bias, float unscale,
                                          f32x4 (&wr)[WinoRing<F, H16, ROWS>::PF][WinoRing<F, H16>::RX][WinoCfg<F>::NN],
                                          f32x4 (&xres)[WinoCfg<F>::NN][4], int w, int lane, bool pre_in,
                                          bool pre_out, int vsel, int* flag, int seq,
                                          unsigned long long* tr = nullptr) {
    constexpr int NN = WinoCfg<F>::NN, RS = F / 4 + 2, VBYTES = WinoCfg<F>::CH * 1024;
    const int l16 = lane & 15, h = lane >> 4;
    const int ty = l16 >> 2, tx = l16 & 3;
    const int co0 = w * 16 * NN + h * 4;
    auto out_addr = [&](int n, int a, int b) { return ((2 * ty + a) * 8 + 2 * tx + b) * RS * 16 + (co0 + n * 16) * 4; };
    // the residual: this wave's outputs of the block input, read before it is overwritten (keeping
    // them in registers from the previous conv's epilogue instead measured +0.4 % at C3)
    if constexpr (!RESID) {
#pragma unroll
        for (int n = 0; n < NN; n++)
#pragma unroll
            for (int q = 0; q < 4; q++) xres[n][q] = *reinterpret_cast<const f32x4*>(ldsb + out_addr(n, q >> 1, q & 1));
    }
    f32x4 y[NN][4];
    wino_stamp(tr, 0);
    // F = 64: the single chunk's V alternates between two buffers from conv to conv (vsel)
    const int vconv = vbase + (F == 64 ? vsel * VBYTES : 0);
    if constexpr (H16) wino_core_h16<F, SP, ROWS, VROWS>(ldsb, vconv, rW, rN, bias, unscale, wr, w, lane, y, pre_in, tr);
    else wino_core<F>(ldsb, vconv, rW, rN, bias, wr, w, lane, y, pre_in, tr);
    wino_stamp(tr, 10);
    f32x4 o[NN][4];
#pragma unroll
    for (int n = 0; n < NN; n++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f32x4 v = y[n][q];
            if constexpr (RESID) v += xres[n][q];
            // split-f16: an activation beyond the f16 range arrives as NaN and stays NaN (fmaxf drops it)
#pragma unroll
            for (int r = 0; r < 4; r++) v[r] = relu_nan<H16>(v[r]);
            *reinterpret_cast<f32x4*>(ldsb + out_addr(n, q >> 1, q & 1)) = v;
            o[n][q] = v;
        }
    wino_stamp(tr, 11);
    // F = 256: the next conv's chunk 0 is this conv's output channels 0-31, all written by wave 0;
    // the first wave of each SIMD pair finishes ahead of its partner, so waves 0-3
    // transform it into V[0] (free since the previous chunk barrier) while waves 4-7 finish, and the
    // next conv starts on its MFMAs after this barrier.  Wave 0's stores are published to waves 1-3
    // through an LDS flag (release / acquire at workgroup scope)
    if constexpr (F == 256) {
        if (pre_out && w < WinoCfg<F>::NWV / 2) {
            if (w == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            else
                while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != seq)
                    __builtin_amdgcn_s_sleep(1);
            // (shared rows: the same items as the tail transform, 4 per wave)
            if constexpr (VROWS) WinoXf<F>(ldsb, vbase, w, lane).template vrows<WinoCfg<F>::NWV / 2>(0, 0);
            else WinoXf<F>(ldsb, vbase, w, lane).template both<H16, ROWS ? WINO_XF_COLS : H16 && SP == 12 ? WINO_XF_NEG1 : WINO_XF_FULL>(0, 0);
        }
    } else if constexpr (F == 64) {
        // F = 64: each wave's 16 output channels are a quarter of the next conv's single chunk;
        // the wave transforms them from its registers (DPP neighbour exchange) into the other V
        // buffer -- no ACT round trip, no barrier between the epilogue and the transform
        if (pre_out) wino_xform_regs<F, H16>(o[0], ldsb + vbase + (1 - vsel) * VBYTES, w, lane);
        (void)flag; (void)seq;
    } else {
        (void)pre_out; (void)flag; (void)seq;
    }
    (void)o;
    __syncthreads();
}

// one board (batch row row0) through the Winograd f32 tower, all NWV waves of the workgroup; SP: the
// split-f16 weights' streamed points per 32-channel group (wino_core_h16)
template <int F, bool SEARCH, bool H16, int SP = 16, bool ROWS = false, bool VROWS = false>
__device__ __forceinline__ void tower32w_board(const float* __restrict__ planes, const TowerArgs& ta, int row0,
                                                      float* __restrict__ pol_out, float* __restrict__ val_out,
                                                      const SearchOut& so, int tid) {
    constexpr int NWV = WinoCfg<F>::NWV, NT = NWV * 64, NN = WinoCfg<F>::NN;
    constexpr int XS = WinoRing<F, H16>::XS, RX = WinoRing<F, H16>::RX;
    constexpr int RSF = F / 4 + 2, RSI = 32 / 4 + 2;
    constexpr int XSZ = 64 * RSF;                        // ACT, uint4 slots
    // both V buffers (one when a single chunk covers the input), also planes staging / heads scratch
    // (F = 64: two single-chunk buffers, alternating from conv to conv)
    // (shared rows: two buffers of WINO_VR_BYTES, 40 KB instead of 64)
    constexpr int VSZ = VROWS ? 2 * WINO_VR_BYTES / 16 : (F / WinoCfg<F>::CH > 1 || F == 64 ? 2 : 1) * WinoCfg<F>::CH * 1024 / 16;
    constexpr int PF = WinoRing<F, H16, ROWS>::PF;
    constexpr int ZN = 16 + F / 4;
    constexpr int PAD = WINO_PAD_SQ * RSF;               // zero squares either side of ACT
    static_assert(HeadsScratch<1, NT, heads_npart(NT, true)>::FLOATS * 4 <= VSZ * 16, "heads scratch must fit in V");
    static_assert(64 * RSI <= VSZ, "input planes must fit in V");
    __shared__ __attribute__((aligned(16))) uint4 lds[PAD + XSZ + PAD + VSZ + ZN + 1];
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint4* X = lds + PAD;
    uint4* V = X + XSZ + PAD;
    const int vbase = (XSZ + PAD) * 16;                  // offsets from ACT
    const int zero_off = (XSZ + PAD + VSZ) * 16;
    static_assert((XSZ + PAD + VSZ) * 16 % 256 == 0, "conv32_lds ORs the zero row's offset into the low byte");
    char* ldsb = reinterpret_cast<char*>(X);
    unsigned long long* tr = nullptr;
#ifdef AZ_TOWER_TRACE
    tr = tt_slot(w);
#endif
    wino_stamp(tr, 0);
    stage_planes_f32<1, RSI, NT>(V, planes, so, row0, 1, tid);
    for (int c = tid; c < ZN + 1; c += NT) V[VSZ + c] = make_uint4(0, 0, 0, 0);   // zero row + the pre-transform flag
    int* flag = reinterpret_cast<int*>(V + VSZ + ZN);
    for (int c = tid; c < PAD; c += NT) {
        lds[c] = make_uint4(0, 0, 0, 0);
        X[XSZ + c] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    wino_stamp(tr, 1);
    {   // input conv 19 -> F: direct, channels 16-18 of four taps packed per k-step (12 k-steps)
        f32x4 wr[T32_PF][NN];
        const __amdgpu_buffer_rsrc_t r0 = t32_rsrc(ta.w0pk, ta.w0pk_bytes);
        const int voff = ((w * NN) * 64 + lane) * 16;
#pragma unroll
        for (int i = 0; i < T32_PF; i++)
#pragma unroll
            for (int n = 0; n < NN; n++)
                wr[i][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                         r0, voff + n * 1024 + i * (F / 16) * 1024, 0, 0));
        conv32_in_packed<F, RSI, RSF, NN>(ldsb, reinterpret_cast<char*>(X), vbase, zero_off, r0, ta.b[0], wr, w, lane);
    }
    if constexpr (VROWS) {
        // the planes staged in V are consumed (the input conv ends in a barrier): zero the off-board rows 0
        // and 9 of both buffers' planes, 32 runs of 256 B, one uint4 per thread; no item writes them, and
        // the chunk-0 transform's barrier publishes them before the first B read
        static_assert(NT == 32 * 16, "one uint4 of the zero rows per thread");
        *reinterpret_cast<uint4*>(ldsb + vbase + wino_vr_zero(tid >> 4) + (tid & 15) * 16) = make_uint4(0, 0, 0, 0);
    }
    wino_stamp(tr, 2);
    f32x4 xres[NN][4];
    f32x4 wring[PF][RX][NN];
    if (ta.blocks > 0) {
        const __amdgpu_buffer_rsrc_t r = t32_rsrc(ta.ww[0], ta.wwbytes[0]);
        const int voff = H16 ? wino16_voff<F>(w, lane) : wino_voff<F>(w, lane);
#pragma unroll
        for (int i = 0; i < PF; i++)
#pragma unroll
            for (int rx = 0; rx < RX; rx++)
#pragma unroll
                for (int n = 0; n < NN; n++) {
                    // split-f16: rx = point rx / 2 of step i, its hi / lo plane (wino_core_h16; the steps
                    // are linear in the weights at either SP)
                    const int off = H16 ? (2 * n + rx % 2) * 1024 + (i * XS + rx / 2) * (F / 16) * 2048
                                        : n * 1024 + wino_toff<F>(0, i * XS + rx);
                    wring[i][rx][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff + off, 0, 0));
                }
    }
    for (int b = 0; b < ta.blocks; b++) {
        const unsigned wb3 = b + 1 < ta.blocks ? ta.wwbytes[2 * b + 2] : 0u;   // after the last conv: nothing (reads 0)
        const __amdgpu_buffer_rsrc_t r1 = t32_rsrc(ta.ww[2 * b], ta.wwbytes[2 * b]);
        const __amdgpu_buffer_rsrc_t r2 = t32_rsrc(ta.ww[2 * b + 1], ta.wwbytes[2 * b + 1]);
        const __amdgpu_buffer_rsrc_t r3 = t32_rsrc(b + 1 < ta.blocks ? ta.ww[2 * b + 2] : ta.ww[2 * b + 1], wb3);
        // F = 256 / 64: each conv transforms the next conv's chunk 0 at its end (conv_wino; C3 A/B
        // -0.3 % against the tail transform alone)
        constexpr bool PRE = F == 256 || F == 64;
        conv_wino<F, false, H16, SP, ROWS, VROWS>(ldsb, vbase, r1, r2, ta.b[1 + 2 * b], ta.wus[2 * b], wring, xres, w, lane, PRE && b > 0, PRE, 0, flag,
                            2 * b + 1, tr ? tr + 3 + 64 * b : nullptr);
        conv_wino<F, true, H16, SP, ROWS, VROWS>(ldsb, vbase, r2, r3, ta.b[2 + 2 * b], ta.wus[2 * b + 1], wring, xres, w, lane, PRE, PRE && b + 1 < ta.blocks,
                           F == 64 ? 1 : 0, flag, 2 * b + 2, tr ? tr + 35 + 64 * b : nullptr);
    }
    heads_group<F, RSF, 1, NT, SEARCH, true, H16>(ldsb, reinterpret_cast<float*>(V), 0, 1, row0, tid, ta.head_frag32, ta.head,
                                             pol_out, val_out, so, tr);
    wino_stamp(tr, 3 + 64 * 20);
}

template <int F, bool SEARCH, bool H16, int SP = 16, bool ROWS = false, bool VROWS = false>
__global__ void __launch_bounds__(WinoCfg<F>::NWV * 64)
tower32w_kernel(const float* __restrict__ planes, TowerArgs ta, const int* __restrict__ count_ptr, int rows,
                float* __restrict__ pol_out, float* __restrict__ val_out, SearchOut so) {
    const int count = count_ptr ? min(load_fresh(count_ptr), rows) : rows;
    if ((int)blockIdx.x >= count) return;
    tower32w_board<F, SEARCH, H16, SP, ROWS, VROWS>(planes, ta, blockIdx.x, pol_out, val_out, so, threadIdx.x);
}

// ---- two boards per workgroup (AZ_WINO_BOARDS = 2, wino.h wino_core_b2): the 256-filter row-direct
// shared-row tower with the residual convs' activations in global memory and both boards' MFMAs fed from
// one weight stream.
typedef unsigned int u32v4 __attribute__((__vector_size__(16)));
// LDS of the two-board kernel, uint4 slots: V, then AUX (the larger of planes staging and heads scratch, in
// 256-byte units), the input conv's zero row and the flag
constexpr int WINO_B2_HS = (HeadsScratch<1, 512, heads_npart(512, true)>::FLOATS * 4 + 15) / 16;
constexpr int WINO_B2_AUX = ((WINO_B2_HS > 64 * 10 ? WINO_B2_HS : 64 * 10) + 15) / 16 * 16;
constexpr int WINO_B2_ZN = 16 + 256 / 4;
constexpr int WINO_B2_LDS = (WINO_B2_VBYTES / 16 + WINO_B2_AUX + WINO_B2_ZN + 1) * 16;
// where one board's ACT overlays V while the input conv and the heads run (bytes from the start of LDS)
constexpr int WINO_B2_OVL = 0;
static_assert(WINO_B2_OVL % 256 == 0 && WINO_B2_OVL + WINO_B2_ACT <= WINO_B2_VBYTES, "the ACT overlay lies inside V");
// every vector memory operation of this wave has completed: before a workgroup hand-off (flag or barrier)
// of global ACT stores, on top of the workgroup-scope fences that order them
__device__ __forceinline__ void b2_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// one residual conv of both boards, global ACT -> global ACT: conv 1 of a block (RESID false) reads X and
// writes H; conv 2 reads H, adds the residual from X -- read by the wave that owns those outputs, after the
// accumulators are dead and before the same wave overwrites the same elements -- and writes X.
template <bool RESID>
__device__ __forceinline__ void conv_wino_b2(char* __restrict__ ldsv, const __amdgpu_buffer_rsrc_t rW,
                                             const __amdgpu_buffer_rsrc_t rN, const __amdgpu_buffer_rsrc_t rA,
                                             const float* __restrict__ bias, float unscale,
                                             f32x4 (&wr)[WINO_B2_PF][2][2], int w, int lane, bool pre_in, bool pre_out,
                                             int* flag, int seq, unsigned long long* tr = nullptr) {
    constexpr int HIN = RESID ? 1 : 0, HOUT = 1 - HIN;
    f32x4 acc[2][8][2];
    wino_stamp(tr, 0);
    wino_core_b2(ldsv, rW, rN, rA, HIN, wr, w, lane, pre_in, acc, tr);
    wino_stamp(tr, 10);
    const int ln = vgpr_index(lane);   // laundered: the epilogue's addresses are not kept through the chunk loop
    const int co0 = w * 32 + (ln >> 4) * 4;
    auto out_addr = [&](int n, int a, int b) { return wino_b2_out(w, ln, n, 2 * a + b); };
    // one (board, output fragment) k = 2 nb + n at a time, its residual requested two fragments ahead (at most
    // 32 VGPRs of residual and 16 of outputs beside the accumulators still to be transformed)
    f32x4 xres[2][4];
    auto xload = [&](int k) {
        if constexpr (RESID) {
#pragma unroll
            for (int q = 0; q < 4; q++)
                xres[k & 1][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                               rA, wino_b2_act(k >> 1, 0) + out_addr(k & 1, q >> 1, q & 1), 0, 0));
        }
    };
    xload(0);
    xload(1);
    (void)xres;
#pragma unroll
    for (int nb = 0; nb < 2; nb++)
#pragma unroll
        for (int n = 0; n < 2; n++) {
            f32x4 y[4];
            wino_rows_out(acc[nb], bias, unscale, co0, n, y);
            f32x4 o[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                o[q] = y[q];
                if constexpr (RESID) o[q] += xres[n][q];
            }
            if (2 * nb + n + 2 < 4) xload(2 * nb + n + 2);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                f32x4 v = o[q];
#pragma unroll
                for (int r = 0; r < 4; r++) v[r] = relu_nan<true>(v[r]);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32v4, v), rA,
                                                       wino_b2_act(nb, HOUT) + out_addr(n, q >> 1, q & 1), 0, 0);
            }
        }
    wino_stamp(tr, 11);
    b2_stores_done();
    // the next conv's chunk 0 is this conv's output channels 0-31 of either board, all written by wave 0:
    // as in conv_wino, waves 0-3 transform it into the V buffers 0 while waves 4-7 finish; wave 0's global
    // stores are published to waves 1-3 through the LDS flag
    if (pre_out && w < 4) {
        if (w == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != seq)
                __builtin_amdgcn_s_sleep(1);
        wino_b2_items<4>(ldsv, rA, HOUT, 0, 0, w, lane);
    }
    __syncthreads();
}

// batch rows row0 and (nbv = 2) row0 + 1 through the tower.  LDS: the four V buffers (80 KB), overlaid by
// one board's ACT [64 squares][66 slots] while the input conv and the heads run, one board after the
// other; AUX (planes staging, heads scratch); the zero row of the input conv and the hand-off flag.
// act: this workgroup's WINO_B2_WG bytes of global ACT.  An absent second board runs on zero planes and
// writes nothing out.
template <bool SEARCH>
__device__ __forceinline__ void tower32w_boards2(const float* __restrict__ planes, const TowerArgs& ta, int row0, int nbv,
                                                 char* __restrict__ act, float* __restrict__ pol_out,
                                                 float* __restrict__ val_out, const SearchOut& so, int tid) {
    constexpr int F = 256, NT = 512, NN = 2, RSF = F / 4 + 2, RSI = 32 / 4 + 2, PF = WINO_B2_PF;
    constexpr int VSZ = WINO_B2_VBYTES / 16, AUX = WINO_B2_AUX, ZN = WINO_B2_ZN;   // uint4 slots
    static_assert(64 * RSF <= VSZ && 64 * RSF * 16 == WINO_B2_ACT, "one board's ACT overlays V");
    static_assert(64 * RSI <= AUX, "input planes must fit in AUX");
    static_assert((VSZ + AUX) * 16 % 256 == 0, "conv32_in_packed ORs the zero row's offset into the low byte");
    static_assert(WINO_B2_LDS <= 163840, "LDS of a CU");
    __shared__ __attribute__((aligned(16))) uint4 lds[VSZ + AUX + ZN + 1];
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* ldsb = reinterpret_cast<char*>(lds);
    char* actl = ldsb + WINO_B2_OVL;                     // the overlaid ACT
    uint4* A = lds + VSZ;
    const int zero_off = (VSZ + AUX) * 16;
    int* flag = reinterpret_cast<int*>(lds + VSZ + AUX + ZN);
    const __amdgpu_buffer_rsrc_t rA = t32_rsrc(reinterpret_cast<const uint4*>(act), WINO_B2_WG);
    unsigned long long* tr = nullptr;
#ifdef AZ_TOWER_TRACE
    tr = tt_slot(w);
#endif
    wino_stamp(tr, 0);
    for (int c = tid; c < ZN + 1; c += NT) lds[VSZ + AUX + c] = make_uint4(0, 0, 0, 0);   // zero row + the flag
#pragma unroll 1
    for (int nb = 0; nb < 2; nb++) {
        stage_planes_f32<1, RSI, NT>(A, planes, so, row0 + nb, nb < nbv ? 1 : 0, tid);
        __syncthreads();
        if (nb == 0) wino_stamp(tr, 1);
        {   // input conv 19 -> F into the overlaid ACT, as tower32w_board
            f32x4 wr[T32_PF][NN];
            const __amdgpu_buffer_rsrc_t r0 = t32_rsrc(ta.w0pk, ta.w0pk_bytes);
            const int voff = ((w * NN) * 64 + lane) * 16;
#pragma unroll
            for (int i = 0; i < T32_PF; i++)
#pragma unroll
                for (int n = 0; n < NN; n++)
                    wr[i][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                             r0, voff + n * 1024 + i * (F / 16) * 1024, 0, 0));
            conv32_in_packed<F, RSI, RSF, NN>(ldsb, actl, VSZ * 16, zero_off, r0, ta.b[0], wr, w, lane);
        }
        // ACT -> the board's X: the 64 channel slots of every square
        for (int i = tid; i < 64 * 64; i += NT) {
            const int o = ((i >> 6) * RSF + (i & 63)) * 16;
            __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32v4*>(actl + o), rA, wino_b2_act(nb, 0) + o, 0, 0);
        }
        b2_stores_done();
        __syncthreads();
    }
    // rows 0 and 9 of the four V buffers' planes: 64 runs of 256 B, never written by an item
    static_assert(NT == 32 * 16, "two uint4 of the zero rows per thread");
#pragma unroll
    for (int k = 0; k < 2; k++)
        *reinterpret_cast<uint4*>(ldsb + wino_vr_zero((tid >> 4) + 32 * k) + (tid & 15) * 16) = make_uint4(0, 0, 0, 0);
    wino_stamp(tr, 2);
    f32x4 wring[PF][2][NN];
    if (ta.blocks > 0) {
        const __amdgpu_buffer_rsrc_t r = t32_rsrc(ta.ww[0], ta.wwbytes[0]);
        const int voff = wino16_voff<F>(w, lane);
#pragma unroll
        for (int i = 0; i < PF; i++)
#pragma unroll
            for (int pl = 0; pl < 2; pl++)
#pragma unroll
                for (int n = 0; n < NN; n++)
                    wring[i][pl][n] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                                    r, voff + (2 * n + pl) * 1024 + i * (F / 16) * 2048, 0, 0));
    }
    for (int b = 0; b < ta.blocks; b++) {
        const unsigned wb3 = b + 1 < ta.blocks ? ta.wwbytes[2 * b + 2] : 0u;   // after the last conv: nothing (reads 0)
        const __amdgpu_buffer_rsrc_t r1 = t32_rsrc(ta.ww[2 * b], ta.wwbytes[2 * b]);
        const __amdgpu_buffer_rsrc_t r2 = t32_rsrc(ta.ww[2 * b + 1], ta.wwbytes[2 * b + 1]);
        const __amdgpu_buffer_rsrc_t r3 = t32_rsrc(b + 1 < ta.blocks ? ta.ww[2 * b + 2] : ta.ww[2 * b + 1], wb3);
        conv_wino_b2<false>(ldsb, r1, r2, rA, ta.b[1 + 2 * b], ta.wus[2 * b], wring, w, lane, b > 0, true, flag, 2 * b + 1,
                            tr ? tr + 3 + 64 * b : nullptr);
        conv_wino_b2<true>(ldsb, r2, r3, rA, ta.b[2 + 2 * b], ta.wus[2 * b + 1], wring, w, lane, true, b + 1 < ta.blocks, flag,
                           2 * b + 2, tr ? tr + 35 + 64 * b : nullptr);
    }
    // heads: the board's X back into the overlaid ACT, one board after the other.  The thread index is made
    // again from the wave's and the lane's (kept from the kernel's entry through the convs it was spilled)
    tid = w * 64 + (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#pragma unroll 1
    for (int nb = 0; nb < nbv; nb++) {
        for (int i = tid; i < 64 * 64; i += NT) {
            const int o = ((i >> 6) * RSF + (i & 63)) * 16;
            *reinterpret_cast<u32v4*>(actl + o) = __builtin_amdgcn_raw_buffer_load_b128(rA, wino_b2_act(nb, 0) + o, 0, 0);
        }
        __syncthreads();
        heads_group<F, RSF, 1, NT, SEARCH, true, true>(actl, reinterpret_cast<float*>(A), 0, 1, row0 + nb, tid, ta.head_frag32,
                                                       ta.head, pol_out, val_out, so, tr);
    }
    wino_stamp(tr, 3 + 64 * 20);
}

template <bool SEARCH>
__global__ void __launch_bounds__(512)
tower32w2_kernel(const float* __restrict__ planes, TowerArgs ta, const int* __restrict__ count_ptr, int rows,
                 char* __restrict__ act, float* __restrict__ pol_out, float* __restrict__ val_out, SearchOut so) {
    const int count = count_ptr ? min(load_fresh(count_ptr), rows) : rows;
    const int row0 = 2 * (int)blockIdx.x;
    if (row0 >= count) return;
    tower32w_boards2<SEARCH>(planes, ta, row0, min(2, count - row0), act + (size_t)blockIdx.x * WINO_B2_WG, pol_out, val_out,
                             so, threadIdx.x);
}

// k_sims32w: simulation steps [step0, step1) of one game per workgroup, with no grid-wide step
// boundary.  A game's simulations only touch its own tree (tree.rs:180-207 runs them one after
// the other per game), so the workgroup of game g loops: wave 0 backs up the previous
// simulation, selects and expands (search_dev.h, the same functions as k_step); if the leaf
// needs the network, all waves evaluate it through the Winograd tower as batch row g, whose
// heads write the priors into the new node's edges and the value into value[g].  The last
// simulation is backed up before the kernel ends.  It replaces 2 launches per simulation step
// (k_step + the tower, each step waiting for the slowest game of both) when every game has a
// CU of its own (G <= CUs: C2), and is bit-identical to them (tests/test_gpu_search.py).
// Cross-wave hand-offs: the workgroup barriers carry workgroup-scope fences; every record written
// inside the kernel is read back through vector loads (vgpr_index), never the scalar cache.
// threads of the persistent kernel's workgroup: the Winograd f32 tower's, or the bf16 tower's
template <int F, bool BF16> struct SimsCfg { static constexpr int NT = WinoCfg<F>::NWV * 64; };
template <int F> struct SimsCfg<F, true> {
    static_assert(TowerCfg<F>::BPB == 1, "persistent bf16 kernel: one board per workgroup");
    static constexpr int NT = (F / (16 * TowerCfg<F>::NCO)) * TowerCfg<F>::WB * 64;
};
template <int F, bool BF16, bool H16 = false, int SP = 16, bool ROWS = false, bool VROWS = false>
__global__ void __launch_bounds__((SimsCfg<F, BF16>::NT))
k_sims32w(Engine E, TowerArgs ta, SearchOut so, int step0, int step1) {
    __shared__ int s_kind;
    if (!E.active[vgpr_index(blockIdx.x)]) return;     // constant within a move
    for (int step = step0; step <= step1; step++) {
        // indices laundered per simulation so that neither phase's loop-invariant address
        // arithmetic is hoisted across the other (it would stay live through it and spill)
        const int tid = vgpr_index(threadIdx.x), g = vgpr_index(blockIdx.x);
        const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
        unsigned long long* tr = tt_slot(w);            // trace builds only (nullptr otherwise)
        wino_stamp(tr, 1910);
        if (w == 0) {
            if (step > step0) {                        // the previous simulation's backup
                backup_game(E, g, lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
            wino_stamp(tr, 1911);
            int kind = X_NONE, nid = -1;
            if (step < step1) {
                select_game(E, g, lane);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                wino_stamp(tr, 1912);
                kind = expand_leaf_wave<1>(E, g, lane, &nid, step);   // wave 0 only
                wino_stamp(tr, 1913);
                if (lane == 0) {
                    if (kind == X_ROW) {
                        E.row_game[g] = g;
                        E.row_node[g] = nid;
                        E.leaf_row[g] = g;
                        // per-game slot, summed at readout: two same-address atomics from every
                        // workgroup per simulation were waited on at the barrier below (batch_hist
                        // is read only for the timed steps, which never run in this kernel)
                        E.g_evals[g] += 1ull;   // g is in a VGPR: a vector load, never the scalar cache
                    } else if (kind == X_TERMINAL) {
                        atomicAdd(&E.ctr->terminal, 1ull);
                    } else if (kind == X_CACHED) {
                        atomicAdd(&E.ctr->cache_hits, 1ull);
                    }
                }
            }
            if (lane == 0) s_kind = kind;
        }
        __syncthreads();
        const int kind = s_kind;
        wino_stamp(tr, 1914);
        if (kind == X_ROW) {
            if constexpr (BF16) tower_board<F, true>(nullptr, ta, g, 1, nullptr, nullptr, so, tid);
            else tower32w_board<F, true, H16, SP, ROWS, VROWS>(nullptr, ta, g, nullptr, nullptr, so, tid);
        }
        __syncthreads();
        wino_stamp(tr, 1915);
    }
}

bool tower_supported(const NetDev* n) {
    if (n->dtype == AZ_DTYPE_FP8) return n->blocks <= 40 && (n->filters == 256 || n->filters == 128);
    return (n->dtype == AZ_DTYPE_BF16 || n->dtype == AZ_DTYPE_F32) && n->blocks <= 40 &&
           (n->filters == 256 || n->filters == 128 || n->filters == 64 || n->filters == 32);
}

// the residual convs' split-f16 weights were built (net_create then builds no f32 Winograd copy)
static bool wino16_built(const NetDev* n) {
    return wino16_selected(n->split16, n->filters) && (int)n->wino16_w.size() == 2 * n->blocks;
}

bool wino_supported(const NetDev* n) {
    return n->dtype == AZ_DTYPE_F32 && n->winograd && n->filters >= 64 && n->in_pk32 != nullptr &&
           ((int)n->wino_w.size() == 2 * n->blocks || wino16_built(n));
}

bool wino_split16(const NetDev* n) { return wino_supported(n) && wino16_built(n); }

static TowerArgs tower_args(const NetDev* n) {
    TowerArgs ta;
    memset(&ta, 0, sizeof(ta));
    for (int i = 0; i < 1 + 2 * n->blocks; i++) {
        ta.w[i] = reinterpret_cast<const uint4*>(n->conv_w[i]);
        ta.b[i] = n->conv_b[i];
        ta.wbytes[i] = (unsigned)n->conv_bytes[i];
    }
    ta.head = n->head;
    ta.head_frag = reinterpret_cast<const uint4*>(n->head_frag);
    ta.head_frag32 = reinterpret_cast<const uint4*>(n->head_frag32);
    const bool h16 = wino_split16(n);
    for (size_t i = 0; i < (h16 ? n->wino16_w.size() : n->wino_w.size()); i++) {
        ta.ww[i] = reinterpret_cast<const uint4*>(h16 ? n->wino16_w[i] : n->wino_w[i]);
        ta.wwbytes[i] = (unsigned)(h16 ? n->wino16_bytes[i] : n->wino_bytes[i]);
        ta.wus[i] = h16 ? n->wino16_us[i] : 1.0f;
    }
    ta.w0pk = reinterpret_cast<const uint4*>(n->in_pk32);
    ta.w0pk_bytes = (unsigned)n->in_pk32_bytes;
    ta.blocks = n->blocks;
    return ta;
}

bool sims_persistent_supported(const NetDev* n) {
    return tower_supported(n) && (wino_supported(n) || (n->dtype == AZ_DTYPE_BF16 && n->filters == 64));
}

// simulation steps [step0, step1) of every game through k_sims32w (one workgroup per game);
// ends with every simulation backed up
int sims_persistent(const NetDev* n, const Engine& E, const SearchOut& so, int step0, int step1, hipStream_t st) {
    if (step1 <= step0) return 0;
    if (!sims_persistent_supported(n)) return fail("persistent simulation kernel: needs the f32 Winograd tower or the bf16 64-filter tower");
    const TowerArgs ta = tower_args(n);
    if (n->dtype == AZ_DTYPE_BF16) {
        k_sims32w<64, true><<<E.G, SimsCfg<64, true>::NT, 0, st>>>(E, ta, so, step0, step1);
        return hipGetLastError() == hipSuccess ? 0 : fail("persistent simulation kernel launch failed");
    }
#define AZ_SIMS32W(FF, H16, SP, ROWS, VR)                                                                   \
    if (n->filters == FF) {                                                                            \
        k_sims32w<FF, false, H16, SP, ROWS, VR><<<E.G, SimsCfg<FF, false>::NT, 0, st>>>(E, ta, so, step0, step1); \
        return hipGetLastError() == hipSuccess ? 0 : fail("persistent simulation kernel launch failed"); \
    }
    if (wino_split16(n)) {
        if (n->wino_streamed == 12 && n->wino_rows && n->wino_vrows) { AZ_SIMS32W(256, true, 12, true, true) }
        if (n->wino_streamed == 12 && n->wino_rows) { AZ_SIMS32W(256, true, 12, true, false) }
        if (n->wino_streamed == 12) { AZ_SIMS32W(256, true, 12, false, false) }
        AZ_SIMS32W(256, true, 16, false, false) AZ_SIMS32W(128, true, 16, false, false) AZ_SIMS32W(64, true, 16, false, false)
    }
    AZ_SIMS32W(256, false, 16, false, false) AZ_SIMS32W(128, false, 16, false, false) AZ_SIMS32W(64, false, 16, false, false)
#undef AZ_SIMS32W
    return fail("persistent simulation kernel: unsupported filters");
}

// the global ACT of stream st's two-board launches, at least `wgs` workgroups of WINO_B2_WG bytes.  Growing
// waits for the stream's earlier launches (they use the old allocation) before freeing it.  The lock covers the
// map and the allocation, not the launch that follows: a stream is used by one host thread at a time, as
// everywhere in this library.  An entry stays until net_destroy, also after its stream is gone
static char* b2_act_for(NetDev* n, hipStream_t st, int wgs) {
    std::lock_guard<std::mutex> lock(n->b2_mu);
    NetDev::B2Act& a = n->b2_act[st];
    if (wgs > a.wgs) {
        if (a.p) {
            if (hipStreamSynchronize(st) != hipSuccess) return nullptr;
            (void)hipFree(a.p);
        }
        a = NetDev::B2Act();
        if (hipMalloc(&a.p, (size_t)wgs * WINO_B2_WG) != hipSuccess) { a.p = nullptr; return nullptr; }
        a.wgs = wgs;
    }
    return static_cast<char*>(a.p);
}

int tower_forward(NetDev* n, const void* planes, const int* count, int rows, float* pol, float* val,
                  const SearchOut* so, hipStream_t st) {
    if (rows <= 0) return 0;
    if (!tower_supported(n)) return fail("fused tower: unsupported net");
    if (!planes && (!so || !so->npos)) return fail("fused tower: no planes and no leaf positions to encode");
    if (n->dtype == AZ_DTYPE_FP8) return tower8_forward(n, planes, count, rows, pol, val, so, st);
    TowerArgs ta = tower_args(n);
    SearchOut dummy;
    memset(&dummy, 0, sizeof(dummy));
    const SearchOut& s = so ? *so : dummy;
#define AZ_TOWER(FF)                                                                                           \
    if (n->filters == FF) {                                                                                    \
        constexpr int BPB = TowerCfg<FF>::BPB;                                                                 \
        constexpr int NT = (FF / (16 * TowerCfg<FF>::NCO)) * TowerCfg<FF>::WB * 64;                            \
        const int grid = (rows + BPB - 1) / BPB;                                                               \
        if (so) tower_kernel<FF, true><<<grid, NT, 0, st>>>((const __bf16*)planes, ta, count, rows, pol, val, s); \
        else tower_kernel<FF, false><<<grid, NT, 0, st>>>((const __bf16*)planes, ta, count, rows, pol, val, s);  \
        return hipGetLastError() == hipSuccess ? 0 : fail("tower launch failed");                              \
    }
#define AZ_TOWER32(FF)                                                                                          \
    if (n->filters == FF) {                                                                                    \
        constexpr int BPB = Tower32Cfg<FF>::BPB;                                                               \
        constexpr int NT = (FF / (16 * Tower32Cfg<FF>::NCO)) * Tower32Cfg<FF>::WB * 64;                        \
        const int grid = (rows + BPB - 1) / BPB;                                                               \
        if (so) tower32_kernel<FF, true><<<grid, NT, 0, st>>>((const float*)planes, ta, count, rows, pol, val, s); \
        else tower32_kernel<FF, false><<<grid, NT, 0, st>>>((const float*)planes, ta, count, rows, pol, val, s);  \
        return hipGetLastError() == hipSuccess ? 0 : fail("f32 tower launch failed");                          \
    }
    if (n->dtype == AZ_DTYPE_F32) {
#define AZ_TOWER32W(FF, H16, SP, ROWS, VR)                                                                       \
        if (n->filters == FF) {                                                                                \
            constexpr int NT = WinoCfg<FF>::NWV * 64;                                                          \
            if (so) tower32w_kernel<FF, true, H16, SP, ROWS, VR><<<rows, NT, 0, st>>>((const float*)planes, ta, count, rows, pol, val, s); \
            else tower32w_kernel<FF, false, H16, SP, ROWS, VR><<<rows, NT, 0, st>>>((const float*)planes, ta, count, rows, pol, val, s);  \
            return hipGetLastError() == hipSuccess ? 0 : fail("f32 Winograd tower launch failed");             \
        }
        if (wino_split16(n)) {
            if (n->filters == 256 && n->wino_streamed == 12 && n->wino_rows && n->wino_vrows && n->wino_boards == 2) {
                // two batch rows per workgroup, their residual activations in the stream's global ACT
                const int grid = (rows + 1) / 2;
                char* act = b2_act_for(n, st, grid);
                if (!act) return fail("two-board tower: global activations allocation failed");
                if (so) tower32w2_kernel<true><<<grid, 512, 0, st>>>((const float*)planes, ta, count, rows, act, pol, val, s);
                else tower32w2_kernel<false><<<grid, 512, 0, st>>>((const float*)planes, ta, count, rows, act, pol, val, s);
                return hipGetLastError() == hipSuccess ? 0 : fail("f32 Winograd tower launch failed");
            }
            if (n->wino_streamed == 12 && n->wino_rows && n->wino_vrows) { AZ_TOWER32W(256, true, 12, true, true) }
            if (n->wino_streamed == 12 && n->wino_rows) { AZ_TOWER32W(256, true, 12, true, false) }
            if (n->wino_streamed == 12) { AZ_TOWER32W(256, true, 12, false, false) }
            AZ_TOWER32W(256, true, 16, false, false) AZ_TOWER32W(128, true, 16, false, false) AZ_TOWER32W(64, true, 16, false, false)
        }
        if (wino_supported(n)) {
            AZ_TOWER32W(256, false, 16, false, false) AZ_TOWER32W(128, false, 16, false, false) AZ_TOWER32W(64, false, 16, false, false)
        }
#undef AZ_TOWER32W
        AZ_TOWER32(256) AZ_TOWER32(128) AZ_TOWER32(64) AZ_TOWER32(32)
        return fail("fused tower: unsupported filters");
    }
    AZ_TOWER(256) AZ_TOWER(128) AZ_TOWER(64) AZ_TOWER(32)
#undef AZ_TOWER
#undef AZ_TOWER32
    return fail("fused tower: unsupported filters");
}

}  // namespace azi

// the shared-row V layout's address functions (wino.h wino_vr_*), tabulated on the host (include/az.h)
extern "C" int az_wino_vrows_layout(int* write, int* read, int* act, int* item, int* dims) {
    using namespace azi;
    if (!write || !read || !act || !item || !dims) return fail("null argument");
    for (int q = 0; q < WINO_VR_ITEMS; q++)
        for (int lane = 0; lane < 64; lane++)
            for (int k = 0; k < 4; k++) {
                write[(q * 64 + lane) * 4 + k] = wino_vr_write(q, lane, k);
                act[(q * 64 + lane) * 4 + k] = wino_vr_act(q, lane, k);
            }
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 4; b++)
            for (int lane = 0; lane < 64; lane++) {
                read[(i * 4 + b) * 64 + lane] = wino_vr_read(i, b, lane);
                read[((4 + i) * 4 + b) * 64 + lane] = wino_vr_lo(wino_vr_rlane(lane, i >> 1)) + wino_vr_rimm(i, b);
            }
    for (int sched = 0; sched < 2; sched++)
        for (int wave = 0; wave < 8; wave++)
            for (int it = 0; it < 4; it++) {
                const int nw = sched ? 8 : 4;
                item[(sched * 8 + wave) * 4 + it] = wave < nw && it < WINO_VR_ITEMS / nw ? wino_vr_item(wave, it, nw) : -1;
            }
    dims[0] = WINO_VR_PLANE; dims[1] = WINO_VR_BYTES; dims[2] = WINO_VR_R16; dims[3] = 4;
    return 0;
}

// the two-board tower's layout (wino.h wino_b2_*, the LDS regions of tower32w_boards2), tabulated on the host
extern "C" int az_wino_boards_layout(int* item, int* act, int* out, int* vbuf, int* zero, int* dims) {
    using namespace azi;
    if (!item || !act || !out || !vbuf || !zero || !dims) return fail("null argument");
    for (int w = 0; w < 8; w++)
        for (int k = 0; k < 8; k++) {
            item[(w * 8 + k) * 2] = k < wino_b2_item_count(w) ? wino_b2_item_board(w, k) : -1;
            item[(w * 8 + k) * 2 + 1] = k < wino_b2_item_count(w) ? wino_b2_item_q(w, k) : -1;
        }
    for (int nb = 0; nb < 2; nb++)
        for (int b = 0; b < 2; b++) {
            act[nb * 2 + b] = wino_b2_act(nb, b);
            vbuf[nb * 2 + b] = wino_b2_v(nb, b);
        }
    for (int w = 0; w < 8; w++)
        for (int lane = 0; lane < 64; lane++)
            for (int n = 0; n < 2; n++)
                for (int q = 0; q < 4; q++) out[((w * 64 + lane) * 2 + n) * 4 + q] = wino_b2_out(w, lane, n, q);
    for (int k = 0; k < 64; k++) zero[k] = wino_vr_zero(k);
    dims[0] = WINO_B2_ACT; dims[1] = WINO_B2_WG; dims[2] = WINO_VR_BYTES; dims[3] = WINO_B2_OVL; dims[4] = WINO_B2_ACT;
    dims[5] = WINO_B2_VBYTES; dims[6] = WINO_B2_AUX * 16; dims[7] = WINO_B2_LDS;
    return 0;
}

#ifdef AZ_TOWER_TRACE
// trace build only: copy the phase stamps of the last tower launch (AZ_TT_WG x 8 waves x
// AZ_TT_SLOTS u64) to the host
extern "C" int az_tower_trace_read(unsigned long long* out, size_t n) {
    const size_t cap = sizeof(azi::az_tower_trace_buf) / sizeof(unsigned long long);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(azi::az_tower_trace_buf), (n < cap ? n : cap) * 8) == hipSuccess ? 0 : -1;
}
#endif
