// tower_dev.h -- device code shared by the fused towers (tower.hip: bf16 and f32; tower8.hip: MX-fp8):
// the launch arguments, the workgroup shapes, the bf16 3x3 conv layer LDS -> LDS and the heads.
#pragma once
#include "az_internal.h"
#include "search_dev.h"
#include "wino.h"

// Tuning constants (the A/B logs under profiles/ measured each alternative):
//   TOWER_LA 4   bf16 tower: activation (B-fragment) LDS reads issued this many fragments ahead
//   TOWER_PF 2   bf16 tower: weight prefetch depth in k-steps (4 measured no faster)
//   HEADS_KPRE 64  value-FC rows per wave prefetched into registers before the heads' 1x1 conv
constexpr int TOWER_LA = 4, TOWER_PF = 2, HEADS_KPRE = 64;

namespace azi {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

struct TowerArgs {
    const uint4* w[1 + 2 * 40];    // swizzled conv weights (input conv, then conv1/conv2 per block)
    const float* b[1 + 2 * 40];    // folded biases
    const float* head;
    const uint4* head_frag;        // 1x1 F->40 head conv as bf16 hi/lo MFMA A-fragments (net.hip)
    const uint4* head_frag32;      // the same conv as f32 A-fragments (f32 tower)
    unsigned wbytes[1 + 2 * 40];   // allocation bytes of each w[i] (buffer-load range check)
    const uint4* ww[2 * 40];       // Winograd weights of the residual convs (tower32w_kernel): f32, or split-f16 (wus)
    unsigned wwbytes[2 * 40];
    float wus[2 * 40];             // split-f16 products: each conv's unscale 1 / (Sa Sw) (ww = the f16 hi / lo weights)
    const uint4* w0pk;             // the input conv packed for tower32w_kernel (net.hip swizzle_f32_input_packed)
    unsigned w0pk_bytes;
    int blocks;
};

// BPB boards per workgroup; NCO 16-channel output fragments per wave; WB board groups.
// waves = (F / (16*NCO)) * WB
template <int F> struct TowerCfg;
// F = 256: 8 waves x 2 boards (16 waves, WB = 2, measured 10 % slower: spills); F = 64: 4 waves of 16
// channels, one per SIMD (NCO 2 left 2 SIMDs idle: C2 tower 52 -> 41 us), one board per workgroup
template <> struct TowerCfg<256> { static constexpr int BPB = 2, WB = 1, NCO = 2; };
template <> struct TowerCfg<128> { static constexpr int BPB = 4, WB = 1, NCO = 2; };
template <> struct TowerCfg<64> { static constexpr int BPB = 1, WB = 1, NCO = 1; };   // C2: 256 games -> 256 workgroups
template <> struct TowerCfg<32> { static constexpr int BPB = 8, WB = 4, NCO = 2; };

__device__ __forceinline__ float t_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float t_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One 3x3 conv layer LDS -> LDS.  IN: CIN channels, row stride RSI slots; OUT: F channels,
// row stride RSO slots.  Wave (cw, bw) computes channels [32cw, 32cw+32) of boards
// [bw*BPW, (bw+1)*BPW).  RESID: out = relu(conv(in) + bias + out).
template <int NCH> struct RingPF { static constexpr int PF = NCH >= TOWER_PF ? TOWER_PF : NCH; };

// Load k-steps [0, PF) of a layer's weight fragments into the ring.
template <int NCH, int F, int NCO>
__device__ __forceinline__ void ring_fill(uint4 (&wr)[RingPF<NCH>::PF][NCO], const uint4* __restrict__ wsw, int cw,
                                          int lane) {
    constexpr int CF = F / 16;
    const uint4* W = wsw + (size_t)(cw * NCO) * 64 + lane;
#pragma unroll
    for (int i = 0; i < RingPF<NCH>::PF; i++)
#pragma unroll
        for (int n = 0; n < NCO; n++) wr[i][n] = W[(size_t)i * CF * 64 + n * 64];
}

// wr: register ring holding this layer's next PF weight k-steps on entry; on exit it holds
// the first PF k-steps of `wnext` (the next layer with the same chunk count), or zeros.
template <int CIN, int RSI, int F, int RSO, int BPW, int NCO, bool RESID>
__device__ __forceinline__ void conv_lds(const char* __restrict__ ldsb, uint4* __restrict__ out_lds, int in_off,
                                         int zero_off, const uint4* __restrict__ wsw, const uint4* __restrict__ wnext,
                                         const float* __restrict__ bias, uint4 (&wr)[RingPF<CIN / 32>::PF][NCO],
                                         int cw, int bw, int lane, unsigned wbytes, unsigned nbytes) {
    constexpr int NCH = CIN / 32;                     // 32-channel K chunks (4 slots)
    constexpr int CF = F / 16;
    constexpr int MF = BPW * 4;
    constexpr int KS = 9 * NCH;
    // weight fragments are prefetched PF k-steps ahead through a register ring; PF divides the
    // chunk count so the ring slot of every k-step is a compile-time constant
    constexpr int PF = RingPF<NCH>::PF;
    static_assert(NCH % PF == 0, "prefetch depth must divide the chunk count");
    const int h = lane >> 4;
    // accumulators start at the folded bias: no bias adds in the epilogue
    f32x4 acc[MF][NCO];
#pragma unroll
    for (int n = 0; n < NCO; n++) {
        const float4 bn = *reinterpret_cast<const float4*>(bias + cw * 16 * NCO + n * 16 + h * 4);
#pragma unroll
        for (int m = 0; m < MF; m++) acc[m][n] = f32x4{bn.x, bn.y, bn.z, bn.w};
    }
    // weight refills as buffer loads: SGPR descriptor + per-lane VGPR offset + the k-step's byte
    // offset in an SGPR -- no 64-bit VALU address adds (and their carry-hazard nops) in the MFMA
    // stream (C3 A/B: tower -2.7 %); num_records = the real allocation (this layer's k-steps + its
    // 8 zero k-steps of prefetch pad), past the last k-step the refills read the next layer
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)wsw, (short)0, (int)wbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rN = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(wnext ? wnext : wsw + (size_t)KS * CF * 64), (short)0,
        (int)(wnext ? nbytes : wbytes - (unsigned)KS * CF * 64 * 16), 0x00020000);
    const int voff = ((cw * NCO) * 64 + lane) * 16;
    // B-fragment (activation) reads run LA fragments ahead, across k-step and tap boundaries
    constexpr int LA = TOWER_LA < MF ? TOWER_LA : MF;
    static_assert(MF % LA == 0, "read-ahead ring must tile the fragment loop");
    // Per-tap LDS addresses of the B fragments, branch-free.  Valid taps read the shifted square;
    // off-board taps read the zero row at the same 16-B slot mod 16 (conflict-free): in_off and
    // zero_off are multiples of 256 B and every row offset keeps the slot, so the zero address is
    // zero_off | (valid-form address & 0xF0).
    const int lane_off = (((lane & 15) * RSI) + h) * 16;
    const int lr = (lane & 15) >> 3, lf = lane & 7;
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
                const int vz = (va & 0xF0) | zero_off;
                base[m] = ok ? va : vz;
            }
        }
    };
    int bcur[MF], bnext[MF];
    uint4 bq[LA];
    tap_bases(0, bcur);
#pragma unroll
    for (int m = 0; m < LA; m++) bq[m] = *reinterpret_cast<const uint4*>(ldsb + bcur[m]);
    // the 9-tap loop fully unrolled: every tap's LDS offsets and off-board masks are compile-time
    // and no accumulator copies cross a loop edge (C3 A/B: tower -2.7 %)
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        tap_bases(tap < 8 ? tap + 1 : 8, bnext);
#pragma unroll
        for (int c4 = 0; c4 < NCH; c4++) {
            uint4 a[NCO];
#pragma unroll
            for (int n = 0; n < NCO; n++) a[n] = wr[c4 % PF][n];
            // refill this ring slot with the k-step PF positions later in the sequence (the next
            // tap, or the next layer once past the end)
            {
                int kidx;
                bool nxt = false;
                if (c4 + PF < NCH) kidx = tap * NCH + c4 + PF;
                else if (tap < 8) kidx = (tap + 1) * NCH + c4 + PF - NCH;
                else { kidx = c4 + PF - NCH; nxt = true; }
                const int soff = kidx * CF * 64 * 16;
#pragma unroll
                for (int n = 0; n < NCO; n++)
                    wr[c4 % PF][n] = __builtin_bit_cast(
                        uint4, __builtin_amdgcn_raw_buffer_load_b128(nxt ? rN : rW, voff + n * 1024, soff, 0));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < MF; m++) {
                const uint4 bv = bq[m % LA];
                if (m + LA < MF) {
                    bq[m % LA] = *reinterpret_cast<const uint4*>(ldsb + bcur[m + LA] + c4 * 64);
                } else if (c4 + 1 < NCH) {                   // next k-step, same tap
                    bq[m % LA] = *reinterpret_cast<const uint4*>(ldsb + bcur[m + LA - MF] + (c4 + 1) * 64);
                } else {                                     // first k-step of the next tap
                    bq[m % LA] = *reinterpret_cast<const uint4*>(ldsb + bnext[m + LA - MF]);
                }
                const bf16x8 Bv = __builtin_bit_cast(bf16x8, bv);
#pragma unroll
                for (int n = 0; n < NCO; n++)
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[n]), Bv,
                                                                        acc[m][n], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < MF; m++) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, NCO, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int m = 0; m < MF; m++) bcur[m] = bnext[m];
    }
    // `in` and `out` are different buffers, so the epilogue needs no barrier before it;
    // the barrier after it publishes `out` to the next layer.
    char* ob = reinterpret_cast<char*>(out_lds);
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    typedef __attribute__((ext_vector_type(2))) short s16x2;
    const s16x2 z = {0, 0};
#pragma unroll
    for (int n = 0; n < NCO; n++) {
        const int co = cw * 16 * NCO + n * 16 + h * 4;
        // per-lane base; each fragment adds a compile-time offset (ds_write immediate)
        char* lane_base = ob + ((bw * BPW * 64 + (lane & 15)) * RSO + (co >> 3)) * 16 + (co & 7) * 2;
#pragma unroll
        for (int m = 0; m < MF; m++) {
            uint2* dst = reinterpret_cast<uint2*>(lane_base + ((m >> 2) * 64 + (m & 3) * 16) * RSO * 16);
            f32x2 lo = {acc[m][n][0], acc[m][n][1]}, hi = {acc[m][n][2], acc[m][n][3]};
            if constexpr (RESID) {
                const uint2 r = *dst;                       // bf16 -> f32 is a 16-bit shift
                lo += f32x2{__builtin_bit_cast(float, r.x << 16), __builtin_bit_cast(float, r.x & 0xFFFF0000u)};
                hi += f32x2{__builtin_bit_cast(float, r.y << 16), __builtin_bit_cast(float, r.y & 0xFFFF0000u)};
            }
            // round to bf16 (v_cvt_pk_bf16_f32), then ReLU as a signed 16-bit max with 0
            s16x2 q0 = __builtin_bit_cast(s16x2, __builtin_convertvector(lo, bf16x2));
            s16x2 q1 = __builtin_bit_cast(s16x2, __builtin_convertvector(hi, bf16x2));
            q0 = __builtin_elementwise_max(q0, z);
            q1 = __builtin_elementwise_max(q1, z);
            *dst = make_uint2(__builtin_bit_cast(unsigned, q0), __builtin_bit_cast(unsigned, q1));
        }
    }
    __syncthreads();
}

// Heads v2 for NB boards [b0, b0 + NB) of the workgroup, from the LDS image x (bf16, or f32 when
// F32X, row stride RS slots), scratch in H; every one of the NT threads reaches every barrier.
//   A: 1x1 F->40 (policy conv 32 + value conv 8, BN folded) on v_mfma_f32_16x16x32_bf16 with the
//      f32 weights split into bf16 hi + lo fragments (16 mantissa bits; activations are bf16
//      already), or for f32 activations on v_mfma_f32_16x16x4_f32 (exact f32), bias + ReLU ->
//      p1v1 (f32);
//   B: policy 1x1 32->64 on v_mfma_f32_16x16x4_f32 (exact f32 products) -> 4096 logits;
//   C: value Linear 512->64 (K split over the waves), ReLU, Linear 64->1, tanh (f32 VALU);
//   then softmax over 4096 and the dense rows or, in search mode, the priors gathered at the
//   new node's legal edges (agent.rs:112-144, tree.rs:84-104).
template <int F> struct HeadsCfg { static constexpr int NB = F >= 128 ? 2 : 1; };
constexpr int HEADS_P1S = 80;                           // p1v1 row stride in floats (conflict-free B reads)
// NPART partial value-FC sums per (board, wave): 4 for the 4-wave f32 heads (WIDE)
constexpr int heads_npart(int NT, bool F32X) { return F32X && NT <= 256 ? 4 : 1; }
template <int NB, int NT, int NPART = 1> struct HeadsScratch {
    static constexpr int PV = 40 * HEADS_P1S, NW = NT / 64;
    static constexpr int P1 = 0, LG = P1 + NB * PV, RED = LG + NB * 4096, STAT = RED + NB * NW * 64 * NPART;
    static constexpr int FLOATS = STAT + NB * (2 * NW + 4);
};

// ReLU; KEEP: a NaN stays NaN (fmaxf returns its other operand).  The split-f16 tower marks an
// activation beyond the f16 range with NaN (wino.h WinoXf::split16), and that NaN has to reach
// the policy and the value
template <bool KEEP> __device__ __forceinline__ float relu_nan(float v) {
    if constexpr (KEEP) return v < 0.0f ? 0.0f : v;
    else return fmaxf(v, 0.0f);
}

// NANKEEP: the two ReLUs keep NaN; the softmax and tanh behind them then give NaN (a NaN logit is
// skipped by the max and makes the exp sum NaN)
template <int F, int RS, int NB, int NT, bool SEARCH, bool F32X = false, bool NANKEEP = false>
__device__ __forceinline__ void heads_group(const char* __restrict__ xb, float* __restrict__ scr, int b0, int nb,
                                            int row0, int tid, const uint4* __restrict__ hfrag,
                                            const float* __restrict__ head, float* pol_out, float* val_out,
                                            const SearchOut& so, unsigned long long* tr = nullptr) {
    constexpr int NPART = heads_npart(NT, F32X);
    wino_stamp(tr, 1900);
    typedef HeadsScratch<NB, NT, NPART> S;
    constexpr int NW = S::NW, PV = S::PV, P1S = HEADS_P1S;
    const HeadLayout L = HeadLayout::make(F);
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), h = lane >> 4, l16 = lane & 15;
    float* p1v1 = scr + S::P1;
    float* lg = scr + S::LG;
    float* red = scr + S::RED;
    float* stat = scr + S::STAT;                        // per board: [NW] max, [NW] sum, value, slot, prior off
    // weights of B and C are fetched into registers first: their latency hides behind A
    constexpr int TPW = 16 * NB / NW;                   // policy tiles per wave
    // value-FC rows prefetched per wave: all of them for the f32 towers' 4-wave workgroups (one wave
    // per SIMD, registers to spare)
    constexpr int KPMAX = (F32X && NW <= 4) ? 128 : HEADS_KPRE;
    constexpr int KP = 512 / NW, KPRE = KP < KPMAX ? KP : KPMAX;
    // 4-wave f32 heads: the value FC with each lane on 4 output units x every 4th row of the wave's
    // rows (16-byte coalesced weight reads, 4x fewer load instructions); partial sums per lane group
    constexpr bool WIDE = F32X && NW <= 4;
    // f32 with 4 waves: A's first KA 16-channel weight groups are requested before everything else,
    // so that the 1x1 conv does not wait behind the B / C prefetch
    constexpr int KA = (F32X && NW <= 4) ? (F / 16 < 4 ? F / 16 : 4) : 0;
    f32x4 hA[KA > 0 ? KA : 1][3];
    if constexpr (KA > 0) {
        if (w < 4 * NB) {
#pragma unroll
            for (int kc = 0; kc < KA; kc++)
#pragma unroll
                for (int cf = 0; cf < 3; cf++) hA[kc][cf] = __builtin_bit_cast(f32x4, hfrag[(kc * 3 + cf) * 64 + lane]);
        }
    }
    float pa[TPW > 0 ? TPW : 1][8];
#pragma unroll
    for (int k = 0; k < TPW; k++) {
        const int t = w + k * NW, cf = (t >> 2) & 3;
        if constexpr (KA > 0) {   // 4-wave f32 heads: the fragment copy, one 32-byte read per lane
            const f32x4* src = reinterpret_cast<const f32x4*>(head + L.p2f + ((size_t)cf * 64 + lane) * 8);
            const f32x4 lo = src[0], hi = src[1];
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
                pa[k][ks] = lo[ks];
                pa[k][ks + 4] = hi[ks];
            }
        } else {   // (the wider read costs the 8-wave F = 256 kernel a spill)
#pragma unroll
            for (int ks = 0; ks < 8; ks++) pa[k][ks] = head[L.p2w + (cf * 16 + l16) * 32 + h + ks * 4];
        }
    }
    float wv[KPRE > 0 && !WIDE ? KPRE : 1];
    f32x4 wq[WIDE ? KP / 4 : 1];
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < KP / 4; i++)
#ifdef AZ_HEADS_NOVFC   // timing-only bound (wrong values): no value-FC weight stream
            wq[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#else
            wq[i] = *reinterpret_cast<const f32x4*>(head + L.l1w + (size_t)(w * KP + 4 * i + h) * 64 + 4 * l16);
#endif
    } else {
#pragma unroll
        for (int i = 0; i < KPRE; i++) wv[i] = head[L.l1w + (size_t)(w * KP + i) * 64 + lane];
    }
    // biases of A, B and the value head, and (search mode) the new node's record: requested here,
    // behind the weight prefetches, so that no phase ends on a dependent global load (C2 heads
    // stamps: ~1-2k cycles each)
    f32x4 b40v[3];
#pragma unroll
    for (int cf = 0; cf < 3; cf++) b40v[cf] = *reinterpret_cast<const f32x4*>(head + L.b40 + cf * 16 + 4 * h);
    f32x4 p2bv[TPW > 0 ? TPW : 1];
#pragma unroll
    for (int k = 0; k < TPW; k++)
        p2bv[k] = *reinterpret_cast<const f32x4*>(head + L.p2b + ((w + k * NW) >> 2 & 3) * 16 + 4 * h);
    const float l1bv = head[L.l1b + lane], l2wv = head[L.l2w + lane], l2bv = head[L.l2b];
    int sgame[NB], snode[NB];
    Node snd[NB];
    if constexpr (SEARCH) {
#pragma unroll
        for (int bb = 0; bb < NB; bb++) {
            if (b0 + bb < nb) {
                const int row = vgpr_index(row0 + b0 + bb);
                sgame[bb] = so.row_game[row];
                snode[bb] = so.row_node[row];
                snd[bb] = so.nodes[(size_t)sgame[bb] * so.NMAX + snode[bb]];
            }
        }
    }
    // A
    for (int sfr = w; sfr < 4 * NB; sfr += NW) {
        const int bb = sfr >> 2, sq = (sfr & 3) * 16 + l16;
        const char* xr = xb + ((size_t)(b0 + bb) * 64 + sq) * RS * 16 + h * 16;
        f32x4 acc[3];
#pragma unroll
        for (int cf = 0; cf < 3; cf++) acc[cf] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (F32X) {
            // f32 activations: exact f32 products on v_mfma_f32_16x16x4_f32, one 16-channel k-chunk
            // (a float4 per lane) per 4 MFMAs
#pragma unroll
            for (int kc = 0; kc < KA; kc++) {
                const f32x4 Bv = *reinterpret_cast<const f32x4*>(xr + kc * 64);
#pragma unroll
                for (int s4 = 0; s4 < 4; s4++)
#pragma unroll
                    for (int cf = 0; cf < 3; cf++)
                        acc[cf] = __builtin_amdgcn_mfma_f32_16x16x4f32(hA[kc][cf][s4], Bv[s4], acc[cf], 0, 0, 0);
            }
#pragma unroll 4
            for (int kc = KA; kc < F / 16; kc++) {
                const f32x4 Bv = *reinterpret_cast<const f32x4*>(xr + kc * 64);
#pragma unroll
                for (int cf = 0; cf < 3; cf++) {
                    const f32x4 Av = __builtin_bit_cast(f32x4, hfrag[(kc * 3 + cf) * 64 + lane]);
#pragma unroll
                    for (int s4 = 0; s4 < 4; s4++)
                        acc[cf] = __builtin_amdgcn_mfma_f32_16x16x4f32(Av[s4], Bv[s4], acc[cf], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < F / 32; ks++) {
                const bf16x8 Bv = *reinterpret_cast<const bf16x8*>(xr + ks * 64);
#pragma unroll
                for (int cf = 0; cf < 3; cf++)
#pragma unroll
                    for (int hl = 0; hl < 2; hl++)
                        acc[cf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            __builtin_bit_cast(bf16x8, hfrag[((ks * 3 + cf) * 2 + hl) * 64 + lane]), Bv, acc[cf], 0, 0,
                            0);
            }
        }
#pragma unroll
        for (int cf = 0; cf < 3; cf++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int ch = cf * 16 + 4 * h + r;
                if (ch < 40) p1v1[bb * PV + ch * P1S + sq] = relu_nan<NANKEEP>(acc[cf][r] + b40v[cf][r]);
            }
    }
    wino_stamp(tr, 1901);
    __syncthreads();
    wino_stamp(tr, 1902);
    // B
    float mxb[NB];
#pragma unroll
    for (int bb = 0; bb < NB; bb++) mxb[bb] = -INFINITY;
#pragma unroll
    for (int k = 0; k < TPW; k++) {
        const int t = w + k * NW;
        const int bb = t >> 4, cf = (t >> 2) & 3, sf = t & 3;
        const float* pb = p1v1 + bb * PV + h * P1S + sf * 16 + l16;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ks = 0; ks < 8; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k][ks], pb[ks * 4 * P1S], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int c2 = cf * 16 + 4 * h + r;
            const float l = acc[r] + p2bv[k][r];
            lg[bb * 4096 + c2 * 64 + sf * 16 + l16] = l;
#pragma unroll
            for (int q = 0; q < NB; q++)
                if (q == bb) mxb[q] = fmaxf(mxb[q], l);
        }
    }
    // C: value FC, wave w owns K rows [w*KP, (w+1)*KP), lane = output unit
    if constexpr (WIDE) {
        f32x4 a[NB];
#pragma unroll
        for (int bb = 0; bb < NB; bb++) a[bb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < KP / 4; i++) {
            const int k = w * KP + 4 * i + h, c = 32 + (k >> 6), sq = k & 63;
#pragma unroll
            for (int bb = 0; bb < NB; bb++) a[bb] += p1v1[bb * PV + c * P1S + sq] * wq[i];
        }
#pragma unroll
        for (int bb = 0; bb < NB; bb++) *reinterpret_cast<f32x4*>(red + ((bb * NW + w) * 4 + h) * 64 + 4 * l16) = a[bb];
    } else {
        float a[NB];
#pragma unroll
        for (int bb = 0; bb < NB; bb++) a[bb] = 0.0f;
#pragma unroll
        for (int i = 0; i < KP; i++) {
            const int k = w * KP + i, c = 32 + (k >> 6), sq = k & 63;
            const float wgt = i < KPRE ? wv[i < KPRE ? i : 0] : head[L.l1w + (size_t)k * 64 + lane];
#pragma unroll
            for (int bb = 0; bb < NB; bb++) a[bb] += p1v1[bb * PV + c * P1S + sq] * wgt;
        }
#pragma unroll
        for (int bb = 0; bb < NB; bb++) red[(bb * NW + w) * 64 + lane] = a[bb];
    }
#pragma unroll
    for (int bb = 0; bb < NB; bb++) {
        const float m = t_wave_max(mxb[bb]);
        if (lane == 0) stat[bb * (2 * NW + 4) + w] = m;
    }
    wino_stamp(tr, 1903);
    __syncthreads();
    wino_stamp(tr, 1904);
    float mx[NB];
#pragma unroll
    for (int bb = 0; bb < NB; bb++) {
        float m = -INFINITY;
        for (int i = 0; i < NW; i++) m = fmaxf(m, stat[bb * (2 * NW + 4) + i]);
        mx[bb] = m;
        float e = 0.0f;
        for (int i = tid; i < 4096; i += NT) e += expf(lg[bb * 4096 + i] - m);
        e = t_wave_sum(e);
        if (lane == 0) stat[bb * (2 * NW + 4) + NW + w] = e;
    }
    if (w < NB) {                                       // wave bb finishes board bb's value head
        const int bb = w;
        float hs = l1bv;
        for (int i = 0; i < NW * NPART; i++) hs += red[(bb * NW * NPART + i) * 64 + lane];
        float hv = t_wave_sum(relu_nan<NANKEEP>(hs) * l2wv);
        if (lane == 0) stat[bb * (2 * NW + 4) + 2 * NW] = tanhf(hv + l2bv);
    }
    if constexpr (SEARCH) {                             // thread 0 reserves eval-log slots
        if (tid == 0 && so.log_cap > 0) {
#pragma unroll
            for (int bb = 0; bb < NB; bb++) {
                int* sl = reinterpret_cast<int*>(stat + bb * (2 * NW + 4) + 2 * NW + 1);
                sl[0] = -1;
                if (b0 + bb >= nb) continue;
                const Node nd = snd[bb];
                const int r = atomicAdd(&so.ctr->log_count, 1);
                const int po = atomicAdd(&so.ctr->log_prior_count, (int)nd.nedges);
                sl[0] = (r < so.log_cap && po + nd.nedges <= so.log_prior_cap) ? r : -1;
                sl[1] = po;
            }
        }
    }
    wino_stamp(tr, 1905);
    __syncthreads();
    wino_stamp(tr, 1906);
#pragma unroll
    for (int bb = 0; bb < NB; bb++) {
        if (b0 + bb >= nb) break;
        const float* st = stat + bb * (2 * NW + 4);
        float sum = 0.0f;
        for (int i = 0; i < NW; i++) sum += st[NW + i];
        const float value = st[2 * NW];
        const int row = vgpr_index(row0 + b0 + bb);
        const float* lb = lg + bb * 4096;
        if constexpr (!SEARCH) {
            float* pr = pol_out + (size_t)row * 4096;
            for (int i = tid; i < 4096; i += NT) pr[i] = expf(lb[i] - mx[bb]) / sum;
            if (tid == 0) val_out[row] = value;
        } else {
            const int game = sgame[bb], node = snode[bb];
            const Node nd = snd[bb];
            Edge* e = so.edges + (size_t)game * so.EMAX + nd.edge_begin;
            const int* sl = reinterpret_cast<const int*>(st + 2 * NW + 1);
            const int slot = so.log_cap > 0 ? sl[0] : -1;
            for (int i = tid; i < nd.nedges; i += NT) {
                const int idx = e[i].idx & azc::IDX_MASK;
                const float P = expf(lb[idx] - mx[bb]) / sum;
                e[i].P = P;
                if (slot >= 0) {
                    so.log_idx[sl[1] + i] = idx;
                    so.log_prior[sl[1] + i] = P;
                }
            }
            if (tid == 0) {
                so.value[row] = value;
                if (slot >= 0) {
                    so.log_key[slot] = azc::fen_key(so.npos[(size_t)game * so.NMAX + node]);
                    so.log_value[slot] = value;
                    so.log_off[slot] = sl[1];
                    so.log_n[slot] = nd.nedges;
                }
            }
        }
    }
    __syncthreads();
}

}  // namespace azi
