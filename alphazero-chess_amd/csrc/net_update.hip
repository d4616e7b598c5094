// net_update.hip -- rewrite an existing net's weight buffers in place from flat f32 parameters that are
// already in HBM (model.valid() without leaving the device, training.rs:83).
//
// net_create (net.hip) folds the BatchNorms and builds every packed layout on the host, one conv after
// another; it stays the reference.  Here the same arithmetic runs as HIP kernels over all 1 + 2 blocks
// convs at once (blockIdx.y = the conv), and the result is byte for byte the host's:
//   k_scales      sc[co] = gamma / sqrt(var + 1e-5) in f64 per BatchNorm channel (convs and heads)
//   k_fold        wf = (float)(w sc), bf = (float)((bias - mean) sc + beta) -> the folded-weight scratch
//                 and the bias buffers (conv_b, b8)
//   k_wino_max    split-f16 streams only: each conv's exact max |U| as an integer atomicMax on the f64
//                 bit patterns (non-negative doubles order as their bits, so the result does not depend
//                 on the order), from which every thread of the packer derives the host's Sw
//   k_pack_*      one launch per layout, in gather form: a thread owns 16-byte pieces of the output,
//                 computes them from the 9 folded taps in the host's expression order and stores them
//                 whole; the zero ring steps / k-steps / padded channels are stored too
//   k_pack_heads  the heads' fold, copies, p2f and the two fragment forms
// Every phase boundary is a launch on one stream; nothing waits across workgroups.  -ffp-contract=off
// (Makefile) keeps the device's f64 products and sums as written, like the host's.
#include <math.h>
#include <string.h>

#include <vector>

#include "az_internal.h"

namespace azi {

struct ConvDesc {                       // one conv of the tower (device table, written once)
    unsigned long long w, b, bn;        // offsets (floats) of weight, bias, BatchNorm in the flat parameters
    unsigned long long wf;              // offset of the folded weights [co][cin][9] in the scratch
    int cin, pad;                       // 19 or F
    float* bias_out;                    // conv_b[i], or the conv's row of b8
    void* direct;                       // conv_w[i] (nullptr: an fp8 net's residual conv)
    void* wino;                         // wino_w / wino16_w of a residual conv (nullptr: none)
};

struct HeadOff { unsigned long long p1w, p1b, pbn, p2w, p2b, vw, vb, vbn, l1w, l1b, l2w, l2b; };

struct NetUpdate {
    float* wts = nullptr;               // the flat parameters of the last update
    float* wf = nullptr;                // folded conv weights, all convs
    double* sc = nullptr;               // [nconv][F] then the heads' 40
    ConvDesc* tab = nullptr;
    unsigned long long* umax = nullptr; // [2 blocks] bits of max |U|
    float* us = nullptr;                // [2 blocks] 1 / (Sa Sw)
    size_t count = 0;
    HeadOff ho{};
};

namespace {

__constant__ double kG[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};

__device__ __forceinline__ bool finite_d(double x) {
    return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool sign_d(double x) { return __double_as_longlong(x) < 0; }

// net.hip f16_rne
__device__ uint16_t f16_rne_dev(double x, double* r) {
    if (!finite_d(x)) {
        *r = x;
        return x != x ? 0x7e00 : (sign_d(x) ? 0xfc00 : 0x7c00);
    }
    const double ax = fabs(x);
    int e;
    (void)frexp(ax, &e);
    int q = ax < ldexp(1.0, -14) ? -24 : e - 11;
    double n = nearbyint(ldexp(ax, -q));
    if (n == 2048.0) { n = 1024.0; q++; }
    *r = copysign(ldexp(n, q), x);
    const uint16_t sign = sign_d(x) ? 0x8000 : 0;
    if (n == 0.0) return sign;
    if (q + 25 >= 31) { *r = copysign((double)INFINITY, x); return sign | 0x7c00; }
    if (n < 1024.0) return sign | (uint16_t)n;
    return sign | (uint16_t)(((q + 25) << 10) | ((int)n - 1024));
}

// tower8.hip e4m3_code
__device__ unsigned char e4m3_code_dev(double a) {
    if (!(a <= 448.0)) return a != a ? 0x7F : 0x7E;
    if (a == 0.0) return 0;
    int e;
    (void)frexp(a, &e);
    const int E = e - 1 < -6 ? -6 : e - 1;
    const int n = (int)nearbyint(ldexp(a, 3 - E));
    return (unsigned char)(((E + 7) << 3) + n - 8);
}

__device__ __forceinline__ uint16_t bf16_rne_dev(float v) {
    uint32_t u = __float_as_uint(v);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// U[a][b] of G g G^T (net.hip winograd_f32 / winograd_split16), g = the 9 folded taps
__device__ __forceinline__ double wino_u(const float* g, int a, int b) {
    double gg[3];
#pragma unroll
    for (int j = 0; j < 3; j++) gg[j] = kG[a][0] * g[0 * 3 + j] + kG[a][1] * g[1 * 3 + j] + kG[a][2] * g[2 * 3 + j];
    return gg[0] * kG[b][0] + gg[1] * kG[b][1] + gg[2] * kG[b][2];
}
// W[k][b] of g G^T (net.hip winograd_split16_rows)
__device__ __forceinline__ double rows_w(const float* g, int k, int b) {
    return (double)g[k * 3 + 0] * kG[b][0] + (double)g[k * 3 + 1] * kG[b][1] + (double)g[k * 3 + 2] * kG[b][2];
}

// the host's Sw exponent from the bits of max |U|
__device__ __forceinline__ int wino_se(unsigned long long bits) {
    const double umax = __longlong_as_double((long long)bits);
    int se = 24;
    if (umax > 0.0 && finite_d(umax)) {
        int e;
        (void)frexp(umax, &e);
        se = 15 - e < 24 ? 15 - e : 24;
    }
    return se;
}

__device__ __forceinline__ unsigned long long load_fresh64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ fold
__global__ void __launch_bounds__(256)
k_scales(const float* __restrict__ wts, const ConvDesc* __restrict__ tab, int nconv, int F, HeadOff ho,
         double* __restrict__ sc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nconv * F) {
        const int conv = i / F, co = i - conv * F;
        const float* bn = wts + tab[conv].bn;
        sc[i] = (double)bn[co] / sqrt((double)bn[3 * F + co] + 1e-5);
    } else if (i < nconv * F + 40) {
        const int ch = i - nconv * F;
        const float* bn = ch < 32 ? wts + ho.pbn : wts + ho.vbn;
        const int cout = ch < 32 ? 32 : 8, co = ch < 32 ? ch : ch - 32;
        sc[i] = (double)bn[co] / sqrt((double)bn[3 * cout + co] + 1e-5);
    }
}

__global__ void __launch_bounds__(256)
k_fold(const float* __restrict__ wts, const ConvDesc* __restrict__ tab, const double* __restrict__ sc, int F,
       float* __restrict__ wf) {
    const int conv = blockIdx.y;
    const ConvDesc d = tab[conv];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int per = d.cin * 9;
    if (i >= F * per) return;
    const int co = i / per;
    const double s = sc[(size_t)conv * F + co];
    wf[d.wf + i] = (float)(wts[d.w + i] * s);
    if (i < F) {
        const float* bn = wts + d.bn;
        const double sb = sc[(size_t)conv * F + i];
        d.bias_out[i] = (float)(((double)wts[d.b + i] - bn[2 * F + i]) * sb + bn[F + i]);
    }
}

// ------------------------------------------------------------------ direct 3x3 fragments
// net.hip swizzle_f32 (BF = false: 16 channels per k-step, 4 floats per lane) and swizzle_bf16 (32
// channels, 8 bf16): a thread stores the 16 bytes of lane `lane` of fragment (k-step, cf); the 8 k-steps
// of prefetch padding and the input conv's channels 19-31 are zeros
template <bool BF>
__global__ void __launch_bounds__(256)
k_pack_direct(const float* __restrict__ wf, const ConvDesc* __restrict__ tab, int F) {
    constexpr int KC = BF ? 32 : 16, PL = KC / 4;
    const ConvDesc d = tab[blockIdx.y];
    if (!d.direct) return;
    const int CIN = d.cin == 19 ? 32 : d.cin, CF = F / 16, per = CF * 64;
    const int nk = 9 * CIN / KC;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= (nk + 8) * per) return;
    const int ks = u / per, r = u - ks * per, cf = r >> 6, lane = r & 63;
    float v[PL];
#pragma unroll
    for (int j = 0; j < PL; j++) v[j] = 0.0f;
    if (ks < nk) {
        const int tap = ks / (CIN / KC), co = cf * 16 + (lane & 15);
        const int c0 = (ks % (CIN / KC)) * KC + PL * (lane >> 4);
#pragma unroll
        for (int j = 0; j < PL; j++)
            if (c0 + j < d.cin) v[j] = wf[d.wf + ((size_t)co * d.cin + c0 + j) * 9 + tap];
    }
    if constexpr (BF) {
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 4; j++) p[j] = (uint32_t)bf16_rne_dev(v[2 * j]) | ((uint32_t)bf16_rne_dev(v[2 * j + 1]) << 16);
        reinterpret_cast<uint4*>(d.direct)[u] = make_uint4(p[0], p[1], p[2], p[3]);
    } else {
        reinterpret_cast<float4*>(d.direct)[u] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// net.hip swizzle_f32_input_packed: 12 k-steps + 8 zero ones of the f32 input conv
__global__ void __launch_bounds__(256)
k_pack_in32(const float* __restrict__ wf, const ConvDesc* __restrict__ tab, int F, float4* __restrict__ out) {
    const ConvDesc d = tab[0];
    const int CF = F / 16, per = CF * 64, NK = 12;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= (NK + 8) * per) return;
    const int k = u / per, r = u - k * per, cf = r >> 6, lane = r & 63;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (k < NK) {
        const int co = cf * 16 + (lane & 15), h = lane >> 4;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int tap = k < 9 ? k : 4 * (k - 9) + s;
            const int ci = k < 9 ? 4 * h + s : 16 + h;
            if (tap < 9 && ci < 19) v[s] = wf[d.wf + ((size_t)co * 19 + ci) * 9 + tap];
        }
    }
    out[u] = make_float4(v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------ Winograd f32
// net.hip winograd_f32: a thread owns lane `lane` of tile cf for the 16 input channels of group g16, 4
// of which (ci % 4) are its components, and stores its 16 bytes of each of the 16 points' steps; group
// F/16 is the 8 zero steps
__global__ void __launch_bounds__(256)
k_pack_wino32(const float* __restrict__ wf, const ConvDesc* __restrict__ tab, int F) {
    const ConvDesc d = tab[1 + blockIdx.y];
    const int CF = F / 16, per = CF * 64, NG = F / 16;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= (NG + 1) * per) return;
    const int g16 = u / per, r = u - g16 * per, cf = r >> 6, lane = r & 63;
    float4* out = reinterpret_cast<float4*>(d.wino);
    if (g16 == NG) {
        for (int x = 0; x < 8; x++) out[((size_t)(NG * 16 + x) * CF + cf) * 64 + lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const int co = cf * 16 + (lane & 15), c0 = g16 * 16 + (lane >> 4) * 4;
    float g[4][9];
    const float* src = wf + d.wf + ((size_t)co * F + c0) * 9;
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int t = 0; t < 9; t++) g[s][t] = src[s * 9 + t];
    for (int x = 0; x < 16; x++) {
        const int a = x >> 2, b = x & 3;
        float v[4];
#pragma unroll
        for (int s = 0; s < 4; s++) v[s] = (float)wino_u(g[s], a, b);
        out[((size_t)(g16 * 16 + x) * CF + cf) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ------------------------------------------------------------------ split-f16 streams
// MODE 0: winograd_split16 with 16 streamed points; 1: with 12 (row 2 left out, row 1 negated); 2:
// winograd_split16_rows
template <int MODE> struct W16 {
    static constexpr int STEPS = MODE == 0 ? 16 : 12;
    static constexpr int PADS = MODE == 2 ? WINO_ROWS_PF : 2;
    static constexpr int INNER = MODE == 0 ? 4 : 3;
    // the value of step o INNER + i of a 32-channel group, before the scale
    static __device__ __forceinline__ double value(const float* g, int o, int i, bool* neg) {
        *neg = false;
        if constexpr (MODE == 0) return wino_u(g, o, i);            // step 4 a + b
        if constexpr (MODE == 1) {                                  // step 3 b + (a of 0, 1, 3)
            const int a = i == 2 ? 3 : i;
            *neg = a == 1;
            return wino_u(g, a, o);
        }
        return rows_w(g, i, o);                                     // step 3 b + k
    }
};

// pass 1: max |U| of each residual conv over all 16 points (12 values in the row-direct form), NaNs
// skipped as the host's `fabs(u) > umax` skips them
template <bool ROWS>
__global__ void __launch_bounds__(256)
k_wino_max(const float* __restrict__ wf, const ConvDesc* __restrict__ tab, int F, unsigned long long* __restrict__ umax) {
    const ConvDesc d = tab[1 + blockIdx.y];
    const int cc = blockIdx.x * 256 + threadIdx.x;
    unsigned long long m = 0;
    if (cc < F * F) {
        float g[9];
#pragma unroll
        for (int t = 0; t < 9; t++) g[t] = wf[d.wf + (size_t)cc * 9 + t];
        for (int x = 0; x < (ROWS ? 12 : 16); x++) {
            const double u = ROWS ? rows_w(g, x >> 2, x & 3) : wino_u(g, x >> 2, x & 3);
            if (u == u) {
                const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(u));
                m = bits > m ? bits : m;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(m, o, 64);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&umax[blockIdx.y], m);
}

// pass 2: a thread owns lane `lane` of tile cf for the 32 input channels of group g32 -- its 8
// components ci % 8 -- and stores the hi and the lo fragment piece (16 bytes each) of every streamed
// step; group F/32 is the zero steps at the end of the stream
template <int MODE>
__global__ void __launch_bounds__(256)
k_pack_wino16(const float* __restrict__ wf, const ConvDesc* __restrict__ tab, int F,
              const unsigned long long* __restrict__ umax, float* __restrict__ us) {
    typedef W16<MODE> M;
    const int conv = vgpr_index(blockIdx.y);
    const ConvDesc d = tab[1 + blockIdx.y];
    const int CF = F / 16, per = CF * 64, NG = F / 32;
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= (NG + 1) * per) return;
    const int se = wino_se(load_fresh64(umax + conv));
    if (u == 0) us[conv] = (float)ldexp(1.0 / (double)WINO16_SA, -se);
    const int g32 = u / per, r = u - g32 * per, cf = r >> 6, lane = r & 63;
    uint4* out = reinterpret_cast<uint4*>(d.wino);
    if (g32 == NG) {
        for (int x = 0; x < M::PADS; x++) {
            const size_t at = (((size_t)(NG * M::STEPS + x) * CF + cf) * 2) * 64 + lane;
            out[at] = make_uint4(0, 0, 0, 0);
            out[at + 64] = make_uint4(0, 0, 0, 0);
        }
        return;
    }
    const int co = cf * 16 + (lane & 15), c0 = g32 * 32 + (lane >> 4) * 8;
    float g[8][9];
    const float* src = wf + d.wf + ((size_t)co * F + c0) * 9;
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int t = 0; t < 9; t++) g[j][t] = src[j * 9 + t];
    // the tap row k (MODE 2) indexes g: kept a compile-time value so that g stays in registers
    for (int so = 0; so < M::STEPS / M::INNER; so++)
#pragma unroll
    for (int si = 0; si < M::INNER; si++) {
        const int st = so * M::INNER + si;
        uint32_t hi[4], lo[4];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            bool neg;
            const double sv = ldexp(M::value(g[j], so, si, &neg), se);
            const double s = neg ? -sv : sv;
            double hv, lv;
            const uint32_t h = f16_rne_dev(s, &hv);
            const uint32_t l = f16_rne_dev(s - hv, &lv);
            if (j & 1) { hi[j >> 1] |= h << 16; lo[j >> 1] |= l << 16; }
            else { hi[j >> 1] = h; lo[j >> 1] = l; }
        }
        const size_t at = (((size_t)(g32 * M::STEPS + st) * CF + cf) * 2) * 64 + lane;
        out[at] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        out[at + 64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    }
}

// ------------------------------------------------------------------ MX-fp8
// az_mx8_quantize's scale of block (co, tap, 32 channels from c0): the E8M0 byte and the exponent
struct Mx8Scale { int se; bool finite; };
__device__ Mx8Scale mx8_scale(const float* __restrict__ w, int F, int co, int tap, int c0) {
    float amax = 0.0f;
    bool finite = true;
    for (int i = 0; i < 32; i++) {
        const float v = w[((size_t)co * F + c0 + i) * 9 + tap];
        finite = finite && finite_f(v);
        if (fabsf(v) > amax) amax = fabsf(v);
    }
    int se = 0;
    if (amax > 0.0f && finite) {
        int e;
        (void)frexp((double)amax, &e);
        se = e - 9 < -127 ? -127 : (e - 9 > 127 ? 127 : e - 9);
    }
    return Mx8Scale{se, finite};
}

// tower8.hip mx8_append_conv (quantise per (co, tap, 32 ci), then mx8_fragments): a thread owns lane
// (l16, h) of fragment (k-step, cf) -- 16 codes of block 4 ks + h / 2, 16 of block 4 ks + 2 + h / 2, and
// the scale byte of block 4 ks + h
__global__ void __launch_bounds__(256)
k_pack_mx8(const float* __restrict__ wf, const ConvDesc* __restrict__ tab, int F, uint8_t* __restrict__ w8,
           uint8_t* __restrict__ w8s) {
    const int conv = blockIdx.y;
    const ConvDesc d = tab[1 + conv];
    const int NK = F / 128, CF = F / 16;
    const int fr = blockIdx.x * 256 + threadIdx.x;
    const int nfr = 9 * NK * CF * 64;
    if (fr >= nfr) return;
    const int lane = fr & 63, cf = (fr >> 6) % CF, kidx = (fr >> 6) / CF;
    const int tap = kidx / NK, ks = kidx - tap * NK, co = cf * 16 + (lane & 15), h = lane >> 4;
    const float* w = wf + d.wf;
    uint32_t p[8];
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int c0 = ks * 128 + 64 * half + 16 * h;
        const Mx8Scale s = mx8_scale(w, F, co, tap, c0 & ~31);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const float v = w[((size_t)co * F + c0 + q * 4 + b) * 9 + tap];
                const uint32_t code = s.finite ? (uint32_t)(e4m3_code_dev(ldexp(fabs((double)v), -s.se)) |
                                                            (__float_as_uint(v) >> 31 ? 0x80 : 0))
                                               : 0x7Fu;
                word |= code << (8 * b);
            }
            p[half * 4 + q] = word;
        }
    }
    uint4* o = reinterpret_cast<uint4*>(w8 + ((size_t)conv * nfr + fr) * 32);
    o[0] = make_uint4(p[0], p[1], p[2], p[3]);
    o[1] = make_uint4(p[4], p[5], p[6], p[7]);
    const Mx8Scale s = mx8_scale(w, F, co, tap, (ks * 4 + h) * 32);
    w8s[(size_t)conv * nfr + fr] = s.finite ? (uint8_t)(s.se + 127) : (uint8_t)0xFF;
}

// ------------------------------------------------------------------ heads
// the folded 1x1 F -> 40 conv (net.hip fold1x1): rows 0-31 policy_conv_1, 32-39 value_conv
__device__ __forceinline__ float w40_at(const float* __restrict__ wts, const HeadOff& ho, const double* __restrict__ hsc,
                                        int F, int co, int ci) {
    if (co >= 40) return 0.0f;
    const float w = co < 32 ? wts[ho.p1w + (size_t)co * F + ci] : wts[ho.vw + (size_t)(co - 32) * F + ci];
    return (float)(w * hsc[co]);
}

__device__ float head_elem(const float* __restrict__ wts, const HeadOff& ho, const double* __restrict__ hsc, int F,
                           const HeadLayout& L, size_t i) {
    if (i < L.b40) return w40_at(wts, ho, hsc, F, (int)(i / F), (int)(i % F));
    if (i < L.p2w) {
        const int ch = (int)(i - L.b40);
        const bool pol = ch < 32;
        const int cout = pol ? 32 : 8, co = pol ? ch : ch - 32;
        const float* bn = wts + (pol ? ho.pbn : ho.vbn);
        const float b = wts[(pol ? ho.p1b : ho.vb) + co];
        return (float)(((double)b - bn[2 * cout + co]) * hsc[ch] + bn[cout + co]);
    }
    if (i < L.p2b) return wts[ho.p2w + (i - L.p2w)];
    if (i < L.l1w) return wts[ho.p2b + (i - L.p2b)];
    if (i < L.l1b) return wts[ho.l1w + (i - L.l1w)];
    if (i < L.l2w) return wts[ho.l1b + (i - L.l1b)];
    if (i < L.l2b) return wts[ho.l2w + (i - L.l2w)];
    if (i < L.p2f) return i == L.l2b ? wts[ho.l2b] : 0.0f;
    const int k = (int)(i - L.p2f), ks = k & 7, lane = (k >> 3) & 63, cf = k >> 9;
    return wts[ho.p2w + (cf * 16 + (lane & 15)) * 32 + (lane >> 4) + ks * 4];
}

// units: L.total / 4 float4 of head, then (F/32) 3 2 64 pieces of head_frag (bf16 hi / lo of the folded
// weight), then (F/16) 3 64 pieces of head_frag32
__global__ void __launch_bounds__(256)
k_pack_heads(const float* __restrict__ wts, HeadOff ho, const double* __restrict__ hsc, int F,
             float4* __restrict__ head, uint4* __restrict__ frag, float4* __restrict__ frag32) {
    const HeadLayout L = HeadLayout::make(F);
    const int nh = (int)(L.total / 4), nf = (F / 32) * 3 * 2 * 64, nf32 = (F / 16) * 3 * 64;
    int u = blockIdx.x * 256 + threadIdx.x;
    if (u < nh) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = head_elem(wts, ho, hsc, F, L, (size_t)u * 4 + j);
        head[u] = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    u -= nh;
    if (u < nf) {
        const int lane = u & 63, hl = (u >> 6) & 1, cf = (u >> 7) % 3, ks = (u >> 7) / 3;
        const int co = cf * 16 + (lane & 15), c0 = ks * 32 + 8 * (lane >> 4);
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float v = w40_at(wts, ho, hsc, F, co, c0 + j);
            const uint16_t hi = bf16_rne_dev(v);
            const float hf = __uint_as_float((uint32_t)hi << 16);
            const uint32_t o = hl ? bf16_rne_dev(v - hf) : hi;
            if (j & 1) p[j >> 1] |= o << 16; else p[j >> 1] = o;
        }
        frag[u] = make_uint4(p[0], p[1], p[2], p[3]);
        return;
    }
    u -= nf;
    if (u < nf32) {
        const int lane = u & 63, cf = (u >> 6) % 3, kc = (u >> 6) / 3;
        const int co = cf * 16 + (lane & 15), c0 = kc * 16 + 4 * (lane >> 4);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = w40_at(wts, ho, hsc, F, co, c0 + j);
        frag32[u] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

inline unsigned cdiv(size_t a, unsigned b) { return (unsigned)((a + b - 1) / b); }

// the sizes net_create allocated, from the layouts' definitions: the kernels write exactly these
int check_sizes(const NetDev* n) {
    const int B = n->blocks, F = n->filters, nconv = 1 + 2 * B, CF = F / 16;
    const bool f32 = n->dtype == AZ_DTYPE_F32, fp8 = n->dtype == AZ_DTYPE_FP8;
    const size_t ndirect = fp8 ? 1 : (size_t)nconv;
    if (n->conv_w.size() != ndirect || n->conv_b.size() != ndirect || n->conv_bytes.size() != ndirect)
        return fail("az_net_update: unexpected conv buffers");
    for (size_t i = 0; i < ndirect; i++) {
        const int CIN = i == 0 ? 32 : F;
        const size_t nk = 9 * (size_t)CIN / (f32 ? 16 : 32);
        if (n->conv_bytes[i] != (nk + 8) * CF * 64 * 16) return fail("az_net_update: unexpected conv buffer size");
    }
    if (n->in_pk32 && n->in_pk32_bytes != (size_t)20 * CF * 64 * 16) return fail("az_net_update: unexpected packed input conv size");
    if (!n->wino_w.empty()) {
        if ((int)n->wino_w.size() != 2 * B || n->wino_bytes.size() != n->wino_w.size()) return fail("az_net_update: unexpected Winograd buffers");
        for (size_t b : n->wino_bytes)
            if (b != (size_t)(F + 8) * CF * 64 * 16) return fail("az_net_update: unexpected Winograd buffer size");
    }
    if (!n->wino16_w.empty()) {
        if ((int)n->wino16_w.size() != 2 * B || n->wino16_bytes.size() != n->wino16_w.size() ||
            n->wino16_us.size() != n->wino16_w.size() || !n->wino_w.empty())
            return fail("az_net_update: unexpected split-f16 buffers");
        if (F < 64 || (n->wino_rows && (F != 256 || n->wino_streamed != 12)) || (n->wino_streamed != 12 && n->wino_streamed != 16))
            return fail("az_net_update: unexpected split-f16 form");
        const size_t steps = (size_t)(F / 32) * n->wino_streamed + (n->wino_rows ? WINO_ROWS_PF : 2);
        for (size_t b : n->wino16_bytes)
            if (b != steps * CF * 2 * 64 * 16) return fail("az_net_update: unexpected split-f16 buffer size");
    }
    if (fp8 && B > 0) {
        const size_t cb = (size_t)9 * (F / 128) * CF * 64 * 32;
        if (!n->w8 || !n->w8s || !n->b8 || n->w8_bytes != 2 * B * cb || n->w8s_bytes != 2 * B * cb / 32)
            return fail("az_net_update: unexpected MX-fp8 buffers");
    }
    if (!n->head || !n->head_frag || !n->head_frag32 || n->head_floats != HeadLayout::make(F).total)
        return fail("az_net_update: unexpected head buffers");
    return 0;
}

int ensure_scratch(NetDev* n) {
    if (n->upd) return 0;
    const int B = n->blocks, F = n->filters, nconv = 1 + 2 * B;
    const bool fp8 = n->dtype == AZ_DTYPE_FP8;
    NetUpdate* U = new NetUpdate();
    U->count = az_net_num_params(B, F);
    std::vector<ConvDesc> tab(nconv);
    unsigned long long p = 0, q = 0;
    for (int i = 0; i < nconv; i++) {
        const int cin = i == 0 ? 19 : F;
        ConvDesc& d = tab[i];
        memset(&d, 0, sizeof(d));
        d.cin = cin;
        d.w = p; d.b = p + (size_t)F * cin * 9; d.bn = d.b + F;
        p = d.bn + 4 * (size_t)F;
        d.wf = q;
        q += (size_t)F * cin * 9;
        const bool res8 = fp8 && i > 0;
        d.direct = res8 ? nullptr : n->conv_w[i];
        d.bias_out = res8 ? n->b8 + (size_t)(i - 1) * F : n->conv_b[i];
        if (i > 0 && !n->wino16_w.empty()) d.wino = n->wino16_w[i - 1];
        else if (i > 0 && !n->wino_w.empty()) d.wino = n->wino_w[i - 1];
    }
    HeadOff& h = U->ho;
    h.p1w = p; h.p1b = h.p1w + 32 * (size_t)F; h.pbn = h.p1b + 32; h.p2w = h.pbn + 128; h.p2b = h.p2w + 64 * 32;
    h.vw = h.p2b + 64; h.vb = h.vw + 8 * (size_t)F; h.vbn = h.vb + 8; h.l1w = h.vbn + 32; h.l1b = h.l1w + 512 * 64;
    h.l2w = h.l1b + 64; h.l2b = h.l2w + 64;
    bool ok = h.l2b + 1 == U->count;
    ok = ok && hipMalloc(&U->wts, U->count * 4) == hipSuccess;
    ok = ok && hipMalloc(&U->wf, q * 4) == hipSuccess;
    ok = ok && hipMalloc(&U->sc, ((size_t)nconv * F + 40) * 8) == hipSuccess;
    ok = ok && hipMalloc(&U->tab, nconv * sizeof(ConvDesc)) == hipSuccess;
    ok = ok && hipMalloc(&U->umax, (size_t)(2 * B + 1) * 8) == hipSuccess;
    ok = ok && hipMalloc(&U->us, (size_t)(2 * B + 1) * 4) == hipSuccess;
    ok = ok && hipMemcpy(U->tab, tab.data(), nconv * sizeof(ConvDesc), hipMemcpyHostToDevice) == hipSuccess;
    n->upd = U;
    if (!ok) {
        net_update_free(n);
        return fail("az_net_update: scratch allocation failed");
    }
    return 0;
}

}  // namespace

void net_update_free(NetDev* n) {
    NetUpdate* U = n->upd;
    if (!U) return;
    (void)hipFree(U->wts); (void)hipFree(U->wf); (void)hipFree(U->sc); (void)hipFree(U->tab);
    (void)hipFree(U->umax); (void)hipFree(U->us);
    delete U;
    n->upd = nullptr;
}

int net_update_device(NetDev* n, const float* d_w, size_t count, hipStream_t st) {
    const int B = n->blocks, F = n->filters, nconv = 1 + 2 * B, CF = F / 16;
    if (!d_w) return fail("az_net_update: null weights");
    if (count != az_net_num_params(B, F)) return fail("az_net_update: weight count mismatch");
    AZ_HIP(hipSetDevice(n->device));
    if (check_sizes(n)) return -1;
    if (ensure_scratch(n)) return -1;
    NetUpdate* U = n->upd;
    if (!st) st = n->stream;
    const bool f32 = n->dtype == AZ_DTYPE_F32, fp8 = n->dtype == AZ_DTYPE_FP8;
    if (d_w != U->wts) AZ_HIP(hipMemcpyAsync(U->wts, d_w, count * 4, hipMemcpyDeviceToDevice, st));
    k_scales<<<cdiv((size_t)nconv * F + 40, 256), 256, 0, st>>>(U->wts, U->tab, nconv, F, U->ho, U->sc);
    k_fold<<<dim3(cdiv((size_t)F * F * 9, 256), nconv), 256, 0, st>>>(U->wts, U->tab, U->sc, F, U->wf);
    {   // conv_w: every conv of an f32 / bf16 net, the bf16 input conv of an fp8 net
        const size_t units = (size_t)(9 * F / (f32 ? 16 : 32) + 8) * CF * 64;   // the residual convs' (>= the input conv's)
        const dim3 grid(cdiv(units, 256), fp8 ? 1 : nconv);
        if (f32) k_pack_direct<false><<<grid, 256, 0, st>>>(U->wf, U->tab, F);
        else k_pack_direct<true><<<grid, 256, 0, st>>>(U->wf, U->tab, F);
    }
    if (n->in_pk32)
        k_pack_in32<<<cdiv((size_t)20 * CF * 64, 256), 256, 0, st>>>(U->wf, U->tab, F, reinterpret_cast<float4*>(n->in_pk32));
    if (B > 0 && !n->wino_w.empty())
        k_pack_wino32<<<dim3(cdiv((size_t)(F / 16 + 1) * CF * 64, 256), 2 * B), 256, 0, st>>>(U->wf, U->tab, F);
    const bool h16 = B > 0 && !n->wino16_w.empty();
    if (h16) {
        AZ_HIP(hipMemsetAsync(U->umax, 0, (size_t)2 * B * 8, st));
        const dim3 gm(cdiv((size_t)F * F, 256), 2 * B), gp(cdiv((size_t)(F / 32 + 1) * CF * 64, 256), 2 * B);
        if (n->wino_rows) {
            k_wino_max<true><<<gm, 256, 0, st>>>(U->wf, U->tab, F, U->umax);
            k_pack_wino16<2><<<gp, 256, 0, st>>>(U->wf, U->tab, F, U->umax, U->us);
        } else {
            k_wino_max<false><<<gm, 256, 0, st>>>(U->wf, U->tab, F, U->umax);
            if (n->wino_streamed == 12) k_pack_wino16<1><<<gp, 256, 0, st>>>(U->wf, U->tab, F, U->umax, U->us);
            else k_pack_wino16<0><<<gp, 256, 0, st>>>(U->wf, U->tab, F, U->umax, U->us);
        }
    }
    if (fp8 && B > 0)
        k_pack_mx8<<<dim3(cdiv((size_t)9 * (F / 128) * CF * 64, 256), 2 * B), 256, 0, st>>>(
            U->wf, U->tab, F, reinterpret_cast<uint8_t*>(n->w8), reinterpret_cast<uint8_t*>(n->w8s));
    {
        const HeadLayout L = HeadLayout::make(F);
        const size_t units = L.total / 4 + (size_t)(F / 32) * 3 * 2 * 64 + (size_t)(F / 16) * 3 * 64;
        k_pack_heads<<<cdiv(units, 256), 256, 0, st>>>(U->wts, U->ho, U->sc + (size_t)nconv * F, F,
                                                      reinterpret_cast<float4*>(n->head), reinterpret_cast<uint4*>(n->head_frag),
                                                      reinterpret_cast<float4*>(n->head_frag32));
    }
    AZ_HIP(hipGetLastError());
    // the tower reads each conv's 1 / (Sa Sw) from NetDev on the host: the only values that come back
    std::vector<float> us(h16 ? 2 * B : 0);
    if (h16) AZ_HIP(hipMemcpyAsync(us.data(), U->us, us.size() * 4, hipMemcpyDeviceToHost, st));
    AZ_HIP(hipStreamSynchronize(st));
    if (h16) n->wino16_us = us;
    n->generation++;
    return 0;
}

}  // namespace azi

using namespace azi;

extern "C" {

int az_net_update_device(az_net* net, const float* d_weights, size_t n, void* stream) {
    if (!net || !d_weights) return fail("az_net_update_device: null argument");
    return net_update_device(net->dev, d_weights, n, (hipStream_t)stream);
}

int az_net_update(az_net* net, const float* weights, size_t n) {
    if (!net || !weights) return fail("az_net_update: null argument");
    NetDev* d = net->dev;
    if (n != az_net_num_params(d->blocks, d->filters)) return fail("az_net_update: weight count mismatch");
    AZ_HIP(hipSetDevice(d->device));
    if (check_sizes(d) || ensure_scratch(d)) return -1;
    AZ_HIP(hipMemcpyAsync(d->upd->wts, weights, n * 4, hipMemcpyHostToDevice, d->stream));
    return net_update_device(d, d->upd->wts, n, d->stream);
}

int64_t az_net_generation(az_net* net) {
    if (!net) return fail("az_net_generation: null net");
    return net->dev->generation;
}

int az_net_get_weights(az_net* net, float* out, size_t n) {
    if (!net || !out) return fail("az_net_get_weights: null argument");
    NetDev* d = net->dev;
    if (d->generation == 0 || !d->upd) return fail("az_net_get_weights: the net was never updated (its creator holds the weights)");
    if (n != d->upd->count) return fail("az_net_get_weights: weight count mismatch");
    AZ_HIP(hipSetDevice(d->device));
    AZ_HIP(hipMemcpy(out, d->upd->wts, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int az_net_packed_read(az_net* net, int kind, int index, void* out, size_t cap) {
    if (!net) return fail("az_net_packed_read: null net");
    if (kind < 0 || kind >= AZ_PACKED_KINDS || index < 0) return fail("az_net_packed_read: bad kind or index");
    NetDev* d = net->dev;
    const size_t F = d->filters, i = (size_t)index;
    const void* src = nullptr;
    size_t bytes = 0;
    bool host = false;
    auto one = [&](const void* p, size_t b) { if (i == 0 && p) { src = p; bytes = b; } };
    switch (kind) {
    case AZ_PACKED_CONV_W: if (i < d->conv_w.size()) { src = d->conv_w[i]; bytes = d->conv_bytes[i]; } break;
    case AZ_PACKED_CONV_B: if (i < d->conv_b.size()) { src = d->conv_b[i]; bytes = F * 4; } break;
    case AZ_PACKED_IN_PK32: one(d->in_pk32, d->in_pk32_bytes); break;
    case AZ_PACKED_WINO_W: if (i < d->wino_w.size()) { src = d->wino_w[i]; bytes = d->wino_bytes[i]; } break;
    case AZ_PACKED_WINO16_W: if (i < d->wino16_w.size()) { src = d->wino16_w[i]; bytes = d->wino16_bytes[i]; } break;
    case AZ_PACKED_WINO16_US: if (i < d->wino16_us.size()) { src = &d->wino16_us[i]; bytes = 4; host = true; } break;
    case AZ_PACKED_W8: one(d->w8, d->w8_bytes); break;
    case AZ_PACKED_W8S: one(d->w8s, d->w8s_bytes); break;
    case AZ_PACKED_B8: one(d->b8, (size_t)2 * d->blocks * F * 4); break;
    case AZ_PACKED_HEAD: one(d->head, d->head_floats * 4); break;
    case AZ_PACKED_HEAD_FRAG: one(d->head_frag, (F / 32) * 3 * 2 * 64 * 8 * 2); break;
    case AZ_PACKED_HEAD_FRAG32: one(d->head_frag32, (F / 16) * 3 * 64 * 4 * 4); break;
    }
    if (!src || bytes == 0) return 0;
    if (bytes > 0x7fffffffu) return fail("az_net_packed_read: buffer too large");
    if (!out) return (int)bytes;
    if (cap < bytes) return fail("az_net_packed_read: output too small");
    if (host) { memcpy(out, src, bytes); return (int)bytes; }
    AZ_HIP(hipSetDevice(d->device));
    AZ_HIP(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
    return (int)bytes;
}

}  // extern "C"
