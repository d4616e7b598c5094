// mx8_lane_map -- the operand and scale lane maps of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3
// operands on gfx950, established with exact integer data on one wave, and what v_cvt_pk_fp8_f32
// does at the edges (saturation, ties, subnormals).  csrc/tower8.hip is written against what this
// prints.
//   hipcc --offload-arch=gfx950 -O2 -o mx8_lane_map mx8_lane_map.hip && ./mx8_lane_map
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CK(e)                                                                  \
    do {                                                                       \
        hipError_t r_ = (e);                                                   \
        if (r_ != hipSuccess) {                                                \
            printf("%s: %s\n", #e, hipGetErrorString(r_));                     \
            return 1;                                                          \
        }                                                                      \
    } while (0)

// e4m3fn code of a small non-negative integer (exact for 0..16)
static __host__ __device__ unsigned code_of(int v) {
    if (v == 0) return 0;
    int e = 0;
    while ((v >> (e + 1)) != 0) e++;
    return (unsigned)(((e + 7) << 3) | (((v << 3) >> e) & 7));
}

__device__ f32x4 mfma(i32x8 a, i32x8 b, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, f32x4{0, 0, 0, 0}, 0, 0, 0, sa, 0, sb);
}

__device__ i32x8 fill(unsigned byte) {
    const int w = (int)(byte * 0x01010101u);
    return i32x8{w, w, w, w, w, w, w, w};
}

// operand map: A = one-hot 1.0 at (lane L, byte j); B element (lane L', byte j') = a small integer
// that names, per pass, j' % 8, j' / 8 or L' / 16.  out[(L*32 + j)*3 + pass][lane][4]
__global__ void k_operands(float* out) {
    const int lane = threadIdx.x;
    for (int L = 0; L < 64; L++)
        for (int j = 0; j < 32; j++) {
            i32x8 a = fill(0);
            if (lane == L) a[j >> 2] = (int)(0x38u << (8 * (j & 3)));
            for (int pass = 0; pass < 3; pass++) {
                i32x8 b;
                for (int q = 0; q < 8; q++) {
                    unsigned w = 0;
                    for (int t = 0; t < 4; t++) {
                        const int jj = q * 4 + t;
                        const int v = pass == 0 ? (jj & 7) + 1 : pass == 1 ? (jj >> 3) + 1 : (lane >> 4) + 1;
                        w |= code_of(v) << (8 * t);
                    }
                    b[q] = (int)w;
                }
                const f32x4 d = mfma(a, b, 127, 127);
                float* o = out + ((size_t)((L * 32 + j) * 3 + pass) * 64 + lane) * 4;
                for (int r = 0; r < 4; r++) o[r] = d[r];
            }
        }
}

// scale map: all elements 1.0; the side NOT under test is non-zero only in one 16-byte chunk (lane
// group t, byte half hf); the side under test has scale 2 in lane L only.
// out[((side*64 + L)*8 + t*2 + hf)][lane][4]
__global__ void k_scales(float* out) {
    const int lane = threadIdx.x;
    for (int side = 0; side < 2; side++)
        for (int L = 0; L < 64; L++)
            for (int ch = 0; ch < 8; ch++) {
                const i32x8 ones = fill(0x38);
                i32x8 part = fill(0);
                if ((lane >> 4) == (ch >> 1))
                    for (int q = 0; q < 4; q++) part[(ch & 1) * 4 + q] = 0x38383838;
                const int s = lane == L ? 128 : 127;
                const f32x4 d = side == 0 ? mfma(ones, part, s, 127) : mfma(part, ones, 127, s);
                float* o = out + ((size_t)((side * 64 + L) * 8 + ch) * 64 + lane) * 4;
                for (int r = 0; r < 4; r++) o[r] = d[r];
            }
}

// op_sel: the scale register holds bytes 127, 128, 129, 130 (2^0 .. 2^3); which byte does op_sel pick?
// out[(side*4 + sel)][lane][4] with all elements 1.0 (unscaled sum = 128)
template <int SEL> __device__ f32x4 sel_a(i32x8 a, i32x8 b, int s) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, f32x4{0, 0, 0, 0}, 0, 0, SEL, s, 0, 127);
}
template <int SEL> __device__ f32x4 sel_b(i32x8 a, i32x8 b, int s) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, f32x4{0, 0, 0, 0}, 0, 0, 0, 127, SEL, s);
}
__global__ void k_opsel(float* out, float* nan_out) {
    const int lane = threadIdx.x;
    const i32x8 ones = fill(0x38);
    const int s = 127 | (128 << 8) | (129 << 16) | (130 << 24);
    f32x4 d[8] = {sel_a<0>(ones, ones, s), sel_a<1>(ones, ones, s), sel_a<2>(ones, ones, s), sel_a<3>(ones, ones, s),
                  sel_b<0>(ones, ones, s), sel_b<1>(ones, ones, s), sel_b<2>(ones, ones, s), sel_b<3>(ones, ones, s)};
    for (int i = 0; i < 8; i++)
        for (int r = 0; r < 4; r++) out[((size_t)i * 64 + lane) * 4 + r] = d[i][r];
    // a NaN scale byte (0xFF) in lane 5 of A, a NaN element (0x7F) in lane 9 of B; high scale bytes garbage
    const f32x4 n0 = mfma(ones, ones, lane == 5 ? 0xFF : 127, 127);
    i32x8 bn = ones;
    if (lane == 9) bn[0] = 0x3838387F;
    const f32x4 n1 = mfma(ones, bn, 127, 127);
    const f32x4 n2 = mfma(ones, ones, (int)0xABCDEF00u | 127, (int)0x12345600u | 127);
    for (int r = 0; r < 4; r++) {
        nan_out[lane * 4 + r] = n0[r];
        nan_out[256 + lane * 4 + r] = n1[r];
        nan_out[512 + lane * 4 + r] = n2[r];
    }
}

__global__ void k_cvt(const float* in, int n, unsigned* out) {
    const int i = threadIdx.x;
    if (i < n) out[i] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(in[i], 0.0f, 0, false) & 0xFFFFu;
}

int main() {
    float* d = nullptr;
    const size_t n_op = (size_t)64 * 32 * 3 * 256, n_sc = (size_t)2 * 64 * 8 * 256;
    CK(hipMalloc(&d, (n_op + n_sc + 8 * 256 + 768) * 4));
    CK(hipMemset(d, 0, (n_op + n_sc + 8 * 256 + 768) * 4));
    k_operands<<<1, 64>>>(d);
    k_scales<<<1, 64>>>(d + n_op);
    k_opsel<<<1, 64>>>(d + n_op + n_sc, d + n_op + n_sc + 8 * 256);
    CK(hipDeviceSynchronize());
    std::vector<float> h(n_op + n_sc + 8 * 256 + 768);
    CK(hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost));

    // D is read as: lane l register r = row 4 (l / 16) + r, column l % 16 (the layout of every 16x16 MFMA)
    auto D = [&](const float* base, int row, int col) { return base[((row >> 2) * 16 + col) * 4 + (row & 3)]; };
    // operands.  Hypothesis: A (lane L, byte j) is row L % 16; it meets B (lane 16 (L / 16) + col, byte j)
    int bad = 0, shown = 0;
    for (int L = 0; L < 64; L++)
        for (int j = 0; j < 32; j++) {
            const float* p0 = &h[(size_t)((L * 32 + j) * 3 + 0) * 256];
            const float *p1 = p0 + 256, *p2 = p1 + 256;
            int rows = 0, row = -1;
            for (int r = 0; r < 16; r++) {
                bool nz = false;
                for (int c = 0; c < 16; c++) nz = nz || D(p0, r, c) != 0.0f;
                if (nz) { rows++; row = r; }
            }
            bool ok = rows == 1 && row == (L & 15);
            int jb = -1, hb = -1;
            if (rows == 1) {
                for (int c = 0; c < 16; c++) {
                    const int jj = ((int)D(p0, row, c) - 1) + 8 * ((int)D(p1, row, c) - 1), hh = (int)D(p2, row, c) - 1;
                    if (c == 0) { jb = jj; hb = hh; }
                    ok = ok && jj == j && hh == (L >> 4);
                }
            }
            if (!ok) {
                bad++;
                if (shown++ < 16) printf("operand map differs: A lane %d byte %d -> rows %d row %d, B byte %d lane group %d\n", L, j, rows, row, jb, hb);
            }
        }
    printf("operands: A(lane L, byte j) is row L%%16 and meets B(lane 16 (L/16) + column, byte j): %s (%d of 2048 differ)\n",
           bad ? "NO" : "yes", bad);
    // scales.  Hypothesis: the scale in lane L applies to row (column) L % 16 and to the K block L / 16, where the
    // 16-byte chunk (lane group t, byte half hf) holds K = 64 hf + 16 t + 0..15, so block g = chunks (2 (g & 1), g >> 1)
    // and (2 (g & 1) + 1, g >> 1)
    for (int side = 0; side < 2; side++) {
        int sbad = 0, sshown = 0;
        for (int L = 0; L < 64; L++)
            for (int ch = 0; ch < 8; ch++) {
                const float* p = &h[n_op + (size_t)((side * 64 + L) * 8 + ch) * 256];
                const int t = ch >> 1, hf = ch & 1, kblock = (64 * hf + 16 * t) / 32;
                for (int r = 0; r < 16; r++)
                    for (int c = 0; c < 16; c++) {
                        const int idx = side == 0 ? r : c;
                        const float want = (idx == (L & 15) && kblock == (L >> 4)) ? 32.0f : 16.0f;
                        if (D(p, r, c) != want) {
                            sbad++;
                            if (sshown++ < 16) printf("scale_%c lane %d chunk (group %d, half %d): D[%d][%d] = %g, expected %g\n", side ? 'b' : 'a', L, t, hf, r, c, D(p, r, c), want);
                        }
                    }
            }
        printf("scale_%c: lane L scales %s L%%16, K block L/16 with K(lane group t, byte j) = 64 (j / 16) + 16 t + j %% 16: %s (%d mismatches)\n",
               side ? 'b' : 'a', side ? "column" : "row", sbad ? "NO" : "yes", sbad);
    }
    const float* po = &h[n_op + n_sc];
    for (int i = 0; i < 8; i++) printf("op_sel_%c = %d: D[0][0] = %g (128 x 2^byte index)\n", i < 4 ? 'a' : 'b', i & 3, po[(size_t)i * 256]);
    const float* pn = po + 8 * 256;
    int nan_rows = 0, nan_cols = 0, g_bad = 0;
    for (int r = 0; r < 16; r++) nan_rows += isnan(D(pn, r, 0)) ? 1 : 0;
    for (int c = 0; c < 16; c++) nan_cols += isnan(D(pn + 256, 0, c)) ? 1 : 0;
    for (int i = 0; i < 256; i++) g_bad += pn[512 + i] != 128.0f;
    printf("NaN scale byte in A lane 5: %d NaN rows (row 5 NaN: %d); NaN element in B lane 9: %d NaN columns (column 9: %d)\n",
           nan_rows, (int)isnan(D(pn, 5, 0)), nan_cols, (int)isnan(D(pn + 256, 0, 9)));
    printf("op_sel 0 with garbage in the upper scale bytes: %d of 256 outputs differ from 128\n", g_bad);

    const float cv[] = {448.0f, 464.0f, 465.0f, 480.0f, 500.0f, 511.0f, 1e6f, INFINITY, NAN, -500.0f, 17.0f, 19.0f, 18.0f,
                        0.001953125f, 0.0009765625f, 0.0029296875f, 0.0048828125f, 0.015625f, -0.0f, 0.0f, 1.0f, 256.0f, 272.0f, 304.0f};
    const int nc = sizeof(cv) / 4;
    float* dc;
    unsigned* du;
    CK(hipMalloc(&dc, nc * 4));
    CK(hipMalloc(&du, nc * 4));
    CK(hipMemcpy(dc, cv, nc * 4, hipMemcpyHostToDevice));
    k_cvt<<<1, 64>>>(dc, nc, du);
    unsigned hu[64];
    CK(hipMemcpy(hu, du, nc * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < nc; i++) printf("v_cvt_pk_fp8_f32(%.10g) = 0x%02x\n", cv[i], hu[i] & 0xFF);
    return 0;
}
