// noise_probe.hip -- the search's random streams and their float math, one op at a time (az_noise_probe).
//
// The engine reaches det_logf / det_expf / uniform01 / open01 / std_normal / gamma_sample (detmath.h) only
// through the root noise of a search, that is only at the arguments a handful of dir_alpha values produce.
// This entry runs exactly those functions -- and dirichlet_row_block, the row k_root_noise draws -- on
// caller-given arguments, on the device or (AZ_DEVICE_HOST) as the host compiles them, so tests can hold
// them to the oracle and to float64 over the whole domain: subnormals, the branch thresholds, +-0, +-inf,
// NaN.  It is a test hook: the engine itself never calls it.
#include <math.h>

#include <vector>

#include "az_internal.h"
#include "detmath.h"

namespace azi {

AZ_HD void noise_item(int op, size_t i, int m, const float* x, const uint64_t* key, float* out) {
    uint64_t ctr = 0;
    switch (op) {
    case AZ_NOISE_LOGF: out[i] = azc::det_logf(x[i]); break;
    case AZ_NOISE_EXPF: out[i] = azc::det_expf(x[i]); break;
    case AZ_NOISE_UNIFORM01:
        for (int j = 0; j < m; j++) out[i * m + j] = azc::uniform01(key[i], ctr);
        break;
    case AZ_NOISE_OPEN01:
        for (int j = 0; j < m; j++) out[i * m + j] = azc::open01(key[i], ctr);
        break;
    case AZ_NOISE_NORMAL: out[i] = azc::std_normal(key[i], ctr); break;
    case AZ_NOISE_GAMMA: out[i] = azc::gamma_sample(x[i], key[i]); break;
    }
}

// one thread per item
__global__ void __launch_bounds__(256) k_noise_probe(int op, int n, int m, const float* __restrict__ x,
                                                     const uint64_t* __restrict__ key, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    noise_item(op, i, m, x, key, out);
}

// one 64-thread block per row, as one game's root noise in k_root_noise
__global__ void __launch_bounds__(64) k_noise_probe_rows(int n, int m, const float* __restrict__ alpha,
                                                         const uint64_t* __restrict__ key, float* __restrict__ out,
                                                         int* __restrict__ fallback) {
    __shared__ float row[AZ_MAX_MOVES];
    __shared__ float sh[2];
    const int i = vgpr_index(blockIdx.x), lane = threadIdx.x;
    if (i >= n) return;
    const int fb = azc::dirichlet_row_block(alpha[i], m, key[i], row, sh);
    for (int k = lane; k < m; k += 64) out[(size_t)i * m + k] = row[k];
    if (lane == 0) fallback[i] = fb;
}

}  // namespace azi

using namespace azi;

extern "C" int az_noise_probe(int device, int op, int n, int m, const float* x, const uint64_t* key, float* out,
                              int32_t* fallback) {
    if (device < AZ_DEVICE_HOST) return fail("az_noise_probe: bad device");
    if (op < AZ_NOISE_LOGF || op > AZ_NOISE_DIRICHLET) return fail("az_noise_probe: unknown op");
    if (n < 0 || (n > 0 && !out)) return fail("az_noise_probe: null argument");
    const bool rows = op == AZ_NOISE_DIRICHLET;
    const bool per_draw = op == AZ_NOISE_UNIFORM01 || op == AZ_NOISE_OPEN01;
    const bool need_x = op == AZ_NOISE_LOGF || op == AZ_NOISE_EXPF || op == AZ_NOISE_GAMMA || rows;
    const bool need_key = op != AZ_NOISE_LOGF && op != AZ_NOISE_EXPF;
    if (n > 0 && ((need_x && !x) || (need_key && !key))) return fail("az_noise_probe: null argument");
    if (rows && (m < 1 || m > AZ_MAX_MOVES)) return fail("az_noise_probe: a row has 1..AZ_MAX_MOVES components");
    if (per_draw && (m < 1 || m > 4096)) return fail("az_noise_probe: 1..4096 draws per key");
    if (!rows && !per_draw) m = 1;
    if ((int64_t)n * m > ((int64_t)1 << 28)) return fail("az_noise_probe: more than 2^28 outputs");
    if (op == AZ_NOISE_GAMMA || rows)   // the samplers loop on anything else
        for (int i = 0; i < n; i++)
            if (!(x[i] > 0.0f && x[i] <= 1e6f))
                return fail("az_noise_probe: item " + std::to_string(i) + ": shape must be in (0, 1e6]");
    if (n == 0) return 0;
    const size_t N = (size_t)n, NO = N * (size_t)m;

    if (device == AZ_DEVICE_HOST) {
        if (!rows) {
            for (size_t i = 0; i < N; i++) noise_item(op, i, m, x, key, out);
            return 0;
        }
        for (size_t i = 0; i < N; i++) {
            const int fb = azc::dirichlet_row_serial(x[i], m, key[i], out + i * m);
            if (fallback) fallback[i] = fb;
        }
        return 0;
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
    float* d_x = need_x ? (float*)dmal(N * 4) : nullptr;
    uint64_t* d_key = need_key ? (uint64_t*)dmal(N * 8) : nullptr;
    float* d_out = (float*)dmal(NO * 4);
    int* d_fb = rows ? (int*)dmal(N * 4) : nullptr;
    int rc = oom ? fail("az_noise_probe: hipMalloc failed") : 0;
    if (!rc) {
        auto run = [&]() -> int {
            if (need_x) AZ_HIP(hipMemcpyAsync(d_x, x, N * 4, hipMemcpyHostToDevice, st));
            if (need_key) AZ_HIP(hipMemcpyAsync(d_key, key, N * 8, hipMemcpyHostToDevice, st));
            if (rows) k_noise_probe_rows<<<n, 64, 0, st>>>(n, m, d_x, d_key, d_out, d_fb);
            else k_noise_probe<<<(unsigned)((N + 255) / 256), 256, 0, st>>>(op, n, m, d_x, d_key, d_out);
            AZ_HIP(hipGetLastError());
            AZ_HIP(hipMemcpyAsync(out, d_out, NO * 4, hipMemcpyDeviceToHost, st));
            if (rows && fallback) AZ_HIP(hipMemcpyAsync(fallback, d_fb, N * 4, hipMemcpyDeviceToHost, st));
            AZ_HIP(hipStreamSynchronize(st));
            return 0;
        };
        rc = run();
    }
    (void)hipStreamSynchronize(st);
    for (void* p : bufs) (void)hipFree(p);
    (void)hipStreamDestroy(st);
    return rc;
}
