// replay_dev.hip -- the device-backed ReplayBuffer (az_replay_create_on): the payload rows in HBM.
//
// The host (replay.hip) keeps what decides the buffer's behaviour -- the FEN keys, the FIFO, the visit
// counts and the key -> slot map -- and every entry's payload lives in one of `slots` rows of three
// arrays: policy [slots][4096] f32, value [slots] f32 and the az_pos rebuilt from the key [slots]
// (16,468 B per slot).  Two kernels touch the rows:
//   k_replay_add     one workgroup per distinct slot of a launch applies that slot's steps in call order:
//                    the dense improved policy from the compact (index, visits) pairs -- last entry wins
//                    on a duplicate index, as the host's serial scatter -- then assign or running mean, in
//                    az_replay_add's operand order (IEEE division, no contraction): bit for bit the host.
//   k_replay_gather  one workgroup per output row: to_tensor planes through plane_value from the stored
//                    position, the policy row as 16-byte copies, the value, to arbitrary device pointers.
// Both are streaming kernels (a row is 16 KB); every slot and index is validated on the host.
#include <string.h>

#include <algorithm>
#include <cstdlib>

#include "replay_int.h"

namespace azi {

namespace {

constexpr int ROW = AZ_ACTION_SPACE;            // floats per policy row
constexpr int PLANE_FLOATS = AZ_PLANES * 64;
constexpr int ADD_THREADS = 256;                // >= MAX_EDGES: one lane per (index, visits) pair
constexpr int ADD_CHUNK_DEFAULT = 256, ADD_CHUNK_MAX = 8192;
static_assert(MAX_EDGES <= ADD_THREADS && ROW % (4 * ADD_THREADS) == 0, "k_replay_add's lane mapping");

struct AddRec {            // one step of a launch, 32 B
    int32_t slot;
    int32_t merge;         // 0: new entry (assign), 1: running mean
    float old_count;       // (float)visit_count before the step
    float value;
    int32_t nvis;
    int32_t pair_off;      // first of the step's nvis pairs (index | visits << 16)
    int32_t pos_idx;       // new entry: its position among the launch's positions
    int32_t dense;         // 1: the policy is the launch's dense row (az_replay_add_dense)
};

__global__ __launch_bounds__(ADD_THREADS) void k_replay_add(const AddRec* __restrict__ recs,
                                                            const uint32_t* __restrict__ pairs,
                                                            const azc::Pos* __restrict__ newpos,
                                                            const float* __restrict__ dense, const int* __restrict__ grp_off,
                                                            const int* __restrict__ grp_steps, float* pol, float* val,
                                                            azc::Pos* pos) {
    __shared__ int ord[ROW];            // per move index: the largest ordinal of a pair that names it, or -1
    __shared__ float cnt[ADD_THREADS];  // (float)visits per pair
    const int t = threadIdx.x;
    // the staging buffers are rewritten between launches: vector loads (az_internal.h, load_fresh)
    const int g = vgpr_index(blockIdx.x);
    const int k0 = grp_off[g], k1 = grp_off[g + 1];
    for (int k = k0; k < k1; k++) {
        const AddRec rc = recs[vgpr_index(grp_steps[vgpr_index(k)])];
        const size_t slot = (size_t)vgpr_index(rc.slot);
        float sum = 0.0f;
        if (!rc.dense) {
            for (int i = t; i < ROW; i += ADD_THREADS) ord[i] = -1;
            uint32_t pr = 0;
            if (t < rc.nvis) {
                pr = pairs[rc.pair_off + t];
                cnt[t] = (float)(pr >> 16);
            }
            __syncthreads();
            if (t < rc.nvis) atomicMax(&ord[pr & 0xFFFFu], t);
            for (int i = 0; i < rc.nvis; i++) sum += cnt[i];   // az_replay_add's f32 sum, in index order
            __syncthreads();
        }
        const float old = rc.old_count, total = rc.old_count + 1.0f;
        float4* row = reinterpret_cast<float4*>(pol + slot * ROW);
        for (int q = t; q < ROW / 4; q += ADD_THREADS) {
            float4 p;
            if (rc.dense) {
                p = reinterpret_cast<const float4*>(dense)[q];
            } else {
                const int4 o = reinterpret_cast<const int4*>(ord)[q];
                p.x = o.x >= 0 ? cnt[o.x] / sum : 0.0f;
                p.y = o.y >= 0 ? cnt[o.y] / sum : 0.0f;
                p.z = o.z >= 0 ? cnt[o.z] / sum : 0.0f;
                p.w = o.w >= 0 ? cnt[o.w] / sum : 0.0f;
            }
            if (rc.merge) {
                const float4 e = row[q];
                p.x = (e.x * old + p.x) / total;
                p.y = (e.y * old + p.y) / total;
                p.z = (e.z * old + p.z) / total;
                p.w = (e.w * old + p.w) / total;
            }
            row[q] = p;
        }
        if (t == 0) val[slot] = rc.merge ? (val[slot] * old + rc.value) / total : rc.value;
        if (!rc.merge && t < (int)(sizeof(azc::Pos) / 4))
            reinterpret_cast<uint32_t*>(pos + slot)[t] = reinterpret_cast<const uint32_t*>(newpos + rc.pos_idx)[t];
        __syncthreads();   // ord and cnt are the next step's; a thread rewrites only elements it wrote itself
    }
}

__global__ __launch_bounds__(256) void k_replay_gather(const int* __restrict__ slots, const float* __restrict__ pol,
                                                       const float* __restrict__ val, const azc::Pos* __restrict__ pos,
                                                       float* o_planes, float* o_pol, float* o_val) {
    __shared__ azc::Pos sp;
    const int t = threadIdx.x;
    const size_t row = blockIdx.x;
    const size_t slot = (size_t)slots[vgpr_index((int)row)];   // rows other launches wrote: vector loads
    if (o_planes) {
        if (t < (int)(sizeof(azc::Pos) / 4))
            reinterpret_cast<uint32_t*>(&sp)[t] = reinterpret_cast<const uint32_t*>(pos + slot)[t];
        __syncthreads();
        for (int e = t; e < PLANE_FLOATS; e += 256) o_planes[row * PLANE_FLOATS + e] = azc::plane_value(sp, e >> 6, e & 63);
    }
    if (o_pol) {
        const float4* src = reinterpret_cast<const float4*>(pol + slot * ROW);
        float4* dst = reinterpret_cast<float4*>(o_pol + row * ROW);
        for (int q = t; q < ROW / 4; q += 256) dst[q] = src[q];
    }
    if (o_val && t == 0) o_val[row] = val[vgpr_index((int)slot)];
}

}  // namespace

struct ReplayDev {
    int device = 0, slots = 0;
    hipStream_t st = nullptr;
    float* pol = nullptr;
    float* val = nullptr;
    azc::Pos* pos = nullptr;
    // a gather queued on a caller's stream reads d_slots and the rows: the next call that rewrites
    // either waits for it first
    hipEvent_t ev_gather = nullptr;
    bool gather_pending = false;
    // add staging for cap_steps steps per launch: pinned host side, device side
    int cap_steps = 0;
    AddRec *h_recs = nullptr, *d_recs = nullptr;
    uint32_t *h_pairs = nullptr, *d_pairs = nullptr;
    azc::Pos *h_pos = nullptr, *d_pos = nullptr;
    int *h_grp = nullptr, *d_grp = nullptr;        // [cap + 1] group offsets, then [cap] step ordinals by group
    float *h_dense = nullptr, *d_dense = nullptr;  // [4096]
    int nrec = 0, npair = 0, npos = 0;
    std::vector<std::pair<int, int>> by_slot;      // flush scratch: (slot, step ordinal)
    // gather
    int* h_slots = nullptr;
    int* d_slots = nullptr;
    int slots_cap = 0;
    float* d_stage = nullptr;                      // az_replay_sample to host pointers: [rows] planes | policy | value
    size_t stage_rows = 0;
};

namespace {

int wait_gather(ReplayDev* d) {
    if (d->gather_pending) {
        AZ_HIP(hipEventSynchronize(d->ev_gather));
        d->gather_pending = false;
    }
    return 0;
}

void free_add_staging(ReplayDev* d) {
    (void)hipHostFree(d->h_recs); (void)hipHostFree(d->h_pairs); (void)hipHostFree(d->h_pos); (void)hipHostFree(d->h_grp);
    (void)hipFree(d->d_recs); (void)hipFree(d->d_pairs); (void)hipFree(d->d_pos); (void)hipFree(d->d_grp);
    d->h_recs = d->d_recs = nullptr; d->h_pairs = d->d_pairs = nullptr; d->h_pos = d->d_pos = nullptr;
    d->h_grp = d->d_grp = nullptr;
    d->cap_steps = 0;
}

int ensure_add_staging(ReplayDev* d, int steps) {
    if (steps <= d->cap_steps) return 0;
    free_add_staging(d);
    const size_t n = (size_t)steps;
    bool ok = hipHostMalloc((void**)&d->h_recs, n * sizeof(AddRec), 0) == hipSuccess &&
              hipHostMalloc((void**)&d->h_pairs, n * MAX_EDGES * sizeof(uint32_t), 0) == hipSuccess &&
              hipHostMalloc((void**)&d->h_pos, n * sizeof(azc::Pos), 0) == hipSuccess &&
              hipHostMalloc((void**)&d->h_grp, (2 * n + 1) * sizeof(int), 0) == hipSuccess &&
              hipMalloc((void**)&d->d_recs, n * sizeof(AddRec)) == hipSuccess &&
              hipMalloc((void**)&d->d_pairs, n * MAX_EDGES * sizeof(uint32_t)) == hipSuccess &&
              hipMalloc((void**)&d->d_pos, n * sizeof(azc::Pos)) == hipSuccess &&
              hipMalloc((void**)&d->d_grp, (2 * n + 1) * sizeof(int)) == hipSuccess;
    if (!ok) { free_add_staging(d); return fail("az_replay_add: out of memory for the add staging buffers"); }
    d->cap_steps = steps;
    return 0;
}

int ensure_slots(ReplayDev* d, int n) {
    if (n <= d->slots_cap) return 0;
    (void)hipHostFree(d->h_slots); (void)hipFree(d->d_slots);
    d->h_slots = d->d_slots = nullptr;
    d->slots_cap = 0;
    const int cap = std::max(n, 1024);
    if (hipHostMalloc((void**)&d->h_slots, (size_t)cap * sizeof(int), 0) != hipSuccess ||
        hipMalloc((void**)&d->d_slots, (size_t)cap * sizeof(int)) != hipSuccess)
        return fail("az_replay_sample: out of memory for the slot list");
    d->slots_cap = cap;
    return 0;
}

// the steps staged so far, in one launch; returns when the rows are written
int add_flush(ReplayDev* d) {
    const int n = d->nrec;
    if (n == 0) return 0;
    // groups = the distinct slots; each group's steps in call order
    d->by_slot.resize(n);
    for (int i = 0; i < n; i++) d->by_slot[i] = {d->h_recs[i].slot, i};
    std::sort(d->by_slot.begin(), d->by_slot.end());   // equal slots stay in call order (the pair's second key)
    int* off = d->h_grp;
    int* steps = d->h_grp + d->cap_steps + 1;
    int ng = 0;
    for (int i = 0; i < n; i++) {
        if (i == 0 || d->by_slot[i].first != d->by_slot[i - 1].first) off[ng++] = i;
        steps[i] = d->by_slot[i].second;
    }
    off[ng] = n;
    hipStream_t st = d->st;
    AZ_HIP(hipMemcpyAsync(d->d_recs, d->h_recs, (size_t)n * sizeof(AddRec), hipMemcpyHostToDevice, st));
    if (d->npair) AZ_HIP(hipMemcpyAsync(d->d_pairs, d->h_pairs, (size_t)d->npair * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (d->npos) AZ_HIP(hipMemcpyAsync(d->d_pos, d->h_pos, (size_t)d->npos * sizeof(azc::Pos), hipMemcpyHostToDevice, st));
    AZ_HIP(hipMemcpyAsync(d->d_grp, d->h_grp, (size_t)(ng + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    AZ_HIP(hipMemcpyAsync(d->d_grp + d->cap_steps + 1, d->h_grp + d->cap_steps + 1, (size_t)n * sizeof(int),
                          hipMemcpyHostToDevice, st));
    k_replay_add<<<ng, ADD_THREADS, 0, st>>>(d->d_recs, d->d_pairs, d->d_pos, d->d_dense, d->d_grp,
                                             d->d_grp + d->cap_steps + 1, d->pol, d->val, d->pos);
    AZ_HIP(hipGetLastError());
    d->nrec = d->npair = d->npos = 0;
    AZ_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

int replay_dev_device(const ReplayDev* d) { return d->device; }

void replay_dev_destroy(ReplayDev* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->gather_pending) (void)hipEventSynchronize(d->ev_gather);
    if (d->st) (void)hipStreamSynchronize(d->st);
    free_add_staging(d);
    (void)hipHostFree(d->h_dense); (void)hipFree(d->d_dense);
    (void)hipHostFree(d->h_slots); (void)hipFree(d->d_slots);
    (void)hipFree(d->d_stage);
    (void)hipFree(d->pol); (void)hipFree(d->val); (void)hipFree(d->pos);
    if (d->ev_gather) (void)hipEventDestroy(d->ev_gather);
    if (d->st) (void)hipStreamDestroy(d->st);
    delete d;
}

int replay_dev_create(int slots, int device, ReplayDev** out) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
    if (device < 0 || device >= count)
        return fail("az_replay_create_on: device " + std::to_string(device) + " is not one of the " + std::to_string(count) +
                    " az_device_count lists");
    if (slots < 1) return fail("az_replay_create_on: bad capacity");
    AZ_HIP(hipSetDevice(device));
    ReplayDev* d = new ReplayDev();
    d->device = device;
    d->slots = slots;
    const size_t n = (size_t)slots;
    const bool ok = hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&d->ev_gather, hipEventDisableTiming) == hipSuccess &&
                    hipMalloc((void**)&d->pol, n * ROW * sizeof(float)) == hipSuccess &&
                    hipMalloc((void**)&d->val, n * sizeof(float)) == hipSuccess &&
                    hipMalloc((void**)&d->pos, n * sizeof(azc::Pos)) == hipSuccess &&
                    hipHostMalloc((void**)&d->h_dense, ROW * sizeof(float), 0) == hipSuccess &&
                    hipMalloc((void**)&d->d_dense, ROW * sizeof(float)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        replay_dev_destroy(d);
        return fail("az_replay_create_on: cannot allocate " + std::to_string(n * (ROW * sizeof(float) + 4 + sizeof(azc::Pos))) +
                    " bytes of device memory for " + std::to_string(slots) + " entries");
    }
    *out = d;
    return 0;
}

int replay_dev_add(az_replay* r, const az_episode_step* steps, int n, const az_pos* dstate, const float* dpolicy,
                   float dvalue) {
    ReplayDev* d = r->dev;
    AZ_HIP(hipSetDevice(d->device));
    if (wait_gather(d) != 0) return -1;
    int chunk = ADD_CHUNK_DEFAULT;
    if (const char* e = getenv("AZ_REPLAY_ADD_CHUNK")) chunk = std::min(std::max(atoi(e), 1), ADD_CHUNK_MAX);
    chunk = std::min(chunk, n);
    // a larger staging buffer from an earlier call serves a smaller chunk as it is
    if (ensure_add_staging(d, chunk) != 0) return -1;
    int added = 0;
    for (int i = 0; i < n; i++) {
        const az_episode_step* st = dstate ? nullptr : steps + i;
        const char* bad = nullptr;
        if (st) {   // refused on the host, before anything of this step is staged
            if (st->nvis < 0 || st->nvis > MAX_EDGES) bad = "az_replay_add: bad arguments";
            for (int j = 0; !bad && j < st->nvis; j++)
                if (st->vis_idx[j] >= AZ_ACTION_SPACE) bad = "az_replay_add: bad move index";
        }
        if (bad) {   // the steps before it are applied, as az_replay_add_many does on the host
            if (add_flush(d) != 0) return -1;
            return fail(bad);
        }
        const std::string key = replay_fen_of(st ? &st->state : dstate);
        AddRec rc{};
        auto it = r->buffer.find(key);
        if (it != r->buffer.end()) {
            auto& e = it->second;
            rc.slot = e.slot;
            rc.merge = 1;
            rc.old_count = (float)e.visit_count;
            e.visit_count += 1;
        } else {
            if ((int)r->order.size() >= r->capacity && !r->order.empty()) {
                auto ev = r->buffer.find(r->order.front());
                r->free_slots.push_back(ev->second.slot);   // may be taken again by this very step
                r->buffer.erase(ev);
                r->order.pop_front();
            }
            if (r->free_slots.empty()) {
                if (add_flush(d) != 0) return -1;
                return fail("az_replay_add: no free slot");   // not reachable: every entry holds exactly one
            }
            az_replay::Entry e;
            e.visit_count = 1;
            e.slot = r->free_slots.back();
            r->free_slots.pop_back();
            e.bad = az_pos_from_fen(key.c_str(), &e.pos) != 0;   // what az_replay_sample returns (memory.rs:95)
            if (e.bad) e.pos = az_pos{};
            rc.slot = e.slot;
            rc.pos_idx = d->npos;
            memcpy(&d->h_pos[d->npos++], &e.pos, sizeof(az_pos));
            r->buffer.emplace(key, std::move(e));
            r->order.push_back(key);
            added++;
        }
        if (rc.slot < 0 || rc.slot >= d->slots) return fail("az_replay_add: slot out of range");
        if (st) {
            rc.value = st->final_value;
            rc.nvis = st->nvis;
            rc.pair_off = d->npair;
            for (int j = 0; j < st->nvis; j++) d->h_pairs[d->npair++] = (uint32_t)st->vis_idx[j] | (uint32_t)st->vis_n[j] << 16;
        } else {
            rc.value = dvalue;
            rc.dense = 1;
            memcpy(d->h_dense, dpolicy, ROW * sizeof(float));
            AZ_HIP(hipMemcpyAsync(d->d_dense, d->h_dense, ROW * sizeof(float), hipMemcpyHostToDevice, d->st));
        }
        d->h_recs[d->nrec++] = rc;
        if (d->nrec == chunk && add_flush(d) != 0) return -1;
    }
    if (add_flush(d) != 0) return -1;
    return added;
}

int replay_dev_gather(ReplayDev* d, const int* slots, int n, int lo, int hi, float* d_planes, float* d_policy,
                      float* d_value, hipStream_t st) {
    AZ_HIP(hipSetDevice(d->device));
    if (wait_gather(d) != 0 || ensure_slots(d, n) != 0) return -1;
    for (int k = 0; k < n; k++)
        if (slots[k] < 0 || slots[k] >= d->slots) return fail("az_replay_sample: slot out of range");
    const bool own = st == nullptr;
    if (own) st = d->st;
    memcpy(d->h_slots, slots, (size_t)n * sizeof(int));
    AZ_HIP(hipMemcpyAsync(d->d_slots, d->h_slots, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    k_replay_gather<<<hi - lo, 256, 0, st>>>(d->d_slots + lo, d->pol, d->val, d->pos, d_planes, d_policy, d_value);
    AZ_HIP(hipGetLastError());
    if (own) {
        AZ_HIP(hipStreamSynchronize(st));
    } else {
        AZ_HIP(hipEventRecord(d->ev_gather, st));
        d->gather_pending = true;
    }
    return 0;
}

int replay_dev_read(ReplayDev* d, const int* slots, int n, float* planes, float* policy, float* value) {
    AZ_HIP(hipSetDevice(d->device));
    if (n < 1) return 0;
    if ((size_t)n > d->stage_rows) {
        if (wait_gather(d) != 0) return -1;
        (void)hipFree(d->d_stage);
        d->d_stage = nullptr;
        d->stage_rows = 0;
        if (hipMalloc((void**)&d->d_stage, (size_t)n * (PLANE_FLOATS + ROW + 1) * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail("az_replay_sample: out of device memory for " + std::to_string(n) + " staged rows");
        }
        d->stage_rows = (size_t)n;
    }
    // policy first: its rows stay 16-byte aligned
    float* s_pol = d->d_stage;
    float* s_planes = s_pol + (size_t)n * ROW;
    float* s_val = s_planes + (size_t)n * PLANE_FLOATS;
    // on the buffer's own stream: the gather returns when the rows are staged
    if (replay_dev_gather(d, slots, n, 0, n, planes ? s_planes : nullptr, policy ? s_pol : nullptr,
                          value ? s_val : nullptr, nullptr) != 0)
        return -1;
    if (planes) AZ_HIP(hipMemcpyAsync(planes, s_planes, (size_t)n * PLANE_FLOATS * sizeof(float), hipMemcpyDeviceToHost, d->st));
    if (policy) AZ_HIP(hipMemcpyAsync(policy, s_pol, (size_t)n * ROW * sizeof(float), hipMemcpyDeviceToHost, d->st));
    if (value) AZ_HIP(hipMemcpyAsync(value, s_val, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, d->st));
    AZ_HIP(hipStreamSynchronize(d->st));
    return 0;
}

int replay_dev_upload(ReplayDev* d, int first, int n, const float* policy, const float* value, const az_pos* pos) {
    if (first < 0 || n < 0 || first + n > d->slots) return fail("az_replay_load_on: slot out of range");
    AZ_HIP(hipSetDevice(d->device));
    AZ_HIP(hipMemcpy(d->pol + (size_t)first * ROW, policy, (size_t)n * ROW * sizeof(float), hipMemcpyHostToDevice));
    AZ_HIP(hipMemcpy(d->val + first, value, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    AZ_HIP(hipMemcpy(d->pos + first, pos, (size_t)n * sizeof(az_pos), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace azi
