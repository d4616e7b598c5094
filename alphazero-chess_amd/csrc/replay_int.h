// replay_int.h -- the replay buffer's record, shared by replay.hip (keys, FIFO, draw, file format) and
// replay_dev.hip (the payload rows in HBM and the kernels that write and gather them).
#pragma once
#include <deque>
#include <string>
#include <unordered_map>
#include <vector>

#include "az_internal.h"

namespace azi { struct ReplayDev; }

struct az_replay {
    struct Entry {
        std::vector<float> policy;   // [4096]; empty in a device-backed buffer (the row is in HBM)
        float value = 0.0f;          // host-backed only
        uint64_t visit_count = 0;
        // device-backed: the payload slot, the position rebuilt from the key (what the slot holds), and
        // whether the key failed to rebuild (az_replay_sample then fails on it, as the host buffer does)
        int slot = -1;
        az_pos pos = {};
        bool bad = false;
    };
    int capacity = 100000;           // REPLAY_BUFFER_SIZE, parameters.rs:10
    std::unordered_map<std::string, Entry> buffer;
    std::deque<std::string> order;
    azi::ReplayDev* dev = nullptr;   // payload rows in HBM (az_replay_create_on), else host memory
    std::vector<int> free_slots;     // device-backed: slots no entry holds
};

namespace azi {

std::string replay_fen_of(const az_pos* p);

// replay_dev.hip.  Every slot handed to these is one the host assigned: 0 <= slot < slots.
int replay_dev_create(int slots, int device, ReplayDev** out);
void replay_dev_destroy(ReplayDev* d);
int replay_dev_device(const ReplayDev* d);
// az_replay_add of steps[0..n) (dstate == nullptr), or az_replay_add_dense of (dstate, dpolicy, dvalue)
// with n = 1: the host resolves keys, FIFO and counts, the rows are written by k_replay_add.  Returns the
// number of new entries; a bad step fails after the steps before it were applied.
int replay_dev_add(az_replay* r, const az_episode_step* steps, int n, const az_pos* dstate, const float* dpolicy,
                   float dvalue);
// rows slots[lo..hi) -> device pointers (any may be null), row lo at index 0, ordered on st (nullptr: the
// buffer's stream).  slots[0..n) is uploaded whole.
int replay_dev_gather(ReplayDev* d, const int* slots, int n, int lo, int hi, float* d_planes, float* d_policy,
                      float* d_value, hipStream_t st);
// the same to host pointers: gather into the staging buffer, one synchronisation
int replay_dev_read(ReplayDev* d, const int* slots, int n, float* planes, float* policy, float* value);
// rows from host memory into slots first .. first + n - 1 (az_replay_load_on)
int replay_dev_upload(ReplayDev* d, int first, int n, const float* policy, const float* value, const az_pos* pos);

}  // namespace azi
