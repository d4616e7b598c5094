// replay.hip -- ReplayBuffer of memory.rs:26-117, host C++ behind the C-ABI.
//
// Entries are keyed by the position's FEN with the pseudo-legal en-passant square
// (memory.rs:42, Fen::from_position(.., EnPassantMode::PseudoLegal)); a position seen again
// folds into a running mean of its improved policy and final value (memory.rs:44-58); a new
// one is appended to a FIFO that evicts the oldest entry at capacity (memory.rs:60-77).
// Sampling draws min(batch, len) distinct entries uniformly (memory.rs:81-101, rand's
// choose_multiple) from a seeded SplitMix64 stream -- the reference's thread_rng is not
// reproducible, so only the distribution is the reference's -- and returns them as network
// inputs (to_tensor planes of the position rebuilt from its FEN, chess.rs:191-245), policies and
// values, ready for az_trainer_step.
// save/load use the reference's on-disk format: bincode 2.0.1 standard config over serde
// (varint lengths and integers, little-endian f32): struct { buffer: HashMap<Fen, MemoryEntry
// { policy: [f32; 4096] (BigArray tuple), value: f32, visit_count: usize }>, order:
// VecDeque<Fen> } with Fen serialised as its string (shakmaty serde).  Restated, not pinned
// against a file the reference wrote (none ships with it).
// A buffer made by az_replay_create_on / az_replay_load_on with a device keeps keys, FIFO and counts
// here and its payload rows in HBM (replay_dev.hip); every entry point below serves both.
#include <string.h>

#include <cstdio>
#include <deque>
#include <string>
#include <unordered_map>
#include <vector>

#include "replay_int.h"

using namespace azi;

namespace azi {
std::string replay_fen_of(const az_pos* p) {
    char buf[128];
    const int n = az_pos_to_fen(p, buf, sizeof(buf));
    return n > 0 ? std::string(buf, n) : std::string();
}
}  // namespace azi

namespace {

// memory.rs:41-79 with the step's improved policy given densely
int replay_add(az_replay* r, const std::string& key, const float* policy, float value) {
    auto it = r->buffer.find(key);
    if (it != r->buffer.end()) {
        auto& e = it->second;
        const float old_count = (float)e.visit_count;
        const float total = old_count + 1.0f;
        e.value = (e.value * old_count + value) / total;
        for (int i = 0; i < AZ_ACTION_SPACE; i++) e.policy[i] = (e.policy[i] * old_count + policy[i]) / total;
        e.visit_count += 1;
        return 0;
    }
    if ((int)r->order.size() >= r->capacity && !r->order.empty()) {
        r->buffer.erase(r->order.front());
        r->order.pop_front();
    }
    az_replay::Entry e;
    e.policy.assign(policy, policy + AZ_ACTION_SPACE);
    e.value = value;
    e.visit_count = 1;
    r->buffer.emplace(key, std::move(e));
    r->order.push_back(key);
    return 1;
}

uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- bincode 2 standard config
void put_varint(std::string& o, uint64_t v) {
    if (v < 251) { o += (char)v; return; }
    if (v <= 0xFFFF) { o += (char)251; for (int i = 0; i < 2; i++) o += (char)(v >> (8 * i)); return; }
    if (v <= 0xFFFFFFFFull) { o += (char)252; for (int i = 0; i < 4; i++) o += (char)(v >> (8 * i)); return; }
    o += (char)253;
    for (int i = 0; i < 8; i++) o += (char)(v >> (8 * i));
}
void put_f32(std::string& o, float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    for (int i = 0; i < 4; i++) o += (char)(u >> (8 * i));
}
void put_str(std::string& o, const std::string& s) { put_varint(o, s.size()); o += s; }

struct Reader {
    const unsigned char* p; size_t n, i = 0; bool ok = true;
    uint64_t le(int k) {
        if (i + k > n) { ok = false; return 0; }
        uint64_t v = 0;
        for (int j = 0; j < k; j++) v |= (uint64_t)p[i + j] << (8 * j);
        i += k;
        return v;
    }
    uint64_t varint() {
        const uint64_t b = le(1);
        if (b < 251) return b;
        if (b == 251) return le(2);
        if (b == 252) return le(4);
        if (b == 253) return le(8);
        ok = false;                  // 254 = u128: never a length here
        return 0;
    }
    float f32() { const uint32_t u = (uint32_t)le(4); float f; memcpy(&f, &u, 4); return f; }
    std::string str() {
        const uint64_t k = varint();
        if (!ok || i + k > n) { ok = false; return std::string(); }
        std::string s(reinterpret_cast<const char*>(p + i), k);
        i += k;
        return s;
    }
};

}  // namespace

extern "C" {

int az_replay_create(int capacity, az_replay** out) {
    if (!out || capacity < 1) return fail("az_replay_create: bad arguments");
    az_replay* r = new az_replay();
    r->capacity = capacity;
    r->buffer.reserve(std::min(capacity, 1 << 20));
    *out = r;
    return 0;
}

int az_replay_create_on(int capacity, int device, az_replay** out) {
    if (device == AZ_DEVICE_HOST) return az_replay_create(capacity, out);
    if (!out || capacity < 1) return fail("az_replay_create_on: bad arguments");
    az_replay* r = new az_replay();
    r->capacity = capacity;
    r->buffer.reserve(std::min(capacity, 1 << 20));
    if (replay_dev_create(capacity, device, &r->dev) != 0) { delete r; return -1; }
    for (int s = capacity - 1; s >= 0; s--) r->free_slots.push_back(s);   // handed out from slot 0 up
    *out = r;
    return 0;
}

int az_replay_destroy(az_replay* r) {
    if (r && r->dev) replay_dev_destroy(r->dev);
    delete r;
    return 0;
}

int az_replay_len(const az_replay* r) { return r ? (int)r->buffer.size() : fail("null"); }

int az_replay_device(const az_replay* r) {
    if (!r) return fail("az_replay_device: null");   // -1 = AZ_DEVICE_HOST as a value: the message tells them apart
    return r->dev ? replay_dev_device(r->dev) : AZ_DEVICE_HOST;
}

int az_replay_add(az_replay* r, const az_episode_step* st) {
    if (!r || !st || st->nvis < 0 || st->nvis > 224) return fail("az_replay_add: bad arguments");
    if (r->dev) return replay_dev_add(r, st, 1, nullptr, nullptr, 0.0f);
    // improved policy = visits / sum(visits) over the 4096 entries (tree.rs:110-114, T = 1)
    std::vector<float> pol(AZ_ACTION_SPACE, 0.0f);
    float sum = 0.0f;
    for (int i = 0; i < st->nvis; i++) sum += (float)st->vis_n[i];
    for (int i = 0; i < st->nvis; i++) {
        if (st->vis_idx[i] >= AZ_ACTION_SPACE) return fail("az_replay_add: bad move index");
        pol[st->vis_idx[i]] = (float)st->vis_n[i] / sum;
    }
    return replay_add(r, replay_fen_of(&st->state), pol.data(), st->final_value);
}

int az_replay_add_many(az_replay* r, const az_episode_step* steps, int n) {
    if (!r || n < 0 || (n > 0 && !steps)) return fail("az_replay_add_many: bad arguments");
    if (r->dev) return n ? replay_dev_add(r, steps, n, nullptr, nullptr, 0.0f) : 0;
    int added = 0;
    for (int i = 0; i < n; i++) {   // in order, exactly as n calls of az_replay_add
        const int rc = az_replay_add(r, steps + i);
        if (rc < 0) return rc;
        added += rc;
    }
    return added;
}

int az_replay_add_dense(az_replay* r, const az_pos* state, const float* policy, float value) {
    if (!r || !state || !policy) return fail("null");
    if (r->dev) return replay_dev_add(r, nullptr, 1, state, policy, value);
    return replay_add(r, replay_fen_of(state), policy, value);
}

// the draw of az_replay_sample: idx[0..n) = FIFO positions of n = min(batch, len) distinct entries
static int replay_draw(const az_replay* r, int batch, uint64_t seed, std::vector<int>& idx) {
    const int len = (int)r->order.size();
    const int n = std::min(batch, len);
    // partial Fisher-Yates over the FIFO positions: n distinct entries, uniformly
    idx.resize(len);
    for (int i = 0; i < len; i++) idx[i] = i;
    uint64_t s = seed ^ 0xA0761D6478BD642Full;
    for (int i = 0; i < n; i++) {
        const int j = i + (int)(splitmix(s) % (uint64_t)(len - i));
        std::swap(idx[i], idx[j]);
    }
    return n;
}

// device-backed: the drawn entries' payload slots (and their positions); < 0 if one's key does not rebuild
static int replay_draw_slots(const az_replay* r, const std::vector<int>& idx, int n, std::vector<int>& slots,
                             az_pos* states) {
    slots.resize(n);
    for (int k = 0; k < n; k++) {
        const auto& e = r->buffer.at(r->order[idx[k]]);
        if (e.bad) { az_pos p; return az_pos_from_fen(r->order[idx[k]].c_str(), &p) != 0 ? -1 : fail("az_replay: bad entry"); }
        slots[k] = e.slot;
        if (states) states[k] = e.pos;
    }
    return 0;
}

int az_replay_sample(az_replay* r, int batch, uint64_t seed, float* planes, float* policy, float* value,
                     az_pos* states) {
    if (!r || batch < 0) return fail("az_replay_sample: bad arguments");
    std::vector<int> idx;
    const int n = replay_draw(r, batch, seed, idx);
    if (r->dev) {   // gather on the device, one read-back
        std::vector<int> slots;
        if (replay_draw_slots(r, idx, n, slots, states) != 0) return -1;
        if (n > 0 && (planes || policy || value) && replay_dev_read(r->dev, slots.data(), n, planes, policy, value) != 0)
            return -1;
        return n;
    }
    for (int k = 0; k < n; k++) {
        const std::string& key = r->order[idx[k]];
        const auto& e = r->buffer.at(key);
        az_pos p;
        if (az_pos_from_fen(key.c_str(), &p) != 0) return -1;   // into_position (memory.rs:95)
        if (states) states[k] = p;
        if (planes) az_pos_encode(&p, planes + (size_t)k * AZ_PLANES * 64);
        if (policy) memcpy(policy + (size_t)k * AZ_ACTION_SPACE, e.policy.data(), AZ_ACTION_SPACE * sizeof(float));
        if (value) value[k] = e.value;
    }
    return n;
}

int az_replay_sample_rows(az_replay* r, int batch, uint64_t seed, int lo, int hi, float* d_planes, float* d_policy,
                          float* d_value, void* stream) {
    if (!r || batch < 0) return fail("az_replay_sample_rows: bad arguments");
    if (!r->dev) return fail("az_replay_sample_rows: the buffer is host-backed (az_replay_create_on a device)");
    if (((uintptr_t)d_planes | (uintptr_t)d_value) % 4 || (uintptr_t)d_policy % 16)
        return fail("az_replay_sample_rows: d_policy must be 16-byte aligned, d_planes and d_value 4-byte");
    std::vector<int> idx, slots;
    const int n = replay_draw(r, batch, seed, idx);
    if (lo < 0 || lo > hi || hi > n)
        return fail("az_replay_sample_rows: rows [" + std::to_string(lo) + ", " + std::to_string(hi) + ") of a draw of " +
                    std::to_string(n));
    if (replay_draw_slots(r, idx, n, slots, nullptr) != 0) return -1;
    if (hi > lo && replay_dev_gather(r->dev, slots.data(), n, lo, hi, d_planes, d_policy, d_value,
                                     reinterpret_cast<hipStream_t>(stream)) != 0)
        return -1;
    return n;
}

int az_replay_save(const az_replay* r, const char* path) {
    if (!r || !path) return fail("null");
    std::string o;
    o.reserve(r->order.size() * (AZ_ACTION_SPACE * 4 + 120) + 16);
    put_varint(o, r->buffer.size());
    // device-backed: the rows come back in FIFO order, SAVE_ROWS at a time
    constexpr int SAVE_ROWS = 256;
    std::vector<float> rows, vals;
    std::vector<int> slots;
    size_t at = 0;
    for (const auto& key : r->order) {        // HashMap order is unspecified; FIFO order here
        const auto& e = r->buffer.at(key);
        const float* pol = e.policy.data();
        float val = e.value;
        if (r->dev) {
            if (at % SAVE_ROWS == 0) {
                const int k = (int)std::min<size_t>(SAVE_ROWS, r->order.size() - at);
                slots.resize(k);
                for (int j = 0; j < k; j++) slots[j] = r->buffer.at(r->order[at + j]).slot;
                rows.resize((size_t)k * AZ_ACTION_SPACE);
                vals.resize(k);
                if (replay_dev_read(r->dev, slots.data(), k, nullptr, rows.data(), vals.data()) != 0) return -1;
            }
            pol = rows.data() + (at % SAVE_ROWS) * AZ_ACTION_SPACE;
            val = vals[at % SAVE_ROWS];
            at++;
        }
        put_str(o, key);
        for (int i = 0; i < AZ_ACTION_SPACE; i++) put_f32(o, pol[i]);
        put_f32(o, val);
        put_varint(o, e.visit_count);
    }
    put_varint(o, r->order.size());
    for (const auto& key : r->order) put_str(o, key);
    FILE* f = fopen(path, "wb");
    if (!f) return fail(std::string("az_replay_save: cannot open ") + path);
    const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
    fclose(f);
    return ok ? 0 : fail("az_replay_save: write failed");
}

int az_replay_load(const char* path, int capacity, az_replay** out) {
    if (!path || !out) return fail("null");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(std::string("az_replay_load: cannot open ") + path);
    std::string data;
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) data.append(buf, k);
    fclose(f);
    Reader rd{reinterpret_cast<const unsigned char*>(data.data()), data.size()};
    az_replay* r = new az_replay();
    r->capacity = capacity > 0 ? capacity : 100000;
    const uint64_t nmap = rd.varint();
    for (uint64_t i = 0; rd.ok && i < nmap; i++) {
        std::string key = rd.str();
        az_replay::Entry e;
        e.policy.resize(AZ_ACTION_SPACE);
        for (int j = 0; j < AZ_ACTION_SPACE; j++) e.policy[j] = rd.f32();
        e.value = rd.f32();
        e.visit_count = rd.varint();
        if (rd.ok) r->buffer[key] = std::move(e);
    }
    const uint64_t nord = rd.ok ? rd.varint() : 0;
    for (uint64_t i = 0; rd.ok && i < nord; i++) r->order.push_back(rd.str());
    if (!rd.ok || rd.i != rd.n || r->order.size() != r->buffer.size()) {
        delete r;
        return fail("az_replay_load: malformed file");
    }
    for (const auto& key : r->order)
        if (!r->buffer.count(key)) { delete r; return fail("az_replay_load: order names a missing entry"); }
    *out = r;
    return 0;
}

int az_replay_load_on(const char* path, int capacity, int device, az_replay** out) {
    if (device == AZ_DEVICE_HOST) return az_replay_load(path, capacity, out);
    if (!path || !out) return fail("null");
    az_replay* r = nullptr;
    if (az_replay_load(path, capacity, &r) != 0) return -1;
    // a file may hold more entries than `capacity` (the host buffer then keeps them all, evicting one
    // per new entry): as many slots as that takes
    const int len = (int)r->order.size(), slots = std::max(r->capacity, len);
    if (replay_dev_create(slots, device, &r->dev) != 0) { delete r; return -1; }
    constexpr int ROWS = 256;
    std::vector<float> pol((size_t)ROWS * AZ_ACTION_SPACE), val(ROWS);
    std::vector<az_pos> pos(ROWS);
    for (int first = 0; first < len; first += ROWS) {
        const int k = std::min(ROWS, len - first);
        for (int j = 0; j < k; j++) {
            const std::string& key = r->order[first + j];
            auto& e = r->buffer.at(key);
            e.slot = first + j;
            e.bad = az_pos_from_fen(key.c_str(), &e.pos) != 0;
            if (e.bad) e.pos = az_pos{};
            memcpy(&pol[(size_t)j * AZ_ACTION_SPACE], e.policy.data(), AZ_ACTION_SPACE * sizeof(float));
            val[j] = e.value;
            pos[j] = e.pos;
            std::vector<float>().swap(e.policy);
        }
        if (replay_dev_upload(r->dev, first, k, pol.data(), val.data(), pos.data()) != 0) {
            az_replay_destroy(r);
            return -1;
        }
    }
    for (int s = slots - 1; s >= len; s--) r->free_slots.push_back(s);
    *out = r;
    return 0;
}

}  // extern "C"
