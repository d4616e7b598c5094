"""The device-backed replay buffer (az_replay_create_on, csrc/replay_dev.hip) against the host buffer fed
the same calls: return values, entries, running means, FIFO order, samples and save files are EQUAL, and
a training step fed from it in HBM (az_trainer_step_replay / _device) is bit for bit the step on the
host sample.  No tolerance anywhere: the kernels restate az_replay_add's arithmetic operation for
operation (f32, IEEE division, no contraction) and plane_value is the host's own function.

Device memory for the *_device entry points comes from azchess.hiprt (the HIP runtime libaz is bound to),
wrapped in an object with data_ptr() -- the form a torch tensor has; a second HIP runtime is kept out of
the test process."""
import ctypes as C

import numpy as np
import pytest

import azchess as A
from azchess import _lib as L
from azchess.memory import ReplayBuffer
from azchess.training import Trainer, train

pytestmark = pytest.mark.gpu

SEEDS = (0, 5, 77)


# ------------------------------------------------------------------ generators (tests/test_replay.py's)
def positions(n, seed):
    """Positions from random playouts, with repeats (transpositions of the opening)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        gs = A.GameState()
        for _ in range(int(rng.integers(0, 12))):
            idx = gs.position.legal_indices()
            if len(idx) == 0 or int(A.play_move(gs, int(rng.choice(idx)))) != 0:
                break
        out.append(gs.position)
    return out


def step(pos, rng):
    idx = np.unique(pos.legal_indices())
    v = rng.integers(1, 30, len(idx)).astype(np.float32)
    pol = np.zeros(4096, np.float32)
    pol[idx] = v / np.float32(v.sum())
    return A.EpisodeStep(pos, pol, float(np.float32(rng.uniform(-1, 1))), 3)


def distinct(n, seed):
    seen, out = set(), []
    for k in range(100):
        for p in positions(2 * n, seed + 1000 * k):
            if p.fen() not in seen:
                seen.add(p.fen())
                out.append(p)
            if len(out) == n:
                return out
    raise AssertionError("too few distinct positions")


def record(pos, pairs, value=0.25, nvis=None):
    """An az_episode_step built by hand: (move index, visits) pairs as given, duplicates included."""
    st = L.AzEpisodeStep()
    st.state = pos._p
    st.final_value = value
    st.nvis = len(pairs) if nvis is None else nvis
    for i, (ix, n) in enumerate(pairs):
        st.vis_idx[i], st.vis_n[i] = ix, n
    return st


def raw_step(pos, rng):
    """What a drain gives: the legal indices in generator order (under-promotions repeat the queen
    promotion's index), a visit count each, some of them 0."""
    idx = pos.legal_indices()
    return record(pos, [(int(ix), int(rng.integers(0, 50))) for ix in idx], float(np.float32(rng.uniform(-1, 1))))


def array_of(steps):
    return (L.AzEpisodeStep * len(steps))(*steps)


def script(nsteps=300, npos=40, seed=11):
    """About nsteps adds over npos distinct positions: one by one (raw and dense) and as add_many arrays."""
    rng = np.random.default_rng(seed)
    pool = distinct(npos, seed + 1)
    ops, left = [], nsteps
    sizes = [1, 1, 23, 1, 1, 40, 1, 17, 1, 64]
    k = 0
    while left > 0:
        n = min(sizes[k % len(sizes)], left)
        pick = [pool[int(i)] for i in rng.integers(0, npos, n)]
        if n == 1:
            ops.append(("one", raw_step(pick[0], rng) if k % 4 == 0 else step(pick[0], rng)))
        else:
            ops.append(("many", array_of([raw_step(p, rng) for p in pick])))
        left -= n
        k += 1
    return ops


def feed(buf, ops):
    """Every op's return value, or the error's class name."""
    out = []
    for kind, x in ops:
        try:
            out.append(buf.add(x) if kind == "one" else buf.add_many(x))
        except L.AzError as e:
            out.append("error: %s" % e)
    return out


def saved(buf, path):
    buf.save(path)
    return path.read_bytes()


def assert_same(host, dev, tmp_path):
    """len, every entry in draw order for three seeds, a short draw, the save file."""
    assert len(host) == len(dev)
    for seed in SEEDS:
        for batch in (1000, 5):
            a, b = host.sample_arrays(batch, seed), dev.sample_arrays(batch, seed)
            for x, y in zip(a[:3], b[:3]):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
            assert [bytes(s._p) for s in a[3]] == [bytes(s._p) for s in b[3]]
        sa, sb = host.sample(1000, seed), dev.sample(1000, seed)
        assert [s.state.fen() for s in sa] == [s.state.fen() for s in sb]
        assert all(x.policy.tobytes() == y.policy.tobytes() and np.float32(x.value).tobytes() == np.float32(y.value).tobytes()
                   for x, y in zip(sa, sb))             # bytes: a 0 / 0 policy is NaN on both sides
    assert saved(host, tmp_path / "host.bin") == saved(dev, tmp_path / "dev.bin")


def pair(capacity):
    host, dev = ReplayBuffer(capacity), ReplayBuffer(capacity, device=0)
    assert host.device is None and dev.device == 0 and L.lib.az_replay_device(dev._h) == 0
    return host, dev


@pytest.fixture(scope="module")
def parity_ops():
    return script()


# ------------------------------------------------------------------ add / merge / evict parity
def test_add_merge_evict_parity(require_gpu, parity_ops, tmp_path):
    host, dev = pair(8)
    ra, rb = feed(host, parity_ops), feed(dev, parity_ops)
    assert ra == rb and not any(isinstance(x, str) for x in ra)
    assert sum(ra) > 8 and len(host) == 8          # evictions happened; merges: fewer new entries than steps
    assert sum(ra) < sum(1 if k == "one" else len(x) for k, x in parity_ops)
    assert_same(host, dev, tmp_path)


# ------------------------------------------------------------------ hand-built records
def test_same_position_five_times_in_one_call(require_gpu, tmp_path):
    host, dev = pair(4)
    p = A.Position.startpos()
    arr = array_of([record(p, [(588, 5 + i), (1540, 3), (12, i)], 0.1 * i - 0.2) for i in range(5)])
    assert host.add_many(arr) == dev.add_many(arr) == 1
    assert_same(host, dev, tmp_path)


def test_evicted_and_readded_within_one_call(require_gpu, tmp_path):
    host, dev = pair(2)
    a, b, c = distinct(3, 2)
    seq = [a, b, a, c, a, b, a, a, c]              # a is merged, evicted by c, re-added, evicted, re-added ...
    arr = array_of([record(p, [(100 + i, 3 + i), (200, 7)], 0.05 * i) for i, p in enumerate(seq)])
    ra, rb = host.add_many(arr), dev.add_many(arr)
    assert ra == rb and ra > 3
    assert_same(host, dev, tmp_path)


def test_duplicate_indices_last_entry_wins(require_gpu, tmp_path):
    host, dev = pair(4)
    p, q = distinct(2, 3)
    two = record(p, [(588, 5), (1540, 3), (588, 9)], 0.5)
    three = record(q, [(7, 1), (7, 20), (4095, 2), (7, 3), (0, 4)], -0.5)
    for st in (two, three, two, three):            # assign, then merge
        assert host.add(st) == dev.add(st)
    pol = {s.state.fen(): s.policy for s in dev.sample(10, 0)}
    assert pol[p.fen()][588] == np.float32(9) / np.float32(17) and pol[q.fen()][7] == np.float32(3) / np.float32(30)
    assert_same(host, dev, tmp_path)


def test_nvis_224_and_nvis_0(require_gpu, tmp_path):
    host, dev = pair(4)
    p, q, r = distinct(3, 4)
    full = record(p, [((i * 37) % 4096, 1 + (i * 7) % 300) for i in range(224)], 0.75)
    empty = record(q, [], -1.0)
    zero = record(r, [(5, 0), (6, 0)], 0.0)        # visits that sum to 0: 0 / 0, as on the host
    for st in (full, empty, zero, full, empty):
        assert host.add(st) == dev.add(st)
    arr = array_of([full, empty, full])
    assert host.add_many(arr) == dev.add_many(arr) == 0
    assert_same(host, dev, tmp_path)


def test_bad_index_in_the_middle_of_an_array(require_gpu, tmp_path):
    host, dev = pair(4)
    a, b, c, d = distinct(4, 5)
    good = [record(a, [(1, 2), (3, 4)]), record(b, [(9, 1)]), record(a, [(1, 5)])]
    bad = record(c, [(10, 1), (4096, 1), (11, 1)])
    arr = array_of(good + [bad, record(d, [(2, 2)])])
    msgs = []
    for buf in (host, dev):
        with pytest.raises(L.AzError, match="bad move index") as e:
            buf.add_many(arr)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    assert len(host) == len(dev) == 2              # the three steps before it, nothing after
    assert_same(host, dev, tmp_path)
    over = record(c, [(1, 1)], nvis=225)
    for buf in (host, dev):
        with pytest.raises(L.AzError, match="bad arguments"):
            buf.add_many(array_of([record(d, [(2, 2)]), over]))
    assert len(host) == len(dev) == 3
    assert_same(host, dev, tmp_path)


# ------------------------------------------------------------------ chunk boundaries
def test_chunk_size_changes_nothing(require_gpu, parity_ops, tmp_path, monkeypatch):
    host = ReplayBuffer(8)
    want = feed(host, parity_ops)
    ref = saved(host, tmp_path / "host.bin")
    p = A.Position.startpos()
    merged = array_of([record(p, [(588, 1 + i), (1540, 2)], 0.01 * i) for i in range(40)])
    want2 = host.add_many(merged)
    ref2 = saved(host, tmp_path / "host2.bin")
    for chunk in ("1", "16", None):
        if chunk is None:
            monkeypatch.delenv("AZ_REPLAY_ADD_CHUNK", raising=False)
        else:
            monkeypatch.setenv("AZ_REPLAY_ADD_CHUNK", chunk)
        dev = ReplayBuffer(8, device=0)
        assert feed(dev, parity_ops) == want
        assert saved(dev, tmp_path / ("dev%s.bin" % chunk)) == ref
        assert dev.add_many(merged) == want2
        assert saved(dev, tmp_path / ("dev2%s.bin" % chunk)) == ref2   # one slot merged across chunks
    assert_same(host, dev, tmp_path)


# ------------------------------------------------------------------ load_on
def test_load_on_device(require_gpu, parity_ops, tmp_path):
    host = ReplayBuffer(8)
    feed(host, parity_ops)
    raw = saved(host, tmp_path / "r.bin")
    dev = ReplayBuffer.load(tmp_path / "r.bin", 8, device=0)
    assert dev.device == 0
    assert_same(host, dev, tmp_path)
    assert saved(dev, tmp_path / "again.bin") == raw
    more = [("many", array_of([raw_step(p, np.random.default_rng(1)) for p in distinct(12, 6)]))]
    assert feed(host, more) == feed(dev, more)      # the loaded counts and FIFO carry on
    assert_same(host, dev, tmp_path)
    big = ReplayBuffer.load(tmp_path / "r.bin", 3, device=0)   # a file longer than the capacity
    small = ReplayBuffer.load(tmp_path / "r.bin", 3)
    assert feed(small, more) == feed(big, more)
    assert_same(small, big, tmp_path)


# ------------------------------------------------------------------ the trainer fed in HBM
B, F, MAXB, LR = 2, 32, 8, 3e-3


@pytest.fixture(scope="module")
def weights():
    return A.random_weights(B, F, seed=7)


@pytest.fixture(scope="module")
def filled():
    """A host and a device buffer of about 30 entries, and a pair of 5."""
    rng = np.random.default_rng(21)
    host, dev = pair(64)
    ops = [("many", array_of([raw_step(p, rng) for p in distinct(30, 8) * 2]))]
    assert feed(host, ops) == feed(dev, ops) == [30]
    h5, d5 = pair(64)
    ops = [("many", array_of([raw_step(p, rng) for p in distinct(5, 9)]))]
    assert feed(h5, ops) == feed(d5, ops) == [5]
    return host, dev, h5, d5


def trainers(weights):
    return Trainer(B, F, weights, max_batch=MAXB), Trainer(B, F, weights, max_batch=MAXB)


def same_trainers(a, b):
    assert a.params().tobytes() == b.params().tobytes()
    assert a.grads().tobytes() == b.grads().tobytes()


@pytest.mark.parametrize("lo,hi", [(0, None), (3, 7)])
def test_step_replay_equals_step_on_the_host_sample(require_gpu, weights, filled, lo, hi):
    host, dev = filled[:2]
    a, b = trainers(weights)
    for seed in (3, 4, 5):
        planes, pol, val, _ = host.sample_arrays(MAXB, seed)
        sl = slice(lo, hi)
        la = a.step(planes[sl], pol[sl], val[sl], LR)
        lb = b.step_replay(dev, MAXB, seed, LR, lo, hi)
        assert la == lb
        same_trainers(a, b)


def test_step_replay_with_batch_larger_than_len(require_gpu, weights, filled):
    h5, d5 = filled[2:]
    a, b = trainers(weights)
    for seed in (1, 2, 3):
        planes, pol, val, _ = h5.sample_arrays(MAXB, seed)
        assert planes.shape[0] == 5
        assert a.step(planes, pol, val, LR) == b.step_replay(d5, MAXB, seed, LR)
        same_trainers(a, b)
    drawn = C.c_int(-1)
    loss = np.zeros(2, np.float32)
    L.check(L.lib.az_trainer_step_replay(b._h, d5._h, 1000, 9, 1, -1, LR, L.fptr(loss), C.byref(drawn)))
    assert drawn.value == 5
    planes, pol, val, _ = h5.sample_arrays(1000, 9)
    assert a.step(planes[1:], pol[1:], val[1:], LR) == (float(loss[0]), float(loss[1]))
    same_trainers(a, b)


def test_compute_grads_replay_then_apply(require_gpu, weights, filled):
    host, dev = filled[:2]
    a, b = trainers(weights)
    for seed in (6, 7, 8):
        planes, pol, val, _ = host.sample_arrays(MAXB, seed)
        assert a.compute_gradients(planes[2:], pol[2:], val[2:]) == b.compute_grads_replay(dev, MAXB, seed, 2)
        same_trainers(a, b)
        a.apply(LR)
        b.apply(LR)
        same_trainers(a, b)


class DeviceArray:
    """A device buffer of the runtime libaz is bound to, with the data_ptr() a torch tensor has."""

    def __init__(self, hip, like):
        self.hip, self.like = hip, np.ascontiguousarray(like, np.float32)
        self.p = hip.malloc(max(self.like.nbytes, 16))

    def data_ptr(self):
        return self.p.value

    def put(self):
        self.hip.copy_in(self.p, self.like)
        return self

    def get(self):
        return self.hip.download(self.p, np.empty_like(self.like))

    def free(self):
        self.hip.free(self.p)


def test_step_device_and_sample_rows(require_gpu, weights, filled):
    from azchess.hiprt import Hip
    hip = Hip()
    host, dev = filled[:2]
    a, b = trainers(weights)
    bufs = []
    try:
        for seed in (12, 13):
            planes, pol, val, _ = host.sample_arrays(MAXB, seed)
            up = [DeviceArray(hip, x).put() for x in (planes, pol, val)]
            bufs += up
            assert a.step(planes, pol, val, LR) == b.step_device(up[0], up[1], up[2], MAXB, LR)
            same_trainers(a, b)
            assert a.compute_gradients(planes[:3], pol[:3], val[:3]) == \
                b.compute_grads_device(up[0].data_ptr(), up[1].data_ptr(), up[2].data_ptr(), 3)
            same_trainers(a, b)
        # sample_rows into caller's buffers: the whole draw on the buffer's stream, rows on a caller's
        stream = hip.stream()
        for lo, hi, st in ((0, None, None), (3, 7, stream), (30, 30, None)):
            planes, pol, val, _ = host.sample_arrays(1000, 31)
            n = planes.shape[0]
            sl = slice(lo, hi)
            out = [DeviceArray(hip, np.full_like(x[sl], 7.0)).put() for x in (planes, pol, val)]
            bufs += out
            assert dev.sample_rows(1000, 31, out[0], out[1], out[2], lo=lo, hi=hi, stream=st) == n
            if st is not None:
                hip.stream_synchronize(st)
            for x, o in zip((planes, pol, val), out):
                assert o.get().tobytes() == x[sl].tobytes()
        hip.stream_destroy(stream)
        only_pol = DeviceArray(hip, np.zeros((2, 4096), np.float32)).put()
        bufs.append(only_pol)
        assert dev.sample_rows(2, 5, policy=only_pol) == 2
        assert only_pol.get().tobytes() == host.sample_arrays(2, 5)[1].tobytes()
    finally:
        for x in bufs:
            x.free()


# ------------------------------------------------------------------ error paths
def test_errors_change_nothing(require_gpu, weights, filled, tmp_path):
    host, dev = filled[:2]
    a, b = trainers(weights)
    before = b.params().tobytes()
    file_before = saved(dev, tmp_path / "before.bin")
    empty = ReplayBuffer(4, device=0)
    n = len(dev)
    cases = [(dev, 1000, 0, MAXB + 1, "batch size"),       # hi - lo > max_batch
             (dev, MAXB, 5, 4, "rows"),                    # lo > hi
             (dev, MAXB, 0, MAXB + 1, "rows"),             # hi > n
             (dev, 1000, n - 1, n + 1, "rows"),
             (dev, MAXB, -1, 3, "rows"),
             (empty, MAXB, 0, None, "empty"),
             (host, MAXB, 0, None, "host-backed")]
    for buf, batch, lo, hi, msg in cases:
        with pytest.raises(L.AzError, match=msg):
            b.step_replay(buf, batch, 1, LR, lo, hi)
        with pytest.raises(L.AzError, match=msg):
            b.compute_grads_replay(buf, batch, 1, lo, hi)
    with pytest.raises(L.AzError, match="rows"):
        dev.sample_rows(MAXB, 1, lo=2, hi=MAXB + 1)
    with pytest.raises(L.AzError, match="host-backed"):
        host.sample_rows(MAXB, 1)
    assert b.params().tobytes() == before == a.params().tobytes()
    assert saved(dev, tmp_path / "after.bin") == file_before and len(empty) == 0
    assert b.step_replay(dev, MAXB, 1, LR) == a.step(*host.sample_arrays(MAXB, 1)[:3], LR)   # still in step
    same_trainers(a, b)


# ------------------------------------------------------------------ train() end to end
def test_train_with_device_replay_equals_host_replay(require_gpu, tmp_path):
    runs = []
    for on in (True, False):
        batches = []
        tr, rp, hist = train(2, blocks=B, filters=F, games=4, sims=8, min_replay=30, train_steps=2, batch_size=16,
                             seed=5, device_replay=on,
                             log_batch=lambda it, b, pl, po, va, lo, hi: batches.append((it, b, pl.tobytes(), po.tobytes(),
                                                                                        va.tobytes(), lo, hi)))
        assert (rp.device == 0) if on else (rp.device is None)
        hist = [{k: v for k, v in h.items() if k not in ("selfplay_s", "train_s")} for h in hist]
        runs.append((tr.params().tobytes(), saved(rp, tmp_path / ("replay%d.bin" % on)), hist, batches))
    assert runs[0][2] == runs[1][2]
    assert runs[0][3] == runs[1][3] and len(runs[0][3]) == 4
    assert runs[0][1] == runs[1][1]
    assert runs[0][0] == runs[1][0]
