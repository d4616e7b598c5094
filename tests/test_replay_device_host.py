"""The device-aware replay entry points on a machine without a GPU: az_replay_create_on / load_on with
AZ_DEVICE_HOST are the host buffer, a device that az_device_count does not list is refused with a
message, and the device-only calls (az_replay_sample_rows, az_trainer_*_replay) refuse a host-backed
handle before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import azchess as A
from azchess import _lib as L
from azchess.memory import ReplayBuffer

HOST = -1                            # AZ_DEVICE_HOST


def positions(n, seed):
    """Positions from random playouts, with repeats (tests/test_replay.py's generator)."""
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


def raw_step(pos, rng):
    st = L.AzEpisodeStep()
    st.state = pos._p
    st.final_value = float(np.float32(rng.uniform(-1, 1)))
    idx = pos.legal_indices()
    st.nvis = len(idx)
    for i, ix in enumerate(idx):
        st.vis_idx[i], st.vis_n[i] = int(ix), int(rng.integers(0, 50))
    return st


def create_on(capacity, device):
    h = C.c_void_p()
    rc = L.lib.az_replay_create_on(capacity, device, C.byref(h))
    return rc, h


def same_samples(a, b, batch, seed):
    pa, qa, va, sa = a.sample_arrays(batch, seed)
    pb, qb, vb, sb = b.sample_arrays(batch, seed)
    assert pa.tobytes() == pb.tobytes() and qa.tobytes() == qb.tobytes() and va.tobytes() == vb.tobytes()
    assert [s.fen() for s in sa] == [s.fen() for s in sb]


def test_create_on_host_is_the_host_buffer(tmp_path):
    rc, h = create_on(8, HOST)
    assert rc == 0 and h.value
    on = ReplayBuffer(8, _handle=h)
    ref = ReplayBuffer(8)
    assert on.device is None and L.lib.az_replay_device(on._h) == HOST == L.lib.az_replay_device(ref._h)
    rng = np.random.default_rng(0)
    ps = positions(60, 1)
    for i, pos in enumerate(ps):                 # merges (repeats) and evictions (capacity 8)
        st = raw_step(pos, rng) if i % 2 else step(pos, rng)
        assert on.add(st) == ref.add(st)
    arr = (L.AzEpisodeStep * 10)(*[raw_step(p, rng) for p in ps[:10]])
    assert on.add_many(arr) == ref.add_many(arr)
    assert len(on) == len(ref) == 8
    for seed in (0, 5):
        same_samples(on, ref, 1000, seed)
        same_samples(on, ref, 3, seed)
    on.save(tmp_path / "a")
    ref.save(tmp_path / "b")
    raw = (tmp_path / "a").read_bytes()
    assert raw == (tmp_path / "b").read_bytes()
    back = ReplayBuffer.load(tmp_path / "a", 8, device=None)
    h2 = C.c_void_p()
    assert L.lib.az_replay_load_on(str(tmp_path / "a").encode(), 8, HOST, C.byref(h2)) == 0
    back_on = ReplayBuffer(8, _handle=h2)
    assert back_on.device is None
    same_samples(back, back_on, 1000, 2)
    back_on.save(tmp_path / "c")
    assert (tmp_path / "c").read_bytes() == raw


def test_create_on_a_device_that_is_not_listed_fails_with_a_message():
    n = C.c_int(-1)
    assert L.lib.az_device_count(C.byref(n)) == 0 and n.value >= 0
    for dev in (n.value, n.value + 7, -2):
        rc, h = create_on(8, dev)
        assert rc < 0 and not h.value
        assert b"az_replay_create_on" in L.lib.az_last_error()
    with pytest.raises(L.AzError, match="az_replay_create_on"):
        ReplayBuffer(8, device=n.value)
    rc, h = create_on(0, HOST)
    assert rc < 0 and not h.value


def test_load_on_a_device_that_is_not_listed_fails(tmp_path):
    buf = ReplayBuffer(4)
    rng = np.random.default_rng(3)
    for pos in positions(6, 4):
        buf.add(step(pos, rng))
    buf.save(tmp_path / "r")
    n = C.c_int(0)
    L.lib.az_device_count(C.byref(n))
    with pytest.raises(L.AzError, match="az_replay_create_on"):
        ReplayBuffer.load(tmp_path / "r", 4, device=n.value)
    with pytest.raises(L.AzError):
        ReplayBuffer.load(tmp_path / "missing", 4, device=n.value)


def test_device_only_calls_refuse_a_host_backed_buffer():
    buf = ReplayBuffer(8)
    rng = np.random.default_rng(5)
    for pos in positions(12, 6):
        buf.add(step(pos, rng))
    with pytest.raises(L.AzError, match="host-backed"):
        buf.sample_rows(4, 0, planes=0, policy=0, value=0)
    # the trainer calls look at the buffer first, so the refusal shows without a trainer (which needs a
    # GPU); tests/test_gpu_replay_device.py repeats it with a real one
    loss = np.zeros(2, np.float32)
    assert L.lib.az_trainer_step_replay(None, buf._h, 4, 0, 0, -1, 1e-3, L.fptr(loss), None) < 0
    assert b"host-backed" in L.lib.az_last_error()
    L.lib.az_last_error()
    assert L.lib.az_trainer_compute_grads_replay(None, buf._h, 4, 0, 0, -1, L.fptr(loss), None) < 0
    assert b"host-backed" in L.lib.az_last_error()
    assert len(buf) > 0 and buf.device is None
