"""In-place weight updates (net_update.hip): az_net_update / az_net_update_from_trainer rebuild every
packed weight buffer of an existing net on the device.  Bar: BYTE IDENTITY with what az_net_create
builds from the same parameters on the host -- every buffer az_net_packed_read exposes, each conv's
split-f16 unscale, and a forward -- plus the searches' generation rule.

Nets have one or two blocks.  w1 is the random init; w2 is a trained-like family of tests/netcases.py on
another init: "var5" (per-channel powers of two moved through gamma and through the running variance,
conv outputs rescaled against running mean / variance) and "signed" (var5 with half of each block's
first BatchNorm gammas negated)."""
import ctypes as C
import functools

import numpy as np
import pytest

import azchess as A
import azchess._lib as L
import netcases as N
from test_gpu_net import random_planes
from test_gpu_search import histories

pytestmark = pytest.mark.gpu

HEADS = {"conv_w", "conv_b", "head", "head_frag", "head_frag32"}
WINO32 = HEADS | {"in_pk32", "wino_w"}
WINO16 = HEADS | {"in_pk32", "wino16_w", "wino16_us"}
FP8 = HEADS | {"w8", "w8s", "b8"}
# (dtype, blocks, filters, environment, the buffer kinds the net must hold, (streamed points, accumulators))
CASES = [
    ("f32", 2, 32, {}, HEADS, (0, 0)),
    ("f32", 2, 64, {}, WINO32, (0, 0)),
    ("f32", 1, 128, {}, WINO32, (0, 0)),
    ("f32", 2, 64, {"AZ_WINO_SPLIT16": "2"}, WINO16, (16, 16)),
    ("f32", 1, 128, {"AZ_WINO_SPLIT16": "2"}, WINO16, (16, 16)),
    ("f32", 1, 256, {}, WINO16, (12, 8)),
    ("f32", 1, 256, {"AZ_WINO_ROWS": "0"}, WINO16, (12, 16)),
    ("f32", 1, 256, {"AZ_WINO_DERIVE": "0"}, WINO16, (16, 16)),
    ("f32", 1, 256, {"AZ_WINO_SPLIT16": "0"}, WINO32, (0, 0)),
    ("f32", 1, 64, {"AZ_WINOGRAD": "0"}, WINO32, (0, 0)),
    ("bf16", 2, 64, {}, HEADS, (0, 0)),
    ("bf16", 1, 256, {}, HEADS, (0, 0)),
    ("fp8", 1, 128, {}, FP8, (0, 0)),
    ("fp8", 1, 256, {}, FP8, (0, 0)),
]
ENV_KNOBS = ("AZ_WINO_SPLIT16", "AZ_WINO_ROWS", "AZ_WINO_DERIVE", "AZ_WINOGRAD", "AZ_FUSED_TOWER")


def case_id(c):
    return "%s-%dx%d%s" % (c[0], c[1], c[2], "".join("-%s=%s" % (k[3:], v) for k, v in c[3].items()))


@functools.lru_cache(maxsize=None)
def w1(blocks, filters):
    w = A.random_weights(blocks, filters, seed=42)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def w2(blocks, filters, family="var5"):
    w = N.family_weights("var5", A.random_weights(blocks, filters, seed=77), blocks, filters)
    if family == "signed":
        w = N.family_weights("signed", w, blocks, filters)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def planes4():
    p = random_planes(4, 9100)
    p.setflags(write=False)
    return p


def set_env(monkeypatch, env):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def buffers(net):
    """{(kind, index): bytes} of every packed buffer the net holds"""
    out = {}
    for kind in L.PACKED_KINDS:
        for i in range(1 + 2 * net.blocks):
            b = net.packed(kind, i)
            if b is None:
                break
            out[(kind, i)] = b
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    bad = [k for k in a if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k])]
    detail = ["%s[%d]: %d of %d bytes differ, first at %d" % (k[0], k[1], int((a[k] != b[k]).sum()), a[k].size,
                                                            int(np.flatnonzero(a[k] != b[k])[0]))
              for k in bad if a[k].shape == b[k].shape]
    assert not bad, detail or bad


def assert_all_differ(a, b):
    """the precondition: before the update no buffer equals the target's (the unscales are powers of two
    that two weight sets can share per conv: at least one of them differs)"""
    assert a.keys() == b.keys()
    same = [k for k in a if k[0] != "wino16_us" and np.array_equal(a[k], b[k])]
    assert not same, same
    us = [k for k in a if k[0] == "wino16_us"]
    assert not us or any(not np.array_equal(a[k], b[k]) for k in us)


def same_forward(a, b):
    pa, va = a.forward(planes4())
    pb, vb = b.forward(planes4())
    assert np.isfinite(pa).all() and np.isfinite(va).all()
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))


def updated_equals_created(dtype, blocks, filters, wa, wb, kinds=None):
    ref = A.AlphaZero(blocks, filters, weights=wb, dtype=dtype)
    upd = A.AlphaZero(blocks, filters, weights=wa, dtype=dtype)
    rb = buffers(ref)
    if kinds is not None:
        assert {k for k, _ in rb} == kinds
    assert upd.generation == 0
    assert_all_differ(buffers(upd), rb)
    upd.update(wb)
    assert upd.generation == 1
    assert_same(buffers(upd), rb)
    same_forward(upd, ref)
    assert np.array_equal(upd.weights.view(np.uint32), np.asarray(wb).view(np.uint32))
    return ref, upd, rb


# ------------------------------------------------------------------ 1. byte identity per layout
@pytest.mark.parametrize("family", ["var5", "signed"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_update_matches_create_byte_for_byte(require_gpu, monkeypatch, case, family):
    dtype, blocks, filters, env, kinds, (streamed, accs) = case
    set_env(monkeypatch, env)
    ref, upd, _ = updated_equals_created(dtype, blocks, filters, w1(blocks, filters), w2(blocks, filters, family), kinds)
    assert upd.tower_kernel == ref.tower_kernel
    assert (upd.wino_streamed_points, upd.wino_accumulators) == (streamed, accs)


# ------------------------------------------------------------------ 2. edge values
def edge_weights(blocks, filters, edge):
    """w2 with: "zero+pow2" the block's first conv all zero (max |U| = 0) and its second conv zero but for
    one corner tap 0.5 behind an identity BatchNorm (max |U| = 0.5 exactly: a corner tap is its own
    Winograd point); "gamma0+block0" one output channel of the input conv and of both residual convs with
    gamma = 0 (folded weights +-0), and the weights of one (output channel, 32 input channels) block of
    each residual conv zero on every tap."""
    w = np.array(w2(blocks, filters), np.float32)
    V = N.views(w, blocks, filters)
    if edge == "zero+pow2":
        V["res_blocks.0.conv1.weight"][...] = 0.0
        c2 = V["res_blocks.0.conv2.weight"]
        c2[...] = 0.0
        c2[5, 9, 0, 0] = 0.5
        bn = V["res_blocks.0.bn2"]
        bn[0, 5], bn[3, 5] = 1.0, np.float32(1.0 - N.EPS)
        sc = np.float64(bn[0, 5]) / np.sqrt(np.float64(bn[3, 5]) + 1e-5)
        assert np.float32(np.float64(c2[5, 9, 0, 0]) * sc) == np.float32(0.5)     # the fold leaves the power of two
    else:
        for name in ("input_bn", "res_blocks.0.bn1", "res_blocks.0.bn2"):
            V[name][0, 3] = 0.0
        for name in ("res_blocks.0.conv1.weight", "res_blocks.0.conv2.weight"):
            V[name][7, 32:64] = 0.0
    return w


@pytest.mark.parametrize("edge", ["zero+pow2", "gamma0+block0"])
@pytest.mark.parametrize("dtype,blocks,filters,env", [("f32", 1, 64, {"AZ_WINO_SPLIT16": "2"}), ("fp8", 1, 128, {})],
                         ids=["f32-1x64-split16", "fp8-1x128"])
def test_update_edge_values(require_gpu, monkeypatch, dtype, blocks, filters, env, edge):
    set_env(monkeypatch, env)
    wb = edge_weights(blocks, filters, edge)
    _, upd, rb = updated_equals_created(dtype, blocks, filters, w1(blocks, filters), wb)
    if dtype == "f32" and edge == "zero+pow2":
        # the host's rule at max |U| = 0: Sw = 2^24; at 0.5 (frexp exponent 0): Sw = 2^15; Sa = 64
        us = [float(rb[("wino16_us", i)].view(np.float32)[0]) for i in range(2)]
        assert us == [2.0 ** -30, 2.0 ** -21]
        assert not rb[("wino16_w", 0)].any()


# ------------------------------------------------------------------ 3. from the trainer
@pytest.mark.parametrize("filters", [64, 256])
def test_update_from_trainer(require_gpu, monkeypatch, filters):
    set_env(monkeypatch, {})
    rng = np.random.default_rng(filters)
    tr = A.Trainer(1, filters, weights=w1(1, filters), max_batch=2)
    tpol = rng.random((2, 4096)).astype(np.float32)
    tpol /= tpol.sum(1, keepdims=True)
    tr.step(planes4()[:2], tpol, np.array([0.5, -0.25], np.float32), 1e-3)
    net = A.AlphaZero(1, filters, weights=w2(1, filters))
    assert net.update_from(tr) is net and net.generation == 1
    params = tr.params()
    assert not np.array_equal(params, w1(1, filters))              # the step moved them (running statistics too)
    ref = A.AlphaZero(1, filters, weights=params)
    assert_same(buffers(net), buffers(ref))
    same_forward(net, ref)
    assert np.array_equal(net.weights.view(np.uint32), params.view(np.uint32))
    # Trainer.model(into=) is the same path and returns the net it refreshed
    assert tr.model("f32", into=net) is net and net.generation == 2
    assert_same(buffers(net), buffers(ref))


def test_update_device_from_a_callers_buffer_and_stream(require_gpu, monkeypatch):
    """az_net_update_device itself: parameters in a caller's device buffer, on a caller's stream and on the
    net's own (NULL); a wrong count is refused before anything is written"""
    from azchess.hiprt import Hip
    set_env(monkeypatch, {})
    hip = Hip()
    ref = buffers(A.AlphaZero(2, 64, weights=w2(2, 64)))
    net = A.AlphaZero(2, 64, weights=w1(2, 64))
    first = buffers(net)
    d_w2, d_w1, st = hip.upload(np.array(w2(2, 64))), hip.upload(np.array(w1(2, 64))), hip.stream()
    try:
        assert L.lib.az_net_update_device(net._h, d_w2, w2(2, 64).size + 1, st) < 0
        assert net.generation == 0
        assert_same(buffers(net), first)
        L.check(L.lib.az_net_update_device(net._h, d_w2, w2(2, 64).size, st))
        assert net.generation == 1
        assert_same(buffers(net), ref)
        L.check(L.lib.az_net_update_device(net._h, d_w1, w1(2, 64).size, None))
        assert net.generation == 2
        assert_same(buffers(net), first)
    finally:
        hip.stream_destroy(st)
        hip.free(d_w2)
        hip.free(d_w1)


# ------------------------------------------------------------------ 4. two updates in a row
@pytest.mark.parametrize("dtype,blocks,filters", [("f32", 1, 256), ("f32", 2, 64), ("bf16", 2, 64), ("fp8", 1, 128)])
def test_two_updates_restore_the_first_bytes(require_gpu, monkeypatch, dtype, blocks, filters):
    set_env(monkeypatch, {})
    net = A.AlphaZero(blocks, filters, weights=w1(blocks, filters), dtype=dtype)
    first = buffers(net)
    net.update(w2(blocks, filters))
    assert_all_differ(buffers(net), first)
    net.update(w1(blocks, filters))
    assert net.generation == 2
    assert_same(buffers(net), first)                               # zero steps, zero k-steps, padded channels included
    assert np.array_equal(net.weights, w1(blocks, filters))


# ------------------------------------------------------------------ 5. error paths
def test_update_errors_change_nothing(require_gpu, monkeypatch):
    set_env(monkeypatch, {})
    net = A.AlphaZero(1, 64, weights=w1(1, 64))
    before = buffers(net)
    w = np.array(w2(1, 64))
    out = np.empty(w.size, np.float32)
    assert L.lib.az_net_get_weights(net._h, L.fptr(out), out.size) < 0
    assert "never updated" in L.lib.az_last_error().decode()
    assert L.lib.az_net_update(net._h, L.fptr(w), w.size - 1) < 0
    assert "count" in L.lib.az_last_error().decode()
    other = A.Trainer(1, 32, max_batch=1)
    with pytest.raises(L.AzError, match="1x32"):
        net.update_from(other)
    with pytest.raises(L.AzError):
        net.update(w[:-3])
    assert net.generation == 0
    assert_same(buffers(net), before)
    assert np.array_equal(net.weights, w1(1, 64))                  # still the creator's copy
    assert L.lib.az_net_packed_read(net._h, len(L.PACKED_KINDS), 0, None, 0) < 0
    small = np.empty(8, np.uint8)
    assert L.lib.az_net_packed_read(net._h, 0, 0, small.ctypes.data_as(C.c_void_p), small.size) < 0


# ------------------------------------------------------------------ 6. searches
def test_search_follows_the_update(require_gpu, monkeypatch):
    """(a) the batched path with a FEN cache: after the update, run refuses until the roots are set again,
    and the result is a fresh search's on a net created from w2 -- a cache kept from w1 would show."""
    set_env(monkeypatch, {})
    cfg = dict(games=4, sims=16, seed=3, cache_capacity=4096, noise=False)
    roots = histories(4, 31)
    net = A.AlphaZero(2, 64, weights=w1(2, 64))
    s = A.BatchedSearch(net, **cfg)
    assert not s.persistent
    s.set_roots(roots)
    old = s.run()
    net.update(w2(2, 64))
    with pytest.raises(L.AzError, match="weights changed.*set roots"):
        s.run()
    with pytest.raises(L.AzError, match="weights changed"):
        s.advance([0] * 4)
    s.read_roots()                                                 # reading still works
    s.set_roots(roots)
    new = s.run()
    fresh = A.BatchedSearch(A.AlphaZero(2, 64, weights=w2(2, 64)), **cfg)
    fresh.set_roots(roots)
    want = fresh.run()
    for a, b in zip(new, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(old[1], new[1])                      # the two nets do search differently


def test_persistent_selfplay_follows_the_update(require_gpu, monkeypatch):
    """(b) the persistent per-game kernel (cache off): step refuses after the update; after a reset, two
    moves equal a fresh SelfPlay's on the w2 net -- the drained steps, and after each move the re-rooted
    trees (root visits, improved policies, depths: they hang on the action each game played)."""
    set_env(monkeypatch, {})
    cfg = dict(games=4, sims=8, seed=11, cache_capacity=0)

    def two_moves(sp):
        out = []
        for _ in range(2):
            fin, act = sp.step()
            steps = [(s.game_id, s.ply, s.action, s.search_depth, s.result, s.visits) for s in sp.drain()]
            out.append((fin, act, steps) + tuple(x.copy() for x in sp.search.read_roots()))
        return out

    net = A.AlphaZero(2, 64, weights=w1(2, 64))
    sp = A.SelfPlay(net, **cfg)
    assert sp.search.persistent
    sp.reset()
    old = two_moves(sp)
    net.update(w2(2, 64))
    with pytest.raises(L.AzError, match="weights changed.*az_selfplay_reset"):
        sp.step()
    assert sp.drain() == []                                        # the drains still work
    sp.reset()
    new = two_moves(sp)
    fresh = A.SelfPlay(A.AlphaZero(2, 64, weights=w2(2, 64)), **cfg)
    fresh.reset()
    want = two_moves(fresh)
    differs = False
    for a, b, o in zip(new, want, old):
        assert a[:3] == b[:3]
        for x, y, z in zip(a[3:], b[3:], o[3:]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
            differs = differs or not np.array_equal(x, z)
    assert differs
