"""tower32w_kernel<256> / k_sims32w<256> with 12 of the 16 Winograd points' weights streamed and the
third row of points derived from the other three (wino.h wino_core_h16<256, 12>, AZ_WINO_DERIVE),
against the 16-point stream (AZ_WINO_DERIVE=0) and the f32 products (AZ_WINO_SPLIT16=0) on the same
weights.  Tolerances are the project's f32 ones (value atol 1e-5; policy rtol 1e-4, atol 1e-8); every
test asserts which variant ran."""
import numpy as np
import pytest

import azchess as A
import netcases as N
import oracle as O
from test_gpu_net import check, random_planes
from test_gpu_split16 import close, scaled_input_conv
from test_netcases import get_case
from test_wino_derive import exact_planes, exact_weights

pytestmark = pytest.mark.gpu

PLAIN = "tower32w_kernel<256> (f32, Winograd F(2x2,3x3) residual convs)"
SPLIT = PLAIN[:-1] + ", split-f16 MFMA products)"


def net_at(monkeypatch, derive, blocks, w, split16=None):
    """a 256-filter f32 net created with AZ_WINO_DERIVE=derive (None: unset); which kernel and how
    many streamed points it reports are asserted"""
    for name, v in (("AZ_WINO_DERIVE", derive), ("AZ_WINO_SPLIT16", split16)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    net = A.AlphaZero(blocks, 256, weights=w, dtype="f32")
    if split16 == 0:
        assert net.tower_kernel == PLAIN and net.wino_streamed_points == 0
    else:
        assert net.tower_kernel == SPLIT, net.tower_kernel
        assert net.wino_streamed_points == (16 if derive == 0 else 12)
    return net


def test_knob_and_accessor(require_gpu, monkeypatch):
    """12 points unset or at 1, 16 at 0; 128 and 64 filters stream 16 at any value; the kernel name does
    not change"""
    w = A.random_weights(2, 256, seed=3)
    for derive in (None, 1, 0):
        net_at(monkeypatch, derive, 2, w)
    net_at(monkeypatch, 1, 2, w, split16=0)
    monkeypatch.setenv("AZ_WINO_SPLIT16", "2")
    monkeypatch.setenv("AZ_WINO_DERIVE", "1")
    for blocks, filters in ((2, 128), (2, 64)):
        net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=3), dtype="f32")
        assert "split-f16 MFMA" in net.tower_kernel and net.wino_streamed_points == 16


def test_derive_matches_f32_products(require_gpu, monkeypatch):
    w = A.random_weights(2, 256, seed=3)
    planes = random_planes(3, 13)
    close(net_at(monkeypatch, 1, 2, w).forward(planes), net_at(monkeypatch, None, 2, w, split16=0).forward(planes))


def test_derive_matches_oracle_20_blocks(require_gpu, monkeypatch):
    """the ring carried across 40 convs of 96 steps each"""
    w = A.random_weights(20, 256, seed=42)
    planes = random_planes(6, 20256)
    pol, val = net_at(monkeypatch, 1, 20, w).forward(planes)
    rpol, rval = O.RefNet(20, 256, w).forward(planes, threads=16)
    check(pol, val, rpol, rval, "f32")


def test_exact_arithmetic_is_bit_equal(require_gpu, monkeypatch):
    """On weights and inputs whose every product and sum is exact (tests/test_wino_derive.py
    exact_weights) the grouping of the sums cannot matter: 12 streamed points, 16 streamed points and
    f32 products give the same bits.  A wrong sign, point order or refill offset changes the sums."""
    w = exact_weights(2, 256, 1)
    planes = exact_planes(4, 2)
    outs = [net_at(monkeypatch, 1, 2, w).forward(planes), net_at(monkeypatch, 0, 2, w).forward(planes),
            net_at(monkeypatch, None, 2, w, split16=0).forward(planes)]
    rpol, rval = N.forward64(2, 256, w, planes)
    check(outs[0][0], outs[0][1], rpol, rval, "f32")
    assert np.unique(outs[0][1]).size == 4 and outs[0][0].max() > 2.0 / 4096     # not a dead net
    for pol, val in outs[1:]:
        assert np.array_equal(val, outs[0][1]), np.abs(val - outs[0][1]).max()
        assert np.array_equal(pol, outs[0][0]), np.abs(pol - outs[0][0]).max()


@pytest.mark.parametrize("family", ["gamma5", "signed"])
def test_derive_on_trained_like_weights(require_gpu, monkeypatch, family):
    """channel spread 2^+-5 / negative gamma (tests/netcases.py) against float64: the project's
    tolerance and the yardstick rule (within M = 8 times the plain float32 evaluation's own error)"""
    c = get_case(family, 2, 256, 5)
    pol, val = net_at(monkeypatch, 1, 2, c.w).forward(c.planes)
    ratios = N.measured_bound(pol, val, c, "f32-split16 derive", enforce=False)
    N.check_tolerance(pol, val, c, "f32")
    N.assert_measured(ratios, c)


def test_derive_rows_are_independent(require_gpu, monkeypatch):
    """a row's outputs are bit-equal alone and inside a batch of 5"""
    net = net_at(monkeypatch, 1, 2, A.random_weights(2, 256, seed=5))
    planes = random_planes(5, 21)
    pb, vb = net.forward(planes)
    for r in (0, 3):
        p1, v1 = net.forward(planes[r:r + 1])
        assert np.array_equal(p1[0], pb[r]) and np.array_equal(v1[0], vb[r])


def test_derive_overflow_reaches_the_outputs(require_gpu, monkeypatch):
    """the input conv scaled up 2^16 x: every policy entry and the value come out non-finite"""
    w = scaled_input_conv(A.random_weights(2, 256, seed=3), 65536.0)
    pol, val = net_at(monkeypatch, 1, 2, w).forward(random_planes(3, 13))
    assert not np.isfinite(pol).any() and not np.isfinite(val).any()


def test_derive_search_replayed_by_oracle(require_gpu, monkeypatch):
    """a 16-simulation search of 2 games replayed bit-exactly by the oracle from the GPU's evaluation
    log, with k_step + tower32w_kernel<256> and with the persistent k_sims32w<256> (evaluation cache
    off); the two run the same tower: bit-equal visits and improved policies"""
    net = net_at(monkeypatch, 1, 2, A.random_weights(2, 256, seed=42))
    hist = [[], [588]]
    cfg = O.make_cfg(sims=16, noise=True, seed=3, eval_kind=2)
    got = []
    for persistent in (False, True):
        kw = dict(cache_capacity=0) if persistent else {}
        s = A.BatchedSearch(net, games=2, sims=16, seed=3, record_evals=True, eval_log_cap=4096, **kw)
        assert s.persistent == persistent
        s.set_roots(hist, apply_noise=True)
        imp, vis, dep = s.run()
        rep = O.Replay(*s.eval_log())
        for g, h in enumerate(hist):
            rv, _, rd, _ = O.search_game(cfg, h, noise=True, noise_key=O.lib().ref_stream_key(3, g, len(h), 0), replay=rep)
            assert np.array_equal(vis[g].astype(np.float32), rv) and dep[g] == rd
        got.append((np.array(imp), np.array(vis)))
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[1][0])
