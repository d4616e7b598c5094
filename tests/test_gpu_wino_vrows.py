"""tower32w_kernel<256> / k_sims32w<256> in the row-direct form with V in the shared-row layout (wino.h
wino_vr_*, AZ_WINO_VROWS=1: every D row of the padded board stored once) against the per-tile layout
(AZ_WINO_VROWS=0): the same bits reach the same products, so every output is bit-equal; and against the
oracle, the float64 reference and the f32-product kernel as the rows test.  Every test asserts which form
ran (AlphaZero.wino_v_rows)."""
import numpy as np
import pytest

import azchess as A
import netcases as N
import oracle as O
from test_gpu_net import check, random_planes
from test_gpu_split16 import close, scaled_input_conv
from test_gpu_wino_derive import PLAIN, SPLIT
from test_gpu_wino_rows import tower_inputs64
from test_netcases import get_case
from test_wino_derive import exact_planes, exact_weights

pytestmark = pytest.mark.gpu

VROWS_DEFAULT = 1     # az_internal.h AZ_WINO_VROWS_DEFAULT


def net_at(monkeypatch, vrows, blocks, w, rows=None, derive=None, split16=None):
    """a 256-filter f32 net created with AZ_WINO_VROWS=vrows, AZ_WINO_ROWS=rows, AZ_WINO_DERIVE=derive,
    AZ_WINO_SPLIT16=split16 (None: unset); the form it reports is asserted"""
    for name, v in (("AZ_WINO_VROWS", vrows), ("AZ_WINO_ROWS", rows), ("AZ_WINO_DERIVE", derive), ("AZ_WINO_SPLIT16", split16)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    net = A.AlphaZero(blocks, 256, weights=w, dtype="f32")
    if split16 == 0:
        assert net.tower_kernel == PLAIN and net.wino_accumulators == 0 and net.wino_v_rows == 0
    elif derive == 0 or rows == 0:
        assert net.tower_kernel == SPLIT and net.wino_accumulators == 16 and net.wino_v_rows == 0
    else:
        on = VROWS_DEFAULT if vrows is None else vrows
        assert net.tower_kernel == SPLIT and net.wino_accumulators == 8 and net.wino_v_rows == on
    return net


def both(monkeypatch, blocks, w, planes):
    """forward with the knob at 1 and at 0; asserts bit-equality and returns the outputs at 1"""
    p1, v1 = net_at(monkeypatch, 1, blocks, w).forward(planes)
    p0, v0 = net_at(monkeypatch, 0, blocks, w).forward(planes)
    assert np.array_equal(v1, v0), np.abs(v1 - v0).max()
    assert np.array_equal(p1, p0), np.abs(p1 - p0).max()
    return p1, v1


def test_knob_and_accessor(require_gpu, monkeypatch):
    """unset follows the compiled default; 0 and 1 report 0 and 1; the other forms report 0 whatever the knob
    says; 128 and 64 filters are unaffected"""
    w = A.random_weights(2, 256, seed=3)
    for vrows in (None, 0, 1):
        net_at(monkeypatch, vrows, 2, w)
        net_at(monkeypatch, vrows, 2, w, rows=1, derive=1)
        net_at(monkeypatch, vrows, 2, w, rows=0)
        net_at(monkeypatch, vrows, 2, w, derive=0)
        net_at(monkeypatch, vrows, 2, w, split16=0)
    monkeypatch.setenv("AZ_WINO_SPLIT16", "2")
    monkeypatch.setenv("AZ_WINO_DERIVE", "1")
    monkeypatch.setenv("AZ_WINO_ROWS", "1")
    monkeypatch.setenv("AZ_WINO_VROWS", "1")
    for blocks, filters in ((2, 128), (2, 64)):
        net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=3), dtype="f32")
        assert "split-f16 MFMA" in net.tower_kernel and net.wino_accumulators == 16 and net.wino_v_rows == 0


def test_bit_equal_random_weights_and_oracle(require_gpu, monkeypatch):
    w = A.random_weights(2, 256, seed=3)
    planes = random_planes(3, 13)
    pol, val = both(monkeypatch, 2, w, planes)
    rpol, rval = O.RefNet(2, 256, w).forward(planes)
    check(pol, val, rpol, rval, "f32")


@pytest.mark.parametrize("family", ["gamma5", "signed"])
def test_bit_equal_trained_like_weights(require_gpu, monkeypatch, family):
    """channel spread 2^+-5 / negative gamma (tests/netcases.py): bit-equal to the per-tile layout, within the
    project's tolerance of float64 and within M = 8 times the plain float32 evaluation's own error"""
    c = get_case(family, 2, 256, 5)
    pol, val = both(monkeypatch, 2, c.w, c.planes)
    ratios = N.measured_bound(pol, val, c, "f32-split16 rows, shared V rows", enforce=False)
    N.check_tolerance(pol, val, c, "f32")
    N.assert_measured(ratios, c)


def test_bit_equal_exact_arithmetic(require_gpu, monkeypatch):
    w = exact_weights(2, 256, 1)
    planes = exact_planes(4, 2)
    pol, val = both(monkeypatch, 2, w, planes)
    rpol, rval = N.forward64(2, 256, w, planes)
    check(pol, val, rpol, rval, "f32")
    assert np.unique(val).size == 4 and pol.max() > 2.0 / 4096     # not a dead net


def test_bit_equal_20_blocks(require_gpu, monkeypatch):
    """the ring, the zero rows and the pre-transform carried over 40 conv boundaries"""
    pol, val = both(monkeypatch, 20, A.random_weights(20, 256, seed=42), random_planes(3, 20256))
    assert np.isfinite(pol).all() and np.isfinite(val).all()


def test_batch_rows_are_independent(require_gpu, monkeypatch):
    """a row's outputs are bit-equal alone and inside a batch of 5"""
    net = net_at(monkeypatch, 1, 2, A.random_weights(2, 256, seed=5))
    planes = random_planes(5, 21)
    pb, vb = net.forward(planes)
    for r in (0, 3):
        p1, v1 = net.forward(planes[r:r + 1])
        assert np.array_equal(p1[0], pb[r]) and np.array_equal(v1[0], vb[r])


def test_overflow_reaches_the_outputs(require_gpu, monkeypatch):
    """the input conv scaled up 2^16 x: every policy entry and the value come out non-finite (the (inf, -inf)
    pair of split16 is stored as the per-tile layout stores it)"""
    w = scaled_input_conv(A.random_weights(2, 256, seed=3), 65536.0)
    pol, val = net_at(monkeypatch, 1, 2, w).forward(random_planes(3, 13))
    assert not np.isfinite(pol).any() and not np.isfinite(val).any()


def test_range_256_to_511(require_gpu, monkeypatch):
    """layer inputs between 256 and 511 (tests/test_gpu_wino_rows.py): finite, within the tolerance of the
    f32-product kernel's"""
    w0 = A.random_weights(2, 256, seed=3)
    planes = random_planes(3, 13)
    base = max(x.max() for x in tower_inputs64(2, w0, planes))
    w = scaled_input_conv(w0, 400.0 / base)
    assert 256 < max(float(x.max()) for x in tower_inputs64(2, w, planes)) < 511
    out = net_at(monkeypatch, 1, 2, w).forward(planes)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    close(out, net_at(monkeypatch, None, 2, w, split16=0).forward(planes))


def test_search_bit_equal(require_gpu, monkeypatch):
    """a 16-simulation search of 2 games through k_step + tower32w_kernel<256> and through the persistent
    k_sims32w<256>: bit-equal visits and improved policies, and bit-equal to the same search with the knob
    at 0"""
    w = A.random_weights(2, 256, seed=42)
    hist = [[], [588]]
    got = []
    for vrows in (1, 0):
        net = net_at(monkeypatch, vrows, 2, w)
        for persistent in (False, True):
            kw = dict(cache_capacity=0) if persistent else {}
            s = A.BatchedSearch(net, games=2, sims=16, seed=3, **kw)
            assert s.persistent == persistent
            s.set_roots(hist, apply_noise=True)
            imp, vis, dep = s.run()
            got.append((np.array(imp), np.array(vis)))
    assert got[0][1].sum() > 0
    for imp, vis in got[1:]:
        assert np.array_equal(vis, got[0][1]) and np.array_equal(imp, got[0][0])
