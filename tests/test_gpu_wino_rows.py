"""tower32w_kernel<256> / k_sims32w<256> in the row-direct form (wino.h wino_core_h16<256, 12, true>,
AZ_WINO_ROWS): Winograd across columns only, the three tap rows summed directly into 8 accumulators
per output fragment, against the derived-row form (AZ_WINO_ROWS=0), the 16-point stream
(AZ_WINO_DERIVE=0), the f32 products (AZ_WINO_SPLIT16=0) and the oracle on the same weights.
Tolerances are the project's f32 ones (value atol 1e-5; policy rtol 1e-4, atol 1e-8); every test
asserts which form ran."""
import numpy as np
import pytest

import azchess as A
import netcases as N
import oracle as O
from test_gpu_net import check, random_planes
from test_gpu_split16 import close, scaled_input_conv
from test_gpu_wino_derive import PLAIN, SPLIT
from test_netcases import get_case
from test_wino_derive import exact_planes, exact_weights

pytestmark = pytest.mark.gpu

ROWS_DEFAULT = 1      # az_internal.h AZ_WINO_ROWS_DEFAULT


def net_at(monkeypatch, rows, blocks, w, derive=None, split16=None):
    """a 256-filter f32 net created with AZ_WINO_ROWS=rows, AZ_WINO_DERIVE=derive, AZ_WINO_SPLIT16=split16
    (None: unset); which kernel, how many streamed points and how many accumulators it reports are
    asserted"""
    for name, v in (("AZ_WINO_ROWS", rows), ("AZ_WINO_DERIVE", derive), ("AZ_WINO_SPLIT16", split16)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    net = A.AlphaZero(blocks, 256, weights=w, dtype="f32")
    if split16 == 0:
        assert net.tower_kernel == PLAIN and net.wino_streamed_points == 0 and net.wino_accumulators == 0
    elif derive == 0:
        assert net.tower_kernel == SPLIT and net.wino_streamed_points == 16 and net.wino_accumulators == 16
    else:
        on = ROWS_DEFAULT if rows is None else rows
        assert net.tower_kernel == SPLIT, net.tower_kernel
        assert net.wino_streamed_points == 12 and net.wino_accumulators == (8 if on else 16)
    return net


def test_knob_and_accessor(require_gpu, monkeypatch):
    """unset follows the compiled default; 1: 8 accumulators; 0: 16 with 12 streamed; AZ_WINO_DERIVE=0: 16
    streamed at any AZ_WINO_ROWS; the kernel name does not change; 128 and 64 filters are unaffected"""
    w = A.random_weights(2, 256, seed=3)
    for rows in (None, 1, 0):
        net_at(monkeypatch, rows, 2, w)
        net_at(monkeypatch, rows, 2, w, derive=1)
        net_at(monkeypatch, rows, 2, w, derive=0)
    net_at(monkeypatch, 1, 2, w, split16=0)
    monkeypatch.setenv("AZ_WINO_SPLIT16", "2")
    monkeypatch.setenv("AZ_WINO_DERIVE", "1")
    monkeypatch.setenv("AZ_WINO_ROWS", "1")
    for blocks, filters in ((2, 128), (2, 64)):
        net = A.AlphaZero(blocks, filters, weights=A.random_weights(blocks, filters, seed=3), dtype="f32")
        assert "split-f16 MFMA" in net.tower_kernel and net.wino_streamed_points == 16 and net.wino_accumulators == 16


def test_rows_match_f32_products(require_gpu, monkeypatch):
    w = A.random_weights(2, 256, seed=3)
    planes = random_planes(3, 13)
    close(net_at(monkeypatch, 1, 2, w).forward(planes), net_at(monkeypatch, None, 2, w, split16=0).forward(planes))


def test_rows_match_oracle_20_blocks(require_gpu, monkeypatch):
    """the ring carried across 40 conv boundaries of 96 steps each"""
    w = A.random_weights(20, 256, seed=42)
    planes = random_planes(6, 20256)
    pol, val = net_at(monkeypatch, 1, 20, w).forward(planes)
    rpol, rval = O.RefNet(20, 256, w).forward(planes, threads=16)
    check(pol, val, rpol, rval, "f32")


def test_exact_arithmetic_is_bit_equal(require_gpu, monkeypatch):
    """On weights and inputs whose every product and sum is exact (tests/test_wino_derive.py
    exact_weights) the grouping of the sums cannot matter: the row-direct form, the derived-row form,
    the 16-point stream and the f32 products give the same bits.  A wrong plane, window slot or step
    order changes the sums."""
    w = exact_weights(2, 256, 1)
    planes = exact_planes(4, 2)
    outs = [net_at(monkeypatch, 1, 2, w).forward(planes), net_at(monkeypatch, 0, 2, w).forward(planes),
            net_at(monkeypatch, 1, 2, w, derive=0).forward(planes), net_at(monkeypatch, None, 2, w, split16=0).forward(planes)]
    rpol, rval = N.forward64(2, 256, w, planes)
    check(outs[0][0], outs[0][1], rpol, rval, "f32")
    assert np.unique(outs[0][1]).size == 4 and outs[0][0].max() > 2.0 / 4096     # not a dead net
    for pol, val in outs[1:]:
        assert np.array_equal(val, outs[0][1]), np.abs(val - outs[0][1]).max()
        assert np.array_equal(pol, outs[0][0]), np.abs(pol - outs[0][0]).max()


@pytest.mark.parametrize("family", ["gamma5", "signed"])
def test_rows_on_trained_like_weights(require_gpu, monkeypatch, family):
    """channel spread 2^+-5 / negative gamma (tests/netcases.py) against float64: the project's
    tolerance and the yardstick rule (within M = 8 times the plain float32 evaluation's own error)"""
    c = get_case(family, 2, 256, 5)
    pol, val = net_at(monkeypatch, 1, 2, c.w).forward(c.planes)
    ratios = N.measured_bound(pol, val, c, "f32-split16 rows", enforce=False)
    N.check_tolerance(pol, val, c, "f32")
    N.assert_measured(ratios, c)


def test_rows_batch_rows_are_independent(require_gpu, monkeypatch):
    """a row's outputs are bit-equal alone and inside a batch of 5"""
    net = net_at(monkeypatch, 1, 2, A.random_weights(2, 256, seed=5))
    planes = random_planes(5, 21)
    pb, vb = net.forward(planes)
    for r in (0, 3):
        p1, v1 = net.forward(planes[r:r + 1])
        assert np.array_equal(p1[0], pb[r]) and np.array_equal(v1[0], vb[r])


def test_rows_overflow_reaches_the_outputs(require_gpu, monkeypatch):
    """the input conv scaled up 2^16 x: every policy entry and the value come out non-finite"""
    w = scaled_input_conv(A.random_weights(2, 256, seed=3), 65536.0)
    pol, val = net_at(monkeypatch, 1, 2, w).forward(random_planes(3, 13))
    assert not np.isfinite(pol).any() and not np.isfinite(val).any()


def tower_inputs64(blocks, w, planes):
    """the inputs of every residual conv [layer][rows, 8, 8, 256] in float64 (BatchNorm inference as
    netcases.forward64)"""
    W = N.views(np.asarray(w).astype(np.float64), blocks, 256)

    def conv_bn(x, conv, bn):
        n, c = x.shape[0], x.shape[3]
        xp = np.zeros((n, 10, 10, c))
        xp[:, 1:9, 1:9] = x
        cols = np.stack([xp[:, i:i + 8, j:j + 8, :] for i in range(3) for j in range(3)], axis=3).reshape(n * 64, 9 * c)
        y = (cols @ W[conv + ".weight"].transpose(2, 3, 1, 0).reshape(9 * c, -1)).reshape(n, 8, 8, -1) + W[conv + ".bias"]
        g, b, m, v = W[bn]
        return (y - m) / np.sqrt(v + N.EPS) * g + b

    ins = []
    x = np.maximum(conv_bn(planes.transpose(0, 2, 3, 1).astype(np.float64), "input_conv", "input_bn"), 0)
    for b in range(blocks):
        ins.append(x)
        h = np.maximum(conv_bn(x, "res_blocks.%d.conv1" % b, "res_blocks.%d.bn1" % b), 0)
        ins.append(h)
        x = np.maximum(conv_bn(h, "res_blocks.%d.conv2" % b, "res_blocks.%d.bn2" % b) + x, 0)
    return ins


def test_rows_new_range_256_to_511(require_gpu, monkeypatch):
    """|D| <= 2 |x|: layer inputs up to 65504 / (2 x 64) = 511.7 stay in the f16 range (255.8 in the
    16-point forms, where |V| <= 4 |x|).  The input conv is scaled so that the largest layer input,
    computed in float64 on the CPU first, lies between 256 and 511; the outputs are finite and within
    the tolerance of the f32-product kernel's."""
    w0 = A.random_weights(2, 256, seed=3)
    planes = random_planes(3, 13)
    base = max(x.max() for x in tower_inputs64(2, w0, planes))
    w = scaled_input_conv(w0, 400.0 / base)
    peaks = [float(x.max()) for x in tower_inputs64(2, w, planes)]
    print("largest input of each residual conv: " + " ".join("%.1f" % p for p in peaks))
    assert 256 < max(peaks) < 511
    out = net_at(monkeypatch, 1, 2, w).forward(planes)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    close(out, net_at(monkeypatch, None, 2, w, split16=0).forward(planes))


def test_rows_search_replayed_by_oracle(require_gpu, monkeypatch):
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
