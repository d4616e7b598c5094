"""Every inference tower on trained-like weights (tests/netcases.py: channels of different
magnitude, BatchNorm folds with var and mean far from 1 and 0, negative gamma, a peaked softmax, a
tanh near +-1) against a float64 numpy reference, on 3-5 positions.

Bounds: the project's tolerances (test_gpu_net.check) for f32 and bf16; for f32 also the measured
bound: errors against float64 within M = 8 times those of a plain float32 evaluation of the same
case (netcases.measured_bound -- taken from the reference, never from a GPU result).  Every test
asserts which kernel ran and prints 'gpu error / yardstick error' (RATIO lines;
profiles/structured_weights_gpu.txt is that table from an MI355X)."""
import numpy as np
import pytest

import azchess as A
import netcases as N
from test_netcases import SEARCH_NETS, get_case, search_case, search_histories

pytestmark = pytest.mark.gpu

LAYERED = "conv3x3_kernel (per layer) + heads_kernel"
WINO = "tower32w_kernel<%d> (f32, Winograd F(2x2,3x3) residual convs)"
# path: (dtype, environment, kernel name, smallest filter count)
PATHS = {
    "f32-layer": ("f32", {"AZ_FUSED_TOWER": "0"}, LAYERED, 32),
    "f32-direct": ("f32", {"AZ_WINOGRAD": "0"}, "tower32_kernel<%d> (f32, direct 3x3)", 32),
    "f32-wino": ("f32", {"AZ_WINO_SPLIT16": "0"}, WINO, 64),
    "f32-split16": ("f32", {"AZ_WINO_SPLIT16": "2"}, WINO[:-1] + ", split-f16 MFMA products)", 64),
    "bf16-fused": ("bf16", {}, "tower_kernel<%d> (bf16, direct 3x3)", 32),
    "bf16-layer": ("bf16", {"AZ_FUSED_TOWER": "0"}, LAYERED, 32),
}


def make_net(monkeypatch, path, blocks, filters, w):
    dtype, env, name, _fmin = PATHS[path]
    for k in ("AZ_FUSED_TOWER", "AZ_WINOGRAD", "AZ_WINO_SPLIT16"):
        monkeypatch.delenv(k, raising=False)
    if not (path == "f32-split16" and filters == 256):      # split-f16 is the default at 256 filters
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    net = A.AlphaZero(blocks, filters, weights=w, dtype=dtype)
    want = name % filters if "%d" in name else name
    assert net.tower_kernel == want, (net.tower_kernel, want)
    return net


def shapes_for(path, shapes):
    return [s for s in shapes if s[1] >= PATHS[path][3]]


A_CASES = [(p, f) + s for p in PATHS for s in shapes_for(p, N.SMALL) for f in N.FAMILIES]
# the one 20x256 case: rescaled + peaked for f32; rescaled for bf16, whose format cannot hold its
# tolerance on peaked logits behind 41 stored layers (netcases.forward_bf16, a numpy restatement of the
# bf16 arithmetic, is at 2.4x the tolerance there: test_netcases.test_bf16_tolerance_is_satisfiable)
A_CASES += [(p, N.big_family(PATHS[p][0])) + N.BIG for p in PATHS]


@pytest.mark.parametrize("path,family,blocks,filters,rows", A_CASES)
def test_tower_matches_float64(require_gpu, monkeypatch, path, family, blocks, filters, rows):
    """test a: every path on every weight family"""
    c = get_case(family, blocks, filters, rows)
    net = make_net(monkeypatch, path, blocks, filters, c.w)
    pol, val = net.forward(c.planes)
    dtype = PATHS[path][0]
    ratios = N.measured_bound(pol, val, c, path, enforce=False)
    N.check_tolerance(pol, val, c, dtype)
    if dtype == "f32":
        N.assert_measured(ratios, c)


B_CASES = [(p,) + s for p in PATHS if p != "f32-split16" for s in shapes_for(p, N.SMALL)]


@pytest.mark.parametrize("path,blocks,filters,rows", B_CASES)
def test_power_of_two_channel_scales_change_no_bit(require_gpu, monkeypatch, path, blocks, filters, rows):
    """test b: with the scales moved through gamma and beta every weight changes by an exact power of
    two.  The BatchNorm fold is computed in double and rounded once, so the power passes through it
    exactly; f32 FMA chains, bf16 rounding and the heads' hi / lo bf16 split are scale invariant away
    from under- and overflow: the outputs are bit-equal to those on the init weights.  (Not the
    split-f16 path: its fixed Sa and per-conv Sw are not per channel -- test c.)"""
    c0 = get_case("base", blocks, filters, rows)
    c1 = get_case("gamma5", blocks, filters, rows)
    p0, v0 = make_net(monkeypatch, path, blocks, filters, c0.w).forward(c0.planes)
    p1, v1 = make_net(monkeypatch, path, blocks, filters, c1.w).forward(c1.planes)
    N.measured_bound(p1, v1, c1, path + " (=base)", enforce=False)
    assert np.array_equal(v0, v1), np.abs(v0 - v1).max()
    assert np.array_equal(p0, p1), (np.abs(p0 - p1) / p0).max()


C_CASES = [(k,) + s for s in N.SPLIT_SHAPES for k in (3, 5, 8)]


@pytest.mark.parametrize("spread,blocks,filters,rows", C_CASES)
def test_split16_channel_spread(require_gpu, monkeypatch, spread, blocks, filters, rows):
    """test c: the split-f16 point GEMMs scale every activation by one Sa = 64 and a conv's weights by
    one Sw.  Channel exponents in [-3, 3] and [-5, 5] keep the activations inside the documented
    |x| < 255.8 and x1/32: the measured bound holds.  Spread 8 draws from [-8, 4], below the
    documented range: the project's tolerance and finite outputs only; its ratio is a measurement."""
    c = get_case("gamma%d" % spread, blocks, filters, rows)
    net = make_net(monkeypatch, "f32-split16", blocks, filters, c.w)
    pol, val = net.forward(c.planes)
    ratios = N.measured_bound(pol, val, c, "f32-split16", enforce=False)
    N.check_tolerance(pol, val, c, "f32")
    if spread <= 5:
        N.assert_measured(ratios, c)


def search_log(net, hs, persistent):
    kw = dict(cache_capacity=0) if persistent else {}
    s = A.BatchedSearch(net, games=len(hs), sims=3, seed=4, record_evals=True, eval_log_cap=1024, **kw)
    assert s.persistent == persistent
    s.set_roots(hs, apply_noise=False)
    s.run()
    keys, vals, off, idx, pri = s.eval_log()
    log = {}
    for r in range(len(keys)):
        row = (np.float32(vals[r]), idx[off[r]:off[r + 1]].copy(), pri[off[r]:off[r + 1]].copy())
        prev = log.setdefault(int(keys[r]), row)    # a position evaluated twice: the same bits
        assert prev[0] == row[0] and np.array_equal(prev[1], row[1]) and np.array_equal(prev[2], row[2])
    return log


@pytest.mark.parametrize("blocks,filters", SEARCH_NETS)
def test_search_mode_rows_match_float64(require_gpu, monkeypatch, blocks, filters):
    """test d: the heads in search mode (priors written at the legal indices of the new nodes) on
    rescaled + peaked weights, as k_step + tower32w_kernel per step and as the persistent k_sims32w
    (split-f16 towers): the logged rows of the roots and their children against float64 with the
    bounds of test a; the two modes bit-equal."""
    c, row_of, pos = search_case(blocks, filters)
    hs = search_histories()
    net = make_net(monkeypatch, "f32-split16", blocks, filters, c.w)
    logs = [search_log(net, hs, persistent) for persistent in (False, True)]
    assert sorted(logs[0]) == sorted(logs[1])
    for k, (v, ii, pr) in logs[0].items():
        v2, ii2, pr2 = logs[1][k]
        assert v == v2 and np.array_equal(ii, ii2) and np.array_equal(pr, pr2)
    roots = set()
    for h in hs:
        p = A.Position.startpos()
        for a in h:
            p = p.play(a)
        roots.add(p.fen_key())
    assert roots <= set(logs[0])
    known = [k for k in logs[0] if k in row_of]
    assert len(known) >= 2 * len(roots)      # every root and the child its first simulation expands
    ev = ep = yv = yp = 0.0
    tiny = 0
    for k in known:
        v, ii, pr = logs[0][k]
        r = row_of[k]
        assert set(ii.tolist()) == set(pos[k].legal_indices().tolist())
        ref, yard = c.pol[r][ii], c.ypol[r][ii]
        assert np.isfinite(v) and np.isfinite(pr).all() and np.all(pr >= 0)
        assert abs(float(v) - c.val[r]) <= 1e-5
        assert np.all(np.abs(pr - ref) <= 1e-4 * ref + 1e-8)      # entries below 1e-8: the absolute term
        big = ref >= 1e-8
        tiny += int((~big).sum())
        ev, yv = max(ev, abs(float(v) - c.val[r])), max(yv, abs(float(c.yval[r]) - c.val[r]))
        if big.any():
            ep = max(ep, (np.abs(pr - ref)[big] / ref[big]).max())
            yp = max(yp, (np.abs(yard - ref)[big] / ref[big]).max())
    assert tiny > 0
    print("RATIO %-22s %-14s %2dx%-3d value %9.3f  policy %9.3f   (yardstick value %.2e policy %.2e; %d rows)"
          % ("f32-split16 search", c.family, blocks, filters, ev / yv, ep / yp, yv, yp, len(known)))
    assert ev <= N.M * yv and ep <= N.M * yp


@pytest.mark.parametrize("path", ["f32-split16", "bf16-fused"])
@pytest.mark.parametrize("blocks,filters", [(6, 64), (2, 256)])
def test_rows_are_independent(require_gpu, monkeypatch, path, blocks, filters):
    """test e: rows 0 and 3 of a batch of 5 alone, bit for bit, on rescaled + peaked weights"""
    c = get_case("gamma5+peaked", blocks, filters, 5)    # both among netcases.SMALL
    net = make_net(monkeypatch, path, blocks, filters, c.w)
    pb, vb = net.forward(c.planes)
    N.measured_bound(pb, vb, c, path + " batch", enforce=False)
    N.check_tolerance(pb, vb, c, PATHS[path][0])
    for r in (0, 3):
        p1, v1 = net.forward(c.planes[r:r + 1])
        assert np.array_equal(p1[0], pb[r]) and np.array_equal(v1[0], vb[r])
