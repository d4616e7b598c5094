"""tests/netcases.py on the CPU: the numpy forward against the torch golden vectors, the
reparametrisations against the function they must preserve, and the float32 yardstick against the
project's tolerances on every case of tests/test_gpu_net_structured.py (the condition that makes
those tolerances satisfiable by a plain f32 evaluation, with room for a correct kernel)."""
import os

import numpy as np
import pytest

import azchess as A
import netcases as N
from azchess.agent import param_shapes
from conftest import ROOT
from test_gpu_net import random_planes


def base_of(blocks, filters):
    return A.random_weights(blocks, filters, seed=42)


def planes_of(rows, blocks, filters):
    return random_planes(rows, N.PLANES_SEED[blocks, filters])


def get_case(family, blocks, filters, rows):
    return N.case(family, blocks, filters, rows, base_of, planes_of)


GPU_CASES = N.gpu_cases()
SEARCH_NETS = [(6, 64), (2, 256)]     # rescaled + peaked, tests/test_gpu_net_structured.py (search mode)


def search_histories(games=4, seed=31):
    """short random histories that end in a position with legal moves"""
    rng = np.random.default_rng(seed)
    hs = []
    while len(hs) < games:
        gs, h = A.GameState(), []
        for _ in range(int(rng.integers(0, 12))):
            a = int(rng.choice(gs.position.legal_indices()))
            if int(A.play_move(gs, a)) != 0:
                break
            h.append(a)
        else:
            if len(gs.position.legal_indices()):
                hs.append(h)
    return hs


def search_positions(hs):
    """{fen key: Position} of the roots and of their children: the rows a 3-simulation search evaluates
    (deeper leaves are not looked up), as test_gpu_net.test_headline_net_many_positions_and_search_rows"""
    pos = {}
    for h in hs:
        p = A.Position.startpos()
        for a in h:
            p = p.play(a)
        pos.setdefault(p.fen_key(), p)
        for i in np.unique(p.legal_indices()):
            q = p.play(int(i))
            pos.setdefault(q.fen_key(), q)
    return pos


def search_case(blocks, filters):
    """the rescaled + peaked Case of a search net on the roots and children of search_histories()"""
    pos = search_positions(search_histories())
    keys = sorted(pos)
    planes_fn = lambda _rows, _blocks, _filters: np.concatenate([A.to_tensor(pos[k]) for k in keys])
    c = N.case("gamma5+peaked", blocks, filters, "search", base_of, planes_fn)
    return c, {k: i for i, k in enumerate(keys)}, pos


def test_layout_is_param_shapes():
    for blocks, filters in ((0, 32), (2, 32), (3, 64)):
        lay = N.layout(blocks, filters)
        p = 0
        for name, shape, _fan in param_shapes(blocks, filters):
            assert lay[name] == (p, shape), name
            p += int(np.prod(shape))
        assert lay["__size__"][0] == p == A.num_params(blocks, filters)


def test_forward64_matches_torch_golden():
    """the fixture is float64 torch output stored as float32: agreement to float32 rounding"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "net_2x32.npz"))
    pol, val = N.forward64(int(g["blocks"]), int(g["filters"]), g["weights"], g["planes"])
    assert pol.shape == g["policy"].shape and val.shape == g["value"].shape
    np.testing.assert_allclose(pol, g["policy"], rtol=2.0 ** -23, atol=0)
    np.testing.assert_allclose(val, g["value"], rtol=2.0 ** -23, atol=2.0 ** -30)
    ypol, yval = N.forward64(int(g["blocks"]), int(g["filters"]), g["weights"], g["planes"], np.float32)
    assert ypol.dtype == np.float32 and N.tolerance_use(ypol, yval, pol, val) <= 0.25


@pytest.mark.parametrize("through,spread", [("gamma", 5), ("var", 5), ("gamma", (-8, 4))])
@pytest.mark.parametrize("blocks,filters", [(2, 32), (3, 64)])
def test_channel_rescaled_preserves_the_function(blocks, filters, through, spread):
    w = base_of(blocks, filters)
    planes = random_planes(3, 7000 + filters)
    r = N.channel_rescaled(w, blocks, filters, spread, seed=5, through=through)
    assert r.dtype == np.float32 and r.shape == w.shape
    pol, val = N.forward64(blocks, filters, w, planes)
    rpol, rval = N.forward64(blocks, filters, r, planes)
    assert np.abs(rpol / pol - 1).max() <= 1e-6 and np.abs(rval - val).max() <= 1e-6
    # ... and is not the identity: BatchNorm scales differ by the drawn powers of two
    V0, V1 = N.views(w, blocks, filters), N.views(r, blocks, filters)
    sc = lambda bn: bn[0] / np.sqrt(bn[3].astype(np.float64) + N.EPS)
    k = np.log2(sc(V1["input_bn"]) / sc(V0["input_bn"]))
    hi = spread if np.isscalar(spread) else max(spread)
    lo = -spread if np.isscalar(spread) else min(spread)
    assert np.allclose(k, np.round(k), atol=1e-6) and k.min() <= lo + 1 and k.max() >= hi - 1
    if through == "var":
        var = np.concatenate([V1[n][3] for n in V1 if n.endswith("bn") or ".bn" in n])
        mean = np.concatenate([V1[n][2] for n in V1 if n.endswith("bn") or ".bn" in n])
        assert var.min() > 0 and var.min() < 1e-2 and var.max() > 1e2 and np.abs(mean).max() > 0.1
        for n in ("policy_bn", "value_bn"):   # fold1x1 too: some var at least 4x away from 1
            assert np.abs(np.log2(V1[n][3])).max() >= 2, n
    else:
        for n in V0:   # exact powers of two everywhere
            m = V0[n] != V1[n]
            q = np.log2(np.abs(V1[n][m].astype(np.float64) / V0[n][m]))
            assert np.array_equal(q, np.round(q)), n


def test_signed_gamma_and_peaked():
    blocks, filters = 2, 32
    w = base_of(blocks, filters)
    V0 = N.views(w, blocks, filters)
    V1 = N.views(N.signed_gamma(w, blocks, filters, seed=17), blocks, filters)
    for b in range(blocks):
        neg = V1["res_blocks.%d.bn1" % b][0] < 0
        assert 8 <= neg.sum() <= 24 and np.array_equal(np.abs(V1["res_blocks.%d.bn1" % b]), np.abs(V0["res_blocks.%d.bn1" % b]))
        assert np.array_equal(V1["res_blocks.%d.bn2" % b], V0["res_blocks.%d.bn2" % b])
    c = get_case("peaked", 2, 32, 5)
    assert c.pol.max() > 20 / 4096 and c.pol.min() < 1e-8 and np.abs(c.val).max() > 0.8
    b = get_case("base", 2, 32, 5)
    assert b.pol.max() < 2 / 4096 and np.abs(b.val).max() < 0.2   # what the init weights give


@pytest.mark.parametrize("family,blocks,filters,rows", GPU_CASES)
def test_yardstick_has_headroom(family, blocks, filters, rows):
    """a plain float32 evaluation uses at most a quarter of the project's f32 tolerance, and errs at
    all (a zero yardstick error would make the measured bound unsatisfiable)"""
    c = get_case(family, blocks, filters, rows)
    use = N.tolerance_use(c.ypol, c.yval, c.pol, c.val)
    print("%-14s %2dx%-3d yardstick: value %.2e policy rel %.2e, %.1f %% of the tolerance; policy max %.3g min %.3g, |v| max %.4f"
          % (family, blocks, filters, c.yard_v, c.yard_p, 100 * use, c.pol.max(), c.pol.min(), np.abs(c.val).max()))
    assert np.isfinite(c.ypol).all() and np.isfinite(c.yval).all()
    assert use <= 0.25
    assert c.yard_v > 0 and c.yard_p > 0
    if "peaked" in family:
        assert c.pol.min() < 1e-8 and c.pol.max() > 10 / 4096


@pytest.mark.parametrize("blocks,filters", SEARCH_NETS)
def test_yardstick_has_headroom_on_search_rows(blocks, filters):
    c, _row_of, pos = search_case(blocks, filters)
    legal = np.zeros(c.pol.shape, bool)
    for r, k in enumerate(sorted(pos)):
        legal[r, pos[k].legal_indices()] = True
    assert len(pos) >= 60 and legal.any(1).all()
    use = N.tolerance_use(c.ypol, c.yval, c.pol, c.val)
    print("%dx%d search rows %d: yardstick uses %.1f %% of the tolerance; legal priors min %.3g, %d below 1e-8"
          % (blocks, filters, len(pos), 100 * use, c.pol[legal].min(), (c.pol[legal] < 1e-8).sum()))
    assert use <= 0.25
    assert (c.pol[legal] < 1e-8).any()     # the peaked priors include entries below the absolute term


REORDER_CASES = [(f,) + s for s in N.SMALL for f in ("base", "var5", "signed", "peaked")] + [(f,) + N.BIG for f in ("base", "peaked")]


@pytest.mark.parametrize("family,blocks,filters,rows", REORDER_CASES)
def test_yardstick_is_representative(family, blocks, filters, rows):
    """The yardstick with its channels in 8 other orders errs at most M / 4 = 2 times as much as in the
    plain order (how netcases.PLANES_SEED is chosen: otherwise M times the yardstick's error could be
    narrower than what float32 summation allows).  The channel scales through gamma are exact in
    float32, so gamma3 / 5 / 8 give the bits of the init weights, and gamma5+peaked those of peaked."""
    c = get_case(family, blocks, filters, rows)
    for other in {"base": ("gamma3", "gamma5", "gamma8"), "peaked": ("gamma5+peaked",)}.get(family, ()):
        if (other, blocks, filters, rows) in GPU_CASES:
            g = get_case(other, blocks, filters, rows)
            assert np.array_equal(g.ypol, c.ypol) and np.array_equal(g.yval, c.yval), other
    worst = 0.0
    for seed in range(N.REORDERINGS):
        pol, val = N.forward64(blocks, filters, N.reordered(c.w, blocks, filters, seed), c.planes, np.float32)
        worst = max(worst, *c.ratios(pol, val))
    print("%dx%d %-7s reordered yardstick / yardstick: %.2f" % (blocks, filters, family, worst))
    assert worst <= N.M / 4


@pytest.mark.parametrize("family,blocks,filters,rows", [(f,) + s for s in N.SMALL for f in N.FAMILIES] + [("gamma5",) + N.BIG])
def test_bf16_tolerance_is_satisfiable(family, blocks, filters, rows):
    """netcases.forward_bf16 (bf16 weights and stored activations, f32 accumulation, in numpy) is
    inside the project's bf16 tolerance on every case that the bf16 towers run"""
    c = get_case(family, blocks, filters, rows)
    pol, val = N.forward_bf16(blocks, filters, c.w, c.planes)
    use = N.tolerance_use(pol, val, c.pol, c.val, "bf16")
    print("%-14s %2dx%-3d bf16 restated in numpy uses %.0f %% of the bf16 tolerance" % (family, blocks, filters, 100 * use))
    N.check_tolerance(pol, val, c, "bf16")


def test_bf16_cannot_hold_peaked_logits_at_20_blocks():
    """why the 20x256 case of the bf16 towers is not peaked: the format itself is over the tolerance"""
    c = get_case("gamma5+peaked", *N.BIG)
    pol, val = N.forward_bf16(N.BIG[0], N.BIG[1], c.w, c.planes)
    use = N.tolerance_use(pol, val, c.pol, c.val, "bf16")
    print("20x256 gamma5+peaked: bf16 restated in numpy uses %.0f %% of the bf16 tolerance" % (100 * use))
    assert use > 1.5
