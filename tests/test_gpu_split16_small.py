"""tower32w_kernel<64> / <128> and k_sims32w<64> / <128> with the Winograd point GEMMs as split-f16
MFMA products (AZ_WINO_SPLIT16=2; tests/test_gpu_split16.py covers 256 filters, where level 1
already selects them).  Tolerances are the project's f32 ones (value atol 1e-5; policy rtol 1e-4,
atol 1e-8), as for split-f16 against f32 products at 256; every test asserts which kernel ran."""
import numpy as np
import pytest

import azchess as A
import oracle as O
from azchess.agent import param_shapes
from test_gpu_net import check, random_planes

pytestmark = pytest.mark.gpu

SMALL = [(6, 64), (2, 128)]


def plain_name(filters):
    return "tower32w_kernel<%d> (f32, Winograd F(2x2,3x3) residual convs)" % filters


def split_name(filters):
    return plain_name(filters)[:-1] + ", split-f16 MFMA products)"


def net_at(monkeypatch, level, blocks, filters, w=None):
    """an f32 net created with AZ_WINO_SPLIT16=level (None: unset)"""
    if level is None:
        monkeypatch.delenv("AZ_WINO_SPLIT16", raising=False)
    else:
        monkeypatch.setenv("AZ_WINO_SPLIT16", str(level))
    if w is None:
        w = A.random_weights(blocks, filters, seed=3)
    return A.AlphaZero(blocks, filters, weights=w, dtype="f32")


def make_pair(monkeypatch, blocks, filters, w):
    """(split-f16 net, f32-product net) on the same weights, kernel names asserted"""
    on = net_at(monkeypatch, 2, blocks, filters, w)
    assert on.tower_kernel == split_name(filters), on.tower_kernel
    off = net_at(monkeypatch, 0, blocks, filters, w)
    assert off.tower_kernel == plain_name(filters), off.tower_kernel
    return on, off


def close(on_out, off_out):
    (pn, vn), (pf, vf) = on_out, off_out
    print("value max |d| %.3e  policy max rel %.3e" % (np.abs(vn - vf).max(), (np.abs(pn - pf) / (pf + 1e-30)).max()))
    np.testing.assert_allclose(vn, vf, atol=1e-5)
    np.testing.assert_allclose(pn, pf, rtol=1e-4, atol=1e-8)


def scaled_input_conv(w, filters, k):
    """the weights with the input conv's output scaled by ~k: the flat layout starts with
    input_conv.weight [F, 19, 3, 3] and input_conv.bias [F] (see tests/test_gpu_split16.py)"""
    assert [n for n, _s, _f in param_shapes(2, filters)[:3]] == ["input_conv.weight", "input_conv.bias", "input_bn"]
    w = w.copy()
    w[:filters * 19 * 9 + filters] *= k
    return w


def test_selection_by_level(require_gpu, monkeypatch):
    """level 2 selects the split-f16 kernels at 64 and 128 filters; unset and 1 leave them on f32
    products; 0 turns the split off everywhere, 256 filters included"""
    for blocks, filters in SMALL:
        assert net_at(monkeypatch, 2, blocks, filters).tower_kernel == split_name(filters)
        for level in (None, 1, 0):
            assert net_at(monkeypatch, level, blocks, filters).tower_kernel == plain_name(filters), (level, filters)
    assert net_at(monkeypatch, 0, 2, 256).tower_kernel == plain_name(256)
    for level in (None, 1, 2):
        assert net_at(monkeypatch, level, 2, 256).tower_kernel == split_name(256), level


@pytest.mark.parametrize("blocks,filters,rows", [(6, 64, 5), (2, 128, 3)])
def test_split16_small_matches_f32_products(require_gpu, monkeypatch, blocks, filters, rows):
    """6x64 (C2's net) alternates both V buffers several times; 2x128 covers all four chunks and the
    ring carry between convs; odd row counts"""
    w = A.random_weights(blocks, filters, seed=3)
    planes = random_planes(rows, 13)
    on, off = make_pair(monkeypatch, blocks, filters, w)
    close(on.forward(planes), off.forward(planes))


@pytest.mark.parametrize("blocks,filters,n", [(6, 64, 8), (2, 128, 4)])
def test_split16_small_matches_oracle(require_gpu, monkeypatch, blocks, filters, n):
    w = A.random_weights(blocks, filters, seed=42)
    planes = random_planes(n, blocks * 1000 + filters)
    net = net_at(monkeypatch, 2, blocks, filters, w)
    assert net.tower_kernel == split_name(filters), net.tower_kernel
    pol, val = net.forward(planes)
    rpol, rval = O.RefNet(blocks, filters, w).forward(planes, threads=16)
    check(pol, val, rpol, rval, "f32")


@pytest.mark.parametrize("filters", [64, 128])
def test_split16_small_rows_are_independent(require_gpu, monkeypatch, filters):
    """a row's outputs are bit-equal alone and inside a batch of 5"""
    net = net_at(monkeypatch, 2, 2, filters, A.random_weights(2, filters, seed=5))
    assert net.tower_kernel == split_name(filters), net.tower_kernel
    planes = random_planes(5, 21)
    pb, vb = net.forward(planes)
    for r in (0, 3):
        p1, v1 = net.forward(planes[r:r + 1])
        assert np.array_equal(p1[0], pb[r]) and np.array_equal(v1[0], vb[r])


@pytest.mark.parametrize("filters", [64, 128])
def test_split16_small_range(require_gpu, monkeypatch, filters):
    """The input conv scaled up 32x stays inside the |x| < 255.8 that Sa = 64 represents
    (profiles/split16_numerics_64.txt, _128.txt): finite, within tolerance of the f32 products.
    Scaled up 2^16 x nothing is clamped: every policy entry and the value come out non-finite,
    while the f32-product net on the same weights stays finite."""
    w0 = A.random_weights(2, filters, seed=3)
    planes = random_planes(3, 13)
    on, off = make_pair(monkeypatch, 2, filters, scaled_input_conv(w0, filters, 32.0))
    out = on.forward(planes)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    close(out, off.forward(planes))
    on, off = make_pair(monkeypatch, 2, filters, scaled_input_conv(w0, filters, 65536.0))
    pol, val = on.forward(planes)
    assert not np.isfinite(pol).any() and not np.isfinite(val).any()
    pf, vf = off.forward(planes)
    assert np.isfinite(pf).all() and np.isfinite(vf).all()


@pytest.mark.parametrize("blocks,filters", SMALL)
def test_split16_small_search_replayed_by_oracle(require_gpu, monkeypatch, blocks, filters):
    """a 16-simulation search of 2 games, noise on, around the split-f16 tower, replayed bit-exactly by
    the oracle from the GPU's evaluation log: with k_step + tower32w_kernel<F> per simulation step,
    and with the evaluation cache off, where the persistent per-game kernel k_sims32w<F> runs the
    same tower (which ran is asserted).  The two modes run the same tower in two kernels: their
    visits and improved policies are bit-equal."""
    net = net_at(monkeypatch, 2, blocks, filters, A.random_weights(blocks, filters, seed=42))
    assert net.tower_kernel == split_name(filters), net.tower_kernel
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
