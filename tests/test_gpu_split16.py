"""tower32w_kernel<256> with the Winograd point GEMMs as split-f16 MFMA products (AZ_WINO_SPLIT16=1:
each f32 factor scaled by a power of two and split into two f16, hi hi + hi lo + lo hi accumulated
in f32) against the same kernel with f32 MFMA products (AZ_WINO_SPLIT16=0) on the same weights.
Tolerances: those of test_winograd_tower_matches_direct_tower (value atol 1e-5; policy rtol 1e-4,
atol 1e-8)."""
import numpy as np
import pytest

import azchess as A
import oracle as O
from azchess.agent import param_shapes
from test_gpu_net import random_planes

pytestmark = pytest.mark.gpu

PREFIX = "tower32w_kernel<256> (f32, Winograd F(2x2,3x3)"


def make_pair(monkeypatch, blocks, w):
    """(split-f16 net, f32-product net) on the same weights, kernel names asserted"""
    monkeypatch.setenv("AZ_WINO_SPLIT16", "1")
    on = A.AlphaZero(blocks, 256, weights=w, dtype="f32")
    assert on.tower_kernel.startswith(PREFIX) and "split-f16 MFMA" in on.tower_kernel, on.tower_kernel
    monkeypatch.setenv("AZ_WINO_SPLIT16", "0")
    off = A.AlphaZero(blocks, 256, weights=w, dtype="f32")
    assert off.tower_kernel.startswith(PREFIX) and "split-f16" not in off.tower_kernel, off.tower_kernel
    return on, off


def scaled_input_conv(w, k):
    """the weights with the input conv's output scaled by ~k.  Relies on the flat layout starting with
    input_conv.weight [256, 19, 3, 3] and input_conv.bias [256] (azchess.param_shapes), and on
    random_weights' BatchNorm being the identity to 1e-2 (mean and beta ~1e-2 are not scaled, so the
    factor is k only approximately); the activations themselves cannot be read back through the API"""
    assert [n for n, _s, _f in param_shapes(2, 256)[:3]] == ["input_conv.weight", "input_conv.bias", "input_bn"]
    w = w.copy()
    w[:256 * 19 * 9 + 256] *= k
    return w


def close(on_out, off_out):
    (pn, vn), (pf, vf) = on_out, off_out
    print("value max |d| %.3e  policy max rel %.3e" % (np.abs(vn - vf).max(), (np.abs(pn - pf) / (pf + 1e-30)).max()))
    np.testing.assert_allclose(vn, vf, atol=1e-5)
    np.testing.assert_allclose(pn, pf, rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("blocks,rows", [(2, 3), (20, 6)])
def test_split16_matches_f32_products(require_gpu, monkeypatch, blocks, rows):
    w = A.random_weights(blocks, 256, seed=3)
    planes = random_planes(rows, 13)
    on, off = make_pair(monkeypatch, blocks, w)
    close(on.forward(planes), off.forward(planes))


def test_split16_rows_are_independent(require_gpu, monkeypatch):
    """a row's outputs are bit-equal alone and inside a batch of 5"""
    monkeypatch.setenv("AZ_WINO_SPLIT16", "1")
    net = A.AlphaZero(2, 256, weights=A.random_weights(2, 256, seed=5), dtype="f32")
    assert "split-f16 MFMA" in net.tower_kernel
    planes = random_planes(5, 21)
    pb, vb = net.forward(planes)
    for r in (0, 3):
        p1, v1 = net.forward(planes[r:r + 1])
        assert np.array_equal(p1[0], pb[r]) and np.array_equal(v1[0], vb[r])


def test_split16_range(require_gpu, monkeypatch):
    """The input conv scaled up 32x (weights and bias: the tower's activations grow ~32x.  The tool's
    random-init tower peaks at |x| = 5.2, 167.5 at 32x -- tools/split16_numerics.py,
    profiles/split16_numerics.txt: inside the |x| < 255.8 that Sa = 64 represents, with the error at
    the f32-product level): finite outputs, still within the tolerance of the f32 products."""
    w = scaled_input_conv(A.random_weights(2, 256, seed=3), 32.0)
    planes = random_planes(3, 13)
    on, off = make_pair(monkeypatch, 2, w)
    out = on.forward(planes)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    close(out, off.forward(planes))


def test_split16_overflow_reaches_the_outputs(require_gpu, monkeypatch):
    """The input conv scaled up 2^16 x: the tower's activations (~5 x 2^16) are far beyond the 255.8
    that Sa = 64 represents.  Nothing is clamped: every policy entry and the value come out
    non-finite (the f32-product net on the same weights stays finite)."""
    w = scaled_input_conv(A.random_weights(2, 256, seed=3), 65536.0)
    planes = random_planes(3, 13)
    on, off = make_pair(monkeypatch, 2, w)
    pol, val = on.forward(planes)
    assert not np.isfinite(pol).any() and not np.isfinite(val).any()
    pf, vf = off.forward(planes)
    assert np.isfinite(pf).all() and np.isfinite(vf).all()


@pytest.mark.parametrize("persistent", [False, True])
def test_split16_search_replayed_by_oracle(require_gpu, monkeypatch, persistent):
    """a 16-simulation search of 2 games with the split-f16 tower in search mode (the heads write the
    priors into the new nodes' edges) replayed bit-exactly by the oracle from the GPU's evaluation
    log: as in smoke() (k_step + tower32w_kernel<256> per simulation step), and with the evaluation
    cache off, where the persistent per-game kernel k_sims32w<256> runs the same tower (which
    kernel ran is asserted).  This checks the search around the split-f16 tower; the tower's
    values are checked by the tests above and the oracle tests."""
    monkeypatch.setenv("AZ_WINO_SPLIT16", "1")
    net = A.AlphaZero(2, 256, weights=A.random_weights(2, 256, seed=42), dtype="f32")
    assert "split-f16 MFMA" in net.tower_kernel
    hist = [[], [588]]
    kw = dict(cache_capacity=0) if persistent else {}
    s = A.BatchedSearch(net, games=2, sims=16, seed=3, record_evals=True, eval_log_cap=4096, **kw)
    assert s.persistent == persistent
    s.set_roots(hist, apply_noise=True)
    _imp, vis, dep = s.run()
    rep = O.Replay(*s.eval_log())
    cfg = O.make_cfg(sims=16, noise=True, seed=3, eval_kind=2)
    for g, h in enumerate(hist):
        rv, _, rd, _ = O.search_game(cfg, h, noise=True, noise_key=O.lib().ref_stream_key(3, g, len(h), 0), replay=rep)
        assert np.array_equal(vis[g].astype(np.float32), rv) and dep[g] == rd
