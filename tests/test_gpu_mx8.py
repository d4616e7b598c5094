"""The MX-fp8 inference mode on the GPU (tower8_kernel, csrc/tower8.hip): one residual conv layer on
exact integer data through az_mx8_conv_probe (accumulators, bf16 output, codes and scale bytes EQUAL
to numpy's), the whole net against float64 within the fp8 tolerance (tests/mx8_ref.py TOL_FP8, fixed
from the numpy restatement alone), row independence, and the search mode bit for bit against the dense
forward and the oracle's replay.  profiles/fp8_numerics.txt is the NUMERICS table from an MI355X."""
import numpy as np
import pytest

import azchess as A
import mx8_ref as R
import netcases as N
import oracle as O
from test_gpu_net import random_planes
from test_gpu_search import compare_steps, histories
from test_netcases import get_case

pytestmark = pytest.mark.gpu

KERNEL = "tower8_kernel<%d> (MX-fp8 e4m3, direct 3x3)"


def int_code(v):
    """e4m3fn codes of integers, |v| <= 16 (exact)"""
    v = np.asarray(v, np.int64)
    a = np.abs(v)
    e = np.floor(np.log2(np.maximum(a, 1))).astype(np.int64)
    code = np.where(a == 0, 0, ((e + 7) << 3) | (((a << 3) >> e) & 7))
    return (code | np.where(v < 0, 0x80, 0)).astype(np.uint8)


def conv_data(F, n, seed, kind="random"):
    """integer operands on the grid: |w| <= 8, 0 <= a <= 8, block scales 2^s, s in [-2, 2] per block"""
    rng = np.random.default_rng(seed)
    w = rng.integers(-8, 9, (F, F, 3, 3))                 # asymmetric: no two (co, tap, ci) patterns alike
    a = rng.integers(0, 9, (n, 64, F))
    if kind == "corner":                                  # a single non-zero input square per board, in a corner
        keep = np.zeros((n, 64, 1), bool)
        for b in range(n):
            keep[b, (0, 7, 56, 63)[b % 4]] = True
        a = np.where(keep, np.maximum(a, 1), 0)
    if kind == "one-channel":                             # a single non-zero input channel per 32-block
        pick = rng.integers(0, 32, (n, 64, F // 32))
        a = np.where(np.arange(32) == pick[..., None], np.maximum(a.reshape(n, 64, F // 32, 32), 1), 0).reshape(n, 64, F)
    ws = rng.integers(-2, 3, (F, 9, F // 32))
    sa = rng.integers(-2, 3, (n, 64, F // 32))
    bias = rng.integers(-8, 9, F).astype(np.float32)
    resid = rng.integers(0, 9, (n, 64, F))
    wv = R.weight_blocks(w.astype(np.float64)) * np.repeat(2.0 ** ws, 32, axis=2)      # [co][tap][ci]
    av = a * np.repeat(2.0 ** sa, 32, axis=2)
    return dict(w=w, a=a, ws=ws, sa=sa, bias=bias, resid=resid, acc=R.conv_exact(av, wv, bias.astype(np.float64)))


CONV_CASES = [(128, 1, "random"), (128, 3, "random"), (128, 6, "random"), (256, 2, "random"), (256, 5, "random"),
              (256, 3, "corner"), (128, 5, "corner"), (256, 3, "one-channel"), (128, 2, "one-channel")]


@pytest.mark.parametrize("F,n,kind", CONV_CASES)
@pytest.mark.parametrize("residual", [False, True])
def test_conv_is_exact_on_integer_data(require_gpu, F, n, kind, residual):
    """test 4: every product and partial sum is exact in f32 (|sum| <= 2304 x 64 x 16 < 2^24 in units of
    2^-4), so the accumulators equal numpy's whatever the summation order; the epilogue's outputs follow
    from them exactly: y = relu(acc (+ residual)), its bf16 rounding, and its block quantisation."""
    d = conv_data(F, n, 1000 * F + 10 * n + len(kind), kind)
    assert np.abs(d["acc"]).max() * 16 < 2 ** 24 and np.all(d["acc"] * 16 == np.round(d["acc"] * 16))
    bf = lambda x: (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)      # exact small integers
    out = A.mx8_conv_probe(F, int_code(d["a"]), (d["sa"] + 127).astype(np.uint8), int_code(d["w"]),
                           (d["ws"] + 127).astype(np.uint8), d["bias"], residual=bf(d["resid"]) if residual else None)
    assert out["acc"].shape == (n, 64, F)
    bad = np.argwhere(out["acc"] != d["acc"])
    assert len(bad) == 0, (len(bad), bad[:5], out["acc"][tuple(bad[0])], d["acc"][tuple(bad[0])])
    y = np.maximum(d["acc"] + (d["resid"] if residual else 0), 0).astype(np.float32)
    assert np.array_equal(y, np.maximum(d["acc"] + (d["resid"] if residual else 0), 0))               # y is exact in f32
    codes, scales = R.quantize(y)
    assert np.array_equal(out["scales"].reshape(-1), scales)
    assert np.array_equal(out["codes"], codes), np.argwhere(out["codes"] != codes)[:5]
    if residual:
        want = (N.bf16_round(y).view(np.uint32) >> 16).astype(np.uint16)
        assert np.array_equal(out["bf16"], want)
    if kind == "random":        # the device quantiser met its edges: saturation above 448, zero blocks aside
        q = y.reshape(-1, 32) / 2.0 ** (scales.astype(np.float64) - 127)[:, None]
        assert (q > 448).any() and (q.max(1) == 0).sum() < len(q)


def fp8_net(blocks, filters, w):
    net = A.AlphaZero(blocks, filters, weights=w, dtype="fp8")
    assert net.tower_kernel == KERNEL % filters, net.tower_kernel
    return net


def report(label, c, pol, val):
    """NUMERICS line: the share of the fp8 tolerance used, and gpu error / forward_mx8 error"""
    mpol, mval = R.mx8_of(c)
    g, m = R.stats(pol, val, c.pol, c.val), R.stats(mpol, mval, c.pol, c.val)
    use = R.tolerance_use(pol, val, c.pol, c.val)
    print("NUMERICS %-9s %-14s %2dx%-3d gpu: value %.3e policy rel %.3e tv %.3e = %5.1f %% of the fp8 tolerance; "
          "gpu / numpy restatement: value %.2f policy %.2f tv %.2f"
          % (label, c.family, c.blocks, c.filters, g[0], g[1], g[2], 100 * use, g[0] / m[0], g[1] / m[1], g[2] / m[2]))


@pytest.mark.parametrize("family,blocks,filters,rows", R.CASES)
def test_net_matches_float64(require_gpu, family, blocks, filters, rows):
    """test 5: within the fp8 tolerance of the float64 reference (value 5e-3; policy 5e-2 relative + 2e-5;
    total variation 5e-3)"""
    c = get_case(family, blocks, filters, rows)
    pol, val = fp8_net(blocks, filters, c.w).forward(c.planes)
    report("enforced", c, pol, val)
    R.check_tolerance(pol, val, c.pol, c.val)


@pytest.mark.parametrize("family,blocks,filters,rows", R.PRINTED)
def test_net_on_peaked_heads_is_printed(require_gpu, family, blocks, filters, rows):
    """the peaked families: printed, not enforced (the bf16 mode cannot hold them at 20 blocks either)"""
    c = get_case(family, blocks, filters, rows)
    pol, val = fp8_net(blocks, filters, c.w).forward(c.planes)
    report("printed", c, pol, val)
    assert np.isfinite(pol).all() and np.isfinite(val).all()


def test_rows_are_batch_independent(require_gpu):
    """test 6: single rows and a rotated batch are bit-identical (13 rows at 2x128: 4 workgroups, the last partial)"""
    planes = random_planes(13, 5)
    net = fp8_net(2, 128, A.random_weights(2, 128, seed=42))
    pol, val = net.forward(planes)
    for i in (0, 5, 12):
        p1, v1 = net.forward(planes[i:i + 1])
        assert np.array_equal(p1[0], pol[i]) and v1[0] == val[i]
    p2, v2 = net.forward(np.concatenate([planes[7:], planes[:7]]))
    assert np.array_equal(p2[:6], pol[7:]) and np.array_equal(v2[6:], val[:7])
    assert np.array_equal(p2[6:], pol[:7]) and np.array_equal(v2[:6], val[7:])


def test_search_rows_equal_the_dense_forward(require_gpu):
    """test 7: every prior row and value the search mode logs equals, bit for bit, the dense forward of
    the same position at the legal indices; root visits sum to the simulations"""
    games, sims = 8, 16
    net = fp8_net(2, 128, A.random_weights(2, 128, seed=42))
    hs = histories(games, 77)
    s = A.BatchedSearch(net, games=games, sims=sims, seed=5, record_evals=True, eval_log_cap=4096)
    assert not s.persistent
    s.set_roots(hs, apply_noise=True)
    _imp, vis, _dep = s.run()
    assert np.all(vis.sum(1) == sims)
    keys, vals, off, idx, pri = s.eval_log()
    assert len(keys) >= games + sims
    # every evaluated position is a root or a child of an evaluated position
    logged, known, todo = set(int(k) for k in keys), {}, []
    for h in hs:
        p = A.Position.startpos()
        for a in h:
            p = p.play(a)
        todo.append(p)
    while todo:
        p = todo.pop()
        k = int(p.fen_key())
        if k in known or k not in logged:
            continue
        known[k] = p
        todo += [p.play(int(i)) for i in np.unique(p.legal_indices())]
    assert logged <= set(known)
    order = sorted(known)
    pol, val = net.forward(np.concatenate([A.to_tensor(known[k]) for k in order]))
    row = {k: i for i, k in enumerate(order)}
    for r in range(len(keys)):
        i = row[int(keys[r])]
        assert vals[r] == val[i], r
        assert np.array_equal(pri[off[r]:off[r + 1]], pol[i][idx[off[r]:off[r + 1]]]), r
        assert set(idx[off[r]:off[r + 1]].tolist()) == set(known[int(keys[r])].legal_indices().tolist())


def test_selfplay_replay_bit_exact(require_gpu):
    """test 7: self-play with a 2x128 fp8 net; the oracle, replaying the GPU's evaluations, reproduces
    every visit count, action, depth and final value"""
    games, sims = 4, 16
    net = fp8_net(2, 128, A.random_weights(2, 128, seed=42))
    sp = A.SelfPlay(net, games=games, sims=sims, seed=9, record_evals=True, eval_log_cap=1 << 17)
    sp.reset()
    steps = []
    for _ in range(600):
        _, active = sp.step()
        steps += sp.drain()
        if active == 0:
            break
    keys, vals, off, idx, pri = sp.search.eval_log()
    rep = O.Replay(keys, vals, off, idx, pri)
    ref, _, _ = O.selfplay(O.make_cfg(sims=sims, noise=True, seed=9, eval_kind=2), games, replay=rep)
    compare_steps(steps, ref)
    assert {s.game_id for s in steps} == set(range(games))


@pytest.mark.parametrize("filters", [128, 256])
def test_kernel_name_and_no_persistent_kernel(require_gpu, filters, monkeypatch):
    """test 8"""
    net = fp8_net(1, filters, A.random_weights(1, filters, seed=1))
    monkeypatch.setenv("AZ_PERSIST", "1")
    s = A.BatchedSearch(net, games=2, sims=4, seed=1)
    assert not s.persistent and A._lib.lib.az_search_persistent(s._h) == 0
    s.set_roots([[], []])
    _imp, vis, _dep = s.run()
    assert np.all(vis.sum(1) == 4)
