"""The split-f16 Winograd weight stream with derived points (net.hip winograd_split16, exported as
az_wino16_pack), on the CPU.

G's rows satisfy r1 + r2 = r0 + r3, so U[2][b] = U[0][b] + U[3][b] - U[1][b]: with 12 streamed points
the packer leaves row 2 of U out, stores row 1 negated, and orders a 32-channel group's steps
[b][a in (0, 1, 3)], so that the three sources of the derived point (2, b) are consecutive steps.
The packer is compared byte for byte with the numpy restatement below; a numpy model of one conv then
prices the derived points' product error."""
import ctypes as C

import numpy as np
import pytest

import azchess._lib as L

G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
SA = 64.0
ROWS12 = (0, 1, 3)


def folded(F, seed):
    """He-scaled random weights [co][ci][3][3], as a BatchNorm-folded conv"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((F, F, 3, 3)) * np.sqrt(2.0 / (9 * F))).astype(np.float32)


def u_f64(wf):
    """U = G g G^T [co][ci][a][b] in float64, in the packer's order of operations"""
    g = wf.astype(np.float64)
    gg = [[G[a][0] * g[:, :, 0, j] + G[a][1] * g[:, :, 1, j] + G[a][2] * g[:, :, 2, j] for j in range(3)] for a in range(4)]
    U = np.empty(wf.shape[:2] + (4, 4))
    for a in range(4):
        for b in range(4):
            U[:, :, a, b] = gg[a][0] * G[b][0] + gg[a][1] * G[b][1] + gg[a][2] * G[b][2]
    return U


def sw_exp(U):
    m = np.abs(U).max()
    return 24 if m == 0 else min(24, 15 - int(np.frexp(m)[1]))


def split(s):
    hi = s.astype(np.float16)
    lo = (s - hi.astype(np.float64)).astype(np.float16)
    return hi, lo


def pack_numpy(wf, streamed):
    """the stream as uint16 [steps + 2][co/16][hi, lo][lane][8] and unscale"""
    F = wf.shape[0]
    U = u_f64(wf)
    se = sw_exp(U)                               # over all 16 values, whatever is streamed
    order = [(a, b) for a in range(4) for b in range(4)] if streamed == 16 else [(a, b) for b in range(4) for a in ROWS12]
    out = np.zeros(((F // 32) * streamed + 2, F // 16, 2, 64, 8), np.uint16)
    co, ci = np.meshgrid(np.arange(F), np.arange(F), indexing="ij")
    lane = co % 16 + 16 * ((ci % 32) // 8)
    for i, (a, b) in enumerate(order):
        s = np.ldexp(U[:, :, a, b], se)
        if streamed == 12 and a == 1:
            s = -s
        hi, lo = split(s)
        step = (ci // 32) * streamed + i
        out[step, co // 16, 0, lane, ci % 8] = hi.view(np.uint16)
        out[step, co // 16, 1, lane, ci % 8] = lo.view(np.uint16)
    return out, np.float32(np.ldexp(1.0 / SA, -se))


def pack_lib(wf, streamed):
    F = wf.shape[0]
    wf = np.ascontiguousarray(wf, np.float32)
    n = L.lib.az_wino16_pack(L.fptr(wf), F, streamed, None, 0, None)
    assert n > 0, L.lib.az_last_error()
    out = np.full(n, 0xFFFF, np.uint16)
    us = C.c_float(0)
    assert L.lib.az_wino16_pack(L.fptr(wf), F, streamed, out.ctypes.data_as(C.POINTER(C.c_uint16)), n, C.byref(us)) == n
    return out, np.float32(us.value)


@pytest.mark.parametrize("streamed", [16, 12])
@pytest.mark.parametrize("F", [64, 256])
def test_packer_matches_numpy(F, streamed):
    wf = folded(F, 11 + F)
    want, wus = pack_numpy(wf, streamed)
    got, gus = pack_lib(wf, streamed)
    assert got.size == want.size == ((F // 32) * streamed + 2) * (F // 16) * 2 * 64 * 8
    got = got.reshape(want.shape)
    assert np.array_equal(got, want)
    assert not got[-2:].any()                    # the zero tail
    assert gus == wus and gus == pack_lib(wf, 16)[1]   # one Sw rule for both streams
    if streamed == 12:
        # against the 16-point stream: the steps [b][0, 1, 3] are its points (0, b), (1, b), (3, b), row 1
        # with the sign bit of hi and lo flipped (a lo of +0, hi being exact, stays +0)
        full = pack_lib(wf, 16)[0].reshape(want.shape[0] // 12 * 16 + 2, F // 16, 2, 64, 8)[:-2]
        full = full.reshape((F // 32), 16, F // 16, 2, 64, 8)
        mine = got[:-2].reshape((F // 32), 12, F // 16, 2, 64, 8)
        for b in range(4):
            assert np.array_equal(mine[:, 3 * b], full[:, b])
            neg = full[:, 4 + b] ^ 0x8000
            neg[:, :, 1][full[:, 4 + b][:, :, 1] == 0] = 0
            assert np.array_equal(mine[:, 3 * b + 1], neg)
            assert np.array_equal(mine[:, 3 * b + 2], full[:, 12 + b])


def test_streamed_16_is_the_documented_layout():
    """[ci/32][xi][co/16][hi, lo][lane][8], lane = co % 16 + 16 (ci % 32 / 8), component ci % 8,
    checked element by element on a handful of (co, ci, xi)"""
    F = 64
    wf = folded(F, 5)
    U = u_f64(wf)
    se = sw_exp(U)
    got = pack_lib(wf, 16)[0]
    rng = np.random.default_rng(0)
    for co, ci, xi in zip(rng.integers(0, F, 40), rng.integers(0, F, 40), rng.integers(0, 16, 40)):
        hi, lo = split(np.ldexp(U[co, ci, xi // 4, xi % 4], se).reshape(1))
        at = ((((ci // 32) * 16 + xi) * (F // 16) + co // 16) * 2 * 64 + co % 16 + 16 * ((ci % 32) // 8)) * 8 + ci % 8
        assert got[at] == hi.view(np.uint16)[0] and got[at + 64 * 8] == lo.view(np.uint16)[0]


def test_packer_rejects_other_counts():
    wf = folded(64, 1)
    assert L.lib.az_wino16_pack(L.fptr(wf), 64, 9, None, 0, None) < 0
    assert L.lib.az_wino16_pack(L.fptr(wf), 48, 16, None, 0, None) < 0


def test_row_identity_is_exact_in_f64():
    U = u_f64(folded(256, 3))
    assert np.array_equal(U[:, :, 2, :], U[:, :, 0, :] + U[:, :, 3, :] - U[:, :, 1, :])


def conv_model(wf, x, streamed):
    """One conv [ci][8][8] -> [co][8][8]: transforms in float32, split-f16 factors, every product
    exact and summed in float64 (the product error alone).  streamed = 12: M[2][b] from the three
    streamed rows against V[2][b]; 9: columns derived as well; 0: plain float64."""
    F = wf.shape[0]
    U = u_f64(wf)
    xp = np.zeros((F, 10, 10), np.float32)
    xp[:, 1:9, 1:9] = x
    d = np.stack([xp[:, 2 * t:2 * t + 4, 2 * u:2 * u + 4] for t in range(4) for u in range(4)], axis=1)   # ci, tile, 4, 4
    if streamed == 0:
        V = np.einsum("ia,ctaj,kj->ctik", BT.astype(np.float64), d.astype(np.float64), BT.astype(np.float64))
        M = np.einsum("ocik,ctik->otik", U, V)
    else:
        V = np.einsum("ia,ctaj,kj->ctik", BT, d, BT).astype(np.float32)
        se = sw_exp(U)
        uh, ul = (p.astype(np.float64) for p in split(np.ldexp(U, se)))
        vh, vl = (p.astype(np.float64) for p in split((V * np.float32(SA)).astype(np.float64)))
        assert np.isfinite(vh).all()
        prod = lambda sl_u, sl_v: (np.einsum("oc...,ct...->ot...", uh[sl_u], vh[sl_v]) + np.einsum("oc...,ct...->ot...", uh[sl_u], vl[sl_v]) +
                                   np.einsum("oc...,ct...->ot...", ul[sl_u], vh[sl_v]))
        M = np.empty((F, 16, 4, 4))
        for a in range(4):
            for b in range(4):
                da, db = streamed <= 12 and a == 2, streamed == 9 and b == 2
                M[:, :, a, b] = sum(sa * sb * prod((slice(None), slice(None), ua, ub), (slice(None), slice(None), a, b))
                                    for ua, sa in (((0, 1), (3, 1), (1, -1)) if da else ((a, 1),))
                                    for ub, sb in (((0, 1), (3, 1), (1, -1)) if db else ((b, 1),)))
        M *= np.ldexp(1.0 / SA, -se)
    return np.einsum("ai,otik,bk->otab", AT, M, AT)


def test_derived_points_cost_little_accuracy():
    """rms relative error of Y against float64: the 12-point model within 1.5x the 16-point model's
    on the same data"""
    F = 256
    wf = folded(F, 7)
    x = np.maximum(np.random.default_rng(8).standard_normal((F, 8, 8)), 0).astype(np.float32)
    ref = conv_model(wf, x, 0)
    rms = lambda y: float(np.sqrt(((y - ref) ** 2).mean() / (ref ** 2).mean()))
    e16, e12 = rms(conv_model(wf, x, 16)), rms(conv_model(wf, x, 12))
    print("rms relative error: 16 streamed %.3e, 12 streamed %.3e (%.2fx)" % (e16, e12, e12 / e16))
    assert 0 < e16 < 1e-6
    assert e12 <= 1.5 * e16


# ---- the exact-arithmetic family (shared with tests/test_gpu_wino_derive.py)
def exact_weights(blocks, F, seed):
    """Weights on which every product and sum of the tower is exact in f16 x f16 -> f32 and in f32
    alike, so that the tower's activations do not depend on how its sums are grouped: BatchNorm the
    identity (var = f32(1 - eps): the fold's factor rounds away), no conv bias, an input conv of two
    taps of 1 per output channel over 0/1 planes, residual convs of three taps of +-1/2 per output
    channel (U then holds multiples of 1/8 with a few significant bits).  Activations stay multiples
    of 2^-(2 blocks) below 2 x 3.25^blocks.  The heads keep their random weights: they run the same
    code on the same activations."""
    import azchess as A
    import netcases as N
    rng = np.random.default_rng(seed)
    w = np.array(A.random_weights(blocks, F, seed=9), np.float32)
    W = N.views(w, blocks, F)
    names = [("input_conv", "input_bn", 19, 2, 1.0)]
    for b in range(blocks):
        names += [("res_blocks.%d.conv%d" % (b, k), "res_blocks.%d.bn%d" % (b, k), F, 3, 0.5) for k in (1, 2)]
    for conv, bn, cin, taps, mag in names:
        W[conv + ".weight"][...] = 0
        W[conv + ".bias"][...] = 0
        W[bn][...] = np.array([1, 0, 0, np.float32(1 - N.EPS)], np.float32).reshape(4, 1)
        for co in range(F):
            for at in rng.choice(cin * 9, taps, replace=False):
                W[conv + ".weight"][co, at // 9, at % 9 // 3, at % 3] = mag * (1 if mag == 1.0 or rng.random() < 0.75 else -1)
    sc = 1.0 / np.sqrt(float(np.float32(1 - N.EPS)) + N.EPS)
    assert np.float32(0.5 * sc) == 0.5 and np.float32(1.0 * sc) == 1.0      # net.hip fold_conv
    return w


def exact_planes(rows, seed):
    return (np.random.default_rng(seed).random((rows, 19, 8, 8)) < 0.2).astype(np.float32)


def exact_tower(blocks, F, w, planes, dt):
    """the residual tower's output [rows, 8, 8, F] on the folded (= raw) conv weights, in dt"""
    import netcases as N
    W = N.views(np.asarray(w).astype(dt), blocks, F)

    def conv3(x, name):
        n, c = x.shape[0], x.shape[3]
        xp = np.zeros((n, 10, 10, c), dt)
        xp[:, 1:9, 1:9] = x
        cols = np.stack([xp[:, i:i + 8, j:j + 8, :] for i in range(3) for j in range(3)], axis=3).reshape(n * 64, 9 * c)
        return (cols @ W[name + ".weight"].transpose(2, 3, 1, 0).reshape(9 * c, -1)).reshape(n, 8, 8, -1)

    x = np.maximum(conv3(planes.transpose(0, 2, 3, 1).astype(dt), "input_conv"), 0)
    for b in range(blocks):
        h = np.maximum(conv3(x, "res_blocks.%d.conv1" % b), 0)
        x = np.maximum(conv3(h, "res_blocks.%d.conv2" % b) + x, 0)
    assert x.dtype == dt
    return x


def test_exact_family_is_exact_and_alive():
    """float32 and float64 evaluation give the same activations, which fit the split-f16 factors
    (multiples of 1/16 below 64: Sa V = 64 x a sum of four of them has at most 22 bits) and are
    non-trivial; Sw U is exact in one f16"""
    blocks, F = 2, 256
    w = exact_weights(blocks, F, 1)
    planes = exact_planes(4, 2)
    a64, a32 = exact_tower(blocks, F, w, planes, np.float64), exact_tower(blocks, F, w, planes, np.float32)
    assert np.array_equal(a64, a32.astype(np.float64))
    assert np.array_equal(a64 * 16, np.round(a64 * 16)) and a64.max() < 64
    alive = (a64 > 0).mean()
    print("exact family: max activation %g, %.0f %% positive, %d distinct values" % (a64.max(), 100 * alive, np.unique(a64).size))
    assert alive > 0.25 and np.unique(a64).size > 20
    import netcases as N
    for b in range(blocks):
        for k in (1, 2):
            U = u_f64(N.views(w, blocks, F)["res_blocks.%d.conv%d.weight" % (b, k)])
            s = np.ldexp(U, sw_exp(U))
            assert np.array_equal(s.astype(np.float16).astype(np.float64), s)
