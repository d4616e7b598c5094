"""The row-direct split-f16 weight stream (net.hip winograd_split16_rows, exported as
az_wino16_pack_rows) and the algebra of wino.h wino_core_h16<256, 12, true>, on the CPU.

F(2,3) Winograd across columns, a direct 3-tap correlation across rows: with W[k][b] = (g G^T)[k][b] for
the 3 tap rows x 4 column points and D[i][b] = (d B)[i][b] for the 4 raw patch rows,
    s_r[b] = sum_k W[k][b] D[r + k][b]      (r = 0, 1; summed over the input channels)
is row r of A^T (U . V), the first stage of the 2-D output transform: 8 accumulators instead of 16.
The packer is compared byte for byte with the numpy restatement below; a numpy model of one conv
compares the form's product error with the 16-point model's."""
import ctypes as C

import numpy as np

import azchess._lib as L
from test_wino_derive import AT, BT, G, SA, conv_model, exact_weights, folded, split, sw_exp, u_f64

RING = 4          # wino.h WinoRing<256, true, true>::PF: the stream ends in as many zero steps


def w_f64(wf):
    """W = g G^T [co][ci][k][b] in float64, in the packer's order of operations"""
    g = wf.astype(np.float64)
    W = np.empty(wf.shape[:2] + (3, 4))
    for k in range(3):
        for b in range(4):
            W[:, :, k, b] = g[:, :, k, 0] * G[b][0] + g[:, :, k, 1] * G[b][1] + g[:, :, k, 2] * G[b][2]
    return W


def pack_rows_numpy(wf):
    """the stream as uint16 [96 steps + RING][co/16][hi, lo][lane][8] and unscale"""
    F = wf.shape[0]
    W = w_f64(wf)
    se = sw_exp(W)                               # over the 12 values
    out = np.zeros(((F // 32) * 12 + RING, F // 16, 2, 64, 8), np.uint16)
    co, ci = np.meshgrid(np.arange(F), np.arange(F), indexing="ij")
    lane = co % 16 + 16 * ((ci % 32) // 8)
    for b in range(4):
        for k in range(3):
            hi, lo = split(np.ldexp(W[:, :, k, b], se))
            step = (ci // 32) * 12 + 3 * b + k
            out[step, co // 16, 0, lane, ci % 8] = hi.view(np.uint16)
            out[step, co // 16, 1, lane, ci % 8] = lo.view(np.uint16)
    return out, np.float32(np.ldexp(1.0 / SA, -se))


def pack_rows_lib(wf):
    F = wf.shape[0]
    wf = np.ascontiguousarray(wf, np.float32)
    n = L.lib.az_wino16_pack_rows(L.fptr(wf), F, None, 0, None)
    assert n > 0, L.lib.az_last_error()
    out = np.full(n, 0xFFFF, np.uint16)
    us = C.c_float(0)
    assert L.lib.az_wino16_pack_rows(L.fptr(wf), F, out.ctypes.data_as(C.POINTER(C.c_uint16)), n, C.byref(us)) == n
    return out, np.float32(us.value)


def test_packer_matches_numpy():
    F = 256
    wf = folded(F, 11 + F)
    want, wus = pack_rows_numpy(wf)
    got, gus = pack_rows_lib(wf)
    assert got.size == want.size == ((F // 32) * 12 + RING) * (F // 16) * 2 * 64 * 8
    got = got.reshape(want.shape)
    assert np.array_equal(got, want)
    assert not got[-RING:].any() and got[-RING - 1].any()      # the zero tail, and nothing before it
    assert gus == wus
    assert gus == np.float32(np.ldexp(1.0 / 64, -sw_exp(w_f64(wf))))
    # a short buffer is refused
    assert L.lib.az_wino16_pack_rows(L.fptr(wf), F, got.ctypes.data_as(C.POINTER(C.c_uint16)), got.size - 1, None) < 0


def test_sw_is_taken_over_the_12_values():
    """a conv whose taps are all equal has max|W| = 3/2 |g| against max|U| = 9/4 |g|: at |g| = 0.5 the
    two rules give different powers of two"""
    F = 256
    wf = np.full((F, F, 3, 3), 0.75, np.float32)            # max|W| = 1.125, max|U| = 1.6875
    assert sw_exp(w_f64(wf)) == 14 and sw_exp(u_f64(wf)) == 14
    wf = np.full((F, F, 3, 3), 0.5, np.float32)             # max|W| = 0.75 (Sw 2^15), max|U| = 1.125 (2^14)
    assert sw_exp(w_f64(wf)) == 15 and sw_exp(u_f64(wf)) == 14
    assert pack_rows_lib(wf)[1] == np.float32(2.0 ** -21)


def test_other_filter_counts_are_refused():
    for F in (64, 128):
        wf = folded(F, 1)
        assert L.lib.az_wino16_pack_rows(L.fptr(wf), F, None, 0, None) < 0
        assert b"256" in L.lib.az_last_error()


def test_row_sums_are_the_first_stage_of_the_output_transform():
    """sum_k W[k][b] D[r + k][b] == row r of A^T (U . V) in float64, for random g and d (dyadic values:
    every operation exact, so the identity holds to the bit)"""
    rng = np.random.default_rng(4)
    g = rng.integers(-64, 65, (50, 3, 3)) / 16.0
    d = rng.integers(-64, 65, (50, 4, 4)) / 16.0
    B64, G64 = BT.astype(np.float64), G
    U = np.einsum("ai,nij,bj->nab", G64, g, G64)
    V = np.einsum("ia,naj,kj->nik", B64, d, B64)
    W = np.einsum("nkj,bj->nkb", g, G64)
    D = np.einsum("nij,bj->nib", d, B64)
    want = np.einsum("ra,nab->nrb", AT, U * V)
    got = np.stack([sum(W[:, k] * D[:, r + k] for k in range(3)) for r in range(2)], axis=1)
    assert np.array_equal(got, want)
    # and the column stage then gives the 2x2 outputs of the direct correlation
    y = np.einsum("nrb,cb->nrc", got, AT)
    ref = np.stack([np.stack([(g * d[:, r:r + 3, c:c + 3]).sum((1, 2)) for c in range(2)], 1) for r in range(2)], 1)
    assert np.array_equal(y, ref)


def conv_model_rows(wf, x):
    """conv_model's scheme (tests/test_wino_derive.py) for the row-direct form: the column transform in
    float32, split-f16 factors, every product exact and summed in float64"""
    F = wf.shape[0]
    W = w_f64(wf)
    xp = np.zeros((F, 10, 10), np.float32)
    xp[:, 1:9, 1:9] = x
    d = np.stack([xp[:, 2 * t:2 * t + 4, 2 * u:2 * u + 4] for t in range(4) for u in range(4)], axis=1)   # ci, tile, 4, 4
    D = np.einsum("ctij,bj->ctib", d, BT).astype(np.float32)
    assert np.abs(D).max() <= 2 * np.abs(x).max()
    se = sw_exp(W)
    wh, wl = (p.astype(np.float64) for p in split(np.ldexp(W, se)))
    dh, dl = (p.astype(np.float64) for p in split((D * np.float32(SA)).astype(np.float64)))
    assert np.isfinite(dh).all()
    S = np.zeros((F, 16, 2, 4))
    for r in range(2):
        for k in range(3):
            for a, b in ((wh, dh), (wh, dl), (wl, dh)):
                S[:, :, r] += np.einsum("ocb,ctb->otb", a[:, :, k], b[:, :, r + k])
    S *= np.ldexp(1.0 / SA, -se)
    return np.einsum("otrb,cb->otrc", S, AT)


def test_row_direct_form_is_no_less_accurate():
    """rms relative error of Y against float64: the row-direct model no larger than the 16-point
    model's on the same data (no derived products, one transform pass fewer)"""
    F = 256
    for ws, xs in ((7, 8), (8, 7)):
        wf = folded(F, ws)
        x = np.maximum(np.random.default_rng(xs).standard_normal((F, 8, 8)), 0).astype(np.float32)
        ref = conv_model(wf, x, 0)
        rms = lambda y: float(np.sqrt(((y - ref) ** 2).mean() / (ref ** 2).mean()))
        e16, er = rms(conv_model(wf, x, 16)), rms(conv_model_rows(wf, x))
        print("rms relative error: 16 points %.3e, row-direct %.3e (%.2fx); Sw 2^%d / 2^%d"
              % (e16, er, er / e16, sw_exp(u_f64(wf)), sw_exp(w_f64(wf))))
        assert 0 < e16 < 1e-6
        assert 0 < er <= e16


def test_exact_family_fits_one_f16():
    """on the exact-arithmetic family (tests/test_wino_derive.py exact_weights) Sw W is exact in one
    f16, so the GPU's bit-equality test compares grouping alone"""
    import netcases as N
    blocks, F = 2, 256
    w = exact_weights(blocks, F, 1)
    for b in range(blocks):
        for k in (1, 2):
            W = w_f64(N.views(w, blocks, F)["res_blocks.%d.conv%d.weight" % (b, k)])
            s = np.ldexp(W, sw_exp(W))
            assert np.array_equal(s.astype(np.float16).astype(np.float64), s)
