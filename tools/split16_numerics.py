"""Numerics of split-f16 point GEMMs in the Winograd F(2x2,3x3) tower (CPU, numpy), in the setting of
tools/wino44_numerics.py: a 20x256 residual tower of random-init 3x3 convs over 8x8 boards (4 boards;
BatchNorm at its random-init identity, ReLU, residual adds) against the same tower in float64 with
direct convs.  The transforms run in float32.  Split products: V scaled by Sa and U by Sw (powers of
two), each split hi = f16(s), lo = f16(s - hi) (round to nearest even), M = hi hi + hi lo + lo hi with
exact f16 x f16 products (exact in f32: 11 + 11 bits) summed in float32 (numpy's blocked sums, not the
MFMA's order -- the error scale, not the bits), then unscaled by 1 / (Sa Sw).
Settles: the scale rule (Sa; Sw per conv = the largest power of two with Sw max|U| <= 32768, as
net.hip winograd_split16), the representable range (|V| <= 4 |x|, so |x| < 65504 / (4 Sa); the input
scaled up until the error leaves the f32-product level), f16 subnormals kept or flushed, and the split
source (U from its f64 value or from its rounded f32 value).
The last section, -- channel spread, gives every activation channel its own power-of-two scale (as a
trained net's BatchNorm does; tests/netcases.py channel_rescaled) on 3x64 and 2x128 towers, 3 boards:
the f32 paths are exactly scale invariant, the split-f16 path (one Sa, one Sw per conv) is not.
The section -- derived points prices streaming 12 (or 9) of the 16 points' weights and deriving the
rest (U[2][b] = U[0][b] + U[3][b] - U[1][b], wino.h wino_core_h16<F, 12>) on one 256x256 conv, products
summed in float64 so that only the product error shows.
Usage: python tools/split16_numerics.py [filters=256] [blocks=20]   (output: profiles/split16_numerics.txt)
       python tools/split16_numerics.py spread      (that section alone: profiles/split16_numerics_spread.txt)
       python tools/split16_numerics.py derive      (that section alone: profiles/derive_numerics.txt)
       python tools/split16_numerics.py rows        (the row-direct form, AZ_WINO_ROWS: profiles/rows_numerics.txt)"""
import sys

import numpy as np

rng = np.random.default_rng(0)
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float32)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float32)
F16_MIN_NORMAL = 2.0 ** -14


def conv_direct(x, w, dt):   # x [B,8,8,C], w [Co,Ci,3,3]
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), dt)
    xp[:, 1:-1, 1:-1] = x
    cols = np.stack([xp[:, i:i + H, j:j + W, :] for i in range(3) for j in range(3)], axis=3)
    wm = w.transpose(2, 3, 1, 0).reshape(9 * C, -1).astype(dt)
    return (cols.reshape(B * H * W, 9 * C).astype(dt) @ wm).reshape(B, H, W, -1)


def split(s, flush):
    """s (f32 or f64) -> (hi, lo) as float32 holding f16 values"""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = s.astype(np.float16)
        lo = (s - hi.astype(s.dtype)).astype(np.float16)
    if flush:
        hi = np.where(np.abs(hi) < F16_MIN_NORMAL, np.float16(0), hi)
        lo = np.where(np.abs(lo) < F16_MIN_NORMAL, np.float16(0), lo)
    return hi.astype(np.float32), lo.astype(np.float32)


def sw_exp(U):
    m = np.abs(U).max()
    return 24 if m == 0 else min(24, 15 - int(np.frexp(m)[1]))


class Conv:
    """one conv's point GEMMs: mode 'f32' (U rounded once to f32), or split-f16 with (Sa, flush, src)"""

    def __init__(self, mode, sa=64.0, flush=False, src="f64", scale=True):
        self.mode, self.sa, self.flush, self.src, self.scale = mode, np.float32(sa if scale else 1.0), flush, src, scale
        self.vmax = 0.0

    def __call__(self, x, w):
        B, H, W, C = x.shape
        U = np.einsum('ik,ockl,jl->ijoc', G, w.astype(np.float64), G)
        xp = np.zeros((B, H + 2, W + 2, C), np.float32)
        xp[:, 1:-1, 1:-1] = x
        d = np.stack([xp[:, 2 * t:2 * t + 4, 2 * u:2 * u + 4, :] for t in range(4) for u in range(4)], axis=1)  # B,16,4,4,C
        V = np.einsum('ia,btajc,kj->btikc', BT, d, BT).astype(np.float32)
        if self.mode == "f32":
            M = np.einsum('ijoc,btijc->btijo', U.astype(np.float32), V).astype(np.float32)
        else:
            se = sw_exp(U) if self.scale else 0
            Us = np.ldexp(U if self.src == "f64" else U.astype(np.float32), se)
            uh, ul = split(Us, self.flush)
            Vs = V * self.sa
            self.vmax = max(self.vmax, float(np.abs(Vs).max()))
            vh, vl = split(Vs, self.flush)
            ein = lambda u, v: np.einsum('ijoc,btijc->btijo', u, v).astype(np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                M = ((ein(uh, vh) + ein(uh, vl)).astype(np.float32) + ein(ul, vh)).astype(np.float32)
                M = M * np.float32(np.ldexp(1.0 / float(self.sa), -se))
        Y = np.einsum('ai,btijo,cj->btaco', AT, M, AT).astype(np.float32)    # B,16,2,2,Co
        return Y.reshape(B, 4, 4, 2, 2, -1).transpose(0, 1, 3, 2, 4, 5).reshape(B, 8, 8, -1)


def tower(x, ws, conv, dt):
    s = dt(1.0 / np.sqrt(1.0 + 1e-5))
    h, amax = x, float(np.abs(x).max())
    for b in range(len(ws) // 2):
        y = np.maximum(conv(h, ws[2 * b]) * s, 0).astype(dt)
        amax = max(amax, float(np.abs(y).max()))
        y = (conv(y, ws[2 * b + 1]) * s + h).astype(dt)
        h = np.maximum(y, 0).astype(dt)
        with np.errstate(invalid="ignore"):
            amax = max(amax, float(np.abs(h).max()))
    return h, amax


def spread_section():
    """Per-channel scales 2^k, k integer: s on the residual stream, t_b on block b's inner activation;
    conv1' = 2^t_b[co] conv1 / 2^s[ci], conv2' = 2^s[co] conv2 / 2^t_b[ci] (the BatchNorm scale folded
    into the conv, as net.hip fold_conv): the same function with the stream carrying 2^s times its
    value.  Statistic: max |out - float64| over the tower's output, each channel in units of its own
    scale 2^s[c] (at k = 0 the plain max abs error)."""
    print("-- channel spread (3 boards; max abs error of the tower output against float64, in channel units;"
          " Sa=64, U split from f64)")
    print("%-8s %-10s %9s | %10s %12s %12s %14s" % ("tower", "k in", "max |act|", "direct f32", "Winograd f32", "split kept", "split flushed"))
    r = np.random.default_rng(1)
    for nb, f in ((3, 64), (2, 128)):
        bound = 1.0 / np.sqrt(f * 9)
        base = [r.uniform(-bound, bound, (f, f, 3, 3)) for _ in range(2 * nb)]
        x = np.maximum(r.standard_normal((3, 8, 8, f)), 0)
        for lo, hi in ((0, 0), (-3, 3), (-5, 5), (-8, 4)):
            s = r.integers(lo, hi + 1, f)
            ws = []
            for b in range(nb):
                t = r.integers(lo, hi + 1, f)
                ws.append(base[2 * b] * (2.0 ** t)[:, None, None, None] / (2.0 ** s)[None, :, None, None])
                ws.append(base[2 * b + 1] * (2.0 ** s)[:, None, None, None] / (2.0 ** t)[None, :, None, None])
            xin = x * 2.0 ** s
            ref, amax = tower(xin, ws, lambda h, w: conv_direct(h, w, np.float64), np.float64)
            errs = []
            for conv in (lambda h, w: conv_direct(h, w, np.float32), Conv("f32"), Conv("h16", 64), Conv("h16", 64, flush=True)):
                out, _ = tower(xin.astype(np.float32), ws, conv, np.float32)
                errs.append((np.abs(out - ref) / 2.0 ** s).max())
            print("%-8s %-10s %9.1f | %10.1e %12.1e %12.1e %14.1e" % ("%dx%d" % (nb, f), "{0}" if lo == hi else "[%d,%d]" % (lo, hi), amax, *errs))


def derive_section(F=256, sa=64.0):
    """One conv, He-scaled random weights, ReLU'd normal input; rms relative error of Y against float64.
    Split products are exact and summed in float64; a derived point sums the products of its three
    (or nine) source points' split weights against its own V."""
    print("-- derived points (one %dx%d conv, Sa=%g, the Sw rule over all 16 points, products summed in float64)" % (F, F, sa))
    r = np.random.default_rng(7)
    w = (r.standard_normal((F, F, 3, 3)) * np.sqrt(2.0 / (9 * F))).astype(np.float32)
    x = np.maximum(r.standard_normal((1, 8, 8, F)), 0).astype(np.float32)
    U = np.einsum('ik,ockl,jl->ijoc', G, w.astype(np.float64), G)
    assert np.array_equal(U[2], U[0] + U[3] - U[1]), "row identity of G"
    xp = np.zeros((1, 10, 10, F), np.float32)
    xp[:, 1:-1, 1:-1] = x
    d = np.stack([xp[:, 2 * t:2 * t + 4, 2 * u:2 * u + 4, :] for t in range(4) for u in range(4)], axis=1)
    out = lambda M: np.einsum('ai,btijo,cj->btaco', AT.astype(np.float64), M, AT.astype(np.float64))
    ref = out(np.einsum('ijoc,btijc->btijo', U, np.einsum('ia,btajc,kj->btikc', BT.astype(np.float64), d.astype(np.float64), BT.astype(np.float64))))
    V = np.einsum('ia,btajc,kj->btikc', BT, d, BT).astype(np.float32)
    rms = lambda y: np.sqrt(((y - ref) ** 2).mean() / (ref ** 2).mean())
    se = sw_exp(U)
    uh, ul = (p.astype(np.float64) for p in split(np.ldexp(U, se), False))
    vh, vl = (p.astype(np.float64) for p in split((V * np.float32(sa)).astype(np.float64), False))
    prod = lambda i, j, a, b: (np.einsum('oc,btc->bto', uh[i, j], vh[:, :, a, b]) + np.einsum('oc,btc->bto', uh[i, j], vl[:, :, a, b]) +
                               np.einsum('oc,btc->bto', ul[i, j], vh[:, :, a, b]))
    src = lambda k, derived: ((0, 1), (3, 1), (1, -1)) if derived and k == 2 else ((k, 1),)
    base = None
    for name, dr, dc in (("16 streamed points", False, False), ("12 streamed, row 2 derived", True, False), ("9 streamed, both dimensions derived", True, True)):
        M = np.zeros((1, 16, 4, 4, F))
        for a in range(4):
            for b in range(4):
                for i, si in src(a, dr):
                    for j, sj in src(b, dc):
                        M[:, :, a, b] += si * sj * prod(i, j, a, b)
        e = rms(out(M * np.ldexp(1.0 / sa, -se)))
        base = base or e
        print("%-40s rms rel %.3e  (%.2fx)" % (name, e, e / base))
    y32 = out(np.einsum('ijoc,btijc->btijo', U.astype(np.float32), V).astype(np.float64))
    print("%-40s rms rel %.3e  (f32 products of the rounded f32 U, summed by numpy in f32)" % ("plain f32 evaluation of the same conv", rms(y32)))


def rows_section(F=256, sa=64.0):
    """The row-direct form (wino.h wino_core_h16<256, 12, true>) on derive_section's conv: W = g G^T
    (3 tap rows x 4 column points, Sw over these 12 values), D = d B (4 raw rows x 4 column points),
    s_r[b] = sum_k W[k][b] D[r + k][b], Y = s A; against the 16-point and the derived-row models."""
    print("-- row-direct form (one %dx%d conv, Sa=%g, products summed in float64)" % (F, F, sa))
    A64, B64 = AT.astype(np.float64), BT.astype(np.float64)
    for seed in (7, 8):
        r = np.random.default_rng(seed)
        w = (r.standard_normal((F, F, 3, 3)) * np.sqrt(2.0 / (9 * F))).astype(np.float32)
        x = np.maximum(r.standard_normal((1, 8, 8, F)), 0).astype(np.float32)
        xp = np.zeros((1, 10, 10, F), np.float32)
        xp[:, 1:-1, 1:-1] = x
        d = np.stack([xp[:, 2 * t:2 * t + 4, 2 * u:2 * u + 4, :] for t in range(4) for u in range(4)], axis=1)
        U = np.einsum('ik,ockl,jl->ijoc', G, w.astype(np.float64), G)
        ref = np.einsum('ai,btijo,cj->btaco', A64, np.einsum('ijoc,btijc->btijo', U, np.einsum('ia,btajc,kj->btikc', B64, d.astype(np.float64), B64)), A64)
        rms = lambda y: np.sqrt(((y - ref) ** 2).mean() / (ref ** 2).mean())
        sp = lambda s: tuple(p.astype(np.float64) for p in split(s, False))
        # 16 points and the derived row
        V = np.einsum('ia,btajc,kj->btikc', BT, d, BT).astype(np.float32)
        se = sw_exp(U)
        uh, ul = sp(np.ldexp(U, se))
        vh, vl = sp((V * np.float32(sa)).astype(np.float64))
        pr = lambda i, a: (np.einsum('joc,btjc->btjo', uh[i], vh[:, :, a]) + np.einsum('joc,btjc->btjo', uh[i], vl[:, :, a]) +
                           np.einsum('joc,btjc->btjo', ul[i], vh[:, :, a]))
        M16 = np.stack([pr(a, a) for a in range(4)], axis=2)
        M12 = M16.copy()
        M12[:, :, 2] = pr(0, 2) + pr(3, 2) - pr(1, 2)
        e16, e12 = (rms(np.einsum('ai,btijo,cj->btaco', A64, M * np.ldexp(1.0 / sa, -se), A64)) for M in (M16, M12))
        # row-direct
        W = np.einsum('ockl,jl->kjoc', w.astype(np.float64), G)
        D = np.einsum('btajc,kj->btakc', d, BT).astype(np.float32)
        sw = sw_exp(W)
        wh, wl = sp(np.ldexp(W, sw))
        dh, dl = sp((D * np.float32(sa)).astype(np.float64))
        S = np.zeros((1, 16, 2, 4, F))
        for rr in range(2):
            for k in range(3):
                for a, b in ((wh, dh), (wh, dl), (wl, dh)):
                    S[:, :, rr] += np.einsum('joc,btjc->btjo', a[k], b[:, :, rr + k])
        er = rms(np.einsum('btrjo,cj->btrco', S * np.ldexp(1.0 / sa, -sw), A64))
        print("seed %d: 16 points %.3e   12 streamed, row 2 derived %.3e (%.2fx)   row-direct %.3e (%.2fx)   Sw 2^%d / 2^%d   "
              "max|V| %.2f max|D| %.2f x max|x|" % (seed, e16, e12, e12 / e16, er, er / e16, se, sw,
                                                  np.abs(V).max() / np.abs(x).max(), np.abs(D).max() / np.abs(x).max()))


if sys.argv[1:2] == ["derive"]:
    derive_section()
    sys.exit(0)
if sys.argv[1:2] == ["rows"]:
    rows_section()
    sys.exit(0)
if sys.argv[1:2] == ["spread"]:
    spread_section()
    sys.exit(0)
F = int(sys.argv[1]) if len(sys.argv) > 1 else 256
NB = int(sys.argv[2]) if len(sys.argv) > 2 else 20
Bn = 4
bound = 1.0 / np.sqrt(F * 9)
ws = [rng.uniform(-bound, bound, (F, F, 3, 3)) for _ in range(2 * NB)]
x0 = np.maximum(rng.standard_normal((Bn, 8, 8, F)), 0)   # stand-in for the input conv's output
print("%dx%d tower, %d boards; Sw exponents of the convs: %s" % (NB, F, Bn, sorted({sw_exp(np.einsum('ik,ockl,jl->ijoc', G, w, G)) for w in ws})))


def report(name, xs, conv):
    ref, amax = tower(x0 * xs, ws, lambda h, w: conv_direct(h, w, np.float64), np.float64)
    out, _ = tower((x0 * xs).astype(np.float32), ws, conv, np.float32)
    with np.errstate(invalid="ignore"):
        e = np.abs(out - ref)
        rms = np.sqrt((e ** 2).mean() / (ref ** 2).mean())
    extra = "  max |Sa V| %.0f" % conv.vmax if getattr(conv, "vmax", 0) else ""
    print("%-46s in x%-5g max |act| %7.1f  rms rel %.3e  max abs %.3e%s" % (name, xs, amax, rms, e.max(), extra))


print("-- scale rule (input x1)")
report("F(2x2) f32 products", 1, Conv("f32"))
report("split-f16, no scaling", 1, Conv("h16", scale=False))
report("split-f16, no scaling, flushed", 1, Conv("h16", scale=False, flush=True))
for sa in (16, 64, 256):
    report("split-f16 Sa=%d" % sa, 1, Conv("h16", sa))
    report("split-f16 Sa=%d, flushed" % sa, 1, Conv("h16", sa, flush=True))
print("-- split source (Sa=64)")
report("split-f16 Sa=64, U split from f32", 1, Conv("h16", 64, src="f32"))
report("split-f16 Sa=64, U split from f32, flushed", 1, Conv("h16", 64, flush=True, src="f32"))
print("-- range (Sa=64: |x| < 65504 / 256 = 255.8; the error is relative, f32 products for comparison)")
for xs in (1 / 32, 8, 32, 64):
    report("F(2x2) f32 products", xs, Conv("f32"))
    report("split-f16 Sa=64", xs, Conv("h16", 64))
    report("split-f16 Sa=64, flushed", xs, Conv("h16", 64, flush=True))
spread_section()
