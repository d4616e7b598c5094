"""The laws of the search's random streams, on the CPU (oracle/detrng_ref.c; no GPU needed).

The engine replaces the reference's thread_rng() draws with its own streams (csrc/detmath.h), and the oracle
restates them; parity between the two says nothing about whether either draws from the right distribution.
Here the oracle's functions are held to what they claim to be:
  det_logf / det_expf   float64 log / exp, below 1 ulp of the correctly rounded result over the whole sweep
                        of tests/noisecases.py, with the IEEE outcomes at the edges;
  uniform01 / open01    their grids, their extreme draws, U(0,1);
  std_normal            N(0,1);
  gamma                 Gamma(shape, 1) for eight shapes, with a negative control;
  the Dirichlet row     its construction from the gamma draws, bit for bit -- so its law follows from theirs
                        -- plus independence of the components' draws and the per-component variance;
  weighted_index        counts of the sampled moves, in the oracle and in azchess.validation;
and az_noise_probe's host flavour -- the engine's own source, compiled for the host -- equals the oracle bit
for bit over the sweep (tests/test_gpu_noise_probe.py: the same for the device).

Every Kolmogorov-Smirnov test asserts D sqrt(N) <= 1.63, the asymptotic 1 % point of the Kolmogorov
distribution, on fixed keys: a condition on the generator, deterministic.  Measured D sqrt(N): uniform01 0.44,
open01 0.44, normal 0.74, gamma 0.93 / 0.73 / 0.67 / 0.67 / 0.79 / 0.74 / 0.74 / 0.74 at shapes 0.03 / 0.1 /
0.3 / 0.999 / 1 / 1.3 / 2.5 / 10; against a shape 10 % off: 5.1 .. 19.2.  Measured accuracy: det_logf 0.742
ulp, det_expf 0.860 ulp (0.746 subnormal spacings where the result is subnormal).  numpy and torch only."""
import math

import numpy as np
import pytest
import torch

import noisecases as N
import oracle as O
from azchess import chess as CH
from azchess import validation as V

KS_BOUND = 1.63
F32_MIN_NORMAL = 2.0 ** -126


# ------------------------------------------------------------------ det_logf / det_expf against float64
def _ulp_error(got, exact):
    """|got - exact| in ulps of the correctly rounded float32 result"""
    cr = exact.astype(np.float32)
    return np.abs(got.astype(np.float64) - exact) / np.spacing(np.abs(cr)).astype(np.float64)


def test_det_logf_accuracy_and_specials():
    x = N.logf_args()
    got = N.oracle("logf")
    pos = (x > 0) & np.isfinite(x)
    assert pos.sum() > 540000 and (x[pos] < F32_MIN_NORMAL).sum() > 26000       # subnormal arguments are in
    exact = np.log(x[pos].astype(np.float64))
    one = exact == 0.0
    assert one.sum() == 1 and np.all(N.bits(got[pos][one]) == 0)                # log(1) = +0
    assert np.all(np.abs(exact[~one]) >= F32_MIN_NORMAL)                        # every other result is a normal f32
    err = _ulp_error(got[pos][~one], exact[~one])
    print("det_logf: max error %.3f ulp over %d arguments" % (err.max(), err.size))
    assert err.max() < 1.0
    b = N.bits(x)
    assert np.all(N.bits(got[(b == 0) | (b == 0x80000000)]) == N.NINF)          # log(+-0) = -inf
    assert np.all(N.bits(got[b == N.PINF]) == N.PINF)
    neg = (x < 0) | np.isnan(x)
    assert neg.sum() >= 8 and np.all(np.isnan(got[neg]))                        # negative, -inf, NaN: NaN


def test_det_expf_accuracy_and_ieee_edges():
    x = N.expf_args()
    got = N.oracle("expf")
    fin = np.isfinite(x)
    with np.errstate(over="ignore", under="ignore"):
        exact = np.exp(x[fin].astype(np.float64))
        cr = exact.astype(np.float32)                                           # the correctly rounded result
    g = got[fin]
    normal = np.isfinite(cr) & (cr >= np.float32(F32_MIN_NORMAL))
    err = _ulp_error(g[normal], exact[normal])
    print("det_expf: max error %.3f ulp over %d arguments with a normal result" % (err.max(), err.size))
    assert normal.sum() > 700000 and err.max() < 1.0
    # gradual underflow: within one subnormal spacing of the true value, and exactly 0 below u_threshold
    sub = np.isfinite(cr) & ~normal
    suberr = np.abs(g[sub].astype(np.float64) - exact[sub]) / 2.0 ** -149
    print("det_expf: max error %.3f subnormal spacings over %d arguments" % (suberr.max(), suberr.size))
    assert sub.sum() > 200000 and (g[sub] > 0).sum() > 150000 and suberr.max() <= 1.0
    below = x[fin] < N.from_bits([N.EXP_U_THRESHOLD])[0]
    assert below.sum() > 400 and np.all(N.bits(g[below]) == 0)
    # overflow: +inf wherever the true result rounds past FLT_MAX -- every float from 0x42b17218 on, the first
    # above log(FLT_MAX) and the only ones the code compares with o_threshold; the floats between o_threshold
    # and there have finite results (k == 128) and are held to 1 ulp above
    over = np.isinf(cr)
    assert over.sum() > 1000 and np.all(N.bits(g[over]) == N.PINF)
    assert np.array_equal(over, (x[fin] > 0) & (N.bits(x[fin]) >= 0x42b17218))
    k128 = (x[fin] > N.from_bits([N.EXP_O_THRESHOLD])[0]) & ~over
    assert k128.sum() >= 8 and np.all(np.isfinite(g[k128]))
    b = N.bits(x)
    assert np.all(N.bits(got[b == N.NINF]) == 0) and np.all(N.bits(got[b == N.PINF]) == N.PINF)
    assert np.all(N.bits(got[(b == 0) | (b == 0x80000000)]) == 0x3f800000)
    assert np.isnan(x).sum() >= 2 and np.all(np.isnan(got[np.isnan(x)]))


# ------------------------------------------------------------------ Kolmogorov-Smirnov
def ks_scaled(x, cdf, zero_atom=False):
    """D sqrt(N) of the sample x against the continuous law cdf (float64 array -> float64 array), ties
    handled as blocks: the empirical CDF below and above each distinct value against the law there.
    zero_atom: a sample that is exactly 0 stands for the law's mass below the smallest positive float32 --
    the block of zeros is compared on its upper side only, with the law at 2^-149."""
    x = np.sort(np.asarray(x, np.float64))
    n = len(x)
    v, cnt = np.unique(x, return_counts=True)
    hi = np.cumsum(cnt) / n
    lo = hi - cnt / n
    f = cdf(np.maximum(v, 2.0 ** -149) if zero_atom else v)
    up, down = hi - f, f - lo
    if zero_atom and v[0] == 0.0:
        down[0] = 0.0
        up[0] = abs(up[0])
    return float(max(up.max(), down.max()) * math.sqrt(n))


def gamma_cdf(shape):
    return lambda v: torch.special.gammainc(torch.tensor(float(shape), dtype=torch.float64),
                                            torch.from_numpy(np.ascontiguousarray(v, np.float64))).numpy()


def normal_cdf(v):
    return 0.5 * (1.0 + torch.special.erf(torch.from_numpy(np.ascontiguousarray(v, np.float64)) / math.sqrt(2.0)).numpy())


# ------------------------------------------------------------------ streams
def test_uniform_streams_grids_extremes_and_law():
    u, o = N.oracle("uniform01"), N.oracle("open01")
    assert u.size == o.size == 1 << 18
    ku, ko = u.astype(np.float64) * 2.0 ** 24, o.astype(np.float64) * 2.0 ** 24
    assert np.all(ku == np.floor(ku)) and ku.min() >= 0 and ku.max() <= 2 ** 24 - 1   # [0, 1) on the 2^-24 grid
    assert np.all(ko == np.floor(ko)) and np.all(ko % 2 == 1)                         # odd multiples of 2^-24
    assert ko.min() >= 1 and ko.max() <= 2 ** 24 - 1                                  # (0, 1)
    # the sweep holds the two extreme draws (noisecases.scan_extreme_keys found the keys)
    assert o[0, 0] == np.float32(0.5 * 2.0 ** -23) == o.min()
    assert u[1, 0] == np.float32(1.0 - 2.0 ** -24) == u.max()
    # draws 1.. of the two planted keys are ordinary; the law is tested without their first draws
    du = ks_scaled(np.delete(u.ravel(), [0, N.STREAM_DRAWS]), lambda v: v)
    do = ks_scaled(np.delete(o.ravel(), [0, N.STREAM_DRAWS]), lambda v: v)
    print("D sqrt(N): uniform01 %.3f, open01 %.3f" % (du, do))
    assert du <= KS_BOUND and do <= KS_BOUND
    assert ks_scaled(u.ravel() ** 1.02, lambda v: v) > KS_BOUND                       # the bound bites at 2^18
    # consecutive draws of a stream are uncorrelated
    r = np.corrcoef(u[:, :-1].ravel(), u[:, 1:].ravel())[0, 1]
    assert abs(r) <= 4 / math.sqrt(u[:, 1:].size)


def test_stream_key_has_no_collision():
    """2^18 tuples (seed, game, ply, purpose): distinct keys, so no two roots or move choices share a stream"""
    f = O.lib().ref_stream_key
    keys = [f(seed, game, ply, purpose) for seed in (0, 1, 2, 3, 5, 23, 2 ** 32, 2 ** 63 + 7)
            for game in range(64) for ply in range(128) for purpose in range(4)]
    assert len(keys) == 1 << 18 and len(set(keys)) == len(keys)
    # and a Dirichlet row's component keys do not collide with each other or with their row's key
    ck = np.concatenate([O.component_keys(k, 256) for k in keys[:256]])
    assert len(set(ck.tolist()) | set(keys[:256])) == ck.size + 256


def test_std_normal_law():
    z = N.oracle("normal").astype(np.float64)
    n = len(z)
    d = ks_scaled(z, normal_cdf)
    print("D sqrt(N): std_normal %.3f; mean %.4f, variance %.4f" % (d, z.mean(), z.var()))
    assert d <= KS_BOUND
    assert ks_scaled(z * 1.1, normal_cdf) > KS_BOUND and ks_scaled(z + 0.05, normal_cdf) > KS_BOUND
    assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)


# ------------------------------------------------------------------ gamma
def _gamma_samples(shape):
    i = N.GAMMA_SHAPES.index(shape)
    return N.oracle("gamma")[i * N.GAMMA_KEYS:(i + 1) * N.GAMMA_KEYS]


@pytest.mark.parametrize("shape", N.GAMMA_SHAPES)
def test_gamma_law(shape):
    g = _gamma_samples(shape)
    n = len(g)
    assert np.all(np.isfinite(g)) and np.all(g >= 0)
    if shape >= 1.0:
        assert np.all(g > 0)                      # no underflow: a row of such draws cannot degenerate
    d = ks_scaled(g, gamma_cdf(shape), zero_atom=True)
    off = [ks_scaled(g, gamma_cdf(shape * f), zero_atom=True) for f in (0.9, 1.1)]
    x = g.astype(np.float64)
    mean, var = x.mean(), x.var()
    se_mean, se_var = math.sqrt(shape / n), math.sqrt((2 * shape ** 2 + 6 * shape) / n)   # mu4 - sigma^4 = 2k^2 + 6k
    print("shape %g: D sqrt(N) %.3f (shape x 0.9: %.2f, x 1.1: %.2f); zeros %d; mean %.4f (%.2f se), "
          "variance %.4f (%.2f se)" % (shape, d, off[0], off[1], int((g == 0).sum()), mean,
                                       (mean - shape) / se_mean, var, (var - shape) / se_var))
    assert d <= KS_BOUND
    assert min(off) > KS_BOUND                    # the negative control: a shape 10 % off is seen
    assert abs(mean - shape) <= 5 * se_mean and abs(var - shape) <= 5 * se_var


def test_gamma_zero_mass_at_tiny_shape():
    """an f32 Gamma(0.03) is exactly 0 with the law's mass below the smallest positive float32"""
    g = _gamma_samples(0.03)
    p0 = float(gamma_cdf(0.03)(np.array([2.0 ** -149]))[0])
    z = int((g == 0).sum())
    print("Gamma(0.03): CDF(2^-149) = %.4f, %d of %d samples are 0" % (p0, z, len(g)))
    assert abs(p0 - 0.0459) < 1e-4
    assert abs(z - p0 * len(g)) <= 5 * math.sqrt(len(g) * p0 * (1 - p0))


# ------------------------------------------------------------------ Dirichlet
LAW_KEYS = N.keys_from(777, 20000)


def _component_keys(keys, n):
    """[rows, n] component keys in numpy; the oracle's own function on the first and last row"""
    keys = np.asarray(keys, np.uint64)
    with np.errstate(over="ignore"):
        ck = N.splitmix64(keys[:, None] + (np.arange(n, dtype=np.uint64) + np.uint64(1))[None, :]
                          * np.uint64(0x9E3779B97F4A7C15))
    for r in (0, len(keys) - 1):
        assert np.array_equal(ck[r], O.component_keys(int(keys[r]), n))
    return ck


def _raw_rows(alphas, n, keys):
    """rand_distr's rows from the oracle's gamma draws in numpy float32: g_i * (1 / sum g), the sum serial in
    index order (np.cumsum accumulates sequentially) -> (rows, sum, 1 / sum)"""
    ck = _component_keys(keys, n)
    g = O.noise_batch("gamma", np.repeat(np.asarray(alphas, np.float32), n), ck.ravel()).reshape(ck.shape)
    s = np.cumsum(g, axis=1, dtype=np.float32)[:, -1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.float32(1.0) / s
        return g * inv[:, None], s, inv


def test_dirichlet_row_is_built_from_the_gamma_draws():
    """bit for bit g_i * (1 / sum g) with g_i = gamma(alpha, component_key(key, i)) and a serial f32 sum in
    index order: the row's law is the gammas' law.  No row of the sweep with alpha >= 0.3 degenerates, and
    every row whose 1 / sum is finite is exactly this arithmetic (what the fallback leaves untouched)."""
    for n in N.DIR_NS:
        rows, fb = N.oracle("dirichlet", n)
        alphas, keys = N.dirichlet_args(n)
        want, s, inv = _raw_rows(alphas, n, keys)
        plain = np.isfinite(inv) & (s != 0)
        assert np.array_equal(fb, ~plain)
        assert np.array_equal(N.bits(rows[plain]), N.bits(want[plain])), n
        assert not fb[alphas >= 0.3].any()
        assert np.all(np.isfinite(rows)) and np.all(rows >= 0)
        assert np.abs(rows.astype(np.float64).sum(1) - 1.0).max() < 1e-5


def _component_gammas(alpha, n, keys):
    ck = _component_keys(keys, n)
    g = O.noise_batch("gamma", np.full(ck.size, alpha, np.float32), ck.ravel())
    return g.reshape(ck.shape)


def test_dirichlet_components_are_uncorrelated():
    g = _component_gammas(0.3, 3, LAW_KEYS).astype(np.float64)
    for a, b in ((0, 1), (1, 2)):
        r = np.corrcoef(g[:, a], g[:, b])[0, 1]
        print("gamma draws of components %d, %d: r = %.4f" % (a, b, r))
        assert abs(r) <= 4 / math.sqrt(len(g))


@pytest.mark.parametrize("n", [2, 4, 20])
def test_dirichlet_component_variance(n):
    """per-component variance (n - 1) / (n^2 (n alpha + 1)) within 3 %, pooled over the components, at alpha
    0.3; rows drawn at an alpha 10 % off miss it"""
    def ratio(alpha):
        rows = O.noise_batch("dirichlet", np.full(len(LAW_KEYS), alpha, np.float32), LAW_KEYS, m=n)
        x = rows.astype(np.float64)
        assert np.abs(x.mean(0) - 1.0 / n).max() < 5 * math.sqrt((n - 1) / (n * n * (n * alpha + 1)) / len(x))
        return float(((x - 1.0 / n) ** 2).mean() / ((n - 1) / (n * n * (n * 0.3 + 1))))
    r = ratio(0.3)
    off = [ratio(0.27), ratio(0.33)]
    print("n = %d: measured / theory %.4f (alpha 0.27: %.4f, 0.33: %.4f)" % (n, r, off[0], off[1]))
    assert abs(r - 1.0) <= 0.03
    if n > 2:                                                 # at n = 2 a 10 % shift moves the variance by < 3 %
        assert all(abs(v - 1.0) > 0.03 for v in off)


# ------------------------------------------------------------------ the tiny-alpha row
def test_tiny_alpha_rows_are_distributions():
    """alpha 0.03, n = 2, raw keys 0..19999: rand_distr's arithmetic gives a non-finite row exactly where both
    gamma draws underflow; those rows, and only those, are computed in the log domain, and every row is a
    finite distribution"""
    rows, fb = N.oracle("tiny")
    _, keys = N.tiny_args()
    g = _component_gammas(N.TINY_ALPHA, 2, keys)
    s = (g[:, 0] + g[:, 1]).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = np.float32(1.0) / s
        raw = g * inv[:, None]
    bad = ~np.isfinite(raw).all(1)
    print("alpha 0.03, n = 2: %d of %d rows are non-finite in rand_distr's arithmetic" % (bad.sum(), len(bad)))
    assert bad.sum() >= 50
    assert np.array_equal(bad, fb)
    assert np.array_equal(N.bits(rows[~bad]), N.bits(raw[~bad]))             # finite rows: unchanged, bit for bit
    assert np.all(np.isfinite(rows)) and np.all(rows >= 0)
    assert np.abs(rows.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    # the fallback row is the same draws' ratio: g_0 / (g_0 + g_1) = 1 / (1 + exp(l_1 - l_0))
    assert np.all(rows[bad].max(1) >= 0.5)
    # at alpha 0.3 none of these keys degenerates
    r3, fb3 = O.noise_batch("dirichlet", np.full(len(keys), 0.3, np.float32), keys, m=2, with_fallback=True)
    g3 = _component_gammas(0.3, 2, keys)
    assert not fb3.any() and np.all(g3 > 0) and np.all(np.isfinite(r3))


def test_fallback_row_is_the_same_draws_in_the_log_domain():
    """the log-domain gamma equals float64 log of the plain draw wherever that is a normal float32, and a
    degenerate row is softmax of its two log-domain draws"""
    rows, fb = N.oracle("tiny")
    _, keys = N.tiny_args()
    ck = _component_keys(keys, 2).ravel()
    a = np.full(ck.size, N.TINY_ALPHA, np.float32)
    g = O.noise_batch("gamma", a, ck).astype(np.float64)
    l = O.noise_batch("gamma_log", a, ck).astype(np.float64)
    ok = g >= F32_MIN_NORMAL
    # l is a sum of two rounded f32 terms of magnitude up to |l| + 4: a few ulps of that, plus the draw's own
    # half ulp relative rounding
    tol = 4 * np.spacing((np.abs(l[ok]) + 4).astype(np.float32)).astype(np.float64) + 2.0 ** -23
    assert ok.sum() > 30000 and np.all(np.abs(l[ok] - np.log(g[ok])) <= tol)
    assert np.all(l[~ok] < math.log(F32_MIN_NORMAL) + 1e-3)
    l = l.reshape(-1, 2)[fb]
    e = np.exp(l - l.max(1, keepdims=True))
    assert np.abs(rows[fb] - e / e.sum(1, keepdims=True)).max() <= 1e-6


# ------------------------------------------------------------------ move sampling
def test_weighted_index_law():
    """WeightedIndex in the oracle (through arena_choose) and in azchess.validation on 2^16 stream uniforms
    over a 20-move policy with a zero and a 1e-6 weight: the same move on every draw, the zero-weight move
    never, every count within 5 binomial standard deviations of N w / sum w"""
    idx = np.array([7, 64, 65, 300, 511, 512, 777, 1000, 1024, 1500, 2047, 2048, 2500, 3000, 3333, 3500, 3999,
                    4000, 4090, 4095])
    w = np.array([0.11, 0.02, 0.0, 0.07, 0.05, 1e-6, 0.09, 0.03, 0.01, 0.13, 0.04, 0.06, 0.08, 0.005, 0.1, 0.015,
                  0.025, 0.035, 0.045, 0.085], np.float32)
    pol = np.zeros(4096, np.float32)
    pol[idx] = w
    u = O.noise_batch("uniform01", keys=N.keys_from(99, 1024), m=64).ravel()
    assert u.size == 1 << 16
    a = np.array([O.arena_choose(pol, 1, 15, float(x)) for x in u])
    b = np.array([V.weighted_index(pol, x) for x in u])
    assert np.array_equal(a, b)
    cnt = np.bincount(a, minlength=4096)
    assert cnt[idx[2]] == 0 and cnt.sum() == cnt[idx].sum()
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    sd = np.sqrt(u.size * p * (1 - p))
    dev = np.abs(cnt[idx] - u.size * p) / np.maximum(sd, 1e-300)
    print("weighted_index: max deviation %.2f sd; the 1e-6 move drawn %d times" % (dev[p > 0].max(), cnt[idx[5]]))
    assert np.all(dev[p > 0] <= 5.0)


# ------------------------------------------------------------------ the engine's source on the host
@pytest.mark.parametrize("case", ["logf", "expf", "uniform01", "open01", "normal", "gamma"])
def test_host_probe_equals_oracle(case):
    N.assert_same_bits(N.probe(case, CH.DEVICE_HOST), N.oracle(case), case)


@pytest.mark.parametrize("n", N.DIR_NS)
def test_host_probe_dirichlet_rows_equal_oracle(n):
    rows, fb = N.probe("dirichlet", CH.DEVICE_HOST, n)
    ref, rfb = N.oracle("dirichlet", n)
    N.assert_same_bits(rows, ref, "n = %d" % n)
    assert np.array_equal(fb, rfb)


def test_host_probe_tiny_alpha_rows_equal_oracle():
    rows, fb = N.probe("tiny", CH.DEVICE_HOST)
    ref, rfb = N.oracle("tiny")
    N.assert_same_bits(rows, ref, "alpha 0.03, n = 2")
    assert np.array_equal(fb, rfb) and fb.sum() >= 50


def test_noise_probe_refuses_bad_arguments():
    from azchess._lib import AzError
    k = np.zeros(2, np.uint64)
    for kw in (dict(op="gamma", x=[0.0, 1.0], keys=k), dict(op="gamma", x=[np.nan, 1.0], keys=k),
               dict(op="dirichlet", x=[0.3, 0.3], keys=k, m=257), dict(op="dirichlet", x=[0.3, 0.3], keys=k, m=0),
               dict(op="uniform01", keys=k, m=0)):
        with pytest.raises(AzError):
            CH.noise_probe(device=CH.DEVICE_HOST, **kw)
