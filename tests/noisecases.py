"""One argument sweep for the search's random streams (csrc/detmath.h), shared by the CPU law tests
(tests/test_noise_laws.py) and the device parity tests (tests/test_gpu_noise_probe.py), and the oracle's
answers over it (oracle/detrng_ref.c), computed once per process.

The sweep is built from bit patterns, not from random floats, so that it names the places where a device
build can differ from a host build -- subnormal arguments and results, every branch threshold of det_logf /
det_expf with its neighbours, +-0, +-inf, NaN -- and is the same on every run.  numpy only; reads nothing
outside the repository."""
import functools

import numpy as np

def splitmix64(x):
    """SplitMix64's output function on a uint64 array (or int): the streams' mixer, restated"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def keys_from(base, n):
    """key_k = splitmix64(base + k), k = 0..n-1"""
    return splitmix64(np.uint64(base) + np.arange(n, dtype=np.uint64))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits1(v):
    """the bit pattern of one float32 value"""
    return int(np.array([v], np.float32).view(np.uint32)[0])


def from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def around(pattern, ulps):
    """the bit patterns pattern - ulps .. pattern + ulps (same sign; clipped at +-0)"""
    lo = max(int(pattern & 0x7fffffff) - ulps, 0)
    hi = int(pattern & 0x7fffffff) + ulps
    return (np.arange(lo, hi + 1, dtype=np.int64) | (pattern & 0x80000000)).astype(np.uint32)


QNAN = 0x7fc00000
PINF, NINF = 0x7f800000, 0xff800000
FLT_MAX = 0x7f7fffff
LOG_MANT_SWITCH = 0x3f800000 + (0x800000 - (0x95f64 << 3))     # det_logf: i flips, k += 1, x halves


@functools.lru_cache(None)
def logf_args():
    """float32 arguments of det_logf: every binade of the positive floats -- the 23 subnormal ones too --
    with 2,048 evenly spaced mantissas each (a binade's own offset below the spacing, so that the low
    mantissa bits vary as well); +-4 ulps around 2^-126, 1, the mantissa switch, FLT_MAX and the smallest
    subnormal; +-0, +-inf, a quiet NaN; negative values."""
    parts = []
    for e in range(1, 255):                                     # normal binades
        m = np.arange(2048, dtype=np.uint32) * 4096 + np.uint32((e * 977) & 4095)
        parts.append((np.uint32(e) << 23) | m)
    for j in range(23):                                         # subnormal binades [2^j, 2^(j+1)) ulps
        size = 1 << j
        if size <= 2048:
            parts.append(np.arange(size, 2 * size, dtype=np.uint32))
        else:
            step = size // 2048
            parts.append((size + np.arange(2048, dtype=np.uint32) * step + np.uint32((j * 977) % step)).astype(np.uint32))
    for p in (0x00800000, 0x3f800000, LOG_MANT_SWITCH, FLT_MAX, 0x00000001):
        parts.append(around(p, 4))
    parts.append(np.array([0x00000000, 0x80000000, PINF, NINF, QNAN, 0x80000001, 0x80800000, 0xbf800000,
                           0xc2c80000, 0xff7fffff], np.uint32))
    return from_bits(np.concatenate(parts))


EXP_THRESHOLDS = (0x42b17218, 0x3eb17218, 0x3F851592, 0x39000000)
EXP_O_THRESHOLD = 0x42b17180            # 8.8721679688e+01f
EXP_U_THRESHOLD = 0xc2cff1b5            # -1.0397208405e+02f


@functools.lru_cache(None)
def expf_args():
    """float32 arguments of det_expf: +-8 ulps around every threshold of the code in both signs, and around
    o_threshold and u_threshold; every 8th float of [-104, -87] (subnormal results, the k < -125 branch);
    every float of [88.0, 88.73] (k == 128 and the overflow edge); every 512th float of 2^-14 <= |x| up to
    89 / -104; +-0, +-inf, NaN."""
    parts = []
    for p in EXP_THRESHOLDS:
        parts += [around(p, 8), around(p | 0x80000000, 8)]
    parts += [around(EXP_O_THRESHOLD, 8), around(EXP_U_THRESHOLD, 8)]
    neg87, neg104 = bits1(-87.0), bits1(-104.0)
    parts.append(np.arange(neg87, neg104 + 1, 8, dtype=np.int64).astype(np.uint32))
    p88, p8873 = bits1(88.0), bits1(88.73)
    parts.append(np.arange(p88, p8873 + 1, dtype=np.int64).astype(np.uint32))
    tiny = bits1(2.0 ** -14)
    parts.append(np.arange(tiny, bits1(89.0) + 1, 512, dtype=np.int64).astype(np.uint32))
    parts.append((np.arange(tiny, bits1(104.0) + 1, 512, dtype=np.int64) | 0x80000000).astype(np.uint32))
    parts.append(np.array([0x00000000, 0x80000000, PINF, NINF, QNAN, 0xffc00001, 0x00000001, 0x80000001,
                           0x7f7fffff, 0xff7fffff], np.uint32))
    return from_bits(np.concatenate(parts))


# ---- streams: 4,096 keys x 64 draws.  The first two keys are found by a scan of raw keys 0, 1, 2, ... on the
# CPU (tests/test_noise_laws.py repeats the check, not the scan): draw 0 of MIN_OPEN01_KEY is the smallest
# open01, 0.5 * 2^-23, and draw 0 of MAX_UNIFORM01_KEY the largest uniform01, 1 - 2^-24.
STREAM_KEYS, STREAM_DRAWS = 4096, 64


def scan_extreme_keys(limit=1 << 26):
    """the scan that found the two constants below: the first raw keys whose draw 0 has 23 / 24 zero / one
    top bits"""
    lo = hi = None
    for base in range(0, limit, 1 << 22):
        r = splitmix64(np.arange(base, base + (1 << 22), dtype=np.uint64))
        if lo is None and (r >> np.uint64(41) == 0).any():
            lo = base + int(np.nonzero(r >> np.uint64(41) == 0)[0][0])
        if hi is None and (r >> np.uint64(40) == (1 << 24) - 1).any():
            hi = base + int(np.nonzero(r >> np.uint64(40) == (1 << 24) - 1)[0][0])
        if lo is not None and hi is not None:
            break
    return lo, hi


MIN_OPEN01_KEY, MAX_UNIFORM01_KEY = 5618432, 3747935


@functools.lru_cache(None)
def stream_keys():
    k = keys_from(424242, STREAM_KEYS)
    k[0], k[1] = MIN_OPEN01_KEY, MAX_UNIFORM01_KEY
    return k


# ---- gamma: 8 shapes x 20,000 keys splitmix64(12345 + k)
GAMMA_SHAPES = (0.03, 0.1, 0.3, 0.999, 1.0, 1.3, 2.5, 10.0)
GAMMA_KEYS = 20000


@functools.lru_cache(None)
def gamma_args():
    """(shapes [8 * 20000] f32, keys [8 * 20000] u64), shape-major"""
    k = keys_from(12345, GAMMA_KEYS)
    return (np.repeat(np.array(GAMMA_SHAPES, np.float32), GAMMA_KEYS), np.tile(k, len(GAMMA_SHAPES)))


def normal_keys():
    return keys_from(12345, GAMMA_KEYS)


# ---- Dirichlet rows: alpha x n; 64 / 65 cross the 64-lane stride, 256 is AZ_MAX_MOVES
DIR_ALPHAS = (0.03, 0.3, 2.5)
DIR_NS = (2, 5, 64, 65, 218, 256)


def dir_rows(n):
    return 2048 if n <= 5 else 512


@functools.lru_cache(None)
def dirichlet_args(n):
    """(alphas [3 * rows] f32, keys [3 * rows] u64) of the rows with n components, alpha-major"""
    r = dir_rows(n)
    return (np.repeat(np.array(DIR_ALPHAS, np.float32), r), np.tile(keys_from(777 + 1000003 * n, r), len(DIR_ALPHAS)))


# ---- the tiny-alpha rows: raw keys 0..19999 at alpha 0.03, n = 2 (100 of them degenerate)
TINY_ALPHA, TINY_N, TINY_KEYS = 0.03, 2, 20000


def tiny_args():
    return np.full(TINY_KEYS, TINY_ALPHA, np.float32), np.arange(TINY_KEYS, dtype=np.uint64)


# ---- the oracle's answers, once per process
@functools.lru_cache(None)
def oracle(case, n=0):
    """case: "logf", "expf", "uniform01", "open01", "normal", "gamma", "dirichlet" (n components; returns
    (rows, fallback)), "tiny" (rows, fallback).  The arrays are shared: read-only."""
    import oracle as O
    if case == "logf":
        out = O.noise_batch("logf", logf_args())
    elif case == "expf":
        out = O.noise_batch("expf", expf_args())
    elif case in ("uniform01", "open01"):
        out = O.noise_batch(case, keys=stream_keys(), m=STREAM_DRAWS)
    elif case == "normal":
        out = O.noise_batch("normal", keys=normal_keys())
    elif case == "gamma":
        out = O.noise_batch("gamma", *gamma_args())
    elif case == "dirichlet":
        out = O.noise_batch("dirichlet", *dirichlet_args(n), m=n, with_fallback=True)
    elif case == "tiny":
        out = O.noise_batch("dirichlet", *tiny_args(), m=TINY_N, with_fallback=True)
    else:
        raise KeyError(case)
    for a in (out if isinstance(out, tuple) else (out,)):
        a.setflags(write=False)
    return out


def probe(case, device, n=0):
    """the same case through az_noise_probe on `device`"""
    from azchess.chess import noise_probe
    if case == "logf":
        return noise_probe("logf", logf_args(), device=device)
    if case == "expf":
        return noise_probe("expf", expf_args(), device=device)
    if case in ("uniform01", "open01"):
        return noise_probe(case, keys=stream_keys(), m=STREAM_DRAWS, device=device)
    if case == "normal":
        return noise_probe("normal", keys=normal_keys(), device=device)
    if case == "gamma":
        return noise_probe("gamma", *gamma_args(), device=device)
    if case == "dirichlet":
        return noise_probe("dirichlet", *dirichlet_args(n), m=n, device=device, with_fallback=True)
    if case == "tiny":
        return noise_probe("dirichlet", *tiny_args(), m=TINY_N, device=device, with_fallback=True)
    raise KeyError(case)


def assert_same_bits(got, ref, what):
    """float32 arrays equal as uint32 bit patterns -- the sign of zero included -- except that any NaN
    matches any NaN"""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    bad = (gn != rn) | (~gn & (bits(got) != bits(ref)))
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d differ, first at %s: %r (0x%08x) vs the oracle's %r (0x%08x)"
                             % (what, int(bad.sum()), bad.size, tuple(i), float(got[tuple(i)]),
                                int(bits(got)[tuple(i)]), float(ref[tuple(i)]), int(bits(ref)[tuple(i)])))
