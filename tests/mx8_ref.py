"""The MX-fp8 inference mode's arithmetic in numpy (numpy only; reads nothing outside the repository).

quantize(x) is the normative block quantiser (OCP MX: e4m3fn elements, one E8M0 scale per 32
consecutive channels): az_mx8_quantize and the conv epilogue of tower8_kernel follow it bit for bit.
forward_mx8 restates the tower on netcases.views / EPS in the manner of netcases.forward_bf16: it is
for the error scale, not the bits (numpy's summation order is not the MFMA's).

The fp8 tolerance (TOL_FP8, same form as the bf16 mode's) is fixed from this file alone: forward_mx8
against netcases.forward64 over CASES, the largest value error, relative policy error (entries >= 1e-8)
and total variation, each times 4 and rounded up to one significant digit; pabs as in the bf16 mode.
Why 4: the statistic is a maximum over 3-5 rows, the MFMA's summation order is not numpy's, and an
e4m3 rounding flip moves an element by 6 % and is carried forward.
Measured (tests/test_mx8.py test_fp8_tolerance_is_satisfiable prints them):
    base    2x128  value 1.64e-4  policy rel 3.94e-3  total variation 2.92e-4
    gamma5  2x128  value 2.25e-4  policy rel 3.10e-3  total variation 2.47e-4
    base    2x256  value 3.79e-4  policy rel 3.08e-3  total variation 2.72e-4
    gamma5  2x256  value 3.23e-4  policy rel 2.89e-3  total variation 2.62e-4
    gamma5 20x256  value 1.24e-3  policy rel 1.19e-2  total variation 1.14e-3
    largest x 4:   value 4.97e-3 -> 5e-3, policy rel 4.74e-2 -> 5e-2, total variation 4.56e-3 -> 5e-3
(forward_bf16 on the same cases: value <= 1.2e-4, policy rel <= 2.5e-3, total variation <= 2.3e-4.)
"""
import numpy as np

import netcases

# (family, blocks, filters, rows) of the enforced GPU cases (tests/test_gpu_mx8.py) and of the tolerance
CASES = (("base", 2, 128, 5), ("gamma5", 2, 128, 5), ("base", 2, 256, 5), ("gamma5", 2, 256, 5), ("gamma5", 20, 256, 3))
# printed, not enforced: bf16 already cannot hold the peaked heads at 20 blocks (test_netcases.py)
PRINTED = (("peaked", 2, 128, 5), ("gamma5+peaked", 2, 256, 5), ("gamma5+peaked", 20, 256, 3))
TOL_FP8 = dict(v=5e-3, prel=5e-2, pabs=2e-5, tv=5e-3)

# value of every e4m3fn code (0x7f / 0xff: NaN)
_m = np.arange(256)
_e, _f = (_m >> 3) & 15, (_m & 7).astype(np.float64)
E4M3 = np.where(_e == 0, _f * 2.0 ** -9, (8 + _f) * 2.0 ** (_e - 10.0)) * np.where(_m & 128, -1.0, 1.0)
E4M3[[0x7F, 0xFF]] = np.nan
E4M3 = E4M3.astype(np.float32)


def quantize(x):
    """x: finite float32, a multiple of 32 values, blocks of 32 consecutive ones -> (codes uint8 of x's
    shape, scales uint8 [blocks]).  Scale exponent floor(log2 amax) - 8 clamped to the E8M0 range
    [-127, 127] (byte = exponent + 127; an all-zero block takes exponent 0); v / scale rounded to nearest
    even on the e4m3fn grid (subnormals kept), saturating at +-448."""
    x = np.ascontiguousarray(x, np.float32)
    v = x.reshape(-1, 32)
    amax = np.abs(v).max(axis=1).astype(np.float64)
    _, e = np.frexp(amax)                                 # amax = m 2^e, m in [0.5, 1): floor(log2 amax) = e - 1
    se = np.where(amax > 0, np.clip(e - 9, -127, 127), 0).astype(np.int64)
    a = np.minimum(np.ldexp(np.abs(v).astype(np.float64), -se[:, None]), 448.0)   # exact scaling, < 512 before
    _, ea = np.frexp(a)
    E = np.where(a > 0, np.maximum(ea - 1, -6), -6)       # the element's exponent; subnormals share 2^-6's quantum
    n = np.rint(np.ldexp(a, 3 - E))                       # units of 2^(E-3), ties to even; 16 carries into E + 1
    codes = ((E + 7) << 3) + n.astype(np.int64) - 8
    assert codes.min() >= 0 and codes.max() <= 0x7E
    codes = codes | np.where(np.signbit(v), 0x80, 0)
    return codes.astype(np.uint8).reshape(x.shape), (se + 127).astype(np.uint8)


def dequantize(codes, scales):
    """the float32 values (exact) of quantize's output"""
    c = np.asarray(codes)
    return (E4M3[c].reshape(-1, 32) * np.ldexp(np.float32(1), np.asarray(scales).astype(np.int64) - 127)[:, None]
            ).astype(np.float32).reshape(c.shape)


def qdq(x):
    return dequantize(*quantize(x))


def weight_blocks(wf):
    """folded conv weights [co][ci][3][3] -> [co][tap][ci]: a block is 32 input channels of one tap"""
    co, ci = wf.shape[:2]
    return np.ascontiguousarray(wf.reshape(co, ci, 9).transpose(0, 2, 1))


def conv_exact(act, wq, bias):
    """3x3 conv, padding 1, of act [n][64][F] with weights wq [co][tap][ci] (tap = 3 dy + dx), in float64"""
    n, F = act.shape[0], act.shape[2]
    xp = np.zeros((n, 10, 10, F))
    xp[:, 1:9, 1:9] = act.reshape(n, 8, 8, F)
    cols = np.stack([xp[:, i:i + 8, j:j + 8, :] for i in range(3) for j in range(3)], axis=3).reshape(n * 64, 9 * F)
    return (cols @ wq.astype(np.float64).reshape(wq.shape[0], 9 * F).T + bias).reshape(n, 64, -1)


def forward_mx8(blocks, filters, w, planes):
    """tower8_kernel's arithmetic: the input conv and the heads as netcases.forward_bf16 (bf16 weights
    and activations, float32 accumulation), the residual stream x kept in bf16; every residual conv on
    MX-quantised operands -- weights per (output channel, tap, 32 input channels) of the folded conv,
    activations per (square, 32 channels) from the float32 post-ReLU values (the first from the bf16 x
    the input conv leaves) -- with float32 accumulation in numpy's order and the float32 folded bias."""
    bf16_round, EPS = netcases.bf16_round, netcases.EPS
    W = netcases.views(np.asarray(w, np.float32).astype(np.float64), blocks, filters)
    F = filters

    def fold(name, bnname):
        g, beta, mean, var = W[bnname]
        sc = g / np.sqrt(var + EPS)
        wf = (W[name + ".weight"] * sc.reshape(-1, 1, 1, 1)).astype(np.float32)
        return wf, ((W[name + ".bias"] - mean) * sc + beta).astype(np.float32)

    def cols_of(x):
        n, c = x.shape[0], x.shape[3]
        xp = np.zeros((n, 10, 10, c), np.float32)
        xp[:, 1:9, 1:9] = x
        return np.stack([xp[:, i:i + 8, j:j + 8, :] for i in range(3) for j in range(3)], axis=3).reshape(n * 64, 9 * c)

    def conv8(xq, name, bnname):
        wf, bf = fold(name, bnname)
        wq = qdq(weight_blocks(wf))                       # [co][tap][ci]
        return (cols_of(xq) @ wq.reshape(F, 9 * F).T + bf).reshape(-1, 8, 8, F)

    def conv1(x, name, bnname):
        wf, bf = fold(name, bnname)
        return np.maximum(x @ wf.reshape(wf.shape[0], -1).T + bf, np.float32(0))

    x = bf16_round(np.ascontiguousarray(planes, np.float32).reshape(-1, 19, 8, 8).transpose(0, 2, 3, 1))
    n = x.shape[0]
    wf, bf = fold("input_conv", "input_bn")
    x = bf16_round(np.maximum((cols_of(x) @ bf16_round(wf).transpose(2, 3, 1, 0).reshape(9 * 19, -1) + bf).reshape(n, 8, 8, F), 0))
    xq = qdq(x)
    for b in range(blocks):
        h = np.maximum(conv8(xq, "res_blocks.%d.conv1" % b, "res_blocks.%d.bn1" % b), 0)
        y = np.maximum(conv8(qdq(h), "res_blocks.%d.conv2" % b, "res_blocks.%d.bn2" % b) + x, 0)
        x, xq = bf16_round(y), qdq(y)
    f = lambda name: W[name].astype(np.float32)
    p = conv1(x, "policy_conv_1", "policy_bn")
    z = (p @ f("policy_conv_2.weight").reshape(64, 32).T + f("policy_conv_2.bias")).transpose(0, 3, 1, 2).reshape(n, 4096)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    v = conv1(x, "value_conv", "value_bn").transpose(0, 3, 1, 2).reshape(n, 512)
    v = np.maximum(v @ f("value_linear_1.weight") + f("value_linear_1.bias"), 0)
    return e / e.sum(axis=1, keepdims=True), np.tanh(v @ f("value_linear_2.weight") + f("value_linear_2.bias"))[:, 0]


def stats(pol, val, rpol, rval):
    """(max |value error|, max relative policy error over entries >= 1e-8, max total variation)"""
    ev, ep = netcases.errors(pol, val, rpol, rval)
    return ev, ep, float(np.max(0.5 * np.abs(pol - rpol).sum(1)))


def tolerance_use(pol, val, rpol, rval):
    """the largest share of TOL_FP8 any output uses"""
    t = TOL_FP8
    return max(float(np.abs(val - rval).max()) / t["v"],
               float((np.abs(pol - rpol) / (t["prel"] * rpol + t["pabs"])).max()),
               float(np.max(0.5 * np.abs(pol - rpol).sum(1))) / t["tv"])


def check_tolerance(pol, val, rpol, rval):
    t = TOL_FP8
    assert np.isfinite(pol).all() and np.isfinite(val).all()
    assert np.all(np.abs(val - rval) <= t["v"]), np.abs(val - rval).max()
    assert np.all(np.abs(pol - rpol) <= t["prel"] * rpol + t["pabs"]), tolerance_use(pol, val, rpol, rval)
    assert np.max(0.5 * np.abs(pol - rpol).sum(1)) <= t["tv"]


_mx8 = {}


def mx8_of(c):
    """forward_mx8 of a netcases.Case, computed once per process"""
    key = (c.family, c.blocks, c.filters, c.planes.shape[0])
    if key not in _mx8:
        _mx8[key] = forward_mx8(c.blocks, c.filters, c.w, c.planes)
    return _mx8[key]
