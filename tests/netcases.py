"""Trained-like weights for the network tests, and a plain numpy restatement of AlphaZero::forward
to compare the HIP towers with (numpy only; reads nothing outside the repository).

azchess.random_weights gives BatchNorm = identity +- 1e-2 and one magnitude for every channel: a
near-uniform policy and a small value.  The families here keep its convolutions and change what a
trained net changes:
  channel_rescaled   per-channel powers of two on the residual stream and on each block's inner
                     activation, undone by the next conv's input weights (function preserving);
                     through="var" moves them through the running variance and also rescales conv
                     outputs against mean / var, so the BatchNorm folds see var and mean far from 1, 0
  signed_gamma       negative gamma on half of each block's first BatchNorm
  peaked             policy logits spanning tens of units, tanh near +-1

forward64(..., np.float64) is the reference; forward64(..., np.float32) is the yardstick: the same
plain evaluation in float32, whose error against float64 is what a correct f32 kernel is held to
(measured_bound).  Cases are built once per process (case) and shared by the tests."""
import numpy as np

EPS = 1e-5          # BatchNorm eps (burn's default, tests/golden/make_golden.py)
M = 8               # a correct f32 tower stays within M x the yardstick's own error (see measured_bound)
TOL = {"f32": dict(v=1e-5, prel=1e-4, pabs=1e-8), "bf16": dict(v=2e-2, prel=5e-2, pabs=2e-5)}   # test_gpu_net.TOL
FAMILIES = ("gamma5", "var5", "signed", "peaked", "gamma5+peaked")
KP, KV = 64.0, 32.0
# (blocks, filters, rows) of the GPU tests; one 20x256 case for the ring carry across many convs
SMALL = ((2, 32, 5), (6, 64, 5), (2, 128, 5), (2, 256, 5))
BIG = (20, 256, 3)
# The positions of each net (seed of test_gpu_net.random_planes).  The value is one number per row, so
# the yardstick's max |value error| over 3-5 rows can come out at half an ulp of the output by luck,
# and M times that is then narrower than what float32 allows: on the first positions tried (3 rows at
# 2x256) the yardstick itself, run with its channels in another order, erred up to 14x as much as in
# the plain order.  So the seeds are chosen, on the CPU and from the reference alone, such that the
# yardstick under 8 other summation orders (reordered) stays within M / 4 = 2 times its own error:
# tests/test_netcases.py test_yardstick_is_representative.
PLANES_SEED = {(2, 32): 7003, (6, 64): 7002, (2, 128): 7003, (2, 256): 7001, (20, 256): 7000}
REORDERINGS = 8
SPLIT_SHAPES = SMALL[1:] + (BIG,)


def big_family(dtype):
    """the family of the 20x256 case of test a (see tests/test_gpu_net_structured.py A_CASES)"""
    return "gamma5+peaked" if dtype == "f32" else "gamma5"


def gpu_cases():
    """every (family, blocks, filters, rows) that tests/test_gpu_net_structured.py evaluates through
    AlphaZero.forward"""
    a = [(f,) + s for s in SMALL for f in FAMILIES] + [("gamma5+peaked",) + BIG]
    c = [(f,) + s for s in SPLIT_SHAPES for f in ("gamma3", "gamma5", "gamma8")]
    return sorted(set(a + c), key=lambda t: (t[1] * t[2], t))


def layout(blocks, filters):
    """{name: (offset, shape)} in the flat order of azchess.agent.param_shapes (BatchNorm: rows
    gamma, beta, running mean, running var)"""
    F = filters
    names = [("input_conv.weight", (F, 19, 3, 3)), ("input_conv.bias", (F,)), ("input_bn", (4, F))]
    for b in range(blocks):
        for k in (1, 2):
            names += [("res_blocks.%d.conv%d.weight" % (b, k), (F, F, 3, 3)), ("res_blocks.%d.conv%d.bias" % (b, k), (F,)),
                      ("res_blocks.%d.bn%d" % (b, k), (4, F))]
    names += [("policy_conv_1.weight", (32, F, 1, 1)), ("policy_conv_1.bias", (32,)), ("policy_bn", (4, 32)),
              ("policy_conv_2.weight", (64, 32, 1, 1)), ("policy_conv_2.bias", (64,)),
              ("value_conv.weight", (8, F, 1, 1)), ("value_conv.bias", (8,)), ("value_bn", (4, 8)),
              ("value_linear_1.weight", (512, 64)), ("value_linear_1.bias", (64,)),
              ("value_linear_2.weight", (64, 1)), ("value_linear_2.bias", (1,))]
    out, p = {}, 0
    for name, shape in names:
        out[name] = (p, shape)
        p += int(np.prod(shape))
    out["__size__"] = (p, ())
    return out


def views(flat, blocks, filters):
    """{name: reshaped view into flat} (writing through a view changes flat)"""
    lay = layout(blocks, filters)
    assert flat.ndim == 1 and flat.size == lay["__size__"][0], (flat.shape, lay["__size__"][0])
    return {n: flat[o:o + int(np.prod(s))].reshape(s) for n, (o, s) in lay.items() if n != "__size__"}


def forward64(blocks, filters, w, planes, dtype=np.float64):
    """AlphaZero::forward in numpy, every operation in dtype: planes [N,19,8,8] -> (policy [N,4096],
    value [N]).  im2col conv with padding 1, BatchNorm inference (eps 1e-5), ReLU, residual add,
    softmax over the 64 x 64 logits in channel-major order, tanh."""
    dt = np.dtype(dtype).type
    W = views(np.asarray(w).astype(dt), blocks, filters)
    eps = dt(EPS)

    def conv3(x, name):
        n, c = x.shape[0], x.shape[3]
        xp = np.zeros((n, 10, 10, c), dt)
        xp[:, 1:9, 1:9] = x
        cols = np.stack([xp[:, i:i + 8, j:j + 8, :] for i in range(3) for j in range(3)], axis=3).reshape(n * 64, 9 * c)
        wm = W[name + ".weight"].transpose(2, 3, 1, 0).reshape(9 * c, -1)
        return (cols @ wm + W[name + ".bias"]).reshape(n, 8, 8, -1)

    def conv1(x, name):
        wt = W[name + ".weight"]
        return x @ wt.reshape(wt.shape[0], -1).T + W[name + ".bias"]

    def bn(y, name):
        g, beta, mean, var = W[name]
        return (y - mean) / np.sqrt(var + eps) * g + beta

    def relu(y):
        return np.maximum(y, dt(0))

    x = np.ascontiguousarray(planes).reshape(-1, 19, 8, 8).transpose(0, 2, 3, 1).astype(dt)
    n = x.shape[0]
    x = relu(bn(conv3(x, "input_conv"), "input_bn"))
    for b in range(blocks):
        h = relu(bn(conv3(x, "res_blocks.%d.conv1" % b), "res_blocks.%d.bn1" % b))
        h = bn(conv3(h, "res_blocks.%d.conv2" % b), "res_blocks.%d.bn2" % b)
        x = relu(h + x)
    p = relu(bn(conv1(x, "policy_conv_1"), "policy_bn"))
    z = conv1(p, "policy_conv_2").transpose(0, 3, 1, 2).reshape(n, 4096)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    pol = e / e.sum(axis=1, keepdims=True)
    v = relu(bn(conv1(x, "value_conv"), "value_bn")).transpose(0, 3, 1, 2).reshape(n, 512)
    v = relu(v @ W["value_linear_1.weight"] + W["value_linear_1.bias"])
    val = np.tanh(v @ W["value_linear_2.weight"] + W["value_linear_2.bias"])[:, 0]
    assert pol.dtype == dt and val.dtype == dt
    return pol, val


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), held in float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def forward_bf16(blocks, filters, w, planes):
    """The bf16 towers' arithmetic restated in numpy, for the error scale and not the bits: BatchNorm
    folded into the conv in double and rounded once (net.hip fold_conv), conv weights and every
    stored activation rounded to bf16, float32 accumulation (numpy's order), bias and heads in
    float32 on the bf16 activations."""
    W = views(np.asarray(w, np.float32).astype(np.float64), blocks, filters)

    def fold(name, bnname):
        g, beta, mean, var = W[bnname]
        sc = g / np.sqrt(var + EPS)
        wf = (W[name + ".weight"] * sc.reshape(-1, 1, 1, 1)).astype(np.float32)
        return wf, ((W[name + ".bias"] - mean) * sc + beta).astype(np.float32)

    def conv3(x, name, bnname):
        wf, bf = fold(name, bnname)
        n, c = x.shape[0], x.shape[3]
        xp = np.zeros((n, 10, 10, c), np.float32)
        xp[:, 1:9, 1:9] = x
        cols = np.stack([xp[:, i:i + 8, j:j + 8, :] for i in range(3) for j in range(3)], axis=3).reshape(n * 64, 9 * c)
        return (cols @ bf16_round(wf).transpose(2, 3, 1, 0).reshape(9 * c, -1) + bf).reshape(n, 8, 8, -1)

    def conv1(x, name, bnname):
        wf, bf = fold(name, bnname)
        return np.maximum(x @ wf.reshape(wf.shape[0], -1).T + bf, np.float32(0))

    x = bf16_round(np.ascontiguousarray(planes, np.float32).reshape(-1, 19, 8, 8).transpose(0, 2, 3, 1))
    n = x.shape[0]
    x = bf16_round(np.maximum(conv3(x, "input_conv", "input_bn"), 0))
    for b in range(blocks):
        h = bf16_round(np.maximum(conv3(x, "res_blocks.%d.conv1" % b, "res_blocks.%d.bn1" % b), 0))
        x = bf16_round(np.maximum(conv3(h, "res_blocks.%d.conv2" % b, "res_blocks.%d.bn2" % b) + x, 0))
    f = lambda name: W[name].astype(np.float32)
    p = conv1(x, "policy_conv_1", "policy_bn")
    z = (p @ f("policy_conv_2.weight").reshape(64, 32).T + f("policy_conv_2.bias")).transpose(0, 3, 1, 2).reshape(n, 4096)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    v = conv1(x, "value_conv", "value_bn").transpose(0, 3, 1, 2).reshape(n, 512)
    v = np.maximum(v @ f("value_linear_1.weight") + f("value_linear_1.bias"), 0)
    return e / e.sum(axis=1, keepdims=True), np.tanh(v @ f("value_linear_2.weight") + f("value_linear_2.bias"))[:, 0]


def _draw(rng, spread, n):
    lo, hi = (-spread, spread) if np.isscalar(spread) else spread
    return rng.integers(lo, hi + 1, n)


def channel_rescaled(w, blocks, filters, spread, seed, through="gamma"):
    """w with activation channel c of the residual stream carrying 2^s[c] times its value and of block
    b's inner activation 2^t_b[c] times, exponents integers in [-spread, spread] (or in the pair
    spread = (lo, hi)); the convs that read them divide their input-channel weights by the same power,
    so the network computes the same function.
    through="gamma": gamma and beta of the producing BatchNorm are multiplied: all exact in float32.
    through="var": a random half of each BatchNorm's channels get the factor through
    var' = (var + eps) / 4^k - eps instead of gamma; each other channel, and a random half of the two
    head convs' channels, has its conv output weights, bias and running mean scaled by 2^j,
    var' = (var + eps) 4^j - eps, j in [-5, 5] (function preserving up to the float32 rounding of var')."""
    assert through in ("gamma", "var")
    rng = np.random.default_rng(seed)
    flat = np.asarray(w, np.float32).astype(np.float64)
    W = views(flat, blocks, filters)
    F = filters

    def out_scale(conv, bnname, k):
        """BatchNorm bnname (after conv) emits 2^k times its output"""
        g, beta, mean, var = W[bnname]
        c = g.size
        k = np.zeros(c, np.int64) if k is None else k
        beta *= 2.0 ** k
        if through == "gamma":
            g *= 2.0 ** k
            return
        byvar = (rng.random(c) < 0.5) & (k != 0)
        g[~byvar] *= 2.0 ** k[~byvar]
        var[byvar] = (var[byvar] + EPS) / 4.0 ** k[byvar] - EPS
        j = np.where(byvar, 0, rng.integers(-5, 6, c))
        if bnname in ("policy_bn", "value_bn"):
            j = np.where(rng.random(c) < 0.5, j, 0)
        W[conv + ".weight"][...] *= (2.0 ** j).reshape(-1, 1, 1, 1)
        W[conv + ".bias"][...] *= 2.0 ** j
        mean *= 2.0 ** j
        var[...] = (var + EPS) * 4.0 ** j - EPS
        assert np.all(var > 0)

    def in_scale(conv, k):
        W[conv + ".weight"][...] /= (2.0 ** k).reshape(1, -1, 1, 1)

    s = _draw(rng, spread, F)
    out_scale("input_conv", "input_bn", s)
    for b in range(blocks):
        t = _draw(rng, spread, F)
        pre = "res_blocks.%d." % b
        in_scale(pre + "conv1", s)
        out_scale(pre + "conv1", pre + "bn1", t)
        in_scale(pre + "conv2", t)
        out_scale(pre + "conv2", pre + "bn2", s)
    in_scale("policy_conv_1", s)
    in_scale("value_conv", s)
    if through == "var":
        out_scale("policy_conv_1", "policy_bn", None)
        out_scale("value_conv", "value_bn", None)
    out = flat.astype(np.float32)
    assert np.isfinite(out).all()
    return out


def signed_gamma(w, blocks, filters, seed):
    """gamma negated on a random half of the channels of each block's first BatchNorm (another
    function: compared with forward64 only)"""
    rng = np.random.default_rng(seed)
    flat = np.array(w, np.float32)
    W = views(flat, blocks, filters)
    for b in range(blocks):
        g = W["res_blocks.%d.bn1" % b][0]
        g[rng.random(filters) < 0.5] *= -1
    return flat


def peaked(w, blocks, filters, kp=KP, kv=KV):
    """policy logits x kp (policy_conv_2 weights and bias), value pre-activation x kv (value_linear_2)"""
    flat = np.array(w, np.float32)
    W = views(flat, blocks, filters)
    for name, k in (("policy_conv_2", kp), ("value_linear_2", kv)):
        W[name + ".weight"][...] *= np.float32(k)
        W[name + ".bias"][...] *= np.float32(k)
    return flat


def reordered(w, blocks, filters, seed):
    """the same network with the channels of the residual stream, of every block's inner activation, of
    the policy head and of the value head's hidden layer permuted: the same function, summed in
    another order"""
    rng = np.random.default_rng(seed)
    flat = np.array(w, np.float32)
    W = views(flat, blocks, filters)

    def outp(conv, bnname, p):
        W[conv + ".weight"][...] = W[conv + ".weight"][p]
        W[conv + ".bias"][...] = W[conv + ".bias"][p]
        W[bnname][...] = W[bnname][:, p]

    def inp(conv, p):
        W[conv + ".weight"][...] = W[conv + ".weight"][:, p]

    s = rng.permutation(filters)
    outp("input_conv", "input_bn", s)
    for b in range(blocks):
        t = rng.permutation(filters)
        pre = "res_blocks.%d." % b
        inp(pre + "conv1", s)
        outp(pre + "conv1", pre + "bn1", t)
        inp(pre + "conv2", t)
        outp(pre + "conv2", pre + "bn2", s)
    inp("policy_conv_1", s)
    inp("value_conv", s)
    q = rng.permutation(32)
    outp("policy_conv_1", "policy_bn", q)
    inp("policy_conv_2", q)
    h = rng.permutation(64)
    W["value_linear_1.weight"][...] = W["value_linear_1.weight"][:, h]
    W["value_linear_1.bias"][...] = W["value_linear_1.bias"][h]
    W["value_linear_2.weight"][...] = W["value_linear_2.weight"][h]
    return flat


def family_weights(family, base, blocks, filters):
    """the weights of one family name: gammaK / varK (channel_rescaled, spread K; K = 8 draws from
    [-8, 4]), signed, peaked, or X+peaked"""
    if family.endswith("+peaked"):
        return peaked(family_weights(family[:-7], base, blocks, filters), blocks, filters)
    if family == "base":
        return np.array(base, np.float32)
    if family == "peaked":
        return peaked(base, blocks, filters)
    if family == "signed":
        return signed_gamma(base, blocks, filters, seed=17)
    through = "gamma" if family.startswith("gamma") else "var"
    assert family.startswith(through), family
    k = int(family[len(through):])
    return channel_rescaled(base, blocks, filters, (-8, 4) if k == 8 else k, seed=100 + k, through=through)


def errors(pol, val, rpol, rval):
    """(max |value - ref|, max relative policy error over the entries with ref >= 1e-8)"""
    big = rpol >= 1e-8
    return float(np.abs(val - rval).max()), float((np.abs(pol - rpol)[big] / rpol[big]).max())


def tolerance_use(pol, val, rpol, rval, dtype="f32"):
    """the largest fraction of the project's tolerance (test_gpu_net.check) that any output uses"""
    t = TOL[dtype]
    return max(float(np.abs(val - rval).max()) / t["v"], float((np.abs(pol - rpol) / (t["prel"] * rpol + t["pabs"])).max()))


class Case:
    """weights of one family on one net, positions, the float64 reference and the yardstick's error"""

    def __init__(self, family, blocks, filters, base, planes):
        self.family, self.blocks, self.filters, self.planes = family, blocks, filters, planes
        self.w = family_weights(family, base, blocks, filters)
        self.pol, self.val = forward64(blocks, filters, self.w, planes)
        self.ypol, self.yval = forward64(blocks, filters, self.w, planes, np.float32)
        self.yard_v, self.yard_p = errors(self.ypol, self.yval, self.pol, self.val)
        self.pol.setflags(write=False)
        self.val.setflags(write=False)

    def ratios(self, pol, val):
        """gpu error / yardstick error, (value, policy)"""
        ev, ep = errors(pol, val, self.pol, self.val)
        return ev / self.yard_v, ep / self.yard_p


_cases = {}


def case(family, blocks, filters, rows, base_of, planes_of):
    """the Case of (family, blocks, filters, rows), built on first use; base_of(blocks, filters) and
    planes_of(rows, blocks, filters) supply the init weights and the positions"""
    key = (family, blocks, filters, rows)
    if key not in _cases:
        _cases[key] = Case(family, blocks, filters, base_of(blocks, filters), planes_of(rows, blocks, filters))
    return _cases[key]


def check_tolerance(pol, val, c, dtype):
    """the project's tolerances (test_gpu_net.check) against the float64 reference"""
    t = TOL[dtype]
    assert np.isfinite(pol).all() and np.isfinite(val).all()
    assert np.all(np.abs(val - c.val) <= t["v"]), np.abs(val - c.val).max()
    assert np.all(np.abs(pol - c.pol) <= t["prel"] * c.pol + t["pabs"]), tolerance_use(pol, val, c.pol, c.val, dtype)
    if dtype == "bf16":
        assert np.max(0.5 * np.abs(pol - c.pol).sum(1)) <= 2e-2


def measured_bound(pol, val, c, label, enforce=True):
    """Prints 'gpu error / yardstick error' for value and policy; enforce (the f32 towers): both
    within M = 8.  Why 8: the CPU emulation (tools/split16_numerics.py, -- channel spread) puts a
    correct split-f16 tower at <= 2.4x the f32 error at spread 5 and Winograd f32 at 1x; the statistic
    is a maximum over a few rows and the MFMA's summation order is not numpy's; a tower that flushes
    f16 subnormals sits at >= 10x at spread 3 and ~500x at spread 5."""
    rv, rp = c.ratios(pol, val)
    print("RATIO %-22s %-14s %2dx%-3d value %9.3f  policy %9.3f   (yardstick value %.2e policy %.2e)"
          % (label, c.family, c.blocks, c.filters, rv, rp, c.yard_v, c.yard_p))
    if enforce:
        assert_measured((rv, rp), c)
    return rv, rp


def assert_measured(ratios, c):
    rv, rp = ratios
    assert rv <= M, "value error %.2f x the yardstick's %.2e" % (rv, c.yard_v)
    assert rp <= M, "policy error %.2f x the yardstick's %.2e" % (rp, c.yard_p)
