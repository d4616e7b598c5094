"""Trained-like weights and hard targets for the training-step tests, and the float32 yardstick they
are measured with (numpy / torch-CPU only; reads nothing outside the repository).

azchess.random_weights gives BatchNorm = identity +- 1e-2, a near-uniform policy (policy loss ~
log 4096), small conv biases and float64 gradients that never reach 1: AdamW's value clip never
clamps, the batch mean of every BatchNorm input is ~0 and -q / (p + 1e-5) only sees p ~ 1 / 4096.
The families here are netcases.family_weights (the training layout) plus
  X+peaked(kp,kv)    policy logits x kp, value pre-activation x kv: (8,4) and (16,4) give policy
                     losses of 9 .. 11.5 with p far below 1e-5 on the target moves and a half-saturated
                     tanh.  (netcases' x64 / x32 pins the loss at -log 1e-5 and every gradient at ~0.)
  offsetK            every BatchNorm-fed conv bias = +-2^j, j an integer in [K-2, K]: |batch mean| >>
                     std, where a one-pass E[x^2] - mean^2 variance loses what the two-pass form keeps.
hard_targets puts a third of the rows on a one-hot policy at the move the float64 net rates least
likely and a third on value targets of exactly +-1.

The yardstick is TrainRef(float32) on its own ReLU branches against TrainRef(float64) under the
float32 run's masks (unmasked, branch flips alone give 8e-3 at offset4, 2x32).  NaiveVarRef is the
same step with var = clamp(E[x^2] - mean^2, 0): what the offset cases must be able to tell apart.
ClosedFormRef is the step with the closed-form BatchNorm backward of the HIP kernels."""
import re

import numpy as np
import torch

import netcases as N
import train_ref as T

M = N.M                     # a correct f32 step stays within M x the yardstick's own error on the offset families
GRAD_TOL = 1e-4             # the project's relative-norm tolerance per gradient tensor (tests/test_gpu_train.py)
FAMILIES = ("base", "gamma5", "signed", "gamma5+peaked(8,4)", "gamma5+peaked(16,4)", "offset6", "offset8")
PEAKED = ("gamma5+peaked(8,4)", "gamma5+peaked(16,4)")
OFFSET = ("offset6", "offset8")
CPU_SHAPES = ((2, 32, 16), (6, 64, 8), (2, 128, 8), (2, 256, 4))
WEIGHT_SEED = 42            # azchess.random_weights seed of the base weights (as tests/test_netcases.py)
OFFSET_SEED = 900           # + K: signs and exponents of offsetK
# Seed of test_gpu_train.batch per (blocks, filters, rows).  Chosen on the CPU from the reference alone,
# as netcases.PLANES_SEED was: the first seed from 8000 upwards at which every condition of
# tests/test_traincases.py holds for every family on that shape (yardstick <= 1e-4 / 8 on the non-offset
# families, naive variance >= 32 x the yardstick on the offset ones, peaked policy loss in [9, 11.51)
# and max |value| < 1 - 1e-3).  The shapes that only the GPU tests run take 8000.
BATCH_SEED = {(2, 32, 16): 8000, (6, 64, 8): 8000, (2, 128, 8): 8000, (2, 256, 4): 8000,
              (2, 256, 272): 8000, (20, 256, 2): 8000, (2, 64, 16): 8000, (2, 256, 16): 8000}
# test_gpu_train.test_adamw_and_clipping_bit_exact / test_data_parallel_world2_bit_exact: their nets,
# random_weights seeds, batch seeds and learning-rate iterations, under gamma5+peaked(8,4) and hard targets
CLIP = dict(blocks=2, filters=32, n=16, wseed=3, batch_seeds=(0, 1, 2), its=(5, 13, 1002), family="gamma5+peaked(8,4)")
WORLD2 = dict(blocks=2, filters=64, n=16, wseed=21, batch_seed=22, its=(3, 12), family="gamma5+peaked(8,4)")


def bn_fed_biases(blocks):
    names = ["input_conv.bias", "policy_conv_1.bias", "value_conv.bias"]
    for b in range(blocks):
        names += ["res_blocks.%d.conv1.bias" % b, "res_blocks.%d.conv2.bias" % b]
    return names


def offset(w, blocks, filters, k, seed):
    """every BatchNorm-fed conv bias = +-2^j, j an integer uniform in [k - 2, k], random sign"""
    rng = np.random.default_rng(seed)
    flat = np.array(w, np.float32)
    W = N.views(flat, blocks, filters)
    for name in sorted(bn_fed_biases(blocks)):
        b = W[name]
        b[...] = (rng.choice([-1.0, 1.0], b.size) * 2.0 ** rng.integers(k - 2, k + 1, b.size)).astype(np.float32)
    return flat


def family_weights(family, base, blocks, filters):
    """netcases.family_weights, plus X+peaked(kp,kv) and offsetK"""
    m = re.fullmatch(r"(.+)\+peaked\((\d+),(\d+)\)", family)
    if m:
        return N.peaked(family_weights(m.group(1), base, blocks, filters), blocks, filters, float(m.group(2)), float(m.group(3)))
    if family.startswith("offset"):
        k = int(family[6:])
        return offset(base, blocks, filters, k, OFFSET_SEED + k)
    return N.family_weights(family, base, blocks, filters)


def hard_targets(batch, blocks, filters, w):
    """(planes, policy targets, value targets) of test_gpu_train.batch with rows 0, 3, 6, .. on a
    one-hot policy at the legal move that the float64 net (TrainRef's training-mode forward on these
    weights and this batch) rates least likely -- legal moves: the support of the row's visit
    distribution -- and rows 1, 4, 7, .. on value targets +1, -1, +1, .."""
    planes, tpol, tval = (np.array(a, np.float32) for a in batch)
    with torch.no_grad():
        pol, _ = T.TrainRef(blocks, filters, w).forward(planes)
    pol = pol.numpy()
    for r in range(0, len(tval), 3):
        legal = np.flatnonzero(tpol[r] > 0)
        a = legal[np.argmin(pol[r, legal])]
        tpol[r] = 0
        tpol[r, a] = 1
    for i, r in enumerate(range(1, len(tval), 3)):
        tval[r] = 1.0 if i % 2 == 0 else -1.0
    return planes, tpol, tval


def tensors(blocks, filters):
    """(name, offset, count, exact_zero) per gradient tensor: BatchNorm rows as .gamma / .beta;
    exact_zero marks the BatchNorm-fed conv biases, whose exact gradient is 0"""
    seg, _ = T.segments(blocks, filters)
    zero = set(bn_fed_biases(blocks))
    out = []
    for name, (o, shape, bn) in seg.items():
        if bn:
            C = shape[1]
            out += [(name + ".gamma", o, C, False), (name + ".beta", o + C, C, False)]
        else:
            out.append((name, o, int(np.prod(shape)), name in zero))
    return out


def tensor_errors(g, rg, blocks, filters):
    """{tensor: ||g - rg|| / ||rg||} over the gradient tensors but the BatchNorm-fed biases"""
    g, rg = np.asarray(g, np.float64), np.asarray(rg, np.float64)
    return {name: float(np.linalg.norm(g[o:o + c] - rg[o:o + c]) / max(np.linalg.norm(rg[o:o + c]), 1e-30))
            for name, o, c, zero in tensors(blocks, filters) if not zero}


def worst(errs):
    name = max(errs, key=errs.get)
    return name, errs[name]


def stat_slices(blocks, filters):
    """(running-mean mask, running-variance mask) over the flat parameters"""
    seg, n = T.segments(blocks, filters)
    mean, var = np.zeros(n, bool), np.zeros(n, bool)
    for name, (o, shape, bn) in seg.items():
        if bn:
            C = shape[1]
            mean[o + 2 * C:o + 3 * C] = True
            var[o + 3 * C:o + 4 * C] = True
    return mean, var


def stat_error(p, rs, sel):
    """max |d| / (1 + |ref|) over the selected running statistics"""
    p, rs = np.asarray(p, np.float64)[sel], np.asarray(rs, np.float64)[sel]
    return float((np.abs(p - rs) / (1 + np.abs(rs))).max())


class NaiveVarRef(T.TrainRef):
    """TrainRef with the one-pass variance clamp(E[x^2] - mean^2, 0) in the run's dtype"""

    def _bn(self, x, name):
        mean = x.mean(dim=(0, 2, 3))
        var = ((x * x).mean(dim=(0, 2, 3)) - mean * mean).clamp(min=0)
        rm, rv = self.stats[name]
        self.stats[name] = [rm * 0.9 + mean.detach() * 0.1, rv * 0.9 + var.detach() * 0.1]
        std = torch.sqrt(var + 1e-5)
        y = (x - mean[None, :, None, None]) / std[None, :, None, None]
        return y * self.P[name + ".gamma"][None, :, None, None] + self.P[name + ".beta"][None, :, None, None]


class _ClosedFormBN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, mean, std):
        yhat = (x - mean[None, :, None, None]) / std[None, :, None, None]
        ctx.save_for_backward(yhat, gamma, std)
        return yhat * gamma[None, :, None, None] + beta[None, :, None, None]

    @staticmethod
    def backward(ctx, dz):
        yhat, gamma, std = ctx.saved_tensors
        R = dz.shape[0] * dz.shape[2] * dz.shape[3]
        dbeta = dz.sum(dim=(0, 2, 3))
        dgamma = (dz * yhat).sum(dim=(0, 2, 3))
        dx = (gamma / std)[None, :, None, None] * (dz - (dbeta / R)[None, :, None, None] - yhat * (dgamma / R)[None, :, None, None])
        return dx, dgamma, dbeta, None, None


class ClosedFormRef(T.TrainRef):
    """TrainRef whose BatchNorm backward is the closed form that the HIP step uses, dx = gamma / std
    (dz - mean(dz) - yhat mean(dz yhat)), in place of autograd through mean and variance: the same
    gradient in exact arithmetic (float64: equal to 1e-13); in float32 the sum of dx over the rows,
    the gradient of the conv bias below, cancels only as far as sum(yhat) does"""

    def _bn(self, x, name):
        xd = x.detach()
        mean = xd.mean(dim=(0, 2, 3))
        var = ((xd - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        rm, rv = self.stats[name]
        self.stats[name] = [rm * 0.9 + mean * 0.1, rv * 0.9 + var * 0.1]
        return _ClosedFormBN.apply(x, self.P[name + ".gamma"], self.P[name + ".beta"], mean, torch.sqrt(var + 1e-5))


class Yard:
    """a float32 restatement (cls) on its own ReLU branches against TrainRef(float64) under its masks"""

    def __init__(self, blocks, filters, w, planes, tpol, tval, cls=T.TrainRef):
        y = cls(blocks, filters, w, dtype=torch.float32)
        masks = []
        g, (pl, vl) = y.grads(planes, tpol, tval, record=masks)
        ref = T.TrainRef(blocks, filters, w)
        rg, (rpl, rvl) = ref.grads(planes, tpol, tval, masks)
        self.errs = tensor_errors(g, rg, blocks, filters)
        self.worst_name, self.worst = worst(self.errs)
        self.zero_bias = max(float(np.abs(g[o:o + c]).max()) for _n, o, c, zero in tensors(blocks, filters) if zero)
        self.loss = (abs(pl - rpl) / (1 + abs(rpl)), abs(vl - rvl) / (1 + abs(rvl)))
        self.ref_loss = (rpl, rvl)
        mean, var = stat_slices(blocks, filters)
        ys, rs = y.running_stats_flat(w), ref.running_stats_flat(w)
        self.stat = stat_error(ys, rs, mean | var)
        self.var = stat_error(ys, rs, var)


class Case:
    """weights of one family on one net, a hard-target batch, and (on first use) its yardstick"""

    def __init__(self, family, blocks, filters, base, batch):
        self.family, self.blocks, self.filters = family, blocks, filters
        self.w = family_weights(family, base, blocks, filters)
        self.planes, self.tpol, self.tval = hard_targets(batch, blocks, filters, self.w)
        self.n = len(self.tval)
        for a in (self.w, self.planes, self.tpol, self.tval):
            a.setflags(write=False)
        self._yard = {}

    def yard(self, cls=T.TrainRef):
        if cls not in self._yard:
            self._yard[cls] = Yard(self.blocks, self.filters, self.w, self.planes, self.tpol, self.tval, cls)
        return self._yard[cls]

    def oracle(self, masks=None):
        """(float64 gradient, (policy loss, value loss), flat parameters with the oracle's running statistics)"""
        ref = T.TrainRef(self.blocks, self.filters, self.w)
        rg, losses = ref.grads(self.planes, self.tpol, self.tval, masks)
        return rg, losses, ref.running_stats_flat(self.w)

    def grad_bound(self):
        """what every gradient tensor of a GPU step is held to, under the GPU's masks: the project's
        1e-4; on the offset families M x this case's yardstick worst-tensor error (the float32
        yardstick itself exceeds 1e-4 at offset8)"""
        return M * self.yard().worst if self.family in OFFSET else GRAD_TOL


_cases = {}


def case(family, blocks, filters, n, base_of, batch_of):
    """the Case of (family, blocks, filters, n), built on first use; base_of(blocks, filters) and
    batch_of(n, seed) supply the init weights and test_gpu_train.batch"""
    key = (family, blocks, filters, n)
    if key not in _cases:
        _cases[key] = Case(family, blocks, filters, base_of(blocks, filters), batch_of(n, BATCH_SEED[blocks, filters, n]))
    return _cases[key]


def clip_counts(g):
    """(entries with |g| > 1, of them positive, negative, entries with |g| < 1, size)"""
    g = np.asarray(g)
    return int((np.abs(g) > 1).sum()), int((g > 1).sum()), int((g < -1).sum()), int((np.abs(g) < 1).sum()), g.size


def assert_clip_engages(g):
    """the value clip clamps >= 100 entries, some of each sign, and leaves more than half alone"""
    over, pos, neg, under, size = clip_counts(g)
    assert over >= 100 and pos >= 1 and neg >= 1 and 2 * under > size, (over, pos, neg, under, size)


def world2_counts(gsum):
    """(entries of |g0 + g1| in (1, 2], above 2): the first are clamped by clip(g) / 2 and not by
    clip(g / 2), the second by both"""
    a = np.abs(np.asarray(gsum))
    return int(((a > 1) & (a <= 2)).sum()), int((a > 2).sum())
