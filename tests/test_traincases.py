"""tests/traincases.py on the CPU, from the oracle alone: the conditions on weights, batches and
seeds under which the bounds of tests/test_gpu_train_structured.py mean something -- a plain float32
step fits the project's gradient tolerance with room on the non-offset families, a one-pass variance
cannot fit the offset bound, the peaked heads are neither uniform nor saturated, and AdamW's value
clip clamps on the batches that tests/test_gpu_train.py feeds it."""
import numpy as np
import pytest
import torch

import azchess as A
import traincases as C
import train_ref as T
from test_gpu_train import batch


def base_of(blocks, filters):
    return A.random_weights(blocks, filters, seed=C.WEIGHT_SEED)


_batches = {}


def batch_of(n, seed):
    if (n, seed) not in _batches:
        _batches[n, seed] = batch(n, seed)
    return _batches[n, seed]


def get_case(family, blocks, filters, n):
    return C.case(family, blocks, filters, n, base_of, batch_of)


def clip_inputs():
    """weights and the three hard-target batches of test_gpu_train.test_adamw_and_clipping_bit_exact"""
    k = C.CLIP
    w = C.family_weights(k["family"], A.random_weights(k["blocks"], k["filters"], seed=k["wseed"]), k["blocks"], k["filters"])
    return w, [C.hard_targets(batch(k["n"], seed=s), k["blocks"], k["filters"], w) for s in k["batch_seeds"]]


def world2_inputs():
    """weights and the 2 x 16 hard-target rows of test_gpu_train.test_data_parallel_world2_bit_exact"""
    k = C.WORLD2
    w = C.family_weights(k["family"], A.random_weights(k["blocks"], k["filters"], seed=k["wseed"]), k["blocks"], k["filters"])
    return w, C.hard_targets(batch(2 * k["n"], seed=k["batch_seed"]), k["blocks"], k["filters"], w)


def test_record_returns_the_runs_own_masks():
    """record= changes nothing, and feeding the recorded masks back reproduces the run"""
    blocks, filters, n = 2, 32, 4
    w = base_of(blocks, filters)
    planes, tpol, tval = batch_of(n, 8000)
    g0, l0 = T.TrainRef(blocks, filters, w).grads(planes, tpol, tval)
    masks = []
    g1, l1 = T.TrainRef(blocks, filters, w).grads(planes, tpol, tval, record=masks)
    assert np.array_equal(g0, g1) and l0 == l1
    assert [m.shape for m in masks] == [(n, filters, 8, 8)] * (2 * blocks + 1) + [(n, 40, 8, 8), (n, 64)]
    assert all(m.dtype == bool and m.any() and not m.all() for m in masks)
    again = []
    g2, l2 = T.TrainRef(blocks, filters, w).grads(planes, tpol, tval, masks, record=again)
    assert np.array_equal(g0, g2) and l0 == l2
    assert all(np.array_equal(a, b) for a, b in zip(masks, again))


def test_families_and_hard_targets():
    blocks, filters, n = 2, 32, 16
    base = base_of(blocks, filters)
    V0 = C.N.views(base, blocks, filters)
    for k in (6, 8):
        V = C.N.views(C.family_weights("offset%d" % k, base, blocks, filters), blocks, filters)
        for name in V:
            if name in C.bn_fed_biases(blocks):
                j = np.log2(np.abs(V[name].astype(np.float64)))
                assert np.array_equal(j, np.round(j)) and j.min() >= k - 2 and j.max() <= k, name
                assert (V[name] > 0).any() and (V[name] < 0).any() or V[name].size <= 8, name
            else:
                assert np.array_equal(V[name], V0[name]), name
    g5 = C.family_weights("gamma5", base, blocks, filters)
    pk = C.N.views(C.family_weights("gamma5+peaked(8,4)", base, blocks, filters), blocks, filters)
    G = C.N.views(g5, blocks, filters)
    assert np.array_equal(pk["policy_conv_2.weight"], 8 * G["policy_conv_2.weight"])
    assert np.array_equal(pk["value_linear_2.bias"], 4 * G["value_linear_2.bias"])
    assert np.array_equal(pk["input_bn"], G["input_bn"])
    c = get_case("gamma5+peaked(8,4)", blocks, filters, n)
    planes, tpol, tval = batch_of(n, C.BATCH_SEED[blocks, filters, n])
    assert np.array_equal(c.planes, planes)
    with torch.no_grad():
        pol = T.TrainRef(blocks, filters, c.w).forward(planes)[0].numpy()
    for r in range(n):
        if r % 3 == 0:
            a = np.flatnonzero(c.tpol[r])
            assert a.size == 1 and c.tpol[r, a[0]] == 1 and tpol[r, a[0]] > 0
            assert pol[r, a[0]] == pol[r, tpol[r] > 0].min() and pol[r, a[0]] < 1e-5
        else:
            assert np.array_equal(c.tpol[r], tpol[r])
        if r % 3 == 1:
            assert c.tval[r] == (1.0 if (r // 3) % 2 == 0 else -1.0)
        else:
            assert c.tval[r] == tval[r]


@pytest.mark.parametrize("blocks,filters,n", C.CPU_SHAPES)
@pytest.mark.parametrize("family", [f for f in C.FAMILIES if f not in C.OFFSET])
def test_yardstick_has_headroom(family, blocks, filters, n):
    """a plain float32 step uses at most 1 / M of the project's 1e-4 per gradient tensor (seen: <= 5.2e-6)"""
    y = get_case(family, blocks, filters, n).yard()
    print("%-20s %2dx%-3d n %2d yardstick worst tensor %.2e (%s), losses %.1e %.1e, statistics %.1e, bn-fed biases %.1e"
          % (family, blocks, filters, n, y.worst, y.worst_name, y.loss[0], y.loss[1], y.stat, y.zero_bias))
    assert 0 < y.worst <= C.GRAD_TOL / C.M
    assert y.zero_bias <= 1e-5 / C.M


@pytest.mark.parametrize("blocks,filters,n", C.CPU_SHAPES)
@pytest.mark.parametrize("family", C.OFFSET)
def test_offset_cases_reject_a_one_pass_variance(family, blocks, filters, n):
    """var = E[x^2] - mean^2 in float32 errs at least 4 x the bound that the GPU step is held to
    (M x the yardstick): a condition on the inputs (seen: naive / yardstick >= 380)"""
    c = get_case(family, blocks, filters, n)
    y, nv = c.yard(), c.yard(C.NaiveVarRef)
    print("%-8s %2dx%-3d n %2d yardstick %.2e (%s) running statistics %.1e; one-pass variance %.2e (%s) running variance %.1e; ratio %.0f"
          % (family, blocks, filters, n, y.worst, y.worst_name, y.stat, nv.worst, nv.worst_name, nv.var, nv.worst / y.worst))
    assert y.worst > 0 and nv.worst >= 4 * (C.M * y.worst)
    assert c.grad_bound() == C.M * y.worst
    assert nv.var >= 4 * (C.M * y.stat)          # the running variance tells them apart too
    assert y.zero_bias <= 1e-5 / C.M


@pytest.mark.parametrize("family,blocks,filters,n", [("gamma5", 2, 32, 16)] + [("offset8",) + s for s in C.CPU_SHAPES])
def test_closed_form_bn_backward_leaves_bias_noise_at_large_means(family, blocks, filters, n):
    """Why the HIP step does not sum dY for the bias gradient of a conv in front of a BatchNorm
    (test_gpu_train_structured.test_bn_fed_bias_gradients_vanish):
    a float32 restatement with the closed-form BatchNorm backward (the HIP step's form for dY) equals
    autograd in float64 and keeps every other gradient tensor at the yardstick's error, but its
    BatchNorm-fed bias gradients, exactly 0, come out above 1e-5 where |mean| >> std (seen at
    offset8: 2.9e-5 .. 1.0e-4, autograd's <= 4e-7; at offset6, not asserted here: 1.0e-5 .. 1.6e-5; on
    gamma5 both 1e-7)."""
    c = get_case(family, blocks, filters, n)
    y, cf = c.yard(), c.yard(C.ClosedFormRef)
    g64, _ = C.ClosedFormRef(blocks, filters, c.w).grads(c.planes, c.tpol, c.tval)
    a64, _, _ = c.oracle()
    same = C.worst(C.tensor_errors(g64, a64, blocks, filters))[1]
    print("%-8s %2dx%-3d closed-form float32: worst tensor %.2e (autograd %.2e), bn-fed biases %.2e (autograd %.2e); float64 closed form vs autograd %.1e"
          % (family, blocks, filters, cf.worst, y.worst, cf.zero_bias, y.zero_bias, same))
    assert same <= 1e-11
    assert cf.worst <= 2 * y.worst
    if family in C.OFFSET:
        assert cf.zero_bias > 1e-5 > C.M * y.zero_bias
    else:
        assert cf.zero_bias <= 1e-5 / C.M


@pytest.mark.parametrize("blocks,filters,n", C.CPU_SHAPES)
@pytest.mark.parametrize("family", C.PEAKED)
def test_peaked_heads_are_neither_uniform_nor_saturated(family, blocks, filters, n):
    c = get_case(family, blocks, filters, n)
    y = c.yard()
    with torch.no_grad():
        pol, val = T.TrainRef(blocks, filters, c.w).forward(c.planes)
    pl = y.ref_loss[0]
    print("%-20s %2dx%-3d policy loss %.3f value loss %.3f max |v| %.5f, yardstick loss errors %.1e %.1e"
          % (family, blocks, filters, pl, y.ref_loss[1], float(val.abs().max()), y.loss[0], y.loss[1]))
    assert 9 <= pl < 11.51
    assert float(val.abs().max()) < 1 - 1e-3
    assert max(y.loss) <= 1e-5
    assert float(pol[c.tpol > 0].min()) < 1e-5       # -q / (p + 1e-5) with p below the 1e-5


def test_clipping_case_clamps():
    """the batches of test_adamw_and_clipping_bit_exact: the float64 gradient has >= 100 entries
    beyond +-1, of both signs, and more than half inside -- on the first step and, stepping with
    the float32 AdamW restatement, on the two after it"""
    k = C.CLIP
    w, batches = clip_inputs()
    mask = T.trainable_mask(k["blocks"], k["filters"])
    p, m, v = w.copy(), np.zeros_like(w), np.zeros_like(w)
    for step, ((planes, tpol, tval), it) in enumerate(zip(batches, k["its"])):
        ref = T.TrainRef(k["blocks"], k["filters"], p)
        g, _ = ref.grads(planes, tpol, tval)
        print("clip case step %d: |g| > 1: %d (+%d / -%d), |g| < 1: %d of %d; max |g| %.1f" % ((step,) + C.clip_counts(g) + (np.abs(g).max(),)))
        C.assert_clip_engages(g)
        p = ref.running_stats_flat(p).astype(np.float32)
        p, m, v = T.adamw_step(p, g.astype(np.float32), m, v, mask, step + 1, T.cyclical_lr(it))


def test_world2_case_tells_the_clip_orders_apart():
    """the halves of test_data_parallel_world2_bit_exact: |g0 + g1| has >= 100 entries in (1, 2]
    (clamped by clip(g) / 2, not by clip(g / 2)) and >= 100 above 2, on both of its steps; on such
    entries the two orders give different parameters"""
    k = C.WORLD2
    w, (planes, tpol, tval) = world2_inputs()
    n = k["n"]
    mask = T.trainable_mask(k["blocks"], k["filters"])
    p, m, v = w.copy(), np.zeros_like(w), np.zeros_like(w)
    for step, it in enumerate(k["its"]):
        refs = [T.TrainRef(k["blocks"], k["filters"], p) for _ in range(2)]
        gs = [ref.grads(planes[r * n:(r + 1) * n], tpol[r * n:(r + 1) * n], tval[r * n:(r + 1) * n])[0] for r, ref in enumerate(refs)]
        mid, high = C.world2_counts(gs[0] + gs[1])
        print("world-2 case step %d: |g0 + g1| in (1, 2]: %d, above 2: %d, of %d" % (step, mid, high, gs[0].size))
        assert mid >= 100 and high >= 100
        gsum = (gs[0] + gs[1]).astype(np.float32)
        lr = T.cyclical_lr(it)
        right, m1, v1 = T.adamw_step(p, gsum, m, v, mask, step + 1, lr, world=2)
        wrong, _, _ = T.adamw_step(p, np.clip(gsum, -1, 1), m, v, mask, step + 1, lr, world=2)
        assert (right != wrong).sum() >= 100
        st = ~mask
        right[st] = ((refs[0].running_stats_flat(p)[st] + refs[1].running_stats_flat(p)[st]) * 0.5).astype(np.float32)
        p, m, v = right, m1, v1
