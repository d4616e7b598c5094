"""agent.rs mirror: AlphaZero network (conv tower + policy/value heads) on libaz.

Weights use the flat f32 layout of include/az.h (burn module order, DESIGN.md "Weights").
`random_weights` is the synthetic random init used by the benchmarks and tests: burn's
default KaimingUniform (gain 1/sqrt(3) => U(-1/sqrt(fan_in), 1/sqrt(fan_in))) for conv and
linear weights and biases (agent.rs:59-84 via burn Conv2dConfig/LinearConfig), BatchNorm
gamma=1, beta=0, running mean 0, var 1, plus a seeded 1e-2 perturbation so that the BN fold
is exercised.
"""
import ctypes as C
import os

import numpy as np

from . import _lib as L
from .parameters import NUM_FILTERS, NUM_RES_BLOCKS, SEED


def num_params(blocks, filters):
    return int(L.lib.az_net_num_params(int(blocks), int(filters)))


def param_shapes(blocks, filters):
    """(name, shape, fan_in or None for BatchNorm) in flat order."""
    F = filters
    out = [("input_conv.weight", (F, 19, 3, 3), 19 * 9), ("input_conv.bias", (F,), 19 * 9),
           ("input_bn", (4, F), None)]
    for b in range(blocks):
        for k in (1, 2):
            out += [("res_blocks.%d.conv%d.weight" % (b, k), (F, F, 3, 3), F * 9),
                    ("res_blocks.%d.conv%d.bias" % (b, k), (F,), F * 9),
                    ("res_blocks.%d.bn%d" % (b, k), (4, F), None)]
    out += [("policy_conv_1.weight", (32, F, 1, 1), F), ("policy_conv_1.bias", (32,), F), ("policy_bn", (4, 32), None),
            ("policy_conv_2.weight", (64, 32, 1, 1), 32), ("policy_conv_2.bias", (64,), 32),
            ("value_conv.weight", (8, F, 1, 1), F), ("value_conv.bias", (8,), F), ("value_bn", (4, 8), None),
            ("value_linear_1.weight", (512, 64), 512), ("value_linear_1.bias", (64,), 512),
            ("value_linear_2.weight", (64, 1), 64), ("value_linear_2.bias", (1,), 64)]
    return out


def random_weights(blocks=NUM_RES_BLOCKS, filters=NUM_FILTERS, seed=SEED, bn_perturb=1e-2):
    rng = np.random.default_rng(seed)
    parts = []
    for _name, shape, fan_in in param_shapes(blocks, filters):
        if fan_in is None:
            c = shape[1]
            g = 1.0 + bn_perturb * rng.uniform(-1, 1, c)
            beta = bn_perturb * rng.uniform(-1, 1, c)
            mean = bn_perturb * rng.uniform(-1, 1, c)
            var = 1.0 + bn_perturb * rng.uniform(-1, 1, c)
            parts.append(np.concatenate([g, beta, mean, var]).astype(np.float32))
        else:
            bound = 1.0 / np.sqrt(fan_in)
            parts.append(rng.uniform(-bound, bound, int(np.prod(shape))).astype(np.float32))
    flat = np.concatenate(parts)
    assert flat.size == num_params(blocks, filters)
    return flat


def load_mpk(path, blocks=NUM_RES_BLOCKS, filters=NUM_FILTERS):
    """NamedMpkFileRecorder::<FullPrecisionSettings>::new().load(path) (main.rs:109-116):
    the record's tensors in the flat layout of include/az.h."""
    out = np.empty(num_params(blocks, filters), np.float32)
    L.check(L.lib.az_net_load_mpk(str(path).encode(), int(blocks), int(filters), L.fptr(out), out.size))
    return out


def save_mpk(path, weights, blocks=NUM_RES_BLOCKS, filters=NUM_FILTERS):
    """model.save_file(path, &NamedMpkFileRecorder::<FullPrecisionSettings>) (training.rs:269-270)."""
    w = np.ascontiguousarray(weights, np.float32)
    L.check(L.lib.az_net_save_mpk(str(path).encode(), int(blocks), int(filters), L.fptr(w), w.size))


# the evaluation precisions of include/az.h: f32 (the reference's), and the opt-in bf16 and MX-fp8 modes
DTYPES = {"f32": L.DTYPE_F32, "bf16": L.DTYPE_BF16, "fp8": L.DTYPE_FP8}


def load_model(path, blocks=NUM_RES_BLOCKS, filters=NUM_FILTERS, dtype="f32", device=0):
    """main.rs:109-116: AlphaZero::new().load_record(record)."""
    return AlphaZero(blocks, filters, weights=load_mpk(path, blocks, filters), dtype=dtype, device=device)


class AlphaZero:
    """AlphaZero::new / forward (agent.rs:49-144) with weights resident in HBM."""

    def __init__(self, blocks=NUM_RES_BLOCKS, filters=NUM_FILTERS, weights=None, dtype="f32", device=0,
                 seed=SEED):
        if dtype not in DTYPES:
            raise ValueError("dtype must be one of %s, not %r" % (", ".join(sorted(DTYPES)), dtype))
        if weights is None:
            weights = random_weights(blocks, filters, seed)
        self._weights = np.ascontiguousarray(weights, np.float32)
        self.blocks, self.filters = blocks, filters
        self.dtype = dtype
        desc = L.AzNetDesc(blocks, filters, DTYPES[dtype])
        h = C.c_void_p()
        L.check(L.lib.az_net_create(C.byref(desc), L.fptr(self._weights), self._weights.size, device, C.byref(h)))
        self._h = h
        # libaz runs the fused tower kernel unless AZ_FUSED_TOWER=0 (an fp8 net has no other: creation fails)
        self.fused_tower = os.environ.get("AZ_FUSED_TOWER", "1") != "0"

    @property
    def weights(self):
        """The flat f32 parameters this net evaluates: the creator's host copy, or after an update the
        net's own device copy, read back on first use (az_net_get_weights)."""
        if self._weights is None:
            out = np.empty(num_params(self.blocks, self.filters), np.float32)
            L.check(L.lib.az_net_get_weights(self._h, L.fptr(out), out.size))
            self._weights = out
        return self._weights

    @property
    def generation(self):
        """0 after creation, + 1 for each update / update_from."""
        return int(L.check(L.lib.az_net_generation(self._h)))

    def update(self, weights):
        """Replace the weights in place from host parameters (a checkpoint, an arena opponent): one
        upload, then the BatchNorm fold and every packed layout rebuilt by kernels on the device
        (az_net_update).  Searches on this net set their roots again (or reset) before they run."""
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        L.check(L.lib.az_net_update(self._h, L.fptr(w), w.size))
        self._weights = None
        return self

    def update_from(self, trainer):
        """model.valid() (training.rs:83): take the trainer's current device parameters, device to device
        (az_net_update_from_trainer)."""
        L.check(L.lib.az_net_update_from_trainer(self._h, trainer._h))
        self._weights = None
        return self

    def packed(self, kind, index=0):
        """Test hook (az_net_packed_read): the bytes of one packed weight buffer, kind one of
        _lib.PACKED_KINDS; None for a buffer this net does not hold."""
        k = L.PACKED_KINDS.index(kind)
        n = L.check(L.lib.az_net_packed_read(self._h, k, int(index), None, 0))
        if n == 0:
            return None
        out = np.empty(n, np.uint8)
        L.check(L.lib.az_net_packed_read(self._h, k, int(index), out.ctypes.data_as(C.c_void_p), n))
        return out

    @property
    def tower_kernel(self):
        """Which kernel evaluates this net (libaz's choice: fused f32 Winograd / f32 direct / bf16 / MX-fp8)."""
        buf = C.create_string_buffer(128)
        L.check(L.lib.az_net_tower_kernel(self._h, buf, 128))
        return buf.value.decode()

    @property
    def wino_streamed_points(self):
        """Winograd points per 32 input channels whose weights the split-f16 tower streams (16, or 12
        with the third row derived: AZ_WINO_DERIVE); 0 when another kernel evaluates this net."""
        return L.check(L.lib.az_net_wino_streamed_points(self._h))

    @property
    def wino_accumulators(self):
        """Winograd-domain accumulators per output fragment of the split-f16 tower: 8 in the row-direct
        form (AZ_WINO_ROWS: Winograd across columns, the tap rows direct), 16 otherwise; 0 when
        another kernel evaluates this net."""
        return L.check(L.lib.az_net_wino_accumulators(self._h))

    @property
    def wino_v_rows(self):
        """1 where the row-direct tower stores every row of its transformed input once (AZ_WINO_VROWS), else 0."""
        return L.check(L.lib.az_net_wino_v_rows(self._h))

    @property
    def wino_boards(self):
        """Batch rows per workgroup of the split-f16 tower: 2 where the shared-row form runs two boards on one
        weight stream (AZ_WINO_BOARDS=2), else 1; 0 when another kernel evaluates this net."""
        return L.check(L.lib.az_net_wino_boards(self._h))

    @property
    def winograd(self):
        return "Winograd" in self.tower_kernel

    def __del__(self):
        try:
            L.lib.az_net_destroy(self._h)
        except Exception:
            pass

    def save_file(self, path):
        save_mpk(path, self.weights, self.blocks, self.filters)

    def forward(self, x):
        """x: [N,19,8,8] float32 -> (policy [N,4096] softmax, value [N] tanh)."""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 19 * 64)
        n = x.shape[0]
        pol = np.zeros((n, 4096), np.float32)
        val = np.zeros(n, np.float32)
        L.check(L.lib.az_net_forward(self._h, L.fptr(x), n, L.fptr(pol), L.fptr(val)))
        return pol, val


def wino_vrows_layout():
    """az_wino_vrows_layout: the shared-row V layout's address tables (include/az.h), tabulated from the
    kernel's own formulas; needs no device."""
    t = dict(write=np.empty((16, 64, 4), np.int32), read=np.empty((2, 4, 4, 64), np.int32),
             act=np.empty((16, 64, 4), np.int32), item=np.empty((2, 8, 4), np.int32), dims=np.empty(4, np.int32))
    L.check(L.lib.az_wino_vrows_layout(*(t[k].ctypes.data_as(C.c_void_p) for k in ("write", "read", "act", "item", "dims"))))
    return t


def wino_boards_layout():
    """az_wino_boards_layout: the two-board tower's item schedule, global activation offsets, epilogue
    addresses and LDS regions (include/az.h), tabulated from the kernel's own constants; needs no device."""
    t = dict(item=np.empty((8, 8, 2), np.int32), act=np.empty((2, 2), np.int32), out=np.empty((8, 64, 2, 4), np.int32),
             vbuf=np.empty((2, 2), np.int32), zero=np.empty(64, np.int32), dims=np.empty(8, np.int32))
    L.check(L.lib.az_wino_boards_layout(*(t[k].ctypes.data_as(C.c_void_p) for k in ("item", "act", "out", "vbuf", "zero", "dims"))))
    return t


def mx8_quantize(x):
    """az_mx8_quantize, the MX-fp8 mode's host block quantiser: x float32, a multiple of 32 values in
    blocks of 32 consecutive ones -> (e4m3fn codes uint8 of x's shape, E8M0 scale bytes uint8 [blocks])."""
    x = np.ascontiguousarray(x, np.float32)
    if x.size % 32:
        raise ValueError("mx8_quantize: %d values are not whole blocks of 32" % x.size)
    codes = np.empty(x.shape, np.uint8)
    scales = np.empty(x.size // 32, np.uint8)
    u8 = lambda a: a.ctypes.data_as(L.P(C.c_uint8))
    L.check(L.lib.az_mx8_quantize(L.fptr(x), x.size // 32, u8(codes), u8(scales)))
    return codes, scales


def mx8_conv_probe(filters, act_codes, act_scales, w_codes, w_scales, bias, residual=None, device=0):
    """az_mx8_conv_probe (test hook): one residual conv layer of tower8_kernel.  act_codes [n,64,F] /
    act_scales [n,64,F/32] uint8, w_codes [F,F,3,3] / w_scales [F,9,F/32] uint8, bias [F] float32,
    residual [n,64,F] bf16 bits (uint16) or None -> dict(acc float32 [n,64,F], codes, scales, and with a
    residual bf16 = the output's bf16 bits)."""
    F = int(filters)
    a = np.ascontiguousarray(act_codes, np.uint8)
    n = a.size // (64 * F)
    s = np.ascontiguousarray(act_scales, np.uint8)
    wc, wsc = np.ascontiguousarray(w_codes, np.uint8), np.ascontiguousarray(w_scales, np.uint8)
    b = np.ascontiguousarray(bias, np.float32)
    if a.size != n * 64 * F or s.size != n * 64 * F // 32 or wc.size != F * F * 9 or wsc.size != F * 9 * F // 32 or b.size != F:
        raise ValueError("mx8_conv_probe: operand shapes do not match filters = %d" % F)
    r = None if residual is None else np.ascontiguousarray(residual, np.uint16)
    if r is not None and r.size != a.size:
        raise ValueError("mx8_conv_probe: residual shape")
    out = dict(acc=np.empty((n, 64, F), np.float32), codes=np.empty((n, 64, F), np.uint8),
               scales=np.empty((n, 64, F // 32), np.uint8))
    if r is not None:
        out["bf16"] = np.empty((n, 64, F), np.uint16)
    u8 = lambda x: x.ctypes.data_as(L.P(C.c_uint8))
    u16 = lambda x: None if x is None else x.ctypes.data_as(L.P(C.c_uint16))
    L.check(L.lib.az_mx8_conv_probe(int(device), F, n, u8(a), u8(s), u8(wc), u8(wsc), u16(r), L.fptr(b), L.fptr(out["acc"]),
                                    u16(out.get("bf16")), u8(out["codes"]), u8(out["scales"])))
    return out
