"""The MX-fp8 inference mode on the CPU: the host block quantiser az_mx8_quantize against the numpy
statement of the rule (tests/mx8_ref.py) byte for byte, what az_net_create refuses, and the condition
that makes the fp8 tolerance satisfiable: the arithmetic restated in numpy uses at most a quarter of it."""
import numpy as np
import pytest

import azchess as A
import mx8_ref as R
from test_netcases import get_case

FLT_MAX = np.finfo(np.float32).max
TINY = np.finfo(np.float32).tiny          # 2^-126, the smallest normal


def block(*head, fill=0.0):
    b = np.full(32, fill, np.float32)
    b[:len(head)] = head
    return b


def edge_blocks():
    """{name: [k, 32] float32}"""
    p2 = lambda e: np.float32(2.0) ** e
    out = {}
    out["all zero"] = np.stack([np.zeros(32, np.float32), block(-0.0, 0.0, -0.0)])
    out["one non-zero element"] = np.stack([block(1.0), block(0.0, 0.0, 3.7), np.roll(block(-1e-3), 31), block(447.0), block(5e8)])
    out["amax an exact power of two"] = np.stack([block(p2(e), *(p2(e) * np.float32(k) / 16 for k in range(1, 16))) for e in (-30, -7, 0, 1, 8, 9, 40)])
    # scale = amax's power of two / 256: v / scale = 256 v / 2^e; 1.75 -> 448 exactly, above it saturates
    out["v / scale in (448, 512)"] = np.stack([block(1.999, 1.76, 1.751, 1.75, 1.8125, 1.8126, -1.9, 1.7499, 1.0),
                                                 block(*(np.float32(3.5) + np.arange(1, 8, dtype=np.float32) / 16), -3.99),
                                                 block(FLT_MAX, FLT_MAX * np.float32(0.9), -FLT_MAX)])
    # amax = 256 -> scale 1: the values are their own quotients.  e4m3 neighbours: step 2 in [16, 32), 32 in [256, 448]
    out["ties between e4m3 neighbours"] = np.stack([
        block(256.0, 17.0, 19.0, 21.0, 23.0, 272.0, 304.0, 336.0, 9.5, 10.5, 1.0625, 1.1875, -17.0, -19.0),
        block(256.0, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 7 * 2.0 ** -10, 15 * 2.0 ** -10, 17 * 2.0 ** -10, -(2.0 ** -10), -3 * 2.0 ** -10),
        block(256.0, 17.000002, 16.999998, 19.000002, 18.999998, 2.0 ** -10 * 1.0000001, 2.0 ** -10 * 0.9999999)])
    # amax = 1 -> scale 2^-8: 2^-14 is the smallest e4m3 normal (2^-6), 2^-17 the smallest subnormal, below it ties and zeros
    out["e4m3 subnormals"] = np.stack([block(1.0, *(p2(-e) for e in range(12, 22)), 1.5 * 2.0 ** -16, 2.5 * 2.0 ** -17, 7 * 2.0 ** -17, 7.5 * 2.0 ** -17,
                                             -(2.0 ** -15), -(2.0 ** -18), -1.5 * 2.0 ** -17)])
    rng = np.random.default_rng(3)
    out["negative values"] = np.stack([-np.abs(rng.standard_normal(32)).astype(np.float32), block(-1.0, fill=-0.3), block(-448.0, -480.0, -500.0, 100.0)])
    out["amax near FLT_MAX"] = np.stack([block(FLT_MAX, 1e38, 1e30, 1.0, -3e38), block(2.0 ** 127, 2.0 ** 126, -(2.0 ** 119), 2.0 ** 118, 2.0 ** 110)])
    out["amax near the smallest normal"] = np.stack([block(TINY, TINY / 2, -TINY / 4, TINY * 2 ** -23), block(TINY * 1.5, TINY * 0.75), block(TINY * 2 ** -23),
                                                       block(TINY * 2 ** -10, -TINY * 2 ** -12), block(2.0 ** -118, 2.0 ** -119, 2.0 ** -127), block(2.0 ** -117, 2.0 ** -126)])
    x = (rng.standard_normal((1000, 32)) * 2.0 ** rng.uniform(-20, 20, (1000, 1)) * 2.0 ** rng.integers(-3, 1, (1000, 32))).astype(np.float32)
    x[rng.random((1000, 32)) < 0.1] = 0
    out["1000 random blocks spanning 2^+-20"] = x
    return out


@pytest.mark.parametrize("name", list(edge_blocks()))
def test_host_quantiser_equals_the_rule(name):
    """test 1: az_mx8_quantize == mx8_ref.quantize, codes and scale bytes"""
    x = edge_blocks()[name]
    assert np.isfinite(x).all()
    codes, scales = A.mx8_quantize(x)
    rcodes, rscales = R.quantize(x)
    assert np.array_equal(scales, rscales), (name, scales[:8], rscales[:8])
    assert np.array_equal(codes, rcodes), (name, np.argwhere(codes != rcodes)[:8])
    # the edge each family is there for is reached
    q = np.abs(x).astype(np.float64) / 2.0 ** (rscales.astype(np.float64) - 127)[:, None]
    if name == "all zero":
        assert np.all(scales == 127) and np.all(codes & 0x7F == 0)
    if name == "v / scale in (448, 512)":
        assert ((q > 448) & (q < 512)).sum() >= 10 and np.all((codes & 0x7F)[q > 448] == 0x7E)
    if name == "e4m3 subnormals":
        c = codes & 0x7F
        assert ((c > 0) & (c < 8)).sum() >= 5 and (c[0, 1:17] == 0).any()
    if name == "amax near the smallest normal":
        assert scales.min() == 0
    if name == "amax near FLT_MAX":
        assert scales.max() == 246
    # no code is the e4m3fn NaN
    assert np.all(codes & 0x7F != 0x7F)


def test_quantiser_error_is_the_formats():
    """dequantised values within half an e4m3 step of the input (2^-4 relative for normals), except above 448 x scale"""
    x = edge_blocks()["1000 random blocks spanning 2^+-20"]
    codes, scales = A.mx8_quantize(x)
    d = R.dequantize(codes, scales)
    sc = 2.0 ** (scales.astype(np.float64) - 127)[:, None]
    q = np.abs(x) / sc
    ok = q <= 448
    assert np.all(np.abs(d - x)[ok] <= np.maximum(np.abs(x)[ok] * 2.0 ** -4, (sc * 2.0 ** -10).repeat(32, 1)[ok]))
    assert np.all(np.abs(d)[~ok] == (448 * sc).repeat(32, 1)[~ok])


@pytest.mark.parametrize("filters", [64, 32])
def test_fp8_refuses_small_filters(filters):
    """test 2: az_net_create(AZ_DTYPE_FP8) at 64 / 32 filters fails, and says which filters it supports"""
    with pytest.raises(A._lib.AzError) as e:
        A.AlphaZero(2, filters, dtype="fp8")
    assert "128" in str(e.value) and "256" in str(e.value)


def test_fp8_has_only_the_fused_kernel(monkeypatch):
    monkeypatch.setenv("AZ_FUSED_TOWER", "0")
    with pytest.raises(A._lib.AzError) as e:
        A.AlphaZero(2, 128, dtype="fp8")
    assert "fused" in str(e.value)


def test_unknown_dtype_string_raises():
    for bad in ("fp16", "float32", "", None):
        with pytest.raises(ValueError):
            A.AlphaZero(2, 32, dtype=bad)
    assert A._lib.DTYPE_FP8 == 2


@pytest.mark.parametrize("family,blocks,filters,rows", R.CASES)
def test_fp8_tolerance_is_satisfiable(family, blocks, filters, rows):
    """test 3: the arithmetic restated in numpy (mx8_ref.forward_mx8) against float64 uses at most a
    quarter of the fp8 tolerance on every case the GPU test enforces"""
    c = get_case(family, blocks, filters, rows)
    pol, val = R.mx8_of(c)
    ev, ep, tv = R.stats(pol, val, c.pol, c.val)
    use = R.tolerance_use(pol, val, c.pol, c.val)
    print("%-8s %2dx%-3d mx8 restated in numpy: value %.3e policy rel %.3e total variation %.3e, %.0f %% of the fp8 tolerance"
          % (family, blocks, filters, ev, ep, tv, 100 * use))
    R.check_tolerance(pol, val, c.pol, c.val)
    assert use <= 0.25


def test_fp8_tolerance_constants_are_four_times_the_restatement():
    """TOL_FP8 = 4 x the largest error of forward_mx8 over CASES, rounded up to one significant digit"""
    worst = np.zeros(3)
    for family, blocks, filters, rows in R.CASES:
        c = get_case(family, blocks, filters, rows)
        worst = np.maximum(worst, R.stats(*R.mx8_of(c), c.pol, c.val))

    def round_up(x):
        e = 10.0 ** np.floor(np.log10(x))
        return np.ceil(x / e - 1e-9) * e
    for got, w in zip((R.TOL_FP8["v"], R.TOL_FP8["prel"], R.TOL_FP8["tv"]), worst):
        assert np.isclose(got, round_up(4 * w)), (got, 4 * w)
    assert R.TOL_FP8["pabs"] == 2e-5
