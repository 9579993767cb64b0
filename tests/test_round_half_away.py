"""The cost core's two-instruction roundf, round_half_away_pos (csrc/derp_kernels.h): trunc(x + pred(0.5)) with one
round-to-nearest fp32 add, restated in numpy, against roundf = floor(x + 0.5) in float64 on its domain (-0.5, 2^23).
tests/test_gpu_cost_trims.py runs the same inputs through the device's instructions."""
import numpy as np

PRED_HALF = np.float32(float.fromhex("0x1.fffffep-2"))  # the float just below 0.5
TWO23 = 0x4B000000  # bit pattern of 2^23
MINUS_HALF = 0xBF000000  # bit pattern of -0.5


def helper(x):
    """round_half_away_pos as the device evaluates it: float32 add (round to nearest even), then trunc"""
    x = np.asarray(x, dtype=np.float32)
    s = x + PRED_HALF
    assert s.dtype == np.float32
    return np.trunc(s)


def roundf(x):
    """roundf (half away from zero) for x >= 0, exact in float64: x + 0.5 is exact there for every float below 2^52"""
    return np.floor(np.asarray(x, dtype=np.float32).astype(np.float64) + 0.5).astype(np.float32)


def _bits(lo, hi, step=1):
    return np.arange(lo, hi, step, dtype=np.uint32).view(np.float32)


def near_halves(ulps=64, kmax=2 * 8200):
    """every float within `ulps` ulps of k / 2, k = 0 .. kmax (for k = 0: the floats 0 .. `ulps` ulps)"""
    k = np.arange(1, kmax + 1, dtype=np.float64) / 2
    centre = k.astype(np.float32).view(np.uint32).astype(np.int64)
    pats = (centre[:, None] + np.arange(-ulps, ulps + 1)[None, :]).reshape(-1)
    zero = np.arange(0, ulps + 1, dtype=np.int64)
    return np.concatenate([zero, pats]).astype(np.uint32).view(np.float32)


def negative_side(stride=257, ulps=64):
    """(-0.5, 0): -0, a strided sweep, and the `ulps` floats next to each end (-0.5 itself excluded)"""
    lo = 0x80000000
    sweep = np.arange(lo, MINUS_HALF, stride, dtype=np.uint32)
    ends = np.concatenate([np.arange(lo, lo + ulps + 1, dtype=np.uint32),
                           np.arange(MINUS_HALF - ulps, MINUS_HALF, dtype=np.uint32)])
    return np.concatenate([sweep, ends]).view(np.float32)


def boundary_set():
    """the inputs the device test shares: near the halves, a strided sweep of [0, 2^23), and (-0.5, 0)"""
    return np.concatenate([near_halves(), _bits(0, TWO23, 257 * 16), negative_side(257 * 16)])


def _same(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def test_near_every_half():
    x = near_halves()
    assert x.size == 2 * 8200 * 129 + 65
    assert (x >= 0).all()
    assert _same(helper(x), roundf(x)) == 0


def test_every_float_from_a_quarter_to_one():
    x = _bits(0x3E800000, 0x3F800000)
    assert x[0] == 0.25 and x[-1] < 1.0 and x.size == 2 << 23
    assert _same(helper(x), roundf(x)) == 0


def test_strided_sweep_below_two_to_23():
    x = _bits(0, TWO23, 257)
    assert x[0] == 0.0 and x[-1] < 2.0 ** 23 and x.size > 4_800_000
    assert _same(helper(x), roundf(x)) == 0
    # the last floats of the domain (spacing 0.5 below 2^23), and 2^23 itself, where the sum is still exact
    top = _bits(TWO23 - 4096, TWO23 + 1)
    assert _same(helper(top), roundf(top)) == 0


def test_negative_side_gives_a_zero():
    x = negative_side()
    assert ((x > -0.5) & (x <= 0)).all() and x.size > 4_000_000
    h = helper(x)
    assert (h == 0).all()
    # roundf's -0 for these, and what the callers form from the result is the same for either zero
    assert (np.round(x.astype(np.float64)) == 0).all()
    assert (h.astype(np.int32) == 0).all()
    assert _same(x - h + np.float32(0.5), x - np.float32(0.0) + np.float32(0.5)) == 0


def test_minus_a_half_is_outside_the_domain():
    x = np.array([-0.5], dtype=np.float32)
    assert helper(x)[0] == 0 and np.signbit(helper(x)[0])
    assert np.float32(-1.0) == -np.floor(0.5 + 0.5)  # roundf(-0.5) = -1: half away from zero
    assert helper(x)[0] != -1.0
    # below it the two part for good: -0.75 -> -0 against -1, -1.5 -> -1 against -2 (ssd_arith's !exact path keeps roundf)
    y = np.array([-0.75, -1.5], dtype=np.float32)
    assert (helper(y) == np.array([0.0, -1.0], dtype=np.float32)).all()


def test_nan_in_nan_out():
    assert np.isnan(helper(np.array([np.nan], dtype=np.float32))[0])
