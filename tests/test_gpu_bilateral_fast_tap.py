"""The joint bilateral filter's fast tap (k_joint_bilateral<true, true>: unit second and third weights, expf with the one
range test an argument in [-inf, -0] needs, no mask reads in a block whose staged tile is all set) against the oracle, bit
for bit, beside the generic tap on the same inputs; and the reduced range test alone against the full expf on the device.
NaN == NaN, +0 != -0, no tolerance anywhere in this file."""
import numpy as np
import pytest

from tests import filter_cases as FC

pytestmark = pytest.mark.gpu

FAST = (0.5, 1.0, 1.0)     # the level loop's weights: the host picks the fast tap
GENERIC = (0.5, 0.7, 1.3)  # same sum, so the same exponents: the generic tap
# sigma 3e-6 (tests/filter_cases.py): a difference of 1, 2, 3, 4 grey levels in every channel gives an exponent of about
# -10.8, -43, -97, -172 with either weight triple (both sum to 2.5); 0.005 is the level loop's
SIGMAS = (3e-6, 0.005)
SHAPES = [(33, 19), (3, 3)]  # w, h; the second is smaller than every radius but 1
T88, TFLUSH = np.float32(-88.0), np.float32(float.fromhex("-0x1.9fe368p6"))


@pytest.fixture(scope="module")
def gpu(built):
    from facebook360_dep_amd import derp, synth

    n, res, _ = synth.config("tiny")
    g = derp.Derp(synth.make_rig(n, res)["cameras"], partial_coverage=1)
    yield g
    g.close()


def inputs(w, h):
    """image f32, guide u16 [h, w, 3]: neighbours differ by 0..5 grey levels, the same in every channel, so that the taps'
    exponents at sigma 3e-6 land on both sides of -88 and of the flush to zero"""
    rng = np.random.default_rng([14, w, h])
    steps = rng.integers(0, 6, size=(h, w))
    guide = np.repeat((30000 + steps)[..., None], 3, axis=2).astype(np.uint16)
    image = (1.0 / rng.uniform(0.6, 30.0, size=(h, w))).astype(np.float32)
    return image, guide


def masks(w, h):
    """all set; about 10 % holes; a cleared 16 x 16 tile beside tiles that stay full (at 33 wide the third tile column
    stages nothing of the cleared tile at any radius <= 5)"""
    rng = np.random.default_rng([15, w, h])
    full = np.ones((h, w), np.uint8)
    holes = (rng.random((h, w)) > 0.1).astype(np.uint8)
    tile = full.copy()
    tile[:16, :16] = 0
    return {"all_set": full, "holes": holes, "cleared_tile": tile}


def exponents(guide, sigma, weights):
    """the expf arguments of the horizontal-neighbour taps, as the kernel forms them in fp32"""
    g = guide.astype(np.float32) * np.float32(1 / 65535.0)
    d = g[:, 1:] - g[:, :-1]
    w0, w1, w2 = (np.float32(v) for v in weights)
    cds = w0 * (d[..., 0] * d[..., 0]) + w1 * (d[..., 1] * d[..., 1]) + w2 * (d[..., 2] * d[..., 2])
    denom = np.float32(2.0) * (np.float32(sigma) * np.float32(sigma))
    return (-cds / np.float32(3.0)) / denom


def test_inputs_reach_both_sides_of_the_range_tests():
    _, guide = inputs(*SHAPES[0])
    for weights in (FAST, GENERIC):
        x = exponents(guide, SIGMAS[0], weights)
        assert (x > T88).any() and ((x <= T88) & (x >= TFLUSH)).any() and (x < TFLUSH).any() and (x == 0).any()


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("weights", [FAST, GENERIC], ids=["fast", "generic"])
def test_fast_and_generic_tap_equal_the_oracle(gpu, w, h, weights):
    from oracle import oracle_lib as O

    image, guide = inputs(w, h)
    for name, mask in masks(w, h).items():
        for sigma in SIGMAS:
            for radius in (1, 2, 3, 4, 5):
                want = O.joint_bilateral_u16(image, guide, mask, radius, sigma, *weights)
                got = gpu.joint_bilateral_u16(image, guide, mask, radius, sigma, *weights)
                n = FC.differing(got, want)
                print("%dx%d %s sigma %g radius %d weights %s: %d differ" % (w, h, name, sigma, radius, weights, n))
                assert n == 0, (w, h, name, sigma, radius, weights, n)


def test_filter_changes_something(gpu):
    """the comparisons above are not of an identity: at the level loop's sigma the filter moves most pixels"""
    image, guide = inputs(*SHAPES[0])
    got = gpu.joint_bilateral_u16(image, guide, masks(*SHAPES[0])["all_set"], 5, 0.005, *FAST)
    assert FC.differing(got, image) > image.size // 2


def _around(value, ulps=65536):
    """the floats within `ulps` of `value` that lie in [-inf, -0]"""
    centre = int(np.array(value, np.float32).view(np.uint32))
    bits = np.arange(centre - ulps, centre + ulps + 1, dtype=np.int64)
    bits = bits[(bits >= 0x80000000) & (bits <= 0xFF800000)]  # sign set, not NaN
    return bits.astype(np.uint32).view(np.float32)


def test_reduced_range_test_equals_the_full_expf(gpu):
    fmax = np.finfo(np.float32).max
    rng = np.random.default_rng(360)
    x = np.concatenate([
        _around(-88.0), _around(TFLUSH), _around(-0.0), _around(-fmax), _around(-np.inf),
        np.arange(0x80000001, 0x80800000, dtype=np.uint32).view(np.float32),  # every negative denormal
        rng.integers(0x80000000, 0xFF800001, size=10**7, dtype=np.int64).astype(np.uint32).view(np.float32),
    ])
    assert not np.isnan(x).any() and np.signbit(x).all()
    assert (x == -np.inf).any() and (x == 0).any() and (x < TFLUSH).any() and ((x > TFLUSH) & (x < T88)).any()
    full = gpu.debug_expf(x)
    reduced = gpu.debug_expf(x, nonpos=True)
    n = FC.differing(reduced, full)
    print("expf: %d arguments, %d differ" % (x.size, n))
    assert n == 0
    # and the full routine is the expf it claims to be where that is easy to say: exact zeros below the flush, 1 at -0
    assert (full[x < TFLUSH] == 0).all() and not np.signbit(full[x < TFLUSH]).any()
    assert (full[x == 0] == 1).all() and (full[x >= -100] > 0).all()
