"""The oracle's masked median and joint bilateral filter against the plain numpy statements of tests/filters_ref.py, on
the inputs of the GPU filter-limit tests (tests/filter_cases.py): the kernels are pinned to the oracle bit for bit, and
at those radii and sizes the oracle's own paths run nowhere else, so here it answers to something written from the
reference's text alone. No GPU."""
import numpy as np
import pytest

from tests import filter_cases as FC
from tests import filters_ref as R


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle_lib as O

    O.build()
    return O


@pytest.mark.parametrize("radius", FC.MEDIAN_RADII)
@pytest.mark.parametrize("w,h", FC.MEDIAN_SHAPES)
def test_oracle_masked_median_is_the_plain_statement_bit_for_bit(oracle, w, h, radius):
    image, background, mask = FC.median_inputs(w, h)
    for bg in (None, background):
        want = R.masked_median(image, bg, mask, radius)
        assert FC.differing(oracle.masked_median(image, bg, mask, radius), want) == 0, (w, h, radius, bg is not None)


def test_median_inputs_reach_every_rule():
    """Counted from the inputs: even counts (a mean of two), windows without one valid tap (0) and means of -inf and
    +inf (NaN) all occur at both radii, and the plain statement's output shows them."""
    for radius in FC.MEDIAN_RADII:
        for w, h in ((33, 9), (35, 19)):
            image, _, mask = FC.median_inputs(w, h)
            even, empty, cancel = FC.median_census(image, mask, radius)
            assert even > 0 and empty > 0 and cancel > 0, (w, h, radius, even, empty, cancel)
            out = R.masked_median(image, None, mask, radius)
            assert int(np.isnan(out).sum()) == cancel  # NaN taps are skipped: the only NaNs are inf - inf
            assert int(((out == 0) & (mask != 0)).sum()) >= empty


# The largest relative difference |oracle - float64 statement| / |statement| seen per radius over all of the cases below
# (both guide types, six shapes, three sigmas), measured on the CPU:
#
#   radius        0        1        5        8        9       16       22       23       26       65
#   sigma 0.005   0        3.02e-7  1.27e-6  3.13e-6  3.11e-6  1.22e-5  2.34e-5  2.49e-5  3.06e-5  1.94e-4
#   sigma 0.05    0        3.47e-7  2.97e-6  1.17e-5  1.33e-5  1.45e-5  7.31e-5  7.03e-5  6.12e-5  3.09e-4
#   sigma 3e-6    0        2.01e-7  1.04e-6  1.68e-6  3.11e-6  9.10e-6  1.42e-5  1.61e-5  1.60e-5  1.12e-4
#   (2N + 16)/2^24 1.07e-6 2.03e-6  1.54e-5  3.54e-5  4.40e-5  1.31e-4  2.42e-4  2.64e-4  3.36e-4  2.05e-3
#
# The 16-bit and the float guide give the same figures to the digits shown.
OBSERVED = {0: 0.0, 1: 3.47e-7, 5: 2.97e-6, 8: 1.17e-5, 9: 1.33e-5, 16: 1.45e-5, 22: 7.31e-5, 23: 7.04e-5, 26: 6.12e-5,
            65: 3.09e-4}


def bilateral_bound(radius):
    """Four times the largest difference observed at this radius, and never more than what float32 accumulation of
    N = (2 radius + 1)^2 taps can cost in the worst case: two sums of N terms, each term's product and weight rounded,
    a handful of roundings before and after — (2N + 16) * 2^-24. The image is positive, so nothing cancels."""
    n = (2 * radius + 1) ** 2
    return min(4.0 * OBSERVED[radius], (2 * n + 16) * 2.0 ** -24)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("w,h", FC.BILATERAL_SHAPES)
def test_oracle_joint_bilateral_is_the_float64_statement_within_float32_accumulation(oracle, w, h, kind):
    """Measured (the table above): at most 3.09e-4 relative at radius 65 and 7.31e-5 up to radius 26, always under a
    third of the accumulation bound. The image is positive throughout (no NaN: the statement sums over pixels, not over
    taps in order)."""
    image, guide, mask = FC.bilateral_inputs(w, h)
    assert (image > 0).all()
    if kind == "f32":
        guide = guide.astype(np.float32) / np.float32(65535.0)
    for sigma, weights in FC.BILATERAL_SIGMAS:
        statement = R.JointBilateral(guide, mask, sigma, weights, 1 / 65535.0 if kind == "u16" else 1.0)
        for radius in FC.bilateral_radii(w, h):
            want = statement.filter(image, radius)
            got = (oracle.joint_bilateral_u16 if kind == "u16" else oracle.joint_bilateral_f32)(
                image, guide, mask, radius, sigma, *weights)
            rel = float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))
            print("bilateral %s %dx%d sigma %g radius %d: max rel %.3g (bound %.3g)" %
                  (kind, w, h, sigma, radius, rel, bilateral_bound(radius)))
            assert rel <= bilateral_bound(radius), (kind, w, h, sigma, radius, rel)
            assert FC.differing(got[mask == 0], image[mask == 0]) == 0  # outside the mask: the input, untouched


def test_small_sigma_reaches_all_three_ranges_of_expf():
    """The inputs of the third sigma put exponents below -104 (0 returned outright), between -104 and -88 (the
    subnormal results) and above -88 at every radius >= 1 of every shape that is not a single row or column."""
    sigma, weights = FC.BILATERAL_SIGMAS[FC.SMALL_SIGMA]
    for w, h in FC.BILATERAL_SHAPES:
        _, guide, mask = FC.bilateral_inputs(w, h)
        statement = R.JointBilateral(guide, mask, sigma, weights, 1 / 65535.0)
        for radius in (r for r in FC.bilateral_radii(w, h) if r >= 1 and min(w, h) >= 15):
            assert min(statement.exponent_census(radius)) > 0, (w, h, radius, statement.exponent_census(radius))
