"""Plain numpy statements of the two simplest image filters, written from the reference's text and not from the
oracle's restatement of it, so that the oracle itself has something independent to answer to at the edges no full-size
run reaches (median radius 2, bilateral radii far larger than the image). Test infrastructure only.

  masked_median    cv_util::maskedMedianBlur (CvUtil.h:336-385), exact: selection and the mean of two floats in double
                   have one answer each, so the oracle must match it bit for bit.
  joint_bilateral  generalizedJointBilateralFilter (TemporalBilateralFilter.h:39-124) in float64 throughout. The
                   reference works in float32 in a fixed tap order; this statement says what the filter computes, not
                   how it rounds, and is compared within a bound (tests/test_filters_ref.py)."""
import numpy as np


def masked_median(image, background, mask, radius):
    """-> float32 [h, w]. Per pixel inside the mask: the taps of the (2 radius + 1)^2 window that are in bounds, inside
    the mask, not NaN and not 0 (CvUtil.h:354-369); odd count -> the middle value, even count -> (a + b) / 2.0 of the
    two middle values, the sum in float and the quotient in double (CvUtil.h:373-380). No such tap -> 0. Outside the
    mask: the background, or 0 without one (CvUtil.h:342-350)."""
    image = np.asarray(image, dtype=np.float32)
    mask = np.asarray(mask).astype(bool)
    h, w = image.shape
    out = np.zeros((h, w), dtype=np.float32)
    for y in range(h):
        for x in range(w):
            if not mask[y, x]:
                if background is not None:
                    out[y, x] = background[y, x]
                continue
            y0, y1, x0, x1 = max(y - radius, 0), min(y + radius, h - 1), max(x - radius, 0), min(x + radius, w - 1)
            win = image[y0:y1 + 1, x0:x1 + 1][mask[y0:y1 + 1, x0:x1 + 1]]
            vals = np.sort(win[~np.isnan(win) & (win != 0)])
            if vals.size:
                n = vals.size // 2
                if vals.size % 2 == 1:
                    out[y, x] = vals[n]
                else:
                    with np.errstate(invalid="ignore"):  # (+inf) + (-inf)
                        out[y, x] = np.float32(np.float64(np.float32(vals[n - 1] + vals[n])) / 2.0)
    return out


def scaled_guide(guide, factor):
    """guideColor * guideFactor as the reference's types make it: a float product (TemporalBilateralFilter.h:77,94),
    hence rounded to float32 before anything in this file happens in float64. It matters for a 16-bit guide only, and
    there only when sigma is so small that single grey levels decide the weights: with sigma = 3e-6 the exact quotient
    g / 65535 moves the results by up to 4.8e-3 relative, which is the conditioning of the filter on its input and not
    an error of either side. A float guide times 1 is itself."""
    return (np.asarray(guide, dtype=np.float32) * np.float32(factor)).astype(np.float64)


def clamp_counts(n, radius):
    """-> int64 [n, n]: how many of the offsets -radius .. radius take coordinate i to j once clamped to 0 .. n - 1
    (math_util::clamp of the sample coordinates, TemporalBilateralFilter.h:82-83): an edge pixel is sampled once for
    every offset that points past it."""
    count = np.zeros((n, n), dtype=np.int64)
    i = np.arange(n)
    for d in range(-radius, radius + 1):
        count[i, np.clip(i + d, 0, n - 1)] += 1
    return count


class JointBilateral:
    """The filter for one guide, mask, sigma and set of weights, in float64. Every tap (u, v) of pixel p samples the
    pixel q at the clamped coordinates, so p's sums run over all pixels q, each taken as often as taps land on it:
    clamp_counts along y times clamp_counts along x. In float64 the order of the sum is of no account, and the weights
    exp((-colorDiffSq / 3) / (2 sigma^2)) (TemporalBilateralFilter.h:91-105) of all pairs are computed once.
    `factor` = 1 / maxPixelValue(guide): 1 / 65535 for a 16-bit guide, 1 for a float one."""

    def __init__(self, guide, mask, sigma, weights, factor):
        self.mask = np.asarray(mask).astype(bool)
        self.h, self.w = self.mask.shape
        flat = scaled_guide(guide, factor).reshape(-1, 3)
        sigma = np.float64(np.float32(sigma))
        sq = 0.0
        for c in range(3):
            diff = flat[:, None, c] - flat[None, :, c]
            sq = sq + np.float64(weights[c]) * (diff * diff)
        self.exponent = -sq / 3.0 / (2.0 * sigma * sigma)  # [pixel p, pixel q]
        m = self.mask.reshape(-1)
        self.live = m[:, None] & m[None, :]  # masked taps are skipped, masked pixels pass through (:68-71, :85-87)
        with np.errstate(under="ignore"):
            self.weight = np.where(self.live, np.exp(self.exponent), 0.0)

    def taps(self, radius):
        """-> int64 [pixel p, pixel q]: the number of p's (2 radius + 1)^2 taps that sample q"""
        cy, cx = clamp_counts(self.h, radius), clamp_counts(self.w, radius)
        n = self.h * self.w
        return (cy[:, None, :, None] * cx[None, :, None, :]).reshape(n, n)

    def filter(self, image, radius):
        """-> float64 [h, w]"""
        image = np.asarray(image, dtype=np.float64)
        weight = self.taps(radius) * self.weight
        total = weight.sum(axis=1).reshape(image.shape)
        acc = (weight @ image.reshape(-1)).reshape(image.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.mask & (total != 0.0), acc / total, image)

    def exponent_census(self, radius):
        """-> the number of unmasked taps whose exponent lies in (-inf, -104), (-104, -88) and (-88, 0]: the first is
        where expf returns 0 outright, the second where its result is subnormal, the third the ordinary one."""
        taps = np.where(self.live, self.taps(radius), 0)
        e = self.exponent
        return tuple(int(taps[sel].sum()) for sel in (e < -104, (e > -104) & (e < -88), e > -88))
