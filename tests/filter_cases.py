"""Seeded inputs of the filter-limit tests, shared by the GPU test (kernels against the oracle,
tests/test_gpu_filter_limits.py) and the CPU one (the oracle against tests/filters_ref.py, tests/test_filters_ref.py),
with the numpy censuses that show a case reaches the branch it exists for. Test infrastructure only."""
import numpy as np

# ---- joint bilateral -----------------------------------------------------------------------------------------------
BILATERAL_SHAPES = [(1, 1), (1, 37), (37, 1), (15, 17), (33, 50), (48, 32)]  # w, h
# 0, 8, 16: the tile's row pitch equals its width; 22: the largest tile that fits in LDS; 23 and above: no tile
BILATERAL_RADII = [0, 1, 5, 8, 9, 16, 22, 23, 26]
BILATERAL_RADIUS_65_SHAPES = [(15, 17), (33, 50)]  # 1024 -> 8192 through UpsampleDisparity: scale^2 + 1
# sigma, (weight0, weight1, weight2). The third: one grey level is 1 / 65535, so differences of 1, 2, 3 and 4 levels in
# every channel give exponents of about -10.8, -43, -97 and -172: both sides of expf's |x| >= 88 test, and both sides of
# its flush to zero below -103.97.
BILATERAL_SIGMAS = [(0.005, (0.5, 1.0, 1.0)), (0.05, (0.5, 0.5, 1.0)), (3e-6, (0.5, 1.0, 1.0))]
SMALL_SIGMA = 2


def bilateral_radii(w, h):
    return BILATERAL_RADII + ([65] if (w, h) in BILATERAL_RADIUS_65_SHAPES else [])


def bilateral_inputs(w, h, seed=0):
    """-> image f32 (positive), guide u16 [h, w, 3], mask u8. The guide: a ramp of one level per pixel on the left,
    flat patches on the right, a few levels of noise on everything, texels at 0 and 65535; the mask: about 10 % zeros
    and one fully masked block with a single unmasked pixel inside it."""
    rng = np.random.default_rng([seed, w, h])
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.where(xx < w // 2, 20000 + xx + yy, 30000 + 7000 * ((xx // 5 + yy // 4) % 3))
    guide = base[..., None] + rng.integers(-2, 3, size=(h, w, 3))
    ends = rng.random((h, w))
    guide[ends < 0.03] = 0
    guide[ends > 0.97] = 65535
    guide = guide.astype(np.uint16)
    image = (1.0 / rng.uniform(0.6, 30.0, size=(h, w))).astype(np.float32)
    mask = (rng.random((h, w)) > 0.1).astype(np.uint8)
    by, bx = h // 3, w // 3
    mask[by:by + 7, bx:bx + 7] = 0
    mask[min(by + 3, h - 1), min(bx + 3, w - 1)] = 1
    return image, guide, mask


def bilateral_nan_inputs():
    """33 x 50 with three isolated NaN pixels at masked-in positions -> image, guide, mask, the three (y, x)."""
    image, guide, mask = bilateral_inputs(33, 50, seed=1)
    spots = [(6, 25), (24, 8), (41, 20)]
    image = image.copy()
    for y, x in spots:
        mask[y, x] = 1
        image[y, x] = np.nan
    return image, guide, mask, spots


# ---- masked median -------------------------------------------------------------------------------------------------
MEDIAN_SHAPES = [(1, 1), (1, 9), (9, 1), (33, 9), (35, 19)]  # w, h
MEDIAN_RADII = [1, 2]


def median_inputs(w, h, seed=0):
    """-> image, background, mask. Values on 8 levels (+-0.25 .. +-1), so ties and even counts are the rule, with +0,
    -0, NaN, +inf and -inf sprinkled in; the mask is half zeros. Where the image is large enough, two planted windows:
    an unmasked -0 alone in a masked 5 x 5 block (nothing valid -> 0), and +inf beside -inf alone in one (NaN)."""
    rng = np.random.default_rng([seed, w, h])
    levels = np.array([-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0], dtype=np.float32)
    image = levels[rng.integers(0, 8, size=(h, w))]
    kind = rng.random((h, w))
    image[kind < 0.06] = 0.0
    image[(kind >= 0.06) & (kind < 0.12)] = -0.0
    image[(kind >= 0.12) & (kind < 0.18)] = np.nan
    image[(kind >= 0.18) & (kind < 0.26)] = np.inf
    image[(kind >= 0.26) & (kind < 0.34)] = -np.inf
    mask = (rng.random((h, w)) < 0.5).astype(np.uint8)
    if w >= 33 and h >= 9:
        mask[2:7, 8:13] = 0
        mask[4, 10] = 1
        image[4, 10] = -0.0
        mask[2:7, 20:25] = 0
        mask[4, 22] = mask[4, 23] = 1
        image[4, 22], image[4, 23] = np.inf, -np.inf
    background = rng.random((h, w)).astype(np.float32) + 2.0
    return image, background, mask


def median_census(image, mask, radius):
    """-> the number of masked-in pixels whose window holds an even number (> 0) of valid taps, no valid tap at all,
    and an even number whose two middle values are -inf and +inf."""
    h, w = image.shape
    even = empty = cancel = 0
    for y in range(h):
        for x in range(w):
            if not mask[y, x]:
                continue
            vals = sorted(float(image[j, i]) for j in range(max(y - radius, 0), min(y + radius, h - 1) + 1)
                          for i in range(max(x - radius, 0), min(x + radius, w - 1) + 1)
                          if mask[j, i] and not np.isnan(image[j, i]) and image[j, i] != 0)
            n = len(vals)
            empty += n == 0
            even += n > 0 and n % 2 == 0
            cancel += n > 0 and n % 2 == 0 and vals[n // 2 - 1] == -np.inf and vals[n // 2] == np.inf
    return even, empty, cancel


def differing(a, b):
    """the number of elements whose bits differ (so +0 is not -0), any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape
    return int((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).sum())
