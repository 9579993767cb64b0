"""The image filters around the depth kernels at their radius and size edges, every one against the oracle bit for bit
(NaN == NaN, +0 != -0, no tolerance anywhere in this file): the joint bilateral filter on partial tiles, images narrower
than a tile and radii larger than the image, at the radii where its tile's row pitch equals its width (0, 8, 16), at the
largest radius whose tile fits in LDS (22) and past it (23, 26, 65: the untiled kernel), with exponents on both sides of
expf's |x| >= 88 branches; the masked median's general branch (radius 2) and both branches on +-0, +-inf, NaN and ties;
Lanczos and masked upsamples of sources smaller than their support; the foreground mask and the SSIM blur on images
smaller than their kernels. Inputs: tests/filter_cases.py. Where a case exists to reach a branch, numpy shows from the
input that it does. The oracle itself answers to plain numpy statements at these cases in tests/test_filters_ref.py."""
import numpy as np
import pytest

from tests import common
from tests import filter_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig(built):
    from facebook360_dep_amd import synth

    n, res, _ = synth.config("tiny")
    return synth.make_rig(n, res)


@pytest.fixture(scope="module")
def gpu(rig):
    from facebook360_dep_amd import derp

    g = derp.Derp(rig["cameras"], partial_coverage=1)
    yield g
    g.close()


# ---- joint bilateral ------------------------------------------------------------------------------------------------
def _bilateral(kind, gpu):
    from oracle import oracle_lib as O

    return (O.joint_bilateral_u16, gpu.joint_bilateral_u16) if kind == "u16" else (O.joint_bilateral_f32,
                                                                                   gpu.joint_bilateral_f32)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("w,h", FC.BILATERAL_SHAPES)
def test_joint_bilateral_every_radius_and_partial_tiles(gpu, w, h, kind):
    from tests import filters_ref as R

    want_fn, got_fn = _bilateral(kind, gpu)
    image, guide, mask = FC.bilateral_inputs(w, h)
    assert 0 < int(mask.sum()) < mask.size or mask.size == 1
    factor = 1 / 65535.0
    if kind == "f32":
        guide, factor = guide.astype(np.float32) / np.float32(65535.0), 1.0
    for i, (sigma, weights) in enumerate(FC.BILATERAL_SIGMAS):
        if i == FC.SMALL_SIGMA and min(w, h) >= 15:
            # the exponents this sigma exists for: 0 outright, subnormal results, ordinary ones — already at radius 1
            assert min(R.JointBilateral(guide, mask, sigma, weights, factor).exponent_census(1)) > 0
        for radius in FC.bilateral_radii(w, h):
            want = want_fn(image, guide, mask, radius, sigma, *weights)
            got = got_fn(image, guide, mask, radius, sigma, *weights)
            n = FC.differing(got, want)
            print("bilateral %s %dx%d sigma %g radius %d: %d differ" % (kind, w, h, sigma, radius, n))
            assert n == 0, (kind, w, h, sigma, radius, n)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_joint_bilateral_spreads_nan_like_the_reference(gpu, kind):
    """A NaN image value poisons every pixel whose window holds it, whatever its weight (0 * NaN): three isolated NaN
    pixels give at most 3 * 121 of 1650 NaN outputs at radius 5."""
    want_fn, got_fn = _bilateral(kind, gpu)
    image, guide, mask, spots = FC.bilateral_nan_inputs()
    assert all(mask[y, x] and np.isnan(image[y, x]) for y, x in spots) and int(np.isnan(image).sum()) == 3
    if kind == "f32":
        guide = guide.astype(np.float32) / np.float32(65535.0)
    for radius in (1, 5):
        want = want_fn(image, guide, mask, radius, 0.005, 0.5, 1.0, 1.0)
        share = float(np.isnan(want).mean())
        assert 0 < share <= 0.25, (radius, share)
        got = got_fn(image, guide, mask, radius, 0.005, 0.5, 1.0, 1.0)
        assert FC.differing(got, want) == 0, (kind, radius, FC.differing(got, want))


# ---- masked median --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", FC.MEDIAN_RADII)
@pytest.mark.parametrize("w,h", FC.MEDIAN_SHAPES)
def test_masked_median_both_radii_on_special_values(gpu, w, h, radius):
    from oracle import oracle_lib as O

    image, background, mask = FC.median_inputs(w, h)
    if (w, h) in ((33, 9), (35, 19)):
        even, empty, cancel = FC.median_census(image, mask, radius)
        assert even > 0 and empty > 0 and cancel > 0, (even, empty, cancel)
        assert np.signbit(image[image == 0]).any() and not np.signbit(image[image == 0]).all()
        want = O.masked_median(image, None, mask, radius)
        assert int(np.isnan(want).sum()) == cancel and int(((want == 0) & (mask != 0)).sum()) >= empty
    for bg in (None, background):
        want = O.masked_median(image, bg, mask, radius)
        got = gpu.masked_median(image, bg, mask, radius)
        assert FC.differing(got, want) == 0, (w, h, radius, bg is not None, FC.differing(got, want))


def test_masked_median_refuses_radius_3(gpu):
    from facebook360_dep_amd import derp

    image, _, mask = FC.median_inputs(9, 1)
    for radius in (0, 3):
        with pytest.raises(derp.DerpError, match="radius must be 1 or 2"):
            gpu.masked_median(image, None, mask, radius)


# ---- upsample -------------------------------------------------------------------------------------------------------
UPSAMPLE_SHAPES = [  # source (w, h), result (w, h)
    ((3, 2), (12, 8)),  # smaller than the 8 taps of Lanczos4 either way
    ((7, 5), (35, 25)),  # scale 5: a spiral of radius 26, larger than the result
    ((40, 30), (100, 40)),  # anisotropic
    ((50, 50), (51, 51)),
]


@pytest.mark.parametrize("src,dst", UPSAMPLE_SHAPES)
def test_upsample_small_sources_and_long_spirals(gpu, rig, src, dst):
    from oracle import oracle_lib as O

    _, rd, _ = common.oracle_rigs(rig)
    (sw, sh), (dw, dh) = src, dst
    rng = np.random.default_rng([5, sw, sh])
    disp = (1.0 / rng.uniform(0.6, 30.0, size=(sh, sw))).astype(np.float32)
    disp[rng.random((sh, sw)) < 0.1] = np.nan
    bg_up = (rng.random((dh, dw)).astype(np.float32) + 2.0)
    one = np.zeros((sh, sw), np.uint8)
    one[sh // 2, sw // 2] = 1  # a single coarse foreground pixel: the spiral travels as far as it can
    cases = [("lanczos", disp, None, None), ("lanczos, all NaN", np.full_like(disp, np.nan), None, None),
             ("masked", disp, (rng.random((sh, sw)) > 0.4).astype(np.uint8),
              (rng.random((dh, dw)) > 0.3).astype(np.uint8)),
             ("masked, one pixel", np.nan_to_num(disp, nan=0.5), one, np.ones((dh, dw), np.uint8)),
             ("masked, all NaN", np.full_like(disp, np.nan), np.ones((sh, sw), np.uint8), np.ones((dh, dw), np.uint8)),
             ("masked, fg empty", disp, np.zeros((sh, sw), np.uint8), np.ones((dh, dw), np.uint8)),
             ("masked, fg_up empty", disp, np.ones((sh, sw), np.uint8), np.zeros((dh, dw), np.uint8))]
    for name, image, fg, fg_up in cases:
        args = () if fg is None else (bg_up, fg, fg_up)
        want = O.upsample_disparity(rd, 1, image, dw, dh, *args)
        got = gpu.upsample_disparity(1, image, dw, dh, *args)
        assert FC.differing(got, want) == 0, (name, src, dst, FC.differing(got, want))
        if name == "lanczos, all NaN":
            assert not np.isnan(want).any()  # NaN -> the smallest disparity before the resize
        if name in ("masked, all NaN", "masked, fg empty", "masked, fg_up empty"):
            assert FC.differing(got, bg_up) == 0, name  # the spiral finds nothing anywhere: the background
        if name == "masked, one pixel":
            assert (want != bg_up).any()


# ---- foreground mask ------------------------------------------------------------------------------------------------
def _fg_inputs(w, h):
    rng = np.random.default_rng([6, w, h])
    yy, xx = np.mgrid[0:h, 0:w]
    template = np.stack([(xx * 900 + yy * 400) % 65536, (xx * 300 + yy * 1100 + 9000) % 65536,
                         (xx * 500 + yy * 500) % 65536], axis=-1).astype(np.int64)
    frame = template + rng.integers(-600, 600, size=template.shape)
    blob = ((yy - h // 2) ** 2 + (xx - w // 2) ** 2 <= (min(w, h) // 3) ** 2) | (rng.random((h, w)) < 0.03)
    frame[blob] = frame[blob] // 2 + 9000
    return template.astype(np.uint16), np.clip(frame, 0, 65535).astype(np.uint16)


@pytest.mark.parametrize("w,h", [(37, 21), (5, 4)])
def test_foreground_mask_kernels_larger_than_the_image(gpu, w, h):
    """Blur 0-3 (a 7 x 7 kernel on 5 x 4: BORDER_REFLECT_101 bounces more than once) and closing sizes 0, 1, 4 and 9."""
    from facebook360_dep_amd import derp
    from oracle import oracle_lib as O

    template, frame = _fg_inputs(w, h)
    seen = set()
    for blur in (0, 1, 2, 3):
        for morph in (0, 1, 4, 9):
            want = O.generate_foreground_mask(template, frame, blur, 0.04, morph)
            got = gpu.generate_foreground_mask(template, frame, blur, 0.04, morph)
            assert np.array_equal(got, want), (w, h, blur, morph, int((got != want).sum()))
            seen.add(want.tobytes())
            assert 0 < int(want.sum()) < want.size or morph == 9 or (w, h) == (5, 4), (blur, morph)
    assert len(seen) > 4  # the options matter on these inputs
    with pytest.raises(derp.DerpError, match=r"blur_radius must be 0\.\.3"):
        gpu.generate_foreground_mask(template, frame, 4, 0.04, 4)


# ---- SSIM -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(40, 9), (9, 40), (3, 3)])
def test_ssim_blur_radii_up_to_the_limit(gpu, w, h):
    """Radii 4, 7 and 15 of the accepted 1..15: on 9 rows or 3 x 3 the blur reflects several times."""
    from facebook360_dep_amd import derp
    from oracle import oracle_lib as O

    rng = np.random.default_rng([11, w, h])
    x = rng.random((h, w, 3), dtype=np.float32)
    y = np.clip(x + 0.1 * rng.standard_normal(x.shape).astype(np.float32), 0, 1).astype(np.float32)
    y[:2, :2] = 0  # a flat corner: sigma = 0 on one side
    for radius in (4, 7, 15):
        for abg in ((1, 1, 1), (0, 0, 1)):
            want = O.compute_ssim(x, y, radius, *abg)
            got = gpu.ssim(x, y, radius, *abg)
            assert FC.differing(got, want) == 0, (w, h, radius, abg, FC.differing(got, want))
    with pytest.raises(derp.DerpError, match=r"blur_radius must be 1\.\.15"):
        gpu.ssim(x, y, 16)
