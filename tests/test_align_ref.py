"""The AlignColors restatement (tests/align_ref.py) without a GPU: every named case of tests/align_cases.py really
contains what it is there for, distortionMax agrees with numpy's polynomial roots, and a geometry check that does not
rest on restating the reference: a pattern rendered through the three channel models comes out of the alignment with
red and blue on green, within the bilinear interpolation bound."""
import math

import numpy as np
import pytest

from tests import align_cases as AC
from tests import align_ref as R

CASES = AC.all_cases()


def _infos(case, cam_index=0, double_ratio=False):
    """the branch masks of camera `cam_index`'s two maps -> (green model, red info, blue info, red map, blue map)"""
    cam = AC.selected(case)[cam_index]
    red, blue = R.derive_cameras(cam, case["red_ref"], case["green_ref"], case["blue_ref"], double_ratio)
    g = R.Model(cam)
    ri, bi = {}, {}
    return g, ri, bi, R.warp_map(g, R.Model(red), ri), R.warp_map(g, R.Model(blue), bi)


def test_case_names():
    assert sorted(CASES) == sorted(["odd_37x23", "principal_on_centre", "principal_outside", "zero_green_distortion",
                                    "zero_red_distortion", "clamped_rim", "leaves_image", "float_ratio", "mixed_rig"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_is_finite_and_sees_truncation(name):
    case = CASES[name]
    rounded_differs = False
    for cam, im, (red, blue, aligned) in zip(AC.selected(case), AC.images(case), AC.expected(case)):
        w, h = cam["resolution"]
        assert red.shape == blue.shape == (h, w, 2) and red.dtype == blue.dtype == np.float32
        assert np.isfinite(red).all() and np.isfinite(blue).all()
        assert aligned.shape == (h, w, 3) and aligned.dtype == np.uint16
        assert np.array_equal(aligned[..., 1], im[..., 1])
        assert (im == 0).any() and (im == 65535).any()
        rounded_differs |= not np.array_equal(R.align(im, red, blue, rounded=True), aligned)
    assert rounded_differs  # rounding the blend instead of truncating it would be seen


def test_odd_size():
    cam = CASES["odd_37x23"]["rig"][0]
    w, h = cam["resolution"]
    assert all((w * h) % k for k in (8, 64, 256)) and w % 2 and h % 2
    assert all((2 * p) % 1 for p in cam["principal"])  # no whole and no half pixel
    g, ri, _, _, _ = _infos(CASES["odd_37x23"])
    assert not ri["on_principal"].any()


def test_principal_on_centre_hits_the_defined_point_once():
    g, ri, bi, red, blue = _infos(CASES["principal_on_centre"])
    assert ri["on_principal"].sum() == 1 and bi["on_principal"].sum() == 1
    y, x = np.argwhere(ri["on_principal"])[0]
    assert (x + 0.5, y + 0.5) == tuple(g.principal)
    assert tuple(red[y, x]) == tuple(blue[y, x]) == (x + 0.5, y + 0.5)
    im = AC.images(CASES["principal_on_centre"])[0]
    assert np.array_equal(AC.expected(CASES["principal_on_centre"])[0][2][y, x], im[y, x])  # its own texel


def test_principal_outside():
    g = R.Model(CASES["principal_outside"]["rig"][0])
    assert not (0 <= g.principal[0] < g.w) and not (0 <= g.principal[1] < g.h)


def test_zero_distortion_short_circuits():
    g, ri, bi, red, blue = _infos(CASES["zero_green_distortion"])
    assert g.dist_zero and not ri["undistort_at_max"].any()
    red_cam, blue_cam = R.derive_cameras(AC.selected(CASES["zero_green_distortion"])[0], *[CASES["zero_green_distortion"][k] for k in ("red_ref", "green_ref", "blue_ref")])
    assert not R.Model(red_cam).dist_zero and not R.Model(blue_cam).dist_zero
    case = CASES["zero_red_distortion"]
    red_cam, blue_cam = R.derive_cameras(AC.selected(case)[0], case["red_ref"], case["green_ref"], case["blue_ref"])
    assert not R.Model(AC.selected(case)[0]).dist_zero
    assert R.Model(red_cam).dist_zero and "distortion" not in red_cam
    assert R.Model(blue_cam).dist_zero and blue_cam["distortion"] == [0.0, 0.0, 0.0]  # all-zero coefficients: the same


def test_clamped_rim_takes_both_clamps_and_not_everywhere():
    g, ri, bi, _, _ = _infos(CASES["clamped_rim"])
    assert math.isfinite(g.dist_max)
    for info in (ri, bi):
        assert info["undistort_at_max"].any() and not info["undistort_at_max"].all()
        assert info["distort_clamped"].any() and not info["distort_clamped"].all()


def test_leaves_image_on_every_side_with_ties():
    case = CASES["leaves_image"]
    cam = AC.selected(case)[0]
    red, blue, _ = AC.expected(case)[0]
    w, h = cam["resolution"]
    xs, ys = np.arange(w) + 0.5, np.arange(h) + 0.5
    px, py = np.meshgrid(xs, ys)
    assert np.array_equal(red[..., 0], (2 * (px - 16.5) + 16.5).astype(np.float32))  # the exact ratio: exact targets
    assert np.array_equal(blue[..., 1], (0.5 * (py - 12.5) + 12.5).astype(np.float32))
    info = {}
    R.sample(AC.images(case)[0][..., 2], red, info)
    for side in ("left", "right", "above", "below"):
        assert info[side].any(), side
    assert info["inside"].any() and info["tie"].all()
    info = {}
    R.sample(AC.images(case)[0][..., 0], blue, info)
    assert info["tie"].any() and not info["tie"].all()


def test_float_ratio_is_part_of_the_result():
    case = CASES["float_ratio"]
    cam = AC.selected(case)[0]
    ratio = cam["focal"][0] / case["green_ref"]["focal"][0]
    assert float(np.float32(ratio)) != ratio
    red, blue, _ = AC.expected(case)[0]
    red64, blue64 = R.maps_of(cam, case["red_ref"], case["green_ref"], case["blue_ref"], double_ratio=True)
    changed = int((red != red64).sum() + (blue != blue64).sum())
    print("float_ratio: %d map values differ under a double focalRatio" % changed)
    assert changed >= 1


def test_mixed_rig():
    case = CASES["mixed_rig"]
    assert len(case["rig"]) == 3 and [c["id"] for c in AC.selected(case)] == ["cam2", "cam1"]
    assert len({tuple(c["resolution"]) for c in case["rig"]}) == 2 and len({c["type"] for c in case["rig"]}) == 2
    assert len({tuple(c["resolution"]) for c in AC.selected(case)}) == 2


@pytest.mark.parametrize("dist", [[-0.2], [-0.25], [-0.22], [-0.03, 0.002], [0.05, -0.01], [-0.03, 0.02, -0.004], [0.01, 0.001, 0.0001]])
def test_distortion_max_against_polynomial_roots(dist):
    d = dist + [0.0] * (3 - len(dist))
    k = [1.0] + [d[i] * (2 * i + 3) for i in range(3)]
    roots = np.roots(k[::-1])
    real = sorted(r.real for r in roots if abs(r.imag) < 1e-9 * max(1.0, abs(r.real)) and r.real > 0)
    got = R.distortion_max(d)
    if real:
        assert got == pytest.approx(math.sqrt(real[0]), rel=1e-9)
    else:
        assert got == math.inf


# ---- geometry -------------------------------------------------------------------------------------------------
def _pattern(theta, k=9.0, mid=32000.0, amp=20000.0):
    """a smooth grey pattern of the incidence angle, flat at the axis"""
    return mid + amp * np.cos(k * theta)


def _render(model, k=9.0):
    """the pattern seen through one channel's model on the model's grid, rounded to u16"""
    px, py = np.meshgrid(np.arange(model.w) + 0.5, np.arange(model.h) + 0.5)
    r = np.hypot(px - model.principal[0], py - model.principal[1])
    return np.rint(_pattern(R.undistort(model, r / model.focal), k)).astype(np.uint16)


def _second_derivative_bound(model, k=9.0, amp=20000.0):
    """max over the image of |d^2/dx^2| of F(r) = pattern(undistort(r / focal)) along any direction: for a radial
    function the second derivative along a direction lies between F''(r) and F'(r) / r. With D = distort,
    theta' = 1 / (focal D'(theta)) and theta'' = -D''(theta) / (focal^2 D'(theta)^3), analytically."""
    corners = [np.hypot(x - model.principal[0], y - model.principal[1]) for x in (0, model.w) for y in (0, model.h)]
    r = np.linspace(1e-3, max(corners) + 1.0, 20001)
    theta = R.undistort(model, r / model.focal)
    d0, d1, d2 = model.dist
    t2 = theta * theta
    D1 = 1 + 3 * d0 * t2 + 5 * d1 * t2 ** 2 + 7 * d2 * t2 ** 3
    D2 = 6 * d0 * theta + 20 * d1 * theta ** 3 + 42 * d2 * theta ** 5
    th1 = 1 / (model.focal * D1)
    th2 = -D2 / (model.focal ** 2 * D1 ** 3)
    I1, I2 = -amp * k * np.sin(k * theta), -amp * k * k * np.cos(k * theta)
    return float(max(np.abs(I2 * th1 ** 2 + I1 * th2).max(), np.abs(I1 * th1 / r).max()))


def test_geometry_red_and_blue_land_on_green():
    """A pattern that is a function of the incidence angle alone, rendered through the derived red, green and blue models
    into the three channels of one image, is the picture a lens with lateral chromatic aberration takes of it. After the
    alignment R and B must equal G up to the bilinear interpolation error of the rendered plane, at most (M_xx + M_yy) / 8
    <= M / 4 for a bound M on its second derivatives (computed analytically from the pattern and the model), plus 1 count
    for the truncating blend. (The pattern's own rounding to u16 gets no allowance.) Before the alignment the same
    difference is far above that bound: a warp in the wrong direction, or red and blue exchanged, doubles the
    misalignment instead of removing it."""
    green_cam = AC.camera("cam0", 96, 64, 60.0, (47.3, 31.6), [-0.03, 0.002])
    red_ref, green_ref, blue_ref = AC._refs((1012.0, [-0.02, 0.001]), (1000.0, [-0.03, 0.002]), (990.0, [-0.04, 0.003]))
    red_cam, blue_cam = R.derive_cameras(green_cam, red_ref, green_ref, blue_ref)
    g, r, b = R.Model(green_cam), R.Model(red_cam), R.Model(blue_cam)
    image = np.stack([_render(b), _render(g), _render(r)], axis=-1)
    red_map, blue_map = R.warp_map(g, r), R.warp_map(g, b)
    aligned = R.align(image, red_map, blue_map)
    for name, channel, model, at in (("R", 2, r, red_map), ("B", 0, b, blue_map)):
        info = {}
        R.sample(image[..., channel], at, info)
        inside = info["inside"]
        assert inside.sum() > 0.8 * inside.size
        bound = _second_derivative_bound(model) / 4 + 1
        diff = lambda im: int(np.abs(im[..., channel].astype(np.int64) - im[..., 1].astype(np.int64))[inside].max())  # noqa: E731
        before, after = diff(image), diff(aligned)
        print("geometry: max |%s - G| before %d, after %d, bound %.1f" % (name, before, after, bound))
        assert after <= bound
        assert before > bound
        # the other channel's map, or the warp turned round (green sampled where the channel lands), does not do it
        other = blue_map if channel == 2 else red_map
        assert diff(R.align(image, other, other)) > bound
