"""The host-only entries of the derp_sweep_* group against the restatement (tests/sweep_ref.py), and the input conditions
the GPU cases of tests/test_gpu_sweep.py rely on, checked on the restatement. No GPU."""
import math

import numpy as np
import pytest

from facebook360_dep_amd import derp, synth
from tests import common
from tests import sweep_cases as K
from tests import sweep_ref as R


# ---------------------------------------------------------------- depth lists, stems, crop size
@pytest.mark.parametrize("num", [1, 2, 50])
@pytest.mark.parametrize("lo,hi", [(1, 10), (2, 1000), (10, 10)])
def test_overlap_disparities(num, lo, hi):
    got_d, got_s = derp.sweep_overlap_disparities(num, lo, hi)
    ref_d, ref_s = R.overlap_disparities(num, lo, hi)
    assert K.same(got_d, ref_d) and K.same(got_s, ref_s)
    assert got_d[0] == np.float32(1) / np.float32(hi)  # probe 0 is the farthest depth
    if num > 1:
        assert got_d[-1] == np.float32(1) / np.float32(lo)


@pytest.mark.parametrize("num", [1, 2, 50])
@pytest.mark.parametrize("lo,hi", [(1.0, 10.0), (0.3, 1000.0), (1.0, 1.001)])
def test_equirect_depths(num, lo, hi):
    got_d, got_s = derp.sweep_equirect_depths(num, lo, hi)
    ref_d, ref_s = R.equirect_depths(num, lo, hi)
    assert K.same(got_d, ref_d) and K.same(got_s, ref_s)
    assert np.isfinite(got_d).all()


def test_depths_that_share_a_stem():
    _, stems = derp.sweep_equirect_depths(50, 1.0, 1.001)
    assert len(set(stems.tolist())) < 50
    _, stems = derp.sweep_overlap_disparities(50, 10, 10)
    assert len(set(stems.tolist())) < 50


def test_depth_lists_refuse_bad_arguments():
    for call in (lambda: derp.sweep_overlap_disparities(0), lambda: derp.sweep_overlap_disparities(3, 0, 10),
                 lambda: derp.sweep_equirect_depths(0), lambda: derp.sweep_equirect_depths(3, 0.0, 10.0),
                 lambda: derp.sweep_equirect_depths(3, 1.0, -1.0)):
        with pytest.raises(derp.DerpError):
            call()


@pytest.mark.parametrize("height,bounds", [(512, (3, 60, 2, 29)), (19, (0, 37, 0, 18)), (32, (10, 11, 0, 31)),
                                           (100, (0, 7, 0, 3)), (512, (17, 1000, 5, 8))])
def test_crop_size(height, bounds):
    assert derp.sweep_crop_size(height, bounds) == R.crop_size(height, bounds)


@pytest.mark.parametrize("bounds", [(64, 0, 32, 0), (5, 5, 2, 9), (5, 9, 4, 4)])
def test_crop_size_refuses_an_empty_box(bounds):
    assert R.crop_size(32, bounds) is None
    with pytest.raises(derp.DerpError, match="crop_equirect"):
        derp.sweep_crop_size(32, bounds)


# ---------------------------------------------------------------- derp_rig_center
def _rolled(cams):
    """every camera rolled about its own forward axis by 0.3 rad, so that the roll of the centring is well above a
    degree whichever camera is selected (the synthetic rigs keep every camera's up in a vertical plane)"""
    out = []
    for cam in cams:
        up, right = np.array(cam["up"]), np.array(cam["right"])
        c, s = math.cos(0.3), math.sin(0.3)
        out.append(dict(cam, up=(c * up + s * right).tolist(), right=(c * right - s * up).tolist()))
    return out


# (the five-camera rig is also pitched as a whole: its middle camera looks along the horizon, a pitch of exactly zero)
RIGS = {"rig5": lambda: R.rotate_rig(_rolled(synth.make_rig(5, 64)["cameras"]), 0, 0.35),
        "mixed": lambda: _rolled(common.mixed_type_rig(64)["cameras"]),
        "real": lambda: common.real_rig()["cameras"]}


@pytest.mark.parametrize("rig", sorted(RIGS))
def test_rig_center(rig):
    cams = RIGS[rig]()
    for index in range(len(cams)):
        angles = []
        ref = R.rig_center(cams, index, angles)
        got = derp.rig_center(cams, index)
        for g, r in zip(got, ref):
            for key in ("origin", "forward", "up", "right"):
                assert np.abs(np.array(g[key]) - np.array(r[key])).max() <= 1e-12, (index, key)
        # the selected camera looks at the equirect's centre, its up in the x-z plane with z > 0 (acos of a cosine near
        # +-1 keeps half the digits, in the reference too: 1e-6)
        f, u = np.array(got[index]["forward"]), np.array(got[index]["up"])
        assert np.abs(f - np.array([-1.0, 0.0, 0.0])).max() <= 1e-6, (index, f)
        assert abs(u[1]) <= 1e-6 and u[2] > 0, (index, u)
        # the rotation is rigid: distances from the origin and the angles between cameras survive
        for g, c in zip(got, cams):
            assert abs(np.linalg.norm(g["origin"]) - np.linalg.norm(c["origin"])) <= 1e-12


@pytest.mark.parametrize("rig", sorted(RIGS))
def test_rig_center_rotations_are_not_degenerate(rig):
    """the input condition of the 1e-12 comparison above: yaw, pitch and roll all exceed one degree, for every camera"""
    cams = RIGS[rig]()
    for index in range(len(cams)):
        angles = []
        R.rig_center(cams, index, angles)
        assert len(angles) == 3 and min(abs(a) for a in angles) > math.radians(1.0), (index, angles)


def test_rig_center_refuses_bad_arguments():
    cams = synth.make_rig(4, 64)["cameras"]
    with pytest.raises(derp.DerpError):
        derp.rig_center(cams, 4)
    bad = [dict(c) for c in cams]
    bad[1]["right"] = [-v for v in bad[1]["right"]]  # left-handed
    with pytest.raises(derp.DerpError, match="right-handed"):
        derp.rig_center(bad, 0)


# ---------------------------------------------------------------- what the GPU cases must contain
@pytest.mark.parametrize("name", sorted(K.OVERLAP_CASES))
def test_overlap_cases_contain_what_they_claim(name):
    dsts = K.overlap_case(name)[4]
    counts = np.concatenate([K.overlap_ref(name, d)[1].reshape(-1) for d in dsts])
    clamped = set().union(*[K.overlap_ref(name, d)[2] for d in dsts])
    if name != "rig34_16":  # (the fibonacci rig's 16 x 16 images: checked for the rest only)
        assert (counts == 1).any(), "no pixel is seen by exactly one camera"
    assert (counts >= 2).any() or name == "isolated"
    if name in ("rig4_32", "rig4_25x19", "rig4_mixed", "rig2", "isolated", "rig34_16"):
        assert (counts == -1).any(), "no pixel lies outside the image circle"
    if name == "isolated":
        ref, count, _ = K.overlap_ref(name, 2)
        assert (count == 0).any() and np.isnan(ref[count == 0]).all()
        assert (R.to_u8(ref)[count == 0] == 0).all()
        assert (count == 1).any() and not (count >= 2).any()
    if name in ("rig4_32", "rig4_mixed"):
        assert clamped == {"left", "right", "top", "bottom"}, clamped


def test_overlap_hole_reaches_the_result():
    ref = K.overlap_ref("rig4_mixed", 0)[0]
    alpha = ref[..., 3][~np.isnan(ref[..., 3])]
    assert (alpha < 1).any() and (alpha == 1).any()


@pytest.mark.parametrize("name", sorted(K.EQUIRECT_CASES))
def test_equirect_cases_contain_what_they_claim(name):
    ref, count, mattered = K.equirect_ref(name)
    if name != "rig34_64x32":  # (34 cameras cover the whole sphere a dozen times over)
        assert (count == 0).any() and (count == 1).any()
    assert (count >= 2).any() or name == "isolated_64x32"
    if name == "rig4_mixed":
        assert mattered, "no truncated index lies past an image's edge"
    elif K.EQUIRECT_CASES[name][2] is None:
        assert not mattered
    black = K.equirect_case(name)[5]
    assert (ref[count == 0] == np.array([0, 0, 0 if black else 1, 1], np.float32)).all()


def test_seeded_defects_change_the_restatement():
    """the restatement tells the orders and roundings apart that the GPU tests are there to pin"""
    rig = K.overlap_rigged("rig4_32")
    d = K.overlap_case("rig4_32")[3][3]
    assert K.differing(rig.overlaps(1, d), rig.overlaps(1, d, order=range(3, -1, -1))) > 0
    e = K.equirect_rigged("rig4_64x32")
    depth = K.equirect_case("rig4_64x32")[4][2]
    assert K.differing(e.equirect(64, 32, depth), e.equirect(64, 32, depth, fetch="round")) > 0
    cams, images, res, _, _ = K.overlap_case("rig4_mixed")
    by_size = R.Rigged(cams, images, [(im.shape[1], im.shape[0]) for im in images])
    assert K.differing(K.overlap_rigged("rig4_mixed").overlaps(0, d), by_size.overlaps(0, d)) > 0


@pytest.mark.parametrize("name", K.BOUNDS_CASES)
def test_bounds_and_crop_of_the_cases(name):
    _, _, _, (W, H), _, _ = K.equirect_case(name)
    rig = K.equirect_rigged(name)
    for depth in K.BOUNDS_DEPTHS:
        b = rig.equirect_bounds(W, H, depth)
        assert b[0] < b[1] and b[2] < b[3], (depth, b)  # a box that --crop_equirect accepts
        assert R.crop_size(H, b) >= 1
