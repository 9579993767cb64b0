"""The tuning previews without a GPU: the host-only threshold arithmetic, depth sampler and rectangles of the C-ABI against the numpy restatement,
the restatement's own overlay rounding, and that every case of tests/preview_cases.py contains what it is named for."""
import numpy as np
import pytest

from tests import preview_cases as cases
from tests import preview_ref as ref

F32 = np.float32


@pytest.mark.parametrize("scale", [1.0, 37.0 / 75.0, 0.5])
def test_variance_levels_equal_the_restatement(built, scale):
    from facebook360_dep_amd import derp

    for lo in (0, 1, 2, 50, 100):
        for hi in (0, 1, 2, 50, 100):
            got = derp.preview_variance_levels(cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, lo, hi, scale)
            want = ref.variance_levels(cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, lo, hi, scale)
            assert got.dtype == F32 and got.tobytes() == want.tobytes(), (lo, hi, got, want)
            if hi == 0:
                assert got[3] == got[2]  # varHighShow falls back on varLowShow
            if lo == 0:
                assert got[2] == ref.K_MIN_VAR and got[0] == 0
            assert got[3] >= got[2] >= ref.K_MIN_VAR


def test_variance_levels_at_the_defaults(built):
    from facebook360_dep_amd import derp

    got = derp.preview_variance_levels(4e-3, 5e-2, 2, 2, 1.0)
    assert ref.c_exp3(got[0]) == "8.000e-05" and ref.c_exp3(got[1]) == "1.000e-03"
    # half the width is a quarter of the variance: scaleVar = 0.25, still above kMinVar
    assert derp.preview_variance_levels(4e-3, 5e-2, 2, 2, 0.5)[2] == F32(got[0] * F32(0.25)) > ref.K_MIN_VAR


@pytest.mark.parametrize("args", [(0.0, 5e-2, 2, 2, 1.0), (4e-3, -1.0, 2, 2, 1.0), (4e-3, 5e-2, -1, 2, 1.0), (4e-3, 5e-2, 2, 101, 1.0),
                                  (4e-3, 5e-2, 2, 2, 0.0), (4e-3, 5e-2, 2, 2, float("nan"))])
def test_variance_levels_refuse_by_name(built, args):
    from facebook360_dep_amd import derp

    with pytest.raises(derp.DerpError, match="derp_preview_variance_levels"):
        derp.preview_variance_levels(*args)


def test_overlay_rounding_of_the_restatement():
    frame = np.zeros((1, 5, 3), np.uint16)
    frame[0, :, 1] = [0, 1, 32767, 32768, 65535]
    frame[0, :, 0], frame[0, :, 2] = 7, 9
    out = ref.overlay(frame, np.ones((1, 5), np.uint8))
    # 32767.5 -> 32768 and 32768.5 -> 32768 (half to even, both parities); 65534.5 -> 65534; 65535.5 and beyond saturate
    assert out[0, :, 1].tolist() == [32768, 32768, 65534, 65535, 65535]
    assert (out[..., 0] == 7).all() and (out[..., 2] == 9).all()
    assert (ref.overlay(frame, np.zeros((1, 5), np.uint8)) == frame).all()


def test_variance_case_contents(built):
    from oracle import oracle_lib

    img = cases.variance_image()
    assert img.shape == (cases.VAR_H, cases.VAR_W, 3)
    var = oracle_lib.cv_variance(img)
    inner = var[cases.FLAT[0].start + 1:cases.FLAT[0].stop - 1, cases.FLAT[1].start + 1:cases.FLAT[1].stop - 1]
    assert (inner == 0).all()  # blue at every setting: 0 < kMinVar
    assert var.max() == var[cases.CHECKER].max() and var.max() > 0.2  # the checker holds the largest variance
    lo, hi = cases.equal_thresholds(var)
    assert ref.K_MIN_VAR < lo < hi
    for t in (lo, hi):  # pixels exactly on each threshold, and pixels strictly on both sides of it
        assert np.count_nonzero(var.view(np.uint32) == t.view(np.uint32)) >= 1
        assert (var < t).any() and (var > t).any()
    images, counts = ref.variance_marks(img, [lo], [hi], var)
    on = (var == lo) | (var == hi)
    assert (images[0][on] == img[on]).all() and counts[0][0] > 0 and counts[0][1] > 0


def test_variance_fullsize_case_contents(built):
    from oracle import oracle_lib

    for w in (74, 75):
        full = cases.variance_fullsize(w, 46)
        assert full.shape == (46, w, 3)
        small = ref.scaled(full, 37)
        assert small.shape == (23, 37, 3)
        var = oracle_lib.cv_variance(small)
        lv = ref.variance_levels(cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, 2, 2, ref.scale_of(37, w))
        _, counts = ref.variance_marks(small, [lv[2]], [lv[3]], var)
        assert 0 < counts[0][0] < 37 * 23 and 0 < counts[0][1] < 37 * 23  # both marks, and pixels with neither
    assert F32(ref.scale_of(37, 74) ** 2) == F32(0.25)


def test_foreground_case_contents(built):
    from oracle import oracle_lib

    template, frame = cases.foreground_pair()
    assert frame.shape == (cases.FG_H, cases.FG_W, 3)
    thr = float(ref.foreground_threshold(4))
    m0 = oracle_lib.generate_foreground_mask(template, frame, 0, thr, 0)
    m4 = oracle_lib.generate_foreground_mask(template, frame, 0, thr, 4)
    m7 = oracle_lib.generate_foreground_mask(template, frame, 0, thr, 7)
    assert not m0[cases.SMALL_HOLE] and m4[cases.SMALL_HOLE]  # the hole the closing fills
    assert not m0[cases.BIG_HOLE_CENTRE] and not m4[cases.BIG_HOLE_CENTRE] and not m7[cases.BIG_HOLE_CENTRE]  # and the one it does not
    assert m0[28, 2]  # the speck just over the default threshold
    for (y, x), g in cases.G_PROBES.items():  # the overlay's probes are foreground with exactly these greens
        assert m0[y, x] and frame[y, x, 1] == g
    assert not oracle_lib.generate_foreground_mask(template, frame, 0, float(ref.foreground_threshold(100)), 0).any()
    assert oracle_lib.generate_foreground_mask(template, frame, 0, 0.0, 0).any()
    assert not m0[0, 0]


# ---------------------------------------------------------------- GenerateKeypointProjections
def _desc_samples(cams, c_point, c_into, px, py, **params):
    from facebook360_dep_amd import derp

    return derp.preview_keypoint_samples(cams[c_point], cams[c_into], px, py, **params)


def test_stride_accumulation():
    assert len(ref.stride_values(0.1)) == 11 and len(ref.stride_values(0.3)) == 4
    assert len(ref.stride_values(0.125)) == 9 and ref.stride_values(0.125)[-1] == 1.0
    v = ref.stride_values(0.1)
    assert v[3] == 0.1 + 0.1 + 0.1 != 0.3 and v[-1] < 1.0  # accumulated, not i * stride: the last value is 0.99999...


def test_sampler_by_hand(built):
    from oracle import oracle_lib

    cams = cases.keypoint_rig()
    rig = oracle_lib.Rig(cams)
    near = dict(cases.KP_BASE, depth_min=0.3, depth_samples=400.0, search_radius=1)
    for px, py in ((32.0, 24.0), (16.0, 12.0), (48.0, 36.0)):
        idx, disp, boxes = _desc_samples(cams, 1, 0, px, py, **near)
        want = ref.keypoint_samples(rig, 1, 0, px, py, **near)
        assert idx.tolist() == [s[0] for s in want] and disp.tolist() == [s[1] for s in want]
        assert boxes.tobytes() == np.array([s[2] for s in want], F32).tobytes()
        assert idx[0] == 0 and len(idx) >= 3  # sample 0 is always taken, against the initial empty box
        depth = 1 / disp
        gaps = depth[:-1] - depth[1:]
        # the samples are uniform in disparity, so the accepted ones lie ever closer in depth towards depth_min
        assert gaps[0] > gaps[-1] > 0 and (np.diff(gaps) < 0).all()
        # search_radius = 0: boxes of no area, none overlaps, every sample is taken
        idx0, _, boxes0 = _desc_samples(cams, 1, 0, px, py, **dict(near, search_radius=0))
        assert idx0.tolist() == list(range(400)) and (boxes0[:, 2:] == 0).all()
        # two identical cameras: the box never moves, only sample 0 is taken
        same, _, _ = _desc_samples(cams, 1, 1, px, py, **near)
        assert same.tolist() == [0]
    # a whole number of samples is not required: next < depth_samples on a double
    idx, _, _ = _desc_samples(cams, 1, 0, 32.0, 24.0, **dict(near, search_radius=0, depth_samples=10.5))
    assert idx.tolist() == list(range(11))


@pytest.mark.parametrize("params,message", [
    (dict(length_stride=0.0), "strides"), (dict(height_stride=float("inf")), "strides"), (dict(search_radius=-1), "search_radius"),
    (dict(search_radius=1.5), "search_radius"), (dict(depth_samples=1.0), "depth_samples"), (dict(depth_min=0.0), "depth_min"),
    (dict(depth_max=0.5), "depth_min <= depth_max"), (dict(search_overlap=-0.1), "search_overlap")])
def test_sampler_refuses_by_name(built, params, message):
    from facebook360_dep_amd import derp

    cams = cases.keypoint_rig()
    with pytest.raises(derp.DerpError, match="derp_preview_keypoint_samples.*" + message):
        derp.preview_keypoint_samples(cams[0], cams[1], 1.0, 1.0, **params)


def test_rectangle_rounding_and_clipping(built):
    from facebook360_dep_amd import derp

    rect = derp.preview_keypoint_rect
    # p - 0.5 on a half: cvRound goes to the even neighbour, down at 2.5 and up at 3.5
    assert rect(3.0, 4.0, 0, 64, 48) == (2, 4, 2, 4)      # 2.5 -> 2, 3.5 -> 4
    assert rect(4.0, 3.0, 0, 64, 48) == (4, 2, 4, 2)
    assert rect(3.0, 4.0, 3, 64, 48) == (0, 0, 6, 6)      # -0.5 -> 0 (clipped anyway), 5.5 -> 6; 0.5 -> 0, 6.5 -> 6
    assert rect(10.25, 20.75, 2, 64, 48) == (8, 18, 12, 22)
    # clipping at the left, right, top and bottom edge, each against the restated corners
    for px, py, radius, want in ((1.0, 24.0, 3, (0, 20, 4, 26)), (63.0, 24.0, 3, (60, 20, 63, 26)),
                                 (32.0, 1.0, 4, (28, 0, 36, 4)), (32.0, 47.0, 4, (28, 42, 36, 47))):
        got = rect(px, py, radius, 64, 48)
        restated = (max(int(ref.cv_round(px - 0.5 - radius)), 0), max(int(ref.cv_round(py - 0.5 - radius)), 0),
                    min(int(ref.cv_round(px - 0.5 + radius)), 63), min(int(ref.cv_round(py - 0.5 + radius)), 47))
        assert got == want == restated, ((px, py), got, restated)
    assert rect(-20.0, 10.0, 3, 64, 48)[2] < 0 and rect(10.0, 80.0, 3, 64, 48)[1] > 47  # wholly outside: empty
    with pytest.raises(derp.DerpError, match="derp_preview_keypoint_rect"):
        rect(1.0, 1.0, -1, 64, 48)


def test_keypoint_case_contents(built):
    from oracle import oracle_lib

    seen_stats = {}
    for name, (rig_args, params) in cases.KP_CASES.items():
        rig = oracle_lib.Rig(cases.keypoint_rig(**rig_args))
        total = dict(skipped_circle=0, unseen=0, shared=0, rects=0, most=0, outside=0)
        for c0 in range(3):
            for c1 in range(c0 + 1, 3):
                rects, st = ref.keypoint_rects(rig, c0, c1, cases.KP_W, cases.KP_H, cases.KP_W, cases.KP_H, **params)
                _, u8, shared = ref.keypoint_blend(cases.keypoint_images()[c0], rects)
                total["skipped_circle"] += st["skipped_circle"]
                total["unseen"] += st["unseen"]
                total["outside"] += st["outside"]
                total["shared"] += shared
                total["rects"] += len(rects)
                total["most"] = max([total["most"]] + [len(s) for _, s in st["samples"]])
                assert (u8 == 255).any() and (u8[..., :3] < 255).any()
        seen_stats[name] = total
    assert seen_stats["base"]["rects"] > 0 and seen_stats["base"]["most"] > 1
    assert seen_stats["radius0"]["most"] == 1000                      # 1-pixel rectangles, every sample taken
    # `sees` fails for some samples and succeeds for others, in the base rig and, differently, with a camera turned
    assert seen_stats["unseen"]["unseen"] > 0 and seen_stats["base"]["unseen"] > 0
    assert 0 < seen_stats["unseen"]["rects"] != seen_stats["base"]["rects"]
    assert seen_stats["circle"]["skipped_circle"] > seen_stats["base"]["skipped_circle"] > 0
    # rectangles wholly outside the image, beside rectangles inside it; none in a rig of equal resolutions
    assert 0 < seen_stats["outside"]["outside"] < seen_stats["outside"]["rects"] and seen_stats["base"]["outside"] == 0
    assert seen_stats["overwrite"]["shared"] > 0 and seen_stats["base"]["shared"] == 0  # rectangles of two grid points meet
