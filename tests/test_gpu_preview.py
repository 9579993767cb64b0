"""derp_preview_variance, derp_preview_foreground and derp_preview_keypoints on the device against the numpy restatement (tests/preview_ref.py,
which takes the variance, the resize and the mask from the oracle): 0 differing values and equal counts."""
import numpy as np
import pytest

from tests import preview_cases as cases
from tests import preview_ref as ref

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ctx(built):
    from facebook360_dep_amd import derp, synth

    g = derp.Derp(synth.make_rig(1, 16)["cameras"])
    yield g
    g.close()


@pytest.fixture(scope="module")
def variance_case(built):
    from oracle import oracle_lib

    img = cases.variance_image()
    var = oracle_lib.cv_variance(img)
    var.setflags(write=False)
    return img, var


def _settings(var):
    """seven settings: the tool's defaults, the slider ends, and thresholds equal to variances present in the image"""
    lo, hi = cases.equal_thresholds(var)
    lv = [ref.variance_levels(cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, a, b, 1.0) for a, b in
          ((2, 2), (0, 0), (100, 100), (0, 100), (50, 1))]
    low = [v[2] for v in lv] + [lo, hi]
    high = [v[3] for v in lv] + [hi, hi]
    return np.array(low, F32), np.array(high, F32)


def test_variance_marks_equal_the_restatement(ctx, variance_case):
    img, var = variance_case
    low, high = _settings(var)
    got, counts, gvar = ctx.preview_variance(img, low, high, with_variance=True)
    assert gvar.tobytes() == var.tobytes()  # the level loop's kernel: the oracle's bits
    want, wcounts = ref.variance_marks(img, low, high, var)
    assert np.count_nonzero(got != want) == 0
    assert counts.tolist() == wcounts.tolist()
    flat = got[:, cases.FLAT[0].start + 1:cases.FLAT[0].stop - 1, cases.FLAT[1].start + 1:cases.FLAT[1].stop - 1]
    assert (flat == ref.BLUE).all()  # variance 0 is blue at every setting
    on = (var == low[5]) | (var == high[5])
    assert on.any() and (got[5][on] == img[on]).all()  # equal to a threshold: marked by neither


def test_variance_one_setting_equals_the_shared_one_of_seven(ctx, variance_case):
    img, var = variance_case
    low, high = _settings(var)
    seven, counts7 = ctx.preview_variance(img, low, high)
    for k in (0, 5):
        one, counts1 = ctx.preview_variance(img, low[k:k + 1], high[k:k + 1])
        assert one.shape == (1,) + img.shape and (one[0] == seven[k]).all() and counts1[0].tolist() == counts7[k].tolist()


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (3, 3), (65, 33)])
def test_variance_sizes(ctx, w, h):
    from oracle import oracle_lib

    img = np.random.default_rng(w * 100 + h).integers(0, 65536, (h, w, 3)).astype(np.uint16)
    var = oracle_lib.cv_variance(img)
    low = np.array([ref.K_MIN_VAR, np.median(var)], F32)
    high = np.array([var.max(), np.median(var)], F32)
    got, counts, gvar = ctx.preview_variance(img, low, high, with_variance=True)
    assert gvar.tobytes() == var.tobytes()
    want, wcounts = ref.variance_marks(img, low, high, var)
    assert np.count_nonzero(got != want) == 0 and counts.tolist() == wcounts.tolist()


def test_variance_refusals(ctx):
    from facebook360_dep_amd import derp

    img = cases.variance_image(4, 4)
    with pytest.raises(derp.DerpError, match="257 settings, 1 .. 256"):
        ctx.preview_variance(img, np.zeros(257, F32), np.zeros(257, F32))
    with pytest.raises(derp.DerpError, match="0 settings, 1 .. 256"):
        ctx.preview_variance(img, np.zeros(0, F32), np.zeros(0, F32))
    out, counts = ctx.preview_variance(img, np.zeros(256, F32), np.full(256, np.inf, F32))  # the cap itself is served
    assert (out == img).all() and not counts.any()


@pytest.fixture(scope="module")
def foreground_case(built):
    template, frame = cases.foreground_pair()
    want = ref.foreground(template, frame, cases.FG_BLURS, cases.FG_SLIDERS, cases.FG_CLOSINGS)
    for a in want:
        a.setflags(write=False)
    return template, frame, want


def test_foreground_overlays_equal_the_restatement(ctx, foreground_case):
    template, frame, (woverlays, wmasks, wcounts) = foreground_case
    from facebook360_dep_amd import derp

    thresholds = [derp.preview_foreground_threshold(s) for s in cases.FG_SLIDERS]
    assert [t.tobytes() for t in thresholds] == [ref.foreground_threshold(s).tobytes() for s in cases.FG_SLIDERS]
    overlays, masks, counts = ctx.preview_foreground(template, frame, cases.FG_BLURS, thresholds, cases.FG_CLOSINGS)
    assert overlays.shape == (36, cases.FG_H, cases.FG_W, 3)
    assert np.count_nonzero(masks != wmasks) == 0
    assert np.count_nonzero(overlays != woverlays) == 0
    assert counts.tolist() == wcounts.tolist()
    k = 0
    for b in cases.FG_BLURS:
        for s, t in zip(cases.FG_SLIDERS, thresholds):
            for c in cases.FG_CLOSINGS:
                assert (masks[k] == ctx.generate_foreground_mask(template, frame, b, float(t), c)).all(), (b, s, c)
                if s == 100:  # an empty mask: the frame as it came
                    assert not masks[k].any() and (overlays[k] == frame).all() and counts[k] == 0
                k += 1
    # blur 0, slider 4, closing 0: the probes' greens at the tie (both parities), at zero and saturated
    o = overlays[(0 * 3 + 1) * 4 + 0]
    assert [int(o[y, x, 1]) for (y, x) in cases.G_PROBES] == [32768, 32768, 65534, 65535, 65535]
    assert (o[..., 0] == frame[..., 0]).all() and (o[..., 2] == frame[..., 2]).all()


def test_foreground_smallest_image(ctx):
    template = np.array([[[100, 200, 300]]], np.uint16)
    frame = np.array([[[40000, 1, 300]]], np.uint16)
    overlays, masks, counts = ctx.preview_foreground(template, frame, (0, 1), (ref.foreground_threshold(4),), (0, 4))
    woverlays, wmasks, wcounts = ref.foreground(template, frame, (0, 1), (4,), (0, 4))
    assert (overlays == woverlays).all() and (masks == wmasks).all() and counts.tolist() == wcounts.tolist() == [1] * 4
    assert overlays[0, 0, 0].tolist() == [40000, 32768, 300]


def test_foreground_refusals(ctx):
    from facebook360_dep_amd import derp

    template, frame = cases.foreground_pair()
    with pytest.raises(derp.DerpError, match=r"bad arguments \(blur_radius must be 0..3\)"):
        ctx.preview_foreground(template, frame, (1, 4), (0.04,), (4,))
    with pytest.raises(derp.DerpError, match=r"bad arguments \(blur_radius must be 0..3\)"):
        ctx.preview_foreground(template, frame, (1,), (0.04,), (-1,))
    with pytest.raises(derp.DerpError, match="1 .. 256 triples"):
        ctx.preview_foreground(template, frame, (0, 1, 2, 3), np.linspace(0, 1, 17), (0, 1, 2, 3))
    with pytest.raises(derp.DerpError, match="1 .. 256 triples"):
        ctx.preview_foreground(template, frame, (), (0.04,), (4,))


def test_budget_refusals(ctx, monkeypatch):
    """the fixed bound of one call's device buffers, lowered so that small images reach it: 26 B per pixel + 6 per output
    pixel for the variance, 40 + 7 per output pixel for the foreground"""
    from facebook360_dep_amd import derp

    img = cases.variance_image()
    template, frame = cases.foreground_pair()
    px = cases.VAR_W * cases.VAR_H
    monkeypatch.setenv("DERP_PREVIEW_BUDGET_MB", repr((px * 26 + 2 * px * 6) / 2.0 ** 20))  # exactly two settings fit
    two = ctx.preview_variance(img, np.zeros(2, F32), np.full(2, np.inf, F32))[0]
    assert (two == img).all()
    with pytest.raises(derp.DerpError, match="derp_preview_variance: the device buffers of this call .* exceed the preview budget"):
        ctx.preview_variance(img, np.zeros(3, F32), np.full(3, np.inf, F32))
    with pytest.raises(derp.DerpError, match="derp_preview_foreground: the device buffers of this call .* exceed the preview budget"):
        ctx.preview_foreground(template, frame, (0, 1), (0.04,), (0, 4))
    for bad in ("", "-1", "nan", "inf", "12x", "0"):
        monkeypatch.setenv("DERP_PREVIEW_BUDGET_MB", bad)
        with pytest.raises(derp.DerpError, match="DERP_PREVIEW_BUDGET_MB='%s' is not a positive finite number" % bad):
            ctx.preview_variance(img, np.zeros(1, F32), np.full(1, np.inf, F32))
    monkeypatch.delenv("DERP_PREVIEW_BUDGET_MB")
    assert ctx.preview_variance(img, np.zeros(3, F32), np.full(3, np.inf, F32))[0].shape[0] == 3


# ---------------------------------------------------------------- GenerateKeypointProjections
@pytest.fixture(scope="module")
def keypoint_wants(built):
    """the restatement of every case and pair, computed once"""
    from oracle import oracle_lib

    images = cases.keypoint_images()
    wants = {}
    for name, (rig_args, params) in cases.KP_CASES.items():
        rig = oracle_lib.Rig(cases.keypoint_rig(**rig_args))
        for c0 in range(3):
            for c1 in range(c0 + 1, 3):
                rects, stats = ref.keypoint_rects(rig, c0, c1, cases.KP_W, cases.KP_H, cases.KP_W, cases.KP_H, **params)
                blend, u8, _ = ref.keypoint_blend(images[c0], rects)
                wants[name, c0, c1] = (blend, u8, len(rects), stats)
    return images, wants


@pytest.mark.parametrize("name", sorted(cases.KP_CASES))
def test_keypoints_equal_the_restatement(keypoint_wants, name):
    from facebook360_dep_amd import derp

    images, wants = keypoint_wants
    rig_args, params = cases.KP_CASES[name]
    cams = cases.keypoint_rig(**rig_args)
    g = derp.Derp(cams)
    try:
        g.sweep_upload(images, cases.keypoint_resolutions(cams))
        for c0 in range(3):
            for c1 in range(c0 + 1, 3):
                blend, u8, n_rects, stats = wants[name, c0, c1]
                got_u8, got_f, got_n = g.preview_keypoints(c0, c1, with_float=True, **params)
                assert got_n == n_rects, (c0, c1)
                assert np.count_nonzero(got_f.view(np.uint32) != blend.view(np.uint32)) == 0, (c0, c1)
                assert np.count_nonzero(got_u8 != u8) == 0, (c0, c1)
                only_u8, only_n = g.preview_keypoints(c0, c1, **params)
                assert (only_u8 == got_u8).all() and only_n == got_n
                # the host sampler answers what the kernel drew from: the same samples, point by point
                for (px, py), samples in stats["samples"]:
                    idx, disp, boxes = derp.preview_keypoint_samples(cams[c1], cams[c0], px, py, **params)
                    assert idx.tolist() == [s[0] for s in samples] and disp.tolist() == [s[1] for s in samples]
                    assert boxes.tobytes() == np.array([s[2] for s in samples], F32).reshape(-1, 4).tobytes()
    finally:
        g.close()


def test_keypoints_refusals(keypoint_wants):
    from facebook360_dep_amd import derp

    images, _ = keypoint_wants
    cams = cases.keypoint_rig()
    g = derp.Derp(cams)
    try:
        with pytest.raises(derp.DerpError, match="sweep_upload"):
            g.preview_keypoints(0, 1, **cases.KP_BASE)
        g.sweep_upload([im[:, :60] for im in images], [(cases.KP_W, cases.KP_H)] * 3)
        with pytest.raises(derp.DerpError, match="the image of camera 0 is 60 x 48, not the first camera's resolution 64 x 48"):
            g.preview_keypoints(0, 1, **cases.KP_BASE)
        g.sweep_upload(images, [(cases.KP_W, cases.KP_H)] * 3)
        for bad, message in ((dict(length_stride=0.0), "strides"), (dict(search_radius=-1), "search_radius"),
                             (dict(depth_samples=1.0), "depth_samples"), (dict(depth_min=0.0), "depth_min"),
                             (dict(length_stride=1e-4, height_stride=1e-4), "more than 1048576 grid points"),
                             (dict(length_stride=0.02, height_stride=0.02, search_radius=0, depth_samples=2000.0),
                              "more than 1048576 rectangles")):
            with pytest.raises(derp.DerpError, match="derp_preview_keypoints.*" + message):
                g.preview_keypoints(0, 1, **dict(cases.KP_BASE, **bad))
        with pytest.raises(derp.DerpError):
            g.preview_keypoints(0, 3, **cases.KP_BASE)
    finally:
        g.close()
