"""bin/ViewColorVarianceThresholds, bin/ViewForegroundMaskThresholds and bin/GenerateKeypointProjections end to end: the files DESIGN §8.12 names decode to
the restatement's arrays (which the entry points equal, tests/test_gpu_preview.py), and thresholds.json equals the
restatement's, strings included."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import preview_cases as cases
from tests import preview_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


def _run(tool, *args):
    p = subprocess.run([os.path.join(BIN, tool)] + list(args), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stderr


def _bgr16(path):
    from facebook360_dep_amd import imageio as dio

    a = dio.read_png(path)
    assert a.dtype == np.uint16 and a.ndim == 3 and a.shape[2] == 3
    return a


# 74 columns: the integer 2 x 2 path of the resize, scaleVar 0.25; 75 columns: its table path
@pytest.mark.parametrize("cols", [74, 75])
def test_variance_files(built, tmp_path, cols):
    from facebook360_dep_amd import imageio as dio

    full = cases.variance_fullsize(cols, 46)
    src, out = str(tmp_path / "full.png"), str(tmp_path / "out")
    dio.write_png16(src, full)
    lows, highs = [0, 2, 100], [2, 40]
    log = _run("ViewColorVarianceThresholds", "--fullsize_image=" + src, "--width=37", "--output=" + out,
               "--low_sliders=0,2,100", "--high_sliders=2,40")
    small = ref.scaled(full, 37)
    scale = ref.scale_of(37, cols)
    lv = [ref.variance_levels(cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, lo, hi, scale) for lo in lows for hi in highs]
    want, counts = ref.variance_marks(small, [v[2] for v in lv], [v[3] for v in lv])
    names = ["low_%03d_high_%03d.png" % (lo, hi) for lo in lows for hi in highs]
    assert sorted(os.listdir(out)) == sorted(names + ["thresholds.json"])
    for k, name in enumerate(names):
        assert np.count_nonzero(_bgr16(os.path.join(out, name)) != want[k]) == 0, name
    with open(os.path.join(out, "thresholds.json")) as f:
        assert json.load(f) == ref.variance_json(lows, highs, cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, scale, counts, 37, 23)
    assert "--var_noise_floor=8.000e-05 --var_high_thresh=1.000e-03" in log  # the defaults' pair, as the reference logs it


def test_variance_defaults_and_original_size(built, tmp_path):
    from facebook360_dep_amd import imageio as dio

    img = cases.variance_image()
    src, out = str(tmp_path / "img.png"), str(tmp_path / "out")
    dio.write_png16(src, img)
    _run("ViewColorVarianceThresholds", "--fullsize_image=" + src, "--width=0", "--output=" + out)
    lv = ref.variance_levels(cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, 2, 2, 1.0)
    want, counts = ref.variance_marks(img, [lv[2]], [lv[3]])
    assert sorted(os.listdir(out)) == ["low_002_high_002.png", "thresholds.json"]
    assert np.count_nonzero(_bgr16(os.path.join(out, "low_002_high_002.png")) != want[0]) == 0
    with open(os.path.join(out, "thresholds.json")) as f:
        assert json.load(f) == ref.variance_json([2], [2], cases.VAR_LOW_MAX, cases.VAR_HIGH_MAX, 1.0, counts, cases.VAR_W, cases.VAR_H)


def test_foreground_files(built, tmp_path):
    from facebook360_dep_amd import imageio as dio

    template, frame = cases.foreground_pair()
    bg, fg, out = str(tmp_path / "bg.png"), str(tmp_path / "fg.png"), str(tmp_path / "out")
    dio.write_png16(bg, template)
    dio.write_png16(fg, frame)
    blurs, sliders, closings = [0, 1], [4, 100], [0, 4]
    _run("ViewForegroundMaskThresholds", "--fullsize_bg_image=" + bg, "--fullsize_fg_image=" + fg, "--width=0",
         "--output=" + out, "--blur_radii=0,1", "--threshold_sliders=4,100", "--closing_sizes=0,4")
    want, _, counts = ref.foreground(template, frame, blurs, sliders, closings)
    names = ["blur_%02d_thresh_%03d_close_%02d.png" % (b, s, c) for b in blurs for s in sliders for c in closings]
    assert sorted(os.listdir(out)) == sorted(names + ["thresholds.json"])
    for k, name in enumerate(names):
        assert np.count_nonzero(_bgr16(os.path.join(out, name)) != want[k]) == 0, name
    with open(os.path.join(out, "thresholds.json")) as f:
        got = json.load(f)
    assert got == ref.foreground_json(blurs, sliders, closings, counts, cases.FG_W, cases.FG_H)
    assert got["images"][1]["threshold"] == "--threshold=4.000e-02" and got["images"][2]["count"] == 0


def test_foreground_scaled_to_width(built, tmp_path):
    from facebook360_dep_amd import imageio as dio

    template, frame = cases.foreground_pair()
    big_t = np.repeat(np.repeat(template, 2, axis=0), 2, axis=1)
    big_f = np.repeat(np.repeat(frame, 2, axis=0), 2, axis=1)
    bg, fg, out = str(tmp_path / "bg.png"), str(tmp_path / "fg.png"), str(tmp_path / "out")
    dio.write_png16(bg, big_t)
    dio.write_png16(fg, big_f)
    _run("ViewForegroundMaskThresholds", "--fullsize_bg_image=" + bg, "--fullsize_fg_image=" + fg, "--width=40", "--output=" + out)
    want, _, counts = ref.foreground(ref.scaled(big_t, 40), ref.scaled(big_f, 40), [1], [4], [4])
    assert np.count_nonzero(_bgr16(os.path.join(out, "blur_01_thresh_004_close_04.png")) != want[0]) == 0
    with open(os.path.join(out, "thresholds.json")) as f:
        assert json.load(f) == ref.foreground_json([1], [4], [4], counts, 40, 30)


def test_keypoint_projection_files(built, tmp_path):
    """one <id0>_<id1>.png per pair, equal to derp_preview_keypoints on the images as the tool loads them"""
    import json as js

    from facebook360_dep_amd import derp
    from facebook360_dep_amd import imageio as dio

    cams = cases.keypoint_rig()
    root, out = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(root)
    with open(os.path.join(root, "rig.json"), "w") as f:
        js.dump({"cameras": cams}, f)
    rng = np.random.default_rng(21)
    loaded = []
    for cam in cams:
        os.makedirs(os.path.join(root, "color", cam["id"]))
        bgr = rng.integers(0, 65536, (cases.KP_H, cases.KP_W, 3)).astype(np.uint16)
        dio.write_png16(os.path.join(root, "color", cam["id"], "000000.png"), bgr)
        im = np.ones((cases.KP_H, cases.KP_W, 4), np.float32)  # loadImage<cv::Vec4f>: x 1.0f / 65535.0f, alpha 1
        im[:, :, :3] = bgr.astype(np.float32) * (np.float32(1) / np.float32(65535))
        loaded.append(im)
    _run("GenerateKeypointProjections", "--rig=" + os.path.join(root, "rig.json"), "--color=" + os.path.join(root, "color"),
         "--frame=000000", "--output_dir=" + out, "--length_stride=0.25", "--height_stride=0.25", "--depth_samples=50",
         "--search_radius=3")
    assert sorted(os.listdir(out)) == ["cam0_cam1.png", "cam0_cam2.png", "cam1_cam2.png"]
    from oracle import oracle_lib

    rig = oracle_lib.Rig(cams)
    g = derp.Derp(cams)
    try:
        g.sweep_upload(loaded, [(cases.KP_W, cases.KP_H)] * 3)
        for c0 in range(3):
            for c1 in range(c0 + 1, 3):
                got = dio.read_png(os.path.join(out, "cam%d_cam%d.png" % (c0, c1)))
                assert got.dtype == np.uint8 and got.shape == (cases.KP_H, cases.KP_W, 4)
                api, _ = g.preview_keypoints(c0, c1, **cases.KP_BASE)
                rects, _ = ref.keypoint_rects(rig, c0, c1, cases.KP_W, cases.KP_H, cases.KP_W, cases.KP_H, **cases.KP_BASE)
                want = ref.keypoint_blend(loaded[c0], rects)[1]
                assert np.count_nonzero(got != api) == 0 and np.count_nonzero(got != want) == 0
    finally:
        g.close()
