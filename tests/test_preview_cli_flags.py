"""The process boundary of bin/ViewColorVarianceThresholds, bin/ViewForegroundMaskThresholds and
bin/GenerateKeypointProjections without a GPU: --helpxml
against the flag tables pinned from the reference's sources (tests/golden/ref_flags_preview.json, written by
gen_ref_pins_preview.py with the reference's own get_flags scraper) and the checks that refuse bad input before any
device is opened."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")
TOOLS = {"ViewColorVarianceThresholds": 4, "ViewForegroundMaskThresholds": 5, "GenerateKeypointProjections": 12}
EXTENSIONS = {"ViewColorVarianceThresholds": {"output", "low_sliders", "high_sliders", "device"},
              "ViewForegroundMaskThresholds": {"output", "blur_radii", "threshold_sliders", "closing_sizes", "device"},
              "GenerateKeypointProjections": {"device"}}
DEFAULTS = {"low_sliders": "2", "high_sliders": "2", "blur_radii": "1", "threshold_sliders": "4", "closing_sizes": "4"}


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_flag_table_matches_the_reference(built, tool):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_preview.json")) as f:
        ref = json.load(f)[tool]["flags"]
    assert len(ref) == TOOLS[tool]
    mine = _helpxml(tool)
    type_of = {"string": "string", "integer": "int32", "float": "double", "boolean": "bool"}
    for fl in ref:
        name = fl["name"]
        assert name in mine, name
        got = mine[name]
        assert got["type"] == type_of[fl["type"]], name
        if fl["type"] == "string":
            assert got["default"] == _cxx_literal(fl["default"]), name
        else:
            assert float(got["default"]) == float(fl["default"]), name
        assert got["meaning"] == _cxx_literal(fl["descr"]), (name, got["meaning"])
    names = {fl["name"] for fl in ref}
    extensions = {name for name, got in mine.items() if name not in names and not got["meaning"].startswith("glog:")}
    assert extensions == EXTENSIONS[tool]
    for name in extensions:
        assert "[extension]" in mine[name]["meaning"], name
        if name in DEFAULTS:
            assert mine[name]["default"] == DEFAULTS[name], name


def test_default_sliders_are_where_the_reference_window_opens():
    # sliderLowVal = varNoiseFloor / varLowMax * sliderMaxCount, float arithmetic truncated to int (:100-101; :106)
    f = np.float32
    assert int(f(1e-4) / f(4e-3) * f(100)) == 2 and int(f(1e-3) / f(5e-2) * f(100)) == 2
    assert int(f(0.04) / f(1.0) * f(100)) == 4


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from facebook360_dep_amd import imageio as dio

    root = str(tmp_path_factory.mktemp("preview_in"))
    rng = np.random.default_rng(0)
    dio.write_png16(os.path.join(root, "a.png"), rng.integers(0, 65535, (6, 8, 3)).astype(np.uint16))
    dio.write_png16(os.path.join(root, "b.png"), rng.integers(0, 65535, (6, 8, 3)).astype(np.uint16))
    dio.write_png16(os.path.join(root, "other_size.png"), rng.integers(0, 65535, (6, 10, 3)).astype(np.uint16))
    return root


def _refused(tool, tree, base, args, message):
    args = [a.replace("TREE", tree) for a in args]
    p = subprocess.run([os.path.join(BIN, tool)] + base + args, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and message in p.stderr, (p.returncode, p.stderr)
    assert "no HIP device" not in p.stderr and "derp_create" not in p.stderr
    assert not os.path.exists(os.path.join(tree, "out"))
    assert "ERROR: " in p.stderr or any(line.startswith("F") and "] " in line for line in p.stderr.split("\n")), p.stderr


MANY = ",".join(str(i) for i in range(17))  # 17 x 17 = 289 pairs


@pytest.mark.parametrize("args,message", [
    (["--fullsize_image="], "fullsize_image"),
    (["--output="], "output"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--fullsize_image=TREE/missing.png"], "Missing file"),
    (["--var_low_max=0"], "var_low_max > 0"),
    (["--var_high_max=-1"], "var_high_max > 0"),
    (["--width=-1"], "width >= 0"),
    (["--low_sliders=101"], "101 is outside 0..100"),
    (["--high_sliders=-1"], "is not an integer"),
    (["--high_sliders=2,,3"], "is not an integer"),
    (["--low_sliders=1.5"], "is not an integer"),
    (["--low_sliders=x"], "is not an integer"),
    (["--low_sliders=" + MANY, "--high_sliders=" + MANY], "at most 256"),
    (["--width=9"], "enlarging"),
])
def test_variance_refuses_bad_input(built, tree, args, message):
    base = ["--fullsize_image=" + os.path.join(tree, "a.png"), "--width=0", "--output=" + os.path.join(tree, "out")]
    _refused("ViewColorVarianceThresholds", tree, base, args, message)


@pytest.mark.parametrize("args,message", [
    (["--fullsize_bg_image="], "fullsize_bg_image"),
    (["--fullsize_fg_image="], "fullsize_fg_image"),
    (["--output="], "output"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--fullsize_fg_image=TREE/missing.png"], "Missing file"),
    (["--fullsize_fg_image=TREE/other_size.png"], "imageBg.size() == imageFg.size()"),
    (["--blur_radius_max=0"], "blur_radius_max > 0"),
    (["--morph_closing_size_max=0"], "morph_closing_size_max > 0"),
    (["--width=-3"], "width >= 0"),
    (["--blur_radii=21"], "21 is outside 0..20"),
    (["--blur_radii=1,4"], "a blur radius of 4 is not supported"),
    (["--blur_radii=20"], "a blur radius of 20 is not supported"),
    (["--blur_radius_max=2", "--blur_radii=3"], "3 is outside 0..2"),
    (["--closing_sizes=21"], "21 is outside 0..20"),
    (["--morph_closing_size_max=5", "--closing_sizes=4,6"], "6 is outside 0..5"),
    (["--threshold_sliders=101"], "101 is outside 0..100"),
    (["--threshold_sliders=4.5"], "is not an integer"),
    (["--blur_radii=0,1,2,3", "--threshold_sliders=" + MANY, "--closing_sizes=0,1,2,3"], "at most 256"),
    (["--width=9"], "enlarging"),
])
def test_foreground_refuses_bad_input(built, tree, args, message):
    base = ["--fullsize_bg_image=" + os.path.join(tree, "a.png"), "--fullsize_fg_image=" + os.path.join(tree, "b.png"),
            "--width=0", "--output=" + os.path.join(tree, "out")]
    _refused("ViewForegroundMaskThresholds", tree, base, args, message)


@pytest.fixture(scope="module")
def rig_tree(tmp_path_factory):
    """a 64 x 48 rig with one image per camera, and a second colour directory in which one image has another size"""
    from facebook360_dep_amd import imageio as dio
    from tests import preview_cases as cases

    root = str(tmp_path_factory.mktemp("keypoints_in"))
    cams = cases.keypoint_rig()
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump({"cameras": cams}, f)
    for name, odd in (("color", None), ("color_odd", "cam1")):
        for cam in cams:
            os.makedirs(os.path.join(root, name, cam["id"]))
            shape = (cases.KP_H, cases.KP_W + (2 if cam["id"] == odd else 0), 3)
            dio.write_png16(os.path.join(root, name, cam["id"], "000000.png"), np.full(shape, 1000, np.uint16))
    return root


@pytest.mark.parametrize("args,message", [
    (["--rig="], "rig"),
    (["--output_dir="], "output_dir"),
    (["--color="], "color"),
    (["--frame="], "frame"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--corners=1"], "corners"),  # the rest of the calibration library's flags are not offered
    (["--frame=000007"], "Missing file"),
    (["--color=TREE/color_odd"], "the image of cam1 is 66 x 48, not the first camera's resolution 64 x 48"),
    (["--length_stride=0"], "length_stride must be a positive finite number"),
    (["--height_stride=-0.5"], "height_stride must be a positive finite number"),
    (["--height_stride=inf"], "height_stride must be a positive finite number"),
    (["--length_stride=nan"], "length_stride must be a positive finite number"),
    (["--length_stride=1e-4", "--height_stride=1e-4"], "make more than 1048576 grid points"),
    (["--search_radius=-1"], "search_radius >= 0"),
    (["--depth_samples=1"], "depth_samples >= 2"),
    (["--depth_min=0"], "depth_min > 0"),
    (["--depth_max=0.5"], "depth_max >= depth_min"),
])
def test_keypoints_refuses_bad_input(built, rig_tree, args, message):
    base = ["--rig=" + os.path.join(rig_tree, "rig.json"), "--color=" + os.path.join(rig_tree, "color"), "--frame=000000",
            "--output_dir=" + os.path.join(rig_tree, "out")]
    _refused("GenerateKeypointProjections", rig_tree, base, args, message)
