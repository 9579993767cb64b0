"""The process boundary of bin/GenerateCameraOverlaps, bin/GenerateEquirect and bin/ProjectCamerasToEquirects without a
GPU: --helpxml against the flag tables pinned from the reference's sources (tests/golden/ref_flags_sweep.json, written by
gen_ref_pins_sweep.py with the reference's own get_flags scraper) and the checks that refuse bad input before any
device is opened."""
import json
import os
import subprocess

import pytest

from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")
TOOLS = {"GenerateCameraOverlaps": 9, "GenerateEquirect": 14, "ProjectCamerasToEquirects": 9}


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_flag_table_matches_the_reference(built, tool):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_sweep.json")) as f:
        ref = json.load(f)[tool]["flags"]
    assert len(ref) == TOOLS[tool]
    mine = _helpxml(tool)
    type_of = {"string": "string", "integer": "int32", "float": "double", "boolean": "bool", "uint64": "uint64"}
    for fl in ref:
        name = fl["name"]
        assert name in mine, name
        got = mine[name]
        assert got["type"] == type_of[fl["type"]], name
        if fl["type"] == "string":
            assert got["default"] == _cxx_literal(fl["default"]), name
        elif fl["type"] == "boolean":
            assert (got["default"] == "true") == bool(fl["default"]), name
        elif fl["type"] == "uint64":
            assert got["default"] == str(int(fl["default"])), name
        else:
            assert float(got["default"]) == float(fl["default"]), name
        assert got["meaning"] == _cxx_literal(fl["descr"]), (name, got["meaning"])
    names = {fl["name"] for fl in ref}
    extensions = {name for name, got in mine.items() if name not in names and not got["meaning"].startswith("glog:")}
    assert extensions == ({"device"} if tool == "GenerateEquirect" else {"device", "threads"})  # (GenerateEquirect has --threads)
    for name in extensions:
        assert "[extension]" in mine[name]["meaning"], name


def test_uint64_flags(built):
    mine = _helpxml("GenerateCameraOverlaps")
    assert [mine[n]["type"] for n in ("max_depth_m", "min_depth_m", "num_depths")] == ["uint64"] * 3
    for value in ("-1", "1.5", "x", "18446744073709551616"):
        p = subprocess.run([os.path.join(BIN, "GenerateCameraOverlaps"), "--num_depths=" + value], capture_output=True,
                           text=True, timeout=60)
        assert p.returncode != 0 and "illegal value" in p.stderr and "uint64" in p.stderr, (value, p.stderr)


@pytest.mark.parametrize("tool", ["GenerateCameraOverlaps", "GenerateEquirect"])
def test_help_says_that_the_label_is_not_drawn(built, tool):
    p = subprocess.run([os.path.join(BIN, tool), "--help"], capture_output=True, text=True, timeout=60)
    text = p.stdout + p.stderr
    assert p.returncode == 0 and "cv::putText" in text and "the depth is in" in text and "file name" in text


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """a rig, an empty rig, and one (empty) image file per camera where verifyImagePaths looks"""
    from facebook360_dep_amd import synth

    root = str(tmp_path_factory.mktemp("sweep_in"))
    rig = synth.make_rig(2, 16)
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump(rig, f)
    with open(os.path.join(root, "rig_empty.json"), "w") as f:
        json.dump({"cameras": []}, f)
    for cam in rig["cameras"]:
        os.makedirs(os.path.join(root, "color", cam["id"]))
        open(os.path.join(root, "color", cam["id"], "000000.png"), "w").close()
    return root


def _refused(tool, tree, base, args, message):
    args = [a.replace("RIG_EMPTY", os.path.join(tree, "rig_empty.json")) for a in args]
    p = subprocess.run([os.path.join(BIN, tool)] + base + args, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and message in p.stderr, (p.returncode, p.stderr)
    assert "no HIP device" not in p.stderr and "derp_create" not in p.stderr
    assert not os.path.exists(os.path.join(tree, "out"))
    # a glog-style fatal line (F<date> <time> <file>:<line>] ...), or gflags' own "ERROR: ..." for a flag it rejects
    assert "ERROR: " in p.stderr or any(line.startswith("F") and "] " in line for line in p.stderr.split("\n")), p.stderr


def _base(tree):
    return ["--rig=" + os.path.join(tree, "rig.json"), "--color=" + os.path.join(tree, "color"),
            "--output=" + os.path.join(tree, "out")]


@pytest.mark.parametrize("args,message", [
    (["--rig="], "Check failed"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--color="], "color"),
    (["--output="], "output"),
    (["--threads=0"], "threads"),
    (["--scale=0"], "scale in (0, 1]"),
    (["--scale=1.5"], "scale in (0, 1]"),
    (["--scale=-0.5"], "scale in (0, 1]"),
    (["--num_depths=0"], "num_depths >= 1"),
    (["--min_depth_m=0"], "depth > 0"),
    (["--max_depth_m=0"], "depth > 0"),
    (["--rig=RIG_EMPTY"], "rig.size() > 0"),
    (["--cameras=nobody"], "no destinations!"),
    (["--frame=000003"], "Missing file"),
])
def test_overlaps_refuses_bad_input(built, tree, args, message):
    _refused("GenerateCameraOverlaps", tree, _base(tree), args, message)


@pytest.mark.parametrize("args,message", [
    (["--rig="], "Check failed"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--color="], "color"),
    (["--output="], "output"),
    (["--scale=0"], "scale in (0, 1]"),
    (["--scale=2"], "scale in (0, 1]"),
    (["--num_depths=0"], "num_depths >= 1"),
    (["--depth_min=0"], "depth > 0"),
    (["--depth_max=-1"], "depth > 0"),
    (["--height=0"], "height in 1 .. 16384"),
    (["--rig=RIG_EMPTY"], "rig.size() > 0"),
    (["--cameras=nobody"], "rig.size() > 0"),
    (["--camera_id=nobody"], "Camera id nobody not found"),
    (["--cameras=cam0", "--camera_id=cam1"], "Camera id cam1 not found"),
    (["--frame=000003"], "Missing file"),
])
def test_equirect_refuses_bad_input(built, tree, args, message):
    _refused("GenerateEquirect", tree, _base(tree), args, message)


@pytest.mark.parametrize("args,message", [
    (["--rig="], "Check failed"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--color="], "color"),
    (["--output="], "output"),
    (["--first="], "first"),
    (["--last="], "last"),
    (["--threads=0"], "threads"),
    (["--depth=0"], "depth > 0"),
    (["--depth=-2"], "depth > 0"),
    (["--eqr_width=63"], "equirect width must be a multiple of 2"),
    (["--eqr_width=0"], "eqr_width >= 2"),
    (["--file_type=exr"], "unsupported --file_type exr"),
    (["--rig=RIG_EMPTY"], "rig.size() > 0"),
    (["--cameras=nobody"], "rig.size() > 0"),
    (["--last=000003"], "Missing file"),
])
def test_project_refuses_bad_input(built, tree, args, message):
    _refused("ProjectCamerasToEquirects", tree, _base(tree) + ["--first=000000", "--last=000000"], args, message)
