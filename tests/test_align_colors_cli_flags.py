"""The process boundary of bin/AlignColors without a GPU: --helpxml against the flag table pinned from the reference's
source (tests/golden/ref_flags_align_colors.json, written by gen_ref_pins_align_colors.py with the reference's own
get_flags scraper) and the checks that refuse bad input before any device is opened. This machine has no device, so a
refusal that came after derp_create would read "no HIP device" instead of its own message."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import align_cases as AC
from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


def test_flag_table_matches_the_reference(built):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_align_colors.json")) as f:
        ref = json.load(f)["AlignColors"]["flags"]
    assert sorted(fl["name"] for fl in ref) == ["calibrated_rig", "cameras", "color", "first", "last", "output", "rig_blue",
                                                "rig_green", "rig_red"]
    mine = _helpxml("AlignColors")
    for fl in ref:
        name = fl["name"]
        assert name in mine, name
        got = mine[name]
        assert fl["type"] == "string" and got["type"] == "string", name
        assert got["default"] == _cxx_literal(fl["default"]) == "", name
        assert got["meaning"] == _cxx_literal(fl["descr"]), (name, got["meaning"])
    names = {fl["name"] for fl in ref}
    extensions = {name for name, got in mine.items() if name not in names and not got["meaning"].startswith("glog:")}
    assert extensions == {"device", "threads"}
    for name in extensions:
        assert "[extension]" in mine[name]["meaning"], name


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """the mixed rig with its reference rigs, two frames of every camera, and the files the refusals need"""
    from facebook360_dep_amd import imageio as dio

    root = str(tmp_path_factory.mktemp("align_in"))
    case = AC.all_cases()["mixed_rig"]

    def rig_file(name, cams):
        with open(os.path.join(root, name), "w") as f:
            json.dump({"cameras": cams}, f)

    rig_file("rig_calibrated.json", case["rig"])
    rig_file("rig_red.json", [case["red_ref"]])
    rig_file("rig_green.json", [case["green_ref"]])
    rig_file("rig_blue.json", [case["blue_ref"]])
    rig_file("rig_two.json", [case["green_ref"], dict(case["green_ref"], id="ref2")])
    rig_file("rig_none.json", [])
    rig_file("rig_oblong.json", [dict(case["rig"][0], focal=[22.0, -23.0])] + case["rig"][1:])
    rng = np.random.default_rng(5)
    for cam in case["rig"]:
        w, h = cam["resolution"]
        os.makedirs(os.path.join(root, "color", cam["id"]))
        os.makedirs(os.path.join(root, "color_small", cam["id"]))
        for frame in (0, 1):
            dio.write_png16(os.path.join(root, "color", cam["id"], "%06d.png" % frame), rng.integers(0, 65536, (h, w, 3), dtype=np.uint16))
            dio.write_png16(os.path.join(root, "color_small", cam["id"], "%06d.png" % frame),
                            rng.integers(0, 65536, (h - 1, w, 3), dtype=np.uint16))
    return root


def _base(tree):
    return ["--calibrated_rig=" + os.path.join(tree, "rig_calibrated.json"), "--rig_red=" + os.path.join(tree, "rig_red.json"),
            "--rig_green=" + os.path.join(tree, "rig_green.json"), "--rig_blue=" + os.path.join(tree, "rig_blue.json"),
            "--color=" + os.path.join(tree, "color"), "--output=" + os.path.join(tree, "out")]


@pytest.mark.parametrize("args,message", [
    (["--color="], "color"),
    (["--calibrated_rig="], "calibrated_rig"),
    (["--rig_red="], "rig_red"),
    (["--rig_green="], "rig_green"),
    (["--rig_blue="], "rig_blue"),
    (["--output="], "output"),
    (["--output=TREE/color"], "the output directory must differ from the color path"),
    (["--threads=0"], "threads"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--rig_red=TREE/rig_two.json"], "the red reference rig must hold exactly one camera (it holds 2)"),
    (["--rig_green=TREE/rig_two.json"], "the green reference rig must hold exactly one camera (it holds 2)"),
    (["--rig_blue=TREE/rig_none.json"], "the blue reference rig must hold exactly one camera (it holds 0)"),
    (["--calibrated_rig=TREE/rig_none.json"], "rig.size() > 0"),
    (["--calibrated_rig=TREE/rig_oblong.json"], "pixels are not square"),
    (["--calibrated_rig=TREE/absent.json"], "could not read JSON file"),
    (["--rig_blue=TREE/absent.json"], "could not read JSON file"),
    (["--cameras=cam1,nobody"], "unknown camera in --cameras: nobody"),
    (["--last=000002"], "Missing file"),
    (["--first=000001", "--last=000000"], "first <= last"),
    (["--color=TREE/absent"], "no images in"),
    (["--color=TREE/color_small"], "image size mismatch"),
])
def test_refuses_bad_input_before_a_device_is_opened(built, tree, args, message):
    args = [a.replace("TREE", tree) for a in args]
    p = subprocess.run([os.path.join(BIN, "AlignColors")] + _base(tree) + args, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and message in p.stderr, (p.returncode, p.stderr)
    assert "no HIP device" not in p.stderr and "derp_create" not in p.stderr
    assert not os.path.exists(os.path.join(tree, "out"))
    # a glog-style fatal line (F<date> <time> <file>:<line>] ...), or gflags' own "ERROR: ..." for a flag it rejects
    assert "ERROR: " in p.stderr or any(line.startswith("F") and "] " in line for line in p.stderr.split("\n")), p.stderr


def test_good_input_reaches_the_device_check(built, tree):
    """the same command line without a fault gets as far as opening the device (and, on this machine, no further)"""
    import torch

    if torch.cuda.is_available():
        return  # with a device the command would succeed and write `out`; tests/test_gpu_align_colors_cli.py covers that path
    p = subprocess.run([os.path.join(BIN, "AlignColors")] + _base(tree), capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "no HIP device" in p.stderr, p.stderr
    assert not os.path.exists(os.path.join(tree, "out"))
