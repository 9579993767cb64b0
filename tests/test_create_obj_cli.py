"""The process boundary of bin/CreateObjFromDisparityEquirect without a GPU: --helpxml against the flag table pinned
from the reference (tests/golden/ref_flags_create_obj_from_disparity_equirect.json, written by
gen_ref_pins_create_obj_from_disparity_equirect.py), and the checks that refuse bad input before any file is read or
written and before a device is opened."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "facebook360_dep_amd", "bin", "CreateObjFromDisparityEquirect")
GOLD = os.path.join(ROOT, "tests", "golden", "ref_flags_create_obj_from_disparity_equirect.json")


def run(*args):
    p = subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=120)
    return p.returncode, p.stderr


@pytest.mark.parametrize("binary,count", [("CreateObjFromDisparityEquirect", 10), ("PngToPfm", 2)])
def test_flag_table_matches_the_reference(built, binary, count):
    with open(GOLD) as f:
        ref = json.load(f)[binary]["flags"]
    mine = _helpxml(binary)
    assert len(ref) == count
    type_of = {"string": "string", "integer": "int32", "float": "double", "boolean": "bool"}
    for fl in ref:
        name = fl["name"]
        assert name in mine, name
        got = mine[name]
        assert got["type"] == type_of[fl["type"]], name
        if fl["type"] == "string":
            assert got["default"] == _cxx_literal(fl["default"]), name
        elif fl["type"] == "boolean":
            assert (got["default"] == "true") == bool(fl["default"]), name
        else:
            assert float(got["default"]) == float(fl["default"]), name
        assert got["meaning"] == _cxx_literal(fl["descr"]), (name, got["meaning"])
    names = {fl["name"] for fl in ref}
    for name, got in mine.items():
        assert name in names or "[extension" in got["meaning"] or got["meaning"].startswith("glog:"), name
    if binary == "CreateObjFromDisparityEquirect":
        assert mine["simplifier"]["default"] == "sequential" and mine["device"]["default"] == "0"


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from facebook360_dep_amd import imageio as dio

    root = str(tmp_path_factory.mktemp("obj_in"))
    dio.write_png16(os.path.join(root, "disp.png"), np.full((4, 8), 20000, np.uint16))
    dio.write_png8(os.path.join(root, "color.png"), np.full((4, 8, 3), 128, np.uint8))
    return root


@pytest.mark.parametrize("args,message", [
    (["--input_png_disp="], 'Check failed: F.s("input_png_disp") != ""'),
    (["--input_png_color="], 'Check failed: F.s("input_png_color") != ""'),
    (["--output_obj="], 'Check failed: F.s("output_obj") != ""'),
    (["--strictness=-0.1"], "strictness must be between 0 and 1"),
    (["--strictness=1.5"], "strictness must be between 0 and 1"),
    (["--strictness=nan"], "strictness must be between 0 and 1"),
    (["--simplifier=fast"], "Invalid --simplifier=fast"),
    (["--scale=0"], "scale must be in (0, 1]"),
    (["--scale=-1"], "scale must be in (0, 1]"),
    (["--scale=1.5"], "scale must be in (0, 1]"),
    (["--bogus_flag=1"], "bogus_flag"),
])
def test_bad_input_exits_nonzero(built, inputs, args, message):
    out = os.path.join(inputs, "out", "mesh.obj")
    base = ["--input_png_disp=" + os.path.join(inputs, "nosuch.png"),  # refused before the disparity is looked for
            "--input_png_color=" + os.path.join(inputs, "color.png"), "--output_obj=" + out, "--create_mtl",
            "--device=99"]  # no such device: a run that got as far as opening one fails in other words
    rc, err = run(*(base + args))
    assert rc != 0 and message in err, (rc, err[-600:])
    assert "derp_create failed" not in err and "failed to load image" not in err
    assert not os.path.exists(os.path.dirname(out))


def test_a_good_command_line_gets_as_far_as_the_device(built, inputs):
    """... which this machine need not have: with --device=99 the first failure is derp_create's, after the PNG was read"""
    out = os.path.join(inputs, "mesh.obj")
    rc, err = run("--input_png_disp=" + os.path.join(inputs, "disp.png"), "--input_png_color=" + os.path.join(inputs, "color.png"),
                  "--output_obj=" + out, "--scale=0.5", "--device=99")
    assert rc != 0 and "derp_create failed" in err, err[-600:]
    assert not os.path.exists(out) and not os.path.exists(os.path.join(inputs, "mesh.mtl"))
