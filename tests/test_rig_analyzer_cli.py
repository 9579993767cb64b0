"""The process boundary of bin/RigAnalyzer without a GPU: --helpxml against the flag table pinned from the reference's
source (tests/golden/ref_flags_rig_analyzer.json, written by gen_ref_pins_rig_analyzer.py with the reference's own
get_flags scraper), the refusals that fire before any device is opened, and pure rig edits, which open none: their rig
JSON and OBJ text against the restatement (tests/coverage_ref.py)."""
import json
import math
import os
import subprocess

import pytest

from tests import coverage_ref as R
from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "facebook360_dep_amd", "bin", "RigAnalyzer")
SYMBOLS = {"Camera::kNearInfinity": 1e4}  # static constexpr Real kNearInfinity = 1e4 (Camera.h)


def test_flag_table_matches_the_reference(built):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_rig_analyzer.json")) as f:
        ref = json.load(f)["RigAnalyzer"]["flags"]
    assert len(ref) == 30
    mine = _helpxml("RigAnalyzer")
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
            assert float(got["default"]) == float(SYMBOLS.get(fl["default"], fl["default"])), name
        assert got["meaning"] == _cxx_literal(fl["descr"]), (name, got["meaning"])
    names = {fl["name"] for fl in ref}
    extensions = {name for name, got in mine.items() if name not in names and not got["meaning"].startswith("glog:")}
    assert extensions == {"device"} and "[extension]" in mine["device"]["meaning"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory, built):
    from facebook360_dep_amd import synth
    from tests import common

    root = str(tmp_path_factory.mktemp("rig_analyzer"))
    oblong = synth.make_rig(2, 64)  # pixels that are not square: Camera::getScalarFocal's CHECK
    oblong["cameras"][1]["focal"] = [20.0, -21.0]
    for name, rig in (("rig4", synth.make_rig(4, 64)), ("real", common.real_rig()), ("empty", {"cameras": []}), ("oblong", oblong)):
        with open(os.path.join(root, name + ".json"), "w") as f:
            json.dump(rig, f)
    files = {"eulers.txt": "=== arrangement 1\n10 20 30\n-170 0.5 90\n", "revolve.txt": "0 0 0\n0.1 0.2 -0.3\n",
             "bad.txt": "1 2 3\n4 five 6\n", "short.txt": "1 2\n", "only_comments.txt": "=== nothing\n",
             "revolve64.txt": "".join("0 0 %g\n" % (0.01 * k) for k in range(64))}
    for name, text in files.items():
        with open(os.path.join(root, name), "w") as f:
            f.write(text)
    return root


def run(tree, args, rig="rig4"):
    args = [a.replace("TREE", tree) for a in args]
    return subprocess.run([TOOL, "--rig=" + os.path.join(tree, rig + ".json")] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,message", [
    (["--rig="], "Check failed"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--rig=TREE/empty.json"], "rig.size() > 0"),
    (["--sample_count=-1"], "sample_count >= 0"),
    (["--sample_count=1000", "--discard_poles=90"], "--discard_poles=90 leaves no sample of 1000"),
    (["--output_camera=TREE/out.pgm", "--output_camera_id=nobody"], "Camera id nobody not found"),
    (["--rearrange=cube", "--output_camera=TREE/out.pgm", "--output_camera_id=cam6"], "Camera id cam6 not found"),
    (["--output_camera=TREE/out.pgm"], "--output_camera and --output_camera_id go together"),
    (["--output_camera_id=cam0"], "--output_camera and --output_camera_id go together"),
    (["--eulers=TREE/bad.txt"], "bad line <4 five 6> in file"),
    (["--revolve=TREE/short.txt"], "bad line <1 2> in file"),
    (["--eulers=TREE/only_comments.txt"], "no angles in file"),
    (["--revolve=TREE/missing.txt"], "could not read file"),
    (["--rearrange=octo"], "unknown arrangement octo"),
    (["--rotate=1 2"], "bad --rotate vector 1 2"),
    (["--rotate=1 2 3 4"], "bad --rotate vector 1 2 3 4"),
    (["--rotate_cam_z=nobody"], "Camera id nobody not found"),
    (["--revolve=TREE/revolve64.txt", "--output_cross_section=TREE/out.pgm"], "too many cameras (256 > 255)"),
    (["--perturb_cameras", "--perturb_focals=1"], "pixels are not square"),
])
def test_refusals_fire_without_a_device(tree, args, message):
    p = run(tree, args, "oblong" if "not square" in message else "rig4")
    assert p.returncode != 0 and message in p.stderr, (p.returncode, p.stderr)
    assert "no HIP device" not in p.stderr and "derp_create" not in p.stderr
    assert not os.path.exists(os.path.join(tree, "out.pgm"))
    assert "ERROR: " in p.stderr or any(line.startswith("F") and "] " in line for line in p.stderr.split("\n")), p.stderr


def rig_of(name):
    from facebook360_dep_amd import synth
    from tests import common

    return synth.make_rig(4, 64)["cameras"] if name == "rig4" else common.real_rig()["cameras"]


EDITS = {
    "cube": ("rig4", ["--rearrange=cube"], lambda c: R.rig_arrangement("cube", c[0])),
    "tetra_custom_one_based": ("real", ["--rearrange=tetra", "--custom=120", "--one_based_indexing"],
                               lambda c: R.rig_arrangement("tetra", c[0], 120.0, True)),
    "eulers": ("rig4", ["--eulers=TREE/eulers.txt"], lambda c: R.rig_from_eulers(c[0], [(10, 20, 30), (-170, 0.5, 90)])),
    "revolve_z_up": ("real", ["--revolve=TREE/revolve.txt", "--z_is_up"],
                     lambda c: R.rig_rotate(R.rig_revolve(c, [(0, 0, 0), (0.1, 0.2, -0.3)]), [[1, 0, 0], [0, 0, -1], [0, 1, 0]])),
    "z_down_scaled": ("real", ["--z_is_down", "--scale_rig=0.01", "--scale_resolution=0.25"],
                      lambda c: R.rig_scale(R.rig_rotate(c, [[1, 0, 0], [0, 0, 1], [0, -1, 0]]), 0.01, 0.0, 0.25)),
    "rotate_radius": ("rig4", ["--rotate=0.4 0.5 0.6", "--radius=0.5"],
                      lambda c: R.rig_scale(R.rig_rotate(c, R.euler_matrix((0.4, 0.5, 0.6))), 1.0, 0.5, 1.0)),
    "cam_z": ("rig4", ["--radius=1", "--rotate_cam_z=cam2"], lambda c: R.rig_scale(R.rig_rotate(c, R.align_z_matrix(R.loaded(c)[2]["origin"])), 1.0, 1.0, 1.0)),
    "perturb": ("real", ["--perturb_cameras", "--perturb_seed=7", "--perturb_positions=0.01", "--perturb_rotations=0.02",
                         "--perturb_principals=3"], lambda c: R.rig_perturb(c, 7, 0.01, 0.02, 3.0, 0.0)),
    "perturb_focals": ("rig4", ["--perturb_cameras", "--perturb_focals=2"], lambda c: R.rig_perturb(c, 1, 0.0, 0.0, 0.0, 2.0)),
    "untouched": ("real", [], lambda c: R.loaded(c)),
}


@pytest.mark.parametrize("name", sorted(EDITS))
def test_pure_rig_edit_needs_no_device(tree, name):
    """--sample_count=0 with no map: the rig JSON and the OBJ text are the restatement's, on a machine with or without a GPU"""
    rig, args, want = EDITS[name]
    out_rig, out_obj = os.path.join(tree, name + ".json"), os.path.join(tree, name + ".obj")
    p = run(tree, args + ["--sample_count=0", "--output_rig=" + out_rig, "--output_obj=" + out_obj], rig)
    assert p.returncode == 0 and p.stdout == "", (p.stdout, p.stderr)
    assert "derp_create" not in p.stderr
    cams = rig_of(rig)
    want = want(cams)
    if name == "untouched":  # (the tool writes the rotation rows as the file held them: rig_writer.h)
        want = [R._floats(c) for c in cams]
    with open(out_rig) as f:
        doc = json.load(f)
    assert doc["comments"][0] == "command line:" and "--output_rig=" + out_rig in doc["comments"][1]
    got = doc["cameras"]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert R.same_camera(g, w), (g, w)
        assert g["type"] == w["type"] and g.get("distortion") == w.get("distortion")
        assert ("fov" in g) == ("fov" in w) and ("fov" not in g or g["fov"] == math.acos(math.cos(w["fov"])))
    with open(out_obj) as f:
        assert f.read() == R.rig_obj(want)
