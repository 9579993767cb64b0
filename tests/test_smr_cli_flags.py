"""bin/SimpleMeshRenderer's process boundary without a GPU: --helpxml against the flag table pinned from the
reference's source (tests/golden/ref_flags_simple_mesh_renderer.json, written by gen_ref_pins_smr.py with the
reference's own get_flags scraper), and the checks that refuse bad input before any device is opened."""
import json
import os
import subprocess

import pytest

from tests import smr_dataset
from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "facebook360_dep_amd", "bin", "SimpleMeshRenderer")


def test_flag_table_matches_the_reference(built):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_simple_mesh_renderer.json")) as f:
        ref = json.load(f)["SimpleMeshRenderer"]["flags"]
    mine = _helpxml("SimpleMeshRenderer")
    assert len(ref) == 18
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
        want = _cxx_literal(fl["descr"])
        if want is None:  # --format's description is a variable (formatsCsv); the scraper cannot read it
            assert got["meaning"].endswith("(empty = on-screen rendering)"), got["meaning"]
            continue
        assert got["meaning"] == want or got["meaning"].startswith(want + " ["), (name, got["meaning"], want)
    names = {fl["name"] for fl in ref}
    for name, got in mine.items():
        assert name in names or "[extension" in got["meaning"] or got["meaning"].startswith("glog:"), name


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("smr_in"))
    smr_dataset.write(root, n=2, res=16, frames=(0,))
    return root


def run(*args):
    p = subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=60)
    return p.returncode, p.stderr


@pytest.mark.parametrize("args,message", [
    (["--bogus_flag=1"], "bogus_flag"),
    (["--format="], "on-screen rendering is not supported"),
    (["--format=cubecolorx"], "Invalid format"),
    (["--format=eqrcolor", "--color="], "eqrcolor needs --color to be set"),
    (["--format=eqrdisp", "--width=101"], "multiple of 2"),
    (["--format=eqrdisp", "--file_type=bmp"], "unsupported --file_type"),
])
def test_bad_input_exits_nonzero(built, tree, args, message):
    base = ["--rig=" + os.path.join(tree, "rig.json"), "--color=" + os.path.join(tree, "color"),
            "--disparity=" + os.path.join(tree, "disparity"), "--output=" + os.path.join(tree, "out")]
    rc, err = run(*(base + args))
    assert rc != 0 and message in err, (rc, err)
