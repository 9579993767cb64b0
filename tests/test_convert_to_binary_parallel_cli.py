"""bin/ConvertToBinary's --simplifier flag at the process boundary, without a GPU: it is listed as an extension, and a
value other than sequential / parallel is refused by name before any file or device is opened."""
import json
import os
import subprocess

import pytest

from tests.test_ref_pins import _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "facebook360_dep_amd", "bin", "ConvertToBinary")


def test_helpxml_lists_the_flag_as_an_extension(built):
    flags = _helpxml("ConvertToBinary")
    assert "simplifier" in flags, sorted(flags)
    got = flags["simplifier"]
    assert got["meaning"].startswith("[extension]") and "sequential" in got["meaning"] and "parallel" in got["meaning"]
    assert got["default"] == "sequential" and got["type"] == "string"


@pytest.mark.parametrize("value", ["bogus", "", "Parallel"])
def test_unknown_simplifier_is_refused_before_anything_is_opened(built, tmp_path, value):
    from facebook360_dep_amd import synth

    with open(tmp_path / "rig.json", "w") as f:
        json.dump(synth.make_rig(2, 16), f)
    # no disparity directory exists and there is no device 99: a run that got as far as either fails in other words
    p = subprocess.run([EXE, "--rig=" + str(tmp_path / "rig.json"), "--disparity=" + str(tmp_path / "disparity"),
                        "--bin=" + str(tmp_path / "bin"), "--first=000000", "--last=000000", "--output_formats=idx,vtx",
                        "--device=99", "--simplifier=" + value], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "Invalid --simplifier=%s (sequential or parallel)" % value in p.stderr, p.stderr[-600:]
    assert "derp_create" not in p.stderr and "Missing file" not in p.stderr
    assert not os.path.exists(tmp_path / "bin")
