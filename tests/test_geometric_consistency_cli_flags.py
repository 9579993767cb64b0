"""The process boundary of bin/GeometricConsistency without a GPU: --helpxml against the flag table pinned from the
reference's source (tests/golden/ref_flags_geometric_consistency.json, written by gen_ref_pins_geometric_consistency.py
with the reference's own get_flags scraper), the checks that refuse bad input before any device is opened, and the
tool's output files (cli/geometric_io.h) through a small native harness: the 16-bit disparity PNG's scaling."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


def test_flag_table_matches_the_reference(built):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_geometric_consistency.json")) as f:
        ref = json.load(f)["GeometricConsistency"]["flags"]
    mine = _helpxml("GeometricConsistency")
    assert sorted(fl["name"] for fl in ref) == ["agree_fraction", "color", "disparity_step", "downscale", "first", "keep_clean",
                                                "last", "median", "output", "pass_count", "rig", "single"]
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
        assert got["meaning"] == want or got["meaning"].startswith(want + " ["), (name, got["meaning"], want)
    for name in ("median", "single"):  # parsed and unused, as in the reference: --help says so
        assert "unused" in mine[name]["meaning"]
    p = subprocess.run([os.path.join(BIN, "GeometricConsistency"), "--help"], capture_output=True, text=True, timeout=60)
    assert "--median and --single are parsed and unused" in p.stdout + p.stderr
    names = {fl["name"] for fl in ref}
    for name, got in mine.items():
        assert name in names or "[extension" in got["meaning"] or got["meaning"].startswith("glog:"), name


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """rigs, and one (empty) image file per camera where verifyImagePaths looks"""
    from facebook360_dep_amd import synth

    root = str(tmp_path_factory.mktemp("gc_in"))
    rig = synth.make_rig(2, 16)
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump(rig, f)
    far = synth.make_rig(2, 16, radius=1.0)  # the mean distance from the origin is 1 m: asin has no value from there on
    with open(os.path.join(root, "rig_far.json"), "w") as f:
        json.dump(far, f)
    for cam in rig["cameras"]:
        os.makedirs(os.path.join(root, "color", cam["id"]))
        open(os.path.join(root, "color", cam["id"], "000000.png"), "w").close()
    return root


@pytest.mark.parametrize("args,message", [
    (["--rig="], "Check failed"),
    (["--bogus_flag=1"], "bogus_flag"),
    (["--color="], "color"),
    (["--output="], "output"),
    (["--first="], "first"),
    (["--last="], "last"),
    (["--threads=0"], "threads"),
    (["--downscale=0"], "downscale > 0"),
    (["--pass_count=-1"], "pass_count >= 0"),
    (["--downscale=8"], "3 x 3 at least"),
    (["--rig=RIG_FAR"], "less than 1 m"),
    (["--disparity_step=100"], "sliceCount 0 < 1"),
    (["--disparity_step=0"], "disparity_step must be positive"),
    (["--last=000003"], "Missing file"),
    (["--first=000005", "--last=000005"], "Missing file"),
])
def test_bad_input_exits_nonzero(built, tree, args, message):
    """every refusal by its message; none of them opens a device (this machine has none: a tool that got as far as
    derp_create would say "no HIP device")"""
    base = ["--rig=" + os.path.join(tree, "rig.json"), "--color=" + os.path.join(tree, "color"),
            "--output=" + os.path.join(tree, "out"), "--first=000000", "--last=000000", "--downscale=2"]
    args = [a.replace("RIG_FAR", os.path.join(tree, "rig_far.json")) for a in args]
    p = subprocess.run([os.path.join(BIN, "GeometricConsistency")] + base + args, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and message in p.stderr, (p.returncode, p.stderr)
    assert "no HIP device" not in p.stderr and "derp_create" not in p.stderr
    assert not os.path.exists(os.path.join(tree, "out"))


def test_host_slice_count_matches_the_restatement(built):
    from facebook360_dep_amd import derp, synth
    from tests import geometric_ref as G
    from tests.conversion_ref import rescaled_rig

    cams = synth.make_rig(4, 64)["cameras"]
    sizes = [(32, 32), (25, 19), (32, 19), (16, 16)]
    rig = rescaled_rig(cams, sizes)
    for step in (0.5, 0.25, 0.0787, 0.013):
        for d in range(4):
            assert derp.gc_slice_count(cams, d, sizes[d], step) == G.slice_count(rig, d, step), (step, d)
    with pytest.raises(derp.DerpError, match="sliceCount 0 < 1"):
        derp.gc_slice_count(cams, 0, (32, 32), 100.0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geometric") / "geometric_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "geometric_main.cpp"), "-lz", "-ldl"])
    return exe


def harness_run(exe, *args, stdin=None):
    p = subprocess.run([exe] + list(args), input=stdin, capture_output=True, text=True, timeout=60)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-1500:]
    return p


def test_disparity_png_scaling(harness, tmp_path):
    """<name>_disparity.png is 1 / depth through cv_util::convertTo<uint16_t>: the float quotient times 65535 in fp32,
    rounded to the nearest integer with halves to even, saturated to 0 .. 65535, NaN -> 0; the .pfm holds the depth"""
    from facebook360_dep_amd import imageio as dio

    F32 = np.float32
    hand = {2.0: 32768,        # 0.5 * 65535 = 32767.5: the tie goes to the even 32768
            4.0: 16384,        # 16383.75
            1.0: 65535, 0.5: 65535, 0.99: 65535,   # nearer than 1 m: saturated
            10000.0: 7,        # 6.5535
            131070.0: 0,       # exactly 0.5: the tie goes to the even 0
            43690.0: 2,        # exactly 1.5 -> 2
            26214.0: 2,        # exactly 2.5 -> 2
            float("inf"): 0, float("nan"): 0, -3.0: 0, 0.0: 65535}  # (1 / 0 = inf: saturated)
    depths = list(hand) + list(np.random.default_rng(5).uniform(1.0, 50.0, 32 - len(hand)))
    depth = np.array(depths, F32).reshape(4, 8)
    path = str(tmp_path / "cam0_iffy")
    text = "\n".join("%08x" % struct.unpack("<I", struct.pack("<f", v))[0] for v in depth.reshape(-1)) + "\n"
    p = harness_run(harness, "dump", path, "8", "4", stdin=text)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["cam0_iffy.pfm", "cam0_iffy_disparity.png"]
    assert np.array_equal(dio.read_pfm(path + ".pfm"), depth, equal_nan=True)
    png = dio.read_png(path + "_disparity.png")
    assert png.dtype == np.uint16 and png.shape[:2] == (4, 8)
    png = png.reshape(-1)
    for k, (d, want) in enumerate(hand.items()):
        assert png[k] == want, (d, png[k], want)
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = (F32(1) / depth.reshape(-1)) * F32(65535)
    want = np.where(np.isnan(scaled), 0, np.clip(np.rint(scaled.astype(np.float64)), 0, 65535)).astype(np.uint16)
    assert scaled.dtype == F32 and np.array_equal(png, want)


def test_small_size_rounds_half_away(harness):
    from tests import geometric_ref as G

    res = [(64, 64), (50, 38), (10, 6), (2048, 2048), (101, 99)]
    for downscale in (2.0, 4.0, 3.0):
        p = harness_run(harness, "small", repr(downscale), stdin="".join("%d %d\n" % r for r in res))
        got = [tuple(int(v) for v in line.split()) for line in p.stdout.split("\n")[:-1]]
        assert got == G.small_sizes([{"resolution": list(r)} for r in res], downscale), downscale
