"""The process boundary of bin/ExportPointCloud, bin/ImportPointCloud and bin/ProjectEquirectsToCameras without a GPU:
--helpxml against the flag tables pinned from the reference's sources (tests/golden/ref_flags_conversion.json, written
by gen_ref_pins_conversion.py with the reference's own get_flags scraper), the checks that refuse bad input before any
device is opened, and the text side of the point-cloud tools (cli/point_cloud_io.h) through a small native harness."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")
TOOLS = {"ExportPointCloud": 11, "ImportPointCloud": 8, "ProjectEquirectsToCameras": 10}


@pytest.mark.parametrize("binary", sorted(TOOLS))
def test_flag_table_matches_the_reference(built, binary):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_conversion.json")) as f:
        ref = json.load(f)[binary]["flags"]
    mine = _helpxml(binary)
    assert len(ref) == TOOLS[binary]
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
    names = {fl["name"] for fl in ref}
    for name, got in mine.items():
        assert name in names or "[extension" in got["meaning"] or got["meaning"].startswith("glog:"), name


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """a rig, and one (empty) image file per camera where verifyImagePaths looks"""
    from facebook360_dep_amd import synth

    root = str(tmp_path_factory.mktemp("conversion_in"))
    rig = synth.make_rig(2, 16)
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump(rig, f)
    for sub, ext in (("color", ".png"), ("disparity", ".pfm"), ("eqr_masks", ".png")):
        for cam in rig["cameras"]:
            os.makedirs(os.path.join(root, sub, cam["id"]))
            open(os.path.join(root, sub, cam["id"], "000000" + ext), "w").close()
    open(os.path.join(root, "points.xyz"), "w").write("1\n0 0 1\n")
    return root


def run(binary, *args):
    p = subprocess.run([os.path.join(BIN, binary)] + list(args), capture_output=True, text=True, timeout=60)
    return p.returncode, p.stderr


@pytest.mark.parametrize("binary,args,message", [
    ("ExportPointCloud", ["--rig="], "Check failed"),
    ("ExportPointCloud", ["--bogus_flag=1"], "bogus_flag"),
    ("ExportPointCloud", ["--threads=0"], "threads"),
    ("ExportPointCloud", ["--color="], "color"),
    ("ExportPointCloud", ["--disparity="], "disparity"),
    ("ExportPointCloud", ["--output="], "output"),
    ("ExportPointCloud", ["--subsample=0"], "subsample >= 1"),
    ("ExportPointCloud", ["--cameras=nosuchcam"], "rig.size() > 0"),
    ("ExportPointCloud", ["--frame=000007"], "Missing file"),
    ("ImportPointCloud", ["--rig="], "Check failed"),
    ("ImportPointCloud", ["--point_cloud="], "point_cloud"),
    ("ImportPointCloud", ["--output="], "output"),
    ("ImportPointCloud", ["--width=-2"], "width >= 0"),
    ("ImportPointCloud", ["--width=33"], "width must be a multiple of 2"),
    ("ImportPointCloud", ["--cameras=nosuchcam"], "rig.size() > 0"),
    ("ImportPointCloud", ["--point_cloud=/nonexistent/points.xyz"], "File does not exist"),
    ("ProjectEquirectsToCameras", ["--rig="], "Check failed"),
    ("ProjectEquirectsToCameras", ["--eqr_masks="], "eqr_masks"),
    ("ProjectEquirectsToCameras", ["--output="], "output"),
    ("ProjectEquirectsToCameras", ["--depth=0"], "depth > 0"),
    ("ProjectEquirectsToCameras", ["--width=33"], "equirect width must be a multiple of 2"),
    ("ProjectEquirectsToCameras", ["--file_type=bmp"], "unsupported --file_type"),
    ("ProjectEquirectsToCameras", ["--last=000003"], "Missing file"),
])
def test_bad_input_exits_nonzero(built, tree, binary, args, message):
    base = ["--rig=" + os.path.join(tree, "rig.json"), "--color=" + os.path.join(tree, "color"),
            "--disparity=" + os.path.join(tree, "disparity"), "--eqr_masks=" + os.path.join(tree, "eqr_masks"),
            "--point_cloud=" + os.path.join(tree, "points.xyz"), "--output=" + os.path.join(tree, "out")]
    known = _helpxml(binary)
    base = [a for a in base if a[2:].split("=")[0] in known]
    rc, err = run(binary, *(base + args))
    assert rc != 0 and message in err, (rc, err)


# ---------------------------------------------------------------- cli/point_cloud_io.h
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("points") / "point_cloud_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "point_cloud_main.cpp"), "-lz", "-ldl"])
    return exe


def harness_run(exe, *args, stdin=None):
    p = subprocess.run([exe] + list(args), input=stdin, capture_output=True, text=True, timeout=60)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-1500:]
    return p


def bits(values):
    return "\n".join("%08x" % struct.unpack("<I", struct.pack("<f", v))[0] for v in values) + "\n"


def test_float_formatter(harness):
    cases = [(1.5, "1.5"), (0.1, "0.1"), (4.0, "4"), (1e-5, "1e-05"), (float("nan"), "nan"), (float("inf"), "inf"),
             (float("-inf"), "-inf"), (0.0, "0"), (-0.0, "-0"), (-2.25, "-2.25"), (1e-4, "0.0001"), (123456.0, "123456"),
             (1e15, "1000000000000000"), (1e16, "1e+16"), (3.4028235e38, "3.4028235e+38"), (1e-45, "1e-45"),
             (0.001, "0.001"), (16777216.0, "16777216"), (-0.00012345, "-0.00012345")]
    p = harness_run(harness, "float", stdin=bits([c[0] for c in cases]))
    assert p.returncode == 0 and p.stdout.split("\n")[:-1] == [c[1] for c in cases]
    # 10 000 random bit patterns (every exponent): the text reads back as the same fp32 value, and is no longer than
    # numpy's own shortest repr
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32)
    vals = raw.view(np.float32)
    p = harness_run(harness, "float", stdin="\n".join("%08x" % b for b in raw) + "\n")
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(vals)
    for v, text in zip(vals, lines):
        if np.isnan(v):
            assert text == "nan"
            continue
        assert np.float32(text) == v, (v, text)
        assert not text.endswith(".0") and ("e" in text) == (not (1e-4 <= abs(float(v)) < 1e16)), (v, text)
        digits = lambda t: t.split("e")[0].replace("-", "").replace(".", "").strip("0")  # noqa: E731
        assert len(digits(text)) <= len(digits(np.format_float_scientific(v, unique=True))), (v, text)


def test_color_rounding(harness):
    cases = [(0.5 / 255, None), (0.0, "0"), (1.0, "255"), (0.5, None), (2.0, "510"), (-1.0, "-255")]
    ties = np.array([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 254.5], np.float32) / np.float32(255)
    vals = [c[0] for c in cases] + [float(t) for t in ties] + list(np.random.default_rng(2).random(500).astype(np.float32))
    p = harness_run(harness, "color", stdin=bits(vals))
    lines = p.stdout.split("\n")[:-1]
    assert len(lines) == len(vals)
    for v, text in zip(vals, lines):
        prod = np.float32(255) * np.float32(v)
        assert text == "%.0f" % float(prod), (v, text)
    hit = [float(np.float32(255) * t) for t in ties]
    assert any(h % 1 == 0.5 for h in hit)  # exact .5 products are among the cases: they round to even
    for h, text in zip(hit, lines[len(cases):len(cases) + len(ties)]):
        if h % 1 == 0.5:
            assert int(text) % 2 == 0 and abs(int(text) - h) == 0.5, (h, text)


def test_point_file_reader(harness, tmp_path):
    rng = np.random.default_rng(9)
    pts = rng.normal(0, 3, (257, 3))
    pts[5] = [1e-320, -1e300, 5.0]
    lines = ["%r %r %r 1 %d 2 3" % (float(p[0]), float(p[1]), float(p[2]), k) for k, p in enumerate(pts)]
    lines[7] = "\t%r   %r\t%r" % tuple(float(v) for v in pts[7])  # no trailing fields, other white space
    pcd = ["# .PCD v.7", "VERSION .7", "FIELDS x y z rgb", "SIZE 4 4 4 4", "TYPE F F F F", "COUNT 1 1 1 1", "WIDTH 257",
           "HEIGHT 1", "VIEWPOINT 0 0 0 1 0 0 0", "POINTS 257", "DATA ascii"]

    def read(name, text, chunk=100):
        path = str(tmp_path / name)
        with open(path, "w") as f:
            f.write(text)
        return harness_run(harness, "read", path, str(chunk))

    def points_of(p):
        out = p.stdout.split("\n")
        assert p.returncode == 0 and out[0] == "ok 257", p.stderr[-300:]
        return np.array([[float(v) for v in line.split()] for line in out[1:-1]])

    body = "\n".join(lines)
    for name, text in (("a.xyz", "257\n" + body + "\n"), ("b.txt", "257\n" + body), ("c.xyz", "257\r\n" + body.replace("\n", "\r\n")),
                       ("d.pcd", "\n".join(pcd) + "\n" + body + "\n"), ("e.xyz", "257\n" + body + "\n9 9 9\n")):
        for chunk in (100, 1, 1000):
            if chunk == 1 and name != "a.xyz":
                continue
            assert np.array_equal(points_of(read(name, text, chunk)), pts), (name, chunk)
    # refusals: every one a fatal line and exit status 1
    bad = [("f.xyz", "257\n" + "\n".join(lines[:200]) + "\n", "does not match number of extracted points"),
           ("g.xyz", "x257\n" + body, "First line should contain point count"),
           ("h.xyz", "", "First line should contain point count"),
           ("i.xyz", "257\n" + body.replace(lines[30], "1.0 abc 2.0"), "cannot read x y z of point 30"),
           ("j.pcd", "\n".join(pcd[:2] + ["FIELDS y x z"] + pcd[3:]) + "\n" + body, "FIELDS must start with x y z"),
           ("k.pcd", "\n".join(pcd[:10] + ["DATA binary"]) + "\n" + body, "DATA must be ascii"),
           ("l.pcd", "\n".join(pcd[:9] + ["WIDTH 257", "DATA ascii"]) + "\n" + body, "expected point count in line 10"),
           ("m.pcd", "\n".join(pcd[:9] + ["POINTS 25x7", "DATA ascii"]) + "\n" + body, "Could not parse point count"),
           ("n.pcd", "\n".join(pcd[:6]), "ends inside its 11-line header"),
           ("o.pcd", "\n".join(pcd) + "\n" + "\n".join(lines[:256]), "does not match number of extracted points")]
    for name, text, message in bad:
        p = read(name, text)
        assert p.returncode == 1 and message in p.stderr, (name, p.stderr[-300:])
    p = harness_run(harness, "read", str(tmp_path / "missing.xyz"), "10")
    assert p.returncode == 1 and "File does not exist" in p.stderr
