"""bin/AlignColors on the mixed rig of tests/align_cases.py: two frames, one camera with 8-bit and one with 16-bit PNG
input, --cameras naming a subset. Every output is a 16-bit 3-channel PNG that decodes to exactly the restatement's image
(tests/align_ref.py); only the requested cameras and frames exist; --first / --last narrow the range; a rerun overwrites."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import align_cases as AC
from tests import align_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")
CASE = AC.all_cases()["mixed_rig"]
EIGHT_BIT = "cam1"  # this camera's files are 8-bit: loaded as value * 257


def _input(cam, frame):
    """the image the tool must see for camera `cam` at `frame`, and the array written to its PNG"""
    k = [c["id"] for c in AC.selected(CASE)].index(cam["id"]) if cam in AC.selected(CASE) else None
    if k is None:
        rng = np.random.default_rng([99, frame])
        im = rng.integers(0, 65536, (cam["resolution"][1], cam["resolution"][0], 3), dtype=np.uint16)
    else:
        im = AC.images(CASE, frame)[k]
    if cam["id"] == EIGHT_BIT:
        small = (im >> 8).astype(np.uint8)
        return small.astype(np.uint16) * 257, small
    return im, im


@pytest.fixture(scope="module")
def dataset(built, tmp_path_factory):
    from facebook360_dep_amd import imageio as dio

    root = str(tmp_path_factory.mktemp("align_dataset"))
    for name, cams in (("rig_calibrated", CASE["rig"]), ("rig_red", [CASE["red_ref"]]), ("rig_green", [CASE["green_ref"]]),
                       ("rig_blue", [CASE["blue_ref"]])):
        with open(os.path.join(root, name + ".json"), "w") as f:
            json.dump({"cameras": cams}, f)
    for cam in CASE["rig"]:
        os.makedirs(os.path.join(root, "color", cam["id"]))
        for frame in (0, 1):
            _, stored = _input(cam, frame)
            write = dio.write_png8 if stored.dtype == np.uint8 else dio.write_png16
            write(os.path.join(root, "color", cam["id"], "%06d.png" % frame), stored)
    return root


def _run(root, out, *args):
    cmd = [os.path.join(BIN, "AlignColors"), "--color=" + os.path.join(root, "color"), "--output=" + out] + \
          ["--%s=%s" % (k, os.path.join(root, k + ".json")) for k in ("rig_red", "rig_green", "rig_blue")] + \
          ["--calibrated_rig=" + os.path.join(root, "rig_calibrated.json")] + list(args)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]


def _tree(path):
    return sorted(os.path.relpath(os.path.join(d, f), path) for d, _, files in os.walk(path) for f in files)


def _want(cam, frame):
    seen, _ = _input(cam, frame)
    red, blue = R.maps_of(cam, CASE["red_ref"], CASE["green_ref"], CASE["blue_ref"])
    return R.align(seen, red, blue)


def _check(out, cams, frames):
    from facebook360_dep_amd import imageio as dio

    assert _tree(out) == sorted("%s/%06d.png" % (cam["id"], f) for cam in cams for f in frames)
    for cam in cams:
        for f in frames:
            png = dio.read_png(os.path.join(out, cam["id"], "%06d.png" % f))
            want = _want(cam, f)
            assert png.dtype == np.uint16 and png.shape == want.shape
            bad = int((png != want).sum())
            print("%s frame %d: %d of %d values differ" % (cam["id"], f, bad, want.size))
            assert bad == 0


def test_subset_of_cameras_both_frames_and_a_rerun(dataset, tmp_path):
    out = str(tmp_path / "out")
    cams = AC.selected(CASE)
    assert EIGHT_BIT in [c["id"] for c in cams] and len(cams) == 2
    _run(dataset, out, "--cameras=" + CASE["cameras"])
    _check(out, cams, (0, 1))
    # a rerun over files that are there, one of them damaged: written anew
    with open(os.path.join(out, "cam2", "000001.png"), "wb") as f:
        f.write(b"not a png")
    _run(dataset, out, "--cameras=" + CASE["cameras"], "--threads=2")
    _check(out, cams, (0, 1))


def test_first_and_last_narrow_the_range_and_every_camera_by_default(dataset, tmp_path):
    out = str(tmp_path / "out")
    _run(dataset, out, "--first=000001", "--last=000001")
    _check(out, CASE["rig"], (1,))
    out2 = str(tmp_path / "out2")
    _run(dataset, out2, "--last=000000", "--cameras=cam0")
    _check(out2, [CASE["rig"][0]], (0,))
