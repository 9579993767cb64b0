"""bin/RigAnalyzer on the GPU: the sweep report on stdout, the three PGM maps and the log's statistics lines equal the
restatement's text (tests/coverage_ref.py) byte for byte."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import coverage_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "facebook360_dep_amd", "bin", "RigAnalyzer")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from facebook360_dep_amd import synth

    root = str(tmp_path_factory.mktemp("rig_analyzer_gpu"))
    with open(os.path.join(root, "rig4.json"), "w") as f:
        json.dump(synth.make_rig(4, 64), f)
    return root


def run(tree, args):
    p = subprocess.run([TOOL, "--rig=" + os.path.join(tree, "rig4.json")] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p


def logged(p):
    """the messages of the log's lines, without glog's prefixes"""
    return [line.split("] ", 1)[1] for line in p.stderr.split("\n") if "] " in line]


def read(path):
    with open(path) as f:
        return f.read()


def test_default_shaped_run(tree):
    from facebook360_dep_amd import synth

    out = {k: os.path.join(tree, k + ".pgm") for k in ("equirect", "camera", "cross")}
    p = run(tree, ["--sample_count=1000", "--output_equirect=" + out["equirect"], "--output_camera=" + out["camera"],
                   "--output_camera_id=cam1", "--output_cross_section=" + out["cross"]])
    ref = R.Coverage(synth.make_rig(4, 64)["cameras"])
    units, distances = R.fibonacci_units(1000), R.coverage_distances(0.5)
    assert p.stdout == R.report(ref.directions(units, distances)[0], distances, 1000)
    assert p.stdout.count("\n") == 20 and p.stdout.startswith("distance: 0.50 quality: ")
    counts, _, stats = ref.equirect(5, 1e4)
    assert counts.shape == (900, 1800) and read(out["equirect"]) == R.pgm(counts, 4)
    assert [m for m in logged(p) if "Holes found" in m or "timing distance" in m] == R.stats_lines(stats, 1800, 900)
    assert read(out["camera"]) == R.pgm(ref.camera(1, 1e4)[0], 4)
    assert read(out["cross"]) == R.pgm(ref.cross_section(400), 4)


def test_show_timing(tree):
    from facebook360_dep_amd import synth

    path = os.path.join(tree, "timed.pgm")
    p = run(tree, ["--sample_count=0", "--show_timing", "--overlap_distance=0.75", "--output_equirect=" + path])
    assert p.stdout == ""
    _, timing, stats = R.Coverage(synth.make_rig(4, 64)["cameras"]).equirect(5, 0.75)
    values = R.timed_values(timing)
    assert read(path) == R.pgm(values, 256) and 0 == values.min() < values.max() <= 255
    assert [m for m in logged(p) if "Holes found" in m or "timing distance" in m] == R.stats_lines(stats, 1800, 900)


def test_rearranged_rig_loads_back(tree):
    from facebook360_dep_amd import derp, synth

    path = os.path.join(tree, "ballcam24.json")
    p = run(tree, ["--rearrange=ballcam24", "--scale_resolution=0.5", "--sample_count=257", "--discard_poles=10",
                   "--min_distance=0.2", "--output_rig=" + path])
    want = R.rig_scale(R.rig_arrangement("ballcam24", synth.make_rig(4, 64)["cameras"][0]), scale_resolution=0.5)
    cams = json.loads(read(path))["cameras"]
    assert len(cams) == 24 and all(R.same_camera(g, w) for g, w in zip(cams, want)) and cams[5]["resolution"] == [32.0, 32.0]
    ref = R.Coverage(want)
    units, distances = R.fibonacci_units(257, 10.0), R.coverage_distances(0.2)
    assert 0 < len(units) < 257 and p.stdout == R.report(ref.directions(units, distances)[0], distances, len(units))
    g = derp.Derp(cams)  # what the tool wrote is a rig the library takes
    try:
        hist, counts = g.coverage_directions(units, distances)
        want_hist, want_counts = ref.directions(units, distances)
        assert np.array_equal(hist, want_hist) and np.array_equal(counts, want_counts)
    finally:
        g.close()
