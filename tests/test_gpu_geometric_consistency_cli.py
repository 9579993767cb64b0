"""bin/GeometricConsistency on one frame of a 4-camera 64^2 dataset: the reference's file list, and PFMs that equal the
C-ABI's arrays (derp_gc_run through the Python binding) byte for byte."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


@pytest.fixture(scope="module")
def dataset(built, tmp_path_factory):
    from facebook360_dep_amd import synth

    root = str(tmp_path_factory.mktemp("gc_dataset"))
    rig = synth.make_rig(4, 64)
    synth.write_dataset(root, rig, [0], [(64, 64)])
    return root, rig["cameras"]


@pytest.mark.parametrize("keep_clean", [False, True])
def test_files_equal_the_api(dataset, tmp_path, keep_clean):
    from facebook360_dep_amd import derp
    from facebook360_dep_amd import imageio as dio
    from tests import geometric_ref as G

    root, cams = dataset
    color = os.path.join(root, "video", "color_levels", "level_0")
    out = str(tmp_path / "out")
    args = [os.path.join(BIN, "GeometricConsistency"), "--rig=" + os.path.join(root, "rigs", "rig_calibrated.json"),
            "--color=" + color, "--output=" + out, "--first=000000", "--last=000000", "--downscale=2", "--disparity_step=0.25",
            "--pass_count=2", "--keep_clean=%s" % ("true" if keep_clean else "false"), "--median=3", "--single=cam1"]
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    names = []
    for cam in cams:
        for stem in ("%s_iffy", "%s_0_clean", "%s_0", "%s_1_clean", "%s_1"):
            names += [stem % cam["id"] + ".pfm", stem % cam["id"] + "_disparity.png"]
    assert sorted(os.listdir(out)) == ["000000"]
    assert sorted(os.listdir(os.path.join(out, "000000"))) == sorted(names)  # (--single is unused: every camera is there)

    g = derp.Derp(cams)
    try:
        images = [dio.load_color_u16(os.path.join(color, cam["id"], "000000.png")) for cam in cams]
        g.gc_upload(images, G.small_sizes(cams, 2))
        g.gc_run(0.25, 0.75, 2, keep_clean)
        finite = 0
        for ci, cam in enumerate(cams):
            for stem, kind, pass_index in (("%s_iffy", "iffy", 0), ("%s_0_clean", "clean", 0), ("%s_0", "depth", 0),
                                           ("%s_1_clean", "clean", 1), ("%s_1", "depth", 1)):
                want = g.gc_result(kind, ci, pass_index)
                path = os.path.join(out, "000000", stem % cam["id"])
                got = dio.read_pfm(path + ".pfm")
                assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), path
                finite += int(np.isfinite(want).sum())
                with np.errstate(divide="ignore", invalid="ignore"):
                    scaled = (np.float32(1) / want) * np.float32(65535)
                png = np.where(np.isnan(scaled), 0, np.clip(np.rint(scaled.astype(np.float64)), 0, 65535)).astype(np.uint16)
                assert np.array_equal(dio.read_png(path + "_disparity.png").reshape(want.shape), png), path
        assert finite > 4000  # of 20 maps of 32 x 32
    finally:
        g.close()
