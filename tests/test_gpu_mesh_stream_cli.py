"""bin/MeshStreamRenderer end to end on the GPU: a 3-camera synth rig at 96 x 96 converted by bin/ConvertToBinary
(--output_formats=idx,vtx,rgba --triangles=300 --depth_scale=0.25, fused over 2 strips), rendered as cubecolor at edge
32. The exr equals the restatement (tests/stream_ref.py) fed by the Python reader (facebook360_dep_amd/meshstream.py),
every bit; --bin gives the same bytes as --catalog; the png is the exr sRGB-encoded. (The quarter-size depth map keeps
the meshes at a few hundred triangles: the restatement tests every pixel of every face for every triangle.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import stream_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")
RES, EDGE, FRAME = 96, 32, "000002"
POSITION = (0.05, -0.02, 0.03)


def run(exe, *args):
    p = subprocess.run([os.path.join(BIN, exe)] + list(args), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1500:]


@pytest.fixture(scope="module")
def tree(built, tmp_path_factory):
    from facebook360_dep_amd import imageio as dio, synth

    root = str(tmp_path_factory.mktemp("msr"))
    rig = synth.make_rig(3, RES)
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump(rig, f)
    frame = synth.make_frame(rig, [(RES, RES)], device="cpu")
    for ci, cam in enumerate(rig["cameras"]):
        for sub in ("color", "disparity"):
            os.makedirs(os.path.join(root, sub, cam["id"]))
        dio.write_pfm(os.path.join(root, "disparity", cam["id"], FRAME + ".pfm"), frame["truth"][ci])
        dio.write_png8(os.path.join(root, "color", cam["id"], FRAME + ".png"), (frame["color"][0][ci] >> 8).astype(np.uint8))
    run("ConvertToBinary", "--rig=" + os.path.join(root, "rig.json"), "--color=" + os.path.join(root, "color"),
        "--disparity=" + os.path.join(root, "disparity"), "--bin=" + os.path.join(root, "bin"),
        "--fused=" + os.path.join(root, "fused"), "--fuse_strip=2", "--first=" + FRAME, "--last=" + FRAME,
        "--output_formats=idx,vtx,rgba", "--triangles=300", "--depth_scale=0.25")
    return root


def render(root, out, file_type, *source):
    run("MeshStreamRenderer", "--rig=" + os.path.join(root, "fused", "rig_fused.json"), "--output=" + os.path.join(root, out),
        "--first=" + FRAME, "--last=" + FRAME, "--format=cubecolor", "--height=%d" % EDGE, "--file_type=" + file_type,
        "--position=%g %g %g" % POSITION, *source)
    return os.path.join(root, out, FRAME + "." + file_type)


def test_stream_to_picture(tree):
    from facebook360_dep_amd import derp, imageio as dio, meshstream

    root = tree
    fused = os.path.join(root, "fused")
    catalog = ["--catalog=" + os.path.join(fused, "fused.json"),
               "--strip_files=" + ",".join(os.path.join(fused, "fused_%d.bin" % i) for i in range(2))]
    exr = render(root, "from_catalog", "exr", *catalog)
    got = dio.read_exr(exr)
    assert got.shape == (6 * EDGE, EDGE, 3)
    # the restatement, fed by the Python reader
    cams = json.load(open(os.path.join(fused, "rig_fused.json")))["cameras"]
    assert [c["resolution"] for c in cams] == [[float(RES)] * 2] * 3
    stream = meshstream.MeshStream(os.path.join(fused, "fused.json"), [os.path.join(fused, "fused_%d.bin" % i) for i in range(2)])
    scene = []
    for cam in cams:
        vtx, idx, rgba = stream.mesh(FRAME, cam["id"], (RES, RES))
        assert 50 < len(idx) // 3 < 2 * 23 * 23  # simplified from the quarter-size depth map
        scene.append(dict(cam=cam, vtx=vtx, idx=idx, rgba=rgba))
        assert meshstream.bin_mesh(os.path.join(root, "bin"), FRAME, cam["id"], (RES, RES))[0].tobytes() == vtx.tobytes()
    table = derp.stream_srgb_table()
    want = R.render(scene, table, kind="cube", height=EDGE, position=POSITION)
    assert R.same(got, want[..., :3]) == 0
    covered = ~np.isnan(want[..., 3])
    assert 0.3 < covered.mean() < 1.0  # three cameras on an arc see part of the sphere
    # --bin gives the same bytes
    assert open(render(root, "from_bin", "exr", "--bin=" + os.path.join(root, "bin")), "rb").read() == open(exr, "rb").read()
    # the png is the exr, sRGB-encoded; alpha marks what was rendered
    png = dio.read_png(render(root, "png", "png", *catalog))  # B G R A
    assert png.dtype == np.uint8 and png.shape == (6 * EDGE, EDGE, 4)
    assert np.array_equal(png[..., :3], meshstream.srgb_encode(got, table))
    assert np.array_equal(png[..., 3], np.where(covered, 255, 0))
