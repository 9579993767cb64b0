"""derp_mesh_simplify_parallel (csrc/derp_mesh.h, "the pass-parallel simplifier") on the GPU: bit for bit against its
restatement (tests/mesh_parallel_ref.py) on the restatement's own cases; at 130 x 67 (16 873 faces) the properties of
every result, its quality against the sequential simplifier of the same mesh, and the same bytes from a second run;
the refusals; and bin/ConvertToBinary --simplifier=parallel end to end."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import mesh_parallel_ref as P
from tests import mesh_ref as R
from tests.test_mesh_parallel_ref import check_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "facebook360_dep_amd", "bin", "ConvertToBinary")


@pytest.fixture(scope="module")
def ctx(built):
    from facebook360_dep_amd import derp, synth

    rig = synth.make_rig(2, 64)
    g = derp.Derp(rig["cameras"])
    yield rig["cameras"], g
    g.close()


# the 70 x 37 map first: 4765 faces over 19 blocks, a NaN block, an infinite depth, exact cost ties on its plateaus
@pytest.mark.parametrize("name", ["disparity", "plain", "boundary", "not_equi", "unreachable", "strip", "above"])
def test_bit_for_bit_against_the_restatement(ctx, name):
    cams, g = ctx
    c = P.case(name)
    wv, wf, wstats = c["out"]
    nv, nf, _ = g.mesh_build(0, c["disparity"])
    assert (nv, nf) == (len(c["V"]), len(c["F"]))
    stats = g.mesh_simplify_parallel(c["budget"], remove_boundary_edges=c["rbe"], equi_error=c["equi"])
    nv, nf, _ = g.mesh_counts()
    print("%s: %d -> %d faces, %d vertices, stats %s (restatement: %d faces, %s)"
          % (name, len(c["F"]), nf, nv, stats, len(wf), wstats))
    assert stats == wstats
    assert (nv, nf) == (len(wv), len(wf))
    v, f = g.mesh_download_f64()
    assert np.array_equal(f, wf)
    assert v.tobytes() == wv.tobytes(), int((v != wv).any(axis=1).sum())
    v32, idx = g.mesh_download(clamp_negative_z=True)
    wv32, widx = R.vtx_idx(wv, wf, clamp_negative_z=True)
    assert v32.tobytes() == wv32.tobytes() and idx.tobytes() == widx.tobytes()
    passes = [g.mesh_parallel_pass(k) for k in range(stats[0])]
    assert [p[0] for p in passes] == sorted((p[0] for p in passes), reverse=True)
    if passes:
        assert passes[0][0] == len(c["F"]) and passes[-1][0] - passes[-1][4] == nf
        assert all(0 < p[3] <= p[2] <= p[1] and p[3] <= p[4] <= 2 * p[3] for p in passes)


def test_larger_mesh_properties_quality_and_reproducibility(ctx):
    cams, g = ctx
    disparity = R.gpu_disparity(130, 67)
    _, nf_in, _ = g.mesh_build(1, disparity)
    assert nf_in == 16873
    built_v, built_f = g.mesh_download_f64()
    stats = g.mesh_simplify_parallel(1000)
    v, f = g.mesh_download_f64()
    print("130 x 67: %d -> %d faces, %d vertices after %d passes" % (nf_in, len(f), len(v), stats[0]))
    assert stats[1] == P.EXIT_BUDGET and 1 < stats[0] <= nf_in and 999 <= len(f) <= 1000
    check_mesh(v, f)
    s = P.ParallelSimplifier(built_v, built_f, R.setup(built_v, built_f), True)
    s.adjacency()
    boundary = s.boundary_rule()
    kept = {tuple(p) for p in v.tolist()}
    assert any(boundary) and all(tuple(p) in kept for p, b in zip(built_v.tolist(), boundary) if b)
    # a second run: the same bytes
    g.mesh_build(1, disparity)
    assert g.mesh_simplify_parallel(1000) == stats
    v2, f2 = g.mesh_download_f64()
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    # the sequential simplifier of the same mesh, at the same budget
    g.mesh_build(1, disparity)
    g.mesh_simplify(1000)
    sv, sf = g.mesh_download_f64()
    got, want = P.surface_rms(built_v, v, f), P.surface_rms(built_v, sv, sf)
    print("RMS point-to-surface distance %.6g (parallel) / %.6g (sequential, %d faces) = %.3f" % (got, want, len(sf), got / want))
    assert want > 0 and got <= 1.5 * want


def test_refusals(built):
    from facebook360_dep_amd import derp, synth

    g = derp.Derp(synth.make_rig(2, 64)["cameras"])
    try:
        with pytest.raises(derp.DerpError, match="derp_mesh_build has not been called"):
            g.mesh_simplify_parallel(10)
        assert g.mesh_build(0, np.ones((1, 9), np.float32)) == (0, 0, 0)  # one row: no quads, an empty mesh
        assert g.mesh_simplify_parallel(10) == (0, P.EXIT_BUDGET)
        with pytest.raises(derp.DerpError, match="simplified already"):
            g.mesh_simplify_parallel(10)
        with pytest.raises(derp.DerpError, match="simplified already"):
            g.mesh_simplify(10)
        g.mesh_build(0, R.synthetic_depth(48, 32))
        g.mesh_simplify(2000)
        with pytest.raises(derp.DerpError, match="simplified already"):
            g.mesh_simplify_parallel(10)
        g.mesh_build(0, R.synthetic_depth(48, 32))
        with pytest.raises(derp.DerpError, match="negative face budget"):
            g.mesh_simplify_parallel(-1)
        assert g.mesh_simplify_parallel(2000)[1] == P.EXIT_BUDGET
        with pytest.raises(derp.DerpError, match="simplified already"):
            g.mesh_simplify(10)
    finally:
        g.close()


def test_executable_with_the_parallel_simplifier(built, tmp_path):
    """two cameras at 70 x 37 -> 600 faces each: .vtx / .idx are the restatement's bytes, and --fused indexes them"""
    from facebook360_dep_amd import imageio as dio, synth

    root = str(tmp_path)
    rig = synth.make_rig(2, 64)
    with open(os.path.join(root, "rig.json"), "w") as f:
        json.dump(rig, f)
    maps = {}
    for ci, cam in enumerate(rig["cameras"]):
        os.makedirs(os.path.join(root, "disparity", cam["id"]))
        maps[cam["id"]] = P.case("disparity")["disparity"] * np.float32(1.0 + 0.02 * ci)
        dio.write_pfm(os.path.join(root, "disparity", cam["id"], "000000.pfm"), maps[cam["id"]])
    p = subprocess.run([EXE, "--rig=" + os.path.join(root, "rig.json"), "--disparity=" + os.path.join(root, "disparity"),
                        "--bin=" + os.path.join(root, "bin"), "--fused=" + os.path.join(root, "fused"), "--fuse_strip=2",
                        "--first=000000", "--last=000000", "--output_formats=idx,vtx", "--triangles=600",
                        "--simplifier=parallel"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1500:]
    files = {}
    for ci, cam in enumerate(rig["cameras"]):
        m = R.build(cam, maps[cam["id"]])
        wv, wf, wstats = P.case("disparity")["out"] if ci == 0 else P.simplify(m["V"], m["F"], 600)
        vtx, idx = R.vtx_idx(wv, wf, clamp_negative_z=True)
        d = os.path.join(root, "bin", cam["id"])
        files[cam["id"]] = {ext: open(os.path.join(d, "000000" + ext), "rb").read() for ext in (".idx", ".vtx")}
        assert files[cam["id"]][".vtx"] == vtx.tobytes(), cam["id"]
        assert files[cam["id"]][".idx"] == idx.tobytes(), cam["id"]
        assert "camera %s: %d faces after %d passes" % (cam["id"], len(wf), wstats[0]) in p.stderr
    assert "Iter: 0, faces: 4765, threshold: " in p.stderr and "device simplifier" in p.stderr
    fused = os.path.join(root, "fused")
    disks = R.Fuser(2)
    disks.disks = [bytearray(open(os.path.join(fused, "fused_%d.bin" % i), "rb").read()) for i in range(2)]
    catalog = json.load(open(os.path.join(fused, "fused.json")))
    for cam in rig["cameras"]:
        entry = catalog["frames"]["000000"][cam["id"]]
        for ext in (".idx", ".vtx"):
            assert entry[ext]["size"] == len(files[cam["id"]][ext])
            assert disks.read_back(entry[ext]["offset"], entry[ext]["size"]) == files[cam["id"]][ext]
