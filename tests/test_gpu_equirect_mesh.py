"""derp_mesh_build_equirect (csrc/derp_mesh.h: k_mesh_vertices_equirect, k_mesh_quads fed the norms, k_mesh_seam_faces,
the seam in k_mesh_vertex_quadrics), the set-up and both simplifiers on the wrapped mesh, and
bin/CreateObjFromDisparityEquirect, against the restatement in tests/equirect_mesh_ref.py (MeshUtil.h) with
tests/mesh_ref.py's set-up and simplifier: everything bit for bit, no tolerance anywhere. Sizes: 2 x 2 (the smallest
accepted: the seam quad and the only grid quad share all four vertices), 3 x 2, 8 x 4, and 67 x 33 (odd both ways, 2211
pixels: the block scan crosses nine blocks and the seam faces land after a non-trivial offset); the tool at 70 x 37."""
import os
import subprocess

import numpy as np
import pytest

from tests import equirect_mesh_ref as E
from tests import mesh_parallel_ref as P
from tests import mesh_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "facebook360_dep_amd", "bin", "CreateObjFromDisparityEquirect")
SIZES = [(2, 2), (3, 2), (8, 4), (67, 33)]
ALL_OUTCOMES = (1 << 1 | 1 << 2, 1 << 0 | 1 << 3, 1, 2, 4, 8, 0)
_cache = {}


def want_build(w, h):
    if ("build", w, h) not in _cache:
        _cache[("build", w, h)] = E.build(E.sample_disparity(w, h))
    return _cache[("build", w, h)]


def want_setup(w, h):
    if ("setup", w, h) not in _cache:
        m = want_build(w, h)
        _cache[("setup", w, h)] = R.setup(m["V"], m["F"], equi_error=False)
    return _cache[("setup", w, h)]


@pytest.fixture(scope="module")
def ctx(built):
    from facebook360_dep_amd import derp, synth

    cams = synth.make_rig(2, 64)["cameras"]
    g = derp.Derp(cams)
    yield cams, g
    g.close()


def test_inputs_reach_every_triangle_mask_outcome():
    m = want_build(67, 33)
    print("outcomes of the 67 x 33 map: %s" % sorted(m["outcomes"].items()))
    for outcome in ALL_OUTCOMES:
        assert m["outcomes"].get(outcome, 0) > 0, outcome
    whole = {1 << 1 | 1 << 2, 1 << 0 | 1 << 3}
    for w, h in ((8, 4), (67, 33)):
        m, disp = want_build(w, h), E.sample_disparity(w, h)
        for column in (0, w - 2):  # the quads next to the seam: some whole, some torn
            assert m["by_column"][column] & whole and m["by_column"][column] - whole, (w, h, column)
        assert (disp == 0).any() and np.isnan(disp).any() and (disp < 0).any()
        assert np.isfinite(m["V"]).all() and (m["norms"].astype(np.float32) == 700).sum() >= 2  # the zero and the NaN
    assert want_build(2, 2)["grid"] == 2 and len(want_build(2, 2)["F"]) == 4
    assert len(want_build(67, 33)["F"]) > 8 * 256  # the face offsets of the last blocks come from the scan


@pytest.mark.parametrize("w,h", SIZES)
def test_build_bit_for_bit(ctx, w, h):
    _, g = ctx
    want = want_build(w, h)
    nv, nf, raw = g.mesh_build_equirect(E.sample_disparity(w, h))
    print("%d x %d: %d vertices, %d faces, %d of them grid faces" % (w, h, nv, nf, want["grid"]))
    assert (nv, nf, raw) == (w * h, len(want["F"]), len(want["F"]))
    v, f = g.mesh_download_f64()
    assert v.tobytes() == want["V"].tobytes(), int((v != want["V"]).sum())
    assert f.dtype == np.int32 and np.array_equal(f[:want["grid"]], want["F"][:want["grid"]])
    assert np.array_equal(f[want["grid"]:], want["F"][want["grid"]:])  # the seam


def test_max_depth_and_tear_ratio_reach_the_kernels(ctx):
    _, g = ctx
    disp = E.sample_disparity(67, 33)
    want = E.build(disp, max_depth=3.125, tear_ratio=0.999)
    assert want["grid"] < want_build(67, 33)["grid"]
    nv, nf, _ = g.mesh_build_equirect(disp, max_depth=3.125, tear_ratio=0.999)
    v, f = g.mesh_download_f64()
    assert nf == len(want["F"]) and v.tobytes() == want["V"].tobytes() and np.array_equal(f, want["F"])


@pytest.mark.parametrize("w,h", [(8, 4), (67, 33)])
def test_setup_bit_for_bit(ctx, w, h):
    _, g = ctx
    g.mesh_build_equirect(E.sample_disparity(w, h))
    got = g.mesh_setup(equi_error=False)
    ref = want_setup(w, h)
    planes, costs, vq = got
    assert planes.tobytes() == ref[0].tobytes(), "face planes"
    column = np.arange(w * h) % w
    inner = (column != 0) & (column != w - 1)
    assert vq[inner].tobytes() == ref[2][inner].tobytes(), "vertex quadrics away from the seam"
    assert vq[column == 0].tobytes() == ref[2][column == 0].tobytes(), "vertex quadrics of column 0: the seam"
    assert vq[column == w - 1].tobytes() == ref[2][column == w - 1].tobytes(), "vertex quadrics of column w - 1: the seam"
    assert costs.shape == ref[1].shape and costs.tobytes() == ref[1].tobytes(), ("edge costs", int((costs != ref[1]).sum()))


@pytest.mark.parametrize("host_setup", [False, True])
def test_sequential_simplify_bit_for_bit(ctx, host_setup):
    _, g = ctx
    if "seq" not in _cache:
        m = want_build(67, 33)
        _cache["seq"] = R.simplify(m["V"], m["F"], 600, 0.8, False, equi_error=False)
    wv, wf, wstats = _cache["seq"]
    g.mesh_build_equirect(E.sample_disparity(67, 33))
    stats = g.mesh_simplify(600, strictness=0.8, equi_error=False, host_setup=host_setup)
    nv, nf, _ = g.mesh_counts()
    print("67 x 33 -> %d faces, %d vertices after %d passes (set-up on the %s)" % (nf, nv, stats[0], "host" if host_setup else "device"))
    assert stats == wstats and nf <= 600 and (nv, nf) == (len(wv), len(wf))
    v, f = g.mesh_download_f64()
    assert np.array_equal(f, wf) and v.tobytes() == wv.tobytes()


def test_parallel_simplify_bit_for_bit(ctx):
    """Bit for bit against tests/mesh_parallel_ref.py: that restatement takes a plain (V, F) and reads nothing of the
    grid, so the properties test_larger_mesh_properties_quality_and_reproducibility falls back on are not needed here
    (face target, indices in range and no degenerate face are asserted all the same)."""
    _, g = ctx
    m = want_build(67, 33)
    wv, wf, wstats = P.simplify(m["V"], m["F"], 600, 0.2, False, False)
    g.mesh_build_equirect(E.sample_disparity(67, 33))
    stats = g.mesh_simplify_parallel(600, strictness=0.2, equi_error=False)
    nv, nf, _ = g.mesh_counts()
    print("67 x 33 -> %d faces, %d vertices after %d passes of the parallel simplifier" % (nf, nv, stats[0]))
    assert stats == wstats and stats[1] == P.EXIT_BUDGET and nf <= 600
    v, f = g.mesh_download_f64()
    assert np.array_equal(f, wf) and v.tobytes() == wv.tobytes()
    assert f.min() >= 0 and f.max() < nv
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])).all()


def test_refusals(built):
    from facebook360_dep_amd import derp, synth

    g = derp.Derp(synth.make_rig(2, 64)["cameras"])
    try:
        with pytest.raises(derp.DerpError, match="derp_mesh_build has not been called"):
            g.mesh_setup()
        with pytest.raises(derp.DerpError, match="1 x 5 equirect"):
            g.mesh_build_equirect(np.ones((5, 1), np.float32))
        with pytest.raises(derp.DerpError, match="5 x 1 equirect"):
            g.mesh_build_equirect(np.ones((1, 5), np.float32))
        with pytest.raises(derp.DerpError, match="tear_ratio is NaN"):
            g.mesh_build_equirect(np.ones((4, 4), np.float32), tear_ratio=float("nan"))
        with pytest.raises(derp.DerpError, match="max_depth is NaN"):
            g.mesh_build_equirect(np.ones((4, 4), np.float32), max_depth=float("nan"))
        with pytest.raises(derp.DerpError, match="derp_mesh_build has not been called"):
            g.mesh_setup()  # a refused build is no build
    finally:
        g.close()


def test_camera_and_equirect_meshes_share_a_context(ctx):
    """the two builds share the context's buffers: each leaves its own mesh and its own set-up, whichever came before"""
    cams, g = ctx
    disp = R.gpu_disparity(70, 37)
    cam = R.build(cams[0], disp)
    cam_setup = R.setup(cam["V"], cam["F"], equi_error=True)
    eqr, eqr_setup = want_build(67, 33), want_setup(67, 33)

    def check_camera():
        assert g.mesh_build(0, disp) == (len(cam["V"]), len(cam["F"]), cam["unmasked"])
        v, f = g.mesh_download_f64()
        assert v.tobytes() == cam["V"].tobytes() and np.array_equal(f, cam["F"])
        for a, b in zip(g.mesh_setup(equi_error=True), cam_setup):
            assert a.tobytes() == b.tobytes()

    def check_equirect():
        g.mesh_build_equirect(E.sample_disparity(67, 33))
        v, f = g.mesh_download_f64()
        assert v.tobytes() == eqr["V"].tobytes() and np.array_equal(f, eqr["F"])
        for a, b in zip(g.mesh_setup(equi_error=False), eqr_setup):
            assert a.tobytes() == b.tobytes()

    check_equirect()
    check_camera()
    check_equirect()


# ---------------------------------------------------------------- the executable, 70 x 37
@pytest.fixture(scope="module")
def tool_inputs(built, tmp_path_factory):
    from facebook360_dep_amd import imageio as dio

    root = str(tmp_path_factory.mktemp("create_obj"))
    os.makedirs(os.path.join(root, "equirects"))
    os.makedirs(os.path.join(root, "meshes"))
    disp = np.nan_to_num(R.gpu_disparity(70, 37), nan=0.0)
    img = np.rint(np.clip(disp, 0, 1).astype(np.float64) * 65535).astype(np.uint16)  # a 16-bit PNG holds [0, 1]
    dio.write_png16(os.path.join(root, "equirects", "disp.png"), img)
    dio.write_png8(os.path.join(root, "equirects", "color.png"), np.full((37, 70, 3), 90, np.uint8))
    return root, E.load_float(img)


def run_tool(root, name, *args):
    out = os.path.join(root, "meshes", name + ".obj")
    p = subprocess.run([EXE, "--input_png_disp=" + os.path.join(root, "equirects", "disp.png"),
                        "--input_png_color=" + os.path.join(root, "equirects", "color.png"), "--output_obj=" + out] + list(args),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-800:]
    return out, open(out).read()


def test_tool_unsimplified_with_material(tool_inputs):
    root, disp = tool_inputs
    m = E.build(disp)
    assert (disp == 0).any()
    out, text = run_tool(root, "plain", "--strictness=0")
    assert text == E.obj_text(m["V"], m["F"])
    assert not os.path.exists(os.path.join(root, "meshes", "plain.mtl"))
    out, text = run_tool(root, "textured", "--strictness=0", "--create_mtl")
    mtl, name = E.mtl_text(out, os.path.join(root, "equirects", "color.png"))
    assert name == "textured.mtl" and open(os.path.join(root, "meshes", name)).read() == mtl
    assert mtl.splitlines() == ["newmtl material", "illum 0", "Kd 1 1 1", "map_Kd ../equirects/color.png"]
    assert text == E.obj_text(m["V"], m["F"], E.texcoords(m["V"]), name)
    assert text.startswith("mtllib textured.mtl\nusemtl material\nv ") and text.count("\nvt ") == 70 * 37


def test_tool_simplified(tool_inputs):
    root, disp = tool_inputs
    m = E.build(disp)
    wv, wf, _ = R.simplify(m["V"], m["F"], 600, 0.8, False, equi_error=False)
    _, text = run_tool(root, "simplified", "--strictness=0.8", "--num_faces=600")
    assert text == E.obj_text(wv, wf) and len(wf) <= 600


def test_tool_scaled(tool_inputs):
    root, disp = tool_inputs
    m = E.build(E.resize_bilinear(disp, 0.5))
    assert (m["w"], m["h"]) == (35, 18)
    _, text = run_tool(root, "scaled", "--strictness=0", "--scale=0.5", "--max_depth=20", "--tear_ratio=0.9")
    want = E.build(E.resize_bilinear(disp, 0.5), max_depth=20.0, tear_ratio=0.9)
    assert text == E.obj_text(want["V"], want["F"])


def test_tool_parallel_simplifier(tool_inputs):
    root, _ = tool_inputs
    _, text = run_tool(root, "parallel", "--strictness=0.2", "--num_faces=600", "--simplifier=parallel")
    faces = [line for line in text.splitlines() if line.startswith("f ")]
    vertices = [line for line in text.splitlines() if line.startswith("v ")]
    assert 0 < len(faces) <= 600 and len(vertices) < 70 * 37
    assert all(1 <= int(i) <= len(vertices) for line in faces for i in line.split()[1:])
