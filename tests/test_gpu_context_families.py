"""Every tool family of the C-ABI on ONE context, in turn, forwards and backwards, with the depth pyramid before and
after: each family keeps its device state in a struct of its own that the context creates on the family's first call,
so a family must neither depend on another having run nor disturb one that did.

The library is compared with itself only: every output is bit-equal (np.array_equal over the bytes, so NaNs and signed
zeros count too) to the same call on a fresh context that ran nothing else, and to its own earlier output on the shared
context. No reference data, no tolerance. While the shared context lives, a derp.Isp and a derp.Sim are created, used
once and closed; their outputs equal those made before any context of this test was open."""
import numpy as np
import pytest

from tests import sim_cases

pytestmark = pytest.mark.gpu

FAMILIES = ["depth", "rephoto", "render", "export", "splat", "project", "mesh", "filters"]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _inputs():
    from facebook360_dep_amd import synth

    n, res, widths = synth.config("tiny")  # 4 cameras, 96 x 96, widths 96 / 64 / 48
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    frame = synth.make_frame(rig, sizes)
    rng = np.random.default_rng(11)
    colors = [np.ascontiguousarray(frame["color"][0][s]) for s in range(n)]  # u16 BGR
    disps = [np.ascontiguousarray(frame["truth"][s], dtype=np.float32) for s in range(n)]
    bgra = [np.concatenate([c.astype(np.float32) / 65535.0, np.ones(c.shape[:2] + (1,), np.float32)], axis=2) for c in colors]
    direction = rng.normal(size=(5000, 3))
    xyz = direction / np.linalg.norm(direction, axis=1, keepdims=True) * rng.uniform(1.0, 20.0, size=(5000, 1))
    mask = (rng.uniform(size=(res, res)) > 0.1).astype(np.uint8)
    eqr = (rng.uniform(size=(32, 64)) > 0.5).astype(np.uint8)
    return dict(n=n, res=res, rig=rig, sizes=sizes, frame=frame, colors=colors, disps=disps, bgra=bgra, xyz=xyz, mask=mask, eqr=eqr)


def _run(g, family, X):
    """One family's calls on context g -> the list of everything they return."""
    from facebook360_dep_amd import derp

    n, res = X["n"], X["res"]
    if family == "depth":
        g.upload_frame(X["frame"])
        g.process_pyramid()
        g.synchronize()
        return [g.download_disparity(0, d) for d in range(n)]
    if family == "rephoto":
        g.rephotograph_upload(X["colors"], X["disps"])
        return [g.canopy_cubemap([1] * n, (0.0, 0.0, 0.0), 16)]
    if family == "render":
        g.render_upload(X["disps"], X["bgra"])
        return [g.render(derp.render_params("equirect", height=32, width=64)),
                g.render(derp.render_params("snapshot", width=48, height=32))]
    if family == "export":
        return [g.export_points(0, X["disps"][0], X["bgra"][0][:, :, :3])]
    if family == "splat":
        g.points_begin([(res, res)] * n)
        g.points_splat(X["xyz"][:3000])
        g.points_splat(X["xyz"][3000:])
        return [g.points_download(d) for d in range(n)]
    if family == "project":
        return [g.project_equirect_mask(1, X["eqr"], res, res)]
    if family == "mesh":
        nv, nf, raw = g.mesh_build(0, X["disps"][0])
        out = [np.array([nv, nf, raw])] + list(g.mesh_setup())
        out.append(np.array(g.mesh_simplify_parallel(nf // 4)))
        return out + list(g.mesh_download_f64())
    if family == "filters":
        return [g.masked_median(X["disps"][1], None, X["mask"], 1),
                g.joint_bilateral_u16(X["disps"][1], X["colors"][1], X["mask"], 3, 0.005, 0.5, 1.0, 1.0)]
    raise KeyError(family)


def _context(X):
    from facebook360_dep_amd import derp

    g = derp.Derp(X["rig"]["cameras"], partial_coverage=1)
    g.set_pyramid(X["sizes"], X["res"], X["res"])
    return g


def _isp_and_sim():
    from facebook360_dep_amd import derp

    cfg = {"width": 6, "height": 6}
    raw = np.random.default_rng(5).choice(65536, size=36, replace=False).astype(">u2").tobytes()
    isp = derp.Isp(cfg)
    image = isp.process(raw)
    isp.close()
    sim = derp.Sim()
    tris, nodes, leaf = sim_cases.build_lib("cubes")
    sim.upload(tris, nodes, leaf, sim_cases.skybox())
    bgr, depth = sim.render_camera(dict(sim_cases.CAMERAS["rect_z"], resolution=[32.0, 32.0]))
    sim.close()
    return [image, bgr, depth]


@pytest.fixture(scope="module")
def runs(built):
    X = _inputs()
    alone = _isp_and_sim()  # before any context of this test exists
    fresh = {}
    for family in FAMILIES:  # each on a context of its own that runs nothing else
        g = _context(X)
        fresh[family] = _run(g, family, X)
        g.close()
    g = _context(X)
    first = {family: _run(g, family, X) for family in FAMILIES}
    beside = _isp_and_sim()  # the shared context is alive and every family has state on it
    second = {family: _run(g, family, X) for family in FAMILIES[:0:-1]}
    second["depth"] = _run(g, "depth", X)
    g.close()
    return dict(fresh=fresh, first=first, second=second, alone=alone, beside=beside)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_on_the_shared_context_equals_a_fresh_context(runs, family):
    fresh, first = runs["fresh"][family], runs["first"][family]
    assert len(fresh) == len(first) > 0
    for k, (a, b) in enumerate(zip(fresh, first)):
        assert a.size > 0 and _same(a, b), "%s: output %d differs from a fresh context's" % (family, k)


@pytest.mark.parametrize("family", FAMILIES)
def test_family_repeats_itself_after_the_others_ran(runs, family):
    first, second = runs["first"][family], runs["second"][family]
    assert len(first) == len(second) > 0
    for k, (a, b) in enumerate(zip(first, second)):
        assert _same(a, b), "%s: output %d of the second round differs from the first" % (family, k)


def test_isp_and_sim_beside_a_context(runs):
    for k, (a, b) in enumerate(zip(runs["alone"], runs["beside"])):
        assert a.size > 0 and _same(a, b), "output %d differs with a context open" % k
