"""The mesh-stream renderer (derp_stream_*, facebook360_dep_amd/csrc/derp_stream.h) through the C ABI against
tests/stream_ref.py: bit for bit, NaN positions included, no tolerance. Rig synth.make_rig(3, 64); hand-made
.vtx / .idx / .rgba arrays; views 64 x 48 unless the case is about the size.

What the picture cannot show is shown by construction: two triangles at the same positions are told apart by texVar
beyond the resolution (the direction lookup clamps, the colour lookup reads another row), so "the lower index wins" changes
the image. Three of the issue's cases cannot be stated through the C ABI and are stated where they can be:
- texVar exactly at the image centre (cone 1) cannot be hit by an interpolated fragment; tests/test_stream_ref.py pins
  that value (test_fragment_cone_and_quantiser), here the fragments around the centre and beyond radius 0.5 are compared.
- A shared edge exactly through pixel centres of the view needs clip coordinates chosen by hand, and the ABI takes abc,
  which reach the view through the direction table and the transform; tests/test_stream_ref.py owns every such centre
  once on the clip coordinates themselves, here the two triangles' coverage is shown to add up with no gap or overlap.
- "Nothing is launched" by a refused upload is not observable from outside the library; the refusals sit before the
  first HIP call of derp_stream_upload (read there), and here the return code, the message and the unchanged scene are
  asserted."""
import numpy as np
import pytest

from tests import stream_ref as R

pytestmark = pytest.mark.gpu

RES = 64
FOCAL = 0.36 * RES
FLT_MIN = np.float32(1.17549435e-38)
VIEW = dict(kind="snapshot", width=64, height=48, position=(0.0, 0.0, 0.0), forward=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fov=90.0)


def c_of(depth):
    """abc.z of a vertex `depth` metres along its ray"""
    return FOCAL / depth


def texture(seed):
    return np.random.default_rng(seed).integers(0, 256, size=(RES, RES, 4), dtype=np.uint8)


def item(rig, s, vtx, idx, seed=None):
    return dict(cam=rig["cameras"][s], vtx=np.array(vtx, dtype=np.float32).reshape(-1, 3),
                idx=np.array(idx, dtype=np.uint32).reshape(-1), rgba=texture(s if seed is None else seed))


def grid(n, depth, lo=4.0, hi=60.0):
    """an n x n vertex grid over the image square [lo, hi]^2 with depth(x, y) metres, two triangles per cell"""
    t = np.linspace(lo, hi, n)
    vtx = [(x, y, c_of(depth(x, y))) for y in t for x in t]
    idx = []
    for j in range(n - 1):
        for i in range(n - 1):
            b = j * n + i
            idx += [b, b + 1, b + n, b + 1, b + n + 1, b + n]
    return vtx, idx


@pytest.fixture(scope="module")
def ctx(built):
    from facebook360_dep_amd import derp, synth

    rig = synth.make_rig(3, RES)
    g = derp.Derp(rig["cameras"])
    yield dict(g=g, rig=rig, table=derp.stream_srgb_table(), dirs=[R.direction_table(c) for c in rig["cameras"]])
    g.close()


def upload(ctx, scene):
    ctx["g"].stream_clear()
    for s, it in enumerate(scene):
        if it is not None:
            it["dirs"] = ctx["dirs"][s]
            ctx["g"].stream_upload(s, it["vtx"], it["idx"], it["rgba"])


def check(ctx, scene, include=None, fade=1.0, zero_nans=False, **view):
    """GPU == restatement, every bit; -> the restatement's image"""
    from facebook360_dep_amd import derp

    v = dict(VIEW, **view)
    p = derp.render_params(v["kind"], width=v["width"], height=v["height"], position=v["position"], forward=v["forward"],
                           up=v["up"], horizontal_fov=v["fov"], zero_nans=zero_nans)
    got = ctx["g"].stream_render(p, include=include, fade=fade)
    want = R.render(scene, ctx["table"], include=include, fade=fade, zero_nans=zero_nans, **v)
    assert R.same(got, want) == 0, "%d of %d values differ" % (R.same(got, want), want.size)
    return want


def covered(img):
    return int((~np.isnan(img[..., 3])).sum())


def standard(rig):
    """three overlapping cameras, each a 6 x 6 grid with its own relief"""
    return [item(rig, s, *grid(6, lambda x, y, s=s: 1.5 + 0.4 * s + 0.01 * x + 0.3 * np.sin(0.2 * y))) for s in range(3)]


def test_vertex_stage(ctx):
    """abc.xy at 0 and at the resolution (the table's edge texels) and beyond, abc.z = FLT_MIN (a non-finite position), a
    tiny positive z (a finite, enormous one): clip coordinates for a snapshot and for a cube face"""
    from facebook360_dep_amd import derp

    rig = ctx["rig"]
    xy = [0.0, 0.25, 13.7, 32.0, 63.999, 64.0, 70.0, -3.0]
    z = [FLT_MIN, 1e-30, 0.37, 5.0, c_of(2.0), 400.0]
    vtx = np.array([(a, b, c) for a in xy for b in xy for c in z], dtype=np.float32)
    for cam in (0, 2):
        upload(ctx, [item(rig, s, vtx, []) if s == cam else None for s in range(3)])
        views = [(derp.render_params("snapshot", width=64, height=48, position=(0.1, -0.2, 0.05), forward=(1, 0.2, -0.1),
                                     horizontal_fov=70.0), R.view("snapshot", 64, 48, (0.1, -0.2, 0.05), (1, 0.2, -0.1), (0, 0, 1), 70.0), 0),
                 (derp.render_params("cube", height=24, position=(0.1, -0.2, 0.05)), R.view("cube", 0, 24, (0.1, -0.2, 0.05), face=3), 3)]
        for p, v, face in views:
            got = ctx["g"].stream_vertices(cam, len(vtx), p, face)
            want, _ = R.vertex_stage(rig["cameras"][cam], ctx["dirs"][cam], vtx, R.transform(v))
            assert R.same(got, want) == 0
            assert np.isfinite(want).all(axis=1).sum() > len(vtx) // 2 and (~np.isfinite(want)).any()


def test_three_cameras_accumulate(ctx):
    """two and three overlapping cameras in rig order, weights up to exp(30) - 1; a camera switched off by include; fade;
    zero_nans; two renders of one scene are the same bits"""
    scene = standard(ctx["rig"])
    upload(ctx, scene)
    full = check(ctx, scene)
    assert covered(full) > 1500
    for include in ([1, 1, 0], [0, 1, 0], [1, 0, 1]):
        part = check(ctx, scene, include=include)
        assert R.same(part, full) > 0
    faded = check(ctx, scene, fade=0.25)
    assert R.same(faded, full) > 0
    zeroed = check(ctx, scene, zero_nans=True, forward=(0.3, 0.0, 1.0))
    assert not np.isnan(zeroed).any() and (zeroed[..., 3] == 0).any()
    again = check(ctx, scene)
    assert R.same(again, full) == 0


@pytest.mark.parametrize("width,height", [(1, 1), (63, 47), (130, 3)])
def test_view_sizes(ctx, width, height):
    scene = standard(ctx["rig"])
    upload(ctx, scene)
    assert covered(check(ctx, scene, width=width, height=height)) > 0


def test_cube_and_equirect(ctx):
    scene = standard(ctx["rig"])
    upload(ctx, scene)
    cube = check(ctx, scene, kind="cube", height=24, position=(0.05, 0.02, -0.03))
    assert cube.shape == (144, 24, 4) and covered(cube) > 300
    eqr = check(ctx, scene, kind="equirect", height=24, position=(0.05, 0.02, -0.03))
    assert eqr.shape == (24, 48, 4) and covered(eqr) > 100


def test_one_triangle_beyond_the_view(ctx):
    """two triangles spanning +-67 degrees of camera 1 seen through a 40-degree view: every pixel is covered, by parts
    of triangles whose vertices lie far outside the view. Then a triangle at the image's left border with texVar.x from
    -0.06 to 0.09: the direction and colour lookups clamp to the border texels, the cone is at its floor 1 / 255."""
    rig = ctx["rig"]
    scene = [None, item(rig, 1, [(8, 32, c_of(2)), (32, 8, c_of(2)), (56, 32, c_of(3)), (32, 56, c_of(2))], [0, 1, 2, 0, 2, 3]), None]
    upload(ctx, scene)
    assert covered(check(ctx, scene, fov=40.0, position=(0.25, 0.0, 0.0))) == 64 * 48
    border = [None, item(rig, 1, [(-4, 26, c_of(2)), (-4, 38, c_of(2)), (6, 32, c_of(2.5))], [0, 1, 2]), None]
    upload(ctx, border)
    assert covered(check(ctx, border, fov=30.0, forward=(0.1, 1.0, 0.0))) > 50


def test_sliver_and_degenerate_triples(ctx):
    """a sliver that covers no centre renders nothing; index triples with two equal indices are skipped"""
    rig = ctx["rig"]
    vtx = [(30.0, 30.0, c_of(2)), (30.004, 30.0, c_of(2)), (30.0, 30.004, c_of(2)), (10, 10, c_of(2)), (50, 12, c_of(2)), (30, 50, c_of(2))]
    sliver = [None, item(rig, 1, vtx, [0, 1, 2]), None]
    upload(ctx, sliver)
    assert covered(check(ctx, sliver)) == 0
    both = [None, item(rig, 1, vtx, [3, 3, 4, 3, 4, 4, 5, 4, 5, 0, 1, 2, 3, 4, 5, 4, 4, 4]), None]
    upload(ctx, both)
    only = [None, item(rig, 1, vtx, [3, 4, 5]), None]
    assert R.same(check(ctx, both), R.render(only, ctx["table"], **VIEW)) == 0 and covered(check(ctx, both)) > 50


def test_shared_edge_and_depth_order(ctx):
    """two triangles sharing an edge; coplanar duplicates (the lower index wins); a nearer triangle later in the buffer"""
    rig = ctx["rig"]
    c = c_of(2.0)
    quad = [(16, 16, c), (48, 16, c), (48, 48, c), (16, 48, c)]
    shared = [None, item(rig, 1, quad, [0, 1, 2, 0, 2, 3]), None]
    upload(ctx, shared)
    whole = check(ctx, shared)
    parts = [covered(R.render([None, item(rig, 1, quad, tri), None], ctx["table"], **VIEW)) for tri in ([0, 1, 2], [0, 2, 3])]
    assert covered(whole) == sum(parts) > 200  # no gap, no overlap
    # the same positions twice: b = 64 and b = 80 give one direction (clamped lookup) and different texVar
    vtx = [(26, 64, c), (38, 64, c), (32, 30, c), (26, 80, c), (38, 80, c)]
    wide = dict(fov=120.0)
    first, second = [0, 1, 2], [3, 4, 2]
    images = []
    for idx in (first + second, second + first):
        scene = [None, item(rig, 1, vtx, idx), None]
        upload(ctx, scene)
        images.append(check(ctx, scene, **wide))
        alone = R.render([None, item(rig, 1, vtx, idx[:3]), None], ctx["table"], **dict(VIEW, **wide))
        assert R.same(images[-1], alone) == 0  # the first of the two is what is seen
    assert R.same(images[0], images[1]) > 0
    # a nearer triangle later in the buffer wins where they overlap
    vtx = [(16, 16, c_of(3)), (48, 16, c_of(3)), (30, 48, c_of(3)), (22, 22, c_of(1)), (50, 30, c_of(1)), (26, 50, c_of(1))]
    scene = [None, item(rig, 1, vtx, [0, 1, 2, 3, 4, 5]), None]
    upload(ctx, scene)
    far_only = R.render([None, item(rig, 1, vtx, [0, 1, 2]), None], ctx["table"], **VIEW)
    assert R.same(check(ctx, scene), far_only) > 0
    swapped = [None, item(rig, 1, vtx, [3, 4, 5, 0, 1, 2]), None]
    upload(ctx, swapped)
    assert R.same(check(ctx, swapped), check(ctx, scene)) == 0  # whichever comes first in the buffer


def test_triangles_behind_the_eye(ctx):
    """one vertex, two vertices and all three behind the eye: the part in front is rendered, not dropped"""
    rig = ctx["rig"]
    cam = rig["cameras"][1]
    vtx = np.array([(14, 14, c_of(1.0)), (52, 16, c_of(1.2)), (30, 54, c_of(0.9))], dtype=np.float32)
    scene = [None, item(rig, 1, vtx, [0, 1, 2]), None]
    upload(ctx, scene)
    seen = {}
    for name, view in (("one", dict(position=(0.55, 0.5, 0.0), forward=(0.3, -1.0, 0.2))),
                       ("two", dict(position=(0.56, 0.03, 0.54), forward=(1.08, -0.3, 2.11))),
                       ("all", dict(position=(3.0, 0.0, 0.0), forward=(1.0, 0.0, 0.0)))):
        v = dict(VIEW, **view)
        clip, _ = R.vertex_stage(cam, ctx["dirs"][1], vtx, R.transform(R.view(**v)))
        seen[name] = (int((clip[:, 3] < 0.1).sum()), covered(check(ctx, scene, **view)))
    assert seen["one"][0] == 1 and seen["one"][1] > 0, seen
    assert seen["two"][0] == 2 and seen["two"][1] > 0, seen
    assert seen["all"] == (3, 0), seen


def test_a_vertex_kilometres_away_and_one_behind_the_eye(ctx):
    """a triangle with one vertex 20 km away, cut by the near plane, in both index orders: the box the triangle is
    rasterised in comes from the crossing points of edges that reach that vertex; the picture is the restatement's, the
    same for both orders, and nothing the edge functions cover anywhere in the view is left out of the box"""
    rig = ctx["rig"]
    cam = rig["cameras"][1]
    vtx = np.array([(14, 14, c_of(1.0)), (52, 16, c_of(20000.0)), (30, 54, c_of(0.9))], dtype=np.float32)
    seen = []
    for view in (dict(position=(0.55, 0.5, 0.0), forward=(0.3, -1.0, 0.2)), dict(position=(0.56, 0.03, 0.54), forward=(1.08, -0.3, 2.11)),
                 dict(position=(0.3, 0.0, 0.0), forward=(0.0, 1.0, 0.0), width=130, height=96)):
        v = dict(VIEW, **view)
        clip, _ = R.vertex_stage(cam, ctx["dirs"][1], vtx, R.transform(R.view(**v)))
        images = []
        for idx in ([0, 1, 2], [1, 0, 2]):
            scene = [None, item(rig, 1, vtx, idx), None]
            upload(ctx, scene)
            images.append(check(ctx, scene, **view))
            T = R.setup(clip, idx, v["width"], v["height"])
            if T is not None:
                assert np.array_equal(R.cover(T, v["width"], v["height"])[0], R.cover(T, v["width"], v["height"], boxed=False)[0])
        assert R.same(images[0], images[1]) == 0
        seen.append((int((clip[:, 3] < 0.1).sum()), float(np.abs(clip[:, 3]).max()), covered(images[0])))
    assert any(behind >= 1 and far > 1000 and pixels > 0 for behind, far, pixels in seen), seen


def test_two_thousand_triangles_in_one_region(ctx):
    """2000 small triangles stacked inside one 8 x 8-pixel region, and big ones over them: none is dropped"""
    rig = ctx["rig"]
    rng = np.random.default_rng(7)
    centres = rng.uniform(31.5, 32.5, size=(2000, 1, 2))
    corners = centres + rng.uniform(-0.25, 0.25, size=(2000, 3, 2))
    depth = rng.uniform(1.0, 4.0, size=(2000, 1)).repeat(3, axis=1) + rng.uniform(-0.05, 0.05, size=(2000, 3))
    vtx = np.concatenate([corners, c_of(depth)[..., None]], axis=2).reshape(-1, 3)
    big = [(8, 32, c_of(5)), (32, 8, c_of(5)), (32, 56, c_of(5)), (56, 32, c_of(4.5))]
    vtx = np.concatenate([vtx, np.array(big)])
    idx = list(range(6000)) + [6000, 6001, 6002, 6001, 6003, 6002]
    scene = [None, item(rig, 1, vtx, idx), None]
    upload(ctx, scene)
    img = check(ctx, scene, fov=30.0, position=(0.25, 0.0, 0.0))
    assert covered(img) == 64 * 48
    m = R.transform(R.view(**dict(VIEW, fov=30.0, position=(0.25, 0.0, 0.0))))
    clip, tex = R.vertex_stage(rig["cameras"][1], ctx["dirs"][1], vtx, m)
    winner = R.raster(clip, tex, idx, 64, 48)[0]
    small = winner[(winner >= 0) & (winner < 2000)]
    span = np.argwhere((winner >= 0) & (winner < 2000))
    assert len(np.unique(small)) > 20 and (span.max(axis=0) - span.min(axis=0) <= 12).all()


def test_empty_mesh_and_refusals(ctx):
    from facebook360_dep_amd import derp

    rig = ctx["rig"]
    scene = standard(rig)
    scene[1] = item(rig, 1, [], [])
    upload(ctx, scene)
    before = check(ctx, scene)
    assert R.same(before, check(ctx, [scene[0], None, scene[2]])) == 0
    g = ctx["g"]
    vtx, idx = grid(3, lambda x, y: 2.0)
    bad = list(idx)
    bad[7] = len(vtx)  # an index equal to the vertex count
    for args, text in (((1, vtx, bad, scene[1]["rgba"]), "index 9 at position 7 is not below the vertex count 9"),
                       ((1, vtx, idx[:-1], scene[1]["rgba"]), "not a multiple of 3"),
                       ((1, vtx, idx, scene[1]["rgba"][:48]), "64x48 but the camera's resolution is 64x64"),
                       ((5, vtx, idx, scene[1]["rgba"]), "bad camera index")):
        with pytest.raises(derp.DerpError, match=text):
            g.stream_upload(*args)
    rc = derp.lib().derp_stream_upload(g.h, 1, None, 9, None, 0, None, 64, 64)
    assert rc != 0 and "null pointer" in derp.lib().derp_last_error(g.h).decode()
    assert R.same(check(ctx, scene), before) == 0  # the scene is what it was
    for kw in (dict(ipd=0.032), dict(disparity_color=True)):
        with pytest.raises(derp.DerpError, match="mono colour only"):
            g.stream_render(derp.render_params("snapshot", width=8, height=8, **kw))
    g.stream_clear()
    with pytest.raises(derp.DerpError, match="derp_stream_upload has not been called"):
        g.stream_render(derp.render_params("snapshot", width=8, height=8))
