"""The mesh renderers (k_smr_* of derp_render.h, k_canopy_* of derp_kernels.h) where triangles outgrow pixels and at
their size edges: every case of tests/render_cases.py on the device against the CPU checker's image (derp_render) or the
oracle's (derp_canopy_cubemap), 0 differing values, NaN positions included, no tolerance. tests/test_render_cases.py
shows on the checker alone that the cases reach the workgroup-per-triangle rasterisers (k_smr_raster_big,
k_canopy_raster_big), contests between the two classes, near-plane drops, alpha discards, id ties and the levels of
odd mip chains; every floor there is put to the checker's image, and the device's is required to equal it. Also:
--background_equirect by value against the restatement of SimpleMeshRenderer.cpp:285-322, stereo formats on a
magnified mesh, and the order independence of the caches of smr_prepare."""
import numpy as np
import pytest

from tests import render_cases as RC
from tests import smr_check

pytestmark = pytest.mark.gpu


class Context:
    """one device context of a rig and the scenes it holds, so that a scene is uploaded when it changes only"""

    def __init__(self, cams):
        from facebook360_dep_amd import derp

        self.g = derp.Derp(cams)
        self.smr = self.canopy = None

    def upload(self, name):
        c = RC.CASES[name]
        s = RC.case_scene(name)
        key = (c["rig"], c["mesh"], c["tex"], c["perturb"])
        if c["renderer"] == "canopy":
            if self.canopy != key:
                self.g.rephotograph_upload(s["colors16"], s["disps"])
                self.canopy = key
        elif self.smr != key:
            self.g.render_upload(s["disps"], s["cols"])
            self.smr = key
        return self.g


@pytest.fixture(scope="module")
def contexts(built):
    held = {}

    def get(rig):
        if rig not in held:
            held[rig] = Context(RC.cameras(rig)[0])
        return held[rig]

    yield get
    for c in held.values():
        c.g.close()


def params(view):
    from facebook360_dep_amd import derp

    view = dict(view)
    view["horizontal_fov"] = view.pop("fov")
    return derp.render_params(**view)


@pytest.mark.parametrize("name", RC.NAMES)
def test_case(contexts, name):
    c = RC.CASES[name]
    g = contexts(c["rig"]).upload(name)
    view = RC.view_args(name)
    if c["renderer"] == "canopy":
        want = RC.oracle(name)
        got = g.canopy_cubemap(RC.include_of(name), view["position"], c["height"])
    else:
        want = RC.checker(name)[0]
        got = g.render(params(view), c["include"])
    assert got.shape == want.shape
    differing = smr_check.float_equal(got, want)
    st = RC.checker(name)[1]
    print("%s: %d of %d values differ; the checker rasterised %d small and %d big triangles" %
          (name, differing, want.size, st["tri_small"], st["tri_big"]))
    assert differing == 0


@pytest.mark.parametrize("fmt", ["lr180", "tbstereo"])
def test_stereo_magnified(contexts, fmt):
    """the stereo formats on the 5 x 4 meshes of rig4 into E = 24. The stereo vertex stage has no bit-exact host twin:
    the checker takes the device's displaced vertices, as in tests/test_gpu_simple_mesh_renderer.py"""
    from facebook360_dep_amd import derp

    name = "rig4_mag5x4_eqr"
    s = RC.case_scene(name)
    g = contexts("rig4").upload(name)
    E = RC.CASES[name]["height"]
    eyes = []
    for ipd in (0.032, -0.032):
        verts = [g.render_vertices(k, d.shape, ipd) for k, d in enumerate(s["disps"])]
        st = {}
        eyes.append(smr_check.render(s["cams"], s["disps"], s["cols"], verts=verts, kind="equirect", height=E, stats=st))
        print("%s eye %+.3f: the checker rasterised %d small and %d big triangles, big ones won %d of %d pixels" %
              (fmt, ipd, st["tri_small"], st["tri_big"], st["pix_big"], st["pix_small"] + st["pix_big"]))
        assert st["tri_big"] > 0 and st["pix_big"] > 0 and st["pix_small"] > 0
    left, right = eyes
    assert smr_check.float_equal(left, right) > 0
    if fmt == "tbstereo":
        want = np.concatenate([left, right], axis=0)
    else:
        w = left.shape[1]
        want = np.concatenate([left[:, w // 4:w // 4 + w // 2], right[:, w // 4:w // 4 + w // 2]], axis=1)
    got = g.render_format(fmt, derp.render_params(width=2 * E, height=E))
    assert got.shape == want.shape
    assert smr_check.float_equal(got, want) == 0


@pytest.fixture(scope="module")
def background_context(built):
    from facebook360_dep_amd import derp

    s = RC.background_scene()
    g = derp.Derp(s["cams"])
    g.render_upload(s["disps"], s["cols"])
    yield g
    g.close()


@pytest.mark.parametrize("name", sorted(RC.BACKGROUNDS))
def test_background_equirect(background_context, name):
    """--background_equirect (smr_fetch_table + k_smr_background_equirect), after --background where the case has one,
    against chk_background_equirect: both run the reference's float arithmetic on the host against the same libm, so
    0 differing values"""
    g = background_context
    fmt, view, equi, back = RC.background_case(name)
    p = params(dict(view, kind="equirect"))  # render_format sets the kind
    fore = g.render_format(fmt, p)
    want_fore, want, clamped = RC.background_checker(name)
    assert smr_check.float_equal(fore, want_fore) == 0
    got = g.render_format(fmt, p, background=back, background_equirect=equi)
    print("%s: the clamp decides %d texels" % (name, clamped))
    assert not np.isnan(got).any()
    assert smr_check.float_equal(got, want) == 0


def test_order_independence(built):
    """smr_prepare caches the disparity textures by position and the stereo vertices by ipd, and derp_render_upload
    replaces the scene: whatever was rendered before, an image equals the one a fresh context gives for the same call"""
    from facebook360_dep_amd import derp

    cams = RC.cameras("rig4")[0]
    first = RC.scene("rig4", (8, 6), (10, 7), None)
    other = RC.scene("rig4", ((2, 2), (5, 4), (8, 6), (12, 9)), (5, 3), None)
    A, B = (0, 0, 0), (0.3, 0.4, 0.2)
    E = 17

    def call(g, fmt, position):
        return g.render_format(fmt, derp.render_params(width=2 * E, height=E, position=position))

    def fresh(scene, fmt, position):
        g = derp.Derp(cams)
        g.render_upload(scene["disps"], scene["cols"])
        out = call(g, fmt, position)
        g.close()
        return out

    sequence = [(first, "eqrdisp", A), (first, "eqrdisp", B), (first, "eqrdisp", A), (first, "tbstereo", A),
                (first, "eqrcolor", A), (first, "lr180", A), (other, "eqrdisp", B), (other, "tbstereo", A),
                (first, "eqrdisp", A), (first, "lr180", B)]
    g = derp.Derp(cams)
    held = None
    images = []
    for scene, fmt, position in sequence:
        if scene is not held:
            g.render_upload(scene["disps"], scene["cols"])
            held = scene
        images.append(call(g, fmt, position))
    g.close()
    for (scene, fmt, position), got in zip(sequence, images):
        assert smr_check.float_equal(got, fresh(scene, fmt, position)) == 0, (fmt, position)
    # the calls are not all alike: the position and the scene matter
    assert smr_check.float_equal(images[0], images[1]) > 0 and images[6].shape == images[0].shape
    assert smr_check.float_equal(images[6], images[1]) > 0
    assert smr_check.float_equal(images[0], images[2]) == 0
    want = smr_check.render(cams, first["disps"], first["cols"], kind="equirect", height=E, position=B, disparity_color=True)
    assert smr_check.float_equal(images[1], want) == 0
