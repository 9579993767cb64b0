"""The other kernels that take a rig camera (camera-space rephotography, the canopy cubemap, the mesh renderer) off the
square FTHETA rig: on common.mixed_type_rig (RECTILINEAR / FTHETA / EQUISOLID / ORTHOGRAPHIC, two cameras with the
default FOV) and on the reference's real calibration with and without a principal point (common.real_rig), at
84 x 54, which is the real sensor's aspect and not the mixed rig's. Bit for bit against the oracles that
tests/test_gpu_parity.py and tests/test_gpu_simple_mesh_renderer.py use on synth.make_rig. Every coverage floor is put
to the oracle's (the checker's) own image, never to the device's: the device's image is then required to equal it."""
import numpy as np
import pytest

from tests import common, smr_check
from tests.test_gpu_simple_mesh_renderer import ULP_BOUND, canopy_vs_fp64

pytestmark = pytest.mark.gpu

N, E = 6, 32
RIGS = ("mixed", "real", "real_nopr")
SIZES = {"mixed": [(96, 96), (84, 54)], "real": [(84, 54)], "real_nopr": [(84, 54)]}


def cameras(name):
    """-> (the cameras under test, the same with a principal point each, for the input renderer)"""
    if name == "mixed":
        cams = common.mixed_type_rig(40)["cameras"]
        return cams, cams
    full = common.real_rig()["cameras"]
    return (full if name == "real" else common.real_rig_no_principal()["cameras"]), full


@pytest.fixture(scope="module")
def scenes(built):
    """(rig name, (w, h)) -> colours, true disparities, the riddled ones of test_rephotography_score and the
    perturbed ones of test_canopy_cubemap; rendered once"""
    from facebook360_dep_amd import synth

    out = {}
    for name in RIGS:
        cams, render_cams = cameras(name)
        for (w, h) in SIZES[name]:
            frame = synth.make_frame({"cameras": render_cams}, [(w, h)], device="cpu")
            truth = [np.asarray(t, dtype=np.float32) for t in frame["truth"]]
            riddled = [t.copy() for t in truth]
            riddled[1][h // 6:h // 3, :] = np.nan
            riddled[2][:, w // 3:w // 3 + 10] = 0
            riddled[3][h // 2:h // 2 + 10, w // 2:w // 2 + 10] = np.inf
            out[(name, (w, h))] = dict(cams=cams, colors=frame["color"][0], truth=truth, riddled=riddled,
                                       perturbed=common.perturbed_disparities(truth))
    return out


CASES = [(name, size) for name in RIGS for size in SIZES[name]]


@pytest.mark.parametrize("name,size", CASES)
def test_rephotograph(scenes, name, size):
    """k_rephoto_splat / k_rephoto_resolve; the oracle covers 0.5 - 0.77 of the target in these cases"""
    from facebook360_dep_amd import derp
    from oracle import oracle_lib as O

    s = scenes[(name, size)]
    R = O.Rig(s["cams"]).normalize()
    g = derp.Derp(s["cams"])
    for kind in ("truth", "riddled"):
        for target in (0, 2, N - 1):
            want = O.rephotograph(R, target, s["colors"], s[kind])
            got = g.rephotograph(target, s["colors"], s[kind])
            cover = float((want[..., 3] > 0).mean())
            print("rephotograph %s %dx%d %s target %d: oracle covers %.3f" % (name, size[0], size[1], kind, target, cover))
            assert 0.2 < cover <= 1.0
            assert got.shape == want.shape == (size[1], size[0], 4)
            assert smr_check.float_equal(got, want) == 0, (kind, target, smr_check.float_equal(got, want))
    g.close()


@pytest.mark.parametrize("name", RIGS)
def test_canopy_cubemap(scenes, name):
    """k_canopy_mesh onward, from cameras 0 and 3, the camera alone and all the others. A 180-degree camera fills
    about 0.4 of the sphere, the mixed rig's 43-degree RECTILINEAR camera 0 fills 0.14: each case's floor is half of
    what the oracle fills, asked of the oracle's image, and at least a tenth of the sphere."""
    from facebook360_dep_amd import derp
    from oracle import oracle_lib as O

    s = scenes[(name, (84, 54))]
    cams, colors, disps = s["cams"], s["colors"], s["perturbed"]
    R = O.Rig(cams).normalize()
    g = derp.Derp(cams)
    g.rephotograph_upload(colors, disps)
    for i in (0, 3):
        centre = cams[i]["origin"]
        for which, include in (("only", [int(k == i) for k in range(N)]), ("others", [int(k != i) for k in range(N)])):
            want = O.canopy_cubemap(R, colors, disps, include, centre, E)
            got = g.canopy_cubemap(include, centre, E)
            alpha = float((want[..., 3] > 0).mean())
            print("canopy %s camera %d %s: oracle alpha %.3f" % (name, i, which, alpha))
            assert set(np.unique(want[..., 3])) <= {0.0, 1.0} and 0.1 < alpha < 1.0
            assert got.shape == want.shape == (6 * E, E, 4)
            assert smr_check.float_equal(got, want) == 0, (i, which, smr_check.float_equal(got, want))
            assert float((got[..., 3] > 0).mean()) > 0.5 * alpha
    g.close()


def bgra(colors):
    return [np.concatenate([c.astype(np.float32) / np.float32(65535), np.ones(c.shape[:2] + (1,), np.float32)], axis=2)
            for c in colors]


def expected_format(fmt, cams, disps, cols, verts_l, verts_r, W, H, forward):
    kw = dict(width=W, height=H, alpha_blend=True, forward=forward)
    if fmt in ("cubecolor", "cubedisp", "eqrcolor", "eqrdisp", "snapcolor", "snapdisp"):
        kind = {"cub": "cube", "eqr": "equirect", "sna": "snapshot"}[fmt[:3]]
        return smr_check.render(cams, disps, cols, kind=kind, disparity_color=fmt.endswith("disp"), **kw)
    if fmt == "tb3dof":
        c = smr_check.render(cams, disps, cols, kind="equirect", **kw)
        d = smr_check.render(cams, disps, cols, kind="equirect", disparity_color=True, **kw)
        return np.concatenate([c, d], axis=0)
    left = smr_check.render(cams, disps, cols, kind="equirect", verts=verts_l, **kw)
    right = smr_check.render(cams, disps, cols, kind="equirect", verts=verts_r, **kw)
    if fmt == "tbstereo":
        return np.concatenate([left, right], axis=0)
    w = left.shape[1]
    return np.concatenate([left[:, w // 4:w // 4 + w // 2], right[:, w // 4:w // 4 + w // 2]], axis=1)


@pytest.mark.parametrize("name", RIGS)
def test_mesh_renderer_formats(scenes, name):
    """k_smr_mesh, k_smr_texture and the rest on 84 x 54 disparities (the existing tests: 96 x 96), every format of
    derp.FORMATS with alpha blending into 64 x 32, and the stereo vertex stage for +-0.032. The snapshot's default
    pose looks along -x, where the mixed rig's arc (which looks along +x, 20 degrees either side) has nothing: the
    checker covers 0.0 of it. On that rig the snapshot looks along +x instead; everything else keeps the defaults.
    lr180 is the half of each eye's equirect about -x, of which that arc reaches the rim only: the checker covers 0.11
    of it there, and its floor on that rig is 0.1. The checker covers more than 0.45 of every other image."""
    from facebook360_dep_amd import derp

    s = scenes[(name, (84, 54))]
    cams, disps = s["cams"], s["perturbed"]
    cols = bgra(s["colors"])
    forward = (1, 0, 0) if name == "mixed" else (-1, 0, 0)
    W, H = 2 * E, E
    g = derp.Derp(cams)
    g.render_upload(disps, cols)
    vl = [g.render_vertices(k, disps[k].shape, 0.032) for k in range(N)]
    vr = [g.render_vertices(k, disps[k].shape, -0.032) for k in range(N)]
    # the stereo stage as test_stereo_vertices_fp64 pins it: within ULP_BOUND float ulps of canopyVS in fp64 on the
    # undisplaced vertices (which the mono formats below pin through the checker's own unprojection)
    worst = 0.0
    for k in range(N):
        mono = g.render_vertices(k, disps[k].shape, 0.0)[..., :3]
        ok = np.isfinite(mono).all(axis=-1) & (np.hypot(mono[..., 0], mono[..., 1]) > 0.1)
        assert ok.mean() > 0.5
        for ipdm, dev in ((0.032, vl[k]), (-0.032, vr[k])):
            with np.errstate(all="ignore"):
                want = canopy_vs_fp64(mono, ipdm)
            scale = np.spacing(np.abs(want).max(axis=-1).astype(np.float32)).astype(np.float64)
            ulps = (np.abs(dev[..., :3].astype(np.float64) - want).max(axis=-1) / scale)[ok]
            worst = max(worst, float(ulps.max()))
            assert np.abs(dev[..., :3] - mono)[ok].max() > 1e-3  # displaced
    print("%s stereo vertices: worst %.2f ulp vs fp64" % (name, worst))
    assert worst <= ULP_BOUND
    p = derp.render_params(width=W, height=H, alpha_blend=True, forward=forward)
    for fmt in derp.FORMATS:
        want = expected_format(fmt, cams, disps, cols, vl, vr, W, H, forward)
        got = g.render_format(fmt, p)
        cover = float((~np.isnan(want[..., 3])).mean())
        print("%s %s: the checker covers %.3f" % (name, fmt, cover))
        assert cover > (0.1 if (name, fmt) == ("mixed", "lr180") else 0.45), (fmt, cover)
        assert got.shape == want.shape, fmt
        assert smr_check.float_equal(got, want) == 0, (fmt, smr_check.float_equal(got, want))
    g.close()
