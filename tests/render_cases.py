"""The scenes and views that tests/test_render_cases.py (CPU) and tests/test_gpu_render_limits.py (GPU) share: the mesh
renderers where triangles outgrow pixels and at their size edges, with the checker's (tests/smr_check.py) or the
oracle's (oracle_lib.canopy_cubemap) image and the checker's statistics computed once per case. Nothing here touches
the GPU.

A case is a dict: rig, mesh (one (w, h) or one per camera), tex (w, h), perturb, renderer "smr" (derp_render against
the checker) or "canopy" (derp_canopy_cubemap against the oracle; u16 colours at the mesh size), and the view."""
import functools

import numpy as np

from tests import smr_check

F32 = np.float32
RIGS = ("rig4", "mixed", "real")
MAGNIFIED_MESHES = ((2, 2), (3, 2), (5, 4), (8, 6), (12, 9))


@functools.lru_cache(maxsize=None)
def cameras(rig):
    """-> (the cameras under test, the same with a principal point each, for the input renderer)"""
    from facebook360_dep_amd import synth
    from tests import common

    if rig == "rig4":
        cams = synth.make_rig(4, 64)["cameras"]
    elif rig == "mixed":
        cams = common.mixed_type_rig(40)["cameras"]
    elif rig == "real":
        cams = common.real_rig()["cameras"]
    elif rig == "real_np":
        return common.real_rig_no_principal()["cameras"], common.real_rig()["cameras"]
    else:
        raise KeyError(rig)
    return cams, cams


@functools.lru_cache(maxsize=None)
def _camera_image(rig, s, w, h):
    """-> (bgr u16 [h, w, 3], true disparity f32 [h, w]) of camera s of the analytic scene"""
    from facebook360_dep_amd import synth

    bgr, disp = synth.render_camera(cameras(rig)[1][s], w, h, device="cpu")[:2]
    return bgr, np.asarray(disp, dtype=F32)


def _perturb(disps, how):
    """closeup (24 x 18 meshes): camera 1 has a x8 slab, camera 0 one pixel each of 0, +inf and -0.5, camera 2 a 2 x 2
    NaN hole; perturbed: common.perturbed_disparities"""
    from tests import common

    if how is None:
        return disps
    if how == "perturbed":
        return common.perturbed_disparities(disps)
    assert how == "closeup"
    disps = [d.copy() for d in disps]
    h, w = disps[1].shape
    disps[1][h // 4:h // 4 + h // 3, w // 3:w // 3 + w // 3] *= 8
    disps[0][4, 5] = 0.0
    disps[0][9, 12] = np.inf
    disps[0][13, 18] = -0.5
    disps[2][7:9, 10:12] = np.nan
    return disps


@functools.lru_cache(maxsize=None)
def scene(rig, mesh, tex, perturb):
    """-> dict(cams, disps f32 per camera, cols float BGRA per camera at `tex`, colors16 u16 BGR at the mesh size)"""
    cams = cameras(rig)[0]
    sizes = mesh if isinstance(mesh[0], tuple) else (mesh,) * len(cams)
    disps = _perturb([_camera_image(rig, s, w, h)[1].copy() for s, (w, h) in enumerate(sizes)], perturb)
    cols = []
    for s in range(len(cams)):
        c = _camera_image(rig, s, tex[0], tex[1])[0]
        cols.append(np.concatenate([c.astype(F32) / F32(65535), np.ones(c.shape[:2] + (1,), F32)], axis=2))
    colors16 = [_camera_image(rig, s, w, h)[0] for s, (w, h) in enumerate(sizes)]
    return dict(cams=cams, disps=disps, cols=cols, colors16=colors16)


def _vec(cams, spec):
    """a position or a direction: a 3-vector, or ("cam", i) / ("ahead", i, metres) / ("forward", i) / ("skew", i) of
    camera i"""
    if spec[0] == "cam":
        return tuple(cams[spec[1]]["origin"])
    if spec[0] == "ahead":
        c = cams[spec[1]]
        return tuple(float(o) + spec[2] * float(f) for o, f in zip(c["origin"], c["forward"]))
    if spec[0] == "forward":
        return tuple(cams[spec[1]]["forward"])
    if spec[0] == "skew":  # camera i's forward, unnormalised and tilted
        return tuple(3.0 * float(f) + d for f, d in zip(cams[spec[1]]["forward"], (0.2, 0.1, -0.4)))
    return tuple(float(v) for v in spec)


def _case(rig, mesh, tex=(10, 7), perturb=None, renderer="smr", kind="cube", width=0, height=24, position=(0, 0, 0),
          forward=(-1, 0, 0), up=(0, 0, 1), fov=90.0, weight="svd", alpha_blend=True, zero_nans=False, include=None):
    return dict(rig=rig, mesh=mesh, tex=tex, perturb=perturb, renderer=renderer, kind=kind, width=width, height=height,
                position=position, forward=forward, up=up, fov=fov, weight=weight, alpha_blend=alpha_blend,
                zero_nans=zero_nans, include=include)


def _snap_forward(rig):
    """the default forward (-1, 0, 0) covers nothing of the mixed rig's arc, which looks along +x"""
    return (1, 0, 0) if rig == "mixed" else (-1, 0, 0)


def _build_cases():
    C = {}
    for rig in RIGS + ("real_np",):
        meshes = MAGNIFIED_MESHES if rig != "real_np" else ((5, 4), (8, 6))
        for (w, h) in meshes:
            # magnified meshes: every triangle big at 2 x 2, both classes at 5 x 4 and 8 x 6, none big at 12 x 9
            C["%s_mag%dx%d_cube" % (rig, w, h)] = _case(rig, (w, h))
            C["%s_mag%dx%d_eqr" % (rig, w, h)] = _case(rig, (w, h), kind="equirect")
            C["%s_mag%dx%d_canopy" % (rig, w, h)] = _case(rig, (w, h), tex=(w, h), renderer="canopy")
    for rig in RIGS:
        # magnifying snapshots: rig4 at fov 20 covers nothing along -x, it looks along camera 1's forward instead
        for fov in (20.0, 150.0):
            fwd = ("forward", 1) if (rig, fov) == ("rig4", 20.0) else _snap_forward(rig)
            C["%s_snap_fov%d" % (rig, fov)] = _case(rig, (24, 24), tex=(48, 48), kind="snapshot", width=50, height=38,
                                                    forward=fwd, fov=fov)
        # close-up with discontinuities
        views = (("origin", (0, 0, 0)), ("cam1", ("cam", 1)), ("ahead1", ("ahead", 1, 1.0)), ("off", (0.3, 0.4, 0.2)))
        for vname, pos in views:
            C["%s_close_%s_cube" % (rig, vname)] = _case(rig, (24, 18), tex=(24, 18), perturb="closeup", height=40,
                                                         position=pos)
            C["%s_close_%s_snap" % (rig, vname)] = _case(rig, (24, 18), tex=(24, 18), perturb="closeup",
                                                         kind="snapshot", width=50, height=38, position=pos,
                                                         forward=("forward", 1), fov=60.0)
            C["%s_close_%s_canopy" % (rig, vname)] = _case(rig, (24, 18), tex=(24, 18), perturb="closeup",
                                                           renderer="canopy", height=40, position=pos)
    # ---- size edges
    for rig in ("real", "rig4"):
        for E in (1, 2, 3, 17):
            C["%s_E%d_cube" % (rig, E)] = _case(rig, (8, 6), height=E)
            C["%s_E%d_eqr" % (rig, E)] = _case(rig, (8, 6), kind="equirect", height=E)
            C["%s_E%d_canopy" % (rig, E)] = _case(rig, (8, 6), tex=(8, 6), renderer="canopy", height=E)
    for (W, H) in ((1, 1), (33, 17), (31, 33)):
        C["mixed_snap_%dx%d" % (W, H)] = _case("mixed", (8, 6), kind="snapshot", width=W, height=H, forward=(1, 0, 0))
    # forward unnormalised, up not perpendicular to it, position off the origin
    for rig in RIGS:
        C["%s_snap_pose" % rig] = _case(rig, (8, 6), kind="snapshot", width=33, height=17, position=(0.05, -0.1, 0.07),
                                        forward=("skew", 1), up=(0.3, 0.2, 2.0), fov=70.0)
    # textures of 1 x 1 (a one-level chain), odd sizes unrelated to the mesh and one larger than the mesh, on an
    # 84 x 54 mesh. A face pixel of E = 8 spans 11 degrees, less than a texel of the small textures (36 degrees in
    # 5 x 3): those are minified, and levels >= 1 of their odd chains read, at E = 2 and E = 1 (TEXTURE_MINIFIED)
    for tex in ((1, 1), (5, 3), (2, 9), (200, 120)):
        for E in (8, 2, 1):
            C["rig4_tex%dx%d_E%d" % (tex + (E,))] = _case("rig4", (84, 54), tex=tex, perturb="perturbed", height=E)
    # include masks for equirect and snapshot
    for iname, inc in (("one", (0, 1, 0, 0)), ("allbut", (1, 1, 0, 1))):
        C["rig4_include_%s_eqr" % iname] = _case("rig4", (8, 6), kind="equirect", height=17, include=inc)
        C["rig4_include_%s_snap" % iname] = _case("rig4", (8, 6), kind="snapshot", width=33, height=17,
                                                  forward=("forward", 1), include=inc)
    # weight x alpha_blend x zero_nans on a magnified and on a sub-pixel case
    for weight in ("svd", "minor"):
        for blend in (True, False):
            for zn in (True, False):
                tag = "%s_%s_%s" % (weight, "blend" if blend else "noblend", "zn" if zn else "nan")
                C["rig4_matrix_mag_" + tag] = _case("rig4", (5, 4), weight=weight, alpha_blend=blend, zero_nans=zn)
                C["rig4_matrix_sub_" + tag] = _case("rig4", (84, 54), tex=(84, 54), perturb="perturbed", height=16,
                                                    weight=weight, alpha_blend=blend, zero_nans=zn)
    # per-camera mesh sizes within one upload: maxTri and the big-triangle list are shared across the cameras
    sizes = ((2, 2), (5, 4), (8, 6), (12, 9))
    C["rig4_sizes_cube"] = _case("rig4", sizes)
    C["rig4_sizes_eqr"] = _case("rig4", sizes, kind="equirect")
    C["rig4_sizes_rev_cube"] = _case("rig4", sizes[::-1])
    return C


CASES = _build_cases()
NAMES = sorted(CASES)
# the cases that must sample a mip level above 0 of their texture (the checker's mip_above0 counter)
TEXTURE_MINIFIED = ("rig4_tex5x3_E2", "rig4_tex5x3_E1", "rig4_tex2x9_E2", "rig4_tex2x9_E1", "rig4_tex200x120_E8",
                    "rig4_tex200x120_E2")


def case_scene(name):
    c = CASES[name]
    return scene(c["rig"], c["mesh"], c["tex"], c["perturb"])


def view_args(name):
    """the case's view as smr_check.render's keyword arguments (derp.render_params takes the same, with
    horizontal_fov for fov)"""
    c = CASES[name]
    cams = case_scene(name)["cams"]
    return dict(kind=c["kind"], width=c["width"] or 2 * c["height"], height=c["height"],
                position=_vec(cams, c["position"]), forward=_vec(cams, c["forward"]), up=c["up"], fov=c["fov"],
                weight=c["weight"], alpha_blend=c["alpha_blend"], zero_nans=c["zero_nans"])


def include_of(name):
    c = CASES[name]
    n = len(case_scene(name)["cams"])
    return [1] * n if c["include"] is None else list(c["include"])


def _u16_bgra(colors16):
    return [np.concatenate([c.astype(F32) / F32(65535), np.ones(c.shape[:2] + (1,), F32)], axis=2) for c in colors16]


@functools.lru_cache(maxsize=None)
def checker(name):
    """-> (the checker's image, its statistics). A canopy case: the checker configured as the rephotography renderer
    (minor weight, alphaBlend, u16 colours at the mesh size, NaN -> 0), which tests/test_render_cases.py shows to be
    the oracle's image."""
    c = CASES[name]
    s = case_scene(name)
    stats = {}
    kw = view_args(name)
    if c["renderer"] == "canopy":
        kw.update(kind="cube", weight="minor", alpha_blend=True, zero_nans=True)
        img = smr_check.render(s["cams"], s["disps"], _u16_bgra(s["colors16"]), include=include_of(name), stats=stats, **kw)
    else:
        img = smr_check.render(s["cams"], s["disps"], s["cols"], include=c["include"], stats=stats, **kw)
    img.setflags(write=False)
    return img, stats


@functools.lru_cache(maxsize=None)
def oracle(name):
    """a canopy case's image from oracle_canopy.h's cubemap"""
    from oracle import oracle_lib as O

    c = CASES[name]
    assert c["renderer"] == "canopy"
    s = case_scene(name)
    R = O.Rig(s["cams"]).normalize()
    img = O.canopy_cubemap(R, s["colors16"], s["disps"], include_of(name), view_args(name)["position"], c["height"])
    img.setflags(write=False)
    return img


def covered(name, img):
    """the pixels an image covers: alpha not NaN, or alpha > 0 where the case turns NaN into 0 (the canopy cases and
    zero_nans); name "": an image with NaN"""
    c = CASES.get(name)
    return img[..., 3] > 0 if c and (c["renderer"] == "canopy" or c["zero_nans"]) else ~np.isnan(img[..., 3])


@functools.lru_cache(maxsize=None)
def checker_faces(name):
    """the image the statistics count pixels of: an equirect case's cube faces, else the case's image"""
    c = CASES[name]
    if c["kind"] != "equirect":
        return checker(name)[0]
    s = case_scene(name)
    return smr_check.render(s["cams"], s["disps"], s["cols"], include=c["include"], **dict(view_args(name), kind="cube"))


def reaches_both(stats):
    """part 2's reach conditions of one case"""
    pix = stats["pix_small"] + stats["pix_big"]
    return (pix > 0 and stats["pix_big"] > 0.2 * pix and stats["pix_small"] > 0 and stats["displaced"] >= 1 and
            stats["near_drops"] > 0 and stats["alpha_discards"] > 0)


# ---- --background_equirect by value (chk_background_equirect restates SimpleMeshRenderer.cpp:285-322) ----
# name -> (format, width, height, forward, up, position, fov, equirect (w, h), a fractional --background first?)
# The scene is rig4's first camera alone (an 8 x 6 mesh): it leaves most of the sphere uncovered, alpha NaN. A background
# of alpha 0.4 blended first makes those alphas fractional. Looking straight down with an odd viewport the centre ray
# has lat = -90 degrees, looking along +x its centre column has lon = -180 degrees: the truncated index is one past the
# image there and the clamp decides the texel. The pose that looks down stands a millimetre off the origin: from the
# origin itself the centre ray's longitude is atan2 of two signed zeros, which the reference's text leaves to the signs
# its matrix inverse happens to produce; a millimetre off, z / |world| still rounds to -1 and the longitude is defined.
BACKGROUNDS = {
    "snap_40x20": ("snapcolor", 33, 17, (-0.5, -1.0, 0.3), (0.3, 0.2, 2.0), (0.05, -0.1, 0.07), 70.0, (40, 20), False),
    "snap_7x3_fractional": ("snapcolor", 33, 17, (-0.5, -1.0, 0.3), (0, 0, 1), (0, 0, 0), 90.0, (7, 3), True),
    "eqr_40x20_fractional": ("eqrcolor", 32, 16, (-1, 0, 0), (0, 0, 1), (0, 0, 0), 90.0, (40, 20), True),
    "eqr_7x3": ("eqrcolor", 32, 16, (-1, 0, 0), (0, 0, 1), (0, 0, 0), 90.0, (7, 3), False),
    "snap_down_lat90": ("snapcolor", 7, 5, (0, 0, -1), (1, 0, 0), (0.001, 0.002, 0), 90.0, (40, 20), False),
    "snap_plusx_lon180": ("snapcolor", 7, 5, (1, 0, 0), (0, 0, 1), (0, 0, 0), 175.0, (7, 3), False),
}
BACKGROUND_CLAMPED = ("snap_down_lat90", "snap_plusx_lon180")


@functools.lru_cache(maxsize=None)
def background_scene():
    s = scene("rig4", (8, 6), (10, 7), None)
    return dict(cams=s["cams"][:1], disps=s["disps"][:1], cols=s["cols"][:1])


def background_case(name):
    """-> (format, view keyword arguments, equirect [eh, ew, 4], background [h, w, 4] or None)"""
    fmt, W, H, fwd, up, pos, fov, (ew, eh), fractional = BACKGROUNDS[name]
    cams = background_scene()["cams"]
    view = dict(width=W, height=H, position=pos, forward=_vec(cams, fwd), up=up, fov=fov)
    rng = np.random.default_rng(sorted(BACKGROUNDS).index(name))
    equi = rng.random((eh, ew, 4), dtype=F32)
    equi[..., 3] = 1
    back = None
    if fractional:
        back = rng.random((H, W, 4), dtype=F32)
        back[..., 3] = F32(0.4)
    return fmt, view, equi, back


def background_composite(name, fore):
    """SimpleMeshWindow::generate on the rendered image `fore`: alphaBlend over --background, then
    backgroundEquirect -> (image, pixels whose texel the clamp decided)"""
    fmt, view, equi, back = background_case(name)
    if back is not None:
        fore = smr_check.alpha_blend(fore, back)
    stats = {}
    out = smr_check.background_equirect(fore, equi, view["position"], view["forward"], view["up"], view["fov"], stats)
    return out, stats["clamped"]


@functools.lru_cache(maxsize=None)
def background_checker(name):
    """-> (the checker's foreground, composited, pixels decided by the clamp)"""
    fmt, view, equi, back = background_case(name)
    s = background_scene()
    fore = smr_check.render(s["cams"], s["disps"], s["cols"], kind={"snapcolor": "snapshot", "eqrcolor": "equirect"}[fmt],
                            **view)
    out, clamped = background_composite(name, fore)
    return fore, out, clamped
