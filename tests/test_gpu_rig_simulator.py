"""RigSimulator on the GPU against the numpy restatement (tests/sim_ref.py) and the oracle's camera model, through the
C-ABI (derp.Sim), and bin/RigSimulator end to end.

The ray stage is compared with oracle_lib.Rig.rig(cam, pixel, 1) - position narrowed to float, to within 1 float ulp per
component, outside flags equal. The trace is fed the GPU's own rays and compared with the restatement on the same rays:
hit index, distance, colour before the downscale, final colour and depth are bit-equal (0 differing values) for every ray
that hits geometry or the ceiling or lies outside the image circle — no libm function takes part there. Sky rays go
through acos / atan2, which device and glibc do not round alike: a sky texel may differ only where the restatement's own
sampleX or sampleY lies within 4 float ulps of an integer, and such rays are at most 0.1 % of a case's sky rays
(tests/test_rig_simulator.py checks the cap on the CPU). The same band holds for the equirect ray directions."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import sim_cases as K
from tests import sim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "facebook360_dep_amd", "bin")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ulps(a, b):
    """distance in float32 ulps (of the larger magnitude) between two float32 arrays"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


@pytest.fixture(scope="module")
def sim(built):
    from facebook360_dep_amd import derp

    s = derp.Sim()
    yield s
    s.close()


def _upload(sim, scene, marble=False, ceiling=False):
    tris, nodes, leaf = K.build_lib(scene)
    kw = dict(marble=marble, marble_scale=0.1)
    if ceiling:
        kw.update(K.CEILING, ceiling=K.ceiling_image())
    sim.upload(tris, nodes, leaf, K.skybox(), **kw)


def _compare_trace(sim, res, eye=0, what="", cap=True):
    """The GPU's planes of the last render against the restatement's result on the same rays. Returns the mask of sky
    rays whose texel may differ."""
    hit = sim.stage("hit", eye).reshape(-1)
    dist = sim.stage("distance", eye).reshape(-1)
    color = sim.stage("color", eye).reshape(-1, 3)
    sky = res["hit"] == -1
    exact = ~sky
    print("%s: %d rays, %d geometry, %d ceiling, %d outside, %d sky" % (
        what, hit.size, (res["hit"] >= 0).sum(), (res["hit"] == -2).sum(), (res["hit"] == -3).sum(), sky.sum()))
    assert np.array_equal(hit, res["hit"]), "%d hit indices differ" % (hit != res["hit"]).sum()
    assert np.array_equal(_bits(dist), _bits(res["distance"])), "%d distances differ" % (_bits(dist) != _bits(res["distance"])).sum()
    assert np.array_equal(_bits(color[exact]), _bits(res["color"][exact]))
    band = sky & (R.near_integer(res["sample_x"]) | R.near_integer(res["sample_y"]))
    differ = (color != res["color"]).any(axis=1)
    print("%s: %d sky texels differ, %d sky rays in the band" % (what, differ.sum(), band.sum()))
    assert not (differ & ~band).any(), "%d sky texels differ outside the band" % (differ & ~band).sum()
    if cap:
        assert band.sum() <= 0.001 * sky.sum()
    return band


@pytest.mark.parametrize("scene,cam,aas,marble,ceiling", K.CAMERA_CASES)
def test_camera_render(sim, scene, cam, aas, marble, ceiling):
    from oracle import oracle_lib as O

    camera = K.CAMERAS[cam]
    _upload(sim, scene, marble, ceiling)
    bgr, depth = sim.render_camera(camera, aas)
    assert bgr.shape == (K.H, K.W, 3) and depth.shape == (K.H, K.W)
    # ---- the ray stage against the oracle's camera
    o, d, hit = sim.stage("origin"), sim.stage("direction"), sim.stage("hit")
    assert o.shape == (K.H * aas, K.W * aas, 3)
    oo, od, outside = K.oracle_rays(camera, aas)
    assert np.array_equal(hit == -3, outside)
    assert np.array_equal(o, oo)
    worst = _ulps(d, od).max()
    print("%s %s aas %d: direction within %.2f ulp of the oracle" % (scene, cam, aas, worst))
    assert worst <= 1.0
    # ---- the trace on the GPU's own rays against the restatement
    res = R.trace(K.ref_scene(scene), o, d, K.skybox(), outside=outside, **K.trace_kwargs(marble, ceiling))
    band = _compare_trace(sim, res, what="%s %s aas %d" % (scene, cam, aas)).reshape(K.H * aas, K.W * aas)
    # ---- the downscale: final colour and depth, bit-equal wherever no band ray is averaged in
    color = res["color"].reshape(K.H * aas, K.W * aas, 3)
    clean = ~band.reshape(K.H, aas, K.W, aas).any(axis=(1, 3))
    want_bgr, want_depth = R.downscale(color, aas), R.downscale(res["distance"].reshape(K.H * aas, K.W * aas), aas)
    assert np.array_equal(_bits(bgr[clean]), _bits(want_bgr[clean]))
    assert np.array_equal(_bits(depth), _bits(want_depth))
    assert not np.isnan(depth).any()  # averaged FLT_MAX sky depths overflow to +inf, never NaN
    if aas > 1 and (res["hit"] < 0).any():
        assert np.isposinf(depth).any()
    # ---- self-consistency, independent of the restatement: a hit point projects back onto its pixel
    if aas == 1:
        geo = (res["hit"] >= 0).reshape(K.H, K.W)
        if geo.any():
            ys, xs = np.nonzero(geo)
            p = o[geo].astype(np.float64) + res["distance"].reshape(K.H, K.W)[geo].astype(np.float64)[:, None] * d[geo].astype(np.float64)
            pix = O.Rig([camera]).pixel(0, p)
            err = np.abs(pix - np.stack([xs + 0.5, ys + 0.5], axis=1)).max()
            print("%s %s: hit points project back within %.2e px" % (scene, cam, err))
            assert err <= 1e-3


def test_ray_parallel_to_the_triangle(sim):
    """The red triangle lies in the plane x = 100: a ray inside that plane has a = 0, a grazing one a * a < 1e-4, and
    both miss (RaytracingPrimitives.h:64); a steeper one hits."""
    _upload(sim, "triangle")
    rays = np.array([
        [100, -5, 1, 0, 1, 0],            # in the plane: a = 0
        [99.9997, -5, 1, 0.00005, 1, 0],  # grazing: a = 100 x 0.00005, a * a = 2.5e-5; it would hit at (100, 1, 1)
        [90, 1, 1, 1, 0, 0],              # straight at it
        [90, 1, 1, 0.7071068, 0.7071068, 0],
        [110, 2, 2, -1, 0, 0],            # from behind
        [0, 0, 0, 0, 0, 1],               # the pole of the sky
        [0, 0, 0, 0, 0, -1],
    ], np.float32)
    sim.trace_rays(rays)
    res = R.trace(K.ref_scene("triangle"), rays[:, :3], rays[:, 3:], K.skybox())
    assert list(res["hit"][:5]) == [-1, -1, 0, -1, 0]
    # seven hand-made rays are no population to take 0.1 % of: the two pole rays sit on a texel border by construction
    # (sampleY = 0 and = rows, the clamp), so instead of the cap every colour here must be equal, the sky texels too
    _compare_trace(sim, res, what="triangle rays", cap=False)
    assert np.array_equal(sim.stage("color").reshape(-1, 3), res["color"])
    sky = K.skybox()
    assert np.array_equal(res["color"][5], np.float32(255) * (sky[0, 3].astype(np.float32) / np.float32(255)))
    assert np.array_equal(res["color"][6], np.float32(255) * (sky[4, 3].astype(np.float32) / np.float32(255)))


@pytest.mark.parametrize("w,h,stereo,aas", K.EQUIRECT_CASES)
def test_equirect_render(sim, w, h, stereo, aas):
    _upload(sim, "icosa12", marble=True)
    a, b = sim.render_equirect(w, h, aas, stereo, 3.2)
    ol, orr, rd = R.equirect_rays(w * aas, h * aas, stereo, 3.2)
    d = sim.stage("direction")
    differ = (d != rd).any(axis=2)
    print("equirect %dx%d aas %d: %d of %d directions differ, worst %.2f ulp" % (w, h, aas, differ.sum(), differ.size, _ulps(d, rd).max()))
    assert _ulps(d, rd).max() <= 4 and differ.sum() <= 0.001 * differ.size
    outs = []
    for eye, ro in enumerate([ol, orr] if stereo else [ol]):
        o = sim.stage("origin", eye)
        assert _ulps(o, ro).max() <= 4 and (o != ro).any(axis=2).sum() <= 0.001 * differ.size
        res = R.trace(K.ref_scene("icosa12"), o, d, K.skybox(), marble=True)
        band = _compare_trace(sim, res, eye, "equirect %dx%d eye %d" % (w, h, eye)).reshape(h * aas, w * aas)
        clean = ~band.reshape(h, aas, w, aas).any(axis=(1, 3))
        want = R.downscale(res["color"].reshape(h * aas, w * aas, 3), aas)
        got = a if eye == 0 else b
        assert np.array_equal(_bits(got[clean]), _bits(want[clean]))
        outs.append(res)
    if not stereo:
        with np.errstate(divide="ignore"):
            inv = np.clip(np.float32(1) / outs[0]["distance"], np.float32(0), np.float32(1)).reshape(h * aas, w * aas)
        assert np.array_equal(_bits(b), _bits(R.downscale(inv, aas)))


# ---------------------------------------------------------------- bin/RigSimulator end to end
def _run(*args):
    p = subprocess.run([os.path.join(BIN, "RigSimulator")] + list(args), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-1500:]


def _to8(m):
    return np.clip(np.rint(m.astype(np.float64)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def sky_png(tmp_path_factory):
    from facebook360_dep_amd import imageio

    path = tmp_path_factory.mktemp("sky") / "sky.png"
    imageio.write_png8(str(path), K.skybox())
    return str(path)


def _ftheta_ring(count, rig_radius, w, h, circle_radius, circle_fov, top_offset):
    """makeHorizontalRingOfFThetaCameras + addTopCamera (RigSimulator.cpp:360-422) with the reference's widths: the
    cameras bin/RigSimulator renders in this mode, before --rig_out rounds them to ten digits."""
    import math

    f32 = np.float32
    focal = float(f32(2 * circle_radius) / (f32(circle_fov) * f32(math.pi) / f32(180)))
    radius = float(f32(rig_radius))
    cams = []
    for i in range(count):
        theta = -2.0 * math.pi * float(i) / float(count)
        fwd = np.array([math.cos(theta), math.sin(theta), 0.0])
        up = np.array([0.0, 0.0, 1.0])
        cams.append(dict(version=1, id=str(i), type="FTHETA", origin=list(radius * fwd), forward=list(fwd), up=list(up),
                         right=list(np.cross(fwd, up)), resolution=[float(w), float(h)], focal=[focal, focal],
                         group="side camera"))
    cams.append(dict(version=1, id=str(count), type="FTHETA", origin=[0.0, 0.0, top_offset], forward=[0.0, 0.0, 1.0],
                     up=[1.0, 0.0, 0.0], right=[0.0, 1.0, 0.0], resolution=[float(w), float(h)], focal=[focal, focal]))
    return cams


@pytest.mark.parametrize("mode", ["rig_from_json", "ftheta_ring"])
def test_cli_cameras(sim, sky_png, tmp_path, mode):
    from facebook360_dep_amd import imageio

    rig_in = tmp_path / "rig.json"
    rig_in.write_text(json.dumps({"cameras": [K.CAMERAS[k] for k in ("rect_z", "rect_x", "ftheta")]}))
    out, rig_out = tmp_path / "images", tmp_path / "rig_out.json"
    _run("--mode=" + mode, "--scene=cube", "--skybox_path=" + sky_png, "--rig_in=%s" % rig_in, "--rig_out=%s" % rig_out,
         "--dest_cam_images=%s" % out, "--anti_alias_supersample=2", "--num_cams_in_ring=2", "--ftheta_width=%d" % K.W,
         "--ftheta_height=%d" % K.H, "--ftheta_image_circle_radius=10", "--top_cam_vertical_offset=1.5")
    written = json.load(open(rig_out))["cameras"]
    if mode == "rig_from_json":
        cams = [K.CAMERAS[k] for k in ("rect_z", "rect_x", "ftheta")]
    else:
        cams = _ftheta_ring(2, 0.218, K.W, K.H, 10, 166.667, 1.5)
    # rig_out read back: the cameras rendered, to the ten digits written
    assert [c["id"] for c in written] == [c["id"] for c in cams]
    for got, want in zip(written, cams):
        assert got["type"] == want["type"] and got.get("group") == want.get("group")
        for key in ("origin", "forward", "up", "right", "resolution", "focal"):
            assert np.allclose(got[key], want[key], rtol=0, atol=1e-9), (want["id"], key)
    assert sorted(os.listdir(out)) == sorted(c["id"] + e for c in cams for e in (".png", "_depth.png", "_depth.pfm"))
    _upload(sim, "cubes")
    for c in cams:
        bgr, depth = sim.render_camera(c, 2)
        assert np.array_equal(imageio.read_png(str(out / (c["id"] + ".png"))), _to8(bgr))
        assert np.array_equal(imageio.read_png(str(out / (c["id"] + "_depth.png"))), _to8(depth))
        assert np.array_equal(_bits(imageio.read_pfm(str(out / (c["id"] + "_depth.pfm")))), _bits(depth))
    if mode == "rig_from_json":
        assert written[2]["distortion"] == [0.01, -0.002, 0.0] and written[2]["fov"] == pytest.approx(1.2, abs=1e-9)
        assert (np.asarray(imageio.read_png(str(out / "rect_z.png"))) > 0).any()


def test_cli_mono_equirect(sim, sky_png, tmp_path):
    from facebook360_dep_amd import imageio

    mono, inv = tmp_path / "mono.png", tmp_path / "inv.png"
    _run("--mode=mono_eqr", "--scene=cube", "--skybox_path=" + sky_png, "--dest_mono=%s" % mono, "--dest_mono_depth=%s" % inv,
         "--eqr_width=16", "--eqr_height=8", "--anti_alias_supersample=3")
    _upload(sim, "cubes")
    bgr, invd = sim.render_equirect(16, 8, 3, False)
    assert np.array_equal(imageio.read_png(str(mono)), _to8(bgr))
    assert np.array_equal(imageio.read_png(str(inv)), _to8(invd * np.float32(255)))
