"""SimpleMeshRenderer's GPU renderer (derp_render_*, facebook360_dep_amd/csrc/derp_render.h) on synth rigs:
anchored to the rephotography renderer's oracle, every format against the CPU checker bit for bit (NaN positions
included), the stereo vertex stage against an fp64 evaluation of canopyVS, and the geometry against the analytic
scene."""
import math
import os

import numpy as np
import pytest

from tests import smr_check

pytestmark = pytest.mark.gpu

N, RES, E = 6, 96, 32


@pytest.fixture(scope="module")
def scene(built):
    from facebook360_dep_amd import synth

    rig = synth.make_rig(N, RES)
    frame = synth.make_frame(rig, [(RES, RES)], device="cpu")
    truth = [d.copy() for d in frame["truth"]]
    pert = [d.copy() for d in truth]
    rng = np.random.default_rng(3)
    pert[1][20:40, 30:50] *= 2.5            # a foreground slab, as test_canopy_cubemap
    pert[3][60:64, 10:14] = np.nan          # a hole
    pert[4] = pert[4] * (1 + 0.02 * rng.standard_normal(pert[4].shape)).astype(np.float32)
    big = synth.make_frame(rig, [(2 * RES, 2 * RES)], device="cpu")["color"][0]
    return dict(rig=rig, colors=frame["color"][0], truth=truth, pert=pert, big=big)


def bgra(colors):
    return [np.concatenate([c.astype(np.float32) / np.float32(65535), np.ones(c.shape[:2] + (1,), np.float32)], axis=2)
            for c in colors]


def test_anchor_rephotography_configuration(scene):
    """minor weight, alphaBlend, ipd 0, same-size u16 colours, NaN -> 0 == the oracle's canopy cubemap"""
    from facebook360_dep_amd import derp
    from oracle import oracle_lib as O

    rig, colors, disps = scene["rig"], scene["colors"], scene["pert"]
    R = O.Rig(rig["cameras"]).normalize()
    g = derp.Derp(rig["cameras"])
    g.render_upload(disps, bgra(colors))
    g.rephotograph_upload(colors, disps)
    for i in (0, 3):
        centre = rig["cameras"][i]["origin"]
        p = derp.render_params("cube", height=E, position=centre, weight="minor", zero_nans=True)
        for include in ([int(s == i) for s in range(N)], [int(s != i) for s in range(N)]):
            want = O.canopy_cubemap(R, colors, disps, include, centre, E)
            assert smr_check.float_equal(g.render(p, include), want) == 0
            assert smr_check.float_equal(g.canopy_cubemap(include, centre, E), want) == 0
    g.close()


def expected_format(fmt, cams, disps, cols, verts_l, verts_r, blend, W, H):
    common = dict(width=W, height=H, alpha_blend=blend)
    if fmt in ("cubecolor", "cubedisp", "eqrcolor", "eqrdisp", "snapcolor", "snapdisp"):
        kind = {"cub": "cube", "eqr": "equirect", "sna": "snapshot"}[fmt[:3]]
        return smr_check.render(cams, disps, cols, kind=kind, disparity_color=fmt.endswith("disp"), **common)
    if fmt == "tb3dof":
        c = smr_check.render(cams, disps, cols, kind="equirect", **common)
        d = smr_check.render(cams, disps, cols, kind="equirect", disparity_color=True, **common)
        return np.concatenate([c, d], axis=0)
    left = smr_check.render(cams, disps, cols, kind="equirect", verts=verts_l, **common)
    right = smr_check.render(cams, disps, cols, kind="equirect", verts=verts_r, **common)
    if fmt == "tbstereo":
        return np.concatenate([left, right], axis=0)
    w = left.shape[1]
    return np.concatenate([left[:, w // 4:w // 4 + w // 2], right[:, w // 4:w // 4 + w // 2]], axis=1)


@pytest.mark.parametrize("case", ["truth", "perturbed_noblend", "perturbed_bigtex"])
def test_formats_against_checker(scene, case):
    from facebook360_dep_amd import derp

    rig = scene["rig"]
    cams = rig["cameras"]
    disps = scene["truth"] if case == "truth" else scene["pert"]
    cols = bgra(scene["big"] if case == "perturbed_bigtex" else scene["colors"])
    blend = case != "perturbed_noblend"
    W, H = 2 * E, E
    g = derp.Derp(cams)
    g.render_upload(disps, cols)
    vl = [g.render_vertices(s, disps[s].shape, 0.032) for s in range(N)]
    vr = [g.render_vertices(s, disps[s].shape, -0.032) for s in range(N)]
    p = derp.render_params(width=W, height=H, alpha_blend=blend)
    for fmt in derp.FORMATS:
        got = g.render_format(fmt, p)
        want = expected_format(fmt, cams, disps, cols, vl, vr, blend, W, H)
        assert got.shape == want.shape, fmt
        nan = np.isnan(got[..., 3])
        assert smr_check.float_equal(got, want) == 0, (fmt, case, smr_check.float_equal(got, want))
        assert 0.5 < (~nan).mean(), (fmt, (~nan).mean())
        print("%s %s: bit-exact, %.1f %% covered" % (case, fmt, 100 * (~nan).mean()))
    g.close()


def test_background_compositing(scene):
    from facebook360_dep_amd import derp

    rig = scene["rig"]
    cams = rig["cameras"][:2]  # partial coverage: NaN pixels to fill
    disps, cols = scene["truth"][:2], bgra(scene["colors"][:2])
    g = derp.Derp(cams)
    g.render_upload(disps, cols)
    p = derp.render_params(width=2 * E, height=E)
    fore = g.render_format("eqrcolor", p)
    assert np.isnan(fore[..., 3]).any()
    back = np.random.default_rng(5).random(fore.shape, dtype=np.float32)
    back[..., 3] = 1
    got = g.render_format("eqrcolor", p, background=back)
    assert smr_check.float_equal(got, smr_check.alpha_blend(fore, back)) == 0
    eq = np.random.default_rng(6).random((20, 40, 4), dtype=np.float32)
    eq[..., 3] = 1
    got = g.render_format("eqrcolor", p, background_equirect=eq)
    assert not np.isnan(got).any()
    assert smr_check.float_equal(got, smr_check.background_equirect(fore, eq)) == 0  # the reference's texel, by value
    g.close()


def canopy_vs_fp64(p, ipdm):
    """canopyVS (CanopyScene.cpp:73-160) in float64 on the undisplaced vertices"""
    x, y, z = (p[..., i].astype(np.float64) for i in range(3))

    def ipd(lat):
        return ipdm * np.exp(-np.exp(25 * (0.17 - 0.5 - lat / math.pi)) - np.exp(25 * (0.17 - 0.5 + lat / math.pi)))

    def err(d):
        return (x * x + y * y) - (ipd(np.arctan(z / d)) / 2) ** 2 - d * d

    d0 = np.sqrt((x * x + y * y) - ipd(np.arctan(z / np.sqrt(x * x + y * y))) ** 2)
    for _ in range(2):
        d1 = (1 + 1e-3) * d0
        e0, e1 = err(d0), err(d1)
        d0 = d0 - e0 / ((e1 - e0) / (d1 - d0))
    k = -d0 / (ipd(np.arctan(z / d0)) / 2)
    det = 1 + k * k
    ex, ey = (x + k * y) / det, (y - k * x) / det
    return np.stack([x - ex, y - ey, z], axis=-1)


ULP_BOUND = 2  # measured on MI355X: 0.52


def test_stereo_vertices_fp64(scene):
    """the device's displaced vertices are within ULP_BOUND float ulps (of the vertex's largest coordinate) of an fp64
    evaluation of canopyVS, for vertices more than 0.1 m from the z axis"""
    from facebook360_dep_amd import derp

    rig = scene["rig"]
    g = derp.Derp(rig["cameras"])
    g.render_upload(scene["truth"], bgra(scene["colors"]))
    worst = 0.0
    for s in range(N):
        mono = g.render_vertices(s, (RES, RES), 0.0)[..., :3]
        for ipdm in (0.032, -0.032):
            dev = g.render_vertices(s, (RES, RES), ipdm)[..., :3]
            ref = canopy_vs_fp64(mono, ipdm)
            ok = np.hypot(mono[..., 0], mono[..., 1]) > 0.1
            scale = np.spacing(np.abs(ref).max(axis=-1).astype(np.float32)).astype(np.float64)
            ulps = (np.abs(dev.astype(np.float64) - ref).max(axis=-1) / scale)[ok]
            worst = max(worst, float(ulps.max()))
            assert np.abs(dev - mono).max() > 1e-3  # displaced
    print("stereo vertices: worst %.2f ulp vs fp64" % worst)
    assert worst <= ULP_BOUND
    g.close()


def test_geometry(scene):
    """eqrdisp from the rig centre against 1 / t of the analytic scene; stereo eyes differ at the equator, agree at
    the poles; ipd 0 through the API is eqrcolor"""
    import torch

    from facebook360_dep_amd import derp, synth

    rig = scene["rig"]
    H = 48
    W = 2 * H
    g = derp.Derp(rig["cameras"])
    g.render_upload(scene["truth"], bgra(scene["colors"]))
    disp = g.render_format("eqrdisp", derp.render_params(width=W, height=H))[..., 0]
    lon = (1 - (np.arange(W) + 0.5) / W) * 2 * math.pi
    lat = -((np.arange(H) + 0.5) / H - 0.5) * math.pi
    d = np.stack([np.cos(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.sin(lon)[None],
                  np.sin(lat)[:, None] * np.ones(W)[None]], axis=-1)
    t = synth.intersect((0, 0, 0), torch.tensor(d, dtype=torch.float64), (0, 0, 0))[0].numpy()
    want = 1 / t
    cov = ~np.isnan(disp)
    rel = np.abs(disp[cov] - want[cov]) / want[cov]
    print("eqrdisp: %.1f %% covered, median relative error %.4f" % (100 * cov.mean(), np.median(rel)))
    assert cov.mean() >= 0.95 and np.median(rel) <= 0.01
    p = derp.render_params(width=W, height=H)
    mono = g.render_format("eqrcolor", p)
    p.ipd = 0.032
    left = g.render(p)
    p.ipd = -0.032
    right = g.render(p)
    p.ipd = 0.0
    assert smr_check.float_equal(g.render(p), mono) == 0
    both = ~np.isnan(left[..., 0]) & ~np.isnan(right[..., 0])
    diff = np.where(both[..., None], np.abs(left - right), 0)[..., :3].max(axis=-1)
    band = H // 10
    equator, poles = diff[H // 2 - band:H // 2 + band], np.concatenate([diff[:band], diff[-band:]])
    print("stereo: eyes differ at %.1f %% of equator pixels; pole max difference %.2e" %
          (100 * (equator > 1e-3).mean(), poles.max()))
    assert (equator > 1e-3).mean() > 0.3
    assert np.median(poles) <= 1e-3
    g.close()


def test_cli_all_formats(built, tmp_path):
    """bin/SimpleMeshRenderer writes every format for two frames in png, jpg and exr; the files decode to the API's
    images (exr: float B, G, R as rendered; png: x65535 rounded, NaN -> 0; jpg: x255, lossy); --background and
    --background_equirect fill the uncovered pixels; --cameras restricts the render."""
    import subprocess

    from facebook360_dep_amd import derp, imageio
    from tests import smr_dataset
    from tests.test_smr_cli_flags import EXE

    root = str(tmp_path / "in")
    rig, data = smr_dataset.write(root, n=4, res=48, frames=(0, 1))
    W, H = 64, 32
    base = ["--rig=" + os.path.join(root, "rig.json"), "--color=" + os.path.join(root, "color"),
            "--disparity=" + os.path.join(root, "disparity"), "--first=000000", "--last=000001", "--width=%d" % W]

    def cli(out, *args):
        p = subprocess.run([EXE] + base + ["--output=" + out] + list(args), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr

    api = {}
    g = derp.Derp(rig["cameras"])
    p = derp.render_params(width=W, height=H)
    for fi in (0, 1):
        g.render_upload(data[fi]["truth"], bgra(data[fi]["color"][0]))
        api[fi] = {fmt: g.render_format(fmt, p) for fmt in derp.FORMATS}
    for fmt in derp.FORMATS:
        for ft in ("png", "jpg", "exr"):
            out = str(tmp_path / fmt / ft)
            cli(out, "--format=" + fmt, "--file_type=" + ft)
            for fi in (0, 1):
                want = api[fi][fmt][..., :3]
                path = os.path.join(out, "%06d.%s" % (fi, ft))
                if ft == "exr":
                    got = imageio.read_exr(path)
                    assert smr_check.float_equal(got, want) == 0, (fmt, fi)
                else:
                    scale = 65535.0 if ft == "png" else 255.0
                    w8 = np.clip(np.rint(np.nan_to_num(want, nan=0.0) * np.float32(scale)), 0, scale)
                    got = imageio.read_image(path).astype(np.float64)
                    assert got.shape == want.shape, (fmt, ft)
                    if ft == "jpg":  # the same 8-bit BGR through the library's JPEG encoder (quality 95)
                        ref = str(tmp_path / "ref.jpg")
                        imageio.write_jpeg(ref, w8.astype(np.uint8))
                        w8 = imageio.read_image(ref).astype(np.float64)
                    assert np.array_equal(got, w8), (fmt, ft, fi)
    # background / background_equirect fill the NaN pixels (4 cameras on an arc do not cover the sphere)
    fore = api[0]["eqrcolor"]
    assert np.isnan(fore[..., 3]).any()
    back = (np.random.default_rng(7).random((H, W, 3)) * 65535).astype(np.uint16)
    imageio.write_png16(str(tmp_path / "back.png"), back)
    cli(str(tmp_path / "bg"), "--format=eqrcolor", "--file_type=exr", "--background=" + str(tmp_path / "back.png"))
    backf = np.concatenate([back.astype(np.float32) / np.float32(65535), np.ones((H, W, 1), np.float32)], axis=2)
    got = imageio.read_exr(str(tmp_path / "bg" / "000000.exr"))
    assert not np.isnan(got).any()
    assert smr_check.float_equal(got, smr_check.alpha_blend(fore, backf)[..., :3]) == 0
    imageio.write_png16(str(tmp_path / "eq.png"), back[:16])
    cli(str(tmp_path / "bge"), "--format=eqrcolor", "--file_type=exr", "--background_equirect=" + str(tmp_path / "eq.png"))
    got = imageio.read_exr(str(tmp_path / "bge" / "000000.exr"))
    assert not np.isnan(got).any()
    assert smr_check.float_equal(got, smr_check.background_equirect(fore, backf[:16])[..., :3]) == 0
    # --cameras: only cam1 is loaded and rendered
    cli(str(tmp_path / "one"), "--format=eqrcolor", "--file_type=exr", "--cameras=cam1")
    g1 = derp.Derp([rig["cameras"][1]])
    g1.render_upload([data[0]["truth"][1]], bgra([data[0]["color"][0][1]]))
    one = g1.render_format("eqrcolor", p)
    assert smr_check.float_equal(imageio.read_exr(str(tmp_path / "one" / "000000.exr")), one[..., :3]) == 0
    assert np.isnan(one[..., 3]).sum() > np.isnan(fore[..., 3]).sum()
    g.close()
    g1.close()
