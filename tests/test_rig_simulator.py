"""RigSimulator without a GPU: --helpxml against the flag table pinned from the reference's source
(tests/golden/ref_flags_rig_simulator.json, written by gen_ref_pins_sim.py), every refusal by message and exit status,
the scene builders and the sphere tree against the numpy restatement (tests/sim_ref.py) bit for bit after srand(1), the
generated rigs through the rig parser and the oracle's camera, the restatement's own share of sky rays in the band where
device and glibc roundings may pick different texels, and the scene unit under the sanitizers in a stand-alone program."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import sim_cases as K
from tests import sim_ref as R
from tests.test_ref_pins import _cxx_literal, _helpxml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "facebook360_dep_amd")
BIN = os.path.join(PKG, "bin")


def test_flag_table_matches_the_reference(built):
    with open(os.path.join(ROOT, "tests", "golden", "ref_flags_rig_simulator.json")) as f:
        ref = json.load(f)["RigSimulator"]["flags"]
    mine = _helpxml("RigSimulator")
    assert len(ref) == 40
    type_of = {"string": "string", "integer": "int32", "float": "double", "boolean": "bool"}
    for fl in ref:
        name = fl["name"]
        got = mine[name]
        assert got["type"] == type_of[fl["type"]], name
        if fl["type"] == "string":
            assert got["default"] == _cxx_literal(fl["default"]), name
        elif fl["type"] == "boolean":
            assert (got["default"] == "true") == bool(fl["default"]), name
        else:
            assert float(got["default"]) == float(fl["default"]), name
        assert got["meaning"] == _cxx_literal(fl["descr"]), (name, got["meaning"])
    names = {fl["name"] for fl in ref}
    for name, got in mine.items():
        assert name in names or "[extension" in got["meaning"] or got["meaning"].startswith("glog:"), name


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from facebook360_dep_amd import imageio

    root = tmp_path_factory.mktemp("rig_simulator")
    imageio.write_png8(str(root / "sky.png"), K.skybox())
    (root / "broken.png").write_bytes(b"\x89PNG\r\n\x1a\nnot a png at all")
    (root / "rig.json").write_text(json.dumps({"cameras": list(K.CAMERAS.values())}))
    return root


def run(*args):
    p = subprocess.run([os.path.join(BIN, "RigSimulator")] + list(args), capture_output=True, text=True, timeout=60)
    return p.returncode, p.stderr


@pytest.mark.parametrize("args,message", [
    (["--mode="], "mode"),
    (["--mode=fisheye_ring"], "unexpected mode: fisheye_ring"),
    (["--scene=teapot"], "unexpected scene: teapot"),
    (["--mode=mono_eqr", "--dest_mono={root}/m.png"], "dest_mono_depth"),
    (["--mode=mono_eqr", "--dest_mono_depth={root}/m.png"], "dest_mono"),
    (["--mode=stereo_eqr", "--dest_left={root}/l.png", "--dest_right={root}/r.png"], "dest_stereo"),
    (["--mode=rig_from_json", "--rig_out={root}/o.json"], "rig_in"),
    (["--mode=rig_from_json", "--rig_in={root}/missing.json", "--rig_out={root}/o.json"], "could not read JSON file"),
    (["--rig_out=", "--dest_cam_images="], "nothing to write"),
    (["--skybox_path={root}/missing.png"], "failed to load image"),
    (["--skybox_path={root}/broken.png"], "failed to load image"),
    (["--ceiling_path={root}/missing.png"], "failed to load image"),
    (["--skybox_path="], "skybox_path"),
    (["--anti_alias_supersample=0"], "anti_alias_supersample"),
    (["--bogus_flag=1"], "bogus_flag"),
])
def test_refusals_need_no_device(built, tree, args, message):
    base = ["--mode=pinhole_ring", "--skybox_path=%s/sky.png" % tree, "--scene=cube", "--dest_cam_images=%s/out" % tree,
            "--rig_out=%s/out.json" % tree]
    rc, err = run(*(base + [a.format(root=tree) for a in args]))
    assert rc != 0 and message in err, (rc, err[-600:])
    assert "derp_sim_create" not in err  # refused before any device was asked for
    assert not (tree / "out").exists() and not (tree / "out.json").exists()


# ---------------------------------------------------------------- scenes and sphere trees, bit for bit
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", K.SCENES)
def test_scene_and_tree_equal_the_restatement(built, name):
    tris, nodes, leaf = K.build_lib(name)
    ref = K.ref_scene(name)
    assert len(tris) == len(ref.tri) == {"empty": 0, "triangle": 1, "four": 4, "cubes": 24, "icosa12": 240, "ground": 2}[name]
    for field in ("v0", "v1", "v2", "e1", "e2", "normal", "color"):
        assert np.array_equal(_bits(tris[field]).reshape(-1, 3), _bits(ref.field(field))), field
    assert len(nodes) == len(ref.nodes)
    for i, nd in enumerate(ref.nodes):
        assert np.array_equal(_bits(nodes["center"][i]), _bits(nd["center"])), ("center", i)
        assert _bits(nodes["radius"][i:i + 1])[0] == _bits([nd["radius"]])[0], ("radius", i)
        for key in ("skip", "first", "count", "n_children"):  # children order = node order; leaf ranges; skip links
            assert int(nodes[key][i]) == nd[key], (key, i)
    assert list(leaf) == ref.leaf  # leaf contents, in order
    # the shapes of the trees the issue names
    inner = [nd for nd in ref.nodes if nd["count"] < 0]
    if name in ("empty", "triangle", "four", "ground"):
        assert len(ref.nodes) == 1 and ref.nodes[0]["count"] == len(ref.tri)
    if name == "empty":
        assert np.isnan(nodes["center"][0]).all()  # the centre of mass of no triangles
    if name == "cubes":
        assert len(inner) == 1 and len(ref.nodes) == 6  # exactly one split
    if name == "icosa12":
        assert len(inner) >= 2 and ref.nodes[1]["count"] < 0 or any(nd["count"] < 0 for nd in ref.nodes[1:])
    assert sorted(leaf) == list(range(len(tris)))  # every triangle in exactly one leaf


def test_perlin_table_is_the_permutation(built):
    from facebook360_dep_amd import derp

    p = derp.sim_perlin_table()
    assert sorted(p[:256]) == list(range(256)) and np.array_equal(p[:256], p[256:])
    assert np.array_equal(p.astype(np.int64), R.PERLIN512)


def test_noise_equals_the_restatement(built):
    from facebook360_dep_amd import derp

    img = np.random.default_rng(3).uniform(-5, 260, size=(5, 7, 3)).astype(np.float32)
    R.srand(5)
    got = derp.sim_noise(img.copy(), 12.5)
    R.srand(5)
    a = np.float32(12.5)
    want = img.copy().reshape(-1)
    for i in range(want.size):
        v = want[i] + np.float32(2.0) * a * (R.randf0to1() - np.float32(0.5))
        want[i] = min(max(v, np.float32(0)), np.float32(255))
    assert np.array_equal(got.reshape(-1), want)
    assert np.array_equal(derp.sim_noise(img.copy(), 0.0), img)


def test_host_tracer_equals_the_restatement(built):
    """derp_sim_trace_host (the CPU baseline of tools/sim_timing.py) on the cube scene, through the sky-free part."""
    from facebook360_dep_amd import derp

    R.srand(1)
    s = derp.SimScene().cubes().build_bvh()
    o, d, _ = K.oracle_rays(K.CAMERAS["rect_z"], 2)
    rays = np.concatenate([o.reshape(-1, 3), d.reshape(-1, 3)], axis=1)
    got = s.trace_host(rays)
    want = R.trace(K.ref_scene("cubes"), o, d, K.skybox())
    geo = want["hit"] >= 0
    assert geo.sum() > 50
    assert np.array_equal(_bits(got[geo, 3]), _bits(want["distance"][geo]))
    assert np.array_equal(_bits(np.float32(255) * got[geo, :3]), _bits(want["color"][geo]))
    assert (got[~geo, 3] == R.FLT_MAX).all()


# ---------------------------------------------------------------- generated rigs
@pytest.mark.parametrize("mode,count", [("pinhole_ring", 5), ("ftheta_ring", 4), ("dodecahedron", 12), ("icosahedron", 20),
                                        ("rig_from_json", 4)])
def test_generated_rigs_load_and_are_right_handed(built, tree, mode, count):
    from oracle import oracle_lib as O

    from facebook360_dep_amd import derp

    out = tree / ("rig_%s.json" % mode)
    rc, err = run("--mode=" + mode, "--skybox_path=%s/sky.png" % tree, "--scene=cube", "--rig_out=%s" % out,
                  "--rig_in=%s/rig.json" % tree, "--num_cams_in_ring=%d" % (count - 1 if mode == "ftheta_ring" else count))
    assert rc == 0, err[-600:]
    cams = json.load(open(out))["cameras"]
    assert len(cams) == count
    assert [c["id"] for c in cams] == ([str(i) for i in range(count)] if mode != "rig_from_json" else list(K.CAMERAS))
    rig = O.Rig(cams)
    for i, c in enumerate(cams):
        derp.camera_desc(c)  # the library's own rig parser takes it
        assert rig.valid(i), c["id"]
        r, u, f = (np.asarray(c[k]) for k in ("right", "up", "forward"))
        assert np.dot(np.cross(r, u), f) < 0
        assert abs(np.linalg.norm(f) - 1) < 1e-6 and abs(np.dot(f, u)) < 1e-6
    if mode == "pinhole_ring":
        assert cams[0]["type"] == "RECTILINEAR" and cams[0]["group"] == "side camera"
        tan_half = np.tan(np.float32(np.float32(77.7) * np.float32(np.pi) / np.float32(180)) / np.float32(2))
        assert abs(cams[0]["focal"][0] - 256.0 / float(tan_half)) < 1e-6
        assert np.allclose(cams[1]["origin"], [0.218 * np.cos(-2 * np.pi / 5), 0.218 * np.sin(-2 * np.pi / 5), 0], atol=1e-7)
    if mode == "ftheta_ring":
        top = cams[-1]
        assert top["origin"] == [0, 0, 13] and top["forward"] == [0, 0, 1] and "group" not in top
        assert abs(top["focal"][0] - 500.0 / np.deg2rad(166.667)) < 1e-3
    if mode == "rig_from_json":
        assert cams[3]["fov"] == pytest.approx(1.2, abs=1e-9) and cams[1]["principal"] == [11.25, 8.5]


# ---------------------------------------------------------------- the sky band of the GPU comparison, restatement alone
@pytest.mark.parametrize("scene,cam,aas,marble,ceiling", K.CAMERA_CASES)
def test_sky_rays_near_a_texel_border_stay_under_the_cap(built, scene, cam, aas, marble, ceiling):
    """tests/test_gpu_rig_simulator.py lets a sky texel differ only where the restatement's sampleX / sampleY lies within
    4 float ulps of an integer, and allows at most 0.1 % of a case's sky rays there. With the oracle's rays (within an
    ulp of the device's) every chosen case must stay under that cap."""
    o, d, outside = K.oracle_rays(K.CAMERAS[cam], aas)
    res = R.trace(K.ref_scene(scene), o, d, K.skybox(), outside=outside, **K.trace_kwargs(marble, ceiling))
    sky = res["hit"] == -1
    band = sky & (R.near_integer(res["sample_x"]) | R.near_integer(res["sample_y"]))
    assert band.sum() <= 0.001 * sky.sum(), (int(band.sum()), int(sky.sum()))
    # the case shows what it is there for
    if scene != "empty":
        assert (res["hit"] >= 0).sum() > 0
    if ceiling and cam == "ftheta":
        assert (res["hit"] == -2).sum() > 0
    if cam == "ftheta":
        assert outside.sum() > 0 and (~outside).sum() > outside.sum()
    if scene == "empty":
        assert sky.all()


@pytest.mark.parametrize("w,h,stereo,aas", K.EQUIRECT_CASES)
def test_equirect_sky_band(built, w, h, stereo, aas):
    ol, orr, d = R.equirect_rays(w * aas, h * aas, stereo)
    for o in ([ol, orr] if stereo else [ol]):
        res = R.trace(K.ref_scene("icosa12"), o, d, K.skybox(), marble=True)
        sky = res["hit"] == -1
        band = sky & (R.near_integer(res["sample_x"]) | R.near_integer(res["sample_y"]))
        assert band.sum() <= 0.001 * sky.sum(), (int(band.sum()), int(sky.sum()))
        assert (res["hit"] >= 0).sum() > 0


# ---------------------------------------------------------------- the scene unit under the sanitizers, stand-alone
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim") / "sim_scene_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "sim_scene_main.cpp"),
                           os.path.join(PKG, "csrc", "derp_sim_scene.cpp")])
    return exe


@pytest.mark.parametrize("name", K.SCENES)
def test_scene_unit_under_sanitizers(built, harness, tmp_path, name):
    out = tmp_path / "scene.bin"
    p = subprocess.run([harness, name, str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    tris, nodes, leaf = K.build_lib(name)
    raw = out.read_bytes()
    n = np.frombuffer(raw, np.int32, 3)
    assert list(n) == [len(tris), len(nodes), len(leaf)]
    at = 12
    for arr in (tris, nodes, leaf):
        assert raw[at:at + arr.nbytes] == arr.tobytes()
        at += arr.nbytes
    assert len(raw) - at == 12 * 24 * 4 * 4
