"""The scenes, cameras and textures the RigSimulator tests share (CPU and GPU): small on purpose. Every scene is built
twice after srand(1), once by the library (derp.SimScene) and once by the restatement (tests/sim_ref.py)."""
import numpy as np

from tests import sim_ref as R

W, H = 24, 16  # neither square nor a multiple of a wave or a tile

SCENES = ["empty", "triangle", "four", "cubes", "icosa12", "ground"]

FOUR = [  # four triangles around the -z axis: fewer than splitK, so the root is a leaf
    ((-2, -2, -10), (2, -2, -10), (0, 2, -10), (1, 0, 0)),
    ((-2, -2, -12), (2, -2, -12), (0, 2, -12), (0, 1, 0)),
    ((0, -1, -8), (1, 1, -8), (-1, 1, -8), (0, 0, 1)),
    ((3, 0, -9), (4, 0, -9), (3, 1, -11), (1, 1, 0)),
]


def build_lib(name):
    from facebook360_dep_amd import derp

    R.srand(1)
    s = derp.SimScene()
    if name == "empty":
        s.icosahedrons(0)
    elif name == "triangle":
        s.icosahedrons(0, red_triangle=True)
    elif name == "four":
        for t in FOUR:
            s.add_triangle(*t)
    elif name == "cubes":
        s.cubes()
    elif name == "icosa12":
        s.icosahedrons(12)
    elif name == "ground":
        s.ground_plane(1.70)
    else:
        raise KeyError(name)
    s.build_bvh()
    out = s.arrays()
    s.close()
    return out


def build_ref(name):
    R.srand(1)
    s = R.Scene()
    if name == "triangle":
        R.make_icosahedron_scene(s, 0, red_triangle=True)
    elif name == "four":
        for t in FOUR:
            s.add(*t)
    elif name == "cubes":
        R.make_cubes_scene(s)
    elif name == "icosa12":
        R.make_icosahedron_scene(s, 12)
    elif name == "ground":
        R.make_ground_plane_scene(s, 1.70)
    elif name != "empty":
        raise KeyError(name)
    return R.make_bvh(s)


_ref_cache = {}


def ref_scene(name):
    """The restatement's scene, computed once and shared (never modified by the tests)."""
    if name not in _ref_cache:
        _ref_cache[name] = build_ref(name)
    return _ref_cache[name]


def _cam(cam_id, cam_type, origin, forward, up, focal, **extra):
    f, u = np.asarray(forward, float), np.asarray(up, float)
    c = dict(version=1, id=cam_id, type=cam_type, origin=list(map(float, origin)), forward=list(f), up=list(u),
             right=list(np.cross(f, u)), resolution=[float(W), float(H)], focal=[float(focal), float(focal)])
    c.update(extra)
    return c


CAMERAS = {
    # rectilinear, looking down -z past both cubes
    "rect_z": _cam("rect_z", "RECTILINEAR", (2.5, 1.0, 0.0), (0, 0, -1), (0, 1, 0), 60.0),
    # rectilinear at the origin looking along +x: the red triangle, and inside the icosahedron scene's root sphere
    "rect_x": _cam("rect_x", "RECTILINEAR", (0.0, 0.0, 0.0), (1, 0, 0), (0, 0, 1), 60.0, principal=[11.25, 8.5]),
    # wide rectilinear at the origin (inside the icosahedron scene's root sphere), looking along -y
    "rect_wide": _cam("rect_wide", "RECTILINEAR", (0.0, 0.0, 0.0), (0, -1, 0), (0, 0, 1), 9.0),
    # f-theta whose fov leaves the corners outside the image circle (radius 8 * 1.2 = 9.6 px), looking along +y
    "ftheta": _cam("ftheta", "FTHETA", (0.3, -0.2, 0.1), (0, 1, 0), (0, 0, 1), 8.0, fov=1.2, distortion=[0.01, -0.002, 0.0]),
}

CAMERA_CASES = [  # (scene, camera, aas, marble, ceiling)
    ("cubes", "rect_z", 1, False, False),
    ("cubes", "rect_z", 2, False, False),
    ("cubes", "rect_z", 3, False, False),
    ("icosa12", "ftheta", 1, True, False),
    ("icosa12", "ftheta", 2, True, False),
    ("icosa12", "rect_wide", 3, True, False),
    ("ground", "ftheta", 2, False, True),
    ("ground", "rect_x", 1, False, True),
    ("empty", "rect_z", 2, False, False),
    ("triangle", "rect_x", 1, False, False),
    ("four", "rect_z", 3, True, False),
]
EQUIRECT_CASES = [(16, 8, False, 2), (16, 8, True, 1), (10, 6, False, 3), (10, 6, True, 1)]  # (w, h, stereo, aas)

CEILING = dict(ceiling_position=3.0, ceiling_width=40.0, ceiling_depth=30.0)


def skybox():
    return np.random.default_rng(7).integers(0, 256, size=(5, 7, 3), dtype=np.uint8)  # 7 x 5: % cols and the pole clamp


def ceiling_image():
    return np.random.default_rng(8).integers(0, 256, size=(3, 4, 3), dtype=np.uint8)


def oracle_rays(cam, aas):
    """(origin, direction, outside) of renderCamera's rays from the oracle's camera model: float32 [h*aas, w*aas, 3]."""
    from oracle import oracle_lib as O

    rig = O.Rig([cam])
    hh, ww = H * aas, W * aas
    xs = ((np.arange(ww, dtype=np.float32) + np.float32(0.5)) / np.float32(aas)).astype(np.float64)
    ys = ((np.arange(hh, dtype=np.float32) + np.float32(0.5)) / np.float32(aas)).astype(np.float64)
    pix = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
    pos = np.asarray(cam["origin"], np.float64)
    d = (rig.rig(0, pix, 1.0) - pos[None, :]).astype(np.float32).reshape(hh, ww, 3)
    outside = np.array([rig.is_outside_image_circle(0, px, py) for px, py in pix]).reshape(hh, ww)
    o = np.broadcast_to(pos.astype(np.float32), (hh, ww, 3)).copy()
    o[outside] = 0
    d[outside] = 0
    return o, d, outside


def trace_kwargs(marble, ceiling):
    kw = dict(marble=marble, marble_scale=0.1)
    if ceiling:
        kw.update(CEILING, ceiling=ceiling_image())
    return kw
