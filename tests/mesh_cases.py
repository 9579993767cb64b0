"""Named inputs at the size, tear, content and strictness edges of the camera-mesh group (derp_mesh_build / _setup /
_simplify / _simplify_parallel) for tests/test_mesh_cases.py, tests/test_mesh_simplifier.py and
tests/test_gpu_mesh_limits.py. Every input is built deterministically; the restatement's result of a case
(tests/mesh_ref.py, tests/mesh_parallel_ref.py) is computed once and kept. Nothing here touches the GPU or the library."""
import json
import os
import time

import numpy as np

from tests import mesh_parallel_ref as P
from tests import mesh_ref as R

F32 = np.float32
BLOCK = 256  # threads per block of the mesh kernels: pixel 255 ends block 0, pixel 256 begins block 1


# ---------------------------------------------------------------- cameras
_cams = {}


def cameras(which):
    """"synth": synth.make_rig(2, 64) (64 x 64); "real": the first two cameras of tests/golden/ref_test_rig.json
    (3360 x 2160, focal x = -focal y): resx / W and resy / H differ. The meshes are camera 0's."""
    if which not in _cams:
        if which == "synth":
            from facebook360_dep_amd import synth

            _cams[which] = synth.make_rig(2, 64)["cameras"]
        else:
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_test_rig.json")) as f:
                _cams[which] = json.load(f)["cameras"][:2]
    return _cams[which]


def camera(which):
    return cameras(which)[0]


# ---------------------------------------------------------------- disparity maps
# (w, h) -> what the size is for
SIZES = [(1, 1), (9, 1), (1, 9),            # no quads
         (2, 2), (3, 2), (2, 3),            # one or two quads
         (16, 16), (64, 4), (128, 2),       # exactly 256 pixels: one full block
         (255, 2), (256, 2), (257, 2),      # row 1 starts in, at and after the block boundary
         (2, 129),                          # two columns, 258 pixels
         (63, 5), (65, 5),                  # a row one short of and one past a wave
         (1025, 256)]                       # 1025 blocks: the strided path of the block scan (build only)
SETUP_SIZES = [s for s in SIZES if s != (1025, 256)]


def ramp(w, h):
    """a tilted plane in depth, neighbouring ratios near 1: no tear, no hole"""
    ys, xs = np.mgrid[0:h, 0:w]
    return (1.0 / (2.0 + 0.01 * xs + 0.007 * ys)).astype(F32)


def boundary_pixels(w, h):
    """the last pixel of block 0 and the first of block 1, as (x, y), where the map has them"""
    return [(p % w, p // w) for p in (BLOCK - 1, BLOCK) if p < w * h]


def edge_disparity(w, h):
    """a ramp whose neighbouring ratios stay above 0.95, in bands of five columns of which every other is 20 % farther
    (a step past the tear ratio at every band edge), and one NaN pixel that is no corner. Every quad with the last pixel
    of block 0 or the first of block 1 as a corner is left whole: no step, no NaN in the 3 x 3 pixels around either.
    Maps of fewer than 16 pixels are the ramp alone."""
    ys, xs = np.mgrid[0:h, 0:w]
    depth = 2.0 + 0.01 * xs + 0.007 * ys + 0.002 * np.sin(xs * 0.9) * np.cos(ys * 0.8)
    if w * h < 16:
        return (1.0 / depth).astype(F32)
    factor = 1.0 + 0.2 * ((xs // 5) % 2)
    guarded = np.zeros((h, w), bool)
    for x, y in boundary_pixels(w, h):
        guarded[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    factor[guarded] = 1.1
    disp = (1.0 / (depth * factor)).astype(F32)
    near = np.zeros((h, w), bool)  # the guarded pixels and their neighbours: a NaN here would cost a guarded quad
    for y, x in zip(*np.nonzero(guarded)):
        near[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    corners = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)}
    start = (h // 2) * w + w // 3
    for p in list(range(start, w * h)) + list(range(start)):
        if (p % w, p // w) not in corners and not near[p // w, p % w]:
            disp[p // w, p % w] = np.nan
            break
    return disp


SPECIAL_VALUES = [0.25, 0.0, -0.0, np.inf, -np.inf, np.nan, -0.25, 1e-45, 3e38, 0.26]


def specials_24():
    """24 x 24 of SPECIAL_VALUES, the first at about 60 % of the pixels. 1e-45 is the smallest subnormal float (1 / d
    overflows to +inf), 1 / 3e38 is a subnormal float (flushed to zero, z would be infinite instead of about 1e38 focal)"""
    rng = np.random.default_rng(3)
    pick = rng.choice(len(SPECIAL_VALUES), size=(24, 24), p=[0.6] + [0.4 / 9] * 9)
    return np.array(SPECIAL_VALUES, dtype=F32)[pick]


def flat_12():
    """one disparity everywhere: few distinct edge costs, of both signs and zero: the (cost, face * 3 + edge) tie order"""
    return np.full((12, 12), 0.25, dtype=F32)


def tear_exact():
    """z ratios of exactly 0.5"""
    return np.array([[1.0, 0.5], [0.5, 1.0]], dtype=F32)


def single_triangle():
    """2 x 2 torn to one triangle: the bottom right corner is twice as far"""
    return np.array([[0.5, 0.5], [0.5, 0.25]], dtype=F32)


HALF_BELOW = float(np.nextafter(F32(0.5), F32(0)))
TEAR_EXACT_RATIOS = {"0.5": 0.5, "below_0.5": HALF_BELOW, "0": 0.0, "1": 1.0, "1.5": 1.5, "nan": float("nan")}
TEAR_RATIOS_70 = [0.5, 0.9, 0.97, 0.999, 1.0]
DEPTH_SCALES = {0.25: (18, 9), 0.3: (21, 11), 1 / 3: (23, 12), 0.999: (70, 37), 0.02: (1, 1), 1.0: (70, 37), 2.0: (70, 37)}


def _masks():
    rng = np.random.default_rng(11)
    return {
        "own_size": (rng.random((37, 70)) > 0.15).astype(np.uint8),
        "one": np.ones((1, 1), np.uint8),
        "zero": np.zeros((1, 1), np.uint8),
        "larger": rng.choice(np.array([0, 2, 255], np.uint8), size=(74, 140), p=[0.2, 0.4, 0.4]),
    }


# name -> (camera, disparity map, keyword arguments shared by mesh_ref.build and Derp.mesh_build)
BUILD_CASES = {}
for _w, _h in SIZES:
    BUILD_CASES["size_%dx%d" % (_w, _h)] = ("synth", lambda w=_w, h=_h: edge_disparity(w, h), {})
BUILD_CASES["single_triangle"] = ("synth", single_triangle, {})
BUILD_CASES["specials_24"] = ("synth", specials_24, {})
BUILD_CASES["flat_12"] = ("synth", flat_12, {})
BUILD_CASES["ramp_3x3"] = ("synth", lambda: ramp(3, 3), {})
BUILD_CASES["depth_48x32"] = ("synth", lambda: R.synthetic_depth(48, 32), {})
BUILD_CASES["depth_40x2"] = ("synth", lambda: R.synthetic_depth(40, 2), {})
for _name, _t in TEAR_EXACT_RATIOS.items():
    BUILD_CASES["tear_exact_" + _name] = ("synth", tear_exact, {"tear_ratio": _t})
for _t in TEAR_RATIOS_70:
    BUILD_CASES["tear_70x37_%g" % _t] = ("synth", lambda: R.gpu_disparity(70, 37), {"tear_ratio": _t})
for _s in DEPTH_SCALES:
    BUILD_CASES["scale_%.3g" % _s] = ("synth", lambda: R.gpu_disparity(70, 37), {"depth_scale": _s})
BUILD_CASES["scale_ties_5x7"] = ("synth", lambda: ramp(5, 7), {"depth_scale": 0.5})  # half to even: 5 -> 2, 7 -> 4
for _name in ("own_size", "one", "zero", "larger"):
    BUILD_CASES["mask_" + _name] = ("synth", lambda: R.gpu_disparity(70, 37), {"mask": _name})
BUILD_CASES["mask_and_scale"] = ("synth", lambda: R.gpu_disparity(70, 37), {"mask": "own_size", "depth_scale": 0.5})
BUILD_CASES["real_84x54"] = ("real", lambda: R.gpu_disparity(84, 54), {})
BUILD_CASES["real_50x38"] = ("real", lambda: R.gpu_disparity(50, 38), {})
BUILD_CASES["real_rescaled"] = ("real", lambda: R.gpu_disparity(84, 54), {"resolution": (840, 540)})

SIZE_NAMES = ["size_%dx%d" % s for s in SIZES]
SETUP_NAMES = ["size_%dx%d" % s for s in SETUP_SIZES] + ["specials_24", "flat_12"]

_built = {}


def build_case(name):
    """-> dict(camera = "synth" / "real", disparity, args = the keyword arguments, want = mesh_ref.build's result)"""
    if name not in _built:
        which, disparity, args = BUILD_CASES[name]
        args = dict(args)
        if "mask" in args:
            args["mask"] = _masks()[args["mask"]]
        if "resolution" in args:
            args["resolution"] = R.resize_rig_resolution(camera(which), *args["resolution"])
            assert args["resolution"] is not None
        disparity = disparity()
        _built[name] = dict(camera=which, disparity=disparity, args=args, want=R.build(camera(which), disparity, **args))
    return _built[name]


_setups = {}


def setup_case(name, equi_error):
    """mesh_ref.setup of a build case -> (face planes, edge costs, vertex quadrics)"""
    if (name, equi_error) not in _setups:
        m = build_case(name)["want"]
        _setups[(name, equi_error)] = R.setup(m["V"], m["F"], equi_error=equi_error)
    return _setups[(name, equi_error)]


# ---------------------------------------------------------------- simplifier cases
# name -> (build case, budget = a number or a function of the built mesh's faces, strictness, remove_boundary_edges)
PARALLEL_CASES = {
    "flat_s0": ("flat_12", 40, 0.0, False),
    "flat_s0.2": ("flat_12", 40, 0.2, False),
    "flat_s1": ("flat_12", 40, 1.0, False),
    "depth_s1": ("depth_48x32", 600, 1.0, False),
    "depth_s0.5": ("depth_48x32", 600, 0.5, False),
    "specials_s0.2": ("specials_24", 50, 0.2, False),
    "specials_s1": ("specials_24", 50, 1.0, False),
    # (two rows: every vertex lies on the boundary, so only boundary edges can go)
    "half_256x2": ("size_256x2", lambda nf: nf // 2, 0.2, True),
    "half_257x2": ("size_257x2", lambda nf: nf // 2, 0.2, True),
    # ... and with the boundary kept no edge is feasible: no pass, at widths that straddle the block
    "half_256x2_kept": ("size_256x2", lambda nf: nf // 2, 0.2, False),
    "half_257x2_kept": ("size_257x2", lambda nf: nf // 2, 0.2, False),
    "half_16x16": ("size_16x16", lambda nf: nf // 2, 0.2, False),
    "triangle_to_nothing": ("single_triangle", 0, 0.2, True),
    "ramp_3x3_inner": ("ramp_3x3", 0, 1.0, False),
    "ramp_3x3_boundary": ("ramp_3x3", 0, 1.0, True),
    "budget_is_faces": ("size_16x16", lambda nf: nf, 0.2, False),
    "budget_one_less": ("size_16x16", lambda nf: nf - 1, 0.2, False),
    "strip_boundary": ("depth_40x2", 10, 0.5, True),
}
SEQUENTIAL_CASES = {
    "flat_s0": ("flat_12", 40, 0.0, False),
    "flat_s1": ("flat_12", 40, 1.0, False),
    "depth_s1": ("depth_48x32", 600, 1.0, False),
    "quad_to_nothing": ("size_2x2", 0, 0.2, False),
    "ramp_3x3_to_nothing": ("ramp_3x3", 0, 0.2, False),
    # with the boundary free to go, the last collapse leaves no face and no cost for the next threshold
    "triangle_to_nothing": ("single_triangle", 0, 0.2, True),
    "quad_to_nothing_boundary": ("size_2x2", 0, 0.2, True),
    "ramp_3x3_boundary": ("ramp_3x3", 0, 1.0, True),
}
# the committed runs at strictness 0.2, for the cases above that exist to differ from them
BASELINES = {
    ("parallel", "depth_s0.2"): ("depth_48x32", 600, 0.2, False),
    ("sequential", "flat_s0.2"): ("flat_12", 40, 0.2, False),
    ("sequential", "depth_s0.2"): ("depth_48x32", 600, 0.2, False),
}
_simplified = {}


def simplify_case(kind, name):
    """kind = "parallel" / "sequential" -> dict(build = the build case's name, V, F = the built mesh, budget,
    strictness, rbe, out = (V', F', stats), log = the parallel restatement's per-pass counters, seconds)"""
    if (kind, name) not in _simplified:
        table = PARALLEL_CASES if kind == "parallel" else SEQUENTIAL_CASES
        build, budget, strictness, rbe = BASELINES[(kind, name)] if (kind, name) in BASELINES else table[name]
        m = build_case(build)["want"]
        if callable(budget):
            budget = budget(len(m["F"]))
        t0 = time.perf_counter()
        if kind == "parallel":
            s = P.ParallelSimplifier(m["V"], m["F"], R.setup(m["V"], m["F"], True), True)
        else:
            s = R.Simplifier(m["V"], m["F"], R.setup(m["V"], m["F"], True), True)
        stats = s.run(budget, strictness, rbe)
        v, f = s.final_mesh()
        _simplified[(kind, name)] = dict(build=build, V=m["V"], F=m["F"], budget=budget, strictness=strictness, rbe=rbe,
                                         out=(v, f, stats), log=getattr(s, "log", None), seconds=time.perf_counter() - t0)
    return _simplified[(kind, name)]


# ---------------------------------------------------------------- the comparison rule of the limits tests
def differing(got, want):
    """how many values differ: floats as bit patterns, except that NaN equals NaN whatever its sign and payload (x86
    and the GPU make different default NaNs); +0 and -0 differ. Integers as integers. Shapes must be equal."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        return int((got != want).sum())
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    same = (np.ascontiguousarray(got).view(bits) == np.ascontiguousarray(want).view(bits)) | (np.isnan(got) & np.isnan(want))
    return int((~same).sum())
