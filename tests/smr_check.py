"""Loader of tests/native/smr_checker.cpp, the CPU restatement of SimpleMeshRenderer's GPU stages (built with g++ into
a temporary directory, loaded through ctypes)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
KINDS = {"cube": 0, "equirect": 1, "snapshot": 2}
# the counters of chk_render_stats, in the order of smr_checker.cpp's enum Stat
STATS = ("tri_small", "tri_big", "pix_small", "pix_big", "displaced", "id_ties", "near_drops", "alpha_discards",
         "suspect", "mip_above0")


def lib():
    global _LIB
    if _LIB is None:
        so = os.path.join(tempfile.mkdtemp(prefix="smr_checker"), "libsmr_checker.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                               os.path.join(ROOT, "tests", "native", "smr_checker.cpp")])
        _LIB = C.CDLL(so)
    return _LIB


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[None if a is None else a.ctypes.data for a in arrs])


def _ints(v):
    return (C.c_int * len(v))(*v)


def render(cameras, disps, colors=None, include=None, verts=None, kind="equirect", width=64, height=32,
           position=(0, 0, 0), forward=(-1, 0, 0), up=(0, 0, 1), fov=90.0, alpha_blend=True, disparity_color=False,
           weight="svd", zero_nans=False, stats=None):
    """The checker's image: the same shapes as derp.Derp.render. `stats`: a dict that receives the counters STATS of
    this call, summed over its canopies and faces."""
    from oracle import oracle_lib as O

    n = len(cameras)
    cams = (O.CameraJson * n)(*[O.camera_json(c) for c in cameras])
    disps = [np.ascontiguousarray(d, dtype=np.float32) for d in disps]
    cols = [None] * n if colors is None else [np.ascontiguousarray(c, dtype=np.float32) for c in colors]
    vs = None if verts is None else [np.ascontiguousarray(v, dtype=np.float32) for v in verts]
    inc = None if include is None else np.ascontiguousarray(include, dtype=np.uint8)
    k = KINDS[kind]
    h = height
    w = {0: h, 1: 2 * h, 2: width}[k]
    out = np.zeros((6 * h if k == 0 else h, w, 4), dtype=np.float32)
    dbl = lambda v: (C.c_double * 3)(*map(float, v))  # noqa: E731
    assert lib().chk_num_stats() == len(STATS)
    counters = (C.c_uint64 * len(STATS))()
    lib().chk_render_stats(
        cams, n, None if inc is None else inc.ctypes.data_as(C.c_void_p), _ptrs(cols),
        _ints([0 if c is None else c.shape[1] for c in cols]), _ints([0 if c is None else c.shape[0] for c in cols]),
        _ptrs(disps), _ints([d.shape[1] for d in disps]), _ints([d.shape[0] for d in disps]),
        None if vs is None else _ptrs(vs), k, width, height, dbl(position), dbl(forward), dbl(up), C.c_double(fov),
        int(alpha_blend), int(disparity_color), int(weight == "minor"), int(zero_nans),
        out.ctypes.data_as(C.c_void_p), None if stats is None else counters)
    if stats is not None:
        stats.update(zip(STATS, (int(v) for v in counters)))
    return out


def equirect(cube_gl):
    """seamless cube [6, E, E, 4] (GL rows) -> equirect [E, 2 E, 4]"""
    cube_gl = np.ascontiguousarray(cube_gl, dtype=np.float32)
    E = cube_gl.shape[1]
    out = np.zeros((E, 2 * E, 4), dtype=np.float32)
    lib().chk_equirect(cube_gl.ctypes.data_as(C.c_void_p), E, out.ctypes.data_as(C.c_void_p))
    return out


def alpha_blend(fore, back):
    out = np.ascontiguousarray(fore, dtype=np.float32).copy()
    back = np.ascontiguousarray(back, dtype=np.float32)
    assert out.shape == back.shape
    lib().chk_alpha_blend(out.ctypes.data_as(C.c_void_p), back.ctypes.data_as(C.c_void_p), C.c_size_t(out.size // 4))
    return out


def background_equirect(fore, equi, position=(0, 0, 0), forward=(-1, 0, 0), up=(0, 0, 1), fov=90.0, stats=None):
    """backgroundEquirect of fore [h, w, 4] over the equirect equi [eh, ew, 4]; stats["clamped"]: the pixels whose
    texel the clamp to the image decided"""
    out = np.ascontiguousarray(fore, dtype=np.float32).copy()
    equi = np.ascontiguousarray(equi, dtype=np.float32)
    dbl = lambda v: (C.c_double * 3)(*map(float, v))  # noqa: E731
    clamped = C.c_uint64(0)
    lib().chk_background_equirect(out.ctypes.data_as(C.c_void_p), out.shape[1], out.shape[0],
                                  equi.ctypes.data_as(C.c_void_p), equi.shape[1], equi.shape[0], dbl(position),
                                  dbl(forward), dbl(up), C.c_double(fov), C.byref(clamped))
    if stats is not None:
        stats["clamped"] = int(clamped.value)
    return out


def float_equal(a, b):
    """number of elements that differ, NaN == NaN"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return int((~same).sum())
