"""Restatement of the reference's equirect scene mesh (source/conversion/CreateObjFromDisparityEquirect.cpp) for
tests/test_equirect_mesh_ref.py, tests/test_create_obj_cli.py and tests/test_gpu_equirect_mesh.py:
mesh_util::getVertexesEquirect, getTriangleMask fed the vertices' norms, getFaces with the horizontal seam,
addTextureCoordinatesEquirect, writeObj / writeMtl (source/render/MeshUtil.h), cv_util::loadImage<float> of a PNG, and
the tool's bilinear rule for --scale. The triangle mask, addTriangle, the simplifier and its
set-up are tests/mesh_ref.py's. Nothing in this file touches the GPU.

Implementation-defined, as in the product: the unqualified sin / cos of float arguments are the C library's double
functions (math.sin / math.cos here: the same libm), and Eigen's norm of a matrix row sums (x^2 + y^2) + z^2."""
import math
import os

import numpy as np

from tests import mesh_ref as R

F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------- MeshUtil.h:298-314
def angle_tables(w, h):
    """-> (cos theta [w], sin theta [w], sin phi [h], cos phi [h]) as f64: `float(x + 0.5) / float(width)`, `u * 2.0f *
    M_PI` and `v * M_PI` narrowed to float, then the double sin / cos of the floats"""
    theta = [F32(float(F32(F32(x + 0.5) / F32(w)) * F32(2.0)) * math.pi) for x in range(w)]
    phi = [F32(float(F32(F32(y + 0.5) / F32(h))) * math.pi) for y in range(h)]
    return (np.array([math.cos(float(t)) for t in theta]), np.array([math.sin(float(t)) for t in theta]),
            np.array([math.sin(float(p)) for p in phi]), np.array([math.cos(float(p)) for p in phi]))


def depths(disparity, max_depth):
    """`std::fmin(maxDepth, 1.0f / disparity(y, x))` in float: 0 and NaN give maxDepth, a negative disparity a negative
    depth (-0 gives -inf)"""
    with np.errstate(all="ignore"):
        return np.fmin(F32(max_depth), F32(1.0) / np.asarray(disparity, dtype=F32))


def vertices(disparity, max_depth=700.0):
    """getVertexesEquirect -> (V f64 [h * w, 3], norms f64 [h * w])"""
    h, w = np.asarray(disparity).shape
    ct, st, sp, cp = angle_tables(w, h)
    with np.errstate(all="ignore"):
        d = depths(disparity, max_depth).astype(F64)
        x = d * (sp[:, None] * ct[None, :])
        y = d * np.broadcast_to(cp[:, None], (h, w))
        z = d * (sp[:, None] * st[None, :])
        norm = np.sqrt((x * x + y * y) + z * z)
    return np.ascontiguousarray(np.stack([x, y, z], axis=2).reshape(-1, 3)), norm.reshape(-1)


def build(disparity, max_depth=700.0, tear_ratio=0.95):
    """getVertexesEquirect + getFaces(wrapHorizontally = true, isRigCoordinates = true) (:264-296): nothing is compacted.
    -> dict(V, F i32 [nf, 3], norms, grid = faces before the seam's, outcomes = {triangle mask: quads}, by_column =
    {quad column: set of outcomes}, w, h)"""
    h, w = np.asarray(disparity).shape
    V, norm = vertices(disparity, max_depth)
    tear = float(F32(tear_ratio))
    key = norm.tolist()
    faces, outcomes, by_column = [], {}, {}
    for y in range(h - 1):
        for x in range(w - 1):
            base = y * w + x
            m = R.triangle_mask(key[base], key[base + 1], key[base + w], key[base + w + 1], tear)
            outcomes[m] = outcomes.get(m, 0) + 1
            by_column.setdefault(x, set()).add(m)
            for t in range(4):
                if m >> t & 1:
                    faces.append(R._triangle(t, base, w))
    grid = len(faces)
    for y in range(h - 1):  # "Link last and first longitudes": after all grid faces, no tear test
        base = y * w
        faces.append((base + w, base, base + w - 1))
        faces.append((base + w - 1, base + 2 * w - 1, base + w))
    return dict(V=V, F=np.array(faces, dtype=np.int32).reshape(-1, 3), norms=norm, grid=grid, outcomes=outcomes,
                by_column=by_column, w=w, h=h)


# ---------------------------------------------------------------- MeshUtil.h:407-419
def texcoords(V):
    """addTextureCoordinatesEquirect -> st f64 [nv, 2]"""
    out = np.zeros((len(V), 2))
    for i, (x, y, z) in enumerate(np.asarray(V, dtype=F64).reshape(-1, 3).tolist()):
        xz = math.sqrt(x * x + z * z)
        out[i, 0] = math.atan2(-z, -x) * 0.5 / math.pi + 0.5
        out[i, 1] = -math.atan2(-y, xz) / math.pi + 0.5
    return out


# ---------------------------------------------------------------- writeObj / writeMtl (:91-144)
def obj_text(V, F, st=None, mtl=None):
    """writeObj of the fp64 vertices as they are (mesh_ref.obj_text is ConvertToBinary's, which reads float32 files
    back); st + mtl: the `vt` lines, `f a/a b/b c/c` and the material header"""
    assert (st is None) == (mtl is None), "texture coordinates and material go together"
    lines = [] if mtl is None else ["mtllib %s\nusemtl material\n" % mtl]
    for i, v in enumerate(np.asarray(V, dtype=F64).reshape(-1, 3).tolist()):
        lines.append("v %g %g %g\n" % tuple(v))
        if st is not None:
            lines.append("vt %g %g\n" % (float(st[i][0]), float(st[i][1])))
    for f in np.asarray(F).reshape(-1, 3).tolist():
        a, b, c = (int(i) + 1 for i in f)
        lines.append("f %d %d %d\n" % (a, b, c) if st is None else "f %d/%d %d/%d %d/%d\n" % (a, a, b, b, c, c))
    return "".join(lines)


def mtl_text(path_obj, path_color):
    """writeMtl -> (the .mtl file's text, its name as mtllib holds it)"""
    rel = os.path.relpath(os.path.realpath(path_color), os.path.realpath(os.path.dirname(path_obj) or "."))
    name = os.path.splitext(os.path.basename(path_obj))[0] + ".mtl"
    return "newmtl material\nillum 0\nKd 1 1 1\nmap_Kd %s\n" % rel, name


# ---------------------------------------------------------------- cv_util::loadImage<float> of a PNG
def load_float(img):
    """img = what imageio.write_png8 / write_png16 were given (u8 / u16, [h, w] or [h, w, 3 | 4] in BGR(A) order) ->
    f32 [h, w]: samples scaled by 1 / 255 or 1 / 65535 in float, colour reduced as b * 0.114f + g * 0.587f + r * 0.299f"""
    img = np.asarray(img)
    scale = F32(1.0) / F32(65535.0 if img.dtype == np.uint16 else 255.0)
    f = img.astype(F32) * scale
    if f.ndim == 2:
        return f
    return (f[..., 0] * F32(0.114) + f[..., 1] * F32(0.587)) + f[..., 2] * F32(0.299)


# ---------------------------------------------------------------- --scale < 1: the tool's bilinear rule
def _taps(ssize, dsize, scale):
    s = (np.arange(dsize, dtype=F32) + F32(0.5)) / F32(scale) - F32(0.5)
    f = np.floor(s)
    lo = np.clip(f.astype(np.int64), 0, ssize - 1)
    hi = np.clip(f.astype(np.int64) + 1, 0, ssize - 1)
    return lo, hi, (s - f).astype(F32)


def resize_bilinear(img, scale):
    """destination size nearbyint(size * scale); destination pixel d reads the source at (d + 0.5) / scale - 0.5 in float,
    between the two pixels around it, each clamped to the image: a * (1 - f) + b * f in float, along the rows first,
    then along the columns"""
    img = np.asarray(img, dtype=F32)
    h, w = img.shape
    dw, dh = int(np.rint(w * scale)), int(np.rint(h * scale))
    one = F32(1.0)
    with np.errstate(all="ignore"):
        lo, hi, f = _taps(w, dw, scale)
        rows = img[:, lo] * (one - f)[None, :] + img[:, hi] * f[None, :]
        lo, hi, f = _taps(h, dh, scale)
        return (rows[lo, :] * (one - f)[:, None] + rows[hi, :] * f[:, None]).astype(F32)


# ---------------------------------------------------------------- shared inputs
def sample_disparity(w, h):
    """mesh_ref.gpu_disparity's features where the size has room for them, and for every size: a much nearer and a much
    farther pixel, a zero, a NaN and a negative disparity, with torn and whole quads in the first and last quad columns"""
    if w >= 20 and h >= 20:
        disp = R.gpu_disparity(w, h)
    else:
        ys, xs = np.mgrid[0:h, 0:w]
        disp = (1.0 / (3.0 + 0.004 * xs + 0.003 * ys)).astype(F32)
    if w * h > 4:
        disp[0, 0] = 1.0            # column 0: much nearer than its neighbours
        disp[h - 1, w - 1] = 0.02   # column w - 1: much farther
    if w >= 8 and h >= 4:
        disp[1, w - 3] = 0.0
        disp[2, 3] = np.nan
        disp[h - 2, w // 2] = -0.25
    return disp

