"""numpy restatement of MeshStreamRenderer's GPU stages (facebook360_dep_amd/csrc/derp_stream.h and the views of
derp_render_api.h / derp_stream_api.h), operation for operation in fp32, for tests/test_stream_ref.py and
tests/test_gpu_mesh_stream*.py. Every array here is float32 and every binary operation rounds once, as the device code
(built with -ffp-contract=off) does. The direction table comes from the oracle's camera, expf from this machine's libm
(the device's expf_glibc equals it), the sRGB table from the library (derp.stream_srgb_table), the cube -> equirect step
from the SimpleMeshRenderer checker. Nothing in this file touches the GPU.

The box of pixels a triangle is rasterised in is part of the coverage rule and is restated too (box): a pixel is covered
when it lies in the box and passes the edge functions. tests/test_stream_ref.py shows that the box leaves out nothing the
edge functions cover, for triangles with vertices kilometres away and behind the eye."""
import ctypes
import math

import numpy as np

F32 = np.float32
NEAR = F32(0.1)
DIRECTIONS = 128
_AXES = [[(0, +1), (2, -1), (1, -1)], [(0, -1), (2, +1), (1, -1)], [(1, +1), (0, +1), (2, +1)],
         [(1, -1), (0, +1), (2, -1)], [(2, +1), (0, +1), (1, -1)], [(2, -1), (0, -1), (1, -1)]]  # {major, sc, tc}

_libm_expf = None


def expf(x):
    """glibc's expf of every element (once per distinct value)"""
    global _libm_expf
    if _libm_expf is None:
        libm = ctypes.CDLL("libm.so.6")
        libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
        _libm_expf = libm.expf
    x = np.asarray(x, dtype=F32)
    values, inverse = np.unique(x, return_inverse=True)
    return np.array([_libm_expf(float(v)) for v in values], dtype=F32)[inverse].reshape(x.shape)


# ---------------------------------------------------------------- views (smr_snapshot_view, smr_face_view)
def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=F32)


def _unit(a):
    return a / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def view(kind, width, height, position=(0, 0, 0), forward=(-1, 0, 0), up=(0, 0, 1), fov=90.0, face=0):
    """-> (R f32 [3, 3] rows right / up / backwards, c f32 [3], kx, ky, W, H) of a snapshot or of cube face `face`"""
    c = np.array(position, dtype=np.float64).astype(F32)
    if kind == "snapshot":
        fwd, upv = np.array(forward, dtype=np.float64).astype(F32), np.array(up, dtype=np.float64).astype(F32)
        right = _cross(upv, -fwd)
        f = _unit(fwd)
        u = _unit(_cross(right, fwd))
        R = np.stack([_cross(u, -f), u, -f])
        n = F32(0.1)
        x_max = F32(float(n) * math.tan(fov / 180 * math.pi / 2))
        y_max = x_max * F32(height) / F32(width)
        return R, c, F32(2) * n / (x_max - -x_max), F32(2) * n / (y_max - -y_max), width, height
    R = np.zeros((3, 3), dtype=F32)
    axes = _AXES[face]
    R[0, axes[1][0]] = axes[1][1]
    R[1, axes[2][0]] = axes[2][1]
    R[2, axes[0][0]] = -axes[0][1]
    return R, c, F32(1), F32(1), height, height


def transform(v):
    """stream_transform: the 4 x 4 matrix of a view"""
    R, c, kx, ky, _, _ = v
    t = np.array([-((R[r, 0] * c[0] + R[r, 1] * c[1]) + R[r, 2] * c[2]) for r in range(3)], dtype=F32)
    rows = np.concatenate([R, t[:, None]], axis=1)
    m = np.stack([kx * rows[0], ky * rows[1], -rows[2], -rows[2]]).astype(F32)
    m[2, 3] = m[2, 3] - F32(2) * NEAR
    return m


# ---------------------------------------------------------------- GL_LINEAR, clamp to edge (canopy_bilinear)
def _to_int(x):
    """the device's float -> int conversion: saturating, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0, np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)


def bilinear(img, u, v):
    """img f32 [H, W, C]; u, v f32 arrays of one shape -> [..., C]. Texel coordinate f = u * size - 0.5, x0 = floor(f),
    fraction a = f - x0, the texels x0 and x0 + 1 clamped, top = p00 (1 - a) + p10 a, then rows the same way."""
    H, W = img.shape[:2]
    with np.errstate(all="ignore"):
        fx, fy = u * F32(W) - F32(0.5), v * F32(H) - F32(0.5)
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = (fx - x0f)[..., None], (fy - y0f)[..., None]
        x0, y0 = _to_int(x0f), _to_int(y0f)
        wrap = lambda i: (i + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31  # noqa: E731  (int32 x0 + 1)
        xa, xb = np.clip(x0, 0, W - 1), np.clip(wrap(x0), 0, W - 1)
        ya, yb = np.clip(y0, 0, H - 1), np.clip(wrap(y0), 0, H - 1)
        one = F32(1)
        top = img[ya, xa] * (one - ax) + img[ya, xb] * ax
        bot = img[yb, xa] * (one - ax) + img[yb, xb] * ax
        return top * (one - ay) + bot * ay


# ---------------------------------------------------------------- the scene
def direction_table(cam):
    """RigScene::createDirection: camera.rig(c * resolution / 127).direction() as float [128, 128, 3]"""
    from oracle import oracle_lib as O

    rig = O.Rig([dict(cam, origin=[0.0, 0.0, 0.0])])  # a ray from the origin at depth 1 is its direction
    resx, resy = float(cam["resolution"][0]), float(cam["resolution"][1])
    pix = [(x * resx / (DIRECTIONS - 1), y * resy / (DIRECTIONS - 1)) for y in range(DIRECTIONS) for x in range(DIRECTIONS)]
    return rig.rig(0, np.array(pix), 1.0).astype(F32).reshape(DIRECTIONS, DIRECTIONS, 3)


def texture(rgba, table):
    """.rgba bytes [h, w, 4] -> linear float texels in the output's B G R order"""
    return np.asarray(table, dtype=F32)[np.asarray(rgba)[:, :, [2, 1, 0]]]


def vertex_stage(cam, dirs, vtx, m):
    """cameraMeshVS -> (clip f32 [n, 4], texVar f32 [n, 2])"""
    vtx = np.asarray(vtx, dtype=F32).reshape(-1, 3)
    w, h = int(cam["resolution"][0]), int(cam["resolution"][1])
    focal = F32(float(cam["focal"][0]))
    pos = np.array(cam["origin"], dtype=np.float64).astype(F32)
    with np.errstate(all="ignore"):
        tu, tv = (F32(1) / F32(w)) * vtx[:, 0], (F32(1) / F32(h)) * vtx[:, 1]
        depth = focal / vtx[:, 2]
        k = F32(DIRECTIONS)
        su, sv = (F32(0.5) + tu * (k - F32(1))) / k, (F32(0.5) + tv * (k - F32(1))) / k
        d = bilinear(dirs, su, sv)
        x, y, z = pos[0] + depth * d[:, 0], pos[1] + depth * d[:, 1], pos[2] + depth * d[:, 2]
        clip = np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(4)], axis=1)
    return clip.astype(F32), np.stack([tu, tv], axis=1).astype(F32)


# ---------------------------------------------------------------- the rasteriser
def setup(clip, tri, W, H):
    """stream_setup -> (a, b, c [3] each, det, hx, hy, hw [3] each) or None when the triangle is skipped"""
    i = [int(t) for t in tri]
    if i[0] == i[1] or i[1] == i[2] or i[0] == i[2]:
        return None
    p = clip[i]
    if not np.isfinite(p).all():
        return None
    with np.errstate(all="ignore"):
        hx = (p[:, 0] + p[:, 3]) * F32(0.5) * F32(W)
        hy = (p[:, 1] + p[:, 3]) * F32(0.5) * F32(H)
        hw = p[:, 3]
        if not (hw >= NEAR).any():
            return None
        k1, k2 = [1, 2, 0], [2, 0, 1]
        a = hy[k1] * hw[k2] - hw[k1] * hy[k2]
        b = hw[k1] * hx[k2] - hx[k1] * hw[k2]
        c = hx[k1] * hy[k2] - hy[k1] * hx[k2]
        det = (hx[0] * a[0] + hy[0] * b[0]) + hw[0] * c[0]
    if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all() and np.isfinite(det)) or det == 0:
        return None
    if det < 0:
        a, b, c, det = -a, -b, -c, -det
    return a, b, c, det, hx, hy, hw


def box(T, W, H):
    """stream_box -> (i0, j0, i1, j1), or None when it is empty"""
    hx, hy, hw = T[4:7]
    cut = NEAR * F32(0.5)
    side = F32(max(W, H))
    base = F32(1) + side * side * F32(2.0 ** -22)
    lo, hi, whole = [F32(np.inf), F32(np.inf)], [F32(-np.inf), F32(-np.inf)], False
    with np.errstate(all="ignore"):
        def take(p, m):
            nonlocal whole
            for d in range(2):
                p0, p1 = p[d] - m[d], p[d] + m[d]
                whole = whole or not (np.isfinite(p0) and np.isfinite(p1))
                lo[d], hi[d] = np.fmin(lo[d], p0), np.fmax(hi[d], p1)

        for k in range(3):
            n = (k + 1) % 3
            if hw[k] >= cut:
                p = (hx[k] / hw[k], hy[k] / hw[k])
                take(p, [base + F32(1e-6) * abs(v) for v in p])
            if (hw[k] >= cut) != (hw[n] >= cut):
                a, b = (k, n) if abs(hw[k] - cut) <= abs(hw[n] - cut) else (n, k)
                f = (cut - hw[a]) / (hw[b] - hw[a])
                t = (f * (hx[b] - hx[a]), f * (hy[b] - hy[a]))
                take(((hx[a] + t[0]) / cut, (hy[a] + t[1]) / cut),
                     (base + F32(1e-5) * (abs(hx[a]) + abs(t[0])), base + F32(1e-5) * (abs(hy[a]) + abs(t[1]))))
        if whole:
            lo, hi = [F32(0), F32(0)], [F32(W), F32(H)]
        lox, hix = np.fmax(lo[0], F32(0)), np.fmin(hi[0], F32(W))
        loy, hiy = np.fmax(lo[1], F32(0)), np.fmin(hi[1], F32(H))
        if not (lox <= hix and loy <= hiy):
            return None
        i0, i1 = int(np.ceil(lox - F32(0.5))), min(W - 1, int(np.floor(hix - F32(0.5))))
        j0, j1 = int(np.ceil(loy - F32(0.5))), min(H - 1, int(np.floor(hiy - F32(0.5))))
    return (i0, j0, i1, j1) if i0 <= i1 and j0 <= j1 else None


def cover(T, W, H, boxed=True):
    """stream_cover at every pixel centre of the triangle's box (boxed=False: of the view, the edge functions alone)
    -> (covered bool [H, W], 1 / w f32 [H, W], e [3, H, W], s [H, W])"""
    a, b, c, det = T[:4]
    px = (np.arange(W, dtype=F32) + F32(0.5))[None, :]
    py = (np.arange(H, dtype=F32) + F32(0.5))[:, None]
    with np.errstate(all="ignore"):
        e = np.stack([(px * a[k] + py * b[k]) + c[k] for k in range(3)])
        inside = np.ones((H, W), dtype=bool)
        for k in range(3):
            owner = bool(a[k] > 0 or (a[k] == 0 and b[k] > 0))
            inside &= (e[k] > 0) | ((e[k] == 0) & owner)
        s = (e[0] + e[1]) + e[2]
        iw = s / det
        w = F32(1) / iw
        inside &= (s > 0) & (iw > 0) & (w >= NEAR)
    if boxed:
        bx = box(T, W, H)
        boxed_in = np.zeros((H, W), dtype=bool)
        if bx is not None:
            boxed_in[bx[1]:bx[3] + 1, bx[0]:bx[2] + 1] = True
        inside &= boxed_in
    return inside, iw.astype(F32), e, s


def raster(clip, tex_var, idx, W, H):
    """One camera's depth buffer -> (winner i64 [H, W] (-1: none), u, v f32 [H, W] of the winner): GL_LESS on the eye
    depth, the triangle that comes first in the index buffer stays at equal depth."""
    idx = np.asarray(idx).reshape(-1, 3)
    winner = np.full((H, W), -1, dtype=np.int64)
    best = np.zeros((H, W), dtype=F32)
    u, v = np.zeros((H, W), dtype=F32), np.zeros((H, W), dtype=F32)
    for t, tri in enumerate(idx):
        T = setup(clip, tri, W, H)
        if T is None:
            continue
        inside, iw, e, s = cover(T, W, H)
        better = inside & (iw > best)
        if not better.any():
            continue
        tu, tv = tex_var[tri, 0], tex_var[tri, 1]
        with np.errstate(all="ignore"):
            tu_p = ((e[0] * tu[0] + e[1] * tu[1]) + e[2] * tu[2]) / s
            tv_p = ((e[0] * tv[0] + e[1] * tv[1]) + e[2] * tv[2]) / s
        winner[better], best[better], u[better], v[better] = t, iw[better], tu_p[better], tv_p[better]
    return winner, u, v


def unorm16(x):
    """GL_RGBA16: clamp to [0, 1] (NaN -> 0), round to nearest even"""
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, np.where(x < 1, x, F32(1)), F32(0)).astype(F32)
    return np.rint(c * F32(65535)) / F32(65535)


def fragment(tex, u, v):
    """cameraFS as the camera buffer stores it -> (bgr f32 [..., 3], weight = exp(30 a) - 1)"""
    color = unorm16(bilinear(tex, u, v))
    with np.errstate(all="ignore"):
        du, dv = u - F32(0.5), v - F32(0.5)
        cone = np.fmax(F32(1) / F32(255), F32(1) - F32(2) * np.sqrt(du * du + dv * dv))
    return color, expf(F32(30) * unorm16(cone)) - F32(1)


def render_view(scene, v, table, include=None, fade=1.0, zero_nans=False, flip=True):
    """RigScene::render in view v. scene = [None | dict(cam, vtx, idx, rgba)] per camera -> BGRA f32 [H, W, 4]"""
    W, H = v[4], v[5]
    m = transform(v)
    acc = np.zeros((H, W, 4), dtype=F32)
    for s, item in enumerate(scene):
        if item is None or (include is not None and not include[s]) or len(np.asarray(item["idx"]).reshape(-1)) == 0:
            continue
        dirs = item.get("dirs")
        if dirs is None:
            dirs = item["dirs"] = direction_table(item["cam"])
        clip, tex_var = vertex_stage(item["cam"], dirs, item["vtx"], m)
        winner, u, v_ = raster(clip, tex_var, item["idx"], W, H)
        hit = winner >= 0
        if not hit.any():
            continue
        color, weight = fragment(texture(item["rgba"], table), u[hit], v_[hit])
        with np.errstate(all="ignore"):
            acc[hit, :3] = weight[:, None] * color + acc[hit, :3]
            acc[hit, 3] = weight + acc[hit, 3]
    with np.errstate(all="ignore"):
        out = np.concatenate([F32(fade) * acc[:, :, :3] / acc[:, :, 3:], acc[:, :, 3:] / acc[:, :, 3:]], axis=2).astype(F32)
    if zero_nans:
        out[np.isnan(out)] = 0
    return out[::-1].copy() if flip else out


def render(scene, table, kind="cube", width=64, height=48, position=(0, 0, 0), forward=(-1, 0, 0), up=(0, 0, 1), fov=90.0,
           include=None, fade=1.0, zero_nans=False):
    """derp_stream_render: snapshot [h, w, 4], cube [6 h, h, 4] or equirect [h, 2 h, 4]"""
    args = dict(include=include, fade=fade, zero_nans=zero_nans)
    if kind == "snapshot":
        return render_view(scene, view(kind, width, height, position, forward, up, fov), table, **args)
    faces = [render_view(scene, view("cube", 0, height, position, face=f), table, flip=kind == "cube", **args)
             for f in range(6)]
    if kind == "cube":
        return np.concatenate(faces, axis=0)
    from tests import smr_check

    return smr_check.equirect(np.stack(faces))


def same(a, b):
    """number of elements whose bits differ; a NaN equals a NaN"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).sum())
