"""numpy restatements of the reference's conversion loops for tests/test_gpu_conversion*.py, on top of the oracle's
camera (oracle_lib.Rig built from the un-normalised cameras, Camera::rescale'd like the tools do), and the inputs
those tests share. Nothing here touches the GPU."""
import json

import numpy as np

F32, F64 = np.float32, np.float64


def rescaled_rig(cams, w, h=None):
    """every camera rescaled to w x h, or camera i to w[i] when `w` is a list of sizes"""
    from oracle import oracle_lib as O

    rig = O.Rig(cams)
    for i in range(len(cams)):
        rig.rescale(i, *((w, h) if h is not None else w[i]))
    return rig


def norm3(p):
    """Eigen's unrolled 3-vector norm: sqrt(a0 + (a1 + a2))"""
    return np.sqrt(p[:, 0] * p[:, 0] + (p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]))


def pixel_centres(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], axis=1)


# ---------------------------------------------------------------- ExportPointCloud.cpp:67-137
def export_inputs(cam, w, h):
    from facebook360_dep_amd import synth

    bgr, disp, _, _ = synth.render_camera(cam, w, h)
    disp = disp.astype(F32).copy()
    cy, cx = h // 2, w // 2
    disp[cy, cx] = np.nan
    disp[cy + 1, cx + 2] = 0.0
    disp[cy - 6:cy - 3, cx - 5:cx - 2] = 0.1  # 10 m: beyond max_depth = 3
    return disp, bgr.astype(F32) / F32(65535)


_outside = {}  # (the whole camera description, w, h) -> isOutsideImageCircle of every pixel centre, computed once


def outside_image_circle(rig, cams, cam, w, h):
    # (the id alone does not do: every rig of the tests calls its cameras cam0, cam1, ...)
    key = (json.dumps(cams[cam], sort_keys=True), w, h)
    if key not in _outside:
        _outside[key] = np.array([rig.is_outside_image_circle(cam, px, py) for px, py in pixel_centres(w, h)])
    return _outside[key]


def mix32(h):
    """derp_points.h's mix32 (the murmur3 finaliser) on uint32 arrays, which wrap like the device's uint32_t"""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def subsample_keeps(cam_index, pixels, subsample):
    """derp_points.h's subsample_keeps: which pixel indices --subsample=N keeps for camera `cam_index`"""
    seed = mix32(np.array([(cam_index + 0x9E3779B9) & 0xFFFFFFFF], dtype=np.uint32))
    return mix32(np.asarray(pixels, dtype=np.uint32) ^ seed) % np.uint32(subsample) == 0


def export_points(cams, cam, disp, color, max_depth, clip, cam_index=None, subsample=1):
    """-> (f32 [count, 6] x y z r g b in row-major pixel order, pixels outside the image circle). `subsample` > 1
    keeps the pixels subsample_keeps names for `cam_index` (the camera's own index unless given)."""
    h, w = disp.shape
    rig = rescaled_rig(cams, w, h)
    pix = pixel_centres(w, h)
    outside = outside_image_circle(rig, cams, cam, w, h)
    with np.errstate(all="ignore"):
        m = (F32(1) / disp.reshape(-1)).astype(F64)  # `1 / disparity(y, x)`: int / float, a float division, then widened
        world = rig.rig(cam, pix, m)
        depth = norm3(world)
        over = depth > max_depth
        keep = ~outside
        if subsample > 1:
            keep &= subsample_keeps(cam if cam_index is None else cam_index, np.arange(w * h), subsample)
        if clip:
            keep &= ~over
        else:
            world[over] *= (max_depth / depth[over])[:, None]
        out = np.concatenate([world.astype(F32), color.reshape(-1, 3)[:, ::-1]], axis=1)
    return np.ascontiguousarray(out[keep]), int(outside.sum())


# ---------------------------------------------------------------- ImportPointCloud.cpp:76-123
def random_cloud(n, seed):
    """directions uniform, radius log-uniform in 0.3-8 m; plus a NaN point, one beyond 6 m and one nearer than 0.5 m"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = np.exp(rng.uniform(np.log(0.3), np.log(8.0), n))
    pts = d * r[:, None]
    extra = np.array([[np.nan, 1.0, 0.2], [7.5, 0.3, 0.1], [0.4, 0.02, -0.01]])
    return np.ascontiguousarray(np.concatenate([pts[: n // 2], extra, pts[n // 2:]]))


EDGE_POINTS = 12  # clamp_cloud's points per camera and axis


def clamp_cloud(cams, sizes, depth=2.0):
    """Points that camera i projects a quarter pixel inside its right edge (x = w - 0.25) and its bottom edge
    (y = h - 0.25): std::round puts them on w (h), the clamp back on w - 1 (h - 1) (ImportPointCloud.cpp:108-109).
    Made with the reference's own unprojection, EDGE_POINTS per camera and axis, spread about the principal point
    along the edge, `depth` metres along the ray. -> (f64 [n, 3], camera of each point, axis of each point: 0 = x)"""
    rig = rescaled_rig(cams, sizes)
    pts, owner, axis = [], [], []
    t = np.linspace(-0.1, 0.1, EDGE_POINTS)  # (the mixed rig's FTHETA circle crosses the edge 0.148 either side)
    for i, (w, h) in enumerate(sizes):
        pr = rig.state(i)["principal"]
        ys = np.clip(pr[1] + t * h, 0.05, h - 0.05)
        xs = np.clip(pr[0] + t * w, 0.05, w - 0.05)
        pix = np.concatenate([np.stack([np.full(EDGE_POINTS, w - 0.25), ys], axis=1),
                              np.stack([xs, np.full(EDGE_POINTS, h - 0.25)], axis=1)])
        pts.append(rig.rig(i, pix, depth))
        owner += [i] * (2 * EDGE_POINTS)
        axis += [0] * EDGE_POINTS + [1] * EDGE_POINTS
    return np.ascontiguousarray(np.concatenate(pts)), np.array(owner), np.array(axis)


def boundary_depths(min_depth, max_depth):
    """the float values at and one ulp either side of both limits -> [(float32 depth, kept by the import)]"""
    out = []
    for limit in (F32(min_depth), F32(max_depth)):
        assert float(limit) in (min_depth, max_depth)  # the limits are floats: `==` after the rounding can happen
        for f in (np.nextafter(limit, F32(0)), limit, np.nextafter(limit, F32(np.inf))):
            out.append((f, min_depth <= float(f) <= max_depth))
    return out


def boundary_cloud(cams, min_depth, max_depth):
    """Points whose distance from the rig origin, ROUNDED TO FLOAT (ImportPointCloud.cpp:110), is each of
    boundary_depths: for every such float three points, of fp64 norm the float itself and 2^-27 (relative) either
    side of it, which all round to it. The 18 points look out of the rig along camera 0's and camera 1's forward
    axis, tilted on a grid of 0.08 rad so that each has a pixel of its own in an image of 40 pixels or more across.
    -> (f64 [36, 3], float32 depth of each point, kept flag of each point)"""
    pts, depths, kept = [], [], []
    for ci in (0, 1):
        fwd, right, up = (np.array(cams[ci][k], dtype=F64) for k in ("forward", "right", "up"))
        k = 0
        for f, keep in boundary_depths(min_depth, max_depth):
            for rel in (0.0, -(2.0 ** -27), 2.0 ** -27):
                d = fwd + 0.08 * (k % 6 - 2.5) * right + 0.08 * (k // 6 - 1) * up
                k += 1
                p = d * (float(f) * (1 + rel) / norm3(d[None])[0])
                assert F32(norm3(p[None])[0]) == f and (rel == 0.0 or norm3(p[None])[0] != float(f))
                pts.append(p)
                depths.append(f)
                kept.append(keep)
    return np.ascontiguousarray(np.array(pts)), np.array(depths, dtype=F32), np.array(kept)


def special_rows():
    """rows with an infinite coordinate of either sign, and the zero vector: none may touch an image"""
    inf = np.inf
    return np.array([[inf, 1.0, 0.2], [-inf, 0.5, 0.5], [1.0, -inf, 0.3], [0.2, 0.1, inf], [inf, -inf, inf],
                     [0.0, 0.0, 0.0]])


def import_points(cams, pts, sizes, min_depth, max_depth):
    """sizes: one (w, h) per camera -> one f32 [h, w] disparity image per camera"""
    rig = rescaled_rig(cams, sizes)
    pts = np.ascontiguousarray(pts, dtype=F64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        depth = norm3(pts).astype(F32)  # from the rig origin (reference quirk)
        depth[(depth.astype(F64) < min_depth) | (depth.astype(F64) > max_depth)] = np.inf
        cand = F32(1.0) / depth
        # `std::max(disparity(ySrc, xSrc), 1.0f / depth)` (:114-115) on an image that starts at 0 (:83): std::max(old, NaN)
        # == old, and std::max(old, 0) == old since no pixel goes below 0. Only positive candidates are looked at; a
        # point with an infinite coordinate has none (its depth is set to INFINITY, :111-112), and no pixel either
        live = cand > 0
    images = []
    pts, cand = pts[live], cand[live]
    for i, (w, h) in enumerate(sizes):
        seen, pix = rig.sees(i, pts)
        sel = seen
        xs = np.clip(np.floor(pix[sel, 0] + 0.5).astype(np.int64), 0, w - 1)  # std::round of a non-negative value
        ys = np.clip(np.floor(pix[sel, 1] + 0.5).astype(np.int64), 0, h - 1)
        img = np.zeros((h, w), F32)
        np.maximum.at(img, (ys, xs), cand[sel])
        images.append(img)
    return images


# ---------------------------------------------------------------- ProjectEquirectsToCameras.cpp:94-125
def blob_mask(w, h, seed):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(14):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 7)
        m |= (xs - cx) ** 2 + (ys - cy) ** 2 < r * r
    return m.astype(np.uint8)


def project_equirect_mask(cams, cam, eqr, w, h, depth):
    """-> (mask u8 [h, w], band bool [h, w]: fp64 equirect coordinate within 2e-4 px of an integer in either axis)"""
    eh, ew = eqr.shape
    rig = rescaled_rig(cams, w, h)
    world = rig.rig(cam, pixel_centres(w, h), depth)
    # image_util::worldToEquirect (ImageUtil.cpp:127-140) with its float roundings; acos / atan2 in fp64 on the float
    # arguments, rounded to float
    d = norm3(world).astype(F32).astype(F64)
    x, y, z = [(world[:, k] / d).astype(F32) for k in range(3)]
    phi = np.arccos(z.astype(F64)).astype(F32)
    theta = np.arctan2(y.astype(F64), x.astype(F64)).astype(F32)
    theta = np.where(theta > 0, (theta.astype(F64) - 2 * np.pi).astype(F32), theta)
    v = (phi.astype(F64) / np.pi).astype(F32)
    u = ((-theta).astype(F64) / (2 * np.pi)).astype(F32)
    px, py = (u * F32(ew)).astype(F64), (v * F32(eh)).astype(F64)
    ok = ~((px < 0) | (py < 0) | (px >= ew) | (py >= eh))
    out = np.zeros(w * h, np.uint8)
    out[ok] = eqr[py[ok].astype(np.int64), px[ok].astype(np.int64)] != 0
    # the same coordinate without the float roundings
    n = norm3(world)
    t = np.arctan2(world[:, 1] / n, world[:, 0] / n)
    t = np.where(t > 0, t - 2 * np.pi, t)
    qx, qy = -t / (2 * np.pi) * ew, np.arccos(world[:, 2] / n) / np.pi * eh
    band = (np.abs(qx - np.rint(qx)) < 2e-4) | (np.abs(qy - np.rint(qy)) < 2e-4)
    return out.reshape(h, w), band.reshape(h, w)
