"""numpy restatements of the reference's conversion loops for tests/test_gpu_conversion*.py, on top of the oracle's
camera (oracle_lib.Rig built from the un-normalised cameras, Camera::rescale'd like the tools do), and the inputs
those tests share. Nothing here touches the GPU."""
import numpy as np

F32, F64 = np.float32, np.float64


def rescaled_rig(cams, w, h):
    from oracle import oracle_lib as O

    rig = O.Rig(cams)
    for i in range(len(cams)):
        rig.rescale(i, w, h)
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


_outside = {}  # (camera id, w, h) -> isOutsideImageCircle of every pixel centre, computed once


def outside_image_circle(rig, cams, cam, w, h):
    key = (cams[cam]["id"], w, h)
    if key not in _outside:
        _outside[key] = np.array([rig.is_outside_image_circle(cam, px, py) for px, py in pixel_centres(w, h)])
    return _outside[key]


def export_points(cams, cam, disp, color, max_depth, clip):
    """-> (f32 [count, 6] x y z r g b in row-major pixel order, pixels outside the image circle)"""
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


def import_points(cams, pts, w, h, min_depth, max_depth):
    rig = rescaled_rig(cams, w, h)
    with np.errstate(all="ignore"):
        depth = norm3(pts).astype(F32)  # from the rig origin (reference quirk)
        depth[(depth.astype(F64) < min_depth) | (depth.astype(F64) > max_depth)] = np.inf
        cand = F32(1.0) / depth
    images = []
    for i in range(len(cams)):
        seen, pix = rig.sees(i, pts)
        sel = seen & ~np.isnan(cand)  # std::max(old, NaN) == old
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
