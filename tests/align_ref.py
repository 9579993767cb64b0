"""numpy restatement of AlignColors (source/calibration/AlignColors.cpp) as DESIGN §8.8 defines it: the per-channel
camera models (createCalibratedRBRigs, :72-96), the warp maps (createWarpMap, :52-70: fp64, stored as float32) and the
resampling (warpImage, :98-117, through getPixelBilinear of CvUtil.h:108-120: float32 blend truncated to u16), with the
two implementation-defined points: a pixel centre on the principal point maps to itself, and undistort never aborts.
Imports nothing from the package. numpy never contracts a multiply and an add, like the reference's x86-64 build."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
SMIDGEN = 1.0 / 1e4  # 1 / kNearInfinity (Camera.h:264)


# ---- Camera::setDistortion (Camera.cpp:119-154): distortionMax = sqrt of the smallest positive real root of the
# derivative 1 + 3 d0 y + 5 d1 y^2 + 7 d2 y^3 in y = r^2. The root by bracketing at the derivative's own stationary
# points and bisection to the last bit, in plain doubles (test_align_ref compares it with numpy's polynomial roots).
def _poly(k, deg, x):
    acc = k[deg]
    for i in range(deg - 1, -1, -1):
        acc = acc * x + k[i]
    return acc


def smallest_positive_root(k, deg):
    stops = []
    if deg == 3:
        a, b, c = 3 * k[3], 2 * k[2], k[1]
        disc = b * b - 4 * a * c
        if disc >= 0:
            q = -0.5 * (b + math.copysign(math.sqrt(disc), b))
            r0 = q / a
            r1 = c / q if q != 0 else r0
            if r0 > r1:
                r0, r1 = r1, r0
            if r0 > 0:
                stops.append(r0)
            if r1 > 0 and r1 != r0:
                stops.append(r1)
    elif deg == 2:
        r = -k[1] / (2 * k[2])
        if r > 0:
            stops.append(r)
    left, f_left = 0.0, k[0]
    for seg in range(len(stops) + 1):
        if seg < len(stops):
            right = stops[seg]
        else:
            right = (left if left > 0 else 1.0) * 2
            tries = 0
            while _poly(k, deg, right) * f_left > 0 and tries < 2000:
                tries += 1
                right *= 2
            if tries >= 2000 or not math.isfinite(right):
                return math.inf
        f_right = _poly(k, deg, right)
        if f_right == 0:
            return right
        if (f_right > 0) != (f_left > 0):
            lo, hi, lo_pos = left, right, f_left > 0
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if not (lo < mid < hi):
                    break
                fm = _poly(k, deg, mid)
                if fm == 0:
                    return mid
                if (fm > 0) == lo_pos:
                    lo = mid
                else:
                    hi = mid
            return 0.5 * (lo + hi)
        left, f_left = right, f_right
    return math.inf


def distortion_max(d):
    count = 3
    while count > 0 and d[count - 1] == 0:
        count -= 1
    if count == 0:
        return math.inf
    k = [1.0, 0.0, 0.0, 0.0]
    for i in range(count):
        k[i + 1] = d[i] * (2 * i + 3)
    return math.sqrt(smallest_positive_root(k, count))


# ---- step 1: the models ----
def _padded(cam):
    d = [float(v) for v in cam.get("distortion", [])]
    return d + [0.0] * (3 - len(d))


def derive_cameras(green, red_ref, green_ref, blue_ref, double_ratio=False):
    """createCalibratedRBRigs for one camera of the rig (dicts as the rig files hold them) -> (red, blue).
    double_ratio: the variant the reference does NOT compute (focalRatio kept in double), for the float_ratio case."""
    for cam in (green, red_ref, green_ref, blue_ref):
        assert cam["focal"][0] == -cam["focal"][1], "pixels are not square"
    ratio = float(green["focal"][0]) / float(green_ref["focal"][0])
    if not double_ratio:
        ratio = float(F32(ratio))
    out = []
    for ref in (red_ref, blue_ref):
        cam = dict(green)
        s = float(ref["focal"][0]) * ratio
        cam["focal"] = [s, -s]
        cam.pop("distortion", None)
        if "distortion" in ref:
            cam["distortion"] = _padded(ref)
        out.append(cam)
    return tuple(out)


class Model:
    """what createWarpMap reads of a camera: scalar focal, principal, distortion and distortionMax, all un-normalised"""

    def __init__(self, cam):
        res = cam["resolution"]
        self.w, self.h = int(res[0]), int(res[1])
        self.focal = float(cam["focal"][0])
        self.principal = [float(v) for v in cam.get("principal", [res[0] / 2, res[1] / 2])]
        self.dist = _padded(cam)
        self.dist_max = distortion_max(self.dist)
        self.dist_zero = all(v == 0 for v in self.dist)


def distort(m, r, info=None):
    """Camera::distort (Camera.h:238-253) on an array"""
    r = np.asarray(r, F64)
    clamped = m.dist_max < r
    if info is not None:
        info["distort_clamped"] = clamped
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(clamped, m.dist_max, r)  # std::min(r, distortionMax_)
        r2 = r * r
        result = F64(m.dist[2])
        result = m.dist[1] + r2 * result
        result = m.dist[0] + r2 * result
        return (1.0 + r2 * result) * r


def undistort(m, y, info=None):
    """Camera::undistort (Camera.h:255-284) on an array, without the abort of :278"""
    y = np.asarray(y, F64)
    if m.dist_zero:
        if info is not None:
            info["undistort_at_max"] = np.zeros(y.shape, bool)
        return y.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        at_max = y >= distort(m, np.asarray(m.dist_max, F64))
        if info is not None:
            info["undistort_at_max"] = at_max
        result = np.where(at_max, m.dist_max, np.nan)
        done = at_max.copy()
        x0, y0, dy0 = np.zeros_like(y), np.zeros_like(y), np.ones_like(y)
        for _ in range(10):
            x1 = (y - y0) / dy0 + x0
            y1 = distort(m, x1)
            hit = ~done & (np.abs(y1 - y) < SMIDGEN)
            result = np.where(hit, x1, result)
            done |= hit
            dy1 = (distort(m, x1 + SMIDGEN) - y1) / SMIDGEN
            x0, y0, dy0 = x1, y1, dy1
        return np.where(done, result, x0)


# ---- step 2: createWarpMap(src, dst = green) ----
def warp_map(green, src, info=None):
    """green, src: Model -> [h, w, 2] float32 (x, y)"""
    px, py = np.meshgrid(np.arange(green.w, dtype=F64) + 0.5, np.arange(green.h, dtype=F64) + 0.5)
    dx, dy = px - green.principal[0], py - green.principal[1]
    norm = np.sqrt(dx * dx + dy * dy)
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = undistort(green, norm / green.focal, info)
        src_r = distort(src, theta, info)
        sx = ((dx / norm) * src.focal) * src_r + green.principal[0]
        sy = ((dy / norm) * src.focal) * src_r + green.principal[1]
    on_principal = norm == 0  # 0 / 0 in the reference: here the pixel centre itself
    if info is not None:
        info["on_principal"] = on_principal
    sx, sy = np.where(on_principal, px, sx), np.where(on_principal, py, sy)
    return np.stack([sx, sy], axis=-1).astype(F32)


def maps_of(green_cam, red_ref, green_ref, blue_ref, double_ratio=False):
    """-> (red map, blue map) of one camera of the calibrated rig"""
    red, blue = derive_cameras(green_cam, red_ref, green_ref, blue_ref, double_ratio)
    g = Model(green_cam)
    return warp_map(g, Model(red)), warp_map(g, Model(blue))


# ---- step 3: warpImage ----
def round_half_away(x):
    """std::round on float32 values (exact: the sum is formed in double)"""
    x64 = x.astype(F64)
    return np.copysign(np.floor(np.abs(x64) + 0.5), x64).astype(F32)


def sample(plane, at, info=None, rounded=False):
    """getPixelBilinear on one u16 plane [h, w] at the float32 positions at[..., 2] -> u16. rounded: the variant the
    reference does NOT compute (round to nearest instead of truncating), to show that a case sees the difference."""
    h, w = plane.shape
    x, y = at[..., 0].astype(F32), at[..., 1].astype(F32)
    xf, yf = round_half_away(x), round_half_away(y)
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    one, half = F32(1), F32(0.5)
    xw, yw = x - xf + half, y - yf + half
    xa, xb = np.clip(xi - 1, 0, w - 1), np.clip(xi, 0, w - 1)
    ya, yb = np.clip(yi - 1, 0, h - 1), np.clip(yi, 0, h - 1)
    if info is not None:
        info["inside"] = (xi - 1 >= 0) & (xi <= w - 1) & (yi - 1 >= 0) & (yi <= h - 1)
        info["tie"] = (np.abs(x.astype(F64) - np.trunc(x.astype(F64))) == 0.5) | (np.abs(y.astype(F64) - np.trunc(y.astype(F64))) == 0.5)
        info["left"], info["right"], info["above"], info["below"] = xi - 1 < 0, xi > w - 1, yi - 1 < 0, yi > h - 1
    p00, p01 = plane[ya, xa].astype(F32), plane[ya, xb].astype(F32)
    p10, p11 = plane[yb, xa].astype(F32), plane[yb, xb].astype(F32)
    v = (one - xw) * (one - yw) * p00 + xw * (one - yw) * p01 + (one - xw) * yw * p10 + xw * yw * p11
    assert v.dtype == F32
    v = np.floor(v + half) if rounded else np.trunc(v)
    return np.clip(v, 0, 65535).astype(np.uint16)


def align(image, red_map, blue_map, rounded=False):
    """image: BGR u16 [h, w, 3] -> the aligned image"""
    out = np.empty_like(image)
    out[..., 1] = image[..., 1]
    out[..., 2] = sample(image[..., 2], red_map, rounded=rounded)
    out[..., 0] = sample(image[..., 0], blue_map, rounded=rounded)
    return out
