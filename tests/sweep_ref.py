"""numpy restatement of the rig preview tools as DESIGN §8.7 defines them (source/render/GenerateCameraOverlaps.cpp and
GenerateEquirect.cpp), on the oracle's camera (oracle_lib.Rig: rescale, rig, sees, is_outside_image_circle). Vectorised
over pixels; transcendentals of the equirect and of the rig centring come from Python's math module (the C library's),
one value at a time. Nothing here touches the GPU."""
import math

import numpy as np

from tests.conversion_ref import pixel_centres

F32, F64 = np.float32, np.float64


def scaled_rig(cams, resolutions):
    """Camera::rescale(resolution * scale): the resolutions are doubles and need not be whole"""
    from oracle import oracle_lib as O

    rig = O.Rig(cams)
    for i, (rx, ry) in enumerate(resolutions):
        rig.rescale(i, float(rx), float(ry))
    return rig


def round_away(x):
    """std::round on float32 arrays (halves away from zero) without the rounding of x + 0.5"""
    x = np.asarray(x, dtype=F32)
    t = np.trunc(x)
    return (t + np.where(np.abs(x - t) >= F32(0.5), np.copysign(F32(1), x), F32(0))).astype(F32)


def to_int(v):
    """float -> int as the device converts it: truncation, NaN -> 0 (the reference's conversion of NaN is undefined)"""
    v = np.asarray(v)
    return np.where(np.isnan(v), 0, np.trunc(np.nan_to_num(v, nan=0.0, posinf=2e9, neginf=-2e9))).astype(np.int64)


def texel(img, x, y):
    h, w = img.shape[:2]
    return img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]


def bilinear(img, px, py):
    """getPixelBilinear (CvUtil.h:83-120) of float BGRA `img` at float coordinates -> ([n, 4] f32, taps' raw indices)"""
    x, y = np.asarray(px).astype(F32), np.asarray(py).astype(F32)
    xf, yf = round_away(x), round_away(y)
    xi, yi = to_int(xf), to_int(yf)
    xw, yw = (x - xf + F32(0.5))[:, None], (y - yf + F32(0.5))[:, None]
    one = F32(1)
    p00, p01 = texel(img, xi - 1, yi - 1), texel(img, xi, yi - 1)
    p10, p11 = texel(img, xi - 1, yi), texel(img, xi, yi)
    out = (one - xw) * (one - yw) * p00 + xw * (one - yw) * p01 + (one - xw) * yw * p10 + xw * yw * p11
    assert out.dtype == F32
    return out, (xi, yi)


class Rigged:
    """the rescaled rig with its float BGRA images"""

    def __init__(self, cams, images, resolutions):
        self.cams, self.n = cams, len(cams)
        self.images = [np.ascontiguousarray(im, dtype=F32) for im in images]
        self.res = [tuple(r) for r in resolutions]
        self.rig = scaled_rig(cams, self.res)
        self._outside = {}

    def outside(self, dst):
        if dst not in self._outside:
            h, w = self.images[dst].shape[:2]
            self._outside[dst] = np.array([self.rig.is_outside_image_circle(dst, px, py) for px, py in pixel_centres(w, h)])
        return self._outside[dst]

    # ---------------------------------------------------------------- GenerateCameraOverlaps.cpp:54-83
    def overlaps(self, dst, disparity, order=None, stats=None):
        """projectSrcsToDst at one disparity -> f32 [h, w, 4]. stats: a dict that receives `count` [h, w] (-1 outside
        the image circle) and `clamped`, the set of image edges ("left", ...) at which some tap was clamped"""
        h, w = self.images[dst].shape[:2]
        outside = self.outside(dst)
        with np.errstate(all="ignore"):
            m = float(F32(1) / F32(disparity))
            world = self.rig.rig(dst, pixel_centres(w, h), m)
            total = np.zeros((w * h, 4), F32)
            count = np.zeros(w * h, np.int64)
            clamped = set()
            for src in (range(self.n) if order is None else order):
                seen, pix = self.rig.sees(src, world)
                seen &= ~outside
                v, (xi, yi) = bilinear(self.images[src], pix[seen, 0], pix[seen, 1])
                total[seen] += v
                count[seen] += 1
                sh, sw = self.images[src].shape[:2]
                if len(xi):
                    clamped |= {name for name, hit in (("left", (xi - 1 < 0).any()), ("right", (xi > sw - 1).any()),
                                                       ("top", (yi - 1 < 0).any()), ("bottom", (yi > sh - 1).any())) if hit}
            out = (F32(1) / count.astype(F32))[:, None] * total
            out[outside] = 0
        if stats is not None:
            stats["count"] = np.where(outside, -1, count).reshape(h, w)
            stats["clamped"] = clamped
        assert out.dtype == F32
        return out.reshape(h, w, 4)

    # ---------------------------------------------------------------- GenerateEquirect.cpp:79-175
    def equirect_points(self, W, H, depth, window=None, out_size=None):
        """getEquirectPoint (:102-115) of every output pixel -> (f64 [h * w, 3], w, h)"""
        ow, oh = (W, H) if window is None else out_size
        xs = [float(x) if window is None else float(x) * float(window[1] - window[0]) / float(ow) + float(window[0])
              for x in range(ow)]
        ys = [float(y) if window is None else float(y) * float(window[3] - window[2]) / float(oh) + float(window[2])
              for y in range(oh)]
        theta = [-1 * ((x + 0.5) / float(W) * 2 * math.pi) for x in xs]
        phi = [(y + 0.5) / float(H) * math.pi for y in ys]
        cos_t, sin_t = np.array([math.cos(t) for t in theta]), np.array([math.sin(t) for t in theta])
        sin_p, cos_p = np.array([math.sin(p) for p in phi]), np.array([math.cos(p) for p in phi])
        depth = float(F32(depth))
        ds = depth * sin_p
        p = np.stack([np.broadcast_to((ds[:, None] * cos_t[None, :]), (oh, ow)),
                      np.broadcast_to((ds[:, None] * sin_t[None, :]), (oh, ow)),
                      np.broadcast_to((depth * cos_p)[:, None], (oh, ow))], axis=2)
        return np.ascontiguousarray(p.reshape(-1, 3)), ow, oh

    def equirect(self, W, H, depth, window=None, out_size=None, black_bg=False, fetch="trunc", stats=None):
        """-> f32 [h, w, 4]. stats receives `count` [h, w] and `clamp_mattered`: some truncated index lay past the image"""
        p, ow, oh = self.equirect_points(W, H, depth, window, out_size)
        total = np.zeros((len(p), 4), F32)
        count = np.zeros(len(p), np.int64)
        past = False
        for src in range(self.n):
            seen, pix = self.rig.sees(src, p)
            q = pix[seen]
            if fetch == "round":  # (the seeded defect of the tests)
                q = np.floor(q + 0.5)
            xi, yi = to_int(q[:, 0]), to_int(q[:, 1])
            sh, sw = self.images[src].shape[:2]
            past |= bool((xi > sw - 1).any() or (yi > sh - 1).any())
            total[seen] += texel(self.images[src], xi, yi)
            count[seen] += 1
        with np.errstate(all="ignore"):
            out = (total.astype(F64) * (1.0 / count.astype(F64))[:, None]).astype(F32)  # Vec / int
        out[count == 0] = np.array([0, 0, 0 if black_bg else 1, 1], F32)
        if stats is not None:
            stats["count"] = count.reshape(oh, ow)
            stats["clamp_mattered"] = past
        return out.reshape(oh, ow, 4)

    def equirect_bounds(self, W, H, depth):
        """createCroppedEquirect's first loop (:139-156) -> (minX, maxX, minY, maxY); (W, 0, H, 0) where nothing is seen"""
        p, _, _ = self.equirect_points(W, H, depth)
        any_seen = np.zeros(len(p), bool)
        for src in range(self.n):
            any_seen |= self.rig.sees(src, p)[0]
        ys, xs = np.nonzero(any_seen.reshape(H, W))
        if len(xs) == 0:
            return (W, 0, H, 0)
        return (int(min(W, xs.min())), int(max(0, xs.max())), int(min(H, ys.min())), int(max(0, ys.max())))


def to_u8(img):
    """`255.0f * image` into an 8-bit file: float product, round half to even, saturate; NaN -> 0"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(img, dtype=F32) * F32(255))
        return np.where(np.isnan(r), 0, np.clip(r, 0, 255)).astype(np.uint8)


def crop_size(height, bounds):
    """newWidth (:158-159): size_t(height / (maxY - minY) * (maxX - minX)); None for an empty box"""
    min_x, max_x, min_y, max_y = [float(b) for b in bounds]
    if not (max_x - min_x > 0 and max_y - min_y > 0):
        return None
    return int(float(height) / (max_y - min_y) * (max_x - min_x))


def overlap_disparities(num, min_depth_m=1, max_depth_m=10):
    """probeDisparity (ImageUtil.cpp:100-107) as dumpOverlaps calls it, and the stems int(depth * 100) in float.
    One depth: fraction 0 (the reference's 0 / 0 is not copied)"""
    a, b = float(F32(1) / F32(min_depth_m)), float(F32(1) / F32(max_depth_m))
    disp, stems = [], []
    for d in range(num):
        fraction = 0.0 if num == 1 else float(d) / float(num - 1)
        disp.append(F32(fraction * a + (1 - fraction) * b))
        stems.append(int(F32(1) / disp[-1] * F32(100)))
    return np.array(disp, F32), np.array(stems, np.int32)


def equirect_depths(num, depth_min=1.0, depth_max=10.0):
    """GenerateEquirect.cpp:264-272 in fp32 by index i, and the stems int(double(depth) * 100)"""
    disp_min, disp_max = F32(1.0 / depth_max), F32(1.0 / depth_min)
    depths, stems = [], []
    for i in range(num):
        if num == 1:
            disp = disp_min
        else:
            fraction = F32(i) / F32(num - 1)
            disp = fraction * disp_min + (F32(1) - fraction) * disp_max
        depths.append(F32(1) / disp)
        stems.append(int(float(depths[-1]) * 100))
    return np.array(depths, F32), np.array(stems, np.int32)


# ---------------------------------------------------------------- centerRig, GenerateEquirect.cpp:177-231
def _sum3(a, b, c):
    return a + (b + c)


def _dot(a, b):
    return _sum3(a[0] * b[0], a[1] * b[1], a[2] * b[2])


def _unitarised(cams):
    """forward / up / right as Camera::setRotation leaves them (Camera.cpp:77-87), through the oracle's camera"""
    from oracle import oracle_lib as O

    rig = O.Rig(cams)
    out = []
    for i, cam in enumerate(cams):
        R = rig.state(i)["R"]
        out.append(dict(cam, right=[float(v) for v in R[0]], up=[float(v) for v in R[1]], forward=[float(-v) for v in R[2]]))
    return out


def _rotation_angle(a, b, sign):
    mag = math.sqrt(_dot(a, a)) * math.sqrt(_dot(b, b))
    return 0.0 if mag == 0 else sign * math.acos(_dot(a, b) / mag)


def rotate_rig(cams, axis, angle):
    """transformRig (RigTransform.h:73-97) about one axis (0 = x, 1 = y, 2 = z): no translation, scale 1"""
    w, s = math.cos(angle / 2), math.sin(angle / 2)
    t = 2 * s
    co, si = 1 - t * s, t * w
    R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    a, b = (axis + 1) % 3, (axis + 2) % 3
    R[a][a], R[b][b], R[a][b], R[b][a] = co, co, -si, si
    out = []
    for cam in cams:
        cam = dict(cam)
        for key in ("forward", "up", "right", "origin"):
            v = [float(x) for x in cam[key]]
            cam[key] = [_sum3(R[r][0] * v[0], R[r][1] * v[1], R[r][2] * v[2]) for r in range(3)]
        out.append(cam)
    return _unitarised(out)


def rig_center(cams, index, angles=None):
    """-> the rotated cameras; `angles` (a list) receives yaw, pitch and roll"""
    cams = _unitarised(cams)
    for step in range(3):
        sel = cams[index]
        f, u = sel["forward"], sel["up"]
        if step == 0:
            angle, axis = _rotation_angle([-1.0, 0.0, 0.0], [f[0], f[1], 0.0], 1 if f[1] > 0 else -1), 2
        elif step == 1:
            angle, axis = _rotation_angle([-1.0, 0.0, 0.0], [f[0], 0.0, f[2]], -1 if f[2] > 0 else 1), 1
        else:
            angle, axis = _rotation_angle([0.0, 0.0, 1.0], [0.0, u[1], u[2]], 1 if u[1] > 0 else -1), 0
        if angles is not None:
            angles.append(angle)
        cams = rotate_rig(cams, axis, angle)
    return cams
