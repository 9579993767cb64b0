"""Plain Python / numpy restatement of RigAnalyzer as DESIGN §8.9 defines it (source/rig/RigAnalyzer.cpp), on the
oracle's camera (oracle_lib.Rig: sees, rig, is_outside_image_circle, state). Points and tables come from Python's math
module (the C library's sin, cos, acos, sqrt), one value at a time; every visibility is the oracle camera's answer; the
rig editing is plain float arithmetic in Eigen's order of operations, with srand / rand taken from libc through ctypes.
Nothing here touches the GPU."""
import ctypes
import math

import numpy as np

from tests.sweep_ref import _unitarised

F32, F64 = np.float32, np.float64
NEAR_INFINITY = 1e4  # Camera::kNearInfinity (Camera.h)


# ---------------------------------------------------------------- sample directions and distances (:68-94, :562-565)
def fibonacci_units(count, discard_poles_deg=0.0):
    threshold = math.cos(discard_poles_deg * math.pi / 180)
    out = []
    for i in range(count):
        y = (i + 0.5) / count * 2 - 1
        r = math.sqrt(1 - y * y)
        phi = (1 + math.sqrt(5)) / 2
        roty = i / phi * 2 * math.pi
        p = (math.sin(roty) * r, y, math.cos(roty) * r)
        if abs(p[2]) < threshold:
            out.append(p)
    return np.array(out, dtype=F64).reshape(-1, 3)


def coverage_distances(min_distance=0.5):
    return np.array([min_distance / (1 - i / float(20)) for i in range(20)], dtype=F64)


# ---------------------------------------------------------------- Eigen's rotations, scalar paths
def _sum3(a, b, c):
    return a + (b + c)


def _quat(angle, axis):
    ha = 0.5 * angle
    s = math.sin(ha)
    return (math.cos(ha), s * axis[0], s * axis[1], s * axis[2])


def _qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx)


def _quat_matrix(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def euler_matrix(e, xyz=True):
    """rotationMatrixFromEulers (:96-101), radians"""
    x, y, z = _quat(e[0], (1.0, 0.0, 0.0)), _quat(e[1], (0.0, 1.0, 0.0)), _quat(e[2], (0.0, 0.0, 1.0))
    return _quat_matrix(_qmul(_qmul(z, y), x) if xyz else _qmul(_qmul(y, x), z))


def aa_matrix(angle, a):
    """AngleAxis::toRotationMatrix"""
    s, cs = math.sin(angle), math.cos(angle)
    sx, sy, sz = s * a[0], s * a[1], s * a[2]
    c1x, c1y, c1z = (1.0 - cs) * a[0], (1.0 - cs) * a[1], (1.0 - cs) * a[2]
    R = [[0.0] * 3 for _ in range(3)]
    t = c1x * a[1]
    R[0][1], R[1][0] = t - sz, t + sz
    t = c1x * a[2]
    R[0][2], R[2][0] = t + sy, t - sy
    t = c1y * a[2]
    R[1][2], R[2][1] = t - sx, t + sx
    R[0][0], R[1][1], R[2][2] = c1x * a[0] + cs, c1y * a[1] + cs, c1z * a[2] + cs
    return R


def matrix_aa(m):
    """AngleAxis(matrix) = AngleAxis(Quaternion(matrix)) -> (angle, axis)"""
    q = [0.0] * 4
    t = _sum3(m[0][0], m[1][1], m[2][2])
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    n = math.sqrt(_sum3(q[0] * q[0], q[1] * q[1], q[2] * q[2]))
    if n != 0:
        angle = 2.0 * math.atan2(n, abs(q[3]))
        if q[3] < 0:
            n = -n
        return angle, [q[0] / n, q[1] / n, q[2] / n]
    return 0.0, [1.0, 0.0, 0.0]


def _apply(m, v):
    return [_sum3(m[r][0] * v[0], m[r][1] * v[1], m[r][2] * v[2]) for r in range(3)]


def _norm(v):
    return math.sqrt(_sum3(v[0] * v[0], v[1] * v[1], v[2] * v[2]))


def _floats(cam):
    cam = dict(cam)
    for k in ("origin", "forward", "up", "right", "resolution", "focal"):
        cam[k] = [float(v) for v in cam[k]]
    if "principal" in cam:
        cam["principal"] = [float(v) for v in cam["principal"]]
    return cam


def loaded(cams):
    """the cameras as Camera::Camera leaves them: forward / up / right through setRotation"""
    return _unitarised([_floats(c) for c in cams])


# ---------------------------------------------------------------- rig construction and editing
ARRANGEMENTS = {  # name -> (xyz, rows that take the custom angle, its default, eulers) (:157-238)
    "ballcam24": (False, 0, None, [
        (22.998, -36.1543, 132.267), (-2.89381, -156.601, 168.482), (-50.2907, -68.7384, 139.028),
        (-80.2662, 172.721, 113.889), (57.5173, 87.6811, 161.596), (6.46204, 162.32, 70.7419),
        (21.8577, 118.439, 114.195), (77.4316, -95.0674, -100.379), (-20.2739, 41.1554, -135.466),
        (-38.2009, 172.776, -171.825), (-0.841465, -110.909, 57.8619), (-39.8563, -128.178, 46.3619),
        (-54.3882, 8.6561, -13.3586), (24.3104, 51.5133, -20.0308), (35.7198, -82.6713, 160.228),
        (-48.4447, 85.1941, 93.5637), (48.4425, 165.464, 19.7297), (-3.41527, 84.0526, 56.5226),
        (-20.5666, -24.4286, 14.2745), (35.8214, -139.006, -27.4138), (-8.22831, -69.3313, -46.6214),
        (51.5282, 4.18718, -133.303), (6.61383, 8.24745, -72.7674), (-22.4038, 126.995, 13.7087)]),
    "tetra": (True, 3, "tetra", [(None, 0, 0), (None, 0, 120), (None, 0, -120), (0, 0, 0)]),
    "tetratilted": (False, 0, None, [(-35.2644, 45, -65.1818), (-35.2644, -135, -137.834), (35.2644, -45, -45.0048),
                                     (35.2644, 135, -104.664)]),
    "ring4": (True, 4, 90, [(None, 0, 0), (None, 0, 90), (None, 0, 180), (None, 0, 270)]),
    "cube": (True, 4, 90, [(None, 0, 0), (None, 0, 90), (None, 0, 180), (None, 0, 270), (0, 0, 0), (180, 0, 0)]),
    "carbon0": (False, 0, None, [(-35.2644, 3.89537e-15, 112.232), (-35.2644, 120, -67.3096), (-35.2644, -120, 155.867),
                                 (35.2644, 180, 21.9328), (35.2644, -60, 14.0236), (35.2644, 60, 66.2737)]),
    "carbon1": (False, 0, None, [(-35.2644, 1.94768e-15, 133.504), (-35.2644, 120, -179.989), (-35.2644, -120, -134.51),
                                 (35.2644, 180, 89.7419), (35.2644, -60, 43.7899), (35.2644, 60, -45.1612)]),
    "diamond": (True, 3, 90, [(None, 0, 0), (None, 0, 120), (None, 0, 240), (0, 0, 0), (180, 0, 0)]),
}


def tetra_default_angle():
    return math.acos(-1 / 3.0) * 180 / math.pi


def rig_from_eulers(model, eulers_deg, xyz=False, one_based=False):
    """makeRigFromEulers (:103-131)"""
    model = _floats(model)
    radius = _norm(model["origin"])
    out = []
    for i, e in enumerate(eulers_deg):
        m = euler_matrix([float(v) * (math.pi / 180) for v in e], xyz)
        cam = dict(model, forward=[m[r][2] for r in range(3)], up=[m[r][1] for r in range(3)],
                   right=[-m[r][0] for r in range(3)])
        cam = _unitarised([cam])[0]
        cam["origin"] = [radius * v for v in cam["forward"]]
        cam["id"] = "cam%d" % (i + (1 if one_based else 0))
        out.append(cam)
    return out


def rig_arrangement(name, model, custom=-1.0, one_based=False):
    xyz, _, default, eulers = ARRANGEMENTS[name]
    default = tetra_default_angle() if default == "tetra" else default
    a = default if custom == -1 else custom
    return rig_from_eulers(model, [(a if e[0] is None else e[0], e[1], e[2]) for e in eulers], xyz, one_based)


def _transformed(cam, m):
    cam = dict(cam)
    for key in ("origin", "forward", "up", "right"):
        cam[key] = _apply(m, cam[key])
    return _unitarised([cam])[0]


def rig_revolve(cams, eulers_rad):
    """revolveRig (:133-155)"""
    cams = loaded(cams)
    out = []
    for frame, e in enumerate(eulers_rad):
        m = euler_matrix([float(v) for v in e], True)
        for cam in cams:
            cam = _transformed(cam, m)
            if len(eulers_rad) > 1:
                cam["id"] = cam["id"] + "_" + str(frame)
            out.append(cam)
    return out


def rig_rotate(cams, m):
    return [_transformed(cam, [[float(v) for v in row] for row in m]) for cam in loaded(cams)]


def align_z_matrix(p):
    """--rotate_cam_z (:505-510)"""
    p = [float(v) for v in p]
    angle = math.acos(_sum3(p[0] * 0, p[1] * 0, p[2] * 1))
    axis = [p[1] * 1 - p[2] * 0, p[2] * 0 - p[0] * 1, p[0] * 0 - p[1] * 0]
    sq = _sum3(axis[0] * axis[0], axis[1] * axis[1], axis[2] * axis[2])
    if sq > 0:
        n = math.sqrt(sq)
        axis = [v / n for v in axis]
    return aa_matrix(angle, axis)


_libc = ctypes.CDLL(None)
_libc.rand.restype = ctypes.c_int
RAND_MAX = 2147483647


def rig_perturb(cams, seed=1, positions=0.0, rotations=0.0, principals=0.0, focals=0.0):
    """std::srand(seed) + Camera::perturbCameras (Camera.cpp:260-280, Camera.h:223-232)"""
    cams = loaded(cams)
    _libc.srand(ctypes.c_uint(seed))

    def perturb(r, amount):
        return r + amount * 2 * (_libc.rand() / float(RAND_MAX) - 0.5)

    out = []
    for i, cam in enumerate(cams):
        cam = dict(cam)
        if i != 0:
            cam["origin"] = [perturb(v, positions) for v in cam["origin"]]
            R = [cam["right"], cam["up"], [-v for v in cam["forward"]]]
            angle, axis = matrix_aa(R)
            if angle > math.pi:
                angle, axis = 2 * math.pi - angle, [-v for v in axis]
            v = [perturb(angle * a, rotations) for a in axis]
            a = _norm(v)
            ax = [1.0, 0.0, 0.0] if a == 0 else [k / a for k in v]
            N = aa_matrix(a, ax)
            cam["right"], cam["up"], cam["forward"] = list(N[0]), list(N[1]), [-k for k in N[2]]
        pr = cam.get("principal", [cam["resolution"][0] / 2, cam["resolution"][1] / 2])
        cam["principal"] = [perturb(pr[0], principals), perturb(pr[1], principals)]
        if focals != 0:
            assert cam["focal"][0] == -cam["focal"][1]
            s = perturb(cam["focal"][0], focals)
            cam["focal"] = [s, -s]
        out.append(cam)
    return out


def rig_scale(cams, scale_rig=1.0, radius=0.0, scale_resolution=1.0):
    """--scale_rig, --radius, --scale_resolution (:538-555, Camera::rescale)"""
    out = []
    for cam in cams:
        cam = _floats(cam)
        if scale_rig != 1:
            cam["origin"] = [v * scale_rig for v in cam["origin"]]
        if radius > 0:
            o = cam["origin"]
            sq = _sum3(o[0] * o[0], o[1] * o[1], o[2] * o[2])
            n = math.sqrt(sq)
            cam["origin"] = [radius * (v / n if sq > 0 else v) for v in o]
        if scale_resolution != 1:
            res = [scale_resolution * v for v in cam["resolution"]]
            q = [res[k] / cam["resolution"][k] for k in range(2)]
            pr = cam.get("principal", [cam["resolution"][0] / 2, cam["resolution"][1] / 2])
            pr = [pr[k] * q[k] for k in range(2)]
            cam["focal"] = [cam["focal"][k] * q[k] for k in range(2)]
            cam["resolution"] = res
            if "principal" in cam or pr != [res[0] / 2, res[1] / 2]:
                cam["principal"] = pr
        out.append(cam)
    return out


def same_camera(a, b):
    """two camera dicts hold the same numbers, bit for bit, and the same id"""
    for k in ("origin", "forward", "up", "right", "resolution", "focal"):
        if [float(v) for v in a[k]] != [float(v) for v in b[k]]:
            return False
    pa = a.get("principal", [a["resolution"][0] / 2, a["resolution"][1] / 2])
    pb = b.get("principal", [b["resolution"][0] / 2, b["resolution"][1] / 2])
    return [float(v) for v in pa] == [float(v) for v in pb] and a["id"] == b["id"]


# ---------------------------------------------------------------- coverage
class Coverage:
    """the rig in its own pixel units on the oracle's camera"""

    def __init__(self, cams):
        from oracle import oracle_lib as O

        self.cams, self.n = [_floats(c) for c in cams], len(cams)
        self.rig = O.Rig(self.cams)

    def count(self, points):
        points = np.ascontiguousarray(points, dtype=F64).reshape(-1, 3)
        total = np.zeros(len(points), dtype=np.int64)
        for i in range(self.n):
            total += self.rig.sees(i, points)[0]
        return total

    def directions(self, units, distances):
        """-> (hist [nd, S + 1] int32, counts [nd, n] uint8): distance * samples[j] (:572)"""
        units = np.asarray(units, dtype=F64).reshape(-1, 3)
        counts = np.stack([self.count(float(d) * units) for d in distances])
        hist = np.stack([np.bincount(c, minlength=self.n + 1) for c in counts]).astype(np.int32)
        return hist, counts.astype(np.uint8)

    def equirect_points(self, ppd, distance):
        W, H = 360 * ppd, 180 * ppd
        lat = [math.pi / 2 - (y + 0.5) / H * math.pi for y in range(H)]
        lon = [-math.pi + (x + 0.5) / W * 2 * math.pi for x in range(W)]
        cl, sl = np.array([math.cos(v) for v in lat]), np.array([math.sin(v) for v in lat])
        co, so = np.array([math.cos(v) for v in lon]), np.array([math.sin(v) for v in lon])
        p = np.stack([cl[:, None] * co[None, :] * distance, cl[:, None] * so[None, :] * distance,
                      np.broadcast_to((sl * distance)[:, None], (H, W))], axis=2)
        return np.ascontiguousarray(p.reshape(-1, 3)), W, H

    def equirect(self, ppd=5, distance=NEAR_INFINITY, pairs="all"):
        """saveEquirect (:376-438) -> (counts [H, W] uint8, min_timing [H, W] float32, (holes, maxMin, aveMin)).
        pairs="all": every pair, as the reference loops. pairs="sorted": neighbours in sorted order only — the same
        minimum, because the rounded difference of two floats grows with the exact one (for rigs of hundreds of cameras;
        tests/test_coverage_ref.py holds the two against each other)"""
        p, W, H = self.equirect_points(ppd, float(distance))
        counts = np.zeros(len(p), dtype=np.int64)
        timing = np.full((self.n, len(p)), np.nan, dtype=F32)
        for i in range(self.n):
            seen, pix = self.rig.sees(i, p)
            timing[i, seen] = (pix[seen, 1] / self.cams[i]["resolution"][1]).astype(F32)
            counts += seen
        best = np.ones(len(p), dtype=F32)
        if pairs == "sorted":
            ordered = np.sort(timing, axis=0)  # (NaN last)
            with np.errstate(invalid="ignore"):
                d = np.abs(ordered[1:] - ordered[:-1])
            assert d.dtype == F32
            if len(d):
                best = np.minimum(best, np.where(np.isnan(d), F32(1), d).min(axis=0))
        for i in range(self.n if pairs == "all" else 0):
            for j in range(i + 1, self.n):
                with np.errstate(invalid="ignore"):
                    d = np.abs(timing[i] - timing[j])
                assert d.dtype == F32
                best = np.where(np.isnan(d), best, np.minimum(best, d))
        m = best.astype(F64)
        stats = (float((counts == 0).sum()), float(max(0.0, m.max())), float(np.cumsum(m)[-1]))  # (cumsum: in order)
        return counts.reshape(H, W).astype(np.uint8), best.reshape(H, W), stats

    def camera(self, cam, distance=NEAR_INFINITY):
        """saveCamera (:346-374) -> counts [h, w] uint8"""
        w, h = int(self.cams[cam]["resolution"][0]), int(self.cams[cam]["resolution"][1])
        pix = np.array([(x + 0.5, y + 0.5) for y in range(h) for x in range(w)], dtype=F64)
        outside = np.array([self.rig.is_outside_image_circle(cam, px, py) for px, py in pix])
        world = self.rig.rig(cam, pix, float(distance))
        counts = np.where(outside, 0, self.count(world))
        return counts.reshape(h, w).astype(np.uint8), outside.reshape(h, w)

    def cross_section(self, dim=400):
        """saveCrossSection (:440-460) -> counts [dim, dim] uint8"""
        p = np.array([(x + 0.5 - 0.5 * dim, y + 0.5 - 0.5 * dim, 0.0) for y in range(dim) for x in range(dim)], dtype=F64)
        return self.count(p).reshape(dim, dim).astype(np.uint8)


# ---------------------------------------------------------------- the tool's text outputs
def report(hist, distances, samples):
    """the sweep's 20 lines on stdout (:261-269, :580-588)"""
    lines = []
    for h, d in zip(hist, distances):
        seen = np.nonzero(h)[0]
        min_c, max_c = int(seen[0]), int(seen[-1])
        quality = min_c + (samples - int(h[min_c])) / float(samples)
        lines.append("distance: %.2f quality: %.2f samples: %d " % (d, quality, samples) +
                     "".join("h[%d] = %d, " % (k, h[k]) for k in range(max_c + 1)))
    return "".join(line + "\n" for line in lines)


def pgm(values, maxval):
    h, w = values.shape
    return "P2\n%d %d\n%d\n" % (w, h, maxval) + "".join("".join("%d " % v for v in row) + "\n" for row in values)


def timed_values(min_timing):
    """int((1.0 - minTimingDiff) * 255.0) (:424)"""
    return ((1.0 - min_timing.astype(F64)) * 255.0).astype(np.int64)


def stats_lines(stats, W, H):
    """the three LOG(INFO) texts (:433-437)"""
    frame_time = float(F32(1000.0) / F32(60.0))
    return ["Holes found (in pixels) = %g" % stats[0], "Max of min timing distance = %gms" % (frame_time * stats[1]),
            "Ave of min timing distance = %gms" % (frame_time * stats[2] / (W * H))]


def rig_obj(cams):
    """saveRigObj (:271-344) of cameras as the tool holds them"""
    out = []

    def axpy(a, s, b):
        return [a[k] + s * b[k] for k in range(3)]

    def face(color, positions):
        for p in positions:
            out.append("v " + " ".join("%g" % v for v in [1000.0 * p[0], 1000.0 * p[1], 1000.0 * p[2]] + list(color)) + "\n")
        n = len(positions)
        for order in range(2):
            out.append("f" + "".join(" %d" % (-n + i if order else -1 - i) for i in range(n)) + "\n")

    def arrow(color, base, direction, t0, t1, length=0.01, radius=0.001):
        face(color, [axpy(base, length, direction), axpy(base, radius, t0), axpy(base, -radius, t0)])
        face(color, [axpy(base, length, direction), axpy(base, radius, t1), axpy(base, -radius, t1)])

    for i, cam in enumerate(cams):
        p, f, r, u = ([float(v) for v in cam[k]] for k in ("origin", "forward", "right", "up"))
        arrow((1, 1, 1), p, f, r, u, 0.02)
        arrow((0, 1, 0), p, r, u, f)
        arrow((0, 0, 1), p, u, f, r)
        for tri in range(i):
            v = axpy(p, -(0.002 * tri), r)
            face((1, 0, 0), [v, axpy(v, -0.002, r), axpy(v, -0.002, u)])
    arrow((1, 1, 0), [0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], 1.0, 0.01)
    return "".join(out)


# ---------------------------------------------------------------- the rigs the tests share
def typed_rig(res=64):
    """one camera of each type — FTHETA whose field exceeds 180 degrees, RECTILINEAR, EQUISOLID, ORTHOGRAPHIC — and an
    FTHETA with the default field, spread over the sphere"""
    from facebook360_dep_amd import synth

    base = synth.make_rig(5, res, layout="fibonacci")["cameras"]
    spec = [("FTHETA", 0.36, 1.9, None), ("RECTILINEAR", 0.50, 0.75, (-0.02, 0.001, 0.0)), ("EQUISOLID", 0.36, 1.4, None),
            ("ORTHOGRAPHIC", 0.52, 1.2, (0.01, 0.0, 0.0)), ("FTHETA", 0.36, None, tuple(synth.DISTORTION))]
    cams = []
    for cam, (kind, f, fov, dist) in zip(base, spec):
        cam = dict(cam, type=kind, focal=[f * res, -f * res])
        cam.pop("fov", None)
        cam.pop("distortion", None)
        if fov is not None:
            cam["fov"] = fov
        if dist is not None:
            cam["distortion"] = list(dist)
        cams.append(cam)
    return cams


def rescaled(cam, w, h):
    """Camera::rescale({w, h}) (Camera.cpp:217-223)"""
    cam = _floats(cam)
    q = [float(w) / cam["resolution"][0], float(h) / cam["resolution"][1]]
    pr = cam.get("principal", [cam["resolution"][0] / 2, cam["resolution"][1] / 2])
    return dict(cam, principal=[pr[k] * q[k] for k in range(2)], focal=[cam["focal"][k] * q[k] for k in range(2)],
                resolution=[float(w), float(h)])


def shared_rigs():
    """name -> cameras: the rigs of tests/test_gpu_coverage.py"""
    from facebook360_dep_amd import synth
    from tests import common

    rig4 = synth.make_rig(4, 64)["cameras"]
    return {
        "rig4": rig4,
        "real": common.real_rig()["cameras"],
        "typed": typed_rig(),
        "one": synth.make_rig(1, 64)["cameras"],
        "revolved40": rig_revolve(rig4, [(0.0, 0.0, 0.1 * k) for k in range(10)]),  # beyond the depth path's 33 cameras
        "small": [rescaled(c, 64, 48) for c in typed_rig()],  # 64 x 48: image circles that end inside the image
    }
