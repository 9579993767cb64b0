"""Cameras and points for the cost kernels' FOV-cone test (`sees<LEAN>`, csrc/derp_camera.h): six cos_fov values, points
on and around the three outcomes' borders, and a numpy restatement of the device's classification and of the
reference's expression. Shared by tests/test_cone_lemmas.py (CPU) and tests/test_gpu_cost_trims.py."""
import math

import numpy as np

RES = 64
KAPPA_MARGIN = 1.0 + 2.0 ** -20
REJECT, ACCEPT, FALL_THROUGH = 0, 1, 2

# (name, type, normalised focal, fov). The types are the ones whose projection is square roots and divisions only:
# correctly rounded on the device and on the host, so the oracle's pixel can be asked for bit for bit (FTHETA's
# atan2 is within an ulp of libm's, not equal to it: ftheta_specs below). cos_fov exactly 0 is RECTILINEAR's default.
SPECS = [
    ("half_pi", "EQUISOLID", 0.30, math.pi / 2),      # cos(pi / 2) in double: 6.1e-17, the bench rig's value
    ("c0.3", "EQUISOLID", 0.30, math.acos(0.3)),
    ("c0.9", "RECTILINEAR", 0.50, math.acos(0.9)),
    ("zero", "RECTILINEAR", 0.50, None),              # cos_fov == 0: isBehind
    ("c-0.2", "EQUISOLID", 0.30, math.acos(-0.2)),
    ("default", "EQUISOLID", 0.30, None),             # cos_fov == -1: no test
]


def ftheta_specs():
    return [(name, "FTHETA", 0.30, fov) for name, _, _, fov in SPECS if fov is not None] + [("default", "FTHETA", 0.30, None)]


def cameras(specs, posed):
    """the six cameras: identity-posed at the origin (camera space = rig space, dot = -v.z exactly), or on an arc"""
    from facebook360_dep_amd import synth

    base = synth.make_rig(len(specs), RES, layout="arc")["cameras"]
    cams = []
    for cam, (name, kind, f, fov) in zip(base, specs):
        cam = dict(cam, id="cone_" + name + ("_posed" if posed else "_eye"), type=kind, focal=[f * RES, -f * RES])
        cam.pop("fov", None)
        cam.pop("distortion", None)
        if fov is not None:
            cam["fov"] = fov
        if not posed:
            cam.update(origin=[0.0, 0.0, 0.0], forward=[0.0, 0.0, -1.0], up=[0.0, 1.0, 0.0], right=[1.0, 0.0, 0.0])
        cams.append(cam)
    return cams


def _ulps(x, k):
    """x moved by k ulps (k an integer array), away from zero for k > 0; x != 0"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return (b + k).view(np.float64)


def camera_space_points(cos_fov, rng, per=500):
    """~4 `per` camera-space points (camera looks down -z), |v| log-uniform in 0.05 m .. 10^4 m:
    dot = -z at 0 and an ulp's scale either side; either side of the accept threshold dot = kappa |v|_1; either side of
    the reference's own border dot^2 = c^2 |v|^2; and directions all over the sphere"""
    c = float(cos_fov)

    def shell(n):
        a = rng.uniform(0, 2 * np.pi, n)
        return np.exp(rng.uniform(np.log(0.05), np.log(1e4), n)), np.cos(a), np.sin(a)

    out = []
    # dot around 0: exact zeros of both signs, the smallest doubles, and fractions of an ulp of |v| down to 2^-70 |v|
    r, ca, sa = shell(per)
    m = per // 8
    z = np.concatenate([np.full(m, s * t) for t in (0.0, 5e-324, 2.0 ** -1022) for s in (1.0, -1.0)])
    rest = per - z.size
    sign = rng.choice([-1.0, 1.0], rest)
    z = np.concatenate([z, sign * np.ldexp(r[per - rest:], -rng.integers(45, 71, rest))])
    out.append(np.stack([r * ca, r * sa, z], 1))
    # the accept threshold: dot (1 - kappa) = kappa (|x| + |y|), moved by -4 .. 4 ulps
    if 0 < c < 1:
        kappa = c * KAPPA_MARGIN
        r, ca, sa = shell(per)
        x, y = r * ca, r * sa
        dot = kappa * (np.abs(x) + np.abs(y)) / (1 - kappa)
        out.append(np.stack([x, y, -_ulps(dot, rng.integers(-4, 5, per))], 1))
    # the reference's border: v on the cone, dot = c |v|, i.e. -z = r c / sqrt(1 - c^2), moved by -4 .. 4 ulps
    if -1 < c < 1 and c != 0:
        r, ca, sa = shell(per)
        dot = r * c / math.sqrt(1 - c * c)
        out.append(np.stack([r * ca, r * sa, -_ulps(dot, rng.integers(-4, 5, per))], 1))
    # next to the optical axis, where |v|_1 is smallest against dot
    r, ca, sa = shell(per // 4)
    off = r * 10.0 ** rng.uniform(-9, -1, per // 4)
    out.append(np.stack([off * ca, off * sa, -r], 1))
    # anywhere
    n = 4 * per - sum(len(p) for p in out)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out.append(d * np.exp(rng.uniform(np.log(0.05), np.log(1e4), n))[:, None])
    return np.concatenate(out)


def to_rig(state, cam_pts):
    """camera-space points -> rig space with the camera's rotation (rows right, up, backward) and position"""
    return cam_pts @ state["R"] + state["position"]


def computed_dot(state, pts):
    """forward().dot(v) as `sees` computes it: -(b.x v.x + (b.y v.y + b.z v.z)), one IEEE operation each"""
    v = pts - state["position"]
    b = state["R"][2]
    return -(b[0] * v[:, 0] + (b[1] * v[:, 1] + b[2] * v[:, 2])), v


def reference_outside(cos_fov, dot, v):
    """Camera::isOutsideFov's expression (Camera.h:154-164) on the computed dot"""
    sq = v[:, 0] * v[:, 0] + (v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return dot * np.abs(dot) <= cos_fov * abs(cos_fov) * sq


def classify(cos_fov, dot, v):
    """the outcome the device's narrow-cone form reaches for each point (cos_fov >= 2^-100): REJECT / ACCEPT /
    FALL_THROUGH"""
    kappa = cos_fov * KAPPA_MARGIN
    t = kappa * (np.abs(v[:, 0]) + (np.abs(v[:, 1]) + np.abs(v[:, 2])))
    out = np.full(len(dot), FALL_THROUGH)
    out[dot > t] = ACCEPT
    out[dot <= 0] = REJECT
    return out
