"""Device probes of the cost core's fp64 primitives (derp_debug_fp64, derp_debug_sees).

sqrt_lean and div_plain (csrc/derp_camera.h) restate the compiler's own expansions without their literals and fix-ups;
the cost kernels' speed rests on them. Ping-pong takes its candidate 0 from random proposals' cost (the memo), and the
two kernels project through different variants of `sees`: random proposals through sqrt_lean, the others through
sqrt(). Both must give the same bits, and both must be the correctly rounded IEEE result on the domains the comments
state. Bulk inputs use numpy (IEEE sqrt / division on the host); the hard cases decide correct rounding with exact
rational arithmetic."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(built):
    from facebook360_dep_amd import derp, synth

    g = derp.Derp(synth.make_rig(2, 64)["cameras"])
    yield g
    g.close()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _from_bits(b):
    return np.ascontiguousarray(b, np.uint64).view(np.float64)


def _same_bits(a, b):
    """count of elements whose bits differ, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))
    return int((~same).sum())


def _binades(rng, per):
    """`per` random mantissas in every binade of the positive doubles: the 52 subnormal ones (top mantissa bit k) and
    the biased exponents 1..2046"""
    out = [np.uint64(1 << k) | (rng.integers(0, 1 << k, per, dtype=np.uint64) if k else np.zeros(per, np.uint64))
           for k in range(52)]
    for e in range(1, 2047):
        out.append((np.uint64(e) << np.uint64(52)) | rng.integers(0, 1 << 52, per, dtype=np.uint64))
    return _from_bits(np.concatenate(out))


def _ulp_steps(x, k):
    """x moved by -k..k units in the last place (through the bit pattern: crosses binades exactly); x > 0"""
    b = _bits(np.asarray(x, np.float64)).astype(np.int64)
    return _from_bits(np.concatenate([b + s for s in range(-k, k + 1)]).astype(np.uint64))


def _sqrt_correct(x, y):
    """exact: y is sqrt(x) rounded to nearest (x > 0 finite) iff x lies inside y's rounding interval squared (a
    midpoint squared needs more than 53 bits, so there are no ties)"""
    fy, fx = Fraction(y), Fraction(x)
    lo = (fy + Fraction(math.nextafter(y, 0.0))) / 2
    hi = (fy + Fraction(math.nextafter(y, math.inf))) / 2
    return lo * lo < fx < hi * hi


def _sqrt_mod_2k(c, k):
    """r with r^2 = c (mod 2^k), c = 1 (mod 8) (Hensel lifting: r or r + 2^(i-1) carries a root mod 2^i one bit on)"""
    r = 1
    for i in range(3, k):
        if (r * r - c) % (1 << (i + 1)):
            r += 1 << (i - 1)
    return r


def _sqrt_hard_cases(rng):
    out = []
    # perfect squares (k^2 < 2^53 is exact) moved through the binades by powers of 4, and their neighbours
    k = rng.integers(1, 94906265, 2048).astype(np.float64)
    sq = k * k * np.ldexp(1.0, 2 * rng.integers(-500, 480, 2048))
    out += [sq, _ulp_steps(sq, 3)]
    # roots next to a rounding midpoint (the cases a short correction sequence gets wrong): for an odd s in
    # [2^53, 2^53.5) with s^2 = c (mod 2^54), c = +-(1 + 8 j) small, x = (s^2 - c) / 4 is a double and its root
    # s / 2 - c / (4 s) lies about c 2^-55 ulp below (c > 0) or above (c < 0) the midpoint s / 2 of two doubles
    mids = []
    for j in range(1, 4096):
        for c in (1 + 8 * j, -(7 + 8 * j)):
            s = _sqrt_mod_2k(c % (1 << 54), 54)
            s = min(v % (1 << 54) for v in (s, -s, s + (1 << 53), (1 << 53) - s) if (1 << 53) <= v % (1 << 54))
            x = Fraction(s * s - c, 4)
            if float(x) == x:
                mids.append(float(x * Fraction(4) ** int(rng.integers(-250, 250))))
    mids = np.array(mids)
    assert mids.size >= 2048
    out += [mids, _ulp_steps(mids, 2)]
    # the scaling threshold of sqrt_lean and of the compiler's expansion, 2^-767, a few ulps each way
    out.append(_ulp_steps(np.array([2.0 ** -767, 2.0 ** -766, 2.0 ** -768]), 8))
    # the extremes
    out.append(np.array([5e-324, 1e-323, 2.0 ** -1022, np.nextafter(2.0 ** -1022, 0), np.finfo(np.float64).max, 1.0, 4.0]))
    return np.concatenate(out)


def test_sqrt_lean_is_ieee_sqrt(probe):
    """sqrt_lean == sqrt() == IEEE sqrt, bit for bit, over every binade, the scaling threshold, perfect squares, roots
    next to rounding midpoints and the special values (+-0 keep their sign, +inf, NaN for negative and NaN inputs)."""
    rng = np.random.default_rng(2026)
    bulk = np.concatenate([_binades(rng, 512), _ulp_steps(np.array([2.0 ** -767]), 64),
                           np.ldexp(rng.uniform(0.5, 1.0, 4096), rng.integers(-770, -764, 4096))])
    hard = _sqrt_hard_cases(rng)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, -1.0, -5e-324, -np.finfo(np.float64).max, -2.0 ** -767])
    x = np.concatenate([bulk, hard, special])
    assert bulk.size >= 1 << 20
    lean, plain = probe.debug_fp64("sqrt_lean", x), probe.debug_fp64("sqrt", x)
    assert _same_bits(lean, plain) == 0, x[_bits(lean) != _bits(plain)][:8]
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)
    assert _same_bits(lean, want) == 0, x[_bits(lean) != _bits(want)][:8]
    # the hard cases, independently of any libm
    h = lean[bulk.size:bulk.size + hard.size]
    wrong = [float(a) for a, b in zip(hard, h) if not _sqrt_correct(float(a), float(b))]
    assert not wrong, wrong[:8]
    s = lean[-special.size:]
    assert _bits(s[0]) == _bits(0.0) and _bits(s[1]) == _bits(-0.0) and s[2] == np.inf
    assert np.isnan(s[3:]).all()
    print("sqrt_lean: %d arguments (%d hard cases) bit-equal to sqrt() and to IEEE sqrt" % (x.size, hard.size))


def _div_domain(rng, n):
    """random (num, den) on div_plain's stated domain: 2^-968 <= |num| < 2^1023, 2^-1021 <= |den| < 2^1021,
    2^-1000 <= |num / den| < 2^766 (held on the exponents; mantissas and signs random)"""
    en = rng.integers(-968, 1023, 4 * n)
    ed = rng.integers(-1021, 1021, 4 * n)
    keep = (en - ed >= -999) & (en - ed <= 765)
    en, ed = en[keep][:n], ed[keep][:n]
    assert en.size == n

    def make(e):
        sign = rng.integers(0, 2, e.size, dtype=np.uint64) << np.uint64(63)
        return _from_bits(sign | ((e + 1023).astype(np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, e.size, dtype=np.uint64))

    return make(en), make(ed)


def _div_hard_cases(rng):
    nums, dens = [], []
    # divisors with all-ones mantissas (the reciprocal's worst start), any binade of the domain
    e = rng.integers(-900, 900, 4096)
    dens.append(_from_bits(((e + 1023).astype(np.uint64) << np.uint64(52)) | np.uint64((1 << 52) - 1)))
    nums.append(np.ldexp(rng.uniform(1.0, 2.0, 4096), rng.integers(-60, 60, 4096)) * np.sign(rng.normal(size=4096)))
    # quotients next to a rounding midpoint: for an odd 53-bit den D and an odd s in [2^53, 2^54) with s D = c
    # (mod 2^54), c small, num = (s D - c) / 2 is a double and num / den = s / 2 - c / (2 D) lies about c 2^-53 ulp
    # from the midpoint s / 2 of two doubles (then both scaled by powers of two)
    mid_n, mid_d = [], []
    while len(mid_n) < 4096:
        dd = int(rng.integers(1 << 52, 1 << 53)) | 1
        c = int(rng.integers(1, 64)) * int(rng.choice([-1, 1]))
        s = c * pow(dd, -1, 1 << 54) % (1 << 54)
        if s >> 53 == 1:
            a, b = (int(v) for v in rng.integers(-300, 300, 2))
            mid_n.append(math.ldexp(float((s * dd - c) // 2), a))
            mid_d.append(math.ldexp(float(dd), b))
    nums.append(np.array(mid_n))
    dens.append(np.array(mid_d))
    n, d = np.concatenate(nums), np.concatenate(dens)
    # and the numerators' neighbours
    steps = _bits(np.abs(n)).astype(np.int64)
    near = [_from_bits((steps + s).astype(np.uint64)) * np.sign(n) for s in (-1, 1)]
    return np.concatenate([n] + near), np.concatenate([d, d, d])


def test_div_plain_is_ieee_division(probe):
    """div_plain == IEEE division (== the compiler's `/`) bit for bit on the domain derp_camera.h states, including
    n = +0; then its edge: a zero divisor and |den| below 2^-1025 give NaN (the reciprocal overflows), n = -0 gives +0,
    and what happens at divisors near 2^-1022 and for tiny numerators is counted and pinned."""
    rng = np.random.default_rng(1022)
    bn, bd = _div_domain(rng, 1 << 20)
    hn, hd = _div_hard_cases(rng)
    zd = np.ldexp(rng.uniform(1.0, 2.0, 256), rng.integers(-1000, 1000, 256)) * np.sign(rng.normal(size=256))
    n = np.concatenate([bn, hn, np.zeros(256)])
    d = np.concatenate([bd, hd, zd])
    got, comp = probe.debug_fp64("div_plain", n, d), probe.debug_fp64("div", n, d)
    want = n / d
    assert _same_bits(comp, want) == 0  # the compiler's division is IEEE here: the yardstick itself
    bad = _bits(got) != _bits(want)
    assert _same_bits(got, want) == 0, (n[bad][:4], d[bad][:4])
    k = bn.size
    wrong = [(a, b) for a, b, q in zip(hn.tolist(), hd.tolist(), got[k:k + hn.size].tolist())
             if q != float(Fraction(a) / Fraction(b))]
    assert not wrong, wrong[:4]
    # ---- the edge of the domain
    neg0 = probe.debug_fp64("div_plain", np.full(256, -0.0), zd)
    assert (neg0 == 0).all() and not np.signbit(neg0).any()  # -0 / d: +0 for either sign of d (IEEE: -0 for d > 0)
    tiny_d = np.concatenate([-_from_bits(rng.integers(1, 1 << 49, 1024, dtype=np.uint64)),
                             _from_bits(rng.integers(1, 1 << 49, 1024, dtype=np.uint64)), [0.0, -0.0]])
    tiny_n = np.concatenate([tiny_d[:-2] * rng.uniform(0.5, 2.0, 2048), [1.0, 1.0]])
    assert np.isnan(probe.debug_fp64("div_plain", tiny_n, tiny_d)).all()  # the reciprocal is inf: NaN, not n / d
    # divisors at 2^-1024 .. 2^-1021 and a few ulps either side, numerators around them
    near_d = _ulp_steps(np.array([2.0 ** -1021, 2.0 ** -1022, 2.0 ** -1023, 2.0 ** -1024]), 16)
    near_d = np.concatenate([near_d, -near_d])
    near_n = np.concatenate([near_d * f for f in (1.0, 0.75, 1.5, 2.0 ** 40)])
    near_dd = np.tile(near_d, 4)
    near = probe.debug_fp64("div_plain", near_n, near_dd)
    # numerators below 2^-968 over ordinary divisors: the residual can underflow
    small_n = np.ldexp(rng.uniform(1.0, 2.0, 4096), rng.integers(-1070, -968, 4096))
    small_d = np.ldexp(rng.uniform(1.0, 2.0, 4096), rng.integers(-60, 2, 4096))
    small = probe.debug_fp64("div_plain", small_n, small_d)
    counts = {"near_2^-1022": _same_bits(near, near_n / near_dd), "near_2^-1022_nan": int(np.isnan(near).sum()),
              "tiny_numerator": _same_bits(small, small_n / small_d)}
    print("div_plain outside its domain (results not bit-equal to IEEE):", counts)
    common.observed("fp64_primitives.div_plain_edge", counts)


# ---- projection variants ------------------------------------------------------------------------------------------
def _identity_posed(cams):
    """the cameras' intrinsics at the origin, looking down -z (rotation exactly the identity): camera space = rig space,
    so edge points can be written down in camera coordinates"""
    return [dict(c, id=c["id"] + "_eye", origin=[0.0, 0.0, 0.0], forward=[0.0, 0.0, -1.0], up=[0.0, 1.0, 0.0],
                 right=[1.0, 0.0, 0.0]) for c in cams]


def _ray_points(R, i, rng, per):
    """points along the other cameras' pixel rays, disparities 0.01..5 / m (the default depth range and beyond)"""
    j = rng.integers(0, R.n - 1, per)
    j = j + (j >= i)
    pts = np.empty((per, 3))
    pix = rng.uniform(0.0, 1.0, (per, 2))
    depth = 1.0 / rng.uniform(0.01, 5.0, per)
    for cam in np.unique(j):
        sel = j == cam
        pts[sel] = R.rig(int(cam), pix[sel], depth[sel])
    return pts


def _edge_points(R, i, rng):
    """points that project onto the image edges: camera i's pixels at exactly 0 and a few ulps under 1 (normalised)
    unprojected with the oracle, then moved by ulps"""
    per = 64
    under = 1.0 - 2.0 ** -53 * rng.integers(1, 4, per)
    px = np.concatenate([np.zeros(per), under, rng.uniform(0, 1, 2 * per)])
    py = np.concatenate([rng.uniform(0, 1, 2 * per), np.zeros(per), under])
    pts = R.rig(i, np.stack([px, py], 1), 1.0 / rng.uniform(0.05, 2.0, px.size))
    return np.concatenate([pts * (1 + s * 2.0 ** -52) for s in (-2, -1, 0, 1, 2)])


def _eye_points(cam, rng):
    """camera-space edge points of an identity-posed camera: the optical axis (xy == 0), tiny and subnormal xy, the
    image plane (camera-space z == 0, both signs), and a few ulps either side of the FOV cone"""
    m = 64
    z = -np.ldexp(rng.uniform(1.0, 2.0, m), rng.integers(-8, 8, m))
    a = rng.uniform(0, 2 * np.pi, m)
    pts = [np.stack([np.zeros(m), np.zeros(m), z], 1)]
    for e in (-30, -200, -1000, -1060):
        xy = np.ldexp(rng.uniform(1.0, 2.0, m), e)
        pts.append(np.stack([xy * np.cos(a), xy * np.sin(a), z], 1))
    pts.append(np.stack([np.cos(a), np.sin(a), np.zeros(m)], 1))
    pts.append(np.stack([np.cos(a), np.sin(a), np.full(m, -0.0)], 1))
    if "fov" in cam:
        for s in range(-4, 5):
            th = cam["fov"] * (1 + s * 2.0 ** -50)
            pts.append(np.stack([np.sin(th) * np.cos(a), np.sin(th) * np.sin(a), -np.cos(th) * np.ones(m)], 1))
    return np.concatenate(pts)


def _band(pts, st, opix, gpix):
    """where vis may differ by rounding: a pixel within 1e-9 of the image edge (either side's pixel), a point within
    1e-9 (relative) of the FOV cone, or of the camera's image plane"""
    edge = np.zeros(len(pts), bool)
    with np.errstate(invalid="ignore"):
        for p in (opix, gpix):
            edge |= (np.abs(p) < 1e-9).any(1) | (np.abs(p - 1.0) < 1e-9).any(1)
    v = pts - st["position"]
    back = v @ st["R"][2]
    c = st["cos_fov"]
    sq = (v * v).sum(1)
    cone = np.abs(-back * np.abs(back) - c * abs(c) * sq) <= 1e-9 * sq
    return edge | cone | (np.abs(back) <= 1e-9 * np.sqrt(sq))


@pytest.mark.parametrize("rig_name", ["ftheta33", "mixed"])
def test_projection_variants(built, rig_name):
    """(i) the ping-pong / brute-force and the random-proposal variants of `sees` agree bit for bit (vis, pix; NaN ==
    NaN) on every input: the memo invariant at the source. (ii) against the oracle's Camera::sees: vis equal away from
    the image-edge / cone band (the band's disagreements are counted and pinned), the fp64 pixel within a few ulps, the
    float pixel the kernels form ((float)(pn.x * W)) equal except for a pinned count."""
    from facebook360_dep_amd import derp, synth
    from oracle import oracle_lib as O

    rng = np.random.default_rng(33 if rig_name == "ftheta33" else 6)
    if rig_name == "ftheta33":
        cams, res, per = synth.make_rig(33, 128)["cameras"], 128, 1 << 15
    else:
        cams, res, per = common.mixed_type_rig(120)["cameras"], 120, 1 << 18
    eyes = _identity_posed(cams[:2] if rig_name == "ftheta33" else cams)
    stats = dict(points=0, band=0, vis_differ_in_band=0, nan_pixel_differ=0, pix_ulp_max=0.0, pix_over_1ulp=0,
                 float_pix_differ=0)
    for rig, eye in ((cams, False), (eyes, True)):
        g = derp.Derp(rig)
        R = O.Rig(rig).normalize()
        for i in range(R.n):
            pts = [_edge_points(R, i, rng)] + ([_eye_points(rig[i], rng)] if eye else [_ray_points(R, i, rng, per)])
            pts = np.concatenate(pts)
            vis, pix = g.debug_sees(i, pts)
            ovis, opix = R.sees(i, pts)
            st = R.state(i)
            stats["points"] += len(pts)
            # (i) the memo invariant: a hard equality
            assert (vis[0] == vis[1]).all(), (rig_name, eye, i, int((vis[0] != vis[1]).sum()))
            assert _same_bits(pix[0], pix[1]) == 0, (rig_name, eye, i)
            # (ii) against the oracle
            band = _band(pts, st, opix, pix[0])
            differ = vis[0] != ovis
            assert not (differ & ~band).any(), (rig_name, eye, i, pts[differ & ~band][:4])
            stats["band"] += int(band.sum())
            stats["vis_differ_in_band"] += int((differ & band).sum())
            seen = vis[0] & ovis
            stats["nan_pixel_differ"] += int((seen & (np.isnan(pix[0]).any(1) != np.isnan(opix).any(1))).sum())
            both = seen & np.isfinite(opix).all(1) & np.isfinite(pix[0]).all(1)
            if both.any():
                # in ulps of the pixel, but at least of 0.5: every pixel is formed by adding the principal point
                ulp = np.abs(pix[0][both] - opix[both]) / np.spacing(np.maximum(np.abs(opix[both]), 0.5))
                stats["pix_ulp_max"] = max(stats["pix_ulp_max"], float(ulp.max()))
                stats["pix_over_1ulp"] += int((ulp > 1).sum())
                fg = (pix[0][both] * float(res)).astype(np.float32)
                fo = (opix[both] * float(res)).astype(np.float32)
                stats["float_pix_differ"] += int((fg != fo).any(1).sum())
        g.close()
    print("%s: %s" % (rig_name, stats))
    assert stats["points"] >= 1 << 20
    assert stats["pix_ulp_max"] <= 2.0  # measured on the MI355X: 2 ulps (of 0.5 at least) for both rigs
    common.observed("fp64_primitives.projection." + rig_name, stats)
