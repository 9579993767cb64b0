"""The cost kernels' trimmed instructions on the device: the two-instruction roundf (round_half_away_pos), the
FOV-cone test of `sees<LEAN>` that settles most lanes with two compares, and the pyramid they feed, each against what
it replaces: numpy's roundf, the oracle's Camera::sees, the oracle's pyramid."""
import math

import numpy as np
import pytest

from tests import common
from tests import cone_cases as CC
from tests import test_round_half_away as RH

pytestmark = pytest.mark.gpu

_REF = {}


def _bits_differ(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return int((a.view(u) != b.view(u)).sum())


def test_round_half_away_on_the_device(built):
    """the helper's instructions (v_add_f32, v_trunc_f32) on the CPU test's boundary set: every bit of numpy's roundf on
    [0, 2^23), a zero on (-0.5, 0)"""
    from facebook360_dep_amd import derp, synth

    x = RH.boundary_set()
    assert 2e5 < x.size < 4e6
    g = derp.Derp(synth.make_rig(2, 64)["cameras"])
    got = g.debug_round_half_away(x)
    nan = g.debug_round_half_away(np.array([np.nan], dtype=np.float32))
    g.close()
    pos = ~np.signbit(x)
    n = _bits_differ(got[pos], RH.roundf(x[pos]))
    print("round_half_away_pos: %d arguments, %d differ from roundf; %d in (-0.5, 0)" % (pos.sum(), n, (~pos).sum()))
    assert n == 0
    assert (got[~pos] == 0).all()
    assert _bits_differ(got, RH.helper(x)) == 0  # and the numpy restatement is the device's arithmetic, sign of zero too
    assert np.isnan(nan[0])


def _cone_case(specs, posed):
    """(cameras, per camera: rig-space points, outcome of the device's form per point or None) for one group"""
    from oracle import oracle_lib as O

    cams = CC.cameras(specs, posed)
    R = O.Rig(cams).normalize()
    rng = np.random.default_rng(180 + posed)
    per_cam = []
    for i in range(R.n):
        st = R.state(i)
        pts = CC.to_rig(st, CC.camera_space_points(st["cos_fov"], rng))
        dot, v = CC.computed_dot(st, pts)
        kind = CC.classify(st["cos_fov"], dot, v) if st["cos_fov"] >= 2.0 ** -100 else None
        per_cam.append((pts, kind))
    return cams, R, per_cam


@pytest.mark.parametrize("posed", [False, True], ids=["eye", "posed"])
def test_cone_test_against_the_oracle(built, posed):
    """six cameras (cos_fov = cos(pi / 2), 0.3, 0.9, exactly 0, -0.2, default), ~2000 points each at depths 0.05 m ..
    10^4 m with dot at 0 and an ulp's scale around it, either side of the accept threshold, and either side of the
    reference's border dot^2 = c^2 |v|^2: visibility equal to the oracle's Camera::sees and the pixel equal bit for bit on
    every point, in both variants the cost kernels project through. The narrow cones' sets reach all three outcomes of
    the device's form (rejected at dot <= 0, accepted past kappa |v|_1, the reference's expression in between)."""
    from facebook360_dep_amd import derp

    cams, R, per_cam = _cone_case(CC.SPECS, posed)
    cos = [R.state(i)["cos_fov"] for i in range(R.n)]
    assert cos[0] == math.cos(math.pi / 2) and abs(cos[1] - 0.3) < 1e-15 and abs(cos[2] - 0.9) < 1e-15
    assert cos[3] == 0.0 and abs(cos[4] + 0.2) < 1e-15 and cos[5] == -1.0
    g = derp.Derp(cams)
    for i, (pts, kind) in enumerate(per_cam):
        assert 1900 <= len(pts) <= 2100
        vis, pix = g.debug_sees(i, pts)
        ovis, opix = R.sees(i, pts)
        if kind is not None:
            counts = [int((kind == k).sum()) for k in (CC.REJECT, CC.ACCEPT, CC.FALL_THROUGH)]
            # (a posed camera's axis is no coordinate axis: past cos_fov |axis|_1 = 1 no direction is accepted outright)
            reachable = cos[i] * CC.KAPPA_MARGIN * np.abs(R.state(i)["R"][2]).sum() < 1
            assert counts[0] > 0 and counts[2] > 0 and (counts[1] > 0) == reachable, (cams[i]["id"], counts)
            # the fall-through decides both ways, and the points it lets through are seen or not by the sensor alone
            dot, v = CC.computed_dot(R.state(i), pts)
            out = CC.reference_outside(cos[i], dot, v)
            assert out[kind == CC.FALL_THROUGH].any() and not out[kind == CC.FALL_THROUGH].all()
            assert not ovis[out].any()
        else:
            counts = None
        opix = np.where(ovis[:, None], opix, np.nan)
        stats = dict(points=len(pts), seen=int(ovis.sum()), outcomes=counts,
                     vis_differ=[int((vis[k] != ovis).sum()) for k in (0, 1)],
                     pix_differ=[_bits_differ(np.where(ovis[:, None], pix[k], np.nan), opix) for k in (0, 1)])
        print(cams[i]["id"], "cos_fov %.17g" % cos[i], stats)
        assert 0 < stats["seen"] < len(pts)
        assert stats["vis_differ"] == [0, 0], (cams[i]["id"], stats)
        assert stats["pix_differ"] == [0, 0], (cams[i]["id"], stats)
    g.close()


def test_cone_test_ftheta(built):
    """the same cones on FTHETA cameras, the bench rig's type. Its projection goes through the kernels' own atan2, which
    is within an ulp of libm's and not equal to it, so the pixel is held to test_projection_variants' 2 ulps and the
    visibility to the oracle's wherever the pixel is not within 1e-9 of the image's edge; the two variants agree bit for
    bit everywhere."""
    from facebook360_dep_amd import derp

    for posed in (False, True):
        cams, R, per_cam = _cone_case(CC.ftheta_specs(), posed)
        g = derp.Derp(cams)
        for i, (pts, kind) in enumerate(per_cam):
            vis, pix = g.debug_sees(i, pts)
            ovis, opix = R.sees(i, pts)
            assert (vis[0] == vis[1]).all() and _bits_differ(pix[0], pix[1]) == 0
            with np.errstate(invalid="ignore"):
                edge = ((np.abs(opix) < 1e-9) | (np.abs(opix - 1.0) < 1e-9)).any(1)
            differ = (vis[0] != ovis) & ~edge
            both = vis[0] & ovis
            ulp = np.abs(pix[0][both] - opix[both]) / np.spacing(np.maximum(np.abs(opix[both]), 0.5))
            print(cams[i]["id"], "points %d seen %d vis differ %d pix ulps max %.2f" % (len(pts), ovis.sum(), differ.sum(), ulp.max()))
            assert 0 < ovis.sum() < len(pts)
            assert not differ.any(), (cams[i]["id"], pts[differ][:4])
            assert ulp.max() <= 2.0
        g.close()


def _pyramid_case(name):
    from facebook360_dep_amd import synth

    if name not in _REF:
        res = 64
        fov = math.acos(0.3) if name == "c0.3" else math.pi / 2
        rig = synth.make_rig(4, res, fov=fov)
        sizes = synth.level_sizes(res, res, [64, 50])
        frame = synth.make_frame(rig, sizes)
        ref = common.oracle_pyramid(rig, sizes, frame, res, res, partial_coverage=True)
        _REF[name] = dict(rig=rig, sizes=sizes, frame=frame, res=res, ref=ref)
    return _REF[name]


@pytest.mark.parametrize("name", ["c0.3", "default_fov"])
def test_pyramid_against_the_oracle(built, name):
    """a 4-camera 64^2 rig, the smallest the cost core runs, with cos_fov = 0.3 (the band between the cone and
    dot = kappa |v|_1 is wide: many lanes evaluate the reference's expression) and with the synthetic rigs' default
    fov = pi / 2 (next to none do): every level's disparities against the oracle's pyramid, no value differing, neither by
    the suite's measure (more than 1e-4 relative, or NaN on one side only) nor in a bit"""
    from facebook360_dep_amd import derp
    from oracle import oracle_lib as O

    case = _pyramid_case(name)
    cams = case["rig"]["cameras"]
    want = 0.3 if name == "c0.3" else math.cos(math.pi / 2)
    assert abs(O.Rig(cams).normalize().state(0)["cos_fov"] - want) < 1e-15
    g = derp.Derp(cams, partial_coverage=1)
    g.set_pyramid(case["sizes"], case["res"], case["res"])
    g.upload_frame({"color": case["frame"]["color"]})
    g.process_pyramid()
    g.synchronize()
    counters = g.counters()
    stats = {}
    for level in sorted(case["ref"]):
        bad = bits = finite = 0
        for d in range(len(cams)):
            got = g.download_disparity(level, d)
            bad += common.compare_disparity(got, case["ref"][level][d])[0]
            bits += common.bit_equal(got, np.asarray(case["ref"][level][d], dtype=np.float32))
            finite += int(np.isfinite(got).sum())
        stats[level] = dict(differ=bad, bits_differ=bits, finite=finite)
    g.close()
    print(name, stats, counters)
    assert counters["n_pair"] > 0
    for level, s in stats.items():
        assert s["finite"] > 0, (name, level)
        assert s["differ"] == 0 and s["bits_differ"] == 0, (name, level, s)
