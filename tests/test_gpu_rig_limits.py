"""The cost core at the limits of the rig sizes the API accepts (2 to 33 cameras: kMaxSrc = 32 sources per cost) against
the CPU oracle, and the memo invariant at pyramid level.

- 2 cameras: one source (keep = 1, costs without a pair, the spare pair slot is slot 1); also brute force alone;
- 3 cameras: two sources;
- 17 cameras: the smallest rig on the three-wave `_w3` cost kernels, bit-equal to the four-wave ones;
- 33 cameras: 32 sources, every bit of the 32-bit source masks (the behind table, the wave cull mask, compute_cost's
  mask / waveMask, the compacted ping-pong's cull loop), under every loop shape, register budget and batching;
- 34 cameras: refused.
Ping-pong's candidate 0 is served from random proposals' cost (the memo); DERP_NO_MEMO=1 recomputes it. The oracle always
recomputes, so only a bitwise comparison of the two runs shows that the memo is exact."""
import os

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

TOL = 1e-4
_CASES = {}
_DEFAULT_RUNS = {}


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _case(name):
    """the rigs of this file, rendered once: 'small' (6 cameras), 'mixed' (test_camera_types' rig) or a camera count"""
    from facebook360_dep_amd import synth

    if name not in _CASES:
        if name == "small":
            n, res, widths = synth.config("small")
            rig, sizes, opts = synth.make_rig(n, res), synth.level_sizes(res, res, widths), dict(partial_coverage=1)
        elif name == "mixed":
            n, res = 6, 120
            rig, sizes, opts = common.mixed_type_rig(res), [(120, 120), (80, 80), (50, 50)], dict(partial_coverage=1)
        else:
            n = int(name)
            res = 96 if n >= 33 else 128
            rig, sizes = synth.make_rig(n, res), synth.level_sizes(res, res, [res, 80, 50])
            opts = dict(partial_coverage=1) if n <= 3 else {}
        frame = synth.make_frame(rig, sizes, with_masks=(name == "33"))
        _CASES[name] = dict(rig=rig, sizes=sizes, frame=frame, res=res, n=n, opts=opts)
    return _CASES[name]


def _gpu(case, monkeypatch, env=(), sizes=None, **opts):
    """one pyramid on the device -> disparities of every level and destination, counters, level-0 ping-pong batches and
    the ping-pong costs served from the memo"""
    from facebook360_dep_amd import derp

    for k, v in env:
        monkeypatch.setenv(k, v)
    sizes = sizes or case["sizes"]
    o = dict(case["opts"], **opts)
    g = derp.Derp(case["rig"]["cameras"], **o)
    g.set_pyramid(sizes, case["res"], case["res"])
    g.upload_frame(case["frame"] if o.get("use_foreground_masks") else {"color": case["frame"]["color"]})
    g.profile_reset()
    g.profile_enable(True)
    g.process_pyramid()
    g.synchronize()
    run = dict(out=[[g.download_disparity(level, d) for d in range(case["n"])] for level in range(len(sizes))],
               counters=g.counters(), batches=g.profile_query("ping_pong", 0)["launches"],
               memo=g.profile_memoised("ping_pong"))
    g.close()
    for k, _ in env:
        monkeypatch.delenv(k)
    return run


def _default_run(name, monkeypatch):
    if name not in _DEFAULT_RUNS:
        _DEFAULT_RUNS[name] = _gpu(_case(name), monkeypatch)
    return _DEFAULT_RUNS[name]


def _differ(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def _assert_bit_equal(a, b, what):
    assert a["counters"] == b["counters"], what
    for level, (x, y) in enumerate(zip(a["out"], b["out"])):
        for d, (p, q) in enumerate(zip(x, y)):
            assert _differ(p, q) == 0, (what, level, d)


def _against_oracle(case, run, key, sizes=None, **opts):
    """every level and destination within 1e-4 of the oracle (the pixels outside pinned), n_cost equal, n_pair within
    test_sixteen_camera_rig_full_pyramid's tolerance (the difference pinned)"""
    sizes = sizes or case["sizes"]
    o = {k: bool(v) for k, v in dict(case["opts"], **opts).items()}
    cnt = {}
    ref = common.oracle_pyramid(case["rig"], sizes, case["frame"], case["res"], case["res"], counters=cnt,
                                threads=_threads(), **o)
    stats, npx = {}, 0
    for level in sorted(ref):
        nbad = 0
        for d in range(case["n"]):
            bad, _ = common.compare_disparity(run["out"][level][d], ref[level][d], TOL)
            nbad += bad
            npx += ref[level][d].size
        stats[str(level)] = nbad
    got = run["counters"]
    n_cost = sum(c["n_cost"] for c in cnt.values())
    n_pair = sum(c["n_pair"] for c in cnt.values())
    print("%s: pixels outside 1e-4 per level %s of %d; n_cost %d / %d, n_pair %d / %d" % (
        key, stats, npx, got["n_cost"], n_cost, got["n_pair"], n_pair))
    assert sum(stats.values()) <= 1e-4 * npx, (key, stats)
    assert got["n_cost"] == n_cost
    assert abs(got["n_pair"] - n_pair) <= 1e-6 * n_pair + 4
    stats["n_pair_diff"] = got["n_pair"] - n_pair
    common.observed("rig_limits." + key, stats)
    return ref


@pytest.mark.parametrize("n", [2, 3])
def test_one_and_two_sources_against_oracle(built, monkeypatch, n):
    case = _case(str(n))
    run = _default_run(str(n), monkeypatch)
    assert run["counters"]["n_cost"] > 0
    _against_oracle(case, run, "cams%d.128" % n)


def test_one_source_brute_force_only(built, monkeypatch):
    """a single-level pyramid: brute force over the 150 disparities with one source, nothing after it"""
    case = _case("2")
    sizes = case["sizes"][:1]
    run = _gpu(case, monkeypatch, sizes=sizes)
    _against_oracle(case, run, "cams2.128.brute_force", sizes=sizes)


def test_seventeen_cameras_three_wave_kernels(built, monkeypatch):
    """17 cameras: the default launches the `_w3` kernels; forced four-wave and three-wave runs are bit-equal to it"""
    case = _case("17")
    run = _default_run("17", monkeypatch)
    _against_oracle(case, run, "cams17.128")
    for waves in ("4", "3"):
        _assert_bit_equal(run, _gpu(case, monkeypatch, env=[("DERP_COST_WAVES", waves)]), "DERP_COST_WAVES=" + waves)


def test_thirty_three_cameras_against_oracle(built, monkeypatch):
    """32 sources per cost; the source in slot 31 (the top bit of every mask) really sees the final level-0 points"""
    from oracle import oracle_lib as O

    case = _case("33")
    run = _default_run("33", monkeypatch)
    _against_oracle(case, run, "cams33.96")
    rs = O.Rig(case["rig"]["cameras"]).normalize()
    w, h = case["sizes"][0]
    ys, xs = np.mgrid[0:h, 0:w]
    pix = np.stack([(xs + 0.5) / w, (ys + 0.5) / h], -1).reshape(-1, 2)
    hits = []
    for d in range(33):
        top = 32 if d < 32 else 31  # slot(s, own) = s - (s > own): slot 31 is camera 32, or camera 31 for camera 32
        disp = run["out"][0][d].reshape(-1).astype(np.float64)
        ok = np.isfinite(disp) & (disp > 0)
        vis, _ = rs.sees(top, rs.rig(d, pix[ok], 1.0 / disp[ok]))
        hits.append(int(vis.sum()))
    print("33 cameras: level-0 pixels that see their slot-31 source, per destination:", hits)
    assert sum(h > 0 for h in hits) >= 2


@pytest.mark.parametrize("variant, env", [
    ("loop", [("DERP_PP_COMPACT", "0")]),
    ("four_waves", [("DERP_COST_WAVES", "4")]),
    ("batched", [("DERP_TABLE_BUDGET_GB", "0.05")]),
])
def test_thirty_three_cameras_variants(built, monkeypatch, variant, env):
    """the one-pixel-per-lane ping-pong loop, the four-wave kernels and destination batches (inverse warps with 32
    sources) bit-equal to the default run, counters included (DERP_NO_MEMO: test_memo_is_exact)"""
    base = _default_run("33", monkeypatch)
    run = _gpu(_case("33"), monkeypatch, env=env)
    _assert_bit_equal(base, run, variant)
    if variant == "batched":
        assert base["batches"] == 1 and run["batches"] >= 2, (base["batches"], run["batches"])


def test_thirty_three_cameras_foreground_masks(built, monkeypatch):
    case = _case("33")
    run = _gpu(case, monkeypatch, use_foreground_masks=1)
    _against_oracle(case, run, "cams33.96.fg", use_foreground_masks=1)


def test_thirty_four_cameras_refused(built):
    """34 cameras are 33 sources per cost: refused with a message naming the limit, also for a one-destination subset
    (sources count, not destinations), and the context stays usable until it closes"""
    from facebook360_dep_amd import derp, synth

    res = 64
    rig = synth.make_rig(34, res)
    sizes = synth.level_sizes(res, res, [64, 50])
    frame = synth.make_frame(rig, sizes)
    cams = rig["cameras"]
    for dst in (None, cams[:1]):
        g = derp.Derp(cams, dst, partial_coverage=1)
        g.set_pyramid(sizes, res, res)
        g.upload_frame({"color": frame["color"]})
        with pytest.raises(derp.DerpError, match=r"too many source cameras \(34 > 33\)"):
            g.process_pyramid()
        g.synchronize()
        g.close()
        assert g.h is None


@pytest.mark.parametrize("name", ["small", "mixed", "33"])
def test_memo_is_exact(built, monkeypatch, name):
    """the default (ping-pong's first candidate from random proposals' cost) against DERP_NO_MEMO=1 (recomputed): every
    level's disparity bit for bit, counters equal. The mixed-type rig's EQUISOLID and ORTHOGRAPHIC cameras take up to
    three square roots per projection."""
    memo = _default_run(name, monkeypatch)
    fresh = _gpu(_case(name), monkeypatch, env=[("DERP_NO_MEMO", "1")])
    assert memo["memo"] > 0 and fresh["memo"] == 0, (memo["memo"], fresh["memo"])
    _assert_bit_equal(memo, fresh, name)
