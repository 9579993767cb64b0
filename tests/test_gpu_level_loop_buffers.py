"""The level loop moves no result by copying: ping-pong's iterations alternate between disparity / cost and dispRes /
costRes and write `changed` themselves, the bilateral filter and the median exchange the working disparity with their
scratch, and the loop's last stage writes the frame's level. What each stage and the whole pyramid compute must be what
the oracle computes: with 1, 2 and 3 ping-pong iterations (both parities, `changed` in real use), with destinations in
batches, with the mismatch stage, without the median (the k_mask_fov tail) and without the bilateral filter, stage by
stage through the stage-level API, and for a sequence whose frames run on work lanes."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

TOL = 1e-4  # tests/test_gpu_parity.py: whole pyramids against the oracle (fp64 libm vs OCML in the last ulp)

CASES = {
    "one_iteration": {},
    "two_iterations": {"ping_pong_iterations": 2},
    "three_iterations": {"ping_pong_iterations": 3},
    "mismatches": {"mismatches_start_level": 1},
    "no_median": {"do_median_filter": 0},
    "no_bilateral": {"do_bilateral_filter": 0},
    "neither_filter": {"do_median_filter": 0, "do_bilateral_filter": 0, "ping_pong_iterations": 2},
}
# table budgets that take level 0's destinations in several batches (tiny: 0.71 MB of tables per destination, 0.93 MB with
# the inverse warps batches need, so 2.68 MB holds two of four; small: tests/test_gpu_cost_tile_order.py's)
BUDGET_GB = {"tiny": "0.0025", "small": "0.012"}


@pytest.fixture(scope="module", params=["tiny", "small"])
def data(request, built):
    from facebook360_dep_amd import synth

    n, res, widths = synth.config(request.param)
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    frame = synth.make_frame(rig, sizes)
    return dict(name=request.param, rig=rig, sizes=sizes, frame=frame, res=res, n=n)


def _differ(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def _gpu(data, **opts):
    from facebook360_dep_amd import derp

    g = derp.Derp(data["rig"]["cameras"], partial_coverage=1, **opts)
    g.set_pyramid(data["sizes"], data["res"], data["res"])
    g.upload_frame({"color": data["frame"]["color"]})
    return g


def _pyramid(data, **opts):
    """-> ([level][dst] disparity, counters, ping-pong launches per level) of one run of the whole pyramid"""
    g = _gpu(data, **opts)
    g.profile_reset()
    g.profile_enable(True)
    g.process_pyramid()
    g.synchronize()
    levels = range(len(data["sizes"]))
    out = [[g.download_disparity(level, d) for d in range(data["n"])] for level in levels]
    c = g.counters()
    launches = [g.profile_query("ping_pong", lv)["launches"] for lv in levels]
    g.close()
    return out, c, launches


_oracle = {}


def _oracle_pyramid(data, case):
    key = (data["name"], case)
    if key not in _oracle:  # once per rig and option set, shared by the tests that need it
        cnt = {}
        ref = common.oracle_pyramid(data["rig"], data["sizes"], data["frame"], data["res"], data["res"], counters=cnt,
                                    partial_coverage=True, **CASES[case])
        _oracle[key] = (ref, cnt)
    return _oracle[key]


def _assert_pyramid(data, case, got, c):
    ref, cnt = _oracle_pyramid(data, case)
    for level in range(len(data["sizes"])):
        for d in range(data["n"]):
            bad, rel = common.compare_disparity(got[level][d], ref[level][d], TOL)
            assert bad == 0, (data["name"], case, level, d, bad, rel)
    assert c["n_cost"] == sum(v["n_cost"] for v in cnt.values()), (c, cnt)
    assert abs(c["n_pair"] - sum(v["n_pair"] for v in cnt.values())) <= 1e-6 * c["n_pair"] + 4, (c, cnt)


@pytest.mark.parametrize("case", list(CASES))
def test_whole_pyramid_equals_the_oracle(data, case):
    got, c, _ = _pyramid(data, **CASES[case])
    _assert_pyramid(data, case, got, c)


@pytest.mark.parametrize("case", ["one_iteration", "two_iterations", "three_iterations"])
def test_destination_batches(data, monkeypatch, case):
    """DB < D: every batch runs its iterations on its own planes, the buffers exchange roles once after the last batch"""
    whole, c_whole, _ = _pyramid(data, **CASES[case])
    monkeypatch.setenv("DERP_TABLE_BUDGET_GB", BUDGET_GB[data["name"]])
    got, c, launches = _pyramid(data, **CASES[case])
    assert launches[0] > 1, "one batch only: the budget no longer splits the destinations"  # (one span per batch)
    assert c == c_whole
    for level in range(len(data["sizes"])):
        for d in range(data["n"]):
            assert _differ(got[level][d], whole[level][d]) == 0, (case, level, d)
    _assert_pyramid(data, case, got, c)


@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_stage_by_stage(data, iterations):
    """after every stage(...) the working disparity and cost are that stage's result, as in the oracle's level; a second
    stage("ping_pong") evaluates its own candidate again instead of taking it from the memo"""
    level = 0
    w, h = data["sizes"][level]
    rng = np.random.default_rng(11)
    start = [(data["frame"]["truth"][d] * rng.uniform(0.8, 1.25, size=(h, w))).astype(np.float32) for d in range(data["n"])]
    opts = {"ping_pong_iterations": iterations}
    L = common.oracle_level(data["rig"], data["sizes"], data["frame"], level, data["res"], data["res"],
                            partial_coverage=True, **opts)
    L.reproject_colors()
    g = _gpu(data, **opts)
    g.profile_reset()
    g.profile_enable(True)
    g.level_begin(level)
    g.stage("reproject_colors")
    for d in range(data["n"]):
        L.set_dst(d, disparity=start[d])
        g.set_level_disparity(d, start[d])

    def same(stage, cost=True):
        for d in range(data["n"]):
            rd, rc, _ = L.get_dst(d)
            assert _differ(g.get_level_disparity(d), rd) == 0, (stage, d)
            if cost:
                assert common.compare_disparity(g.download_cost(level, d)[0], rc, 1e-5)[0] == 0, (stage, d)

    L.random_proposals()
    g.stage("random_proposals")
    same("random_proposals")
    L.ping_pong()
    g.stage("ping_pong")
    same("ping_pong")
    assert g.profile_memoised("ping_pong", level) > 0, "the memo served nothing: the next check would be vacuous"
    memo = g.profile_memoised("ping_pong", level)
    L.ping_pong()
    g.stage("ping_pong")
    same("ping_pong again")
    assert g.profile_memoised("ping_pong", level) == memo, "the second ping-pong took candidates from the memo"
    L.bilateral()
    g.stage("bilateral")
    same("bilateral", cost=False)
    L.median()
    g.stage("median")
    same("median", cost=False)
    L.mask_fov()
    g.stage("mask_fov")
    same("mask_fov", cost=False)
    g.stage("end")
    g.synchronize()
    for d in range(data["n"]):
        assert _differ(g.download_disparity(level, d), L.get_dst(d)[0]) == 0, d
    oc = L.counters()
    c = g.counters()
    assert c["n_cost"] == oc["n_cost"], (c, oc)
    g.close()


def _sequence_crcs(data, frames, monkeypatch, lanes):
    from facebook360_dep_amd import sequence

    if lanes is not None:
        monkeypatch.setenv("DERP_SEQ_LANES", lanes)
    else:
        monkeypatch.delenv("DERP_SEQ_LANES", raising=False)
    g = _gpu(data)
    runner = sequence.SequenceRunner(g, 0, len(frames) - 1, 0, 1, do_temporal_filter=1)
    for t, frame in enumerate(frames):
        runner.upload_frame(t, frame)
    g.profile_reset()
    g.profile_enable(True)
    runner.run()
    g.synchronize()
    crcs = [runner.result_crc(level) for level in range(len(data["sizes"]))]
    laned = [lv for lv in range(len(data["sizes"])) if g.profile_query("lanes_wall", lv)["ms"] > 0]
    c = g.counters()
    runner.close()
    g.close()
    return crcs, laned, c


def test_sequence_on_work_lanes_equals_one_after_the_other(data, monkeypatch):
    """three frames with the temporal filter: every level of these rigs runs on work lanes, each lane with a working set
    of its own whose buffers exchange roles independently; frame by frame on one working set must give the same CRCs"""
    from facebook360_dep_amd import synth

    frames = [synth.make_frame(data["rig"], data["sizes"], frame=t, seed=360 + t) for t in range(3)]
    on_lanes, laned, c_lanes = _sequence_crcs(data, frames, monkeypatch, None)
    assert laned == list(range(len(data["sizes"]))), laned
    in_turn, laned0, c_turn = _sequence_crcs(data, frames, monkeypatch, "0")
    assert laned0 == []
    assert on_lanes == in_turn
    assert c_lanes == c_turn


def test_mismatch_mask_of_a_level_without_the_stage_is_empty(data):
    """the mask is cleared only where the mismatch stage runs; a level without it must still read as "nothing flagged",
    also right after a level that flagged pixels (perturbed disparities, as tests/test_gpu_parity.py provokes them)"""
    g = _gpu(data, mismatches_start_level=0)
    w, h = data["sizes"][0]
    rng = np.random.default_rng(4)
    g.level_begin(0)
    for d in range(data["n"]):
        g.set_level_disparity(d, (data["frame"]["truth"][d] * rng.uniform(0.7, 1.4, size=(h, w))).astype(np.float32))
    g.stage("mismatches")
    flagged = sum(int(g.mismatch_mask(d).sum()) for d in range(data["n"]))
    assert flagged > 0, "level 0 flagged nothing: the test would be vacuous"
    g.level_begin(1)
    g.stage("mismatches")  # level 1 is above mismatches_start_level: the stage does nothing
    for d in range(data["n"]):
        assert int(g.mismatch_mask(d).sum()) == 0, d
    g.close()


def test_shared_fov_mask_follows_the_level(data):
    """the FOV masks live on the context under the projection warps' rule: with cached warp tables a level met again is
    not rebuilt, another level is"""
    g = _gpu(data, rebuild_warp_tables=0)
    for level in (1, 0, 0, 1):
        L = common.oracle_level(data["rig"], data["sizes"], data["frame"], level, data["res"], data["res"],
                                partial_coverage=True)
        g.level_begin(level)
        for d in range(data["n"]):
            assert np.array_equal(g.debug(d, 0, "fov"), L.fov_mask(d)), (level, d)
    g.close()
