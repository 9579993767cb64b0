"""The level's plan (derp_debug_level_plan): what the frames of a pass over a level share (the destination batch that
fits the table budget, whether inverse warps are stored) is decided once per pass, by the frame that opens the level;
the other frames, in turn or on the work lanes, join it. Inputs: tests/test_gpu_context_reuse.py's (the 4-camera `tiny`
rig at resolution 96, levels 96 / 64 / 48, three frames). The library is compared with itself: same bytes, NaN
positions included."""
import pytest

from tests.test_gpu_context_reuse import A, RES, _assert_same, _context, _drive, _frames, _switches
from tests.test_gpu_level_loop_buffers import BUDGET_GB

pytestmark = pytest.mark.gpu

LEVELS = len(A)
_runs = {}


def _run(monkeypatch, name, env, laned):
    """run() of the three frames on a fresh context under the switches `env`, once per name -> dict(disp, opened (levels
    opened during run()), plan (after it), warps (proj_warp launches per level), rebuilds (see below))"""
    if name not in _runs:
        from facebook360_dep_amd import sequence

        _switches(monkeypatch, **env)
        g = _context()
        try:
            assert g.opt.rebuild_warp_tables == 1  # the default: the frame that opens a level rebuilds its warps
            g.set_pyramid(A, RES, RES)
            r = sequence.SequenceRunner(g, 0, 2)
            before = g.debug_level_plan()
            assert (before["level"], before["decisions"]) == (-1, 0)
            disp = _drive(g, r, _frames(A), laned)
            plan = g.debug_level_plan()
            warps = [g.profile_query("proj_warp", lv)["launches"] for lv in range(LEVELS)]
            # the option as the library holds it after the run: a direct call opens level 0 again and, although that
            # level's warps are the cached ones, rebuilds them if and only if rebuild_warp_tables still reads 1
            rebuilds = None
            if plan["batch"] == g.D:
                g.process_level(0)
                g.synchronize()
                rebuilds = g.profile_query("proj_warp", 0)["launches"] - warps[0]
                assert g.debug_level_plan()["decisions"] == plan["decisions"] + 1
            r.close()
            _runs[name] = dict(disp=disp, opened=plan["decisions"] - before["decisions"], plan=plan, warps=warps,
                               rebuilds=rebuilds, D=g.D, option=g.opt.rebuild_warp_tables)
        finally:
            g.close()
    return _runs[name]


def _lanes(monkeypatch):
    return _run(monkeypatch, "lanes", {}, [0, 1, 2])


def _in_turn(monkeypatch):
    return _run(monkeypatch, "in_turn", {"DERP_SEQ_LANES": "0"}, [])


def test_lanes_open_each_level_once(built, monkeypatch):
    """(a) default lanes, all three levels laned: one decision per level, made by the first frame; the lanes' frames join"""
    got = _lanes(monkeypatch)
    assert got["opened"] == LEVELS
    assert (got["plan"]["level"], got["plan"]["batch"]) == (0, got["D"])


def test_in_turn_opens_each_level_once_and_equals_lanes(built, monkeypatch):
    """(b) DERP_SEQ_LANES=0: frame after frame on the context's own work set, still one decision per level"""
    got = _in_turn(monkeypatch)
    assert got["opened"] == LEVELS
    assert (got["plan"]["level"], got["plan"]["batch"]) == (0, got["D"])
    _assert_same(got["disp"], _lanes(monkeypatch)["disp"], "in turn against lanes")


def test_table_budget_batches_and_equals_in_turn(built, monkeypatch):
    """(c) a table budget that takes level 0's destinations in batches: no lanes, inverse warps stored, same bytes"""
    got = _run(monkeypatch, "budget", {"DERP_TABLE_BUDGET_GB": BUDGET_GB["tiny"]}, [])
    assert got["plan"]["level"] == 0 and 1 <= got["plan"]["batch"] < got["D"]
    assert got["plan"]["store_inverse"] == 1
    _assert_same(got["disp"], _in_turn(monkeypatch)["disp"], "batched against whole")


def test_only_the_opening_frame_rebuilds_the_warps(built, monkeypatch):
    """(d) rebuild_warp_tables=1, three frames in turn: proj_warp launches once per level, by the frame that opens it,
    and not once per frame. The commit before the level plan (the options were rewritten around every frame then)
    measures [1, 1, 1] launches for levels 0, 1, 2 on the MI355X; the same is asserted here. The option still reads 1
    afterwards: in the binding, and in the library, where a direct call of level 0 rebuilds its cached warps."""
    got = _in_turn(monkeypatch)
    print("proj_warp launches per level:", got["warps"], "rebuilds by a direct call afterwards:", got["rebuilds"])
    assert got["warps"] == [1, 1, 1]
    assert got["option"] == 1 and got["rebuilds"] == 1
    assert _lanes(monkeypatch)["warps"] == [1, 1, 1]


def test_another_level_in_between_reopens_the_plan(built, monkeypatch):
    """(e) compute_frame of the top level, frame by frame, with a derp_process_level of the level below between the first
    two: the second frame finds the plan made for another level and opens its own level again; the third joins."""
    from facebook360_dep_amd import sequence

    _switches(monkeypatch, DERP_SEQ_LANES="0")
    top = LEVELS - 1
    frames = _frames(A)

    def top_level(disturb):
        g = _context()
        try:
            g.set_pyramid(A, RES, RES)
            r = sequence.SequenceRunner(g, 0, 2)
            for t, frame in enumerate(frames):
                r.upload_frame(t, frame)
            opened = []
            for t in range(len(frames)):
                if disturb and t == 1:
                    g.process_level(top - 1)  # (frame 0's, from its top level)
                before = g.debug_level_plan()["decisions"]
                r.compute_frame(top, t)
                plan = g.debug_level_plan()
                opened.append(plan["decisions"] - before)
                assert (plan["level"], plan["batch"]) == (top, g.D)
            g.synchronize()
            out = {(t, top): [r.download_disparity(t, top, d) for d in range(g.D)] for t in range(len(frames))}
            r.close()
            return out, opened
        finally:
            g.close()

    fresh, opened = top_level(False)
    assert opened == [1, 0, 0]
    got, opened = top_level(True)
    assert opened == [1, 1, 0]
    _assert_same(got, fresh, "a level in between")
