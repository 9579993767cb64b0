"""A depth context that is used more than once: another geometry, another sequence, other options, another lane count
or table budget between runs. What decides which kernels run then, and with which flags, is host-side state keyed on a
level index: the cached warps and FOV masks of the context, and in every work set, the context's own and one per work
lane, the level whose colour tables are clean, the blank-tile flags, the rank powers and the mismatch mask.

The library is compared with itself only. A *used* context runs a history H and then a job J, a *fresh* one runs only J:
every level of every frame of every destination of J must be the same bytes, NaN positions included. No tolerance. One
job (scenario 2a's) is also held against the oracle, under tests/test_gpu_sequence.py's bound.

The inputs are the 4-camera `tiny` rig at resolution 96, three frames (so that two work lanes exist) and levels of 96 px at
the most. Geometry A is the rig's own pyramid; the other level sizes are those at which tests/test_gpu_reproject_pipeline.py
shows blank and mixed tiles on this rig.

On a library without the warp generation in the work sets (a lane's colorTablesCleanLevel alone decided skipBlank), the
three routes of scenario 1 differ from a fresh context in 4287 (one_level), 32322 (lane_width_rule) and 49890 (phase_api)
disparity values; nothing faults. Routes whose history leaves no 0 flag where the job reads its flags, or leaves one only at
tiles that are blank in the job too, pass there as well, with 0 differing values; _route_shows_something keeps both kinds out."""
import numpy as np
import pytest

from tests import common
from tests.test_gpu_context_families import _same
from tests.test_gpu_level_loop_buffers import BUDGET_GB
from tests.test_gpu_sequence import _bad, _oracle_sequence

pytestmark = pytest.mark.gpu

RES = 96
TILE = 32  # k_reproject_bias's tile: the grid of the blank-tile flags
A = [(96, 96), (64, 64), (48, 48)]
B = [(64, 64), (48, 48), (33, 31)]
LANE_SWITCHES = ("DERP_SEQ_LANES", "DERP_SEQ_LANE_MAX_WIDTH", "DERP_TABLE_BUDGET_GB")  # read per call
TABLES = ("color_padded", "bias_padded", "tile_seen", "fov")

_cache = {}


def _rig():
    from facebook360_dep_amd import synth

    if "rig" not in _cache:
        assert synth.config("tiny") == (4, RES, [w for (w, _) in A])
        _cache["rig"] = synth.make_rig(4, RES)
    return _cache["rig"]


def _frame(sizes, t):
    """Frame t of the sequence (seed 360 + t) at the level sizes `sizes`: the rendered scene on geometry A; elsewhere, as
    test_gpu_reproject_pipeline._frame makes its colours (a ramp plus noise), which takes any level size."""
    from facebook360_dep_amd import synth

    key = ("frame", tuple(sizes), t)
    if key not in _cache:
        if list(sizes) == A:
            _cache[key] = synth.make_frame(_rig(), A, frame=t, seed=360 + t, device="cpu")
        else:
            rng = np.random.default_rng([15, 360 + t])
            color = []
            for w, h in sizes:
                yy, xx = np.mgrid[0:h, 0:w]
                cams = []
                for s in range(4):
                    ramp = ((xx * (700 + 90 * s) + yy * (500 + 70 * s)) % 65536)[..., None]
                    img = np.clip(ramp + rng.integers(-9000, 9001, size=(h, w, 3)), 0, 65535).astype(np.uint16)
                    img[rng.random((h, w)) < 0.05] = 65535
                    img[rng.random((h, w)) < 0.05] = 0
                    cams.append(img)
                color.append(cams)
            _cache[key] = {"color": color}
    return _cache[key]


def _frames(sizes, ts=(0, 1, 2)):
    return [_frame(sizes, t) for t in ts]


def _switches(monkeypatch, **env):
    for k in LANE_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _context(**options):
    from facebook360_dep_amd import derp

    return derp.Derp(_rig()["cameras"], partial_coverage=1, **options)


def _drive(g, r, frames, laned, top_only=False):
    """Upload `frames` to runner r and run it: all levels, or the top level's compute alone. -> {(frame, level):
    [disparity per destination]}. `laned`: the levels whose frames must have run on work lanes, and no other."""
    levels = range(len(g.sizes))
    for t, frame in enumerate(frames):
        r.upload_frame(t, frame)
    g.profile_reset()
    g.profile_enable(True)
    if top_only:
        r.compute(len(g.sizes) - 1)
    else:
        r.run()
    g.synchronize()
    on_lanes = [lv for lv in levels if g.profile_query("lanes_wall", lv)["ms"] > 0]
    assert on_lanes == sorted(laned), (on_lanes, laned)
    if top_only:
        return None
    return {(t, lv): [r.download_disparity(t, lv, d) for d in range(g.D)] for t in range(len(frames)) for lv in levels}


def _sequence(g, sizes, frames, laned, top_only=False):
    """One runner's life on context g under geometry `sizes`; the runner is closed before the geometry can change."""
    from facebook360_dep_amd import sequence

    g.set_pyramid(sizes, RES, RES)
    r = sequence.SequenceRunner(g, 0, len(frames) - 1)
    try:
        return _drive(g, r, frames, laned, top_only)
    finally:
        r.close()


def _fresh(sizes, ts, laned, **options):
    """Frames `ts` under geometry `sizes` on a context that runs nothing else, with the lane switches as they are now:
    run once, shared by the tests that compare with it and left unchanged."""
    import os

    key = ("fresh", tuple(sizes), tuple(ts), tuple(os.environ.get(k) for k in LANE_SWITCHES), tuple(sorted(options.items())))
    if key not in _cache:
        g = _context(**options)
        try:
            _cache[key] = _sequence(g, sizes, _frames(sizes, ts), laned)
        finally:
            g.close()
    return _cache[key]


def _differing(a, b):
    assert a.keys() == b.keys()
    return {k: sum(_bad(x, y) for x, y in zip(a[k], b[k])) for k in a}


def _assert_same(got, want, what):
    bad = {k: v for k, v in _differing(got, want).items() if v}
    print("%s: %d disparity values differ, per (frame, level): %s" % (what, sum(bad.values()), bad))
    assert not bad, (what, bad)
    for k in got:
        for d, (x, y) in enumerate(zip(got[k], want[k])):
            assert _same(x, y), (what, k, d)


def _grid(size):
    return ((size[1] + TILE - 1) // TILE, (size[0] + TILE - 1) // TILE)


def _tile_flags(sizes, level):
    """k_reproject_bias's blank-tile flags at `level` on a fresh context, [table][tile row][tile column] in the tables'
    order. They depend on the rig and the level size only, so the context's own work set stands for the lanes'."""
    key = ("flags", tuple(sizes), level)
    if key not in _cache:
        g = _context()
        try:
            g.set_pyramid(sizes, RES, RES)
            g.upload_frame(_frame(sizes, 0))
            g.level_begin(level)
            g.stage("reproject_colors")
            _cache[key] = np.stack([g.debug(d, s, "tile_seen") for d in range(g.D) for s in range(g.S) if s != d])
        finally:
            g.close()
    return _cache[key]


# ---- 1. stale lanes: J's first laned level has the index of H's last laned level, under other warps
# (h / j: the geometries; *_laned: the levels that run on lanes; level: the index they share)
ROUTES = {
    # one-level pyramids
    "one_level": dict(env={}, h=[(70, 45)], h_laned=[0], j=[(33, 31)], j_laned=[0], level=0),
    # lanes up to 80 px: level 0 of either geometry runs frame after frame, H ends its laned levels at index 1 and J,
    # two levels, starts there
    "lane_width_rule": dict(env={"DERP_SEQ_LANE_MAX_WIDTH": "80"}, h=[(96, 96), (70, 45), (33, 31)], h_laned=[1, 2],
                            j=[(64, 64), (48, 48)], j_laned=[0, 1], level=1),
    # the phase API: H is the top level's compute alone, J a full run of another three-level geometry. (The top level of
    # H is never upsampled from, so its geometry need not shrink level by level.)
    "phase_api": dict(env={}, h=[(96, 96), (64, 64), (70, 45)], h_top_only=True, h_laned=[2], j=B, j_laned=[0, 1, 2],
                      level=2),
}


def _route_shows_something(R):
    """The conditions without which a route passes whatever the lanes do."""
    level = R["level"]
    assert max(R["j_laned"]) == min(R["h_laned"]) == level
    # J has blank and seen tiles at that level, on another tile grid than H's ...
    was, now = _tile_flags(R["h"], level), _tile_flags(R["j"], level)
    assert (now == 0).any() and (now != 0).any()
    assert _grid(R["h"][level]) != _grid(R["j"][level]) and was.shape != now.shape
    # ... and a lane that believed H's flags there would skip a tile that source pixels map into: H left a 0 where J reads
    # the flag of a seen tile (the flags are one array, [table][tile row][tile column]). A 0 at tiles that are blank in J
    # too is not enough: the texels H left there change no disparity.
    assert was.size >= now.size and ((was.reshape(-1)[:now.size] == 0) & (now.reshape(-1) != 0)).any()


def _route_runs(monkeypatch, R):
    """-> (J on the context that ran H, J on a fresh context)"""
    _switches(monkeypatch, **R["env"])
    g = _context()
    try:
        _sequence(g, R["h"], _frames(R["h"]), R["h_laned"], top_only=R.get("h_top_only", False))
        used = _sequence(g, R["j"], _frames(R["j"]), R["j_laned"])
    finally:
        g.close()
    return used, _fresh(R["j"], (0, 1, 2), R["j_laned"])


@pytest.mark.parametrize("route", list(ROUTES))
def test_lanes_do_not_keep_the_tables_of_another_geometry(built, monkeypatch, route):
    """A lane whose last level under the old geometry has the index of its first level under the new one must rewrite its
    colour tables in full: its blank-tile flags were laid out for the old tile grid, and the tiles it would skip hold the
    old geometry's texels."""
    _route_shows_something(ROUTES[route])
    used, fresh = _route_runs(monkeypatch, ROUTES[route])
    _assert_same(used, fresh, "stale lanes, " + route)


# ---- 2. grow, then shrink
def test_grow_reallocates_and_equals_fresh_and_the_oracle(built, monkeypatch):
    """H on a small geometry, J on A: every grow-only buffer is reallocated and loses its contents. J's level 0 needs more
    bytes for one of its colour tables' buffers than the largest buffer H allocated."""
    small = [(48, 48), (33, 31)]
    n = 4

    def largest_buffer(w, h):  # of a level: the warps, a colour table set, the pixel rays, a frame's colour planes
        px = w * h
        return max(n * (n - 1) * (w + 2) * (h + 2) * 8, n * (n - 1) * (w + 4) * (h + 4) * 8, 3 * px * n * 8, px * n * 8)

    w0, h0 = A[0]
    assert n * (n - 1) * (w0 + 4) * (h0 + 4) * 8 > max(largest_buffer(w, h) for (w, h) in small)
    assert all(w0 > w and h0 > h for (w, h) in small)
    _switches(monkeypatch)
    g = _context()
    try:
        _sequence(g, small, _frames(small), [0, 1])
        used = _sequence(g, A, _frames(A), [0, 1, 2])
    finally:
        g.close()
    _assert_same(used, _fresh(A, (0, 1, 2), [0, 1, 2]), "grow")
    ref = _oracle_sequence("tiny", 0, 2)  # test_gpu_sequence._compare_with_oracle's bound
    for (t, level), planes in used.items():
        for d in range(n):
            bad, _ = common.compare_disparity(planes[d], ref.disp[t][level][d].numpy(), 1e-4)
            assert bad == 0, (t, level, d, bad)


def test_grow_shrink_and_grow_again(built, monkeypatch):
    """A, then B, then A again on one context: the second A equals a fresh context's and the bytes of the first A."""
    _switches(monkeypatch)
    g = _context()
    try:
        first = _sequence(g, A, _frames(A), [0, 1, 2])
        _sequence(g, B, _frames(B), [0, 1, 2])
        again = _sequence(g, A, _frames(A), [0, 1, 2])
    finally:
        g.close()
    _assert_same(again, _fresh(A, (0, 1, 2), [0, 1, 2]), "A after A and B")
    _assert_same(again, first, "the second A against the first")


# ---- 3. the lane count changes
@pytest.mark.parametrize("order", ["few_then_many", "many_then_few"])
def test_new_lanes_beside_used_ones(built, monkeypatch, order):
    """DERP_SEQ_LANES=3 and 3 frames (two lanes), then the default lane count and 6 frames (five lanes: three new ones
    beside two used ones) on the same geometry; and the other way round."""
    few = dict(env={"DERP_SEQ_LANES": "3"}, frames=(0, 1, 2))
    many = dict(env={}, frames=(0, 1, 2, 3, 4, 5))
    h, j = (few, many) if order == "few_then_many" else (many, few)
    g = _context()
    try:
        _switches(monkeypatch, **h["env"])
        _sequence(g, A, _frames(A, h["frames"]), [0, 1, 2])
        _switches(monkeypatch, **j["env"])
        used = _sequence(g, A, _frames(A, j["frames"]), [0, 1, 2])
    finally:
        g.close()
    _assert_same(used, _fresh(A, j["frames"], [0, 1, 2]), order)


# ---- 4. the same runner twice
@pytest.mark.parametrize("sizes,options", [(A, {}), ([(70, 45)], {"rebuild_warp_tables": 0})],
                         ids=["pyramid", "one_level_cached_warps"])
def test_the_same_runner_runs_other_frames(built, monkeypatch, sizes, options):
    """run(), three other frames, run() again. With one level and rebuild_warp_tables=0 the second run finds the warps
    of its only level cached and every work set's tables clean for them: the lanes skip their blank tiles with every
    right to, and the result must still be a fresh runner's."""
    from facebook360_dep_amd import sequence

    _switches(monkeypatch)
    laned = list(range(len(sizes)))
    if len(sizes) == 1:
        assert (_tile_flags(sizes, 0) == 0).any(), "no blank tile to skip"
    g = _context(**options)
    try:
        g.set_pyramid(sizes, RES, RES)
        r = sequence.SequenceRunner(g, 0, 2)
        first = _drive(g, r, _frames(sizes), laned)
        used = _drive(g, r, _frames(sizes, (3, 4, 5)), laned)
        r.close()
    finally:
        g.close()
    fresh = _fresh(sizes, (3, 4, 5), laned, **options)
    _assert_same(used, fresh, "second run of one runner")
    assert sum(_differing(first, fresh).values()) > 0, "the second set of frames gives the first set's result"


# ---- 5. no lanes, cached warps
def test_cached_warps_follow_the_geometry_stage_by_stage(built, monkeypatch):
    """rebuild_warp_tables=0: a pyramid under A, set_pyramid(B) with as many levels, a pyramid under B, then the
    stage-level path in level order 2, 0, 1, 0. After every reproject stage the padded colour and bias tables, the
    blank-tile flags and the FOV masks are a fresh context's at that level."""
    _switches(monkeypatch)
    assert len(A) == len(B)

    def tables(g):
        out = {}
        for d in range(g.D):
            for s in range(g.S):
                if s != d:
                    for x in TABLES:
                        out[(d, s, x)] = g.debug(d, s, x)
        return out

    def fresh_tables(level):
        f = _context(rebuild_warp_tables=0)
        try:
            f.set_pyramid(B, RES, RES)
            f.upload_frame(_frame(B, 0))
            f.level_begin(level)
            f.stage("reproject_colors")
            return tables(f)
        finally:
            f.close()

    want = {level: fresh_tables(level) for level in range(len(B))}
    g = _context(rebuild_warp_tables=0)
    try:
        g.set_pyramid(A, RES, RES)
        g.upload_frame(_frame(A, 0))
        g.process_pyramid()
        g.set_pyramid(B, RES, RES)
        g.upload_frame(_frame(B, 0))
        g.process_pyramid()
        for step, level in enumerate((2, 0, 1, 0)):
            g.level_begin(level)
            g.stage("reproject_colors")
            got = tables(g)
            assert got.keys() == want[level].keys()
            for key in got:
                assert _same(got[key], want[level][key]), (step, level, key)
    finally:
        g.close()
    assert any((v == 0).any() for (d, s, x), v in want[2].items() if x == "tile_seen"), "no blank tile at B's top level"


# ---- 6. options between runs
def test_other_random_proposals_between_runs(built, monkeypatch):
    """The lanes key their rank powers on random_proposals: H with the default, J after set_options(another value)."""
    _switches(monkeypatch)
    g = _context()
    other = g.opt.random_proposals + 3
    try:
        _sequence(g, A, _frames(A), [0, 1, 2])
        g.set_options(random_proposals=other)
        used = _sequence(g, A, _frames(A), [0, 1, 2])
    finally:
        g.close()
    fresh = _fresh(A, (0, 1, 2), [0, 1, 2], random_proposals=other)
    _assert_same(used, fresh, "random_proposals=%d" % other)
    assert sum(_differing(fresh, _fresh(A, (0, 1, 2), [0, 1, 2])).values()) > 0, "the option changes nothing"


# ---- 7. the table budget between runs
def test_table_budget_between_runs(built, monkeypatch):
    """H under a table budget that takes level 0's destinations in batches (no lanes, no cached warps), J without it (lanes)."""
    g = _context()
    try:
        _switches(monkeypatch, DERP_TABLE_BUDGET_GB=BUDGET_GB["tiny"])
        _sequence(g, A, _frames(A), [])
        assert g.profile_query("ping_pong", 0)["launches"] > len(_frames(A)), "one batch only: the budget splits nothing"
        _switches(monkeypatch)
        used = _sequence(g, A, _frames(A), [0, 1, 2])
    finally:
        g.close()
    _assert_same(used, _fresh(A, (0, 1, 2), [0, 1, 2]), "after a budgeted run")


# ---- a geometry change under an open sequence is refused
def test_set_pyramid_is_refused_while_a_sequence_is_open(built):
    """The sequence's filter, halo and mask buffers and its frame slots have the sizes of the geometry it was made under.
    No kernel runs here."""
    from facebook360_dep_amd import derp, sequence

    g = _context()
    try:
        g.set_pyramid(B, RES, RES)
        r = sequence.SequenceRunner(g, 0, 2)
        assert g.frame_slots() == (3, 0)
        with pytest.raises(derp.DerpError, match=r"derp_seq \(frames 0\.\.2, rank 0 of 1\) is still open"):
            g.set_pyramid(A, RES, RES)
        assert g.frame_slots() == (3, 0) and g.sizes == B  # the geometry stays as it was
        g.select_frame(2)  # (the third slot is still there)
        other = sequence.SequenceRunner(g, 5, 6)  # two open: closing one is not enough
        r.close()
        with pytest.raises(derp.DerpError, match=r"frames 5\.\.6"):
            g.set_pyramid(A, RES, RES)
        other.close()
        g.set_pyramid(A, RES, RES)
        assert g.frame_slots() == (1, 0) and g.sizes == A
    finally:
        g.close()
