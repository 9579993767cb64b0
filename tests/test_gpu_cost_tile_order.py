"""The tile order of random proposals and ping-pong (K bands per XCD, DERP_XCD_BANDS; blocks that walk N tiles,
DERP_COST_TILES_PER_BLOCK; tiles left early when nothing in them evaluates) changes where and when a tile runs, never
what it computes: against the run with K = 1, N = 1 the whole pyramid must come out bit for bit the same and every
counter must agree — under the three-wave kernels, with foreground masks (tiles the gate empties), with several
ping-pong iterations (tiles without a task), with the memo off, with the one-pixel-per-lane loop, without the band
rotation, on level sizes that are no multiple of a tile or a square (padded grids), and with destinations in batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = [(k, n) for k in (2, 4) for n in (1, 2, 4)]


@pytest.fixture(scope="module")
def small(built):
    from facebook360_dep_amd import synth

    n, res, widths = synth.config("small")
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    frame = synth.make_frame(rig, sizes, with_masks=True)
    return dict(rig=rig, sizes=sizes, frame=frame, w=res, h=res, n=n)


@pytest.fixture(scope="module")
def odd(built):
    """levels of 72 x 40, 50 x 28 and 36 x 20: no multiple of 16 or 64 either way, and not square"""
    from facebook360_dep_amd import synth

    n, w, h = 4, 72, 40
    rig = synth.make_rig(n, w)
    sizes = synth.level_sizes(w, h, [72, 50, 36])
    assert sizes == [(72, 40), (50, 28), (36, 20)]
    frame = synth.make_frame(rig, sizes, with_masks=True)
    return dict(rig=rig, sizes=sizes, frame=frame, w=w, h=h, n=n)


def _run(data, monkeypatch, bands, per_block, env, opts):
    from facebook360_dep_amd import derp

    monkeypatch.setenv("DERP_XCD_BANDS", str(bands))
    monkeypatch.setenv("DERP_COST_TILES_PER_BLOCK", str(per_block))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = derp.Derp(data["rig"]["cameras"], partial_coverage=1, **opts)
    g.set_pyramid(data["sizes"], data["w"], data["h"])
    g.upload_frame(data["frame"] if opts.get("use_foreground_masks") else {"color": data["frame"]["color"]})
    g.profile_reset()
    g.profile_enable(True)
    g.process_pyramid()
    g.synchronize()
    levels = range(len(data["sizes"]))
    out = [[g.download_disparity(level, d) for d in range(data["n"])] for level in levels]
    stages = []
    for stage in ("ping_pong", "random_proposals"):
        for lv in levels:
            q = g.profile_query(stage, lv)
            stages.append((stage, lv, q["launches"], q["n_cost"], q["n_pair"], g.profile_memoised(stage, lv)))
    c = g.counters()
    g.close()
    return out, c, stages


def _differ(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


_reference = {}


def _check(data, monkeypatch, case, bands, per_block, env, opts):
    if case not in _reference:  # the K = 1, N = 1 run of the case, once for its six orders
        _reference[case] = _run(data, monkeypatch, 1, 1, env, opts)
    ref, c_ref, st_ref = _reference[case]
    got, c_got, st_got = _run(data, monkeypatch, bands, per_block, env, opts)
    assert c_got == c_ref
    assert st_got == st_ref
    for stage in ("ping_pong", "random_proposals"):
        assert sum(s[3] for s in st_got if s[0] == stage) > 0, stage + " evaluated nothing"
    for level, (a, b) in enumerate(zip(ref, got)):
        for d, (x, y) in enumerate(zip(a, b)):
            assert _differ(x, y) == 0, (case, bands, per_block, level, d)
    return st_got


@pytest.mark.parametrize("bands, per_block", ORDERS)
@pytest.mark.parametrize("case, env, opts", [
    ("small", {}, {}),
    ("three_waves", {"DERP_COST_WAVES": "3"}, {}),
    ("foreground_masks", {}, {"use_foreground_masks": 1}),
    ("three_iterations", {}, {"ping_pong_iterations": 3}),
    ("no_memo", {"DERP_NO_MEMO": "1"}, {}),
    ("loop", {"DERP_PP_COMPACT": "0"}, {}),
    ("no_rotation", {"DERP_XCD_ROTATE": "0"}, {}),
])
def test_tile_order_is_bit_equal(small, monkeypatch, case, env, opts, bands, per_block):
    _check(small, monkeypatch, case, bands, per_block, env, opts)


@pytest.mark.parametrize("bands, per_block", ORDERS)
def test_padded_non_square_levels(odd, monkeypatch, bands, per_block):
    _check(odd, monkeypatch, "odd", bands, per_block, {}, {"use_foreground_masks": 1})


@pytest.mark.parametrize("bands, per_block", ORDERS)
def test_destination_batches(small, monkeypatch, bands, per_block):
    """a table budget that takes the six destinations in several batches: dst0 > 0 in the later launches"""
    stages = _check(small, monkeypatch, "batched", bands, per_block, {"DERP_TABLE_BUDGET_GB": "0.012"}, {})
    launches = [s[2] for s in stages if s[0] == "ping_pong" and s[1] == 0]
    assert launches[0] > 1, "one batch only: the budget no longer splits the destinations"
