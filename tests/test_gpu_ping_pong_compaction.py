"""Ping-pong's compacted candidate loop (full waves of (pixel, candidate) tasks) against the one-pixel-per-lane loop it
replaced (DERP_PP_COMPACT=0): same comparisons in the same order, so the pyramid must come out bit for bit the same and
every counter must agree — with foreground masks, with several ping-pong iterations (sparse `changed` flags: short, uneven
task lists), with the memoised candidate switched off (candidate 0 always computed) and under the three-wave kernels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(built):
    from facebook360_dep_amd import synth

    n, res, widths = synth.config("small")
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    frame = synth.make_frame(rig, sizes, with_masks=True)
    return dict(rig=rig, sizes=sizes, frame=frame, res=res, n=n)


def _run(small, monkeypatch, compact, env, opts):
    from facebook360_dep_amd import derp

    monkeypatch.setenv("DERP_PP_COMPACT", "1" if compact else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = derp.Derp(small["rig"]["cameras"], partial_coverage=1, **opts)
    g.set_pyramid(small["sizes"], small["res"], small["res"])
    g.upload_frame(small["frame"] if opts.get("use_foreground_masks") else {"color": small["frame"]["color"]})
    g.profile_reset()
    g.profile_enable(True)
    g.process_pyramid()
    g.synchronize()
    out = [[g.download_disparity(level, d) for d in range(small["n"])] for level in range(len(small["sizes"]))]
    pp = [(g.profile_query("ping_pong", lv), g.profile_memoised("ping_pong", lv)) for lv in range(len(small["sizes"]))]
    c = g.counters()
    g.close()
    return out, c, [(q["launches"], q["n_cost"], q["n_pair"], m) for q, m in pp]


def _differ(a, b):
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


@pytest.mark.parametrize("case, env, opts", [
    ("small", {}, {}),
    ("foreground_masks", {}, {"use_foreground_masks": 1}),
    ("three_iterations", {}, {"ping_pong_iterations": 3}),
    ("no_memo", {"DERP_NO_MEMO": "1"}, {}),
    ("three_waves", {"DERP_COST_WAVES": "3"}, {}),
])
def test_compacted_candidate_loop_is_bit_equal(small, monkeypatch, case, env, opts):
    loop, c_loop, pp_loop = _run(small, monkeypatch, False, env, opts)
    comp, c_comp, pp_comp = _run(small, monkeypatch, True, env, opts)
    assert c_comp == c_loop
    assert pp_comp == pp_loop
    assert sum(n_cost for _, n_cost, _, _ in pp_comp) > 0, "ping-pong evaluated nothing"
    for level, (a, b) in enumerate(zip(loop, comp)):
        for d, (x, y) in enumerate(zip(a, b)):
            assert _differ(x, y) == 0, (case, level, d)
