"""Brute force in runs: a block of k_brute_costs evaluates a run of consecutive disparity indices for its strip, with the
strip's cull mask. Whatever the run length (DERP_BRUTE_RUN: 1, 8 — 150 is no multiple of it, so the last run is partial —
and 150) the selected disparity, cost, confidence and the counters are the same bits, and they are the oracle's (to
tests/test_gpu_parity.py's measure for this stage: fp64 libm on the host, OCML on the device). One case puts candidates
nearer than 0.05 m, where the cull mask switches itself off; one runs an eight-camera rig whose cameras look away from one
another, so that the mask holds sources at all."""
import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

RUNS = (1, 8, 150)


def _tiny():
    from facebook360_dep_amd import synth

    n, res, widths = synth.config("tiny")
    rig = synth.make_rig(n, res)
    sizes = synth.level_sizes(res, res, widths)
    return dict(rig=rig, sizes=sizes, frame=synth.make_frame(rig, sizes, with_masks=True), w=res, h=res, n=n)


def _odd():
    """one level of 45 x 37: an interior of 43 x 35, partial strips both ways"""
    from facebook360_dep_amd import synth

    n, w, h = 4, 45, 37
    rig = synth.make_rig(n, w)
    sizes = [(w, h)]
    return dict(rig=rig, sizes=sizes, frame=synth.make_frame(rig, sizes, with_masks=True), w=w, h=h, n=n)


def _ring():
    """eight cameras whose neighbours across the rig look the other way: strips have sources behind them, so the cull mask
    is not empty (on the four-camera rigs it may be)"""
    from facebook360_dep_amd import synth

    n, w, h = 8, 40, 40
    rig = synth.make_rig(n, w)
    fwd = np.array([c["forward"] for c in rig["cameras"]], dtype=np.float64)
    fwd /= np.linalg.norm(fwd, axis=1, keepdims=True)
    assert (fwd @ fwd.T).min() < -0.5, "no camera of the rig looks away from another"
    sizes = [(w, h)]
    return dict(rig=rig, sizes=sizes, frame=synth.make_frame(rig, sizes, with_masks=True), w=w, h=h, n=n)


CASES = {
    "tiny": (_tiny, {}),
    "tiny_masks": (_tiny, {"use_foreground_masks": 1}),
    "tiny_near": (_tiny, {"min_depth_m": 0.02}),  # probe disparities up to 50: depths down to 0.02 m
    "odd": (_odd, {}),
    "ring": (_ring, {}),
}
_data, _ref = {}, {}


def _differ(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return int((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).sum())


def _brute(data, opts, monkeypatch, run):
    from facebook360_dep_amd import derp

    monkeypatch.setenv("DERP_BRUTE_RUN", str(run))
    g = derp.Derp(data["rig"]["cameras"], partial_coverage=1, **opts)
    g.set_pyramid(data["sizes"], data["w"], data["h"])
    g.upload_frame(data["frame"] if opts.get("use_foreground_masks") else {"color": data["frame"]["color"]})
    level = len(data["sizes"]) - 1
    g.profile_reset()
    g.profile_enable(True)
    g.level_begin(level)
    g.stage("reproject_colors")
    g.stage("brute_force")
    g.synchronize()
    out = []
    for d in range(data["n"]):
        cost, conf = g.download_cost(level, d)
        out.append((g.get_level_disparity(d), cost, conf))
    q = g.profile_query("brute_force", level)
    g.close()
    return out, (q["n_cost"], q["n_pair"])


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("case", list(CASES))
def test_run_length_changes_nothing_and_the_oracle_agrees(built, monkeypatch, case, run):
    make, opts = CASES[case]
    if make not in _data:
        _data[make] = make()
    data = _data[make]
    level = len(data["sizes"]) - 1
    if case not in _ref:  # the oracle's level and the run-length-1 launch, once per case
        L = common.oracle_level(data["rig"], data["sizes"], data["frame"], level, data["w"], data["h"],
                                partial_coverage=True, **opts)
        L.reproject_colors()
        L.brute_force()
        _ref[case] = ([L.get_dst(d) for d in range(data["n"])], L.counters(), _brute(data, opts, monkeypatch, 1))
    oracle, oc, (one, c_one) = _ref[case]
    got, c = _brute(data, opts, monkeypatch, run)
    assert c == c_one, (c, c_one)
    assert c[0] == oc["n_cost"] and abs(c[1] - oc["n_pair"]) <= 4, (c, oc)
    assert c[0] > 0
    for d in range(data["n"]):
        for what, a, b in zip(("disparity", "cost", "confidence"), got[d], one[d]):
            assert _differ(a, b) == 0, (case, run, d, what)
        rd, rc, rf = oracle[d]
        assert common.compare_disparity(got[d][0], rd, 1e-4)[0] == 0, (case, run, d)
        assert common.compare_disparity(got[d][1], rc, 1e-5)[0] == 0, (case, run, d)
        assert _differ(got[d][2], rf) == 0, (case, run, d)
