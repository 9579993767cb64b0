"""k_coverage against the restatement (tests/coverage_ref.py): counts, histograms, min_timing and the three statistics
equal it exactly — no tolerance anywhere. Rigs: the 4-camera synthetic rig, the reference's own test rig, one camera of
each type, a single camera, a 40-camera revolve (beyond the depth path's cap) and a rig rescaled to 64 x 48. Point sets:
1, 63, 257 and 1000 directions (a lone lane, a wave's tail, a block's tail, several blocks), a point at a camera's own
position, sample spheres that the cameras lie outside of, the smallest equirect, even and odd cross sections."""
import numpy as np
import pytest

from facebook360_dep_amd import derp
from tests import coverage_ref as R

pytestmark = pytest.mark.gpu

_state = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_last_context():
    yield
    for g, _ in _state.values():
        g.close()
    _state.clear()


def rig(name):
    """(context, restatement) of one rig at a time"""
    if name not in _state:
        for g, _ in _state.values():
            g.close()
        _state.clear()
        cams = R.shared_rigs()[name] if name != "typed_x20" else R.rig_scale(R.typed_rig(), 20.0)
        _state[name] = (derp.Derp(cams), R.Coverage(cams))
    return _state[name]


RIGS = ["rig4", "real", "typed", "one", "revolved40"]


@pytest.mark.parametrize("name", RIGS)
def test_directions(name):
    g, ref = rig(name)
    # 0.05 .. 1: the synthetic cameras sit 0.25 from the origin, outside the first sample spheres; then out to 10
    distances = np.concatenate([R.coverage_distances(0.05), R.coverage_distances(0.5)[15:]])
    for n in (1, 63, 257, 1000):
        units = R.fibonacci_units(max(n, 2))[:n]  # (one sample alone is the pole (0, 0, 1), which discardPoles drops)
        assert len(units) == n
        want_hist, want_counts = ref.directions(units, distances)
        hist, counts = g.coverage_directions(units, distances)
        print(name, n, "differing counts", int((counts != want_counts).sum()), "max coverage", int(want_counts.max()))
        assert counts.dtype == np.uint8 and counts.shape == (len(distances), n) and np.array_equal(counts, want_counts)
        assert hist.dtype == np.int32 and np.array_equal(hist, want_hist)
        own = np.stack([np.bincount(c, minlength=g.D + 1) for c in counts])
        assert np.array_equal(hist, own) and (hist.sum(axis=1) == n).all()
        assert np.array_equal(g.coverage_directions(units, distances, want_counts=False)[0], hist)
    assert want_counts.max() >= 1 and (name == "one" or len(np.unique(want_counts)) > 1)


@pytest.mark.parametrize("name", ["rig4", "typed", "real"])
def test_a_point_at_a_camera(name):
    """distance 1 times the camera's own position, and its neighbours one ulp away"""
    g, ref = rig(name)
    pts = []
    for cam in ref.cams:
        o = np.array(cam["origin"])
        pts += [o, np.nextafter(o, np.inf), np.nextafter(o, -np.inf), -o]
    want_hist, want_counts = ref.directions(pts, [1.0])
    hist, counts = g.coverage_directions(pts, [1.0])
    assert np.array_equal(counts, want_counts) and np.array_equal(hist, want_hist)


@pytest.mark.parametrize("name,ppd,distance", [("rig4", 1, 1e4), ("rig4", 2, 0.3), ("real", 1, 1e4), ("typed", 1, 1e4),
                                               ("typed", 1, 0.26), ("one", 1, 1e4), ("revolved40", 1, 1e4)])
def test_equirect(name, ppd, distance):
    g, ref = rig(name)
    want_counts, want_timing, want_stats = ref.equirect(ppd, distance)
    counts, timing, stats = g.coverage_equirect(ppd, distance)
    print(name, ppd, distance, "differing counts", int((counts != want_counts).sum()), "timings",
          int((timing.view(np.uint32) != want_timing.view(np.uint32)).sum()), "stats", stats, want_stats)
    assert counts.shape == (180 * ppd, 360 * ppd) and np.array_equal(counts, want_counts)
    assert timing.dtype == np.float32 and np.array_equal(timing.view(np.uint32), want_timing.view(np.uint32))
    assert stats == want_stats
    assert (timing[want_counts < 2] == 1.0).all() and (name == "one" or (timing < 1.0).any())
    only_counts, none, no_stats = g.coverage_equirect(ppd, distance, timing=False)
    assert none is None and no_stats is None and np.array_equal(only_counts, want_counts)


@pytest.mark.parametrize("name,cams,distance", [("small", (0, 1, 3), 1e4), ("small", (1,), 0.5), ("rig4", (0, 3), 1e4),
                                                ("revolved40", (39,), 2.0)])
def test_camera(name, cams, distance):
    g, ref = rig(name)
    for cam in cams:
        want, outside = ref.camera(cam, distance)
        got = g.coverage_camera(cam, distance)
        print(name, cam, "differing", int((got != want).sum()), "outside the circle", int(outside.sum()), "of", outside.size)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert (got[outside] == 0).all() and (got[~outside] >= 1).any()
    if name == "small":
        assert want.shape == (48, 64) and 0 < outside.sum() < outside.size  # (camera 3: the circle ends inside the image)


@pytest.mark.parametrize("name", ["rig4", "typed_x20", "real"])
def test_cross_section(name):
    g, ref = rig(name)
    for dim in (16, 17, 1):
        want = ref.cross_section(dim)
        got = g.coverage_cross_section(dim)
        print(name, dim, "differing", int((got != want).sum()), "values", np.unique(want))
        assert got.shape == (dim, dim) and np.array_equal(got, want)
    assert name != "typed_x20" or len(np.unique(ref.cross_section(17))) > 1


def test_two_calls_on_one_context_agree():
    g, _ = rig("typed")
    units, distances = R.fibonacci_units(257), R.coverage_distances(0.1)
    a, b = g.coverage_directions(units, distances), g.coverage_directions(units, distances)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    e = g.coverage_equirect(1, 1e4)
    g.coverage_cross_section(16)
    g.coverage_camera(2)
    f = g.coverage_equirect(1, 1e4)
    assert np.array_equal(e[0], f[0]) and np.array_equal(e[1].view(np.uint32), f[1].view(np.uint32)) and e[2] == f[2]


def test_refusals_by_name():
    g, _ = rig("rig4")
    units, distances = R.fibonacci_units(10), R.coverage_distances()
    for call, message in (
            (lambda: g.coverage_directions(np.zeros((0, 3)), distances), "zero points"),
            (lambda: g.coverage_directions(units, []), "zero points"),
            (lambda: g.coverage_equirect(0), "pixels_per_degree must be >= 1"),
            (lambda: g.coverage_equirect(-3), "pixels_per_degree must be >= 1"),
            (lambda: g.coverage_cross_section(0), "dim must be >= 1"),
            (lambda: g.coverage_camera(4), "camera index 4 out of range"),
            (lambda: g.coverage_camera(-1), "camera index -1 out of range")):
        with pytest.raises(derp.DerpError, match=message):
            call()
    assert g.coverage_directions(units, distances)[0].sum() == 10 * 20  # (the context still works)


def test_more_than_255_cameras_are_refused():
    from facebook360_dep_amd import synth

    for g, _ in _state.values():
        g.close()
    _state.clear()
    cams = R.rig_revolve(synth.make_rig(4, 64)["cameras"], [(0.0, 0.0, 0.01 * k) for k in range(64)])
    assert len(cams) == 256
    g = derp.Derp(cams)
    try:
        for call in (lambda: g.coverage_directions(R.fibonacci_units(10), [1.0]), lambda: g.coverage_equirect(1),
                     lambda: g.coverage_camera(0), lambda: g.coverage_cross_section(16)):
            with pytest.raises(derp.DerpError, match=r"too many cameras \(256 > 255\)"):
                call()
    finally:
        g.close()
    g = derp.Derp(cams[:255])  # the most the counts hold
    try:
        ref = R.Coverage(cams[:255])
        units = R.fibonacci_units(63)
        want_hist, want_counts = ref.directions(units, [2.0])
        hist, counts = g.coverage_directions(units, [2.0])
        assert np.array_equal(counts, want_counts) and np.array_equal(hist, want_hist) and hist.shape == (1, 256)
        # ... and the longest list of timings a lane can hold: 255 floats of LDS each
        want = ref.equirect(1, 1e4, pairs="sorted")
        got = g.coverage_equirect(1, 1e4)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert got[2] == want[2] and want[0].max() > 100
    finally:
        g.close()
