"""RigAnalyzer without a GPU: the restatement (tests/coverage_ref.py) against what can be said of it by hand, and every
host-only derp_rig_* function of the library against the restatement, bit for bit."""
import math

import numpy as np
import pytest

from tests import coverage_ref as R


@pytest.fixture(scope="module")
def model(built):
    from facebook360_dep_amd import synth

    return synth.make_rig(4, 64)["cameras"][1]


@pytest.fixture(scope="module")
def real(built):
    from tests import common

    return common.real_rig()["cameras"]


def same_rig(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert R.same_camera(g, w), (g, w)


# ---------------------------------------------------------------- the restatement
def test_fibonacci_points_are_unit_and_poles_are_counted(built):
    from facebook360_dep_amd import derp

    u = R.fibonacci_units(1000)
    assert u.shape == (1000, 3) and np.abs(np.sqrt((u * u).sum(axis=1)) - 1).max() < 1e-15
    # y runs over (i + 0.5) / n * 2 - 1; the pole test is on z = cos(roty) * r, not on the axis the points wind round
    kept = R.fibonacci_units(1000, 30.0)
    by_hand = sum(1 for p in u if abs(p[2]) < math.cos(30.0 * math.pi / 180))
    assert len(kept) == by_hand and 0 < by_hand < 1000 and len(derp.rig_fibonacci_units(1000, 30.0)) == by_hand
    assert all(abs(p[2]) < math.cos(math.pi / 6) for p in kept)
    assert len(R.fibonacci_units(1000, 90.0)) == 0 and len(R.fibonacci_units(0)) == 0


def test_distances(built):
    from facebook360_dep_amd import derp

    d = R.coverage_distances(0.5)
    assert list(derp.rig_coverage_distances(0.5)) == list(d)
    assert len(d) == 20 and d[0] == 0.5 and d[10] == 1.0 and d[19] == 0.5 / (1 - 19 / 20.0)


@pytest.mark.parametrize("name", sorted(R.ARRANGEMENTS))
def test_arrangements_are_rigid(model, name):
    from facebook360_dep_amd import derp

    cams = R.rig_arrangement(name, model)
    assert len(cams) == len(R.ARRANGEMENTS[name][3]) == len(derp.rig_arrangement(name, model))
    radius = math.sqrt(sum(v * v for v in model["origin"]))
    for i, cam in enumerate(cams):
        m = np.array([cam["right"], cam["up"], cam["forward"]])
        assert np.abs(m @ m.T - np.eye(3)).max() < 1e-12
        assert np.linalg.det(np.array([cam["right"], cam["up"], [-v for v in cam["forward"]]])) > 0.999
        assert np.abs(np.array(cam["origin"]) - radius * np.array(cam["forward"])).max() < 1e-15
        assert cam["id"] == "cam%d" % i
    assert [c["id"] for c in R.rig_arrangement(name, model, one_based=True)] == ["cam%d" % (i + 1) for i in range(len(cams))]


def test_tetra_and_cube(model):
    from facebook360_dep_amd import derp

    assert R.tetra_default_angle() == math.acos(-1 / 3.0) * 180 / math.pi and abs(R.tetra_default_angle() - 109.4712) < 1e-4
    tetra = R.rig_arrangement("tetra", model)
    f = np.array([c["forward"] for c in tetra])
    dots = f @ f.T
    assert np.abs(dots[~np.eye(4, dtype=bool)] + 1 / 3.0).max() < 1e-12  # a regular tetrahedron
    cube = np.array([c["forward"] for c in R.rig_arrangement("cube", model)])
    assert np.array_equal(cube, np.array([c["forward"] for c in derp.rig_arrangement("cube", model)]))
    assert sorted(tuple(int(v) for v in np.rint(row)) for row in cube) == sorted(
        [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    assert np.abs(cube - np.rint(cube)).max() < 1e-12
    assert np.abs(np.array(R.rig_arrangement("cube", model, custom=45.0)[0]["forward"])[2] - math.cos(math.pi / 4)) < 1e-12


@pytest.mark.parametrize("name", ["typed", "revolved40"])
def test_min_timing_needs_sorted_neighbours_only(built, name):
    """the restatement's two ways to the smallest |t_i - t_j| give the same floats; the maps are not trivial"""
    ref = R.Coverage(R.shared_rigs()[name])
    counts, timing, stats = ref.equirect(1, 1e4)
    counts2, timing2, stats2 = ref.equirect(1, 1e4, pairs="sorted")
    assert np.array_equal(counts, counts2) and np.array_equal(timing.view(np.uint32), timing2.view(np.uint32)) and stats == stats2
    assert counts.shape == (180, 360) and len(np.unique(counts)) > 2 and (timing[counts < 2] == 1).all()
    assert (timing[counts >= 2] < 1).all() and stats[0] == (counts == 0).sum() and 0 < stats[1] <= 1
    assert abs(stats[2] - timing.astype(np.float64).sum()) < 1e-6


def test_report_and_pgm_text():
    hist = np.array([[0, 3, 7, 0, 0], [10, 0, 0, 0, 0]])
    text = R.report(hist, [0.5, 0.526315789], 10)
    assert text == ("distance: 0.50 quality: 1.70 samples: 10 h[0] = 0, h[1] = 3, h[2] = 7, \n"
                    "distance: 0.53 quality: 0.00 samples: 10 h[0] = 10, \n")
    assert R.pgm(np.array([[0, 1, 2], [3, 4, 4]]), 4) == "P2\n3 2\n4\n0 1 2 \n3 4 4 \n"
    assert list(R.timed_values(np.array([1.0, 0.0, 0.5], dtype=np.float32))) == [0, 255, 127]


# ---------------------------------------------------------------- the library against the restatement
def test_library_units_and_distances(built):
    from facebook360_dep_amd import derp

    for count, poles in ((1, 0.0), (63, 0.0), (1000, 0.0), (1000, 30.0), (257, 75.5), (10, 90.0), (0, 0.0)):
        assert np.array_equal(derp.rig_fibonacci_units(count, poles), R.fibonacci_units(count, poles)), (count, poles)
    for lo in (0.5, 0.1, 3.0):
        assert np.array_equal(derp.rig_coverage_distances(lo), R.coverage_distances(lo))


def test_library_matrices(built):
    from facebook360_dep_amd import derp

    for e in ((0.0, 0.0, 0.0), (0.1, -2.0, 3.0), (math.pi, math.pi / 2, -math.pi / 2), (1e-9, 0.0, 7.0)):
        for xyz in (True, False):
            assert np.array_equal(derp.rig_euler_matrix(e, xyz), np.array(R.euler_matrix(e, xyz))), (e, xyz)
    for p in ((0.0, 1.0, 0.0), (0.3, -0.2, 0.93), (0.0, 0.0, 1.0), (0.6, 0.0, -0.8)):
        assert np.array_equal(derp.rig_align_z_matrix(p), np.array(R.align_z_matrix(p))), p
    turned = derp.rig_align_z_matrix((0.6, 0.0, -0.8)) @ np.array((0.6, 0.0, -0.8))
    assert np.abs(turned - (0, 0, 1)).max() < 1e-15


@pytest.mark.parametrize("name", sorted(R.ARRANGEMENTS))
def test_library_arrangements(model, real, name):
    from facebook360_dep_amd import derp

    assert set(derp.RIG_ARRANGEMENTS) == set(R.ARRANGEMENTS)
    for m, custom, one_based in ((model, -1.0, False), (real[2], -1.0, True), (model, 37.5, False)):
        same_rig(derp.rig_arrangement(name, m, custom, one_based), R.rig_arrangement(name, m, custom, one_based))


def test_library_unknown_arrangement(model):
    from facebook360_dep_amd import derp

    with pytest.raises(derp.DerpError, match="unknown arrangement octo"):
        derp.rig_arrangement("octo", model)


def test_library_from_eulers(model):
    from facebook360_dep_amd import derp

    eulers = [(10.0, 20.0, 30.0), (-170.0, 0.5, 90.0), (0.0, 0.0, 0.0), (180.0, -90.0, 45.0)]
    for xyz in (False, True):
        same_rig(derp.rig_from_eulers(model, eulers, xyz), R.rig_from_eulers(model, eulers, xyz))


def test_library_revolve_rotate_scale(real):
    from facebook360_dep_amd import derp

    eulers = [(0.0, 0.0, 0.0), (0.1, 0.2, -0.3), (3.0, -1.0, 2.0)]
    got = derp.rig_revolve(real, eulers)
    same_rig(got, R.rig_revolve(real, eulers))
    assert len(got) == 18 and got[6]["id"] == real[0]["id"] + "_1"
    same_rig(derp.rig_revolve(real, eulers[1:2]), R.rig_revolve(real, eulers[1:2]))
    assert derp.rig_revolve(real, eulers[1:2])[0]["id"] == real[0]["id"]
    for m in ([[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[1, 0, 0], [0, 0, 1], [0, -1, 0]], R.euler_matrix((0.4, 0.5, 0.6)),
              R.align_z_matrix(real[3]["origin"])):
        same_rig(derp.rig_rotate(real, m), R.rig_rotate(real, m))
    for args in ((0.01, 0.0, 1.0), (1.0, 0.3, 1.0), (1.0, 0.0, 0.5), (2.0, 1.5, 0.25), (1.0, 0.0, 1.0)):
        same_rig(derp.rig_scale(real, *args), R.rig_scale(real, *args))
    from tests import common

    nopr = common.real_rig_no_principal()["cameras"]
    same_rig(derp.rig_scale(nopr, 1.0, 0.0, 0.3), R.rig_scale(nopr, 1.0, 0.0, 0.3))


@pytest.mark.parametrize("seed", [1, 12345])
def test_library_perturb(real, model, seed):
    from facebook360_dep_amd import derp, synth

    for cams, amounts in ((real, (0.01, 0.02, 3.0, 0.0)), (synth.make_rig(4, 64)["cameras"], (0.05, 0.3, 1.5, 2.0))):
        got = derp.rig_perturb(cams, seed, *amounts)
        want = R.rig_perturb(cams, seed, *amounts)
        same_rig(got, want)
        start = R.loaded(cams)
        for k in ("origin", "forward", "up", "right"):
            assert got[0][k] == start[0][k]  # camera 0 keeps its pose
        assert got[1]["origin"] != start[1]["origin"] and got[1]["forward"] != start[1]["forward"]
        assert got[0]["principal"] != start[0]["principal"]
    assert not R.same_camera(derp.rig_perturb(real, 1, 0.01, 0.02, 3.0, 0.0)[1], derp.rig_perturb(real, 2, 0.01, 0.02, 3.0, 0.0)[1])
    with pytest.raises(derp.DerpError, match="pixels are not square"):
        derp.rig_perturb([dict(model, focal=[20.0, -21.0])], 1, 0.0, 0.0, 0.0, 1.0)
