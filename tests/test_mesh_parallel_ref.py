"""The pass-parallel simplifier's restatement (tests/mesh_parallel_ref.py) on the CPU: the properties every result of
the algorithm of DESIGN section 8.3 has, its boundary rule against mesh_ref.Simplifier.identify_boundaries, and its
quality against the reference's sequential algorithm (mesh_ref.simplify) at the same budget."""
import numpy as np
import pytest

from tests import mesh_parallel_ref as P
from tests import mesh_ref as R

BUDGET_CASES = ["plain", "boundary", "not_equi", "disparity"]


def check_mesh(V, F):
    """no face with a repeated index, no two faces with the same vertex set, every vertex used"""
    F = np.asarray(F)
    assert (F[:, 0] != F[:, 1]).all() and (F[:, 1] != F[:, 2]).all() and (F[:, 0] != F[:, 2]).all()
    assert len(np.unique(np.sort(F, axis=1), axis=0)) == len(F)
    assert np.array_equal(np.unique(F), np.arange(len(V)))


def boundary_vertices(V, F):
    s = P.ParallelSimplifier(V, F, R.setup(V, F), True)
    s.adjacency()
    s.identify_boundaries()
    return s, list(s.boundary)


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_properties(name):
    c = P.case(name)
    V, F, (passes, reason) = c["out"]
    print("%s: %d -> %d faces, %d vertices, %d passes, exit %d" % (name, len(c["F"]), len(F), len(V), passes, reason))
    assert passes <= len(c["F"])
    check_mesh(V, F)
    if name in BUDGET_CASES:
        # manifold inputs: a collapse removes at most two faces
        assert reason == P.EXIT_BUDGET and c["budget"] - 1 <= len(F) <= c["budget"] and passes > 1
    elif name == "above":
        assert (passes, reason) == (0, P.EXIT_BUDGET)
        assert V.tobytes() == c["V"].tobytes() and np.array_equal(F, c["F"])
    elif name == "strip":  # every vertex lies on the boundary
        assert (passes, reason) == (0, P.EXIT_NO_CANDIDATES)
        assert V.tobytes() == c["V"].tobytes() and np.array_equal(F, c["F"])
    else:
        assert name == "unreachable" and reason == P.EXIT_NO_CANDIDATES and len(F) > c["budget"] and passes > 1
    if not c["rbe"]:  # boundary vertices never move and never go
        _, boundary = boundary_vertices(c["V"], c["F"])
        kept = {tuple(v) for v in V.tolist()}
        assert any(boundary)
        for v, b in zip(c["V"].tolist(), boundary):
            assert not b or tuple(v) in kept


@pytest.mark.parametrize("name", ["plain", "strip", "disparity"])
def test_boundary_rule_is_identify_boundaries(name):
    c = P.case(name)
    s, want = boundary_vertices(c["V"], c["F"])
    assert s.boundary_rule() == want and any(want)
    if name == "strip":
        assert all(want)
    else:
        assert not all(want)


@pytest.mark.parametrize("name", BUDGET_CASES + ["unreachable"])
def test_quality_against_the_sequential_algorithm(name):
    c = P.case(name)
    V, F, _ = c["out"]
    sv, sf, _ = R.simplify(c["V"], c["F"], c["budget"], 0.2, c["rbe"], c["equi"])
    got, want = P.surface_rms(c["V"], V, F), P.surface_rms(c["V"], sv, sf)
    print("%s: RMS point-to-surface distance %.6g (parallel, %d faces) / %.6g (sequential, %d faces) = %.3f"
          % (name, got, len(F), want, len(sf), got / want))
    assert want > 0 and got <= 1.5 * want


def test_surface_rms():
    """the measure itself: a unit right triangle in z = 0, points over its interior, an edge and a corner"""
    V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    pts = np.array([[0.25, 0.25, 2.0], [0.5, -3.0, 0.0], [-3.0, -4.0, 0.0], [1.0, 1.0, 0.0]])
    d = [P.surface_rms(pts[i:i + 1], V, [[0, 1, 2]]) for i in range(4)]
    assert np.allclose(d, [2.0, 3.0, 5.0, np.sqrt(0.5)], rtol=1e-15, atol=0)
