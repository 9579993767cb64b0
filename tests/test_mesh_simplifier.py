"""The host mesh simplifier (csrc/derp_simplify.cpp: MeshSimplifier::simplify restated without Eigen) against the
restatement in tests/mesh_ref.py, bit for bit, without a GPU: through the library's host-only entries, and once more
through a stand-alone program built with AddressSanitizer + UBSan (tests/native/mesh_simplify_main.cpp; nothing
sanitized is loaded into Python)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cam():
    from facebook360_dep_amd import synth

    return synth.make_rig(2, 64)["cameras"][0]


@pytest.fixture(scope="module")
def mesh_a(cam):
    """(a): 48 x 32 with ripples, a step edge and a NaN hole: about 3 000 faces"""
    m = R.build(cam, R.synthetic_depth(48, 32))
    assert 2500 < len(m["F"]) < 3100 and m["unmasked"] > len(m["F"])  # the hole removed faces, the step tore quads
    assert m["outcomes"].get(0, 0) > 0
    return m["V"], m["F"]


@pytest.fixture(scope="module")
def mesh_b(cam):
    """(b): a 40 x 2 strip of uneven depth: every vertex lies on the boundary"""
    rng = np.random.default_rng(5)
    depth = 2.0 + 0.05 * rng.random((2, 40))  # ratios stay above the tear ratio: the strip is whole
    m = R.build(cam, (1.0 / depth).astype(np.float32))
    assert len(m["F"]) == 78 and len(m["V"]) == 80
    return m["V"], m["F"]


@pytest.fixture(scope="module")
def mesh_flat(cam):
    """tests/mesh_cases.py's flat 12 x 12 map: 4 distinct edge costs, negative, zero and positive"""
    from tests import mesh_cases as M

    m = M.build_case("flat_12")["want"]
    assert len(m["F"]) == 242
    return m["V"], m["F"]


@pytest.fixture(scope="module")
def mesh_triangle(cam):
    """tests/mesh_cases.py's 2 x 2 map torn to one triangle"""
    from tests import mesh_cases as M

    m = M.build_case("single_triangle")["want"]
    assert len(m["F"]) == 1 and len(m["V"]) == 3
    return m["V"], m["F"]


@pytest.fixture(scope="module")
def mesh_quad(cam):
    """tests/mesh_cases.py's whole 2 x 2 map: two faces with a common edge"""
    from tests import mesh_cases as M

    m = M.build_case("size_2x2")["want"]
    assert len(m["F"]) == 2 and len(m["V"]) == 4
    return m["V"], m["F"]


# name -> (mesh fixture, budget, strictness, remove_boundary_edges, equi_error)
CASES = {
    "a": ("mesh_a", 600, 0.2, False, True),
    "b": ("mesh_b", 10, 0.2, False, True),
    "c": ("mesh_a", 100000, 0.2, False, True),
    "d_boundary": ("mesh_a", 600, 0.2, True, True),
    "d_not_equi": ("mesh_a", 600, 0.2, False, False),
    "d_both": ("mesh_a", 600, 0.2, True, False),
    # both ends of getThreshold's index: the smallest cost and the largest
    "s0_a": ("mesh_a", 600, 0.0, False, True),
    "s1_a": ("mesh_a", 600, 1.0, False, True),
    "s0_flat": ("mesh_flat", 40, 0.0, False, True),
    "s1_flat": ("mesh_flat", 40, 1.0, False, True),
    # the last collapse deletes what is left: no cost remains for the next pass's threshold
    "to_nothing_triangle": ("mesh_triangle", 0, 0.2, True, True),
    "to_nothing_quad": ("mesh_quad", 0, 0.2, True, True),
    "to_one_of_quad": ("mesh_quad", 1, 1.0, True, True),
}
BAD_STRICTNESS = [1.5, -0.1, float("nan")]
_want = {}


def want(name, request):
    """the restatement's result of a case, computed once"""
    if name not in _want:
        fixture, budget, strictness, rbe, equi = CASES[name]
        V, F = request.getfixturevalue(fixture)
        _want[name] = R.simplify(V, F, budget, strictness, rbe, equi)
    return _want[name]


def check_properties(name, request, v, f, stats):
    fixture, budget, _, rbe, _ = CASES[name]
    V, F = request.getfixturevalue(fixture)
    if name == "b":  # no edge may collapse: the threshold doubles until it is infinite; only re-indexing is left
        assert stats[1] == R.EXIT_INFINITE_THRESHOLD and stats[0] > 3
        assert np.array_equal(v, V) and np.array_equal(f, F)
    elif name == "c":  # the loop is not entered
        assert stats == (0, R.EXIT_BUDGET)
        assert np.array_equal(v, V) and np.array_equal(f, F)
    elif name in ("s0_a", "s0_flat"):  # the smallest cost is negative: it doubles to -inf and nothing collapses
        assert stats[1] == R.EXIT_INFINITE_THRESHOLD and stats[0] > 3
        assert np.array_equal(v, V) and np.array_equal(f, F)
    elif name.startswith("to_"):  # one pass, one collapse, nothing left: empty arrays, not an index into no costs
        assert stats == (1, R.EXIT_BUDGET) and v.shape == (0, 3) and f.shape == (0, 3)
    elif name == "s1_flat":  # every edge is under the threshold; the boundary stays, so the budget is out of reach
        assert stats[1] == R.EXIT_INFINITE_THRESHOLD and budget < len(f) < len(F)
    else:
        assert stats[1] == R.EXIT_BUDGET and stats[0] > 1
        assert budget - 2 <= len(f) <= budget  # a collapse removes at most two faces
        assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    if name == "s1_a":
        assert stats != want("a", request)[2] and not np.array_equal(f, want("a", request)[1])
    if name == "d_boundary":
        assert len(v) != len(want("a", request)[0]) or not np.array_equal(v, want("a", request)[0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_simplifier_matches_the_restatement(built, request, name):
    from facebook360_dep_amd import derp

    fixture, budget, strictness, rbe, equi = CASES[name]
    V, F = request.getfixturevalue(fixture)
    wv, wf, wstats = want(name, request)
    v, f, stats = derp.mesh_simplify_host(V, F, budget, strictness, rbe, equi)
    print("case %s: %d -> %d faces, %d -> %d vertices, %d passes, exit %d" % (name, len(F), len(f), len(V), len(v), *stats))
    assert stats == wstats
    assert f.shape == wf.shape and np.array_equal(f, wf)
    assert v.shape == wv.shape and v.tobytes() == wv.tobytes()  # fp64 vertices, bit for bit
    check_properties(name, request, v, f, stats)


def test_host_setup_matches_the_restatement(built, mesh_a):
    from facebook360_dep_amd import derp

    for equi in (True, False):
        got = derp.mesh_setup_host(*mesh_a, equi_error=equi)
        for g, w, what in zip(got, R.setup(*mesh_a, equi_error=equi), ("face planes", "edge costs", "vertex quadrics")):
            assert g.tobytes() == w.tobytes(), (what, equi)
    # the set-up handed in and the set-up computed inside give the same mesh
    a = derp.mesh_simplify_host(*mesh_a, 600)
    b = derp.mesh_simplify_host(*mesh_a, 600, setup=derp.mesh_setup_host(*mesh_a))
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_host_entries_refuse_bad_arguments(built, mesh_a):
    from facebook360_dep_amd import derp

    V, F = mesh_a
    bad = F.copy()
    bad[7, 1] = len(V)  # an index past the vertices
    with pytest.raises(derp.DerpError):
        derp.mesh_simplify_host(V, bad, 600)
    with pytest.raises(derp.DerpError):
        derp.mesh_setup_host(V, bad)
    with pytest.raises(derp.DerpError):
        derp.mesh_simplify_host(V, F, -1)
    for strictness in BAD_STRICTNESS:  # getThreshold's index would leave its vector
        with pytest.raises(derp.DerpError):
            derp.mesh_simplify_host(V, F, 600, strictness)
        with pytest.raises(derp.DerpError):
            derp.mesh_simplify_host(V, F, 600, strictness, setup=derp.mesh_setup_host(V, F))
    for strictness in (0.0, -0.0, 1.0):
        derp.mesh_simplify_host(V, F, len(F), strictness)


# ---------------------------------------------------------------- the same cases under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh") / "mesh_simplify_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "mesh_simplify_main.cpp"),
                           os.path.join(ROOT, "facebook360_dep_amd", "csrc", "derp_simplify.cpp")])
    return exe


@pytest.mark.parametrize("name", sorted(CASES))
def test_sanitized_program_matches_the_restatement(harness, request, tmp_path, name):
    fixture, budget, strictness, rbe, equi = CASES[name]
    V, F = request.getfixturevalue(fixture)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<QQ", len(V), len(F)) + V.astype(np.float64).tobytes() + F.astype(np.int32).tobytes())
    p = subprocess.run([harness, "run", src, dst, str(budget), repr(strictness), str(int(rbe)), str(int(equi))],
                       capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-1500:]
    assert p.returncode == 0, p.stderr[-500:]
    raw = open(dst, "rb").read()
    nv, nf, passes, reason = struct.unpack("<QQQQ", raw[:32])
    v = np.frombuffer(raw, np.float64, nv * 3, 32).reshape(-1, 3)
    f = np.frombuffer(raw, np.int32, nf * 3, 32 + nv * 24).reshape(-1, 3)
    wv, wf, wstats = want(name, request)
    assert (passes, reason) == wstats
    assert np.array_equal(f, wf) and v.tobytes() == wv.tobytes()


@pytest.mark.parametrize("strictness", BAD_STRICTNESS)
def test_sanitized_program_refuses_strictness_out_of_range(harness, mesh_a, tmp_path, strictness):
    V, F = mesh_a
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<QQ", len(V), len(F)) + V.astype(np.float64).tobytes() + F.astype(np.int32).tobytes())
    p = subprocess.run([harness, "run", src, dst, "600", repr(strictness), "0", "1"], capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-1500:]
    assert p.returncode == 1 and "bad arguments" in p.stderr and not os.path.exists(dst)
