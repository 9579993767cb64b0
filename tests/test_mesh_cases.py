"""tests/mesh_cases.py against the restatement alone (no GPU, no library): every case reaches what it exists for. All
conditions, no tolerance."""
import numpy as np
import pytest

from tests import mesh_cases as M
from tests import mesh_parallel_ref as P
from tests import mesh_ref as R

F32 = np.float32
ALL_OUTCOMES = (1 << 1 | 1 << 2, 1 << 0 | 1 << 3, 1, 2, 4, 8, 0)


def test_sizes_are_what_they_are_for():
    faces = {s: len(M.build_case("size_%dx%d" % s)["want"]["F"]) for s in M.SIZES}
    print("faces by size: %s" % faces)
    assert [faces[s] for s in ((1, 1), (9, 1), (1, 9))] == [0, 0, 0]
    assert [faces[s] for s in ((2, 2), (3, 2), (2, 3))] == [2, 4, 4]
    assert all(w * h == M.BLOCK for w, h in ((16, 16), (64, 4), (128, 2)))
    assert [M.boundary_pixels(w, 2)[1] for w in (255, 256, 257)] == [(1, 1), (0, 1), (256, 0)]  # row 1: in, at, after
    assert (1025 * 256 + M.BLOCK - 1) // M.BLOCK == 1025 > 1024
    assert len(M.build_case("single_triangle")["want"]["F"]) == 1 and len(M.build_case("single_triangle")["want"]["V"]) == 3


@pytest.mark.parametrize("size", [s for s in M.SIZES if s[0] * s[1] > M.BLOCK], ids=lambda s: "%dx%d" % s)
def test_faces_are_kept_at_the_block_boundary(size):
    """the last pixel of block 0 and the first of block 1 are vertices of kept faces, every quad they are a corner of is
    whole, and where they are the base (top left corner) of a quad, both of its faces are kept"""
    w, h = size
    c = M.build_case("size_%dx%d" % size)
    m, d = c["want"], c["disparity"]
    # the map itself: a tear, a NaN that is no corner
    assert m["outcomes"].get(0, 0) > 0 and m["outcomes"].get(9, 0) + m["outcomes"].get(6, 0) > 0
    nan = np.argwhere(np.isnan(d))
    assert len(nan) == 1 and tuple(nan[0]) not in {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
    assert m["unmasked"] == len(m["F"]) or h == 1 or w == 1  # (the NaN tears its quads: z is NaN, every ratio false)
    # vertices of the restatement by pixel: a kept vertex's x, y name its pixel
    cam = M.camera(c["camera"])
    px = np.rint(m["V"][:, 0] / (cam["resolution"][0] / w) - 0.5).astype(int)
    py = np.rint(m["V"][:, 1] / (cam["resolution"][1] / h) - 0.5).astype(int)
    index_of = {(int(x), int(y)): i for i, (x, y) in enumerate(zip(px, py))}
    assert len(index_of) == len(m["V"])
    for x, y in M.boundary_pixels(w, h):
        assert (x, y) in index_of, "pixel (%d, %d) is in no kept face" % (x, y)
        for qx in (x - 1, x):
            for qy in (y - 1, y):
                if 0 <= qx < w - 1 and 0 <= qy < h - 1:
                    corners = [index_of.get(p) for p in ((qx, qy), (qx + 1, qy), (qx, qy + 1), (qx + 1, qy + 1))]
                    assert None not in corners
                    inside = np.isin(m["F"], corners).all(axis=1).sum()
                    assert inside == 2, "quad (%d, %d) keeps %d faces" % (qx, qy, inside)
    bases = [(x, y) for x, y in M.boundary_pixels(w, h) if x < w - 1 and y < h - 1]
    print("%d x %d: block-boundary pixels %s, quad bases among them %s" % (w, h, M.boundary_pixels(w, h), bases))
    if size in ((257, 2), (65, 5), (1025, 256)):
        assert len(bases) >= 1
    if size in ((65, 5), (1025, 256)):
        assert len(bases) == 2  # faces based in the last pixel of block 0 and in the first of block 1


def test_specials_24_reaches_every_class():
    c = M.build_case("specials_24")
    d, m = c["disparity"], c["want"]
    bits = d.view(np.uint32)
    for v in M.SPECIAL_VALUES:
        if v != v:
            assert np.isnan(d).any()
        else:
            assert (bits == np.array(v, F32).view(np.uint32)).any(), v
    assert 0.5 < (d == F32(0.25)).mean() < 0.7
    with np.errstate(all="ignore"):
        assert np.isposinf(F32(1) / F32(1e-45)) and 0 < F32(1) / F32(3e38) < np.finfo(F32).tiny
    print("specials_24: %d kept faces of %d, outcomes %s" % (len(m["F"]), m["unmasked"], sorted(m["outcomes"].items())))
    for outcome in ALL_OUTCOMES:
        assert m["outcomes"].get(outcome, 0) > 0, outcome
    assert m["unmasked"] > len(m["F"]) > 0
    bad = (~np.isfinite(m["V"])).any(axis=1).sum()
    z = m["V"][:, 2]
    assert bad >= 1
    # download's clamp takes z < 0 and leaves -0: both are there
    assert (z < 0).any() and ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()
    planes, costs, vq = M.setup_case("specials_24", True)
    counts = (int(np.isnan(costs).sum()), int((costs < 0).sum()), int((costs == 0).sum()), int((costs > 0).sum()))
    print("specials_24: %d non-finite vertices, %d NaN plane values, NaN / negative / zero / positive costs %s"
          % (bad, np.isnan(planes).sum(), counts))
    assert min(counts) >= 1


def test_flat_12_has_few_costs_of_every_sign():
    planes, costs, vq = M.setup_case("flat_12", True)
    counts = (int((costs < 0).sum()), int((costs == 0).sum()), int((costs > 0).sum()))
    distinct = len(np.unique(costs))
    print("flat_12: negative / zero / positive costs %s, %d distinct" % (counts, distinct))
    assert not np.isnan(costs).any() and min(counts) >= 1 and distinct < 10
    assert counts == (44, 160, 522) and distinct == 4


def test_tear_ratios_decide_the_result():
    def outcome(name):
        m = M.build_case(name)["want"]
        return m["outcomes"], len(m["V"]), len(m["F"])

    # z ratios of exactly 0.5: `>` against `>=` at tear 0.5, and one float below
    assert outcome("tear_exact_0.5") == ({4: 1}, 3, 1)
    assert outcome("tear_exact_below_0.5") == ({9: 1}, 4, 2)
    assert outcome("tear_exact_0") == ({9: 1}, 4, 2)
    for name in ("1", "1.5", "nan"):
        assert outcome("tear_exact_" + name) == ({0: 1}, 0, 0)
    assert F32(M.HALF_BELOW) < F32(0.5) and float(F32(M.HALF_BELOW)) == M.HALF_BELOW
    faces = [len(M.build_case("tear_70x37_%g" % t)["want"]["F"]) for t in M.TEAR_RATIOS_70]
    print("70 x 37 faces at tear ratios %s: %s (0.95: %d)" % (M.TEAR_RATIOS_70, faces, len(M.build_case("scale_1")["want"]["F"])))
    assert all(a != b for a, b in zip(faces, faces[1:]))
    assert len(M.build_case("scale_1")["want"]["F"]) not in faces


def test_scales_masks_and_cameras():
    for s, size in M.DEPTH_SCALES.items():
        m = M.build_case("scale_%.3g" % s)["want"]
        assert (m["w"], m["h"]) == size, s
    assert len(M.build_case("scale_0.02")["want"]["F"]) == 0
    assert int(np.rint(70 * 0.01)) == 1 and int(np.rint(37 * 0.01)) == 0  # 0.01 leaves no rows
    ties = M.build_case("scale_ties_5x7")["want"]
    assert (ties["w"], ties["h"]) == (2, 4)  # 2.5 -> 2 and 3.5 -> 4
    plain = len(M.build_case("scale_1")["want"]["F"])
    faces = {n: len(M.build_case("mask_" + n)["want"]["F"]) for n in ("own_size", "one", "zero", "larger")}
    print("70 x 37 faces under the masks: %s (no mask: %d)" % (faces, plain))
    assert faces["one"] == plain and faces["zero"] == 0 and 0 < faces["own_size"] < plain and 0 < faces["larger"] < plain
    assert set(np.unique(M.build_case("mask_larger")["args"]["mask"])) == {0, 2, 255}
    both = M.build_case("mask_and_scale")["want"]
    assert (both["w"], both["h"]) == (35, 18) and 0 < len(both["F"]) < both["unmasked"]
    cam = M.camera("real")
    assert cam["resolution"] == [3360, 2160] and cam["focal"][0] == -cam["focal"][1]
    for name, (w, h) in (("real_84x54", (84, 54)), ("real_50x38", (50, 38))):
        assert M.build_case(name)["disparity"].shape == (h, w)
    assert 3360 / 84 == 2160 / 54 and 3360 / 50 != 2160 / 38
    assert M.build_case("real_rescaled")["args"]["resolution"] == [840.0, 540.0]
    a, b = M.build_case("real_84x54")["want"]["V"], M.build_case("real_rescaled")["want"]["V"]
    assert a.shape == b.shape and (a != b).all()  # another pixel size and another focal


def _result(kind, name):
    v, f, stats = M.simplify_case(kind, name)["out"]
    return stats, v.tobytes(), f.tobytes()


def test_strictness_decides_the_result():
    for kind, name, base in (("parallel", "flat_s0", "flat_s0.2"), ("parallel", "flat_s1", "flat_s0.2"),
                             ("parallel", "depth_s1", "depth_s0.2"), ("parallel", "depth_s0.5", "depth_s0.2"),
                             ("sequential", "flat_s0", "flat_s0.2"), ("sequential", "flat_s1", "flat_s0.2"),
                             ("sequential", "depth_s1", "depth_s0.2")):
        a, b = _result(kind, name), _result(kind, base)
        print("%s %s against %s: stats %s / %s, the mesh %s" % (kind, name, base, a[0], b[0], "differs" if a[1:] != b[1:] else "is the same"))
        assert a[0] != b[0]  # (the passes at the least: the flat map can end at the same mesh by another road)
        if name.startswith("depth") or (kind, name) == ("sequential", "flat_s1"):
            assert a[1] != b[1] and a[2] != b[2]  # other vertices and other faces
    passes = [M.simplify_case("parallel", n)["out"][2][0] for n in ("flat_s0", "flat_s0.2", "flat_s1")]
    assert passes[0] > passes[1] > passes[2]


def test_simplifier_cases_end_where_they_should():
    def out(name, kind="parallel"):
        c = M.simplify_case(kind, name)
        return len(c["F"]), c["budget"], len(c["out"][0]), len(c["out"][1]), c["out"][2]

    assert out("triangle_to_nothing") == (1, 0, 0, 0, (1, R.EXIT_BUDGET))  # the empty-output path
    assert M.simplify_case("parallel", "triangle_to_nothing")["out"][0].shape == (0, 3)
    assert out("ramp_3x3_inner")[3] == 8 and out("ramp_3x3_boundary")[3] == 3
    nf, budget, _, left, stats = out("budget_is_faces")
    assert budget == nf == left and stats == (0, R.EXIT_BUDGET)
    nf, budget, _, left, stats = out("budget_one_less")
    assert budget == nf - 1 and left in (nf - 1, nf - 2) and stats == (1, R.EXIT_BUDGET)
    for name in ("half_256x2", "half_257x2", "half_16x16"):
        nf, budget, _, left, stats = out(name)
        assert budget == nf // 2 and budget - 1 <= left <= budget and stats[0] >= 1, name
    assert out("strip_boundary")[3] == 10
    for name in ("half_256x2_kept", "half_257x2_kept"):  # every vertex lies on the boundary, which stays
        nf, budget, nv, left, stats = out(name)
        assert left == nf > budget and stats == (0, P.EXIT_NO_CANDIDATES), name
    for name in ("specials_s0.2", "specials_s1"):
        nf, budget, _, left, stats = out(name)
        assert stats[0] >= 1 and left < nf, name
    assert out("quad_to_nothing", "sequential")[3] == 2 and out("ramp_3x3_to_nothing", "sequential")[3] == 8
    # the boundary free to go: the last collapse leaves no face, and the loop ends with no cost to index
    assert out("triangle_to_nothing", "sequential") == (1, 0, 0, 0, (1, R.EXIT_BUDGET))
    assert out("quad_to_nothing_boundary", "sequential") == (2, 0, 0, 0, (1, R.EXIT_BUDGET))
    assert out("ramp_3x3_boundary", "sequential")[3] == 3


def test_threshold_index_is_cut_at_the_last_cost():
    n = 2 ** 24 + 4
    assert int(F32(1) * F32(n - 1)) > n - 1  # float(2^24 + 3) rounds up to 2^24 + 4
    assert R.threshold_index(1.0, n) == n - 1
    for strictness in (0.0, 0.2, 0.5, 0.8, 1.0):
        for m in (1, 2, 3, 726, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, n, 2 ** 25 + 7, 50_000_000, 2 ** 31 - 1, 2 ** 31 + 5,
                  3 * (2 ** 31 - 1)):  # (the last two: more costs than an int counts, the host entry's limit)
            idx = R.threshold_index(strictness, m)
            assert 0 <= idx <= m - 1
            assert idx == int(F32(strictness) * F32(m - 1)) or (strictness == 1.0 and m > 2 ** 24)  # nothing else moves


def test_simplifier_cases_are_quick():
    slow = []
    for kind, table in (("parallel", M.PARALLEL_CASES), ("sequential", M.SEQUENTIAL_CASES)):
        for name in table:
            c = M.simplify_case(kind, name)
            print("%-10s %-22s %5d -> %5d faces, stats %s, %.2f s" % (kind, name, len(c["F"]), len(c["out"][1]), c["out"][2], c["seconds"]))
            if not c["seconds"] < 5:
                slow.append((kind, name, c["seconds"]))
    assert not slow, slow
