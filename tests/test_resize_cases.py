"""The cases of tests/resize_cases.py on the CPU alone: every code path of cv::resize(INTER_AREA) is reached by every kind
that can reach it, and the conditions the cases are there for are met on the oracle's own images: exact .5 means that
round both ways off the 2 x 2 shortcut and only up on it, a mask mean that the fp32 product puts on the other side of
the threshold than the exact quotient, u16 block sums past 2^24, table taps under the 1e-3 cut. A case that does not is
a broken case; the GPU file (tests/test_gpu_resize_limits.py) then compares the device with the same oracle images bit
for bit. Last, the oracle itself is held to the float64 exact area average within a derived bound."""
import numpy as np
import pytest

from tests import resize_cases as RC

U = 2.0 ** -24  # the unit roundoff of fp32


def reachable(kind):
    paths = set(RC.PATHS)
    paths.discard("int2x2" if kind in RC.FLOAT_KINDS else "enlarge")
    if kind == "bgra":
        paths.discard("refused")  # derp_gc_upload's own size check answers before the resize is asked
    return paths


def test_every_path_reached_per_kind():
    for kind in RC.KINDS:
        reached = {}
        for n in RC.NAMES:
            if RC.CASES[n][0] == kind:
                reached.setdefault(RC.path_of(n), []).append(n)
        for (k, (sw, sh), (dw, dh)) in RC.REFUSALS:
            if k == kind:
                assert RC.classify(sw, sh, dw, dh, k)[0] == "refused"
                reached.setdefault("refused", []).append("%dx%d_to_%dx%d" % (sw, sh, dw, dh))
        print("%-6s %s" % (kind, ", ".join("%s: %d" % (p, len(reached.get(p, []))) for p in RC.PATHS)))
        assert set(reached) == reachable(kind), (kind, sorted(reached))


def test_classifier_on_known_geometries():
    """the rule on the geometries whose path the case list is built around"""
    want = {
        ((102, 68), (102, 68)): "identity", ((102, 68), (51, 34)): "int2x2", ((102, 68), (6, 4)): "int_block",
        ((102, 68), (3, 2)): "int_block", ((102, 68), (51, 68)): "int_block", ((102, 68), (102, 34)): "int_block",
        ((102, 68), (51, 17)): "int_block", ((102, 68), (34, 17)): "int_block", ((102, 68), (101, 67)): "table",
        ((102, 68), (100, 68)): "table_forced_y", ((102, 68), (102, 67)): "table_forced_x", ((102, 68), (7, 5)): "table",
        ((102, 68), (51, 67)): "table_forced_x", ((102, 68), (101, 34)): "table_forced_y",
        ((102, 68), (1, 1)): "int_block", ((102, 68), (1, 68)): "int_block", ((102, 68), (102, 1)): "int_block",
        ((2001, 3), (2000, 3)): "table_forced_y", ((1001, 3), (999, 3)): "table_forced_y",
        ((1, 9), (1, 3)): "int_block", ((1, 9), (1, 4)): "table_forced_x", ((9, 1), (4, 1)): "table_forced_y",
    }
    for ((sw, sh), (dw, dh)), path in want.items():
        assert RC.classify(sw, sh, dw, dh, "u16")[0] == path, (sw, sh, dw, dh)
        float_path = "int_block" if path == "int2x2" else path
        assert RC.classify(sw, sh, dw, dh, "f32")[0] == float_path, (sw, sh, dw, dh)
    assert RC.classify(102, 68, 150, 100, "f32x3")[0] == "enlarge"
    assert RC.classify(102, 68, 51, 100, "f32")[0] == "enlarge"
    assert RC.classify(102, 68, 51, 100, "u8")[0] == "refused"
    # the geometries kind 4 cannot be given through derp_gc_upload
    print("left out of kind 4:", RC.GC_LEFT_OUT)
    assert all(not any(RC.CASES[n][0] == "bgra" and RC.CASES[n][2:] == g for n in RC.NAMES) for g in RC.GC_LEFT_OUT)
    # its uploads hold every other case once, four different geometries each
    assert sorted(n for b in RC.GC_BATCHES for n in b) == [n for n in RC.NAMES if RC.CASES[n][0] == "bgra"]
    assert all(len({RC.CASES[n][2:] for n in b}) == len(b) == 4 for b in RC.GC_BATCHES)


def _ties(name):
    """-> (exact .5 means of a case, those the oracle rounded up, those it rounded down)"""
    ex = RC.exact(name)
    got = RC.oracle(name).astype(np.float64)
    tie = ex - np.floor(ex) == 0.5
    up, down = tie & (got == ex + 0.5), tie & (got == ex - 0.5)
    assert (up | down)[tie].all()
    return int(tie.sum()), int(up.sum()), int(down.sum())


def test_ties_round_both_ways_off_the_2x2_shortcut(built):
    """the 2 x 2 shortcut rounds half up, (a + b + c + d + 2) >> 2; every other path rounds half to even"""
    for kind, pattern in (("u16", "ties"), ("u8", "half")):
        n22 = RC.name_of(kind, pattern, RC.BASE, (51, 34))
        ties, up, down = _ties(n22)
        print("%s: %d ties, %d up, %d down" % (n22, ties, up, down))
        assert RC.path_of(n22) == "int2x2" and ties > 0 and up == ties and down == 0
    for kind in ("u16", "u8"):
        n22 = RC.name_of(kind, "ties", RC.BASE, (51, 34))
        assert _ties(n22)[1] == _ties(n22)[0] > 0
        for dst in ((51, 68), (102, 34), (51, 17)):
            name = RC.name_of(kind, "ties", RC.BASE, dst)
            ties, up, down = _ties(name)
            print("%s: %d ties, %d up, %d down" % (name, ties, up, down))
            assert RC.path_of(name) == "int_block" and up > 0 and down > 0
    # the forced table beside a fractional axis has no exact .5 means to speak of; its cells must not take the shortcut
    # either, which the 2 x 1 and 1 x 2 blocks above and the bit-for-bit comparison on the device pin


def test_half_mask_to_one_pixel_is_127(built):
    """half of 102 x 68 texels are 255: the exact mean is 127.5, and 884340 * (1.f / 6936) in fp32 lies below it: 127,
    where a division by the area, or a sum in float64, gives 127.5 -> 128"""
    name = RC.name_of("u8", "half", RC.BASE, (1, 1))
    src = RC.case_source(name)
    assert int(src.astype(np.int64).sum()) == 884340 and (src == 255).sum() * 2 == src.size
    assert RC.exact(name)[0, 0] == 127.5
    got = RC.oracle(name)
    print("half mask to 1 x 1:", int(got[0, 0]), "fp32 product:", np.float32(884340) * (np.float32(1) / np.float32(6936)))
    assert got.shape == (1, 1) and got[0, 0] == 127
    assert np.float32(884340) / np.float32(6936) == np.float32(127.5)
    # at 2 x 2 the same mask gives 128 where a block straddles the halves: both sides of `> 127` are on show
    small = RC.oracle(RC.name_of("u8", "half", RC.BASE, (51, 34)))
    assert (small == 128).any()


def test_block_sums_pass_2_to_the_24(built):
    """past 2^24 the fp32 sum of u16 texels rounds at every addition: its order is part of the result"""
    for dst, factor in (((6, 4), 17), ((3, 2), 34), ((1, 1), 102 * 68)):
        name = RC.name_of("u16", "bright", RC.BASE, dst)
        area = (RC.BASE[0] // dst[0]) * (RC.BASE[1] // dst[1])
        sums = RC.exact(name) * area
        print("%s: block sums up to %.0f (2^24 = %d)" % (name, sums.max(), 1 << 24))
        assert RC.path_of(name) == "int_block" and sums.min() > 2 ** 24


def test_strips_drop_taps():
    for n in RC.NAMES:
        dx, dy = RC.dropped_of(n)
        assert 0 <= dx <= RC.TAP_CUT and 0 <= dy <= RC.TAP_CUT
    for (src, dst) in (((2001, 3), (2000, 3)), ((2001, 3), (1999, 3)), ((1001, 3), (1000, 3)), ((1001, 3), (999, 3))):
        path, (dx, dy) = RC.classify(src[0], src[1], dst[0], dst[1], "u16")
        cells = RC.area_table(src[0], dst[0])[0]
        short = min(sum(w for _, w in taps) for taps in cells)
        lightest = min(w for taps in cells for _, w in taps)
        print("%d -> %d: widest piece cut %.3g of a pixel, lightest cell weighs %.6f, lightest tap kept %.6f" %
              (src[0], dst[0], dx, short, lightest))
        assert path == "table_forced_y" and dy == 0
        if dst[0] == 999:  # cell ends fall on multiples of 2 / 999 of a pixel: 1000 / 999 leaves 1.001e-3, just kept
            assert dx == 0 and short > 1 - 1e-12 and RC.TAP_CUT < lightest * src[0] / dst[0] < 1.01 * RC.TAP_CUT
        else:
            assert dx > 1e-4 and short < 1 - 1e-4
    # nothing else drops a tap, but for pieces that are the rounding of a cell's end in float64 (102 -> 100: 50 * 1.02)
    assert all(max(RC.dropped_of(n)) < 1e-12 for n in RC.NAMES if RC.CASES[n][2][0] not in (2001, 1001))


SANITY = [n for n in RC.NAMES if RC.is_finite(n) and RC.path_of(n) != "enlarge"]


def sanity_bound(name):
    kind, _, (sw, sh), (dw, dh) = RC.CASES[name]
    top = float(np.abs(RC.case_source(name).astype(np.float64)).max())
    n = RC.tap_count(sw, sh, dw, dh, kind)
    bound = n * U / (1 - n * U) * top
    bound += 2 * sum(RC.dropped_of(name)) * top
    if kind not in RC.FLOAT_KINDS:
        bound += 0.5
    return bound


@pytest.mark.parametrize("kind", RC.KINDS)
def test_oracle_within_bound_of_exact_area_average(built, kind):
    """oracle_lib.cv_resize_area against the float64 exact area average, on every finite shrinking case (the enlarging
    ones are no area average: tests/test_oracle_cv.py holds that restatement to its own properties).

    The bound, with u = 2^-24, top = max |src| and n = resize_cases.tap_count, the fp32 roundings on the way to one
    result: the oracle computes sum_i w_i s_i with weights w_i >= 0 that sum to 1 (before their own rounding), and the
    standard bound of a recursive fp32 sum of products gives |computed - exact| <= gamma_n sum_i w_i |s_i| <=
    gamma_n top, gamma_n = n u / (1 - n u).
      * identity and the 2 x 2 shortcut: n = 0 (a copy; an integer sum);
      * an integer block of area A: A - 1 additions, the rounding of 1.f / A and the product: n = A + 1;
      * the tables, with at most nx and ny taps per cell: per row a weight's rounding, a product and nx - 1
        additions, the same over the rows: n = nx + ny + 2;
      * a table that drops end taps, each at most p <= 1e-3 of a source pixel wide (resize_cases.area_table reports
        the widest, p), one at each end of a cell that is one pixel wide at least, is short of weight 2 p per axis at
        most: + 2 (p_x + p_y) top, which is 2e-3 top at most for the strips, whose rows keep every tap;
      * the integer kinds round the result to an integer (the clamp to the type's range moves it no further from an
        exact average that lies within the range): + 0.5. Kind 4's u16 stage is what is compared.
    The float64 reference's own rounding (1e-16 relative) is far below u and left out."""
    worst = {}
    for name in SANITY:
        if RC.CASES[name][0] != kind:
            continue
        dw, dh = RC.CASES[name][3]
        got = RC.oracle_resize(kind, RC.case_source(name), dw, dh, u16_stage=True) if kind == "bgra" else RC.oracle(name)
        want = RC.exact(name)
        err = float(np.abs(got.astype(np.float64) - want).max())
        bound = sanity_bound(name)
        print("%-40s %-15s max |oracle - exact| %.6g, bound %.6g" % (name, RC.path_of(name), err, bound))
        assert err <= bound, name
        key = (RC.CASES[name][1], RC.path_of(name))
        worst[key] = max(worst.get(key, 0.0), err)
    assert worst
