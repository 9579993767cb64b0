"""cv::resize(INTER_AREA) on the device (k_resize_area<KIND>, k_resize_linear_area_f32<CN> of derp_kernels.h, driven by
resize_area_dev / get_area_tab of derp_capi.hip) on every kind, code path and size edge: every case of
tests/resize_cases.py against the oracle's image, bit for bit: NaN is NaN, +0 is not -0, 0 differing values, no
tolerance anywhere in this file. tests/test_resize_cases.py shows on the CPU that the cases reach every path per kind,
hold exact .5 means that round both ways, a mask mean on the threshold's edge, block sums past 2^24 and tables with taps
under the 1e-3 cut, and that the oracle lies within a derived bound of the exact area average.

Kinds 0 to 3 run through derp_resize_area, the pyramid builder through derp_build_pyramid_* and the level downloads,
kind 4 through derp_gc_upload / derp_gc_download_image; then the order independence of the per-context table cache and
the state of a context after a refused call."""
import numpy as np
import pytest

from tests import resize_cases as RC

pytestmark = pytest.mark.gpu

STANDALONE = [n for n in RC.NAMES if RC.CASES[n][0] != "bgra"]
LEVELS = [(102, 68), (51, 34), (6, 4), (51, 68), (102, 34), (51, 67), (101, 34), (101, 67), (100, 68), (102, 67), (7, 5),
          (3, 2), (1, 68), (102, 1), (1, 1)]


def cameras(n=4):
    from facebook360_dep_amd import synth

    return synth.make_rig(n, 64)["cameras"]


@pytest.fixture(scope="module")
def ctx(built):
    from facebook360_dep_amd import derp

    g = derp.Derp(cameras())
    yield g
    g.close()


def check(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    d = RC.differing(got, want)
    print("%s: %d of %d values differ" % (what, d, want.size))
    assert d == 0, what


@pytest.mark.parametrize("name", STANDALONE)
def test_resize_area(ctx, name):
    """kinds 0 to 3 stand-alone, one context for all: its table cache fills with every pair of the cases"""
    _, _, _, (dw, dh) = RC.CASES[name]
    check(ctx.resize_area(RC.case_source(name), dw, dh), RC.oracle(name), "%s (%s)" % (name, RC.path_of(name)))


def _level(kind, pattern, level):
    return RC.oracle(RC.name_of(kind, pattern, RC.BASE, LEVELS[level]))


def test_pyramid_builder(built):
    """derp_build_pyramid_*: one 102 x 68 frame in, levels on the identity, 2 x 2, block, table, forced-table and 1 x 1
    paths out. The half mask's levels hold 127 (1 x 1) and 128 (2 x 2, where a block straddles the halves): thresholds
    126, 127 and 128 show both sides of `>` on each. A second camera's build leaves the first camera's planes alone."""
    from facebook360_dep_amd import derp

    paths = {RC.classify(102, 68, w, h, "u8")[0] for (w, h) in LEVELS}
    assert {"identity", "int2x2", "int_block", "table", "table_forced_x", "table_forced_y"} <= paths and (1, 1) in LEVELS
    half = [_level("u8", "half", li) for li in range(len(LEVELS))]
    assert any((m == 127).any() for m in half) and any((m == 128).any() for m in half)
    src = lambda kind, pattern: RC.source(kind, pattern, *RC.BASE)
    g = derp.Derp(cameras(2), use_foreground_masks=1)
    try:
        g.set_pyramid(LEVELS, *RC.BASE)
        for pattern in RC.PATTERNS["u16"]:
            g.build_pyramid_color(0, src("u16", pattern))
            for li in range(len(LEVELS)):
                check(g.download_level_color(li, 0), _level("u16", pattern, li), "colour %s level %d" % (pattern, li))
        for pattern in RC.PATTERNS["f32"]:
            g.build_pyramid_background_disparity(0, src("f32", pattern))
            for li in range(len(LEVELS)):
                check(g.download_level_background(li, 0), _level("f32", pattern, li), "background %s level %d" % (pattern, li))
        for pattern in RC.PATTERNS["u8"]:
            for threshold in (127, 126, 128):
                g.build_pyramid_foreground_mask(0, src("u8", pattern), threshold)
                for li in range(len(LEVELS)):
                    want = (_level("u8", pattern, li) > threshold).astype(np.uint8)
                    check(g.download_level_mask(li, 0), want, "mask %s > %d level %d" % (pattern, threshold, li))
        # camera 0 now holds: colour "sat", background "special", mask "sat" > 128
        g.build_pyramid_color(1, src("u16", "ties"))
        g.build_pyramid_background_disparity(1, src("f32", "uniform"))
        g.build_pyramid_foreground_mask(1, src("u8", "half"), 127)
        g.build_pyramid_color(1, src("u16", "bright"))  # the second call
        for li in range(len(LEVELS)):
            check(g.download_level_color(li, 1), _level("u16", "bright", li), "camera 1 colour level %d" % li)
            check(g.download_level_background(li, 1), _level("f32", "uniform", li), "camera 1 background level %d" % li)
            check(g.download_level_mask(li, 1), (half[li] > 127).astype(np.uint8), "camera 1 mask level %d" % li)
            check(g.download_level_color(li, 0), _level("u16", "sat", li), "camera 0 colour kept, level %d" % li)
            check(g.download_level_background(li, 0), _level("f32", "special", li), "camera 0 background kept, level %d" % li)
            check(g.download_level_mask(li, 0), (_level("u8", "sat", li) > 128).astype(np.uint8),
                  "camera 0 mask kept, level %d" % li)
    finally:
        g.close()


@pytest.mark.parametrize("batch", range(len(RC.GC_BATCHES)))
def test_kind4_through_gc_upload(ctx, batch):
    """BGRA u16 -> int16: the oracle's u16 resize per channel, then rint(v * (32767 / 65535.0)) in float64. One upload
    holds four cameras with full and small sizes of their own.

    derp_gc_upload takes no small size below 3 x 3 (gc_check_sizes) and nothing enlarged, so these geometries of the
    cases are left out of this test only (resize_cases.GC_LEFT_OUT): 102 x 68 to 3 x 2, 1 x 1, 1 x 68 and 102 x 1,
    68 x 102 to 1 x 1, and the 1 x 9 / 9 x 1 sources. Kinds 0 to 3 run them above.

    What this kind cannot show: rint(v * 32767 / 65535) gives an even v and v + 1 the same int16, and those are the two
    values a .5 mean can round to, so the direction of a tie is invisible here. Kinds 0 and 1 pin it."""
    names = RC.GC_BATCHES[batch]
    assert len(names) == ctx.D
    ctx.gc_upload([RC.case_source(n) for n in names], [RC.CASES[n][3] for n in names])
    for cam, n in enumerate(names):
        check(ctx.gc_image(cam), RC.oracle(n), "camera %d: %s (%s)" % (cam, n, RC.path_of(n)))


CACHE_ORDER = (((102, 68), (51, 34)), ((102, 68), (51, 67)), ((102, 68), (51, 34)), ((102, 68), (101, 34)),
               ((102, 68), (51, 34)), ((100, 68), (51, 34)))
CACHE_INPUTS = (("u16", "ties"), ("u8", "half"), ("f32", "special"), ("f32x3", "uniform"))


def test_table_cache_order(built):
    """the tables are cached per context under (+-ssize, dsize): 102 -> 51 is asked for as an integer factor, then as
    the forced table beside 68 -> 67, and back; 68 -> 34 likewise beside 102 -> 101; 102 -> 51 and 100 -> 51 share a
    destination size. One context runs the calls in this order, for each kind in turn; each result must be what a
    context made for that call alone gives (its cache holds what the same call of the kinds before put there, nothing
    else), which in turn must be the oracle's."""
    from facebook360_dep_amd import derp

    assert [RC.classify(s[0], s[1], d[0], d[1], "u16")[0] for s, d in CACHE_ORDER] == [
        "int2x2", "table_forced_x", "int2x2", "table_forced_y", "int2x2", "table_forced_y"]
    fresh = {}
    for step, (s, d) in enumerate(CACHE_ORDER):
        g = derp.Derp(cameras(2))
        try:
            for kind, pattern in CACHE_INPUTS:
                fresh[step, kind] = g.resize_area(RC.source(kind, pattern, *s), *d)
                check(fresh[step, kind], RC.oracle_resize(kind, RC.source(kind, pattern, *s), *d),
                      "fresh context, %s %s -> %s" % (kind, s, d))
        finally:
            g.close()
    g = derp.Derp(cameras(2))
    try:
        for kind, pattern in CACHE_INPUTS:
            for step, (s, d) in enumerate(CACHE_ORDER):
                check(g.resize_area(RC.source(kind, pattern, *s), *d), fresh[step, kind],
                      "one context, call %d: %s %s -> %s" % (step, kind, s, d))
    finally:
        g.close()


def test_refusals_leave_the_context_working(built):
    """kinds 0 and 1 enlarged along either axis and a zero size are refused; the same context then resizes a case as
    before (through a forced table, which the refused call must not have left half made)"""
    from facebook360_dep_amd import derp

    g = derp.Derp(cameras(2))
    try:
        for (kind, (sw, sh), (dw, dh)) in RC.REFUSALS:
            pattern = RC.PATTERNS[kind][0]
            src = RC.source(kind, pattern, sw, sh)
            if min(dw, dh) > 0:
                match = r"%dx%d -> %dx%d" % (sw, sh, dw, dh)  # the refusal names the sizes
            else:
                match = "bad arguments"
            with pytest.raises(derp.DerpError, match=match):
                g.resize_area(src, dw, dh)
            name = RC.name_of(kind, pattern, RC.BASE, (51, 67))
            check(g.resize_area(RC.case_source(name), 51, 67), RC.oracle(name),
                  "%s after the refused %dx%d -> %dx%d" % (name, sw, sh, dw, dh))
    finally:
        g.close()
