"""The cases that tests/test_resize_cases.py (CPU) and tests/test_gpu_resize_limits.py (GPU) share: cv::resize(INTER_AREA)
as k_resize_area / k_resize_linear_area_f32 (derp_kernels.h) compute it, on every kind, code path and size edge, with the
oracle's image (oracle_lib.cv_resize_area) and the float64 exact area average (synth.resize_area) computed once per case.
Nothing here touches the GPU or the device library.

A case is (kind, pattern, (sw, sh), (dw, dh)); its name spells the four out. Kinds: "u16" (BGR u16, kind 0), "u8" (kind
1), "f32" (kind 2), "f32x3" (kind 3) and "bgra" (BGRA u16 in, int16 out, kind 4: only derp_gc_upload reaches it).

classify() restates the dispatch rule of cv::resize from its text (oracle_cv.h resizeAreaCv documents it), on its own:
it imports neither the oracle nor the library, and the two test files hold both of them to it."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
KINDS = ("u16", "u8", "f32", "f32x3", "bgra")
KIND_ID = {"u16": 0, "u8": 1, "f32": 2, "f32x3": 3, "bgra": 4}
FLOAT_KINDS = ("f32", "f32x3")
PATHS = ("identity", "int2x2", "int_block", "table", "table_forced_x", "table_forced_y", "enlarge", "refused")
PATTERNS = {
    "u16": ("uniform", "ties", "bright", "sat"),
    "u8": ("binary", "half", "ties", "sat"),
    "f32": ("uniform", "special"),
    "f32x3": ("uniform", "special"),
    "bgra": ("uniform", "ties", "bright", "sat"),
}
DBL_EPSILON = 2.220446049250313e-16
TAP_CUT = 1e-3  # computeResizeAreaTab leaves out an end tap that covers this much of a source pixel, or less


# ---- the rule ----
def integer_factor(ssize, dsize):
    """the factor of the "area fast" paths: ssize / dsize when it is an integer to within DBL_EPSILON, else 0"""
    scale = ssize / dsize
    i = int(round(scale))  # (halves never get here as integers: the test below refuses them)
    return i if i >= 1 and abs(scale - i) < DBL_EPSILON else 0


def area_table(ssize, dsize):
    """computeResizeAreaTab of one axis -> (cells: per destination index a list of (source index, weight in float64
    before its rounding to fp32), the widest end piece, in source pixels, that the 1e-3 cut left out: 0 when none)"""
    scale = ssize / dsize
    cells, dropped = [], 0.0
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        width = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > TAP_CUT:
            taps.append((s1 - 1, (s1 - f1) / width))
        elif s1 - f1 > 0:
            dropped = max(dropped, s1 - f1)
        taps += [(s, 1.0 / width) for s in range(s1, s2)]
        if f2 - s2 > TAP_CUT:
            taps.append((s2, min(min(f2 - s2, 1.0), width) / width))
        elif f2 - s2 > 0:
            dropped = max(dropped, f2 - s2)
        cells.append(taps)
    return cells, dropped


def classify(sw, sh, dw, dh, kind):
    """-> (path, (dropped_x, dropped_y)): which code path cv::resize(INTER_AREA) takes for a (sw, sh) image of `kind`
    resized to (dw, dh), as this project offers it (the integer kinds are not enlarged: refused), and per axis the
    widest end piece that a table leaves out (0 off the table paths)"""
    assert kind in KINDS
    if min(sw, sh, dw, dh) <= 0:
        return "refused", (0.0, 0.0)
    if (sw, sh) == (dw, dh):
        return "identity", (0.0, 0.0)
    if dw > sw or dh > sh:
        return ("enlarge" if kind in FLOAT_KINDS else "refused"), (0.0, 0.0)
    ix, iy = integer_factor(sw, dw), integer_factor(sh, dh)
    if ix and iy:
        return ("int2x2" if ix == 2 and iy == 2 and kind not in FLOAT_KINDS else "int_block"), (0.0, 0.0)
    # one fractional axis takes both through computeResizeAreaTab: the integer one gets a table too
    path = "table_forced_x" if ix else "table_forced_y" if iy else "table"
    return path, (area_table(sw, dw)[1], area_table(sh, dh)[1])


def tap_count(sw, sh, dw, dh, kind):
    """the fp32 roundings between the source texels and one result of the path, at most: what the accumulation bound
    of tests/test_resize_cases.py counts"""
    path = classify(sw, sh, dw, dh, kind)[0]
    if path in ("identity", "int2x2"):
        return 0  # a copy; an exact integer sum
    if path == "int_block":
        # area - 1 additions, the rounding of 1.f / area and the product with it
        return integer_factor(sw, dw) * integer_factor(sh, dh) + 1
    assert path.startswith("table")
    nx = max(len(t) for t in area_table(sw, dw)[0])
    ny = max(len(t) for t in area_table(sh, dh)[0])
    # per row: a weight's rounding, a product and nx - 1 additions (nx + 1); the same over the rows (ny + 1)
    return nx + ny + 2


# ---- geometries ----
BASE = (102, 68)
BASE_T = (68, 102)
GEOMETRIES = (
    [(BASE, d) for d in (
        (102, 68),  # identity
        (51, 34), (6, 4), (3, 2),  # factors 2, 17, 34 on both axes
        (51, 68), (102, 34), (51, 17), (34, 17),  # 2 x 1, 1 x 2, 2 x 4, 3 x 4
        (101, 67), (100, 68), (102, 67), (7, 5),  # fractional; one axis untouched, the other through a forced table
        (51, 67), (101, 34),  # an integer factor beside a fractional one: the forced table at factor 2
        (1, 1), (1, 68), (102, 1),
    )] +
    [(BASE_T, d) for d in ((34, 51), (4, 6), (67, 101), (68, 100), (34, 101), (1, 1))] +
    [((2001, 3), (2000, 3)), ((2001, 3), (1999, 3)), ((1001, 3), (1000, 3)), ((1001, 3), (999, 3))] +  # strips
    [((1, 9), (1, 3)), ((1, 9), (1, 4)), ((9, 1), (3, 1)), ((9, 1), (4, 1))]  # one pixel wide / high
)
ENLARGED = [(BASE, d) for d in ((150, 100), (204, 68), (102, 100), (51, 100))] + [((1, 9), (2, 12))]
# (kind, source, destination) that the library must refuse: the integer kinds enlarged along either axis, a zero size
REFUSALS = ([(k, BASE, d) for k in ("u16", "u8") for d in ((103, 68), (102, 69), (51, 100), (204, 136))] +
            [(k, BASE, d) for k in ("u16", "u8", "f32", "f32x3") for d in ((0, 34), (51, 0))])
# derp_gc_upload takes no small size below 3 x 3 (gc_check_sizes) and nothing enlarged: kind 4 runs on the rest
GC_MIN = 3


def name_of(kind, pattern, src, dst):
    return "%s_%s_%dx%d_to_%dx%d" % ((kind, pattern) + tuple(src) + tuple(dst))


def _build_cases():
    C = {}
    for kind in KINDS:
        geos = list(GEOMETRIES) + (ENLARGED if kind in FLOAT_KINDS else [])
        for (src, dst) in geos:
            if kind == "bgra" and min(dst) < GC_MIN:
                continue
            for pattern in PATTERNS[kind]:
                C[name_of(kind, pattern, src, dst)] = (kind, pattern, src, dst)
    return C


CASES = _build_cases()
NAMES = sorted(CASES)
# the geometries of GEOMETRIES that derp_gc_upload cannot express (a size rule of its own)
GC_LEFT_OUT = [(src, dst) for (src, dst) in GEOMETRIES if min(dst) < GC_MIN]
# kind 4 by uploads of four cameras: batch i gives camera k the k-th pattern at geometry i + 5 k, so that every case is
# uploaded once and the cameras of one upload differ in their full and small sizes
_GC_GEOMETRIES = [g for g in GEOMETRIES if g not in GC_LEFT_OUT]
GC_BATCHES = [[name_of("bgra", p, *_GC_GEOMETRIES[(i + 5 * k) % len(_GC_GEOMETRIES)]) for k, p in enumerate(PATTERNS["bgra"])]
              for i in range(len(_GC_GEOMETRIES))]


def path_of(name):
    kind, _, (sw, sh), (dw, dh) = CASES[name]
    return classify(sw, sh, dw, dh, kind)[0]


def dropped_of(name):
    kind, _, (sw, sh), (dw, dh) = CASES[name]
    return classify(sw, sh, dw, dh, kind)[1]


# ---- inputs ----
def _seed(*key):
    return [sum(ord(ch) * (i + 1) for i, ch in enumerate(str(k))) for k in key]


def _u16(pattern, w, h):
    rng = np.random.default_rng(_seed("u16", pattern, w, h))
    if pattern == "uniform":
        img = rng.integers(0, 65536, size=(h, w, 3))
    elif pattern == "ties":  # means of exactly .5 abound; a few 65535 keep the sums out of the small integers
        img = rng.integers(0, 4, size=(h, w, 3))
        img[rng.random((h, w, 3)) < 0.01] = 65535
    elif pattern == "bright":  # 17 x 17 of these sum past 2^24
        img = rng.integers(60000, 65536, size=(h, w, 3))
    else:
        assert pattern == "sat"
        img = np.full((h, w, 3), 65535)
    return img.astype(np.uint16)


def _u8(pattern, w, h):
    rng = np.random.default_rng(_seed("u8", pattern, w, h))
    if pattern == "binary":
        img = rng.integers(0, 2, size=(h, w)) * 255
    elif pattern == "half":  # the left half set, inverted in the bottom half: half the image is 255
        img = np.zeros((h, w), dtype=np.int64)
        img[:, :w // 2] = 255
        img[h // 2:] = 255 - img[h // 2:]
    elif pattern == "ties":  # the means of 0 / 255 texels tie at 127.5 alone, which both roundings take to 128
        img = rng.integers(0, 4, size=(h, w))
        img[rng.random((h, w)) < 0.01] = 255
    else:
        assert pattern == "sat"
        img = np.full((h, w), 255)
    return img.astype(np.uint8)


def _f32(pattern, w, h, cn):
    rng = np.random.default_rng(_seed("f32", pattern, w, h, cn))
    img = rng.random((h, w, cn), dtype=F32)
    if pattern == "special":
        for v in (np.nan, np.inf, -np.inf, -0.0):
            img[rng.random(img.shape) < 0.01] = F32(v)
        flat = img.reshape(-1)  # each of them once at least, whatever the size
        pos = rng.permutation(flat.size)
        for i, v in enumerate((np.nan, np.inf, -np.inf, -0.0)):
            flat[pos[i % flat.size]] = F32(v)
        # a stretch of -0 alone: a sum of -0 only is -0, beside any +0 it is +0
        img[h // 2, :max(1, w // 3)] = F32(-0.0)
    else:
        assert pattern == "uniform"
    return img if cn == 3 else np.ascontiguousarray(img[..., 0])


def _bgra(pattern, w, h):
    rng = np.random.default_rng(_seed("bgra", pattern, w, h))
    # alpha in blocks of 5 x 3 of 0 / 65535: their edges fall inside the cells of every factor
    blocks = rng.integers(0, 2, size=((h + 2) // 3, (w + 4) // 5)) * 65535
    alpha = np.repeat(np.repeat(blocks, 3, axis=0), 5, axis=1)[:h, :w]
    return np.ascontiguousarray(np.concatenate([_u16(pattern, w, h), alpha[..., None].astype(np.uint16)], axis=2))


@functools.lru_cache(maxsize=None)
def source(kind, pattern, w, h):
    """the seeded input of a kind and pattern at w x h, read-only"""
    if kind == "u16":
        img = _u16(pattern, w, h)
    elif kind == "u8":
        img = _u8(pattern, w, h)
    elif kind == "bgra":
        img = _bgra(pattern, w, h)
    else:
        img = _f32(pattern, w, h, 3 if kind == "f32x3" else 1)
    img.setflags(write=False)
    return img


def case_source(name):
    kind, pattern, (sw, sh), _ = CASES[name]
    return source(kind, pattern, sw, sh)


def is_finite(name):
    return CASES[name][1] != "special"


# ---- references ----
def to_int16(u16):
    """convertTo(CV_16S, 32767 / 65535.0) of a u16 image: the product in float64, rounded half to even, saturated"""
    return np.clip(np.rint(u16.astype(F64) * (32767.0 / 65535.0)), -32768, 32767).astype(np.int16)


def oracle_resize(kind, src, dw, dh, u16_stage=False):
    """the oracle's resize of an image of `kind`; kind 4 is its u16 resize per channel (the three colours in one call,
    the alpha replicated in another: `u16_stage` stops there) and then to_int16"""
    from oracle import oracle_lib as O

    if kind != "bgra":
        return O.cv_resize_area(src, dw, dh)
    bgr = O.cv_resize_area(np.ascontiguousarray(src[..., :3]), dw, dh)
    alpha = O.cv_resize_area(np.ascontiguousarray(np.repeat(src[..., 3:], 3, axis=2)), dw, dh)[..., :1]
    small = np.concatenate([bgr, alpha], axis=2)
    return small if u16_stage else to_int16(small)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's image of a case, read-only"""
    kind, _, _, (dw, dh) = CASES[name]
    out = oracle_resize(kind, case_source(name), dw, dh)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def exact(name):
    """the float64 exact area average of a finite, shrinking case (for kind 4: of its u16 stage), read-only"""
    from facebook360_dep_amd import synth

    _, _, _, (dw, dh) = CASES[name]
    assert is_finite(name) and path_of(name) not in ("enlarge", "refused")
    out = np.asarray(synth.resize_area(case_source(name).astype(F64), dw, dh))
    out.setflags(write=False)
    return out


def differing(a, b):
    """the values of two images that are not the same bits (every NaN counts as one value; +0 is not -0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == F32:
        both_nan = np.isnan(a) & np.isnan(b)
        return int(((a.view(np.uint32) != b.view(np.uint32)) & ~both_nan).sum())
    return int((a != b).sum())
