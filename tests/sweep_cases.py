"""The rigs, images and depth lists that tests/test_sweep_ref.py and tests/test_gpu_sweep*.py share, with the
restatement's results (tests/sweep_ref.py) computed once per case. Nothing here touches the GPU."""
import functools

import numpy as np

from tests import sweep_ref as R
from tests.geometric_cases import differing, isolated_rig, same  # noqa: F401  (the comparison the GPU tests use)

F32 = np.float32


def _rig(name):
    from facebook360_dep_amd import synth
    from tests import common

    if name == "rig4":
        return synth.make_rig(4, 64)["cameras"]
    if name == "rig2":
        return synth.make_rig(2, 64)["cameras"]
    if name == "rig34":
        return synth.make_rig(34, 64)["cameras"]
    if name == "mixed":
        return common.mixed_type_rig(64)["cameras"]
    if name == "real":
        return common.real_rig()["cameras"]
    if name == "real_np":
        return common.real_rig_no_principal()["cameras"]
    if name == "isolated":
        cams = isolated_rig()
        # the lone camera's field cut to 0.6 rad: the image's edges (0.5 rad) lie inside the circle, its corners outside
        cams[2] = dict(cams[2], fov=0.6)
        return cams
    raise KeyError(name)


def _same(sizes):
    return [(float(w), float(h)) for w, h in sizes]


# name -> (rig, image sizes, camera resolutions (None: the image sizes), (num_depths, min_depth_m, max_depth_m),
#          destinations compared, camera whose image has a transparent hole or None)
OVERLAP_CASES = {
    "rig4_32": ("rig4", [(32, 32)] * 4, None, (7, 1, 10), (0, 1, 2, 3), None),
    # 475 pixels: two blocks, the second partly empty; 50 depths in 13 runs of 4, the last of 2
    "rig4_25x19": ("rig4", [(25, 19)] * 4, None, (50, 1, 10), (0, 3), None),
    "rig4_one_depth": ("rig4", [(25, 19)] * 4, None, (1, 1, 10), (1,), None),
    # per-camera sizes; the resolutions Camera::rescale gets are resolution * scale, not rounded: 64 * 0.505 = 32.32,
    # a 27-pixel-high camera at 0.7 = 18.9, ...
    "rig4_mixed": ("rig4", [(32, 32), (25, 19), (32, 19), (16, 16)],
                   [(32.32, 32.32), (25.2, 18.9), (31.6, 19.3), (16.2, 15.8)], (7, 1, 10), (0, 1, 2, 3), 1),
    "mixed_40": ("mixed", [(40, 40)] * 6, None, (7, 1, 10), (0, 1, 2, 3, 4, 5), None),
    "mixed_50x38": ("mixed", [(50, 38)] * 6, [(50.4, 37.6)] * 6, (3, 1, 10), (0, 3, 5), None),
    "real_40": ("real", [(40, 40)] * 6, None, (3, 1, 10), (0, 2, 5), None),
    "real_np_50x38": ("real_np", [(50, 38)] * 6, None, (3, 1, 10), (1, 4), None),
    "rig34_16": ("rig34", [(16, 16)] * 34, None, (7, 1, 10), (0, 17, 33), None),
    "rig2": ("rig2", [(32, 32)] * 2, None, (7, 1, 10), (0, 1), None),
    # nobody overlaps camera 2; its resolution 31.2 lies below its image's 32 pixels, so the last row's and column's
    # centres (31.5) are off its own sensor: inside the image circle and seen by no camera, count == 0
    "isolated": ("isolated", [(32, 32)] * 3, [(32.0, 32.0), (32.0, 32.0), (31.2, 31.2)], (3, 1, 10), (0, 2), None),
}

# name -> (rig, image sizes, resolutions, (W, H), (num_depths, depth_min, depth_max), black_bg, hole, centred on camera or None)
EQUIRECT_CASES = {
    "rig4_64x32": ("rig4", [(32, 32)] * 4, None, (64, 32), (7, 1.0, 10.0), False, None, None),
    "rig4_38x19_black": ("rig4", [(25, 19)] * 4, None, (38, 19), (1, 1.0, 10.0), True, None, None),
    # the resolutions exceed the images: the truncated index reaches one past the edge and the clamp decides
    "rig4_mixed": ("rig4", [(32, 32), (25, 19), (32, 19), (16, 16)],
                   [(32.9, 32.9), (25.8, 19.9), (32.9, 19.9), (16.9, 16.9)], (64, 32), (7, 0.3, 10.0), False, 1, None),
    "mixed_64x32": ("mixed", [(40, 40)] * 6, None, (64, 32), (7, 1.0, 10.0), False, None, None),
    "real_38x19": ("real", [(50, 38)] * 6, None, (38, 19), (7, 1.0, 10.0), True, None, None),
    "real_np_64x32": ("real_np", [(40, 40)] * 6, None, (64, 32), (1, 1.0, 10.0), False, None, None),
    "rig34_64x32": ("rig34", [(16, 16)] * 34, None, (64, 32), (7, 1.0, 10.0), False, None, None),
    "rig2_38x19": ("rig2", [(32, 32)] * 2, None, (38, 19), (7, 1.0, 10.0), False, None, None),
    "isolated_64x32": ("isolated", [(32, 32)] * 3, None, (64, 32), (7, 1.0, 10.0), True, None, None),
    "rig4_centred": ("rig4", [(32, 32)] * 4, None, (64, 32), (7, 1.0, 10.0), False, None, 2),
}
BOUNDS_DEPTHS = (0.3, 2.0, 1000.0)
BOUNDS_CASES = ["rig4_64x32", "mixed_64x32", "rig2_38x19", "rig4_centred"]


def _images(sizes, hole, seed):
    """float BGRA in [0, 1), alpha 1, every texel different; `hole`: that camera has a transparent rectangle"""
    rng = np.random.default_rng(seed)
    out = []
    for i, (w, h) in enumerate(sizes):
        im = rng.random((h, w, 4), dtype=F32)
        im[:, :, 3] = 1
        if hole == i:
            im[h // 3:h // 3 + h // 4, w // 4:w // 4 + w // 3, 3] = 0
        out.append(im)
    return out


@functools.lru_cache(maxsize=None)
def overlap_case(name):
    """-> (cams, images, resolutions, disparities, destinations)"""
    rig, sizes, res, (num, lo, hi), dsts, hole = OVERLAP_CASES[name]
    return _rig(rig), _images(sizes, hole, 11), res or _same(sizes), R.overlap_disparities(num, lo, hi)[0], dsts


@functools.lru_cache(maxsize=None)
def overlap_rigged(name):
    cams, images, res, _, _ = overlap_case(name)
    return R.Rigged(cams, images, res)


@functools.lru_cache(maxsize=None)
def overlap_ref(name, dst):
    """-> (f32 [n, h, w, 4], count [n, h, w], edges at which a tap was clamped)"""
    disp = overlap_case(name)[3]
    outs, counts, clamped = [], [], set()
    for d in disp:
        stats = {}
        outs.append(overlap_rigged(name).overlaps(dst, d, stats=stats))
        counts.append(stats["count"])
        clamped |= stats["clamped"]
    return np.stack(outs), np.stack(counts), clamped


@functools.lru_cache(maxsize=None)
def equirect_case(name):
    """-> (cams, images, resolutions, (W, H), depths, black_bg)"""
    rig, sizes, res, wh, (num, lo, hi), black, hole, centre = EQUIRECT_CASES[name]
    cams = _rig(rig)
    if centre is not None:
        cams = R.rig_center(cams, centre)
    return cams, _images(sizes, hole, 12), res or _same(sizes), wh, R.equirect_depths(num, lo, hi)[0], black


@functools.lru_cache(maxsize=None)
def equirect_rigged(name):
    cams, images, res = equirect_case(name)[:3]
    return R.Rigged(cams, images, res)


@functools.lru_cache(maxsize=None)
def equirect_ref(name):
    """-> (f32 [n, H, W, 4], count [n, H, W], whether the clamp of the truncating fetch mattered)"""
    _, _, _, (W, H), depths, black = equirect_case(name)
    outs, counts, mattered = [], [], False
    for d in depths:
        stats = {}
        outs.append(equirect_rigged(name).equirect(W, H, d, black_bg=black, stats=stats))
        counts.append(stats["count"])
        mattered |= stats["clamp_mattered"]
    return np.stack(outs), np.stack(counts), mattered
