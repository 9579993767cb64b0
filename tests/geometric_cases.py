"""The rigs, frames and clean-depth maps that tests/test_gpu_geometric_consistency*.py share, with the restatement's
results (tests/geometric_ref.py) computed once per case. Nothing here touches the GPU."""
import functools

import numpy as np

from tests import geometric_ref as G

FULL = 64  # every camera's full resolution


def _camera(index, origin, forward):
    """a 64^2 FTHETA camera with a field of +-40 degrees (focal = resolution) looking along `forward`"""
    from facebook360_dep_amd import synth

    f, up, right = synth._frame(np.array(forward, dtype=np.float64))
    return {"version": 1, "type": "FTHETA", "id": "cam%d" % index, "origin": list(origin), "forward": f.tolist(),
            "up": up.tolist(), "right": right.tolist(), "resolution": [FULL, FULL], "focal": [1.0 * FULL, -1.0 * FULL],
            "principal": [FULL / 2.0, FULL / 2.0], "fov": np.pi / 2}


def isolated_rig():
    """two cameras side by side looking along +x, and one behind them looking along -x: every point of its rays has
    x < -0.25 and lies behind the two (their cone is the half space in front), so no camera overlaps it"""
    return [_camera(0, (0.25, 0.06, 0.0), (1, 0, 0)), _camera(1, (0.25, -0.06, 0.0), (1, 0, 0)),
            _camera(2, (-0.25, 0.0, 0.0), (-1, 0, 0))]


# name -> (cameras, small (w, h) per camera, disparity_step, slices of camera 0)
def case(name):
    from facebook360_dep_amd import synth

    rig4 = synth.make_rig(4, FULL)["cameras"]
    return {
        "rig4_32": (rig4, [(32, 32)] * 4, 0.0787, 37),  # 3 x 3 tiles of 14, 37 slices: no multiple of any split but 1 and 37
        "rig4_25x19": (rig4, [(25, 19)] * 4, 0.3, 7),   # no multiple of the tile: the halo crosses all four edges
        "rig4_3x3": (rig4, [(3, 3)] * 4, 0.3, 1),       # one interior pixel, every halo sample a mirror; one slice
        "rig4_mixed": (rig4, [(32, 32), (25, 19), (32, 19), (16, 16)], 0.25, 12),  # per-camera sizes and slice counts
        "rig2": (synth.make_rig(2, FULL)["cameras"], [(32, 32)] * 2, 0.25, 12),  # one source
        "rig5": (synth.make_rig(5, FULL)["cameras"], [(25, 19)] * 5, 0.25, 8),
        "isolated": (isolated_rig(), [(32, 32)] * 3, 0.5, 16),
    }[name]


CASES = ["rig4_32", "rig4_25x19", "rig4_3x3", "rig4_mixed", "rig2", "rig5", "isolated"]


@functools.lru_cache(maxsize=None)
def images(name):
    """full-size BGRA u16 per camera; camera 1 of the mixed rig has a transparent hole"""
    from facebook360_dep_amd import synth

    cams = case(name)[0]
    out = [G.with_alpha(synth.render_camera(c, FULL, FULL)[0]) for c in cams]
    if name == "rig4_mixed":
        out[1] = out[1].copy()
        out[1][20:34, 24:44, 3] = 0
    return out


@functools.lru_cache(maxsize=None)
def frame(name):
    cams, sizes, _, _ = case(name)
    return G.Frame(cams, images(name), sizes)


@functools.lru_cache(maxsize=None)
def truth_depths(name):
    """the synthetic scene's true depth along each small camera's rays, f32 [h, w] per camera"""
    from facebook360_dep_amd import synth

    cams, sizes, _, _ = case(name)
    with np.errstate(divide="ignore"):
        return [(1.0 / synth.render_camera(c, w, h)[1].astype(np.float64)).astype(np.float32)
                for c, (w, h) in zip(cams, sizes)]


@functools.lru_cache(maxsize=None)
def occluding_clean(name, patch=True):
    """clean-depth maps for the occlusion test: the true depths with NaN holes and, with `patch`, a patch of very small
    depths in every camera (5 cm: nearer than any hypothesis, so whatever lands there counts as occluded)"""
    out = []
    for i, d in enumerate(truth_depths(name)):
        d = d.copy()
        h, w = d.shape
        d[h // 5:h // 5 + max(h // 6, 1), w // 6:w // 6 + max(w // 4, 1)] = np.nan
        d[(i * 7) % h, :] = np.nan
        if patch:
            d[h // 2:h // 2 + max(h // 4, 1), w // 3:w // 3 + max(w // 3, 1)] = 0.05
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def ref_sweep(name, dst, clean=None, agree=0.75):
    """clean: None, "holes" or "patch" (occluding_clean)"""
    maps = None if clean is None else occluding_clean(name, clean == "patch")
    return frame(name).sweep(dst, case(name)[2], maps, agree)


@functools.lru_cache(maxsize=None)
def ref_run(name, agree=0.75, pass_count=2, keep_clean=False):
    return frame(name).run(case(name)[2], agree, pass_count, keep_clean)


def same(a, b):
    """bit for bit, NaN masks included"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True))
    return bool(np.array_equal(a, b))


def differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())
    return int((a != b).sum())
