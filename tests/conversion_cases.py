"""The rigs, sizes and inputs that tests/test_conversion_ref.py (CPU, on the references alone) and
tests/test_gpu_conversion_limits.py (the kernels against those references) share, so that what the first states about
the inputs holds for the second. Nothing here touches the GPU."""
import functools
import math

import numpy as np

from tests import common
from tests import conversion_ref as ref

F32 = np.float32
MIN_DEPTH, MAX_DEPTH = 0.5, 6.0  # of the import

MIXED_RES = 40  # the mixed rig's sensor: 40 x 40


@functools.lru_cache(maxsize=None)
def rig(name):
    """-> (cameras under test, the same cameras with a principal point each: what the input renderer needs)"""
    if name == "mixed":
        cams = common.mixed_type_rig(MIXED_RES)["cameras"]
        return cams, cams
    full = common.real_rig()["cameras"]
    return {"real": full, "real_nopr": common.real_rig_no_principal()["cameras"]}[name], full


NO_PRINCIPAL = (1, 4)  # the cameras real_nopr differs from real in: the only ones its cases run
SIZES = {"mixed": [(40, 40), (50, 38)], "real": [(84, 54), (50, 38)], "real_nopr": [(84, 54), (50, 38)]}


def cameras_of(name):
    return NO_PRINCIPAL if name == "real_nopr" else range(6)


# ---------------------------------------------------------------- export
EXPORT_SETTINGS = [(math.inf, False), (math.inf, True), (3.0, False), (3.0, True)]  # (max_depth, clip)
EXPORT_CASES = [(name, size) for name in ("mixed", "real", "real_nopr") for size in SIZES[name]]

# isOutsideImageCircle pixels per camera, from the reference's camera on the CPU (test_conversion_ref pins them). The
# mixed rig's cameras 4 and 5 have the default FOV, which has no image circle: their compaction work comes from clip
# (or subsample) alone.
OUTSIDE = {
    ("mixed", (40, 40)): [556, 320, 524, 408, 0, 0],
    ("mixed", (50, 38)): [656, 388, 612, 484, 0, 0],
    ("real", (84, 54)): [690, 708, 697, 708, 706, 686],
    ("real", (50, 38)): [290, 294, 292, 298, 296, 288],
    ("real_nopr", (84, 54)): [708, 708],  # cameras 1 and 4
    ("real_nopr", (50, 38)): [296, 296],
}
SCAN_OUTSIDE = {(256, 1024): 53692, (256, 1025): 53744, (256, 2049): 107460, (1025, 256): 53744}


@functools.lru_cache(maxsize=None)
def export_inputs(name, size, cam):
    w, h = size
    disp, color = ref.export_inputs(rig(name)[1][cam], w, h)
    disp.setflags(write=False)
    color.setflags(write=False)
    return disp, color


def compacts(outside, max_depth, clip):
    """whether an export case is meant to drop pixels: an image circle, or clipping at 3 m in a scene of 1.5 - 4 m"""
    return outside > 0 or (clip and max_depth == 3.0)


# block scan: k_scan_block_counts sums `per` = ceil(blocks / 1024) block counts per thread. The images are 256 wide, one
# block per row: the last block is then the last row, whose middle lies inside the image circle (in a 1025 x 256 image
# it is the end of the last row, a corner, where no camera with an image circle keeps a pixel).
SCAN_CAM = 1  # the mixed rig's FTHETA camera with an image circle
SCAN_SIZES = [(256, 1024), (256, 1025), (256, 2049)]  # 1024 blocks (per 1, full), 1025 (per 2, ragged), 2049 (per 3)
SCAN_WIDE = (1025, 256)  # 1025 blocks again, none of which is a row
TINY_SIZES = [(1, 1), (255, 1), (256, 1), (257, 1), (1, 257)]
TINY_CAMS = (1, 4)


@functools.lru_cache(maxsize=None)
def striped_inputs(size, seed=17):
    """2 m everywhere but 10 m (beyond max_depth = 3) in every other band of eight rows, which is blocks of 256 pixels
    with nothing kept under clip, and in five columns of every 97 in every other band of 64 rows, which is blocks with
    a few dropped beside blocks that keep all 256; random colour"""
    w, h = size
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    far = ((ys // 8) % 2 == 1) | ((xs % 97 < 5) & ((ys // 64) % 2 == 1))
    disp = np.where(far, F32(0.1), F32(0.5)).astype(F32)
    color = rng.random((h, w, 3), dtype=F32)
    disp.setflags(write=False)
    color.setflags(write=False)
    return disp, color


# ---------------------------------------------------------------- import
IMPORT_SIZES = [(50, 38), (32, 32), (84, 54), (1, 1), (40, 40), (56, 36)]
IMPORT_RIGS = ("mixed", "real", "real_nopr")
# (camera, axis) pairs of clamp_cloud whose edge no point can be seen at, because the camera's image circle ends
# before that edge (the reference's `sees` says so of every point built there; test_conversion_ref pins the list). The
# mixed rig's cameras 0, 2 and 3 have a circle inside the square image: 0 and 2 in both axes, 3 is the 1 x 1 image,
# whose edge is no edge of the sensor. The real rig's circle (radius 1.40 focal lengths) ends before the left and right
# edges (1.51) and beyond the top and bottom ones (0.97).
_REAL_X = {(0, 0), (1, 0), (2, 0), (4, 0), (5, 0)}
UNREACHABLE = {"mixed": {(0, 0), (0, 1), (2, 0), (2, 1)}, "real": _REAL_X, "real_nopr": _REAL_X}


@functools.lru_cache(maxsize=None)
def import_clouds(name):
    """-> {cloud name: f64 [n, 3]}: `dense` is the random cloud with the built points in its middle, `sparse` the built
    points alone, where no random point hides them behind a nearer one"""
    cams = rig(name)[0]
    built = np.concatenate([ref.clamp_cloud(cams, IMPORT_SIZES)[0], ref.boundary_cloud(cams, MIN_DEPTH, MAX_DEPTH)[0],
                            ref.special_rows()])
    rnd = ref.random_cloud(20000, seed=11)
    clouds = {"dense": np.concatenate([rnd[:9000], built, rnd[9000:]]), "sparse": built}
    for c in clouds.values():
        c.setflags(write=False)
    return clouds


@functools.lru_cache(maxsize=None)
def import_reference(name, cloud):
    return ref.import_points(rig(name)[0], import_clouds(name)[cloud], IMPORT_SIZES, MIN_DEPTH, MAX_DEPTH)


def three_ways(pts):
    """whole, as [256, 0, 512, rest] and permuted with a fixed seed"""
    perm = np.random.default_rng(5).permutation(len(pts))
    return {"whole": [pts], "chunks": [pts[:256], pts[256:256], pts[256:768], pts[768:]], "permuted": [pts[perm]]}


# ---------------------------------------------------------------- equirect mask
EQUIRECT_SIZES = [(64, 32), (37, 19)]
EQUIRECT_TARGETS = [(50, 38), (84, 54)]
EQUIRECT_DEPTHS = [1000.0, 1.0]
BAND_CAP = 0.01  # test_equirect_mask's: pixels within 2e-4 px of an equirect pixel border, at most 1 % of an image


@functools.lru_cache(maxsize=None)
def equirect(size):
    m = ref.blob_mask(size[0], size[1], seed=5)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def equirect_reference(name, cam, eqr_size, size, depth):
    return ref.project_equirect_mask(rig(name)[0], cam, equirect(eqr_size), size[0], size[1], depth)
