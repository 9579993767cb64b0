"""The images the tuning previews are tested on, and what each must contain (tests/test_preview_ref.py checks the
contents with the oracle, so that a case cannot quietly stop exercising what it is named for)."""
import numpy as np

VAR_W, VAR_H = 37, 23
FLAT = (slice(2, 10), slice(3, 14))      # rows, columns of the flat patch: variance 0 away from its rim
CHECKER = (slice(12, 22), slice(20, 36))  # the 0 / 65535 checker: the largest variances
VAR_LOW_MAX, VAR_HIGH_MAX = 4e-3, 5e-2    # the reference's defaults


def variance_image(w=VAR_W, h=VAR_H, seed=11):
    """gentle noise everywhere, a flat patch, a hard checker (B, G, R uint16)"""
    rng = np.random.default_rng(seed)
    img = (30000 + rng.integers(-3000, 3000, (h, w, 3))).astype(np.uint16)
    if w >= VAR_W and h >= VAR_H:
        img[FLAT] = 12345
        yy, xx = np.mgrid[CHECKER[0], CHECKER[1]]
        img[CHECKER] = (((yy + xx) & 1) * 65535).astype(np.uint16)[..., None]
    return img


def variance_fullsize(w, h, seed=5):
    """a full-size image for the executable: blocks of 2 x 2 texels with noise on top, the flat patch and checker kept
    at twice the size so that the scaled image holds all three kinds of region"""
    small = variance_image(VAR_W, VAR_H, seed)
    big = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)
    big = np.concatenate([big, big[:, -1:]], axis=1)[:h, :w]  # 75 columns: the last one repeated
    rng = np.random.default_rng(seed + 1)
    noisy = np.clip(big.astype(np.int64) + rng.integers(-40, 41, big.shape), 0, 65535).astype(np.uint16)
    flat = big == 12345
    noisy[flat] = 12345
    return np.ascontiguousarray(noisy)


def equal_thresholds(var):
    """two variances present in the image: the median of the positive ones (as the low threshold) and the second
    largest distinct value (as the high one), so that pixels sit exactly on both and others beyond both"""
    positive = np.unique(var[var > 0])
    return np.float32(positive[len(positive) // 2]), np.float32(positive[-2])


FG_W, FG_H = 40, 30
BLOB = (slice(6, 24), slice(8, 30))
SMALL_HOLE = (12, 14)                       # one texel inside the blob: a closing of 4 fills it
BIG_HOLE = (slice(14, 22), slice(18, 27))   # 8 x 9 texels inside the blob: a closing of 7 does not fill its middle
BIG_HOLE_CENTRE = (18, 22)
G_PROBES = {(8, 10): 0, (8, 12): 1, (8, 14): 32767, (8, 16): 32768, (8, 18): 65535}  # (row, col) -> frame G


def foreground_pair():
    """template and frame (B, G, R uint16): the frame holds a blob the template lacks, with two holes in it, and green
    values on the blob that hit the overlay's tie (odd and even), its zero and its saturation"""
    rng = np.random.default_rng(3)
    template = (30000 + rng.integers(-200, 200, (FG_H, FG_W, 3))).astype(np.uint16)
    frame = template.copy()
    frame[BLOB] = template[BLOB] + np.array([20000, 9000, 25000], np.uint16)
    frame[SMALL_HOLE] = template[SMALL_HOLE]
    frame[BIG_HOLE] = template[BIG_HOLE]
    for (y, x), g in G_PROBES.items():
        frame[y, x, 1] = g
    frame[28, 2] = template[28, 2] + np.array([0, 2700, 0], np.uint16)  # ~0.041 of the range: beside the default threshold
    return template, frame


FG_BLURS, FG_SLIDERS, FG_CLOSINGS = (0, 1, 3), (0, 4, 100), (0, 1, 4, 7)


# ---------------------------------------------------------------- GenerateKeypointProjections
KP_W, KP_H = 64, 48


def keypoint_rig(fov=None, turn=None, enlarge=None):
    """synth.make_rig(3, ...) at 64 x 48; fov narrows every camera's image circle; turn = (camera, degrees) turns one
    camera about its up axis, so that it no longer sees some of its neighbours' points; enlarge = (camera, factor)
    multiplies a camera's resolution and principal point (its images stay 64 x 48, the first camera's resolution, as the
    reference requires of them): it then sees points beyond the image, whose rectangles are clipped to nothing"""
    import math

    from facebook360_dep_amd import synth

    cams = synth.make_rig(3, KP_W)["cameras"]
    for cam in cams:
        cam["resolution"] = [KP_W, KP_H]
        cam["principal"] = [KP_W / 2.0, KP_H / 2.0]
        if fov is not None:
            cam["fov"] = fov
    if turn is not None:
        index, degrees = turn
        cam = cams[index]
        a = math.radians(degrees)
        f, r = np.array(cam["forward"]), np.array(cam["right"])
        cam["forward"] = (math.cos(a) * f + math.sin(a) * r).tolist()
        cam["right"] = (math.cos(a) * r - math.sin(a) * f).tolist()
    if enlarge is not None:
        index, factor = enlarge
        cams[index]["resolution"] = [KP_W * factor, KP_H * factor]
        cams[index]["principal"] = [KP_W * factor / 2.0, KP_H * factor / 2.0]
    return cams


def keypoint_resolutions(cams):
    return [tuple(cam["resolution"]) for cam in cams]


def keypoint_images(seed=9):
    """float BGRA images in [0, 1] with values beyond it here and there, so that the file's saturation is met"""
    rng = np.random.default_rng(seed)
    images = []
    for _ in range(3):
        im = rng.random((KP_H, KP_W, 4)).astype(np.float32)
        im[::7, ::5, :3] = 0.9  # + 0.6 of a colour: beyond 1, saturated in the file
        im[..., 3] = 1.0
        images.append(im)
    return images


KP_BASE = dict(length_stride=0.25, height_stride=0.25, depth_min=1.0, depth_max=100.0, depth_samples=50.0,
               search_overlap=0.25, search_radius=3)
# name -> (rig arguments, parameters): what each must contain is checked in tests/test_preview_ref.py
KP_CASES = {
    "base": ({}, KP_BASE),
    "radius0": ({}, dict(KP_BASE, search_radius=0, depth_samples=1000.0)),
    "unseen": (dict(turn=(0, 35.0)), KP_BASE),
    "circle": (dict(fov=1.0), KP_BASE),
    "overwrite": ({}, dict(KP_BASE, search_radius=9)),
    "outside": (dict(enlarge=(1, 2)), KP_BASE),
}
