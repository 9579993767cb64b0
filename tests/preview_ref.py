"""The tuning previews restated in plain numpy: TrackVar::update of ViewColorVarianceThresholds.cpp:69-81
and of ViewForegroundMaskThresholds.cpp:71-81, the constructors' scale (:92-97 / :96-100) and the executables'
thresholds.json, and GenerateKeypointProjections (below). The resize, the variance and the mask come from the oracle (cv_resize_area, cv_variance,
generate_foreground_mask); everything else is float32 arithmetic in the reference's order."""
import numpy as np

from oracle import oracle_lib

F32 = np.float32
K_MIN_VAR = F32(1.0) / F32(12.0) / F32(65025.0)  # DerpUtil.h:32
BLUE = np.array([65535, 0, 0], np.uint16)  # B, G, R
PURPLE = np.array([65535, 0, 65535], np.uint16)


def variance_levels(var_low_max, var_high_max, lo, hi, scale=1.0):
    """(varNoiseFloor, varHighThresh, varLowShow, varHighShow): float x int -> float, / int -> float (:70-73)"""
    scale_var = F32(float(scale) * float(scale))
    noise_floor = F32(F32(var_low_max) * F32(lo)) / F32(100)
    high_thresh = F32(F32(var_high_max) * F32(hi)) / F32(100)
    low_show = max(F32(noise_floor * scale_var), K_MIN_VAR)
    high_show = max(high_thresh, low_show)
    return np.array([noise_floor, high_thresh, low_show, high_show], F32)


def scale_of(width, cols):
    return float(width) / cols if width > 0 else 1.0


def scaled(bgr, width):
    """scaleImage(image, width / cols) with INTER_AREA (CvUtil.h:140-154); the image itself at its own size"""
    h, w = bgr.shape[:2]
    s = scale_of(width, w)
    dw, dh = int(np.floor(w * s + 0.5)), int(np.floor(h * s + 0.5))
    return bgr if (dw, dh) == (w, h) else oracle_lib.cv_resize_area(bgr, dw, dh)


def variance_marks(bgr, low_show, high_show, var=None):
    """-> images [n][h][w][3], counts [n][2] (blue, purple): strict comparisons, purple after blue"""
    var = oracle_lib.cv_variance(bgr) if var is None else var
    images, counts = [], []
    for lo, hi in zip(np.asarray(low_show, F32), np.asarray(high_show, F32)):
        out = bgr.copy()
        blue, purple = var < lo, var > hi
        out[blue] = BLUE
        out[purple] = PURPLE
        images.append(out)
        counts.append((int(np.count_nonzero(blue & ~purple)), int(np.count_nonzero(purple))))
    return np.stack(images), np.array(counts, np.uint32)


def foreground_threshold(slider):
    return F32(F32(1.0) * F32(slider)) / F32(100)  # threshMax * sliderThreshVal / sliderThreshMaxCount (:72)


def overlay(frame, mask):
    """addWeighted(frame, 1.0, green where the mask is set, 0.5, 0) on u16: fp32, rounded half to even, saturated"""
    out = frame.copy()
    g = np.rint(frame[..., 1].astype(F32) * F32(1.0) + F32(65535.0) * F32(0.5))
    out[..., 1] = np.where(mask != 0, np.minimum(g, F32(65535.0)).astype(np.uint16), frame[..., 1])
    return out


def foreground(template, frame, blurs, sliders, closings):
    """-> overlays, masks, counts of every triple, blur-major"""
    overlays, masks, counts = [], [], []
    for b in blurs:
        for s in sliders:
            for c in closings:
                m = oracle_lib.generate_foreground_mask(template, frame, int(b), float(foreground_threshold(s)), int(c))
                m = (np.asarray(m) != 0).astype(np.uint8)
                masks.append(m)
                overlays.append(overlay(frame, m))
                counts.append(int(np.count_nonzero(m)))
    return np.stack(overlays), np.stack(masks), np.array(counts, np.uint32)


def c_exp3(x):
    """printf("%.3e") of a float, which is what fmt's {:.3e} prints"""
    return "%.3e" % float(F32(x))


def variance_json(lows, highs, var_low_max, var_high_max, scale, counts, w, h):
    images = []
    for a, lo in enumerate(lows):
        for b, hi in enumerate(highs):
            lv = variance_levels(var_low_max, var_high_max, lo, hi, scale)
            k = a * len(highs) + b
            images.append({"file": "low_%03d_high_%03d.png" % (lo, hi), "low_slider": lo, "high_slider": hi,
                           "var_noise_floor": "--var_noise_floor=" + c_exp3(lv[0]),
                           "var_high_thresh": "--var_high_thresh=" + c_exp3(lv[1]), "blue": int(counts[k][0]),
                           "purple": int(counts[k][1]), "width": w, "height": h})
    return {"images": images}


def foreground_json(blurs, sliders, closings, counts, w, h):
    images, k = [], 0
    for b in blurs:
        for s in sliders:
            for c in closings:
                pct = F32(F32(100.0) * F32(int(counts[k]))) / F32(w * h)  # BackgroundSubtractionUtil.h:56-57
                images.append({"file": "blur_%02d_thresh_%03d_close_%02d.png" % (b, s, c),
                               "blur_radius": "--blur_radius=%d" % b, "threshold_slider": s,
                               "threshold": "--threshold=" + c_exp3(foreground_threshold(s)),
                               "morph_closing_size": "--morph_closing_size=%d" % c, "count": int(counts[k]),
                               "percent": "%.9g" % float(pct), "width": w, "height": h})
                k += 1
    return {"images": images}


# ---------------------------------------------------------------- GenerateKeypointProjections
# source/render/GenerateKeypointProjections.cpp:57-104 on the oracle's camera (oracle_lib.Rig: rig, pixel, sees,
# is_outside_image_circle); the depth sampler is FeatureMatcher.cpp:116-133 and :186-207.
KP_DEFAULTS = dict(length_stride=0.125, height_stride=0.125, depth_min=1.0, depth_max=100.0, depth_samples=1000.0,
                   search_overlap=0.25, search_radius=100)


def stride_values(stride):
    """for (f = 0; f <= 1; f += stride): the accumulated doubles, not a count"""
    out, f = [], 0.0
    while f <= 1:
        out.append(f)
        f += stride
    return out


def too_much_overlap(a, b, search_overlap):
    """(box & lastBox).area() > search_overlap * box.area() on cv::Rect2f (x, y, width, height as float32)"""
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    w = F32(min(F32(a[0] + a[2]), F32(b[0] + b[2])) - x1)
    h = F32(min(F32(a[1] + a[3]), F32(b[1] + b[3])) - y1)
    if w <= 0 or h <= 0:
        w = h = F32(0)
    return float(F32(w * h)) > search_overlap * float(F32(a[2] * a[3]))


def keypoint_samples(rig, c_point, c_into, px, py, **params):
    """getNextDepthSample until it answers false -> [(index, disparity, box float32 [4], world f64 [3])]"""
    p = dict(KP_DEFAULTS, **params)
    count = int(np.ceil(p["depth_samples"]))  # next < depth_samples, a double
    alpha = np.arange(count, dtype=np.float64) / (p["depth_samples"] - 1.0)
    disp = (1 / p["depth_max"]) * (1.0 - alpha) + (1 / p["depth_min"]) * alpha
    world = rig.rig(c_point, np.tile([[px, py]], (count, 1)), 1 / disp)
    pix = rig.pixel(c_into, world)
    r = int(p["search_radius"])
    boxes = np.stack([(pix[:, 0] - r).astype(F32), (pix[:, 1] - r).astype(F32), np.full(count, 2 * r, F32),
                      np.full(count, 2 * r, F32)], axis=1)
    out, last = [], np.zeros(4, F32)
    for i in range(count):
        if not too_much_overlap(boxes[i], last, p["search_overlap"]):
            out.append((i, float(disp[i]), boxes[i], world[i]))
            last = boxes[i]
    return out


def cv_round(v):
    return np.rint(np.asarray(v, dtype=np.float64)).astype(np.int64)  # half to even


def keypoint_rects(rig, c0, c1, width, height, w, h, **params):
    """the rectangles in drawing order: [(x0, y0, x1, y1 clipped and inclusive, colour f32 [4], grid point index)], and
    statistics of what the walk met"""
    p = dict(KP_DEFAULTS, **params)
    r = int(p["search_radius"])
    rects, point = [], 0
    stats = dict(skipped_circle=0, unseen=0, outside=0, samples=[])
    for wf in stride_values(p["length_stride"]):
        for hf in stride_values(p["height_stride"]):
            px, py = width * wf, height * hf
            if rig.is_outside_image_circle(c1, px + 0.5, py + 0.5):
                stats["skipped_circle"] += 1
                continue
            samples = keypoint_samples(rig, c1, c0, px, py, **params)
            stats["samples"].append(((px, py), samples))
            colour = np.array([hf, wf, 1 - hf, 1], np.float64).astype(F32)
            if samples:
                seen, pix = rig.sees(c0, np.array([s[3] for s in samples]))
                for ok, q in zip(seen, pix):
                    if not ok:
                        stats["unseen"] += 1
                        continue
                    x0, y0 = int(cv_round(q[0] - 0.5 - r)), int(cv_round(q[1] - 0.5 - r))
                    x1, y1 = int(cv_round(q[0] - 0.5 + r)), int(cv_round(q[1] - 0.5 + r))
                    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
                    stats["outside"] += int(x1 < x0 or y1 < y0)
                    rects.append((x0, y0, x1, y1, colour, point))
            point += 1
    return rects, stats


def keypoint_blend(image, rects):
    """-> (blend f32 [h][w][4], u8 [h][w][4], pixels covered by rectangles of two or more grid points)"""
    h, w = image.shape[:2]
    kp = np.zeros((h, w, 4), F32)
    owners = [[set() for _ in range(w)] for _ in range(h)] if w * h <= 64 * 64 else None
    for x0, y0, x1, y1, colour, point in rects:
        if x1 < x0 or y1 < y0:
            continue
        kp[y0:y1 + 1, x0:x1 + 1] = colour
        if owners is not None:
            for y in range(y0, y1 + 1):
                for x in range(x0, x1 + 1):
                    owners[y][x].add(point)
    blend = np.asarray(image, F32) * F32(1.0) + kp * F32(0.6) + F32(0.0)
    assert blend.dtype == F32
    from tests import sweep_ref

    shared = sum(len(o) > 1 for row in owners for o in row) if owners is not None else -1
    return blend, sweep_ref.to_u8(blend), shared
