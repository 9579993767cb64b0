"""numpy restatement of GeometricConsistency as DESIGN §8.6 defines it (source/render/GeometricConsistency.cpp with the
OpenGL reprojection replaced by a defined sampling rule), on the oracle's camera (oracle_lib.Rig: rescale, rig, sees) and
oracle_lib.cv_resize_area. Vectorised over pixels. Nothing here touches the GPU."""
import numpy as np

from tests.conversion_ref import norm3, pixel_centres, rescaled_rig

F32, F64, I16 = np.float32, np.float64, np.int16
SIGNED_MAX = 32767
MIN_DISPARITY = F32(1.0 / 1e4)  # 1.0f / Camera::kNearInfinity
MAX_DISPARITY = F32(1.0)


def small_sizes(cams, downscale):
    """downscale() (:324-331): round(resolution / downscale), halves away from zero"""
    return [tuple(int(np.floor(r / downscale + 0.5)) for r in cam["resolution"]) for cam in cams]


def with_alpha(bgr):
    """alpha 65535 where the file has none"""
    bgr = np.asarray(bgr, dtype=np.uint16)
    if bgr.shape[2] == 4:
        return bgr
    return np.concatenate([bgr, np.full(bgr.shape[:2] + (1,), 65535, np.uint16)], axis=2)


def saturate16(v):
    return np.clip(v, -32768, 32767).astype(I16)


def prepare(bgra, w, h):
    """computeReference (:158-163): INTER_AREA to (w, h) on four channels, then convertTo(CV_16S, 32767 / 65535.0)"""
    from oracle import oracle_lib as O

    bgra = with_alpha(bgra)
    bgr = O.cv_resize_area(np.ascontiguousarray(bgra[:, :, :3]), w, h)
    # (cv::resize treats channels alike: alpha goes through the three-channel routine on its own)
    alpha = O.cv_resize_area(np.ascontiguousarray(np.repeat(bgra[:, :, 3:], 3, axis=2)), w, h)[:, :, :1]
    small = np.concatenate([bgr, alpha], axis=2).astype(F64)
    return saturate16(np.rint(small * (32767.0 / 65535.0)))


def rig_radius(rig):
    """computeRigRadius (:97-103)"""
    total = 0.0
    for i in range(rig.n):
        total += float(norm3(rig.state(i)["position"][None])[0])
    return total / rig.n


def slice_count(rig, dst, disparity_step):
    radius = rig_radius(rig)
    assert radius < 1.0
    f = rig.state(dst)["focal"]
    focal = np.sqrt(f[0] * f[0] + f[1] * f[1]) * np.sqrt(0.5)
    v = focal * np.arcsin(radius) / disparity_step
    return int(np.floor(abs(v) + 0.5) * np.sign(v))  # std::round


def slice_disparities(count):
    """sliceDisparity (:126-128) through unnormalizeDisparity (ReprojectionTable.h:161-165): fp32"""
    n = ((np.arange(count, dtype=F64) + 0.5) / count).astype(F32)
    return (F32(1) - n) * MIN_DISPARITY + n * MAX_DISPARITY


def sq(a):
    """diff.mul(diff, 1.0 / kSignedMax) as §8.6 defines it: fp64, round half to even, saturate"""
    a = np.asarray(a).astype(F64)
    return saturate16(np.rint(a * a * (1.0 / SIGNED_MAX)))


def blur3(img):
    """cv::blur 3 x 3 on CV_16S as §8.6 defines it: BORDER_REFLECT_101, int32 sum, * (1.0 / 9) in fp64, round half to even"""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    if squeeze:
        img = img[:, :, None]
    h, w = img.shape[:2]
    p = np.pad(img.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    total = np.zeros(img.shape, np.int32)
    for j in range(3):
        for i in range(3):
            total += p[j:j + h, i:i + w]
    out = saturate16(np.rint(total.astype(F64) * (1.0 / 9)))
    return out[:, :, 0] if squeeze else out


class Frame:
    """the rescaled rig, the int16 images and the destination rays of one frame"""

    def __init__(self, cams, images, sizes):
        self.cams, self.sizes = cams, [tuple(s) for s in sizes]
        self.rig = rescaled_rig(cams, self.sizes)
        self.n = len(cams)
        self.I16 = [prepare(images[i], *self.sizes[i]) for i in range(self.n)]
        self.pos = [self.rig.state(i)["position"].copy() for i in range(self.n)]

    def world(self, dst, depth):
        w, h = self.sizes[dst]
        return self.rig.rig(dst, pixel_centres(w, h), depth)

    def sample(self, dst, src, disparity, clean=None, agree=0.75):
        """the int16 sample image of source `src` at slice disparity `disparity` -> [h, w, 4]"""
        w, h = self.sizes[dst]
        sw, sh = self.sizes[src]
        world = self.world(dst, 1.0 / float(disparity))
        seen, p = self.rig.sees(src, world)
        seen &= ~np.isnan(p).any(axis=1)
        p = p[seen]
        u, v = p[:, 0] - 0.5, p[:, 1] - 0.5
        x0, y0 = np.floor(u), np.floor(v)
        fx, fy = (u - x0).astype(F32)[:, None], (v - y0).astype(F32)[:, None]
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        padded = np.zeros((sh + 2, sw + 2, 4), F32)  # texels outside the image: (0, 0, 0, 0)
        padded[1:-1, 1:-1] = self.I16[src]
        t00, t10 = padded[y0 + 1, x0 + 1], padded[y0 + 1, x0 + 2]
        t01, t11 = padded[y0 + 2, x0 + 1], padded[y0 + 2, x0 + 2]
        ax, ay = F32(1) - fx, F32(1) - fy
        top = ax * t00 + fx * t10
        bottom = ax * t01 + fx * t11
        value = saturate16(np.rint(ay * top + fy * bottom))
        assert top.dtype == F32 and value.dtype == I16
        if clean is not None:
            d = clean[src][p[:, 1].astype(np.int64), p[:, 0].astype(np.int64)]
            distance = norm3(world[seen] - self.pos[src])
            with np.errstate(invalid="ignore"):
                occluded = ~np.isnan(d) & (d.astype(F64) < distance * agree)
            value[occluded, 3] = 0
        out = np.zeros((h * w, 4), I16)
        out[seen] = value
        return out.reshape(h, w, 4)

    def source_terms(self, dst, src, disparity, clean=None, agree=0.75):
        """-> (sample, average, averageOfSq, contributes [h, w] bool, term [h, w] f32)"""
        image = self.sample(dst, src, disparity, clean, agree)
        diff = saturate16(image.astype(np.int32) - self.I16[dst].astype(np.int32))
        average = blur3(diff)
        average_of_sq = blur3(sq(diff))
        contributes = (image[:, :, 3] == SIGNED_MAX) & (average[:, :, 3] == 0)
        a = np.zeros(image.shape[:2], F32)
        b = np.zeros(image.shape[:2], F32)
        for c in range(3):  # sumNorm / sumSqNorm (:110-124): alpha excluded
            a = a + average_of_sq[:, :, c].astype(F32)
            f = average[:, :, c].astype(F32)
            b = b + f * f
        term = a / F32(SIGNED_MAX) - b / (F32(SIGNED_MAX) * F32(SIGNED_MAX))
        assert term.dtype == F32
        return image, average, average_of_sq, contributes, term

    def cost(self, dst, disparity, clean=None, agree=0.75):
        """the cost plane of one slice (:200-253)"""
        w, h = self.sizes[dst]
        accum0, accum1 = np.zeros((h, w), F32), np.zeros((h, w), F32)
        for s in range(self.n):
            if s == dst:
                continue
            _, _, _, contributes, term = self.source_terms(dst, s, disparity, clean, agree)
            accum0 = np.where(contributes, accum0 + term, accum0)
            accum1 = np.where(contributes, accum1 + F32(1), accum1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return accum0 / accum1

    def sweep(self, dst, disparity_step, clean=None, agree=0.75, return_slice=False):
        """computeDepth + winnerTakesAll (:132-258) -> depth f32 [h, w] (and the winning slice, -1 where none)"""
        w, h = self.sizes[dst]
        disparities = slice_disparities(slice_count(self.rig, dst, disparity_step))
        best = np.full((h, w), np.finfo(F32).max, F32)
        at = np.full((h, w), -1, np.int64)
        for k, d in enumerate(disparities):
            cost = self.cost(dst, d, clean, agree)
            with np.errstate(invalid="ignore"):
                wins = best > cost
            best = np.where(wins, cost, best)
            at[wins] = k
        depth = np.full((h, w), np.nan, F32)
        depth[at >= 0] = (1.0 / disparities[at[at >= 0]].astype(F64)).astype(F32)
        depth[0, :] = depth[-1, :] = np.nan
        depth[:, 0] = depth[:, -1] = np.nan
        return (depth, at) if return_slice else depth

    def run(self, disparity_step, agree=0.75, pass_count=2, keep_clean=False):
        """processFrame (:333-384) -> dict(iffy [cam], clean [pass][cam], depth [pass][cam], final [cam])"""
        depths = [self.sweep(d, disparity_step) for d in range(self.n)]
        out = {"iffy": [d.copy() for d in depths], "clean": [], "depth": []}
        for _ in range(pass_count):
            cleaned = clean_depths(self.rig, depths, agree)
            out["clean"].append(cleaned)
            depths = [self.sweep(d, disparity_step, cleaned, agree) for d in range(self.n)]
            out["depth"].append([d.copy() for d in depths])
            if keep_clean:  # restoreCleanDepth (:312-322)
                depths = [np.where(np.isnan(c), d, c) for d, c in zip(depths, cleaned)]
        out["final"] = depths
        return out


def clean_depths(rig, depths, agree=0.75):
    """cleanDepth / isPointBad (:260-310) of every camera; `rig` rescaled to the maps' sizes. A NaN depth stays NaN (the
    reference indexes the sources' maps with a NaN pixel there), a NaN source depth never rejects."""
    out = []
    for d in range(rig.n):
        h, w = depths[d].shape
        depth = depths[d].reshape(-1)
        valid = ~np.isnan(depth)
        world = rig.rig(d, pixel_centres(w, h)[valid], depth[valid].astype(F64))
        bad = np.zeros(len(world), bool)
        for s in range(rig.n):
            if s == d:
                continue
            seen, p = rig.sees(s, world)
            seen &= ~np.isnan(p).any(axis=1)
            src_depth = depths[s][p[seen, 1].astype(np.int64), p[seen, 0].astype(np.int64)]
            proposal = norm3(world[seen] - rig.state(s)["position"]).astype(F32)
            with np.errstate(invalid="ignore"):
                rejects = proposal.astype(F64) < src_depth.astype(F64) * agree
            bad[np.flatnonzero(seen)[rejects]] = True
        res = depth.copy()
        res[np.flatnonzero(valid)[bad]] = np.nan
        out.append(res.reshape(h, w))
    return out


def clean(cams, depths, agree=0.75):
    return clean_depths(rescaled_rig(cams, [(d.shape[1], d.shape[0]) for d in depths]), depths, agree)
