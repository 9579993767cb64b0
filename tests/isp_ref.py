"""CPU restatement of the reference's camera ISP (source/isp/CameraIsp.h, source/isp/Filter.h, source/util/MathUtil.h,
source/util/RawUtil.cpp), written from those sources: numpy float32, one operation at a time, and Python loops wherever
the reference's loop is sequential (the in-place demosaic, the stuck-pixel scan, the recursive low pass). It is what the
GPU stages are compared with, bit for bit.

Where the reference reads memory it never wrote (cv::Mat_ allocated without a fill), this restatement and the library
both read 0: the difference planes of demosaicChromaSuppressed at pixels of another colour, element cols - 1 of
iirLowPass's line buffer during the horizontal pass, and column 0 of lpImage before the vertical pass.

The composite colour matrix is a chain of 3 x 3 products whose rounding in the reference is cv::gemm's; here, as in the
library, every product accumulates in double and rounds to float once.

powf, tanf and expf are this machine's libm through ctypes (np.power / np.exp may take a SIMD path)."""
import ctypes
import ctypes.util
import math

import numpy as np

F = np.float32
LUT_SIZE = 4096  # kToneCurveLutSize, CameraIsp.h:40

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n in ("powf", "tanf", "expf"):
    getattr(_libm, _n).restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.tanf.argtypes = [ctypes.c_float]
_libm.expf.argtypes = [ctypes.c_float]


def powf(x, y):
    return F(_libm.powf(float(x), float(y)))


def tanf(x):
    return F(_libm.tanf(float(x)))


def expf(x):
    return F(_libm.expf(float(x)))


DEFAULTS = {  # CameraIsp::CameraIsp, CameraIsp.h:490-519
    "bitsPerPixel": 16, "width": 0, "height": 0, "isLittleEndian": False, "isRowMajor": True, "bayerPattern": "GBRG",
    "planeOrder": "", "compandingLut": [[0, 0, 0], [1, 1, 1]], "blackLevel": [0, 0, 0], "clampMin": [0, 0, 0],
    "clampMax": [1, 1, 1], "stuckPixelThreshold": 0, "stuckPixelDarknessThreshold": 0, "stuckPixelRadius": 0,
    "vignetteRollOffH": [[1, 1, 1]], "vignetteRollOffV": [[1, 1, 1]], "whiteBalanceGain": [1, 1, 1],
    "ccm": [[1, 0, 0], [0, 1, 0], [0, 0, 1]], "saturation": 1.0, "gamma": [1, 1, 1], "lowKeyBoost": [0, 0, 0],
    "highKeyBoost": [0, 0, 0], "contrast": 1.0, "sharpening": [0, 0, 0], "sharpeningSupport": float(F(10.0) / F(2048.0)),
    "noiseCore": 1000.0,
}


def reflect(x, r):  # MathUtil.h:42-44
    return -x if x < 0 else (2 * r - x - 1 if x >= r else x)


def clamp(x, a, b):  # MathUtil.h:37-39
    return a if x < a else (b if x > b else x)


def lerp(x0, x1, alpha):  # MathUtil.h:51-59: x0 * (1 - alpha) + x1 * alpha
    return x0 * (F(1) - alpha) + x1 * alpha


def bezier_curve(points, t):  # BezierCurve::operator(), MathUtil.h:122-128: recursive De Casteljau on Vec3f
    pts = [np.asarray(p, F) for p in points]

    def rec(i, j):
        return pts[i] if i == j else lerp(rec(i, j - 1), rec(i + 1, j), F(t))

    return rec(0, len(pts) - 1)


def bilerp_half(p00, p01, p10, p11):  # cv_util::bilerp(.., 0.5f, 0.5f), CvUtil.h:84-86
    q = F(0.5) * F(0.5)
    return q * p00 + q * p01 + q * p10 + q * p11


def _bezier4(a, b, c, d, t):  # CameraIsp.h:357-363
    return lerp(lerp(lerp(a, b, t), lerp(b, c, t), t), lerp(lerp(b, c, t), lerp(c, d, t), t), t)


def _high_key(boost, x):  # :365-371
    b = clamp(F(0.6666), F(0), F(1))
    c = clamp(F(0.8333) + boost, F(0), F(1))
    return _bezier4(F(0.5), b, c, F(1), (x - F(0.5)) * F(2)) if x > F(0.5) else F(0)


def _low_key(boost, x):  # :373-379
    b = clamp(F(0.1666) + boost, F(0), F(1))
    c = clamp(F(0.3333), F(0), F(1))
    return _bezier4(F(0), b, c, F(0.5), x * F(2)) if x <= F(0.5) else F(0)


def tone_curve_lut(cfg, enabled):  # buildToneCurveLut, CameraIsp.h:382-416
    lut = np.zeros((LUT_SIZE, 3), F)
    dx = F(1) / F(LUT_SIZE - 1)
    angle = F(math.pi * float(F(0.25)) * float(F(cfg["contrast"])))
    slope = tanf(angle)
    bias = F(0.5) * (F(1) - slope)
    for i in range(LUT_SIZE):
        x = dx * F(i)
        for c in range(3):
            y = x
            if enabled:
                y = powf(x, F(cfg["gamma"][c]))
                y = _low_key(F(cfg["lowKeyBoost"][c]), y) + _high_key(F(cfg["highKeyBoost"][c]), y)
                y = clamp(slope * y + bias, F(0), F(1))
            lut[i, c] = y
    return lut


def _mul3(a, b):  # double accumulation, one rounding per element
    out = np.zeros((3, 3), F)
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += float(a[i, k]) * float(b[k, j])
            out[i, j] = F(s)
    return out


def composite_ccm(cfg):  # setup(), CameraIsp.h:630-645; ColorspaceConversion.h:17-25
    rgb2yuv = np.array([[0.299, 0.587, 0.114], [-0.14713, -0.28886, 0.436], [0.615, -0.51499, -0.10001]], F)
    yuv2rgb = np.array([[1.0, 0.0, 1.13983], [1.0, -0.39465, -0.58060], [1.0, 2.03211, 0.0]], F)
    s = F(cfg["saturation"])
    sat = np.array([[1, 0, 0], [0, s, 0], [0, 0, s]], F)
    m = _mul3(_mul3(yuv2rgb, sat), rgb2yuv)
    out = _mul3(np.array(cfg["ccm"], F).T.copy(), m)
    return out * F(LUT_SIZE - 1)


class Isp:
    """CameraIsp with RawToRgb's options (RawUtil.cpp:42-57). run(raw_bytes) returns every stage and the image."""

    def __init__(self, config=None, demosaic_filter=0, pow2_downscale=1, apply_tone_curve=True):
        cfg = dict(DEFAULTS)
        cfg.update((config or {}).get("CameraIsp", config or {}))
        cfg["bayerPattern"] = cfg["bayerPattern"].upper()
        cfg["planeOrder"] = cfg["planeOrder"].upper()
        self.cfg = cfg
        self.filter, self.resize = demosaic_filter, pow2_downscale
        assert demosaic_filter in (0, 2, 3) and pow2_downscale in (1, 2, 4, 8)
        # setup() :573-618
        self.color = np.zeros((2, 2), np.int32)  # 0 red, 1 green, 2 blue at (i % 2, j % 2)
        pattern = next(p for p in ("RGGB", "GRBG", "GBRG", "BGGR") if p in cfg["bayerPattern"])
        for p, ch in enumerate(pattern):
            self.color[p // 2, p % 2] = "RGB".index(ch)
        self.ccm = composite_ccm(cfg)
        self.lut = tone_curve_lut(cfg, apply_tone_curve)
        self.width = cfg["width"] // pow2_downscale  # setDimensions :1239-1245
        self.height = cfg["height"] // pow2_downscale
        self.max_dimension = max(self.width, self.height)
        self.vig_h = np.array([bezier_curve(cfg["vignetteRollOffH"], F(x) / F(self.max_dimension)) for x in range(self.width)], F)
        self.vig_v = np.array([bezier_curve(cfg["vignetteRollOffV"], F(y) / F(self.max_dimension)) for y in range(self.height)], F)
        ii, jj = np.meshgrid(np.arange(self.height), np.arange(self.width), indexing="ij")
        self.ch = self.color[ii % 2, jj % 2]

    def channel(self, i, j):
        return int(self.color[i % 2, j % 2])

    # ---- loadImageFromSensor (:767-835) + resizeInput (:323-344)
    def sensor_image(self, raw_bytes):
        cfg = self.cfg
        sw, sh, bits = cfg["width"], cfg["height"], cfg["bitsPerPixel"]
        assert sw and sh and sw % 2 == 0 and sh % 2 == 0 and bits in (8, 16)
        dt = np.uint8 if bits == 8 else np.dtype("<u2" if cfg["isLittleEndian"] else ">u2")  # byteSwap :826
        data = np.frombuffer(raw_bytes, dtype=dt, count=sw * sh).astype(np.int64)
        planar, row_major = cfg["planeOrder"] != "", cfg["isRowMajor"]
        pw, ph = sw // 2, sh // 2
        k = np.arange(sw * sh)

        def linear_to_matrix(k, rows, cols, row_major=True):  # MathUtil.h:132-136
            return (k // cols, k % cols) if row_major else (k % rows, k // rows)

        if planar:
            order, bayer, found = cfg["planeOrder"], cfg["bayerPattern"], False
            to_bayer = []
            for i in range(4):  # getPlaneOrderToBayerOrder :346-354
                to_bayer.append(order.rfind(bayer[i]) if found else order.find(bayer[i]))
                found |= bayer[i] == "G"
            channel = k // (pw * ph)
            row, col = linear_to_matrix(k - channel * pw * ph, ph, pw, row_major)
            channel = np.array(to_bayer)[channel]
        else:
            row, col = linear_to_matrix(k, sh, sw, row_major)
            channel = (row % 2) * 2 + (col % 2)
            row, col = row // 2, col // 2
        image = np.zeros((sh, sw), np.int64)
        image[2 * row + channel // 2, 2 * col + channel % 2] = data
        return image

    def load(self, raw_bytes):
        image = self.sensor_image(raw_bytes)
        rows, cols = image.shape
        n = self.resize
        area_recip = F(1) / (F((1 << self.cfg["bitsPerPixel"]) - 1) * F(n * n))
        r = 2 if n > 1 else 1
        raw = np.zeros((self.height, self.width), F)
        for i in range(self.height):
            for j in range(self.width):
                s = F(0)
                for k in range(n):
                    ipp = reflect(i * n + k * 2 + (i % r), rows)
                    for l in range(n):  # noqa: E741
                        jpp = reflect(j * n + l * 2 + (j % r), cols)
                        s = s + F(image[ipp, jpp])
                raw[i, j] = s * area_recip
        return raw

    # ---- blackLevelAdjust :1061-1081, antiVignette :1096-1105, whiteBalance :962-978, clampAndStretch :1083-1094
    def pixel_stages(self, raw):
        cfg, ch = self.cfg, self.ch
        raw = raw.copy()
        black = np.array(cfg["blackLevel"], F)
        scale = F(1) / (F(1) - black)
        adjusted = (raw - black[ch]) * scale[ch]
        raw = np.where(raw < F(1), adjusted, raw).astype(F)
        v_h = self.vig_h[np.arange(self.width)[None, :], ch]
        v_v = self.vig_v[np.arange(self.height)[:, None], ch]
        raw = raw * (v_h * v_v)
        raw = raw * np.array(cfg["whiteBalanceGain"], F)[ch]
        raw = np.where(raw < F(0), F(0), np.where(raw > F(1), F(1), raw)).astype(F)
        lo, hi = np.array(cfg["clampMin"], F)[ch], np.array(cfg["clampMax"], F)[ch]
        v = np.where(raw < lo, lo, np.where(raw > hi, hi, raw)).astype(F)
        with np.errstate(all="ignore"):
            return ((v - lo) / (hi - lo)).astype(F)

    # ---- removeStuckPixels :980-1059
    def remove_stuck_pixels(self, raw):
        cfg = self.cfg
        radius, threshold = cfg["stuckPixelRadius"], cfg["stuckPixelThreshold"]
        darkness = F(cfg["stuckPixelDarknessThreshold"])
        raw = raw.copy()
        if radius <= 0:
            return raw
        h, w = raw.shape
        for i in range(h):
            even = i % 2 == 0
            j_start, j_end, j_step = (0, w - 1, 1) if even else (w - 1, 0, -1)
            j = j_start
            while j != j_end:  # the scan's last pixel of each row is skipped
                mine = self.channel(i, j)
                region = []
                mean = F(0)
                for y in range(-radius, radius + 1):
                    ip = reflect(i + y, h)
                    for x in range(-radius, radius + 1):
                        jp = reflect(j + x, w)
                        if self.channel(ip, jp) == mine:
                            mean = mean + raw[ip, jp]
                            region.append((raw[ip, jp], ip, jp))
                mean = mean / F(len(region))
                if mean < darkness:
                    region.sort(key=lambda p: p[0])
                    k = len(region) - 1
                    while k >= len(region) - threshold and k >= 0:
                        if region[k][1] == i and region[k][2] == j:
                            raw[i, j] = region[len(region) // 2][0]
                            break
                        k -= 1
                j += j_step
        return raw

    # ---- demosaic :1115-1175
    def split(self, raw):
        return [np.where(self.ch == c, raw, F(0)).astype(F) for c in range(3)]

    def red_green_row(self, i):
        return self.channel(i, 0) == 0 or self.channel(i, 1) == 0

    def demosaic_bilinear(self, r, g, b):  # :93-127, in place, in scan order
        h, w = self.height, self.width
        two = F(2)
        for i in range(h):
            i_1, i1 = reflect(i - 1, h), reflect(i + 1, h)
            rg_row = self.red_green_row(i)
            for j in range(w):
                j_1, j1 = reflect(j - 1, w), reflect(j + 1, w)
                c = self.channel(i, j)
                if c == 0:
                    g[i, j] = bilerp_half(g[i_1, j], g[i1, j], g[i, j_1], g[i, j1])
                    b[i, j] = bilerp_half(b[i_1, j_1], b[i1, j_1], b[i_1, j1], b[i1, j1])
                elif c == 1:
                    if rg_row:
                        b[i, j] = (b[i_1, j] + b[i1, j]) / two
                        r[i, j] = (r[i, j_1] + r[i, j1]) / two
                    else:
                        r[i, j] = (r[i_1, j] + r[i1, j]) / two
                        b[i, j] = (b[i, j_1] + b[i, j1]) / two
                else:
                    g[i, j] = bilerp_half(g[i_1, j], g[i1, j], g[i, j_1], g[i, j1])
                    r[i, j] = bilerp_half(r[i_1, j_1], r[i1, j_1], r[i_1, j1], r[i1, j1])

    def demosaic_green_bilinear(self, r, g, b):  # :227-248
        h, w = self.height, self.width
        for i in range(h):
            i_1, i1 = reflect(i - 1, h), reflect(i + 1, h)
            for j in range(w):
                j_1, j1 = reflect(j - 1, w), reflect(j + 1, w)
                if self.channel(i, j) != 1:
                    g[i, j] = bilerp_half(g[i_1, j], g[i1, j], g[i, j_1], g[i, j1])
        self.demosaic_chroma_suppressed(r, g, b)

    def demosaic_chroma_suppressed(self, red, green, blue):  # :250-320
        h, w = self.height, self.width
        rmg, bmg = np.zeros((h, w), F), np.zeros((h, w), F)  # unfilled in the reference: 0 here
        for i in range(h):
            for j in range(w):
                c = self.channel(i, j)
                if c == 0:
                    rmg[i, j] = red[i, j] - green[i, j]
                elif c == 2:
                    bmg[i, j] = blue[i, j] - green[i, j]
        for i in range(h):
            i_1, i1, i_2, i2 = reflect(i - 1, h), reflect(i + 1, h), reflect(i - 2, h), reflect(i + 2, h)
            rg_row = self.red_green_row(i)
            for j in range(w):
                j_1, j1, j_2, j2 = reflect(j - 1, w), reflect(j + 1, w), reflect(j - 2, w), reflect(j + 2, w)
                c = self.channel(i, j)
                if c == 0:
                    blue[i, j] = (bmg[i_1, j_1] + bmg[i1, j_1] + bmg[i_1, j1] + bmg[i1, j1]) / F(4) + green[i, j]
                    red[i, j] = (rmg[i, j] + rmg[i_2, j] + rmg[i2, j] + rmg[i, j_2] + rmg[i, j2]) / F(5) + green[i, j]
                elif c == 1:
                    d1, d2 = (bmg, rmg) if rg_row else (rmg, bmg)
                    ch1, ch2 = (blue, red) if rg_row else (red, blue)
                    ch1[i, j] = (d1[i_1, j_2] + d1[i_1, j] + d1[i_1, j2] + d1[i1, j_2] + d1[i1, j2] + d1[i1, j2]) / F(6) + green[i, j]
                    ch2[i, j] = (d2[i_2, j_1] + d2[i, j_1] + d2[i2, j_1] + d2[i_2, j1] + d2[i, j1] + d2[i2, j1]) / F(6) + green[i, j]
                else:
                    red[i, j] = (rmg[i_1, j_1] + rmg[i1, j_1] + rmg[i_1, j1] + rmg[i1, j1]) / F(4) + green[i, j]
                    blue[i, j] = (bmg[i, j] + bmg[i_2, j] + bmg[i2, j] + bmg[i, j_2] + bmg[i, j2]) / F(5) + green[i, j]

    def demosaic_edge_aware(self, red, green, blue):  # :161-225
        h, w = self.height, self.width
        g_v, g_h, d_v, d_h = (np.zeros((h, w), F) for _ in range(4))
        two, four = F(2), F(4)
        for i in range(h):
            i_1, i1, i_2, i2 = reflect(i - 1, h), reflect(i + 1, h), reflect(i - 2, h), reflect(i + 2, h)
            for j in range(w):
                j_1, j1, j_2, j2 = reflect(j - 1, w), reflect(j + 1, w), reflect(j - 2, w), reflect(j + 2, w)
                c = self.channel(i, j)
                if c == 1:
                    g_v[i, j] = green[i, j]
                    g_h[i, j] = green[i, j]
                    d_v[i, j] = (abs(green[i2, j] - green[i, j]) + abs(green[i, j] - green[i_2, j])) / two
                    d_h[i, j] = (abs(green[i, j2] - green[i, j]) + abs(green[i, j] - green[i, j_2])) / two
                else:
                    g_v[i, j] = (green[i_1, j] + green[i1, j]) / two
                    g_h[i, j] = (green[i, j_1] + green[i, j1]) / two
                    d_v[i, j] = abs(green[i_1, j] - green[i1, j]) / two
                    d_h[i, j] = abs(green[i, j_1] - green[i, j1]) / two
                    ch = red if c == 0 else blue
                    g_v[i, j] += (two * ch[i, j] - ch[i_2, j] - ch[i2, j]) / four
                    g_h[i, j] += (two * ch[i, j] - ch[i, j_2] - ch[i, j2]) / four
                    d_v[i, j] += abs(-two * ch[i, j] + ch[i_2, j] + ch[i2, j]) / two
                    d_h[i, j] += abs(-two * ch[i, j] + ch[i, j_2] + ch[i, j2]) / two
        vote = (d_h <= d_v).astype(np.int32)
        rows = [reflect(x, h) for x in range(-4, h + 4)]
        cols = [reflect(x, w) for x in range(-4, w + 4)]
        padded = vote[np.ix_(rows, cols)]
        for i in range(h):
            for j in range(w):
                count = int(padded[i:i + 9, j:j + 9].sum())  # an integer count: the order of the sum cannot matter
                green[i, j] = lerp(g_v[i, j], g_h[i, j], F(count) / F(81))
        self.demosaic_chroma_suppressed(red, green, blue)

    def demosaic(self, raw):
        r, g, b = self.split(raw)
        if self.filter == 0:
            self.demosaic_bilinear(r, g, b)
        elif self.filter == 3:
            self.demosaic_green_bilinear(r, g, b)
        else:
            self.demosaic_edge_aware(r, g, b)
        return np.stack([r, g, b])

    # ---- colorCorrect :1177-1205
    def color_correct(self, rgb):
        m, top = self.ccm, F(LUT_SIZE - 1)
        out = np.zeros_like(rgb)
        with np.errstate(all="ignore"):
            for c in range(3):
                v = m[c, 0] * rgb[0] + m[c, 1] * rgb[1] + m[c, 2] * rgb[2]
                v = np.where(v < F(0), F(0), np.where(v > top, top, v)).astype(F)
                idx = np.where(np.isnan(v), 0, v).astype(np.int64)  # truncation; NaN (undefined there) -> entry 0
                out[c] = self.lut[idx, c]
        return out

    # ---- sharpen :1207-1223
    def sharpens(self):
        s = self.cfg["sharpening"]
        return s[0] != 0.0 and s[1] != 0.0 and s[2] != 0.0

    def iir_low_pass(self, image):  # Filter.h:35-85 with ReflectBoundary both ways, maxVal = 1; image [3, h, w]
        h, w = self.height, self.width
        alpha = powf(F(self.cfg["sharpeningSupport"]), F(1) / F(4))
        img = np.ascontiguousarray(image.transpose(1, 2, 0))  # Vec3f per pixel
        lp = np.zeros((h, w, 3), F)  # unfilled in the reference: 0 here
        buffer = np.zeros((max(h, w), 3), F)  # likewise
        zero, one = F(0), F(1)

        def clamp3(v):
            return np.where(v < zero, zero, np.where(v > one, one, v)).astype(F)

        for i in range(h):
            v = img[i, w - 1].copy()
            for j in range(w):
                v = lerp(img[i, j], v, alpha)
                buffer[reflect(j - 1, w)] = v
            v = buffer[0].copy()
            for j in range(w - 1, -1, -1):
                v = lerp(buffer[j].copy(), v, alpha)  # math_util::wrap(j, cols) = j
                lp[i, reflect(j + 1, w)] = clamp3(v)
        for j in range(w):
            v = lp[1, j].copy()
            for i in range(h):
                v = lerp(lp[i, j], v, alpha)
                buffer[reflect(i - 1, h)] = v
            v = buffer[h - 2].copy()
            for i in range(h - 1, -2, -1):
                v = lerp(buffer[reflect(i, h)].copy(), v, alpha)
                lp[reflect(i + 1, h), j] = clamp3(v)
        return np.ascontiguousarray(lp.transpose(2, 0, 1))

    def sharpen_with_low_pass(self, image, lp):  # Filter.h:87-118
        out = np.zeros_like(image)
        noise_core = F(self.cfg["noiseCore"])
        vexp = np.vectorize(lambda x: _libm.expf(float(x)), otypes=[F])
        for c in range(3):
            amount = F(1) + F(self.cfg["sharpening"][c])
            hp = image[c] - lp[c]
            ng = F(1) - vexp(-((hp * hp) * noise_core))
            v = lp[c] + hp * ng * amount
            out[c] = np.where(v < F(0), F(0), np.where(v > F(1), F(1), v))
        return out

    # ---- getImage :1276-1297
    def output(self, rgb):
        bits = self.cfg["bitsPerPixel"]
        scaled = F((1 << bits) - 1) * rgb
        img = np.where(np.isnan(scaled), 0, scaled).astype(np.uint8 if bits == 8 else np.uint16)  # truncation
        return np.ascontiguousarray(img[::-1].transpose(1, 2, 0))  # BGR, [h, w, 3]

    def run(self, raw_bytes):
        out = {"load": self.load(raw_bytes)}
        out["pixel"] = self.pixel_stages(out["load"])
        out["stuck"] = self.remove_stuck_pixels(out["pixel"])
        out["demosaic"] = self.demosaic(out["stuck"])
        out["color"] = self.color_correct(out["demosaic"])
        last = out["color"]
        if self.sharpens():
            out["lowpass"] = self.iir_low_pass(out["color"])
            out["sharpened"] = self.sharpen_with_low_pass(out["color"], out["lowpass"])
            last = out["sharpened"]
        out["image"] = self.output(last)
        return out
