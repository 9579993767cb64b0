"""tests/isp_ref.py (the CPU restatement of the reference's camera ISP that the GPU stages are compared with) held to
answers that can be derived by hand. No GPU."""
import numpy as np
import pytest

from tests import isp_ref
from tests.isp_ref import F


def config(w=16, h=12, **kw):
    c = {"width": w, "height": h, "bitsPerPixel": 16, "isLittleEndian": True}
    c.update(kw)
    return c


def test_reflect_at_both_borders():
    # MathUtil.h:42-44: the low border mirrors about pixel 0, the high border about the edge after the last pixel
    assert [isp_ref.reflect(x, 5) for x in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 4, 3]


def test_bezier_curves():
    one = [[0.25, 0.5, 2.0]]
    for t in (0.0, 0.5, 1.0):
        assert np.array_equal(isp_ref.bezier_curve(one, t), np.array(one[0], F))
    a, b, c = [1.0, 2.0, 4.0], [0.5, 0.25, 8.0], [3.0, 1.0, 2.0]
    assert np.array_equal(isp_ref.bezier_curve([a, b, c], 0.0), np.array(a, F))
    assert np.array_equal(isp_ref.bezier_curve([a, b, c], 1.0), np.array(c, F))
    mid = 0.25 * np.array(a) + 0.5 * np.array(b) + 0.25 * np.array(c)  # dyadic values: exact in fp32
    assert np.array_equal(isp_ref.bezier_curve([a, b, c], 0.5), mid.astype(F))


@pytest.mark.parametrize("pattern", ["RGGB", "GRBG", "GBRG", "BGGR"])
@pytest.mark.parametrize("filt", [0, 2, 3])
def test_constant_plane_stays_constant(filt, pattern):
    """Every filter interpolates with weights that sum to one, so a constant plane comes out constant. reflect() maps
    the pixel after the last one onto the last one itself, which breaks the Bayer phase there, and the edge-aware vote
    looks 4 pixels further: the claim holds away from the high border."""
    isp = isp_ref.Isp(config(24, 20, bayerPattern=pattern), demosaic_filter=filt)
    plane = np.full((20, 24), F(0.375))
    rgb = isp.demosaic(plane)
    m = 8 if filt == 2 else 3
    assert np.array_equal(rgb[:, :-m, :-m], np.full((3, 20 - m, 24 - m), F(0.375)))


@pytest.mark.parametrize("pattern", ["RGGB", "GBRG"])
def test_horizontal_ramp_through_bilinear(pattern):
    isp = isp_ref.Isp(config(16, 12, bayerPattern=pattern), demosaic_filter=0)
    ramp = np.tile(np.arange(16, dtype=F) / F(64), (12, 1))  # dyadic: the averages are exact
    rgb = isp.demosaic(ramp)
    for c in range(3):
        assert np.array_equal(rgb[c][1:-1, 1:-1], ramp[1:-1, 1:-1]), c


def test_tone_curve_off_is_a_quantiser():
    isp = isp_ref.Isp(config(), apply_tone_curve=False)
    assert np.array_equal(isp.lut[:, 0], (F(1) / F(4095)) * np.arange(4096, dtype=F))
    isp.ccm = np.eye(3, dtype=F) * F(4095)  # the composite matrix of an exact identity
    x = np.random.default_rng(0).random((3, 12, 16)).astype(F)
    out = isp.color_correct(x)
    k = np.floor(x * F(4095)).astype(np.int64)
    assert np.array_equal(out, isp.lut[k, 0])
    assert np.abs(out.astype(np.float64) - k / 4095.0).max() < 1e-7
    # the default config's composite matrix is the identity up to the rounding of yuv2rgb * rgb2yuv
    assert np.abs(isp_ref.Isp(config()).ccm / F(4095) - np.eye(3)).max() < 1e-4


def _raw(values, little):
    return values.astype("<u2" if little else ">u2").tobytes()


def test_big_and_little_endian_input_agree():
    v = np.random.default_rng(1).integers(0, 65536, (12, 16))
    a = isp_ref.Isp(config(isLittleEndian=True)).run(_raw(v, True))
    b = isp_ref.Isp(config(isLittleEndian=False)).run(_raw(v, False))
    assert np.array_equal(a["image"], b["image"]) and np.array_equal(a["load"], b["load"])
    assert np.array_equal(a["load"], v.astype(F) * (F(1) / F(65535)))


@pytest.mark.parametrize("row_major", [True, False])
def test_planar_and_interleaved_input_agree(row_major):
    v = np.random.default_rng(2).integers(0, 65536, (12, 16))
    a = isp_ref.Isp(config(bayerPattern="GBRG")).run(_raw(v, True))
    # planes in the pattern's own order: plane p holds Bayer position p (getPlaneOrderToBayerOrder is then the identity)
    planes = [v[p // 2::2, p % 2::2] for p in range(4)]
    flat = np.concatenate([(p if row_major else p.T).reshape(-1) for p in planes])
    b = isp_ref.Isp(config(bayerPattern="GBRG", planeOrder="GBRG", isRowMajor=row_major)).run(_raw(flat, True))
    assert np.array_equal(a["load"], b["load"]) and np.array_equal(a["image"], b["image"])
    # column-major interleaved input
    c = isp_ref.Isp(config(isRowMajor=False)).run(_raw(v.T.reshape(-1), True))
    assert np.array_equal(a["load"], c["load"])


def test_binning_is_bayer_aware():
    """resizeInput with factor 2 (:323-344): output (i, j) sums the 2 x 2 sensor pixels of its own Bayer phase."""
    v = np.random.default_rng(3).integers(0, 65536, (12, 16))
    isp = isp_ref.Isp(config(), pow2_downscale=2)
    got = isp.load(_raw(v, True))
    assert got.shape == (6, 8)
    i, j = 3, 4  # odd row, even column: sensor rows 6 + 1, 6 + 3 and columns 8, 10
    want = ((F(v[7, 8]) + F(v[7, 10])) + F(v[9, 8])) + F(v[9, 10])
    assert got[i, j] == want * (F(1) / (F(65535) * F(4)))


def test_hot_pixel_in_a_dark_region_becomes_the_median():
    cfg = config(16, 12, stuckPixelRadius=2, stuckPixelThreshold=1, stuckPixelDarknessThreshold=0.5)
    isp = isp_ref.Isp(cfg)
    rng = np.random.default_rng(4)
    plane = (rng.permutation(16 * 12).reshape(12, 16).astype(F) + F(1)) / F(4096)  # distinct, dark
    plane[5, 6] = F(0.9)
    out = isp.remove_stuck_pixels(plane)
    same = [plane[i, j] for i in range(3, 8) for j in range(4, 9) if isp.channel(i, j) == isp.channel(5, 6)]
    assert out[5, 6] == sorted(same)[len(same) // 2] and out[5, 6] < F(0.1)
    # only a pixel among the `stuckPixelThreshold` largest of its own window is ever replaced, and only in a dark region
    for kw in ({"stuckPixelThreshold": 0}, {"stuckPixelDarknessThreshold": 0.0}, {"stuckPixelRadius": 0}):
        assert np.array_equal(isp_ref.Isp(dict(cfg, **kw)).remove_stuck_pixels(plane), plane), kw
    # the scan skips the last pixel of each row: a hot pixel there stays
    plane2 = plane.copy()
    plane2[5, 6] = plane[5, 7]
    plane2[4, 15] = F(0.9)  # row 4 is scanned left to right, so column 15 is its last pixel
    assert isp.remove_stuck_pixels(plane2)[4, 15] == F(0.9)
