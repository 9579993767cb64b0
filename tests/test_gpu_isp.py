"""The camera ISP on the GPU (derp_isp_*, csrc/derp_isp.h) against tests/isp_ref.py, the CPU restatement of the
reference's CameraIsp: every stage derp_isp_stage can show, the host-built tables and the final image, bit for bit
(0 differing values; no tolerance anywhere in this file).

Sensor sizes: 6 x 6 is the smallest at which the 9 x 9 vote's reflection stays in range, and every pixel there is a
border pixel; 70 x 38 is a multiple of no tile or wave size; 130 x 66 with downscale 2 gives 65 x 33, so both output
dimensions are odd and the Bayer phase meets an odd edge. 38 x 70 is the same the other way up: iirLowPass's line buffer
leaves the vertical pass a stale element only when rows < cols."""
import numpy as np
import pytest

from tests import isp_ref

pytestmark = pytest.mark.gpu

STAGES = ["load", "pixel", "stuck", "demosaic", "color", "lowpass", "sharpened"]

RICH = {  # every knob away from its default
    "blackLevel": [0.02, 0.03, 0.025], "vignetteRollOffH": [[1.3, 1.2, 1.25], [0.9, 1.0, 0.95], [1.4, 1.3, 1.2]],
    "vignetteRollOffV": [[1.2, 1.25, 1.3], [1.0, 0.9, 0.95], [1.1, 1.3, 1.35]], "whiteBalanceGain": [1.6, 1.0, 1.9],
    "clampMin": [0.01, 0.02, 0.015], "clampMax": [0.95, 0.9, 0.97],
    "ccm": [[1.5, -0.3, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], "saturation": 1.2, "gamma": [0.45, 0.5, 0.55],
    "lowKeyBoost": [0.1, 0.05, 0.0], "highKeyBoost": [0.05, 0.1, -0.05], "contrast": 1.1, "sharpening": [0.5, 0.4, 0.6],
    "sharpeningSupport": 0.01, "noiseCore": 50.0,
}


def case(name, w, h, filt=0, down=1, tone=True, **cfg):
    return pytest.param(dict(w=w, h=h, filt=filt, down=down, tone=tone, cfg=cfg), id=name)


CASES = []
for filt in (0, 2, 3):
    CASES += [case("6x6-f%d" % filt, 6, 6, filt), case("70x38-f%d" % filt, 70, 38, filt),
              case("130x66-down2-f%d" % filt, 130, 66, filt, down=2)]
    for pattern in ("RGGB", "GRBG", "BGGR"):  # GBRG is the default of every other case
        CASES.append(case("70x38-f%d-%s" % (filt, pattern), 70, 38, filt, bayerPattern=pattern))
    CASES.append(case("70x38-f%d-rich" % filt, 70, 38, filt, **RICH))
CASES += [
    case("70x38-8bit", 70, 38, 0, bitsPerPixel=8),
    case("70x38-8bit-rich-f2", 70, 38, 2, bitsPerPixel=8, **RICH),
    case("70x38-little-endian", 70, 38, 3, isLittleEndian=True),
    case("70x38-planar-column-major", 70, 38, 0, planeOrder="RGGB", isRowMajor=False),
    case("70x38-planar-row-major-f2", 70, 38, 2, planeOrder="bggr", bayerPattern="grbg"),
    case("70x38-column-major", 70, 38, 3, isRowMajor=False),
    case("130x66-down2-rich-f3", 130, 66, 3, down=2, **RICH),
    case("130x66-down2-rich-RGGB", 130, 66, 0, down=2, bayerPattern="RGGB", **RICH),
    case("38x70-rich", 38, 70, 0, **RICH),
    case("6x6-rich-f2", 6, 6, 2, **RICH),
    case("130x66-down8-f2", 130, 66, 2, down=8),
    case("130x66-down4-rich", 130, 66, 0, down=4, **RICH),
    case("70x38-stuck-pixels", 70, 38, 0, stuckPixelRadius=2, stuckPixelThreshold=2, stuckPixelDarknessThreshold=0.6),
    case("70x38-stuck-pixels-f2-BGGR", 70, 38, 2, stuckPixelRadius=2, stuckPixelThreshold=3,
         stuckPixelDarknessThreshold=0.45, bayerPattern="BGGR"),
    case("70x38-tone-curve-off", 70, 38, 0, tone=False, **RICH),
    case("70x38-sharpening-one-zero", 70, 38, 0, **dict(RICH, sharpening=[0.5, 0.0, 0.6])),
]


def raw_bytes(cfg, seed):
    """seeded values, distinct over the whole 16-bit frame (so no sort tie can decide a stuck-pixel result)"""
    rng = np.random.default_rng(seed)
    n = cfg["width"] * cfg["height"]
    if cfg.get("bitsPerPixel", 16) == 8:
        return rng.integers(0, 256, n).astype(np.uint8).tobytes()
    values = rng.choice(65536, size=n, replace=False)
    return values.astype("<u2" if cfg.get("isLittleEndian") else ">u2").tobytes()


def differing(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return int(np.count_nonzero(got.view(np.uint32 if got.dtype == np.float32 else got.dtype) !=
                                want.view(np.uint32 if want.dtype == np.float32 else want.dtype)))


@pytest.mark.parametrize("c", CASES)
def test_stages_and_image_equal_the_restatement(built, c):
    from facebook360_dep_amd import derp

    cfg = dict(c["cfg"], width=c["w"], height=c["h"])
    raw = raw_bytes(cfg, seed=c["w"] * 1000 + c["h"] + c["filt"])
    ref = isp_ref.Isp(cfg, c["filt"], c["down"], c["tone"])
    want = ref.run(raw)
    isp = derp.Isp(cfg, c["filt"], c["down"], c["tone"])
    try:
        assert (isp.width, isp.height) == (ref.width, ref.height)
        image = isp.process(raw)
        report = {}
        for name, table, mine in zip(("vignette_h", "vignette_v", "ccm", "tone_lut"), isp.tables(),
                                     (ref.vig_h, ref.vig_v, ref.ccm, ref.lut)):
            report[name] = differing(table, mine)
        for stage in STAGES:
            if stage in want:
                report[stage] = differing(isp.stage(stage), want[stage])
            else:  # sharpening does not run (a zero component): the library says so instead of showing a stale plane
                with pytest.raises(derp.DerpError, match="sharpening does not run"):
                    isp.stage(stage)
        report["image"] = differing(image, want["image"])
        print("differing values:", report)
        assert all(v == 0 for v in report.values()), report
        if ref.sharpens():
            assert differing(want["sharpened"], want["color"]) > 0  # the case does exercise the sharpener
        if cfg.get("stuckPixelRadius"):
            assert differing(want["stuck"], want["pixel"]) > 0  # ... and the stuck-pixel scan replaces something
    finally:
        isp.close()


def test_one_handle_serves_many_frames(built):
    """the second frame's result does not depend on the first (stale element, scratch planes)"""
    from facebook360_dep_amd import derp

    cfg = dict(RICH, width=70, height=38)
    isp = derp.Isp(cfg, 2)
    try:
        a, b = raw_bytes(cfg, 1), raw_bytes(cfg, 2)
        first = isp.process(a)
        isp.process(b)
        assert np.array_equal(isp.process(a), first)
    finally:
        isp.close()


@pytest.mark.parametrize("kwargs,message", [
    (dict(demosaic_filter=4), "expecting Demosaic filter"),
    (dict(demosaic_filter=1), "frequency demosaic is not built"),
    (dict(pow2_downscale=3), "expecting a resize value of 1, 2, 4, or 8"),
    (dict(width=71), "must be even"),
    (dict(bitsPerPixel=12), "bitsPerPixel must be 8 or 16"),
    (dict(planeOrder="RGBB"), "planeOrder"),
    (dict(width=16, height=16, pow2_downscale=8), "too small"),
])
def test_refusals(built, kwargs, message):
    from facebook360_dep_amd import derp

    kwargs = dict(kwargs)
    opts = {k: kwargs.pop(k) for k in ("demosaic_filter", "pow2_downscale") if k in kwargs}
    with pytest.raises(derp.DerpError, match=message):
        derp.Isp(dict(dict(width=70, height=38), **kwargs), **opts)


def test_short_input_is_refused(built):
    from facebook360_dep_amd import derp

    isp = derp.Isp(dict(width=70, height=38))
    try:
        with pytest.raises(derp.DerpError, match="unexpected end of file"):
            isp.process(bytes(70 * 38 * 2 - 1))
    finally:
        isp.close()
