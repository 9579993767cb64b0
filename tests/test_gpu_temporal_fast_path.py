"""The tiled temporal filter's fast form (k_temporal_tiled<1, true> and <-1, true>: expf with the one range test an
argument in [-inf, -0] needs, a block vote per window frame that lets a fully set tile skip its mask reads, radius 1
unrolled) beside the generic form (DERP_TEMPORAL_GENERIC=1) and the oracle's `temporal_filter` on the same inputs.
NaN == NaN, +0 != -0, no tolerance anywhere in this file."""
import numpy as np
import pytest

SHAPES = [(5, 3), (32, 8), (33, 9)]  # w, h: smaller than a tile, exactly one 32 x 8 tile, one tile and a second row / column
WINDOWS = [(1, 0), (2, 0), (2, 1), (5, 0), (5, 4)]  # frames, index of the filtered frame: the centre at either end
RADII = (1, 2)
MASKS = ("all_set", "halo_byte", "frame_zero", "ref_holes")
SIGMA = 0.01
LEVEL_LOOP = (SIGMA, 0.5, 1.0, 0.5)  # what the sequence driver passes
PARAMS = {
    "level_loop": LEVEL_LOOP,
    "zero_weight": (SIGMA, 0.5, 0.0, 0.5),
    "negative_weight": (SIGMA, 0.5, -1.0, 0.5),
    "sigma_zero": (0.0, 0.5, 1.0, 0.5),
}
TFLUSH = np.float32(float.fromhex("-0x1.9fe368p6"))  # -103.97: expf returns 0 below it


def takes_fast_form(sigma, w0, w1, w2):
    """The host's choice restated (temporal_fast_tap_ok in csrc/derp_capi.hip). The context does not report which kernel
    ran, so this formula is what pins that the parameter sets above sit on either side of the switch."""
    sig2 = np.float32(sigma) * np.float32(sigma)
    ok = all(np.float32(w) >= 0 and np.isfinite(np.float32(w)) for w in (w0, w1, w2))
    return bool(ok and sig2 > 0 and np.isfinite(sig2))


def test_parameter_sets_sit_on_both_sides_of_the_predicate():
    assert takes_fast_form(*PARAMS["level_loop"]) and takes_fast_form(*PARAMS["zero_weight"])
    assert not takes_fast_form(*PARAMS["negative_weight"]) and not takes_fast_form(*PARAMS["sigma_zero"])
    assert not takes_fast_form(1e-30, 0.5, 1.0, 0.5)  # sigma^2 underflows to 0 in fp32
    assert not takes_fast_form(SIGMA, np.inf, 1.0, 0.5) and not takes_fast_form(SIGMA, np.nan, 1.0, 0.5)


def inputs(w, h, n):
    """guides u16 [h, w, 3] whose differences between frames and between neighbours reach about 18000 grey levels: at
    sigma 0.01 the exponent -(sum of w * (d / 65535)^2) / sigma^2 then runs from 0 to about -1500"""
    rng = np.random.default_rng([15, w, h, n])
    base = rng.integers(20000, 40000, size=(h, w, 1))
    guides = [np.clip(base + rng.integers(-9000, 9001, size=(h, w, 3)), 0, 65535).astype(np.uint16) for _ in range(n)]
    guides[-1][0, 0] = guides[0][0, 0]  # and an exponent of exactly -0
    disps = [(1.0 / rng.uniform(0.6, 30.0, size=(h, w))).astype(np.float32) for _ in range(n)]
    return guides, disps


def masks(name, w, h, n, centre):
    rng = np.random.default_rng([16, w, h, n, centre])
    out = [np.ones((h, w), np.uint8) for _ in range(n)]
    if name == "halo_byte":
        # the last pixel of row 0: at 33 wide it lies in the halo of the first tile (and inside the second), in the smaller
        # shapes the clamped halo cells of the only tile repeat it
        out[n - 1 - centre if n > 1 else 0][0, w - 1] = 0
    elif name == "frame_zero":
        out[(centre + 1) % n][:] = 0  # (the filtered frame itself when the window has one frame)
    elif name == "ref_holes":
        out[centre] = (rng.random((h, w)) > 0.3).astype(np.uint8)
        out[centre][0, 0] = 0
    return out


def exponents(guides, centre, params):
    """the expf arguments of the centre taps of every window frame, as the kernel forms them in fp32"""
    sigma, w0, w1, w2 = (np.float32(v) for v in params)
    ref = guides[centre].astype(np.int32)
    xs = []
    for g in guides:
        e = ((ref - g.astype(np.int32)).astype(np.float32) / np.float32(65535.0))
        wd = w0 * (e[..., 0] * e[..., 0]) + w1 * (e[..., 1] * e[..., 1]) + w2 * (e[..., 2] * e[..., 2])
        xs.append(-wd / (sigma * sigma))
    return np.stack(xs)


def test_inputs_reach_both_sides_of_the_range_test():
    for w, h in SHAPES:
        guides, _ = inputs(w, h, 5)
        for name in ("level_loop", "zero_weight"):
            x = exponents(guides, 0, PARAMS[name])
            assert ((x > TFLUSH) & (x < 0)).any() and (x < TFLUSH).any() and (x == 0).any(), (w, h, name)


def differing(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return int((~same).sum())


@pytest.fixture(scope="module")
def contexts(built):
    """(default, generic): two contexts of one process; the switch is read when a context is created"""
    import os

    from facebook360_dep_amd import derp, synth

    n, res, _ = synth.config("tiny")
    cams = synth.make_rig(n, res)["cameras"]
    saved = os.environ.pop("DERP_TEMPORAL_GENERIC", None)
    try:
        fast = derp.Derp(cams, partial_coverage=1)
        os.environ["DERP_TEMPORAL_GENERIC"] = "1"
        generic = derp.Derp(cams, partial_coverage=1)
    finally:
        os.environ.pop("DERP_TEMPORAL_GENERIC", None)
        if saved is not None:
            os.environ["DERP_TEMPORAL_GENERIC"] = saved
    yield fast, generic
    fast.close()
    generic.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_fast_form_equals_the_generic_form_and_the_oracle(contexts, w, h):
    from oracle import oracle_lib as O

    fast, generic = contexts
    moved = 0
    for n, centre in WINDOWS:
        guides, disps = inputs(w, h, n)
        for mask_name in MASKS:
            mk = masks(mask_name, w, h, n, centre)
            for pname, (sigma, w0, w1, w2) in PARAMS.items():
                for radius in RADII:
                    want = O.temporal_filter(guides, disps, mk, centre, sigma, radius, w0, w1, w2)
                    got = fast.temporal_filter(guides, disps, mk, centre, sigma, radius, w0, w1, w2)
                    kept = generic.temporal_filter(guides, disps, mk, centre, sigma, radius, w0, w1, w2)
                    a, b = differing(got, kept), differing(got, want)
                    print("%dx%d n %d centre %d %s %s r %d: %d differ from the generic form, %d from the oracle" %
                          (w, h, n, centre, mask_name, pname, radius, a, b))
                    assert a == 0 and b == 0, (w, h, n, centre, mask_name, pname, radius, a, b)
                    if pname == "level_loop":
                        moved += differing(got, disps[centre])
    assert moved > 0  # the comparisons above are not of an identity
