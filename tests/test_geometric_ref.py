"""The numpy restatement of GeometricConsistency (tests/geometric_ref.py) against values worked out by hand,
and its depths against the synthetic scene's truth. No GPU."""
import numpy as np

from tests import geometric_ref as G

I16, F32 = np.int16, np.float32


def test_blur3_rounds_half_to_even_saturates_and_reflects():
    # a box sum of 9 * 4.5 = 40.5 is no integer; the nearest an int32 sum comes to a tie is k + 4/9 and k + 5/9:
    # sums 40 and 41 (4.44.., 4.55..) either side of 4.5, and their negatives
    for total, want in ((40, 4), (41, 5), (-40, -4), (-41, -5), (36, 4), (45, 5), (-45, -5), (4, 0), (5, 1), (-5, -1)):
        img = np.zeros((5, 5), I16)
        img[2, 2] = total  # the only non-zero texel of the centre's box
        assert G.blur3(img)[2, 2] == want, total
    # the rule itself at an exact tie, where a product with (1.0 / 9) cannot land: rint is half to even
    assert np.rint(4.5) == 4 and np.rint(5.5) == 6 and np.rint(-4.5) == -4
    # saturation: nine texels of -32768 average to -32768, of 32767 to 32767, and neither wraps
    assert (G.blur3(np.full((4, 4), -32768, I16)) == -32768).all()
    assert (G.blur3(np.full((4, 4), 32767, I16)) == 32767).all()
    assert G.saturate16(np.array([40000, -40000, 32767, -32768])).tolist() == [32767, -32768, 32767, -32768]
    # reflect-101 at a corner: the box of (0, 0) of
    #   1 2 3      is   5 4 5
    #   4 5 6           2 1 2      sum 33 -> 3.67 -> 4
    #   7 8 9           5 4 5
    img = np.arange(1, 10, dtype=I16).reshape(3, 3)
    out = G.blur3(img)
    assert out[0, 0] == 4
    assert out[1, 1] == 5  # 45 / 9
    assert out[2, 2] == 6  # 5 6 5 / 8 9 8 / 5 6 5 = 57 -> 6.33
    assert out[0, 2] == 4  # 5 6 5 / 2 3 2 / 5 6 5 = 39 -> 4.33
    # four channels are blurred independently
    img4 = np.stack([img, -img, 2 * img, np.zeros_like(img)], axis=2)
    out4 = G.blur3(img4)
    assert np.array_equal(out4[:, :, 0], out) and np.array_equal(out4[:, :, 1], -out) and (out4[:, :, 3] == 0).all()


def test_sq_by_hand():
    # a * a / 32767, round half to even, saturate
    cases = {0: 0, 1: 0, 128: 1, 127: 0, 181: 1, 182: 1, 222: 2, 1000: 31, -1000: 31, 32767: 32767, -32767: 32767,
             -32768: 32767, 23170: 16384, 100: 0, 200: 1}
    # 128^2 = 16384 = 0.50002 * 32767 -> 1; 127^2 = 16129 = 0.492 -> 0; 222^2 = 49284 = 1.504 -> 2; 10^6 / 32767 = 30.52
    for a, want in cases.items():
        assert int(G.sq(np.array([a], I16))[0]) == want, a
    # the integer form the kernel uses, (2 a^2 + 32767) / 65534 capped at 32767, is the same function on all of int16
    a = np.arange(-32768, 32768, dtype=np.int64)
    assert np.array_equal(G.sq(a.astype(I16)).astype(np.int64), np.minimum((2 * a * a + 32767) // 65534, 32767))


def test_blur9_integer_form():
    """the kernel's integer rounding of a box sum, floor((2 s + 9) / 18), is rint(s * (1.0 / 9)) for every sum nine
    int16 values can make"""
    s = np.arange(-9 * 32768, 9 * 32767 + 1, dtype=np.int64)
    assert np.array_equal(np.rint(s.astype(np.float64) * (1.0 / 9)).astype(np.int64), (2 * s + 9) // 18)


def test_slice_disparities_in_fp32():
    lo = F32(1.0 / 1e4)
    for count in (1, 2, 37, 113):
        got = G.slice_disparities(count)
        assert got.dtype == F32 and len(got) == count
        for s in (0, count // 2, count - 1):
            n = F32((s + 0.5) / count)  # the double quotient, rounded once to float
            a = F32(F32(1) - n) * lo
            b = n * F32(1)
            assert got[s] == F32(a + b), (count, s)
        assert np.all(np.diff(got) > 0) and got[0] > lo and got[-1] < 1
    assert G.slice_disparities(1)[0] == F32(F32(0.5) * lo + F32(0.5))
    # by hand for one slice of two: n = 0.25 -> 0.75 * 1e-4f + 0.25
    assert G.slice_disparities(2)[0] == F32(F32(0.75) * lo) + F32(0.25)


def test_small_sizes_round_half_away():
    cams = [{"resolution": [64, 64]}, {"resolution": [50, 38]}, {"resolution": [10, 6]}]
    assert G.small_sizes(cams, 2) == [(32, 32), (25, 19), (5, 3)]
    assert G.small_sizes(cams, 4) == [(16, 16), (13, 10), (3, 2)]  # 12.5 -> 13, 9.5 -> 10, 2.5 -> 3, 1.5 -> 2


SANITY_STEP = 0.12
MEASURED_SHARE = 0.3457  # of 5398 finite interior pixels, measured with this restatement (chance: 3 / 24 = 0.125)
# (2 of the 5400 interior pixels are NaN in the restatement's output: 0.0004, against the cap of 0.20 below)


def test_sweep_finds_the_scene(built):
    """On the 6-camera 64^2 synthetic frame at downscale 2 (24 slices): the share of interior finite pixels whose winning
    slice lies within one slice of the slice nearest the true depth. At 32 x 32 a slice is a quarter of a pixel of
    parallax, so texture noise decides many pixels (the same scene at 64 x 64 small images and 23 slices: 0.81)."""
    from facebook360_dep_amd import synth

    cams = synth.make_rig(6, 64)["cameras"]
    rendered = [synth.render_camera(c, 64, 64) for c in cams]
    sizes = G.small_sizes(cams, 2)
    frame = G.Frame(cams, [r[0] for r in rendered], sizes)
    count = G.slice_count(frame.rig, 0, SANITY_STEP)
    assert count >= 24
    disparities = G.slice_disparities(count).astype(np.float64)
    good = finite = interior = 0
    for d in range(len(cams)):
        depth, at = frame.sweep(d, SANITY_STEP, return_slice=True)
        truth = synth.resize_area(rendered[d][1].astype(np.float64), *sizes[d])
        nearest = np.abs(truth[:, :, None] - disparities[None, None, :]).argmin(axis=2)
        inner = np.zeros(depth.shape, bool)
        inner[1:-1, 1:-1] = True
        assert np.isnan(depth[~inner]).all()
        ok = inner & ~np.isnan(depth)
        good += int((ok & (np.abs(at - nearest) <= 1)).sum())
        finite += int(ok.sum())
        interior += int(inner.sum())
    share, nan_share = good / finite, 1 - finite / interior
    print("share %.4f of %d finite interior pixels, NaN share %.4f" % (share, finite, nan_share))
    assert nan_share <= 0.20
    assert share >= MEASURED_SHARE - 0.05
