"""k_reproject_bias_front (the default: maps front-loaded, gathers from 32-bit offsets, coefficients from an LDS table, the
border form behind a ballot) beside the kept one-cell-at-a-time kernel (DERP_REPROJECT_SERIAL=1): the padded colour and bias
tables, ring included, bit for bit for every (dst, src), on the first frame of a level and on a second frame at the same
level (which skips the tiles the first one found blank), at level sizes around the 32 x 32 tile; and against the oracle
under test_gpu_parity.test_level_tables' bounds."""
import os

import numpy as np
import pytest

from tests import common

pytestmark = pytest.mark.gpu

RES = 96
# w, h: a second tile of one column and less than one tile of rows; exact tiles; the smallest level_begin accepts; and
# 70 x 45 (three tile columns, two tile rows, both partial)
SIZES = [(70, 45), (64, 64), (33, 31), (3, 3)]
ORACLE_SIZES = [(70, 45), (33, 31)]
TILE = 32


def _rigs():
    from facebook360_dep_amd import synth

    return {"tiny": synth.make_rig(synth.config("tiny")[0], RES), "mixed": common.mixed_type_rig(RES)}


def _frame(n_cams, seed):
    """color[level][cam] u16 [h, w, 3]: a smooth ramp plus noise, so that neighbouring taps differ and the cubic
    overshoots both ends of the u16 range somewhere"""
    rng = np.random.default_rng([15, seed])
    color = []
    for w, h in SIZES:
        yy, xx = np.mgrid[0:h, 0:w]
        cams = []
        for s in range(n_cams):
            ramp = ((xx * (700 + 90 * s) + yy * (500 + 70 * s)) % 65536)[..., None]
            img = np.clip(ramp + rng.integers(-9000, 9001, size=(h, w, 3)), 0, 65535).astype(np.uint16)
            img[rng.random((h, w)) < 0.05] = 65535
            img[rng.random((h, w)) < 0.05] = 0
            cams.append(img)
        color.append(cams)
    return {"color": color}


def _context(cams, serial):
    from facebook360_dep_amd import derp

    saved = os.environ.pop("DERP_REPROJECT_SERIAL", None)
    try:
        if serial:
            os.environ["DERP_REPROJECT_SERIAL"] = "1"
        g = derp.Derp(cams, partial_coverage=1)  # the switch is read here
    finally:
        os.environ.pop("DERP_REPROJECT_SERIAL", None)
        if saved is not None:
            os.environ["DERP_REPROJECT_SERIAL"] = saved
    g.set_pyramid(SIZES, RES, RES)
    return g


def _tables(g, n, frames):
    """per level: [after frame 0, after frame 1 at the same level] of {(d, s): (color_padded, bias_padded)}, the
    blank-tile flags, and the inverse warps the kernel read"""
    g.upload_frame(frames[0])
    out = []
    for level in range(len(SIZES)):
        g.level_begin(level)
        pair = []
        for k, frame in enumerate(frames):
            if k:
                for s in range(n):
                    g.upload_color(level, s, frame["color"][level][s])
            g.stage("reproject_colors")
            pair.append({(d, s): (g.debug(d, s, "color_padded"), g.debug(d, s, "bias_padded"))
                         for d in range(n) for s in range(n) if s != d})
        seen = {(d, s): g.debug(d, s, "tile_seen") for d in range(n) for s in range(n) if s != d}
        # projWarpInv(d, s) is projWarp(s, d) when every camera is a destination
        maps = {(d, s): g.debug(s, d, "warp") for d in range(n) for s in range(n) if s != d}
        plain = {(d, s): (g.debug(d, s, "color"), g.debug(d, s, "bias")) for d in range(n) for s in range(n) if s != d}
        out.append(dict(tables=pair, seen=seen, maps=maps, plain=plain))
    return out


@pytest.fixture(scope="module")
def runs(built):
    res = {}
    for name, rig in _rigs().items():
        cams = rig["cameras"]
        n = len(cams)
        frames = [_frame(n, 1), _frame(n, 2)]
        got = {}
        for serial in (False, True):
            g = _context(cams, serial)
            try:
                got[serial] = _tables(g, n, frames)
            finally:
                g.close()
        res[name] = dict(rig=rig, n=n, frames=frames, pipe=got[False], serial=got[True])
    return res


def _classify(m, w, h):
    """what remap_cubic_u16 does at each map position: (valid, interior, border) as the kernels decide them"""
    def fixed(v):
        p = (v.astype(np.float32) * np.float32(32.0)).astype(np.float64)
        bad = ~(np.abs(p) < 2147483648.0)  # NaN too
        q = np.where(bad, 0.0, np.rint(np.where(bad, 0.0, p))).astype(np.int64)
        return np.where(bad, -2147483648, q)

    fsx, fsy = fixed(m[..., 0]), fixed(m[..., 1])
    sx, sy = np.clip(fsx >> 5, -32768, 32767) - 1, np.clip(fsy >> 5, -32768, 32767) - 1
    valid = ~np.isnan(m[..., 0])
    interior = valid & (sx >= 0) & (sx < max(w - 3, 0)) & (sy >= 0) & (sy < max(h - 3, 0))
    outside = (sx >= w) | (sx + 4 <= 0) | (sy >= h) | (sy + 4 <= 0)
    return valid, interior, valid & ~interior & ~outside


def test_cases_cover_nan_beside_valid_border_positions_and_blank_tiles(runs):
    mixed_tile = border = blank = interior_any = 0
    for run in runs.values():
        for level, (w, h) in enumerate(SIZES):
            for key, m in run["pipe"][level]["maps"].items():
                valid, interior, on_border = _classify(m, w, h)
                border += int(on_border.sum())
                interior_any += int(interior.sum())
                for ty in range(0, h, TILE):
                    for tx in range(0, w, TILE):
                        v = valid[ty:ty + TILE, tx:tx + TILE]
                        mixed_tile += int(v.any() and not v.all())
                blank += int((run["pipe"][level]["seen"][key] == 0).sum())
    print("tiles with NaN and valid maps: %d, border-path positions: %d, interior positions: %d, blank tiles: %d" %
          (mixed_tile, border, interior_any, blank))
    assert mixed_tile > 0 and border > 0 and blank > 0 and interior_any > 0


def test_blank_tile_flags_are_what_the_maps_say(runs):
    """a tile is seen iff a map position of the tile or its 1-pixel halo (reflected at the image edge) is valid"""
    for run in runs.values():
        for level, (w, h) in enumerate(SIZES):
            for key, m in run["pipe"][level]["maps"].items():
                valid = np.pad(~np.isnan(m[..., 0]), 1, mode="reflect")
                want = np.array([[valid[ty:ty + TILE + 2, tx:tx + TILE + 2].any() for tx in range(0, w, TILE)]
                                 for ty in range(0, h, TILE)], np.uint8)
                assert np.array_equal(run["pipe"][level]["seen"][key], want), (level, key)
                assert np.array_equal(run["serial"][level]["seen"][key], want), (level, key)


@pytest.mark.parametrize("rig", ["tiny", "mixed"])
def test_padded_tables_equal_the_kept_kernel_bit_for_bit(runs, rig):
    run = runs[rig]
    for level in range(len(SIZES)):
        for k in range(2):  # the first frame of the level, and a second one: skipBlank = 1
            new, old = run["pipe"][level]["tables"][k], run["serial"][level]["tables"][k]
            for key in new:
                for which in range(2):
                    bad = int((new[key][which] != old[key][which]).sum())
                    assert bad == 0, (rig, SIZES[level], "frame %d" % k, key, ("color", "bias")[which], bad)
        a, b = run["pipe"][level]["tables"]
        assert any((a[key][0] != b[key][0]).any() for key in a) or SIZES[level] == (3, 3)  # the second frame is another one


@pytest.mark.parametrize("rig", ["tiny", "mixed"])
def test_skipped_tiles_still_hold_zeros(runs, rig):
    run = runs[rig]
    for level, (w, h) in enumerate(SIZES):
        for key, seen in run["pipe"][level]["seen"].items():
            for which in range(2):
                t = run["pipe"][level]["tables"][1][key][which][2:-2, 2:-2]  # after the second frame, the interior
                for ty, tx in zip(*np.nonzero(seen == 0)):
                    assert not t[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].any(), (rig, level, key, ty, tx)


@pytest.mark.parametrize("rig", ["tiny", "mixed"])
def test_ring_replicates_the_edge_pixels(runs, rig):
    run = runs[rig]
    for level in range(len(SIZES)):
        for key, tabs in run["pipe"][level]["tables"][0].items():
            for t in tabs:
                assert np.array_equal(t, np.pad(t[2:-2, 2:-2], ((2, 2), (2, 2), (0, 0)), mode="edge")), (rig, level, key)


@pytest.mark.parametrize("rig", ["tiny", "mixed"])
def test_tables_against_the_oracle(runs, rig):
    run = runs[rig]
    total = [0, 0]
    for size in ORACLE_SIZES:
        level = SIZES.index(size)
        L = common.oracle_level(run["rig"], SIZES, run["frames"][1], level, RES, RES, partial_coverage=True)
        L.reproject_colors()
        for (d, s), (color, bias) in run["pipe"][level]["plain"].items():  # (the tables hold the second frame)
            c_bad = int((color != L.proj(d, s, "color")).sum())
            b_bad = int((bias != L.proj(d, s, "bias")).sum())
            total[0] += c_bad
            total[1] += b_bad
            # test_level_tables' bounds: last-ulp differences between the host's and the device's fp64 transcendentals
            assert c_bad <= 12 and b_bad <= 40, (rig, size, d, s, c_bad, b_bad)
    print("%s: colour / bias elements differing from the oracle: %s" % (rig, total))
