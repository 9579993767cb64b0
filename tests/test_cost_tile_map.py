"""The tile order of the random-proposal / ping-pong launches (xcd_swizzle with K bands per XCD, blocks that walk N
tiles), computed on the host by the kernels' own arithmetic (derp_host_cost_tile_map): every tile of the level exactly
once, padding past the level only, and K = 1, N = 1 the order the kernels always had."""
import numpy as np
import pytest


def _tiles_of(w, h):
    """tiles_of (derp_capi.hip): 16x16 super-tiles padded to whole 4x4 squares, four 8x8 wave tiles each"""
    tx = ((w + 15) // 16 + 3) // 4 * 4
    ty = ((h + 15) // 16 + 3) // 4 * 4
    return tx * ty * 4


def _bench_level_tiles():
    from facebook360_dep_amd import synth

    n, res, widths = synth.config("cfg2")
    sizes = synth.level_sizes(res, res, widths)
    assert len(sizes) == 10
    return [_tiles_of(w, h) for w, h in sizes]


def _check(derp, tiles, bands, rot, per_block):
    m = derp.host_cost_tile_map(tiles, bands, rot, per_block)
    blocks = m.shape[0]
    assert m.shape == (blocks, per_block)
    assert blocks % (8 * bands) == 0 and blocks * per_block >= tiles
    assert blocks * per_block - tiles < 8 * bands * per_block, "more padding than one unit of the grid"
    flat = m.ravel()
    # a bijection of the padded range: every tile below `tiles` exactly once, everything else is padding past the level
    assert np.array_equal(np.sort(flat), np.arange(blocks * per_block)), (tiles, bands, rot, per_block)
    # a block's tiles are consecutive
    assert np.array_equal(m, m[:, :1] + np.arange(per_block)[None, :])
    if bands == 1 and per_block == 1:
        b = np.arange(blocks)
        per = (blocks + 7) // 8
        assert np.array_equal(flat, (((b & 7) + rot) & 7) * per + (b >> 3)), (tiles, rot)
    return m


def test_every_tile_exactly_once(built):
    from facebook360_dep_amd import derp

    for tiles in list(range(1, 601)) + _bench_level_tiles():
        for rot in range(8):
            for bands in (1, 2, 4):
                for per_block in (1, 2, 4):
                    _check(derp, tiles, bands, rot, per_block)


def test_an_xcd_owns_k_bands_spread_over_the_level(built):
    """block b runs on XCD b & 7: its tiles are K runs of tiles / (8 K), eight runs apart, walked one after another"""
    from facebook360_dep_amd import derp

    tiles = _bench_level_tiles()[0]
    assert tiles == 65536
    for bands in (1, 2, 4):
        run = tiles // (8 * bands)
        for rot in (0, 3):
            m = _check(derp, tiles, bands, rot, 1).ravel()
            for xcd in range(8):
                mine = m[xcd::8]
                runs = mine // run
                assert np.array_equal(runs, np.repeat(np.arange(bands) * 8 + ((xcd + rot) & 7), run))
                assert np.array_equal(mine % run, np.tile(np.arange(run), bands))


def test_bad_arguments_are_refused(built):
    from facebook360_dep_amd import derp

    for args in ((0, 1, 0, 1), (64, 3, 0, 1), (64, 8, 0, 1), (64, 1, 0, 3), (64, 1, 0, 8)):
        with pytest.raises(ValueError):
            derp.host_cost_tile_map(*args)
