"""k_sweep_overlaps, k_sweep_equirect and k_sweep_equirect_bounds against the restatement (tests/sweep_ref.py), bit for
bit: 0 differing values, NaN masks equal. The cases and what each must contain: tests/sweep_cases.py, checked on the
restatement by tests/test_sweep_ref.py."""
import numpy as np
import pytest

from facebook360_dep_amd import derp
from tests import sweep_cases as K
from tests import sweep_ref as R

pytestmark = pytest.mark.gpu

_ctx = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_last_context():
    yield
    for g in _ctx.values():
        g.close()
    _ctx.clear()


def _uploaded(kind, name):
    """one context per case, shared by the tests of that case"""
    key = (kind, name)
    if key not in _ctx:
        cams, images, res = (K.overlap_case(name) if kind == "overlaps" else K.equirect_case(name))[:3]
        for old in _ctx.values():  # (a context per case at a time)
            old.close()
        _ctx.clear()
        g = derp.Derp(cams)
        g.sweep_upload(images, res)
        _ctx[key] = g
    return _ctx[key]


@pytest.mark.parametrize("name", sorted(K.OVERLAP_CASES))
def test_overlaps(name):
    g = _uploaded("overlaps", name)
    disp, dsts = K.overlap_case(name)[3:5]
    for dst in dsts:
        ref = K.overlap_ref(name, dst)[0]
        got = g.sweep_overlaps(dst, disp)
        assert got.shape == ref.shape
        print(name, dst, "float: differing", K.differing(got, ref), "of", ref.size)
        assert K.differing(got, ref) == 0 and K.same(got, ref)
        got8 = g.sweep_overlaps(dst, disp, u8=True)
        print(name, dst, "u8: differing", K.differing(got8, R.to_u8(ref)))
        assert K.same(got8, R.to_u8(ref))


def test_overlaps_do_not_depend_on_the_length_of_the_list():
    """a depth gives the same image alone, in a list of 7 and in a list of 50 (other runs, other parts of the grid)"""
    g = _uploaded("overlaps", "rig4_25x19")
    disp = K.overlap_case("rig4_25x19")[3]
    whole = g.sweep_overlaps(3, disp)
    assert K.same(g.sweep_overlaps(3, disp[:7]), whole[:7])
    assert K.same(g.sweep_overlaps(3, disp[49:]), whole[49:])
    assert K.same(g.sweep_overlaps(3, disp[13:20]), whole[13:20])


@pytest.mark.parametrize("name", sorted(K.EQUIRECT_CASES))
def test_equirect(name):
    g = _uploaded("equirect", name)
    _, _, _, (W, H), depths, black = K.equirect_case(name)
    ref = K.equirect_ref(name)[0]
    got = g.sweep_equirect(W, H, depths, black_bg=black)
    print(name, "float: differing", K.differing(got, ref), "of", ref.size)
    assert K.differing(got, ref) == 0 and K.same(got, ref)
    got8 = g.sweep_equirect(W, H, depths, black_bg=black, u8=True)
    assert K.same(got8, R.to_u8(ref))
    # the other background changes the uncovered pixels alone
    other = g.sweep_equirect(W, H, depths[:1], black_bg=not black)
    rig = K.equirect_rigged(name)
    assert K.same(other[0], rig.equirect(W, H, depths[0], black_bg=not black))


@pytest.mark.parametrize("name", K.BOUNDS_CASES)
def test_equirect_bounds_and_crop(name):
    g = _uploaded("equirect", name)
    _, _, _, (W, H), _, black = K.equirect_case(name)
    rig = K.equirect_rigged(name)
    for depth in K.BOUNDS_DEPTHS:
        bounds = g.sweep_equirect_bounds(W, H, depth)
        assert bounds == rig.equirect_bounds(W, H, depth), depth
        new_w = derp.sweep_crop_size(H, bounds)
        assert new_w == R.crop_size(H, bounds)
        got = g.sweep_equirect(W, H, [depth], window=bounds, out_size=(new_w, H), black_bg=black)
        ref = rig.equirect(W, H, depth, window=bounds, out_size=(new_w, H), black_bg=black)
        print(name, depth, bounds, new_w, "differing", K.differing(got[0], ref))
        assert got.shape == (1, H, new_w, 4) and K.same(got[0], ref)


def test_equirect_bounds_where_nothing_is_seen():
    """the isolated rig at 5 cm: every point lies inside the rig, behind all three cameras"""
    g = _uploaded("equirect", "isolated_64x32")
    rig = K.equirect_rigged("isolated_64x32")
    assert rig.equirect_bounds(64, 32, 0.05) == (64, 0, 32, 0)
    bounds = g.sweep_equirect_bounds(64, 32, 0.05)
    assert bounds == (64, 0, 32, 0)
    with pytest.raises(derp.DerpError, match="crop_equirect"):
        derp.sweep_crop_size(32, bounds)


def test_refusals():
    cams, images, res = K.overlap_case("rig2")[:3]
    g = derp.Derp(cams)
    with pytest.raises(derp.DerpError, match="derp_sweep_upload has not been called"):
        g.sweep_equirect(8, 4, [1.0])
    with pytest.raises(derp.DerpError, match="resolution"):
        g.sweep_upload(images, [(32.0, 0.0), (32.0, 32.0)])
    g.sweep_upload(images, res)
    with pytest.raises(derp.DerpError, match="bad camera index"):
        g.sweep_overlaps(2, [0.5])
    with pytest.raises(derp.DerpError, match="empty list"):
        g.sweep_overlaps(0, [])
    with pytest.raises(derp.DerpError, match="empty window"):
        g.sweep_equirect(8, 4, [1.0], window=(3, 3, 0, 2), out_size=(4, 4))
    with pytest.raises(derp.DerpError, match="without a window"):
        g.sweep_equirect(8, 4, [1.0], out_size=(4, 4))
    g.close()
