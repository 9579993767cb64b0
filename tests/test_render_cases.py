"""The cases of tests/render_cases.py on the CPU checker alone: every case must reach, on the checker's statistics,
the branch it is there for: triangles of more than 64 pixels (which the product rasterises with a kernel of their
own), both classes contesting one pixel, near-plane drops, alpha discards, id ties, the mip levels of odd textures,
the clamp of the background equirect's fetch. A case that does not is a broken case; the GPU file
(tests/test_gpu_render_limits.py) then compares the device's image with the same checker image, value for value.

The canopy cases compare the device with oracle_canopy.h's cubemap, which has no counters of its own. The checker
configured as the rephotography renderer stands in for them: test_canopy_cases_are_the_oracle shows, for every canopy
case, that its image is the oracle's bit for bit, NaN -> 0 included. Both rasterise the same triangles in the same
order with the same depth key, so a pixel's winner, and with it every counter, is the same."""
import numpy as np
import pytest

from tests import render_cases as RC
from tests import smr_check

SMR = [n for n in RC.NAMES if RC.CASES[n]["renderer"] == "smr"]
CANOPY = [n for n in RC.NAMES if RC.CASES[n]["renderer"] == "canopy"]

# (tri_small, tri_big) of the checker, pinned: the scenes are analytic and the classification is integer arithmetic
# on fp32 window coordinates
PINNED = {
    "rig4_mag2x2_cube": (0, 6), "rig4_mag3x2_cube": (0, 20), "rig4_mag5x4_cube": (77, 97), "rig4_mag8x6_cube": (425, 22),
    "rig4_mag12x9_cube": (960, 0), "rig4_mag5x4_canopy": (77, 97), "mixed_mag2x2_cube": (0, 12),
    "real_mag2x2_cube": (0, 11), "mixed_mag12x9_cube": (1354, 0), "mixed_snap_fov20": (112, 186),
    "real_snap_fov20": (26, 101), "rig4_snap_fov20": (46, 90), "mixed_snap_fov150": (3462, 117),
    "mixed_snap_33x17": (252, 9), "mixed_snap_1x1": (12, 0),
}


def line(name, img, st):
    return ("%-34s covered %.3f | triangles <=64 px %5d, >64 px %5d | pixels won %5d / %5d | displaced %4d | id ties %3d | "
            "near drops %4d | alpha discards %5d | suspect %d | mip > 0 %5d" %
            (name, RC.covered(name, img).mean(), st["tri_small"], st["tri_big"], st["pix_small"], st["pix_big"],
             st["displaced"], st["id_ties"], st["near_drops"], st["alpha_discards"], st["suspect"], st["mip_above0"]))


@pytest.mark.parametrize("name", RC.NAMES)
def test_case_statistics(name):
    """every case: its statistics are consistent, and no inside fragment has a texture coordinate or derivative that
    is non-finite or beyond 2^31 (where the float -> int conversions of the filter would be undefined on the host and
    saturate on the device): the counter is 0 on every case, and is pinned there"""
    img, st = RC.checker(name)
    print(line(name, img, st))
    assert st["suspect"] == 0
    # pixels are counted per canopy: every covered pixel once at least, once per camera at most
    faces = RC.covered(name, RC.checker_faces(name))
    assert faces.sum() <= st["pix_small"] + st["pix_big"] <= faces.size * sum(RC.include_of(name))
    assert (st["pix_small"] + st["pix_big"] == 0) == (faces.sum() == 0)
    assert st["pix_big"] == 0 or st["tri_big"] > 0
    assert st["id_ties"] <= st["pix_small"] + st["pix_big"]
    if name in PINNED:
        assert (st["tri_small"], st["tri_big"]) == PINNED[name]


@pytest.mark.parametrize("name", CANOPY)
def test_canopy_cases_are_the_oracle(built, name):
    img, _ = RC.checker(name)
    assert smr_check.float_equal(img, RC.oracle(name)) == 0


def test_reach_per_rig_and_renderer():
    """per rig and renderer one case at least in which big triangles win more than 20 % of the covered pixels, small
    ones win some, a triangle of one class displaces a winner of the other, the near plane drops triangles and the
    filtered alpha discards fragments"""
    for rig in RC.RIGS:
        for renderer in ("smr", "canopy"):
            names = [n for n in RC.NAMES if RC.CASES[n]["rig"] == rig and RC.CASES[n]["renderer"] == renderer and
                     RC.reaches_both(RC.checker(n)[1])]
            print(rig, renderer, names)
            assert names, (rig, renderer)


def test_magnified_meshes():
    for rig in RC.RIGS:
        for suffix in ("cube", "eqr", "canopy"):
            st = {m: RC.checker("%s_mag%dx%d_%s" % ((rig,) + m + (suffix,)))[1] for m in RC.MAGNIFIED_MESHES}
            # 2 x 2: every triangle is big; 5 x 4 and 8 x 6: both classes win pixels in one view
            assert st[(2, 2)]["tri_small"] == 0 and st[(2, 2)]["tri_big"] > 0 and st[(2, 2)]["pix_big"] > 0
            for m in ((5, 4), (8, 6)):
                assert st[m]["pix_small"] > 0 and st[m]["pix_big"] > 0
            assert st[(12, 9)]["pix_small"] > 0
    # 12 x 9: the boundary from below
    assert RC.checker("rig4_mag12x9_cube")[1]["tri_big"] == 0 and RC.checker("mixed_mag12x9_cube")[1]["tri_big"] == 0
    # equal depth bits from two triangles, decided by the id
    assert RC.checker("rig4_mag5x4_cube")[1]["id_ties"] == 5
    assert RC.checker("rig4_mag5x4_canopy")[1]["id_ties"] == 5


def test_snapshots_and_closeups():
    for rig in RC.RIGS:
        for fov in (20, 150):
            img, st = RC.checker("%s_snap_fov%d" % (rig, fov))
            assert st["pix_big"] > 0 and st["pix_small"] > 0 and RC.covered("", img).mean() > 0.5
        assert RC.checker("%s_snap_fov20" % rig)[1]["pix_big"] > 4 * RC.checker("%s_snap_fov20" % rig)[1]["pix_small"]
        for view in ("origin", "cam1", "ahead1", "off"):
            for suffix in ("cube", "snap", "canopy"):
                st = RC.checker("%s_close_%s_%s" % (rig, view, suffix))[1]
                assert st["near_drops"] > 0 and (st["tri_big"] > 0 or view in ("origin", "cam1")), (rig, view, suffix)
        # the closeup's zero, infinite and negative disparities and its NaN hole reach the mesh
        disps = RC.case_scene("%s_close_origin_cube" % rig)["disps"]
        assert (disps[0] == 0).sum() == 1 and np.isinf(disps[0]).sum() == 1 and (disps[0] < 0).sum() == 1
        assert np.isnan(disps[2]).sum() == 4
        img, st = RC.checker("%s_snap_pose" % rig)
        assert st["pix_big"] > 0 and st["pix_small"] > 0


def test_size_edges():
    # E = 1 on the real rig covers the whole sphere: the equirect pins values; on rig4 uncovered faces poison every
    # tap of the seamless cube: the equirect pins NaN spreading, while the cube it is made from is half covered
    assert RC.covered("real_E1_eqr", RC.checker("real_E1_eqr")[0]).all()
    assert not RC.covered("rig4_E1_eqr", RC.checker("rig4_E1_eqr")[0]).any()
    assert RC.covered("rig4_E1_cube", RC.checker("rig4_E1_cube")[0]).mean() == 0.5
    for rig in ("real", "rig4"):
        for E in (2, 3, 17):
            cov = RC.covered("", RC.checker("%s_E%d_eqr" % (rig, E))[0]).mean()
            assert 0 < cov < 1, (rig, E, cov)
            assert RC.checker("%s_E%d_eqr" % (rig, E))[0].shape == (E, 2 * E, 4)
    # viewports that are no multiple of the 32 x 8 block; 33 x 17 is covered whole, with 9 big triangles
    img, st = RC.checker("mixed_snap_33x17")
    assert img.shape == (17, 33, 4) and RC.covered("", img).all() and st["tri_big"] == 9
    assert RC.checker("mixed_snap_1x1")[0].shape == (1, 1, 4) and RC.covered("", RC.checker("mixed_snap_1x1")[0]).all()
    assert RC.checker("mixed_snap_31x33")[0].shape == (33, 31, 4)
    # odd mip chains: a level above 0 is sampled; a 1 x 1 texture has no such level
    for name in RC.TEXTURE_MINIFIED:
        assert RC.checker(name)[1]["mip_above0"] > 0, name
    for E in (8, 2, 1):
        assert RC.checker("rig4_tex1x1_E%d" % E)[1]["mip_above0"] == 0
        assert RC.covered("", RC.checker("rig4_tex1x1_E%d" % E)[0]).any()
    # include masks change the image
    for kind in ("eqr", "snap"):
        one, allbut = RC.checker("rig4_include_one_%s" % kind)[0], RC.checker("rig4_include_allbut_%s" % kind)[0]
        assert smr_check.float_equal(one, allbut) > 0
    assert RC.covered("", RC.checker("rig4_include_one_eqr")[0]).sum() < RC.covered("", RC.checker("rig4_include_allbut_eqr")[0]).sum()
    # per-camera mesh sizes: both classes in one upload, and the order of the sizes matters
    st = RC.checker("rig4_sizes_cube")[1]
    assert st["tri_big"] > 0 and st["tri_small"] > 0
    assert smr_check.float_equal(RC.checker("rig4_sizes_cube")[0], RC.checker("rig4_sizes_rev_cube")[0]) > 0


def test_parameter_matrix():
    """weight x alpha_blend x zero_nans: every combination gives another image, on the magnified and the sub-pixel case"""
    for which in ("mag", "sub"):
        names = [n for n in RC.NAMES if n.startswith("rig4_matrix_%s_" % which)]
        assert len(names) == 8
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                assert smr_check.float_equal(RC.checker(a)[0], RC.checker(b)[0]) > 0, (a, b)
    assert RC.checker("rig4_matrix_mag_svd_blend_nan")[1]["tri_big"] == 97
    assert RC.checker("rig4_matrix_sub_svd_blend_nan")[1]["tri_big"] == 0


@pytest.mark.parametrize("name", sorted(RC.BACKGROUNDS))
def test_background_equirect_restatement(name):
    """chk_background_equirect: pixels of alpha 1 keep their value, every other pixel loses its NaN to the equirect,
    a NaN alpha takes a texel of the equirect as it is, and the poses of BACKGROUND_CLAMPED have rays whose texel the
    clamp decides"""
    fmt, view, equi, back = RC.background_case(name)
    fore, out, clamped = RC.background_checker(name)
    alpha = fore[..., 3]
    print("%s: %d pixels, alpha NaN %d, alpha 1 %d, clamp decided %d" %
          (name, alpha.size, np.isnan(alpha).sum(), (alpha == 1).sum(), clamped))
    assert np.isnan(alpha).any() and (alpha == 1).any()
    assert not np.isnan(out).any()
    assert smr_check.float_equal(out[alpha == 1], fore[alpha == 1]) == 0
    assert (clamped > 0) == (name in RC.BACKGROUND_CLAMPED)
    texels = {tuple(t) for t in equi.reshape(-1, 4)}
    if back is None:
        assert all(tuple(t) in texels for t in out[np.isnan(alpha)])
    else:  # alphaBlend made the NaN alphas 0.4 first: the result is fractional, between the two
        assert np.all(out[np.isnan(alpha)][:, 3] == np.float32(0.4) + (1 - np.float32(0.4)) * 1)
