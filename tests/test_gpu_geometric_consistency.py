"""The GeometricConsistency group of the C-ABI (derp_gc_*) against tests/geometric_ref.py, the numpy restatement of
DESIGN §8.6 on the oracle's camera: bit for bit, NaN masks included, for the int16 images, every stage download, the swept
depth, the cleaning and the whole frame."""
import numpy as np
import pytest

from tests import geometric_cases as K
from tests import geometric_ref as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(built):
    """one context per case, the frame uploaded"""
    from facebook360_dep_amd import derp

    made = {}

    def get(name):
        if name not in made:
            cams, sizes, _, _ = K.case(name)
            g = derp.Derp(cams)
            g.gc_upload(K.images(name), sizes)
            made[name] = g
        return made[name]

    yield get
    for g in made.values():
        g.close()


def check(got, want, what):
    bad = K.differing(got, want)
    print("%s: %d of %d values differ" % (what, bad, np.asarray(want).size))
    assert K.same(got, want), what


@pytest.mark.parametrize("name", K.CASES)
def test_images_and_slices(contexts, name):
    """k_gc_prepare (the resize kernel on four channels, then int16) and the slice table"""
    g = contexts(name)
    cams, sizes, step, slices0 = K.case(name)
    fr = K.frame(name)
    for cam in range(len(cams)):
        check(g.gc_image(cam), fr.I16[cam], "%s image %d" % (name, cam))
        want = G.slice_disparities(G.slice_count(fr.rig, cam, step))
        check(g.gc_slices(cam, step), want, "%s slices %d" % (name, cam))
    assert len(g.gc_slices(0, step)) == slices0
    if name == "rig4_mixed":
        assert len({len(g.gc_slices(cam, step)) for cam in range(4)}) > 1  # the slice count follows the camera's size
        assert (fr.I16[1][:, :, 3] == 0).any() and (fr.I16[1][:, :, 3] == 32767).any()  # the transparent hole


STAGE_CASES = [("rig4_32", 1, 0, 0, None), ("rig4_32", 1, 2, 18, None), ("rig4_32", 2, 3, 36, "patch"),
               ("rig4_25x19", 0, 1, 3, None), ("rig4_25x19", 3, 2, 6, "patch"), ("rig4_3x3", 1, 2, 0, None),
               ("rig4_3x3", 2, 1, 0, "patch"), ("rig4_mixed", 0, 1, 5, None), ("rig4_mixed", 2, 1, 4, "patch"),
               ("rig4_mixed", 3, 0, 2, None), ("rig2", 0, 1, 7, None), ("rig5", 4, 2, 3, "patch"),
               ("isolated", 2, 0, 8, None), ("isolated", 0, 1, 8, None)]


@pytest.mark.parametrize("name,dst,src,slice_index,clean", STAGE_CASES)
def test_stage_downloads(contexts, name, dst, src, slice_index, clean):
    """the sample image, average, averageOfSq and the slice's cost plane of one (destination, source, slice)"""
    g = contexts(name)
    fr = K.frame(name)
    step = K.case(name)[2]
    disparity = G.slice_disparities(G.slice_count(fr.rig, dst, step))[slice_index]
    maps = None if clean is None else K.occluding_clean(name, True)
    g.gc_set_clean(maps)
    got = g.gc_stage(dst, src, slice_index, step, use_clean=maps is not None, agree_fraction=0.75)
    image, average, average_of_sq, contributes, _ = fr.source_terms(dst, src, disparity, maps, 0.75)
    tag = "%s dst %d src %d slice %d" % (name, dst, src, slice_index)
    check(got["sample"], image, tag + " sample")
    check(got["average"], average, tag + " average")
    check(got["average_of_sq"], average_of_sq, tag + " averageOfSq")
    check(got["cost"], fr.cost(dst, disparity, maps, 0.75), tag + " cost")
    if name == "isolated":
        # nothing of camera 2 is seen by the others, nor theirs by it; cameras 0 and 1 overlap
        assert contributes.any() == (dst != 2)
    elif name != "rig4_3x3":
        assert contributes.any() and not contributes.all()
        if maps is not None:  # the occlusion test takes both branches
            plain = fr.sample(dst, src, disparity)
            assert (image[:, :, 3] != plain[:, :, 3]).any() and (image[:, :, 3] == 32767).any()


@pytest.mark.parametrize("name", K.CASES)
def test_sweep(contexts, name):
    g = contexts(name)
    cams, _, step, _ = K.case(name)
    finite = 0
    for dst in range(len(cams)):
        want = K.ref_sweep(name, dst)
        check(g.gc_sweep(dst, step), want, "%s sweep %d" % (name, dst))
        finite += int(np.isfinite(want).sum())
        assert np.isnan(want[0]).all() and np.isnan(want[:, -1]).all()
    # (3 x 3: every texel of a source lies within a texel of its border, so no sample is opaque and nothing has a cost;
    # what the mirrored halo computes there shows in the stage downloads)
    assert (finite > 0) == (name != "rig4_3x3")
    if name == "isolated":
        assert np.isnan(K.ref_sweep(name, 2)).all()  # no camera overlaps camera 2: every cost is NaN
        assert np.isfinite(K.ref_sweep(name, 0)).sum() > 400


@pytest.mark.parametrize("name,dst", [("rig4_32", 0), ("rig4_32", 3), ("rig4_25x19", 1), ("rig4_mixed", 2), ("rig4_3x3", 0)])
def test_slice_split_does_not_matter(contexts, name, dst):
    """the slice range in one part, in as many parts as the library allows, in two and as the library chooses: the
    same bytes (37 slices are no multiple of 2 or 64)"""
    g = contexts(name)
    step = K.case(name)[2]
    want = K.ref_sweep(name, dst)
    for split in (1, 64, 2, 5, 0):
        check(g.gc_sweep(dst, step, split=split), want, "%s sweep %d split %d" % (name, dst, split))


@pytest.mark.parametrize("agree", [0.75, 1.0])
@pytest.mark.parametrize("name", ["rig4_32", "rig4_25x19", "rig4_mixed", "rig5"])
def test_sweep_with_occlusion(contexts, name, agree):
    g = contexts(name)
    cams, _, step, _ = K.case(name)
    g.gc_set_clean(K.occluding_clean(name, True))
    changed = 0
    for dst in range(len(cams)):
        want = K.ref_sweep(name, dst, "patch", agree)
        check(g.gc_sweep(dst, step, use_clean=True, agree_fraction=agree), want, "%s occluded sweep %d" % (name, dst))
        # (on the CPU) the patch of small depths changes the restatement's own output, and so do the clean depths at all
        changed += K.differing(want, K.ref_sweep(name, dst, "holes", agree))
        assert K.differing(K.ref_sweep(name, dst, "holes", agree), K.ref_sweep(name, dst)) > 0 or name == "rig4_25x19"
    assert changed > 0
    g.gc_set_clean(K.occluding_clean(name, False))
    check(g.gc_sweep(0, step, use_clean=True, agree_fraction=agree), K.ref_sweep(name, 0, "holes", agree),
          "%s sweep 0 without the patch" % name)


RUN_CASES = [("rig4_32", 0.75, 2, False), ("rig4_32", 1.0, 1, True), ("rig4_32", 0.75, 2, True),
             ("rig4_25x19", 0.75, 2, True), ("rig4_3x3", 0.75, 1, False), ("rig4_mixed", 0.75, 2, False),
             ("rig4_mixed", 1.0, 1, True), ("rig2", 0.75, 1, True), ("rig5", 0.75, 1, False), ("isolated", 0.75, 1, True)]


@pytest.mark.parametrize("name,agree,passes,keep", RUN_CASES)
def test_run(contexts, name, agree, passes, keep):
    """processFrame: every map the tool dumps, and the depths it ends with"""
    g = contexts(name)
    cams, _, step, _ = K.case(name)
    want = K.ref_run(name, agree, passes, keep)
    g.gc_run(step, agree, passes, keep)
    for cam in range(len(cams)):
        check(g.gc_result("iffy", cam), want["iffy"][cam], "%s iffy %d" % (name, cam))
        for p in range(passes):
            check(g.gc_result("clean", cam, p), want["clean"][p][cam], "%s clean %d pass %d" % (name, cam, p))
            check(g.gc_result("depth", cam, p), want["depth"][p][cam], "%s depth %d pass %d" % (name, cam, p))
        check(g.gc_result("final", cam), want["final"][cam], "%s final %d" % (name, cam))
    if name == "rig4_32":
        # the cleaning rejects something and keeps something, and keep_clean restores what it kept
        rejected = sum(K.differing(want["clean"][0][c], want["iffy"][c]) for c in range(4))
        kept = sum(int(np.isfinite(want["clean"][0][c]).sum()) for c in range(4))
        assert rejected > 0 and kept > 0
        if keep:
            for c in range(4):
                m = np.isfinite(want["clean"][passes - 1][c])
                assert np.array_equal(want["final"][c][m], want["clean"][passes - 1][c][m])


def test_two_runs_give_the_same_bytes(contexts):
    g = contexts("rig4_32")
    step = K.case("rig4_32")[2]
    outs = []
    for _ in range(2):
        g.gc_run(step, 0.75, 2, True)
        outs.append([g.gc_result(kind, cam, p).tobytes() for cam in range(4) for kind, p in
                     (("iffy", 0), ("clean", 0), ("clean", 1), ("depth", 0), ("depth", 1), ("final", 0))])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("name", ["rig4_32", "rig4_mixed"])
def test_standalone_clean(contexts, name):
    """derp_gc_clean on depth maps that are not the sweep's: the scene's true depths. The maps agree with one another, so
    the cleaning rejects next to nothing: what it does reject lies on the silhouettes of the scene's planes, where the
    nearest sample of the other camera's map falls on the far side of the edge. The bound is the restatement's own
    count for these maps, written down here per camera (of 1024 pixels each at 32 x 32; of 1024, 475, 608 and 256 in the
    rig of mixed sizes, whose coarser maps have fatter silhouettes)."""
    bounds = {"rig4_32": (31, 18, 14, 14), "rig4_mixed": (42, 9, 24, 5)}[name]
    g = contexts(name)
    cams = K.case(name)[0]
    truth = K.truth_depths(name)
    for agree in (0.75, 1.0):
        want = G.clean(cams, truth, agree)
        got = g.gc_clean(truth, agree)
        for cam in range(len(cams)):
            check(got[cam], want[cam], "%s clean of truth, camera %d, agree %.2f" % (name, cam, agree))
            if agree == 0.75:
                rejected = int(np.isnan(want[cam]).sum())
                print("camera %d: %d of %d true depths rejected" % (cam, rejected, want[cam].size))
                assert rejected <= bounds[cam] and rejected <= 0.05 * want[cam].size
    # a patch of camera 1 pushed to a quarter of its true depth floats in front of what the others see: all rejected
    pushed = [d.copy() for d in truth]
    h, w = pushed[1].shape
    patch = (slice(h // 2 - 3, h // 2 + 3), slice(w // 2 - 3, w // 2 + 3))
    pushed[1][patch] *= np.float32(0.25)
    pushed[0][2, 3] = np.nan  # a NaN depth stays NaN, a NaN source depth rejects nothing
    want = G.clean(cams, pushed, 0.75)
    assert np.isnan(want[1][patch]).all() and np.isnan(want[0][2, 3])
    got = g.gc_clean(pushed, 0.75)
    for cam in range(len(cams)):
        check(got[cam], want[cam], "%s clean with the pushed patch, camera %d" % (name, cam))


def test_refusals(contexts):
    from facebook360_dep_amd import derp

    g = contexts("rig4_32")
    with pytest.raises(derp.DerpError, match="sliceCount"):
        g.gc_slices(0, 100.0)
    with pytest.raises(derp.DerpError, match="out of range"):
        g.gc_stage(0, 1, 37, K.case("rig4_32")[2])
    with pytest.raises(derp.DerpError, match="own sources"):
        g.gc_stage(1, 1, 0, K.case("rig4_32")[2])
    g.gc_set_clean(None)
    with pytest.raises(derp.DerpError, match="derp_gc_set_clean"):
        g.gc_sweep(0, 0.5, use_clean=True)
    cams = [dict(c) for c in K.case("rig2")[0]]
    for c in cams:
        c["origin"] = [6.0 * v for v in c["origin"]]  # 1.5 m from the origin
    far = derp.Derp(cams)
    try:
        far.gc_upload(K.images("rig2"), [(32, 32)] * 2)
        with pytest.raises(derp.DerpError, match="less than 1 m"):
            far.gc_sweep(0, 0.5)
        with pytest.raises(derp.DerpError, match="3 x 3 at least"):
            far.gc_upload(K.images("rig2"), [(32, 2)] * 2)
    finally:
        far.close()
    fresh = derp.Derp(K.case("rig2")[0])
    try:
        with pytest.raises(derp.DerpError, match="derp_gc_upload has not been called"):
            fresh.gc_sweep(0, 0.5)
    finally:
        fresh.close()
