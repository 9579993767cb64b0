"""What tests/test_gpu_conversion_limits.py leans on, stated on the references alone (tests/conversion_ref.py over the
oracle's camera) for the inputs of tests/conversion_cases.py: an equirect band that stays small, a cloud whose points
do cross the image edge when rounded, depth-boundary points that no other point hides, export cases that have something
to compact, and a cache that tells two rigs apart. A GPU test can then not pass for want of a case. No GPU."""
import numpy as np
import pytest

from tests import conversion_cases as CC
from tests import conversion_ref as ref


@pytest.fixture(scope="module", autouse=True)
def oracle():
    from oracle import oracle_lib as O

    O.build()
    return O


# ---------------------------------------------------------------- the cache of the circle test
def test_outside_cache_tells_rigs_apart():
    """Two rigs call their cameras cam0, cam1, ...: the real rig at 50 x 38 was once handed the mixed rig's counts. In
    either order, each camera gets its own."""
    for order in (("mixed", "real"), ("real", "mixed")):
        ref._outside.clear()
        got = {}
        for name in order:
            cams = CC.rig(name)[0]
            rig = ref.rescaled_rig(cams, 50, 38)
            got[name] = [int(ref.outside_image_circle(rig, cams, cam, 50, 38).sum()) for cam in range(4)]
        assert got["mixed"] == CC.OUTSIDE[("mixed", (50, 38))][:4], order
        assert got["real"] == CC.OUTSIDE[("real", (50, 38))][:4], order


# ---------------------------------------------------------------- subsampling
def test_mix32_is_the_murmur3_finaliser():
    """against Python integers, which do not wrap on their own; and the known fixed point and avalanche of fmix32"""
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)

    xs = np.array([0, 1, 2, 255, 256, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x9E3779B9, 123456789], dtype=np.uint32)
    assert [int(v) for v in ref.mix32(xs)] == [fmix(int(v)) for v in xs]
    assert int(ref.mix32(np.array([0], np.uint32))[0]) == 0 and fmix(1) == 0x514E28B7
    for cam in (0, 3, 5):
        for n in (2, 3, 7):
            keep = ref.subsample_keeps(cam, np.arange(5000), n)
            want = [fmix(p ^ fmix((cam + 0x9E3779B9) & 0xFFFFFFFF)) % n == 0 for p in range(5000)]
            assert keep.tolist() == want
    # the camera index matters: what a kernel handed the wrong one would get differs
    a, b = ref.subsample_keeps(0, np.arange(1900), 3), ref.subsample_keeps(3, np.arange(1900), 3)
    assert (a != b).sum() > 500


# ---------------------------------------------------------------- export
@pytest.mark.parametrize("name,size", CC.EXPORT_CASES)
def test_export_cases_have_something_to_compact(name, size):
    """The counts of pixels outside the image circle are the recorded ones (0 for the two default-FOV cameras), every
    case keeps something, and every case meant to exercise the compaction keeps strictly less than everything."""
    cams = CC.rig(name)[0]
    n = size[0] * size[1]
    for k, cam in enumerate(CC.cameras_of(name)):
        disp, color = CC.export_inputs(name, size, cam)
        for max_depth, clip in CC.EXPORT_SETTINGS:
            want, outside = ref.export_points(cams, cam, disp, color, max_depth, clip)
            assert outside == CC.OUTSIDE[(name, size)][k], (cam, outside)
            assert 0 < len(want) <= n
            if CC.compacts(outside, max_depth, clip):
                assert len(want) < n, (cam, max_depth, clip)
            else:
                assert cams[cam].get("fov") is None and len(want) == n  # the default FOV: nothing to drop
            for s in (2, 3, 7):
                sub, _ = ref.export_points(cams, cam, disp, color, max_depth, clip, subsample=s)
                assert 0 < len(sub) < len(want)
    if name == "mixed":
        assert CC.OUTSIDE[(name, size)][4:] == [0, 0]


def test_no_principal_changes_the_camera():
    """dropping "principal" moves the principal point (the file's are off-centre): cases on real_nopr are not copies"""
    a, b = CC.rig("real_nopr")
    for cam in CC.NO_PRINCIPAL:
        assert "principal" not in a[cam] and "principal" in b[cam]
        ra, rb = ref.rescaled_rig(a, 84, 54), ref.rescaled_rig(b, 84, 54)
        pa, pb = ra.state(cam)["principal"], rb.state(cam)["principal"]
        assert tuple(pa) == (42.0, 27.0) and np.abs(pa - pb).max() > 0.1


@pytest.mark.parametrize("size", CC.SCAN_SIZES + [CC.SCAN_WIDE])
def test_scan_inputs_have_empty_full_and_ragged_blocks(size):
    cams = CC.rig("mixed")[0]
    disp, color = CC.striped_inputs(size)
    n = size[0] * size[1]
    rig = ref.rescaled_rig(cams, *size)
    keep = ~ref.outside_image_circle(rig, cams, CC.SCAN_CAM, *size) & (disp.reshape(-1) == np.float32(0.5))
    assert int((~ref.outside_image_circle(rig, cams, CC.SCAN_CAM, *size)).sum()) == n - CC.SCAN_OUTSIDE[size]
    want, _ = ref.export_points(cams, CC.SCAN_CAM, disp, color, 3.0, True)
    assert len(want) == int(keep.sum())  # what is clipped is exactly the 10 m pixels
    blocks = -(-n // 256)
    per_block = np.add.reduceat(keep.astype(np.int64), np.arange(0, n, 256))
    assert len(per_block) == blocks == {(256, 1024): 1024, (256, 1025): 1025, (256, 2049): 2049, (1025, 256): 1025}[size]
    sizes = np.minimum(256, n - 256 * np.arange(blocks))
    empty, full = int((per_block == 0).sum()), int((per_block == sizes).sum())
    print("scan %dx%d: %d blocks, %d empty, %d full, %d ragged" % (size + (blocks, empty, full, blocks - empty - full)))
    assert empty > 100 and full > 20 and blocks - empty - full > 100
    # where rows are whole blocks, an empty block directly follows a full one (at the other widths a block that
    # straddles the two bands lies between them)
    e, f = per_block == 0, per_block == sizes
    assert (f[:-1] & e[1:]).any() == (size[0] % 256 == 0)
    # the blocks past the last multiple of 1024 keep points, so that a scan which dropped them would count short; in
    # the wide image they are the end of the last row, a corner outside the image circle
    if size != CC.SCAN_WIDE and blocks % 1024:
        assert per_block[blocks // 1024 * 1024:].sum() > 0


# ---------------------------------------------------------------- import
@pytest.mark.parametrize("name", CC.IMPORT_RIGS)
def test_clamp_cloud_crosses_the_edge(name):
    """At least 10 points that camera i sees land in [w - 0.5, w) (and [h - 0.5, h)): std::round sends them to w, the
    clamp back. Where the camera's image circle ends before an edge nothing can be seen there at all; those (camera,
    axis) pairs are listed in CC.UNREACHABLE and none of their points is seen. The random cloud alone gives the real
    rig not one such point in x."""
    cams = CC.rig(name)[0]
    pts, owner, axis = ref.clamp_cloud(cams, CC.IMPORT_SIZES)
    rig = ref.rescaled_rig(cams, CC.IMPORT_SIZES)
    unreachable = set()
    for i, (w, h) in enumerate(CC.IMPORT_SIZES):
        seen, pix = rig.sees(i, pts)
        for ax, edge in ((0, w), (1, h)):
            mine = (owner == i) & (axis == ax)
            assert mine.sum() == ref.EDGE_POINTS
            crossing = seen & mine & (pix[:, ax] >= edge - 0.5)
            if not seen[mine].any():
                unreachable.add((i, ax))
            else:
                assert crossing.sum() >= 10, (i, ax, int(crossing.sum()))
                assert (np.floor(pix[crossing, ax] + 0.5) == edge).all()  # rounds past the last pixel
    assert unreachable == CC.UNREACHABLE[name]
    if name == "real":
        rnd = ref.random_cloud(20000, seed=11)
        for i in (0, 2, 5):
            seen, pix = rig.sees(i, rnd)
            assert not (seen & (pix[:, 0] >= CC.IMPORT_SIZES[i][0] - 0.5)).any()


@pytest.mark.parametrize("name", CC.IMPORT_RIGS)
def test_boundary_points_decide_pixels(name):
    """In the sparse cloud every depth that is kept (min, max and their inner neighbours, as floats) is the value of
    at least three pixels, and the two one ulp outside are the value of none: a kernel that compared the fp64 norm, or
    used < for <=, would differ from the reference in those pixels."""
    cams = CC.rig(name)[0]
    pts, depths, kept = ref.boundary_cloud(cams, CC.MIN_DEPTH, CC.MAX_DEPTH)
    assert len(pts) == 36 and kept.sum() == 24
    norms = ref.norm3(pts)
    assert ((norms < CC.MIN_DEPTH) & kept).sum() >= 2 and ((norms > CC.MAX_DEPTH) & kept).sum() >= 2  # fp64 disagrees
    images = CC.import_reference(name, "sparse")
    for f, keep in ref.boundary_depths(CC.MIN_DEPTH, CC.MAX_DEPTH):
        hits = sum(int((im == np.float32(1) / f).sum()) for im in images)
        assert hits >= 3 if keep else hits == 0, (f, keep, hits)
    # the infinite rows and the zero vector leave no trace: the same images without them
    without = ref.import_points(cams, CC.import_clouds(name)["sparse"][:-len(ref.special_rows())], CC.IMPORT_SIZES,
                                CC.MIN_DEPTH, CC.MAX_DEPTH)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(images, without))


@pytest.mark.parametrize("name", CC.IMPORT_RIGS)
def test_import_reference_is_order_independent(name):
    for cloud in ("dense", "sparse"):
        pts = CC.import_clouds(name)[cloud]
        want = CC.import_reference(name, cloud)
        assert [im.shape for im in want] == [(h, w) for w, h in CC.IMPORT_SIZES]
        perm = CC.three_ways(pts)["permuted"][0]
        got = ref.import_points(CC.rig(name)[0], perm, CC.IMPORT_SIZES, CC.MIN_DEPTH, CC.MAX_DEPTH)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        assert sum(int((im > 0).sum()) for im in want) > (4000 if cloud == "dense" else 200)
    chunks = CC.three_ways(CC.import_clouds(name)["dense"])["chunks"]
    assert [len(c) for c in chunks[:3]] == [256, 0, 512] and len(chunks[3]) > 256


# ---------------------------------------------------------------- equirect mask
@pytest.mark.parametrize("name", ("mixed", "real", "real_nopr"))
def test_equirect_band_is_small(name):
    """Pixels whose fp64 equirect coordinate lies within 2e-4 px of an integer may go either way on the device; in
    every case of the GPU test they are at most 1 % of the image (measured: at most 0.27 %), and the mask is neither
    empty nor full."""
    worst = 0.0
    for cam in CC.cameras_of(name):
        for eqr_size in CC.EQUIRECT_SIZES:
            assert 0.1 < CC.equirect(eqr_size).mean() < 0.9
            for size in CC.EQUIRECT_TARGETS:
                for depth in CC.EQUIRECT_DEPTHS:
                    want, band = CC.equirect_reference(name, cam, eqr_size, size, depth)
                    assert want.shape == band.shape == (size[1], size[0])
                    assert band.sum() <= CC.BAND_CAP * band.size, (cam, eqr_size, size, depth, int(band.sum()))
                    assert 0.02 < want.mean() < 0.98, (cam, eqr_size, size, depth, want.mean())
                    worst = max(worst, float(band.mean()))
    print("equirect band, %s rig: at most %.2f %% of an image" % (name, 100 * worst))
