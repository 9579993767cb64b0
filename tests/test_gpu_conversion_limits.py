"""The conversion group's kernels (derp_points.h: export, import, equirect mask) off the square FTHETA rig and at their
own edges, bit for bit against tests/conversion_ref.py as tests/test_gpu_conversion.py does: the four camera types with
and without an explicit FOV (common.mixed_type_rig), the reference's real calibration with and without a principal
point (common.real_rig), image sizes of another aspect than the sensor's, the strided block scan, the exact
subsampling hash, empty and tiny exports, per-camera import sizes, points that round past the image edge, depths at
the limits, and clouds fed whole, in chunks and shuffled. What these cases need of their inputs (that they compact,
cross the edge, decide pixels, keep the equirect band small) is asserted on the CPU in tests/test_conversion_ref.py."""
import numpy as np
import pytest

from tests import conversion_cases as CC
from tests import conversion_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(built):
    from facebook360_dep_amd import derp

    made = {name: derp.Derp(CC.rig(name)[0]) for name in ("mixed", "real", "real_nopr")}
    yield made
    for g in made.values():
        g.close()


def same_points(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)


# ---------------------------------------------------------------- export
@pytest.mark.parametrize("max_depth,clip", CC.EXPORT_SETTINGS)
@pytest.mark.parametrize("name,size", CC.EXPORT_CASES)
def test_export_rigs_bit_for_bit(ctxs, name, size, max_depth, clip):
    cams, g = CC.rig(name)[0], ctxs[name]
    compacted = 0
    for k, cam in enumerate(CC.cameras_of(name)):
        disp, color = CC.export_inputs(name, size, cam)
        want, outside = ref.export_points(cams, cam, disp, color, max_depth, clip)
        got = g.export_points(cam, disp, color, max_depth=max_depth, clip=clip)
        print("export %s %dx%d cam %d max_depth %s clip %d: %d points of %d pixels, %d outside the image circle"
              % (name, size[0], size[1], cam, max_depth, clip, len(got), disp.size, outside))
        assert outside == CC.OUTSIDE[(name, size)][k]
        assert got.shape == want.shape, (cam, got.shape, want.shape)
        assert same_points(got, want), (cam, int((got != want).sum()))
        assert g.last_point_count == len(want)
        compacted += 0 < len(want) < disp.size
    assert compacted >= (len(CC.cameras_of(name)) if clip and max_depth == 3.0 else 2)


@pytest.mark.parametrize("subsample", [2, 3, 7])
@pytest.mark.parametrize("cam", [0, 3])
@pytest.mark.parametrize("name,size", [("mixed", (50, 38)), ("real_nopr", (84, 54))])
def test_export_subsample_exact(ctxs, name, size, cam, subsample):
    """the kept rows are the reference's rows at the pixels that mix32 of (camera index, pixel index) names"""
    cams, g = CC.rig(name)[0], ctxs[name]
    disp, color = CC.export_inputs(name, size, cam)
    full, _ = ref.export_points(cams, cam, disp, color, 3.0, False)
    want, _ = ref.export_points(cams, cam, disp, color, 3.0, False, subsample=subsample)
    got = g.export_points(cam, disp, color, max_depth=3.0, subsample=subsample)
    print("subsample %d, %s cam %d: %d of %d points" % (subsample, name, cam, len(got), len(full)))
    assert 0 < len(want) < len(full)
    assert same_points(got, want), (got.shape, want.shape)
    for wrong in (0, 3):  # what the other camera index would keep is something else
        if wrong != cam:
            other, _ = ref.export_points(cams, cam, disp, color, 3.0, False, cam_index=wrong, subsample=subsample)
            assert not same_points(other, want)


@pytest.mark.parametrize("size,subsample", [(s, 1) for s in CC.SCAN_SIZES + [CC.SCAN_WIDE]] + [((256, 1025), 3)])
def test_export_block_scan(ctxs, size, subsample):
    """1024, 1025 and 2049 blocks of 256 pixels: k_scan_block_counts with one count per thread and every thread busy,
    two per thread with the last threads idle, and three; empty, full and ragged blocks among them, and the last
    block keeps points. 256 x 1025 is 1025 x 256 pixels stood upright (see CC.SCAN_SIZES), run both ways."""
    cams, g = CC.rig("mixed")[0], ctxs["mixed"]
    disp, color = CC.striped_inputs(size)
    want, outside = ref.export_points(cams, CC.SCAN_CAM, disp, color, 3.0, True, subsample=subsample)
    got = g.export_points(CC.SCAN_CAM, disp, color, max_depth=3.0, clip=True, subsample=subsample)
    print("block scan %dx%d subsample %d: %d points of %d pixels, %d outside the image circle"
          % (size[0], size[1], subsample, len(got), disp.size, outside))
    assert outside == CC.SCAN_OUTSIDE[size] and 0 < len(want) < disp.size - outside
    assert got.shape == want.shape, (got.shape, want.shape)
    assert same_points(got, want)


def tiny_inputs(size):
    w, h = size
    n = w * h
    rng = np.random.default_rng(n)
    disp = np.where(np.arange(n) % 3 == 1, np.float32(0.1), np.float32(0.5)).reshape(h, w)  # every third beyond 3 m
    return disp, rng.random((h, w, 3), dtype=np.float32)


@pytest.mark.parametrize("cam", CC.TINY_CAMS)
@pytest.mark.parametrize("size", CC.TINY_SIZES)
def test_export_tiny(ctxs, size, cam):
    """one pixel; one block short by a pixel, exactly full, and one pixel into a second block; a column"""
    cams, g = CC.rig("mixed")[0], ctxs["mixed"]
    disp, color = tiny_inputs(size)
    for clip in (False, True):
        for subsample in (1, 2):
            want, _ = ref.export_points(cams, cam, disp, color, 3.0, clip, subsample=subsample)
            got = g.export_points(cam, disp, color, max_depth=3.0, clip=clip, subsample=subsample)
            assert same_points(got, want), (clip, subsample, got.shape, want.shape)
    want, _ = ref.export_points(cams, cam, disp, color, 3.0, True)
    assert len(want) == disp.size - len(range(1, disp.size, 3))  # nothing is outside the circle: clip does the work


@pytest.mark.parametrize("size", [(1, 1), (50, 38), (257, 3)])
def test_export_everything_clipped(ctxs, size):
    """no point survives: count 0, shape (0, 6), no error; and the context goes on working"""
    cams, g = CC.rig("mixed")[0], ctxs["mixed"]
    w, h = size
    disp = np.full((h, w), 0.1, np.float32)
    color = np.zeros((h, w, 3), np.float32)
    for cam in (1, 4):
        want, _ = ref.export_points(cams, cam, disp, color, 3.0, True)
        got = g.export_points(cam, disp, color, max_depth=3.0, clip=True)
        assert want.shape == (0, 6) and got.shape == (0, 6) and got.dtype == np.float32
        assert g.last_point_count == 0
        assert len(g.export_points(cam, disp, color, max_depth=3.0, clip=True, cap=0)) == 0
        kept = g.export_points(cam, disp, color, max_depth=3.0, clip=False)
        want, _ = ref.export_points(cams, cam, disp, color, 3.0, False)
        assert len(want) > 0 and same_points(kept, want)


# ---------------------------------------------------------------- import
def splat(g, chunks):
    g.points_begin(CC.IMPORT_SIZES)
    for c in chunks:
        g.points_splat(c, CC.MIN_DEPTH, CC.MAX_DEPTH)
    return [g.points_download(i) for i in range(len(CC.IMPORT_SIZES))]


@pytest.mark.parametrize("cloud", ["dense", "sparse"])
@pytest.mark.parametrize("name", CC.IMPORT_RIGS)
def test_import_sizes_edges_and_order(ctxs, name, cloud):
    """a size of its own per camera (offset, width and height all differ, one image is a single pixel); the cloud
    whole, as chunks of 256, 0, 512 and the rest, and shuffled: the reference's bytes each time"""
    g = ctxs[name]
    want = CC.import_reference(name, cloud)
    pts = CC.import_clouds(name)[cloud]
    for way, chunks in CC.three_ways(pts).items():
        got = splat(g, chunks)
        for i, (w, h) in enumerate(CC.IMPORT_SIZES):
            assert got[i].shape == (h, w)
            diff = int((got[i].view(np.uint32) != want[i].view(np.uint32)).sum())
            assert diff == 0, (way, i, diff)
    print("import %s %s: pixels hit per camera %s" % (name, cloud, [int((im > 0).sum()) for im in want]))
    assert all((im > 0).any() for im in want)


@pytest.mark.parametrize("name", CC.IMPORT_RIGS)
def test_import_one_point(ctxs, name):
    cams, g = CC.rig(name)[0], ctxs[name]
    pts = ref.clamp_cloud(cams, CC.IMPORT_SIZES)[0]
    for k in (len(pts) - 1, len(pts) - 2 * ref.EDGE_POINTS):  # camera 5's bottom edge and right edge
        one = pts[k:k + 1]
        want = ref.import_points(cams, one, CC.IMPORT_SIZES, CC.MIN_DEPTH, CC.MAX_DEPTH)
        got = splat(g, [one])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        assert sum(int((im > 0).sum()) for im in want) >= 1


# ---------------------------------------------------------------- equirect mask -> camera
@pytest.mark.parametrize("depth", CC.EQUIRECT_DEPTHS)
@pytest.mark.parametrize("size", CC.EQUIRECT_TARGETS)
@pytest.mark.parametrize("eqr_size", CC.EQUIRECT_SIZES)
@pytest.mark.parametrize("name", ("mixed", "real", "real_nopr"))
def test_equirect_mask_rigs(ctxs, name, eqr_size, size, depth):
    g = ctxs[name]
    eqr = CC.equirect(eqr_size)
    for cam in CC.cameras_of(name):
        want, band = CC.equirect_reference(name, cam, eqr_size, size, depth)
        got = g.project_equirect_mask(cam, eqr, size[0], size[1], depth)
        assert got.shape == want.shape and set(np.unique(got)) <= {0, 1}
        wrong = (got != want) & ~band
        print("equirect %dx%d -> %s cam %d %dx%d depth %g: %d set, %d band pixels, %d mismatches in the band, %d outside"
              % (eqr_size + (name, cam) + size + (depth, int(got.sum()), int(band.sum()),
                                                  int(((got != want) & band).sum()), int(wrong.sum()))))
        assert wrong.sum() == 0
        assert band.sum() <= CC.BAND_CAP * band.size, (cam, int(band.sum()))
