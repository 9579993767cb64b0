"""The conversion group of the C-ABI (derp_export_points, derp_points_*, derp_project_equirect_mask) against short
numpy restatements of the reference's loops (ExportPointCloud.cpp:67-137, ImportPointCloud.cpp:76-123,
ProjectEquirectsToCameras.cpp:94-125 with ImageUtil.cpp:127-140) on top of the oracle's camera: a Rig built from the
UN-normalised cameras and rescaled with Camera::rescale, as the three tools do. 3-vector norms use Eigen's unrolled
association a0 + (a1 + a2), like the oracle's camera."""
import math

import numpy as np
import pytest

from tests import conversion_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built):
    from facebook360_dep_amd import derp, synth

    rig = synth.make_rig(4, 64)
    g = derp.Derp(rig["cameras"])
    yield rig["cameras"], g
    g.close()


# ---------------------------------------------------------------- export
@pytest.fixture(scope="module")
def export_inputs():
    """(w, h, cam) -> disparity with one NaN pixel, one zero pixel and a patch beyond 3 m; float BGR colour"""
    from facebook360_dep_amd import synth

    cams = synth.make_rig(4, 64)["cameras"]
    out = {}
    for (w, h) in ((32, 32), (50, 38)):
        for cam in (0, 2):
            out[(w, h, cam)] = ref.export_inputs(cams[cam], w, h)
    return out


@pytest.mark.parametrize("size", [(32, 32), (50, 38)])
@pytest.mark.parametrize("cam", [0, 2])
@pytest.mark.parametrize("max_depth,clip", [(math.inf, False), (3.0, False), (3.0, True)])
def test_export_bit_for_bit(ctx, export_inputs, size, cam, max_depth, clip):
    cams, g = ctx
    w, h = size
    disp, color = export_inputs[(w, h, cam)]
    want, outside = ref.export_points(cams, cam, disp, color, max_depth, clip)
    got = g.export_points(cam, disp, color, max_depth=max_depth, clip=clip)
    print("export %dx%d cam %d max_depth %s clip %d: %d points, %d pixels outside the image circle"
          % (w, h, cam, max_depth, clip, len(got), outside))
    assert 0 < outside < w * h  # the compaction has something to do
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[:, :3]).any()  # the NaN disparity is kept (and, clamped, the zero one: inf * 0)
    if max_depth == math.inf:
        assert np.isinf(got[:, :3]).any()  # the zero disparity is kept
    else:
        depth = np.sqrt((got[:, :3].astype(np.float64) ** 2).sum(axis=1))
        assert (np.abs(depth[np.isfinite(depth)] - 3.0) < 1e-5).sum() >= (0 if clip else 9)  # the far patch, clamped
    if (w, h) == (32, 32):
        assert outside == 212  # (checked on the CPU for this rig: 848 of the four cameras' 4096 pixels)


def test_export_subsample(ctx, export_inputs):
    cams, g = ctx
    for cam in (0, 2):
        disp, color = export_inputs[(50, 38, cam)]
        full = g.export_points(cam, disp, color)
        a = g.export_points(cam, disp, color, subsample=4)
        b = g.export_points(cam, disp, color, subsample=4)
        assert a.tobytes() == b.tobytes()
        # exactly the rows that the hash of (camera index, pixel index) names, of the reference's output
        want, _ = ref.export_points(cams, cam, disp, color, math.inf, False, subsample=4)
        assert a.shape == want.shape and np.array_equal(a, want, equal_nan=True)
        other, _ = ref.export_points(cams, cam, disp, color, math.inf, False, cam_index=cam + 1, subsample=4)
        assert other.shape != want.shape or not np.array_equal(other, want, equal_nan=True)  # the camera index counts
        rows = [r.tobytes() for r in full]
        at = 0
        for r in a:  # an in-order subset of the subsample=1 output
            r = r.tobytes()
            while at < len(rows) and rows[at] != r:
                at += 1
            assert at < len(rows), "a subsampled point is not in the full output, or out of order"
            at += 1
        n = len(full)
        sigma = math.sqrt(n * 0.25 * 0.75)
        print("subsample=4 cam %d: kept %d of %d (expected %.1f, sigma %.1f)" % (cam, len(a), n, n / 4, sigma))
        assert abs(len(a) - n / 4) <= 5 * sigma


# ---------------------------------------------------------------- import
@pytest.fixture(scope="module")
def cloud():
    return ref.random_cloud(20000, seed=11)


MIN_DEPTH, MAX_DEPTH = 0.5, 6.0


def splat(g, n_cams, chunks):
    g.points_begin([(32, 32)] * n_cams)
    for c in chunks:
        g.points_splat(c, MIN_DEPTH, MAX_DEPTH)
    return [g.points_download(i) for i in range(n_cams)]


def test_import_bit_for_bit(ctx, cloud):
    cams, g = ctx
    want = ref.import_points(cams, cloud, [(32, 32)] * 4, MIN_DEPTH, MAX_DEPTH)
    one = splat(g, 4, [cloud])
    parts = splat(g, 4, [cloud[:7], cloud[7:71], cloud[71:]])
    hits = 0
    for i in range(4):
        nz = int((want[i] > 0).sum())
        hits += nz
        print("import cam %d: %d pixels hit, max disparity %.4f" % (i, nz, want[i].max()))
        assert one[i].tobytes() == want[i].tobytes(), i
        assert parts[i].tobytes() == want[i].tobytes(), i
    assert hits > 1000 and max(w.max() for w in want) <= np.float32(1 / MIN_DEPTH)
    # points_begin starts the images over
    again = splat(g, 4, [cloud[:100]])
    assert sum(int((a > 0).sum()) for a in again) < hits


def test_import_one_camera(built, cloud):
    from facebook360_dep_amd import derp, synth

    cams = synth.make_rig(4, 64)["cameras"][1:2]
    g = derp.Derp(cams)
    want = ref.import_points(cams, cloud, [(32, 32)], MIN_DEPTH, MAX_DEPTH)
    got = splat(g, 1, [cloud[:64], cloud[64:]])
    g.close()
    assert got[0].tobytes() == want[0].tobytes() and (want[0] > 0).sum() > 100


# ---------------------------------------------------------------- equirect mask -> camera
@pytest.mark.parametrize("depth", [1000.0, 1.0])
def test_equirect_mask(ctx, depth):
    cams, g = ctx
    eqr = ref.blob_mask(64, 32, seed=5)
    assert 0.1 < eqr.mean() < 0.9
    for cam in range(4):
        want, band = ref.project_equirect_mask(cams, cam, eqr, 32, 32, depth)
        got = g.project_equirect_mask(cam, eqr, 32, 32, depth)
        assert set(np.unique(got)) <= {0, 1}
        wrong = (got != want) & ~band
        print("equirect mask depth %g cam %d: %d set, %d band pixels, %d mismatches in the band, %d outside"
              % (depth, cam, int(got.sum()), int(band.sum()), int(((got != want) & band).sum()), int(wrong.sum())))
        assert wrong.sum() == 0
        # pixels whose fp64 equirect coordinate lies within 2e-4 px of an integer may go either way; at most 1 % of an
        # image are such
        assert band.sum() <= 0.01 * band.size, (cam, int(band.sum()))


# ---------------------------------------------------------------- errors
def test_errors(ctx, export_inputs):
    from facebook360_dep_amd import derp

    cams, g = ctx
    disp, color = export_inputs[(32, 32, 0)]
    n = len(g.export_points(0, disp, color))
    with pytest.raises(derp.DerpError, match="capacity"):
        g.export_points(0, disp, color, cap=n - 1)
    assert g.last_point_count == n  # count > cap still reports the count
    assert len(g.export_points(0, disp, color, cap=n)) == n
    with pytest.raises(derp.DerpError, match="camera index"):
        g.export_points(4, disp, color)
    with pytest.raises(derp.DerpError, match="camera index"):
        g.project_equirect_mask(-1, np.zeros((8, 16), np.uint8), 32, 32)
    g.points_begin([(32, 32)] * 4)
    with pytest.raises(derp.DerpError, match="camera index"):
        g.points_download(4)
    lib = derp.lib()
    import ctypes as C

    count = C.c_size_t()
    assert lib.derp_export_points(g.h, 0, None, 32, 32, None, C.c_double(1.0), 0, 1, None, C.c_size_t(0), C.byref(count)) != 0
    assert b"null" in lib.derp_last_error(g.h)
    assert lib.derp_points_begin(g.h, None, None) != 0
    assert lib.derp_points_splat(g.h, None, C.c_size_t(5), C.c_double(0.0), C.c_double(1.0)) != 0
    assert lib.derp_project_equirect_mask(g.h, 0, None, 16, 8, 32, 32, C.c_double(1.0), None) != 0
    with pytest.raises(derp.DerpError, match="subsample"):
        g.export_points(0, disp, color, subsample=0)
