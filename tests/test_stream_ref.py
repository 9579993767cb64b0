"""tests/stream_ref.py, the restatement the GPU's mesh-stream renderer is held to bit for bit, against answers worked
out by hand: one triangle, the fill rule on shared edges through pixel centres, a triangle cut by the near plane against
an explicitly clipped polygon, the skipped triangles, the depth rule. CPU only."""
import numpy as np

from tests import stream_ref as R

F32 = np.float32


def clip_of(window_xyw, W, H):
    """clip coordinates (x, y, 0, w) whose window position is (x, y) at depth w; exact for the values used here"""
    p = np.asarray(window_xyw, dtype=np.float64)
    x, y, w = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(2 * x / W - 1) * w, (2 * y / H - 1) * w, np.zeros(len(p)), w], axis=1).astype(F32)


def coverage(clip, tris, W, H):
    count = np.zeros((H, W), dtype=int)
    for tri in tris:
        T = R.setup(clip, tri, W, H)
        if T is not None:
            count += R.cover(T, W, H)[0]
    return count


def test_one_triangle():
    """window (0,0) (8,0) (0,8) at w = 1 in an 8 x 8 view: a = -8, b = -8, c = 64 on the hypotenuse, so the 28 centres
    with i + j <= 6 are inside, the 8 centres on the hypotenuse (i + j = 7) belong to the other side (a < 0), 1 / w is
    exactly 1 and texVar = (px / 8, py / 8) exactly."""
    clip = clip_of([(0, 0, 1), (8, 0, 1), (0, 8, 1)], 8, 8)
    T = R.setup(clip, (0, 1, 2), 8, 8)
    a, b, c, det = T[:4]
    assert det == 64 and (a[0], b[0], c[0]) == (-8, -8, 64) and (a[1], b[1], c[1]) == (8, 0, 0) and (a[2], b[2], c[2]) == (0, 8, 0)
    inside, iw, _, _ = R.cover(T, 8, 8)
    jj, ii = np.mgrid[0:8, 0:8]
    assert np.array_equal(inside, ii + jj <= 6) and inside.sum() == 28
    assert (iw[inside] == 1).all()
    tex = np.array([[0, 0], [1, 0], [0, 1]], dtype=F32)
    winner, u, v = R.raster(clip, tex, [0, 1, 2], 8, 8)
    assert np.array_equal(winner >= 0, inside)
    assert np.array_equal(u[inside], ((ii + F32(0.5)) / F32(8))[inside]) and np.array_equal(v[inside], ((jj + F32(0.5)) / F32(8))[inside])
    # the other winding covers the same pixels
    assert np.array_equal(R.cover(R.setup(clip, (0, 2, 1), 8, 8), 8, 8)[0], inside)


def test_perspective_correct_interpolation():
    """u is linear in the 3-D triangle, not in the window: at window (2.5, 2.5) of (0,0,w=1) (8,0,w=4) (0,8,w=1) with
    u = 1 at the deep vertex, the barycentrics in the window are (3/8, 5/16, 5/16) and u = (l1 / 4) / (l0 + l1 / 4 + l2)"""
    clip = clip_of([(0, 0, 1), (8, 0, 4), (0, 8, 1)], 8, 8)
    tex = np.array([[0, 0], [1, 0], [0, 0]], dtype=F32)
    winner, u, _ = R.raster(clip, tex, [0, 1, 2], 8, 8)
    l0, l1, l2 = 3 / 8, 5 / 16, 5 / 16
    assert winner[2, 2] == 0 and abs(float(u[2, 2]) - (l1 / 4) / (l0 + l1 / 4 + l2)) < 1e-6
    T = R.setup(clip, (0, 1, 2), 8, 8)
    assert abs(float(R.cover(T, 8, 8)[1][2, 2]) - (l0 + l1 / 4 + l2)) < 1e-6  # 1 / w


def test_shared_edges_through_centres_own_every_centre_once():
    W = H = 8
    corners = [(0, 0, 1), (8, 0, 1), (8, 8, 1), (0, 8, 1)]
    clip = clip_of(corners, W, H)
    # the diagonals pass through the centres (i + 0.5, i + 0.5) and (i + 0.5, 7.5 - i); every winding of either triangle
    for tris in ([(0, 1, 2), (0, 2, 3)], [(0, 1, 2), (0, 3, 2)], [(2, 1, 0), (0, 2, 3)], [(1, 2, 3), (1, 3, 0)],
                 [(1, 2, 3), (3, 1, 0)], [(2, 0, 1), (3, 0, 2)]):
        assert (coverage(clip, tris, W, H) == 1).all(), tris
    # a vertical and a horizontal shared edge through centres (x = 4.5, y = 2.5), depths that differ along the edge
    clip = clip_of([(0, 0, 1), (4.5, 0, 2), (8, 0, 1), (0, 2.5, 2), (4.5, 2.5, 1), (8, 2.5, 3), (0, 8, 1), (4.5, 8, 2), (8, 8, 1)], W, H)
    quads = [(0, 1, 4, 3), (1, 2, 5, 4), (3, 4, 7, 6), (4, 5, 8, 7)]
    tris = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    assert (coverage(clip, tris, W, H) == 1).all()
    # a fan around a vertex on a pixel centre: that centre has one owner too
    clip = clip_of([(3.5, 3.5, 1), (0, 0, 1), (8, 0, 1), (8, 8, 1), (0, 8, 1)], W, H)
    assert (coverage(clip, [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 1)], W, H) == 1).all()


def clipped_coverage(clip, W, H, near=0.1):
    """float64: the triangle cut at w = near (Sutherland-Hodgman), projected, and which centres lie inside the polygon;
    also the least distance of a centre to the polygon's boundary lines"""
    p = clip.astype(np.float64)[:, [0, 1, 3]]
    poly = []
    for k in range(3):
        a, b = p[k], p[(k + 1) % 3]
        if a[2] >= near:
            poly.append(a)
        if (a[2] >= near) != (b[2] >= near):
            f = (near - a[2]) / (b[2] - a[2])
            poly.append(a + f * (b - a))
    win = np.array([((q[0] / q[2] + 1) / 2 * W, (q[1] / q[2] + 1) / 2 * H) for q in poly])
    jj, ii = np.mgrid[0:H, 0:W]
    px, py = ii + 0.5, jj + 0.5
    signs, least = [], np.inf
    for k in range(len(win)):
        (x0, y0), (x1, y1) = win[k], win[(k + 1) % len(win)]
        cross = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
        signs.append(cross)
        least = min(least, np.abs(cross / np.hypot(x1 - x0, y1 - y0)).min())
    signs = np.array(signs)
    return (signs > 0).all(axis=0) | (signs < 0).all(axis=0), least


def test_near_plane_cuts_the_triangle():
    """One vertex and two vertices behind the eye: the covered centres are those of the explicitly clipped polygon. No
    centre lies within 1e-4 pixels of a boundary line of the polygon, ten times what the fp32 edge functions can be off by
    here (2^-24 relative on terms of at most 1e4, over gradients of at least 10 per pixel: 1e-5 pixels), so the fp64 answer
    is the answer."""
    W, H = 64, 48
    cases = {
        "one_behind": np.array([[-0.9, -0.6, 0, 1.0], [0.8, -0.7, 0, 1.0], [0.3, 1.7, 0, -2.0]], dtype=F32),
        "two_behind": np.array([[0.07, -0.55, 0, 1.0], [-2.1, 1.3, 0, -0.7], [2.6, 1.9, 0, -1.3]], dtype=F32),
        "vertex_on_the_eye_plane": np.array([[-0.4, -0.8, 0, 2.0], [0.9, 0.1, 0, 1.5], [0.2, 0.6, 0, 0.0]], dtype=F32),
    }
    for name, clip in cases.items():
        want, least = clipped_coverage(clip, W, H)
        assert least > 1e-4, (name, least)
        assert 100 < want.sum() < W * H, (name, want.sum())
        for tri in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
            got, iw, _, _ = R.cover(R.setup(clip, tri, W, H), W, H)
            assert np.array_equal(got, want), (name, tri, int((got != want).sum()))
            assert (iw[got] > 0).all() and (F32(1) / iw[got] >= F32(0.1)).all()


def test_skipped_triangles():
    ok = clip_of([(0, 0, 1), (8, 0, 1), (0, 8, 1)], 8, 8)
    assert R.setup(ok, (0, 1, 2), 8, 8) is not None
    for tri in ((0, 0, 1), (0, 1, 1), (2, 1, 2)):  # two equal indices
        assert R.setup(ok, tri, 8, 8) is None
    behind = ok.copy()
    behind[:, 3] = [0.05, -1.0, 0.0999]  # wholly behind the near plane
    assert R.setup(behind, (0, 1, 2), 8, 8) is None
    for bad in (np.inf, -np.inf, np.nan):
        for column in range(4):
            p = ok.copy()
            p[1, column] = bad
            assert R.setup(p, (0, 1, 2), 8, 8) is None
    flat = clip_of([(0, 0, 1), (4, 4, 1), (8, 8, 1)], 8, 8)  # no area
    assert R.setup(flat, (0, 1, 2), 8, 8) is None
    huge = ok.copy() * F32(3e30)  # finite coordinates whose products are not
    assert R.setup(huge, (0, 1, 2), 8, 8) is None


def test_depth_rule():
    """GL_LESS on the eye depth; at equal depth the first triangle in the index buffer stays"""
    far = [(0, 0, 2), (8, 0, 2), (0, 8, 2)]
    near = [(0, 0, 1), (8, 0, 1), (0, 8, 1)]
    clip = clip_of(far + near + far, 8, 8)
    tex = np.zeros((9, 2), dtype=F32)
    covered = R.raster(clip, tex, [0, 1, 2], 8, 8)[0] >= 0
    for order, want in (([0, 1, 2, 3, 4, 5], 1), ([3, 4, 5, 0, 1, 2], 0), ([0, 1, 2, 6, 7, 8], 0), ([6, 7, 8, 0, 1, 2, 3, 4, 5], 2)):
        winner = R.raster(clip, tex, order, 8, 8)[0]
        assert (winner[covered] == want).all() and (winner[~covered] == -1).all(), order


def test_fragment_cone_and_quantiser():
    """cone 1 at texVar = (0.5, 0.5): weight exp(30) - 1; beyond radius 0.5 the floor 1 / 255, stored as GL_RGBA16"""
    tex = np.full((4, 4, 3), 0.25, dtype=F32)
    color, weight = R.fragment(tex, np.array([0.5, 1.25, 0.5], dtype=F32), np.array([0.5, 0.5, -3.0], dtype=F32))
    assert weight[0] == R.expf(F32(30)) - F32(1)
    floor = np.rint(F32(1) / F32(255) * F32(65535)) / F32(65535)
    assert floor == F32(257) / F32(65535) and weight[1] == weight[2] == R.expf(F32(30) * floor) - F32(1)
    assert (color == np.rint(F32(0.25) * F32(65535)) / F32(65535)).all()
    assert np.array_equal(R.unorm16(np.array([-1, np.nan, 2, 0.5], dtype=F32)), np.array([0, 0, 1, 32768 / 65535], dtype=F32))


def test_the_box_leaves_out_nothing_the_edge_functions_cover():
    """The box is part of the coverage rule, so this is the one guard that it cuts nothing off: the pixels covered inside
    the box are the pixels the edge functions cover anywhere in the view. Triangles that cross the near plane with one
    vertex up to 1000 km away, one behind the eye and one near, at 64 to 2048 pixels and 3072 x 1536; small triangles of a
    pixel or a few at any depth, where the edge functions' own rounding is largest against the triangle; thin distant ones.
    Every index order."""
    rng = np.random.default_rng(11)

    def held(clip, W, H):
        hit = 0
        for tri in ((0, 1, 2), (1, 0, 2), (2, 1, 0)):
            T = R.setup(clip, tri, W, H)
            if T is None:
                continue
            free = R.cover(T, W, H, boxed=False)[0]
            assert np.array_equal(R.cover(T, W, H)[0], free), (W, H, clip.tolist(), tri, R.box(T, W, H))
            hit += int(free.any())
        return hit

    for W, H, far, count in ((256, 256, 1e4, 300), (256, 256, 1e6, 300), (1024, 1024, 5.6e4, 40), (64, 48, 1e5, 300),
                             (2048, 2048, 1e3, 8), (2048, 2048, 1e5, 8), (3072, 1536, 1e4, 8)):
        hit = 0
        for _ in range(count):
            w = np.array([far * rng.uniform(0.2, 1.0), -rng.uniform(0.05, 50.0), rng.uniform(0.15, 5.0)])
            ndc = rng.uniform(-3.0, 3.0, size=(3, 2))
            hit += held(np.concatenate([ndc * w[:, None], np.zeros((3, 1)), w[:, None]], axis=1).astype(F32), W, H)
        assert hit > count // 2, (W, far, hit)  # the case is not vacuous
    for W, H, count in ((2048, 2048, 12), (3072, 1536, 12), (130, 3, 200)):
        hit = 0
        for k in range(count):
            depth = 10.0 ** rng.uniform(-0.5, 4.0)
            centre = rng.uniform(-1.0, 1.0, size=2)
            if k % 2:  # thin and distant: a long edge, a fraction of a pixel wide
                along = rng.normal(size=2)
                along *= rng.uniform(0.05, 0.5) / np.linalg.norm(along)
                ndc = centre + np.array([-along, along, along[::-1] * [1, -1] * rng.uniform(0.5, 4.0) / max(W, H)])
            else:  # a pixel or a few across
                ndc = centre + rng.uniform(-1.0, 1.0, size=(3, 2)) * rng.uniform(1.0, 6.0) / min(W, H)
            w = depth * rng.uniform(0.98, 1.02, size=3)
            hit += held(np.concatenate([ndc * w[:, None], np.zeros((3, 1)), w[:, None]], axis=1).astype(F32), W, H)
        assert hit > count // 2, (W, H, hit)
