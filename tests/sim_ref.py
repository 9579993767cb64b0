"""numpy restatement of RigSimulator (source/rig/RigSimulator.cpp), independent of the library's C++: the scene builders
and the sphere tree with the C library's rand() through ctypes, and the tracer on float32 arrays, vectorised over rays.

The tracer walks the same pre-order flat tree with the same sphere tests (rejecting a grazing ray at a sphere is part of
the result): the nodes are visited in index order, every ray carries the index of the node it visits next, a sphere hit
moves it to the next node, a miss to the node's skip link. Links only point forward, so one pass over the nodes is the
walk. A hit is kept only when strictly nearer, in leaf and triangle order.

Widths (float / double) follow the stated choices of DESIGN section 8.5; every float32 product and sum is a separate
numpy operation, so nothing is fused."""
import ctypes
import math

import numpy as np

F = np.float32
D = np.float64
FLT_MAX = np.finfo(np.float32).max
RAND_MAX = 2147483647
LIGHT = np.array([2.0, 1.0, 5.2], np.float32)

_libc = ctypes.CDLL(None)
_libc.rand.restype = ctypes.c_int
_libc.srand.argtypes = [ctypes.c_uint]


def srand(seed):
    _libc.srand(seed)


def randf0to1():
    return F(_libc.rand()) / F(RAND_MAX)


# Ken Perlin, "Improved Noise" (2002): the reference implementation's permutation
PERLIN = [151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240,
          21, 10, 23, 190, 6, 148, 247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88,
          237, 149, 56, 87, 174, 20, 125, 136, 171, 168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231,
          83, 111, 229, 122, 60, 211, 133, 230, 220, 105, 92, 41, 55, 46, 245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1,
          216, 80, 73, 209, 76, 132, 187, 208, 89, 18, 169, 200, 196, 135, 130, 116, 188, 159, 86, 164, 100, 109, 198,
          173, 186, 3, 64, 52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118, 126, 255, 82, 85, 212, 207, 206, 59, 227,
          47, 16, 58, 17, 182, 189, 28, 42, 223, 183, 170, 213, 119, 248, 152, 2, 44, 154, 163, 70, 221, 153, 101, 155,
          167, 43, 172, 9, 129, 22, 39, 253, 19, 98, 108, 110, 79, 113, 224, 232, 178, 185, 112, 104, 218, 246, 97, 228,
          251, 34, 242, 193, 238, 210, 144, 12, 191, 179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31,
          181, 199, 106, 157, 184, 84, 204, 176, 115, 121, 50, 45, 127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29,
          24, 72, 243, 141, 128, 195, 78, 66, 215, 61, 156, 180]
PERLIN512 = np.array(PERLIN + PERLIN, np.int64)


# ---------------------------------------------------------------- cv::Vec3f arithmetic on [..., 3] float32 arrays
def v3(x, y, z):
    return np.array([x, y, z], np.float32)


def dot(a, b):
    s = F(0) + a[..., 0] * b[..., 0]
    s = s + a[..., 1] * b[..., 1]
    return s + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(np.float32)


def norm(a):
    a = a.astype(np.float64)
    s = 0.0 + a[..., 0] * a[..., 0]
    s = s + a[..., 1] * a[..., 1]
    s = s + a[..., 2] * a[..., 2]
    return np.sqrt(s)


def div_float(a, alpha):
    with np.errstate(all="ignore"):
        ialpha = F(1) / np.asarray(alpha, np.float32)
        return (a * ialpha[..., None] if np.ndim(ialpha) else a * ialpha).astype(np.float32)


def div_double(a, alpha):
    with np.errstate(all="ignore"):
        ialpha = 1.0 / np.asarray(alpha, np.float64)
        return (a.astype(np.float64) * (ialpha[..., None] if np.ndim(ialpha) else ialpha)).astype(np.float32)


# ---------------------------------------------------------------- scene
class Scene:
    def __init__(self):
        self.tri = []  # dicts of float32 [3]: v0 v1 v2 e1 e2 normal color
        self.nodes = []  # dicts: center, radius, skip, first, count, n_children
        self.leaf = []

    def add(self, v0, v1, v2, color):
        v0, v1, v2, color = (np.asarray(a, np.float32) for a in (v0, v1, v2, color))
        e1, e2 = v1 - v0, v2 - v0
        n = cross(e1, e2)
        n = div_double(n, norm(n))
        self.tri.append(dict(v0=v0, v1=v1, v2=v2, e1=e1, e2=e2, normal=n, color=color))

    def field(self, name):
        return np.array([t[name] for t in self.tri], np.float32).reshape(-1, 3)


def icosa_tables():
    phi = (1.0 + math.sqrt(5.0)) / 2.0
    length = math.sqrt(1.0 + phi * phi)
    X, Z, O = F(1.0 / length), F(phi / length), F(0)
    vert = [(-X, O, Z), (X, O, Z), (-X, O, -Z), (X, O, -Z), (O, Z, X), (O, Z, -X), (O, -Z, X), (O, -Z, -X), (Z, X, O),
            (-Z, X, O), (Z, -X, O), (-Z, -X, O)]
    # the face list of RigSimulator.cpp:139-142
    faces = [(1, 4, 0), (4, 9, 0), (4, 5, 9), (8, 5, 4), (1, 8, 4), (1, 10, 8), (10, 3, 8), (8, 3, 5), (3, 2, 5), (3, 7, 2),
             (3, 10, 7), (10, 6, 7), (6, 11, 7), (6, 0, 11), (6, 1, 0), (10, 1, 6), (11, 0, 9), (2, 11, 9), (5, 2, 9),
             (11, 2, 7)]
    return np.array(vert, np.float32), faces


def make_icosahedron(scene, center, radius):
    vert, faces = icosa_tables()
    if center[2] > 0:
        color = v3(0, 1, 0)
    else:
        b = randf0to1()
        g = randf0to1()
        r = randf0to1()
        color = v3(b, g, r)
    for f in faces:
        scene.add(*[vert[i] * F(radius) + center for i in f], color)


def make_icosahedron_scene(scene, count=250, min_dist=100.0, max_dist=250.0, min_radius=20.0, max_radius=50.0,
                           red_triangle=False):
    for _ in range(count):
        min_allowed = F(min_dist + max_radius)
        while True:
            xyz = [F(2.0 * (float(randf0to1()) - 0.5) * max_dist) for _ in range(3)]
            center = v3(*xyz)
            if not (float(norm(center)) < float(min_allowed)):
                break
        radius_range = F(max_radius - min_radius)
        radius = F(min_radius + float(randf0to1() * radius_range))
        make_icosahedron(scene, center, radius)
    if red_triangle:
        depth = F(min_dist)
        side = F(0.1) * depth
        scene.add(v3(depth, 0, 0), v3(depth, 0, side), v3(depth, side, 0), v3(0, 0, 1))


def make_cubes_scene(scene):
    verts = [v3(0, 0, 0), v3(0, 0, 1), v3(0, 1, 0), v3(0, 1, 1), v3(1, 0, 0), v3(1, 0, 1), v3(1, 1, 0), v3(1, 1, 1)]
    faces = [(2, 0, 1), (1, 3, 2), (6, 2, 0), (0, 4, 6), (4, 0, 1), (1, 5, 4), (3, 1, 5), (5, 7, 3), (7, 3, 2), (2, 6, 7),
             (5, 4, 6), (6, 7, 5)]
    scales = [F(2), F(1)]
    offsets = [v3(0, 0, -25), v3(5, 2, -20)]
    shift = v3(-0.5, -0.5, -0.5)
    colors = [[(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0)],
              [(0.5, 1, 0), (1, 0, 0.5), (1, 1, 1), (0, 0.5, 1), (0.5, 0.5, 1), (0, 0, 0)]]
    for t, f in enumerate(faces):
        for cube in range(2):
            scene.add(*[scales[cube] * (verts[i] + shift) + offsets[cube] for i in f], v3(*colors[cube][t // 2]))


def make_ground_plane_scene(scene, dist=1.70):
    r, z = F(100.0), F(-dist)
    v = [v3(-r, -r, z), v3(r, -r, z), v3(r, r, z), v3(-r, r, z)]
    red = v3(0, 0, 1)
    scene.add(v[0], v[1], v[2], red)
    scene.add(v[3], v[0], v[2], red)


def make_bvh(scene, leaf_threshold=20, split_k=5, max_depth=50):
    """BoundingVolumeHierarchy::makeBVH into the pre-order flat form."""
    scene.nodes, scene.leaf = [], []
    v0, v1, v2 = scene.field("v0"), scene.field("v1"), scene.field("v2")

    def build(tris, depth):
        cm = v3(0, 0, 0)
        for i in tris:
            cm = cm + ((v0[i] + v1[i]) + v2[i])
        cm = div_float(cm, F(len(tris) * 3))
        radius = F(0)
        for i in tris:
            for v in (v0, v1, v2):
                radius = max(radius, F(norm(cm - v[i])))
        node = dict(center=cm, radius=F(radius), skip=0, first=0, count=-1, n_children=0)
        scene.nodes.append(node)
        n = len(tris)
        if depth >= max_depth or n < split_k or n < leaf_threshold:
            node["first"], node["count"] = len(scene.leaf), n
            scene.leaf.extend(tris)
            node["skip"] = len(scene.nodes)
            return
        centers = []
        while len(centers) < split_k:
            r = _libc.rand() % n
            if r not in centers:
                centers.append(r)
        clusters = [[] for _ in range(split_k)]
        for i in tris:
            diff = v0[i][None, :] - v0[[tris[c] for c in centers]]
            dist2 = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2]
            best, pick = FLT_MAX, 0
            for j in range(split_k):
                if dist2[j] < best:
                    best, pick = dist2[j], j
            clusters[pick].append(i)
        node["n_children"] = split_k
        for c in clusters:
            build(c, depth + 1)
        node["skip"] = len(scene.nodes)

    build(list(range(len(scene.tri))), 0)
    return scene


# ---------------------------------------------------------------- tracer
def _sphere_hit(o, d, center, radius):
    with np.errstate(all="ignore"):
        c = center[None, :] - o
        len2 = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
        r2 = radius * radius
        inside = len2 < r2
        closest = dot(c, d)
        half = r2 + closest * closest - len2
        return inside | (~(closest < F(0)) & (half >= F(0)))


def _triangle_hit(o, d, t):
    with np.errstate(all="ignore"):
        q = cross(d, t["e2"][None, :])
        a = dot(t["e1"][None, :], q)
        ok = ~(a * a < F(0.0001))
        s = div_float(o - t["v0"][None, :], a)
        r = cross(s, t["e1"][None, :])
        b0 = dot(s, q)
        b1 = dot(r, d)
        b2 = F(1) - b0 - b1
        ok &= ~((b0 < F(0)) | (b1 < F(0)) | (b2 < F(0)))
        dist = dot(t["e2"][None, :], r)
        ok &= ~(dist < F(0))
        return ok, dist


def trace_tree(scene, o, d):
    n = o.shape[0]
    nxt = np.zeros(n, np.int64)
    best = np.full(n, FLT_MAX, np.float32)
    hit = np.full(n, -1, np.int32)
    for j, node in enumerate(scene.nodes):
        act = np.nonzero(nxt == j)[0]
        if act.size == 0:
            continue
        h = _sphere_hit(o[act], d[act], node["center"], node["radius"])
        nxt[act[~h]] = node["skip"]
        go = act[h]
        nxt[go] = j + 1
        for k in range(max(node["count"], 0)):
            ti = scene.leaf[node["first"] + k]
            ok, dist = _triangle_hit(o[go], d[go], scene.tri[ti])
            with np.errstate(invalid="ignore"):
                better = ok & (dist < best[go])
            best[go[better]] = dist[better]
            hit[go[better]] = ti
    return hit, best


def _fade(t):
    return t * t * t * (t * (t * F(6) - F(15)) + F(10))


def _lerp(t, a, b):
    return a + t * (b - a)


def _grad(h, x, y, z):
    h = h & 15
    u = np.where(h < 8, x, y)
    v = np.where(h < 4, y, np.where((h == 12) | (h == 14), x, z))
    return np.where((h & 1) == 0, u, -u) + np.where((h & 2) == 0, v, -v)


def pnoise(x, y, z):
    p = PERLIN512
    fx, fy, fz = (np.floor(a.astype(np.float64)) for a in (x, y, z))
    X, Y, Z = (a.astype(np.int64) & 255 for a in (fx, fy, fz))
    x, y, z = ((a.astype(np.float64) - f).astype(np.float32) for a, f in ((x, fx), (y, fy), (z, fz)))
    u, v, w = _fade(x), _fade(y), _fade(z)
    A = p[X] + Y
    AA, AB = p[A] + Z, p[A + 1] + Z
    B = p[X + 1] + Y
    BA, BB = p[B] + Z, p[B + 1] + Z
    one = F(1)
    return _lerp(w,
                 _lerp(v, _lerp(u, _grad(p[AA], x, y, z), _grad(p[BA], x - one, y, z)),
                       _lerp(u, _grad(p[AB], x, y - one, z), _grad(p[BB], x - one, y - one, z))),
                 _lerp(v, _lerp(u, _grad(p[AA + 1], x, y, z - one), _grad(p[BA + 1], x - one, y, z - one)),
                       _lerp(u, _grad(p[AB + 1], x, y - one, z - one), _grad(p[BB + 1], x - one, y - one, z - one))))


def trace(scene, origin, direction, skybox, outside=None, ceiling=None, ceiling_position=0.0, ceiling_width=0.0,
          ceiling_depth=0.0, marble=False, marble_scale=0.1):
    """traceRayToGetColor for rays [n, 3] float32. Returns a dict: hit (index, -1 sky, -2 ceiling, -3 outside), distance,
    color (BGR x 255), and for the sky rays sample_x / sample_y (NaN elsewhere)."""
    o = np.ascontiguousarray(origin, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(direction, np.float32).reshape(-1, 3)
    n = o.shape[0]
    outside = np.zeros(n, bool) if outside is None else np.asarray(outside, bool).reshape(-1)
    live = np.nonzero(~outside)[0]
    hit = np.full(n, -3, np.int32)
    dist = np.full(n, FLT_MAX, np.float32)
    col = np.zeros((n, 3), np.float32)
    sx = np.full(n, np.nan, np.float32)
    sy = np.full(n, np.nan, np.float32)
    h, best = trace_tree(scene, o[live], d[live])
    hit[live] = h
    done = np.zeros(n, bool)
    if ceiling is not None:
        rows, cols = ceiling.shape[:2]
        with np.errstate(all="ignore"):
            cd = ((ceiling_position - o[live, 2].astype(np.float64)) / d[live, 2].astype(np.float64)).astype(np.float32)
            cand = (F(0) < cd) & (cd < best)
            p = o[live] + cd[:, None] * d[live]
            s = (p[:, 0].astype(np.float64) / ceiling_width + 0.5).astype(np.float32)
            t = (p[:, 1].astype(np.float64) / ceiling_depth + 0.5).astype(np.float32)
            cand &= (F(0) <= s) & (s < F(1)) & (F(0) <= t) & (t < F(1))
        idx = live[cand]
        row = np.minimum((t[cand] * F(rows)).astype(np.int64), rows - 1)
        cl = np.minimum((s[cand] * F(cols)).astype(np.int64), cols - 1)
        col[idx] = ceiling[row, cl].astype(np.float32) / F(255)
        dist[idx] = cd[cand]
        hit[idx] = -2
        done[idx] = True
    sky = live[(h < 0) & ~done[live]]
    if sky.size:
        rows, cols = skybox.shape[:2]
        dz = np.clip(d[sky, 2], F(-1), F(1))
        phi = np.array([math.acos(float(v)) for v in dz], np.float64).astype(np.float32)
        theta = np.array([math.pi + math.atan2(float(y), float(x)) for x, y in zip(d[sky, 0], d[sky, 1])],
                         np.float64).astype(np.float32)
        sample_x = ((theta.astype(np.float64) / (2.0 * math.pi)) * cols).astype(np.float32)
        sample_y = ((phi.astype(np.float64) / math.pi) * rows).astype(np.float32)
        col[sky] = skybox[np.minimum(sample_y.astype(np.int64), rows - 1), sample_x.astype(np.int64) % cols].astype(
            np.float32) / F(255)
        hit[sky] = -1
        sx[sky], sy[sky] = sample_x, sample_y
    geo = live[(h >= 0) & ~done[live]]
    if geo.size:
        dist[geo] = best[(h >= 0) & ~done[live]]
        ti = hit[geo]
        base = scene.field("color")[ti]
        normal = scene.field("normal")[ti]
        p = o[geo] + dist[geo][:, None] * d[geo]
        if marble:
            m = [(marble_scale * p[:, k].astype(np.float64)).astype(np.float32) for k in range(3)]
            base = base * (F(0.7) + F(0.3) * np.abs(pnoise(*m)))[:, None]
        ld = LIGHT[None, :] - p
        ld = div_double(ld, norm(ld))
        nd = dot(normal, ld)
        coef = F(0.25) + F(0.75) * np.where(F(0) < nd, nd, F(0)).astype(np.float32)
        col[geo] = base * coef[:, None]
    return dict(hit=hit, distance=dist, color=(F(255) * col).astype(np.float32), sample_x=sx, sample_y=sy)


def downscale(img, aas):
    """cv::resize INTER_AREA by an integer factor on both axes: the block's values summed in float32 in row-major
    order, times float32(1 / aas^2). A copy at aas 1."""
    if aas == 1:
        return img.copy()
    h, w = img.shape[0] // aas, img.shape[1] // aas
    acc = np.zeros((h, w) + img.shape[2:], np.float32)
    with np.errstate(over="ignore"):
        for sy in range(aas):
            for sx in range(aas):
                acc = acc + img[sy::aas, sx::aas][:h, :w]
        return (acc * (F(1) / F(aas * aas))).astype(np.float32)


def equirect_rays(w, h, stereo=False, ipr=3.2):
    """renderMonoEquirect / renderStereoEquirect's rays: (origin_left, origin_right, direction), [h, w, 3] float32."""
    ol, orr, dr = (np.zeros((h, w, 3), np.float32) for _ in range(3))
    for y in range(h):
        phi = F(math.pi * float(F(y) + F(0.5)) / float(F(h)))
        for x in range(w):
            theta = F(float(F(2.0)) * math.pi * float(F(1.0) - (F(x) + F(0.5)) / F(w)))
            sp, cp, st, ct = math.sin(float(phi)), math.cos(float(phi)), math.sin(float(theta)), math.cos(float(theta))
            dr[y, x] = (F(sp * ct), F(sp * st), F(cp))
            if stereo:
                a, b = float(theta) + math.pi / 2.0, float(theta) - math.pi / 2.0
                ol[y, x] = (F(float(F(math.cos(a))) * ipr), F(float(F(math.sin(a))) * ipr), F(0.0 * ipr))
                orr[y, x] = (F(float(F(math.cos(b))) * ipr), F(float(F(math.sin(b))) * ipr), F(0.0 * ipr))
    return ol, orr, dr


def near_integer(s, ulps=4):
    """True where a float32 sample lies within `ulps` float ulps of an integer (the band in which device and glibc
    roundings of acos / atan2 may pick different texels)."""
    s = np.asarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        return np.abs(s - np.rint(s)) <= ulps * np.spacing(np.abs(s))
