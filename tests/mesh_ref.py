"""Restatement of the reference's camera-mesh path for tests/test_mesh*.py and tests/test_gpu_mesh*.py:
mesh_util::getVertexesEquiError / getTriangleMask / getFaces / applyMaskToVertexesAndFaces / writeObj
(source/render/MeshUtil.h), render::MeshSimplifier (source/render/MeshSimplifier.cpp), and binary_fusion::addFile /
pad / fuseFrame with StripedFile::calcStripe (source/mesh_stream). fp64 throughout: numpy arrays where the reference
loops over independent elements, plain Python floats (IEEE doubles, never contracted) in the sequential collapse loop.

Eigen's own evaluation order is not readable here; the one fixed for the product is used:
squaredNorm / dot = a0 + (a1 + a2); cross = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0); det3 = cofactors along the
first row, (a m0 - b m1) + c m2; normalized() = v / sqrt(squaredNorm) when squaredNorm > 0.

The camera enters only through Camera::rescale (Camera.cpp:217-223) and getScalarFocal (:185-188): two lines of
fp64, written out here. Nothing in this file touches the GPU."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
EXIT_BUDGET, EXIT_INFINITE_THRESHOLD, EXIT_STUCK = 0, 1, 2


# ---------------------------------------------------------------- cv::resize INTER_NEAREST (resizeNN)
def nearest_table(ssize, dsize, fx):
    ifx = 1.0 / fx
    return np.minimum(np.floor(np.arange(dsize) * ifx).astype(np.int64), ssize - 1)


def resize_nearest_scale(img, s):
    """cv::resize(img, img, cv::Size(), s, s, INTER_NEAREST): dsize = saturate_cast<int>(ssize * s) (round half even)"""
    h, w = img.shape
    dw, dh = int(np.rint(w * s)), int(np.rint(h * s))
    return img[nearest_table(h, dh, s)][:, nearest_table(w, dw, s)]


def resize_nearest_to(img, dw, dh):
    h, w = img.shape
    return img[nearest_table(h, dh, dh / h)][:, nearest_table(w, dw, dw / w)]


# ---------------------------------------------------------------- Camera::rescale + getScalarFocal
def scalar_focal(cam, resolution=None):
    """-> (resolution x, resolution y, focal) of the camera the mesh is built for"""
    resx, resy = float(cam["resolution"][0]), float(cam["resolution"][1])
    fx, fy = float(cam["focal"][0]), float(cam["focal"][1])
    if resolution is not None:
        fx *= float(resolution[0]) / resx
        fy *= float(resolution[1]) / resy
        resx, resy = float(resolution[0]), float(resolution[1])
    assert fx == -fy, "pixels are not square"
    return resx, resy, fx


def resize_rig_resolution(cam, cols, rows):
    """resizeRig (ConvertToBinary.cpp:318-339): xScale is a float; -> the new resolution, or None when xScale == 1"""
    xs, ys = F32(cols) / F32(cam["resolution"][0]), F32(rows) / F32(cam["resolution"][1])
    assert xs == ys
    if xs == 1:
        return None
    return [float(xs) * float(cam["resolution"][0]), float(xs) * float(cam["resolution"][1])]


# ---------------------------------------------------------------- MeshUtil.h
def fdiv(a, b):
    """IEEE a / b on Python floats (Python raises on a zero divisor)"""
    if b == 0:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _less(a, b):  # std::tuple<double, int> operator<
    return a[0] < b[0] or (not (b[0] < a[0]) and a[1] < b[1])


def triangle_mask(tl, tr, bl, br, tear):
    """getTriangleMask (:167-220), isRigCoordinates = false; std::sort of four elements is an insertion sort"""
    v = [(tl, 0), (tr, 1), (bl, 2), (br, 3)]
    for i in range(1, 4):
        val = v[i]
        j = i
        if _less(val, v[0]):
            while j > 0:
                v[j] = v[j - 1]
                j -= 1
        else:
            while _less(val, v[j - 1]):
                v[j] = v[j - 1]
                j -= 1
        v[j] = val
    if fdiv(v[0][0], v[3][0]) > tear:
        if abs(tl - br) < abs(tr - bl):
            return 1 << 1 | 1 << 2
        return 1 << 0 | 1 << 3
    lo, hi = fdiv(v[0][0], v[2][0]), fdiv(v[1][0], v[3][0])
    if lo >= tear and lo > hi:
        return 1 << (v[3][1] ^ 3)
    if hi >= tear:
        return 1 << (v[0][1] ^ 3)
    return 0


def _triangle(which, base, width):  # addTriangle (:222-247)
    return [(base + width, base + 1, base), (base, base + width + 1, base + 1), (base + width + 1, base, base + width),
            (base + 1, base + width, base + width + 1)][which]


def build(cam, disparity, resolution=None, depth_scale=1.0, mask=None, tear_ratio=0.95):
    """convertDepth (ConvertToBinary.cpp:164-198) up to applyMaskToVertexesAndFaces.
    -> dict(V f64 [nv, 3], F i32 [nf, 3], unmasked = faces before the mask, outcomes = {triangle mask: quads})"""
    with np.errstate(all="ignore"):
        depth = F32(1.0) / np.asarray(disparity, dtype=F32)
        if depth_scale < 1:
            depth = resize_nearest_scale(depth, depth_scale)
        h, w = depth.shape
        resx, resy, focal = scalar_focal(cam, resolution)
        ys, xs = np.mgrid[0:h, 0:w]
        vert = np.stack([resx / w * (xs + 0.5), resy / h * (ys + 0.5), focal / depth.astype(F64)], axis=2).reshape(-1, 3)
    valid = ~np.isnan(depth)
    if mask is not None:
        valid &= resize_nearest_to(np.asarray(mask) != 0, w, h)
    valid = valid.reshape(-1)
    tear = float(F32(tear_ratio))  # `const float tearRatio`, promoted in every comparison
    z = vert[:, 2].tolist()
    faces, outcomes = [], {}
    for y in range(h - 1):
        for x in range(w - 1):
            base = y * w + x
            m = triangle_mask(z[base], z[base + 1], z[base + w], z[base + w + 1], tear)
            outcomes[m] = outcomes.get(m, 0) + 1
            for t in range(4):
                if m >> t & 1:
                    faces.append(_triangle(t, base, w))
    faces = np.array(faces, dtype=np.int64).reshape(-1, 3)
    keep = valid[faces].all(axis=1)
    kept = faces[keep]
    used = np.zeros(len(vert), bool)
    used[kept.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return dict(V=np.ascontiguousarray(vert[used]), F=remap[kept].astype(np.int32).reshape(-1, 3), unmasked=len(faces),
                outcomes=outcomes, w=w, h=h)


def vtx_idx(V, F, clamp_negative_z):
    """the simplified branch's FLT_MIN clamp (:211-217) and writeDepth's casts (MeshUtil.h:72-89)"""
    V = np.array(V, dtype=F64).reshape(-1, 3)
    if clamp_negative_z:
        V[V[:, 2] < 0, 2] = float(np.finfo(F32).tiny)
    with np.errstate(all="ignore"):
        return V.astype(F32), np.asarray(F).astype(np.uint32).reshape(-1, 3)


def obj_text(vtx, idx):
    """writeObj (MeshUtil.h:91-129) of readVertexes / readFaces of the files just written"""
    lines = ["v %g %g %g\n" % tuple(float(c) for c in v) for v in np.asarray(vtx, dtype=F32).astype(F64)]
    lines += ["f %d %d %d\n" % tuple(int(i) + 1 for i in f) for f in np.asarray(idx).astype(np.int32)]
    return "".join(lines)


# ---------------------------------------------------------------- MeshSimplifier: set-up (arrays)
def _fast_error(q, x, y, z):  # computeFastError (:103-107), as written
    return (q[0] * x * x + 2 * q[1] * x * y + 2 * q[2] * x * z + 2 * q[3] * x + q[4] * y * y + 2 * q[5] * y * z +
            2 * q[6] * y + q[7] * z * z + 2 * q[8] * z + q[9])


def _det3(a, b, c, d, e, f, g, h, i):
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


def setup(V, F, equi_error=True):
    """computeInitialQuadrics (:182-239) -> (face planes [nf, 4], edge costs [nf, 3], vertex quadrics [nv, 10])"""
    V = np.asarray(V, dtype=F64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    nf = len(F)
    with np.errstate(all="ignore"):
        p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        u, v = p1 - p0, p2 - p0
        c = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                      u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        n2 = c[:, 0] * c[:, 0] + (c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])
        n = np.where((n2 > 0)[:, None], c / np.sqrt(n2)[:, None], c)
        d = -(n[:, 0] * p0[:, 0] + (n[:, 1] * p0[:, 1] + n[:, 2] * p0[:, 2]))
        planes = np.concatenate([n, d[:, None]], axis=1)
        Q = np.stack([planes[:, i] * planes[:, j] for i in range(4) for j in range(i, 4)], axis=1)
        # vertex.q += face.q in ascending face index: the k-th face of every vertex, k = 0, 1, ...
        vert, face = F.reshape(-1), np.repeat(np.arange(nf), 3)
        order = np.argsort(vert, kind="stable")
        vert, face = vert[order], face[order]
        start = np.searchsorted(vert, vert, side="left")
        rank = np.arange(len(vert)) - start
        vq = np.zeros((len(V), 10))
        for k in range(int(rank.max()) + 1 if len(rank) else 0):
            sel = rank == k
            vq[vert[sel]] = vq[vert[sel]] + Q[face[sel]]
        costs = np.zeros((nf, 3))
        for j in range(3):
            i0, i1 = F[:, j], F[:, (j + 1) % 3]
            q = (vq[i0] + vq[i1]).T
            det = _det3(q[0], q[1], q[2], q[1], q[4], q[5], q[2], q[5], q[7])
            mx = _det3(q[1], q[2], q[3], q[4], q[5], q[6], q[5], q[7], q[8])
            my = _det3(q[0], q[2], q[3], q[1], q[5], q[6], q[2], q[7], q[8])
            mz = _det3(q[0], q[1], q[3], q[1], q[4], q[6], q[2], q[5], q[8])
            s = 1 / det
            tq = np.stack([s * -mx, s * my, s * -mz], axis=1)
            eq = _fast_error(q, tq[:, 0], tq[:, 1], tq[:, 2])
            c0, c1 = V[i0], V[i1]
            cand = [c0, c1, (c0 + c1) / 2]
            errs = [_fast_error(q, k[:, 0], k[:, 1], k[:, 2]) for k in cand]
            best_e, best_t = errs[0].copy(), cand[0].copy()
            for k in (1, 2):  # std::min_element: the first of the smallest
                lt = errs[k] < best_e
                best_e = np.where(lt, errs[k], best_e)
                best_t = np.where(lt[:, None], cand[k], best_t)
            quad = det != 0
            err = np.where(quad, eq, best_e)
            tgt = np.where(quad[:, None], tq, best_t)
            if not equi_error:
                err = err / (tgt[:, 0] * tgt[:, 0] + (tgt[:, 1] * tgt[:, 1] + tgt[:, 2] * tgt[:, 2]))
            costs[:, j] = err
    return planes, costs, vq


# ---------------------------------------------------------------- MeshSimplifier: the collapse loop (Python floats)
def _norm(v):
    n2 = v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])
    if n2 > 0:
        n = math.sqrt(n2)
        return (v[0] / n, v[1] / n, v[2] / n)
    return v


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def threshold_index(strictness, n):
    """getThreshold's index into n sorted costs: a float product, truncated; F32(n - 1) rounds up past 2^24, where the
    reference reads past the end, so it is cut at the last cost"""
    return min(int(F32(strictness) * F32(n - 1)), n - 1)


class Simplifier:
    def __init__(self, V, F, setup_arrays, equi_error):
        planes, costs, vq = setup_arrays
        self.coord = [tuple(r) for r in np.asarray(V, dtype=F64).reshape(-1, 3).tolist()]
        self.q = np.asarray(vq, dtype=F64).tolist()
        self.boundary = [False] * len(self.coord)
        self.faces_of = [[] for _ in self.coord]
        # a face: [v0, v1, v2, normal, [cost0, cost1, cost2], deleted, touched]
        self.faces = [[f[0], f[1], f[2], tuple(p[:3]), list(c), False, False]
                      for f, p, c in zip(np.asarray(F).reshape(-1, 3).tolist(), np.asarray(planes).tolist(),
                                         np.asarray(costs).tolist())]
        self.equi = equi_error

    def error(self, i0, i1):  # computeError (:132-170) -> (error, target)
        q = [a + b for a, b in zip(self.q[i0], self.q[i1])]
        det = _det3(q[0], q[1], q[2], q[1], q[4], q[5], q[2], q[5], q[7])
        if det != 0 and not (self.boundary[i0] and self.boundary[i1]):
            mx = _det3(q[1], q[2], q[3], q[4], q[5], q[6], q[5], q[7], q[8])
            my = _det3(q[0], q[2], q[3], q[1], q[5], q[6], q[2], q[7], q[8])
            mz = _det3(q[0], q[1], q[3], q[1], q[4], q[6], q[2], q[5], q[8])
            s = 1 / det
            t = (s * -mx, s * my, s * -mz)
            e = _fast_error(q, *t)
        else:
            c0, c1 = self.coord[i0], self.coord[i1]
            cand = [c0, c1, ((c0[0] + c1[0]) / 2, (c0[1] + c1[1]) / 2, (c0[2] + c1[2]) / 2)]
            errs = [_fast_error(q, *k) for k in cand]
            best = 0
            for k in (1, 2):
                if errs[k] < errs[best]:
                    best = k
            t, e = cand[best], errs[best]
        if not self.equi:
            e = fdiv(e, t[0] * t[0] + (t[1] * t[1] + t[2] * t[2]))
        return e, t

    def remove_deleted_faces(self):
        for f in self.faces:
            f[6] = False
        self.faces = [f for f in self.faces if not f[5]]

    def assign_face_vertexes(self):
        self.faces_of = [[] for _ in self.coord]
        for i, f in enumerate(self.faces):
            for j in range(3):
                self.faces_of[f[j]].append(i)

    def common_faces(self, v0, v1):
        return [i1 for i1 in self.faces_of[v0] for i2 in self.faces_of[v1] if i1 == i2]

    def identify_boundaries(self):  # identifySubBoundaries (:280-319), one range
        b, fo = self.boundary, self.faces_of
        for i in range(len(b)):
            b[i] = False
        for i in range(len(b)):
            if b[i]:
                continue
            if len(fo[i]) == 1:
                b[i] = True
                continue
            border, visited = False, set()
            for fi in fo[i]:
                for j in range(3):
                    v = self.faces[fi][j]
                    if v != i and v not in visited:
                        visited.add(v)
                        if len(fo[v]) == 1 or len(self.common_faces(i, v)) == 1:
                            b[v] = True
                            border = True
            if border:
                b[i] = True

    def threshold(self, strictness):  # getThreshold (:333-344)
        errors = [c for f in self.faces for c in f[4]]
        assert not any(c != c for c in errors), "a NaN cost: std::nth_element's result is not defined"
        idx = threshold_index(strictness, len(errors))
        return sorted(errors)[idx]

    def normals_flipped(self, p, v0, v1):  # haveNormalsFlipped (:348-382)
        for fi in self.faces_of[v0]:
            f = self.faces[fi]
            if f[5]:
                continue
            order = 0
            for j in range(3):
                if f[j] == v0:
                    order = j
                    break
            i0, i1 = f[(order + 1) % 3], f[(order + 2) % 3]
            if i0 == v1 or i1 == v1:
                continue
            a, b = _norm(_sub(self.coord[i0], p)), _norm(_sub(self.coord[i1], p))
            n = _norm(_cross(a, b))
            if n[0] * f[3][0] + (n[1] * f[3][1] + n[2] * f[3][2]) < 0:
                return True
        return False

    def update_costs(self, v0, v1, target):  # updateCosts (:384-420)
        self.coord[v0] = target
        self.q[v0] = [a + b for a, b in zip(self.q[v0], self.q[v1])]
        for fi in self.faces_of[v0] + self.faces_of[v1]:
            f = self.faces[fi]
            if f[5]:
                continue
            for i in range(3):
                if f[i] == v0 or f[i] == v1:
                    f[i] = v0
                    f[6] = True
                    break
            for i in range(3):
                f[4][i] = self.error(f[i], f[(i + 1) % 3])[0]

    def run(self, num_faces_out, strictness, remove_boundary_edges):  # simplify (:456-562)
        n_in = len(self.faces)
        deleted = deleted_prev = same = iteration = 0
        threshold, reason = 0.0, EXIT_BUDGET
        while len(self.faces) > num_faces_out:
            self.remove_deleted_faces()
            if not self.faces:  # the last collapse deleted what was left: the reference indexes an empty vector here
                break
            self.assign_face_vertexes()
            if iteration == 0:
                self.identify_boundaries()
            if iteration == 0 or deleted_prev != deleted:
                threshold = self.threshold(strictness)
                same = 0
            else:
                same += 1
                threshold *= 2 * same
                if math.isinf(threshold):
                    reason = EXIT_INFINITE_THRESHOLD
                    break
                if not abs(threshold) > 0:  # the product's one departure: the reference repeats this pass for ever
                    reason = EXIT_STUCK
                    break
            deleted_prev = deleted
            b = self.boundary
            for f in self.faces:
                if f[5] or f[6]:
                    continue
                for i in range(3):
                    if f[4][i] > threshold:
                        continue
                    v0, v1 = f[i], f[(i + 1) % 3]
                    if b[v0] != b[v1]:
                        continue
                    if not remove_boundary_edges and (b[v0] or b[v1]):
                        continue
                    target = self.error(v0, v1)[1]
                    if self.normals_flipped(target, v0, v1) or self.normals_flipped(target, v1, v0):
                        continue
                    common = self.common_faces(v0, v1)
                    for fi in common:
                        self.faces[fi][5] = True
                    deleted += len(common)
                    self.update_costs(v0, v1, target)
                    break
                if n_in - deleted <= num_faces_out:
                    break
            iteration += 1
        return iteration, reason

    def final_mesh(self):  # createFinalMesh (:423-454)
        self.remove_deleted_faces()
        used = np.zeros(len(self.coord), bool)
        F = np.array([f[:3] for f in self.faces], dtype=np.int64).reshape(-1, 3)
        used[F.reshape(-1)] = True
        remap = np.cumsum(used) - 1
        V = np.array(self.coord, dtype=F64).reshape(-1, 3)[used]
        return np.ascontiguousarray(V), remap[F].astype(np.int32).reshape(-1, 3)


def simplify(V, F, num_faces_out, strictness=0.2, remove_boundary_edges=False, equi_error=True):
    """MeshSimplifier(V, F, equi_error, 1).simplify(...) -> (V', F', (passes, EXIT_*))"""
    s = Simplifier(V, F, setup(V, F, equi_error), equi_error)
    stats = s.run(num_faces_out, strictness, remove_boundary_edges)
    v, f = s.final_mesh()
    return v, f, stats


# ---------------------------------------------------------------- BinaryFusionUtil.h + StripedFile.h
STRIPE = 512 * 1024


def _align(offset):
    return (offset + STRIPE - 1) & ~(STRIPE - 1)


class Fuser:
    """disks = bytearrays; addFile / pad / fuseFrame with every fwrite appended to the disk calcStripe names"""

    def __init__(self, disk_count):
        self.disks = [bytearray() for _ in range(disk_count)]
        self.offset = 0
        self.catalog = {"metadata": {"isLittleEndian": True}, "frames": {}}

    def _disk(self, offset):
        return (offset // STRIPE) % len(self.disks)

    def add_file(self, data):
        aligned = _align(self.offset)
        end = self.offset + STRIPE if self.offset == aligned else aligned
        at = 0
        while at < len(data):
            n = min(len(data) - at, end - self.offset)
            self.disks[self._disk(self.offset)] += data[at:at + n]
            self.offset += n
            end = self.offset + STRIPE
            at += n

    def pad(self):
        aligned = _align(self.offset)
        if aligned != self.offset:
            self.disks[self._disk(self.offset)] += b"\x5a" * (aligned - self.offset)
            self.offset = aligned

    def fuse_frame(self, frame, cameras, extensions, read):
        """read(camera, extension) -> the bytes of <bin>/<camera>/<frame><extension>"""
        entry = self.catalog["frames"].setdefault(frame, {})
        for cam in cameras:
            begin = self.offset
            c = entry.setdefault(cam, {})
            for ext in extensions:
                b = self.offset
                self.add_file(read(cam, ext))
                c[ext] = {"offset": b, "size": self.offset - b}
            c["offset"] = begin
            c["size"] = self.offset - begin
            self.pad()

    def read_back(self, offset, size):
        """`size` bytes at the logical `offset`, through the stripe mapping (StripedFile::calcStripe)"""
        out = bytearray()
        while size:
            stripe = offset // STRIPE
            local = (stripe // len(self.disks)) * STRIPE + offset % STRIPE
            n = min(size, STRIPE - offset % STRIPE)
            out += self.disks[stripe % len(self.disks)][local:local + n]
            offset += n
            size -= n
        return bytes(out)


# ---------------------------------------------------------------- shared inputs
def synthetic_depth(w, h, seed=0):
    """a smooth ramp with ripples, a step edge, a NaN hole -> disparity f32 [h, w] (cases (a), (d) of the host tests)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    depth = 2.0 + 0.02 * xs + 0.01 * ys + 0.05 * np.sin(xs * 0.7) * np.cos(ys * 0.5) + 0.003 * rng.random((h, w))
    depth[:, w // 2:] += 1.5  # a step well past the tear ratio
    disp = (1.0 / depth).astype(F32)
    disp[h // 3:h // 3 + 4, w // 4:w // 4 + 5] = np.nan
    return disp


def gpu_disparity(w, h):
    """the GPU tests' map: ramp, a step below the tear ratio, one much nearer and one much farther pixel, two equal-depth
    plateaus, a NaN block, a zero disparity"""
    ys, xs = np.mgrid[0:h, 0:w]
    depth = 3.0 + 0.004 * xs + 0.003 * ys + 0.01 * np.sin(xs * 0.9) * np.cos(ys * 0.8)
    depth[:, (2 * w) // 3:] *= 1.03          # a step edge that stays connected (ratio 0.97 > 0.95)
    depth[h // 4, w // 5] = 1.0              # one pixel much nearer
    depth[h // 2, w // 2] = 40.0             # one pixel much farther
    depth[3:9, 3:11] = 3.25                  # two plateaus of exactly equal depth: the sort's tie rule
    depth[h - 10:h - 4, w // 3:w // 3 + 7] = 3.5
    depth[h // 5:h // 5 + 3, (3 * w) // 5:(3 * w) // 5 + 6] *= 1.08  # a torn patch: single triangles at its corners
    disp = (1.0 / depth).astype(F32)
    disp[h // 2 + 5:h // 2 + 9, 5:10] = np.nan
    disp[h - 3, w - 4] = 0.0                 # infinite depth
    return disp
