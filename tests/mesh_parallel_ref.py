"""Restatement of the pass-parallel mesh simplifier (derp_mesh_simplify_parallel) for
tests/test_mesh_parallel_ref.py and tests/test_gpu_mesh_parallel.py. The collapse arithmetic and rules are
mesh_ref.Simplifier's (computeError, haveNormalsFlipped, commonFaces, updateCosts, createFinalMesh); only how a pass
chooses what to collapse is new: the threshold is a rank over the feasible edges alone, and the collapses of a pass are
the cost-ordered independent set of the candidates (no two of them touch a common face), cut at the face budget.

Faces keep their index in the built mesh for the whole loop (it is part of a candidate's key); a deleted face stays in
the list. Nothing here touches the GPU."""
import numpy as np

from tests import mesh_ref as R

F32 = np.float32
EXIT_BUDGET, EXIT_NO_CANDIDATES = R.EXIT_BUDGET, 3


class ParallelSimplifier(R.Simplifier):
    def adjacency(self):
        """the alive faces of every vertex (step 1); the order inside a list is never read"""
        self.faces_of = [[] for _ in self.coord]
        for i, f in enumerate(self.faces):
            if not f[5]:
                for j in range(3):
                    self.faces_of[f[j]].append(i)

    def boundary_rule(self):
        """step 1's rule: a vertex is a boundary vertex iff one of its edges has exactly one common face"""
        b = [False] * len(self.coord)
        for f in self.faces:
            if f[5]:
                continue
            for i in range(3):
                v0, v1 = f[i], f[(i + 1) % 3]
                if len(self.common_faces(v0, v1)) == 1:
                    b[v0] = b[v1] = True
        return b

    def feasible(self, fi, i, remove_boundary_edges):
        f = self.faces[fi]
        v0, v1 = f[i], f[(i + 1) % 3]
        b = self.boundary
        if b[v0] != b[v1]:
            return False
        if not remove_boundary_edges and (b[v0] or b[v1]):
            return False
        if f[4][i] != f[4][i]:
            return False
        target = self.error(v0, v1)[1]
        return not (self.normals_flipped(target, v0, v1) or self.normals_flipped(target, v1, v0))

    def run(self, num_faces_out, strictness, remove_boundary_edges):
        n_in = alive = len(self.faces)
        passes, reason = 0, EXIT_BUDGET
        self.log = []  # per pass: (alive before, feasible, winners, winners applied, faces deleted, threshold)
        known = {}  # (face, edge) -> feasible, for the edges whose two vertices no collapse has come near since
        while alive > num_faces_out:
            assert passes < n_in, "every pass with a candidate deletes a face"
            self.adjacency()
            if passes == 0:
                self.boundary = self.boundary_rule()
            # ---- step 2: the feasible set
            feasible = []
            for fi, f in enumerate(self.faces):
                if f[5]:
                    continue
                for i in range(3):
                    if (fi, i) not in known:
                        known[(fi, i)] = self.feasible(fi, i, remove_boundary_edges)
                    if known[(fi, i)]:
                        feasible.append((f[4][i] + 0.0, fi, i))  # + 0.0: one zero, so that the key order is a total one
            if not feasible:
                reason = EXIT_NO_CANDIDATES
                break
            # ---- step 3: the threshold, getThreshold's float product over the feasible costs only
            feasible.sort()
            threshold = feasible[R.threshold_index(strictness, len(feasible))][0]
            candidates = [k for k in feasible if k[0] <= threshold]
            # ---- step 4: winners = the candidates that hold the smallest key on every face they touch
            claim = {}
            touched = {}
            for key in candidates:
                f = self.faces[key[1]]
                v0, v1 = f[key[2]], f[(key[2] + 1) % 3]
                touched[key] = set(self.faces_of[v0]) | set(self.faces_of[v1])
                for t in touched[key]:
                    if t not in claim or key < claim[t]:
                        claim[t] = key
            winners = [key for key in candidates if all(claim[t] == key for t in touched[key])]
            assert winners and winners[0] == candidates[0]
            seen = set()
            for key in winners:
                assert not (seen & touched[key]), "the winners' touched sets are disjoint"
                seen |= touched[key]
            # ---- steps 5, 6: in key order up to the face budget
            deleted = applied = 0
            dirty = set()
            for key in winners:
                if not alive - deleted > num_faces_out:
                    break
                f = self.faces[key[1]]
                v0, v1 = f[key[2]], f[(key[2] + 1) % 3]
                target = self.error(v0, v1)[1]
                for t in touched[key]:
                    dirty.update(self.faces[t][:3])
                common = self.common_faces(v0, v1)
                for t in common:
                    self.faces[t][5] = True
                deleted += len(common)
                applied += 1
                self.update_costs(v0, v1, target)
            self.log.append((alive, len(feasible), len(winners), applied, deleted, threshold))
            alive -= deleted
            passes += 1
            # an edge's feasibility reads the faces of its two vertices and nothing else: it stands while neither vertex
            # belonged to a touched face (read before the relabelling: v1 is among them)
            known = {k: v for k, v in known.items()
                     if not self.faces[k[0]][5] and self.faces[k[0]][k[1]] not in dirty
                     and self.faces[k[0]][(k[1] + 1) % 3] not in dirty}
        return passes, reason


def simplify(V, F, num_faces_out, strictness=0.2, remove_boundary_edges=False, equi_error=True):
    """-> (V', F', (passes, EXIT_*)), like mesh_ref.simplify"""
    s = ParallelSimplifier(V, F, R.setup(V, F, equi_error), equi_error)
    stats = s.run(num_faces_out, strictness, remove_boundary_edges)
    v, f = s.final_mesh()
    return v, f, stats


# ---------------------------------------------------------------- shared cases and the quality measure
# name -> (disparity map, budget, remove_boundary_edges, equi_error); the camera is synth.make_rig(2, 64)'s first
CASES = {
    "plain": (lambda: R.synthetic_depth(48, 32), 600, False, True),
    "boundary": (lambda: R.synthetic_depth(48, 32), 600, True, True),
    "not_equi": (lambda: R.synthetic_depth(48, 32), 600, False, False),
    "unreachable": (lambda: R.synthetic_depth(48, 32), 100, False, True),
    "strip": (lambda: R.synthetic_depth(40, 2), 10, False, True),
    "above": (lambda: R.synthetic_depth(48, 32), 100000, False, True),
    "disparity": (lambda: R.gpu_disparity(70, 37), 600, False, True),
}
_results = {}


def case(name):
    """-> dict(disparity, budget, rbe, equi, V, F of the built mesh, out = simplify's result), computed once"""
    if name not in _results:
        from facebook360_dep_amd import synth

        disparity, budget, rbe, equi = CASES[name]
        disparity = disparity()
        m = R.build(synth.make_rig(2, 64)["cameras"][0], disparity)
        _results[name] = dict(disparity=disparity, budget=budget, rbe=rbe, equi=equi, V=m["V"], F=m["F"],
                              out=simplify(m["V"], m["F"], budget, 0.2, rbe, equi))
    return _results[name]


def surface_rms(points, V, F, chunk=256):
    """RMS over `points` of the distance to the nearest triangle of (V, F): brute force, the closest point on every
    triangle by its Voronoi regions (vertex, edge, interior)"""
    points, V = np.asarray(points, dtype=np.float64), np.asarray(V, dtype=np.float64)
    A, B, C = (V[np.asarray(F)[:, k]][None] for k in range(3))
    ab, ac = B - A, C - A
    best = np.empty(len(points))
    with np.errstate(all="ignore"):
        for at in range(0, len(points), chunk):
            P = points[at:at + chunk, None, :]
            ap, bp, cp = P - A, P - B, P - C
            d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
            d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
            d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
            va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
            denom = va + vb + vc
            Q = A + ab * (vb / denom)[..., None] + ac * (vc / denom)[..., None]  # inside the face
            for region, q in (  # later regions take precedence: the reverse of the usual first-match order
                    ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), B + (C - B) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]),
                    ((vb <= 0) & (d2 >= 0) & (d6 <= 0), A + ac * (d2 / (d2 - d6))[..., None]),
                    ((d6 >= 0) & (d5 <= d6), C + 0 * ap),
                    ((vc <= 0) & (d1 >= 0) & (d3 <= 0), A + ab * (d1 / (d1 - d3))[..., None]),
                    ((d3 >= 0) & (d4 <= d3), B + 0 * ap),
                    ((d1 <= 0) & (d2 <= 0), A + 0 * ap)):
                Q = np.where(region[..., None], q, Q)
            dist2 = ((P - Q) ** 2).sum(-1)
            dist2 = np.fmin(dist2, (ap ** 2).sum(-1))  # a degenerate face (no interior): one of its corners
            best[at:at + chunk] = np.nanmin(dist2, axis=1)
    return float(np.sqrt(best.mean()))
