"""tests/equirect_mesh_ref.py against what must hold for any restatement of getVertexesEquirect + getFaces with the seam
(counts and the topology of a sphere with its two polar caps open), where 0 / NaN / negative disparities go, and the
host-only derp_mesh_texcoords_equirect against the restatement bit for bit. No GPU."""
import math

import numpy as np
import pytest

from tests import equirect_mesh_ref as E

F32 = np.float32


def edge_counts(F):
    """{undirected edge: faces that hold it}; the winding is not read"""
    counts = {}
    for a, b, c in np.asarray(F).tolist():
        for e in ((a, b), (b, c), (c, a)):
            k = (min(e), max(e))
            counts[k] = counts.get(k, 0) + 1
    return counts


@pytest.mark.parametrize("w,h,disp,max_depth", [(8, 4, 0.25, 700.0), (67, 33, 0.125, 700.0), (9, 5, 0.001, 20.0), (2, 2, 0.5, 700.0)])
def test_constant_disparity_is_a_sphere_with_open_caps(w, h, disp, max_depth):
    m = E.build(np.full((h, w), disp, F32), max_depth=max_depth)
    V, F = m["V"], m["F"]
    assert len(V) == w * h and len(F) == 2 * w * (h - 1) and m["grid"] == 2 * (w - 1) * (h - 1)
    depth = min(F32(max_depth), F32(1.0) / F32(disp))
    assert (m["norms"].astype(F32) == depth).all()  # to the last bit of the float depth
    assert F.min() == 0 and F.max() == w * h - 1
    if w == 2:
        return  # the seam quad and the grid quad share their four vertices: edges are doubled, no sphere
    edges = edge_counts(F)
    assert len(edges) == 3 * w * h - 2 * w
    assert len(V) - len(edges) + len(F) == 0
    once = [e for e, n in edges.items() if n == 1]
    assert len(once) == 2 * w and all(n == 2 for e, n in edges.items() if e not in set(once))
    rows = {a // w for a, b in once} | {b // w for a, b in once}
    assert rows == {0, h - 1}  # the two open caps
    # across the seam: h edges along the rows (one face in the top and bottom rows) and h - 1 diagonals
    seam = [n for (a, b), n in edges.items() if {a % w, b % w} == {0, w - 1}]
    assert len(seam) == 2 * h - 1 and sorted(seam) == [1, 1] + [2] * (2 * h - 3)


def test_zero_nan_and_negative_disparities():
    disp = np.array([[0.0, np.nan, -0.5, -0.0], [2.0, 1e-9, np.inf, 0.5]], F32)
    d = E.depths(disp, 700.0)
    assert d.dtype == F32
    assert d.tolist() == [[700.0, 700.0, -2.0, -math.inf], [0.5, 700.0, 0.0, 2.0]]
    V, norm = E.vertices(disp, 700.0)
    assert norm.astype(F32).tolist()[:3] == [700.0, 700.0, 2.0]
    assert np.isinf(norm[3]) and norm[6] == 0
    # a negative depth mirrors the vertex through the rig centre
    ct, st, sp, cp = E.angle_tables(4, 2)
    assert V[2].tolist() == [-2.0 * (sp[0] * ct[2]), -2.0 * cp[0], -2.0 * (sp[0] * st[2])]


def test_angle_tables_are_the_float_expressions():
    ct, st, sp, cp = E.angle_tables(4, 2)
    theta = F32(float(F32(F32(2.5) / F32(4)) * F32(2)) * math.pi)
    assert ct[2] == math.cos(float(theta)) and st[2] == math.sin(float(theta))
    assert float(theta) != (2.5 / 4) * 2 * math.pi  # the narrowing is visible
    phi = F32(float(F32(F32(1.5) / F32(2))) * math.pi)
    assert sp[1] == math.sin(float(phi)) and cp[1] == math.cos(float(phi))


def test_texcoords_on_the_host(built):
    from facebook360_dep_amd import derp

    tiny = 5e-324
    V = np.array([[1, 0, 0], [0, 0, 1], [-1, 0, 0], [0, 0, -1],  # +x, +z, -x, -z: s = 0, 0.25, 0.5, 0.75
                  [0, 1, 0], [0, -1, 0], [0, 0, 0],              # the poles, and the rig centre
                  [1, 0.3, 1e-300], [1, 0.3, -1e-300], [1, 0.3, tiny], [1, 0.3, -tiny], [1, 0.3, -0.0],  # the branch cut
                  [3.5, -2.25, 0.125], [-700, 12, 41], [np.inf, 1, 1], [np.nan, 1, 1]], np.float64)
    with np.errstate(all="ignore"):
        want = E.texcoords(V)
    got = derp.mesh_texcoords_equirect(V)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert want[:4, 0].tolist() == [0.0, 0.25, 0.5, 0.75] and (want[:4, 1] == 0.5).all()  # atan2(-0, -1) = -pi
    assert want[4:6, 1].tolist() == [1.0, 0.0]
    assert want[7, 0] == 0.0 and want[8, 0] == 1.0  # either side of the cut
    assert derp.mesh_texcoords_equirect(np.zeros((0, 3))).shape == (0, 2)


def test_bilinear_rule():
    img = np.arange(12, dtype=F32).reshape(3, 4)
    half = E.resize_bilinear(img, 0.5)  # 4 x 3 -> 2 x 2 (rint(1.5) = 2): columns at 0.5 and 2.5, rows at 0.5 and 2.5 -> 2
    assert half.shape == (2, 2)
    assert half.tolist() == [[(0.5 + 4.5) / 2, (2.5 + 6.5) / 2], [8.5, 10.5]]
    assert E.resize_bilinear(img, 0.75).shape == (2, 3)  # rint(2.25), rint(3)
    ramp = np.linspace(0, 1, 70 * 37, dtype=F32).reshape(37, 70)
    ramp[5, 5] = np.nan
    out = E.resize_bilinear(ramp, 0.5)
    assert out.shape == (18, 35) and out.dtype == F32 and np.isnan(out).sum() == 1
