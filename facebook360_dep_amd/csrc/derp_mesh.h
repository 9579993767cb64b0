// Kernels of ConvertToBinary's camera meshes (source/mesh_stream/ConvertToBinary.cpp:150-245): a disparity map ->
// equi-error vertices (MeshUtil.h:317-341), the faces of every 2x2 quad that does not tear (getTriangleMask / getFaces,
// :167-296), the vertex mask applied to both (applyMaskToVertexesAndFaces, :345-405), and MeshSimplifier's set-up
// (computeInitialQuadrics, MeshSimplifier.cpp:182-239) on the compacted mesh. The reference walks the quads in row-major
// order and re-indexes through a std::map; here every pixel is the base of (at most) one quad, block counts + one scan +
// a scatter give the same order. getFaces and the mask are fused: a quad's triangle mask and the subset of it whose
// three vertices pass the vertex mask are computed together, the unmasked face list is only counted.
// All fp64 expressions are the reference's, in its order; the file builds with -ffp-contract=off.
#pragma once
#include "derp_mesh_math.h"
#include "derp_points.h"

namespace derp {

constexpr int kMeshBlock = 256;  // threads per block of every kernel here (four waves)

// ---- block-wide exclusive scan of one small count per thread (wave shuffles, then the four wave totals in LDS) ----
__device__ __forceinline__ uint32_t mesh_block_scan(uint32_t v, uint32_t* waveTotal, uint32_t& blockTotal) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if (lane >= d) {
      inc += up;
    }
  }
  if (lane == 63) {
    waveTotal[wave] = inc;
  }
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (int w = 0; w < kMeshBlock / 64; ++w) {
    before += w < wave ? waveTotal[w] : 0;
    total += waveTotal[w];
  }
  blockTotal = total;
  return before + inc - v;
}

// ---- getVertexesEquiError on `depth = 1.0f / disparity` after the optional INTER_NEAREST resize, and the vertex mask
// (ConvertToBinary.cpp:164-189). xofs / yofs: resizeNN's source column / row of every output column / row (identity
// without --depth_scale); mxofs / myofs: the same for the foreground mask, resized to the depth's size.
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_vertices(const float* __restrict__ disparity, int srcW, const int* __restrict__ xofs, const int* __restrict__ yofs,
                    int W, int H, double resx, double resy, double scale, const uint8_t* __restrict__ mask, int maskW,
                    const int* __restrict__ mxofs, const int* __restrict__ myofs, double* __restrict__ vert,
                    uint8_t* __restrict__ valid) {
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= (size_t)W * H) {
    return;
  }
  const int x = (int)(i % W), y = (int)(i / W);
  const float depth = 1.0f / disparity[(size_t)yofs[y] * srcW + xofs[x]];
  vert[3 * i] = resx / W * (x + 0.5);
  vert[3 * i + 1] = resy / H * (y + 0.5);
  vert[3 * i + 2] = scale / (double)depth;
  bool ok = !(depth != depth);
  if (mask) {
    ok = ok && mask[(size_t)myofs[y] * maskW + mxofs[x]] != 0;
  }
  valid[i] = ok;
}

// ---- getVertexesEquirect (MeshUtil.h:298-314): depth = fmin(maxDepth, 1.0f / disparity) in float, times the unit
// direction of the pixel's centre in fp64. theta depends on the column and phi on the row alone: tabs holds cos(theta) [W],
// sin(theta) [W], sin(phi) [H], cos(phi) [H], computed on the host as the reference's expressions round them. norm = the
// vertex's distance from the rig centre as Eigen's row norm sums it, which is getTriangleMask's key in rig coordinates.
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_vertices_equirect(const float* __restrict__ disparity, int W, int H, float maxDepth, const double* __restrict__ tabs,
                             double* __restrict__ V, double* __restrict__ norm) {
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (i >= (size_t)W * H) {
    return;
  }
  const int x = (int)(i % W), y = (int)(i / W);
  const double depth = (double)fminf(maxDepth, 1.0f / disparity[i]);
  const double sinPhi = tabs[2 * (size_t)W + y], cosPhi = tabs[2 * (size_t)W + H + y];
  const double px = depth * (sinPhi * tabs[x]), py = depth * cosPhi, pz = depth * (sinPhi * tabs[(size_t)W + x]);
  V[3 * i] = px;
  V[3 * i + 1] = py;
  V[3 * i + 2] = pz;
  norm[i] = sqrt((px * px + py * py) + pz * pz);
}

// ---- getTriangleMask for camera meshes (isRigCoordinates = false: the key is the vertex's z) -----------------------
// std::sort of four (z, corner) tuples is libstdc++'s insertion sort with the tuples' lexicographic operator<; written
// out so that a NaN key (a comparator that is no strict weak order) lands where it lands there.
struct MeshKey {
  double z;
  int c;
};
__host__ __device__ __forceinline__ bool mesh_key_less(const MeshKey& a, const MeshKey& b) {
  return a.z < b.z || (!(b.z < a.z) && a.c < b.c);
}
__host__ __device__ __forceinline__ unsigned mesh_triangle_mask(double tl, double tr, double bl, double br, float tearRatio) {
  // __insertion_sort on four elements, unrolled over named values (an indexed array would live in scratch memory): an
  // element smaller than the first moves the whole prefix up; otherwise it walks down while it is smaller than its
  // left neighbour (and cannot pass the first, which it was just found not smaller than)
  MeshKey v0 = {tl, 0}, v1 = {tr, 1}, v2 = {bl, 2}, v3 = {br, 3};
  {
    const MeshKey val = v1;
    if (mesh_key_less(val, v0)) {
      v1 = v0;
      v0 = val;
    }
  }
  {
    const MeshKey val = v2;
    if (mesh_key_less(val, v0)) {
      v2 = v1;
      v1 = v0;
      v0 = val;
    } else if (mesh_key_less(val, v1)) {
      v2 = v1;
      v1 = val;
    }
  }
  {
    const MeshKey val = v3;
    if (mesh_key_less(val, v0)) {
      v3 = v2;
      v2 = v1;
      v1 = v0;
      v0 = val;
    } else if (mesh_key_less(val, v2)) {
      v3 = v2;
      if (mesh_key_less(val, v1)) {
        v2 = v1;
        v1 = val;
      } else {
        v2 = val;
      }
    }
  }
  const MeshKey v[4] = {v0, v1, v2, v3};
  const double tear = (double)tearRatio;
  if (v[0].z / v[3].z > tear) {
    if (fabs(tl - br) < fabs(tr - bl)) {
      return 1u << 1 | 1u << 2;
    }
    return 1u << 0 | 1u << 3;
  }
  const double lo = v[0].z / v[2].z, hi = v[1].z / v[3].z;
  if (lo >= tear && lo > hi) {
    return 1u << (v[3].c ^ 3);
  }
  if (hi >= tear) {
    return 1u << (v[0].c ^ 3);
  }
  return 0;
}

// Every pixel is the base (top-left corner) of one quad, except in the last column and row. qmask = the quad's triangle
// mask (low nibble) and the triangles of it whose three vertices pass the vertex mask (high nibble). Triangle t of a
// quad (addTriangle) has every corner but t ^ 3. key[keyStride * pixel] = getTriangleMask's depth of the pixel's vertex:
// its z in a camera mesh, its norm in rig coordinates. valid == nullptr: no vertex mask.
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_quads(const double* __restrict__ key, int keyStride, const uint8_t* __restrict__ valid, int W, int H, float tearRatio,
                 uint8_t* __restrict__ qmask, uint32_t* __restrict__ blockFaces, unsigned long long* __restrict__ unmasked) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  __shared__ uint32_t rawTotal[kMeshBlock / 64];
  const size_t n = (size_t)W * H;
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  unsigned tm = 0, km = 0;
  if (i < n) {
    const int x = (int)(i % W), y = (int)(i / W);
    if (x < W - 1 && y < H - 1) {
      const size_t c[4] = {i, i + 1, i + (size_t)W, i + (size_t)W + 1};
      tm = mesh_triangle_mask(key[keyStride * c[0]], key[keyStride * c[1]], key[keyStride * c[2]], key[keyStride * c[3]],
                              tearRatio);
      unsigned ok = valid ? 0u : 0xfu;
      if (valid) {
        for (int k = 0; k < 4; ++k) {
          ok |= (valid[c[k]] ? 1u : 0u) << k;
        }
      }
      for (int t = 0; t < 4; ++t) {
        const unsigned need = 0xfu & ~(1u << (t ^ 3));
        if ((tm >> t & 1) && (ok & need) == need) {
          km |= 1u << t;
        }
      }
    }
    qmask[i] = (uint8_t)(tm | km << 4);
  }
  uint32_t total;
  mesh_block_scan((uint32_t)__popc(km), waveTotal, total);
  // the unmasked count is needed as a total only: one wave reduction, one atomic per block
  uint32_t raw = (uint32_t)__popc(tm);
  for (int d = 32; d > 0; d >>= 1) {
    raw += __shfl_down(raw, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    rawTotal[threadIdx.x >> 6] = raw;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    blockFaces[blockIdx.x] = total;
    uint32_t r = 0;
    for (int w = 0; w < kMeshBlock / 64; ++w) {
      r += rawTotal[w];
    }
    atomicAdd(unmasked, (unsigned long long)r);
  }
}

// the kept triangles of the quad at (qx, qy) that contain its corner `corner`; 0 outside the grid of quads
__device__ __forceinline__ unsigned mesh_kept_at_corner(const uint8_t* __restrict__ qmask, int W, int H, int qx, int qy,
                                                        int corner) {
  if (qx < 0 || qy < 0 || qx >= W - 1 || qy >= H - 1) {
    return 0;
  }
  return (unsigned)(qmask[(size_t)qy * W + qx] >> 4) & ~(1u << (corner ^ 3));
}

// "Keep only vertexes of retained faces": a vertex is the br / bl / tr / tl corner of the (up to) four quads around it
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_vertex_used(const uint8_t* __restrict__ qmask, int W, int H, uint8_t* __restrict__ used,
                       uint32_t* __restrict__ blockVerts) {
  __shared__ uint32_t waveCount[kMeshBlock / 64];
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  bool u = false;
  if (i < (size_t)W * H) {
    const int x = (int)(i % W), y = (int)(i / W);
    u = (mesh_kept_at_corner(qmask, W, H, x - 1, y - 1, 3) | mesh_kept_at_corner(qmask, W, H, x, y - 1, 2) |
         mesh_kept_at_corner(qmask, W, H, x - 1, y, 1) | mesh_kept_at_corner(qmask, W, H, x, y, 0)) != 0;
    used[i] = u;
  }
  const unsigned long long ballot = __ballot(u);
  if ((threadIdx.x & 63) == 0) {
    waveCount[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int w = 0; w < kMeshBlock / 64; ++w) {
      total += waveCount[w];
    }
    blockVerts[blockIdx.x] = total;
  }
}

// surviving vertices in ascending order: vmap = new index of every kept pixel, vorig = the pixel of every new index
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_vertex_scatter(const double* __restrict__ vert, const uint8_t* __restrict__ used, size_t n,
                          const unsigned long long* __restrict__ blockOffset, uint32_t* __restrict__ vmap,
                          uint32_t* __restrict__ vorig, double* __restrict__ outV) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const bool u = i < n && used[i];
  uint32_t total;
  const uint32_t rank = mesh_block_scan(u ? 1u : 0u, waveTotal, total);
  if (u) {
    const size_t o = (size_t)blockOffset[blockIdx.x] + rank;
    vmap[i] = (uint32_t)o;
    vorig[o] = (uint32_t)i;
    outV[3 * o] = vert[3 * i];
    outV[3 * o + 1] = vert[3 * i + 1];
    outV[3 * o + 2] = vert[3 * i + 2];
  }
}

// kept faces in row-major quad order, triangles 0..3 ascending, addTriangle's vertex orders, re-indexed (vmap ==
// nullptr: every vertex keeps its pixel's index); qoff = the index of every quad's first kept face
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_face_scatter(const uint8_t* __restrict__ qmask, int W, int H, const unsigned long long* __restrict__ blockOffset,
                        const uint32_t* __restrict__ vmap, uint32_t* __restrict__ qoff, int32_t* __restrict__ outF) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t n = (size_t)W * H;
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const unsigned km = i < n ? (unsigned)qmask[i] >> 4 : 0u;
  uint32_t total;
  const uint32_t rank = mesh_block_scan((uint32_t)__popc(km), waveTotal, total);
  if (i >= n) {
    return;
  }
  size_t f = (size_t)blockOffset[blockIdx.x] + rank;
  qoff[i] = (uint32_t)f;
  if (km == 0) {
    return;
  }
  const size_t tl = i, tr = i + 1, bl = i + (size_t)W, br = i + (size_t)W + 1;
  const size_t tri[4][3] = {{bl, tr, tl}, {tl, br, tr}, {br, tl, bl}, {tr, bl, br}};
  for (int t = 0; t < 4; ++t) {
    if (km >> t & 1) {
      for (int k = 0; k < 3; ++k) {
        outF[3 * f + k] = (int32_t)(vmap ? vmap[tri[t][k]] : (uint32_t)tri[t][k]);
      }
      ++f;
    }
  }
}

// getFaces' wrapHorizontally (MeshUtil.h:285-293): after the last grid face, two faces per row that link column W - 1
// back to column 0, in row order, with no tear test
__global__ void __launch_bounds__(kMeshBlock) k_mesh_seam_faces(int W, int H, size_t firstSeamFace, int32_t* __restrict__ outF) {
  const int y = blockIdx.x * kMeshBlock + threadIdx.x;
  if (y >= H - 1) {
    return;
  }
  const int32_t base = y * W;
  int32_t* f = outF + 3 * (firstSeamFace + 2 * (size_t)y);
  f[0] = base + W;
  f[1] = base;
  f[2] = base + W - 1;
  f[3] = base + W - 1;
  f[4] = base + 2 * W - 1;
  f[5] = base + W;
}

// ---- MeshSimplifier::computeInitialQuadrics on the compacted mesh ---------------------------------------------------
// computeSubQuadrics: one thread per face -> its plane [n, -n.p0] (the normal is what haveNormalsFlipped reads later)
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_face_planes(const double* __restrict__ V, const int32_t* __restrict__ F, size_t nf, double* __restrict__ planes) {
  const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf) {
    return;
  }
  derp_mesh::V3 p[3];
  for (int k = 0; k < 3; ++k) {
    const size_t v = (size_t)F[3 * f + k];
    p[k] = {V[3 * v], V[3 * v + 1], V[3 * v + 2]};
  }
  double q4[4];
  derp_mesh::face_plane(p[0], p[1], p[2], q4);
  for (int k = 0; k < 4; ++k) {
    planes[4 * f + k] = q4[k];
  }
}

// "Accumulating quadrics...": vertex.q += face.q over the faces in ascending index. A vertex's faces lie in the four
// quads around it, whose faces are numbered in the order (x-1, y-1), (x, y-1), (x-1, y), (x, y), triangles ascending:
// a gather in that order is the sequential sum, with no atomics. vorig == nullptr: the mesh is the whole grid. seam:
// the mesh has k_mesh_seam_faces' faces from index firstSeamFace on; those of a vertex of column 0 or W - 1 follow all
// its grid faces, by ascending row: (y - 1: both, y: the first) in column 0, (y - 1: the second, y: both) in column W - 1.
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_vertex_quadrics(const uint8_t* __restrict__ qmask, const uint32_t* __restrict__ qoff,
                           const uint32_t* __restrict__ vorig, int W, int H, size_t nv, const double* __restrict__ planes,
                           int seam, size_t firstSeamFace, double* __restrict__ vq) {
  const size_t v = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= nv) {
    return;
  }
  const uint32_t i = vorig ? vorig[v] : (uint32_t)v;
  const int x = (int)(i % (uint32_t)W), y = (int)(i / (uint32_t)W);
  double Q[derp_mesh::kQuadric];
  for (int k = 0; k < derp_mesh::kQuadric; ++k) {
    Q[k] = 0.0;
  }
  const int qx[4] = {x - 1, x, x - 1, x}, qy[4] = {y - 1, y - 1, y, y}, corner[4] = {3, 2, 1, 0};
  for (int a = 0; a < 4; ++a) {
    if (qx[a] < 0 || qy[a] < 0 || qx[a] >= W - 1 || qy[a] >= H - 1) {
      continue;
    }
    const size_t qi = (size_t)qy[a] * W + qx[a];
    const unsigned km = (unsigned)qmask[qi] >> 4;
    size_t f = qoff[qi];
    for (int t = 0; t < 4; ++t) {
      if (km >> t & 1) {
        if (t != (corner[a] ^ 3)) {
          double q4[4];
          for (int k = 0; k < 4; ++k) {
            q4[k] = planes[4 * f + k];
          }
          derp_mesh::add_plane_quadric(Q, q4);
        }
        ++f;
      }
    }
  }
  if (seam && (x == 0 || x == W - 1)) {
    // the seam faces of rows y - 1 and y as a run of four; bit k set = face firstSeamFace + 2 (y - 1) + k holds the vertex
    const unsigned has = x == 0 ? 0x7u : 0xeu;
    for (int k = 0; k < 4; ++k) {
      const int row = y - 1 + (k >> 1);
      if ((has >> k & 1) && row >= 0 && row < H - 1) {
        const size_t f = firstSeamFace + 2 * (size_t)row + (k & 1);
        double q4[4];
        for (int j = 0; j < 4; ++j) {
          q4[j] = planes[4 * f + j];
        }
        derp_mesh::add_plane_quadric(Q, q4);
      }
    }
  }
  for (int k = 0; k < derp_mesh::kQuadric; ++k) {
    vq[v * derp_mesh::kQuadric + k] = Q[k];
  }
}

// computeSubError: one thread per (face, edge); isBoundary is false everywhere before identifyBoundaries has run
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_edge_costs(const double* __restrict__ V, const int32_t* __restrict__ F, size_t nf, const double* __restrict__ vq,
                      int equiError, double* __restrict__ costs) {
  const size_t e = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (e >= nf * 3) {
    return;
  }
  const size_t f = e / 3;
  const int j = (int)(e % 3);
  const size_t i0 = (size_t)F[3 * f + j], i1 = (size_t)F[3 * f + (j + 1) % 3];
  derp_mesh::V3 target;
  costs[e] = derp_mesh::compute_error(vq + i0 * derp_mesh::kQuadric, vq + i1 * derp_mesh::kQuadric,
                                      {V[3 * i0], V[3 * i0 + 1], V[3 * i0 + 2]}, {V[3 * i1], V[3 * i1 + 1], V[3 * i1 + 2]},
                                      false, equiError != 0, target);
}


// ---- the pass-parallel simplifier (derp_mesh_simplify_parallel) --------------------------------
// MeshSimplifier's collapse arithmetic and rules (computeError, haveNormalsFlipped, commonFaces, updateCosts) with
// another choice of what a pass collapses: the threshold is a rank over the feasible edges only, and the collapses of
// a pass are the candidates that hold the smallest (cost, face, edge) key on every face they touch, so that no two of
// them share a face and all of them can be applied at once. Faces keep their index in the built mesh; a deleted face
// only loses its alive flag. A vertex's alive faces are a CSR list rebuilt every pass; its order is whatever the
// atomics gave, and every use of it below is a minimum, an OR or a count.
constexpr unsigned long long kMeshNoKey = ~0ull;  // (the pattern of a NaN: never a feasible cost)
constexpr uint32_t kMeshNoClaim = 0xffffffffu;
constexpr uint32_t kMeshApplied = 0x80000000u;
// slots of the per-pass counters
enum { MESH_CNT_FEASIBLE = 0, MESH_CNT_WINNERS, MESH_CNT_APPLIED, MESH_CNT_DELETED, MESH_CNT_THRESHOLD, MESH_CNT_SLOTS };

// a cost as a 64-bit pattern whose unsigned order is the order of the doubles (-0 counts as +0)
__host__ __device__ __forceinline__ unsigned long long mesh_cost_key(double c) {
  c = c == 0 ? 0.0 : c;
  unsigned long long b;
  memcpy(&b, &c, 8);
  return (b >> 63) ? ~b : b | 1ull << 63;
}
__host__ __device__ __forceinline__ double mesh_key_cost(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? k & ~(1ull << 63) : ~k;
  double c;
  memcpy(&c, &b, 8);
  return c;
}

struct MeshAdjacency {  // faces [start[v], start[v] + count[v]) of adj are vertex v's alive faces
  const uint32_t* __restrict__ start;
  const uint32_t* __restrict__ count;
  const uint32_t* __restrict__ adj;
};

__device__ __forceinline__ derp_mesh::V3 mesh_coord(const double* __restrict__ V, int v) {
  return {V[3 * (size_t)v], V[3 * (size_t)v + 1], V[3 * (size_t)v + 2]};
}
__device__ __forceinline__ bool mesh_face_has(const int32_t* __restrict__ F, uint32_t f, int v) {
  return F[3 * (size_t)f] == v || F[3 * (size_t)f + 1] == v || F[3 * (size_t)f + 2] == v;
}
// commonFaces(v0, v1).size(): a face is in both lists once, so it is the faces of v0 that hold v1
__device__ __forceinline__ uint32_t mesh_common_faces(const MeshAdjacency& A, const int32_t* __restrict__ F, int v0, int v1) {
  uint32_t n = 0;
  const uint32_t s = A.start[v0], e = s + A.count[v0];
  for (uint32_t k = s; k < e; ++k) {
    n += mesh_face_has(F, A.adj[k], v1) ? 1u : 0u;
  }
  return n;
}
// computeError of the edge (v0, v1) as MeshSimplifier::computeError(v0, v1, target) calls it
__device__ __forceinline__ double mesh_edge_error(const double* __restrict__ V, const double* __restrict__ vq,
                                                  const uint8_t* __restrict__ boundary, int v0, int v1, bool equiError,
                                                  derp_mesh::V3& target) {
  return derp_mesh::compute_error(vq + (size_t)v0 * derp_mesh::kQuadric, vq + (size_t)v1 * derp_mesh::kQuadric,
                                  mesh_coord(V, v0), mesh_coord(V, v1), boundary[v0] && boundary[v1], equiError, target);
}
// haveNormalsFlipped (MeshSimplifier.cpp:348-382) over the alive faces of v0, against the set-up's face normals
__device__ __forceinline__ bool mesh_normals_flipped(const MeshAdjacency& A, const double* __restrict__ V,
                                                     const int32_t* __restrict__ F, const double* __restrict__ planes,
                                                     const derp_mesh::V3& p, int v0, int v1) {
  const uint32_t s = A.start[v0], e = s + A.count[v0];
  for (uint32_t k = s; k < e; ++k) {
    const size_t t = A.adj[k];
    const int a = F[3 * t], b = F[3 * t + 1], c = F[3 * t + 2];
    // the two vertices after v0 in the face's order (order 0 when v0 is not found, as there)
    const int i0 = a == v0 ? b : b == v0 ? c : c == v0 ? a : b;
    const int i1 = a == v0 ? c : b == v0 ? a : c == v0 ? b : c;
    if (i0 == v1 || i1 == v1) {
      continue;
    }
    const derp_mesh::V3 d0 = derp_mesh::normalized(derp_mesh::sub(mesh_coord(V, i0), p));
    const derp_mesh::V3 d1 = derp_mesh::normalized(derp_mesh::sub(mesh_coord(V, i1), p));
    const derp_mesh::V3 normal = derp_mesh::normalized(derp_mesh::cross(d0, d1));
    if (derp_mesh::dot(normal, {planes[4 * t], planes[4 * t + 1], planes[4 * t + 2]}) < 0) {
      return true;
    }
  }
  return false;
}

// ---- a pass's adjacency: count, scan, fill
__global__ void __launch_bounds__(kMeshBlock)
    k_par_vertex_degrees(const int32_t* __restrict__ F, const uint8_t* __restrict__ alive, size_t nf, uint32_t* __restrict__ count) {
  const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf || !alive[f]) {
    return;
  }
  for (int k = 0; k < 3; ++k) {
    atomicAdd(&count[F[3 * f + k]], 1u);
  }
}
// the sum of every block's values (counts or 0 / 1 flags), for k_scan_block_counts
template <typename T>
__global__ void __launch_bounds__(kMeshBlock) k_par_block_sums(const T* __restrict__ values, size_t n, uint32_t* __restrict__ blockSum) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  uint32_t total;
  mesh_block_scan(i < n ? (uint32_t)values[i] : 0u, waveTotal, total);
  if (threadIdx.x == 0) {
    blockSum[blockIdx.x] = total;
  }
}
__global__ void __launch_bounds__(kMeshBlock)
    k_par_vertex_starts(const uint32_t* __restrict__ count, size_t nv, const unsigned long long* __restrict__ blockOffset,
                        uint32_t* __restrict__ start, uint32_t* __restrict__ cursor) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t v = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  uint32_t total;
  const uint32_t rank = mesh_block_scan(v < nv ? count[v] : 0u, waveTotal, total);
  if (v < nv) {
    start[v] = cursor[v] = (uint32_t)blockOffset[blockIdx.x] + rank;
  }
}
__global__ void __launch_bounds__(kMeshBlock)
    k_par_adjacency_fill(const int32_t* __restrict__ F, const uint8_t* __restrict__ alive, size_t nf, uint32_t* __restrict__ cursor,
                         uint32_t* __restrict__ adj) {
  const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf || !alive[f]) {
    return;
  }
  for (int k = 0; k < 3; ++k) {
    adj[atomicAdd(&cursor[F[3 * f + k]], 1u)] = (uint32_t)f;
  }
}

// identifyBoundaries' set, before the first pass: both ends of every edge with exactly one common face
__global__ void __launch_bounds__(kMeshBlock)
    k_par_boundaries(MeshAdjacency A, const int32_t* __restrict__ F, size_t nf, uint8_t* __restrict__ boundary) {
  const size_t e = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (e >= nf * 3) {
    return;
  }
  const size_t f = e / 3;
  const int i = (int)(e % 3);
  const int v0 = F[3 * f + i], v1 = F[3 * f + (i + 1) % 3];
  if (mesh_common_faces(A, F, v0, v1) == 1) {
    boundary[v0] = 1;
    boundary[v1] = 1;
  }
}

// ---- the feasible set: one thread per (face, edge) -> its sort key (kMeshNoKey when barred), and every block's count
__global__ void __launch_bounds__(kMeshBlock)
    k_par_feasible(MeshAdjacency A, const double* __restrict__ V, const int32_t* __restrict__ F, const uint8_t* __restrict__ alive,
                   size_t nf, const double* __restrict__ planes, const double* __restrict__ costs, const double* __restrict__ vq,
                   const uint8_t* __restrict__ boundary, int removeBoundaryEdges, int equiError, unsigned long long* __restrict__ keys,
                   uint32_t* __restrict__ blockSum) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t e = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  unsigned long long key = kMeshNoKey;
  if (e < nf * 3 && alive[e / 3]) {
    const size_t f = e / 3;
    const int i = (int)(e % 3);
    const int v0 = F[3 * f + i], v1 = F[3 * f + (i + 1) % 3];
    const bool b0 = boundary[v0] != 0, b1 = boundary[v1] != 0;
    const double cost = costs[e];
    if (b0 == b1 && (removeBoundaryEdges || !(b0 || b1)) && cost == cost) {
      derp_mesh::V3 target;
      mesh_edge_error(V, vq, boundary, v0, v1, equiError != 0, target);
      if (!mesh_normals_flipped(A, V, F, planes, target, v0, v1) && !mesh_normals_flipped(A, V, F, planes, target, v1, v0)) {
        key = mesh_cost_key(cost);
      }
    }
  }
  if (e < nf * 3) {
    keys[e] = key;
  }
  uint32_t total;
  mesh_block_scan(key != kMeshNoKey ? 1u : 0u, waveTotal, total);
  if (threadIdx.x == 0) {
    blockSum[blockIdx.x] = total;
  }
}
// the feasible edges alone, by ascending face * 3 + edge: what the sort reads
__global__ void __launch_bounds__(kMeshBlock)
    k_par_feasible_compact(const unsigned long long* __restrict__ keys, size_t n3, const unsigned long long* __restrict__ blockOffset,
                           unsigned long long* __restrict__ ckeys, uint32_t* __restrict__ cvals) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t e = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const unsigned long long key = e < n3 ? keys[e] : kMeshNoKey;
  uint32_t total;
  const uint32_t rank = mesh_block_scan(key != kMeshNoKey ? 1u : 0u, waveTotal, total);
  if (key != kMeshNoKey) {
    const size_t o = (size_t)blockOffset[blockIdx.x] + rank;
    ckeys[o] = key;
    cvals[o] = (uint32_t)e;
  }
}

// The sorted keys are the feasible edges in (cost, face * 3 + edge) order (a stable sort of keys that went in by
// ascending index), so an edge's position r is its rank. getThreshold's index over them (n > 0; the entries keep
// strictness within [0, 1]):
__device__ __forceinline__ unsigned long long mesh_threshold_key(const unsigned long long* __restrict__ skeys, unsigned long long n,
                                                               float strictness) {
  const unsigned long long idx = (unsigned long long)(strictness * (float)(n - 1));  // (64 bits: no int to overflow)
  return skeys[idx < n - 1 ? idx : n - 1];  // (float)(n - 1) rounds up past 2^24: the last rank at most
}
// claim: every candidate writes its rank to each face it touches; the smallest stays
__global__ void __launch_bounds__(kMeshBlock)
    k_par_claim(MeshAdjacency A, const int32_t* __restrict__ F, const unsigned long long* __restrict__ skeys,
                const uint32_t* __restrict__ svals, float strictness, unsigned long long* __restrict__ counters,
                uint32_t* __restrict__ claim) {
  const size_t r = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const unsigned long long n = counters[MESH_CNT_FEASIBLE];
  if (r >= n) {
    return;
  }
  const unsigned long long threshold = mesh_threshold_key(skeys, n, strictness);
  if (r == 0) {
    counters[MESH_CNT_THRESHOLD] = threshold;
  }
  if (skeys[r] > threshold) {
    return;
  }
  const size_t f = svals[r] / 3;
  const int i = (int)(svals[r] % 3);
  const int v[2] = {F[3 * f + i], F[3 * f + (i + 1) % 3]};
  for (int side = 0; side < 2; ++side) {
    const uint32_t s = A.start[v[side]], e = s + A.count[v[side]];
    for (uint32_t k = s; k < e; ++k) {
      atomicMin(&claim[A.adj[k]], (uint32_t)r);
    }
  }
}
// winners: the candidates that kept every face they touch -> wins[r] = commonFaces(v0, v1).size() (0: no winner), and
// every block's sum of them for the prefix sums of the budget cut
__global__ void __launch_bounds__(kMeshBlock)
    k_par_winners(MeshAdjacency A, const int32_t* __restrict__ F, const unsigned long long* __restrict__ skeys,
                  const uint32_t* __restrict__ svals, float strictness, const uint32_t* __restrict__ claim,
                  unsigned long long* __restrict__ counters, uint32_t* __restrict__ wins, uint32_t* __restrict__ blockSum) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t r = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const unsigned long long n = counters[MESH_CNT_FEASIBLE];
  uint32_t common = 0;
  if (r < n && skeys[r] <= mesh_threshold_key(skeys, n, strictness)) {
    const size_t f = svals[r] / 3;
    const int i = (int)(svals[r] % 3);
    const int v[2] = {F[3 * f + i], F[3 * f + (i + 1) % 3]};
    bool won = true;
    for (int side = 0; side < 2; ++side) {
      const uint32_t s = A.start[v[side]], e = s + A.count[v[side]];
      for (uint32_t k = s; k < e; ++k) {
        won = won && claim[A.adj[k]] == (uint32_t)r;
      }
    }
    if (won) {
      common = mesh_common_faces(A, F, v[0], v[1]);
    }
  }
  if (r < n) {
    wins[r] = common;
  }
  const unsigned long long ballot = __ballot(common != 0);
  if ((threadIdx.x & 63) == 0 && ballot) {
    atomicAdd(&counters[MESH_CNT_WINNERS], (unsigned long long)__popcll(ballot));
  }
  uint32_t total;
  mesh_block_scan(common, waveTotal, total);
  if (threadIdx.x == 0) {
    blockSum[blockIdx.x] = total;
  }
}

// The budget cut and updateCosts' vertex half: a winner is applied while the faces alive before the pass, less those
// the winners before it (in key order) delete, exceed the budget. v0 takes the target and q0 + q1. No other winner
// reads or writes v0 or v1: they are vertices of faces that only this winner touches.
__global__ void __launch_bounds__(kMeshBlock)
    k_par_apply_vertices(double* __restrict__ V, const int32_t* __restrict__ F, double* __restrict__ vq,
                         const uint8_t* __restrict__ boundary, int equiError, const uint32_t* __restrict__ svals,
                         const unsigned long long* __restrict__ blockOffset, long long aliveFaces, long long numFacesOut,
                         uint32_t* __restrict__ wins, unsigned long long* __restrict__ counters) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t r = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const uint32_t common = r < counters[MESH_CNT_FEASIBLE] ? wins[r] : 0u;
  uint32_t total;
  const unsigned long long before = blockOffset[blockIdx.x] + mesh_block_scan(common, waveTotal, total);
  if (common == 0 || !(aliveFaces - (long long)before > numFacesOut)) {
    return;
  }
  const size_t f = svals[r] / 3;
  const int i = (int)(svals[r] % 3);
  const int v0 = F[3 * f + i], v1 = F[3 * f + (i + 1) % 3];
  derp_mesh::V3 target;
  mesh_edge_error(V, vq, boundary, v0, v1, equiError != 0, target);
  V[3 * (size_t)v0] = target.x;
  V[3 * (size_t)v0 + 1] = target.y;
  V[3 * (size_t)v0 + 2] = target.z;
  for (int k = 0; k < derp_mesh::kQuadric; ++k) {
    vq[(size_t)v0 * derp_mesh::kQuadric + k] = vq[(size_t)v0 * derp_mesh::kQuadric + k] + vq[(size_t)v1 * derp_mesh::kQuadric + k];
  }
  wins[r] = common | kMeshApplied;
  atomicAdd(&counters[MESH_CNT_APPLIED], 1ull);
  atomicAdd(&counters[MESH_CNT_DELETED], (unsigned long long)common);
}
// ... and its face half, one thread per face: a face claimed by an applied winner is deleted when it holds both ends
// of the edge (commonFaces); otherwise its first v0 or v1 becomes v0 and its three costs are computed again. The
// winner's own face holds both ends, so nothing rewrites the indices read through svals here.
__global__ void __launch_bounds__(kMeshBlock)
    k_par_apply_faces(const double* __restrict__ V, int32_t* __restrict__ F, uint8_t* __restrict__ alive, size_t nf,
                      const double* __restrict__ vq, const uint8_t* __restrict__ boundary, int equiError,
                      const uint32_t* __restrict__ svals, const uint32_t* __restrict__ claim, const uint32_t* __restrict__ wins,
                      double* __restrict__ costs) {
  const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf || !alive[f]) {
    return;
  }
  const uint32_t r = claim[f];
  if (r == kMeshNoClaim || !(wins[r] & kMeshApplied)) {
    return;
  }
  const size_t wf = svals[r] / 3;
  const int wi = (int)(svals[r] % 3);
  const int v0 = F[3 * wf + wi], v1 = F[3 * wf + (wi + 1) % 3];
  int a = F[3 * f], b = F[3 * f + 1], c = F[3 * f + 2];
  const bool has0 = a == v0 || b == v0 || c == v0, has1 = a == v1 || b == v1 || c == v1;
  if (has0 && has1) {
    alive[f] = 0;
    return;
  }
  if (a == v0 || a == v1) {
    a = v0;
  } else if (b == v0 || b == v1) {
    b = v0;
  } else if (c == v0 || c == v1) {
    c = v0;
  }
  F[3 * f] = a;
  F[3 * f + 1] = b;
  F[3 * f + 2] = c;
  // one copy of computeError, three turns (three inlined copies spill to scratch memory)
#pragma unroll 1
  for (int k = 0; k < 3; ++k) {
    derp_mesh::V3 target;
    costs[3 * f + k] = mesh_edge_error(V, vq, boundary, a, b, equiError != 0, target);
    const int first = a;
    a = b;
    b = c;
    c = first;
  }
}

// ---- createFinalMesh: faces in their original order, the vertices they use ascending
__global__ void __launch_bounds__(kMeshBlock)
    k_par_vertices_used(const int32_t* __restrict__ F, const uint8_t* __restrict__ alive, size_t nf, uint8_t* __restrict__ used) {
  const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (f >= nf || !alive[f]) {
    return;
  }
  for (int k = 0; k < 3; ++k) {
    used[F[3 * f + k]] = 1;
  }
}
__global__ void __launch_bounds__(kMeshBlock)
    k_par_final_vertices(const double* __restrict__ V, const uint8_t* __restrict__ used, size_t nv,
                         const unsigned long long* __restrict__ blockOffset, uint32_t* __restrict__ vmap, double* __restrict__ outV) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t v = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const bool u = v < nv && used[v];
  uint32_t total;
  const uint32_t rank = mesh_block_scan(u ? 1u : 0u, waveTotal, total);
  if (u) {
    const size_t o = (size_t)blockOffset[blockIdx.x] + rank;
    vmap[v] = (uint32_t)o;
    outV[3 * o] = V[3 * v];
    outV[3 * o + 1] = V[3 * v + 1];
    outV[3 * o + 2] = V[3 * v + 2];
  }
}
__global__ void __launch_bounds__(kMeshBlock)
    k_par_final_faces(const int32_t* __restrict__ F, const uint8_t* __restrict__ alive, size_t nf,
                      const unsigned long long* __restrict__ blockOffset, const uint32_t* __restrict__ vmap, int32_t* __restrict__ outF) {
  __shared__ uint32_t waveTotal[kMeshBlock / 64];
  const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  const bool u = f < nf && alive[f];
  uint32_t total;
  const uint32_t rank = mesh_block_scan(u ? 1u : 0u, waveTotal, total);
  if (u) {
    const size_t o = (size_t)blockOffset[blockIdx.x] + rank;
    for (int k = 0; k < 3; ++k) {
      outF[3 * o + k] = (int32_t)vmap[F[3 * f + k]];
    }
  }
}

}  // namespace derp
