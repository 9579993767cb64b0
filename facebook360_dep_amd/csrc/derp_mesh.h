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
// quad (addTriangle) has every corner but t ^ 3.
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_quads(const double* __restrict__ vert, const uint8_t* __restrict__ valid, int W, int H, float tearRatio,
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
      tm = mesh_triangle_mask(vert[3 * c[0] + 2], vert[3 * c[1] + 2], vert[3 * c[2] + 2], vert[3 * c[3] + 2], tearRatio);
      unsigned ok = 0;
      for (int k = 0; k < 4; ++k) {
        ok |= (valid[c[k]] ? 1u : 0u) << k;
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

// kept faces in row-major quad order, triangles 0..3 ascending, addTriangle's vertex orders, re-indexed; qoff = the
// index of every quad's first kept face
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
        outF[3 * f + k] = (int32_t)vmap[tri[t][k]];
      }
      ++f;
    }
  }
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
// a gather in that order is the sequential sum, with no atomics.
__global__ void __launch_bounds__(kMeshBlock)
    k_mesh_vertex_quadrics(const uint8_t* __restrict__ qmask, const uint32_t* __restrict__ qoff,
                           const uint32_t* __restrict__ vorig, int W, int H, size_t nv, const double* __restrict__ planes,
                           double* __restrict__ vq) {
  const size_t v = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= nv) {
    return;
  }
  const uint32_t i = vorig[v];
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

}  // namespace derp
