// MeshStreamRenderer's GPU stages — RigScene's mesh path (source/render/RigScene.cpp: cameraMeshVS :195-218, cameraFS
// :244-259, createDirection :869-885, renderSubframe :920-974, exponentialFS / updateAccumulation :281-292, 1009-1020,
// resolveFS :294-307) for the indexed triangle meshes of the fused stream (.vtx / .idx / .rgba), without OpenGL.
//   k_stream_texture     .rgba bytes -> linear float BGR texels (GL_SRGB8_ALPHA8's decode, a 256-entry table)
//   k_stream_vertex      one thread per vertex: abc -> texVar, direction lookup, clip = transform * (pos, 1)
//   k_stream_raster      one thread per triangle: small ones rasterised in place, big ones listed with their boxes
//   k_stream_raster_big  a workgroup (times kStreamBigSplit) per listed triangle
//   k_stream_resolve     one thread per pixel: the winner's texVar, cameraFS, GL_RGBA16, exp(30 a) - 1, accumulate
//   k_stream_finish      resolveFS: fade * rgb / a
// Triangles are rasterised with 2-D homogeneous edge functions on (x, y, w) (Olano & Greer 1997), so one that crosses
// the near plane covers exactly what its part in front covers, with no clipped polygon; a clipped polygon only bounds
// the box of pixels that are tested. Rules and the choices where
// OpenGL is implementation-defined: DESIGN.md §8.11. fp32 like the shaders.
// Shared with the other renderers: canopy_bilinear (GL_LINEAR, clamp to edge), smr_unorm16 (GL_RGBA16), expf_glibc,
// k_smr_equirect, kCanopyBigTri.
#pragma once

namespace derp {

constexpr int kStreamDirections = 128;  // RigScene::kDirections
constexpr int kStreamBigSplit = 8;      // workgroups that share one listed triangle's box
constexpr float kStreamNear = 0.1f;     // kNearZ, metres

// clip = transform * (pos, 1): rows x, y, z, w; W x H viewport, GL rows
struct StreamView {
  float m[4][4];
  int W, H;
};

// one GL_LINEAR level of w x h texels for canopy_bilinear
__host__ __device__ inline CanopyMips stream_level(int w, int h) {
  CanopyMips M = {};
  M.n = 1;
  M.w[0] = w;
  M.h[0] = h;
  return M;
}

// tab = sRGB -> linear per code; texel = (B, G, R, 0): the output's channel order, cameraFS replaces the alpha
__global__ void k_stream_texture(const uchar4* __restrict__ rgba, const float* __restrict__ tab, size_t n,
                                 float4* __restrict__ tex) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) {
    return;
  }
  const uchar4 p = rgba[i];
  tex[i] = make_float4(tab[p.z], tab[p.y], tab[p.x], 0.0f);
}

// cameraMeshVS. vtx = abc per vertex; dirTab = kStreamDirections^2 directions (xyz + 0); cam = camera position
__global__ void k_stream_vertex(const float* __restrict__ vtx, unsigned n, float scaleX, float scaleY, float focalR,
                                const float4* __restrict__ dirTab, float camx, float camy, float camz, StreamView V,
                                float4* __restrict__ clip, float2* __restrict__ texVar) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) {
    return;
  }
  const float a = vtx[3 * (size_t)i], b = vtx[3 * (size_t)i + 1], c = vtx[3 * (size_t)i + 2];
  const float tu = scaleX * a, tv = scaleY * b;
  const float depth = focalR / c;
  const float kD = (float)kStreamDirections;
  const float su = (0.5f + tu * (kD - 1.0f)) / kD, sv = (0.5f + tv * (kD - 1.0f)) / kD;
  const float4 d = canopy_bilinear(dirTab, stream_level(kStreamDirections, kStreamDirections), 0, su, sv);
  const float x = camx + depth * d.x, y = camy + depth * d.y, z = camz + depth * d.z;
  float o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    o[r] = ((V.m[r][0] * x + V.m[r][1] * y) + V.m[r][2] * z) + V.m[r][3];
  }
  clip[i] = make_float4(o[0], o[1], o[2], o[3]);
  texVar[i] = make_float2(tu, tv);
}

// Edge k runs from vertex k + 1 to vertex k + 2 (mod 3). With h = (window x * w, window y * w, w) per vertex, the edge
// function of pixel centre (px, py) is e[k] = (px a[k] + py b[k]) + c[k] = det(p, h[k+1], h[k+2]) for p = (px, py, 1).
// Reversing an edge negates a, b and c exactly, so two triangles sharing an edge compute e and -e: no gap, no overlap.
// The coefficients are negated when det < 0, so inside is e >= 0 for either winding.
struct StreamTri {
  float a[3], b[3], c[3], det;
  float tu[3], tv[3];
  float hx[3], hy[3], hw[3];
};

__device__ __forceinline__ bool stream_finite4(float4 p) {
  return isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w);
}

// false: the triangle is skipped (two equal indices, a non-finite clip coordinate or coefficient, wholly behind the near
// plane, no area)
__device__ __forceinline__ bool stream_setup(const float4* __restrict__ clip, const float2* __restrict__ texVar,
                                             const unsigned* __restrict__ idx, unsigned t, int W, int H, StreamTri& T) {
  const unsigned i[3] = {idx[3 * (size_t)t], idx[3 * (size_t)t + 1], idx[3 * (size_t)t + 2]};
  if (i[0] == i[1] || i[1] == i[2] || i[0] == i[2]) {
    return false;
  }
  bool front = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float4 p = clip[i[k]];
    if (!stream_finite4(p)) {
      return false;
    }
    T.hx[k] = (p.x + p.w) * 0.5f * (float)W;
    T.hy[k] = (p.y + p.w) * 0.5f * (float)H;
    T.hw[k] = p.w;
    front = front || p.w >= kStreamNear;
    const float2 tv = texVar[i[k]];
    T.tu[k] = tv.x;
    T.tv[k] = tv.y;
  }
  if (!front) {
    return false;
  }
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
    T.a[k] = T.hy[k1] * T.hw[k2] - T.hw[k1] * T.hy[k2];
    T.b[k] = T.hw[k1] * T.hx[k2] - T.hx[k1] * T.hw[k2];
    T.c[k] = T.hx[k1] * T.hy[k2] - T.hy[k1] * T.hx[k2];
    finite = finite && isfinite(T.a[k]) && isfinite(T.b[k]) && isfinite(T.c[k]);
  }
  T.det = (T.hx[0] * T.a[0] + T.hy[0] * T.b[0]) + T.hw[0] * T.c[0];
  if (!finite || !isfinite(T.det) || T.det == 0.0f) {
    return false;
  }
  if (T.det < 0.0f) {
    T.det = -T.det;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      T.a[k] = -T.a[k];
      T.b[k] = -T.b[k];
      T.c[k] = -T.c[k];
    }
  }
  return true;
}

// e[k] and their sum s at pixel centre (px, py). 1 / w = s / det and the perspective-correct weights are e[k] / s.
__device__ __forceinline__ float stream_edges(const StreamTri& T, float px, float py, float (&e)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    e[k] = (px * T.a[k] + py * T.b[k]) + T.c[k];
  }
  return (e[0] + e[1]) + e[2];
}

// Coverage of pixel (i, j) of the triangle's box (stream_box): inside every edge, where a centre exactly on an edge belongs to the triangle for which
// a > 0, or a == 0 and b > 0 (the shared edge's other triangle has the negated pair); in front of the near plane.
// -> 1 / w of the fragment, or 0 when it is not covered.
__device__ __forceinline__ float stream_cover(const StreamTri& T, int i, int j) {
  float e[3];
  const float s = stream_edges(T, (float)i + 0.5f, (float)j + 0.5f, e);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const bool owner = T.a[k] > 0.0f || (T.a[k] == 0.0f && T.b[k] > 0.0f);
    if (!(e[k] > 0.0f || (e[k] == 0.0f && owner))) {
      return 0.0f;
    }
  }
  if (!(s > 0.0f)) {
    return 0.0f;
  }
  const float iw = s / T.det;
  const float w = 1.0f / iw;
  return (iw > 0.0f && w >= kStreamNear) ? iw : 0.0f;
}

// The box of pixels a triangle is rasterised in, which is part of the coverage rule (the restatement computes the same
// box): the window positions of the vertices with w >= near / 2 and of the points where its edges cross w = near / 2,
// each grown by a margin, cut to the viewport. The margin is what fp32 can put between the edge functions' coverage
// and these positions: 1 + 2^-22 max(W, H)^2 pixels for the edge functions themselves (their coefficients are
// products of window-sized numbers: 2 pixels at 2048, 1 at the sizes of the tests), 1e-6 of a projected position, and
// for a crossing point, which is interpolated from the end nearer the plane so that a far vertex does not cancel,
// 1e-5 of the magnitudes that went into it (2^-24 times the 20 of the division by near / 2, times the six roundings).
// Half the near distance, because 1 / w of a fragment carries the relative error of det, which a thin or distant
// triangle computes with cancellation. A position that is not finite: the whole viewport. false: empty.
__device__ __forceinline__ bool stream_box(const StreamTri& T, int W, int H, int& i0, int& j0, int& i1, int& j1) {
  const float inf = __builtin_huge_valf(), cut = kStreamNear * 0.5f;
  const float side = (float)max(W, H), base = 1.0f + side * side * 0x1p-22f;
  float minx = inf, maxx = -inf, miny = inf, maxy = -inf;
  bool whole = false;
  auto take = [&](float x, float y, float mx, float my) {
    const float x0 = x - mx, x1 = x + mx, y0 = y - my, y1 = y + my;
    whole = whole || !(isfinite(x0) && isfinite(x1) && isfinite(y0) && isfinite(y1));
    minx = fminf(minx, x0);
    maxx = fmaxf(maxx, x1);
    miny = fminf(miny, y0);
    maxy = fmaxf(maxy, y1);
  };
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int n = (k + 1) % 3;
    if (T.hw[k] >= cut) {
      const float px = T.hx[k] / T.hw[k], py = T.hy[k] / T.hw[k];
      take(px, py, base + 1e-6f * fabsf(px), base + 1e-6f * fabsf(py));
    }
    if ((T.hw[k] >= cut) != (T.hw[n] >= cut)) {
      const bool first = fabsf(T.hw[k] - cut) <= fabsf(T.hw[n] - cut);
      const int a = first ? k : n, b = first ? n : k;  // a: the end nearer the plane
      const float f = (cut - T.hw[a]) / (T.hw[b] - T.hw[a]);
      const float tx = f * (T.hx[b] - T.hx[a]), ty = f * (T.hy[b] - T.hy[a]);
      take((T.hx[a] + tx) / cut, (T.hy[a] + ty) / cut, base + 1e-5f * (fabsf(T.hx[a]) + fabsf(tx)),
           base + 1e-5f * (fabsf(T.hy[a]) + fabsf(ty)));
    }
  }
  if (whole) {
    minx = miny = 0.0f;
    maxx = (float)W;
    maxy = (float)H;
  }
  const float lox = fmaxf(minx, 0.0f), hix = fminf(maxx, (float)W);
  const float loy = fmaxf(miny, 0.0f), hiy = fminf(maxy, (float)H);
  if (!(lox <= hix && loy <= hiy)) {
    return false;
  }
  i0 = (int)ceilf(lox - 0.5f);
  i1 = min(W - 1, (int)floorf(hix - 0.5f));
  j0 = (int)ceilf(loy - 0.5f);
  j1 = min(H - 1, (int)floorf(hiy - 0.5f));
  return i0 <= i1 && j0 <= j1;
}

// GL_LESS on the eye depth in the camera's own buffer; of equal depths the triangle that comes first in the index buffer
// stays: atomicMax of (1 / w bits, ~triangle), independent of the order of arrival. 0 = nothing rendered.
__device__ __forceinline__ void stream_fragment(const StreamTri& T, int i, int j, int W, unsigned t,
                                                unsigned long long* __restrict__ zbuf) {
  const float iw = stream_cover(T, i, j);
  if (iw > 0.0f) {
    atomicMax(&zbuf[(size_t)j * W + i], ((unsigned long long)__float_as_uint(iw) << 32) | (0xffffffffu - t));
  }
}

// One thread per triangle. A box of more than kCanopyBigTri pixels goes to `big` as {triangle, i0 | j0 << 16,
// i1 | j1 << 16, 0}; the list has room for every triangle, so none is dropped.
__global__ void k_stream_raster(const float4* __restrict__ clip, const float2* __restrict__ texVar,
                                const unsigned* __restrict__ idx, unsigned nTri, int W, int H,
                                unsigned long long* __restrict__ zbuf, uint4* __restrict__ big, unsigned* __restrict__ nBig) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nTri) {
    return;
  }
  StreamTri T;
  int i0, j0, i1, j1;
  if (!stream_setup(clip, texVar, idx, t, W, H, T) || !stream_box(T, W, H, i0, j0, i1, j1)) {
    return;
  }
  if ((long long)(i1 - i0 + 1) * (j1 - j0 + 1) > kCanopyBigTri) {
    big[atomicAdd(nBig, 1u)] = make_uint4(t, (unsigned)i0 | (unsigned)j0 << 16, (unsigned)i1 | (unsigned)j1 << 16, 0u);
    return;
  }
  for (int j = j0; j <= j1; ++j) {
    for (int i = i0; i <= i1; ++i) {
      stream_fragment(T, i, j, W, t, zbuf);
    }
  }
}

// grid (x, kStreamBigSplit): block (bx, by) takes the listed triangles bx, bx + gridDim.x, ... and of each box the
// pixels by * 256 + thread, + kStreamBigSplit * 256, ...; a box with fewer pixels than by * 256 costs it one load.
// The viewport is at most 32768 x 16384 (derp_stream_render), so the box corners fit 16 bits.
__global__ void __launch_bounds__(256)
    k_stream_raster_big(const float4* __restrict__ clip, const float2* __restrict__ texVar, const unsigned* __restrict__ idx,
                        int W, int H, unsigned long long* __restrict__ zbuf, const uint4* __restrict__ big,
                        const unsigned* __restrict__ nBig) {
  const unsigned count = *nBig;
  for (unsigned b = blockIdx.x; b < count; b += gridDim.x) {
    const uint4 entry = big[b];
    const int i0 = entry.y & 0xffff, j0 = entry.y >> 16, i1 = entry.z & 0xffff, j1 = entry.z >> 16;
    const int bw = i1 - i0 + 1;
    const long long area = (long long)bw * (j1 - j0 + 1);
    const long long first = (long long)blockIdx.y * blockDim.x;
    if (first >= area) {
      continue;
    }
    StreamTri T;
    stream_setup(clip, texVar, idx, entry.x, W, H, T);
    for (long long p = first + threadIdx.x; p < area; p += (long long)gridDim.y * blockDim.x) {
      stream_fragment(T, i0 + (int)(p % bw), j0 + (int)(p / bw), W, entry.x, zbuf);
    }
  }
}

// The winner's fragment: texVar interpolated perspective-correctly, cameraFS (texture rgb, cone alpha), stored as the
// camera buffer stores it (GL_RGBA16), then exponentialFS and the blend of updateAccumulation:
// acc.rgb += w rgb, acc.a += w with w = exp(30 a) - 1. tex = tw x th linear texels.
__global__ void k_stream_resolve(const float4* __restrict__ clip, const float2* __restrict__ texVar,
                                 const unsigned* __restrict__ idx, const float4* __restrict__ tex, int tw, int th, int W,
                                 int H, const unsigned long long* __restrict__ zbuf, float4* __restrict__ acc) {
  __shared__ unsigned long long expTab[32];
  {
    const int t = threadIdx.y * blockDim.x + threadIdx.x;
    if (t < 32) {
      expTab[t] = kExp2fTab[t];
    }
  }
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= W || j >= H) {
    return;
  }
  const unsigned long long key = zbuf[(size_t)j * W + i];
  if (!key) {
    return;
  }
  StreamTri T;
  stream_setup(clip, texVar, idx, 0xffffffffu - (unsigned)key, W, H, T);
  float e[3];
  const float s = stream_edges(T, (float)i + 0.5f, (float)j + 0.5f, e);
  const float u = ((e[0] * T.tu[0] + e[1] * T.tu[1]) + e[2] * T.tu[2]) / s;
  const float v = ((e[0] * T.tv[0] + e[1] * T.tv[1]) + e[2] * T.tv[2]) / s;
  const float4 c = canopy_bilinear(tex, stream_level(tw, th), 0, u, v);
  const float du = u - 0.5f, dv = v - 0.5f;
  const float cone = fmaxf(1.0f / 255.0f, 1.0f - 2.0f * sqrtf(du * du + dv * dv));
  const float weight = expf_glibc(30.0f * smr_unorm16(cone), expTab) - 1.0f;
  float4 a = acc[(size_t)j * W + i];
  a.x = weight * smr_unorm16(c.x) + a.x;
  a.y = weight * smr_unorm16(c.y) + a.y;
  a.z = weight * smr_unorm16(c.z) + a.z;
  a.w = weight + a.w;
  acc[(size_t)j * W + i] = a;
}

// resolveFS: rgb = fade * acc.rgb / acc.a; alpha = acc.a / acc.a, so a pixel no camera covered is NaN in every channel
// (this group's convention). GL row j -> row (flip ? H - 1 - j : j) of `out`.
__global__ void k_stream_finish(const float4* __restrict__ acc, int W, int H, float fade, int zeroNans, int flip,
                                float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= W || j >= H) {
    return;
  }
  const float4 a = acc[(size_t)j * W + i];
  float4 o = make_float4(fade * a.x / a.w, fade * a.y / a.w, fade * a.z / a.w, a.w / a.w);
  if (zeroNans) {
    o.x = o.x != o.x ? 0.0f : o.x;
    o.y = o.y != o.y ? 0.0f : o.y;
    o.z = o.z != o.z ? 0.0f : o.z;
    o.w = o.w != o.w ? 0.0f : o.w;
  }
  out[(size_t)(flip ? H - 1 - j : j) * W + i] = o;
}

}  // namespace derp
