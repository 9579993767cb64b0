// SimpleMeshRenderer's GPU stages — CanopyScene::render / cubemap / equirect (source/render/CanopyScene.cpp:36-69,
// 72-160, 195-266, 288-475) for any view, DisparityColor.h:18-57 and the compositing of SimpleMeshRenderer.cpp:265-330,
// 407-437. The rasteriser is the rephotography renderer's (derp_kernels.h k_canopy_*): same triangles, depth key,
// barycentrics, derivatives and texture filter (canopy_bary / canopy_grad / canopy_sample / k_canopy_mip), with
//   - a general view: eye = R (p - c), depth d = -eye.z, window = ((k * eye.xy / d + 1) / 2) * size (SmrView);
//   - a texture of its own size (float BGRA quantised to GL_RGBA16, alpha = alphaFov on the texture's size),
//     texVar = (vertex index + 0.5) / mesh size;
//   - canopyFS_SVD (sigma2 / sigma1 * cone) or canopyFS (minor * cone) as the fragment weight;
//   - accumulateFS with or without alphaBlend; unpremulFS with or without the rephotography's NaN -> 0;
//   - canopyVS's stereo displacement, once per (camera, eye) in k_smr_stereo.
// Choices where OpenGL is implementation-defined: DESIGN.md §8 "SimpleMeshRenderer". fp32 like the shaders.
#pragma once

namespace derp {

// eye = R (p - c); rows of R: screen x, screen y, backwards (the GL eye looks along -z). ndc = k * eye.xy / d,
// d = -eye.z; a triangle with a vertex at d < 0.1 m (kNearZ) is dropped, not clipped. W x H viewport, GL rows.
struct SmrView {
  float R[3][3];
  float c[3];
  float kx, ky;
  int W, H;
};

__device__ __forceinline__ float smr_dot(const float (&r)[3], const float (&q)[3]) {
  return (r[0] * q[0] + r[1] * q[1]) + r[2] * q[2];
}

// triangle t of quad (qx, qy) of a w x h mesh (t = 0: A B C, t = 1: B C D as in canopy_setup) in view V
__device__ __forceinline__ bool smr_setup(const float4* __restrict__ vert, int w, int h, int qx, int qy, int t,
                                          const SmrView& V, CanopyTri& T) {
  const float scaleX = (float)(1.0 / (double)w), scaleY = (float)(1.0 / (double)h);  // Canopy::scale
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int ox = t == 0 ? (k == 2) : (k >= 1), oy = t == 0 ? (k == 1) : (k != 1);
    const int vx = qx + ox, vy = qy + oy;
    const float4 p = vert[(size_t)vy * w + vx];
    if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) {
      return false;
    }
    const float q[3] = {p.x - V.c[0], p.y - V.c[1], p.z - V.c[2]};
    const float ex = smr_dot(V.R[0], q), ey = smr_dot(V.R[1], q), d = -smr_dot(V.R[2], q);
    if (!(d >= 0.1f)) {  // kNearZ
      return false;
    }
    T.sx[k] = ((V.kx * ex) / d + 1.0f) * 0.5f * (float)V.W;
    T.sy[k] = ((V.ky * ey) / d + 1.0f) * 0.5f * (float)V.H;
    T.invd[k] = 1.0f / d;
    T.tu[k] = scaleX * ((float)vx + 0.5f);
    T.tv[k] = scaleY * ((float)vy + 0.5f);
  }
  T.area = (T.sx[1] - T.sx[0]) * (T.sy[2] - T.sy[0]) - (T.sx[2] - T.sx[0]) * (T.sy[1] - T.sy[0]);
  return T.area != 0.0f && isfinite(T.area);
}

// disparityMesh (CanopyScene.cpp:447-460): the vertex of every disparity pixel, as k_canopy_mesh computes it
__global__ void k_smr_mesh(const Cam* __restrict__ cams, int s, const float* __restrict__ disp, int w, int h,
                           float4* __restrict__ vert) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) {
    return;
  }
  const Cam& c = cams[s];
  const size_t i = (size_t)y * w + x;
  const double px = (x + 0.5) / (double)w, py = (y + 0.5) / (double)h;
  const float distance = 1.0f / disp[i];
  const D3 dir = rig_direction(c, px, py, c.principal[0], c.principal[1], c.focal[0], c.focal[1]);
  const double depth = (double)distance;
  vert[i] = make_float4((float)(c.pos[0] + dir.x * depth), (float)(c.pos[1] + dir.y * depth),
                        (float)(c.pos[2] + dir.z * depth), 0.0f);
}

// Canopy::Canopy's texture (GL_RGBA16 from float BGRA: clamp to [0, 1], round to nearest even, NaN -> 0) with
// alphaFov's alpha on the texture's own size (CanopyScene.cpp:15-20, 462-476). bgra == nullptr: the disparity
// colour of DisparityColor.h:18-57 instead, from the mesh of the same size: 1 / |vertex - position|, alpha 1.
__device__ __forceinline__ float smr_unorm16(float v) {
  const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;  // NaN -> 0
  return rintf(c * 65535.0f) / 65535.0f;
}
__global__ void k_smr_texture(const Cam* __restrict__ cams, int s, const float4* __restrict__ bgra,
                              const float4* __restrict__ vert, float px0, float py0, float pz0, int tw, int th,
                              float4* __restrict__ tex) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= tw || y >= th) {
    return;
  }
  const size_t i = (size_t)y * tw + x;
  float4 v;
  if (bgra) {
    v = bgra[i];
  } else {
    const float4 p = vert[i];
    const float dx = p.x - px0, dy = p.y - py0, dz = p.z - pz0;
    const float dsp = 1.0f / sqrtf((dx * dx + dy * dy) + dz * dz);  // metersToGrayscale(norm)
    v = make_float4(dsp, dsp, dsp, 1.0f);
  }
  const Cam& c = cams[s];
  const double px = (x + 0.5) / (double)tw, py = (y + 0.5) / (double)th;
  const float a = outside_image_circle(c, px, py, c.principal[0], c.principal[1], c.focal[0], c.focal[1]) ? 0.0f : 1.0f;
  tex[i] = make_float4(smr_unorm16(v.x), smr_unorm16(v.y), smr_unorm16(v.z), a);
}

// canopyVS's stereo vertex stage (CanopyScene.cpp:73-160) for ipdm != 0: pos -= eye(pos). fp32 with the device's
// expf / atanf / sqrtf; no host twin is bit-exact, so the checker consumes these vertices (derp_render_vertices).
__device__ __forceinline__ float smr_ipd(float ipdm, float lat) {
  const float kPi = 3.1415926535897932384626433832795f, kA = 25.0f, kB = 0.17f;
  return ipdm * expf(-expf(kA * (kB - 0.5f - lat / kPi)) - expf(kA * (kB - 0.5f + lat / kPi)));
}
__device__ __forceinline__ float smr_sq(float x) {
  return x * x;
}
__device__ __forceinline__ float smr_error(float x, float y, float z, float dEst, float ipdm) {
  return (x * x + y * y) - smr_sq(smr_ipd(ipdm, atanf(z / dEst)) / 2.0f) - smr_sq(dEst);
}
__global__ void k_smr_stereo(const float4* __restrict__ in, size_t n, float ipdm, float4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) {
    return;
  }
  const float4 p = in[i];
  const float xy2 = p.x * p.x + p.y * p.y;
  float d0 = sqrtf(xy2 - smr_sq(smr_ipd(ipdm, atanf(p.z / sqrtf(xy2)))));
  for (int it = 0; it < 2; ++it) {
    const float kSmidgen = 1e-3f;
    const float d1 = (1.0f + kSmidgen) * d0;
    const float e0 = smr_error(p.x, p.y, p.z, d0, ipdm), e1 = smr_error(p.x, p.y, p.z, d1, ipdm);
    const float de = (e1 - e0) / (d1 - d0);
    d0 -= e0 / de;
  }
  const float eNorm = smr_ipd(ipdm, atanf(p.z / d0)) / 2.0f;
  const float k = -d0 / eNorm;
  // inverse(mat2(1, k, -k, 1)) * p.xy
  const float det = 1.0f + k * k;
  const float ex = (p.x + k * p.y) / det, ey = (p.y - k * p.x) / det;
  out[i] = make_float4(p.x - ex, p.y - ey, p.z, 0.0f);
}

__device__ __forceinline__ void smr_fragment(const CanopyTri& T, const float4* __restrict__ rgba, const CanopyMips& M,
                                             int i, int j, int W, unsigned triId, unsigned long long* __restrict__ zbuf) {
  float l[3];
  if (!canopy_bary(T, i + 0.5f, j + 0.5f, l, true)) {
    return;
  }
  const float iz = canopy_invz(T, l);
  if (!(iz > 0.0f)) {
    return;
  }
  float u, v, ax, ay, bx, by;
  canopy_grad(T, i, j, u, v, ax, ay, bx, by);
  if (canopy_sample(rgba, M, u, v, ax, ay, bx, by).w == 0.0f) {
    return;  // discard
  }
  atomicMax(&zbuf[(size_t)j * W + i], ((unsigned long long)__float_as_uint(iz) << 32) | triId);
}

// k_canopy_raster / _big for view V: small triangles one per thread, big ones (> kCanopyBigTri pixels) one per workgroup
__global__ void k_smr_raster(const float4* __restrict__ vert, int w, int h, const float4* __restrict__ rgba, CanopyMips M,
                             SmrView V, unsigned long long* __restrict__ zbuf, unsigned* __restrict__ big,
                             unsigned* __restrict__ nBig) {
  const int qx = blockIdx.x * blockDim.x + threadIdx.x, qy = blockIdx.y * blockDim.y + threadIdx.y;
  const int t = blockIdx.z;
  if (qx + 1 >= w || qy + 1 >= h) {
    return;
  }
  CanopyTri T;
  if (!smr_setup(vert, w, h, qx, qy, t, V, T)) {
    return;
  }
  const float minx = fminf(T.sx[0], fminf(T.sx[1], T.sx[2])), maxx = fmaxf(T.sx[0], fmaxf(T.sx[1], T.sx[2]));
  const float miny = fminf(T.sy[0], fminf(T.sy[1], T.sy[2])), maxy = fmaxf(T.sy[0], fmaxf(T.sy[1], T.sy[2]));
  if (!(maxx >= 0.0f && maxy >= 0.0f && minx <= (float)V.W && miny <= (float)V.H)) {
    return;
  }
  const int i0 = max(0, (int)ceilf(minx - 0.5f)), i1 = min(V.W - 1, (int)floorf(maxx - 0.5f));
  const int j0 = max(0, (int)ceilf(miny - 0.5f)), j1 = min(V.H - 1, (int)floorf(maxy - 0.5f));
  if (i1 < i0 || j1 < j0) {
    return;
  }
  const unsigned triId = (unsigned)(((size_t)qy * w + qx) * 2 + t);
  if ((long long)(i1 - i0 + 1) * (j1 - j0 + 1) > kCanopyBigTri) {
    big[atomicAdd(nBig, 1u)] = triId;
    return;
  }
  for (int j = j0; j <= j1; ++j) {
    for (int i = i0; i <= i1; ++i) {
      smr_fragment(T, rgba, M, i, j, V.W, triId, zbuf);
    }
  }
}
__global__ void __launch_bounds__(256)
    k_smr_raster_big(const float4* __restrict__ vert, int w, int h, const float4* __restrict__ rgba, CanopyMips M, SmrView V,
                     unsigned long long* __restrict__ zbuf, const unsigned* __restrict__ big,
                     const unsigned* __restrict__ nBig) {
  const unsigned count = *nBig;
  for (unsigned b = blockIdx.x; b < count; b += gridDim.x) {
    const unsigned triId = big[b];
    const int t = triId & 1, q = triId >> 1, qx = q % w, qy = q / w;
    CanopyTri T;
    if (!smr_setup(vert, w, h, qx, qy, t, V, T)) {
      continue;
    }
    const float minx = fminf(T.sx[0], fminf(T.sx[1], T.sx[2])), maxx = fmaxf(T.sx[0], fmaxf(T.sx[1], T.sx[2]));
    const float miny = fminf(T.sy[0], fminf(T.sy[1], T.sy[2])), maxy = fmaxf(T.sy[0], fmaxf(T.sy[1], T.sy[2]));
    const int i0 = max(0, (int)ceilf(minx - 0.5f)), i1 = min(V.W - 1, (int)floorf(maxx - 0.5f));
    const int j0 = max(0, (int)ceilf(miny - 0.5f)), j1 = min(V.H - 1, (int)floorf(maxy - 0.5f));
    const int bw = i1 - i0 + 1;
    const long long area = (long long)bw * (j1 - j0 + 1);
    for (long long p = threadIdx.x; p < area; p += blockDim.x) {
      smr_fragment(T, rgba, M, i0 + (int)(p % bw), j0 + (int)(p / bw), V.W, triId, zbuf);
    }
  }
}

// winner's fragment colour and weight, accumulated (accumulateFS + glBlendFuncSeparate(GL_SRC_ALPHA, GL_ONE, GL_ONE,
// GL_ONE)). svd != 0: canopyFS_SVD's sigma2 / sigma1, else canopyFS's minor axis. blend != 0: weight = exp(30 a) - 1,
// else the alpha itself.
__global__ void k_smr_resolve(const float4* __restrict__ vert, int w, int h, const float4* __restrict__ rgba, CanopyMips M,
                              SmrView V, int svd, int blend, const unsigned long long* __restrict__ zbuf,
                              float4* __restrict__ acc) {
  __shared__ unsigned long long expTab[32];
  {
    const int t = threadIdx.y * blockDim.x + threadIdx.x;
    if (t < 32) {
      expTab[t] = kExp2fTab[t];
    }
  }
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= V.W || j >= V.H) {
    return;
  }
  const unsigned long long key = zbuf[(size_t)j * V.W + i];
  if (!key) {
    return;
  }
  const unsigned triId = (unsigned)key;
  const int t = triId & 1, q = triId >> 1, qx = q % w, qy = q / w;
  CanopyTri T;
  smr_setup(vert, w, h, qx, qy, t, V, T);
  float u, v, ax, ay, bx, by;
  canopy_grad(T, i, j, u, v, ax, ay, bx, by);
  const float4 c = canopy_sample(rgba, M, u, v, ax, ay, bx, by);
  float alpha = c.w;
  if (svd) {
    const float s1 = ((ax * ax + ay * ay) + bx * bx) + by * by;
    const float sb = ((ax * ax + ay * ay) - bx * bx) - by * by;
    const float sc = ax * bx + ay * by;
    const float s2 = sqrtf(sb * sb + 4.0f * sc * sc);
    const float sigma1 = sqrtf((s1 + s2) / 2.0f), sigma2 = sqrtf((s1 - s2) / 2.0f);
    alpha *= sigma2 / sigma1;
  } else {
    const float aa = ax * ax + ay * ay, bb = bx * bx + by * by, ab = ax * bx + ay * by;
    const float hx = (aa - bb) / 2.0f;
    alpha *= (aa + bb) / 2.0f - sqrtf(hx * hx + ab * ab);
  }
  const float du = u - 0.5f, dv = v - 0.5f;
  alpha *= fmaxf(1.0f / 255.0f, 1.0f - 2.0f * sqrtf(du * du + dv * dv));
  const float weight = blend ? expf_glibc(30.0f * alpha, expTab) - 1.0f : alpha;
  float4 a = acc[(size_t)j * V.W + i];
  a.x = weight * c.x + a.x;
  a.y = weight * c.y + a.y;
  a.z = weight * c.z + a.z;
  a.w = weight + a.w;
  acc[(size_t)j * V.W + i] = a;
}

// unpremulFS: colour / alpha; zeroNans = ComputeRephotographyErrors' zeroOutNans. GL row j -> row (flip ? H - 1 - j : j)
// of `out` (row pitch W).
__global__ void k_smr_finish(const float4* __restrict__ acc, int W, int H, int zeroNans, int flip, float4* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= W || j >= H) {
    return;
  }
  const float4 a = acc[(size_t)j * W + i];
  float4 o = make_float4(a.x / a.w, a.y / a.w, a.z / a.w, a.w / a.w);
  if (zeroNans) {
    o.x = o.x != o.x ? 0.0f : o.x;
    o.y = o.y != o.y ? 0.0f : o.y;
    o.z = o.z != o.z ? 0.0f : o.z;
    o.w = o.w != o.w ? 0.0f : o.w;
  }
  out[(size_t)(flip ? H - 1 - j : j) * W + i] = o;
}

// ---- cube -> equirect (equirectFS + CanopyScene::equirect, CanopyScene.cpp:416-475) ----
// cube = six E x E faces in GL rows (texel row t * E), face order +X -X +Y -Y +Z -Z (kCubeAxes).
// texel (i, j) of `face`, with i or j possibly one texel outside the face: GL_TEXTURE_CUBE_MAP_SEAMLESS reads the
// adjacent face's texel. The texel centre's direction, in half-texel units, has the out-of-range axis at E + 1 > E:
// that axis is the neighbour's major axis, and the neighbour's texel follows exactly in integers.
__device__ __forceinline__ int smr_cube_texel(int face, int i, int j, int E) {
  if (i >= 0 && i < E && j >= 0 && j < E) {
    return (face * E + j) * E + i;
  }
  int q[3];
  q[kCubeAxes[face][0][0]] = kCubeAxes[face][0][1] * E;
  q[kCubeAxes[face][1][0]] = kCubeAxes[face][1][1] * (2 * i + 1 - E);
  q[kCubeAxes[face][2][0]] = kCubeAxes[face][2][1] * (2 * j + 1 - E);
  const int M = E + 1;
  int nf = 0;
  for (int f = 0; f < 6; ++f) {
    if (kCubeAxes[f][0][1] * q[kCubeAxes[f][0][0]] == M) {
      nf = f;
    }
  }
  const int sc = kCubeAxes[nf][1][1] * q[kCubeAxes[nf][1][0]], tc = kCubeAxes[nf][2][1] * q[kCubeAxes[nf][2][0]];
  const int ni = min(E - 1, (int)(((long long)(sc + M) * E) / (2 * M)));
  const int nj = min(E - 1, (int)(((long long)(tc + M) * E) / (2 * M)));
  return (nf * E + nj) * E + ni;
}
__global__ void k_smr_equirect(const float4* __restrict__ cube, int E, const float* __restrict__ lonTab,
                               const float* __restrict__ latTab, int W, int H, float4* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= W || r >= H) {
    return;
  }
  // lonTab = {cos, sin}(lon(x)) per column, latTab = {cos, sin}(lat(r)) per row, rounded from double on the host
  const float cl = latTab[2 * r], sl = latTab[2 * r + 1];
  const float d[3] = {cl * lonTab[2 * x], cl * lonTab[2 * x + 1], sl};
  const float a0 = fabsf(d[0]), a1 = fabsf(d[1]), a2 = fabsf(d[2]);
  const int axis = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);  // ties: x, then y, then z
  const int face = 2 * axis + (d[axis] >= 0.0f ? 0 : 1);
  const float ma = fabsf(d[axis]);
  const float sc = (float)kCubeAxes[face][1][1] * d[kCubeAxes[face][1][0]];
  const float tc = (float)kCubeAxes[face][2][1] * d[kCubeAxes[face][2][0]];
  const float s = (sc / ma + 1.0f) * 0.5f, t = (tc / ma + 1.0f) * 0.5f;
  const float u = s * (float)E - 0.5f, v = t * (float)E - 0.5f;
  const float x0f = floorf(u), y0f = floorf(v);
  const float fa = u - x0f, fb = v - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  float4 tap[4];
  int corner = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ti = x0 + (k & 1), tj = y0 + (k >> 1);
    if ((ti < 0 || ti >= E) && (tj < 0 || tj >= E)) {
      corner = k;
      tap[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      tap[k] = cube[smr_cube_texel(face, ti, tj, E)];
    }
  }
  if (corner >= 0) {  // the corner texel that no face holds: the average of the three others
    const float4 p = tap[(corner + 1) & 3], q = tap[(corner + 2) & 3], w = tap[(corner + 3) & 3];
    tap[corner] = make_float4(((p.x + q.x) + w.x) / 3.0f, ((p.y + q.y) + w.y) / 3.0f, ((p.z + q.z) + w.z) / 3.0f,
                              ((p.w + q.w) + w.w) / 3.0f);
  }
  auto lerp2 = [&](float p00, float p10, float p01, float p11) {
    const float top = p00 * (1.0f - fa) + p10 * fa, bot = p01 * (1.0f - fa) + p11 * fa;
    return top * (1.0f - fb) + bot * fb;
  };
  out[(size_t)r * W + x] = make_float4(lerp2(tap[0].x, tap[1].x, tap[2].x, tap[3].x), lerp2(tap[0].y, tap[1].y, tap[2].y, tap[3].y),
                                       lerp2(tap[0].z, tap[1].z, tap[2].z, tap[3].z), lerp2(tap[0].w, tap[1].w, tap[2].w, tap[3].w));
}

// ---- compositing (SimpleMeshRenderer.cpp:265-330) ----
// alphaBlend: a NaN alpha takes the background, else fore * a + back * (1 - a), alpha a + (1 - a) back.a
__device__ __forceinline__ float4 smr_over(float4 f, float4 b) {
  const float a = f.w;
  if (a != a) {
    return b;
  }
  return make_float4(a * f.x + (1.0f - a) * b.x, a * f.y + (1.0f - a) * b.y, a * f.z + (1.0f - a) * b.z,
                     a + (1.0f - a) * b.w);
}
__global__ void k_smr_alpha_blend(float4* __restrict__ img, const float4* __restrict__ back, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    img[i] = smr_over(img[i], back[i]);
  }
}
// backgroundEquirect: pixels with alpha != 1 take the nearest texel of the background equirect along their snapshot
// ray. fetch = (row, col) per output pixel, computed on the host (the reference's atan2 / asin), clamped to the image.
__global__ void k_smr_background_equirect(float4* __restrict__ img, const int* __restrict__ fetch, size_t n,
                                          const float4* __restrict__ equi, int ew) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) {
    return;
  }
  const float4 f = img[i];
  if (f.w == 1.0f) {
    return;
  }
  img[i] = smr_over(f, equi[(size_t)fetch[2 * i] * ew + fetch[2 * i + 1]]);
}

}  // namespace derp
