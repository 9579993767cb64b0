// CPU restatement of SimpleMeshRenderer's GPU stages (facebook360_dep_amd/csrc/derp_render.h), for the tests:
// CanopyScene::render for a cube face or a snapshot view, canopyFS_SVD / canopyFS weights, accumulateFS with and
// without alphaBlend, unpremulFS with and without the rephotography's NaN -> 0, colour textures of their own size,
// disparity colours (DisparityColor.h), the seamless cube -> equirect of CanopyScene::equirect and the compositing of
// SimpleMeshRenderer.cpp:265-330. It reuses oracle_canopy.h's rasteriser primitives (barycentrics, derivatives,
// texture filter, mip chain) and states only what is new; it shares no source with the product. Built by
// tests/test_smr_checker.py / tests/test_gpu_simple_mesh_renderer.py with g++ and loaded through ctypes.
// chk_render_stats also counts what a render met (enum Stat): tests/test_render_cases.py shows with it that a case
// reaches the branch it is there for. chk_background_equirect restates backgroundEquirect from the reference's text.
// The stereo vertex stage has no bit-exact host twin (GLSL exp / atan): the caller passes the device's displaced
// vertices in `verts`, so everything downstream of them is compared bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../oracle/oracle_canopy.h"

using namespace oracle;

namespace {

struct View {
  float R[3][3];
  float c[3];
  float kx, ky;
  int W, H;
};

struct F3 {
  float x, y, z;
};
F3 cross(F3 a, F3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
F3 normalized(F3 a) {
  const float n = std::sqrt((a.x * a.x + a.y * a.y) + a.z * a.z);
  return {a.x / n, a.y / n, a.z / n};
}

View snapshotView(const double* pos, const double* fwdD, const double* upD, double fov, int W, int H) {
  View V;
  const F3 fwd = {(float)fwdD[0], (float)fwdD[1], (float)fwdD[2]}, up = {(float)upD[0], (float)upD[1], (float)upD[2]};
  const F3 right = cross(up, F3{-fwd.x, -fwd.y, -fwd.z});
  const F3 f = normalized(fwd), u = normalized(cross(right, fwd)), nf = {-f.x, -f.y, -f.z};
  const F3 r = cross(u, nf);
  const F3 rows[3] = {r, u, nf};
  for (int k = 0; k < 3; ++k) {
    V.R[k][0] = rows[k].x;
    V.R[k][1] = rows[k].y;
    V.R[k][2] = rows[k].z;
    V.c[k] = (float)pos[k];
  }
  const float n = 0.1f, xMax = (float)(0.1f * std::tan(fov / 180 * M_PI / 2)), yMax = xMax * H / W;
  V.kx = 2 * n / (xMax - -xMax);
  V.ky = 2 * n / (yMax - -yMax);
  V.W = W;
  V.H = H;
  return V;
}

View faceView(const double* pos, int face, int E) {
  View V;
  std::memset(&V, 0, sizeof V);
  V.R[0][kCubeAxes[face][1][0]] = (float)kCubeAxes[face][1][1];
  V.R[1][kCubeAxes[face][2][0]] = (float)kCubeAxes[face][2][1];
  V.R[2][kCubeAxes[face][0][0]] = (float)-kCubeAxes[face][0][1];
  for (int k = 0; k < 3; ++k) {
    V.c[k] = (float)pos[k];
  }
  V.kx = V.ky = 1.0f;
  V.W = V.H = E;
  return V;
}

float dot3(const float r[3], const float q[3]) {
  return (r[0] * q[0] + r[1] * q[1]) + r[2] * q[2];
}

// The product rasterises a triangle whose clamped bounding box holds more than kCanopyBigTri = 64 pixels with a
// workgroup of its own (derp_kernels.h); this mirrors that constant. It only classifies triangles for the statistics
// below, which the tests use to show that a case reaches both rasterisers: no image value depends on it.
constexpr int kBigTriPixels = 64;

// what one chk_render_stats call met, summed over the rendered canopies and faces (tests/smr_check.py STATS)
enum Stat {
  kTriSmall,       // triangles rasterised with a clamped bounding box of <= kBigTriPixels pixels
  kTriBig,         // ... of more
  kPixSmall,       // covered pixels won by a small triangle
  kPixBig,         // ... by a big one
  kDisplaced,      // pixels at which a triangle of one class took the depth test from a winner of the other class
  kIdTies,         // pixels decided by the triangle id: the winner's depth bits came from two triangles
  kNearDrops,      // triangles dropped by the near plane with at least one vertex at d >= 0.1 (all vertices finite)
  kAlphaDiscards,  // fragments discarded by a filtered alpha of 0
  kSuspect,        // inside fragments whose u, v or a derivative is non-finite or above 2^31 in magnitude
  kMipAbove0,      // fragments whose filter read a mip level above 0
  kNumStats
};
struct Stats {
  uint64_t n[kNumStats];
};

struct Canopy {
  int w, h;                 // mesh
  std::vector<float> v;     // [h][w][4]
  CanopyMesh tex;           // the texture and its mips (tex.w x tex.h)
};

bool setup(const Canopy& m, int qx, int qy, int t, const View& V, CanopyTri& T) {
  static const int off[2][3][2] = {{{0, 0}, {0, 1}, {1, 0}}, {{0, 1}, {1, 0}, {1, 1}}};
  const float scaleX = (float)(1.0 / m.w), scaleY = (float)(1.0 / m.h);
  for (int k = 0; k < 3; ++k) {
    const int vx = qx + off[t][k][0], vy = qy + off[t][k][1];
    const float* p = &m.v[((size_t)vy * m.w + vx) * 4];
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) {
      return false;
    }
    const float q[3] = {p[0] - V.c[0], p[1] - V.c[1], p[2] - V.c[2]};
    const float ex = dot3(V.R[0], q), ey = dot3(V.R[1], q), d = -dot3(V.R[2], q);
    if (!(d >= 0.1f)) {
      return false;
    }
    T.sx[k] = ((V.kx * ex) / d + 1.0f) * 0.5f * (float)V.W;
    T.sy[k] = ((V.ky * ey) / d + 1.0f) * 0.5f * (float)V.H;
    T.invd[k] = 1.0f / d;
    T.tu[k] = scaleX * ((float)vx + 0.5f);
    T.tv[k] = scaleY * ((float)vy + 0.5f);
  }
  T.area = (T.sx[1] - T.sx[0]) * (T.sy[2] - T.sy[0]) - (T.sx[2] - T.sx[0]) * (T.sy[1] - T.sy[0]);
  return T.area != 0.0f && std::isfinite(T.area);
}

// setup() refused the triangle: was it the near plane, with a vertex in front of it?
bool nearDropped(const Canopy& m, int qx, int qy, int t, const View& V) {
  static const int off[2][3][2] = {{{0, 0}, {0, 1}, {1, 0}}, {{0, 1}, {1, 0}, {1, 1}}};
  int front = 0;
  for (int k = 0; k < 3; ++k) {
    const float* p = &m.v[((size_t)(qy + off[t][k][1]) * m.w + qx + off[t][k][0]) * 4];
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) {
      return false;
    }
    const float q[3] = {p[0] - V.c[0], p[1] - V.c[1], p[2] - V.c[2]};
    front += -dot3(V.R[2], q) >= 0.1f;
  }
  return front > 0 && front < 3;
}

// canopySample's level choice: does it read a level above 0?
bool aboveLevel0(const CanopyMesh& m, float ax, float ay, float bx, float by) {
  const float axT = ax * (float)m.w, ayT = ay * (float)m.h, bxT = bx * (float)m.w, byT = by * (float)m.h;
  const float px2 = axT * axT + ayT * ayT, py2 = bxT * bxT + byT * byT;
  const float pMax = std::sqrt(px2 >= py2 ? px2 : py2), pMin = std::sqrt(px2 >= py2 ? py2 : px2);
  if (!(pMax > 0.0f) || !std::isfinite(pMax)) {
    return false;
  }
  int n = kCanopyMaxAniso;
  if (pMin > 0.0f) {
    const float r = std::ceil(pMax / pMin);
    n = r < (float)kCanopyMaxAniso ? (int)r : kCanopyMaxAniso;
  }
  return pMax / (float)n > 1.0f && m.mipW.size() > 1;
}

bool suspect(float x) {
  return !(std::fabs(x) <= 2147483648.0f);
}

float unorm16(float v) {
  const float c = v > 0.0f ? (v < 1.0f ? v : 1.0f) : 0.0f;
  return std::nearbyint(c * 65535.0f) / 65535.0f;
}

// accumulate one canopy into acc (CanopyScene::render's loop body)
void renderCanopy(const Canopy& m, const View& V, bool svd, bool blend, std::vector<float>& acc, Stats* st) {
  const size_t nf = (size_t)V.W * V.H;
  std::vector<uint64_t> zbuf(nf, 0);
  // statistics only: the winner's class, whether it displaced the other class, the depth bits two triangles shared
  std::vector<uint8_t> cls(st ? nf : 0, 0), displaced(st ? nf : 0, 0);
  std::vector<uint32_t> tied(st ? nf : 0, 0);
  for (int qy = 0; qy + 1 < m.h; ++qy) {
    for (int qx = 0; qx + 1 < m.w; ++qx) {
      for (int t = 0; t < 2; ++t) {
        CanopyTri T;
        if (!setup(m, qx, qy, t, V, T)) {
          if (st && nearDropped(m, qx, qy, t, V)) {
            ++st->n[kNearDrops];
          }
          continue;
        }
        const float minx = std::min(T.sx[0], std::min(T.sx[1], T.sx[2])), maxx = std::max(T.sx[0], std::max(T.sx[1], T.sx[2]));
        const float miny = std::min(T.sy[0], std::min(T.sy[1], T.sy[2])), maxy = std::max(T.sy[0], std::max(T.sy[1], T.sy[2]));
        if (!(maxx >= 0.0f && maxy >= 0.0f && minx <= (float)V.W && miny <= (float)V.H)) {
          continue;
        }
        const int i0 = std::max(0, (int)std::ceil(minx - 0.5f)), i1 = std::min(V.W - 1, (int)std::floor(maxx - 0.5f));
        const int j0 = std::max(0, (int)std::ceil(miny - 0.5f)), j1 = std::min(V.H - 1, (int)std::floor(maxy - 0.5f));
        const uint32_t triId = (uint32_t)(((size_t)qy * m.w + qx) * 2 + t);
        const bool big = i1 >= i0 && j1 >= j0 && (long long)(i1 - i0 + 1) * (j1 - j0 + 1) > kBigTriPixels;
        if (st && i1 >= i0 && j1 >= j0) {
          ++st->n[big ? kTriBig : kTriSmall];
        }
        for (int j = j0; j <= j1; ++j) {
          for (int i = i0; i <= i1; ++i) {
            float l[3];
            if (!canopyBary(T, i + 0.5f, j + 0.5f, l, true)) {
              continue;
            }
            const float iz = canopyInvZ(T, l);
            if (!(iz > 0.0f)) {
              continue;
            }
            float u, v, ax, ay, bx, by, c[4];
            canopyGrad(T, i, j, u, v, ax, ay, bx, by);
            canopySample(m.tex, u, v, ax, ay, bx, by, c);
            if (st) {
              st->n[kSuspect] += suspect(u) || suspect(v) || suspect(ax) || suspect(ay) || suspect(bx) || suspect(by);
              st->n[kMipAbove0] += aboveLevel0(m.tex, ax, ay, bx, by);
              st->n[kAlphaDiscards] += c[3] == 0.0f;
            }
            if (c[3] == 0.0f) {
              continue;
            }
            uint32_t bits;
            std::memcpy(&bits, &iz, 4);
            const size_t px = (size_t)j * V.W + i;
            uint64_t& slot = zbuf[px];
            const uint64_t key = ((uint64_t)bits << 32) | triId;
            if (st) {
              if (slot && (uint32_t)(slot >> 32) == bits) {
                tied[px] = bits;
              }
              if (key > slot) {
                displaced[px] |= slot && cls[px] != (uint8_t)big;
                cls[px] = big;
              }
            }
            slot = std::max(slot, key);
          }
        }
      }
    }
  }
  for (int j = 0; j < V.H; ++j) {
    for (int i = 0; i < V.W; ++i) {
      const uint64_t key = zbuf[(size_t)j * V.W + i];
      if (!key) {
        continue;
      }
      const uint32_t triId = (uint32_t)key;
      if (st) {
        const size_t px = (size_t)j * V.W + i;
        ++st->n[cls[px] ? kPixBig : kPixSmall];
        st->n[kDisplaced] += displaced[px];
        st->n[kIdTies] += tied[px] == (uint32_t)(key >> 32);
      }
      const int t = triId & 1, q = triId >> 1, qx = q % m.w, qy = q / m.w;
      CanopyTri T;
      setup(m, qx, qy, t, V, T);
      float u, v, ax, ay, bx, by, c[4];
      canopyGrad(T, i, j, u, v, ax, ay, bx, by);
      canopySample(m.tex, u, v, ax, ay, bx, by, c);
      float alpha = c[3];
      if (svd) {  // canopyFS_SVD, CanopyScene.cpp:195-229
        const float s1 = ((ax * ax + ay * ay) + bx * bx) + by * by;
        const float sb = ((ax * ax + ay * ay) - bx * bx) - by * by;
        const float sc = ax * bx + ay * by;
        const float s2 = std::sqrt(sb * sb + 4.0f * sc * sc);
        const float sigma1 = std::sqrt((s1 + s2) / 2.0f), sigma2 = std::sqrt((s1 - s2) / 2.0f);
        alpha *= sigma2 / sigma1;
      } else {
        const float aa = ax * ax + ay * ay, bb = bx * bx + by * by, ab = ax * bx + ay * by;
        const float hx = (aa - bb) / 2.0f;
        alpha *= (aa + bb) / 2.0f - std::sqrt(hx * hx + ab * ab);
      }
      const float du = u - 0.5f, dv = v - 0.5f;
      alpha *= std::max(1.0f / 255.0f, 1.0f - 2.0f * std::sqrt(du * du + dv * dv));
      const float weight = blend ? std::exp(30.0f * alpha) - 1.0f : alpha;
      float* a = &acc[((size_t)j * V.W + i) * 4];
      a[0] = weight * c[0] + a[0];
      a[1] = weight * c[1] + a[1];
      a[2] = weight * c[2] + a[2];
      a[3] = weight + a[3];
    }
  }
}

void renderView(const std::vector<Canopy>& cans, const View& V, bool svd, bool blend, bool zeroNans, bool flip, float* out,
                Stats* st) {
  std::vector<float> acc((size_t)V.W * V.H * 4, 0.0f);
  for (const Canopy& m : cans) {
    renderCanopy(m, V, svd, blend, acc, st);
  }
  for (int j = 0; j < V.H; ++j) {
    for (int i = 0; i < V.W; ++i) {
      const float* a = &acc[((size_t)j * V.W + i) * 4];
      float* o = out + ((size_t)(flip ? V.H - 1 - j : j) * V.W + i) * 4;
      for (int c = 0; c < 4; ++c) {
        const float v = a[c] / a[3];
        o[c] = zeroNans && v != v ? 0.0f : v;
      }
    }
  }
}

// GL_TEXTURE_CUBE_MAP_SEAMLESS: a texel one step outside face `face` is the adjacent face's edge texel. In half-texel
// units the texel centre's direction has the outside axis at E + 1, which names the neighbour; its texel follows.
size_t cubeTexel(int face, int i, int j, int E) {
  if (i >= 0 && i < E && j >= 0 && j < E) {
    return ((size_t)face * E + j) * E + i;
  }
  int q[3];
  q[kCubeAxes[face][0][0]] = kCubeAxes[face][0][1] * E;
  q[kCubeAxes[face][1][0]] = kCubeAxes[face][1][1] * (2 * i + 1 - E);
  q[kCubeAxes[face][2][0]] = kCubeAxes[face][2][1] * (2 * j + 1 - E);
  const int M = E + 1;
  int nf = -1;
  for (int f = 0; f < 6; ++f) {
    if (kCubeAxes[f][0][1] * q[kCubeAxes[f][0][0]] == M) {
      nf = f;
    }
  }
  const int sc = kCubeAxes[nf][1][1] * q[kCubeAxes[nf][1][0]], tc = kCubeAxes[nf][2][1] * q[kCubeAxes[nf][2][0]];
  const int ni = std::min(E - 1, (int)(((long long)(sc + M) * E) / (2 * M)));
  const int nj = std::min(E - 1, (int)(((long long)(tc + M) * E) / (2 * M)));
  return ((size_t)nf * E + nj) * E + ni;
}

void equirect(const float* cube, int E, float* out) {
  const int W = 2 * E, H = E;
  std::vector<float> lon(2 * W), lat(2 * H);
  for (int x = 0; x < W; ++x) {
    const double a = (1 - (x + 0.5) / W) * 2.0 * M_PI;
    lon[2 * x] = (float)std::cos(a);
    lon[2 * x + 1] = (float)std::sin(a);
  }
  for (int r = 0; r < H; ++r) {
    const double a = -((r + 0.5) / H - 0.5) * M_PI;
    lat[2 * r] = (float)std::cos(a);
    lat[2 * r + 1] = (float)std::sin(a);
  }
  for (int r = 0; r < H; ++r) {
    for (int x = 0; x < W; ++x) {
      const float d[3] = {lat[2 * r] * lon[2 * x], lat[2 * r] * lon[2 * x + 1], lat[2 * r + 1]};
      const float a0 = std::fabs(d[0]), a1 = std::fabs(d[1]), a2 = std::fabs(d[2]);
      const int axis = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
      const int face = 2 * axis + (d[axis] >= 0.0f ? 0 : 1);
      const float ma = std::fabs(d[axis]);
      const float sc = (float)kCubeAxes[face][1][1] * d[kCubeAxes[face][1][0]];
      const float tc = (float)kCubeAxes[face][2][1] * d[kCubeAxes[face][2][0]];
      const float s = (sc / ma + 1.0f) * 0.5f, t = (tc / ma + 1.0f) * 0.5f;
      const float u = s * (float)E - 0.5f, v = t * (float)E - 0.5f;
      const float x0f = std::floor(u), y0f = std::floor(v);
      const float fa = u - x0f, fb = v - y0f;
      const int x0 = (int)x0f, y0 = (int)y0f;
      float tap[4][4];
      int corner = -1;
      for (int k = 0; k < 4; ++k) {
        const int ti = x0 + (k & 1), tj = y0 + (k >> 1);
        if ((ti < 0 || ti >= E) && (tj < 0 || tj >= E)) {
          corner = k;
        } else {
          std::memcpy(tap[k], cube + cubeTexel(face, ti, tj, E) * 4, 16);
        }
      }
      if (corner >= 0) {
        const float *p = tap[(corner + 1) & 3], *q = tap[(corner + 2) & 3], *w = tap[(corner + 3) & 3];
        for (int c = 0; c < 4; ++c) {
          tap[corner][c] = ((p[c] + q[c]) + w[c]) / 3.0f;
        }
      }
      for (int c = 0; c < 4; ++c) {
        const float top = tap[0][c] * (1.0f - fa) + tap[1][c] * fa, bot = tap[2][c] * (1.0f - fa) + tap[3][c] * fa;
        out[((size_t)r * W + x) * 4 + c] = top * (1.0f - fb) + bot * fb;
      }
    }
  }
}

}  // namespace

extern "C" {

// kind 0 cube (stacked, flipped), 1 equirect, 2 snapshot (flipped); verts[s] (xyzw [dh][dw][4]) or NULL: disparityMesh;
// stats: kNumStats counters (enum Stat) or NULL
int chk_render_stats(const CameraJson* cams, int n, const uint8_t* include, const float* const* tex, const int* tw, const int* th,
               const float* const* disp, const int* dw, const int* dh, const float* const* verts, int kind, int width,
               int height, const double* position, const double* forward, const double* up, double fov, int alphaBlend,
               int dispColor, int weightMinor, int zeroNans, float* out, uint64_t* stats) {
  Stats counters, *st = stats ? &counters : nullptr;
  std::memset(&counters, 0, sizeof counters);
  const float pos[3] = {(float)position[0], (float)position[1], (float)position[2]};
  std::vector<Canopy> cans;
  for (int s = 0; s < n; ++s) {
    if (include && !include[s]) {
      continue;
    }
    Camera cam(cams[s]);
    if (!cam.isNormalized()) {
      cam.normalize();
    }
    Canopy m;
    m.w = dw[s];
    m.h = dh[s];
    m.v.resize((size_t)m.w * m.h * 4);
    std::vector<float> mono((size_t)m.w * m.h * 3);
    for (int y = 0; y < m.h; ++y) {
      for (int x = 0; x < m.w; ++x) {
        const size_t i = (size_t)y * m.w + x;
        const float distance = 1.0f / disp[s][i];
        const V3 rig = cam.rig({(x + 0.5) / m.w, (y + 0.5) / m.h}, (double)distance);
        mono[3 * i] = (float)rig.x;
        mono[3 * i + 1] = (float)rig.y;
        mono[3 * i + 2] = (float)rig.z;
        for (int c = 0; c < 3; ++c) {
          m.v[4 * i + c] = verts ? verts[s][4 * i + c] : mono[3 * i + c];
        }
        m.v[4 * i + 3] = 0.0f;
      }
    }
    CanopyMesh& t = m.tex;
    t.w = dispColor ? m.w : tw[s];
    t.h = dispColor ? m.h : th[s];
    t.rgba.resize((size_t)t.w * t.h * 4);
    for (int y = 0; y < t.h; ++y) {
      for (int x = 0; x < t.w; ++x) {
        const size_t i = (size_t)y * t.w + x;
        float bgr[3];
        if (dispColor) {  // disparityColor + metersToGrayscale (DisparityColor.h:18-57)
          const float dx = mono[3 * i] - pos[0], dy = mono[3 * i + 1] - pos[1], dz = mono[3 * i + 2] - pos[2];
          const float d = 1.0f / std::sqrt((dx * dx + dy * dy) + dz * dz);
          bgr[0] = bgr[1] = bgr[2] = d;
        } else {
          for (int c = 0; c < 3; ++c) {
            bgr[c] = tex[s][4 * i + c];
          }
        }
        for (int c = 0; c < 3; ++c) {
          t.rgba[4 * i + c] = unorm16(bgr[c]);  // GL_RGBA16
        }
        t.rgba[4 * i + 3] = cam.isOutsideImageCircle({(x + 0.5) / t.w, (y + 0.5) / t.h}) ? 0.0f : 1.0f;  // alphaFov
      }
    }
    canopyBuildMips(t);
    cans.push_back(std::move(m));
  }
  const bool svd = !weightMinor, blend = alphaBlend != 0, zn = zeroNans != 0;
  if (kind == 2) {
    renderView(cans, snapshotView(position, forward, up, fov, width, height), svd, blend, zn, true, out, st);
    if (stats) {
      std::memcpy(stats, counters.n, sizeof counters.n);
    }
    return 0;
  }
  const int E = height;
  if (kind == 0) {
    for (int f = 0; f < 6; ++f) {
      renderView(cans, faceView(position, f, E), svd, blend, zn, true, out + (size_t)f * E * E * 4, st);
    }
    if (stats) {
      std::memcpy(stats, counters.n, sizeof counters.n);
    }
    return 0;
  }
  std::vector<float> cube((size_t)6 * E * E * 4);
  for (int f = 0; f < 6; ++f) {
    renderView(cans, faceView(position, f, E), svd, blend, zn, false, cube.data() + (size_t)f * E * E * 4, st);
  }
  equirect(cube.data(), E, out);
  if (stats) {
    std::memcpy(stats, counters.n, sizeof counters.n);
  }
  return 0;
}

int chk_render(const CameraJson* cams, int n, const uint8_t* include, const float* const* tex, const int* tw, const int* th,
               const float* const* disp, const int* dw, const int* dh, const float* const* verts, int kind, int width,
               int height, const double* position, const double* forward, const double* up, double fov, int alphaBlend,
               int dispColor, int weightMinor, int zeroNans, float* out) {
  return chk_render_stats(cams, n, include, tex, tw, th, disp, dw, dh, verts, kind, width, height, position, forward, up,
                          fov, alphaBlend, dispColor, weightMinor, zeroNans, out, nullptr);
}

int chk_num_stats() {
  return kNumStats;
}

// seamless cube -> equirect alone, on a given GL-row cube [6][E][E][4]
void chk_equirect(const float* cube, int E, float* out) {
  equirect(cube, E, out);
}

// alphaBlend (SimpleMeshRenderer.cpp:265-283), in place on fore
void chk_alpha_blend(float* fore, const float* back, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    float* f = fore + 4 * i;
    const float* b = back + 4 * i;
    const float a = f[3];
    if (std::isnan(a)) {
      std::memcpy(f, b, 16);
      continue;
    }
    for (int c = 0; c < 3; ++c) {
      f[c] = a * f[c] + (1 - a) * b[c];
    }
    f[3] = a + (1 - a) * b[3];
  }
}

// backgroundEquirect (SimpleMeshRenderer.cpp:285-322), in place on fore [h][w][4], written from the reference's text:
// transform = posForwardUp(position, forward, up) with translation = linear * -position; its general inverse (the
// 3 x 3 cofactor inverse, translation = -inverse * translation); per pixel with alpha != 1 the centre on the near
// plane scaled by kNearInfinity = 1e4, taken to the world, lon = atan2(-y, -x), lat = asin(z / |world|), and the
// texel equi(int(equiY), int(equiX)). The reference reads one past the last row / column when lat = -90 degrees or
// lon = -180 degrees; the index is clamped to the image here and *clamped counts the pixels where that decided.
void chk_background_equirect(float* fore, int w, int h, const float* equi, int ew, int eh, const double* position,
                             const double* forward, const double* up, double fov, uint64_t* clamped) {
  const View V = snapshotView(position, forward, up, fov, w, h);
  const float (&L)[3][3] = V.R;
  float t[3], inv[3][3], it[3];
  for (int k = 0; k < 3; ++k) {
    t[k] = (L[k][0] * -V.c[0] + L[k][1] * -V.c[1]) + L[k][2] * -V.c[2];
  }
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return L[i1][j1] * L[i2][j2] - L[i1][j2] * L[i2][j1];
  };
  const float det = (cof(0, 0) * L[0][0] + cof(1, 0) * L[1][0]) + cof(2, 0) * L[2][0];
  const float invdet = 1.0f / det;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      inv[j][i] = cof(i, j) * invdet;
    }
  }
  for (int k = 0; k < 3; ++k) {
    it[k] = -((inv[k][0] * t[0] + inv[k][1] * t[1]) + inv[k][2] * t[2]);
  }
  const float kNearZ = 0.1f;
  const float xMax = (float)(kNearZ * std::tan(fov / 180 * M_PI / 2));
  uint64_t nClamped = 0;
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) {
      float* f = fore + ((size_t)y * w + x) * 4;
      const float alpha = f[3];
      if (alpha == 1) {
        continue;
      }
      const float pixel[3] = {((x + 0.5f) / w * 2 - 1) * xMax, -((y + 0.5f) / h * 2 - 1) * xMax * h / w, -kNearZ};
      const float far[3] = {1e4f * pixel[0], 1e4f * pixel[1], 1e4f * pixel[2]};
      float world[3];
      for (int k = 0; k < 3; ++k) {
        world[k] = ((inv[k][0] * far[0] + inv[k][1] * far[1]) + inv[k][2] * far[2]) + it[k];
      }
      const float lon = std::atan2(-world[1], -world[0]);
      const float norm = std::sqrt((world[0] * world[0] + world[1] * world[1]) + world[2] * world[2]);
      const float lat = std::asin(world[2] / norm);
      const float equiX = (float)((-lon / M_PI + 1) / 2 * ew), equiY = (float)((-lat / M_PI + 0.5) * eh);
      const int ix = (int)equiX, iy = (int)equiY;
      const int cx = std::min(std::max(ix, 0), ew - 1), cy = std::min(std::max(iy, 0), eh - 1);
      nClamped += cx != ix || cy != iy;
      const float* back = equi + ((size_t)cy * ew + cx) * 4;
      if (std::isnan(alpha)) {
        std::memcpy(f, back, 16);
      } else {
        for (int c = 0; c < 3; ++c) {
          f[c] = alpha * f[c] + (1 - alpha) * back[c];
        }
        f[3] = alpha + (1 - alpha) * back[3];
      }
    }
  }
  if (clamped) {
    *clamped = nClamped;
  }
}

}  // extern "C"
