// The fp32 arithmetic of RigSimulator's tracer, once, for the device kernels (derp_sim.h) and the host scene unit
// (derp_sim_scene.cpp). The reference writes it with cv::Vec3f; OpenCV is not available to check against, so the widths
// below are stated choices read from OpenCV 4's core/matx.hpp:
//   a.dot(b)            float, ((0 + a0 b0) + a1 b1) + a2 b2                      (Matx::dot)
//   a.cross(b)          float, (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)      (Vec<float, 3>::cross)
//   v * float, float * v, v + w, v - w   float per component
//   v / float           float ialpha = 1.f / a; v * ialpha                        (operator/ (Vec, float))
//   v /= float          the same                                                  (operator/= (Vec, float))
//   v /= double         double ialpha = 1. / a; float(double(v_i) * ialpha)       (operator/= (Vec, double))
//   norm(v)             double: sqrt of the squares summed in double, in order    (normL2Sqr<float, double>)
// Nothing here may be contracted into an FMA: the library and every harness build with -ffp-contract=off.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/derp_hip.h"

#if defined(__HIP__)
#define SIM_HD __host__ __device__ inline
#else
#define SIM_HD inline
#endif

namespace derp_sim_math {

struct V3f {
  float x, y, z;
};
SIM_HD V3f f3(const float* p) {
  return {p[0], p[1], p[2]};
}
SIM_HD V3f add(const V3f& a, const V3f& b) {
  return {a.x + b.x, a.y + b.y, a.z + b.z};
}
SIM_HD V3f sub(const V3f& a, const V3f& b) {
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
SIM_HD V3f scale(const V3f& a, float s) {
  return {a.x * s, a.y * s, a.z * s};
}
SIM_HD float dot(const V3f& a, const V3f& b) {
  float s = 0;
  s += a.x * b.x;
  s += a.y * b.y;
  s += a.z * b.z;
  return s;
}
SIM_HD V3f cross(const V3f& a, const V3f& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
SIM_HD double norm(const V3f& a) {
  double s = 0;
  s += (double)a.x * (double)a.x;
  s += (double)a.y * (double)a.y;
  s += (double)a.z * (double)a.z;
  return sqrt(s);
}
SIM_HD V3f div_float(const V3f& a, float alpha) {
  const float ialpha = 1.f / alpha;
  return scale(a, ialpha);
}
SIM_HD V3f div_double(const V3f& a, double alpha) {
  const double ialpha = 1. / alpha;
  return {(float)((double)a.x * ialpha), (float)((double)a.y * ialpha), (float)((double)a.z * ialpha)};
}

// rayIntersectSphereYesNo, RaytracingPrimitives.h:90-110. A NaN sphere (the empty scene's) misses: every comparison
// with NaN is false up to `halfCord2 >= 0`.
SIM_HD bool ray_hits_sphere(const V3f& o, const V3f& d, const derp_sim_node& s) {
  const V3f c = sub(f3(s.center), o);
  const float len2 = c.x * c.x + c.y * c.y + c.z * c.z;
  if (len2 < s.radius * s.radius) {
    return true;
  }
  const float closest = dot(c, d);
  if (closest < 0.0f) {
    return false;
  }
  const float halfCord2 = s.radius * s.radius + closest * closest - len2;
  return halfCord2 >= 0.0f;
}

// rayIntersectTriangle, RaytracingPrimitives.h:59-86
SIM_HD bool ray_hits_triangle(const V3f& o, const V3f& d, const derp_sim_triangle& t, float& dist) {
  const V3f e1 = f3(t.e1), e2 = f3(t.e2);
  const V3f q = cross(d, e2);
  const float a = dot(e1, q);
  if (a * a < 0.0001f) {
    return false;
  }
  const V3f s = div_float(sub(o, f3(t.v0)), a);
  const V3f r = cross(s, e1);
  const float b0 = dot(s, q);
  const float b1 = dot(r, d);
  const float b2 = 1.0f - b0 - b1;
  if (b0 < 0.0f || b1 < 0.0f || b2 < 0.0f) {
    return false;
  }
  dist = dot(e2, r);
  return !(dist < 0.0f);
}

// raytraceBVH, RigSimulator.cpp:169-193, on the pre-order flat tree: a sphere hit goes on to the next node (the first
// child, or the node behind a leaf), a miss to the skip link. Leaves and their triangles come in the recursion's
// depth-first order and a hit is kept only when it is strictly nearer, so the first of equal distances wins as it does
// through the reference's nested comparisons. No stack.
SIM_HD int trace_tree(const V3f& o, const V3f& d, const derp_sim_node* nodes, int nNodes, const int32_t* leaf,
                      const derp_sim_triangle* tris, float& best) {
  int hit = -1;
  best = FLT_MAX;
  int i = 0;
  while (i < nNodes) {
    const derp_sim_node nd = nodes[i];
    if (!ray_hits_sphere(o, d, nd)) {
      i = nd.skip;
      continue;
    }
    for (int k = 0; k < nd.count; ++k) {
      const int ti = leaf[nd.first + k];
      float dist;
      if (ray_hits_triangle(o, d, tris[ti], dist) && dist < best) {
        best = dist;
        hit = ti;
      }
    }
    ++i;
  }
  return hit;
}

// PerlinNoise.h:47-88 (Ken Perlin, "Improved Noise", 2002), float as the reference declares it; floor() resolves to
// the double function there, which changes nothing: x - floor(x) is exact in double and rounds to float once.
SIM_HD float perlin_fade(float t) {
  return t * t * t * (t * (t * 6 - 15) + 10);
}
SIM_HD float perlin_lerp(float t, float a, float b) {
  return a + t * (b - a);
}
SIM_HD float perlin_grad(int hash, float x, float y, float z) {
  const int h = hash & 15;
  const float u = h < 8 ? x : y;
  const float v = h < 4 ? y : h == 12 || h == 14 ? x : z;
  return ((h & 1) == 0 ? u : -u) + ((h & 2) == 0 ? v : -v);
}
// p: the permutation twice over, 512 entries
SIM_HD float perlin_noise(const uint8_t* p, float x, float y, float z) {
  const double fx = floor((double)x), fy = floor((double)y), fz = floor((double)z);
  const int X = (int)fx & 255, Y = (int)fy & 255, Z = (int)fz & 255;
  x = (float)((double)x - fx);
  y = (float)((double)y - fy);
  z = (float)((double)z - fz);
  const float u = perlin_fade(x), v = perlin_fade(y), w = perlin_fade(z);
  const int A = p[X] + Y, AA = p[A] + Z, AB = p[A + 1] + Z, B = p[X + 1] + Y, BA = p[B] + Z, BB = p[B + 1] + Z;
  return perlin_lerp(
      w,
      perlin_lerp(v, perlin_lerp(u, perlin_grad(p[AA], x, y, z), perlin_grad(p[BA], x - 1, y, z)),
                  perlin_lerp(u, perlin_grad(p[AB], x, y - 1, z), perlin_grad(p[BB], x - 1, y - 1, z))),
      perlin_lerp(v, perlin_lerp(u, perlin_grad(p[AA + 1], x, y, z - 1), perlin_grad(p[BA + 1], x - 1, y, z - 1)),
                  perlin_lerp(u, perlin_grad(p[AB + 1], x, y - 1, z - 1), perlin_grad(p[BB + 1], x - 1, y - 1, z - 1))));
}

// the shading of a geometry hit, RigSimulator.cpp:242-261: marble, then the Lambert term with the fixed light
SIM_HD V3f shade_hit(const V3f& o, const V3f& d, float dist, const derp_sim_triangle& t, bool marble, double marbleScale,
                    const uint8_t* perm) {
  V3f base = f3(t.color);
  const V3f p = add(o, scale(d, dist));
  if (marble) {
    const float n = perlin_noise(perm, (float)(marbleScale * (double)p.x), (float)(marbleScale * (double)p.y),
                                 (float)(marbleScale * (double)p.z));
    base = scale(base, 0.7f + 0.3f * fabsf(n));
  }
  const V3f light = {2.0f, 1.0f, 5.2f};
  V3f dir = sub(light, p);
  dir = div_double(dir, norm(dir));
  const float nd = dot(f3(t.normal), dir);
  const float coef = .25f + .75f * (0.0f < nd ? nd : 0.0f);  // std::max(0.0f, x): x when 0 < x
  return scale(base, coef);
}

}  // namespace derp_sim_math
