// The fp64 arithmetic of MeshSimplifier.cpp's set-up and collapse loop, once, for the device kernels (derp_mesh.h) and
// the host simplifier (derp_simplify.cpp). The reference writes these with Eigen, whose evaluation order is not
// readable from its sources here, so one order is fixed (implementation-defined; the tests'
// restatement tests/mesh_ref.py uses the same):
//   squaredNorm / dot of 3-vectors: a0 + (a1 + a2), like derp_camera.h's sum3
//   cross(u, v): (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)
//   3x3 determinant: cofactor expansion along the first row, (a m0 - b m1) + c m2
//   normalized(): v / sqrt(squaredNorm) when squaredNorm > 0, else v
// computeFastError is plain C++ in the reference and keeps its left-to-right order. Nothing here may be contracted
// into an FMA: the library and every harness build with -ffp-contract=off.
#pragma once
#include <cmath>

#if defined(__HIP__)
#define MESH_HD __host__ __device__ inline
#else
#define MESH_HD inline
#endif

namespace derp_mesh {

struct V3 {
  double x, y, z;
};
// a symmetric 4x4 quadric: q00 q01 q02 q03 q11 q12 q13 q22 q23 q33
constexpr int kQuadric = 10;

MESH_HD V3 sub(const V3& a, const V3& b) {
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
MESH_HD double dot(const V3& a, const V3& b) {
  return a.x * b.x + (a.y * b.y + a.z * b.z);
}
MESH_HD double squared_norm(const V3& a) {
  return dot(a, a);
}
MESH_HD V3 cross(const V3& u, const V3& v) {
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
MESH_HD V3 normalized(const V3& a) {
  const double n2 = squared_norm(a);
  if (n2 > 0) {
    const double n = sqrt(n2);
    return {a.x / n, a.y / n, a.z / n};
  }
  return a;
}
MESH_HD double det3(double a, double b, double c, double d, double e, double f, double g, double h, double i) {
  return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}

// computeSubQuadrics (MeshSimplifier.cpp:182-195): the unit normal of a face and its plane q = [n, -n.p0]
MESH_HD void face_plane(const V3& p0, const V3& p1, const V3& p2, double q4[4]) {
  const V3 n = normalized(cross(sub(p1, p0), sub(p2, p0)));
  q4[0] = n.x;
  q4[1] = n.y;
  q4[2] = n.z;
  q4[3] = -dot(n, p0);
}
// vertex.q += q qT, the ten distinct entries
MESH_HD void add_plane_quadric(double* Q, const double q4[4]) {
  int k = 0;
  for (int i = 0; i < 4; ++i) {
    for (int j = i; j < 4; ++j) {
      Q[k] = Q[k] + q4[i] * q4[j];
      ++k;
    }
  }
}

// computeFastError (:103-107), as written
MESH_HD double fast_error(const double* q, const V3& v) {
  return q[0] * v.x * v.x + 2 * q[1] * v.x * v.y + 2 * q[2] * v.x * v.z + 2 * q[3] * v.x + q[4] * v.y * v.y +
         2 * q[5] * v.y * v.z + 2 * q[6] * v.y + q[7] * v.z * v.z + 2 * q[8] * v.z + q[9];
}

// MeshSimplifier::computeError (:132-170)
MESH_HD double compute_error(const double* q0, const double* q1, const V3& c0, const V3& c1, bool isBoundary,
                             bool equiError, V3& target) {
  double q[kQuadric];
  for (int k = 0; k < kQuadric; ++k) {
    q[k] = q0[k] + q1[k];
  }
  const double det = det3(q[0], q[1], q[2], q[1], q[4], q[5], q[2], q[5], q[7]);
  double error;
  if (det != 0 && !isBoundary) {
    const double mX = det3(q[1], q[2], q[3], q[4], q[5], q[6], q[5], q[7], q[8]);
    const double mY = det3(q[0], q[2], q[3], q[1], q[5], q[6], q[2], q[7], q[8]);
    const double mZ = det3(q[0], q[1], q[3], q[1], q[4], q[6], q[2], q[5], q[8]);
    const double s = 1 / det;
    target = {s * -mX, s * mY, s * -mZ};
    error = fast_error(q, target);
  } else {
    const V3 cand[3] = {c0, c1, {(c0.x + c1.x) / 2, (c0.y + c1.y) / 2, (c0.z + c1.z) / 2}};
    double errors[3];
    int best = 0;  // std::min_element: the first of the smallest
    for (int k = 0; k < 3; ++k) {
      errors[k] = fast_error(q, cand[k]);
      if (errors[k] < errors[best]) {
        best = k;
      }
    }
    target = cand[best];
    error = errors[best];
  }
  return equiError ? error : error / squared_norm(target);
}

}  // namespace derp_mesh
