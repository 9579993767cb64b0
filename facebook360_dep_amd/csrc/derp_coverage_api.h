// RigAnalyzer (source/rig/RigAnalyzer.cpp), host side: the four coverage entry points on derp_ctx (kernels:
// derp_coverage.h) and the host-only rig construction and editing (Fibonacci directions, sweep distances, named
// arrangements, eulers, revolve, rotate, perturb, scale). Definitions: DESIGN §8.9. Included by derp_capi.hip after
// derp_sweep_api.h, whose sweep_unitarise (Camera::setRotation's re-unitarisation) the rig editing shares.
#pragma once

namespace {

struct CoverageState {
  DevBuf scams, units, distances, tables, counts, hist, timing;
};

// the cameras in their own pixel units: principal, focal and resolution as the rig file holds them
int coverage_begin(derp_ctx* c, const char* what, CoverageState** out) {
  if (!c) {
    return 1;
  }
  if (c->D > kCovMaxCams) {
    return fail(c, "%s: too many cameras (%d > %d): coverage counts are 8-bit", what, c->D, kCovMaxCams);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the call before this one may still read the buffers
  if (!c->coverage) {
    c->coverage.reset(new CoverageState);
    std::vector<ScaledCam> sc(c->D);
    for (int i = 0; i < c->D; ++i) {
      const derp_camera_desc& j = c->descDstH[i];
      sc[i] = {j.has_principal ? j.principal[0] : j.resolution[0] / 2, j.has_principal ? j.principal[1] : j.resolution[1] / 2,
               j.focal[0], j.focal[1], j.resolution[0], j.resolution[1]};
    }
    if (upload_sync(c, c->coverage->scams, sc.data(), sc.size() * sizeof(ScaledCam))) {
      c->coverage.reset();
      return 1;
    }
  }
  *out = c->coverage.get();
  return 0;
}

template <int GEN>
int coverage_image(derp_ctx* c, CoverageState& S, const CovPoints& P, size_t pixels, uint8_t* counts) {
  ALLOC(c, S.counts, pixels);
  {
    Span sp(c, ST_COVERAGE, 0);
    hipLaunchKernelGGL((k_coverage<GEN, false>), dim3(blocks_of(pixels, kCovBlock)), dim3(kCovBlock), 0, c->stream,
                       c->camsDst.as<Cam>(), S.scams.as<ScaledCam>(), c->D, P, pixels, S.counts.as<uint8_t>(), (int*)nullptr,
                       (float*)nullptr);
    KCHECK(c);
  }
  return download_sync(c, counts, S.counts.p, pixels);
}

// ---- Eigen's rotations as the reference's host code uses them (Eigen 3.3, Geometry module, scalar paths) ----
struct CovQuat {
  double w, x, y, z;
};
// Quaternion(AngleAxis): w = cos(angle / 2), vec = sin(angle / 2) * axis
CovQuat cov_quat(double angle, double ax, double ay, double az) {
  const double ha = 0.5 * angle, s = std::sin(ha);
  return {std::cos(ha), s * ax, s * ay, s * az};
}
// Quaternion * Quaternion, the generic product
CovQuat cov_mul(const CovQuat& a, const CovQuat& b) {
  return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
// Quaternion::toRotationMatrix, row-major
void cov_quat_matrix(const CovQuat& q, double* m) {
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  m[0] = 1 - (tyy + tzz);
  m[1] = txy - twz;
  m[2] = txz + twy;
  m[3] = txy + twz;
  m[4] = 1 - (txx + tzz);
  m[5] = tyz - twx;
  m[6] = txz - twy;
  m[7] = tyz + twx;
  m[8] = 1 - (txx + tyy);
}
// AngleAxis::toRotationMatrix, row-major (the arithmetic of host_prepare_camera)
void cov_aa_matrix(double angle, const double* a, double* R) {
  const double s = std::sin(angle), cs = std::cos(angle);
  const double sx = s * a[0], sy = s * a[1], sz = s * a[2];
  const double c1x = (1.0 - cs) * a[0], c1y = (1.0 - cs) * a[1], c1z = (1.0 - cs) * a[2];
  double t;
  t = c1x * a[1];
  R[1] = t - sz;
  R[3] = t + sz;
  t = c1x * a[2];
  R[2] = t + sy;
  R[6] = t - sy;
  t = c1y * a[2];
  R[5] = t - sx;
  R[7] = t + sx;
  R[0] = c1x * a[0] + cs;
  R[4] = c1y * a[1] + cs;
  R[8] = c1z * a[2] + cs;
}
// AngleAxis(matrix) = AngleAxis(Quaternion(matrix)), row-major m (the arithmetic of host_prepare_camera)
void cov_matrix_aa(const double* R, double* angle, double* axis) {
  const double m[3][3] = {{R[0], R[1], R[2]}, {R[3], R[4], R[5]}, {R[6], R[7], R[8]}};
  double q[4];
  double t = sum3(m[0][0], m[1][1], m[2][2]);
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) {
      i = 1;
    }
    if (m[2][2] > m[i][i]) {
      i = 2;
    }
    const int jj = (i + 1) % 3, kk = (jj + 1) % 3;
    t = std::sqrt(m[i][i] - m[jj][jj] - m[kk][kk] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[kk][jj] - m[jj][kk]) * t;
    q[jj] = (m[jj][i] + m[i][jj]) * t;
    q[kk] = (m[kk][i] + m[i][kk]) * t;
  }
  double n = std::sqrt(sum3(q[0] * q[0], q[1] * q[1], q[2] * q[2]));
  if (n != 0) {
    *angle = 2.0 * std::atan2(n, std::fabs(q[3]));
    if (q[3] < 0) {
      n = -n;
    }
    axis[0] = q[0] / n;
    axis[1] = q[1] / n;
    axis[2] = q[2] / n;
  } else {
    *angle = 0;
    axis[0] = 1;
    axis[1] = 0;
    axis[2] = 0;
  }
}
// rotationMatrixFromEulers (RigAnalyzer.cpp:96-101): (z * y * x) or (y * x * z) of the axis rotations, as a matrix
void cov_euler_matrix(const double* e, bool xyz, double* m) {
  const CovQuat x = cov_quat(e[0], 1, 0, 0), y = cov_quat(e[1], 0, 1, 0), z = cov_quat(e[2], 0, 0, 1);
  cov_quat_matrix(xyz ? cov_mul(cov_mul(z, y), x) : cov_mul(cov_mul(y, x), z), m);
}
void cov_apply(const double* m, double* v) {
  const double x = v[0], y = v[1], z = v[2];
  for (int r = 0; r < 3; ++r) {
    v[r] = sum3(m[3 * r] * x, m[3 * r + 1] * y, m[3 * r + 2] * z);
  }
}
double cov_norm(const double* v) {
  return std::sqrt(sum3(v[0] * v[0], v[1] * v[1], v[2] * v[2]));
}
// the cameras as Camera::Camera leaves them: forward / up / right through setRotation
int cov_load(const char* what, const derp_camera_desc* cams, int n, derp_camera_desc* out) {
  for (int i = 0; i < n; ++i) {
    out[i] = cams[i];
    if (const char* err = sweep_unitarise(out[i])) {
      return create_fail(std::string(what) + ": camera " + cams[i].id + ": " + err);
    }
  }
  return 0;
}
// position = m * position; setRotation(m * forward, m * up, m * right) (RigAnalyzer.cpp:146-147, :514-515, :533-534)
const char* cov_transform(derp_camera_desc& j, const double* m) {
  cov_apply(m, j.origin);
  cov_apply(m, j.forward);
  cov_apply(m, j.up);
  cov_apply(m, j.right);
  return sweep_unitarise(j);
}
void cov_set_id(derp_camera_desc& j, const std::string& id) {
  snprintf(j.id, sizeof j.id, "%s", id.c_str());
}

struct CovArrangement {
  const char* name;
  bool xyz;
  int custom;  // the first `custom` rows hold the custom angle `a` in place of their x (marked -1 below)
  double defaultAngle;  // a when --custom is -1; NaN: acos(-1 / 3.0) * 180 / pi (tetra)
  int n;
  double e[24][3];
};
// RigAnalyzer.cpp:157-238
const CovArrangement kCovArrangements[] = {
    {"ballcam24", false, 0, 0, 24,
     {{22.998, -36.1543, 132.267},    {-2.89381, -156.601, 168.482}, {-50.2907, -68.7384, 139.028},  {-80.2662, 172.721, 113.889},
      {57.5173, 87.6811, 161.596},    {6.46204, 162.32, 70.7419},    {21.8577, 118.439, 114.195},    {77.4316, -95.0674, -100.379},
      {-20.2739, 41.1554, -135.466},  {-38.2009, 172.776, -171.825}, {-0.841465, -110.909, 57.8619}, {-39.8563, -128.178, 46.3619},
      {-54.3882, 8.6561, -13.3586},   {24.3104, 51.5133, -20.0308},  {35.7198, -82.6713, 160.228},   {-48.4447, 85.1941, 93.5637},
      {48.4425, 165.464, 19.7297},    {-3.41527, 84.0526, 56.5226},  {-20.5666, -24.4286, 14.2745},  {35.8214, -139.006, -27.4138},
      {-8.22831, -69.3313, -46.6214}, {51.5282, 4.18718, -133.303},  {6.61383, 8.24745, -72.7674},   {-22.4038, 126.995, 13.7087}}},
    {"tetra", true, 3, NAN, 4, {{-1, 0, 0}, {-1, 0, 120}, {-1, 0, -120}, {0, 0, 0}}},
    {"tetratilted", false, 0, 0, 4,
     {{-35.2644, 45, -65.1818}, {-35.2644, -135, -137.834}, {35.2644, -45, -45.0048}, {35.2644, 135, -104.664}}},
    {"ring4", true, 4, 90, 4, {{-1, 0, 0}, {-1, 0, 90}, {-1, 0, 180}, {-1, 0, 270}}},
    {"cube", true, 4, 90, 6, {{-1, 0, 0}, {-1, 0, 90}, {-1, 0, 180}, {-1, 0, 270}, {0, 0, 0}, {180, 0, 0}}},
    {"carbon0", false, 0, 0, 6,
     {{-35.2644, 3.89537e-15, 112.232}, {-35.2644, 120, -67.3096}, {-35.2644, -120, 155.867},
      {35.2644, 180, 21.9328},          {35.2644, -60, 14.0236},   {35.2644, 60, 66.2737}}},
    {"carbon1", false, 0, 0, 6,
     {{-35.2644, 1.94768e-15, 133.504}, {-35.2644, 120, -179.989}, {-35.2644, -120, -134.51},
      {35.2644, 180, 89.7419},          {35.2644, -60, 43.7899},   {35.2644, 60, -45.1612}}},
    {"diamond", true, 3, 90, 5, {{-1, 0, 0}, {-1, 0, 120}, {-1, 0, 240}, {0, 0, 0}, {180, 0, 0}}},
};

}  // namespace

// ---- host only: no context and no device; a refusal leaves its text in derp_last_error(NULL) ----
// getFibonacciUnits + discardPoles (RigAnalyzer.cpp:68-94); the pole test is on z, as the reference writes it
int derp_rig_fibonacci_units(int count, double discard_poles_deg, double* out_xyz, int* kept) {
  if (count < 0 || !kept || (count > 0 && !out_xyz)) {
    return create_fail("derp_rig_fibonacci_units: bad arguments");
  }
  const double threshold = std::cos(discard_poles_deg * M_PI / 180);
  int k = 0;
  for (int i = 0; i < count; ++i) {
    const double y = (i + 0.5) / count * 2 - 1;
    const double r = std::sqrt(1 - y * y);
    const double phi = (1 + std::sqrt(5.0)) / 2;
    const double roty = i / phi * 2 * M_PI;
    const double p[3] = {std::sin(roty) * r, y, std::cos(roty) * r};
    if (std::fabs(p[2]) < threshold) {
      out_xyz[3 * k] = p[0];
      out_xyz[3 * k + 1] = p[1];
      out_xyz[3 * k + 2] = p[2];
      ++k;
    }
  }
  *kept = k;
  return 0;
}

// the N = 20 distances from min_distance towards infinity (RigAnalyzer.cpp:562-565)
int derp_rig_coverage_distances(double min_distance, double* out) {
  if (!out) {
    return create_fail("derp_rig_coverage_distances: bad arguments");
  }
  const int kN = DERP_RIG_COVERAGE_DISTANCES;
  for (int i = 0; i < kN; ++i) {
    const double frac = i / double(kN);
    out[i] = min_distance / (1 - frac);
  }
  return 0;
}

// rotationMatrixFromEulers (RigAnalyzer.cpp:96-101), radians -> row-major m9
int derp_rig_euler_matrix(const double* euler_rad, int xyz, double* m9) {
  if (!euler_rad || !m9) {
    return create_fail("derp_rig_euler_matrix: bad arguments");
  }
  cov_euler_matrix(euler_rad, xyz != 0, m9);
  return 0;
}

// --rotate_cam_z's rotation (RigAnalyzer.cpp:505-510): the angle-axis turn that takes `position` onto +z
int derp_rig_align_z_matrix(const double* position, double* m9) {
  if (!position || !m9) {
    return create_fail("derp_rig_align_z_matrix: bad arguments");
  }
  const double* p = position;
  const double angle = std::acos(sum3(p[0] * 0, p[1] * 0, p[2] * 1));
  double axis[3] = {p[1] * 1 - p[2] * 0, p[2] * 0 - p[0] * 1, p[0] * 0 - p[1] * 0};
  const double sq = sum3(axis[0] * axis[0], axis[1] * axis[1], axis[2] * axis[2]);
  if (sq > 0) {  // Eigen's normalize() leaves a zero vector alone
    const double len = std::sqrt(sq);
    for (double& v : axis) {
      v /= len;
    }
  }
  cov_aa_matrix(angle, axis, m9);
  return 0;
}

// makeRigFromEulers (RigAnalyzer.cpp:103-131): eulers in degrees, ids cam0, cam1, ...
int derp_rig_from_eulers(const derp_camera_desc* model, const double* eulers_deg, int n, int xyz, derp_camera_desc* out) {
  if (!model || !eulers_deg || !out || n < 1) {
    return create_fail("derp_rig_from_eulers: bad arguments");
  }
  const double radius = cov_norm(model->origin);
  for (int i = 0; i < n; ++i) {
    const double e[3] = {eulers_deg[3 * i] * (M_PI / 180), eulers_deg[3 * i + 1] * (M_PI / 180), eulers_deg[3 * i + 2] * (M_PI / 180)};
    double m[9];
    cov_euler_matrix(e, xyz != 0, m);
    derp_camera_desc& j = out[i];
    j = *model;
    for (int r = 0; r < 3; ++r) {  // setRotation(xform.col(2), xform.col(1), -xform.col(0))
      j.forward[r] = m[3 * r + 2];
      j.up[r] = m[3 * r + 1];
      j.right[r] = -m[3 * r];
    }
    if (const char* err = sweep_unitarise(j)) {
      return create_fail(std::string("derp_rig_from_eulers: camera ") + std::to_string(i) + ": " + err);
    }
    for (int r = 0; r < 3; ++r) {
      j.origin[r] = radius * j.forward[r];
    }
    cov_set_id(j, "cam" + std::to_string(i));
  }
  return 0;
}

// makeNamedArrangement (RigAnalyzer.cpp:240-259) with the tables of :157-238
int derp_rig_arrangement(const char* name, const derp_camera_desc* model, double custom, derp_camera_desc* out, int* n) {
  if (!name || !model || !out || !n) {
    return create_fail("derp_rig_arrangement: bad arguments");
  }
  for (const CovArrangement& a : kCovArrangements) {
    if (strcmp(a.name, name) != 0) {
      continue;
    }
    double e[24][3];
    memcpy(e, a.e, sizeof e);
    const double def = std::isnan(a.defaultAngle) ? std::acos(-1 / 3.0) * 180 / M_PI : a.defaultAngle;
    for (int i = 0; i < a.custom; ++i) {
      e[i][0] = custom == -1 ? def : custom;
    }
    *n = a.n;
    return derp_rig_from_eulers(model, &e[0][0], a.n, a.xyz, out);
  }
  return create_fail(std::string("unknown arrangement ") + name +
                     " (ballcam24, tetra, tetratilted, ring4, cube, carbon0, carbon1, diamond)");
}

// revolveRig (RigAnalyzer.cpp:133-155): out[frame * n + i]; eulers in radians, as the reference reads them
int derp_rig_revolve(const derp_camera_desc* cams, int n, const double* eulers, int m, derp_camera_desc* out) {
  if (!cams || !eulers || !out || n < 1 || m < 1) {
    return create_fail("derp_rig_revolve: bad arguments");
  }
  for (int frame = 0; frame < m; ++frame) {
    double x[9];
    cov_euler_matrix(eulers + 3 * frame, true, x);
    derp_camera_desc* o = out + (size_t)frame * n;
    TRY(cov_load("derp_rig_revolve", cams, n, o));
    for (int i = 0; i < n; ++i) {
      if (const char* err = cov_transform(o[i], x)) {
        return create_fail(std::string("derp_rig_revolve: camera ") + cams[i].id + ": " + err);
      }
      if (m > 1) {
        cov_set_id(o[i], std::string(cams[i].id, strnlen(cams[i].id, sizeof cams[i].id)) + '_' + std::to_string(frame));
      }
    }
  }
  return 0;
}

// the rig turned by the row-major matrix m9 (RigAnalyzer.cpp:511-516, :532-535)
int derp_rig_rotate(const derp_camera_desc* cams, int n, const double* m9, derp_camera_desc* out) {
  if (!cams || !m9 || !out || n < 1) {
    return create_fail("derp_rig_rotate: bad arguments");
  }
  TRY(cov_load("derp_rig_rotate", cams, n, out));
  for (int i = 0; i < n; ++i) {
    if (const char* err = cov_transform(out[i], m9)) {
      return create_fail(std::string("derp_rig_rotate: camera ") + cams[i].id + ": " + err);
    }
  }
  return 0;
}

// std::srand(seed) + Camera::perturbCameras (Camera.cpp:260-280, Camera.h:223-232), in place. Draws, in the reference's
// order: position x y z, rotation x y z (both skipped for camera 0), principal x y, the focal when focal != 0.
int derp_rig_perturb(derp_camera_desc* cams, int n, int seed, double pos, double rot, double principal, double focal) {
  if (!cams || n < 1) {
    return create_fail("derp_rig_perturb: bad arguments");
  }
  std::vector<derp_camera_desc> work(n);
  TRY(cov_load("derp_rig_perturb", cams, n, work.data()));
  for (int i = 0; i < n; ++i) {
    if (focal != 0 && work[i].focal[0] != -work[i].focal[1]) {
      return create_fail(std::string("derp_rig_perturb: camera ") + cams[i].id + ": pixels are not square");
    }
  }
  std::srand((unsigned)seed);
  const auto perturb = [](double& r, double amount) { r += amount * 2 * (std::rand() / double(RAND_MAX) - 0.5); };
  for (int i = 0; i < n; ++i) {
    derp_camera_desc& j = work[i];
    if (i != 0) {
      for (double& v : j.origin) {
        perturb(v, pos);
      }
      // getRotation (Camera.cpp:103-112): the rotation matrix as angle * axis
      const double R[9] = {j.right[0], j.right[1], j.right[2], j.up[0], j.up[1], j.up[2], -j.forward[0], -j.forward[1], -j.forward[2]};
      double angle, axis[3];
      cov_matrix_aa(R, &angle, axis);
      if (angle > M_PI) {
        angle = 2 * M_PI - angle;
        for (double& v : axis) {
          v = -v;
        }
      }
      double v[3] = {angle * axis[0], angle * axis[1], angle * axis[2]};
      for (double& k : v) {
        perturb(k, rot);
      }
      // setRotation(angleAxis) (Camera.cpp:93-101)
      const double a = cov_norm(v);
      double ax[3] = {v[0] / a, v[1] / a, v[2] / a};
      if (a == 0) {
        ax[0] = 1;
        ax[1] = 0;
        ax[2] = 0;
      }
      double N[9];
      cov_aa_matrix(a, ax, N);
      for (int k = 0; k < 3; ++k) {
        j.right[k] = N[k];
        j.up[k] = N[3 + k];
        j.forward[k] = -N[6 + k];
      }
    }
    if (!j.has_principal) {
      j.principal[0] = j.resolution[0] / 2;
      j.principal[1] = j.resolution[1] / 2;
      j.has_principal = 1;
    }
    perturb(j.principal[0], principal);
    perturb(j.principal[1], principal);
    if (focal != 0) {
      double s = j.focal[0];
      perturb(s, focal);
      j.focal[0] = s;
      j.focal[1] = -s;
    }
  }
  std::copy(work.begin(), work.end(), cams);
  return 0;
}

// --scale_rig, --radius and --scale_resolution (RigAnalyzer.cpp:538-555, Camera::rescale, Camera.cpp:217-223), in
// place and in that order; 1, 0 and 1 leave the rig alone
int derp_rig_scale(derp_camera_desc* cams, int n, double scale_rig, double radius, double scale_resolution) {
  if (!cams || n < 1) {
    return create_fail("derp_rig_scale: bad arguments");
  }
  for (int i = 0; i < n; ++i) {
    derp_camera_desc& j = cams[i];
    if (scale_rig != 1) {
      for (double& v : j.origin) {
        v *= scale_rig;
      }
    }
    if (radius > 0) {
      const double sq = sum3(j.origin[0] * j.origin[0], j.origin[1] * j.origin[1], j.origin[2] * j.origin[2]);
      const double len = std::sqrt(sq);
      for (double& v : j.origin) {  // radius * position.normalized(); a zero vector stays
        v = radius * (sq > 0 ? v / len : v);
      }
    }
    if (scale_resolution != 1) {
      for (int k = 0; k < 2; ++k) {
        const double res = scale_resolution * j.resolution[k];
        const double q = res / j.resolution[k];
        const double pr = (j.has_principal ? j.principal[k] : j.resolution[k] / 2) * q;
        j.principal[k] = pr;
        j.focal[k] *= q;
        j.resolution[k] = res;
      }
      // (the file's principal is optional: it is written when it is not the centre, Camera.cpp:163)
      j.has_principal = j.has_principal || j.principal[0] != j.resolution[0] / 2 || j.principal[1] != j.resolution[1] / 2;
    }
  }
  return 0;
}

// ---- device ----
int derp_coverage_directions(derp_ctx* c, const double* units_xyz, int n, const double* distances, int nd, int32_t* hist,
                             uint8_t* counts) {
  CoverageState* S;
  TRY(coverage_begin(c, "derp_coverage_directions", &S));
  if (n < 1 || nd < 1) {
    return fail(c, "derp_coverage_directions: zero points (%d directions, %d distances)", n, nd);
  }
  if (!units_xyz || !distances || !hist || nd > 65535) {
    return fail(c, "derp_coverage_directions: bad arguments (null pointer, or more than 65535 distances)");
  }
  const size_t bins = (size_t)nd * (c->D + 1), total = (size_t)nd * n;
  TRY(upload_sync(c, S->units, units_xyz, (size_t)n * 3 * sizeof(double)));
  TRY(upload_sync(c, S->distances, distances, (size_t)nd * sizeof(double)));
  ALLOC(c, S->hist, bins * sizeof(int32_t));
  HIPCHK(c, hipMemsetAsync(S->hist.p, 0, bins * sizeof(int32_t), c->stream));
  if (counts) {
    ALLOC(c, S->counts, total);
  }
  CovPoints P = {};
  P.units = S->units.as<double>();
  P.distances = S->distances.as<double>();
  {
    Span sp(c, ST_COVERAGE, 0);
    hipLaunchKernelGGL((k_coverage<kCovDirections, false>), dim3(blocks_of((size_t)n, kCovBlock), nd), dim3(kCovBlock), 0,
                       c->stream, c->camsDst.as<Cam>(), S->scams.as<ScaledCam>(), c->D, P, (size_t)n,
                       counts ? S->counts.as<uint8_t>() : (uint8_t*)nullptr, S->hist.as<int>(), (float*)nullptr);
    KCHECK(c);
  }
  TRY(download_sync(c, hist, S->hist.p, bins * sizeof(int32_t)));
  if (counts) {
    TRY(download_sync(c, counts, S->counts.p, total));
  }
  return 0;
}

int derp_coverage_equirect(derp_ctx* c, int pixels_per_degree, double distance, uint8_t* counts, float* min_timing,
                           double* stats) {
  CoverageState* S;
  TRY(coverage_begin(c, "derp_coverage_equirect", &S));
  if (pixels_per_degree < 1) {
    return fail(c, "derp_coverage_equirect: pixels_per_degree must be >= 1 (%d)", pixels_per_degree);
  }
  if (!counts || pixels_per_degree > 64) {
    return fail(c, "derp_coverage_equirect: bad arguments (null counts, or more than 64 pixels per degree)");
  }
  const int W = 360 * pixels_per_degree, H = 180 * pixels_per_degree;
  const size_t pixels = (size_t)W * H;
  // lat, lon and their sines and cosines from the host's libm (RigAnalyzer.cpp:393-397): [cos lon | sin lon] of W, then
  // [cos lat | sin lat] of H
  std::vector<double> t((size_t)2 * W + 2 * H);
  for (int x = 0; x < W; ++x) {
    const double lon = -M_PI + (x + 0.5) / W * 2 * M_PI;
    t[x] = std::cos(lon);
    t[W + x] = std::sin(lon);
  }
  for (int y = 0; y < H; ++y) {
    const double lat = M_PI / 2 - (y + 0.5) / H * M_PI;
    t[2 * W + y] = std::cos(lat);
    t[2 * W + H + y] = std::sin(lat);
  }
  TRY(upload_sync(c, S->tables, t.data(), t.size() * sizeof(double)));
  const double* p = S->tables.as<double>();
  CovPoints P = {};
  P.cosLon = p;
  P.sinLon = p + W;
  P.cosLat = p + 2 * W;
  P.sinLat = p + 2 * W + H;
  P.distance = distance;
  P.w = W;
  if (!min_timing && !stats) {
    return coverage_image<kCovEquirect>(c, *S, P, pixels, counts);
  }
  ALLOC(c, S->counts, pixels);
  ALLOC(c, S->timing, pixels * sizeof(float));
  {
    Span sp(c, ST_COVERAGE, 0);
    hipLaunchKernelGGL((k_coverage<kCovEquirect, true>), dim3(blocks_of(pixels, kCovTimingBlock)), dim3(kCovTimingBlock),
                       (size_t)c->D * kCovTimingBlock * sizeof(float), c->stream, c->camsDst.as<Cam>(), S->scams.as<ScaledCam>(),
                       c->D, P, pixels, S->counts.as<uint8_t>(), (int*)nullptr, S->timing.as<float>());
    KCHECK(c);
  }
  TRY(download_sync(c, counts, S->counts.p, pixels));
  std::vector<float> own;
  if (!min_timing) {
    own.resize(pixels);
    min_timing = own.data();
  }
  TRY(download_sync(c, min_timing, S->timing.p, pixels * sizeof(float)));
  if (stats) {
    // holes, maxMin and aveMin (RigAnalyzer.cpp:388-390, :420-421, :429) in row-major order and in double, so that aveMin
    // is the reference's sum: no floating-point reduction runs on the device
    double holes = 0, maxMin = 0, aveMin = 0;
    for (size_t i = 0; i < pixels; ++i) {
      const double m = min_timing[i];
      maxMin = std::max(maxMin, m);
      aveMin += m;
      holes += (0 == counts[i]) ? 1 : 0;
    }
    stats[0] = holes;
    stats[1] = maxMin;
    stats[2] = aveMin;
  }
  return 0;
}

int derp_coverage_camera(derp_ctx* c, int cam, double distance, uint8_t* counts) {
  CoverageState* S;
  TRY(coverage_begin(c, "derp_coverage_camera", &S));
  if (cam < 0 || cam >= c->D) {
    return fail(c, "derp_coverage_camera: camera index %d out of range (the context has %d)", cam, c->D);
  }
  const derp_camera_desc& j = c->descDstH[cam];
  if (!(j.resolution[0] >= 1) || !(j.resolution[1] >= 1) || !(j.resolution[0] * j.resolution[1] < (double)kMaxPixels)) {
    return fail(c, "derp_coverage_camera: zero points (camera %d is %g x %g)", cam, j.resolution[0], j.resolution[1]);
  }
  if (!counts) {
    return fail(c, "derp_coverage_camera: bad arguments (null counts)");
  }
  const int w = (int)j.resolution[0], h = (int)j.resolution[1];  // const int kDimX = cam.resolution.x() (:351-352)
  CovPoints P = {};
  P.distance = distance;
  P.w = w;
  P.cam = cam;
  return coverage_image<kCovCamera>(c, *S, P, (size_t)w * h, counts);
}

int derp_coverage_cross_section(derp_ctx* c, int dim, uint8_t* counts) {
  CoverageState* S;
  TRY(coverage_begin(c, "derp_coverage_cross_section", &S));
  if (dim < 1) {
    return fail(c, "derp_coverage_cross_section: dim must be >= 1 (%d)", dim);
  }
  if (!counts || dim > 32768) {
    return fail(c, "derp_coverage_cross_section: bad arguments (null counts, or dim beyond 32768)");
  }
  CovPoints P = {};
  P.w = dim;
  return coverage_image<kCovPlane>(c, *S, P, (size_t)dim * dim, counts);
}
