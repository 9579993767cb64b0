// GenerateCameraOverlaps and GenerateEquirect (source/render), host side: the float BGRA images and the cameras rescaled
// to their (fractional) resolutions, the overlaps of one destination over a list of disparities, the equirect over a list
// of depths (whole or cropped to a window), the window's bounds, and the host-only depth lists, crop size and rig
// centring. Kernels: derp_sweep.h. Definitions: DESIGN §8.7. Included by derp_capi.hip after the depth core.
#pragma once

namespace {

struct SweepState {
  std::vector<SweepCam> camsH;  // empty: derp_sweep_upload has not succeeded
  DevBuf scams, images, list, tables, bounds, out;
};

// Camera::rescale(newResolution) (Camera.cpp:217-223) to a resolution that need not be whole: scaled_cam's order
ScaledCam scaled_cam_res(const derp_camera_desc& j, double rx, double ry) {
  const double qx = rx / j.resolution[0], qy = ry / j.resolution[1];
  const double prx = j.has_principal ? j.principal[0] : j.resolution[0] / 2;
  const double pry = j.has_principal ? j.principal[1] : j.resolution[1] / 2;
  return {prx * qx, pry * qy, j.focal[0] * qx, j.focal[1] * qy, rx, ry};
}

int sweep_need_upload(derp_ctx* c) {
  if (!c->sweep || c->sweep->camsH.empty()) {
    return fail(c, "derp_sweep_upload has not been called");
  }
  return 0;
}

// parts of a list of `n` depths for an image of `pixels`: enough blocks to fill the device; -> (parts, depths per part)
void sweep_split(size_t pixels, int n, int* splits, int* per) {
  const size_t blocks = blocks_of(pixels, kSweepBlock);
  int s = (int)std::min<size_t>((1024 + blocks - 1) / blocks, (size_t)kSweepMaxSplit);
  s = std::max(1, std::min(s, n));
  *per = (n + s - 1) / s;
  *splits = (n + *per - 1) / *per;
}

int sweep_check_out(derp_ctx* c, int out_kind, const void* out, int n) {
  if (!out || n < 1 || (out_kind != kSweepFloat && out_kind != kSweepU8)) {
    return fail(c, "bad arguments (null output, an empty list or an unknown output kind)");
  }
  return 0;
}

// the sines and cosines of an equirect call's columns and rows (getEquirectPoint, GenerateEquirect.cpp:102-110; the
// cropped positions of :164-166), from the host's libm: [cos theta | sin theta] of out_w, then [sin phi | cos phi] of out_h
std::vector<double> sweep_tables(int W, int H, const int* window, int out_w, int out_h) {
  std::vector<double> t((size_t)2 * out_w + 2 * out_h);
  for (int xi = 0; xi < out_w; ++xi) {
    const double x = window ? (double)xi * (double)(window[1] - window[0]) / (double)out_w + (double)window[0] : (double)xi;
    const double theta = -1 * ((x + 0.5) / (double)W * 2 * M_PI);
    t[xi] = std::cos(theta);
    t[out_w + xi] = std::sin(theta);
  }
  for (int yi = 0; yi < out_h; ++yi) {
    const double y = window ? (double)yi * (double)(window[3] - window[2]) / (double)out_h + (double)window[2] : (double)yi;
    const double phi = (y + 0.5) / (double)H * M_PI;
    t[2 * out_w + yi] = std::sin(phi);
    t[2 * out_w + out_h + yi] = std::cos(phi);
  }
  return t;
}

int sweep_upload_tables(derp_ctx* c, SweepState& S, int W, int H, const int* window, int out_w, int out_h, SweepEqr* e) {
  const std::vector<double> t = sweep_tables(W, H, window, out_w, out_h);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the call before this one may still read the tables
  TRY(upload_sync(c, S.tables, t.data(), t.size() * sizeof(double)));
  const double* p = S.tables.as<double>();
  *e = {p, p + out_w, p + 2 * out_w, p + 2 * out_w + out_h, out_w, out_h};
  return 0;
}

// ---- centerRig (GenerateEquirect.cpp:177-231) ----
// Camera::setRotation's re-unitarisation (Camera.cpp:77-87, host_prepare_camera): forward, up and right as the camera
// returns them afterwards
const char* sweep_unitarise(derp_camera_desc& j) {
  Cam c;
  const char* err = host_prepare_camera(j, c);
  if (err) {
    return err;
  }
  for (int k = 0; k < 3; ++k) {
    j.right[k] = c.R[k];
    j.up[k] = c.R[3 + k];
    j.forward[k] = -c.R[6 + k];
  }
  return nullptr;
}

// getRotationAngle (:178-183)
double sweep_rotation_angle(const double* a, const double* b, int sign) {
  const double dot = sum3(a[0] * b[0], a[1] * b[1], a[2] * b[2]);
  const double mag = std::sqrt(sum3(a[0] * a[0], a[1] * a[1], a[2] * a[2])) * std::sqrt(sum3(b[0] * b[0], b[1] * b[1], b[2] * b[2]));
  return mag == 0 ? 0 : sign * std::acos(dot / mag);
}

// transformRig (RigTransform.h:73-97) with a rotation about one axis (0 = x, 1 = y, 2 = z), no translation, scale 1:
// AngleAxis z * y * x with two of the three the identity is the one quaternion (cos a/2, sin a/2 on the axis), and its
// matrix is Eigen's toRotationMatrix of it
const char* sweep_rotate_rig(derp_camera_desc* cams, int n, int axis, double angle) {
  const double w = std::cos(angle / 2), s = std::sin(angle / 2);
  const double t = 2 * s, co = 1 - t * s, si = t * w;
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const int a = (axis + 1) % 3, b = (axis + 2) % 3;
  R[a][a] = co;
  R[b][b] = co;
  R[a][b] = -si;
  R[b][a] = si;
  for (int i = 0; i < n; ++i) {
    double* vecs[4] = {cams[i].forward, cams[i].up, cams[i].right, cams[i].origin};
    for (double* v : vecs) {
      const double x = v[0], y = v[1], z = v[2];
      for (int r = 0; r < 3; ++r) {
        v[r] = sum3(R[r][0] * x, R[r][1] * y, R[r][2] * z);
      }
    }
    const char* err = sweep_unitarise(cams[i]);
    if (err) {
      return err;
    }
  }
  return nullptr;
}

}  // namespace

// ---- host only: no context and no device ----
int derp_sweep_overlap_disparities(int num_depths, uint64_t min_depth_m, uint64_t max_depth_m, float* disparities, int* stems) {
  if (num_depths < 1 || min_depth_m == 0 || max_depth_m == 0 || !disparities) {
    return create_fail("derp_sweep_overlap_disparities: num_depths >= 1 and depths > 0 are required");
  }
  // dumpOverlaps is handed 1.0f / min_depth_m as ITS minDisparity and 1.0f / max_depth_m as its maxDisparity
  // (GenerateCameraOverlaps.cpp:148-155), so probe 0 is the farthest depth
  const float a = 1.0f / (float)min_depth_m, b = 1.0f / (float)max_depth_m;
  for (int d = 0; d < num_depths; ++d) {
    // probeDisparity (ImageUtil.cpp:100-107); one depth: the reference's 0 / 0 is not copied, the fraction is 0
    const double fraction = num_depths == 1 ? 0.0 : (double)d / (double)(num_depths - 1);
    disparities[d] = (float)(fraction * (double)a + (1 - fraction) * (double)b);
    if (stems) {
      const float depth = 1.0f / disparities[d];
      const float depthCm = depth * 100;
      stems[d] = (int)depthCm;
    }
  }
  return 0;
}

int derp_sweep_equirect_depths(int num_depths, double depth_min, double depth_max, float* depths, int* stems) {
  if (num_depths < 1 || !(depth_min > 0) || !(depth_max > 0) || !depths) {
    return create_fail("derp_sweep_equirect_depths: num_depths >= 1 and depths > 0 are required");
  }
  const float dispMin = (float)(1.0f / depth_max), dispMax = (float)(1.0f / depth_min);
  for (int i = 0; i < num_depths; ++i) {
    const float fraction = (float)i / (float)(num_depths - 1);
    const float disp = num_depths == 1 ? dispMin : fraction * dispMin + (1 - fraction) * dispMax;
    depths[i] = 1.0f / disp;
    if (stems) {
      stems[i] = (int)((double)depths[i] * 100);
    }
  }
  return 0;
}

int derp_sweep_crop_size(int height, const int* bounds, int* new_width) {
  if (height < 1 || !bounds || !new_width) {
    return create_fail("derp_sweep_crop_size: bad arguments");
  }
  const double minX = bounds[0], maxX = bounds[1], minY = bounds[2], maxY = bounds[3];
  if (!(maxX - minX > 0) || !(maxY - minY > 0)) {
    return create_fail(fmt_string("crop_equirect: no camera sees this depth, or the visible box is empty "
                                  "(columns %d..%d, rows %d..%d)", bounds[0], bounds[1], bounds[2], bounds[3]));
  }
  const double w = (double)height / (maxY - minY) * (maxX - minX);  // :159
  if (!(w >= 1) || w >= 2147483648.0) {
    return create_fail(fmt_string("crop_equirect: cropped width %.0f is out of range", w));
  }
  *new_width = (int)w;
  return 0;
}

int derp_rig_center(const derp_camera_desc* cams, int n, int index, derp_camera_desc* out_cams) {
  if (!cams || !out_cams || n < 1 || index < 0 || index >= n) {
    return create_fail("derp_rig_center: bad arguments");
  }
  for (int i = 0; i < n; ++i) {
    out_cams[i] = cams[i];
    const char* err = sweep_unitarise(out_cams[i]);
    if (err) {
      return create_fail(std::string("derp_rig_center: camera ") + cams[i].id + ": " + err);
    }
  }
  const double centre[3] = {-1, 0, 0}, upwards[3] = {0, 0, 1};
  for (int step = 0; step < 3; ++step) {
    const derp_camera_desc& sel = out_cams[index];
    double angle;
    int axis;
    if (step == 0) {  // yaw
      const double v[3] = {sel.forward[0], sel.forward[1], 0};
      angle = sweep_rotation_angle(centre, v, sel.forward[1] > 0 ? 1 : -1);
      axis = 2;
    } else if (step == 1) {  // pitch
      const double v[3] = {sel.forward[0], 0, sel.forward[2]};
      angle = sweep_rotation_angle(centre, v, sel.forward[2] > 0 ? -1 : 1);
      axis = 1;
    } else {  // roll
      const double v[3] = {0, sel.up[1], sel.up[2]};
      angle = sweep_rotation_angle(upwards, v, sel.up[1] > 0 ? 1 : -1);
      axis = 0;
    }
    const char* err = sweep_rotate_rig(out_cams, n, axis, angle);
    if (err) {
      return create_fail(std::string("derp_rig_center: ") + err);
    }
  }
  return 0;
}

// ---- device ----
int derp_sweep_upload(derp_ctx* c, const float* const* bgra, const int* img_w, const int* img_h, const double* cam_res_xy) {
  if (!c || !bgra || !img_w || !img_h || !cam_res_xy) {
    return fail(c, "bad arguments (null pointer)");
  }
  std::vector<SweepCam> t(c->D);
  size_t texels = 0;
  for (int i = 0; i < c->D; ++i) {
    const double rx = cam_res_xy[2 * i], ry = cam_res_xy[2 * i + 1];
    if (!bgra[i] || img_w[i] < 1 || img_h[i] < 1 || (size_t)img_w[i] * img_h[i] >= kMaxPixels || !(rx > 0) || !(ry > 0) ||
        !std::isfinite(rx) || !std::isfinite(ry)) {
      return fail(c, "camera %d: null image, bad image size %d x %d or bad resolution %g x %g", i, img_w[i], img_h[i], rx, ry);
    }
    t[i] = {scaled_cam_res(c->descDstH[i], rx, ry), (unsigned long long)texels, img_w[i], img_h[i]};
    texels += (size_t)img_w[i] * img_h[i];
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->sweep) {
    c->sweep.reset(new SweepState);
  }
  SweepState& S = *c->sweep;
  S.camsH.clear();
  ALLOC(c, S.images, texels * 16);
  for (int i = 0; i < c->D; ++i) {
    HIPCHK(c, hipMemcpy(S.images.as<float4>() + t[i].offset, bgra[i], (size_t)t[i].w * t[i].h * 16, hipMemcpyHostToDevice));
  }
  TRY(upload_sync(c, S.scams, t.data(), t.size() * sizeof(SweepCam)));
  S.camsH = t;
  return 0;
}

int derp_sweep_overlaps(derp_ctx* c, int dst, const float* disparities, int n, int out_kind, void* out) {
  if (!c || !disparities) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(sweep_check_out(c, out_kind, out, n));
  TRY(sweep_need_upload(c));
  TRY(check_camera(c, dst));
  HIPCHK(c, hipSetDevice(c->device));
  SweepState& S = *c->sweep;
  const size_t pixels = (size_t)S.camsH[dst].w * S.camsH[dst].h;
  const size_t bytes = pixels * n * (out_kind == kSweepU8 ? 4 : 16);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  TRY(upload_sync(c, S.list, disparities, (size_t)n * sizeof(float)));
  ALLOC(c, S.out, bytes);
  int splits, per;
  sweep_split(pixels, n, &splits, &per);
  {
    Span sp(c, ST_SWEEP_OVERLAPS, 0);
    hipLaunchKernelGGL(k_sweep_overlaps, dim3(blocks_of(pixels, kSweepBlock), 1, splits), dim3(kSweepBlock), 0, c->stream,
                       c->camsDst.as<Cam>(), S.scams.as<SweepCam>(), c->D, dst, S.images.as<float4>(), S.list.as<float>(), n,
                       per, out_kind, S.out.p);
    KCHECK(c);
  }
  return download_sync(c, out, S.out.p, bytes);
}

int derp_sweep_equirect_bounds(derp_ctx* c, int W, int H, float depth, int* bounds) {
  if (!c || !bounds || W < 1 || H < 1 || (size_t)W * H >= kMaxPixels) {
    return fail(c, "bad arguments (null pointer or equirect size)");
  }
  TRY(sweep_need_upload(c));
  HIPCHK(c, hipSetDevice(c->device));
  SweepState& S = *c->sweep;
  SweepEqr e;
  TRY(sweep_upload_tables(c, S, W, H, nullptr, W, H, &e));
  const int init[4] = {W, 0, H, 0};  // (:139-142)
  TRY(upload_sync(c, S.bounds, init, sizeof init));
  hipLaunchKernelGGL(k_sweep_equirect_bounds, dim3(blocks_of((size_t)W * H, kSweepBlock)), dim3(kSweepBlock), 0, c->stream,
                     c->camsDst.as<Cam>(), S.scams.as<SweepCam>(), c->D, e, (double)depth, S.bounds.as<int>());
  KCHECK(c);
  return download_sync(c, bounds, S.bounds.p, sizeof init);
}

int derp_sweep_equirect(derp_ctx* c, int W, int H, const int* window, int out_w, int out_h, const float* depths, int n,
                        const float* background_bgra, int out_kind, void* out) {
  if (!c || !depths || !background_bgra || W < 1 || H < 1 || out_w < 1 || out_h < 1 || (size_t)out_w * out_h >= kMaxPixels) {
    return fail(c, "bad arguments (null pointer or equirect size)");
  }
  if (!window && (out_w != W || out_h != H)) {
    return fail(c, "an equirect without a window has the full size %d x %d, not %d x %d", W, H, out_w, out_h);
  }
  if (window && (window[1] <= window[0] || window[3] <= window[2])) {
    return fail(c, "empty window: columns %d..%d, rows %d..%d", window[0], window[1], window[2], window[3]);
  }
  TRY(sweep_check_out(c, out_kind, out, n));
  TRY(sweep_need_upload(c));
  HIPCHK(c, hipSetDevice(c->device));
  SweepState& S = *c->sweep;
  SweepEqr e;
  TRY(sweep_upload_tables(c, S, W, H, window, out_w, out_h, &e));
  const size_t pixels = (size_t)out_w * out_h;
  const size_t bytes = pixels * n * (out_kind == kSweepU8 ? 4 : 16);
  TRY(upload_sync(c, S.list, depths, (size_t)n * sizeof(float)));
  ALLOC(c, S.out, bytes);
  int splits, per;
  sweep_split(pixels, n, &splits, &per);
  const float4 bg = make_float4(background_bgra[0], background_bgra[1], background_bgra[2], background_bgra[3]);
  {
    Span sp(c, ST_SWEEP_EQUIRECT, 0);
    hipLaunchKernelGGL(k_sweep_equirect, dim3(blocks_of(pixels, kSweepBlock), 1, splits), dim3(kSweepBlock), 0, c->stream,
                       c->camsDst.as<Cam>(), S.scams.as<SweepCam>(), c->D, S.images.as<float4>(), e, S.list.as<float>(), n, per,
                       bg, out_kind, S.out.p);
    KCHECK(c);
  }
  return download_sync(c, out, S.out.p, bytes);
}
