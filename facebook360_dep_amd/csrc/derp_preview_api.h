// The tuning previews, host side: ViewColorVarianceThresholds' threshold arithmetic and marked images,
// ViewForegroundMaskThresholds' overlays, GenerateKeypointProjections' depth sampler, rectangle list and blend. Every setting of a call is rendered from one upload: the variance once per
// call, the blurred pair once per blur radius, the thresholded mask once per (blur, threshold), the closing once per
// triple. Kernels: derp_preview.h and the level loop's own (derp_kernels.h). Included by derp_capi.hip.
#pragma once

namespace {

// What one call may hold on the device at once, inputs, work planes and outputs together: 4 GiB, a fixed bound that does
// not depend on what else the device holds (DERP_PREVIEW_BUDGET_MB overrides it, for tests and for larger sweeps)
constexpr size_t kPreviewBudgetBytes = (size_t)4 << 30;
int preview_budget(derp_ctx* c, size_t bytes, const char* what) {
  size_t budget = kPreviewBudgetBytes;
  if (const char* e = getenv("DERP_PREVIEW_BUDGET_MB")) {
    char* end = nullptr;
    const double mb = strtod(e, &end);
    if (end == e || *end || !(mb > 0) || !(mb < 1e9)) {
      return fail(c, "%s: DERP_PREVIEW_BUDGET_MB='%s' is not a positive finite number of MiB", what, e);
    }
    budget = (size_t)(mb * (double)(1 << 20));
  }
  if (bytes > budget) {
    return fail(c, "%s: the device buffers of this call (%zu bytes) exceed the preview budget (%zu bytes): render fewer "
                "settings per call", what, bytes, budget);
  }
  return 0;
}

// ---- GenerateKeypointProjections: the calibration library's depth sampler (FeatureMatcher.cpp:116-133, 186-207) ----
// params: {length_stride, height_stride, depth_min, depth_max, depth_samples, search_overlap, search_radius}
struct KpParams {
  double lengthStride, heightStride, depthMin, depthMax, depthSamples, searchOverlap;
  int searchRadius;
};

const char* kp_params(const double* p, KpParams* out) {
  if (!p) {
    return "null parameters";
  }
  *out = {p[0], p[1], p[2], p[3], p[4], p[5], p[6] >= 0 && p[6] <= (1 << 20) ? (int)p[6] : -1};
  if (!(p[0] > 0) || !(p[1] > 0) || !std::isfinite(p[0]) || !std::isfinite(p[1])) {
    return "the grid strides must be positive finite numbers (the reference's loops never end otherwise)";
  }
  if (!(p[6] >= 0) || p[6] > 1 << 20 || p[6] != (double)(int)p[6]) {
    return "search_radius must be a whole number >= 0";
  }
  if (!(p[4] >= 2) || !std::isfinite(p[4])) {
    return "depth_samples must be >= 2";
  }
  if (!(p[2] > 0) || !(p[3] >= p[2]) || !std::isfinite(p[3])) {
    return "0 < depth_min <= depth_max is required";
  }
  if (!(p[5] >= 0) || !std::isfinite(p[5])) {
    return "search_overlap must be >= 0";
  }
  return nullptr;
}

// Camera::rig(pixel, depth) (Camera.h:131-142): origin + direction * depth
D3 kp_rig(const Cam& cam, const ScaledCam& sc, double px, double py, double depth) {
  const D3 d = rig_direction(cam, px, py, sc.prx, sc.pry, sc.fx, sc.fy);
  return {cam.pos[0] + d.x * depth, cam.pos[1] + d.y * depth, cam.pos[2] + d.z * depth};
}

// Camera::pixel(rig) (Camera.h:121-128): `sees` without its tests
D2 kp_pixel(const Cam& cam, const ScaledCam& sc, const D3& rig) {
  const D3 v = {rig.x - cam.pos[0], rig.y - cam.pos[1], rig.z - cam.pos[2]};
  const D3 k = {sum3(cam.R[0] * v.x, cam.R[1] * v.y, cam.R[2] * v.z), sum3(cam.R[3] * v.x, cam.R[4] * v.y, cam.R[5] * v.z),
                sum3(cam.R[6] * v.x, cam.R[7] * v.y, cam.R[8] * v.z)};
  const D2 s = camera_to_sensor<0>(cam, k);
  return {sc.fx * s.x + sc.prx, sc.fy * s.y + sc.pry};
}

struct KpBox {  // cv::Rect2f
  float x, y, w, h;
};

// (box & lastBox).area() > search_overlap * box.area() (tooMuchOverlap, :131-133; cv::Rect_<float>::operator&=)
bool kp_too_much_overlap(const KpBox& a, const KpBox& b, double searchOverlap) {
  const float x1 = std::max(a.x, b.x), y1 = std::max(a.y, b.y);
  float w = std::min(a.x + a.w, b.x + b.w) - x1, h = std::min(a.y + a.h, b.y + b.h) - y1;
  if (w <= 0 || h <= 0) {
    w = h = 0;
  }
  return (double)(w * h) > searchOverlap * (double)(a.w * a.h);
}

// getNextDepthSample (:186-207): camPoint holds the point, the boxes lie in camInto. false: no further sample
bool kp_next_sample(const KpParams& P, const Cam& camPoint, const ScaledCam& scPoint, const Cam& camInto, const ScaledCam& scInto,
                    double px, double py, int* sample, double* disparity, KpBox* box) {
  for (int next = *sample + 1; next < P.depthSamples; ++next) {
    const double alpha = next / (P.depthSamples - 1.0);
    const double disp = (1 / P.depthMax) * (1.0 - alpha) + (1 / P.depthMin) * alpha;  // math_util::lerp
    const D2 p1 = kp_pixel(camInto, scInto, kp_rig(camPoint, scPoint, px, py, 1 / disp));
    const KpBox nb = {(float)(p1.x - P.searchRadius), (float)(p1.y - P.searchRadius), (float)(2 * P.searchRadius),
                      (float)(2 * P.searchRadius)};
    if (!kp_too_much_overlap(nb, *box, P.searchOverlap)) {
      *sample = next;
      *disparity = disp;
      *box = nb;
      return true;
    }
  }
  return false;
}

// saturate_cast<int>(double): cvRound, half to even, of a cv::Point2d turned into a cv::Point
int kp_round(double v) {
  const double r = std::nearbyint(v);
  return r >= 2147483647.0 ? 2147483647 : r <= -2147483648.0 ? (-2147483647 - 1) : (int)r;
}

// cv::rectangle(Point2d(p - 0.5 - radius), Point2d(p - 0.5 + radius), colour, filled) (GenerateKeypointProjections.cpp:84-93):
// the corners rounded to cv::Point, both inclusive, clipped to the image -> {x0, y0, x1, y1}; x1 < x0 or y1 < y0: empty
void kp_rect(double px, double py, int radius, int w, int h, int* q) {
  q[0] = std::max(kp_round(px - 0.5 - radius), 0);
  q[1] = std::max(kp_round(py - 0.5 - radius), 0);
  q[2] = std::min(kp_round(px - 0.5 + radius), w - 1);
  q[3] = std::min(kp_round(py - 0.5 + radius), h - 1);
}

// What one pair may ask of the host walk and of the rectangle list: grid points and rectangles drawn
constexpr double kKpMaxGridPoints = 1 << 20;
constexpr size_t kKpMaxRects = (size_t)1 << 20;  // (the reference's defaults draw at most 81 000)

// an upper bound of the values for (f = 0; f <= 1; f += stride) visits, without walking them
double kp_stride_count(double stride) {
  return std::floor(1 / stride) + 2;
}

// the rectangles of the pair (c0, c1) in drawing order (GenerateKeypointProjections.cpp:63-97): the grid lives in cam1,
// the rectangles land in cam0's image of w x h; false: more than kKpMaxRects rectangles
bool kp_rects(const KpParams& P, const Cam& cam0, const ScaledCam& sc0, const Cam& cam1, const ScaledCam& sc1, double width,
              double height, int w, int h, std::vector<PreviewRect>* rects) {
  for (double width_frac = 0; width_frac <= 1; width_frac += P.lengthStride) {
    for (double height_frac = 0; height_frac <= 1; height_frac += P.heightStride) {
      const double px = width * width_frac, py = height * height_frac;
      if (outside_image_circle(cam1, px + 0.5, py + 0.5, sc1.prx, sc1.pry, sc1.fx, sc1.fy)) {
        continue;
      }
      int sample = -1;
      double disparity = 0;
      KpBox box = {0, 0, 0, 0};
      const float4 color = make_float4((float)height_frac, (float)width_frac, (float)(1 - height_frac), 1.0f);
      while (kp_next_sample(P, cam1, sc1, cam0, sc0, px, py, &sample, &disparity, &box)) {
        const D3 world = kp_rig(cam1, sc1, px, py, 1 / disparity);
        D2 p;
        if (sees<0>(cam0, world, sc0.prx, sc0.pry, sc0.fx, sc0.fy, sc0.resx, sc0.resy, p)) {
          int q[4];
          kp_rect(p.x, p.y, P.searchRadius, w, h, q);
          if (rects->size() >= kKpMaxRects) {
            return false;
          }
          rects->push_back({q[0], q[1], q[2], q[3], color});
        }
      }
    }
  }
  return true;
}

}  // namespace

// ---- host only: no context and no device ----
// TrackVar::update and the constructor's scaleVar (ViewColorVarianceThresholds.cpp:69-73, :92-97), in the reference's
// types: the maxima are floats, the sliders ints, scale a double whose square is narrowed to float
int derp_preview_variance_levels(float var_low_max, float var_high_max, int low_slider, int high_slider, double scale,
                                 float* levels4) {
  if (!levels4 || !(var_low_max > 0) || !(var_high_max > 0) || low_slider < 0 || low_slider > 100 || high_slider < 0 ||
      high_slider > 100 || !(scale > 0) || !std::isfinite(scale)) {
    return create_fail("derp_preview_variance_levels: maxima > 0, sliders in 0..100 and a scale > 0 are required");
  }
  const int sliderMaxCount = 100;
  const float scaleVar = (float)(scale * scale);
  const float varNoiseFloor = var_low_max * low_slider / sliderMaxCount;
  const float varHighThresh = var_high_max * high_slider / sliderMaxCount;
  const float varLowShow = std::max(varNoiseFloor * scaleVar, kMinVar);
  const float varHighShow = std::max(varHighThresh, varLowShow);
  levels4[0] = varNoiseFloor;
  levels4[1] = varHighThresh;
  levels4[2] = varLowShow;
  levels4[3] = varHighShow;
  return 0;
}

// ---- device ----
int derp_preview_variance(derp_ctx* c, const uint16_t* bgr16, int w, int h, const float* low_show, const float* high_show,
                          int n, uint16_t* out_bgr16, uint32_t* counts, float* out_variance) {
  if (!c || !bgr16 || !low_show || !high_show || !out_bgr16 || !counts) {
    return fail(c, "derp_preview_variance: bad arguments (null pointer)");
  }
  if (w < 1 || h < 1 || (size_t)w * h >= kMaxPixels) {
    return fail(c, "derp_preview_variance: bad image size %d x %d", w, h);
  }
  if (n < 1 || n > kPreviewMaxImages) {
    return fail(c, "derp_preview_variance: %d settings, 1 .. %d are rendered by one call", n, kPreviewMaxImages);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t px = (size_t)w * h;
  // raw 6 + BGRX 8 + variance 4 + the variance kernel's colour bias 8 (written and not used) per pixel, 6 per output pixel
  TRY(preview_budget(c, px * 26 + (size_t)n * px * 6, "derp_preview_variance"));
  DevBuf raw, img, var, bias, lo, hi, out, cnt;
  ALLOC(c, img, px * 8);
  ALLOC(c, var, px * 4);
  ALLOC(c, bias, px * 8);
  ALLOC(c, out, (size_t)n * px * 6);
  ALLOC(c, cnt, (size_t)2 * n * sizeof(unsigned));
  TRY(upload_sync(c, raw, bgr16, px * 6));
  TRY(upload_sync(c, lo, low_show, (size_t)n * sizeof(float)));
  TRY(upload_sync(c, hi, high_show, (size_t)n * sizeof(float)));
  HIPCHK(c, hipMemsetAsync(cnt.p, 0, (size_t)2 * n * sizeof(unsigned), c->stream));
  hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(px)), dim3(256), 0, c->stream, raw.as<uint16_t>(), img.as<ushort4>(), px);
  // computeImageVariance (DerpUtil.cpp:214-237): the level loop's kernel, one plane; its colour bias is not used here
  hipLaunchKernelGGL(k_variance_bias, blur_grid(w, h, 1), kBlurBlk, 0, c->stream, img.as<ushort4>(), w, h, var.as<float>(),
                     bias.as<ushort4>());
  KCHECK(c);
  hipLaunchKernelGGL(k_preview_marks, dim3(blocks_of(px, kPreviewBlock), n), dim3(kPreviewBlock), 0, c->stream,
                     img.as<ushort4>(), var.as<float>(), px, lo.as<float>(), hi.as<float>(), out.as<uint16_t>(),
                     cnt.as<unsigned>());
  KCHECK(c);
  TRY(download_sync(c, out_bgr16, out.p, (size_t)n * px * 6));
  HIPCHK(c, hipMemcpy(counts, cnt.p, (size_t)2 * n * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (out_variance) {
    HIPCHK(c, hipMemcpy(out_variance, var.p, px * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}

int derp_preview_foreground(derp_ctx* c, const uint16_t* template_bgr16, const uint16_t* frame_bgr16, int w, int h,
                            const int* blur, int nb, const float* threshold, int nt, const int* closing, int nc,
                            uint16_t* out_bgr16, uint8_t* out_mask, uint32_t* counts) {
  if (!c || !template_bgr16 || !frame_bgr16 || !blur || !threshold || !closing || !out_bgr16 || !counts) {
    return fail(c, "derp_preview_foreground: bad arguments (null pointer)");
  }
  if (nb < 1 || nt < 1 || nc < 1 || (long long)nb * nt * nc > kPreviewMaxImages) {
    return fail(c, "derp_preview_foreground: %d x %d x %d settings, 1 .. %d triples are rendered by one call", nb, nt, nc,
                kPreviewMaxImages);
  }
  // derp_generate_foreground_mask's limits, with its message
  bool bad = w <= 0 || h <= 0;
  for (int i = 0; i < nb; ++i) {
    bad = bad || blur[i] < 0 || blur[i] > 3;
  }
  for (int i = 0; i < nt; ++i) {
    bad = bad || !(threshold[i] >= 0);
  }
  for (int i = 0; i < nc; ++i) {
    bad = bad || closing[i] < 0;
  }
  if (bad) {
    return fail(c, "bad arguments (blur_radius must be 0..3)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t px = (size_t)w * h, triples = (size_t)nb * nt * nc;
  // raw 6 + four BGRX planes 32 + two work masks 2 per pixel; overlay 6 + mask 1 per output pixel
  TRY(preview_budget(c, px * 40 + triples * px * 7, "derp_preview_foreground"));
  DevBuf raw, t4, f4, tb, fb, m0, m1, masks, out, cnt;
  ALLOC(c, t4, px * 8);
  ALLOC(c, f4, px * 8);
  ALLOC(c, tb, px * 8);
  ALLOC(c, fb, px * 8);
  ALLOC(c, m0, px);
  ALLOC(c, m1, px);
  ALLOC(c, masks, triples * px);
  ALLOC(c, out, triples * px * 6);
  ALLOC(c, cnt, triples * sizeof(unsigned));
  HIPCHK(c, hipMemsetAsync(cnt.p, 0, triples * sizeof(unsigned), c->stream));
  TRY(upload_sync(c, raw, template_bgr16, px * 6));
  hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(px)), dim3(256), 0, c->stream, raw.as<uint16_t>(), t4.as<ushort4>(), px);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // `raw` is overwritten by the frame
  TRY(upload_sync(c, raw, frame_bgr16, px * 6));
  hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(px)), dim3(256), 0, c->stream, raw.as<uint16_t>(), f4.as<ushort4>(), px);
  KCHECK(c);
  const dim3 g2 = grid2d(w, h, 1, kBlk2d);
  size_t t = 0;
  for (int ib = 0; ib < nb; ++ib) {
    const ushort4 *tp = t4.as<ushort4>(), *fp = f4.as<ushort4>();
    if (blur[ib] > 0) {
      hipLaunchKernelGGL(k_gauss_u16, g2, kBlk2d, 0, c->stream, t4.as<ushort4>(), tb.as<ushort4>(), w, h, blur[ib]);
      hipLaunchKernelGGL(k_gauss_u16, g2, kBlk2d, 0, c->stream, f4.as<ushort4>(), fb.as<ushort4>(), w, h, blur[ib]);
      KCHECK(c);
      tp = tb.as<ushort4>();
      fp = fb.as<ushort4>();
    }
    for (int it = 0; it < nt; ++it) {
      hipLaunchKernelGGL(k_fg_threshold, dim3(flat_grid(px)), dim3(256), 0, c->stream, tp, fp, px, threshold[it], m0.as<uint8_t>());
      KCHECK(c);
      for (int ic = 0; ic < nc; ++ic, ++t) {
        uint8_t* m = masks.as<uint8_t>() + t * px;
        if (closing[ic] > 0) {
          hipLaunchKernelGGL(k_morph_rect, g2, kBlk2d, 0, c->stream, m0.as<uint8_t>(), m1.as<uint8_t>(), w, h, closing[ic], 1);
          hipLaunchKernelGGL(k_morph_rect, g2, kBlk2d, 0, c->stream, m1.as<uint8_t>(), m, w, h, closing[ic], 0);
        } else {
          HIPCHK(c, hipMemcpyAsync(m, m0.p, px, hipMemcpyDeviceToDevice, c->stream));
        }
        // the overlay is laid over the frame as it was loaded, not over its blur (imageFg, :79)
        hipLaunchKernelGGL(k_preview_overlay, dim3(blocks_of(px, kPreviewBlock)), dim3(kPreviewBlock), 0, c->stream,
                           f4.as<ushort4>(), m, px, out.as<uint16_t>() + t * px * 3, cnt.as<unsigned>() + t);
        KCHECK(c);
      }
    }
  }
  TRY(download_sync(c, out_bgr16, out.p, triples * px * 6));
  HIPCHK(c, hipMemcpy(counts, cnt.p, triples * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (out_mask) {
    HIPCHK(c, hipMemcpy(out_mask, masks.p, triples * px, hipMemcpyDeviceToHost));
  }
  return 0;
}

// ---- GenerateKeypointProjections ----
// host only: the accepted depth samples of one point of cam_point, with their boxes in cam_into
int derp_preview_keypoint_samples(const derp_camera_desc* cam_point, const derp_camera_desc* cam_into, double px, double py,
                                  const double* params, int max_out, int* indices, double* disparities, float* boxes4, int* n) {
  KpParams P;
  if (!cam_point || !cam_into || !n || max_out < 0 || (max_out > 0 && (!indices || !disparities || !boxes4))) {
    return create_fail("derp_preview_keypoint_samples: bad arguments (null pointer)");
  }
  if (const char* m = kp_params(params, &P)) {
    return create_fail(std::string("derp_preview_keypoint_samples: ") + m);
  }
  Cam a, b;
  if (const char* m = host_prepare_camera(*cam_point, a)) {
    return create_fail(std::string("derp_preview_keypoint_samples: camera ") + cam_point->id + ": " + m);
  }
  if (const char* m = host_prepare_camera(*cam_into, b)) {
    return create_fail(std::string("derp_preview_keypoint_samples: camera ") + cam_into->id + ": " + m);
  }
  const ScaledCam sa = scaled_cam_res(*cam_point, cam_point->resolution[0], cam_point->resolution[1]);
  const ScaledCam sb = scaled_cam_res(*cam_into, cam_into->resolution[0], cam_into->resolution[1]);
  int sample = -1, count = 0;
  double disparity = 0;
  KpBox box = {0, 0, 0, 0};
  while (kp_next_sample(P, a, sa, b, sb, px, py, &sample, &disparity, &box)) {
    if (count < max_out) {
      indices[count] = sample;
      disparities[count] = disparity;
      boxes4[4 * count] = box.x;
      boxes4[4 * count + 1] = box.y;
      boxes4[4 * count + 2] = box.w;
      boxes4[4 * count + 3] = box.h;
    }
    ++count;
  }
  *n = count;
  return 0;
}

// host only: the rectangle drawn for a projected point (px, py), clipped to a w x h image
int derp_preview_keypoint_rect(double px, double py, int search_radius, int w, int h, int* rect4) {
  if (!rect4 || search_radius < 0 || w < 1 || h < 1 || !std::isfinite(px) || !std::isfinite(py)) {
    return create_fail("derp_preview_keypoint_rect: a finite point, search_radius >= 0 and an image of at least 1 x 1 are required");
  }
  kp_rect(px, py, search_radius, w, h, rect4);
  return 0;
}

int derp_preview_keypoints(derp_ctx* c, int c0, int c1, const double* params, uint8_t* out_bgra8, float* out_float,
                           int* n_rects) {
  KpParams P;
  if (!c || !out_bgra8 || !n_rects) {
    return fail(c, "derp_preview_keypoints: bad arguments (null pointer)");
  }
  if (const char* m = kp_params(params, &P)) {
    return fail(c, "derp_preview_keypoints: %s", m);
  }
  TRY(sweep_need_upload(c));
  TRY(check_camera(c, c0));
  TRY(check_camera(c, c1));
  SweepState& S = *c->sweep;
  const SweepCam& im = S.camsH[c0];
  const double width = c->descDstH[0].resolution[0], height = c->descDstH[0].resolution[1];
  if ((double)im.w != width || (double)im.h != height) {  // the reference's addWeighted throws on sizes that differ
    return fail(c, "derp_preview_keypoints: the image of camera %d is %d x %d, not the first camera's resolution %g x %g", c0,
                im.w, im.h, width, height);
  }
  std::vector<PreviewRect> rects;
  if (kp_stride_count(P.lengthStride) * kp_stride_count(P.heightStride) > kKpMaxGridPoints) {
    return fail(c, "derp_preview_keypoints: strides of %g x %g make more than %.0f grid points", P.lengthStride, P.heightStride,
                kKpMaxGridPoints);
  }
  if (!kp_rects(P, c->camsDstH[c0], S.camsH[c0].sc, c->camsDstH[c1], S.camsH[c1].sc, width, height, im.w, im.h, &rects)) {
    return fail(c, "derp_preview_keypoints: more than %zu rectangles for one pair: use larger strides, fewer depth_samples or a "
                "larger search_radius", kKpMaxRects);
  }
  *n_rects = (int)rects.size();
  HIPCHK(c, hipSetDevice(c->device));
  const size_t px = (size_t)im.w * im.h;
  DevBuf list, plane, u8, f32;
  const PreviewRect none = {0, 0, -1, -1, make_float4(0, 0, 0, 0)};
  TRY(upload_sync(c, list, rects.empty() ? &none : rects.data(), std::max<size_t>(rects.size(), 1) * sizeof(PreviewRect)));
  ALLOC(c, plane, px * 4);
  ALLOC(c, u8, px * 4);
  if (out_float) {
    ALLOC(c, f32, px * 16);
  }
  HIPCHK(c, hipMemsetAsync(plane.p, 0, px * 4, c->stream));
  if (!rects.empty()) {
    hipLaunchKernelGGL(k_preview_splat, dim3((unsigned)std::min<size_t>(rects.size(), 65536)), dim3(kPreviewBlock), 0, c->stream,
                       list.as<PreviewRect>(), (unsigned)rects.size(), im.w, plane.as<unsigned>());
    KCHECK(c);
  }
  hipLaunchKernelGGL(k_preview_keypoint_blend, dim3(blocks_of(px, kPreviewBlock)), dim3(kPreviewBlock), 0, c->stream,
                     S.images.as<float4>() + im.offset, plane.as<unsigned>(), list.as<PreviewRect>(), px, u8.as<uchar4>(),
                     out_float ? f32.as<float4>() : (float4*)nullptr);
  KCHECK(c);
  TRY(download_sync(c, out_bgra8, u8.p, px * 4));
  if (out_float) {
    HIPCHK(c, hipMemcpy(out_float, f32.p, px * 16, hipMemcpyDeviceToHost));
  }
  return 0;
}
