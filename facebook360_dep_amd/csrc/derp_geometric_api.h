// GeometricConsistency (source/render/GeometricConsistency.cpp), host side: the int16 images, the slice table, the sweep
// of one destination, the cross-camera cleaning, the whole frame and the stage downloads. Kernels: derp_geometric.h.
// The cameras are the context's destinations as the rig file holds them (un-normalised), Camera::rescale'd to the small
// sizes of derp_gc_upload. Included by derp_capi.hip after the depth core.
#pragma once

namespace {

struct GcState {
  std::vector<GcCam> camsH;  // empty: derp_gc_upload has not succeeded
  size_t pixels = 0;         // of all small images together
  DevBuf gcams, images, full;
  DevBuf clean;  // derp_gc_set_clean's maps
  bool haveClean = false;
  DevBuf slices, bestCost, bestSlice, depth;
  DevBuf stageSample, stageAverage, stageAverageOfSq, stageCost;
  // derp_gc_run's frame: the depths as the next pass reads them, and what the tool dumps
  DevBuf cur, iffy, cleanRun, depthRun;
  int passes = -1;  // of the last derp_gc_run (-1: none)
};

std::string fmt_string(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

GcState* gc_state(derp_ctx* c) {
  if (!c->gc) {
    c->gc.reset(new GcState);
  }
  return c->gc.get();
}

// the table of small images: offsets in pixels, cameras rescaled as the reference's downscale() does (:324-331)
std::vector<GcCam> gc_table(const derp_ctx* c, const int* w, const int* h, size_t* pixels) {
  std::vector<GcCam> t(c->D);
  size_t n = 0;
  for (int i = 0; i < c->D; ++i) {
    t[i] = {scaled_cam(c->descDstH[i], w[i], h[i]), (unsigned long long)n, w[i], h[i]};
    n += (size_t)w[i] * h[i];
  }
  *pixels = n;
  return t;
}

int gc_check_sizes(derp_ctx* c, const int* w, const int* h) {
  for (int i = 0; i < c->D; ++i) {
    if (w[i] < 3 || h[i] < 3 || (size_t)w[i] * h[i] >= kMaxPixels) {
      return fail(c, "bad image size %d x %d for camera %d (3 x 3 at least)", w[i], h[i], i);
    }
  }
  return 0;
}

// computeRigRadius (:97-103): the mean distance of the cameras from the rig's origin
double gc_rig_radius(const derp_camera_desc* cams, int n) {
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double* o = cams[i].origin;
    sum += std::sqrt(sum3(o[0] * o[0], o[1] * o[1], o[2] * o[2]));
  }
  return sum / n;
}

// sliceCount of computeDepth (:186-192) for a destination rescaled to `sc`; the refusal's text, or empty
std::string gc_slice_count(double radius, const ScaledCam& sc, double disparityStep, int* count) {
  if (!(radius < 1.0)) {
    return fmt_string("rig radius %.6g m: the cameras must lie less than 1 m from the rig's origin on average (asin)", radius);
  }
  if (!(disparityStep > 0)) {
    return "disparity_step must be positive";
  }
  const double focal = std::sqrt(sc.fx * sc.fx + sc.fy * sc.fy) * std::sqrt(0.5);
  const double n = std::round(focal * std::asin(radius) / disparityStep);
  if (!(n >= 1)) {
    return fmt_string("sliceCount %.0f < 1: disparity_step %.6g is too coarse for this rig", n, disparityStep);
  }
  if (n > 1e6) {
    return fmt_string("sliceCount %.0f is beyond 10^6: disparity_step %.6g is too fine", n, disparityStep);
  }
  *count = (int)n;
  return "";
}

// sliceCount and sliceDisparity (:126-128, ReprojectionTable.h:161-165: fp32) of the destination `g`
int gc_slices(derp_ctx* c, const GcCam& g, double disparityStep, std::vector<float>& out) {
  int n = 0;
  const std::string refusal = gc_slice_count(gc_rig_radius(c->descDstH.data(), c->D), g.sc, disparityStep, &n);
  if (!refusal.empty()) {
    return fail(c, "%s", refusal.c_str());
  }
  const float minDisp = (float)(1.0 / 1e4), maxDisp = 1.0f;  // 1.0f / Camera::kNearInfinity
  out.resize(n);
  for (int s = 0; s < n; ++s) {
    const float t = (float)((s + 0.5) / n);
    out[s] = (1 - t) * minDisp + t * maxDisp;
  }
  return 0;
}

int gc_need_upload(derp_ctx* c) {
  if (!c->gc || c->gc->camsH.empty()) {
    return fail(c, "derp_gc_upload has not been called");
  }
  return 0;
}

// the slice table of `dst` on the device; -> the number of slices
int gc_upload_slices(derp_ctx* c, GcState& G, int dst, double step, int* count) {
  std::vector<float> slices;
  TRY(gc_slices(c, G.camsH[dst], step, slices));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the sweep before this one may still read the table
  TRY(upload_sync(c, G.slices, slices.data(), slices.size() * sizeof(float)));
  *count = (int)slices.size();
  return 0;
}

// computeDepth (:165-258) of `dst` into `depthOut` (device, [h][w]); clean: the sources' clean depths or null.
// split: parts of the slice range, 0 = as many as fill the device (the result does not depend on it)
int gc_sweep_dev(derp_ctx* c, GcState& G, int dst, double step, const float* clean, double agree, int split,
                 float* depthOut) {
  int count = 0;
  TRY(gc_upload_slices(c, G, dst, step, &count));
  const GcCam& g = G.camsH[dst];
  const int tilesX = (g.w + kGcTile - 1) / kGcTile, tilesY = (g.h + kGcTile - 1) / kGcTile;
  int splits = split > 0 ? split : (1024 + tilesX * tilesY - 1) / (tilesX * tilesY);
  splits = std::max(1, std::min(std::min(splits, count), kGcMaxSplit));
  const int per = (count + splits - 1) / splits;
  splits = (count + per - 1) / per;
  const size_t n = (size_t)g.w * g.h;
  ALLOC(c, G.bestCost, n * splits * sizeof(float));
  ALLOC(c, G.bestSlice, n * splits * sizeof(int));
  {
    Span sp(c, ST_GC_SWEEP, 0);
    hipLaunchKernelGGL(k_gc_sweep<false>, dim3(tilesX, tilesY, splits), dim3(kGcBlock), 0, c->stream, c->camsDst.as<Cam>(),
                       G.gcams.as<GcCam>(), c->D, dst, G.images.as<short4>(), clean, agree, G.slices.as<float>(), count, per,
                       G.bestCost.as<float>(), G.bestSlice.as<int>(), -1, GcStageOut{});
    hipLaunchKernelGGL(k_gc_reduce, grid2d(g.w, g.h, 1, kBlk2d), kBlk2d, 0, c->stream, G.bestCost.as<float>(),
                       G.bestSlice.as<int>(), splits, G.slices.as<float>(), g.w, g.h, depthOut);
    KCHECK(c);
  }
  return 0;
}

// cleanDepth (:293-310) of every camera: depths -> out, both laid out by `gcams`
int gc_clean_dev(derp_ctx* c, const std::vector<GcCam>& camsH, const GcCam* gcams, const float* depths, double agree,
                 float* out) {
  Span sp(c, ST_GC_CLEAN, 0);
  for (int d = 0; d < c->D; ++d) {
    const size_t n = (size_t)camsH[d].w * camsH[d].h;
    hipLaunchKernelGGL(k_gc_clean, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, c->camsDst.as<Cam>(), gcams, c->D, d,
                       depths, agree, out);
  }
  KCHECK(c);
  return 0;
}

int gc_check_fraction(derp_ctx* c, double agree) {
  if (!(agree == agree)) {
    return fail(c, "agree_fraction is NaN");
  }
  return 0;
}

}  // namespace

// host only: no context and no device
int derp_gc_slice_count(const derp_camera_desc* cams, int n_cams, int dst, int small_w, int small_h, double disparity_step,
                        int* count) {
  if (!cams || n_cams < 1 || dst < 0 || dst >= n_cams || small_w < 1 || small_h < 1 || !count) {
    return create_fail("derp_gc_slice_count: bad arguments");
  }
  const std::string refusal =
      gc_slice_count(gc_rig_radius(cams, n_cams), scaled_cam(cams[dst], small_w, small_h), disparity_step, count);
  return refusal.empty() ? 0 : create_fail(refusal);
}

int derp_gc_upload(derp_ctx* c, const uint16_t* const* bgra, const int* full_w, const int* full_h, const int* small_w,
                   const int* small_h) {
  if (!c || !bgra || !full_w || !full_h || !small_w || !small_h) {
    return fail(c, "bad arguments (null pointer)");
  }
  if (c->D < 2) {
    return fail(c, "GeometricConsistency needs at least two cameras");
  }
  TRY(gc_check_sizes(c, small_w, small_h));
  for (int i = 0; i < c->D; ++i) {
    if (!bgra[i] || full_w[i] < small_w[i] || full_h[i] < small_h[i] || (size_t)full_w[i] * full_h[i] >= kMaxPixels) {
      return fail(c, "camera %d: null image, or full size %d x %d below the small size %d x %d", i, full_w[i], full_h[i],
                  small_w[i], small_h[i]);
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  GcState& G = *gc_state(c);
  G.camsH.clear();
  G.haveClean = false;
  G.passes = -1;
  size_t pixels = 0;
  std::vector<GcCam> table = gc_table(c, small_w, small_h, &pixels);
  ALLOC(c, G.images, pixels * sizeof(short4));
  TRY(upload_sync(c, G.gcams, table.data(), table.size() * sizeof(GcCam)));
  {
    Span sp(c, ST_GC_PREPARE, 0);
    for (int i = 0; i < c->D; ++i) {
      const size_t n = (size_t)full_w[i] * full_h[i];
      TRY(upload_sync(c, G.full, bgra[i], n * 4 * sizeof(uint16_t)));
      TRY(resize_area_dev(c, 4, G.full.p, full_w[i], full_h[i], G.images.as<short4>() + table[i].offset, small_w[i],
                          small_h[i], -1));
      HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffer takes the next camera
    }
  }
  G.pixels = pixels;
  G.camsH = table;
  return 0;
}

int derp_gc_download_image(derp_ctx* c, int cam, int16_t* out_bgra) {
  if (!c || !out_bgra) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(gc_need_upload(c));
  TRY(check_camera(c, cam));
  HIPCHK(c, hipSetDevice(c->device));
  const GcCam& g = c->gc->camsH[cam];
  return download_sync(c, out_bgra, c->gc->images.as<short4>() + g.offset, (size_t)g.w * g.h * sizeof(short4));
}

int derp_gc_slices(derp_ctx* c, int dst, double disparity_step, int* count, float* disparities, int cap) {
  if (!c || !count) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(gc_need_upload(c));
  TRY(check_camera(c, dst));
  std::vector<float> slices;
  TRY(gc_slices(c, c->gc->camsH[dst], disparity_step, slices));
  *count = (int)slices.size();
  if (disparities) {
    if (cap < *count) {
      return fail(c, "derp_gc_slices: %d slices do not fit the output's capacity of %d", *count, cap);
    }
    memcpy(disparities, slices.data(), slices.size() * sizeof(float));
  }
  return 0;
}

int derp_gc_set_clean(derp_ctx* c, const float* const* clean) {
  if (!c) {
    return 1;
  }
  TRY(gc_need_upload(c));
  GcState& G = *c->gc;
  G.haveClean = false;
  if (!clean) {
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ALLOC(c, G.clean, G.pixels * sizeof(float));
  for (int i = 0; i < c->D; ++i) {
    if (!clean[i]) {
      return fail(c, "null clean depth for camera %d", i);
    }
    const GcCam& g = G.camsH[i];
    HIPCHK(c, hipMemcpy(G.clean.as<float>() + g.offset, clean[i], (size_t)g.w * g.h * sizeof(float), hipMemcpyHostToDevice));
  }
  G.haveClean = true;
  return 0;
}

int derp_gc_sweep(derp_ctx* c, int dst, double disparity_step, int use_clean, double agree_fraction, int split,
                  float* depth) {
  if (!c || !depth) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(gc_need_upload(c));
  TRY(check_camera(c, dst));
  TRY(gc_check_fraction(c, agree_fraction));
  GcState& G = *c->gc;
  if (use_clean && !G.haveClean) {
    return fail(c, "derp_gc_set_clean has not been called");
  }
  if (split < 0) {
    return fail(c, "split must be 0 (the library's choice) or positive");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)G.camsH[dst].w * G.camsH[dst].h;
  ALLOC(c, G.depth, n * sizeof(float));
  TRY(gc_sweep_dev(c, G, dst, disparity_step, use_clean ? G.clean.as<float>() : nullptr, agree_fraction, split,
                   G.depth.as<float>()));
  return download_sync(c, depth, G.depth.p, n * sizeof(float));
}

int derp_gc_clean(derp_ctx* c, const float* const* depths, const int* w, const int* h, double agree_fraction,
                  float* const* out) {
  if (!c || !depths || !w || !h || !out) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(gc_check_sizes(c, w, h));
  TRY(gc_check_fraction(c, agree_fraction));
  for (int i = 0; i < c->D; ++i) {
    if (!depths[i] || !out[i]) {
      return fail(c, "null depth map for camera %d", i);
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  size_t pixels = 0;
  const std::vector<GcCam> table = gc_table(c, w, h, &pixels);
  DevBuf gcams, in, res;
  TRY(upload_sync(c, gcams, table.data(), table.size() * sizeof(GcCam)));
  ALLOC(c, in, pixels * sizeof(float));
  ALLOC(c, res, pixels * sizeof(float));
  for (int i = 0; i < c->D; ++i) {
    HIPCHK(c, hipMemcpy(in.as<float>() + table[i].offset, depths[i], (size_t)w[i] * h[i] * sizeof(float), hipMemcpyHostToDevice));
  }
  TRY(gc_clean_dev(c, table, gcams.as<GcCam>(), in.as<float>(), agree_fraction, res.as<float>()));
  KCHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < c->D; ++i) {
    HIPCHK(c, hipMemcpy(out[i], res.as<float>() + table[i].offset, (size_t)w[i] * h[i] * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 0;
}

// processFrame (:333-384)
int derp_gc_run(derp_ctx* c, double disparity_step, double agree_fraction, int pass_count, int keep_clean) {
  if (!c) {
    return 1;
  }
  TRY(gc_need_upload(c));
  TRY(gc_check_fraction(c, agree_fraction));
  if (pass_count < 0 || pass_count > 1024) {
    return fail(c, "pass_count %d out of range (0..1024)", pass_count);
  }
  HIPCHK(c, hipSetDevice(c->device));
  GcState& G = *c->gc;
  G.passes = -1;
  const size_t bytes = G.pixels * sizeof(float);
  ALLOC(c, G.cur, bytes);
  ALLOC(c, G.iffy, bytes);
  ALLOC(c, G.cleanRun, bytes * std::max(pass_count, 1));
  ALLOC(c, G.depthRun, bytes * std::max(pass_count, 1));
  for (int d = 0; d < c->D; ++d) {
    TRY(gc_sweep_dev(c, G, d, disparity_step, nullptr, agree_fraction, 0, G.iffy.as<float>() + G.camsH[d].offset));
  }
  HIPCHK(c, hipMemcpyAsync(G.cur.p, G.iffy.p, bytes, hipMemcpyDeviceToDevice, c->stream));
  for (int pass = 0; pass < pass_count; ++pass) {
    float* cleanDepths = G.cleanRun.as<float>() + (size_t)pass * G.pixels;
    float* depths = G.depthRun.as<float>() + (size_t)pass * G.pixels;
    TRY(gc_clean_dev(c, G.camsH, G.gcams.as<GcCam>(), G.cur.as<float>(), agree_fraction, cleanDepths));
    for (int d = 0; d < c->D; ++d) {
      TRY(gc_sweep_dev(c, G, d, disparity_step, cleanDepths, agree_fraction, 0, depths + G.camsH[d].offset));
    }
    HIPCHK(c, hipMemcpyAsync(G.cur.p, depths, bytes, hipMemcpyDeviceToDevice, c->stream));
    if (keep_clean) {
      hipLaunchKernelGGL(k_gc_restore, dim3(flat_grid(G.pixels)), dim3(256), 0, c->stream, cleanDepths, G.cur.as<float>(),
                         G.pixels);
      KCHECK(c);
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  G.passes = pass_count;
  return 0;
}

int derp_gc_result(derp_ctx* c, int kind, int pass, int cam, float* out) {
  if (!c || !out) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(gc_need_upload(c));
  TRY(check_camera(c, cam));
  GcState& G = *c->gc;
  if (G.passes < 0) {
    return fail(c, "derp_gc_run has not been called");
  }
  if (kind < DERP_GC_IFFY || kind > DERP_GC_FINAL) {
    return fail(c, "bad result kind %d", kind);
  }
  if (kind != DERP_GC_IFFY && kind != DERP_GC_FINAL && (pass < 0 || pass >= G.passes)) {
    return fail(c, "pass %d out of range [0, %d)", pass, G.passes);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const GcCam& g = G.camsH[cam];
  const float* base = kind == DERP_GC_IFFY    ? G.iffy.as<float>()
                      : kind == DERP_GC_CLEAN ? G.cleanRun.as<float>() + (size_t)pass * G.pixels
                      : kind == DERP_GC_DEPTH ? G.depthRun.as<float>() + (size_t)pass * G.pixels
                                              : G.cur.as<float>();
  return download_sync(c, out, base + g.offset, (size_t)g.w * g.h * sizeof(float));
}

int derp_gc_stage(derp_ctx* c, int dst, int src, int slice, double disparity_step, int use_clean, double agree_fraction,
                  int16_t* sample, int16_t* average, int16_t* average_of_sq, float* cost) {
  if (!c) {
    return 1;
  }
  TRY(gc_need_upload(c));
  TRY(check_camera(c, dst));
  TRY(check_camera(c, src));
  TRY(gc_check_fraction(c, agree_fraction));
  if (src == dst) {
    return fail(c, "the destination is not one of its own sources");
  }
  GcState& G = *c->gc;
  if (use_clean && !G.haveClean) {
    return fail(c, "derp_gc_set_clean has not been called");
  }
  HIPCHK(c, hipSetDevice(c->device));
  int count = 0;
  TRY(gc_upload_slices(c, G, dst, disparity_step, &count));
  if (slice < 0 || slice >= count) {
    return fail(c, "slice %d out of range [0, %d)", slice, count);
  }
  const GcCam& g = G.camsH[dst];
  const size_t n = (size_t)g.w * g.h;
  ALLOC(c, G.stageSample, n * sizeof(short4));
  ALLOC(c, G.stageAverage, n * sizeof(short4));
  ALLOC(c, G.stageAverageOfSq, n * sizeof(short4));
  ALLOC(c, G.stageCost, n * sizeof(float));
  const GcStageOut so{G.stageSample.as<short4>(), G.stageAverage.as<short4>(), G.stageAverageOfSq.as<short4>(),
                      G.stageCost.as<float>()};
  const int tilesX = (g.w + kGcTile - 1) / kGcTile, tilesY = (g.h + kGcTile - 1) / kGcTile;
  hipLaunchKernelGGL(k_gc_sweep<true>, dim3(tilesX, tilesY, 1), dim3(kGcBlock), 0, c->stream, c->camsDst.as<Cam>(),
                     G.gcams.as<GcCam>(), c->D, dst, G.images.as<short4>(), use_clean ? G.clean.as<float>() : nullptr,
                     agree_fraction, G.slices.as<float>(), count, slice, (float*)nullptr, (int*)nullptr, src, so);
  KCHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (sample) {
    HIPCHK(c, hipMemcpy(sample, G.stageSample.p, n * sizeof(short4), hipMemcpyDeviceToHost));
  }
  if (average) {
    HIPCHK(c, hipMemcpy(average, G.stageAverage.p, n * sizeof(short4), hipMemcpyDeviceToHost));
  }
  if (average_of_sq) {
    HIPCHK(c, hipMemcpy(average_of_sq, G.stageAverageOfSq.p, n * sizeof(short4), hipMemcpyDeviceToHost));
  }
  if (cost) {
    HIPCHK(c, hipMemcpy(cost, G.stageCost.p, n * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 0;
}
