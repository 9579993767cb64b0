// AlignColors (source/calibration/AlignColors.cpp), host side: the red and blue camera models derived from the three
// one-camera reference rigs (host only), the warp maps of every camera of the context's rig (built once, downloadable),
// and one frame of every camera resampled through them. Kernels: derp_align.h. Definitions: DESIGN §8.8. Included by
// derp_capi.hip after the depth core.
#pragma once

namespace {

struct AlignState {
  std::vector<AlignCam> camsH;  // empty: derp_align_setup has not succeeded
  size_t pixels = 0;            // of all cameras together, each padded to a multiple of kAlignPad
  DevBuf cams, red, blue, in, out;
};

// getScalarFocal (Camera.cpp:185-188)
const char* align_scalar_focal(const derp_camera_desc& j, double* focal) {
  if (j.focal[0] != -j.focal[1]) {
    return "Check failed: focal.x() == -focal.y() pixels are not square";
  }
  *focal = j.focal[0];
  return nullptr;
}

// createCalibratedRBRigs for one camera (AlignColors.cpp:79-94): red / blue = the green camera with the reference
// channel's focal times a FLOAT ratio and the reference channel's distortion
const char* align_derive(const derp_camera_desc& green, const derp_camera_desc& redRef, const derp_camera_desc& greenRef,
                         const derp_camera_desc& blueRef, derp_camera_desc* red, derp_camera_desc* blue) {
  double greenFocal, refFocal[3];
  const derp_camera_desc* refs[3] = {&greenRef, &redRef, &blueRef};
  if (const char* err = align_scalar_focal(green, &greenFocal)) {
    return err;
  }
  for (int k = 0; k < 3; ++k) {
    if (const char* err = align_scalar_focal(*refs[k], &refFocal[k])) {
      return err;
    }
  }
  const float focalRatio = (float)(greenFocal / refFocal[0]);  // (:87)
  derp_camera_desc* outs[2] = {red, blue};
  for (int k = 0; k < 2; ++k) {
    derp_camera_desc& o = *outs[k];
    const derp_camera_desc& ref = *refs[k + 1];
    o = green;
    const double scalar = refFocal[k + 1] * (double)focalRatio;  // setScalarFocal (Camera.cpp:181-183)
    o.focal[0] = scalar;
    o.focal[1] = -scalar;
    o.has_distortion = ref.has_distortion;  // setDistortion(getDistortion()): distortionMax follows in host_prepare_camera
    for (int i = 0; i < 3; ++i) {
      o.distortion[i] = ref.has_distortion ? ref.distortion[i] : 0.0;
    }
  }
  return nullptr;
}

int align_need_setup(derp_ctx* c) {
  if (!c->align || c->align->camsH.empty()) {
    return fail(c, "derp_align_setup has not been called");
  }
  return 0;
}

}  // namespace

// ---- host only: no context and no device ----
int derp_align_derive_cameras(const derp_camera_desc* green, const derp_camera_desc* red_ref, const derp_camera_desc* green_ref,
                              const derp_camera_desc* blue_ref, derp_camera_desc* red, derp_camera_desc* blue) {
  if (!green || !red_ref || !green_ref || !blue_ref || !red || !blue) {
    return create_fail("derp_align_derive_cameras: bad arguments (null pointer)");
  }
  if (const char* err = align_derive(*green, *red_ref, *green_ref, *blue_ref, red, blue)) {
    return create_fail(std::string("derp_align_derive_cameras: camera ") + green->id + ": " + err);
  }
  return 0;
}

// ---- device ----
int derp_align_setup(derp_ctx* c, const derp_camera_desc* red_ref, int n_red, const derp_camera_desc* green_ref, int n_green,
                     const derp_camera_desc* blue_ref, int n_blue) {
  if (!c || !red_ref || !green_ref || !blue_ref) {
    return fail(c, "bad arguments (null pointer)");
  }
  if (n_red != 1 || n_green != 1 || n_blue != 1) {  // CHECK_EQ(greenRig.size(), 1) ... (AlignColors.cpp:164-166), up front
    return fail(c, "a reference rig must hold exactly one camera (red %d, green %d, blue %d)", n_red, n_green, n_blue);
  }
  std::vector<AlignCam> t(c->D);
  size_t pixels = 0;
  for (int i = 0; i < c->D; ++i) {
    const derp_camera_desc& g = c->descDstH[i];
    derp_camera_desc models[3];
    models[0] = g;
    if (const char* err = align_derive(g, *red_ref, *green_ref, *blue_ref, &models[1], &models[2])) {
      return fail(c, "camera %s: %s", g.id, err);
    }
    AlignCam& a = t[i];
    for (int k = 0; k < 3; ++k) {
      if (const char* err = host_prepare_camera(models[k], a.lens[k])) {
        return fail(c, "camera %s: %s", g.id, err);
      }
      a.focal[k] = models[k].focal[0];
    }
    a.principal[0] = g.has_principal ? g.principal[0] : g.resolution[0] / 2;
    a.principal[1] = g.has_principal ? g.principal[1] : g.resolution[1] / 2;
    // int(resolution) as createWarpMap and warpImage take it (:53-54, :171-172)
    if (!(g.resolution[0] >= 1) || !(g.resolution[1] >= 1) || g.resolution[0] * g.resolution[1] >= (double)kMaxPixels) {
      return fail(c, "camera %s: bad resolution %g x %g", g.id, g.resolution[0], g.resolution[1]);
    }
    a.w = (int)g.resolution[0];
    a.h = (int)g.resolution[1];
    a.offset = (unsigned long long)pixels;
    pixels += ((size_t)a.w * a.h + kAlignPad - 1) / kAlignPad * kAlignPad;
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->align) {
    c->align.reset(new AlignState);
  }
  AlignState& S = *c->align;
  S.camsH.clear();
  ALLOC(c, S.red, pixels * sizeof(float2));
  ALLOC(c, S.blue, pixels * sizeof(float2));
  ALLOC(c, S.in, pixels * 3 * sizeof(uint16_t));
  ALLOC(c, S.out, pixels * 3 * sizeof(uint16_t));
  TRY(upload_sync(c, S.cams, t.data(), t.size() * sizeof(AlignCam)));
  {
    Span sp(c, ST_ALIGN_MAPS, 0);
    for (int i = 0; i < c->D; ++i) {
      hipLaunchKernelGGL(k_align_maps, dim3(blocks_of((size_t)t[i].w * t[i].h, kAlignBlock)), dim3(kAlignBlock), 0, c->stream,
                         S.cams.as<AlignCam>(), i, S.red.as<float2>(), S.blue.as<float2>());
    }
    KCHECK(c);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  S.pixels = pixels;
  S.camsH = t;
  return 0;
}

int derp_align_maps(derp_ctx* c, int cam, float* red_xy, float* blue_xy) {
  if (!c || !red_xy || !blue_xy) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(align_need_setup(c));
  TRY(check_camera(c, cam));
  HIPCHK(c, hipSetDevice(c->device));
  const AlignState& S = *c->align;
  const AlignCam& a = S.camsH[cam];
  const size_t bytes = (size_t)a.w * a.h * sizeof(float2);
  TRY(download_sync(c, red_xy, S.red.as<float2>() + a.offset, bytes));
  return download_sync(c, blue_xy, S.blue.as<float2>() + a.offset, bytes);
}

int derp_align_frame(derp_ctx* c, const uint16_t* const* bgr, const int* img_w, const int* img_h, uint16_t* const* out) {
  if (!c || !bgr || !img_w || !img_h || !out) {
    return fail(c, "bad arguments (null pointer)");
  }
  TRY(align_need_setup(c));
  AlignState& S = *c->align;
  size_t maxPairs = 0;
  for (int i = 0; i < c->D; ++i) {
    const AlignCam& a = S.camsH[i];
    if (!bgr[i] || !out[i]) {
      return fail(c, "camera %d: null image", i);
    }
    if (img_w[i] != a.w || img_h[i] != a.h) {
      return fail(c, "camera %d (%s): the image is %d x %d, the camera's resolution %d x %d", i, c->descDstH[i].id, img_w[i],
                  img_h[i], a.w, a.h);
    }
    maxPairs = std::max(maxPairs, ((size_t)a.w * a.h + 1) / 2);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < c->D; ++i) {
    const AlignCam& a = S.camsH[i];
    HIPCHK(c, hipMemcpy(S.in.as<uint16_t>() + a.offset * 3, bgr[i], (size_t)a.w * a.h * 3 * sizeof(uint16_t), hipMemcpyHostToDevice));
  }
  {
    Span sp(c, ST_ALIGN_COLORS, 0);
    hipLaunchKernelGGL(k_align_colors, dim3(blocks_of(maxPairs, (size_t)kAlignBlock * kAlignPairs), c->D), dim3(kAlignBlock), 0, c->stream,
                       S.cams.as<AlignCam>(), S.red.as<float2>(), S.blue.as<float2>(), S.in.as<uint16_t>(), S.out.as<uint16_t>());
    KCHECK(c);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < c->D; ++i) {
    const AlignCam& a = S.camsH[i];
    HIPCHK(c, hipMemcpy(out[i], S.out.as<uint16_t>() + a.offset * 3, (size_t)a.w * a.h * 3 * sizeof(uint16_t), hipMemcpyDeviceToHost));
  }
  return 0;
}
