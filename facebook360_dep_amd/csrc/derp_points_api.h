// ExportPointCloud, ImportPointCloud, ProjectEquirectsToCameras: the conversion tools at the depth stage's inputs and
// outputs, host side. Kernels: derp_points.h. Included by derp_capi.hip after the depth core.
#pragma once

namespace {

// derp_points_begin .. derp_points_download: every camera's disparity image in one buffer, and the chunk in flight
struct PointsState {
  DevBuf disp, images, xyz;
  std::vector<PointsImage> imagesH;  // empty: derp_points_begin has not succeeded
};

// Camera::rescale({w, h}) of the rig camera as the file holds it (Camera.cpp:217-223): principal *= new / res and
// focal *= new / res, the quotient first — the order that gives the reference's rescaled camera bit for bit. (The depth
// path's normalised camera x level size rounds differently.) No principal in the file: resolution / 2 (Camera.cpp:44-48).
ScaledCam scaled_cam(const derp_camera_desc& j, int w, int h) {
  const double qx = (double)w / j.resolution[0], qy = (double)h / j.resolution[1];
  const double prx = j.has_principal ? j.principal[0] : j.resolution[0] / 2;
  const double pry = j.has_principal ? j.principal[1] : j.resolution[1] / 2;
  return {prx * qx, pry * qy, j.focal[0] * qx, j.focal[1] * qy, (double)w, (double)h};
}
constexpr size_t kMaxPixels = (size_t)1 << 31;  // one image of these calls (block counts and pixel hashes are 32-bit)
}  // namespace

int derp_export_points(derp_ctx* c, int cam, const float* disparity, int w, int h, const float* color_bgr,
                       double max_depth, int clip, int subsample, float* out_xyzrgb, size_t cap, size_t* count) {
  if (!c || !disparity || !color_bgr || !count || (!out_xyzrgb && cap > 0) || w <= 0 || h <= 0 ||
      (size_t)w * h >= kMaxPixels) {
    return fail(c, "bad arguments (null pointer or image size)");
  }
  *count = 0;
  TRY(check_camera(c, cam));
  if (subsample < 1) {
    return fail(c, "subsample must be >= 1");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  const int nb = (int)blocks_of(n, kPointsBlock);
  DevBuf disp, color, planes, keep, counts, offsets, total, out;
  TRY(upload_sync(c, disp, disparity, n * 4));
  TRY(upload_sync(c, color, color_bgr, n * 12));
  ALLOC(c, planes, n * 24);
  ALLOC(c, keep, n);
  ALLOC(c, counts, (size_t)nb * 4);
  ALLOC(c, offsets, (size_t)nb * 8);
  ALLOC(c, total, 8);
  hipLaunchKernelGGL(k_export_points, dim3(nb), dim3(kPointsBlock), 0, c->stream, c->camsDst.as<Cam>() + cam,
                     scaled_cam(c->descDstH[cam], w, h), (uint32_t)cam, disp.as<float>(), color.as<float>(), w, h, max_depth,
                     clip, (uint32_t)subsample, planes.as<float>(), keep.as<uint8_t>(), counts.as<uint32_t>());
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, counts.as<uint32_t>(), nb,
                     offsets.as<unsigned long long>(), total.as<unsigned long long>());
  KCHECK(c);
  unsigned long long kept = 0;
  TRY(download_sync(c, &kept, total.p, 8));
  *count = (size_t)kept;
  if (kept > cap) {
    return fail(c, "derp_export_points: %llu points do not fit the output's capacity of %zu", kept, cap);
  }
  if (kept == 0) {
    return 0;
  }
  ALLOC(c, out, (size_t)kept * 24);
  hipLaunchKernelGGL(k_export_scatter, dim3(nb), dim3(kPointsBlock), 0, c->stream, planes.as<float>(), keep.as<uint8_t>(), n,
                     offsets.as<unsigned long long>(), out.as<float>());
  KCHECK(c);
  return download_sync(c, out_xyzrgb, out.p, (size_t)kept * 24);
}

int derp_points_begin(derp_ctx* c, const int* widths, const int* heights) {
  if (!c || !widths || !heights) {
    return fail(c, "bad arguments (null pointer)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<PointsImage> images(c->D);
  size_t floats = 0;
  for (int i = 0; i < c->D; ++i) {
    if (widths[i] <= 0 || heights[i] <= 0 || (size_t)widths[i] * heights[i] >= kMaxPixels) {
      return fail(c, "bad image size %d x %d for camera %d", widths[i], heights[i], i);
    }
    images[i] = {scaled_cam(c->descDstH[i], widths[i], heights[i]), (unsigned long long)floats, widths[i], heights[i]};
    floats += (size_t)widths[i] * heights[i];
  }
  if (!c->points) {
    c->points.reset(new PointsState);
  }
  PointsState& P = *c->points;
  P.imagesH.clear();
  ALLOC(c, P.disp, floats * 4);
  TRY(upload_sync(c, P.images, images.data(), images.size() * sizeof(PointsImage)));
  HIPCHK(c, hipMemset(P.disp.p, 0, floats * 4));  // (the images start at 0: ImportPointCloud.cpp:83)
  P.imagesH = images;
  return 0;
}

int derp_points_splat(derp_ctx* c, const double* xyz, size_t n, double min_depth, double max_depth) {
  if (!c || (!xyz && n > 0)) {
    return fail(c, "bad arguments (null pointer)");
  }
  if (!c->points || c->points->imagesH.empty()) {
    return fail(c, "derp_points_begin has not been called");
  }
  if (n == 0) {
    return 0;
  }
  if (n >= kMaxPixels) {
    return fail(c, "derp_points_splat: at most 2^31 - 1 points per call (feed the cloud in chunks)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  // the chunk before this one may still be read by its kernel: wait for it, then the host is free to parse the next
  // chunk while this one's kernel runs
  HIPCHK(c, hipStreamSynchronize(c->stream));
  PointsState& P = *c->points;
  TRY(upload_sync(c, P.xyz, xyz, n * 24));
  hipLaunchKernelGGL(k_points_splat, dim3(blocks_of(n, kPointsBlock)), dim3(kPointsBlock), 0, c->stream, c->camsDst.as<Cam>(),
                     P.images.as<PointsImage>(), c->D, P.xyz.as<double>(), n, min_depth, max_depth, P.disp.as<float>());
  KCHECK(c);
  return 0;
}

int derp_points_download(derp_ctx* c, int cam, float* disparity) {
  if (!c || !disparity) {
    return fail(c, "bad arguments (null pointer)");
  }
  if (!c->points || c->points->imagesH.empty()) {
    return fail(c, "derp_points_begin has not been called");
  }
  TRY(check_camera(c, cam));
  HIPCHK(c, hipSetDevice(c->device));
  const PointsImage& im = c->points->imagesH[cam];
  return download_sync(c, disparity, c->points->disp.as<float>() + im.offset, (size_t)im.w * im.h * 4);
}

int derp_project_equirect_mask(derp_ctx* c, int cam, const uint8_t* eqr, int eqr_w, int eqr_h, int w, int h, double depth,
                               uint8_t* out) {
  if (!c || !eqr || !out || eqr_w <= 0 || eqr_h <= 0 || w <= 0 || h <= 0 || (size_t)w * h >= kMaxPixels ||
      (size_t)eqr_w * eqr_h >= kMaxPixels) {
    return fail(c, "bad arguments (null pointer or image size)");
  }
  TRY(check_camera(c, cam));
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  DevBuf e, m;
  TRY(upload_sync(c, e, eqr, (size_t)eqr_w * eqr_h));
  ALLOC(c, m, n);
  hipLaunchKernelGGL(k_project_equirect_mask, dim3(blocks_of(n, kPointsBlock)), dim3(kPointsBlock), 0, c->stream,
                     c->camsDst.as<Cam>() + cam, scaled_cam(c->descDstH[cam], w, h), e.as<uint8_t>(), eqr_w, eqr_h, w, h, depth,
                     m.as<uint8_t>());
  KCHECK(c);
  return download_sync(c, out, m.p, n);
}
