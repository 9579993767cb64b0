// The sibling tools' filters in their host-pointer forms: each call uploads with plain copies, runs the level loop's
// own kernels (derp_kernels.h) on the context's stream and downloads after a synchronise. Included by derp_capi.hip.
#pragma once

// one image: kind 0 = BGR u16 x3, 1 = u8, 2 = f32, 3 = BGR f32 x3 (host in / host out)
int derp_resize_area(derp_ctx* c, int kind, const void* src, int w, int h, void* dst, int dw, int dh) {
  if (!c || !src || !dst || kind < 0 || kind > 3 || w <= 0 || h <= 0 || dw <= 0 || dh <= 0) {
    return fail(c, "bad arguments");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t elem = kind == 0 ? 6 : kind == 1 ? 1 : kind == 3 ? 12 : 4, n = (size_t)w * h, nd = (size_t)dw * dh;
  DevBuf in, out, out3;
  TRY(upload_sync(c, in, src, n * elem));
  ALLOC(c, out, nd * (kind == 0 ? 8 : elem));
  TRY(resize_area_dev(c, kind, in.p, w, h, out.p, dw, dh, -1));
  if (kind == 0) {
    ALLOC(c, out3, nd * 6);
    hipLaunchKernelGGL(k_bgrx_to_bgr, dim3(flat_grid(nd)), dim3(256), 0, c->stream, out.as<ushort4>(),
                       out3.as<uint16_t>(), nd);
  }
  return download_sync(c, dst, kind == 0 ? out3.p : out.p, nd * elem);
}

// ---- GenerateForegroundMasks (source/render/BackgroundSubtractionUtil.h:20-60) ----
int derp_generate_foreground_mask(derp_ctx* c, const uint16_t* template_bgr, const uint16_t* frame_bgr, int w, int h,
                                  int blur_radius, float threshold, int morph_closing_size, uint8_t* mask01) {
  if (!c || !template_bgr || !frame_bgr || !mask01 || w <= 0 || h <= 0 || blur_radius < 0 || blur_radius > 3 ||
      morph_closing_size < 0 || !(threshold >= 0)) {
    return fail(c, "bad arguments (blur_radius must be 0..3)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  DevBuf raw, t4, f4, tb, fb, m0, m1;
  ALLOC(c, t4, n * 8);
  ALLOC(c, f4, n * 8);
  ALLOC(c, m0, n);
  TRY(upload_sync(c, raw, template_bgr, n * 6));
  hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(n)), dim3(256), 0, c->stream, raw.as<uint16_t>(), t4.as<ushort4>(), n);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // `raw` is overwritten by the frame
  TRY(upload_sync(c, raw, frame_bgr, n * 6));
  hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(n)), dim3(256), 0, c->stream, raw.as<uint16_t>(), f4.as<ushort4>(), n);
  const ushort4 *tp = t4.as<ushort4>(), *fp = f4.as<ushort4>();
  if (blur_radius > 0) {
    ALLOC(c, tb, n * 8);
    ALLOC(c, fb, n * 8);
    hipLaunchKernelGGL(k_gauss_u16, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, t4.as<ushort4>(), tb.as<ushort4>(), w, h, blur_radius);
    hipLaunchKernelGGL(k_gauss_u16, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, f4.as<ushort4>(), fb.as<ushort4>(), w, h, blur_radius);
    tp = tb.as<ushort4>();
    fp = fb.as<ushort4>();
  }
  hipLaunchKernelGGL(k_fg_threshold, dim3(flat_grid(n)), dim3(256), 0, c->stream, tp, fp, n, threshold, m0.as<uint8_t>());
  if (morph_closing_size > 0) {
    ALLOC(c, m1, n);
    hipLaunchKernelGGL(k_morph_rect, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, m0.as<uint8_t>(), m1.as<uint8_t>(), w, h, morph_closing_size, 1);
    hipLaunchKernelGGL(k_morph_rect, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, m1.as<uint8_t>(), m0.as<uint8_t>(), w, h, morph_closing_size, 0);
  }
  return download_sync(c, mask01, m0.p, n);
}

// ---- sibling binaries' kernels, host-pointer convenience forms ----
int derp_layer_disparities(derp_ctx* c, const float* foreground, const float* background, size_t n, uint8_t* out) {
  if (!c || !foreground || !background || !out) {
    return fail(c, "bad arguments");
  }
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf f, b, o;
  TRY(upload_sync(c, f, foreground, n * 4));
  TRY(upload_sync(c, b, background, n * 4));
  ALLOC(c, o, n);
  hipLaunchKernelGGL(k_layer_disparities, dim3(flat_grid(n)), dim3(256), 0, c->stream, f.as<float>(), b.as<float>(), n,
                     o.as<uint8_t>());
  return download_sync(c, out, o.p, n);
}
int derp_fov_mask(derp_ctx* c, int d, int w, int h, uint8_t* out) {
  if (!c || !out || d < 0 || d >= c->D || w <= 0 || h <= 0) {
    return fail(c, "bad arguments");
  }
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf m;
  ALLOC(c, m, (size_t)w * h);
  hipLaunchKernelGGL(k_fov_mask, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>() + d, w, h,
                     m.as<uint8_t>());
  return download_sync(c, out, m.p, (size_t)w * h);
}

int derp_upsample_disparity(derp_ctx* c, int d, const float* disp, int w, int h, const float* bg_disp_up,
                            const uint8_t* fg_mask, const uint8_t* fg_mask_up, int w_up, int h_up, int use_fg,
                            float* out) {
  if (!c || !disp || !out || d < 0 || d >= c->D) {
    return fail(c, "bad arguments");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h, nu = (size_t)w_up * h_up;
  DevBuf in, res, m, mu, bg, fov, fovu, idx;
  TRY(upload_sync(c, in, disp, n * 4));
  ALLOC(c, res, nu * 4);
  if (!use_fg) {
    TRY(upsample_lanczos_dev(c, in.as<float>(), w, h, res.as<float>(), w_up, h_up, 1, n, nu));
    return download_sync(c, out, res.p, nu * 4);
  }
  if (!bg_disp_up || !fg_mask || !fg_mask_up) {
    return fail(c, "foreground-mask upsample needs bg_disp_up, fg_mask and fg_mask_up");
  }
  const int zero = 0;
  TRY(upload_sync(c, m, fg_mask, n));
  TRY(upload_sync(c, mu, fg_mask_up, nu));
  TRY(upload_sync(c, bg, bg_disp_up, nu * 4));
  TRY(upload_sync(c, idx, &zero, sizeof(int)));
  ALLOC(c, fov, n);
  ALLOC(c, fovu, nu);
  // fov masks of camera d at both sizes, AND-ed with the fg masks (UpsampleDisparityLib.cpp:163-179)
  hipLaunchKernelGGL(k_fov_mask, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>() + d, w, h,
                     fov.as<uint8_t>());
  hipLaunchKernelGGL(k_fov_mask, grid2d(w_up, h_up, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>() + d, w_up,
                     h_up, fovu.as<uint8_t>());
  hipLaunchKernelGGL(k_and_masks, dim3(flat_grid(n), 1), dim3(256), 0, c->stream, fov.as<uint8_t>(), m.as<uint8_t>(),
                     idx.as<int>(), 0, n, fov.as<uint8_t>());
  hipLaunchKernelGGL(k_and_masks, dim3(flat_grid(nu), 1), dim3(256), 0, c->stream, fovu.as<uint8_t>(), mu.as<uint8_t>(),
                     idx.as<int>(), 0, nu, fovu.as<uint8_t>());
  TRY(upsample_masked_dev(c, in.as<float>(), fov.as<uint8_t>(), w, h, fovu.as<uint8_t>(), bg.as<float>(), res.as<float>(),
                          w_up, h_up));
  return download_sync(c, out, res.p, nu * 4);
}

// The tiled kernel while its tile fits the 64 KiB of LDS a block may have (radius <= 22: 65 280 B plus the kernel's
// 256 B exp table), the untiled one beyond: the same bits either way, so no radius is refused (UpsampleDisparity's is
// scale^2 + 1, UpsampleDisparityLib.cpp:93-96).
template <bool GUIDE_U16>
static void launch_joint_bilateral(derp_ctx* c, const float* image, const void* guide, const uint8_t* mask, int w, int h,
                                   int radius, float sigma, float w0, float w1, float w2, float* out) {
  const size_t n = (size_t)w * h;
  const dim3 grid((w + 15) / 16, (h + 15) / 16, 1);
  if (bilateral_lds_bytes(radius) <= kBilateralMaxLds) {
    if (GUIDE_U16) {  // the level loop's launcher: the fast tap where the parameters allow it
      launch_joint_bilateral_u16_tiled(c, grid, image, guide, mask, w, h, radius, sigma, w0, w1, w2, out, n, n, nullptr);
    } else {
      hipLaunchKernelGGL(k_joint_bilateral<false>, grid, dim3(256), bilateral_lds_bytes(radius), c->stream, image, guide,
                         mask, w, h, radius, sigma, w0, w1, w2, out, n, n, (const int*)nullptr);
    }
  } else {
    hipLaunchKernelGGL(k_joint_bilateral_direct<GUIDE_U16>, grid, dim3(256), 0, c->stream, image, guide, mask, w, h,
                       radius, sigma, w0, w1, w2, out);
  }
}

int derp_joint_bilateral_u16(derp_ctx* c, const float* image, const uint16_t* guide, const uint8_t* mask, int w, int h,
                             int radius, float sigma, float w0, float w1, float w2, float* out) {
  if (!c || !image || !guide || !mask || !out || w <= 0 || h <= 0 || radius < 0 || radius > (1 << 30)) {
    return fail(c, "bad arguments (radius must be in [0, 2^30])");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  DevBuf im, g3, g4, m, res;
  TRY(upload_sync(c, im, image, n * 4));
  TRY(upload_sync(c, g3, guide, n * 6));
  TRY(upload_sync(c, m, mask, n));
  ALLOC(c, g4, n * 8);
  ALLOC(c, res, n * 4);
  hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(n)), dim3(256), 0, c->stream, g3.as<uint16_t>(), g4.as<ushort4>(), n);
  launch_joint_bilateral<true>(c, im.as<float>(), (const void*)g4.as<ushort4>(), m.as<uint8_t>(), w, h, radius, sigma, w0,
                               w1, w2, res.as<float>());
  return download_sync(c, out, res.p, n * 4);
}

int derp_joint_bilateral_f32(derp_ctx* c, const float* image, const float* guide, const uint8_t* mask, int w, int h,
                             int radius, float sigma, float w0, float w1, float w2, float* out) {
  if (!c || !image || !guide || !mask || !out || w <= 0 || h <= 0 || radius < 0 || radius > (1 << 30)) {
    return fail(c, "bad arguments (radius must be in [0, 2^30])");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  DevBuf im, g, m, res;
  TRY(upload_sync(c, im, image, n * 4));
  TRY(upload_sync(c, g, guide, n * 12));
  TRY(upload_sync(c, m, mask, n));
  ALLOC(c, res, n * 4);
  launch_joint_bilateral<false>(c, im.as<float>(), (const void*)g.as<float>(), m.as<uint8_t>(), w, h, radius, sigma, w0, w1,
                                w2, res.as<float>());
  return download_sync(c, out, res.p, n * 4);
}

int derp_masked_median(derp_ctx* c, const float* image, const float* background, const uint8_t* mask, int w, int h,
                       int radius, float* out) {
  if (!c || !image || !mask || !out || radius < 1 || radius > 2) {
    return fail(c, "bad arguments (radius must be 1 or 2)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  DevBuf im, bg, m, res;
  TRY(upload_sync(c, im, image, n * 4));
  if (background) {
    TRY(upload_sync(c, bg, background, n * 4));
  }
  TRY(upload_sync(c, m, mask, n));
  ALLOC(c, res, n * 4);
  hipLaunchKernelGGL(k_masked_median, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, im.as<float>(),
                     background ? bg.as<float>() : (const float*)nullptr, m.as<uint8_t>(), w, h, radius,
                     res.as<float>(), n, (const uint8_t*)nullptr);
  return download_sync(c, out, res.p, n * 4);
}

int derp_temporal_filter_dev(derp_ctx* c, const void* const* guides, const float* const* disps,
                             const uint8_t* const* masks, int n_frames, int w, int h, int frame_offset, float sigma,
                             int space_radius, float w0, float w1, float w2, float* out_dev) {
  if (!c || n_frames < 1 || frame_offset < 0 || frame_offset >= n_frames) {
    return fail(c, "temporal window must hold at least one frame and contain the centre frame");
  }
  HIPCHK(c, hipSetDevice(c->device));
  return temporal_launch(c, guides, disps, masks, n_frames, frame_offset, w, h, 1, sigma, space_radius, w0, w1, w2, out_dev,
                         nullptr);
}

int derp_temporal_filter(derp_ctx* c, const uint16_t* const* guides, const float* const* disps,
                         const uint8_t* const* masks, int n_frames, int w, int h, int frame_offset, float sigma,
                         int space_radius, float w0, float w1, float w2, float* out) {
  if (!c || n_frames < 1) {
    return fail(c, "temporal window must hold at least one frame");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  std::vector<DevBuf> g4(n_frames), im(n_frames), m(n_frames);
  DevBuf g3, res;
  std::vector<const void*> gp(n_frames);
  std::vector<const float*> ip(n_frames);
  std::vector<const uint8_t*> mp(n_frames);
  for (int t = 0; t < n_frames; ++t) {
    ALLOC(c, g4[t], n * 8);
    TRY(upload_sync(c, g3, guides[t], n * 6));
    hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(n)), dim3(256), 0, c->stream, g3.as<uint16_t>(),
                       g4[t].as<ushort4>(), n);
    HIPCHK(c, hipStreamSynchronize(c->stream));  // `g3` is overwritten by the next frame
    TRY(upload_sync(c, im[t], disps[t], n * 4));
    TRY(upload_sync(c, m[t], masks[t], n));
    gp[t] = g4[t].p;
    ip[t] = im[t].as<float>();
    mp[t] = m[t].as<uint8_t>();
  }
  ALLOC(c, res, n * 4);
  TRY(derp_temporal_filter_dev(c, gp.data(), ip.data(), mp.data(), n_frames, w, h, frame_offset, sigma, space_radius, w0,
                               w1, w2, res.as<float>()));
  return download_sync(c, out, res.p, n * 4);
}
