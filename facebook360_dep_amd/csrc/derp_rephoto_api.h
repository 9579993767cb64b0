// ComputeRephotographyErrors, host side: SSIM / NCC score, forward-splat rephotograph, canopy cubemap. Kernels:
// derp_kernels.h. Included by derp_capi.hip after derp_render_api.h, whose mip geometry the cubemap shares.
#pragma once

namespace {

struct RephotoState {
  DevBuf color, disp;  // derp_rephotograph_upload: S planes of BGR u16 / f32 disparity
  int w = 0, h = 0;    // their size (0: no upload succeeded yet)
  DevBuf cnVert, cnRgba, cnZ, cnAcc, cnOut, cnBig, cnNBig;  // derp_canopy_cubemap's buffers, kept between calls
};

int need_rephoto(derp_ctx* c) {
  if (!c->rephoto || c->rephoto->w <= 0) {
    return fail(c, "derp_rephotograph_upload has not been called");
  }
  return 0;
}

}  // namespace

// ---- rephotography score (RephotographyUtil.h:38-116, ComputeRephotographyErrors.cpp:69-189) ----
int derp_ssim(derp_ctx* c, const float* x_bgr, const float* y_bgr, int w, int h, int blur_radius, float alpha,
              float beta, float gamma, float* score_bgr) {
  auto is01 = [](float v) { return v == 0.0f || v == 1.0f; };
  if (!c || !x_bgr || !y_bgr || !score_bgr || w <= 0 || h <= 0 || blur_radius < 1 || blur_radius > 15) {
    return fail(c, "bad arguments (blur_radius must be 1..15)");
  }
  if (!is01(alpha) || !is01(beta) || !is01(gamma)) {
    return fail(c, "exponents other than 0 and 1 are not supported (computeScoreMap uses MSSIM = 1,1,1 / NCC = 0,0,1)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  // getGaussianKernel(2r + 1, 1.5, CV_32F): OpenCV 4's order of operations, in double, rounded to float
  GaussCoef coef{};
  {
    const int n = 2 * blur_radius + 1;
    const double sigma = 1.5f, scale2X = -0.125 / (sigma * sigma);
    double t[16], sum = 0;
    for (int i = 0, x = 1 - n; i < blur_radius; ++i, x += 2) {
      t[i] = std::exp((double)(x * x) * scale2X);
      sum += t[i];
    }
    sum *= 2;
    sum += 1;
    const double mul = 1.0 / sum;
    coef.k[0] = (float)mul;
    for (int i = 0; i < blur_radius; ++i) {
      coef.k[blur_radius - i] = (float)(t[i] * mul);
    }
  }
  const size_t n3 = (size_t)w * h * 3, bytes = n3 * 4;
  DevBuf x, y, muX, muY, a, b, cc, tmp, s2x, s2y, sxy;
  TRY(upload_sync(c, x, x_bgr, bytes));
  TRY(upload_sync(c, y, y_bgr, bytes));
  for (DevBuf* buf : {&muX, &muY, &a, &b, &cc, &tmp, &s2x, &s2y, &sxy}) {
    ALLOC(c, *buf, bytes);
  }
  const dim3 grid = grid2d(w * 3, h, 1, kBlk2d);
  auto blur = [&](const DevBuf& in, DevBuf& out) {
    hipLaunchKernelGGL(k_gauss_f32c3, grid, kBlk2d, 0, c->stream, in.as<float>(), tmp.as<float>(), w, h, blur_radius, coef, 0);
    hipLaunchKernelGGL(k_gauss_f32c3, grid, kBlk2d, 0, c->stream, tmp.as<float>(), out.as<float>(), w, h, blur_radius, coef, 1);
  };
  blur(x, muX);
  blur(y, muY);
  hipLaunchKernelGGL(k_ssim_moments, dim3(flat_grid(n3)), dim3(256), 0, c->stream, x.as<float>(), y.as<float>(),
                     muX.as<float>(), muY.as<float>(), a.as<float>(), b.as<float>(), cc.as<float>(), n3);
  blur(a, s2x);
  blur(b, s2y);
  blur(cc, sxy);
  // the score overwrites `a`
  hipLaunchKernelGGL(k_ssim_score, dim3(flat_grid(n3)), dim3(256), 0, c->stream, muX.as<float>(), muY.as<float>(),
                     s2x.as<float>(), s2y.as<float>(), sxy.as<float>(), alpha != 0.0f, beta != 0.0f, gamma != 0.0f,
                     a.as<float>(), n3);
  return download_sync(c, score_bgr, a.p, bytes);
}

int derp_average_score(const float* score_bgr, const uint8_t* mask, int w, int h, double* avg_bgr3) {
  if (!score_bgr || !mask || !avg_bgr3 || w <= 0 || h <= 0) {
    return 1;
  }
  const size_t n = (size_t)w * h;
  for (int ch = 0; ch < 3; ++ch) {
    double sum = 0;
    size_t cnt = 0;
    for (size_t i = 0; i < n; ++i) {
      const float v = score_bgr[i * 3 + ch];
      if (mask[i] && !std::isnan(v)) {
        sum += v;
        ++cnt;
      }
    }
    avg_bgr3[ch] = cnt ? sum / (double)cnt : 0.0;
  }
  return 0;
}

int derp_rephotograph_upload(derp_ctx* c, const uint16_t* const* colors, const float* const* disparities, int w, int h) {
  if (!c || !colors || !disparities || w <= 0 || h <= 0) {
    return fail(c, "bad arguments");
  }
  if ((size_t)w * h > (1u << 24) || c->S > 256) {
    return fail(c, "rephotography keys hold 24 bits of pixel index and 8 bits of camera index");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  if (!c->rephoto) {
    c->rephoto.reset(new RephotoState);
  }
  RephotoState& R = *c->rephoto;
  R.w = R.h = 0;
  ALLOC(c, R.color, (size_t)c->S * n * 6);
  ALLOC(c, R.disp, (size_t)c->S * n * 4);
  for (int s = 0; s < c->S; ++s) {
    if (!colors[s] || !disparities[s]) {
      return fail(c, "null colour / disparity for source %d", s);
    }
    HIPCHK(c, hipMemcpy((char*)R.color.p + (size_t)s * n * 6, colors[s], n * 6, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy((char*)R.disp.p + (size_t)s * n * 4, disparities[s], n * 4, hipMemcpyHostToDevice));
  }
  R.w = w;
  R.h = h;
  return 0;
}

int derp_rephotograph_render(derp_ctx* c, int target, float* out_bgra) {
  if (!c || !out_bgra || target < 0 || target >= c->S) {
    return fail(c, "bad arguments");
  }
  TRY(need_rephoto(c));
  HIPCHK(c, hipSetDevice(c->device));
  const RephotoState& R = *c->rephoto;
  const int w = R.w, h = R.h;
  const size_t n = (size_t)w * h;
  DevBuf key, out;
  ALLOC(c, key, n * 8);
  ALLOC(c, out, n * 16);
  HIPCHK(c, hipMemsetAsync(key.p, 0xff, n * 8, c->stream));
  hipLaunchKernelGGL(k_rephoto_splat, grid2d(w, h, c->S, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), target,
                     R.disp.as<float>(), w, h, key.as<unsigned long long>());
  hipLaunchKernelGGL(k_rephoto_resolve, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), target,
                     R.color.as<uint16_t>(), key.as<unsigned long long>(), w, h, out.as<float4>());
  return download_sync(c, out_bgra, out.p, n * 16);
}

int derp_rephotograph(derp_ctx* c, int target, const uint16_t* const* colors, const float* const* disparities, int w,
                      int h, float* out_bgra) {
  if (!c || target < 0 || target >= c->S) {
    return fail(c, "bad arguments");
  }
  TRY(derp_rephotograph_upload(c, colors, disparities, w, h));
  return derp_rephotograph_render(c, target, out_bgra);
}

// CanopyScene::cubemap for the cameras `include[s] != 0` of the last derp_rephotograph_upload, seen from
// `centre` (rig space): BGRA float [6 * edge][edge] (ComputeRephotographyErrors.cpp:77-95 generateCubemaps)
int derp_canopy_cubemap(derp_ctx* c, const uint8_t* include, const double* centre, int edge, float* out_bgra) {
  if (!c || !include || !centre || !out_bgra || edge < 1 || edge > 8192) {
    return fail(c, "bad arguments");
  }
  TRY(need_rephoto(c));
  HIPCHK(c, hipSetDevice(c->device));
  RephotoState& R = *c->rephoto;
  const int w = R.w, h = R.h, E = edge;
  const size_t n = (size_t)w * h, nf = (size_t)E * E;
  CanopyMips M;  // mip chain geometry (glGenerateMipmap)
  size_t texels = 0;
  if (!smr_mips(w, h, M, texels)) {
    return fail(c, "image too large for the mip chain");
  }
  int nInc = 0;
  for (int s = 0; s < c->S; ++s) {
    nInc += include[s] != 0;
  }
  // per included camera: mesh vertices + the colour mip chain, built once and reused by the six faces
  DevBuf &vert = R.cnVert, &rgba = R.cnRgba, &zbuf = R.cnZ, &acc = R.cnAcc, &out = R.cnOut, &big = R.cnBig, &nBig = R.cnNBig;
  if (vert.ensure((size_t)std::max(nInc, 1) * n * 16) || rgba.ensure((size_t)std::max(nInc, 1) * texels * 16) ||
      zbuf.ensure(nf * 8) || acc.ensure(nf * 16) || out.ensure(nf * 6 * 16) || big.ensure(n * 2 * sizeof(unsigned)) ||
      nBig.ensure(sizeof(unsigned))) {
    return fail(c, "out of device memory");
  }
  const float cx = (float)centre[0], cy = (float)centre[1], cz = (float)centre[2];  // position.cast<float>()
  std::vector<int> slotOf(c->S, -1);
  for (int s = 0, k = 0; s < c->S; ++s) {
    if (!include[s]) {
      continue;
    }
    slotOf[s] = k;
    float4* v = vert.as<float4>() + (size_t)k * n;
    float4* tex = rgba.as<float4>() + (size_t)k * texels;
    hipLaunchKernelGGL(k_canopy_mesh, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), s,
                       R.color.as<uint16_t>() + (size_t)s * n * 3, R.disp.as<float>() + (size_t)s * n, w, h, v, tex);
    smr_build_mips(c, tex, M);
    ++k;
  }
  // the reference's order: face-outer, camera-inner (the accumulation order of the cameras is part of the result)
  for (int face = 0; face < 6; ++face) {
    (void)hipMemsetAsync(acc.p, 0, nf * 16, c->stream);
    for (int s = 0; s < c->S; ++s) {
      if (!include[s]) {
        continue;
      }
      const float4* v = vert.as<float4>() + (size_t)slotOf[s] * n;
      const float4* tex = rgba.as<float4>() + (size_t)slotOf[s] * texels;
      (void)hipMemsetAsync(zbuf.p, 0, nf * 8, c->stream);
      (void)hipMemsetAsync(nBig.p, 0, sizeof(unsigned), c->stream);
      hipLaunchKernelGGL(k_canopy_raster, grid2d(w - 1, h - 1, 2, kBlk2d), kBlk2d, 0, c->stream, v, tex, M, w, h, cx, cy, cz,
                         face, E, zbuf.as<unsigned long long>(), big.as<unsigned>(), nBig.as<unsigned>());
      hipLaunchKernelGGL(k_canopy_raster_big, dim3(4096), dim3(256), 0, c->stream, v, tex, M, w, h, cx, cy, cz, face, E,
                         zbuf.as<unsigned long long>(), big.as<unsigned>(), nBig.as<unsigned>());
      hipLaunchKernelGGL(k_canopy_resolve, grid2d(E, E, 1, kBlk2d), kBlk2d, 0, c->stream, v, tex, M, w, h, cx, cy, cz, face, E,
                         zbuf.as<unsigned long long>(), acc.as<float4>());
    }
    hipLaunchKernelGGL(k_canopy_finish, grid2d(E, E, 1, kBlk2d), kBlk2d, 0, c->stream, acc.as<float4>(), face, E,
                       out.as<float4>());
    KCHECK(c);
  }
  return download_sync(c, out_bgra, out.p, nf * 6 * 16);
}
