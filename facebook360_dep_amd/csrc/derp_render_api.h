// SimpleMeshRenderer, host side: the scene, its views and passes, the derp_render_* entry points (which
// include/derp_hip.h declares extern "C"). Kernels: derp_render.h. Included by derp_capi.hip after the depth core.
#pragma once

namespace {

// derp_render_*: SimpleMeshRenderer's scene (derp_render.h)
struct SmrCam {
  int dw = 0, dh = 0, tw = 0, th = 0;  // disparity (mesh) and colour texture sizes
  CanopyMips Mc, Md;                   // mip geometry of the colour texture and of the disparity-colour texture
  DevBuf vert, eyeVert, texColor, texDisp;
  float eyeIpd = 0.0f;  // ipdm eyeVert was computed for (0: none yet)
};
struct SmrState {
  std::vector<SmrCam> cams;
  bool haveColor = false;
  bool dispValid = false;
  float dispPos[3] = {0, 0, 0};  // position the disparity colours were computed for
  DevBuf zbuf, acc, big, nBig, cube, img, img2, tabs, back, equi, fetch, staging;
};

// glGenerateMipmap's level sizes (halve, round down, never below 1); false when the chain does not fit (also canopy's)
bool smr_mips(int w, int h, CanopyMips& M, size_t& texels) {
  M.n = 0;
  texels = 0;
  for (int lw = w, lh = h;; lw = std::max(1, lw >> 1), lh = std::max(1, lh >> 1)) {
    if (M.n >= kCanopyMaxLevels) {
      return false;
    }
    M.w[M.n] = lw;
    M.h[M.n] = lh;
    M.off[M.n] = (unsigned)texels;
    texels += (size_t)lw * lh;
    ++M.n;
    if (lw == 1 && lh == 1) {
      return true;
    }
  }
}

void smr_build_mips(derp_ctx* c, float4* tex, const CanopyMips& M) {
  for (int l = 1; l < M.n; ++l) {
    hipLaunchKernelGGL(k_canopy_mip, grid2d(M.w[l], M.h[l], 1, kBlk2d), kBlk2d, 0, c->stream, tex + M.off[l - 1], M.w[l - 1],
                       M.h[l - 1], tex + M.off[l], M.w[l], M.h[l]);
  }
}

struct F3 {
  float x, y, z;
};
F3 f3_cross(F3 a, F3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
F3 f3_norm(F3 a) {
  const float n = std::sqrt((a.x * a.x + a.y * a.y) + a.z * a.z);
  return {a.x / n, a.y / n, a.z / n};
}
// posForwardUp (SimpleMeshRenderer.cpp:243-263): rows right, up, -forward
void smr_pos_forward_up(const derp_render_params& p, float R[3][3]) {
  const F3 fwd = {(float)p.forward[0], (float)p.forward[1], (float)p.forward[2]};
  const F3 up = {(float)p.up[0], (float)p.up[1], (float)p.up[2]};
  const F3 back = {-fwd.x, -fwd.y, -fwd.z};
  const F3 right = f3_cross(up, back);
  const F3 f = f3_norm(fwd), u = f3_norm(f3_cross(right, fwd));
  const F3 nf = {-f.x, -f.y, -f.z};
  const F3 r = f3_cross(u, nf);
  const F3 rows[3] = {r, u, nf};
  for (int k = 0; k < 3; ++k) {
    R[k][0] = rows[k].x;
    R[k][1] = rows[k].y;
    R[k][2] = rows[k].z;
  }
}
// xMax = kNearZ * tan(fov / 2) (SimpleMeshRenderer.cpp:292, 390)
float smr_xmax(const derp_render_params& p) {
  return (float)(0.1f * std::tan(p.horizontal_fov / 180 * M_PI / 2));
}
SmrView smr_snapshot_view(const derp_render_params& p) {
  SmrView V;
  smr_pos_forward_up(p, V.R);
  for (int k = 0; k < 3; ++k) {
    V.c[k] = (float)p.position[k];
  }
  // frustum(-xMax, xMax, -yMax, yMax, kNearZ): clip.x = 2 n / (2 xMax) eye.x, clip.w = -eye.z
  const float n = 0.1f, xMax = smr_xmax(p), yMax = xMax * p.height / p.width;
  V.kx = 2 * n / (xMax - -xMax);
  V.ky = 2 * n / (yMax - -yMax);
  V.W = p.width;
  V.H = p.height;
  return V;
}
SmrView smr_face_view(const derp_render_params& p, int face, int E) {
  // createCubemapTexture (CanopyScene.cpp:345-383): rows sc, tc, -major axis; 90-degree frustum
  static const int axes[6][3][2] = {{{0, +1}, {2, -1}, {1, -1}}, {{0, -1}, {2, +1}, {1, -1}}, {{1, +1}, {0, +1}, {2, +1}},
                                    {{1, -1}, {0, +1}, {2, -1}}, {{2, +1}, {0, +1}, {1, -1}}, {{2, -1}, {0, -1}, {1, -1}}};
  SmrView V;
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) {
      V.R[r][k] = 0.0f;
    }
  }
  V.R[0][axes[face][1][0]] = (float)axes[face][1][1];
  V.R[1][axes[face][2][0]] = (float)axes[face][2][1];
  V.R[2][axes[face][0][0]] = (float)-axes[face][0][1];
  for (int k = 0; k < 3; ++k) {
    V.c[k] = (float)p.position[k];
  }
  V.kx = V.ky = 1.0f;
  V.W = V.H = E;
  return V;
}

// the scene's cameras in `cams` rendered in view V (CanopyScene::render): accumulate, un-premultiply into out
int smr_view(derp_ctx* c, const SmrView& V, const std::vector<int>& cams, const derp_render_params& p, int flip, float4* out) {
  SmrState& S = *c->smr;
  const size_t nf = (size_t)V.W * V.H;
  size_t maxTri = 1;
  for (int s : cams) {
    maxTri = std::max(maxTri, (size_t)S.cams[s].dw * S.cams[s].dh * 2);
  }
  ALLOC(c, S.zbuf, nf * 8);
  ALLOC(c, S.acc, nf * 16);
  ALLOC(c, S.big, maxTri * sizeof(unsigned));
  ALLOC(c, S.nBig, sizeof(unsigned));
  (void)hipMemsetAsync(S.acc.p, 0, nf * 16, c->stream);
  for (int s : cams) {  // the reference's order: cameras in rig order, each a full canopy pass
    SmrCam& k = S.cams[s];
    const float4* v = (p.ipd != 0.0f ? k.eyeVert : k.vert).as<float4>();
    const float4* tex = (p.disparity_color ? k.texDisp : k.texColor).as<float4>();
    const CanopyMips& M = p.disparity_color ? k.Md : k.Mc;
    (void)hipMemsetAsync(S.zbuf.p, 0, nf * 8, c->stream);
    (void)hipMemsetAsync(S.nBig.p, 0, sizeof(unsigned), c->stream);
    hipLaunchKernelGGL(k_smr_raster, grid2d(k.dw - 1, k.dh - 1, 2, kBlk2d), kBlk2d, 0, c->stream, v, k.dw, k.dh, tex, M, V,
                       S.zbuf.as<unsigned long long>(), S.big.as<unsigned>(), S.nBig.as<unsigned>());
    hipLaunchKernelGGL(k_smr_raster_big, dim3(4096), dim3(256), 0, c->stream, v, k.dw, k.dh, tex, M, V,
                       S.zbuf.as<unsigned long long>(), S.big.as<unsigned>(), S.nBig.as<unsigned>());
    hipLaunchKernelGGL(k_smr_resolve, grid2d(V.W, V.H, 1, kBlk2d), kBlk2d, 0, c->stream, v, k.dw, k.dh, tex, M, V,
                       p.weight == DERP_WEIGHT_SVD ? 1 : 0, p.alpha_blend ? 1 : 0, S.zbuf.as<unsigned long long>(),
                       S.acc.as<float4>());
  }
  hipLaunchKernelGGL(k_smr_finish, grid2d(V.W, V.H, 1, kBlk2d), kBlk2d, 0, c->stream, S.acc.as<float4>(), V.W, V.H,
                     p.zero_nans ? 1 : 0, flip, out);
  KCHECK(c);
  return 0;
}

// per-render inputs: the disparity colours seen from p.position, the stereo vertices for p.ipd
int smr_prepare(derp_ctx* c, const derp_render_params& p, const std::vector<int>& cams) {
  SmrState& S = *c->smr;
  const float pos[3] = {(float)p.position[0], (float)p.position[1], (float)p.position[2]};  // position.cast<float>()
  if (p.disparity_color && !(S.dispValid && std::memcmp(pos, S.dispPos, sizeof pos) == 0)) {
    for (size_t s = 0; s < S.cams.size(); ++s) {
      SmrCam& k = S.cams[s];
      hipLaunchKernelGGL(k_smr_texture, grid2d(k.dw, k.dh, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), (int)s,
                         (const float4*)nullptr, k.vert.as<float4>(), pos[0], pos[1], pos[2], k.dw, k.dh, k.texDisp.as<float4>());
      smr_build_mips(c, k.texDisp.as<float4>(), k.Md);
    }
    std::memcpy(S.dispPos, pos, sizeof pos);
    S.dispValid = true;
  }
  if (p.ipd != 0.0f) {
    for (int s : cams) {
      SmrCam& k = S.cams[s];
      if (k.eyeIpd != p.ipd) {
        const size_t n = (size_t)k.dw * k.dh;
        ALLOC(c, k.eyeVert, n * 16);
        hipLaunchKernelGGL(k_smr_stereo, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, k.vert.as<float4>(), n,
                           p.ipd, k.eyeVert.as<float4>());
        k.eyeIpd = p.ipd;
      }
    }
  }
  KCHECK(c);
  return 0;
}

// equirectFS over the fullscreen triangle on the cube texture `cube` (six E x E faces, GL rows) -> out [E][2 E]:
// texVar = (pixel centre) / size, GL rows read bottom-up and not flipped, so output row r has
// texVar.y = (r + 0.5) / H and lat = -(texVar.y - 0.5) pi: row 0 is the north pole. `tabs` is the caller's scratch.
int smr_cube_to_equirect(derp_ctx* c, const float4* cube, int E, DevBuf& tabs, float4* out) {
  const int W = 2 * E;
  std::vector<float> tab((size_t)2 * (W + E));
  for (int x = 0; x < W; ++x) {
    const double lon = (1 - (x + 0.5) / W) * 2.0 * M_PI;
    tab[2 * x] = (float)std::cos(lon);
    tab[2 * x + 1] = (float)std::sin(lon);
  }
  for (int r = 0; r < E; ++r) {
    const double lat = -((r + 0.5) / E - 0.5) * M_PI;
    tab[2 * W + 2 * r] = (float)std::cos(lat);
    tab[2 * W + 2 * r + 1] = (float)std::sin(lat);
  }
  ALLOC(c, tabs, tab.size() * 4);
  HIPCHK(c, hipMemcpyAsync(tabs.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_smr_equirect, grid2d(W, E, 1, kBlk2d), kBlk2d, 0, c->stream, cube, E, tabs.as<float>(),
                     tabs.as<float>() + 2 * W, W, E, out);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // `tab` goes out of scope
  return 0;
}

// one derp_render image into the device buffer `out` (CanopyScene::cubemap / equirect, the snapshot)
int smr_image(derp_ctx* c, const derp_render_params& p, const uint8_t* include, float4* out) {
  SmrState& S = *c->smr;
  std::vector<int> cams;
  for (int s = 0; s < (int)S.cams.size(); ++s) {
    if (!include || include[s]) {
      cams.push_back(s);
    }
  }
  if (!p.disparity_color && !S.haveColor) {
    return fail(c, "a colour rendering needs colour textures (derp_render_upload got none)");
  }
  TRY(smr_prepare(c, p, cams));
  const int E = p.height;
  if (p.kind == DERP_RENDER_SNAPSHOT) {
    return smr_view(c, smr_snapshot_view(p), cams, p, 1, out);  // glReadPixels + cv::flip
  }
  if (p.kind == DERP_RENDER_CUBE) {  // glGetTexImage per face, stacked bottom to top, then flipped
    for (int face = 0; face < 6; ++face) {
      TRY(smr_view(c, smr_face_view(p, face, E), cams, p, 1, out + (size_t)face * E * E));
    }
    return 0;
  }
  ALLOC(c, S.cube, (size_t)6 * E * E * 16);
  for (int face = 0; face < 6; ++face) {  // the cube texture keeps GL rows
    TRY(smr_view(c, smr_face_view(p, face, E), cams, p, 0, S.cube.as<float4>() + (size_t)face * E * E));
  }
  return smr_cube_to_equirect(c, S.cube.as<float4>(), E, S.tabs, out);
}

// backgroundEquirect's nearest fetch (SimpleMeshRenderer.cpp:285-330) for a w x h image: the snapshot camera's ray
// through each pixel, in the reference's float arithmetic; the reference reads equi(equiY, equiX) with the indices
// truncated, one past the last row / column when lat = -90 degrees or lon = -180 degrees: clamped here
void smr_fetch_table(const derp_render_params& p, int w, int h, int ew, int eh, std::vector<int>& fetch) {
  float R[3][3];
  smr_pos_forward_up(p, R);
  const float xMax = smr_xmax(p), kNearZ = 0.1f;
  const float pos[3] = {(float)p.position[0], (float)p.position[1], (float)p.position[2]};
  fetch.resize((size_t)2 * w * h);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) {
      const float px = ((x + 0.5f) / w * 2 - 1) * xMax, py = -((y + 0.5f) / h * 2 - 1) * xMax * h / w, pz = -kNearZ;
      const float v[3] = {(float)(1e4 * px), (float)(1e4 * py), (float)(1e4 * pz)};  // kNearInfinity * pixel
      float wd[3];  // inverse of posForwardUp: R^T v + position
      for (int k = 0; k < 3; ++k) {
        wd[k] = (R[0][k] * v[0] + R[1][k] * v[1]) + R[2][k] * v[2] + pos[k];
      }
      const float lon = std::atan2(-wd[1], -wd[0]);
      const float n = std::sqrt((wd[0] * wd[0] + wd[1] * wd[1]) + wd[2] * wd[2]);
      const float lat = std::asin(wd[2] / n);
      const float ex = (float)((-lon / M_PI + 1) / 2 * ew), ey = (float)((-lat / M_PI + 0.5) * eh);
      const int ix = std::min(std::max((int)ex, 0), ew - 1), iy = std::min(std::max((int)ey, 0), eh - 1);
      fetch[2 * ((size_t)y * w + x)] = iy;
      fetch[2 * ((size_t)y * w + x) + 1] = ix;
    }
  }
}

// SimpleMeshWindow::generate (SimpleMeshRenderer.cpp:407-418) on the device image img (w x h)
int smr_generate(derp_ctx* c, const derp_render_params& p, float4* img, int w, int h, int outW, int outH, bool back,
                 bool equi, int ew, int eh) {
  SmrState& S = *c->smr;
  const size_t n = (size_t)w * h;
  const dim3 g(blocks_of(n, 256)), b(256);
  if (back) {
    if (w != outW || h != outH) {  // alphaBlend's CHECK_EQ(fore.rows, back.rows) / cols
      return fail(c, "--background is %dx%d but the image it is blended with is %dx%d", outW, outH, w, h);
    }
    hipLaunchKernelGGL(k_smr_alpha_blend, g, b, 0, c->stream, img, S.back.as<float4>(), n);
  }
  if (equi) {
    std::vector<int> fetch;
    smr_fetch_table(p, w, h, ew, eh, fetch);
    ALLOC(c, S.fetch, fetch.size() * sizeof(int));
    HIPCHK(c, hipMemcpyAsync(S.fetch.p, fetch.data(), fetch.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_smr_background_equirect, g, b, 0, c->stream, img, S.fetch.as<int>(), n, S.equi.as<float4>(), ew);
    HIPCHK(c, hipStreamSynchronize(c->stream));  // `fetch` goes out of scope
  }
  KCHECK(c);
  return 0;
}

int smr_check(derp_ctx* c, const derp_render_params* p) {
  if (!c || !p) {
    return fail(c, "bad arguments");
  }
  if (!c->smr) {
    return fail(c, "derp_render_upload has not been called");
  }
  if (p->kind < DERP_RENDER_CUBE || p->kind > DERP_RENDER_SNAPSHOT || p->height < 1 || p->height > 16384 ||
      (p->kind == DERP_RENDER_SNAPSHOT && (p->width < 1 || p->width > 32768))) {
    return fail(c, "bad render kind / size");
  }
  return hipSetDevice(c->device) == hipSuccess ? 0 : fail(c, "hipSetDevice failed");
}

void smr_out_size(const derp_render_params& p, int& w, int& h) {
  w = p.kind == DERP_RENDER_SNAPSHOT ? p.width : p.kind == DERP_RENDER_CUBE ? p.height : 2 * p.height;
  h = p.kind == DERP_RENDER_CUBE ? 6 * p.height : p.height;
}

// SimpleMeshRenderer's --format list (SimpleMeshRenderer.cpp:66-77): what each renders and how it is stacked
enum SmrFormat { kCubeColor, kCubeDisp, kEqrColor, kEqrDisp, kLr180, kSnapColor, kSnapDisp, kTb3dof, kTbStereo };
int smr_format(const char* f) {
  static const char* names[] = {"cubecolor", "cubedisp", "eqrcolor", "eqrdisp", "lr180", "snapcolor", "snapdisp", "tb3dof", "tbstereo"};
  for (int i = 0; f && i < 9; ++i) {
    if (std::strcmp(f, names[i]) == 0) {
      return i;
    }
  }
  return -1;
}

}  // namespace

// ---- SimpleMeshRenderer (include/derp_hip.h derp_render_*) ----
void derp_render_params_default(derp_render_params* p) {
  if (!p) {
    return;
  }
  std::memset(p, 0, sizeof *p);
  p->kind = DERP_RENDER_EQUIRECT;
  p->width = 3072;
  p->height = 1536;
  p->forward[0] = -1.0;  // SimpleMeshRenderer.cpp:97-110 defaults
  p->up[2] = 1.0;
  p->horizontal_fov = 90.0;
  p->alpha_blend = 1;
  p->weight = DERP_WEIGHT_SVD;
}

int derp_render_upload(derp_ctx* c, const float* const* colors_bgra, const int* color_w, const int* color_h,
                       const float* const* disparities, const int* disp_w, const int* disp_h) {
  if (!c || !disparities || !disp_w || !disp_h || (colors_bgra && (!color_w || !color_h))) {
    return fail(c, "bad arguments");
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->smr = std::make_unique<SmrState>();
  SmrState& S = *c->smr;
  S.cams.resize(c->S);
  S.haveColor = colors_bgra != nullptr;
  for (int s = 0; s < c->S; ++s) {
    SmrCam& k = S.cams[s];
    k.dw = disp_w[s];
    k.dh = disp_h[s];
    k.tw = S.haveColor ? color_w[s] : 0;
    k.th = S.haveColor ? color_h[s] : 0;
    if (!disparities[s] || k.dw < 2 || k.dh < 2 || (size_t)k.dw * k.dh * 2 > (1ull << 31) ||
        (S.haveColor && (!colors_bgra[s] || k.tw < 1 || k.th < 1))) {
      return fail(c, "bad disparity / colour for camera %d", s);
    }
    size_t nd = (size_t)k.dw * k.dh, texD = 0, texC = 0;
    if (!smr_mips(k.dw, k.dh, k.Md, texD) || (S.haveColor && !smr_mips(k.tw, k.th, k.Mc, texC))) {
      return fail(c, "image too large for the mip chain (camera %d)", s);
    }
    ALLOC(c, k.vert, nd * 16);
    ALLOC(c, k.texDisp, texD * 16);
    ALLOC(c, S.staging, std::max(nd * 4, (size_t)k.tw * k.th * 16));
    HIPCHK(c, hipMemcpy(S.staging.p, disparities[s], nd * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_smr_mesh, grid2d(k.dw, k.dh, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), s,
                       S.staging.as<float>(), k.dw, k.dh, k.vert.as<float4>());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (S.haveColor) {
      ALLOC(c, k.texColor, texC * 16);
      HIPCHK(c, hipMemcpy(S.staging.p, colors_bgra[s], (size_t)k.tw * k.th * 16, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_smr_texture, grid2d(k.tw, k.th, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), s,
                         S.staging.as<float4>(), (const float4*)nullptr, 0.f, 0.f, 0.f, k.tw, k.th, k.texColor.as<float4>());
      smr_build_mips(c, k.texColor.as<float4>(), k.Mc);
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  return 0;
}

int derp_render(derp_ctx* c, const derp_render_params* p, const uint8_t* include, float* out_bgra) {
  TRY(smr_check(c, p));
  if (!out_bgra) {
    return fail(c, "bad arguments");
  }
  int w, h;
  smr_out_size(*p, w, h);
  const size_t n = (size_t)w * h;
  SmrState& S = *c->smr;
  ALLOC(c, S.img, n * 16);
  TRY(smr_image(c, *p, include, S.img.as<float4>()));
  return download_sync(c, out_bgra, S.img.p, n * 16);
}

int derp_render_vertices(derp_ctx* c, int cam, float ipd, float* out_xyzw) {
  if (!c || !out_xyzw || !c->smr || cam < 0 || cam >= (int)c->smr->cams.size()) {
    return fail(c, "bad arguments (or derp_render_upload has not been called)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  derp_render_params p;
  derp_render_params_default(&p);
  p.ipd = ipd;
  TRY(smr_prepare(c, p, {cam}));
  SmrCam& k = c->smr->cams[cam];
  return download_sync(c, out_xyzw, (ipd != 0.0f ? k.eyeVert : k.vert).p, (size_t)k.dw * k.dh * 16);
}

int derp_render_format_size(const char* format, int width, int height, int* out_w, int* out_h) {
  const int f = smr_format(format);
  if (f < 0 || !out_w || !out_h) {
    return 1;
  }
  const bool stacked = f == kTb3dof || f == kTbStereo;
  *out_w = (f == kSnapColor || f == kSnapDisp) ? width : (f == kCubeColor || f == kCubeDisp) ? height : 2 * height;
  *out_h = (f == kCubeColor || f == kCubeDisp) ? 6 * height : stacked ? 2 * height : height;
  return 0;
}

int derp_render_format(derp_ctx* c, const char* format, const derp_render_params* pin, const float* background,
                       const float* background_equirect, int eq_w, int eq_h, float* out_bgra) {
  const int f = smr_format(format);
  if (f < 0) {
    return fail(c, "Invalid format: %s", format ? format : "(null)");
  }
  TRY(smr_check(c, pin));
  if (!out_bgra || (background_equirect && (eq_w < 1 || eq_h < 1))) {
    return fail(c, "bad arguments");
  }
  SmrState& S = *c->smr;
  derp_render_params p = *pin;
  int W, H;
  derp_render_format_size(format, p.width, p.height, &W, &H);
  const size_t n = (size_t)W * H;
  ALLOC(c, S.img, n * 16);
  if (background) {
    ALLOC(c, S.back, n * 16);
    HIPCHK(c, hipMemcpy(S.back.p, background, n * 16, hipMemcpyHostToDevice));
  }
  if (background_equirect) {
    ALLOC(c, S.equi, (size_t)eq_w * eq_h * 16);
    HIPCHK(c, hipMemcpy(S.equi.p, background_equirect, (size_t)eq_w * eq_h * 16, hipMemcpyHostToDevice));
  }
  auto generate = [&](float4* img, int w, int h) {
    return smr_generate(c, p, img, w, h, W, H, background != nullptr, background_equirect != nullptr, eq_w, eq_h);
  };
  p.disparity_color = f == kCubeDisp || f == kEqrDisp || f == kSnapDisp;
  p.kind = (f == kCubeColor || f == kCubeDisp) ? DERP_RENDER_CUBE
           : (f == kSnapColor || f == kSnapDisp) ? DERP_RENDER_SNAPSHOT : DERP_RENDER_EQUIRECT;
  if (f == kLr180 || f == kTb3dof || f == kTbStereo) {
    // stereo(): the two eyes at +-0.032 m, tb3dof(): colour and disparity colour at ipd 0; each eye generate()d,
    // then stacked (SimpleMeshRenderer.cpp:420-451)
    const int ew = 2 * p.height, eh = p.height;
    const size_t ne = (size_t)ew * eh;
    ALLOC(c, S.img2, ne * 16);
    for (int e = 0; e < 2; ++e) {
      p.ipd = f == kTb3dof ? 0.0f : (e == 0 ? 0.032f : -0.032f);
      p.disparity_color = f == kTb3dof && e == 1;
      TRY(smr_image(c, p, nullptr, S.img2.as<float4>()));
      TRY(generate(S.img2.as<float4>(), ew, eh));
      if (f == kLr180) {  // cv::Rect(cols / 4, 0, cols / 2, rows) of each eye, side by side
        HIPCHK(c, hipMemcpy2DAsync(S.img.as<float4>() + (size_t)e * (ew / 2), (size_t)W * 16, S.img2.as<float4>() + ew / 4,
                                   (size_t)ew * 16, (size_t)(ew / 2) * 16, eh, hipMemcpyDeviceToDevice, c->stream));
      } else {
        HIPCHK(c, hipMemcpyAsync(S.img.as<float4>() + (size_t)e * ne, S.img2.p, ne * 16, hipMemcpyDeviceToDevice, c->stream));
      }
    }
  } else {
    p.ipd = 0.0f;
    TRY(smr_image(c, p, nullptr, S.img.as<float4>()));
  }
  TRY(generate(S.img.as<float4>(), W, H));
  return download_sync(c, out_bgra, S.img.p, n * 16);
}
