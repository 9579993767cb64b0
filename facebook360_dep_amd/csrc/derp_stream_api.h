// MeshStreamRenderer, host side: the uploaded camera meshes, the direction tables, the views and passes, the
// derp_stream_* entry points (which include/derp_hip.h declares extern "C"). Kernels: derp_stream.h. The views are
// SimpleMeshRenderer's (derp_render_api.h: smr_snapshot_view, smr_face_view). Included by derp_capi.hip after it.
#pragma once

namespace {

struct StreamCam {
  bool uploaded = false;
  size_t nVert = 0, nTri = 0;
  int w = 0, h = 0;
  float focalR = 0.0f;
  DevBuf vtx, idx, tex, dirTab;
};
struct StreamState {
  std::vector<StreamCam> cams;
  DevBuf srgb, staging, clip, texVar, zbuf, acc, big, nBig, cube, img, tabs;
};

// sRGB -> linear of GL_SRGB8_ALPHA8 per code, in fp64, rounded once
void stream_srgb_table(float* out) {
  for (int i = 0; i < 256; ++i) {
    const double s = i / 255.0;
    out[i] = (float)(s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4));
  }
}

// transform = projection * view of V in rig space: eye = R p + t with t = -R c; clip.xy = k * eye.xy, clip.w = -eye.z,
// clip.z = clip.w - 2 near (a far plane at infinity, so that z >= -w is the near plane)
StreamView stream_transform(const SmrView& V) {
  StreamView T;
  float t[3];
  for (int r = 0; r < 3; ++r) {
    t[r] = -((V.R[r][0] * V.c[0] + V.R[r][1] * V.c[1]) + V.R[r][2] * V.c[2]);
  }
  for (int k = 0; k < 4; ++k) {
    const float r0 = k < 3 ? V.R[0][k] : t[0], r1 = k < 3 ? V.R[1][k] : t[1], r2 = k < 3 ? V.R[2][k] : t[2];
    T.m[0][k] = V.kx * r0;
    T.m[1][k] = V.ky * r1;
    T.m[2][k] = -r2;
    T.m[3][k] = -r2;
  }
  T.m[2][3] = T.m[2][3] - 2.0f * kStreamNear;
  T.W = V.W;
  T.H = V.H;
  return T;
}

int stream_vertex_stage(derp_ctx* c, int cam, const StreamView& T) {
  StreamState& S = *c->meshStream;
  const StreamCam& k = S.cams[cam];
  ALLOC(c, S.clip, std::max<size_t>(k.nVert, 1) * 16);
  ALLOC(c, S.texVar, std::max<size_t>(k.nVert, 1) * 8);
  if (k.nVert == 0) {
    return 0;
  }
  const Cam& cm = c->camsDstH[cam];
  hipLaunchKernelGGL(k_stream_vertex, dim3(blocks_of(k.nVert, 256)), dim3(256), 0, c->stream, k.vtx.as<float>(),
                     (unsigned)k.nVert, 1.0f / (float)k.w, 1.0f / (float)k.h, k.focalR, k.dirTab.as<float4>(),
                     (float)cm.pos[0], (float)cm.pos[1], (float)cm.pos[2], T, S.clip.as<float4>(), S.texVar.as<float2>());
  return 0;
}

// RigScene::render in view V: the cameras in rig order, each into its own depth buffer, then accumulated; resolved
int stream_view(derp_ctx* c, const SmrView& V, const std::vector<int>& cams, float fade, int zeroNans, int flip, float4* out) {
  StreamState& S = *c->meshStream;
  const StreamView T = stream_transform(V);
  const size_t nf = (size_t)V.W * V.H;
  ALLOC(c, S.zbuf, nf * 8);
  ALLOC(c, S.acc, nf * 16);
  ALLOC(c, S.nBig, sizeof(unsigned));
  (void)hipMemsetAsync(S.acc.p, 0, nf * 16, c->stream);
  for (int s : cams) {
    const StreamCam& k = S.cams[s];
    if (k.nTri == 0) {
      continue;
    }
    ALLOC(c, S.big, k.nTri * sizeof(uint4));
    TRY(stream_vertex_stage(c, s, T));
    (void)hipMemsetAsync(S.zbuf.p, 0, nf * 8, c->stream);
    (void)hipMemsetAsync(S.nBig.p, 0, sizeof(unsigned), c->stream);
    hipLaunchKernelGGL(k_stream_raster, dim3(blocks_of(k.nTri, 256)), dim3(256), 0, c->stream, S.clip.as<float4>(),
                       S.texVar.as<float2>(), k.idx.as<unsigned>(), (unsigned)k.nTri, V.W, V.H,
                       S.zbuf.as<unsigned long long>(), S.big.as<uint4>(), S.nBig.as<unsigned>());
    hipLaunchKernelGGL(k_stream_raster_big, dim3(1024, kStreamBigSplit), dim3(256), 0, c->stream, S.clip.as<float4>(),
                       S.texVar.as<float2>(), k.idx.as<unsigned>(), V.W, V.H, S.zbuf.as<unsigned long long>(),
                       S.big.as<uint4>(), S.nBig.as<unsigned>());
    hipLaunchKernelGGL(k_stream_resolve, grid2d(V.W, V.H, 1, kBlk2d), kBlk2d, 0, c->stream, S.clip.as<float4>(),
                       S.texVar.as<float2>(), k.idx.as<unsigned>(), k.tex.as<float4>(), k.w, k.h, V.W, V.H,
                       S.zbuf.as<unsigned long long>(), S.acc.as<float4>());
  }
  hipLaunchKernelGGL(k_stream_finish, grid2d(V.W, V.H, 1, kBlk2d), kBlk2d, 0, c->stream, S.acc.as<float4>(), V.W, V.H, fade,
                     zeroNans, flip, out);
  KCHECK(c);
  return 0;
}

int stream_check(derp_ctx* c, const derp_render_params* p) {
  if (!c || !p) {
    return fail(c, "bad arguments");
  }
  if (!c->meshStream) {
    return fail(c, "derp_stream_upload has not been called");
  }
  if (p->kind < DERP_RENDER_CUBE || p->kind > DERP_RENDER_SNAPSHOT || p->height < 1 || p->height > 16384 ||
      (p->kind == DERP_RENDER_SNAPSHOT && (p->width < 1 || p->width > 32768))) {
    return fail(c, "bad render kind / size");
  }
  if (p->ipd != 0.0f || p->disparity_color) {
    return fail(c, "the mesh stream renders mono colour only: ipd and disparity_color must be 0");
  }
  return hipSetDevice(c->device) == hipSuccess ? 0 : fail(c, "hipSetDevice failed");
}

SmrView stream_smr_view(const derp_render_params& p, int face) {
  return p.kind == DERP_RENDER_SNAPSHOT ? smr_snapshot_view(p) : smr_face_view(p, face, p.height);
}

}  // namespace

// ---- MeshStreamRenderer (include/derp_hip.h derp_stream_*) ----
void derp_stream_srgb_table(float* out256) {
  if (out256) {
    stream_srgb_table(out256);
  }
}

int derp_stream_upload(derp_ctx* c, int cam, const float* vtx, size_t vertices, const uint32_t* idx, size_t indices,
                       const uint8_t* rgba, int w, int h) {
  if (!c) {
    return 1;
  }
  TRY(check_camera(c, cam));
  // everything is refused here, on the host, before a byte reaches the device
  if (indices % 3 != 0) {
    return fail(c, "derp_stream_upload: %zu indices are not a multiple of 3 (camera %d)", indices, cam);
  }
  if ((vertices > 0 && !vtx) || (indices > 0 && !idx) || !rgba) {
    return fail(c, "derp_stream_upload: null pointer with a non-zero count (camera %d)", cam);
  }
  if (vertices > 0xffffffffull || indices / 3 >= 0xffffffffull) {
    return fail(c, "derp_stream_upload: the mesh of camera %d is too large (32-bit vertex and triangle indices)", cam);
  }
  const derp_camera_desc& desc = c->descDstH[cam];
  if (w < 1 || h < 1 || (double)w != desc.resolution[0] || (double)h != desc.resolution[1]) {
    return fail(c, "derp_stream_upload: the colour of camera %d is %dx%d but the camera's resolution is %gx%g", cam, w, h,
                desc.resolution[0], desc.resolution[1]);
  }
  if (desc.focal[0] != -desc.focal[1]) {  // Camera::getScalarFocal's CHECK
    return fail(c, "derp_stream_upload: the pixels of camera %d are not square", cam);
  }
  for (size_t i = 0; i < indices; ++i) {  // the guard that keeps a corrupt file from reading outside the vertex buffer
    if (idx[i] >= vertices) {
      return fail(c, "derp_stream_upload: index %u at position %zu is not below the vertex count %zu (camera %d)", idx[i], i,
                  vertices, cam);
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->meshStream) {
    c->meshStream = std::make_unique<StreamState>();
    c->meshStream->cams.resize(c->D);
  }
  StreamState& S = *c->meshStream;
  if (!S.srgb.p) {
    float tab[256];
    stream_srgb_table(tab);
    TRY(upload_sync(c, S.srgb, tab, sizeof tab));
  }
  StreamCam& k = S.cams[cam];
  k.uploaded = false;
  k.nVert = k.nTri = 0;
  if (vertices > 0) {
    TRY(upload_sync(c, k.vtx, vtx, vertices * 12));
  }
  if (indices > 0) {
    TRY(upload_sync(c, k.idx, idx, indices * 4));
  }
  const size_t n = (size_t)w * h;
  TRY(upload_sync(c, S.staging, rgba, n * 4));
  ALLOC(c, k.tex, n * 16);
  hipLaunchKernelGGL(k_stream_texture, dim3(blocks_of(n, 256)), dim3(256), 0, c->stream, S.staging.as<uchar4>(),
                     S.srgb.as<float>(), n, k.tex.as<float4>());
  KCHECK(c);
  // RigScene::createDirection: pixel = c * resolution / (kDirections - 1), camera.rig(pixel).direction() cast to float
  const ScaledCam sc = scaled_cam(desc, w, h);
  std::vector<float> dirs((size_t)kStreamDirections * kStreamDirections * 4);
  for (int y = 0; y < kStreamDirections; ++y) {
    for (int x = 0; x < kStreamDirections; ++x) {
      const D3 d = rig_direction(c->camsDstH[cam], x * sc.resx / (kStreamDirections - 1), y * sc.resy / (kStreamDirections - 1),
                                 sc.prx, sc.pry, sc.fx, sc.fy);
      float* o = &dirs[((size_t)y * kStreamDirections + x) * 4];
      o[0] = (float)d.x;
      o[1] = (float)d.y;
      o[2] = (float)d.z;
      o[3] = 0.0f;
    }
  }
  TRY(upload_sync(c, k.dirTab, dirs.data(), dirs.size() * 4));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging buffer is free again
  k.focalR = (float)sc.fx;  // getScalarFocal() * kR, kR = 1
  k.w = w;
  k.h = h;
  k.nVert = vertices;
  k.nTri = indices / 3;
  k.uploaded = true;
  return 0;
}

int derp_stream_clear(derp_ctx* c) {
  TRY(use_device(c));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->meshStream.reset();
  return 0;
}

int derp_stream_render(derp_ctx* c, const derp_render_params* p, const uint8_t* include, float fade, float* out_bgra) {
  TRY(stream_check(c, p));
  if (!out_bgra) {
    return fail(c, "bad arguments");
  }
  StreamState& S = *c->meshStream;
  std::vector<int> cams;
  for (int s = 0; s < (int)S.cams.size(); ++s) {
    if (S.cams[s].uploaded && (!include || include[s])) {
      cams.push_back(s);
    }
  }
  int w, h;
  smr_out_size(*p, w, h);
  const size_t n = (size_t)w * h;
  const int E = p->height, zn = p->zero_nans ? 1 : 0;
  ALLOC(c, S.img, n * 16);
  float4* img = S.img.as<float4>();
  if (p->kind == DERP_RENDER_SNAPSHOT) {
    TRY(stream_view(c, stream_smr_view(*p, 0), cams, fade, zn, 1, img));
  } else if (p->kind == DERP_RENDER_CUBE) {
    for (int face = 0; face < 6; ++face) {
      TRY(stream_view(c, stream_smr_view(*p, face), cams, fade, zn, 1, img + (size_t)face * E * E));
    }
  } else {
    ALLOC(c, S.cube, (size_t)6 * E * E * 16);
    for (int face = 0; face < 6; ++face) {  // the cube texture keeps GL rows
      TRY(stream_view(c, stream_smr_view(*p, face), cams, fade, zn, 0, S.cube.as<float4>() + (size_t)face * E * E));
    }
    TRY(smr_cube_to_equirect(c, S.cube.as<float4>(), E, S.tabs, img));
  }
  return download_sync(c, out_bgra, S.img.p, n * 16);
}

int derp_stream_vertices(derp_ctx* c, int cam, const derp_render_params* p, int face, float* out_clip_xyzw) {
  TRY(stream_check(c, p));
  TRY(check_camera(c, cam));
  if (!out_clip_xyzw || face < 0 || face > 5 || !c->meshStream->cams[cam].uploaded) {
    return fail(c, "bad arguments (or derp_stream_upload has not been called for camera %d)", cam);
  }
  TRY(stream_vertex_stage(c, cam, stream_transform(stream_smr_view(*p, face))));
  KCHECK(c);
  const size_t nVert = c->meshStream->cams[cam].nVert;
  if (nVert == 0) {
    return 0;
  }
  return download_sync(c, out_clip_xyzw, c->meshStream->clip.p, nVert * 16);
}
