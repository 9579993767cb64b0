// RigSimulator on the GPU (source/rig/RigSimulator.cpp): one ray per supersampled pixel. Three kernels — the rays of a
// rig camera (fp64 camera model of derp_camera.h, narrowed to float), the rays of a mono / stereo equirect, and the
// trace (sphere tree, ceiling, sky, marble, Lambert) — then the aas x aas INTER_AREA downscale with the area-resize
// kernels of derp_kernels.h. The fp32 arithmetic lives in derp_sim_math.h, shared with the host scene unit; this file
// is included at the end of derp_capi.hip and uses its DevBuf, launch helpers and error slot.
#pragma once
#include "derp_sim_math.h"

extern "C" void derp_sim_perlin_table(uint8_t* p512);

namespace {

using derp_sim_math::V3f;

constexpr int kSimBlock = 256;
constexpr int kSimOutside = -3, kSimCeiling = -2, kSimSky = -1;

struct SimScene {
  const derp_sim_triangle* tris;
  const derp_sim_node* nodes;
  const int32_t* leaf;
  const uint8_t* perm;     // Perlin's permutation, 512 entries
  const uint8_t* sky;      // [skyH][skyW][3] BGR
  const uint8_t* ceiling;  // [ceilH][ceilW][3] BGR or null
  int nNodes, skyW, skyH, ceilW, ceilH, marble;
  double ceilingPosition, ceilingWidth, ceilingDepth, marbleScale;
};

// renderCamera's ray, RigSimulator.cpp:606-616: pixel ((x + 0.5f) / aas, (y + 0.5f) / aas) in float, widened;
// Camera::isOutsideImageCircle (Camera.h:166-178); Camera::rig(pixel) (Camera.h:131-138) in fp64, narrowed to float.
__global__ __launch_bounds__(kSimBlock) void k_sim_camera_rays(Cam cam, ScaledCam sc, int W, int H, int aas,
                                                               float* __restrict__ origin, float* __restrict__ dir,
                                                               int* __restrict__ hit) {
  const size_t n = (size_t)W * H, i = (size_t)blockIdx.x * kSimBlock + threadIdx.x;
  if (i >= n) {
    return;
  }
  const int x = (int)(i % W), y = (int)(i / W);
  const double px = (double)((x + 0.5f) / (float)aas), py = (double)((y + 0.5f) / (float)aas);
  V3f o = {0, 0, 0}, d = {0, 0, 0};
  int flag = kSimSky;
  if (outside_image_circle(cam, px, py, sc.prx, sc.pry, sc.fx, sc.fy)) {
    flag = kSimOutside;
  } else {
    const D3 r = rig_direction(cam, px, py, sc.prx, sc.pry, sc.fx, sc.fy);
    o = {(float)cam.pos[0], (float)cam.pos[1], (float)cam.pos[2]};
    d = {(float)r.x, (float)r.y, (float)r.z};
  }
  origin[3 * i] = o.x;
  origin[3 * i + 1] = o.y;
  origin[3 * i + 2] = o.z;
  dir[3 * i] = d.x;
  dir[3 * i + 1] = d.y;
  dir[3 * i + 2] = d.z;
  hit[i] = flag;
}

// renderMonoEquirect / renderStereoEquirect's rays, RigSimulator.cpp:533-540, 562-576. theta and phi are floats there;
// M_PI makes the products double, and the unqualified sin / cos are taken as the double functions.
__global__ __launch_bounds__(kSimBlock) void k_sim_equirect_rays(int W, int H, int stereo, double ipr,
                                                                 float* __restrict__ originL, float* __restrict__ originR,
                                                                 float* __restrict__ dir, int* __restrict__ hitL,
                                                                 int* __restrict__ hitR) {
  const size_t n = (size_t)W * H, i = (size_t)blockIdx.x * kSimBlock + threadIdx.x;
  if (i >= n) {
    return;
  }
  const int x = (int)(i % W), y = (int)(i / W);
  const float theta = (float)((double)2.0f * M_PI * (double)(1.0f - (x + 0.5f) / float(W)));
  const float phi = (float)(M_PI * (double)(y + 0.5f) / (double)float(H));
  const double sp = sin((double)phi), cp = cos((double)phi), st = sin((double)theta), ct = cos((double)theta);
  dir[3 * i] = (float)(sp * ct);
  dir[3 * i + 1] = (float)(sp * st);
  dir[3 * i + 2] = (float)cp;
  V3f l = {0, 0, 0}, r = {0, 0, 0};
  if (stereo) {
    const double a = (double)theta + M_PI / (double)2.0f, b = (double)theta - M_PI / (double)2.0f;
    l = {(float)((double)(float)cos(a) * ipr), (float)((double)(float)sin(a) * ipr), (float)((double)0.0f * ipr)};
    r = {(float)((double)(float)cos(b) * ipr), (float)((double)(float)sin(b) * ipr), (float)((double)0.0f * ipr)};
    originR[3 * i] = r.x;
    originR[3 * i + 1] = r.y;
    originR[3 * i + 2] = r.z;
    hitR[i] = kSimSky;
  }
  originL[3 * i] = l.x;
  originL[3 * i + 1] = l.y;
  originL[3 * i + 2] = l.z;
  hitL[i] = kSimSky;
}

// traceRayToGetColor, RigSimulator.cpp:196-262, for every ray whose flag is not "outside the image circle". colour is
// written x 255 as the callers store it (:542, :583, :618); aux is the depth (cameras) or the inverse depth clamped to
// 0..1 (mono equirect, :543).
__global__ __launch_bounds__(kSimBlock) void k_sim_trace(SimScene S, const float* __restrict__ origin,
                                                         const float* __restrict__ dir, size_t n, int invDepth,
                                                         int* __restrict__ hit, float* __restrict__ dist,
                                                         float* __restrict__ color, float* __restrict__ aux) {
  using namespace derp_sim_math;
  const size_t i = (size_t)blockIdx.x * kSimBlock + threadIdx.x;
  if (i >= n) {
    return;
  }
  V3f c = {0, 0, 0};
  float depth = FLT_MAX;
  int flag = hit[i];
  if (flag != kSimOutside) {
    const V3f o = f3(origin + 3 * i), d = f3(dir + 3 * i);
    float best;
    flag = trace_tree(o, d, S.nodes, S.nNodes, S.leaf, S.tris, best);
    bool done = false;
    if (S.ceiling) {  // :205-220
      const float cd = (float)((S.ceilingPosition - (double)o.z) / (double)d.z);
      if (0 < cd && cd < best) {
        const V3f p = add(o, scale(d, cd));
        const float s = (float)((double)p.x / S.ceilingWidth + 0.5), t = (float)((double)p.y / S.ceilingDepth + 0.5);
        if (0 <= s && s < 1 && 0 <= t && t < 1) {
          // (float products that round up to rows / cols read past the image in the reference; clamped here)
          const int row = min((int)(t * S.ceilH), S.ceilH - 1), col = min((int)(s * S.ceilW), S.ceilW - 1);
          const uint8_t* q = S.ceiling + ((size_t)row * S.ceilW + col) * 3;
          c = {(float)q[0] / 255.0f, (float)q[1] / 255.0f, (float)q[2] / 255.0f};
          depth = cd;
          flag = kSimCeiling;
          done = true;
        }
      }
    }
    if (!done && flag < 0) {  // :223-237, acos / atan2 taken as the double functions
      const float dz = d.z < -1.0f ? -1.0f : d.z > 1.0f ? 1.0f : d.z;
      const float phi = (float)acos((double)dz);
      const float theta = (float)(M_PI + atan2((double)d.y, (double)d.x));
      const float sampleX = (float)(((double)theta / (2.0 * M_PI)) * (double)S.skyW);
      const float sampleY = (float)(((double)phi / M_PI) * (double)S.skyH);
      const int row = max(min((int)sampleY, S.skyH - 1), 0), col = max(min((int)sampleX % S.skyW, S.skyW - 1), 0);
      const uint8_t* q = S.sky + ((size_t)row * S.skyW + col) * 3;
      c = {(float)q[0] / 255.0f, (float)q[1] / 255.0f, (float)q[2] / 255.0f};
      flag = kSimSky;
    } else if (!done) {
      c = shade_hit(o, d, best, S.tris[flag], S.marble != 0, S.marbleScale, S.perm);
      depth = best;
    }
  }
  hit[i] = flag;
  dist[i] = depth;
  color[3 * i] = 255.0f * c.x;
  color[3 * i + 1] = 255.0f * c.y;
  color[3 * i + 2] = 255.0f * c.z;
  if (invDepth) {
    const float v = 1.0f / depth;
    aux[i] = v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v;
  } else {
    aux[i] = depth;
  }
}

}  // namespace

struct derp_sim {
  int device = 0;
  hipStream_t stream = nullptr;
  bool haveScene = false;
  SimScene scene{};
  DevBuf tris, nodes, leaf, perm, sky, ceiling;
  // supersampled planes of the last render; index 1 = the right eye of a stereo equirect
  DevBuf origin[2], dir, hit[2], dist[2], color[2], aux[2], small3[2], small1;
  int W = 0, H = 0, eyes = 0;
  std::string* errSink() const {  // every derp_sim_* call reports through derp_last_error(nullptr)
    return &g_create_error;
  }
};

namespace {

constexpr size_t kSimMaxRays = (size_t)1 << 28;  // rays of one render: 3 floats each stay far below 2^32 bytes per plane

int sim_alloc(derp_sim* s, int W, int H, int eyes) {
  const size_t n = (size_t)W * H;
  if (s->dir.ensure(n * 12)) {
    return create_fail("out of device memory");
  }
  for (int e = 0; e < eyes; ++e) {
    if (s->origin[e].ensure(n * 12) || s->hit[e].ensure(n * 4) || s->dist[e].ensure(n * 4) || s->color[e].ensure(n * 12) ||
        s->aux[e].ensure(n * 4)) {
      return create_fail("out of device memory");
    }
  }
  s->W = W;
  s->H = H;
  s->eyes = eyes;
  return 0;
}

int sim_trace(derp_sim* s, int eye, int invDepth) {
  const size_t n = (size_t)s->W * s->H;
  k_sim_trace<<<blocks_of(n, kSimBlock), kSimBlock, 0, s->stream>>>(s->scene, s->origin[eye].as<float>(), s->dir.as<float>(), n,
                                                                    invDepth, s->hit[eye].as<int>(), s->dist[eye].as<float>(),
                                                                    s->color[eye].as<float>(), s->aux[eye].as<float>());
  KCHECK(s);
  return 0;
}

// downscale(), RigSimulator.cpp:510-517: cv::resize INTER_AREA by the integer factor aas on both axes (k_resize_area's
// integer-factor path; a copy at aas 1). Sums of FLT_MAX sky depths overflow to +inf there as they do in cv::resize.
int sim_downscale(derp_sim* s, int kind, const DevBuf& src, int w, int h, int aas, DevBuf& dst, float* out) {
  const size_t bytes = (size_t)w * h * (kind == 3 ? 12 : 4);
  if (dst.ensure(bytes)) {
    return create_fail("out of device memory");
  }
  const AreaAxis ax{nullptr, nullptr, nullptr, aas};
  const dim3 g = grid2d(w, h, 1, kBlk2d);
  if (kind == 3) {
    hipLaunchKernelGGL(k_resize_area<3>, g, kBlk2d, 0, s->stream, (const void*)src.p, w * aas, h * aas, dst.p, w, h, ax, ax, -1);
  } else {
    hipLaunchKernelGGL(k_resize_area<2>, g, kBlk2d, 0, s->stream, (const void*)src.p, w * aas, h * aas, dst.p, w, h, ax, ax, -1);
  }
  KCHECK(s);
  HIPCHK(s, hipMemcpyAsync(out, dst.p, bytes, hipMemcpyDeviceToHost, s->stream));
  return 0;
}

int sim_check_render(derp_sim* s, int w, int h, int aas) {
  if (!s->haveScene) {
    return create_fail("derp_sim: no scene was uploaded");
  }
  if (w <= 0 || h <= 0 || aas < 1 || aas > 64 || (size_t)w * aas * h * aas > kSimMaxRays) {
    return create_fail("derp_sim: bad image size or anti_alias_supersample (at most 2^28 rays per image)");
  }
  return 0;
}

}  // namespace

int derp_sim_create(derp_sim** out, int device) {
  if (!out) {
    return 1;
  }
  *out = nullptr;
  hipDeviceProp_t prop;
  TRY(open_device(device, "the simulator's tracer", &prop));
  std::unique_ptr<derp_sim> owner(new derp_sim);
  derp_sim* s = owner.get();
  s->device = device;
  uint8_t perm[512];
  derp_sim_perlin_table(perm);
  if (s->perm.ensure(sizeof perm)) {
    return create_fail("out of device memory");
  }
  HIPCHK(s, hipMemcpy(s->perm.p, perm, sizeof perm, hipMemcpyHostToDevice));
  HIPCHK(s, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  *out = owner.release();
  return 0;
}

void derp_sim_destroy(derp_sim* s) {
  if (!s) {
    return;
  }
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->stream);
  (void)hipStreamDestroy(s->stream);
  delete s;
}

int derp_sim_upload(derp_sim* s, const derp_sim_triangle* triangles, int n_triangles, const derp_sim_node* nodes, int n_nodes,
                    const int32_t* leaf_indices, int n_leaf_indices, const uint8_t* skybox_bgr, int sky_w, int sky_h,
                    const uint8_t* ceiling_bgr, int ceiling_w, int ceiling_h, const derp_sim_params* params) {
  if (!s || !nodes || n_nodes < 1 || n_triangles < 0 || n_leaf_indices < 0 || (n_triangles > 0 && !triangles) ||
      (n_leaf_indices > 0 && !leaf_indices) || !skybox_bgr || sky_w <= 0 || sky_h <= 0 || !params ||
      (ceiling_bgr && (ceiling_w <= 0 || ceiling_h <= 0))) {
    return create_fail("derp_sim_upload: bad arguments");
  }
  // the walk trusts the tree: every link must move forward and every leaf must stay inside the lists
  for (int i = 0; i < n_nodes; ++i) {
    const derp_sim_node& nd = nodes[i];
    if (nd.skip <= i || nd.skip > n_nodes || nd.count < -1 ||
        (nd.count > 0 && (nd.first < 0 || (int64_t)nd.first + nd.count > n_leaf_indices))) {
      return create_fail("derp_sim_upload: node " + std::to_string(i) + " has a bad skip link or leaf range");
    }
  }
  for (int i = 0; i < n_leaf_indices; ++i) {
    if (leaf_indices[i] < 0 || leaf_indices[i] >= n_triangles) {
      return create_fail("derp_sim_upload: leaf index out of range");
    }
  }
  HIPCHK(s, hipSetDevice(s->device));
  s->haveScene = false;
  const size_t tb = std::max<size_t>(1, n_triangles) * sizeof(derp_sim_triangle), nb = (size_t)n_nodes * sizeof(derp_sim_node),
               lb = std::max<size_t>(1, n_leaf_indices) * 4, sb = (size_t)sky_w * sky_h * 3,
               cb = ceiling_bgr ? (size_t)ceiling_w * ceiling_h * 3 : 0;
  HIPCHK(s, hipStreamSynchronize(s->stream));
  if (s->tris.ensure(tb) || s->nodes.ensure(nb) || s->leaf.ensure(lb) || s->sky.ensure(sb) || (cb && s->ceiling.ensure(cb))) {
    return create_fail("out of device memory");
  }
  if (n_triangles > 0) {
    HIPCHK(s, hipMemcpy(s->tris.p, triangles, (size_t)n_triangles * sizeof(derp_sim_triangle), hipMemcpyHostToDevice));
  }
  HIPCHK(s, hipMemcpy(s->nodes.p, nodes, nb, hipMemcpyHostToDevice));
  if (n_leaf_indices > 0) {
    HIPCHK(s, hipMemcpy(s->leaf.p, leaf_indices, (size_t)n_leaf_indices * 4, hipMemcpyHostToDevice));
  }
  HIPCHK(s, hipMemcpy(s->sky.p, skybox_bgr, sb, hipMemcpyHostToDevice));
  if (cb) {
    HIPCHK(s, hipMemcpy(s->ceiling.p, ceiling_bgr, cb, hipMemcpyHostToDevice));
  }
  SimScene& S = s->scene;
  S.tris = s->tris.as<derp_sim_triangle>();
  S.nodes = s->nodes.as<derp_sim_node>();
  S.leaf = s->leaf.as<int32_t>();
  S.perm = s->perm.as<uint8_t>();
  S.sky = s->sky.as<uint8_t>();
  S.ceiling = cb ? s->ceiling.as<uint8_t>() : nullptr;
  S.nNodes = n_nodes;
  S.skyW = sky_w;
  S.skyH = sky_h;
  S.ceilW = ceiling_w;
  S.ceilH = ceiling_h;
  S.marble = params->marble;
  S.ceilingPosition = params->ceiling_position;
  S.ceilingWidth = params->ceiling_width;
  S.ceilingDepth = params->ceiling_depth;
  S.marbleScale = params->marble_scale;
  s->haveScene = true;
  return 0;
}

int derp_sim_render_camera(derp_sim* s, const derp_camera_desc* cam, int aas, float* bgr_out, float* depth_out) {
  if (!s || !cam || !bgr_out || !depth_out) {
    return create_fail("derp_sim_render_camera: bad arguments");
  }
  const int w = (int)cam->resolution[0], h = (int)cam->resolution[1];
  TRY(sim_check_render(s, w, h, aas));
  Cam c;
  if (const char* why = host_prepare_camera(*cam, c)) {
    return create_fail(std::string("camera ") + cam->id + ": " + why);
  }
  HIPCHK(s, hipSetDevice(s->device));
  TRY(sim_alloc(s, w * aas, h * aas, 1));
  const size_t n = (size_t)s->W * s->H;
  // the camera as the rig file holds it, in pixels: Camera::rescale to its own resolution changes nothing
  k_sim_camera_rays<<<blocks_of(n, kSimBlock), kSimBlock, 0, s->stream>>>(c, scaled_cam(*cam, w, h), s->W, s->H, aas,
                                                                          s->origin[0].as<float>(), s->dir.as<float>(),
                                                                          s->hit[0].as<int>());
  KCHECK(s);
  TRY(sim_trace(s, 0, 0));
  TRY(sim_downscale(s, 3, s->color[0], w, h, aas, s->small3[0], bgr_out));
  TRY(sim_downscale(s, 2, s->aux[0], w, h, aas, s->small1, depth_out));
  HIPCHK(s, hipStreamSynchronize(s->stream));
  return 0;
}

int derp_sim_render_equirect(derp_sim* s, int w, int h, int aas, int stereo, double interpupillary_radius, float* bgr_a,
                             float* bgr_b, float* aux_out) {
  if (!s || !bgr_a || (stereo ? !bgr_b : !aux_out)) {
    return create_fail("derp_sim_render_equirect: bad arguments");
  }
  TRY(sim_check_render(s, w, h, aas));
  HIPCHK(s, hipSetDevice(s->device));
  TRY(sim_alloc(s, w * aas, h * aas, stereo ? 2 : 1));
  const size_t n = (size_t)s->W * s->H;
  k_sim_equirect_rays<<<blocks_of(n, kSimBlock), kSimBlock, 0, s->stream>>>(
      s->W, s->H, stereo ? 1 : 0, interpupillary_radius, s->origin[0].as<float>(), s->origin[1].as<float>(), s->dir.as<float>(),
      s->hit[0].as<int>(), s->hit[1].as<int>());
  KCHECK(s);
  TRY(sim_trace(s, 0, 1));
  TRY(sim_downscale(s, 3, s->color[0], w, h, aas, s->small3[0], bgr_a));
  if (stereo) {
    TRY(sim_trace(s, 1, 1));
    TRY(sim_downscale(s, 3, s->color[1], w, h, aas, s->small3[1], bgr_b));
  } else {
    TRY(sim_downscale(s, 2, s->aux[0], w, h, aas, s->small1, aux_out));
  }
  HIPCHK(s, hipStreamSynchronize(s->stream));
  return 0;
}

int derp_sim_trace_rays(derp_sim* s, const float* rays6, size_t n) {
  if (!s || !rays6 || n == 0 || n > (size_t)INT32_MAX) {
    return create_fail("derp_sim_trace_rays: bad arguments");
  }
  TRY(sim_check_render(s, (int)n, 1, 1));
  HIPCHK(s, hipSetDevice(s->device));
  TRY(sim_alloc(s, (int)n, 1, 1));
  std::vector<float> o(3 * n), d(3 * n);
  for (size_t i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) {
      o[3 * i + k] = rays6[6 * i + k];
      d[3 * i + k] = rays6[6 * i + 3 + k];
    }
  }
  HIPCHK(s, hipMemcpyAsync(s->origin[0].p, o.data(), n * 12, hipMemcpyHostToDevice, s->stream));
  HIPCHK(s, hipMemcpyAsync(s->dir.p, d.data(), n * 12, hipMemcpyHostToDevice, s->stream));
  HIPCHK(s, hipMemsetAsync(s->hit[0].p, 0xff, n * 4, s->stream));  // -1: not outside
  TRY(sim_trace(s, 0, 0));
  HIPCHK(s, hipStreamSynchronize(s->stream));  // (the host vectors go out of scope)
  return 0;
}

int derp_sim_stage_size(const derp_sim* s, int* width, int* height) {
  if (!s || !width || !height) {
    return create_fail("derp_sim_stage_size: bad arguments");
  }
  *width = s->W;
  *height = s->H;
  return 0;
}

int derp_sim_stage(derp_sim* s, int stage, int eye, void* out) {
  if (!s || !out) {
    return create_fail("derp_sim_stage: bad arguments");
  }
  if (s->eyes == 0 || eye < 0 || eye >= s->eyes) {
    return create_fail("derp_sim_stage: nothing was rendered yet for this eye");
  }
  const size_t n = (size_t)s->W * s->H;
  const void* src = nullptr;
  size_t bytes = n * 4;
  switch (stage) {
    case DERP_SIM_STAGE_ORIGIN: src = s->origin[eye].p, bytes = n * 12; break;
    case DERP_SIM_STAGE_DIRECTION: src = s->dir.p, bytes = n * 12; break;
    case DERP_SIM_STAGE_HIT: src = s->hit[eye].p; break;
    case DERP_SIM_STAGE_DISTANCE: src = s->dist[eye].p; break;
    case DERP_SIM_STAGE_COLOR: src = s->color[eye].p, bytes = n * 12; break;
    default: return create_fail("derp_sim_stage: no such stage " + std::to_string(stage));
  }
  HIPCHK(s, hipSetDevice(s->device));
  HIPCHK(s, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
  return 0;
}
