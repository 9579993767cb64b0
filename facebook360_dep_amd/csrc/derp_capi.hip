// C-ABI implementation of include/derp_hip.h: context, HBM-resident pyramid, level driver.
// Host side mirrors the reference's DerpCLI level loop (DerpCLI.cpp:220-323) and processLevel
// (Derp.cpp:1005-1034). No CPU compute path: every stage is a kernel in derp_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/derp_hip.h"
#include "derp_kernels.h"
#include "derp_mesh.h"
#include "derp_points.h"
#include "derp_render.h"

using namespace derp;

namespace {

enum Stage {
  ST_FOV = 0,
  ST_VARIANCE,
  ST_OWN_BIAS,
  ST_UPSAMPLE,
  ST_PROJ_WARP,
  ST_REPROJECT,
  ST_PROJ_BIAS,
  ST_BRUTE,
  ST_RANDOM,
  ST_PINGPONG,
  ST_MISMATCH,
  ST_BILATERAL,
  ST_MEDIAN,
  ST_MASKFOV,
  ST_TEMPORAL,
  ST_LANES,  // wall of a level whose frames ran on overlapping work lanes (their per-stage spans overlap in time)
  ST_COUNT
};
const char* kStageNames[ST_COUNT] = {"fov_mask",  "variance",    "own_bias",         "upsample",  "proj_warp",
                                     "reproject", "proj_bias",   "brute_force",      "random_proposals",
                                     "ping_pong", "mismatches",  "bilateral",        "median",    "mask_fov",
                                     "temporal",  "lanes_wall"};
constexpr int kMaxLevels = 24;

// A device allocation and its owner: move-only, freed when the owner dies
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() {
    release();
  }
  // grow-only; the contents are lost on growth; non-zero (and an empty buffer) when the allocation fails
  int ensure(size_t n) {
    if (n <= bytes) {
      return 0;
    }
    release();
    if (hipMalloc(&p, n) != hipSuccess) {
      p = nullptr;
      return 1;
    }
    bytes = n;
    return 0;
  }
  void release() {
    if (p) {
      (void)hipFree(p);
    }
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

struct TimedSpan {
  int stage, level;
  hipEvent_t a, b;
};

struct LanczosTab {
  DevBuf ofs, coef;
};

struct AreaTabDev {  // computeResizeAreaTab of one axis, resident in HBM
  DevBuf start, si, alpha;
  int iscale = 0;
};

// Everything processLevel writes per frame. The context has one and every work lane has one; the rig-only tables of a
// level (projWarp, projWarpInv, rayDir, behind, resampling tables) are shared by the lanes and stay on the context.
struct WorkSet {
  DevBuf srcVar, ownBias, fovMask, maskAnd, disparity, cost, confidence, dispRes, costRes, changed, tmpF, rank, mismatchMask, pairCount;
  DevBuf tileSeen;    // k_reproject_bias: per (table, tile) whether any map position is valid
  DevBuf projColor, projBias;
  DevBuf projColorT;  // projColor again in 4x4-texel tiles: the random-proposal kernel's copy (DERP_RANDOM_TILED)
  DevBuf bruteCost, bruteConf, lanczosTmp, staging, stagingB;
  int colorTablesCleanLevel = -1;  // level whose colour / bias tables were written in full since its warps were built
};

// HBM-resident pyramid of one frame, per level: colour, fg masks, background disparity, result
struct FramePyramid {
  std::vector<DevBuf> color, fg, bg, disp;
  std::vector<char> haveBg, haveDisp;
};

struct WorkLane {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  WorkSet w;
};

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

// derp_mesh_*: one camera's mesh (derp_mesh.h). The grid-sized buffers stay for the next camera; the compacted mesh
// (V, F) and what the set-up gathers through (qmask, qoff, vorig) describe the mesh built last.
struct MeshState {
  DevBuf disparity, mask, tabs, vert, valid, qmask, used, blockFaces, blockVerts, offF, offV, totals, vmap, vorig, qoff, V, F;
  DevBuf planes, costs, vq;
  int W = 0, H = 0;
  size_t nv = 0, nf = 0, nfUnmasked = 0;
  bool built = false;
  // derp_mesh_simplify's / derp_mesh_simplify_parallel's result (host): what the downloads return once one has run
  bool simplified = false;
  std::vector<double> sV;
  std::vector<int32_t> sF;
  // derp_mesh_simplify_parallel's state besides V, F, planes, costs and vq, which it works on in place
  DevBuf alive, boundary, vcount, vstart, vcursor, adj, keys, keysFeasible, keysSorted, vals, valsSorted, claim, wins, blockSum, blockOff,
      counters, sortTemp, outV, outF;
  std::vector<derp_mesh_pass> passes;  // of the last derp_mesh_simplify_parallel (derp_mesh_parallel_pass)
};

}  // namespace

struct derp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copyStream = nullptr;  // input uploads of a frame that is not being computed (sequence driver), with
  DevBuf copyStaging;                // their own staging buffer: they overlap the compute of the frame before
  DevBuf cnVert, cnRgba, cnZ, cnAcc, cnOut, cnBig, cnNBig;  // derp_canopy_cubemap's buffers, kept between calls
  std::unique_ptr<SmrState> smr;                            // derp_render_*'s scene (derp_render_upload)
  std::unique_ptr<MeshState> mesh;                          // derp_mesh_*'s camera mesh (derp_mesh_build)
  std::string err;
  derp_options opt;
  int S = 0, D = 0;
  std::vector<Cam> camsSrcH, camsDstH;
  std::vector<int> dst2srcH;
  std::vector<derp_camera_desc> descDstH;  // the destinations as the rig file holds them (un-normalised: derp_points_* etc.)
  DevBuf camsSrc, camsDst, dst2src;

  int numLevels = 0, widthFull = 0, heightFull = 0;
  std::vector<int> LW, LH;
  // one pyramid per frame slot (derp_set_frame_slots / derp_select_frame: several frames of one sequence resident on
  // this GPU); the level loop works on the selected one
  std::vector<FramePyramid> frames;
  int curSlot = 0;
  FramePyramid& frame() {
    return frames[curSlot];
  }
  int xcdRotate = 1;

  // working level
  int cur = -1;
  int DB = 0;  // dst batch that fits the table budget
  WorkSet w;             // the per-frame working set in use: the context's own, or a lane's while its frame runs
  DevBuf temporalCarry;  // accumulators of a temporal window longer than one launch holds
  DevBuf projWarp, projWarpInv;
  DevBuf rayDir, behind;  // per destination pixel: ray direction [3][D][n] f64, sources facing away [D][n] (k_pixel_rays)
  int warpCachedLevel = -1;
  bool randomRanThisLevel = false;  // cost / confidence hold random-proposal results for this level
  bool tablesValid = false;
  DevBuf counters;  // [ST_COUNT][kMaxLevels][4] u64
  std::map<std::pair<int, int>, LanczosTab> lanczos;  // (map nodes keep their addresses: get_lanczos / get_area_tab
  std::map<std::pair<int, int>, AreaTabDev> areaTabs;  // hand out pointers into them)
  DevBuf fullFrame;
  DevBuf devMask;  // derp_dev_mask result (not a working buffer)
  DevBuf rephotoColor, rephotoDisp;  // derp_rephotograph_upload: S planes of BGR u16 / f32 disparity
  int rephotoW = 0, rephotoH = 0;
  DevBuf spiral;
  int spiralN = 0, spiralRadius = -1;
  // derp_points_begin .. derp_points_download: every camera's disparity image in one buffer, and the chunk in flight
  DevBuf pointsDisp, pointsImages, pointsXyz;
  std::vector<PointsImage> pointsImagesH;

  // Work lanes (round 6): a second, third ... working set + stream for processLevel of ANOTHER frame of a sequence at the
  // same coarse level (derp_seq_level_compute). The frames of a level are independent, and at the coarse levels one
  // frame's kernels fill a fraction of the chip (level 6 of the 16-camera rig: 784 waves for 4096 wave slots) and are
  // bound by their own serial latency — on lanes the frames' kernels overlap. A lane holds everything processLevel writes
  // per frame (a WorkSet); the rig-only tables of the level (projWarp, projWarpInv, rayDir, behind, resampling tables) stay
  // shared.
  std::vector<std::unique_ptr<WorkLane>> lanes;
  hipEvent_t laneReady = nullptr;  // recorded on the main stream behind what the lanes' frames depend on
  int activeLane = -1;             // the lane whose work set is swapped in (-1: the context's own)

  bool profiling = false;
  bool noMemo = false;  // DERP_NO_MEMO (developer switch), read once in derp_create
  // ping-pong's candidate loop: compacted into full waves of (pixel, candidate) tasks, or one pixel per lane
  // (DERP_PP_COMPACT=0, developer A/B switch; same results), read once in derp_create
  bool ppCompact = true;
  // waves per SIMD of the random-proposal / ping-pong kernels (0 = what their registers and LDS allow: four up to 16
  // cameras): a launch can ask for fewer by reserving more LDS per (one-wave) block — DERP_RANDOM_WAVES / DERP_PP_WAVES,
  // developer A/B switches
  int randomWaves = 0, ppWaves = 0;
  size_t ldsPerCu = 160 * 1024;  // hipDeviceProp.maxSharedMemoryPerMultiProcessor (derp_create)
  bool noTemporalTile = false;  // DERP_NO_TEMPORAL_TILE (developer A/B: the direct form of the temporal filter)
  bool noBlankSkip = false;     // DERP_NO_BLANK_SKIP (developer A/B: every frame rewrites the blank tiles of the colour tables)
  std::vector<TimedSpan> spans;
  double accMs[ST_COUNT][kMaxLevels];
  int accLaunch[ST_COUNT][kMaxLevels];
};

namespace {

int fail(derp_ctx* c, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) {
    c->err = buf;
  }
  return 1;
}

#define HIPCHK(c, expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      return fail(c, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #expr); \
    }                                                                                     \
  } while (0)
#define ALLOC(c, buf, n)                                                         \
  do {                                                                           \
    if ((buf).ensure(n)) {                                                       \
      return fail(c, "out of device memory allocating %zu bytes (%s)", (size_t)(n), #buf); \
    }                                                                            \
  } while (0)
#define KCHECK(c) HIPCHK(c, hipGetLastError())
#define TRY(expr)       \
  do {                  \
    int r_ = (expr);    \
    if (r_) {           \
      return r_;        \
    }                   \
  } while (0)

struct Span {
  derp_ctx* c;
  int stage, level;
  hipEvent_t a = nullptr, b = nullptr;
  Span(derp_ctx* ctx, int st, int lv) : c(ctx), stage(st), level(lv) {
    if (c->profiling) {
      (void)hipEventCreate(&a);
      (void)hipEventCreate(&b);
      (void)hipEventRecord(a, c->stream);
    }
  }
  ~Span() {
    if (c->profiling && a) {
      (void)hipEventRecord(b, c->stream);
      c->spans.push_back({stage, level, a, b});
    }
  }
};

void drain_spans(derp_ctx* c) {
  for (auto& s : c->spans) {
    (void)hipEventSynchronize(s.b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, s.a, s.b);
    if (s.level >= 0 && s.level < kMaxLevels) {
      c->accMs[s.stage][s.level] += ms;
      c->accLaunch[s.stage][s.level] += 1;
    }
    (void)hipEventDestroy(s.a);
    (void)hipEventDestroy(s.b);
  }
  c->spans.clear();
}

size_t npx(const derp_ctx* c, int level) {
  return (size_t)c->LW[level] * c->LH[level];
}

unsigned long long* counter_slot(derp_ctx* c, int stage, int level) {
  return c->counters.as<unsigned long long>() + ((size_t)stage * kMaxLevels + level) * 4;
}

LevelView make_view(derp_ctx* c, int stage, int dst0, int nd) {
  LevelView V;
  const int L = c->cur;
  V.W = c->LW[L];
  V.H = c->LH[L];
  V.Wd = (double)V.W;
  V.Hd = (double)V.H;
  V.S = c->S;
  V.D = nd;
  V.level = L;
  V.numLevels = c->numLevels;
  V.dst0 = dst0;
  V.hasFg = c->opt.use_foreground_masks;
  // PyramidLevel.h:232-236 — scale = float(width) / heightFullSize (reference quirk kept)
  const float scale = float(V.W) / c->heightFull;
  const float scaleVar = scale * scale;
  V.varNoiseFloor = std::max(c->opt.var_noise_floor * scaleVar, kMinVar);
  V.varHighThresh = c->opt.var_high_thresh;
  V.minDepthM = c->opt.min_depth_m;
  V.maxDepthM = c->opt.max_depth_m;
  V.randomProposals = c->opt.random_proposals;
  V.partialCoverage = c->opt.partial_coverage;
  V.xcdRotate = c->xcdRotate;
  V.camsSrc = c->camsSrc.as<Cam>();
  V.camsDst = c->camsDst.as<Cam>();
  V.dst2src = c->dst2src.as<int>();
  V.srcColor = c->frame().color[L].as<ushort4>();
  V.ownBias = c->w.ownBias.as<ushort4>();
  V.srcVar = c->w.srcVar.as<float>();
  V.srcFg = c->frame().fg[L].as<uint8_t>();
  V.rayDir = c->rayDir.as<double>();
  V.behind = c->behind.as<unsigned>();
  V.rayStride = (size_t)c->D * V.W * V.H;
  V.projWarp = c->projWarp.as<float2>();
  V.projColor = c->w.projColor.as<ushort4>();
  V.projBias = c->w.projBias.as<ushort4>();
  V.projColorT = c->w.projColorT.as<ushort4>();
  V.disparity = c->w.disparity.as<float>();
  V.cost = c->w.cost.as<float>();
  V.confidence = c->w.confidence.as<float>();
  V.bgDisp = c->frame().bg[L].as<float>();
  V.fovMask = c->w.fovMask.as<uint8_t>();
  V.pairCount = c->w.pairCount.as<uint8_t>();
  V.counters = counter_slot(c, stage, L);
  return V;
}

dim3 grid2d(int w, int h, int z, dim3 b) {
  return dim3((w + b.x - 1) / b.x, (h + b.y - 1) / b.y, z);
}
const dim3 kBlk2d(32, 8, 1);

// k_blur3_u16: 64 x 4 threads, each a column strip of kBlurRows rows
const dim3 kBlurBlk(64, 4, 1);
dim3 blur_grid(int ow, int oh, int planes) {
  return dim3((ow + 63) / 64, (oh + 4 * kBlurRows - 1) / (4 * kBlurRows), planes);
}

int flat_grid(size_t n) {
  return (int)std::min<size_t>((n + 255) / 256, 2048 * 4);
}

// ---- Lanczos4 tables: resize.cpp interpolateLanczos4 + offset computation (fp64 libm on host) ----
void lanczos_coeffs(float x, float* coeffs) {
  static const double s45 = 0.70710678118654752440084436210485;
  static const double cs[][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
  if (x < 1.1920928955078125e-07f) {
    for (int i = 0; i < 8; i++) {
      coeffs[i] = 0;
    }
    coeffs[3] = 1;
    return;
  }
  float sum = 0;
  const double y0 = -(x + 3) * M_PI * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
  for (int i = 0; i < 8; i++) {
    const double y = -(x + 3 - i) * M_PI * 0.25;
    coeffs[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
    sum += coeffs[i];
  }
  sum = 1.f / sum;
  for (int i = 0; i < 8; i++) {
    coeffs[i] *= sum;
  }
}

int get_lanczos(derp_ctx* c, int ssize, int dsize, LanczosTab** out) {
  auto key = std::make_pair(ssize, dsize);
  auto it = c->lanczos.find(key);
  if (it != c->lanczos.end()) {
    *out = &it->second;
    return 0;
  }
  std::vector<int> ofs(dsize);
  std::vector<float> coef((size_t)dsize * 8);
  const double scale = (double)ssize / dsize;
  for (int d = 0; d < dsize; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)f;
    s -= (s > f);  // cvFloor
    f -= s;
    ofs[d] = s;
    lanczos_coeffs(f, &coef[(size_t)d * 8]);
  }
  LanczosTab t;
  ALLOC(c, t.ofs, ofs.size() * sizeof(int));
  ALLOC(c, t.coef, coef.size() * sizeof(float));
  HIPCHK(c, hipMemcpyAsync(t.ofs.p, ofs.data(), ofs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(t.coef.p, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors go out of scope
  *out = &(c->lanczos[key] = std::move(t));
  return 0;
}

// cv::resize INTER_AREA, one axis: resize.cpp computeResizeAreaTab (fractional scales) or the integer
// scale factor of the "area fast" paths (|scale - round(scale)| < DBL_EPSILON)
int get_area_tab(derp_ctx* c, int ssize, int dsize, AreaTabDev** out, bool forceTable = false) {
  // cv::resize takes the integer-factor paths only when BOTH axes have integer factors; otherwise both
  // axes go through computeResizeAreaTab — forceTable builds the table of an integer-factor axis
  auto key = std::make_pair(forceTable ? -ssize : ssize, dsize);
  auto it = c->areaTabs.find(key);
  if (it != c->areaTabs.end()) {
    *out = &it->second;
    return 0;
  }
  AreaTabDev t;
  const double scale = (double)ssize / dsize;
  const int iscale = (int)std::nearbyint(scale);
  std::vector<int> start(dsize + 1, 0), si;
  std::vector<float> alpha;
  if (!forceTable && iscale >= 1 && std::abs(scale - iscale) < 2.220446049250313e-16) {
    t.iscale = iscale;
  } else {
    for (int dx = 0; dx < dsize; ++dx) {
      start[dx] = (int)si.size();
      const double fsx1 = dx * scale, fsx2 = fsx1 + scale;
      const double cellWidth = std::min(scale, ssize - fsx1);
      int sx1 = (int)std::ceil(fsx1), sx2 = (int)std::floor(fsx2);
      sx2 = std::min(sx2, ssize - 1);
      sx1 = std::min(sx1, sx2);
      if (sx1 - fsx1 > 1e-3) {
        si.push_back(sx1 - 1);
        alpha.push_back((float)((sx1 - fsx1) / cellWidth));
      }
      for (int sx = sx1; sx < sx2; ++sx) {
        si.push_back(sx);
        alpha.push_back(float(1.0 / cellWidth));
      }
      if (fsx2 - sx2 > 1e-3) {
        si.push_back(sx2);
        alpha.push_back((float)(std::min(std::min(fsx2 - sx2, 1.), cellWidth) / cellWidth));
      }
    }
    start[dsize] = (int)si.size();
  }
  if (si.empty()) {
    si.push_back(0);
    alpha.push_back(0.f);
  }
  ALLOC(c, t.start, start.size() * sizeof(int));
  ALLOC(c, t.si, si.size() * sizeof(int));
  ALLOC(c, t.alpha, alpha.size() * sizeof(float));
  HIPCHK(c, hipMemcpy(t.start.p, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(t.si.p, si.data(), si.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(t.alpha.p, alpha.data(), alpha.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = &(c->areaTabs[key] = std::move(t));
  return 0;
}

// cv2.resize(src, (dw, dh), INTER_AREA): kind 0 BGR u16 -> BGRX, 1 u8 (-> {0,1} when threshold >= 0), 2 f32
int resize_area_dev(derp_ctx* c, int kind, const void* src, int sw, int sh, void* dst, int dw, int dh, int threshold) {
  if (dw > sw || dh > sh) {
    // enlarging along an axis: cv::resize(INTER_AREA) turns into its bilinear emulation (float images only here)
    if (kind < 2) {
      return fail(c, "pyramid levels must not be larger than the full-size frame (%dx%d -> %dx%d)", sw, sh, dw, dh);
    }
    const dim3 g = grid2d(dw, dh, 1, kBlk2d);
    if (kind == 3) {
      hipLaunchKernelGGL(k_resize_linear_area_f32<3>, g, kBlk2d, 0, c->stream, (const float*)src, sw, sh, (float*)dst, dw, dh);
    } else {
      hipLaunchKernelGGL(k_resize_linear_area_f32<1>, g, kBlk2d, 0, c->stream, (const float*)src, sw, sh, (float*)dst, dw, dh);
    }
    KCHECK(c);
    return 0;
  }
  AreaTabDev *tx, *ty;
  TRY(get_area_tab(c, sw, dw, &tx));
  TRY(get_area_tab(c, sh, dh, &ty));
  if ((tx->iscale > 0) != (ty->iscale > 0)) {
    if (tx->iscale > 0) {
      TRY(get_area_tab(c, sw, dw, &tx, true));
    } else {
      TRY(get_area_tab(c, sh, dh, &ty, true));
    }
  }
  AreaAxis ax{tx->start.as<int>(), tx->si.as<int>(), tx->alpha.as<float>(), tx->iscale};
  AreaAxis ay{ty->start.as<int>(), ty->si.as<int>(), ty->alpha.as<float>(), ty->iscale};
  const dim3 g = grid2d(dw, dh, 1, kBlk2d);
  if (kind == 0) {
    hipLaunchKernelGGL(k_resize_area<0>, g, kBlk2d, 0, c->stream, src, sw, sh, dst, dw, dh, ax, ay, threshold);
  } else if (kind == 1) {
    hipLaunchKernelGGL(k_resize_area<1>, g, kBlk2d, 0, c->stream, src, sw, sh, dst, dw, dh, ax, ay, threshold);
  } else if (kind == 3) {
    hipLaunchKernelGGL(k_resize_area<3>, g, kBlk2d, 0, c->stream, src, sw, sh, dst, dw, dh, ax, ay, threshold);
  } else {
    hipLaunchKernelGGL(k_resize_area<2>, g, kBlk2d, 0, c->stream, src, sw, sh, dst, dw, dh, ax, ay, threshold);
  }
  KCHECK(c);
  return 0;
}

// UpsampleDisparityLib.cpp:27-54 — clockwise outward spiral of diameter w
std::vector<int2> make_spiral(int w) {
  int x = 0, y = 0, dx = 0, dy = -1, t = w;
  const int samples = t * t;
  std::vector<int2> locs;
  for (int i = 0; i < samples; ++i) {
    const bool vx = (-w / 2 <= x) && (x <= w / 2), vy = (-w / 2 <= y) && (y <= w / 2);
    if (vx && vy) {
      locs.push_back(make_int2(x, y));
    }
    if (x == y || ((x < 0) && (x == -y)) || ((x > 0) && (x == 1 - y))) {
      t = dx;
      dx = -dy;
      dy = t;
    }
    x += dx;
    y += dy;
  }
  return locs;
}

int ensure_spiral(derp_ctx* c, int radius) {
  if (c->spiralRadius == radius) {
    return 0;
  }
  const std::vector<int2> s = make_spiral(radius * 2 + 1);
  ALLOC(c, c->spiral, s.size() * sizeof(int2));
  HIPCHK(c, hipMemcpy(c->spiral.p, s.data(), s.size() * sizeof(int2), hipMemcpyHostToDevice));
  c->spiralN = (int)s.size();
  c->spiralRadius = radius;
  return 0;
}

// upsampleDisparityInPlace for `nd` planes living on the device (Lanczos path) or one plane (mask path)
int upsample_lanczos_dev(derp_ctx* c, const float* in, int sw, int sh, float* out, int dw, int dh, int planes,
                         size_t inStride, size_t outStride) {
  if (sw == dw && sh == dh) {  // cv::resize to the same size is a copy (after NaN -> 1e-4)
    return fail(c, "upsample to identical size not supported");
  }
  LanczosTab *tx, *ty;
  TRY(get_lanczos(c, sw, dw, &tx));
  TRY(get_lanczos(c, sh, dh, &ty));
  const size_t tmpStride = (size_t)dw * sh;
  ALLOC(c, c->w.lanczosTmp, tmpStride * planes * sizeof(float));
  hipLaunchKernelGGL(k_lanczos_h, grid2d(dw, sh, planes, kBlk2d), kBlk2d, 0, c->stream, in, sw, sh, dw,
                     tx->ofs.as<int>(), tx->coef.as<float>(), c->w.lanczosTmp.as<float>(), inStride, tmpStride);
  KCHECK(c);
  hipLaunchKernelGGL(k_lanczos_v, grid2d(dw, dh, planes, kBlk2d), kBlk2d, 0, c->stream, c->w.lanczosTmp.as<float>(), sh,
                     dw, dh, ty->ofs.as<int>(), ty->coef.as<float>(), out, tmpStride, outStride);
  KCHECK(c);
  return 0;
}

// `planes` images (destination cameras) in one launch: every pointer addresses `planes` contiguous planes
int upsample_masked_dev(derp_ctx* c, const float* in, const uint8_t* mask, int sw, int sh, const uint8_t* maskUp,
                        const float* bgUp, float* out, int dw, int dh, int planes = 1) {
  // getRadius (UpsampleDisparityLib.cpp:93-96): int(scale*scale + 1), float arithmetic
  const float scale = float(dw) / float(sw);
  const int radius = (int)(scale * scale + 1);
  TRY(ensure_spiral(c, radius));
  ALLOC(c, c->w.lanczosTmp, (size_t)dw * dh * planes * sizeof(float));
  hipLaunchKernelGGL(k_upsample_nearest_masked, grid2d(dw, dh, planes, kBlk2d), kBlk2d, 0, c->stream, in, mask, sw, sh,
                     maskUp, dw, dh, c->w.lanczosTmp.as<float>());
  KCHECK(c);
  hipLaunchKernelGGL(k_spiral_fill, grid2d(dw, dh, planes, kBlk2d), kBlk2d, 0, c->stream, c->w.lanczosTmp.as<float>(), bgUp,
                     maskUp, dw, dh, c->spiral.as<int2>(), c->spiralN, out);
  KCHECK(c);
  return 0;
}

// Stored inverse warps (projWarpInv) are needed only for sources that are not the own source of a destination of the
// same batch: everywhere else projWarpInv(d, s) is projWarp(ds, own(d)) (derp_kernels.h, batch_dst_of_source).
bool batch_needs_inverse_warps(const derp_ctx* c, int dst0, int nd) {
  std::vector<char> covered(c->S, 0);
  for (int d = dst0; d < dst0 + nd; ++d) {
    covered[c->dst2srcH[d]] = 1;
  }
  for (int s = 0; s < c->S; ++s) {
    if (!covered[s]) {
      return true;
    }
  }
  return false;
}

size_t table_bytes_per_dst(const derp_ctx* c, int W, int H, bool withInverse) {
  const size_t wp = (size_t)(W + 2 * kPadW) * (H + 2 * kPadW), cp = (size_t)(W + 2 * kPadC) * (H + 2 * kPadC);
  return (size_t)(c->S - 1) * (wp * sizeof(float2) + 2 * cp * sizeof(ushort4) + (withInverse ? (size_t)W * H * sizeof(float2) : 0) +
                               (DERP_RANDOM_TILED ? tiled_plane(W, H) * sizeof(ushort4) : 0));
}

int compute_fov_and_masks(derp_ctx* c, int level) {
  const int W = c->LW[level], H = c->LH[level];
  const size_t n = (size_t)W * H;
  {
    Span sp(c, ST_FOV, level);
    hipLaunchKernelGGL(k_fov_mask, grid2d(W, H, c->D, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>(), W, H,
                       c->w.fovMask.as<uint8_t>());
    KCHECK(c);
    hipLaunchKernelGGL(k_and_masks, dim3(flat_grid(n), c->D), dim3(256), 0, c->stream, c->w.fovMask.as<uint8_t>(),
                       c->frame().fg[level].as<uint8_t>(), c->dst2src.as<int>(), 0, n, c->w.maskAnd.as<uint8_t>());
    KCHECK(c);
  }
  return 0;
}

int build_warp(derp_ctx* c, int dst0, int nd) {
  const int L = c->cur;
  Span sp(c, ST_PROJ_WARP, L);
  {
    const size_t n = (size_t)c->LW[L] * c->LH[L];
    ALLOC(c, c->rayDir, 3 * n * c->D * sizeof(double));
    ALLOC(c, c->behind, n * c->D * sizeof(unsigned));
  }
  LevelView V = make_view(c, ST_PROJ_WARP, dst0, nd);
  hipLaunchKernelGGL(k_proj_warp, grid2d(V.W + 2 * kPadW, V.H + 2 * kPadW, c->S, kBlk2d), kBlk2d, 0, c->stream, V,
                     c->projWarp.as<float2>());
  KCHECK(c);
  // the destination pixels' ray directions and behind-the-camera source masks: rig + level size only, like the warps
  hipLaunchKernelGGL(k_pixel_rays, grid2d(V.W, V.H, nd, kBlk2d), kBlk2d, 0, c->stream, V, c->rayDir.as<double>(),
                     c->behind.as<unsigned>());
  KCHECK(c);
  c->w.colorTablesCleanLevel = -1;  // new warps (another level, batch or rig state): the colour tables must be rewritten in full
  // ... and the inverse warps reprojectColors reads (projWarpInv, PyramidLevel.h:46-51) — those that are not a
  // projWarp table of this batch already (all of them are when every source is a destination of the batch)
  if (batch_needs_inverse_warps(c, dst0, nd)) {
    hipLaunchKernelGGL(k_proj_warp_inv, grid2d(V.W, V.H, nd, kBlk2d), kBlk2d, 0, c->stream, V, c->projWarpInv.as<float2>());
    KCHECK(c);
  }
  return 0;
}

int build_color_tables(derp_ctx* c, int dst0, int nd) {
  const int L = c->cur;
  LevelView V = make_view(c, ST_REPROJECT, dst0, nd);
  // colours and their 3x3 biases in one pass (the bias stage's time is inside ST_REPROJECT now)
  Span sp(c, ST_REPROJECT, L);
  const dim3 grid((V.W + kRbTile - 1) / kRbTile, (V.H + kRbTile - 1) / kRbTile, nd * (c->S - 1));
  ALLOC(c, c->w.tileSeen, (size_t)grid.x * grid.y * grid.z);
  // a frame that finds the tables of this level as an earlier frame left them (same warps: a sequence running the
  // level frame after frame) skips the tiles no source pixel maps into — they still hold their zeros
  const int skipBlank = c->w.colorTablesCleanLevel == L && nd == c->D && !c->noBlankSkip;
  hipLaunchKernelGGL(k_reproject_bias, grid, dim3(256), 0, c->stream, V, c->projWarpInv.as<float2>(),
                     c->w.projColor.as<ushort4>(), c->w.projBias.as<ushort4>(), c->w.projColorT.as<ushort4>(),
                     c->w.tileSeen.as<uint8_t>(), skipBlank);
  KCHECK(c);
  c->w.colorTablesCleanLevel = nd == c->D ? L : -1;
  return 0;
}

// number of cost-kernel blocks covering a W x H image (16x16 super-tiles of four 8x8 wave tiles)
int tiles_of(int W, int H, int& tilesX) {
  constexpr int B = kTileBlock;  // tile grid padded to whole B x B squares
  tilesX = ((W + 15) / 16 + B - 1) / B * B;
  const int tilesY = ((H + 15) / 16 + B - 1) / B * B;
  return tilesX * tilesY * (256 / kCostBlock);
}
constexpr size_t kCostLdsPerSrc = (size_t)kCostBlock * sizeof(SsdPair);
int round8(int n) {
  return (n + 7) / 8 * 8;
}
// dynamic LDS of a one-wave block such that at most `waves` blocks per SIMD (4 x waves per CU) fit a CU's LDS
// (`ldsPerCu`: hipDeviceProp.maxSharedMemoryPerMultiProcessor, 160 KB on gfx950); `fixed` = the kernel's static LDS
size_t lds_for_waves(size_t needed, int waves, size_t ldsPerCu, size_t fixed) {
  if (waves <= 0 || waves >= 4) {
    return needed;
  }
  const size_t perBlock = ldsPerCu / (size_t)(4 * waves + 1) + 256;  // 4 * waves blocks fit, 4 * waves + 1 do not
  return std::max(needed, perBlock > fixed ? perBlock - fixed : needed);
}
constexpr size_t kCostLdsStatic = sizeof(PatchWin) * (kCostBlock / 64) + kAtanLutDoubles * sizeof(double);
// Which register budget of the two cost kernels to launch (k_ping_pong / k_random_proposals vs their _w3 twins): four waves
// per SIMD need sixteen one-wave blocks per CU, i.e. LDS for sixteen — true up to 16 cameras (9.3 KB each of 160 KB; measured
// 3.9 resident waves), not beyond (24 cameras: 13.3 KB, twelve blocks). DERP_COST_WAVES=3 / 4 forces one (developer A/B).
bool cost_four_waves(const derp_ctx* c) {
  if (const char* e = getenv("DERP_COST_WAVES")) {
    return atoi(e) >= 4;
  }
  return 16 * (kCostLdsPerSrc * (size_t)c->S + kCostLdsStatic) <= c->ldsPerCu && c->S <= 16;
}

int run_brute_force(derp_ctx* c, int dst0, int nd) {
  const int L = c->cur;
  if (L != c->numLevels - 1) {
    return 0;
  }
  Span sp(c, ST_BRUTE, L);
  LevelView V = make_view(c, ST_BRUTE, dst0, nd);
  const size_t n = (size_t)V.W * V.H;
  ALLOC(c, c->w.bruteCost, (size_t)nd * kNumDepths * n * sizeof(float));
  ALLOC(c, c->w.bruteConf, (size_t)nd * kNumDepths * n * sizeof(float));
  // 8 x 8 pixel strips over the interior (W - 2) x (H - 2) pixels, one wave each
  const int tilesX = std::max(1, (V.W - 2 + 7) / 8), tilesY = std::max(1, (V.H - 2 + 7) / 8);
  const int tiles = tilesX * tilesY;
  const size_t lds = kCostLdsPerSrc * (size_t)(c->S);
  hipLaunchKernelGGL(k_brute_costs, dim3(tiles, kNumDepths, nd), dim3(kCostBlock), lds, c->stream, V,
                     c->w.bruteCost.as<float>(), c->w.bruteConf.as<float>(), tilesX, tiles);
  KCHECK(c);
  hipLaunchKernelGGL(k_brute_select, grid2d(V.W, V.H, nd, kBlk2d), kBlk2d, 0, c->stream, V, c->w.bruteCost.as<float>(),
                     c->w.bruteConf.as<float>());
  KCHECK(c);
  hipLaunchKernelGGL(k_brute_margin, grid2d(V.W, V.H, nd, kBlk2d), kBlk2d, 0, c->stream, V);
  KCHECK(c);
  return 0;
}

int run_random_proposals(derp_ctx* c, int dst0, int nd) {
  const int L = c->cur;
  if (c->opt.random_proposals <= 0 || L == c->numLevels - 1) {
    return 0;
  }
  Span sp(c, ST_RANDOM, L);
  c->randomRanThisLevel = true;
  LevelView V = make_view(c, ST_RANDOM, dst0, nd);
  if (V.H > 2 && V.W > 2) {
    hipLaunchKernelGGL(k_row_rank, dim3(V.H - 2, nd), dim3(256), 0, c->stream, V, c->w.rank.as<int>());
    KCHECK(c);
  }
  int tilesX;
  const int tiles = tiles_of(V.W, V.H, tilesX);
  const size_t lds = lds_for_waves(kCostLdsPerSrc * (size_t)(c->S), c->randomWaves, c->ldsPerCu, kCostLdsStatic);
  hipLaunchKernelGGL(cost_four_waves(c) ? k_random_proposals : k_random_proposals_w3, dim3(round8(tiles), nd),
                     dim3(kCostBlock), lds, c->stream, V, c->w.rank.as<int>(), tilesX, tiles);
  KCHECK(c);
  return 0;
}

int run_ping_pong(derp_ctx* c, int dst0, int nd) {
  const int L = c->cur;
  if (L == c->numLevels - 1) {
    return 0;
  }
  Span sp(c, ST_PINGPONG, L);
  LevelView V = make_view(c, ST_PINGPONG, dst0, nd);
  const size_t n = (size_t)V.W * V.H;
  HIPCHK(c, hipMemsetAsync(c->w.changed.as<uint8_t>() + (size_t)dst0 * n, 1, n * nd, c->stream));
  int tilesX;
  const int tiles = tiles_of(V.W, V.H, tilesX);
  const size_t lds = lds_for_waves(kCostLdsPerSrc * (size_t)(c->S), c->ppWaves, c->ldsPerCu, kCostLdsStatic);
  const bool four = cost_four_waves(c);
  const auto kernel = c->ppCompact ? (four ? k_ping_pong : k_ping_pong_w3) : (four ? k_ping_pong_loop : k_ping_pong_loop_w3);
  for (int it = 1; it <= c->opt.ping_pong_iterations; ++it) {
    hipLaunchKernelGGL(kernel, dim3(round8(tiles), nd), dim3(kCostBlock), lds,
                       c->stream, V, c->w.changed.as<uint8_t>(), c->w.dispRes.as<float>(), c->w.costRes.as<float>(), tilesX,
                       (int)(it == 1 && c->randomRanThisLevel && !c->noMemo));
    KCHECK(c);
    hipLaunchKernelGGL(k_ping_pong_commit, dim3(flat_grid(n * nd)), dim3(256), 0, c->stream,
                       c->w.disparity.as<float>() + (size_t)dst0 * n, c->w.cost.as<float>() + (size_t)dst0 * n,
                       c->w.dispRes.as<float>() + (size_t)dst0 * n, c->w.costRes.as<float>() + (size_t)dst0 * n,
                       c->w.changed.as<uint8_t>() + (size_t)dst0 * n, n * nd);
    KCHECK(c);
  }
  // cost / confidence now belong to ping-pong's result (+inf where every candidate was rejected): the
  // memoised candidate must not be served from them by a later derp_stage_ping_pong call
  if (dst0 + nd >= c->D) {
    c->randomRanThisLevel = false;
  }
  return 0;
}

// handleDisparityMismatches (Derp.cpp:722-748): after every destination finished ping-pong
int run_mismatches(derp_ctx* c) {
  const int L = c->cur;
  if (L > c->opt.mismatches_start_level || L == c->numLevels - 1) {
    return 0;
  }
  if (c->D != c->S) {
    return fail(c, "Check failed: rigDst.size() == rigSrc.size()  Mismatches only valid when considering all cameras");
  }
  for (int d = 0; d < c->D; ++d) {
    if (c->dst2srcH[d] != d) {
      return fail(c, "mismatch handling needs destinations in rig order (dst %d maps to src %d)", d, c->dst2srcH[d]);
    }
  }
  Span sp(c, ST_MISMATCH, L);
  c->randomRanThisLevel = false;  // the working disparity changes: cost[] no longer matches it
  LevelView V = make_view(c, ST_MISMATCH, 0, c->D);
  const size_t n = (size_t)V.W * V.H;
  hipLaunchKernelGGL(k_mismatch, dim3((V.W + 15) / 16, (V.H + 15) / 16, c->D), dim3(256), 256 * sizeof(float) * c->S,
                     c->stream, V, c->w.dispRes.as<float>(), c->w.mismatchMask.as<uint8_t>());
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(c->w.disparity.p, c->w.dispRes.p, n * c->D * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int bilateral_radius(int level) {  // Derp.cpp:876-878
  const float scale = std::pow(0.9f, level);
  return (int)std::max(std::ceil(5 * scale), float(1));
}

size_t bilateral_lds_bytes(int radius) {
  // rows of the tile are padded to a multiple of 16 texels (k_joint_bilateral: bank-conflict-free float4 reads)
  const size_t t = (size_t)((16 + 2 * radius + 15) & ~15) * (16 + 2 * radius);
  return t * 4 * sizeof(float) + ((t + 3) & ~(size_t)3);
}

int run_bilateral(derp_ctx* c) {
  const int L = c->cur;
  Span sp(c, ST_BILATERAL, L);
  c->randomRanThisLevel = false;  // the working disparity changes: cost[] no longer matches it
  const int W = c->LW[L], H = c->LH[L];
  const size_t n = (size_t)W * H;
  // weights passed (B, G, R) = (0.5, 1, 1) — Derp.cpp:893-896, Derp.h:44-48; sigma 0.005
  const int radius = bilateral_radius(L);
  hipLaunchKernelGGL(k_joint_bilateral<true>, dim3((W + 15) / 16, (H + 15) / 16, c->D), dim3(256),
                     bilateral_lds_bytes(radius), c->stream, c->w.disparity.as<float>(),
                     (const void*)c->frame().color[L].as<ushort4>(), c->w.maskAnd.as<uint8_t>(), W, H, radius, 0.005f, 0.5f,
                     1.0f, 1.0f, c->w.tmpF.as<float>(), n, n, c->dst2src.as<int>());
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(c->w.disparity.p, c->w.tmpF.p, n * c->D * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int run_median(derp_ctx* c, bool fuseMaskFov) {
  const int L = c->cur;
  Span sp(c, ST_MEDIAN, L);
  c->randomRanThisLevel = false;  // the working disparity changes: cost[] no longer matches it
  const int W = c->LW[L], H = c->LH[L];
  const size_t n = (size_t)W * H;
  hipLaunchKernelGGL(k_masked_median, grid2d(W, H, c->D, kBlk2d), kBlk2d, 0, c->stream, c->w.disparity.as<float>(),
                     c->opt.use_foreground_masks ? c->frame().bg[L].as<float>() : (const float*)nullptr,
                     c->w.maskAnd.as<uint8_t>(), W, H, 1, c->w.tmpF.as<float>(), n,
                     fuseMaskFov ? c->w.fovMask.as<uint8_t>() : (const uint8_t*)nullptr);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(c->w.disparity.p, c->w.tmpF.p, n * c->D * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int run_mask_fov(derp_ctx* c) {
  const int L = c->cur;
  Span sp(c, ST_MASKFOV, L);
  const size_t n = npx(c, L) * c->D;
  hipLaunchKernelGGL(k_mask_fov, dim3(flat_grid(n)), dim3(256), 0, c->stream, c->w.disparity.as<float>(),
                     c->w.fovMask.as<uint8_t>(), n);
  KCHECK(c);
  return 0;
}

int check_level(derp_ctx* c, int level) {
  if (!c || c->numLevels == 0) {
    return fail(c, "derp_set_pyramid has not been called");
  }
  if (level < 0 || level >= c->numLevels) {
    return fail(c, "level %d out of range [0, %d)", level, c->numLevels);
  }
  if (c->LW[level] <= 0 || c->LH[level] <= 0) {
    return fail(c, "level %d was declared absent in derp_set_pyramid", level);
  }
  return 0;
}

// Level set-up: what DerpCLI does before processLevel (DerpCLI.cpp:221-303)
int level_begin(derp_ctx* c, int level, bool buildAllTables) {
  TRY(check_level(c, level));
  if (c->S - 1 > kMaxSrc) {
    return fail(c, "too many source cameras (%d > %d)", c->S, kMaxSrc + 1);
  }
  c->cur = level;
  const int W = c->LW[level], H = c->LH[level];
  const size_t n = (size_t)W * H;
  if (W < 3 || H < 3) {
    return fail(c, "level %d is too small (%dx%d)", level, W, H);
  }
  TRY(compute_fov_and_masks(c, level));
  {
    Span sp(c, ST_VARIANCE, level);
    hipLaunchKernelGGL(k_variance, grid2d(W, H, c->S, kBlk2d), kBlk2d, 0, c->stream, c->frame().color[level].as<ushort4>(),
                       W, H, c->w.srcVar.as<float>());
    KCHECK(c);
  }
  {
    Span sp(c, ST_OWN_BIAS, level);
    hipLaunchKernelGGL(k_blur3_u16, blur_grid(W, H, c->S), kBlurBlk, 0, c->stream,
                       c->frame().color[level].as<ushort4>(), 0, c->w.ownBias.as<ushort4>(), 0, W, H, n, n);
    KCHECK(c);
  }
  // fresh PyramidLevel: disparity / cost / confidence start at 0 (PyramidLevel.h:209-221)
  HIPCHK(c, hipMemsetAsync(c->w.cost.p, 0, n * c->D * sizeof(float), c->stream));
  HIPCHK(c, hipMemsetAsync(c->w.confidence.p, 0, n * c->D * sizeof(float), c->stream));
  HIPCHK(c, hipMemsetAsync(c->w.mismatchMask.p, 0, n * c->D, c->stream));
  if (level < c->numLevels - 1 && !c->frame().haveDisp[level + 1] && !buildAllTables) {
    return fail(c, "Missing disparity of level %d needed to start level %d", level + 1, level);
  }
  if (level < c->numLevels - 1 && c->frame().haveDisp[level + 1]) {
    Span sp(c, ST_UPSAMPLE, level);
    const int sw = c->LW[level + 1], sh = c->LH[level + 1];
    if (!c->opt.use_foreground_masks) {
      TRY(upsample_lanczos_dev(c, c->frame().disp[level + 1].as<float>(), sw, sh, c->w.disparity.as<float>(), W, H, c->D,
                               (size_t)sw * sh, n));
    } else {
      // masks = fov & fg at both sizes (UpsampleDisparityLib.cpp:163-179); coarse fov&fg recomputed into tmpF bytes
      ALLOC(c, c->w.staging, (size_t)sw * sh * c->D);
      hipLaunchKernelGGL(k_fov_mask, grid2d(sw, sh, c->D, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>(), sw, sh,
                         c->w.staging.as<uint8_t>());
      KCHECK(c);
      hipLaunchKernelGGL(k_and_masks, dim3(flat_grid((size_t)sw * sh), c->D), dim3(256), 0, c->stream,
                         c->w.staging.as<uint8_t>(), c->frame().fg[level + 1].as<uint8_t>(), c->dst2src.as<int>(), 0,
                         (size_t)sw * sh, c->w.staging.as<uint8_t>());
      KCHECK(c);
      TRY(upsample_masked_dev(c, c->frame().disp[level + 1].as<float>(), c->w.staging.as<uint8_t>(), sw, sh,
                              c->w.maskAnd.as<uint8_t>(), c->frame().bg[level].as<float>(), c->w.disparity.as<float>(), W, H, c->D));
    }
  } else {
    HIPCHK(c, hipMemsetAsync(c->w.disparity.p, 0, n * c->D * sizeof(float), c->stream));
  }
  // table budget -> dst batch. When the buffers already hold every destination's tables of this level (the
  // steady state of a sequence: same levels frame after frame) there is nothing to ask the runtime.
  // (the inverse-warp table only exists when a batch holds a source that is not one of its destinations)
  const bool invAll = batch_needs_inverse_warps(c, 0, c->D);
  size_t per = table_bytes_per_dst(c, W, H, invAll);
  int DB = c->D;
  bool needInv = invAll;
  {
    const size_t wpAll = (size_t)(W + 2 * kPadW) * (H + 2 * kPadW) * (c->S - 1) * c->D * sizeof(float2);
    const size_t cpAll = (size_t)(W + 2 * kPadC) * (H + 2 * kPadC) * (c->S - 1) * c->D * sizeof(ushort4);
    const size_t ipAll = (size_t)W * H * (c->S - 1) * c->D * sizeof(float2);
    const bool resident = c->projWarp.bytes >= wpAll && c->w.projColor.bytes >= cpAll && c->w.projBias.bytes >= cpAll &&
        (!invAll || c->projWarpInv.bytes >= ipAll) && !getenv("DERP_TABLE_BUDGET_GB") &&
        (!DERP_RANDOM_TILED || c->w.projColorT.bytes >= tiled_plane(W, H) * (c->S - 1) * c->D * sizeof(ushort4));
    if (!resident) {
      size_t freeB = 0, totalB = 0;
      HIPCHK(c, hipMemGetInfo(&freeB, &totalB));
      size_t budget = freeB + c->projWarp.bytes + c->w.projColor.bytes + c->w.projBias.bytes + c->projWarpInv.bytes + c->w.projColorT.bytes;
      if (const char* e = getenv("DERP_TABLE_BUDGET_GB")) {
        budget = std::min<size_t>(budget, (size_t)(atof(e) * (1ull << 30)));
      } else {
        budget = (size_t)(budget * 0.85);
      }
      DB = (int)std::min<size_t>((size_t)c->D, budget / std::max<size_t>(per, 1));
      if (DB < c->D && !needInv) {  // batches: the sources outside a batch need stored inverse warps
        needInv = true;
        per = table_bytes_per_dst(c, W, H, true);
        DB = (int)std::min<size_t>((size_t)c->D, budget / std::max<size_t>(per, 1));
      }
      if (DB < 1) {
        return fail(c, "projection tables for one destination (%zu bytes) exceed the table budget (%zu bytes)", per, budget);
      }
      // equal-sized batches: 24 destinations under a 23-destination budget run as 12 + 12, not 23 + 1
      const int batches = (c->D + DB - 1) / DB;
      DB = (c->D + batches - 1) / batches;
    }
  }
  c->DB = DB;
  const size_t wp = (size_t)(W + 2 * kPadW) * (H + 2 * kPadW), cp = (size_t)(W + 2 * kPadC) * (H + 2 * kPadC);
  ALLOC(c, c->projWarp, (size_t)DB * (c->S - 1) * wp * sizeof(float2));
  ALLOC(c, c->w.projColor, (size_t)DB * (c->S - 1) * cp * sizeof(ushort4));
  ALLOC(c, c->w.projBias, (size_t)DB * (c->S - 1) * cp * sizeof(ushort4));
  if (needInv) {
    ALLOC(c, c->projWarpInv, (size_t)DB * (c->S - 1) * n * sizeof(float2));
  }
  if (DERP_RANDOM_TILED) {
    ALLOC(c, c->w.projColorT, (size_t)DB * (c->S - 1) * tiled_plane(W, H) * sizeof(ushort4));
  }
  c->tablesValid = false;
  c->randomRanThisLevel = false;
  if (buildAllTables) {
    if (DB < c->D) {
      return fail(c, "stage-level API needs all destinations' tables resident (batch %d < %d)", DB, c->D);
    }
    if (c->opt.rebuild_warp_tables || c->warpCachedLevel != level) {
      TRY(build_warp(c, 0, c->D));
      c->warpCachedLevel = level;
    }
  }
  return 0;
}

int level_end(derp_ctx* c) {
  const int L = c->cur;
  HIPCHK(c, hipMemcpyAsync(c->frame().disp[L].p, c->w.disparity.p, npx(c, L) * c->D * sizeof(float),
                           hipMemcpyDeviceToDevice, c->stream));
  c->frame().haveDisp[L] = 1;
  return 0;
}

int process_level(derp_ctx* c, int level) {
  TRY(level_begin(c, level, false));
  const int L = level;
  for (int d0 = 0; d0 < c->D; d0 += c->DB) {
    const int nd = std::min(c->DB, c->D - d0);
    const bool single = (c->DB == c->D);
    if (!single || c->opt.rebuild_warp_tables || c->warpCachedLevel != L) {
      TRY(build_warp(c, d0, nd));
      c->warpCachedLevel = single ? L : -1;
    }
    TRY(build_color_tables(c, d0, nd));
    TRY(run_brute_force(c, d0, nd));
    TRY(run_random_proposals(c, d0, nd));
    TRY(run_ping_pong(c, d0, nd));
  }
  TRY(run_mismatches(c));
  if (c->opt.do_bilateral_filter) {
    TRY(run_bilateral(c));
  }
  if (c->opt.do_median_filter) {
    TRY(run_median(c, true));
  } else {
    TRY(run_mask_fov(c));
  }
  TRY(level_end(c));
  return 0;
}

int need_current(derp_ctx* c, bool tables) {
  if (!c || c->cur < 0) {
    return fail(c, "derp_level_begin has not been called");
  }
  if (tables && !c->tablesValid) {
    return fail(c, "derp_stage_reproject_colors must run before this stage");
  }
  return 0;
}

template <typename T>
int upload_tmp(derp_ctx* c, DevBuf& buf, const T* host, size_t count) {
  ALLOC(c, buf, count * sizeof(T));
  HIPCHK(c, hipMemcpyAsync(buf.p, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// The host-pointer entry points copy with plain hipMemcpy: the context's stream is non-blocking, so these null-stream
// copies do not order against it — a kernel's input is complete when the call returns, its output is read after a
// synchronise.
int upload_sync(derp_ctx* c, DevBuf& buf, const void* host, size_t bytes) {
  ALLOC(c, buf, bytes);
  HIPCHK(c, hipMemcpy(buf.p, host, bytes, hipMemcpyHostToDevice));
  return 0;
}
int download_sync(derp_ctx* c, void* host, const void* dev, size_t bytes) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// the buffers of one frame's pyramid at the context's geometry
int alloc_pyramid(derp_ctx* c, FramePyramid& f) {
  const int num_levels = c->numLevels;
  f.color.resize(num_levels);
  f.fg.resize(num_levels);
  f.bg.resize(num_levels);
  f.disp.resize(num_levels);
  f.haveBg.assign(num_levels, 0);
  f.haveDisp.assign(num_levels, 0);
  for (int l = 0; l < num_levels; ++l) {
    const size_t n = npx(c, l);
    if (n == 0) {
      continue;  // level not present / not needed by this run
    }
    ALLOC(c, f.color[l], n * c->S * sizeof(ushort4));
    ALLOC(c, f.fg[l], n * c->S);
    ALLOC(c, f.bg[l], n * c->D * sizeof(float));
    ALLOC(c, f.disp[l], n * c->D * sizeof(float));
    HIPCHK(c, hipMemsetAsync(f.fg[l].p, 1, n * c->S, c->stream));  // generateAllPassMasks
    HIPCHK(c, hipMemsetAsync(f.bg[l].p, 0, n * c->D * sizeof(float), c->stream));
  }
  return 0;
}

// the per-frame working buffers of a level of up to `n` pixels (the colour tables and scratch grow where they are used)
int alloc_work_set(derp_ctx* c, WorkSet& w, size_t n) {
  ALLOC(c, w.srcVar, n * c->S * sizeof(float));
  ALLOC(c, w.ownBias, n * c->S * sizeof(ushort4));
  ALLOC(c, w.fovMask, n * c->D);
  ALLOC(c, w.maskAnd, n * c->D);
  for (DevBuf* b : {&w.disparity, &w.cost, &w.confidence, &w.dispRes, &w.costRes, &w.tmpF, &w.rank}) {
    ALLOC(c, *b, n * c->D * sizeof(float));
  }
  ALLOC(c, w.changed, n * c->D);
  ALLOC(c, w.mismatchMask, n * c->D);
  ALLOC(c, w.pairCount, n * c->D);
  return 0;
}

// make `slot` the frame the level loop works on
int select_frame(derp_ctx* c, int slot) {
  if (slot < 0 || slot >= (int)c->frames.size()) {
    return fail(c, "frame slot %d out of range [0, %d)", slot, (int)c->frames.size());
  }
  if (slot != c->curSlot) {
    c->curSlot = slot;
    c->cur = -1;  // working buffers belong to the previously selected frame
  }
  return 0;
}

// exchange the context's per-frame working set (and stream) with lane `i`'s: applied twice it is the identity
void lane_swap(derp_ctx* c, int i) {
  std::swap(c->stream, c->lanes[i]->stream);
  std::swap(c->w, c->lanes[i]->w);
}

// lanes 0 .. count - 1 exist and hold working buffers for a level of `n` pixels
int lanes_prepare(derp_ctx* c, int count, size_t n) {
  while ((int)c->lanes.size() < count) {
    c->lanes.emplace_back(new WorkLane);
    WorkLane& l = *c->lanes.back();
    if (hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&l.done, hipEventDisableTiming) != hipSuccess) {
      return fail(c, "work lane: hipStreamCreate / hipEventCreate failed");
    }
  }
  if (!c->laneReady) {
    HIPCHK(c, hipEventCreateWithFlags(&c->laneReady, hipEventDisableTiming));
  }
  for (int i = 0; i < count; ++i) {
    TRY(alloc_work_set(c, c->lanes[i]->w, n));
  }
  return 0;
}

// processLevel of the frame in slot `slot` on lane `i` (i < 0: on the context's own working set and stream). The lane's
// stream first waits for c->laneReady.
int process_level_on_lane(derp_ctx* c, int i, int slot, int level) {
  if (i < 0) {
    TRY(select_frame(c, slot));
    return process_level(c, level);
  }
  HIPCHK(c, hipStreamWaitEvent(c->lanes[i]->stream, c->laneReady, 0));
  lane_swap(c, i);
  c->activeLane = i;
  int rc = select_frame(c, slot);
  if (!rc) {
    rc = process_level(c, level);
  }
  if (!rc && hipEventRecord(c->lanes[i]->done, c->stream) != hipSuccess) {
    rc = fail(c, "work lane: hipEventRecord failed");
  }
  lane_swap(c, i);
  c->activeLane = -1;
  c->cur = -1;  // the context's own working buffers do not hold that frame's level
  return rc;
}

// temporalJointBilateralFilter (TemporalBilateralFilter.h:126-215) of `planes` planes over a window of n frames,
// frame `centre` being the one filtered: one launch per kMaxTemporalFrames frames, the sums carried between them
int temporal_launch(derp_ctx* c, const void* const* guides, const float* const* images, const uint8_t* const* masks, int n,
                    int centre, int W, int H, int planes, float sigma, int radius, float w0, float w1, float w2,
                    float* out, const int* dst2src) {
  if (n < 1 || centre < 0 || centre >= n) {
    return fail(c, "temporal window must hold at least the centre frame");
  }
  if (n > kMaxTemporalFrames) {
    ALLOC(c, c->temporalCarry, (size_t)planes * W * H * sizeof(float2));
  }
  for (int t0 = 0; t0 < n; t0 += kMaxTemporalFrames) {
    TemporalFrames F;
    F.n = std::min(kMaxTemporalFrames, n - t0);
    for (int t = 0; t < F.n; ++t) {
      F.guides[t] = reinterpret_cast<const ushort4*>(guides[t0 + t]);
      F.images[t] = images[t0 + t];
      F.masks[t] = masks[t0 + t];
    }
    F.refGuide = reinterpret_cast<const ushort4*>(guides[centre]);
    F.refImage = images[centre];
    F.refMask = masks[centre];
    F.carry = n > kMaxTemporalFrames ? c->temporalCarry.as<float2>() : nullptr;
    F.first = t0 == 0;
    F.last = t0 + F.n >= n;
    // taps staged through LDS unless the halo makes the tile too big (two buffers of (32 + 2r) x (8 + 2r) x 9 bytes)
    const size_t lds = 2 * ((((size_t)(32 + 2 * radius) * (8 + 2 * radius) * 9) + 15) & ~(size_t)15);
    if (radius >= 0 && lds <= 48 * 1024 && !c->noTemporalTile) {
      hipLaunchKernelGGL(k_temporal_tiled, grid2d(W, H, planes, kBlk2d), kBlk2d, lds, c->stream, F, W, H, sigma, radius, w0,
                         w1, w2, out, dst2src);
    } else {
      hipLaunchKernelGGL(k_temporal, grid2d(W, H, planes, kBlk2d), kBlk2d, 0, c->stream, F, W, H, sigma, radius, w0, w1, w2,
                         out, dst2src);
    }
    KCHECK(c);
  }
  return 0;
}


}  // namespace

// ---- derp_render_*: SimpleMeshRenderer (derp_render.h) ----
namespace {

// glGenerateMipmap's level sizes (halve, round down, never below 1); false when the chain does not fit
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
  if (hipGetLastError() != hipSuccess) {
    return fail(c, "HIP error launching the render kernels");
  }
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
        hipLaunchKernelGGL(k_smr_stereo, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, k.vert.as<float4>(), n,
                           p.ipd, k.eyeVert.as<float4>());
        k.eyeIpd = p.ipd;
      }
    }
  }
  if (hipGetLastError() != hipSuccess) {
    return fail(c, "HIP error preparing the render inputs");
  }
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
  // equirectFS over the fullscreen triangle: texVar = (pixel centre) / size, GL rows read bottom-up and not flipped,
  // so output row r has texVar.y = (r + 0.5) / H and lat = -(texVar.y - 0.5) pi: row 0 is the north pole
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
  ALLOC(c, S.tabs, tab.size() * 4);
  HIPCHK(c, hipMemcpyAsync(S.tabs.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_smr_equirect, grid2d(W, E, 1, kBlk2d), kBlk2d, 0, c->stream, S.cube.as<float4>(), E, S.tabs.as<float>(),
                     S.tabs.as<float>() + 2 * W, W, E, out);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // `tab` goes out of scope
  return 0;
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
  const dim3 g((unsigned)((n + 255) / 256)), b(256);
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
  if (hipGetLastError() != hipSuccess) {
    return fail(c, "HIP error in the compositing kernels");
  }
  return 0;
}

}  // namespace

// =========================================================================================
extern "C" {

void derp_options_default(derp_options* o) {
  o->min_depth_m = 0.5f;
  o->max_depth_m = 1e4f;
  o->var_noise_floor = 4e-5f;
  o->var_high_thresh = 1e-3f;
  o->random_proposals = 2;
  o->ping_pong_iterations = 1;
  o->mismatches_start_level = -1;
  o->do_bilateral_filter = 1;
  o->do_median_filter = 1;
  o->use_foreground_masks = 0;
  o->partial_coverage = 0;
  o->rebuild_warp_tables = 1;
}

static thread_local std::string g_create_error;

int derp_create(derp_ctx** out, int device, const derp_camera_desc* src, int n_src, const derp_camera_desc* dst,
                int n_dst) {
  if (!out) {
    return 1;
  }
  *out = nullptr;
  std::unique_ptr<derp_ctx> owner(new derp_ctx);  // until success: an early return frees what was allocated so far
  derp_ctx* c = owner.get();
  derp_options_default(&c->opt);
  memset(c->accMs, 0, sizeof c->accMs);
  memset(c->accLaunch, 0, sizeof c->accLaunch);
  auto bail = [&](const std::string& m) {
    g_create_error = m;
    return 1;
  };
  if (n_src <= 0 || n_dst <= 0) {
    return bail("no source / destination cameras!");
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    return bail("no HIP device present: the depth path has no CPU fallback");
  }
  if (device < 0 || device >= count) {
    return bail("HIP device index out of range");
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    return bail("hipGetDeviceProperties failed");
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !getenv("DERP_ALLOW_ANY_ARCH")) {
    return bail(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  }
  if (hipSetDevice(device) != hipSuccess) {
    return bail("hipSetDevice failed");
  }
  c->device = device;
  if (prop.maxSharedMemoryPerMultiProcessor > 0) {
    c->ldsPerCu = prop.maxSharedMemoryPerMultiProcessor;
  }
  if (const char* e = getenv("DERP_XCD_ROTATE")) {
    c->xcdRotate = atoi(e);
  }
  c->noMemo = getenv("DERP_NO_MEMO") != nullptr;
  if (const char* e = getenv("DERP_PP_COMPACT")) {
    c->ppCompact = atoi(e) != 0;
  }
  if (const char* e = getenv("DERP_RANDOM_WAVES")) {
    c->randomWaves = atoi(e);
  }
  if (const char* e = getenv("DERP_PP_WAVES")) {
    c->ppWaves = atoi(e);
  }
  c->noTemporalTile = getenv("DERP_NO_TEMPORAL_TILE") != nullptr;
  c->noBlankSkip = getenv("DERP_NO_BLANK_SKIP") != nullptr;
  c->S = n_src;
  c->D = n_dst;
  c->frames.resize(1);
  c->camsSrcH.resize(n_src);
  c->camsDstH.resize(n_dst);
  for (int i = 0; i < n_src; ++i) {
    if (const char* m = host_prepare_camera(src[i], c->camsSrcH[i])) {
      return bail(std::string("camera ") + src[i].id + ": " + m);
    }
  }
  c->dst2srcH.assign(n_dst, 0);
  c->descDstH.assign(dst, dst + n_dst);
  for (int i = 0; i < n_dst; ++i) {
    if (const char* m = host_prepare_camera(dst[i], c->camsDstH[i])) {
      return bail(std::string("camera ") + dst[i].id + ": " + m);
    }
    bool found = false;
    for (int s = 0; s < n_src; ++s) {  // mapSrcToDstIndexes, DerpUtil.cpp:75-89
      if (strncmp(dst[i].id, src[s].id, sizeof dst[i].id) == 0) {
        c->dst2srcH[i] = s;
        found = true;
        break;
      }
    }
    if (!found) {
      return bail(std::string("destination camera ") + dst[i].id + " is not a source camera");
    }
    // The reference's destinations ARE rig cameras (filterDestinations, Derp.cpp:42-70, keeps a subset of the rig), and
    // k_reproject_bias relies on it: projWarpInv(d, s) is read from projWarp(ds, own) when s is destination ds. A
    // descriptor that shares an id with a source but not its intrinsics / pose would silently warp with the wrong camera.
    if (memcmp(&c->camsDstH[i], &c->camsSrcH[c->dst2srcH[i]], sizeof(Cam)) != 0) {
      return bail(std::string("destination camera ") + dst[i].id + " differs from the source camera of the same id "
                  "(destinations must be cameras of the source rig, as filterDestinations makes them)");
    }
  }
  if (c->camsSrc.ensure(sizeof(Cam) * n_src) || c->camsDst.ensure(sizeof(Cam) * n_dst) ||
      c->dst2src.ensure(sizeof(int) * n_dst) || c->counters.ensure(sizeof(unsigned long long) * ST_COUNT * kMaxLevels * 4)) {
    return bail("out of device memory");
  }
  // the streams last: they are torn down by derp_destroy alone, and nothing after them fails
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    return bail("hipStreamCreate failed");
  }
  if (hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    return bail("hipStreamCreate failed");
  }
  (void)hipMemcpy(c->camsSrc.p, c->camsSrcH.data(), sizeof(Cam) * n_src, hipMemcpyHostToDevice);
  (void)hipMemcpy(c->camsDst.p, c->camsDstH.data(), sizeof(Cam) * n_dst, hipMemcpyHostToDevice);
  (void)hipMemcpy(c->dst2src.p, c->dst2srcH.data(), sizeof(int) * n_dst, hipMemcpyHostToDevice);
  (void)hipMemset(c->counters.p, 0, c->counters.bytes);
  *out = owner.release();  // (the unique_ptr's: the caller owns the context now)
  return 0;
}

void derp_destroy(derp_ctx* c) {
  if (!c) {
    return;
  }
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (auto& l : c->lanes) {
    (void)hipStreamSynchronize(l->stream);
  }
  drain_spans(c);
  for (auto& l : c->lanes) {
    (void)hipStreamDestroy(l->stream);
    (void)hipEventDestroy(l->done);
  }
  if (c->laneReady) {
    (void)hipEventDestroy(c->laneReady);
  }
  (void)hipStreamDestroy(c->stream);
  (void)hipStreamDestroy(c->copyStream);
  delete c;  // every device buffer goes with its owner
}

const char* derp_last_error(const derp_ctx* c) {
  return c ? c->err.c_str() : g_create_error.c_str();
}

int derp_set_options(derp_ctx* c, const derp_options* o) {
  if (!c || !o) {
    return 1;
  }
  if (o->random_proposals < 0) {
    return fail(c, "Check failed: random_proposals >= 0");
  }
  c->opt = *o;
  return 0;
}

int derp_set_pyramid(derp_ctx* c, int num_levels, const int* widths, const int* heights, int width_full,
                     int height_full) {
  if (!c) {
    return 1;
  }
  if (num_levels <= 0 || num_levels > kMaxLevels) {
    return fail(c, "num_levels %d out of range (1..%d)", num_levels, kMaxLevels);
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->numLevels = num_levels;
  c->widthFull = width_full;
  c->heightFull = height_full;
  c->LW.assign(widths, widths + num_levels);
  c->LH.assign(heights, heights + num_levels);
  // a new geometry drops every frame slot (their buffers have the old sizes) and starts again with slot 0
  c->frames.clear();
  c->frames.resize(1);
  c->curSlot = 0;
  TRY(alloc_pyramid(c, c->frame()));
  size_t nmax = 0;
  for (int l = 0; l < num_levels; ++l) {
    nmax = std::max(nmax, npx(c, l));
  }
  TRY(alloc_work_set(c, c->w, nmax));
  c->cur = -1;
  c->warpCachedLevel = -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_set_frame_slots(derp_ctx* c, int n_slots) {
  if (!c || c->numLevels == 0) {
    return fail(c, "derp_set_pyramid has not been called");
  }
  if (n_slots < 1 || n_slots > 4096) {
    return fail(c, "n_slots %d out of range (1..4096)", n_slots);
  }
  HIPCHK(c, hipSetDevice(c->device));
  TRY(select_frame(c, 0));
  const int had = (int)c->frames.size();
  c->frames.resize(n_slots);  // growing moves the pyramids that exist: their buffers stay where they are
  for (int k = had; k < n_slots; ++k) {
    TRY(alloc_pyramid(c, c->frames[k]));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_select_frame(derp_ctx* c, int slot) {
  if (!c || c->numLevels == 0) {
    return fail(c, "derp_set_pyramid has not been called");
  }
  return select_frame(c, slot);
}

int derp_frame_slots(const derp_ctx* c, int* n_slots, int* selected) {
  if (!c) {
    return 1;
  }
  if (n_slots) {
    *n_slots = (int)c->frames.size();
  }
  if (selected) {
    *selected = c->curSlot;
  }
  return 0;
}

int derp_bind_thread(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return 0;
}
void* derp_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void derp_host_free(void* p) {
  if (p) {
    (void)hipHostFree(p);
  }
}
int derp_host_register(void* p, size_t bytes) {
  if (!p || bytes == 0 || hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return 1;
  }
  return 0;
}
void derp_host_unregister(void* p) {
  if (p && hipHostUnregister(p) != hipSuccess) {
    (void)hipGetLastError();
  }
}

int derp_upload_color(derp_ctx* c, int level, int s, const uint16_t* bgr) {
  TRY(check_level(c, level));
  if (s < 0 || s >= c->S || !bgr) {
    return fail(c, "bad source index / null image");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = npx(c, level);
  TRY(upload_tmp(c, c->w.staging, bgr, n * 3));
  hipLaunchKernelGGL(k_bgr_to_bgrx, dim3(flat_grid(n)), dim3(256), 0, c->stream, c->w.staging.as<uint16_t>(),
                     c->frame().color[level].as<ushort4>() + (size_t)s * n, n);
  KCHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));  // staging buffer is reused by the next upload
  if (c->warpCachedLevel == level) {
    // colour does not affect the warp tables; nothing to invalidate
  }
  return 0;
}

int derp_upload_foreground_mask(derp_ctx* c, int level, int s, const uint8_t* mask) {
  TRY(check_level(c, level));
  if (s < 0 || s >= c->S || !mask) {
    return fail(c, "bad source index / null mask");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = npx(c, level);
  HIPCHK(c, hipMemcpy(c->frame().fg[level].as<uint8_t>() + (size_t)s * n, mask, n, hipMemcpyHostToDevice));
  return 0;
}

int derp_upload_background_disparity(derp_ctx* c, int level, int d, const float* disp) {
  TRY(check_level(c, level));
  if (d < 0 || d >= c->D || !disp) {
    return fail(c, "bad destination index / null image");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = npx(c, level);
  HIPCHK(c, hipMemcpy(c->frame().bg[level].as<float>() + (size_t)d * n, disp, n * sizeof(float), hipMemcpyHostToDevice));
  c->frame().haveBg[level] = 1;
  return 0;
}

int derp_upload_disparity(derp_ctx* c, int level, int d, const float* disp) {
  TRY(check_level(c, level));
  if (d < 0 || d >= c->D || !disp) {
    return fail(c, "bad destination index / null image");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = npx(c, level);
  HIPCHK(c, hipMemcpy(c->frame().disp[level].as<float>() + (size_t)d * n, disp, n * sizeof(float), hipMemcpyHostToDevice));
  c->frame().haveDisp[level] = 1;
  return 0;
}

int derp_process_level(derp_ctx* c, int level) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return process_level(c, level);
}

int derp_process_pyramid(derp_ctx* c, int level_start, int level_end_) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (level_start < level_end_) {
    return fail(c, "Check failed: level_start >= level_end (%d vs %d)", level_start, level_end_);
  }
  for (int level = level_start; level >= level_end_; --level) {
    TRY(process_level(c, level));
  }
  return 0;
}

int derp_synchronize(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // coverage CHECK of computeBruteForceDisparity (Derp.cpp:334-349)
  if (c->numLevels > 0 && !c->opt.partial_coverage && !c->opt.use_foreground_masks) {
    unsigned long long v[4];
    HIPCHK(c, hipMemcpy(v, counter_slot(c, ST_BRUTE, c->numLevels - 1), sizeof v, hipMemcpyDeviceToHost));
    if (v[2] != 0) {
      return fail(c, "Check failed: partialCoverage || useForegroundMasks  Insufficient coverage at %llu pixels", v[2]);
    }
  }
  return 0;
}

int derp_download_disparity(derp_ctx* c, int level, int d, float* disparity) {
  TRY(check_level(c, level));
  if (d < 0 || d >= c->D || !disparity) {
    return fail(c, "bad destination index / null output");
  }
  if (!c->frame().haveDisp[level]) {
    return fail(c, "level %d has not been processed", level);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t n = npx(c, level);
  HIPCHK(c, hipMemcpy(disparity, c->frame().disp[level].as<float>() + (size_t)d * n, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int derp_download_cost(derp_ctx* c, int d, float* cost, float* confidence) {
  TRY(need_current(c, false));
  if (d < 0 || d >= c->D) {
    return fail(c, "bad destination index");
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t n = npx(c, c->cur);
  if (cost) {
    HIPCHK(c, hipMemcpy(cost, c->w.cost.as<float>() + (size_t)d * n, n * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (confidence) {
    HIPCHK(c, hipMemcpy(confidence, c->w.confidence.as<float>() + (size_t)d * n, n * sizeof(float), hipMemcpyDeviceToHost));
  }
  return 0;
}

// ---- stage-level API ----
int derp_level_begin(derp_ctx* c, int level) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return level_begin(c, level, true);
}
int derp_stage_reproject_colors(derp_ctx* c) {
  TRY(need_current(c, false));
  TRY(build_color_tables(c, 0, c->D));
  c->tablesValid = true;
  return 0;
}
int derp_stage_brute_force(derp_ctx* c) {
  TRY(need_current(c, true));
  return run_brute_force(c, 0, c->D);
}
int derp_stage_random_proposals(derp_ctx* c) {
  TRY(need_current(c, true));
  return run_random_proposals(c, 0, c->D);
}
int derp_stage_ping_pong(derp_ctx* c) {
  TRY(need_current(c, true));
  return run_ping_pong(c, 0, c->D);
}
int derp_stage_mismatches(derp_ctx* c) {
  TRY(need_current(c, false));
  return run_mismatches(c);
}
int derp_stage_bilateral_filter(derp_ctx* c) {
  TRY(need_current(c, false));
  return run_bilateral(c);
}
int derp_stage_median_filter(derp_ctx* c) {
  TRY(need_current(c, false));
  return run_median(c, false);
}
int derp_stage_mask_fov(derp_ctx* c) {
  TRY(need_current(c, false));
  return run_mask_fov(c);
}
int derp_level_end(derp_ctx* c) {
  TRY(need_current(c, false));
  return level_end(c);
}
int derp_set_level_disparity(derp_ctx* c, int d, const float* disp) {
  TRY(need_current(c, false));
  if (d < 0 || d >= c->D || !disp) {
    return fail(c, "bad destination index / null image");
  }
  const size_t n = npx(c, c->cur);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->w.disparity.as<float>() + (size_t)d * n, disp, n * sizeof(float), hipMemcpyHostToDevice));
  c->randomRanThisLevel = false;  // cost[] no longer belongs to the working disparity
  return 0;
}
int derp_get_level_disparity(derp_ctx* c, int d, float* disp) {
  TRY(need_current(c, false));
  if (d < 0 || d >= c->D || !disp) {
    return fail(c, "bad destination index / null output");
  }
  const size_t n = npx(c, c->cur);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(disp, c->w.disparity.as<float>() + (size_t)d * n, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int derp_cost_map(derp_ctx* c, int d, const float* disp, float* cost, float* confidence) {
  TRY(need_current(c, true));
  if (d < 0 || d >= c->D || !disp || !cost || !confidence) {
    return fail(c, "bad arguments");
  }
  const int L = c->cur;
  const size_t n = npx(c, L);
  TRY(upload_tmp(c, c->w.staging, disp, n));
  ALLOC(c, c->w.stagingB, 2 * n * sizeof(float));
  HIPCHK(c, hipMemsetAsync(c->w.stagingB.p, 0xff, 2 * n * sizeof(float), c->stream));  // NaN fill
  LevelView V = make_view(c, ST_PINGPONG, 0, c->D);
  int tilesX;
  const int tiles = tiles_of(V.W, V.H, tilesX);
  const size_t lds = kCostLdsPerSrc * (size_t)(c->S);
  hipLaunchKernelGGL(k_cost_map, dim3(tiles), dim3(kCostBlock), lds, c->stream, V, d, c->w.staging.as<float>(),
                     c->w.stagingB.as<float>(), c->w.stagingB.as<float>() + n, tilesX);
  KCHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(cost, c->w.stagingB.p, n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(confidence, c->w.stagingB.as<float>() + n, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int derp_debug_atan2_ypos(derp_ctx* c, const double* y, const double* x, double* out, size_t n) {
  if (!c || !y || !x || !out) {
    return fail(c, "bad arguments");
  }
  ALLOC(c, c->w.staging, 3 * n * sizeof(double));
  double* d = c->w.staging.as<double>();
  HIPCHK(c, hipMemcpyAsync(d, y, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + n, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_debug_atan2_ypos, dim3(flat_grid(n)), dim3(256), 0, c->stream, d, d + n, d + 2 * n, n);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(out, d + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_debug_fp64(derp_ctx* c, int op, const double* a, const double* b, double* out, size_t n) {
  if (!c || !a || !out || op < 0 || op > 3 || (op >= 2 && !b)) {
    return fail(c, "bad arguments");
  }
  if (n == 0) {
    return 0;
  }
  ALLOC(c, c->w.staging, 3 * n * sizeof(double));
  double* d = c->w.staging.as<double>();
  HIPCHK(c, hipMemcpyAsync(d, a, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + n, op >= 2 ? b : a, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_debug_fp64, dim3(flat_grid(n)), dim3(256), 0, c->stream, op, d, d + n, d + 2 * n, n);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(out, d + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_debug_sees(derp_ctx* c, int src, const double* xyz, size_t n, double* out) {
  if (!c || !xyz || !out || src < 0 || src >= c->S) {
    return fail(c, "bad arguments");
  }
  if (n == 0) {
    return 0;
  }
  ALLOC(c, c->w.staging, 9 * n * sizeof(double));
  double* d = c->w.staging.as<double>();
  HIPCHK(c, hipMemcpyAsync(d, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_debug_sees, dim3(flat_grid(n)), dim3(256), 0, c->stream, c->camsSrc.as<Cam>(), src, d, d + 3 * n, n);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(out, d + 3 * n, 6 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_debug_download(derp_ctx* c, int d, int s, int which, void* out) {
  TRY(need_current(c, false));
  const int L = c->cur;
  const int W = c->LW[L], H = c->LH[L];
  const size_t n = (size_t)W * H;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (which == 4) {
    HIPCHK(c, hipMemcpy(out, c->w.srcVar.as<float>() + (size_t)s * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  if (which == 5) {
    HIPCHK(c, hipMemcpy(out, c->w.fovMask.as<uint8_t>() + (size_t)d * n, n, hipMemcpyDeviceToHost));
    return 0;
  }
  if (d < 0 || d >= c->D || s < 0 || s >= c->S || s == c->dst2srcH[d]) {
    return fail(c, "bad (dst, src) pair");
  }
  const size_t tab = (size_t)d * (c->S - 1) + (s < c->dst2srcH[d] ? s : s - 1);
  if (which == 0) {
    const int PW = W + 2 * kPadW, PH = H + 2 * kPadW;
    std::vector<float2> tmp((size_t)PW * PH);
    HIPCHK(c, hipMemcpy(tmp.data(), c->projWarp.as<float2>() + tab * tmp.size(), tmp.size() * sizeof(float2),
                        hipMemcpyDeviceToHost));
    float2* o = reinterpret_cast<float2*>(out);
    for (int y = 0; y < H; ++y) {
      memcpy(o + (size_t)y * W, &tmp[(size_t)(y + kPadW) * PW + kPadW], (size_t)W * sizeof(float2));
    }
    return 0;
  }
  if (which == 2 || which == 3) {
    const int PW = W + 2 * kPadC, PH = H + 2 * kPadC;
    std::vector<ushort4> tmp((size_t)PW * PH);
    const ushort4* base = (which == 2 ? c->w.projColor.as<ushort4>() : c->w.projBias.as<ushort4>()) + tab * tmp.size();
    HIPCHK(c, hipMemcpy(tmp.data(), base, tmp.size() * sizeof(ushort4), hipMemcpyDeviceToHost));
    uint16_t* o = reinterpret_cast<uint16_t*>(out);
    for (int y = 0; y < H; ++y) {
      for (int x = 0; x < W; ++x) {
        const ushort4 q = tmp[(size_t)(y + kPadC) * PW + x + kPadC];
        o[((size_t)y * W + x) * 3 + 0] = q.x;
        o[((size_t)y * W + x) * 3 + 1] = q.y;
        o[((size_t)y * W + x) * 3 + 2] = q.z;
      }
    }
    return 0;
  }
  return fail(c, "unknown table id %d", which);
}

// ---- pyramid builder (scripts/render/resize.py:51-85) ----
static int build_pyramid(derp_ctx* c, int kind, int index, int count, const void* host, size_t elem, int w, int h,
                         int threshold) {
  if (!c || c->numLevels == 0) {
    return fail(c, "derp_set_pyramid has not been called");
  }
  if (index < 0 || index >= count || !host || w <= 0 || h <= 0) {
    return fail(c, "bad camera index / null image");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  ALLOC(c, c->fullFrame, n * elem);
  HIPCHK(c, hipMemcpyAsync(c->fullFrame.p, host, n * elem, hipMemcpyHostToDevice, c->stream));
  for (int l = 0; l < c->numLevels; ++l) {
    const size_t nl = npx(c, l);
    if (nl == 0) {
      continue;
    }
    void* dst = kind == 0 ? (void*)(c->frame().color[l].as<ushort4>() + (size_t)index * nl)
        : kind == 1       ? (void*)(c->frame().fg[l].as<uint8_t>() + (size_t)index * nl)
                          : (void*)(c->frame().bg[l].as<float>() + (size_t)index * nl);
    TRY(resize_area_dev(c, kind, c->fullFrame.p, w, h, dst, c->LW[l], c->LH[l], threshold));
    if (kind == 2) {
      c->frame().haveBg[l] = 1;
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));  // fullFrame is reused by the next call
  return 0;
}
int derp_build_pyramid_color(derp_ctx* c, int src, const uint16_t* bgr, int w, int h) {
  return build_pyramid(c, 0, src, c ? c->S : 0, bgr, 6, w, h, -1);
}
int derp_build_pyramid_foreground_mask(derp_ctx* c, int src, const uint8_t* mask, int w, int h, int threshold) {
  return build_pyramid(c, 1, src, c ? c->S : 0, mask, 1, w, h, threshold);
}
int derp_build_pyramid_background_disparity(derp_ctx* c, int dst, const float* disp, int w, int h) {
  return build_pyramid(c, 2, dst, c ? c->D : 0, disp, 4, w, h, -1);
}
int derp_download_level_color(derp_ctx* c, int level, int src, uint16_t* bgr) {
  TRY(check_level(c, level));
  if (src < 0 || src >= c->S || !bgr) {
    return fail(c, "bad source index / null output");
  }
  const size_t n = npx(c, level);
  ALLOC(c, c->w.staging, n * 6);
  hipLaunchKernelGGL(k_bgrx_to_bgr, dim3(flat_grid(n)), dim3(256), 0, c->stream,
                     c->frame().color[level].as<ushort4>() + (size_t)src * n, c->w.staging.as<uint16_t>(), n);
  KCHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(bgr, c->w.staging.p, n * 6, hipMemcpyDeviceToHost));
  return 0;
}
int derp_download_level_mask(derp_ctx* c, int level, int src, uint8_t* mask) {
  TRY(check_level(c, level));
  if (src < 0 || src >= c->S || !mask) {
    return fail(c, "bad source index / null output");
  }
  const size_t n = npx(c, level);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(mask, c->frame().fg[level].as<uint8_t>() + (size_t)src * n, n, hipMemcpyDeviceToHost));
  return 0;
}
int derp_download_level_background(derp_ctx* c, int level, int dst, float* disp) {
  TRY(check_level(c, level));
  if (dst < 0 || dst >= c->D || !disp) {
    return fail(c, "bad destination index / null output");
  }
  const size_t n = npx(c, level);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(disp, c->frame().bg[level].as<float>() + (size_t)dst * n, n * 4, hipMemcpyDeviceToHost));
  return 0;
}
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
  c->rephotoW = c->rephotoH = 0;
  ALLOC(c, c->rephotoColor, (size_t)c->S * n * 6);
  ALLOC(c, c->rephotoDisp, (size_t)c->S * n * 4);
  for (int s = 0; s < c->S; ++s) {
    if (!colors[s] || !disparities[s]) {
      return fail(c, "null colour / disparity for source %d", s);
    }
    HIPCHK(c, hipMemcpy((char*)c->rephotoColor.p + (size_t)s * n * 6, colors[s], n * 6, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy((char*)c->rephotoDisp.p + (size_t)s * n * 4, disparities[s], n * 4, hipMemcpyHostToDevice));
  }
  c->rephotoW = w;
  c->rephotoH = h;
  return 0;
}

int derp_rephotograph_render(derp_ctx* c, int target, float* out_bgra) {
  if (!c || !out_bgra || target < 0 || target >= c->S) {
    return fail(c, "bad arguments");
  }
  if (c->rephotoW <= 0) {
    return fail(c, "derp_rephotograph_upload has not been called");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int w = c->rephotoW, h = c->rephotoH;
  const size_t n = (size_t)w * h;
  DevBuf key, out;
  ALLOC(c, key, n * 8);
  ALLOC(c, out, n * 16);
  HIPCHK(c, hipMemsetAsync(key.p, 0xff, n * 8, c->stream));
  hipLaunchKernelGGL(k_rephoto_splat, grid2d(w, h, c->S, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), target,
                     c->rephotoDisp.as<float>(), w, h, key.as<unsigned long long>());
  hipLaunchKernelGGL(k_rephoto_resolve, grid2d(w, h, 1, kBlk2d), kBlk2d, 0, c->stream, c->camsSrc.as<Cam>(), target,
                     c->rephotoColor.as<uint16_t>(), key.as<unsigned long long>(), w, h, out.as<float4>());
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
  if (c->rephotoW <= 0) {
    return fail(c, "derp_rephotograph_upload has not been called");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const int w = c->rephotoW, h = c->rephotoH, E = edge;
  const size_t n = (size_t)w * h, nf = (size_t)E * E;
  // mip chain geometry (glGenerateMipmap): level sizes halve, rounding down, never below 1
  CanopyMips M;
  M.n = 0;
  size_t texels = 0;
  for (int lw = w, lh = h;; lw = std::max(1, lw >> 1), lh = std::max(1, lh >> 1)) {
    if (M.n >= kCanopyMaxLevels) {
      return fail(c, "image too large for the mip chain");
    }
    M.w[M.n] = lw;
    M.h[M.n] = lh;
    M.off[M.n] = (unsigned)texels;
    texels += (size_t)lw * lh;
    ++M.n;
    if (lw == 1 && lh == 1) {
      break;
    }
  }
  int nInc = 0;
  for (int s = 0; s < c->S; ++s) {
    nInc += include[s] != 0;
  }
  // per included camera: mesh vertices + the colour mip chain, built once and reused by the six faces
  DevBuf &vert = c->cnVert, &rgba = c->cnRgba, &zbuf = c->cnZ, &acc = c->cnAcc, &out = c->cnOut, &big = c->cnBig,
         &nBig = c->cnNBig;
  int rc = 0;
  if (vert.ensure((size_t)std::max(nInc, 1) * n * 16) || rgba.ensure((size_t)std::max(nInc, 1) * texels * 16) ||
      zbuf.ensure(nf * 8) || acc.ensure(nf * 16) || out.ensure(nf * 6 * 16) || big.ensure(n * 2 * sizeof(unsigned)) ||
      nBig.ensure(sizeof(unsigned))) {
    rc = fail(c, "out of device memory");
  } else {
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
                         c->rephotoColor.as<uint16_t>() + (size_t)s * n * 3, c->rephotoDisp.as<float>() + (size_t)s * n, w,
                         h, v, tex);
      for (int l = 1; l < M.n; ++l) {
        hipLaunchKernelGGL(k_canopy_mip, grid2d(M.w[l], M.h[l], 1, kBlk2d), kBlk2d, 0, c->stream, tex + M.off[l - 1],
                           M.w[l - 1], M.h[l - 1], tex + M.off[l], M.w[l], M.h[l]);
      }
      ++k;
    }
    // the reference's order: face-outer, camera-inner (the accumulation order of the cameras is part of the result)
    for (int face = 0; face < 6 && !rc; ++face) {
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
      if (hipGetLastError() != hipSuccess) {
        rc = fail(c, "HIP error launching the canopy kernels");
      }
    }
    if (!rc && (hipStreamSynchronize(c->stream) != hipSuccess ||
                hipMemcpy(out_bgra, out.p, nf * 6 * 16, hipMemcpyDeviceToHost) != hipSuccess)) {
      rc = fail(c, "HIP error in derp_canopy_cubemap: %s", hipGetErrorString(hipGetLastError()));
    }
  }
  return rc;
}

int derp_download_mismatch_mask(derp_ctx* c, int d, uint8_t* out) {
  TRY(need_current(c, false));
  if (d < 0 || d >= c->D || !out) {
    return fail(c, "bad destination index / null output");
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t n = npx(c, c->cur);
  HIPCHK(c, hipMemcpy(out, c->w.mismatchMask.as<uint8_t>() + (size_t)d * n, n, hipMemcpyDeviceToHost));
  return 0;
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

// ---- conversion tools at the depth stage's inputs and outputs (derp_points.h) ----
namespace {
// Camera::rescale({w, h}) of the rig camera as the file holds it (Camera.cpp:217-223): principal *= new / res and
// focal *= new / res, the quotient first — the order that gives the reference's rescaled camera bit for bit. (The depth
// path's normalised camera x level size rounds differently.) No principal in the file: resolution / 2 (Camera.cpp:44-48).
ScaledCam scaled_cam(const derp_camera_desc& j, int w, int h) {
  const double qx = (double)w / j.resolution[0], qy = (double)h / j.resolution[1];
  const double prx = j.has_principal ? j.principal[0] : j.resolution[0] / 2;
  const double pry = j.has_principal ? j.principal[1] : j.resolution[1] / 2;
  return {prx * qx, pry * qy, j.focal[0] * qx, j.focal[1] * qy, (double)w, (double)h};
}
int points_blocks(size_t n) {
  return (int)((n + kPointsBlock - 1) / kPointsBlock);
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
  if (cam < 0 || cam >= c->D) {
    return fail(c, "bad camera index %d (the context has %d)", cam, c->D);
  }
  if (subsample < 1) {
    return fail(c, "subsample must be >= 1");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  const int nb = points_blocks(n);
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
  c->pointsImagesH.clear();
  ALLOC(c, c->pointsDisp, floats * 4);
  TRY(upload_sync(c, c->pointsImages, images.data(), images.size() * sizeof(PointsImage)));
  HIPCHK(c, hipMemset(c->pointsDisp.p, 0, floats * 4));  // (the images start at 0: ImportPointCloud.cpp:83)
  c->pointsImagesH = images;
  return 0;
}

int derp_points_splat(derp_ctx* c, const double* xyz, size_t n, double min_depth, double max_depth) {
  if (!c || (!xyz && n > 0)) {
    return fail(c, "bad arguments (null pointer)");
  }
  if (c->pointsImagesH.empty()) {
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
  TRY(upload_sync(c, c->pointsXyz, xyz, n * 24));
  hipLaunchKernelGGL(k_points_splat, dim3(points_blocks(n)), dim3(kPointsBlock), 0, c->stream, c->camsDst.as<Cam>(),
                     c->pointsImages.as<PointsImage>(), c->D, c->pointsXyz.as<double>(), n, min_depth, max_depth,
                     c->pointsDisp.as<float>());
  KCHECK(c);
  return 0;
}

int derp_points_download(derp_ctx* c, int cam, float* disparity) {
  if (!c || !disparity) {
    return fail(c, "bad arguments (null pointer)");
  }
  if (c->pointsImagesH.empty()) {
    return fail(c, "derp_points_begin has not been called");
  }
  if (cam < 0 || cam >= c->D) {
    return fail(c, "bad camera index %d (the context has %d)", cam, c->D);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const PointsImage& im = c->pointsImagesH[cam];
  return download_sync(c, disparity, c->pointsDisp.as<float>() + im.offset, (size_t)im.w * im.h * 4);
}

int derp_project_equirect_mask(derp_ctx* c, int cam, const uint8_t* eqr, int eqr_w, int eqr_h, int w, int h, double depth,
                               uint8_t* out) {
  if (!c || !eqr || !out || eqr_w <= 0 || eqr_h <= 0 || w <= 0 || h <= 0 || (size_t)w * h >= kMaxPixels ||
      (size_t)eqr_w * eqr_h >= kMaxPixels) {
    return fail(c, "bad arguments (null pointer or image size)");
  }
  if (cam < 0 || cam >= c->D) {
    return fail(c, "bad camera index %d (the context has %d)", cam, c->D);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  DevBuf e, m;
  TRY(upload_sync(c, e, eqr, (size_t)eqr_w * eqr_h));
  ALLOC(c, m, n);
  hipLaunchKernelGGL(k_project_equirect_mask, dim3(points_blocks(n)), dim3(kPointsBlock), 0, c->stream,
                     c->camsDst.as<Cam>() + cam, scaled_cam(c->descDstH[cam], w, h), e.as<uint8_t>(), eqr_w, eqr_h, w, h, depth,
                     m.as<uint8_t>());
  KCHECK(c);
  return download_sync(c, out, m.p, n);
}

// ---- ConvertToBinary's camera meshes (derp_mesh.h; the collapse loop is derp_simplify.cpp) ----
namespace {
// resizeNN's source index of every destination index (cv::resize INTER_NEAREST): min(floor(x * (1 / fx)), ssize - 1),
// where fx is the scale the caller gave (cv::Size() + fx) or dsize / ssize (a given dsize)
void nearest_table(int ssize, int dsize, double fx, int* out) {
  const double ifx = 1. / fx;
  for (int x = 0; x < dsize; ++x) {
    out[x] = std::min((int)std::floor(x * ifx), ssize - 1);
  }
}
int mesh_blocks(size_t n) {
  return (int)((n + kMeshBlock - 1) / kMeshBlock);
}
int need_mesh(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  if (!c->mesh || !c->mesh->built) {
    return fail(c, "derp_mesh_build has not been called");
  }
  return 0;
}
// computeInitialQuadrics of the built mesh into m.planes / m.costs / m.vq
int mesh_setup_dev(derp_ctx* c, int equi_error) {
  MeshState& m = *c->mesh;
  ALLOC(c, m.planes, std::max<size_t>(m.nf * 32, 8));
  ALLOC(c, m.costs, std::max<size_t>(m.nf * 24, 8));
  ALLOC(c, m.vq, std::max<size_t>(m.nv * derp_mesh::kQuadric * 8, 8));
  if (m.nf == 0 || m.nv == 0) {
    return 0;
  }
  hipLaunchKernelGGL(k_mesh_face_planes, dim3(mesh_blocks(m.nf)), dim3(kMeshBlock), 0, c->stream, m.V.as<double>(),
                     m.F.as<int32_t>(), m.nf, m.planes.as<double>());
  hipLaunchKernelGGL(k_mesh_vertex_quadrics, dim3(mesh_blocks(m.nv)), dim3(kMeshBlock), 0, c->stream, m.qmask.as<uint8_t>(),
                     m.qoff.as<uint32_t>(), m.vorig.as<uint32_t>(), m.W, m.H, m.nv, m.planes.as<double>(), m.vq.as<double>());
  hipLaunchKernelGGL(k_mesh_edge_costs, dim3(mesh_blocks(m.nf * 3)), dim3(kMeshBlock), 0, c->stream, m.V.as<double>(),
                     m.F.as<int32_t>(), m.nf, m.vq.as<double>(), equi_error, m.costs.as<double>());
  KCHECK(c);
  return 0;
}
}  // namespace

int derp_mesh_build(derp_ctx* c, int cam, const float* disparity, int w, int h, const double* resolution, double depth_scale,
                    const uint8_t* mask, int mask_w, int mask_h, float tear_ratio) {
  if (!c || !disparity || w <= 0 || h <= 0 || (size_t)w * h >= kMaxPixels || !(depth_scale > 0) ||
      (mask && (mask_w <= 0 || mask_h <= 0 || (size_t)mask_w * mask_h >= kMaxPixels))) {
    return fail(c, "bad arguments (null pointer, image size or depth scale)");
  }
  if (cam < 0 || cam >= c->D) {
    return fail(c, "bad camera index %d (the context has %d)", cam, c->D);
  }
  // Camera::rescale(resolution) of the rig camera as the file holds it (resizeRig, ConvertToBinary.cpp:318-339), then
  // getScalarFocal (Camera.cpp:185-188)
  const derp_camera_desc& j = c->descDstH[cam];
  double resx = j.resolution[0], resy = j.resolution[1], fx = j.focal[0], fy = j.focal[1];
  if (resolution) {
    fx *= resolution[0] / resx;
    fy *= resolution[1] / resy;
    resx = resolution[0];
    resy = resolution[1];
  }
  if (fx != -fy) {
    return fail(c, "Check failed: focal.x() == -focal.y() (%.17g vs. %.17g) pixels are not square", fx, -fy);
  }
  // cv::resize(depth, depth, cv::Size(), s, s, INTER_NEAREST) when s < 1: dsize = saturate_cast<int>(ssize * s)
  const bool scaled = depth_scale < 1;
  const int W = scaled ? (int)std::nearbyint(w * depth_scale) : w, H = scaled ? (int)std::nearbyint(h * depth_scale) : h;
  if (W <= 0 || H <= 0) {
    return fail(c, "depth scale %g leaves no pixels of a %d x %d map", depth_scale, w, h);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the mesh built before this one may still be read
  if (!c->mesh) {
    c->mesh.reset(new MeshState);
  }
  MeshState& m = *c->mesh;
  m.built = m.simplified = false;
  m.W = W;
  m.H = H;
  std::vector<int> tabs(2 * (size_t)W + 2 * (size_t)H);
  int *xofs = tabs.data(), *yofs = xofs + W, *mxofs = yofs + H, *myofs = mxofs + W;
  nearest_table(w, W, scaled ? depth_scale : 1.0, xofs);
  nearest_table(h, H, scaled ? depth_scale : 1.0, yofs);
  if (mask) {  // cv::resize(foregroundMask, foregroundMask, depth.size(), 0, 0, INTER_NEAREST)
    nearest_table(mask_w, W, (double)W / mask_w, mxofs);
    nearest_table(mask_h, H, (double)H / mask_h, myofs);
  }
  const size_t n = (size_t)W * H;
  const int nb = mesh_blocks(n);
  TRY(upload_sync(c, m.disparity, disparity, (size_t)w * h * 4));
  TRY(upload_sync(c, m.tabs, tabs.data(), tabs.size() * 4));
  if (mask) {
    TRY(upload_sync(c, m.mask, mask, (size_t)mask_w * mask_h));
  }
  ALLOC(c, m.vert, n * 24);
  ALLOC(c, m.valid, n);
  ALLOC(c, m.qmask, n);
  ALLOC(c, m.used, n);
  ALLOC(c, m.blockFaces, (size_t)nb * 4);
  ALLOC(c, m.blockVerts, (size_t)nb * 4);
  ALLOC(c, m.offF, (size_t)nb * 8);
  ALLOC(c, m.offV, (size_t)nb * 8);
  ALLOC(c, m.totals, 24);
  ALLOC(c, m.vmap, n * 4);
  ALLOC(c, m.qoff, n * 4);
  const int* dt = m.tabs.as<int>();
  unsigned long long* totals = m.totals.as<unsigned long long>();  // kept faces, kept vertices, unmasked faces
  HIPCHK(c, hipMemsetAsync(totals, 0, 24, c->stream));
  hipLaunchKernelGGL(k_mesh_vertices, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.disparity.as<float>(), w, dt, dt + W, W, H,
                     resx, resy, fx, mask ? m.mask.as<uint8_t>() : (const uint8_t*)nullptr, mask_w, dt + W + H,
                     dt + 2 * W + H, m.vert.as<double>(), m.valid.as<uint8_t>());
  hipLaunchKernelGGL(k_mesh_quads, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.vert.as<double>(), m.valid.as<uint8_t>(), W, H,
                     tear_ratio, m.qmask.as<uint8_t>(), m.blockFaces.as<uint32_t>(), totals + 2);
  hipLaunchKernelGGL(k_mesh_vertex_used, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.qmask.as<uint8_t>(), W, H,
                     m.used.as<uint8_t>(), m.blockVerts.as<uint32_t>());
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, m.blockFaces.as<uint32_t>(), nb,
                     m.offF.as<unsigned long long>(), totals);
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, m.blockVerts.as<uint32_t>(), nb,
                     m.offV.as<unsigned long long>(), totals + 1);
  KCHECK(c);
  unsigned long long t[3] = {0, 0, 0};
  TRY(download_sync(c, t, totals, 24));
  m.nf = (size_t)t[0];
  m.nv = (size_t)t[1];
  m.nfUnmasked = (size_t)t[2];
  if (m.nv > n || m.nf > 2 * n) {
    return fail(c, "derp_mesh_build: inconsistent counts (%zu vertices, %zu faces for %zu pixels)", m.nv, m.nf, n);
  }
  ALLOC(c, m.vorig, std::max<size_t>(m.nv * 4, 8));
  ALLOC(c, m.V, std::max<size_t>(m.nv * 24, 8));
  ALLOC(c, m.F, std::max<size_t>(m.nf * 12, 8));
  hipLaunchKernelGGL(k_mesh_vertex_scatter, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.vert.as<double>(), m.used.as<uint8_t>(),
                     n, m.offV.as<unsigned long long>(), m.vmap.as<uint32_t>(), m.vorig.as<uint32_t>(), m.V.as<double>());
  hipLaunchKernelGGL(k_mesh_face_scatter, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.qmask.as<uint8_t>(), W, H,
                     m.offF.as<unsigned long long>(), m.vmap.as<uint32_t>(), m.qoff.as<uint32_t>(), m.F.as<int32_t>());
  KCHECK(c);
  m.built = true;
  return 0;
}

int derp_mesh_counts(derp_ctx* c, size_t* vertices, size_t* faces, size_t* faces_unmasked) {
  TRY(need_mesh(c));
  const MeshState& m = *c->mesh;
  if (vertices) {
    *vertices = m.simplified ? m.sV.size() / 3 : m.nv;
  }
  if (faces) {
    *faces = m.simplified ? m.sF.size() / 3 : m.nf;
  }
  if (faces_unmasked) {
    *faces_unmasked = m.nfUnmasked;
  }
  return 0;
}

int derp_mesh_download_f64(derp_ctx* c, double* vertices, int32_t* faces) {
  TRY(need_mesh(c));
  const MeshState& m = *c->mesh;
  if (m.simplified) {
    if (vertices) {
      memcpy(vertices, m.sV.data(), m.sV.size() * 8);
    }
    if (faces) {
      memcpy(faces, m.sF.data(), m.sF.size() * 4);
    }
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (vertices && m.nv) {
    TRY(download_sync(c, vertices, m.V.p, m.nv * 24));
  }
  if (faces && m.nf) {
    TRY(download_sync(c, faces, m.F.p, m.nf * 12));
  }
  return 0;
}

int derp_mesh_download(derp_ctx* c, int clamp_negative_z, float* vtx, uint32_t* idx) {
  TRY(need_mesh(c));
  size_t nv = 0, nf = 0;
  TRY(derp_mesh_counts(c, &nv, &nf, nullptr));
  std::vector<double> v(nv * 3);
  std::vector<int32_t> f(nf * 3);
  TRY(derp_mesh_download_f64(c, vtx ? v.data() : nullptr, idx ? f.data() : nullptr));
  if (vtx) {
    for (size_t i = 0; i < nv * 3; ++i) {
      // "If depth is slightly negative ... we force this values to the minimum positive value" (:211-217), on the
      // double, before writeDepth's cast<float>
      vtx[i] = clamp_negative_z && i % 3 == 2 && v[i] < 0 ? FLT_MIN : (float)v[i];
    }
  }
  if (idx) {
    for (size_t i = 0; i < nf * 3; ++i) {
      idx[i] = (uint32_t)f[i];
    }
  }
  return 0;
}

int derp_mesh_setup(derp_ctx* c, int equi_error, double* face_planes, double* edge_costs, double* vertex_quadrics) {
  TRY(need_mesh(c));
  MeshState& m = *c->mesh;
  if (m.simplified) {
    return fail(c, "derp_mesh_setup: the mesh has been simplified (the set-up belongs to the mesh as built)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  TRY(mesh_setup_dev(c, equi_error));
  if (face_planes && m.nf) {
    TRY(download_sync(c, face_planes, m.planes.p, m.nf * 32));
  }
  if (edge_costs && m.nf) {
    TRY(download_sync(c, edge_costs, m.costs.p, m.nf * 24));
  }
  if (vertex_quadrics && m.nv) {
    TRY(download_sync(c, vertex_quadrics, m.vq.p, m.nv * derp_mesh::kQuadric * 8));
  }
  return 0;
}

int derp_mesh_simplify(derp_ctx* c, int num_faces_out, float strictness, int remove_boundary_edges, int equi_error,
                       int host_setup, int* stats) {
  TRY(need_mesh(c));
  MeshState& m = *c->mesh;
  if (m.simplified) {
    return fail(c, "derp_mesh_simplify: the mesh has been simplified already");
  }
  if (num_faces_out < 0) {
    return fail(c, "derp_mesh_simplify: a negative face budget");
  }
  std::vector<double> V(m.nv * 3), planes, costs, vq;
  std::vector<int32_t> F(m.nf * 3);
  TRY(derp_mesh_download_f64(c, V.data(), F.data()));
  if (!host_setup) {
    planes.resize(m.nf * 4);
    costs.resize(m.nf * 3);
    vq.resize(m.nv * derp_mesh::kQuadric);
    TRY(derp_mesh_setup(c, equi_error, planes.data(), costs.data(), vq.data()));
  }
  m.sV.resize(V.size());
  m.sF.resize(F.size());
  size_t nv = 0, nf = 0;
  if (derp_mesh_simplify_host(V.data(), m.nv, F.data(), m.nf, host_setup ? nullptr : planes.data(),
                              host_setup ? nullptr : costs.data(), host_setup ? nullptr : vq.data(), num_faces_out, strictness,
                              remove_boundary_edges, equi_error, m.sV.data(), m.sF.data(), &nv, &nf, stats)) {
    return fail(c, "derp_mesh_simplify_host refused the built mesh");
  }
  m.sV.resize(nv * 3);
  m.sF.resize(nf * 3);
  m.simplified = true;
  return 0;
}

// rocPRIM's stable radix sort of (cost key, face * 3 + edge): Onesweep with 256 threads x 8 items (its default for
// this pair of types spills to scratch memory), from 4096 items on, so that the tests' meshes take the path of
// full-size ones
namespace {
using MeshSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<256, 8>, 8>, 4096>;
}

// The pass-parallel simplifier (derp_mesh.h, "the pass-parallel simplifier"): the whole loop on the device, the host
// reads one set of counters per pass.
int derp_mesh_simplify_parallel(derp_ctx* c, int num_faces_out, float strictness, int remove_boundary_edges, int equi_error,
                                int* stats) {
  TRY(need_mesh(c));
  MeshState& m = *c->mesh;
  if (m.simplified) {
    return fail(c, "derp_mesh_simplify_parallel: the mesh has been simplified already");
  }
  if (num_faces_out < 0) {
    return fail(c, "derp_mesh_simplify_parallel: a negative face budget");
  }
  HIPCHK(c, hipSetDevice(c->device));
  m.passes.clear();
  int passes = 0, reason = DERP_MESH_EXIT_BUDGET;
  const size_t nf = m.nf, nv = m.nv, n3 = nf * 3;
  long long aliveFaces = (long long)nf;
  if (n3 >= (size_t)kMeshApplied) {
    return fail(c, "derp_mesh_simplify_parallel: %zu faces are more than an edge rank holds", nf);
  }
  if (aliveFaces > num_faces_out) {
    TRY(mesh_setup_dev(c, equi_error));
    const int nbF = mesh_blocks(nf), nbV = mesh_blocks(nv), nbE = mesh_blocks(n3);
    ALLOC(c, m.alive, nf);
    ALLOC(c, m.boundary, nv);
    ALLOC(c, m.vcount, nv * 4);
    ALLOC(c, m.vstart, nv * 4);
    ALLOC(c, m.vcursor, nv * 4);
    ALLOC(c, m.adj, n3 * 4);
    ALLOC(c, m.keys, n3 * 8);
    ALLOC(c, m.keysFeasible, n3 * 8);
    ALLOC(c, m.keysSorted, n3 * 8);
    ALLOC(c, m.vals, n3 * 4);
    ALLOC(c, m.valsSorted, n3 * 4);
    ALLOC(c, m.claim, nf * 4);
    ALLOC(c, m.wins, n3 * 4);
    ALLOC(c, m.blockSum, (size_t)nbE * 4);
    ALLOC(c, m.blockOff, (size_t)nbE * 8);
    ALLOC(c, m.counters, (MESH_CNT_SLOTS + 1) * 8);
    double* V = m.V.as<double>();
    int32_t* F = m.F.as<int32_t>();
    double *costs = m.costs.as<double>(), *vq = m.vq.as<double>();
    const double* planes = m.planes.as<double>();
    uint8_t *alive = m.alive.as<uint8_t>(), *boundary = m.boundary.as<uint8_t>();
    uint32_t *claim = m.claim.as<uint32_t>(), *wins = m.wins.as<uint32_t>(), *blockSum = m.blockSum.as<uint32_t>();
    unsigned long long *blockOff = m.blockOff.as<unsigned long long>(), *counters = m.counters.as<unsigned long long>();
    const MeshAdjacency A = {m.vstart.as<uint32_t>(), m.vcount.as<uint32_t>(), m.adj.as<uint32_t>()};
    const dim3 blk(kMeshBlock);
    HIPCHK(c, hipMemsetAsync(alive, 1, nf, c->stream));
    HIPCHK(c, hipMemsetAsync(boundary, 0, nv, c->stream));
    while (aliveFaces > num_faces_out) {
      if ((size_t)passes >= nf) {  // every pass with a candidate deletes a face
        return fail(c, "derp_mesh_simplify_parallel: %d passes over %zu faces", passes, nf);
      }
      // adjacency of the alive faces
      HIPCHK(c, hipMemsetAsync(m.vcount.p, 0, nv * 4, c->stream));
      HIPCHK(c, hipMemsetAsync(counters, 0, MESH_CNT_SLOTS * 8, c->stream));
      HIPCHK(c, hipMemsetAsync(claim, 0xff, nf * 4, c->stream));
      hipLaunchKernelGGL(k_par_vertex_degrees, dim3(nbF), blk, 0, c->stream, F, alive, nf, m.vcount.as<uint32_t>());
      hipLaunchKernelGGL(k_par_block_sums<uint32_t>, dim3(nbV), blk, 0, c->stream, m.vcount.as<uint32_t>(), nv, blockSum);
      hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbV, blockOff,
                         counters + MESH_CNT_SLOTS);
      hipLaunchKernelGGL(k_par_vertex_starts, dim3(nbV), blk, 0, c->stream, m.vcount.as<uint32_t>(), nv, blockOff,
                         m.vstart.as<uint32_t>(), m.vcursor.as<uint32_t>());
      hipLaunchKernelGGL(k_par_adjacency_fill, dim3(nbF), blk, 0, c->stream, F, alive, nf, m.vcursor.as<uint32_t>(),
                         m.adj.as<uint32_t>());
      if (passes == 0) {
        hipLaunchKernelGGL(k_par_boundaries, dim3(nbE), blk, 0, c->stream, A, F, nf, boundary);
      }
      // feasible set, its order, claims, winners
      hipLaunchKernelGGL(k_par_feasible, dim3(nbE), blk, 0, c->stream, A, V, F, alive, nf, planes, costs, vq, boundary,
                         remove_boundary_edges, equi_error, m.keys.as<unsigned long long>(), blockSum);
      hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbE, blockOff,
                         counters + MESH_CNT_FEASIBLE);
      hipLaunchKernelGGL(k_par_feasible_compact, dim3(nbE), blk, 0, c->stream, m.keys.as<unsigned long long>(), n3, blockOff,
                         m.keysFeasible.as<unsigned long long>(), m.vals.as<uint32_t>());
      KCHECK(c);
      unsigned long long feasible = 0;
      TRY(download_sync(c, &feasible, counters + MESH_CNT_FEASIBLE, 8));
      if (feasible == 0) {
        reason = DERP_MESH_EXIT_NO_CANDIDATES;
        break;
      }
      if (feasible > n3) {
        return fail(c, "derp_mesh_simplify_parallel: %llu feasible edges of %zu", feasible, n3);
      }
      size_t tempBytes = 0;
      HIPCHK(c, rocprim::radix_sort_pairs<MeshSortConfig>(nullptr, tempBytes, m.keysFeasible.as<unsigned long long>(),
                                                          m.keysSorted.as<unsigned long long>(), m.vals.as<uint32_t>(),
                                                          m.valsSorted.as<uint32_t>(), (size_t)feasible, 0, 64, c->stream));
      ALLOC(c, m.sortTemp, std::max<size_t>(tempBytes, 8));
      HIPCHK(c, rocprim::radix_sort_pairs<MeshSortConfig>(m.sortTemp.p, tempBytes, m.keysFeasible.as<unsigned long long>(),
                                                          m.keysSorted.as<unsigned long long>(), m.vals.as<uint32_t>(),
                                                          m.valsSorted.as<uint32_t>(), (size_t)feasible, 0, 64, c->stream));
      const unsigned long long* skeys = m.keysSorted.as<unsigned long long>();
      const uint32_t* svals = m.valsSorted.as<uint32_t>();
      const int nbN = mesh_blocks((size_t)feasible);  // from here on one thread per feasible edge, by rank
      hipLaunchKernelGGL(k_par_claim, dim3(nbN), blk, 0, c->stream, A, F, skeys, svals, strictness, counters, claim);
      hipLaunchKernelGGL(k_par_winners, dim3(nbN), blk, 0, c->stream, A, F, skeys, svals, strictness, claim, counters, wins,
                         blockSum);
      // budget cut in key order, then the collapses
      hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbN, blockOff,
                         counters + MESH_CNT_SLOTS);
      hipLaunchKernelGGL(k_par_apply_vertices, dim3(nbN), blk, 0, c->stream, V, F, vq, boundary, equi_error, svals, blockOff,
                         aliveFaces, (long long)num_faces_out, wins, counters);
      hipLaunchKernelGGL(k_par_apply_faces, dim3(nbF), blk, 0, c->stream, V, F, alive, nf, vq, boundary, equi_error, svals, claim,
                         wins, costs);
      KCHECK(c);
      unsigned long long cnt[MESH_CNT_SLOTS];
      TRY(download_sync(c, cnt, counters, sizeof cnt));
      if (cnt[MESH_CNT_DELETED] == 0 || cnt[MESH_CNT_DELETED] > (unsigned long long)aliveFaces) {
        return fail(c, "derp_mesh_simplify_parallel: pass %d deleted %llu of %lld faces", passes, cnt[MESH_CNT_DELETED], aliveFaces);
      }
      derp_mesh_pass p;
      p.faces = aliveFaces;
      p.feasible = (long long)cnt[MESH_CNT_FEASIBLE];
      p.winners = (long long)cnt[MESH_CNT_WINNERS];
      p.applied = (long long)cnt[MESH_CNT_APPLIED];
      p.deleted = (long long)cnt[MESH_CNT_DELETED];
      p.threshold = mesh_key_cost(cnt[MESH_CNT_THRESHOLD]);
      m.passes.push_back(p);
      aliveFaces -= (long long)cnt[MESH_CNT_DELETED];
      ++passes;
    }
    // createFinalMesh
    uint8_t* used = m.used.as<uint8_t>();  // (grid-sized: at least nv bytes)
    uint32_t* vmap = m.vmap.as<uint32_t>();
    ALLOC(c, m.outV, std::max<size_t>(nv * 24, 8));
    ALLOC(c, m.outF, std::max<size_t>(nf * 12, 8));
    HIPCHK(c, hipMemsetAsync(used, 0, nv, c->stream));
    hipLaunchKernelGGL(k_par_vertices_used, dim3(nbF), blk, 0, c->stream, F, alive, nf, used);
    hipLaunchKernelGGL(k_par_block_sums<uint8_t>, dim3(nbV), blk, 0, c->stream, used, nv, blockSum);
    hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbV, blockOff, counters);
    hipLaunchKernelGGL(k_par_final_vertices, dim3(nbV), blk, 0, c->stream, V, used, nv, blockOff, vmap, m.outV.as<double>());
    hipLaunchKernelGGL(k_par_block_sums<uint8_t>, dim3(nbF), blk, 0, c->stream, alive, nf, blockSum);
    hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbF, blockOff, counters + 1);
    hipLaunchKernelGGL(k_par_final_faces, dim3(nbF), blk, 0, c->stream, F, alive, nf, blockOff, vmap, m.outF.as<int32_t>());
    KCHECK(c);
    unsigned long long out[2] = {0, 0};
    TRY(download_sync(c, out, counters, sizeof out));
    if (out[0] > nv || (long long)out[1] != aliveFaces) {
      return fail(c, "derp_mesh_simplify_parallel: inconsistent result (%llu vertices, %llu faces, %lld alive)", out[0], out[1],
                  aliveFaces);
    }
    m.sV.resize((size_t)out[0] * 3);
    m.sF.resize((size_t)out[1] * 3);
    if (out[0]) {
      TRY(download_sync(c, m.sV.data(), m.outV.p, m.sV.size() * 8));
    }
    if (out[1]) {
      TRY(download_sync(c, m.sF.data(), m.outF.p, m.sF.size() * 4));
    }
  } else {  // 0 passes: the mesh as built
    m.sV.resize(nv * 3);
    m.sF.resize(nf * 3);
    TRY(derp_mesh_download_f64(c, m.sV.data(), m.sF.data()));
  }
  m.simplified = true;
  if (stats) {
    stats[0] = passes;
    stats[1] = reason;
  }
  return 0;
}

int derp_mesh_parallel_pass(derp_ctx* c, int pass, derp_mesh_pass* out) {
  TRY(need_mesh(c));
  const MeshState& m = *c->mesh;
  if (!out || pass < 0 || (size_t)pass >= m.passes.size()) {
    return fail(c, "derp_mesh_parallel_pass: no pass %d (the last derp_mesh_simplify_parallel ran %zu)", pass, m.passes.size());
  }
  *out = m.passes[pass];
  return 0;
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

int derp_joint_bilateral_u16(derp_ctx* c, const float* image, const uint16_t* guide, const uint8_t* mask, int w, int h,
                             int radius, float sigma, float w0, float w1, float w2, float* out) {
  if (!c || !image || !guide || !mask || !out || radius < 0 || bilateral_lds_bytes(radius) > 64 * 1024) {
    return fail(c, "bad arguments (radius must be in [0, 47])");
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
  hipLaunchKernelGGL(k_joint_bilateral<true>, dim3((w + 15) / 16, (h + 15) / 16, 1), dim3(256),
                     bilateral_lds_bytes(radius), c->stream, im.as<float>(), (const void*)g4.as<ushort4>(),
                     m.as<uint8_t>(), w, h, radius, sigma, w0, w1, w2, res.as<float>(), n, n, (const int*)nullptr);
  return download_sync(c, out, res.p, n * 4);
}

int derp_joint_bilateral_f32(derp_ctx* c, const float* image, const float* guide, const uint8_t* mask, int w, int h,
                             int radius, float sigma, float w0, float w1, float w2, float* out) {
  if (!c || !image || !guide || !mask || !out || radius < 0 || bilateral_lds_bytes(radius) > 64 * 1024) {
    return fail(c, "bad arguments (radius must be in [0, 47])");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)w * h;
  DevBuf im, g, m, res;
  TRY(upload_sync(c, im, image, n * 4));
  TRY(upload_sync(c, g, guide, n * 12));
  TRY(upload_sync(c, m, mask, n));
  ALLOC(c, res, n * 4);
  hipLaunchKernelGGL(k_joint_bilateral<false>, dim3((w + 15) / 16, (h + 15) / 16, 1), dim3(256),
                     bilateral_lds_bytes(radius), c->stream, im.as<float>(), (const void*)g.as<float>(),
                     m.as<uint8_t>(), w, h, radius, sigma, w0, w1, w2, res.as<float>(), n, n, (const int*)nullptr);
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

int derp_dev_disparity(derp_ctx* c, int level, int d, float** ptr, size_t* bytes) {
  TRY(check_level(c, level));
  if (d < 0 || d >= c->D || !ptr || !bytes) {
    return fail(c, "bad destination index / null output");
  }
  const size_t n = npx(c, level);
  *ptr = c->frame().disp[level].as<float>() + (size_t)d * n;
  *bytes = n * sizeof(float);
  return 0;
}
int derp_dev_color(derp_ctx* c, int level, int s, void** ptr, size_t* bytes) {
  TRY(check_level(c, level));
  if (s < 0 || s >= c->S || !ptr || !bytes) {
    return fail(c, "bad source index / null output");
  }
  const size_t n = npx(c, level);
  *ptr = c->frame().color[level].as<ushort4>() + (size_t)s * n;
  *bytes = n * sizeof(ushort4);
  return 0;
}
int derp_dev_mask(derp_ctx* c, int level, int d, uint8_t** ptr, size_t* bytes) {
  TRY(check_level(c, level));
  if (d < 0 || d >= c->D || !ptr || !bytes) {
    return fail(c, "bad destination index / null output");
  }
  HIPCHK(c, hipSetDevice(c->device));
  // fov & fg of `level` (TemporalBilateralFilter.cpp:150-160) for every destination, into a buffer of its
  // own (never a working buffer of the level loop), complete when this call returns
  const int W = c->LW[level], H = c->LH[level];
  const size_t n = (size_t)W * H;
  ALLOC(c, c->devMask, n * c->D);
  hipLaunchKernelGGL(k_fov_mask, grid2d(W, H, c->D, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>(), W, H,
                     c->devMask.as<uint8_t>());
  KCHECK(c);
  hipLaunchKernelGGL(k_and_masks, dim3(flat_grid(n), c->D), dim3(256), 0, c->stream, c->devMask.as<uint8_t>(),
                     c->frame().fg[level].as<uint8_t>(), c->dst2src.as<int>(), 0, n, c->devMask.as<uint8_t>());
  KCHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *ptr = c->devMask.as<uint8_t>() + (size_t)d * n;
  *bytes = n;
  return 0;
}

int derp_get_counters(derp_ctx* c, uint64_t* n_cost, uint64_t* n_pair, uint64_t* insufficient) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> h((size_t)ST_COUNT * kMaxLevels * 4);
  HIPCHK(c, hipMemcpy(h.data(), c->counters.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  uint64_t a = 0, b = 0, i = 0;
  for (size_t k = 0; k < h.size(); k += 4) {
    a += h[k];
    b += h[k + 1];
    i += h[k + 2];
  }
  if (n_cost) {
    *n_cost = a;
  }
  if (n_pair) {
    *n_pair = b;
  }
  if (insufficient) {
    *insufficient = i;
  }
  return 0;
}
int derp_reset_counters(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipMemsetAsync(c->counters.p, 0, c->counters.bytes, c->stream));
  return 0;
}
int derp_profile_enable(derp_ctx* c, int on) {
  if (!c) {
    return 1;
  }
  c->profiling = on != 0;
  return 0;
}
int derp_profile_reset(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  drain_spans(c);
  memset(c->accMs, 0, sizeof c->accMs);
  memset(c->accLaunch, 0, sizeof c->accLaunch);
  return derp_reset_counters(c);
}
int derp_profile_query(derp_ctx* c, const char* stage, int level, double* ms, int* launches, uint64_t* n_cost,
                       uint64_t* n_pair) {
  if (!c || !stage) {
    return 1;
  }
  int st = -1;
  for (int i = 0; i < ST_COUNT; ++i) {
    if (strcmp(stage, kStageNames[i]) == 0) {
      st = i;
    }
  }
  if (st < 0) {
    return fail(c, "unknown stage '%s'", stage);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  drain_spans(c);
  std::vector<unsigned long long> h((size_t)kMaxLevels * 4);
  HIPCHK(c, hipMemcpy(h.data(), counter_slot(c, st, 0), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double m = 0;
  int l = 0;
  uint64_t a = 0, b = 0;
  for (int lv = 0; lv < kMaxLevels; ++lv) {
    if (level >= 0 && lv != level) {
      continue;
    }
    m += c->accMs[st][lv];
    l += c->accLaunch[st][lv];
    a += h[(size_t)lv * 4];
    b += h[(size_t)lv * 4 + 1];
  }
  if (ms) {
    *ms = m;
  }
  if (launches) {
    *launches = l;
  }
  if (n_cost) {
    *n_cost = a;
  }
  if (n_pair) {
    *n_pair = b;
  }
  return 0;
}
int derp_profile_memoised(derp_ctx* c, const char* stage, int level, uint64_t* n_memoised) {
  if (!c || !stage || !n_memoised) {
    return 1;
  }
  int st = -1;
  for (int i = 0; i < ST_COUNT; ++i) {
    if (strcmp(stage, kStageNames[i]) == 0) {
      st = i;
    }
  }
  if (st < 0) {
    return fail(c, "unknown stage '%s'", stage);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> h((size_t)kMaxLevels * 4);
  HIPCHK(c, hipMemcpy(h.data(), counter_slot(c, st, 0), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  uint64_t m = 0;
  for (int lv = 0; lv < kMaxLevels; ++lv) {
    if (level < 0 || lv == level) {
      m += h[(size_t)lv * 4 + 3];
    }
  }
  *n_memoised = m;
  return 0;
}
int derp_device_memory(derp_ctx* c, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipSetDevice(c->device));
  size_t f = 0, t = 0;
  HIPCHK(c, hipMemGetInfo(&f, &t));
  if (free_bytes) {
    *free_bytes = f;
  }
  if (total_bytes) {
    *total_bytes = t;
  }
  return 0;
}

int derp_device_name(derp_ctx* c, char* buf, int n) {
  if (!c || !buf || n <= 0) {
    return 1;
  }
  hipDeviceProp_t prop;
  HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
  snprintf(buf, n, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return 0;
}

// ---- host-only self checks ----
namespace {
struct HostPairs {
  SsdPair* p;
  SsdPair get(int i) const {
    return p[i];
  }
  void set(int i, const SsdPair& v) {
    p[i] = v;
  }
};
}  // namespace
int derp_host_nth_element_pairs(float* pairs, int n, int nth) {
  HostPairs acc{reinterpret_cast<SsdPair*>(pairs)};
  GccSelect<HostPairs> sel(acc);
  sel.nth_element(nth, n);
  return 0;
}
float derp_host_minstd_uniform(int seed, uint64_t draw_index, float a, float b) {
  uint32_t state = minstd_jump(minstd_seed(seed), draw_index);
  return minstd_uniform(state, a, b);
}

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

static int smr_check(derp_ctx* c, const derp_render_params* p) {
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

static void smr_out_size(const derp_render_params& p, int& w, int& h) {
  w = p.kind == DERP_RENDER_SNAPSHOT ? p.width : p.kind == DERP_RENDER_CUBE ? p.height : 2 * p.height;
  h = p.kind == DERP_RENDER_CUBE ? 6 * p.height : p.height;
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
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out_bgra, S.img.p, n * 16, hipMemcpyDeviceToHost));
  return 0;
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
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out_xyzw, (ipd != 0.0f ? k.eyeVert : k.vert).p, (size_t)k.dw * k.dh * 16, hipMemcpyDeviceToHost));
  return 0;
}

// SimpleMeshRenderer's --format list (SimpleMeshRenderer.cpp:66-77): what each renders and how it is stacked
enum SmrFormat { kCubeColor, kCubeDisp, kEqrColor, kEqrDisp, kLr180, kSnapColor, kSnapDisp, kTb3dof, kTbStereo };
static int smr_format(const char* f) {
  static const char* names[] = {"cubecolor", "cubedisp", "eqrcolor", "eqrdisp", "lr180", "snapcolor", "snapdisp", "tb3dof", "tbstereo"};
  for (int i = 0; f && i < 9; ++i) {
    if (std::strcmp(f, names[i]) == 0) {
      return i;
    }
  }
  return -1;
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
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out_bgra, S.img.p, n * 16, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

#include "derp_sequence.h"
#include "derp_isp.h"
#include "derp_sim.h"
