// C-ABI implementation of include/derp_hip.h, the root of the library's one HIP translation unit. This file is the depth
// core: context, HBM-resident pyramid and frame slots, level driver and its stages, the stage-level API, work lanes and
// the pyramid builder. The tool families' entry points are the derp_*_api.h included at the end ("where
// things live in csrc/"). Host side mirrors the reference's DerpCLI level loop (DerpCLI.cpp:220-323) and processLevel
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
#include "derp_host.h"
#include "derp_kernels.h"
#include "derp_mesh.h"
#include "derp_points.h"
#include "derp_render.h"
#include "derp_stream.h"
#include "derp_geometric.h"
#include "derp_sweep.h"
#include "derp_align.h"
#include "derp_coverage.h"
#include "derp_preview.h"

using namespace derp;

#include "derp_ctx.h"

namespace {

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
  V.fovMask = c->fovMask.as<uint8_t>();
  V.pairCount = c->w.pairCount.as<uint8_t>();
  V.counters = counter_slot(c, stage, L);
#if DERP_BLOCK_TRACE
  V.blockTrace = nullptr;
#endif
  return V;
}
// DERP_BLOCK_TRACE builds: the launch of random proposals (which = 0) / ping-pong (1) about to go out records its blocks
int block_trace_attach(derp_ctx* c, LevelView& V, int which, int gridX, int gridY) {
#if DERP_BLOCK_TRACE
  DevBuf& buf = c->blockTrace[which][V.level];
  const size_t bytes = (size_t)gridX * gridY * 2 * sizeof(unsigned long long);
  ALLOC(c, buf, bytes);
  HIPCHK(c, hipMemsetAsync(buf.as<unsigned long long>(), 0, bytes, c->stream));
  V.blockTrace = buf.as<unsigned long long>();
  c->blockTraceGrid[which][V.level][0] = gridX;
  c->blockTraceGrid[which][V.level][1] = gridY;
#else
  (void)c, (void)V, (void)which, (void)gridX, (void)gridY;
#endif
  return 0;
}

// k_variance_bias: 64 x 4 threads, each a column strip of kBlurRows rows
const dim3 kBlurBlk(64, 4, 1);
dim3 blur_grid(int ow, int oh, int planes) {
  return dim3((ow + 63) / 64, (oh + 4 * kBlurRows - 1) / (4 * kBlurRows), planes);
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
  // the most source positions a run of kLanczosH outputs reaches: first tap of its first output to last tap of its last
  for (int d0 = 0; d0 < dsize; d0 += kLanczosH) {
    const int d1 = std::min(d0 + kLanczosH, dsize) - 1;
    const int lo = std::min(std::max(ofs[d0] - 3, 0), ssize - 1), hi = std::min(std::max(ofs[d1] + 4, 0), ssize - 1);
    t.tileSpan = std::max(t.tileSpan, hi - lo + 1);
    t.monotone = t.monotone && std::is_sorted(ofs.begin() + d0, ofs.begin() + d1 + 1);
  }
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

// cv2.resize(src, (dw, dh), INTER_AREA): kind 0 BGR u16 -> BGRX, 1 u8 (-> {0,1} when threshold >= 0), 2 f32, 3 f32 x3,
// 4 BGRA u16 -> BGRA int16 (k_resize_area)
int resize_area_dev(derp_ctx* c, int kind, const void* src, int sw, int sh, void* dst, int dw, int dh, int threshold) {
  if (dw > sw || dh > sh) {
    // enlarging along an axis: cv::resize(INTER_AREA) turns into its bilinear emulation (float images only here)
    if (kind < 2 || kind == 4) {
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
  } else if (kind == 4) {
    hipLaunchKernelGGL(k_resize_area<4>, g, kBlk2d, 0, c->stream, src, sw, sh, dst, dw, dh, ax, ay, threshold);
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
  if (ty->monotone && ty->tileSpan <= kLanczosRows) {
    hipLaunchKernelGGL(k_lanczos, dim3((dw + kLanczosW - 1) / kLanczosW, (dh + kLanczosH - 1) / kLanczosH, planes),
                       dim3(kLanczosW, 4), 0, c->stream, in, sw, sh, dw, dh, tx->ofs.as<int>(), tx->coef.as<float>(),
                       ty->ofs.as<int>(), ty->coef.as<float>(), out, inStride, outStride);
    KCHECK(c);
    return 0;
  }
  // a tile that reaches over more source rows than the kernel's window holds (downsampling): the two passes
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

// The table budget -> the destination batch: how many of the D destinations' projection tables fit `budget` bytes.
// Batches need stored inverse warps for the sources outside them, so a level that does not fit whole pays
// `perWithInverse` bytes per destination. DB = 0: bad sizes, or not even one destination fits. Pure arithmetic.
TableBatch plan_table_batch(int D, size_t perNoInverse, size_t perWithInverse, bool inverseNeededAnyway, size_t budget) {
  if (D < 1 || perNoInverse == 0 || perWithInverse == 0) {
    return {0, false};
  }
  const bool inv = inverseNeededAnyway || budget / perNoInverse < (size_t)D;
  const int DB = (int)std::min<size_t>(D, budget / (inv ? perWithInverse : perNoInverse));
  if (DB < 1) {
    return {0, inv};
  }
  // equal-sized batches: 24 destinations under a 23-destination budget run as 12 + 12, not 23 + 1
  const int batches = (D + DB - 1) / DB;
  return {(D + batches - 1) / batches, inv};
}

// only the frame that opens a level honours opt.rebuild_warp_tables, for the warps and the FOV masks alike
bool rebuilds_tables(const derp_ctx* c, LevelUse use) {
  return use == LevelUse::Open && c->opt.rebuild_warp_tables;
}

int compute_fov_and_masks(derp_ctx* c, int level, LevelUse use) {
  const int W = c->LW[level], H = c->LH[level];
  const size_t n = (size_t)W * H;
  {
    Span sp(c, ST_FOV, level);
    // the FOV masks depend on the rig and the level size only, like the projection warps, and follow their rule
    // (rebuilds_tables, warpCachedLevel): the first frame of a level builds them into the context's buffer, the
    // other frames of the level, on the work lanes too, read them there. fov & fg stays per frame.
    if (rebuilds_tables(c, use) || c->fovCachedLevel != level) {
      hipLaunchKernelGGL(k_fov_mask, grid2d(W, H, c->D, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>(), W, H,
                         c->fovMask.as<uint8_t>());
      KCHECK(c);
      c->fovCachedLevel = level;
    }
    hipLaunchKernelGGL(k_and_masks, dim3(flat_grid(n), c->D), dim3(256), 0, c->stream, c->fovMask.as<uint8_t>(),
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
  // new warps (another level, batch or rig state): every work set's colour tables, the lanes' too, must be rewritten in full
  ++c->warpGeneration;
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
  // level frame after frame) skips the tiles no source pixel maps into — they still hold their zeros. The level index
  // alone does not say so: this work set may have met the index last under other warps or another geometry (a lane keeps
  // its state from sequence to sequence), with its tables and flags laid out for those.
  const int skipBlank = c->w.colorTablesCleanLevel == L && c->w.colorTablesWarpGeneration == c->warpGeneration &&
      nd == c->D && !c->noBlankSkip;
  const auto kernel = c->reprojectSerial ? k_reproject_bias : k_reproject_bias_front;  // the same tables either way
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, V, c->projWarpInv.as<float2>(),
                     c->w.projColor.as<ushort4>(), c->w.projBias.as<ushort4>(), c->w.projColorT.as<ushort4>(),
                     c->w.tileSeen.as<uint8_t>(), skipBlank);
  KCHECK(c);
  c->w.colorTablesCleanLevel = nd == c->D ? L : -1;
  c->w.colorTablesWarpGeneration = c->warpGeneration;
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
// How a launch of random proposals / ping-pong lays a level's `tiles` (tiles_of) over its blocks: the blocks of the
// grid's x (a multiple of 8 * bands: xcd_swizzle), each walking `perBlock` consecutive tiles. Tile indices at or past
// `tiles` fall below the image (tile_pixel) and do nothing.
struct CostGrid {
  int blocks, bands, perBlock;
};
// bands (K), random proposals (`spread`): as many as leave a run no shorter than one row of kTileBlock squares (tilesX * 4 *
// kTileBlock wave tiles: thinner runs would widen what an XCD's L2 serves at one time), at most kCostMaxBands. Their gate
// passes the pixels unevenly over the image, and with one band each the XCDs' shares differ. Ping-pong: 1. Its XCDs end
// within 1 % of one another as it is, and four bands cost its level-0 launch 1 % (profiles/r13_cost_tile_order.txt).
// perBlock (N): 1. The kernels that walk N > 1 tiles spill (the level's scalars stay live around the tile loop) and are a
// quarter slower; they stay for the A/B. DERP_XCD_BANDS / DERP_COST_TILES_PER_BLOCK force K / N for both kernels.
constexpr int kCostMaxBands = 4, kCostMaxTilesPerBlock = 4;
int cost_grid_blocks(int tiles, int bands, int perBlock) {
  const int items = (tiles + perBlock - 1) / perBlock, unit = 8 * bands;
  return (items + unit - 1) / unit * unit;
}
CostGrid cost_grid(const derp_ctx* c, int tiles, int tilesX, bool spread) {
  const auto pow2_floor = [](int v, int cap) {
    int p = 1;
    while (p * 2 <= std::min(v, cap)) {
      p *= 2;
    }
    return p;
  };
  CostGrid g;
  g.perBlock = c->costTilesPerBlock > 0 ? pow2_floor(c->costTilesPerBlock, kCostMaxTilesPerBlock) : 1;
  const int rowOfSquares = tilesX * (256 / kCostBlock) * kTileBlock;
  g.bands = c->xcdBands > 0 ? pow2_floor(c->xcdBands, kCostMaxBands)
                            : spread ? pow2_floor(std::max(1, tiles / (8 * rowOfSquares)), kCostMaxBands) : 1;
  g.blocks = cost_grid_blocks(tiles, g.bands, g.perBlock);
  return g;
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
  // one wave per (strip, run of disparity indices, destination): 49 x 15 x 16 at the 16-camera rig's 50 x 50 level with runs
  // of 10, times the frames on the work lanes — still far above the chip's 4096 wave slots
  const int run = std::min(std::max(c->bruteRun, 1), kNumDepths);
  hipLaunchKernelGGL(k_brute_costs, dim3(tiles, (kNumDepths + run - 1) / run, nd), dim3(kCostBlock), lds, c->stream, V,
                     c->w.bruteCost.as<float>(), c->w.bruteConf.as<float>(), tilesX, tiles, run);
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
    // (a^P)^k for every count k of gated-in pixels a row can hold: built when P changes or a wider level arrives
    WorkSet& w = c->w;
    if (w.rankPowersP != V.randomProposals || w.rankPowersN < V.W) {
      const int count = *std::max_element(c->LW.begin(), c->LW.end());  // the widest level: once per pyramid
      ALLOC(c, w.rankPowers, (size_t)count * sizeof(uint32_t));
      hipLaunchKernelGGL(k_minstd_powers, dim3(blocks_of(count, 256)), dim3(256), 0, c->stream, V.randomProposals, count,
                         w.rankPowers.as<uint32_t>());
      KCHECK(c);
      w.rankPowersP = V.randomProposals;
      w.rankPowersN = count;
    }
    hipLaunchKernelGGL(k_row_rank, dim3(V.H - 2, nd), dim3(256), 0, c->stream, V, w.rankPowers.as<uint32_t>(),
                       w.rank.as<int>());
    KCHECK(c);
  }
  int tilesX;
  const int tiles = tiles_of(V.W, V.H, tilesX);
  const size_t lds = lds_for_waves(kCostLdsPerSrc * (size_t)(c->S), c->randomWaves, c->ldsPerCu, kCostLdsStatic);
  const CostGrid cg = cost_grid(c, tiles, tilesX, true);
  TRY(block_trace_attach(c, V, 0, cg.blocks, nd));
  const bool four = cost_four_waves(c);
  const auto kernel = cg.perBlock > 1 ? (four ? k_random_proposals_walk : k_random_proposals_walk_w3)
                                      : (four ? k_random_proposals : k_random_proposals_w3);
  hipLaunchKernelGGL(kernel, dim3(cg.blocks, nd), dim3(kCostBlock), lds, c->stream, V, c->w.rank.as<int>(), tilesX, cg.bands, cg.perBlock);
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
  int tilesX;
  const int tiles = tiles_of(V.W, V.H, tilesX);
  const size_t lds = lds_for_waves(kCostLdsPerSrc * (size_t)(c->S), c->ppWaves, c->ldsPerCu, kCostLdsStatic);
  const bool four = cost_four_waves(c);
  const CostGrid cg = cost_grid(c, tiles, tilesX, false);
  const auto kernel = cg.perBlock > 1
                          ? (c->ppCompact ? (four ? k_ping_pong_walk : k_ping_pong_walk_w3) : (four ? k_ping_pong_loop_walk : k_ping_pong_loop_walk_w3))
                          : (c->ppCompact ? (four ? k_ping_pong : k_ping_pong_w3) : (four ? k_ping_pong_loop : k_ping_pong_loop_w3));
  TRY(block_trace_attach(c, V, 1, cg.blocks, nd));
  // Every iteration writes all pixels of its result planes, and `changed` = result != input for the next one (what the
  // reference's commit does, Derp.cpp:527-529), so nothing is copied back: the odd iterations read disparity / cost and
  // write dispRes / costRes, the even ones the other way round, and `changed` alternates between the two halves of its
  // buffer — none before the first iteration (null: every pixel counts as changed). The memoised candidate is read in the
  // first iteration only, from cost / confidence / pairCount as random proposals left them.
  float* dispBuf[2] = {c->w.disparity.as<float>(), c->w.dispRes.as<float>()};
  float* costBuf[2] = {c->w.cost.as<float>(), c->w.costRes.as<float>()};
  uint8_t* chgBuf[2] = {c->w.changed.as<uint8_t>(), c->w.changed.as<uint8_t>() + n * c->D};
  const int iterations = c->opt.ping_pong_iterations;
  for (int it = 1; it <= iterations; ++it) {
    const int from = (it - 1) & 1, to = it & 1;
    V.disparity = dispBuf[from];
    V.cost = costBuf[from];
    hipLaunchKernelGGL(kernel, dim3(cg.blocks, nd), dim3(kCostBlock), lds, c->stream, V,
                       it == 1 ? (const uint8_t*)nullptr : chgBuf[from], chgBuf[to], dispBuf[to], costBuf[to], tilesX,
                       (int)(it == 1 && c->randomRanThisLevel && !c->noMemo), cg.bands, cg.perBlock);
    KCHECK(c);
  }
  if (dst0 + nd >= c->D) {
    // the last batch is through: every batch ran the same number of iterations, so after an odd number all of them left
    // their results in dispRes / costRes, which now become the working disparity and cost
    if (iterations > 0 && (iterations & 1)) {
      std::swap(c->w.disparity, c->w.dispRes);
      std::swap(c->w.cost, c->w.costRes);
    }
    // cost / confidence now belong to ping-pong's result (+inf where every candidate was rejected): the
    // memoised candidate must not be served from them by a later derp_stage_ping_pong call
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
  const size_t side = 16 + 2 * (size_t)radius;
  const size_t t = ((side + 15) & ~(size_t)15) * side;
  return t * 4 * sizeof(float) + ((t + 3) & ~(size_t)3);
}

// what a block of k_joint_bilateral may ask for: 64 KiB less the kernel's own 256 B (its exp table)
constexpr size_t kBilateralMaxLds = 64 * 1024 - 256;

// The preconditions of k_joint_bilateral's FAST_TAP form with a u16 guide (bilateral_tap_fast): unit second and third
// weights, a first weight in [0, inf), and 0 < 2 sigma^2 < inf as the kernel computes it
bool bilateral_fast_tap_ok(float sigma, float w0, float w1, float w2) {
  const float denom = 2.0f * (sigma * sigma);
  return w1 == 1.0f && w2 == 1.0f && w0 >= 0.0f && std::isfinite(w0) && denom > 0.0f && std::isfinite(denom);
}

// The preconditions of k_temporal_tiled's FAST form (temporal_tap<true>): all three weights in [0, inf), and
// 0 < sigma^2 < inf as the kernel computes it
bool temporal_fast_tap_ok(float sigma, float w0, float w1, float w2) {
  const float sig2 = sigma * sigma;
  const auto weight_ok = [](float w) { return w >= 0.0f && std::isfinite(w); };
  return weight_ok(w0) && weight_ok(w1) && weight_ok(w2) && sig2 > 0.0f && std::isfinite(sig2);
}

// the tiled kernel with a u16 guide, in the form its parameters allow: the same bits either way
void launch_joint_bilateral_u16_tiled(derp_ctx* c, dim3 grid, const float* image, const void* guide, const uint8_t* mask,
                                      int W, int H, int radius, float sigma, float w0, float w1, float w2, float* out,
                                      size_t planeStride, size_t guideStride, const int* guideIndex) {
  // (the fast form's block vote takes another 256 B of static LDS: the largest tiles, radius 22, leave no room for it)
  const bool fast = bilateral_fast_tap_ok(sigma, w0, w1, w2) && bilateral_lds_bytes(radius) + 256 <= kBilateralMaxLds;
  const auto kernel = fast ? k_joint_bilateral<true, true> : k_joint_bilateral<true, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), bilateral_lds_bytes(radius), c->stream, image, guide, mask, W, H, radius, sigma,
                     w0, w1, w2, out, planeStride, guideStride, guideIndex);
}

int run_bilateral(derp_ctx* c) {
  const int L = c->cur;
  Span sp(c, ST_BILATERAL, L);
  c->randomRanThisLevel = false;  // the working disparity changes: cost[] no longer matches it
  const int W = c->LW[L], H = c->LH[L];
  const size_t n = (size_t)W * H;
  // weights passed (B, G, R) = (0.5, 1, 1) — Derp.cpp:893-896, Derp.h:44-48; sigma 0.005
  const int radius = bilateral_radius(L);
  launch_joint_bilateral_u16_tiled(c, dim3((W + 15) / 16, (H + 15) / 16, c->D), c->w.disparity.as<float>(),
                                   (const void*)c->frame().color[L].as<ushort4>(), c->w.maskAnd.as<uint8_t>(), W, H, radius,
                                   0.005f, 0.5f, 1.0f, 1.0f, c->w.tmpF.as<float>(), n, n, c->dst2src.as<int>());
  KCHECK(c);
  // the filtered planes become the working disparity: the two buffers exchange roles (both hold D planes of the
  // largest level), nothing is copied back
  std::swap(c->w.disparity, c->w.tmpF);
  return 0;
}

// `levelOut`: the level loop's last stage writes the frame's level (frame().disp[L]) itself and the level is complete;
// as a stage of its own (null) the result becomes the working disparity, like the bilateral filter's
int run_median(derp_ctx* c, bool fuseMaskFov, float* levelOut = nullptr) {
  const int L = c->cur;
  Span sp(c, ST_MEDIAN, L);
  c->randomRanThisLevel = false;  // the working disparity changes: cost[] no longer matches it
  const int W = c->LW[L], H = c->LH[L];
  const size_t n = (size_t)W * H;
  hipLaunchKernelGGL(k_masked_median, grid2d(W, H, c->D, kBlk2d), kBlk2d, 0, c->stream, c->w.disparity.as<float>(),
                     c->opt.use_foreground_masks ? c->frame().bg[L].as<float>() : (const float*)nullptr,
                     c->w.maskAnd.as<uint8_t>(), W, H, 1, levelOut ? levelOut : c->w.tmpF.as<float>(), n,
                     fuseMaskFov ? c->fovMask.as<uint8_t>() : (const uint8_t*)nullptr);
  KCHECK(c);
  if (!levelOut) {
    std::swap(c->w.disparity, c->w.tmpF);
  }
  return 0;
}

int run_mask_fov(derp_ctx* c, float* levelOut = nullptr) {
  const int L = c->cur;
  Span sp(c, ST_MASKFOV, L);
  const size_t n = npx(c, L) * c->D;
  hipLaunchKernelGGL(k_mask_fov, dim3(flat_grid(n)), dim3(256), 0, c->stream, c->w.disparity.as<float>(),
                     c->fovMask.as<uint8_t>(), levelOut ? levelOut : c->w.disparity.as<float>(), n);
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

// a level the level loop can run: present, 3 x 3 at least, on a rig within the cost kernels' source limit
int check_level_runs(derp_ctx* c, int level) {
  TRY(check_level(c, level));
  if (c->S - 1 > kMaxSrc) {
    return fail(c, "too many source cameras (%d > %d)", c->S, kMaxSrc + 1);
  }
  if (c->LW[level] < 3 || c->LH[level] < 3) {
    return fail(c, "level %d is too small (%dx%d)", level, c->LW[level], c->LH[level]);
  }
  return 0;
}

// What the frames of a pass over `level` share: the table budget -> the destination batch, and the warp buffers at that
// batch. It depends on the rig, the level size and the free memory only. The one place that asks the runtime for the
// free memory and the one place that allocates a buffer the work lanes share; it enqueues nothing.
int level_open(derp_ctx* c, int level) {
  TRY(check_level_runs(c, level));
  ++c->plan.decisions;
  c->plan.level = -1;  // until the new plan stands
  const int W = c->LW[level], H = c->LH[level];
  const size_t n = (size_t)W * H;
  // When the buffers already hold every destination's tables of this level (the steady state of a sequence: same
  // levels frame after frame) there is nothing to ask the runtime.
  // (the inverse-warp table only exists when a batch holds a source that is not one of its destinations)
  const bool invAll = batch_needs_inverse_warps(c, 0, c->D);
  TableBatch batch{c->D, invAll};
  const size_t wpAll = (size_t)(W + 2 * kPadW) * (H + 2 * kPadW) * (c->S - 1) * c->D * sizeof(float2);
  const size_t cpAll = (size_t)(W + 2 * kPadC) * (H + 2 * kPadC) * (c->S - 1) * c->D * sizeof(ushort4);
  const size_t ipAll = n * (c->S - 1) * c->D * sizeof(float2);
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
    const size_t perInverse = table_bytes_per_dst(c, W, H, true);
    batch = plan_table_batch(c->D, table_bytes_per_dst(c, W, H, false), perInverse, invAll, budget);
    if (batch.DB < 1) {
      return fail(c, "projection tables for one destination (%zu bytes) exceed the table budget (%zu bytes)", perInverse, budget);
    }
  }
  ALLOC(c, c->projWarp, (size_t)batch.DB * (c->S - 1) * (W + 2 * kPadW) * (H + 2 * kPadW) * sizeof(float2));
  if (batch.storeInverse) {
    ALLOC(c, c->projWarpInv, (size_t)batch.DB * (c->S - 1) * n * sizeof(float2));
  }
  c->plan.level = level;
  c->plan.DB = batch.DB;
  c->plan.storeInverse = batch.storeInverse;
  return 0;
}

// One frame's set-up of a level whose plan stands: what DerpCLI does before processLevel (DerpCLI.cpp:221-303), on this
// work set. `seedOptional`: the stage-level API starts a level without the level above's disparity.
int frame_level_begin(derp_ctx* c, int level, LevelUse use, bool seedOptional = false) {
  TRY(check_level_runs(c, level));
  c->cur = level;
  const int W = c->LW[level], H = c->LH[level];
  const size_t n = (size_t)W * H;
  TRY(compute_fov_and_masks(c, level, use));
  {
    // the variance and the own colour bias come from one pass over the colour plane: the pass reports under `variance`,
    // and `own_bias` reads 0
    Span sp(c, ST_VARIANCE, level);
    hipLaunchKernelGGL(k_variance_bias, blur_grid(W, H, c->S), kBlurBlk, 0, c->stream, c->frame().color[level].as<ushort4>(),
                       W, H, c->w.srcVar.as<float>(), c->w.ownBias.as<ushort4>());
    KCHECK(c);
  }
  // fresh PyramidLevel: disparity / cost / confidence start at 0 (PyramidLevel.h:209-221)
  HIPCHK(c, hipMemsetAsync(c->w.cost.p, 0, n * c->D * sizeof(float), c->stream));
  HIPCHK(c, hipMemsetAsync(c->w.confidence.p, 0, n * c->D * sizeof(float), c->stream));
  // the mismatch mask is written by run_mismatches alone, under this condition: a level without the stage holds none
  // (derp_download_mismatch_mask then answers zeros) and needs no clear
  c->w.mismatchMaskHeld = level <= c->opt.mismatches_start_level && level != c->numLevels - 1;
  if (c->w.mismatchMaskHeld) {
    HIPCHK(c, hipMemsetAsync(c->w.mismatchMask.p, 0, n * c->D, c->stream));
  }
  if (level < c->numLevels - 1 && !c->frame().haveDisp[level + 1] && !seedOptional) {
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
  // this work set's own colour tables, at the plan's batch
  const size_t tables = (size_t)c->plan.DB * (c->S - 1);
  ALLOC(c, c->w.projColor, tables * (W + 2 * kPadC) * (H + 2 * kPadC) * sizeof(ushort4));
  ALLOC(c, c->w.projBias, tables * (W + 2 * kPadC) * (H + 2 * kPadC) * sizeof(ushort4));
  if (DERP_RANDOM_TILED) {
    ALLOC(c, c->w.projColorT, tables * tiled_plane(W, H) * sizeof(ushort4));
  }
  c->tablesValid = false;
  c->randomRanThisLevel = false;
  return 0;
}

int level_end(derp_ctx* c) {
  const int L = c->cur;
  HIPCHK(c, hipMemcpyAsync(c->frame().disp[L].p, c->w.disparity.p, npx(c, L) * c->D * sizeof(float),
                           hipMemcpyDeviceToDevice, c->stream));
  c->frame().haveDisp[L] = 1;
  return 0;
}

// A work lane's frame, whose kernels overlap other frames', may only Join, and only a level that the first frame of the
// pass left complete: then nothing process_level reaches asks for free memory, grows a shared buffer or builds warps.
int check_lane_join(derp_ctx* c, int level, LevelUse use) {
  const LevelPlan& p = c->plan;
  if (use != LevelUse::Join || p.level != level || p.DB != c->D || c->warpCachedLevel != level || c->fovCachedLevel != level) {
    return fail(c, "work lanes need every destination's tables in one batch (level %d: %d of %d)", level,
                p.level == level ? p.DB : 0, c->D);
  }
  return 0;
}

// processLevel of the selected frame. In turn on the context's own work set, a Join whose plan is not for this level
// (something else used the context in between) opens the level itself; on a lane check_lane_join has passed
// (process_level_on_lane).
int process_level(derp_ctx* c, int level, LevelUse use) {
  if (use == LevelUse::Join && c->plan.level != level) {
    use = LevelUse::Open;
  }
  if (use == LevelUse::Open) {
    TRY(level_open(c, level));
  }
  TRY(frame_level_begin(c, level, use));
  const int DB = c->plan.DB;
  for (int d0 = 0; d0 < c->D; d0 += DB) {
    const int nd = std::min(DB, c->D - d0);
    const bool single = (DB == c->D);
    if (!single || rebuilds_tables(c, use) || c->warpCachedLevel != level) {
      TRY(build_warp(c, d0, nd));
      c->warpCachedLevel = single ? level : -1;
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
  // the last stage writes the frame's level itself: no copy of the working disparity at the end (level_end)
  float* levelOut = c->frame().disp[level].as<float>();
  if (c->opt.do_median_filter) {
    TRY(run_median(c, true, levelOut));
  } else {
    TRY(run_mask_fov(c, levelOut));
  }
  c->frame().haveDisp[level] = 1;
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
  ALLOC(c, w.maskAnd, n * c->D);
  for (DevBuf* b : {&w.disparity, &w.cost, &w.confidence, &w.dispRes, &w.costRes, &w.tmpF, &w.rank}) {
    ALLOC(c, *b, n * c->D * sizeof(float));
  }
  ALLOC(c, w.changed, 2 * n * c->D);  // ping-pong's `changed` of the iteration before and of this one
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
// stream first waits for c->laneReady; a frame that may not join is refused before anything is enqueued there.
int process_level_on_lane(derp_ctx* c, int i, int slot, int level, LevelUse use) {
  if (i < 0) {
    TRY(select_frame(c, slot));
    return process_level(c, level, use);
  }
  TRY(check_lane_join(c, level, use));
  HIPCHK(c, hipStreamWaitEvent(c->lanes[i]->stream, c->laneReady, 0));
  lane_swap(c, i);
  c->activeLane = i;
  int rc = select_frame(c, slot);
  if (!rc) {
    rc = process_level(c, level, use);
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
      // the form the parameters allow: the same bits either way
      const bool fast = temporal_fast_tap_ok(sigma, w0, w1, w2) && !c->temporalGeneric;
      const auto kernel = !fast ? k_temporal_tiled<-1, false> : radius == 1 ? k_temporal_tiled<1, true> : k_temporal_tiled<-1, true>;
      hipLaunchKernelGGL(kernel, grid2d(W, H, planes, kBlk2d), kBlk2d, lds, c->stream, F, W, H, sigma, radius, w0, w1, w2, out,
                         dst2src);
    } else {
      hipLaunchKernelGGL(k_temporal, grid2d(W, H, planes, kBlk2d), kBlk2d, 0, c->stream, F, W, H, sigma, radius, w0, w1, w2,
                         out, dst2src);
    }
    KCHECK(c);
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

int derp_create(derp_ctx** out, int device, const derp_camera_desc* src, int n_src, const derp_camera_desc* dst,
                int n_dst) {
  if (!out) {
    return 1;
  }
  *out = nullptr;
  std::unique_ptr<derp_ctx> owner(new derp_ctx);  // until success: an early return frees what was allocated so far
  derp_ctx* c = owner.get();
  derp_options_default(&c->opt);
  if (n_src <= 0 || n_dst <= 0) {
    return create_fail("no source / destination cameras!");
  }
  hipDeviceProp_t prop;
  TRY(open_device(device, "the depth path", &prop));
  c->device = device;
  if (prop.maxSharedMemoryPerMultiProcessor > 0) {
    c->ldsPerCu = prop.maxSharedMemoryPerMultiProcessor;
  }
  if (const char* e = getenv("DERP_XCD_ROTATE")) {
    c->xcdRotate = atoi(e);
  }
  if (const char* e = getenv("DERP_XCD_BANDS")) {
    c->xcdBands = atoi(e);
  }
  if (const char* e = getenv("DERP_COST_TILES_PER_BLOCK")) {
    c->costTilesPerBlock = atoi(e);
  }
  c->noMemo = getenv("DERP_NO_MEMO") != nullptr;
  if (const char* e = getenv("DERP_BRUTE_RUN")) {
    c->bruteRun = atoi(e);
  }
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
  if (const char* e = getenv("DERP_TEMPORAL_GENERIC")) {
    c->temporalGeneric = atoi(e) != 0;
  }
  if (const char* e = getenv("DERP_REPROJECT_SERIAL")) {
    c->reprojectSerial = atoi(e) != 0;
  }
  c->S = n_src;
  c->D = n_dst;
  c->frames.resize(1);
  c->camsSrcH.resize(n_src);
  c->camsDstH.resize(n_dst);
  for (int i = 0; i < n_src; ++i) {
    if (const char* m = host_prepare_camera(src[i], c->camsSrcH[i])) {
      return create_fail(std::string("camera ") + src[i].id + ": " + m);
    }
  }
  c->dst2srcH.assign(n_dst, 0);
  c->descDstH.assign(dst, dst + n_dst);
  for (int i = 0; i < n_dst; ++i) {
    if (const char* m = host_prepare_camera(dst[i], c->camsDstH[i])) {
      return create_fail(std::string("camera ") + dst[i].id + ": " + m);
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
      return create_fail(std::string("destination camera ") + dst[i].id + " is not a source camera");
    }
    // The reference's destinations ARE rig cameras (filterDestinations, Derp.cpp:42-70, keeps a subset of the rig), and
    // k_reproject_bias relies on it: projWarpInv(d, s) is read from projWarp(ds, own) when s is destination ds. A
    // descriptor that shares an id with a source but not its intrinsics / pose would silently warp with the wrong camera.
    if (memcmp(&c->camsDstH[i], &c->camsSrcH[c->dst2srcH[i]], sizeof(Cam)) != 0) {
      return create_fail(std::string("destination camera ") + dst[i].id + " differs from the source camera of the same id "
                  "(destinations must be cameras of the source rig, as filterDestinations makes them)");
    }
  }
  if (c->camsSrc.ensure(sizeof(Cam) * n_src) || c->camsDst.ensure(sizeof(Cam) * n_dst) ||
      c->dst2src.ensure(sizeof(int) * n_dst) || c->counters.ensure(sizeof(unsigned long long) * ST_COUNT * kMaxLevels * 4)) {
    return create_fail("out of device memory");
  }
  // the streams last: they are torn down by derp_destroy alone, and nothing after them fails
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    return create_fail("hipStreamCreate failed");
  }
  if (hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    return create_fail("hipStreamCreate failed");
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
  // the cost kernels round tap positions with a form that holds below 2^23 (round_half_away_pos: a padded side below 2^22
  // leaves room to spare). No other check bounds a single side.
  for (int l = 0; l < num_levels; ++l) {
    if (widths[l] >= (1 << 22) || heights[l] >= (1 << 22)) {
      return fail(c, "level %d is too large (%dx%d, a side may be 4194303 at most)", l, widths[l], heights[l]);
    }
  }
  // a sequence sized its halo, filter and mask buffers for the geometry it was made under and indexes the frame slots
  // this call drops: with one open, nothing changes
  if (!c->openSeqs.empty()) {
    return fail(c, "derp_set_pyramid: %s is still open on this context (%d open; derp_seq_destroy first)",
                c->openSeqs.back().second.c_str(), (int)c->openSeqs.size());
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->numLevels = num_levels;
  c->widthFull = width_full;
  c->heightFull = height_full;
  c->LW.assign(widths, widths + num_levels);
  c->LH.assign(heights, heights + num_levels);
  ++c->warpGeneration;  // no work set's colour tables or tile flags, on the context or on a lane, fit this geometry
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
  ALLOC(c, c->fovMask, nmax * c->D);
  c->cur = -1;
  c->plan.level = -1;
  c->warpCachedLevel = -1;
  c->fovCachedLevel = -1;
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
  return use_device(c);
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
  return 0;  // (colour does not affect the warp tables: nothing to invalidate)
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
  TRY(use_device(c));
  return process_level(c, level, LevelUse::Open);
}

int derp_process_pyramid(derp_ctx* c, int level_start, int level_end_) {
  TRY(use_device(c));
  if (level_start < level_end_) {
    return fail(c, "Check failed: level_start >= level_end (%d vs %d)", level_start, level_end_);
  }
  for (int level = level_start; level >= level_end_; --level) {
    TRY(process_level(c, level, LevelUse::Open));
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
  const size_t n = npx(c, level);
  return download_sync(c, disparity, c->frame().disp[level].as<float>() + (size_t)d * n, n * sizeof(float));
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
  TRY(use_device(c));
  TRY(level_open(c, level));
  TRY(frame_level_begin(c, level, LevelUse::Open, true));
  if (c->plan.DB < c->D) {
    return fail(c, "stage-level API needs all destinations' tables resident (batch %d < %d)", c->plan.DB, c->D);
  }
  if (c->opt.rebuild_warp_tables || c->warpCachedLevel != level) {
    TRY(build_warp(c, 0, c->D));
    c->warpCachedLevel = level;
  }
  return 0;
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
  return download_sync(c, disp, c->w.disparity.as<float>() + (size_t)d * n, n * sizeof(float));
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
  return download_sync(c, bgr, c->w.staging.p, n * 6);
}
int derp_download_level_mask(derp_ctx* c, int level, int src, uint8_t* mask) {
  TRY(check_level(c, level));
  if (src < 0 || src >= c->S || !mask) {
    return fail(c, "bad source index / null output");
  }
  const size_t n = npx(c, level);
  return download_sync(c, mask, c->frame().fg[level].as<uint8_t>() + (size_t)src * n, n);
}
int derp_download_level_background(derp_ctx* c, int level, int dst, float* disp) {
  TRY(check_level(c, level));
  if (dst < 0 || dst >= c->D || !disp) {
    return fail(c, "bad destination index / null output");
  }
  const size_t n = npx(c, level);
  return download_sync(c, disp, c->frame().bg[level].as<float>() + (size_t)dst * n, n * 4);
}
int derp_download_mismatch_mask(derp_ctx* c, int d, uint8_t* out) {
  TRY(need_current(c, false));
  if (d < 0 || d >= c->D || !out) {
    return fail(c, "bad destination index / null output");
  }
  const size_t n = npx(c, c->cur);
  if (!c->w.mismatchMaskHeld) {  // no mismatch stage at this level: nothing was flagged (frame_level_begin)
    memset(out, 0, n);
    return 0;
  }
  return download_sync(c, out, c->w.mismatchMask.as<uint8_t>() + (size_t)d * n, n);
}

}  // extern "C"

#include "derp_render_api.h"
#include "derp_rephoto_api.h"
#include "derp_points_api.h"
#include "derp_stream_api.h"
#include "derp_mesh_api.h"
#include "derp_geometric_api.h"
#include "derp_sweep_api.h"
#include "derp_coverage_api.h"
#include "derp_align_api.h"
#include "derp_filters_api.h"
#include "derp_preview_api.h"
#include "derp_debug_api.h"
#include "derp_sequence.h"
#include "derp_isp.h"
#include "derp_sim.h"

// here every family's state is a complete type: the context's unique_ptr members can be created and destroyed
derp_ctx::derp_ctx() = default;
derp_ctx::~derp_ctx() = default;
