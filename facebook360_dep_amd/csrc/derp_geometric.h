// Kernels of GeometricConsistency (source/render/GeometricConsistency.cpp): the plane sweep over uniformly spaced
// disparities (computeDepth + winnerTakesAll, :132-258) and the cross-camera cleaning (cleanDepth / isPointBad,
// :260-310). The reference's OpenGL reprojection is replaced by the sampling rule of DESIGN §8.6; everything after it is
// the reference's integer / fp32 arithmetic. The cameras are Camera::rescale of the un-normalised rig cameras
// (ScaledCam, derp_points.h). The int16 images come from k_resize_area<4> (derp_kernels.h).
#pragma once
#include "derp_kernels.h"
#include "derp_points.h"

namespace derp {

struct GcCam {  // one camera's small image inside the shared buffers (int16 colour, clean depth)
  ScaledCam sc;
  unsigned long long offset;  // in pixels
  int32_t w, h;
};

constexpr int kGcSide = 16;               // samples per tile side: one lane each (256 lanes, four waves)
constexpr int kGcTile = kGcSide - 2;      // destination pixels per tile side: the samples less the halo of the 3 x 3 box
constexpr int kGcBlock = kGcSide * kGcSide;
constexpr int kGcMaxSplit = 64;  // parts of the slice range (grid z)

__device__ __forceinline__ int gc_sat16(int v) {
  return min(max(v, -32768), 32767);
}
// saturate_int16(rint(double(a) * double(a) * (1.0 / 32767))) in integers. a^2 / 32767 is never half way between two
// integers (that needs 2 a^2 = 32767 (2k + 1), even = odd) and is at least 1 / 65534 away from it, far beyond the 2^-52
// relative error of the fp64 product: round-to-nearest of the exact quotient is the same number.
__device__ __forceinline__ int gc_sq(int a) {
  const unsigned q = (2u * (unsigned)(a * a) + 32767u) / 65534u;
  return (int)min(q, 32767u);
}
// saturate_int16(rint(sum * (1.0 / 9))) of an int32 box sum in integers: sum / 9 is never half way either (9 is odd)
// and at least 1 / 18 away from it. Floor division of 2 sum + 9 by 18.
__device__ __forceinline__ int gc_blur9(int sum) {
  const int t = 2 * sum + 9;
  const int q = t >= 0 ? t / 18 : -((17 - t) / 18);
  return gc_sat16(q);
}

// The sample of source `s` where it sees `world`: bilinear in fp32 on the int16 image, texels outside the
// image (0, 0, 0, 0), every product and sum rounded on its own (-ffp-contract=off), round half to even. Then the
// occlusion test against the source's clean depth, nearest sample.
__device__ __forceinline__ short4 gc_sample(const Cam& cam, const GcCam& g, const short4* __restrict__ image,
                                            const float* __restrict__ clean, double agree, const D3& world) {
  D2 p;
  if (!sees<0>(cam, world, g.sc.prx, g.sc.pry, g.sc.fx, g.sc.fy, g.sc.resx, g.sc.resy, p)) {
    return make_short4(0, 0, 0, 0);
  }
  if (!(p.x == p.x && p.y == p.y)) {  // (a NaN pixel passes Camera::sees; no finite world point makes one)
    return make_short4(0, 0, 0, 0);
  }
  const double u = p.x - 0.5, v = p.y - 0.5;
  const double fu = floor(u), fv = floor(v);
  const int x0 = (int)fu, y0 = (int)fv;
  const float fx = (float)(u - fu), fy = (float)(v - fv);
  const short4* img = image + g.offset;
  const short4 zero = make_short4(0, 0, 0, 0);
  const bool xa = x0 >= 0, xb = x0 + 1 < g.w, ya = y0 >= 0, yb = y0 + 1 < g.h;
  const short4 t00 = xa && ya ? img[(size_t)y0 * g.w + x0] : zero;
  const short4 t10 = xb && ya ? img[(size_t)y0 * g.w + x0 + 1] : zero;
  const short4 t01 = xa && yb ? img[(size_t)(y0 + 1) * g.w + x0] : zero;
  const short4 t11 = xb && yb ? img[(size_t)(y0 + 1) * g.w + x0 + 1] : zero;
  const float ax = 1.0f - fx, ay = 1.0f - fy;
  const auto lerp = [&](short a, short b, short c, short d) {
    const float top = ax * (float)a + fx * (float)b;
    const float bottom = ax * (float)c + fx * (float)d;
    return (short)gc_sat16((int)rintf(ay * top + fy * bottom));
  };
  short4 r = make_short4(lerp(t00.x, t10.x, t01.x, t11.x), lerp(t00.y, t10.y, t01.y, t11.y),
                         lerp(t00.z, t10.z, t01.z, t11.z), lerp(t00.w, t10.w, t01.w, t11.w));
  if (clean) {
    // p lies in [0, res) (sees): the nearest sample is inside the image
    const float d = clean[g.offset + (size_t)(int)p.y * g.w + (int)p.x];
    if (d == d) {
      const double distance = norm3(world.x - cam.pos[0], world.y - cam.pos[1], world.z - cam.pos[2]);
      if ((double)d < distance * agree) {
        r.w = 0;
      }
    }
  }
  return r;
}

struct GcStageOut {  // STAGE: the intermediates of (stageSrc, the one slice swept) and the slice's cost plane
  short4* sample;
  short4* average;
  short4* averageOfSq;
  float* cost;
};

// The sweep. One workgroup owns a 14 x 14 tile of destination pixels plus its one-pixel halo: 16 x 16 samples, one per
// lane (an 18 x 18 tile would give 68 lanes a second sample and leave two of the four waves idle meanwhile). Per (slice,
// source) every lane projects and samples its position and leaves the four int16 differences in LDS; after one barrier
// the 196 inner lanes form their two 3 x 3 sums there. The LDS tile is double-buffered, so one barrier per (slice,
// source) does. A halo position beyond the image edge is the reflect-101 mirror, i.e. the sample of the mirrored pixel:
// it is computed at that pixel's coordinates (the same bits as a copy, and no second barrier). Positions further out
// feed no pixel of the image and stay idle. The lane's ray (unit direction) lives in registers across the whole sweep.
// grid (tilesX, tilesY, splits): part z sweeps slices [z * per, min((z + 1) * per, sliceCount)) and writes its running
// best (cost, slice) to plane z of bestCost / bestSlice; k_gc_reduce merges the parts.
template <bool STAGE>
__global__ void __launch_bounds__(kGcBlock)
    k_gc_sweep(const Cam* __restrict__ cams, const GcCam* __restrict__ gcams, int nCams, int dst,
               const short4* __restrict__ images, const float* __restrict__ clean, double agree,
               const float* __restrict__ slices, int sliceCount, int per, float* __restrict__ bestCost,
               int* __restrict__ bestSlice, int stageSrc, GcStageOut stage) {
  __shared__ short4 tile[2][kGcBlock];
  const GcCam gd = gcams[dst];
  const Cam& cd = cams[dst];
  const int W = gd.w, H = gd.h;
  const int tid = threadIdx.x;
  const int lx = tid % kGcSide, ly = tid / kGcSide;
  const int gx = blockIdx.x * kGcTile - 1 + lx, gy = blockIdx.y * kGcTile - 1 + ly;
  const bool live = gx <= W && gy <= H;  // (-1 and W are the mirrors of 1 and W - 2)
  // a pixel of the image whose 3 x 3 box lies in this tile
  const bool inside = lx >= 1 && lx <= kGcTile && ly >= 1 && ly <= kGcTile && gx < W && gy < H;
  D3 ray = {0, 0, 0};
  short4 ref = make_short4(0, 0, 0, 0);
  if (live) {
    const int mx = reflect101(gx, W), my = reflect101(gy, H);
    ray = rig_direction(cd, mx + 0.5, my + 0.5, gd.sc.prx, gd.sc.pry, gd.sc.fx, gd.sc.fy);
    ref = images[gd.offset + (size_t)my * W + mx];
  }
  const size_t o = inside ? (size_t)gy * W + gx : 0;

  const int s0 = STAGE ? per : blockIdx.z * per;  // STAGE: `per` is the one slice
  const int s1 = STAGE ? per + 1 : min(s0 + per, sliceCount);
  float best = FLT_MAX;
  int bestAt = -1;
  int buf = 0;
  for (int slice = s0; slice < s1; ++slice) {
    const double depth = 1.0 / (double)slices[slice];
    // Ray::pointAt: origin + direction * t
    const D3 world = {cd.pos[0] + ray.x * depth, cd.pos[1] + ray.y * depth, cd.pos[2] + ray.z * depth};
    float accum0 = 0.0f, accum1 = 0.0f;
    for (int s = 0; s < nCams; ++s) {
      if (s == dst) {
        continue;
      }
      short4 v = make_short4(0, 0, 0, 0), diff = v;
      if (live) {
        v = gc_sample(cams[s], gcams[s], images, clean, agree, world);
        diff = make_short4((short)gc_sat16(v.x - ref.x), (short)gc_sat16(v.y - ref.y), (short)gc_sat16(v.z - ref.z),
                           (short)gc_sat16(v.w - ref.w));
      }
      tile[buf][tid] = diff;
      __syncthreads();
      if (inside) {
        int sum[4] = {0, 0, 0, 0}, sumSq[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
#pragma unroll
          for (int i = -1; i <= 1; ++i) {
            const short4 d = tile[buf][tid + j * kGcSide + i];
            sum[0] += d.x;
            sum[1] += d.y;
            sum[2] += d.z;
            sum[3] += d.w;
            sumSq[0] += gc_sq(d.x);
            sumSq[1] += gc_sq(d.y);
            sumSq[2] += gc_sq(d.z);
            if (STAGE) {
              sumSq[3] += gc_sq(d.w);
            }
          }
        }
        const int avg[4] = {gc_blur9(sum[0]), gc_blur9(sum[1]), gc_blur9(sum[2]), gc_blur9(sum[3])};
        const int avgSq[4] = {gc_blur9(sumSq[0]), gc_blur9(sumSq[1]), gc_blur9(sumSq[2]), STAGE ? gc_blur9(sumSq[3]) : 0};
        if (v.w == 32767 && avg[3] == 0) {
          // sumNorm(averageOfSq) - sumSqNorm(average), :110-124, fp32 as written there
          float a = 0.0f;
          a += (float)avgSq[0];
          a += (float)avgSq[1];
          a += (float)avgSq[2];
          float b = 0.0f;
          b += (float)avg[0] * (float)avg[0];
          b += (float)avg[1] * (float)avg[1];
          b += (float)avg[2] * (float)avg[2];
          accum0 += a / 32767.0f - b / (32767.0f * 32767.0f);
          accum1 += 1.0f;
        }
        if (STAGE && s == stageSrc) {
          stage.sample[o] = v;
          stage.average[o] = make_short4((short)avg[0], (short)avg[1], (short)avg[2], (short)avg[3]);
          stage.averageOfSq[o] = make_short4((short)avgSq[0], (short)avgSq[1], (short)avgSq[2], (short)avgSq[3]);
        }
      }
      buf ^= 1;
    }
    const float cost = accum0 / accum1;  // 0 / 0: NaN, which never wins
    if (best > cost) {
      best = cost;
      bestAt = slice;
    }
    if (STAGE && inside) {
      stage.cost[o] = cost;
    }
  }
  if (!STAGE && inside) {
    bestCost[(size_t)blockIdx.z * W * H + o] = best;
    bestSlice[(size_t)blockIdx.z * W * H + o] = bestAt;
  }
}

// winnerTakesAll (:132-156) over the parts: ascending slices, strict `best > cost` from FLT_MAX, so the first minimum
// wins whatever the split; depth = 1 / sliceDisparity in fp64, rounded to float; NaN where nothing won and on the
// outermost rows and columns.
__global__ void k_gc_reduce(const float* __restrict__ bestCost, const int* __restrict__ bestSlice, int splits,
                            const float* __restrict__ slices, int W, int H, float* __restrict__ depth) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= W || y >= H) {
    return;
  }
  const size_t n = (size_t)W * H, o = (size_t)y * W + x;
  float best = FLT_MAX;
  int at = -1;
  for (int z = 0; z < splits; ++z) {
    const float cost = bestCost[z * n + o];
    const int slice = bestSlice[z * n + o];
    if (slice >= 0 && best > cost) {
      best = cost;
      at = slice;
    }
  }
  float d = NAN;
  if (at >= 0 && x > 0 && y > 0 && x < W - 1 && y < H - 1) {
    d = (float)(1.0 / (double)slices[at]);
  }
  depth[o] = d;
}

// cleanDepth / isPointBad (:260-310): one lane per destination pixel, the sources in rig order. depths: every camera's
// map at its GcCam offset. A NaN depth makes a NaN point that no camera sees and stays NaN.
__global__ void __launch_bounds__(256)
    k_gc_clean(const Cam* __restrict__ cams, const GcCam* __restrict__ gcams, int nCams, int dst,
               const float* __restrict__ depths, double agree, float* __restrict__ out) {
  const GcCam gd = gcams[dst];
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)gd.w * gd.h) {
    return;
  }
  const Cam& cd = cams[dst];
  const int x = (int)(i % gd.w), y = (int)(i / gd.w);
  const float depth = depths[gd.offset + i];
  if (!(depth == depth)) {  // the reference indexes the sources' maps with a NaN pixel here (Camera::sees passes NaN)
    out[gd.offset + i] = depth;
    return;
  }
  const double m = (double)depth;
  const D3 dir = rig_direction(cd, x + 0.5, y + 0.5, gd.sc.prx, gd.sc.pry, gd.sc.fx, gd.sc.fy);
  const D3 world = {cd.pos[0] + dir.x * m, cd.pos[1] + dir.y * m, cd.pos[2] + dir.z * m};
  bool bad = false;
  for (int s = 0; s < nCams && !bad; ++s) {
    if (s == dst) {
      continue;
    }
    const Cam& cs = cams[s];
    const GcCam gs = gcams[s];
    D2 p;
    if (!sees<0>(cs, world, gs.sc.prx, gs.sc.pry, gs.sc.fx, gs.sc.fy, gs.sc.resx, gs.sc.resy, p)) {
      continue;
    }
    if (!(p.x == p.x && p.y == p.y)) {
      continue;
    }
    const float srcDepth = depths[gs.offset + (size_t)(int)p.y * gs.w + (int)p.x];
    const float proposal = (float)norm3(world.x - cs.pos[0], world.y - cs.pos[1], world.z - cs.pos[2]);
    bad = (double)proposal < (double)srcDepth * agree;
  }
  out[gd.offset + i] = bad ? NAN : depth;
}

// restoreCleanDepth (:312-322)
__global__ void k_gc_restore(const float* __restrict__ cleanDepth, float* __restrict__ depth, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = cleanDepth[i];
    if (v == v) {
      depth[i] = v;
    }
  }
}

}  // namespace derp
