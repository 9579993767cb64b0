// RigAnalyzer (source/rig/RigAnalyzer.cpp), device side: how many cameras of the rig see each point of a point set, and
// for the equirect the smallest rolling-shutter timing distance between two cameras that see a pixel. One kernel family,
// k_coverage<GEN, TIMING>: a thread owns one point and walks every camera of the context; the camera index is the same
// in every lane, so Cam and ScaledCam arrive through scalar loads. Each camera is asked with sees<0>, the reference's
// expression (Camera.h:184-190), in the camera's own pixel units. Definitions: DESIGN §8.9. Host side: derp_coverage_api.h.
#pragma once
#include "derp_camera.h"
#include "derp_points.h"

namespace derp {

enum { kCovDirections = 0, kCovEquirect = 1, kCovCamera = 2, kCovPlane = 3 };
constexpr int kCovBlock = 256;       // threads per block of the counting kernels (four waves)
constexpr int kCovTimingBlock = 64;  // ... of the timing kernel: one wave, so that 255 cameras' list still fits 64 KB of LDS
constexpr int kCovMaxCams = 255;     // counts are u8
constexpr int kCovHistBins = kCovMaxCams + 1;

struct CovPoints {  // what the generators read; only the selected generator's fields are set
  // (a) unit vectors [n][3] and distances [gridDim.y]
  const double* units;
  const double* distances;
  // (b) [w] cos lon, [w] sin lon, [h] cos lat, [h] sin lat from the host's libm; (b), (c) the distance
  const double *cosLon, *sinLon, *cosLat, *sinLat;
  double distance;
  // (b), (c) image width; (d) dim
  int w;
  // (c) the camera whose pixels are the points
  int cam;
};

// The point of index i (and of distance blockIdx.y for the directions); false: the reference counts 0 without asking
template <int GEN>
__device__ __forceinline__ bool coverage_point(const CovPoints& P, const Cam* __restrict__ cams,
                                               const ScaledCam* __restrict__ scs, size_t i, D3& p) {
  if (GEN == kCovDirections) {
    // distance * samples[j] (RigAnalyzer.cpp:572)
    const double d = P.distances[blockIdx.y];
    p = {d * P.units[3 * i], d * P.units[3 * i + 1], d * P.units[3 * i + 2]};
    return true;
  } else if (GEN == kCovEquirect) {
    // direction(cos(lat) * cos(lon), cos(lat) * sin(lon), sin(lat)) * overlap_distance (:393-402)
    const int x = (int)(i % P.w), y = (int)(i / P.w);
    const double cl = P.cosLat[y];
    p = {cl * P.cosLon[x] * P.distance, cl * P.sinLon[x] * P.distance, P.sinLat[y] * P.distance};
    return true;
  } else if (GEN == kCovCamera) {
    // p(x + 0.5, y + 0.5); isOutsideImageCircle; cam.rig(p, distance) = position + direction * distance (:359-362)
    const int x = (int)(i % P.w), y = (int)(i / P.w);
    const Cam& c = cams[P.cam];
    const ScaledCam& sc = scs[P.cam];
    const double px = x + 0.5, py = y + 0.5;
    if (outside_image_circle(c, px, py, sc.prx, sc.pry, sc.fx, sc.fy)) {
      return false;
    }
    const D3 dir = rig_direction(c, px, py, sc.prx, sc.pry, sc.fx, sc.fy);
    p = {c.pos[0] + dir.x * P.distance, c.pos[1] + dir.y * P.distance, c.pos[2] + dir.z * P.distance};
    return true;
  } else {
    // point(x + 0.5 - 0.5 * kDim, y + 0.5 - 0.5 * kDim, 0) (:449)
    const int x = (int)(i % P.w), y = (int)(i / P.w);
    p = {x + 0.5 - 0.5 * P.w, y + 0.5 - 0.5 * P.w, 0.0};
    return true;
  }
}

// counts [gridDim.y][n] u8 (null: not wanted; the directions only). hist [gridDim.y][nCams + 1] int32, zeroed by the
// caller (the directions only, else null): a block counts into LDS and adds each of its non-empty bins once; integer
// addition, so the order of the blocks does not show. minTiming [n] f32 (TIMING only).
// TIMING: the list of timings of the cameras that see the point, at most nCams floats, lies in dynamic LDS
// (nCams * kCovTimingBlock floats, entry k of lane l at [k * kCovTimingBlock + l]), not in registers or scratch.
template <int GEN, bool TIMING>
__global__ void __launch_bounds__(TIMING ? kCovTimingBlock : kCovBlock)
    k_coverage(const Cam* __restrict__ cams, const ScaledCam* __restrict__ scs, int nCams, CovPoints P, size_t n,
               uint8_t* __restrict__ counts, int* __restrict__ hist, float* __restrict__ minTiming) {
  constexpr int kBlock = TIMING ? kCovTimingBlock : kCovBlock;
  extern __shared__ float covTimings[];
  __shared__ int bins[GEN == kCovDirections ? kCovHistBins : 1];
  if (GEN == kCovDirections) {
    for (int b = threadIdx.x; b < kCovHistBins; b += kBlock) {
      bins[b] = 0;
    }
    __syncthreads();
  }
  const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const bool active = i < n;
  int count = 0;
  D3 p = {0, 0, 0};
  if (active && coverage_point<GEN>(P, cams, scs, i, p)) {
    for (int k = 0; k < nCams; ++k) {
      const ScaledCam& sc = scs[k];
      D2 pix;
      if (sees<0>(cams[k], p, sc.prx, sc.pry, sc.fx, sc.fy, sc.resx, sc.resy, pix)) {
        if (TIMING) {
          // timing[count] = p.y() / camera.resolution.y(), a float (:406)
          covTimings[count * kBlock + threadIdx.x] = (float)(pix.y / sc.resy);
        }
        ++count;
      }
    }
  }
  if (active) {
    if (counts) {
      counts[(size_t)blockIdx.y * n + i] = (uint8_t)count;
    }
    if (TIMING) {
      // the minimum over pairs of |timing[i] - timing[j]|, taken in float as the reference takes it (:411-417); 1.0 where
      // fewer than two cameras see the pixel. (The differences are floats, so the reference's min in double is this one.)
      float best = 1.0f;
      for (int a = 0; a < count; ++a) {
        const float ta = covTimings[a * kBlock + threadIdx.x];
        for (int b = a + 1; b < count; ++b) {
          best = fminf(best, fabsf(ta - covTimings[b * kBlock + threadIdx.x]));
        }
      }
      minTiming[i] = best;
    }
  }
  if (GEN == kCovDirections) {
    if (active) {
      atomicAdd(&bins[count], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b <= nCams; b += kBlock) {
      if (bins[b] != 0) {
        atomicAdd(&hist[(size_t)blockIdx.y * (nCams + 1) + b], bins[b]);
      }
    }
  }
}

}  // namespace derp
