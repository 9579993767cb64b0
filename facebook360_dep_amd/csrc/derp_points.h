// Kernels of the conversion tools at the depth stage's inputs and outputs: ExportPointCloud (disparity + colour ->
// coloured points), ImportPointCloud (points -> per-camera disparity images), ProjectEquirectsToCameras (equirect
// mask -> camera mask). All three work on Camera::rescale of the UN-normalised rig camera (Camera.cpp:217-223), so
// the scaled principal / focal / resolution arrive from the host (ScaledCam), computed in the reference's order.
#pragma once
#include "derp_camera.h"

namespace derp {

// Camera::rescale(newResolution) of a rig camera: principal and focal in pixels of the new size
struct ScaledCam {
  double prx, pry, fx, fy, resx, resy;
};

constexpr int kPointsBlock = 256;  // threads per block of every kernel here (four waves)

// squaredNorm / norm of a 3-vector with Eigen's unrolled association (derp_camera.h: a0 + (a1 + a2))
__device__ __forceinline__ double norm3(double x, double y, double z) {
  return sqrt(sum3(x * x, y * y, z * z));
}

// Which pixels ExportPointCloud --subsample=N keeps. The reference keeps a pixel when rand() % N == 0, with rand()
// called from racing pool threads (ExportPointCloud.cpp:98): not reproducible even there. Here: a counter-based hash
// (the murmur3 finaliser) of (camera index, pixel index), kept when hash % N == 0 — the same pixels on every run.
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
__host__ __device__ __forceinline__ bool subsample_keeps(uint32_t cam, uint32_t pixel, uint32_t subsample) {
  return mix32(pixel ^ mix32(cam + 0x9e3779b9u)) % subsample == 0;
}

// ---- ExportPointCloud.cpp:67-137 (getPoints) --------------------------------------------------------------------
// Pass 1, one thread per pixel: the point of every pixel into six planes (coalesced stores), its keep flag, and the
// number of kept pixels of each block. NaN and zero disparities fall through IEEE arithmetic as they do in the
// reference (NaN / inf coordinates, kept).
__global__ void __launch_bounds__(kPointsBlock)
    k_export_points(const Cam* __restrict__ cam, ScaledCam sc, uint32_t camIndex, const float* __restrict__ disparity,
                    const float* __restrict__ colorBgr, int W, int H, double maxDepth, int clip, uint32_t subsample,
                    float* __restrict__ planes, uint8_t* __restrict__ keep, uint32_t* __restrict__ blockCount) {
  __shared__ uint32_t waveCount[kPointsBlock / 64];
  const size_t n = (size_t)W * H;
  const size_t i = (size_t)blockIdx.x * kPointsBlock + threadIdx.x;
  bool kept = false;
  if (i < n) {
    const Cam& c = *cam;
    const int x = (int)(i % W), y = (int)(i / W);
    const double px = x + 0.5, py = y + 0.5;
    kept = (subsample <= 1 || subsample_keeps(camIndex, (uint32_t)i, subsample)) &&
           !outside_image_circle(c, px, py, sc.prx, sc.pry, sc.fx, sc.fy);
    if (kept) {
      // `const double m = 1 / disparity(y, x)` (:108) on a Mat_<float>: int / float, a single-precision division
      // whose quotient is then widened
      const double m = (double)(1.0f / disparity[i]);
      const D3 dir = rig_direction(c, px, py, sc.prx, sc.pry, sc.fx, sc.fy);
      // Ray::pointAt: origin + direction * t
      double wx = c.pos[0] + dir.x * m, wy = c.pos[1] + dir.y * m, wz = c.pos[2] + dir.z * m;
      const double depth = norm3(wx, wy, wz);
      if (depth > maxDepth) {
        if (clip) {
          kept = false;
        } else {
          const double s = maxDepth / depth;
          wx *= s;
          wy *= s;
          wz *= s;
        }
      }
      if (kept) {
        planes[i] = (float)wx;
        planes[n + i] = (float)wy;
        planes[2 * n + i] = (float)wz;
        planes[3 * n + i] = colorBgr[3 * i + 2];
        planes[4 * n + i] = colorBgr[3 * i + 1];
        planes[5 * n + i] = colorBgr[3 * i];
      }
    }
    keep[i] = kept;
  }
  const unsigned long long ballot = __ballot(kept);
  if ((threadIdx.x & 63) == 0) {
    waveCount[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    for (int w = 0; w < kPointsBlock / 64; ++w) {
      total += waveCount[w];
    }
    blockCount[blockIdx.x] = total;
  }
}

// Pass 2, one block: exclusive scan of the block counts in place; total[0] = the number of points. 64-bit sums: a
// frame of more than 2^32 pixels is not a case, but the running offset is a size.
__global__ void __launch_bounds__(1024) k_scan_block_counts(const uint32_t* __restrict__ counts, int nBlocks,
                                                            unsigned long long* __restrict__ offsets,
                                                            unsigned long long* __restrict__ total) {
  __shared__ unsigned long long part[1024];
  const int t = threadIdx.x;
  const int per = (nBlocks + 1023) / 1024;
  const int b0 = min(t * per, nBlocks), b1 = min(b0 + per, nBlocks);
  unsigned long long sum = 0;
  for (int b = b0; b < b1; ++b) {
    sum += counts[b];
  }
  part[t] = sum;
  __syncthreads();
  for (int step = 1; step < 1024; step <<= 1) {  // Hillis-Steele, inclusive
    const unsigned long long v = t >= step ? part[t - step] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = part[t] - sum;
  for (int b = b0; b < b1; ++b) {
    offsets[b] = run;
    run += counts[b];
  }
  if (t == 1023) {
    total[0] = part[t];
  }
}

// Pass 3: the kept pixels of a block, in pixel order, are one contiguous run of 24-byte points in the output. They are
// gathered into LDS in that order (rank = kept pixels before this one: per-wave ballot + popcount + the waves before)
// and written out as consecutive floats, so that a wave stores whole lines whatever the survivors' pattern.
__global__ void __launch_bounds__(kPointsBlock)
    k_export_scatter(const float* __restrict__ planes, const uint8_t* __restrict__ keep, size_t n,
                     const unsigned long long* __restrict__ offsets, float* __restrict__ out) {
  __shared__ uint32_t waveCount[kPointsBlock / 64];
  __shared__ float stage[kPointsBlock * 6];
  const size_t i = (size_t)blockIdx.x * kPointsBlock + threadIdx.x;
  const bool kept = i < n && keep[i];
  const unsigned long long ballot = __ballot(kept);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    waveCount[wave] = (uint32_t)__popcll(ballot);
  }
  __syncthreads();
  uint32_t rank = (uint32_t)__popcll(ballot & ((1ull << lane) - 1)), total = 0;
  for (int w = 0; w < kPointsBlock / 64; ++w) {
    rank += w < wave ? waveCount[w] : 0;
    total += waveCount[w];
  }
  if (kept) {
    for (int k = 0; k < 6; ++k) {
      stage[rank * 6 + k] = planes[(size_t)k * n + i];
    }
  }
  __syncthreads();
  float* dst = out + offsets[blockIdx.x] * 6;
  for (uint32_t k = threadIdx.x; k < total * 6; k += kPointsBlock) {
    dst[k] = stage[k];
  }
}

// ---- ImportPointCloud.cpp:76-123 (projectPointsToCameras) -------------------------------------------------------
struct PointsImage {  // one camera's disparity image inside the shared buffer
  ScaledCam sc;
  unsigned long long offset;  // in floats
  int32_t w, h;
};

// One thread per point, every camera in turn. The points are rows of three doubles: a block reads its 768 doubles
// as consecutive words into LDS and each thread picks its row there. A candidate 1 / depth is a non-negative float or
// +inf, whose bit pattern orders like its value: one device-scope atomicMax on the unsigned view, independent of the
// order of arrival and so bit-reproducible. Zero candidates (depth outside [min, max] -> inf) cannot raise an image
// that starts at zero and NaN never wins std::max(old, NaN): neither is sent.
__global__ void __launch_bounds__(kPointsBlock)
    k_points_splat(const Cam* __restrict__ cams, const PointsImage* __restrict__ images, int nCams,
                   const double* __restrict__ xyz, size_t n, double minDepth, double maxDepth,
                   float* __restrict__ disparity) {
  __shared__ double rows[kPointsBlock * 3];
  const size_t first = (size_t)blockIdx.x * kPointsBlock;
  const size_t words = min((size_t)kPointsBlock, n - first) * 3;
  for (size_t k = threadIdx.x; k < words; k += kPointsBlock) {
    rows[k] = xyz[first * 3 + k];
  }
  __syncthreads();
  if (first + threadIdx.x >= n) {
    return;
  }
  const D3 p = {rows[threadIdx.x * 3], rows[threadIdx.x * 3 + 1], rows[threadIdx.x * 3 + 2]};
  // the distance from the RIG ORIGIN, not from the camera (reference quirk, :110), rounded to float
  float depth = (float)norm3(p.x, p.y, p.z);
  if ((double)depth < minDepth || (double)depth > maxDepth) {
    depth = INFINITY;
  }
  const float candidate = 1.0f / depth;
  if (!(candidate > 0.0f)) {  // zero or NaN
    return;
  }
  for (int ci = 0; ci < nCams; ++ci) {
    const PointsImage& im = images[ci];
    D2 pix;
    if (!sees<0>(cams[ci], p, im.sc.prx, im.sc.pry, im.sc.fx, im.sc.fy, im.sc.resx, im.sc.resy, pix)) {
      continue;
    }
    // std::round (half away from zero), then clamp: reference quirk (:108-109), not floor
    const int xs = min(max((int)round(pix.x), 0), im.w - 1);
    const int ys = min(max((int)round(pix.y), 0), im.h - 1);
    atomicMax(reinterpret_cast<unsigned*>(disparity + im.offset) + (size_t)ys * im.w + xs, __float_as_uint(candidate));
  }
}

// ---- ProjectEquirectsToCameras.cpp:94-125 -----------------------------------------------------------------------
// image_util::worldToEquirect (ImageUtil.cpp:127-140) with its float roundings as written. acos / atan2: evaluated
// in fp64 on the float arguments and rounded to float (the reference's unqualified calls may bind to either overload;
// a correctly rounded result is what both give up to libm's last ulp — implementation-defined).
__device__ __forceinline__ D2 world_to_equirect(double wx, double wy, double wz, int eqrW, int eqrH) {
  const float depth = (float)norm3(wx, wy, wz);
  const float x = (float)(wx / (double)depth);
  const float y = (float)(wy / (double)depth);
  const float z = (float)(wz / (double)depth);
  const float phi = (float)acos((double)z);
  float theta = (float)atan2((double)y, (double)x);
  if (theta > 0) {
    theta = (float)((double)theta - 2 * M_PI);
  }
  const float v = (float)((double)phi / M_PI);
  const float u = (float)((double)-theta / (2.0f * M_PI));
  return {(double)(u * (float)eqrW), (double)(v * (float)eqrH)};
}

__global__ void __launch_bounds__(kPointsBlock)
    k_project_equirect_mask(const Cam* __restrict__ cam, ScaledCam sc, const uint8_t* __restrict__ eqr, int eqrW,
                            int eqrH, int W, int H, double depth, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kPointsBlock + threadIdx.x;
  if (i >= (size_t)W * H) {
    return;
  }
  const Cam& c = *cam;
  const int x = (int)(i % W), y = (int)(i / W);
  const D3 dir = rig_direction(c, x + 0.5, y + 0.5, sc.prx, sc.pry, sc.fx, sc.fy);
  const D2 e = world_to_equirect(c.pos[0] + dir.x * depth, c.pos[1] + dir.y * depth, c.pos[2] + dir.z * depth, eqrW, eqrH);
  uint8_t m = 0;
  if (!(e.x < 0 || e.y < 0 || e.x >= eqrW || e.y >= eqrH) && e.x == e.x && e.y == e.y) {
    m = eqr[(size_t)(int)e.y * eqrW + (int)e.x] != 0;  // rounding can put us at the image edge: ignored (:113-116)
  }
  out[i] = m;
}

}  // namespace derp
