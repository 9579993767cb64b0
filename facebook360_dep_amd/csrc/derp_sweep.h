// Kernels of the rig preview tools: GenerateCameraOverlaps (every camera projected into a destination camera over a
// series of depths) and GenerateEquirect (the same into one equirect of the whole rig). Both work on Camera::rescale of
// the UN-normalised rig camera to a resolution that need not be whole (resolution * scale), so a camera's resolution
// (ScaledCam, doubles) and its image's size (ints) are separate. Definitions: DESIGN §8.7.
#pragma once
#include "derp_points.h"

namespace derp {

struct SweepCam {  // one camera's float BGRA image inside the shared buffer
  ScaledCam sc;
  unsigned long long offset;  // in texels (float4)
  int32_t w, h;               // the image's own size: the clamp of every fetch
};

constexpr int kSweepBlock = 256;  // threads per block (four waves), one per pixel
constexpr int kSweepChunk = 16;   // cameras resident in LDS at a time (Cam + SweepCam: 264 bytes each)
constexpr int kSweepMaxSplit = 16;  // parts of the depth list (gridDim.z) at most: a run keeps its rays for several depths

enum { kSweepFloat = 0, kSweepU8 = 1 };

struct SweepLds {
  Cam cam[kSweepChunk];
  SweepCam im[kSweepChunk];
};

// the block's copy of cameras [c0, c0 + kSweepChunk) as words; every thread of the block calls it
__device__ __forceinline__ void sweep_load_chunk(SweepLds& L, const Cam* __restrict__ cams,
                                                 const SweepCam* __restrict__ ims, int c0, int nCams) {
  const int count = min(kSweepChunk, nCams - c0);
  const int camWords = count * (int)(sizeof(Cam) / 8), imWords = count * (int)(sizeof(SweepCam) / 8);
  const unsigned long long* srcCam = reinterpret_cast<const unsigned long long*>(cams + c0);
  const unsigned long long* srcIm = reinterpret_cast<const unsigned long long*>(ims + c0);
  unsigned long long* dstCam = reinterpret_cast<unsigned long long*>(L.cam);
  unsigned long long* dstIm = reinterpret_cast<unsigned long long*>(L.im);
  for (int k = threadIdx.x; k < camWords; k += kSweepBlock) {
    dstCam[k] = srcCam[k];
  }
  for (int k = threadIdx.x; k < imWords; k += kSweepBlock) {
    dstIm[k] = srcIm[k];
  }
}

// `255.0f * image` into an 8-bit file: float product, round half to even, saturate; NaN -> 0
__device__ __forceinline__ unsigned sweep_u8(float v) {
  const float r = rintf(v * 255.0f);
  return r != r ? 0u : (unsigned)fminf(fmaxf(r, 0.0f), 255.0f);
}

__device__ __forceinline__ void sweep_store(int outKind, void* __restrict__ out, size_t at, float4 v) {
  if (outKind == kSweepU8) {
    reinterpret_cast<uchar4*>(out)[at] =
        make_uchar4((unsigned char)sweep_u8(v.x), (unsigned char)sweep_u8(v.y), (unsigned char)sweep_u8(v.z),
                    (unsigned char)sweep_u8(v.w));
  } else {
    reinterpret_cast<float4*>(out)[at] = v;
  }
}

__device__ __forceinline__ float4 sweep_texel(const float4* __restrict__ image, int w, int h, int x, int y) {
  return image[(size_t)min(max(y, 0), h - 1) * w + min(max(x, 0), w - 1)];  // clampToEdge, CvUtil.h:78-81
}

// bilerp of CvUtil.h:83-86 on one channel, in its order
__device__ __forceinline__ float sweep_bilerp(float p00, float p01, float p10, float p11, float xw, float yw) {
  return (1 - xw) * (1 - yw) * p00 + xw * (1 - yw) * p01 + (1 - xw) * yw * p10 + xw * yw * p11;
}

// getPixelBilinear (CvUtil.h:107-120): float coordinates, std::round, clamp-to-edge taps
__device__ __forceinline__ float4 sweep_bilinear(const float4* __restrict__ image, int w, int h, float x, float y) {
  const float xf = roundf(x), yf = roundf(y);
  const int xi = (int)xf, yi = (int)yf;
  const float4 p00 = sweep_texel(image, w, h, xi - 1, yi - 1), p01 = sweep_texel(image, w, h, xi, yi - 1);
  const float4 p10 = sweep_texel(image, w, h, xi - 1, yi), p11 = sweep_texel(image, w, h, xi, yi);
  const float xw = x - xf + 0.5f, yw = y - yf + 0.5f;
  return make_float4(sweep_bilerp(p00.x, p01.x, p10.x, p11.x, xw, yw), sweep_bilerp(p00.y, p01.y, p10.y, p11.y, xw, yw),
                     sweep_bilerp(p00.z, p01.z, p10.z, p11.z, xw, yw), sweep_bilerp(p00.w, p01.w, p10.w, p11.w, xw, yw));
}

// ---- GenerateCameraOverlaps.cpp:54-83 (projectSrcsToDst) over a list of disparities ------------------------------
// One thread per destination pixel. The pixel's ray does not depend on the depth: image-circle test, Newton undistort
// and rotation happen once, then the thread walks its part of the disparity list (blockIdx.z). The cameras sit in LDS,
// kSweepChunk at a time; a rig that fits one chunk loads it once. The source loop is serial in camera order: the order
// of the fp32 sum is part of the result. out: [n][h][w] float4 or uchar4.
__global__ void __launch_bounds__(kSweepBlock)
    k_sweep_overlaps(const Cam* __restrict__ cams, const SweepCam* __restrict__ ims, int nCams, int dst,
                     const float4* __restrict__ images, const float* __restrict__ disparities, int nDisp, int perSplit,
                     int outKind, void* __restrict__ out) {
  __shared__ SweepLds L;
  const SweepCam me = ims[dst];
  const size_t n = (size_t)me.w * me.h;
  const size_t i = (size_t)blockIdx.x * kSweepBlock + threadIdx.x;
  const bool active = i < n;
  bool outside = true;
  D3 dir = {0, 0, 0}, pos = {0, 0, 0};
  if (active) {
    const Cam& c = cams[dst];
    const double px = (int)(i % me.w) + 0.5, py = (int)(i / me.w) + 0.5;
    outside = outside_image_circle(c, px, py, me.sc.prx, me.sc.pry, me.sc.fx, me.sc.fy);
    if (!outside) {
      dir = rig_direction(c, px, py, me.sc.prx, me.sc.pry, me.sc.fx, me.sc.fy);
      pos = {c.pos[0], c.pos[1], c.pos[2]};
    }
  }
  const int d0 = blockIdx.z * perSplit, d1 = min(d0 + perSplit, nDisp);
  const bool resident = nCams <= kSweepChunk;
  for (int d = d0; d < d1; ++d) {
    // `camDst.rig(dstPixel, 1.0f / disparity)` (:68): a float division whose quotient is widened; Ray::pointAt
    const double m = (double)(1.0f / disparities[d]);
    const D3 world = {pos.x + dir.x * m, pos.y + dir.y * m, pos.z + dir.z * m};
    float4 sum = make_float4(0, 0, 0, 0);
    int count = 0;
    for (int c0 = 0; c0 < nCams; c0 += kSweepChunk) {
      if (!resident || d == d0) {
        __syncthreads();  // (the chunk before this one is still being read)
        sweep_load_chunk(L, cams, ims, c0, nCams);
        __syncthreads();
      }
      if (outside) {
        continue;
      }
      const int c1 = min(kSweepChunk, nCams - c0);
      for (int k = 0; k < c1; ++k) {
        const SweepCam& im = L.im[k];
        D2 pix;
        if (sees<0>(L.cam[k], world, im.sc.prx, im.sc.pry, im.sc.fx, im.sc.fy, im.sc.resx, im.sc.resy, pix)) {
          const float4 v = sweep_bilinear(images + im.offset, im.w, im.h, (float)pix.x, (float)pix.y);
          sum.x += v.x;
          sum.y += v.y;
          sum.z += v.z;
          sum.w += v.w;
          ++count;
        }
      }
    }
    if (active) {
      float4 r = make_float4(0, 0, 0, 0);  // outside the image circle (:64-67)
      if (!outside) {
        const float s = 1.0f / (float)count;  // `1.0f / count * sum` (:78); count == 0: inf * 0 = NaN
        r = make_float4(s * sum.x, s * sum.y, s * sum.z, s * sum.w);
      }
      sweep_store(outKind, out, (size_t)d * n + i, r);
    }
  }
}

// ---- GenerateEquirect.cpp:79-175 ----------------------------------------------------------------------------------
// The window of an equirect call: the full equirect is W x H; the output is w x h; column x samples the angle of the
// host's table entry x (cropped or not, the host fills the tables), so one kernel serves both.
struct SweepEqr {
  const double* cosTheta;  // [w]
  const double* sinTheta;  // [w]
  const double* sinPhi;    // [h]
  const double* cosPhi;    // [h]
  int w, h;
};

// getEquirectPoint (:102-115) from the host's sines and cosines: products only, left to right
__device__ __forceinline__ D3 sweep_eqr_point(const SweepEqr& e, int x, int y, double depth) {
  const double ds = depth * e.sinPhi[y];
  return {ds * e.cosTheta[x], ds * e.sinTheta[x], depth * e.cosPhi[y]};
}

// getPixelColor (:79-100) over a list of depths. out: [n][h][w] float4 or uchar4.
__global__ void __launch_bounds__(kSweepBlock)
    k_sweep_equirect(const Cam* __restrict__ cams, const SweepCam* __restrict__ ims, int nCams,
                     const float4* __restrict__ images, SweepEqr e, const float* __restrict__ depths, int nDepths,
                     int perSplit, float4 background, int outKind, void* __restrict__ out) {
  __shared__ SweepLds L;
  const size_t n = (size_t)e.w * e.h;
  const size_t i = (size_t)blockIdx.x * kSweepBlock + threadIdx.x;
  const bool active = i < n;
  const int x = active ? (int)(i % e.w) : 0, y = active ? (int)(i / e.w) : 0;
  const int d0 = blockIdx.z * perSplit, d1 = min(d0 + perSplit, nDepths);
  const bool resident = nCams <= kSweepChunk;
  for (int d = d0; d < d1; ++d) {
    const D3 p = sweep_eqr_point(e, x, y, (double)depths[d]);
    float4 sum = make_float4(0, 0, 0, 0);
    int count = 0;
    for (int c0 = 0; c0 < nCams; c0 += kSweepChunk) {
      if (!resident || d == d0) {
        __syncthreads();
        sweep_load_chunk(L, cams, ims, c0, nCams);
        __syncthreads();
      }
      if (!active) {
        continue;
      }
      const int c1 = min(kSweepChunk, nCams - c0);
      for (int k = 0; k < c1; ++k) {
        const SweepCam& im = L.im[k];
        D2 pix;
        if (sees<0>(L.cam[k], p, im.sc.prx, im.sc.pry, im.sc.fx, im.sc.fy, im.sc.resx, im.sc.resy, pix)) {
          // `images[cam](pixel.y(), pixel.x())` (:89): truncated, not interpolated; clamped to the image, which a
          // fractional camera resolution can exceed by one
          const float4 v = sweep_texel(images + im.offset, im.w, im.h, (int)pix.x, (int)pix.y);
          sum.x += v.x;
          sum.y += v.y;
          sum.z += v.z;
          sum.w += v.w;
          ++count;
        }
      }
    }
    if (active) {
      float4 r = background;
      if (count > 0) {  // `accColor / accImages` (:95): Vec / int = the product with 1.0 / n in fp64, then rounded
        const double s = 1.0 / (double)count;
        r = make_float4((float)((double)sum.x * s), (float)((double)sum.y * s), (float)((double)sum.z * s),
                        (float)((double)sum.w * s));
      }
      sweep_store(outKind, out, (size_t)d * n + i, r);
    }
  }
}

// createCroppedEquirect's first loop (:139-156): the smallest and largest column and row at which any camera sees
// the point. bounds = {minX, maxX, minY, maxY}, initialised by the host to {W, 0, H, 0}. Integer atomicMin / atomicMax:
// the result does not depend on the order of arrival.
__global__ void __launch_bounds__(kSweepBlock)
    k_sweep_equirect_bounds(const Cam* __restrict__ cams, const SweepCam* __restrict__ ims, int nCams, SweepEqr e,
                            double depth, int* __restrict__ bounds) {
  const size_t n = (size_t)e.w * e.h;
  const size_t i = (size_t)blockIdx.x * kSweepBlock + threadIdx.x;
  const int x = (int)(i % e.w), y = (int)(i / e.w);
  bool seen = false;
  if (i < n) {
    const D3 p = sweep_eqr_point(e, x, y, depth);
    for (int k = 0; k < nCams && !seen; ++k) {
      const SweepCam& im = ims[k];
      D2 pix;
      seen = sees<0>(cams[k], p, im.sc.prx, im.sc.pry, im.sc.fx, im.sc.fy, im.sc.resx, im.sc.resy, pix);
    }
  }
  if (__ballot(seen) == 0) {
    return;  // (the whole wave)
  }
  int minX = seen ? x : 0x7fffffff, maxX = seen ? x : -1, minY = seen ? y : 0x7fffffff, maxY = seen ? y : -1;
  for (int step = 32; step > 0; step >>= 1) {
    minX = min(minX, __shfl_xor(minX, step));
    maxX = max(maxX, __shfl_xor(maxX, step));
    minY = min(minY, __shfl_xor(minY, step));
    maxY = max(maxY, __shfl_xor(maxY, step));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(bounds, minX);
    atomicMax(bounds + 1, maxX);
    atomicMin(bounds + 2, minY);
    atomicMax(bounds + 3, maxY);
  }
}

}  // namespace derp
