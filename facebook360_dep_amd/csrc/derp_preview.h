// The tuning previews' kernels: the marks of ViewColorVarianceThresholds and the overlay of
// ViewForegroundMaskThresholds, and the rectangle splat and blend of GenerateKeypointProjections. The first two are one
// pass over an image: one thread per pixel, a wave reads 64 consecutive texels (512 B of BGRX) and writes the 384
// consecutive bytes of their interleaved BGR as three 2-byte stores per lane (6-byte stride: the wave's stores touch the
// same lines, they are not one wide store each); nothing is kept but a few registers.
// The counts are reduced per wave with a ballot, and one lane of the wave adds them to the device counter.
// Included by derp_capi.hip after derp_kernels.h.
#pragma once
#include "derp_kernels.h"
#include "derp_points.h"

namespace derp {

constexpr int kPreviewBlock = 256;
constexpr int kPreviewMaxImages = 256;  // settings rendered by one call

// bits set among the active lanes of the wave (wave64 on gfx950)
__device__ __forceinline__ unsigned preview_wave_count(bool flag) {
  return (unsigned)__popcll(__ballot(flag));
}
// the first active lane of a wave: the one that issues the wave's atomic
__device__ __forceinline__ bool preview_wave_leader() {
  return (int)__lane_id() == __ffsll((long long)__ballot(true)) - 1;
}

// TrackVar::update (ViewColorVarianceThresholds.cpp:69-81): srcMarked = image; setTo(blue, var < varLowShow);
// setTo(purple, var > varHighShow) — the second after the first, so purple wins where both hold (they cannot:
// varHighShow >= varLowShow); a variance equal to a threshold is marked by neither. blockIdx.y = the setting.
// counts[2k] = blue pixels of setting k, counts[2k + 1] = purple ones.
__global__ void __launch_bounds__(kPreviewBlock) k_preview_marks(const ushort4* __restrict__ image, const float* __restrict__ var,
                                                                 size_t n, const float* __restrict__ lowShow,
                                                                 const float* __restrict__ highShow, uint16_t* __restrict__ out,
                                                                 unsigned* __restrict__ counts) {
  const int k = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * kPreviewBlock + threadIdx.x;
  const bool live = i < n;
  bool blue = false, purple = false;
  if (live) {
    const float v = var[i];
    ushort4 q = image[i];
    blue = v < lowShow[k];
    purple = v > highShow[k];
    if (blue) {
      q = make_ushort4(65535, 0, 0, 0);
    }
    if (purple) {
      q = make_ushort4(65535, 0, 65535, 0);
    }
    uint16_t* o = out + ((size_t)k * n + i) * 3;
    o[0] = q.x;
    o[1] = q.y;
    o[2] = q.z;
  }
  const unsigned nb = preview_wave_count(blue && !purple), np = preview_wave_count(purple);
  if (preview_wave_leader()) {
    if (nb) {
      atomicAdd(counts + 2 * k, nb);
    }
    if (np) {
      atomicAdd(counts + 2 * k + 1, np);
    }
  }
}

// TrackVar::update (ViewForegroundMaskThresholds.cpp:71-81): maskPt = green where the mask is set, 0 elsewhere;
// addWeighted(fg, 1.0, maskPt, 0.5, 0) on CV_16UC3 = saturate_cast<ushort>(cvRound(fg * 1.0f + maskPt * 0.5f + 0.0f)).
// Outside the mask and on B and R the second term is 0 and the value is returned as it is; on G of a masked pixel it is
// g + 32767.5, exact in fp32 (below 2^17 with one fraction bit), rounded half to even and saturated.
// count = the masked pixels (the reference's "foreground amount").
__global__ void __launch_bounds__(kPreviewBlock) k_preview_overlay(const ushort4* __restrict__ frame, const uint8_t* __restrict__ mask,
                                                                   size_t n, uint16_t* __restrict__ out,
                                                                   unsigned* __restrict__ count) {
  const size_t i = (size_t)blockIdx.x * kPreviewBlock + threadIdx.x;
  const bool live = i < n;
  bool set = false;
  if (live) {
    const ushort4 q = frame[i];
    set = mask[i] != 0;
    unsigned g = q.y;
    if (set) {
      const float r = rintf((float)q.y * 1.0f + 65535.0f * 0.5f);
      g = r >= 65535.0f ? 65535u : (unsigned)r;
    }
    uint16_t* o = out + i * 3;
    o[0] = q.x;
    o[1] = (uint16_t)g;
    o[2] = q.z;
  }
  const unsigned ns = preview_wave_count(set);
  if (ns && preview_wave_leader()) {
    atomicAdd(count, ns);
  }
}

// ---- GenerateKeypointProjections (source/render/GenerateKeypointProjections.cpp:57-104) ----
// One filled cv::rectangle of the reference: corners inclusive and already clipped to the image (x1 < x0 or y1 < y0:
// nothing of it is inside), and the grid point's colour B, G, R, A. The list is in the reference's drawing order.
struct PreviewRect {
  int x0, y0, x1, y1;
  float4 color;
};

// A later rectangle overwrites an earlier one, so a pixel belongs to the covering rectangle of the highest sequence
// number: one block per rectangle (grid-stride), consecutive threads on consecutive pixels of a row of it, atomicMax of
// (sequence number + 1) into a zeroed plane. Integer maxima: the result does not depend on the order of execution.
__global__ void __launch_bounds__(kPreviewBlock) k_preview_splat(const PreviewRect* __restrict__ rects, unsigned n, int w,
                                                                 unsigned* __restrict__ plane) {
  for (unsigned r = blockIdx.x; r < n; r += gridDim.x) {
    const PreviewRect q = rects[r];
    const long long rw = (long long)q.x1 - q.x0 + 1, rh = (long long)q.y1 - q.y0 + 1;
    if (rw <= 0 || rh <= 0) {
      continue;
    }
    for (long long t = threadIdx.x; t < rw * rh; t += kPreviewBlock) {
      const long long y = q.y0 + t / rw, x = q.x0 + t % rw;
      atomicMax(plane + (size_t)y * w + (size_t)x, r + 1);
    }
  }
}

__device__ __forceinline__ unsigned preview_u8(float v) {  // `255.0f * blend` into an 8-bit file (sweep_ref.to_u8)
  const float r = rintf(255.0f * v);
  return r != r ? 0u : (unsigned)fminf(fmaxf(r, 0.0f), 255.0f);
}

// cv::addWeighted(image, 1, keypointProjection, 0.6, 0) on CV_32FC4: img * 1.0f + kp * 0.6f + 0.0f, a product and a sum
// each rounded (the build never fuses them), then the file's bytes. outFloat may be null.
__global__ void __launch_bounds__(kPreviewBlock) k_preview_keypoint_blend(const float4* __restrict__ image,
                                                                          const unsigned* __restrict__ plane,
                                                                          const PreviewRect* __restrict__ rects, size_t n,
                                                                          uchar4* __restrict__ outU8, float4* __restrict__ outFloat) {
  const size_t i = (size_t)blockIdx.x * kPreviewBlock + threadIdx.x;
  if (i >= n) {
    return;
  }
  const unsigned seq = plane[i];
  const float4 kp = seq ? rects[seq - 1].color : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float4 im = image[i];
  float4 b;
  b.x = im.x * 1.0f + kp.x * 0.6f + 0.0f;
  b.y = im.y * 1.0f + kp.y * 0.6f + 0.0f;
  b.z = im.z * 1.0f + kp.z * 0.6f + 0.0f;
  b.w = im.w * 1.0f + kp.w * 0.6f + 0.0f;
  outU8[i] = make_uchar4((unsigned char)preview_u8(b.x), (unsigned char)preview_u8(b.y), (unsigned char)preview_u8(b.z),
                         (unsigned char)preview_u8(b.w));
  if (outFloat) {
    outFloat[i] = b;
  }
}

}  // namespace derp
