// Kernels of AlignColors (source/calibration/AlignColors.cpp): the red and the blue plane of every camera resampled
// through per-channel lens models onto the green one. k_align_maps builds the two warp maps of a camera once per rig
// (createWarpMap, :52-70); k_align_colors resamples one frame of every camera through them (warpImage, :98-117).
// Definitions and the two implementation-defined points: DESIGN §8.8.
#pragma once
#include "derp_kernels.h"

namespace derp {

constexpr int kAlignBlock = 256;  // threads per block (four waves)
constexpr int kAlignPairs = 4;    // pairs of pixels per thread of k_align_colors: a block takes 2048 pixels
constexpr int kAlignPad = 8;      // every camera starts at a multiple of this many pixels in the maps and the images

// One camera of the calibrated (green) rig with its derived red and blue models. Channel order: green, red, blue.
struct AlignCam {
  Cam lens[3];                // distort / undistort read dist, dist_max and dist_zero of these; nothing else is used
  double principal[2];        // of the green camera, in pixels: the centre of all three models
  double focal[3];            // getScalarFocal() of the three models, in pixels
  unsigned long long offset;  // of the camera's first pixel in the maps and the images, in pixels (a multiple of kAlignPad)
  int32_t w, h;
};

// createWarpMap(src = red / blue, dst = green) (AlignColors.cpp:52-70), fp64, one thread per pixel centre. The green
// undistort (Newton) is shared by the two channels. At n == 0 (a pixel centre on the principal point) the reference
// forms 0 / 0; here the map value is the pixel centre itself, the limit of the expression.
__global__ void __launch_bounds__(kAlignBlock)
    k_align_maps(const AlignCam* __restrict__ cams, int cam, float2* __restrict__ red, float2* __restrict__ blue) {
  const AlignCam& A = cams[cam];
  const size_t n = (size_t)A.w * A.h;
  const size_t i = (size_t)blockIdx.x * kAlignBlock + threadIdx.x;
  if (i >= n) {
    return;
  }
  const double px = (int)(i % A.w) + 0.5, py = (int)(i / A.w) + 0.5;
  const double dx = px - A.principal[0], dy = py - A.principal[1];
  const double norm = sqrt(dx * dx + dy * dy);  // Eigen's norm of a 2-vector (:59)
  float2 r = make_float2((float)px, (float)py), b = r;
  if (norm != 0) {
    const double dstR = norm / A.focal[0];
    const double theta = undistort(A.lens[0], dstR);
    const double ux = dx / norm, uy = dy / norm;
    // (d / n * srcFocal * srcR + principal), coefficient-wise and left to right (:63-65); cv::Point2f rounds to float
    const double redR = distort(A.lens[1], theta), blueR = distort(A.lens[2], theta);
    r = make_float2((float)((ux * A.focal[1]) * redR + A.principal[0]), (float)((uy * A.focal[1]) * redR + A.principal[1]));
    b = make_float2((float)((ux * A.focal[2]) * blueR + A.principal[0]), (float)((uy * A.focal[2]) * blueR + A.principal[1]));
  }
  red[A.offset + i] = r;
  blue[A.offset + i] = b;
}

// One channel of getPixelBilinear on Vec3w (CvUtil.h:78-120, the function bilerp_u16 of derp_kernels.h restates): round
// half away from zero, taps (xi - 1, yi - 1) .. (xi, yi) clamped to the edge, float blend truncated to u16
__device__ __forceinline__ unsigned align_tap(const uint16_t* __restrict__ image, int w, int h, float2 at, int channel) {
  const float xf = roundf(at.x), yf = roundf(at.y);
  const int xi = (int)xf, yi = (int)yf;
  const float xw = at.x - xf + 0.5f, yw = at.y - yf + 0.5f;
  const float w00 = (1 - xw) * (1 - yw), w01 = xw * (1 - yw), w10 = (1 - xw) * yw, w11 = xw * yw;
  const int xa = min(max(xi - 1, 0), w - 1), xb = min(max(xi, 0), w - 1);
  const int ya = min(max(yi - 1, 0), h - 1), yb = min(max(yi, 0), h - 1);
  const uint16_t* rowA = image + (size_t)ya * w * 3 + channel;
  const uint16_t* rowB = image + (size_t)yb * w * 3 + channel;
  const float p00 = (float)rowA[xa * 3], p01 = (float)rowA[xb * 3], p10 = (float)rowB[xa * 3], p11 = (float)rowB[xb * 3];
  return (unsigned)bilerp_u16(p00, p01, p10, p11, w00, w01, w10, w11);
}

// warpImage (AlignColors.cpp:98-117) of one frame of every camera (blockIdx.y): G is the own texel, R the red map's
// bilinear tap, B the blue map's. A streaming pass. A lane owns pairs of neighbouring pixels of the camera's flat image,
// kAlignPairs of them a block's width apart: a pair's two values of a map are one 16-byte word, its two texels three
// 32-bit words (B0 G0 | R0 B1 | G1 R1) of which the first and the last hold the G it keeps, and neighbouring lanes read
// and write neighbouring words. The eight taps of a pixel fall within a few pixels of it, so one gather instruction of
// a wave touches the few cache lines under its 128 pixels, which the wave's own reads bring in. An image with an odd
// number of pixels ends in a lane with one pixel.
__global__ void __launch_bounds__(kAlignBlock)
    k_align_colors(const AlignCam* __restrict__ cams, const float2* __restrict__ red, const float2* __restrict__ blue,
                   const uint16_t* __restrict__ in, uint16_t* __restrict__ out) {
  const AlignCam& A = cams[blockIdx.y];
  const int w = A.w, h = A.h;
  const size_t n = (size_t)w * h;
  // (offset is a multiple of kAlignPad: the maps' words below are 16-byte aligned, the images' 4-byte aligned)
  const uint16_t* image = in + A.offset * 3;
  const float4* red4 = reinterpret_cast<const float4*>(red + A.offset);
  const float4* blue4 = reinterpret_cast<const float4*>(blue + A.offset);
  const uint32_t* own = reinterpret_cast<const uint32_t*>(image);
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + A.offset * 3);
  const size_t q0 = (size_t)blockIdx.x * (kAlignBlock * kAlignPairs) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kAlignPairs; ++j) {
    const size_t q = q0 + (size_t)j * kAlignBlock;  // the pair of pixels 2 q and 2 q + 1
    if (2 * q + 1 < n) {
      const float4 mr = red4[q], mb = blue4[q];
      const uint32_t first = own[3 * q], last = own[3 * q + 2];
      const unsigned b0 = align_tap(image, w, h, make_float2(mb.x, mb.y), 0), r0 = align_tap(image, w, h, make_float2(mr.x, mr.y), 2);
      const unsigned b1 = align_tap(image, w, h, make_float2(mb.z, mb.w), 0), r1 = align_tap(image, w, h, make_float2(mr.z, mr.w), 2);
      dst[3 * q] = b0 | (first & 0xffff0000u);
      dst[3 * q + 1] = r0 | (b1 << 16);
      dst[3 * q + 2] = (last & 0xffffu) | (r1 << 16);
    } else if (2 * q < n) {
      const size_t i = 2 * q;
      uint16_t* px = out + (A.offset + i) * 3;
      px[0] = (uint16_t)align_tap(image, w, h, blue[A.offset + i], 0);
      px[1] = image[i * 3 + 1];
      px[2] = (uint16_t)align_tap(image, w, h, red[A.offset + i], 2);
    }
  }
}

}  // namespace derp
