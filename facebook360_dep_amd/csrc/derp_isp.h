// Camera ISP: raw Bayer -> RGB. The stages of CameraIsp::executePipeline (source/isp/CameraIsp.h:1227-1237) in the
// reference's order, arithmetic and operand order, fp32, one kernel (or a few) per stage; the planes stay in HBM
// between stages and every stage keeps its own output so that derp_isp_stage can show it.
//
//   load (loadImageFromSensor :767-835 + resizeInput :323-344)          k_isp_load
//   blackLevelAdjust, antiVignette, whiteBalance, clampAndStretch        k_isp_pixel (one launch)
//   removeStuckPixels (:980-1059)                                        host, between two device phases
//   demosaic (:1115-1175)                                                k_isp_bilinear | k_isp_green_bilinear |
//                                                                        k_isp_ea_gradient + k_isp_ea_vote, k_isp_chroma
//   colorCorrect (:1177-1205)                                            k_isp_color
//   sharpen (:1207-1223; Filter.h:35-118)                                k_isp_iir_rows, k_isp_iir_cols, k_isp_sharpen
//   getImage (:1276-1297)                                                k_isp_output
//
// Memory the reference reads before it wrote it (cv::Mat_ allocations without a fill) is taken as 0 here:
// redMinusGreen / blueMinusGreen at pixels of another colour (demosaicChromaSuppressed :253-264 fills only its own
// phase, and reflect() at the high border maps onto the other phase), element cols-1 of iirLowPass's line buffer in
// the horizontal pass, and column 0 of lpImage, which the horizontal pass never writes (Filter.h:43-64).
// Included by derp_capi.hip (one translation unit).
#pragma once

namespace {

constexpr int kIspLutSize = 4096;  // kToneCurveLutSize, CameraIsp.h:40

// math_util::reflect (MathUtil.h:42-44): -1 -> 1, but r -> r - 1
__host__ __device__ __forceinline__ int isp_reflect(int x, int r) {
  return x < 0 ? -x : x >= r ? 2 * r - x - 1 : x;
}
// math_util::clamp (MathUtil.h:37-39), same comparisons (a NaN passes through)
__host__ __device__ __forceinline__ float isp_clamp(float x, float a, float b) {
  return x < a ? a : x > b ? b : x;
}

// the raw plane and its Bayer pattern: 2 bits per position (i % 2) * 2 + (j % 2), 0 = red, 1 = green, 2 = blue
struct IspMosaic {
  const float* raw;
  int w, h;
  unsigned pat;
};
__host__ __device__ __forceinline__ int isp_color(unsigned pat, int i, int j) {
  return (pat >> (2 * (((i & 1) << 1) | (j & 1)))) & 3;
}
// plane X of demosaic()'s split (:1118-1134): the raw value at pixels of colour X, 0 elsewhere
__device__ __forceinline__ float isp_init(const IspMosaic& M, int X, int i, int j) {
  return isp_color(M.pat, i, j) == X ? M.raw[(size_t)i * M.w + j] : 0.0f;
}

// ---- load ----------------------------------------------------------------------------------------
struct IspLoad {
  int sw, sh, w, h, resize, swap, planar, rowMajor;
  int planeOf[4];  // plane that lands on Bayer position p (inverse of getPlaneOrderToBayerOrder as :821 applies it)
  float areaRecip;
};
// value of the interleaved, host-order sensor image at (R, C): the inverse of the reorder loop :829-833
template <typename T>
__device__ __forceinline__ float isp_sensor(const T* in, const IspLoad& L, int R, int C) {
  size_t k;
  if (L.planar) {
    const int pw = L.sw / 2, ph = L.sh / 2, r = R >> 1, c = C >> 1;
    const int plane = L.planeOf[((R & 1) << 1) | (C & 1)];
    k = (size_t)plane * pw * ph + (L.rowMajor ? (size_t)r * pw + c : (size_t)r + (size_t)ph * c);
  } else {
    k = L.rowMajor ? (size_t)R * L.sw + C : (size_t)R + (size_t)L.sh * C;
  }
  unsigned v = in[k];
  if (sizeof(T) == 2 && L.swap) {
    v = ((v & 0xffu) << 8) | (v >> 8);
  }
  return (float)v;
}
template <typename T>
__global__ __launch_bounds__(256) void k_isp_load(const T* __restrict__ in, float* __restrict__ raw, IspLoad L) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= L.h || j >= L.w) {
    return;
  }
  const int r = L.resize > 1 ? 2 : 1;
  float sum = 0.0f;
  for (int k = 0; k < L.resize; ++k) {
    const int ipp = isp_reflect(i * L.resize + k * 2 + (i % r), L.sh);
    for (int l = 0; l < L.resize; ++l) {
      const int jpp = isp_reflect(j * L.resize + l * 2 + (j % r), L.sw);
      sum += isp_sensor(in, L, ipp, jpp);
    }
  }
  raw[(size_t)i * L.w + j] = sum * L.areaRecip;
}

// ---- blackLevelAdjust (:1061-1081), antiVignette (:1096-1105), whiteBalance (:962-978), clampAndStretch (:1083-1094)
struct IspPixel {
  float black[3], blackScale[3], gain[3], cmin[3], cmax[3];
};
__global__ __launch_bounds__(256) void k_isp_pixel(const float* __restrict__ in, float* __restrict__ out,
                                                   const float* __restrict__ vigH, const float* __restrict__ vigV, int w,
                                                   int h, unsigned pat, IspPixel P) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= h || j >= w) {
    return;
  }
  const int ch = isp_color(pat, i, j);
  float v = in[(size_t)i * w + j];
  if (v < 1.0f) {
    v = (v - P.black[ch]) * P.blackScale[ch];
  }
  v *= vigH[3 * j + ch] * vigV[3 * i + ch];
  v *= P.gain[ch];
  v = isp_clamp(v, 0.0f, 1.0f);
  const float c = isp_clamp(v, P.cmin[ch], P.cmax[ch]);
  out[(size_t)i * w + j] = (c - P.cmin[ch]) / (P.cmax[ch] - P.cmin[ch]);
}

// ---- demosaicBilinearFilter (:93-127) --------------------------------------------------------------
// The reference updates r, g, b in place while it scans. A pixel writes the two planes that are not its own colour,
// from neighbours at (i +- 1, j +- 1). Away from the high border those neighbours hold their own colour in the plane
// read (the other Bayer phase), which no pixel writes, so the order of the scan does not matter. reflect() maps
// i + 1 = height onto row height - 1 and j + 1 = width onto column width - 1, i.e. onto the pixel's own row / column
// (or the pixel itself, not yet written: 0). Of those reads only the diagonal ones of a red or blue pixel in the last
// row / column land on a pixel the scan has already passed AND in a plane that pixel wrote: a green pixel's red or
// blue. That value came from a vertical or horizontal pair made of one own-colour pixel and the green pixel itself
// (0), so the chain ends after one step. TOP = true resolves such a read by computing what the earlier pixel wrote.
template <bool TOP>
__device__ float isp_bilinear_value(const IspMosaic& M, int X, int i, int j) {
  const int i_1 = isp_reflect(i - 1, M.h), i1 = isp_reflect(i + 1, M.h);
  const int j_1 = isp_reflect(j - 1, M.w), j1 = isp_reflect(j + 1, M.w);
  auto rd = [&](int qi, int qj) {
    if constexpr (TOP) {
      if ((qi < i || (qi == i && qj < j)) && isp_color(M.pat, qi, qj) != X) {
        return isp_bilinear_value<false>(M, X, qi, qj);
      }
    }
    return isp_init(M, X, qi, qj);
  };
  const int c = isp_color(M.pat, i, j);
  if (c == 1) {
    const bool redGreenRow = isp_color(M.pat, i, 0) == 0 || isp_color(M.pat, i, 1) == 0;
    if ((X == 2) == redGreenRow) {
      return (rd(i_1, j) + rd(i1, j)) * 0.5f;  // / 2.0f
    }
    return (rd(i, j_1) + rd(i, j1)) * 0.5f;
  }
  if (X == 1) {  // cv_util::bilerp(.., 0.5f, 0.5f), CvUtil.h:84-86: four products by 0.25f summed left to right
    return 0.25f * rd(i_1, j) + 0.25f * rd(i1, j) + 0.25f * rd(i, j_1) + 0.25f * rd(i, j1);
  }
  return 0.25f * rd(i_1, j_1) + 0.25f * rd(i1, j_1) + 0.25f * rd(i_1, j1) + 0.25f * rd(i1, j1);
}
__global__ __launch_bounds__(256) void k_isp_bilinear(IspMosaic M, float* __restrict__ R, float* __restrict__ G,
                                                      float* __restrict__ B) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= M.h || j >= M.w) {
    return;
  }
  const int c = isp_color(M.pat, i, j);
  const float own = M.raw[(size_t)i * M.w + j];
  const size_t o = (size_t)i * M.w + j;
  R[o] = c == 0 ? own : isp_bilinear_value<true>(M, 0, i, j);
  G[o] = c == 1 ? own : isp_bilinear_value<true>(M, 1, i, j);
  B[o] = c == 2 ? own : isp_bilinear_value<true>(M, 2, i, j);
}

// ---- demosaicGreenBilinear (:227-248), green part --------------------------------------------------
// In place in the reference; a red or blue pixel reads green at its four edge neighbours, which are green pixels
// (never written) or, through reflect() at the high border, the pixel itself before its write (0).
__global__ __launch_bounds__(256) void k_isp_green_bilinear(IspMosaic M, float* __restrict__ G) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= M.h || j >= M.w) {
    return;
  }
  G[(size_t)i * M.w + j] =
      isp_color(M.pat, i, j) == 1 ? M.raw[(size_t)i * M.w + j] : isp_bilinear_value<false>(M, 1, i, j);
}

// ---- demosaicEdgeAware (:161-225) ------------------------------------------------------------------
// Gradient pass: reads the split planes only (nothing is written to them in this loop). Keeps gV, gH and the one bit
// of dV / dH the vote needs: dH <= dV.
__global__ __launch_bounds__(256) void k_isp_ea_gradient(IspMosaic M, float* __restrict__ gVo, float* __restrict__ gHo,
                                                         unsigned char* __restrict__ bit) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= M.h || j >= M.w) {
    return;
  }
  const int i_1 = isp_reflect(i - 1, M.h), i1 = isp_reflect(i + 1, M.h);
  const int i_2 = isp_reflect(i - 2, M.h), i2 = isp_reflect(i + 2, M.h);
  const int j_1 = isp_reflect(j - 1, M.w), j1 = isp_reflect(j + 1, M.w);
  const int j_2 = isp_reflect(j - 2, M.w), j2 = isp_reflect(j + 2, M.w);
  const int c = isp_color(M.pat, i, j);
  float gV, gH, dV, dH;
  if (c == 1) {
    const float g = isp_init(M, 1, i, j);
    gV = g;
    gH = g;
    dV = (fabsf(isp_init(M, 1, i2, j) - g) + fabsf(g - isp_init(M, 1, i_2, j))) * 0.5f;
    dH = (fabsf(isp_init(M, 1, i, j2) - g) + fabsf(g - isp_init(M, 1, i, j_2))) * 0.5f;
  } else {
    const float gu = isp_init(M, 1, i_1, j), gd = isp_init(M, 1, i1, j);
    const float gl = isp_init(M, 1, i, j_1), gr = isp_init(M, 1, i, j1);
    gV = (gu + gd) * 0.5f;
    gH = (gl + gr) * 0.5f;
    dV = fabsf(gu - gd) * 0.5f;
    dH = fabsf(gl - gr) * 0.5f;
    const float p = isp_init(M, c, i, j);
    const float pu = isp_init(M, c, i_2, j), pd = isp_init(M, c, i2, j);
    const float pl = isp_init(M, c, i, j_2), pr = isp_init(M, c, i, j2);
    gV += (2.0f * p - pu - pd) * 0.25f;
    gH += (2.0f * p - pl - pr) * 0.25f;
    dV += fabsf(-2.0f * p + pu + pd) * 0.5f;
    dH += fabsf(-2.0f * p + pl + pr) * 0.5f;
  }
  const size_t o = (size_t)i * M.w + j;
  gVo[o] = gV;
  gHo[o] = gH;
  bit[o] = dH <= dV ? 1 : 0;
}
// Homogeneity vote (:206-223): hCount = number of (dH <= dV) over the 9 x 9 reflected neighbourhood, an integer, so a
// separable box sum of the bit is exact. One 16 x 16 tile per block; the 24 x 24 bits with halo are staged once in LDS.
// Writes green for EVERY pixel, green ones included, as the reference does (lerp(g, g, a) is not always g).
__global__ __launch_bounds__(256) void k_isp_ea_vote(const unsigned char* __restrict__ bit, const float* __restrict__ gV,
                                                     const float* __restrict__ gH, float* __restrict__ G, int w, int h) {
  __shared__ unsigned char t[24][24];
  __shared__ unsigned char hs[24][16];
  const int tid = threadIdx.y * 16 + threadIdx.x;
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  for (int idx = tid; idx < 24 * 24; idx += 256) {
    const int r = idx / 24, c = idx % 24;
    const int y = y0 + r - 4, x = x0 + c - 4;
    unsigned char v = 0;
    if (y <= h + 3 && x <= w + 3) {  // what a pixel inside the image can reach; h, w >= 5 keep one reflection in range
      v = bit[(size_t)isp_reflect(y, h) * w + isp_reflect(x, w)];
    }
    t[r][c] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < 24 * 16; idx += 256) {
    const int r = idx / 16, c = idx % 16;
    int s = 0;
    for (int k = 0; k < 9; ++k) {
      s += t[r][c + k];
    }
    hs[r][c] = (unsigned char)s;
  }
  __syncthreads();
  const int j = x0 + threadIdx.x, i = y0 + threadIdx.y;
  if (i >= h || j >= w) {
    return;
  }
  int hCount = 0;
  for (int k = 0; k < 9; ++k) {
    hCount += hs[threadIdx.y + k][threadIdx.x];
  }
  const float a = div_int_by_const(hCount, 1.0 / 81.0);  // float(hCount) / diameterSquared
  const size_t o = (size_t)i * w + j;
  G[o] = gV[o] * (1.0f - a) + gH[o] * a;  // math_util::lerp, MathUtil.h:56-59
}

// ---- demosaicChromaSuppressed (:250-320) -----------------------------------------------------------
// redMinusGreen / blueMinusGreen are arrays of their own and green is not written here, so the second loop reads
// nothing it writes: no ordering to respect. A difference plane at a pixel of another colour is memory the reference
// never filled; 0 here (see the head of this file). The green-pixel case sums diffCh1(i1, j2) twice, as :298-299 does.
__global__ __launch_bounds__(256) void k_isp_chroma(IspMosaic M, const float* __restrict__ G, float* __restrict__ R,
                                                    float* __restrict__ B) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= M.h || j >= M.w) {
    return;
  }
  const int i_1 = isp_reflect(i - 1, M.h), i1 = isp_reflect(i + 1, M.h);
  const int i_2 = isp_reflect(i - 2, M.h), i2 = isp_reflect(i + 2, M.h);
  const int j_1 = isp_reflect(j - 1, M.w), j1 = isp_reflect(j + 1, M.w);
  const int j_2 = isp_reflect(j - 2, M.w), j2 = isp_reflect(j + 2, M.w);
  auto diff = [&](int X, int qi, int qj) {
    const size_t q = (size_t)qi * M.w + qj;
    return isp_color(M.pat, qi, qj) == X ? M.raw[q] - G[q] : 0.0f;
  };
  const double rcp5 = 1.0 / 5.0, rcp6 = 1.0 / 6.0;
  const int c = isp_color(M.pat, i, j);
  const size_t o = (size_t)i * M.w + j;
  const float g = G[o];
  if (c != 1) {
    const int X = c, Y = 2 - c;  // own colour: five-point cross; the other: four diagonals
    const float other = (diff(Y, i_1, j_1) + diff(Y, i1, j_1) + diff(Y, i_1, j1) + diff(Y, i1, j1)) * 0.25f + g;
    const float own =
        div_by_const(diff(X, i, j) + diff(X, i_2, j) + diff(X, i2, j) + diff(X, i, j_2) + diff(X, i, j2), rcp5) + g;
    (c == 0 ? R : B)[o] = own;
    (c == 0 ? B : R)[o] = other;
  } else {
    const bool redGreenRow = isp_color(M.pat, i, 0) == 0 || isp_color(M.pat, i, 1) == 0;
    const int X1 = redGreenRow ? 2 : 0, X2 = 2 - X1;
    const float ch1 = div_by_const(diff(X1, i_1, j_2) + diff(X1, i_1, j) + diff(X1, i_1, j2) + diff(X1, i1, j_2) +
                                       diff(X1, i1, j2) + diff(X1, i1, j2),
                                   rcp6) +
                      g;
    const float ch2 = div_by_const(diff(X2, i_2, j_1) + diff(X2, i, j_1) + diff(X2, i2, j_1) + diff(X2, i_2, j1) +
                                       diff(X2, i, j1) + diff(X2, i2, j1),
                                   rcp6) +
                      g;
    (X1 == 0 ? R : B)[o] = ch1;
    (X1 == 0 ? B : R)[o] = ch2;
  }
}

// ---- colorCorrect (:1177-1205) ---------------------------------------------------------------------
struct IspCcm {
  float m[9];
};
// the index: clamped in float, then the float -> size_t conversion of vector::operator[] (truncation). A NaN, which
// the reference's conversion leaves undefined, indexes entry 0.
__device__ __forceinline__ int isp_lut_index(float v) {
  const float c = isp_clamp(v, 0.0f, (float)(kIspLutSize - 1));
  return c == c ? (int)c : 0;
}
__global__ __launch_bounds__(256) void k_isp_color(const float* __restrict__ in, float* __restrict__ out,
                                                   const float* __restrict__ lut, size_t n, IspCcm C) {
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) {
    return;
  }
  const float p0 = in[o], p1 = in[n + o], p2 = in[2 * n + o];
  out[o] = lut[3 * isp_lut_index(C.m[0] * p0 + C.m[1] * p1 + C.m[2] * p2) + 0];
  out[n + o] = lut[3 * isp_lut_index(C.m[3] * p0 + C.m[4] * p1 + C.m[5] * p2) + 1];
  out[2 * n + o] = lut[3 * isp_lut_index(C.m[6] * p0 + C.m[7] * p1 + C.m[8] * p2) + 2];
}

// ---- iirLowPass (Filter.h:35-85) -------------------------------------------------------------------
// fp32 addition is not associative: every row, then every column, is one sequential chain, one lane each, per channel
// (blockIdx.y). Horizontal pass: a wave owns 64 rows and walks them 64 columns at a time through an LDS tile, so that
// global loads and stores run along rows. The line buffer of the reference becomes `scr` (one plane per channel):
// the causal loop writes buffer(reflect(j - 1)), so after it buffer[k] = causal value of column k + 1 for k <= cols - 2
// and buffer[cols - 1] is never written (0). The anticausal loop starts from buffer(0), reads buffer(j) and writes
// lpImage(i, reflect(j + 1)): column j + 1 for j <= cols - 2 (the value of j = cols - 1 is overwritten), column 0 never.
// The same buffer serves the vertical pass, which never writes element rows - 1: when rows < cols it still holds what
// the last row's causal loop left there, the causal value of column `rows`; that is `stale[channel]`.
__global__ __launch_bounds__(64) void k_isp_iir_rows(const float* __restrict__ inP, float* __restrict__ scrP,
                                                     float* __restrict__ lpP, float* __restrict__ stale, int w, int h,
                                                     float alpha) {
  __shared__ float tile[64][65];
  const int lane = threadIdx.x, row0 = blockIdx.x * 64, row = row0 + lane;
  const size_t plane = (size_t)w * h * blockIdx.y;
  const float* in = inP + plane;
  float* scr = scrP + plane;
  float* lp = lpP + plane;
  const bool live = row < h;
  const float oma = 1.0f - alpha;
  float v = live ? in[(size_t)row * w + (w - 1)] : 0.0f;
  for (int c0 = 0; c0 < w; c0 += 64) {
    for (int r = 0; r < 64; ++r) {
      tile[r][lane] = (row0 + r < h && c0 + lane < w) ? in[(size_t)(row0 + r) * w + c0 + lane] : 0.0f;
    }
    __syncthreads();
    if (live) {
      const int n = min(64, w - c0);
      for (int c = 0; c < n; ++c) {
        v = tile[lane][c] * oma + v * alpha;  // math_util::lerp(ip, v, alpha)
        tile[lane][c] = v;
        if (row == h - 1 && c0 + c == h) {
          stale[blockIdx.y] = v;
        }
      }
    }
    __syncthreads();
    for (int r = 0; r < 64; ++r) {
      if (row0 + r < h && c0 + lane < w) {
        scr[(size_t)(row0 + r) * w + c0 + lane] = tile[r][lane];
      }
    }
    __syncthreads();
  }
  v = live ? scr[(size_t)row * w + 1] : 0.0f;  // buffer(0, 0)
  for (int c0 = ((w - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
    for (int r = 0; r < 64; ++r) {  // buffer[j] for j = c0 + lane
      tile[r][lane] = (row0 + r < h && c0 + lane <= w - 2) ? scr[(size_t)(row0 + r) * w + c0 + lane + 1] : 0.0f;
    }
    __syncthreads();
    if (live) {
      for (int c = min(64, w - c0) - 1; c >= 0; --c) {
        v = tile[lane][c] * oma + v * alpha;
        tile[lane][c] = isp_clamp(v, 0.0f, 1.0f);
      }
    }
    __syncthreads();
    for (int r = 0; r < 64; ++r) {
      if (row0 + r < h && c0 + lane <= w - 2) {
        lp[(size_t)(row0 + r) * w + c0 + lane + 1] = tile[r][lane];
      }
    }
    __syncthreads();
  }
  if (live) {
    lp[(size_t)row * w] = 0.0f;
  }
}
// Vertical pass, in place on lpImage: one lane per column, so a wave reads and writes along rows as it is. Starts from
// row 1, buffer[k] = causal value of row k + 1, the anticausal loop starts from buffer(rows - 2), runs to i = -1
// (which reads buffer(1) and writes row 0) and reads the stale element at i = rows - 1.
__global__ __launch_bounds__(64) void k_isp_iir_cols(float* __restrict__ lpP, float* __restrict__ scrP,
                                                     const float* __restrict__ stale, int w, int h, float alpha) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= w) {
    return;
  }
  const size_t plane = (size_t)w * h * blockIdx.y;
  float* lp = lpP + plane;
  float* scr = scrP + plane;
  const float oma = 1.0f - alpha;
  const float last = stale[blockIdx.y];
  float v = lp[(size_t)w + j];
  for (int i = 0; i < h; ++i) {
    v = lp[(size_t)i * w + j] * oma + v * alpha;
    if (i >= 1) {
      scr[(size_t)(i - 1) * w + j] = v;
    }
  }
  v = scr[(size_t)(h - 2) * w + j];
  for (int i = h - 1; i >= -1; --i) {
    const int k = isp_reflect(i, h);
    const float ip = k == h - 1 ? last : scr[(size_t)k * w + j];
    v = ip * oma + v * alpha;
    lp[(size_t)isp_reflect(i + 1, h) * w + j] = isp_clamp(v, 0.0f, 1.0f);
  }
}
// sharpenWithIirLowPass (Filter.h:87-118), maxVal = 1; expf is glibc's (derp_kernels.h)
struct IspSharpen {
  float amount[3], noiseCore;
};
__global__ __launch_bounds__(256) void k_isp_sharpen(const float* __restrict__ in, const float* __restrict__ lpP,
                                                     float* __restrict__ out, size_t n, IspSharpen S) {
  __shared__ unsigned long long expTab[32];
  if (threadIdx.x < 32) {
    expTab[threadIdx.x] = kExp2fTab[threadIdx.x];
  }
  __syncthreads();
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) {
    return;
  }
  for (int c = 0; c < 3; ++c) {
    const float p = in[c * n + o], lp = lpP[c * n + o];
    const float hp = p - lp;
    const float ng = 1.0f - expf_glibc(-(hp * hp * S.noiseCore), expTab);
    out[c * n + o] = isp_clamp(lp + hp * ng * S.amount[c], 0.0f, 1.0f);
  }
}

// ---- getImage (:1276-1297): scale, the plain float -> integer conversion (truncation), BGR -------------
template <typename T>
__global__ __launch_bounds__(256) void k_isp_output(const float* __restrict__ in, T* __restrict__ out, size_t n,
                                                    float scale) {
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) {
    return;
  }
  for (int c = 0; c < 3; ++c) {
    const float dp = scale * in[c * n + o];
    out[3 * o + (2 - c)] = dp == dp ? (T)dp : (T)0;  // values are in [0, scale]; a NaN (undefined there) gives 0
  }
}

// ---- host: tables ----------------------------------------------------------------------------------
// math_util::BezierCurve<float, Vec3f>::operator() (MathUtil.h:122-128): recursive De Casteljau, lerp per component
void isp_bezier(const float (*pts)[3], int i, int j, float t, float out[3]) {
  if (i == j) {
    memcpy(out, pts[i], sizeof(float) * 3);
    return;
  }
  float a[3], b[3];
  isp_bezier(pts, i, j - 1, t, a);
  isp_bezier(pts, i + 1, j, t, b);
  for (int c = 0; c < 3; ++c) {
    out[c] = a[c] * (1.0f - t) + b[c] * t;
  }
}
inline float isp_lerp(float x0, float x1, float a) {
  return x0 * (1.0f - a) + x1 * a;
}
inline float isp_bezier4(float a, float b, float c, float d, float t) {  // CameraIsp.h:357-363
  return isp_lerp(isp_lerp(isp_lerp(a, b, t), isp_lerp(b, c, t), t), isp_lerp(isp_lerp(b, c, t), isp_lerp(c, d, t), t), t);
}
inline float isp_high_key(float boost, float x) {  // :365-371
  const float b = isp_clamp(0.6666f, 0.0f, 1.0f), c = isp_clamp(0.8333f + boost, 0.0f, 1.0f);
  return x > 0.5f ? isp_bezier4(0.5f, b, c, 1.0f, (x - 0.5f) * 2.0f) : 0;
}
inline float isp_low_key(float boost, float x) {  // :373-379
  const float b = isp_clamp(0.1666f + boost, 0.0f, 1.0f), c = isp_clamp(0.3333f, 0.0f, 1.0f);
  return x <= 0.5f ? isp_bezier4(0.0f, b, c, 0.5f, x * 2.0f) : 0;
}
// buildToneCurveLut (:382-416) with libm's powf / tanf
void isp_tone_lut(const derp_isp_config& k, bool enabled, std::vector<float>& lut) {
  lut.resize((size_t)kIspLutSize * 3);
  const float dx = 1.0f / float(kIspLutSize - 1);
  const float angle = M_PI * 0.25f * k.contrast;
  const float slope = tanf(angle);
  const float bias = 0.5f * (1.0f - slope);
  for (int i = 0; i < kIspLutSize; ++i) {
    const float x = dx * i;
    for (int c = 0; c < 3; ++c) {
      float y = x;
      if (enabled) {
        y = powf(x, k.gamma[c]);
        y = isp_low_key(k.low_key_boost[c], y) + isp_high_key(k.high_key_boost[c], y);
        y = isp_clamp(slope * y + bias, 0.0f, 1.0f);
      }
      lut[3 * i + c] = y;
    }
  }
}
// 3 x 3 product: the reference's is cv::gemm, whose rounding is its implementation's; here every element is
// accumulated in double and rounded to float once
void isp_mul3(const float* a, const float* b, float* out) {
  float r[9];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) {
        s += (double)a[3 * i + k] * (double)b[3 * k + j];
      }
      r[3 * i + j] = (float)s;
    }
  }
  memcpy(out, r, sizeof r);
}
// setup() :630-645: ccm^T * (yuv2rgb * sat * rgb2yuv) * 4095
void isp_composite_ccm(const derp_isp_config& k, float out[9]) {
  const float rgb2yuv[9] = {0.299f, 0.587f, 0.114f, -0.14713f, -0.28886f, 0.436f, 0.615f, -0.51499f, -0.10001f};
  const float yuv2rgb[9] = {1.0f, 0.0f, 1.13983f, 1.0f, -0.39465f, -0.58060f, 1.0f, 2.03211f, 0.0f};
  const float sat[9] = {1.0f, 0, 0, 0, k.saturation, 0, 0, 0, k.saturation};
  float m[9], t[9];
  isp_mul3(yuv2rgb, sat, m);
  isp_mul3(m, rgb2yuv, m);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      t[3 * i + j] = k.ccm[3 * j + i];
    }
  }
  isp_mul3(t, m, out);
  for (int i = 0; i < 9; ++i) {
    out[i] *= float(kIspLutSize - 1);
  }
}

// removeStuckPixels (:980-1059): a sequential in-place boustrophedon scan that reads what it replaced; host only
void isp_remove_stuck_pixels(float* raw, int width, int height, unsigned pat, const derp_isp_config& k) {
  struct Pval {
    float val;
    int i, j;
    bool operator<(const Pval& p) const { return val < p.val; }
  };
  const int radius = k.stuck_pixel_radius;
  std::vector<Pval> region;
  for (int i = 0; i < height; ++i) {
    const bool evenScanLine = (i % 2) == 0;
    const int jStart = evenScanLine ? 0 : width - 1;
    const int jEnd = evenScanLine ? width - 1 : 0;
    const int jStep = evenScanLine ? 1 : -1;
    for (int j = jStart; j != jEnd; j += jStep) {  // the last pixel of the scan line is skipped, as there
      const int mine = isp_color(pat, i, j);
      region.clear();
      float mean = 0.0f;
      for (int y = -radius; y <= radius; y++) {
        const int ip = isp_reflect(i + y, height);
        for (int x = -radius; x <= radius; x++) {
          const int jp = isp_reflect(j + x, width);
          if (isp_color(pat, ip, jp) == mine) {
            const Pval p{raw[(size_t)ip * width + jp], ip, jp};
            mean += p.val;
            region.push_back(p);
          }
        }
      }
      mean /= float(region.size());
      if (mean < k.stuck_pixel_darkness_threshold) {
        std::sort(region.begin(), region.end());
        for (int q = int(region.size()) - 1; q >= int(region.size()) - k.stuck_pixel_threshold && q >= 0; --q) {
          if (region[q].i == i && region[q].j == j) {
            raw[(size_t)i * width + j] = region[region.size() / 2].val;
            break;
          }
        }
      }
    }
  }
}

}  // namespace

struct derp_isp {
  int device = 0;
  derp_isp_config cfg;
  int filter = 0, resize = 1, w = 0, h = 0;
  unsigned pat = 0;
  bool sharpen = false, processed = false;
  IspLoad load;
  IspPixel pixel;
  IspCcm ccm;
  IspSharpen sharp;
  float alpha = 0;
  std::vector<float> vigH, vigV, lut;
  hipStream_t stream = nullptr;
  DevBuf in, raw0, raw1, raw2, dem, col, lp, shp, scr, gV, gH, bit, dVigH, dVigV, dLut, stale, out;
  std::vector<float> hostPlane;
  std::string* errSink() const {  // every derp_isp_* call reports through derp_last_error(nullptr)
    return &g_create_error;
  }
};

namespace {

// setup() :573-618; false for a pattern it does not know
bool isp_pattern(const char* bayer, unsigned* pat) {
  const std::string b(bayer);
  for (const char* known : {"RGGB", "GRBG", "GBRG", "BGGR"}) {
    if (b.find(known) != std::string::npos) {
      *pat = 0;
      for (int p = 0; p < 4; ++p) {
        *pat |= (unsigned)(known[p] == 'R' ? 0 : known[p] == 'G' ? 1 : 2) << (2 * p);
      }
      return true;
    }
  }
  return false;
}

}  // namespace

void derp_isp_config_default(derp_isp_config* k) {
  if (!k) {
    return;
  }
  memset(k, 0, sizeof *k);
  k->bits_per_pixel = 16;
  k->is_row_major = 1;
  strcpy(k->bayer_pattern, "GBRG");
  for (int c = 0; c < 3; ++c) {
    k->clamp_max[c] = 1.0f;
    k->rolloff_h[0][c] = 1.0f;
    k->rolloff_v[0][c] = 1.0f;
    k->white_balance_gain[c] = 1.0f;
    k->ccm[4 * c] = 1.0f;
    k->gamma[c] = 1.0f;
  }
  k->n_rolloff_h = 1;
  k->n_rolloff_v = 1;
  k->saturation = 1.0f;
  k->contrast = 1.0f;
  k->sharpening_support = 10.0f / 2048.0f;
  k->noise_core = 1000.0f;
  k->n_companding_lut = 2;
}

int derp_isp_create(derp_isp** out, int device, const derp_isp_config* cfg, int demosaic_filter, int pow2_downscale,
                    int apply_tone_curve) {
  if (!out) {
    return 1;
  }
  *out = nullptr;
  if (!cfg) {
    return create_fail("derp_isp_create: no config");
  }
  // ---- refusals, before anything is allocated
  if (demosaic_filter < 0 || demosaic_filter > DERP_ISP_CHROMA_SUPPRESSED) {  // setDemosaicFilter :949-953
    return create_fail("expecting Demosaic filter in [0,3]");
  }
  if (demosaic_filter == DERP_ISP_FREQUENCY) {
    return create_fail("frequency demosaic is not built (it needs a DCT of the whole plane)");
  }
  if (pow2_downscale != 1 && pow2_downscale != 2 && pow2_downscale != 4 && pow2_downscale != 8) {  // setResize :955-959
    return create_fail("expecting a resize value of 1, 2, 4, or 8. got " + std::to_string(pow2_downscale));
  }
  if (cfg->width <= 0 || cfg->height <= 0 || cfg->width % 2 || cfg->height % 2) {  // loadImageFromSensor :769-772
    return create_fail("sensor width and height must be even and non-zero");
  }
  if (cfg->bits_per_pixel != 8 && cfg->bits_per_pixel != 16) {  // RawUtil.cpp:111
    return create_fail("Unsupported precision: bitsPerPixel must be 8 or 16");
  }
  if ((size_t)cfg->width * cfg->height > ((size_t)1 << 28)) {
    return create_fail("sensor larger than 2^28 pixels");
  }
  unsigned pat = 0;
  if (strlen(cfg->bayer_pattern) != 4 || !isp_pattern(cfg->bayer_pattern, &pat)) {
    return create_fail("bayerPattern must be RGGB, GRBG, GBRG or BGGR");
  }
  int planeOf[4] = {0, 1, 2, 3};
  const bool planar = cfg->plane_order[0] != 0;
  if (planar) {
    // getPlaneOrderToBayerOrder :346-354, used at :821 as plane -> Bayer position; its inverse exists only when the
    // plane order is a permutation of the pattern
    const std::string order(cfg->plane_order), bayer(cfg->bayer_pattern);
    int map[4], seen = 0;
    bool foundFirstG = false;
    for (int i = 0; i < 4; ++i) {
      const size_t at = foundFirstG ? order.rfind(bayer[i]) : order.find(bayer[i]);
      map[i] = at == std::string::npos ? -1 : (int)at;
      foundFirstG |= bayer[i] == 'G';
    }
    for (int p = 0; p < 4; ++p) {
      if (order.size() == 4 && map[p] >= 0 && map[p] < 4) {
        planeOf[map[p]] = p;
        seen |= 1 << map[p];
      }
    }
    if (seen != 15) {
      return create_fail("planeOrder must hold the four letters of bayerPattern");
    }
  }
  if (cfg->n_rolloff_h < 1 || cfg->n_rolloff_h > DERP_ISP_MAX_ROLLOFF || cfg->n_rolloff_v < 1 ||
      cfg->n_rolloff_v > DERP_ISP_MAX_ROLLOFF) {
    return create_fail("vignetteRollOffH / vignetteRollOffV must hold 1.." + std::to_string((int)DERP_ISP_MAX_ROLLOFF) + " points");
  }
  if (cfg->stuck_pixel_threshold < 0 || cfg->stuck_pixel_radius < 0) {
    return create_fail("Check failed: stuckPixelThreshold >= 0");
  }
  const int w = cfg->width / pow2_downscale, h = cfg->height / pow2_downscale;  // setDimensions :1239-1245
  const int least = demosaic_filter == DERP_ISP_EDGE_AWARE ? 5 : 3;  // one reflection must stay inside the plane
  if (w < least || h < least || cfg->stuck_pixel_radius >= std::min(w, h)) {
    return create_fail("output of " + std::to_string(w) + " x " + std::to_string(h) + " is too small for this filter");
  }
  hipDeviceProp_t prop;
  TRY(open_device(device, "the ISP", &prop));
  std::unique_ptr<derp_isp> owner(new derp_isp);
  derp_isp* s = owner.get();
  s->device = device;
  s->cfg = *cfg;
  s->filter = demosaic_filter;
  s->resize = pow2_downscale;
  s->w = w;
  s->h = h;
  s->pat = pat;
  s->sharpen = cfg->sharpening[0] != 0.0 && cfg->sharpening[1] != 0.0 && cfg->sharpening[2] != 0.0;  // :1208
  IspLoad& L = s->load;
  L.sw = cfg->width;
  L.sh = cfg->height;
  L.w = w;
  L.h = h;
  L.resize = pow2_downscale;
  L.swap = cfg->is_little_endian ? 0 : 1;  // folly::Endian::big on a little-endian host
  L.planar = planar;
  L.rowMajor = cfg->is_row_major != 0;
  memcpy(L.planeOf, planeOf, sizeof planeOf);
  const int maxPixelValue = (1 << cfg->bits_per_pixel) - 1;
  L.areaRecip = 1.0f / (maxPixelValue * float(pow2_downscale * pow2_downscale));  // :326
  for (int c = 0; c < 3; ++c) {
    s->pixel.black[c] = cfg->black_level[c];
    s->pixel.blackScale[c] = 1.0f / (1.0f - cfg->black_level[c]);
    s->pixel.gain[c] = cfg->white_balance_gain[c];
    s->pixel.cmin[c] = cfg->clamp_min[c];
    s->pixel.cmax[c] = cfg->clamp_max[c];
    s->sharp.amount[c] = 1.0f + cfg->sharpening[c];
  }
  s->sharp.noiseCore = cfg->noise_core;
  s->alpha = powf(cfg->sharpening_support, 1.0f / 4.0f);  // Filter.h:42
  const int maxDimension = std::max(w, h);
  s->vigH.resize((size_t)w * 3);
  s->vigV.resize((size_t)h * 3);
  for (int x = 0; x < w; ++x) {  // curveHAtPixel :668-670
    isp_bezier(cfg->rolloff_h, 0, cfg->n_rolloff_h - 1, float(x) / float(maxDimension), &s->vigH[3 * x]);
  }
  for (int y = 0; y < h; ++y) {
    isp_bezier(cfg->rolloff_v, 0, cfg->n_rolloff_v - 1, float(y) / float(maxDimension), &s->vigV[3 * y]);
  }
  isp_composite_ccm(*cfg, s->ccm.m);
  isp_tone_lut(*cfg, apply_tone_curve != 0, s->lut);
  const size_t n = (size_t)w * h, plane = n * sizeof(float);
  const size_t inBytes = (size_t)cfg->width * cfg->height * (cfg->bits_per_pixel / 8);
  const bool stuck = cfg->stuck_pixel_radius > 0, ea = demosaic_filter == DERP_ISP_EDGE_AWARE;
  if (s->in.ensure(inBytes) || s->raw0.ensure(plane) || s->raw1.ensure(plane) || (stuck && s->raw2.ensure(plane)) ||
      s->dem.ensure(3 * plane) || s->col.ensure(3 * plane) ||
      (s->sharpen && (s->lp.ensure(3 * plane) || s->shp.ensure(3 * plane) || s->scr.ensure(3 * plane))) ||
      (ea && (s->gV.ensure(plane) || s->gH.ensure(plane) || s->bit.ensure(n))) || s->dVigH.ensure(s->vigH.size() * 4) ||
      s->dVigV.ensure(s->vigV.size() * 4) || s->dLut.ensure(s->lut.size() * 4) || s->stale.ensure(3 * sizeof(float)) ||
      s->out.ensure(3 * n * (cfg->bits_per_pixel / 8))) {
    return create_fail("out of device memory");
  }
  HIPCHK(s, hipMemcpy(s->dVigH.p, s->vigH.data(), s->vigH.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(s, hipMemcpy(s->dVigV.p, s->vigV.data(), s->vigV.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(s, hipMemcpy(s->dLut.p, s->lut.data(), s->lut.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(s, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  *out = owner.release();
  return 0;
}

void derp_isp_destroy(derp_isp* s) {
  if (!s) {
    return;
  }
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->stream);
  (void)hipStreamDestroy(s->stream);
  delete s;
}

int derp_isp_output_size(const derp_isp* s, int* width, int* height) {
  if (!s || !width || !height) {
    return create_fail("derp_isp_output_size: bad arguments");
  }
  *width = s->w;
  *height = s->h;
  return 0;
}

int derp_isp_process(derp_isp* s, const void* raw, size_t raw_bytes, void* out_bgr) {
  if (!s || !raw || !out_bgr) {
    return create_fail("derp_isp_process: bad arguments");
  }
  const derp_isp_config& k = s->cfg;
  const int bytes = k.bits_per_pixel / 8, w = s->w, h = s->h;
  const size_t inBytes = (size_t)k.width * k.height * bytes, n = (size_t)w * h;
  if (raw_bytes < inBytes) {  // readRawImage, RawUtil.cpp:37
    return create_fail("unexpected end of file: raw image holds " + std::to_string(raw_bytes) + " bytes, the sensor " +
                    std::to_string(inBytes));
  }
  HIPCHK(s, hipSetDevice(s->device));
  hipStream_t st = s->stream;
  s->processed = false;
  HIPCHK(s, hipMemcpyAsync(s->in.p, raw, inBytes, hipMemcpyHostToDevice, st));
  const dim3 b2(32, 8), g2((w + 31) / 32, (h + 7) / 8);
  const dim3 b16(16, 16), g16((w + 15) / 16, (h + 15) / 16);
  const unsigned g1 = blocks_of(n, 256);
  if (bytes == 1) {
    k_isp_load<uint8_t><<<g2, b2, 0, st>>>(s->in.as<uint8_t>(), s->raw0.as<float>(), s->load);
  } else {
    k_isp_load<uint16_t><<<g2, b2, 0, st>>>(s->in.as<uint16_t>(), s->raw0.as<float>(), s->load);
  }
  k_isp_pixel<<<g2, b2, 0, st>>>(s->raw0.as<float>(), s->raw1.as<float>(), s->dVigH.as<float>(), s->dVigV.as<float>(), w, h,
                                 s->pat, s->pixel);
  const float* mosaic = s->raw1.as<float>();
  if (k.stuck_pixel_radius > 0) {  // host, between two device phases
    s->hostPlane.resize(n);
    HIPCHK(s, hipMemcpyAsync(s->hostPlane.data(), s->raw1.p, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(s, hipStreamSynchronize(st));
    isp_remove_stuck_pixels(s->hostPlane.data(), w, h, s->pat, k);
    HIPCHK(s, hipMemcpyAsync(s->raw2.p, s->hostPlane.data(), n * 4, hipMemcpyHostToDevice, st));
    mosaic = s->raw2.as<float>();
  }
  const IspMosaic M{mosaic, w, h, s->pat};
  float* R = s->dem.as<float>();
  float* G = R + n;
  float* B = G + n;
  if (s->filter == DERP_ISP_BILINEAR) {
    k_isp_bilinear<<<g2, b2, 0, st>>>(M, R, G, B);
  } else {
    if (s->filter == DERP_ISP_EDGE_AWARE) {
      k_isp_ea_gradient<<<g2, b2, 0, st>>>(M, s->gV.as<float>(), s->gH.as<float>(), s->bit.as<unsigned char>());
      k_isp_ea_vote<<<g16, b16, 0, st>>>(s->bit.as<unsigned char>(), s->gV.as<float>(), s->gH.as<float>(), G, w, h);
    } else {
      k_isp_green_bilinear<<<g2, b2, 0, st>>>(M, G);
    }
    k_isp_chroma<<<g2, b2, 0, st>>>(M, G, R, B);
  }
  k_isp_color<<<g1, 256, 0, st>>>(s->dem.as<float>(), s->col.as<float>(), s->dLut.as<float>(), n, s->ccm);
  const float* last = s->col.as<float>();
  if (s->sharpen) {
    HIPCHK(s, hipMemsetAsync(s->stale.p, 0, 3 * sizeof(float), st));
    k_isp_iir_rows<<<dim3((h + 63) / 64, 3), 64, 0, st>>>(s->col.as<float>(), s->scr.as<float>(), s->lp.as<float>(),
                                                          s->stale.as<float>(), w, h, s->alpha);
    k_isp_iir_cols<<<dim3((w + 63) / 64, 3), 64, 0, st>>>(s->lp.as<float>(), s->scr.as<float>(), s->stale.as<float>(), w, h,
                                                          s->alpha);
    k_isp_sharpen<<<g1, 256, 0, st>>>(s->col.as<float>(), s->lp.as<float>(), s->shp.as<float>(), n, s->sharp);
    last = s->shp.as<float>();
  }
  if (bytes == 1) {
    k_isp_output<uint8_t><<<g1, 256, 0, st>>>(last, s->out.as<uint8_t>(), n, 255.0f);
  } else {
    k_isp_output<uint16_t><<<g1, 256, 0, st>>>(last, s->out.as<uint16_t>(), n, 65535.0f);
  }
  KCHECK(s);
  HIPCHK(s, hipMemcpyAsync(out_bgr, s->out.p, 3 * n * bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(s, hipStreamSynchronize(st));
  s->processed = true;
  return 0;
}

int derp_isp_stage(derp_isp* s, int stage, float* out) {
  if (!s || !out) {
    return create_fail("derp_isp_stage: bad arguments");
  }
  if (!s->processed) {
    return create_fail("derp_isp_stage: no image was processed yet");
  }
  const size_t plane = (size_t)s->w * s->h * sizeof(float);
  const void* src = nullptr;
  size_t bytes = plane;
  switch (stage) {
    case DERP_ISP_STAGE_LOAD: src = s->raw0.p; break;
    case DERP_ISP_STAGE_PIXEL: src = s->raw1.p; break;
    case DERP_ISP_STAGE_STUCK: src = s->cfg.stuck_pixel_radius > 0 ? s->raw2.p : s->raw1.p; break;
    case DERP_ISP_STAGE_DEMOSAIC: src = s->dem.p, bytes = 3 * plane; break;
    case DERP_ISP_STAGE_COLOR: src = s->col.p, bytes = 3 * plane; break;
    case DERP_ISP_STAGE_LOWPASS:
    case DERP_ISP_STAGE_SHARPENED:
      if (!s->sharpen) {
        return create_fail("derp_isp_stage: sharpening does not run with this config (a zero component)");
      }
      src = stage == DERP_ISP_STAGE_LOWPASS ? s->lp.p : s->shp.p;
      bytes = 3 * plane;
      break;
    default: return create_fail("derp_isp_stage: no such stage " + std::to_string(stage));
  }
  HIPCHK(s, hipSetDevice(s->device));
  HIPCHK(s, hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int derp_isp_tables(const derp_isp* s, float* vignette_h, float* vignette_v, float* ccm9, float* tone_lut) {
  if (!s) {
    return create_fail("derp_isp_tables: bad arguments");
  }
  if (vignette_h) {
    memcpy(vignette_h, s->vigH.data(), s->vigH.size() * sizeof(float));
  }
  if (vignette_v) {
    memcpy(vignette_v, s->vigV.data(), s->vigV.size() * sizeof(float));
  }
  if (ccm9) {
    memcpy(ccm9, s->ccm.m, sizeof s->ccm.m);
  }
  if (tone_lut) {
    memcpy(tone_lut, s->lut.data(), s->lut.size() * sizeof(float));
  }
  return 0;
}
