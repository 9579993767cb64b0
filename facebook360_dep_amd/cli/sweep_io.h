// What GenerateCameraOverlaps and GenerateEquirect share: loadScaledImages<cv::Vec4f> (ImageUtil.h, CvUtil.h:139-154),
// the 8-bit BGRA PNG of `255.0f * image`, and the slab pipeline that encodes one slab of depths while the device computes
// the next. Definitions: DESIGN §8.7.
#pragma once
#include "cli_common.h"

namespace cli {

// the 8-bit output of one slab of depths stays within this many bytes of host memory (two slabs are alive at a time)
constexpr size_t kSweepSlabBytes = (size_t)256 << 20;

struct SweepImage {
  std::vector<float> bgra;  // [h][w][4]
  int w = 0, h = 0;
};

// scaleImage's size (CvUtil.h:151-154): std::round of the product
inline void sweep_scaled_size(int w, int h, double scale, int& sw, int& sh) {
  sw = (int)std::round(w * scale);
  sh = (int)std::round(h * scale);
}

// loadImage<cv::Vec4f>: the 8- or 16-bit file as 16-bit BGRA (alpha 65535 where it has none) times 1 / 65535 in float.
// Parity unpinned to OpenCV (its convertTo of an 8-bit file multiplies by 1 / 255).
inline SweepImage sweep_load_bgra_f32(const fs::path& path) {
  SweepImage im;
  const std::vector<uint16_t> px = load_color_bgra16(path, im.w, im.h);
  im.bgra.resize(px.size());
  const float k = 1.0f / 65535.0f;
  for (size_t i = 0; i < px.size(); ++i) {
    im.bgra[i] = (float)px[i] * k;
  }
  return im;
}

// scaleImage(image, scale), INTER_AREA (CvUtil.h:139-154) through the library's float area resize: the three colours
// together and the alpha on its own (cv::resize treats channels alike). Untouched when the size does not change.
// Runs on the thread that owns the context.
inline SweepImage sweep_scale_image(derp_ctx* ctx, const SweepImage& in, double scale) {
  int sw, sh;
  sweep_scaled_size(in.w, in.h, scale, sw, sh);
  CHECK_MSG(sw >= 1 && sh >= 1, fmt("an image of %d x %d scaled by %g has no pixels", in.w, in.h, scale));
  if (sw == in.w && sh == in.h) {
    return in;
  }
  const size_t n = (size_t)in.w * in.h, m = (size_t)sw * sh;
  std::vector<float> bgr(n * 3), alpha(n), bgrS(m * 3), alphaS(m);
  for (size_t i = 0; i < n; ++i) {
    bgr[3 * i] = in.bgra[4 * i];
    bgr[3 * i + 1] = in.bgra[4 * i + 1];
    bgr[3 * i + 2] = in.bgra[4 * i + 2];
    alpha[i] = in.bgra[4 * i + 3];
  }
  DERP_OK(ctx, derp_resize_area(ctx, 3, bgr.data(), in.w, in.h, bgrS.data(), sw, sh));
  DERP_OK(ctx, derp_resize_area(ctx, 2, alpha.data(), in.w, in.h, alphaS.data(), sw, sh));
  SweepImage out;
  out.w = sw;
  out.h = sh;
  out.bgra.resize(m * 4);
  for (size_t i = 0; i < m; ++i) {
    out.bgra[4 * i] = bgrS[3 * i];
    out.bgra[4 * i + 1] = bgrS[3 * i + 1];
    out.bgra[4 * i + 2] = bgrS[3 * i + 2];
    out.bgra[4 * i + 3] = alphaS[i];
  }
  return out;
}

// loadScaledImages<cv::Vec4f>(dir, rig, frame, scale) + Camera::rescale(resolution * scale) + derp_sweep_upload: the
// files are decoded on the pool, resized and uploaded on the calling thread -> the images' sizes
inline void sweep_load_and_upload(derp_ctx* ctx, IoPool& pool, const std::string& color, const std::vector<derp_camera_desc>& rig,
                                  const std::string& frame, double scale, std::vector<int>& w, std::vector<int>& h) {
  const int n = (int)rig.size();
  std::vector<SweepImage> images(n);
  parallel_rows(pool, n, [&](int a, int b) {
    for (int i = a; i < b; ++i) {
      images[i] = sweep_load_bgra_f32(image_path(color, rig[i].id, frame));
    }
  });
  std::vector<const float*> ptrs(n);
  std::vector<double> res(2 * n);
  w.resize(n);
  h.resize(n);
  for (int i = 0; i < n; ++i) {
    images[i] = sweep_scale_image(ctx, images[i], scale);
    ptrs[i] = images[i].bgra.data();
    w[i] = images[i].w;
    h[i] = images[i].h;
    res[2 * i] = rig[i].resolution[0] * scale;  // (not rounded: the camera and its image can differ by a fraction)
    res[2 * i + 1] = rig[i].resolution[1] * scale;
  }
  DERP_OK(ctx, derp_sweep_upload(ctx, ptrs.data(), w.data(), h.data(), res.data()));
}

// cv::imwrite of a four-channel 8-bit image: B, G, R, A in memory, R, G, B, A in the file
inline void write_png_bgra8(const fs::path& path, const uint8_t* bgra, int w, int h) {
  std::vector<uint16_t> rgba((size_t)w * h * 4);
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    rgba[4 * i] = bgra[4 * i + 2];
    rgba[4 * i + 1] = bgra[4 * i + 1];
    rgba[4 * i + 2] = bgra[4 * i];
    rgba[4 * i + 3] = bgra[4 * i + 3];
  }
  write_png(path, rgba.data(), w, h, 4, 8);
}

// depths per slab for images of w x h
inline int sweep_slab_depths(int w, int h, int total) {
  const size_t per = (size_t)w * h * 4;
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)total, kSweepSlabBytes / per));
}

// The slab pipeline: compute(first, count, out) fills `count` 8-bit images of w x h for list entries first.. on the calling
// thread (the device), while the pool encodes the slab before it. name(k) is entry k's file. Entries that share a file:
// the later one in list order wins, so only the last entry of each name is written.
inline void sweep_run_slabs(IoPool& pool, int total, int w, int h, const std::function<void(int, int, uint8_t*)>& compute,
                            const std::function<fs::path(int)>& name) {
  std::vector<char> last(total, 1);
  {
    std::map<std::string, int> seen;
    for (int k = total - 1; k >= 0; --k) {
      last[k] = seen.emplace(name(k).string(), k).second;
    }
  }
  const int slab = sweep_slab_depths(w, h, total);
  const size_t image = (size_t)w * h * 4;
  std::vector<uint8_t> buf[2];
  IoBatch batch[2];
  int which = 0;
  for (int first = 0; first < total; first += slab, which ^= 1) {
    const int count = std::min(slab, total - first);
    batch[which].wait();  // the slab that used this buffer two rounds ago is on disk
    buf[which].resize(image * count);
    compute(first, count, buf[which].data());
    const uint8_t* base = buf[which].data();
    for (int k = 0; k < count; ++k) {
      if (last[first + k]) {
        const fs::path file = name(first + k);
        batch[which].add(pool, [=] { write_png_bgra8(file, base + image * k, w, h); });
      }
    }
  }
  batch[0].wait();
  batch[1].wait();
}

}  // namespace cli
