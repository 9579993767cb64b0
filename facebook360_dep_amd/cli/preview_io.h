// What the tuning previews (ViewColorVarianceThresholds, ViewForegroundMaskThresholds) share on the host: the comma lists
// that stand in for the sliders, the reference's scale of the loaded image, the 16-bit RGB file of a BGR matrix and
// thresholds.json. Nothing here opens a device.
#pragma once
#include "cli_common.h"

namespace cli {

constexpr int kPreviewMaxImages = 256;  // derp_preview_*'s cap on the settings of one call

// "2,50,100" -> {2, 50, 100}; every entry a whole number in lo..hi, or the run ends by the flag's name
inline std::vector<int> preview_int_list(const std::string& flag, const std::string& text, int lo, int hi) {
  std::vector<int> out;
  size_t at = 0;
  while (at <= text.size()) {
    const size_t comma = std::min(text.find(',', at), text.size());
    const std::string tok = text.substr(at, comma - at);
    char* end = nullptr;
    errno = 0;
    const long long v = strtoll(tok.c_str(), &end, 10);
    if (tok.empty() || !end || *end || errno == ERANGE || tok.find_first_not_of("0123456789") != std::string::npos) {
      LOG_FATAL("--" + flag + ": '" + tok + "' is not an integer (a comma list of integers " + std::to_string(lo) + ".." +
                std::to_string(hi) + " is expected)");
    }
    if (v < lo || v > hi) {
      LOG_FATAL("--" + flag + ": " + tok + " is outside " + std::to_string(lo) + ".." + std::to_string(hi));
    }
    out.push_back((int)v);
    at = comma + 1;
  }
  return out;
}

// the constructor's scale (ViewColorVarianceThresholds.cpp:92, ViewForegroundMaskThresholds.cpp:96) and scaleImage's
// size (CvUtil.h:151-154); an integer image is not enlarged by the INTER_AREA resize here, so that is refused by name
inline double preview_scale(int width, int cols, int rows, int& outW, int& outH) {
  const double scale = width > 0 ? double(width) / cols : 1.0;
  if (width > cols) {
    LOG_FATAL(fmt("--width=%d would be enlarging the %d x %d image: only --width <= the image's width (or 0) is supported",
                  width, cols, rows));
  }
  outW = width > 0 ? (int)std::round(cols * scale) : cols;
  outH = width > 0 ? (int)std::round(rows * scale) : rows;
  CHECK_MSG(outW >= 1 && outH >= 1, fmt("--width=%d leaves an empty image", width));
  return scale;
}

inline std::vector<uint16_t> preview_load(const std::string& flag, const std::string& path, int& w, int& h) {
  if (!fs::is_regular_file(path)) {
    LOG_FATAL("Missing file: " + path + " (--" + flag + ")");
  }
  return load_color_bgr16(path, w, h);
}

// the image scaled as the reference scales it: the image itself when the size matches (resizeImage, CvUtil.h:140-147)
inline std::vector<uint16_t> preview_resize(derp_ctx* ctx, const std::vector<uint16_t>& img, int w, int h, int outW, int outH) {
  if (w == outW && h == outH) {
    return img;
  }
  std::vector<uint16_t> out((size_t)outW * outH * 3);
  DERP_OK(ctx, derp_resize_area(ctx, 0, img.data(), w, h, out.data(), outW, outH));
  return out;
}

// a context needs a camera; these tools read none
inline derp_camera_desc preview_camera() {
  derp_camera_desc c;
  memset(&c, 0, sizeof c);
  c.type = DERP_FTHETA;
  snprintf(c.id, sizeof c.id, "preview");
  c.forward[2] = -1;
  c.up[1] = 1;
  c.right[0] = 1;
  c.resolution[0] = c.resolution[1] = 2;
  c.focal[0] = 1;
  c.focal[1] = -1;
  return c;
}

// the matrix the reference hands to imshow, B, G, R uint16, as a 16-bit RGB PNG
inline void preview_write_rgb16(const fs::path& path, const uint16_t* bgr, int w, int h) {
  std::vector<uint16_t> rgb((size_t)w * h * 3);
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    rgb[3 * i] = bgr[3 * i + 2];
    rgb[3 * i + 1] = bgr[3 * i + 1];
    rgb[3 * i + 2] = bgr[3 * i];
  }
  write_png(path, rgb.data(), w, h, 3, 16);
}

inline void preview_write_json(const fs::path& path, const std::vector<std::string>& entries) {
  std::ofstream f(path);
  f << "{\n \"images\": [\n";
  for (size_t i = 0; i < entries.size(); ++i) {
    f << "  {" << entries[i] << "}" << (i + 1 < entries.size() ? "," : "") << "\n";
  }
  f << " ]\n}\n";
  CHECK_MSG(f.good(), "failed to write: " + path.string());
}

}  // namespace cli
