// GeometricConsistency's output files (source/render/GeometricConsistency.cpp:64-70, dump): a depth map as <path>.pfm and,
// for convenience, 1 m / depth as <path>_disparity.png through cv_util::convertTo<uint16_t> (CvUtil.h:196-220).
#pragma once
#include "cli_common.h"

namespace cli {

// `cv::Mat_<float> disparity = 1.0 / mat`: the scalar is narrowed to the matrix's type first, so a float division.
// convertTo<uint16_t> of a float image is convertTo(CV_16U, 65535 / 1.0): the product in fp32, rounded to the nearest
// integer with halves to even, saturated to 0 .. 65535; a NaN depth (every rejected or edge pixel) gives 0
// (write_disparity_png). Depths nearer than 1 m saturate at 65535.
inline std::vector<float> gc_depth_to_disparity(const float* depth, size_t n) {
  std::vector<float> disparity(n);
  for (size_t i = 0; i < n; ++i) {
    disparity[i] = 1.0f / depth[i];
  }
  return disparity;
}

inline void gc_dump(const fs::path& path, const float* depth, int w, int h) {
  write_pfm(path.string() + ".pfm", depth, w, h);
  write_disparity_png(path.string() + "_disparity.png", gc_depth_to_disparity(depth, (size_t)w * h).data(), w, h);
}

// downscale() (:324-331): round(resolution / downscale), halves away from zero (Eigen's array().round())
inline void gc_small_size(const derp_camera_desc& cam, double downscale, int& w, int& h) {
  w = (int)std::round(cam.resolution[0] / downscale);
  h = (int)std::round(cam.resolution[1] / downscale);
}

}  // namespace cli
