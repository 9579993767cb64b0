// GenerateKeypointProjections — drop-in for source/render/GenerateKeypointProjections.cpp: its four flags (:34-37), the
// calibration library's flags it reads (Calibration.cpp: color, frame, threads; FeatureMatcher.cpp: depth_max, depth_min,
// depth_samples, search_overlap, search_radius) and its output files, <output_dir>/<id0>_<id1>.png (8-bit BGRA) for
// every pair id0 before id1. Compute = derp_sweep_upload at scale 1 once, then derp_preview_keypoints per pair.
#include "sweep_io.h"

using namespace cli;

static const char* kUsage = R"(
   - Shows, pair by pair, where a grid of points of one camera lands in another over the depth range: every accepted
     depth sample of a grid point is a filled square of the point's colour, blended over the other camera's image.

   - Example:
     ./GenerateKeypointProjections \
     --color=/path/to/video/color \
     --frame=000000 \
     --rig=/path/to/rigs/rig.json \
     --output_dir=/path/to/output
)";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.dbl("height_stride", 0.125, "x grid stride in percent");
  F.dbl("length_stride", 0.125, "y grid stride in percent");
  F.str("output_dir", "", "path to output directory");
  F.str("rig", "", "path to camera rig .json file");
  F.str("color", "", "path to input data");
  F.str("frame", "", "frame to process (lexical)");
  F.i32("threads", -1, "number of threads (-1 = max allowed, 0 = no threading)");
  F.dbl("depth_max", 100.0, "max depth in m");
  F.dbl("depth_min", 1.0, "min depth in m");
  F.dbl("depth_samples", 1000, "number of depths to sample");
  F.dbl("search_overlap", 0.25, "overlap fraction between search windows at different disparities");
  F.i32("search_radius", 100, "search radius in pixels");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("rig") != "", "rig");
  CHECK_MSG(F.s("output_dir") != "", "output_dir");
  CHECK_MSG(F.s("color") != "", "color");
  CHECK_MSG(F.s("frame") != "", "frame");
  const double ls = F.d("length_stride"), hs = F.d("height_stride");
  CHECK_MSG(ls > 0 && std::isfinite(ls), "length_stride must be a positive finite number (the reference loops forever)");
  CHECK_MSG(hs > 0 && std::isfinite(hs), "height_stride must be a positive finite number (the reference loops forever)");
  CHECK_MSG((std::floor(1 / ls) + 2) * (std::floor(1 / hs) + 2) <= 1048576.0,
            fmt("strides of %g x %g make more than 1048576 grid points", ls, hs));
  CHECK_MSG(F.i("search_radius") >= 0, "search_radius >= 0");
  CHECK_MSG(F.d("depth_samples") >= 2, "depth_samples >= 2");
  CHECK_MSG(F.d("depth_min") > 0, "depth_min > 0");
  CHECK_MSG(F.d("depth_max") >= F.d("depth_min") && std::isfinite(F.d("depth_max")), "depth_max >= depth_min");
  CHECK_MSG(F.d("search_overlap") >= 0, "search_overlap >= 0");
  const std::vector<derp_camera_desc> rig = load_rig(F.s("rig"));
  CHECK_MSG(!rig.empty(), "rig.size() > 0");
  verify_image_paths(F.s("color"), rig, F.s("frame"), F.s("frame"));
  for (const derp_camera_desc& cam : rig) {  // the reference's addWeighted throws on sizes that differ
    int w = 0, h = 0;
    const fs::path path = image_path(F.s("color"), cam.id, F.s("frame"));
    CHECK_MSG(image_size(path, w, h), "cannot read " + path.string());
    CHECK_MSG((double)w == rig[0].resolution[0] && (double)h == rig[0].resolution[1],
              fmt("the image of %s is %d x %d, not the first camera's resolution %g x %g", cam.id, w, h, rig[0].resolution[0],
                  rig[0].resolution[1]));
  }
  const int n = (int)rig.size();
  const double params[7] = {ls, hs, F.d("depth_min"), F.d("depth_max"), F.d("depth_samples"), F.d("search_overlap"),
                            (double)F.i("search_radius")};

  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), n, rig.data(), n) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  IoPool pool(F.i("threads") == 0 ? 1 : F.i("threads"));
  LOG_INFO("Loading images...");
  std::vector<int> w, h;
  sweep_load_and_upload(ctx, pool, F.s("color"), rig, F.s("frame"), 1.0, w, h);
  fs::create_directories(F.s("output_dir"));
  for (int c0 = 0; c0 < n; ++c0) {
    for (int c1 = c0 + 1; c1 < n; ++c1) {
      std::vector<uint8_t> out((size_t)w[c0] * h[c0] * 4);
      int rects = 0;
      DERP_OK(ctx, derp_preview_keypoints(ctx, c0, c1, params, out.data(), nullptr, &rects));
      const fs::path fn = fs::path(F.s("output_dir")) / (std::string(rig[c0].id) + "_" + rig[c1].id + ".png");
      LOG_INFO(fmt("%s: %d rectangles", fn.filename().c_str(), rects));
      write_png_bgra8(fn, out.data(), w[c0], h[c0]);
    }
  }
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
