// GenerateEquirect — drop-in for source/render/GenerateEquirect.cpp: same flags (:41-54) and output files
// (<output>/equirect/<depth in cm, five digits>_cm.png, 8-bit BGRA). Compute = derp_rig_center (--camera_id, host),
// derp_sweep_upload once, then derp_sweep_equirect per slab of depths (or, with --crop_equirect, per depth behind
// derp_sweep_equirect_bounds), with the PNGs of one slab encoded while the next is computed. The depth label the
// reference draws into the image (cv::putText) is not drawn: the depth is in the file's name.
#include "sweep_io.h"

using namespace cli;

static const char* kUsage = R"(
  - Generates an equirect from a set of color images at a uniformly spaced range of depths.

  - The reference draws each depth into its image as a text label (cv::putText); this build does not: the depth is in
  the file name, <output>/equirect/<depth in cm>_cm.png. Two depths with one name: the later one wins.

  - Example:
    ./GenerateEquirect \
    --color=/path/to/video/color \
    --output=/path/to/output \
    --rig=/path/to/rigs/rig.json \
    --frame=000000 \
    --depth_min=1.0 \
    --depth_max=1000.0 \
    --num_depths=50
  )";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.boolean("black_bg", false, "set the background to be optionally black (red by default)");
  F.str("camera_id", "", "id of camera selected to be centered");
  F.str("cameras", "", "cameras to render (comma-separated)");
  F.str("color", "", "path to input color images (required)");
  F.boolean("crop_equirect", false, "crop the equirect to only include visible images");
  F.dbl("depth_max", 10.0, "max depth in m");
  F.dbl("depth_min", 1.0, "min depth in m");
  F.str("frame", "000000", "frame to process (lexical)");
  F.u64("height", 512, "equirect height in pixels");
  F.u64("num_depths", 50, "num depths");
  F.str("output", "", "path to output directory (required)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.dbl("scale", 1, "image scale factor");
  F.i32("threads", -1, "number of threads (-1 = max allowed, 0 = no threading)");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("color") != "", "color");
  CHECK_MSG(F.s("rig") != "", "rig");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.d("scale") > 0 && F.d("scale") <= 1, "scale in (0, 1]: INTER_AREA upscaling is not restated");
  CHECK_MSG(F.ull("num_depths") >= 1 && F.ull("num_depths") <= 1000000, "num_depths >= 1");
  CHECK_MSG(F.d("depth_min") > 0 && F.d("depth_max") > 0, "depth > 0");
  CHECK_MSG(F.ull("height") >= 1 && F.ull("height") <= 16384, "height in 1 .. 16384");
  std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(!rig.empty(), "rig.size() > 0");
  const int n = (int)rig.size();
  if (!F.s("camera_id").empty()) {
    int index = 0;
    while (index < n && F.s("camera_id") != rig[index].id) {
      ++index;
    }
    CHECK_MSG(index < n, "Camera id " + F.s("camera_id") + " not found");
    std::vector<derp_camera_desc> centred(n);
    if (derp_rig_center(rig.data(), n, index, centred.data()) != 0) {
      LOG_FATAL(std::string(derp_last_error(nullptr)));
    }
    rig = centred;
  }
  verify_image_paths(F.s("color"), rig, F.s("frame"), F.s("frame"));
  const int num = (int)F.ull("num_depths"), H = (int)F.ull("height"), W = 2 * H;
  std::vector<float> depths(num);
  std::vector<int> stems(num);
  if (derp_sweep_equirect_depths(num, F.d("depth_min"), F.d("depth_max"), depths.data(), stems.data()) != 0) {
    LOG_FATAL(std::string(derp_last_error(nullptr)));
  }

  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), n, rig.data(), n) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  IoPool pool(F.i("threads") == 0 ? 1 : F.i("threads"));  // (0 = no threading: one worker behind the device)
  LOG_INFO("Loading images...");
  std::vector<int> w, h;
  sweep_load_and_upload(ctx, pool, F.s("color"), rig, F.s("frame"), F.d("scale"), w, h);
  const fs::path dir = fs::path(F.s("output")) / "equirect";
  fs::create_directories(dir);
  const float background[4] = {0, 0, F.b("black_bg") ? 0.0f : 1.0f, 1};
  const auto name = [&](int k) { return dir / fmt("%05d_cm.png", stems[k]); };
  if (!F.b("crop_equirect")) {
    sweep_run_slabs(
        pool, num, W, H,
        [&](int first, int count, uint8_t* out) {
          DERP_OK(ctx, derp_sweep_equirect(ctx, W, H, nullptr, W, H, depths.data() + first, count, background, DERP_SWEEP_U8, out));
        },
        name);
  } else {
    // every depth has its own window and width: computed and written one at a time, not overlapped
    for (int k = 0; k < num; ++k) {
      bool later = false;  // a later depth has this file's name: it wins
      for (int j = k + 1; j < num && !later; ++j) {
        later = stems[j] == stems[k];
      }
      int bounds[4], newW = 0;
      DERP_OK(ctx, derp_sweep_equirect_bounds(ctx, W, H, depths[k], bounds));
      if (derp_sweep_crop_size(H, bounds, &newW) != 0) {
        LOG_FATAL(fmt("depth %g m: ", (double)depths[k]) + derp_last_error(nullptr));
      }
      CHECK_MSG((size_t)newW * H * 4 <= kSweepSlabBytes, fmt("cropped width %d is beyond the output budget", newW));
      if (later) {
        continue;
      }
      sweep_run_slabs(
          pool, 1, newW, H,
          [&](int, int, uint8_t* out) {
            DERP_OK(ctx, derp_sweep_equirect(ctx, W, H, bounds, newW, H, &depths[k], 1, background, DERP_SWEEP_U8, out));
          },
          [&](int) { return name(k); });
    }
  }
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
