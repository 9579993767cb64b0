// ViewColorVarianceThresholds — the headless form of source/render/ViewColorVarianceThresholds.cpp: the reference opens
// a window with two trackbars; here --low_sliders x --high_sliders name the trackbar positions, and every pair's marked
// image (the matrix the reference hands to imshow) is written to --output with thresholds.json beside it.
// Compute = derp_resize_area (INTER_AREA to --width) + derp_preview_variance_levels + derp_preview_variance.
#include "preview_io.h"

using namespace cli;

static const char* kUsage = R"(
   - Marks, on one colour image, the pixels whose variance DerpCLI would floor (blue: below --var_noise_floor scaled to
     the loaded width) or ignore (purple: above --var_high_thresh), for every pair of slider positions 0..100 given in
     --low_sliders and --high_sliders. No window is opened: the images go to --output as
     low_LLL_high_HHH.png (16-bit RGB), and thresholds.json lists the flags to pass on and the pixel counts.

   - Example:
     ./ViewColorVarianceThresholds \
     --fullsize_image=/path/to/video/color/cam0/000000.png \
     --width=2048 \
     --low_sliders=0,2,10 --high_sliders=2,50 \
     --output=/path/to/preview
)";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("fullsize_image", "", "path to full-size RGB image (required)");
  F.dbl("var_high_max", 5e-2, "max high variance allowed");
  F.dbl("var_low_max", 4e-3, "max low variance allowed");
  F.i32("width", 2048, "loaded image width (0 = original size)");
  F.str("output", "", "[extension] directory the marked images and thresholds.json are written to (required)");
  // the positions the reference's window opens at: int(1e-4 / 4e-3 * 100) and int(1e-3 / 5e-2 * 100)
  F.str("low_sliders", "2", "[extension] comma list of --var_noise_floor trackbar positions, integers 0..100");
  F.str("high_sliders", "2", "[extension] comma list of --var_high_thresh trackbar positions, integers 0..100");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("fullsize_image") != "", "fullsize_image");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.d("var_low_max") > 0, "var_low_max > 0");
  CHECK_MSG(F.d("var_high_max") > 0, "var_high_max > 0");
  CHECK_MSG(F.i("width") >= 0, "width >= 0");
  const std::vector<int> lows = preview_int_list("low_sliders", F.s("low_sliders"), 0, 100);
  const std::vector<int> highs = preview_int_list("high_sliders", F.s("high_sliders"), 0, 100);
  const size_t n = lows.size() * highs.size();
  CHECK_MSG(n <= (size_t)kPreviewMaxImages, fmt("%zu slider pairs: at most %d are rendered by one run", n, kPreviewMaxImages));
  int w = 0, h = 0, outW = 0, outH = 0;
  const std::vector<uint16_t> full = preview_load("fullsize_image", F.s("fullsize_image"), w, h);
  const double scale = preview_scale(F.i("width"), w, h, outW, outH);

  // TrackVar takes the maxima as floats (:84-89)
  const float varLowMax = (float)F.d("var_low_max"), varHighMax = (float)F.d("var_high_max");
  std::vector<float> lowShow(n), highShow(n), floorOf(n), threshOf(n);
  for (size_t a = 0, k = 0; a < lows.size(); ++a) {
    for (size_t b = 0; b < highs.size(); ++b, ++k) {
      float lv[4];
      CHECK_MSG(derp_preview_variance_levels(varLowMax, varHighMax, lows[a], highs[b], scale, lv) == 0, derp_last_error(nullptr));
      floorOf[k] = lv[0];
      threshOf[k] = lv[1];
      lowShow[k] = lv[2];
      highShow[k] = lv[3];
    }
  }

  derp_ctx* ctx = nullptr;
  const derp_camera_desc cam = preview_camera();
  if (derp_create(&ctx, F.i("device"), &cam, 1, &cam, 1) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  const std::vector<uint16_t> image = preview_resize(ctx, full, w, h, outW, outH);
  const size_t px = (size_t)outW * outH;
  std::vector<uint16_t> marked(n * px * 3);
  std::vector<uint32_t> counts(2 * n);
  DERP_OK(ctx, derp_preview_variance(ctx, image.data(), outW, outH, lowShow.data(), highShow.data(), (int)n, marked.data(),
                                     counts.data(), nullptr));
  derp_destroy(ctx);

  const fs::path dir(F.s("output"));
  fs::create_directories(dir);
  std::vector<std::string> entries;
  for (size_t a = 0, k = 0; a < lows.size(); ++a) {
    for (size_t b = 0; b < highs.size(); ++b, ++k) {
      const std::string name = fmt("low_%03d_high_%03d.png", lows[a], highs[b]);
      preview_write_rgb16(dir / name, marked.data() + k * px * 3, outW, outH);
      // the two lines the reference logs on exit (:133-134)
      const std::string lowFlag = fmt("--var_noise_floor=%.3e", floorOf[k]), highFlag = fmt("--var_high_thresh=%.3e", threshOf[k]);
      LOG_INFO(name + ": " + lowFlag + " " + highFlag + fmt(" (%u blue, %u purple of %zu pixels)", counts[2 * k], counts[2 * k + 1], px));
      entries.push_back(fmt("\"file\": \"%s\", \"low_slider\": %d, \"high_slider\": %d, \"var_noise_floor\": \"%s\", "
                            "\"var_high_thresh\": \"%s\", \"blue\": %u, \"purple\": %u, \"width\": %d, \"height\": %d",
                            name.c_str(), lows[a], highs[b], lowFlag.c_str(), highFlag.c_str(), counts[2 * k],
                            counts[2 * k + 1], outW, outH));
    }
  }
  preview_write_json(dir / "thresholds.json", entries);
  return EXIT_SUCCESS;
}
