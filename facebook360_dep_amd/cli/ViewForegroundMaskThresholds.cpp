// ViewForegroundMaskThresholds — the headless form of source/render/ViewForegroundMaskThresholds.cpp: the reference
// opens a window with three trackbars; here --blur_radii x --threshold_sliders x --closing_sizes name their positions,
// and every triple's overlay (the matrix the reference hands to imshow) is written to --output with thresholds.json.
// Compute = derp_resize_area (INTER_AREA to --width) + derp_preview_foreground.
#include "preview_io.h"

using namespace cli;

static const char* kUsage = R"(
   - Lays the foreground mask GenerateForegroundMasks would produce, in green, over the foreground image, for every
     triple of --blur_radii, --threshold_sliders (positions 0..100, threshold = position / 100) and --closing_sizes.
     No window is opened: the overlays go to --output as blur_BB_thresh_TTT_close_CC.png (16-bit RGB), and
     thresholds.json lists the flags to pass to GenerateForegroundMasks and the foreground amounts.

   - Example:
     ./ViewForegroundMaskThresholds \
     --fullsize_bg_image=/path/to/background/color/cam0/000000.png \
     --fullsize_fg_image=/path/to/video/color/cam0/000000.png \
     --blur_radii=0,1 --threshold_sliders=2,4,8 --closing_sizes=0,4 \
     --output=/path/to/preview
)";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.i32("blur_radius_max", 20, "max Gaussian blur radius allowed");
  F.str("fullsize_bg_image", "", "path to full-size RGB background image (required)");
  F.str("fullsize_fg_image", "", "path to full-size RGB foreground image (required)");
  F.i32("morph_closing_size_max", 20, "max morphological closing size allowed");
  F.i32("width", 2048, "loaded image width (0 = original size)");
  F.str("output", "", "[extension] directory the overlays and thresholds.json are written to (required)");
  // the positions the reference's window opens at (:91): blur 1, threshold 0.04 of 1.0, closing 4
  F.str("blur_radii", "1", "[extension] comma list of --blur_radius trackbar positions, integers 0..min(blur_radius_max, 3): larger Gaussian kernels are not built");
  F.str("threshold_sliders", "4", "[extension] comma list of --threshold trackbar positions, integers 0..100");
  F.str("closing_sizes", "4", "[extension] comma list of --morph_closing_size trackbar positions, integers 0..morph_closing_size_max");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("fullsize_bg_image") != "", "fullsize_bg_image");
  CHECK_MSG(F.s("fullsize_fg_image") != "", "fullsize_fg_image");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.i("blur_radius_max") > 0, "blur_radius_max > 0");
  CHECK_MSG(F.i("morph_closing_size_max") > 0, "morph_closing_size_max > 0");
  CHECK_MSG(F.i("width") >= 0, "width >= 0");
  const std::vector<int> blurs = preview_int_list("blur_radii", F.s("blur_radii"), 0, F.i("blur_radius_max"));
  for (int b : blurs) {  // derp_generate_foreground_mask's limit, refused here before a device is opened
    CHECK_MSG(b <= 3, fmt("--blur_radii: a blur radius of %d is not supported (0..3 are built)", b));
  }
  const std::vector<int> sliders = preview_int_list("threshold_sliders", F.s("threshold_sliders"), 0, 100);
  const std::vector<int> closings = preview_int_list("closing_sizes", F.s("closing_sizes"), 0, F.i("morph_closing_size_max"));
  const size_t n = blurs.size() * sliders.size() * closings.size();
  CHECK_MSG(n <= (size_t)kPreviewMaxImages, fmt("%zu slider triples: at most %d are rendered by one run", n, kPreviewMaxImages));
  int w = 0, h = 0, fw = 0, fh = 0, outW = 0, outH = 0;
  const std::vector<uint16_t> bgFull = preview_load("fullsize_bg_image", F.s("fullsize_bg_image"), w, h);
  const std::vector<uint16_t> fgFull = preview_load("fullsize_fg_image", F.s("fullsize_fg_image"), fw, fh);
  CHECK_MSG(w == fw && h == fh, fmt("imageBg.size() == imageFg.size() (%d x %d vs. %d x %d)", w, h, fw, fh));
  preview_scale(F.i("width"), w, h, outW, outH);
  std::vector<float> thresholds(sliders.size());
  for (size_t i = 0; i < sliders.size(); ++i) {
    const float threshMax = 1.0f;
    thresholds[i] = threshMax * sliders[i] / 100;  // (:72)
  }

  derp_ctx* ctx = nullptr;
  const derp_camera_desc cam = preview_camera();
  if (derp_create(&ctx, F.i("device"), &cam, 1, &cam, 1) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  const std::vector<uint16_t> bg = preview_resize(ctx, bgFull, w, h, outW, outH);
  const std::vector<uint16_t> fg = preview_resize(ctx, fgFull, w, h, outW, outH);
  const size_t px = (size_t)outW * outH;
  std::vector<uint16_t> overlays(n * px * 3);
  std::vector<uint32_t> counts(n);
  DERP_OK(ctx, derp_preview_foreground(ctx, bg.data(), fg.data(), outW, outH, blurs.data(), (int)blurs.size(), thresholds.data(),
                                       (int)thresholds.size(), closings.data(), (int)closings.size(), overlays.data(), nullptr,
                                       counts.data()));
  derp_destroy(ctx);

  const fs::path dir(F.s("output"));
  fs::create_directories(dir);
  std::vector<std::string> entries;
  size_t k = 0;
  for (int blur : blurs) {
    for (size_t t = 0; t < sliders.size(); ++t) {
      for (int closing : closings) {
        const std::string name = fmt("blur_%02d_thresh_%03d_close_%02d.png", blur, sliders[t], closing);
        preview_write_rgb16(dir / name, overlays.data() + k * px * 3, outW, outH);
        // the three lines the reference logs on exit (:153-155) and generateForegroundMask's amount
        // (BackgroundSubtractionUtil.h:56-57), the float printed with the digits that identify it
        const float fgPct = 100.0f * (int)counts[k] / (outW * outH);
        const std::string thr = fmt("--threshold=%.3e", thresholds[t]);
        LOG_INFO(name + fmt(": --blur_radius=%d ", blur) + thr + fmt(" --morph_closing_size=%d, foreground amount: %.2f%%", closing, fgPct));
        entries.push_back(fmt("\"file\": \"%s\", \"blur_radius\": \"--blur_radius=%d\", \"threshold_slider\": %d, \"threshold\": \"%s\", "
                              "\"morph_closing_size\": \"--morph_closing_size=%d\", \"count\": %u, \"percent\": \"%.9g\", "
                              "\"width\": %d, \"height\": %d",
                              name.c_str(), blur, sliders[t], thr.c_str(), closing, counts[k], fgPct, outW, outH));
        ++k;
      }
    }
  }
  preview_write_json(dir / "thresholds.json", entries);
  return EXIT_SUCCESS;
}
