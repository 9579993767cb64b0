// ExportPointCloud — drop-in for source/conversion/ExportPointCloud.cpp: same flags (:42-52) and checks, one ASCII
// file with an optional count line and "x y z 1 R G B" per point. Compute = derp_resize_area (the colour, INTER_AREA
// to the disparity's size) + derp_export_points per camera; the text is formatted on the host in parallel.
#include "point_cloud_io.h"

using namespace cli;

static const char* kUsage = R"(
  - Reads a set of color and disparity images and produces an ascii file with a
  single point per line

  Each line contains "x y z 1 r g b", where
  - x y z is the position (in meters)
  - r g b is the color (0..255)

  The format can be imported as a .txt into meshlab with File -> Import Mesh
  set Separator to "SPACE" and set Point format to "X Y Z Reflectance R G B"

  - Example:
    ./ExportPointCloud \
    --output=/path/to/video/output \
    --color=/path/to/video/color \
    --disparity=/path/to/output/disparity \
    --rig=/path/to/rigs/rig.json \
    --frame=000000
)";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("cameras", "", "comma-separated cameras to render (empty for all)");
  F.boolean("clip", false, "points beyond max_depth are clipped, not clamped");
  F.str("color", "", "path to input color images (required)");
  F.str("disparity", "", "path to disparity files (.pfm) (required)");
  F.str("frame", "000000", "frame to process (lexical)");
  F.boolean("header_count", true, "add point count to the start of the file");
  F.dbl("max_depth", INFINITY, "depth is clamped to this value (m). Use e.g. 20 to visualize");
  F.str("output", "", "output filename (required)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.i32("subsample", 1, "how often we sample (>= 1)");
  F.i32("threads", -1, "number of threads (-1 = auto, 0 = none)");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("rig") != "", "rig");
  const std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(F.i("threads") != 0, "threads");
  CHECK_MSG(F.s("color") != "", "color");
  CHECK_MSG(F.s("disparity") != "", "disparity");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.i("subsample") >= 1, "subsample >= 1");
  CHECK_MSG(!rig.empty(), "rig.size() > 0");
  verify_image_paths(F.s("color"), rig, F.s("frame"), F.s("frame"));
  for (const auto& cam : rig) {  // verifyImagePaths(FLAGS_disparity, ..., ".pfm") (:64): the disparity is a .pfm file
    const fs::path pfm = fs::path(F.s("disparity")) / cam.id / (F.s("frame") + ".pfm");
    CHECK_MSG(fs::is_regular_file(pfm), "Missing file: " + pfm.string());
  }
  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), (int)rig.size(), rig.data(), (int)rig.size()) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  IoPool pool(F.i("threads"));

  std::vector<std::vector<float>> clouds(rig.size());
  size_t lines = 0;
  for (size_t i = 0; i < rig.size(); ++i) {
    LOG_INFO(fmt("Processing camera %s...", rig[i].id));
    int w, h, cw, ch;
    const std::vector<float> disparity = load_float(image_path(F.s("disparity"), rig[i].id, F.s("frame"), ".pfm"), w, h);
    // loadResizedImage<cv::Vec3f>(..., disparity.size()): loadImage<Vec3f> (16-bit BGR / 65535), then INTER_AREA
    const std::vector<uint16_t> c16 = load_color_bgr16(image_path(F.s("color"), rig[i].id, F.s("frame")), cw, ch);
    CHECK_MSG(cw >= w && ch >= h, fmt("the colour image of %s (%dx%d) is smaller than its disparity (%dx%d): enlarging is "
                                      "not supported", rig[i].id, cw, ch, w, h));
    std::vector<float> color(c16.size());
    const float s = 1.0f / 65535.0f;
    for (size_t k = 0; k < c16.size(); ++k) {
      color[k] = c16[k] * s;
    }
    if (cw != w || ch != h) {
      std::vector<float> resized((size_t)w * h * 3);
      DERP_OK(ctx, derp_resize_area(ctx, 3, color.data(), cw, ch, resized.data(), w, h));
      color.swap(resized);
    }
    clouds[i].resize((size_t)w * h * 6);
    size_t count = 0;
    DERP_OK(ctx, derp_export_points(ctx, (int)i, disparity.data(), w, h, color.data(), F.d("max_depth"), F.b("clip"),
                                    F.i("subsample"), clouds[i].data(), (size_t)w * h, &count));
    clouds[i].resize(count * 6);
    lines += count;
  }
  derp_destroy(ctx);

  const fs::path fnOut(F.s("output"));
  if (fnOut.has_parent_path()) {
    fs::create_directories(fnOut.parent_path());
  }
  FILE* file = fopen(fnOut.c_str(), "wb");
  CHECK_MSG(file != nullptr, "Cannot open file for writing: " + fnOut.string());
  if (F.b("header_count")) {
    fprintf(file, "%zu\n", lines);
  }
  LOG_INFO(fmt("Writing %zu points to file...", lines));
  // the text of a camera's points, a bounded round at a time: every pool thread formats one block of kBlockPoints
  // consecutive points into its own buffer (sized for the longest possible lines, reused), then the blocks are
  // written in order
  const size_t kBlockPoints = 4096;
  const int parts = std::max(1, (int)pool.workers.size());
  std::vector<std::vector<char>> text(parts, std::vector<char>(kBlockPoints * kPointLineMax));
  std::vector<size_t> used(parts);
  for (const std::vector<float>& cloud : clouds) {
    const size_t n = cloud.size() / 6;
    for (size_t round0 = 0; round0 < n; round0 += kBlockPoints * parts) {
      parallel_rows(pool, parts, [&](int a, int b) {
        for (int p = a; p < b; ++p) {
          const size_t k0 = std::min(n, round0 + kBlockPoints * p), k1 = std::min(n, k0 + kBlockPoints);
          size_t at = 0;
          for (size_t k = k0; k < k1; ++k) {
            at += format_point_line(&cloud[k * 6], &text[p][at]);
          }
          used[p] = at;
        }
      });
      for (int p = 0; p < parts; ++p) {
        CHECK_MSG(fwrite(text[p].data(), 1, used[p], file) == used[p], "failed to write: " + fnOut.string());
      }
    }
  }
  CHECK_MSG(fclose(file) == 0, "failed to write: " + fnOut.string());
  LOG_INFO(fmt("%zu lines written", lines));
  return EXIT_SUCCESS;
}
