// GenerateCameraOverlaps — drop-in for source/render/GenerateCameraOverlaps.cpp: same flags (:41-49) and output files
// (<output>/overlaps/<id>/<depth in cm, five digits>_cm.png, 8-bit BGRA). Compute = derp_sweep_upload once, then
// derp_sweep_overlaps per destination and slab of depths, with the PNGs of one slab encoded while the next is computed.
// The depth label the reference draws into the image (cv::putText) is not drawn: the depth is in the file's name.
#include "sweep_io.h"

using namespace cli;

static const char* kUsage = R"(
   - Generates a series of images of the rig cameras projected into destination cameras over
   a series of fixed depths.

   - The reference draws each depth into its image as a text label (cv::putText); this build does not: the depth is in
   the file name, <output>/overlaps/<camera>/<depth in cm>_cm.png. Two depths with one name: the later one wins.

   - Example:
     ./GenerateCameraOverlaps \
     --frame=000000 \
     --output=/path/to/output \
     --rig=/path/to/rigs/rig.json \
     --color=/path/to/video/color

     A typical extension of this is creating a video over the series of depth generated, i.e.:

     ffmpeg -framerate 10 -pattern_type glob \
     -i '/path/to/output/overlaps/cam0/*.png' -c:v libx264 -pix_fmt yuv420p \
     -vf "scale=trunc(iw/2)*2:trunc(ih/2)*2" /path/to/output/overlaps/cam0.mp4 -y
 )";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("cameras", "", "cameras to render (comma-separated)");
  F.str("color", "", "path to input color images (required)");
  F.str("frame", "000000", "frame to process (lexical)");
  F.u64("max_depth_m", 10, "max depth in cm");
  F.u64("min_depth_m", 1, "min depth in cm");
  F.u64("num_depths", 50, "num depths");
  F.str("output", "", "path to output directory (required)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.dbl("scale", 0.5, "image scale factor");
  F.i32("threads", -1, "number of threads reading and writing images (-1 = auto) [extension]");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("color") != "", "color");
  CHECK_MSG(F.s("rig") != "", "rig");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.i("threads") != 0, "threads");
  CHECK_MSG(F.d("scale") > 0 && F.d("scale") <= 1, "scale in (0, 1]: INTER_AREA upscaling is not restated");
  CHECK_MSG(F.ull("num_depths") >= 1 && F.ull("num_depths") <= 1000000, "num_depths >= 1");
  CHECK_MSG(F.ull("min_depth_m") > 0 && F.ull("max_depth_m") > 0, "depth > 0");
  const std::vector<derp_camera_desc> rig = load_rig(F.s("rig"));
  CHECK_MSG(!rig.empty(), "rig.size() > 0");
  const std::vector<derp_camera_desc> dsts = filter_destinations(rig, F.s("cameras"));
  CHECK_MSG(dsts.size() > 0, "no destinations!");
  verify_image_paths(F.s("color"), rig, F.s("frame"), F.s("frame"));
  const int n = (int)rig.size(), num = (int)F.ull("num_depths");
  std::vector<float> disparities(num);
  std::vector<int> stems(num);
  if (derp_sweep_overlap_disparities(num, F.ull("min_depth_m"), F.ull("max_depth_m"), disparities.data(), stems.data()) != 0) {
    LOG_FATAL(std::string(derp_last_error(nullptr)));
  }

  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), n, rig.data(), n) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  IoPool pool(F.i("threads"));
  LOG_INFO("Loading images...");
  std::vector<int> w, h;
  sweep_load_and_upload(ctx, pool, F.s("color"), rig, F.s("frame"), F.d("scale"), w, h);
  const fs::path dir = fs::path(F.s("output")) / "overlaps";
  for (const derp_camera_desc& dst : dsts) {
    int index = 0;
    while (std::string(rig[index].id) != dst.id) {
      ++index;
    }
    LOG_INFO(std::string("Camera ") + dst.id + "...");
    fs::create_directories(dir / dst.id);
    sweep_run_slabs(
        pool, num, w[index], h[index],
        [&](int first, int count, uint8_t* out) {
          DERP_OK(ctx, derp_sweep_overlaps(ctx, index, disparities.data() + first, count, DERP_SWEEP_U8, out));
        },
        [&](int k) { return dir / dst.id / fmt("%05d_cm.png", stems[k]); });
  }
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
