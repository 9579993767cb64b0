// ProjectEquirectsToCameras — drop-in for source/conversion/ProjectEquirectsToCameras.cpp: same flags (:33-42) and
// checks; reads <eqr_masks>/<cam>/<frame>.<ext> (threshold > 127), writes <output>/<cam>/<frame>.<file_type>
// (8-bit, 0 / 255). Compute = derp_project_equirect_mask.
#include "cli_common.h"

using namespace cli;

static const char* kUsage = R"(
  - Reads equirect masks and projects them to individual cameras assuming a given depth.

  - Example:
    ./ProjectEquirectsToCameras \
    --eqr_masks=/path/to/video/equirect_masks/ \
    --rig=/path/to/rigs/rig.json \
    --first=000000 \
    --last=000000 \
    --output=/path/to/output/
)";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("cameras", "", "comma-separated cameras to render (empty for all)");
  F.dbl("depth", 1000, "depth to project at (m)");
  F.str("eqr_masks", "", "path to input equirect masks (required)");
  F.str("file_type", "png", "Supports any image type allowed in OpenCV [png and jpg here]");
  F.str("first", "000000", "first frame to process (lexical) (required)");
  F.str("last", "000000", "last frame to process (lexical) (required)");
  F.str("output", "", "output directory (required)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.i32("threads", -1, "number of threads (-1 = auto, 0 = none) [accepted; the GPU path ignores it]");
  F.i32("width", 0, "width of projected camera images (0 = size from rig file)");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("rig") != "", "rig");
  const std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(F.s("eqr_masks") != "", "eqr_masks");
  CHECK_MSG(F.s("first") != "", "first");
  CHECK_MSG(F.s("last") != "", "last");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.d("depth") > 0, "depth > 0");
  CHECK_MSG(F.i("width") >= 0, "width >= 0");
  CHECK_MSG(F.i("width") % 2 == 0, "equirect width must be a multiple of 2");
  CHECK_MSG(!rig.empty(), "rig.size() > 0");
  const std::string fileType = F.s("file_type");
  CHECK_MSG(fileType == "png" || fileType == "jpg", "unsupported --file_type " + fileType + " (png, jpg)");
  verify_image_paths(F.s("eqr_masks"), rig, F.s("first"), F.s("last"));
  std::vector<int> widths(rig.size()), heights(rig.size());
  for (size_t i = 0; i < rig.size(); ++i) {  // rescaleCameras (:59-70): ceil here, round in ImportPointCloud
    widths[i] = (int)rig[i].resolution[0];
    heights[i] = (int)rig[i].resolution[1];
    if (F.i("width") > 0) {
      int height = (int)ceil(F.i("width") * rig[i].resolution[1] / float(rig[i].resolution[0]));
      height += height % 2;  // force even number of rows
      widths[i] = F.i("width");
      heights[i] = height;
    }
    LOG_INFO(fmt("%s output resolution: %dx%d", rig[i].id, widths[i], heights[i]));
  }
  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), (int)rig.size(), rig.data(), (int)rig.size()) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  for (int f = std::stoi(F.s("first")); f <= std::stoi(F.s("last")); ++f) {
    const std::string frame = zero_pad(f);
    LOG_INFO(fmt("Frame %s: Loading equirect masks...", frame.c_str()));
    for (size_t i = 0; i < rig.size(); ++i) {
      int ew, eh;
      const std::vector<uint8_t> eqr = load_mask(image_path(F.s("eqr_masks"), rig[i].id, frame), ew, eh);
      LOG_INFO(fmt("-- Frame %s: Projecting to %s...", frame.c_str(), rig[i].id));
      const int w = widths[i], h = heights[i];
      std::vector<uint8_t> mask((size_t)w * h);
      DERP_OK(ctx, derp_project_equirect_mask(ctx, (int)i, eqr.data(), ew, eh, w, h, F.d("depth"), mask.data()));
      const fs::path fn = fs::path(F.s("output")) / rig[i].id / (frame + "." + fileType);
      fs::create_directories(fn.parent_path());
      if (fileType == "png") {  // imwrite(255.0f * camMask)
        std::vector<uint16_t> px(mask.size());
        for (size_t k = 0; k < mask.size(); ++k) {
          px[k] = mask[k] ? 255 : 0;
        }
        write_png(fn, px.data(), w, h, 1, 8);
      } else {
        for (auto& v : mask) {
          v = v ? 255 : 0;
        }
        const std::vector<unsigned char> j = codecs::encode_jpeg(mask.data(), w, h, 1);
        std::ofstream out(fn, std::ios::binary);
        out.write(reinterpret_cast<const char*>(j.data()), (std::streamsize)j.size());
        CHECK_MSG(out.good(), "failed to save image: " + fn.string());
      }
    }
  }
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
