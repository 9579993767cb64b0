// PngToPfm — drop-in for source/conversion/PngToPfm.cpp (:28-40): cv_util::loadImage<float> of --png (8-bit / 16-bit
// samples scaled to [0, 1], colour reduced to grey) written as a one-channel PFM. Host only: no device is opened.
#include "cli_common.h"

using namespace cli;

static const char* kUsage = R"(
 - Converts a PNG single-channel disparity image to a PFM.

 - Example:
   ./PngToPfm \
   --png=/path/to/video/000000.png \
   --pfm=/path/to/video/000000.pfm
 )";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("pfm", "", "path to output disparity pfm (required)");
  F.str("png", "", "path to input disparity png (required)");
  F.parse(argc, argv);

  CHECK_MSG(F.s("png") != "", "png");
  CHECK_MSG(F.s("pfm") != "", "pfm");

  int w = 0, h = 0;
  const std::vector<float> image = load_float(F.s("png"), w, h);
  write_pfm(F.s("pfm"), image.data(), w, h);
  return EXIT_SUCCESS;
}
