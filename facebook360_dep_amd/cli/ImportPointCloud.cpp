// ImportPointCloud — drop-in for source/conversion/ImportPointCloud.cpp: same flags (:46-53) and checks, writes
// <output>/<cam>/000000.png (16-bit, one channel). The file is parsed in chunks on the pool's threads while the chunk
// before is projected on the GPU (derp_points_splat accumulates into the same images).
#include "point_cloud_io.h"

using namespace cli;

static const char* kUsage = R"(
  - Reads a point cloud as an ASCII file with a single point per line and generates a disparity
  image per camera.

  Supports multiple point cloud formats, but only extracts the xyz coordinates.

  The input file can have a single line header with a point count.

  - Example:
    ./ImportPointCloud \
    --output=/path/to/output \
    --rig=/path/to/rigs/rig.json \
    --point_cloud=/path/to/points.xyz

    Where points.xyz may be of the form:

    10000
    -0.04503071680665016 -2.2521071434020996 4.965743541717529 1 90 104 136
    -0.005194493103772402 -2.323836088180542 4.938142776489258 1 94 110 143
    0.046292994171381 -2.2623345851898193 4.609960079193115 1 101 122 149
    ...
)";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("cameras", "", "comma-separated cameras to render (empty for all)");
  F.dbl("max_depth", INFINITY, "ignore depths farther than this value (m)");
  F.dbl("min_depth", 0, "ignore depths closer than this value (m)");
  F.str("output", "", "output directory (required)");
  F.str("point_cloud", "", "input point cloud (required)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.i32("threads", -1, "number of threads (-1 = auto, 0 = none)");
  F.i32("width", 1024, "width of output camera images (0 = size from rig file)");
  F.i32("device", 0, "HIP device index [extension]");
  F.i32("chunk_points", 1 << 20, "points parsed and projected at a time [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("rig") != "", "rig");
  const std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(F.s("point_cloud") != "", "point_cloud");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.i("width") >= 0, "width >= 0");
  CHECK_MSG(F.i("width") % 2 == 0, "width must be a multiple of 2");
  CHECK_MSG(!rig.empty(), "rig.size() > 0");
  CHECK_MSG(F.i("chunk_points") > 0, "chunk_points > 0");
  std::vector<int> widths(rig.size()), heights(rig.size());
  for (size_t i = 0; i < rig.size(); ++i) {  // rescaleCameras (:63-74)
    widths[i] = (int)rig[i].resolution[0];
    heights[i] = (int)rig[i].resolution[1];
    if (F.i("width") > 0) {
      int height = (int)std::round(F.i("width") * rig[i].resolution[1] / float(rig[i].resolution[0]));
      height += height % 2;  // force even number of rows
      widths[i] = F.i("width");
      heights[i] = height;
    }
    LOG_INFO(fmt("%s output resolution: %dx%d", rig[i].id, widths[i], heights[i]));
  }
  PointFileReader reader;
  reader.open(F.s("point_cloud"));
  LOG_INFO(fmt("Extracting %lld points from %s...", reader.count, F.s("point_cloud").c_str()));
  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), (int)rig.size(), rig.data(), (int)rig.size()) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  DERP_OK(ctx, derp_points_begin(ctx, widths.data(), heights.data()));
  IoPool pool(F.i("threads"));
  std::vector<double> xyz;
  while (const size_t n = reader.next(pool, (size_t)F.i("chunk_points"), xyz)) {
    DERP_OK(ctx, derp_points_splat(ctx, xyz.data(), n, F.d("min_depth"), F.d("max_depth")));
  }
  LOG_INFO(fmt("Extracted %lld points.", reader.done));
  LOG_INFO("Saving images...");
  for (size_t i = 0; i < rig.size(); ++i) {
    std::vector<float> disparity((size_t)widths[i] * heights[i]);
    DERP_OK(ctx, derp_points_download(ctx, (int)i, disparity.data()));
    const fs::path fn = fs::path(F.s("output")) / rig[i].id / "000000.png";
    fs::create_directories(fn.parent_path());
    write_disparity_png(fn, disparity.data(), widths[i], heights[i]);  // cv_util::convertTo<uint16_t>
  }
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
