// GeometricConsistency — drop-in for source/render/GeometricConsistency.cpp: same flags (:44-55) and output files
// (<output>/<frame>/<id>_iffy, <id>_<pass>_clean, <id>_<pass>, each a .pfm of depth and a _disparity.png). Compute =
// derp_gc_upload + derp_gc_run per frame; the reference's OpenGL reprojection is replaced by the sampling rule of
// DESIGN §8.6, so no GL context is needed.
#include "geometric_io.h"

using namespace cli;

static const char* kUsage = R"(
- Compute initial depth for every camera
- Repeat pass_count times:
  - Clean away depths that are implausible
  - Recompute depths using clean depths to estimate occlusions

--median and --single are parsed and unused, as in the reference.

- Example:
    GeometricConsistency \
    --color /path/to/color \
    --output /path/to/output \
    --rig /path/to/rigs/rig.json \
    --first 000000 \
    --last 000000
)";

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.dbl("agree_fraction", 0.75, "fraction considered in agreement");
  F.str("color", "", "color directory (required)");
  F.dbl("disparity_step", 0.5, "pixels per disparity step");
  F.dbl("downscale", 4, "reduced resolution output");
  F.str("first", "", "first frame to process (lexical)");
  F.boolean("keep_clean", false, "only recompute implausible depths");
  F.str("last", "", "last frame to process (lexical)");
  F.i32("median", 0, "radius of median filter applied to input [parsed and unused, as in the reference]");
  F.str("output", "", "output subdirectory (required)");
  F.i32("pass_count", 2, "how many times to refine depth");
  F.str("rig", "", "path to rig .json file (required)");
  F.str("single", "", "render a single destination camera [parsed and unused, as in the reference]");
  F.i32("threads", -1, "number of threads reading and writing images (-1 = auto) [extension]");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("rig") != "", "rig");
  CHECK_MSG(F.s("color") != "", "color");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.s("first") != "", "first");
  CHECK_MSG(F.s("last") != "", "last");
  CHECK_MSG(F.i("threads") != 0, "threads");
  CHECK_MSG(F.d("downscale") > 0, "downscale > 0");
  CHECK_MSG(F.i("pass_count") >= 0, "pass_count >= 0");
  const std::vector<derp_camera_desc> rig = load_rig(F.s("rig"));  // (not normalised: the depths are in metres)
  CHECK_MSG(rig.size() >= 2, "rig.size() >= 2");
  const int n = (int)rig.size();
  std::vector<int> smallW(n), smallH(n);
  for (int i = 0; i < n; ++i) {
    gc_small_size(rig[i], F.d("downscale"), smallW[i], smallH[i]);
    CHECK_MSG(smallW[i] >= 3 && smallH[i] >= 3,
              fmt("camera %s is %d x %d at downscale %g: 3 x 3 at least", rig[i].id, smallW[i], smallH[i], F.d("downscale")));
    int slices = 0;  // the rig's radius (asin has no value from 1 m on) and sliceCount >= 1, before any device is opened
    if (derp_gc_slice_count(rig.data(), n, i, smallW[i], smallH[i], F.d("disparity_step"), &slices) != 0) {
      LOG_FATAL(std::string(derp_last_error(nullptr)));
    }
  }
  verify_image_paths(F.s("color"), rig, F.s("first"), F.s("last"));

  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), n, rig.data(), n) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  IoPool pool(F.i("threads"));
  fs::create_directories(F.s("output"));
  const int first = std::stoi(F.s("first")), last = std::stoi(F.s("last"));
  for (int frame = first; frame <= last; ++frame) {
    const std::string frameName = zero_pad(frame);
    LOG_INFO("Processing frame " + frameName);
    const fs::path dir = fs::path(F.s("output")) / frameName;
    fs::create_directories(dir);
    std::vector<std::vector<uint16_t>> images(n);
    std::vector<int> fullW(n), fullH(n);
    parallel_rows(pool, n, [&](int a, int b) {
      for (int i = a; i < b; ++i) {
        images[i] = load_color_bgra16(image_path(F.s("color"), rig[i].id, frameName), fullW[i], fullH[i]);
      }
    });
    std::vector<const uint16_t*> ptrs(n);
    for (int i = 0; i < n; ++i) {
      ptrs[i] = images[i].data();
    }
    DERP_OK(ctx, derp_gc_upload(ctx, ptrs.data(), fullW.data(), fullH.data(), smallW.data(), smallH.data()));
    DERP_OK(ctx, derp_gc_run(ctx, F.d("disparity_step"), F.d("agree_fraction"), F.i("pass_count"), F.b("keep_clean")));
    // every map of the frame, then the files in parallel
    struct Dump {
      std::string name;
      int cam;
      std::vector<float> depth;
    };
    std::vector<Dump> dumps;
    const auto fetch = [&](int kind, int pass, int cam, const std::string& name) {
      Dump d{name, cam, std::vector<float>((size_t)smallW[cam] * smallH[cam])};
      DERP_OK(ctx, derp_gc_result(ctx, kind, pass, cam, d.depth.data()));
      dumps.push_back(std::move(d));
    };
    for (int i = 0; i < n; ++i) {
      fetch(DERP_GC_IFFY, 0, i, fmt("%s_iffy", rig[i].id));
      for (int pass = 0; pass < F.i("pass_count"); ++pass) {
        fetch(DERP_GC_CLEAN, pass, i, fmt("%s_%d_clean", rig[i].id, pass));
        fetch(DERP_GC_DEPTH, pass, i, fmt("%s_%d", rig[i].id, pass));
      }
    }
    parallel_rows(pool, (int)dumps.size(), [&](int a, int b) {
      for (int k = a; k < b; ++k) {
        gc_dump(dir / dumps[k].name, dumps[k].depth.data(), smallW[dumps[k].cam], smallH[dumps[k].cam]);
      }
    });
  }
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
