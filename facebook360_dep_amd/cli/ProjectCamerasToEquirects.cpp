// ProjectCamerasToEquirects — drop-in for source/conversion/ProjectCamerasToEquirects.cpp: same flags (:35-43) and
// output files (<output>/<id>/<frame>.<file_type>: 16-bit BGRA, or 8-bit BGR for jpg). The inverse of
// ProjectEquirectsToCameras. Compute = derp_render_upload of the frame's colours with constant-disparity maps (1.0f /
// depth) once per frame, then derp_render EQUIRECT once per camera with only that camera included — CanopyScene::equirect
// of a one-camera scene (:93-105), without OpenGL. Pixels the camera does not cover leave the renderer as NaN (the
// un-premultiplied clear colour) and convertImage's saturate_cast stores them as 0 in every channel, alpha included.
#include "sweep_io.h"

using namespace cli;

static const char* kUsage = R"(
   - Projects each camera of a rig into its own equirect at a fixed depth.

   - Example:
     ./ProjectCamerasToEquirects \
     --color=/path/to/video/color \
     --rig=/path/to/rigs/rig.json \
     --first=000000 \
     --last=000000 \
     --output=/path/to/output
)";

// save (:60-69): convertImage<cv::Vec3b> for jpg, convertImage<cv::Vec4w> otherwise: scale, round to nearest, saturate;
// NaN -> 0
static void save(const fs::path& path, const std::string& type, const std::vector<float>& img, int w, int h) {
  fs::create_directories(path.parent_path());
  const size_t n = (size_t)w * h;
  const float scale = type == "jpg" ? 255.0f : 65535.0f;
  auto sat = [scale](float v) {
    const float s = v * scale;
    return !(s == s) ? 0 : s <= 0 ? 0 : s >= scale ? (int)scale : (int)lrintf(s);
  };
  if (type == "jpg") {
    std::vector<uint8_t> rgb(n * 3);
    for (size_t i = 0; i < n; ++i) {
      for (int c = 0; c < 3; ++c) {
        rgb[3 * i + (2 - c)] = (uint8_t)sat(img[4 * i + c]);
      }
    }
    const std::vector<unsigned char> j = codecs::encode_jpeg(rgb.data(), w, h, 3);
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(j.data()), (std::streamsize)j.size());
    CHECK_MSG(f.good(), "failed to save image: " + path.string());
    return;
  }
  std::vector<uint16_t> rgba(n * 4);
  for (size_t i = 0; i < n; ++i) {
    rgba[4 * i] = (uint16_t)sat(img[4 * i + 2]);  // write_png takes R, G, B, A
    rgba[4 * i + 1] = (uint16_t)sat(img[4 * i + 1]);
    rgba[4 * i + 2] = (uint16_t)sat(img[4 * i]);
    rgba[4 * i + 3] = (uint16_t)sat(img[4 * i + 3]);
  }
  write_png(path, rgba.data(), w, h, 4, 16);
}

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("cameras", "", "comma-separated cameras to render (empty for all)");
  F.str("color", "", "path to input color images (required)");
  F.dbl("depth", 1000, "depth to project at (m)");
  F.i32("eqr_width", 1024, "equirect width (pixels)");
  F.str("file_type", "png", "Supports any image type allowed in OpenCV");
  F.str("first", "000000", "first frame to process (lexical)");
  F.str("last", "000000", "last frame to process (lexical)");
  F.str("output", "", "output directory (required)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.i32("threads", -1, "number of threads reading and writing images (-1 = auto) [extension]");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("rig") != "", "rig");
  const std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(F.s("color") != "", "color");
  CHECK_MSG(F.s("first") != "", "first");
  CHECK_MSG(F.s("last") != "", "last");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.i("threads") != 0, "threads");
  CHECK_MSG(F.d("depth") > 0, "depth > 0");
  CHECK_MSG(F.i("eqr_width") >= 2, "eqr_width >= 2");
  CHECK_MSG(F.i("eqr_width") % 2 == 0, "equirect width must be a multiple of 2");
  CHECK_MSG(F.s("file_type") == "png" || F.s("file_type") == "jpg", "unsupported --file_type " + F.s("file_type") + " (png, jpg)");
  CHECK_MSG(rig.size() > 0, "rig.size() > 0");
  verify_image_paths(F.s("color"), rig, F.s("first"), F.s("last"));
  const int n = (int)rig.size();

  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), n, rig.data(), n) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  IoPool pool(F.i("threads"));
  // constant disparity at each camera's resolution (:79-82): `1.0f / FLAGS_depth` is a double quotient stored as float
  std::vector<std::vector<float>> disparities(n);
  std::vector<int> dw(n), dh(n);
  for (int i = 0; i < n; ++i) {
    dw[i] = (int)rig[i].resolution[0];
    dh[i] = (int)rig[i].resolution[1];
    disparities[i].assign((size_t)dw[i] * dh[i], (float)(1.0 / F.d("depth")));
  }
  derp_render_params p;
  derp_render_params_default(&p);
  p.kind = DERP_RENDER_EQUIRECT;
  p.height = (int)((float)F.i("eqr_width") / 2.0f);
  p.width = 2 * p.height;
  p.position[0] = p.position[1] = p.position[2] = 0;
  p.ipd = 0;
  p.alpha_blend = 0;
  const int first = std::stoi(F.s("first")), last = std::stoi(F.s("last"));
  IoBatch writes;
  for (int frame = first; frame <= last; ++frame) {
    const std::string frameName = zero_pad(frame);
    LOG_INFO("Frame " + frameName + ": Loading colors...");
    std::vector<SweepImage> colors(n);
    parallel_rows(pool, n, [&](int a, int b) {
      for (int i = a; i < b; ++i) {
        colors[i] = sweep_load_bgra_f32(image_path(F.s("color"), rig[i].id, frameName));
      }
    });
    std::vector<const float*> cp(n), dp(n);
    std::vector<int> cw(n), ch(n);
    for (int i = 0; i < n; ++i) {
      cp[i] = colors[i].bgra.data();
      dp[i] = disparities[i].data();
      cw[i] = colors[i].w;
      ch[i] = colors[i].h;
    }
    DERP_OK(ctx, derp_render_upload(ctx, cp.data(), cw.data(), ch.data(), dp.data(), dw.data(), dh.data()));
    for (int i = 0; i < n; ++i) {
      LOG_INFO("-- Frame " + frameName + ": Projecting " + rig[i].id + "...");
      std::vector<uint8_t> include(n, 0);
      include[i] = 1;
      auto eqr = std::make_shared<std::vector<float>>((size_t)p.width * p.height * 4);
      DERP_OK(ctx, derp_render(ctx, &p, include.data(), eqr->data()));
      const fs::path file = fs::path(F.s("output")) / rig[i].id / (frameName + "." + F.s("file_type"));
      const std::string type = F.s("file_type");
      const int w = p.width, h = p.height;
      writes.add(pool, [=] { save(file, type, *eqr, w, h); });
      writes.raise_if_failed();
    }
  }
  writes.wait();
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
