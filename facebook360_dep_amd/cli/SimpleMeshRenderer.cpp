// SimpleMeshRenderer — drop-in for source/render/SimpleMeshRenderer.cpp's off-screen exports (the exports_<format>
// stage of scripts/render/pipeline.py): every camera's colour and disparity fused into a cubemap, an equirect, a
// snapshot, a top/bottom or left/right stereo pair or a colour + disparity stack. Same flags, defaults and checks
// (:92-150); the rendering is derp_render_format, a HIP software rasteriser with CanopyScene's pipeline (what
// OpenGL leaves implementation-defined is fixed in DESIGN.md §8). An empty --format asks for the reference's
// on-screen viewer, which this build does not have: it exits 1 with a message.
// Output: <output>/<frame>.<file_type>; png = 16-bit BGR, jpg = 8-bit BGR, exr = float B, G, R (convertImage of the
// BGRA result, alpha dropped, NaN -> 0 for the integer types).
#include "derp_job.h"

using namespace cli;

static const char* kUsage = R"(
  - Reads a set of disparity (and optionally color) images for a rig and renders a fused version.
  It outputs images in a specified format (the reference's real-time on-screen rendering is not part of
  this build).

  - Example:
    ./SimpleMeshRenderer \
    --first=000000 \
    --last=000000 \
    --rig=/path/to/rigs/rig.json \
    --color=/path/to/video/color \
    --disparity=/path/to/output/disparity \
    --output=/path/to/output/meshes \
    --format=cubecolor
)";

static const char* kFormatsCsv =
    "cubecolor, cubedisp, eqrcolor, eqrdisp, lr180, snapcolor, snapdisp, tb3dof, tbstereo (empty = on-screen rendering)";

static void decode_vector(const std::string& flag, double* out) {  // decodeVector
  std::istringstream s(flag);
  s >> out[0] >> out[1] >> out[2];
  CHECK_MSG(!s.fail(), "Unexpected flag " + flag);
}

// cv_util::loadImage<cv::Vec4f>: colour in [0, 1], alpha 1
static std::vector<float> load_bgra(const fs::path& path, int& w, int& h) {
  const std::vector<uint16_t> bgr = load_color_bgr16(path, w, h);
  std::vector<float> out((size_t)w * h * 4);
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    for (int c = 0; c < 3; ++c) {
      out[4 * i + c] = (float)bgr[3 * i + c] / 65535.0f;
    }
    out[4 * i + 3] = 1.0f;
  }
  return out;
}

static void save(const fs::path& path, const std::string& type, const std::vector<float>& img, int w, int h) {
  fs::create_directories(path.parent_path());
  const size_t n = (size_t)w * h;
  if (type == "exr") {
    std::vector<float> bgr(n * 3);
    for (size_t i = 0; i < n; ++i) {
      for (int c = 0; c < 3; ++c) {
        bgr[3 * i + c] = img[4 * i + c];
      }
    }
    write_exr_f32(path, bgr.data(), w, h, 3);
    return;
  }
  const float scale = type == "jpg" ? 255.0f : 65535.0f;
  auto sat = [scale](float v) {  // saturate_cast: round to nearest, clamp, NaN -> 0
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
  CHECK_MSG(type == "png", "unsupported --file_type " + type + " (png, jpg, exr)");
  std::vector<uint16_t> rgb(n * 3);
  for (size_t i = 0; i < n; ++i) {
    for (int c = 0; c < 3; ++c) {
      rgb[3 * i + (2 - c)] = (uint16_t)sat(img[4 * i + c]);  // write_png takes RGB
    }
  }
  write_png(path, rgb.data(), w, h, 3, 16);
}

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("cameras", "", "comma-separated cameras to render (empty for all)");
  F.str("color", "", "path to input color images (required)");
  F.str("disparity", "", "path to disparity images (required)");
  F.str("background", "", "path to optional background image");
  F.str("background_equirect", "", "path to optional background equirect image");
  F.str("file_type", "png", "Supports any image type allowed in OpenCV [png, jpg and exr here]");
  F.str("first", "000000", "first frame to process (lexical)");
  F.str("forward", "-1.0 0.0 0.0", "forward for rendering");
  F.i32("height", -1, "height of the rendering (pixels), default is width / 2");
  F.dbl("horizontal_fov", 90, "horizontal field of view for rendering (degrees)");
  F.boolean("ignore_alpha_blend", false, "ignore alpha blend (useful if rendering single camera)");
  F.str("last", "000000", "last frame to process (lexical) (ignored if on-screen rendering)");
  F.str("output", "", "path to output directory");
  F.str("position", "0.0 0.0 0.0", "position to render from (m)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.str("up", "0.0 0.0 1.0", "up for rendering");
  F.i32("width", 3072, "width of the rendering (pixels)");
  F.str("format", "", kFormatsCsv);
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);

  CHECK_MSG(F.s("rig") != "", "rig");
  const std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(rig.size() > 0, "rig.size() > 0");
  // verifyInputs (SimpleMeshRenderer.cpp:113-150)
  const std::string format = F.s("format");
  CHECK_MSG(format != "", "--format is empty: on-screen rendering is not supported by this build; pass one of " +
                              std::string(kFormatsCsv));
  CHECK_MSG(F.s("disparity") != "", "disparity");
  CHECK_MSG(F.s("first") != "", "first");
  CHECK_MSG(F.s("last") != "", "last");
  verify_image_paths(F.s("disparity"), rig, F.s("first"), F.s("last"));
  if (F.s("color") != "") {
    verify_image_paths(F.s("color"), rig, F.s("first"), F.s("last"));
  }
  const int width = F.i("width");
  CHECK_MSG(width > 0, "FLAGS_width > 0");
  CHECK_MSG(width % 2 == 0, "width must be a multiple of 2");
  const int height = F.i("height") == -1 ? width / 2 : F.i("height");
  CHECK_MSG(height > 0, "FLAGS_height > 0");
  int outW = 0, outH = 0;
  CHECK_MSG(derp_render_format_size(format.c_str(), width, height, &outW, &outH) == 0, "Invalid format: " + format);
  const bool needsColor = format == "eqrcolor" || format == "cubecolor" || format == "tbstereo" || format == "lr180" ||
                          format == "snapcolor";
  CHECK_MSG(!needsColor || F.s("color") != "", format + " needs --color to be set");
  const std::string fileType = F.s("file_type");
  CHECK_MSG(fileType == "png" || fileType == "jpg" || fileType == "exr",
            "unsupported --file_type " + fileType + " (png, jpg, exr)");

  derp_render_params p;
  derp_render_params_default(&p);
  p.width = width;
  p.height = height;
  decode_vector(F.s("position"), p.position);
  decode_vector(F.s("forward"), p.forward);
  decode_vector(F.s("up"), p.up);
  p.horizontal_fov = F.d("horizontal_fov");
  p.alpha_blend = !F.b("ignore_alpha_blend");

  IoPool pool(-1);
  std::vector<float> background, backgroundEquirect;
  int eqW = 0, eqH = 0;
  if (F.s("background") != "") {
    int bw = 0, bh = 0;
    background = load_bgra(F.s("background"), bw, bh);
    CHECK_MSG(bw == outW && bh == outH, fmt("--background is %dx%d, the %s image is %dx%d", bw, bh, format.c_str(), outW, outH));
  }
  if (F.s("background_equirect") != "") {
    backgroundEquirect = load_bgra(F.s("background_equirect"), eqW, eqH);
  }

  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), (int)rig.size(), rig.data(), (int)rig.size()) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  const int first = std::stoi(F.s("first")), last = std::stoi(F.s("last"));
  const bool useColor = F.s("color") != "";
  IoBatch saves;  // each frame's file is encoded and written behind the next frame's rendering
  for (int iFrame = first; iFrame <= last; ++iFrame) {
    const std::string frame = zero_pad(iFrame);
    LOG_INFO("Processing frame " + frame + "...");
    const size_t n = rig.size();
    std::vector<std::vector<float>> disps(n), colors(n);
    std::vector<int> dw(n), dh(n), cw(n), ch(n);
    {
      IoBatch loads;
      for (size_t i = 0; i < n; ++i) {
        loads.add(pool, [&, i] { disps[i] = read_pfm(image_path(F.s("disparity"), rig[i].id, frame, ".pfm"), dw[i], dh[i]); });
        if (useColor) {
          loads.add(pool, [&, i] { colors[i] = load_bgra(image_path(F.s("color"), rig[i].id, frame), cw[i], ch[i]); });
        }
      }
      loads.wait();
    }
    std::vector<const float*> dp(n), cp(n);
    for (size_t i = 0; i < n; ++i) {
      dp[i] = disps[i].data();
      cp[i] = colors[i].data();
    }
    DERP_OK(ctx, derp_render_upload(ctx, useColor ? cp.data() : nullptr, cw.data(), ch.data(), dp.data(), dw.data(), dh.data()));
    auto out = std::make_shared<std::vector<float>>((size_t)outW * outH * 4);
    DERP_OK(ctx, derp_render_format(ctx, format.c_str(), &p, background.empty() ? nullptr : background.data(),
                                    backgroundEquirect.empty() ? nullptr : backgroundEquirect.data(), eqW, eqH, out->data()));
    const fs::path path = fs::path(F.s("output")) / (frame + "." + fileType);
    saves.add(pool, [out, path, fileType, outW, outH] { save(path, fileType, *out, outW, outH); });
    LOG_INFO("File saved in " + path.string());
  }
  saves.wait();
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
