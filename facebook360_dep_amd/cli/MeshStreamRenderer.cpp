// MeshStreamRenderer — the headless counterpart of source/viewer/GlViewer.cpp: renders views from the fused mesh stream
// that ConvertToBinary writes (fused.json + fused_<i>.bin, or the unfused <bin> tree) as the viewer's RigScene renders it
// (source/render/RigScene.cpp, mesh path), to files, for the views SimpleMeshRenderer takes. The rig is the stream's own
// <rig>_fused.json (cameras at the colour's size). Rendering: derp_stream_* (include/derp_hip.h); reading: mesh_stream_io.h.
// Frame n + 1 is read on the I/O pool while frame n renders; the output files are encoded and written behind the
// rendering. Not built: bc7 colour, the interactive window, GlViewer's --readahead (one frame is read ahead).
// Output: <output>/<frame>.<file_type>; png = 8-bit RGBA, the colour sRGB-encoded (the framebuffer's GL_FRAMEBUFFER_SRGB),
// alpha 255 where something was rendered; exr = the linear floats B, G, R (NaN where nothing was rendered).
#include "mesh_stream_io.h"

using namespace cli;

static const char* kUsage = R"(
   - Renders views from the fused binary mesh stream, headless.

   - Example:
     ./MeshStreamRenderer \
     --first=000000 \
     --last=000000 \
     --rig=/path/to/output/fused/rig_fused.json \
     --catalog=/path/to/output/fused/fused.json \
     --strip_files=/path/to/output/fused/fused_0.bin \
     --output=/path/to/output/stream_views \
     --format=cubecolor
)";

static void decode_vector(const std::string& flag, double* out) {  // decodeVector
  std::istringstream s(flag);
  s >> out[0] >> out[1] >> out[2];
  CHECK_MSG(!s.fail(), "Unexpected flag " + flag);
}

// RigScene::render's fade (RigScene.cpp:1089-1096) for a viewer `displacement` metres from the rig's centre
static float fade_of(float displacement) {
  const float kBeginFade = 0.5f, kEndFade = 0.75f, kMinimumFade = 0.05f;
  const float fade =
      kMinimumFade + (1.0f - kMinimumFade) * std::max(0.0f, std::min(1.0f, (displacement - kEndFade) / (kBeginFade - kEndFade)));
  return fade * fade;
}

static std::vector<uint8_t> read_whole(const fs::path& path) {
  const std::string s = read_file_or_empty(path);
  return std::vector<uint8_t>(s.begin(), s.end());
}

static void save(const fs::path& path, const std::string& type, const std::vector<float>& img, int w, int h,
                 const SrgbEncoder& encode) {
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
  std::vector<uint16_t> rgba(n * 4);
  for (size_t i = 0; i < n; ++i) {
    for (int c = 0; c < 3; ++c) {
      rgba[4 * i + (2 - c)] = encode(img[4 * i + c]);  // write_png takes RGBA
    }
    rgba[4 * i + 3] = img[4 * i + 3] == img[4 * i + 3] && img[4 * i + 3] > 0.0f ? 255 : 0;
  }
  write_png(path, rgba.data(), w, h, 4, 8);
}

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("rig", "", "path to rig .json file (required)");
  F.str("catalog", "", "json file describing strip files");
  F.str("strip_files", "", "comma-separated list of strip files");
  F.str("bin", "", "ConvertToBinary's --bin directory, for a stream that was not fused (instead of --catalog) [extension]");
  F.str("cameras", "", "comma-separated cameras to render (empty for all)");
  F.str("first", "000000", "first frame to process (lexical)");
  F.str("last", "000000", "last frame to process (lexical)");
  F.str("output", "", "path to output directory");
  F.str("format", "", "cubecolor, eqrcolor, snapcolor");
  F.str("file_type", "png", "png (8-bit sRGB RGBA) or exr (linear float)");
  F.i32("width", 3072, "width of the rendering (pixels)");
  F.i32("height", -1, "height of the rendering (pixels), default is width / 2");
  F.str("position", "0.0 0.0 0.0", "position to render from (m)");
  F.str("forward", "-1.0 0.0 0.0", "forward for rendering");
  F.str("up", "0.0 0.0 1.0", "up for rendering");
  F.dbl("horizontal_fov", 90, "horizontal field of view for rendering (degrees)");
  F.boolean("fade", false, "fade the image with the distance of --position from the rig's centre, as the viewer does");
  F.i32("device", 0, "HIP device index [extension]");
  F.i32("threads", -1, "I/O worker threads (-1 = auto, 0 = inline) [extension]");
  F.parse(argc, argv);

  // ---- everything below is refused, by name, before a device is opened
  CHECK_MSG(F.s("rig") != "", "rig");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.s("first") != "", "first");
  CHECK_MSG(F.s("last") != "", "last");
  const bool fused = F.s("catalog") != "";
  CHECK_MSG(fused != (F.s("bin") != ""), "exactly one of --catalog and --bin must be given");
  CHECK_MSG(!fused || F.s("strip_files") != "", "strip_files");
  const std::string format = F.s("format"), fileType = F.s("file_type");
  CHECK_MSG(format == "snapcolor" || format == "cubecolor" || format == "eqrcolor",
            "Invalid format: " + format + " (snapcolor, cubecolor, eqrcolor)");
  CHECK_MSG(fileType == "png" || fileType == "exr", "unsupported --file_type " + fileType + " (png, exr)");
  const int width = F.i("width");
  CHECK_MSG(width > 0, "FLAGS_width > 0");
  CHECK_MSG(width % 2 == 0, "width must be a multiple of 2");
  const int height = F.i("height") == -1 ? width / 2 : F.i("height");
  CHECK_MSG(height > 0, "FLAGS_height > 0");
  const std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(rig.size() > 0, "rig.size() > 0");
  int first = 0, last = 0;
  try {
    first = std::stoi(F.s("first"));
    last = std::stoi(F.s("last"));
  } catch (...) {
    LOG_FATAL("Invalid frame name: " + F.s("first") + " / " + F.s("last"));
  }
  CHECK_MSG(first <= last, "first <= last");

  MeshCatalog catalog;
  std::unique_ptr<StripedReader> reader;
  if (fused) {
    CHECK_MSG(fs::is_regular_file(F.s("catalog")), "Missing file: " + F.s("catalog"));
    std::vector<std::string> disks;
    std::stringstream ss(F.s("strip_files"));
    for (std::string d; std::getline(ss, d, ',');) {
      CHECK_MSG(fs::is_regular_file(d), "Missing file: " + d);
      disks.push_back(d);
    }
    catalog = load_mesh_catalog(F.s("catalog"));
    reader = std::make_unique<StripedReader>(disks);
  }
  const char* kExts[3] = {".vtx", ".idx", ".rgba"};
  for (int iFrame = first; iFrame <= last; ++iFrame) {
    const std::string frame = zero_pad(iFrame);
    for (const derp_camera_desc& cam : rig) {
      const std::string what = frame + "/" + cam.id;
      const int w = (int)cam.resolution[0], h = (int)cam.resolution[1];
      uint64_t size[3];
      if (fused) {
        const MeshStreamCamera& entry = catalog_camera(catalog, frame, cam.id);
        for (int k = 0; k < 3; ++k) {
          const MeshStreamEntry& e = entry.files.at(kExts[k]);
          reader->check(e.offset, e.size, what + kExts[k]);
          size[k] = e.size;
        }
      } else {
        const fs::path dir = fs::path(F.s("bin")) / cam.id;
        if (!fs::is_regular_file(dir / (frame + ".rgba"))) {
          CHECK_MSG(!fs::is_regular_file(dir / (frame + ".bc7")), "frame " + frame + " holds " + cam.id +
                    ".bc7 but no .rgba: bc7 colour is not built; write the stream with --output_formats=idx,vtx,rgba");
        }
        for (int k = 0; k < 3; ++k) {
          const fs::path p = dir / (frame + kExts[k]);
          CHECK_MSG(fs::is_regular_file(p), "Missing file: " + p.string());
          size[k] = (uint64_t)fs::file_size(p);
        }
      }
      check_mesh_sizes(size[0], size[1], size[2], w, h, what);
    }
  }

  derp_render_params p;
  derp_render_params_default(&p);
  p.kind = format == "snapcolor" ? DERP_RENDER_SNAPSHOT : format == "cubecolor" ? DERP_RENDER_CUBE : DERP_RENDER_EQUIRECT;
  p.width = width;
  p.height = height;
  decode_vector(F.s("position"), p.position);
  decode_vector(F.s("forward"), p.forward);
  decode_vector(F.s("up"), p.up);
  p.horizontal_fov = F.d("horizontal_fov");
  int outW = 0, outH = 0;
  CHECK_MSG(derp_render_format_size(format.c_str(), width, height, &outW, &outH) == 0, "Invalid format: " + format);
  const float displacement = (float)std::sqrt(p.position[0] * p.position[0] + p.position[1] * p.position[1] + p.position[2] * p.position[2]);
  const float fade = F.b("fade") ? fade_of(displacement) : 1.0f;
  float srgb[256];
  derp_stream_srgb_table(srgb);
  const SrgbEncoder encode(srgb);

  IoPool pool(F.i("threads"));
  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), (int)rig.size(), rig.data(), (int)rig.size()) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  struct Loaded {
    std::vector<MeshStreamFrameCamera> cams;
    IoBatch batch;
  };
  auto load = [&](int iFrame) {
    auto L = std::make_shared<Loaded>();
    L->cams.resize(rig.size());
    const std::string frame = zero_pad(iFrame);
    for (size_t i = 0; i < rig.size(); ++i) {
      L->batch.add(pool, [&, L, i, frame] {
        MeshStreamFrameCamera& m = L->cams[i];
        std::vector<uint8_t>* into[3] = {&m.vtx, &m.idx, &m.rgba};
        for (int k = 0; k < 3; ++k) {
          if (fused) {
            const MeshStreamEntry& e = catalog.frames.at(frame).at(rig[i].id).files.at(kExts[k]);
            *into[k] = reader->read(e.offset, e.size, frame + "/" + rig[i].id + kExts[k]);
          } else {
            *into[k] = read_whole(fs::path(F.s("bin")) / rig[i].id / (frame + kExts[k]));
          }
        }
      });
    }
    return L;
  };
  // at most kSavesInFlight rendered images wait for their encoder (a 2048-pixel cube is 400 MB of floats, and a PNG
  // takes longer to deflate than a frame to render): the loop waits for the oldest before it renders another
  const size_t kSavesInFlight = 4;
  std::deque<std::unique_ptr<IoBatch>> saves;
  std::shared_ptr<Loaded> next = load(first);
  for (int iFrame = first; iFrame <= last; ++iFrame) {
    const std::string frame = zero_pad(iFrame);
    LOG_INFO("Processing frame " + frame + "...");
    std::shared_ptr<Loaded> cur = next;
    cur->batch.wait();
    if (iFrame < last) {
      next = load(iFrame + 1);
    }
    for (size_t i = 0; i < rig.size(); ++i) {
      const MeshStreamFrameCamera& m = cur->cams[i];
      const int w = (int)rig[i].resolution[0], h = (int)rig[i].resolution[1];
      check_mesh_sizes(m.vtx.size(), m.idx.size(), m.rgba.size(), w, h, frame + "/" + rig[i].id);  // (a file may have changed)
      DERP_OK(ctx, derp_stream_upload(ctx, (int)i, reinterpret_cast<const float*>(m.vtx.data()), m.vtx.size() / 12,
                                      reinterpret_cast<const uint32_t*>(m.idx.data()), m.idx.size() / 4, m.rgba.data(), w, h));
    }
    while (saves.size() >= kSavesInFlight) {
      saves.front()->wait();
      saves.pop_front();
    }
    auto out = std::make_shared<std::vector<float>>((size_t)outW * outH * 4);
    DERP_OK(ctx, derp_stream_render(ctx, &p, nullptr, fade, out->data()));
    const fs::path path = fs::path(F.s("output")) / (frame + "." + fileType);
    saves.push_back(std::make_unique<IoBatch>());
    saves.back()->add(pool, [out, path, fileType, outW, outH, &encode] {
      save(path, fileType, *out, outW, outH, encode);
      LOG_INFO("File saved in " + path.string());
    });
  }
  for (auto& s : saves) {
    s->wait();
  }
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
