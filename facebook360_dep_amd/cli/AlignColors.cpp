// AlignColors — drop-in for source/calibration/AlignColors.cpp: same flags (:35-43) and output files
// (<output>/<camera id>/<frame>.png, 16-bit, 3-channel). Compute = derp_align_setup once (the warp maps of every
// camera), then derp_align_frame per frame, with frame f + 1 decoded and frame f - 1 encoded while frame f is on the
// device. Every bad input is refused before a device is opened. Definitions: DESIGN §8.8.
#include "cli_common.h"

using namespace cli;

static const char* kUsage = R"(
   - Aligns colors using separate (calibrated) color rigs.

   - Example:
     ./AlignColors \
     --output=/path/to/output \
     --color=/path/to/video/color \
     --calibrated_rig=/path/to/rigs/rig_calibrated.json \
     --rig_blue=/path/to/rigs/rig_blue.json \
     --rig_green=/path/to/rigs/rig_green.json \
     --rig_red=/path/to/rigs/rig_red.json
 )";

namespace {

// one frame of every camera in flight: decoded into `in`, aligned into `out`, encoded from `out`
struct Slot {
  std::vector<std::vector<uint16_t>> in, out;
  IoBatch decode, encode;
};

// seconds spent inside the jobs of one kind, summed over the workers
struct JobClock {
  std::mutex mu;
  double seconds = 0;
  void add(double s) {
    std::lock_guard<std::mutex> lk(mu);
    seconds += s;
  }
};

}  // namespace

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("calibrated_rig", "", "path to calibrated green rig .json filename (required)");
  F.str("cameras", "", "cameras to align (comma-separated)");
  F.str("color", "", "path to input color images (required)");
  F.str("first", "", "first frame to process (lexical)");
  F.str("last", "", "last frame to process (lexical)");
  F.str("output", "", "path to output directory (must be different than color path)");
  F.str("rig_blue", "", "path to camera blue rig .json filename (required)");
  F.str("rig_green", "", "path to camera green rig .json filename (required)");
  F.str("rig_red", "", "path to camera red rig .json filename (required)");
  F.i32("threads", -1, "number of threads reading and writing images (-1 = auto) [extension]");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("color") != "", "color");
  CHECK_MSG(F.s("calibrated_rig") != "", "calibrated_rig");
  CHECK_MSG(F.s("rig_red") != "", "rig_red");
  CHECK_MSG(F.s("rig_green") != "", "rig_green");
  CHECK_MSG(F.s("rig_blue") != "", "rig_blue");
  CHECK_MSG(F.s("output") != "", "output");
  CHECK_MSG(F.s("color") != F.s("output"), "color vs output: the output directory must differ from the color path");
  CHECK_MSG(F.i("threads") != 0, "threads");

  const std::vector<derp_camera_desc> all = load_rig(F.s("calibrated_rig"));
  CHECK_MSG(!all.empty(), "rig.size() > 0");
  // (the reference's filterDestinations passes over a name the rig does not hold; here it is refused)
  {
    std::stringstream names(F.s("cameras"));
    std::string name;
    while (std::getline(names, name, ',')) {
      const bool known = std::any_of(all.begin(), all.end(), [&](const derp_camera_desc& c) { return name == c.id; });
      CHECK_MSG(known, "unknown camera in --cameras: " + name);
    }
  }
  const std::vector<derp_camera_desc> rig = filter_destinations(all, F.s("cameras"));
  CHECK_MSG(!rig.empty(), "no cameras to align");
  const std::vector<derp_camera_desc> red = load_rig(F.s("rig_red")), green = load_rig(F.s("rig_green")),
                                      blue = load_rig(F.s("rig_blue"));
  CHECK_MSG(green.size() == 1, fmt("the green reference rig must hold exactly one camera (it holds %zu)", green.size()));
  CHECK_MSG(red.size() == 1, fmt("the red reference rig must hold exactly one camera (it holds %zu)", red.size()));
  CHECK_MSG(blue.size() == 1, fmt("the blue reference rig must hold exactly one camera (it holds %zu)", blue.size()));
  const int n = (int)rig.size();
  std::vector<int> w(n), h(n);
  for (int i = 0; i < n; ++i) {
    derp_camera_desc r, b;
    if (derp_align_derive_cameras(&rig[i], &red[0], &green[0], &blue[0], &r, &b) != 0) {
      LOG_FATAL(std::string(derp_last_error(nullptr)));
    }
    w[i] = (int)rig[i].resolution[0];
    h[i] = (int)rig[i].resolution[1];
    CHECK_MSG(w[i] >= 1 && h[i] >= 1, std::string("bad resolution of camera ") + rig[i].id);
  }

  // getFrameRange (ImageUtil.cpp:41-59): an empty --first / --last is the first / last file of the first camera
  std::string first = F.s("first"), last = F.s("last");
  if (first.empty() || last.empty()) {
    const std::vector<fs::path> files = visible_files_sorted(fs::path(F.s("color")) / rig[0].id);
    CHECK_MSG(!files.empty(), "Missing file: no images in " + (fs::path(F.s("color")) / rig[0].id).string());
    first = first.empty() ? files.front().stem().string() : first;
    last = last.empty() ? files.back().stem().string() : last;
  }
  verify_image_paths(F.s("color"), rig, first, last);
  const int firstFrame = std::stoi(first), lastFrame = std::stoi(last);
  std::vector<std::string> ext(n);  // imagePath's extension (ImageUtil.h:48-56), one directory listing per camera
  for (int i = 0; i < n; ++i) {
    ext[i] = first_extension(fs::path(F.s("color")) / rig[i].id);
  }
  for (int i = 0; i < n; ++i) {
    for (int f = firstFrame; f <= lastFrame; ++f) {
      const fs::path path = image_path(F.s("color"), rig[i].id, zero_pad(f), ext[i]);
      int iw = 0, ih = 0;
      CHECK_MSG(raster_size(path, iw, ih), "failed to load image: " + path.string());
      CHECK_MSG(iw == w[i] && ih == h[i],
                fmt("image size mismatch: %s is %d x %d, the camera's resolution %d x %d", path.c_str(), iw, ih, w[i], h[i]));
    }
  }

  Timer wall;
  derp_ctx* ctx = nullptr;
  if (derp_create(&ctx, F.i("device"), rig.data(), n, rig.data(), n) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  DERP_OK(ctx, derp_align_setup(ctx, red.data(), 1, green.data(), 1, blue.data(), 1));
  const double setupS = wall.s();
  for (int i = 0; i < n; ++i) {
    fs::create_directories(fs::path(F.s("output")) / rig[i].id);
  }

  JobClock decodeClock, encodeClock;
  double deviceS = 0;
  {
    IoPool pool(F.i("threads"));
    Slot slots[3];
    for (Slot& s : slots) {
      s.in.resize(n);
      s.out.resize(n);
      for (int i = 0; i < n; ++i) {
        s.in[i].resize((size_t)w[i] * h[i] * 3);
        s.out[i].resize((size_t)w[i] * h[i] * 3);
      }
    }
    const auto start_decode = [&](int f) {
      Slot& s = slots[f % 3];
      s.encode.wait();  // the frame three before this one has left the slot
      for (int i = 0; i < n; ++i) {
        const fs::path path = image_path(F.s("color"), rig[i].id, zero_pad(f), ext[i]);
        uint16_t* dst = s.in[i].data();
        const int iw = w[i], ih = h[i];
        s.decode.add(pool, [path, dst, iw, ih, &decodeClock] {
          Timer t;
          load_color_bgr16_into(path, dst, iw, ih);  // 8-bit -> 16 bits x 257, alpha dropped (CvUtil.h:196-284)
          decodeClock.add(t.s());
        });
      }
    };
    start_decode(firstFrame);
    for (int f = firstFrame; f <= lastFrame; ++f) {
      if (f + 1 <= lastFrame) {
        start_decode(f + 1);
      }
      Slot& s = slots[f % 3];
      s.decode.wait();
      LOG_INFO("Aligning frame " + zero_pad(f));
      std::vector<const uint16_t*> in(n);
      std::vector<uint16_t*> out(n);
      for (int i = 0; i < n; ++i) {
        in[i] = s.in[i].data();
        out[i] = s.out[i].data();
      }
      Timer t;
      DERP_OK(ctx, derp_align_frame(ctx, in.data(), w.data(), h.data(), out.data()));
      deviceS += t.s();
      for (int i = 0; i < n; ++i) {
        const fs::path path = fs::path(F.s("output")) / rig[i].id / (zero_pad(f) + ".png");
        uint16_t* px = s.out[i].data();
        const size_t count = (size_t)w[i] * h[i];
        const int iw = w[i], ih = h[i];
        s.encode.add(pool, [path, px, count, iw, ih, &encodeClock] {
          Timer te;
          for (size_t k = 0; k < count; ++k) {
            std::swap(px[3 * k], px[3 * k + 2]);  // write_png takes R, G, B
          }
          write_png(path, px, iw, ih, 3, 16);
          encodeClock.add(te.s());
        }, 1);
      }
    }
    for (Slot& s : slots) {
      s.encode.wait();
    }
  }
  LOG_INFO(fmt("%d frames x %d cameras: wall %.3f s (set-up with the maps %.3f s); decode %.3f s and encode %.3f s summed over "
               "the workers, device calls with their copies %.3f s",
               lastFrame - firstFrame + 1, n, wall.s(), setupS, decodeClock.seconds, encodeClock.seconds, deviceS));
  derp_destroy(ctx);
  return EXIT_SUCCESS;
}
