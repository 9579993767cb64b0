// RawToRgb — drop-in for source/isp/RawToRgb.cpp: same flags (:36-48), defaults and checks. A .raw Bayer file (or
// every *.raw under a directory, recursively) goes through the camera ISP on the GPU (derp_isp_*) and comes out as an
// 8- or 16-bit colour PNG. One derp_isp per config file serves all the files that use it; reads and PNG encodes run on
// the pool's threads while the GPU works on the next file.
#include <memory>

#include "isp_config.h"

using namespace cli;

static const char* kUsage = R"(
   - Converts a RAW image to RGB using a given ISP configuration.

   - Example:
     ./RawToRgb \
     --input_image_path=/path/to/video/color/000000.raw \
     --output_image_path=/path/to/video/color/000000.png \
     --isp_config_path=/path/to/video/isp.json
 )";

struct Job {
  fs::path input, output, config;
  std::vector<unsigned char> raw, bgr;
  IoBatch read;
};

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.boolean("apply_tone_curve", true, "Apply tone curve to image");
  F.u32("demosaic_filter", DERP_ISP_BILINEAR,
        "Demosaic filter type: 0=Bilinear(fast), 1=Frequency, 2=Edge aware, 3=Chroma supressed bilinear");
  F.str("input_image_path", "", "input image path (required)");
  F.str("isp_config_path", "", "ISP config file path. Defaults to <input_image_path>/isp.json");
  F.str("output_dng_path", "", "optional path to output a DNG version of the raw file.");
  F.str("output_image_path", "", "output image path (required)");
  F.i32("pow2_downscale_factor", 1, "Amount to \"bin-down\" the input. Legal values are 1, 2, 4, and 8");
  F.i32("device", 0, "HIP device index [extension]");
  F.i32("threads", -1, "number of I/O threads (-1 = auto, 0 = none) [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("input_image_path") != "", "input_image_path");
  // ---- what is not built, by name, before any file or device is touched
  const unsigned filter = F.u("demosaic_filter");
  if (filter == DERP_ISP_FREQUENCY) {
    LOG_FATAL("frequency demosaic is not built (--demosaic_filter=1 needs a DCT of the whole plane)");
  }
  CHECK_MSG(filter <= DERP_ISP_CHROMA_SUPPRESSED, "expecting Demosaic filter in [0,3]");
  if (!F.s("output_dng_path").empty()) {
    LOG_FATAL("dng output is not built (--output_dng_path)");
  }
  const int resize = F.i("pow2_downscale_factor");
  CHECK_MSG(resize == 1 || resize == 2 || resize == 4 || resize == 8,
            fmt("expecting a resize value of 1, 2, 4, or 8. got %d", resize));

  std::vector<std::unique_ptr<Job>> jobs;
  const fs::path input = F.s("input_image_path");
  if (fs::is_directory(input)) {  // RawToRgb.cpp:59-72
    std::vector<fs::path> files;
    for (fs::recursive_directory_iterator it(input), end; it != end; ++it) {
      if (fs::is_regular_file(it->path()) && it->path().extension() == ".raw") {
        files.push_back(it->path());
      }
    }
    std::sort(files.begin(), files.end());
    for (const fs::path& f : files) {
      jobs.emplace_back(new Job);
      jobs.back()->input = f;
      jobs.back()->output = fs::path(f).replace_extension(".png");
    }
  } else {
    CHECK_MSG(F.s("output_image_path") != "", "output_image_path");
    CHECK_MSG(input.extension() == ".raw", "rawImageFilename.extension() == .raw: " + input.string());  // RawUtil.cpp:102
    jobs.emplace_back(new Job);
    jobs.back()->input = input;
    jobs.back()->output = F.s("output_image_path");
  }
  // ---- configs (RawUtil.cpp:103-107: the file given, or isp.json beside each input) and file sizes
  std::map<std::string, derp_isp_config> configs;
  for (auto& j : jobs) {
    j->config = F.s("isp_config_path").empty() ? j->input.parent_path() / "isp.json" : fs::path(F.s("isp_config_path"));
    auto it = configs.find(j->config.string());
    if (it == configs.end()) {
      it = configs.emplace(j->config.string(), load_isp_config(j->config)).first;
    }
    const derp_isp_config& k = it->second;
    CHECK_MSG(k.bits_per_pixel == 8 || k.bits_per_pixel == 16, "Unsupported precision");
    CHECK_MSG(k.width > 0 && k.height > 0 && k.width % 2 == 0 && k.height % 2 == 0,
              "sensor width and height must be even and non-zero");
    std::error_code ec;
    const uintmax_t have = fs::file_size(j->input, ec);
    CHECK_MSG(!ec, "could not open raw image file: " + j->input.string());
    const uintmax_t need = (uintmax_t)k.width * k.height * (k.bits_per_pixel / 8);
    if (have < need) {  // readRawImage, RawUtil.cpp:37
      LOG_FATAL(fmt("unexpected end of file: %s holds %ju bytes, width x height x bytes is %ju", j->input.c_str(), have, need));
    }
  }
  // ---- devices
  std::map<std::string, derp_isp*> isps;
  for (const auto& kv : configs) {
    derp_isp* isp = nullptr;
    if (derp_isp_create(&isp, F.i("device"), &kv.second, (int)filter, resize, F.b("apply_tone_curve")) != 0) {
      LOG_FATAL(std::string("derp_isp_create failed: ") + derp_last_error(nullptr));
    }
    isps[kv.first] = isp;
  }
  {
    IoPool pool(F.i("threads"));
    IoBatch writes;
    const size_t ahead = 4;  // files read in advance of the GPU
    auto start_read = [&](Job* j) {
      const derp_isp_config& k = configs.at(j->config.string());
      const size_t need = (size_t)k.width * k.height * (k.bits_per_pixel / 8);
      j->read.add(pool, [j, need] {
        j->raw.resize(need);
        std::ifstream f(j->input, std::ios::binary);
        f.read(reinterpret_cast<char*>(j->raw.data()), (std::streamsize)need);
        CHECK_MSG(f.good(), "unexpected end of file: " + j->input.string());
      });
    };
    for (size_t i = 0; i < std::min(ahead, jobs.size()); ++i) {
      start_read(jobs[i].get());
    }
    for (size_t i = 0; i < jobs.size(); ++i) {
      Job* j = jobs[i].get();
      j->read.wait();
      if (i + ahead < jobs.size()) {
        start_read(jobs[i + ahead].get());
      }
      Timer timer;
      derp_isp* isp = isps.at(j->config.string());
      const int bytes = configs.at(j->config.string()).bits_per_pixel / 8;
      int w = 0, h = 0;
      DERP_OK(nullptr, derp_isp_output_size(isp, &w, &h));
      j->bgr.resize((size_t)w * h * 3 * bytes);
      DERP_OK(nullptr, derp_isp_process(isp, j->raw.data(), j->raw.size(), j->bgr.data()));
      LOG_INFO(fmt("Runtime = %.3f s (%s)", timer.s(), j->input.c_str()));
      std::vector<unsigned char>().swap(j->raw);
      writes.add(pool, [j, w, h, bytes] {  // imwriteExceptionOnFail: BGR -> the PNG's RGB
        std::vector<uint16_t> rgb((size_t)w * h * 3);
        for (size_t p = 0; p < (size_t)w * h; ++p) {
          for (int c = 0; c < 3; ++c) {
            rgb[3 * p + (2 - c)] = bytes == 1 ? j->bgr[3 * p + c] : reinterpret_cast<const uint16_t*>(j->bgr.data())[3 * p + c];
          }
        }
        write_png(j->output, rgb.data(), w, h, 3, 8 * bytes);
        std::vector<unsigned char>().swap(j->bgr);
      }, 1);
      writes.raise_if_failed();
    }
    writes.wait();
  }
  for (auto& kv : isps) {
    derp_isp_destroy(kv.second);
  }
  return EXIT_SUCCESS;
}
