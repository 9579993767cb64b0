// ConvertToBinary — drop-in for source/mesh_stream/ConvertToBinary.cpp, the pipeline's convert_to_binary and fusion
// stages (scripts/render/pipeline.py:458-492): same 18 flags (:63-86), checks and <dir>/<camera>/<frame>.<ext> layout.
// Per frame and camera: the colour as raw RGBA bytes (.rgba), the disparity as a simplified triangle mesh (.vtx / .idx,
// optionally .obj); then everything striped into fused_<i>.bin with a catalog (BinaryFusionUtil.h, StripedFile.h).
// Compute = derp_mesh_build + derp_mesh_setup on the GPU per camera; the sequential collapse loop
// (derp_mesh_simplify_host) runs on the I/O pool while the GPU builds the next camera's mesh. Fusion needs no device
// and opens none. --simplifier=parallel [extension] keeps a camera's mesh on the GPU instead: derp_mesh_simplify_parallel,
// a pass-parallel collapse on the device, and the pool only writes the files. Not built: --output_formats bc7 (the ISPC codec) and pfm (writePfm's Eigen QR); both are refused
// by name before anything is opened.
#include <cfloat>
#include <set>

#include "cli_common.h"
#include "rig_writer.h"

using namespace cli;

static const char* kUsage = R"(
       - Expects all files to be in the format <dir>/<camera>/<frame>.extension

       If <color> is specified:
       - Read .png files and save them as .rgba files in <bin> folder
       If <disparity> is specified:
       - Read .pfm files and save them as .vtx and .idx files in <bin> folder

       <bin> folder is created for each frame if it does not exist

       If <rgba> is specified:
       - Convert color image into an RGBA binary stream

       If <obj> is specified:
       - Read .vtx and .idx files from <bin> and save .obj files to <obj> folder

       - Example:
         ./ConvertToBinary \
         --color=/path/to/video/color \
         --rig=/path/to/rigs/rig.json \
         --first=000000 \
         --last=000000 \
         --disparity=/path/to/output/disparity \
         --bin=/path/to/output/bin \
         --fused=/path/to/output/fused
     )";

// the optional "group" of every camera of a rig file (Camera.cpp:72-74), by id
static std::map<std::string, std::string> rig_groups(const std::string& path) {
  const std::string text = read_file_or_empty(path);
  JsonParser jp(text);
  const Json root = jp.value();
  std::map<std::string, std::string> groups;
  for (const Json& c : root.at("cameras").arr) {
    if (const Json* g = c.find("group")) {
      groups[c.at("id").str] = g->str;
    }
  }
  return groups;
}

// Camera::rescale (Camera.cpp:217-223)
static void rescale_camera(derp_camera_desc& c, double newX, double newY) {
  if (!c.has_principal) {  // (Camera.cpp:46-50)
    c.has_principal = 1;
    c.principal[0] = c.resolution[0] / 2;
    c.principal[1] = c.resolution[1] / 2;
  }
  const double qx = newX / c.resolution[0], qy = newY / c.resolution[1];
  c.principal[0] *= qx;
  c.principal[1] *= qy;
  c.focal[0] *= qx;
  c.focal[1] *= qy;
  c.resolution[0] = newX;
  c.resolution[1] = newY;
}

// the size of cv_util::scaleImage's result (CvUtil.h:149-154): std::round
static void scaled_size(int w, int h, double scale, int& sw, int& sh) {
  sw = (int)std::round(w * scale);
  sh = (int)std::round(h * scale);
}

// cv_util::loadImage<cv::Vec4b> (CvUtil.h:196-284): IMREAD_UNCHANGED -> convertTo(CV_8U, 255 / max of the depth) ->
// GRAY2BGRA / BGR2BGRA (alpha 255) -> and, for the .rgba stream, COLOR_BGRA2RGBA: written here as R G B A directly
static std::vector<uint8_t> load_rgba8(const fs::path& path, int& w, int& h) {
  const Raster p = read_raster(path);
  w = p.w;
  h = p.h;
  const size_t n = (size_t)w * h;
  std::vector<uint8_t> out(n * 4);
  auto to8 = [&](size_t at) -> uint8_t {
    if (p.bitdepth == 32) {
      return (uint8_t)float_to_uint_sat(p.f32[at], 255.0f, 255u);
    }
    const unsigned v = p.px[at];
    return (uint8_t)(p.bitdepth == 16 ? (unsigned)lrintf(v * (255.0f / 65535.0f)) : v);
  };
  CHECK_MSG(p.bitdepth == 8 || p.bitdepth == 16 || (p.bitdepth == 32 && p.channels == 1),
            "unsupported bit depth of a colour image: " + path.string());
  CHECK_MSG(p.channels == 1 || p.channels == 3 || p.channels == 4,
            fmt("Conversion from %d channels to 4 channels not supported: %s", p.channels, path.c_str()));
  for (size_t i = 0; i < n; ++i) {
    if (p.channels == 1) {
      out[4 * i] = out[4 * i + 1] = out[4 * i + 2] = to8(i);
      out[4 * i + 3] = 255;
    } else {
      for (int k = 0; k < 3; ++k) {
        out[4 * i + k] = to8((size_t)p.channels * i + k);
      }
      out[4 * i + 3] = p.channels == 4 ? to8(4 * i + 3) : 255;
    }
  }
  return out;
}

// ---------------------------------------------------------------- fusion (BinaryFusionUtil.h:26-84, StripedFile.h)
static const uint64_t kStripeSize = 512 * 1024;
static uint64_t align_stripe(uint64_t offset) {
  return (offset + kStripeSize - 1) & ~(kStripeSize - 1);
}
static size_t stripe_disk(uint64_t global, size_t diskCount) {  // StripedFile::calcStripe's `disk`
  return (size_t)((global / kStripeSize) % diskCount);
}
static void add_file(std::vector<FILE*>& disks, uint64_t& offset, const fs::path& filename) {
  const uint64_t aligned = align_stripe(offset);
  uint64_t end = offset == aligned ? offset + kStripeSize : aligned;
  std::error_code ec;
  uint64_t size = fs::file_size(filename, ec);
  CHECK_MSG(!ec, "Missing file: " + filename.string());
  FILE* file = fopen(filename.c_str(), "rb");
  CHECK_MSG(file != nullptr, "Missing file: " + filename.string());
  LOG_INFO("Fusing " + filename.string() + "...");
  std::vector<uint8_t> buffer;
  while (size) {
    buffer.resize((size_t)std::min(size, end - offset));
    CHECK_MSG(fread(buffer.data(), 1, buffer.size(), file) == buffer.size(), "Error reading buffer data");
    FILE* disk = disks[stripe_disk(offset, disks.size())];
    CHECK_MSG(fwrite(buffer.data(), 1, buffer.size(), disk) == buffer.size(), "failed to write a fused file");
    offset += buffer.size();
    end = offset + kStripeSize;
    size -= buffer.size();
  }
  fclose(file);
}
static void pad(std::vector<FILE*>& disks, uint64_t& offset) {
  const uint64_t aligned = align_stripe(offset);
  if (offset == aligned) {
    return;
  }
  const std::vector<uint8_t> buffer((size_t)(aligned - offset), 0x5A);
  FILE* disk = disks[stripe_disk(offset, disks.size())];
  CHECK_MSG(fwrite(buffer.data(), 1, buffer.size(), disk) == buffer.size(), "failed to write a fused file");
  offset += buffer.size();
}

static void fuse(const Flags& F, const std::vector<derp_camera_desc>& rig, const std::vector<std::string>& formats) {
  const fs::path fused(F.s("fused")), bin(F.s("bin"));
  fs::create_directories(fused);
  CHECK_MSG(F.i("fuse_strip") >= 1, "fuse_strip >= 1");
  std::vector<FILE*> disks;
  for (int i = 0; i < F.i("fuse_strip"); ++i) {
    const fs::path diskName = fused / fmt("fused_%d.bin", i);
    FILE* disk = fopen(diskName.c_str(), "wb");
    CHECK_MSG(disk != nullptr, "Failed to open " + diskName.string());
    disks.push_back(disk);
  }
  uint64_t offset = 0;
  JsonOut catalog = JsonOut::object();
  catalog.obj["metadata"] = JsonOut::object();
  catalog.obj["metadata"].obj["isLittleEndian"] = JsonOut::boolean(true);  // (gfx950 hosts are x86-64)
  catalog.obj["frames"] = JsonOut::object();
  const int first = std::stoi(F.s("first")), numFrames = std::stoi(F.s("last")) - first + 1;
  for (int iFrame = 0; iFrame < numFrames; ++iFrame) {
    const std::string frameName = zero_pad(iFrame + first, 6);
    LOG_INFO("Fusing frame " + frameName + "...");
    JsonOut& frame = catalog.obj["frames"].obj[frameName] = JsonOut::object();
    for (const derp_camera_desc& cam : rig) {
      const uint64_t begin = offset;
      JsonOut& camera = frame.obj[cam.id] = JsonOut::object();
      for (const std::string& format : formats) {
        const uint64_t b = offset;
        add_file(disks, offset, bin / cam.id / (frameName + "." + format));
        JsonOut entry = JsonOut::object();
        entry.obj["offset"] = JsonOut::integer(b);
        entry.obj["size"] = JsonOut::integer(offset - b);
        camera.obj["." + format] = entry;
      }
      camera.obj["offset"] = JsonOut::integer(begin);
      camera.obj["size"] = JsonOut::integer(offset - begin);
      pad(disks, offset);
    }
  }
  std::string text;
  catalog.write(text, 10);
  write_text(fused / "fused.json", text + "\n");
  for (FILE* disk : disks) {
    CHECK_MSG(fclose(disk) == 0, "failed to write a fused file");
  }
  // "Copy original fused rig": the first .json under <bin> (getFirstFile walks the tree in directory order; here the
  // paths are sorted first, so that the choice does not depend on the file system)
  std::vector<fs::path> jsons;
  for (const auto& e : fs::recursive_directory_iterator(bin)) {
    if (e.is_regular_file() && !is_hidden(e.path()) && e.path().extension() == ".json") {
      jsons.push_back(e.path());
    }
  }
  CHECK_MSG(!jsons.empty(), "no .json rig in " + bin.string());
  std::sort(jsons.begin(), jsons.end());
  fs::copy_file(jsons[0], fused / jsons[0].filename(), fs::copy_options::overwrite_existing);
}

// ---------------------------------------------------------------- conversion
struct Timings {
  std::mutex mu;
  double build = 0, setup = 0, collapse = 0, write = 0, color = 0, parallel = 0;
  int meshes = 0;
  long long parallelPasses = 0;
  void add(double& slot, double s) {
    std::lock_guard<std::mutex> lk(mu);
    slot += s;
  }
};

static void write_floats(const fs::path& path, const void* data, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  CHECK_MSG(f != nullptr, "Cannot open file for writing: " + path.string());
  CHECK_MSG(fwrite(data, 1, bytes, f) == bytes && fclose(f) == 0, "failed to write: " + path.string());
}

// writeDepth + writeObj (MeshUtil.h:72-129) of one camera's final mesh
static void write_mesh(const Flags& F, const std::string& camId, const std::string& frameName, std::vector<double>& V,
                       const std::vector<int32_t>& Fc, bool clamp, bool saveMesh, bool saveObj) {
  const size_t nv = V.size() / 3, nf = Fc.size() / 3;
  std::vector<float> vtx(nv * 3);
  std::vector<uint32_t> idx(nf * 3);
  for (size_t i = 0; i < nv * 3; ++i) {
    // "If depth is slightly negative, the viewer will take it to -infinity" (:211-217): on the double, before the cast
    vtx[i] = clamp && i % 3 == 2 && V[i] < 0 ? FLT_MIN : (float)V[i];
  }
  for (size_t i = 0; i < nf * 3; ++i) {
    idx[i] = (uint32_t)Fc[i];
  }
  const fs::path dir = fs::path(F.s("bin")) / camId;
  fs::create_directories(dir);
  if (saveMesh) {
    write_floats(dir / (frameName + ".vtx"), vtx.data(), vtx.size() * 4);
    write_floats(dir / (frameName + ".idx"), idx.data(), idx.size() * 4);
  }
  if (saveObj) {  // readVertexes / readFaces of the two files just written: the float32 values, widened
    LOG_INFO(fmt("Exporting obj: frame %s, camera %s...", frameName.c_str(), camId.c_str()));
    const fs::path path = dir / (frameName + ".obj");
    FILE* fp = fopen(path.c_str(), "w");
    CHECK_MSG(fp != nullptr, "file open failed: " + path.string());
    for (size_t i = 0; i < nv; ++i) {
      fprintf(fp, "v %g %g %g\n", (double)vtx[3 * i], (double)vtx[3 * i + 1], (double)vtx[3 * i + 2]);
    }
    for (size_t i = 0; i < nf; ++i) {
      fprintf(fp, "f %d %d %d\n", (int)idx[3 * i] + 1, (int)idx[3 * i + 1] + 1, (int)idx[3 * i + 2] + 1);
    }
    CHECK_MSG(fclose(fp) == 0, "failed to write: " + path.string());
  }
}

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.str("bin", "bin", "output directory containing binary data");
  F.str("cameras", "", "cameras to render (comma-separated)");
  F.str("color", "", "path to input color images");
  F.dbl("color_scale", 1, "optional color scale before compression & fusion (>= 1 = no scale)");
  F.dbl("depth_scale", 1, "optional depthmap scale before simplification (>= 1 = no scale)");
  F.str("disparity", "", "path to disparity images (pfm)");
  F.str("first", "", "first frame to process (lexical) (required)");
  F.str("foreground_masks", "", "path to foreground masks specifying regions to include in per-frame geometry");
  F.i32("fuse_strip", 1, "number of strip files");
  F.str("fused", "", "output directory containing fused binary data, ready for playback");
  F.dbl("gamma_correction", 2.2 / 1.8, "exponent to raise color channels before BC7 encoding");
  F.str("last", "", "last frame to process (lexical) (required)");
  F.str("output_formats", "idx,vtx,bc7", "saved formats, comma separated (idx, vtx, bc7 default; rgba, pfm, obj also supported)");
  F.str("rig", "", "path to camera rig .json (required)");
  F.boolean("run_conversion", true, "whether or not to run binary conversion");
  F.dbl("tear_ratio", 0.95, "depth ratio that causes mesh to tear");
  F.i32("threads", -1, "number of threads (-1 = max allowed, 0 = no threading)");
  F.i32("triangles", 150000, "number of triangles per camera mesh (<= 0: no simplification)");
  F.i32("device", 0, "HIP device index [extension]");
  F.str("simplifier", "sequential", "[extension] mesh simplifier: sequential (the reference's collapse loop, on the host) or "
                                    "parallel (pass-parallel collapses on the device)");
  F.parse(argc, argv);

  CHECK_MSG(F.d("color_scale") <= 1., "color_scale <= 1");
  CHECK_MSG(F.d("depth_scale") <= 1., "depth_scale <= 1");
  CHECK_MSG(F.d("color_scale") > 0 && F.d("depth_scale") > 0, "color_scale > 0 and depth_scale > 0");
  CHECK_MSG(F.s("rig") != "", "rig");
  CHECK_MSG(F.s("first") != "", "first");
  CHECK_MSG(F.s("last") != "", "last");

  const std::string simplifier = F.s("simplifier");
  if (simplifier != "sequential" && simplifier != "parallel") {
    LOG_FATAL("Invalid --simplifier=" + simplifier + " (sequential or parallel)");
  }
  const bool parallel = simplifier == "parallel";

  // verifyInputs' format check (:93-97), and the two formats this build does not have: before any file or device
  std::vector<std::string> formats;
  {
    static const std::set<std::string> supported = {"idx", "vtx", "bc7", "obj", "pfm", "rgba"};
    std::stringstream ss(F.s("output_formats"));
    std::string item;
    while (std::getline(ss, item, ',')) {
      if (item.empty()) {
        continue;  // "exr,,png is fine"
      }
      CHECK_MSG(supported.count(item) != 0, "Invalid output format specified: " + item);
      formats.push_back(item);
    }
    for (const std::string& f : formats) {
      if (f == "bc7") {
        LOG_FATAL("output format bc7 is not built here (it needs the ISPC BC7 encoder); use --output_formats=idx,vtx,rgba");
      }
      if (f == "pfm") {
        LOG_FATAL("output format pfm is not built here (writePfm's barycentric solve needs Eigen); use "
                  "--output_formats=idx,vtx,rgba");
      }
    }
  }
  auto has = [&](const char* f) { return std::find(formats.begin(), formats.end(), f) != formats.end(); };
  const bool saveRgba = has("rgba"), saveMesh = has("idx") || has("vtx"), saveObj = has("obj");
  int firstFrame = 0, lastFrame = 0;
  try {
    firstFrame = std::stoi(F.s("first"));
    lastFrame = std::stoi(F.s("last"));
  } catch (...) {
    LOG_FATAL("Invalid frame name: " + F.s("first") + " / " + F.s("last"));
  }

  std::vector<derp_camera_desc> rig = filter_destinations(load_rig(F.s("rig")), F.s("cameras"));
  CHECK_MSG(!rig.empty(), "rig.size() > 0 No cameras to convert");

  // resizeRig (:318-339): scale every camera's resolution to its (scaled) colour image
  if (!F.s("color").empty()) {
    for (derp_camera_desc& cam : rig) {
      const fs::path path = image_path(F.s("color"), cam.id, F.s("first"));
      int w = 0, h = 0, cols = 0, rows = 0;
      CHECK_MSG(image_size(path, w, h), "failed to load image: " + path.string());
      scaled_size(w, h, F.d("color_scale"), cols, rows);
      const float xScale = float(cols) / cam.resolution[0], yScale = float(rows) / cam.resolution[1];
      CHECK_MSG(xScale == yScale, fmt("Aspect ratio must be kept. %gx%g vs %dx%d, x-scale: %g, y-scale: %g",
                                      cam.resolution[0], cam.resolution[1], cols, rows, xScale, yScale));
      if (&cam == &rig[0]) {
        LOG_INFO(fmt("Fusing color images at %dx%d resolution", cols, rows));
      }
      if (xScale != 1) {
        rescale_camera(cam, xScale * cam.resolution[0], xScale * cam.resolution[1]);
      }
    }
  }

  // verifyInputs (:88-116)
  const bool doColor = !F.s("color").empty() && saveRgba;
  const bool doDepth = !F.s("disparity").empty() && (saveMesh || saveObj);
  if (doColor) {
    verify_image_paths(F.s("color"), rig, F.s("first"), F.s("last"));
  } else {
    LOG_INFO("No color directory provided. Ignoring color conversion...");
  }
  if (doDepth) {
    verify_image_paths(F.s("disparity"), rig, F.s("first"), F.s("last"));
    if (!F.s("foreground_masks").empty()) {
      verify_image_paths(F.s("foreground_masks"), rig, F.s("first"), F.s("last"));
    }
  } else {
    LOG_INFO("No disparity directory provided. Ignoring depth conversion...");
  }

  if (F.b("run_conversion")) {
    // The collapse loops and the file writes share the pool. Unlike the other tools' I/O-bound pools (-1 = 1.5 workers
    // per usable CPU), these jobs compute and hold about a gigabyte each: -1 = one worker per usable CPU, 16 at the most
    const int threads = F.i("threads") < 0 ? std::min(IoPool::usable_cpus(), 16) : F.i("threads");
    IoPool pool(threads);
    derp_ctx* ctx = nullptr;
    if (doDepth || (doColor && F.d("color_scale") < 1)) {
      if (derp_create(&ctx, F.i("device"), rig.data(), (int)rig.size(), rig.data(), (int)rig.size()) != 0) {
        LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
      }
    }
    Timings T;
    Timer wall;
    std::deque<std::unique_ptr<IoBatch>> inFlight;  // collapse + write jobs, oldest first
    const size_t maxInFlight = (size_t)std::max(1, threads);
    const int triangles = F.i("triangles");
    for (int frame = firstFrame; frame <= lastFrame; ++frame) {
      const std::string frameName = zero_pad(frame, 6);
      for (size_t ci = 0; ci < rig.size(); ++ci) {
        const std::string camId = rig[ci].id;
        if (doColor) {  // convertColor (:118-148)
          LOG_INFO(fmt("Converting color: frame %s, camera %s...", frameName.c_str(), camId.c_str()));
          Timer t;
          int w = 0, h = 0, sw = 0, sh = 0;
          std::vector<uint8_t> rgba = load_rgba8(image_path(F.s("color"), camId, frameName), w, h);
          scaled_size(w, h, F.d("color_scale"), sw, sh);
          if (sw != w || sh != h) {  // INTER_AREA treats the channels alike: four single-channel resizes
            CHECK_MSG(sw > 0 && sh > 0, "color_scale leaves no pixels");
            const size_t n = (size_t)w * h, ns = (size_t)sw * sh;
            std::vector<uint8_t> plane(n), small(ns), out(ns * 4);
            for (int k = 0; k < 4; ++k) {
              for (size_t i = 0; i < n; ++i) {
                plane[i] = rgba[4 * i + k];
              }
              DERP_OK(ctx, derp_resize_area(ctx, 1, plane.data(), w, h, small.data(), sw, sh));
              for (size_t i = 0; i < ns; ++i) {
                out[4 * i + k] = small[i];
              }
            }
            rgba.swap(out);
          }
          const fs::path dir = fs::path(F.s("bin")) / camId;
          fs::create_directories(dir);
          write_floats(dir / (frameName + ".rgba"), rgba.data(), rgba.size());
          T.add(T.color, t.s());
        }
        if (!doDepth) {
          continue;
        }
        // convertDepth (:150-245)
        LOG_INFO(fmt("Converting depth: frame %s, camera %s...", frameName.c_str(), camId.c_str()));
        int w = 0, h = 0, mw = 0, mh = 0;
        const std::vector<float> disparity = read_pfm(image_path(F.s("disparity"), camId, frameName, ".pfm"), w, h);
        std::vector<uint8_t> mask;
        if (!F.s("foreground_masks").empty()) {
          mask = load_mask(image_path(F.s("foreground_masks"), camId, frameName), mw, mh);
        }
        Timer tb;
        DERP_OK(ctx, derp_mesh_build(ctx, (int)ci, disparity.data(), w, h, nullptr, F.d("depth_scale"),
                                     mask.empty() ? nullptr : mask.data(), mw, mh, (float)F.d("tear_ratio")));
        size_t nv = 0, nf = 0, nfAll = 0;
        DERP_OK(ctx, derp_mesh_counts(ctx, &nv, &nf, &nfAll));
        const bool onDevice = parallel && triangles > 0;  // the mesh leaves the device simplified
        auto V = std::make_shared<std::vector<double>>(onDevice ? 0 : nv * 3);
        auto Fc = std::make_shared<std::vector<int32_t>>(onDevice ? 0 : nf * 3);
        if (!onDevice) {
          DERP_OK(ctx, derp_mesh_download_f64(ctx, V->data(), Fc->data()));
        }
        T.add(T.build, tb.s());
        LOG_INFO(fmt("Removed %zu of %zu faces (%.2f%%) corresponding to invalid depths and masked vertexes", nfAll - nf,
                     nfAll, 100.f * (nfAll - nf) / (float)nfAll));
        if (onDevice) {
          LOG_INFO(fmt("Target number of faces: %d", triangles));
          Timer tp;
          int stats[2] = {0, 0};
          // the rules of MeshSimplifier(vertexes, faces, kIsEquierror, 1).simplify(triangles, 0.2, false)
          DERP_OK(ctx, derp_mesh_simplify_parallel(ctx, triangles, 0.2f, 0, 1, stats));
          size_t onv = 0, onf = 0;
          DERP_OK(ctx, derp_mesh_counts(ctx, &onv, &onf, nullptr));
          V->resize(onv * 3);
          Fc->resize(onf * 3);
          DERP_OK(ctx, derp_mesh_download_f64(ctx, V->data(), Fc->data()));
          const double seconds = tp.s();
          T.add(T.parallel, seconds);
          T.parallelPasses += stats[0];
          for (int pass = 0; pass < stats[0]; ++pass) {
            derp_mesh_pass info;
            DERP_OK(ctx, derp_mesh_parallel_pass(ctx, pass, &info));
            LOG_INFO(fmt("Iter: %d, faces: %lld, threshold: %g", pass, info.faces, info.threshold));
          }
          static const char* kExit[] = {"the budget", "an infinite threshold", "a stuck threshold", "no candidate"};
          LOG_INFO(fmt("Simplified frame %s, camera %s: %zu faces after %d passes in %.3f s on the device (ended by %s)",
                       frameName.c_str(), camId.c_str(), onf, stats[0], seconds, kExit[stats[1] & 3]));
          while (inFlight.size() >= maxInFlight) {
            inFlight.front()->wait();
            inFlight.pop_front();
          }
          inFlight.emplace_back(new IoBatch);
          inFlight.back()->add(pool, [&F, &T, camId, frameName, V, Fc, saveMesh, saveObj] {
            Timer tw;
            write_mesh(F, camId, frameName, *V, *Fc, true, saveMesh, saveObj);
            T.add(T.write, tw.s());
          }, 1);
          ++T.meshes;
          continue;
        }
        auto planes = std::make_shared<std::vector<double>>(), costs = std::make_shared<std::vector<double>>(),
             vq = std::make_shared<std::vector<double>>();
        if (triangles > 0) {
          LOG_INFO(fmt("Target number of faces: %d", triangles));
          Timer ts;
          planes->resize(nf * 4);
          costs->resize(nf * 3);
          vq->resize(nv * 10);
          DERP_OK(ctx, derp_mesh_setup(ctx, 1, planes->data(), costs->data(), vq->data()));
          T.add(T.setup, ts.s());
        }
        while (inFlight.size() >= maxInFlight) {
          inFlight.front()->wait();
          inFlight.pop_front();
        }
        inFlight.emplace_back(new IoBatch);
        inFlight.back()->add(pool, [&F, &T, camId, frameName, V, Fc, planes, costs, vq, triangles, saveMesh, saveObj] {
          std::vector<double> outV;
          std::vector<int32_t> outF;
          if (triangles > 0) {
            Timer tc;
            outV.resize(V->size());
            outF.resize(Fc->size());
            size_t onv = 0, onf = 0;
            int stats[2] = {0, 0};
            // MeshSimplifier(vertexes, faces, kIsEquierror, 1).simplify(triangles, 0.2, false)
            CHECK_MSG(derp_mesh_simplify_host(V->data(), V->size() / 3, Fc->data(), Fc->size() / 3, planes->data(), costs->data(),
                                              vq->data(), triangles, 0.2f, 0, 1, outV.data(), outF.data(), &onv, &onf,
                                              stats) == 0,
                      "derp_mesh_simplify_host refused the mesh of camera " + camId);
            outV.resize(onv * 3);
            outF.resize(onf * 3);
            T.add(T.collapse, tc.s());
            LOG_INFO(fmt("Simplified frame %s, camera %s: %zu faces after %d passes", frameName.c_str(), camId.c_str(), onf,
                         stats[0]));
          } else {
            outV = *V;
            outF = *Fc;
          }
          Timer tw;
          write_mesh(F, camId, frameName, outV, outF, triangles > 0, saveMesh, saveObj);
          T.add(T.write, tw.s());
        }, 1);  // class 1: every worker of the pool takes it (class 2 leaves the two express workers idle)
        ++T.meshes;
      }
    }
    for (auto& b : inFlight) {
      b->wait();
    }
    if (ctx) {
      derp_destroy(ctx);
    }
    if (T.meshes > 0) {
      const double n = T.meshes;
      LOG_INFO(fmt("Timing: %d camera meshes in %.3f s wall; per mesh: device build %.4f s, device set-up %.4f s, host "
                   "collapse %.4f s, file writes %.4f s, device simplifier %.4f s in %.1f passes",
                   T.meshes, wall.s(), T.build / n, T.setup / n, T.collapse / n, T.write / n, T.parallel / n,
                   T.parallelPasses / n));
    }
    fs::create_directories(F.s("bin"));
    save_rig(fs::path(F.s("bin")) / (fs::path(F.s("rig")).stem().string() + "_fused.json"), rig,
             rig_groups(F.s("rig")), 10);
  }

  if (!F.s("fused").empty()) {
    fuse(F, rig, formats);
  }
  return EXIT_SUCCESS;
}
