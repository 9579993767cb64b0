// RigAnalyzer — drop-in for source/rig/RigAnalyzer.cpp: same flags (:30-65), same order of work as main() (:478-612) and
// the same outputs: the 20-line coverage sweep on stdout, --output_rig, --output_obj, and the plain PGM maps
// --output_equirect, --output_camera and --output_cross_section. The rig is built and edited on the host (derp_rig_*);
// every camera count is a GPU pass (derp_coverage_*). No device is opened when neither the sweep nor a map is asked for.
#include "rig_writer.h"

using namespace cli;

static const char* kUsage = R"(
   - Miscellaneous analysis utilities for a rig. Various output formats are supported to
   visualize the rig setup (e.g. equirect projection).

   - --sample_count=0 skips the coverage sweep; with no map requested the rig is only edited and no device is opened.

   - Example:
     ./RigAnalyzer \
     --rig=/path/to/rigs/rig.json \
     --output_equirect=/path/to/output/equirect.png
 )";

#define HOST_OK(expr)                                                      \
  do {                                                                     \
    if ((expr) != 0) {                                                     \
      LOG_FATAL(std::string(derp_last_error(nullptr)));                    \
    }                                                                      \
  } while (0)

// `file << double` with the stream's default precision
static std::string g6(double v) {
  return fmt("%g", v);
}

// readVectorFile (:462-476): three numbers per line; lines beginning with "===" are skipped
static std::vector<double> read_vector_file(const std::string& filename) {
  std::vector<double> result;
  std::ifstream file(filename);
  CHECK_MSG(file.good(), "could not read file: " + filename);
  for (std::string line; getline(file, line);) {
    if (line.find("===") == 0) {
      continue;
    }
    std::istringstream s(line);
    double a[3];
    s >> a[0] >> a[1] >> a[2];
    CHECK_MSG(!s.fail(), "bad line <" + line + "> in file " + filename);
    result.insert(result.end(), a, a + 3);
  }
  CHECK_MSG(!result.empty(), "no angles in file " + filename);
  return result;
}

static int find_camera(const std::vector<derp_camera_desc>& rig, const std::string& id) {
  for (size_t i = 0; i < rig.size(); ++i) {
    if (id == rig[i].id) {
      return (int)i;
    }
  }
  LOG_FATAL("Camera id " + id + " not found");
  return -1;
}

// ---- saveRigObj (:271-344) ----
struct V3 {
  double x, y, z;
};
static V3 axpy(const V3& a, double s, const V3& b) {  // a + s * b
  return {a.x + s * b.x, a.y + s * b.y, a.z + s * b.z};
}
static void obj_face(std::string& out, const V3& color, const std::vector<V3>& positions) {
  const double kScale = 1000;  // CAD wants mm, json is meters
  for (const V3& p : positions) {
    out += "v " + g6(kScale * p.x) + " " + g6(kScale * p.y) + " " + g6(kScale * p.z) + " " + g6(color.x) + " " +
        g6(color.y) + " " + g6(color.z) + "\n";
  }
  const int n = (int)positions.size();
  for (int order = 0; order < 2; ++order) {  // both orders, to avoid backface culling
    out += "f";
    for (int i = 0; i < n; ++i) {
      out += " " + std::to_string(order ? -n + i : -1 - i);
    }
    out += "\n";
  }
}
static void obj_arrow(std::string& out, const V3& color, const V3& base, const V3& dir, const V3& t0, const V3& t1,
                      double length = 0.01, double radius = 0.001) {
  obj_face(out, color, {axpy(base, length, dir), axpy(base, radius, t0), axpy(base, -radius, t0)});
  obj_face(out, color, {axpy(base, length, dir), axpy(base, radius, t1), axpy(base, -radius, t1)});
}
static std::string rig_obj(const std::vector<derp_camera_desc>& rig) {
  std::string out;
  for (int i = 0; i < (int)rig.size(); ++i) {
    const derp_camera_desc& c = rig[i];
    const V3 p = {c.origin[0], c.origin[1], c.origin[2]}, f = {c.forward[0], c.forward[1], c.forward[2]};
    const V3 r = {c.right[0], c.right[1], c.right[2]}, u = {c.up[0], c.up[1], c.up[2]};
    // a camera is white forward, green right and blue up arrows
    obj_arrow(out, {1, 1, 1}, p, f, r, u, 0.02);
    obj_arrow(out, {0, 1, 0}, p, r, u, f);
    obj_arrow(out, {0, 0, 1}, p, u, f, r);
    for (int tri = 0; tri < i; ++tri) {  // the index as i triangles
      const double kSize = 0.002;
      const V3 v = axpy(p, -(kSize * tri), r);
      obj_face(out, {1, 0, 0}, {v, axpy(v, -kSize, r), axpy(v, -kSize, u)});
    }
  }
  obj_arrow(out, {1, 1, 0}, {0, 0, -1}, {0, 0, 1}, {1, 0, 0}, {0, 1, 0}, 1.0, 0.01);
  return out;
}

// plain PGM as the reference's streams leave it: every value followed by one space, every row by a newline
template <typename Value>
static void write_pgm(const std::string& path, int w, int h, size_t maxval, Value value) {
  std::string out = "P2\n" + std::to_string(w) + " " + std::to_string(h) + "\n" + std::to_string(maxval) + "\n";
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) {
      out += std::to_string(value((size_t)y * w + x));
      out += ' ';
    }
    out += '\n';
  }
  write_text(path, out);
}

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.dbl("custom", -1, "custom angle away from north");
  F.dbl("discard_poles", 0, "degrees from poles to ignore");
  F.str("eulers", "", "create from eulers file");
  F.dbl("min_distance", 0.50, "min distance to test");
  F.dbl("overlap_distance", 1e4, "distance to visualize equirect overlap, default is INF");
  F.boolean("one_based_indexing", false, "enable to index cameras starting at 1 instead of 0");
  F.str("output_camera", "", "path to output camera .ppm file");
  F.str("output_camera_id", "", "output camera id");
  F.str("output_cross_section", "", "path to output cross section .ppm file");
  F.str("output_equirect", "", "path to output equirect .ppm file");
  F.str("output_obj", "", "path to output rig .obj file");
  F.str("output_rig", "", "path to output rig .json file");
  F.boolean("perturb_cameras", false, "");
  F.dbl("perturb_focals", 0, "pertub focals");
  F.dbl("perturb_positions", 0, "perturb positions (cm)");
  F.dbl("perturb_principals", 0, "pertub principals (pixels)");
  F.dbl("perturb_rotations", 0, "perturb rotations (radians)");
  F.i32("perturb_seed", 1, "seed for perturb cameras. Default: 1, same as no seed");
  F.dbl("radius", 0, "change rig radius");
  F.str("rearrange", "", "create specific arrangement (ballcam24, tetra, ring4, cube, carbon0, carbon1, diamond)");
  F.str("revolve", "", "create from angle file");
  F.str("rig", "", "path to rig .json file (required)");
  F.str("rotate", "", "rotate rig by euler angles");
  F.str("rotate_cam_z", "", "rotate camera to align with z");
  F.i32("sample_count", 100000, "number of samples");
  F.dbl("scale_resolution", 1, "scale camera resolutions");
  F.boolean("show_timing", false, "visualize time as well as spatial overlap");
  F.boolean("z_is_down", false, "modify rig from y-is-up to z-is-down");
  F.boolean("z_is_up", false, "modify rig from y-is-up to z-is-up");
  F.dbl("scale_rig", 1, "scale rig space, e.g., by 1e-2 to convert from cm to m");
  F.i32("device", 0, "HIP device index [extension]");
  F.parse(argc, argv);
  CHECK_MSG(F.s("rig") != "", "rig");
  CHECK_MSG(F.i("sample_count") >= 0, "sample_count >= 0");
  CHECK_MSG(F.s("output_camera").empty() == F.s("output_camera_id").empty(),
            "--output_camera and --output_camera_id go together");

  // Read the cameras
  std::vector<derp_camera_desc> rig = load_rig(F.s("rig"));
  CHECK_MSG(!rig.empty(), "rig.size() > 0");

  // Modify rig
  const auto renumbered = [&](std::vector<derp_camera_desc> cams) {
    if (F.b("one_based_indexing")) {
      for (size_t i = 0; i < cams.size(); ++i) {
        snprintf(cams[i].id, sizeof cams[i].id, "cam%zu", i + 1);
      }
    }
    return cams;
  };
  if (!F.s("rearrange").empty()) {  // clone rig[0] into named configuration
    std::vector<derp_camera_desc> out(DERP_RIG_ARRANGEMENT_MAX);
    int n = 0;
    HOST_OK(derp_rig_arrangement(F.s("rearrange").c_str(), &rig[0], F.d("custom"), out.data(), &n));
    out.resize(n);
    rig = renumbered(out);
  } else if (!F.s("eulers").empty()) {  // clone first camera according to eulers
    const std::vector<double> e = read_vector_file(F.s("eulers"));
    std::vector<derp_camera_desc> out(e.size() / 3);
    HOST_OK(derp_rig_from_eulers(&rig[0], e.data(), (int)out.size(), 0, out.data()));
    rig = renumbered(out);
  } else if (!F.s("revolve").empty()) {
    const std::vector<double> e = read_vector_file(F.s("revolve"));
    std::vector<derp_camera_desc> out(e.size() / 3 * rig.size());
    HOST_OK(derp_rig_revolve(rig.data(), (int)rig.size(), e.data(), (int)(e.size() / 3), out.data()));
    rig = out;
  } else if (F.b("perturb_cameras")) {
    HOST_OK(derp_rig_perturb(rig.data(), (int)rig.size(), F.i("perturb_seed"), F.d("perturb_positions"),
                             F.d("perturb_rotations"), F.d("perturb_principals"), F.d("perturb_focals")));
  }
  const auto rotated = [&](const double* m) {
    std::vector<derp_camera_desc> out(rig.size());
    HOST_OK(derp_rig_rotate(rig.data(), (int)rig.size(), m, out.data()));
    rig = out;
  };
  if (!F.s("rotate_cam_z").empty()) {
    double m[9];
    HOST_OK(derp_rig_align_z_matrix(rig[find_camera(rig, F.s("rotate_cam_z"))].origin, m));
    rotated(m);
  }
  if (F.b("z_is_up") || F.b("z_is_down") || !F.s("rotate").empty()) {
    double m[9] = {1, 0, 0, 0, 0, -1, 0, 1, 0};
    if (F.b("z_is_up")) {
    } else if (F.b("z_is_down")) {
      m[5] = 1;
      m[7] = -1;
    } else {
      double euler[3];
      std::istringstream s(F.s("rotate"));
      s >> euler[0] >> euler[1] >> euler[2];
      CHECK_MSG(s.eof() && !s.fail(), "bad --rotate vector " + F.s("rotate"));
      HOST_OK(derp_rig_euler_matrix(euler, 1, m));
    }
    rotated(m);
  }
  if (F.d("scale_rig") != 1) {
    LOG_INFO("scaling rig by " + g6(F.d("scale_rig")));
  }
  HOST_OK(derp_rig_scale(rig.data(), (int)rig.size(), F.d("scale_rig"), F.d("radius"), F.d("scale_resolution")));

  // what the reference leaves undefined is settled before any device is opened
  const int mapCam = F.s("output_camera_id").empty() ? -1 : find_camera(rig, F.s("output_camera_id"));
  const int S = (int)rig.size();

  // Generate the directions that we want to test
  int kept = 0;
  std::vector<double> samples((size_t)F.i("sample_count") * 3);
  HOST_OK(derp_rig_fibonacci_units(F.i("sample_count"), F.d("discard_poles"), samples.data(), &kept));
  const bool sweep = F.i("sample_count") > 0;
  CHECK_MSG(!sweep || kept > 0, fmt("--discard_poles=%g leaves no sample of %d", F.d("discard_poles"), F.i("sample_count")));

  derp_ctx* ctx = nullptr;
  if (sweep || !F.s("output_equirect").empty() || mapCam >= 0 || !F.s("output_cross_section").empty()) {
    CHECK_MSG(S <= 255, fmt("too many cameras (%d > 255): coverage counts are 8-bit", S));
    if (derp_create(&ctx, F.i("device"), rig.data(), S, rig.data(), S) != 0) {
      LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
    }
  }

  // Go through N distances from min_distance to kNearInfinity
  if (sweep) {
    const int kN = DERP_RIG_COVERAGE_DISTANCES;
    double distances[kN];
    HOST_OK(derp_rig_coverage_distances(F.d("min_distance"), distances));
    std::vector<int32_t> hist((size_t)kN * (S + 1));
    DERP_OK(ctx, derp_coverage_directions(ctx, samples.data(), kept, distances, kN, hist.data(), nullptr));
    for (int i = 0; i < kN; ++i) {
      const int32_t* h = &hist[(size_t)i * (S + 1)];
      int minC = 0, maxC = S;
      while (h[minC] == 0) {
        ++minC;
      }
      while (h[maxC] == 0) {
        --maxC;
      }
      const double quality = minC + (kept - h[minC]) / double(kept);
      std::string line = fmt("distance: %.2f quality: %.2f samples: %d ", distances[i], quality, kept);
      for (int k = 0; k <= maxC; ++k) {
        line += "h[" + std::to_string(k) + "] = " + std::to_string(h[k]) + ", ";
      }
      printf("%s\n", line.c_str());
    }
    fflush(stdout);
  }

  // Write the cameras
  if (!F.s("output_rig").empty()) {
    std::string commandLine;
    for (int i = 0; i < argc; ++i) {
      commandLine += (i ? " " : "") + std::string(argv[i]);
    }
    save_rig(F.s("output_rig"), rig, {}, -1, {"command line:", commandLine});
  }
  if (!F.s("output_obj").empty()) {
    write_text(F.s("output_obj"), rig_obj(rig));
  }
  if (!F.s("output_equirect").empty()) {
    const int kPixelsPerDegree = 5;
    const int w = 360 * kPixelsPerDegree, h = 180 * kPixelsPerDegree;
    std::vector<uint8_t> counts((size_t)w * h);
    std::vector<float> minTiming((size_t)w * h);
    double stats[3];
    DERP_OK(ctx, derp_coverage_equirect(ctx, kPixelsPerDegree, F.d("overlap_distance"), counts.data(), minTiming.data(), stats));
    if (F.b("show_timing")) {
      write_pgm(F.s("output_equirect"), w, h, 256, [&](size_t i) { return int((1.0 - (double)minTiming[i]) * 255.0); });
    } else {
      write_pgm(F.s("output_equirect"), w, h, (size_t)S, [&](size_t i) { return (int)counts[i]; });
    }
    const float kFrameRate = 60.0f;                 // 60 fps
    const float kFrameTime = 1000.0f / kFrameRate;  // in milliseconds
    LOG_INFO("Holes found (in pixels) = " + g6(stats[0]));
    LOG_INFO("Max of min timing distance = " + g6(kFrameTime * stats[1]) + "ms");
    LOG_INFO("Ave of min timing distance = " + g6(kFrameTime * stats[2] / (w * h)) + "ms");
  }
  if (mapCam >= 0) {
    const int w = (int)rig[mapCam].resolution[0], h = (int)rig[mapCam].resolution[1];
    std::vector<uint8_t> counts((size_t)std::max(w, 0) * std::max(h, 0));
    DERP_OK(ctx, derp_coverage_camera(ctx, mapCam, F.d("overlap_distance"), counts.data()));
    write_pgm(F.s("output_camera"), w, h, (size_t)S, [&](size_t i) { return (int)counts[i]; });
  }
  if (!F.s("output_cross_section").empty()) {
    const int kDim = 400;
    std::vector<uint8_t> counts((size_t)kDim * kDim);
    DERP_OK(ctx, derp_coverage_cross_section(ctx, kDim, counts.data()));
    write_pgm(F.s("output_cross_section"), kDim, kDim, (size_t)S, [&](size_t i) { return (int)counts[i]; });
  }
  if (ctx) {
    derp_destroy(ctx);
  }
  return EXIT_SUCCESS;
}
