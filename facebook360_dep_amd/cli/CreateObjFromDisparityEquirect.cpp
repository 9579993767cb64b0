// CreateObjFromDisparityEquirect — drop-in for source/conversion/CreateObjFromDisparityEquirect.cpp: a disparity
// equirect -> the scene as one mesh in rig coordinates that closes over the 0 / 360 degree seam, simplified to
// --num_faces, as an OBJ; with --create_mtl also <obj stem>.mtl that maps the colour equirect onto it. Same 10 flags
// (:36-45) and checks. Compute = derp_mesh_build_equirect on the GPU, then derp_mesh_simplify (the reference's
// sequential collapse loop on the host, set-up on the GPU) or, with --simplifier=parallel [extension],
// derp_mesh_simplify_parallel (pass-parallel collapses on the device). Where this tool leaves the reference on purpose:
// --create_mtl works (the reference's material name is shadowed at :91 and writeObj's check aborts), and --scale < 1 is
// a defined bilinear rule instead of cv::resize's INTER_LINEAR bits (resize_bilinear below).
#include "cli_common.h"
#include "rig_writer.h"

using namespace cli;

static const char* kUsage = R"(
  - Creates an OBJ (optionally with texturing) from a disparity equirect.

  - Example:
    ./CreateObjFromDisparityEquirect \
    --input_png_color=/path/to/equirects/color.png \
    --input_png_disp=/path/to/equirects/disparity.png \
    --output_obj=/path/to/output/test.obj
  )";

// --scale < 1: the destination has nearbyint(size * scale) pixels a side; destination pixel d reads the source at
// (d + 0.5) / scale - 0.5 (float), between the two pixels around it, both clamped to the image; rows first, then columns
struct Taps {
  std::vector<int> lo, hi;
  std::vector<float> frac;
};
static Taps bilinear_taps(int ssize, int dsize, float scale) {
  Taps t;
  t.lo.resize(dsize);
  t.hi.resize(dsize);
  t.frac.resize(dsize);
  for (int d = 0; d < dsize; ++d) {
    const float s = ((float)d + 0.5f) / scale - 0.5f;
    const float f = std::floor(s);
    t.frac[d] = s - f;
    t.lo[d] = std::min(std::max((int)f, 0), ssize - 1);
    t.hi[d] = std::min(std::max((int)f + 1, 0), ssize - 1);
  }
  return t;
}
static std::vector<float> resize_bilinear(const std::vector<float>& src, int w, int h, double scale, int& dw, int& dh) {
  dw = (int)std::nearbyint(w * scale);
  dh = (int)std::nearbyint(h * scale);
  CHECK_MSG(dw > 0 && dh > 0, fmt("scale %g leaves no pixels of a %d x %d map", scale, w, h));
  const Taps tx = bilinear_taps(w, dw, (float)scale), ty = bilinear_taps(h, dh, (float)scale);
  std::vector<float> rows((size_t)h * dw), out((size_t)dw * dh);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < dw; ++x) {
      const float a = src[(size_t)y * w + tx.lo[x]], b = src[(size_t)y * w + tx.hi[x]];
      const float wa = a * (1.0f - tx.frac[x]), wb = b * tx.frac[x];
      rows[(size_t)y * dw + x] = wa + wb;
    }
  }
  for (int y = 0; y < dh; ++y) {
    for (int x = 0; x < dw; ++x) {
      const float a = rows[(size_t)ty.lo[y] * dw + x], b = rows[(size_t)ty.hi[y] * dw + x];
      const float wa = a * (1.0f - ty.frac[y]), wb = b * ty.frac[y];
      out[(size_t)y * dw + x] = wa + wb;
    }
  }
  return out;
}

// a context needs a camera; this mesh reads none
static derp_camera_desc placeholder_camera() {
  derp_camera_desc c;
  memset(&c, 0, sizeof c);
  c.type = DERP_FTHETA;
  snprintf(c.id, sizeof c.id, "equirect");
  c.forward[2] = -1;
  c.up[1] = 1;
  c.right[0] = 1;
  c.resolution[0] = c.resolution[1] = 2;
  c.focal[0] = 1;
  c.focal[1] = -1;
  return c;
}

// writeMtl (MeshUtil.h:131-144) -> the file's name, as mtllib names it
static std::string write_mtl(const fs::path& pathObj, const fs::path& pathColor) {
  const fs::path dir = pathObj.parent_path().empty() ? fs::path(".") : pathObj.parent_path();
  const std::string rel = fs::relative(pathColor, dir).string();
  fs::path pathMtl(pathObj);
  pathMtl.replace_extension(".mtl");
  write_text(pathMtl, "newmtl material\nillum 0\nKd 1 1 1\nmap_Kd " + rel + "\n");
  return pathMtl.filename().string();
}

// writeObj (MeshUtil.h:91-129); st == nullptr: no texture coordinates and no material
static void write_obj(const fs::path& path, const std::vector<double>& V, const std::vector<int32_t>& Fc, const double* st,
                      const std::string& mtl) {
  FILE* fp = fopen(path.c_str(), "w");
  CHECK_MSG(fp != nullptr, "file open failed: " + path.string());
  if (st) {
    fprintf(fp, "mtllib %s\nusemtl material\n", mtl.c_str());
  }
  const size_t nv = V.size() / 3, nf = Fc.size() / 3;
  for (size_t i = 0; i < nv; ++i) {
    fprintf(fp, "v %g %g %g\n", V[3 * i], V[3 * i + 1], V[3 * i + 2]);
    if (st) {
      fprintf(fp, "vt %g %g\n", st[2 * i], st[2 * i + 1]);
    }
  }
  for (size_t i = 0; i < nf; ++i) {
    const int a = Fc[3 * i] + 1, b = Fc[3 * i + 1] + 1, c = Fc[3 * i + 2] + 1;
    if (st) {
      fprintf(fp, "f %d/%d %d/%d %d/%d\n", a, a, b, b, c, c);
    } else {
      fprintf(fp, "f %d %d %d\n", a, b, c);
    }
  }
  CHECK_MSG(fclose(fp) == 0, "failed to write: " + path.string());
}

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.boolean("create_mtl", false, "cerate MTL file and attach to OBJ");
  F.str("input_png_color", "", "path to input color png (required)");
  F.str("input_png_disp", "", "path to input disparity png (required)");
  F.dbl("max_depth", 700.0, "maximum depth. Use something like 20 to visualize");
  F.i32("num_faces", 200000, "number of output faces");
  F.str("output_obj", "", "path to output obj file (required)");
  F.dbl("scale", 1.0, "depth map resolution before decimation");
  F.dbl("strictness", 0.8, "[0, 1] mesh simplification aggressiveness. 0 = no simplification");
  F.dbl("tear_ratio", 0.95, "depth ratio that causes mesh to tear");
  F.i32("threads", 12, "number of threads");
  F.i32("device", 0, "HIP device index [extension]");
  F.str("simplifier", "sequential", "[extension] mesh simplifier: sequential (the reference's collapse loop, on the host) or "
                                    "parallel (pass-parallel collapses on the device)");
  F.parse(argc, argv);

  CHECK_MSG(F.s("input_png_disp") != "", "input_png_disp");
  CHECK_MSG(F.s("input_png_color") != "", "input_png_color");
  CHECK_MSG(F.s("output_obj") != "", "output_obj");
  const double strictness = F.d("strictness"), scale = F.d("scale");
  CHECK_MSG(0 <= strictness && strictness <= 1, "strictness must be between 0 and 1");
  const std::string simplifier = F.s("simplifier");
  if (simplifier != "sequential" && simplifier != "parallel") {
    LOG_FATAL("Invalid --simplifier=" + simplifier + " (sequential or parallel)");
  }
  CHECK_MSG(0 < scale && scale <= 1, "scale must be in (0, 1]");
  CHECK_MSG(F.i("num_faces") >= 0, "num_faces >= 0");

  LOG_INFO("Reading disparity image...");
  int w = 0, h = 0;
  std::vector<float> disp = load_float(F.s("input_png_disp"), w, h);
  if (scale < 1) {
    LOG_INFO("Resizing input file...");
    int dw = 0, dh = 0;
    disp = resize_bilinear(disp, w, h, scale, dw, dh);
    w = dw;
    h = dh;
  }

  derp_ctx* ctx = nullptr;
  const derp_camera_desc cam = placeholder_camera();
  if (derp_create(&ctx, F.i("device"), &cam, 1, &cam, 1) != 0) {
    LOG_FATAL(std::string("derp_create failed: ") + derp_last_error(nullptr));
  }
  LOG_INFO("Generating vertexes and faces...");
  Timer tb;
  DERP_OK(ctx, derp_mesh_build_equirect(ctx, disp.data(), w, h, (float)F.d("max_depth"), (float)F.d("tear_ratio")));
  size_t nv = 0, nf = 0;
  DERP_OK(ctx, derp_mesh_counts(ctx, &nv, &nf, nullptr));
  LOG_INFO(fmt("Built %zu vertexes and %zu faces of a %d x %d equirect in %.3f s", nv, nf, w, h, tb.s()));
  if (strictness > 0) {
    LOG_INFO("Mesh simplification...");
    Timer ts;
    int stats[2] = {0, 0};
    // MeshSimplifier(vertexes, faces, kIsEquiError = false, threads).simplify(num_faces, strictness)
    if (simplifier == "parallel") {
      DERP_OK(ctx, derp_mesh_simplify_parallel(ctx, F.i("num_faces"), (float)strictness, 0, 0, stats));
    } else {
      DERP_OK(ctx, derp_mesh_simplify(ctx, F.i("num_faces"), (float)strictness, 0, 0, 0, stats));
    }
    DERP_OK(ctx, derp_mesh_counts(ctx, &nv, &nf, nullptr));
    static const char* kExit[] = {"the budget", "an infinite threshold", "a stuck threshold", "no candidate"};
    LOG_INFO(fmt("Simplified to %zu faces after %d passes in %.3f s (%s, ended by %s)", nf, stats[0], ts.s(), simplifier.c_str(),
                 kExit[stats[1] & 3]));
  }
  std::vector<double> V(nv * 3);
  std::vector<int32_t> Fc(nf * 3);
  DERP_OK(ctx, derp_mesh_download_f64(ctx, V.data(), Fc.data()));
  derp_destroy(ctx);
  LOG_INFO(fmt("Num vertexes: %zu, num faces: %zu", V.size(), Fc.size()));  // (Eigen's size(): rows x cols)

  LOG_INFO("Creating OBJ...");
  const fs::path pathObj(F.s("output_obj"));
  if (F.b("create_mtl")) {
    std::vector<double> st(nv * 2);
    CHECK_MSG(derp_mesh_texcoords_equirect(V.data(), nv, st.data()) == 0, "derp_mesh_texcoords_equirect");
    write_obj(pathObj, V, Fc, st.data(), write_mtl(pathObj, F.s("input_png_color")));
  } else {
    write_obj(pathObj, V, Fc, nullptr, "");
  }
  return EXIT_SUCCESS;
}
