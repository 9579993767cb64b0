// RigSimulator — drop-in for source/rig/RigSimulator.cpp: same 40 flags (:46-121), modes and outputs. A procedural scene
// (icosahedra, two cubes or a ground plane, in front of a skybox) is ray-traced on the GPU as a rig sees it
// (derp_sim_*): per camera <id>.png, <id>_depth.png and <id>_depth.pfm, the rig as JSON, or a mono / stereo equirect.
// Scene and sphere tree are built on the host with the C library's rand(), scene first, as the reference does; the
// image noise (--noise_amplitude) is drawn on the host camera by camera in rig order (the reference's render threads
// race on rand() there). Every bad input is refused before a device is opened.
#include <cfloat>

#include "rig_writer.h"

using namespace cli;

static const char* kUsage = R"(
  - Render an artificial scene as seen by the specified rig.

  - Example:
    ./RigSimulator \
    --mode=pinhole_ring \
    --skybox_path=/path/to/skybox.png
)";

struct V3 {
  double x, y, z;
};
static V3 cross(const V3& a, const V3& b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
static V3 normalized(const V3& a) {
  const double n = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return {a.x / n, a.y / n, a.z / n};
}
static float to_radians(float deg) {  // MathUtil.h:27-29
  return deg * static_cast<float>(M_PI) / 180.0f;
}

// Camera::Camera(type, resolution, focal) (Camera.cpp:21-28): at the origin, principal in the middle, no distortion,
// the type's default fov
static derp_camera_desc generic_camera(int type, int w, int h, double fx, double fy) {
  derp_camera_desc c;
  memset(&c, 0, sizeof c);
  c.type = type;
  c.resolution[0] = w;
  c.resolution[1] = h;
  c.focal[0] = fx;
  c.focal[1] = fy;
  return c;
}
// Camera::setRotation(forward, up) (Camera.cpp:89-91): right = forward x up. The vectors are kept as given; the
// reference passes them through Eigen::AngleAxis and back, which moves an orthonormal frame by rounding errors only.
static void set_rotation(derp_camera_desc& c, const V3& forward, const V3& up) {
  const V3 right = cross(forward, up);
  const double f[3] = {forward.x, forward.y, forward.z}, u[3] = {up.x, up.y, up.z}, r[3] = {right.x, right.y, right.z};
  memcpy(c.forward, f, sizeof f);
  memcpy(c.up, u, sizeof u);
  memcpy(c.right, r, sizeof r);
}
static void set_id(derp_camera_desc& c, size_t i) {
  snprintf(c.id, sizeof c.id, "%zu", i);
}

struct Rig {
  std::vector<derp_camera_desc> cameras;
  std::map<std::string, std::string> groups;
};

// ringOfClones, RigSimulator.cpp:360-372
static void ring_of_clones(Rig& rig, const derp_camera_desc& camera, int count, double radius) {
  for (int i = 0; i < count; ++i) {
    const double theta = -2.0 * M_PI * double(i) / double(count);  // clockwise
    derp_camera_desc clone = camera;
    const V3 forward = {std::cos(theta), std::sin(theta), 0};
    set_rotation(clone, forward, {0, 0, 1});
    clone.origin[0] = radius * forward.x;
    clone.origin[1] = radius * forward.y;
    clone.origin[2] = radius * forward.z;
    set_id(clone, (size_t)i);
    rig.groups[clone.id] = "side camera";
    rig.cameras.push_back(clone);
  }
}
// makeGenericFTheta, :389-398: focal = 2 * radius / toRadians(fov), an int over a float
static derp_camera_desc generic_ftheta(int w, int h, int imageCircleRadius, float circleFov) {
  const double focal = (double)((float)(2 * imageCircleRadius) / to_radians(circleFov));
  return generic_camera(DERP_FTHETA, w, h, focal, focal);
}
// makeFThetaCameraOnSphere, :426-444 (the position is image circle radius x normal there, not the sphere's radius)
static derp_camera_desc ftheta_on_sphere(const V3& normal, int w, int h, int imageCircleRadius, float circleFov, size_t id) {
  derp_camera_desc c = generic_ftheta(w, h, imageCircleRadius, circleFov);
  c.origin[0] = imageCircleRadius * normal.x;
  c.origin[1] = imageCircleRadius * normal.y;
  c.origin[2] = imageCircleRadius * normal.z;
  const V3 right = normalized(cross(normal, {0, 0, 1}));
  set_rotation(c, normal, cross(normal, {-right.x, -right.y, -right.z}));
  set_id(c, id);
  return c;
}

static Rig make_rig(const Flags& F) {
  Rig rig;
  const std::string mode = F.s("mode");
  const int fw = F.i("ftheta_width"), fh = F.i("ftheta_height"), fr = F.i("ftheta_image_circle_radius");
  const float ffov = (float)F.d("ftheta_image_circle_fov"), radius = (float)F.d("rig_radius");
  if (mode == "pinhole_ring") {  // makeHorizontalRingOfPinholeCameras, :374-387
    const int w = F.i("pinhole_width"), h = F.i("pinhole_height");
    const float aspect = (float)F.d("pinhole_aspect_ratio");
    const float tanHalfFov = std::tan(to_radians((float)F.d("pinhole_fov_horizontal")) / 2);
    ring_of_clones(rig, generic_camera(DERP_RECTILINEAR, w, h, (w / 2.0) / tanHalfFov, (h / 2.0) / (tanHalfFov / aspect)),
                   F.i("num_cams_in_ring"), radius);
  } else if (mode == "ftheta_ring") {  // makeHorizontalRingOfFThetaCameras + addTopCamera, :400-422
    ring_of_clones(rig, generic_ftheta(fw, fh, fr, ffov), F.i("num_cams_in_ring"), radius);
    derp_camera_desc top = generic_ftheta(fw, fh, fr, ffov);
    top.origin[2] = F.d("top_cam_vertical_offset");
    set_rotation(top, {0, 0, 1}, {1, 0, 0});
    set_id(top, rig.cameras.size());
    rig.cameras.push_back(top);
  } else if (mode == "dodecahedron" || mode == "icosahedron") {  // :451-491
    float vert[36];
    int32_t faces[60];
    derp_sim_icosahedron(vert, faces);
    auto vertex = [&](int i) { return V3{vert[3 * i], vert[3 * i + 1], vert[3 * i + 2]}; };
    if (mode == "dodecahedron") {  // one camera per icosahedron vertex
      for (int i = 0; i < 12; ++i) {
        rig.cameras.push_back(ftheta_on_sphere(vertex(i), fw, fh, fr, ffov, rig.cameras.size()));
      }
    } else {  // one per face, at the normalised sum of its vertices
      for (int i = 0; i < 20; ++i) {
        const V3 a = vertex(faces[3 * i]), b = vertex(faces[3 * i + 1]), c = vertex(faces[3 * i + 2]);
        const V3 mid = normalized({a.x + b.x + c.x, a.y + b.y + c.y, a.z + b.z + c.z});
        rig.cameras.push_back(ftheta_on_sphere(mid, fw, fh, fr, ffov, rig.cameras.size()));
      }
    }
  } else {  // rig_from_json
    rig.cameras = load_rig(F.s("rig_in"));
    const std::string text = read_file_or_empty(F.s("rig_in"));
    JsonParser jp(text);
    const Json root = jp.value();
    for (const Json& c : root.at("cameras").arr) {
      if (const Json* g = c.find("group")) {
        rig.groups[c.at("id").str] = g->str;
      }
    }
  }
  return rig;
}

struct Bgr8 {
  int w = 0, h = 0;
  std::vector<uint8_t> px;
};
// imreadExceptionOnFail(path, cv::IMREAD_COLOR): three 8-bit channels in BGR order; a 16-bit source keeps its high
// byte, grey is replicated, alpha is dropped
static Bgr8 read_color8(const fs::path& path) {
  CHECK_MSG(fs::is_regular_file(path), "failed to load image: " + path.string());
  const Raster p = read_raster(path);
  CHECK_MSG((p.bitdepth == 8 || p.bitdepth == 16) && p.w > 0 && p.h > 0, "failed to load image: " + path.string());
  Bgr8 out;
  out.w = p.w;
  out.h = p.h;
  out.px.resize((size_t)p.w * p.h * 3);
  const int shift = p.bitdepth == 16 ? 8 : 0;
  for (size_t i = 0; i < (size_t)p.w * p.h; ++i) {
    for (int c = 0; c < 3; ++c) {
      const size_t at = p.channels >= 3 ? (size_t)p.channels * i + (2 - c) : (size_t)p.channels * i;
      out.px[3 * i + c] = (uint8_t)(p.px[at] >> shift);
    }
  }
  return out;
}

// cv::imwrite of a float matrix as an 8-bit PNG: convertTo(CV_8U), saturating, ties to even; BGR -> the file's RGB
static void write_png8(const fs::path& path, const float* m, int w, int h, int channels) {
  std::vector<uint16_t> px((size_t)w * h * channels);
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    for (int c = 0; c < channels; ++c) {
      px[channels * i + (channels == 3 ? 2 - c : c)] = (uint16_t)float_to_uint_sat(m[channels * i + c], 1.0f, 255u);
    }
  }
  write_png(path, px.data(), w, h, channels, 8);
}

int main(int argc, char** argv) {
  Flags F;
  F.usage_msg = kUsage;
  F.i32("anti_alias_supersample", 1, "1 = no supersampling, 2 or higher = anti-alias supersampling");
  F.dbl("ceiling_depth", 0, "depth of ceiling texture (m)");
  F.str("ceiling_path", "", "path to image to use for ceiling");
  F.dbl("ceiling_position", 0, "how far up the ceiling is (m)");
  F.dbl("ceiling_width", 0, "width of ceiling texture (m)");
  F.str("dest_cam_images", "", "path to directory to write camera images for multi-camera rigs");
  F.str("dest_left", "", "path to left-eye image");
  F.str("dest_mono", "", "path to mono image");
  F.str("dest_mono_depth", "", "path to mono 1/depthmap (intensity = 1 / depth in meters)");
  F.str("dest_right", "", "path to right-eye image");
  F.str("dest_stereo", "", "path to right-eye image");
  F.i32("eqr_height", 1540, "height of equirect output");
  F.i32("eqr_width", 3080, "width of equirect output");
  F.i32("ftheta_height", 400, "height of ftheta camera output");
  F.dbl("ftheta_image_circle_fov", 166.667, "ftheta FOV, i.e. number of degrees spanned at the image circle");
  F.i32("ftheta_image_circle_radius", 250, "image circle radius corresponding to specified ftheta FOV");
  F.i32("ftheta_width", 300, "width of ftheta camera output");
  F.dbl("ground_plane_dist_m", 1.70, "for 'ground_plane' scene, distance from camera to ground");
  F.dbl("interpupillary_radius", 3.2, "half distance between eyes");
  F.boolean("marble", false, "if true, adds a marble (perlin noise) texture to the objects in the scene");
  F.dbl("marble_scale", 0.1, "scale applied to marble texture");
  F.dbl("max_icosahedron_dist", 250, "maximum distance from origin that a randomly generated icosahedron can spawn");
  F.dbl("max_icosahedron_radius", 50, "max radius of a randomly generated icosahedron");
  F.dbl("min_icosahedron_dist", 100,
        "minimum distance from a center of camera to the closest point on a randomly generated icosahedron");
  F.dbl("min_icosahedron_radius", 20, "min radius of a randomly generated icosahedron");
  F.str("mode", "", "mono_eqr,stereo_eqr,pinhole_ring,ftheta_ring,dodecahedron,icosahedron,rig_from_json (required)");
  F.dbl("noise_amplitude", 0.0,
        "amount of noise to be added to pixels (to simulate real camera noise). pixel intensities are scaled in 0...255");
  F.i32("num_cams_in_ring", 14, "number of cameras in simulated rings of cameras");
  F.i32("num_random_icosahedrons", 250, "number of icosahedrons to generate");
  F.dbl("pinhole_aspect_ratio", 1.0, "aspect ratio of pinhole lens = horizontal fov / vertical fov");
  F.dbl("pinhole_fov_horizontal", 77.7, "horizontal FOV of pinhole lens (degrees)");
  F.i32("pinhole_height", 512, "height of pinhole camera output");
  F.i32("pinhole_width", 512, "width of pinhole camera output");
  F.boolean("red_triangle", false, "add a red triangle at (0,0)");
  F.str("rig_in", "", "path to read json rig file if mode = rig_from_json");
  F.str("rig_out", "", "path to write json description of multi-camera rig");
  F.dbl("rig_radius", 0.218, "radius of the rig/sphere of cameras (m). distance from center to lens exit pupil.");
  F.str("scene", "icosahedron", "scene to draw: 'icosahedron', 'cube', 'ground_plane'");
  F.str("skybox_path", "res/skybox.jpg", "path to image to use as background/skybox");
  F.dbl("top_cam_vertical_offset", 13.0, "distance from center plane to top camera");
  F.i32("device", 0, "HIP device index [extension]");
  F.i32("threads", -1, "number of I/O threads (-1 = auto, 0 = none) [extension]");
  F.parse(argc, argv);

  // ---- every refusal, before any image is read or a device is opened
  const std::string mode = F.s("mode"), sceneName = F.s("scene");
  CHECK_MSG(mode != "", "mode");
  CHECK_MSG(F.s("skybox_path") != "", "skybox_path");
  const bool eqr = mode == "mono_eqr" || mode == "stereo_eqr";
  if (!eqr && mode != "pinhole_ring" && mode != "ftheta_ring" && mode != "dodecahedron" && mode != "icosahedron" &&
      mode != "rig_from_json") {
    LOG_FATAL("unexpected mode: " + mode);
  }
  if (sceneName != "icosahedron" && sceneName != "cube" && sceneName != "ground_plane") {
    LOG_FATAL("unexpected scene: " + sceneName);
  }
  if (mode == "mono_eqr") {
    CHECK_MSG(F.s("dest_mono") != "", "dest_mono");
    CHECK_MSG(F.s("dest_mono_depth") != "", "dest_mono_depth");
  } else if (mode == "stereo_eqr") {
    CHECK_MSG(F.s("dest_left") != "", "dest_left");
    CHECK_MSG(F.s("dest_right") != "", "dest_right");
    CHECK_MSG(F.s("dest_stereo") != "", "dest_stereo");
  } else {
    if (mode == "rig_from_json") {
      CHECK_MSG(F.s("rig_in") != "", "rig_in");
    }
    // (the reference runs to the end and writes nothing here)
    CHECK_MSG(F.s("rig_out") != "" || F.s("dest_cam_images") != "", "rig_out or dest_cam_images: nothing to write");
  }
  const int aas = F.i("anti_alias_supersample");
  CHECK_MSG(aas >= 1 && aas <= 64, "anti_alias_supersample must be in 1..64");
  if (eqr) {
    CHECK_MSG(F.i("eqr_width") > 0 && F.i("eqr_height") > 0, "eqr_width and eqr_height must be positive");
  }
  CHECK_MSG(F.i("num_random_icosahedrons") >= 0 && F.i("num_cams_in_ring") >= 1, "bad icosahedron or camera count");

  const bool render = eqr || F.s("dest_cam_images") != "";
  const Bgr8 skybox = read_color8(F.s("skybox_path"));  // (read in every mode, as the reference does: :666)
  Bgr8 ceiling;
  if (F.s("ceiling_path") != "") {
    ceiling = read_color8(F.s("ceiling_path"));
  }
  Rig rig;
  if (!eqr) {
    rig = make_rig(F);
    CHECK_MSG(!rig.cameras.empty(), "the rig has no cameras");
    for (const derp_camera_desc& c : rig.cameras) {
      CHECK_MSG(c.resolution[0] >= 1 && c.resolution[1] >= 1, std::string("bad resolution of camera ") + c.id);
    }
  }

  // ---- scene, then its sphere tree: the order of the rand() draws (RigSimulator.cpp:668-696)
  derp_sim_scene* scene = derp_sim_scene_create();
  if (sceneName == "icosahedron") {
    derp_sim_scene_icosahedrons(scene, F.i("num_random_icosahedrons"), F.d("min_icosahedron_dist"), F.d("max_icosahedron_dist"),
                                F.d("min_icosahedron_radius"), F.d("max_icosahedron_radius"), F.b("red_triangle"));
  } else if (sceneName == "cube") {
    derp_sim_scene_cubes(scene);
  } else {
    derp_sim_scene_ground_plane(scene, F.d("ground_plane_dist_m"));
  }
  LOG_INFO("building BVH");
  derp_sim_bvh_build(scene, 20, 5, 50);

  if (!eqr && F.s("rig_out") != "") {
    save_rig(F.s("rig_out"), rig.cameras, rig.groups, 10);
  }
  if (!render) {
    derp_sim_scene_destroy(scene);
    return EXIT_SUCCESS;
  }

  int nt = 0, nn = 0, nl = 0;
  derp_sim_scene_counts(scene, &nt, &nn, &nl);
  std::vector<derp_sim_triangle> tris((size_t)nt);
  std::vector<derp_sim_node> nodes((size_t)nn);
  std::vector<int32_t> leaf((size_t)nl);
  derp_sim_scene_get(scene, tris.data(), nodes.data(), leaf.data());
  derp_sim_scene_destroy(scene);

  derp_sim* sim = nullptr;
  if (derp_sim_create(&sim, F.i("device")) != 0) {
    LOG_FATAL(std::string("derp_sim_create failed: ") + derp_last_error(nullptr));
  }
  derp_sim_params params;
  memset(&params, 0, sizeof params);
  params.ceiling_position = F.d("ceiling_position");
  params.ceiling_width = F.d("ceiling_width");
  params.ceiling_depth = F.d("ceiling_depth");
  params.marble = F.b("marble");
  params.marble_scale = F.d("marble_scale");
  DERP_OK(nullptr, derp_sim_upload(sim, tris.data(), nt, nodes.data(), nn, leaf.data(), nl, skybox.px.data(), skybox.w, skybox.h,
                                   ceiling.px.empty() ? nullptr : ceiling.px.data(), ceiling.w, ceiling.h, &params));
  // a camera's planes, from its render until its files are written. Declared before the pool, so they outlive every
  // write job: the pool's destructor joins its threads first.
  struct Out {
    std::vector<float> bgr, depth;
  };
  std::vector<std::unique_ptr<Out>> outs;
  {
    IoPool pool(F.i("threads"));
    IoBatch writes;
    if (eqr) {
      const int w = F.i("eqr_width"), h = F.i("eqr_height");
      const size_t n = (size_t)w * h;
      std::vector<float> a(3 * n), b(3 * n), inv(n);
      Timer timer;
      DERP_OK(nullptr, derp_sim_render_equirect(sim, w, h, aas, mode == "stereo_eqr", F.d("interpupillary_radius"), a.data(),
                                                b.data(), inv.data()));
      LOG_INFO(fmt("Runtime = %.3f s (%s)", timer.s(), mode.c_str()));
      if (mode == "mono_eqr") {
        write_png8(F.s("dest_mono"), a.data(), w, h, 3);
        for (float& v : inv) {  // monoEquirectInvDepth * 255.0 (:707): a float matrix scaled, then imwrite's conversion
          v = v * 255.0f;
        }
        write_png8(F.s("dest_mono_depth"), inv.data(), w, h, 1);
      } else {
        write_png8(F.s("dest_left"), a.data(), w, h, 3);
        write_png8(F.s("dest_right"), b.data(), w, h, 3);
        a.insert(a.end(), b.begin(), b.end());  // vconcat: left over right
        write_png8(F.s("dest_stereo"), a.data(), w, 2 * h, 3);
      }
    } else {
      const fs::path dest = F.s("dest_cam_images");
      fs::create_directories(dest);
      for (const derp_camera_desc& cam : rig.cameras) {
        const int w = (int)cam.resolution[0], h = (int)cam.resolution[1];
        LOG_INFO(fmt("------ rendering camera %s", cam.id));
        outs.emplace_back(new Out);
        Out* o = outs.back().get();
        o->bgr.resize((size_t)w * h * 3);
        o->depth.resize((size_t)w * h);
        Timer timer;
        DERP_OK(nullptr, derp_sim_render_camera(sim, &cam, aas, o->bgr.data(), o->depth.data()));
        derp_sim_noise(o->bgr.data(), w, h, F.d("noise_amplitude"));
        LOG_INFO(fmt("Runtime = %.3f s (camera %s)", timer.s(), cam.id));
        const std::string id = cam.id;
        writes.add(pool, [o, dest, id, w, h] {  // renderCamerasThreaded, :652-656
          write_png8(dest / (id + ".png"), o->bgr.data(), w, h, 3);
          write_png8(dest / (id + "_depth.png"), o->depth.data(), w, h, 1);
          write_pfm(dest / (id + "_depth.pfm"), o->depth.data(), w, h);
          std::vector<float>().swap(o->bgr);
          std::vector<float>().swap(o->depth);
        }, 1);
        writes.raise_if_failed();
      }
      writes.wait();
    }
  }
  derp_sim_destroy(sim);
  return EXIT_SUCCESS;
}
