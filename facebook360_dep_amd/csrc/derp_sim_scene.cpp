// Host-side entry points of the C-ABI (include/derp_hip.h, "RigSimulator"): the procedural scenes of
// source/rig/RigSimulator.cpp (:144-167, 264-358), the randomized sphere tree of
// source/render/BoundingVolumeHierarchy.h:32-114, its pre-order flat form, the image noise (:494-508) and a
// single-thread tracer. No device code and no HIP call: a host-only translation unit of libderp_hip.so, like
// derp_simplify.cpp. Scene and tree draw from the C library's rand() in the reference's call order (scene first, then
// the tree, children depth-first), so one process start gives the reference's scene on the same C library.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "derp_sim_math.h"

using namespace derp_sim_math;

struct derp_sim_scene {
  std::vector<derp_sim_triangle> triangles;
  std::vector<derp_sim_node> nodes;
  std::vector<int32_t> leaf;
};

namespace {

float randf0to1() {  // MathUtil.h:23-25
  return float(rand()) / float(RAND_MAX);
}

void put(float* dst, const V3f& v) {
  dst[0] = v.x;
  dst[1] = v.y;
  dst[2] = v.z;
}

// Triangle::Triangle, RaytracingPrimitives.h:45-49
derp_sim_triangle make_triangle(const V3f& v0, const V3f& v1, const V3f& v2, const V3f& color) {
  derp_sim_triangle t;
  const V3f e1 = sub(v1, v0), e2 = sub(v2, v0);
  V3f n = cross(e1, e2);
  n = div_double(n, norm(n));
  put(t.v0, v0);
  put(t.v1, v1);
  put(t.v2, v2);
  put(t.e1, e1);
  put(t.e2, e2);
  put(t.normal, n);
  put(t.color, color);
  return t;
}

// The regular icosahedron on the unit sphere from the golden ratio phi: vertices (+-1, 0, +-phi) / sqrt(1 + phi^2) and
// their cyclic shifts, in the vertex and face order of the OpenGL Programming Guide's subdivision example; the scene
// uses each face with its winding reversed (RigSimulator.cpp:139-142 lists them that way).
const int kIcosaFaces[20][3] = {{0, 4, 1}, {0, 9, 4},  {9, 5, 4},  {4, 5, 8},  {4, 8, 1},  {8, 10, 1}, {8, 3, 10},
                                {5, 3, 8}, {5, 2, 3},  {2, 7, 3},  {7, 10, 3}, {7, 6, 10}, {7, 11, 6}, {11, 0, 6},
                                {0, 1, 6}, {6, 1, 10}, {9, 0, 11}, {9, 11, 2}, {9, 2, 5},  {7, 2, 11}};
void icosa_vertices(float v[12][3]) {
  const double phi = (1.0 + std::sqrt(5.0)) / 2.0, len = std::sqrt(1.0 + phi * phi);
  const float X = (float)(1.0 / len), Z = (float)(phi / len);
  const float t[12][3] = {{-X, 0, Z}, {X, 0, Z},   {-X, 0, -Z}, {X, 0, -Z}, {0, Z, X},  {0, Z, -X},
                          {0, -Z, X}, {0, -Z, -X}, {Z, X, 0},   {-Z, X, 0}, {Z, -X, 0}, {-Z, -X, 0}};
  std::memcpy(v, t, sizeof t);
}

// makeIcosahedron, RigSimulator.cpp:145-167
void make_icosahedron(std::vector<derp_sim_triangle>& out, const V3f& center, float radius) {
  float vert[12][3];
  icosa_vertices(vert);
  V3f color = {0, 1, 0};
  if (!(center.z > 0)) {
    // (the three draws are the arguments of one constructor call, whose evaluation order C++ leaves to the compiler;
    // source order is taken here and wherever a call draws more than once: DESIGN section 8.5)
    const float b = randf0to1(), g = randf0to1(), r = randf0to1();
    color = {b, g, r};
  }
  for (int i = 0; i < 20; ++i) {
    const V3f v1 = f3(vert[kIcosaFaces[i][2]]), v2 = f3(vert[kIcosaFaces[i][1]]), v3 = f3(vert[kIcosaFaces[i][0]]);
    out.push_back(make_triangle(add(scale(v1, radius), center), add(scale(v2, radius), center),
                                add(scale(v3, radius), center), color));
  }
}

struct Builder {
  int threshold, splitK, maxDepth;
  const std::vector<derp_sim_triangle>* all;
  std::vector<derp_sim_node>* nodes;
  std::vector<int32_t>* leaf;

  // makeBVH, BoundingVolumeHierarchy.h:32-114, over triangle indices; appends the subtree in pre-order
  void build(const std::vector<int32_t>& tris, int depth) {
    const std::vector<derp_sim_triangle>& T = *all;
    V3f cm = {0.0f, 0.0f, 0.0f};
    for (int32_t i : tris) {
      cm = add(cm, add(add(f3(T[i].v0), f3(T[i].v1)), f3(T[i].v2)));
    }
    cm = div_float(cm, float(tris.size() * 3));  // 0 triangles: 0 * inf = NaN, a sphere no ray hits
    float radius = 0.0f;
    for (int32_t i : tris) {
      radius = std::max(radius, float(norm(sub(cm, f3(T[i].v0)))));
      radius = std::max(radius, float(norm(sub(cm, f3(T[i].v1)))));
      radius = std::max(radius, float(norm(sub(cm, f3(T[i].v2)))));
    }
    const size_t self = nodes->size();
    derp_sim_node nd;
    put(nd.center, cm);
    nd.radius = radius;
    nd.skip = 0;
    nd.first = 0;
    nd.count = -1;
    nd.n_children = 0;
    nodes->push_back(nd);
    const int n = (int)tris.size();
    if (depth >= maxDepth || n < splitK || n < threshold) {
      (*nodes)[self].first = (int32_t)leaf->size();
      (*nodes)[self].count = n;
      leaf->insert(leaf->end(), tris.begin(), tris.end());
      (*nodes)[self].skip = (int32_t)nodes->size();
      return;
    }
    std::vector<int> centers;
    std::set<int> seen;
    while ((int)centers.size() < splitK) {
      const int r = (int)(rand() % tris.size());
      if (seen.count(r) == 0) {
        centers.push_back(r);
        seen.insert(r);
      }
    }
    std::vector<std::vector<int32_t>> cluster((size_t)splitK);
    for (int i = 0; i < n; ++i) {
      float minDist = FLT_MAX;
      int pick = 0;  // (the reference's vector<int> starts at 0: a triangle no centre is nearer than FLT_MAX to)
      for (int j = 0; j < splitK; ++j) {
        const V3f diff = sub(f3(T[tris[i]].v0), f3(T[tris[centers[j]]].v0));
        const float dist2 = diff.x * diff.x + diff.y * diff.y + diff.z * diff.z;
        if (dist2 < minDist) {
          minDist = dist2;
          pick = j;
        }
      }
      cluster[(size_t)pick].push_back(tris[i]);
    }
    (*nodes)[self].n_children = splitK;
    for (int j = 0; j < splitK; ++j) {
      build(cluster[(size_t)j], depth + 1);
    }
    (*nodes)[self].skip = (int32_t)nodes->size();
  }
};

const uint8_t kPerlinPermutation[256] = {
    151, 160, 137, 91,  90,  15,  131, 13,  201, 95,  96,  53,  194, 233, 7,   225, 140, 36,  103, 30,  69,  142,
    8,   99,  37,  240, 21,  10,  23,  190, 6,   148, 247, 120, 234, 75,  0,   26,  197, 62,  94,  252, 219, 203,
    117, 35,  11,  32,  57,  177, 33,  88,  237, 149, 56,  87,  174, 20,  125, 136, 171, 168, 68,  175, 74,  165,
    71,  134, 139, 48,  27,  166, 77,  146, 158, 231, 83,  111, 229, 122, 60,  211, 133, 230, 220, 105, 92,  41,
    55,  46,  245, 40,  244, 102, 143, 54,  65,  25,  63,  161, 1,   216, 80,  73,  209, 76,  132, 187, 208, 89,
    18,  169, 200, 196, 135, 130, 116, 188, 159, 86,  164, 100, 109, 198, 173, 186, 3,   64,  52,  217, 226, 250,
    124, 123, 5,   202, 38,  147, 118, 126, 255, 82,  85,  212, 207, 206, 59,  227, 47,  16,  58,  17,  182, 189,
    28,  42,  223, 183, 170, 213, 119, 248, 152, 2,   44,  154, 163, 70,  221, 153, 101, 155, 167, 43,  172, 9,
    129, 22,  39,  253, 19,  98,  108, 110, 79,  113, 224, 232, 178, 185, 112, 104, 218, 246, 97,  228, 251, 34,
    242, 193, 238, 210, 144, 12,  191, 179, 162, 241, 81,  51,  145, 235, 249, 14,  239, 107, 49,  192, 214, 31,
    181, 199, 106, 157, 184, 84,  204, 176, 115, 121, 50,  45,  127, 4,   150, 254, 138, 236, 205, 93,  222, 114,
    67,  29,  24,  72,  243, 141, 128, 195, 78,  66,  215, 61,  156, 180};

}  // namespace

extern "C" {

// Ken Perlin's reference permutation ("Improved Noise", 2002), twice over as his p[512]
void derp_sim_perlin_table(uint8_t* p512) {
  for (int i = 0; i < 512; ++i) {
    p512[i] = kPerlinPermutation[i & 255];
  }
}

// the unit icosahedron of the scenes and of the dodecahedron / icosahedron rigs: 12 vertices, 20 faces in the scene's
// winding
void derp_sim_icosahedron(float* vertices36, int32_t* faces60) {
  float vert[12][3];
  icosa_vertices(vert);
  if (vertices36) {
    std::memcpy(vertices36, vert, sizeof vert);
  }
  if (faces60) {
    for (int i = 0; i < 20; ++i) {
      for (int k = 0; k < 3; ++k) {
        faces60[3 * i + k] = kIcosaFaces[i][2 - k];
      }
    }
  }
}

derp_sim_scene* derp_sim_scene_create(void) {
  return new derp_sim_scene;
}

void derp_sim_scene_destroy(derp_sim_scene* s) {
  delete s;
}

int derp_sim_scene_icosahedrons(derp_sim_scene* s, int count, double min_dist, double max_dist, double min_radius,
                                double max_radius, int red_triangle) {
  if (!s || count < 0) {
    return 1;
  }
  for (int i = 0; i < count; ++i) {  // makeIcosahedronScene, RigSimulator.cpp:264-278
    const float minAllowedCenterDist = (float)(min_dist + max_radius);
    V3f center;
    do {
      // float * (float - double) * double: all in double, narrowed once; x, y, z draw in source order
      const float x = (float)(2.0 * ((double)randf0to1() - 0.5) * max_dist);
      const float y = (float)(2.0 * ((double)randf0to1() - 0.5) * max_dist);
      const float z = (float)(2.0 * ((double)randf0to1() - 0.5) * max_dist);
      center = {x, y, z};
    } while (norm(center) < (double)minAllowedCenterDist);
    const float radiusRange = (float)(max_radius - min_radius);
    const float radius = (float)(min_radius + (double)(randf0to1() * radiusRange));
    make_icosahedron(s->triangles, center, radius);
  }
  if (red_triangle) {  // :280-288
    const float kDepth = (float)min_dist;
    const float kSide = 0.1f * kDepth;
    s->triangles.push_back(make_triangle({kDepth, 0, 0}, {kDepth, 0, kSide}, {kDepth, kSide, 0}, {0, 0, 1}));
  }
  return 0;
}

int derp_sim_scene_cubes(derp_sim_scene* s) {  // makeCubesScene, RigSimulator.cpp:291-343
  if (!s) {
    return 1;
  }
  // vertex i of the unit cube is the bits of i: (i >> 2 & 1, i >> 1 & 1, i & 1); two triangles per face
  static const int kFaces[12][3] = {{2, 0, 1}, {1, 3, 2}, {6, 2, 0}, {0, 4, 6}, {4, 0, 1}, {1, 5, 4},
                                    {3, 1, 5}, {5, 7, 3}, {7, 3, 2}, {2, 6, 7}, {5, 4, 6}, {6, 7, 5}};
  static const float kScales[2] = {2, 1};
  static const V3f kOffsets[2] = {{0, 0, -25}, {5, 2, -20}};
  static const V3f kColors[2][6] = {
      {{0, 0, 1}, {0, 1, 0}, {0, 1, 1}, {1, 0, 0}, {1, 0, 1}, {1, 1, 0}},
      {{0.5, 1, 0}, {1, 0, 0.5}, {1, 1, 1}, {0, 0.5, 1}, {0.5, 0.5, 1}, {0, 0, 0}}};
  const V3f shift = {-0.5, -0.5, -0.5};
  for (int t = 0; t < 12; ++t) {
    V3f v[3];
    for (int k = 0; k < 3; ++k) {
      const int i = kFaces[t][k];
      v[k] = {(float)(i >> 2 & 1), (float)(i >> 1 & 1), (float)(i & 1)};
    }
    for (int cube = 0; cube < 2; ++cube) {
      s->triangles.push_back(make_triangle(add(scale(add(v[0], shift), kScales[cube]), kOffsets[cube]),
                                           add(scale(add(v[1], shift), kScales[cube]), kOffsets[cube]),
                                           add(scale(add(v[2], shift), kScales[cube]), kOffsets[cube]),
                                           kColors[cube][t / 2]));
    }
  }
  return 0;
}

int derp_sim_scene_ground_plane(derp_sim_scene* s, double ground_plane_dist_m) {  // :345-358
  if (!s) {
    return 1;
  }
  const float kR = 100.0f, z = (float)-ground_plane_dist_m;
  const V3f v[4] = {{-kR, -kR, z}, {+kR, -kR, z}, {+kR, +kR, z}, {-kR, +kR, z}};
  const V3f red = {0, 0, 1};
  s->triangles.push_back(make_triangle(v[0], v[1], v[2], red));
  s->triangles.push_back(make_triangle(v[3], v[0], v[2], red));
  return 0;
}

int derp_sim_scene_add_triangle(derp_sim_scene* s, const float* v0, const float* v1, const float* v2,
                                const float* color_bgr) {
  if (!s || !v0 || !v1 || !v2 || !color_bgr) {
    return 1;
  }
  s->triangles.push_back(make_triangle(f3(v0), f3(v1), f3(v2), f3(color_bgr)));
  return 0;
}

int derp_sim_bvh_build(derp_sim_scene* s, int leaf_threshold, int split_k, int max_depth) {
  if (!s || split_k < 1) {
    return 1;
  }
  s->nodes.clear();
  s->leaf.clear();
  std::vector<int32_t> all(s->triangles.size());
  for (size_t i = 0; i < all.size(); ++i) {
    all[i] = (int32_t)i;
  }
  Builder b{leaf_threshold, split_k, max_depth, &s->triangles, &s->nodes, &s->leaf};
  b.build(all, 0);
  return 0;
}

int derp_sim_scene_counts(const derp_sim_scene* s, int* n_triangles, int* n_nodes, int* n_leaf_indices) {
  if (!s) {
    return 1;
  }
  if (n_triangles) {
    *n_triangles = (int)s->triangles.size();
  }
  if (n_nodes) {
    *n_nodes = (int)s->nodes.size();
  }
  if (n_leaf_indices) {
    *n_leaf_indices = (int)s->leaf.size();
  }
  return 0;
}

int derp_sim_scene_get(const derp_sim_scene* s, derp_sim_triangle* triangles, derp_sim_node* nodes, int32_t* leaf_indices) {
  if (!s) {
    return 1;
  }
  if (triangles && !s->triangles.empty()) {
    std::memcpy(triangles, s->triangles.data(), s->triangles.size() * sizeof(derp_sim_triangle));
  }
  if (nodes && !s->nodes.empty()) {
    std::memcpy(nodes, s->nodes.data(), s->nodes.size() * sizeof(derp_sim_node));
  }
  if (leaf_indices && !s->leaf.empty()) {
    std::memcpy(leaf_indices, s->leaf.data(), s->leaf.size() * sizeof(int32_t));
  }
  return 0;
}

int derp_sim_noise(float* bgr, int w, int h, double amplitude) {  // corruptImageWithNoise, :494-508
  if (!bgr || w < 0 || h < 0) {
    return 1;
  }
  const float a = (float)amplitude;
  if (a == 0.0f) {
    return 0;
  }
  for (size_t i = 0; i < (size_t)w * h * 3; ++i) {  // (channels 0, 1, 2 of a pixel draw in source order)
    const float v = bgr[i] + 2.0f * a * (randf0to1() - 0.5f);
    bgr[i] = v < 0 ? 0 : v > 255.0f ? 255.0f : v;
  }
  return 0;
}

int derp_sim_trace_host(const derp_sim_scene* s, const float* rays6, size_t n, float* out_bgrd) {
  if (!s || !rays6 || !out_bgrd || s->nodes.empty()) {
    return 1;
  }
  uint8_t perm[512];
  derp_sim_perlin_table(perm);
  for (size_t i = 0; i < n; ++i) {
    const V3f o = f3(rays6 + 6 * i), d = f3(rays6 + 6 * i + 3);
    float dist;
    const int hit = trace_tree(o, d, s->nodes.data(), (int)s->nodes.size(), s->leaf.data(), s->triangles.data(), dist);
    V3f c = {0, 0, 0};
    if (hit >= 0) {
      c = shade_hit(o, d, dist, s->triangles[(size_t)hit], false, 0.0, perm);
    }
    out_bgrd[4 * i] = c.x;
    out_bgrd[4 * i + 1] = c.y;
    out_bgrd[4 * i + 2] = c.z;
    out_bgrd[4 * i + 3] = dist;
  }
  return 0;
}

}  // extern "C"
