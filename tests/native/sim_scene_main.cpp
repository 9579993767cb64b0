// Stand-alone harness of csrc/derp_sim_scene.cpp for the sanitizer run of tests/test_rig_simulator.py: after srand(1)
// it builds one of the test scenes and its sphere tree, traces a fan of rays on the host, and writes
// [nt, nn, nl][triangles][nodes][leaf indices][n x bgrd] to a file the test compares with the library's arrays.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/derp_hip.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: sim_scene_main <empty|triangle|four|cubes|icosa12|ground> <out.bin>\n");
    return 2;
  }
  const std::string name = argv[1];
  srand(1);
  derp_sim_scene* s = derp_sim_scene_create();
  int rc = 0;
  if (name == "empty") {
    rc = derp_sim_scene_icosahedrons(s, 0, 100, 250, 20, 50, 0);
  } else if (name == "triangle") {
    rc = derp_sim_scene_icosahedrons(s, 0, 100, 250, 20, 50, 1);
  } else if (name == "four") {
    const float t[4][12] = {{-2, -2, -10, 2, -2, -10, 0, 2, -10, 1, 0, 0},
                            {-2, -2, -12, 2, -2, -12, 0, 2, -12, 0, 1, 0},
                            {0, -1, -8, 1, 1, -8, -1, 1, -8, 0, 0, 1},
                            {3, 0, -9, 4, 0, -9, 3, 1, -11, 1, 1, 0}};
    for (const auto& q : t) {
      rc |= derp_sim_scene_add_triangle(s, q, q + 3, q + 6, q + 9);
    }
  } else if (name == "cubes") {
    rc = derp_sim_scene_cubes(s);
  } else if (name == "icosa12") {
    rc = derp_sim_scene_icosahedrons(s, 12, 100, 250, 20, 50, 0);
  } else if (name == "ground") {
    rc = derp_sim_scene_ground_plane(s, 1.70);
  } else {
    return 2;
  }
  rc |= derp_sim_bvh_build(s, 20, 5, 50);
  int n[3] = {0, 0, 0};
  rc |= derp_sim_scene_counts(s, &n[0], &n[1], &n[2]);
  std::vector<derp_sim_triangle> tris((size_t)n[0]);
  std::vector<derp_sim_node> nodes((size_t)n[1]);
  std::vector<int32_t> leaf((size_t)n[2]);
  rc |= derp_sim_scene_get(s, tris.data(), nodes.data(), leaf.data());
  // a fan of rays from the origin over the whole sphere
  std::vector<float> rays, out;
  for (int a = 0; a < 12; ++a) {
    for (int b = 0; b < 24; ++b) {
      const float phi = 3.14159265f * (a + 0.5f) / 12, theta = 6.2831853f * b / 24;
      const float r[6] = {0.1f, 0.2f, 0.3f, sinf(phi) * cosf(theta), sinf(phi) * sinf(theta), cosf(phi)};
      rays.insert(rays.end(), r, r + 6);
    }
  }
  out.resize(rays.size() / 6 * 4);
  rc |= derp_sim_trace_host(s, rays.data(), rays.size() / 6, out.data());
  derp_sim_scene_destroy(s);
  if (rc) {
    fprintf(stderr, "a scene call failed\n");
    return 1;
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f) {
    return 1;
  }
  fwrite(n, sizeof n, 1, f);
  if (!tris.empty()) {  // (the empty scene's vectors hold no storage)
    fwrite(tris.data(), sizeof(derp_sim_triangle), tris.size(), f);
  }
  fwrite(nodes.data(), sizeof(derp_sim_node), nodes.size(), f);
  if (!leaf.empty()) {
    fwrite(leaf.data(), sizeof(int32_t), leaf.size(), f);
  }
  fwrite(out.data(), sizeof(float), out.size(), f);
  fclose(f);
  printf("%d %d %d\n", n[0], n[1], n[2]);
  return 0;
}
