// Test harness (CPU only) for csrc/derp_simplify.cpp, the host mesh simplifier, built with the sanitizers. usage:
//   mesh_simplify_main run <in> <out> <budget> <strictness> <remove_boundary_edges> <equi_error>
//     <in>:  u64 vertices, u64 faces, f64 [vertices][3], i32 [faces][3]
//     <out>: u64 vertices, u64 faces, u64 passes, u64 exit reason, f64 [vertices][3], i32 [faces][3]
//   mesh_simplify_main synth <n> <budget>   an n x n height field (two triangles per quad), simplified; prints counts
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/derp_hip.h"

static int simplify(const std::vector<double>& V, const std::vector<int32_t>& F, int budget, float strictness, int rbe, int equi,
                    std::vector<double>& oV, std::vector<int32_t>& oF, int stats[2]) {
  oV.resize(V.size());
  oF.resize(F.size());
  size_t nv = 0, nf = 0;
  if (derp_mesh_simplify_host(V.data(), V.size() / 3, F.data(), F.size() / 3, nullptr, nullptr, nullptr, budget, strictness, rbe,
                              equi, oV.data(), oF.data(), &nv, &nf, stats)) {
    return 1;
  }
  oV.resize(nv * 3);
  oF.resize(nf * 3);
  return 0;
}

int main(int argc, char** argv) {
  const std::string kind = argc > 1 ? argv[1] : "";
  std::vector<double> V, oV;
  std::vector<int32_t> F, oF;
  int stats[2] = {0, 0};
  if (kind == "run" && argc == 8) {
    FILE* in = fopen(argv[2], "rb");
    uint64_t n[2];
    if (!in || fread(n, 8, 2, in) != 2) {
      return 2;
    }
    V.resize(n[0] * 3);
    F.resize(n[1] * 3);
    if (fread(V.data(), 8, V.size(), in) != V.size() || fread(F.data(), 4, F.size(), in) != F.size()) {
      return 2;
    }
    fclose(in);
    if (simplify(V, F, atoi(argv[4]), (float)atof(argv[5]), atoi(argv[6]), atoi(argv[7]), oV, oF, stats)) {
      fprintf(stderr, "derp_mesh_simplify_host: bad arguments\n");
      return 1;
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out) {
      return 2;
    }
    const uint64_t head[4] = {oV.size() / 3, oF.size() / 3, (uint64_t)stats[0], (uint64_t)stats[1]};
    fwrite(head, 8, 4, out);
    fwrite(oV.data(), 8, oV.size(), out);
    fwrite(oF.data(), 4, oF.size(), out);
    return fclose(out) == 0 ? 0 : 2;
  }
  if (kind == "synth" && argc == 4) {
    const int n = atoi(argv[2]);
    for (int y = 0; y < n; ++y) {
      for (int x = 0; x < n; ++x) {
        V.push_back(x + 0.5);
        V.push_back(y + 0.5);
        V.push_back(20.0 + 3.0 * std::sin(x * 0.05) * std::cos(y * 0.07) + 0.01 * ((x * 7 + y * 13) % 11));
      }
    }
    for (int y = 0; y + 1 < n; ++y) {
      for (int x = 0; x + 1 < n; ++x) {
        const int b = y * n + x;
        const int quad[6] = {b + n, b + 1, b, b + 1, b + n, b + n + 1};
        F.insert(F.end(), quad, quad + 6);
      }
    }
    if (simplify(V, F, atoi(argv[3]), 0.2f, 0, 1, oV, oF, stats)) {
      return 1;
    }
    printf("synth %d: %zu -> %zu faces, %zu -> %zu vertices, %d passes, exit %d\n", n, F.size() / 3, oF.size() / 3, V.size() / 3,
           oV.size() / 3, stats[0], stats[1]);
    return 0;
  }
  return 2;
}
