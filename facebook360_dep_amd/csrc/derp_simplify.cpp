// Host-side entry points of the C-ABI (include/derp_hip.h, "camera meshes"): the greedy edge-collapse loop of
// render::MeshSimplifier (source/render/MeshSimplifier.cpp:456-562) restated without Eigen, and its set-up
// (computeInitialQuadrics, :209-239) for callers without a device. No device code and no HIP call: a host-only
// translation unit of libderp_hip.so, like derp_images.cpp. The collapse order is sequential by construction (every
// collapse changes the costs the next one reads), so it stays on the host; the data-parallel set-up has device
// kernels (derp_mesh.h) that produce the same arrays bit for bit — both sides use derp_mesh_math.h.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/derp_hip.h"
#include "derp_mesh_math.h"

using namespace derp_mesh;

namespace {

struct Face {
  int v[3];
  V3 normal;
  double cost[3];
  bool deleted = false, touched = false;
};

struct Simplifier {
  std::vector<V3> coord;
  std::vector<double> vq;  // [nv][kQuadric]
  std::vector<char> boundary;
  std::vector<std::vector<int>> facesOf;
  std::vector<Face> faces;
  bool equiError = true;

  double error(int i0, int i1, V3& target) const {
    return compute_error(&vq[(size_t)i0 * kQuadric], &vq[(size_t)i1 * kQuadric], coord[i0], coord[i1],
                         boundary[i0] && boundary[i1], equiError, target);
  }

  void removeDeletedFaces() {  // :242-251
    size_t idx = 0;
    for (Face& face : faces) {
      face.touched = false;
      if (!face.deleted) {
        faces[idx++] = face;
      }
    }
    faces.resize(idx);
  }

  void assignFaceVertexes() {  // :253-264
    for (auto& f : facesOf) {
      f.clear();
    }
    for (int i = 0; i < (int)faces.size(); ++i) {
      for (int j = 0; j < 3; ++j) {
        facesOf[faces[i].v[j]].push_back(i);
      }
    }
  }

  int commonFaces(int v0, int v1, std::vector<int>* out) const {  // :266-276
    int n = 0;
    for (int i1 : facesOf[v0]) {
      for (int i2 : facesOf[v1]) {
        if (i1 == i2) {
          ++n;
          if (out) {
            out->push_back(i1);
          }
        }
      }
    }
    return n;
  }

  // identifySubBoundaries (:280-319) over the one range a single thread gets
  void identifyBoundaries() {
    std::fill(boundary.begin(), boundary.end(), 0);
    std::vector<int> visited;
    for (int i = 0; i < (int)coord.size(); ++i) {
      if (boundary[i]) {
        continue;
      }
      if (facesOf[i].size() == 1) {
        boundary[i] = 1;
        continue;
      }
      bool isBorder = false;
      visited.clear();
      for (int faceIdx : facesOf[i]) {
        for (int j = 0; j < 3; ++j) {
          const int v = faces[faceIdx].v[j];
          if (v != i && std::find(visited.begin(), visited.end(), v) == visited.end()) {
            visited.push_back(v);
            if (facesOf[v].size() == 1 || commonFaces(i, v, nullptr) == 1) {
              boundary[v] = 1;
              isBorder = true;
            }
          }
        }
      }
      if (isBorder) {
        boundary[i] = 1;
      }
    }
  }

  double getThreshold(float strictness) const {  // :333-344
    std::vector<double> errors(faces.size() * 3);
    for (size_t i = 0; i < faces.size(); ++i) {
      for (int j = 0; j < 3; ++j) {
        errors[i * 3 + j] = faces[i].cost[j];
      }
    }
    // float x size_t: a float product; (float)(n - 1) rounds up past 2^24, where the reference reads past the end
    // (narrowed to 64 bits, not to the reference's int: 3 x 2^31 costs fit the vector and not an int)
    const size_t idxPerc = std::min((size_t)(strictness * (float)(errors.size() - 1)), errors.size() - 1);
    std::nth_element(errors.begin(), errors.begin() + idxPerc, errors.end());
    return errors[idxPerc];
  }

  bool haveNormalsFlipped(const V3& p, int v0, int v1) const {  // :348-382
    for (int fi : facesOf[v0]) {
      const Face& face = faces[fi];
      if (face.deleted) {
        continue;
      }
      int order = 0;
      for (int j = 0; j < 3; ++j) {
        if (face.v[j] == v0) {
          order = j;
          break;
        }
      }
      const int i0 = face.v[(order + 1) % 3], i1 = face.v[(order + 2) % 3];
      if (i0 == v1 || i1 == v1) {
        continue;
      }
      const V3 a = normalized(sub(coord[i0], p)), b = normalized(sub(coord[i1], p));
      const V3 normal = normalized(cross(a, b));
      if (dot(normal, face.normal) < 0) {
        return true;
      }
    }
    return false;
  }

  void updateCosts(int v0, int v1, const V3& target) {  // :384-420
    coord[v0] = target;
    for (int k = 0; k < kQuadric; ++k) {
      vq[(size_t)v0 * kQuadric + k] += vq[(size_t)v1 * kQuadric + k];
    }
    std::vector<int> all(facesOf[v0]);
    all.insert(all.end(), facesOf[v1].begin(), facesOf[v1].end());
    for (int fi : all) {
      Face& face = faces[fi];
      if (face.deleted) {
        continue;
      }
      for (int i = 0; i < 3; ++i) {
        if (face.v[i] == v0 || face.v[i] == v1) {
          face.v[i] = v0;
          face.touched = true;
          break;
        }
      }
      for (int i = 0; i < 3; ++i) {
        V3 p;
        face.cost[i] = error(face.v[i], face.v[(i + 1) % 3], p);
      }
    }
  }

  // simplify (:456-562) after computeInitialQuadrics; -> iterations run and how the loop ended
  void run(int numFacesOut, float strictness, bool removeBoundaryEdges, int stats[2]) {
    const int numFacesIn = (int)faces.size();
    int numFacesDeleted = 0, numFacesDeletedPrev = 0, countNumFacesSame = 0, iteration = 0;
    double threshold = 0;
    int reason = DERP_MESH_EXIT_BUDGET;
    std::vector<int> common;
    while ((int)faces.size() > numFacesOut) {
      removeDeletedFaces();
      if (faces.empty()) {  // the last collapse deleted what was left: getThreshold has no cost to index (the reference
        break;              // indexes an empty vector here)
      }
      assignFaceVertexes();
      if (iteration == 0) {
        identifyBoundaries();
      }
      if (iteration == 0 || numFacesDeletedPrev != numFacesDeleted) {
        threshold = getThreshold(strictness);
        countNumFacesSame = 0;
      } else {
        threshold *= 2 * ++countNumFacesSame;
        if (std::isinf(threshold)) {
          reason = DERP_MESH_EXIT_INFINITE_THRESHOLD;
          break;
        }
        // A zero or NaN threshold does not grow, and a pass that deleted nothing left the mesh as it was: the
        // reference would repeat that pass for ever. Leave instead.
        if (!(std::fabs(threshold) > 0)) {
          reason = DERP_MESH_EXIT_STUCK;
          break;
        }
      }
      numFacesDeletedPrev = numFacesDeleted;
      for (size_t f = 0; f < faces.size(); ++f) {
        Face& face = faces[f];
        if (!(face.deleted || face.touched)) {
          for (int i = 0; i < 3; ++i) {
            if (face.cost[i] > threshold) {
              continue;
            }
            const int v0 = face.v[i], v1 = face.v[(i + 1) % 3];
            if (boundary[v0] != boundary[v1]) {
              continue;
            }
            if (!removeBoundaryEdges && (boundary[v0] || boundary[v1])) {
              continue;
            }
            V3 target;
            error(v0, v1, target);
            if (haveNormalsFlipped(target, v0, v1) || haveNormalsFlipped(target, v1, v0)) {
              continue;
            }
            common.clear();
            commonFaces(v0, v1, &common);
            for (int fi : common) {
              faces[fi].deleted = true;
            }
            numFacesDeleted += (int)common.size();
            updateCosts(v0, v1, target);
            break;
          }
        } else {
          continue;  // (`continue` in the reference skips the budget check below as well)
        }
        if (numFacesIn - numFacesDeleted <= numFacesOut) {
          break;
        }
      }
      ++iteration;
    }
    stats[0] = iteration;
    stats[1] = reason;
  }

  // createFinalMesh (:423-454)
  void finish(double* outV, int32_t* outF, size_t* outNv, size_t* outNf) {
    removeDeletedFaces();
    std::vector<int> map(coord.size(), -1);
    for (const Face& face : faces) {
      for (int i = 0; i < 3; ++i) {
        map[face.v[i]] = 0;
      }
    }
    size_t n = 0;
    for (size_t i = 0; i < coord.size(); ++i) {
      if (map[i] == 0) {
        map[i] = (int)n;
        outV[3 * n] = coord[i].x;
        outV[3 * n + 1] = coord[i].y;
        outV[3 * n + 2] = coord[i].z;
        ++n;
      }
    }
    for (size_t f = 0; f < faces.size(); ++f) {
      for (int i = 0; i < 3; ++i) {
        outF[3 * f + i] = map[faces[f].v[i]];
      }
    }
    *outNv = n;
    *outNf = faces.size();
  }
};

bool faces_in_range(const int32_t* faces, size_t nf, size_t nv) {
  for (size_t i = 0; i < nf * 3; ++i) {
    if (faces[i] < 0 || (size_t)faces[i] >= nv) {
      return false;
    }
  }
  return true;
}

V3 vertex_at(const double* v, int i) {
  return {v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]};
}

}  // namespace

extern "C" int derp_mesh_setup_host(const double* vertices, size_t nv, const int32_t* faces, size_t nf, int equi_error,
                                    double* face_planes, double* edge_costs, double* vertex_quadrics) {
  if ((!vertices && nv) || (!faces && nf) || (!face_planes && nf) || (!edge_costs && nf) || (!vertex_quadrics && nv) ||
      nv > (size_t)INT32_MAX || nf > (size_t)INT32_MAX || !faces_in_range(faces, nf, nv)) {
    return 1;
  }
  for (size_t f = 0; f < nf; ++f) {  // computeSubQuadrics
    face_plane(vertex_at(vertices, faces[3 * f]), vertex_at(vertices, faces[3 * f + 1]), vertex_at(vertices, faces[3 * f + 2]),
               face_planes + 4 * f);
  }
  std::fill(vertex_quadrics, vertex_quadrics + nv * kQuadric, 0.0);
  for (size_t f = 0; f < nf; ++f) {  // "Accumulating quadrics...": in ascending face index
    for (int j = 0; j < 3; ++j) {
      add_plane_quadric(vertex_quadrics + (size_t)faces[3 * f + j] * kQuadric, face_planes + 4 * f);
    }
  }
  for (size_t f = 0; f < nf; ++f) {  // computeSubError: no vertex is a boundary vertex yet
    for (int j = 0; j < 3; ++j) {
      const int i0 = faces[3 * f + j], i1 = faces[3 * f + (j + 1) % 3];
      V3 p;
      edge_costs[3 * f + j] = compute_error(vertex_quadrics + (size_t)i0 * kQuadric, vertex_quadrics + (size_t)i1 * kQuadric,
                                            vertex_at(vertices, i0), vertex_at(vertices, i1), false, equi_error != 0, p);
    }
  }
  return 0;
}

extern "C" int derp_mesh_simplify_host(const double* vertices, size_t nv, const int32_t* faces, size_t nf,
                                       const double* face_planes, const double* edge_costs, const double* vertex_quadrics,
                                       int num_faces_out, float strictness, int remove_boundary_edges, int equi_error,
                                       double* out_vertices, int32_t* out_faces, size_t* out_nv, size_t* out_nf,
                                       int* stats) {
  if ((!vertices && nv) || (!faces && nf) || (!out_vertices && nv) || (!out_faces && nf) || !out_nv || !out_nf ||
      num_faces_out < 0 || nv > (size_t)INT32_MAX || nf > (size_t)INT32_MAX || !faces_in_range(faces, nf, nv)) {
    return 1;
  }
  if (!(0 <= strictness && strictness <= 1)) {  // (NaN too) getThreshold's index would leave its vector
    return 1;
  }
  const bool given = face_planes && edge_costs && vertex_quadrics;
  if (!given && (face_planes || edge_costs || vertex_quadrics)) {
    return 1;  // the set-up comes whole or not at all
  }
  std::vector<double> planes, costs;
  Simplifier s;
  s.equiError = equi_error != 0;
  s.vq.resize(nv * kQuadric);
  if (given) {
    std::copy(vertex_quadrics, vertex_quadrics + nv * kQuadric, s.vq.begin());
  } else {
    planes.resize(nf * 4);
    costs.resize(nf * 3);
    if (derp_mesh_setup_host(vertices, nv, faces, nf, equi_error, planes.data(), costs.data(), s.vq.data())) {
      return 1;
    }
    face_planes = planes.data();
    edge_costs = costs.data();
  }
  s.coord.resize(nv);
  for (size_t i = 0; i < nv; ++i) {
    s.coord[i] = vertex_at(vertices, (int)i);
  }
  s.boundary.assign(nv, 0);
  s.facesOf.resize(nv);
  s.faces.resize(nf);
  for (size_t f = 0; f < nf; ++f) {
    Face& face = s.faces[f];
    for (int j = 0; j < 3; ++j) {
      face.v[j] = faces[3 * f + j];
      face.cost[j] = edge_costs[3 * f + j];
    }
    face.normal = {face_planes[4 * f], face_planes[4 * f + 1], face_planes[4 * f + 2]};
  }
  int st[2] = {0, DERP_MESH_EXIT_BUDGET};
  s.run(num_faces_out, strictness, remove_boundary_edges != 0, st);
  s.finish(out_vertices, out_faces, out_nv, out_nf);
  if (stats) {
    stats[0] = st[0];
    stats[1] = st[1];
  }
  return 0;
}

// addTextureCoordinatesEquirect (MeshUtil.h:407-419): "texture goes +x, +z, -x, -z, +x from left to right (0 to 1) and
// -y to +y from top to bottom (0 to 1)"
extern "C" int derp_mesh_texcoords_equirect(const double* vertices, size_t nv, double* st) {
  if ((!vertices || !st) && nv) {
    return 1;
  }
  for (size_t v = 0; v < nv; ++v) {
    const double x = vertices[3 * v], y = vertices[3 * v + 1], z = vertices[3 * v + 2];
    const double xzNorm = std::sqrt(x * x + z * z);
    st[2 * v] = std::atan2(-z, -x) * 0.5 / M_PI + 0.5;
    st[2 * v + 1] = -std::atan2(-y, xzNorm) / M_PI + 0.5;
  }
  return 0;
}
