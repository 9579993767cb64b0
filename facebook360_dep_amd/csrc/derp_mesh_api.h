// ConvertToBinary's camera meshes and CreateObjFromDisparityEquirect's wrapped scene mesh, host side: build, quadric
// set-up, the drivers of the host simplifier (derp_simplify.cpp) and of the pass-parallel one. Kernels: derp_mesh.h.
// Included by derp_capi.hip after the depth core.
#pragma once

namespace {

// derp_mesh_*: one camera's mesh, or one equirect's (derp_mesh.h). The grid-sized buffers stay for the next mesh; the
// compacted mesh (V, F) and what the set-up gathers through (qmask, qoff, vorig) describe the mesh built last. An
// equirect mesh keeps the whole grid (no vorig) and ends in its seam faces, from index nfGrid on.
struct MeshState {
  DevBuf disparity, mask, tabs, vert, valid, qmask, used, blockFaces, blockVerts, offF, offV, totals, vmap, vorig, qoff, V, F;
  DevBuf norm;
  DevBuf planes, costs, vq;
  int W = 0, H = 0;
  size_t nv = 0, nf = 0, nfUnmasked = 0, nfGrid = 0;
  bool built = false, equirect = false;
  // derp_mesh_simplify's / derp_mesh_simplify_parallel's result (host): what the downloads return once one has run
  bool simplified = false;
  std::vector<double> sV;
  std::vector<int32_t> sF;
  // derp_mesh_simplify_parallel's state besides V, F, planes, costs and vq, which it works on in place
  DevBuf alive, boundary, vcount, vstart, vcursor, adj, keys, keysFeasible, keysSorted, vals, valsSorted, claim, wins, blockSum, blockOff,
      counters, sortTemp, outV, outF;
  std::vector<derp_mesh_pass> passes;  // of the last derp_mesh_simplify_parallel (derp_mesh_parallel_pass)
};

// resizeNN's source index of every destination index (cv::resize INTER_NEAREST): min(floor(x * (1 / fx)), ssize - 1),
// where fx is the scale the caller gave (cv::Size() + fx) or dsize / ssize (a given dsize)
void nearest_table(int ssize, int dsize, double fx, int* out) {
  const double ifx = 1. / fx;
  for (int x = 0; x < dsize; ++x) {
    out[x] = std::min((int)std::floor(x * ifx), ssize - 1);
  }
}
int need_mesh(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  if (!c->mesh || !c->mesh->built) {
    return fail(c, "derp_mesh_build has not been called");  // (nor derp_mesh_build_equirect)
  }
  return 0;
}
// computeInitialQuadrics of the built mesh into m.planes / m.costs / m.vq
int mesh_setup_dev(derp_ctx* c, int equi_error) {
  MeshState& m = *c->mesh;
  ALLOC(c, m.planes, std::max<size_t>(m.nf * 32, 8));
  ALLOC(c, m.costs, std::max<size_t>(m.nf * 24, 8));
  ALLOC(c, m.vq, std::max<size_t>(m.nv * derp_mesh::kQuadric * 8, 8));
  if (m.nf == 0 || m.nv == 0) {
    return 0;
  }
  hipLaunchKernelGGL(k_mesh_face_planes, dim3(blocks_of(m.nf, kMeshBlock)), dim3(kMeshBlock), 0, c->stream, m.V.as<double>(),
                     m.F.as<int32_t>(), m.nf, m.planes.as<double>());
  hipLaunchKernelGGL(k_mesh_vertex_quadrics, dim3(blocks_of(m.nv, kMeshBlock)), dim3(kMeshBlock), 0, c->stream,
                     m.qmask.as<uint8_t>(), m.qoff.as<uint32_t>(), m.equirect ? (const uint32_t*)nullptr : m.vorig.as<uint32_t>(),
                     m.W, m.H, m.nv, m.planes.as<double>(), m.equirect ? 1 : 0, m.nfGrid, m.vq.as<double>());
  hipLaunchKernelGGL(k_mesh_edge_costs, dim3(blocks_of(m.nf * 3, kMeshBlock)), dim3(kMeshBlock), 0, c->stream, m.V.as<double>(),
                     m.F.as<int32_t>(), m.nf, m.vq.as<double>(), equi_error, m.costs.as<double>());
  KCHECK(c);
  return 0;
}
// rocPRIM's stable radix sort of (cost key, face * 3 + edge): Onesweep with 256 threads x 8 items (its default for
// this pair of types spills to scratch memory), from 4096 items on, so that the tests' meshes take the path of
// full-size ones
using MeshSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 12>, rocprim::kernel_config<256, 8>, 8>, 4096>;

}  // namespace

int derp_mesh_build(derp_ctx* c, int cam, const float* disparity, int w, int h, const double* resolution, double depth_scale,
                    const uint8_t* mask, int mask_w, int mask_h, float tear_ratio) {
  if (!c || !disparity || w <= 0 || h <= 0 || (size_t)w * h >= kMaxPixels || !(depth_scale > 0) ||
      (mask && (mask_w <= 0 || mask_h <= 0 || (size_t)mask_w * mask_h >= kMaxPixels))) {
    return fail(c, "bad arguments (null pointer, image size or depth scale)");
  }
  TRY(check_camera(c, cam));
  // Camera::rescale(resolution) of the rig camera as the file holds it (resizeRig, ConvertToBinary.cpp:318-339), then
  // getScalarFocal (Camera.cpp:185-188)
  const derp_camera_desc& j = c->descDstH[cam];
  double resx = j.resolution[0], resy = j.resolution[1], fx = j.focal[0], fy = j.focal[1];
  if (resolution) {
    fx *= resolution[0] / resx;
    fy *= resolution[1] / resy;
    resx = resolution[0];
    resy = resolution[1];
  }
  if (fx != -fy) {
    return fail(c, "Check failed: focal.x() == -focal.y() (%.17g vs. %.17g) pixels are not square", fx, -fy);
  }
  // cv::resize(depth, depth, cv::Size(), s, s, INTER_NEAREST) when s < 1: dsize = saturate_cast<int>(ssize * s)
  const bool scaled = depth_scale < 1;
  const int W = scaled ? (int)std::nearbyint(w * depth_scale) : w, H = scaled ? (int)std::nearbyint(h * depth_scale) : h;
  if (W <= 0 || H <= 0) {
    return fail(c, "depth scale %g leaves no pixels of a %d x %d map", depth_scale, w, h);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the mesh built before this one may still be read
  if (!c->mesh) {
    c->mesh.reset(new MeshState);
  }
  MeshState& m = *c->mesh;
  m.built = m.simplified = m.equirect = false;
  m.W = W;
  m.H = H;
  std::vector<int> tabs(2 * (size_t)W + 2 * (size_t)H);
  int *xofs = tabs.data(), *yofs = xofs + W, *mxofs = yofs + H, *myofs = mxofs + W;
  nearest_table(w, W, scaled ? depth_scale : 1.0, xofs);
  nearest_table(h, H, scaled ? depth_scale : 1.0, yofs);
  if (mask) {  // cv::resize(foregroundMask, foregroundMask, depth.size(), 0, 0, INTER_NEAREST)
    nearest_table(mask_w, W, (double)W / mask_w, mxofs);
    nearest_table(mask_h, H, (double)H / mask_h, myofs);
  }
  const size_t n = (size_t)W * H;
  const int nb = (int)blocks_of(n, kMeshBlock);
  TRY(upload_sync(c, m.disparity, disparity, (size_t)w * h * 4));
  TRY(upload_sync(c, m.tabs, tabs.data(), tabs.size() * 4));
  if (mask) {
    TRY(upload_sync(c, m.mask, mask, (size_t)mask_w * mask_h));
  }
  ALLOC(c, m.vert, n * 24);
  ALLOC(c, m.valid, n);
  ALLOC(c, m.qmask, n);
  ALLOC(c, m.used, n);
  ALLOC(c, m.blockFaces, (size_t)nb * 4);
  ALLOC(c, m.blockVerts, (size_t)nb * 4);
  ALLOC(c, m.offF, (size_t)nb * 8);
  ALLOC(c, m.offV, (size_t)nb * 8);
  ALLOC(c, m.totals, 24);
  ALLOC(c, m.vmap, n * 4);
  ALLOC(c, m.qoff, n * 4);
  const int* dt = m.tabs.as<int>();
  unsigned long long* totals = m.totals.as<unsigned long long>();  // kept faces, kept vertices, unmasked faces
  HIPCHK(c, hipMemsetAsync(totals, 0, 24, c->stream));
  hipLaunchKernelGGL(k_mesh_vertices, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.disparity.as<float>(), w, dt, dt + W, W, H,
                     resx, resy, fx, mask ? m.mask.as<uint8_t>() : (const uint8_t*)nullptr, mask_w, dt + W + H,
                     dt + 2 * W + H, m.vert.as<double>(), m.valid.as<uint8_t>());
  hipLaunchKernelGGL(k_mesh_quads, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.vert.as<double>() + 2, 3, m.valid.as<uint8_t>(),
                     W, H, tear_ratio, m.qmask.as<uint8_t>(), m.blockFaces.as<uint32_t>(), totals + 2);
  hipLaunchKernelGGL(k_mesh_vertex_used, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.qmask.as<uint8_t>(), W, H,
                     m.used.as<uint8_t>(), m.blockVerts.as<uint32_t>());
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, m.blockFaces.as<uint32_t>(), nb,
                     m.offF.as<unsigned long long>(), totals);
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, m.blockVerts.as<uint32_t>(), nb,
                     m.offV.as<unsigned long long>(), totals + 1);
  KCHECK(c);
  unsigned long long t[3] = {0, 0, 0};
  TRY(download_sync(c, t, totals, 24));
  m.nf = (size_t)t[0];
  m.nv = (size_t)t[1];
  m.nfUnmasked = (size_t)t[2];
  m.nfGrid = m.nf;
  if (m.nv > n || m.nf > 2 * n) {
    return fail(c, "derp_mesh_build: inconsistent counts (%zu vertices, %zu faces for %zu pixels)", m.nv, m.nf, n);
  }
  ALLOC(c, m.vorig, std::max<size_t>(m.nv * 4, 8));
  ALLOC(c, m.V, std::max<size_t>(m.nv * 24, 8));
  ALLOC(c, m.F, std::max<size_t>(m.nf * 12, 8));
  hipLaunchKernelGGL(k_mesh_vertex_scatter, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.vert.as<double>(), m.used.as<uint8_t>(),
                     n, m.offV.as<unsigned long long>(), m.vmap.as<uint32_t>(), m.vorig.as<uint32_t>(), m.V.as<double>());
  hipLaunchKernelGGL(k_mesh_face_scatter, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.qmask.as<uint8_t>(), W, H,
                     m.offF.as<unsigned long long>(), m.vmap.as<uint32_t>(), m.qoff.as<uint32_t>(), m.F.as<int32_t>());
  KCHECK(c);
  m.built = true;
  return 0;
}

// getVertexesEquirect + getFaces(wrapHorizontally = true, isRigCoordinates = true) (MeshUtil.h:264-314). Nothing is
// compacted: the vertices are the grid, and the set-up reads them as such.
int derp_mesh_build_equirect(derp_ctx* c, const float* disparity, int w, int h, float max_depth, float tear_ratio) {
  if (!c || !disparity) {
    return fail(c, "derp_mesh_build_equirect: null pointer");
  }
  if (w < 2 || h < 2) {
    return fail(c, "derp_mesh_build_equirect: a %d x %d equirect (the seam needs 2 columns, a face 2 rows)", w, h);
  }
  if ((size_t)w * h >= kMaxPixels) {
    return fail(c, "derp_mesh_build_equirect: %d x %d pixels are more than an index holds", w, h);
  }
  if (tear_ratio != tear_ratio) {
    return fail(c, "derp_mesh_build_equirect: tear_ratio is NaN");
  }
  if (max_depth != max_depth) {
    return fail(c, "derp_mesh_build_equirect: max_depth is NaN");
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // the mesh built before this one may still be read
  if (!c->mesh) {
    c->mesh.reset(new MeshState);
  }
  MeshState& m = *c->mesh;
  m.built = m.simplified = m.equirect = false;
  m.W = w;
  m.H = h;
  // `const float theta = u * 2.0f * M_PI`, `phi = v * M_PI` with u = float(x + 0.5) / float(width): the products with
  // M_PI are doubles, narrowed; sin / cos of them are the C library's double functions
  std::vector<double> tabs(2 * (size_t)w + 2 * (size_t)h);
  for (int x = 0; x < w; ++x) {
    const float u = float(x + 0.5) / float(w);
    const float theta = (float)(u * 2.0f * M_PI);
    tabs[x] = std::cos((double)theta);
    tabs[(size_t)w + x] = std::sin((double)theta);
  }
  for (int y = 0; y < h; ++y) {
    const float v = float(y + 0.5) / float(h);
    const float phi = (float)(v * M_PI);
    tabs[2 * (size_t)w + y] = std::sin((double)phi);
    tabs[2 * (size_t)w + h + y] = std::cos((double)phi);
  }
  const size_t n = (size_t)w * h;
  const int nb = (int)blocks_of(n, kMeshBlock);
  TRY(upload_sync(c, m.disparity, disparity, n * 4));
  TRY(upload_sync(c, m.tabs, tabs.data(), tabs.size() * 8));
  ALLOC(c, m.V, n * 24);
  ALLOC(c, m.norm, n * 8);
  ALLOC(c, m.qmask, n);
  ALLOC(c, m.used, n);      // (derp_mesh_simplify_parallel's createFinalMesh works in these two)
  ALLOC(c, m.vmap, n * 4);
  ALLOC(c, m.qoff, n * 4);
  ALLOC(c, m.blockFaces, (size_t)nb * 4);
  ALLOC(c, m.offF, (size_t)nb * 8);
  ALLOC(c, m.totals, 24);
  unsigned long long* totals = m.totals.as<unsigned long long>();  // grid faces, -, the same again
  HIPCHK(c, hipMemsetAsync(totals, 0, 24, c->stream));
  hipLaunchKernelGGL(k_mesh_vertices_equirect, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.disparity.as<float>(), w, h, max_depth,
                     m.tabs.as<double>(), m.V.as<double>(), m.norm.as<double>());
  hipLaunchKernelGGL(k_mesh_quads, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.norm.as<double>(), 1, (const uint8_t*)nullptr, w, h,
                     tear_ratio, m.qmask.as<uint8_t>(), m.blockFaces.as<uint32_t>(), totals + 2);
  hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, m.blockFaces.as<uint32_t>(), nb,
                     m.offF.as<unsigned long long>(), totals);
  KCHECK(c);
  unsigned long long t[3] = {0, 0, 0};
  TRY(download_sync(c, t, totals, 24));
  const size_t seamFaces = 2 * (size_t)(h - 1);
  if (t[0] != t[2] || t[0] > 2 * (size_t)(w - 1) * (size_t)(h - 1)) {
    return fail(c, "derp_mesh_build_equirect: inconsistent counts (%llu and %llu faces for %zu pixels)", t[0], t[2], n);
  }
  m.nfGrid = (size_t)t[0];
  m.nf = m.nfUnmasked = m.nfGrid + seamFaces;
  m.nv = n;
  ALLOC(c, m.F, m.nf * 12);
  hipLaunchKernelGGL(k_mesh_face_scatter, dim3(nb), dim3(kMeshBlock), 0, c->stream, m.qmask.as<uint8_t>(), w, h,
                     m.offF.as<unsigned long long>(), (const uint32_t*)nullptr, m.qoff.as<uint32_t>(), m.F.as<int32_t>());
  hipLaunchKernelGGL(k_mesh_seam_faces, dim3(blocks_of((size_t)h - 1, kMeshBlock)), dim3(kMeshBlock), 0, c->stream, w, h, m.nfGrid,
                     m.F.as<int32_t>());
  KCHECK(c);
  m.built = m.equirect = true;
  return 0;
}

int derp_mesh_counts(derp_ctx* c, size_t* vertices, size_t* faces, size_t* faces_unmasked) {
  TRY(need_mesh(c));
  const MeshState& m = *c->mesh;
  if (vertices) {
    *vertices = m.simplified ? m.sV.size() / 3 : m.nv;
  }
  if (faces) {
    *faces = m.simplified ? m.sF.size() / 3 : m.nf;
  }
  if (faces_unmasked) {
    *faces_unmasked = m.nfUnmasked;
  }
  return 0;
}

int derp_mesh_download_f64(derp_ctx* c, double* vertices, int32_t* faces) {
  TRY(need_mesh(c));
  const MeshState& m = *c->mesh;
  if (m.simplified) {
    if (vertices) {
      memcpy(vertices, m.sV.data(), m.sV.size() * 8);
    }
    if (faces) {
      memcpy(faces, m.sF.data(), m.sF.size() * 4);
    }
    return 0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (vertices && m.nv) {
    TRY(download_sync(c, vertices, m.V.p, m.nv * 24));
  }
  if (faces && m.nf) {
    TRY(download_sync(c, faces, m.F.p, m.nf * 12));
  }
  return 0;
}

int derp_mesh_download(derp_ctx* c, int clamp_negative_z, float* vtx, uint32_t* idx) {
  TRY(need_mesh(c));
  size_t nv = 0, nf = 0;
  TRY(derp_mesh_counts(c, &nv, &nf, nullptr));
  std::vector<double> v(nv * 3);
  std::vector<int32_t> f(nf * 3);
  TRY(derp_mesh_download_f64(c, vtx ? v.data() : nullptr, idx ? f.data() : nullptr));
  if (vtx) {
    for (size_t i = 0; i < nv * 3; ++i) {
      // "If depth is slightly negative ... we force this values to the minimum positive value" (:211-217), on the
      // double, before writeDepth's cast<float>
      vtx[i] = clamp_negative_z && i % 3 == 2 && v[i] < 0 ? FLT_MIN : (float)v[i];
    }
  }
  if (idx) {
    for (size_t i = 0; i < nf * 3; ++i) {
      idx[i] = (uint32_t)f[i];
    }
  }
  return 0;
}

int derp_mesh_setup(derp_ctx* c, int equi_error, double* face_planes, double* edge_costs, double* vertex_quadrics) {
  TRY(need_mesh(c));
  MeshState& m = *c->mesh;
  if (m.simplified) {
    return fail(c, "derp_mesh_setup: the mesh has been simplified (the set-up belongs to the mesh as built)");
  }
  HIPCHK(c, hipSetDevice(c->device));
  TRY(mesh_setup_dev(c, equi_error));
  if (face_planes && m.nf) {
    TRY(download_sync(c, face_planes, m.planes.p, m.nf * 32));
  }
  if (edge_costs && m.nf) {
    TRY(download_sync(c, edge_costs, m.costs.p, m.nf * 24));
  }
  if (vertex_quadrics && m.nv) {
    TRY(download_sync(c, vertex_quadrics, m.vq.p, m.nv * derp_mesh::kQuadric * 8));
  }
  return 0;
}

int derp_mesh_simplify(derp_ctx* c, int num_faces_out, float strictness, int remove_boundary_edges, int equi_error,
                       int host_setup, int* stats) {
  TRY(need_mesh(c));
  MeshState& m = *c->mesh;
  if (m.simplified) {
    return fail(c, "derp_mesh_simplify: the mesh has been simplified already");
  }
  if (num_faces_out < 0) {
    return fail(c, "derp_mesh_simplify: a negative face budget");
  }
  if (!(0 <= strictness && strictness <= 1)) {  // (NaN too) the threshold's rank would leave the feasible edges
    return fail(c, "strictness must be between 0 and 1 (got %g)", (double)strictness);
  }
  std::vector<double> V(m.nv * 3), planes, costs, vq;
  std::vector<int32_t> F(m.nf * 3);
  TRY(derp_mesh_download_f64(c, V.data(), F.data()));
  if (!host_setup) {
    planes.resize(m.nf * 4);
    costs.resize(m.nf * 3);
    vq.resize(m.nv * derp_mesh::kQuadric);
    TRY(derp_mesh_setup(c, equi_error, planes.data(), costs.data(), vq.data()));
  }
  m.sV.resize(V.size());
  m.sF.resize(F.size());
  size_t nv = 0, nf = 0;
  if (derp_mesh_simplify_host(V.data(), m.nv, F.data(), m.nf, host_setup ? nullptr : planes.data(),
                              host_setup ? nullptr : costs.data(), host_setup ? nullptr : vq.data(), num_faces_out, strictness,
                              remove_boundary_edges, equi_error, m.sV.data(), m.sF.data(), &nv, &nf, stats)) {
    return fail(c, "derp_mesh_simplify_host refused the built mesh");
  }
  m.sV.resize(nv * 3);
  m.sF.resize(nf * 3);
  m.simplified = true;
  return 0;
}

// The pass-parallel simplifier (derp_mesh.h, "the pass-parallel simplifier"): the whole loop on the device, the host
// reads one set of counters per pass.
int derp_mesh_simplify_parallel(derp_ctx* c, int num_faces_out, float strictness, int remove_boundary_edges, int equi_error,
                                int* stats) {
  TRY(need_mesh(c));
  MeshState& m = *c->mesh;
  if (m.simplified) {
    return fail(c, "derp_mesh_simplify_parallel: the mesh has been simplified already");
  }
  if (num_faces_out < 0) {
    return fail(c, "derp_mesh_simplify_parallel: a negative face budget");
  }
  if (!(0 <= strictness && strictness <= 1)) {  // (NaN too) the threshold's rank would leave the feasible edges
    return fail(c, "strictness must be between 0 and 1 (got %g)", (double)strictness);
  }
  HIPCHK(c, hipSetDevice(c->device));
  m.passes.clear();
  int passes = 0, reason = DERP_MESH_EXIT_BUDGET;
  const size_t nf = m.nf, nv = m.nv, n3 = nf * 3;
  long long aliveFaces = (long long)nf;
  if (n3 >= (size_t)kMeshApplied) {
    return fail(c, "derp_mesh_simplify_parallel: %zu faces are more than an edge rank holds", nf);
  }
  if (aliveFaces > num_faces_out) {
    TRY(mesh_setup_dev(c, equi_error));
    const int nbF = (int)blocks_of(nf, kMeshBlock), nbV = (int)blocks_of(nv, kMeshBlock);
    const int nbE = (int)blocks_of(n3, kMeshBlock);
    ALLOC(c, m.alive, nf);
    ALLOC(c, m.boundary, nv);
    ALLOC(c, m.vcount, nv * 4);
    ALLOC(c, m.vstart, nv * 4);
    ALLOC(c, m.vcursor, nv * 4);
    ALLOC(c, m.adj, n3 * 4);
    ALLOC(c, m.keys, n3 * 8);
    ALLOC(c, m.keysFeasible, n3 * 8);
    ALLOC(c, m.keysSorted, n3 * 8);
    ALLOC(c, m.vals, n3 * 4);
    ALLOC(c, m.valsSorted, n3 * 4);
    ALLOC(c, m.claim, nf * 4);
    ALLOC(c, m.wins, n3 * 4);
    ALLOC(c, m.blockSum, (size_t)nbE * 4);
    ALLOC(c, m.blockOff, (size_t)nbE * 8);
    ALLOC(c, m.counters, (MESH_CNT_SLOTS + 1) * 8);
    double* V = m.V.as<double>();
    int32_t* F = m.F.as<int32_t>();
    double *costs = m.costs.as<double>(), *vq = m.vq.as<double>();
    const double* planes = m.planes.as<double>();
    uint8_t *alive = m.alive.as<uint8_t>(), *boundary = m.boundary.as<uint8_t>();
    uint32_t *claim = m.claim.as<uint32_t>(), *wins = m.wins.as<uint32_t>(), *blockSum = m.blockSum.as<uint32_t>();
    unsigned long long *blockOff = m.blockOff.as<unsigned long long>(), *counters = m.counters.as<unsigned long long>();
    const MeshAdjacency A = {m.vstart.as<uint32_t>(), m.vcount.as<uint32_t>(), m.adj.as<uint32_t>()};
    const dim3 blk(kMeshBlock);
    HIPCHK(c, hipMemsetAsync(alive, 1, nf, c->stream));
    HIPCHK(c, hipMemsetAsync(boundary, 0, nv, c->stream));
    while (aliveFaces > num_faces_out) {
      if ((size_t)passes >= nf) {  // every pass with a candidate deletes a face
        return fail(c, "derp_mesh_simplify_parallel: %d passes over %zu faces", passes, nf);
      }
      // adjacency of the alive faces
      HIPCHK(c, hipMemsetAsync(m.vcount.p, 0, nv * 4, c->stream));
      HIPCHK(c, hipMemsetAsync(counters, 0, MESH_CNT_SLOTS * 8, c->stream));
      HIPCHK(c, hipMemsetAsync(claim, 0xff, nf * 4, c->stream));
      hipLaunchKernelGGL(k_par_vertex_degrees, dim3(nbF), blk, 0, c->stream, F, alive, nf, m.vcount.as<uint32_t>());
      hipLaunchKernelGGL(k_par_block_sums<uint32_t>, dim3(nbV), blk, 0, c->stream, m.vcount.as<uint32_t>(), nv, blockSum);
      hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbV, blockOff,
                         counters + MESH_CNT_SLOTS);
      hipLaunchKernelGGL(k_par_vertex_starts, dim3(nbV), blk, 0, c->stream, m.vcount.as<uint32_t>(), nv, blockOff,
                         m.vstart.as<uint32_t>(), m.vcursor.as<uint32_t>());
      hipLaunchKernelGGL(k_par_adjacency_fill, dim3(nbF), blk, 0, c->stream, F, alive, nf, m.vcursor.as<uint32_t>(),
                         m.adj.as<uint32_t>());
      if (passes == 0) {
        hipLaunchKernelGGL(k_par_boundaries, dim3(nbE), blk, 0, c->stream, A, F, nf, boundary);
      }
      // feasible set, its order, claims, winners
      hipLaunchKernelGGL(k_par_feasible, dim3(nbE), blk, 0, c->stream, A, V, F, alive, nf, planes, costs, vq, boundary,
                         remove_boundary_edges, equi_error, m.keys.as<unsigned long long>(), blockSum);
      hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbE, blockOff,
                         counters + MESH_CNT_FEASIBLE);
      hipLaunchKernelGGL(k_par_feasible_compact, dim3(nbE), blk, 0, c->stream, m.keys.as<unsigned long long>(), n3, blockOff,
                         m.keysFeasible.as<unsigned long long>(), m.vals.as<uint32_t>());
      KCHECK(c);
      unsigned long long feasible = 0;
      TRY(download_sync(c, &feasible, counters + MESH_CNT_FEASIBLE, 8));
      if (feasible == 0) {
        reason = DERP_MESH_EXIT_NO_CANDIDATES;
        break;
      }
      if (feasible > n3) {
        return fail(c, "derp_mesh_simplify_parallel: %llu feasible edges of %zu", feasible, n3);
      }
      size_t tempBytes = 0;
      HIPCHK(c, rocprim::radix_sort_pairs<MeshSortConfig>(nullptr, tempBytes, m.keysFeasible.as<unsigned long long>(),
                                                          m.keysSorted.as<unsigned long long>(), m.vals.as<uint32_t>(),
                                                          m.valsSorted.as<uint32_t>(), (size_t)feasible, 0, 64, c->stream));
      ALLOC(c, m.sortTemp, std::max<size_t>(tempBytes, 8));
      HIPCHK(c, rocprim::radix_sort_pairs<MeshSortConfig>(m.sortTemp.p, tempBytes, m.keysFeasible.as<unsigned long long>(),
                                                          m.keysSorted.as<unsigned long long>(), m.vals.as<uint32_t>(),
                                                          m.valsSorted.as<uint32_t>(), (size_t)feasible, 0, 64, c->stream));
      const unsigned long long* skeys = m.keysSorted.as<unsigned long long>();
      const uint32_t* svals = m.valsSorted.as<uint32_t>();
      const int nbN = (int)blocks_of((size_t)feasible, kMeshBlock);  // from here on one thread per feasible edge, by rank
      hipLaunchKernelGGL(k_par_claim, dim3(nbN), blk, 0, c->stream, A, F, skeys, svals, strictness, counters, claim);
      hipLaunchKernelGGL(k_par_winners, dim3(nbN), blk, 0, c->stream, A, F, skeys, svals, strictness, claim, counters, wins,
                         blockSum);
      // budget cut in key order, then the collapses
      hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbN, blockOff,
                         counters + MESH_CNT_SLOTS);
      hipLaunchKernelGGL(k_par_apply_vertices, dim3(nbN), blk, 0, c->stream, V, F, vq, boundary, equi_error, svals, blockOff,
                         aliveFaces, (long long)num_faces_out, wins, counters);
      hipLaunchKernelGGL(k_par_apply_faces, dim3(nbF), blk, 0, c->stream, V, F, alive, nf, vq, boundary, equi_error, svals, claim,
                         wins, costs);
      KCHECK(c);
      unsigned long long cnt[MESH_CNT_SLOTS];
      TRY(download_sync(c, cnt, counters, sizeof cnt));
      if (cnt[MESH_CNT_DELETED] == 0 || cnt[MESH_CNT_DELETED] > (unsigned long long)aliveFaces) {
        return fail(c, "derp_mesh_simplify_parallel: pass %d deleted %llu of %lld faces", passes, cnt[MESH_CNT_DELETED], aliveFaces);
      }
      derp_mesh_pass p;
      p.faces = aliveFaces;
      p.feasible = (long long)cnt[MESH_CNT_FEASIBLE];
      p.winners = (long long)cnt[MESH_CNT_WINNERS];
      p.applied = (long long)cnt[MESH_CNT_APPLIED];
      p.deleted = (long long)cnt[MESH_CNT_DELETED];
      p.threshold = mesh_key_cost(cnt[MESH_CNT_THRESHOLD]);
      m.passes.push_back(p);
      aliveFaces -= (long long)cnt[MESH_CNT_DELETED];
      ++passes;
    }
    // createFinalMesh
    uint8_t* used = m.used.as<uint8_t>();  // (grid-sized: at least nv bytes)
    uint32_t* vmap = m.vmap.as<uint32_t>();
    ALLOC(c, m.outV, std::max<size_t>(nv * 24, 8));
    ALLOC(c, m.outF, std::max<size_t>(nf * 12, 8));
    HIPCHK(c, hipMemsetAsync(used, 0, nv, c->stream));
    hipLaunchKernelGGL(k_par_vertices_used, dim3(nbF), blk, 0, c->stream, F, alive, nf, used);
    hipLaunchKernelGGL(k_par_block_sums<uint8_t>, dim3(nbV), blk, 0, c->stream, used, nv, blockSum);
    hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbV, blockOff, counters);
    hipLaunchKernelGGL(k_par_final_vertices, dim3(nbV), blk, 0, c->stream, V, used, nv, blockOff, vmap, m.outV.as<double>());
    hipLaunchKernelGGL(k_par_block_sums<uint8_t>, dim3(nbF), blk, 0, c->stream, alive, nf, blockSum);
    hipLaunchKernelGGL(k_scan_block_counts, dim3(1), dim3(1024), 0, c->stream, blockSum, nbF, blockOff, counters + 1);
    hipLaunchKernelGGL(k_par_final_faces, dim3(nbF), blk, 0, c->stream, F, alive, nf, blockOff, vmap, m.outF.as<int32_t>());
    KCHECK(c);
    unsigned long long out[2] = {0, 0};
    TRY(download_sync(c, out, counters, sizeof out));
    if (out[0] > nv || (long long)out[1] != aliveFaces) {
      return fail(c, "derp_mesh_simplify_parallel: inconsistent result (%llu vertices, %llu faces, %lld alive)", out[0], out[1],
                  aliveFaces);
    }
    m.sV.resize((size_t)out[0] * 3);
    m.sF.resize((size_t)out[1] * 3);
    if (out[0]) {
      TRY(download_sync(c, m.sV.data(), m.outV.p, m.sV.size() * 8));
    }
    if (out[1]) {
      TRY(download_sync(c, m.sF.data(), m.outF.p, m.sF.size() * 4));
    }
  } else {  // 0 passes: the mesh as built
    m.sV.resize(nv * 3);
    m.sF.resize(nf * 3);
    TRY(derp_mesh_download_f64(c, m.sV.data(), m.sF.data()));
  }
  m.simplified = true;
  if (stats) {
    stats[0] = passes;
    stats[1] = reason;
  }
  return 0;
}

int derp_mesh_parallel_pass(derp_ctx* c, int pass, derp_mesh_pass* out) {
  TRY(need_mesh(c));
  const MeshState& m = *c->mesh;
  if (!out || pass < 0 || (size_t)pass >= m.passes.size()) {
    return fail(c, "derp_mesh_parallel_pass: no pass %d (the last derp_mesh_simplify_parallel ran %zu)", pass, m.passes.size());
  }
  *out = m.passes[pass];
  return 0;
}
