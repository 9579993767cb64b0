// Debug and introspection: derp_debug_*, device pointers into the pyramid (derp_dev_*), counters, per-stage profiling,
// device queries, host-only self checks. Included by derp_capi.hip after the depth core.
#pragma once

namespace {
struct HostPairs {
  SsdPair* p;
  SsdPair get(int i) const {
    return p[i];
  }
  void set(int i, const SsdPair& v) {
    p[i] = v;
  }
};
// kStageNames' index of a stage name (-1: none)
int stage_index(const char* stage) {
  for (int i = 0; i < ST_COUNT; ++i) {
    if (strcmp(stage, kStageNames[i]) == 0) {
      return i;
    }
  }
  return -1;
}
}  // namespace

int derp_debug_atan2_ypos(derp_ctx* c, const double* y, const double* x, double* out, size_t n) {
  if (!c || !y || !x || !out) {
    return fail(c, "bad arguments");
  }
  ALLOC(c, c->w.staging, 3 * n * sizeof(double));
  double* d = c->w.staging.as<double>();
  HIPCHK(c, hipMemcpyAsync(d, y, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + n, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_debug_atan2_ypos, dim3(flat_grid(n)), dim3(256), 0, c->stream, d, d + n, d + 2 * n, n);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(out, d + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_debug_fp64(derp_ctx* c, int op, const double* a, const double* b, double* out, size_t n) {
  if (!c || !a || !out || op < 0 || op > 3 || (op >= 2 && !b)) {
    return fail(c, "bad arguments");
  }
  if (n == 0) {
    return 0;
  }
  ALLOC(c, c->w.staging, 3 * n * sizeof(double));
  double* d = c->w.staging.as<double>();
  HIPCHK(c, hipMemcpyAsync(d, a, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + n, op >= 2 ? b : a, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_debug_fp64, dim3(flat_grid(n)), dim3(256), 0, c->stream, op, d, d + n, d + 2 * n, n);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(out, d + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_debug_expf(derp_ctx* c, int mode, const float* x, float* out, size_t n) {
  if (!c || !x || !out || mode < 0 || mode > 2) {  // (2: the cost core's round_half_away_pos)
    return fail(c, "bad arguments");
  }
  if (n == 0) {
    return 0;
  }
  ALLOC(c, c->w.staging, 2 * n * sizeof(float));
  float* d = c->w.staging.as<float>();
  HIPCHK(c, hipMemcpyAsync(d, x, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_debug_expf, dim3(flat_grid(n)), dim3(256), 0, c->stream, mode, d, d + n, n);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(out, d + n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_debug_sees(derp_ctx* c, int src, const double* xyz, size_t n, double* out) {
  if (!c || !xyz || !out || src < 0 || src >= c->S) {
    return fail(c, "bad arguments");
  }
  if (n == 0) {
    return 0;
  }
  ALLOC(c, c->w.staging, 9 * n * sizeof(double));
  double* d = c->w.staging.as<double>();
  HIPCHK(c, hipMemcpyAsync(d, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_debug_sees, dim3(flat_grid(n)), dim3(256), 0, c->stream, c->camsSrc.as<Cam>(), src, d, d + 3 * n, n);
  KCHECK(c);
  HIPCHK(c, hipMemcpyAsync(out, d + 3 * n, 6 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int derp_debug_download(derp_ctx* c, int d, int s, int which, void* out) {
  TRY(need_current(c, false));
  const int L = c->cur;
  const int W = c->LW[L], H = c->LH[L];
  const size_t n = (size_t)W * H;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (which == 4) {
    HIPCHK(c, hipMemcpy(out, c->w.srcVar.as<float>() + (size_t)s * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  if (which == 5) {
    HIPCHK(c, hipMemcpy(out, c->fovMask.as<uint8_t>() + (size_t)d * n, n, hipMemcpyDeviceToHost));
    return 0;
  }
  if (which == 9) {  // the own colour bias of source `s`, as u16 x 3
    if (s < 0 || s >= c->S) {
      return fail(c, "bad source index");
    }
    std::vector<ushort4> tmp(n);
    HIPCHK(c, hipMemcpy(tmp.data(), c->w.ownBias.as<ushort4>() + (size_t)s * n, n * sizeof(ushort4), hipMemcpyDeviceToHost));
    uint16_t* o = reinterpret_cast<uint16_t*>(out);
    for (size_t i = 0; i < n; ++i) {
      o[i * 3 + 0] = tmp[i].x;
      o[i * 3 + 1] = tmp[i].y;
      o[i * 3 + 2] = tmp[i].z;
    }
    return 0;
  }
  if (which == 10) {  // k_row_rank's engine states of destination `d`: defined at the gated-in interior pixels only
    if (d < 0 || d >= c->D) {
      return fail(c, "bad destination index");
    }
    HIPCHK(c, hipMemcpy(out, c->w.rank.as<int>() + (size_t)d * n, n * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
  }
  if (d < 0 || d >= c->D || s < 0 || s >= c->S || s == c->dst2srcH[d]) {
    return fail(c, "bad (dst, src) pair");
  }
  const size_t tab = (size_t)d * (c->S - 1) + (s < c->dst2srcH[d] ? s : s - 1);
  if (which == 0) {
    const int PW = W + 2 * kPadW, PH = H + 2 * kPadW;
    std::vector<float2> tmp((size_t)PW * PH);
    HIPCHK(c, hipMemcpy(tmp.data(), c->projWarp.as<float2>() + tab * tmp.size(), tmp.size() * sizeof(float2),
                        hipMemcpyDeviceToHost));
    float2* o = reinterpret_cast<float2*>(out);
    for (int y = 0; y < H; ++y) {
      memcpy(o + (size_t)y * W, &tmp[(size_t)(y + kPadW) * PW + kPadW], (size_t)W * sizeof(float2));
    }
    return 0;
  }
  if (which == 2 || which == 3) {
    const int PW = W + 2 * kPadC, PH = H + 2 * kPadC;
    std::vector<ushort4> tmp((size_t)PW * PH);
    const ushort4* base = (which == 2 ? c->w.projColor.as<ushort4>() : c->w.projBias.as<ushort4>()) + tab * tmp.size();
    HIPCHK(c, hipMemcpy(tmp.data(), base, tmp.size() * sizeof(ushort4), hipMemcpyDeviceToHost));
    uint16_t* o = reinterpret_cast<uint16_t*>(out);
    for (int y = 0; y < H; ++y) {
      for (int x = 0; x < W; ++x) {
        const ushort4 q = tmp[(size_t)(y + kPadC) * PW + x + kPadC];
        o[((size_t)y * W + x) * 3 + 0] = q.x;
        o[((size_t)y * W + x) * 3 + 1] = q.y;
        o[((size_t)y * W + x) * 3 + 2] = q.z;
      }
    }
    return 0;
  }
  if (which == 6 || which == 7) {  // the whole padded plane, ring included: what the cost kernels read at the image edge
    const size_t plane = (size_t)(W + 2 * kPadC) * (H + 2 * kPadC);
    const DevBuf& buf = which == 6 ? c->w.projColor : c->w.projBias;
    if (buf.bytes < (tab + 1) * plane * sizeof(ushort4)) {
      return fail(c, "the colour tables of this level have not been built");
    }
    HIPCHK(c, hipMemcpy(out, buf.as<ushort4>() + tab * plane, plane * sizeof(ushort4), hipMemcpyDeviceToHost));
    return 0;
  }
  if (which == 8) {  // k_reproject_bias's tileSeen flags of the table, [tilesY][tilesX]
    const size_t tiles = (size_t)((W + kRbTile - 1) / kRbTile) * ((H + kRbTile - 1) / kRbTile);
    if (c->w.tileSeen.bytes < (tab + 1) * tiles) {
      return fail(c, "the colour tables of this level have not been built");
    }
    HIPCHK(c, hipMemcpy(out, c->w.tileSeen.as<uint8_t>() + tab * tiles, tiles, hipMemcpyDeviceToHost));
    return 0;
  }
  return fail(c, "unknown table id %d", which);
}

int derp_dev_disparity(derp_ctx* c, int level, int d, float** ptr, size_t* bytes) {
  TRY(check_level(c, level));
  if (d < 0 || d >= c->D || !ptr || !bytes) {
    return fail(c, "bad destination index / null output");
  }
  const size_t n = npx(c, level);
  *ptr = c->frame().disp[level].as<float>() + (size_t)d * n;
  *bytes = n * sizeof(float);
  return 0;
}
int derp_dev_color(derp_ctx* c, int level, int s, void** ptr, size_t* bytes) {
  TRY(check_level(c, level));
  if (s < 0 || s >= c->S || !ptr || !bytes) {
    return fail(c, "bad source index / null output");
  }
  const size_t n = npx(c, level);
  *ptr = c->frame().color[level].as<ushort4>() + (size_t)s * n;
  *bytes = n * sizeof(ushort4);
  return 0;
}
int derp_dev_mask(derp_ctx* c, int level, int d, uint8_t** ptr, size_t* bytes) {
  TRY(check_level(c, level));
  if (d < 0 || d >= c->D || !ptr || !bytes) {
    return fail(c, "bad destination index / null output");
  }
  HIPCHK(c, hipSetDevice(c->device));
  // fov & fg of `level` (TemporalBilateralFilter.cpp:150-160) for every destination, into a buffer of its
  // own (never a working buffer of the level loop), complete when this call returns
  const int W = c->LW[level], H = c->LH[level];
  const size_t n = (size_t)W * H;
  ALLOC(c, c->devMask, n * c->D);
  hipLaunchKernelGGL(k_fov_mask, grid2d(W, H, c->D, kBlk2d), kBlk2d, 0, c->stream, c->camsDst.as<Cam>(), W, H,
                     c->devMask.as<uint8_t>());
  KCHECK(c);
  hipLaunchKernelGGL(k_and_masks, dim3(flat_grid(n), c->D), dim3(256), 0, c->stream, c->devMask.as<uint8_t>(),
                     c->frame().fg[level].as<uint8_t>(), c->dst2src.as<int>(), 0, n, c->devMask.as<uint8_t>());
  KCHECK(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *ptr = c->devMask.as<uint8_t>() + (size_t)d * n;
  *bytes = n;
  return 0;
}

int derp_get_counters(derp_ctx* c, uint64_t* n_cost, uint64_t* n_pair, uint64_t* insufficient) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> h((size_t)ST_COUNT * kMaxLevels * 4);
  HIPCHK(c, hipMemcpy(h.data(), c->counters.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  uint64_t a = 0, b = 0, i = 0;
  for (size_t k = 0; k < h.size(); k += 4) {
    a += h[k];
    b += h[k + 1];
    i += h[k + 2];
  }
  if (n_cost) {
    *n_cost = a;
  }
  if (n_pair) {
    *n_pair = b;
  }
  if (insufficient) {
    *insufficient = i;
  }
  return 0;
}
int derp_reset_counters(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipMemsetAsync(c->counters.p, 0, c->counters.bytes, c->stream));
  return 0;
}
int derp_profile_enable(derp_ctx* c, int on) {
  if (!c) {
    return 1;
  }
  c->profiling = on != 0;
  return 0;
}
int derp_profile_reset(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  drain_spans(c);
  memset(c->accMs, 0, sizeof c->accMs);
  memset(c->accLaunch, 0, sizeof c->accLaunch);
  return derp_reset_counters(c);
}
int derp_profile_query(derp_ctx* c, const char* stage, int level, double* ms, int* launches, uint64_t* n_cost,
                       uint64_t* n_pair) {
  if (!c || !stage) {
    return 1;
  }
  const int st = stage_index(stage);
  if (st < 0) {
    return fail(c, "unknown stage '%s'", stage);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  drain_spans(c);
  std::vector<unsigned long long> h((size_t)kMaxLevels * 4);
  HIPCHK(c, hipMemcpy(h.data(), counter_slot(c, st, 0), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  double m = 0;
  int l = 0;
  uint64_t a = 0, b = 0;
  for (int lv = 0; lv < kMaxLevels; ++lv) {
    if (level >= 0 && lv != level) {
      continue;
    }
    m += c->accMs[st][lv];
    l += c->accLaunch[st][lv];
    a += h[(size_t)lv * 4];
    b += h[(size_t)lv * 4 + 1];
  }
  if (ms) {
    *ms = m;
  }
  if (launches) {
    *launches = l;
  }
  if (n_cost) {
    *n_cost = a;
  }
  if (n_pair) {
    *n_pair = b;
  }
  return 0;
}
int derp_profile_memoised(derp_ctx* c, const char* stage, int level, uint64_t* n_memoised) {
  if (!c || !stage || !n_memoised) {
    return 1;
  }
  const int st = stage_index(stage);
  if (st < 0) {
    return fail(c, "unknown stage '%s'", stage);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> h((size_t)kMaxLevels * 4);
  HIPCHK(c, hipMemcpy(h.data(), counter_slot(c, st, 0), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  uint64_t m = 0;
  for (int lv = 0; lv < kMaxLevels; ++lv) {
    if (level < 0 || lv == level) {
      m += h[(size_t)lv * 4 + 3];
    }
  }
  *n_memoised = m;
  return 0;
}
int derp_debug_block_trace(derp_ctx* c, const char* stage, int level, uint64_t* out, size_t capacity, int* grid_x, int* grid_y) {
  if (!c || !stage || !grid_x || !grid_y || level < 0 || level >= kMaxLevels) {
    return fail(c, "bad arguments");
  }
#if DERP_BLOCK_TRACE
  const int which = strcmp(stage, "random_proposals") == 0 ? 0 : strcmp(stage, "ping_pong") == 0 ? 1 : -1;
  if (which < 0) {
    return fail(c, "no block trace of stage '%s'", stage);
  }
  *grid_x = c->blockTraceGrid[which][level][0];
  *grid_y = c->blockTraceGrid[which][level][1];
  const size_t n = (size_t)*grid_x * *grid_y * 2;
  if (!out || capacity < n) {
    return 0;  // (the size query)
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, c->blockTrace[which][level].as<unsigned long long>(), n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return 0;
#else
  (void)out, (void)capacity;
  return fail(c, "this library records no block trace: build it with -DDERP_BLOCK_TRACE=1 (tools/block_trace.py)");
#endif
}
int derp_debug_level_plan(derp_ctx* c, int32_t* out) {
  if (!c || !out) {
    return fail(c, "bad arguments");
  }
  out[0] = c->plan.level;
  out[1] = c->plan.DB;
  out[2] = c->plan.storeInverse;
  out[3] = c->plan.decisions;
  return 0;
}
int derp_device_memory(derp_ctx* c, uint64_t* free_bytes, uint64_t* total_bytes) {
  TRY(use_device(c));
  size_t f = 0, t = 0;
  HIPCHK(c, hipMemGetInfo(&f, &t));
  if (free_bytes) {
    *free_bytes = f;
  }
  if (total_bytes) {
    *total_bytes = t;
  }
  return 0;
}

int derp_device_name(derp_ctx* c, char* buf, int n) {
  if (!c || !buf || n <= 0) {
    return 1;
  }
  hipDeviceProp_t prop;
  HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
  snprintf(buf, n, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return 0;
}

// ---- host-only self checks ----
int derp_host_nth_element_pairs(float* pairs, int n, int nth) {
  HostPairs acc{reinterpret_cast<SsdPair*>(pairs)};
  GccSelect<HostPairs> sel(acc);
  sel.nth_element(nth, n);
  return 0;
}
float derp_host_minstd_uniform(int seed, uint64_t draw_index, float a, float b) {
  uint32_t state = minstd_jump(minstd_seed(seed), draw_index);
  return minstd_uniform(state, a, b);
}
// the tile order of a random-proposal / ping-pong launch over `tiles` tiles as the kernels compute it: out[b * per_block +
// step] for every block b of the grid and step of its walk; returns the grid's block count (0: bad arguments or capacity)
int derp_host_cost_tile_map(int tiles, int bands, int rot, int per_block, int* out, int capacity) {
  const auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
  if (tiles <= 0 || !pow2(bands) || bands > kCostMaxBands || !pow2(per_block) || per_block > kCostMaxTilesPerBlock || !out) {
    return 0;
  }
  const int blocks = cost_grid_blocks(tiles, bands, per_block);
  if ((long long)blocks * per_block > capacity) {
    return 0;
  }
  for (int b = 0; b < blocks; ++b) {
    for (int step = 0; step < per_block; ++step) {
      out[b * per_block + step] = cost_block_tile(b, blocks, rot, bands, per_block, step);
    }
  }
  return blocks;
}
// the table budget -> the destination batch, as level_open decides it (plan_table_batch); 1: refused
int derp_host_table_batch(int n_dst, uint64_t bytes_no_inverse, uint64_t bytes_with_inverse, int inverse_needed,
                          uint64_t budget_bytes, int* batch, int* store_inverse) {
  const TableBatch b = plan_table_batch(n_dst, bytes_no_inverse, bytes_with_inverse, inverse_needed != 0, budget_bytes);
  if (!batch || !store_inverse || b.DB < 1) {
    return 1;
  }
  *batch = b.DB;
  *store_inverse = b.storeInverse;
  return 0;
}
