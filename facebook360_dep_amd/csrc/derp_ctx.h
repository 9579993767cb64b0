// The depth context behind the C-ABI (include/derp_hip.h): the rig, the HBM-resident pyramid of every frame slot, the
// working level of the level loop, profiling and developer switches, and one lazily created state per tool family (each
// defined in that family's derp_*_api.h). Included by derp_capi.hip (one translation unit) after the kernel headers.
#pragma once

namespace {

enum Stage {
  ST_FOV = 0,
  ST_VARIANCE,
  ST_OWN_BIAS,
  ST_UPSAMPLE,
  ST_PROJ_WARP,
  ST_REPROJECT,
  ST_PROJ_BIAS,
  ST_BRUTE,
  ST_RANDOM,
  ST_PINGPONG,
  ST_MISMATCH,
  ST_BILATERAL,
  ST_MEDIAN,
  ST_MASKFOV,
  ST_TEMPORAL,
  ST_LANES,  // wall of a level whose frames ran on overlapping work lanes (their per-stage spans overlap in time)
  ST_GC_PREPARE,  // GeometricConsistency (derp_geometric_api.h), timed under level 0
  ST_GC_SWEEP,
  ST_GC_CLEAN,
  ST_SWEEP_OVERLAPS,  // the rig preview tools (derp_sweep_api.h), timed under level 0
  ST_SWEEP_EQUIRECT,
  ST_ALIGN_MAPS,  // AlignColors (derp_align_api.h), timed under level 0
  ST_ALIGN_COLORS,
  ST_COVERAGE,  // RigAnalyzer (derp_coverage_api.h), timed under level 0
  ST_COUNT
};
const char* kStageNames[ST_COUNT] = {"fov_mask",  "variance",    "own_bias",         "upsample",  "proj_warp",
                                     "reproject", "proj_bias",   "brute_force",      "random_proposals",
                                     "ping_pong", "mismatches",  "bilateral",        "median",    "mask_fov",
                                     "temporal",  "lanes_wall", "gc_prepare",       "gc_sweep",  "gc_clean",
                                     "sweep_overlaps", "sweep_equirect", "align_maps",       "align_colors", "coverage"};
constexpr int kMaxLevels = 24;

struct TimedSpan {
  int stage, level;
  hipEvent_t a, b;
};

struct LanczosTab {
  DevBuf ofs, coef;
  // as the vertical table of k_lanczos: the source rows one output tile needs at the most, and whether the offsets never
  // decrease (they do not; the kernel's row window rests on it)
  int tileSpan = 0;
  bool monotone = true;
};

struct AreaTabDev {  // computeResizeAreaTab of one axis, resident in HBM
  DevBuf start, si, alpha;
  int iscale = 0;
};

// Everything processLevel writes per frame. The context has one and every work lane has one; the rig-only tables of a
// level (projWarp, projWarpInv, rayDir, behind, resampling tables) are shared by the lanes and stay on the context.
struct WorkSet {
  DevBuf srcVar, ownBias, maskAnd, disparity, cost, confidence, dispRes, costRes, changed, tmpF, rank, mismatchMask, pairCount;
  DevBuf rankPowers;  // k_row_rank: (a^P)^k mod m for k < rankPowersN, P = rankPowersP (k_minstd_powers)
  int rankPowersP = -1, rankPowersN = 0;
  DevBuf tileSeen;    // k_reproject_bias: per (table, tile) whether any map position is valid
  DevBuf projColor, projBias;
  DevBuf projColorT;  // projColor again in 4x4-texel tiles: the random-proposal kernel's copy (DERP_RANDOM_TILED)
  DevBuf bruteCost, bruteConf, lanczosTmp, staging, stagingB;
  bool mismatchMaskHeld = false;   // mismatchMask was cleared for the current level (the mismatch stage runs at it)
  // level whose colour / bias tables were written in full, and the warps they were written for (derp_ctx::warpGeneration
  // at that time): blank tiles may be skipped only while both still hold
  int colorTablesCleanLevel = -1;
  uint64_t colorTablesWarpGeneration = 0;
};

// HBM-resident pyramid of one frame, per level: colour, fg masks, background disparity, result
struct FramePyramid {
  std::vector<DevBuf> color, fg, bg, disp;
  std::vector<char> haveBg, haveDisp;
};

// What the frames of one pass over a level share (level_open): the destination batch that fits the table budget and
// whether inverse warps are stored. The first frame of the pass makes it, the others, the work lanes' too, only read it.
struct LevelPlan {
  int level = -1;  // the level it was made for (-1: none)
  int DB = 0;
  bool storeInverse = false;
  int decisions = 0;  // level_open calls since derp_create (derp_debug_level_plan)
};
struct TableBatch {  // plan_table_batch's answer
  int DB;
  bool storeInverse;
};
// A frame's place in a pass over a level. Open: the first frame, and every direct call: it makes the level's plan and
// honours opt.rebuild_warp_tables. Join: a later frame: it reuses the plan and what Open left in the shared tables.
enum class LevelUse { Open, Join };

struct WorkLane {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  WorkSet w;
};

// per tool family, defined in its derp_*_api.h and created by the family's first call that needs it
struct SmrState; struct RephotoState; struct PointsState; struct MeshState; struct GcState; struct SweepState; struct AlignState; struct CoverageState; struct StreamState;

}  // namespace

struct derp_ctx {
  derp_ctx();  // both defined at the end of derp_capi.hip, where the family states are complete types
  ~derp_ctx();
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copyStream = nullptr;  // input uploads of a frame that is not being computed (sequence driver), with
  DevBuf copyStaging;                // their own staging buffer: they overlap the compute of the frame before
  std::string err;
  std::string* errSink() {
    return &err;
  }
  derp_options opt;
  // ---- the rig
  int S = 0, D = 0;
  std::vector<Cam> camsSrcH, camsDstH;
  std::vector<int> dst2srcH;
  std::vector<derp_camera_desc> descDstH;  // the destinations as the rig file holds them (un-normalised: derp_points_* etc.)
  DevBuf camsSrc, camsDst, dst2src;

  // ---- the pyramid and its frame slots
  int numLevels = 0, widthFull = 0, heightFull = 0;
  std::vector<int> LW, LH;
  // one pyramid per frame slot (derp_set_frame_slots / derp_select_frame: several frames of one sequence resident on
  // this GPU); the level loop works on the selected one
  std::vector<FramePyramid> frames;
  int curSlot = 0;
  FramePyramid& frame() {
    return frames[curSlot];
  }
  // the sequences made on this context and not destroyed yet (derp_seq_create / derp_seq_destroy), each with the words an
  // error message names it by: their buffers have this geometry's sizes, so derp_set_pyramid refuses while one is open
  std::vector<std::pair<const derp_seq*, std::string>> openSeqs;
  DevBuf fullFrame;  // the pyramid builder's full-size input
  DevBuf devMask;    // derp_dev_mask result (not a working buffer)

  // ---- the working level
  int cur = -1;
  LevelPlan plan;
  WorkSet w;             // the per-frame working set in use: the context's own, or a lane's while its frame runs
  DevBuf temporalCarry;  // accumulators of a temporal window longer than one launch holds
  DevBuf projWarp, projWarpInv;
  DevBuf rayDir, behind;  // per destination pixel: ray direction [3][D][n] f64, sources facing away [D][n] (k_pixel_rays)
  int warpCachedLevel = -1;
  // counts every rebuild of the shared warps and every new geometry (build_warp, derp_set_pyramid): what a work set, the
  // context's own or a lane's, wrote for an earlier value was written for other warps
  uint64_t warpGeneration = 1;
  DevBuf fovMask;  // the destinations' FOV masks of level fovCachedLevel [D][n]: rig + level size only, shared by the lanes
  int fovCachedLevel = -1;
  bool randomRanThisLevel = false;  // cost / confidence hold random-proposal results for this level
  bool tablesValid = false;
  std::map<std::pair<int, int>, LanczosTab> lanczos;  // (map nodes keep their addresses: get_lanczos / get_area_tab
  std::map<std::pair<int, int>, AreaTabDev> areaTabs;  // hand out pointers into them)
  DevBuf spiral;
  int spiralN = 0, spiralRadius = -1;
  // Work lanes (round 6): a second, third ... working set + stream for processLevel of ANOTHER frame of a sequence at the
  // same coarse level (derp_seq_level_compute). The frames of a level are independent, and at the coarse levels one
  // frame's kernels fill a fraction of the chip (level 6 of the 16-camera rig: 784 waves for 4096 wave slots) and are
  // bound by their own serial latency — on lanes the frames' kernels overlap. A lane holds everything processLevel writes
  // per frame (a WorkSet); the rig-only tables of the level (projWarp, projWarpInv, rayDir, behind, resampling tables) stay
  // shared.
  std::vector<std::unique_ptr<WorkLane>> lanes;
  hipEvent_t laneReady = nullptr;  // recorded on the main stream behind what the lanes' frames depend on
  int activeLane = -1;             // the lane whose work set is swapped in (-1: the context's own)

  // ---- profiling and developer switches
  DevBuf counters;  // [ST_COUNT][kMaxLevels][4] u64
  bool profiling = false;
  std::vector<TimedSpan> spans;
  double accMs[ST_COUNT][kMaxLevels] = {};
  int accLaunch[ST_COUNT][kMaxLevels] = {};
  int xcdRotate = 1;
  // random proposals' / ping-pong's tile order (cost_grid): bands per XCD and tiles per block, 0 = the launcher's rule
  // (DERP_XCD_BANDS / DERP_COST_TILES_PER_BLOCK, developer A/B switches; same results), read once in derp_create
  int xcdBands = 0, costTilesPerBlock = 0;
  // DERP_BLOCK_TRACE builds (tools/block_trace.py): {start, end} of every block of the last random-proposal [0] /
  // ping-pong [1] launch of a level, and that launch's grid (x, y)
  DevBuf blockTrace[2][kMaxLevels];
  int blockTraceGrid[2][kMaxLevels][2] = {};
  bool noMemo = false;  // DERP_NO_MEMO (developer switch), read once in derp_create
  // consecutive disparity indices one block of k_brute_costs evaluates (DERP_BRUTE_RUN, developer A/B switch; same
  // results for every length from 1 to 150), read once in derp_create
  int bruteRun = 10;
  // ping-pong's candidate loop: compacted into full waves of (pixel, candidate) tasks, or one pixel per lane
  // (DERP_PP_COMPACT=0, developer A/B switch; same results), read once in derp_create
  bool ppCompact = true;
  // waves per SIMD of the random-proposal / ping-pong kernels (0 = what their registers and LDS allow: four up to 16
  // cameras): a launch can ask for fewer by reserving more LDS per (one-wave) block — DERP_RANDOM_WAVES / DERP_PP_WAVES,
  // developer A/B switches
  int randomWaves = 0, ppWaves = 0;
  size_t ldsPerCu = 160 * 1024;  // hipDeviceProp.maxSharedMemoryPerMultiProcessor (derp_create)
  bool noTemporalTile = false;  // DERP_NO_TEMPORAL_TILE (developer A/B: the direct form of the temporal filter)
  bool noBlankSkip = false;     // DERP_NO_BLANK_SKIP (developer A/B: every frame rewrites the blank tiles of the colour tables)
  // DERP_TEMPORAL_GENERIC (developer A/B: k_temporal_tiled's generic form — full expf, a mask read per tap, run-time
  // radius — where the fast form would run) and DERP_REPROJECT_SERIAL (developer A/B: k_reproject_bias's one-cell-at-a-time
  // form instead of the front-loaded one); same results either way, read once in derp_create
  bool temporalGeneric = false, reprojectSerial = false;
  // ---- the tool families' states
  std::unique_ptr<SmrState> smr;
  std::unique_ptr<RephotoState> rephoto;
  std::unique_ptr<PointsState> points;
  std::unique_ptr<MeshState> mesh;
  std::unique_ptr<GcState> gc;
  std::unique_ptr<SweepState> sweep;
  std::unique_ptr<AlignState> align;
  std::unique_ptr<CoverageState> coverage;
  std::unique_ptr<StreamState> meshStream;
};

namespace {

// the context's error channel (derp_last_error(c)); a null context drops the text
int fail(derp_ctx* c, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(c ? &c->err : nullptr, fmt, ap);
  va_end(ap);
  return 1;
}

// the prologue of the entry points that take nothing to validate but the context: bind its device to the thread
int use_device(derp_ctx* c) {
  if (!c) {
    return 1;
  }
  HIPCHK(c, hipSetDevice(c->device));
  return 0;
}

// `cam` indexes a destination camera of the context
int check_camera(derp_ctx* c, int cam) {
  if (cam < 0 || cam >= c->D) {
    return fail(c, "bad camera index %d (the context has %d)", cam, c->D);
  }
  return 0;
}

}  // namespace
