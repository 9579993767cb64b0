/*
 * derp_hip.h — C-ABI of the MI355X-native depth_estimation hot path.
 *
 * The reference (facebook360_dep) has no plugin/FFI seam for this path: its boundary is the
 * DerpCLI / TemporalBilateralFilter / UpsampleDisparity process CLIs and, in-process, the free
 * functions of source/depth_estimation/Derp.h. This header is the seam a maintainer would bind
 * those mains to (INTEGRATION.md shows the binding). Every entry point cites the reference
 * function it replaces (paths relative to the reference tree).
 *
 * Conventions: POD only, plain pointers and sizes; images row-major; colour = interleaved BGR
 * uint16 (cv::Vec3w, DerpUtil.h:19); masks uint8 {0,1}; disparity float32 with NaN = invalid.
 * Host pointers unless a name says `_dev`. One context per GPU, one calling thread per context.
 * Every function returns 0 on success, non-zero on error (never throws / aborts across the ABI);
 * derp_last_error() holds the glog-style message the CLI prints before exiting 1.
 * There is NO CPU fallback: derp_create fails when no gfx950-class HIP device is present.
 */
#ifndef DERP_HIP_H
#define DERP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct derp_ctx derp_ctx;

/* Camera::Type, source/util/Camera.h:43 */
enum { DERP_FTHETA = 0, DERP_RECTILINEAR = 1, DERP_EQUISOLID = 2, DERP_ORTHOGRAPHIC = 3 };

/* One camera exactly as the rig JSON holds it (Camera::Camera(const folly::dynamic&),
 * source/util/Camera.cpp:30-75). The library performs the constructor's work itself:
 * right-handedness check + AngleAxis re-unitarisation (Camera.cpp:77-87), distortionMax
 * (Camera.cpp:119-154), cosFov (Camera.cpp:204-207), then Camera::normalize (Camera.cpp:225-229). */
typedef struct {
  int32_t type;
  int32_t has_principal;
  int32_t has_distortion;
  int32_t has_fov;
  double origin[3];
  double forward[3];
  double up[3];
  double right[3];
  double resolution[2];
  double focal[2];
  double principal[2];
  double distortion[3];
  double fov;
  char id[64];
} derp_camera_desc;

/* DerpCLI flags that shape the computation (source/depth_estimation/DerpCLI.cpp:40-67);
 * derp_options_default() fills the reference defaults. */
typedef struct {
  float min_depth_m;            /* --min_depth_m            0.5   */
  float max_depth_m;            /* --max_depth_m            1e4   */
  float var_noise_floor;        /* --var_noise_floor        4e-5  */
  float var_high_thresh;        /* --var_high_thresh        1e-3  */
  int32_t random_proposals;     /* --random_proposals       2     */
  int32_t ping_pong_iterations; /* --ping_pong_iterations   1     */
  int32_t mismatches_start_level; /* --mismatches_start_level -1 (-1 = no mismatch handling) */
  int32_t do_bilateral_filter;  /* --do_bilateral_filter    1     */
  int32_t do_median_filter;     /* --do_median_filter       1     */
  int32_t use_foreground_masks; /* --use_foreground_masks   0     */
  int32_t partial_coverage;     /* --partial_coverage       0     */
  int32_t rebuild_warp_tables;  /* 1 = recompute projection warps every process_level like the
                                   reference (DerpCLI.cpp:274); 0 = cache per level across frames */
} derp_options;

void derp_options_default(derp_options* o);

/* ---- lifetime --------------------------------------------------------------------------- */
/* rigSrc / rigDst (DerpCLI.cpp:185-192). dst cameras are matched to src by id
 * (mapSrcToDstIndexes, DerpUtil.cpp:75-89). */
int derp_create(derp_ctx** out, int device, const derp_camera_desc* src, int n_src,
                const derp_camera_desc* dst, int n_dst);
void derp_destroy(derp_ctx* ctx);
const char* derp_last_error(const derp_ctx* ctx);
int derp_set_options(derp_ctx* ctx, const derp_options* o);

/* Pyramid geometry (getPyramidLevelSizes, Derp.cpp:72-99; widthFullSize/heightFullSize,
 * DerpCLI.cpp:212-214). Allocates the HBM-resident colour / disparity pyramid. May be called again with
 * another geometry: the frame slots start again from one, and every table cached for a level is dropped.
 * Fails, and changes nothing, while a derp_seq made on the context is open (derp_seq_destroy first): the
 * sequence's buffers and slots have the old geometry's sizes. */
int derp_set_pyramid(derp_ctx* ctx, int num_levels, const int* widths, const int* heights,
                     int width_full, int height_full);

/* ---- frame slots: several frames of one sequence resident on this GPU ------------------------
 * The reference keeps a sequence's frames on disk and loads one PyramidLevel at a time
 * (DerpCLI.cpp:220-323 frame loop); here each frame's colour / mask / background / result pyramid can
 * stay in HBM. derp_set_frame_slots (after derp_set_pyramid) allocates n_slots pyramids; uploads,
 * derp_process_*, derp_download_* and derp_dev_* act on the slot chosen by derp_select_frame (slot 0
 * initially). Working buffers and projection tables are shared by all slots. */
int derp_set_frame_slots(derp_ctx* ctx, int n_slots);
int derp_select_frame(derp_ctx* ctx, int slot);
int derp_frame_slots(const derp_ctx* ctx, int* n_slots, int* selected);

/* ---- host staging memory ----------------------------------------------------------------------
 * Page-locked host memory for the buffers handed to derp_upload_* / derp_download_*: the copies then run
 * at PCIe rate instead of through the runtime's pageable bounce buffers. Optional: any host pointer works.
 * derp_host_alloc returns NULL on failure (callers fall back to malloc). */
void* derp_host_alloc(size_t bytes);
void derp_host_free(void* p);
/* make the context's device current on the CALLING thread: a worker thread that allocates page-locked memory
 * (derp_host_alloc) or registers buffers for a context created on another thread calls this first */
int derp_bind_thread(derp_ctx* ctx);
/* page-lock / release memory the caller allocated itself (image buffers decoded before the runtime was up):
 * uploads from it then run at the PCIe rate. derp_host_register returns non-zero when the runtime refuses; the
 * memory stays usable, only slower. */
int derp_host_register(void* p, size_t bytes);
void derp_host_unregister(void* p);

/* ---- inputs (loadLevelImages, ImageUtil.h:79-94; DerpCLI.cpp:235-248,276-303) ------------ */
int derp_upload_color(derp_ctx* ctx, int level, int src, const uint16_t* bgr);
int derp_upload_foreground_mask(derp_ctx* ctx, int level, int src, const uint8_t* mask);
int derp_upload_background_disparity(derp_ctx* ctx, int level, int dst, const float* disp);
/* disparity of an already-finished level (resume from disk: DerpCLI.cpp:153-155,276-303) */
int derp_upload_disparity(derp_ctx* ctx, int level, int dst, const float* disp);

/* ---- pyramid builder: the step before the path (scripts/render/resize.py:51-85 resize_camera) --
 * cv2.resize(full-size frame, (w_L, h_L), INTER_AREA) into every level declared in derp_set_pyramid;
 * the frame crosses PCIe once and all its levels are produced in HBM. Masks: 8-bit image, resized,
 * then `> threshold` (resize.py passes 127; DerpCLI re-thresholds at 127, CvUtil.h:235-239). */
int derp_build_pyramid_color(derp_ctx* ctx, int src, const uint16_t* bgr, int w, int h);
int derp_build_pyramid_foreground_mask(derp_ctx* ctx, int src, const uint8_t* mask, int w, int h,
                                       int threshold);
int derp_build_pyramid_background_disparity(derp_ctx* ctx, int dst, const float* disp, int w, int h);
/* read a level back (what resize.py writes to level_<L>/<cam>/<frame>) */
int derp_download_level_color(derp_ctx* ctx, int level, int src, uint16_t* bgr);
int derp_download_level_mask(derp_ctx* ctx, int level, int src, uint8_t* mask01);
int derp_download_level_background(derp_ctx* ctx, int level, int dst, float* disp);
/* ---- raster inputs (host only; facebook360_dep_amd/csrc/derp_images.cpp over cli/image_codecs.h) ------------------
 * What `cv::imread(path, cv::IMREAD_UNCHANGED)` returns (CvUtil.cpp:23-29; scripts/render/resize.py:66-70) for the bytes
 * of a PNG / JPEG / TIFF / BMP / PNM file, the decoder chosen by signature: derp_image_info gives the geometry
 * (channels 1 / 3 / 4; bitdepth 8, 16 or 32 = float), derp_image_decode fills `out` with w * h * channels samples in
 * OpenCV's order (B, G, R [, A]) — uint16 for bitdepth 8 (widened, not scaled) and 16, float for 32. 0 / non-zero;
 * derp_image_last_error() holds the reason ("unsupported JPEG colour space (CMYK / YCCK)", ...), per thread. */
int derp_image_info(const void* bytes, size_t n, int* w, int* h, int* channels, int* bitdepth);
int derp_image_decode(const void* bytes, size_t n, void* out, size_t out_bytes);
const char* derp_image_last_error(void);
/* What cv::imwrite(".jpg", 8-bit image) writes with its defaults (scripts/render/resize.py:82-85 on a JPEG source
 * directory): baseline JPEG, 4:2:0, the standard tables, `quality` as libjpeg scales it (OpenCV's default: 95) — libjpeg's
 * compressor restated, byte-identical to libjpeg-turbo's output. pixels: w * h * channels bytes, gray or B, G, R.
 * out == NULL: only *size is set (the bytes needed); otherwise 0 and *size bytes written, non-zero if cap is too small. */
int derp_jpeg_encode(const void* pixels, int w, int h, int channels, int quality, void* out, size_t cap, size_t* size);

/* one image: kind 0 = BGR u16 x3, 1 = u8 x1, 2 = f32 x1, 3 = BGR f32 x3 (cv_util::resizeImage<Vec3f>,
 * CvUtil.h:139-147 — the colour guide of UpsampleDisparity.cpp:117). Shrinking only. */
int derp_resize_area(derp_ctx* ctx, int kind, const void* src, int w, int h, void* dst, int dw, int dh);

/* background_subtraction::generateForegroundMask<Vec3w, Vec3f> for one camera
 * (source/render/BackgroundSubtractionUtil.h:20-60; GenerateForegroundMasks.cpp:65-130): Gaussian blur
 * (radius 0..3) of template and frame, ||template - frame||_2 > threshold on [0,1] colours, k x k
 * morphological close. Both images BGR u16 at the same size; mask01 gets {0,1}. */
int derp_generate_foreground_mask(derp_ctx* ctx, const uint16_t* template_bgr, const uint16_t* frame_bgr,
                                  int w, int h, int blur_radius, float threshold,
                                  int morph_closing_size, uint8_t* mask01);

/* ---- the hot path ------------------------------------------------------------------------ */
/* One (frame, level): generateFovMasks (DerpUtil.cpp:259-276) + PyramidLevel ctor's
 * computeVariances (PyramidLevel.h:232-247) + precomputeProjections (Derp.cpp:955-976) +
 * upsampleDisparities from level+1 when level < num_levels-1 (UpsampleDisparityLib.cpp:149-182)
 * + processLevel (Derp.cpp:1005-1034) minus file output. */
int derp_process_level(derp_ctx* ctx, int level);
/* DerpCLI main's level loop for one frame (DerpCLI.cpp:220-323), level_start >= level_end. */
int derp_process_pyramid(derp_ctx* ctx, int level_start, int level_end);
int derp_synchronize(derp_ctx* ctx);

/* ---- outputs (PyramidLevel::saveResults, PyramidLevel.h:487-529) -------------------------- */
int derp_download_disparity(derp_ctx* ctx, int level, int dst, float* disparity);
/* cost / confidence of the level processed last (debug images, PyramidLevel.h:418-485) */
int derp_download_cost(derp_ctx* ctx, int dst, float* cost, float* confidence);

/* ---- stage-level entry points (Derp.h:64-133), used by the parity tests ------------------ */
int derp_level_begin(derp_ctx* ctx, int level);     /* masks, variances, warp tables, upsample hand-off */
int derp_stage_reproject_colors(derp_ctx* ctx);     /* reprojectColors,        Derp.cpp:978-1003 */
int derp_stage_brute_force(derp_ctx* ctx);          /* preprocessLevel,        Derp.cpp:826-842  */
int derp_stage_random_proposals(derp_ctx* ctx);     /* randomProposals,        Derp.cpp:844-873  */
int derp_stage_ping_pong(derp_ctx* ctx);            /* pingPongPropagation,    Derp.cpp:540-551  */
int derp_stage_mismatches(derp_ctx* ctx);           /* handleDisparityMismatches, Derp.cpp:722-748 */
int derp_stage_bilateral_filter(derp_ctx* ctx);     /* bilateralFilter,        Derp.cpp:875-902  */
int derp_stage_median_filter(derp_ctx* ctx);        /* medianFilter,           Derp.cpp:904-920  */
int derp_stage_mask_fov(derp_ctx* ctx);             /* maskFov,                Derp.cpp:940-951  */
int derp_level_end(derp_ctx* ctx);                  /* publish the level's disparity to the pyramid */
/* set / read the working disparity of the current level (between stages). After derp_process_level the level's result is
 * in the pyramid (derp_download_disparity): the loop's last stage writes it there, and the working disparity keeps what that
 * stage read */
int derp_set_level_disparity(derp_ctx* ctx, int dst, const float* disp);
int derp_get_level_disparity(derp_ctx* ctx, int dst, float* disp);
/* computeCost (Derp.cpp:104-226) of a caller-supplied disparity map at every interior pixel */
int derp_cost_map(derp_ctx* ctx, int dst, const float* disp, float* cost, float* confidence);
/* tables of the current level: which = 0 projWarp (float2), 2 projColor (u16x3), 3 projColorBias
 * (u16x3), 4 variance of src (float), 5 fov mask of dst (u8; src ignored), 6 / 7 projColor / projColorBias as stored:
 * the padded (H + 4) x (W + 4) plane of u16x4 texels with its replicated 2-texel ring, 8 the table's blank-tile flags
 * (u8 per 32 x 32 tile, row-major; 0 = no source pixel maps into the tile), 9 the own colour bias of src (u16x3; dst
 * ignored), 10 the random proposals' engine states of dst (u32; src ignored; defined at the gated-in interior pixels only,
 * after derp_stage_random_proposals) */
int derp_debug_download(derp_ctx* ctx, int dst, int src, int which, void* out);
/* the cost kernels' own fp64 atan2 (FTHETA branch of Camera::cameraToSensor, Camera.h:306-309): out[i] =
 * atan2(y[i], x[i]) for y >= 0, as the device routine computes it — so that a test can hold it against libm */
int derp_debug_atan2_ypos(derp_ctx* ctx, const double* y, const double* x, double* out, size_t n);
/* the cost kernels' fp64 primitives on the device: out[i] = op 0 sqrt_lean(a[i]), 1 sqrt(a[i]), 2 div_plain(a[i], b[i]),
 * 3 a[i] / b[i] (the compiler's division); b may be null for ops 0 and 1 */
int derp_debug_fp64(derp_ctx* ctx, int op, const double* a, const double* b, double* out, size_t n);
/* Camera::sees (Camera.h:184-190) of source camera `src`, as the cost kernels evaluate it (normalised camera, res 1):
 * out[6 i .. 6 i + 5] = (vis, pix.x, pix.y) of the ping-pong / brute-force variant, then of the random-proposal variant,
 * for the rig points xyz[3 i .. 3 i + 2]; pix is NaN where the point lies outside the FOV cone */
int derp_debug_sees(derp_ctx* ctx, int src, const double* xyz, size_t n, double* out);
/* the filters' expf on the device: out[i] = mode 0 the full routine, 1 the form with the single range test that the joint
 * bilateral filter's fast tap uses, which equals the full one for x[i] in [-inf, -0]; 2 not expf at all but the cost
 * kernels' two-instruction roundf (round_half_away_pos), which equals roundf for x[i] in (-0.5, 2^23) */
int derp_debug_expf(derp_ctx* ctx, int mode, const float* x, float* out, size_t n);

/* developer builds (-DDERP_BLOCK_TRACE=1, tools/block_trace.py): {start, end} in 10 ns ticks of every block of the last
 * random-proposal ("random_proposals") / ping-pong ("ping_pong") launch of `level`, out[(y * grid_x + x) * 2 ..]; with
 * out = NULL or too small a capacity (in uint64s) only the grid is returned. Fails in the shipped library. */
int derp_debug_block_trace(derp_ctx* ctx, const char* stage, int level, uint64_t* out, size_t capacity, int* grid_x, int* grid_y);
/* what the frames of the level opened last share: out[0 .. 3] = {the level (-1: none), the destination batch that fits
 * the table budget, 1 if inverse warps are stored, how many times a level was opened since derp_create}. A level is
 * opened once per pass over it: by its first frame, and by every direct derp_process_level / derp_level_begin. */
int derp_debug_level_plan(derp_ctx* ctx, int32_t* out);

/* mismatch mask of the level processed last (dstMismatchedDisparityMask, PyramidLevel.h:332-338) */
int derp_download_mismatch_mask(derp_ctx* ctx, int dst, uint8_t* out);

/* ---- the sibling binaries' kernels ------------------------------------------------------- */
/* layerDisparities (LayerDisparities.cpp:45-55): fg over bg where fg > 0, x255, saturate to 8 bit */
int derp_layer_disparities(derp_ctx* ctx, const float* foreground, const float* background, size_t n,
                           uint8_t* out);
/* ---- rephotography score ---------------------------------------------------- */
/* rephoto_util::computeSSIM (RephotographyUtil.h:38-86) on two interleaved BGR float images in
 * [0, 1]; alpha / beta / gamma must each be 0 or 1 (computeScoreMap, :110-123: MSSIM = 1,1,1 and
 * NCC = 0,0,1). score = [h][w][3] float. */
int derp_ssim(derp_ctx* ctx, const float* x_bgr, const float* y_bgr, int w, int h, int blur_radius, float alpha,
              float beta, float gamma, float* score_bgr);
/* rephoto_util::averageScore (RephotographyUtil.h:88-108): per-channel mean of the score over
 * mask != 0 and not-NaN pixels, accumulated in double (host side, row-major order). */
int derp_average_score(const float* score_bgr, const uint8_t* mask, int w, int h, double* avg_bgr3);
/* Camera-space stand-in for ComputeRephotographyErrors.cpp:69-189 `generateCubemaps(removeOne(i))`:
 * what the other source cameras' colour + disparity say camera `target` sees (point z-buffer + one
 * bilinear fetch; no OpenGL). colors[s] = BGR u16 [h][w][3], disparities[s] = f32 [h][w] for every
 * source camera s. out = BGRA float [h][w][4], alpha = covered. */
int derp_rephotograph(derp_ctx* ctx, int target, const uint16_t* const* colors, const float* const* disparities,
                      int w, int h, float* out_bgra);
/* the same in two steps, for rendering several targets from one upload (every entry must be non-NULL) */
int derp_rephotograph_upload(derp_ctx* ctx, const uint16_t* const* colors, const float* const* disparities, int w,
                             int h);
int derp_rephotograph_render(derp_ctx* ctx, int target, float* out_bgra);
/* The reference's renderer for that score, without OpenGL: CanopyScene::cubemap
 * (source/render/CanopyScene.cpp:198-374) of the cameras include[s] != 0 of the last
 * derp_rephotograph_upload, seen from `centre` (rig space, 3 doubles) — disparity meshes, depth test, stretch /
 * cone weights, soft-max accumulation, un-premultiply — as six edge x edge faces (+X -X +Y -Y +Z -Z) stacked
 * top to bottom: out = BGRA float [6 * edge][edge][4], alpha in {0, 1}. generateCubemaps(removeOne(i)) =
 * include everything but i; the reference side = include only i (ComputeRephotographyErrors.cpp:140-145). */
int derp_canopy_cubemap(derp_ctx* ctx, const uint8_t* include, const double* centre, int edge, float* out_bgra);
/* SimpleMeshRenderer's renderer without OpenGL (source/render/SimpleMeshRenderer.cpp, CanopyScene.cpp:15-69, 72-266,
 * 288-475, DisparityColor.h:18-57): the engine of derp_canopy_cubemap for any view. Conventions of this group:
 * colour textures float BGRA [h][w][4] (a loaded cv::Vec4f image; stored as GL_RGBA16), disparities f32, every
 * camera with its own texture and disparity size; outputs BGRA float with NaN where nothing was rendered.
 * derp_render_upload: the scene (CanopyScene::CanopyScene). colors may be NULL (no colour; disparity formats only).
 * derp_render: one image of the cameras include[s] != 0 (include NULL = all) per derp_render_params:
 *   CUBE      CanopyScene::cubemap(height): six height x height faces stacked, out [6 h][h][4];
 *   EQUIRECT  CanopyScene::equirect(height): out [h][2 h][4], row 0 = north;
 *   SNAPSHOT  the snapshot of SimpleMeshRenderer.cpp:386-405 (frustum of horizontal_fov, posForwardUp): [h][w][4].
 * derp_render_format: a whole SimpleMeshRenderer --format (cubecolor cubedisp eqrcolor eqrdisp lr180 snapcolor
 *   snapdisp tb3dof tbstereo) with its stacks and generate() compositing (--background: background [out_h][out_w][4]
 *   or NULL; --background_equirect: [eq_h][eq_w][4] or NULL); derp_render_format_size gives out_w x out_h.
 * derp_render_vertices: camera `cam`'s mesh vertices after canopyVS's stereo stage for half-IPD `ipd` (0 = none),
 *   xyz + 0 [dh][dw][4] (the test hook for the device's transcendental functions). */
enum { DERP_RENDER_CUBE = 0, DERP_RENDER_EQUIRECT = 1, DERP_RENDER_SNAPSHOT = 2 };
enum { DERP_WEIGHT_SVD = 0, DERP_WEIGHT_MINOR = 1 };
typedef struct {
  int32_t kind;            /* DERP_RENDER_* */
  int32_t width, height;   /* snapshot viewport; cube edge and equirect height = height */
  double position[3];      /* --position (rig space) */
  double forward[3], up[3];/* --forward, --up (snapshot and the background equirect's ray) */
  double horizontal_fov;   /* --horizontal_fov, degrees */
  float ipd;               /* canopyVS ipdm: +0.032 left eye, -0.032 right eye, 0 mono */
  int32_t alpha_blend;     /* accumulateFS alphaBlend (!--ignore_alpha_blend) */
  int32_t disparity_color; /* 0: the colour textures, 1: the disparity colours seen from position */
  int32_t weight;          /* DERP_WEIGHT_SVD (SimpleMeshRenderer) or DERP_WEIGHT_MINOR (rephotography) */
  int32_t zero_nans;       /* ComputeRephotographyErrors' zeroOutNans after un-premultiplying */
} derp_render_params;
void derp_render_params_default(derp_render_params* p);
int derp_render_upload(derp_ctx* ctx, const float* const* colors_bgra, const int* color_w, const int* color_h,
                       const float* const* disparities, const int* disp_w, const int* disp_h);
int derp_render(derp_ctx* ctx, const derp_render_params* p, const uint8_t* include, float* out_bgra);
int derp_render_format_size(const char* format, int width, int height, int* out_w, int* out_h);
int derp_render_format(derp_ctx* ctx, const char* format, const derp_render_params* p, const float* background,
                       const float* background_equirect, int eq_w, int eq_h, float* out_bgra);
int derp_render_vertices(derp_ctx* ctx, int cam, float ipd, float* out_xyzw);
/* MeshStreamRenderer: the fused mesh stream (ConvertToBinary's .vtx / .idx / .rgba) rendered as the viewer renders it,
 * without OpenGL — RigScene's mesh path (source/render/RigScene.cpp: cameraMeshVS :195-218, cameraFS :244-259,
 * createDirection :869-885, renderSubframe :920-974, exponentialFS + updateAccumulation :281-292, 1009-1020, resolveFS
 * :294-307, render :1071-1098) with indexed triangles, a near plane at 0.1 m that cuts a triangle instead of dropping
 * it, GL_LESS with the earlier triangle kept on ties. Cameras = the destinations of derp_create as the rig file holds
 * them (<rig>_fused.json: already at the colour's size). Outputs follow derp_render: BGRA float, NaN where nothing was
 * rendered, the same CUBE / EQUIRECT / SNAPSHOT views and stacking.
 * derp_stream_upload: camera `cam`'s mesh and colour of one frame: vtx = `vertices` x (a, b, c) floats, idx = `indices`
 *   uint32 (three per triangle), rgba = [h][w][4] sRGB bytes. Refused on the host, before anything reaches the device:
 *   indices not a multiple of 3, an index >= vertices (every index is read), (w, h) not the camera's resolution, a
 *   null pointer with a non-zero count. A refused call leaves the scene as it was. An empty mesh renders nothing.
 * derp_stream_clear: forgets every camera's upload.
 * derp_stream_render: one image of the uploaded cameras include[s] != 0 (include NULL = all) for the view in p (kind,
 *   width, height, position, forward, up, horizontal_fov, zero_nans; ipd and disparity_color must be 0; alpha_blend and
 *   weight are not used: RigScene has one weight), rgb multiplied by `fade` (resolveFS).
 * derp_stream_vertices: the vertex stage alone for p's view (`face` of the cube; ignored for a snapshot): clip
 *   coordinates [vertices][4] (a test hook).
 * derp_stream_srgb_table: host only; the sRGB -> linear value of every code, as the colour texture is decoded. */
int derp_stream_upload(derp_ctx* ctx, int cam, const float* vtx, size_t vertices, const uint32_t* idx, size_t indices,
                       const uint8_t* rgba, int w, int h);
int derp_stream_clear(derp_ctx* ctx);
int derp_stream_render(derp_ctx* ctx, const derp_render_params* p, const uint8_t* include, float fade, float* out_bgra);
int derp_stream_vertices(derp_ctx* ctx, int cam, const derp_render_params* p, int face, float* out_clip_xyzw);
void derp_stream_srgb_table(float* out256);
/* ---- conversion tools at the depth stage's inputs and outputs (source/conversion) -------------------------------
 * The cameras are the destinations of derp_create (a --cameras-filtered rig is passed as both src and dst); `cam`
 * indexes them. Every call rescales the rig camera as the file holds it, Camera::rescale (Camera.cpp:217-223), to the
 * image size it is given. No limit on the number of cameras beyond derp_create's.
 * derp_export_points: getPoints (ExportPointCloud.cpp:67-137) for one camera. color_bgr = float [h][w][3] in 0..1,
 *   already at the disparity's size. Pixels outside the image circle are dropped; depth > max_depth is dropped (clip)
 *   or pulled back to max_depth; NaN / zero disparities are kept as IEEE arithmetic leaves them. Survivors come in
 *   row-major pixel order, six floats each: x y z r g b. subsample > 1 keeps the pixels whose hash of (cam, pixel
 *   index) is 0 modulo subsample: one in `subsample`, the same ones on every run (the reference's rand() from racing
 *   threads is not reproducible). *count = the number of points; count > cap is an error that still reports it. */
int derp_export_points(derp_ctx* ctx, int cam, const float* disparity, int w, int h, const float* color_bgr,
                       double max_depth, int clip, int subsample, float* out_xyzrgb, size_t cap, size_t* count);
/* projectPointsToCameras (ImportPointCloud.cpp:63-123): derp_points_begin sets one image size per camera and zeroes the
 * images; derp_points_splat projects n points (rows of x y z) into every camera that sees them and keeps the largest
 * 1 / |p| per pixel (|p| outside [min_depth, max_depth] counts as infinitely far), accumulating over any number of
 * calls, in any chunking, to the same bits; it returns once the chunk is on the device, while its kernel runs.
 * derp_points_download reads one camera's image [h][w] back. */
int derp_points_begin(derp_ctx* ctx, const int* widths, const int* heights);
int derp_points_splat(derp_ctx* ctx, const double* xyz, size_t n, double min_depth, double max_depth);
int derp_points_download(derp_ctx* ctx, int cam, float* disparity);
/* ProjectEquirectsToCameras.cpp:94-125 with image_util::worldToEquirect (ImageUtil.cpp:127-140): out [h][w] = the
 * equirect mask (u8, non-zero = set) where the camera's pixel lands when projected at `depth` metres; {0,1}. */
int derp_project_equirect_mask(derp_ctx* ctx, int cam, const uint8_t* eqr, int eqr_w, int eqr_h, int w, int h,
                               double depth, uint8_t* out);
/* ---- camera meshes (source/mesh_stream/ConvertToBinary.cpp:150-245) ----------------------------------------------
 * derp_mesh_build: convertDepth up to applyMaskToVertexesAndFaces for camera `cam` of derp_create's destinations, on
 *   the device: depth = 1.0f / disparity [h][w]; depth_scale < 1 resizes it with INTER_NEAREST (cv::resize with
 *   cv::Size(), :166-169); mesh_util::getVertexesEquiError (MeshUtil.h:317-341); mesh_util::getFaces(wrap = false,
 *   isRigCoordinates = false, tear_ratio) with getTriangleMask / addTriangle (:167-296); the vertex mask "depth is not
 *   NaN", AND-ed with `mask` (u8 [mask_h][mask_w], non-zero = keep, INTER_NEAREST to the depth's size; NULL: none);
 *   mesh_util::applyMaskToVertexesAndFaces (:345-405). `resolution` (double[2], NULL: as the rig file holds it) is
 *   what resizeRig hands Camera::rescale (:318-339). Camera::getScalarFocal's focal.x == -focal.y is checked here.
 *   The context holds one mesh: the one built last.
 * derp_mesh_counts: vertices and faces of the mesh (after a simplify: of its result), and the faces getFaces
 *   made before the mask removed any (the "Removed N of M faces" line, :191-198).
 * derp_mesh_setup: MeshSimplifier::computeInitialQuadrics (MeshSimplifier.cpp:182-239) of the built mesh on the
 *   device: face_planes [faces][4] (Face::normal and -normal.p0), edge_costs [faces][3] (Face::cost), vertex_quadrics
 *   [vertices][10] (Vertex::q, the distinct entries q00 q01 q02 q03 q11 q12 q13 q22 q23 q33). NULL outputs are skipped.
 * derp_mesh_simplify: MeshSimplifier(vertexes, faces, equi_error, threads = 1).simplify(num_faces_out, strictness,
 *   remove_boundary_edges) (:456-562) of the built mesh: the set-up on the device (host_setup = 0) or on the host, the
 *   collapse loop on the host (derp_mesh_simplify_host). stats (int[2], may be NULL): passes of the loop, and how it
 *   ended (DERP_MESH_EXIT_*).
 * derp_mesh_simplify_parallel: a second simplifier of the built mesh, set-up and loop on the device, with the same
 *   preconditions, refusals and stats. The reference's: the set-up, computeError and its target, haveNormalsFlipped
 *   against the set-up's face normals, the boundary vertices of identifyBoundaries (found once), commonFaces,
 *   updateCosts, createFinalMesh. Not the reference's: what a pass collapses. Feasible edges = those the reference
 *   would not bar (equal boundary flags, no boundary vertex unless remove_boundary_edges, a cost that is no NaN, no
 *   flipped normal on either side); the threshold is getThreshold's rank int(strictness * float(n - 1)) over the n
 *   feasible costs alone; of the feasible edges at or under it, those with the smallest (cost, face, edge) on every
 *   alive face of their two vertices are collapsed together, in that order while the faces left exceed
 *   num_faces_out. The loop ends when they do not (DERP_MESH_EXIT_BUDGET) or no edge is feasible
 *   (DERP_MESH_EXIT_NO_CANDIDATES). Results are the same from run to run, and differ from derp_mesh_simplify's.
 * derp_mesh_parallel_pass: what pass `pass` (0 .. passes - 1) of the last derp_mesh_simplify_parallel saw.
 * derp_mesh_download_f64 / derp_mesh_download: MeshSimplifier::getVertexes / getFaces, or the built mesh when it was
 *   not simplified; the second as mesh_util::writeDepth lays the files out (MeshUtil.h:72-89): float32 x y z rows and
 *   uint32 index triples, with z < 0 raised to FLT_MIN first when clamp_negative_z (ConvertToBinary.cpp:211-217).
 * derp_mesh_build_equirect: CreateObjFromDisparityEquirect's mesh (source/conversion/CreateObjFromDisparityEquirect.cpp)
 *   of a disparity equirect [h][w], on the device: mesh_util::getVertexesEquirect and mesh_util::getFaces(wrap = true,
 *   isRigCoordinates = true, tear_ratio) (MeshUtil.h:264-314). Vertex y * w + x is fmin(max_depth, 1.0f / disparity)
 *   (float: a disparity of 0 or NaN gives max_depth, a negative one a negative depth) times the unit direction of the
 *   pixel's centre, in rig coordinates; getTriangleMask reads the vertices' norms; after the grid's faces come two faces
 *   per row that link column w - 1 to column 0, with no tear test. All w * h vertices stay, used or not, so
 *   faces_unmasked == faces. The cameras of the context are not read. It leaves the context as derp_mesh_build does:
 *   derp_mesh_counts / _setup / _simplify / _simplify_parallel / _parallel_pass / _download* work on the mesh, with
 *   equi_error = 0. Refused: null pointers, w < 2 or h < 2, w * h >= 2^31, a tear_ratio or max_depth that is NaN. */
enum {
  DERP_MESH_EXIT_BUDGET = 0,
  DERP_MESH_EXIT_INFINITE_THRESHOLD = 1,
  DERP_MESH_EXIT_STUCK = 2,
  DERP_MESH_EXIT_NO_CANDIDATES = 3
};
typedef struct derp_mesh_pass {
  long long faces;     /* alive before the pass */
  long long feasible;  /* feasible edges */
  long long winners;   /* candidates that held every face they touch */
  long long applied;   /* winners collapsed (all of them except in a pass cut at the budget) */
  long long deleted;   /* faces the pass deleted */
  double threshold;
} derp_mesh_pass;
int derp_mesh_build(derp_ctx* ctx, int cam, const float* disparity, int w, int h, const double* resolution,
                    double depth_scale, const uint8_t* mask, int mask_w, int mask_h, float tear_ratio);
int derp_mesh_build_equirect(derp_ctx* ctx, const float* disparity, int w, int h, float max_depth, float tear_ratio);
int derp_mesh_counts(derp_ctx* ctx, size_t* vertices, size_t* faces, size_t* faces_unmasked);
int derp_mesh_setup(derp_ctx* ctx, int equi_error, double* face_planes, double* edge_costs, double* vertex_quadrics);
int derp_mesh_simplify(derp_ctx* ctx, int num_faces_out, float strictness, int remove_boundary_edges, int equi_error,
                       int host_setup, int* stats);
int derp_mesh_simplify_parallel(derp_ctx* ctx, int num_faces_out, float strictness, int remove_boundary_edges,
                                int equi_error, int* stats);
int derp_mesh_parallel_pass(derp_ctx* ctx, int pass, derp_mesh_pass* out);
int derp_mesh_download_f64(derp_ctx* ctx, double* vertices, int32_t* faces);
int derp_mesh_download(derp_ctx* ctx, int clamp_negative_z, float* vtx, uint32_t* idx);
/* ---- GeometricConsistency (source/render/GeometricConsistency.cpp): plane-sweep depth with cross-camera cleaning ----
 * The cameras are the destinations of derp_create (the whole rig passed as both src and dst, not normalised); `cam`,
 * `dst` and `src` index them. The reference's OpenGL reprojection (ReprojectionGpuUtil.h reproject<T>, :208-214) is
 * replaced by a defined sampling rule; everything after it is the reference's arithmetic.
 * derp_gc_upload: loadImages + downscale + computeReference (:158-163, :324-331, :338): per camera one full-size BGRA
 *   u16 image [full_h][full_w][4] (alpha 65535 where the file has none), area-resized to the small size (at least
 *   3 x 3, the size Camera::rescale is given) and converted to int16 with 32767 / 65535. The result is both the
 *   destination's reference and the source's texture. derp_gc_download_image reads one back, [h][w][4].
 * derp_gc_slices: sliceCount of computeDepth (:186-192) for `dst` and its slice disparities (:126-128; null: the count
 *   alone). Refuses a rig whose mean camera distance from the origin is 1 m or more, and a count below 1.
 * derp_gc_slice_count: the same count on the host, with no context and no device, for a rig as the file holds it and
 *   the destination's small size; a refusal leaves its text in derp_last_error(NULL).
 * derp_gc_set_clean: the clean depth of every camera [h][w] at the small sizes, for sweeps and stages with use_clean
 *   (null: none).
 * derp_gc_sweep: computeDepth + winnerTakesAll (:132-258) of one destination -> depth [h][w], NaN on the outermost
 *   rows and columns and where no slice has a cost. split: parts the slice range is swept in (grid dimension), 0 = the
 *   library's choice; the result does not depend on it.
 * derp_gc_clean: cleanDepth / isPointBad (:260-310) over caller-supplied depth maps of any origin, one [h[i]][w[i]]
 *   per camera, cameras rescaled to those sizes -> out[i], NaN where another camera's map contradicts the depth. Needs
 *   no derp_gc_upload.
 * derp_gc_run: processFrame (:333-384) of the uploaded frame; derp_gc_result reads what the tool dumps: DERP_GC_IFFY
 *   (<id>_iffy), DERP_GC_CLEAN (<id>_<pass>_clean), DERP_GC_DEPTH (<id>_<pass>), and DERP_GC_FINAL, the depths after
 *   the last pass (after restoreCleanDepth when keep_clean).
 * derp_gc_stage: for one (dst, src, slice): the int16 sample image (`image`, :208 + occlusion :212-226), `average` and
 *   `averageOfSq` (:229-236), each [h][w][4], and the slice's cost plane over all sources (:251). Null outputs are
 *   skipped. The outermost pixels are computed like the others (the sweep blanks them at the end). */
enum { DERP_GC_IFFY = 0, DERP_GC_CLEAN = 1, DERP_GC_DEPTH = 2, DERP_GC_FINAL = 3 };
int derp_gc_upload(derp_ctx* ctx, const uint16_t* const* bgra, const int* full_w, const int* full_h, const int* small_w,
                   const int* small_h);
int derp_gc_download_image(derp_ctx* ctx, int cam, int16_t* out_bgra);
int derp_gc_slices(derp_ctx* ctx, int dst, double disparity_step, int* count, float* disparities, int cap);
int derp_gc_slice_count(const derp_camera_desc* cams, int n_cams, int dst, int small_w, int small_h,
                        double disparity_step, int* count);
int derp_gc_set_clean(derp_ctx* ctx, const float* const* clean);
int derp_gc_sweep(derp_ctx* ctx, int dst, double disparity_step, int use_clean, double agree_fraction, int split,
                  float* depth);
int derp_gc_clean(derp_ctx* ctx, const float* const* depths, const int* w, const int* h, double agree_fraction,
                  float* const* out);
int derp_gc_run(derp_ctx* ctx, double disparity_step, double agree_fraction, int pass_count, int keep_clean);
int derp_gc_result(derp_ctx* ctx, int kind, int pass, int cam, float* out);
int derp_gc_stage(derp_ctx* ctx, int dst, int src, int slice, double disparity_step, int use_clean,
                  double agree_fraction, int16_t* sample, int16_t* average, int16_t* average_of_sq, float* cost);
/* ---- The rig preview tools (source/render/GenerateCameraOverlaps.cpp, GenerateEquirect.cpp): every camera projected
 * into a destination camera, or into one equirect of the whole rig, over a series of depths ----
 * The cameras are the destinations of derp_create (the whole rig, not normalised), as in the conversion group.
 * derp_sweep_upload: loadScaledImages<cv::Vec4f> + Camera::rescale(resolution * scale) (GenerateCameraOverlaps.cpp:135-145,
 *   GenerateEquirect.cpp:251-259): per camera one float BGRA image [img_h][img_w][4] at its scaled size (alpha 1 where the
 *   file has none) and the camera's resolution {x, y} as doubles, which need not be whole or equal the image's size.
 * derp_sweep_overlaps: projectSrcsToDst (GenerateCameraOverlaps.cpp:54-83) of destination `dst` for each of `n`
 *   disparities -> out [n][img_h][img_w][4], float (DERP_SWEEP_FLOAT; NaN where no camera sees the point) or the 8-bit
 *   values of `255.0f * image` (DERP_SWEEP_U8; NaN -> 0).
 * derp_sweep_equirect_bounds: createCroppedEquirect's first loop (GenerateEquirect.cpp:139-156) over the W x H equirect
 *   at `depth` -> bounds = {minX, maxX, minY, maxY}; {W, 0, H, 0} where no camera sees anything.
 * derp_sweep_equirect: createEquirect / createCroppedEquirect + getPixelColor (GenerateEquirect.cpp:79-175) for each of
 *   `n` depths -> out [n][out_h][out_w][4]. window NULL: the whole equirect (out_w = W, out_h = H); otherwise the four
 *   bounds, sampled at x * (maxX - minX) / out_w + minX and likewise in y. background_bgra: where no camera sees the point.
 * Host only, no context and no device; a refusal leaves its text in derp_last_error(NULL):
 * derp_sweep_overlap_disparities: probeDisparity (ImageUtil.cpp:100-107) of dumpOverlaps
 *   (GenerateCameraOverlaps.cpp:100-120) and the files' stems int(depth * 100) (stems may be NULL). One depth: the
 *   farthest (the reference divides 0 by 0).
 * derp_sweep_equirect_depths: the depth of index i of GenerateEquirect.cpp:264-272 and its stem (saveImage, :74-75).
 * derp_sweep_crop_size: newWidth of GenerateEquirect.cpp:158-159; refuses an empty box (the reference divides by zero).
 * derp_rig_center: centerRig (GenerateEquirect.cpp:177-231, transformRig of source/rig/RigTransform.h:73-97) for the
 *   camera `index` -> out_cams[n], with forward / up / right re-unitarised as Camera::setRotation leaves them. */
enum { DERP_SWEEP_FLOAT = 0, DERP_SWEEP_U8 = 1 };
int derp_sweep_upload(derp_ctx* ctx, const float* const* bgra, const int* img_w, const int* img_h, const double* cam_res_xy);
int derp_sweep_overlaps(derp_ctx* ctx, int dst, const float* disparities, int n, int out_kind, void* out);
int derp_sweep_equirect_bounds(derp_ctx* ctx, int W, int H, float depth, int* bounds);
int derp_sweep_equirect(derp_ctx* ctx, int W, int H, const int* window, int out_w, int out_h, const float* depths, int n,
                        const float* background_bgra, int out_kind, void* out);
int derp_sweep_overlap_disparities(int num_depths, uint64_t min_depth_m, uint64_t max_depth_m, float* disparities,
                                   int* stems);
int derp_sweep_equirect_depths(int num_depths, double depth_min, double depth_max, float* depths, int* stems);
int derp_sweep_crop_size(int height, const int* bounds, int* new_width);
int derp_rig_center(const derp_camera_desc* cams, int n, int index, derp_camera_desc* out_cams);
/* ---- RigAnalyzer (source/rig/RigAnalyzer.cpp): how many cameras of the rig see each point of a point set, and the rig
 * construction and editing that goes with it ----
 * The cameras are the destinations of derp_create (the whole rig, in their own pixel units); each is asked with
 * Camera::sees (Camera.h:184-190). At most 255 cameras (the counts are 8-bit); the depth path's camera cap does not apply.
 * derp_coverage_directions: the sweep of main() (:567-577): points distances[i] * units[j] -> hist [nd][S + 1], the number
 *   of directions seen by exactly k cameras at each distance, and counts [nd][n] (may be NULL).
 * derp_coverage_equirect: saveEquirect (:376-438) at 360 x 180 degrees times pixels_per_degree (the reference: 5) ->
 *   counts [H][W]; min_timing [H][W] (may be NULL): the smallest |t_i - t_j| over the pairs of cameras that see the pixel,
 *   t = float(pix.y / resolution.y), 1 with fewer than two; stats (may be NULL) = {holes, maxMin, aveMin} summed on the
 *   host in row-major order, aveMin being the sum, not the mean.
 * derp_coverage_camera: saveCamera (:346-374): the pixels of camera `cam` at its own resolution, at `distance`; 0 outside
 *   the image circle -> counts [h][w].
 * derp_coverage_cross_section: saveCrossSection (:440-460) with kDim = dim (the reference: 400) -> counts [dim][dim].
 * Host only, no context and no device; a refusal leaves its text in derp_last_error(NULL):
 * derp_rig_fibonacci_units: getFibonacciUnits + discardPoles (:68-94) -> out_xyz [count][3], of which *kept are filled.
 * derp_rig_coverage_distances: the 20 distances of :562-565.
 * derp_rig_euler_matrix: rotationMatrixFromEulers (:96-101), radians -> row-major 3 x 3.
 * derp_rig_align_z_matrix: --rotate_cam_z's rotation (:505-510) for a camera at `position`.
 * derp_rig_from_eulers: makeRigFromEulers (:103-131), degrees, ids cam0, cam1, ...
 * derp_rig_arrangement: makeNamedArrangement (:240-259, tables :157-238) -> out (room for DERP_RIG_ARRANGEMENT_MAX), *n.
 * derp_rig_revolve: revolveRig (:133-155), radians -> out [m][n]; ids gain _<frame> when m > 1.
 * derp_rig_rotate: position = m * position, setRotation(m * forward, m * up, m * right) (:511-516, :532-535).
 * derp_rig_perturb: std::srand(seed) + Camera::perturbCameras (Camera.cpp:260-280), in place.
 * derp_rig_scale: --scale_rig, --radius, --scale_resolution (:538-555), in place; 1, 0, 1 change nothing. */
enum { DERP_RIG_COVERAGE_DISTANCES = 20, DERP_RIG_ARRANGEMENT_MAX = 24 };
int derp_coverage_directions(derp_ctx* ctx, const double* units_xyz, int n, const double* distances, int nd, int32_t* hist,
                             uint8_t* counts);
int derp_coverage_equirect(derp_ctx* ctx, int pixels_per_degree, double distance, uint8_t* counts, float* min_timing,
                           double* stats);
int derp_coverage_camera(derp_ctx* ctx, int cam, double distance, uint8_t* counts);
int derp_coverage_cross_section(derp_ctx* ctx, int dim, uint8_t* counts);
int derp_rig_fibonacci_units(int count, double discard_poles_deg, double* out_xyz, int* kept);
int derp_rig_coverage_distances(double min_distance, double* out);
int derp_rig_euler_matrix(const double* euler_rad, int xyz, double* m9);
int derp_rig_align_z_matrix(const double* position, double* m9);
int derp_rig_from_eulers(const derp_camera_desc* model, const double* eulers_deg, int n, int xyz, derp_camera_desc* out);
int derp_rig_arrangement(const char* name, const derp_camera_desc* model, double custom, derp_camera_desc* out, int* n);
int derp_rig_revolve(const derp_camera_desc* cams, int n, const double* eulers, int m, derp_camera_desc* out);
int derp_rig_rotate(const derp_camera_desc* cams, int n, const double* m9, derp_camera_desc* out);
int derp_rig_perturb(derp_camera_desc* cams, int n, int seed, double pos, double rot, double principal, double focal);
int derp_rig_scale(derp_camera_desc* cams, int n, double scale_rig, double radius, double scale_resolution);
/* ---- AlignColors (source/calibration/AlignColors.cpp): the red and blue planes of every camera resampled through
 * per-channel lens models onto the calibrated (green) rig, ahead of the pyramid ----
 * The cameras are the destinations of derp_create: the calibrated rig after --cameras, not normalised. Images are
 * interleaved BGR uint16 at the camera's resolution.
 * derp_align_derive_cameras: createCalibratedRBRigs for one camera (AlignColors.cpp:72-96). red / blue = `green` with
 *   scalar focal = the reference channel's times (float)(green focal / reference green focal), {s, -s}, and the reference
 *   channel's distortion (distortionMax follows, Camera.cpp:119-154). Refuses non-square pixels (getScalarFocal,
 *   Camera.cpp:185-188). Host only, no context and no device; a refusal leaves its text in derp_last_error(NULL).
 * derp_align_setup: the three reference rigs must hold exactly one camera each (AlignColors.cpp:164-166, checked here
 *   and not per frame); derives the models and builds createWarpMap (:52-70) for every camera of the context's rig, red
 *   and blue, once.
 * derp_align_maps: one camera's maps, each [h][w][2] float (x, y), as cv::Point2f holds them.
 * derp_align_frame: warpImage (:98-117) of one frame of every camera: out.G = in.G, out.R = getPixelBilinear(in, red
 *   map).R, out.B = getPixelBilinear(in, blue map).B (CvUtil.h:108-120, truncating u16 blend). img_w / img_h: the images'
 *   sizes, which must be the cameras' resolutions. in and out must not overlap.
 * Two points the reference leaves undefined: a pixel centre exactly on the principal point (0 / 0 there) maps to itself,
 * the limit of the expression, so its R and B are its own texel's; and undistort's abort when Newton "went past a
 * maximum" (Camera.h:278) does not exist here: the iteration's value is used. */
int derp_align_derive_cameras(const derp_camera_desc* green, const derp_camera_desc* red_ref,
                              const derp_camera_desc* green_ref, const derp_camera_desc* blue_ref,
                              derp_camera_desc* red, derp_camera_desc* blue);
int derp_align_setup(derp_ctx* ctx, const derp_camera_desc* red_ref, int n_red, const derp_camera_desc* green_ref,
                     int n_green, const derp_camera_desc* blue_ref, int n_blue);
int derp_align_maps(derp_ctx* ctx, int cam, float* red_xy, float* blue_xy);
int derp_align_frame(derp_ctx* ctx, const uint16_t* const* bgr, const int* img_w, const int* img_h, uint16_t* const* out);
/* ---- The tuning previews (source/render/ViewColorVarianceThresholds.cpp, ViewForegroundMaskThresholds.cpp): the images
 * the reference's trackbar windows show, for lists of slider positions instead of a window ----
 * Images are interleaved BGR uint16; the context's cameras are not read. One call renders at most 256 settings, and
 * a call whose device buffers exceed 4 GiB (DERP_PREVIEW_BUDGET_MB overrides it) is refused by name.
 * derp_preview_variance_levels: TrackVar::update's thresholds (ViewColorVarianceThresholds.cpp:69-73) for slider positions
 *   0..100 and scale = width / cols (1 when --width=0), in the reference's fp32 order -> levels4 = {varNoiseFloor,
 *   varHighThresh, varLowShow, varHighShow}. Host only, no context and no device; a refusal leaves its text in
 *   derp_last_error(NULL).
 * derp_preview_variance: computeImageVariance (DerpUtil.cpp:214-237, the level loop's kernel) once, then n marked copies
 *   of the image [n][h][w][3]: variance < low_show[k] -> (65535, 0, 0), variance > high_show[k] -> (65535, 0, 65535),
 *   both strict. counts[2k] / counts[2k + 1] = the blue / purple pixels of image k. out_variance ([h][w] float) may be
 *   NULL.
 * derp_preview_foreground: for every (blur, threshold, closing), blur-major, the mask derp_generate_foreground_mask
 *   answers for it, laid over the frame as cv::addWeighted(frame, 1.0, green where the mask is set, 0.5, 0) does on
 *   CV_16UC3: G = min(65535, rint(g + 32767.5)) half to even inside the mask, everything else unchanged.
 *   out_bgr16 [nb*nt*nc][h][w][3], out_mask [nb*nt*nc][h][w] 0 / 1 or NULL, counts[nb*nt*nc] = the mask's set pixels.
 *   The limits on the image and the radius are derp_generate_foreground_mask's, refused with its message.
 * GenerateKeypointProjections (source/render/GenerateKeypointProjections.cpp:57-104): where a grid of points of camera c1
 * lands in camera c0 over the depth range. params = {length_stride, height_stride, depth_min, depth_max, depth_samples,
 * search_overlap, search_radius} (seven doubles; the strides positive and finite, search_radius a whole number >= 0,
 * depth_samples >= 2, 0 < depth_min <= depth_max, else refused by name).
 * derp_preview_keypoint_samples: getNextDepthSample + computeBox (FeatureMatcher.cpp:116-133, 186-207) for the pixel
 *   (px, py) of cam_point, boxes in cam_into, both at their own resolutions: the accepted sample indices, their
 *   disparities and cv::Rect2f boxes (x, y, width, height). *n = how many were accepted, of which min(*n, max_out) are
 *   written. Host only, no context and no device; a refusal leaves its text in derp_last_error(NULL).
 * derp_preview_keypoint_rect: the filled cv::rectangle of one projected point: corners cvRound(p - 0.5 -+ search_radius)
 *   (half to even), both inclusive, clipped to w x h -> rect4 = {x0, y0, x1, y1}; x1 < x0 or y1 < y0: nothing of it is
 *   inside. Host only.
 * derp_preview_keypoints: the pair (c0, c1) of the context's destinations after derp_sweep_upload at scale 1: the
 *   rectangles (corners cvRound(p - 0.5 -+ search_radius), inclusive, clipped, a later one over an earlier one in the
 *   reference's loop order) in the grid point's colour (height_frac, width_frac, 1 - height_frac, 1), blended as
 *   image * 1.0f + rectangles * 0.6f + 0.0f. out_bgra8 [h][w][4] = 255.0f * blend as the rig preview tools convert it;
 *   out_float [h][w][4] the blend itself, or NULL; *n_rects = the rectangles drawn, those clipped away included (a
 *   camera whose resolution exceeds the first camera's sees points beyond the image). More than 2^20 grid points or
 *   2^20 rectangles of one pair are refused by name. */
int derp_preview_variance_levels(float var_low_max, float var_high_max, int low_slider, int high_slider, double scale,
                                 float* levels4);
int derp_preview_variance(derp_ctx* ctx, const uint16_t* bgr16, int w, int h, const float* low_show,
                          const float* high_show, int n, uint16_t* out_bgr16, uint32_t* counts, float* out_variance);
int derp_preview_foreground(derp_ctx* ctx, const uint16_t* template_bgr16, const uint16_t* frame_bgr16, int w, int h,
                            const int* blur, int nb, const float* threshold, int nt, const int* closing, int nc,
                            uint16_t* out_bgr16, uint8_t* out_mask, uint32_t* counts);
int derp_preview_keypoint_samples(const derp_camera_desc* cam_point, const derp_camera_desc* cam_into, double px, double py,
                                  const double* params, int max_out, int* indices, double* disparities, float* boxes4,
                                  int* n);
int derp_preview_keypoint_rect(double px, double py, int search_radius, int w, int h, int* rect4);
int derp_preview_keypoints(derp_ctx* ctx, int c0, int c1, const double* params, uint8_t* out_bgra8, float* out_float,
                           int* n_rects);
/* Host only, no context and no device (derp_simplify.cpp); non-zero = bad arguments (null pointer, an index out of
 * range, a negative budget, more than 2^31 - 1 vertices or faces).
 * derp_mesh_setup_host: computeInitialQuadrics over plain arrays: vertices f64 [nv][3], faces i32 [nf][3] -> the three
 *   arrays of derp_mesh_setup.
 * derp_mesh_simplify_host: MeshSimplifier::simplify + createFinalMesh (removeDeletedFaces, assignFaceVertexes,
 *   identifyBoundaries, getThreshold, haveNormalsFlipped, commonFaces, updateCosts). The set-up arrays come from
 *   derp_mesh_setup / derp_mesh_setup_host, or all three NULL: computed here. out_vertices / out_faces have room for
 *   the input's counts. One departure: a pass that deleted nothing under a zero or NaN threshold repeats for ever in
 *   the reference; here the loop ends (DERP_MESH_EXIT_STUCK).
 * derp_mesh_texcoords_equirect: mesh_util::addTextureCoordinatesEquirect (MeshUtil.h:407-419): vertices f64 [nv][3] in
 *   rig coordinates -> st f64 [nv][2], s = atan2(-z, -x) * 0.5 / pi + 0.5, t = -atan2(-y, |(x, z)|) / pi + 0.5. */
int derp_mesh_setup_host(const double* vertices, size_t nv, const int32_t* faces, size_t nf, int equi_error,
                         double* face_planes, double* edge_costs, double* vertex_quadrics);
int derp_mesh_simplify_host(const double* vertices, size_t nv, const int32_t* faces, size_t nf, const double* face_planes,
                            const double* edge_costs, const double* vertex_quadrics, int num_faces_out, float strictness,
                            int remove_boundary_edges, int equi_error, double* out_vertices, int32_t* out_faces,
                            size_t* out_nv, size_t* out_nf, int* stats);
int derp_mesh_texcoords_equirect(const double* vertices, size_t nv, double* st);
/* generateFovMasks for one destination camera at an arbitrary size (DerpUtil.cpp:259-276) */
int derp_fov_mask(derp_ctx* ctx, int dst, int w, int h, uint8_t* out);
/* upsampleDisparities for one camera (UpsampleDisparityLib.cpp:98-182). fg_mask / fg_mask_up /
 * bg_disp_up may be NULL when use_foreground_masks == 0. `dst` selects the FOV mask camera. */
int derp_upsample_disparity(derp_ctx* ctx, int dst, const float* disp, int w, int h,
                            const float* bg_disp_up, const uint8_t* fg_mask,
                            const uint8_t* fg_mask_up, int w_up, int h_up,
                            int use_foreground_masks, float* out);
/* generalizedJointBilateralFilter<float, Vec3w / Vec3f> (TemporalBilateralFilter.h:39-124) */
int derp_joint_bilateral_u16(derp_ctx* ctx, const float* image, const uint16_t* guide_bgr,
                             const uint8_t* mask, int w, int h, int radius, float sigma,
                             float weight0, float weight1, float weight2, float* out);
int derp_joint_bilateral_f32(derp_ctx* ctx, const float* image, const float* guide_bgr,
                             const uint8_t* mask, int w, int h, int radius, float sigma,
                             float weight0, float weight1, float weight2, float* out);
/* cv_util::maskedMedianBlur (CvUtil.h:336-385); background may be NULL */
int derp_masked_median(derp_ctx* ctx, const float* image, const float* background,
                       const uint8_t* mask, int w, int h, int radius, float* out);
/* temporalJointBilateralFilter (TemporalBilateralFilter.h:126-215) over n frames of one camera;
 * masks[t] = fg & fov as filterFrame builds them (TemporalBilateralFilter.cpp:139-160). */
int derp_temporal_filter(derp_ctx* ctx, const uint16_t* const* guides_bgr,
                         const float* const* disparities, const uint8_t* const* masks, int n_frames,
                         int w, int h, int frame_offset, float sigma, int space_radius,
                         float weight0, float weight1, float weight2, float* out);
/* same, on disparities that already live in HBM (multi-GPU path: received over RCCL) */
int derp_temporal_filter_dev(derp_ctx* ctx, const void* const* guides_bgrx_dev,
                             const float* const* disparities_dev, const uint8_t* const* masks_dev,
                             int n_frames, int w, int h, int frame_offset, float sigma,
                             int space_radius, float weight0, float weight1, float weight2,
                             float* out_dev);
/* device views of the selected frame's resident pyramid (not owned by the caller). Pointer lifetime:
 * derp_dev_disparity / derp_dev_color stay valid until derp_set_pyramid / derp_set_frame_slots /
 * derp_destroy; their CONTENT is written by kernels on the context's stream, so call derp_synchronize
 * before reading it from another stream. derp_dev_mask computes fov & fg of every destination at
 * `level` into a buffer of its own and has finished when it returns; that buffer is reused by the next
 * derp_dev_mask call (copy it if you need two levels at once). */
int derp_dev_disparity(derp_ctx* ctx, int level, int dst, float** ptr, size_t* bytes);
int derp_dev_color(derp_ctx* ctx, int level, int src, void** ptr_bgrx_u16, size_t* bytes);
int derp_dev_mask(derp_ctx* ctx, int level, int dst, uint8_t** ptr_fov_and_fg, size_t* bytes);

/* ---- sequence driver: frames of a sequence sharded over GPUs ----------------------
 * Replaces the depth_estimation stage of scripts/render/pipeline.py:364-408 for the frames one process
 * (= one GPU) owns: per level L, coarse to fine, DerpCLI(L) on every frame -> TemporalBilateralFilter(L)
 * over the window [t - R, t + R] clamped to the sequence (TemporalBilateralFilter.cpp:96-119) ->
 * "Transfer" (the filtered level overwrites disparity_levels/level_L) -> level L-1. Frames are
 * partitioned over `world` ranks in contiguous chunks (render.py:169-175) or cyclically; the raw level
 * disparity of the frames a neighbour rank's window reaches into is the only data exchanged inside the
 * level loop. Transports: RCCL send/recv on the context's stream (derp_seq_attach_rccl), same-process
 * loopback (tests: several ranks emulated on one GPU), or external (the caller moves the buffers that
 * derp_seq_buffer names). */
typedef struct derp_seq derp_seq;
enum { DERP_SEQ_BLOCK = 0, DERP_SEQ_CYCLIC = 1 };
typedef struct {
  int32_t time_radius;          /* --time_radius  2     TemporalBilateralFilter.cpp:54 */
  float sigma;                  /* --sigma        0.01  :51 */
  float weight_b;               /* --weight_b     0.5   :57 */
  float weight_g;               /* --weight_g     1.0   :58 */
  float weight_r;               /* --weight_r     1.0   :59; never read by the reference (:176-178 passes b, g, b) */
  int32_t space_radius;         /* --space_radius -1 = max(ceil(0.9^level), 1)  :52,164-168 */
  int32_t use_foreground_masks; /* temporal masking (pipeline.py:386 do_temporal_masking) */
  int32_t partition;            /* DERP_SEQ_BLOCK | DERP_SEQ_CYCLIC */
  int32_t do_temporal_filter;   /* 0 = replicas: no window, no exchange (pipeline.py:378) */
  int32_t resident_frames;      /* 0 = every owned frame lives in HBM; N < owned frames = out of core: N frame slots,
                                 * inputs streamed per level from host memory (derp_seq_host_inputs), results kept in
                                 * page-locked host buffers; N >= 2 * time_radius + 1. The reference is independent of
                                 * the sequence length because every level round-trips through the file system
                                 * (render.py:169-175, pipeline.py:120-171) */
} derp_seq_options;
typedef struct {
  int32_t frame, from_rank, to_rank;
} derp_seq_transfer;
void derp_seq_options_default(derp_seq_options* o);
/* host-only plan (no GPU needed): window of a frame, owner of a frame, and every (frame, from, to)
 * transfer of one exchange, in the global order all ranks post them. derp_seq_plan returns the count. */
void derp_seq_window(int frame, int first, int last, int time_radius, int* lo, int* hi);
int derp_seq_owner(int first, int last, int world, int partition, int frame);
int derp_seq_plan(int first, int last, int world, int time_radius, int partition, derp_seq_transfer* out, int cap);
/* Allocates one frame slot per owned frame (derp_set_frame_slots) and the halo buffers; call after
 * derp_set_pyramid and before uploading frames. Upload frame t with derp_select_frame(ctx,
 * derp_seq_frame_slot(seq, t)) + the derp_upload_* / derp_build_pyramid_* functions. */
int derp_seq_create(derp_seq** out, derp_ctx* ctx, int first, int last, int rank, int world,
                    const derp_seq_options* opt);
void derp_seq_destroy(derp_seq* seq);
int derp_seq_counts(const derp_seq* seq, int* n_owned, int* n_halo);
int derp_seq_frames(const derp_seq* seq, int halo, int* frames, int cap);
int derp_seq_frame_slot(const derp_seq* seq, int frame);   /* -1 when not owned by this rank */
/* Inputs of one level of an owned frame from host memory — loadLevelImages (ImageUtil.h:79-94) for the frame:
 * colour [S][h*w][3] interleaved BGR u16, optional foreground masks [S][h*w] u8 and background disparity
 * [D][h*w] f32. Resident mode: uploaded into the frame's slot now. Out of core: the pointers are kept and must
 * stay valid until the sequence is destroyed (or replaced by another call). */
int derp_seq_host_inputs(derp_seq* seq, int frame, int level, const uint16_t* color_bgr, const uint8_t* fg_masks,
                         const float* background_disparity);
/* Resident mode: one camera's colour image [h*w][3] BGR u16 into the frame's slot on the library's copy stream —
 * it overlaps whatever another frame is computing (the frame itself must not be in flight). */
int derp_seq_upload_color_plane(derp_seq* seq, int frame, int level, int src, const uint16_t* bgr);
/* level disparity of an owned frame, whichever mode: upload = the previous level read back from disk when a run
 * resumes (DerpCLI.cpp:287-288); download = the level's result (filtered when the temporal filter is on) */
int derp_seq_upload_disparity(derp_seq* seq, int frame, int level, int dst, const float* disparity);
int derp_seq_download_disparity(derp_seq* seq, int frame, int level, int dst, float* disparity);  /* dst = -1: all, [D][h*w] */
/* buffer of an owned or halo frame: kind 0 colour [S][h*w] BGRX u16, 1 fg mask [S][h*w] u8,
 * 2 level disparity [D][h*w] f32 */
int derp_seq_buffer(derp_seq* seq, int frame, int level, int kind, void** ptr, size_t* bytes);
/* external transports that stage through host memory: copy such a buffer to (to_device = 0) or from (1) `host` */
int derp_seq_buffer_copy(derp_seq* seq, int frame, int level, int kind, void* host, size_t bytes, int to_device);
/* transports */
int derp_rccl_unique_id(void* out128, size_t cap);         /* ncclGetUniqueId; rank 0 calls, caller distributes */
int derp_seq_attach_rccl(derp_seq* seq, const void* unique_id, size_t bytes);
int derp_seq_attach_loopback(derp_seq* seq, derp_seq* const* peers, int n_peers);
int derp_seq_attach_external(derp_seq* seq);
int derp_seq_selftest(derp_seq* seq, int words);           /* one ring step over RCCL, verified */
/* schedule */
int derp_seq_exchange_inputs(derp_seq* seq);               /* colour (+ fg) pyramids of the halo frames, once */
int derp_seq_exchange_inputs_level(derp_seq* seq, int level);  /* ... one level of them (inputs that arrive level by level) */
int derp_seq_level_compute(derp_seq* seq, int level);      /* processLevel(level) of every owned frame */
int derp_seq_level_compute_frame(derp_seq* seq, int level, int frame);  /* ... of one owned frame (each once per level) */
/* ... or: the frame's raw level was computed by another process and uploaded with derp_seq_upload_disparity
 * (TemporalBilateralFilter's inputs: DerpCLI's files of the level, TemporalBilateralFilter.cpp:139-160) */
int derp_seq_level_provided_frame(derp_seq* seq, int level, int frame);
int derp_seq_level_exchange(derp_seq* seq, int level);     /* raw level disparity of the halo frames */
int derp_seq_mark_exchanged(derp_seq* seq, int level);     /* external transport: the halo frames' level has arrived */
int derp_seq_level_filter(derp_seq* seq, int level);       /* temporal filter of every owned frame + Transfer; fails
                                                            * unless compute (and, with halo frames, the exchange) of
                                                            * this level completed first */
/* One owned frame's filter AHEAD of derp_seq_level_filter: possible as soon as every frame of its window holds the
 * level's raw result (owned frames computed, halo frames exchanged) — for the frames in the middle of a chunk long
 * before the level's last frame is computed, so that their files can be written behind the remaining compute
 * (TemporalBilateralFilter.cpp:139-184 per frame). The result stays in the frame's scratch; the Transfer is still
 * derp_seq_level_filter's. Returns 0 = filtered, 2 = not possible yet / out of core / filter off (no error), 1 = error. */
int derp_seq_level_filter_frame(derp_seq* seq, int level, int frame);
/* ... and its download from that scratch, on the copy stream (the compute stream keeps running); dst = -1: every
 * destination's plane in one copy, [D][h*w] */
int derp_seq_download_filtered(derp_seq* seq, int frame, int level, int dst, float* disparity);
int derp_seq_run(derp_seq* seq, int level_start, int level_end);
int derp_seq_stats(derp_seq* seq, uint64_t* bytes_sent, uint64_t* bytes_received, double* exchange_ms);
int derp_seq_stats_reset(derp_seq* seq);
/* the part of derp_seq_stats' exchange_ms this rank's compute stream stood still for: a level's exchange runs on its own
 * stream beside the filter of the owned frames whose windows hold no halo frame (reset by derp_seq_stats_reset) */
int derp_seq_exchange_exposed_ms(derp_seq* seq, double* exposed_ms);

/* ---- camera ISP: raw Bayer -> RGB (source/isp/CameraIsp.h, RawToRgb.cpp, RawUtil.cpp) ---------------
 * The ISP has no rig, so it has a handle of its own. Errors of every derp_isp_* call (creation included) are
 * left, per thread, where derp_last_error(NULL) reads them. */
typedef struct derp_isp derp_isp;
enum { DERP_ISP_MAX_ROLLOFF = 16 };
enum { DERP_ISP_BILINEAR = 0, DERP_ISP_FREQUENCY = 1, DERP_ISP_EDGE_AWARE = 2, DERP_ISP_CHROMA_SUPPRESSED = 3 };
enum {
  DERP_ISP_STAGE_LOAD = 0,        /* loadImageFromSensor + resizeInput: 1 plane [h][w] */
  DERP_ISP_STAGE_PIXEL = 1,       /* blackLevelAdjust, antiVignette, whiteBalance, clampAndStretch: 1 plane */
  DERP_ISP_STAGE_STUCK = 2,       /* removeStuckPixels (the plane of stage 1 when stuckPixelRadius is 0): 1 plane */
  DERP_ISP_STAGE_DEMOSAIC = 3,    /* demosaic: 3 planes R, G, B, each [h][w] */
  DERP_ISP_STAGE_COLOR = 4,       /* colorCorrect: 3 planes */
  DERP_ISP_STAGE_LOWPASS = 5,     /* iirLowPass (only when sharpening runs): 3 planes */
  DERP_ISP_STAGE_SHARPENED = 6    /* sharpenWithIirLowPass (only when sharpening runs): 3 planes */
};
/* every field of the "CameraIsp" JSON object (CameraIsp.h:521-562); points are x, y, z = r, g, b */
typedef struct {
  int32_t bits_per_pixel;         /* "bitsPerPixel"  16 */
  int32_t width, height;          /* "width", "height": the sensor's, 0 until set */
  int32_t is_little_endian;       /* "isLittleEndian"  0 */
  int32_t is_row_major;           /* "isRowMajor"  1 */
  char bayer_pattern[8];          /* "bayerPattern"  "GBRG" (upper case) */
  char plane_order[8];            /* "planeOrder"  "": interleaved */
  float black_level[3];           /* "blackLevel"  0 */
  float clamp_min[3];             /* "clampMin"  0 */
  float clamp_max[3];             /* "clampMax"  1 */
  int32_t stuck_pixel_threshold;  /* "stuckPixelThreshold"  0 */
  float stuck_pixel_darkness_threshold; /* "stuckPixelDarknessThreshold"  0 */
  int32_t stuck_pixel_radius;     /* "stuckPixelRadius"  0 = off */
  int32_t n_rolloff_h, n_rolloff_v;  /* "vignetteRollOffH" / "vignetteRollOffV": one point (1, 1, 1) each */
  float rolloff_h[DERP_ISP_MAX_ROLLOFF][3];
  float rolloff_v[DERP_ISP_MAX_ROLLOFF][3];
  float white_balance_gain[3];    /* "whiteBalanceGain"  1 */
  float ccm[9];                   /* "ccm"  identity, row major */
  float saturation;               /* "saturation"  1 */
  float gamma[3];                 /* "gamma"  1 */
  float low_key_boost[3];         /* "lowKeyBoost"  0 */
  float high_key_boost[3];        /* "highKeyBoost"  0 */
  float contrast;                 /* "contrast"  1 */
  float sharpening[3];            /* "sharpening"  0: runs only when all three are non-zero */
  float sharpening_support;       /* "sharpeningSupport"  10 / 2048 */
  float noise_core;               /* "noiseCore"  1000 */
  int32_t n_companding_lut;       /* "compandingLut": parsed and, as in the reference, never used */
} derp_isp_config;
void derp_isp_config_default(derp_isp_config* cfg);   /* CameraIsp::CameraIsp, CameraIsp.h:490-519 */
/* cameraIspFromConfigFileWithOptions (RawUtil.cpp:42-57): setup(), setResize, setDemosaicFilter, setToneCurveEnabled.
 * Refused before any allocation: a filter outside 0..3, DERP_ISP_FREQUENCY, a downscale other than 1, 2, 4, 8, odd or
 * zero sensor dimensions, bits_per_pixel other than 8 or 16. Fails without a HIP device: there is no CPU path. */
int derp_isp_create(derp_isp** out, int device, const derp_isp_config* cfg, int demosaic_filter, int pow2_downscale,
                    int apply_tone_curve);
void derp_isp_destroy(derp_isp* isp);
int derp_isp_output_size(const derp_isp* isp, int* width, int* height);   /* getOutputWidth / getOutputHeight */
/* rawToRgb (RawUtil.cpp:59-63): loadImageFromSensor + getImage<T>. `raw` is the file's content, raw_bytes >=
 * width * height * bits_per_pixel / 8; out_bgr is [h][w][3] BGR, u8 or u16 like the sensor. */
int derp_isp_process(derp_isp* isp, const void* raw, size_t raw_bytes, void* out_bgr);
/* the fp32 plane(s) the last derp_isp_process left after a stage (tests) */
int derp_isp_stage(derp_isp* isp, int stage, float* out);
/* the host-built tables: curveHAtPixel [w][3] and curveVAtPixel [h][3] (CameraIsp.h:668-674), compositeCCM [9]
 * (:630-645), toneCurveLut [4096][3] (buildToneCurveLut, :382-416). Any pointer may be NULL. */
int derp_isp_tables(const derp_isp* isp, float* vignette_h, float* vignette_v, float* ccm9, float* tone_lut);

/* ---- RigSimulator: a ray-traced procedural scene as a rig sees it (source/rig/RigSimulator.cpp) -------------
 * The scene and its sphere tree are built on the host (derp_sim_scene_*: no device, no context), flattened in
 * pre-order and handed to a derp_sim, which traces one ray per supersampled pixel on the GPU. */
typedef struct {        /* render::Triangle, RaytracingPrimitives.h:35-50 */
  float v0[3], v1[3], v2[3];
  float e1[3], e2[3];   /* v1 - v0, v2 - v0 */
  float normal[3];      /* e1 x e2, normalised */
  float color[3];       /* BGR in 0..1 */
} derp_sim_triangle;
typedef struct {        /* one BoundingVolumeHierarchy node of the pre-order flat tree */
  float center[3];
  float radius;
  int32_t skip;         /* index of the first node behind this node's subtree (the walk goes there on a sphere miss) */
  int32_t first;        /* leaf: offset of its triangles in the leaf index list */
  int32_t count;        /* leaf: number of triangles (may be 0); inner node: -1 */
  int32_t n_children;   /* inner node: number of children (they follow in order); leaf: 0 */
} derp_sim_node;
typedef struct derp_sim_scene derp_sim_scene;
derp_sim_scene* derp_sim_scene_create(void);
void derp_sim_scene_destroy(derp_sim_scene* scene);
/* The builders append to the scene; the random ones call the C library's rand() in the reference's order.
 * makeIcosahedronScene (RigSimulator.cpp:264-289, flags num_random_icosahedrons, min / max_icosahedron_dist,
 * min / max_icosahedron_radius, red_triangle), makeCubesScene (:291-343), makeGroundPlaneScene (:345-358). */
int derp_sim_scene_icosahedrons(derp_sim_scene* scene, int count, double min_dist, double max_dist, double min_radius,
                                double max_radius, int red_triangle);
int derp_sim_scene_cubes(derp_sim_scene* scene);
int derp_sim_scene_ground_plane(derp_sim_scene* scene, double ground_plane_dist_m);
/* Triangle::Triangle of three vertices and a BGR colour */
int derp_sim_scene_add_triangle(derp_sim_scene* scene, const float* v0, const float* v1, const float* v2,
                                const float* color_bgr);
/* BoundingVolumeHierarchy::makeBVH (BoundingVolumeHierarchy.h:32-114); the reference passes 20, 5, 50 */
int derp_sim_bvh_build(derp_sim_scene* scene, int leaf_threshold, int split_k, int max_depth);
int derp_sim_scene_counts(const derp_sim_scene* scene, int* n_triangles, int* n_nodes, int* n_leaf_indices);
/* triangles [n_triangles], nodes [n_nodes], leaf index list [n_leaf_indices]; any pointer may be NULL */
int derp_sim_scene_get(const derp_sim_scene* scene, derp_sim_triangle* triangles, derp_sim_node* nodes,
                       int32_t* leaf_indices);
/* Ken Perlin's reference permutation ("Improved Noise", 2002) twice over: the p[512] of PerlinNoise.h */
void derp_sim_perlin_table(uint8_t* p512);
/* the unit icosahedron of the scenes and of the dodecahedron / icosahedron rigs (icosahedron_data, :123-143): 12
 * vertices x 3, 20 faces x 3 vertex indices */
void derp_sim_icosahedron(float* vertices36, int32_t* faces60);
/* corruptImageWithNoise (:494-508) on a [h][w][3] float image in 0..255, rand() in row order */
int derp_sim_noise(float* bgr, int w, int h, double amplitude);
/* traceRayToGetColor on the host, one thread: the CPU baseline of tools/sim_timing.py. rays = n x (origin, dir);
 * out_bgrd = n x (b, g, r, depth). The sky lookup is not part of it (a miss gives 0, 0, 0, FLT_MAX). */
int derp_sim_trace_host(const derp_sim_scene* scene, const float* rays6, size_t n, float* out_bgrd);

typedef struct {
  double ceiling_position, ceiling_width, ceiling_depth; /* --ceiling_*: used when a ceiling image is uploaded */
  double marble_scale;                                    /* --marble_scale 0.1 */
  int32_t marble;                                         /* --marble */
  int32_t pad;
} derp_sim_params;
enum {
  DERP_SIM_STAGE_ORIGIN = 0, /* [H][W][3] f32 */
  DERP_SIM_STAGE_DIRECTION,  /* [H][W][3] f32 */
  DERP_SIM_STAGE_HIT,        /* [H][W] i32: triangle index, -1 sky, -2 ceiling, -3 outside the image circle */
  DERP_SIM_STAGE_DISTANCE,   /* [H][W] f32: the depth the ray returns (FLT_MAX for sky / outside) */
  DERP_SIM_STAGE_COLOR       /* [H][W][3] f32 BGR x 255, before the downscale */
};
typedef struct derp_sim derp_sim;
/* Fails without a HIP device: the tracer has no CPU path behind this object. */
int derp_sim_create(derp_sim** out, int device);
void derp_sim_destroy(derp_sim* sim);
/* skybox / ceiling: 8-bit BGR as IMREAD_COLOR gives them; ceiling_bgr NULL = no ceiling (--ceiling_path empty) */
int derp_sim_upload(derp_sim* sim, const derp_sim_triangle* triangles, int n_triangles, const derp_sim_node* nodes,
                    int n_nodes, const int32_t* leaf_indices, int n_leaf_indices, const uint8_t* skybox_bgr, int sky_w,
                    int sky_h, const uint8_t* ceiling_bgr, int ceiling_w, int ceiling_h, const derp_sim_params* params);
/* renderCamera (:591-625) without the noise: bgr_out [h][w][3] f32 in 0..255, depth_out [h][w] f32, (w, h) the
 * camera's resolution, after the aas x aas INTER_AREA downscale */
int derp_sim_render_camera(derp_sim* sim, const derp_camera_desc* cam, int aas, float* bgr_out, float* depth_out);
/* renderMonoEquirect (:520-547; bgr_a = colour, aux_out = inverse depth clamped to 0..1, bgr_b unused) or
 * renderStereoEquirect (:549-589; bgr_a = left, bgr_b = right, aux_out unused) */
int derp_sim_render_equirect(derp_sim* sim, int w, int h, int aas, int stereo, double interpupillary_radius,
                             float* bgr_a, float* bgr_b, float* aux_out);
/* re-trace caller-given rays (n x (origin, dir)) as one row of n pixels; read the result with derp_sim_stage */
int derp_sim_trace_rays(derp_sim* sim, const float* rays6, size_t n);
/* a plane of the last render at its supersampled size (`eye` 1 = the right eye of a stereo equirect); tests */
int derp_sim_stage_size(const derp_sim* sim, int* width, int* height);
int derp_sim_stage(derp_sim* sim, int stage, int eye, void* out);

/* ---- measurement -------------------------------------------------------------------------- */
/* computeCost evaluations and (evaluation, src) pairs reaching computeSSD since the last reset:
 * the N_cost / N_pair of BASELINE.md's B_alg = 64*N_cost + 272*N_pair. */
int derp_get_counters(derp_ctx* ctx, uint64_t* n_cost, uint64_t* n_pair, uint64_t* insufficient);
int derp_reset_counters(derp_ctx* ctx);
/* per-stage HIP-event timing on the context's own stream, plus per-stage computeCost counters.
 * stage names: "fov_mask", "variance", "own_bias", "upsample", "proj_warp", "reproject",
 * "proj_bias", "brute_force", "random_proposals", "ping_pong", "mismatches", "bilateral", "median", "mask_fov", "temporal" (the
 * sequence driver's filter + Transfer), "lanes_wall" (a coarse level whose frames derp_seq_level_compute ran on overlapping
 * work lanes: the level's wall on the context's stream — the per-stage spans of such a level overlap in time).
 * level = -1 aggregates all levels. ms / launches / n_cost / n_pair may be NULL. */
int derp_profile_enable(derp_ctx* ctx, int on);
int derp_profile_reset(derp_ctx* ctx);
int derp_profile_query(derp_ctx* ctx, const char* stage, int level, double* ms, int* launches,
                       uint64_t* n_cost, uint64_t* n_pair);
/* computeCost evaluations of `stage` / `level` that were served from an earlier identical evaluation
 * instead of being recomputed (first ping-pong iteration, candidate (0,0)); they ARE included in the
 * logical n_cost / n_pair above, which count what the reference algorithm issues. */
int derp_profile_memoised(derp_ctx* ctx, const char* stage, int level, uint64_t* n_memoised);
int derp_device_name(derp_ctx* ctx, char* buf, int n);
/* free / total HBM of the context's device right now (hipMemGetInfo): what a host uses to decide how many frames of a
 * sequence to keep resident (the reference has no counterpart: its working set lives in host memory) */
int derp_device_memory(derp_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);

/* host-only self checks (no GPU needed): restated libstdc++ algorithms the device code uses */
int derp_host_nth_element_pairs(float* pairs, int n, int nth);
float derp_host_minstd_uniform(int seed, uint64_t draw_index, float a, float b);
/* the tile order of the random-proposal / ping-pong launches: out[b * per_block + step] = the tile that block b of the
 * grid handles at `step` of its walk, for a level of `tiles` tiles, `bands` bands per XCD (1, 2, 4), band rotation `rot`
 * (the destination index) and `per_block` tiles per block (1, 2, 4). Returns the number of blocks of the grid (a tile
 * index at or past `tiles` is padding), or 0 on bad arguments or when `capacity` ints do not hold the map. */
int derp_host_cost_tile_map(int tiles, int bands, int rot, int per_block, int* out, int capacity);
/* the table budget -> the destination batch of a level: how many of `n_dst` destinations' projection tables fit
 * `budget_bytes` at `bytes_no_inverse` each, or at `bytes_with_inverse` each when inverse warps are stored: always if
 * `inverse_needed`, otherwise as soon as the level runs in batches. *batch is the size of the equal-sized batches,
 * *store_inverse whether inverse warps are stored. Returns 1 on bad arguments or when not even one destination fits. */
int derp_host_table_batch(int n_dst, uint64_t bytes_no_inverse, uint64_t bytes_with_inverse, int inverse_needed,
                          uint64_t budget_bytes, int* batch, int* store_inverse);

#ifdef __cplusplus
}
#endif
#endif /* DERP_HIP_H */
