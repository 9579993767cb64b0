"""ctypes binding of the C-ABI in include/derp_hip.h (libderp_hip.so, built in-tree).

Plumbing only: every computation happens in the HIP library. There is no CPU fallback —
`Derp(...)` raises when the library or a gfx950 device is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DERP_LIB") or os.path.join(_HERE, "libderp_hip.so")
CAM_TYPES = {"FTHETA": 0, "RECTILINEAR": 1, "EQUISOLID": 2, "ORTHOGRAPHIC": 3}

STAGES = ["fov_mask", "variance", "own_bias", "upsample", "proj_warp", "reproject", "proj_bias", "brute_force",
          "random_proposals", "ping_pong", "mismatches", "bilateral", "median", "mask_fov", "temporal"]


class SeqOptions(C.Structure):
    _fields_ = [
        ("time_radius", C.c_int32), ("sigma", C.c_float), ("weight_b", C.c_float), ("weight_g", C.c_float),
        ("weight_r", C.c_float), ("space_radius", C.c_int32), ("use_foreground_masks", C.c_int32),
        ("partition", C.c_int32), ("do_temporal_filter", C.c_int32), ("resident_frames", C.c_int32),
    ]


class SeqTransfer(C.Structure):
    _fields_ = [("frame", C.c_int32), ("from_rank", C.c_int32), ("to_rank", C.c_int32)]


class CameraDesc(C.Structure):
    _fields_ = [
        ("type", C.c_int32), ("has_principal", C.c_int32), ("has_distortion", C.c_int32), ("has_fov", C.c_int32),
        ("origin", C.c_double * 3), ("forward", C.c_double * 3), ("up", C.c_double * 3), ("right", C.c_double * 3),
        ("resolution", C.c_double * 2), ("focal", C.c_double * 2), ("principal", C.c_double * 2),
        ("distortion", C.c_double * 3), ("fov", C.c_double), ("id", C.c_char * 64),
    ]


class Options(C.Structure):
    _fields_ = [
        ("min_depth_m", C.c_float), ("max_depth_m", C.c_float), ("var_noise_floor", C.c_float),
        ("var_high_thresh", C.c_float), ("random_proposals", C.c_int32), ("ping_pong_iterations", C.c_int32),
        ("mismatches_start_level", C.c_int32), ("do_bilateral_filter", C.c_int32), ("do_median_filter", C.c_int32),
        ("use_foreground_masks", C.c_int32), ("partial_coverage", C.c_int32), ("rebuild_warp_tables", C.c_int32),
    ]


class MeshPass(C.Structure):  # derp_mesh_pass
    _fields_ = [("faces", C.c_longlong), ("feasible", C.c_longlong), ("winners", C.c_longlong), ("applied", C.c_longlong),
                ("deleted", C.c_longlong), ("threshold", C.c_double)]


class RenderParams(C.Structure):
    """derp_render_params (include/derp_hip.h): one SimpleMeshRenderer view."""
    _fields_ = [
        ("kind", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("position", C.c_double * 3),
        ("forward", C.c_double * 3), ("up", C.c_double * 3), ("horizontal_fov", C.c_double), ("ipd", C.c_float),
        ("alpha_blend", C.c_int32), ("disparity_color", C.c_int32), ("weight", C.c_int32), ("zero_nans", C.c_int32),
    ]


ISP_MAX_ROLLOFF = 16


class IspConfig(C.Structure):
    """derp_isp_config (include/derp_hip.h)."""
    _fields_ = [
        ("bits_per_pixel", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("is_little_endian", C.c_int32),
        ("is_row_major", C.c_int32), ("bayer_pattern", C.c_char * 8), ("plane_order", C.c_char * 8),
        ("black_level", C.c_float * 3), ("clamp_min", C.c_float * 3), ("clamp_max", C.c_float * 3),
        ("stuck_pixel_threshold", C.c_int32), ("stuck_pixel_darkness_threshold", C.c_float),
        ("stuck_pixel_radius", C.c_int32), ("n_rolloff_h", C.c_int32), ("n_rolloff_v", C.c_int32),
        ("rolloff_h", (C.c_float * 3) * ISP_MAX_ROLLOFF), ("rolloff_v", (C.c_float * 3) * ISP_MAX_ROLLOFF),
        ("white_balance_gain", C.c_float * 3), ("ccm", C.c_float * 9), ("saturation", C.c_float), ("gamma", C.c_float * 3),
        ("low_key_boost", C.c_float * 3), ("high_key_boost", C.c_float * 3), ("contrast", C.c_float),
        ("sharpening", C.c_float * 3), ("sharpening_support", C.c_float), ("noise_core", C.c_float),
        ("n_companding_lut", C.c_int32),
    ]


class SimParams(C.Structure):
    """derp_sim_params (include/derp_hip.h)."""
    _fields_ = [("ceiling_position", C.c_double), ("ceiling_width", C.c_double), ("ceiling_depth", C.c_double),
                ("marble_scale", C.c_double), ("marble", C.c_int32), ("pad", C.c_int32)]


RENDER_KINDS = {"cube": 0, "equirect": 1, "snapshot": 2}
WEIGHTS = {"svd": 0, "minor": 1}
FORMATS = ["cubecolor", "cubedisp", "eqrcolor", "eqrdisp", "lr180", "snapcolor", "snapdisp", "tb3dof", "tbstereo"]


def render_params(kind="equirect", width=3072, height=None, position=(0, 0, 0), forward=(-1, 0, 0), up=(0, 0, 1),
                  horizontal_fov=90.0, ipd=0.0, alpha_blend=True, disparity_color=False, weight="svd", zero_nans=False):
    """derp_render_params with SimpleMeshRenderer's defaults (height = width / 2)."""
    p = RenderParams()
    lib().derp_render_params_default(C.byref(p))
    p.kind = RENDER_KINDS[kind]
    p.width = width
    p.height = width // 2 if height is None else height
    for k, v in (("position", position), ("forward", forward), ("up", up)):
        for i in range(3):
            getattr(p, k)[i] = float(v[i])
    p.horizontal_fov = horizontal_fov
    p.ipd = ipd
    p.alpha_blend = int(bool(alpha_blend))
    p.disparity_color = int(bool(disparity_color))
    p.weight = WEIGHTS[weight]
    p.zero_nans = int(bool(zero_nans))
    return p


def stream_srgb_table():
    """sRGB -> linear of every 8-bit code, as derp_stream_upload decodes the colour texture -> f32 [256]"""
    out = np.zeros(256, dtype=np.float32)
    lib().derp_stream_srgb_table(out.ctypes.data_as(C.c_void_p))
    return out


def render_format_size(fmt, width, height):
    w, h = C.c_int(), C.c_int()
    if lib().derp_render_format_size(fmt.encode(), width, height, C.byref(w), C.byref(h)):
        raise ValueError("Invalid format: %s" % fmt)
    return w.value, h.value


# The prototype of every function include/derp_hip.h declares: name -> (restype, [argtypes]), applied by lib() and held
# against the header by tests/test_abi.py. int32_t / uint64_t / size_t / float / double by value keep their width;
# const char* is c_char_p; a pointer to a struct mirrored above is POINTER(mirror); handles and every other pointer are
# c_void_p (None = NULL).
_int, _size, _u64, _f32, _f64, _str, _ptr = C.c_int, C.c_size_t, C.c_uint64, C.c_float, C.c_double, C.c_char_p, C.c_void_p
_cam, _opt, _seq_opt, _transfer = C.POINTER(CameraDesc), C.POINTER(Options), C.POINTER(SeqOptions), C.POINTER(SeqTransfer)
_pass, _view, _isp, _sim = C.POINTER(MeshPass), C.POINTER(RenderParams), C.POINTER(IspConfig), C.POINTER(SimParams)
PROTOTYPES = {
    "derp_options_default": (None, [_opt]),
    "derp_create": (_int, [_ptr, _int, _cam, _int, _cam, _int]),
    "derp_destroy": (None, [_ptr]),
    "derp_last_error": (_str, [_ptr]),
    "derp_set_options": (_int, [_ptr, _opt]),
    "derp_set_pyramid": (_int, [_ptr, _int, _ptr, _ptr, _int, _int]),
    "derp_set_frame_slots": (_int, [_ptr, _int]),
    "derp_select_frame": (_int, [_ptr, _int]),
    "derp_frame_slots": (_int, [_ptr, _ptr, _ptr]),
    "derp_host_alloc": (_ptr, [_size]),
    "derp_host_free": (None, [_ptr]),
    "derp_bind_thread": (_int, [_ptr]),
    "derp_host_register": (_int, [_ptr, _size]),
    "derp_host_unregister": (None, [_ptr]),
    "derp_upload_color": (_int, [_ptr, _int, _int, _ptr]),
    "derp_upload_foreground_mask": (_int, [_ptr, _int, _int, _ptr]),
    "derp_upload_background_disparity": (_int, [_ptr, _int, _int, _ptr]),
    "derp_upload_disparity": (_int, [_ptr, _int, _int, _ptr]),
    "derp_build_pyramid_color": (_int, [_ptr, _int, _ptr, _int, _int]),
    "derp_build_pyramid_foreground_mask": (_int, [_ptr, _int, _ptr, _int, _int, _int]),
    "derp_build_pyramid_background_disparity": (_int, [_ptr, _int, _ptr, _int, _int]),
    "derp_download_level_color": (_int, [_ptr, _int, _int, _ptr]),
    "derp_download_level_mask": (_int, [_ptr, _int, _int, _ptr]),
    "derp_download_level_background": (_int, [_ptr, _int, _int, _ptr]),
    "derp_image_info": (_int, [_ptr, _size, _ptr, _ptr, _ptr, _ptr]),
    "derp_image_decode": (_int, [_ptr, _size, _ptr, _size]),
    "derp_image_last_error": (_str, []),
    "derp_jpeg_encode": (_int, [_ptr, _int, _int, _int, _int, _ptr, _size, _ptr]),
    "derp_resize_area": (_int, [_ptr, _int, _ptr, _int, _int, _ptr, _int, _int]),
    "derp_generate_foreground_mask": (_int, [_ptr, _ptr, _ptr, _int, _int, _int, _f32, _int, _ptr]),
    "derp_preview_variance_levels": (_int, [_f32, _f32, _int, _int, _f64, _ptr]),
    "derp_preview_variance": (_int, [_ptr, _ptr, _int, _int, _ptr, _ptr, _int, _ptr, _ptr, _ptr]),
    "derp_preview_foreground": (_int, [_ptr, _ptr, _ptr, _int, _int, _ptr, _int, _ptr, _int, _ptr, _int, _ptr, _ptr, _ptr]),
    "derp_preview_keypoint_samples": (_int, [_cam, _cam, _f64, _f64, _ptr, _int, _ptr, _ptr, _ptr, _ptr]),
    "derp_preview_keypoint_rect": (_int, [_f64, _f64, _int, _int, _int, _ptr]),
    "derp_preview_keypoints": (_int, [_ptr, _int, _int, _ptr, _ptr, _ptr, _ptr]),
    "derp_process_level": (_int, [_ptr, _int]),
    "derp_process_pyramid": (_int, [_ptr, _int, _int]),
    "derp_synchronize": (_int, [_ptr]),
    "derp_download_disparity": (_int, [_ptr, _int, _int, _ptr]),
    "derp_download_cost": (_int, [_ptr, _int, _ptr, _ptr]),
    "derp_level_begin": (_int, [_ptr, _int]),
    "derp_stage_reproject_colors": (_int, [_ptr]),
    "derp_stage_brute_force": (_int, [_ptr]),
    "derp_stage_random_proposals": (_int, [_ptr]),
    "derp_stage_ping_pong": (_int, [_ptr]),
    "derp_stage_mismatches": (_int, [_ptr]),
    "derp_stage_bilateral_filter": (_int, [_ptr]),
    "derp_stage_median_filter": (_int, [_ptr]),
    "derp_stage_mask_fov": (_int, [_ptr]),
    "derp_level_end": (_int, [_ptr]),
    "derp_set_level_disparity": (_int, [_ptr, _int, _ptr]),
    "derp_get_level_disparity": (_int, [_ptr, _int, _ptr]),
    "derp_cost_map": (_int, [_ptr, _int, _ptr, _ptr, _ptr]),
    "derp_debug_download": (_int, [_ptr, _int, _int, _int, _ptr]),
    "derp_debug_atan2_ypos": (_int, [_ptr, _ptr, _ptr, _ptr, _size]),
    "derp_debug_fp64": (_int, [_ptr, _int, _ptr, _ptr, _ptr, _size]),
    "derp_debug_sees": (_int, [_ptr, _int, _ptr, _size, _ptr]),
    "derp_debug_expf": (_int, [_ptr, _int, _ptr, _ptr, _size]),
    "derp_debug_block_trace": (_int, [_ptr, _str, _int, _ptr, _size, _ptr, _ptr]),
    "derp_debug_level_plan": (_int, [_ptr, _ptr]),
    "derp_download_mismatch_mask": (_int, [_ptr, _int, _ptr]),
    "derp_layer_disparities": (_int, [_ptr, _ptr, _ptr, _size, _ptr]),
    "derp_ssim": (_int, [_ptr, _ptr, _ptr, _int, _int, _int, _f32, _f32, _f32, _ptr]),
    "derp_average_score": (_int, [_ptr, _ptr, _int, _int, _ptr]),
    "derp_rephotograph": (_int, [_ptr, _int, _ptr, _ptr, _int, _int, _ptr]),
    "derp_rephotograph_upload": (_int, [_ptr, _ptr, _ptr, _int, _int]),
    "derp_rephotograph_render": (_int, [_ptr, _int, _ptr]),
    "derp_canopy_cubemap": (_int, [_ptr, _ptr, _ptr, _int, _ptr]),
    "derp_render_params_default": (None, [_view]),
    "derp_render_upload": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "derp_render": (_int, [_ptr, _view, _ptr, _ptr]),
    "derp_render_format_size": (_int, [_str, _int, _int, _ptr, _ptr]),
    "derp_render_format": (_int, [_ptr, _str, _view, _ptr, _ptr, _int, _int, _ptr]),
    "derp_render_vertices": (_int, [_ptr, _int, _f32, _ptr]),
    "derp_stream_upload": (_int, [_ptr, _int, _ptr, _size, _ptr, _size, _ptr, _int, _int]),
    "derp_stream_clear": (_int, [_ptr]),
    "derp_stream_render": (_int, [_ptr, _view, _ptr, _f32, _ptr]),
    "derp_stream_vertices": (_int, [_ptr, _int, _view, _int, _ptr]),
    "derp_stream_srgb_table": (None, [_ptr]),
    "derp_export_points": (_int, [_ptr, _int, _ptr, _int, _int, _ptr, _f64, _int, _int, _ptr, _size, _ptr]),
    "derp_points_begin": (_int, [_ptr, _ptr, _ptr]),
    "derp_points_splat": (_int, [_ptr, _ptr, _size, _f64, _f64]),
    "derp_points_download": (_int, [_ptr, _int, _ptr]),
    "derp_project_equirect_mask": (_int, [_ptr, _int, _ptr, _int, _int, _int, _int, _f64, _ptr]),
    "derp_mesh_build": (_int, [_ptr, _int, _ptr, _int, _int, _ptr, _f64, _ptr, _int, _int, _f32]),
    "derp_mesh_build_equirect": (_int, [_ptr, _ptr, _int, _int, _f32, _f32]),
    "derp_mesh_counts": (_int, [_ptr, _ptr, _ptr, _ptr]),
    "derp_mesh_setup": (_int, [_ptr, _int, _ptr, _ptr, _ptr]),
    "derp_mesh_simplify": (_int, [_ptr, _int, _f32, _int, _int, _int, _ptr]),
    "derp_mesh_simplify_parallel": (_int, [_ptr, _int, _f32, _int, _int, _ptr]),
    "derp_mesh_parallel_pass": (_int, [_ptr, _int, _pass]),
    "derp_mesh_download_f64": (_int, [_ptr, _ptr, _ptr]),
    "derp_mesh_download": (_int, [_ptr, _int, _ptr, _ptr]),
    "derp_gc_upload": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr, _ptr]),
    "derp_gc_download_image": (_int, [_ptr, _int, _ptr]),
    "derp_gc_slices": (_int, [_ptr, _int, _f64, _ptr, _ptr, _int]),
    "derp_gc_slice_count": (_int, [_cam, _int, _int, _int, _int, _f64, _ptr]),
    "derp_gc_set_clean": (_int, [_ptr, _ptr]),
    "derp_gc_sweep": (_int, [_ptr, _int, _f64, _int, _f64, _int, _ptr]),
    "derp_gc_clean": (_int, [_ptr, _ptr, _ptr, _ptr, _f64, _ptr]),
    "derp_gc_run": (_int, [_ptr, _f64, _f64, _int, _int]),
    "derp_gc_result": (_int, [_ptr, _int, _int, _int, _ptr]),
    "derp_gc_stage": (_int, [_ptr, _int, _int, _int, _f64, _int, _f64, _ptr, _ptr, _ptr, _ptr]),
    "derp_sweep_upload": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr]),
    "derp_sweep_overlaps": (_int, [_ptr, _int, _ptr, _int, _int, _ptr]),
    "derp_sweep_equirect_bounds": (_int, [_ptr, _int, _int, _f32, _ptr]),
    "derp_sweep_equirect": (_int, [_ptr, _int, _int, _ptr, _int, _int, _ptr, _int, _ptr, _int, _ptr]),
    "derp_sweep_overlap_disparities": (_int, [_int, _u64, _u64, _ptr, _ptr]),
    "derp_sweep_equirect_depths": (_int, [_int, _f64, _f64, _ptr, _ptr]),
    "derp_sweep_crop_size": (_int, [_int, _ptr, _ptr]),
    "derp_rig_center": (_int, [_cam, _int, _int, _cam]),
    "derp_coverage_directions": (_int, [_ptr, _ptr, _int, _ptr, _int, _ptr, _ptr]),
    "derp_coverage_equirect": (_int, [_ptr, _int, _f64, _ptr, _ptr, _ptr]),
    "derp_coverage_camera": (_int, [_ptr, _int, _f64, _ptr]),
    "derp_coverage_cross_section": (_int, [_ptr, _int, _ptr]),
    "derp_rig_fibonacci_units": (_int, [_int, _f64, _ptr, _ptr]),
    "derp_rig_coverage_distances": (_int, [_f64, _ptr]),
    "derp_rig_euler_matrix": (_int, [_ptr, _int, _ptr]),
    "derp_rig_align_z_matrix": (_int, [_ptr, _ptr]),
    "derp_rig_from_eulers": (_int, [_cam, _ptr, _int, _int, _cam]),
    "derp_rig_arrangement": (_int, [_str, _cam, _f64, _cam, _ptr]),
    "derp_rig_revolve": (_int, [_cam, _int, _ptr, _int, _cam]),
    "derp_rig_rotate": (_int, [_cam, _int, _ptr, _cam]),
    "derp_rig_perturb": (_int, [_cam, _int, _int, _f64, _f64, _f64, _f64]),
    "derp_rig_scale": (_int, [_cam, _int, _f64, _f64, _f64]),
    "derp_align_derive_cameras": (_int, [_cam, _cam, _cam, _cam, _cam, _cam]),
    "derp_align_setup": (_int, [_ptr, _cam, _int, _cam, _int, _cam, _int]),
    "derp_align_maps": (_int, [_ptr, _int, _ptr, _ptr]),
    "derp_align_frame": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr]),
    "derp_mesh_setup_host": (_int, [_ptr, _size, _ptr, _size, _int, _ptr, _ptr, _ptr]),
    "derp_mesh_simplify_host": (_int, [_ptr, _size, _ptr, _size, _ptr, _ptr, _ptr, _int, _f32, _int, _int, _ptr, _ptr, _ptr,
                                      _ptr, _ptr]),
    "derp_mesh_texcoords_equirect": (_int, [_ptr, _size, _ptr]),
    "derp_fov_mask": (_int, [_ptr, _int, _int, _int, _ptr]),
    "derp_upsample_disparity": (_int, [_ptr, _int, _ptr, _int, _int, _ptr, _ptr, _ptr, _int, _int, _int, _ptr]),
    "derp_joint_bilateral_u16": (_int, [_ptr, _ptr, _ptr, _ptr, _int, _int, _int, _f32, _f32, _f32, _f32, _ptr]),
    "derp_joint_bilateral_f32": (_int, [_ptr, _ptr, _ptr, _ptr, _int, _int, _int, _f32, _f32, _f32, _f32, _ptr]),
    "derp_masked_median": (_int, [_ptr, _ptr, _ptr, _ptr, _int, _int, _int, _ptr]),
    "derp_temporal_filter": (_int, [_ptr, _ptr, _ptr, _ptr, _int, _int, _int, _int, _f32, _int, _f32, _f32, _f32, _ptr]),
    "derp_temporal_filter_dev": (_int, [_ptr, _ptr, _ptr, _ptr, _int, _int, _int, _int, _f32, _int, _f32, _f32, _f32, _ptr]),
    "derp_dev_disparity": (_int, [_ptr, _int, _int, _ptr, _ptr]),
    "derp_dev_color": (_int, [_ptr, _int, _int, _ptr, _ptr]),
    "derp_dev_mask": (_int, [_ptr, _int, _int, _ptr, _ptr]),
    "derp_seq_options_default": (None, [_seq_opt]),
    "derp_seq_window": (None, [_int, _int, _int, _int, _ptr, _ptr]),
    "derp_seq_owner": (_int, [_int, _int, _int, _int, _int]),
    "derp_seq_plan": (_int, [_int, _int, _int, _int, _int, _transfer, _int]),
    "derp_seq_create": (_int, [_ptr, _ptr, _int, _int, _int, _int, _seq_opt]),
    "derp_seq_destroy": (None, [_ptr]),
    "derp_seq_counts": (_int, [_ptr, _ptr, _ptr]),
    "derp_seq_frames": (_int, [_ptr, _int, _ptr, _int]),
    "derp_seq_frame_slot": (_int, [_ptr, _int]),
    "derp_seq_host_inputs": (_int, [_ptr, _int, _int, _ptr, _ptr, _ptr]),
    "derp_seq_upload_color_plane": (_int, [_ptr, _int, _int, _int, _ptr]),
    "derp_seq_upload_disparity": (_int, [_ptr, _int, _int, _int, _ptr]),
    "derp_seq_download_disparity": (_int, [_ptr, _int, _int, _int, _ptr]),
    "derp_seq_buffer": (_int, [_ptr, _int, _int, _int, _ptr, _ptr]),
    "derp_seq_buffer_copy": (_int, [_ptr, _int, _int, _int, _ptr, _size, _int]),
    "derp_rccl_unique_id": (_int, [_ptr, _size]),
    "derp_seq_attach_rccl": (_int, [_ptr, _ptr, _size]),
    "derp_seq_attach_loopback": (_int, [_ptr, _ptr, _int]),
    "derp_seq_attach_external": (_int, [_ptr]),
    "derp_seq_selftest": (_int, [_ptr, _int]),
    "derp_seq_exchange_inputs": (_int, [_ptr]),
    "derp_seq_exchange_inputs_level": (_int, [_ptr, _int]),
    "derp_seq_level_compute": (_int, [_ptr, _int]),
    "derp_seq_level_compute_frame": (_int, [_ptr, _int, _int]),
    "derp_seq_level_provided_frame": (_int, [_ptr, _int, _int]),
    "derp_seq_level_exchange": (_int, [_ptr, _int]),
    "derp_seq_mark_exchanged": (_int, [_ptr, _int]),
    "derp_seq_level_filter": (_int, [_ptr, _int]),
    "derp_seq_level_filter_frame": (_int, [_ptr, _int, _int]),
    "derp_seq_download_filtered": (_int, [_ptr, _int, _int, _int, _ptr]),
    "derp_seq_run": (_int, [_ptr, _int, _int]),
    "derp_seq_stats": (_int, [_ptr, _ptr, _ptr, _ptr]),
    "derp_seq_stats_reset": (_int, [_ptr]),
    "derp_seq_exchange_exposed_ms": (_int, [_ptr, _ptr]),
    "derp_isp_config_default": (None, [_isp]),
    "derp_isp_create": (_int, [_ptr, _int, _isp, _int, _int, _int]),
    "derp_isp_destroy": (None, [_ptr]),
    "derp_isp_output_size": (_int, [_ptr, _ptr, _ptr]),
    "derp_isp_process": (_int, [_ptr, _ptr, _size, _ptr]),
    "derp_isp_stage": (_int, [_ptr, _int, _ptr]),
    "derp_isp_tables": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr]),
    "derp_sim_scene_create": (_ptr, []),
    "derp_sim_scene_destroy": (None, [_ptr]),
    "derp_sim_scene_icosahedrons": (_int, [_ptr, _int, _f64, _f64, _f64, _f64, _int]),
    "derp_sim_scene_cubes": (_int, [_ptr]),
    "derp_sim_scene_ground_plane": (_int, [_ptr, _f64]),
    "derp_sim_scene_add_triangle": (_int, [_ptr, _ptr, _ptr, _ptr, _ptr]),
    "derp_sim_bvh_build": (_int, [_ptr, _int, _int, _int]),
    "derp_sim_scene_counts": (_int, [_ptr, _ptr, _ptr, _ptr]),
    "derp_sim_scene_get": (_int, [_ptr, _ptr, _ptr, _ptr]),
    "derp_sim_perlin_table": (None, [_ptr]),
    "derp_sim_icosahedron": (None, [_ptr, _ptr]),
    "derp_sim_noise": (_int, [_ptr, _int, _int, _f64]),
    "derp_sim_trace_host": (_int, [_ptr, _ptr, _size, _ptr]),
    "derp_sim_create": (_int, [_ptr, _int]),
    "derp_sim_destroy": (None, [_ptr]),
    "derp_sim_upload": (_int, [_ptr, _ptr, _int, _ptr, _int, _ptr, _int, _ptr, _int, _int, _ptr, _int, _int, _sim]),
    "derp_sim_render_camera": (_int, [_ptr, _cam, _int, _ptr, _ptr]),
    "derp_sim_render_equirect": (_int, [_ptr, _int, _int, _int, _int, _f64, _ptr, _ptr, _ptr]),
    "derp_sim_trace_rays": (_int, [_ptr, _ptr, _size]),
    "derp_sim_stage_size": (_int, [_ptr, _ptr, _ptr]),
    "derp_sim_stage": (_int, [_ptr, _int, _int, _ptr]),
    "derp_get_counters": (_int, [_ptr, _ptr, _ptr, _ptr]),
    "derp_reset_counters": (_int, [_ptr]),
    "derp_profile_enable": (_int, [_ptr, _int]),
    "derp_profile_reset": (_int, [_ptr]),
    "derp_profile_query": (_int, [_ptr, _str, _int, _ptr, _ptr, _ptr, _ptr]),
    "derp_profile_memoised": (_int, [_ptr, _str, _int, _ptr]),
    "derp_device_name": (_int, [_ptr, _str, _int]),
    "derp_device_memory": (_int, [_ptr, _ptr, _ptr]),
    "derp_host_nth_element_pairs": (_int, [_ptr, _int, _int]),
    "derp_host_minstd_uniform": (_f32, [_int, _u64, _f32, _f32]),
    "derp_host_cost_tile_map": (_int, [_int, _int, _int, _int, _ptr, _int]),
    "derp_host_table_batch": (_int, [_int, _u64, _u64, _int, _u64, _ptr, _ptr]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/derp_hip.h declares

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libderp_hip.so is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the depth path."
            )
        # One HIP runtime per process: PyTorch-ROCm preloads its bundled libamdhip64 by path, and a
        # second copy (the system one this library would otherwise pull in) cannot open the device.
        # Importing torch first makes libderp_hip.so bind to the runtime torch already loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(_lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return _lib


def camera_desc(cam):
    j = CameraDesc()
    j.type = CAM_TYPES[cam["type"]]
    for k in ("origin", "forward", "up", "right", "resolution", "focal"):
        for i, v in enumerate(cam[k]):
            getattr(j, k)[i] = float(v)
    j.has_principal = int("principal" in cam)
    if "principal" in cam:
        j.principal[0], j.principal[1] = map(float, cam["principal"])
    j.has_distortion = int("distortion" in cam)
    if "distortion" in cam:
        d = list(cam["distortion"]) + [0.0] * (3 - len(cam["distortion"]))
        for i in range(3):
            j.distortion[i] = float(d[i])
    j.has_fov = int("fov" in cam)
    if "fov" in cam:
        j.fov = float(cam["fov"])
    j.id = cam["id"].encode()
    return j


def filter_destinations(cams, destinations):
    """image_util::filterDestinations (source/util/ImageUtil.cpp:110-125)."""
    if not destinations:
        return list(cams)
    out = []
    for dest in destinations.split(","):
        for cam in cams:
            if cam["id"] == dest:
                out.append(cam)
    return out


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ptrs(arrays):
    """T* const*: the arrays' addresses (the caller keeps the arrays alive)"""
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _ints(values):
    return (C.c_int * len(values))(*values)


class DerpError(RuntimeError):
    pass


class Derp:
    """One context per GPU (derp_create .. derp_destroy)."""

    def __init__(self, cams_src, cams_dst=None, device=0, **options):
        cams_dst = cams_src if cams_dst is None else cams_dst
        self.cams_src, self.cams_dst = list(cams_src), list(cams_dst)
        self.S, self.D = len(self.cams_src), len(self.cams_dst)
        a = (CameraDesc * self.S)(*[camera_desc(c) for c in self.cams_src])
        b = (CameraDesc * self.D)(*[camera_desc(c) for c in self.cams_dst])
        h = C.c_void_p()
        if lib().derp_create(C.byref(h), device, a, self.S, b, self.D):
            raise DerpError(lib().derp_last_error(None).decode())
        self.h = h
        self._seqs = []  # derp_seq objects living on this context (destroyed first)
        self.sizes = None
        self.opt = Options()
        lib().derp_options_default(C.byref(self.opt))
        self.set_options(**options)

    def close(self):
        if getattr(self, "h", None):
            for ref in list(getattr(self, "_seqs", [])):
                seq = ref()
                if seq is not None:
                    seq.close()
            lib().derp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise DerpError(lib().derp_last_error(self.h).decode())

    def set_options(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.opt, k):
                raise KeyError(k)
            setattr(self.opt, k, type(getattr(self.opt, k))(v))
        self._ck(lib().derp_set_options(self.h, C.byref(self.opt)))

    def set_pyramid(self, sizes, width_full, height_full):
        sizes = list(sizes)
        self._ck(lib().derp_set_pyramid(self.h, len(sizes), _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes]),
                                        width_full, height_full))
        self.sizes = sizes  # (a refused call, e.g. with a SequenceRunner still open, leaves the geometry as it was)

    def _shape(self, level):
        w, h = self.sizes[level]
        return h, w

    def upload_color(self, level, s, bgr):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint16)
        assert bgr.shape == self._shape(level) + (3,)
        self._ck(lib().derp_upload_color(self.h, level, s, _p(bgr)))

    def upload_foreground_mask(self, level, s, mask):
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        assert mask.shape == self._shape(level)
        self._ck(lib().derp_upload_foreground_mask(self.h, level, s, _p(mask)))

    def upload_background_disparity(self, level, d, disp):
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        assert disp.shape == self._shape(level)
        self._ck(lib().derp_upload_background_disparity(self.h, level, d, _p(disp)))

    def upload_disparity(self, level, d, disp):
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        assert disp.shape == self._shape(level)
        self._ck(lib().derp_upload_disparity(self.h, level, d, _p(disp)))

    # ---- pyramid builder (scripts/render/resize.py)
    def build_pyramid_color(self, s, bgr):
        bgr = np.ascontiguousarray(bgr, dtype=np.uint16)
        self._ck(lib().derp_build_pyramid_color(self.h, s, _p(bgr), bgr.shape[1], bgr.shape[0]))

    def build_pyramid_foreground_mask(self, s, mask_u8, threshold=127):
        mask_u8 = np.ascontiguousarray(mask_u8, dtype=np.uint8)
        self._ck(lib().derp_build_pyramid_foreground_mask(self.h, s, _p(mask_u8), mask_u8.shape[1], mask_u8.shape[0],
                                                          threshold))

    def build_pyramid_background_disparity(self, d, disp):
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        self._ck(lib().derp_build_pyramid_background_disparity(self.h, d, _p(disp), disp.shape[1], disp.shape[0]))

    def download_level_color(self, level, s):
        out = np.zeros(self._shape(level) + (3,), dtype=np.uint16)
        self._ck(lib().derp_download_level_color(self.h, level, s, _p(out)))
        return out

    def download_level_mask(self, level, s):
        out = np.zeros(self._shape(level), dtype=np.uint8)
        self._ck(lib().derp_download_level_mask(self.h, level, s, _p(out)))
        return out

    def download_level_background(self, level, d):
        out = np.zeros(self._shape(level), dtype=np.float32)
        self._ck(lib().derp_download_level_background(self.h, level, d, _p(out)))
        return out

    def resize_area(self, src, dw, dh):
        src = np.ascontiguousarray(src)
        kind = {(np.dtype(np.uint16), 3): 0, (np.dtype(np.uint8), 2): 1, (np.dtype(np.float32), 2): 2,
                (np.dtype(np.float32), 3): 3}[(src.dtype, src.ndim)]
        out = np.zeros((dh, dw, 3) if kind in (0, 3) else (dh, dw), dtype=src.dtype)
        self._ck(lib().derp_resize_area(self.h, kind, _p(src), src.shape[1], src.shape[0], _p(out), dw, dh))
        return out

    def generate_foreground_mask(self, template, frame, blur_radius=1, threshold=0.04, morph_closing_size=4):
        template = np.ascontiguousarray(template, dtype=np.uint16)
        frame = np.ascontiguousarray(frame, dtype=np.uint16)
        h, w = frame.shape[:2]
        out = np.zeros((h, w), dtype=np.uint8)
        self._ck(lib().derp_generate_foreground_mask(self.h, _p(template), _p(frame), w, h, blur_radius,
                                                     threshold, morph_closing_size, _p(out)))
        return out

    # ---- tuning previews (ViewColorVarianceThresholds, ViewForegroundMaskThresholds)
    def preview_variance(self, bgr, low_show, high_show, with_variance=False):
        """n marked copies [n][h][w][3] of a BGR u16 image and counts [n][2] (blue, purple); the variance on request"""
        bgr = np.ascontiguousarray(bgr, dtype=np.uint16)
        low_show = np.ascontiguousarray(low_show, dtype=np.float32).reshape(-1)
        high_show = np.ascontiguousarray(high_show, dtype=np.float32).reshape(-1)
        assert bgr.ndim == 3 and bgr.shape[2] == 3 and low_show.size == high_show.size
        h, w = bgr.shape[:2]
        n = low_show.size
        out = np.zeros((n, h, w, 3), dtype=np.uint16)
        counts = np.zeros((n, 2), dtype=np.uint32)
        var = np.zeros((h, w), dtype=np.float32) if with_variance else None
        self._ck(lib().derp_preview_variance(self.h, _p(bgr), w, h, _p(low_show), _p(high_show), n, _p(out), _p(counts),
                                             _p(var)))
        return (out, counts, var) if with_variance else (out, counts)

    def preview_foreground(self, template, frame, blur_radii=(1,), thresholds=(0.04,), closing_sizes=(4,)):
        """overlays [nb*nt*nc][h][w][3], masks [..][h][w] and counts [..] of every (blur, threshold, closing), blur-major"""
        template = np.ascontiguousarray(template, dtype=np.uint16)
        frame = np.ascontiguousarray(frame, dtype=np.uint16)
        assert template.shape == frame.shape and frame.ndim == 3 and frame.shape[2] == 3
        blur = np.ascontiguousarray(blur_radii, dtype=np.int32).reshape(-1)
        thr = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
        close = np.ascontiguousarray(closing_sizes, dtype=np.int32).reshape(-1)
        h, w = frame.shape[:2]
        n = max(blur.size * thr.size * close.size, 1)
        out = np.zeros((n, h, w, 3), dtype=np.uint16)
        masks = np.zeros((n, h, w), dtype=np.uint8)
        counts = np.zeros(n, dtype=np.uint32)
        self._ck(lib().derp_preview_foreground(self.h, _p(template), _p(frame), w, h, _p(blur), blur.size, _p(thr), thr.size,
                                               _p(close), close.size, _p(out), _p(masks), _p(counts)))
        return out, masks, counts

    def preview_keypoints(self, c0, c1, with_float=False, **params):
        """GenerateKeypointProjections for the pair (c0, c1) after sweep_upload at scale 1 -> (u8 BGRA [h][w][4],
        rectangles drawn), with the float blend in between on request"""
        shapes = getattr(self, "_sweep_shapes", [])
        if not 0 <= c0 < len(shapes):
            raise DerpError("sweep_upload has not been called, or bad camera index %d" % c0)
        p = keypoint_params(**params)
        out = np.zeros(tuple(shapes[c0]) + (4,), dtype=np.uint8)
        flt = np.zeros(tuple(shapes[c0]) + (4,), dtype=np.float32) if with_float else None
        n = C.c_int(0)
        self._ck(lib().derp_preview_keypoints(self.h, c0, c1, _p(p), _p(out), _p(flt), C.byref(n)))
        return (out, flt, n.value) if with_float else (out, n.value)

    # ---- frame slots
    def set_frame_slots(self, n):
        self._ck(lib().derp_set_frame_slots(self.h, n))

    def select_frame(self, slot):
        self._ck(lib().derp_select_frame(self.h, slot))

    def frame_slots(self):
        n, cur = C.c_int(), C.c_int()
        self._ck(lib().derp_frame_slots(self.h, C.byref(n), C.byref(cur)))
        return n.value, cur.value

    def upload_frame(self, frame):
        """frame: dict from synth.make_frame (color[level][cam], optional masks / bg_disp)."""
        for level in range(len(self.sizes)):
            for s in range(self.S):
                self.upload_color(level, s, frame["color"][level][s])
                if frame.get("masks"):
                    self.upload_foreground_mask(level, s, frame["masks"][level][s])
            if frame.get("bg_disp"):
                for d in range(self.D):
                    self.upload_background_disparity(level, d, frame["bg_disp"][level][self._dst_src(d)])

    def _dst_src(self, d):
        ids = [c["id"] for c in self.cams_src]
        return ids.index(self.cams_dst[d]["id"])

    def process_level(self, level):
        self._ck(lib().derp_process_level(self.h, level))

    def process_pyramid(self, level_start=None, level_end=0):
        level_start = len(self.sizes) - 1 if level_start is None else level_start
        self._ck(lib().derp_process_pyramid(self.h, level_start, level_end))

    def synchronize(self):
        self._ck(lib().derp_synchronize(self.h))

    def download_disparity(self, level, d):
        out = np.zeros(self._shape(level), dtype=np.float32)
        self._ck(lib().derp_download_disparity(self.h, level, d, _p(out)))
        return out

    def download_cost(self, level, d):
        cost = np.zeros(self._shape(level), dtype=np.float32)
        conf = np.zeros(self._shape(level), dtype=np.float32)
        self._ck(lib().derp_download_cost(self.h, d, _p(cost), _p(conf)))
        return cost, conf

    # ---- stage-level
    def level_begin(self, level):
        self._cur = level
        self._ck(lib().derp_level_begin(self.h, level))

    def stage(self, name):
        fn = {
            "reproject_colors": "derp_stage_reproject_colors", "brute_force": "derp_stage_brute_force",
            "random_proposals": "derp_stage_random_proposals", "ping_pong": "derp_stage_ping_pong",
            "mismatches": "derp_stage_mismatches", "bilateral": "derp_stage_bilateral_filter", "median": "derp_stage_median_filter",
            "mask_fov": "derp_stage_mask_fov", "end": "derp_level_end",
        }[name]
        self._ck(getattr(lib(), fn)(self.h))

    def set_level_disparity(self, d, disp):
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        self._ck(lib().derp_set_level_disparity(self.h, d, _p(disp)))

    def get_level_disparity(self, d):
        out = np.zeros(self._shape(self._cur), dtype=np.float32)
        self._ck(lib().derp_get_level_disparity(self.h, d, _p(out)))
        return out

    def cost_map(self, d, disp):
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        cost = np.zeros(self._shape(self._cur), dtype=np.float32)
        conf = np.zeros(self._shape(self._cur), dtype=np.float32)
        self._ck(lib().derp_cost_map(self.h, d, _p(disp), _p(cost), _p(conf)))
        return cost, conf

    def debug_atan2_ypos(self, y, x):
        """The cost kernels' own fp64 atan2(y >= 0, x) evaluated on the device."""
        y = np.ascontiguousarray(y, np.float64)
        x = np.ascontiguousarray(x, np.float64)
        out = np.zeros_like(y)
        self._ck(lib().derp_debug_atan2_ypos(self.h, _p(y), _p(x), _p(out), y.size))
        return out

    FP64_OPS = {"sqrt_lean": 0, "sqrt": 1, "div_plain": 2, "div": 3}

    def debug_fp64(self, op, a, b=None):
        """One of the cost kernels' fp64 primitives (FP64_OPS) evaluated on the device, element by element."""
        a = np.ascontiguousarray(a, np.float64)
        b = None if b is None else np.ascontiguousarray(b, np.float64)
        assert b is None or b.shape == a.shape
        out = np.zeros_like(a)
        self._ck(lib().derp_debug_fp64(self.h, self.FP64_OPS[op], _p(a), _p(b), _p(out), a.size))
        return out

    def debug_expf(self, x, nonpos=False):
        """The filters' expf on the device, element by element: the full routine, or (nonpos) the form with one range
        test that stands in for it on arguments in [-inf, -0]."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        self._ck(lib().derp_debug_expf(self.h, int(bool(nonpos)), _p(x), _p(out), x.size))
        return out

    def debug_round_half_away(self, x):
        """The cost kernels' roundf (round_half_away_pos) on the device, element by element."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        self._ck(lib().derp_debug_expf(self.h, 2, _p(x), _p(out), x.size))
        return out

    def debug_sees(self, src, xyz):
        """Camera::sees of source camera `src` as the cost kernels evaluate it -> (vis [2, n] bool, pix [2, n, 2] f64):
        row 0 the ping-pong / brute-force variant, row 1 the random-proposal variant (NaN pixels outside the FOV cone)."""
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        out = np.zeros((len(xyz), 2, 3))
        self._ck(lib().derp_debug_sees(self.h, src, _p(xyz), len(xyz), _p(out)))
        return out[:, :, 0].T != 0, np.ascontiguousarray(out[:, :, 1:].transpose(1, 0, 2))

    def debug(self, d, s, which):
        h, w = self._shape(self._cur)
        spec = {"warp": (0, (h, w, 2), np.float32), "color": (2, (h, w, 3), np.uint16),
                "bias": (3, (h, w, 3), np.uint16), "variance": (4, (h, w), np.float32),
                "fov": (5, (h, w), np.uint8),
                # the colour tables as stored (2-texel replicated ring, u16 x 4 texels) and their blank-tile flags
                "color_padded": (6, (h + 4, w + 4, 4), np.uint16), "bias_padded": (7, (h + 4, w + 4, 4), np.uint16),
                "tile_seen": (8, ((h + 31) // 32, (w + 31) // 32), np.uint8),
                # source s's own colour bias; destination d's engine states in front of its gated-in pixels (minstd_rand0,
                # written by the random-proposal stage; the other pixels hold nothing meaningful)
                "own_bias": (9, (h, w, 3), np.uint16), "rank": (10, (h, w), np.uint32)}[which]
        out = np.zeros(spec[1], dtype=spec[2])
        self._ck(lib().derp_debug_download(self.h, d, s, spec[0], _p(out)))
        return out

    def mismatch_mask(self, d):
        out = np.zeros(self._shape(self._cur), dtype=np.uint8)
        self._ck(lib().derp_download_mismatch_mask(self.h, d, _p(out)))
        return out

    # ---- sibling kernels
    def layer_disparities(self, fg, bg):
        fg = np.ascontiguousarray(fg, dtype=np.float32)
        bg = np.ascontiguousarray(bg, dtype=np.float32)
        out = np.zeros(fg.shape, dtype=np.uint8)
        self._ck(lib().derp_layer_disparities(self.h, _p(fg), _p(bg), fg.size, _p(out)))
        return out

    # ---- rephotography score (RephotographyUtil.h, ComputeRephotographyErrors.cpp)
    def ssim(self, x, y, blur_radius=1, alpha=1.0, beta=1.0, gamma=1.0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        h, w = x.shape[:2]
        out = np.zeros((h, w, 3), dtype=np.float32)
        self._ck(lib().derp_ssim(self.h, _p(x), _p(y), w, h, blur_radius, alpha, beta, gamma, _p(out)))
        return out

    def rephotograph(self, target, colors, disps):
        """colors[s] u16 [h, w, 3], disps[s] f32 [h, w] for every source camera -> BGRA f32 [h, w, 4]."""
        colors = [np.ascontiguousarray(c, dtype=np.uint16) for c in colors]
        disps = [np.ascontiguousarray(d, dtype=np.float32) for d in disps]
        h, w = disps[0].shape
        out = np.zeros((h, w, 4), dtype=np.float32)
        self._ck(lib().derp_rephotograph(self.h, target, _ptrs(colors), _ptrs(disps), w, h, _p(out)))
        return out

    def rephotograph_upload(self, colors, disps):
        colors = [np.ascontiguousarray(c, dtype=np.uint16) for c in colors]
        disps = [np.ascontiguousarray(d, dtype=np.float32) for d in disps]
        h, w = disps[0].shape
        self._ck(lib().derp_rephotograph_upload(self.h, _ptrs(colors), _ptrs(disps), w, h))

    def canopy_cubemap(self, include, centre, edge):
        """CanopyScene::cubemap of the uploaded cameras with include[s] != 0, seen from `centre`
        -> BGRA f32 [6 * edge, edge, 4]."""
        inc = np.ascontiguousarray(include, dtype=np.uint8)
        ctr = np.ascontiguousarray(centre, dtype=np.float64)
        out = np.zeros((6 * edge, edge, 4), dtype=np.float32)
        self._ck(lib().derp_canopy_cubemap(self.h, _p(inc), _p(ctr), edge, _p(out)))
        return out

    def render_upload(self, disps, colors=None):
        """SimpleMeshRenderer's scene: disps[s] f32 [h, w], colors[s] float BGRA [h', w', 4] (own sizes) or None."""
        disps = [np.ascontiguousarray(d, dtype=np.float32) for d in disps]
        dp, dw, dh = _ptrs(disps), _ints([d.shape[1] for d in disps]), _ints([d.shape[0] for d in disps])
        if colors is None:
            self._ck(lib().derp_render_upload(self.h, None, None, None, dp, dw, dh))
            return
        colors = [np.ascontiguousarray(c, dtype=np.float32) for c in colors]
        assert all(c.ndim == 3 and c.shape[2] == 4 for c in colors)
        self._ck(lib().derp_render_upload(self.h, _ptrs(colors), _ints([c.shape[1] for c in colors]),
                                          _ints([c.shape[0] for c in colors]), dp, dw, dh))

    def render(self, params, include=None):
        """derp_render of the uploaded scene -> BGRA f32: cube [6 h, h, 4], equirect [h, 2 h, 4], snapshot [h, w, 4]."""
        h = params.height
        w = {0: h, 1: 2 * h, 2: params.width}[params.kind]
        out = np.zeros((6 * h if params.kind == 0 else h, w, 4), dtype=np.float32)
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.uint8)
        self._ck(lib().derp_render(self.h, C.byref(params), None if inc is None else _p(inc), _p(out)))
        return out

    def render_format(self, fmt, params, background=None, background_equirect=None):
        """One SimpleMeshRenderer --format, stacked and composited -> BGRA f32."""
        w, h = render_format_size(fmt, params.width, params.height)
        out = np.zeros((h, w, 4), dtype=np.float32)
        bg = None if background is None else np.ascontiguousarray(background, dtype=np.float32)
        eq = None if background_equirect is None else np.ascontiguousarray(background_equirect, dtype=np.float32)
        assert bg is None or bg.shape == out.shape
        self._ck(lib().derp_render_format(self.h, fmt.encode(), C.byref(params), None if bg is None else _p(bg),
                                          None if eq is None else _p(eq), 0 if eq is None else eq.shape[1],
                                          0 if eq is None else eq.shape[0], _p(out)))
        return out

    def render_vertices(self, cam, shape, ipd):
        """camera `cam`'s mesh vertices after canopyVS's stereo stage (ipd 0: none) -> f32 [h, w, 4]."""
        out = np.zeros((shape[0], shape[1], 4), dtype=np.float32)
        self._ck(lib().derp_render_vertices(self.h, cam, ipd, _p(out)))
        return out

    # ---- MeshStreamRenderer (RigScene's mesh path): cameras = this context's destinations, at the colour's size
    def stream_upload(self, cam, vtx, idx, rgba):
        """camera `cam`'s mesh of one frame: vtx f32 [n, 3] (a, b, c), idx u32 [m] or [m / 3, 3], rgba u8 [h, w, 4]"""
        vtx = np.ascontiguousarray(vtx, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert rgba.ndim == 3 and rgba.shape[2] == 4
        self._ck(lib().derp_stream_upload(self.h, cam, _p(vtx) if len(vtx) else None, len(vtx),
                                          _p(idx) if len(idx) else None, len(idx), _p(rgba), rgba.shape[1], rgba.shape[0]))

    def stream_clear(self):
        self._ck(lib().derp_stream_clear(self.h))

    def stream_render(self, params, include=None, fade=1.0):
        """derp_stream_render of the uploaded meshes -> BGRA f32, the shapes of render()"""
        h = params.height
        w = {0: h, 1: 2 * h, 2: params.width}[params.kind]
        out = np.zeros((6 * h if params.kind == 0 else h, w, 4), dtype=np.float32)
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.uint8)
        self._ck(lib().derp_stream_render(self.h, C.byref(params), None if inc is None else _p(inc), fade, _p(out)))
        return out

    def stream_vertices(self, cam, count, params, face=0):
        """clip coordinates of camera `cam`'s `count` uploaded vertices in params' view -> f32 [count, 4]"""
        out = np.zeros((count, 4), dtype=np.float32)
        self._ck(lib().derp_stream_vertices(self.h, cam, C.byref(params), face, _p(out)))
        return out

    # ---- conversion tools (source/conversion): cameras = this context's destinations, rescaled to the image size
    def export_points(self, cam, disparity, color_bgr, max_depth=float("inf"), clip=False, subsample=1, cap=None):
        """getPoints of ExportPointCloud for one camera: disparity f32 [h, w] + colour float BGR [h, w, 3] in 0..1
        -> f32 [count, 6] rows of x y z r g b in row-major pixel order. `cap` (points) defaults to every pixel."""
        disparity = np.ascontiguousarray(disparity, dtype=np.float32)
        color_bgr = np.ascontiguousarray(color_bgr, dtype=np.float32)
        h, w = disparity.shape
        assert color_bgr.shape == (h, w, 3)
        cap = h * w if cap is None else cap
        out = np.zeros((cap, 6), dtype=np.float32)
        count = C.c_size_t()
        rc = lib().derp_export_points(self.h, cam, _p(disparity), w, h, _p(color_bgr), max_depth, int(clip),
                                      subsample, _p(out), cap, C.byref(count))
        self.last_point_count = count.value
        self._ck(rc)
        return out[:count.value].copy()

    def points_begin(self, sizes):
        """One (w, h) per camera; the disparity images start at zero."""
        assert len(sizes) == self.D
        self._points_sizes = [tuple(s) for s in sizes]
        self._ck(lib().derp_points_begin(self.h, _ints([s[0] for s in sizes]), _ints([s[1] for s in sizes])))

    def points_splat(self, xyz, min_depth=0.0, max_depth=float("inf")):
        """projectPointsToCameras of ImportPointCloud for one chunk of points f64 [n, 3]; chunks accumulate."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self._ck(lib().derp_points_splat(self.h, _p(xyz), len(xyz), min_depth, max_depth))

    def points_download(self, cam):
        sizes = getattr(self, "_points_sizes", [])
        w, h = sizes[cam] if 0 <= cam < len(sizes) else (1, 1)  # (a bad index is the library's to refuse)
        out = np.zeros((h, w), dtype=np.float32)
        self._ck(lib().derp_points_download(self.h, cam, _p(out)))
        return out

    def project_equirect_mask(self, cam, eqr, w, h, depth=1000.0):
        """ProjectEquirectsToCameras for one camera: equirect mask u8 [eh, ew] (non-zero = set) -> u8 {0,1} [h, w]."""
        eqr = np.ascontiguousarray(eqr, dtype=np.uint8)
        out = np.zeros((h, w), dtype=np.uint8)
        self._ck(lib().derp_project_equirect_mask(self.h, cam, _p(eqr), eqr.shape[1], eqr.shape[0], w, h, depth,
                                                  _p(out)))
        return out

    # ---- GeometricConsistency (source/render/GeometricConsistency.cpp): cameras = this context's destinations (the
    # whole rig, not normalised), rescaled to the small sizes
    GC_KINDS = {"iffy": 0, "clean": 1, "depth": 2, "final": 3}

    def gc_upload(self, images, small_sizes):
        """images[cam]: BGRA (or BGR: alpha 65535) u16 [H, W, 4] at full size; small_sizes[cam] = (w, h)."""
        assert len(images) == self.D and len(small_sizes) == self.D
        full = []
        for im in images:
            im = np.asarray(im, dtype=np.uint16)
            if im.shape[2] == 3:
                im = np.concatenate([im, np.full(im.shape[:2] + (1,), 65535, np.uint16)], axis=2)
            full.append(np.ascontiguousarray(im))
        self._gc_sizes = [(int(w), int(h)) for w, h in small_sizes]
        self._ck(lib().derp_gc_upload(self.h, _ptrs(full), _ints([im.shape[1] for im in full]),
                                      _ints([im.shape[0] for im in full]), _ints([s[0] for s in self._gc_sizes]),
                                      _ints([s[1] for s in self._gc_sizes])))

    def _gc_shape(self, cam):
        sizes = getattr(self, "_gc_sizes", [])
        w, h = sizes[cam] if 0 <= cam < len(sizes) else (1, 1)  # (a bad index is the library's to refuse)
        return h, w

    def gc_image(self, cam):
        """the int16 BGRA image of `cam` at its small size: the reference and the texture of the sweep"""
        out = np.zeros(self._gc_shape(cam) + (4,), dtype=np.int16)
        self._ck(lib().derp_gc_download_image(self.h, cam, _p(out)))
        return out

    def gc_slices(self, dst, disparity_step=0.5):
        """-> the slice disparities of `dst`, f32 [sliceCount]"""
        n = C.c_int()
        self._ck(lib().derp_gc_slices(self.h, dst, disparity_step, C.byref(n), None, 0))
        out = np.zeros(n.value, dtype=np.float32)
        self._ck(lib().derp_gc_slices(self.h, dst, disparity_step, C.byref(n), _p(out), n.value))
        return out

    def gc_set_clean(self, clean):
        """clean[cam] f32 [h, w] at the small sizes, or None"""
        if clean is None:
            self._ck(lib().derp_gc_set_clean(self.h, None))
            return
        clean = [np.ascontiguousarray(d, dtype=np.float32) for d in clean]
        assert [d.shape for d in clean] == [self._gc_shape(i) for i in range(self.D)]
        self._ck(lib().derp_gc_set_clean(self.h, _ptrs(clean)))

    def gc_sweep(self, dst, disparity_step=0.5, use_clean=False, agree_fraction=0.75, split=0):
        """computeDepth of one destination -> depth f32 [h, w]"""
        out = np.zeros(self._gc_shape(dst), dtype=np.float32)
        self._ck(lib().derp_gc_sweep(self.h, dst, disparity_step, int(bool(use_clean)), agree_fraction, split,
                                     _p(out)))
        return out

    def gc_clean(self, depths, agree_fraction=0.75):
        """cleanDepth over any per-camera depth maps f32 [h_i, w_i] -> the cleaned maps"""
        depths = [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
        assert len(depths) == self.D
        outs = [np.zeros_like(d) for d in depths]
        self._ck(lib().derp_gc_clean(self.h, _ptrs(depths), _ints([d.shape[1] for d in depths]),
                                     _ints([d.shape[0] for d in depths]), agree_fraction, _ptrs(outs)))
        return outs

    def gc_run(self, disparity_step=0.5, agree_fraction=0.75, pass_count=2, keep_clean=False):
        """processFrame of the uploaded frame; results through gc_result"""
        self._ck(lib().derp_gc_run(self.h, disparity_step, agree_fraction, pass_count,
                                   int(bool(keep_clean))))

    def gc_result(self, kind, cam, pass_index=0):
        """kind: "iffy", "clean" (of pass), "depth" (of pass), "final" -> f32 [h, w]"""
        out = np.zeros(self._gc_shape(cam), dtype=np.float32)
        self._ck(lib().derp_gc_result(self.h, self.GC_KINDS[kind], pass_index, cam, _p(out)))
        return out

    def gc_stage(self, dst, src, slice_index, disparity_step=0.5, use_clean=False, agree_fraction=0.75):
        """-> dict(sample, average, average_of_sq: i16 [h, w, 4]; cost: f32 [h, w]) of one (dst, src, slice)"""
        shape = self._gc_shape(dst)
        out = {k: np.zeros(shape + (4,), dtype=np.int16) for k in ("sample", "average", "average_of_sq")}
        out["cost"] = np.zeros(shape, dtype=np.float32)
        self._ck(lib().derp_gc_stage(self.h, dst, src, slice_index, disparity_step, int(bool(use_clean)),
                                     agree_fraction, _p(out["sample"]), _p(out["average"]),
                                     _p(out["average_of_sq"]), _p(out["cost"])))
        return out

    # ---- camera meshes (source/mesh_stream/ConvertToBinary.cpp:150-245): one mesh per context, the one built last
    def mesh_build(self, cam, disparity, resolution=None, depth_scale=1.0, mask=None, tear_ratio=0.95):
        """convertDepth up to applyMaskToVertexesAndFaces: disparity f32 [h, w], optional foreground mask u8 of any
        size (non-zero = keep), `resolution` = what resizeRig hands Camera::rescale. -> (vertices, faces, faces
        before the mask)."""
        disparity = np.ascontiguousarray(disparity, dtype=np.float32)
        h, w = disparity.shape
        res = None if resolution is None else (C.c_double * 2)(float(resolution[0]), float(resolution[1]))
        mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        mh, mw = (0, 0) if mask is None else mask.shape
        self._ck(lib().derp_mesh_build(self.h, cam, _p(disparity), w, h, res, depth_scale, _p(mask), mw, mh, tear_ratio))
        return self.mesh_counts()

    def mesh_build_equirect(self, disparity, max_depth=700.0, tear_ratio=0.95):
        """getVertexesEquirect + getFaces(wrap, rig coordinates) (MeshUtil.h:264-314) of a disparity equirect f32
        [h, w]: the whole grid as vertices, the seam faces last. The context's cameras are not read; the other mesh_*
        methods then work on this mesh, with equi_error=False. -> (vertices, faces, faces again)."""
        disparity = np.ascontiguousarray(disparity, dtype=np.float32)
        h, w = disparity.shape
        self._ck(lib().derp_mesh_build_equirect(self.h, _p(disparity), w, h, max_depth, tear_ratio))
        return self.mesh_counts()

    def mesh_counts(self):
        nv, nf, raw = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._ck(lib().derp_mesh_counts(self.h, C.byref(nv), C.byref(nf), C.byref(raw)))
        return nv.value, nf.value, raw.value

    def mesh_setup(self, equi_error=True):
        """computeInitialQuadrics on the device -> (face planes f64 [nf, 4], edge costs [nf, 3], vertex quadrics [nv, 10])"""
        nv, nf, _ = self.mesh_counts()
        planes, costs, vq = np.zeros((nf, 4)), np.zeros((nf, 3)), np.zeros((nv, 10))
        self._ck(lib().derp_mesh_setup(self.h, int(equi_error), _p(planes), _p(costs), _p(vq)))
        return planes, costs, vq

    def mesh_simplify(self, num_faces_out, strictness=0.2, remove_boundary_edges=False, equi_error=True, host_setup=False):
        """MeshSimplifier::simplify of the built mesh -> (passes of the loop, DERP_MESH_EXIT_*)"""
        stats = (C.c_int * 2)()
        self._ck(lib().derp_mesh_simplify(self.h, num_faces_out, strictness, int(remove_boundary_edges),
                                          int(equi_error), int(host_setup), stats))
        return stats[0], stats[1]

    def mesh_simplify_parallel(self, num_faces_out, strictness=0.2, remove_boundary_edges=False, equi_error=True):
        """the pass-parallel simplifier of the built mesh, on the device -> (passes, DERP_MESH_EXIT_*)"""
        stats = (C.c_int * 2)()
        self._ck(lib().derp_mesh_simplify_parallel(self.h, num_faces_out, strictness, int(remove_boundary_edges),
                                                   int(equi_error), stats))
        return stats[0], stats[1]

    def mesh_parallel_pass(self, index):
        """-> (alive faces before, feasible edges, winners, winners applied, faces deleted, threshold) of pass `index`"""
        p = MeshPass()
        self._ck(lib().derp_mesh_parallel_pass(self.h, index, C.byref(p)))
        return p.faces, p.feasible, p.winners, p.applied, p.deleted, p.threshold

    def mesh_download_f64(self):
        nv, nf, _ = self.mesh_counts()
        v, f = np.zeros((nv, 3)), np.zeros((nf, 3), dtype=np.int32)
        self._ck(lib().derp_mesh_download_f64(self.h, _p(v), _p(f)))
        return v, f

    def mesh_download(self, clamp_negative_z=False):
        """the .vtx / .idx layouts: f32 [nv, 3], u32 [nf, 3]"""
        nv, nf, _ = self.mesh_counts()
        v, f = np.zeros((nv, 3), dtype=np.float32), np.zeros((nf, 3), dtype=np.uint32)
        self._ck(lib().derp_mesh_download(self.h, int(clamp_negative_z), _p(v), _p(f)))
        return v, f

    def fov_mask(self, d, w, h):
        out = np.zeros((h, w), dtype=np.uint8)
        self._ck(lib().derp_fov_mask(self.h, d, w, h, _p(out)))
        return out

    def upsample_disparity(self, d, disp, w_up, h_up, bg_up=None, fg=None, fg_up=None):
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        h, w = disp.shape
        use = fg is not None
        out = np.zeros((h_up, w_up), dtype=np.float32)
        if use:
            bg_up = np.ascontiguousarray(bg_up, dtype=np.float32)
            fg = np.ascontiguousarray(fg, dtype=np.uint8)
            fg_up = np.ascontiguousarray(fg_up, dtype=np.uint8)
        self._ck(lib().derp_upsample_disparity(self.h, d, _p(disp), w, h, _p(bg_up) if use else None,
                                               _p(fg) if use else None, _p(fg_up) if use else None, w_up, h_up,
                                               int(use), _p(out)))
        return out

    def joint_bilateral_u16(self, image, guide, mask, radius, sigma, w0, w1, w2):
        image = np.ascontiguousarray(image, dtype=np.float32)
        guide = np.ascontiguousarray(guide, dtype=np.uint16)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        h, w = image.shape
        out = np.zeros_like(image)
        self._ck(lib().derp_joint_bilateral_u16(self.h, _p(image), _p(guide), _p(mask), w, h, radius, sigma, w0, w1, w2,
                                                _p(out)))
        return out

    def joint_bilateral_f32(self, image, guide, mask, radius, sigma, w0, w1, w2):
        image = np.ascontiguousarray(image, dtype=np.float32)
        guide = np.ascontiguousarray(guide, dtype=np.float32)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        h, w = image.shape
        out = np.zeros_like(image)
        self._ck(lib().derp_joint_bilateral_f32(self.h, _p(image), _p(guide), _p(mask), w, h, radius, sigma, w0, w1, w2,
                                                _p(out)))
        return out

    def masked_median(self, image, background, mask, radius=1):
        image = np.ascontiguousarray(image, dtype=np.float32)
        background = None if background is None else np.ascontiguousarray(background, dtype=np.float32)
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        h, w = image.shape
        out = np.zeros_like(image)
        self._ck(lib().derp_masked_median(self.h, _p(image), _p(background), _p(mask), w, h, radius, _p(out)))
        return out

    def temporal_filter(self, guides, images, masks, frame_offset, sigma, radius, w0, w1, w2):
        n = len(guides)
        guides = [np.ascontiguousarray(g, dtype=np.uint16) for g in guides]
        images = [np.ascontiguousarray(g, dtype=np.float32) for g in images]
        masks = [np.ascontiguousarray(g, dtype=np.uint8) for g in masks]
        h, w = images[0].shape
        out = np.zeros((h, w), dtype=np.float32)
        self._ck(lib().derp_temporal_filter(self.h, _ptrs(guides), _ptrs(images), _ptrs(masks), n, w, h, frame_offset,
                                            sigma, radius, w0, w1, w2, _p(out)))
        return out

    def temporal_filter_dev(self, guide_ptrs, disp_ptrs, mask_ptrs, w, h, frame_offset, sigma, radius, w0, w1, w2,
                            out_ptr):
        n = len(guide_ptrs)
        gp = (C.c_void_p * n)(*guide_ptrs)
        ip = (C.c_void_p * n)(*disp_ptrs)
        mp = (C.c_void_p * n)(*mask_ptrs)
        self._ck(lib().derp_temporal_filter_dev(self.h, gp, ip, mp, n, w, h, frame_offset, sigma, radius, w0, w1, w2,
                                                out_ptr))

    def dev_disparity(self, level, d):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(lib().derp_dev_disparity(self.h, level, d, C.byref(p), C.byref(n)))
        return p.value, n.value

    def dev_color(self, level, s):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(lib().derp_dev_color(self.h, level, s, C.byref(p), C.byref(n)))
        return p.value, n.value

    def dev_mask(self, level, d):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(lib().derp_dev_mask(self.h, level, d, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- measurement
    def counters(self):
        a, b, i = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._ck(lib().derp_get_counters(self.h, C.byref(a), C.byref(b), C.byref(i)))
        return dict(n_cost=a.value, n_pair=b.value, insufficient=i.value)

    def reset_counters(self):
        self._ck(lib().derp_reset_counters(self.h))

    def profile_enable(self, on=True):
        self._ck(lib().derp_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._ck(lib().derp_profile_reset(self.h))

    def profile_query(self, stage, level=-1):
        ms, n = C.c_double(), C.c_int()
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(lib().derp_profile_query(self.h, stage.encode(), level, C.byref(ms), C.byref(n), C.byref(a), C.byref(b)))
        return dict(ms=ms.value, launches=n.value, n_cost=a.value, n_pair=b.value)

    def profile_memoised(self, stage, level=-1):
        m = C.c_uint64()
        self._ck(lib().derp_profile_memoised(self.h, stage.encode(), level, C.byref(m)))
        return m.value

    def block_trace(self, stage, level):
        """-> uint64 [grid_y, grid_x, 2]: start / end (10 ns ticks) of the blocks of the stage's last launch at `level`
        (a library built with -DDERP_BLOCK_TRACE=1 only)"""
        gx, gy = C.c_int(), C.c_int()
        self._ck(lib().derp_debug_block_trace(self.h, stage.encode(), level, None, 0, C.byref(gx), C.byref(gy)))
        out = np.zeros((gy.value, gx.value, 2), dtype=np.uint64)
        self._ck(lib().derp_debug_block_trace(self.h, stage.encode(), level, _p(out), out.size, C.byref(gx), C.byref(gy)))
        return out

    def debug_level_plan(self):
        """What the frames of the level opened last share -> dict(level, batch, store_inverse, decisions); `decisions`
        counts the levels opened since the context was made"""
        out = np.zeros(4, dtype=np.int32)
        self._ck(lib().derp_debug_level_plan(self.h, _p(out)))
        return dict(level=int(out[0]), batch=int(out[1]), store_inverse=int(out[2]), decisions=int(out[3]))

    def device_memory(self):
        """-> (free, total) bytes of HBM right now"""
        f, t = C.c_uint64(), C.c_uint64()
        self._ck(lib().derp_device_memory(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    # ---- the rig preview tools: GenerateCameraOverlaps / GenerateEquirect
    def sweep_upload(self, images, resolutions):
        """images: per camera float BGRA [h, w, 4] at its scaled size; resolutions: per camera (x, y) the camera is
        rescaled to (doubles: resolution * scale, not rounded)"""
        assert len(images) == self.D and len(resolutions) == self.D
        ims = [np.ascontiguousarray(im, dtype=np.float32) for im in images]
        assert all(im.ndim == 3 and im.shape[2] == 4 for im in ims)
        res = np.ascontiguousarray(np.asarray(resolutions, dtype=np.float64).reshape(self.D, 2))
        self._ck(lib().derp_sweep_upload(self.h, _ptrs(ims), _ints([im.shape[1] for im in ims]),
                                         _ints([im.shape[0] for im in ims]), _p(res)))
        self._sweep_shapes = [im.shape[:2] for im in ims]

    def sweep_overlaps(self, dst, disparities, u8=False):
        """-> [n, h, w, 4] float32 (NaN where no camera sees the point) or uint8 (255.0f * image)"""
        d = np.ascontiguousarray(disparities, dtype=np.float32).reshape(-1)
        shapes = getattr(self, "_sweep_shapes", [])
        if not 0 <= dst < len(shapes):
            raise DerpError("sweep_upload has not been called, or bad camera index %d" % dst)
        out = np.zeros((len(d),) + tuple(shapes[dst]) + (4,), dtype=np.uint8 if u8 else np.float32)
        self._ck(lib().derp_sweep_overlaps(self.h, dst, _p(d), len(d), int(bool(u8)), _p(out)))
        return out

    def sweep_equirect_bounds(self, width, height, depth):
        """-> (minX, maxX, minY, maxY) of the columns and rows at which any camera sees the equirect's point"""
        b = (C.c_int * 4)()
        self._ck(lib().derp_sweep_equirect_bounds(self.h, int(width), int(height), depth, b))
        return tuple(b)

    def sweep_equirect(self, width, height, depths, window=None, out_size=None, black_bg=False, u8=False):
        """window: None or (minX, maxX, minY, maxY) with out_size = (w, h) -> [n, h, w, 4] float32 or uint8"""
        d = np.ascontiguousarray(depths, dtype=np.float32).reshape(-1)
        ow, oh = (width, height) if out_size is None else out_size
        win = None if window is None else _ints([int(v) for v in window])
        bg = (C.c_float * 4)(0, 0, 0 if black_bg else 1, 1)
        out = np.zeros((len(d), int(oh), int(ow), 4), dtype=np.uint8 if u8 else np.float32)
        self._ck(lib().derp_sweep_equirect(self.h, int(width), int(height), win, int(ow), int(oh), _p(d), len(d), bg,
                                           int(bool(u8)), _p(out)))
        return out

    # ---- RigAnalyzer: how many cameras see each point
    def coverage_directions(self, units, distances, want_counts=True):
        """units [n, 3] float64, distances [nd] float64 -> (hist [nd, S + 1] int32, counts [nd, n] uint8 or None)"""
        u = np.ascontiguousarray(units, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(distances, dtype=np.float64).reshape(-1)
        hist = np.zeros((len(d), self.D + 1), dtype=np.int32)
        counts = np.zeros((len(d), len(u)), dtype=np.uint8) if want_counts else None
        self._ck(lib().derp_coverage_directions(self.h, _p(u), len(u), _p(d), len(d), _p(hist), _p(counts)))
        return hist, counts

    def coverage_equirect(self, pixels_per_degree=5, distance=1e4, timing=True):
        """-> (counts [H, W] uint8, min_timing [H, W] float32 or None, (holes, maxMin, aveMin) or None)"""
        ppd = int(pixels_per_degree)
        shape = (180 * max(ppd, 0), 360 * max(ppd, 0))
        counts = np.zeros(shape, dtype=np.uint8)
        mt = np.zeros(shape, dtype=np.float32) if timing else None
        stats = np.zeros(3, dtype=np.float64) if timing else None
        self._ck(lib().derp_coverage_equirect(self.h, ppd, float(distance), _p(counts), _p(mt), _p(stats)))
        return counts, mt, (None if stats is None else tuple(float(v) for v in stats))

    def coverage_camera(self, cam, distance=1e4):
        """-> counts [h, w] uint8 over the pixels of camera `cam` at its own resolution; 0 outside the image circle"""
        cam = int(cam)
        res = self.cams_dst[cam]["resolution"] if 0 <= cam < self.D else (0, 0)
        counts = np.zeros((int(res[1]), int(res[0])), dtype=np.uint8)
        self._ck(lib().derp_coverage_camera(self.h, cam, float(distance), _p(counts)))
        return counts

    def coverage_cross_section(self, dim=400):
        """-> counts [dim, dim] uint8 over the plane z = 0, one unit per pixel, centred on the rig's origin"""
        counts = np.zeros((max(int(dim), 0),) * 2, dtype=np.uint8)
        self._ck(lib().derp_coverage_cross_section(self.h, int(dim), _p(counts)))
        return counts

    # ---- AlignColors: red and blue resampled onto the green rig
    def align_setup(self, red_ref, green_ref, blue_ref):
        """red_ref / green_ref / blue_ref: the cameras (dicts) of the three reference rigs, one each; builds the warp
        maps of every camera of this context's rig"""
        rigs = [(CameraDesc * max(len(r), 1))(*[camera_desc(cam) for cam in r]) for r in (red_ref, green_ref, blue_ref)]
        self._ck(lib().derp_align_setup(self.h, rigs[0], len(red_ref), rigs[1], len(green_ref), rigs[2], len(blue_ref)))

    def _align_shape(self, cam):
        if not 0 <= cam < self.D:
            raise DerpError("bad camera index %d (the context has %d)" % (cam, self.D))
        return int(self.cams_dst[cam]["resolution"][1]), int(self.cams_dst[cam]["resolution"][0])

    def align_maps(self, cam):
        """-> (red, blue), each [h, w, 2] float32: where pixel (x, y) of the green grid samples its channel"""
        h, w = self._align_shape(cam)
        red, blue = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 2), np.float32)
        self._ck(lib().derp_align_maps(self.h, int(cam), _p(red), _p(blue)))
        return red, blue

    def align_frame(self, images):
        """images: per camera BGR uint16 [h, w, 3] -> the aligned images, same shapes"""
        assert len(images) == self.D
        ims = [np.ascontiguousarray(im, dtype=np.uint16) for im in images]
        assert all(im.ndim == 3 and im.shape[2] == 3 for im in ims)
        outs = [np.zeros_like(im) for im in ims]
        self._ck(lib().derp_align_frame(self.h, _ptrs(ims), _ints([im.shape[1] for im in ims]),
                                        _ints([im.shape[0] for im in ims]), _ptrs(outs)))
        return outs

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._ck(lib().derp_device_name(self.h, buf, 256))
        return buf.value.decode()


MESH_EXIT_BUDGET, MESH_EXIT_INFINITE_THRESHOLD, MESH_EXIT_STUCK = 0, 1, 2


def gc_slice_count(cams, dst, small_size, disparity_step=0.5):
    """GeometricConsistency's sliceCount for destination `dst` of the rig `cams` (as the file holds it) at its small
    size (w, h), on the host (no device); raises DerpError with the refusal's text."""
    a = (CameraDesc * len(cams))(*[camera_desc(c) for c in cams])
    n = C.c_int()
    if lib().derp_gc_slice_count(a, len(cams), dst, int(small_size[0]), int(small_size[1]), disparity_step,
                                 C.byref(n)):
        raise DerpError(lib().derp_last_error(None).decode())
    return n.value


def _host_ck(rc):
    if rc:
        raise DerpError(lib().derp_last_error(None).decode())


def preview_variance_levels(var_low_max, var_high_max, low_slider, high_slider, scale=1.0):
    """(varNoiseFloor, varHighThresh, varLowShow, varHighShow) of TrackVar::update, float32 [4]"""
    out = np.zeros(4, dtype=np.float32)
    _host_ck(lib().derp_preview_variance_levels(var_low_max, var_high_max, int(low_slider), int(high_slider), scale, _p(out)))
    return out


def keypoint_params(length_stride=0.125, height_stride=0.125, depth_min=1.0, depth_max=100.0, depth_samples=1000.0,
                    search_overlap=0.25, search_radius=100):
    """the seven doubles of derp_preview_keypoint*, at the reference's defaults"""
    return np.array([length_stride, height_stride, depth_min, depth_max, depth_samples, search_overlap, search_radius],
                    dtype=np.float64)


def preview_keypoint_samples(cam_point, cam_into, px, py, max_out=4096, **params):
    """-> (indices int32 [n], disparities f64 [n], boxes f32 [n][4] as x, y, width, height) of the accepted samples"""
    p = keypoint_params(**params)
    idx, disp = np.zeros(max_out, np.int32), np.zeros(max_out, np.float64)
    boxes = np.zeros((max_out, 4), np.float32)
    n = C.c_int(0)
    _host_ck(lib().derp_preview_keypoint_samples(C.byref(camera_desc(cam_point)), C.byref(camera_desc(cam_into)), float(px),
                                                 float(py), _p(p), max_out, _p(idx), _p(disp), _p(boxes), C.byref(n)))
    k = min(n.value, max_out)
    return idx[:k], disp[:k], boxes[:k]


def preview_keypoint_rect(px, py, search_radius, w, h):
    """(x0, y0, x1, y1), inclusive and clipped, of the rectangle drawn for a projected point"""
    out = np.zeros(4, np.int32)
    _host_ck(lib().derp_preview_keypoint_rect(float(px), float(py), int(search_radius), int(w), int(h), _p(out)))
    return tuple(int(v) for v in out)


def preview_foreground_threshold(slider):
    """threshold = threshMax * slider / 100 with threshMax = 1.0f (ViewForegroundMaskThresholds.cpp:72, :141)"""
    return np.float32(1.0) * np.float32(int(slider)) / np.float32(100)


def sweep_overlap_disparities(num_depths, min_depth_m=1, max_depth_m=10):
    """GenerateCameraOverlaps' disparities in sweep order and their files' stems (int(depth * 100)), on the host"""
    d, s = np.zeros(max(num_depths, 0), dtype=np.float32), np.zeros(max(num_depths, 0), dtype=np.int32)
    _host_ck(lib().derp_sweep_overlap_disparities(int(num_depths), min_depth_m, max_depth_m, _p(d), _p(s)))
    return d, s


def sweep_equirect_depths(num_depths, depth_min=1.0, depth_max=10.0):
    """GenerateEquirect's depths by index and their files' stems, on the host"""
    d, s = np.zeros(max(num_depths, 0), dtype=np.float32), np.zeros(max(num_depths, 0), dtype=np.int32)
    _host_ck(lib().derp_sweep_equirect_depths(int(num_depths), depth_min, depth_max, _p(d), _p(s)))
    return d, s


def sweep_crop_size(height, bounds):
    """--crop_equirect's width for the bounds (minX, maxX, minY, maxY); raises DerpError on an empty box"""
    w = C.c_int()
    _host_ck(lib().derp_sweep_crop_size(int(height), _ints([int(v) for v in bounds]), C.byref(w)))
    return w.value


def rig_center(cams, index):
    """GenerateEquirect --camera_id: the rig rotated so that camera `index` faces the equirect's centre, on the host.
    -> the cameras (dicts) with origin, forward, up and right replaced"""
    a = (CameraDesc * len(cams))(*[camera_desc(c) for c in cams])
    b = (CameraDesc * len(cams))()
    _host_ck(lib().derp_rig_center(a, len(cams), int(index), b))
    out = []
    for cam, j in zip(cams, b):
        cam = dict(cam)
        for k in ("origin", "forward", "up", "right"):
            cam[k] = [float(v) for v in getattr(j, k)]
        out.append(cam)
    return out


# ---- RigAnalyzer's rig construction and editing, on the host
RIG_ARRANGEMENTS = ("ballcam24", "tetra", "tetratilted", "ring4", "cube", "carbon0", "carbon1", "diamond")


def _descs(cams):
    return (CameraDesc * len(cams))(*[camera_desc(c) for c in cams])


def _cam_dict(template, j):
    """the camera dict `template` with what derp_rig_* may change taken from the descriptor j"""
    cam = dict(template)
    for k in ("origin", "forward", "up", "right", "resolution", "focal"):
        cam[k] = [float(v) for v in getattr(j, k)]
    cam.pop("principal", None)
    if j.has_principal:
        cam["principal"] = [float(v) for v in j.principal]
    cam["id"] = j.id.decode()
    return cam


def _rename(cams, one_based):
    """--one_based_indexing: cam0, cam1, ... become cam1, cam2, ..."""
    return [dict(c, id="cam%d" % (i + 1)) for i, c in enumerate(cams)] if one_based else cams


def rig_fibonacci_units(count, discard_poles_deg=0.0):
    """RigAnalyzer's sample directions -> [kept, 3] float64"""
    out, kept = np.zeros((max(int(count), 0), 3), dtype=np.float64), C.c_int()
    _host_ck(lib().derp_rig_fibonacci_units(int(count), float(discard_poles_deg), _p(out), C.byref(kept)))
    return out[:kept.value].copy()


def rig_coverage_distances(min_distance=0.5):
    """RigAnalyzer's 20 sweep distances -> [20] float64"""
    out = np.zeros(20, dtype=np.float64)
    _host_ck(lib().derp_rig_coverage_distances(float(min_distance), _p(out)))
    return out


def rig_euler_matrix(euler_rad, xyz=True):
    """rotationMatrixFromEulers -> [3, 3] float64"""
    e, m = np.ascontiguousarray(euler_rad, dtype=np.float64).reshape(3), np.zeros((3, 3), dtype=np.float64)
    _host_ck(lib().derp_rig_euler_matrix(_p(e), int(bool(xyz)), _p(m)))
    return m


def rig_align_z_matrix(position):
    """--rotate_cam_z's rotation for a camera at `position` -> [3, 3] float64"""
    p, m = np.ascontiguousarray(position, dtype=np.float64).reshape(3), np.zeros((3, 3), dtype=np.float64)
    _host_ck(lib().derp_rig_align_z_matrix(_p(p), _p(m)))
    return m


def rig_from_eulers(model, eulers_deg, xyz=False, one_based=False):
    """clones of the camera `model` (a dict) turned by each row of eulers_deg [n, 3] -> cameras cam0, cam1, ..."""
    e = np.ascontiguousarray(eulers_deg, dtype=np.float64).reshape(-1, 3)
    out = (CameraDesc * max(len(e), 1))()
    _host_ck(lib().derp_rig_from_eulers(C.byref(camera_desc(model)), _p(e), len(e), int(bool(xyz)), out))
    return _rename([_cam_dict(model, j) for j in out[:len(e)]], one_based)


def rig_arrangement(name, model, custom=-1.0, one_based=False):
    """one of RIG_ARRANGEMENTS built from the camera `model`; raises DerpError on an unknown name"""
    out, n = (CameraDesc * 24)(), C.c_int()
    _host_ck(lib().derp_rig_arrangement(name.encode(), C.byref(camera_desc(model)), float(custom), out, C.byref(n)))
    return _rename([_cam_dict(model, j) for j in out[:n.value]], one_based)


def rig_revolve(cams, eulers_rad):
    """the rig repeated once per row of eulers_rad [m, 3] (radians), turned by it -> m * n cameras"""
    e = np.ascontiguousarray(eulers_rad, dtype=np.float64).reshape(-1, 3)
    out = (CameraDesc * max(len(e) * len(cams), 1))()
    _host_ck(lib().derp_rig_revolve(_descs(cams), len(cams), _p(e), len(e), out))
    return [_cam_dict(cams[i % len(cams)], j) for i, j in enumerate(out[:len(e) * len(cams)])]


def rig_rotate(cams, matrix):
    """every camera's position and rotation turned by the 3 x 3 `matrix`"""
    m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(3, 3)
    out = (CameraDesc * max(len(cams), 1))()
    _host_ck(lib().derp_rig_rotate(_descs(cams), len(cams), _p(m), out))
    return [_cam_dict(c, j) for c, j in zip(cams, out)]


def rig_perturb(cams, seed=1, positions=0.0, rotations=0.0, principals=0.0, focals=0.0):
    """Camera::perturbCameras after std::srand(seed); camera 0 keeps its pose"""
    a = _descs(cams)
    _host_ck(lib().derp_rig_perturb(a, len(cams), int(seed), float(positions), float(rotations), float(principals), float(focals)))
    return [_cam_dict(c, j) for c, j in zip(cams, a)]


def rig_scale(cams, scale_rig=1.0, radius=0.0, scale_resolution=1.0):
    """--scale_rig, --radius and --scale_resolution, in that order"""
    a = _descs(cams)
    _host_ck(lib().derp_rig_scale(a, len(cams), float(scale_rig), float(radius), float(scale_resolution)))
    return [_cam_dict(c, j) for c, j in zip(cams, a)]


def align_derive_cameras(green, red_ref, green_ref, blue_ref):
    """AlignColors' red and blue models of the calibrated camera `green` (dicts in, dicts out), on the host: the green
    camera with the reference channel's focal times a float ratio, {s, -s}, and the reference channel's distortion"""
    a = [camera_desc(c) for c in (green, red_ref, green_ref, blue_ref)]
    red, blue = CameraDesc(), CameraDesc()
    _host_ck(lib().derp_align_derive_cameras(C.byref(a[0]), C.byref(a[1]), C.byref(a[2]), C.byref(a[3]), C.byref(red), C.byref(blue)))
    out = []
    for j in (red, blue):
        cam = dict(green)
        cam["focal"] = [float(j.focal[0]), float(j.focal[1])]
        cam.pop("distortion", None)
        if j.has_distortion:
            cam["distortion"] = [float(v) for v in j.distortion]
        out.append(cam)
    return tuple(out)


def mesh_setup_host(vertices, faces, equi_error=True):
    """computeInitialQuadrics on the host (no device) -> (face planes [nf, 4], edge costs [nf, 3], vertex quadrics [nv, 10])"""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    planes, costs, vq = np.zeros((len(f), 4)), np.zeros((len(f), 3)), np.zeros((len(v), 10))
    if lib().derp_mesh_setup_host(_p(v), len(v), _p(f), len(f), int(equi_error), _p(planes),
                                  _p(costs), _p(vq)):
        raise DerpError("derp_mesh_setup_host: bad arguments")
    return planes, costs, vq


def mesh_simplify_host(vertices, faces, num_faces_out, strictness=0.2, remove_boundary_edges=False, equi_error=True,
                       setup=None):
    """MeshSimplifier::simplify on the host (no device); setup = (planes, costs, quadrics) or None: computed here.
    -> (vertices f64 [nv', 3], faces i32 [nf', 3], (passes of the loop, MESH_EXIT_*))"""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    planes, costs, vq = (None, None, None) if setup is None else [np.ascontiguousarray(a, dtype=np.float64) for a in setup]
    ov, of = np.zeros_like(v), np.zeros_like(f)
    nv, nf = C.c_size_t(), C.c_size_t()
    stats = (C.c_int * 2)()
    if lib().derp_mesh_simplify_host(_p(v), len(v), _p(f), len(f), _p(planes), _p(costs), _p(vq),
                                     num_faces_out, strictness, int(remove_boundary_edges), int(equi_error),
                                     _p(ov), _p(of), C.byref(nv), C.byref(nf), stats):
        raise DerpError("derp_mesh_simplify_host: bad arguments")
    return ov[:nv.value].copy(), of[:nf.value].copy(), (stats[0], stats[1])


def mesh_texcoords_equirect(vertices):
    """addTextureCoordinatesEquirect (MeshUtil.h:407-419) on the host (no device): f64 [nv, 3] -> st f64 [nv, 2]"""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    st = np.zeros((len(v), 2))
    if lib().derp_mesh_texcoords_equirect(_p(v), len(v), _p(st)):
        raise DerpError("derp_mesh_texcoords_equirect: bad arguments")
    return st


def host_nth_element_pairs(pairs, nth):
    p = np.ascontiguousarray(pairs, dtype=np.float32).copy()
    lib().derp_host_nth_element_pairs(_p(p), len(p), nth)
    return p


def host_minstd_uniform(seed, draw_index, a, b):
    return lib().derp_host_minstd_uniform(seed, draw_index, a, b)


def host_cost_tile_map(tiles, bands, rot, per_block):
    """Tile order of a random-proposal / ping-pong launch: int32 array [blocks, per_block] (host arithmetic, no GPU)."""
    cap = (tiles + 8 * bands * per_block) // per_block * per_block + 8 * bands * per_block
    out = np.empty(cap, dtype=np.int32)
    blocks = lib().derp_host_cost_tile_map(tiles, bands, rot, per_block, _p(out), cap)
    if blocks <= 0:
        raise ValueError("bad tile map arguments")
    return out[:blocks * per_block].reshape(blocks, per_block)


def host_table_batch(n_dst, bytes_no_inverse, bytes_with_inverse, inverse_needed, budget_bytes):
    """The table budget -> (destinations per batch, inverse warps stored) of a level (host arithmetic, no GPU)."""
    batch, inverse = C.c_int(), C.c_int()
    if lib().derp_host_table_batch(n_dst, bytes_no_inverse, bytes_with_inverse, int(bool(inverse_needed)), budget_bytes,
                                   C.byref(batch), C.byref(inverse)):
        raise ValueError("bad arguments, or not even one destination's tables fit the budget")
    return batch.value, bool(inverse.value)


def average_score(score, mask):
    """rephoto_util::averageScore -> [B, G, R] means over mask != 0 and not-NaN."""
    score = np.ascontiguousarray(score, dtype=np.float32)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    h, w = mask.shape
    out = (C.c_double * 3)()
    if lib().derp_average_score(_p(score), _p(mask), w, h, out):
        raise DerpError("derp_average_score: bad arguments")
    return [out[0], out[1], out[2]]


def format_results(avg):
    """rephoto_util::formatResults (RephotographyUtil.h:110-116)."""
    return "R %.2f%%, G %.2f%%, B %.2f%%" % (100 * avg[2], 100 * avg[1], 100 * avg[0])


# ---------------------------------------------------------------- camera ISP (raw Bayer -> RGB)
ISP_FILTERS = {"bilinear": 0, "frequency": 1, "edge_aware": 2, "chroma_suppressed_bilinear": 3}
ISP_STAGES = ["load", "pixel", "stuck", "demosaic", "color", "lowpass", "sharpened"]


def isp_config(config):
    """The "CameraIsp" object of an isp.json (or the whole file's dict) -> derp_isp_config; missing keys keep the
    reference's defaults (CameraIsp.h:490-562)."""
    k = IspConfig()
    lib().derp_isp_config_default(C.byref(k))
    j = config.get("CameraIsp", config) if config else {}
    for key, field in (("bitsPerPixel", "bits_per_pixel"), ("width", "width"), ("height", "height"),
                       ("stuckPixelThreshold", "stuck_pixel_threshold"), ("stuckPixelRadius", "stuck_pixel_radius")):
        if key in j:
            setattr(k, field, int(j[key]))
    for key, field in (("isLittleEndian", "is_little_endian"), ("isRowMajor", "is_row_major")):
        if key in j:
            setattr(k, field, int(bool(j[key])))
    for key, field in (("bayerPattern", "bayer_pattern"), ("planeOrder", "plane_order")):
        if key in j:
            setattr(k, field, j[key].upper().encode())
    for key, field in (("stuckPixelDarknessThreshold", "stuck_pixel_darkness_threshold"), ("saturation", "saturation"),
                       ("contrast", "contrast"), ("sharpeningSupport", "sharpening_support"), ("noiseCore", "noise_core")):
        if key in j:
            setattr(k, field, float(j[key]))
    for key, field in (("blackLevel", "black_level"), ("clampMin", "clamp_min"), ("clampMax", "clamp_max"),
                       ("whiteBalanceGain", "white_balance_gain"), ("gamma", "gamma"), ("lowKeyBoost", "low_key_boost"),
                       ("highKeyBoost", "high_key_boost"), ("sharpening", "sharpening")):
        if j.get(key) is not None:
            for i in range(3):
                getattr(k, field)[i] = float(j[key][i])
    for key, field, count in (("vignetteRollOffH", "rolloff_h", "n_rolloff_h"), ("vignetteRollOffV", "rolloff_v", "n_rolloff_v")):
        if j.get(key) is not None:
            if len(j[key]) > ISP_MAX_ROLLOFF:
                raise DerpError("%s holds more than %d points" % (key, ISP_MAX_ROLLOFF))
            setattr(k, count, len(j[key]))
            for n, p in enumerate(j[key]):
                for i in range(3):
                    getattr(k, field)[n][i] = float(p[i])
    if j.get("ccm") is not None:
        for r in range(3):
            for c in range(3):
                k.ccm[3 * r + c] = float(j["ccm"][r][c])
    if j.get("compandingLut") is not None:
        k.n_companding_lut = len(j["compandingLut"])
    return k


class Isp:
    """One camera ISP (derp_isp_create .. derp_isp_destroy): CameraIsp of the reference, on the GPU."""

    def __init__(self, config, demosaic_filter=0, pow2_downscale=1, apply_tone_curve=True, device=0):
        self.cfg = config if isinstance(config, IspConfig) else isp_config(config)
        h = C.c_void_p()
        if lib().derp_isp_create(C.byref(h), device, C.byref(self.cfg), int(demosaic_filter), int(pow2_downscale),
                                 int(bool(apply_tone_curve))):
            raise DerpError(lib().derp_last_error(None).decode())
        self.h = h
        w, hh = C.c_int(), C.c_int()
        self._ck(lib().derp_isp_output_size(self.h, C.byref(w), C.byref(hh)))
        self.width, self.height = w.value, hh.value
        self.dtype = np.uint8 if self.cfg.bits_per_pixel == 8 else np.uint16

    def _ck(self, rc):
        if rc:
            raise DerpError(lib().derp_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            lib().derp_isp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, raw):
        """raw: the .raw file's bytes (or an array of them) -> [h, w, 3] BGR, u8 or u16 like the sensor"""
        buf = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        out = np.zeros((self.height, self.width, 3), self.dtype)
        self._ck(lib().derp_isp_process(self.h, _p(buf), buf.size, _p(out)))
        return out

    def stage(self, stage):
        """the fp32 result of a stage of the last process(): [h, w] (load, pixel, stuck) or [3, h, w] R, G, B"""
        s = ISP_STAGES.index(stage) if isinstance(stage, str) else int(stage)
        out = np.zeros((self.height, self.width) if s < 3 else (3, self.height, self.width), np.float32)
        self._ck(lib().derp_isp_stage(self.h, s, _p(out)))
        return out

    def tables(self):
        """-> (vignette_h [w, 3], vignette_v [h, 3], composite ccm [3, 3], tone lut [4096, 3]), as built on the host"""
        vh, vv = np.zeros((self.width, 3), np.float32), np.zeros((self.height, 3), np.float32)
        ccm, lut = np.zeros((3, 3), np.float32), np.zeros((4096, 3), np.float32)
        self._ck(lib().derp_isp_tables(self.h, _p(vh), _p(vv), _p(ccm), _p(lut)))
        return vh, vv, ccm, lut


# ---------------------------------------------------------------- RigSimulator (derp_sim_*)
SIM_TRIANGLE = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3),
                         ("normal", "<f4", 3), ("color", "<f4", 3)])  # derp_sim_triangle
SIM_NODE = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("skip", "<i4"), ("first", "<i4"), ("count", "<i4"),
                     ("n_children", "<i4")])  # derp_sim_node
SIM_STAGES = {"origin": (0, np.float32, 3), "direction": (1, np.float32, 3), "hit": (2, np.int32, 1),
              "distance": (3, np.float32, 1), "color": (4, np.float32, 3)}


class SimScene:
    """RigSimulator's triangles and sphere tree, built on the host (no device): the builders append, build_bvh()
    flattens. The random builders draw from the C library's rand(): srand() first for a repeatable scene."""

    def __init__(self):
        self.h = C.c_void_p(lib().derp_sim_scene_create())

    def close(self):
        if self.h:
            lib().derp_sim_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @staticmethod
    def _ck(rc):
        if rc:
            raise DerpError("derp_sim_scene: bad arguments")

    def icosahedrons(self, count=250, min_dist=100.0, max_dist=250.0, min_radius=20.0, max_radius=50.0, red_triangle=False):
        self._ck(lib().derp_sim_scene_icosahedrons(self.h, int(count), min_dist, max_dist, min_radius, max_radius,
                                                   int(bool(red_triangle))))
        return self

    def cubes(self):
        self._ck(lib().derp_sim_scene_cubes(self.h))
        return self

    def ground_plane(self, dist=1.70):
        self._ck(lib().derp_sim_scene_ground_plane(self.h, dist))
        return self

    def add_triangle(self, v0, v1, v2, color_bgr):
        a = [np.ascontiguousarray(v, dtype=np.float32) for v in (v0, v1, v2, color_bgr)]
        self._ck(lib().derp_sim_scene_add_triangle(self.h, *[_p(v) for v in a]))
        return self

    def build_bvh(self, leaf_threshold=20, split_k=5, max_depth=50):
        self._ck(lib().derp_sim_bvh_build(self.h, leaf_threshold, split_k, max_depth))
        return self

    def arrays(self):
        """(triangles [SIM_TRIANGLE], nodes [SIM_NODE], leaf indices int32)."""
        nt, nn, nl = C.c_int(), C.c_int(), C.c_int()
        self._ck(lib().derp_sim_scene_counts(self.h, C.byref(nt), C.byref(nn), C.byref(nl)))
        tris, nodes, leaf = np.zeros(nt.value, SIM_TRIANGLE), np.zeros(nn.value, SIM_NODE), np.zeros(nl.value, np.int32)
        self._ck(lib().derp_sim_scene_get(self.h, _p(tris), _p(nodes), _p(leaf)))
        return tris, nodes, leaf

    def trace_host(self, rays):
        """Single-thread CPU tracer (geometry only): rays [n, 6] -> [n, 4] (b, g, r, depth)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 4), np.float32)
        self._ck(lib().derp_sim_trace_host(self.h, _p(rays), rays.shape[0], _p(out)))
        return out


def sim_noise(bgr, amplitude):
    """corruptImageWithNoise in place on a float32 [h, w, 3] image (rand() of the C library)."""
    assert bgr.dtype == np.float32 and bgr.flags.c_contiguous and bgr.ndim == 3 and bgr.shape[2] == 3
    if lib().derp_sim_noise(_p(bgr), bgr.shape[1], bgr.shape[0], amplitude):
        raise DerpError("derp_sim_noise: bad arguments")
    return bgr


def sim_perlin_table():
    p = np.zeros(512, np.uint8)
    lib().derp_sim_perlin_table(_p(p))
    return p


class Sim:
    """RigSimulator's tracer on the GPU (derp_sim_create .. derp_sim_destroy)."""

    def __init__(self, device=0):
        h = C.c_void_p()
        if lib().derp_sim_create(C.byref(h), device):
            raise DerpError(lib().derp_last_error(None).decode())
        self.h = h

    def _ck(self, rc):
        if rc:
            raise DerpError(lib().derp_last_error(None).decode())

    def close(self):
        if self.h:
            lib().derp_sim_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def upload(self, triangles, nodes, leaf, skybox, ceiling=None, ceiling_position=0.0, ceiling_width=0.0,
               ceiling_depth=0.0, marble=False, marble_scale=0.1):
        """triangles / nodes / leaf as SimScene.arrays() gives them; skybox and ceiling uint8 BGR [h, w, 3]."""
        triangles = np.ascontiguousarray(triangles, dtype=SIM_TRIANGLE)
        nodes = np.ascontiguousarray(nodes, dtype=SIM_NODE)
        leaf = np.ascontiguousarray(leaf, dtype=np.int32)
        skybox = np.ascontiguousarray(skybox, dtype=np.uint8)
        assert skybox.ndim == 3 and skybox.shape[2] == 3
        cw = ch = 0
        if ceiling is not None:
            ceiling = np.ascontiguousarray(ceiling, dtype=np.uint8)
            assert ceiling.ndim == 3 and ceiling.shape[2] == 3
            ch, cw = ceiling.shape[:2]
        p = SimParams(ceiling_position, ceiling_width, ceiling_depth, marble_scale, int(bool(marble)), 0)
        self._ck(lib().derp_sim_upload(self.h, _p(triangles), len(triangles), _p(nodes), len(nodes), _p(leaf), len(leaf),
                                       _p(skybox), skybox.shape[1], skybox.shape[0],
                                       _p(ceiling) if ceiling is not None else None, cw, ch, C.byref(p)))

    def render_camera(self, cam, aas=1):
        """cam: a rig-file camera dict or CameraDesc -> (bgr float32 [h, w, 3] in 0..255, depth float32 [h, w])."""
        d = cam if isinstance(cam, CameraDesc) else camera_desc(cam)
        w, h = int(d.resolution[0]), int(d.resolution[1])
        bgr, depth = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
        self._ck(lib().derp_sim_render_camera(self.h, C.byref(d), int(aas), _p(bgr), _p(depth)))
        return bgr, depth

    def render_equirect(self, w, h, aas=1, stereo=False, interpupillary_radius=3.2):
        """mono: (bgr, inverse depth); stereo: (left, right)."""
        a = np.zeros((h, w, 3), np.float32)
        b = np.zeros((h, w, 3), np.float32) if stereo else np.zeros((h, w), np.float32)
        self._ck(lib().derp_sim_render_equirect(self.h, w, h, int(aas), int(bool(stereo)), interpupillary_radius,
                                                _p(a), _p(b) if stereo else None, None if stereo else _p(b)))
        return a, b

    def trace_rays(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        self._ck(lib().derp_sim_trace_rays(self.h, _p(rays), rays.shape[0]))

    def stage(self, name, eye=0):
        """A supersampled plane of the last render: origin, direction, hit, distance, color."""
        idx, dtype, cn = SIM_STAGES[name]
        w, h = C.c_int(), C.c_int()
        self._ck(lib().derp_sim_stage_size(self.h, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value, cn) if cn > 1 else (h.value, w.value), dtype)
        self._ck(lib().derp_sim_stage(self.h, idx, int(eye), _p(out)))
        return out
