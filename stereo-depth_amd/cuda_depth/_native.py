"""ctypes binding of libstereo_mi355x.so (include/stereo_mi355x.h).  No CPU fallback:
if the library is missing or has the wrong ABI, importing this module fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SMX_LIB_PATH") or os.path.join(_PKG, "libstereo_mi355x.so")   # override: kernel experiments only

SMX_ABI_VERSION = 4
SMX_OK = 0
MATCH_MODES = {"auto": 0, "exact_order": 1, "fast_grid": 2}
# smx_fp_convention (include/stereo_mi355x.h): how step 1 and the parabola's two sums of products are contracted
FP_CONVENTIONS = {"source": 0, "fma_first": 1, "fma_second": 2, "fma_outer": 3, "fma_first_in": 4, "fma_second_in": 5}


def fp_mixed(step1, parabola) -> int:
    """SMX_FP_MIXED: step 1 and the parabola contracted differently (names or 0..5)."""
    s, p = (FP_CONVENTIONS[v] if isinstance(v, str) else int(v) for v in (step1, parabola))
    return s | ((p + 1) << 3)

STAGE_GRAY_LEFT, STAGE_GRAY_RIGHT, STAGE_DOWN_LEFT, STAGE_DOWN_RIGHT = 0, 1, 2, 3
STAGE_WTA, STAGE_MBM_COSTS, STAGE_REFINED, STAGE_AGG_VOLUME, STAGE_GRID_FLAG = 4, 5, 6, 7, 8


class SmxConfig(C.Structure):
    _fields_ = [
        ("height", C.c_uint32), ("width", C.c_uint32), ("downscale_factor", C.c_uint32),
        ("min_disparity", C.c_int32), ("max_disparity", C.c_int32),
        ("ncc_patch_radius", C.c_uint32), ("sad_patch_radius", C.c_uint32), ("threshold", C.c_uint32),
        ("small_mbm_radius", C.c_int32), ("mid_mbm_radius", C.c_int32), ("large_mbm_radius", C.c_int32),
        ("device_id", C.c_int32), ("max_batch", C.c_int32), ("match_mode", C.c_int32),
        ("overlap_min_pairs", C.c_int32), ("exact_filter", C.c_int32), ("fp_convention", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class SmxDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("H", "W", "K", "h", "w", "dmin", "dmax", "Dd")]


class SmxMatchGeometry(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("band_rows", C.c_int32), ("rows_marched", C.c_int32),
                ("waves_per_workgroup", C.c_int32), ("workgroups", C.c_int32),
                ("columns_per_wave", C.c_double), ("useful_fraction", C.c_double)]


MATCH_KERNELS = ("exact_only", "fast_window", "fast_split", "fast_wide")
FEATURE_EXPERIMENTAL = 1


class SmxRouteInfo(C.Structure):
    _fields_ = [("filter_available", C.c_int32), ("route_dense", C.c_int32), ("last_call_filtered", C.c_int32),
                ("probe_period", C.c_int32), ("candidate_density", C.c_float), ("offgrid_hint", C.c_int32),
                ("compute_units", C.c_int32), ("fast_dense", C.c_int32)]


EXPORTS = {
    # name: (restype, argtypes)
    "smx_abi_version": (C.c_int, []),
    "smx_config_default": (None, [C.POINTER(SmxConfig)]),
    "smx_get_dims": (C.c_int, [C.POINTER(SmxConfig), C.POINTER(SmxDims)]),
    "smx_last_error": (C.c_char_p, []),
    "smx_create": (C.c_int, [C.POINTER(SmxConfig), C.POINTER(C.c_void_p)]),
    "smx_destroy": (None, [C.c_void_p]),
    "smx_compute_rgb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_compute_gray": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_compute_gray_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_compute_gray_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_compute_rgb_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_compute_gray_u8_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_compute_rgb_u8_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_get_intermediate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "smx_stage_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "smx_last_match_mode": (C.c_int, [C.c_void_p]),
    "smx_overlap_lanes": (C.c_int, [C.c_void_p, C.c_int]),
    "smx_join": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smx_get_match_geometry": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SmxMatchGeometry)]),
    "smx_build_features": (C.c_int, []),
    "smx_get_route_info": (C.c_int, [C.c_void_p, C.POINTER(SmxRouteInfo)]),
    "smx_profile_begin": (C.c_int, [C.c_void_p, C.c_int]),
    "smx_profile_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "smx_compute_rgb_u8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_disparity_to_points": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_eval_metrics": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float,
                                   C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    # left-right consistency check: (engine, n, left, right, out, right_out, max_diff, invalid_disparity, stream)
    "smx_compute_lr_gray_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_float, C.c_float, C.c_void_p]),
    "smx_compute_lr_gray_u8_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_float, C.c_float, C.c_void_p]),
    "smx_compute_lr_rgb_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_float, C.c_float, C.c_void_p]),
    "smx_compute_lr_rgb_u8_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_float, C.c_float, C.c_void_p]),
    # (device_id, n, H, W, left_disp, right_disp, out, max_diff, invalid_disparity, stream)
    "smx_lr_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                               C.c_float, C.c_void_p]),
    # post-processing: (n, H, W) -> workspace bytes;
    # (device_id, n, H, W, in, out, max_speckle_size, max_diff, invalid_disparity, workspace, workspace_bytes, stream)
    "smx_postprocess_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_filter_speckles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                      C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    # (device_id, n, H, W, in, out, invalid_disparity, workspace, workspace_bytes, stream)
    "smx_fill_invalid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    # weighted median: (n, H, W) -> workspace bytes; (device_id, n, H, W, in, holes, guide, out, radius, range_weight,
    # spatial_weight, invalid_disparity, workspace, workspace_bytes, stream); the tables are host uint16 arrays
    "smx_median_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_weighted_median": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    # weighted least squares filter: (n, H, W) -> workspace bytes; (device_id, n, H, W, in, confidence, guide, out,
    # num_iterations, lambdas, range_weight, min_weight, invalid_disparity, workspace, workspace_bytes, stream); the
    # tables are host float32 arrays
    "smx_wls_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_wls_filter": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    # per-pixel confidence: (device_id, n, H, W, left_disp, right_disp, guide, radius, lr_scale, texture_scale,
    # invalid_disparity, out, stream)
    "smx_confidence_map": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    # temporal filter: (device_id, n, H, W, disp, confidence, guide, prev_guide, state_disp, state_weight, guide_out,
    # out, motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight, invalid_disparity, stream)
    "smx_temporal_filter": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                      C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    # rectification: (device_id, n, channels, dtype, H_in, W_in, H_out, W_out, left_in, right_in, left_map, right_map,
    # left_out, right_out, border_mode, border_value, stream)
    "smx_remap_pairs": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                  C.c_void_p]),
    # right-view synthesis head: (device_id, n, channels, dtype, D, h, w, scale, prob, left, out, stream)
    "smx_synthesize_right_view": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # its training form and backward: (..., scale, prob, left, view, stream); (..., scale, grad_view, left, grad_prob,
    # stream)
    "smx_synthesis_head_forward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "smx_synthesis_head_backward": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # semi-global matching: (n, H, W, num_disparities, paths) -> workspace bytes; (device_id, n, channels, dtype, H, W,
    # left, right, min_disparity, num_disparities, paths, P1, P2, uniqueness, lr_max_diff, subpixel, invalid_disparity,
    # out, gray_left_out, workspace, workspace_bytes, stream)
    "smx_sgm_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "smx_sgm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_size_t, C.c_void_p]),
    # smx_sgm plus right_out, after gray_left_out
    "smx_sgm_with_right_map": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                         C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    # metric 3D points: (n, H, W) -> workspace bytes; (device_id, n, H, W, disp, Q (host float32[16]), confidence,
    # min_confidence, z_min, z_max, invalid_disparity, image, image_channels, image_dtype, points, colors, indices,
    # xyz_map, offsets, workspace, workspace_bytes, stream)
    "smx_reproject_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_reproject_points": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float),
                                       C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    # voxel downsampling: (n, capacity) -> workspace bytes; (device_id, n, capacity, points, colors, offsets,
    # voxel_size, min_points, out_points, out_colors, out_counts, out_offsets, dropped, workspace, workspace_bytes,
    # stream)
    "smx_voxel_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "smx_voxel_downsample": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    # projection of point clouds into views: (n, H, W) -> workspace bytes; (device_id, n, capacity, H, W, points, offsets,
    # world_to_camera, P (host float32[16]), radius, z_min, z_max, invalid_disparity, disp, index, depth, workspace,
    # workspace_bytes, stream)
    "smx_project_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_project_points": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_float), C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # TSDF fusion: (n, H, W) -> workspace bytes; (device_id, nx, ny, nz, origin (host float32[3]), voxel_size,
    # truncation, max_weight, tsdf, weight, color, n, H, W, disp, Q, P (host float32[16]), world_to_camera, confidence,
    # min_confidence, z_min, z_max, invalid_disparity, image, image_channels, image_dtype, workspace, workspace_bytes,
    # stream)
    "smx_tsdf_integrate_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_tsdf_integrate": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_float,
                                     C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    # surface extraction: (nx, ny, nz) -> workspace bytes; (device_id, nx, ny, nz, origin, voxel_size, tsdf, weight,
    # color, min_weight, capacity, points, normals, colors, count, workspace, workspace_bytes, stream)
    "smx_tsdf_extract_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_tsdf_extract_points": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # triangles over those points: (nx, ny, nz) -> workspace bytes; (device_id, nx, ny, nz, tsdf, weight, min_weight,
    # capacity, triangles, count, workspace, workspace_bytes, stream)
    "smx_tsdf_extract_triangles_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_tsdf_extract_triangles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # views of the volume by ray casting: (nx, ny, nz) -> workspace bytes; (device_id, nx, ny, nz, origin, voxel_size,
    # tsdf, weight, color, min_weight, n, H, W, Q (host float32[16]), camera_to_world, step, z_min, z_max,
    # invalid_disparity, disp, depth, normals, colors, weight out, workspace, workspace_bytes, stream)
    "smx_tsdf_raycast_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_tsdf_raycast": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                   C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    # a window of the volume's state: (device_id, nx, ny, nz, tsdf, weight, color, x0, y0, z0, bx, by, bz, tsdf_out,
    # weight_out, color_out, stream)
    "smx_tsdf_window": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    # one volume's state merged into another in place: (device_id, nx, ny, nz, tsdf, weight, color, sx, sy, sz, src_tsdf,
    # src_weight, src_color, x0, y0, z0, rx, ry, rz, cx, cy, cz, mode, max_weight, stream)
    "smx_tsdf_merge": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                 C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                 C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                 C.c_void_p]),
    # camera tracking: (n, H, W) -> workspace bytes; (device_id, n, H, W, disp, confidence, Q (host float32[16]),
    # min_confidence, z_min, z_max, invalid_disparity, Hm, Wm, model_depth, model_normals, Qm, Pm (host float32[16]),
    # model_camera_to_world, model_world_to_camera, pose_in, schedule_pairs, schedule (host int32[pairs][2]),
    # max_distance, min_inliers, min_pivot, rot_eps, trans_eps, pose_out, info, rms, normal_equations, workspace,
    # workspace_bytes, stream)
    "smx_track_camera_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "smx_track_camera": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float),
                                   C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int, C.POINTER(C.c_int32), C.c_float, C.c_int, C.c_float, C.c_float, C.c_float,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "smx_track_camera_photometric_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    # uint8 frames to float32 intensity planes: (device_id, n, channels, H, W, image, out, stream)
    "smx_intensity_planes": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# tracking with a photometric term: smx_track_camera's 27 arguments up to trans_eps, then frame_intensity, model_intensity,
# photometric_weight, max_intensity_difference; its four outputs (normal_equations: [n][33]), then photometric_info,
# photometric_rms; its workspace, workspace_bytes, stream
_TRACK = EXPORTS["smx_track_camera"][1]
EXPORTS["smx_track_camera_photometric"] = (C.c_int, _TRACK[:27] + [C.c_void_p, C.c_void_p, C.c_float, C.c_float] +
                                           _TRACK[27:31] + [C.c_void_p, C.c_void_p] + _TRACK[31:])
# intensity pyramids: (n, H, W, levels) -> bytes; (device_id, n, H, W, levels, plane, mask_depth or NULL, pyramid, stream)
EXPORTS["smx_intensity_pyramid_bytes"] = (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int])
EXPORTS["smx_intensity_pyramid"] = (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p])
# tracking with the term read from pyramids: the photometric entry's arguments with frame_pyramid, model_pyramid, levels,
# schedule_levels (host int32[pairs]) in place of the two planes, and huber_delta after max_intensity_difference
EXPORTS["smx_track_camera_pyramid"] = (C.c_int, _TRACK[:27] + [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32),
                                                               C.c_float, C.c_float, C.c_float] +
                                       _TRACK[27:31] + [C.c_void_p, C.c_void_p] + _TRACK[31:])

BORDER_CONSTANT, BORDER_REPLICATE = 0, 1   # SMX_BORDER_*
DTYPE_U8, DTYPE_F32 = 0, 1                 # SMX_DTYPE_*
TSDF_MERGE_MODES = {"fill": 0, "average": 1}   # SMX_TSDF_MERGE_*
STREAM_ENGINE = C.c_void_p(-1)          # SMX_STREAM_ENGINE: the engine's own streams
KERNEL_SLOTS = ("prologue", "match_fast", "match_exact", "refine", "fill")


def load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP library first "
            "(python stereo-depth_amd/build.py or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.smx_abi_version() != SMX_ABI_VERSION:
        raise ImportError(f"{LIB_PATH}: ABI version {lib.smx_abi_version()} != {SMX_ABI_VERSION}")
    return lib


LIB = load()


def last_error() -> str:
    msg = LIB.smx_last_error()
    return msg.decode() if msg else ""


def check(rc: int) -> None:
    if rc != SMX_OK:
        raise RuntimeError(f"stereo_mi355x: {last_error()} (status {rc})")
