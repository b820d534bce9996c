"""vors_amd — Python host-side mirror of the reference's tracking interface over libvors_hip.so.

This is plumbing (ctypes over the C ABI of include/vors_hip.h), used by tests/ and bench.py; the product is the HIP
library. Names follow the reference crate (paths relative to the reference repository root):

    Intrinsics                 src/core/camera.rs:84-91
    Config / Config.init       src/core/track/inverse_compositional.rs:37-49, 74-100
    Tracker.track / .current_frame                      inverse_compositional.rs:170-248
    State / Continue / iterative_solve                  src/math/optimizer.rs:9-70   (the "optimizer trait")
    LMOptimizerState                                    src/core/track/lm_optimizer.rs:16-193
    se3_exp / se3_log / so3_exp / so3_log               src/math/se3.rs, src/math/so3.rs

There is no CPU fallback: importing works anywhere (so symbol checks can run without a GPU) but every compute call
raises VorsError when the library or a HIP device is missing.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VORS_HIP_LIB") or os.path.join(_HERE, "libvors_hip.so")  # VORS_HIP_LIB: development builds (ablations)
MAX_LEVELS = 8
RESIDUAL_BINS = 256  # VORS_RESIDUAL_BINS
RENDER_COUNTS = 4  # VORS_RENDER_COUNTS: considered, in front, landed, covered
NORMAL_COUNTS = 3  # VORS_NORMAL_COUNTS: considered, with depth, with a normal
UNDISTORT_COUNTS = 3  # VORS_UNDISTORT_COUNTS: pixels, grey inside, depth inside and non-zero
REGISTER_COUNTS = 4  # VORS_REGISTER_COUNTS: with depth, in front, landed, covered
SRC_NONE = 0xFFFFFFFF  # vors_register_depth's source index of a pixel nothing landed on
ICP_ITERATIONS, ICP_CONVERGED, ICP_TOO_FEW, ICP_SINGULAR = 0, 1, 2, 3  # VORS_ICP_*: vors_icp_stats.status

ROW_MAJOR, COL_MAJOR = 0, 1
CANDIDATES_COARSE_TO_FINE, CANDIDATES_DENSE, CANDIDATES_DSO = 0, 1, 2
TRACK_OK, TRACK_OPTIMIZER_FAILED_POSE_KEPT = 0, 1
ARITH_REFERENCE, ARITH_EXACT, ARITH_FUSED = 0, 1, 2  # 0 = the reference's own arithmetic AND summation order (bit-identical poses)


class VorsError(RuntimeError):
    pass


class vors_config(C.Structure):
    _fields_ = [
        ("nb_levels", C.c_int32),
        ("candidates_diff_threshold", C.c_int32),
        ("depth_scale", C.c_float),
        ("cu", C.c_float),
        ("cv", C.c_float),
        ("fu", C.c_float),
        ("fv", C.c_float),
        ("skew", C.c_float),
        ("idepth_variance", C.c_float),
        ("candidates_mode", C.c_int32),
        ("huber_delta", C.c_float),
        ("arithmetic", C.c_int32),
    ]


class vors_pair_stats(C.Structure):
    _fields_ = [
        ("lm_model", C.c_float * 7),
        ("optical_flow", C.c_float),
        ("change_keyframe", C.c_int32),
        ("nb_iter", C.c_int32 * MAX_LEVELS),
        ("n_points", C.c_int32 * MAX_LEVELS),
        ("energy", C.c_float * MAX_LEVELS),
        ("nb_grad_evals", C.c_int32 * MAX_LEVELS),
    ]


PAIR_STATS_DTYPE = np.dtype([
    ("lm_model", np.float32, 7),
    ("optical_flow", np.float32),
    ("change_keyframe", np.int32),
    ("nb_iter", np.int32, MAX_LEVELS),
    ("n_points", np.int32, MAX_LEVELS),
    ("energy", np.float32, MAX_LEVELS),
    ("nb_grad_evals", np.int32, MAX_LEVELS),
])
assert PAIR_STATS_DTYPE.itemsize == C.sizeof(vors_pair_stats)


class vors_obs(C.Structure):
    _fields_ = [
        ("cu", C.c_float), ("cv", C.c_float), ("fu", C.c_float), ("fv", C.c_float), ("skew", C.c_float),
        ("rows", C.c_int32), ("cols", C.c_int32),
        ("template_", C.POINTER(C.c_uint8)),
        ("image", C.POINTER(C.c_uint8)),
        ("n", C.c_int32),
        ("coordinates", C.POINTER(C.c_int32)),
        ("_z_candidates", C.POINTER(C.c_float)),
        ("jacobians", C.POINTER(C.c_float)),
        ("huber_delta", C.c_float),
        ("arithmetic", C.c_int32),
    ]


# every symbol include/vors_hip.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = [
    "vors_last_error", "vors_device_count", "vors_device_info", "vors_abi_version", "vors_selfcheck_isqrt",
    "vors_tracker_create", "vors_tracker_track", "vors_tracker_track_checked", "vors_tracker_current_frame", "vors_tracker_last_stats",
    "vors_tracker_keyframe", "vors_tracker_enable_depth_filter", "vors_tracker_enable_map", "vors_tracker_read_map", "vors_tracker_enable_map_voxels",
    "vors_tracker_read_map_voxels", "vors_tracker_render_map", "vors_tracker_destroy",
    "vors_track_pairs",
    "vors_batch_create", "vors_batch_create_on", "vors_batch_device", "vors_batch_track_pairs", "vors_batch_prepare_keyframes", "vors_batch_track_current",
    "vors_batch_workspace_bytes", "vors_batch_enable_kernel_timing", "vors_batch_kernel_times", "vors_batch_last_kernel_ms",
    "vors_batch_destroy",
    "vors_batch_get_keyframe_image", "vors_batch_get_current_image", "vors_batch_get_points", "vors_batch_eval_level", "vors_batch_lm_predict_log",
    "vors_batch_eval_pairs", "vors_batch_pose_information", "vors_pose_information_from_sums",
    "vors_batch_residual_maps", "vors_residual_scale_from_hist",
    "vors_batch_reproject_depth", "vors_to_depth", "vors_from_depth",
    "vors_batch_point_cloud", "vors_camera_back_project", "vors_camera_project",
    "vors_batch_fuse_depth", "vors_fuse_depth_pixels",
    "vors_render_points", "vors_render_points_host", "vors_trackers_render_map",
    "vors_depth_normals", "vors_points_normals", "vors_depth_normals_host", "vors_trackers_enable_map_normals", "vors_trackers_map_normals",
    "vors_undistort_frames", "vors_undistort_frame_host", "vors_undistort_source_host", "vors_register_depth", "vors_register_depth_host",
    "vors_icp_workspace_bytes", "vors_icp_points", "vors_icp_points_host", "vors_trackers_icp_map",
    "vors_icp_points_robust", "vors_icp_points_robust_host", "vors_trackers_icp_map_robust",
    "vors_icp_points_joint", "vors_icp_points_joint_host", "vors_trackers_icp_map_joint",
    "vors_pose_graph_workspace_bytes", "vors_pose_graph_optimize", "vors_pose_graph_optimize_host", "vors_pose_graph_jacobians_host",
    "vors_loop_signatures", "vors_loop_signatures_host", "vors_loop_candidates", "vors_loop_candidates_host",
    "vors_loop_verify_edges", "vors_loop_verify_edges_host",
    "vors_repose_points", "vors_repose_points_host", "vors_trackers_repose_map",
    "vors_voxel_filter_workspace_bytes", "vors_voxel_filter_points", "vors_voxel_filter_points_host",
    "vors_tracker_enable_map_normals", "vors_tracker_read_map_normals",
    "vors_trackers_enable_map_icp", "vors_trackers_map_icp", "vors_tracker_enable_map_icp", "vors_tracker_read_map_icp",
    "vors_map_icp_window_host", "vors_map_icp_verdict_host",
    "vors_icp_condition_from_sums", "vors_icp_condition", "vors_trackers_enable_map_icp_joint", "vors_trackers_map_icp_joint",
    "vors_tracker_enable_map_icp_joint", "vors_tracker_read_map_icp_joint", "vors_map_icp_verdict_joint_host",
    "vors_trackers_enable_map_icp_means", "vors_trackers_map_icp_means", "vors_tracker_enable_map_icp_means", "vors_tracker_read_map_icp_means",
    "vors_lm_eval", "vors_lm_step", "vors_lm_solve",
    "vors_ref_sincos", "vors_se3_exp", "vors_se3_log", "vors_so3_exp", "vors_so3_log", "vors_iso_mul", "vors_iso_inverse",
    "vors_synth_render_pairs",
    "vors_multi_create", "vors_multi_device_count", "vors_multi_shard", "vors_multi_track_pairs", "vors_multi_track_pairs_host",
    "vors_multi_destroy", "vors_multi_rccl_version",
    "vors_trackers_create", "vors_trackers_create_on", "vors_trackers_count", "vors_trackers_init", "vors_trackers_track", "vors_trackers_state",
    "vors_trackers_current_frames", "vors_trackers_last_stats", "vors_trackers_enable_kernel_timing", "vors_trackers_kernel_times", "vors_trackers_destroy",
    "vors_trackers_enable_depth_filter", "vors_trackers_keyframe_depth", "vors_trackers_workspace_bytes",
    "vors_trackers_enable_map", "vors_trackers_map", "vors_trackers_enable_map_voxels", "vors_trackers_map_voxels", "vors_voxel_keys",
    "vors_trackers_enable_map_voxel_stats", "vors_trackers_map_voxel_stats", "vors_trackers_map_voxel_means", "vors_tracker_enable_map_voxel_stats",
    "vors_tracker_read_map_voxel_stats", "vors_tracker_map_voxel_means", "vors_voxel_means", "vors_voxel_means_host", "vors_voxel_stats_host",
    "vors_synth_render_frames",
    "vors_pipeline_create", "vors_pipeline_submit", "vors_pipeline_wait", "vors_pipeline_drain", "vors_pipeline_destroy",
]

_lib = None


def lib():
    """Load libvors_hip.so. Import torch first when sharing device memory with it (same HIP runtime SONAME)."""
    global _lib
    if _lib is None:
        # torch ships its own HIP runtime: load it FIRST so that libvors_hip.so binds to the same one (two runtimes in one process
        # do not see each other's devices / allocations). The library itself does not depend on torch.
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        if not os.path.exists(LIB_PATH):
            raise VorsError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback)")
        _lib = C.CDLL(LIB_PATH)
        _lib.vors_last_error.restype = C.c_char_p
        vp, i, d, f = C.c_void_p, C.c_int, C.c_double, C.c_float
        _lib.vors_tracker_create.argtypes = [C.POINTER(vors_config), d, vp, d, vp, i, i, i, C.POINTER(vp)]
        _lib.vors_tracker_track.argtypes = [vp, d, vp, d, vp, C.POINTER(i)]
        _lib.vors_tracker_track_checked.argtypes = [vp, d, vp, d, vp, i, i, C.POINTER(i)]
        _lib.vors_tracker_current_frame.argtypes = [vp, C.POINTER(d), vp]
        _lib.vors_tracker_keyframe.argtypes = [vp, C.POINTER(d), vp]
        _lib.vors_tracker_last_stats.argtypes = [vp, C.POINTER(vors_pair_stats)]
        _lib.vors_tracker_destroy.argtypes = [vp]
        _lib.vors_tracker_destroy.restype = None
        _lib.vors_track_pairs.argtypes = [C.POINTER(vors_config), i, vp, vp, vp, i, i, i, vp, vp, vp, vp]
        _lib.vors_batch_create.argtypes = [C.POINTER(vors_config), i, i, i, C.POINTER(vp)]
        _lib.vors_batch_create_on.argtypes = [i, C.POINTER(vors_config), i, i, i, C.POINTER(vp)]
        _lib.vors_batch_device.argtypes = [vp, C.POINTER(i)]
        _lib.vors_multi_create.argtypes = [C.POINTER(vors_config), i, vp, i, i, i, C.POINTER(vp)]
        _lib.vors_multi_device_count.argtypes = [vp]
        _lib.vors_multi_shard.argtypes = [vp, i, i, C.POINTER(i), C.POINTER(i)]
        _lib.vors_multi_track_pairs.argtypes = [vp, i, vp, vp, vp, vp, vp]
        _lib.vors_multi_track_pairs_host.argtypes = [vp, i, vp, vp, vp, vp, vp]
        _lib.vors_multi_destroy.argtypes = [vp]
        _lib.vors_multi_destroy.restype = None
        _lib.vors_multi_rccl_version.argtypes = [vp]
        _lib.vors_trackers_create.argtypes = [C.POINTER(vors_config), i, i, i, C.POINTER(vp)]
        _lib.vors_trackers_create_on.argtypes = [i, C.POINTER(vors_config), i, i, i, C.POINTER(vp)]
        _lib.vors_trackers_count.argtypes = [vp]
        _lib.vors_trackers_init.argtypes = [vp, vp, vp, vp]
        _lib.vors_trackers_track.argtypes = [vp, vp, vp, vp]
        _lib.vors_trackers_state.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        _lib.vors_trackers_current_frames.argtypes = [vp, vp, vp, vp, vp]
        _lib.vors_trackers_last_stats.argtypes = [vp, vp, vp]
        _lib.vors_trackers_enable_kernel_timing.argtypes = [vp, i]
        _lib.vors_trackers_kernel_times.argtypes = [vp, i, vp, i, C.POINTER(i)]
        _lib.vors_trackers_destroy.argtypes = [vp]
        _lib.vors_trackers_destroy.restype = None
        _lib.vors_trackers_enable_depth_filter.argtypes = [vp, f, i, i]
        _lib.vors_trackers_keyframe_depth.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        _lib.vors_trackers_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
        _lib.vors_tracker_enable_depth_filter.argtypes = [vp, f, i, i]
        _lib.vors_trackers_enable_map.argtypes = [vp, i, i, i, i]
        _lib.vors_trackers_map.argtypes = [vp] + [C.POINTER(vp)] * 6
        _lib.vors_tracker_enable_map.argtypes = [vp, i, i, i, i]
        _lib.vors_tracker_read_map.argtypes = [vp, i, vp, vp, vp, C.POINTER(C.c_uint32), i, vp, C.POINTER(C.c_uint32)]
        _lib.vors_trackers_enable_map_voxels.argtypes = [vp, f, i]
        _lib.vors_trackers_map_voxels.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        _lib.vors_tracker_enable_map_voxels.argtypes = [vp, f, i]
        _lib.vors_tracker_read_map_voxels.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _lib.vors_trackers_enable_map_voxel_stats.argtypes = [vp]
        _lib.vors_trackers_map_voxel_stats.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        _lib.vors_trackers_map_voxel_means.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        _lib.vors_tracker_enable_map_voxel_stats.argtypes = [vp]
        _lib.vors_tracker_read_map_voxel_stats.argtypes = [vp, i, vp, vp]
        _lib.vors_tracker_map_voxel_means.argtypes = [vp, C.c_uint32, C.c_uint32, i, vp, vp, C.POINTER(C.c_uint32)]
        _lib.vors_voxel_means.argtypes = [i, vp, vp, i, vp, vp, f, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
        _lib.vors_voxel_means_host.argtypes = [vp, C.c_uint32, i, vp, vp, f, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint32)]
        _lib.vors_voxel_stats_host.argtypes = [vp, vp, vp, C.c_uint32, f, i, C.POINTER(C.c_uint32), vp, vp, vp]
        _lib.vors_render_points.argtypes = [i, vp, vp, vp, i, vp, C.c_size_t, vp, i, i, f, vp, C.c_size_t, i, vp, vp, vp, vp, vp]
        _lib.vors_render_points_host.argtypes = [vp, vp, C.c_uint32, i, vp, vp, i, i, f, vp, i, vp, vp, vp, vp]
        _lib.vors_trackers_render_map.argtypes = [vp, i, vp, C.c_size_t, vp, C.c_size_t, i, vp, vp, vp, vp, vp]
        _lib.vors_tracker_render_map.argtypes = [vp, i, vp, vp, i, vp, vp, vp, vp]
        _lib.vors_depth_normals.argtypes = [i, vp, vp, i, i, f, i, f, vp, C.c_size_t, vp, vp, vp]
        _lib.vors_points_normals.argtypes = [i, vp, vp, vp, i, vp, C.c_size_t, vp, i, i, f, i, f, vp, C.c_size_t, vp, vp, vp]
        _lib.vors_depth_normals_host.argtypes = [vp, vp, i, i, f, i, f, vp, vp, C.c_uint32, i, vp, vp, vp]
        _lib.vors_trackers_enable_map_normals.argtypes = [vp, i, f]
        _lib.vors_trackers_map_normals.argtypes = [vp, C.POINTER(vp)]
        _lib.vors_tracker_enable_map_normals.argtypes = [vp, i, f]
        _lib.vors_tracker_read_map_normals.argtypes = [vp, i, vp]
        _lib.vors_undistort_frames.argtypes = [i, vp, vp, i, i, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]
        _lib.vors_undistort_frame_host.argtypes = [vp, vp, i, i, vp, vp, vp, i, i, i, vp, vp, vp, vp]
        _lib.vors_undistort_source_host.argtypes = [vp, vp, vp, i, vp, vp]
        _lib.vors_register_depth.argtypes = [i, vp, vp, i, i, f, vp, vp, i, i, f, i, vp, vp, vp, vp, vp]
        _lib.vors_register_depth_host.argtypes = [vp, vp, i, i, f, vp, vp, i, i, f, i, vp, vp, vp, vp]
        _lib.vors_icp_workspace_bytes.argtypes = [i, i]
        _lib.vors_icp_workspace_bytes.restype = C.c_uint64
        # The nine ICP entries (include/vors_hip.h 2e and the handle's forwards) from the pieces their lists share, each counted once:
        u32, sz = C.c_uint32, C.c_size_t
        strided = [vp, sz, vp, sz]  # ranges and poses, each with its stride in bytes
        plane = [i, i, f]  # rows, cols, depth_scale
        scalars = [f, f, f, i, i]  # dist_m, damping, step_eps, iters, min_points
        out = [vp, vp, vp, vp]  # poses, stats, sums29, residuals
        robust, joint = [vp, f, f], [f, f]  # frame normals, min_cos, huber_m; photo_scale_m, photo_huber_grey
        # per form: the grey levels (of the lists, of the frames: one pointer each), its inputs behind min_points, its outputs behind residuals
        for form, gray, more_in, more_out in (("", [], [], []), ("_robust", [], robust, [vp]), ("_joint", [vp], robust + joint, [vp, vp, vp])):
            getattr(_lib, f"vors_icp_points{form}").argtypes = ([i, vp, vp] + gray + [vp, i] + strided + [vp] + gray + [vp] + plane + scalars + more_in
                                                                + [vp] + out + more_out + [vp])
            getattr(_lib, f"vors_icp_points{form}_host").argtypes = ([vp, vp] + gray + [u32, i, vp, vp, vp] + gray + [vp] + plane + scalars + more_in
                                                                     + out + more_out)
            getattr(_lib, f"vors_trackers_icp_map{form}").argtypes = [vp, vp] + gray + scalars + strided + more_in + [vp] + out + more_out + [vp]
        _lib.vors_pose_graph_workspace_bytes.argtypes = [i, i, i]
        _lib.vors_pose_graph_workspace_bytes.restype = C.c_uint64
        pg_scalars = [f, f, f, i, i]  # lambda0, step_eps, cg_tol, iters, cg_iters
        _lib.vors_pose_graph_optimize.argtypes = [i, vp, sz, vp, i, vp, vp, i, vp, vp, vp, vp] + pg_scalars + [vp, vp, vp, vp, vp, vp]
        _lib.vors_pose_graph_optimize_host.argtypes = [vp, u32, i, vp, u32, i, vp, vp, vp, vp] + pg_scalars + [vp, vp, vp, vp]
        _lib.vors_pose_graph_jacobians_host.argtypes = [vp] * 6
        _lib.vors_pose_graph_jacobians_host.restype = None
        _lib.vors_loop_signatures.argtypes = [i, vp, i, i, i, i, vp, vp, vp]
        _lib.vors_loop_signatures_host.argtypes = [vp, i, i, i, i, vp, vp]
        lc_gates = [u32, i, f, f, f]  # min_gap, k, min_score, max_dist_m, min_qdot
        _lib.vors_loop_candidates.argtypes = [i, vp, vp, vp, i, i, vp, sz, vp] + lc_gates + [vp, vp, vp, vp]
        _lib.vors_loop_candidates_host.argtypes = [vp, vp, u32, i, i, vp, u32] + lc_gates + [vp, vp, vp]
        lc_verify = [u32, vp, vp, sz, vp, sz, vp, vp, vp, vp, sz, u32, f, f, f, f, f, vp, vp, vp, vp, vp, i, vp, vp, vp]
        _lib.vors_loop_verify_edges.argtypes = lc_verify + [vp]
        _lib.vors_loop_verify_edges_host.argtypes = lc_verify
        repose_out = [vp, vp, vp, vp]  # xyz, normals, segments, counts
        _lib.vors_repose_points.argtypes = [i, vp, vp, vp, i, vp, vp, i, vp, sz, i, vp, vp] + repose_out + [vp]
        _lib.vors_repose_points_host.argtypes = [vp, vp, u32, i, vp, u32, i, vp, u32, i, vp] + repose_out
        _lib.vors_trackers_repose_map.argtypes = [vp, vp, sz, i, vp, vp] + repose_out + [vp]
        _lib.vors_voxel_filter_workspace_bytes.argtypes = [i, i, i]
        _lib.vors_voxel_filter_workspace_bytes.restype = C.c_uint64
        _lib.vors_voxel_filter_points.argtypes = [i, vp, vp, i, f, i, vp, vp, vp, vp, vp, vp, i] + [vp] * 8 + [vp]
        _lib.vors_voxel_filter_points_host.argtypes = [vp, u32, i, f, i, vp, vp, vp, vp, u32, i, vp, C.POINTER(u32), C.POINTER(u32)] + [vp] * 5
        _lib.vors_trackers_enable_map_icp.argtypes = [vp, vp]
        _lib.vors_trackers_map_icp.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        _lib.vors_tracker_enable_map_icp.argtypes = [vp, vp]
        _lib.vors_tracker_read_map_icp.argtypes = [vp, vp, vp]
        _lib.vors_map_icp_window_host.argtypes = [vp, C.c_uint32, i, C.c_uint32, i, i, vp]
        _lib.vors_map_icp_verdict_host.argtypes = [vp, vp, vp, vp, vp]
        _lib.vors_icp_condition_from_sums.argtypes = [vp, vp, vp, vp]
        _lib.vors_icp_condition.argtypes = [i, vp, vp, vp, vp]
        _lib.vors_trackers_enable_map_icp_joint.argtypes = [vp, vp]
        _lib.vors_trackers_map_icp_joint.argtypes = [vp, C.POINTER(vp)]
        _lib.vors_tracker_enable_map_icp_joint.argtypes = [vp, vp]
        _lib.vors_tracker_read_map_icp_joint.argtypes = [vp, vp]
        _lib.vors_map_icp_verdict_joint_host.argtypes = [vp, vp, vp, vp, f, f, vp]
        _lib.vors_trackers_enable_map_icp_means.argtypes = [vp, C.c_uint32, C.c_uint32]
        _lib.vors_trackers_map_icp_means.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        _lib.vors_tracker_enable_map_icp_means.argtypes = [vp, C.c_uint32, C.c_uint32]
        _lib.vors_tracker_read_map_icp_means.argtypes = [vp, vp]
        _lib.vors_voxel_keys.argtypes = [f, vp, i, vp]
        _lib.vors_voxel_keys.restype = None
        _lib.vors_synth_render_frames.argtypes = [i, vp, vp, vp, i, i, vp, i, vp, vp, vp]
        _lib.vors_batch_track_pairs.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.vors_pipeline_create.argtypes = [i, C.POINTER(vors_config), i, i, i, i, C.POINTER(vp)]
        _lib.vors_pipeline_submit.argtypes = [vp, i, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int64)]
        _lib.vors_pipeline_wait.argtypes = [vp, C.c_int64, vp, i]
        _lib.vors_pipeline_drain.argtypes = [vp, vp, i]
        _lib.vors_pipeline_destroy.argtypes = [vp]
        _lib.vors_pipeline_destroy.restype = None
        _lib.vors_batch_prepare_keyframes.argtypes = [vp, i, vp, vp, vp]
        _lib.vors_batch_track_current.argtypes = [vp, i, vp, vp, vp, vp, vp, vp]
        _lib.vors_batch_workspace_bytes.argtypes = [vp, C.POINTER(C.c_uint64)]
        _lib.vors_batch_enable_kernel_timing.argtypes = [vp, i]
        _lib.vors_batch_kernel_times.argtypes = [vp, i, vp, i, C.POINTER(i)]
        _lib.vors_batch_last_kernel_ms.argtypes = [vp, C.POINTER(f), C.POINTER(f), C.POINTER(f)]
        _lib.vors_batch_destroy.argtypes = [vp]
        _lib.vors_batch_destroy.restype = None
        _lib.vors_batch_get_keyframe_image.argtypes = [vp, i, i, vp, C.POINTER(i), C.POINTER(i)]
        _lib.vors_batch_get_current_image.argtypes = [vp, i, i, vp, C.POINTER(i), C.POINTER(i)]
        _lib.vors_batch_get_points.argtypes = [vp, i, i, i, vp, vp, vp, vp, C.POINTER(i)]
        _lib.vors_batch_eval_level.argtypes = [vp, i, i, vp, i, vp]
        _lib.vors_batch_lm_predict_log.argtypes = [vp, i, vp]
        _lib.vors_batch_eval_pairs.argtypes = [vp, i, i, i, vp, C.c_size_t, i, i, vp, vp]
        _lib.vors_batch_pose_information.argtypes = [vp, i, i, vp, C.c_size_t, vp, vp, vp, vp, vp]
        _lib.vors_pose_information_from_sums.argtypes = [vp, vp, vp, C.POINTER(f), C.POINTER(C.c_int32)]
        _lib.vors_batch_residual_maps.argtypes = [vp, i, i, vp, C.c_size_t, vp, vp, vp, vp, vp]
        _lib.vors_residual_scale_from_hist.argtypes = [vp, C.POINTER(f), C.POINTER(f), C.POINTER(C.c_uint32)]
        _lib.vors_batch_reproject_depth.argtypes = [vp, i, i, vp, C.c_size_t, vp, f, vp, vp, vp, vp, vp]
        for name in ("vors_to_depth", "vors_from_depth"):
            getattr(_lib, name).argtypes = [f, vp, i, vp]
            getattr(_lib, name).restype = None
        _lib.vors_batch_point_cloud.argtypes = [vp, i, i, vp, C.c_size_t, vp, i, vp, vp, vp, vp, vp]
        _lib.vors_camera_back_project.argtypes = [vp, vp, vp, vp, i, vp]
        _lib.vors_camera_back_project.restype = None
        _lib.vors_camera_project.argtypes = [vp, vp, vp, i, vp]
        _lib.vors_camera_project.restype = None
        _lib.vors_batch_fuse_depth.argtypes = [vp, i, vp, C.c_size_t, vp, f, vp, i, i, vp, vp, vp, vp, vp]
        _lib.vors_fuse_depth_pixels.argtypes = [f, f, i, i, C.c_size_t, vp, vp, vp, C.c_size_t, vp, vp, vp]
        _lib.vors_lm_eval.argtypes = [C.POINTER(vors_obs), vp, C.POINTER(f), C.POINTER(C.c_int32), vp, vp, vp]
        _lib.vors_ref_sincos.argtypes = [vp, i, vp, vp]
        _lib.vors_ref_sincos.restype = None
        _lib.vors_lm_step.argtypes = [vp, vp, vp, f, vp, C.POINTER(i)]
        _lib.vors_lm_solve.argtypes = [C.POINTER(vors_obs), vp, vp, C.POINTER(C.c_int32), C.POINTER(f), C.POINTER(f), C.POINTER(i)]
        _lib.vors_synth_render_pairs.argtypes = [C.c_uint64, i, i, i, vp, d, i, vp, vp, vp, vp, vp, vp]
        for name in ("vors_se3_exp", "vors_se3_log", "vors_so3_exp", "vors_so3_log", "vors_iso_inverse"):
            getattr(_lib, name).argtypes = [vp, vp]
            getattr(_lib, name).restype = None
        _lib.vors_iso_mul.argtypes = [vp, vp, vp]
        _lib.vors_iso_mul.restype = None
    return _lib


def _check(st):
    if st != 0:
        raise VorsError(f"vors_hip error {st}: {lib().vors_last_error().decode()}")


def device_count():
    return lib().vors_device_count()


def device_info(device=0):
    """-> dict(clock_khz = peak shader clock, compute_units, memory_bytes) of a HIP device."""
    clk, cu, mem = C.c_int(), C.c_int(), C.c_uint64()
    lib().vors_device_info.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    _check(lib().vors_device_info(int(device), C.byref(clk), C.byref(cu), C.byref(mem)))
    return dict(clock_khz=clk.value, compute_units=cu.value, memory_bytes=mem.value)


def selfcheck_isqrt():
    """Arguments 0 .. 65535 for which the DSO selector's four-instruction integer root differs from floor(sqrt(n)) on this device (0)."""
    n = C.c_int(-1)
    lib().vors_selfcheck_isqrt.argtypes = [C.POINTER(C.c_int)]
    _check(lib().vors_selfcheck_isqrt(C.byref(n)))
    return n.value


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _asked(o):
    """An output argument that may also be a tensor to write into: anything but False / None asks for the output."""
    return o is not False and o is not None


def _out_buf(o, shape, dtype, dev, always=False):
    """The tensor behind an output argument: True = a new one, a tensor = that one after a check of dtype, shape and contiguity, False /
    None = not wanted (always: made all the same, for a plane the pass needs)."""
    import torch
    if o is True or (always and not _asked(o)):
        return torch.empty(shape, dtype=dtype, device=dev)
    if not _asked(o):
        return None
    if o.dtype != dtype or not o.is_contiguous() or tuple(o.shape) != tuple(shape):
        raise VorsError(f"expected a contiguous {dtype} output {tuple(shape)}, got {o.dtype} {tuple(o.shape)}")
    return o


def _result(*items):
    """(name, kept, tensor) per output -> the dict a product returns: the kept ones. `kept` is the caller's own test of its argument: the
    argument itself where it is a flag, _asked() of it where it may be a tensor."""
    return {name: t for name, kept, t in items if kept}


# ----------------------------------------------------------------------------------------------- reference mirror
class Intrinsics:
    """src/core/camera.rs:84-91."""

    def __init__(self, principal_point, focal, skew=0.0):
        self.principal_point = (float(principal_point[0]), float(principal_point[1]))
        self.focal = (float(focal[0]), float(focal[1]))
        self.skew = float(skew)


# src/dataset/tum_rgbd.rs:15-52
DEPTH_SCALE = 5000.0
INTRINSICS_ICL_NUIM = Intrinsics((319.5, 239.5), (481.20, -480.00), 0.0)
INTRINSICS_FR1 = Intrinsics((318.643040, 255.313989), (517.306408, 516.469215), 0.0)
INTRINSICS_FR2 = Intrinsics((325.141442, 249.701764), (520.908620, 521.007327), 0.0)
INTRINSICS_FR3 = Intrinsics((320.106653, 247.632132), (535.433105, 539.212524), 0.0)


def scaled_intrinsics(rows, cols, base=INTRINSICS_FR1):
    """Intrinsics of the synthetic scenes: FR1 for 640x480; other sizes scale by s = cols / 640:
    f' = s f, c' = s (c + 0.5) - 0.5. Returns (cu, cv, fu, fv, skew)."""
    s = cols / 640.0
    cu, cv = base.principal_point
    fu, fv = base.focal
    return (s * (cu + 0.5) - 0.5, s * (cv + 0.5) - 0.5, s * fu, s * fv, base.skew)


class Config:
    """src/core/track/inverse_compositional.rs:37-49 (+ two extension fields, zero = reference behaviour)."""

    def __init__(self, nb_levels=6, candidates_diff_threshold=7, depth_scale=DEPTH_SCALE, intrinsics=INTRINSICS_FR1,
                 idepth_variance=0.0001, candidates_mode=CANDIDATES_COARSE_TO_FINE, huber_delta=0.0, arithmetic=ARITH_REFERENCE):
        self.nb_levels = nb_levels
        self.candidates_diff_threshold = candidates_diff_threshold
        self.depth_scale = depth_scale
        self.intrinsics = intrinsics
        self.idepth_variance = idepth_variance
        self.candidates_mode = candidates_mode
        self.huber_delta = huber_delta
        self.arithmetic = arithmetic

    def to_c(self):
        k = self.intrinsics
        return vors_config(self.nb_levels, self.candidates_diff_threshold, self.depth_scale, k.principal_point[0],
                           k.principal_point[1], k.focal[0], k.focal[1], k.skew, self.idepth_variance,
                           self.candidates_mode, self.huber_delta, self.arithmetic)

    def init(self, keyframe_depth_timestamp, depth_map, keyframe_img_timestamp, img, layout=ROW_MAJOR):
        """Config::init (inverse_compositional.rs:74-100) -> Tracker."""
        return Tracker(self, keyframe_depth_timestamp, depth_map, keyframe_img_timestamp, img, layout)


_REQUIRED = object()


def _spec_args(switch, fields, spec, scalar=False, lenient=False):
    """The one parser of the switches' tuples. fields: (name, int or float, default or _REQUIRED) per value, in order. None -> None, else
    the typed values with the defaults filled in. Only the SHAPE of the argument is judged here; the values are judged by the library, in
    one place for every caller. scalar: a bare number stands for (number,). lenient (depth_filter, kept as it always was): the integers are
    not held to the range of a C int, and the numbers are converted with float(), after the integers, rather than tested by type."""
    if spec is None:
        return None
    names = [f[0] for f in fields]
    lo, hi = sum(f[2] is _REQUIRED for f in fields), len(fields)
    sig = "(" + ", ".join(names[:lo]) + "".join(f"[, {n}" for n in names[lo:]) + "]" * (hi - lo) + ")"
    if scalar and isinstance(spec, (int, float, np.integer, np.floating)) and not isinstance(spec, bool):
        spec = (spec,)
    try:
        spec = tuple(spec)
    except TypeError:
        raise VorsError(f"{switch}: expected None or {sig}, got {spec!r}") from None
    if not lo <= len(spec) <= hi:
        count = str(lo) if lo == hi else f"{lo} or {hi}" if hi == lo + 1 else f"{lo} to {hi}"
        raise VorsError(f"{switch}: expected {count} values {sig}, got {len(spec)}")
    out = list(spec) + [f[2] for f in fields[len(spec):]]

    def integer(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise VorsError(f"{switch}: {name} must be an integer, got {v!r}")
        if not lenient and not -2 ** 31 <= int(v) < 2 ** 31:
            raise VorsError(f"{switch}: {name} does not fit the C int it is passed as, got {v!r}")
        return int(v)

    def number(name, v):
        if lenient:
            try:
                return float(v)
            except (TypeError, ValueError):
                pass
        elif not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)):
            return float(v)
        raise VorsError(f"{switch}: {name} must be a number, got {v!r}") from None

    for kinds in ((int,), (float,)) if lenient else ((int, float),):
        for i, (name, kind, _) in enumerate(fields):
            if kind in kinds:
                out[i] = integer(name, out[i]) if kind is int else number(name, out[i])
    return tuple(out)


def _depth_filter_args(spec):
    """None, a number or (tol_m[, max_weight[, fill_min_weight]]) -> None or (float, int, int)."""
    return _spec_args("depth_filter", (("tol_m", float, _REQUIRED), ("max_weight", int, 255), ("fill_min_weight", int, 0)), spec, scalar=True,
                      lenient=True)


class vors_map_segment(C.Structure):
    """One keyframe of a sequence's map (include/vors_hip.h vors_map_segment, 40 bytes)."""
    _fields_ = [("frame", C.c_int32), ("first", C.c_uint32), ("count", C.c_uint32), ("pose7", C.c_float * 7)]


MAP_SEGMENT_DTYPE = np.dtype([("frame", "<i4"), ("first", "<u4"), ("count", "<u4"), ("pose7", "<f4", (7,))])


def decode_map_segments(segments):
    """The "segments" entry of Trackers.map() (uint8 [n, max_keyframes, 40], any device) -> structured numpy array [n, max_keyframes]."""
    a = segments.cpu().numpy() if hasattr(segments, "cpu") else np.asarray(segments)
    return np.ascontiguousarray(a).view(MAP_SEGMENT_DTYPE)[..., 0]


def _map_args(spec):
    """None or (level, capacity, max_keyframes[, min_weight]) -> None or four ints."""
    return _spec_args("map", (("level", int, _REQUIRED), ("capacity", int, _REQUIRED), ("max_keyframes", int, _REQUIRED), ("min_weight", int, 0)), spec)


def _map_voxels_args(spec):
    """None or (voxel_m, table_slots) -> None or (float, int); the library wants a finite voxel_m > 0 and a power of two in 64..2^30."""
    return _spec_args("map_voxels", (("voxel_m", float, _REQUIRED), ("table_slots", int, _REQUIRED)), spec)


def _map_normals_args(spec):
    """None or (step, jump_m) -> None or (int, float); the library wants step in 1..8 and jump_m >= 0."""
    return _spec_args("map_normals", (("step", int, _REQUIRED), ("jump_m", float, _REQUIRED)), spec)


VOXEL_NONE = 0xFFFFFFFFFFFFFFFF


def voxel_keys(voxel_m, xyz):
    """The voxel keys of points on a grid of edge voxel_m, on the host (vors_voxel_keys; needs no GPU): xyz [..., 3] float32 -> uint64
    [...], the rule of the keyframe map's voxel filter (Trackers.enable_map_voxels). VOXEL_NONE where a point has no key."""
    p = np.ascontiguousarray(xyz, np.float32)
    if p.ndim < 1 or p.shape[-1] != 3:
        raise VorsError("voxel_keys: xyz must be [..., 3]")
    if p.size // 3 >= 2 ** 31:
        raise VorsError("voxel_keys: too many points for one call")
    out = np.empty(p.shape[:-1], np.uint64)
    lib().vors_voxel_keys(float(voxel_m), _ptr(p), p.size // 3, _ptr(out))
    return out


def _u32(name, v):
    """An argument the library takes as uint32."""
    v = int(v)
    if v < 0 or v > 0xFFFFFFFF:
        raise VorsError(f"{name} must be in 0..2^32 - 1")
    return v


def voxel_stats_host(xyz, gray, voxel_m, capacity, segment_of=None):
    """The statistics of the map's voxels for ONE unfiltered list on the host (vors_voxel_stats_host; needs no GPU; the texts the kernels
    run): xyz [m, 3] float32, gray [m] uint8, segment_of [m] uint32 (the segment index of every entry; None = all 0) -> dict: "total", the
    unclipped length of the filtered list, "first_index" [k] uint32, the index of every rank's first point, k = min(total, capacity),
    "sums" [k, 4] int64 and "obs" [k, 2] uint32 (count, last segment) — what Trackers.map_voxel_stats() holds for the sequence."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    g = np.ascontiguousarray(gray, np.uint8).reshape(-1)
    seg = None if segment_of is None else np.ascontiguousarray(segment_of, np.uint32).reshape(-1)
    if len(p) != len(g) or (seg is not None and len(seg) != len(p)):
        raise VorsError("voxel_stats_host: xyz [m, 3], gray [m], segment_of [m] or None")
    cap = int(capacity)
    total = C.c_uint32()
    first = np.zeros(max(cap, 0), np.uint32)
    sums, obs = np.zeros((max(cap, 0), 4), np.int64), np.zeros((max(cap, 0), 2), np.uint32)
    _check(lib().vors_voxel_stats_host(_ptr(p), _ptr(g), _ptr(seg), len(p), float(voxel_m), cap, C.byref(total), _ptr(first), _ptr(sums), _ptr(obs)))
    k = min(total.value, cap)
    return dict(total=total.value, first_index=first[:k], sums=sums[:k], obs=obs[:k])


def voxel_means_host(xyz, sums, obs, voxel_m, min_count=1, min_span=0, first_segment_of_rank=None, count=None):
    """The rule of voxel_means for ONE list on the host (vors_voxel_means_host; needs no GPU; the text the kernel runs): xyz [capacity, 3]
    float32, sums [capacity, 4] int64, obs [capacity, 2] uint32, count = the list's count (None = capacity; above it: clipped),
    first_segment_of_rank [capacity] uint32 or None (then min_span must be 0) -> dict: "xyz_mean" [capacity, 3] float32 and "gray_mean"
    [capacity] uint8 (zeros beyond the clipped count), "kept"."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(sums, np.int64).reshape(-1, 4)
    o = np.ascontiguousarray(obs, np.uint32).reshape(-1, 2)
    fs = None if first_segment_of_rank is None else np.ascontiguousarray(first_segment_of_rank, np.uint32).reshape(-1)
    if len(s) != len(p) or len(o) != len(p) or (fs is not None and len(fs) != len(p)):
        raise VorsError("voxel_means_host: xyz [capacity, 3], sums [capacity, 4], obs [capacity, 2], first_segment_of_rank [capacity] or None")
    out = dict(xyz_mean=np.zeros((len(p), 3), np.float32), gray_mean=np.zeros(len(p), np.uint8))
    kept = C.c_uint32()
    _check(lib().vors_voxel_means_host(_ptr(p), len(p) if count is None else _u32("count", count), len(p), _ptr(s), _ptr(o), float(voxel_m),
                                       _u32("min_count", min_count), _u32("min_span", min_span), _ptr(fs), _ptr(out["xyz_mean"]),
                                       _ptr(out["gray_mean"]), C.byref(kept)))
    out["kept"] = kept.value
    return out


class Tracker:
    """core::track::inverse_compositional::Tracker. Construct through Config.init."""

    def __init__(self, config, depth_t, depth_map, img_t, img, layout=ROW_MAJOR, depth_filter=None, map=None, map_voxels=None,
                 map_normals=None, map_icp=None, map_icp_joint=None, map_voxel_stats=False, map_icp_means=None):
        """depth_filter: None, or (tol_m[, max_weight[, fill_min_weight]]) — the recursive depth filter across keyframe promotions
        (vors_tracker_enable_depth_filter; Trackers.enable_depth_filter). map: None, or (level, capacity, max_keyframes[, min_weight]) — the
        keyframe map (vors_tracker_enable_map; Trackers.enable_map), switched on after the filter; read_map() returns it. map_voxels: None,
        or (voxel_m, table_slots) — the map's voxel filter (vors_tracker_enable_map_voxels; Trackers.enable_map_voxels); needs map.
        map_normals: None, or (step, jump_m) — a surface normal per map entry (vors_tracker_enable_map_normals;
        Trackers.enable_map_normals), switched on after the voxel filter; needs map with level 0; read_map_normals() returns them.
        map_icp: None, a number (dist_m) or a dict of map_icp_params()' keywords — the ICP correction at keyframe promotion
        (vors_tracker_enable_map_icp; Trackers.enable_map_icp), switched on last; needs map_normals; read_map_icp() returns its record.
        map_icp_joint: None, or a dict of map_icp_joint_params()' keywords — the same correction through the joint pass with the condition
        test (vors_tracker_enable_map_icp_joint; Trackers.enable_map_icp_joint), INSTEAD of map_icp; read_map_icp() works unchanged and
        read_map_icp_joint() returns the joint record. map_voxel_stats: True — the statistics of the map's voxels
        (vors_tracker_enable_map_voxel_stats; Trackers.enable_map_voxel_stats), switched on right after the voxel filter; needs map_voxels;
        read_map_voxel_stats() and map_voxel_means() return them. map_icp_means: None, or (min_count[, min_span]) — the averaged map as the
        correction's model (vors_tracker_enable_map_icp_means; Trackers.enable_map_icp_means), switched on last; needs map_voxel_stats
        and one of map_icp / map_icp_joint; read_map_icp_means() returns its record."""
        depth_filter = _depth_filter_args(depth_filter)  # (before anything is created: a bad tuple costs no handle)
        self._map = map = _map_args(map)
        self._map_voxels = map_voxels = _map_voxels_args(map_voxels)
        if map_voxels is not None and map is None:
            raise VorsError("map_voxels: the voxel filter needs the keyframe map (Tracker(..., map=(level, capacity, max_keyframes)))")
        self._map_voxel_stats = bool(map_voxel_stats)
        if self._map_voxel_stats and map_voxels is None:
            raise VorsError("map_voxel_stats: the statistics need the voxel filter (Tracker(..., map_voxels=(voxel_m, table_slots)))")
        self._map_normals = map_normals = _map_normals_args(map_normals)
        if map_normals is not None and map is None:
            raise VorsError("map_normals: the normals need the keyframe map (Tracker(..., map=(0, capacity, max_keyframes)))")
        self._map_icp = map_icp = _map_icp_arg(map_icp)
        if map_icp is not None and map_normals is None:
            raise VorsError("map_icp: the correction needs the map's normals (Tracker(..., map_normals=(step, jump_m)))")
        self._map_icp_joint = map_icp_joint = None if map_icp_joint is None else map_icp_joint_params(**map_icp_joint)
        if map_icp_joint is not None and map_icp is not None:
            raise VorsError("map_icp_joint: the joint stage stands INSTEAD of map_icp: give one of the two")
        if map_icp_joint is not None and map_normals is None:
            raise VorsError("map_icp_joint: the correction needs the map's normals (Tracker(..., map_normals=(step, jump_m)))")
        self._map_icp_means = map_icp_means = _map_icp_means_args(map_icp_means)
        if map_icp_means is not None and not self._map_voxel_stats:
            raise VorsError("map_icp_means: the averaged model needs the voxel statistics (Tracker(..., map_voxel_stats=True))")
        if map_icp_means is not None and map_icp is None and map_icp_joint is None:
            raise VorsError("map_icp_means: the averaged model needs the correction (Tracker(..., map_icp=... or map_icp_joint=...))")
        img = np.ascontiguousarray(img, np.uint8)
        depth_map = np.ascontiguousarray(depth_map, np.uint16)
        rows, cols = img.shape if layout == ROW_MAJOR else img.shape[::-1]
        self.config = config
        self._shape = (rows, cols)
        self._layout = layout
        self._h = C.c_void_p()
        cfg = config.to_c()
        _check(lib().vors_tracker_create(C.byref(cfg), depth_t, _ptr(depth_map), img_t, _ptr(img), rows, cols, layout,
                                         C.byref(self._h)))
        if depth_filter is not None:
            _check(lib().vors_tracker_enable_depth_filter(self._h, *depth_filter))
        if map is not None:
            _check(lib().vors_tracker_enable_map(self._h, *map))
        if map_voxels is not None:
            _check(lib().vors_tracker_enable_map_voxels(self._h, *map_voxels))
        if self._map_voxel_stats:
            _check(lib().vors_tracker_enable_map_voxel_stats(self._h))
        if map_normals is not None:
            _check(lib().vors_tracker_enable_map_normals(self._h, *map_normals))
        if map_icp is not None:
            _check(lib().vors_tracker_enable_map_icp(self._h, C.byref(map_icp)))
        if map_icp_joint is not None:
            _check(lib().vors_tracker_enable_map_icp_joint(self._h, C.byref(map_icp_joint)))
        if map_icp_means is not None:
            _check(lib().vors_tracker_enable_map_icp_means(self._h, *map_icp_means))

    def read_map_icp_means(self):
        """The averaged model's record of the last track() on the host (vors_tracker_read_map_icp_means; synchronises) -> a structured
        scalar of MAP_ICP_MEANS_RECORD_DTYPE: resolved, the window's length, and kept, its ranks that passed."""
        if self._map_icp_means is None:
            raise VorsError("read_map_icp_means: the averaged model is not enabled (Tracker(..., map_icp_means=(min_count, min_span)))")
        rec = np.zeros(1, MAP_ICP_MEANS_RECORD_DTYPE)
        _check(lib().vors_tracker_read_map_icp_means(self._h, _ptr(rec)))
        return rec[0]

    def read_map_icp_joint(self):
        """The joint stage's record of the last track() on the host (vors_tracker_read_map_icp_joint; synchronises) -> a structured scalar
        of MAP_ICP_JOINT_RECORD_DTYPE, beside read_map_icp()'s record."""
        if self._map_icp_joint is None:
            raise VorsError("read_map_icp_joint: the joint correction is not enabled (Tracker(..., map_icp_joint=a dict of parameters))")
        rec = np.zeros(1, MAP_ICP_JOINT_RECORD_DTYPE)
        _check(lib().vors_tracker_read_map_icp_joint(self._h, _ptr(rec)))
        return rec[0]

    def read_map_icp(self):
        """The correction's record of the last track() and its running totals on the host (vors_tracker_read_map_icp; synchronises) ->
        dict: "record", a structured scalar of MAP_ICP_RECORD_DTYPE, and "totals" [2] uint32 (attempted, accepted)."""
        if self._map_icp is None and self._map_icp_joint is None:
            raise VorsError("read_map_icp: the correction is not enabled (Tracker(..., map_icp=dist_m or a dict of parameters))")
        rec, totals = np.zeros(1, MAP_ICP_RECORD_DTYPE), np.zeros(2, np.uint32)
        _check(lib().vors_tracker_read_map_icp(self._h, _ptr(rec), _ptr(totals)))
        return dict(record=rec[0], totals=totals)

    def read_map_normals(self, capacity=None):
        """The map's normals so far on the host (vors_tracker_read_map_normals; synchronises) -> [m, 3] float32, rank for rank the entries
        of read_map(capacity), m = min(count, capacity, the handle's capacity); three zeros where a point has no normal."""
        if self._map_normals is None:
            raise VorsError("read_map_normals: the normals are not enabled (Tracker(..., map_normals=(step, jump_m)))")
        cap = self._map[1] if capacity is None else int(capacity)
        normals = np.zeros((max(cap, 0), 3), np.float32)
        _check(lib().vors_tracker_read_map_normals(self._h, cap, _ptr(normals)))
        return normals[:min(self.read_map(capacity=0)["count"], max(cap, 0), self._map[1])]

    def _voxel_stats_rows(self, who, capacity):
        if not self._map_voxel_stats:
            raise VorsError(f"{who}: the voxel statistics are not enabled (Tracker(..., map_voxel_stats=True))")
        cap = self._map[1] if capacity is None else int(capacity)
        return cap, min(self.read_map(capacity=0)["count"], max(cap, 0), self._map[1])

    def read_map_voxel_stats(self, capacity=None):
        """The voxels' statistics so far on the host (vors_tracker_read_map_voxel_stats; synchronises) -> dict: "sums" [m, 4] int64 and
        "obs" [m, 2] uint32 (count, last segment), rank for rank the entries of read_map(capacity)."""
        cap, m = self._voxel_stats_rows("read_map_voxel_stats", capacity)
        sums, obs = np.zeros((max(cap, 0), 4), np.int64), np.zeros((max(cap, 0), 2), np.uint32)
        _check(lib().vors_tracker_read_map_voxel_stats(self._h, cap, _ptr(sums), _ptr(obs)))
        return dict(sums=sums[:m], obs=obs[:m])

    def map_voxel_means(self, min_count=1, min_span=0, capacity=None):
        """The averaged map on the host (vors_tracker_map_voxel_means; synchronises) -> dict: "xyz_mean" [m, 3] float32 and "gray_mean" [m]
        uint8, rank for rank the entries of read_map(capacity) — NaN and grey 0 where a rank was seen fewer than min_count times or over
        fewer than min_span segments —, and "kept", the passing ranks of the whole list."""
        cap, m = self._voxel_stats_rows("map_voxel_means", capacity)
        xyz, gray, kept = np.zeros((max(cap, 0), 3), np.float32), np.zeros(max(cap, 0), np.uint8), C.c_uint32()
        _check(lib().vors_tracker_map_voxel_means(self._h, _u32("min_count", min_count), _u32("min_span", min_span), cap, _ptr(xyz), _ptr(gray),
                                                  C.byref(kept)))
        return dict(xyz_mean=xyz[:m], gray_mean=gray[:m], kept=kept.value)

    def read_map_voxels(self):
        """The voxel filter's counters (vors_tracker_read_map_voxels; synchronises) -> dict: "occupied", the distinct voxels so far, and
        "overflow", non-zero once they outgrew table_slots."""
        if self._map_voxels is None:
            raise VorsError("read_map_voxels: the voxel filter is not enabled (Tracker(..., map_voxels=(voxel_m, table_slots)))")
        occupied, overflow = C.c_uint32(), C.c_uint32()
        _check(lib().vors_tracker_read_map_voxels(self._h, C.byref(occupied), C.byref(overflow)))
        return dict(occupied=occupied.value, overflow=overflow.value)

    def read_map(self, capacity=None, max_segments=None):
        """The map so far on the host (vors_tracker_read_map; synchronises) -> dict: "count" and "n_segments", the UNCLIPPED totals, "xyz"
        [m, 3] float32, "pixel" [m] uint32 (x | y << 16), "gray" [m] uint8 with m = min(count, capacity, the handle's capacity), and
        "segments" [k] MAP_SEGMENT_DTYPE with k = min(n_segments, max_segments, the handle's max_keyframes). None = the handle's figure."""
        if self._map is None:
            raise VorsError("read_map: the keyframe map is not enabled (Tracker(..., map=(level, capacity, max_keyframes)))")
        cap = self._map[1] if capacity is None else int(capacity)
        nseg = self._map[2] if max_segments is None else int(max_segments)
        xyz, pixel, gray = np.zeros((max(cap, 0), 3), np.float32), np.zeros(max(cap, 0), np.uint32), np.zeros(max(cap, 0), np.uint8)
        seg = np.zeros(max(nseg, 0), MAP_SEGMENT_DTYPE)
        count, n_segments = C.c_uint32(), C.c_uint32()
        _check(lib().vors_tracker_read_map(self._h, cap, _ptr(xyz), _ptr(pixel), _ptr(gray), C.byref(count), nseg, _ptr(seg), C.byref(n_segments)))
        m, k = min(count.value, cap, self._map[1]), min(n_segments.value, nseg, self._map[2])
        return dict(count=count.value, n_segments=n_segments.value, xyz=xyz[:m], pixel=pixel[:m], gray=gray[:m], segments=seg[:k])

    def render_map(self, level=0, pose7=None, range2=None, footprint=1):
        """The map seen from a pose on the host (vors_tracker_render_map; synchronises): Trackers.render_map for the single sequence ->
        dict: "zkey" [rows_l, cols_l] uint64, "depth" uint16, "gray" uint8, "counts" [4] uint32. pose7 None = the current frame's pose;
        range2 None = the whole map, else (first, count) of the ranks to render."""
        if self._map is None:
            raise VorsError("render_map: the keyframe map is not enabled (Tracker(..., map=(level, capacity, max_keyframes)))")
        rows, cols = self._shape[0] >> int(level), self._shape[1] >> int(level)
        pose = None if pose7 is None else np.ascontiguousarray(pose7, np.float32)
        rng = None if range2 is None else np.ascontiguousarray(range2, np.uint32)
        if (pose is not None and pose.shape != (7,)) or (rng is not None and rng.shape != (2,)):
            raise VorsError("render_map: pose7 [7] or None, range2 (first, count) or None")
        shape = (max(rows, 0), max(cols, 0))
        out = dict(zkey=np.empty(shape, np.uint64), depth=np.empty(shape, np.uint16), gray=np.empty(shape, np.uint8),
                   counts=np.zeros(RENDER_COUNTS, np.uint32))
        _check(lib().vors_tracker_render_map(self._h, int(level), _ptr(pose), _ptr(rng), int(footprint), _ptr(out["zkey"]), _ptr(out["depth"]),
                                             _ptr(out["gray"]), _ptr(out["counts"])))
        return out

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            try:
                _lib.vors_tracker_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def track(self, depth_time, depth_map, img_time, img):
        """Tracker::track (inverse_compositional.rs:170-240). Returns the VORS_TRACK_* status (the reference returns ())."""
        img = np.ascontiguousarray(img, np.uint8)
        depth_map = np.ascontiguousarray(depth_map, np.uint16)
        want = self._shape if self._layout == ROW_MAJOR else self._shape[::-1]
        if img.shape != want or depth_map.shape != want:  # the C ABI carries no dimensions after create(): check them here
            raise VorsError(f"Tracker.track: frame shape {img.shape} / depth shape {depth_map.shape} differ from the {want} "
                            "this tracker was created with")
        st = C.c_int()
        rows, cols = img.shape if self._layout == ROW_MAJOR else img.shape[::-1]
        _check(lib().vors_tracker_track_checked(self._h, depth_time, _ptr(depth_map), img_time, _ptr(img), rows, cols, C.byref(st)))
        return st.value

    def current_frame(self):
        """Tracker::current_frame (inverse_compositional.rs:243-248) -> (depth timestamp, pose7)."""
        t = C.c_double()
        p = np.zeros(7, np.float32)
        _check(lib().vors_tracker_current_frame(self._h, C.byref(t), _ptr(p)))
        return t.value, p

    def keyframe(self):
        t = C.c_double()
        p = np.zeros(7, np.float32)
        _check(lib().vors_tracker_keyframe(self._h, C.byref(t), _ptr(p)))
        return t.value, p

    def last_stats(self):
        s = vors_pair_stats()
        _check(lib().vors_tracker_last_stats(self._h, C.byref(s)))
        return np.frombuffer(bytes(s), PAIR_STATS_DTYPE)[0]


def track_pairs(config, kf_gray, kf_depth, cur_gray, prev_poses7=None, layout=ROW_MAJOR, want_stats=True):
    """Host-buffer batch entry (vors_track_pairs): per pair Config::init(keyframe) + Tracker::track(current)."""
    kf_gray = np.ascontiguousarray(kf_gray, np.uint8)
    kf_depth = np.ascontiguousarray(kf_depth, np.uint16)
    cur_gray = np.ascontiguousarray(cur_gray, np.uint8)
    n = kf_gray.shape[0]
    rows, cols = kf_gray.shape[1:] if layout == ROW_MAJOR else kf_gray.shape[1:][::-1]
    poses = np.zeros((n, 7), np.float32)
    status = np.zeros(n, np.int32)
    stats = np.zeros(n, PAIR_STATS_DTYPE) if want_stats else None
    if prev_poses7 is not None:
        prev_poses7 = np.ascontiguousarray(prev_poses7, np.float32)
    cfg = config.to_c()
    _check(lib().vors_track_pairs(C.byref(cfg), n, _ptr(kf_gray), _ptr(kf_depth), _ptr(cur_gray), rows, cols, layout,
                                  _ptr(prev_poses7), _ptr(poses), _ptr(status), _ptr(stats)))
    return poses, status, stats


class MultiGpu:
    """vors_multi_*: ONE process, several devices, pairs sharded by contiguous blocks, one RCCL all-gather of pose + status."""

    def __init__(self, config, max_pairs_per_device, rows, cols, n_devices=0, device_ids=None):
        self.rows, self.cols = rows, cols
        self._h = C.c_void_p()
        cfg = config.to_c()
        ids = np.ascontiguousarray(device_ids, np.int32) if device_ids is not None else None
        self._device_ids = [int(x) for x in device_ids] if device_ids is not None else None
        _check(lib().vors_multi_create(C.byref(cfg), n_devices, _ptr(ids), max_pairs_per_device, rows, cols, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            try:
                _lib.vors_multi_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def device_count(self):
        return lib().vors_multi_device_count(self._h)

    def rccl_version(self):
        """ncclGetVersion of the RCCL bound at run time; 0 for a one-device handle (RCCL is not loaded then)."""
        return lib().vors_multi_rccl_version(self._h)

    def _device_of(self, k):
        return self._device_ids[k] if self._device_ids is not None else k

    def shard(self, n_total, k):
        a, b = C.c_int(), C.c_int()
        _check(lib().vors_multi_shard(self._h, n_total, k, C.byref(a), C.byref(b)))
        return a.value, b.value

    def track_pairs_host(self, kf_gray, kf_depth, cur_gray):
        kf_gray = np.ascontiguousarray(kf_gray, np.uint8)
        kf_depth = np.ascontiguousarray(kf_depth, np.uint16)
        cur_gray = np.ascontiguousarray(cur_gray, np.uint8)
        n = kf_gray.shape[0]
        for name, a in (("kf_gray", kf_gray), ("kf_depth", kf_depth), ("cur_gray", cur_gray)):  # the C ABI reads n * rows * cols of each
            if a.shape != (n, self.rows, self.cols):
                raise VorsError(f"{name}: expected [{n}, {self.rows}, {self.cols}] images, got {a.shape}")
        poses = np.zeros((n, 7), np.float32)
        status = np.zeros(n, np.int32)
        _check(lib().vors_multi_track_pairs_host(self._h, n, _ptr(kf_gray), _ptr(kf_depth), _ptr(cur_gray), _ptr(poses), _ptr(status)))
        return poses, status

    def track_pairs(self, shards_kf_gray, shards_kf_depth, shards_cur_gray, n_total):
        """Device-resident: one torch tensor per device slot (that device's block of pairs)."""
        nd = self.device_count()
        for ts in (shards_kf_gray, shards_kf_depth, shards_cur_gray):
            if len(ts) != nd:
                raise VorsError(f"expected {nd} shards, got {len(ts)}")
            for k, t in enumerate(ts):
                cnt = self.shard(n_total, k)[1]
                if cnt and (t is None or tuple(t.shape) != (cnt, self.rows, self.cols) or not t.is_contiguous() or t.device.index != self._device_of(k)):
                    raise VorsError(f"shard {k}: expected a contiguous [{cnt}, {self.rows}, {self.cols}] tensor on device slot {k}, got "
                                    f"{None if t is None else (tuple(t.shape), t.device)}")
        arr = lambda ts: (C.c_void_p * nd)(*[t.data_ptr() if t is not None and t.numel() else None for t in ts])
        poses = np.zeros((n_total, 7), np.float32)
        status = np.zeros(n_total, np.int32)
        _check(lib().vors_multi_track_pairs(self._h, n_total, arr(shards_kf_gray), arr(shards_kf_depth), arr(shards_cur_gray), _ptr(poses),
                                            _ptr(status)))
        return poses, status


class Batch:
    """Device-resident engine (vors_batch_*). Tensors are torch CUDA(HIP) tensors; work is enqueued on torch's current
    stream and not synchronised."""

    def __init__(self, config, max_pairs, rows, cols, device=None):
        self.config, self.max_pairs, self.rows, self.cols = config, max_pairs, rows, cols
        self._h = C.c_void_p()
        cfg = config.to_c()
        if device is None:
            _check(lib().vors_batch_create(C.byref(cfg), max_pairs, rows, cols, C.byref(self._h)))
        else:
            _check(lib().vors_batch_create_on(int(device), C.byref(cfg), max_pairs, rows, cols, C.byref(self._h)))

    def device(self):
        d = C.c_int()
        _check(lib().vors_batch_device(self._h, C.byref(d)))
        return d.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            try:
                _lib.vors_batch_destroy(self._h)
            except Exception:
                pass
            self._h = None

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _dp(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def workspace_bytes(self):
        b = C.c_uint64()
        _check(lib().vors_batch_workspace_bytes(self._h, C.byref(b)))
        return b.value

    def enable_kernel_timing(self, ring=64):
        _check(lib().vors_batch_enable_kernel_timing(self._h, int(ring)))

    STAGES = {"pyramid_keyframe": 0, "keyframe": 1, "pyramid_current": 2, "lm": 3}

    def kernel_times(self, stage):
        """Durations (ms) of the last min(steps, ring) steps of a stage, oldest first (HIP events on the stream)."""
        out = np.zeros(4096, np.float32)
        n = C.c_int()
        _check(lib().vors_batch_kernel_times(self._h, self.STAGES[stage], _ptr(out), 4096, C.byref(n)))
        return out[:n.value].copy()

    def last_kernel_ms(self):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        _check(lib().vors_batch_last_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(lm_ms=a.value, keyframe_ms=b.value, pyramid_ms=c.value)

    def _check_images(self, *tensors):
        for t in tensors:
            if t is None:
                continue
            if tuple(t.shape[-2:]) != (self.rows, self.cols) or not t.is_contiguous() or t.shape[0] > self.max_pairs:
                raise VorsError(f"expected contiguous [n <= {self.max_pairs}, {self.rows}, {self.cols}] images, got {tuple(t.shape)}")

    def prepare_keyframes(self, kf_gray, kf_depth):
        n = kf_gray.shape[0]
        self._check_images(kf_gray, kf_depth)
        # lifetime contract of vors_batch_prepare_keyframes: the handle keeps POINTERS to level 0 and the depth map (zero copy);
        # hold the tensors so that torch's caching allocator cannot hand their memory to someone else while the handle uses them
        self._kf_refs = (kf_gray, kf_depth)
        _check(lib().vors_batch_prepare_keyframes(self._h, n, self._dp(kf_gray), self._dp(kf_depth), self._stream()))

    def track_current(self, cur_gray, out_poses7, out_status, out_stats=None, prev_poses7=None):
        n = cur_gray.shape[0]
        self._check_images(cur_gray)
        self._cur_ref = cur_gray
        _check(lib().vors_batch_track_current(self._h, n, self._dp(cur_gray), self._dp(prev_poses7), self._dp(out_poses7),
                                              self._dp(out_status), self._dp(out_stats), self._stream()))

    def track_pairs(self, kf_gray, kf_depth, cur_gray, out_poses7, out_status, out_stats=None, prev_poses7=None):
        n = kf_gray.shape[0]
        self._check_images(kf_gray, kf_depth, cur_gray)
        self._kf_refs, self._cur_ref = (kf_gray, kf_depth), cur_gray
        _check(lib().vors_batch_track_pairs(self._h, n, self._dp(kf_gray), self._dp(kf_depth), self._dp(cur_gray),
                                            self._dp(prev_poses7), self._dp(out_poses7), self._dp(out_status),
                                            self._dp(out_stats), self._stream()))

    def lm_predict_log(self, n_pairs):
        """What the go-on prediction of the dense FUSED rounds did with each pair in the last track -> int32[n_pairs] of PREDICT_* bits."""
        out = np.zeros(n_pairs, np.int32)
        _check(lib().vors_batch_lm_predict_log(self._h, n_pairs, _ptr(out)))
        return out

    def eval_level(self, pair, level, model7, arithmetic):
        """One evaluation of a level of a pair at `model7` in the given arithmetic -> (sum r^2, n_inside, g[6], H[6,6])."""
        m = np.ascontiguousarray(model7, np.float32)
        out = np.zeros(29, np.float32)
        _check(lib().vors_batch_eval_level(self._h, pair, level, _ptr(m), int(arithmetic), _ptr(out)))
        H = np.zeros((6, 6), np.float32)
        H[np.triu_indices(6)] = out[8:29]
        H = H + np.triu(H, 1).T
        return float(out[0]), int(out[1]), out[2:8].copy(), H

    @staticmethod
    def _models_arg(models):
        """models [n, 7] / [n, K, 7] float32, or the out_stats bytes of a track (its row size tells) -> (tensor, n, K, stride in bytes)."""
        import torch
        if not models.is_contiguous():
            raise VorsError("models must be a contiguous tensor")
        if models.dtype == torch.uint8:
            if models.numel() % PAIR_STATS_DTYPE.itemsize != 0:
                raise VorsError("a uint8 `models` tensor must be the out_stats buffer of a track")
            return models, models.numel() // PAIR_STATS_DTYPE.itemsize, 1, PAIR_STATS_DTYPE.itemsize
        if models.dtype != torch.float32 or models.shape[-1] != 7 or models.dim() not in (2, 3):
            raise VorsError(f"expected float32 models [n, 7] or [n, K, 7], got {models.dtype} {tuple(models.shape)}")
        return models, models.shape[0], (models.shape[1] if models.dim() == 3 else 1), 0

    @staticmethod
    def _one_per_pair(models, refusal):
        """_models_arg for the products that take ONE model (pose) per pair -> (tensor, n, stride in bytes)."""
        models, n, k, stride = Batch._models_arg(models)
        if k != 1:
            raise VorsError(refusal)
        return models, n, stride

    EVAL_WHAT = {"full": 0, "energy": 1}

    def eval_pairs(self, level, models, arithmetic=None, what="full", out=None):
        """One evaluation of `level` per (pair, model) on the device (vors_batch_eval_pairs) -> sums [n, K, 29] on the current stream,
        not synchronised. `models`: [n, 7], [n, K, 7], or the out_stats tensor of a track (evaluates at each pair's lm_model)."""
        import torch
        models, n, k, stride = self._models_arg(models)
        if out is None:
            out = torch.empty((n, k, 29), dtype=torch.float32, device=models.device)
        elif out.dtype != torch.float32 or out.numel() != n * k * 29 or not out.is_contiguous():
            raise VorsError(f"out must be a contiguous float32 tensor of {n} x {k} x 29 elements")
        arith = self.config.arithmetic if arithmetic is None else arithmetic
        if what not in self.EVAL_WHAT:
            raise VorsError(f"eval_pairs: unknown `what` {what!r} (one of {', '.join(map(repr, self.EVAL_WHAT))})")
        _check(lib().vors_batch_eval_pairs(self._h, n, int(level), k, self._dp(models), stride, int(arith), self.EVAL_WHAT[what],
                                           self._dp(out), self._stream()))
        return out.view(n, k, 29)

    def pose_information(self, level, models):
        """Information matrix, covariance of the twist, residual variance and flags of every pair at `models` ([n, 7] or a track's out_stats)
        in the handle's arithmetic (vors_batch_pose_information) -> (info [n, 6, 6], cov [n, 6, 6], sigma2 [n], flags [n]), not synchronised."""
        import torch
        models, n, stride = self._one_per_pair(models, "pose_information takes one model per pair")
        info = torch.empty((n, 6, 6), dtype=torch.float32, device=models.device)
        cov = torch.empty((n, 6, 6), dtype=torch.float32, device=models.device)
        sigma2 = torch.empty(n, dtype=torch.float32, device=models.device)
        flags = torch.empty(n, dtype=torch.int32, device=models.device)
        _check(lib().vors_batch_pose_information(self._h, n, int(level), self._dp(models), stride, self._dp(info), self._dp(cov),
                                                 self._dp(sigma2), self._dp(flags), self._stream()))
        return info, cov, sigma2, flags

    def residual_maps(self, level, models, residuals=True, warp=False, hist=False, scale=False):
        """The per-point quantities of one evaluation of `level` per pair at `models` ([n, 7] or a track's out_stats), in the reference's
        per-point arithmetic whatever the handle's (vors_batch_residual_maps) -> dict of the requested tensors on the current stream, not
        synchronised: "residuals" [n, rows_l, cols_l] (raw residual, NaN where the point is not inside), "warp" [n, rows_l, cols_l, 2]
        ((u, v) of every usable candidate, NaN elsewhere), "hist" [n, 256] (int32 view of the counts of min(int(|r|), 255)), "scale" [n, 2]
        (median |r|, 1.4826 median |r|; computed from the histogram, which is made for it when `hist` is not asked for)."""
        import torch
        models, n, stride = self._one_per_pair(models, "residual_maps takes one model per pair")
        if not (residuals or warp or hist or scale):
            raise VorsError("residual_maps: nothing requested")
        rows, cols = self.rows >> int(level), self.cols >> int(level)
        dev = models.device
        t_res = torch.empty((n, rows, cols), dtype=torch.float32, device=dev) if residuals else None
        t_uv = torch.empty((n, rows, cols, 2), dtype=torch.float32, device=dev) if warp else None
        t_hist = torch.empty((n, RESIDUAL_BINS), dtype=torch.int32, device=dev) if (hist or scale) else None
        t_scale = torch.empty((n, 2), dtype=torch.float32, device=dev) if scale else None
        _check(lib().vors_batch_residual_maps(self._h, n, int(level), self._dp(models), stride, self._dp(t_res), self._dp(t_uv), self._dp(t_hist),
                                              self._dp(t_scale), self._stream()))
        return _result(("residuals", residuals, t_res), ("warp", warp, t_uv), ("hist", hist, t_hist), ("scale", scale, t_scale))

    def reproject_depth(self, level, models, cur_depth=None, tol_m=0.0, pred_z=True, pred_depth=False, residual=False, counts=False):
        """The keyframe's depth carried into the current frame at `models` ([n, 7] or a track's out_stats) with a z-buffer, and compared with
        the measured current depth maps `cur_depth` ([n, rows, cols] int16 tensor holding the u16 payload, level 0 only)
        (vors_batch_reproject_depth; needs prepare_keyframes only) -> dict of the requested tensors on the current stream, not synchronised:
        "pred_z" [n, rows_l, cols_l] (current frame: nearest Z' in metres, +inf where no point lands), "pred_depth" [n, rows_l, cols_l]
        (int16 tensor holding the u16 to_depth of pred_z, 0 where nothing lands; pred_z is made for it when not asked for), "residual"
        [n, rows, cols] (keyframe geometry: Z' - cur_depth / depth_scale, NaN elsewhere), "counts" [n, 4] (int32: usable points, points
        that land, those with a current depth, those with |residual| <= tol_m)."""
        import torch
        models, n, stride = self._one_per_pair(models, "reproject_depth takes one model per pair")
        if not (pred_z or pred_depth or residual or counts):
            raise VorsError("reproject_depth: nothing requested")
        if cur_depth is not None and (cur_depth.dtype != torch.int16 or not cur_depth.is_contiguous() or
                                      tuple(cur_depth.shape) != (n, self.rows, self.cols)):
            raise VorsError(f"expected a contiguous int16 cur_depth [{n}, {self.rows}, {self.cols}], got {cur_depth.dtype} {tuple(cur_depth.shape)}")
        rows, cols = self.rows >> int(level), self.cols >> int(level)
        dev = models.device
        t_z = torch.empty((n, rows, cols), dtype=torch.float32, device=dev) if (pred_z or pred_depth) else None
        t_d = torch.empty((n, rows, cols), dtype=torch.int16, device=dev) if pred_depth else None
        t_res = torch.empty((n, rows, cols), dtype=torch.float32, device=dev) if residual else None
        t_cnt = torch.empty((n, 4), dtype=torch.int32, device=dev) if counts else None
        _check(lib().vors_batch_reproject_depth(self._h, n, int(level), self._dp(models), stride, self._dp(cur_depth), float(tol_m), self._dp(t_z),
                                                self._dp(t_d), self._dp(t_res), self._dp(t_cnt), self._stream()))
        return _result(("pred_z", pred_z, t_z), ("pred_depth", pred_depth, t_d), ("residual", residual, t_res), ("counts", counts, t_cnt))

    def point_cloud(self, level, poses=None, keep=None, capacity=None, xyz=True, pixel=True, gray=False, counts=True, n_pairs=None):
        """The usable points of `level` of every pair as lists in the world frame (vors_batch_point_cloud; needs prepare_keyframes only) ->
        dict of the requested tensors on the current stream, not synchronised: "xyz" [n, capacity, 3] (poses * back_project of each point;
        `poses` [n, 7] float32 or a track's out_stats, camera -> world, None = identity), "pixel" [n, capacity] (int32: x | y << 16), "gray"
        [n, capacity] (uint8), "counts" [n] (int32: the total per pair, which may exceed capacity). Only the first min(count, capacity)
        entries of a list are written. `keep` [n, rows_l, cols_l] uint8: non-zero keeps the pixel's point. capacity None = rows_l * cols_l.
        xyz / pixel / gray / counts may also be a tensor of that shape to write into (its other entries stay as they are). n is `n_pairs`,
        else the rows of poses, else of keep, else the pairs of the last prepare_keyframes."""
        import torch
        lvl = int(level)
        rows, cols = self.rows >> lvl, self.cols >> lvl
        stride = 0
        if poses is not None:
            poses, n, stride = self._one_per_pair(poses, "point_cloud takes one pose per pair")
        elif keep is not None:
            n = keep.shape[0]
        else:
            refs = getattr(self, "_kf_refs", None)
            if refs is None:
                raise VorsError("point_cloud needs prepare_keyframes first")
            n = refs[0].shape[0]
        if n_pairs is not None:
            if int(n_pairs) > n:
                raise VorsError(f"point_cloud: n_pairs {n_pairs} exceeds the {n} poses / masks given")
            n = int(n_pairs)
        if keep is not None and (keep.dtype != torch.uint8 or not keep.is_contiguous() or keep.shape[0] < n or tuple(keep.shape[1:]) != (rows, cols)):
            raise VorsError(f"expected a contiguous uint8 keep [{n}, {rows}, {cols}], got {keep.dtype} {tuple(keep.shape)}")
        cap = rows * cols if capacity is None else int(capacity)
        if not any(_asked(o) for o in (xyz, pixel, gray, counts)):
            raise VorsError("point_cloud: nothing requested")
        refs = getattr(self, "_kf_refs", None)
        dev = poses.device if poses is not None else keep.device if keep is not None else refs[0].device if refs else torch.device("cuda")

        t_xyz = _out_buf(xyz, (n, cap, 3), torch.float32, dev)
        t_pix = _out_buf(pixel, (n, cap), torch.int32, dev)
        t_gray = _out_buf(gray, (n, cap), torch.uint8, dev)
        t_cnt = _out_buf(counts, (n,), torch.int32, dev)
        _check(lib().vors_batch_point_cloud(self._h, n, lvl, self._dp(poses), stride, self._dp(keep), cap, self._dp(t_xyz), self._dp(t_pix),
                                            self._dp(t_gray), self._dp(t_cnt), self._stream()))
        return _result(("xyz", _asked(xyz), t_xyz), ("pixel", _asked(pixel), t_pix), ("gray", _asked(gray), t_gray), ("counts", _asked(counts), t_cnt))

    def fuse_depth(self, models, cur_depth, tol_m, kf_weight=None, max_weight=255, fill_min_weight=0, depth=True, weight=True, zkey=False,
                   counts=False):
        """The keyframe's depth carried into the current frame at `models` ([n, 7] or a track's out_stats) through a keyed z-buffer and merged
        with the measured current depth maps `cur_depth` ([n, rows, cols] int16 tensor holding the u16 payload) (vors_batch_fuse_depth; level
        0, needs prepare_keyframes only) -> dict of the requested tensors on the current stream, not synchronised: "depth" [n, rows, cols]
        (int16 tensor holding the u16 fused depth, the next prepare_keyframes' depth), "weight" [n, rows, cols] (uint8, the next call's
        `kf_weight`), "zkey" [n, rows, cols] (int64 tensor holding the u64 payload bits(Z') << 32 | source pixel, -1 = nothing landed),
        "counts" [n, 6] (int32: agree, prediction in front, prediction behind, measured only, filled, empty). `kf_weight` [n, rows, cols]
        uint8 in keyframe geometry: None = 1 everywhere, 0 removes the point. The key plane is made when it is not asked for."""
        import torch
        models, n, stride = self._one_per_pair(models, "fuse_depth takes one model per pair")
        shape = (n, self.rows, self.cols)
        if cur_depth is None or cur_depth.dtype != torch.int16 or not cur_depth.is_contiguous() or tuple(cur_depth.shape) != shape:
            raise VorsError(f"expected a contiguous int16 cur_depth {list(shape)}")
        if kf_weight is not None and (kf_weight.dtype != torch.uint8 or not kf_weight.is_contiguous() or tuple(kf_weight.shape) != shape):
            raise VorsError(f"expected a contiguous uint8 kf_weight {list(shape)}, got {kf_weight.dtype} {tuple(kf_weight.shape)}")
        if not (depth or weight or zkey or counts):
            raise VorsError("fuse_depth: nothing requested")
        dev = models.device
        t_key = torch.empty(shape, dtype=torch.int64, device=dev)
        t_d = torch.empty(shape, dtype=torch.int16, device=dev) if depth else None
        t_w = torch.empty(shape, dtype=torch.uint8, device=dev) if weight else None
        t_cnt = torch.empty((n, 6), dtype=torch.int32, device=dev) if counts else None
        _check(lib().vors_batch_fuse_depth(self._h, n, self._dp(models), stride, self._dp(cur_depth), float(tol_m), self._dp(kf_weight),
                                           int(max_weight), int(fill_min_weight), self._dp(t_key), self._dp(t_d), self._dp(t_w),
                                           self._dp(t_cnt), self._stream()))
        return _result(("depth", depth, t_d), ("weight", weight, t_w), ("zkey", zkey, t_key), ("counts", counts, t_cnt))

    def keyframe_image(self, pair, level):
        out = np.empty(self.rows * self.cols, np.uint8)
        r, c = C.c_int(), C.c_int()
        _check(lib().vors_batch_get_keyframe_image(self._h, pair, level, _ptr(out), C.byref(r), C.byref(c)))
        return out[:r.value * c.value].reshape(r.value, c.value).copy()

    def current_image(self, pair, level):
        out = np.empty(self.rows * self.cols, np.uint8)
        r, c = C.c_int(), C.c_int()
        _check(lib().vors_batch_get_current_image(self._h, pair, level, _ptr(out), C.byref(r), C.byref(c)))
        return out[:r.value * c.value].reshape(r.value, c.value).copy()

    def points(self, pair, level):
        """Usable candidates of a level in device slot order: xy[n,2], idepth[n], jac[n,6], tmpl[n]."""
        cap = (self.rows >> level) * (self.cols >> level)
        xy = np.empty((cap, 2), np.int32)
        iz = np.empty(cap, np.float32)
        jac = np.empty((cap, 6), np.float32)
        tm = np.empty(cap, np.uint8)
        n = C.c_int()
        _check(lib().vors_batch_get_points(self._h, pair, level, cap, _ptr(xy), _ptr(iz), _ptr(jac), _ptr(tm), C.byref(n)))
        n = n.value
        return xy[:n].copy(), iz[:n].copy(), jac[:n].copy(), tm[:n].copy()


class Pipeline:
    """vors_pipeline_*: a ring of `depth` batch handles on internal streams for a continuous feed of independent batches (throughput mode).
    submit() orders the step after everything on torch's current stream and returns a ticket; wait() / drain() order torch's current
    stream after the step(s) (host=True: block the calling thread instead). Results are those of Batch.track_pairs bit for bit."""

    def __init__(self, config, max_pairs, rows, cols, depth=2, device=None):
        self.config, self.max_pairs, self.rows, self.cols, self.depth = config, max_pairs, rows, cols, depth
        self._h = C.c_void_p()
        self._refs = {}
        cfg = config.to_c()
        _check(lib().vors_pipeline_create(-1 if device is None else int(device), C.byref(cfg), int(depth), max_pairs, rows, cols,
                                          C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            try:
                _lib.vors_pipeline_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def submit(self, kf_gray, kf_depth, cur_gray, out_poses7, out_status, out_stats=None, prev_poses7=None):
        n = kf_gray.shape[0]
        for t in (kf_gray, kf_depth, cur_gray):
            if tuple(t.shape) != (n, self.rows, self.cols) or not t.is_contiguous() or n > self.max_pairs:
                raise VorsError(f"expected contiguous [n <= {self.max_pairs}, {self.rows}, {self.cols}] images, got {tuple(t.shape)}")
        ticket = C.c_int64(-1)
        st = lib().vors_pipeline_submit(self._h, n, Batch._dp(kf_gray), Batch._dp(kf_depth), Batch._dp(cur_gray), Batch._dp(prev_poses7),
                                        Batch._dp(out_poses7), Batch._dp(out_status), Batch._dp(out_stats), Batch._stream(), C.byref(ticket))
        # the step reads and writes these buffers until it completes: keep them alive for as long as its slot can be running it. A call
        # that failed before it was given a ticket touches no slot's references (ticket -1 would otherwise evict those of slot depth - 1
        # while that slot's step may still be running); its buffers are kept aside instead.
        refs = (kf_gray, kf_depth, cur_gray, out_poses7, out_status, out_stats, prev_poses7)
        if ticket.value >= 0:
            self._refs[ticket.value % self.depth] = refs
        else:
            self._refs.setdefault("failed", []).append(refs)
        _check(st)
        return ticket.value

    def wait(self, ticket, host=False):
        _check(lib().vors_pipeline_wait(self._h, int(ticket), Batch._stream(), 1 if host else 0))

    def drain(self, host=False):
        _check(lib().vors_pipeline_drain(self._h, Batch._stream(), 1 if host else 0))


class Trackers:
    """N sequences in lock-step, device resident (vors_trackers_*): Config::init / Tracker::track / current_frame for every
    sequence with the whole tracker state machine (poses, keyframe test, per-sequence keyframe promotion) on the device."""

    _map = None  # enable_map()'s arguments, once it was accepted
    _map_normals = None  # enable_map_normals()'s, likewise

    def __init__(self, config, n_sequences, rows, cols, device=None):
        self.config, self.n, self.rows, self.cols = config, n_sequences, rows, cols
        self._device = None if device is None else int(device)
        self._h = C.c_void_p()
        cfg = config.to_c()
        if device is None:
            _check(lib().vors_trackers_create(C.byref(cfg), n_sequences, rows, cols, C.byref(self._h)))
        else:
            _check(lib().vors_trackers_create_on(int(device), C.byref(cfg), n_sequences, rows, cols, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            try:
                _lib.vors_trackers_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def _check_frames(self, gray, depth):
        for t in (gray, depth):
            if tuple(t.shape) != (self.n, self.rows, self.cols) or not t.is_contiguous():
                raise VorsError(f"expected contiguous [{self.n}, {self.rows}, {self.cols}] frames, got {tuple(t.shape)}")

    def init(self, gray, depth):
        """Config::init for every sequence (frame 0). Only enqueues work on torch's current stream: the frames must stay alive (and unmodified)
        until that work has run — this object keeps a reference until the next call, like track()."""
        self._check_frames(gray, depth)
        self._last = (gray, depth)
        _check(lib().vors_trackers_init(self._h, Batch._dp(gray), Batch._dp(depth), Batch._stream()))

    def track(self, gray, depth):
        """Tracker::track for every sequence (one new frame each); only enqueues work on torch's current stream."""
        self._check_frames(gray, depth)
        self._last = (gray, depth)  # keep the frames alive until the next call (the enqueued work reads them)
        _check(lib().vors_trackers_track(self._h, Batch._dp(gray), Batch._dp(depth), Batch._stream()))

    def current_frames(self):
        """-> (poses7 [n,7], status [n], keyframe frame index [n]) on the host; synchronises the current stream."""
        poses = np.zeros((self.n, 7), np.float32)
        status = np.zeros(self.n, np.int32)
        kf = np.zeros(self.n, np.int32)
        _check(lib().vors_trackers_current_frames(self._h, _ptr(poses), _ptr(status), _ptr(kf), Batch._stream()))
        return poses, status, kf

    def stats(self):
        """Diagnostics of the last track() of every sequence (host copy; synchronises the current stream)."""
        out = np.zeros(self.n, PAIR_STATS_DTYPE)
        _check(lib().vors_trackers_last_stats(self._h, _ptr(out), Batch._stream()))
        return out

    def enable_depth_filter(self, tol_m, max_weight=255, fill_min_weight=0):
        """Recursive depth filter across keyframe promotions (vors_trackers_enable_depth_filter): before init(), once. A promoted frame's
        keyframe is then built on the depth FUSED from the old keyframe and the measurement (Batch.fuse_depth's rule), on the device."""
        _check(lib().vors_trackers_enable_depth_filter(self._h, *_depth_filter_args((tol_m, max_weight, fill_min_weight))))

    def keyframe_depth(self, copy=True):
        """-> (depth [n, rows, cols] int16 tensor holding the u16 payload, weight [n, rows, cols] uint8) of every sequence's current keyframe
        (vors_trackers_keyframe_depth), valid in stream order after the last init() / track(). copy=False: views of the handle's own
        planes, which the next track() rewrites and which die with this object."""
        plane = (self.rows, self.cols)
        return tuple(self._views(lib().vors_trackers_keyframe_depth, copy, depth=(plane, "<i2"), weight=(plane, "|u1")).values())

    def _views(self, entry, copy, **specs):
        """What the getters share. entry(handle, a pointer out per item of specs) -> dict of tensors over the handle's own buffers, cloned
        when copy. specs: key=(the shape behind [n], typestr), in the order of the entry's pointers."""
        p = [C.c_void_p() for _ in specs]
        _check(entry(self._h, *[C.byref(q) for q in p]))
        dev = _torch_device(self._device)
        out = {key: _device_view(q.value, (self.n,) + tuple(shape), typestr, dev) for q, (key, (shape, typestr)) in zip(p, specs.items())}
        return {key: t.clone() for key, t in out.items()} if copy else out

    def workspace_bytes(self):
        b = C.c_uint64()
        _check(lib().vors_trackers_workspace_bytes(self._h, C.byref(b)))
        return b.value

    def enable_map(self, level, capacity, max_keyframes, min_weight=0):
        """Keyframe map (vors_trackers_enable_map): before init(), once. From then on the cloud of every new keyframe of a sequence — the
        usable points of `level` through the keyframe pose, Batch.point_cloud's rule — is appended on the device to that sequence's list,
        with a segment record per keyframe. min_weight >= 2 keeps the points whose depth-filter weight reaches it (level 0, filter first)."""
        args = _map_args((level, capacity, max_keyframes, min_weight))
        _check(lib().vors_trackers_enable_map(self._h, *args))
        self._map = args

    def map(self, copy=True):
        """-> dict of tensors (vors_trackers_map), valid in stream order after the last init() / track(): "xyz" [n, capacity, 3] float32,
        "pixel" [n, capacity] int32 (x | y << 16), "gray" [n, capacity] uint8, "counts" [n] int32 (the u32 running totals, which may exceed
        capacity), "n_segments" [n] int32, "segments" [n, max_keyframes, 40] uint8 — the vors_map_segment records as bytes:
        decode_map_segments() gives the structured view. Only the first min(counts, capacity) entries of a list and the first
        min(n_segments, max_keyframes) records are written. copy=False: views of the handle's own buffers, which die with this object."""
        _, cap, nkf, _ = self._map or (0, 0, 0, 0)  # (no map: the entry refuses)
        return self._views(lib().vors_trackers_map, copy, xyz=((cap, 3), "<f4"), pixel=((cap,), "<i4"), gray=((cap,), "|u1"), counts=((), "<i4"),
                           segments=((nkf, 40), "|u1"), n_segments=((), "<i4"))

    def enable_map_voxels(self, voxel_m, table_slots):
        """Voxel filter of the keyframe map (vors_trackers_enable_map_voxels): after enable_map(), before init(), once. The map then keeps
        one point per occupied voxel of a world grid of edge voxel_m — the first in the map's own order — through a table of table_slots
        entries per sequence (a power of two in 64..2^30; 16 bytes each)."""
        args = _map_voxels_args((voxel_m, table_slots))
        _check(lib().vors_trackers_enable_map_voxels(self._h, *args))

    def enable_map_voxel_stats(self):
        """Statistics of the map's voxels (vors_trackers_enable_map_voxel_stats): after enable_map_voxels(), before init(), once. Every
        rank of the filtered list then carries fixed-point sums of all observations of its voxel, the sum of their greys, their number and
        the last segment that saw it, beside the lists, which keep their bits: map_voxel_stats(), map_voxel_means()."""
        _check(lib().vors_trackers_enable_map_voxel_stats(self._h))

    def map_voxel_stats(self, copy=True):
        """-> dict of tensors (vors_trackers_map_voxel_stats), valid in stream order after the last init() / track(): "sums" [n, capacity,
        4] int64 (offsets x, y, z from the rank's stored point in units of voxel_m / 2^20, and grey) and "obs" [n, capacity, 2] int32
        (the u32 count and last segment), rank for rank with map(). copy=False: views of the handle's own buffers, which die with this
        object."""
        cap = self._map[1] if self._map else 0  # (no map: the entry refuses)
        return self._views(lib().vors_trackers_map_voxel_stats, copy, sums=((cap, 4), "<i8"), obs=((cap, 2), "<i4"))

    def map_voxel_means(self, min_count=1, min_span=0, xyz_mean=True, gray_mean=True, kept=True):
        """The averaged map (vors_trackers_map_voxel_means): voxel_means() on the handle's own lists and statistics, the span taken from
        its segments, on the current stream, not synchronised. The result as in voxel_means()."""
        import torch
        cap = self._map[1] if self._map else 1  # (no map: the entry refuses)
        dev = _torch_device(self._device)
        bufs = (_out_buf(xyz_mean, (self.n, cap, 3), torch.float32, dev), _out_buf(gray_mean, (self.n, cap), torch.uint8, dev),
                _out_buf(kept, (self.n,), torch.int32, dev))
        _check(lib().vors_trackers_map_voxel_means(self._h, _u32("min_count", min_count), _u32("min_span", min_span),
                                                   *[Batch._dp(t) for t in bufs], Batch._stream()))
        return _voxel_means_result(bufs, xyz_mean, gray_mean, kept)

    def enable_map_normals(self, step, jump_m):
        """Normals of the keyframe map (vors_trackers_enable_map_normals): after enable_map() with level 0, before init(), once. Every map
        entry then carries the surface normal of its pixel in its keyframe's depth plane, in the world frame (points_normals' rule with the
        keyframe's pose): central differences `step` pixels wide, neighbours further than jump_m metres in depth left out."""
        args = _map_normals_args((step, jump_m))
        _check(lib().vors_trackers_enable_map_normals(self._h, *args))
        self._map_normals = args

    def map_normals(self, copy=True):
        """-> [n, capacity, 3] float32 tensor (vors_trackers_map_normals), valid in stream order after the last init() / track(): entry r
        of a sequence is the normal of map()'s entry r, written for r < min(counts, capacity); three zeros = no normal. copy=False: a view
        of the handle's own buffer, which dies with this object."""
        cap = self._map[1] if self._map else 0  # (no map: the entry refuses)
        return self._views(lib().vors_trackers_map_normals, copy, normals=((cap, 3), "<f4"))["normals"]

    def enable_map_icp(self, **params):
        """ICP correction at keyframe promotion (vors_trackers_enable_map_icp): after enable_map_normals(), before init(), once. Every
        promoted sequence's existing map is then aligned to the new keyframe's depth (icp_points_robust's pass from the keyframe pose the
        LM stage produced) before the keyframe's cloud is emitted; a result that passes the verdict replaces the sequence's poses.
        params: map_icp_params()' keywords — dist_m required, the rest MAP_ICP_DEFAULTS."""
        p = map_icp_params(**params)
        _check(lib().vors_trackers_enable_map_icp(self._h, C.byref(p)))

    def enable_map_icp_joint(self, **params):
        """The correction of enable_map_icp() through the joint pass and with the condition test (vors_trackers_enable_map_icp_joint):
        INSTEAD of enable_map_icp(), legal where it is. The pass is icp_points_joint()'s (list grey = the map's, frame grey = the promoted
        frame's level 0); behind ACCEPTED the verdict returns MAP_ICP_CONDITION when a dilution (icp_condition() of the pass's final sums)
        exceeds its bound. params: map_icp_joint_params()' keywords — dist_m required, the rest MAP_ICP_DEFAULTS and MAP_ICP_JOINT_DEFAULTS."""
        p = map_icp_joint_params(**params)
        _check(lib().vors_trackers_enable_map_icp_joint(self._h, C.byref(p)))

    def map_icp_joint(self, copy=True):
        """-> [n, 20] uint8 tensor (vors_trackers_map_icp_joint), valid in stream order after the last track(): the
        vors_map_icp_joint_record of every sequence beside map_icp()'s records, as bytes: decode_map_icp_joint_records(). copy=False: a view
        of the handle's own buffer, which dies with this object."""
        return self._views(lib().vors_trackers_map_icp_joint, copy, records=((MAP_ICP_JOINT_RECORD_DTYPE.itemsize,), "|u1"))["records"]

    def enable_map_icp_means(self, min_count=1, min_span=0):
        """The averaged map as the correction's model (vors_trackers_enable_map_icp_means): after enable_map_voxel_stats() and one of
        enable_map_icp() / enable_map_icp_joint(), before init(), once. Every track() then resolves the window of each promoted sequence
        (map_voxel_means()' rule with min_count, min_span, on the statistics as they stood before the promotion's emission) into staging
        of the handle, and the correction's pass reads centroids and mean grey in the lists' place; rejected ranks are NaN rows the pass
        skips and still count as `considered`."""
        _check(lib().vors_trackers_enable_map_icp_means(self._h, _u32("min_count", min_count), _u32("min_span", min_span)))

    def map_icp_means(self, copy=True):
        """-> dict (vors_trackers_map_icp_means), valid in stream order after the last track(): "xyz_mean" [n, capacity, 3] float32 and
        "gray_mean" [n, capacity] uint8 tensors — the staging: per sequence what its windows have written since init(), zero bytes
        elsewhere — and "records", a structured numpy array [n] of MAP_ICP_MEANS_RECORD_DTYPE for the LAST track call (decoded:
        synchronises). copy=False: the tensors are views of the handle's own buffers, which die with this object."""
        cap = self._map[1] if self._map else 0  # (no map: the entry refuses)
        out = self._views(lib().vors_trackers_map_icp_means, copy, xyz_mean=((cap, 3), "<f4"), gray_mean=((cap,), "|u1"),
                          records=((MAP_ICP_MEANS_RECORD_DTYPE.itemsize,), "|u1"))
        out["records"] = decode_map_icp_means_records(out["records"])
        return out

    def map_icp(self, copy=True):
        """-> dict of tensors (vors_trackers_map_icp), valid in stream order after the last track(): "records" [n, 112] uint8 — the
        vors_map_icp_record of every sequence for the LAST track call as bytes: decode_map_icp_records() — and "totals" [n, 2] int32,
        promotions attempted and accepted since init(). copy=False: views of the handle's own buffers, which die with this object."""
        return self._views(lib().vors_trackers_map_icp, copy, records=((MAP_ICP_RECORD_DTYPE.itemsize,), "|u1"), totals=((2,), "<i4"))

    def map_voxels(self, copy=True):
        """-> dict of tensors (vors_trackers_map_voxels), valid in stream order after the last init() / track(): "occupied" [n] int32, the
        distinct voxels of a sequence so far (== map()["counts"] while it has not overflowed), "overflow" [n] int32, non-zero once a
        sequence's voxels outgrew table_slots. copy=False: views of the handle's own buffers, which die with this object."""
        return self._views(lib().vors_trackers_map_voxels, copy, occupied=((), "<i4"), overflow=((), "<i4"))

    def repose_map(self, poses, node_counts, node_of_segment=None, xyz_out=True, normals_out=None, segments_out=True, counts=True):
        """The keyframe map re-posed after pose-graph optimisation (vors_trackers_repose_map): repose_points() on the handle's own lists,
        normals (with enable_map_normals()), counters and segments, written into NEW tensors (or the caller's), on the current stream, not
        synchronised. The handle is only read: its map stays as tracking left it. poses [n, node_capacity, >= 7] float32, node_counts [n]
        int32, node_of_segment [n, max_keyframes] int32 or None (segment k is node k). normals_out None = True exactly when the map has
        normals. The result as in repose_points(); a new tensor starts as a copy of the handle's."""
        import torch
        who = "repose_map"
        _, cap, nkf, _ = self._map or (0, 1, 1, 0)  # (no map: the entry refuses)
        dev = _torch_device(self._device)
        _repose_list_args(who, self.n, cap, nkf, dev, (("node_counts", node_counts, torch.int32, ()),
                                                       ("node_of_segment", node_of_segment, torch.int32, (nkf,))))
        ncap, stride = _repose_poses(who, poses, self.n)
        if normals_out is None:
            normals_out = self._map_normals is not None
        own = self.map(copy=False) if self._map else {}
        bufs = (own["xyz"].clone() if xyz_out is True and own else _out_buf(xyz_out, (self.n, cap, 3), torch.float32, dev),
                self.map_normals() if normals_out is True and self._map_normals else _out_buf(normals_out, (self.n, cap, 3), torch.float32, dev),
                own["segments"].clone() if segments_out is True and own else _out_buf(segments_out, (self.n, nkf, 40), torch.uint8, dev),
                _out_buf(counts, (self.n, REPOSE_COUNTS), torch.int32, dev))
        dp = Batch._dp
        _check(lib().vors_trackers_repose_map(self._h, dp(poses), stride, ncap, dp(node_counts), dp(node_of_segment), *[dp(t) for t in bufs],
                                              Batch._stream()))
        self._repose_refs = (poses, node_counts, node_of_segment)
        return _repose_result(bufs, xyz_out, normals_out, segments_out, counts)

    def render_map(self, level=0, poses=None, ranges=None, footprint=1, depth=True, gray=True, counts=False, zkey=False):
        """The keyframe map seen from one pose per sequence (vors_trackers_render_map): render_points() on the handle's own map with the
        intrinsics and the shape of pyramid level `level`, on the current stream, not synchronised. poses None = every sequence's current
        frame pose, read on the device. Everything else, and the result, as in render_points()."""
        lvl = int(level)
        shape = (self.n, self.rows >> lvl, self.cols >> lvl)
        dev = _torch_device(self._device)
        poses, pose_stride = _render_poses(poses, self.n)
        rng, range_stride = _render_ranges(ranges, self.n)
        bufs = _render_outputs(shape, dev, zkey, depth, gray, counts)
        _check(lib().vors_trackers_render_map(self._h, lvl, Batch._dp(poses), pose_stride, rng, range_stride, int(footprint),
                                              *[Batch._dp(t) for t in bufs], Batch._stream()))
        self._render_refs = (poses, ranges)
        return _render_result(bufs, zkey, depth, gray, counts)

    def icp_map(self, depth, dist_m, damping=0.0, step_eps=1e-5, iters=8, min_points=6, poses=None, ranges=None, workspace=None, stats=True,
                sums29=False, residuals=False):
        """The keyframe map aligned to one depth frame per sequence (vors_trackers_icp_map): icp_points() on the handle's own map and map
        normals with its level-0 intrinsics, on the current stream, not synchronised. depth [n, rows, cols] int16 tensor holding the u16
        payload; poses None = every sequence's current frame pose, read on the device. The tracker itself is only read. Everything else,
        and the result, as in icp_points()."""
        return self._icp_map("icp_map", depth, dist_m, damping, step_eps, iters, min_points, poses, ranges, workspace, stats, sums29, residuals)

    def _icp_map(self, who, depth, dist_m, damping, step_eps, iters, min_points, poses, ranges, workspace, stats, sums29, residuals, robust=None,
                 joint=None):
        """The body of icp_map(), icp_map_robust() and icp_map_joint(): vors_trackers_<who>. robust, joint: see _icp_pass (the lists' grey
        levels are the handle's own: None)."""
        import torch
        self._check_frames(depth, depth)
        if depth.dtype != torch.int16:
            raise VorsError(f"{who}: depth int16 [n, rows, cols], contiguous")
        poses, pose_stride = _render_poses(poses, self.n)
        rng, range_stride = _render_ranges(ranges, self.n)
        cap = self._map[1] if self._map else 1  # (no map: the entry refuses)
        ws, more_in, outs, result = _icp_pass(who, self.n, cap, depth, _torch_device(self._device), workspace, stats, sums29, residuals, robust, joint)
        frame_gray = [] if joint is None else [Batch._dp(joint[1])]
        _check(getattr(lib(), "vors_trackers_" + who)(self._h, Batch._dp(depth), *frame_gray, float(dist_m), float(damping), float(step_eps),
                                                      int(iters), int(min_points), rng, range_stride, Batch._dp(poses), pose_stride, *more_in, *outs,
                                                      Batch._stream()))
        self._icp_refs = (depth, poses, ranges, ws) + (() if robust is None else (robust[0],)) + (() if joint is None else (joint[1],))
        return result

    def icp_map_robust(self, depth, dist_m, damping=0.0, step_eps=1e-5, iters=8, min_points=6, frame_normals=None, min_cos=0.0, huber_m=0.0,
                       poses=None, ranges=None, workspace=None, stats=True, sums29=False, residuals=False, gate_counts=False):
        """icp_map() through the robust pass (vors_trackers_icp_map_robust): icp_points_robust() on the handle's own map and map normals.
        frame_normals [n, rows, cols, 3] float32 (depth_normals() of `depth` at level 0 without poses; None = no gate), min_cos, huber_m
        and gate_counts as in icp_points_robust(); everything else as in icp_map()."""
        return self._icp_map("icp_map_robust", depth, dist_m, damping, step_eps, iters, min_points, poses, ranges, workspace, stats, sums29, residuals,
                             (frame_normals, min_cos, huber_m, gate_counts))

    def icp_map_joint(self, depth, dist_m, frame_gray=None, damping=0.0, step_eps=1e-5, iters=8, min_points=6, frame_normals=None, min_cos=0.0,
                      huber_m=0.0, photo_scale_m=0.0, photo_huber_grey=0.0, poses=None, ranges=None, workspace=None, stats=True, sums29=False,
                      residuals=False, gate_counts=False, photo_residuals=False, photo_counts=False):
        """icp_map_robust() through the joint pass (vors_trackers_icp_map_joint): icp_points_joint() on the handle's own map, map normals
        and map grey levels. frame_gray [n, rows, cols] uint8 (the level-0 grey frames `depth` belongs to; None only with photo_scale_m 0),
        photo_scale_m, photo_huber_grey, photo_residuals and photo_counts as in icp_points_joint(); everything else as in icp_map_robust()."""
        return self._icp_map("icp_map_joint", depth, dist_m, damping, step_eps, iters, min_points, poses, ranges, workspace, stats, sums29, residuals,
                             (frame_normals, min_cos, huber_m, gate_counts),
                             (None, frame_gray, photo_scale_m, photo_huber_grey, photo_residuals, photo_counts))

    def enable_kernel_timing(self, ring=64):
        _check(lib().vors_trackers_enable_kernel_timing(self._h, int(ring)))

    def kernel_times(self, stage):
        out = np.zeros(4096, np.float32)
        n = C.c_int()
        _check(lib().vors_trackers_kernel_times(self._h, Batch.STAGES[stage], _ptr(out), 4096, C.byref(n)))
        return out[:n.value].copy()


class _DeviceArray:
    """A device pointer the library owns, dressed for torch.as_tensor (__cuda_array_interface__)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def _device_view(ptr, shape, typestr, device):
    import torch
    return torch.as_tensor(_DeviceArray(ptr, shape, typestr), device=device)


def synth_render_frames(seeds, salts, xis, rows, cols, cam5, invalid_percent=2, device="cuda"):
    """Frames of the synthetic scene at explicit twists (vors_synth_render_frames) -> gray u8 [n,rows,cols], depth (int16 payload u16)."""
    import torch
    seeds = np.ascontiguousarray(seeds, np.uint64)
    salts = np.ascontiguousarray(salts, np.uint64)
    xis = np.ascontiguousarray(xis, np.float64).reshape(-1, 6)
    n = len(seeds)
    assert len(salts) == n and len(xis) == n
    gray = torch.empty((n, rows, cols), dtype=torch.uint8, device=device)
    depth = torch.empty((n, rows, cols), dtype=torch.int16, device=device)
    cam = np.asarray(cam5, np.float64)
    _check(lib().vors_synth_render_frames(n, _ptr(seeds), _ptr(salts), _ptr(xis), rows, cols, _ptr(cam), invalid_percent,
                                          Batch._dp(gray), Batch._dp(depth), Batch._stream()))
    return gray, depth


def stats_tensor(n, device="cuda"):
    """Device buffer for n vors_pair_stats (as raw bytes); decode with decode_stats()."""
    import torch
    return torch.zeros(n * PAIR_STATS_DTYPE.itemsize, dtype=torch.uint8, device=device)


def decode_stats(t):
    return np.frombuffer(t.cpu().numpy().tobytes(), PAIR_STATS_DTYPE)


def synth_render_pairs(seed0, n_pairs, rows, cols, cam5, motion_scale=1.0, invalid_percent=2, want_cur_depth=False,
                       device="cuda"):
    """Render synthetic frame pairs on the device (vors_synth_render_pairs). Returns torch tensors."""
    import torch
    kg = torch.empty((n_pairs, rows, cols), dtype=torch.uint8, device=device)
    kd = torch.empty((n_pairs, rows, cols), dtype=torch.int16, device=device)  # u16 payload
    cg = torch.empty((n_pairs, rows, cols), dtype=torch.uint8, device=device)
    cd = torch.empty((n_pairs, rows, cols), dtype=torch.int16, device=device) if want_cur_depth else None
    gt = torch.empty((n_pairs, 7), dtype=torch.float32, device=device)
    cam = np.asarray(cam5, np.float64)
    _check(lib().vors_synth_render_pairs(int(seed0), n_pairs, rows, cols, _ptr(cam), float(motion_scale), invalid_percent,
                                         Batch._dp(kg), Batch._dp(kd), Batch._dp(cg), Batch._dp(cd), Batch._dp(gt),
                                         Batch._stream()))
    return kg, kd, cg, cd, gt


# ----------------------------------------------------------------------------------------------- operator level
class Obs:
    """lm_optimizer.rs:43-58 (hessians are recomputed on the device, not passed)."""

    def __init__(self, intrinsics5, template, image, coordinates, _z_candidates, jacobians, huber_delta=0.0, arithmetic=ARITH_REFERENCE):
        self.intrinsics = np.ascontiguousarray(intrinsics5, np.float32)
        self.template = np.ascontiguousarray(template, np.uint8)
        self.image = np.ascontiguousarray(image, np.uint8)
        self.coordinates = np.ascontiguousarray(coordinates, np.int32).reshape(-1, 2)
        self._z_candidates = np.ascontiguousarray(_z_candidates, np.float32)
        self.jacobians = np.ascontiguousarray(jacobians, np.float32).reshape(-1, 6)
        self.huber_delta = float(huber_delta)
        self.arithmetic = int(arithmetic)  # ARITH_REFERENCE: sequential sums in the order of `coordinates`

    def to_c(self):
        k = self.intrinsics
        rows, cols = self.template.shape
        u8p, i32p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)
        return vors_obs(k[0], k[1], k[2], k[3], k[4], rows, cols, self.template.ctypes.data_as(u8p),
                        self.image.ctypes.data_as(u8p), len(self._z_candidates), self.coordinates.ctypes.data_as(i32p),
                        self._z_candidates.ctypes.data_as(f32p), self.jacobians.ctypes.data_as(f32p), self.huber_delta, self.arithmetic)


def lm_eval(obs, model7, want_residuals=False):
    """eval_energy + compute_eval_data (lm_optimizer.rs:68-107) on the device -> energy, n_inside, g[6], H[6,6]."""
    model7 = np.ascontiguousarray(model7, np.float32)
    e, n = C.c_float(), C.c_int32()
    g = np.zeros(6, np.float32)
    H = np.zeros((6, 6), np.float32)
    res = np.zeros(len(obs._z_candidates), np.float32) if want_residuals else None
    o = obs.to_c()
    _check(lib().vors_lm_eval(C.byref(o), _ptr(model7), C.byref(e), C.byref(n), _ptr(g), _ptr(H), _ptr(res)))
    return (e.value, n.value, g, H, res) if want_residuals else (e.value, n.value, g, H)


def pose_information_from_sums(sums29):
    """Pose information of one evaluation's 29 sums on the host (vors_pose_information_from_sums; needs no GPU)
    -> (info [6, 6], cov [6, 6], sigma2, flags)."""
    sums29 = np.ascontiguousarray(sums29, np.float32)
    if sums29.shape != (29,):
        raise VorsError(f"expected 29 sums, got shape {sums29.shape}")
    info, cov = np.zeros((6, 6), np.float32), np.zeros((6, 6), np.float32)
    s2, fl = C.c_float(), C.c_int32()
    _check(lib().vors_pose_information_from_sums(_ptr(sums29), _ptr(info), _ptr(cov), C.byref(s2), C.byref(fl)))
    return info, cov, np.float32(s2.value), int(fl.value)


def residual_scale_from_hist(hist):
    """Scale of the residuals from a 256-bin histogram of |r| on the host (vors_residual_scale_from_hist; needs no GPU)
    -> (median_abs, sigma_mad = 1.4826 median_abs, n_inside); both scales NaN when the histogram is empty."""
    hist = np.asarray(hist)
    if hist.shape != (RESIDUAL_BINS,) or hist.dtype.kind not in "iu" or (hist < 0).any() or (hist > 0xffffffff).any():
        raise VorsError(f"expected {RESIDUAL_BINS} counts (non-negative integers below 2^32), got {hist.dtype} {hist.shape}")
    hist = np.ascontiguousarray(hist.astype(np.uint32))
    med, sig, n = C.c_float(), C.c_float(), C.c_uint32()
    _check(lib().vors_residual_scale_from_hist(_ptr(hist), C.byref(med), C.byref(sig), C.byref(n)))
    return np.float32(med.value), np.float32(sig.value), int(n.value)


def to_depth(scale, idepth):
    """inverse_depth.rs:37-42 for an array on the host (vors_to_depth; needs no GPU): round(scale / idepth), halves away from zero, converted
    like Rust's `as u16` (NaN -> 0, <= 0 -> 0, >= 65535 -> 65535) -> uint16 array of idepth's shape."""
    x = np.ascontiguousarray(idepth, np.float32)
    out = np.empty(x.shape, np.uint16)
    lib().vors_to_depth(float(scale), _ptr(x), x.size, _ptr(out))
    return out


def from_depth(scale, depth):
    """inverse_depth.rs:24-29 for an array on the host (vors_from_depth): scale / depth, NaN (Unknown) where depth is 0 -> float32 array."""
    d = np.ascontiguousarray(depth, np.uint16)
    out = np.empty(d.shape, np.float32)
    lib().vors_from_depth(float(scale), _ptr(d), d.size, _ptr(out))
    return out


def camera_back_project(cam5, pose7, xy, depth):
    """Camera::back_project for arrays on the host (vors_camera_back_project; needs no GPU): pose7 * intrinsics.back_project(xy, depth) with
    cam5 = (cu, cv, fu, fv, skew), pose7 camera -> world or None (identity, no transform), xy [n, 2], depth [n] -> float32 [n, 3]. The
    arithmetic Batch.point_cloud runs per point."""
    k = np.ascontiguousarray(cam5, np.float32)
    pose = None if pose7 is None else np.ascontiguousarray(pose7, np.float32)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(depth, np.float32).reshape(-1)
    if k.shape != (5,) or (pose is not None and pose.shape != (7,)) or len(d) != len(xy):
        raise VorsError("camera_back_project: cam5 [5], pose7 [7] or None, xy [n, 2], depth [n]")
    out = np.empty((len(xy), 3), np.float32)
    lib().vors_camera_back_project(_ptr(k), _ptr(pose), _ptr(xy), _ptr(d), len(xy), _ptr(out))
    return out


def camera_project(cam5, pose7, xyz):
    """Camera::project for arrays on the host (vors_camera_project): intrinsics.project(rotation^-1 * (translation^-1 * point)) -> float32
    [n, 3] homogeneous (u w, v w, w); pose7 None = identity (no transform)."""
    k = np.ascontiguousarray(cam5, np.float32)
    pose = None if pose7 is None else np.ascontiguousarray(pose7, np.float32)
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if k.shape != (5,) or (pose is not None and pose.shape != (7,)):
        raise VorsError("camera_project: cam5 [5], pose7 [7] or None, xyz [n, 3]")
    out = np.empty((len(p), 3), np.float32)
    lib().vors_camera_project(_ptr(k), _ptr(pose), _ptr(p), len(p), _ptr(out))
    return out


ZKEY_EMPTY = 0xFFFFFFFFFFFFFFFF
FUSE_COUNTS = 6


def fuse_depth_pixels(depth_scale, tol_m, zkey, cur_depth, kf_weight=None, max_weight=255, fill_min_weight=0, n_kf_pixels=None):
    """The merge of Batch.fuse_depth for arrays on the host (vors_fuse_depth_pixels; needs no GPU): zkey (uint64, or int64 holding that
    payload) and cur_depth (uint16) of one shape, kf_weight (uint8, any shape: indexed flat by the keys' source pixel) or None ->
    (depth uint16, weight uint8, counts uint32 [6]). n_kf_pixels bounds the source indices (default: kf_weight's size, else zkey's)."""
    key = np.ascontiguousarray(zkey)
    if key.dtype == np.int64:
        key = key.view(np.uint64)
    d = np.ascontiguousarray(cur_depth)
    if d.dtype == np.int16:
        d = d.view(np.uint16)
    w = None if kf_weight is None else np.ascontiguousarray(kf_weight)
    if key.dtype != np.uint64 or d.dtype != np.uint16 or key.shape != d.shape or (w is not None and w.dtype != np.uint8):
        raise VorsError("fuse_depth_pixels: zkey uint64 and cur_depth uint16 of one shape, kf_weight uint8 or None")
    if n_kf_pixels is None:
        n_kf_pixels = w.size if w is not None else key.size
    if w is not None and int(n_kf_pixels) > w.size:
        raise VorsError("fuse_depth_pixels: n_kf_pixels exceeds kf_weight")
    depth, weight, counts = np.empty(key.shape, np.uint16), np.empty(key.shape, np.uint8), np.zeros(FUSE_COUNTS, np.uint32)
    _check(lib().vors_fuse_depth_pixels(float(depth_scale), float(tol_m), int(max_weight), int(fill_min_weight), key.size, _ptr(key), _ptr(d),
                                        _ptr(w), int(n_kf_pixels), _ptr(depth), _ptr(weight), _ptr(counts)))
    return depth, weight, counts


def _torch_device(index=None):
    import torch
    return torch.device("cuda", torch.cuda.current_device() if index is None else int(index))


def _render_poses(poses, n):
    """poses [n, 7] float32 or a track's out_stats bytes, or None -> (tensor, stride in bytes)."""
    if poses is None:
        return None, 0
    refusal = f"render: expected one pose for each of the {n} lists"
    poses, m, stride = Batch._one_per_pair(poses, refusal)
    if m < n:
        raise VorsError(refusal)
    return poses, stride


def _render_ranges(ranges, n):
    """ranges: None, an int32 tensor [n, 2] of (first, count), or (tensor, offset_bytes, stride_bytes) — e.g. (map["segments"], 40 k + 4, 40
    MAX_KEYFRAMES) for keyframe k of every sequence -> (device pointer, stride in bytes)."""
    import torch
    if ranges is None:
        return None, 0
    if isinstance(ranges, tuple):
        t, off, stride = ranges
        if not t.is_contiguous() or int(off) < 0 or int(off) + 8 + (n - 1) * int(stride) > t.numel() * t.element_size():
            raise VorsError("render: the (first, count) pairs must lie inside the contiguous ranges tensor")
        return C.c_void_p(t.data_ptr() + int(off)), int(stride)
    if ranges.dtype != torch.int32 or not ranges.is_contiguous() or tuple(ranges.shape) != (n, 2):
        raise VorsError(f"render: expected a contiguous int32 ranges [{n}, 2], got {ranges.dtype} {tuple(ranges.shape)}")
    return C.c_void_p(ranges.data_ptr()), 0


def _render_outputs(shape, dev, zkey, depth, gray, counts):
    """The output arguments of a rendering (_out_buf) -> (zkey, depth, gray, counts); the key plane is made all the same."""
    import torch
    return (_out_buf(zkey, shape, torch.int64, dev, always=True), _out_buf(depth, shape, torch.int16, dev), _out_buf(gray, shape, torch.uint8, dev),
            _out_buf(counts, (shape[0], RENDER_COUNTS), torch.int32, dev))


def _render_result(bufs, zkey, depth, gray, counts):
    return _result(*((name, _asked(want), t) for name, want, t in zip(("zkey", "depth", "gray", "counts"), (zkey, depth, gray, counts), bufs)))


def render_points(xyz, list_gray, list_counts, cam5, rows, cols, depth_scale, poses=None, ranges=None, footprint=1, depth=True, gray=True,
                  counts=False, zkey=False):
    """n world-frame point lists seen from one camera pose each (vors_render_points; handle-free) -> dict of the requested tensors on the
    current stream, not synchronised: "depth" [n, rows, cols] (int16 tensor holding the u16 payload, 0 = nothing landed), "gray" [n, rows,
    cols] uint8, "zkey" [n, rows, cols] (int64 tensor holding bits(Z') << 32 | rank, -1 = empty), "counts" [n, 4] int32 (considered, in
    front, landed, covered). xyz [n, capacity, 3] float32, list_gray [n, capacity] uint8, list_counts [n] int32: the tensors of
    Trackers.map() / Batch.point_cloud(). poses [n, 7] float32 camera -> world (None = no transform); ranges: see _render_ranges;
    footprint 1, 2 or 3 pixels wide. depth / gray / counts / zkey may also be a tensor of that shape to write into."""
    import torch
    n = xyz.shape[0]
    cap = xyz.shape[1] if xyz.dim() == 3 else -1
    if (xyz.dtype != torch.float32 or not xyz.is_contiguous() or xyz.dim() != 3 or xyz.shape[2] != 3 or list_gray.dtype != torch.uint8
            or not list_gray.is_contiguous() or tuple(list_gray.shape) != (n, cap) or list_counts.dtype != torch.int32
            or not list_counts.is_contiguous() or tuple(list_counts.shape) != (n,)):
        raise VorsError("render_points: xyz float32 [n, capacity, 3], list_gray uint8 [n, capacity], list_counts int32 [n], contiguous")
    k = np.ascontiguousarray(cam5, np.float32)
    if k.shape != (5,):
        raise VorsError("render_points: cam5 [5]")
    poses, pose_stride = _render_poses(poses, n)
    rng, range_stride = _render_ranges(ranges, n)
    bufs = _render_outputs((n, int(rows), int(cols)), xyz.device, zkey, depth, gray, counts)
    _check(lib().vors_render_points(n, Batch._dp(xyz), Batch._dp(list_gray), Batch._dp(list_counts), cap, rng, range_stride, _ptr(k), int(rows),
                                    int(cols), float(depth_scale), Batch._dp(poses), pose_stride, int(footprint),
                                    *[Batch._dp(t) for t in bufs], Batch._stream()))
    return _render_result(bufs, zkey, depth, gray, counts)


def _voxel_means_result(bufs, xyz_mean, gray_mean, kept):
    return _result(*((name, _asked(want), t) for name, want, t in zip(("xyz_mean", "gray_mean", "kept"), (xyz_mean, gray_mean, kept), bufs)))


def voxel_means(xyz, list_counts, sums, obs, voxel_m, min_count=1, min_span=0, first_segment_of_rank=None, xyz_mean=True, gray_mean=True,
                kept=True):
    """Voxel statistics resolved into an averaged list (vors_voxel_means; handle-free) -> dict of the requested tensors on the current
    stream, not synchronised: "xyz_mean" [n, capacity, 3] float32 and "gray_mean" [n, capacity] uint8, written for the ranks below
    min(count, capacity) — the centroid and mean grey of the rank's voxel, or NaN and grey 0 where it was seen fewer than max(min_count, 1)
    times or over fewer than min_span segments, which render_points() and every ICP pass skip — and "kept" [n] int32, the passing ranks.
    xyz [n, capacity, 3] float32, list_counts [n] int32: the tensors of Trackers.map(); sums [n, capacity, 4] int64, obs [n, capacity, 2]
    int32: those of Trackers.map_voxel_stats(); first_segment_of_rank [n, capacity] int32 or None (then min_span must be 0). xyz_mean /
    gray_mean / kept may also be a tensor of that shape to write into."""
    import torch
    n = xyz.shape[0]
    cap = xyz.shape[1] if xyz.dim() == 3 else -1
    fs = first_segment_of_rank
    if (xyz.dtype != torch.float32 or not xyz.is_contiguous() or xyz.dim() != 3 or xyz.shape[2] != 3 or list_counts.dtype != torch.int32
            or not list_counts.is_contiguous() or tuple(list_counts.shape) != (n,) or sums.dtype != torch.int64 or not sums.is_contiguous()
            or tuple(sums.shape) != (n, cap, 4) or obs.dtype != torch.int32 or not obs.is_contiguous() or tuple(obs.shape) != (n, cap, 2)
            or (fs is not None and (fs.dtype != torch.int32 or not fs.is_contiguous() or tuple(fs.shape) != (n, cap)))):
        raise VorsError("voxel_means: xyz float32 [n, capacity, 3], list_counts int32 [n], sums int64 [n, capacity, 4], obs int32 [n, capacity, 2], "
                        "first_segment_of_rank int32 [n, capacity] or None, contiguous")
    bufs = (_out_buf(xyz_mean, (n, cap, 3), torch.float32, xyz.device), _out_buf(gray_mean, (n, cap), torch.uint8, xyz.device),
            _out_buf(kept, (n,), torch.int32, xyz.device))
    _check(lib().vors_voxel_means(n, Batch._dp(xyz), Batch._dp(list_counts), cap, Batch._dp(sums), Batch._dp(obs), float(voxel_m),
                                  _u32("min_count", min_count), _u32("min_span", min_span), Batch._dp(fs), *[Batch._dp(t) for t in bufs],
                                  Batch._stream()))
    return _voxel_means_result(bufs, xyz_mean, gray_mean, kept)


def render_points_host(xyz, list_gray, cam5, rows, cols, depth_scale, pose7=None, footprint=1, count=None, range2=None):
    """The rule of render_points for ONE list on the host (vors_render_points_host; needs no GPU; the text the kernels run): xyz
    [capacity, 3] float32, list_gray [capacity] uint8, count = the list's count (None = capacity; above it: clipped), range2 = (first,
    count) or None, pose7 camera -> world or None -> dict: "zkey" [rows, cols] uint64, "depth" uint16, "gray" uint8, "counts" [4] uint32."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    g = np.ascontiguousarray(list_gray, np.uint8).reshape(-1)
    k = np.ascontiguousarray(cam5, np.float32)
    pose = None if pose7 is None else np.ascontiguousarray(pose7, np.float32)
    rng = None if range2 is None else np.ascontiguousarray(range2, np.uint32)
    if len(p) != len(g) or k.shape != (5,) or (pose is not None and pose.shape != (7,)) or (rng is not None and rng.shape != (2,)):
        raise VorsError("render_points_host: xyz [capacity, 3], list_gray [capacity], cam5 [5], pose7 [7] or None, range2 [2] or None")
    shape = (max(int(rows), 0), max(int(cols), 0))
    out = dict(zkey=np.empty(shape, np.uint64), depth=np.empty(shape, np.uint16), gray=np.empty(shape, np.uint8),
               counts=np.zeros(RENDER_COUNTS, np.uint32))
    _check(lib().vors_render_points_host(_ptr(p), _ptr(g), len(p) if count is None else int(count), len(p), _ptr(rng), _ptr(k), int(rows),
                                         int(cols), float(depth_scale), _ptr(pose), int(footprint), _ptr(out["zkey"]), _ptr(out["depth"]),
                                         _ptr(out["gray"]), _ptr(out["counts"])))
    return out


def _normals_common(cam5, who):
    k = np.ascontiguousarray(cam5, np.float32)
    if k.shape != (5,):
        raise VorsError(f"{who}: cam5 [5]")
    return k


def _normals_outputs(shape3, dev, normals, counts):
    """The output arguments of a normals pass (_out_buf) -> (normals, counts)."""
    import torch
    return _out_buf(normals, shape3, torch.float32, dev), _out_buf(counts, (shape3[0], NORMAL_COUNTS), torch.int32, dev)


def depth_normals(depth, cam5, depth_scale, step, jump_m, poses=None, normals=True, counts=False):
    """Surface normals of n level-0 depth planes (vors_depth_normals; handle-free) -> dict of the requested tensors on the current stream,
    not synchronised: "normals" [n, rows, cols, 3] float32 (unit, facing the camera, three zeros = no normal), "counts" [n, 3] int32
    (considered, with depth, with a normal). depth [n, rows, cols] int16 tensor holding the u16 payload; cam5 = cu cv fu fv skew; step
    1..8 pixels to the neighbours; jump_m: a neighbour further than this in depth is left out. poses [n, 7] float32 camera -> world (None =
    camera frame; only the rotation is applied). normals / counts may also be a tensor of that shape to write into."""
    import torch
    if depth.dtype != torch.int16 or depth.dim() != 3 or not depth.is_contiguous():
        raise VorsError("depth_normals: depth int16 [n, rows, cols], contiguous")
    n, rows, cols = depth.shape
    k = _normals_common(cam5, "depth_normals")
    poses, pose_stride = _render_poses(poses, n)
    o_n, o_c = _normals_outputs((n, rows, cols, 3), depth.device, normals, counts)
    _check(lib().vors_depth_normals(n, Batch._dp(depth), _ptr(k), rows, cols, float(depth_scale), int(step), float(jump_m), Batch._dp(poses),
                                    pose_stride, Batch._dp(o_n), Batch._dp(o_c), Batch._stream()))
    return _result(("normals", _asked(normals), o_n), ("counts", _asked(counts), o_c))


def points_normals(depth, pixel, list_counts, cam5, depth_scale, step, jump_m, poses=None, ranges=None, normals=True, counts=False):
    """Surface normals of LISTED pixels of n level-0 depth planes (vors_points_normals; handle-free) -> dict as depth_normals(), "normals"
    [n, capacity, 3]: exactly the ranks of each list's clipped range are written, everything else of a tensor passed in is left untouched
    (a new tensor is zeroed first). pixel [n, capacity] int32 (x | y << 16) and list_counts [n] int32: the tensors of Trackers.map() /
    Batch.point_cloud(); ranges: see _render_ranges; a pixel outside the plane has no normal."""
    import torch
    if depth.dtype != torch.int16 or depth.dim() != 3 or not depth.is_contiguous():
        raise VorsError("points_normals: depth int16 [n, rows, cols], contiguous")
    n, rows, cols = depth.shape
    cap = pixel.shape[1] if pixel.dim() == 2 else -1
    if (pixel.dtype != torch.int32 or not pixel.is_contiguous() or tuple(pixel.shape) != (n, cap) or list_counts.dtype != torch.int32
            or not list_counts.is_contiguous() or tuple(list_counts.shape) != (n,)):
        raise VorsError("points_normals: pixel int32 [n, capacity], list_counts int32 [n], contiguous")
    k = _normals_common(cam5, "points_normals")
    poses, pose_stride = _render_poses(poses, n)
    rng, range_stride = _render_ranges(ranges, n)
    o_n, o_c = _normals_outputs((n, cap, 3), depth.device, normals, counts)
    if normals is True:
        o_n.zero_()
    _check(lib().vors_points_normals(n, Batch._dp(depth), Batch._dp(pixel), Batch._dp(list_counts), cap, rng, range_stride, _ptr(k), rows, cols,
                                     float(depth_scale), int(step), float(jump_m), Batch._dp(poses), pose_stride, Batch._dp(o_n),
                                     Batch._dp(o_c), Batch._stream()))
    return _result(("normals", _asked(normals), o_n), ("counts", _asked(counts), o_c))


def depth_normals_host(depth, cam5, depth_scale, step, jump_m, pose7=None, pixel=None, count=None, range2=None, normals=None):
    """The rule of depth_normals / points_normals for ONE plane on the host (vors_depth_normals_host; needs no GPU; the text the kernels
    run): depth [rows, cols] uint16 -> dict: "normals" float32 and "counts" [3] uint32. pixel None: the plane form, normals [rows, cols, 3].
    pixel [capacity] uint32 (x | y << 16): the list form, normals [capacity, 3] with only the ranks of the clipped range written — count =
    the list's count (None = capacity; above it: clipped), range2 = (first, count) or None; `normals`: an array to write into (None = a
    zeroed one). pose7 camera -> world or None."""
    d = np.ascontiguousarray(depth, np.uint16)
    k = np.ascontiguousarray(cam5, np.float32)
    pose = None if pose7 is None else np.ascontiguousarray(pose7, np.float32)
    rng = None if range2 is None else np.ascontiguousarray(range2, np.uint32)
    px = None if pixel is None else np.ascontiguousarray(pixel, np.uint32).reshape(-1)
    if d.ndim != 2 or k.shape != (5,) or (pose is not None and pose.shape != (7,)) or (rng is not None and rng.shape != (2,)):
        raise VorsError("depth_normals_host: depth [rows, cols], cam5 [5], pose7 [7] or None, range2 [2] or None")
    rows, cols = d.shape
    shape = (rows, cols, 3) if px is None else (len(px), 3)
    if normals is None:
        normals = np.zeros(shape, np.float32)
    elif normals.dtype != np.float32 or normals.shape != shape or not normals.flags.c_contiguous:
        raise VorsError(f"depth_normals_host: normals must be a contiguous float32 array {shape}")
    cap = 0 if px is None else len(px)
    out = dict(normals=normals, counts=np.zeros(NORMAL_COUNTS, np.uint32))
    _check(lib().vors_depth_normals_host(_ptr(d), _ptr(k), rows, cols, float(depth_scale), int(step), float(jump_m), _ptr(pose), _ptr(px),
                                         cap if count is None else int(count), cap, _ptr(rng), _ptr(normals), _ptr(out["counts"])))
    return out


# ----------------------------------------------------------------------------------------------- sensor front end
def _front_cameras(who, cams, dist5=None, pose7=None):
    """cam5 arrays, the distortion coefficients and a pose as contiguous float32 (None stays None), shapes checked."""
    ks = [np.ascontiguousarray(k, np.float32) for k in cams]
    d = None if dist5 is None else np.ascontiguousarray(dist5, np.float32)
    p = None if pose7 is None else np.ascontiguousarray(pose7, np.float32)
    if any(k.shape != (5,) for k in ks) or (d is not None and d.shape != (5,)) or (p is not None and p.shape != (7,)):
        raise VorsError(f"{who}: a camera is cu cv fu fv skew [5], dist5 k1 k2 p1 p2 k3 [5] or None, pose7 [7] or None")
    return ks, d, p


def _front_planes(who, planes, dtypes):
    """The input planes of a device pass: each None or a contiguous tensor [n, rows, cols] of its dtype, all of one shape -> that shape
    and the device (None, None without any plane: the C entry refuses that)."""
    shape = dev = None
    for t, dtype in zip(planes, dtypes):
        if t is None:
            continue
        if t.dtype != dtype or t.dim() != 3 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise VorsError(f"{who}: the planes are contiguous tensors [n, rows, cols] of one shape (grey uint8, depth int16)")
        shape, dev = tuple(t.shape), t.device
    return shape, dev


def _host_out(who, o, shape, dtype, fill=None):
    """An output argument of a host entry: True = a new array, an array = that one after a check, False / None = not wanted."""
    if o is True:
        return np.empty(shape, dtype) if fill is None else np.full(shape, fill, dtype)
    if not _asked(o):
        return None
    if not isinstance(o, np.ndarray) or o.dtype != dtype or o.shape != tuple(shape) or not o.flags.c_contiguous:
        raise VorsError(f"{who}: expected a contiguous {np.dtype(dtype)} output {tuple(shape)}")
    return o


def undistort_frames(gray, depth, cam_in5, dist5, cam_out5, out_rows, out_cols, border=0, gray_out=None, depth_out=None, map=False,
                     counts=False):
    """n grey and / or depth planes of a real camera resampled into an ideal pinhole camera (vors_undistort_frames; handle-free) -> dict
    of the requested tensors on the current stream, not synchronised: "gray" [n, out_rows, out_cols] uint8 (bilinear), "depth" (int16
    tensor holding the u16 payload; nearest source pixel, never interpolated, 0 outside), "map" [out_rows, out_cols, 2] float32 (the
    source coordinate (u, v) of every output pixel), "counts" [n, 3] int32 (pixels, grey inside, depth inside and non-zero). gray uint8 /
    depth int16 [n, in_rows, in_cols] or None; cam_in5 / cam_out5 = cu cv fu fv skew of the real and of the ideal camera; dist5 = k1 k2 p1
    p2 k3 (Brown-Conrady) or None; border 0 = zero outside, 1 = edge replicate (grey only). gray_out / depth_out default to "where the
    input is given"; every output may also be a tensor of its shape to write into."""
    import torch
    who = "undistort_frames"
    (k_in, k_out), d5, _ = _front_cameras(who, (cam_in5, cam_out5), dist5)
    shape, dev = _front_planes(who, (gray, depth), (torch.uint8, torch.int16))
    n, in_rows, in_cols = shape if shape else (1, 0, 0)
    dev = dev if dev is not None else next((t.device for t in (gray_out, depth_out, map, counts) if hasattr(t, "device")), None)
    gray_out = (gray is not None) if gray_out is None else gray_out
    depth_out = (depth is not None) if depth_out is None else depth_out
    oshape = (n, int(out_rows), int(out_cols))
    bufs = (_out_buf(gray_out, oshape, torch.uint8, dev), _out_buf(depth_out, oshape, torch.int16, dev),
            _out_buf(map, oshape[1:] + (2,), torch.float32, dev), _out_buf(counts, (n, UNDISTORT_COUNTS), torch.int32, dev))
    _check(lib().vors_undistort_frames(n, Batch._dp(gray), Batch._dp(depth), in_rows, in_cols, _ptr(k_in), _ptr(d5), _ptr(k_out), oshape[1],
                                       oshape[2], int(border), *[Batch._dp(t) for t in bufs], Batch._stream()))
    return _result(*((name, _asked(want), t) for name, want, t in zip(("gray", "depth", "map", "counts"), (gray_out, depth_out, map, counts), bufs)))


def undistort_frame_host(gray, depth, cam_in5, dist5, cam_out5, out_rows, out_cols, border=0, gray_out=None, depth_out=None, map=True,
                         counts=True):
    """The rule of undistort_frames for ONE plane of each kind on the host (vors_undistort_frame_host; needs no GPU; the text the kernel
    runs): gray [in_rows, in_cols] uint8 / depth uint16 or None -> dict: "gray", "depth" (where the input is given), "map" [out_rows,
    out_cols, 2] float32, "counts" [3] uint32. Every output may also be an array of its shape to write into, or False."""
    who = "undistort_frame_host"
    (k_in, k_out), d5, _ = _front_cameras(who, (cam_in5, cam_out5), dist5)
    g = None if gray is None else np.ascontiguousarray(gray, np.uint8)
    d = None if depth is None else np.ascontiguousarray(depth, np.uint16)
    shapes = {a.shape for a in (g, d) if a is not None}
    if len(shapes) > 1 or any(len(sh) != 2 for sh in shapes):
        raise VorsError(f"{who}: gray and depth [in_rows, in_cols] of one shape (each may be None)")
    in_rows, in_cols = shapes.pop() if shapes else (0, 0)
    gray_out = (g is not None) if gray_out is None else gray_out
    depth_out = (d is not None) if depth_out is None else depth_out
    oshape = (max(int(out_rows), 0), max(int(out_cols), 0))
    bufs = (_host_out(who, gray_out, oshape, np.uint8), _host_out(who, depth_out, oshape, np.uint16),
            _host_out(who, map, oshape + (2,), np.float32), _host_out(who, counts, (UNDISTORT_COUNTS,), np.uint32, fill=0))
    _check(lib().vors_undistort_frame_host(_ptr(g), _ptr(d), in_rows, in_cols, _ptr(k_in), _ptr(d5), _ptr(k_out), int(out_rows), int(out_cols),
                                           int(border), *[_ptr(b) for b in bufs]))
    return _result(*((name, _asked(want), t) for name, want, t in zip(("gray", "depth", "map", "counts"), (gray_out, depth_out, map, counts), bufs)))


def undistort_source_host(cam_in5, dist5, cam_out5, xy):
    """The source coordinate (u, v) in the real camera of output pixels xy [m, 2] int32 (x, y) of the ideal camera
    (vors_undistort_source_host; needs no GPU; the text the kernel runs) -> [m, 2] float32."""
    who = "undistort_source_host"
    (k_in, k_out), d5, _ = _front_cameras(who, (cam_in5, cam_out5), dist5)
    p = np.ascontiguousarray(xy, np.int32)
    if p.ndim != 2 or p.shape[1] != 2:
        raise VorsError(f"{who}: xy [m, 2]")
    uv = np.empty(p.shape, np.float32)
    _check(lib().vors_undistort_source_host(_ptr(k_in), _ptr(d5), _ptr(k_out), len(p), _ptr(p), _ptr(uv)))
    return uv


def register_depth(depth, dcam5, depth_scale_in, ccam5, c_rows, c_cols, depth_scale_out, pose7=None, footprint=1, depth_out=True,
                   src_index=False, counts=False, zkey=False):
    """n depth planes of a pinhole depth camera registered into a colour camera (vors_register_depth; handle-free) -> dict of the requested
    tensors on the current stream, not synchronised: "depth" [n, c_rows, c_cols] (int16 tensor holding the u16 payload in units of 1 /
    depth_scale_out, 0 = nothing landed), "src_index" (int32 tensor holding the u32 payload: y * d_cols + x of the winning source pixel, -1
    = nothing landed), "zkey" (int64 tensor holding bits(Z') << 32 | source index, -1 = empty), "counts" [n, 4] int32 (with depth, in
    front, landed, covered). depth [n, d_rows, d_cols] int16 tensor holding the u16 payload in units of 1 / depth_scale_in; dcam5 / ccam5 =
    cu cv fu fv skew of the depth and of the colour camera; pose7 (host) = depth camera -> colour camera, tx ty tz qi qj qk qw, or None;
    footprint 1, 2 or 3 pixels wide. Every output may also be a tensor of its shape to write into."""
    import torch
    who = "register_depth"
    (k_d, k_c), _, pose = _front_cameras(who, (dcam5, ccam5), None, pose7)
    shape, dev = _front_planes(who, (depth,), (torch.int16,))
    if shape is None:
        raise VorsError(f"{who}: depth int16 [n, d_rows, d_cols], contiguous")
    n, d_rows, d_cols = shape
    oshape = (n, int(c_rows), int(c_cols))
    bufs = (_out_buf(zkey, oshape, torch.int64, dev, always=True), _out_buf(depth_out, oshape, torch.int16, dev),
            _out_buf(src_index, oshape, torch.int32, dev), _out_buf(counts, (n, REGISTER_COUNTS), torch.int32, dev))
    _check(lib().vors_register_depth(n, Batch._dp(depth), _ptr(k_d), d_rows, d_cols, float(depth_scale_in), _ptr(pose), _ptr(k_c), oshape[1],
                                     oshape[2], float(depth_scale_out), int(footprint), *[Batch._dp(t) for t in bufs], Batch._stream()))
    return _result(*((name, _asked(want), t) for name, want, t in zip(("zkey", "depth", "src_index", "counts"), (zkey, depth_out, src_index, counts), bufs)))


def register_depth_host(depth, dcam5, depth_scale_in, ccam5, c_rows, c_cols, depth_scale_out, pose7=None, footprint=1, depth_out=True,
                        src_index=True, counts=True, zkey=True):
    """The rule of register_depth for ONE plane on the host (vors_register_depth_host; needs no GPU; the text the kernels run): depth
    [d_rows, d_cols] uint16 -> dict: "zkey" [c_rows, c_cols] uint64, "depth" uint16, "src_index" uint32 (SRC_NONE = nothing landed),
    "counts" [4] uint32. Every output may also be an array of its shape to write into; zkey is made all the same."""
    who = "register_depth_host"
    (k_d, k_c), _, pose = _front_cameras(who, (dcam5, ccam5), None, pose7)
    d = np.ascontiguousarray(depth, np.uint16)
    if d.ndim != 2:
        raise VorsError(f"{who}: depth [d_rows, d_cols]")
    oshape = (max(int(c_rows), 0), max(int(c_cols), 0))
    bufs = (_host_out(who, zkey if _asked(zkey) else True, oshape, np.uint64), _host_out(who, depth_out, oshape, np.uint16),
            _host_out(who, src_index, oshape, np.uint32), _host_out(who, counts, (REGISTER_COUNTS,), np.uint32, fill=0))
    _check(lib().vors_register_depth_host(_ptr(d), _ptr(k_d), d.shape[0], d.shape[1], float(depth_scale_in), _ptr(pose), _ptr(k_c), int(c_rows),
                                          int(c_cols), float(depth_scale_out), int(footprint), *[_ptr(b) for b in bufs]))
    return _result(*((name, want, t) for name, want, t in zip(("zkey", "depth", "src_index", "counts"),
                                                               (True, _asked(depth_out), _asked(src_index), _asked(counts)), bufs)))


class vors_icp_stats(C.Structure):
    _fields_ = [("status", C.c_uint32), ("iterations", C.c_uint32), ("considered", C.c_uint32), ("matched", C.c_uint32), ("rms", C.c_float),
                ("last_step_norm", C.c_float)]


ICP_STATS_DTYPE = np.dtype([("status", "<u4"), ("iterations", "<u4"), ("considered", "<u4"), ("matched", "<u4"), ("rms", "<f4"),
                            ("last_step_norm", "<f4")])
assert ICP_STATS_DTYPE.itemsize == C.sizeof(vors_icp_stats) == 24


def decode_icp_stats(stats):
    """The "stats" tensor of icp_points() ([n, 24] uint8: the vors_icp_stats records as bytes) -> a structured numpy array [n]."""
    return np.ascontiguousarray(stats.cpu().numpy()).view(ICP_STATS_DTYPE).reshape(-1)


def icp_workspace_bytes(n, capacity):
    """Bytes of the workspace icp_points() needs for n lists of `capacity` (vors_icp_workspace_bytes)."""
    return int(lib().vors_icp_workspace_bytes(int(n), int(capacity)))


def _icp_buffers(n, cap, dev, workspace, stats, sums29, residuals):
    """The workspace (None = a new one) and the output arguments of an ICP pass (_out_buf) -> (workspace, (poses, stats, sums29, residuals))."""
    import torch
    need = icp_workspace_bytes(n, cap)
    if workspace is None:
        workspace = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise VorsError(f"icp: expected a contiguous uint8 workspace of at least {need} bytes")
    bufs = (torch.empty((n, 7), dtype=torch.float32, device=dev), _out_buf(stats, (n, ICP_STATS_DTYPE.itemsize), torch.uint8, dev),
            _out_buf(sums29, (n, 29), torch.float32, dev), _out_buf(residuals, (n, cap), torch.float32, dev))
    if residuals is True:
        bufs[3].fill_(float("nan"))
    return workspace, bufs


def _icp_result(bufs, stats, sums29, residuals):
    return _result(("poses", True, bufs[0]), ("stats", _asked(stats), bufs[1]), ("sums29", _asked(sums29), bufs[2]),
                   ("residuals", _asked(residuals), bufs[3]))


def icp_points(xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping=0.0, step_eps=1e-5, iters=8, min_points=6,
               ranges=None, workspace=None, stats=True, sums29=False, residuals=False):
    """Point-to-plane ICP of n world-frame point lists with normals against one level-0 depth plane each (vors_icp_points; handle-free)
    -> dict of tensors on the current stream, not synchronised: "poses" [n, 7] float32, the refined camera -> world poses; "stats"
    [n, 24] uint8 (the vors_icp_stats records as bytes: decode_icp_stats()); "sums29" [n, 29] float32 of the final evaluation (the layout
    of Batch.eval_level, for pose_information_from_sums); "residuals" [n, capacity] float32, NaN = not matched, exactly the ranks of each
    list's clipped range written (a new tensor is filled with NaN first). xyz / normals [n, capacity, 3] float32 and list_counts [n] int32:
    the tensors of Trackers.map() / map_normals() or Batch.point_cloud() / points_normals(). depth [n, rows, cols] int16 tensor holding
    the u16 payload; poses [n, 7] float32 (or a track's out_stats bytes), required; ranges: see _render_ranges. iters = 0 evaluates at
    the given poses. workspace: a uint8 tensor of icp_workspace_bytes(n, capacity) to reuse (None = a new one). stats / sums29 /
    residuals may also be a tensor of that shape to write into."""
    return _icp_device("icp_points", xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping, step_eps, iters, min_points,
                       ranges, workspace, stats, sums29, residuals)


def _icp_pass(who, n, cap, depth, dev, workspace, stats, sums29, residuals, robust, joint):
    """What the handle-free and the Trackers forms of a device pass share behind their own checks: the workspace, the output tensors and
    what a form adds. robust: None or (frame_normals, min_cos, huber_m, gate_counts); joint (with robust): None or (list_gray, frame_gray,
    photo_scale_m, photo_huber_grey, photo_residuals, photo_counts) -> (workspace, the form's C arguments behind min_points, the C
    arguments from the workspace to the last output, the result dict)."""
    ws, bufs = _icp_buffers(n, cap, dev, workspace, stats, sums29, residuals)
    more_in, outs, result = [], list(bufs), _icp_result(bufs, stats, sums29, residuals)
    if robust is not None:
        frame_normals, min_cos, huber_m, gate_counts = robust
        gates = _icp_robust_buffers(who, frame_normals, depth.shape, gate_counts, dev)
        more_in += [Batch._dp(frame_normals), float(min_cos), float(huber_m)]
        outs.append(gates)
        result.update(_result(("gate_counts", _asked(gate_counts), gates)))
    if joint is not None:
        list_gray, frame_gray, photo_scale_m, photo_huber_grey, photo_residuals, photo_counts = joint
        photo = _icp_joint_buffers(who, list_gray, frame_gray, depth.shape, cap, photo_residuals, photo_counts, dev)
        more_in += [float(photo_scale_m), float(photo_huber_grey)]
        outs += photo
        result.update(_result(("photo_residuals", _asked(photo_residuals), photo[0]), ("photo_counts", _asked(photo_counts), photo[1])))
    return ws, more_in, [Batch._dp(t) for t in [ws] + outs], result


def _icp_device(who, xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping, step_eps, iters, min_points, ranges, workspace,
                stats, sums29, residuals, robust=None, joint=None):
    """The body of icp_points(), icp_points_robust() and icp_points_joint(): vors_<who>. robust, joint: see _icp_pass."""
    import torch
    n = xyz.shape[0]
    cap = xyz.shape[1] if xyz.dim() == 3 else -1
    if (xyz.dtype != torch.float32 or not xyz.is_contiguous() or xyz.dim() != 3 or xyz.shape[2] != 3 or normals.dtype != torch.float32
            or not normals.is_contiguous() or tuple(normals.shape) != (n, cap, 3) or list_counts.dtype != torch.int32
            or not list_counts.is_contiguous() or tuple(list_counts.shape) != (n,)):
        raise VorsError(f"{who}: xyz and normals float32 [n, capacity, 3], list_counts int32 [n], contiguous")
    if depth.dtype != torch.int16 or depth.dim() != 3 or depth.shape[0] != n or not depth.is_contiguous():
        raise VorsError(f"{who}: depth int16 [n, rows, cols], contiguous")
    if poses is None:
        raise VorsError(f"{who}: poses are required")
    k = _normals_common(cam5, who)
    poses, pose_stride = _render_poses(poses, n)
    rng, range_stride = _render_ranges(ranges, n)
    _, more_in, outs, result = _icp_pass(who, n, cap, depth, xyz.device, workspace, stats, sums29, residuals, robust, joint)
    list_gray, frame_gray = ([], []) if joint is None else ([Batch._dp(joint[0])], [Batch._dp(joint[1])])
    _check(getattr(lib(), "vors_" + who)(n, Batch._dp(xyz), Batch._dp(normals), *list_gray, Batch._dp(list_counts), cap, rng, range_stride,
                                         Batch._dp(poses), pose_stride, Batch._dp(depth), *frame_gray, _ptr(k), depth.shape[1], depth.shape[2],
                                         float(depth_scale), float(dist_m), float(damping), float(step_eps), int(iters), int(min_points), *more_in,
                                         *outs, Batch._stream()))
    return result


def _icp_host(who, xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping, step_eps, iters, min_points, count, range2, residuals,
              robust=None, joint=None):
    """The body of icp_points_host(), icp_points_robust_host() and icp_points_joint_host(): vors_<who>. robust: None or (frame_normals,
    min_cos, huber_m); joint (with robust): None or (list_gray, frame_gray, photo_scale_m, photo_huber_grey, photo_residuals)."""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nn = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(depth, np.uint16)
    k = np.ascontiguousarray(cam5, np.float32)
    pose = None if pose7 is None else np.ascontiguousarray(pose7, np.float32)
    rng = None if range2 is None else np.ascontiguousarray(range2, np.uint32)
    bad = len(p) != len(nn) or d.ndim != 2 or k.shape != (5,) or (pose is not None and pose.shape != (7,)) or (rng is not None and rng.shape != (2,))
    wanted = {"residuals": residuals}
    more_in, gray_shapes = [], ("", "")
    if robust is not None:
        fn = None if robust[0] is None else np.ascontiguousarray(robust[0], np.float32)
        bad = bad or (fn is not None and fn.shape != d.shape + (3,))
        more_in += [_ptr(fn), float(robust[1]), float(robust[2])]
    if joint is not None:
        lg = None if joint[0] is None else np.ascontiguousarray(joint[0], np.uint8).reshape(-1)
        fg = None if joint[1] is None else np.ascontiguousarray(joint[1], np.uint8)
        bad = bad or (lg is not None and len(lg) != len(p)) or (fg is not None and fg.shape != d.shape)
        more_in += [float(joint[2]), float(joint[3])]
        wanted["photo_residuals"] = joint[4]
        gray_shapes = ("list_gray [capacity] or None, ", "frame_gray [rows, cols] or None, ")
    if bad:
        raise VorsError(f"{who}: xyz and normals [capacity, 3], {gray_shapes[0]}depth [rows, cols], {gray_shapes[1]}cam5 [5], pose7 [7], "
                        f"range2 [2] or None{'' if robust is None else ', frame_normals [rows, cols, 3] or None'}")
    for name, given in wanted.items():
        if given is None:
            given = np.full(len(p), np.nan, np.float32)
        elif given.dtype != np.float32 or given.shape != (len(p),) or not given.flags.c_contiguous:
            raise VorsError(f"{who}: {name} must be a contiguous float32 array ({len(p)},)")
        wanted[name] = given
    stats = np.zeros(1, ICP_STATS_DTYPE)
    out = dict(pose=np.zeros(7, np.float32), stats=stats[0], sums29=np.zeros(29, np.float32), residuals=wanted["residuals"])
    if robust is not None:
        out["gate_counts"] = np.zeros(ICP_GATE_COUNTS, np.uint32)
    if joint is not None:
        out.update(photo_residuals=wanted["photo_residuals"], photo_counts=np.zeros(ICP_PHOTO_COUNTS, np.uint32))
    list_gray, frame_gray = ([], []) if joint is None else ([_ptr(lg) if lg is not None and len(lg) else None], [_ptr(fg)])
    _check(getattr(lib(), "vors_" + who)(_ptr(p) if len(p) else None, _ptr(nn) if len(nn) else None, *list_gray,
                                         len(p) if count is None else int(count), len(p), _ptr(rng), _ptr(pose), _ptr(d), *frame_gray, _ptr(k),
                                         d.shape[0], d.shape[1], float(depth_scale), float(dist_m), float(damping), float(step_eps), int(iters),
                                         int(min_points), *more_in, _ptr(out["pose"]), _ptr(stats),
                                         *[_ptr(a) for name, a in out.items() if name not in ("pose", "stats")]))
    return out


# ----------------------------------------------------------------------------------------------- pose-graph optimisation
PG_ITERATIONS, PG_CONVERGED, PG_TOO_FEW, PG_SINGULAR = range(4)  # VORS_PG_*
PG_STATS_DTYPE = np.dtype([("status", "<u4"), ("accepted_steps", "<u4"), ("rejected_steps", "<u4"), ("cg_iterations", "<u4"),
                           ("valid_edges", "<u4"), ("skipped_edges", "<u4"), ("free_nodes", "<u4"), ("fixed_nodes", "<u4"),
                           ("isolated_nodes", "<u4"), ("initial_energy", "<f4"), ("final_energy", "<f4"), ("last_step_norm", "<f4"),
                           ("final_lambda", "<f4")])
assert PG_STATS_DTYPE.itemsize == 52


def decode_pose_graph_stats(stats):
    """The "stats" tensor of pose_graph_optimize() ([n, 52] uint8: the vors_pose_graph_stats records as bytes) -> a structured array [n]."""
    return np.ascontiguousarray(stats.cpu().numpy()).view(PG_STATS_DTYPE).reshape(-1)


def pose_graph_workspace_bytes(n, node_capacity, edge_capacity):
    """Bytes of the workspace pose_graph_optimize() needs (vors_pose_graph_workspace_bytes)."""
    return int(lib().vors_pose_graph_workspace_bytes(int(n), int(node_capacity), int(edge_capacity)))


def pose_graph_optimize(poses, node_counts, edges, edge_counts, meas, info=None, edge_weight=None, fixed=None, lambda0=1e-4, step_eps=1e-6,
                        cg_tol=1e-6, iters=8, cg_iters=32, workspace=None, stats=True, edge_residuals=False, edge_energy=False, out=None):
    """Pose-graph optimisation of n graphs side by side (vors_pose_graph_optimize; handle-free) -> dict of tensors on the current stream,
    not synchronised: "poses" [n, node_capacity, 7] float32 (exactly the nodes of each graph written; a new tensor starts as a copy of the
    input poses), "stats" [n, 52] uint8 (decode_pose_graph_stats()), "edge_residuals" [n, edge_capacity, 6] and "edge_energy"
    [n, edge_capacity] float32 of the final evaluation, NaN for a skipped edge (a new tensor is filled with NaN first). poses
    [n, node_capacity, >= 7] float32 camera -> world, the last dimension's stride 1 and the others those of a contiguous tensor (a wider
    last dimension is the pose stride); node_counts / edge_counts [n] int32; edges [n, edge_capacity, 2] int32 (i, j); meas
    [n, edge_capacity, 7] float32: M_ij maps camera i's coordinates into camera j's (a track's lm_model of keyframe i and frame j); info
    [n, edge_capacity, 36] float32 or None (identity); edge_weight [n, edge_capacity] float32 or None; fixed [n, node_capacity] uint8 or
    None (node 0 of every graph). iters = 0 evaluates. workspace: a uint8 tensor of pose_graph_workspace_bytes() to reuse; out: a
    [n, node_capacity, 7] tensor for the poses (may be `poses` itself when that is packed); stats / edge_residuals / edge_energy may also
    be a tensor of that shape to write into."""
    import torch
    who = "pose_graph_optimize"
    if poses.dtype != torch.float32 or poses.dim() != 3 or poses.shape[2] < 7 or not poses.is_contiguous():
        raise VorsError(f"{who}: poses float32 [n, node_capacity, >= 7], contiguous")
    n, ncap, width = poses.shape
    ecap = edges.shape[1] if edges.dim() == 3 else -1
    dev = poses.device
    for name, t, dtype, shape in (("node_counts", node_counts, torch.int32, (n,)), ("edge_counts", edge_counts, torch.int32, (n,)),
                                  ("edges", edges, torch.int32, (n, ecap, 2)), ("meas", meas, torch.float32, (n, ecap, 7)),
                                  ("info", info, torch.float32, (n, ecap, 36)), ("edge_weight", edge_weight, torch.float32, (n, ecap)),
                                  ("fixed", fixed, torch.uint8, (n, ncap))):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise VorsError(f"{who}: {name} must be a contiguous {dtype} tensor {shape} on the poses' device")
    need = pose_graph_workspace_bytes(n, ncap, ecap)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise VorsError(f"{who}: expected a contiguous uint8 workspace of at least {need} bytes")
    if out is None:
        out = poses[:, :, :7].contiguous() if width != 7 else poses.clone()
    elif out.dtype != torch.float32 or tuple(out.shape) != (n, ncap, 7) or not out.is_contiguous():
        raise VorsError(f"{who}: out must be a contiguous float32 tensor ({n}, {ncap}, 7)")
    bufs = (_out_buf(stats, (n, PG_STATS_DTYPE.itemsize), torch.uint8, dev), _out_buf(edge_residuals, (n, ecap, 6), torch.float32, dev),
            _out_buf(edge_energy, (n, ecap), torch.float32, dev))
    if edge_residuals is True:
        bufs[1].fill_(float("nan"))
    if edge_energy is True:
        bufs[2].fill_(float("nan"))
    dp = Batch._dp
    _check(lib().vors_pose_graph_optimize(n, dp(poses), 0 if width == 7 else 4 * width, dp(node_counts), ncap, dp(edges), dp(edge_counts), ecap,
                                          dp(meas), dp(info), dp(edge_weight), dp(fixed), float(lambda0), float(step_eps), float(cg_tol),
                                          int(iters), int(cg_iters), dp(workspace), dp(out), dp(bufs[0]), dp(bufs[1]), dp(bufs[2]),
                                          Batch._stream()))
    return _result(("poses", True, out), ("stats", _asked(stats), bufs[0]), ("edge_residuals", _asked(edge_residuals), bufs[1]),
                   ("edge_energy", _asked(edge_energy), bufs[2]))


def pose_graph_optimize_host(poses, edges, meas, info=None, edge_weight=None, fixed=None, lambda0=1e-4, step_eps=1e-6, cg_tol=1e-6, iters=8,
                             cg_iters=32, node_count=None, edge_count=None):
    """The loop of pose_graph_optimize for ONE graph on the host (vors_pose_graph_optimize_host; needs no GPU; the texts and the order of
    sums the kernels run): poses [node_capacity, 7], edges [edge_capacity, 2], meas [edge_capacity, 7], info [edge_capacity, 36] or None,
    edge_weight [edge_capacity] or None, fixed [node_capacity] or None; node_count / edge_count: None = the capacities -> dict: "poses"
    (starts as a copy of the input), "stats" (a PG_STATS_DTYPE record), "edge_residuals" [edge_capacity, 6] and "edge_energy"
    [edge_capacity] float32 (NaN where not written or skipped)."""
    who = "pose_graph_optimize_host"
    p = np.ascontiguousarray(poses, np.float32)
    e = np.ascontiguousarray(edges, np.uint32)
    m = np.ascontiguousarray(meas, np.float32)
    om = None if info is None else np.ascontiguousarray(info, np.float32)
    w = None if edge_weight is None else np.ascontiguousarray(edge_weight, np.float32)
    fx = None if fixed is None else np.ascontiguousarray(fixed, np.uint8)
    if (p.ndim != 2 or p.shape[1] != 7 or e.ndim != 2 or e.shape[1] != 2 or m.shape != (len(e), 7) or (om is not None and om.shape != (len(e), 36))
            or (w is not None and w.shape != (len(e),)) or (fx is not None and fx.shape != (len(p),))):
        raise VorsError(f"{who}: poses [node_capacity, 7], edges [edge_capacity, 2], meas [edge_capacity, 7], info [edge_capacity, 36] or "
                        "None, edge_weight [edge_capacity] or None, fixed [node_capacity] or None")
    stats = np.zeros(1, PG_STATS_DTYPE)
    out = dict(poses=p.copy(), stats=stats[0], edge_residuals=np.full((len(e), 6), np.nan, np.float32),
               edge_energy=np.full(len(e), np.nan, np.float32))
    some = lambda a: _ptr(a) if a is not None and a.size else None  # noqa: E731
    _check(lib().vors_pose_graph_optimize_host(some(p), len(p) if node_count is None else int(node_count), len(p), some(e),
                                               len(e) if edge_count is None else int(edge_count), len(e), some(m), some(om), some(w), some(fx),
                                               float(lambda0), float(step_eps), float(cg_tol), int(iters), int(cg_iters), some(out["poses"]),
                                               _ptr(stats), some(out["edge_residuals"]), some(out["edge_energy"])))
    return out


def pose_graph_jacobians_host(ti7, tj7, meas7):
    """The residual and the closed-form Jacobians of one edge at the poses (ti, tj) (vors_pose_graph_jacobians_host; the kernels' own text)
    -> (r [6], J_i [6, 6], J_j [6, 6]) float32, for the perturbation T_k <- T_k exp(d_k), d in se3_exp's (v, w) order."""
    a = [np.ascontiguousarray(v, np.float32).reshape(7) for v in (ti7, tj7, meas7)]
    r, ji, jj = np.zeros(6, np.float32), np.zeros((6, 6), np.float32), np.zeros((6, 6), np.float32)
    lib().vors_pose_graph_jacobians_host(*[_ptr(v) for v in a], _ptr(r), _ptr(ji), _ptr(jj))
    return r, ji, jj


# ----------------------------------------------------------------------------------------------- loop closure
LOOP_MAX_K, LOOP_COUNTS, LOOP_VERDICTS = 8, 5, 9  # VORS_LOOP_MAX_K, VORS_LOOP_COUNTS, VORS_LOOP_VERDICTS
(LOOP_ACCEPTED, LOOP_STATUS, LOOP_INDEX, LOOP_NONFINITE, LOOP_CYCLE_TRANS, LOOP_CYCLE_ROT, LOOP_PRIOR_TRANS, LOOP_PRIOR_ROT,
 LOOP_CAPACITY) = range(9)  # VORS_LOOP_*
LOOP_EMPTY = 0xFFFFFFFF
LOOP_META_DTYPE = np.dtype([("sum", "<i4"), ("sumsq", "<u4")])       # vors_loop_sig_meta
LOOP_CAND_DTYPE = np.dtype([("i", "<u4"), ("score", "<f4")])         # vors_loop_candidate


def loop_signatures(gray, tr, tc, sig=None, meta=None, at=0):
    """Thumbnail signatures of n grey planes (vors_loop_signatures; handle-free, on the current stream, not synchronised) -> dict: "sig"
    int8 [n or capacity, tr * tc] and "meta" int32 [n or capacity, 2] (sum, sumsq; the bytes of vors_loop_sig_meta). gray uint8
    [n, rows, cols] contiguous. sig / meta: existing [capacity, D] / [capacity, 2] tensors to write rows [at, at + n) of — keyframes
    appended as they are promoted; the other rows keep their bits."""
    import torch
    who = "loop_signatures"
    if gray.dtype != torch.uint8 or gray.dim() != 3 or not gray.is_contiguous():
        raise VorsError(f"{who}: gray uint8 [n, rows, cols], contiguous")
    n, rows, cols = gray.shape
    d = int(tr) * int(tc)
    if sig is None:
        sig = torch.empty((at + n, d), dtype=torch.int8, device=gray.device)
    if meta is None:
        meta = torch.empty((at + n, 2), dtype=torch.int32, device=gray.device)
    if (sig.dtype != torch.int8 or sig.dim() != 2 or sig.shape[1] != d or not sig.is_contiguous() or meta.dtype != torch.int32
            or tuple(meta.shape) != (sig.shape[0], 2) or not meta.is_contiguous() or at < 0 or at + n > sig.shape[0]):
        raise VorsError(f"{who}: sig int8 [capacity, {d}] and meta int32 [capacity, 2], contiguous, with rows [at, at + n) inside")
    _check(lib().vors_loop_signatures(n, Batch._dp(gray), rows, cols, int(tr), int(tc), C.c_void_p(sig.data_ptr() + at * d),
                                      C.c_void_p(meta.data_ptr() + at * 8), Batch._stream()))
    return dict(sig=sig, meta=meta)


def loop_signatures_host(gray, tr, tc):
    """The signature of ONE plane on the host (vors_loop_signatures_host; needs no GPU) -> (sig int8 [tr * tc], sum, sumsq)."""
    g = np.ascontiguousarray(gray, np.uint8)
    if g.ndim != 2:
        raise VorsError("loop_signatures_host: gray uint8 [rows, cols]")
    sig = np.zeros(max(int(tr) * int(tc), 1), np.int8)
    meta = np.zeros(1, LOOP_META_DTYPE)
    _check(lib().vors_loop_signatures_host(_ptr(g), g.shape[0], g.shape[1], int(tr), int(tc), _ptr(sig), _ptr(meta)))
    return sig, int(meta[0]["sum"]), int(meta[0]["sumsq"])


def loop_candidates(sig, meta, counts_in, min_gap, k, min_score, poses=None, max_dist_m=0.0, min_qdot=0.0, query_first=None, counts=True,
                    cand=None, cand_counts=None):
    """All-pairs ZNCC of signatures, gated, the best k per query (vors_loop_candidates; handle-free, on the current stream, not
    synchronised) -> dict: "cand_i" int32 [n, capacity, k] (-1 = unused) and "cand_score" float32 [n, capacity, k] — views of ONE
    [n, capacity, k, 2] int32 tensor "cand", the vors_loop_candidate records —, "cand_counts" int32 [n, capacity], "counts" int32 [n, 5]
    (examined, flat, pose-gated, score-gated, survivors). Only the queries in [query_first, count) of each set are written; new tensors
    start as unused slots and zero counts. sig int8 [n, capacity, D], meta int32 [n, capacity, 2], counts_in int32 [n]; poses float32
    [n, capacity, >= 7] camera -> world or None; query_first int32 [n] or None."""
    import torch
    who = "loop_candidates"
    if sig.dtype != torch.int8 or sig.dim() != 3 or not sig.is_contiguous():
        raise VorsError(f"{who}: sig int8 [n, capacity, D], contiguous")
    n, cap, d = sig.shape
    dev = sig.device
    width = poses.shape[2] if poses is not None and poses.dim() == 3 else 7
    for name, t, dtype, shape in (("meta", meta, torch.int32, (n, cap, 2)), ("counts_in", counts_in, torch.int32, (n,)),
                                  ("poses", poses, torch.float32, (n, cap, width)), ("query_first", query_first, torch.int32, (n,))):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise VorsError(f"{who}: {name} must be a contiguous {dtype} tensor {shape} on the signatures' device")
    kk = max(int(k), 1)
    if cand is None:
        cand = torch.zeros((n, cap, kk, 2), dtype=torch.int32, device=dev)
        cand[..., 0] = -1
    if cand_counts is None:
        cand_counts = torch.zeros((n, cap), dtype=torch.int32, device=dev)
    if (cand.dtype != torch.int32 or tuple(cand.shape) != (n, cap, kk, 2) or not cand.is_contiguous() or cand_counts.dtype != torch.int32
            or tuple(cand_counts.shape) != (n, cap) or not cand_counts.is_contiguous()):
        raise VorsError(f"{who}: cand int32 ({n}, {cap}, {kk}, 2) and cand_counts int32 ({n}, {cap}), contiguous")
    cbuf = _out_buf(counts, (n, LOOP_COUNTS), torch.int32, dev)
    dp = Batch._dp
    _check(lib().vors_loop_candidates(n, dp(sig), dp(meta), dp(counts_in), cap, d, dp(poses), 0 if width == 7 else 4 * width, dp(query_first),
                                      int(min_gap), int(k), float(min_score), float(max_dist_m), float(min_qdot), dp(cand), dp(cand_counts),
                                      dp(cbuf), Batch._stream()))
    return _result(("cand", True, cand), ("cand_i", True, cand[..., 0]), ("cand_score", True, cand[..., 1].view(torch.float32)),
                   ("cand_counts", True, cand_counts), ("counts", _asked(counts), cbuf))


def loop_candidates_host(sig, meta, min_gap, k, min_score, poses=None, max_dist_m=0.0, min_qdot=0.0, query_first=0, count=None):
    """The same for ONE set on the host (vors_loop_candidates_host; needs no GPU): sig int8 [capacity, D], meta [capacity, 2] (sum,
    sumsq), poses [capacity, 7] or None; count: None = the capacity -> dict: "cand" (a LOOP_CAND_DTYPE array [capacity, k], unused
    slots (0xFFFFFFFF, 0)), "cand_counts" uint32 [capacity], "counts" uint32 [5]."""
    s = np.ascontiguousarray(sig, np.int8)
    m = np.ascontiguousarray(meta, np.int32)
    p = None if poses is None else np.ascontiguousarray(poses, np.float32)
    if s.ndim != 2 or m.shape != (len(s), 2) or (p is not None and p.shape != (len(s), 7)):
        raise VorsError("loop_candidates_host: sig int8 [capacity, D], meta [capacity, 2], poses [capacity, 7] or None")
    kk = max(int(k), 1)
    cand = np.zeros((len(s), kk), LOOP_CAND_DTYPE)
    cand["i"] = LOOP_EMPTY
    out = dict(cand=cand, cand_counts=np.zeros(len(s), np.uint32), counts=np.zeros(LOOP_COUNTS, np.uint32))
    _check(lib().vors_loop_candidates_host(_ptr(s), _ptr(m), len(s) if count is None else int(count), len(s), s.shape[1], _ptr(p),
                                           int(query_first), int(min_gap), int(k), float(min_score), float(max_dist_m), float(min_qdot),
                                           _ptr(cand), _ptr(out["cand_counts"]), _ptr(out["counts"])))
    return out


def loop_verify_edges(pairs, model_fwd, status_fwd, edges, meas, edge_count, model_bwd=None, status_bwd=None, info=None, poses=None,
                      max_cycle_trans=0.0, max_cycle_rot=0.0, max_prior_trans=0.0, max_prior_rot=0.0, weight=1.0, info_out=None,
                      edge_weight=None, residuals=True, counts=True):
    """From tracked loop candidates to pose-graph edges (vors_loop_verify_edges; handle-free, on the current stream, not synchronised):
    the accepted candidates are appended in candidate order to edges [edge_capacity, 2] int32, meas [edge_capacity, 7], info_out
    [edge_capacity, 36] and edge_weight [edge_capacity] float32 (the last two optional) from edge_count[0] (int32 [1], in / out) on —
    the tensors pose_graph_optimize takes -> dict: "verdict" int32 [m] (LOOP_*), "residuals" float32 [m, 12], "counts" int32 [9].
    pairs int32 [m, 2]; model_fwd / model_bwd float32 [m, >= 7] (row stride = the width: the lm_model columns of a stats tensor go in
    as a [m, width] view whose first 7 columns are the model); status_* int32 [m]; info float32 [m, 36]; poses float32
    [node_count, >= 7] camera -> world."""
    import torch
    who = "loop_verify_edges"
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise VorsError(f"{who}: pairs int32 [m, 2], contiguous")
    m, dev = pairs.shape[0], pairs.device

    def rows(name, t, least):  # a float32 [*, >= least] matrix whose rows are `width` floats apart -> its stride in bytes (0 = packed)
        if t is None:
            return 0
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < least or t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.device != dev:
            raise VorsError(f"{who}: {name} must be a float32 [rows, >= {least}] tensor with unit column stride on the pairs' device")
        return 0 if t.stride(0) == least else 4 * t.stride(0)

    fwd_bytes, bwd_bytes, pose_bytes = rows("model_fwd", model_fwd, 7), rows("model_bwd", model_bwd, 7), rows("poses", poses, 7)
    ecap = edges.shape[0]
    for name, t, dtype, shape in (("status_fwd", status_fwd, torch.int32, (m,)), ("status_bwd", status_bwd, torch.int32, (m,)),
                                  ("info", info, torch.float32, (m, 36)), ("edges", edges, torch.int32, (ecap, 2)),
                                  ("meas", meas, torch.float32, (ecap, 7)), ("info_out", info_out, torch.float32, (ecap, 36)),
                                  ("edge_weight", edge_weight, torch.float32, (ecap,)), ("edge_count", edge_count, torch.int32, (1,))):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise VorsError(f"{who}: {name} must be a contiguous {dtype} tensor {shape} on the pairs' device")
    if model_fwd.shape[0] != m or (model_bwd is not None and model_bwd.shape[0] != m):
        raise VorsError(f"{who}: one model per pair")
    verdict = torch.empty(m, dtype=torch.int32, device=dev)
    rbuf, cbuf = _out_buf(residuals, (m, 12), torch.float32, dev), _out_buf(counts, (LOOP_VERDICTS,), torch.int32, dev)
    dp = Batch._dp
    _check(lib().vors_loop_verify_edges(m, dp(pairs), dp(model_fwd), fwd_bytes, dp(model_bwd), bwd_bytes, dp(status_fwd), dp(status_bwd),
                                        dp(info), dp(poses), pose_bytes, 0 if poses is None else poses.shape[0], float(max_cycle_trans),
                                        float(max_cycle_rot), float(max_prior_trans), float(max_prior_rot), float(weight), dp(edges), dp(meas),
                                        dp(info_out), dp(edge_weight), dp(edge_count), ecap, dp(verdict), dp(rbuf), dp(cbuf), Batch._stream()))
    return _result(("verdict", True, verdict), ("residuals", _asked(residuals), rbuf), ("counts", _asked(counts), cbuf))


def loop_verify_edges_host(pairs, model_fwd, status_fwd, edge_capacity, model_bwd=None, status_bwd=None, info=None, poses=None,
                           max_cycle_trans=0.0, max_cycle_rot=0.0, max_prior_trans=0.0, max_prior_rot=0.0, weight=1.0, edges=None, meas=None,
                           info_out=None, edge_weight=None, edge_count=0):
    """The same on the host (vors_loop_verify_edges_host; needs no GPU): pairs [m, 2], model_* [m, 7], status_* [m], info [m, 36], poses
    [node_count, 7]; edges / meas / info_out / edge_weight: the lists to append to from edge_count on (None = new ones of edge_capacity
    rows, filled with 0xFFFFFFFF and NaN) -> dict: "edges", "meas", "info", "edge_weight" (copies, appended to), "edge_count", "verdict"
    uint32 [m], "residuals" [m, 12], "counts" uint32 [9]."""
    pr = np.ascontiguousarray(pairs, np.uint32)
    mf = np.ascontiguousarray(model_fwd, np.float32)
    mb = None if model_bwd is None else np.ascontiguousarray(model_bwd, np.float32)
    sf = np.ascontiguousarray(status_fwd, np.int32)
    sb = None if status_bwd is None else np.ascontiguousarray(status_bwd, np.int32)
    om = None if info is None else np.ascontiguousarray(info, np.float32)
    ps = None if poses is None else np.ascontiguousarray(poses, np.float32)
    m, ecap = len(pr), max(int(edge_capacity), 0)
    if (pr.ndim != 2 or pr.shape[1] != 2 or mf.shape != (m, 7) or (mb is not None and mb.shape != (m, 7)) or sf.shape != (m,)
            or (sb is not None and sb.shape != (m,)) or (om is not None and om.shape != (m, 36)) or (ps is not None and (ps.ndim != 2 or ps.shape[1] != 7))):
        raise VorsError("loop_verify_edges_host: pairs [m, 2], models [m, 7], statuses [m], info [m, 36], poses [node_count, 7]")
    e = np.full((ecap, 2), LOOP_EMPTY, np.uint32) if edges is None else np.array(edges, np.uint32).reshape(ecap, 2)
    ms = np.full((ecap, 7), np.nan, np.float32) if meas is None else np.array(meas, np.float32).reshape(ecap, 7)
    io = np.full((ecap, 36), np.nan, np.float32) if info_out is None else np.array(info_out, np.float32).reshape(ecap, 36)
    ew = np.full(ecap, np.nan, np.float32) if edge_weight is None else np.array(edge_weight, np.float32).reshape(ecap)
    ec = np.array([edge_count], np.uint32)
    out = dict(edges=e, meas=ms, info=io, edge_weight=ew, verdict=np.full(m, 0xFFFFFFFF, np.uint32), residuals=np.full((m, 12), 7.5, np.float32),
               counts=np.full(LOOP_VERDICTS, 0xFFFFFFFF, np.uint32))
    some = lambda a: _ptr(a) if a is not None and a.size else None  # noqa: E731
    _check(lib().vors_loop_verify_edges_host(m, some(pr), some(mf), 0, some(mb), 0, some(sf), some(sb), some(om), some(ps), 0,
                                             0 if ps is None else len(ps), float(max_cycle_trans), float(max_cycle_rot), float(max_prior_trans),
                                             float(max_prior_rot), float(weight), some(e), some(ms), some(io), some(ew), _ptr(ec), int(edge_capacity),
                                             some(out["verdict"]), some(out["residuals"]), some(out["counts"])))
    out["edge_count"] = int(ec[0])
    return out


# ----------------------------------------------------------------------------------------------- the corrected map
REPOSE_COUNTS = 6  # VORS_REPOSE_COUNTS: points moved, kept, non-finite, without a record; segments moved; bits of the largest shift
REPOSE_NO_NODE = 0xFFFFFFFF  # a word of node_of_segment: this keyframe is not in the graph


def _repose_list_args(who, n, cap, nkf, dev, tensors):
    """(name, tensor or None, dtype, shape behind [n]) per argument: dtype, shape, contiguity and device, the way pose_graph_optimize
    checks its own."""
    for name, t, dtype, shape in tensors:
        if t is not None and (t.dtype != dtype or tuple(t.shape) != (n,) + shape or not t.is_contiguous() or t.device != dev):
            raise VorsError(f"{who}: {name} must be a contiguous {dtype} tensor {(n,) + shape} on the lists' device")


def _repose_poses(who, poses, n):
    import torch
    if poses.dtype != torch.float32 or poses.dim() != 3 or poses.shape[0] != n or poses.shape[2] < 7 or not poses.is_contiguous():
        raise VorsError(f"{who}: poses float32 [n, node_capacity, >= 7], contiguous")
    return poses.shape[1], (0 if poses.shape[2] == 7 else 4 * poses.shape[2])


def _repose_result(bufs, xyz_out, normals_out, segments_out, counts):
    return _result(("xyz", _asked(xyz_out), bufs[0]), ("normals", _asked(normals_out), bufs[1]), ("segments", _asked(segments_out), bufs[2]),
                   ("counts", _asked(counts), bufs[3]))


def repose_points(xyz, list_counts, segments, n_segments, poses, node_counts, normals=None, node_of_segment=None, xyz_out=True,
                  normals_out=None, segments_out=True, counts=True):
    """Re-pose n point lists after pose-graph optimisation (vors_repose_points; handle-free) -> dict of tensors on the current stream, not
    synchronised: "xyz" and "normals" [n, capacity, 3] float32 (exactly the ranks below min(count, capacity) written), "segments"
    [n, max_keyframes, 40] uint8 (the used records, pose7 replaced where the segment moved), "counts" [n, REPOSE_COUNTS] int32. xyz /
    normals [n, capacity, 3] float32, list_counts / n_segments / node_counts [n] int32, segments [n, max_keyframes, 40] uint8 — the tensors
    of Trackers.map() and map_normals(); poses [n, node_capacity, >= 7] float32, pose_graph_optimize()'s "poses" (a wider last dimension
    is the pose stride); node_of_segment [n, max_keyframes] int32 or None (segment k is node k; -1 = REPOSE_NO_NODE). Each output may be
    True (a new tensor: xyz / normals start as copies of the inputs, segments likewise), a tensor to write into — xyz, normals and
    segments themselves for in place — or False; normals_out None = True exactly when normals are given."""
    import torch
    who = "repose_points"
    if xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3 or not xyz.is_contiguous():
        raise VorsError(f"{who}: xyz float32 [n, capacity, 3], contiguous")
    n, cap, _ = xyz.shape
    nkf = segments.shape[1] if segments.dim() == 3 else -1
    dev = xyz.device
    _repose_list_args(who, n, cap, nkf, dev, (("normals", normals, torch.float32, (cap, 3)), ("list_counts", list_counts, torch.int32, ()),
                                              ("segments", segments, torch.uint8, (nkf, 40)), ("n_segments", n_segments, torch.int32, ()),
                                              ("node_counts", node_counts, torch.int32, ()),
                                              ("node_of_segment", node_of_segment, torch.int32, (nkf,))))
    ncap, stride = _repose_poses(who, poses, n)
    if normals_out is None:
        normals_out = normals is not None
    bufs = (xyz.clone() if xyz_out is True else _out_buf(xyz_out, (n, cap, 3), torch.float32, dev),
            normals.clone() if normals_out is True and normals is not None else _out_buf(normals_out, (n, cap, 3), torch.float32, dev),
            segments.clone() if segments_out is True else _out_buf(segments_out, (n, nkf, 40), torch.uint8, dev),
            _out_buf(counts, (n, REPOSE_COUNTS), torch.int32, dev))
    dp = Batch._dp
    _check(lib().vors_repose_points(n, dp(xyz), dp(normals), dp(list_counts), cap, dp(segments), dp(n_segments), nkf, dp(poses), stride, ncap,
                                    dp(node_counts), dp(node_of_segment), *[dp(t) for t in bufs], Batch._stream()))
    return _repose_result(bufs, xyz_out, normals_out, segments_out, counts)


def _segments_host(who, segments):
    """A list's records on the host: a MAP_SEGMENT_DTYPE array [k] or their bytes [k, 40] -> a contiguous structured array [k]."""
    a = np.asarray(segments)
    if a.dtype != MAP_SEGMENT_DTYPE:
        a = np.ascontiguousarray(a, np.uint8)
        if a.ndim != 2 or a.shape[1] != 40:
            raise VorsError(f"{who}: segments must be a MAP_SEGMENT_DTYPE array [k] or uint8 [k, 40]")
        a = a.view(MAP_SEGMENT_DTYPE)[:, 0]
    return np.ascontiguousarray(a.reshape(-1))


def repose_points_host(xyz, segments, poses, normals=None, node_of_segment=None, count=None, n_segments=None, node_count=None):
    """The rule of repose_points for ONE list on the host (vors_repose_points_host; needs no GPU; the texts the kernels run): xyz /
    normals [capacity, 3] float32, segments a MAP_SEGMENT_DTYPE array [max_keyframes], poses [node_capacity, 7] float32, node_of_segment
    [max_keyframes] uint32 or None; count / n_segments / node_count: None = the capacities (above them: clipped) -> dict: "xyz",
    "normals" (None without normals), "segments" (copies of the inputs, re-posed), "counts" uint32 [REPOSE_COUNTS]."""
    who = "repose_points_host"
    p = np.ascontiguousarray(xyz, np.float32)
    nm = None if normals is None else np.ascontiguousarray(normals, np.float32)
    sg = _segments_host(who, segments)
    ps = np.ascontiguousarray(poses, np.float32)
    nos = None if node_of_segment is None else np.ascontiguousarray(node_of_segment, np.uint32)
    if (p.ndim != 2 or p.shape[1] != 3 or (nm is not None and nm.shape != p.shape) or ps.ndim != 2 or ps.shape[1] != 7
            or (nos is not None and nos.shape != (len(sg),))):
        raise VorsError(f"{who}: xyz / normals [capacity, 3], poses [node_capacity, 7], node_of_segment [max_keyframes] or None")
    out = dict(xyz=p.copy(), normals=None if nm is None else nm.copy(), segments=sg.copy(), counts=np.zeros(REPOSE_COUNTS, np.uint32))
    some = lambda a: _ptr(a) if a is not None and a.size else None  # noqa: E731
    _check(lib().vors_repose_points_host(some(p), some(nm), len(p) if count is None else _u32("count", count), len(p), some(sg),
                                         len(sg) if n_segments is None else _u32("n_segments", n_segments), len(sg), some(ps),
                                         len(ps) if node_count is None else _u32("node_count", node_count), len(ps), some(nos),
                                         some(out["xyz"]), some(out["normals"]), some(out["segments"]), _ptr(out["counts"])))
    return out


def voxel_filter_workspace_bytes(n, capacity, table_slots):
    """Bytes of the workspace voxel_filter_points() needs (vors_voxel_filter_workspace_bytes); 0 for arguments the pass refuses."""
    return int(lib().vors_voxel_filter_workspace_bytes(int(n), int(capacity), int(table_slots)))


def voxel_filter_points(xyz, list_counts, voxel_m, table_slots, pixel=None, gray=None, normals=None, segments=None, n_segments=None,
                        workspace=None, xyz_out=True, index=True, counts=True, overflow=True, pixel_out=None, gray_out=None, normals_out=None,
                        segments_out=None):
    """One point per occupied voxel of n point lists, the first in each list's order (vors_voxel_filter_points; handle-free) -> dict of
    tensors on the current stream, not synchronised: "index" [n, capacity] int32 (the source rank of every kept entry), "counts" and
    "overflow" [n] int32, and the gathered "xyz" [n, capacity, 3], "pixel" [n, capacity] int32, "gray" [n, capacity] uint8, "normals"
    [n, capacity, 3] and "segments" [n, max_keyframes, 40] uint8 (first / count for the filtered list) of the inputs that are given.
    Entries at or beyond a list's count are not written. xyz [n, capacity, 3] float32, list_counts [n] int32; table_slots a power of two
    in 64..2^30 that is at least a list's distinct voxels (otherwise that list's overflow word is set and its outputs are unspecified).
    workspace: a uint8 tensor of voxel_filter_workspace_bytes() to reuse. An output may be True, a tensor to write into (never an input)
    or False; the gathered ones default to True exactly when their input is given."""
    import torch
    who = "voxel_filter_points"
    if xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3 or not xyz.is_contiguous():
        raise VorsError(f"{who}: xyz float32 [n, capacity, 3], contiguous")
    n, cap, _ = xyz.shape
    nkf = segments.shape[1] if segments is not None and segments.dim() == 3 else 0
    dev = xyz.device
    _repose_list_args(who, n, cap, nkf, dev, (("list_counts", list_counts, torch.int32, ()), ("pixel", pixel, torch.int32, (cap,)),
                                              ("gray", gray, torch.uint8, (cap,)), ("normals", normals, torch.float32, (cap, 3)),
                                              ("segments", segments, torch.uint8, (nkf, 40)), ("n_segments", n_segments, torch.int32, ())))
    pixel_out, gray_out, normals_out, segments_out = [given is not None if o is None else o for o, given in
                                                      ((pixel_out, pixel), (gray_out, gray), (normals_out, normals), (segments_out, segments))]
    need = voxel_filter_workspace_bytes(n, cap, int(table_slots))
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need:
        raise VorsError(f"{who}: expected a contiguous uint8 workspace of at least {need} bytes")
    bufs = (_out_buf(index, (n, cap), torch.int32, dev, always=True), _out_buf(counts, (n,), torch.int32, dev, always=True),
            _out_buf(overflow, (n,), torch.int32, dev, always=True), _out_buf(xyz_out, (n, cap, 3), torch.float32, dev),
            _out_buf(pixel_out, (n, cap), torch.int32, dev), _out_buf(gray_out, (n, cap), torch.uint8, dev),
            _out_buf(normals_out, (n, cap, 3), torch.float32, dev), _out_buf(segments_out, (n, nkf, 40), torch.uint8, dev))
    dp = Batch._dp
    _check(lib().vors_voxel_filter_points(n, dp(xyz), dp(list_counts), cap, float(voxel_m), int(table_slots), dp(workspace), dp(pixel), dp(gray),
                                          dp(normals), dp(segments), dp(n_segments), nkf, *[dp(t) for t in bufs], Batch._stream()))
    names = ("index", "counts", "overflow", "xyz", "pixel", "gray", "normals", "segments")
    asked = (index, counts, overflow, xyz_out, pixel_out, gray_out, normals_out, segments_out)
    return _result(*[(name, _asked(o), t) for name, o, t in zip(names, asked, bufs)])


def voxel_filter_points_host(xyz, voxel_m, table_slots=1 << 30, pixel=None, gray=None, normals=None, segments=None, count=None,
                             n_segments=None):
    """The rule of voxel_filter_points for ONE list on the host (vors_voxel_filter_points_host; needs no GPU): the first occurrence of
    every key of voxel_keys(). xyz [capacity, 3] float32, pixel [capacity] uint32, gray [capacity] uint8, normals [capacity, 3], segments
    a MAP_SEGMENT_DTYPE array; count / n_segments: None = the capacities -> dict: "count", "overflow" (1 when the distinct voxels exceed
    table_slots; the result is exact all the same), "index" uint32 [count], and "xyz", "pixel", "gray", "normals" [count, ...],
    "segments" of the inputs that are given."""
    who = "voxel_filter_points_host"
    p = np.ascontiguousarray(xyz, np.float32)
    px = None if pixel is None else np.ascontiguousarray(pixel, np.uint32)
    g = None if gray is None else np.ascontiguousarray(gray, np.uint8)
    nm = None if normals is None else np.ascontiguousarray(normals, np.float32)
    sg = None if segments is None else _segments_host(who, segments)
    if (p.ndim != 2 or p.shape[1] != 3 or (px is not None and px.shape != (len(p),)) or (g is not None and g.shape != (len(p),))
            or (nm is not None and nm.shape != p.shape)):
        raise VorsError(f"{who}: xyz / normals [capacity, 3], pixel / gray [capacity]")
    cap = len(p)
    like = lambda a: None if a is None else np.zeros_like(a)  # noqa: E731
    out = dict(index=np.zeros(cap, np.uint32), xyz=np.zeros_like(p), pixel=like(px), gray=like(g), normals=like(nm), segments=like(sg))
    kept, over = C.c_uint32(), C.c_uint32()
    some = lambda a: _ptr(a) if a is not None and a.size else None  # noqa: E731
    _check(lib().vors_voxel_filter_points_host(some(p), cap if count is None else _u32("count", count), cap, float(voxel_m), int(table_slots),
                                               some(px), some(g), some(nm), some(sg),
                                               0 if sg is None else (len(sg) if n_segments is None else _u32("n_segments", n_segments)),
                                               0 if sg is None else len(sg), some(out["index"]), C.byref(kept), C.byref(over), some(out["xyz"]),
                                               some(out["pixel"]), some(out["gray"]), some(out["normals"]), some(out["segments"])))
    k = kept.value
    out = {name: (a if name == "segments" else a[:k]) for name, a in out.items() if a is not None}
    out.update(count=k, overflow=over.value)
    return out


ICP_GATE_COUNTS = 4  # VORS_ICP_GATE_COUNTS: with_depth, within_dist, matched, huber_linear


class vors_map_icp_params(C.Structure):
    """Parameters of the map ICP correction at keyframe promotion (include/vors_hip.h vors_map_icp_params, 52 bytes)."""
    _fields_ = [("dist_m", C.c_float), ("damping", C.c_float), ("step_eps", C.c_float), ("iters", C.c_int32), ("min_points", C.c_int32),
                ("normal_gate", C.c_int32), ("min_cos", C.c_float), ("huber_m", C.c_float), ("last_keyframes", C.c_int32),
                ("min_match_ratio", C.c_float), ("max_rms", C.c_float), ("max_trans_m", C.c_float), ("max_rot_rad", C.c_float)]


class vors_map_icp_record(C.Structure):
    """What the correction keeps per sequence of the last track call (include/vors_hip.h vors_map_icp_record, 112 bytes)."""
    _fields_ = [("frame", C.c_int32), ("verdict", C.c_uint32), ("range_first", C.c_uint32), ("range_count", C.c_uint32),
                ("stats", vors_icp_stats), ("gate_counts", C.c_uint32 * ICP_GATE_COUNTS), ("pose_before", C.c_float * 7),
                ("pose_after", C.c_float * 7)]


MAP_ICP_RECORD_DTYPE = np.dtype([("frame", "<i4"), ("verdict", "<u4"), ("range_first", "<u4"), ("range_count", "<u4"), ("stats", ICP_STATS_DTYPE),
                                 ("gate_counts", "<u4", (ICP_GATE_COUNTS,)), ("pose_before", "<f4", (7,)), ("pose_after", "<f4", (7,))])
assert MAP_ICP_RECORD_DTYPE.itemsize == C.sizeof(vors_map_icp_record) == 112 and C.sizeof(vors_map_icp_params) == 52
MAP_ICP_NOT_ATTEMPTED, MAP_ICP_ACCEPTED, MAP_ICP_ICP_STATUS, MAP_ICP_FEW_MATCHES, MAP_ICP_RMS, MAP_ICP_STEP, MAP_ICP_NONFINITE = range(7)
# The defaults of every parameter but dist_m (the vors_track CLI documents the same): the ICP's as in icp_points_robust(), the frame-normal
# gate on at min_cos 0.9, the whole map as the window, and a verdict that asks for three matches in ten, 1 cm rms, and a correction of at
# most 5 cm and 0.05 rad.
MAP_ICP_DEFAULTS = dict(damping=0.0, step_eps=1e-5, iters=8, min_points=6, normal_gate=1, min_cos=0.9, huber_m=0.0, last_keyframes=0,
                        min_match_ratio=0.3, max_rms=0.01, max_trans_m=0.05, max_rot_rad=0.05)


def map_icp_params(dist_m=_REQUIRED, **params):
    """The vors_map_icp_params record of keyword arguments: dist_m is required, the rest defaults to MAP_ICP_DEFAULTS. Only names and types
    are judged here; the values are judged by the library, in one place for every caller."""
    if dist_m is _REQUIRED:
        raise VorsError("map_icp: dist_m is required")
    unknown = sorted(set(params) - set(MAP_ICP_DEFAULTS))
    if unknown:
        raise VorsError(f"map_icp: unknown parameter {unknown[0]!r} (dist_m, {', '.join(MAP_ICP_DEFAULTS)})")
    return _map_icp_fields(vors_map_icp_params(), "map_icp", vors_map_icp_params._fields_, dict(MAP_ICP_DEFAULTS, dist_m=dist_m, **params))


def _map_icp_fields(record, who, fields, values):
    """The field coercion of map_icp_params() and map_icp_joint_params(): every (name, C type) of `fields` set in `record` from values[name]
    — a number, an integer where the field is one, a bool only for normal_gate — refused in the name of `who` -> record."""
    for name, kind in fields:
        v = values[name]
        if isinstance(v, (bool, np.bool_)) and name == "normal_gate":
            v = int(v)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise VorsError(f"{who}: {name} must be a number, got {v!r}")
        if kind is C.c_int32:
            if not isinstance(v, (int, np.integer)) or not -2 ** 31 <= int(v) < 2 ** 31:
                raise VorsError(f"{who}: {name} must be an integer that fits a C int, got {v!r}")
            v = int(v)
        setattr(record, name, v)
    return record


def _map_icp_arg(spec):
    """Tracker(map_icp=...): None, a number (dist_m) or a dict of map_icp_params()' keywords -> None or the record."""
    if spec is None:
        return None
    if isinstance(spec, dict):
        return map_icp_params(**spec)
    return map_icp_params(dist_m=spec)


def decode_map_icp_records(records):
    """The "records" tensor of Trackers.map_icp() ([n, 112] uint8: the vors_map_icp_record records as bytes) -> a structured numpy array
    [n] of MAP_ICP_RECORD_DTYPE (its "stats" field is ICP_STATS_DTYPE)."""
    return _decode_records(records, MAP_ICP_RECORD_DTYPE)


def _decode_records(records, dtype):
    a = records.cpu().numpy() if hasattr(records, "cpu") else np.asarray(records)
    return np.ascontiguousarray(a).view(dtype).reshape(-1)


def map_icp_window_host(segments, n_segments, max_keyframes, count, capacity, last_keyframes):
    """The window rule of the map ICP correction on the host (vors_map_icp_window_host; needs no GPU): segments = the sequence's records
    (MAP_SEGMENT_DTYPE, at least min(n_segments, max_keyframes) of them, or None), n_segments / count its unclipped totals ->
    (first, count) of the ranks the new keyframe is aligned against."""
    seg = None if segments is None else np.ascontiguousarray(segments, MAP_SEGMENT_DTYPE).reshape(-1)
    if seg is not None and len(seg) < min(int(n_segments), int(max_keyframes)):
        raise VorsError("map_icp_window_host: fewer segment records than min(n_segments, max_keyframes)")
    out = np.zeros(2, np.uint32)
    _check(lib().vors_map_icp_window_host(_ptr(seg) if seg is not None and len(seg) else None, int(n_segments), int(max_keyframes), int(count),
                                          int(capacity), int(last_keyframes), _ptr(out)))
    return int(out[0]), int(out[1])


def map_icp_verdict_host(params, stats, pose_before, pose_after):
    """The verdict rule of the map ICP correction on the host (vors_map_icp_verdict_host; needs no GPU): params = map_icp_params(...) or
    a dict of its keywords (only the four verdict fields are read), stats = a structured scalar of ICP_STATS_DTYPE -> a MAP_ICP_* verdict."""
    return _map_icp_verdict("map_icp_verdict_host", map_icp_params, params, stats, pose_before, pose_after)


def _map_icp_verdict(who, build, params, stats, pose_before, pose_after, *dilutions):
    """The body of map_icp_verdict_host() and map_icp_verdict_joint_host(): vors_<who>; build: the parameter builder a dict goes through."""
    p = build(**params) if isinstance(params, dict) else params
    s = np.zeros(1, ICP_STATS_DTYPE)
    s[0] = stats
    a, b = np.ascontiguousarray(pose_before, np.float32), np.ascontiguousarray(pose_after, np.float32)
    if a.shape != (7,) or b.shape != (7,):
        raise VorsError(f"{who}: pose_before and pose_after [7]")
    v = C.c_uint32(99)
    _check(getattr(lib(), "vors_" + who)(C.byref(p), _ptr(s), _ptr(a), _ptr(b), *[float(x) for x in dilutions], C.byref(v)))
    return v.value


ICP_PHOTO_COUNTS = 2  # VORS_ICP_PHOTO_COUNTS: photo_used, photo_huber_linear


class vors_map_icp_joint_params(C.Structure):
    """Parameters of the correction through the joint pass with the condition test (include/vors_hip.h vors_map_icp_joint_params, 68 bytes)."""
    _fields_ = [("icp", vors_map_icp_params), ("photo_scale_m", C.c_float), ("photo_huber_grey", C.c_float), ("max_dilution_t", C.c_float),
                ("max_dilution_r", C.c_float)]


class vors_map_icp_joint_record(C.Structure):
    """What the joint stage keeps beside a vors_map_icp_record (include/vors_hip.h vors_map_icp_joint_record, 20 bytes)."""
    _fields_ = [("dilution_t", C.c_float), ("dilution_r", C.c_float), ("condition_flags", C.c_int32), ("photo_counts", C.c_uint32 * ICP_PHOTO_COUNTS)]


MAP_ICP_JOINT_RECORD_DTYPE = np.dtype([("dilution_t", "<f4"), ("dilution_r", "<f4"), ("condition_flags", "<i4"),
                                       ("photo_counts", "<u4", (ICP_PHOTO_COUNTS,))])
assert MAP_ICP_JOINT_RECORD_DTYPE.itemsize == C.sizeof(vors_map_icp_joint_record) == 20 and C.sizeof(vors_map_icp_joint_params) == 68
MAP_ICP_CONDITION = 7
# The defaults of the joint stage's own parameters: no photometric row (the robust pass) and both bounds off — vors_trackers_enable_map_icp's
# behaviour, with the dilutions recorded.
MAP_ICP_JOINT_DEFAULTS = dict(photo_scale_m=0.0, photo_huber_grey=0.0, max_dilution_t=0.0, max_dilution_r=0.0)


def map_icp_joint_params(dist_m=_REQUIRED, **params):
    """The vors_map_icp_joint_params record of keyword arguments: map_icp_params()' keywords and MAP_ICP_JOINT_DEFAULTS'. Only names and
    types are judged here; the values are judged by the library."""
    own = {k: params.pop(k) for k in list(params) if k in MAP_ICP_JOINT_DEFAULTS}
    p = vors_map_icp_joint_params()
    p.icp = map_icp_params(dist_m, **params)
    return _map_icp_fields(p, "map_icp_joint", vors_map_icp_joint_params._fields_[1:], dict(MAP_ICP_JOINT_DEFAULTS, **own))


def decode_map_icp_joint_records(records):
    """The tensor of Trackers.map_icp_joint() ([n, 20] uint8) -> a structured numpy array [n] of MAP_ICP_JOINT_RECORD_DTYPE."""
    return _decode_records(records, MAP_ICP_JOINT_RECORD_DTYPE)


class vors_map_icp_means_record(C.Structure):
    """What the averaged model keeps per sequence of the last track call (include/vors_hip.h vors_map_icp_means_record, 8 bytes)."""
    _fields_ = [("resolved", C.c_uint32), ("kept", C.c_uint32)]


MAP_ICP_MEANS_RECORD_DTYPE = np.dtype([("resolved", "<u4"), ("kept", "<u4")])
assert MAP_ICP_MEANS_RECORD_DTYPE.itemsize == C.sizeof(vors_map_icp_means_record) == 8


def decode_map_icp_means_records(records):
    """The bytes of vors_trackers_map_icp_means' records ([n, 8] uint8 tensor or array) -> a structured numpy array [n] of
    MAP_ICP_MEANS_RECORD_DTYPE."""
    return _decode_records(records, MAP_ICP_MEANS_RECORD_DTYPE)


def _map_icp_means_args(arg):
    """Tracker(map_icp_means=...): None, or (min_count[, min_span]) -> None or the two u32."""
    if arg is None:
        return None
    arg = tuple(arg) if isinstance(arg, (tuple, list)) else (arg,)
    if not 1 <= len(arg) <= 2:
        raise VorsError("map_icp_means: (min_count[, min_span])")
    return _u32("min_count", arg[0]), _u32("min_span", arg[1] if len(arg) > 1 else 0)


def icp_condition_from_sums(sums29):
    """The conditioning of one ICP system on the host (vors_icp_condition_from_sums; needs no GPU): sums29 [29] float32 of one evaluation
    (icp_points*()'s "sums29") -> (dilution_t, dilution_r, flags): numpy float32 scalars, NaN when flags != 0 (bit 0: at most 6 matched
    points, bit 1: H has no Cholesky factor)."""
    s = np.ascontiguousarray(sums29, np.float32)
    if s.shape != (29,):
        raise VorsError("icp_condition_from_sums: sums29 [29]")
    out = np.zeros(2, np.float32)
    fl = C.c_int32(0)
    _check(lib().vors_icp_condition_from_sums(_ptr(s), out[0:].ctypes.data_as(C.c_void_p), out[1:].ctypes.data_as(C.c_void_p), C.byref(fl)))
    return out[0], out[1], fl.value


def icp_condition(sums29, dilutions=None, flags=None):
    """The conditioning of n ICP systems on the device (vors_icp_condition; current stream, not synchronised): sums29 [n, 29] float32
    tensor -> (dilutions [n, 2] float32: dilution_t, dilution_r; flags [n] int32), the bits of icp_condition_from_sums(). dilutions /
    flags: tensors of that shape to write into (None = new ones)."""
    import torch
    if sums29.dtype != torch.float32 or sums29.dim() != 2 or sums29.shape[1] != 29 or not sums29.is_contiguous():
        raise VorsError("icp_condition: sums29 float32 [n, 29], contiguous")
    n = sums29.shape[0]
    if dilutions is None:
        dilutions = torch.empty((n, 2), dtype=torch.float32, device=sums29.device)
    if flags is None:
        flags = torch.empty(n, dtype=torch.int32, device=sums29.device)
    if (dilutions.dtype != torch.float32 or tuple(dilutions.shape) != (n, 2) or not dilutions.is_contiguous() or flags.dtype != torch.int32
            or tuple(flags.shape) != (n,) or not flags.is_contiguous()):
        raise VorsError("icp_condition: dilutions float32 [n, 2] and flags int32 [n], contiguous")
    _check(lib().vors_icp_condition(n, Batch._dp(sums29), Batch._dp(dilutions), Batch._dp(flags), Batch._stream()))
    return dilutions, flags


def map_icp_verdict_joint_host(params, stats, pose_before, pose_after, dilution_t, dilution_r):
    """The joint stage's verdict on the host (vors_map_icp_verdict_joint_host; needs no GPU): params = map_icp_joint_params(...) or a dict
    of its keywords (the four verdict fields and the two bounds are read), stats = a structured scalar of ICP_STATS_DTYPE -> a MAP_ICP_*
    verdict, MAP_ICP_CONDITION among them."""
    return _map_icp_verdict("map_icp_verdict_joint_host", map_icp_joint_params, params, stats, pose_before, pose_after, dilution_t, dilution_r)


def _icp_robust_buffers(who, frame_normals, shape, gate_counts, dev):
    """The frame normals (None = no normal gate; float32 [n, rows, cols, 3], contiguous) checked, and the tensor behind gate_counts."""
    import torch
    if frame_normals is not None and (frame_normals.dtype != torch.float32 or not frame_normals.is_contiguous()
                                      or tuple(frame_normals.shape) != tuple(shape) + (3,)):
        raise VorsError(f"{who}: frame_normals float32 {tuple(shape) + (3,)}, contiguous (depth_normals() of the same depth without poses)")
    return _out_buf(gate_counts, (shape[0], ICP_GATE_COUNTS), torch.int32, dev)


def icp_points_robust(xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping=0.0, step_eps=1e-5, iters=8, min_points=6,
                      frame_normals=None, min_cos=0.0, huber_m=0.0, ranges=None, workspace=None, stats=True, sums29=False, residuals=False,
                      gate_counts=False):
    """icp_points() with a normal-compatibility gate against the frame's own normals and Huber weights (vors_icp_points_robust):
    frame_normals [n, rows, cols, 3] float32 in the camera frame (depth_normals() of the same depth without poses; None = no gate), a
    point is matched only if dot(model normal in the camera, frame normal) >= min_cos; huber_m > 0 = the Huber threshold on the
    point-to-plane residual in metres ("sums29"[0] and stats rms are then the Huber loss). gate_counts: "gate_counts" [n, 4] int32 of the
    final evaluation (with_depth, within_dist, matched, huber_linear). frame_normals None and huber_m 0: icp_points() bit for bit.
    Everything else, and the result, as in icp_points()."""
    return _icp_device("icp_points_robust", xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping, step_eps, iters, min_points,
                       ranges, workspace, stats, sums29, residuals, (frame_normals, min_cos, huber_m, gate_counts))


def icp_points_robust_host(xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping=0.0, step_eps=1e-5, iters=8, min_points=6,
                           frame_normals=None, min_cos=0.0, huber_m=0.0, count=None, range2=None, residuals=None):
    """The loop of icp_points_robust for ONE list on the host (vors_icp_points_robust_host; needs no GPU): icp_points_host()'s arguments,
    frame_normals [rows, cols, 3] float32 (None = no gate), min_cos, huber_m -> icp_points_host()'s dict and "gate_counts" [4] uint32."""
    return _icp_host("icp_points_robust_host", xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping, step_eps, iters, min_points, count,
                     range2, residuals, (frame_normals, min_cos, huber_m))


def _icp_joint_buffers(who, list_gray, frame_gray, shape, cap, photo_residuals, photo_counts, dev):
    """The grey levels of the lists (None = not given or the handle's own; uint8 [n, capacity]) and of the frames (None or uint8
    [n, rows, cols]) checked, and the tensors behind photo_residuals and photo_counts -> (photo_residuals, photo_counts)."""
    import torch
    n = shape[0]
    if list_gray is not None and (list_gray.dtype != torch.uint8 or not list_gray.is_contiguous() or tuple(list_gray.shape) != (n, cap)):
        raise VorsError(f"{who}: list_gray uint8 {(n, cap)}, contiguous")
    if frame_gray is not None and (frame_gray.dtype != torch.uint8 or not frame_gray.is_contiguous() or tuple(frame_gray.shape) != tuple(shape)):
        raise VorsError(f"{who}: frame_gray uint8 {tuple(shape)}, contiguous")
    res = _out_buf(photo_residuals, (n, cap), torch.float32, dev)
    if photo_residuals is True:
        res.fill_(float("nan"))
    return res, _out_buf(photo_counts, (n, ICP_PHOTO_COUNTS), torch.int32, dev)


def icp_points_joint(xyz, normals, list_gray, list_counts, depth, frame_gray, cam5, depth_scale, poses, dist_m, damping=0.0, step_eps=1e-5,
                     iters=8, min_points=6, frame_normals=None, min_cos=0.0, huber_m=0.0, photo_scale_m=0.0, photo_huber_grey=0.0, ranges=None,
                     workspace=None, stats=True, sums29=False, residuals=False, gate_counts=False, photo_residuals=False, photo_counts=False):
    """icp_points_robust() with a photometric row per matched point against the frames' level-0 grey (vors_icp_points_joint), which holds
    what point-to-plane leaves free: the motion inside a plane. list_gray [n, capacity] uint8 (the "gray" of Trackers.map() /
    Batch.point_cloud()) and frame_gray [n, rows, cols] uint8; both may be None only with photo_scale_m 0. photo_scale_m: metres per grey
    level (0 = no photometric row: icp_points_robust() bit for bit); photo_huber_grey: its Huber threshold in grey levels (0 = off).
    "sums29"[0] and stats rms are then the joint energy's; matched stays the geometric count. photo_residuals: "photo_residuals"
    [n, capacity] float32, I - grey in grey levels, NaN = no photometric row (a new tensor is filled with NaN first); photo_counts:
    "photo_counts" [n, 2] int32 of the final evaluation (photo_used, photo_huber_linear). Everything else, and the rest of the result,
    as in icp_points_robust()."""
    return _icp_device("icp_points_joint", xyz, normals, list_counts, depth, cam5, depth_scale, poses, dist_m, damping, step_eps, iters, min_points,
                       ranges, workspace, stats, sums29, residuals, (frame_normals, min_cos, huber_m, gate_counts),
                       (list_gray, frame_gray, photo_scale_m, photo_huber_grey, photo_residuals, photo_counts))


def icp_points_joint_host(xyz, normals, list_gray, depth, frame_gray, cam5, depth_scale, pose7, dist_m, damping=0.0, step_eps=1e-5, iters=8,
                          min_points=6, frame_normals=None, min_cos=0.0, huber_m=0.0, photo_scale_m=0.0, photo_huber_grey=0.0, count=None,
                          range2=None, residuals=None, photo_residuals=None):
    """The loop of icp_points_joint for ONE list on the host (vors_icp_points_joint_host; needs no GPU): icp_points_robust_host()'s
    arguments, list_gray [capacity] uint8 and frame_gray [rows, cols] uint8 (None only with photo_scale_m 0), photo_scale_m,
    photo_huber_grey -> icp_points_robust_host()'s dict, "photo_residuals" [capacity] float32 (`photo_residuals`: an array to write
    into, None = one filled with NaN) and "photo_counts" [2] uint32."""
    return _icp_host("icp_points_joint_host", xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping, step_eps, iters, min_points, count,
                     range2, residuals, (frame_normals, min_cos, huber_m), (list_gray, frame_gray, photo_scale_m, photo_huber_grey, photo_residuals))


def icp_points_host(xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping=0.0, step_eps=1e-5, iters=8, min_points=6, count=None,
                    range2=None, residuals=None):
    """The loop of icp_points for ONE list on the host (vors_icp_points_host; needs no GPU; the texts and the order of sums the kernels
    run): xyz / normals [capacity, 3] float32, depth [rows, cols] uint16, pose7 camera -> world -> dict: "pose" [7] float32, "stats" (a
    structured scalar of ICP_STATS_DTYPE), "sums29" [29] float32, "residuals" [capacity] float32 with only the ranks of the clipped range
    written (`residuals`: an array to write into, None = one filled with NaN). count = the list's count (None = capacity; above it:
    clipped), range2 = (first, count) or None."""
    return _icp_host("icp_points_host", xyz, normals, depth, cam5, depth_scale, pose7, dist_m, damping, step_eps, iters, min_points, count, range2,
                     residuals)


def ref_sincos(x):
    """sinf / cosf as se3::exp evaluates them on host and device (lie.h ref_sinf / ref_cosf) -> (sin, cos) float32 arrays."""
    x = np.ascontiguousarray(x, np.float32)
    s, c = np.empty_like(x), np.empty_like(x)
    lib().vors_ref_sincos(_ptr(x), x.size, _ptr(s), _ptr(c))
    return s, c


def lm_step(H, g, model7, lm_coef):
    """step() (lm_optimizer.rs:123-136). Returns (ok, model7)."""
    H = np.ascontiguousarray(H, np.float32)
    g = np.ascontiguousarray(g, np.float32)
    model7 = np.ascontiguousarray(model7, np.float32)
    out = np.zeros(7, np.float32)
    ok = C.c_int()
    _check(lib().vors_lm_step(_ptr(H), _ptr(g), _ptr(model7), C.c_float(lm_coef), _ptr(out), C.byref(ok)))
    return bool(ok.value), out


def lm_solve(obs, model7):
    """State::iterative_solve for LMOptimizerState, whole loop on the device -> status, model7, nb_iter, energy, lm_coef."""
    model7 = np.ascontiguousarray(model7, np.float32)
    out = np.zeros(7, np.float32)
    it, e, lam, st = C.c_int32(), C.c_float(), C.c_float(), C.c_int()
    o = obs.to_c()
    _check(lib().vors_lm_solve(C.byref(o), _ptr(model7), _ptr(out), C.byref(it), C.byref(e), C.byref(lam), C.byref(st)))
    return st.value, out, it.value, e.value, lam.value


class Continue:
    """src/math/optimizer.rs:9-14."""
    Stop, Forward = 0, 1


class State:
    """The optimizer trait (src/math/optimizer.rs:32-70). Subclasses provide init / step / eval / stop_criterion;
    `iterative_solve` is the provided method. `step` signals Err by raising StepError."""

    class StepError(Exception):
        pass

    @classmethod
    def init(cls, obs, model):
        raise NotImplementedError

    def step(self):
        raise NotImplementedError

    def eval(self, obs, new_model):
        raise NotImplementedError

    def stop_criterion(self, nb_iter, eval_state):
        raise NotImplementedError

    @classmethod
    def iterative_solve(cls, obs, initial_model):
        state = cls.init(obs, initial_model)
        nb_iter = 0
        while True:
            nb_iter += 1
            new_model = state.step()
            eval_state = state.eval(obs, new_model)
            state, continuation = state.stop_criterion(nb_iter, eval_state)
            if continuation == Continue.Stop:
                return state, nb_iter


class EvalData:
    """lm_optimizer.rs:31-40."""

    def __init__(self, hessian, gradient, energy, model):
        self.hessian, self.gradient, self.energy, self.model = hessian, gradient, energy, model


class LMOptimizerState(State):
    """impl optimizer::State<Obs, EvalState, Iso3, String> for LMOptimizerState (lm_optimizer.rs:111-193), host-driven:
    eval runs on the device through vors_lm_eval, step through vors_lm_step. EvalState = EvalData | float (Err)."""

    def __init__(self, lm_coef, eval_data):
        self.lm_coef, self.eval_data = lm_coef, eval_data

    @staticmethod
    def _full_eval(obs, model):
        e, _, g, H = lm_eval(obs, model)
        return EvalData(H, g, np.float32(e), np.asarray(model, np.float32))

    @classmethod
    def init(cls, obs, model):
        return cls(np.float32(0.1), cls._full_eval(obs, model))

    def step(self):
        ok, model = lm_step(self.eval_data.hessian, self.eval_data.gradient, self.eval_data.model, float(self.lm_coef))
        if not ok:
            raise State.StepError("Error at Cholesky decomposition of hessian")
        return model

    def eval(self, obs, model):
        new = self._full_eval(obs, model)  # the device computes energy and (g, H) in one fused pass
        if new.energy > self.eval_data.energy:
            return float(new.energy)
        return new

    def stop_criterion(self, nb_iter, eval_state):
        too_many_iterations = nb_iter > 20
        is_err = not isinstance(eval_state, EvalData)
        if is_err and too_many_iterations:
            return self, Continue.Stop
        if too_many_iterations:
            return LMOptimizerState(self.lm_coef, eval_state), Continue.Stop
        if is_err:
            return LMOptimizerState(np.float32(self.lm_coef * np.float32(10.0)), self.eval_data), Continue.Forward
        d_energy = np.float32(self.eval_data.energy - eval_state.energy)
        cont = Continue.Forward if d_energy > 1.0 else Continue.Stop
        return LMOptimizerState(np.float32(np.float32(0.1) * self.lm_coef), eval_state), cont


def _vecfn(name, n_in, n_out):
    def f(x):
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        assert x.size == n_in
        out = np.zeros(n_out, np.float32)
        getattr(lib(), name)(_ptr(x), _ptr(out))
        return out
    f.__name__ = name
    return f


se3_exp = _vecfn("vors_se3_exp", 6, 7)
se3_log = _vecfn("vors_se3_log", 7, 6)
so3_exp = _vecfn("vors_so3_exp", 3, 4)
so3_log = _vecfn("vors_so3_log", 4, 3)
iso_inverse = _vecfn("vors_iso_inverse", 7, 7)


def iso_mul(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    out = np.zeros(7, np.float32)
    lib().vors_iso_mul(_ptr(a), _ptr(b), _ptr(out))
    return out
