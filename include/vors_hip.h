/* vors_hip.h — C ABI of the MI355X-native direct RGB-D alignment hot path (libvors_hip.so).
 *
 * Drop-in boundary for the ONE hot path of mpizenberg/visual-odometry-rs ("vors"): pyramidal
 * inverse-compositional direct image alignment. Each entry point cites the reference interface it replaces
 * (paths relative to the reference repository root). The reference has no FFI today (100 % safe Rust); these
 * are the symbols a `-sys` style Rust binding would declare (see INTEGRATION.md for the Rust shim).
 *
 * Conventions
 *  - Plain C types only. Caller owns every buffer. No callbacks, no exceptions/aborts across the ABI.
 *  - Every function returns a vors_status (0 = ok, <0 = error); vors_last_error() gives the message of the last
 *    error on the calling thread.
 *  - Handles are NOT thread-safe (one thread per handle, mirroring `&mut self`); distinct handles are independent.
 *    Tested: distinct handles of every kind, creation and destruction included, used from distinct host threads
 *    at the same time give the bits of one thread's calls. The settings read once per process are read race-free
 *    (function-local statics); the library never writes the environment.
 *  - Images: gray u8 and depth u16 (TUM scale, 0 = unknown), rows x cols, `layout` = VORS_ROW_MAJOR (decoder order)
 *    or VORS_COL_MAJOR (nalgebra DMatrix::as_slice(), element (row,col) at col*rows+row).
 *  - Poses / models: 7 floats  tx ty tz qx qy qz qw  (nalgebra Isometry3<f32>: translation + unit quaternion
 *    coords [i,j,k,w]; same order as the TUM trajectory line, src/dataset/tum_rgbd.rs:76-86).
 *  - There is NO CPU fallback: every compute entry point fails with VORS_ERR_NO_DEVICE when no HIP device exists.
 */
#ifndef VORS_HIP_H
#define VORS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vors_status {
    VORS_OK = 0,
    VORS_ERR_INVALID_ARGUMENT = -1,
    VORS_ERR_NO_DEVICE = -2,        /* no HIP device / HIP runtime error */
    VORS_ERR_HIP = -3,
    VORS_ERR_PYRAMID_TOO_SHORT = -4, /* image too small for nb_levels: the reference panics (inverse_compositional.rs:124,183) */
    VORS_ERR_UNSUPPORTED = -5
} vors_status;

enum { VORS_ROW_MAJOR = 0, VORS_COL_MAJOR = 1 };

/* Candidate mask source. 0 reproduces the reference (candidates::coarse_to_fine, inverse_compositional.rs:120-125).
 * 1 = dense: all-true level-0 mask (extension for BASELINE config "dense candidates"; not in the reference).
 * 2 = DSO-style selection (src/core/candidates/dso.rs with the parameters of examples/candidates_dso.rs:40-59) as the
 *     level-0 mask source (BASELINE config 3; the reference's Tracker never uses it). Its random sub-sampling branch uses a
 *     counter-based hash instead of the reference's unseeded thread_rng. */
enum { VORS_CANDIDATES_COARSE_TO_FINE = 0, VORS_CANDIDATES_DENSE = 1, VORS_CANDIDATES_DSO = 2 };

/* Arithmetic of the LM evaluation (f32 in every mode; the integer stages, the inside test and the LM control flow do not depend on it).
 * The reference has no such choice (Config, inverse_compositional.rs:37-49): ZERO — what a zero-initialised vors_config, the Rust shim of
 * INTEGRATION.md, the vors_track CLI, host/tracker.hpp and vors_amd.Config select — is the mode that reproduces it.
 * 0 = REFERENCE: every per-point expression in the reference's evaluation order without FMA contraction AND the reference's summation:
 *     candidates in extract_z's column-major order (inverse_compositional.rs:260-279), `energy_sum += r * r`, `gradient += jac * r`,
 *     `hessian += hes` (lm_optimizer.rs:72-84,94-100) as sequential f32 multiply-then-add chains in that order, the optical-flow sum of
 *     the keyframe test likewise, sinf / cosf of se3::exp as glibc computes them. The device takes the oracle's LM path decision for
 *     decision: iteration counts equal at every level, poses BIT-IDENTICAL to the oracle's (tests/test_gpu_reference.py, bench.py
 *     `parity_reference`: 4096 / 4096 pairs per candidate mode, 64 / 64 sequences). Every candidate mode, Huber, the trackers and the
 *     operator level support it. Cost (640x480, 6 levels, 4096 pairs, MI355X): see `reference` in bench.py's line.
 * 1 = EXACT: the same per-point arithmetic (inverse depths, Jacobians, residuals bit-identical to the reference's), sums in the
 *     device's tree order. The LM loop's accept / stop comparisons (lm_optimizer.rs:144,179) are decided at ties, so a different order
 *     of the additions forks the loop in some pairs: measured tail beyond 1e-4 rad / 1e-4 m of the oracle — per 4096 pairs:
 *     coarse-to-fine 3, DSO 14, dense 0; per 64 sequences x 39 frames: 1-2 coarse-to-fine, 6-8 DSO (the oracle against its own
 *     f64-accumulation build shows the same counts: it is the order, not the precision).
 * 2 = FUSED: algebraically equivalent shorter forms (warp through the homography K R K^-1 plus _z K t with one hardware reciprocal,
 *     lerp-form bilinear interpolation, factored Jacobian; FMA) on the levels of MANY points; a level of at most 2500 points
 *     (VORS_FUSED_EXACT_POINTS) and every near-identity model is evaluated in the EXACT arithmetic. Per-point values agree
 *     to a few ulp; the tail beyond 1e-4 equals EXACT's (per 4096 pairs: coarse-to-fine 3, DSO 10, dense 0). The fastest mode: what
 *     bench.py's headline times. Pyramids of < 5 levels on large images exceed 1e-4 from summation order alone in modes 1 and 2. */
enum { VORS_ARITH_REFERENCE = 0, VORS_ARITH_EXACT = 1, VORS_ARITH_FUSED = 2 };

/* Per-pair tracking status. Mirrors `optimization_went_well` (inverse_compositional.rs:180,195-199,206-208). */
enum { VORS_TRACK_OK = 0, VORS_TRACK_OPTIMIZER_FAILED_POSE_KEPT = 1 };

/* Replaces `pub struct Config` (src/core/track/inverse_compositional.rs:37-49) with `Intrinsics`
 * (src/core/camera.rs:84-91) flattened. The last two fields are extensions; zero reproduces the reference. */
typedef struct vors_config {
    int32_t nb_levels;                 /* Config::nb_levels */
    int32_t candidates_diff_threshold; /* Config::candidates_diff_threshold (u16) */
    float depth_scale;                 /* Config::depth_scale (5000 for TUM, tum_rgbd.rs:15) */
    float cu, cv;                      /* Intrinsics::principal_point */
    float fu, fv;                      /* Intrinsics::focal */
    float skew;                        /* Intrinsics::skew */
    float idepth_variance;             /* Config::idepth_variance */
    int32_t candidates_mode;           /* extension: VORS_CANDIDATES_* */
    float huber_delta;                 /* extension: Huber threshold on |r| in grey levels; <= 0 = plain L2 (reference) */
    int32_t arithmetic;                /* extension: VORS_ARITH_* (how the per-point f32 expressions are evaluated) */
} vors_config;

#define VORS_MAX_LEVELS 8

/* Per-pair diagnostics of one track() (none of this exists in the reference API; it is what its commented-out
 * eprintln!s would show, lm_optimizer.rs:162,171,184, plus the counters the byte model of DESIGN.md needs). */
typedef struct vors_pair_stats {
    float lm_model[7];                 /* final lm_model (keyframe camera -> current camera), inverse_compositional.rs:177,193 */
    float optical_flow;                /* inverse_compositional.rs:213-221 */
    int32_t change_keyframe;           /* optical_flow >= 1.0 (inverse_compositional.rs:224) */
    int32_t nb_iter[VORS_MAX_LEVELS];  /* iterations returned by iterative_solve per level (optimizer.rs:57-70); 0 = level not run */
    int32_t n_points[VORS_MAX_LEVELS]; /* usable candidates per level (extract_z, inverse_compositional.rs:260-279) */
    float energy[VORS_MAX_LEVELS];     /* energy of the state kept at each level */
    int32_t nb_grad_evals[VORS_MAX_LEVELS]; /* of the nb_iter + 1 evaluations of a level, those for which the reference also forms g and H
                                             * (compute_eval_data, lm_optimizer.rs:90-107,147): the initial one and every accepted candidate */
} vors_pair_stats;

const char* vors_last_error(void);
/* Number of visible HIP devices (0 when none / no runtime). Never fails. */
int vors_device_count(void);
/* Peak shader clock (hipDeviceAttributeClockRate, kHz), compute units and device memory of a HIP device (all nullable). */
vors_status vors_device_info(int device, int* clock_khz, int* compute_units, uint64_t* memory_bytes);
/* Self-check of the DSO selector's gradient-magnitude root (dso_kernels.hip isqrt_floor_u16: the hardware square root + 0.001, truncated):
 * the number of arguments 0 .. 65535 for which it differs from floor(sqrt(n)) on this device — 0 on gfx950 (tests/test_gpu_parity.py). */
vors_status vors_selfcheck_isqrt(int* mismatches);
/* ABI version of this header: bump on any signature change. */
int vors_abi_version(void);  /* 2: vors_config.arithmetic, vors_pair_stats.nb_grad_evals, vors_batch_eval_level
                              * 3: vors_trackers_*, vors_synth_render_frames, vors_multi_rccl_version, vors_pipeline_*, vors_device_info,
                              *    vors_tracker_track_checked
                              * 4: VORS_ARITH_REFERENCE, vors_obs.arithmetic, vors_ref_sincos
                              * 5: VORS_ARITH_* renumbered: 0 = REFERENCE (a zero-initialised vors_config reproduces the reference), 1 = EXACT, 2 = FUSED
                              *    (+ vors_selfcheck_isqrt, added without a signature change; + vors_batch_eval_pairs, vors_batch_pose_information,
                              *    vors_pose_information_from_sums, likewise additions; + vors_batch_residual_maps, vors_residual_scale_from_hist,
                              *    likewise; + vors_batch_reproject_depth, vors_to_depth, vors_from_depth, likewise; + vors_batch_point_cloud,
                              *    vors_camera_back_project, vors_camera_project, likewise; + vors_batch_fuse_depth, vors_fuse_depth_pixels,
                              *    likewise; + vors_trackers_enable_depth_filter, vors_trackers_keyframe_depth, vors_trackers_workspace_bytes,
                              *    vors_tracker_enable_depth_filter, likewise; + vors_trackers_enable_map, vors_trackers_map,
                              *    vors_tracker_enable_map, vors_tracker_read_map, vors_map_segment, likewise; + vors_trackers_enable_map_voxels,
                              *    vors_trackers_map_voxels, vors_tracker_enable_map_voxels, vors_tracker_read_map_voxels, vors_voxel_keys,
                              *    VORS_VOXEL_NONE, likewise; + vors_render_points, vors_render_points_host, vors_trackers_render_map,
                              *    vors_tracker_render_map, VORS_RENDER_COUNTS, likewise; + vors_icp_points, vors_icp_points_host,
                              *    vors_icp_workspace_bytes, vors_trackers_icp_map, vors_icp_stats, likewise; + vors_icp_points_robust,
                              *    vors_icp_points_robust_host, vors_trackers_icp_map_robust, VORS_ICP_GATE_COUNTS, likewise; + vors_trackers_enable_map_icp,
                              *    vors_trackers_map_icp, vors_tracker_enable_map_icp, vors_tracker_read_map_icp, vors_map_icp_window_host,
                              *    vors_map_icp_verdict_host, vors_map_icp_params, vors_map_icp_record, VORS_MAP_ICP_*, likewise; + vors_icp_points_joint,
                              *    vors_icp_points_joint_host, vors_trackers_icp_map_joint, VORS_ICP_PHOTO_COUNTS, likewise; + vors_icp_condition,
                              *    vors_icp_condition_from_sums, vors_trackers_enable_map_icp_joint, vors_trackers_map_icp_joint,
                              *    vors_tracker_enable_map_icp_joint, vors_tracker_read_map_icp_joint, vors_map_icp_verdict_joint_host,
                              *    vors_map_icp_joint_params, vors_map_icp_joint_record, VORS_MAP_ICP_CONDITION, likewise;
                              *    + vors_trackers_enable_map_voxel_stats, vors_trackers_map_voxel_stats, vors_trackers_map_voxel_means,
                              *    vors_tracker_enable_map_voxel_stats, vors_tracker_read_map_voxel_stats, vors_tracker_map_voxel_means,
                              *    vors_voxel_means, vors_voxel_means_host, vors_voxel_stats_host, likewise; + vors_trackers_enable_map_icp_means,
                              *    vors_trackers_map_icp_means, vors_tracker_enable_map_icp_means, vors_tracker_read_map_icp_means,
                              *    vors_map_icp_means_record, likewise; + vors_undistort_frames, vors_undistort_frame_host,
                              *    vors_undistort_source_host, vors_register_depth, vors_register_depth_host, VORS_UNDISTORT_COUNTS,
                              *    VORS_REGISTER_COUNTS, likewise; + vors_pose_graph_optimize, vors_pose_graph_optimize_host,
                              *    vors_pose_graph_workspace_bytes, vors_pose_graph_jacobians_host, vors_pose_graph_stats, VORS_PG_*, likewise;
                              *    + vors_loop_signatures, vors_loop_candidates, vors_loop_verify_edges, their _host twins, vors_loop_sig_meta,
                              *    vors_loop_candidate, VORS_LOOP_*, likewise; + vors_repose_points, vors_repose_points_host,
                              *    vors_trackers_repose_map, vors_voxel_filter_points, vors_voxel_filter_points_host,
                              *    vors_voxel_filter_workspace_bytes, VORS_REPOSE_COUNTS, likewise) */

/* ------------------------------------------------------------------------------------------------------------
 * 1. Tracker: one sequence, host buffers.  Replaces
 *      Config::init(self, f64, &DMatrix<u16>, f64, DMatrix<u8>) -> Tracker      inverse_compositional.rs:74-100
 *      Tracker::track(&mut self, f64, &DMatrix<u16>, f64, DMatrix<u8>)           inverse_compositional.rs:170-240
 *      Tracker::current_frame(&self) -> (f64, Iso3)                              inverse_compositional.rs:243-248
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct vors_tracker vors_tracker;

vors_status vors_tracker_create(const vors_config* cfg, double depth_time, const uint16_t* depth, double img_time,
                                const uint8_t* gray, int rows, int cols, int layout, vors_tracker** out);
/* Returns VORS_OK and writes the VORS_TRACK_* status of this frame to *track_status (nullable). */
vors_status vors_tracker_track(vors_tracker* t, double depth_time, const uint16_t* depth, double img_time,
                               const uint8_t* gray, int* track_status);
/* Same with the frame's shape stated: fails with VORS_ERR_INVALID_ARGUMENT when rows x cols differ from the shape the tracker was created
 * with (vors_tracker_track trusts the caller's buffers to hold rows * cols elements, like the reference trusts its DMatrix arguments). */
vors_status vors_tracker_track_checked(vors_tracker* t, double depth_time, const uint16_t* depth, double img_time, const uint8_t* gray,
                                       int rows, int cols, int* track_status);
vors_status vors_tracker_current_frame(const vors_tracker* t, double* timestamp, float pose7[7]);
/* Diagnostics of the last track() and keyframe pose (not in the reference API). */
vors_status vors_tracker_last_stats(const vors_tracker* t, vors_pair_stats* stats);
vors_status vors_tracker_keyframe(const vors_tracker* t, double* timestamp, float pose7[7]);
/* The recursive depth filter of vors_trackers_enable_depth_filter (below) for the single sequence, its N = 1 case: same arguments, same
 * refusals. vors_tracker_create already took the first frame, so the call is legal until the first vors_tracker_track (refused after it and
 * when repeated); the weights of the first keyframe are derived at this call from the depth map the tracker holds. */
vors_status vors_tracker_enable_depth_filter(vors_tracker* t, float tol_m, int max_weight, int fill_min_weight);
/* One keyframe of a sequence's KEYFRAME MAP (vors_trackers_enable_map, below): 40 bytes, one per keyframe, in order of creation. */
typedef struct vors_map_segment {
    int32_t  frame;      /* frame index of the keyframe (0 = the init frame): the value vors_trackers_state reports as keyframe index */
    uint32_t first;      /* rank of its first point in the sequence's list = the sequence's total before it */
    uint32_t count;      /* its kept points — NOT clipped by capacity */
    float    pose7[7];   /* the keyframe camera -> world pose the points were carried through */
} vors_map_segment;
/* The keyframe map of vors_trackers_enable_map (below) for the single sequence, its N = 1 case: same arguments, same refusals (min_weight
 * >= 2 needs vors_tracker_enable_depth_filter before it). vors_tracker_create already made keyframe 0, so the call is legal until the
 * first vors_tracker_track (refused after it and when repeated) and itself emits keyframe 0's cloud, on the tracker's stream. */
vors_status vors_tracker_enable_map(vors_tracker* t, int level, int capacity, int max_keyframes, int min_weight);
/* The map so far to HOST buffers, each nullable; synchronises. xyz [capacity][3], pixel [capacity], gray [capacity]: the first
 * min(total, capacity, the handle's capacity) points; segments [max_segments]: the first min(keyframes, max_segments, the handle's
 * max_keyframes) records. *count and *n_segments are the UNCLIPPED totals. capacity / max_segments negative, or no enabled map:
 * VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_read_map(vors_tracker* t, int capacity, float* xyz, uint32_t* pixel, uint8_t* gray, uint32_t* count,
                                  int max_segments, vors_map_segment* segments, uint32_t* n_segments);
/* The voxel filter of vors_trackers_enable_map_voxels (below) for the single sequence: same arguments, same refusals. Legal after
 * vors_tracker_enable_map and until the first vors_tracker_track (refused after it and when repeated). vors_tracker_enable_map has already
 * emitted keyframe 0 unfiltered, so THIS CALL RESETS THE MAP (counters, segment count, voxel table) and emits keyframe 0 again through the
 * filter, on the tracker's stream: keyframe 0 appears once. */
vors_status vors_tracker_enable_map_voxels(vors_tracker* t, float voxel_m, int table_slots);
/* The filter's two counters (vors_trackers_map_voxels, below) to the host, each nullable; synchronises. Filter not enabled:
 * VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_read_map_voxels(vors_tracker* t, uint32_t* occupied, uint32_t* overflow);
/* The voxels' statistics of vors_trackers_enable_map_voxel_stats (below) for the single sequence: same refusals. Legal after
 * vors_tracker_enable_map_voxels, before vors_tracker_enable_map_normals and until the first vors_tracker_track (refused after it and
 * when repeated). Like vors_tracker_enable_map_voxels THIS CALL RESETS THE MAP and emits keyframe 0 again, now counted. */
vors_status vors_tracker_enable_map_voxel_stats(vors_tracker* t);
/* The statistics so far to HOST buffers, each nullable; synchronises. sums [capacity][4] int64, obs [capacity][2]: the first
 * min(total, capacity, the handle's capacity) ranks, rank for rank those of vors_tracker_read_map. Negative capacity or statistics not
 * enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_read_map_voxel_stats(vors_tracker* t, int capacity, int64_t* sums, uint32_t* obs);
/* The averaged list of vors_trackers_map_voxel_means (below) for the single sequence, to HOST buffers, each nullable but at least one
 * required; synchronises. xyz_mean [capacity][3], gray_mean [capacity]: the first min(total, capacity, the handle's capacity) ranks;
 * *kept counts the passing ranks of the whole clipped list. The handle keeps no device staging for it: the statistics are read back and
 * resolved by vors_voxel_means_host, the text of the device pass, so the bits are those of the N = 1 handle. */
vors_status vors_tracker_map_voxel_means(vors_tracker* t, uint32_t min_count, uint32_t min_span, int capacity, float* xyz_mean,
                                         uint8_t* gray_mean, uint32_t* kept);
/* The rendering of vors_trackers_render_map (below) for the single sequence, its N = 1 case, to HOST buffers; synchronises. pose7 (HOST,
 * nullable): camera -> world, NULL = the current frame's pose as the device holds it. range2 (HOST, nullable): (first, count) of the ranks
 * to render, NULL = the whole map. zkey / depth / gray [rows_l * cols_l] and counts [VORS_RENDER_COUNTS] are each nullable (zkey too: the
 * key plane is staging here). The device staging (11 bytes per level-0 pixel and 64 bytes of arguments and counters) is the handle's own,
 * created by the first call; no later call allocates. Same refusals; no enabled map: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_render_map(vors_tracker* t, int level, const float pose7[7] /* nullable */, const uint32_t range2[2] /* nullable */,
                                    int footprint, uint64_t* zkey, uint16_t* depth, uint8_t* gray, uint32_t* counts);
/* The normals of vors_trackers_enable_map_normals (below) for the single sequence: same arguments, same refusals. Legal after
 * vors_tracker_enable_map (and vors_tracker_enable_map_voxels, if used) and until the first vors_tracker_track (refused after it and when
 * repeated); it computes keyframe 0's normals itself, on the tracker's stream, from the depth map the tracker holds (with the depth
 * filter: the filter's copy of it). vors_tracker_enable_map_voxels called AFTER it is refused: that call emits keyframe 0 again. */
vors_status vors_tracker_enable_map_normals(vors_tracker* t, int step, float jump_m);
/* The map's normals so far to a HOST buffer normals [capacity][3]: the first min(total, capacity, the handle's capacity) entries, rank for
 * rank those of vors_tracker_read_map; synchronises. capacity negative, normals NULL or not enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_read_map_normals(vors_tracker* t, int capacity, float* normals);
/* Parameters of the MAP ICP CORRECTION at keyframe promotion (vors_trackers_enable_map_icp, below). */
typedef struct vors_map_icp_params {
    float dist_m, damping, step_eps; int32_t iters, min_points;   /* vors_icp_points' */
    int32_t normal_gate; float min_cos, huber_m;                  /* vors_icp_points_robust'; normal_gate = 0: no frame normals are computed or kept */
    int32_t last_keyframes;                                       /* window: 0 = the whole map */
    float min_match_ratio, max_rms, max_trans_m, max_rot_rad;     /* the verdict */
} vors_map_icp_params;
#define VORS_MAP_ICP_NOT_ATTEMPTED 0   /* not promoted in the last call */
#define VORS_MAP_ICP_ACCEPTED      1
#define VORS_MAP_ICP_ICP_STATUS    2   /* TOO_FEW or SINGULAR (an empty window ends here) */
#define VORS_MAP_ICP_FEW_MATCHES   3
#define VORS_MAP_ICP_RMS           4
#define VORS_MAP_ICP_STEP          5   /* correction larger than max_trans_m / max_rot_rad */
#define VORS_MAP_ICP_NONFINITE     6
struct vors_map_icp_record;  /* section 2e, behind vors_icp_stats */
/* The correction of vors_trackers_enable_map_icp (below) for the single sequence, its N = 1 case: same parameters, same refusals. Legal
 * after vors_tracker_enable_map_normals and until the first vors_tracker_track (refused after it and when repeated). With it,
 * vors_tracker_track reads its results back BEHIND the promotion instead of under it, so that the pose it returns, vors_tracker_current_frame
 * and vors_tracker_keyframe report the corrected pose; a frame then waits for its promotion. */
vors_status vors_tracker_enable_map_icp(vors_tracker* t, const vors_map_icp_params* params);
/* The record of the LAST vors_tracker_track and the running totals (attempted, accepted) to the host, each nullable; synchronises. Not
 * enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_read_map_icp(vors_tracker* t, struct vors_map_icp_record* record, uint32_t totals[2]);
/* Parameters of the map ICP correction THROUGH THE JOINT PASS AND WITH THE CONDITION TEST (vors_trackers_enable_map_icp_joint, below). */
typedef struct vors_map_icp_joint_params {
    vors_map_icp_params icp;                 /* every field as in vors_trackers_enable_map_icp */
    float photo_scale_m, photo_huber_grey;   /* vors_icp_points_joint's; photo_scale_m = 0: the robust pass */
    float max_dilution_t, max_dilution_r;    /* the CONDITION test; 0 = that bound is off */
} vors_map_icp_joint_params;
#define VORS_MAP_ICP_CONDITION     7   /* joint stage only: a dilution above its bound, or no dilution at all (H has no Cholesky factor) */
struct vors_map_icp_joint_record;  /* section 2e, behind vors_map_icp_record */
/* The correction of vors_trackers_enable_map_icp_joint (below) for the single sequence, its N = 1 case: same parameters, same refusals.
 * Legal exactly where vors_tracker_enable_map_icp is, INSTEAD of it: either one after the other is refused. vors_tracker_track reads its
 * results back behind the promotion, as with vors_tracker_enable_map_icp, and vors_tracker_read_map_icp works unchanged. */
vors_status vors_tracker_enable_map_icp_joint(vors_tracker* t, const vors_map_icp_joint_params* params);
/* The joint record of the LAST vors_tracker_track to the host (nullable); synchronises. No joint stage: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_read_map_icp_joint(vors_tracker* t, struct vors_map_icp_joint_record* record);
struct vors_map_icp_means_record;  /* section 2e, behind vors_map_icp_joint_record */
/* The averaged model of vors_trackers_enable_map_icp_means (below) for the single sequence, its N = 1 case: same arguments, same refusals.
 * Legal after vors_tracker_enable_map_voxel_stats and after one of vors_tracker_enable_map_icp / _joint, until the first
 * vors_tracker_track (refused after it and when repeated). */
vors_status vors_tracker_enable_map_icp_means(vors_tracker* t, uint32_t min_count, uint32_t min_span);
/* The means record of the LAST vors_tracker_track to the host (nullable); synchronises. Means not enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_tracker_read_map_icp_means(vors_tracker* t, struct vors_map_icp_means_record* record);
void vors_tracker_destroy(vors_tracker* t);

/* ------------------------------------------------------------------------------------------------------------
 * 1b. N sequences advancing in lock-step, device resident — what a host that tracks many cameras / many replays calls. For every
 *     sequence s the calls below are exactly
 *        tracker[s] = cfg.init(depth0[s], gray0[s])        vors_trackers_init     (vors_track.rs:46)
 *        tracker[s].track(depth_k[s], gray_k[s])            vors_trackers_track    (vors_track.rs:54-59), k = 1, 2, ...
 *        tracker[s].current_frame()                         vors_trackers_current_frames / _state  (vors_track.rs:62)
 *     with the WHOLE state machine of Tracker::track on the device: the initial guess from the poses of the previous frame
 *     (inverse_compositional.rs:177), the LM loop, the pose composition (:203-208), the optical-flow keyframe test (:211-224) and — for
 *     exactly the sequences whose flow reached the threshold — the promotion of the current frame to keyframe (:227-239:
 *     precompute_multires_data on the current pyramid and THIS call's depth map, keyframe_pose <- current_frame_pose). No host round
 *     trip, no synchronisation: init and track only enqueue work on hip_stream. (A trackers-owned batch keeps no pointer into the
 *     caller's frames in the sparse modes: keyframe inspection through vors_batch_* is not available for it.) Results per sequence are bit-identical to a vors_tracker fed
 *     the same frames for handles of fewer than 512 sequences (tests/test_gpu_trackers.py); larger handles are scheduled differently
 *     (threads per sequence, evaluation rounds), which changes the ORDER of the f32 sums and with it the last bits, nothing else.
 *     Frames: DEVICE buffers, row-major, sequence s at offset s * rows * cols; they are read by the work this call enqueues and by
 *     nothing later (dense mode copies a promoted frame into the handle), so the caller may reuse them once the stream has passed
 *     the call. Timestamps stay with the caller: vors_trackers_state / _current_frames report, per sequence, the index of the frame
 *     that is its keyframe (0 = the init frame, k = the k-th track call).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct vors_trackers vors_trackers;
vors_status vors_trackers_create(const vors_config* cfg, int n_sequences, int rows, int cols, vors_trackers** out);
/* Same on an explicit HIP device (several GPUs = one handle per device, each with its own sequences: "replicas only", like batches). */
vors_status vors_trackers_create_on(int device, const vors_config* cfg, int n_sequences, int rows, int cols, vors_trackers** out);
int vors_trackers_count(const vors_trackers* t);
vors_status vors_trackers_init(vors_trackers* t, const uint8_t* d_gray, const uint16_t* d_depth, void* hip_stream);
vors_status vors_trackers_track(vors_trackers* t, const uint8_t* d_gray, const uint16_t* d_depth, void* hip_stream);
/* DEVICE pointers (valid for the life of the handle, contents valid once the stream has passed the last track call; all nullable):
 * current_frame_pose [n,7], keyframe_pose [n,7], VORS_TRACK_* status of the last track [n], keyframe frame index [n], diagnostics of the
 * last track [n]. */
vors_status vors_trackers_state(const vors_trackers* t, const float** d_current_poses7, const float** d_keyframe_poses7,
                                const int32_t** d_status, const int32_t** d_keyframe_index, const vors_pair_stats** d_stats);
/* Same to HOST buffers (nullable each); synchronises hip_stream. */
vors_status vors_trackers_current_frames(vors_trackers* t, float* poses7, int32_t* status, int32_t* keyframe_index, void* hip_stream);
/* Diagnostics of the last track of every sequence to a HOST buffer [n]; synchronises hip_stream. */
vors_status vors_trackers_last_stats(vors_trackers* t, vors_pair_stats* stats, void* hip_stream);
/* Stage timing as for a batch handle (stages 1 = keyframe promotion, 2 = current pyramid, 3 = LM). */
vors_status vors_trackers_enable_kernel_timing(vors_trackers* t, int ring);
vors_status vors_trackers_kernel_times(vors_trackers* t, int stage, float* ms_out, int capacity, int* n_out);
/* RECURSIVE DEPTH FILTER across keyframe promotions (opt-in; without this call nothing changes: no launch, no allocation, no kernel
 * argument). Every sequence keeps, next to its keyframe, the keyframe's depth map and a weight map (how many measurements a pixel's depth
 * stands for). vors_trackers_init: depth = the measured depth, weight = 1 where it is non-zero, 0 where it is 0. vors_trackers_track, for
 * exactly the sequences that promote, before the keyframe stage and on the device: the OLD keyframe's usable level-0 points are splatted
 * at the sequence's final model of this frame (the head of its vors_pair_stats) with the keyframe's weights, and merged with this frame's
 * d_depth — the pass and the rule table of vors_batch_fuse_depth (section 2), unchanged, as masked launches over the promotion list. The
 * keyframe stage (all candidate modes and arithmetics) then runs on the FUSED depth instead of d_depth, and the fused weight becomes
 * the keyframe's weight. A sequence that does not promote keeps both planes bit for bit: the filter advances at promotions only.
 * tol_m, max_weight, fill_min_weight: those of vors_batch_fuse_depth, with its refusals (tol_m negative or NaN, max_weight outside
 * 1..255, fill_min_weight outside 0..255). Legal after create and before vors_trackers_init only (afterwards the weights would have no
 * history) and only once: otherwise VORS_ERR_INVALID_ARGUMENT. The call allocates every plane the filter needs (13 bytes per pixel and
 * sequence: key plane, depth, weight, staged weight); no later call allocates. vors_trackers_workspace_bytes — the workspace of the
 * batch handle the sequences run on, vors_batch_workspace_bytes' figure — includes them from then on. */
vors_status vors_trackers_enable_depth_filter(vors_trackers* t, float tol_m, int max_weight, int fill_min_weight);
/* DEVICE views [n_sequences][rows * cols] of every sequence's current keyframe depth (u16) and weight (u8), in the keyframe's geometry;
 * valid for the life of the handle, contents valid in stream order after the last init / track. Either output may be NULL. Without an
 * enabled filter: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_keyframe_depth(const vors_trackers* t, const uint16_t** d_depth, const uint8_t** d_weight);
vors_status vors_trackers_workspace_bytes(const vors_trackers* t, uint64_t* bytes);
/* KEYFRAME MAP (opt-in; without this call nothing changes: no launch, no allocation, no kernel argument on any existing path). Every time
 * a sequence gets a new keyframe — vors_trackers_init: every sequence; vors_trackers_track: exactly the promoted ones — the keyframe's
 * cloud is appended, on the device and in stream order, to a list the handle owns for that sequence, with one vors_map_segment per
 * keyframe. The emission comes after the keyframe stage (REFERENCE arithmetic: after the column-major sort, so the records are in their
 * final order) as masked launches over the promotion list, and reads the handle's own data only: the records, in dense mode the handle's
 * copy of the keyframe image and depth, and the keyframe pose, which the track call has already moved forward. Nothing of the caller's
 * frames is read, and a sequence that does not promote is touched by no launch.
 * Points: vors_batch_point_cloud's rule (section 2), unchanged — the usable points of `level` (extract_z's set) in ascending slot order of
 * the level's source: row-major raster order in dense mode, the order vors_batch_get_points reports for the candidate lists. Per point:
 * xyz = keyframe pose * back_project(K_level, x, y, 1.0f / idepth) in the reference's per-point arithmetic (the bits of
 * vors_camera_back_project; the pose is ALWAYS applied), pixel = x | y << 16, gray = the template intensity.
 * Keep rule: min_weight <= 1 keeps every usable point and reads no weight. min_weight >= 2 keeps a point iff the depth filter's weight at
 * its pixel — the NEW keyframe's, after the promotion — is >= min_weight; at init every weight is 1 and nothing is kept. It needs
 * vors_trackers_enable_depth_filter BEFORE this call and level == 0 (the weight plane exists at full resolution only).
 * Legal after create and before vors_trackers_init, once. VORS_ERR_INVALID_ARGUMENT, with nothing allocated and nothing enqueued: NULL
 * handle, repeated call, call after init, level outside 0..nb_levels-1, capacity < 1, max_keyframes < 1, min_weight outside 0..255,
 * min_weight >= 2 without the filter or with level != 0. The call allocates, as part of vors_trackers_workspace_bytes' figure and freed
 * with the handle, n * capacity * 17 bytes of lists, n * max_keyframes * 40 bytes of segments, 8 n bytes of counters and the count
 * workspace of the pass (4 bytes per sequence and chunk of `level`, vors_batch_point_cloud's cut); no later call allocates.
 * vors_trackers_init zeroes both counters on the stream: a handle that is initialised again starts an empty map. */
vors_status vors_trackers_enable_map(vors_trackers* t, int level, int capacity, int max_keyframes, int min_weight);
/* DEVICE pointers, owned by the handle and valid for its life, contents valid in stream order after the last init / track; every output
 * is nullable:
 *   d_xyz [n][capacity][3] f32, d_pixel [n][capacity] u32, d_gray [n][capacity] u8   the lists
 *   d_counts [n] u32       running total of kept points of a sequence; may exceed capacity, saturates at 0xFFFFFFFF. Exactly the entries
 *                          of rank < min(total, capacity) are written: later points are dropped but COUNTED, here and in their segment
 *   d_segments [n][max_keyframes] vors_map_segment, d_n_segments [n] u32   every keyframe created is counted, the first max_keyframes
 *                          records are written
 * The order of ranks is a function of the sequence's own frames alone. Without an enabled map: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_map(const vors_trackers* t, const float** d_xyz, const uint32_t** d_pixel, const uint8_t** d_gray,
                              const uint32_t** d_counts, const vors_map_segment** d_segments, const uint32_t** d_n_segments);
/* VOXEL FILTER OF THE KEYFRAME MAP (opt-in on top of an enabled map; without this call nothing changes: no launch, no allocation, no
 * kernel argument on any existing path). The map then keeps, per sequence, exactly ONE point per occupied voxel of a world-frame grid of
 * edge voxel_m: the first in the map's own order. Precisely: let U be the list the map would hold without the filter (unclipped). The
 * filtered list is U restricted to the entries whose voxel key (vors_voxel_keys, section 4, of the stored xyz) is not VORS_VOXEL_NONE and
 * occurs at no lower rank of U, in U's order; xyz, pixel and gray of a kept entry are U's bits. A segment keeps frame and pose7, `count`
 * is the keyframe's kept points and `first` the filtered total before it; d_counts, clipping by capacity / max_keyframes and saturation
 * are vors_trackers_map's rules applied to the filtered list. The keep rule of the map (min_weight) is applied first, unchanged. The
 * result does not depend on scheduling, on the other sequences, on the stream or on table_slots — as long as the table has not overflowed.
 * Table: per sequence, open addressing with linear probing over table_slots entries (a power of two) of two 64-bit words, which places
 * every voxel while a sequence's DISTINCT voxels are <= table_slots. Beyond that the sequence's sticky overflow word is set: from the
 * overflowing keyframe on its map contents are unspecified (every store stays inside its buffers, d_counts and the segment records are
 * still written, every call returns normally, tracking is untouched, and a point probes at most table_slots entries); the other sequences
 * keep the exact result. vors_trackers_init empties the table and zeroes both words on the stream.
 * Legal after vors_trackers_enable_map and before vors_trackers_init, once. VORS_ERR_INVALID_ARGUMENT, with nothing allocated and nothing
 * enqueued: NULL handle, no enabled map, repeated call, call after init, voxel_m not finite or <= 0, table_slots not a power of two or
 * outside 64..2^30. The call allocates, as part of vors_trackers_workspace_bytes' figure and freed with the handle,
 * n * (16 * table_slots + 8) bytes: the table and the two words per sequence; no later call allocates. */
vors_status vors_trackers_enable_map_voxels(vors_trackers* t, float voxel_m, int table_slots);
/* DEVICE pointers [n] u32, owned by the handle and valid for its life, contents valid in stream order after the last init / track, each
 * nullable: d_occupied = claimed table entries of a sequence = its distinct voxels so far (== d_counts while it has not overflowed),
 * d_overflow = non-zero once the sequence has overflowed. Filter not enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_map_voxels(const vors_trackers* t, const uint32_t** d_occupied, const uint32_t** d_overflow);
/* STATISTICS OF THE MAP'S VOXELS (opt-in on top of the voxel filter; without this call nothing changes: no launch, no allocation, no
 * kernel argument on any existing path). The map's own lists, counts, segments and normals keep exactly their bits; the statistics live
 * in arrays of their own, rank-aligned with the lists. Per sequence and rank r < min(total, capacity): let f be the stored xyz of rank r
 * (the voxel's first point) and P(r) every point of every keyframe emitted so far that passes the map's keep rule (min_weight) and whose
 * voxel key (vors_voxel_keys, of the world point the map would store) equals f's; the first point itself is in P(r). Then
 *   sums[r][a] = sum over P(r) of (int64) rintf(((w_a - f_a) / voxel_m) * 1048576.0f), a = x, y, z: an f32 subtraction, an IEEE f32
 *                division, an exact multiplication, round-half-even. |q_a| stays near 2^20, so 2^32 observations fit below 2^53;
 *   sums[r][3] = sum over P(r) of the u8 grey the map would store;
 *   obs[r]     = {|P(r)| (wraps at 2^32), the highest segment index — the keyframe's index among the sequence's keyframes — of a
 *                contributor}; the rank's own segment is the lowest, so the difference is the span over which the voxel was re-observed.
 * The sums are integers accumulated with integer atomics, so they do not depend on scheduling, on the other sequences, on the stream or
 * on table_slots. A voxel whose rank is at or beyond capacity accumulates nothing. From the keyframe at which a sequence overflows its
 * table its statistics are unspecified like the rest of its map; every store stays inside its buffers. vors_trackers_init zeroes
 * everything on the stream. Per emission the filter's WRITE launch is replaced by one that also records ranks, and one launch is added.
 * Legal after vors_trackers_enable_map_voxels and before vors_trackers_init, once; VORS_ERR_INVALID_ARGUMENT otherwise and for a NULL
 * handle, with nothing allocated and nothing enqueued. The call allocates, as part of vors_trackers_workspace_bytes' figure and freed
 * with the handle, n * (4 * table_slots + 40 * capacity) bytes; no later call allocates. */
vors_status vors_trackers_enable_map_voxel_stats(vors_trackers* t);
/* DEVICE pointers, owned by the handle and valid for its life, contents valid in stream order after the last init / track, each
 * nullable: d_sums [n][capacity][4] int64, d_obs [n][capacity][2] u32. Statistics not enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_map_voxel_stats(const vors_trackers* t, const int64_t** d_sums, const uint32_t** d_obs);
/* THE AVERAGED MAP: vors_voxel_means (section 2d) on the handle's own lists and statistics, with the handle's voxel_m. The first segment
 * of a rank is found inside the pass by a binary search over the `first` of the sequence's segment records (no plane of its own, no
 * launch more); a rank of a keyframe beyond max_keyframes has no record and takes the last recorded segment. Outputs (DEVICE, each
 * nullable, at least one required) as in vors_voxel_means. Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: NULL handle,
 * statistics not enabled, a call before vors_trackers_init, no output at all, misaligned outputs, a stream of another device. The pass
 * reads the map only, writes the caller's arrays only and allocates nothing; enqueued on hip_stream, NOT synchronised. */
vors_status vors_trackers_map_voxel_means(vors_trackers* t, uint32_t min_count, uint32_t min_span, float* d_xyz_mean /* nullable */,
                                          uint8_t* d_gray_mean /* nullable */, uint32_t* d_kept /* nullable */, void* hip_stream);
/* THE KEYFRAME MAP SEEN FROM A POSE: vors_render_points (section 2c) on the handle's own map — its lists, its counters, the intrinsics and
 * the shape of pyramid level `level` (rows_l x cols_l), the handle's depth_scale. d_poses7 (DEVICE, nullable): one camera -> world pose per
 * sequence, pose_stride_bytes apart (0 = 28); NULL = every sequence's CURRENT FRAME pose, read on the device from the handle's pose table
 * (the pointer vors_trackers_state reports), so the call needs no synchronisation after a track. d_ranges / range_stride_bytes, footprint
 * and the outputs d_zkey (required) / d_depth / d_gray / d_counts [n][rows_l * cols_l] resp. [n][VORS_RENDER_COUNTS]: as in
 * vors_render_points; sizeof(vors_map_segment) with &d_segments[k].first renders keyframe k alone. Refused with
 * VORS_ERR_INVALID_ARGUMENT, nothing enqueued: no enabled map, a call before vors_trackers_init, a level out of range, a stream of another
 * device, and every refusal of vors_render_points. The pass reads the map and the pose table only, writes the caller's planes only, and
 * allocates nothing; enqueued on hip_stream, NOT synchronised. */
vors_status vors_trackers_render_map(vors_trackers* t, int level, const void* d_poses7 /* nullable */, size_t pose_stride_bytes,
                                     const void* d_ranges /* nullable */, size_t range_stride_bytes, int footprint,
                                     uint64_t* d_zkey, uint16_t* d_depth /* nullable */, uint8_t* d_gray /* nullable */,
                                     uint32_t* d_counts /* nullable */, void* hip_stream);
/* NORMALS OF THE KEYFRAME MAP (opt-in on top of an enabled map; without this call nothing changes: no launch, no allocation, no kernel
 * argument on any existing path). Every map entry then carries the surface normal of its pixel in its keyframe's depth plane, in the world
 * frame: vors_points_normals (section 2d) over the ranks a keyframe's emission appended, with the stored pixels, the keyframe's pose and
 * (step, jump_m). The depth plane is the one the keyframe stage of that call ran on: the frame's depth map, with the depth filter the
 * fused map (what vors_trackers_keyframe_depth shows after the call), at init the init depth. The caller's plane is read only by work the
 * call itself enqueues. The pass is keyed on the stored pixels, so the voxel filter and the keep rule need nothing; a keyframe beyond
 * max_keyframes still gets its normals; ranks at or above capacity are never stored. Per track call two more launches: a copy of the
 * running totals before the emission and one masked launch after it. Tracking, the map's lists and its segments keep their bits.
 * Legal after vors_trackers_enable_map and before vors_trackers_init, once. VORS_ERR_INVALID_ARGUMENT, with nothing allocated and nothing
 * enqueued: NULL handle, no enabled map, a map whose level is not 0 (depth planes exist at full resolution only), repeated call, call
 * after init, step outside 1..8, jump_m negative or NaN. The call allocates, as part of vors_trackers_workspace_bytes' figure and freed
 * with the handle, n * capacity * 12 + 4 n bytes; no later call allocates. */
vors_status vors_trackers_enable_map_normals(vors_trackers* t, int step, float jump_m);
/* DEVICE pointer [n][capacity][3] f32, owned by the handle and valid for its life: entry r of a sequence is the normal of the map's entry
 * r, valid in stream order after the last init / track for r < min(total, capacity). Not enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_map_normals(const vors_trackers* t, const float** d_normals);
/* THE KEYFRAME MAP ALIGNED TO DEPTH FRAMES: vors_icp_points (section 2e) on the handle's own map and map normals, its level-0 intrinsics
 * and shape and its depth_scale, against d_depth [n][rows * cols] u16 (DEVICE; usually the frames of the last track call). d_poses7_in
 * (DEVICE, nullable): the start poses, pose_stride_bytes apart (0 = 28); NULL = every sequence's CURRENT FRAME pose, read on the device
 * from the handle's pose table, so the call needs no synchronisation after a track. d_workspace: vors_icp_workspace_bytes(n, the map's
 * capacity) bytes. Everything else as in vors_icp_points. The pass READS the handle only: the tracker's poses, its map and its later
 * results keep their bits. Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: a NULL handle, no enabled map, no enabled map
 * normals, a call before vors_trackers_init, a stream of another device, and every refusal of vors_icp_points. Allocates nothing;
 * enqueued on hip_stream, NOT synchronised. */
struct vors_icp_stats;  /* section 2e */
vors_status vors_trackers_icp_map(vors_trackers* t, const uint16_t* d_depth, float dist_m, float damping, float step_eps, int iters,
                                  int min_points, const void* d_ranges /* nullable */, size_t range_stride_bytes,
                                  const void* d_poses7_in /* nullable */, size_t pose_stride_bytes, void* d_workspace,
                                  float* d_poses7_out, struct vors_icp_stats* d_stats /* nullable */, float* d_sums29 /* nullable */,
                                  float* d_residuals /* nullable */, void* hip_stream);
/* ... and the robust pass (vors_icp_points_robust, section 2e) on the same inputs: d_frame_normals [n][rows * cols][3] f32 (DEVICE,
 * nullable; vors_depth_normals of d_depth at level 0 without poses), min_cos, huber_m and d_gate_counts [n][4] u32 (nullable) as there.
 * The same checks, then every refusal of vors_icp_points_robust. Reads the handle only. */
vors_status vors_trackers_icp_map_robust(vors_trackers* t, const uint16_t* d_depth, float dist_m, float damping, float step_eps, int iters,
                                         int min_points, const void* d_ranges /* nullable */, size_t range_stride_bytes,
                                         const void* d_poses7_in /* nullable */, size_t pose_stride_bytes,
                                         const float* d_frame_normals /* nullable */, float min_cos, float huber_m, void* d_workspace,
                                         float* d_poses7_out, struct vors_icp_stats* d_stats /* nullable */, float* d_sums29 /* nullable */,
                                         float* d_residuals /* nullable */, uint32_t* d_gate_counts /* nullable */, void* hip_stream);
/* ... and the joint pass (vors_icp_points_joint, section 2e) on the same inputs, with the map's own grey levels (vors_trackers_map's
 * d_gray) as the list's: d_frame_gray [n][rows * cols] u8 (DEVICE, the level-0 grey frames the depth belongs to; nullable when
 * photo_scale_m is 0), photo_scale_m, photo_huber_grey, d_photo_residuals [n][capacity] f32 and d_photo_counts [n][2] u32 (both
 * nullable) as there. The same checks, then every refusal of vors_icp_points_joint. Reads the handle only. */
vors_status vors_trackers_icp_map_joint(vors_trackers* t, const uint16_t* d_depth, const uint8_t* d_frame_gray /* nullable */, float dist_m,
                                        float damping, float step_eps, int iters, int min_points, const void* d_ranges /* nullable */,
                                        size_t range_stride_bytes, const void* d_poses7_in /* nullable */, size_t pose_stride_bytes,
                                        const float* d_frame_normals /* nullable */, float min_cos, float huber_m, float photo_scale_m,
                                        float photo_huber_grey, void* d_workspace, float* d_poses7_out,
                                        struct vors_icp_stats* d_stats /* nullable */, float* d_sums29 /* nullable */,
                                        float* d_residuals /* nullable */, uint32_t* d_gate_counts /* nullable */,
                                        float* d_photo_residuals /* nullable */, uint32_t* d_photo_counts /* nullable */, void* hip_stream);
/* MAP ICP CORRECTION AT KEYFRAME PROMOTION (opt-in on top of an enabled map with normals; without this call nothing changes: no launch, no
 * allocation, no kernel argument on any existing path). vors_trackers_track then closes the loop between the map and the trajectory: for
 * every sequence it promotes — behind the keyframe stage and BEFORE the new keyframe's cloud is emitted — the EXISTING map (a window of it)
 * is aligned to the new keyframe's depth by vors_icp_points_robust's pass, starting from the keyframe pose the call has just written; a
 * result that passes the verdict replaces the sequence's keyframe pose, current frame pose and output pose, so that the emission and the
 * normals pass behind it append the new cloud at the corrected pose, vors_trackers_current_frames / _state report it and the next
 * frame's LM starts from it. A rejected result changes nothing. The depth plane is the one the emission's normals pass reads: the caller's
 * frame, with the depth filter the fused plane, in dense mode the handle's copy. Not run at vors_trackers_init (the map is still empty).
 * Window (one text, lie.h map_icp_window; host twin vors_map_icp_window_host): n_rec = min(n_segments, max_keyframes), total = min(count,
 *   capacity); first = 0 when last_keyframes == 0 or n_rec <= last_keyframes, else the `first` of recorded segment n_rec - last_keyframes,
 *   clipped to total; the window is (first, total - first) — always to the end of the list — of the map as it stood BEFORE this
 *   promotion's emission: a keyframe's own cloud is never part of its model.
 * Verdict (one text, lie.h map_icp_verdict; host twin vors_map_icp_verdict_host), the first failure names it, every comparison in float,
 *   NaN fails: NONFINITE — a non-finite number in the ICP's pose; ICP_STATUS — status neither ITERATIONS nor CONVERGED; FEW_MATCHES —
 *   (float)matched >= min_match_ratio * (float)considered fails; RMS — rms <= max_rms fails; STEP — with D = inverse(pose before) * pose
 *   after, dot3(D.t, D.t) <= max_trans_m^2 or fabsf(D.q.w) >= cosf(0.5f * max_rot_rad) fails (the cosine is taken once, at this call).
 * Launches: the host cannot know whether a sequence promotes, so EVERY track call enqueues the stage — ARM (one thread per sequence: promoted
 *   flag, window, start pose, record reset), with normal_gate one masked launch for the frame normals of the promoted sequences (the rule
 *   of vors_depth_normals without poses, at the map normals' step / jump_m), the ICP's memset and 2 * iters + 3 launches, APPLY (one thread
 *   per promoted sequence): 2 * iters + 5 kernel launches and one memset, + 1 with normal_gate. A sequence that is not promoted has the
 *   window (0, 0): its evaluation workgroups return at once and the first solve freezes it. Nothing waits on the host. Measured (64 sequences of
 *   640x480, 6 rounds): 0.157 ms per track call when nothing promotes.
 * Legal where vors_trackers_enable_map_normals is legal and after it: before vors_trackers_init, once. VORS_ERR_INVALID_ARGUMENT, nothing
 * allocated: NULL handle or params, no enabled map, no enabled map normals, repeated call, call after init, everything
 * vors_icp_points_robust refuses of the shared parameters, last_keyframes < 0, min_match_ratio outside [0, 1] or NaN, max_rms /
 * max_trans_m / max_rot_rad negative or NaN. The call allocates, as part of vors_trackers_workspace_bytes' figure and freed with the
 * handle: vors_icp_workspace_bytes(n, capacity), and per sequence 8 bytes of window, 4 of flag, 56 of poses, 24 + 16 of staged
 * statistics and gate counts, a vors_map_icp_record (112 bytes) and 8 bytes of totals; with normal_gate n * rows * cols * 12 bytes of
 * frame normals. No later call allocates. vors_trackers_init zeroes records and totals on the stream. */
vors_status vors_trackers_enable_map_icp(vors_trackers* t, const vors_map_icp_params* params);
/* DEVICE pointers, owned by the handle and valid for its life, contents valid in stream order after the last track, each nullable:
 * d_records [n] — of the LAST track call, verdict NOT_ATTEMPTED for a sequence it did not promote — and d_totals [n][2] u32: promotions
 * attempted and accepted since init. Not enabled: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_map_icp(const vors_trackers* t, const struct vors_map_icp_record** d_records,
                                  const uint32_t** d_totals /* [n][2]: attempted, accepted */);
/* THE SAME CORRECTION THROUGH THE JOINT PASS, WITH A TEST ON THE CONDITIONING OF H IN THE VERDICT (opt-in, INSTEAD of
 * vors_trackers_enable_map_icp: legal exactly where that call is, and either one after the other is refused). Point-to-plane rows do not
 * constrain motion inside a plane, and nothing vors_trackers_enable_map_icp's verdict reads notices a slide; this stage differs from it in
 * three things and in nothing else (window, launches' order, hazards, what an accepted or rejected result does are that call's):
 * 1. The pass is vors_icp_points_joint's: list grey = the map's grey levels (vors_trackers_map's d_gray), frame grey = the level-0 grey
 *    plane of the promoted frame (the caller's d_gray; in dense mode the handle's copy of it), photo_scale_m and photo_huber_grey as there.
 *    photo_scale_m = 0 is the robust pass bit for bit. The pass's sums29 and photo counts are staged per sequence.
 * 2. The verdict (one text, lie.h map_icp_verdict_joint; host twin vors_map_icp_verdict_joint_host) is vors_trackers_enable_map_icp's,
 *    called as it stands, and ONLY BEHIND ACCEPTED: CONDITION when max_dilution_t > 0 and dilution_t <= max_dilution_t does not hold,
 *    then the same for dilution_r; in float, NaN fails — a system whose H has no Cholesky factor fails every bound that is on. The
 *    dilutions are vors_icp_condition's (section 2e) of the staged sums29, i.e. of the pass's FINAL evaluation at the pose it proposes.
 *    With both bounds 0 the verdict is vors_trackers_enable_map_icp's for every input; the dilutions are computed and recorded all the same.
 * 3. Beside every vors_map_icp_record there is a vors_map_icp_joint_record (section 2e), same indexing and lifetime: zeros for a sequence
 *    the call did not promote.
 * vors_trackers_map_icp works on such a handle unchanged; d_totals counts a CONDITION verdict as attempted and not accepted.
 * Launches per track call: vors_trackers_enable_map_icp's, with the joint evaluation kernel in the evaluation's place and APPLY replaced
 * by one that also takes the condition, plus the memset of the photo counts and one launch of one thread per sequence that resets the
 * joint records (ARM itself stays as it is). Measured (64 sequences of 640x480, 6 rounds): 0.180 ms per track call when
 * nothing promotes, against 0.159 ms for vors_trackers_enable_map_icp in the same session.
 * VORS_ERR_INVALID_ARGUMENT, nothing allocated: everything vors_trackers_enable_map_icp refuses (of params->icp), either enable called
 * before, photo_scale_m or photo_huber_grey negative or NaN, max_dilution_t or max_dilution_r negative or NaN. On top of
 * vors_trackers_enable_map_icp's memory the call allocates per sequence 116 bytes of sums, 8 of photo counts and a
 * vors_map_icp_joint_record (20 bytes), part of vors_trackers_workspace_bytes' figure and freed with the handle. No later call allocates. */
vors_status vors_trackers_enable_map_icp_joint(vors_trackers* t, const vors_map_icp_joint_params* params);
/* DEVICE pointer, owned by the handle and valid for its life, contents valid in stream order after the last track: d_joint_records [n],
 * entry for entry beside vors_trackers_map_icp's d_records (nullable). No joint stage on this handle: VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_map_icp_joint(const vors_trackers* t, const struct vors_map_icp_joint_record** d_joint_records);
/* THE AVERAGED MAP AS THE CORRECTION'S MODEL (opt-in on top of either correction and of the voxels' statistics; without
 * this call nothing changes: no launch, no allocation, no kernel argument on any existing path). With the voxel filter the map's lists
 * hold the FIRST point that fell into each voxel; the correction then aligns that one sample per voxel. With this call the pass reads,
 * in the lists' place, the centroid and mean grey of every observation of the voxel: in every track call, behind ARM and before the
 * ICP's first launch, one pass resolves the ranks of every promoted sequence's window — vors_trackers_map_voxel_means' rule (lie.h
 * voxel_mean with min_count, min_span; the first segment of a rank by the same search over the segment records) on the statistics as
 * they stood BEFORE this promotion's emission — into staging the handle owns, rank for rank: xyz_mean [n][capacity][3] f32 and gray_mean
 * [n][capacity] u8. A rank that fails gets voxel_mean's NaN triple and grey 0, which every gate of the ICP skips; nothing is compacted,
 * so the map's normals (the normal of the voxel's first point; there are no mean normals) stay aligned. The pass's xyz is the staging,
 * and with the joint stage its list grey is gray_mean. ARM, APPLY, the window, both verdicts and the ICP itself are what they were:
 * `considered` stays the ranks of the WINDOW, rejected ranks included, so min_match_ratio is a ratio of the whole window — a caller who
 * filters hard reads `kept` of the record below and sets the ratio accordingly.
 * Per sequence a vors_map_icp_means_record (section 2e) of the LAST track call: resolved = the window's length, kept = its passing ranks;
 * zeros for a sequence the call did not promote. Launches per track call: one memset of the records and one launch over n sequences (the
 * host cannot know which promote: a sequence with the window (0, 0) is left by its workgroups at once).
 * Legal after vors_trackers_enable_map_voxel_stats and after one of vors_trackers_enable_map_icp / _joint, before vors_trackers_init,
 * once. VORS_ERR_INVALID_ARGUMENT, nothing allocated and nothing enqueued: NULL handle, no statistics enabled, no correction enabled,
 * repeated call, call after init. The call allocates, as part of vors_trackers_workspace_bytes' figure and freed with the handle,
 * n * capacity * 13 + 8 n bytes; no later call allocates. vors_trackers_init zeroes staging and records on the stream. */
vors_status vors_trackers_enable_map_icp_means(vors_trackers* t, uint32_t min_count, uint32_t min_span);
/* DEVICE pointers, owned by the handle and valid for its life, contents valid in stream order after the last track, each nullable:
 * d_xyz_mean [n][capacity][3] f32, d_gray_mean [n][capacity] u8, d_records [n]. The staging holds, per sequence, whatever its windows
 * have written since init — a later window overwrites only its own ranks — and zero bytes elsewhere. Means not enabled:
 * VORS_ERR_INVALID_ARGUMENT. */
vors_status vors_trackers_map_icp_means(const vors_trackers* t, const float** d_xyz_mean, const uint8_t** d_gray_mean,
                                        const struct vors_map_icp_means_record** d_records);
void vors_trackers_destroy(vors_trackers* t);

/* ------------------------------------------------------------------------------------------------------------
 * 2. Batch of independent frame pairs — the data-parallel hot path. For each pair p:
 *      tracker = cfg.init(kf_depth[p], kf_gray[p]); tracker.track(cur_gray[p]); pose[p] = tracker.current_frame()
 *    i.e. vors_track.rs:46-62 for a 2-frame sequence, for n_pairs sequences at once.
 *    Images of pair p start at offset p*rows*cols. prev_poses7 (nullable) = current_frame_pose before track()
 *    (identity in the reference's init; the initial guess is its inverse, inverse_compositional.rs:177).
 * ---------------------------------------------------------------------------------------------------------- */
/* Host buffers (copies in and out; PCIe-inclusive). */
vors_status vors_track_pairs(const vors_config* cfg, int n_pairs, const uint8_t* kf_gray, const uint16_t* kf_depth,
                             const uint8_t* cur_gray, int rows, int cols, int layout, const float* prev_poses7,
                             float* out_poses7, int32_t* out_status, vors_pair_stats* out_stats /* nullable, n_pairs */);

/* Device-resident engine: buffers are DEVICE pointers (row-major), work is enqueued on `hip_stream`
 * (a hipStream_t passed as void*; NULL = default stream) and NOT synchronised: outputs are valid once the stream
 * reaches this point. Workspaces are allocated once at create() for up to max_pairs pairs. */
typedef struct vors_batch vors_batch;
/* Scheduling knobs (environment, read at create() — except VORS_DSO_SCAN and VORS_DSO_PLANES, which are read at every keyframe stage, and
 * VORS_PYRAMID_FUSED, which is read ONCE PER PROCESS, at the first pyramid, race-free; results stay within the stated tolerance whatever
 * their value — they only change how the same arithmetic is spread over the chip; tests/test_gpu_parity.py covers the variants):
 *   VORS_LM_BLOCK=64..1024       threads per frame pair in the per-pair LM kernel (default by batch size and mode)
 *   VORS_LM_SPLIT=0              dense mode: one per-pair kernel for all levels instead of evaluation rounds
 *   VORS_LM_SPLIT_LEVELS=n       dense mode: the n finest levels are solved by evaluation rounds (default: levels of >= 64 Ki pixels)
 *   VORS_LM_SPLIT_ROUNDS=n       rounds launched before per-pair workgroups finish the stragglers (default by batch size and by the number
 *                                of levels solved by rounds; the defaults of all these knobs come from tools/speed_sweep.py)
 *   VORS_LM_CHUNKS=n             partial-sum chunks per pair of a level-0 evaluation (default by batch size)
 *   VORS_KF_R=1|2|4|8            tree roots per wavefront in the coarse-to-fine keyframe kernel (default 4)
 *   VORS_NO_FASTDIV=1            plain IEEE division by the focal lengths (the verified 3-instruction form is bit-identical)
 *   VORS_DSO_PLANES=1            DSO mode: keyframe records through per-level inverse-depth planes instead of the sorted pick list
 *                                (same candidates and values; the lists then come out in raster instead of Morton order)
 *   VORS_DSO_SCAN=1              DSO mode: the usable picks from a pass over the stamp plane instead of the selection rounds' own list
 *                                (identical lists)
 *   VORS_DSO_ROUNDS_THREADS=n    DSO mode: threads per pair in the selection-rounds kernel, a multiple of 64 (default 768 from 512 pairs on,
 *                                else 1024: profiles/r04_dso_rounds_threads.log; read per launch)
 *   VORS_DSO_SORT=bitonic        DSO mode: the pick list ordered by round 3's bitonic network instead of the bucket sort (identical lists;
 *                                read per launch)
 *   VORS_REF_SORT_REGCAP=n       REFERENCE arithmetic: lists longer than n records take the multi-pass form of the column-major sort
 *                                (default 4096 = what the register-resident form holds; identical lists; read per launch)
 *   VORS_DSO_RECORDS_THREADS=512|1024  DSO mode: threads per pair in the sparse records kernel (default 512 from 512 pairs on, else 1024)
 *   VORS_PYRAMID_FUSED=0         mean pyramid one level per launch instead of up to five halvings in one (bit-identical; read once per process)
 *   VORS_IDEPTH_LEVEL12=1        dense mode: inverse-depth levels 1-2 in one pass + a halving launch instead of levels 1-3 in one (bit-identical)
 *   VORS_FUSED_EXACT_POINTS=n    FUSED arithmetic: levels of at most n points take (u, v) from the reference's own warp chain (candidate
 *                                lists) or run the whole EXACT evaluation (dense pixel levels); default 2500, re-derived in round 4 on
 *                                six draws of 64 sequences + 4096 pairs (profiles/r04_parity_sequences.md); 0 = the round-2 behaviour
 *   VORS_FUSED_SMALL=exact       FUSED arithmetic, candidate lists: the whole EXACT evaluation on those levels (round 3's rule) */
vors_status vors_batch_create(const vors_config* cfg, int max_pairs, int rows, int cols, vors_batch** out);
/* Same on an explicit HIP device (vors_batch_create = the calling thread's current device). The handle remembers its device: every
 * entry point switches to it for the call and restores the caller's current device; a hip_stream of another device is rejected with
 * VORS_ERR_INVALID_ARGUMENT. Device buffers passed to the handle must live on that device. */
vors_status vors_batch_create_on(int device, const vors_config* cfg, int max_pairs, int rows, int cols, vors_batch** out);
vors_status vors_batch_device(const vors_batch* b, int* device);
/* A dense handle of at least 4096 pairs runs a vors_batch_track_pairs call of at least 4096 pairs as two overlapped halves: pairs [0, h)
 * on the caller's stream, pairs [h, n_pairs) on an internal stream forked from it at entry and joined before return. The
 * call stays stream-ordered for the caller and capturable, and every output keeps its bits. VORS_BATCH_HALVES (read when the handle is
 * created; development and test knob): 0 turns this off, 1 forces it from 2 pairs on. */
vors_status vors_batch_track_pairs(vors_batch* b, int n_pairs, const uint8_t* d_kf_gray, const uint16_t* d_kf_depth,
                                   const uint8_t* d_cur_gray, const float* d_prev_poses7 /* nullable */,
                                   float* d_out_poses7, int32_t* d_out_status,
                                   vors_pair_stats* d_out_stats /* nullable */, void* hip_stream);
/* The three stages of the above, separately (keyframe data persists in the handle between calls):
 *   prepare_keyframes = mean_pyramid + precompute_multires_data        inverse_compositional.rs:83-85,105-161
 *   track_current     = mean_pyramid + coarse->fine LM + keyframe test  inverse_compositional.rs:177-224
 * LIFETIME CONTRACT (zero copy, like the reference, which MOVES the image into the pyramid as level 0, multires.rs:14-15):
 * the handle keeps the caller's POINTERS to level 0 and to the depth map, not copies.
 *   - VORS_CANDIDATES_DENSE: d_kf_gray and d_kf_depth are re-read by every track_current (points are recomputed from them on the
 *     fly); they must stay allocated and unchanged until the next prepare_keyframes on this handle or its destruction.
 *   - coarse-to-fine / DSO: they are read during prepare_keyframes only (everything later needs is in the handle's records);
 *     vors_batch_get_keyframe_image(level 0) still reads d_kf_gray.
 * track_current accepts n_pairs <= the n_pairs of the last prepare_keyframes (more would read keyframe slots never prepared) and
 * fails with VORS_ERR_INVALID_ARGUMENT otherwise. */
vors_status vors_batch_prepare_keyframes(vors_batch* b, int n_pairs, const uint8_t* d_kf_gray, const uint16_t* d_kf_depth,
                                         void* hip_stream);
vors_status vors_batch_track_current(vors_batch* b, int n_pairs, const uint8_t* d_cur_gray, const float* d_prev_poses7,
                                     float* d_out_poses7, int32_t* d_out_status, vors_pair_stats* d_out_stats,
                                     void* hip_stream);
/* Bytes of device workspace held by the handle. */
vors_status vors_batch_workspace_bytes(const vors_batch* b, uint64_t* bytes);
/* Per-stage kernel timing with HIP events recorded on hip_stream (non-blocking during a step).
 * ring = number of most recent steps kept per stage (0 disables). Stages: 0 keyframe pyramid, 1 keyframe
 * precompute, 2 current pyramid, 3 LM kernel (the dominant one). kernel_times() synchronises on the events it reads
 * and returns the durations (ms) of the last min(steps, ring) steps, oldest first. */
vors_status vors_batch_enable_kernel_timing(vors_batch* b, int ring);
vors_status vors_batch_kernel_times(vors_batch* b, int stage, float* ms_out, int capacity, int* n_out);
/* Most recent step only; pyramid_ms = keyframe + current pyramids; a value < 0 = not measured. */
vors_status vors_batch_last_kernel_ms(vors_batch* b, float* lm_ms, float* keyframe_ms, float* pyramid_ms);
void vors_batch_destroy(vors_batch* b);

/* Throughput mode for a continuous feed of independent batches: a ring of `depth` batch handles, each on its own internal stream.
 * The tail of a step leaves the GPU partly idle (dependent straggler rounds of the dense LM stage, the last workgroups of the per-pair
 * kernel), its body VALU- or bandwidth-bound: with consecutive steps on different streams the GPU fills one with the other. Measured on one
 * MI355X (round 6, profiles/r06_stage_times_512_vs_4096.log; bench.py `pipelined` reports the current figures), depth 3 — the optimum; 2 is
 * within 10 %, 4 and 6 are no better: 4096-pair steps +3 % (dense FUSED), +10 % (coarse-to-fine, DSO), +25-33 % (dense in the default REFERENCE
 * arithmetic: the straggler tail of its one-wavefront-per-pair kernel); 512-pair steps — BASELINE config 4's share per GPU, which alone leave
 * most of the chip idle — +20-45 %: the 4096 / 512 step-time ratio goes from 4.3-5.5 to 6.3-7.0 (FUSED) and 5.0-5.3 (REFERENCE). Every step is a
 * plain vors_batch_track_pairs — same results bit for bit; the price is `depth` workspaces. NOTE: the HIP runtime maps a process's streams onto
 * GPU_MAX_HW_QUEUES hardware queues (ROCm default 4) in creation order; a process that holds other streams besides the ring's (torch, a
 * dense handle's side lane, a second ring) should start with GPU_MAX_HW_QUEUES=8 in its environment, or two slots can share one queue and
 * run one after the other (measured: 0.61 instead of 0.46 ms per 512-pair step; bench.py sets it).
 *   submit: the slot's stream first waits for everything enqueued on hip_stream so far (the inputs, and earlier readers of the output
 *           buffers), then runs the step; nothing is synchronised. Buffers as for vors_batch_track_pairs, and they must stay valid
 *           until the step has completed. *ticket (nullable) identifies the step.
 *   wait:   host_sync = 0: hip_stream waits for the step (its outputs are then ordered on hip_stream); host_sync != 0: the calling
 *           thread blocks until the step has completed.
 *   drain:  the same for every step submitted so far.
 * device < 0 = the calling thread's current device. */
typedef struct vors_pipeline vors_pipeline;
vors_status vors_pipeline_create(int device, const vors_config* cfg, int depth, int max_pairs, int rows, int cols, vors_pipeline** out);
vors_status vors_pipeline_submit(vors_pipeline* p, int n_pairs, const uint8_t* d_kf_gray, const uint16_t* d_kf_depth,
                                 const uint8_t* d_cur_gray, const float* d_prev_poses7 /* nullable */, float* d_out_poses7,
                                 int32_t* d_out_status, vors_pair_stats* d_out_stats /* nullable */, void* hip_stream, int64_t* ticket);
vors_status vors_pipeline_wait(vors_pipeline* p, int64_t ticket, void* hip_stream, int host_sync);
vors_status vors_pipeline_drain(vors_pipeline* p, void* hip_stream, int host_sync);
void vors_pipeline_destroy(vors_pipeline* p);

/* Inspection of the keyframe data held by a batch handle (device -> host copies; tests and debugging).
 * level image (mean_pyramid, multires.rs:21-31), row-major rows_l x cols_l: */
vors_status vors_batch_get_keyframe_image(vors_batch* b, int pair, int level, uint8_t* out, int* rows, int* cols);
vors_status vors_batch_get_current_image(vors_batch* b, int pair, int level, uint8_t* out, int* rows, int* cols);
/* usable candidates of a level (extract_z + warp_jacobians, inverse_compositional.rs:260-341): up to `capacity`
 * points, xy int32[2n], idepth f32[n], jac f32[6n], tmpl u8[n] (all nullable). Order is the device slot order,
 * NOT the reference's column-major order: sort by (x, y) to compare. *n = number of usable candidates. */
vors_status vors_batch_get_points(vors_batch* b, int pair, int level, int capacity, int32_t* xy, float* idepth, float* jac,
                                  uint8_t* tmpl, int* n);

/* ------------------------------------------------------------------------------------------------------------
 * 2b. Several GPUs from ONE process (no torch, no MPI): what a Rust host calls for BASELINE config 4 (4096 pairs over 8 MI355X).
 *     Frame pairs are independent (a Tracker is self-contained: inverse_compositional.rs:31-34), so pairs shard by contiguous blocks —
 *     pair i lives on device floor(i / ceil(n / G)) — each device runs its own vors_batch on its own stream with no data-path exchange,
 *     and the ONLY collective is one all-gather of 8 f32 per pair (pose 7 + status) over RCCL / xGMI (ncclAllGather; 16 KiB per GPU for
 *     4096 pairs on 8 GPUs), after which every device holds all results. RCCL is loaded at run time (librccl.so) and only when the
 *     handle spans more than one device.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct vors_multi vors_multi;
/* n_devices <= 0: all visible devices; device_ids NULL: 0 .. n_devices-1. */
vors_status vors_multi_create(const vors_config* cfg, int n_devices, const int* device_ids, int max_pairs_per_device, int rows, int cols,
                              vors_multi** out);
int vors_multi_device_count(const vors_multi* m);
/* Version code of the RCCL the handle bound at run time (ncclGetVersion), 0 when the handle spans one device (RCCL not loaded). */
int vors_multi_rccl_version(const vors_multi* m);
/* Block of pairs owned by device slot k for a batch of n_pairs_total: [*first, *first + *count). */
vors_status vors_multi_shard(const vors_multi* m, int n_pairs_total, int k, int* first, int* count);
/* Device-resident: d_*[k] = device slot k's block (row-major images of ITS pairs, allocated on that device). Runs all devices
 * concurrently, gathers, and returns poses (n_pairs_total x 7) and statuses on the host. Synchronous. */
vors_status vors_multi_track_pairs(vors_multi* m, int n_pairs_total, const uint8_t* const* d_kf_gray, const uint16_t* const* d_kf_depth,
                                   const uint8_t* const* d_cur_gray, float* out_poses7, int32_t* out_status);
/* Host buffers (row-major, all pairs contiguous): uploads each block to its device first (PCIe-inclusive). */
vors_status vors_multi_track_pairs_host(vors_multi* m, int n_pairs_total, const uint8_t* kf_gray, const uint16_t* kf_depth,
                                        const uint8_t* cur_gray, float* out_poses7, int32_t* out_status);
void vors_multi_destroy(vors_multi* m);

/* One evaluation — eval_energy + compute_eval_data (lm_optimizer.rs:68-107) — of level `level` of pair `pair` as the handle holds it
 * after prepare_keyframes + track_current, at an explicit model (HOST pointer, 7 floats), in the given VORS_ARITH_* mode whatever the
 * handle's own: sums29 (HOST) = sum r^2 (Huber loss with huber_delta), n_inside, g[6], H upper triangle row-wise [21]. Synchronises.
 * This is the operator-level window on the tracker's own point sources; tests compare EXACT and FUSED through it. */
vors_status vors_batch_eval_level(vors_batch* b, int pair, int level, const float model7[7], int arithmetic, float sums29[29]);

/* What the go-on prediction of the dense FUSED evaluation rounds did with each of the first n_pairs pairs in the handle's last
 * track: log (HOST, n_pairs ints) = OR of the bits below over the pair's level-0 candidates; all zero on a handle without the prediction.
 * The prediction chooses a schedule, never a number, so no other output shows it: this is the window tests look through. Synchronises. */
#define VORS_PREDICT_FULL 1        /* a candidate was predicted to go on and evaluated in full at once ... */
#define VORS_PREDICT_FULL_GO_ON 2  /* ... and was accepted with the level going on: its g and H were kept */
#define VORS_PREDICT_FULL_STOP 4   /* ... and was accepted with the level ending there */
#define VORS_PREDICT_FULL_REJECTED 8 /* ... and was rejected */
#define VORS_PREDICT_MISSED 16     /* a candidate that could have been predicted was not, and was accepted with the level going on */
vors_status vors_batch_lm_predict_log(vors_batch* b, int n_pairs, int32_t* log);

/* The same evaluation for a whole batch, device-resident: what scoring candidate motions against a keyframe (relocalisation, loop-closure
 * verification, a sweep of the energy around a solution) and the pose information below are made of.
 * VORS_EVAL_FULL = eval_energy + compute_eval_data (lm_optimizer.rs:68-107), VORS_EVAL_ENERGY = eval_energy alone (lm_optimizer.rs:68-87). */
enum { VORS_EVAL_FULL = 0, VORS_EVAL_ENERGY = 1 };

/* For every pair p < n_pairs and every k < models_per_pair: one evaluation of level `level` of pair p as the handle holds it after
 * prepare_keyframes + track_current, at model d_models[(p * models_per_pair + k)], in the given VORS_ARITH_* mode.
 * Models: DEVICE, 7 floats each, consecutive models model_stride_bytes apart (0 = 28; sizeof(vors_pair_stats) lets the caller pass the
 * d_out_stats array of the last track directly with models_per_pair = 1: lm_model is its first field).
 * d_sums29: DEVICE [n_pairs * models_per_pair][29], layout of vors_batch_eval_level; VORS_EVAL_ENERGY fills [0], [1] and zeroes the rest.
 * Enqueued on hip_stream, NOT synchronised, no allocation after the first call on a handle (that call creates the pass's workspace, which
 * vors_batch_workspace_bytes counts from then on). The sums of a (pair, model) are the same bits whatever n_pairs, models_per_pair and
 * its place in the batch: EXACT / FUSED cut a level into chunks by its point count alone and add the chunk sums in index order (a level
 * whose GRID is one chunk — at most 16384 pixels, dense, or 4096 candidate slots — gives vors_batch_eval_level's bits; through the
 * addition of chunks a sum of -0.0 comes out as +0.0); REFERENCE gives the reference's sequential sums, one wavefront per evaluation. */
vors_status vors_batch_eval_pairs(vors_batch* b, int n_pairs, int level, int models_per_pair, const void* d_models, size_t model_stride_bytes,
                                  int arithmetic, int what, float* d_sums29, void* hip_stream);

/* POSE INFORMATION of one evaluation (29 sums) at the solution:
 *   info36 = H, the upper triangle sums[8..28] mirrored to the full 6x6 matrix (row-major);
 *   sigma2 = sums[0] / (n_inside - 6), the residual variance left after 6 fitted parameters;
 *   cov36  = sigma2 * H^-1, through a 6x6 Cholesky in FLOAT64, rounded to f32 at the end (symmetric).
 * cov36 is the covariance of the twist xi = (v, w) — the order of vors_se3_exp — in the parametrisation the reference's step uses:
 * true model = model * exp(xi)^-1 (lm_optimizer.rs:134-135). With Huber on, sums[0] is the Huber loss and H the weighted matrix: the same
 * formula then is an approximation. How well it is calibrated is not asserted anywhere and is NOT MEASURED yet (tools/eval_pairs_bench.py
 * is the tool for it; DESIGN.md 7b says where that stands): a relative weight between pairs, not an absolute uncertainty.
 * flags: bit 0 = n_inside <= 6, bit 1 = the Cholesky met a pivot that is not > 0; with either, cov36 and sigma2 are NaN; info36 is
 * written all the same.
 *
 * vors_batch_pose_information = vors_batch_eval_pairs (VORS_EVAL_FULL, the handle's own arithmetic, one model per pair) followed by that
 * algebra, all on the device. Outputs DEVICE, each nullable: info36 [n][36]; cov36 [n][36]; sigma2 [n]; flags [n]. Enqueued, not synchronised. */
vors_status vors_batch_pose_information(vors_batch* b, int n_pairs, int level, const void* d_models, size_t model_stride_bytes,
                                        float* d_info36, float* d_cov36, float* d_sigma2, int32_t* d_flags, void* hip_stream);

/* The same algebra on the host, from one set of 29 sums (host arithmetic, needs no GPU, like vors_lm_step). Outputs nullable. */
vors_status vors_pose_information_from_sums(const float sums29[29], float info36[36], float cov36[36], float* sigma2, int32_t* flag);

/* THE PER-POINT QUANTITIES of one evaluation, for a whole batch, device-resident: what the sums above are made of. For every pair
 * p < n_pairs, level `level` of pair p as the handle holds it after prepare_keyframes + track_current, at model d_models[p] (DEVICE, 7
 * floats each, model_stride_bytes apart: 0 = 28; sizeof(vors_pair_stats) takes the d_out_stats array of the last track, as in
 * vors_batch_eval_pairs). Outputs DEVICE, each nullable (at least one must be given):
 *   d_residuals [n_pairs][rows_l * cols_l]      interpolate(u, v) - template (lm_optimizer.rs:236-247): the RAW residual, no Huber weight
 *                                               whatever huber_delta is. Finite exactly where the point passes the strict inside test
 *                                               (lm_optimizer.rs:227-231), NaN everywhere else.
 *   d_warp_uv   [n_pairs][rows_l * cols_l][2]   (u, v) of warp (lm_optimizer.rs:213-219) for every usable candidate, inside or not;
 *                                               (NaN, NaN) at every pixel that is not one.
 *   d_hist      [n_pairs][VORS_RESIDUAL_BINS]   d_hist[p][min((int)|r|, 255)] counts the finite residuals of pair p: bins one grey level
 *                                               wide (|r| <= 255 up to float32 rounding of the interpolation); integer counts, independent of scheduling; their sum
 *                                               is n_inside of the evaluation.
 *   d_scale     [n_pairs][2]                    median |r| and 1.4826 median |r| read off d_hist (vors_residual_scale_from_hist, the same
 *                                               text on the device, bit for bit): a starting point for huber_delta. NEEDS d_hist: the
 *                                               pass keeps no histogram of its own, d_scale without d_hist is VORS_ERR_INVALID_ARGUMENT.
 * The planes have the KEYFRAME pixel geometry of the level, row-major rows_l x cols_l (the level's shape: floor halving), in every
 * candidate mode: element (y, x) belongs to the usable candidate of this level at pixel (x, y) — extract_z's set
 * (inverse_compositional.rs:260-279), the set vors_batch_get_points returns: a pixel with a candidate whose inverse depth is known.
 * The arithmetic is always the reference's per point (what VORS_ARITH_REFERENCE and VORS_ARITH_EXACT evaluate: residuals bit-identical to
 * the reference's), whatever the handle's: there is no arithmetic argument. A VORS_ARITH_FUSED track minimises values a few ulp away from
 * these (its warp and its interpolation are shorter, algebraically equivalent forms), and a point within rounding of the window border may
 * be inside for one and outside for the other.
 * Enqueued on hip_stream, NOT synchronised, no allocation ever (the pass has no workspace: vors_batch_workspace_bytes does not change). In
 * dense mode the keyframe's d_kf_gray / d_kf_depth must still be alive, as for vors_batch_track_current. Touches nothing track computes or reads.
 * vors_trackers handles are out of scope, for the reason given for the pose information: a track may promote the current
 * frame to keyframe before the caller can ask, so the pair that was solved no longer exists in the handle. */
#define VORS_RESIDUAL_BINS 256
vors_status vors_batch_residual_maps(vors_batch* b, int n_pairs, int level, const void* d_models, size_t model_stride_bytes,
                                     float* d_residuals, float* d_warp_uv, uint32_t* d_hist, float* d_scale, void* hip_stream);

/* The scale of a residual histogram on the host (host arithmetic, needs no GPU). In float64: n = sum of the bins (*n_inside),
 * target = n / 2, b = the first bin whose cumulative count reaches target, *median_abs = b + (target - cumulative count before b) / hist[b],
 * *sigma_mad = 1.4826 * that (the standard deviation of a normal distribution with this median of |r|), each rounded to f32 at the end.
 * The median is exact to within the bin width (one grey level). n = 0: both NaN, status VORS_OK. Outputs nullable. */
vors_status vors_residual_scale_from_hist(const uint32_t hist[VORS_RESIDUAL_BINS], float* median_abs, float* sigma_mad, uint32_t* n_inside);

/* DEPTH REPROJECTION of a prepared batch, device-resident: where the keyframe's depth lands in the current frame (a forward warp with a
 * z-buffer), and whether it agrees with the depth the sensor measured there — the current depth map the reference's Tracker::track takes
 * in every call (inverse_compositional.rs:170-176) but uses only when the frame becomes a keyframe. Needs vors_batch_prepare_keyframes
 * ONLY: no current image and no current pyramid is read, so the pass is legal before any track_current; n_pairs <= the n_pairs of the last
 * prepare. d_models / model_stride_bytes as in vors_batch_residual_maps (DEVICE, 7 floats each; 0 = 28; sizeof(vors_pair_stats) takes the
 * d_out_stats array of the last track).
 * For every usable point i of level `level` of pair p (extract_z's set, inverse_compositional.rs:260-279, the set vors_batch_get_points
 * returns and the planes above mark; in dense mode it includes the zero-gradient border of level 0):
 *   P' = M * back_project(x, y, 1 / idepth), (u, v) = project(P') / P'.z — warp, lm_optimizer.rs:213-219, in the reference's per-point
 *   arithmetic: (u, v) have the bits vors_batch_residual_maps writes to d_warp_uv — and Z' = P'.z.
 *   The point LANDS iff Z' > 0 and fu = floorf(u + 0.5f), fv = floorf(v + 0.5f) satisfy 0 <= fu < cols_l, 0 <= fv < rows_l (all compares in
 *   float: NaN and huge values fail them), at the pixel q = (int)fv * cols_l + (int)fu of the CURRENT frame.
 * Outputs DEVICE, each nullable (at least one must be given):
 *   d_pred_z         [n_pairs][rows_l * cols_l]  current frame: the minimum Z' (metres) over the points that land at the pixel — the
 *                                                nearest surface wins —, +inf where none lands. Bitwise reproducible (a minimum does not
 *                                                depend on the order of arrival).
 *   d_pred_depth     [n_pairs][rows_l * cols_l]  current frame: to_depth(depth_scale, 1.0f / z) of d_pred_z (inverse_depth.rs:37-42, see
 *                                                vors_to_depth), 0 where it is +inf. NEEDS d_pred_z: the pass keeps no plane of its own,
 *                                                d_pred_depth without d_pred_z is VORS_ERR_INVALID_ARGUMENT.
 *   d_depth_residual [n_pairs][rows * cols]      KEYFRAME geometry: Z' - (float)d_cur_depth[p][q] / depth_scale at each point that lands on a
 *                                                pixel with non-zero current depth, NaN at every other pixel. Needs d_cur_depth (and so
 *                                                level 0).
 *   d_counts         [n_pairs][4]                {usable points, points that land, those with a current depth, those with |residual| <=
 *                                                tol_m}; the last two are 0 without d_cur_depth. Integers, independent of scheduling.
 * d_cur_depth [n_pairs][rows * cols] (DEVICE, nullable): the current frames' depth maps, 0 = unknown; level 0 only (depth maps exist at full
 * resolution only). Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: d_cur_depth with level != 0, d_depth_residual without
 * d_cur_depth, negative or NaN tol_m, no output at all, a level out of range, a stream of another device.
 * Contracts of vors_batch_residual_maps: enqueued on hip_stream, NOT synchronised, no allocation ever (vors_batch_workspace_bytes does not
 * change); in dense mode the keyframe's d_kf_gray / d_kf_depth must still be alive; touches nothing track computes or reads; always the
 * reference's per-point arithmetic whatever the handle's; vors_trackers handles are out of scope. */
vors_status vors_batch_reproject_depth(vors_batch* b, int n_pairs, int level, const void* d_models, size_t model_stride_bytes,
                                       const uint16_t* d_cur_depth /* nullable */, float tol_m,
                                       float* d_pred_z, uint16_t* d_pred_depth, float* d_depth_residual, uint32_t* d_counts,
                                       void* hip_stream);

/* POINT CLOUDS of a prepared batch, device-resident: the keyframe's usable points of level `level` as a LIST per pair, in 3-D, in a common
 * frame — Camera::back_project (camera.rs:43-45): extrinsics::back_project(pose, intrinsics.back_project(point, depth)) — by an ordered,
 * deterministic stream compaction. Needs vors_batch_prepare_keyframes ONLY (legal before any track_current); n_pairs <= the n_pairs of the
 * last prepare.
 * d_poses7 (DEVICE, nullable): 7 floats per pair, pose_stride_bytes apart (0 = 28; sizeof(vors_pair_stats) takes a d_out_stats array):
 *   the keyframe camera -> world pose, Camera::extrinsics. NULL = identity for every pair: NO transform is applied, the camera-frame
 *   bits come out untouched.
 * d_keep (DEVICE, nullable) [n_pairs][rows_l * cols_l], keyframe geometry of the level: non-zero = keep; NULL keeps everything. The masks
 *   of vors_batch_residual_maps / vors_batch_reproject_depth feed in here once the caller has thresholded them into bytes.
 * The points of pair p are the usable points of the level (extract_z's set: what vors_batch_get_points returns and the planes above
 * mark), with d_keep only those whose byte is non-zero, in ascending slot order of the level's source: dense mode = row-major raster
 * order of the pixels; candidate lists = the order of vors_batch_get_points (which depends on the handle's arithmetic, see there). The
 * order is a function of the pair's own data alone — never of scheduling or of the batch around the pair. For the point of rank
 * i < capacity:
 *   d_xyz   [n_pairs][capacity][3]  pose * back_project(K_level, (float)x, (float)y, 1.0f / idepth): the reference's per-point arithmetic,
 *                                   the bits vors_camera_back_project gives for the same inputs (rows of 12 bytes)
 *   d_pixel [n_pairs][capacity]     x | y << 16
 *   d_gray  [n_pairs][capacity]     the template intensity of the level
 *   d_counts[n_pairs]               the TOTAL number of points of the pair, which may exceed capacity
 * Exactly the first min(count, capacity) entries of each list are written; the entries beyond them are left untouched. Every output is
 * nullable, at least one must be given; capacity > 0 is required iff one of the three lists is given; d_counts alone runs only the
 * counting pass. Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: no output at all, a level out of range, a negative capacity
 * (or 0 with a list), n_pairs beyond the prepared count, a stream of another device.
 * Contracts of vors_batch_residual_maps: enqueued on hip_stream, NOT synchronised; no allocation after the first call on a handle (the
 * first call creates the per-(pair, chunk) count workspace, which vors_batch_workspace_bytes counts from then on); in dense mode the
 * keyframe's d_kf_gray / d_kf_depth must still be alive; touches nothing track computes or reads; vors_trackers handles are out of
 * scope: the sequence handles have their own switch, vors_trackers_enable_map / vors_tracker_enable_map (section 1,
 * DESIGN.md 7h). Two launches ordered by the stream; no workgroup waits for another and there is no atomic. */
vors_status vors_batch_point_cloud(vors_batch* b, int n_pairs, int level,
                                   const void* d_poses7 /* nullable */, size_t pose_stride_bytes,
                                   const uint8_t* d_keep /* nullable */, int capacity,
                                   float* d_xyz, uint32_t* d_pixel, uint8_t* d_gray, uint32_t* d_counts,
                                   void* hip_stream);

/* DEPTH FUSION of a prepared batch, device-resident: the keyframe's depth carried into the current frame and MERGED with the depth the
 * sensor measured there, into a depth map and a weight map in the current frame's geometry — the maps the caller hands to the next
 * vors_batch_prepare_keyframes (the depth) and to the next fuse call (the weight): a recursive per-pixel depth filter around a tracker
 * that otherwise drops all depth knowledge of the old keyframe the moment a new frame is promoted. Level 0 only (depth maps exist at full
 * resolution only). Needs vors_batch_prepare_keyframes ONLY; n_pairs <= the n_pairs of the last prepare. d_models / model_stride_bytes as in
 * vors_batch_reproject_depth (DEVICE, 7 floats each; 0 = 28; sizeof(vors_pair_stats) takes the d_out_stats array of the last track).
 * SPLAT. The points are the usable points of level 0 (extract_z's set) whose d_kf_weight byte is non-zero; d_kf_weight (DEVICE, nullable)
 *   [n_pairs][rows * cols] in KEYFRAME geometry, NULL = weight 1 everywhere; a zero byte removes the point, so the plane doubles as a keep
 *   mask. Each point is warped and LANDS by the rule of vors_batch_reproject_depth, unchanged (Z' > 0, floorf(u + 0.5f), floorf(v + 0.5f)
 *   inside the window, all compares in float), at the pixel q of the CURRENT frame.
 *   d_zkey [n_pairs][rows * cols] (DEVICE, REQUIRED, 8-byte aligned; the pass keeps no plane of its own): the minimum over the points
 *   landing at q of (uint64)bits(Z') << 32 | src, src = y * cols + x of the keyframe pixel; VORS_ZKEY_EMPTY where no point lands. The
 *   nearest surface wins, among equal Z' bits the smallest source index: a minimum, bitwise reproducible whatever the order of arrival.
 *   key >> 32 has the bits of d_pred_z; the plane is an output in its own right, a current -> keyframe correspondence map.
 * MERGE, per current pixel q, with has_p = key != VORS_ZKEY_EMPTY, zp = the float of bits key >> 32, wk = d_kf_weight ?
 *   d_kf_weight[key & 0xFFFFFFFF] : 1, d = d_cur_depth[q], has_m = d != 0, r = zp - (float)d / depth_scale (the depth residual's text):
 *     case                              condition                                   fused depth                    fused weight          counter
 *     agree                             has_p && has_m && fabsf(r) <= tol_m         to_depth(scale, MEAN)          min(wk + 1, max_weight)  0
 *     conflict, prediction in front     has_p && has_m && r < -tol_m                d                              1                        1
 *     conflict, prediction behind       has_p && has_m && r > tol_m                 d                              1                        2
 *     measured only                     !has_p && has_m                             d                              1                        3
 *     filled                            has_p && !has_m && fill_min_weight > 0      to_depth(scale, 1.0f / zp)     wk                       4
 *                                         && wk >= fill_min_weight                  (the bits of d_pred_depth)
 *     empty                             everything else                             0                              0                        5
 *   MEAN = ((float)wk * (1.0f / zp) + depth_scale / (float)d) / ((float)wk + 1.0f): the weighted mean in INVERSE depth, the measurement
 *   inverted exactly as vors_from_depth does (scale / (float)d), in this expression order on host and device. A fused depth that rounds to
 *   0 (a surface nearer than half a depth unit) gets weight 0: a depth of 0 and a weight of 0 always coincide.
 *   d_fused_depth [n_pairs][rows * cols] u16, d_fused_weight [n_pairs][rows * cols] u8, d_counts [n_pairs][VORS_FUSE_COUNTS] (the six
 *   counters of a pair add up to rows * cols): DEVICE, each nullable. d_zkey alone is legal: the pass is then only the splat.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: NULL b, d_models, d_cur_depth or d_zkey; a misaligned d_zkey; tol_m negative or
 * NaN; max_weight outside 1..255; fill_min_weight outside 0..255 (0 = never fill); a bad stride; n_pairs out of range; no
 * prepare_keyframes; a stream of another device.
 * Contracts of vors_batch_reproject_depth: enqueued on hip_stream, NOT synchronised, no allocation ever (vors_batch_workspace_bytes does not
 * change); in dense mode the keyframe's d_kf_gray / d_kf_depth must still be alive; touches nothing track computes or reads; always the
 * reference's per-point arithmetic whatever the handle's. Not available on the batch of a vors_trackers / vors_tracker handle: the
 * sequence handles have their own switch, vors_trackers_enable_depth_filter / vors_tracker_enable_depth_filter (section 1). */
#define VORS_FUSE_COUNTS 6
#define VORS_ZKEY_EMPTY 0xFFFFFFFFFFFFFFFFull
vors_status vors_batch_fuse_depth(vors_batch* b, int n_pairs, const void* d_models, size_t model_stride_bytes,
                                  const uint16_t* d_cur_depth, float tol_m,
                                  const uint8_t* d_kf_weight /* nullable */, int max_weight, int fill_min_weight,
                                  uint64_t* d_zkey, uint16_t* d_fused_depth /* nullable */, uint8_t* d_fused_weight /* nullable */,
                                  uint32_t* d_counts /* nullable */, void* hip_stream);
/* The merge alone for arrays on the host (the text the device kernel runs; needs no GPU): n_pixels keys and measured depths ->
 * fused_depth, fused_weight, counts (each nullable). kf_weight (nullable) has n_kf_pixels entries. Refused with
 * VORS_ERR_INVALID_ARGUMENT, nothing written: NULL zkey or cur_depth, depth_scale not > 0, the tol_m / max_weight / fill_min_weight
 * refusals above, and a key other than VORS_ZKEY_EMPTY whose source index is >= n_kf_pixels (checked with or without kf_weight). */
vors_status vors_fuse_depth_pixels(float depth_scale, float tol_m, int max_weight, int fill_min_weight, size_t n_pixels,
                                   const uint64_t* zkey, const uint16_t* cur_depth,
                                   const uint8_t* kf_weight /* nullable */, size_t n_kf_pixels,
                                   uint16_t* fused_depth, uint8_t* fused_weight, uint32_t counts[VORS_FUSE_COUNTS] /* each nullable */);

/* ------------------------------------------------------------------------------------------------------------
 * 2c. RENDERING OF POINT LISTS INTO A CAMERA, device-resident and handle-free (like the renderer of section 5): n world-frame lists
 *     xyz / gray — exactly the pointers of vors_trackers_map and of vors_batch_point_cloud — seen from one pose per list, as a z-buffered
 *     u16 depth map and u8 grey image in the camera's geometry: the arguments of vors_tracker_create, vors_batch_prepare_keyframes and
 *     vors_trackers_init. (Camera::project, camera.rs:36-39, per point; the reference has no renderer.)
 * Lists: d_xyz [n][capacity][3] f32, d_list_gray [n][capacity] u8, d_list_counts [n] u32 (a count above capacity is clipped to it).
 * d_ranges (DEVICE, nullable): per list a pair of u32 (first, count), range_stride_bytes apart (0 = 8; a multiple of 4 of at least 8):
 *   only the ranks first <= rank < first + count take part, clipped to the written prefix; NULL = the whole list.
 * Camera: cam5 (HOST) = cu cv fu fv skew, rows x cols, depth_scale; d_poses7 (DEVICE, nullable): camera -> world, Camera::extrinsics, 7
 *   floats per list, pose_stride_bytes apart (0 = 28; a multiple of 4 of at least 28); NULL = no transform at all (the lists are already
 *   in the camera frame), the rule of vors_batch_point_cloud.
 * PER POINT w of rank r: c = rotation.inverse() * (translation.inverse() * w) (camera.rs:70-72), Z' = c.z, (u, v) = project(c) / c.z:
 *   (u Z', v Z', Z') are the bits of vors_camera_project. The anchor (x0f, y0f) is (floorf(u + 0.5f), floorf(v + 0.5f)) for footprint 1
 *   and 3 and (floorf(u), floorf(v)) for footprint 2. The point is a candidate iff Z' > 0, -4.0f <= x0f < (float)cols + 4.0f and
 *   -4.0f <= y0f < (float)rows + 4.0f, compared in float before any integer conversion (NaN and huge values fail). Footprint 1: the
 *   anchor pixel (the landing rule of vors_batch_reproject_depth); 2: the four pixels x0 + {0, 1}, y0 + {0, 1}; 3: the nine pixels
 *   x0 + {-1, 0, 1}, y0 + {-1, 0, 1}. A footprint pixel is written iff it lies inside [0, cols) x [0, rows), tested in integers; the point
 *   LANDS iff at least one is.
 * d_zkey [n][rows * cols] (DEVICE, REQUIRED, 8-byte aligned): the minimum over the points written at the pixel of
 *   (uint64)bits(Z') << 32 | r; VORS_ZKEY_EMPTY where none is. The nearest surface wins, among equal Z' bits the lowest rank: bitwise
 *   reproducible whatever the order of arrival. d_zkey alone is the splat alone.
 * d_depth [n][rows * cols] u16 = to_depth(depth_scale, 1.0f / Z') of the key (the bits of d_pred_depth), 0 where empty; d_gray
 *   [n][rows * cols] u8 = d_list_gray at the key's rank, 0 where empty; d_counts [n][VORS_RENDER_COUNTS] u32 = {considered: the ranks in
 *   the clipped range; in_front: those with Z' > 0; landed; covered: the pixels whose key is not empty}. DEVICE, each nullable.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: n < 1; a NULL list (d_xyz, d_list_gray, d_list_counts) or cam5; a NULL or
 * misaligned d_zkey; footprint outside 1..3; rows, cols or capacity < 1; rows or cols > 65535 or rows * cols > 2^28 (the plane limits of
 * vors_batch_create); depth_scale not > 0; a bad stride; a pointer off its natural alignment (d_xyz, d_list_counts, d_ranges, d_poses7,
 * d_counts: 4 bytes; d_depth: 2 bytes). Enqueued on hip_stream on the calling thread's current device, NOT synchronised, no allocation
 * ever. The fill of the key plane, a memset of the counters when they are asked for, the splat kernel and — with any of d_depth, d_gray,
 * d_counts — the resolve kernel, ordered by the stream; no workgroup waits for another. */
#define VORS_RENDER_COUNTS 4
vors_status vors_render_points(int n, const float* d_xyz, const uint8_t* d_list_gray, const uint32_t* d_list_counts, int capacity,
                               const void* d_ranges /* nullable */, size_t range_stride_bytes,
                               const float cam5[5], int rows, int cols, float depth_scale,
                               const void* d_poses7 /* nullable */, size_t pose_stride_bytes, int footprint,
                               uint64_t* d_zkey, uint16_t* d_depth /* nullable */, uint8_t* d_gray /* nullable */,
                               uint32_t* d_counts /* nullable */, void* hip_stream);
/* The same rule for ONE list on the host (host arithmetic, needs no GPU; the text the kernels run): HOST pointers, count = the list's
 * count (clipped to capacity), range2 (nullable) = (first, count), pose7 (nullable) = camera -> world. Outputs zkey [rows * cols] (required
 * here too: it is the z-buffer), depth, gray, counts (each nullable). The refusals above, with nothing written. */
vors_status vors_render_points_host(const float* xyz, const uint8_t* list_gray, uint32_t count, int capacity, const uint32_t range2[2],
                                    const float cam5[5], int rows, int cols, float depth_scale, const float pose7[7], int footprint,
                                    uint64_t* zkey, uint16_t* depth, uint8_t* gray, uint32_t counts[VORS_RENDER_COUNTS]);
/* THE AVERAGED LIST OF VOXEL STATISTICS (vors_trackers_enable_map_voxel_stats, section 2), device-resident and handle-free,
 * in the shape this section's and the next sections' passes take: n lists d_xyz [n][capacity][3] / d_list_counts [n] with statistics
 * d_sums [n][capacity][4] int64 / d_obs [n][capacity][2] u32 — the pointers of vors_trackers_map and vors_trackers_map_voxel_stats —
 * resolved per rank r below min(count, capacity), with f = d_xyz[r]:
 *   mean_a = f_a + voxel_m * (float)((double)sums_a / ((double)count * 1048576.0)), the division and conversions in IEEE f64;
 *   grey   = (uint8)((2 * sum_grey + count) / (2 * count)) in integers.
 * A rank with count < max(min_count, 1), or with last_segment - first_segment < min_span, gets a NaN triple (bits 0x7FC00000) and grey 0.
 * The candidate test of vors_render_points and every ICP gate are written so that NaN fails: such a rank is skipped by every consumer
 * without compaction, and the list stays rank-aligned with vors_trackers_map_normals. d_first_segment_of_rank [n][capacity] u32
 * (nullable): the segment index of every rank's own keyframe; NULL = no span test, and min_span must then be 0. Nothing of the map's
 * grey list is read (the mean grey comes from the sums). Outputs, each nullable, at least one required: d_xyz_mean [n][capacity][3] f32,
 * d_gray_mean [n][capacity] u8 — ranks at or beyond the clipped count are not written — and d_kept [n] u32, the passing ranks.
 * VORS_ERR_INVALID_ARGUMENT, nothing enqueued: n outside 1..65535, a NULL list, no output at all, d_sums not 8-byte aligned, a 4-byte
 * array not 4-byte aligned, voxel_m not finite or <= 0, capacity < 1, min_span != 0 without d_first_segment_of_rank. The call allocates
 * nothing; the clear of d_kept and one launch are enqueued on hip_stream, NOT synchronised. */
vors_status vors_voxel_means(int n, const float* d_xyz, const uint32_t* d_list_counts, int capacity, const int64_t* d_sums,
                             const uint32_t* d_obs, float voxel_m, uint32_t min_count, uint32_t min_span,
                             const uint32_t* d_first_segment_of_rank /* nullable */, float* d_xyz_mean /* nullable */,
                             uint8_t* d_gray_mean /* nullable */, uint32_t* d_kept /* nullable */, void* hip_stream);
/* The same resolve for ONE list in HOST memory (no GPU): the text the kernel runs, bit for bit. Same refusals. */
vors_status vors_voxel_means_host(const float* xyz, uint32_t count, int capacity, const int64_t* sums, const uint32_t* obs, float voxel_m,
                                  uint32_t min_count, uint32_t min_span, const uint32_t* first_segment_of_rank /* nullable */,
                                  float* xyz_mean /* nullable */, uint8_t* gray_mean /* nullable */, uint32_t* kept /* nullable */);
/* The statistics themselves for ONE unfiltered list U in HOST memory (no GPU): what the device map of a sequence holds after the
 * keyframes that make up U. xyz [n][3], gray [n], segment_of [n] (nullable = all 0): U's entries and the segment index of each. The
 * filtered list is U at the first occurrence of every voxel key, in U's order: *total (nullable) its unclipped length, first_index
 * [min(total, capacity)] (nullable) the index in U of every rank's first point. sums [capacity][4] and obs [capacity][2] are required
 * and written whole (zeros beyond the filtered list). Refused: a NULL list with n > 0, NULL sums or obs, voxel_m not finite or <= 0,
 * capacity < 1. */
vors_status vors_voxel_stats_host(const float* xyz, const uint8_t* gray, const uint32_t* segment_of /* nullable */, uint32_t n, float voxel_m,
                                  int capacity, uint32_t* total /* nullable */, uint32_t* first_index /* nullable */, int64_t* sums,
                                  uint32_t* obs);

/* ------------------------------------------------------------------------------------------------------------
 * 2d. SURFACE NORMALS OF DEPTH MAPS, device-resident and handle-free (the reference has no normals): per pixel of a level-0
 *     depth plane D (u16, rows x cols, row-major) the unit normal of the surface through its back-projected neighbours.
 * PER PIXEL (x, y): z(d) = 1.0f / (depth_scale / (float)d) (vors_from_depth's text, then the reciprocal the point cloud takes) and
 *   P(x', y') = back_project(K, (float)x', (float)y', z(D[y'][x'])): the centre P_c has the camera-frame bits of vors_batch_point_cloud
 *   without a pose. No normal if (x, y) is outside the plane or D[y][x] == 0. A neighbour is usable iff it lies inside the plane, its depth
 *   is non-zero and fabsf(z_n - z_c) <= jump_m, compared in float (NaN fails). Horizontal tangent tx from (x - step, y) and (x + step, y):
 *   both usable P(x + step) - P(x - step); only the right one P(x + step) - P_c; only the left one P_c - P(x - step); neither: no normal.
 *   Vertical tangent ty: the same with (x, y -/+ step). m = cross(ty, tx), l2 = (m.x m.x + m.y m.y) + m.z m.z, no normal unless
 *   l2 > 0.0f; n = m / sqrtf(l2) (three divisions), negated if (n.x P_c.x + n.y P_c.y) + n.z P_c.z > 0.0f: the normal faces the camera
 *   whatever the signs of the focal lengths and the skew. With a pose the normal is rotated by the pose's rotation (no translation);
 *   without one it is untouched. "No normal" is stored as three +0.0f. The one text (lie.h depth_normal) runs on the host and on the
 *   device: the device results equal vors_depth_normals_host's bit for bit.
 * Counts: VORS_NORMAL_COUNTS u32 per plane / list = {considered: the pixels of the plane resp. the ranks of the clipped range; with
 *   depth: those inside the plane whose depth is non-zero; with a normal}.
 * vors_depth_normals (PLANE form): d_depth [n][rows * cols] u16, cam5 (HOST) = cu cv fu fv skew, d_poses7 (DEVICE, nullable): camera ->
 *   world, 7 floats per plane, pose_stride_bytes apart (0 = 28; a multiple of 4 of at least 28). Outputs (DEVICE, each nullable, at least
 *   one required): d_normals [n][rows * cols][3] f32, every pixel written; d_counts [n][VORS_NORMAL_COUNTS].
 * vors_points_normals (LIST form): the normals of listed pixels of the planes: d_pixel [n][capacity] u32 = x | y << 16 and d_list_counts
 *   [n] u32 (a count above capacity is clipped to it) are the pointers of vors_batch_point_cloud and vors_trackers_map; d_ranges /
 *   range_stride_bytes and d_poses7 / pose_stride_bytes as in vors_render_points. Outputs: d_normals [n][capacity][3] — exactly the ranks
 *   of the clipped range are written, everything else is left untouched — and d_counts. A listed pixel outside the plane has no normal.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued and nothing written: n < 1; a NULL d_depth or cam5 (list form: d_pixel,
 *   d_list_counts); both outputs NULL; step outside 1..8; jump_m negative or NaN; depth_scale not > 0; rows or cols < 1 (list form:
 *   capacity < 1); rows or cols > 65535 or rows * cols > 2^28; a bad stride; a pointer off its natural alignment (d_depth: 2 bytes, the
 *   others: 4). Enqueued on hip_stream on the calling thread's current device, NOT synchronised, no allocation ever: a memset of the
 *   counters when they are asked for and one kernel; no workgroup waits for another. */
#define VORS_NORMAL_COUNTS 3
vors_status vors_depth_normals(int n, const uint16_t* d_depth, const float cam5[5], int rows, int cols, float depth_scale, int step,
                               float jump_m, const void* d_poses7 /* nullable */, size_t pose_stride_bytes,
                               float* d_normals /* nullable */, uint32_t* d_counts /* nullable */, void* hip_stream);
vors_status vors_points_normals(int n, const uint16_t* d_depth, const uint32_t* d_pixel, const uint32_t* d_list_counts, int capacity,
                                const void* d_ranges /* nullable */, size_t range_stride_bytes,
                                const float cam5[5], int rows, int cols, float depth_scale, int step, float jump_m,
                                const void* d_poses7 /* nullable */, size_t pose_stride_bytes,
                                float* d_normals /* nullable */, uint32_t* d_counts /* nullable */, void* hip_stream);
/* The same rule for ONE plane — or, with pixel non-NULL, ONE list — on the host (host arithmetic, needs no GPU; the text the kernels run):
 * HOST pointers. Plane form (pixel NULL; count, capacity and range2 are not read): normals [rows * cols][3]. List form: pixel [capacity],
 * count = the list's count (clipped to capacity), range2 (nullable) = (first, count), normals [capacity][3], only the ranks of the clipped
 * range written. pose7 (nullable) = camera -> world. The refusals above, with nothing written. */
vors_status vors_depth_normals_host(const uint16_t* depth, const float cam5[5], int rows, int cols, float depth_scale, int step, float jump_m,
                                    const float pose7[7], const uint32_t* pixel, uint32_t count, int capacity, const uint32_t range2[2],
                                    float* normals, uint32_t counts[VORS_NORMAL_COUNTS]);

/* ------------------------------------------------------------------------------------------------------------
 * 2e. POINT-TO-PLANE ICP OF POINT LISTS WITH NORMALS AGAINST DEPTH FRAMES, device-resident and handle-free (the reference
 *     has none): refine one camera -> world pose per list so that the measured level-0 depth plane lies on the planes of the model.
 * Lists: d_xyz / d_normals [n][capacity][3] f32 in the world frame (a normal of three zeros = no normal) and d_list_counts [n] u32 —
 *   the pointers of vors_trackers_map / vors_trackers_map_normals and of vors_batch_point_cloud / vors_points_normals; d_ranges /
 *   range_stride_bytes and d_poses7_in / pose_stride_bytes as in vors_render_points, except that the poses are REQUIRED. d_depth
 *   [n][rows * cols] u16, cam5 (HOST) = cu cv fu fv skew, depth_scale.
 * PER POINT of rank r at the pose T: c = extr_project(T, w); the landing pixel (x, y) is vors_render_points' footprint-1 anchor
 *   (floorf(u + 0.5f), floorf(v + 0.5f)), with its float comparisons before any integer conversion, and must lie inside the plane (tested
 *   in integers). MATCHED iff the point is such a candidate, its normal is not three zeros, d = D[y][x] != 0 and, with
 *   q = back_project(K, (float)x, (float)y, 1.0f / (depth_scale / (float)d)) and e = q - c, dot3(e, e) <= dist_m * dist_m in float (NaN
 *   fails). n = conj(T.q) * nw; residual r = dot3(n, e); Jacobian row J = (n, cross(q, n)), translational three first (se3_exp's order).
 *   A matched point contributes r r, J[i] r (6) and J[i] J[j] for i <= j row-wise (21) — sums29's slots 0, 2..7, 8..28 — and 1 to the
 *   matched count; an unmatched one +0.0f to every sum.
 * ORDER OF THE SUMS (part of the definition): the clipped range [first, first + count) is cut into chunks of 1024 consecutive ranks from
 *   `first`; slot s is a rank's offset in its chunk, slots beyond the range hold zeros. Chunk sum: for (w = 512; w >= 1; w /= 2)
 *   v[s] = v[s] + v[s + w] for s < w, in f32, per product. List sum: the chunk sums added sequentially in ascending chunk order, starting
 *   from chunk 0's. Counts are integers. The result depends neither on capacity nor on the grid or the schedule; the device equals
 *   vors_icp_points_host bit for bit.
 * LOOP per list, no host round trip: `iters` times evaluate, solve, update; then ONE final evaluation at the returned pose, which is what
 *   d_stats, d_sums29 and d_residuals describe (iters = 0: a pure evaluator at the given poses). The update is vors_lm_step's:
 *   H mirrored from the 21 sums, g = the 6, lm_coef = damping, T' = renormalize(T * exp(delta)^-1). A list is FROZEN — its later
 *   rounds do nothing — when matched < min_points (VORS_ICP_TOO_FEW, pose kept), when the step is refused (VORS_ICP_SINGULAR, pose kept),
 *   or when after an update dot6(delta, delta) <= step_eps * step_eps (VORS_ICP_CONVERGED); otherwise VORS_ICP_ITERATIONS.
 * Outputs (DEVICE): d_poses7_out [n][7] (required, may alias d_poses7_in when packed alike); d_stats [n] vors_icp_stats; d_sums29 [n][29],
 *   the layout of vors_batch_eval_level with the matched count in slot 1, so that vors_pose_information_from_sums gives the ICP's
 *   information matrix and covariance; d_residuals [n][capacity] f32, NaN = not matched, exactly the ranks of the clipped range written.
 *   The last three are nullable. stats: iterations = updates applied; considered = ranks of the clipped range; matched, rms =
 *   sqrtf(sums[0] / (float)matched) (NaN without a matched point) of the final evaluation; last_step_norm = sqrtf(dot6(delta, delta)) of
 *   the last update (0 without one).
 * d_workspace (DEVICE, 4-byte aligned): vors_icp_workspace_bytes(n, capacity) bytes — the chunk partials [n][chunks][28] f32, the chunk
 *   counts and the per-list state; chunks = ceil(capacity / 1024). 0 for n < 1 or capacity < 1.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: n < 1; a NULL list, d_poses7_in, d_depth, cam5, d_workspace or d_poses7_out;
 *   rows, cols or capacity < 1; rows or cols > 65535 or rows * cols > 2^28; depth_scale not > 0; dist_m, damping or step_eps negative or
 *   NaN; iters outside 0..64; min_points < 6; a bad stride; a pointer off its natural alignment (d_depth: 2 bytes, the others: 4).
 * Enqueued on hip_stream on the calling thread's current device, NOT synchronised, no allocation ever: one launch that starts the state,
 *   per round one evaluation launch (grid = chunks x lists) and one solve launch (one wavefront per list), then the final evaluation and
 *   the launch that writes the outputs; no workgroup waits for another and no floating-point atomic exists. */
#define VORS_ICP_ITERATIONS 0
#define VORS_ICP_CONVERGED 1
#define VORS_ICP_TOO_FEW 2
#define VORS_ICP_SINGULAR 3
typedef struct vors_icp_stats {
    uint32_t status, iterations, considered, matched;
    float rms, last_step_norm;
} vors_icp_stats;
uint64_t vors_icp_workspace_bytes(int n, int capacity);
vors_status vors_icp_points(int n, const float* d_xyz, const float* d_normals, const uint32_t* d_list_counts, int capacity,
                            const void* d_ranges /* nullable */, size_t range_stride_bytes,
                            const void* d_poses7_in, size_t pose_stride_bytes, const uint16_t* d_depth,
                            const float cam5[5], int rows, int cols, float depth_scale,
                            float dist_m, float damping, float step_eps, int iters, int min_points, void* d_workspace,
                            float* d_poses7_out, vors_icp_stats* d_stats /* nullable */, float* d_sums29 /* nullable */,
                            float* d_residuals /* nullable */, void* hip_stream);
/* The same loop for ONE list on the host (host arithmetic, needs no GPU; the texts and the order of sums the kernels run): HOST pointers,
 * count = the list's count (clipped to capacity), range2 (nullable) = (first, count), depth [rows * cols]. No workspace. The refusals
 * above, with nothing written. */
vors_status vors_icp_points_host(const float* xyz, const float* normals, uint32_t count, int capacity, const uint32_t range2[2],
                                 const float pose7_in[7], const uint16_t* depth, const float cam5[5], int rows, int cols, float depth_scale,
                                 float dist_m, float damping, float step_eps, int iters, int min_points,
                                 float pose7_out[7], vors_icp_stats* stats, float sums29[29], float* residuals);
/* THE ROBUST PASS: vors_icp_points with two optional remedies against foreign surfaces inside the distance gate. Every
 * argument up to min_points as in vors_icp_points, then:
 * d_frame_normals (nullable = no normal gate): [n][rows * cols][3] f32 in the CAMERA frame — the output of vors_depth_normals on the same
 *   d_depth with d_poses7 = NULL; three zeros = no normal. NORMAL GATE: after the tests above (lands, model normal present, d != 0, the
 *   distance gate) and with n = conj(T.q) * nw, nf = N[y][x] at the landing pixel: MATCHED only if nf is not three zeros and
 *   dot3(n, nf) >= min_cos in float (NaN fails). Both normals face their camera, so any min_cos > 0 culls a back-facing model point.
 * huber_m (0 = off; > 0 = the threshold in metres): the LM kernels' Huber convention (huber_delta) on the point-to-plane residual:
 *   ar = fabsf(r), lin = ar <= huber_m, w = lin ? 1.0f : huber_m / ar, e = lin ? r * r : huber_m * (2.0f * ar - huber_m), wr = w * r; the
 *   28 products are e, J[i] * wr, w * (J[i] * J[j]) in the slots above. Slot 0 of d_sums29, and hence stats.rms =
 *   sqrtf(sums[0] / matched), is then the HUBER LOSS, not the sum of squares — as huber_delta makes the trackers' energy. d_residuals
 *   stays the raw r, unweighted, NaN for unmatched points.
 * d_gate_counts (nullable): [n][VORS_ICP_GATE_COUNTS] u32 of the FINAL evaluation over the clipped range: [0] with_depth — lands, model
 *   normal present, d != 0; [1] within_dist — also inside the distance gate; [2] matched — also passes the normal gate (= stats.matched);
 *   [3] huber_linear — matched with |r| > huber_m (0 when Huber is off). Cleared by a memset when asked for; every workgroup of the final
 *   evaluation adds once per counter with an INTEGER atomic (the order of arrival cannot matter; no floating-point atomic exists).
 * The order of the sums, the loop, the freezing, the statuses, the stats and the workspace (vors_icp_workspace_bytes, unchanged) are
 * vors_icp_points', word for word. d_frame_normals = NULL and huber_m = 0 reproduce vors_icp_points bit for bit in every output; the
 * device equals vors_icp_points_robust_host bit for bit, gate counts included.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued or written: everything vors_icp_points refuses; min_cos NaN or outside
 * [-1, 1]; huber_m negative or NaN; d_frame_normals or d_gate_counts off 4-byte alignment. */
#define VORS_ICP_GATE_COUNTS 4
vors_status vors_icp_points_robust(int n, const float* d_xyz, const float* d_normals, const uint32_t* d_list_counts, int capacity,
                                   const void* d_ranges /* nullable */, size_t range_stride_bytes,
                                   const void* d_poses7_in, size_t pose_stride_bytes, const uint16_t* d_depth,
                                   const float cam5[5], int rows, int cols, float depth_scale,
                                   float dist_m, float damping, float step_eps, int iters, int min_points,
                                   const float* d_frame_normals /* nullable */, float min_cos, float huber_m, void* d_workspace,
                                   float* d_poses7_out, vors_icp_stats* d_stats /* nullable */, float* d_sums29 /* nullable */,
                                   float* d_residuals /* nullable */, uint32_t* d_gate_counts /* nullable */, void* hip_stream);
/* ... and its host twin for ONE list: vors_icp_points_host's arguments, frame_normals [rows * cols][3] (nullable), gate_counts[4]
 * (nullable). The same lie.h texts and the same tree as the kernels. */
vors_status vors_icp_points_robust_host(const float* xyz, const float* normals, uint32_t count, int capacity, const uint32_t range2[2],
                                        const float pose7_in[7], const uint16_t* depth, const float cam5[5], int rows, int cols,
                                        float depth_scale, float dist_m, float damping, float step_eps, int iters, int min_points,
                                        const float* frame_normals /* nullable */, float min_cos, float huber_m,
                                        float pose7_out[7], vors_icp_stats* stats, float sums29[29], float* residuals,
                                        uint32_t gate_counts[VORS_ICP_GATE_COUNTS] /* nullable */);
/* THE JOINT PASS: vors_icp_points_robust with a PHOTOMETRIC row per matched point against the frame's level-0 grey plane.
 * Point-to-plane rows do not constrain motion inside a plane; a grey-level row holds exactly the in-plane translation and the rotation
 * about the normal. vors_icp_points_robust's arguments, and:
 * d_list_gray [n][capacity] u8: the grey level of every list point (vors_trackers_map's d_gray, vors_batch_point_cloud's grey);
 *   d_frame_gray [n][rows * cols] u8: the level-0 grey frame d_depth belongs to. Both nullable when photo_scale_m is 0, else required.
 * photo_scale_m (0 = no photometric row; > 0 = metres per grey level, which puts both residuals into one unit) and photo_huber_grey (0 =
 *   off; > 0 = the Huber threshold in grey levels; photo_huber_m = photo_scale_m * photo_huber_grey is taken once on the host).
 * PER POINT: everything up to and including MATCHED, the geometric row and its 28 products are vors_icp_points_robust's, word for word.
 *   PHOTO iff photo_scale_m > 0, the point is MATCHED and, with c = extr_project(T, w), (u, v) = project_uv(K, c), x0f = floorf(u),
 *   y0f = floorf(v): x0f >= 0 && x0f + 1 <= cols - 1 && y0f >= 0 && y0f + 1 <= rows - 1, in float before any integer conversion (NaN
 *   fails). fx = u - x0f, fy = v - y0f; taps I00 = G[y0][x0], I10 = G[y0][x0 + 1], I01 = G[y0 + 1][x0], I11 = G[y0 + 1][x0 + 1] as
 *   float; top = I00 + fx * (I10 - I00), bot = I01 + fx * (I11 - I01), I = top + fy * (bot - top); gx = (1 - fy) * (I10 - I00) +
 *   fy * (I11 - I01), gy = (1 - fx) * (I01 - I00) + fx * (I11 - I10) — the derivatives of the interpolant itself, no gradient image.
 *   Residual r_p = s * (I - (float)grey) with s = photo_scale_m. Jacobian (the camera moves to T * exp(xi), c(xi) = exp(xi)^-1 c):
 *   iz = 1.0f / c.z, du/dc = (fu * iz, skew * iz, -(((fu * c.x + skew * c.y) * iz) * iz)), dv/dc = (0, fv * iz, -(((fv * c.y) * iz) * iz)),
 *   a = s * (gx * du/dc + gy * dv/dc), J_p = (-a, cross(a, c)), translational three first. Its 28 products p_p are those of the Huber
 *   rule above applied to {r_p, J_p} with the threshold photo_huber_m. A PHOTO point contributes p_g[k] + p_p[k] in f32, geometric
 *   first; any other point p_g[k] alone, with NOTHING added — so that photo_scale_m = 0 is vors_icp_points_robust bit for bit in every
 *   shared output (-0.0f + +0.0f would be +0.0f).
 * Slot 0 of d_sums29 is the JOINT energy (the geometric loss plus the photometric loss, both in square metres), and stats.rms =
 *   sqrtf(sums[0] / matched) is the joint energy's; matched, and slot 1, stay the GEOMETRIC count. d_residuals stays the raw geometric r.
 * d_photo_residuals (nullable): [n][capacity] f32, I - grey in GREY LEVELS, unscaled and unweighted, NaN = not PHOTO; exactly the ranks
 *   of the clipped range written. d_photo_counts (nullable): [n][VORS_ICP_PHOTO_COUNTS] u32 of the FINAL evaluation: [0] photo_used — the
 *   PHOTO points; [1] photo_huber_linear — those with |r_p| > photo_huber_m (0 when that Huber is off). A memset when asked for and one
 *   integer atomic per workgroup and counter, as the gate counts.
 * The order of the sums, the loop, the freezing, the statuses and the workspace (vors_icp_workspace_bytes, unchanged) are
 * vors_icp_points', word for word; the device equals vors_icp_points_joint_host bit for bit, every count included.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued or written: everything vors_icp_points_robust refuses; photo_scale_m or
 * photo_huber_grey negative or NaN; photo_scale_m > 0 with d_list_gray or d_frame_gray NULL; d_photo_residuals or d_photo_counts off
 * 4-byte alignment.
 * Launches: vors_icp_points', with the joint evaluation kernel in the evaluation's place, after a memset per asked-for count array. */
#define VORS_ICP_PHOTO_COUNTS 2
vors_status vors_icp_points_joint(int n, const float* d_xyz, const float* d_normals, const uint8_t* d_list_gray /* nullable */,
                                  const uint32_t* d_list_counts, int capacity,
                                  const void* d_ranges /* nullable */, size_t range_stride_bytes,
                                  const void* d_poses7_in, size_t pose_stride_bytes, const uint16_t* d_depth,
                                  const uint8_t* d_frame_gray /* nullable */, const float cam5[5], int rows, int cols, float depth_scale,
                                  float dist_m, float damping, float step_eps, int iters, int min_points,
                                  const float* d_frame_normals /* nullable */, float min_cos, float huber_m,
                                  float photo_scale_m, float photo_huber_grey, void* d_workspace,
                                  float* d_poses7_out, vors_icp_stats* d_stats /* nullable */, float* d_sums29 /* nullable */,
                                  float* d_residuals /* nullable */, uint32_t* d_gate_counts /* nullable */,
                                  float* d_photo_residuals /* nullable */, uint32_t* d_photo_counts /* nullable */, void* hip_stream);
/* ... and its host twin for ONE list: vors_icp_points_robust_host's arguments, list_gray [capacity], frame_gray [rows * cols],
 * photo_residuals [capacity] (nullable), photo_counts[2] (nullable). The same lie.h texts and the same tree as the kernels. */
vors_status vors_icp_points_joint_host(const float* xyz, const float* normals, const uint8_t* list_gray /* nullable */, uint32_t count,
                                       int capacity, const uint32_t range2[2], const float pose7_in[7], const uint16_t* depth,
                                       const uint8_t* frame_gray /* nullable */, const float cam5[5], int rows, int cols, float depth_scale,
                                       float dist_m, float damping, float step_eps, int iters, int min_points,
                                       const float* frame_normals /* nullable */, float min_cos, float huber_m,
                                       float photo_scale_m, float photo_huber_grey,
                                       float pose7_out[7], vors_icp_stats* stats, float sums29[29], float* residuals,
                                       uint32_t gate_counts[VORS_ICP_GATE_COUNTS] /* nullable */, float* photo_residuals /* nullable */,
                                       uint32_t photo_counts[VORS_ICP_PHOTO_COUNTS] /* nullable */);
/* CONDITIONING OF AN ICP SYSTEM: the "dilution of precision" of the 29 sums of one evaluation (d_sums29 of vors_icp_points*: slot 1 = the
 * matched count n, slots 8..28 = the upper triangle of H). One text (lie.h icp_condition) for the host entry and the device kernel. H is
 * mirrored from the sums and is UNDAMPED; it is factored by the left-looking lower Cholesky in float64, the order of
 * vors_pose_information_from_sums; C = H^-1 = L^-T L^-1 in float64; tt = (C00 + C11) + C22, rr = (C33 + C44) + C55;
 * dilution_t = (float)sqrt((double)n * tt), dilution_r = (float)sqrt((double)n * rr). Geometric and photometric rows are both in metres:
 * dilution_t has no unit, dilution_r is in 1/m. A direction the rows do not hold makes them large — or leaves H without a factor.
 * Neither the list length nor the residuals enter (the residual-scaled covariance of vors_pose_information_from_sums depends on both: a
 * perfect synthetic scene has rms -> 0 and would pass any bound on it while it slides). With Huber weights H is the weighted matrix.
 * flags: bit 0 = !(sums29[1] > 6.0f), bit 1 = a pivot that is not > 0 (no early exit, as there); with either, both dilutions are NaN.
 * vors_icp_condition_from_sums: host arithmetic, no GPU, outputs nullable; sums29 NULL is refused.
 * vors_icp_condition: n systems, d_sums29 [n][29] -> d_dilution2 [n][2] = (dilution_t, dilution_r), d_flags [n] (nullable); one thread
 * per system, enqueued on hip_stream, not synchronised, no allocation; bit for bit the host entry's. Refused with
 * VORS_ERR_INVALID_ARGUMENT, nothing enqueued: n < 1, d_sums29 or d_dilution2 NULL, a pointer off 4-byte alignment. */
vors_status vors_icp_condition_from_sums(const float sums29[29], float* dilution_t /* nullable */, float* dilution_r /* nullable */,
                                         int32_t* flags /* nullable */);
vors_status vors_icp_condition(int n, const float* d_sums29 /* [n][29] */, float* d_dilution2 /* [n][2] */, int32_t* d_flags /* nullable */,
                               void* hip_stream);
/* What vors_trackers_enable_map_icp (section 1b) keeps per sequence of the LAST track call: 112 bytes. A sequence the call did not
 * promote has verdict NOT_ATTEMPTED, frame = its keyframe's index, the window (0, 0), pose_before = pose_after = its keyframe pose and
 * zeros elsewhere. For a promoted one: frame = the new keyframe's index, the window, the pass's statistics and gate counts, pose_before =
 * the keyframe pose the LM stage produced and pose_after = the ICP's output, ACCEPTED OR NOT. */
typedef struct vors_map_icp_record {
    int32_t frame; uint32_t verdict, range_first, range_count;
    vors_icp_stats stats; uint32_t gate_counts[VORS_ICP_GATE_COUNTS];
    float pose_before[7], pose_after[7];
} vors_map_icp_record;
/* The two rules of the correction on the HOST, host arithmetic, no GPU: the texts the kernels run (lie.h map_icp_window, map_icp_verdict).
 * window: segments [min(n_segments, max_keyframes)] (nullable when that is 0 or last_keyframes is 0), count / n_segments the unclipped
 * totals of vors_trackers_map -> range2 = (first, count). Refused: range2 NULL, capacity or max_keyframes < 1, last_keyframes < 0, segments
 * NULL where a record is read. verdict: params' four verdict fields (the others are not read) -> *verdict, a VORS_MAP_ICP_* other than
 * NOT_ATTEMPTED. Refused: a NULL argument, and the verdict fields vors_trackers_enable_map_icp refuses. */
vors_status vors_map_icp_window_host(const vors_map_segment* segments, uint32_t n_segments, int max_keyframes, uint32_t count, int capacity,
                                     int last_keyframes, uint32_t range2[2]);
vors_status vors_map_icp_verdict_host(const vors_map_icp_params* params, const vors_icp_stats* stats, const float pose_before[7],
                                      const float pose_after[7], uint32_t* verdict);
/* What vors_trackers_enable_map_icp_joint (section 1b) keeps BESIDE the vors_map_icp_record of a sequence, same indexing and lifetime:
 * 20 bytes. dilution_t / dilution_r / condition_flags: vors_icp_condition of the pass's final sums29 (NaN, NaN and flags != 0 where H has
 * no factor or too few points matched); photo_counts: vors_icp_points_joint's. Zeros for a sequence the call did not promote. */
typedef struct vors_map_icp_joint_record {
    float dilution_t, dilution_r; int32_t condition_flags; uint32_t photo_counts[VORS_ICP_PHOTO_COUNTS];
} vors_map_icp_joint_record;
/* What vors_trackers_enable_map_icp_means (section 1b) keeps per sequence of the LAST track call: 8 bytes. resolved = the length of the
 * window whose ranks were resolved into the staging, kept = those of them that passed (min_count, min_span). Zeros for a sequence the
 * call did not promote. */
typedef struct vors_map_icp_means_record {
    uint32_t resolved, kept;
} vors_map_icp_means_record;
/* The joint stage's verdict on the HOST (lie.h map_icp_verdict_joint, the text map_icp_apply_joint_kernel runs): vors_map_icp_verdict_host
 * on params->icp, and only behind ACCEPTED the two bounds on the dilutions given -> *verdict, a VORS_MAP_ICP_* other than NOT_ATTEMPTED.
 * Refused: a NULL argument, the verdict fields vors_trackers_enable_map_icp refuses, a dilution bound negative or NaN. */
vors_status vors_map_icp_verdict_joint_host(const vors_map_icp_joint_params* params, const vors_icp_stats* stats, const float pose_before[7],
                                            const float pose_after[7], float dilution_t, float dilution_r, uint32_t* verdict);

/* ------------------------------------------------------------------------------------------------------------
 * 2f. SENSOR FRONT END, device-resident and handle-free (the reference has none and ignores lens distortion): what turns
 *     a real RGB-D stream into the three things every other entry assumes — an ideal pinhole grey image, a u16 depth map registered to
 *     it pixel for pixel, and one cu cv fu fv skew for both.
 *
 * vors_undistort_frames: n planes of grey u8 and / or depth u16, [n][in_rows * in_cols] row-major (DEVICE, each nullable, one required),
 *   of the real camera cam_in5 (HOST) with Brown-Conrady coefficients dist5 = k1 k2 p1 p2 k3 (HOST; NULL = all zero), resampled into the
 *   ideal camera cam_out5 (HOST) of out_rows x out_cols pixels (crops and re-centred cameras are the normal case).
 * SOURCE COORDINATE of output pixel (x, y), in f32, in the written order, without FMA:
 *     (X, Y, 1) = back_project(K_out, (float)x, (float)y, 1.0f)        (Y = (y - cv) / fv, X = ((x - cu) - skew * Y) / fu)
 *     xx = X*X;  yy = Y*Y;  xy = X*Y;  r2 = xx + yy
 *     rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3))
 *     Xd = (X * rad + (2.0f * p1) * xy) + p2 * (r2 + 2.0f * xx)
 *     Yd = (Y * rad + p1 * (r2 + 2.0f * yy)) + (2.0f * p2) * xy
 *     u = (fu_in * Xd + skew_in * Yd) + cu_in;   v = fv_in * Yd + cv_in
 * GREY: bilinear in lerp form. x0 = floorf(u), a = u - x0, x1 = min(x0 + 1, in_cols - 1), rows likewise with b; t0 = I00 + a * (I01 - I00),
 *   t1 = I10 + a * (I11 - I10), val = t0 + b * (t1 - t0), all in f32; the output is floorf(val + 0.5f) clamped to 0..255. A pixel is inside
 *   iff 0 <= u <= in_cols - 1 and 0 <= v <= in_rows - 1, compared in float before any conversion (NaN fails). border = 0 writes 0
 *   outside; border = 1 clamps u and v into the plane first (edge replicate); a NaN coordinate still writes 0.
 * DEPTH: never interpolated. xs = floorf(u + 0.5f), ys = floorf(v + 0.5f) (the landing rule of vors_batch_reproject_depth); the output is
 *   D[ys][xs] if that pixel lies inside the plane (tested in float), else 0. border does not apply: depth is never invented.
 * Outputs (DEVICE, each nullable, at least one required; every output pixel is written): d_gray_out / d_depth_out [n][out_rows * out_cols];
 *   d_map [out_rows * out_cols][2] f32 = (u, v), written once, not per plane; d_counts [n][VORS_UNDISTORT_COUNTS] u32 = {pixels: out_rows *
 *   out_cols; grey inside: the pixels whose (u, v) lies inside the plane, whatever the border mode and whether or not there is a grey
 *   plane; depth inside and non-zero: the pixels of d_depth_out that are not 0 (0 without a depth plane)}.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued and nothing written: n < 1; both input planes NULL; d_gray_out without d_gray or
 *   d_depth_out without d_depth; no output at all; a NULL cam_in5 or cam_out5; a non-finite coefficient or camera value, fu or fv equal
 *   to 0; border outside 0..1; any of the four sizes < 1 or > 65535, or a plane above 2^28 pixels; a pointer off its natural alignment
 *   (depth planes: 2 bytes, d_map and d_counts: 4). Enqueued on hip_stream on the calling thread's current device, NOT synchronised, no
 *   allocation ever: a memset of the counters when they are asked for and one kernel; no workgroup waits for another. The one text
 *   (lie.h undistort_source, undistort_taps, undistort_gray) runs on the host and on the device: the device results equal
 *   vors_undistort_frame_host's bit for bit. */
#define VORS_UNDISTORT_COUNTS 3
vors_status vors_undistort_frames(int n, const uint8_t* d_gray /* nullable */, const uint16_t* d_depth /* nullable */, int in_rows, int in_cols,
                                  const float cam_in5[5], const float dist5[5] /* nullable */, const float cam_out5[5], int out_rows,
                                  int out_cols, int border, uint8_t* d_gray_out /* nullable */, uint16_t* d_depth_out /* nullable */,
                                  float* d_map /* nullable */, uint32_t* d_counts /* nullable */, void* hip_stream);
/* The same rule for ONE plane of each kind on the host (host arithmetic, needs no GPU; the text the kernel runs): HOST pointers, counts
 * [VORS_UNDISTORT_COUNTS]. The refusals above, with nothing written. */
vors_status vors_undistort_frame_host(const uint8_t* gray /* nullable */, const uint16_t* depth /* nullable */, int in_rows, int in_cols,
                                      const float cam_in5[5], const float dist5[5] /* nullable */, const float cam_out5[5], int out_rows,
                                      int out_cols, int border, uint8_t* gray_out /* nullable */, uint16_t* depth_out /* nullable */,
                                      float* map /* nullable */, uint32_t counts[VORS_UNDISTORT_COUNTS] /* nullable */);
/* The source coordinates alone, for a list of output pixels on the host: xy [n_pixels][2] int32 (x, y), anywhere — the ideal camera has no
 * border — -> uv [n_pixels][2] f32. Refused: n_pixels < 0, a NULL xy or uv with n_pixels > 0, and what the above refuse of the cameras
 * and the coefficients. */
vors_status vors_undistort_source_host(const float cam_in5[5], const float dist5[5] /* nullable */, const float cam_out5[5], int n_pixels,
                                       const int32_t* xy, float* uv);
/* vors_register_depth: n depth planes d_depth [n][d_rows * d_cols] u16 (DEVICE) of a PINHOLE depth camera dcam5 (HOST) with depth_scale_in
 *   (a distorted depth camera goes through vors_undistort_frames first), seen from the colour camera ccam5 (HOST) of c_rows x c_cols pixels
 *   with depth_scale_out. pose7 (HOST, nullable): depth camera -> colour camera, tx ty tz qi qj qk qw; NULL = no transform at all.
 * PER SOURCE PIXEL s = y * d_cols + x with d != 0: z = 1.0f / (depth_scale_in / (float)d), P = back_project(K_d, (float)x, (float)y, z) —
 *   the camera-frame bits of vors_batch_point_cloud —, c = rotation * P + translation (the point cloud's camera -> world text), then
 *   exactly vors_render_points' rule for the point c in the camera ccam5 WITHOUT a pose: Z' = c.z, the candidate test, the footprint
 *   (1..3) and the key (uint64)bits(Z') << 32 | s, entered into d_zkey [n][c_rows * c_cols] (DEVICE, REQUIRED, 8-byte aligned) by an
 *   unsigned 64-bit minimum; VORS_ZKEY_EMPTY where nothing lands. The nearest surface wins, among equal Z' bits the lowest source index:
 *   bitwise reproducible whatever the order of arrival.
 * Outputs (DEVICE, each nullable): d_depth_out [n][c_rows * c_cols] u16 = to_depth(depth_scale_out, 1.0f / Z') of the key, 0 where empty;
 *   d_src_index [n][c_rows * c_cols] u32 = the winning s, 0xFFFFFFFF where empty (with it a caller carries IR, confidence or the depth
 *   filter's weight plane across); d_counts [n][VORS_REGISTER_COUNTS] u32 = {with depth: the source pixels with d != 0; in front: those
 *   with Z' > 0; landed; covered: the colour pixels whose key is not empty}.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued and nothing written: n < 1; a NULL d_depth, dcam5 or ccam5; a NULL or misaligned
 *   d_zkey; footprint outside 1..3; any of the four sizes < 1 or > 65535, or a plane above 2^28 pixels; a depth scale not > 0; a pointer
 *   off its natural alignment (depth planes: 2 bytes, d_src_index and d_counts: 4). Enqueued on hip_stream on the calling thread's current
 *   device, NOT synchronised, no allocation ever: the fill of the key planes, a memset of the counters when they are asked for, the splat
 *   kernel and — with any of d_depth_out, d_src_index, d_counts — the resolve kernel, ordered by the stream. */
#define VORS_REGISTER_COUNTS 4
vors_status vors_register_depth(int n, const uint16_t* d_depth, const float dcam5[5], int d_rows, int d_cols, float depth_scale_in,
                                const float pose7[7] /* nullable */, const float ccam5[5], int c_rows, int c_cols, float depth_scale_out,
                                int footprint, uint64_t* d_zkey, uint16_t* d_depth_out /* nullable */, uint32_t* d_src_index /* nullable */,
                                uint32_t* d_counts /* nullable */, void* hip_stream);
/* The same rule for ONE plane on the host (host arithmetic, needs no GPU; the text the kernels run): HOST pointers, zkey [c_rows * c_cols]
 * required here too (it is the z-buffer). The refusals above, with nothing written. */
vors_status vors_register_depth_host(const uint16_t* depth, const float dcam5[5], int d_rows, int d_cols, float depth_scale_in,
                                     const float pose7[7] /* nullable */, const float ccam5[5], int c_rows, int c_cols, float depth_scale_out,
                                     int footprint, uint64_t* zkey, uint16_t* depth_out /* nullable */, uint32_t* src_index /* nullable */,
                                     uint32_t counts[VORS_REGISTER_COUNTS] /* nullable */);

/* ------------------------------------------------------------------------------------------------------------
 * 2g. POSE-GRAPH OPTIMISATION OF KEYFRAME POSES, device-resident and handle-free (the reference has none): given N poses and
 *     E relative-pose measurements with information matrices, the poses that best satisfy all of them — the consumer of
 *     vors_batch_track_pairs' lm_model and of vors_batch_pose_information's info36, which go in unchanged.
 * Graphs: n graphs are solved side by side. DEVICE pointers: d_poses7_in [n][node_capacity] camera -> world poses, pose_stride_bytes apart
 *   (0 = packed, 28; as in vors_render_points); d_node_counts [n] u32 and d_edge_counts [n] u32 (a count above its capacity is clipped);
 *   d_edges [n][edge_capacity] {u32 i, j}; d_meas7 [n][edge_capacity][7]; d_info36 [n][edge_capacity][36] row-major (nullable =
 *   identity); d_edge_weight [n][edge_capacity] f32, multiplies the information (nullable = 1); d_fixed [n][node_capacity] u8, non-zero =
 *   fixed (nullable = node 0 of every graph is fixed).
 * MEASUREMENT: M_ij maps coordinates of camera i into camera j — vors_pair_stats.lm_model of keyframe i and frame j; consistent poses
 *   have T_j = T_i M_ij^-1. Edge error E = T_i^-1 T_j M_ij. Under the LM's parametrisation (true model = model exp(xi)^-1) E = exp(xi)
 *   exactly, so the residual below is xi to first order and info36 = sum J^T J of the LM is its information WITHOUT an adjoint transport.
 * RESIDUAL: r = (E.t, 2 s E.q.ijk), s = +1 if E.q.w >= 0 else -1; no transcendental. Energy of an edge: w (r . (Omega r)), Omega r row by
 *   row left to right, then the six products in ascending order (lie.h pg_edge_energy). With d_info36 = NULL the same arithmetic runs on
 *   an identity matrix: NULL equals identity matrices bit for bit.
 * JACOBIANS (exact, closed form; perturbation T_k <- renormalize(T_k se3_exp(d_k))): A(E) = blockdiag(R_E, s (E.q.w I + [E.q.ijk]x)),
 *   Ad(R, t) = [[R, [t]x R], [0, R]] in se3_exp's (v, w) order: J_j = A(E) Ad(M_ij^-1), J_i = -A(E) Ad(E^-1) (lie.h pg_edge_jacobians).
 * SKIPPED EDGES, counted, contributing nothing anywhere: i == j; an index >= node_count; a weight that is not finite or not > 0; a
 *   measurement or information entry that is not finite. A free node without a valid edge is treated as fixed and counted as isolated.
 * ORDER OF THE SUMS (part of the definition): the graph energy — edges in chunks of 1024 consecutive indices (a skipped edge and a slot
 *   beyond the count hold +0.0f), inside a chunk vors_icp_points' halving tree in f32, the chunk sums added in ascending order from chunk
 *   0's. Per node k, g_k and the lower triangle of H_kk: sequential f32 sums over k's incident valid edges in ascending edge index,
 *   starting from the first edge's term. Per edge W_e = J_i^T (w Omega) J_j, stored once per linearisation. Dot products of the solve:
 *   nodes in chunks of 1024, the same tree and chunk order IN f64 (a node that is not free holds 0.0).
 * OUTER LOOP per graph, Levenberg-Marquardt, no host round trip: `iters` rounds of linearise; solve (H + lambda D) delta = -g over the
 *   free nodes, D = diag(H) (cholesky6_solve's damping: diagonal times 1 + lambda); candidates T_k' = renormalize(T_k se3_exp(delta_k));
 *   energy at the candidates; ACCEPT iff energy' <= energy (a NaN is rejected): the candidates become the poses and lambda = 0.1f lambda;
 *   otherwise the poses stay and lambda = 10 lambda (lm_verdict's constants; lie.h pg_accepts / pg_lambda_after). A rejected round keeps
 *   its linearisation. Then ONE final evaluation at the returned poses, which is what the per-edge outputs and final_energy describe
 *   (iters = 0: a pure evaluator).
 * INNER SOLVE: block-Jacobi preconditioned conjugate gradients from delta = 0; the 6x6 blocks H_kk + lambda D_kk are factored by a
 *   Cholesky per node. Exactly cg_iters iterations unless, before an iteration, r.r <= cg_tol^2 r0.r0 (a NaN ends them too). The product
 *   is a gather per node: the own block first, then W_e p_j (the node is the edge's i) or W_e^T p_i over its incidence list in ascending
 *   edge index. THE SCALARS ARE f64 (dot products, alpha, beta; lie.h pg_dot6, pg_cg_alpha, pg_cg_beta); alpha and beta are rounded to
 *   f32 once and the vectors are f32.
 * FREEZING: VORS_PG_CONVERGED when an accepted step has max_k dot6(delta_k, delta_k) <= step_eps^2; VORS_PG_SINGULAR when a block has no
 *   Cholesky factor (poses kept); VORS_PG_TOO_FEW when there is no valid edge or no free node (poses returned as given);
 *   VORS_PG_ITERATIONS otherwise.
 * Outputs (DEVICE): d_poses7_out [n][node_capacity][7] packed, exactly the nodes below node_count written (may alias d_poses7_in when
 *   that is packed; fixed and isolated nodes, and every node of a graph that accepted no step, keep their bits); d_stats [n] (nullable);
 *   d_edge_residuals [n][edge_capacity][6] and d_edge_energy [n][edge_capacity] (nullable) of the final evaluation, exactly the edges
 *   below edge_count written, NaN for a skipped edge.
 * d_workspace (DEVICE, 16-byte aligned): vors_pose_graph_workspace_bytes(n, node_capacity, edge_capacity) bytes; 0 for an argument < 1.
 * The result of a graph depends neither on the graphs around it, nor on the capacities, the grid or the schedule; the device equals
 *   vors_pose_graph_optimize_host bit for bit. No floating-point atomic exists; the incidence lists are built with integer atomics and
 *   then ordered per node.
 * Refused with VORS_ERR_INVALID_ARGUMENT, nothing enqueued: n < 1; a NULL d_poses7_in, d_node_counts, d_edges, d_edge_counts, d_meas7,
 *   d_workspace or d_poses7_out; a capacity < 1 or > 2^28; a bad pose stride; lambda0, step_eps or cg_tol negative or NaN; iters outside
 *   0..64; cg_iters outside 1..256; a pointer off its alignment (d_workspace: 16 bytes, d_fixed: none, the others: 4).
 * Enqueued on hip_stream on the calling thread's current device, NOT synchronised, no allocation ever. Launches: the incidence build (five)
 *   and the initial energy (two) once; per round the linearisation, the gather, two per CG iteration (product with partial dots; reduce
 *   and update), the candidates, their energy, the verdict; then the final evaluation and the launch that writes the outputs. Every
 *   launch is enqueued unconditionally, graphs freeze by state, no workgroup waits for another. */
#define VORS_PG_ITERATIONS 0
#define VORS_PG_CONVERGED 1
#define VORS_PG_TOO_FEW 2
#define VORS_PG_SINGULAR 3
typedef struct vors_pose_graph_stats {
    uint32_t status, accepted_steps, rejected_steps, cg_iterations;
    uint32_t valid_edges, skipped_edges, free_nodes, fixed_nodes, isolated_nodes;
    float initial_energy, final_energy, last_step_norm, final_lambda;
} vors_pose_graph_stats;
uint64_t vors_pose_graph_workspace_bytes(int n, int node_capacity, int edge_capacity);
vors_status vors_pose_graph_optimize(int n, const void* d_poses7_in, size_t pose_stride_bytes, const uint32_t* d_node_counts, int node_capacity,
                                     const uint32_t* d_edges, const uint32_t* d_edge_counts, int edge_capacity, const float* d_meas7,
                                     const float* d_info36 /* nullable */, const float* d_edge_weight /* nullable */,
                                     const uint8_t* d_fixed /* nullable */, float lambda0, float step_eps, float cg_tol, int iters, int cg_iters,
                                     void* d_workspace, float* d_poses7_out, vors_pose_graph_stats* d_stats /* nullable */,
                                     float* d_edge_residuals /* nullable */, float* d_edge_energy /* nullable */, void* hip_stream);
/* The same loop for ONE graph on the host (host arithmetic, needs no GPU; the texts and the order of sums the kernels run): HOST pointers,
 * poses packed [node_capacity][7], no workspace. The refusals above, with nothing written. */
vors_status vors_pose_graph_optimize_host(const float* poses7_in, uint32_t node_count, int node_capacity, const uint32_t* edges,
                                          uint32_t edge_count, int edge_capacity, const float* meas7, const float* info36 /* nullable */,
                                          const float* edge_weight /* nullable */, const uint8_t* fixed /* nullable */, float lambda0,
                                          float step_eps, float cg_tol, int iters, int cg_iters, float* poses7_out,
                                          vors_pose_graph_stats* stats /* nullable */, float* edge_residuals /* nullable */,
                                          float* edge_energy /* nullable */);
/* The residual and the two Jacobians of ONE edge at the poses (ti, tj), the kernels' own text (lie.h pg_edge_jacobians), for tests:
 * r6, ji36 and jj36 row-major (HOST). */
void vors_pose_graph_jacobians_host(const float ti7[7], const float tj7[7], const float meas7[7], float r6[6], float ji36[36], float jj36[36]);

/* ------------------------------------------------------------------------------------------------------------
 * 2h. LOOP CLOSURE, device-resident and handle-free (the reference has none): which earlier keyframes a keyframe should be
 *     matched against, and which of the tracked loop pairs may become edges of 2g's graph. Three entries, each with a host twin that the
 *     device equals bit for bit; the shared texts are csrc/lie.h lc_*. Every entry is enqueued on hip_stream on the calling thread's
 *     current device, NOT synchronised, allocates nothing; no workgroup waits for another; no floating-point atomic exists. Every refusal
 *     is VORS_ERR_INVALID_ARGUMENT with nothing enqueued and nothing written.
 *
 * (1) vors_loop_signatures: a thumbnail signature per grey plane. d_gray [n][rows * cols] u8 (DEVICE); the thumbnail is tr x tc cells,
 *   D = tr * tc. Cell (cy, cx) covers rows [cy rows / tr, (cy + 1) rows / tr) and columns [cx cols / tc, (cx + 1) cols / tc) (integer
 *   division); S = the sum of its pixels, cnt their number, q = (2 S + cnt) / (2 cnt) the rounded mean, s = q - 128 the stored int8. All
 *   of it is exact integer arithmetic: no order of sums to define. Outputs (DEVICE): d_sig [n][D] i8, cell-major cy * tc + cx, 16-byte
 *   aligned; d_sig_meta [n] {sum of s, sum of s * s}. Both may point INTO larger [capacity][D] / [capacity] arrays (plain pointer
 *   arithmetic; D is a multiple of 64, so every row keeps the alignment): keyframes are appended as they are promoted, and nothing
 *   outside the n rows is written. One launch, a workgroup per plane; the plane is read once, as whole 16-byte words at 16-byte
 *   aligned addresses: where d_gray or a plane's end is off that alignment, up to 15 bytes BEFORE d_gray and up to 15 bytes PAST the
 *   last plane are loaded and ignored — they lie in the same aligned 16-byte block as a byte of the planes, so in the same page.
 *   Refused: n < 1; a NULL pointer; D not a multiple of 64 or outside 64..1024; tr or tc < 1; rows < tr, cols < tc; rows or cols > 65535
 *   or rows * cols > 2^28; d_sig off 16 bytes, d_sig_meta off 4.
 * (2) vors_loop_candidates: all pairs of signatures of a set scored, gated, the best k per query. n sets side by side: d_sig
 *   [n][capacity][D], d_sig_meta [n][capacity], d_counts_in [n] u32 (a count above capacity is clipped); d_poses7 (nullable) the
 *   keyframes' camera -> world poses [n][capacity], pose_stride_bytes apart (0 = packed, 28); d_query_first [n] u32 (nullable = 0): only
 *   queries j in [first, count) are answered — the keyframes promoted since the last call.
 *   DEFINITION. The candidates of query j are every i with i + min_gap <= j. dot = sum_c s_i[c] s_j[c] (exact, i32); num = D dot -
 *   sum_i sum_j (i64); va = D sumsq - sum^2 (i64) per signature; root = sqrt((double)va); score = (float)((double)num / (root_i *
 *   root_j)): f64 multiply and divide, no contraction, rounded once to f32. Three gates in this order, a pair counted under the first that
 *   removes it: FLAT va_i == 0 or va_j == 0; POSE (only with d_poses7; f32): dot3(d, d) <= max_dist_m^2 must hold for d = t_i - t_j,
 *   and |dot3(q_i.ijk, q_j.ijk) + q_i.w q_j.w| >= min_qdot must hold and be finite — max_dist_m = 0 and min_qdot = 0 switch their half
 *   off, a NaN fails a half that is on; SCORE not score >= min_score (a NaN fails). Survivors are ordered by (score descending, i
 *   ascending), a total order: the result depends on no tile, grid or schedule.
 *   d_sig_meta MUST BE the record of its signature, as vors_loop_signatures writes it. Then |num| <= root_i root_j and |score| <= 1, and
 *   the kernel relies on it: before the f64 divide it drops a pair whose f32 estimate of the score (error below 1e-6 for |score| <= 1)
 *   lies more than 1e-4 under min_score, which the exact score would drop as well. With meta records that belong to other signatures
 *   the device may count a pair as score-gated that the host twin keeps.
 *   Outputs (DEVICE): d_cand [n][capacity][k] vors_loop_candidate, the first min(k, survivors) of that order, unused slots {0xFFFFFFFF,
 *   0.0f}; d_cand_counts [n][capacity] u32 = min(k, survivors); exactly the queries in [first, count) are written. d_counts
 *   [n][VORS_LOOP_COUNTS] u32 (nullable) = {examined, flat, pose-gated, score-gated, survivors} over the answered queries (modulo 2^32),
 *   integer atomics after a memset that the entry enqueues. One launch (two with d_counts): the dot products are
 *   v_mfma_i32_32x32x32_i8 tiles of the signature matrix against itself, tiles wholly above the band are skipped.
 *   Refused: n < 1; a NULL d_sig, d_sig_meta, d_counts_in, d_cand or d_cand_counts; capacity < 1 or > 2^20; D not a multiple of 64 or
 *   outside 64..1024; min_gap < 1; k outside 1..VORS_LOOP_MAX_K; max_dist_m or min_qdot negative or NaN; a bad pose stride; d_sig off 16
 *   bytes, another pointer off 4.
 * (3) vors_loop_verify_edges: from tracked candidate pairs to pose-graph edges. The caller has tracked every candidate both ways with
 *   the existing entries: keyframe i against frame j gives M_ij, j against i gives M_ji, vors_batch_pose_information gives info36 of the
 *   forward pair. DEVICE: d_pairs [m] {u32 i, j}; d_model_fwd / d_model_bwd [m] models, fwd / bwd_stride_bytes apart (0 = packed, 28;
 *   vors_pair_stats.lm_model goes in with sizeof(vors_pair_stats)); d_model_bwd nullable; d_status_fwd / d_status_bwd [m] int32
 *   (d_status_bwd nullable); d_info36 [m][36] nullable; d_poses7 (nullable) the current estimates of node_count nodes, pose_stride_bytes
 *   apart.
 *   VERDICT per candidate, the first rule that applies: VORS_LOOP_STATUS a given status is not VORS_TRACK_OK; VORS_LOOP_INDEX i == j, or —
 *   with poses — an index >= node_count; VORS_LOOP_NONFINITE an entry of a given model or of the information is not finite;
 *   VORS_LOOP_CYCLE_TRANS / _ROT (with a backward model) C = M_ji M_ij, r = 2g's residual of C, dot3(r.t) > max_cycle_trans^2 /
 *   dot3(r.rot) > max_cycle_rot^2; VORS_LOOP_PRIOR_TRANS / _ROT (with poses) the same on 2g's edge error E = T_i^-1 T_j M_ij;
 *   VORS_LOOP_CAPACITY accepted, but the edge list is full; VORS_LOOP_ACCEPTED. A bound of 0 switches its test off; a NaN residual fails
 *   a test that is on.
 *   Outputs (DEVICE), in 2g's formats: the accepted candidates IN CANDIDATE ORDER appended to d_edges, d_meas7 (= M_ij), d_info36_out
 *   (nullable; identity rows when d_info36 is NULL) and d_edge_weight (nullable; = weight), starting at the in / out d_edge_count[0]
 *   (where the caller's odometry edges end; a count above edge_capacity is clipped to it) — an ordered compaction, the list is a function
 *   of the inputs alone; d_verdict [m] u32; d_residuals [m][12] (nullable) the cycle's r6, then the prior's r6, both computed for every
 *   candidate that passes STATUS, INDEX and NONFINITE, NaN otherwise and where their input is not given; d_counts [VORS_LOOP_VERDICTS]
 *   u32 (nullable), one per verdict code. One launch of one workgroup.
 *   Refused: m < 1 or > 2^28; a NULL d_pairs, d_model_fwd, d_status_fwd, d_edges, d_meas7, d_edge_count or d_verdict; edge_capacity < 1 or
 *   > 2^28; a bad stride; a bound negative or NaN; weight not finite or not > 0; a pointer off 4 bytes. */
#define VORS_LOOP_MAX_K 8
#define VORS_LOOP_COUNTS 5
#define VORS_LOOP_ACCEPTED 0
#define VORS_LOOP_STATUS 1
#define VORS_LOOP_INDEX 2
#define VORS_LOOP_NONFINITE 3
#define VORS_LOOP_CYCLE_TRANS 4
#define VORS_LOOP_CYCLE_ROT 5
#define VORS_LOOP_PRIOR_TRANS 6
#define VORS_LOOP_PRIOR_ROT 7
#define VORS_LOOP_CAPACITY 8
#define VORS_LOOP_VERDICTS 9
typedef struct vors_loop_sig_meta {
    int32_t sum;
    uint32_t sumsq;
} vors_loop_sig_meta;
typedef struct vors_loop_candidate {
    uint32_t i;
    float score;
} vors_loop_candidate;
vors_status vors_loop_signatures(int n, const uint8_t* d_gray, int rows, int cols, int tr, int tc, int8_t* d_sig, vors_loop_sig_meta* d_sig_meta,
                                 void* hip_stream);
/* ONE plane on the host (HOST pointers; needs no GPU). The refusals above. */
vors_status vors_loop_signatures_host(const uint8_t* gray, int rows, int cols, int tr, int tc, int8_t* sig, vors_loop_sig_meta* sig_meta);
vors_status vors_loop_candidates(int n, const int8_t* d_sig, const vors_loop_sig_meta* d_sig_meta, const uint32_t* d_counts_in, int capacity, int D,
                                 const void* d_poses7 /* nullable */, size_t pose_stride_bytes, const uint32_t* d_query_first /* nullable */,
                                 uint32_t min_gap, int k, float min_score, float max_dist_m, float min_qdot, vors_loop_candidate* d_cand,
                                 uint32_t* d_cand_counts, uint32_t* d_counts /* nullable */, void* hip_stream);
/* ONE set on the host: HOST pointers, poses packed [capacity][7]. The refusals above. */
vors_status vors_loop_candidates_host(const int8_t* sig, const vors_loop_sig_meta* sig_meta, uint32_t count, int capacity, int D,
                                      const float* poses7 /* nullable */, uint32_t query_first, uint32_t min_gap, int k, float min_score,
                                      float max_dist_m, float min_qdot, vors_loop_candidate* cand, uint32_t* cand_counts,
                                      uint32_t counts[VORS_LOOP_COUNTS] /* nullable */);
vors_status vors_loop_verify_edges(uint32_t m, const uint32_t* d_pairs, const void* d_model_fwd, size_t fwd_stride_bytes,
                                   const void* d_model_bwd /* nullable */, size_t bwd_stride_bytes, const int32_t* d_status_fwd,
                                   const int32_t* d_status_bwd /* nullable */, const float* d_info36 /* nullable */,
                                   const void* d_poses7 /* nullable */, size_t pose_stride_bytes, uint32_t node_count, float max_cycle_trans,
                                   float max_cycle_rot, float max_prior_trans, float max_prior_rot, float weight, uint32_t* d_edges,
                                   float* d_meas7, float* d_info36_out /* nullable */, float* d_edge_weight /* nullable */,
                                   uint32_t* d_edge_count, int edge_capacity, uint32_t* d_verdict, float* d_residuals /* nullable */,
                                   uint32_t* d_counts /* nullable */, void* hip_stream);
/* The same on the host: HOST pointers, the same strides. The refusals above. */
vors_status vors_loop_verify_edges_host(uint32_t m, const uint32_t* pairs, const void* model_fwd, size_t fwd_stride_bytes,
                                        const void* model_bwd /* nullable */, size_t bwd_stride_bytes, const int32_t* status_fwd,
                                        const int32_t* status_bwd /* nullable */, const float* info36 /* nullable */,
                                        const void* poses7 /* nullable */, size_t pose_stride_bytes, uint32_t node_count, float max_cycle_trans,
                                        float max_cycle_rot, float max_prior_trans, float max_prior_rot, float weight, uint32_t* edges,
                                        float* meas7, float* info36_out /* nullable */, float* edge_weight /* nullable */, uint32_t* edge_count,
                                        int edge_capacity, uint32_t* verdict, float* residuals /* nullable */, uint32_t* counts /* nullable */);

/* ------------------------------------------------------------------------------------------------------------
 * 2i. THE CORRECTED MAP, device-resident and handle-free (the reference has none): what a caller who closed a loop does with
 *     the poses vors_pose_graph_optimize returned. RE-POSE moves every point and normal of a list from the pose its keyframe had to the
 *     pose the optimiser gave it; RE-FILTER restores "one point per occupied voxel, the first in the list's order" on any point list.
 *     Both are stream-ordered, allocate nothing, use integer atomics only, and equal their host twins bit for bit.
 * RE-POSE. n lists side by side, the pointers of vors_trackers_map / vors_trackers_map_normals and of vors_pose_graph_optimize:
 *   d_xyz [n][capacity][3] f32, d_normals likewise (nullable), d_list_counts [n] u32 (unclipped: the ranks treated are those below
 *   min(count, capacity)); d_segments [n][max_keyframes] with d_n_segments [n] (the first min(n_segments, max_keyframes) records are
 *   used; their `first` must ascend, as a map's do — otherwise which record a rank takes is unspecified, and every store still stays
 *   inside its buffers); d_poses7_new, node_capacity poses per list, pose_stride_bytes apart (0 = 28; a multiple of 4 of at least 28),
 *   d_node_counts [n] (clipped to node_capacity); d_node_of_segment [n][max_keyframes] u32 (nullable = segment k is node k; the value
 *   0xFFFFFFFF = this keyframe is not in the graph).
 *   A rank belongs to the LAST record whose `first` is not above it, if it lies below that record's first + count; a zero-count segment
 *   owns no rank; the ranks at or beyond the end of the last record have NO RECORD (keyframes beyond max_keyframes).
 *   A recorded segment k with old pose A = segments[k].pose7 and new pose B MOVES iff it has a node (an index below the node count, not
 *   the sentinel), all seven floats of B are finite and B's bits differ from A's. Otherwise it is KEPT: points, normals and record are
 *   copied bit for bit — re-posing with the poses the map already has is the identity on bits, and a fixed node never drifts.
 *   Moved point: c = extrinsics::project(A, p), p' = B * c (the texts of vors_camera_project and vors_camera_back_project, unchanged):
 *   through the keyframe's camera frame, so p' is what the map would have stored with the keyframe at B, up to rounding. Moved normal:
 *   n' = B.q * (A.q^-1 * n). A point with a non-finite component (a NaN row of vors_voxel_means) is copied bit for bit wherever it lies,
 *   likewise a normal, each on its own; a rank without a record is copied. A NaN the arithmetic itself produces is stored as 0x7FC00000.
 *   Outputs, each nullable, one of the first two required: d_xyz_out, d_normals_out (refused without d_normals) — exactly the ranks below
 *   min(count, capacity) are written; d_segments_out — exactly the used records, pose7 replaced where the segment moved, frame / first /
 *   count kept; d_counts_out [n][VORS_REPOSE_COUNTS] u32 = {points moved; kept; non-finite (wherever they lie); without a record;
 *   segments moved; the largest |p' - p| over the moved points as the bits of a non-negative f32 under an unsigned maximum}. The first
 *   four add up to min(count, capacity).
 *   d_xyz_out == d_xyz, d_normals_out == d_normals and d_segments_out == d_segments are legal (a rank is read and written by one lane;
 *   the records are written by a launch behind the point pass, which reads the old ones). Refused with VORS_ERR_INVALID_ARGUMENT, nothing
 *   enqueued: a NULL required pointer; n outside 1..65535; capacity, max_keyframes or node_capacity < 1; a bad stride; an array off
 *   4-byte alignment; any other overlap of an output with an input or with another output; d_normals_out without d_normals; a stream of
 *   another device than the current one. A 16-byte aligned list is moved with 16-byte accesses, any other point by point: same bits. */
#define VORS_REPOSE_COUNTS 6
vors_status vors_repose_points(int n, const float* d_xyz, const float* d_normals /* nullable */, const uint32_t* d_list_counts, int capacity,
                               const vors_map_segment* d_segments, const uint32_t* d_n_segments, int max_keyframes, const void* d_poses7_new,
                               size_t pose_stride_bytes, int node_capacity, const uint32_t* d_node_counts,
                               const uint32_t* d_node_of_segment /* nullable */, float* d_xyz_out /* nullable */,
                               float* d_normals_out /* nullable */, vors_map_segment* d_segments_out /* nullable */,
                               uint32_t* d_counts_out /* nullable */, void* hip_stream);
/* The same for ONE list in HOST memory (no GPU): the text the kernels run, bit for bit; poses7_new packed [node_capacity][7]. Same
 * refusals. */
vors_status vors_repose_points_host(const float* xyz, const float* normals /* nullable */, uint32_t count, int capacity,
                                    const vors_map_segment* segments, uint32_t n_segments, int max_keyframes, const float* poses7_new,
                                    uint32_t node_count, int node_capacity, const uint32_t* node_of_segment /* nullable */,
                                    float* xyz_out /* nullable */, float* normals_out /* nullable */, vors_map_segment* segments_out /* nullable */,
                                    uint32_t counts_out[VORS_REPOSE_COUNTS] /* nullable */);
/* vors_repose_points on a sequence handle's own map: its lists, its normals (when vors_trackers_enable_map_normals is on), its counters
 * and its segments are the inputs, the CALLER's arrays the outputs. The handle is read only: its map, voxel table, statistics and poses
 * stay as tracking left them (feeding corrected poses back into a running tracker is not done here). Refused like
 * vors_trackers_render_map — no enabled map, a call before vors_trackers_init, a stream of another device — and with every refusal of
 * vors_repose_points; an output that IS one of the handle's arrays is refused too. Enqueued on hip_stream, NOT synchronised. */
vors_status vors_trackers_repose_map(vors_trackers* t, const void* d_poses7_new, size_t pose_stride_bytes, int node_capacity,
                                     const uint32_t* d_node_counts, const uint32_t* d_node_of_segment /* nullable */,
                                     float* d_xyz_out /* nullable */, float* d_normals_out /* nullable */,
                                     vors_map_segment* d_segments_out /* nullable */, uint32_t* d_counts_out /* nullable */, void* hip_stream);
/* RE-FILTER. Per list of d_xyz [n][capacity][3] / d_list_counts [n]: the ranks r below min(count, capacity) whose voxel key
 *   (vors_voxel_keys with voxel_m, section 4) is not VORS_VOXEL_NONE and occurs at no lower rank, in ascending order — the definition of
 *   vors_trackers_enable_map_voxels, for a list that already exists.
 *   d_index [n][capacity] u32: the source rank of every kept entry; d_counts_out [n] u32: their number; d_overflow [n] u32 (all three
 *   required). Gathered copies through the index, each pair nullable: d_xyz_out; d_pixel -> d_pixel_out (u32); d_gray -> d_gray_out (u8);
 *   d_normals -> d_normals_out. With d_segments / d_n_segments / max_keyframes and d_segments_out: the used records for the filtered
 *   list — first = the kept ranks below the old first, count = the kept ranks in [first, first + count) of the source, frame and pose7
 *   kept. Entries at or beyond a list's kept count are not written.
 *   d_workspace: vors_voxel_filter_workspace_bytes(n, capacity, table_slots) bytes, 16-byte aligned — per list a table of table_slots (a
 *   power of two in 64..2^30) entries of 16 bytes, emptied inside the call, and 4 bytes per 1024 ranks of capacity. The probes are the
 *   keyframe map's (open addressing, linear probing, the owner of a voxel the minimum rank): the result does not depend on scheduling,
 *   on the other lists, on the stream or on table_slots while a list's distinct voxels are <= table_slots. Beyond that the list's
 *   overflow word is set and its outputs are unspecified (every store stays inside its buffers, a point probes at most table_slots
 *   entries); the other lists keep the exact result.
 *   Six launches: EMPTY, CLAIM, COUNT, SCAN, WRITE, SEGMENTS (the last with d_segments_out only). Refused with VORS_ERR_INVALID_ARGUMENT,
 *   nothing enqueued: a NULL required pointer; n outside 1..65535; capacity < 1; voxel_m not finite or <= 0; a bad table_slots; a gathered
 *   output without its input; d_segments_out without the records, their count or max_keyframes >= 1; an array off its alignment; ANY
 *   overlap of an output or the workspace with an input or another output (nothing may be filtered in place); a stream of another device. */
uint64_t vors_voxel_filter_workspace_bytes(int n, int capacity, int table_slots);  /* 0 for arguments the pass refuses */
vors_status vors_voxel_filter_points(int n, const float* d_xyz, const uint32_t* d_list_counts, int capacity, float voxel_m, int table_slots,
                                     void* d_workspace, const uint32_t* d_pixel /* nullable */, const uint8_t* d_gray /* nullable */,
                                     const float* d_normals /* nullable */, const vors_map_segment* d_segments /* nullable */,
                                     const uint32_t* d_n_segments /* nullable */, int max_keyframes, uint32_t* d_index, uint32_t* d_counts_out,
                                     uint32_t* d_overflow, float* d_xyz_out /* nullable */, uint32_t* d_pixel_out /* nullable */,
                                     uint8_t* d_gray_out /* nullable */, float* d_normals_out /* nullable */,
                                     vors_map_segment* d_segments_out /* nullable */, void* hip_stream);
/* The same for ONE list in HOST memory (no GPU): the first occurrence of every key of vors_voxel_keys. No workspace; *overflow is 1
 * when the list's distinct voxels exceed table_slots — where the device's result is unspecified — and the result is exact all the same. */
vors_status vors_voxel_filter_points_host(const float* xyz, uint32_t count, int capacity, float voxel_m, int table_slots,
                                          const uint32_t* pixel /* nullable */, const uint8_t* gray /* nullable */,
                                          const float* normals /* nullable */, const vors_map_segment* segments /* nullable */,
                                          uint32_t n_segments, int max_keyframes, uint32_t* index, uint32_t* count_out, uint32_t* overflow,
                                          float* xyz_out /* nullable */, uint32_t* pixel_out /* nullable */, uint8_t* gray_out /* nullable */,
                                          float* normals_out /* nullable */, vors_map_segment* segments_out /* nullable */);

/* ------------------------------------------------------------------------------------------------------------
 * 3. Operator level — the optimizer trait's pieces for one pyramid level.  Replaces, for
 *    `impl optimizer::State<Obs, EvalState, Iso3, String> for LMOptimizerState` (lm_optimizer.rs:111-193):
 *      vors_lm_eval  = eval_energy + compute_eval_data at a model          lm_optimizer.rs:68-107 (the body of init/eval)
 *      vors_lm_step  = step()                                              lm_optimizer.rs:123-136
 *      vors_lm_solve = State::iterative_solve(&obs, model)                 src/math/optimizer.rs:57-70
 *    vors_obs replaces `pub struct Obs<'a>` (lm_optimizer.rs:43-58); hessians are not passed (J J^T is recomputed).
 *    Host buffers, row-major images.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct vors_obs {
    float cu, cv, fu, fv, skew; /* Obs::intrinsics (of this level) */
    int32_t rows, cols;         /* shape of template and image */
    const uint8_t* template_;   /* Obs::template (keyframe image of this level) */
    const uint8_t* image;       /* Obs::image (current image of this level) */
    int32_t n;                  /* number of candidates */
    const int32_t* coordinates; /* Obs::coordinates: (x, y) pairs, int32[2n] */
    const float* _z_candidates; /* Obs::_z_candidates: inverse depths, f32[n] */
    const float* jacobians;     /* Obs::jacobians: f32[6n] */
    float huber_delta;          /* extension, <= 0 = reference */
    int32_t arithmetic;         /* VORS_ARITH_EXACT (sums in the device's tree order) or VORS_ARITH_REFERENCE: sequential f32 sums in the
                                 * order of `coordinates` — the reference's eval on this Obs, bit for bit (lm_optimizer.rs:68-107) */
} vors_obs;

vors_status vors_lm_eval(const vors_obs* obs, const float model7[7], float* energy, int32_t* n_inside, float g[6],
                         float H[36] /* row-major 6x6 */, float* residuals /* nullable f32[n], NaN = outside */);
/* Host-only arithmetic (6x6 Cholesky + se3::exp + compose + renormalise). *chol_ok = 0 mirrors
 * Err("Error at Cholesky decomposition of hessian"). */
vors_status vors_lm_step(const float H[36], const float g[6], const float model7[7], float lm_coef, float out_model7[7],
                         int* chol_ok);
/* *solve_status: VORS_TRACK_OK or VORS_TRACK_OPTIMIZER_FAILED_POSE_KEPT (step error). */
vors_status vors_lm_solve(const vors_obs* obs, const float model7[7], float out_model7[7], int32_t* nb_iter, float* energy,
                          float* lm_coef, int* solve_status);

/* ------------------------------------------------------------------------------------------------------------
 * 4. Lie algebra helpers (host arithmetic; src/math/se3.rs:65-129, src/math/so3.rs:62-99). API parity only:
 *    the tracker itself only uses se3::exp.
 * ---------------------------------------------------------------------------------------------------------- */
void vors_se3_exp(const float xi[6], float out_iso7[7]);
void vors_se3_log(const float iso7[7], float out_xi[6]);
/* sinf / cosf as se3::exp evaluates them here, host and device alike (csrc/lie.h ref_sinf / ref_cosf: glibc's algorithm restated; equal to
 * the platform's sinf / cosf for every f32 in [0, 4), which tests/test_oracle_kat.py checks exhaustively). Outputs nullable. */
void vors_ref_sincos(const float* x, int n, float* sin_out, float* cos_out);
void vors_so3_exp(const float w[3], float out_q4[4]);
void vors_so3_log(const float q4[4], float out_w[3]);
void vors_iso_mul(const float a7[7], const float b7[7], float out7[7]);
void vors_iso_inverse(const float a7[7], float out7[7]);
/* inverse_depth.rs:24-29 and :37-42 for arrays (host arithmetic). from_depth: 0 -> NaN (Unknown), else scale / depth. to_depth:
 * roundf(scale / idepth) — halves away from zero, f32::round — converted like Rust's `as u16`: NaN -> 0, <= 0 -> 0, >= 65535 -> 65535. */
void vors_to_depth(float scale, const float* idepth, int n, uint16_t* depth_out);
void vors_from_depth(float scale, const uint16_t* depth, int n, float* idepth_out);
/* Camera::back_project and Camera::project for arrays (host arithmetic; cam5 = cu cv fu fv skew, pose7 = camera -> world, NULL =
 * identity: no transform at all). back_project: pose * intrinsics.back_project((x, y), depth) (camera.rs:43-45, 75-77, 135-140), the text
 * vors_batch_point_cloud runs per point. project: intrinsics.project(rotation.inverse() * (translation.inverse() * point))
 * (camera.rs:36-39, 70-72, 126-132) -> homogeneous (u w, v w, w), no division. xy [2n], depth [n], xyz [3n], uvw [3n]; n = 0 is legal. */
void vors_camera_back_project(const float cam5[5], const float pose7[7] /* nullable */, const float* xy, const float* depth, int n, float* xyz_out);
void vors_camera_project(const float cam5[5], const float pose7[7] /* nullable */, const float* xyz, int n, float* uvw_out);
/* The voxel of a point on a grid of edge voxel_m, for arrays (host arithmetic): the text the voxel filter of the keyframe map runs per
 * point (vors_trackers_enable_map_voxels). Per axis q = floorf(w / voxel_m), an IEEE f32 division. A point has a key iff all three q are
 * finite and -2^20 <= q < 2^20: key = (q_x + 2^20) | (q_y + 2^20) << 21 | (q_z + 2^20) << 42, below 2^63. Every other point — NaN,
 * infinities, a quotient out of range — and every point when voxel_m is not finite or <= 0 gets VORS_VOXEL_NONE. xyz [3n], keys_out [n];
 * n = 0 is legal. */
#define VORS_VOXEL_NONE 0xFFFFFFFFFFFFFFFFull
void vors_voxel_keys(float voxel_m, const float* xyz, int n, uint64_t* keys_out);

/* ------------------------------------------------------------------------------------------------------------
 * 5. Synthetic scene renderer on the device (bench/test tooling). Renders, for pair i in
 *    [0, n_pairs), the keyframe (identity) and the current frame (exp(xi(seed0+i))) of the textured-plane scene
 *    into DEVICE buffers, and the ground-truth models (keyframe->current) into d_gt_models7 (nullable).
 * ---------------------------------------------------------------------------------------------------------- */
vors_status vors_synth_render_pairs(uint64_t seed0, int n_pairs, int rows, int cols, const double cam5[5],
                                    double motion_scale, int invalid_percent, uint8_t* d_kf_gray, uint16_t* d_kf_depth,
                                    uint8_t* d_cur_gray, uint16_t* d_cur_depth /* nullable */, float* d_gt_models7,
                                    void* hip_stream);

/* Frames of the same scene at explicit twists (sequence tooling): frame f = scene seeds[f], depth-dropout salt salts[f], camera at
 * exp(xi6[6 f .. 6 f + 5]) (twist (v, w), keyframe -> camera); host tables, DEVICE images [n_frames, rows, cols]. Synchronises. */
vors_status vors_synth_render_frames(int n_frames, const uint64_t* seeds, const uint64_t* salts, const double* xi6, int rows, int cols,
                                     const double cam5[5], int invalid_percent, uint8_t* d_gray, uint16_t* d_depth, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VORS_HIP_H */
