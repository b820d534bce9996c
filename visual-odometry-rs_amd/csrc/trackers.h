// The sequence handles as their two host units share them (private: not installed). trackers.cpp holds the lock-step state machine, the
// depth filter and the single Tracker's frame loop; trackers_map.cpp holds everything of the keyframe map (vors_trackers::Map).
#pragma once
#include "host_common.h"

// ---------------------------------------------------------------------------------------------------------------
// N sequences in lock-step, device resident (vors_trackers_*): the state machine of Tracker::track
// (inverse_compositional.rs:170-240) for every sequence without a host round trip — initial guess from the poses kept on the device,
// LM, pose composition, keyframe test, and the promotion of the current frame to keyframe for exactly the sequences whose optical flow
// reached the threshold (masked launches of the keyframe stage over the list trackers_advance_kernel builds).
// ---------------------------------------------------------------------------------------------------------------
struct vors_trackers {
    vors_batch* batch = nullptr;
    int n_seq = 0;
    int frame_index = 0;  // index of the last frame submitted (0 = the init frame)
    bool initialised = false;
    DevBuf cur_poses, kf_poses, out_poses, status, stats, kf_frame, promo_list, promo_count, frame_counter;
    DevBuf own_gray, own_depth;  // dense mode: the keyframes' level 0 and depth maps (re-read by every evaluation) live in the handle
    // Depth filter (vors_trackers_enable_depth_filter; off: nothing below exists and no launch changes). The planes belong to the batch
    // handle's resources (counted by its workspace figure, freed with it), [n_seq][S0] each:
    //   zkey          the keyed z-buffer of a promotion
    //   fused         the merge's depth output. Sparse modes: it IS the keyframe depth (nothing else reads a keyframe's depth map there).
    //                 Dense mode: staging — the splat reads own_depth, the keyframe depth — copied into own_depth for the promoted sequences
    //   weight        the keyframes' weights, read by the splat and gathered by the merge at the SOURCE pixel, hence:
    //   stage_weight  the merge's weight output, copied into `weight` for the promoted sequences
    struct DepthFilter {
        bool on = false;
        float tol_m = 0.f;
        int max_weight = 255, fill_min_weight = 0;
        uint64_t* zkey = nullptr;
        uint16_t* fused = nullptr;
        uint8_t *weight = nullptr, *stage_weight = nullptr;
    } filter;
    // Keyframe map (vors_trackers_enable_map; off: nothing below exists and no launch changes). Lists, segment records, counters and the
    // count workspace of the point-cloud pass belong to the batch handle's resources, like the filter's planes:
    //   xyz / pixel / gray  [n_seq][capacity] entries, the clouds of a sequence's keyframes one after the other
    //   counts, n_segments  [n_seq] running totals (kept points, keyframes)
    //   segments            [n_seq][max_keyframes]
    //   ws                  [n_seq][ws_chunks] kept points per chunk of the keyframe being appended
    struct Map {
        bool on = false;
        int level = 0, capacity = 0, max_keyframes = 0, min_weight = 0, ws_chunks = 0;
        float* xyz = nullptr;
        uint32_t *pixel = nullptr, *counts = nullptr, *n_segments = nullptr, *ws = nullptr;
        uint8_t* gray = nullptr;
        vors_map_segment* segments = nullptr;
        // Voxel filter of the map (vors_trackers_enable_map_voxels; off: nothing below exists and the emission is the unfiltered one):
        //   table               [n_seq][table_slots][2] 64-bit words, voxel key and owner tag of an entry, all ones = empty
        //   occupied, overflow  [n_seq] claimed entries; sticky flag of a sequence whose voxels outgrew its table
        struct Voxels {
            bool on = false;
            float voxel_m = 0.f;
            int table_slots = 0;
            unsigned long long* table = nullptr;
            uint32_t *occupied = nullptr, *overflow = nullptr;
            // Statistics of the voxels (vors_trackers_enable_map_voxel_stats; off: nothing below exists and the emission is the filter's):
            //   rank_of  [n_seq][table_slots] the rank of an entry's voxel in the list, all ones = none; cleared with the table
            //   sums     [n_seq][capacity][4] int64, obs [n_seq][capacity][2] u32: rank-aligned with the lists
            bool stats = false;
            uint32_t *rank_of = nullptr, *obs = nullptr;
            long long* sums = nullptr;
        } voxels;
        // Normals of the map (vors_trackers_enable_map_normals; off: nothing below exists and no launch changes):
        //   n      [n_seq][capacity][3] the normal of every stored entry, rank for rank
        //   first  [n_seq] the running totals as they stood before the emission in flight: the ranks its normals pass starts from
        struct Normals {
            bool on = false;
            int step = 0;
            float jump_m = 0.f;
            float* n = nullptr;
            uint32_t* first = nullptr;
        } normals;
        // ICP correction at promotion (vors_trackers_enable_map_icp; off: nothing below exists and no launch changes):
        //   workspace          the ICP pass's (engine.h icp_workspace_bytes)
        //   promoted, ranges   [n_seq], [n_seq][2]: this call's promotion flags and windows
        //   start, result      [n_seq][7] the ICP's input and output poses
        //   stats, gates       [n_seq] staging of the ICP's statistics and gate counts, copied into the records by APPLY
        //   records, totals    [n_seq], [n_seq][2]: what vors_trackers_map_icp shows
        //   frame_normals      [n_seq][S0][3], with normal_gate only
        // Through the joint pass with the condition test (vors_trackers_enable_map_icp_joint; `joint`, otherwise nothing below exists):
        //   jp                 the parameters; p above is jp.icp
        //   sums29, photo_counts   [n_seq][29], [n_seq][VORS_ICP_PHOTO_COUNTS] staging of the pass's final sums and photo counts
        //   joint_records      [n_seq], beside records: what vors_trackers_map_icp_joint shows
        // With the averaged model (vors_trackers_enable_map_icp_means; `means`, otherwise nothing below exists):
        //   mean_xyz, mean_gray    [n_seq][capacity][3], [n_seq][capacity] staging of the resolve, rank-aligned with the lists: the pass's
        //                          xyz and (joint) list grey in the lists' place
        //   means_records          [n_seq]: what vors_trackers_map_icp_means shows
        struct Icp {
            bool on = false, joint = false;
            vors_map_icp_params p{};
            vors_map_icp_joint_params jp{};
            float* sums29 = nullptr;
            uint32_t* photo_counts = nullptr;
            vors_map_icp_joint_record* joint_records = nullptr;
            vors::MapIcpGates gates{};
            void* workspace = nullptr;
            uint32_t *promoted = nullptr, *ranges = nullptr, *gate_counts = nullptr, *totals = nullptr;
            float *start = nullptr, *result = nullptr, *frame_normals = nullptr;
            vors_icp_stats* stats = nullptr;
            vors_map_icp_record* records = nullptr;
            bool means = false;
            uint32_t means_min_count = 1, means_min_span = 0;
            float* mean_xyz = nullptr;
            uint8_t* mean_gray = nullptr;
            vors_map_icp_means_record* means_records = nullptr;
        } icp;
    } map;
    const uint16_t* keyframe_depth() const {
        return batch->g.mode == VORS_CANDIDATES_DENSE ? static_cast<const uint16_t*>(own_depth.p) : filter.fused;
    }
    ~vors_trackers() { vors_batch_destroy(batch); }
};

// ---------------------------------------------------------------------------------------------------------------
// Tracker: one sequence (Config::init / Tracker::track / Tracker::current_frame)
// ---------------------------------------------------------------------------------------------------------------
// The single sequence is the N = 1 case of the lock-step engine (vors_trackers_*): poses, the keyframe test and the promotion of
// the current frame stay on the device, so a frame is ONE chain of stream-ordered work and ONE synchronisation — upload (pinned staging,
// the depth map on a second stream: it is only read by a promotion, after the LM stage), Tracker::track, read-back of pose / status /
// diagnostics. The host mirrors only what current_frame() / keyframe() report.
struct vors_tracker {
    vors_config cfg;
    int rows = 0, cols = 0, layout = 0, device = 0;
    vors_trackers* seq = nullptr;  // n_sequences = 1
    DevBuf gray, depth, tmp8, tmp16;   // the frame on the device (row-major); tmp*: column-major uploads before the transpose
    PinnedBuf h_gray, h_depth, h_out;  // staging: frame in; pose7 + status + keyframe index + vors_pair_stats out
    DevBuf render_zkey, render_depth, render_gray, render_args;  // vors_tracker_render_map: created by its first call (level 0's shape)
    hipStream_t s_main = nullptr, s_copy = nullptr;
    hipEvent_t ev_depth = nullptr, ev_frame_done = nullptr, ev_result = nullptr;
    // State of inverse_compositional.rs:52-60 as the host reports it
    double keyframe_depth_timestamp = 0, keyframe_img_timestamp = 0;
    vors::Iso keyframe_pose = vors::iso_identity();
    double current_frame_depth_timestamp = 0, current_frame_img_timestamp = 0;
    vors::Iso current_frame_pose = vors::iso_identity();
    vors_pair_stats last{};
    bool has_last = false;
    ~vors_tracker() {
        vors_trackers_destroy(seq);
        if (ev_depth) (void)hipEventDestroy(ev_depth);
        if (ev_frame_done) (void)hipEventDestroy(ev_frame_done);
        if (ev_result) (void)hipEventDestroy(ev_result);
        if (s_main) (void)hipStreamDestroy(s_main);
        if (s_copy) (void)hipStreamDestroy(s_copy);
    }
};
struct TrackerOut {  // layout of vors_tracker::h_out
    float pose[7];
    int32_t status, kf_index;
    vors_pair_stats stats;
};

// What crosses the two units. Internal: hidden, so that the library's dynamic symbols stay the ones it had.
#pragma GCC visibility push(hidden)
// trackers.cpp. The keyframes as the batch products read them (FuseDepthCall, PointCloudAppendCall): the records, and in dense mode the
// handle's own level 0 and depth maps with the batch's upper levels. No current frame: these passes never read one.
vors::LmScene keyframe_scene(vors_trackers* t);
// trackers_map.cpp, for vors_trackers_init: the map, the correction's records and the averaged model's staging as a handle starts (and
// starts again) with ...
vors_status trackers_map_init(vors_trackers* t, const uint16_t* depth, hipStream_t s);
vors_status trackers_map_icp_init(vors_trackers* t, hipStream_t s);
vors_status trackers_map_icp_means_init(vors_trackers* t, hipStream_t s);
// ... and for trackers_promote: the ICP correction of the promoted sequences, and the emission of their new keyframes behind it.
void trackers_map_icp_stage(vors_trackers* t, const vors::Geom& gm, const uint16_t* depth, const uint8_t* gray, hipStream_t s);
void trackers_map_emit_all(vors_trackers* t, const vors::Geom& gm, const uint16_t* depth, hipStream_t s);
#pragma GCC visibility pop
