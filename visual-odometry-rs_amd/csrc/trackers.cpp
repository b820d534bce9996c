// Sequences: N of them in lock-step on the device (vors_trackers_*), and the single Tracker of the reference as their N = 1 case
// (vors_tracker_*). Both sit on a batch handle (host_common.h, batch.cpp).
#include <algorithm>
#include <cstring>
#include <memory>

#include "host_common.h"

using namespace vors;

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
            MapIcpGates gates{};
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

// The keyframes as the batch products read them (FuseDepthCall, PointCloudAppendCall): the records, and in dense mode the handle's own
// level 0 and depth maps with the batch's upper levels. No current frame: these passes never read one.
static LmScene keyframe_scene(vors_trackers* t) {
    const vors_batch* b = t->batch;
    const bool dense = b->g.mode == VORS_CANDIDATES_DENSE;
    return LmScene{Pyramid{nullptr, nullptr}, Pyramid{dense ? t->own_gray.as<uint8_t>() : nullptr, b->kf_upper},
                   dense ? t->own_depth.as<uint16_t>() : nullptr, b->rec};
}

// The cloud of the NEW keyframe of every selected sequence (gm.sel_list; null: all) appended to its map. Hazards, all settled by the
// stream: the emission reads the records, own_gray / own_depth / kf_upper (dense mode) and the filter's weight plane AFTER everything that
// writes them in the same promotion (keyframe stage, column-major sort, the stage_weight -> weight copy) and the keyframe pose after
// launch_trackers_advance moved it; the next frame's LM stage only reads them too; the next promotion, which rewrites them, is enqueued
// behind. It writes the map's own buffers, which nothing else touches (the count workspace is the map's, not vors_batch_point_cloud's).
static void trackers_map_emit(vors_trackers* t, const Geom& gm, hipStream_t s) {
    PointCloudAppendCall call{keyframe_scene(t)};
    call.n_seq = t->n_seq;
    call.lvl = t->map.level;
    call.kf_poses = t->kf_poses.as<float>();
    call.kf_frame = t->kf_frame.as<int32_t>();
    call.weight = t->map.min_weight >= 2 ? t->filter.weight : nullptr;
    call.min_weight = t->map.min_weight;
    call.capacity = t->map.capacity;
    call.max_keyframes = t->map.max_keyframes;
    call.xyz = t->map.xyz;
    call.pixel = t->map.pixel;
    call.gray = t->map.gray;
    call.counts = t->map.counts;
    call.segments = t->map.segments;
    call.n_segments = t->map.n_segments;
    call.ws = t->map.ws;
    call.ws_chunks = t->map.ws_chunks;
    // The voxel filter's table is the map's own too: CLAIM, COUNT and WRITE of one emission follow each other on the stream, and the next
    // emission, which reads what this one claimed, is enqueued behind.
    const vors_trackers::Map::Voxels& v = t->map.voxels;
    if (v.on) call.voxels = PointCloudVoxelArgs{v.voxel_m, (uint32_t)v.table_slots, v.table, v.occupied, v.overflow};
    // ... and so are the statistics: WRITE stores rank_of, ACCUMULATE behind it reads rank_of and the list entries WRITE (of this or an
    // earlier emission) stored, and touches sums / obs with integer atomics only; later emissions read and extend rank_of. Besides
    // ACCUMULATE only init's clear writes sums / obs.
    if (v.stats) call.voxel_stats = PointCloudVoxelStatsArgs{v.rank_of, v.sums, v.obs};
    launch_lm_point_cloud_append(gm, call, s);
}

// The normals of the entries an emission appended (vors_trackers_enable_map_normals): the list form of the normals pass over the ranks
// [first[seq], min(counts[seq], capacity)) of the selected sequences (gm.sel_list; null: all), keyed on the stored pixels, in `depth`, the
// [n_seq][S0] planes the keyframe stage of this call ran on. Hazards: it reads map.pixel / map.counts behind the emission that wrote them
// and the keyframe pose behind launch_trackers_advance; `depth` is the handle's own plane or the caller's frame, which this call may read
// in work it enqueues; it writes map.normals.n, which nothing else touches.
static void trackers_map_normals_pass(vors_trackers* t, const Geom& gm, const uint16_t* depth, hipStream_t s) {
    const Geom& g = t->batch->g;
    NormalCall call{};
    call.n = t->n_seq;
    call.depth = depth;
    call.k = g.lv[0].k;
    call.rows = g.lv[0].rows;
    call.cols = g.lv[0].cols;
    call.depth_scale = g.depth_scale;
    call.step = t->map.normals.step;
    call.jump_m = t->map.normals.jump_m;
    call.poses = t->kf_poses.as<float>();
    call.pose_stride = 7;
    call.normals = t->map.normals.n;
    call.pixel = t->map.pixel;
    call.list_counts = t->map.counts;
    call.capacity = t->map.capacity;
    call.first = t->map.normals.first;
    call.sel_list = gm.sel_list;
    call.sel_count = gm.sel_count;
    launch_points_normals(call, s);
}
// The emission with what surrounds it when the map carries normals: the running totals are copied first, the normals pass follows.
// `depth` is read only then.
static void trackers_map_emit_all(vors_trackers* t, const Geom& gm, const uint16_t* depth, hipStream_t s) {
    const vors_trackers::Map::Normals& nm = t->map.normals;
    if (nm.on) launch_normals_snapshot(t->map.counts, nm.first, t->n_seq, s);
    trackers_map_emit(t, gm, s);
    if (nm.on) trackers_map_normals_pass(t, gm, depth, s);
}

// What every ICP pass over the handle's own map states of it, the correction's stage and the vors_trackers_icp_map* forwards alike: the
// lists, the level-0 camera and shape (map normals exist for a level-0 map only), the depth scale. The rest is the caller's.
static IcpCall map_icp_call(const vors_trackers* t, const uint16_t* depth) {
    const Geom& g = t->batch->g;
    IcpCall call{};
    call.n = t->n_seq; call.xyz = t->map.xyz; call.normals = t->map.normals.n; call.list_counts = t->map.counts; call.capacity = t->map.capacity;
    call.depth = depth; call.k = g.lv[0].k; call.rows = g.lv[0].rows; call.cols = g.lv[0].cols; call.depth_scale = g.depth_scale;
    return call;
}

// The ICP correction of the promoted sequences (vors_trackers_enable_map_icp), between the keyframe stage and the emission: ARM, the frame
// normals of the promoted sequences (normal_gate), the robust ICP pass as vors_trackers_icp_map_robust forwards it — device ranges, the
// handle's workspace, statistics and gate counts into staging — and APPLY. `depth`: the planes the emission's normals pass reads.
// Hazards, all settled by the stream: ARM reads the keyframe poses and kf_frame behind launch_trackers_advance, and the map's counts and
// segments BEFORE this promotion's emission (enqueued behind the stage) and behind the previous one; the ICP reads map.xyz / map.normals.n,
// which only an emission and its normals pass write; APPLY writes the three pose tables behind everything of this call that reads them
// (the LM stage, launch_trackers_advance, a single tracker's read-back when it is ordered here) and before the emission, the normals pass
// and the next call's LM stage, which read them. Everything else is the stage's own.
// The joint stage (vors_trackers_enable_map_icp_joint) is this sequence with three differences: the pass is the joint one — list grey =
// the map's, frame grey = `gray`, the level-0 plane the keyframe stage of this call read (the caller's frame, or own_gray behind its
// promote copy), which nothing writes before the next call — with its sums and photo counts into staging; ARM is followed by the reset
// of the joint records; APPLY is the joint one. `gray` is read only then.
// With the averaged model (vors_trackers_enable_map_icp_means) one pass stands between ARM (and the joint records' reset) and the ICP's
// first launch: the windowed resolve of the voxels' statistics into the stage's own staging, which the pass then reads as its xyz and
// (joint) list grey. Hazards: the resolve reads ic.ranges behind ARM; it reads sums, obs, the rank-aligned map.xyz, the segment records
// and n_segments as they stood BEFORE this promotion's emission (enqueued behind the stage), which only an emission writes; the ICP reads
// the staging behind the resolve; nothing else writes the staging or the means records, and the resolve writes nothing else.
static void trackers_map_icp_stage(vors_trackers* t, const Geom& gm, const uint16_t* depth, const uint8_t* gray, hipStream_t s) {
    const Geom& g = t->batch->g;
    const vors_trackers::Map& m = t->map;
    const vors_trackers::Map::Icp& ic = m.icp;
    const LevelGeom& lv = g.lv[0];  // (map normals exist for a level-0 map only)
    MapIcpCall mc{};
    mc.n = t->n_seq;
    mc.promo_list = gm.sel_list;
    mc.promo_count = gm.sel_count;
    mc.kf_frame = t->kf_frame.as<int32_t>();
    mc.counts = m.counts;
    mc.segments = m.segments;
    mc.n_segments = m.n_segments;
    mc.capacity = m.capacity;
    mc.max_keyframes = m.max_keyframes;
    mc.last_keyframes = ic.p.last_keyframes;
    mc.gates = ic.gates;
    mc.kf_poses = t->kf_poses.as<float>();
    mc.cur_poses = t->cur_poses.as<float>();
    mc.out_poses = t->out_poses.as<float>();
    mc.promoted = ic.promoted;
    mc.ranges = ic.ranges;
    mc.start_poses = ic.start;
    mc.result_poses = ic.result;
    mc.stats = ic.stats;
    mc.gate_counts = ic.gate_counts;
    mc.records = ic.records;
    mc.totals = ic.totals;
    launch_map_icp_arm(mc, s);
    // (the joint stage's record: built only where the joint stage runs, so that the plain path reads as it always did)
    auto joint_call = [&] {
        return MapIcpJointCall{mc, MapIcpConditionGates{ic.jp.max_dilution_t, ic.jp.max_dilution_r}, ic.sums29, ic.photo_counts, ic.joint_records};
    };
    if (ic.joint) launch_map_icp_arm_joint(joint_call(), s);
    if (ic.frame_normals) {
        NormalCall nc{};
        nc.n = t->n_seq;
        nc.depth = depth;
        nc.k = lv.k;
        nc.rows = lv.rows;
        nc.cols = lv.cols;
        nc.depth_scale = g.depth_scale;
        nc.step = m.normals.step;
        nc.jump_m = m.normals.jump_m;
        nc.normals = ic.frame_normals;
        nc.sel_list = gm.sel_list;
        nc.sel_count = gm.sel_count;
        launch_map_icp_frame_normals(nc, s);
    }
    IcpCall call = map_icp_call(t, depth);
    if (ic.means) {
        VoxelMeansCall vm{};
        vm.n = t->n_seq; vm.xyz = m.xyz; vm.list_counts = m.counts; vm.capacity = m.capacity; vm.sums = m.voxels.sums; vm.obs = m.voxels.obs;
        vm.voxel_m = m.voxels.voxel_m; vm.min_count = ic.means_min_count; vm.min_span = ic.means_min_span;
        vm.segments = m.segments; vm.n_segments = m.n_segments; vm.max_keyframes = m.max_keyframes;
        vm.xyz_mean = ic.mean_xyz; vm.gray_mean = ic.mean_gray; vm.ranges = ic.ranges; vm.records = ic.means_records;
        launch_voxel_means_window(vm, s);
        call.xyz = ic.mean_xyz;
    }
    call.ranges = reinterpret_cast<const uint8_t*>(ic.ranges);
    call.range_stride = 8;
    call.poses_in = ic.start;
    call.pose_stride = 7;
    call.dist_m = ic.p.dist_m;
    call.damping = ic.p.damping;
    call.step_eps = ic.p.step_eps;
    call.iters = ic.p.iters;
    call.min_points = (uint32_t)ic.p.min_points;
    icp_workspace_carve(&call, ic.workspace, t->n_seq, m.capacity);
    call.poses_out = ic.result;
    call.stats = ic.stats;
    const IcpRobust robust{ic.frame_normals, ic.p.min_cos, ic.p.huber_m, ic.gate_counts};
    if (!ic.joint) {
        launch_icp_points(call, &robust, s);
        launch_map_icp_apply(mc, s);
        return;
    }
    call.sums29 = ic.sums29;
    const IcpJoint joint{ic.means ? ic.mean_gray : m.gray, gray, ic.jp.photo_scale_m, map_icp_photo_huber_m(ic.jp), nullptr, ic.photo_counts};
    launch_icp_points(call, &robust, s, &joint);
    launch_map_icp_apply_joint(joint_call(), s);
}

// The two halves of vors_trackers_track: Tracker::track up to the keyframe test, and the promotion of the sequences that switch — the
// only reader of the depth map, which may arrive on another stream (depth_ready). vors_tracker_track runs them apart, with the depth
// upload in between.
static vors_status trackers_track_lm(vors_trackers* t, const uint8_t* d_gray, hipStream_t s) {
    if (!t || !d_gray) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "vors_trackers_track called before vors_trackers_init");
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    vors_status st = check_stream(b, s);
    if (st != VORS_OK) return st;
    const int n = t->n_seq;
    t->frame_index += 1;
    // Tracker::track up to the keyframe test (inverse_compositional.rs:177-224), all sequences
    st = batch_track_current(b, n, d_gray, t->cur_poses.as<float>(), t->kf_poses.as<float>(), t->out_poses.as<float>(), t->status.as<int32_t>(),
                             t->stats.as<vors_pair_stats>(), s);
    if (st != VORS_OK) return st;
    // :203-208 and :224-239 on the device: poses forward, promotion list
    launch_trackers_advance(n, t->frame_counter.as<int>(), t->out_poses.as<float>(), t->stats.as<vors_pair_stats>(), t->cur_poses.as<float>(),
                            t->kf_poses.as<float>(), t->kf_frame.as<int32_t>(), t->promo_list.as<int>(), t->promo_count.as<int>(), s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}


// depth_ready (nullable): an event after which d_depth holds this frame's depth map (uploaded on another stream).
static vors_status trackers_promote(vors_trackers* t, const uint8_t* d_gray, const uint16_t* d_depth, hipEvent_t depth_ready, hipStream_t s) {
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    const int n = t->n_seq;
    // precompute_multires_data (:230-235) for the promoted sequences only: the pyramid of the current frame is reused, the depth map is
    // the one that came with it
    Geom gm = b->g;
    gm.sel_list = t->promo_list.as<int>();
    gm.sel_count = t->promo_count.as<int>();
    if (depth_ready) HIP_TRY(hipStreamWaitEvent(s, depth_ready, 0));
    STAGE_BEGIN(b, 1, s);
    if (t->filter.on) {
        // The OLD keyframes of the promoted sequences (records; dense mode: own_gray / own_depth; weights) splatted at the final models of
        // this frame's LM stage and merged with the measured depth. Everything the keyframe stage below overwrites is read here, before
        // it in stream order; the merge writes planes nothing here reads. From here on the fused map stands for d_depth.
        FuseDepthCall call{keyframe_scene(t)};
        call.n_pairs = n;
        call.models = reinterpret_cast<const float*>(t->stats.p);  // (lm_model is the head of vors_pair_stats)
        call.model_stride = (int)(sizeof(vors_pair_stats) / 4);
        call.cur_depth = d_depth;
        call.tol_m = t->filter.tol_m;
        call.kf_weight = t->filter.weight;
        call.max_weight = t->filter.max_weight;
        call.fill_min_weight = t->filter.fill_min_weight;
        call.zkey = t->filter.zkey;
        call.fused_depth = t->filter.fused;
        call.fused_weight = t->filter.stage_weight;
        call.counts = nullptr;
        launch_lm_fuse_depth_selected(gm, call, s);
        launch_promote_copy(gm, t->filter.stage_weight, (size_t)b->g.S0, t->filter.weight, (size_t)b->g.S0, (size_t)b->g.S0, n, s);
        d_depth = t->filter.fused;
    }
    if (b->g.mode == VORS_CANDIDATES_DENSE) {
        const size_t S = (size_t)b->g.S0;
        launch_promote_copy(gm, d_gray, S, t->own_gray.p, S, S, n, s);
        launch_promote_copy(gm, d_depth, 2 * S, t->own_depth.p, 2 * S, 2 * S, n, s);
        launch_promote_copy(gm, b->cur_upper, (size_t)b->g.upper_stride, b->kf_upper, (size_t)b->g.upper_stride, (size_t)b->g.upper_stride, n, s);
        launch_keyframe(gm, Pyramid{t->own_gray.as<uint8_t>(), b->kf_upper}, t->own_depth.as<uint16_t>(), b->rec, n, s);
    } else if (b->g.mode == VORS_CANDIDATES_DSO) {
        launch_keyframe_dso(gm, Pyramid{d_gray, b->cur_upper}, d_depth, b->dso, b->mask0, b->pp, b->rec, n, s);
    } else {
        launch_keyframe(gm, Pyramid{d_gray, b->cur_upper}, d_depth, b->rec, n, s);
    }
    if (b->g.arith == VORS_ARITH_REFERENCE) {
        launch_sort_colmajor(gm, b->rec, n, s);
        if (b->g.mode == VORS_CANDIDATES_DENSE)
            launch_ref_dense_planes_keyframe(gm, Pyramid{t->own_gray.as<uint8_t>(), b->kf_upper}, t->own_depth.as<uint16_t>(), b->rec, n, s);
    }
    if (t->map.on) {
        const uint16_t* map_depth = b->g.mode == VORS_CANDIDATES_DENSE ? t->own_depth.as<uint16_t>() : d_depth;
        if (t->map.icp.on)
            trackers_map_icp_stage(t, gm, map_depth, b->g.mode == VORS_CANDIDATES_DENSE ? t->own_gray.as<uint8_t>() : d_gray, s);
        trackers_map_emit_all(t, gm, map_depth, s);
    }
    STAGE_END(b, 1, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Tracker: one sequence (Config::init / Tracker::track / Tracker::current_frame)
// ---------------------------------------------------------------------------------------------------------------
// The single sequence is the N = 1 case of the lock-step engine below (vors_trackers_*): poses, the keyframe test and the promotion of
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
    Iso keyframe_pose = iso_identity();
    double current_frame_depth_timestamp = 0, current_frame_img_timestamp = 0;
    Iso current_frame_pose = iso_identity();
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

// Frame -> device (row-major). The caller's buffers are pageable: they are copied into pinned staging first, so that the transfers are
// truly asynchronous (the depth map travels on its own stream under the LM stage).
// Two halves, so that vors_tracker_track can stage the depth map (the larger copy, on the CPU) WHILE the device already runs the pyramid
// and the LM stage of the frame: only the promotion at the end of the frame reads it.
static vors_status tracker_upload_gray(vors_tracker* t, const uint8_t* gray) {
    const size_t S = (size_t)t->rows * t->cols;
    std::memcpy(t->h_gray.p, gray, S);  // (the previous upload has completed: its results were waited for)
    if (t->layout == VORS_ROW_MAJOR) {
        HIP_TRY(hipMemcpyAsync(t->gray.p, t->h_gray.p, S, hipMemcpyHostToDevice, t->s_main));
    } else {
        HIP_TRY(hipMemcpyAsync(t->tmp8.p, t->h_gray.p, S, hipMemcpyHostToDevice, t->s_main));
        launch_transpose_u8(t->tmp8.as<uint8_t>(), t->gray.as<uint8_t>(), t->rows, t->cols, 1, t->s_main);
    }
    return VORS_OK;
}
static vors_status tracker_upload_depth(vors_tracker* t, const uint16_t* depth) {
    const size_t S = (size_t)t->rows * t->cols;
    HIP_TRY(hipEventSynchronize(t->ev_depth));  // (track() returns once the RESULTS are back: the previous depth upload may still be reading the staging buffer)
    std::memcpy(t->h_depth.p, depth, S * 2);
    // the previous frame's promotion may still read t->depth: the copy stream first waits for the end of the previous frame
    HIP_TRY(hipStreamWaitEvent(t->s_copy, t->ev_frame_done, 0));
    if (t->layout == VORS_ROW_MAJOR) {
        HIP_TRY(hipMemcpyAsync(t->depth.p, t->h_depth.p, S * 2, hipMemcpyHostToDevice, t->s_copy));
    } else {
        HIP_TRY(hipMemcpyAsync(t->tmp16.p, t->h_depth.p, S * 2, hipMemcpyHostToDevice, t->s_copy));
        launch_transpose_u16(t->tmp16.as<uint16_t>(), t->depth.as<uint16_t>(), t->rows, t->cols, 1, t->s_copy);
    }
    HIP_TRY(hipEventRecord(t->ev_depth, t->s_copy));
    return VORS_OK;
}
static vors_status tracker_upload(vors_tracker* t, const uint8_t* gray, const uint16_t* depth) {
    vors_status st = tracker_upload_gray(t, gray);
    return st != VORS_OK ? st : tracker_upload_depth(t, depth);
}

// The filter's state of frame 0: the keyframe depth is the measured depth, seen once where it is non-zero.
static vors_status trackers_filter_init(vors_trackers* t, const uint16_t* d_depth, hipStream_t s) {
    const size_t n = (size_t)t->n_seq, S = (size_t)t->batch->g.S0;
    if (t->batch->g.mode != VORS_CANDIDATES_DENSE) HIP_TRY(hipMemcpyAsync(t->filter.fused, d_depth, n * S * 2, hipMemcpyDeviceToDevice, s));
    launch_depth_weight_init(d_depth, t->filter.weight, n * S, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}
// The switch itself: the refusals of vors_batch_fuse_depth, then every plane at once.
static vors_status trackers_filter_enable(vors_trackers* t, float tol_m, int max_weight, int fill_min_weight) {
    if (t->filter.on) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: the filter is already enabled");
    if (!(tol_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: tol_m must be >= 0 (and not NaN)");
    if (max_weight < 1 || max_weight > 255) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: max_weight must be in 1..255");
    if (fill_min_weight < 0 || fill_min_weight > 255) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: fill_min_weight must be in 0..255");
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    const size_t planes = (size_t)t->n_seq * (size_t)b->g.S0;
    b->own.alloc(&t->filter.zkey, planes);
    b->own.alloc(&t->filter.fused, planes);
    b->own.alloc(&t->filter.weight, planes);
    b->own.alloc(&t->filter.stage_weight, planes);
    if (b->own.err != hipSuccess) return own_alloc_failed(b, "depth filter planes");
    t->filter.tol_m = tol_m;
    t->filter.max_weight = max_weight;
    t->filter.fill_min_weight = fill_min_weight;
    t->filter.on = true;
    return VORS_OK;
}

// The switch itself: every refusal, then every buffer at once.
static vors_status trackers_map_enable(vors_trackers* t, int level, int capacity, int max_keyframes, int min_weight) {
    vors_batch* b = t->batch;
    if (t->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: the map is already enabled");
    if (level < 0 || level >= b->g.L) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: level out of range");
    if (capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: capacity must be >= 1");
    if (max_keyframes < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: max_keyframes must be >= 1");
    if (min_weight < 0 || min_weight > 255) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: min_weight must be in 0..255");
    if (min_weight >= 2 && !t->filter.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: min_weight >= 2 needs the depth filter enabled first (its weights are what is tested)");
    if (min_weight >= 2 && level != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: min_weight >= 2 needs level 0 (the weight plane exists at full resolution only)");
    DeviceGuard guard(b->device);
    const size_t n = (size_t)t->n_seq;
    const int chunks = eval_pairs_chunks(b->g, level);
    b->own.alloc(&t->map.xyz, n * (size_t)capacity * 3);
    b->own.alloc(&t->map.pixel, n * (size_t)capacity);
    b->own.alloc(&t->map.gray, n * (size_t)capacity);
    b->own.alloc(&t->map.segments, n * (size_t)max_keyframes);
    b->own.alloc(&t->map.counts, n);
    b->own.alloc(&t->map.n_segments, n);
    b->own.alloc(&t->map.ws, n * (size_t)chunks);
    if (b->own.err != hipSuccess) return own_alloc_failed(b, "keyframe map");
    t->map.level = level;
    t->map.capacity = capacity;
    t->map.max_keyframes = max_keyframes;
    t->map.min_weight = min_weight;
    t->map.ws_chunks = chunks;
    t->map.on = true;
    return VORS_OK;
}
// The voxel filter's switch: every refusal, then every buffer at once. `started`: the handle has passed the point up to which the call
// is legal (vors_trackers_init / the first vors_tracker_track).
static vors_status trackers_map_voxels_enable(vors_trackers* t, bool started, const char* before, float voxel_m, int table_slots) {
    if (!t->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: needs an enabled keyframe map first (vors_trackers_enable_map)");
    if (t->map.voxels.on) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: the voxel filter is already enabled");
    if (started) return fail(VORS_ERR_INVALID_ARGUMENT, std::string("enable_map_voxels: legal only before ") + before);
    if (!(voxel_m > 0.0f) || !(voxel_m <= 3.4028234663852886e38f))
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: voxel size voxel_m must be finite and > 0");
    if (table_slots < 64 || table_slots > (1 << 30) || (table_slots & (table_slots - 1)) != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: table_slots must be a power of two in 64..2^30");
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    const size_t n = (size_t)t->n_seq;
    vors_trackers::Map::Voxels& v = t->map.voxels;
    b->own.alloc(&v.table, n * (size_t)table_slots * 2);
    b->own.alloc(&v.occupied, n);
    b->own.alloc(&v.overflow, n);
    if (b->own.err != hipSuccess) return own_alloc_failed(b, "voxel table of the keyframe map");
    v.voxel_m = voxel_m;
    v.table_slots = table_slots;
    v.on = true;
    return VORS_OK;
}
// The switch of the voxels' statistics: every refusal, then every buffer at once. `started` / `before`: as for the voxel filter.
static vors_status trackers_map_voxel_stats_enable(vors_trackers* t, bool started, const char* before) {
    vors_trackers::Map::Voxels& v = t->map.voxels;
    if (!v.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxel_stats: needs the voxel filter of the map first (vors_trackers_enable_map_voxels)");
    if (v.stats) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxel_stats: the statistics are already enabled");
    if (started) return fail(VORS_ERR_INVALID_ARGUMENT, std::string("enable_map_voxel_stats: legal only before ") + before);
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    const size_t n = (size_t)t->n_seq;
    uint32_t *rank_of = nullptr, *obs = nullptr;
    long long* sums = nullptr;
    b->own.alloc(&rank_of, n * (size_t)v.table_slots);
    b->own.alloc(&sums, n * (size_t)t->map.capacity * 4);
    b->own.alloc(&obs, n * (size_t)t->map.capacity * 2);
    if (b->own.err != hipSuccess) return own_alloc_failed(b, "voxel statistics of the keyframe map");
    v.rank_of = rank_of;
    v.sums = sums;
    v.obs = obs;
    v.stats = true;
    return VORS_OK;
}
// The normals' switch: every refusal, then both buffers at once. `started` / `before`: as for the voxel filter.
static vors_status trackers_map_normals_enable(vors_trackers* t, bool started, const char* before, int step, float jump_m) {
    if (!t->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_normals: needs an enabled keyframe map first (vors_trackers_enable_map)");
    if (t->map.level != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_normals: needs a map of level 0 (depth planes exist at full resolution only)");
    if (t->map.normals.on) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_normals: the normals are already enabled");
    if (started) return fail(VORS_ERR_INVALID_ARGUMENT, std::string("enable_map_normals: legal only before ") + before);
    if (step < 1 || step > 8) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_normals: step must be in 1..8");
    if (!(jump_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_normals: jump_m must be >= 0 (and not NaN)");
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    const size_t n = (size_t)t->n_seq;
    vors_trackers::Map::Normals& nm = t->map.normals;
    b->own.alloc(&nm.n, n * (size_t)t->map.capacity * 3);
    b->own.alloc(&nm.first, n);
    if (b->own.err != hipSuccess) return own_alloc_failed(b, "normals of the keyframe map");
    nm.step = step;
    nm.jump_m = jump_m;
    nm.on = true;
    return VORS_OK;
}
// The ICP correction's switch: every refusal, then every buffer at once. `started` / `before`: as for the voxel filter.
// jp: NULL = vors_trackers_enable_map_icp with p; otherwise vors_trackers_enable_map_icp_joint (p is not read). One flag for both: either
// enable after the other finds the correction already enabled.
static vors_status trackers_map_icp_enable(vors_trackers* t, bool started, const char* before, const vors_map_icp_params* p,
                                           const vors_map_icp_joint_params* jp = nullptr, bool joint = false) {
    const std::string w(joint ? "enable_map_icp_joint" : "enable_map_icp");
    if (!t->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": needs an enabled keyframe map first (vors_trackers_enable_map)");
    if (!t->map.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": needs the normals of the map first (vors_trackers_enable_map_normals)");
    if (t->map.icp.on) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the correction is already enabled");
    if (started) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": legal only before " + before);
    vors_status st = joint ? map_icp_joint_params_refusals(w.c_str(), jp) : map_icp_params_refusals(w.c_str(), p);
    if (st != VORS_OK) return st;
    if (joint) p = &jp->icp;
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    const size_t n = (size_t)t->n_seq;
    vors_trackers::Map::Icp& ic = t->map.icp;
    uint8_t* ws = nullptr;
    b->own.alloc(&ws, icp_workspace_bytes(t->n_seq, t->map.capacity));
    b->own.alloc(&ic.promoted, n);
    b->own.alloc(&ic.ranges, n * 2);
    b->own.alloc(&ic.start, n * 7);
    b->own.alloc(&ic.result, n * 7);
    b->own.alloc(&ic.stats, n);
    b->own.alloc(&ic.gate_counts, n * VORS_ICP_GATE_COUNTS);
    b->own.alloc(&ic.records, n);
    b->own.alloc(&ic.totals, n * 2);
    if (p->normal_gate) b->own.alloc(&ic.frame_normals, n * (size_t)b->g.S0 * 3);
    if (joint) {
        b->own.alloc(&ic.sums29, n * 29);
        b->own.alloc(&ic.photo_counts, n * VORS_ICP_PHOTO_COUNTS);
        b->own.alloc(&ic.joint_records, n);
    }
    if (b->own.err != hipSuccess) {
        ic = vors_trackers::Map::Icp{};
        return own_alloc_failed(b, "ICP correction of the keyframe map");
    }
    ic.workspace = ws;
    ic.p = *p;
    ic.gates = map_icp_gates(*p);
    if (joint) ic.jp = *jp;
    ic.joint = joint;
    ic.on = true;
    return VORS_OK;
}
// Records and totals of the correction as a handle starts (and starts again) with: zeros, i.e. NOT_ATTEMPTED and nothing counted.
static vors_status trackers_map_icp_init(vors_trackers* t, hipStream_t s) {
    const size_t n = (size_t)t->n_seq;
    HIP_TRY(hipMemsetAsync(t->map.icp.records, 0, n * sizeof(vors_map_icp_record), s));
    HIP_TRY(hipMemsetAsync(t->map.icp.totals, 0, n * 2 * sizeof(uint32_t), s));
    if (t->map.icp.joint) HIP_TRY(hipMemsetAsync(t->map.icp.joint_records, 0, n * sizeof(vors_map_icp_joint_record), s));
    return VORS_OK;
}
// The switch of the correction's averaged model: every refusal, then every buffer at once. `started` / `before`: as for the voxel filter.
static vors_status trackers_map_icp_means_enable(vors_trackers* t, bool started, const char* before, uint32_t min_count, uint32_t min_span) {
    vors_trackers::Map::Icp& ic = t->map.icp;
    if (!t->map.voxels.stats)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp_means: needs the voxel statistics first (vors_trackers_enable_map_voxel_stats)");
    if (!ic.on)
        return fail(VORS_ERR_INVALID_ARGUMENT,
                    "enable_map_icp_means: needs the correction first (vors_trackers_enable_map_icp or vors_trackers_enable_map_icp_joint)");
    if (ic.means) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp_means: the averaged model is already enabled");
    if (started) return fail(VORS_ERR_INVALID_ARGUMENT, std::string("enable_map_icp_means: legal only before ") + before);
    vors_batch* b = t->batch;
    DeviceGuard guard(b->device);
    const size_t n = (size_t)t->n_seq;
    float* xyz = nullptr;
    uint8_t* gray = nullptr;
    vors_map_icp_means_record* records = nullptr;
    b->own.alloc(&xyz, n * (size_t)t->map.capacity * 3);
    b->own.alloc(&gray, n * (size_t)t->map.capacity);
    b->own.alloc(&records, n);
    if (b->own.err != hipSuccess) return own_alloc_failed(b, "averaged model of the ICP correction");
    ic.mean_xyz = xyz;
    ic.mean_gray = gray;
    ic.means_records = records;
    ic.means_min_count = min_count;
    ic.means_min_span = min_span;
    ic.means = true;
    return VORS_OK;
}
// Staging and records of the averaged model as a handle starts (and starts again) with: zero bytes.
static vors_status trackers_map_icp_means_init(vors_trackers* t, hipStream_t s) {
    const vors_trackers::Map::Icp& ic = t->map.icp;
    const size_t n = (size_t)t->n_seq, cap = (size_t)t->map.capacity;
    HIP_TRY(hipMemsetAsync(ic.mean_xyz, 0, n * cap * 3 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(ic.mean_gray, 0, n * cap, s));
    HIP_TRY(hipMemsetAsync(ic.means_records, 0, n * sizeof(vors_map_icp_means_record), s));
    return VORS_OK;
}
// An empty map (and an empty voxel table), then keyframe 0 of every sequence. `depth`: the planes keyframe 0 was made from, read only
// when the map carries normals.
static vors_status trackers_map_init(vors_trackers* t, const uint16_t* depth, hipStream_t s) {
    const size_t n = (size_t)t->n_seq;
    HIP_TRY(hipMemsetAsync(t->map.counts, 0, n * sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(t->map.n_segments, 0, n * sizeof(uint32_t), s));
    if (const vors_trackers::Map::Voxels& v = t->map.voxels; v.on) {
        HIP_TRY(hipMemsetAsync(v.table, 0xFF, n * (size_t)v.table_slots * 2 * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(v.occupied, 0, n * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(v.overflow, 0, n * sizeof(uint32_t), s));
        if (v.stats) {
            HIP_TRY(hipMemsetAsync(v.rank_of, 0xFF, n * (size_t)v.table_slots * sizeof(uint32_t), s));
            HIP_TRY(hipMemsetAsync(v.sums, 0, n * (size_t)t->map.capacity * 4 * sizeof(long long), s));
            HIP_TRY(hipMemsetAsync(v.obs, 0, n * (size_t)t->map.capacity * 2 * sizeof(uint32_t), s));
        }
    }
    trackers_map_emit_all(t, t->batch->g, depth, s);  // (unmasked: the handle's geometry carries no selection)
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

extern "C" {

vors_status vors_trackers_enable_map(vors_trackers* t, int level, int capacity, int max_keyframes, int min_weight) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: the handle t is NULL");
    if (t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: legal only before vors_trackers_init (keyframe 0 would be missing)");
    return trackers_map_enable(t, level, capacity, max_keyframes, min_weight);
}

vors_status vors_trackers_map(const vors_trackers* t, const float** d_xyz, const uint32_t** d_pixel, const uint8_t** d_gray,
                              const uint32_t** d_counts, const vors_map_segment** d_segments, const uint32_t** d_n_segments) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map: the handle t is NULL");
    if (!t->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, "map: the keyframe map is not enabled (vors_trackers_enable_map)");
    if (d_xyz) *d_xyz = t->map.xyz;
    if (d_pixel) *d_pixel = t->map.pixel;
    if (d_gray) *d_gray = t->map.gray;
    if (d_counts) *d_counts = t->map.counts;
    if (d_segments) *d_segments = t->map.segments;
    if (d_n_segments) *d_n_segments = t->map.n_segments;
    return VORS_OK;
}

vors_status vors_tracker_enable_map(vors_tracker* t, int level, int capacity, int max_keyframes, int min_weight) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: the handle t is NULL");
    if (t->has_last) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: legal only before the first vors_tracker_track");
    vors_status st = trackers_map_enable(t->seq, level, capacity, max_keyframes, min_weight);
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    // keyframe 0 exists since create: its records, the handle's copies (dense mode) and the identity pose are what init left on s_main
    return trackers_map_init(t->seq, nullptr, t->s_main);  // (no normals yet: they are enabled after the map)
}

vors_status vors_trackers_enable_map_normals(vors_trackers* t, int step, float jump_m) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_normals: the handle t is NULL");
    return trackers_map_normals_enable(t, t->initialised, "vors_trackers_init (keyframe 0 would have no normals)", step, jump_m);
}

vors_status vors_trackers_map_normals(const vors_trackers* t, const float** d_normals) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_normals: the handle t is NULL");
    if (!t->map.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_normals: the normals of the map are not enabled (vors_trackers_enable_map_normals)");
    if (d_normals) *d_normals = t->map.normals.n;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_normals(vors_tracker* t, int step, float jump_m) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_normals: the handle t is NULL");
    vors_trackers* q = t->seq;
    vors_status st = trackers_map_normals_enable(q, t->has_last, "the first vors_tracker_track", step, jump_m);
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    // Keyframe 0 is in the map already: its normals are the pass over every rank so far, in the plane keyframe 0 was made from — the
    // handle's copy (dense mode), the filter's copy, or t->depth, which still holds the first frame's depth map (the next upload waits for
    // ev_frame_done, which therefore moves behind this reader, as in vors_tracker_enable_depth_filter)
    const uint16_t* depth = (q->batch->g.mode == VORS_CANDIDATES_DENSE || q->filter.on) ? q->keyframe_depth() : t->depth.as<uint16_t>();
    HIP_TRY(hipMemsetAsync(q->map.normals.first, 0, sizeof(uint32_t), t->s_main));
    trackers_map_normals_pass(q, q->batch->g, depth, t->s_main);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(t->ev_frame_done, t->s_main));
    return VORS_OK;
}

vors_status vors_tracker_read_map_normals(vors_tracker* t, int capacity, float* normals) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_normals: the handle t is NULL");
    const vors_trackers::Map& m = t->seq->map;
    if (!m.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_normals: the normals of the map are not enabled (vors_tracker_enable_map_normals)");
    if (capacity < 0 || !normals) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_normals: negative capacity or NULL normals");
    DeviceGuard guard(t->device);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, m.counts, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    const size_t np = std::min<size_t>(std::min<uint32_t>(total, (uint32_t)m.capacity), (size_t)capacity);
    if (np) HIP_TRY(hipMemcpyAsync(normals, m.normals.n, np * 3 * sizeof(float), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    return VORS_OK;
}

vors_status vors_trackers_enable_map_icp(vors_trackers* t, const vors_map_icp_params* params) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp: the handle t is NULL");
    return trackers_map_icp_enable(t, t->initialised, "vors_trackers_init", params);
}

vors_status vors_trackers_map_icp(const vors_trackers* t, const vors_map_icp_record** d_records, const uint32_t** d_totals) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp: the handle t is NULL");
    if (!t->map.icp.on) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp: the ICP correction is not enabled (vors_trackers_enable_map_icp)");
    if (d_records) *d_records = t->map.icp.records;
    if (d_totals) *d_totals = t->map.icp.totals;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_icp(vors_tracker* t, const vors_map_icp_params* params) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp: the handle t is NULL");
    vors_status st = trackers_map_icp_enable(t->seq, t->has_last, "the first vors_tracker_track", params);
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    return trackers_map_icp_init(t->seq, t->s_main);
}

vors_status vors_tracker_read_map_icp(vors_tracker* t, vors_map_icp_record* record, uint32_t totals[2]) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_icp: the handle t is NULL");
    const vors_trackers::Map::Icp& ic = t->seq->map.icp;
    if (!ic.on) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_icp: the ICP correction is not enabled (vors_tracker_enable_map_icp)");
    DeviceGuard guard(t->device);
    if (record) HIP_TRY(hipMemcpyAsync(record, ic.records, sizeof(vors_map_icp_record), hipMemcpyDeviceToHost, t->s_main));
    if (totals) HIP_TRY(hipMemcpyAsync(totals, ic.totals, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    return VORS_OK;
}

vors_status vors_trackers_enable_map_icp_joint(vors_trackers* t, const vors_map_icp_joint_params* params) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp_joint: the handle t is NULL");
    return trackers_map_icp_enable(t, t->initialised, "vors_trackers_init", nullptr, params, true);
}

vors_status vors_trackers_map_icp_joint(const vors_trackers* t, const vors_map_icp_joint_record** d_joint_records) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_joint: the handle t is NULL");
    if (!t->map.icp.joint)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_joint: the joint ICP correction is not enabled (vors_trackers_enable_map_icp_joint)");
    if (d_joint_records) *d_joint_records = t->map.icp.joint_records;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_icp_joint(vors_tracker* t, const vors_map_icp_joint_params* params) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp_joint: the handle t is NULL");
    vors_status st = trackers_map_icp_enable(t->seq, t->has_last, "the first vors_tracker_track", nullptr, params, true);
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    return trackers_map_icp_init(t->seq, t->s_main);
}

vors_status vors_tracker_read_map_icp_joint(vors_tracker* t, vors_map_icp_joint_record* record) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_icp_joint: the handle t is NULL");
    const vors_trackers::Map::Icp& ic = t->seq->map.icp;
    if (!ic.joint)
        return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_icp_joint: the joint ICP correction is not enabled (vors_tracker_enable_map_icp_joint)");
    DeviceGuard guard(t->device);
    if (record) HIP_TRY(hipMemcpyAsync(record, ic.joint_records, sizeof(vors_map_icp_joint_record), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    return VORS_OK;
}

vors_status vors_trackers_enable_map_icp_means(vors_trackers* t, uint32_t min_count, uint32_t min_span) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp_means: the handle t is NULL");
    return trackers_map_icp_means_enable(t, t->initialised, "vors_trackers_init", min_count, min_span);
}

vors_status vors_trackers_map_icp_means(const vors_trackers* t, const float** d_xyz_mean, const uint8_t** d_gray_mean,
                                        const vors_map_icp_means_record** d_records) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_means: the handle t is NULL");
    if (!t->map.icp.means)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_means: the averaged model is not enabled (vors_trackers_enable_map_icp_means)");
    if (d_xyz_mean) *d_xyz_mean = t->map.icp.mean_xyz;
    if (d_gray_mean) *d_gray_mean = t->map.icp.mean_gray;
    if (d_records) *d_records = t->map.icp.means_records;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_icp_means(vors_tracker* t, uint32_t min_count, uint32_t min_span) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_icp_means: the handle t is NULL");
    vors_status st = trackers_map_icp_means_enable(t->seq, t->has_last, "the first vors_tracker_track", min_count, min_span);
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    return trackers_map_icp_means_init(t->seq, t->s_main);
}

vors_status vors_tracker_read_map_icp_means(vors_tracker* t, vors_map_icp_means_record* record) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_icp_means: the handle t is NULL");
    const vors_trackers::Map::Icp& ic = t->seq->map.icp;
    if (!ic.means)
        return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_icp_means: the averaged model is not enabled (vors_tracker_enable_map_icp_means)");
    DeviceGuard guard(t->device);
    if (record) HIP_TRY(hipMemcpyAsync(record, ic.means_records, sizeof(vors_map_icp_means_record), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    return VORS_OK;
}

vors_status vors_trackers_enable_map_voxels(vors_trackers* t, float voxel_m, int table_slots) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: the handle t is NULL");
    return trackers_map_voxels_enable(t, t->initialised, "vors_trackers_init (keyframe 0 would be unfiltered)", voxel_m, table_slots);
}

vors_status vors_trackers_map_voxels(const vors_trackers* t, const uint32_t** d_occupied, const uint32_t** d_overflow) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxels: the handle t is NULL");
    if (!t->map.voxels.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxels: the voxel filter of the map is not enabled (vors_trackers_enable_map_voxels)");
    if (d_occupied) *d_occupied = t->map.voxels.occupied;
    if (d_overflow) *d_overflow = t->map.voxels.overflow;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_voxels(vors_tracker* t, float voxel_m, int table_slots) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: the handle t is NULL");
    if (t->seq->map.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: legal only before vors_tracker_enable_map_normals (keyframe 0 is emitted again)");
    vors_status st = trackers_map_voxels_enable(t->seq, t->has_last, "the first vors_tracker_track", voxel_m, table_slots);
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    // vors_tracker_enable_map has emitted keyframe 0 unfiltered: the map is emptied and keyframe 0 emitted again, through the filter
    return trackers_map_init(t->seq, nullptr, t->s_main);  // (no normals yet: see the refusal above)
}

vors_status vors_tracker_read_map_voxels(vors_tracker* t, uint32_t* occupied, uint32_t* overflow) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_voxels: the handle t is NULL");
    const vors_trackers::Map::Voxels& v = t->seq->map.voxels;
    if (!v.on) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_voxels: the voxel filter of the map is not enabled (vors_tracker_enable_map_voxels)");
    DeviceGuard guard(t->device);
    uint32_t words[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&words[0], v.occupied, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipMemcpyAsync(&words[1], v.overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    if (occupied) *occupied = words[0];
    if (overflow) *overflow = words[1];
    return VORS_OK;
}

vors_status vors_trackers_enable_map_voxel_stats(vors_trackers* t) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxel_stats: the handle t is NULL");
    return trackers_map_voxel_stats_enable(t, t->initialised, "vors_trackers_init (keyframe 0 would not be counted)");
}

vors_status vors_trackers_map_voxel_stats(const vors_trackers* t, const int64_t** d_sums, const uint32_t** d_obs) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_stats: the handle t is NULL");
    if (!t->map.voxels.stats)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_stats: the voxel statistics are not enabled (vors_trackers_enable_map_voxel_stats)");
    if (d_sums) *d_sums = reinterpret_cast<const int64_t*>(t->map.voxels.sums);
    if (d_obs) *d_obs = t->map.voxels.obs;
    return VORS_OK;
}

vors_status vors_trackers_map_voxel_means(vors_trackers* t, uint32_t min_count, uint32_t min_span, float* d_xyz_mean, uint8_t* d_gray_mean,
                                          uint32_t* d_kept, void* hip_stream) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: the handle t is NULL");
    const vors_trackers::Map& m = t->map;
    if (!m.voxels.stats)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: the voxel statistics are not enabled (vors_trackers_enable_map_voxel_stats)");
    if (!t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: called before vors_trackers_init (there is no map yet)");
    if (!d_xyz_mean && !d_gray_mean && !d_kept)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: no output at all (d_xyz_mean, d_gray_mean and d_kept are NULL)");
    if ((uintptr_t)d_xyz_mean % 4 != 0 || (uintptr_t)d_kept % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: d_xyz_mean and d_kept must be 4-byte aligned");
    vors_batch* b = t->batch;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    vors_status st = check_stream(b, s);
    if (st != VORS_OK) return st;
    // the first segment of a rank: a binary search over the handle's segment records, inside the pass (no plane of its own)
    VoxelMeansCall call{};
    call.n = t->n_seq; call.xyz = m.xyz; call.list_counts = m.counts; call.capacity = m.capacity; call.sums = m.voxels.sums; call.obs = m.voxels.obs;
    call.voxel_m = m.voxels.voxel_m; call.min_count = min_count; call.min_span = min_span;
    call.segments = m.segments; call.n_segments = m.n_segments; call.max_keyframes = m.max_keyframes;
    call.xyz_mean = d_xyz_mean; call.gray_mean = d_gray_mean; call.kept = d_kept;
    launch_voxel_means(call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_tracker_enable_map_voxel_stats(vors_tracker* t) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxel_stats: the handle t is NULL");
    if (t->seq->map.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxel_stats: legal only before vors_tracker_enable_map_normals (keyframe 0 is emitted again)");
    vors_status st = trackers_map_voxel_stats_enable(t->seq, t->has_last, "the first vors_tracker_track");
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    // vors_tracker_enable_map_voxels has emitted keyframe 0 without statistics: the map is emptied and keyframe 0 emitted again, counted
    return trackers_map_init(t->seq, nullptr, t->s_main);  // (no normals yet: see the refusal above)
}

// The clipped count of the single sequence's list (synchronises).
static vors_status tracker_map_clipped_count(vors_tracker* t, uint32_t* np) {
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, t->seq->map.counts, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    *np = std::min<uint32_t>(total, (uint32_t)t->seq->map.capacity);
    return VORS_OK;
}

vors_status vors_tracker_read_map_voxel_stats(vors_tracker* t, int capacity, int64_t* sums, uint32_t* obs) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_voxel_stats: the handle t is NULL");
    const vors_trackers::Map::Voxels& v = t->seq->map.voxels;
    if (!v.stats)
        return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_voxel_stats: the voxel statistics are not enabled (vors_tracker_enable_map_voxel_stats)");
    if (capacity < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_voxel_stats: negative capacity");
    DeviceGuard guard(t->device);
    uint32_t clipped = 0;
    vors_status st = tracker_map_clipped_count(t, &clipped);
    if (st != VORS_OK) return st;
    const size_t np = std::min<size_t>(clipped, (size_t)capacity);
    if (sums && np) HIP_TRY(hipMemcpyAsync(sums, v.sums, np * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, t->s_main));
    if (obs && np) HIP_TRY(hipMemcpyAsync(obs, v.obs, np * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    return VORS_OK;
}

// Host buffers, like its siblings, and no device buffer of its own: the statistics, the list and the segment records are read back and
// resolved by vors_voxel_means_host — lie.h voxel_mean, the text the device pass runs, so the bits are those of
// vors_trackers_map_voxel_means; the first segment of a rank is the same search over the records.
vors_status vors_tracker_map_voxel_means(vors_tracker* t, uint32_t min_count, uint32_t min_span, int capacity, float* xyz_mean, uint8_t* gray_mean,
                                         uint32_t* kept) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: the handle t is NULL");
    const vors_trackers::Map& m = t->seq->map;
    if (!m.voxels.stats)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: the voxel statistics are not enabled (vors_tracker_enable_map_voxel_stats)");
    if (capacity < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: negative capacity");
    if (!xyz_mean && !gray_mean && !kept)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: no output at all (xyz_mean, gray_mean and kept are NULL)");
    DeviceGuard guard(t->device);
    uint32_t np = 0, n_seg = 0;
    vors_status st = tracker_map_clipped_count(t, &np);
    if (st != VORS_OK) return st;
    HIP_TRY(hipMemcpyAsync(&n_seg, m.n_segments, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    n_seg = std::min<uint32_t>(n_seg, (uint32_t)m.max_keyframes);
    std::vector<float> xyz((size_t)np * 3), mean((size_t)np * 3);
    std::vector<int64_t> sums((size_t)np * 4);
    std::vector<uint32_t> obs((size_t)np * 2), first_segment(np);
    std::vector<uint8_t> gray(np);
    std::vector<vors_map_segment> seg(n_seg);
    if (np) {
        HIP_TRY(hipMemcpyAsync(xyz.data(), m.xyz, xyz.size() * sizeof(float), hipMemcpyDeviceToHost, t->s_main));
        HIP_TRY(hipMemcpyAsync(sums.data(), m.voxels.sums, sums.size() * sizeof(int64_t), hipMemcpyDeviceToHost, t->s_main));
        HIP_TRY(hipMemcpyAsync(obs.data(), m.voxels.obs, obs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    }
    if (n_seg) HIP_TRY(hipMemcpyAsync(seg.data(), m.segments, seg.size() * sizeof(vors_map_segment), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    for (uint32_t r = 0, j = 0; r < np; ++r) {  // (the last record whose first is <= r; ranks ascend, so j only moves on)
        while (j + 1 < n_seg && seg[j + 1].first <= r) ++j;
        first_segment[r] = j;
    }
    uint32_t k = 0;
    if (np) {
        st = vors_voxel_means_host(xyz.data(), np, (int)np, sums.data(), obs.data(), m.voxels.voxel_m, min_count, min_span, first_segment.data(),
                                   mean.data(), gray.data(), &k);
        if (st != VORS_OK) return st;
    }
    const size_t no = std::min<size_t>(np, (size_t)capacity);
    if (xyz_mean && no) std::memcpy(xyz_mean, mean.data(), no * 3 * sizeof(float));
    if (gray_mean && no) std::memcpy(gray_mean, gray.data(), no);
    if (kept) *kept = k;
    return VORS_OK;
}

vors_status vors_tracker_read_map(vors_tracker* t, int capacity, float* xyz, uint32_t* pixel, uint8_t* gray, uint32_t* count, int max_segments,
                                  vors_map_segment* segments, uint32_t* n_segments) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map: the handle t is NULL");
    const vors_trackers::Map& m = t->seq->map;
    if (!m.on) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map: the keyframe map is not enabled (vors_tracker_enable_map)");
    if (capacity < 0 || max_segments < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map: negative capacity / max_segments");
    DeviceGuard guard(t->device);
    uint32_t totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&totals[0], m.counts, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipMemcpyAsync(&totals[1], m.n_segments, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    const size_t np = std::min<size_t>(std::min<uint32_t>(totals[0], (uint32_t)m.capacity), (size_t)capacity);
    const size_t ns = std::min<size_t>(std::min<uint32_t>(totals[1], (uint32_t)m.max_keyframes), (size_t)max_segments);
    if (xyz && np) HIP_TRY(hipMemcpyAsync(xyz, m.xyz, np * 3 * sizeof(float), hipMemcpyDeviceToHost, t->s_main));
    if (pixel && np) HIP_TRY(hipMemcpyAsync(pixel, m.pixel, np * sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    if (gray && np) HIP_TRY(hipMemcpyAsync(gray, m.gray, np, hipMemcpyDeviceToHost, t->s_main));
    if (segments && ns) HIP_TRY(hipMemcpyAsync(segments, m.segments, ns * sizeof(vors_map_segment), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    if (count) *count = totals[0];
    if (n_segments) *n_segments = totals[1];
    return VORS_OK;
}

vors_status vors_trackers_render_map(vors_trackers* t, int level, const void* d_poses7, size_t pose_stride_bytes, const void* d_ranges,
                                     size_t range_stride_bytes, int footprint, uint64_t* d_zkey, uint16_t* d_depth, uint8_t* d_gray,
                                     uint32_t* d_counts, void* hip_stream) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "render_map: the handle t is NULL");
    if (!t->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, "render_map: the keyframe map is not enabled (vors_trackers_enable_map)");
    if (!t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "render_map: called before vors_trackers_init (there is no map and no pose yet)");
    vors_batch* b = t->batch;
    if (level < 0 || level >= b->g.L) return fail(VORS_ERR_INVALID_ARGUMENT, "render_map: level out of range");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    vors_status st = check_stream(b, s);
    if (st != VORS_OK) return st;
    const LevelGeom& lv = b->g.lv[level];
    const float cam5[5] = {lv.k.cu, lv.k.cv, lv.k.fu, lv.k.fv, lv.k.skew};
    // NULL poses: the current frame poses, which the track call has already moved forward in stream order
    if (!d_poses7) pose_stride_bytes = 0;
    return vors_render_points(t->n_seq, t->map.xyz, t->map.gray, t->map.counts, t->map.capacity, d_ranges, range_stride_bytes, cam5, lv.rows,
                              lv.cols, b->g.depth_scale, d_poses7 ? d_poses7 : t->cur_poses.p, pose_stride_bytes, footprint, d_zkey, d_depth,
                              d_gray, d_counts, s);
}

// What the icp_map entries check of the handle before they forward (the stream is checked under the forward's DeviceGuard)
static vors_status icp_map_refusals(const vors_trackers* t) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "icp_map: the handle t is NULL");
    if (!t->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, "icp_map: the keyframe map is not enabled (vors_trackers_enable_map)");
    if (!t->map.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "icp_map: the normals of the map are not enabled (vors_trackers_enable_map_normals)");
    if (!t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "icp_map: called before vors_trackers_init (there is no map and no pose yet)");
    return VORS_OK;
}

// The forward of the three entries below: the handle's own refusals, then icp_points_device (operators.cpp) on the handle's lists with
// its level-0 intrinsics, refusing in the name of `who`, the handle-free entry of the form. robust / joint: as IcpArgs takes them; the
// joint part's list grey is the map's, filled here.
static vors_status trackers_icp_map(const char* who, vors_trackers* t, const uint16_t* d_depth, float dist_m, float damping, float step_eps,
                                    int iters, int min_points, const void* d_ranges, size_t range_stride_bytes, const void* d_poses7_in,
                                    size_t pose_stride_bytes, void* d_workspace, float* d_poses7_out, vors_icp_stats* d_stats, float* d_sums29,
                                    float* d_residuals, const IcpRobust* robust, IcpJoint* joint, void* hip_stream) {
    vors_status st = icp_map_refusals(t);
    if (st != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(t->batch->device);
    if ((st = check_stream(t->batch, s)) != VORS_OK) return st;
    IcpArgs a{};
    IcpCall& c = a.call = map_icp_call(t, d_depth);
    const float cam5[5] = {c.k.cu, c.k.cv, c.k.fu, c.k.fv, c.k.skew};
    a.cam5 = cam5;
    c.ranges = static_cast<const uint8_t*>(d_ranges); a.range_stride_bytes = range_stride_bytes;
    // NULL poses: the current frame poses, which the track call has already moved forward in stream order; the pass only reads them
    c.poses_in = d_poses7_in ? static_cast<const float*>(d_poses7_in) : t->cur_poses.as<float>();
    a.pose_stride_bytes = d_poses7_in ? pose_stride_bytes : 0;
    c.dist_m = dist_m; c.damping = damping; c.step_eps = step_eps; c.iters = iters; a.min_points = min_points;
    a.workspace = d_workspace; c.poses_out = d_poses7_out; c.stats = d_stats; c.sums29 = d_sums29; c.residuals = d_residuals;
    if (joint) joint->list_gray = t->map.gray;
    a.robust = robust; a.joint = joint;
    return icp_points_device(who, a, s);
}

vors_status vors_trackers_icp_map(vors_trackers* t, const uint16_t* d_depth, float dist_m, float damping, float step_eps, int iters, int min_points,
                                  const void* d_ranges, size_t range_stride_bytes, const void* d_poses7_in, size_t pose_stride_bytes,
                                  void* d_workspace, float* d_poses7_out, vors_icp_stats* d_stats, float* d_sums29, float* d_residuals,
                                  void* hip_stream) {
    return trackers_icp_map("icp_points", t, d_depth, dist_m, damping, step_eps, iters, min_points, d_ranges, range_stride_bytes, d_poses7_in,
                            pose_stride_bytes, d_workspace, d_poses7_out, d_stats, d_sums29, d_residuals, nullptr, nullptr, hip_stream);
}

vors_status vors_trackers_icp_map_robust(vors_trackers* t, const uint16_t* d_depth, float dist_m, float damping, float step_eps, int iters,
                                         int min_points, const void* d_ranges, size_t range_stride_bytes, const void* d_poses7_in,
                                         size_t pose_stride_bytes, const float* d_frame_normals, float min_cos, float huber_m, void* d_workspace,
                                         float* d_poses7_out, vors_icp_stats* d_stats, float* d_sums29, float* d_residuals,
                                         uint32_t* d_gate_counts, void* hip_stream) {
    const IcpRobust robust{d_frame_normals, min_cos, huber_m, d_gate_counts};
    return trackers_icp_map("icp_points_robust", t, d_depth, dist_m, damping, step_eps, iters, min_points, d_ranges, range_stride_bytes, d_poses7_in,
                            pose_stride_bytes, d_workspace, d_poses7_out, d_stats, d_sums29, d_residuals, &robust, nullptr, hip_stream);
}

vors_status vors_trackers_icp_map_joint(vors_trackers* t, const uint16_t* d_depth, const uint8_t* d_frame_gray, float dist_m, float damping,
                                        float step_eps, int iters, int min_points, const void* d_ranges, size_t range_stride_bytes,
                                        const void* d_poses7_in, size_t pose_stride_bytes, const float* d_frame_normals, float min_cos,
                                        float huber_m, float photo_scale_m, float photo_huber_grey, void* d_workspace, float* d_poses7_out,
                                        vors_icp_stats* d_stats, float* d_sums29, float* d_residuals, uint32_t* d_gate_counts,
                                        float* d_photo_residuals, uint32_t* d_photo_counts, void* hip_stream) {
    const IcpRobust robust{d_frame_normals, min_cos, huber_m, d_gate_counts};
    IcpJoint joint{nullptr, d_frame_gray, photo_scale_m, photo_huber_grey, d_photo_residuals, d_photo_counts};
    return trackers_icp_map("icp_points_joint", t, d_depth, dist_m, damping, step_eps, iters, min_points, d_ranges, range_stride_bytes, d_poses7_in,
                            pose_stride_bytes, d_workspace, d_poses7_out, d_stats, d_sums29, d_residuals, &robust, &joint, hip_stream);
}

vors_status vors_tracker_render_map(vors_tracker* t, int level, const float pose7[7], const uint32_t range2[2], int footprint, uint64_t* zkey,
                                    uint16_t* depth, uint8_t* gray, uint32_t* counts) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "render_map: the handle t is NULL");
    if (!t->seq->map.on) return fail(VORS_ERR_INVALID_ARGUMENT, "render_map: the keyframe map is not enabled (vors_tracker_enable_map)");
    const Geom& g = t->seq->batch->g;
    if (level < 0 || level >= g.L) return fail(VORS_ERR_INVALID_ARGUMENT, "render_map: level out of range");
    DeviceGuard guard(t->device);
    const size_t S = (size_t)t->rows * t->cols, plane = (size_t)g.lv[level].rows * g.lv[level].cols;
    struct Args {  // layout of render_args
        float pose[7];
        uint32_t range[2];
        uint32_t counts[VORS_RENDER_COUNTS];
    };
    if (!t->render_args.p) {  // (the last of the four: a call that failed half way allocates the missing ones, DevBuf keeps what exists)
        if (!t->render_zkey.p) HIP_TRY(t->render_zkey.alloc(S * sizeof(uint64_t)));
        if (!t->render_depth.p) HIP_TRY(t->render_depth.alloc(S * sizeof(uint16_t)));
        if (!t->render_gray.p) HIP_TRY(t->render_gray.alloc(S));
        HIP_TRY(t->render_args.alloc(64));
    }
    static_assert(sizeof(Args) <= 64, "render_args holds one Args");
    Args h{};
    if (pose7) std::memcpy(h.pose, pose7, sizeof(h.pose));
    if (range2) std::memcpy(h.range, range2, sizeof(h.range));
    Args* d = t->render_args.as<Args>();
    HIP_TRY(hipMemcpyAsync(d, &h, sizeof(Args), hipMemcpyHostToDevice, t->s_main));
    vors_status st = vors_trackers_render_map(t->seq, level, pose7 ? d->pose : nullptr, 0, range2 ? d->range : nullptr, 0, footprint,
                                              t->render_zkey.as<uint64_t>(), t->render_depth.as<uint16_t>(), t->render_gray.as<uint8_t>(),
                                              d->counts, t->s_main);
    if (st != VORS_OK) {
        (void)hipStreamSynchronize(t->s_main);  // (h leaves scope)
        return st;
    }
    if (zkey) HIP_TRY(hipMemcpyAsync(zkey, t->render_zkey.p, plane * sizeof(uint64_t), hipMemcpyDeviceToHost, t->s_main));
    if (depth) HIP_TRY(hipMemcpyAsync(depth, t->render_depth.p, plane * sizeof(uint16_t), hipMemcpyDeviceToHost, t->s_main));
    if (gray) HIP_TRY(hipMemcpyAsync(gray, t->render_gray.p, plane, hipMemcpyDeviceToHost, t->s_main));
    if (counts) HIP_TRY(hipMemcpyAsync(counts, d->counts, sizeof(h.counts), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    return VORS_OK;
}

vors_status vors_trackers_enable_depth_filter(vors_trackers* t, float tol_m, int max_weight, int fill_min_weight) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: the handle t is NULL");
    if (t->initialised)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: legal only before vors_trackers_init (the weights would have no history)");
    return trackers_filter_enable(t, tol_m, max_weight, fill_min_weight);
}

vors_status vors_trackers_keyframe_depth(const vors_trackers* t, const uint16_t** d_depth, const uint8_t** d_weight) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "keyframe_depth: the handle t is NULL");
    if (!t->filter.on) return fail(VORS_ERR_INVALID_ARGUMENT, "keyframe_depth: the depth filter is not enabled (vors_trackers_enable_depth_filter)");
    if (d_depth) *d_depth = t->keyframe_depth();
    if (d_weight) *d_weight = t->filter.weight;
    return VORS_OK;
}

vors_status vors_trackers_workspace_bytes(const vors_trackers* t, uint64_t* bytes) {
    if (!t || !bytes) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    return vors_batch_workspace_bytes(t->batch, bytes);
}

vors_status vors_tracker_enable_depth_filter(vors_tracker* t, float tol_m, int max_weight, int fill_min_weight) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: the handle t is NULL");
    if (t->has_last) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_depth_filter: legal only before the first vors_tracker_track");
    vors_status st = trackers_filter_enable(t->seq, tol_m, max_weight, fill_min_weight);
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    // t->depth still holds the first frame's depth map (create ordered its upload before everything on s_main); the next upload
    // waits for ev_frame_done, which therefore moves behind this reader
    if ((st = trackers_filter_init(t->seq, t->depth.as<uint16_t>(), t->s_main)) != VORS_OK) return st;
    HIP_TRY(hipEventRecord(t->ev_frame_done, t->s_main));
    return VORS_OK;
}

vors_status vors_trackers_create(const vors_config* cfg, int n_sequences, int rows, int cols, vors_trackers** out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = 0;
    }
    return vors_trackers_create_on(dev, cfg, n_sequences, rows, cols, out);
}

vors_status vors_trackers_create_on(int device, const vors_config* cfg, int n_sequences, int rows, int cols, vors_trackers** out) {
    if (!out) return fail(VORS_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    vors_batch* b = nullptr;
    vors_status st = vors_batch_create_on(device, cfg, n_sequences, rows, cols, &b);
    if (st != VORS_OK) return st;
    DeviceGuard on_device(device);  // the state buffers live on the handle's device
    vors_trackers* t = new vors_trackers();
    t->batch = b;
    t->n_seq = n_sequences;
    std::unique_ptr<vors_trackers> guard(t);
    const size_t n = (size_t)n_sequences, S = (size_t)rows * cols;
    HIP_TRY(t->cur_poses.alloc(n * 7 * sizeof(float)));
    HIP_TRY(t->kf_poses.alloc(n * 7 * sizeof(float)));
    HIP_TRY(t->out_poses.alloc(n * 7 * sizeof(float)));
    HIP_TRY(t->status.alloc(n * sizeof(int32_t)));
    HIP_TRY(t->stats.alloc(n * sizeof(vors_pair_stats)));
    HIP_TRY(t->kf_frame.alloc(n * sizeof(int32_t)));
    HIP_TRY(t->promo_list.alloc(n * sizeof(int)));
    HIP_TRY(t->promo_count.alloc(sizeof(int)));
    HIP_TRY(t->frame_counter.alloc(sizeof(int)));
    if (b->g.mode == VORS_CANDIDATES_DENSE) {
        HIP_TRY(t->own_gray.alloc(n * S));
        HIP_TRY(t->own_depth.alloc(n * S * 2));
    }
    *out = guard.release();
    return VORS_OK;
}

void vors_trackers_destroy(vors_trackers* t) {
    if (!t) return;
    DeviceGuard guard(t->batch ? t->batch->device : 0);
    delete t;
}

int vors_trackers_count(const vors_trackers* t) { return t ? t->n_seq : 0; }

vors_status vors_trackers_init(vors_trackers* t, const uint8_t* d_gray, const uint16_t* d_depth, void* hip_stream) {
    if (!t || !d_gray || !d_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    vors_batch* b = t->batch;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    vors_status st = check_stream(b, s);
    if (st != VORS_OK) return st;
    const size_t n = (size_t)t->n_seq, S = (size_t)b->g.S0;
    const uint8_t* kf_gray = d_gray;
    const uint16_t* kf_depth = d_depth;
    if (b->g.mode == VORS_CANDIDATES_DENSE) {  // the handle's own copies (zero copy is impossible: keyframes outlive the caller's frames)
        HIP_TRY(hipMemcpyAsync(t->own_gray.p, d_gray, n * S, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(t->own_depth.p, d_depth, n * S * 2, hipMemcpyDeviceToDevice, s));
        kf_gray = t->own_gray.as<uint8_t>();
        kf_depth = t->own_depth.as<uint16_t>();
    }
    st = vors_batch_prepare_keyframes(b, t->n_seq, kf_gray, kf_depth, s);
    if (st != VORS_OK) return st;
    if (b->g.mode != VORS_CANDIDATES_DENSE) {
        // Sparse modes: everything later stages need is in the records; the caller may reuse or free its frames, and keyframe promotion
        // (trackers_promote) rebuilds the records from later frames. The handle must not keep pointers into frames it does not own:
        // the keyframe-inspection entry points (vors_batch_get_keyframe_image / get_points) are not available on a trackers-owned batch.
        b->kf_level0 = nullptr;
        b->kf_depth = nullptr;
    }
    // first frame: keyframe_pose = current_frame_pose = identity (inverse_compositional.rs:86-99)
    launch_identity_poses(t->cur_poses.as<float>(), t->kf_poses.as<float>(), t->n_seq, s);  // (on the device: init only enqueues work, like track)
    HIP_TRY(hipMemsetAsync(t->kf_frame.p, 0, n * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(t->status.p, 0, n * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(t->frame_counter.p, 0, sizeof(int), s));
    HIP_TRY(hipGetLastError());
    if (t->filter.on && (st = trackers_filter_init(t, d_depth, s)) != VORS_OK) return st;
    if (t->map.on && (st = trackers_map_init(t, kf_depth, s)) != VORS_OK) return st;
    if (t->map.icp.on && (st = trackers_map_icp_init(t, s)) != VORS_OK) return st;  // (the stage itself is not run: the map was empty)
    if (t->map.icp.means && (st = trackers_map_icp_means_init(t, s)) != VORS_OK) return st;
    t->frame_index = 0;
    t->initialised = true;
    return VORS_OK;
}

vors_status vors_trackers_track(vors_trackers* t, const uint8_t* d_gray, const uint16_t* d_depth, void* hip_stream) {
    if (!d_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    vors_status st = trackers_track_lm(t, d_gray, s);
    return st != VORS_OK ? st : trackers_promote(t, d_gray, d_depth, nullptr, s);
}

vors_status vors_trackers_state(const vors_trackers* t, const float** d_current_poses7, const float** d_keyframe_poses7,
                                const int32_t** d_status, const int32_t** d_keyframe_index, const vors_pair_stats** d_stats) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL handle");
    if (d_current_poses7) *d_current_poses7 = static_cast<const float*>(t->cur_poses.p);
    if (d_keyframe_poses7) *d_keyframe_poses7 = static_cast<const float*>(t->kf_poses.p);
    if (d_status) *d_status = static_cast<const int32_t*>(t->status.p);
    if (d_keyframe_index) *d_keyframe_index = static_cast<const int32_t*>(t->kf_frame.p);
    if (d_stats) *d_stats = static_cast<const vors_pair_stats*>(t->stats.p);
    return VORS_OK;
}

vors_status vors_trackers_current_frames(vors_trackers* t, float* poses7, int32_t* status, int32_t* keyframe_index, void* hip_stream) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL handle");
    if (!t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "vors_trackers_current_frames called before vors_trackers_init");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(t->batch->device);
    const size_t n = (size_t)t->n_seq;
    if (poses7) HIP_TRY(hipMemcpyAsync(poses7, t->cur_poses.p, n * 7 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(hipMemcpyAsync(status, t->status.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (keyframe_index) HIP_TRY(hipMemcpyAsync(keyframe_index, t->kf_frame.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VORS_OK;
}

vors_status vors_trackers_last_stats(vors_trackers* t, vors_pair_stats* stats, void* hip_stream) {
    if (!t || !stats) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t->frame_index < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "no frame has been tracked yet");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(t->batch->device);
    HIP_TRY(hipMemcpyAsync(stats, t->stats.p, (size_t)t->n_seq * sizeof(vors_pair_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VORS_OK;
}

vors_status vors_trackers_enable_kernel_timing(vors_trackers* t, int ring) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL handle");
    return vors_batch_enable_kernel_timing(t->batch, ring);
}
vors_status vors_trackers_kernel_times(vors_trackers* t, int stage, float* ms_out, int capacity, int* n_out) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL handle");
    return vors_batch_kernel_times(t->batch, stage, ms_out, capacity, n_out);
}

vors_status vors_tracker_create(const vors_config* cfg, double depth_time, const uint16_t* depth, double img_time,
                                const uint8_t* gray, int rows, int cols, int layout, vors_tracker** out) {
    if (!out) return fail(VORS_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!depth || !gray) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL image pointer");
    if (layout != VORS_ROW_MAJOR && layout != VORS_COL_MAJOR) return fail(VORS_ERR_INVALID_ARGUMENT, "bad layout");
    vors_trackers* seq = nullptr;
    vors_status st = vors_trackers_create(cfg, 1, rows, cols, &seq);
    if (st != VORS_OK) return st;
    vors_tracker* t = new vors_tracker();
    t->seq = seq;
    t->cfg = *cfg;
    t->rows = rows;
    t->cols = cols;
    t->layout = layout;
    std::unique_ptr<vors_tracker> guard(t);
    if (hipGetDevice(&t->device) != hipSuccess) t->device = 0;  // the tracker lives on the device that is current at creation
    const size_t S = (size_t)rows * cols;
    HIP_TRY(t->gray.alloc(S));
    HIP_TRY(t->depth.alloc(S * 2));
    if (layout == VORS_COL_MAJOR) {
        HIP_TRY(t->tmp8.alloc(S));
        HIP_TRY(t->tmp16.alloc(S * 2));
    }
    HIP_TRY(t->h_gray.alloc(S));
    HIP_TRY(t->h_depth.alloc(S * 2));
    HIP_TRY(t->h_out.alloc(sizeof(TrackerOut)));
    HIP_TRY(hipStreamCreateWithFlags(&t->s_main, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&t->s_copy, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_depth, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_frame_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_result, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(t->ev_frame_done, t->s_main));
    if ((st = tracker_upload(t, gray, depth)) != VORS_OK) return st;
    HIP_TRY(hipStreamWaitEvent(t->s_main, t->ev_depth, 0));
    st = vors_trackers_init(t->seq, t->gray.as<uint8_t>(), t->depth.as<uint16_t>(), t->s_main);  // (synchronises s_main)
    if (st != VORS_OK) return st;
    HIP_TRY(hipEventRecord(t->ev_frame_done, t->s_main));
    t->keyframe_depth_timestamp = depth_time;
    t->keyframe_img_timestamp = img_time;
    t->current_frame_depth_timestamp = depth_time;
    t->current_frame_img_timestamp = img_time;
    *out = guard.release();
    return VORS_OK;
}

vors_status vors_tracker_track(vors_tracker* t, double depth_time, const uint16_t* depth, double img_time, const uint8_t* gray,
                               int* track_status) {
    if (!t || !depth || !gray) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard guard(t->device);
    // Tracker::track (inverse_compositional.rs:170-240) incl. the keyframe switch, all on the device. Order on the host: grey image up,
    // pyramid + LM + keyframe test enqueued, THEN the depth map staged and sent on the copy stream (under the LM stage), then the
    // promotion, which waits for it.
    // ... and the host returns as soon as the RESULTS are back (a packed record the device stores into pinned host memory), while the
    // promotion of a switching frame still runs: the next call is ordered behind it on the stream.
    const float* d_pose = nullptr;
    const int32_t *d_status = nullptr, *d_kf = nullptr;
    const vors_pair_stats* d_stats = nullptr;
    (void)vors_trackers_state(t->seq, &d_pose, nullptr, &d_status, &d_kf, &d_stats);
    TrackerOut* o = t->h_out.as<TrackerOut>();
    vors_status st = VORS_OK;
    // (A HIP graph of this per-frame sequence — it has no per-frame argument any more: the frame index lives on the device — was built and
    // measured in round 4: 0.172 vs 0.174 ms per frame. The launches are enqueued ahead of the device anyway; what the frame waits for is
    // the LM kernel's chain of ~35 dependent evaluations. Not kept.)
    if ((st = tracker_upload_gray(t, gray)) != VORS_OK) return st;
    if ((st = trackers_track_lm(t->seq, t->gray.as<uint8_t>(), t->s_main)) != VORS_OK) return st;
    // With the map ICP correction the promotion may still move the pose: the results are then packed BEHIND it, and the frame waits for
    // its promotion. Without it nothing changes: packed here, read back under the promotion.
    const bool corrected = t->seq->map.icp.on;
    if (!corrected) {
        launch_tracker_pack_out(d_pose, d_status, d_kf, d_stats, o, t->s_main);
        HIP_TRY(hipGetLastError());  // (a failed launch is reported against THIS frame, not against whatever touches the stream next)
        HIP_TRY(hipEventRecord(t->ev_result, t->s_main));
    }
    if ((st = tracker_upload_depth(t, depth)) != VORS_OK) return st;
    if ((st = trackers_promote(t->seq, t->gray.as<uint8_t>(), t->depth.as<uint16_t>(), t->ev_depth, t->s_main)) != VORS_OK) return st;
    if (corrected) {
        launch_tracker_pack_out(d_pose, d_status, d_kf, d_stats, o, t->s_main);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(t->ev_result, t->s_main));
    }
    HIP_TRY(hipEventRecord(t->ev_frame_done, t->s_main));
    HIP_TRY(hipEventSynchronize(t->ev_result));
    t->last = o->stats;
    t->has_last = true;
    // inverse_compositional.rs:203-208
    t->current_frame_depth_timestamp = depth_time;
    t->current_frame_img_timestamp = img_time;
    t->current_frame_pose = iso_load(o->pose);  // == previous pose when the optimizer failed
    // inverse_compositional.rs:224-239 (the device has already promoted the frame)
    if (t->last.change_keyframe) {
        t->keyframe_depth_timestamp = depth_time;
        t->keyframe_img_timestamp = img_time;
        t->keyframe_pose = t->current_frame_pose;
    }
    if (track_status) *track_status = o->status;
    return VORS_OK;
}

vors_status vors_tracker_track_checked(vors_tracker* t, double depth_time, const uint16_t* depth, double img_time, const uint8_t* gray,
                                       int rows, int cols, int* track_status) {
    if (!t) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rows != t->rows || cols != t->cols)
        return fail(VORS_ERR_INVALID_ARGUMENT, "frame is " + std::to_string(rows) + " x " + std::to_string(cols) + " but the tracker was created for " +
                                                   std::to_string(t->rows) + " x " + std::to_string(t->cols));
    return vors_tracker_track(t, depth_time, depth, img_time, gray, track_status);
}

vors_status vors_tracker_current_frame(const vors_tracker* t, double* timestamp, float pose7[7]) {
    if (!t || !timestamp || !pose7) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    *timestamp = t->current_frame_depth_timestamp;  // the DEPTH timestamp: inverse_compositional.rs:243-247
    iso_store(t->current_frame_pose, pose7);
    return VORS_OK;
}
vors_status vors_tracker_keyframe(const vors_tracker* t, double* timestamp, float pose7[7]) {
    if (!t || !timestamp || !pose7) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    *timestamp = t->keyframe_depth_timestamp;
    iso_store(t->keyframe_pose, pose7);
    return VORS_OK;
}
vors_status vors_tracker_last_stats(const vors_tracker* t, vors_pair_stats* stats) {
    if (!t || !stats) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!t->has_last) return fail(VORS_ERR_INVALID_ARGUMENT, "no frame has been tracked yet");
    *stats = t->last;
    return VORS_OK;
}
void vors_tracker_destroy(vors_tracker* t) {
    if (!t) return;
    DeviceGuard guard(t->device);  // the buffers are freed on the device they live on
    if (t->s_main) (void)hipStreamSynchronize(t->s_main);
    if (t->s_copy) (void)hipStreamSynchronize(t->s_copy);
    delete t;
}

}  // extern "C"
