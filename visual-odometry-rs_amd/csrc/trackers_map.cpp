// The keyframe map of the sequence handles (vors_trackers::Map, trackers.h): emission, normals, voxels and their statistics, the ICP
// correction at promotion, and every entry that switches them on, shows, reads back, renders or aligns them — for the lock-step handle
// (vors_trackers_*) and for the single Tracker on top of it (vors_tracker_*). The state machine that calls in here is trackers.cpp.
#include <algorithm>
#include <cstring>
#include <initializer_list>

#include "trackers.h"

using namespace vors;
using Map = vors_trackers::Map;

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
    const Map::Voxels& v = t->map.voxels;
    if (v.on) call.voxels = PointCloudVoxelArgs{v.voxel_m, (uint32_t)v.table_slots, v.table, v.occupied, v.overflow};
    // ... and so are the statistics: WRITE stores rank_of, ACCUMULATE behind it reads rank_of and the list entries WRITE (of this or an
    // earlier emission) stored, and touches sums / obs with integer atomics only; later emissions read and extend rank_of. Besides
    // ACCUMULATE only init's clear writes sums / obs.
    if (v.stats) call.voxel_stats = PointCloudVoxelStatsArgs{v.rank_of, v.sums, v.obs};
    launch_lm_point_cloud_append(gm, call, s);
}

// What both normals passes of the map state alike, the one over an emission's entries and the ICP stage's frame normals: the [n_seq][S0]
// planes `depth` with the level-0 camera and shape (map normals exist for a level-0 map only), the map normals' step and jump, the
// selection of gm. Poses, outputs and list arguments are the caller's.
static NormalCall map_normal_call(const vors_trackers* t, const Geom& gm, const uint16_t* depth) {
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
    call.sel_list = gm.sel_list;
    call.sel_count = gm.sel_count;
    return call;
}

// The normals of the entries an emission appended (vors_trackers_enable_map_normals): the list form of the normals pass over the ranks
// [first[seq], min(counts[seq], capacity)) of the selected sequences (gm.sel_list; null: all), keyed on the stored pixels, in `depth`, the
// [n_seq][S0] planes the keyframe stage of this call ran on. Hazards: it reads map.pixel / map.counts behind the emission that wrote them
// and the keyframe pose behind launch_trackers_advance; `depth` is the handle's own plane or the caller's frame, which this call may read
// in work it enqueues; it writes map.normals.n, which nothing else touches.
static void trackers_map_normals_pass(vors_trackers* t, const Geom& gm, const uint16_t* depth, hipStream_t s) {
    NormalCall call = map_normal_call(t, gm, depth);
    call.poses = t->kf_poses.as<float>();
    call.pose_stride = 7;
    call.normals = t->map.normals.n;
    call.pixel = t->map.pixel;
    call.list_counts = t->map.counts;
    call.capacity = t->map.capacity;
    call.first = t->map.normals.first;
    launch_points_normals(call, s);
}
// The emission with what surrounds it when the map carries normals: the running totals are copied first, the normals pass follows.
// `depth` is read only then.
void trackers_map_emit_all(vors_trackers* t, const Geom& gm, const uint16_t* depth, hipStream_t s) {
    const Map::Normals& nm = t->map.normals;
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
void trackers_map_icp_stage(vors_trackers* t, const Geom& gm, const uint16_t* depth, const uint8_t* gray, hipStream_t s) {
    const Map& m = t->map;
    const Map::Icp& ic = m.icp;
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
        NormalCall nc = map_normal_call(t, gm, depth);
        nc.normals = ic.frame_normals;
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
    Map::Voxels& v = t->map.voxels;
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
    Map::Voxels& v = t->map.voxels;
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
    Map::Normals& nm = t->map.normals;
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
    Map::Icp& ic = t->map.icp;
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
        ic = Map::Icp{};
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
vors_status trackers_map_icp_init(vors_trackers* t, hipStream_t s) {
    const size_t n = (size_t)t->n_seq;
    HIP_TRY(hipMemsetAsync(t->map.icp.records, 0, n * sizeof(vors_map_icp_record), s));
    HIP_TRY(hipMemsetAsync(t->map.icp.totals, 0, n * 2 * sizeof(uint32_t), s));
    if (t->map.icp.joint) HIP_TRY(hipMemsetAsync(t->map.icp.joint_records, 0, n * sizeof(vors_map_icp_joint_record), s));
    return VORS_OK;
}
// The switch of the correction's averaged model: every refusal, then every buffer at once. `started` / `before`: as for the voxel filter.
static vors_status trackers_map_icp_means_enable(vors_trackers* t, bool started, const char* before, uint32_t min_count, uint32_t min_span) {
    Map::Icp& ic = t->map.icp;
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
vors_status trackers_map_icp_means_init(vors_trackers* t, hipStream_t s) {
    const Map::Icp& ic = t->map.icp;
    const size_t n = (size_t)t->n_seq, cap = (size_t)t->map.capacity;
    HIP_TRY(hipMemsetAsync(ic.mean_xyz, 0, n * cap * 3 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(ic.mean_gray, 0, n * cap, s));
    HIP_TRY(hipMemsetAsync(ic.means_records, 0, n * sizeof(vors_map_icp_means_record), s));
    return VORS_OK;
}
// An empty map (and an empty voxel table), then keyframe 0 of every sequence. `depth`: the planes keyframe 0 was made from, read only
// when the map carries normals.
vors_status trackers_map_init(vors_trackers* t, const uint16_t* depth, hipStream_t s) {
    const size_t n = (size_t)t->n_seq;
    HIP_TRY(hipMemsetAsync(t->map.counts, 0, n * sizeof(uint32_t), s));
    HIP_TRY(hipMemsetAsync(t->map.n_segments, 0, n * sizeof(uint32_t), s));
    if (const Map::Voxels& v = t->map.voxels; v.on) {
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

// ---------------------------------------------------------------------------------------------------------------
// What the entries below repeat, stated once
// ---------------------------------------------------------------------------------------------------------------
// An option of the map as an entry that reads it names it when it is off: "<is> not enabled (<the handle's prefix><enable>)".
struct Option {
    bool (*on)(const Map&);
    const char *is, *enable;
};
static const Option MAP{[](const Map& m) { return m.on; }, "the keyframe map is", "enable_map"};
static const Option NORMALS{[](const Map& m) { return m.normals.on; }, "the normals of the map are", "enable_map_normals"};
static const Option ICP{[](const Map& m) { return m.icp.on; }, "the ICP correction is", "enable_map_icp"};
static const Option ICP_JOINT{[](const Map& m) { return m.icp.joint; }, "the joint ICP correction is", "enable_map_icp_joint"};
static const Option ICP_MEANS{[](const Map& m) { return m.icp.means; }, "the averaged model is", "enable_map_icp_means"};
static const Option VOXELS{[](const Map& m) { return m.voxels.on; }, "the voxel filter of the map is", "enable_map_voxels"};
static const Option VOXEL_STATS{[](const Map& m) { return m.voxels.stats; }, "the voxel statistics are", "enable_map_voxel_stats"};

// The refusals an entry opens with, in its name `who`: the handle is NULL (m: its map, or NULL); the option the entry reads is off
// (o; NULL: the entry reads none). A lock-step handle points at vors_trackers_enable_*, a single Tracker at vors_tracker_enable_*.
static vors_status entry_guard(const char* who, const Map* m, const char* prefix, const Option* o) {
    if (!m) return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": the handle t is NULL");
    if (o && !o->on(*m)) return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": " + o->is + " not enabled (" + prefix + o->enable + ")");
    return VORS_OK;
}
static vors_status entry_guard(const char* who, const vors_trackers* t, const Option* o = nullptr) {
    return entry_guard(who, t ? &t->map : nullptr, "vors_trackers_", o);
}
static vors_status entry_guard(const char* who, const vors_tracker* t, const Option* o = nullptr) {
    return entry_guard(who, t ? &t->seq->map : nullptr, "vors_tracker_", o);
}

// An option's switch on the single Tracker: the shared enable — started = a frame has been tracked — and, once it holds, what the option
// owes keyframe 0, which exists since create, on s_main under the Tracker's device. enable(seq, started, before), then(seq, s_main).
template <class Enable, class Then>
static vors_status tracker_enable(vors_tracker* t, Enable enable, Then then) {
    vors_status st = enable(t->seq, t->has_last, "the first vors_tracker_track");
    if (st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    return then(t->seq, t->s_main);
}
// ... for the options that change what an emission stores: the map emptied and keyframe 0 emitted (again), without normals — every caller
// comes before vors_tracker_enable_map_normals.
static vors_status tracker_map_emit_keyframe0(vors_trackers* q, hipStream_t s) { return trackers_map_init(q, nullptr, s); }

// The clipped count of the single sequence's list (synchronises). totals2 (nullable): the running totals themselves, kept points and
// keyframes, read in the same trip.
static vors_status tracker_map_clipped_count(vors_tracker* t, uint32_t* np, uint32_t* totals2 = nullptr) {
    const Map& m = t->seq->map;
    uint32_t total = 0;
    uint32_t* count = totals2 ? &totals2[0] : &total;
    HIP_TRY(hipMemcpyAsync(count, m.counts, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    if (totals2) HIP_TRY(hipMemcpyAsync(&totals2[1], m.n_segments, sizeof(uint32_t), hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    *np = std::min<uint32_t>(*count, (uint32_t)m.capacity);
    return VORS_OK;
}
// A single Tracker's read-back: every span with a host pointer and bytes to copy, device -> host on s_main in the order given, then ONE
// synchronisation. `bytes` is the whole span's (entries read x bytes per entry; a record's size).
struct Span {
    const void* device;
    void* host;
    size_t bytes;
};
static vors_status tracker_read_spans(vors_tracker* t, std::initializer_list<Span> spans) {
    for (const Span& sp : spans)
        if (sp.host && sp.bytes) HIP_TRY(hipMemcpyAsync(sp.host, sp.device, sp.bytes, hipMemcpyDeviceToHost, t->s_main));
    HIP_TRY(hipStreamSynchronize(t->s_main));
    return VORS_OK;
}

extern "C" {

vors_status vors_trackers_enable_map(vors_trackers* t, int level, int capacity, int max_keyframes, int min_weight) {
    if (vors_status st = entry_guard("enable_map", t); st != VORS_OK) return st;
    if (t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: legal only before vors_trackers_init (keyframe 0 would be missing)");
    return trackers_map_enable(t, level, capacity, max_keyframes, min_weight);
}

vors_status vors_trackers_map(const vors_trackers* t, const float** d_xyz, const uint32_t** d_pixel, const uint8_t** d_gray,
                              const uint32_t** d_counts, const vors_map_segment** d_segments, const uint32_t** d_n_segments) {
    if (vors_status st = entry_guard("map", t, &MAP); st != VORS_OK) return st;
    if (d_xyz) *d_xyz = t->map.xyz;
    if (d_pixel) *d_pixel = t->map.pixel;
    if (d_gray) *d_gray = t->map.gray;
    if (d_counts) *d_counts = t->map.counts;
    if (d_segments) *d_segments = t->map.segments;
    if (d_n_segments) *d_n_segments = t->map.n_segments;
    return VORS_OK;
}

vors_status vors_tracker_enable_map(vors_tracker* t, int level, int capacity, int max_keyframes, int min_weight) {
    if (vors_status st = entry_guard("enable_map", t); st != VORS_OK) return st;
    if (t->has_last) return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map: legal only before the first vors_tracker_track");
    // keyframe 0 exists since create: its records, the handle's copies (dense mode) and the identity pose are what init left on s_main
    return tracker_enable(
        t, [&](vors_trackers* q, bool, const char*) { return trackers_map_enable(q, level, capacity, max_keyframes, min_weight); },
        tracker_map_emit_keyframe0);  // (no normals yet: they are enabled after the map)
}

vors_status vors_trackers_enable_map_normals(vors_trackers* t, int step, float jump_m) {
    if (vors_status st = entry_guard("enable_map_normals", t); st != VORS_OK) return st;
    return trackers_map_normals_enable(t, t->initialised, "vors_trackers_init (keyframe 0 would have no normals)", step, jump_m);
}

vors_status vors_trackers_map_normals(const vors_trackers* t, const float** d_normals) {
    if (vors_status st = entry_guard("map_normals", t, &NORMALS); st != VORS_OK) return st;
    if (d_normals) *d_normals = t->map.normals.n;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_normals(vors_tracker* t, int step, float jump_m) {
    if (vors_status st = entry_guard("enable_map_normals", t); st != VORS_OK) return st;
    return tracker_enable(
        t, [&](vors_trackers* q, bool started, const char* before) { return trackers_map_normals_enable(q, started, before, step, jump_m); },
        [&](vors_trackers* q, hipStream_t s) -> vors_status {
            // Keyframe 0 is in the map already: its normals are the pass over every rank so far, in the plane keyframe 0 was made from — the
            // handle's copy (dense mode), the filter's copy, or t->depth, which still holds the first frame's depth map (the next upload waits
            // for ev_frame_done, which therefore moves behind this reader, as in vors_tracker_enable_depth_filter)
            const uint16_t* depth = (q->batch->g.mode == VORS_CANDIDATES_DENSE || q->filter.on) ? q->keyframe_depth() : t->depth.as<uint16_t>();
            HIP_TRY(hipMemsetAsync(q->map.normals.first, 0, sizeof(uint32_t), s));
            trackers_map_normals_pass(q, q->batch->g, depth, s);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(t->ev_frame_done, s));
            return VORS_OK;
        });
}

vors_status vors_tracker_read_map_normals(vors_tracker* t, int capacity, float* normals) {
    if (vors_status st = entry_guard("read_map_normals", t, &NORMALS); st != VORS_OK) return st;
    if (capacity < 0 || !normals) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_normals: negative capacity or NULL normals");
    DeviceGuard guard(t->device);
    uint32_t clipped = 0;
    if (vors_status st = tracker_map_clipped_count(t, &clipped); st != VORS_OK) return st;
    const size_t np = std::min<size_t>(clipped, (size_t)capacity);
    return tracker_read_spans(t, {{t->seq->map.normals.n, normals, np * 3 * sizeof(float)}});
}

vors_status vors_trackers_enable_map_icp(vors_trackers* t, const vors_map_icp_params* params) {
    if (vors_status st = entry_guard("enable_map_icp", t); st != VORS_OK) return st;
    return trackers_map_icp_enable(t, t->initialised, "vors_trackers_init", params);
}

vors_status vors_trackers_map_icp(const vors_trackers* t, const vors_map_icp_record** d_records, const uint32_t** d_totals) {
    if (vors_status st = entry_guard("map_icp", t, &ICP); st != VORS_OK) return st;
    if (d_records) *d_records = t->map.icp.records;
    if (d_totals) *d_totals = t->map.icp.totals;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_icp(vors_tracker* t, const vors_map_icp_params* params) {
    if (vors_status st = entry_guard("enable_map_icp", t); st != VORS_OK) return st;
    return tracker_enable(
        t, [&](vors_trackers* q, bool started, const char* before) { return trackers_map_icp_enable(q, started, before, params); },
        trackers_map_icp_init);
}

vors_status vors_tracker_read_map_icp(vors_tracker* t, vors_map_icp_record* record, uint32_t totals[2]) {
    if (vors_status st = entry_guard("read_map_icp", t, &ICP); st != VORS_OK) return st;
    const Map::Icp& ic = t->seq->map.icp;
    DeviceGuard guard(t->device);
    return tracker_read_spans(t, {{ic.records, record, sizeof(vors_map_icp_record)}, {ic.totals, totals, 2 * sizeof(uint32_t)}});
}

vors_status vors_trackers_enable_map_icp_joint(vors_trackers* t, const vors_map_icp_joint_params* params) {
    if (vors_status st = entry_guard("enable_map_icp_joint", t); st != VORS_OK) return st;
    return trackers_map_icp_enable(t, t->initialised, "vors_trackers_init", nullptr, params, true);
}

vors_status vors_trackers_map_icp_joint(const vors_trackers* t, const vors_map_icp_joint_record** d_joint_records) {
    if (vors_status st = entry_guard("map_icp_joint", t, &ICP_JOINT); st != VORS_OK) return st;
    if (d_joint_records) *d_joint_records = t->map.icp.joint_records;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_icp_joint(vors_tracker* t, const vors_map_icp_joint_params* params) {
    if (vors_status st = entry_guard("enable_map_icp_joint", t); st != VORS_OK) return st;
    return tracker_enable(
        t, [&](vors_trackers* q, bool started, const char* before) { return trackers_map_icp_enable(q, started, before, nullptr, params, true); },
        trackers_map_icp_init);
}

vors_status vors_tracker_read_map_icp_joint(vors_tracker* t, vors_map_icp_joint_record* record) {
    if (vors_status st = entry_guard("read_map_icp_joint", t, &ICP_JOINT); st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    return tracker_read_spans(t, {{t->seq->map.icp.joint_records, record, sizeof(vors_map_icp_joint_record)}});
}

vors_status vors_trackers_enable_map_icp_means(vors_trackers* t, uint32_t min_count, uint32_t min_span) {
    if (vors_status st = entry_guard("enable_map_icp_means", t); st != VORS_OK) return st;
    return trackers_map_icp_means_enable(t, t->initialised, "vors_trackers_init", min_count, min_span);
}

vors_status vors_trackers_map_icp_means(const vors_trackers* t, const float** d_xyz_mean, const uint8_t** d_gray_mean,
                                        const vors_map_icp_means_record** d_records) {
    if (vors_status st = entry_guard("map_icp_means", t, &ICP_MEANS); st != VORS_OK) return st;
    if (d_xyz_mean) *d_xyz_mean = t->map.icp.mean_xyz;
    if (d_gray_mean) *d_gray_mean = t->map.icp.mean_gray;
    if (d_records) *d_records = t->map.icp.means_records;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_icp_means(vors_tracker* t, uint32_t min_count, uint32_t min_span) {
    if (vors_status st = entry_guard("enable_map_icp_means", t); st != VORS_OK) return st;
    return tracker_enable(
        t, [&](vors_trackers* q, bool started, const char* before) { return trackers_map_icp_means_enable(q, started, before, min_count, min_span); },
        trackers_map_icp_means_init);
}

vors_status vors_tracker_read_map_icp_means(vors_tracker* t, vors_map_icp_means_record* record) {
    if (vors_status st = entry_guard("read_map_icp_means", t, &ICP_MEANS); st != VORS_OK) return st;
    DeviceGuard guard(t->device);
    return tracker_read_spans(t, {{t->seq->map.icp.means_records, record, sizeof(vors_map_icp_means_record)}});
}

vors_status vors_trackers_enable_map_voxels(vors_trackers* t, float voxel_m, int table_slots) {
    if (vors_status st = entry_guard("enable_map_voxels", t); st != VORS_OK) return st;
    return trackers_map_voxels_enable(t, t->initialised, "vors_trackers_init (keyframe 0 would be unfiltered)", voxel_m, table_slots);
}

vors_status vors_trackers_map_voxels(const vors_trackers* t, const uint32_t** d_occupied, const uint32_t** d_overflow) {
    if (vors_status st = entry_guard("map_voxels", t, &VOXELS); st != VORS_OK) return st;
    if (d_occupied) *d_occupied = t->map.voxels.occupied;
    if (d_overflow) *d_overflow = t->map.voxels.overflow;
    return VORS_OK;
}

vors_status vors_tracker_enable_map_voxels(vors_tracker* t, float voxel_m, int table_slots) {
    if (vors_status st = entry_guard("enable_map_voxels", t); st != VORS_OK) return st;
    if (t->seq->map.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxels: legal only before vors_tracker_enable_map_normals (keyframe 0 is emitted again)");
    // vors_tracker_enable_map has emitted keyframe 0 unfiltered: the map is emptied and keyframe 0 emitted again, through the filter
    return tracker_enable(
        t, [&](vors_trackers* q, bool started, const char* before) { return trackers_map_voxels_enable(q, started, before, voxel_m, table_slots); },
        tracker_map_emit_keyframe0);  // (no normals yet: see the refusal above)
}

vors_status vors_tracker_read_map_voxels(vors_tracker* t, uint32_t* occupied, uint32_t* overflow) {
    if (vors_status st = entry_guard("read_map_voxels", t, &VOXELS); st != VORS_OK) return st;
    const Map::Voxels& v = t->seq->map.voxels;
    DeviceGuard guard(t->device);
    uint32_t words[2] = {0, 0};
    if (vors_status st = tracker_read_spans(t, {{v.occupied, &words[0], sizeof(uint32_t)}, {v.overflow, &words[1], sizeof(uint32_t)}}); st != VORS_OK)
        return st;
    if (occupied) *occupied = words[0];
    if (overflow) *overflow = words[1];
    return VORS_OK;
}

vors_status vors_trackers_enable_map_voxel_stats(vors_trackers* t) {
    if (vors_status st = entry_guard("enable_map_voxel_stats", t); st != VORS_OK) return st;
    return trackers_map_voxel_stats_enable(t, t->initialised, "vors_trackers_init (keyframe 0 would not be counted)");
}

vors_status vors_trackers_map_voxel_stats(const vors_trackers* t, const int64_t** d_sums, const uint32_t** d_obs) {
    if (vors_status st = entry_guard("map_voxel_stats", t, &VOXEL_STATS); st != VORS_OK) return st;
    if (d_sums) *d_sums = reinterpret_cast<const int64_t*>(t->map.voxels.sums);
    if (d_obs) *d_obs = t->map.voxels.obs;
    return VORS_OK;
}

vors_status vors_trackers_map_voxel_means(vors_trackers* t, uint32_t min_count, uint32_t min_span, float* d_xyz_mean, uint8_t* d_gray_mean,
                                          uint32_t* d_kept, void* hip_stream) {
    if (vors_status st = entry_guard("map_voxel_means", t, &VOXEL_STATS); st != VORS_OK) return st;
    const Map& m = t->map;
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

vors_status vors_trackers_repose_map(vors_trackers* t, const void* d_poses7_new, size_t pose_stride_bytes, int node_capacity,
                                     const uint32_t* d_node_counts, const uint32_t* d_node_of_segment, float* d_xyz_out, float* d_normals_out,
                                     vors_map_segment* d_segments_out, uint32_t* d_counts_out, void* hip_stream) {
    if (vors_status st = entry_guard("repose_map", t, &MAP); st != VORS_OK) return st;
    const Map& m = t->map;
    if (!t->initialised) return fail(VORS_ERR_INVALID_ARGUMENT, "repose_map: called before vors_trackers_init (there is no map yet)");
    if (d_xyz_out == m.xyz || (d_normals_out && d_normals_out == m.normals.n) || d_segments_out == m.segments)
        return fail(VORS_ERR_INVALID_ARGUMENT, "repose_map: an output is the handle's own array (the handle's map stays as tracking left it)");
    vors_batch* b = t->batch;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if (vors_status st = check_stream(b, s); st != VORS_OK) return st;
    // the handle's own lists, normals (when enabled), counters and segments are the inputs: read only, the caller's arrays are written
    const ReposeCall call{t->n_seq, m.xyz, m.normals.on ? m.normals.n : nullptr, m.counts, m.capacity, m.segments, m.n_segments, m.max_keyframes,
                          static_cast<const float*>(d_poses7_new), 7, node_capacity, d_node_counts, d_node_of_segment, d_xyz_out, d_normals_out,
                          d_segments_out, d_counts_out};
    return repose_points_device("repose_map", call, pose_stride_bytes, s);
}

vors_status vors_tracker_enable_map_voxel_stats(vors_tracker* t) {
    if (vors_status st = entry_guard("enable_map_voxel_stats", t); st != VORS_OK) return st;
    if (t->seq->map.normals.on)
        return fail(VORS_ERR_INVALID_ARGUMENT, "enable_map_voxel_stats: legal only before vors_tracker_enable_map_normals (keyframe 0 is emitted again)");
    // vors_tracker_enable_map_voxels has emitted keyframe 0 without statistics: the map is emptied and keyframe 0 emitted again, counted
    return tracker_enable(t, trackers_map_voxel_stats_enable, tracker_map_emit_keyframe0);  // (no normals yet: see the refusal above)
}

vors_status vors_tracker_read_map_voxel_stats(vors_tracker* t, int capacity, int64_t* sums, uint32_t* obs) {
    if (vors_status st = entry_guard("read_map_voxel_stats", t, &VOXEL_STATS); st != VORS_OK) return st;
    const Map::Voxels& v = t->seq->map.voxels;
    if (capacity < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map_voxel_stats: negative capacity");
    DeviceGuard guard(t->device);
    uint32_t clipped = 0;
    if (vors_status st = tracker_map_clipped_count(t, &clipped); st != VORS_OK) return st;
    const size_t np = std::min<size_t>(clipped, (size_t)capacity);
    return tracker_read_spans(t, {{v.sums, sums, np * 4 * sizeof(int64_t)}, {v.obs, obs, np * 2 * sizeof(uint32_t)}});
}

// Host buffers, like its siblings, and no device buffer of its own: the statistics, the list and the segment records are read back and
// resolved by vors_voxel_means_host — lie.h voxel_mean, the text the device pass runs, so the bits are those of
// vors_trackers_map_voxel_means; the first segment of a rank is the same search over the records.
vors_status vors_tracker_map_voxel_means(vors_tracker* t, uint32_t min_count, uint32_t min_span, int capacity, float* xyz_mean, uint8_t* gray_mean,
                                         uint32_t* kept) {
    if (vors_status st = entry_guard("map_voxel_means", t, &VOXEL_STATS); st != VORS_OK) return st;
    const Map& m = t->seq->map;
    if (capacity < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: negative capacity");
    if (!xyz_mean && !gray_mean && !kept)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_voxel_means: no output at all (xyz_mean, gray_mean and kept are NULL)");
    DeviceGuard guard(t->device);
    uint32_t np = 0, n_seg = 0;
    vors_status st = tracker_map_clipped_count(t, &np);
    if (st != VORS_OK) return st;
    if ((st = tracker_read_spans(t, {{m.n_segments, &n_seg, sizeof(uint32_t)}})) != VORS_OK) return st;
    n_seg = std::min<uint32_t>(n_seg, (uint32_t)m.max_keyframes);
    std::vector<float> xyz((size_t)np * 3), mean((size_t)np * 3);
    std::vector<int64_t> sums((size_t)np * 4);
    std::vector<uint32_t> obs((size_t)np * 2), first_segment(np);
    std::vector<uint8_t> gray(np);
    std::vector<vors_map_segment> seg(n_seg);
    st = tracker_read_spans(t, {{m.xyz, xyz.data(), xyz.size() * sizeof(float)}, {m.voxels.sums, sums.data(), sums.size() * sizeof(int64_t)},
                                {m.voxels.obs, obs.data(), obs.size() * sizeof(uint32_t)}, {m.segments, seg.data(), seg.size() * sizeof(vors_map_segment)}});
    if (st != VORS_OK) return st;
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
    if (vors_status st = entry_guard("read_map", t, &MAP); st != VORS_OK) return st;
    const Map& m = t->seq->map;
    if (capacity < 0 || max_segments < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "read_map: negative capacity / max_segments");
    DeviceGuard guard(t->device);
    uint32_t totals[2] = {0, 0}, clipped = 0;
    vors_status st = tracker_map_clipped_count(t, &clipped, totals);
    if (st != VORS_OK) return st;
    const size_t np = std::min<size_t>(clipped, (size_t)capacity);
    const size_t ns = std::min<size_t>(std::min<uint32_t>(totals[1], (uint32_t)m.max_keyframes), (size_t)max_segments);
    st = tracker_read_spans(t, {{m.xyz, xyz, np * 3 * sizeof(float)}, {m.pixel, pixel, np * sizeof(uint32_t)}, {m.gray, gray, np},
                                {m.segments, segments, ns * sizeof(vors_map_segment)}});
    if (st != VORS_OK) return st;
    if (count) *count = totals[0];
    if (n_segments) *n_segments = totals[1];
    return VORS_OK;
}

vors_status vors_trackers_render_map(vors_trackers* t, int level, const void* d_poses7, size_t pose_stride_bytes, const void* d_ranges,
                                     size_t range_stride_bytes, int footprint, uint64_t* d_zkey, uint16_t* d_depth, uint8_t* d_gray,
                                     uint32_t* d_counts, void* hip_stream) {
    if (vors_status st = entry_guard("render_map", t, &MAP); st != VORS_OK) return st;
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
    if (vors_status st = entry_guard("icp_map", t, &MAP); st != VORS_OK) return st;
    if (vors_status st = entry_guard("icp_map", t, &NORMALS); st != VORS_OK) return st;
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
    if (vors_status st = entry_guard("render_map", t, &MAP); st != VORS_OK) return st;
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
    return tracker_read_spans(t, {{t->render_zkey.p, zkey, plane * sizeof(uint64_t)}, {t->render_depth.p, depth, plane * sizeof(uint16_t)},
                                  {t->render_gray.p, gray, plane}, {d->counts, counts, sizeof(h.counts)}});
}

}  // extern "C"
