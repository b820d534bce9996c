// Sequences: N of them in lock-step on the device (vors_trackers_*), and the single Tracker of the reference as their N = 1 case
// (vors_tracker_*). Both sit on a batch handle (host_common.h, batch.cpp). The handles themselves are in trackers.h; this unit holds the
// lock-step state machine, the depth filter and the single Tracker's frame loop, and trackers_map.cpp everything of the keyframe map.
#include <algorithm>
#include <cstring>
#include <memory>

#include "trackers.h"

using namespace vors;

// (trackers.h)
LmScene keyframe_scene(vors_trackers* t) {
    const vors_batch* b = t->batch;
    const bool dense = b->g.mode == VORS_CANDIDATES_DENSE;
    return LmScene{Pyramid{nullptr, nullptr}, Pyramid{dense ? t->own_gray.as<uint8_t>() : nullptr, b->kf_upper},
                   dense ? t->own_depth.as<uint16_t>() : nullptr, b->rec};
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
// Tracker: one sequence (Config::init / Tracker::track / Tracker::current_frame; vors_tracker, trackers.h)
// ---------------------------------------------------------------------------------------------------------------
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

extern "C" {

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
