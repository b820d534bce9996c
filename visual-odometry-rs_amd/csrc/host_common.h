// What the host sources of libvors_hip.so share (batch.cpp, trackers.cpp, trackers_map.cpp, pipeline.cpp, operators.cpp): error plumbing, device and buffer
// guards, and the batch handle every other handle is built on. None of them contains a kernel; no CPU compute path exists here: every
// compute entry point needs a HIP device and fails loudly (VORS_ERR_NO_DEVICE) without one.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "engine.h"

// ---------------------------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------------------------
vors_status vors_set_last_error(vors_status st, const std::string& msg);  // operators.cpp (also used by multi.cpp)
inline vors_status fail(vors_status st, const std::string& msg) { return vors_set_last_error(st, msg); }
#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t _e = (expr);                                                                                \
        if (_e != hipSuccess)                                                                                  \
            return fail(VORS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                      \
    } while (0)

inline vors_status require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(VORS_ERR_NO_DEVICE, "vors_hip: no HIP device available (this library has no CPU fallback)");
    }
    return VORS_OK;
}

// Record strides arrive in bytes; 0 asks for the packed record. The sentence is one, the upper limits are two: the batch products stop at
// 1 MiB, the handle-free operators at what fits an int. They differ by history; making them one would change what is accepted.
constexpr size_t BATCH_STRIDE_LIMIT = 1u << 20;
constexpr size_t OPERATOR_STRIDE_LIMIT = 0x7fffffffu;
inline vors_status stride_refusal(const char* who, const char* arg, size_t bytes, size_t min_bytes, size_t limit) {
    if (bytes == 0 || (bytes % 4 == 0 && bytes >= min_bytes && bytes <= limit)) return VORS_OK;
    return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": " + arg + " must be 0 or a multiple of 4 of at least " + std::to_string(min_bytes));
}
inline int stride_words(size_t bytes, int packed_words) { return bytes ? (int)(bytes / 4) : packed_words; }

// cam5 of the C ABI: cu cv fu fv skew
inline vors::Intr intr_from_cam5(const float cam5[5]) { return vors::Intr{cam5[0], cam5[1], cam5[2], cam5[3], cam5[4]}; }

// Entry points run on the handle's device whatever the caller's current device is, and restore the caller's on exit.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) ok = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Short-lived and per-tracker buffers.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    template <class T>
    T* as() { return static_cast<T*>(p); }
};
struct PinnedBuf {
    void* p = nullptr;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault); }
    template <class T>
    T* as() { return static_cast<T*>(p); }
};

// ---------------------------------------------------------------------------------------------------------------
// device-resident batch engine
// ---------------------------------------------------------------------------------------------------------------
// Owner of what a batch handle creates on its device: one hipMalloc per buffer (the caller-visible pointers keep their own alignment,
// `bytes` is what vors_batch_workspace_bytes reports), streams and events. The first error sticks and turns the later calls into no-ops,
// so the creation code is straight-line statements followed by ONE check of `err`; the destructor releases whatever was created. A new
// workspace buffer is one alloc() line and nothing else.
struct DeviceResources {
    std::vector<void*> buffers;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    uint64_t bytes = 0;
    hipError_t err = hipSuccess;
    DeviceResources() = default;
    DeviceResources(const DeviceResources&) = delete;
    DeviceResources& operator=(const DeviceResources&) = delete;
    ~DeviceResources() {
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (void* p : buffers) (void)hipFree(p);
    }
    template <class T>
    void alloc(T** p, size_t n) {
        if (err != hipSuccess) return;
        if ((err = hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T))) != hipSuccess) return;
        buffers.push_back(*p);
        bytes += n * sizeof(T);
    }
    void stream(hipStream_t* s, unsigned flags) {
        if (err == hipSuccess && (err = hipStreamCreateWithFlags(s, flags)) == hipSuccess) streams.push_back(*s);
    }
    void event(hipEvent_t* e, unsigned flags) {
        if (err == hipSuccess && (err = hipEventCreateWithFlags(e, flags)) == hipSuccess) events.push_back(*e);
    }
};

// Per-stage HIP-event ring (stage: 0 keyframe pyramid, 1 keyframe precompute, 2 current pyramid, 3 LM kernel).
// Events are only RECORDED on the caller's stream during a step (non-blocking); elapsed times are read afterwards.
// A step that ran as two halves (HalvesPlan below) has a second interval per stage, the second half's on its own stream (evb0 / evb1, created
// with the others; `two` marks the ring entries that hold one): vors_batch_kernel_times adds the two intervals of a pre-LM stage and takes
// the LM stage from the first start of either half to the last end.
struct StageTimers {
    int ring = 0;
    std::vector<hipEvent_t> ev0[4], ev1[4], evb0[4], evb1[4];
    std::vector<char> two[4];
    long count[4] = {0, 0, 0, 0};
    StageTimers() = default;
    StageTimers(const StageTimers&) = delete;
    StageTimers& operator=(const StageTimers&) = delete;
    ~StageTimers() { clear(); }
    void clear() {  // ring -> 0: no stage is timed
        ring = 0;
        for (int st = 0; st < 4; ++st) {
            two[st].clear();
            for (auto* ring_events : {&ev0[st], &ev1[st], &evb0[st], &evb1[st]}) {
                for (hipEvent_t e : *ring_events)
                    if (e) (void)hipEventDestroy(e);
                ring_events->clear();
            }
            count[st] = 0;
        }
    }
};
#define STAGE_BEGIN(b, st, s) \
    do {                      \
        if ((b)->timers.ring > 0) HIP_TRY(hipEventRecord((b)->timers.ev0[st][(b)->timers.count[st] % (b)->timers.ring], s)); \
    } while (0)
#define STAGE_END(b, st, s)   \
    do {                      \
        if ((b)->timers.ring > 0) {  \
            HIP_TRY(hipEventRecord((b)->timers.ev1[st][(b)->timers.count[st] % (b)->timers.ring], s)); \
            (b)->timers.two[st][(b)->timers.count[st] % (b)->timers.ring] = 0; \
            (b)->timers.count[st] += 1; \
        }                     \
    } while (0)

// One dense vors_batch_track_pairs call as two slices of pairs, [0, h) on the caller's stream and [h, n_pairs) on `stream`, so that each
// slice's dependent tails (round boundaries, late rounds, stragglers, epilogue) are filled by the other slice; as measured, the two slices'
// pre-LM stages run side by side from the fork on and the two LM stages side by side after them (batch.cpp plan_halves, track_pairs_halves). Per-pair buffers are shared: a slice addresses them through
// pointers advanced by h pairs. What an LM stage shares through the handle exists once per slice: `split` (state, partials, lists,
// counters, side lane with its stream and events; pred_log points into the first slice's) and the REFERENCE hand-over counters.
struct HalvesPlan {
    bool present = false;
    int from = 0;         // calls of at least this many pairs take the plan
    int align = 1;        // h is a multiple of this many pairs: a slice's level-0 buffers then keep the 16-byte alignment of the caller's
    int cap = 0;          // most pairs of the second slice
    vors::LmSplitWs split{};
    int* handoff_counters = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

struct vors_batch {
    vors_config cfg;
    vors::Geom g;
    int max_pairs = 0;
    int device = 0;          // HIP device the workspaces live on (vors_batch_create_on); every entry point switches to it
    int prepared_pairs = 0;  // n_pairs of the last prepare_keyframes: track_current may not ask for more
    int current_pairs = 0;   // n_pairs of the last track_current: the current-frame pyramid slots that hold an image
    uint8_t* kf_upper = nullptr;
    uint8_t* cur_upper = nullptr;
    const uint8_t* kf_level0 = nullptr;   // caller's buffer of the last prepare_keyframes
    const uint8_t* cur_level0 = nullptr;  // caller's buffer of the last track_current
    const uint16_t* kf_depth = nullptr;   // caller's depth buffer of the last prepare_keyframes (read by the dense LM kernel)
    vors::Records rec{};
    vors::LmSplitWs split{};
    HalvesPlan halves;  // large dense handles: one track_pairs call as two overlapped slices (off: halves.present == false)
    vors::EvalPairsWs eval_pairs{};  // vors_batch_eval_pairs / _pose_information: allocated by the first of those calls (items = 0 until then)
    uint32_t* cloud_counts = nullptr;  // vors_batch_point_cloud: [max_pairs][cloud_chunks] kept points per chunk, allocated by its first call
    int cloud_chunks = 0;
    int lm_block = 256;  // threads per frame pair in the LM kernel (256 / 512 / 1024)
    vors::RefDevice ref_device;  // REFERENCE arithmetic: what the device offers the workgroup-per-pair kernel
    // generic-mask (DSO) mode workspaces
    vors::DsoWs dso{};
    vors::PixelPlanes pp{};
    uint8_t* mask0 = nullptr;
    StageTimers timers;
    DeviceResources own;  // every device pointer, stream and event above that the handle created (destroy on the handle's device)
};

// Allocations from the handle's resources failed (own.err): what was created stays with them and is freed with the handle, the error is
// cleared so that the handle stays usable, and whatever asked (a switch, a product's workspace) stays off. `what`: the noun of the message.
inline vors_status own_alloc_failed(vors_batch* b, const char* what) {
    const hipError_t e = b->own.err;
    b->own.err = hipSuccess;
    (void)hipGetLastError();
    return fail(VORS_ERR_HIP, std::string("hipMalloc (") + what + "): " + hipGetErrorString(e));
}

// The map ICP correction's parameters (operators.cpp, beside the ICP's own refusals): every refusal of vors_map_icp_params, in the name
// of `who`, and the verdict's thresholds as lie.h map_icp_verdict reads them (the cosine of half max_rot_rad is taken here, once).
extern "C" {
vors_status map_icp_params_refusals(const char* who, const vors_map_icp_params* params);
vors::MapIcpGates map_icp_gates(const vors_map_icp_params& params);
// ... and of vors_map_icp_joint_params: the above of its `icp`, what vors_icp_points_joint refuses of the two photo fields, the two
// dilution bounds; photo_huber_m = photo_scale_m * photo_huber_grey as vors_icp_points_joint takes it (once, on the host).
vors_status map_icp_joint_params_refusals(const char* who, const vors_map_icp_joint_params* params);
float map_icp_photo_huber_m(const vors_map_icp_joint_params& params);
// One ICP pass as a C entry states it, before anything is judged (operators.cpp): `call` holds the lists, planes, scalars and outputs as
// given, and what IcpCall keeps in other units or derives stands beside it — the pass fills call.k, range_stride, pose_stride,
// min_points and the workspace's three pointers from these after the refusals. robust NULL: the plain pass; joint (needs robust): its
// photo_huber_m still holds photo_huber_grey, scaled once by the pass.
struct IcpArgs {
    vors::IcpCall call;
    const float* cam5;
    int min_points;
    size_t range_stride_bytes, pose_stride_bytes;
    void* workspace;
    const vors::IcpRobust* robust;
    const vors::IcpJoint* joint;
};
// The device pass of vors_icp_points, _robust and _joint, and of their forwards on the sequence handle: every refusal in the name of
// `who`, then launch_icp_points on s. Internal: hidden, so that the library's dynamic symbols stay the ones it had.
__attribute__((visibility("hidden"))) vors_status icp_points_device(const char* who, const IcpArgs& args, hipStream_t s);
// The device pass of vors_repose_points and of its forward on the sequence handle (operators.cpp): every refusal in the name of `who` —
// call.pose_stride is set from pose_stride_bytes here —, then launch_repose_points on s. Hidden likewise.
__attribute__((visibility("hidden"))) vors_status repose_points_device(const char* who, vors::ReposeCall call, size_t pose_stride_bytes, hipStream_t s);
}
// vors_batch_create_on with one more decision: allow_halves = false keeps the handle on the plain path whatever its size (HalvesPlan is
// then never created). A vors_pipeline slot is created so: its steps already overlap with its neighbours', on the ring's own streams.
// Internal: hidden, so that the library's dynamic symbols stay the ones it had.
extern "C" __attribute__((visibility("hidden"))) vors_status batch_create_on(int device, const vors_config* cfg, int max_pairs, int rows, int cols,
                                                                           bool allow_halves, vors_batch** out);
// The stream work is enqueued on must belong to the handle's device (a stream of another device would silently run nothing useful).
vors_status check_stream(const vors_batch* b, hipStream_t s);
// Tracker::track up to the keyframe test for the prepared keyframes of `b`, with the keyframe poses on the device (batch.cpp;
// vors_batch_track_current is the kf_poses7 = NULL case)
vors_status batch_track_current(vors_batch* b, int n_pairs, const uint8_t* d_cur_gray, const float* d_prev_poses7, const float* d_kf_poses7,
                                float* d_out_poses7, int32_t* d_out_status, vors_pair_stats* d_out_stats, hipStream_t s);
