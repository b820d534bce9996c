// Everything of the C ABI that is not a handle: last error, device queries and self-checks, the LM operators on explicit observations
// (vors_lm_*), Lie helpers and the synthetic scenes.
#include <algorithm>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "host_common.h"

using namespace vors;

static thread_local std::string g_last_error;
vors_status vors_set_last_error(vors_status st, const std::string& msg) {
    g_last_error = msg;
    return st;
}

// ---------------------------------------------------------------------------------------------------------------
// operator level
// ---------------------------------------------------------------------------------------------------------------
struct ObsDev {
    DevBuf tmpl, img, xy, iz, jac, A, B, C, XY, IZ, model, out, res;
    Records rec{};
    Intr k;
};
static vors_status upload_obs(const vors_obs* o, const float model7[7], ObsDev& d, bool want_res, hipStream_t s) {
    if (!o || !model7) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (o->rows < 2 || o->cols < 2 || o->n < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "bad observation shape");
    if (o->arithmetic != VORS_ARITH_EXACT && o->arithmetic != VORS_ARITH_REFERENCE)
        return fail(VORS_ERR_INVALID_ARGUMENT, "vors_obs.arithmetic must be VORS_ARITH_EXACT or VORS_ARITH_REFERENCE");
    if (!o->template_ || !o->image || (o->n > 0 && (!o->coordinates || !o->_z_candidates || !o->jacobians)))
        return fail(VORS_ERR_INVALID_ARGUMENT, "NULL observation array");
    vors_status st = require_device();
    if (st != VORS_OK) return st;
    const size_t S = (size_t)o->rows * o->cols, n = (size_t)o->n;
    for (size_t i = 0; i < n; ++i) {
        const int x = o->coordinates[2 * i], y = o->coordinates[2 * i + 1];
        if (x < 0 || y < 0 || x >= o->cols || y >= o->rows) return fail(VORS_ERR_INVALID_ARGUMENT, "coordinate outside the template");
    }
    HIP_TRY(d.tmpl.alloc(S));
    HIP_TRY(d.img.alloc(S));
    HIP_TRY(d.xy.alloc(n * 8));
    HIP_TRY(d.iz.alloc(n * 4));
    HIP_TRY(d.jac.alloc(n * 24));
    HIP_TRY(d.A.alloc(n * 16));
    HIP_TRY(d.B.alloc(n * 16));
    HIP_TRY(d.C.alloc(n * 8));
    HIP_TRY(d.XY.alloc(n * 4));
    HIP_TRY(d.IZ.alloc(n * 4));
    HIP_TRY(d.model.alloc(7 * 4));
    HIP_TRY(d.out.alloc(64 * 4));
    if (want_res) HIP_TRY(d.res.alloc(n * 4));
    HIP_TRY(hipMemcpyAsync(d.tmpl.p, o->template_, S, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.img.p, o->image, S, hipMemcpyHostToDevice, s));
    if (n) {
        HIP_TRY(hipMemcpyAsync(d.xy.p, o->coordinates, n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d.iz.p, o->_z_candidates, n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d.jac.p, o->jacobians, n * 24, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(d.model.p, model7, 28, hipMemcpyHostToDevice, s));
    d.k = Intr{o->cu, o->cv, o->fu, o->fv, o->skew};
    d.rec = Records{d.A.as<float4>(), d.B.as<float4>(), d.C.as<float2>(), d.XY.as<uint32_t>(), d.IZ.as<float>(), nullptr, nullptr, nullptr};
    launch_records_from_obs(d.k, o->rows, o->cols, d.tmpl.as<uint8_t>(), o->n, d.xy.as<int32_t>(), d.iz.as<float>(),
                            d.jac.as<float>(), d.rec, s);
    return VORS_OK;
}

extern "C" {

const char* vors_last_error(void) { return g_last_error.c_str(); }
int vors_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}
int vors_abi_version(void) { return 5; }

vors_status vors_selfcheck_isqrt(int* mismatches) {
    vors_status st = require_device();
    if (st != VORS_OK) return st;
    if (!mismatches) return fail(VORS_ERR_INVALID_ARGUMENT, "mismatches is null");
    const int n = vors::count_isqrt_u16_mismatches(nullptr);
    if (n < 0) return fail(VORS_ERR_HIP, "isqrt self-check could not run");
    *mismatches = n;
    return VORS_OK;
}

vors_status vors_device_info(int device, int* clock_khz, int* compute_units, uint64_t* memory_bytes) {
    vors_status st = require_device();
    if (st != VORS_OK) return st;
    if (device < 0 || device >= vors_device_count()) return fail(VORS_ERR_INVALID_ARGUMENT, "device index out of range");
    int v = 0;
    if (clock_khz) {
        HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeClockRate, device));
        *clock_khz = v;
    }
    if (compute_units) {
        HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device));
        *compute_units = v;
    }
    if (memory_bytes) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        *memory_bytes = (uint64_t)prop.totalGlobalMem;
    }
    return VORS_OK;
}

vors_status vors_lm_eval(const vors_obs* obs, const float model7[7], float* energy, int32_t* n_inside, float g[6], float H[36],
                         float* residuals) {
    if (!energy || !n_inside || !g || !H) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL output");
    ObsDev d;
    hipStream_t s = nullptr;
    vors_status st = upload_obs(obs, model7, d, residuals != nullptr, s);
    if (st != VORS_OK) return st;
    if (obs->arithmetic == VORS_ARITH_REFERENCE)
        launch_lm_eval_obs_reference(d.k, obs->rows, obs->cols, d.img.as<uint8_t>(), obs->n, d.rec, obs->huber_delta, d.model.as<float>(),
                                     d.out.as<float>(), residuals ? d.res.as<float>() : nullptr, s);
    else
        launch_lm_eval_obs(d.k, obs->rows, obs->cols, d.img.as<uint8_t>(), obs->n, d.rec, obs->huber_delta, d.model.as<float>(),
                           d.out.as<float>(), residuals ? d.res.as<float>() : nullptr, s);
    float out[44];
    HIP_TRY(hipMemcpyAsync(out, d.out.p, sizeof(out), hipMemcpyDeviceToHost, s));
    if (residuals && obs->n) HIP_TRY(hipMemcpyAsync(residuals, d.res.p, (size_t)obs->n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    *energy = out[0];
    *n_inside = (int32_t)out[1];
    std::memcpy(g, out + 2, 24);
    std::memcpy(H, out + 8, 144);
    return VORS_OK;
}

vors_status vors_lm_solve(const vors_obs* obs, const float model7[7], float out_model7[7], int32_t* nb_iter, float* energy,
                          float* lm_coef, int* solve_status) {
    if (!out_model7 || !nb_iter || !energy || !lm_coef || !solve_status) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL output");
    ObsDev d;
    hipStream_t s = nullptr;
    vors_status st = upload_obs(obs, model7, d, false, s);
    if (st != VORS_OK) return st;
    if (obs->arithmetic == VORS_ARITH_REFERENCE)
        launch_lm_solve_obs_reference(d.k, obs->rows, obs->cols, d.img.as<uint8_t>(), obs->n, d.rec, obs->huber_delta, d.model.as<float>(),
                                      d.out.as<float>(), s);
    else
        launch_lm_solve_obs(d.k, obs->rows, obs->cols, d.img.as<uint8_t>(), obs->n, d.rec, obs->huber_delta, d.model.as<float>(),
                            d.out.as<float>(), s);
    float out[11];
    HIP_TRY(hipMemcpyAsync(out, d.out.p, sizeof(out), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipGetLastError());
    std::memcpy(out_model7, out, 28);
    *nb_iter = (int32_t)out[7];
    *energy = out[8];
    *lm_coef = out[9];
    *solve_status = out[10] != 0.f ? VORS_TRACK_OPTIMIZER_FAILED_POSE_KEPT : VORS_TRACK_OK;
    return VORS_OK;
}

vors_status vors_lm_step(const float H[36], const float g[6], const float model7[7], float lm_coef, float out_model7[7],
                         int* chol_ok) {
    if (!H || !g || !model7 || !out_model7 || !chol_ok) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    Iso out;
    const bool ok = lm_step(H, g, iso_load(model7), lm_coef, &out);
    *chol_ok = ok ? 1 : 0;
    if (ok) iso_store(out, out_model7);
    return VORS_OK;
}

vors_status vors_pose_information_from_sums(const float sums29[29], float info36[36], float cov36[36], float* sigma2, int32_t* flag) {
    if (!sums29) return fail(VORS_ERR_INVALID_ARGUMENT, "sums29 is NULL");
    const int fl = pose_information(sums29, info36, cov36, sigma2);
    if (flag) *flag = fl;
    return VORS_OK;
}

vors_status vors_residual_scale_from_hist(const uint32_t hist[VORS_RESIDUAL_BINS], float* median_abs, float* sigma_mad, uint32_t* n_inside) {
    if (!hist) return fail(VORS_ERR_INVALID_ARGUMENT, "hist is NULL");
    residual_scale_from_hist(hist, median_abs, sigma_mad, n_inside);
    return VORS_OK;
}

// The merge of vors_batch_fuse_depth for arrays: lie.h fuse_depth_pixel, the text the device kernel runs. Every key is checked before
// anything is written.
vors_status vors_fuse_depth_pixels(float depth_scale, float tol_m, int max_weight, int fill_min_weight, size_t n_pixels, const uint64_t* zkey,
                                   const uint16_t* cur_depth, const uint8_t* kf_weight, size_t n_kf_pixels, uint16_t* fused_depth,
                                   uint8_t* fused_weight, uint32_t counts[VORS_FUSE_COUNTS]) {
    if (!zkey || !cur_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth_pixels: zkey or cur_depth is NULL");
    if (!(depth_scale > 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth_pixels: depth_scale must be > 0");
    if (!(tol_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth_pixels: tol_m must be >= 0 (and not NaN)");
    if (max_weight < 1 || max_weight > 255) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth_pixels: max_weight must be in 1..255");
    if (fill_min_weight < 0 || fill_min_weight > 255) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth_pixels: fill_min_weight must be in 0..255");
    for (size_t i = 0; i < n_pixels; ++i)
        if (zkey[i] != VORS_ZKEY_EMPTY && (zkey[i] & 0xFFFFFFFFull) >= n_kf_pixels)
            return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth_pixels: a key names a source pixel beyond n_kf_pixels");
    uint32_t n[VORS_FUSE_COUNTS] = {0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n_pixels; ++i) {
        const FusedPixel o = fuse_depth_pixel(depth_scale, tol_m, max_weight, fill_min_weight, zkey[i], kf_weight, cur_depth[i]);
        if (fused_depth) fused_depth[i] = o.depth;
        if (fused_weight) fused_weight[i] = o.weight;
        n[o.kase] += 1;
    }
    if (counts)
        for (int k = 0; k < VORS_FUSE_COUNTS; ++k) counts[k] = n[k];
    return VORS_OK;
}

// The strides of the operators on point lists (vors_render_points, vors_depth_normals, vors_points_normals): one pose of 7 floats and one
// (first, count) range of 2 u32 per list. What each entry says about the alignment of its pointers stays with it.
static vors_status list_stride_refusals(const char* who, size_t pose_stride_bytes, size_t range_stride_bytes) {
    vors_status st = stride_refusal(who, "pose_stride_bytes", pose_stride_bytes, 28, OPERATOR_STRIDE_LIMIT);
    return st != VORS_OK ? st : stride_refusal(who, "range_stride_bytes", range_stride_bytes, 8, OPERATOR_STRIDE_LIMIT);
}

// ---------------------------------------------------------------------------------------------------------------
// Rendering of point lists into a camera (vors_render_points, vors_render_points_host): the refusals both share, the device entry
// (render_kernels.hip) and the host entry, which runs the kernels' own text (lie.h render_point, render_footprint, render_resolve).
// ---------------------------------------------------------------------------------------------------------------
static vors_status render_refusals(const char* who, const void* xyz, const void* list_gray, const float* cam5, int capacity, int rows, int cols,
                                   float depth_scale, int footprint, const void* zkey) {
    const std::string w(who);
    if (!xyz || !list_gray) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a list (xyz, list_gray) is NULL");
    if (!cam5) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": cam5 is NULL");
    if (!zkey) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": zkey is NULL (the pass keeps no plane of its own)");
    if ((uintptr_t)zkey % 8 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": zkey must be 8-byte aligned");
    if (footprint < 1 || footprint > 3) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": footprint must be 1, 2 or 3");
    if (rows < 1 || cols < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows and cols must be >= 1");
    if (capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": capacity must be >= 1");
    if (rows > 65535 || cols > 65535 || (long long)rows * cols > (1ll << 28))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels");
    if (!(depth_scale > 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth_scale must be > 0");
    return VORS_OK;
}

vors_status vors_render_points(int n, const float* d_xyz, const uint8_t* d_list_gray, const uint32_t* d_list_counts, int capacity,
                               const void* d_ranges, size_t range_stride_bytes, const float cam5[5], int rows, int cols, float depth_scale,
                               const void* d_poses7, size_t pose_stride_bytes, int footprint, uint64_t* d_zkey, uint16_t* d_depth,
                               uint8_t* d_gray, uint32_t* d_counts, void* hip_stream) {
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "render_points: n must be >= 1");
    if (!d_list_counts) return fail(VORS_ERR_INVALID_ARGUMENT, "render_points: a list (d_list_counts) is NULL");
    vors_status st = render_refusals("render_points", d_xyz, d_list_gray, cam5, capacity, rows, cols, depth_scale, footprint, d_zkey);
    if (st != VORS_OK) return st;
    if ((st = list_stride_refusals("render_points", pose_stride_bytes, range_stride_bytes)) != VORS_OK) return st;
    if ((uintptr_t)d_ranges % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, "render_points: d_ranges must be 4-byte aligned");
    // the kernels read floats and u32 and write u16 and u32 through these: each at its natural alignment
    if ((uintptr_t)d_xyz % 4 != 0 || (uintptr_t)d_list_counts % 4 != 0 || (uintptr_t)d_poses7 % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, "render_points: d_xyz, d_list_counts and d_poses7 must be 4-byte aligned");
    if ((uintptr_t)d_depth % 2 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, "render_points: d_depth must be 2-byte aligned");
    if ((uintptr_t)d_counts % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, "render_points: d_counts must be 4-byte aligned");
    if ((st = require_device()) != VORS_OK) return st;
    RenderCall call{};
    call.n = n;
    call.xyz = d_xyz;
    call.list_gray = d_list_gray;
    call.list_counts = d_list_counts;
    call.capacity = capacity;
    call.ranges = static_cast<const uint8_t*>(d_ranges);
    call.range_stride = range_stride_bytes ? (int)range_stride_bytes : 8;
    call.k = intr_from_cam5(cam5);
    call.rows = rows;
    call.cols = cols;
    call.depth_scale = depth_scale;
    call.poses = static_cast<const float*>(d_poses7);
    call.pose_stride = stride_words(pose_stride_bytes, 7);
    call.footprint = footprint;
    call.zkey = d_zkey;
    call.depth = d_depth;
    call.gray = d_gray;
    call.counts = d_counts;
    launch_render_points(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_render_points_host(const float* xyz, const uint8_t* list_gray, uint32_t count, int capacity, const uint32_t range2[2],
                                    const float cam5[5], int rows, int cols, float depth_scale, const float pose7[7], int footprint, uint64_t* zkey,
                                    uint16_t* depth, uint8_t* gray, uint32_t counts[VORS_RENDER_COUNTS]) {
    vors_status st = render_refusals("render_points_host", xyz, list_gray, cam5, capacity, rows, cols, depth_scale, footprint, zkey);
    if (st != VORS_OK) return st;
    const Intr k = intr_from_cam5(cam5);
    Iso pose = iso_identity();
    if (pose7) pose = iso_load(pose7);
    const size_t plane = (size_t)rows * (size_t)cols;
    // the range of ranks, clipped to the written prefix (the text of render_splat_kernel)
    const uint32_t n = count < (uint32_t)capacity ? count : (uint32_t)capacity;
    uint32_t first = 0, last = n;
    if (range2) {
        first = range2[0] < n ? range2[0] : n;
        last = range2[1] > n - first ? n : first + range2[1];
    }
    for (size_t q = 0; q < plane; ++q) zkey[q] = VORS_ZKEY_EMPTY;
    uint32_t c[VORS_RENDER_COUNTS] = {0, 0, 0, 0};
    for (uint32_t rank = first; rank < last; ++rank) {
        const float* p = xyz + 3 * (size_t)rank;
        const RenderPoint rp = render_point(k, pose7 != nullptr, pose, V3{p[0], p[1], p[2]}, footprint, cols, rows);
        bool landed = false;
        if (rp.candidate) {
            const uint64_t key = render_key(rp.z, rank);
            landed = render_footprint(rp, footprint, cols, rows, [&](int q) {
                if (key < zkey[q]) zkey[q] = key;
            });
        }
        c[0] += 1;
        c[1] += rp.in_front ? 1 : 0;
        c[2] += landed ? 1 : 0;
    }
    for (size_t q = 0; q < plane; ++q) {
        const RenderedPixel o = render_resolve(depth_scale, zkey[q], list_gray);
        if (depth) depth[q] = o.depth;
        if (gray) gray[q] = o.gray;
        c[3] += o.covered ? 1 : 0;
    }
    if (counts)
        for (int i = 0; i < VORS_RENDER_COUNTS; ++i) counts[i] = c[i];
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Surface normals of depth planes (vors_depth_normals, vors_points_normals, vors_depth_normals_host): the refusals all three share, the
// device entries (normal_kernels.hip) and the host entry, which runs the kernels' own text (lie.h depth_normal_taps, depth_normal).
// ---------------------------------------------------------------------------------------------------------------
static vors_status normal_refusals(const char* who, const void* depth, const float* cam5, int rows, int cols, float depth_scale, int step,
                                   float jump_m, bool list, const void* pixel, int capacity, const void* normals, const void* counts) {
    const std::string w(who);
    if (!depth) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth is NULL");
    if (!cam5) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": cam5 is NULL");
    if (list && !pixel) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a list (pixel) is NULL");
    if (!normals && !counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": normals and counts are both NULL (at least one output is required)");
    if (step < 1 || step > 8) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": step must be in 1..8");
    if (!(jump_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": jump_m must be >= 0 (and not NaN)");
    if (!(depth_scale > 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth_scale must be > 0");
    if (rows < 1 || cols < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows and cols must be >= 1");
    if (list && capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": capacity must be >= 1");
    if (rows > 65535 || cols > 65535 || (long long)rows * cols > (1ll << 28))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels");
    if ((uintptr_t)depth % 2 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth must be 2-byte aligned");
    if ((uintptr_t)pixel % 4 != 0 || (uintptr_t)normals % 4 != 0 || (uintptr_t)counts % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": pixel, normals and counts must be 4-byte aligned");
    return VORS_OK;
}
static vors_status normal_stride_refusals(const char* who, const void* d_poses7, size_t pose_stride_bytes, const void* d_ranges,
                                          size_t range_stride_bytes) {
    vors_status st = list_stride_refusals(who, pose_stride_bytes, range_stride_bytes);
    if (st != VORS_OK) return st;
    if ((uintptr_t)d_ranges % 4 != 0 || (uintptr_t)d_poses7 % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": d_ranges and d_poses7 must be 4-byte aligned");
    return VORS_OK;
}
static NormalCall normal_call(int n, const uint16_t* d_depth, const float cam5[5], int rows, int cols, float depth_scale, int step, float jump_m,
                              const void* d_poses7, size_t pose_stride_bytes, float* d_normals, uint32_t* d_counts) {
    NormalCall call{};
    call.n = n;
    call.depth = d_depth;
    call.k = intr_from_cam5(cam5);
    call.rows = rows;
    call.cols = cols;
    call.depth_scale = depth_scale;
    call.step = step;
    call.jump_m = jump_m;
    call.poses = static_cast<const float*>(d_poses7);
    call.pose_stride = stride_words(pose_stride_bytes, 7);
    call.normals = d_normals;
    call.counts = d_counts;
    return call;
}

vors_status vors_depth_normals(int n, const uint16_t* d_depth, const float cam5[5], int rows, int cols, float depth_scale, int step,
                               float jump_m, const void* d_poses7, size_t pose_stride_bytes, float* d_normals, uint32_t* d_counts,
                               void* hip_stream) {
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "depth_normals: n must be >= 1");
    vors_status st = normal_refusals("depth_normals", d_depth, cam5, rows, cols, depth_scale, step, jump_m, false, nullptr, 0, d_normals, d_counts);
    if (st != VORS_OK) return st;
    if ((st = normal_stride_refusals("depth_normals", d_poses7, pose_stride_bytes, nullptr, 0)) != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    launch_depth_normals(normal_call(n, d_depth, cam5, rows, cols, depth_scale, step, jump_m, d_poses7, pose_stride_bytes, d_normals, d_counts),
                         static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_points_normals(int n, const uint16_t* d_depth, const uint32_t* d_pixel, const uint32_t* d_list_counts, int capacity,
                                const void* d_ranges, size_t range_stride_bytes, const float cam5[5], int rows, int cols, float depth_scale,
                                int step, float jump_m, const void* d_poses7, size_t pose_stride_bytes, float* d_normals, uint32_t* d_counts,
                                void* hip_stream) {
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "points_normals: n must be >= 1");
    if (!d_list_counts) return fail(VORS_ERR_INVALID_ARGUMENT, "points_normals: a list (d_list_counts) is NULL");
    if ((uintptr_t)d_list_counts % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, "points_normals: d_list_counts must be 4-byte aligned");
    vors_status st =
        normal_refusals("points_normals", d_depth, cam5, rows, cols, depth_scale, step, jump_m, true, d_pixel, capacity, d_normals, d_counts);
    if (st != VORS_OK) return st;
    if ((st = normal_stride_refusals("points_normals", d_poses7, pose_stride_bytes, d_ranges, range_stride_bytes)) != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    NormalCall call = normal_call(n, d_depth, cam5, rows, cols, depth_scale, step, jump_m, d_poses7, pose_stride_bytes, d_normals, d_counts);
    call.pixel = d_pixel;
    call.list_counts = d_list_counts;
    call.capacity = capacity;
    call.ranges = static_cast<const uint8_t*>(d_ranges);
    call.range_stride = range_stride_bytes ? (int)range_stride_bytes : 8;
    launch_points_normals(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_depth_normals_host(const uint16_t* depth, const float cam5[5], int rows, int cols, float depth_scale, int step, float jump_m,
                                    const float pose7[7], const uint32_t* pixel, uint32_t count, int capacity, const uint32_t range2[2],
                                    float* normals, uint32_t counts[VORS_NORMAL_COUNTS]) {
    const bool list = pixel != nullptr;
    vors_status st =
        normal_refusals("depth_normals_host", depth, cam5, rows, cols, depth_scale, step, jump_m, list, pixel, capacity, normals, counts);
    if (st != VORS_OK) return st;
    const Intr k = intr_from_cam5(cam5);
    Iso pose = iso_identity();
    if (pose7) pose = iso_load(pose7);
    uint32_t c[VORS_NORMAL_COUNTS] = {0, 0, 0};
    // one pixel, written at `slot` (the text of the kernels: the taps of a pixel inside the plane, then depth_normal)
    auto one = [&](int x, int y, size_t slot) {
        const bool inside = x < cols && y < rows;
        const NormalTaps t = inside ? depth_normal_taps(x, y, cols, rows, step) : NormalTaps{0, 0, 0, 0, 0};
        const DepthNormal o = depth_normal(k, depth_scale, step, jump_m, x, y, cols, rows, depth[t.c], depth[t.l], depth[t.r], depth[t.u], depth[t.d],
                                           pose7 != nullptr, pose);
        c[0] += 1;
        c[1] += o.has_depth ? 1 : 0;
        c[2] += o.has_normal ? 1 : 0;
        if (normals) {
            normals[3 * slot] = o.n.x;
            normals[3 * slot + 1] = o.n.y;
            normals[3 * slot + 2] = o.n.z;
        }
    };
    if (!list) {
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) one(x, y, (size_t)y * (size_t)cols + (size_t)x);
    } else {
        // the range of ranks, clipped to the written prefix (the text of points_normals_kernel)
        const uint32_t n = count < (uint32_t)capacity ? count : (uint32_t)capacity;
        uint32_t first = 0, last = n;
        if (range2) {
            first = range2[0] < n ? range2[0] : n;
            last = range2[1] > n - first ? n : first + range2[1];
        }
        for (uint32_t rank = first; rank < last; ++rank) one((int)(pixel[rank] & 0xffffu), (int)(pixel[rank] >> 16), rank);
    }
    if (counts)
        for (int i = 0; i < VORS_NORMAL_COUNTS; ++i) counts[i] = c[i];
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The sensor front end (vors_undistort_frames, vors_undistort_frame_host, vors_undistort_source_host, vors_register_depth,
// vors_register_depth_host): the refusals each pair shares, the device entries (frontend_kernels.hip) and the host entries, which run the
// kernels' own texts (lie.h undistort_source, undistort_taps, undistort_gray; register_point, render_point, render_footprint,
// register_resolve).
// ---------------------------------------------------------------------------------------------------------------
static bool plane_size_ok(int rows, int cols) {
    return rows >= 1 && cols >= 1 && rows <= 65535 && cols <= 65535 && (long long)rows * cols <= (1ll << 28);
}
// The cameras and the coefficients of an undistortion: every value finite, no focal length 0
static vors_status undistort_camera_refusals(const std::string& w, const float* cam_in5, const float* dist5, const float* cam_out5) {
    if (!cam_in5 || !cam_out5) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": cam_in5 or cam_out5 is NULL");
    for (int i = 0; i < 5; ++i)
        if (!f32_finite(cam_in5[i]) || !f32_finite(cam_out5[i]) || (dist5 && !f32_finite(dist5[i])))
            return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a camera value or a distortion coefficient is not finite");
    if (cam_in5[2] == 0.0f || cam_in5[3] == 0.0f || cam_out5[2] == 0.0f || cam_out5[3] == 0.0f)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": fu and fv of both cameras must not be 0");
    return VORS_OK;
}
static Dist5 dist_from_dist5(const float* dist5) {
    return dist5 ? Dist5{dist5[0], dist5[1], dist5[2], dist5[3], dist5[4]} : Dist5{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
}
static vors_status undistort_refusals(const char* who, const UndistortCall& c, const float* cam_in5, const float* dist5, const float* cam_out5) {
    const std::string w(who);
    if (!c.gray && !c.depth) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the grey and the depth planes are both NULL");
    if ((c.gray_out && !c.gray) || (c.depth_out && !c.depth))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": an output plane is asked for without its input plane");
    if (!c.gray_out && !c.depth_out && !c.map && !c.counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": no output at all");
    vors_status st = undistort_camera_refusals(w, cam_in5, dist5, cam_out5);
    if (st != VORS_OK) return st;
    if (c.border < 0 || c.border > 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": border must be 0 (zero) or 1 (edge replicate)");
    if (!plane_size_ok(c.in_rows, c.in_cols) || !plane_size_ok(c.out_rows, c.out_cols))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows and cols must lie in 1..65535 and rows * cols must not exceed 2^28 pixels");
    if ((uintptr_t)c.depth % 2 != 0 || (uintptr_t)c.depth_out % 2 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the depth planes must be 2-byte aligned");
    if ((uintptr_t)c.map % 4 != 0 || (uintptr_t)c.counts % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": map and counts must be 4-byte aligned");
    return VORS_OK;
}
static UndistortCall undistort_call(int n, const uint8_t* gray, const uint16_t* depth, int in_rows, int in_cols, int out_rows, int out_cols,
                                    int border, uint8_t* gray_out, uint16_t* depth_out, float* map, uint32_t* counts) {
    UndistortCall c{};
    c.n = n; c.gray = gray; c.depth = depth; c.in_rows = in_rows; c.in_cols = in_cols; c.out_rows = out_rows; c.out_cols = out_cols;
    c.border = border; c.gray_out = gray_out; c.depth_out = depth_out; c.map = map; c.counts = counts;
    return c;
}
// (after the refusals: the cameras are there)
static void undistort_cameras(UndistortCall& c, const float* cam_in5, const float* dist5, const float* cam_out5) {
    c.k_in = intr_from_cam5(cam_in5);
    c.dist = dist_from_dist5(dist5);
    c.k_out = intr_from_cam5(cam_out5);
}

vors_status vors_undistort_frames(int n, const uint8_t* d_gray, const uint16_t* d_depth, int in_rows, int in_cols, const float cam_in5[5],
                                  const float dist5[5], const float cam_out5[5], int out_rows, int out_cols, int border, uint8_t* d_gray_out,
                                  uint16_t* d_depth_out, float* d_map, uint32_t* d_counts, void* hip_stream) {
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "undistort_frames: n must be >= 1");
    UndistortCall call = undistort_call(n, d_gray, d_depth, in_rows, in_cols, out_rows, out_cols, border, d_gray_out, d_depth_out, d_map, d_counts);
    vors_status st = undistort_refusals("undistort_frames", call, cam_in5, dist5, cam_out5);
    if (st != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    undistort_cameras(call, cam_in5, dist5, cam_out5);
    launch_undistort(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_undistort_frame_host(const uint8_t* gray, const uint16_t* depth, int in_rows, int in_cols, const float cam_in5[5],
                                      const float dist5[5], const float cam_out5[5], int out_rows, int out_cols, int border, uint8_t* gray_out,
                                      uint16_t* depth_out, float* map, uint32_t counts[VORS_UNDISTORT_COUNTS]) {
    UndistortCall c = undistort_call(1, gray, depth, in_rows, in_cols, out_rows, out_cols, border, gray_out, depth_out, map, counts);
    vors_status st = undistort_refusals("undistort_frame_host", c, cam_in5, dist5, cam_out5);
    if (st != VORS_OK) return st;
    undistort_cameras(c, cam_in5, dist5, cam_out5);
    uint32_t n[VORS_UNDISTORT_COUNTS] = {0, 0, 0};
    for (int y = 0; y < out_rows; ++y)
        for (int x = 0; x < out_cols; ++x) {
            const size_t i = (size_t)y * (size_t)out_cols + (size_t)x;
            float u, v;
            undistort_source(c.k_out, c.k_in, c.dist, x, y, &u, &v);
            const UndistortTaps t = undistort_taps(u, v, border, in_cols, in_rows);
            const uint16_t od = depth && t.depth >= 0 ? depth[t.depth] : (uint16_t)0;
            if (gray_out) gray_out[i] = undistort_gray(t, gray[t.i00], gray[t.i01], gray[t.i10], gray[t.i11]);
            if (depth_out) depth_out[i] = od;
            if (map) {
                map[2 * i] = u;
                map[2 * i + 1] = v;
            }
            n[0] += 1;
            n[1] += t.inside ? 1 : 0;
            n[2] += od != 0 ? 1 : 0;
        }
    if (counts)
        for (int k = 0; k < VORS_UNDISTORT_COUNTS; ++k) counts[k] = n[k];
    return VORS_OK;
}

vors_status vors_undistort_source_host(const float cam_in5[5], const float dist5[5], const float cam_out5[5], int n_pixels, const int32_t* xy,
                                       float* uv) {
    const std::string w("undistort_source_host");
    if (n_pixels < 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": n_pixels must be >= 0");
    if (n_pixels > 0 && (!xy || !uv)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": xy or uv is NULL");
    vors_status st = undistort_camera_refusals(w, cam_in5, dist5, cam_out5);
    if (st != VORS_OK) return st;
    const Intr k_in = intr_from_cam5(cam_in5), k_out = intr_from_cam5(cam_out5);
    const Dist5 dist = dist_from_dist5(dist5);
    for (int i = 0; i < n_pixels; ++i) undistort_source(k_out, k_in, dist, xy[2 * i], xy[2 * i + 1], &uv[2 * i], &uv[2 * i + 1]);
    return VORS_OK;
}

static vors_status register_refusals(const char* who, const RegisterCall& c, const float* dcam5, const float* ccam5) {
    const std::string w(who);
    if (!c.depth) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth is NULL");
    if (!dcam5 || !ccam5) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": dcam5 or ccam5 is NULL");
    if (!c.zkey) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": zkey is NULL (the pass keeps no plane of its own)");
    if ((uintptr_t)c.zkey % 8 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": zkey must be 8-byte aligned");
    if (c.footprint < 1 || c.footprint > 3) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": footprint must be 1, 2 or 3");
    if (!plane_size_ok(c.d_rows, c.d_cols) || !plane_size_ok(c.c_rows, c.c_cols))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows and cols must lie in 1..65535 and rows * cols must not exceed 2^28 pixels");
    if (!(c.scale_in > 0.0f) || !(c.scale_out > 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the depth scales must be > 0");
    if ((uintptr_t)c.depth % 2 != 0 || (uintptr_t)c.depth_out % 2 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the depth planes must be 2-byte aligned");
    if ((uintptr_t)c.src_index % 4 != 0 || (uintptr_t)c.counts % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": src_index and counts must be 4-byte aligned");
    return VORS_OK;
}
static RegisterCall register_call(int n, const uint16_t* depth, int d_rows, int d_cols, float scale_in, const float* pose7, int c_rows, int c_cols,
                                  float scale_out, int footprint, uint64_t* zkey, uint16_t* depth_out, uint32_t* src_index, uint32_t* counts) {
    RegisterCall c{};
    c.n = n; c.depth = depth; c.d_rows = d_rows; c.d_cols = d_cols; c.scale_in = scale_in; c.has_pose = pose7 != nullptr;
    c.pose = pose7 ? iso_load(pose7) : iso_identity();
    c.c_rows = c_rows; c.c_cols = c_cols; c.scale_out = scale_out; c.footprint = footprint;
    c.zkey = zkey; c.depth_out = depth_out; c.src_index = src_index; c.counts = counts;
    return c;
}

vors_status vors_register_depth(int n, const uint16_t* d_depth, const float dcam5[5], int d_rows, int d_cols, float depth_scale_in,
                                const float pose7[7], const float ccam5[5], int c_rows, int c_cols, float depth_scale_out, int footprint,
                                uint64_t* d_zkey, uint16_t* d_depth_out, uint32_t* d_src_index, uint32_t* d_counts, void* hip_stream) {
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "register_depth: n must be >= 1");
    RegisterCall call = register_call(n, d_depth, d_rows, d_cols, depth_scale_in, pose7, c_rows, c_cols, depth_scale_out, footprint, d_zkey,
                                      d_depth_out, d_src_index, d_counts);
    vors_status st = register_refusals("register_depth", call, dcam5, ccam5);
    if (st != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    call.k_d = intr_from_cam5(dcam5);
    call.k_c = intr_from_cam5(ccam5);
    launch_register_depth(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_register_depth_host(const uint16_t* depth, const float dcam5[5], int d_rows, int d_cols, float depth_scale_in,
                                     const float pose7[7], const float ccam5[5], int c_rows, int c_cols, float depth_scale_out, int footprint,
                                     uint64_t* zkey, uint16_t* depth_out, uint32_t* src_index, uint32_t counts[VORS_REGISTER_COUNTS]) {
    RegisterCall c = register_call(1, depth, d_rows, d_cols, depth_scale_in, pose7, c_rows, c_cols, depth_scale_out, footprint, zkey, depth_out,
                                   src_index, counts);
    vors_status st = register_refusals("register_depth_host", c, dcam5, ccam5);
    if (st != VORS_OK) return st;
    c.k_d = intr_from_cam5(dcam5);
    c.k_c = intr_from_cam5(ccam5);
    const size_t c_plane = (size_t)c_rows * (size_t)c_cols;
    for (size_t q = 0; q < c_plane; ++q) zkey[q] = VORS_ZKEY_EMPTY;
    uint32_t n[VORS_REGISTER_COUNTS] = {0, 0, 0, 0};
    for (int y = 0; y < d_rows; ++y)
        for (int x = 0; x < d_cols; ++x) {
            const int s = y * d_cols + x;
            const uint16_t d = depth[s];
            if (d == 0) continue;
            const V3 p = register_point(c.k_d, c.scale_in, c.has_pose, c.pose, x, y, d);
            const RenderPoint rp = render_point(c.k_c, false, c.pose, p, footprint, c_cols, c_rows);
            bool landed = false;
            if (rp.candidate) {
                const uint64_t key = render_key(rp.z, (uint32_t)s);
                landed = render_footprint(rp, footprint, c_cols, c_rows, [&](int q) {
                    if (key < zkey[q]) zkey[q] = key;
                });
            }
            n[0] += 1;
            n[1] += rp.in_front ? 1 : 0;
            n[2] += landed ? 1 : 0;
        }
    for (size_t q = 0; q < c_plane; ++q) {
        const RegisteredPixel o = register_resolve(c.scale_out, zkey[q]);
        if (depth_out) depth_out[q] = o.depth;
        if (src_index) src_index[q] = o.src;
        n[3] += o.covered ? 1 : 0;
    }
    if (counts)
        for (int k = 0; k < VORS_REGISTER_COUNTS; ++k) counts[k] = n[k];
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Point-to-plane ICP of point lists with normals against depth planes (vors_icp_points, vors_icp_points_host): the refusals both share,
// the device entry (icp_kernels.hip) and the host entry, which runs the kernels' own texts (lie.h icp_landing, icp_row, icp_products,
// icp_round) and the order of sums lie.h states.
// ---------------------------------------------------------------------------------------------------------------
static vors_status icp_refusals(const char* who, const IcpArgs& a) {
    const std::string w(who);
    const IcpCall& c = a.call;
    if (!c.xyz || !c.normals) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a list (xyz, normals) is NULL");
    if (!c.poses_in) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the start poses are NULL (an alignment needs a pose to refine)");
    if (!c.depth) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth is NULL");
    if (!a.cam5) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": cam5 is NULL");
    if (!c.poses_out) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the output poses are NULL");
    if (c.rows < 1 || c.cols < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows and cols must be >= 1");
    if (c.capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": capacity must be >= 1");
    if (c.rows > 65535 || c.cols > 65535 || (long long)c.rows * c.cols > (1ll << 28))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows / cols must not exceed 65535 and rows * cols must not exceed 2^28 pixels");
    if (!(c.depth_scale > 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth_scale must be > 0");
    if (!(c.dist_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": dist_m must be >= 0 (and not NaN)");
    if (!(c.damping >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": damping must be >= 0 (and not NaN)");
    if (!(c.step_eps >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": step_eps must be >= 0 (and not NaN)");
    if (c.iters < 0 || c.iters > 64) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": iters must be in 0..64");
    if (a.min_points < 6) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": min_points must be >= 6 (a pose has six degrees of freedom)");
    if ((uintptr_t)c.depth % 2 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": depth must be 2-byte aligned");
    if ((uintptr_t)c.xyz % 4 != 0 || (uintptr_t)c.normals % 4 != 0 || (uintptr_t)c.poses_in % 4 != 0 || (uintptr_t)c.poses_out % 4 != 0 ||
        (uintptr_t)c.stats % 4 != 0 || (uintptr_t)c.sums29 % 4 != 0 || (uintptr_t)c.residuals % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": xyz, normals, the poses, stats, sums29 and residuals must be 4-byte aligned");
    return VORS_OK;
}

// ... and what the robust entries refuse beyond that
static vors_status icp_robust_refusals(const char* who, const IcpRobust& r) {
    const std::string w(who);
    if (!(r.min_cos >= -1.0f && r.min_cos <= 1.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": min_cos must lie in [-1, 1] (and not be NaN)");
    if (!(r.huber_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": huber_m must be >= 0 (and not NaN; 0 = no Huber weight)");
    if ((uintptr_t)r.frame_normals % 4 != 0 || (uintptr_t)r.gate_counts % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the frame normals and the gate counts must be 4-byte aligned");
    return VORS_OK;
}

// photo_huber_m = photo_scale_m * photo_huber_grey, the ONE product that kernel and host twin both read
static float icp_photo_huber_m(float photo_scale_m, float photo_huber_grey) { return photo_scale_m * photo_huber_grey; }

// ... and what the joint entries refuse beyond those (j.photo_huber_m still holds photo_huber_grey, as the entries take it)
static vors_status icp_joint_refusals(const char* who, const IcpJoint& j) {
    const std::string w(who);
    if (!(j.photo_scale_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": photo_scale_m must be >= 0 (and not NaN; 0 = no photometric term)");
    if (!(j.photo_huber_m >= 0.0f))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": photo_huber_grey must be >= 0 (and not NaN; 0 = no Huber weight)");
    if (j.photo_scale_m > 0.0f && (!j.list_gray || !j.frame_gray))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": photo_scale_m > 0 needs the grey levels of the list and of the frame");
    if ((uintptr_t)j.photo_residuals % 4 != 0 || (uintptr_t)j.photo_counts % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the photo residuals and the photo counts must be 4-byte aligned");
    return VORS_OK;
}

// The three in the order every entry states them: the common part, then the parts of the form
static vors_status icp_form_refusals(const char* who, const IcpArgs& a) {
    vors_status st = icp_refusals(who, a);
    if (st == VORS_OK && a.robust) st = icp_robust_refusals(who, *a.robust);
    if (st == VORS_OK && a.joint) st = icp_joint_refusals(who, *a.joint);
    return st;
}

uint64_t vors_icp_workspace_bytes(int n, int capacity) { return n < 1 || capacity < 1 ? 0 : (uint64_t)icp_workspace_bytes(n, capacity); }

// The device pass of every form (host_common.h IcpArgs): the refusals in the name of `who`, then what the record leaves to derive
vors_status icp_points_device(const char* who, const IcpArgs& a, hipStream_t s) {
    const std::string w(who);
    IcpCall call = a.call;
    if (call.n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": n must be >= 1");
    if (!call.list_counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a list (d_list_counts) is NULL");
    vors_status st = icp_form_refusals(who, a);
    if (st != VORS_OK) return st;
    if (!a.workspace) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": d_workspace is NULL (the pass allocates nothing: vors_icp_workspace_bytes)");
    if ((st = list_stride_refusals(who, a.pose_stride_bytes, a.range_stride_bytes)) != VORS_OK) return st;
    if ((uintptr_t)call.ranges % 4 != 0 || (uintptr_t)call.list_counts % 4 != 0 || (uintptr_t)a.workspace % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": d_ranges, d_list_counts and d_workspace must be 4-byte aligned");
    if ((st = require_device()) != VORS_OK) return st;
    call.range_stride = a.range_stride_bytes ? (int)a.range_stride_bytes : 8;
    call.pose_stride = stride_words(a.pose_stride_bytes, 7);
    call.k = intr_from_cam5(a.cam5);
    call.min_points = (uint32_t)a.min_points;
    icp_workspace_carve(&call, a.workspace, call.n, call.capacity);
    IcpJoint jt{};
    if (a.joint) {
        jt = *a.joint;
        jt.photo_huber_m = icp_photo_huber_m(jt.photo_scale_m, jt.photo_huber_m);
    }
    launch_icp_points(call, a.robust, s, a.joint ? &jt : nullptr);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

// The arguments every entry shares, device and host, as the record holds them. A host entry states its ONE list as n = 1 with the
// count behind d_list_counts (the caller's to keep alive through the pass), range2 behind d_ranges, no strides and no workspace.
static IcpArgs icp_args(int n, const float* d_xyz, const float* d_normals, const uint32_t* d_list_counts, int capacity, const void* d_ranges,
                        size_t range_stride_bytes, const void* d_poses7_in, size_t pose_stride_bytes, const uint16_t* d_depth, const float cam5[5],
                        int rows, int cols, float depth_scale, float dist_m, float damping, float step_eps, int iters, int min_points,
                        void* d_workspace, float* d_poses7_out, vors_icp_stats* d_stats, float* d_sums29, float* d_residuals,
                        const IcpRobust* robust = nullptr, const IcpJoint* joint = nullptr) {
    IcpArgs a{};
    IcpCall& c = a.call;
    c.n = n; c.xyz = d_xyz; c.normals = d_normals; c.list_counts = d_list_counts; c.capacity = capacity;
    c.ranges = static_cast<const uint8_t*>(d_ranges); a.range_stride_bytes = range_stride_bytes;
    c.poses_in = static_cast<const float*>(d_poses7_in); a.pose_stride_bytes = pose_stride_bytes;
    c.depth = d_depth; a.cam5 = cam5; c.rows = rows; c.cols = cols; c.depth_scale = depth_scale;
    c.dist_m = dist_m; c.damping = damping; c.step_eps = step_eps; c.iters = iters; a.min_points = min_points;
    a.workspace = d_workspace; c.poses_out = d_poses7_out; c.stats = d_stats; c.sums29 = d_sums29; c.residuals = d_residuals;
    a.robust = robust; a.joint = joint;
    return a;
}

vors_status vors_icp_points(int n, const float* d_xyz, const float* d_normals, const uint32_t* d_list_counts, int capacity, const void* d_ranges,
                            size_t range_stride_bytes, const void* d_poses7_in, size_t pose_stride_bytes, const uint16_t* d_depth,
                            const float cam5[5], int rows, int cols, float depth_scale, float dist_m, float damping, float step_eps, int iters,
                            int min_points, void* d_workspace, float* d_poses7_out, vors_icp_stats* d_stats, float* d_sums29, float* d_residuals,
                            void* hip_stream) {
    return icp_points_device("icp_points",
                             icp_args(n, d_xyz, d_normals, d_list_counts, capacity, d_ranges, range_stride_bytes, d_poses7_in, pose_stride_bytes,
                                      d_depth, cam5, rows, cols, depth_scale, dist_m, damping, step_eps, iters, min_points, d_workspace,
                                      d_poses7_out, d_stats, d_sums29, d_residuals),
                             static_cast<hipStream_t>(hip_stream));
}

vors_status vors_icp_points_robust(int n, const float* d_xyz, const float* d_normals, const uint32_t* d_list_counts, int capacity,
                                   const void* d_ranges, size_t range_stride_bytes, const void* d_poses7_in, size_t pose_stride_bytes,
                                   const uint16_t* d_depth, const float cam5[5], int rows, int cols, float depth_scale, float dist_m, float damping,
                                   float step_eps, int iters, int min_points, const float* d_frame_normals, float min_cos, float huber_m,
                                   void* d_workspace, float* d_poses7_out, vors_icp_stats* d_stats, float* d_sums29, float* d_residuals,
                                   uint32_t* d_gate_counts, void* hip_stream) {
    const IcpRobust robust{d_frame_normals, min_cos, huber_m, d_gate_counts};
    return icp_points_device("icp_points_robust",
                             icp_args(n, d_xyz, d_normals, d_list_counts, capacity, d_ranges, range_stride_bytes, d_poses7_in, pose_stride_bytes,
                                      d_depth, cam5, rows, cols, depth_scale, dist_m, damping, step_eps, iters, min_points, d_workspace,
                                      d_poses7_out, d_stats, d_sums29, d_residuals, &robust),
                             static_cast<hipStream_t>(hip_stream));
}

vors_status vors_icp_points_joint(int n, const float* d_xyz, const float* d_normals, const uint8_t* d_list_gray, const uint32_t* d_list_counts,
                                  int capacity, const void* d_ranges, size_t range_stride_bytes, const void* d_poses7_in, size_t pose_stride_bytes,
                                  const uint16_t* d_depth, const uint8_t* d_frame_gray, const float cam5[5], int rows, int cols, float depth_scale,
                                  float dist_m, float damping, float step_eps, int iters, int min_points, const float* d_frame_normals,
                                  float min_cos, float huber_m, float photo_scale_m, float photo_huber_grey, void* d_workspace,
                                  float* d_poses7_out, vors_icp_stats* d_stats, float* d_sums29, float* d_residuals, uint32_t* d_gate_counts,
                                  float* d_photo_residuals, uint32_t* d_photo_counts, void* hip_stream) {
    const IcpRobust robust{d_frame_normals, min_cos, huber_m, d_gate_counts};
    const IcpJoint joint{d_list_gray, d_frame_gray, photo_scale_m, photo_huber_grey, d_photo_residuals, d_photo_counts};
    return icp_points_device("icp_points_joint",
                             icp_args(n, d_xyz, d_normals, d_list_counts, capacity, d_ranges, range_stride_bytes, d_poses7_in, pose_stride_bytes,
                                      d_depth, cam5, rows, cols, depth_scale, dist_m, damping, step_eps, iters, min_points, d_workspace,
                                      d_poses7_out, d_stats, d_sums29, d_residuals, &robust, &joint),
                             static_cast<hipStream_t>(hip_stream));
}

// The loop of the host entries, after their refusals, over the ONE list of c (c.list_counts[0], c.ranges = its range2 or NULL, c.k set).
// point(pose, landing, nw, pixel, rank, a, products) is the per-point rule: it fills the row a[7] and the point's 28 products, and
// returns the last gate passed and whether the point lies on Huber's linear branch (the joint pass: and what its photometric row gave).
struct IcpHostPoint {
    IcpGate gate;
    bool linear;
    bool photo = false, photo_linear = false;  // the joint pass: a photometric row exists; it lies on its Huber's linear branch
    float photo_d = 0.0f;                      // I - grey in grey levels
};
extern "C++" template <class Point>
static void icp_host_loop(const IcpCall& c, Point point, uint32_t* gate_counts, float* photo_residuals, uint32_t* photo_counts) {
    const Intr& k = c.k;
    const int rows = c.rows, cols = c.cols;
    uint32_t first, last;
    icp_range(c.list_counts[0], c.capacity, reinterpret_cast<const uint32_t*>(c.ranges), &first, &last);
    const uint32_t nchunks = (last - first + (VORS_ICP_CHUNK - 1)) / VORS_ICP_CHUNK;
    std::vector<float> v((size_t)VORS_ICP_CHUNK * VORS_ICP_SUMS);
    float sums[VORS_ICP_SUMS];
    uint32_t matched = 0, gates[VORS_ICP_GATE_COUNTS], photos[ICP_PHOTO_COUNTS];
    // one evaluation at `pose`: per chunk the slots, the halving tree, then the chunk sums in ascending order (the text of icp_eval_kernel
    // and icp_solve_kernel)
    auto evaluate = [&](const Iso& pose, float* res, float* photo_res) {
        for (int q = 0; q < VORS_ICP_SUMS; ++q) sums[q] = 0.0f;
        for (int q = 0; q < VORS_ICP_GATE_COUNTS; ++q) gates[q] = 0u;
        for (int q = 0; q < ICP_PHOTO_COUNTS; ++q) photos[q] = 0u;
        matched = 0;
        for (uint32_t chunk = 0; chunk < nchunks; ++chunk) {
            const uint32_t base = first + chunk * VORS_ICP_CHUNK;
            for (uint32_t s = 0; s < VORS_ICP_CHUNK; ++s) {
                float a[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                float* products = v.data() + (size_t)s * VORS_ICP_SUMS;
                const uint32_t rank = base + s;
                if (rank < last) {
                    const float* p = c.xyz + 3 * (size_t)rank;
                    const float* nn = c.normals + 3 * (size_t)rank;
                    const IcpLanding l = icp_landing(k, pose, V3{p[0], p[1], p[2]}, cols, rows);
                    const size_t pixel = l.lands ? (size_t)l.y * (size_t)cols + (size_t)l.x : 0;
                    const IcpHostPoint o = point(pose, l, V3{nn[0], nn[1], nn[2]}, pixel, rank, a, products);
                    const bool m = o.gate == ICP_GATE_MATCHED;
                    matched += m ? 1u : 0u;
                    gates[0] += o.gate >= ICP_GATE_DEPTH ? 1u : 0u;
                    gates[1] += o.gate >= ICP_GATE_DIST ? 1u : 0u;
                    gates[2] += m ? 1u : 0u;
                    gates[3] += o.linear ? 1u : 0u;
                    photos[0] += o.photo ? 1u : 0u;
                    photos[1] += o.photo_linear ? 1u : 0u;
                    if (res) res[rank] = m ? a[0] : nanf("");
                    if (photo_res) photo_res[rank] = o.photo ? o.photo_d : nanf("");
                } else {
                    icp_products(a, products);  // (a slot beyond the range: zeros)
                }
            }
            for (uint32_t w = VORS_ICP_CHUNK / 2; w >= 1; w /= 2)
                for (uint32_t s = 0; s < w; ++s)
                    for (int q = 0; q < VORS_ICP_SUMS; ++q) v[(size_t)s * VORS_ICP_SUMS + q] = v[(size_t)s * VORS_ICP_SUMS + q] + v[(size_t)(s + w) * VORS_ICP_SUMS + q];
            for (int q = 0; q < VORS_ICP_SUMS; ++q) sums[q] = chunk == 0 ? v[q] : sums[q] + v[q];
        }
    };
    Iso pose = iso_load(c.poses_in);
    vors_icp_stats o{VORS_ICP_ITERATIONS, 0u, last - first, 0u, 0.0f, 0.0f};
    for (int it = 0; it < c.iters; ++it) {
        evaluate(pose, nullptr, nullptr);
        float step_norm = 0.0f;
        const IcpStatus verdict = icp_round(sums, matched, c.min_points, c.damping, c.step_eps, &pose, &step_norm);
        if (verdict == ICP_ITERATIONS || verdict == ICP_CONVERGED) {
            o.iterations += 1u;
            o.last_step_norm = step_norm;
        }
        if (verdict != ICP_ITERATIONS) {  // frozen
            o.status = (uint32_t)verdict;
            break;
        }
    }
    evaluate(pose, c.residuals, photo_residuals);
    o.matched = matched;
    o.rms = sqrtf(sums[0] / (float)matched);
    iso_store(pose, c.poses_out);
    if (c.stats) *c.stats = o;
    if (c.sums29) icp_sums29(sums, matched, c.sums29);
    if (gate_counts)
        for (int q = 0; q < VORS_ICP_GATE_COUNTS; ++q) gate_counts[q] = gates[q];
    if (photo_counts)
        for (int q = 0; q < ICP_PHOTO_COUNTS; ++q) photo_counts[q] = photos[q];
}

// The host pass of every form, mirroring icp_points_device: the refusals in the name of `who`, then the loop with the form's per-point
// rule. The rules are three texts: the plain one (icp_row / icp_products), the robust one (icp_row_robust / icp_products_robust), and the
// joint one, which is the robust one followed by the photometric row.
static vors_status icp_points_host(const char* who, const IcpArgs& a) {
    vors_status st = icp_form_refusals(who, a);
    if (st != VORS_OK) return st;
    IcpCall c = a.call;
    const Intr k = c.k = intr_from_cam5(a.cam5);
    c.min_points = (uint32_t)a.min_points;
    const uint16_t* depth = c.depth;
    const int rows = c.rows, cols = c.cols;
    if (!a.robust) {
        icp_host_loop(c,
                      [&](const Iso& pose, const IcpLanding& l, const V3& nw, size_t pixel, uint32_t, float* row, float* products) {
                          const bool m = icp_row(k, c.depth_scale, c.dist_m, pose, l, nw, depth[pixel], row);
                          icp_products(row, products);
                          return IcpHostPoint{m ? ICP_GATE_MATCHED : ICP_GATE_NONE, false};
                      },
                      nullptr, nullptr, nullptr);
        return VORS_OK;
    }
    const IcpRobust r = *a.robust;
    IcpJoint j{};
    if (a.joint) j = *a.joint;
    const float photo_huber_m = icp_photo_huber_m(j.photo_scale_m, j.photo_huber_m);
    const bool photo_on = j.photo_scale_m > 0.0f && rows >= 2 && cols >= 2;  // (no footprint fits a plane of one row or column)
    with_bool(r.frame_normals != nullptr, [&](auto nrm) {
        with_bool(r.huber_m > 0.0f, [&](auto hub) {
            auto robust_point = [&](const Iso& pose, const IcpLanding& l, const V3& nw, size_t pixel, uint32_t, float* row, float* products) {
                V3 nf{0.0f, 0.0f, 0.0f};
                if constexpr (decltype(nrm)::value) nf = V3{r.frame_normals[3 * pixel], r.frame_normals[3 * pixel + 1], r.frame_normals[3 * pixel + 2]};
                const IcpGate g = icp_row_robust<decltype(nrm)::value>(k, c.depth_scale, c.dist_m, r.min_cos, pose, l, nw, depth[pixel], nf, row);
                return IcpHostPoint{g, icp_products_robust<decltype(hub)::value>(row, r.huber_m, products)};
            };
            if (!a.joint) {
                icp_host_loop(c, robust_point, r.gate_counts, nullptr, nullptr);
                return;
            }
            with_bool(photo_huber_m > 0.0f, [&](auto phub) {
                icp_host_loop(c,
                              [&](const Iso& pose, const IcpLanding& l, const V3& nw, size_t pixel, uint32_t rank, float* row, float* products) {
                                  IcpHostPoint o = robust_point(pose, l, nw, pixel, rank, row, products);
                                  const IcpFootprint f = icp_photo_footprint(k, l.c, cols, rows);
                                  o.photo = o.gate == ICP_GATE_MATCHED && photo_on && f.inside;
                                  if (o.photo) {
                                      const uint8_t* t = j.frame_gray + f.off;
                                      float ap[7], pp[VORS_ICP_SUMS];
                                      o.photo_d = icp_row_photo(k, j.photo_scale_m, l.c, f, true, t[0], t[1], t[cols], t[cols + 1], j.list_gray[rank], ap);
                                      o.photo_linear = icp_products_robust<decltype(phub)::value>(ap, photo_huber_m, pp);
                                      for (int q = 0; q < VORS_ICP_SUMS; ++q) products[q] = products[q] + pp[q];
                                  }
                                  return o;
                              },
                              r.gate_counts, j.photo_residuals, j.photo_counts);
            });
        });
    });
    return VORS_OK;
}

vors_status vors_icp_points_host(const float* xyz, const float* normals, uint32_t count, int capacity, const uint32_t range2[2],
                                 const float pose7_in[7], const uint16_t* depth, const float cam5[5], int rows, int cols, float depth_scale,
                                 float dist_m, float damping, float step_eps, int iters, int min_points, float pose7_out[7], vors_icp_stats* stats,
                                 float sums29[29], float* residuals) {
    return icp_points_host("icp_points_host",
                           icp_args(1, xyz, normals, &count, capacity, range2, 0, pose7_in, 0, depth, cam5, rows, cols, depth_scale, dist_m, damping,
                                    step_eps, iters, min_points, nullptr, pose7_out, stats, sums29, residuals));
}

vors_status vors_icp_points_robust_host(const float* xyz, const float* normals, uint32_t count, int capacity, const uint32_t range2[2],
                                        const float pose7_in[7], const uint16_t* depth, const float cam5[5], int rows, int cols,
                                        float depth_scale, float dist_m, float damping, float step_eps, int iters, int min_points,
                                        const float* frame_normals, float min_cos, float huber_m, float pose7_out[7], vors_icp_stats* stats,
                                        float sums29[29], float* residuals, uint32_t gate_counts[VORS_ICP_GATE_COUNTS]) {
    const IcpRobust robust{frame_normals, min_cos, huber_m, gate_counts};
    return icp_points_host("icp_points_robust_host",
                           icp_args(1, xyz, normals, &count, capacity, range2, 0, pose7_in, 0, depth, cam5, rows, cols, depth_scale, dist_m, damping,
                                    step_eps, iters, min_points, nullptr, pose7_out, stats, sums29, residuals, &robust));
}

vors_status vors_icp_points_joint_host(const float* xyz, const float* normals, const uint8_t* list_gray, uint32_t count, int capacity,
                                       const uint32_t range2[2], const float pose7_in[7], const uint16_t* depth, const uint8_t* frame_gray,
                                       const float cam5[5], int rows, int cols, float depth_scale, float dist_m, float damping, float step_eps,
                                       int iters, int min_points, const float* frame_normals, float min_cos, float huber_m, float photo_scale_m,
                                       float photo_huber_grey, float pose7_out[7], vors_icp_stats* stats, float sums29[29], float* residuals,
                                       uint32_t gate_counts[VORS_ICP_GATE_COUNTS], float* photo_residuals,
                                       uint32_t photo_counts[VORS_ICP_PHOTO_COUNTS]) {
    const IcpRobust robust{frame_normals, min_cos, huber_m, gate_counts};
    const IcpJoint joint{list_gray, frame_gray, photo_scale_m, photo_huber_grey, photo_residuals, photo_counts};
    return icp_points_host("icp_points_joint_host",
                           icp_args(1, xyz, normals, &count, capacity, range2, 0, pose7_in, 0, depth, cam5, rows, cols, depth_scale, dist_m, damping,
                                    step_eps, iters, min_points, nullptr, pose7_out, stats, sums29, residuals, &robust, &joint));
}

// ---------------------------------------------------------------------------------------------------------------
// Pose-graph optimisation (vors_pose_graph_optimize, vors_pose_graph_optimize_host; include/vors_hip.h 2g): the refusals both share, the
// device entry (pose_graph_kernels.hip) and the host entry, which runs the kernels' own texts (lie.h pg_*) launch by launch, with the
// order of sums the header states.
// ---------------------------------------------------------------------------------------------------------------
static vors_status pg_refusals(const char* who, const PgCall& c) {
    const std::string w(who);
    if (!c.poses_in) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the input poses are NULL");
    if (!c.node_counts || !c.edge_counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a count (nodes, edges) is NULL");
    if (!c.edges || !c.meas) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the edges or their measurements are NULL");
    if (!c.poses_out) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the output poses are NULL");
    if (c.node_capacity < 1 || c.edge_capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": node_capacity and edge_capacity must be >= 1");
    if (c.node_capacity > (1 << 28) || c.edge_capacity > (1 << 28))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": node_capacity and edge_capacity must not exceed 2^28");
    if (!(c.lambda0 >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": lambda0 must be >= 0 (and not NaN)");
    if (!(c.step_eps >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": step_eps must be >= 0 (and not NaN)");
    if (!(c.cg_tol >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": cg_tol must be >= 0 (and not NaN)");
    if (c.iters < 0 || c.iters > 64) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": iters must be in 0..64");
    if (c.cg_iters < 1 || c.cg_iters > 256) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": cg_iters must be in 1..256");
    if ((uintptr_t)c.poses_in % 4 != 0 || (uintptr_t)c.node_counts % 4 != 0 || (uintptr_t)c.edge_counts % 4 != 0 || (uintptr_t)c.edges % 4 != 0 ||
        (uintptr_t)c.meas % 4 != 0 || (uintptr_t)c.info % 4 != 0 || (uintptr_t)c.weight % 4 != 0 || (uintptr_t)c.poses_out % 4 != 0 ||
        (uintptr_t)c.stats % 4 != 0 || (uintptr_t)c.edge_residuals % 4 != 0 || (uintptr_t)c.edge_energy % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the poses, counts, edges, measurements, information, weights, stats, residuals and energies "
                                                   "must be 4-byte aligned");
    return VORS_OK;
}

static PgCall pg_call(int n, const void* poses7_in, const uint32_t* node_counts, int node_capacity, const uint32_t* edges, const uint32_t* edge_counts,
                      int edge_capacity, const float* meas7, const float* info36, const float* edge_weight, const uint8_t* fixed, float lambda0,
                      float step_eps, float cg_tol, int iters, int cg_iters, float* poses7_out, vors_pose_graph_stats* stats, float* edge_residuals,
                      float* edge_energy) {
    PgCall c{};
    c.n = n; c.node_capacity = node_capacity; c.edge_capacity = edge_capacity;
    c.poses_in = static_cast<const float*>(poses7_in); c.pose_stride = 7;
    c.node_counts = node_counts; c.edges = edges; c.edge_counts = edge_counts; c.meas = meas7; c.info = info36; c.weight = edge_weight; c.fixed = fixed;
    c.lambda0 = lambda0; c.step_eps = step_eps; c.cg_tol = cg_tol; c.iters = iters; c.cg_iters = cg_iters;
    c.poses_out = poses7_out; c.stats = stats; c.edge_residuals = edge_residuals; c.edge_energy = edge_energy;
    return c;
}

uint64_t vors_pose_graph_workspace_bytes(int n, int node_capacity, int edge_capacity) {
    if (n < 1 || node_capacity < 1 || edge_capacity < 1) return 0;
    return (uint64_t)pg_workspace_carve(nullptr, nullptr, n, node_capacity, edge_capacity);
}

vors_status vors_pose_graph_optimize(int n, const void* d_poses7_in, size_t pose_stride_bytes, const uint32_t* d_node_counts, int node_capacity,
                                     const uint32_t* d_edges, const uint32_t* d_edge_counts, int edge_capacity, const float* d_meas7,
                                     const float* d_info36, const float* d_edge_weight, const uint8_t* d_fixed, float lambda0, float step_eps,
                                     float cg_tol, int iters, int cg_iters, void* d_workspace, float* d_poses7_out, vors_pose_graph_stats* d_stats,
                                     float* d_edge_residuals, float* d_edge_energy, void* hip_stream) {
    const char* who = "pose_graph_optimize";
    const std::string w(who);
    PgCall call = pg_call(n, d_poses7_in, d_node_counts, node_capacity, d_edges, d_edge_counts, edge_capacity, d_meas7, d_info36, d_edge_weight,
                          d_fixed, lambda0, step_eps, cg_tol, iters, cg_iters, d_poses7_out, d_stats, d_edge_residuals, d_edge_energy);
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": n must be >= 1");
    vors_status st = pg_refusals(who, call);
    if (st != VORS_OK) return st;
    if (!d_workspace) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": d_workspace is NULL (the pass allocates nothing: vors_pose_graph_workspace_bytes)");
    if ((st = stride_refusal(who, "pose_stride_bytes", pose_stride_bytes, 28, OPERATOR_STRIDE_LIMIT)) != VORS_OK) return st;
    if ((uintptr_t)d_workspace % 16 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": d_workspace must be 16-byte aligned");
    if ((st = require_device()) != VORS_OK) return st;
    call.pose_stride = stride_words(pose_stride_bytes, 7);
    pg_workspace_carve(&call, d_workspace, n, node_capacity, edge_capacity);
    launch_pose_graph(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

// The loop of ONE graph on the host: the kernels of pose_graph_kernels.hip in their launch order, each a plain loop.
static void pg_host_loop(const PgCall& c) {
    const uint32_t nodes = std::min<uint32_t>(c.node_counts[0], (uint32_t)c.node_capacity), edges = std::min<uint32_t>(c.edge_counts[0], (uint32_t)c.edge_capacity);
    const uint32_t nchunks = (nodes + (VORS_PG_CHUNK - 1)) / VORS_PG_CHUNK, echunks = (edges + (VORS_PG_CHUNK - 1)) / VORS_PG_CHUNK;
    auto weight_of = [&](uint32_t e) { return c.weight ? c.weight[e] : 1.0f; };
    auto info_of = [&](uint32_t e) { return c.info ? c.info + (size_t)e * 36 : nullptr; };
    // BEGIN .. RANK: validity, classes, the incidence lists in ascending edge index
    PgState st{};
    st.status = PG_ITERATIONS;
    st.lambda = c.lambda0;
    std::vector<float> poses[2];
    poses[0].assign((size_t)nodes * 7, 0.0f);
    poses[1].assign((size_t)nodes * 7, 0.0f);
    for (size_t k = 0; k < (size_t)nodes * 7; ++k) poses[0][k] = c.poses_in[k];
    std::vector<uint8_t> ok(edges);
    std::vector<std::vector<uint32_t>> inc(nodes);
    for (uint32_t e = 0; e < edges; ++e) {
        const uint32_t i = c.edges[2 * (size_t)e], j = c.edges[2 * (size_t)e + 1];
        ok[e] = pg_edge_valid(i, j, nodes, weight_of(e), c.meas + (size_t)e * 7, info_of(e)) ? 1 : 0;
        if (!ok[e]) continue;
        st.valid_edges += 1u;
        inc[i].push_back(e << 1);
        inc[j].push_back((e << 1) | 1u);
    }
    st.skipped_edges = edges - st.valid_edges;
    std::vector<uint32_t> cls(nodes);
    for (uint32_t k = 0; k < nodes; ++k) {
        const bool fixed = c.fixed ? c.fixed[k] != 0 : k == 0;
        cls[k] = fixed ? PG_NODE_FIXED : (inc[k].empty() ? PG_NODE_ISOLATED : PG_NODE_FREE);
        (cls[k] == PG_NODE_FREE ? st.free_nodes : cls[k] == PG_NODE_FIXED ? st.fixed_nodes : st.isolated_nodes) += 1u;
    }
    if (st.valid_edges == 0u || st.free_nodes == 0u) {
        st.status = PG_TOO_FEW;
        st.frozen = 1u;
    }
    // ENERGY at one of the two pose buffers; final: the per-edge outputs as well
    std::vector<float> slots(VORS_PG_CHUNK);
    auto energy_at = [&](uint32_t which, bool final) {
        const float* p = poses[which].data();
        const float nan = nanf("");
        float sum = 0.0f;
        for (uint32_t chunk = 0; chunk < echunks; ++chunk) {
            for (uint32_t s = 0; s < VORS_PG_CHUNK; ++s) {
                const uint32_t e = chunk * VORS_PG_CHUNK + s;
                slots[s] = 0.0f;
                if (e >= edges) continue;
                float r[6], energy = 0.0f;
                if (ok[e]) {
                    float om[36];
                    pg_load_info(info_of(e), om);
                    Iso err;
                    pg_edge_error(iso_load(p + (size_t)c.edges[2 * (size_t)e] * 7), iso_load(p + (size_t)c.edges[2 * (size_t)e + 1] * 7),
                                  iso_load(c.meas + (size_t)e * 7), &err, r);
                    energy = pg_edge_energy(r, om, weight_of(e));
                    slots[s] = energy;
                }
                if (final && c.edge_residuals)
                    for (int k = 0; k < 6; ++k) c.edge_residuals[(size_t)e * 6 + k] = ok[e] ? r[k] : nan;
                if (final && c.edge_energy) c.edge_energy[e] = ok[e] ? energy : nan;
            }
            const float v = pg_chunk_tree(slots.data());
            sum = chunk == 0 ? v : sum + v;
        }
        return sum;
    };
    st.energy = st.initial_energy = energy_at(st.cur, false);
    std::vector<float> wmat((size_t)edges * 36), lin((size_t)edges * VORS_PG_LIN), hd((size_t)nodes * 21), fac((size_t)nodes * 21);
    std::vector<float> x((size_t)nodes * 6, 0.0f), r((size_t)nodes * 6, 0.0f), z((size_t)nodes * 6, 0.0f), q((size_t)nodes * 6, 0.0f), p[2];
    p[0].assign((size_t)nodes * 6, 0.0f);
    p[1].assign((size_t)nodes * 6, 0.0f);
    std::vector<double> dslots(VORS_PG_CHUNK), dot_pq(nchunks), dot_rz[2], dot_rr[2], dot_rr0(nchunks);
    for (int b = 0; b < 2; ++b) {
        dot_rz[b].assign(nchunks, 0.0);
        dot_rr[b].assign(nchunks, 0.0);
    }
    auto sum_chunks = [&](const std::vector<double>& part) {
        double s = nchunks > 0 ? part[0] : 0.0;
        for (uint32_t ch = 1; ch < nchunks; ++ch) s = s + part[ch];
        return s;
    };
    // one dot product's chunk sums: share(k) for the free nodes, 0.0 for the others and beyond the count
    auto node_dots = [&](std::vector<double>& part, auto share) {
        for (uint32_t chunk = 0; chunk < nchunks; ++chunk) {
            for (uint32_t s = 0; s < VORS_PG_CHUNK; ++s) {
                const uint32_t k = chunk * VORS_PG_CHUNK + s;
                dslots[s] = k < nodes && cls[k] == PG_NODE_FREE ? share(k) : 0.0;
            }
            part[chunk] = pg_chunk_tree(dslots.data());
        }
    };
    for (int it = 0; it < c.iters; ++it) {
        if (st.frozen) break;
        const float* cur = poses[st.cur].data();
        if (!st.lin_ok)  // LINEARISE
            for (uint32_t e = 0; e < edges; ++e) {
                if (!ok[e]) continue;
                float om[36];
                pg_load_info(info_of(e), om);
                pg_edge_linearise(iso_load(cur + (size_t)c.edges[2 * (size_t)e] * 7), iso_load(cur + (size_t)c.edges[2 * (size_t)e + 1] * 7),
                                  iso_load(c.meas + (size_t)e * 7), om, weight_of(e), wmat.data() + (size_t)e * 36, lin.data() + (size_t)e * VORS_PG_LIN);
            }
        // GATHER
        for (uint32_t k = 0; k < nodes; ++k) {
            if (cls[k] != PG_NODE_FREE) continue;
            float h[21], gk[6], rk[6];
            for (size_t s = 0; s < inc[k].size(); ++s) {
                const uint32_t key = inc[k][s];
                const float* le = lin.data() + (size_t)(key >> 1) * VORS_PG_LIN + (key & 1u) * 21;
                const float* ge = lin.data() + (size_t)(key >> 1) * VORS_PG_LIN + 42 + (key & 1u) * 6;
                for (int m = 0; m < 21; ++m) h[m] = s == 0 ? le[m] : h[m] + le[m];
                for (int m = 0; m < 6; ++m) gk[m] = s == 0 ? ge[m] : gk[m] + ge[m];
            }
            if (!pg_node_factor(h, st.lambda, hd.data() + (size_t)k * 21, fac.data() + (size_t)k * 21)) st.singular = 1u;
            for (int m = 0; m < 6; ++m) rk[m] = -gk[m];
            pg_factor_solve(fac.data() + (size_t)k * 21, rk, z.data() + (size_t)k * 6);
            for (int m = 0; m < 6; ++m) {
                r[(size_t)k * 6 + m] = rk[m];
                x[(size_t)k * 6 + m] = 0.0f;
                p[1][(size_t)k * 6 + m] = 0.0f;
            }
        }
        node_dots(dot_rz[0], [&](uint32_t k) { return pg_dot6(r.data() + (size_t)k * 6, z.data() + (size_t)k * 6); });
        node_dots(dot_rr[0], [&](uint32_t k) { return pg_dot6(r.data() + (size_t)k * 6, r.data() + (size_t)k * 6); });
        dot_rr0 = dot_rr[0];
        if (st.singular) {  // VERDICT's first branch
            st.status = PG_SINGULAR;
            st.frozen = 1u;
            break;
        }
        for (int t = 0; t < c.cg_iters; ++t) {
            const uint32_t tc = (uint32_t)t & 1u, tp = tc ^ 1u;
            // CG A
            const bool done = st.cg_done[tp] != 0u || pg_cg_reached(sum_chunks(dot_rr[tc]), sum_chunks(dot_rr0), c.cg_tol);
            st.cg_done[tc] = done ? 1u : 0u;
            if (done) continue;
            const float beta = t > 0 ? pg_cg_beta(sum_chunks(dot_rz[tc]), sum_chunks(dot_rz[tp])) : 0.0f;
            for (uint32_t k = 0; k < nodes; ++k) {
                if (cls[k] != PG_NODE_FREE) continue;
                float pk[6], y[6];
                pg_cg_direction(z.data() + (size_t)k * 6, beta, p[tp].data() + (size_t)k * 6, pk);
                for (int m = 0; m < 6; ++m) p[tc][(size_t)k * 6 + m] = pk[m];
                pg_matvec_own(hd.data() + (size_t)k * 21, pk, y);
                for (uint32_t key : inc[k]) {
                    const uint32_t e = key >> 1, side = key & 1u, other = c.edges[2 * (size_t)e + (side ^ 1u)];
                    float d[6];
                    pg_cg_direction(z.data() + (size_t)other * 6, beta, p[tp].data() + (size_t)other * 6, d);
                    pg_matvec_edge(wmat.data() + (size_t)e * 36, side != 0u, d, y);
                }
                for (int m = 0; m < 6; ++m) q[(size_t)k * 6 + m] = y[m];
            }
            node_dots(dot_pq, [&](uint32_t k) { return pg_dot6(p[tc].data() + (size_t)k * 6, q.data() + (size_t)k * 6); });
            // CG B
            const float alpha = pg_cg_alpha(sum_chunks(dot_rz[tc]), sum_chunks(dot_pq));
            st.cg_spent += 1u;
            for (uint32_t k = 0; k < nodes; ++k) {
                if (cls[k] != PG_NODE_FREE) continue;
                for (int m = 0; m < 6; ++m) {
                    x[(size_t)k * 6 + m] = x[(size_t)k * 6 + m] + alpha * p[tc][(size_t)k * 6 + m];
                    r[(size_t)k * 6 + m] = r[(size_t)k * 6 + m] - alpha * q[(size_t)k * 6 + m];
                }
                pg_factor_solve(fac.data() + (size_t)k * 21, r.data() + (size_t)k * 6, z.data() + (size_t)k * 6);
            }
            node_dots(dot_rz[tp], [&](uint32_t k) { return pg_dot6(r.data() + (size_t)k * 6, z.data() + (size_t)k * 6); });
            node_dots(dot_rr[tp], [&](uint32_t k) { return pg_dot6(r.data() + (size_t)k * 6, r.data() + (size_t)k * 6); });
        }
        // CANDIDATE
        float* cand = poses[st.cur ^ 1u].data();
        float d2max = 0.0f;
        for (uint32_t k = 0; k < nodes; ++k) {
            if (cls[k] != PG_NODE_FREE) {
                for (int m = 0; m < 7; ++m) cand[(size_t)k * 7 + m] = cur[(size_t)k * 7 + m];
                continue;
            }
            iso_store(pg_candidate(iso_load(cur + (size_t)k * 7), x.data() + (size_t)k * 6), cand + (size_t)k * 7);
            const float d2 = pg_step2(x.data() + (size_t)k * 6);
            if (d2 > d2max) d2max = d2;  // (a NaN is left out)
        }
        // ENERGY at the candidates, VERDICT
        const float energy = energy_at(st.cur ^ 1u, false);
        const bool accepted = pg_accepts(energy, st.energy);
        st.lambda = pg_lambda_after(accepted, st.lambda);
        if (accepted) {
            st.cur ^= 1u;
            st.energy = energy;
            st.accepted += 1u;
            st.last_step_norm = sqrtf(d2max);
            st.lin_ok = 0u;
            if (d2max <= c.step_eps * c.step_eps) {
                st.status = PG_CONVERGED;
                st.frozen = 1u;
            }
        } else {
            st.rejected += 1u;
            st.lin_ok = 1u;
        }
        st.cg_done[0] = st.cg_done[1] = 0u;
    }
    // the final ENERGY, FINISH
    const float final_energy = energy_at(st.cur, true);
    for (size_t k = 0; k < (size_t)nodes * 7; ++k) c.poses_out[k] = poses[st.cur][k];
    if (c.stats)
        *c.stats = vors_pose_graph_stats{st.status,     st.accepted,       st.rejected,       st.cg_spent,  st.valid_edges,    st.skipped_edges, st.free_nodes,
                                         st.fixed_nodes, st.isolated_nodes, st.initial_energy, final_energy, st.last_step_norm, st.lambda};
}

vors_status vors_pose_graph_optimize_host(const float* poses7_in, uint32_t node_count, int node_capacity, const uint32_t* edges, uint32_t edge_count,
                                          int edge_capacity, const float* meas7, const float* info36, const float* edge_weight, const uint8_t* fixed,
                                          float lambda0, float step_eps, float cg_tol, int iters, int cg_iters, float* poses7_out,
                                          vors_pose_graph_stats* stats, float* edge_residuals, float* edge_energy) {
    const PgCall call = pg_call(1, poses7_in, &node_count, node_capacity, edges, &edge_count, edge_capacity, meas7, info36, edge_weight, fixed, lambda0,
                                step_eps, cg_tol, iters, cg_iters, poses7_out, stats, edge_residuals, edge_energy);
    const vors_status st = pg_refusals("pose_graph_optimize_host", call);
    if (st != VORS_OK) return st;
    pg_host_loop(call);
    return VORS_OK;
}

void vors_pose_graph_jacobians_host(const float ti7[7], const float tj7[7], const float meas7[7], float r6[6], float ji36[36], float jj36[36]) {
    pg_edge_jacobians(iso_load(ti7), iso_load(tj7), iso_load(meas7), r6, ji36, jj36);
}

// ---------------------------------------------------------------------------------------------------------------
// Loop closure (vors_loop_signatures, vors_loop_candidates, vors_loop_verify_edges and their host twins; include/vors_hip.h 2h): per
// entry the refusals both forms share, the device entry (loop_closure_kernels.hip) and the host entry, which runs the kernels' own texts
// (lie.h lc_*) as plain loops.
// ---------------------------------------------------------------------------------------------------------------
static_assert(sizeof(LcMeta) == sizeof(vors_loop_sig_meta) && sizeof(LcCand) == sizeof(vors_loop_candidate), "records of the C ABI");
static_assert(VORS_LC_MAX_K == VORS_LOOP_MAX_K && VORS_LC_COUNTS == VORS_LOOP_COUNTS && VORS_LC_VERDICTS == VORS_LOOP_VERDICTS &&
                  LC_CAPACITY == VORS_LOOP_CAPACITY && LC_PRIOR_ROT == VORS_LOOP_PRIOR_ROT && LC_NONFINITE == VORS_LOOP_NONFINITE,
              "lie.h and the header state the same codes");

static vors_status lc_thumbnail_refusal(const std::string& w, int d) {
    if (d < 64 || d > 1024 || d % 64 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": D must be a multiple of 64 in 64..1024");
    return VORS_OK;
}

static vors_status lc_sig_refusals(const char* who, const LcSigCall& c) {
    const std::string w(who);
    if (!c.gray || !c.sig || !c.meta) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the planes, the signatures or their meta records are NULL");
    if (c.tr < 1 || c.tc < 1 || c.tr > 1024 || c.tc > 1024) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": tr and tc must be in 1..1024");
    const vors_status st = lc_thumbnail_refusal(w, c.tr * c.tc);
    if (st != VORS_OK) return st;
    if (c.rows < c.tr || c.cols < c.tc) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows >= tr and cols >= tc are required");
    if (c.rows > 65535 || c.cols > 65535 || (int64_t)c.rows * c.cols > (1 << 28))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": rows and cols must not exceed 65535, rows * cols not 2^28");
    if ((uintptr_t)c.sig % 16 != 0 || (uintptr_t)c.meta % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the signatures must be 16-byte aligned, their meta records 4-byte aligned");
    return VORS_OK;
}

vors_status vors_loop_signatures(int n, const uint8_t* d_gray, int rows, int cols, int tr, int tc, int8_t* d_sig, vors_loop_sig_meta* d_sig_meta,
                                 void* hip_stream) {
    const char* who = "loop_signatures";
    const LcSigCall call{n, rows, cols, tr, tc, d_gray, d_sig, reinterpret_cast<LcMeta*>(d_sig_meta)};
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": n must be >= 1");
    vors_status st = lc_sig_refusals(who, call);
    if (st != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    launch_loop_signatures(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_loop_signatures_host(const uint8_t* gray, int rows, int cols, int tr, int tc, int8_t* sig, vors_loop_sig_meta* sig_meta) {
    const LcSigCall c{1, rows, cols, tr, tc, gray, sig, reinterpret_cast<LcMeta*>(sig_meta)};
    const vors_status st = lc_sig_refusals("loop_signatures_host", c);
    if (st != VORS_OK) return st;
    const uint32_t R = (uint32_t)rows, C = (uint32_t)cols, TR = (uint32_t)tr, TC = (uint32_t)tc;
    LcMeta meta{0, 0u};
    for (uint32_t cy = 0; cy < TR; ++cy)
        for (uint32_t cx = 0; cx < TC; ++cx) {
            const uint32_t y0 = lc_cell_begin(cy, R, TR), y1 = lc_cell_begin(cy + 1u, R, TR), x0 = lc_cell_begin(cx, C, TC), x1 = lc_cell_begin(cx + 1u, C, TC);
            uint64_t sum = 0;
            for (uint32_t y = y0; y < y1; ++y)
                for (uint32_t x = x0; x < x1; ++x) sum += gray[(size_t)y * C + x];
            const int8_t s = lc_cell_value(sum, (uint64_t)(y1 - y0) * (x1 - x0));
            sig[cy * TC + cx] = s;
            meta.sum += (int32_t)s;
            meta.sumsq += (uint32_t)((int32_t)s * (int32_t)s);
        }
    *c.meta = meta;
    return VORS_OK;
}

static vors_status lc_cand_refusals(const char* who, const LcCandCall& c, int k) {
    const std::string w(who);
    if (!c.sig || !c.meta || !c.counts_in) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the signatures, their meta records or the counts are NULL");
    if (!c.cand || !c.cand_counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the candidate lists or their counts are NULL");
    if (c.capacity < 1 || c.capacity > (1 << 20)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": capacity must be in 1..2^20");
    const vors_status st = lc_thumbnail_refusal(w, c.d);
    if (st != VORS_OK) return st;
    if (c.min_gap < 1u) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": min_gap must be >= 1");
    if (k < 1 || k > VORS_LOOP_MAX_K) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": k must be in 1..VORS_LOOP_MAX_K (8)");
    if (!(c.max_dist_m >= 0.0f) || !(c.min_qdot >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": max_dist_m and min_qdot must be >= 0 (and not NaN)");
    if ((uintptr_t)c.sig % 16 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the signatures must be 16-byte aligned");
    if ((uintptr_t)c.meta % 4 != 0 || (uintptr_t)c.counts_in % 4 != 0 || (uintptr_t)c.poses % 4 != 0 || (uintptr_t)c.query_first % 4 != 0 ||
        (uintptr_t)c.cand % 4 != 0 || (uintptr_t)c.cand_counts % 4 != 0 || (uintptr_t)c.counts % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the meta records, counts, poses, lists and their counts must be 4-byte aligned");
    return VORS_OK;
}

vors_status vors_loop_candidates(int n, const int8_t* d_sig, const vors_loop_sig_meta* d_sig_meta, const uint32_t* d_counts_in, int capacity, int D,
                                 const void* d_poses7, size_t pose_stride_bytes, const uint32_t* d_query_first, uint32_t min_gap, int k,
                                 float min_score, float max_dist_m, float min_qdot, vors_loop_candidate* d_cand, uint32_t* d_cand_counts,
                                 uint32_t* d_counts, void* hip_stream) {
    const char* who = "loop_candidates";
    LcCandCall call{n, capacity, D, d_sig, reinterpret_cast<const LcMeta*>(d_sig_meta), d_counts_in, static_cast<const float*>(d_poses7), 7,
                    d_query_first, min_gap, (uint32_t)k, min_score, max_dist_m, min_qdot, reinterpret_cast<LcCand*>(d_cand), d_cand_counts, d_counts};
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": n must be >= 1");
    vors_status st = lc_cand_refusals(who, call, k);
    if (st != VORS_OK) return st;
    if ((st = stride_refusal(who, "pose_stride_bytes", pose_stride_bytes, 28, OPERATOR_STRIDE_LIMIT)) != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    call.pose_stride = stride_words(pose_stride_bytes, 7);
    HIP_TRY(launch_loop_candidates(call, static_cast<hipStream_t>(hip_stream)));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_loop_candidates_host(const int8_t* sig, const vors_loop_sig_meta* sig_meta, uint32_t count, int capacity, int D, const float* poses7,
                                      uint32_t query_first, uint32_t min_gap, int k, float min_score, float max_dist_m, float min_qdot,
                                      vors_loop_candidate* cand, uint32_t* cand_counts, uint32_t counts[VORS_LOOP_COUNTS]) {
    const LcCandCall c{1, capacity, D, sig, reinterpret_cast<const LcMeta*>(sig_meta), &count, poses7, 7, &query_first, min_gap, (uint32_t)k,
                       min_score, max_dist_m, min_qdot, reinterpret_cast<LcCand*>(cand), cand_counts, counts};
    const vors_status st = lc_cand_refusals("loop_candidates_host", c, k);
    if (st != VORS_OK) return st;
    const uint32_t n = std::min<uint32_t>(count, (uint32_t)capacity);
    uint32_t tally[VORS_LC_COUNTS] = {0u, 0u, 0u, 0u, 0u};
    std::vector<int64_t> va(n);
    std::vector<double> root(n);
    for (uint32_t r = 0; r < n; ++r) {
        va[r] = lc_variance(D, c.meta[r].sum, c.meta[r].sumsq);
        root[r] = lc_root(va[r]);
    }
    for (uint32_t j = query_first; j < n; ++j) {
        uint32_t idx[VORS_LC_MAX_K], have = 0u;
        float score[VORS_LC_MAX_K];
        for (int p = 0; p < VORS_LC_MAX_K; ++p) {
            idx[p] = VORS_LC_EMPTY;
            score[p] = 0.0f;
        }
        for (uint32_t i = 0; (uint64_t)i + min_gap <= (uint64_t)j; ++i) {
            tally[0] += 1u;
            if (va[i] == 0 || va[j] == 0) {
                tally[1] += 1u;
                continue;
            }
            if (poses7 && !lc_pose_passes(poses7 + (size_t)i * 7, poses7 + (size_t)j * 7, max_dist_m, min_qdot)) {
                tally[2] += 1u;
                continue;
            }
            int32_t dot = 0;
            for (int e = 0; e < D; ++e) dot += (int32_t)sig[(size_t)i * D + e] * (int32_t)sig[(size_t)j * D + e];
            const float s = lc_score(lc_numerator(D, dot, c.meta[i].sum, c.meta[j].sum), root[i], root[j]);
            if (!lc_score_passes(s, min_score)) {
                tally[3] += 1u;
                continue;
            }
            tally[4] += 1u;
            lc_topk_insert(idx, score, &have, (uint32_t)k, i, s);
        }
        for (int p = 0; p < k; ++p) c.cand[(size_t)j * k + p] = LcCand{idx[p], score[p]};
        cand_counts[j] = have;
    }
    if (counts)
        for (int p = 0; p < VORS_LC_COUNTS; ++p) counts[p] = tally[p];
    return VORS_OK;
}

static vors_status lc_verify_refusals(const char* who, const LcVerifyCall& c, int edge_capacity, size_t fwd_bytes, size_t bwd_bytes, size_t pose_bytes) {
    const std::string w(who);
    if (c.m < 1u || c.m > (1u << 28)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": m must be in 1..2^28");
    if (!c.pairs || !c.fwd || !c.status_fwd) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the pairs, the forward models or their statuses are NULL");
    if (!c.edges || !c.meas || !c.edge_count || !c.verdict)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the edges, their measurements, the edge count or the verdicts are NULL");
    if (edge_capacity < 1 || edge_capacity > (1 << 28)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": edge_capacity must be in 1..2^28");
    vors_status st;
    if ((st = stride_refusal(who, "fwd_stride_bytes", fwd_bytes, 28, OPERATOR_STRIDE_LIMIT)) != VORS_OK) return st;
    if ((st = stride_refusal(who, "bwd_stride_bytes", bwd_bytes, 28, OPERATOR_STRIDE_LIMIT)) != VORS_OK) return st;
    if ((st = stride_refusal(who, "pose_stride_bytes", pose_bytes, 28, OPERATOR_STRIDE_LIMIT)) != VORS_OK) return st;
    if (!(c.max_cycle_trans >= 0.0f) || !(c.max_cycle_rot >= 0.0f) || !(c.max_prior_trans >= 0.0f) || !(c.max_prior_rot >= 0.0f))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the four bounds must be >= 0 (and not NaN)");
    if (!(pg_finite(c.weight) && c.weight > 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": weight must be finite and > 0");
    if ((uintptr_t)c.pairs % 4 != 0 || (uintptr_t)c.fwd % 4 != 0 || (uintptr_t)c.bwd % 4 != 0 || (uintptr_t)c.status_fwd % 4 != 0 ||
        (uintptr_t)c.status_bwd % 4 != 0 || (uintptr_t)c.info % 4 != 0 || (uintptr_t)c.poses % 4 != 0 || (uintptr_t)c.edges % 4 != 0 ||
        (uintptr_t)c.meas % 4 != 0 || (uintptr_t)c.info_out % 4 != 0 || (uintptr_t)c.edge_weight % 4 != 0 || (uintptr_t)c.edge_count % 4 != 0 ||
        (uintptr_t)c.verdict % 4 != 0 || (uintptr_t)c.residuals % 4 != 0 || (uintptr_t)c.counts % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": every pointer must be 4-byte aligned");
    return VORS_OK;
}

static LcVerifyCall lc_verify_call(uint32_t m, const uint32_t* pairs, const void* model_fwd, size_t fwd_stride_bytes, const void* model_bwd,
                                   size_t bwd_stride_bytes, const int32_t* status_fwd, const int32_t* status_bwd, const float* info36,
                                   const void* poses7, size_t pose_stride_bytes, uint32_t node_count, float max_cycle_trans, float max_cycle_rot,
                                   float max_prior_trans, float max_prior_rot, float weight, uint32_t* edges, float* meas7, float* info36_out,
                                   float* edge_weight, uint32_t* edge_count, int edge_capacity, uint32_t* verdict, float* residuals, uint32_t* counts) {
    LcVerifyCall c{};
    c.m = m; c.pairs = pairs;
    c.fwd = static_cast<const float*>(model_fwd); c.bwd = static_cast<const float*>(model_bwd);
    c.fwd_stride = stride_words(fwd_stride_bytes, 7); c.bwd_stride = stride_words(bwd_stride_bytes, 7);
    c.status_fwd = status_fwd; c.status_bwd = status_bwd; c.info = info36;
    c.poses = static_cast<const float*>(poses7); c.pose_stride = stride_words(pose_stride_bytes, 7); c.node_count = node_count;
    c.max_cycle_trans = max_cycle_trans; c.max_cycle_rot = max_cycle_rot; c.max_prior_trans = max_prior_trans; c.max_prior_rot = max_prior_rot;
    c.weight = weight;
    c.edges = edges; c.meas = meas7; c.info_out = info36_out; c.edge_weight = edge_weight; c.edge_count = edge_count;
    c.edge_capacity = edge_capacity > 0 ? (uint32_t)edge_capacity : 0u;
    c.verdict = verdict; c.residuals = residuals; c.counts = counts;
    return c;
}

vors_status vors_loop_verify_edges(uint32_t m, const uint32_t* d_pairs, const void* d_model_fwd, size_t fwd_stride_bytes, const void* d_model_bwd,
                                   size_t bwd_stride_bytes, const int32_t* d_status_fwd, const int32_t* d_status_bwd, const float* d_info36,
                                   const void* d_poses7, size_t pose_stride_bytes, uint32_t node_count, float max_cycle_trans, float max_cycle_rot,
                                   float max_prior_trans, float max_prior_rot, float weight, uint32_t* d_edges, float* d_meas7, float* d_info36_out,
                                   float* d_edge_weight, uint32_t* d_edge_count, int edge_capacity, uint32_t* d_verdict, float* d_residuals,
                                   uint32_t* d_counts, void* hip_stream) {
    const char* who = "loop_verify_edges";
    const LcVerifyCall call = lc_verify_call(m, d_pairs, d_model_fwd, fwd_stride_bytes, d_model_bwd, bwd_stride_bytes, d_status_fwd, d_status_bwd,
                                             d_info36, d_poses7, pose_stride_bytes, node_count, max_cycle_trans, max_cycle_rot, max_prior_trans,
                                             max_prior_rot, weight, d_edges, d_meas7, d_info36_out, d_edge_weight, d_edge_count, edge_capacity,
                                             d_verdict, d_residuals, d_counts);
    vors_status st = lc_verify_refusals(who, call, edge_capacity, fwd_stride_bytes, bwd_stride_bytes, pose_stride_bytes);
    if (st != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    launch_loop_verify(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_loop_verify_edges_host(uint32_t m, const uint32_t* pairs, const void* model_fwd, size_t fwd_stride_bytes, const void* model_bwd,
                                        size_t bwd_stride_bytes, const int32_t* status_fwd, const int32_t* status_bwd, const float* info36,
                                        const void* poses7, size_t pose_stride_bytes, uint32_t node_count, float max_cycle_trans, float max_cycle_rot,
                                        float max_prior_trans, float max_prior_rot, float weight, uint32_t* edges, float* meas7, float* info36_out,
                                        float* edge_weight, uint32_t* edge_count, int edge_capacity, uint32_t* verdict, float* residuals,
                                        uint32_t* counts) {
    const LcVerifyCall c = lc_verify_call(m, pairs, model_fwd, fwd_stride_bytes, model_bwd, bwd_stride_bytes, status_fwd, status_bwd, info36, poses7,
                                          pose_stride_bytes, node_count, max_cycle_trans, max_cycle_rot, max_prior_trans, max_prior_rot, weight, edges,
                                          meas7, info36_out, edge_weight, edge_count, edge_capacity, verdict, residuals, counts);
    const vors_status st = lc_verify_refusals("loop_verify_edges_host", c, edge_capacity, fwd_stride_bytes, bwd_stride_bytes, pose_stride_bytes);
    if (st != VORS_OK) return st;
    uint32_t tally[VORS_LC_VERDICTS] = {};
    uint32_t at = std::min<uint32_t>(c.edge_count[0], c.edge_capacity);
    for (uint32_t e = 0; e < m; ++e) {
        const uint32_t i = pairs[2 * (size_t)e], j = pairs[2 * (size_t)e + 1];
        const float* fwd = c.fwd + (size_t)e * c.fwd_stride;
        const float* info = c.info ? c.info + (size_t)e * 36 : nullptr;
        const bool status_ok = status_fwd[e] == VORS_TRACK_OK && (!status_bwd || status_bwd[e] == VORS_TRACK_OK);
        float r12[12];
        uint32_t v = lc_verify(i, j, status_ok, fwd, c.bwd ? c.bwd + (size_t)e * c.bwd_stride : nullptr, info, c.poses, c.pose_stride, node_count,
                               max_cycle_trans, max_cycle_rot, max_prior_trans, max_prior_rot, r12);
        if (v == LC_ACCEPTED) {
            if (at < c.edge_capacity) {
                edges[2 * (size_t)at] = i;
                edges[2 * (size_t)at + 1] = j;
                for (int k = 0; k < 7; ++k) meas7[(size_t)at * 7 + k] = fwd[k];
                if (info36_out)
                    for (int k = 0; k < 36; ++k) info36_out[(size_t)at * 36 + k] = info ? info[k] : (k % 7 == 0 ? 1.0f : 0.0f);
                if (edge_weight) edge_weight[at] = weight;
                at += 1u;
            } else {
                v = LC_CAPACITY;
            }
        }
        verdict[e] = v;
        if (residuals)
            for (int k = 0; k < 12; ++k) residuals[(size_t)e * 12 + k] = r12[k];
        tally[v] += 1u;
    }
    c.edge_count[0] = at;
    if (counts)
        for (int k = 0; k < VORS_LC_VERDICTS; ++k) counts[k] = tally[k];
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The map ICP correction at keyframe promotion (vors_trackers_enable_map_icp, trackers.cpp): what it refuses of its parameters — one
// sentence each, shared by the enable entries and the host twins — the verdict's thresholds as the rule reads them, and the two host
// twins, which run lie.h map_icp_window / map_icp_verdict, the kernels' own texts.
// ---------------------------------------------------------------------------------------------------------------
static vors_status map_icp_verdict_refusals(const std::string& w, const vors_map_icp_params& p) {
    if (!(p.min_match_ratio >= 0.0f && p.min_match_ratio <= 1.0f))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": min_match_ratio must lie in [0, 1] (and not be NaN)");
    if (!(p.max_rms >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": max_rms must be >= 0 (and not NaN)");
    if (!(p.max_trans_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": max_trans_m must be >= 0 (and not NaN)");
    if (!(p.max_rot_rad >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": max_rot_rad must be >= 0 (and not NaN)");
    return VORS_OK;
}
vors_status map_icp_params_refusals(const char* who, const vors_map_icp_params* p) {
    const std::string w(who);
    if (!p) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": params is NULL");
    // (what vors_icp_points_robust refuses of the shared parameters, in its own sentences: the lists, planes and shapes are the handle's)
    alignas(16) static float some[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    vors_status st = icp_refusals(who, icp_args(1, some, some, nullptr, 1, nullptr, 0, some, 0, reinterpret_cast<const uint16_t*>(some), some, 1, 1, 1.0f,
                                                p->dist_m, p->damping, p->step_eps, p->iters, p->min_points, nullptr, some, nullptr, nullptr, nullptr));
    if (st != VORS_OK) return st;
    if ((st = icp_robust_refusals(who, IcpRobust{nullptr, p->min_cos, p->huber_m, nullptr})) != VORS_OK) return st;
    if (p->last_keyframes < 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": last_keyframes must be >= 0 (0 = the whole map)");
    return map_icp_verdict_refusals(w, *p);
}
MapIcpGates map_icp_gates(const vors_map_icp_params& p) {
    return MapIcpGates{p.min_match_ratio, p.max_rms, p.max_trans_m, cosf(0.5f * p.max_rot_rad)};
}

vors_status vors_map_icp_window_host(const vors_map_segment* segments, uint32_t n_segments, int max_keyframes, uint32_t count, int capacity,
                                     int last_keyframes, uint32_t range2[2]) {
    if (!range2) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_window_host: range2 is NULL");
    if (capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_window_host: capacity must be >= 1");
    if (max_keyframes < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_window_host: max_keyframes must be >= 1");
    if (last_keyframes < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_window_host: last_keyframes must be >= 0 (0 = the whole map)");
    const uint32_t n_rec = n_segments < (uint32_t)max_keyframes ? n_segments : (uint32_t)max_keyframes;
    if (!segments && last_keyframes != 0 && n_rec > (uint32_t)last_keyframes)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_window_host: segments is NULL where a record is read");
    if ((uintptr_t)segments % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_window_host: segments must be 4-byte aligned");
    static_assert(sizeof(vors_map_segment) == MAP_SEGMENT_WORDS * 4 && offsetof(vors_map_segment, first) == 4, "lie.h map_icp_window's record");
    map_icp_window(reinterpret_cast<const uint32_t*>(segments), n_segments, max_keyframes, count, capacity, last_keyframes, range2);
    return VORS_OK;
}

vors_status vors_map_icp_verdict_host(const vors_map_icp_params* params, const vors_icp_stats* stats, const float pose_before[7],
                                      const float pose_after[7], uint32_t* verdict) {
    if (!params || !stats || !pose_before || !pose_after || !verdict)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_verdict_host: a NULL argument (params, stats, pose_before, pose_after, verdict)");
    vors_status st = map_icp_verdict_refusals("map_icp_verdict_host", *params);
    if (st != VORS_OK) return st;
    *verdict = (uint32_t)map_icp_verdict(map_icp_gates(*params), stats->status, stats->matched, stats->considered, stats->rms, pose_before, pose_after);
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The correction through the joint pass with the condition test (vors_trackers_enable_map_icp_joint, trackers.cpp): the
// refusals of its parameters, the conditioning measure on the host and on the device (lie.h icp_condition) and the verdict's host twin
// (lie.h map_icp_verdict_joint).
// ---------------------------------------------------------------------------------------------------------------
static vors_status map_icp_condition_refusals(const std::string& w, const vors_map_icp_joint_params& p) {
    if (!(p.max_dilution_t >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": max_dilution_t must be >= 0 (and not NaN; 0 = that bound is off)");
    if (!(p.max_dilution_r >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": max_dilution_r must be >= 0 (and not NaN; 0 = that bound is off)");
    return VORS_OK;
}
vors_status map_icp_joint_params_refusals(const char* who, const vors_map_icp_joint_params* p) {
    if (!p) return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": params is NULL");
    vors_status st = map_icp_params_refusals(who, &p->icp);
    if (st != VORS_OK) return st;
    // (what vors_icp_points_joint refuses of the two photo fields, in its own sentences: the grey levels are the handle's)
    static const uint8_t some[4] = {0, 0, 0, 0};
    if ((st = icp_joint_refusals(who, IcpJoint{some, some, p->photo_scale_m, p->photo_huber_grey, nullptr, nullptr})) != VORS_OK) return st;
    return map_icp_condition_refusals(who, *p);
}
float map_icp_photo_huber_m(const vors_map_icp_joint_params& p) { return icp_photo_huber_m(p.photo_scale_m, p.photo_huber_grey); }

vors_status vors_icp_condition_from_sums(const float sums29[29], float* dilution_t, float* dilution_r, int32_t* flags) {
    if (!sums29) return fail(VORS_ERR_INVALID_ARGUMENT, "icp_condition_from_sums: sums29 is NULL");
    const int fl = icp_condition(sums29, dilution_t, dilution_r);
    if (flags) *flags = fl;
    return VORS_OK;
}

vors_status vors_icp_condition(int n, const float* d_sums29, float* d_dilution2, int32_t* d_flags, void* hip_stream) {
    if (n < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "icp_condition: n must be >= 1");
    if (!d_sums29) return fail(VORS_ERR_INVALID_ARGUMENT, "icp_condition: d_sums29 is NULL");
    if (!d_dilution2) return fail(VORS_ERR_INVALID_ARGUMENT, "icp_condition: d_dilution2 is NULL");
    if ((uintptr_t)d_sums29 % 4 != 0 || (uintptr_t)d_dilution2 % 4 != 0 || (uintptr_t)d_flags % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, "icp_condition: d_sums29, d_dilution2 and d_flags must be 4-byte aligned");
    vors_status st = require_device();
    if (st != VORS_OK) return st;
    launch_icp_condition(d_sums29, n, d_dilution2, d_flags, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_map_icp_verdict_joint_host(const vors_map_icp_joint_params* params, const vors_icp_stats* stats, const float pose_before[7],
                                            const float pose_after[7], float dilution_t, float dilution_r, uint32_t* verdict) {
    if (!params || !stats || !pose_before || !pose_after || !verdict)
        return fail(VORS_ERR_INVALID_ARGUMENT, "map_icp_verdict_joint_host: a NULL argument (params, stats, pose_before, pose_after, verdict)");
    vors_status st = map_icp_verdict_refusals("map_icp_verdict_joint_host", params->icp);
    if (st != VORS_OK) return st;
    if ((st = map_icp_condition_refusals("map_icp_verdict_joint_host", *params)) != VORS_OK) return st;
    *verdict = map_icp_verdict_joint(map_icp_gates(params->icp), MapIcpConditionGates{params->max_dilution_t, params->max_dilution_r}, stats->status,
                                     stats->matched, stats->considered, stats->rms, pose_before, pose_after, dilution_t, dilution_r);
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Lie helpers (host arithmetic)
// ---------------------------------------------------------------------------------------------------------------
void vors_se3_exp(const float xi[6], float out_iso7[7]) { iso_store(se3_exp(xi), out_iso7); }
void vors_ref_sincos(const float* x, int n, float* sin_out, float* cos_out) {
    for (int i = 0; i < n; ++i) {
        if (sin_out) sin_out[i] = ref_sinf(x[i]);
        if (cos_out) cos_out[i] = ref_cosf(x[i]);
    }
}
void vors_se3_log(const float iso7[7], float out_xi[6]) { se3_log(iso_load(iso7), out_xi); }
void vors_so3_exp(const float w[3], float out_q4[4]) {
    const Quat q = so3_exp(w);
    out_q4[0] = q.i; out_q4[1] = q.j; out_q4[2] = q.k; out_q4[3] = q.w;
}
void vors_so3_log(const float q4[4], float out_w[3]) { so3_log(Quat{q4[0], q4[1], q4[2], q4[3]}, out_w); }
void vors_iso_mul(const float a7[7], const float b7[7], float out7[7]) { iso_store(iso_mul(iso_load(a7), iso_load(b7)), out7); }
void vors_iso_inverse(const float a7[7], float out7[7]) { iso_store(iso_inverse(iso_load(a7)), out7); }
void vors_to_depth(float scale, const float* idepth, int n, uint16_t* depth_out) {
    for (int i = 0; i < n; ++i) depth_out[i] = to_depth(scale, idepth[i]);
}
void vors_from_depth(float scale, const uint16_t* depth, int n, float* idepth_out) {
    for (int i = 0; i < n; ++i) idepth_out[i] = depth[i] ? scale / (float)depth[i] : nanf("");  // inverse_depth.rs:24-29, Unknown = NaN
}
// Camera::back_project / Camera::project (camera.rs:43-45, 36-39) for arrays: the texts the point-cloud kernel runs (lie.h back_project,
// iso_transform_point). A NULL pose is the identity and skips the transform, so the camera-frame bits come out untouched.
void vors_camera_back_project(const float cam5[5], const float pose7[7], const float* xy, const float* depth, int n, float* xyz_out) {
    const Intr k = intr_from_cam5(cam5);
    for (int i = 0; i < n; ++i) {
        V3 p = back_project(k, xy[2 * i], xy[2 * i + 1], depth[i]);
        if (pose7) p = iso_transform_point(iso_load(pose7), p);
        xyz_out[3 * i] = p.x; xyz_out[3 * i + 1] = p.y; xyz_out[3 * i + 2] = p.z;
    }
}
// The voxel keys of the keyframe map's voxel filter for arrays: lie.h voxel_key, the text the device kernels run. A voxel_m that no
// handle accepts (not finite, <= 0) gives no point a key.
void vors_voxel_keys(float voxel_m, const float* xyz, int n, uint64_t* keys_out) {
    const bool ok = voxel_m > 0.0f && voxel_m <= 3.4028234663852886e38f;
    for (int i = 0; i < n; ++i) keys_out[i] = ok ? voxel_key(voxel_m, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]) : VORS_VOXEL_NONE;
}
// The statistics of the map's voxels for ONE unfiltered list U (vors_trackers_enable_map_voxel_stats): what the device map of a sequence
// holds after the keyframes that make up U, by lie.h voxel_key / voxel_offset_q, the texts the device kernels run. Ranks are handed out
// in U's order of first occurrence of a key, which is the order of the filtered list.
vors_status vors_voxel_stats_host(const float* xyz, const uint8_t* gray, const uint32_t* segment_of, uint32_t n, float voxel_m, int capacity,
                                  uint32_t* total, uint32_t* first_index, int64_t* sums, uint32_t* obs) {
    if (n && (!xyz || !gray)) return fail(VORS_ERR_INVALID_ARGUMENT, "voxel_stats_host: a list (xyz, gray) is NULL");
    if (!sums || !obs) return fail(VORS_ERR_INVALID_ARGUMENT, "voxel_stats_host: sums or obs is NULL");
    if (!(voxel_m > 0.0f) || !(voxel_m <= 3.4028234663852886e38f))
        return fail(VORS_ERR_INVALID_ARGUMENT, "voxel_stats_host: voxel size voxel_m must be finite and > 0");
    if (capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "voxel_stats_host: capacity must be >= 1");
    std::memset(sums, 0, (size_t)capacity * 4 * sizeof(int64_t));
    std::memset(obs, 0, (size_t)capacity * 2 * sizeof(uint32_t));
    std::unordered_map<uint64_t, uint32_t> rank_of;    // key -> rank
    std::vector<uint32_t> first;                       // rank < capacity -> index in U of the voxel's first point
    uint32_t next = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float* w = xyz + 3 * (size_t)i;
        const uint64_t key = voxel_key(voxel_m, w[0], w[1], w[2]);
        if (key == VORS_VOXEL_NONE) continue;
        auto it = rank_of.find(key);
        if (it == rank_of.end()) {
            it = rank_of.emplace(key, next).first;
            if (next < (uint32_t)capacity) first.push_back(i);
            next += 1;
        }
        const uint32_t r = it->second;
        if (r >= (uint32_t)capacity) continue;
        const float* f = xyz + 3 * (size_t)first[r];
        for (int a = 0; a < 3; ++a) sums[4 * (size_t)r + a] += voxel_offset_q(voxel_m, w[a], f[a]);
        sums[4 * (size_t)r + 3] += gray[i];
        obs[2 * (size_t)r] += 1u;
        const uint32_t seg = segment_of ? segment_of[i] : 0u;
        if (seg > obs[2 * (size_t)r + 1]) obs[2 * (size_t)r + 1] = seg;
    }
    if (total) *total = next;
    if (first_index)
        for (size_t r = 0; r < first.size(); ++r) first_index[r] = first[r];
    return VORS_OK;
}

// The resolve of the statistics (vors_voxel_means, vors_voxel_means_host): the refusals both share, the device entry
// (product_kernels.hip voxel_means_kernel) and the host entry, which runs the kernel's own text (lie.h voxel_mean).
static vors_status voxel_means_refusals(const char* who, const void* xyz, const void* sums, const void* obs, float voxel_m, int capacity,
                                        uint32_t min_span, const void* first_segment, const void* xyz_mean, const void* gray_mean,
                                        const void* kept) {
    const std::string w(who);
    if (!xyz || !sums || !obs) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a list (xyz, sums, obs) is NULL");
    if (!xyz_mean && !gray_mean && !kept) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": no output at all (xyz_mean, gray_mean and kept are NULL)");
    if (!(voxel_m > 0.0f) || !(voxel_m <= 3.4028234663852886e38f))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": voxel size voxel_m must be finite and > 0");
    if (capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": capacity must be >= 1");
    if (!first_segment && min_span != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": min_span must be 0 without the first segment of every rank (there is no span to test)");
    if ((uintptr_t)sums % 8 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": sums must be 8-byte aligned");
    if ((uintptr_t)xyz % 4 != 0 || (uintptr_t)obs % 4 != 0 || (uintptr_t)first_segment % 4 != 0 || (uintptr_t)xyz_mean % 4 != 0 ||
        (uintptr_t)kept % 4 != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": xyz, obs, first_segment_of_rank, xyz_mean and kept must be 4-byte aligned");
    return VORS_OK;
}

vors_status vors_voxel_means(int n, const float* d_xyz, const uint32_t* d_list_counts, int capacity, const int64_t* d_sums, const uint32_t* d_obs,
                             float voxel_m, uint32_t min_count, uint32_t min_span, const uint32_t* d_first_segment_of_rank, float* d_xyz_mean,
                             uint8_t* d_gray_mean, uint32_t* d_kept, void* hip_stream) {
    if (n < 1 || n > 65535) return fail(VORS_ERR_INVALID_ARGUMENT, "voxel_means: n must be in 1..65535");
    if (!d_list_counts) return fail(VORS_ERR_INVALID_ARGUMENT, "voxel_means: a list (d_list_counts) is NULL");
    if ((uintptr_t)d_list_counts % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, "voxel_means: d_list_counts must be 4-byte aligned");
    vors_status st = voxel_means_refusals("voxel_means", d_xyz, d_sums, d_obs, voxel_m, capacity, min_span, d_first_segment_of_rank, d_xyz_mean,
                                          d_gray_mean, d_kept);
    if (st != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    VoxelMeansCall call{};
    call.n = n;
    call.xyz = d_xyz;
    call.list_counts = d_list_counts;
    call.capacity = capacity;
    call.sums = reinterpret_cast<const long long*>(d_sums);
    call.obs = d_obs;
    call.voxel_m = voxel_m;
    call.min_count = min_count;
    call.min_span = min_span;
    call.first_segment = d_first_segment_of_rank;
    call.xyz_mean = d_xyz_mean;
    call.gray_mean = d_gray_mean;
    call.kept = d_kept;
    launch_voxel_means(call, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_voxel_means_host(const float* xyz, uint32_t count, int capacity, const int64_t* sums, const uint32_t* obs, float voxel_m,
                                  uint32_t min_count, uint32_t min_span, const uint32_t* first_segment_of_rank, float* xyz_mean,
                                  uint8_t* gray_mean, uint32_t* kept) {
    vors_status st = voxel_means_refusals("voxel_means_host", xyz, sums, obs, voxel_m, capacity, min_span, first_segment_of_rank, xyz_mean,
                                          gray_mean, kept);
    if (st != VORS_OK) return st;
    const uint32_t n = count < (uint32_t)capacity ? count : (uint32_t)capacity;
    uint32_t k = 0;
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t* ob = obs + 2 * (size_t)r;
        const VoxelMean m = voxel_mean(voxel_m, xyz + 3 * (size_t)r, sums + 4 * (size_t)r, ob[0], ob[1],
                                       first_segment_of_rank ? first_segment_of_rank[r] : ob[1], min_count, min_span);
        if (xyz_mean)
            for (int a = 0; a < 3; ++a) xyz_mean[3 * (size_t)r + a] = m.xyz[a];
        if (gray_mean) gray_mean[r] = m.gray;
        k += m.kept ? 1u : 0u;
    }
    if (kept) *kept = k;
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Re-posing of point lists and the voxel filter of plain lists (include/vors_hip.h 2i): the refusals the device and the host entries
// share, the device entries (repose_kernels.hip) and the host twins, which run the kernels' own texts (lie.h repose_*, voxel_key,
// voxel_filter_below).
// ---------------------------------------------------------------------------------------------------------------
// An array of a call as the overlap test sees it. Two arrays overlap when they share a byte; `same` names the one input an output may
// be — exactly, base and extent — without being refused.
struct ArgSpan {
    const char* name;
    const void* p;
    size_t bytes;
    const void* same;
};
static bool spans_share(const ArgSpan& a, const ArgSpan& b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
static vors_status overlap_refusals(const std::string& w, const std::vector<ArgSpan>& in, const std::vector<ArgSpan>& out) {
    for (size_t o = 0; o < out.size(); ++o) {
        for (const ArgSpan& i : in)
            if (spans_share(out[o], i) && !(out[o].same && out[o].same == i.p && out[o].p == i.p))
                return fail(VORS_ERR_INVALID_ARGUMENT, w + ": " + out[o].name + " overlaps " + i.name);
        for (size_t q = 0; q < o; ++q)
            if (spans_share(out[o], out[q])) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": " + out[o].name + " overlaps " + out[q].name);
    }
    return VORS_OK;
}
// A handle-free pass runs on the calling thread's current device: a stream of another one is refused (a stream nobody can place: let the
// launch report).
static vors_status stream_refusal(const std::string& w, hipStream_t s) {
    if (!s) return VORS_OK;
    hipDevice_t of;
    int cur = -1;
    if (hipStreamGetDevice(s, &of) != hipSuccess || hipGetDevice(&cur) != hipSuccess) {
        (void)hipGetLastError();
        return VORS_OK;
    }
    if ((int)of != cur)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the stream belongs to device " + std::to_string((int)of) + " but the current device is " + std::to_string(cur));
    return VORS_OK;
}

static vors_status repose_refusals(const char* who, const ReposeCall& c) {
    const std::string w(who);
    if (c.n < 1 || c.n > 65535) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": n must be in 1..65535");
    if (c.capacity < 1 || c.max_keyframes < 1 || c.node_capacity < 1)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": capacity, max_keyframes and node_capacity must be >= 1");
    if (!c.xyz || !c.list_counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a list (xyz, list_counts) is NULL");
    if (!c.segments || !c.n_segments) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the segments or their count are NULL");
    if (!c.poses_new || !c.node_counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": the new poses or their count are NULL");
    if (!c.xyz_out && !c.normals_out) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": no list output at all (xyz_out and normals_out are NULL)");
    if (c.normals_out && !c.normals) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": normals_out without normals");
    for (const void* p : {(const void*)c.xyz, (const void*)c.normals, (const void*)c.list_counts, (const void*)c.segments, (const void*)c.n_segments,
                          (const void*)c.poses_new, (const void*)c.node_counts, (const void*)c.node_of_segment, (const void*)c.xyz_out,
                          (const void*)c.normals_out, (const void*)c.segments_out, (const void*)c.counts_out})
        if ((uintptr_t)p % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": every array must be 4-byte aligned");
    const size_t lists = (size_t)c.n * (size_t)c.capacity * 12, words = (size_t)c.n * 4, recs = (size_t)c.n * (size_t)c.max_keyframes * sizeof(vors_map_segment);
    const std::vector<ArgSpan> in{{"xyz", c.xyz, lists, nullptr}, {"normals", c.normals, lists, nullptr}, {"list_counts", c.list_counts, words, nullptr},
                                  {"segments", c.segments, recs, nullptr}, {"n_segments", c.n_segments, words, nullptr},
                                  {"poses7_new", c.poses_new, (size_t)c.n * (size_t)c.node_capacity * (size_t)c.pose_stride * 4, nullptr},
                                  {"node_counts", c.node_counts, words, nullptr},
                                  {"node_of_segment", c.node_of_segment, (size_t)c.n * (size_t)c.max_keyframes * 4, nullptr}};
    const std::vector<ArgSpan> out{{"xyz_out", c.xyz_out, lists, c.xyz}, {"normals_out", c.normals_out, lists, c.normals},
                                   {"segments_out", c.segments_out, recs, c.segments},
                                   {"counts_out", c.counts_out, (size_t)c.n * VORS_REPOSE_COUNTS * 4, nullptr}};
    return overlap_refusals(w, in, out);
}

extern "C" vors_status repose_points_device(const char* who, ReposeCall call, size_t pose_stride_bytes, hipStream_t s) {
    vors_status st = stride_refusal(who, "pose_stride_bytes", pose_stride_bytes, 28, OPERATOR_STRIDE_LIMIT);
    if (st != VORS_OK) return st;
    call.pose_stride = stride_words(pose_stride_bytes, 7);
    if ((st = repose_refusals(who, call)) != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    if ((st = stream_refusal(who, s)) != VORS_OK) return st;
    launch_repose_points(call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_repose_points(int n, const float* d_xyz, const float* d_normals, const uint32_t* d_list_counts, int capacity,
                               const vors_map_segment* d_segments, const uint32_t* d_n_segments, int max_keyframes, const void* d_poses7_new,
                               size_t pose_stride_bytes, int node_capacity, const uint32_t* d_node_counts, const uint32_t* d_node_of_segment,
                               float* d_xyz_out, float* d_normals_out, vors_map_segment* d_segments_out, uint32_t* d_counts_out, void* hip_stream) {
    const ReposeCall call{n, d_xyz, d_normals, d_list_counts, capacity, d_segments, d_n_segments, max_keyframes, static_cast<const float*>(d_poses7_new),
                          7, node_capacity, d_node_counts, d_node_of_segment, d_xyz_out, d_normals_out, d_segments_out, d_counts_out};
    return repose_points_device("repose_points", call, pose_stride_bytes, static_cast<hipStream_t>(hip_stream));
}

vors_status vors_repose_points_host(const float* xyz, const float* normals, uint32_t count, int capacity, const vors_map_segment* segments,
                                    uint32_t n_segments, int max_keyframes, const float* poses7_new, uint32_t node_count, int node_capacity,
                                    const uint32_t* node_of_segment, float* xyz_out, float* normals_out, vors_map_segment* segments_out,
                                    uint32_t counts_out[VORS_REPOSE_COUNTS]) {
    const ReposeCall c{1, xyz, normals, &count, capacity, segments, &n_segments, max_keyframes, poses7_new, 7, node_capacity, &node_count,
                       node_of_segment, xyz_out, normals_out, segments_out, counts_out};
    if (vors_status st = repose_refusals("repose_points_host", c); st != VORS_OK) return st;
    const uint32_t total = std::min<uint32_t>(count, (uint32_t)capacity), n_rec = std::min<uint32_t>(n_segments, (uint32_t)max_keyframes);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(segments);
    // the decision and the two poses of every recorded segment, from the records as they are before anything is written
    std::vector<uint8_t> moved(n_rec);
    std::vector<Iso> A(n_rec), B(n_rec);
    uint32_t counts[VORS_REPOSE_COUNTS] = {0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < n_rec; ++k) {
        const uint32_t node = repose_node(k, node_of_segment, node_count, node_capacity);
        const float* b7 = node != VORS_REPOSE_NO_NODE ? poses7_new + (size_t)node * 7 : nullptr;
        moved[k] = repose_moves(segments[k].pose7, b7) ? 1 : 0;
        A[k] = iso_load(segments[k].pose7);
        B[k] = moved[k] ? iso_load(b7) : A[k];
        counts[REPOSE_SEGMENTS_MOVED] += moved[k];
    }
    uint32_t k = 0;
    for (uint32_t r = 0; r < total; ++r) {
        while (k + 1u < n_rec && words[(size_t)(k + 1u) * MAP_SEGMENT_WORDS + 1] <= r) ++k;  // the last record whose first is <= r
        uint32_t lo = 0, hi = 0;
        if (n_rec) repose_segment_ranks(words, k, n_rec, total, &lo, &hi);
        const bool recorded = r >= lo && r < hi;
        const V3 p{xyz[3 * (size_t)r], xyz[3 * (size_t)r + 1], xyz[3 * (size_t)r + 2]};
        const bool finite = repose_finite3(p);
        V3 q = p;
        if (recorded && moved[k] && finite) {
            q = repose_point(A[k], B[k], p);
            counts[REPOSE_MAX_SHIFT] = std::max(counts[REPOSE_MAX_SHIFT], repose_shift_bits(p, q));
        }
        counts[!finite ? REPOSE_NONFINITE : !recorded ? REPOSE_NO_RECORD : moved[k] ? REPOSE_MOVED : REPOSE_KEPT] += 1u;
        if (xyz_out) {
            float* o = xyz_out + 3 * (size_t)r;
            o[0] = q.x; o[1] = q.y; o[2] = q.z;
        }
        if (normals_out) {
            V3 m{normals[3 * (size_t)r], normals[3 * (size_t)r + 1], normals[3 * (size_t)r + 2]};
            if (recorded && moved[k] && repose_finite3(m)) m = repose_normal(A[k], B[k], m);
            float* o = normals_out + 3 * (size_t)r;
            o[0] = m.x; o[1] = m.y; o[2] = m.z;
        }
    }
    if (segments_out)
        for (uint32_t s = 0; s < n_rec; ++s) {
            vors_map_segment rec = segments[s];
            if (moved[s]) iso_store(B[s], rec.pose7);
            segments_out[s] = rec;
        }
    if (counts_out) std::memcpy(counts_out, counts, sizeof(counts));
    return VORS_OK;
}

static vors_status voxel_filter_refusals(const char* who, const VoxelFilterCall& c, const void* workspace, size_t workspace_bytes) {
    const std::string w(who);
    if (c.n < 1 || c.n > 65535) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": n must be in 1..65535");
    if (c.capacity < 1) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": capacity must be >= 1");
    if (!c.xyz || !c.list_counts) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a list (xyz, list_counts) is NULL");
    if (!c.index || !c.counts_out || !c.overflow) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": index, counts_out or overflow is NULL");
    if (!(c.voxel_m > 0.0f) || !(c.voxel_m <= 3.4028234663852886e38f))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": voxel size voxel_m must be finite and > 0");
    if (c.table_slots < 64 || c.table_slots > (1 << 30) || (c.table_slots & (c.table_slots - 1)) != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": table_slots must be a power of two in 64..2^30");
    if ((c.pixel_out && !c.pixel) || (c.gray_out && !c.gray) || (c.normals_out && !c.normals))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": a gathered output (pixel_out, gray_out, normals_out) without its input");
    if (c.segments_out && (!c.segments || !c.n_segments || c.max_keyframes < 1))
        return fail(VORS_ERR_INVALID_ARGUMENT, w + ": segments_out without segments, their count or max_keyframes >= 1");
    for (const void* p : {(const void*)c.xyz, (const void*)c.list_counts, (const void*)c.index, (const void*)c.counts_out, (const void*)c.overflow,
                          (const void*)c.pixel, (const void*)c.normals, (const void*)c.xyz_out, (const void*)c.pixel_out, (const void*)c.normals_out,
                          (const void*)c.segments, (const void*)c.n_segments, (const void*)c.segments_out})
        if ((uintptr_t)p % 4 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, w + ": every array but the greys must be 4-byte aligned");
    const size_t ranks = (size_t)c.n * (size_t)c.capacity, words = (size_t)c.n * 4;
    const size_t recs = c.segments_out ? (size_t)c.n * (size_t)c.max_keyframes * sizeof(vors_map_segment) : 0;
    const std::vector<ArgSpan> in{{"xyz", c.xyz, ranks * 12, nullptr}, {"list_counts", c.list_counts, words, nullptr}, {"pixel", c.pixel, ranks * 4, nullptr},
                                  {"gray", c.gray, ranks, nullptr}, {"normals", c.normals, ranks * 12, nullptr}, {"segments", c.segments, recs, nullptr},
                                  {"n_segments", c.segments_out ? c.n_segments : nullptr, words, nullptr}};
    const std::vector<ArgSpan> out{{"workspace", workspace, workspace_bytes, nullptr}, {"index", c.index, ranks * 4, nullptr},
                                   {"counts_out", c.counts_out, words, nullptr}, {"overflow", c.overflow, words, nullptr},
                                   {"xyz_out", c.xyz_out, ranks * 12, nullptr}, {"pixel_out", c.pixel_out, ranks * 4, nullptr},
                                   {"gray_out", c.gray_out, ranks, nullptr}, {"normals_out", c.normals_out, ranks * 12, nullptr},
                                   {"segments_out", c.segments_out, recs, nullptr}};
    return overlap_refusals(w, in, out);
}

uint64_t vors_voxel_filter_workspace_bytes(int n, int capacity, int table_slots) {
    if (n < 1 || capacity < 1 || table_slots < 64 || table_slots > (1 << 30)) return 0;
    return (uint64_t)voxel_filter_workspace_carve(nullptr, nullptr, n, capacity, table_slots);
}

vors_status vors_voxel_filter_points(int n, const float* d_xyz, const uint32_t* d_list_counts, int capacity, float voxel_m, int table_slots,
                                     void* d_workspace, const uint32_t* d_pixel, const uint8_t* d_gray, const float* d_normals,
                                     const vors_map_segment* d_segments, const uint32_t* d_n_segments, int max_keyframes, uint32_t* d_index,
                                     uint32_t* d_counts_out, uint32_t* d_overflow, float* d_xyz_out, uint32_t* d_pixel_out, uint8_t* d_gray_out,
                                     float* d_normals_out, vors_map_segment* d_segments_out, void* hip_stream) {
    const char* who = "voxel_filter_points";
    VoxelFilterCall call{};
    call.n = n; call.xyz = d_xyz; call.list_counts = d_list_counts; call.capacity = capacity; call.voxel_m = voxel_m; call.table_slots = table_slots;
    call.index = d_index; call.counts_out = d_counts_out; call.overflow = d_overflow;
    call.pixel = d_pixel; call.gray = d_gray; call.normals = d_normals;
    call.xyz_out = d_xyz_out; call.pixel_out = d_pixel_out; call.gray_out = d_gray_out; call.normals_out = d_normals_out;
    call.segments = d_segments; call.n_segments = d_n_segments; call.max_keyframes = max_keyframes; call.segments_out = d_segments_out;
    if (!d_workspace)
        return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": d_workspace is NULL (the pass allocates nothing: vors_voxel_filter_workspace_bytes)");
    if ((uintptr_t)d_workspace % 16 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": d_workspace must be 16-byte aligned");
    vors_status st = voxel_filter_refusals(who, call, d_workspace, (size_t)vors_voxel_filter_workspace_bytes(n, capacity, table_slots));
    if (st != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if ((st = stream_refusal(who, s)) != VORS_OK) return st;
    voxel_filter_workspace_carve(&call, d_workspace, n, capacity, table_slots);
    launch_voxel_filter_points(call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_voxel_filter_points_host(const float* xyz, uint32_t count, int capacity, float voxel_m, int table_slots, const uint32_t* pixel,
                                          const uint8_t* gray, const float* normals, const vors_map_segment* segments, uint32_t n_segments,
                                          int max_keyframes, uint32_t* index, uint32_t* count_out, uint32_t* overflow, float* xyz_out,
                                          uint32_t* pixel_out, uint8_t* gray_out, float* normals_out, vors_map_segment* segments_out) {
    VoxelFilterCall c{};
    c.n = 1; c.xyz = xyz; c.list_counts = &count; c.capacity = capacity; c.voxel_m = voxel_m; c.table_slots = table_slots;
    c.index = index; c.counts_out = count_out; c.overflow = overflow; c.pixel = pixel; c.gray = gray; c.normals = normals;
    c.xyz_out = xyz_out; c.pixel_out = pixel_out; c.gray_out = gray_out; c.normals_out = normals_out;
    c.segments = segments; c.n_segments = &n_segments; c.max_keyframes = max_keyframes; c.segments_out = segments_out;
    if (vors_status st = voxel_filter_refusals("voxel_filter_points_host", c, nullptr, 0); st != VORS_OK) return st;
    const uint32_t total = std::min<uint32_t>(count, (uint32_t)capacity);
    std::unordered_map<uint64_t, uint32_t> first_of;  // key -> its first rank
    uint32_t kept = 0;
    for (uint32_t r = 0; r < total; ++r) {
        const float* w = xyz + 3 * (size_t)r;
        const uint64_t key = voxel_key(voxel_m, w[0], w[1], w[2]);
        if (key == VORS_VOXEL_NONE || !first_of.emplace(key, r).second) continue;
        index[kept] = r;
        if (xyz_out) std::memcpy(xyz_out + 3 * (size_t)kept, w, 12);
        if (pixel_out) pixel_out[kept] = pixel[r];
        if (gray_out) gray_out[kept] = gray[r];
        if (normals_out) std::memcpy(normals_out + 3 * (size_t)kept, normals + 3 * (size_t)r, 12);
        kept += 1;
    }
    *count_out = kept;
    *overflow = first_of.size() > (size_t)table_slots ? 1u : 0u;  // (the device's result is then unspecified; this one stays exact)
    if (segments_out) {
        const uint32_t n_rec = std::min<uint32_t>(n_segments, (uint32_t)max_keyframes);
        for (uint32_t k = 0; k < n_rec; ++k) {
            vors_map_segment rec = segments[k];
            const uint32_t lo = voxel_filter_below(index, kept, (uint64_t)rec.first);
            const uint32_t hi = voxel_filter_below(index, kept, (uint64_t)rec.first + (uint64_t)rec.count);
            rec.first = lo;
            rec.count = hi - lo;
            segments_out[k] = rec;
        }
    }
    return VORS_OK;
}

void vors_camera_project(const float cam5[5], const float pose7[7], const float* xyz, int n, float* uvw_out) {
    const Intr k = intr_from_cam5(cam5);
    for (int i = 0; i < n; ++i) {
        V3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (pose7) p = extr_project(iso_load(pose7), p);
        const V3 w = intr_project(k, p);
        uvw_out[3 * i] = w.x; uvw_out[3 * i + 1] = w.y; uvw_out[3 * i + 2] = w.z;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// synthetic scenes
// ---------------------------------------------------------------------------------------------------------------
vors_status vors_synth_render_pairs(uint64_t seed0, int n_pairs, int rows, int cols, const double cam5[5], double motion_scale,
                                    int invalid_percent, uint8_t* d_kf_gray, uint16_t* d_kf_depth, uint8_t* d_cur_gray,
                                    uint16_t* d_cur_depth, float* d_gt_models7, void* hip_stream) {
    if (!cam5 || !d_kf_gray || !d_kf_depth || !d_cur_gray) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_pairs < 1 || rows < 1 || cols < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "bad shape");
    vors_status st = require_device();
    if (st != VORS_OK) return st;
    launch_synth_pairs(seed0, n_pairs, rows, cols, cam5, motion_scale, invalid_percent, d_kf_gray, d_kf_depth, d_cur_gray,
                       d_cur_depth, d_gt_models7, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_synth_render_frames(int n_frames, const uint64_t* seeds, const uint64_t* salts, const double* xi6, int rows, int cols,
                                     const double cam5[5], int invalid_percent, uint8_t* d_gray, uint16_t* d_depth, void* hip_stream) {
    if (!seeds || !salts || !xi6 || !cam5 || !d_gray || !d_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_frames < 1 || rows < 1 || cols < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "bad shape");
    vors_status st = require_device();
    if (st != VORS_OK) return st;
    struct Frame {
        uint64_t seed, salt;
        double xi[6];
    };
    std::vector<Frame> h((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        h[f].seed = seeds[f];
        h[f].salt = salts[f];
        for (int q = 0; q < 6; ++q) h[f].xi[q] = xi6[6 * f + q];
    }
    DevBuf d;
    HIP_TRY(d.alloc(h.size() * sizeof(Frame)));
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(Frame), hipMemcpyHostToDevice, s));
    launch_synth_frames(d.p, n_frames, rows, cols, cam5, invalid_percent, d_gray, d_depth, s);
    HIP_TRY(hipStreamSynchronize(s));  // (the table is freed on return)
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

}  // extern "C"
