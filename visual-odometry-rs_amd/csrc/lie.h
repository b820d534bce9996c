// Rigid-motion arithmetic of the tracker, host + device (f32, compile with -ffp-contract=off).
//
// Implements what the reference gets from src/math/se3.rs, src/math/so3.rs and from nalgebra 0.17
// (Isometry3 / UnitQuaternion / 6x6 Cholesky). Operation ORDER matters: the LM loop branches on f32
// comparisons, so every expression below is written in the order the reference evaluates it.
// nalgebra itself is not vendored in the reference; its evaluation orders are restated from its source
// (see DESIGN.md "nalgebra assumptions").
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VORS_HD __host__ __device__ inline
#define VORS_UNROLL _Pragma("unroll")
#else
#define VORS_HD inline
#define VORS_UNROLL  // (a host compiler unrolls, or not, as it sees fit)
#endif

namespace vors {

struct V3 {
    float x, y, z;
};
struct Quat {  // nalgebra coords order [i, j, k, w]
    float i, j, k, w;
};
struct Iso {  // Isometry3<f32>
    V3 t;
    Quat q;
};

VORS_HD Iso iso_identity() { return Iso{{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 1.f}}; }
VORS_HD Iso iso_load(const float* p) { return Iso{{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}}; }
VORS_HD void iso_store(const Iso& m, float* p) {
    p[0] = m.t.x; p[1] = m.t.y; p[2] = m.t.z;
    p[3] = m.q.i; p[4] = m.q.j; p[5] = m.q.k; p[6] = m.q.w;
}

VORS_HD V3 cross(const V3& a, const V3& b) {
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
VORS_HD float dot3(const V3& a, const V3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
VORS_HD float quat_norm_squared(const Quat& q) {
    float a = q.i * q.i, b = q.j * q.j;
    const float c = q.k * q.k, d = q.w * q.w;
    a += c;
    b += d;
    return a + b;
}
// UnitQuaternion * Vector3:  t = 2 (qv x p);  p' = (t w + qv x t) + p
VORS_HD V3 quat_rotate(const Quat& q, const V3& p) {
    const V3 qv{q.i, q.j, q.k};
    V3 t = cross(qv, p);
    t = V3{t.x * 2.0f, t.y * 2.0f, t.z * 2.0f};
    const V3 c = cross(qv, t);
    return V3{(t.x * q.w + c.x) + p.x, (t.y * q.w + c.y) + p.y, (t.z * q.w + c.z) + p.z};
}
VORS_HD Quat quat_mul(const Quat& a, const Quat& b) {
    Quat r;
    r.w = a.w * b.w - dot3(V3{a.i, a.j, a.k}, V3{b.i, b.j, b.k});
    r.i = a.w * b.i + a.i * b.w + a.j * b.k - a.k * b.j;
    r.j = a.w * b.j - a.i * b.k + a.j * b.w + a.k * b.i;
    r.k = a.w * b.k + a.i * b.j - a.j * b.i + a.k * b.w;
    return r;
}
VORS_HD Quat unit_from_quaternion(const Quat& q) {
    const float n = sqrtf(quat_norm_squared(q));
    return Quat{q.i / n, q.j / n, q.k / n, q.w / n};
}
VORS_HD V3 iso_transform_point(const Iso& m, const V3& p) {
    const V3 r = quat_rotate(m.q, p);
    return V3{r.x + m.t.x, r.y + m.t.y, r.z + m.t.z};
}
VORS_HD Iso iso_mul(const Iso& a, const Iso& b) {
    const V3 s = quat_rotate(a.q, b.t);
    return Iso{V3{a.t.x + s.x, a.t.y + s.y, a.t.z + s.z}, quat_mul(a.q, b.q)};
}
VORS_HD Iso iso_inverse(const Iso& a) {
    const Quat qi{-a.q.i, -a.q.j, -a.q.k, a.q.w};
    return Iso{quat_rotate(qi, V3{-a.t.x, -a.t.y, -a.t.z}), qi};
}
// reference: src/core/track/lm_optimizer.rs:198-209 (first-order re-normalisation)
VORS_HD Iso renormalize(Iso m) {
    const float f = 0.5f * (3.0f - quat_norm_squared(m.q));
    m.q = Quat{f * m.q.i, f * m.q.j, f * m.q.k, f * m.q.w};
    return m;
}

// sinf / cosf as the reference computes them: Rust's f32::sin / cos call the platform libm, i.e. glibc's sinf / cosf (>= 2.28: the
// ARM optimized-routines algorithm — argument widened to f64, |x| < pi/4: odd / even polynomial in f64; otherwise x - n pi/2 with
// n = round(x 2/pi) and the polynomial selected by the quadrant — rounded ONCE to f32). That function is NOT the correctly rounded
// sine (1 % of the arguments in [1e-3, 4] differ from RN(sin x) by one ulp), and the device's ocml sinf is a third function, so the
// algorithm is restated here, host + device: bit-identical to glibc 2.35's sinf / cosf for EVERY f32 in [2^-12, 4) — with or
// without FMA contraction of the f64 polynomial (checked exhaustively against the platform libm through vors_ref_sincos: tests/test_capi_host.py). se3::exp
// only calls them with theta / 2 and theta, theta >= 0.01 (se3.rs:82-87); arguments >= 4 rad go to the platform function.
VORS_HD float ref_sincos_poly(double x, int n) {
    const double x2 = x * x;
    if ((n & 1) == 0) {
        const double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
        const double x3 = x * x2, s1 = S2 + x2 * S3, x7 = x3 * x2, s = x + x3 * S1;
        return (float)(s + x7 * s1);
    }
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10, C4 = 0x1.99343027bf8c3p-16;
    const double x4 = x2 * x2, c2 = C3 + x2 * C4, c1 = C0 + x2 * C1, x6 = x4 * x2, c = c1 + x4 * C2;
    return (float)(c + x6 * c2);
}
VORS_HD float ref_sincos(float y, int quadrant_shift) {  // 0: sin, 1: cos; 0 <= y < 4
    double x = (double)y;
    int n = 0;
    if (!(y < 0x1.921fb6p-1f)) {  // pi/4
        const double r = x * 0x1.45F306DC9C883p+23;  // x * 2/pi * 2^24
        n = ((int32_t)r + 0x800000) >> 24;
        x = x - (double)n * 0x1.921FB54442D18p0;
    } else if (y < 0x1p-12f) {
        return quadrant_shift ? 1.0f : y;
    }
    n += quadrant_shift;
    const float v = ref_sincos_poly((n & 2) && !(n & 1) ? -x : x, n);
    return ((n & 2) && (n & 1)) ? -v : v;
}
VORS_HD float ref_sinf(float y) { return (y >= 0.f && y < 4.0f) ? ref_sincos(y, 0) : sinf(y); }
VORS_HD float ref_cosf(float y) { return (y >= 0.f && y < 4.0f) ? ref_sincos(y, 1) : cosf(y); }

// reference: src/math/se3.rs:65-95 with so3::hat / hat_2 (src/math/so3.rs:27-51) expanded in place.
VORS_HD Iso se3_exp(const float xi[6]) {
    const float vx = xi[0], vy = xi[1], vz = xi[2];
    const float wx = xi[3], wy = xi[4], wz = xi[5];
    const float theta_2 = (wx * wx + wy * wy) + wz * wz;
    float real_factor, imag_factor, c1, c2;
    if (theta_2 < 1e-2f * 1e-2f) {
        real_factor = 1.0f - 0.125f * theta_2;
        imag_factor = 0.5f - (1.0f / 48.0f) * theta_2;
        c1 = 0.5f - (1.0f / 24.0f) * theta_2;
        c2 = (1.0f / 6.0f) - (1.0f / 120.0f) * theta_2;
    } else {
        const float theta = sqrtf(theta_2);
        const float half_theta = 0.5f * theta;
        real_factor = ref_cosf(half_theta);
        imag_factor = ref_sinf(half_theta) / theta;
        c1 = (1.0f - ref_cosf(theta)) / theta_2;
        c2 = (theta - ref_sinf(theta)) / (theta * theta_2);
    }
    const float w11 = wx * wx, w12 = wx * wy, w13 = wx * wz, w22 = wy * wy, w23 = wy * wz, w33 = wz * wz;
    const float O[3][3] = {{0.0f, -wz, wy}, {wz, 0.0f, -wx}, {-wy, wx, 0.0f}};
    const float O2[3][3] = {{-w22 - w33, w12, w13}, {w12, -w11 - w33, w23}, {w13, w23, -w11 - w22}};
    float V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) V[r][c] = ((r == c ? 1.0f : 0.0f) + c1 * O[r][c]) + c2 * O2[r][c];
    Iso out;
    out.t.x = (V[0][0] * vx + V[0][1] * vy) + V[0][2] * vz;
    out.t.y = (V[1][0] * vx + V[1][1] * vy) + V[1][2] * vz;
    out.t.z = (V[2][0] * vx + V[2][1] * vy) + V[2][2] * vz;
    out.q = unit_from_quaternion(Quat{imag_factor * wx, imag_factor * wy, imag_factor * wz, real_factor});
    return out;
}

// 6x6 Cholesky (lower, left-looking) + solve, the order nalgebra's Cholesky::new / ::solve use.
// H is the full symmetric matrix, row-major h[r*6+c]; only the lower triangle is read.
// Returns false when a pivot is not > 0 (nalgebra returns None -> Err at lm_optimizer.rs:131-133).
VORS_HD bool cholesky6_solve(const float* h, const float* g, float lm_coef, float* delta) {
    float a[6][6];
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) a[r][c] = h[r * 6 + c];
    const float scale = 1.0f + lm_coef;  // lm_optimizer.rs:125-130
    for (int r = 0; r < 6; ++r) a[r][r] *= scale;
    for (int j = 0; j < 6; ++j) {
        for (int k = 0; k < j; ++k) {
            const float factor = -a[j][k];
            for (int i = j; i < 6; ++i) a[i][j] = factor * a[i][k] + a[i][j];
        }
        const float diag = a[j][j];
        if (!(diag > 0.0f)) return false;
        const float denom = sqrtf(diag);
        a[j][j] = denom;
        for (int i = j + 1; i < 6; ++i) a[i][j] /= denom;
    }
    float b[6];
    for (int i = 0; i < 6; ++i) b[i] = g[i];
    for (int i = 0; i < 6; ++i) {
        const float coeff = b[i] / a[i][i];
        b[i] = coeff;
        for (int k = i + 1; k < 6; ++k) b[k] = (-coeff) * a[k][i] + b[k];
    }
    for (int i = 5; i >= 0; --i) {
        float dot = 0.0f;
        for (int k = i + 1; k < 6; ++k) dot += a[k][i] * b[k];
        b[i] = (b[i] - dot) / a[i][i];
    }
    for (int i = 0; i < 6; ++i) delta[i] = b[i];
    return true;
}

// Pose information from the 29 sums of one evaluation (include/vors_hip.h, "pose information"): info36 = H, the upper triangle
// sums[8..28] mirrored; sigma2 = sums[0] / (n_inside - 6); cov36 = sigma2 * H^-1 through a 6x6 Cholesky in f64 (H = L L^T,
// H^-1 = L^-T L^-1), rounded to f32 at the end and symmetric by construction. Returns the flags: bit 0 = n_inside <= 6, bit 1 = a pivot
// that is not > 0; with either, cov36 and sigma2 are NaN (info36 is written all the same). Every output is nullable. The one text the
// host entry (vors_pose_information_from_sums) and the device kernel (lm_kernels.hip pose_information_kernel) both run.
VORS_HD int pose_information(const float* sums29, float* info36, float* cov36, float* sigma2) {
    double a[6][6];
    int k = 8;
VORS_UNROLL
    for (int r = 0; r < 6; ++r)
VORS_UNROLL
        for (int c = r; c < 6; ++c) {
            const float v = sums29[k++];
            a[r][c] = a[c][r] = (double)v;
            if (info36) info36[r * 6 + c] = info36[c * 6 + r] = v;
        }
    int flags = (sums29[1] > 6.0f) ? 0 : 1;  // (a NaN count is "too few points" as well)
    // Left-looking, lower triangle, like cholesky6_solve. No early exit: a pivot that is not > 0 is remembered and the factorisation runs
    // on (whatever it then holds is never handed out), so that the loops unroll and the device keeps the factor in registers.
    bool pivots_ok = true;
VORS_UNROLL
    for (int j = 0; j < 6; ++j) {
VORS_UNROLL
        for (int q = 0; q < j; ++q)
VORS_UNROLL
            for (int i = j; i < 6; ++i) a[i][j] -= a[j][q] * a[i][q];
        pivots_ok = pivots_ok && a[j][j] > 0.0;
        const double d = sqrt(a[j][j]);
        a[j][j] = d;
VORS_UNROLL
        for (int i = j + 1; i < 6; ++i) a[i][j] /= d;
    }
    if (!pivots_ok) flags |= 2;
    const float nan = nanf("");
    if (flags) {
        if (sigma2) *sigma2 = nan;
        if (cov36)
VORS_UNROLL
            for (int i = 0; i < 36; ++i) cov36[i] = nan;
        return flags;
    }
    const double s2 = (double)sums29[0] / ((double)sums29[1] - 6.0);
    if (sigma2) *sigma2 = (float)s2;
    if (!cov36) return flags;
    double inv[6][6];  // L^-1, lower triangular, column by column (forward substitution on the unit vectors)
VORS_UNROLL
    for (int c = 0; c < 6; ++c)
VORS_UNROLL
        for (int r = 0; r < 6; ++r) {
            if (r < c) {
                inv[r][c] = 0.0;
                continue;
            }
            double t = r == c ? 1.0 : 0.0;
VORS_UNROLL
            for (int q = c; q < r; ++q) t -= a[r][q] * inv[q][c];
            inv[r][c] = t / a[r][r];
        }
VORS_UNROLL
    for (int r = 0; r < 6; ++r)
VORS_UNROLL
        for (int c = 0; c <= r; ++c) {
            double t = 0.0;
VORS_UNROLL
            for (int q = r; q < 6; ++q) t += inv[q][r] * inv[q][c];  // (L^-T L^-1)[r][c], q >= max(r, c) = r
            cov36[r * 6 + c] = cov36[c * 6 + r] = (float)(s2 * t);
        }
    return flags;
}

// Scale of the residuals from the 256-bin histogram of |r| (include/vors_hip.h, vors_batch_residual_maps: bin k counts k <= |r| < k + 1, the
// last one 255 <= |r|), in f64: n = sum of the bins, target = n / 2, b = the first bin whose cumulative count reaches target,
// median_abs = b + (target - count below b) / hist[b] (the bin's counts spread evenly over its width), sigma_mad = 1.4826 median_abs, each
// rounded to f32 at the end. n = 0: both NaN. Every output is nullable. The one text the host entry (vors_residual_scale_from_hist) and
// the device kernel (product_kernels.hip residual_scale_kernel) both run.
VORS_HD void residual_scale_from_hist(const uint32_t* hist, float* median_abs, float* sigma_mad, uint32_t* n_inside) {
    unsigned long long n = 0;
    for (int k = 0; k < 256; ++k) n += hist[k];
    if (n_inside) *n_inside = (uint32_t)n;
    if (n == 0) {
        if (median_abs) *median_abs = nanf("");
        if (sigma_mad) *sigma_mad = nanf("");
        return;
    }
    const double target = 0.5 * (double)n;
    unsigned long long below = 0;
    int b = 0;
    while (b < 255 && (double)(below + hist[b]) < target) below += hist[b++];  // (n > 0: some bin reaches target, and that bin is not empty)
    const double med = (double)b + (target - (double)below) / (double)hist[b];
    if (median_abs) *median_abs = (float)med;
    if (sigma_mad) *sigma_mad = (float)(1.4826 * med);
}

// Inverse depth -> depth map value: inverse_depth.rs:37-42, `(scale / x).round() as u16`. roundf rounds halves away from zero like
// f32::round; the cast saturates like Rust's `as` (NaN -> 0, <= 0 -> 0, >= 65535 -> 65535). The comparisons are made in float BEFORE the
// integer conversion, so no out-of-range float is ever converted. The one text the host entry (vors_to_depth) and the device kernel
// (product_kernels.hip pred_depth_kernel) both run.
VORS_HD uint16_t to_depth(float scale, float idepth) {
    const float r = roundf(scale / idepth);
    if (!(r > 0.0f)) return 0;  // NaN, zero, negative
    if (r >= 65535.0f) return 65535;
    return (uint16_t)(int)r;
}

// Depth fusion of one pixel of the current frame: the keyed z-buffer entry `key` = bits(Z') << 32 | src of the nearest keyframe point
// that lands here (all ones: none), its weight (kf_weight[src], 1 without a plane) and the measured depth d (0 = unknown).
// r = Z' - (float)d / depth_scale is the text of the depth residual (product_kernels.hip reproject_sweep). Cases, which are also the counters:
//   0 agree      |r| <= tol_m         depth = to_depth(scale, (wk / Z' + scale / d) / (wk + 1)), weight = min(wk + 1, max_weight)
//   1 conflict, prediction in front   r < -tol_m: the measurement, weight 1
//   2 conflict, prediction behind     r > tol_m:  the measurement, weight 1
//   3 measured only                   no prediction: the measurement, weight 1
//   4 filled     no measurement, fill_min_weight > 0 and wk >= fill_min_weight: to_depth(scale, 1 / Z') (the bits of d_pred_depth), weight wk
//   5 empty      everything else (a NaN residual included): 0, 0
// The mean is taken in inverse depth, the quantity the tracker works in; scale / (float)d is from_depth's expression. A fused depth that
// rounds to 0 (a surface nearer than half a depth unit) gets weight 0, so that depth 0 and weight 0 always coincide; its case stays.
// The expression order is fixed: the one text the host entry (vors_fuse_depth_pixels) and the device kernel (product_kernels.hip
// fuse_depth_kernel) both run, bit for bit. kf_weight is read at src only when the key is not empty.
struct FusedPixel {
    uint16_t depth;
    uint8_t weight;
    uint8_t kase;
};
VORS_HD FusedPixel fuse_depth_pixel(float depth_scale, float tol_m, int max_weight, int fill_min_weight, uint64_t key, const uint8_t* kf_weight,
                                    uint16_t d) {
    const bool has_p = key != 0xFFFFFFFFFFFFFFFFull, has_m = d != 0;
    const float zp = __builtin_bit_cast(float, (uint32_t)(key >> 32));
    const int wk = (has_p && kf_weight) ? (int)kf_weight[(uint32_t)key] : 1;
    const float r = zp - (float)d / depth_scale;
    FusedPixel o{0, 0, 5};
    if (has_p && has_m) {
        if (fabsf(r) <= tol_m) {
            o.depth = to_depth(depth_scale, ((float)wk * (1.0f / zp) + depth_scale / (float)d) / ((float)wk + 1.0f));
            o.weight = (uint8_t)(wk + 1 < max_weight ? wk + 1 : max_weight);
            o.kase = 0;
        } else if (r < -tol_m || r > tol_m) {
            o.depth = d;
            o.weight = 1;
            o.kase = r < -tol_m ? 1 : 2;
        }
    } else if (has_m) {
        o.depth = d;
        o.weight = 1;
        o.kase = 3;
    } else if (has_p && fill_min_weight > 0 && wk >= fill_min_weight) {
        o.depth = to_depth(depth_scale, 1.0f / zp);
        o.weight = (uint8_t)wk;
        o.kase = 4;
    }
    if (o.depth == 0) o.weight = 0;
    return o;
}

// Voxel of a world point on a grid of edge voxel_m (the keyframe map's voxel filter): per axis q = floorf(w / voxel_m), an
// IEEE division (never a multiplication by a reciprocal; the translation units that hold this text are built with -ffp-contract=off).
// A point has a key iff all three q are finite and -2^20 <= q < 2^20: key = (qx + 2^20) | (qy + 2^20) << 21 | (qz + 2^20) << 42, below
// 2^63. Everything else — NaN, infinities, a quotient out of range — is all ones (VORS_VOXEL_NONE), which is also what an empty table
// entry holds: no point ever carries it. The comparisons are made in float BEFORE the integer conversion. The one text the host entry
// (vors_voxel_keys) and the device kernels (product_kernels.hip voxel_claim / voxel_owns) both run, bit for bit.
VORS_HD uint64_t voxel_key(float voxel_m, float x, float y, float z) {
    const float q[3] = {floorf(x / voxel_m), floorf(y / voxel_m), floorf(z / voxel_m)};
    uint64_t key = 0;
    for (int a = 0; a < 3; ++a) {
        if (!(q[a] >= -1048576.0f && q[a] < 1048576.0f)) return 0xFFFFFFFFFFFFFFFFull;
        key |= (uint64_t)((int)q[a] + 1048576) << (21 * a);
    }
    return key;
}

// Statistics of a voxel of that map (vors_trackers_enable_map_voxel_stats). The sums are FIXED POINT in 64-bit integers:
// integer addition is associative and commutative, so a sum of these has the same bits whatever the order of arrival.
// voxel_offset_q: one axis of an observation w relative to the voxel's first point f (the stored xyz of the rank), in units of
// voxel_m / 2^20: an f32 subtraction, an IEEE f32 division (never a reciprocal multiply), an exact multiplication by 2^20, rintf (halves
// to even). Bound: two points with one voxel key lie within one edge of each other on every axis, up to the rounding of the two
// quotients, so |q| stays near 2^20 < 2^21, and 2^32 observations (the count wraps there) sum below 2^53 < 2^63: no overflow, and the
// f64 conversion of voxel_mean is exact.
VORS_HD int64_t voxel_offset_q(float voxel_m, float w, float f) { return (int64_t)rintf(((w - f) / voxel_m) * 1048576.0f); }
// The resolve of one rank (vors_voxel_means, vors_voxel_means_host): centroid = f + voxel_m * (float)(sum / (count 2^20)) per axis, the
// division and conversions in IEEE f64; grey = (2 sum + count) / (2 count) in integers (the mean rounded half up). A rank seen fewer than
// max(min_count, 1) times, or over a span of segments last_segment - first_segment below min_span, is rejected: a NaN triple (one bit
// pattern) and grey 0, which every consumer of a list skips. The one text host and device run.
#define VORS_VOXEL_MEAN_NAN_BITS 0x7FC00000u
struct VoxelMean {
    float xyz[3];
    uint8_t gray;
    bool kept;
};
VORS_HD VoxelMean voxel_mean(float voxel_m, const float* f, const int64_t* sums4, uint32_t count, uint32_t last_segment, uint32_t first_segment,
                             uint32_t min_count, uint32_t min_span) {
    VoxelMean o;
    const uint32_t span = last_segment > first_segment ? last_segment - first_segment : 0u;
    o.kept = count >= (min_count > 1u ? min_count : 1u) && span >= min_span;
    if (!o.kept) {
        union {
            uint32_t u;
            float f;
        } nan;
        nan.u = VORS_VOXEL_MEAN_NAN_BITS;
        o.xyz[0] = o.xyz[1] = o.xyz[2] = nan.f;
        o.gray = 0;
        return o;
    }
    const double den = (double)count * 1048576.0;
    for (int a = 0; a < 3; ++a) o.xyz[a] = f[a] + voxel_m * (float)((double)sums4[a] / den);
    o.gray = (uint8_t)((2 * (uint64_t)sums4[3] + count) / (2 * (uint64_t)count));
    return o;
}

// One LM step: lm_optimizer.rs:123-136.
VORS_HD bool lm_step(const float* h36, const float* g6, const Iso& model, float lm_coef, Iso* out) {
    float delta[6];
    if (!cholesky6_solve(h36, g6, lm_coef, delta)) return false;
    const Iso dw = se3_exp(delta);
    *out = renormalize(iso_mul(model, iso_inverse(dw)));
    return true;
}

// What one evaluated candidate means for the level: eval()'s accept test (lm_optimizer.rs:140-149) + stop_criterion
// (lm_optimizer.rs:156-192), and stop_criterion's update of lm_coef. `energy`: the candidate's; `cur_energy`: the kept state's;
// `nb_iter`: step() calls of the level so far, this candidate's included. The comparisons are written as the reference
// writes them (a NaN energy is accepted and stops the level), and 0.1f * lm_coef keeps its operand order.
enum LmVerdict { LM_REJECTED_GO_ON = 0, LM_REJECTED_STOP = 1, LM_ACCEPTED_GO_ON = 2, LM_ACCEPTED_STOP = 3 };
VORS_HD bool lm_too_many_iterations(int nb_iter) { return nb_iter > 20; }
VORS_HD LmVerdict lm_verdict(float energy, float cur_energy, int nb_iter, float& lm_coef) {
    const bool too_many_iterations = lm_too_many_iterations(nb_iter);
    if (energy > cur_energy) {  // Err(energy)
        if (too_many_iterations) return LM_REJECTED_STOP;
        lm_coef *= 10.0f;
        return LM_REJECTED_GO_ON;
    }
    const float d_energy = cur_energy - energy;
    if (too_many_iterations) return LM_ACCEPTED_STOP;
    lm_coef = 0.1f * lm_coef;
    if (!(d_energy > 1.0f)) return LM_ACCEPTED_STOP;
    return LM_ACCEPTED_GO_ON;
}
VORS_HD bool lm_accepted(LmVerdict v) { return v >= LM_ACCEPTED_GO_ON; }
VORS_HD bool lm_stops(LmVerdict v) { return (v & 1) != 0; }

// Per-level pinhole intrinsics; reference: src/core/camera.rs:84-140.
struct Intr {
    float cu, cv, fu, fv, skew;
};
VORS_HD Intr intr_half_res(const Intr& k) {  // camera.rs:115-123 (skew left unscaled, as in the reference)
    return Intr{(k.cu + 0.5f) / 2.0f - 0.5f, (k.cv + 0.5f) / 2.0f - 0.5f, 0.5f * k.fu, 0.5f * k.fv, k.skew};
}
VORS_HD V3 back_project(const Intr& k, float px, float py, float depth) {  // camera.rs:135-140
    const float z = depth;
    const float y = (py - k.cv) * z / k.fv;
    const float x = ((px - k.cu) * z - k.skew * y) / k.fu;
    return V3{x, y, z};
}
// project + perspective division: camera.rs:126-132 and lm_optimizer.rs:217-218.
VORS_HD void project_uv(const Intr& k, const V3& p, float* u, float* v) {
    const float pu = (k.fu * p.x + k.skew * p.y) + k.cu * p.z;
    const float pv = k.fv * p.y + k.cv * p.z;
    *u = pu / p.z;
    *v = pv / p.z;
}
// Intrinsics::project, camera.rs:126-132: the homogeneous image point (no perspective division).
VORS_HD V3 intr_project(const Intr& k, const V3& p) {
    return V3{(k.fu * p.x + k.skew * p.y) + k.cu * p.z, k.fv * p.y + k.cv * p.z, p.z};
}
// extrinsics::project, camera.rs:70-72: world -> camera, rotation.inverse() * (translation.inverse() * point).
VORS_HD V3 extr_project(const Iso& pose, const V3& p) {
    const Quat qi{-pose.q.i, -pose.q.j, -pose.q.k, pose.q.w};
    return quat_rotate(qi, V3{p.x + -pose.t.x, p.y + -pose.t.y, p.z + -pose.t.z});
}
// One point of a world-frame list seen from a camera (the renderer of the keyframe map): c = extr_project(pose, w) — with no
// pose (has_pose false: `pose` is not read) c = w, no transform at all, the rule of vors_batch_point_cloud —, Z' = c.z, (u, v) = project_uv(K, c): existing texts, unchanged, so
// (u Z', v Z', Z') has the bits of vors_camera_project. The footprint is anchored at (x0, y0): footprint 1 the one pixel
// (floorf(u + 0.5f), floorf(v + 0.5f)), the landing rule of the depth reprojection; 2 the four pixels floorf(u) + {0, 1}, floorf(v) + {0, 1};
// 3 the nine pixels around footprint 1's. The point is a candidate iff Z' > 0 and the anchor lies within four pixels of the window, compared
// in float BEFORE any integer conversion, so that NaN and huge values fail and no out-of-range float is ever converted. A footprint pixel
// is written iff it lies inside [0, cols) x [0, rows), tested in integers (render_footprint). The one text the host entry
// (vors_render_points_host) and the device kernel (render_kernels.hip render_splat_kernel) both run, bit for bit.
struct RenderPoint {
    float z;        // Z'
    int x0, y0;     // the anchor; meaningful only for a candidate
    bool in_front;  // Z' > 0
    bool candidate;
};
VORS_HD RenderPoint render_point(const Intr& k, bool has_pose, const Iso& pose, const V3& w, int footprint, int cols, int rows) {
    const V3 c = has_pose ? extr_project(pose, w) : w;
    float u, v;
    project_uv(k, c, &u, &v);
    const float x0f = footprint == 2 ? floorf(u) : floorf(u + 0.5f), y0f = footprint == 2 ? floorf(v) : floorf(v + 0.5f);
    RenderPoint p{c.z, 0, 0, c.z > 0.0f, false};
    p.candidate = p.in_front && (x0f >= -4.0f) && (x0f < (float)cols + 4.0f) && (y0f >= -4.0f) && (y0f < (float)rows + 4.0f);
    if (p.candidate) {
        p.x0 = (int)x0f;
        p.y0 = (int)y0f;
    }
    return p;
}
// The pixels of a candidate's footprint that lie inside the window, in row-major order of the footprint: write(y * cols + x) for each.
// Returns whether there was one (the point "lands").
template <class Write>
VORS_HD bool render_footprint(const RenderPoint& p, int footprint, int cols, int rows, Write&& write) {
    const int lo = footprint == 3 ? -1 : 0, hi = footprint == 1 ? 0 : 1;
    bool landed = false;
    for (int dy = lo; dy <= hi; ++dy)
        for (int dx = lo; dx <= hi; ++dx) {
            const int x = p.x0 + dx, y = p.y0 + dy;
            if (x >= 0 && x < cols && y >= 0 && y < rows) {
                write(y * cols + x);
                landed = true;
            }
        }
    return landed;
}
// Key of a point in the keyed z-buffer: bits(Z') << 32 | rank. Z' > 0 orders as its bits, so the unsigned minimum picks the nearest surface
// and, among equal Z' bits, the lowest rank; all ones (VORS_ZKEY_EMPTY) is no point.
VORS_HD uint64_t render_key(float z, uint32_t rank) { return ((uint64_t)__builtin_bit_cast(uint32_t, z) << 32) | (uint64_t)rank; }
// One pixel of the key plane resolved: depth = to_depth(scale, 1.0f / Z') — the bits of d_pred_depth — and the grey level of the winning
// point, both 0 where the key is empty.
struct RenderedPixel {
    uint16_t depth;
    uint8_t gray;
    bool covered;
};
VORS_HD RenderedPixel render_resolve(float depth_scale, uint64_t key, const uint8_t* list_gray) {
    if (key == 0xFFFFFFFFFFFFFFFFull) return RenderedPixel{0, 0, false};
    const float zp = __builtin_bit_cast(float, (uint32_t)(key >> 32));
    return RenderedPixel{to_depth(depth_scale, 1.0f / zp), list_gray[(uint32_t)key], true};
}

// Surface normal of one pixel of a level-0 depth plane: central differences of back-projected neighbours `step` pixels
// away, one-sided where a neighbour is missing. z(d) = 1.0f / (depth_scale / (float)d) — vors_from_depth's text, then the reciprocal the
// point cloud takes — and P(x', y') = back_project(K, (float)x', (float)y', z): the centre P_c has the camera-frame bits of
// vors_batch_point_cloud. A neighbour is usable iff it lies inside the plane, its depth is non-zero and fabsf(z_n - z_c) <= jump_m (in
// float; NaN fails). tx from (x -/+ step, y): both usable P(x + step) - P(x - step), only the right one P(x + step) - P_c, only the left
// one P_c - P(x - step), neither: no normal; ty the same with (x, y -/+ step). m = cross(ty, tx), l2 = (m.x m.x + m.y m.y) + m.z m.z, no
// normal unless l2 > 0; n = m / sqrtf(l2), three divisions; negated if (n.x P_c.x + n.y P_c.y) + n.z P_c.z > 0, so that it faces the
// camera whatever the signs of the focal lengths; with a pose quat_rotate(pose.q, n), no translation, without one n untouched. "No
// normal" is three +0.0f. The taps: depth_normal_taps gives the five flat offsets of a pixel INSIDE the plane, a tap outside the plane
// aliasing the centre (a safe address; its value is ignored), so that a kernel issues every load before the first use. The expression
// order is fixed: the one text the host entry (vors_depth_normals_host) and the device kernels (normal_kernels.hip) both run, bit for bit.
struct NormalTaps {
    int c, l, r, u, d;
};
VORS_HD NormalTaps depth_normal_taps(int x, int y, int cols, int rows, int step) {
    const int c = y * cols + x;
    return NormalTaps{c, x - step >= 0 ? c - step : c, x + step < cols ? c + step : c, y - step >= 0 ? c - step * cols : c,
                      y + step < rows ? c + step * cols : c};
}
struct DepthNormal {
    V3 n;
    bool has_depth, has_normal;
};
VORS_HD float depth_normal_z(float depth_scale, uint16_t d) { return 1.0f / (depth_scale / (float)d); }
// One tangent: `lo` / `hi` are the neighbours at -step / +step along the axis (dx, dy), in_lo / in_hi whether they lie inside the plane.
VORS_HD bool depth_normal_tangent(const Intr& k, float depth_scale, float jump_m, int x, int y, int dx, int dy, const V3& pc, bool in_lo,
                                  uint16_t lo, bool in_hi, uint16_t hi, V3* t) {
    const float z_lo = depth_normal_z(depth_scale, lo), z_hi = depth_normal_z(depth_scale, hi);
    const bool use_lo = in_lo && lo != 0 && fabsf(z_lo - pc.z) <= jump_m, use_hi = in_hi && hi != 0 && fabsf(z_hi - pc.z) <= jump_m;
    if (!use_lo && !use_hi) return false;
    const V3 a = use_lo ? back_project(k, (float)(x - dx), (float)(y - dy), z_lo) : pc;
    const V3 b = use_hi ? back_project(k, (float)(x + dx), (float)(y + dy), z_hi) : pc;
    *t = V3{b.x - a.x, b.y - a.y, b.z - a.z};
    return true;
}
VORS_HD DepthNormal depth_normal(const Intr& k, float depth_scale, int step, float jump_m, int x, int y, int cols, int rows, uint16_t dc,
                                 uint16_t dl, uint16_t dr, uint16_t du, uint16_t dd, bool has_pose, const Iso& pose) {
    DepthNormal o{V3{0.0f, 0.0f, 0.0f}, false, false};
    if (x < 0 || x >= cols || y < 0 || y >= rows || dc == 0) return o;
    o.has_depth = true;
    const V3 pc = back_project(k, (float)x, (float)y, depth_normal_z(depth_scale, dc));
    V3 tx, ty;
    if (!depth_normal_tangent(k, depth_scale, jump_m, x, y, step, 0, pc, x - step >= 0, dl, x + step < cols, dr, &tx)) return o;
    if (!depth_normal_tangent(k, depth_scale, jump_m, x, y, 0, step, pc, y - step >= 0, du, y + step < rows, dd, &ty)) return o;
    const float mx = ty.y * tx.z - ty.z * tx.y;
    const float my = ty.z * tx.x - ty.x * tx.z;
    const float mz = ty.x * tx.y - ty.y * tx.x;
    const float l2 = (mx * mx + my * my) + mz * mz;
    if (!(l2 > 0.0f)) return o;
    const float l = sqrtf(l2);
    V3 n{mx / l, my / l, mz / l};
    if ((n.x * pc.x + n.y * pc.y) + n.z * pc.z > 0.0f) n = V3{-n.x, -n.y, -n.z};
    o.n = has_pose ? quat_rotate(pose.q, n) : n;
    o.has_normal = true;
    return o;
}

// The sensor front end (the reference has none): undistortion of grey and depth planes into an ideal pinhole camera, and
// registration of a depth camera's planes into a colour camera. K_in / dist = the real camera and its Brown-Conrady coefficients
// k1 k2 p1 p2 k3, K_out = the ideal camera of the output plane.
// SOURCE COORDINATE of output pixel (x, y): (X, Y, 1) = back_project(K_out, (float)x, (float)y, 1.0f), the distorted normalised point
// (Xd, Yd) and (u, v) = K_in (Xd, Yd, 1), in the written order, no FMA (-ffp-contract=off):
//   xx = X X, yy = Y Y, xy = X Y, r2 = xx + yy, rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
//   Xd = (X rad + (2 p1) xy) + p2 (r2 + 2 xx),  Yd = (Y rad + p1 (r2 + 2 yy)) + (2 p2) xy
//   u = (fu Xd + skew Yd) + cu,  v = fv Yd + cv
// GREY, bilinear in lerp form: inside iff 0 <= u <= cols - 1 and 0 <= v <= rows - 1, compared in float BEFORE any conversion (NaN
// fails); border 1 clamps u and v into the plane first (edge replicate; a NaN coordinate still fails). x0 = floorf(u), a = u - x0,
// x1 = min(x0 + 1, cols - 1), rows likewise with b; t0 = I00 + a (I01 - I00), t1 = I10 + a (I11 - I10), val = t0 + b (t1 - t0);
// the output floorf(val + 0.5f) clamped to 0..255, 0 outside. The taps of a pixel outside alias pixel 0 (a safe address; the value is
// ignored), so that a kernel issues every load before the first use.
// DEPTH, never interpolated: xs = floorf(u + 0.5f), ys = floorf(v + 0.5f) (the landing rule of the depth reprojection), D[ys][xs] if
// that pixel lies inside the plane (in float), else 0; the border mode does not apply.
// The one text the host entries (vors_undistort_frame_host, vors_undistort_source_host) and the device kernel (frontend_kernels.hip
// undistort_kernel) both run, bit for bit.
struct Dist5 {
    float k1, k2, p1, p2, k3;
};
VORS_HD void undistort_source(const Intr& k_out, const Intr& k_in, const Dist5& d, int x, int y, float* u, float* v) {
    const V3 p = back_project(k_out, (float)x, (float)y, 1.0f);
    const float X = p.x, Y = p.y;
    const float xx = X * X, yy = Y * Y, xy = X * Y;
    const float r2 = xx + yy;
    const float rad = 1.0f + r2 * (d.k1 + r2 * (d.k2 + r2 * d.k3));
    const float Xd = (X * rad + (2.0f * d.p1) * xy) + d.p2 * (r2 + 2.0f * xx);
    const float Yd = (Y * rad + d.p1 * (r2 + 2.0f * yy)) + (2.0f * d.p2) * xy;
    *u = (k_in.fu * Xd + k_in.skew * Yd) + k_in.cu;
    *v = k_in.fv * Yd + k_in.cv;
}
VORS_HD bool undistort_inside(float u, float v, int cols, int rows) {
    return u >= 0.0f && u <= (float)(cols - 1) && v >= 0.0f && v <= (float)(rows - 1);
}
struct UndistortTaps {
    int i00, i01, i10, i11;  // flat offsets into the grey plane
    float a, b;
    bool ok;     // the output is interpolated (else 0)
    bool inside; // the coordinate itself lies inside the plane, whatever the border mode (the counter)
    int depth;   // flat offset of the depth pixel, -1 = outside
};
VORS_HD UndistortTaps undistort_taps(float u, float v, int border, int cols, int rows) {
    UndistortTaps t{0, 0, 0, 0, 0.0f, 0.0f, false, undistort_inside(u, v, cols, rows), -1};
    const float xs = floorf(u + 0.5f), ys = floorf(v + 0.5f);
    if (undistort_inside(xs, ys, cols, rows)) t.depth = (int)ys * cols + (int)xs;
    float uc = u, vc = v;
    if (border == 1 && u == u && v == v) {  // (NaN stays NaN and fails below)
        const float cmax = (float)(cols - 1), rmax = (float)(rows - 1);
        uc = u < 0.0f ? 0.0f : u > cmax ? cmax : u;
        vc = v < 0.0f ? 0.0f : v > rmax ? rmax : v;
    }
    t.ok = undistort_inside(uc, vc, cols, rows);
    if (t.ok) {
        const float x0f = floorf(uc), y0f = floorf(vc);
        const int x0 = (int)x0f, y0 = (int)y0f;
        const int x1 = x0 + 1 < cols - 1 ? x0 + 1 : cols - 1, y1 = y0 + 1 < rows - 1 ? y0 + 1 : rows - 1;
        t.a = uc - x0f;
        t.b = vc - y0f;
        t.i00 = y0 * cols + x0;
        t.i01 = y0 * cols + x1;
        t.i10 = y1 * cols + x0;
        t.i11 = y1 * cols + x1;
    }
    return t;
}
VORS_HD uint8_t undistort_gray(const UndistortTaps& t, uint8_t i00, uint8_t i01, uint8_t i10, uint8_t i11) {
    if (!t.ok) return 0;
    const float f00 = (float)i00, f01 = (float)i01, f10 = (float)i10, f11 = (float)i11;
    const float t0 = f00 + t.a * (f01 - f00), t1 = f10 + t.a * (f11 - f10);
    const float val = t0 + t.b * (t1 - t0);
    const float r = floorf(val + 0.5f);
    if (!(r > 0.0f)) return 0;
    if (r >= 255.0f) return 255;
    return (uint8_t)(int)r;
}
// REGISTRATION of source pixel (x, y) of a pinhole depth camera K_d with d != 0: z = depth_normal_z(scale_in, d),
// P = back_project(K_d, (float)x, (float)y, z) — the camera-frame bits of the point cloud — carried into the colour camera by the depth
// camera -> colour camera pose with the point cloud's text (iso_transform_point: rotate, then add the translation; without a pose P
// untouched). The point then goes through render_point(K_c, no pose, ...), render_footprint and render_key(Z', s), s = y * d_cols + x,
// unchanged. A key resolves to to_depth(scale_out, 1.0f / Z') and the winning s; an empty key to 0 and 0xFFFFFFFF. The one text the host
// entry (vors_register_depth_host) and the device kernels (frontend_kernels.hip) both run, bit for bit.
VORS_HD V3 register_point(const Intr& k_d, float scale_in, bool has_pose, const Iso& pose, int x, int y, uint16_t d) {
    const V3 p = back_project(k_d, (float)x, (float)y, depth_normal_z(scale_in, d));
    return has_pose ? iso_transform_point(pose, p) : p;
}
struct RegisteredPixel {
    uint16_t depth;
    uint32_t src;
    bool covered;
};
VORS_HD RegisteredPixel register_resolve(float scale_out, uint64_t key) {
    if (key == 0xFFFFFFFFFFFFFFFFull) return RegisteredPixel{0, 0xFFFFFFFFu, false};
    const float zp = __builtin_bit_cast(float, (uint32_t)(key >> 32));
    return RegisteredPixel{to_depth(scale_out, 1.0f / zp), (uint32_t)key, true};
}

// Projective point-to-plane ICP of a world-frame point list with normals against a level-0 depth plane (the reference has
// none). T = the camera -> world pose being refined, w / nw = a world point and its world normal (three zeros: no normal). Everything in
// the camera frame, existing texts unchanged: c = extr_project(T, w); the landing pixel (x, y) = render_point's footprint-1 anchor, which
// must lie inside the plane (integers); d = D[y][x]; q = back_project(K, (float)x, (float)y, depth_normal_z(depth_scale, d)); e = q - c.
// MATCHED iff the point is a candidate that lands inside the plane, its normal is not three zeros, d != 0 and
// dot3(e, e) <= dist_m * dist_m (in float; NaN fails). n = quat_rotate(conj(T.q), nw); the residual r = dot3(n, e); the Jacobian row
// J = (n, cross(q, n)): the derivative of n . (exp(xi) q - c) at xi = 0, n . v + w . (q x n) for xi = (v, w) — the translational three,
// then the rotational three, the order se3_exp reads its argument (checked against central differences of se3_exp in f64:
// tests/test_icp_host.py test_jacobian_rule). The minimiser of sum (r + J xi)^2 is xi = -delta with H delta = g, H = sum J^T J,
// g = sum J r: the measured cloud moves by exp(delta)^-1 in the camera frame, so the camera moves to T * exp(delta)^-1 — lm_step's update.
// A row is a[7] = {r, J[0..5]}; an unmatched point's row is seven +0.0f, so that each of its products is +0.0f.
// The two halves are separate so that a kernel issues the gather of d between them. The one text the host entry (vors_icp_points_host) and
// the device kernels (icp_kernels.hip) both run, bit for bit.
struct IcpLanding {
    V3 c;
    int x, y;    // meaningful only when the point lands
    bool lands;  // a candidate whose pixel lies inside the plane
};
VORS_HD IcpLanding icp_landing(const Intr& k, const Iso& pose, const V3& w, int cols, int rows) {
    const RenderPoint rp = render_point(k, true, pose, w, 1, cols, rows);
    IcpLanding o{extr_project(pose, w), 0, 0, false};
    if (rp.candidate && rp.x0 >= 0 && rp.x0 < cols && rp.y0 >= 0 && rp.y0 < rows) {
        o.x = rp.x0;
        o.y = rp.y0;
        o.lands = true;
    }
    return o;
}
VORS_HD bool icp_row(const Intr& k, float depth_scale, float dist_m, const Iso& pose, const IcpLanding& l, const V3& nw, uint16_t d, float a[7]) {
VORS_UNROLL
    for (int i = 0; i < 7; ++i) a[i] = 0.0f;
    const bool has_normal = !(nw.x == 0.0f && nw.y == 0.0f && nw.z == 0.0f);
    if (!l.lands || !has_normal || d == 0) return false;
    const V3 q = back_project(k, (float)l.x, (float)l.y, depth_normal_z(depth_scale, d));
    const V3 e{q.x - l.c.x, q.y - l.c.y, q.z - l.c.z};
    if (!(dot3(e, e) <= dist_m * dist_m)) return false;
    const V3 n = quat_rotate(Quat{-pose.q.i, -pose.q.j, -pose.q.k, pose.q.w}, nw);
    const V3 m = cross(q, n);
    a[0] = dot3(n, e);
    a[1] = n.x; a[2] = n.y; a[3] = n.z;
    a[4] = m.x; a[5] = m.y; a[6] = m.z;
    return true;
}
// The 28 products of a row, in the order of sums29's slots 0, 2..7, 8..28 (vors_batch_eval_level): r r, J[i] r, J[i] J[j] for i <= j row-wise.
#define VORS_ICP_SUMS 28
VORS_HD void icp_products(const float a[7], float p[VORS_ICP_SUMS]) {
    int k = 0;
    p[k++] = a[0] * a[0];
VORS_UNROLL
    for (int i = 1; i < 7; ++i) p[k++] = a[i] * a[0];
VORS_UNROLL
    for (int i = 1; i < 7; ++i)
VORS_UNROLL
        for (int j = i; j < 7; ++j) p[k++] = a[i] * a[j];
}
// The robust rule (vors_icp_points_robust): icp_row's tests in icp_row's order and arithmetic, then — NORMALS — the gate
// against the frame's own normal at the landing pixel, nf (camera frame, vors_depth_normals' output without a pose; three zeros = none):
// MATCHED only if nf is not three zeros and dot3(n, nf) >= min_cos in float (NaN fails). Both normals face their camera, so any
// min_cos > 0 culls a back-facing model point. -> the last gate passed, which is what vors_icp_points_robust's gate counts count;
// ICP_GATE_MATCHED is icp_row's `true`, and only then is the row other than seven +0.0f. NORMALS = false is icp_row's arithmetic.
enum IcpGate { ICP_GATE_NONE = 0, ICP_GATE_DEPTH = 1, ICP_GATE_DIST = 2, ICP_GATE_MATCHED = 3 };
template <bool NORMALS>
VORS_HD IcpGate icp_row_robust(const Intr& k, float depth_scale, float dist_m, float min_cos, const Iso& pose, const IcpLanding& l, const V3& nw,
                               uint16_t d, const V3& nf, float a[7]) {
VORS_UNROLL
    for (int i = 0; i < 7; ++i) a[i] = 0.0f;
    const bool has_normal = !(nw.x == 0.0f && nw.y == 0.0f && nw.z == 0.0f);
    if (!l.lands || !has_normal || d == 0) return ICP_GATE_NONE;
    const V3 q = back_project(k, (float)l.x, (float)l.y, depth_normal_z(depth_scale, d));
    const V3 e{q.x - l.c.x, q.y - l.c.y, q.z - l.c.z};
    if (!(dot3(e, e) <= dist_m * dist_m)) return ICP_GATE_DEPTH;
    const V3 n = quat_rotate(Quat{-pose.q.i, -pose.q.j, -pose.q.k, pose.q.w}, nw);
    if (NORMALS) {
        const bool has_frame_normal = !(nf.x == 0.0f && nf.y == 0.0f && nf.z == 0.0f);
        if (!has_frame_normal || !(dot3(n, nf) >= min_cos)) return ICP_GATE_DIST;
    }
    const V3 m = cross(q, n);
    a[0] = dot3(n, e);
    a[1] = n.x; a[2] = n.y; a[3] = n.z;
    a[4] = m.x; a[5] = m.y; a[6] = m.z;
    return ICP_GATE_MATCHED;
}
// The 28 products under the Huber weight of the LM kernels (lm_reference.hip refw_residual2 / refw_products_of), huber_m > 0:
// ar = |r|, lin = ar <= huber_m, w = lin ? 1 : huber_m / ar, e = lin ? r r : huber_m (2 ar - huber_m), wr = w r; the products are e,
// J[i] wr, w (J[i] J[j]) in icp_products' slots — slot 0 is then the Huber loss, not the sum of squares. -> the point lies on the
// linear branch (|r| > huber_m); a row of zeros gives +0.0f everywhere and false. HUBER = false is icp_products' own text.
template <bool HUBER>
VORS_HD bool icp_products_robust(const float a[7], float huber_m, float p[VORS_ICP_SUMS]) {
    if (!HUBER) {
        icp_products(a, p);
        return false;
    }
    const float r = a[0], ar = fabsf(r);
    const bool lin = ar <= huber_m;
    const float w = lin ? 1.0f : huber_m / ar;
    const float e = lin ? r * r : huber_m * (2.0f * ar - huber_m);
    const float wr = w * r;
    int k = 0;
    p[k++] = e;
VORS_UNROLL
    for (int i = 1; i < 7; ++i) p[k++] = a[i] * wr;
VORS_UNROLL
    for (int i = 1; i < 7; ++i)
VORS_UNROLL
        for (int j = i; j < 7; ++j) p[k++] = w * (a[i] * a[j]);
    return !lin;
}
// The joint rule (vors_icp_points_joint): icp_row_robust's row, and for a MATCHED point a PHOTOMETRIC row against the
// frame's level-0 grey plane G, which holds what point-to-plane leaves free — the translation inside the plane, the rotation about its
// normal. With c = l.c and (u, v) = project_uv(K, c): x0f = floorf(u), y0f = floorf(v); the bilinear footprint lies inside G iff
// x0f >= 0 && x0f + 1 <= cols - 1 && y0f >= 0 && y0f + 1 <= rows - 1, compared in float BEFORE any integer conversion (render_point's
// convention: NaN fails, no out-of-range float is converted). PHOTO iff photo_scale_m > 0, the point is MATCHED and its footprint is
// inside. fx = u - x0f, fy = v - y0f; the taps I00 = G[y0][x0], I10 = G[y0][x0 + 1], I01 = G[y0 + 1][x0], I11 = G[y0 + 1][x0 + 1] as
// float; top = I00 + fx (I10 - I00), bot = I01 + fx (I11 - I01), I = top + fy (bot - top); gx = (1 - fy)(I10 - I00) + fy (I11 - I01),
// gy = (1 - fx)(I01 - I00) + fx (I11 - I10): the exact derivatives of the interpolant, no gradient image. (The LM kernels' bilinear text,
// lm_sources.h bilinear_residual, is a device function over their own records and gives no derivative: this is a text of its own.)
// d = I - (float)grey_w in grey levels, r_p = s d with s = photo_scale_m (metres per grey level: both residuals in one unit).
// Jacobian, icp_row's convention — the camera moves to T exp(xi), so c(xi) = exp(xi)^-1 c = c - v - w x c + ...: iz = 1 / z,
// du/dc = (fu iz, skew iz, -((fu x + skew y) iz) iz), dv/dc = (0, fv iz, -((fv y) iz) iz), a = s (gx du/dc + gy dv/dc),
// J_p = (-a, cross(a, c)) (checked against central differences of se3_exp in f64: tests/test_icp_joint_host.py test_jacobian_rule).
// The row is a[7] = {r_p, J_p}; a point that is not PHOTO has seven +0.0f and contributes its geometric products ALONE (nothing is
// added to them, so that photo_scale_m = 0 is vors_icp_points_robust bit for bit; -0.0f + +0.0f would be +0.0f). A PHOTO point's 28
// products are p_g[k] + p_p[k] in f32, geometric first, p_p = icp_products_robust<PHUBER>(a_p, photo_huber_m).
// The two halves are separate so that a kernel issues the four gathers between them; a footprint that is not inside has offset 0.
struct IcpFootprint {
    float fx, fy;
    int off;      // y0 * cols + x0; 0 unless inside (a safe address when the plane has two rows and two columns)
    bool inside;
};
VORS_HD IcpFootprint icp_photo_footprint(const Intr& k, const V3& c, int cols, int rows) {
    float u, v;
    project_uv(k, c, &u, &v);
    const float x0f = floorf(u), y0f = floorf(v);
    IcpFootprint f{0.0f, 0.0f, 0, false};
    f.inside = (x0f >= 0.0f) && (x0f + 1.0f <= (float)(cols - 1)) && (y0f >= 0.0f) && (y0f + 1.0f <= (float)(rows - 1));
    if (f.inside) {
        f.fx = u - x0f;
        f.fy = v - y0f;
        f.off = (int)y0f * cols + (int)x0f;
    }
    return f;
}
// -> d = I - grey in grey levels (meaningful only when `photo`, which the caller decides: MATCHED && f.inside && photo_scale_m > 0).
VORS_HD float icp_row_photo(const Intr& k, float photo_scale_m, const V3& c, const IcpFootprint& f, bool photo, uint8_t t00, uint8_t t10,
                            uint8_t t01, uint8_t t11, uint8_t grey_w, float a[7]) {
VORS_UNROLL
    for (int i = 0; i < 7; ++i) a[i] = 0.0f;
    if (!photo) return 0.0f;
    const float i00 = (float)t00, i10 = (float)t10, i01 = (float)t01, i11 = (float)t11;
    const float dx0 = i10 - i00, dx1 = i11 - i01;
    const float top = i00 + f.fx * dx0, bot = i01 + f.fx * dx1;
    const float im = top + f.fy * (bot - top);
    const float gx = (1.0f - f.fy) * dx0 + f.fy * dx1;
    const float gy = (1.0f - f.fx) * (i01 - i00) + f.fx * (i11 - i10);
    const float d = im - (float)grey_w;
    const float iz = 1.0f / c.z;
    const float dux = k.fu * iz, duy = k.skew * iz, duz = -(((k.fu * c.x + k.skew * c.y) * iz) * iz);
    const float dvy = k.fv * iz, dvz = -(((k.fv * c.y) * iz) * iz);
    const V3 g{photo_scale_m * (gx * dux), photo_scale_m * (gx * duy + gy * dvy), photo_scale_m * (gx * duz + gy * dvz)};
    const V3 m = cross(g, c);
    a[0] = photo_scale_m * d;
    a[1] = -g.x; a[2] = -g.y; a[3] = -g.z;
    a[4] = m.x; a[5] = m.y; a[6] = m.z;
    return d;
}
// The clipped range of ranks of a list (render_splat_kernel's text): count clipped to capacity, range2 (nullable) = (first, count).
VORS_HD void icp_range(uint32_t count, int capacity, const uint32_t* range2, uint32_t* first, uint32_t* last) {
    const uint32_t n = count < (uint32_t)capacity ? count : (uint32_t)capacity;
    *first = 0;
    *last = n;
    if (range2) {
        *first = range2[0] < n ? range2[0] : n;
        *last = range2[1] > n - *first ? n : *first + range2[1];
    }
}
// ORDER OF THE SUMS: the clipped range is cut into chunks of VORS_ICP_CHUNK consecutive ranks from `first`; slot s of a chunk is a rank's
// offset in it, slots beyond the range hold zeros. Chunk sum: the halving tree for (w = 512; w >= 1; w /= 2) v[s] = v[s] + v[s + w] for
// s < w, in f32, per product. List sum: the chunk sums added sequentially in ascending chunk order, starting from chunk 0's. The matched
// counts are integers. Neither capacity nor the grid nor the schedule enters.
#define VORS_ICP_CHUNK 1024
// One round's verdict from the list sums: the statuses of vors_icp_points. H is mirrored from the 21 sums, g = sums[1..6]; the step is
// lm_step's (the existing text), delta = cholesky6_solve's solution of the same system, kept for the convergence test.
enum IcpStatus { ICP_ITERATIONS = 0, ICP_CONVERGED = 1, ICP_TOO_FEW = 2, ICP_SINGULAR = 3 };
VORS_HD float dot6(const float* a, const float* b) {
    return ((((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]) + a[4] * b[4]) + a[5] * b[5];
}
// -> ICP_ITERATIONS: *pose moved, go on; ICP_CONVERGED: *pose moved, stop; ICP_TOO_FEW / ICP_SINGULAR: *pose kept, stop.
VORS_HD IcpStatus icp_round(const float sums[VORS_ICP_SUMS], uint32_t matched, uint32_t min_points, float damping, float step_eps, Iso* pose,
                            float* step_norm) {
    if (matched < min_points) return ICP_TOO_FEW;
    float h[36], delta[6];
    int k = 7;
VORS_UNROLL
    for (int r = 0; r < 6; ++r)
VORS_UNROLL
        for (int c = r; c < 6; ++c) h[r * 6 + c] = h[c * 6 + r] = sums[k++];
    Iso next;
    if (!cholesky6_solve(h, sums + 1, damping, delta) || !lm_step(h, sums + 1, *pose, damping, &next)) return ICP_SINGULAR;
    *pose = next;
    const float d2 = dot6(delta, delta);
    *step_norm = sqrtf(d2);
    return d2 <= step_eps * step_eps ? ICP_CONVERGED : ICP_ITERATIONS;
}
// sums29 of vors_batch_eval_level from the 28 list sums and the matched count (slot 1).
VORS_HD void icp_sums29(const float sums[VORS_ICP_SUMS], uint32_t matched, float* out29) {
    out29[0] = sums[0];
    out29[1] = (float)matched;
VORS_UNROLL
    for (int i = 1; i < VORS_ICP_SUMS; ++i) out29[i + 1] = sums[i];
}

// The map ICP correction at keyframe promotion (vors_trackers_enable_map_icp): its two rules, each ONE text, run by the
// host twins (vors_map_icp_window_host, vors_map_icp_verdict_host) and by map_icp_arm_kernel / map_icp_apply_kernel.
// WINDOW: the ranks of a sequence's map the new keyframe is aligned against. DEFINITION: n_rec = min(n_segments, max_keyframes),
// total = min(count, capacity); first = 0 when last_keyframes == 0 or n_rec <= last_keyframes, otherwise the `first` of recorded segment
// n_rec - last_keyframes, clipped to total; the window is (first, total - first): it always runs to the end of the list, so the points of
// keyframes beyond max_keyframes stay inside it. segment_words: the sequence's vors_map_segment records as 32-bit words, ten per record,
// `first` at word 1 (read only in the second case).
#define MAP_SEGMENT_WORDS 10
VORS_HD void map_icp_window(const uint32_t* segment_words, uint32_t n_segments, int max_keyframes, uint32_t count, int capacity, int last_keyframes,
                            uint32_t range2[2]) {
    const uint32_t n_rec = n_segments < (uint32_t)max_keyframes ? n_segments : (uint32_t)max_keyframes;
    const uint32_t total = count < (uint32_t)capacity ? count : (uint32_t)capacity;
    uint32_t first = 0;
    if (last_keyframes != 0 && n_rec > (uint32_t)last_keyframes) {
        first = segment_words[(size_t)(n_rec - (uint32_t)last_keyframes) * MAP_SEGMENT_WORDS + 1];
        if (first > total) first = total;
    }
    range2[0] = first;
    range2[1] = total - first;
}
// VERDICT on one alignment. DEFINITION: the tests run in this order and the first failure names the verdict; every comparison is in
// float and NaN fails. 1 NONFINITE: any of pose_after's seven numbers is not finite. 2 ICP_STATUS: the status is neither ITERATIONS nor
// CONVERGED (rms is read only behind this test: it is NaN when nothing matched). 3 FEW_MATCHES: (float)matched >= min_match_ratio *
// (float)considered does not hold. 4 RMS: rms <= max_rms does not hold. 5 STEP: with D = inverse(pose_before) * pose_after (iso_inverse,
// iso_mul), dot3(D.t, D.t) <= max_trans_m * max_trans_m or fabsf(D.q.w) >= cos_half_rot does not hold; cos_half_rot =
// cosf(0.5f * max_rot_rad) is evaluated once, on the host, when the stage is enabled, and handed to the kernel and the twin alike.
enum MapIcpVerdict {
    MAP_ICP_NOT_ATTEMPTED = 0, MAP_ICP_ACCEPTED = 1, MAP_ICP_ICP_STATUS = 2, MAP_ICP_FEW_MATCHES = 3, MAP_ICP_RMS = 4, MAP_ICP_STEP = 5,
    MAP_ICP_NONFINITE = 6
};
struct MapIcpGates {
    float min_match_ratio, max_rms, max_trans_m, cos_half_rot;
};
VORS_HD bool f32_finite(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}
VORS_HD MapIcpVerdict map_icp_verdict(const MapIcpGates& g, uint32_t status, uint32_t matched, uint32_t considered, float rms,
                                      const float pose_before[7], const float pose_after[7]) {
VORS_UNROLL
    for (int i = 0; i < 7; ++i)
        if (!f32_finite(pose_after[i])) return MAP_ICP_NONFINITE;
    if (status != (uint32_t)ICP_ITERATIONS && status != (uint32_t)ICP_CONVERGED) return MAP_ICP_ICP_STATUS;
    if (!((float)matched >= g.min_match_ratio * (float)considered)) return MAP_ICP_FEW_MATCHES;
    if (!(rms <= g.max_rms)) return MAP_ICP_RMS;
    const Iso d = iso_mul(iso_inverse(iso_load(pose_before)), iso_load(pose_after));
    if (!(dot3(d.t, d.t) <= g.max_trans_m * g.max_trans_m)) return MAP_ICP_STEP;
    if (!(fabsf(d.q.w) >= g.cos_half_rot)) return MAP_ICP_STEP;
    return MAP_ICP_ACCEPTED;
}

// The correction with the joint pass and a test on the conditioning of H (vors_trackers_enable_map_icp_joint): two rules,
// each ONE text, run by the host entries (vors_icp_condition_from_sums, vors_map_icp_verdict_joint_host) and by icp_condition_kernel /
// map_icp_apply_joint_kernel.
// CONDITION: the "dilution of precision" of an ICP system from the 29 sums of one evaluation (slot 1 = matched count n, slots 8..28 =
// the upper triangle of H). H is mirrored from the sums, UNDAMPED, and factored by the left-looking lower Cholesky in f64, in
// pose_information's order; C = H^-1 = L^-T L^-1 in f64; tt = (C00 + C11) + C22, rr = (C33 + C44) + C55;
// dilution_t = (float)sqrt((double)n * tt), dilution_r = (float)sqrt((double)n * rr). Geometric and photometric rows are both in metres,
// so dilution_t has no unit and dilution_r is in 1/m. Neither the list length nor the residuals enter: sigma2 of pose_information does,
// and a perfect synthetic scene, whose rms tends to 0, would pass any bound on its covariance while it slides. With Huber weights H is
// the WEIGHTED matrix; that is accepted. -> flags: bit 0 = !(n > 6.0f) (a NaN count too), bit 1 = a pivot that is not > 0 (no early
// exit: as in pose_information, the factorisation runs on and what it then holds is never handed out); with either, both dilutions are
// NaN. Both outputs are nullable. A second text of the factorisation and the inverse beside pose_information's, on purpose: that function
// and its kernel stay word for word as they are, and only the diagonal of C is formed here.
VORS_HD int icp_condition(const float* sums29, float* dilution_t, float* dilution_r) {
    double a[6][6];
    int k = 8;
VORS_UNROLL
    for (int r = 0; r < 6; ++r)
VORS_UNROLL
        for (int c = r; c < 6; ++c) {
            const double v = (double)sums29[k++];
            a[r][c] = a[c][r] = v;
        }
    int flags = (sums29[1] > 6.0f) ? 0 : 1;
    bool pivots_ok = true;
VORS_UNROLL
    for (int j = 0; j < 6; ++j) {
VORS_UNROLL
        for (int q = 0; q < j; ++q)
VORS_UNROLL
            for (int i = j; i < 6; ++i) a[i][j] -= a[j][q] * a[i][q];
        pivots_ok = pivots_ok && a[j][j] > 0.0;
        const double d = sqrt(a[j][j]);
        a[j][j] = d;
VORS_UNROLL
        for (int i = j + 1; i < 6; ++i) a[i][j] /= d;
    }
    if (!pivots_ok) flags |= 2;
    if (flags) {
        const float nan = nanf("");
        if (dilution_t) *dilution_t = nan;
        if (dilution_r) *dilution_r = nan;
        return flags;
    }
    double inv[6][6];  // L^-1, lower triangular, column by column (forward substitution on the unit vectors)
VORS_UNROLL
    for (int c = 0; c < 6; ++c)
VORS_UNROLL
        for (int r = 0; r < 6; ++r) {
            if (r < c) {
                inv[r][c] = 0.0;
                continue;
            }
            double t = r == c ? 1.0 : 0.0;
VORS_UNROLL
            for (int q = c; q < r; ++q) t -= a[r][q] * inv[q][c];
            inv[r][c] = t / a[r][r];
        }
    double diag[6];  // (L^-T L^-1)[r][r]
VORS_UNROLL
    for (int r = 0; r < 6; ++r) {
        double t = 0.0;
VORS_UNROLL
        for (int q = r; q < 6; ++q) t += inv[q][r] * inv[q][r];
        diag[r] = t;
    }
    const double n = (double)sums29[1];
    const double tt = (diag[0] + diag[1]) + diag[2], rr = (diag[3] + diag[4]) + diag[5];
    if (dilution_t) *dilution_t = (float)sqrt(n * tt);
    if (dilution_r) *dilution_r = (float)sqrt(n * rr);
    return flags;
}
// VERDICT of the joint stage. DEFINITION: map_icp_verdict as it stands; only behind ACCEPTED it returns CONDITION (7, the value of
// VORS_MAP_ICP_CONDITION) when a bound is > 0 and dilution <= bound does not hold — dilution_t first — compared in float, NaN fails: a
// failed Cholesky therefore fails every bound that is on. With both bounds 0 it is map_icp_verdict for every input.
#define MAP_ICP_CONDITION 7u
struct MapIcpConditionGates {
    float max_dilution_t, max_dilution_r;
};
VORS_HD uint32_t map_icp_verdict_joint(const MapIcpGates& g, const MapIcpConditionGates& cg, uint32_t status, uint32_t matched, uint32_t considered,
                                       float rms, const float pose_before[7], const float pose_after[7], float dilution_t, float dilution_r) {
    const MapIcpVerdict v = map_icp_verdict(g, status, matched, considered, rms, pose_before, pose_after);
    if (v != MAP_ICP_ACCEPTED) return (uint32_t)v;
    if (cg.max_dilution_t > 0.0f && !(dilution_t <= cg.max_dilution_t)) return MAP_ICP_CONDITION;
    if (cg.max_dilution_r > 0.0f && !(dilution_r <= cg.max_dilution_r)) return MAP_ICP_CONDITION;
    return (uint32_t)MAP_ICP_ACCEPTED;
}

// Jacobian of the warp: src/core/track/inverse_compositional.rs:313-341.
VORS_HD void warp_jacobian_at(float gu, float gv, float u, float v, float _z, const Intr& k, float J[6]) {
    const float a = u - k.cu;
    const float b = v - k.cv;
    const float c = a * k.fv - k.skew * b;
    const float _fv = 1.0f / k.fv;
    const float _fuv = 1.0f / (k.fu * k.fv);
    J[0] = gu * _z * k.fu;
    J[1] = _z * (gu * k.skew + gv * k.fv);
    J[2] = -_z * (gu * a + gv * b);
    J[3] = gu * (-a * b * _fv - k.skew) + gv * (-b * b * _fv - k.fv);
    J[4] = gu * (a * c * _fuv + k.fu) + gv * (b * c * _fuv);
    J[5] = gu * (-k.fu * k.fu * b + k.skew * c) * _fuv + gv * (c / k.fu);
}

// Division by a value that is uniform over a level (the focal lengths): x / d == fma(fma(-q, d, x), r, q) with r = RN(1/d),
// q = RN(x r), whenever `ok` — and `ok` is only set after the identity has been checked EXHAUSTIVELY for this d over all 2^23
// significands of x on the device (kernels.hip, verify_fastdiv_kernel): both sides scale exactly with the exponent of x and
// are odd in x, so one binade proves every finite x whose quotient stays in the normal range. Otherwise: IEEE division.
struct FastDiv {
    float d, r;
    int ok;
};
template <bool FAST>
VORS_HD float div_uniform(float x, const FastDiv& f) {
    if (FAST) {
        const float q = x * f.r;
        const float e = fmaf(-q, f.d, x);
        const float q1 = fmaf(e, f.r, q);
        // q already carries the sign of the true quotient (also for x = -0, where the correction term would give +0): one v_bfi
        return __builtin_copysignf(q1, q);
    }
    return x / f.d;
}
// The same with the choice made at run time (`ok` is uniform over a level: one scalar branch), for code that has no template to spare.
VORS_HD float div_uniform_rt(float x, const FastDiv& f) {
    return f.ok ? div_uniform<true>(x, f) : x / f.d;
}
struct IntrFast {
    Intr k;
    FastDiv fu, fv;
};
// back_project / warp_jacobian_at with the three divisions by the focal lengths through div_uniform_rt (bit-identical by construction).
VORS_HD V3 back_project_rt(const IntrFast& kf, float px, float py, float depth) {
    const float z = depth;
    const float y = div_uniform_rt((py - kf.k.cv) * z, kf.fv);
    const float x = div_uniform_rt((px - kf.k.cu) * z - kf.k.skew * y, kf.fu);
    return V3{x, y, z};
}
// back_project with the two divisions by fv / fu through div_uniform (bit-identical to back_project by construction).
template <bool FAST>
VORS_HD V3 back_project_fast(const IntrFast& kf, float px, float py, float depth) {
    const float z = depth;
    const float y = div_uniform<FAST>((py - kf.k.cv) * z, kf.fv);
    const float x = div_uniform<FAST>((px - kf.k.cu) * z - kf.k.skew * y, kf.fu);
    return V3{x, y, z};
}
template <bool FAST>
VORS_HD void warp_jacobian_at_fast(float gu, float gv, float u, float v, float _z, const IntrFast& kf, float J[6]) {
    const Intr& k = kf.k;
    const float a = u - k.cu;
    const float b = v - k.cv;
    const float c = a * k.fv - k.skew * b;
    const float _fv = 1.0f / k.fv;
    const float _fuv = 1.0f / (k.fu * k.fv);
    J[0] = gu * _z * k.fu;
    J[1] = _z * (gu * k.skew + gv * k.fv);
    J[2] = -_z * (gu * a + gv * b);
    J[3] = gu * (-a * b * _fv - k.skew) + gv * (-b * b * _fv - k.fv);
    J[4] = gu * (a * c * _fuv + k.fu) + gv * (b * c * _fuv);
    J[5] = gu * (-k.fu * k.fu * b + k.skew * c) * _fuv + gv * div_uniform<FAST>(c, kf.fu);
}
VORS_HD void warp_jacobian_at_rt(float gu, float gv, float u, float v, float _z, const IntrFast& kf, float J[6]) {
    const Intr& k = kf.k;
    const float a = u - k.cu;
    const float b = v - k.cv;
    const float c = a * k.fv - k.skew * b;
    const float _fv = 1.0f / k.fv;
    const float _fuv = 1.0f / (k.fu * k.fv);
    J[0] = gu * _z * k.fu;
    J[1] = _z * (gu * k.skew + gv * k.fv);
    J[2] = -_z * (gu * a + gv * b);
    J[3] = gu * (-a * b * _fv - k.skew) + gv * (-b * b * _fv - k.fv);
    J[4] = gu * (a * c * _fuv + k.fu) + gv * (b * c * _fuv);
    J[5] = gu * (-k.fu * k.fu * b + k.skew * c) * _fuv + gv * div_uniform_rt(c, kf.fu);
}

// so3 / se3 log: API parity only (src/math/so3.rs:81-99, src/math/se3.rs:99-129); host use.
inline void so3_log(const Quat& r, float w[3]) {
    const V3 imag{r.i, r.j, r.k};
    const float imag_norm_2 = dot3(imag, imag);
    const float real_factor = r.w;
    float s;
    if (imag_norm_2 < 1e-2f * 1e-2f) {
        s = 2.0f / real_factor;
    } else if (fabsf(real_factor) < 1e-2f) {
        const float imag_norm = sqrtf(imag_norm_2);
        const float alpha = fabsf(real_factor) / imag_norm;
        const float sign = signbit(real_factor) ? -1.0f : 1.0f;
        s = (sign * (3.14159265358979323846f - 2.0f * alpha)) / imag_norm;
    } else {
        const float imag_norm = sqrtf(imag_norm_2);
        s = (2.0f * atanf(imag_norm / real_factor)) / imag_norm;
    }
    w[0] = s * imag.x; w[1] = s * imag.y; w[2] = s * imag.z;
}
inline Quat so3_exp(const float w[3]) {  // so3.rs:62-77
    const float theta_2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    float real_factor, imag_factor;
    if (theta_2 < 1e-2f * 1e-2f) {
        real_factor = 1.0f - 0.125f * theta_2;
        imag_factor = 0.5f - (1.0f / 48.0f) * theta_2;
    } else {
        const float theta = sqrtf(theta_2);
        const float half_theta = 0.5f * theta;
        real_factor = cosf(half_theta);
        imag_factor = sinf(half_theta) / theta;
    }
    return unit_from_quaternion(Quat{imag_factor * w[0], imag_factor * w[1], imag_factor * w[2], real_factor});
}
inline void se3_log(const Iso& iso, float xi[6]) {
    const V3 imag{iso.q.i, iso.q.j, iso.q.k};
    const float imag_norm_2 = dot3(imag, imag);
    const float real_factor = iso.q.w;
    float w[3], c2;
    if (imag_norm_2 < 1e-2f * 1e-2f) {
        const float s = 2.0f / real_factor;
        w[0] = s * imag.x; w[1] = s * imag.y; w[2] = s * imag.z;
        const float x_2 = imag_norm_2 / (real_factor * real_factor);
        c2 = (1.0f / 12.0f) * (1.0f + (1.0f / 15.0f) * x_2);
    } else {
        const float imag_norm = sqrtf(imag_norm_2);
        float theta;
        if (fabsf(real_factor) < 1e-2f) {
            const float alpha = fabsf(real_factor) / imag_norm;
            const float sign = signbit(real_factor) ? -1.0f : 1.0f;
            theta = sign * (3.14159265358979323846f - 2.0f * alpha);
        } else {
            theta = 2.0f * atanf(imag_norm / real_factor);
        }
        const float theta_2 = theta * theta;
        const float s = theta / imag_norm;
        w[0] = s * imag.x; w[1] = s * imag.y; w[2] = s * imag.z;
        c2 = (1.0f - 0.5f * theta * real_factor / imag_norm) / theta_2;
    }
    const float wx = w[0], wy = w[1], wz = w[2];
    const float w11 = wx * wx, w12 = wx * wy, w13 = wx * wz, w22 = wy * wy, w23 = wy * wz, w33 = wz * wz;
    const float O[3][3] = {{0.0f, -wz, wy}, {wz, 0.0f, -wx}, {-wy, wx, 0.0f}};
    const float O2[3][3] = {{-w22 - w33, w12, w13}, {w12, -w11 - w33, w23}, {w13, w23, -w11 - w22}};
    float V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) V[r][c] = ((r == c ? 1.0f : 0.0f) + (-0.5f) * O[r][c]) + c2 * O2[r][c];
    const float tx = iso.t.x, ty = iso.t.y, tz = iso.t.z;
    xi[0] = (V[0][0] * tx + V[0][1] * ty) + V[0][2] * tz;
    xi[1] = (V[1][0] * tx + V[1][1] * ty) + V[1][2] * tz;
    xi[2] = (V[2][0] * tx + V[2][1] * ty) + V[2][2] * tz;
    xi[3] = w[0]; xi[4] = w[1]; xi[5] = w[2];
}

// Pose-graph optimisation (vors_pose_graph_optimize, include/vors_hip.h 2g; the reference has none): the texts the kernels
// (pose_graph_kernels.hip) and the host twin (operators.cpp vors_pose_graph_optimize_host) both run, bit for bit. No libm transcendental
// below: the residual needs no logarithm, and the update is se3_exp's (ref_sinf / ref_cosf).
// An edge (i, j, M, Omega, w), poses camera -> world, M maps coordinates of camera i into camera j: E = T_i^-1 T_j M (the identity when
// consistent), s = E.q.w >= 0 ? 1 : -1, r = (E.t, 2 s E.q.ijk), energy = w * (r . (Omega r)).
// Jacobians for T_k <- T_k exp(d_k): T_j exp(d) M = E exp(Ad(M^-1) d) and exp(-d) E = E exp(-Ad(E^-1) d), and E exp(e) has the residual
// r + A(E) e to first order, A(E) = blockdiag(R_E, s (E.q.w I + [E.q.ijk]x)) — so J_j = A Ad(M^-1), J_i = -A Ad(E^-1), with
// Ad(R, t) = [[R, [t]x R], [0, R]] in se3_exp's (v, w) order (checked against central differences: tests/test_pose_graph_host.py).
#define VORS_PG_CHUNK 1024
#define VORS_PG_LIN 56  // floats of an edge's record beside W: H_ii (21, lower triangle row-wise), H_jj (21), g_i (6), g_j (6), 2 of padding
enum PgStatus { PG_ITERATIONS = 0, PG_CONVERGED = 1, PG_TOO_FEW = 2, PG_SINGULAR = 3 };
VORS_HD bool pg_finite(float x) { return x - x == 0.0f; }
// SKIPPED unless: i != j, both below node_count, w finite and > 0, every entry of the measurement and of the information finite
VORS_HD bool pg_edge_valid(uint32_t i, uint32_t j, uint32_t node_count, float w, const float* meas7, const float* info36 /* nullable */) {
    bool ok = i != j && i < node_count && j < node_count && pg_finite(w) && w > 0.0f;
    for (int k = 0; k < 7; ++k) ok = ok && pg_finite(meas7[k]);
    if (info36)
        for (int k = 0; k < 36; ++k) ok = ok && pg_finite(info36[k]);
    return ok;
}
// The information of an edge as the arithmetic reads it: the given matrix, or — none given — the identity, through the SAME arithmetic,
// so that NULL equals identity matrices bit for bit.
VORS_HD void pg_load_info(const float* info36 /* nullable */, float om[36]) {
VORS_UNROLL
    for (int k = 0; k < 36; ++k) om[k] = info36 ? info36[k] : (k % 7 == 0 ? 1.0f : 0.0f);
}
// the residual of an error E: r = (E.t, 2 s E.q.ijk) -> s (also what vors_loop_verify_edges measures a cycle and a prior with)
VORS_HD float pg_error_residual(const Iso& e, float r[6]) {
    const float s = e.q.w >= 0.0f ? 1.0f : -1.0f;
    r[0] = e.t.x; r[1] = e.t.y; r[2] = e.t.z;
    r[3] = (2.0f * s) * e.q.i; r[4] = (2.0f * s) * e.q.j; r[5] = (2.0f * s) * e.q.k;
    return s;
}
VORS_HD float pg_edge_error(const Iso& ti, const Iso& tj, const Iso& m, Iso* e, float r[6]) {
    *e = iso_mul(iso_mul(iso_inverse(ti), tj), m);
    return pg_error_residual(*e, r);
}
// w * (r . (Omega r)): rows of Omega r left to right, then the six products r[a] (Omega r)[a] in ascending a
VORS_HD float pg_edge_energy(const float r[6], const float om[36], float w) {
    float e = 0.0f;
VORS_UNROLL
    for (int a = 0; a < 6; ++a) {
        float t = om[a * 6] * r[0];
VORS_UNROLL
        for (int b = 1; b < 6; ++b) t = t + om[a * 6 + b] * r[b];
        e = a == 0 ? r[0] * t : e + r[a] * t;
    }
    return w * e;
}
VORS_HD void pg_rot(const Quat& q, float m[9]) {
    const float ii = q.i * q.i, jj = q.j * q.j, kk = q.k * q.k, ij = q.i * q.j, ik = q.i * q.k, jk = q.j * q.k;
    const float iw = q.i * q.w, jw = q.j * q.w, kw = q.k * q.w;
    m[0] = 1.0f - 2.0f * (jj + kk); m[1] = 2.0f * (ij - kw); m[2] = 2.0f * (ik + jw);
    m[3] = 2.0f * (ij + kw); m[4] = 1.0f - 2.0f * (ii + kk); m[5] = 2.0f * (jk - iw);
    m[6] = 2.0f * (ik - jw); m[7] = 2.0f * (jk + iw); m[8] = 1.0f - 2.0f * (ii + jj);
}
VORS_HD void pg_mul3(const float a[9], const float b[9], float c[9]) {
VORS_UNROLL
    for (int r = 0; r < 3; ++r)
VORS_UNROLL
        for (int q = 0; q < 3; ++q) c[r * 3 + q] = (a[r * 3] * b[q] + a[r * 3 + 1] * b[3 + q]) + a[r * 3 + 2] * b[6 + q];
}
// A(E) Ad(T) for T = (rotation matrix rt, translation t), scaled by sign: the 6x6 Jacobian, row-major, its lower-left block exact zeros
VORS_HD void pg_jacobian(const float re[9], const float qe[9], const float rt[9], const V3& t, float sign, float j[36]) {
    const float hat[9] = {0.0f, -t.z, t.y, t.z, 0.0f, -t.x, -t.y, t.x, 0.0f};
    float hr[9], a[9], b[9], c[9];
    pg_mul3(hat, rt, hr);
    pg_mul3(re, rt, a);
    pg_mul3(re, hr, b);
    pg_mul3(qe, rt, c);
VORS_UNROLL
    for (int r = 0; r < 3; ++r)
VORS_UNROLL
        for (int q = 0; q < 3; ++q) {
            j[r * 6 + q] = sign * a[r * 3 + q];
            j[r * 6 + 3 + q] = sign * b[r * 3 + q];
            j[(r + 3) * 6 + q] = 0.0f;
            j[(r + 3) * 6 + 3 + q] = sign * c[r * 3 + q];
        }
}
// The residual and both Jacobians of an edge at the poses (ti, tj)
VORS_HD void pg_edge_jacobians(const Iso& ti, const Iso& tj, const Iso& m, float r[6], float ji[36], float jj[36]) {
    Iso e;
    const float s = pg_edge_error(ti, tj, m, &e, r);
    float re[9], rm[9], rei[9];
    pg_rot(e.q, re);
    const float qe[9] = {s * e.q.w, s * -e.q.k, s * e.q.j, s * e.q.k, s * e.q.w, s * -e.q.i, s * -e.q.j, s * e.q.i, s * e.q.w};
    const Iso mi = iso_inverse(m), ei = iso_inverse(e);
    pg_rot(mi.q, rm);
    pg_rot(ei.q, rei);
    pg_jacobian(re, qe, rm, mi.t, 1.0f, jj);
    pg_jacobian(re, qe, rei, ei.t, -1.0f, ji);
}
// c = a b, 6x6 row-major, each entry summed left to right; at = true: c = a^T b
VORS_HD void pg_mul6(const float a[36], bool at, const float b[36], float c[36]) {
VORS_UNROLL
    for (int r = 0; r < 6; ++r)
VORS_UNROLL
        for (int q = 0; q < 6; ++q) {
            float t = (at ? a[r] : a[r * 6]) * b[q];
VORS_UNROLL
            for (int k = 1; k < 6; ++k) t = t + (at ? a[k * 6 + r] : a[r * 6 + k]) * b[k * 6 + q];
            c[r * 6 + q] = t;
        }
}
// The linearisation of a valid edge: W = J_i^T (w Omega) J_j (36, row-major), and lin = the lower triangles of J_i^T (w Omega) J_i and
// J_j^T (w Omega) J_j, g_i = J_i^T (w Omega) r, g_j = J_j^T (w Omega) r. w Omega is formed first, entry by entry.
VORS_HD void pg_edge_linearise(const Iso& ti, const Iso& tj, const Iso& m, const float om[36], float w, float wmat[36], float lin[VORS_PG_LIN]) {
    float r[6], ji[36], jj[36], ow[36], bi[36], bj[36], v[6];
    pg_edge_jacobians(ti, tj, m, r, ji, jj);
VORS_UNROLL
    for (int k = 0; k < 36; ++k) ow[k] = w * om[k];
    pg_mul6(ow, false, ji, bi);
    pg_mul6(ow, false, jj, bj);
    pg_mul6(ji, true, bj, wmat);
VORS_UNROLL
    for (int a = 0; a < 6; ++a) {
        float t = ow[a * 6] * r[0];
VORS_UNROLL
        for (int b = 1; b < 6; ++b) t = t + ow[a * 6 + b] * r[b];
        v[a] = t;
    }
    int k = 0;
VORS_UNROLL
    for (int a = 0; a < 6; ++a)
VORS_UNROLL
        for (int b = 0; b <= a; ++b, ++k) {
            float hi = ji[a] * bi[b], hj = jj[a] * bj[b];
VORS_UNROLL
            for (int c = 1; c < 6; ++c) {
                hi = hi + ji[c * 6 + a] * bi[c * 6 + b];
                hj = hj + jj[c * 6 + a] * bj[c * 6 + b];
            }
            lin[k] = hi;
            lin[21 + k] = hj;
        }
VORS_UNROLL
    for (int a = 0; a < 6; ++a) {
        float gi = ji[a] * v[0], gj = jj[a] * v[0];
VORS_UNROLL
        for (int c = 1; c < 6; ++c) {
            gi = gi + ji[c * 6 + a] * v[c];
            gj = gj + jj[c * 6 + a] * v[c];
        }
        lin[42 + a] = gi;
        lin[48 + a] = gj;
    }
    lin[54] = lin[55] = 0.0f;
}
// A node's damped block and its factor from the sums over its edges: hd = H_kk with the diagonal times (1 + lambda) — cholesky6_solve's
// damping, D = diag(H) — and fac = its Cholesky factor (lower, cholesky6_solve's left-looking order). No early exit: a pivot that is not
// > 0 is remembered and the loops run on. -> whether a factor exists. Lower triangles row-wise: (r, c) at r (r + 1) / 2 + c.
VORS_HD bool pg_node_factor(const float h21[21], float lambda, float hd[21], float fac[21]) {
    float a[6][6];
    const float scale = 1.0f + lambda;
    int k = 0;
VORS_UNROLL
    for (int r = 0; r < 6; ++r)
VORS_UNROLL
        for (int c = 0; c <= r; ++c, ++k) {
            hd[k] = r == c ? h21[k] * scale : h21[k];
            a[r][c] = hd[k];
        }
    bool ok = true;
VORS_UNROLL
    for (int j = 0; j < 6; ++j) {
VORS_UNROLL
        for (int q = 0; q < j; ++q) {
            const float factor = -a[j][q];
VORS_UNROLL
            for (int i = j; i < 6; ++i) a[i][j] = factor * a[i][q] + a[i][j];
        }
        ok = ok && a[j][j] > 0.0f;
        const float denom = sqrtf(a[j][j]);
        a[j][j] = denom;
VORS_UNROLL
        for (int i = j + 1; i < 6; ++i) a[i][j] /= denom;
    }
    k = 0;
VORS_UNROLL
    for (int r = 0; r < 6; ++r)
VORS_UNROLL
        for (int c = 0; c <= r; ++c, ++k) fac[k] = a[r][c];
    return ok;
}
// x = (L L^T)^-1 b: forward, then backward substitution, cholesky6_solve's order
VORS_HD void pg_factor_solve(const float fac[21], const float b6[6], float x[6]) {
    float b[6];
VORS_UNROLL
    for (int i = 0; i < 6; ++i) b[i] = b6[i];
VORS_UNROLL
    for (int i = 0; i < 6; ++i) {
        const float coeff = b[i] / fac[i * (i + 1) / 2 + i];
        b[i] = coeff;
VORS_UNROLL
        for (int k = i + 1; k < 6; ++k) b[k] = (-coeff) * fac[k * (k + 1) / 2 + i] + b[k];
    }
VORS_UNROLL
    for (int i = 5; i >= 0; --i) {
        float dot = 0.0f;
VORS_UNROLL
        for (int k = i + 1; k < 6; ++k) dot += fac[k * (k + 1) / 2 + i] * b[k];
        b[i] = (b[i] - dot) / fac[i * (i + 1) / 2 + i];
    }
VORS_UNROLL
    for (int i = 0; i < 6; ++i) x[i] = b[i];
}
// The product (H + lambda D) p at one node: y = hd p first (the lower triangle mirrored, each row left to right), then per incident
// valid edge in ascending edge index y = y + W p_other (the node is the edge's i) or y + W^T p_other (it is the edge's j).
VORS_HD void pg_matvec_own(const float hd[21], const float p[6], float y[6]) {
VORS_UNROLL
    for (int r = 0; r < 6; ++r) {
        float t = hd[r * (r + 1) / 2] * p[0];
VORS_UNROLL
        for (int c = 1; c < 6; ++c) t = t + (c <= r ? hd[r * (r + 1) / 2 + c] : hd[c * (c + 1) / 2 + r]) * p[c];
        y[r] = t;
    }
}
VORS_HD void pg_matvec_edge(const float wmat[36], bool transposed, const float po[6], float y[6]) {
VORS_UNROLL
    for (int r = 0; r < 6; ++r) {
        float t = (transposed ? wmat[r] : wmat[r * 6]) * po[0];
VORS_UNROLL
        for (int c = 1; c < 6; ++c) t = t + (transposed ? wmat[c * 6 + r] : wmat[r * 6 + c]) * po[c];
        y[r] = y[r] + t;
    }
}
// THE SCALARS OF THE CONJUGATE GRADIENTS ARE f64: a node's share of a dot product is the f64 sum, left to right, of the exact f64
// products of its six f32 pairs; the shares go through the chunk tree in f64. alpha and beta are rounded to f32 ONCE, and the vectors
// are updated in f32.
VORS_HD double pg_dot6(const float a[6], const float b[6]) {
    double s = (double)a[0] * (double)b[0];
VORS_UNROLL
    for (int k = 1; k < 6; ++k) s = s + (double)a[k] * (double)b[k];
    return s;
}
VORS_HD float pg_cg_alpha(double rz, double pq) { return pq > 0.0 ? (float)(rz / pq) : 0.0f; }
VORS_HD float pg_cg_beta(double rz, double rz_prev) { return rz_prev > 0.0 ? (float)(rz / rz_prev) : 0.0f; }
// the iterations end when |r| <= cg_tol |r_0| (a NaN ends them as well)
VORS_HD bool pg_cg_reached(double rr, double rr0, float cg_tol) { return !(rr > ((double)cg_tol * (double)cg_tol) * rr0); }
// p_t = z_t + beta_t p_(t-1), the direction a node and its neighbours both form from the stored z and p_(t-1)
VORS_HD void pg_cg_direction(const float z[6], float beta, const float p_prev[6], float p[6]) {
VORS_UNROLL
    for (int k = 0; k < 6; ++k) p[k] = z[k] + beta * p_prev[k];
}
VORS_HD float pg_step2(const float d[6]) {
    float s = d[0] * d[0];
VORS_UNROLL
    for (int k = 1; k < 6; ++k) s = s + d[k] * d[k];
    return s;
}
VORS_HD Iso pg_candidate(const Iso& t, const float delta[6]) { return renormalize(iso_mul(t, se3_exp(delta))); }
// The round's verdict. lm_verdict's constants (accepted: lambda = 0.1f * lambda, rejected: lambda *= 10.0f), not its rule: a NaN energy
// is REJECTED here, and nothing stops on a small decrease of the energy — the step norm does that.
VORS_HD bool pg_accepts(float energy, float cur_energy) { return energy <= cur_energy; }
VORS_HD float pg_lambda_after(bool accepted, float lambda) { return accepted ? 0.1f * lambda : lambda * 10.0f; }
// The halving tree of a chunk on the host: v[s] = v[s] + v[s + w] for w = 512 .. 1; the chunk's sum is v[0].
template <class T>
inline T pg_chunk_tree(T* v) {
    for (int w = VORS_PG_CHUNK / 2; w >= 1; w /= 2)
        for (int s = 0; s < w; ++s) v[s] = v[s] + v[s + w];
    return v[0];
}

// Loop closure (vors_loop_signatures, vors_loop_candidates, vors_loop_verify_edges; include/vors_hip.h 2h; the reference has
// none): the texts the kernels (loop_closure_kernels.hip) and the host twins (operators.cpp) both run, bit for bit. Signatures and dot
// products are exact integers; the score is ONE f64 divide of an exact numerator by the product of two correctly rounded f64 roots.
#define VORS_LC_MAX_K 8
#define VORS_LC_COUNTS 5    // examined, flat, pose-gated, score-gated, survivors
#define VORS_LC_VERDICTS 9  // LcVerdict
#define VORS_LC_EMPTY 0xFFFFFFFFu
enum LcVerdict { LC_ACCEPTED = 0, LC_STATUS = 1, LC_INDEX = 2, LC_NONFINITE = 3, LC_CYCLE_TRANS = 4, LC_CYCLE_ROT = 5, LC_PRIOR_TRANS = 6,
                 LC_PRIOR_ROT = 7, LC_CAPACITY = 8 };
// the thumbnail cell that pixel coordinate x of `extent` falls into: cell c covers [c extent / cells, (c + 1) extent / cells)
// (extent <= 65535 and cells <= 1024, which the entries see to: the products fit 32 bits)
VORS_HD uint32_t lc_cell_of(uint32_t x, uint32_t extent, uint32_t cells) { return ((x + 1u) * cells - 1u) / extent; }
VORS_HD uint32_t lc_cell_begin(uint32_t c, uint32_t extent, uint32_t cells) { return (c * extent) / cells; }
// the stored value of a cell: the rounded mean of its pixels minus 128
VORS_HD int8_t lc_cell_value(uint64_t sum, uint64_t cnt) { return (int8_t)((int)((2u * sum + cnt) / (2u * cnt)) - 128); }
// D sumsq - sum^2 of a signature (>= 0; 0 = flat), and its root
VORS_HD int64_t lc_variance(int d, int32_t sum, uint32_t sumsq) { return (int64_t)d * (int64_t)sumsq - (int64_t)sum * (int64_t)sum; }
VORS_HD double lc_root(int64_t va) { return sqrt((double)va); }
VORS_HD int64_t lc_numerator(int d, int32_t dot, int32_t sum_i, int32_t sum_j) { return (int64_t)d * (int64_t)dot - (int64_t)sum_i * (int64_t)sum_j; }
VORS_HD float lc_score(int64_t num, double root_i, double root_j) { return (float)((double)num / (root_i * root_j)); }
VORS_HD bool lc_score_passes(float score, float min_score) { return score >= min_score; }  // a NaN fails
// The pose gate of a pair of camera -> world poses, f32 in this order; a half whose parameter is 0 is off; in a half that is on, a
// value that is not finite fails.
VORS_HD bool lc_pose_passes(const float* pi7, const float* pj7, float max_dist_m, float min_qdot) {
    bool ok = true;
    if (max_dist_m > 0.0f) {
        const V3 d{pi7[0] - pj7[0], pi7[1] - pj7[1], pi7[2] - pj7[2]};
        ok = dot3(d, d) <= max_dist_m * max_dist_m;
    }
    if (min_qdot > 0.0f) {
        const float qd = fabsf(dot3(V3{pi7[3], pi7[4], pi7[5]}, V3{pj7[3], pj7[4], pj7[5]}) + pi7[6] * pj7[6]);
        ok = ok && pg_finite(qd) && qd >= min_qdot;
    }
    return ok;
}
// THE ORDER of candidates: score descending, then index ascending — total, since an index occurs once
VORS_HD bool lc_before(float score_a, uint32_t a, float score_b, uint32_t b) { return score_a > score_b || (score_a == score_b && a < b); }
// Insertion into a list of at most k <= VORS_LC_MAX_K entries kept in that order; slots [*n, k) are unused. The loop has a fixed trip
// count and constant indices, so a kernel keeps the list in registers.
VORS_HD void lc_topk_insert(uint32_t idx[VORS_LC_MAX_K], float score[VORS_LC_MAX_K], uint32_t* n, uint32_t k, uint32_t i, float s) {
    bool have = true;
VORS_UNROLL
    for (uint32_t p = 0; p < VORS_LC_MAX_K; ++p) {
        if (p < k && have) {
            if (p >= *n) {
                idx[p] = i;
                score[p] = s;
                have = false;
            } else if (lc_before(s, i, score[p], idx[p])) {
                const uint32_t ti = idx[p];
                const float ts = score[p];
                idx[p] = i;
                score[p] = s;
                i = ti;
                s = ts;
            }
        }
    }
    if (*n < k) *n += 1u;
}
// The verdict of one tracked loop candidate before the edge list's capacity is looked at, and its residuals r12 = the cycle's r6, then
// the prior's r6 (NaN where not computed). The first rule that applies wins; both residuals are computed for every candidate that
// passes STATUS, INDEX and NONFINITE. A bound of 0 switches its test off; the comparisons are written so that a NaN residual FAILS.
// fwd / bwd: M_ij and M_ji (bwd nullable); poses: camera -> world, pose_stride floats apart (nullable).
VORS_HD uint32_t lc_verify(uint32_t i, uint32_t j, bool status_ok, const float* fwd7, const float* bwd7, const float* info36, const float* poses,
                           int pose_stride, uint32_t node_count, float max_cycle_trans, float max_cycle_rot, float max_prior_trans,
                           float max_prior_rot, float r12[12]) {
    const float nan = nanf("");
VORS_UNROLL
    for (int k = 0; k < 12; ++k) r12[k] = nan;
    if (!status_ok) return LC_STATUS;
    if (i == j || (poses && (i >= node_count || j >= node_count))) return LC_INDEX;
    bool finite = true;
    for (int k = 0; k < 7; ++k) finite = finite && pg_finite(fwd7[k]) && (!bwd7 || pg_finite(bwd7[k]));
    if (info36)
        for (int k = 0; k < 36; ++k) finite = finite && pg_finite(info36[k]);
    if (!finite) return LC_NONFINITE;
    const Iso m = iso_load(fwd7);
    uint32_t verdict = LC_ACCEPTED;
    if (bwd7) {
        pg_error_residual(iso_mul(iso_load(bwd7), m), r12);
        const float t2 = dot3(V3{r12[0], r12[1], r12[2]}, V3{r12[0], r12[1], r12[2]});
        const float w2 = dot3(V3{r12[3], r12[4], r12[5]}, V3{r12[3], r12[4], r12[5]});
        if (max_cycle_trans > 0.0f && !(t2 <= max_cycle_trans * max_cycle_trans)) verdict = LC_CYCLE_TRANS;
        else if (max_cycle_rot > 0.0f && !(w2 <= max_cycle_rot * max_cycle_rot)) verdict = LC_CYCLE_ROT;
    }
    if (poses) {
        Iso e;
        pg_edge_error(iso_load(poses + (size_t)i * pose_stride), iso_load(poses + (size_t)j * pose_stride), m, &e, r12 + 6);
        const float t2 = dot3(V3{r12[6], r12[7], r12[8]}, V3{r12[6], r12[7], r12[8]});
        const float w2 = dot3(V3{r12[9], r12[10], r12[11]}, V3{r12[9], r12[10], r12[11]});
        if (verdict == LC_ACCEPTED) {
            if (max_prior_trans > 0.0f && !(t2 <= max_prior_trans * max_prior_trans)) verdict = LC_PRIOR_TRANS;
            else if (max_prior_rot > 0.0f && !(w2 <= max_prior_rot * max_prior_rot)) verdict = LC_PRIOR_ROT;
        }
    }
    return verdict;
}

// Re-posing of point lists after pose-graph optimisation (vors_repose_points, include/vors_hip.h 2i): the texts the
// kernels of repose_kernels.hip and the host twin (vors_repose_points_host) both run, bit for bit.
#define VORS_REPOSE_NO_NODE 0xFFFFFFFFu
enum { REPOSE_MOVED = 0, REPOSE_KEPT = 1, REPOSE_NONFINITE = 2, REPOSE_NO_RECORD = 3, REPOSE_SEGMENTS_MOVED = 4, REPOSE_MAX_SHIFT = 5 };
VORS_HD uint32_t repose_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
// The node of recorded segment k: k itself without a table, the table's word with one; VORS_REPOSE_NO_NODE when the word is the
// sentinel or the index is not below the graph's node count (itself clipped to node_capacity: no pose beyond it is ever read).
VORS_HD uint32_t repose_node(uint32_t k, const uint32_t* node_of_segment /* nullable */, uint32_t node_count, int node_capacity) {
    const uint32_t nodes = node_count < (uint32_t)node_capacity ? node_count : (uint32_t)node_capacity;
    const uint32_t node = node_of_segment ? node_of_segment[k] : k;
    return node != VORS_REPOSE_NO_NODE && node < nodes ? node : VORS_REPOSE_NO_NODE;
}
// A segment with old pose a7 MOVES to b7 (NULL: it has no node) iff all seven floats of b7 are finite and their bits differ from a7's.
VORS_HD bool repose_moves(const float* a7, const float* b7 /* nullable */) {
    if (!b7) return false;
    bool finite = true, differs = false;
VORS_UNROLL
    for (int k = 0; k < 7; ++k) {
        finite = finite && f32_finite(b7[k]);
        differs = differs || repose_bits(a7[k]) != repose_bits(b7[k]);
    }
    return finite && differs;
}
VORS_HD bool repose_finite3(const V3& p) { return f32_finite(p.x) && f32_finite(p.y) && f32_finite(p.z); }
// A NaN that arithmetic produced (a finite input that overflowed on the way) is stored as ONE bit pattern: what the hardware would
// put into its payload and sign is not the same on every machine.
VORS_HD float repose_canonical(float v) { return v != v ? __builtin_bit_cast(float, VORS_VOXEL_MEAN_NAN_BITS) : v; }
VORS_HD V3 repose_canonical3(const V3& p) { return V3{repose_canonical(p.x), repose_canonical(p.y), repose_canonical(p.z)}; }
// A point of a moved segment: through the keyframe's camera frame at the old pose, out again at the new one — existing texts, unchanged.
VORS_HD V3 repose_point(const Iso& a, const Iso& b, const V3& p) { return repose_canonical3(iso_transform_point(b, extr_project(a, p))); }
// Its normal: the two rotations alone.
VORS_HD V3 repose_normal(const Iso& a, const Iso& b, const V3& n) {
    const Quat qi{-a.q.i, -a.q.j, -a.q.k, a.q.w};
    return repose_canonical3(quat_rotate(b.q, quat_rotate(qi, n)));
}
// |p' - p| as the bits of a non-negative f32 (a NaN: the one pattern above, which an unsigned maximum ranks above every length).
VORS_HD uint32_t repose_shift_bits(const V3& p, const V3& q) {
    const V3 d{q.x - p.x, q.y - p.y, q.z - p.z};
    return repose_bits(repose_canonical(sqrtf(dot3(d, d))));
}
// The ranks of recorded segment k of a list of `total` ranks, [*lo, *hi) (empty: *lo >= *hi): from its `first` to its own end, to the
// next record's `first` and to the list's end, whichever comes first — so that with ascending `first`, which a map's records have, a
// rank belongs to the LAST record whose `first` is not above it, and a zero-count segment owns no rank. words: the list's records as
// 32-bit words (MAP_SEGMENT_WORDS per record, first at word 1, count at word 2).
VORS_HD void repose_segment_ranks(const uint32_t* words, uint32_t k, uint32_t n_rec, uint32_t total, uint32_t* lo, uint32_t* hi) {
    const uint32_t first = words[(size_t)k * MAP_SEGMENT_WORDS + 1], count = words[(size_t)k * MAP_SEGMENT_WORDS + 2];
    const uint64_t end64 = (uint64_t)first + (uint64_t)count;
    uint32_t end = end64 < (uint64_t)total ? (uint32_t)end64 : total;
    if (k + 1u < n_rec) {
        const uint32_t next = words[(size_t)(k + 1u) * MAP_SEGMENT_WORDS + 1];
        if (next < end) end = next;
    }
    *lo = first;
    *hi = end;
}
// The voxel filter of plain point lists (vors_voxel_filter_points): the number of kept source ranks below x, a lower-bound search in the
// ascending index list of a filtered list. A segment [first, first + count) of the source becomes [below(first), below(first + count)).
VORS_HD uint32_t voxel_filter_below(const uint32_t* index, uint32_t kept, uint64_t x) {
    uint32_t lo = 0, hi = kept;  // the first position in [0, kept] whose entry is >= x
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((uint64_t)index[mid] < x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

}  // namespace vors
