// vors_undistort_frames / vors_register_depth: the sensor front end. Handle-free: no Geom, no records; the per-pixel rules
// are lie.h undistort_source / undistort_taps / undistort_gray and register_point / render_point / render_footprint / register_resolve, the
// texts vors_undistort_frame_host and vors_register_depth_host run.
// UNDISTORT (undistort_kernel): fuse_depth_kernel's shape — elementwise over the OUTPUT plane, 1024 pixels per workgroup, grid = (chunks of
//         the plane) x planes. The source coordinate is computed per pixel (about 25 flops; a table would cost 8 bytes of traffic per pixel
//         and plane), once for the grey and the depth of the pixel. Where every output plane allows it (out_cols % 4 == 0, grey 4-byte
//         and depth 8-byte aligned) a thread takes four adjacent pixels of one row and stores them as one 4-byte and one 8-byte word;
//         else four pixels a workgroup width apart, the same bits. The source taps are plain gathers — four bytes of grey, one u16 of
//         depth — all issued before the first use; a tap outside the plane reads pixel 0 and is ignored. Distortion is smooth: the taps of a
//         wavefront stay within a few rows of the source. The coordinate table, when asked for, is written by the first plane's workgroups.
// SPLAT   (register_splat_kernel): elementwise over the SOURCE depth plane, four pixels a workgroup width apart per thread, all loads
//         first; per written colour pixel one 64-bit global atomicMin without return value of bits(Z') << 32 | s (render_splat_kernel's
//         scheme: a minimum, bitwise reproducible whatever the order of arrival; no workgroup waits for another).
// RESOLVE (register_resolve_kernel): elementwise over the colour plane: 8 bytes of key in, 2 bytes of depth and 4 of source index out.
//         (render_resolve_kernel gathers a grey level of a list at the key's rank and has no index output: it does not fit, and stays as it is.)
// COUNTS: per-thread integers, device_common.h block_counts into a zeroed array; compiled out without them. No LDS otherwise, no scratch.
#include <algorithm>

#include "device_common.h"

namespace vors {

struct UndistortArgs {
    int seq0;
    UndistortCall c;
    int wide;  // every output plane allows four adjacent pixels per thread
};
struct RegisterArgs {
    int seq0;
    RegisterCall c;
};

template <bool COUNTS>
__global__ __launch_bounds__(FRONT_BLOCK) void undistort_kernel(UndistortArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? (FRONT_BLOCK / 64) * VORS_UNDISTORT_COUNTS : 1];
    const UndistortCall& c = a.c;
    const int seq = a.seq0 + blockIdx.y;
    const int in_plane = c.in_rows * c.in_cols, out_plane = c.out_rows * c.out_cols;
    const uint8_t* gray = c.gray_out ? c.gray + (size_t)seq * (size_t)in_plane : nullptr;  // (read only for the grey output)
    const uint16_t* depth = c.depth ? c.depth + (size_t)seq * (size_t)in_plane : nullptr;
    uint8_t* gray_out = c.gray_out ? c.gray_out + (size_t)seq * (size_t)out_plane : nullptr;
    uint16_t* depth_out = c.depth_out ? c.depth_out + (size_t)seq * (size_t)out_plane : nullptr;
    float* map = seq == 0 ? c.map : nullptr;
    const int base = blockIdx.x * (FRONT_BLOCK * FRONT_POINTS);
    int idx[FRONT_POINTS], px[FRONT_POINTS], py[FRONT_POINTS];
    bool valid[FRONT_POINTS];
    if (a.wide) {  // (uniform; out_cols % 4 == 0: a thread's four pixels share a row and are all inside or all outside)
        const int i = base + FRONT_POINTS * (int)threadIdx.x;
        const int y = i / c.out_cols, x = i - y * c.out_cols;
#pragma unroll
        for (int j = 0; j < FRONT_POINTS; ++j) {
            idx[j] = i + j;
            px[j] = x + j;
            py[j] = y;
            valid[j] = i < out_plane;
        }
    } else {
#pragma unroll
        for (int j = 0; j < FRONT_POINTS; ++j) {
            idx[j] = base + j * FRONT_BLOCK + (int)threadIdx.x;
            py[j] = idx[j] / c.out_cols;
            px[j] = idx[j] - py[j] * c.out_cols;
            valid[j] = idx[j] < out_plane;
        }
    }
    UndistortTaps t[FRONT_POINTS];
    float u[FRONT_POINTS], v[FRONT_POINTS];
#pragma unroll
    for (int j = 0; j < FRONT_POINTS; ++j) {
        undistort_source(c.k_out, c.k_in, c.dist, px[j], py[j], &u[j], &v[j]);
        t[j] = undistort_taps(u[j], v[j], c.border, c.in_cols, c.in_rows);
        if (!valid[j]) t[j] = UndistortTaps{0, 0, 0, 0, 0.0f, 0.0f, false, false, -1};
    }
    uint8_t g00[FRONT_POINTS], g01[FRONT_POINTS], g10[FRONT_POINTS], g11[FRONT_POINTS];
    uint16_t d[FRONT_POINTS];
#pragma unroll
    for (int j = 0; j < FRONT_POINTS; ++j) {  // (every offset lies inside the plane: 0 where there is no tap)
        g00[j] = gray ? gray[t[j].i00] : 0;
        g01[j] = gray ? gray[t[j].i01] : 0;
        g10[j] = gray ? gray[t[j].i10] : 0;
        g11[j] = gray ? gray[t[j].i11] : 0;
        d[j] = depth ? depth[t[j].depth >= 0 ? t[j].depth : 0] : 0;
    }
    uint8_t og[FRONT_POINTS];
    uint16_t od[FRONT_POINTS];
    uint32_t cnt[VORS_UNDISTORT_COUNTS] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < FRONT_POINTS; ++j) {
        og[j] = undistort_gray(t[j], g00[j], g01[j], g10[j], g11[j]);
        od[j] = t[j].depth >= 0 ? d[j] : (uint16_t)0;
        cnt[0] += valid[j] ? 1u : 0u;
        cnt[1] += t[j].inside ? 1u : 0u;
        cnt[2] += od[j] != 0 ? 1u : 0u;
    }
    if (a.wide) {
        if (valid[0]) {
            if (gray_out)
                *reinterpret_cast<uint32_t*>(gray_out + idx[0]) =
                    (uint32_t)og[0] | ((uint32_t)og[1] << 8) | ((uint32_t)og[2] << 16) | ((uint32_t)og[3] << 24);
            if (depth_out) *reinterpret_cast<ushort4*>(depth_out + idx[0]) = make_ushort4(od[0], od[1], od[2], od[3]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < FRONT_POINTS; ++j) {
            if (!valid[j]) continue;
            if (gray_out) gray_out[idx[j]] = og[j];
            if (depth_out) depth_out[idx[j]] = od[j];
        }
    }
    if (map) {
#pragma unroll
        for (int j = 0; j < FRONT_POINTS; ++j) {
            if (!valid[j]) continue;
            map[2 * (size_t)idx[j]] = u[j];
            map[2 * (size_t)idx[j] + 1] = v[j];
        }
    }
    if constexpr (COUNTS) block_counts<VORS_UNDISTORT_COUNTS, FRONT_BLOCK>(cnt, lds_counts, CountsAdd{c.counts + (size_t)seq * VORS_UNDISTORT_COUNTS});
}

#define REGISTER_SPLAT_COUNTS 3  // with depth, in front, landed (covered is the resolve's)

template <int F, bool COUNTS>
__global__ __launch_bounds__(FRONT_BLOCK) void register_splat_kernel(RegisterArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? (FRONT_BLOCK / 64) * REGISTER_SPLAT_COUNTS : 1];
    const RegisterCall& c = a.c;
    const int seq = a.seq0 + blockIdx.y;
    const int d_plane = c.d_rows * c.d_cols;
    const uint16_t* depth = c.depth + (size_t)seq * (size_t)d_plane;
    unsigned long long* zkey = reinterpret_cast<unsigned long long*>(c.zkey) + (size_t)seq * (size_t)c.c_rows * (size_t)c.c_cols;
    const int base = blockIdx.x * (FRONT_BLOCK * FRONT_POINTS);
    uint16_t d[FRONT_POINTS];
#pragma unroll
    for (int j = 0; j < FRONT_POINTS; ++j) {
        const int s = base + j * FRONT_BLOCK + (int)threadIdx.x;
        d[j] = s < d_plane ? depth[s] : (uint16_t)0;  // (a pixel beyond the plane: no depth, nothing to do)
    }
    uint32_t cnt[REGISTER_SPLAT_COUNTS] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < FRONT_POINTS; ++j) {
        if (d[j] == 0) continue;
        const int s = base + j * FRONT_BLOCK + (int)threadIdx.x;
        const int y = s / c.d_cols, x = s - y * c.d_cols;
        const V3 p = register_point(c.k_d, c.scale_in, c.has_pose, c.pose, x, y, d[j]);
        const RenderPoint rp = render_point(c.k_c, false, c.pose, p, F, c.c_cols, c.c_rows);
        bool landed = false;
        if (rp.candidate) {
            const unsigned long long key = render_key(rp.z, (uint32_t)s);
            landed = render_footprint(rp, F, c.c_cols, c.c_rows, [&](int q) { atomicMin(zkey + q, key); });
        }
        if constexpr (COUNTS) {
            cnt[0] += 1u;
            cnt[1] += rp.in_front ? 1u : 0u;
            cnt[2] += landed ? 1u : 0u;
        }
    }
    if constexpr (COUNTS) block_counts<REGISTER_SPLAT_COUNTS, FRONT_BLOCK>(cnt, lds_counts, CountsAdd{c.counts + (size_t)seq * VORS_REGISTER_COUNTS});
}

template <bool COUNTS>
__global__ __launch_bounds__(FRONT_BLOCK) void register_resolve_kernel(RegisterArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? FRONT_BLOCK / 64 : 1];
    const RegisterCall& c = a.c;
    const int seq = a.seq0 + blockIdx.y;
    const int c_plane = c.c_rows * c.c_cols;
    const size_t off = (size_t)seq * (size_t)c_plane;
    const uint64_t* zkey = c.zkey + off;
    uint16_t* depth_out = c.depth_out ? c.depth_out + off : nullptr;
    uint32_t* src_index = c.src_index ? c.src_index + off : nullptr;
    const int base = blockIdx.x * (FRONT_BLOCK * FRONT_POINTS);
    uint64_t key[FRONT_POINTS];
#pragma unroll
    for (int j = 0; j < FRONT_POINTS; ++j) {
        const int i = base + j * FRONT_BLOCK + (int)threadIdx.x;
        key[j] = i < c_plane ? zkey[i] : 0xFFFFFFFFFFFFFFFFull;
    }
    uint32_t covered[1] = {0u};
#pragma unroll
    for (int j = 0; j < FRONT_POINTS; ++j) {
        const int i = base + j * FRONT_BLOCK + (int)threadIdx.x;
        if (i >= c_plane) continue;
        const RegisteredPixel o = register_resolve(c.scale_out, key[j]);
        if (depth_out) depth_out[i] = o.depth;
        if (src_index) src_index[i] = o.src;
        covered[0] += o.covered ? 1u : 0u;
    }
    if constexpr (COUNTS) block_counts<1, FRONT_BLOCK>(covered, lds_counts, CountsAdd{c.counts + (size_t)seq * VORS_REGISTER_COUNTS + 3});
}

static unsigned front_blocks(size_t plane) { return (unsigned)((plane + FRONT_BLOCK * FRONT_POINTS - 1) / (FRONT_BLOCK * FRONT_POINTS)); }

void launch_undistort(const UndistortCall& c, hipStream_t s) {
    const size_t out_plane = (size_t)c.out_rows * (size_t)c.out_cols;
    if (c.counts) (void)hipMemsetAsync(c.counts, 0, (size_t)c.n * VORS_UNDISTORT_COUNTS * sizeof(uint32_t), s);
    // (out_plane % 4 == 0 with out_cols % 4 == 0, so every plane of the batch starts at the alignment of the first)
    const bool wide = c.out_cols % 4 == 0 && (uintptr_t)c.gray_out % 4 == 0 && (uintptr_t)c.depth_out % 8 == 0;
    UndistortArgs a{0, c, wide ? 1 : 0};
    const unsigned blocks = front_blocks(out_plane);
    for_pair_slices(c.n, [&](int seq0, int ns) {
        a.seq0 = seq0;
        with_bool(c.counts != nullptr, [&](auto k) {
            hipLaunchKernelGGL(undistort_kernel<decltype(k)::value>, dim3(blocks, ns), dim3(FRONT_BLOCK), 0, s, a);
        });
    });
}

void launch_register_depth(const RegisterCall& c, hipStream_t s) {
    const size_t d_plane = (size_t)c.d_rows * (size_t)c.d_cols, c_plane = (size_t)c.c_rows * (size_t)c.c_cols, n = (size_t)c.n;
    // all ones = VORS_ZKEY_EMPTY: nothing has landed (a 32-bit fill over twice as many dwords)
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.zkey), 0xFFFFFFFF, 2 * n * c_plane, s);
    if (c.counts) (void)hipMemsetAsync(c.counts, 0, n * VORS_REGISTER_COUNTS * sizeof(uint32_t), s);
    RegisterArgs a{0, c};
    const bool resolve = c.depth_out || c.src_index || c.counts;
    const unsigned splat_blocks = front_blocks(d_plane), resolve_blocks = front_blocks(c_plane);
    for_pair_slices(c.n, [&](int seq0, int ns) {
        a.seq0 = seq0;
        with_bool(c.counts != nullptr, [&](auto k) {
            constexpr bool COUNTS = decltype(k)::value;
            if (c.footprint == 1) hipLaunchKernelGGL((register_splat_kernel<1, COUNTS>), dim3(splat_blocks, ns), dim3(FRONT_BLOCK), 0, s, a);
            else if (c.footprint == 2) hipLaunchKernelGGL((register_splat_kernel<2, COUNTS>), dim3(splat_blocks, ns), dim3(FRONT_BLOCK), 0, s, a);
            else hipLaunchKernelGGL((register_splat_kernel<3, COUNTS>), dim3(splat_blocks, ns), dim3(FRONT_BLOCK), 0, s, a);
            if (resolve) hipLaunchKernelGGL(register_resolve_kernel<COUNTS>, dim3(resolve_blocks, ns), dim3(FRONT_BLOCK), 0, s, a);
        });
    });
}

}  // namespace vors
