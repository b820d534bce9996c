// vors_render_points / vors_trackers_render_map: world-frame point lists rendered into a camera per sequence. Handle-free:
// no Geom, no records; the per-point rule is lie.h render_point / render_footprint / render_resolve, the text vors_render_points_host runs.
// FILL    the key planes to VORS_ZKEY_EMPTY on the stream (the launcher, like launch_lm_fuse_depth).
// SPLAT   (render_splat_kernel): grid = (chunks of the list) x sequences. The counts live on the device, so the x extent is sized from the
//         capacity, capped at RENDER_MAX_CHUNKS; a workgroup that starts beyond the sequence's clipped range returns at once, a longer range
//         goes through the stride loop. A trip takes RENDER_POINTS points per thread a workgroup width apart: consecutive lanes read
//         consecutive 12-byte rows, all loads of a trip issued before the first use. Per written pixel one 64-bit global atomicMin without
//         return value of bits(Z') << 32 | rank: a minimum, bitwise reproducible whatever the order of arrival; no workgroup waits for
//         another. No LDS without COUNTS; with them block_counts (device_common.h) into a zeroed array, like the depth reprojection.
//         (The landing test stays lie.h render_point's: that text is also the host's, and it rounds a footprint, not one pixel.)
// RESOLVE (render_resolve_kernel): fuse_depth_kernel's shape — elementwise over the plane, 1024 pixels per workgroup, four adjacent pixels
//         per thread where every plane allows it (two 16-byte key loads, an 8-byte and a 4-byte store), else four pixels a workgroup width
//         apart; the grey level is gathered from the list at the winning rank. COUNTS: the covered pixels, same pattern.
#include <algorithm>

#include "device_common.h"

namespace vors {

struct RenderSplatArgs {
    int seq0;
    const float* xyz;
    const uint32_t* list_counts;
    int capacity;
    const uint8_t* ranges;
    int range_stride;
    Intr k;
    int rows, cols;
    const float* poses;
    int pose_stride;
    unsigned long long* zkey;
    uint32_t* counts;
};
struct RenderResolveArgs {
    int seq0, plane, capacity;
    float depth_scale;
    const uint64_t* zkey;
    const uint8_t* list_gray;
    uint16_t* depth;
    uint8_t* gray;
    uint32_t* counts;
    int wide;  // every plane allows four pixels per thread
};

#define RENDER_SPLAT_COUNTS 3  // considered, in front, landed (covered is the resolve's)

template <int F, bool COUNTS>
__global__ __launch_bounds__(RENDER_BLOCK) void render_splat_kernel(RenderSplatArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? (RENDER_BLOCK / 64) * RENDER_SPLAT_COUNTS : 1];
    const int seq = a.seq0 + blockIdx.y;
    // the sequence's range of ranks, clipped to the written prefix (uniform)
    const uint32_t n = min(a.list_counts[seq], (uint32_t)a.capacity);
    uint32_t first = 0, last = n;
    if (a.ranges) {
        const uint32_t* r = reinterpret_cast<const uint32_t*>(a.ranges + (size_t)seq * (size_t)a.range_stride);
        first = min(r[0], n);
        last = r[1] > n - first ? n : first + r[1];
    }
    constexpr uint32_t TRIP = RENDER_BLOCK * RENDER_POINTS;
    // (first <= capacity < 2^31 and the grid spans at most RENDER_MAX_CHUNKS * TRIP = 2^20 ranks: nothing below wraps)
    const uint32_t start = first + blockIdx.x * TRIP;
    if (start >= last) return;  // the whole workgroup
    const float* xyz = a.xyz + (size_t)seq * (size_t)a.capacity * 3;
    unsigned long long* zkey = a.zkey + (size_t)seq * (size_t)a.rows * (size_t)a.cols;
    Iso pose = iso_identity();
    if (a.poses) pose = iso_load(a.poses + (size_t)seq * (size_t)a.pose_stride);
    const bool has_pose = a.poses != nullptr;
    uint32_t cnt[RENDER_SPLAT_COUNTS] = {0u, 0u, 0u};
    for (uint32_t base = start; base < last; base += gridDim.x * TRIP) {
        V3 w[RENDER_POINTS];
        bool valid[RENDER_POINTS];
#pragma unroll
        for (int j = 0; j < RENDER_POINTS; ++j) {
            const uint32_t rank = base + j * RENDER_BLOCK + threadIdx.x;
            valid[j] = rank < last;
            const float* p = xyz + 3 * (size_t)(valid[j] ? rank : base);  // (a lane past the end reads the trip's first row: a safe address)
            w[j] = V3{p[0], p[1], p[2]};
        }
#pragma unroll
        for (int j = 0; j < RENDER_POINTS; ++j) {
            if (!valid[j]) continue;
            const uint32_t rank = base + j * RENDER_BLOCK + threadIdx.x;
            const RenderPoint rp = render_point(a.k, has_pose, pose, w[j], F, a.cols, a.rows);
            bool landed = false;
            if (rp.candidate) {
                const unsigned long long key = render_key(rp.z, rank);
                landed = render_footprint(rp, F, a.cols, a.rows, [&](int q) { atomicMin(zkey + q, key); });
            }
            if constexpr (COUNTS) {
                cnt[0] += 1u;
                cnt[1] += rp.in_front ? 1u : 0u;
                cnt[2] += landed ? 1u : 0u;
            }
        }
    }
    if constexpr (COUNTS) block_counts<RENDER_SPLAT_COUNTS, RENDER_BLOCK>(cnt, lds_counts, CountsAdd{a.counts + (size_t)seq * VORS_RENDER_COUNTS});
}

template <bool COUNTS>
__global__ __launch_bounds__(RENDER_BLOCK) void render_resolve_kernel(RenderResolveArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? RENDER_BLOCK / 64 : 1];
    const int seq = a.seq0 + blockIdx.y;
    const size_t off = (size_t)seq * (size_t)a.plane;
    const uint64_t* zkey = a.zkey + off;
    const uint8_t* list_gray = a.list_gray + (size_t)seq * (size_t)a.capacity;
    uint16_t* depth = a.depth ? a.depth + off : nullptr;
    uint8_t* gray = a.gray ? a.gray + off : nullptr;
    const int base = blockIdx.x * (RENDER_BLOCK * RENDER_POINTS);
    uint32_t covered[1] = {0u};
    RenderedPixel o[RENDER_POINTS];
    if (a.wide) {  // (uniform; plane % 4 == 0: a thread's four pixels are all inside or all outside)
        const int i = base + RENDER_POINTS * (int)threadIdx.x;
        if (i < a.plane) {
            const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(zkey + i), k23 = *reinterpret_cast<const ulonglong2*>(zkey + i + 2);
            o[0] = render_resolve(a.depth_scale, k01.x, list_gray);
            o[1] = render_resolve(a.depth_scale, k01.y, list_gray);
            o[2] = render_resolve(a.depth_scale, k23.x, list_gray);
            o[3] = render_resolve(a.depth_scale, k23.y, list_gray);
            if (depth) *reinterpret_cast<ushort4*>(depth + i) = make_ushort4(o[0].depth, o[1].depth, o[2].depth, o[3].depth);
            if (gray)
                *reinterpret_cast<uint32_t*>(gray + i) =
                    (uint32_t)o[0].gray | ((uint32_t)o[1].gray << 8) | ((uint32_t)o[2].gray << 16) | ((uint32_t)o[3].gray << 24);
#pragma unroll
            for (int j = 0; j < RENDER_POINTS; ++j) covered[0] += o[j].covered ? 1u : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < RENDER_POINTS; ++j) {
            const int i = base + j * RENDER_BLOCK + (int)threadIdx.x;
            if (i >= a.plane) continue;
            o[j] = render_resolve(a.depth_scale, zkey[i], list_gray);
            if (depth) depth[i] = o[j].depth;
            if (gray) gray[i] = o[j].gray;
            covered[0] += o[j].covered ? 1u : 0u;
        }
    }
    if constexpr (COUNTS) block_counts<1, RENDER_BLOCK>(covered, lds_counts, CountsAdd{a.counts + (size_t)seq * VORS_RENDER_COUNTS + 3});
}

void launch_render_points(const RenderCall& c, hipStream_t s) {
    const size_t plane = (size_t)c.rows * (size_t)c.cols, n = (size_t)c.n;
    // all ones = VORS_ZKEY_EMPTY: nothing has landed (a 32-bit fill over twice as many dwords)
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.zkey), 0xFFFFFFFF, 2 * n * plane, s);
    if (c.counts) (void)hipMemsetAsync(c.counts, 0, n * VORS_RENDER_COUNTS * sizeof(uint32_t), s);
    RenderSplatArgs a{0, c.xyz, c.list_counts, c.capacity, c.ranges, c.range_stride, c.k, c.rows, c.cols, c.poses, c.pose_stride,
                      reinterpret_cast<unsigned long long*>(c.zkey), c.counts};
    const bool resolve = c.depth || c.gray || c.counts;
    const bool wide = plane % 4 == 0 && (uintptr_t)c.zkey % 16 == 0 && (uintptr_t)c.depth % 8 == 0 && (uintptr_t)c.gray % 4 == 0;
    RenderResolveArgs m{0, (int)plane, c.capacity, c.depth_scale, c.zkey, c.list_gray, c.depth, c.gray, c.counts, wide ? 1 : 0};
    const unsigned chunks = (unsigned)render_chunks(c.capacity);
    const unsigned blocks = (unsigned)((plane + RENDER_BLOCK * RENDER_POINTS - 1) / (RENDER_BLOCK * RENDER_POINTS));
    for_pair_slices(c.n, [&](int seq0, int ns) {
        a.seq0 = m.seq0 = seq0;
        with_bool(c.counts != nullptr, [&](auto k) {
            constexpr bool COUNTS = decltype(k)::value;
            if (c.footprint == 1) hipLaunchKernelGGL((render_splat_kernel<1, COUNTS>), dim3(chunks, ns), dim3(RENDER_BLOCK), 0, s, a);
            else if (c.footprint == 2) hipLaunchKernelGGL((render_splat_kernel<2, COUNTS>), dim3(chunks, ns), dim3(RENDER_BLOCK), 0, s, a);
            else hipLaunchKernelGGL((render_splat_kernel<3, COUNTS>), dim3(chunks, ns), dim3(RENDER_BLOCK), 0, s, a);
            if (resolve) hipLaunchKernelGGL(render_resolve_kernel<COUNTS>, dim3(blocks, ns), dim3(RENDER_BLOCK), 0, s, m);
        });
    });
}

}  // namespace vors
