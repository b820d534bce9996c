// vors_depth_normals / vors_points_normals and the normals of the keyframe map: surface normals of level-0 depth planes.
// Handle-free: no Geom, no records; the per-pixel rule is lie.h depth_normal, the text vors_depth_normals_host runs.
// PLANE (depth_normals_kernel): fuse_depth_kernel's shape — elementwise over the plane, 1024 pixels per workgroup. Where every plane allows
//         it (cols % 4 == 0, depth 8-byte and normals 16-byte aligned) a thread takes four adjacent pixels of one row: the centres and the
//         rows above and below as 8-byte loads, the eight horizontal taps as u16 loads, the four 12-byte rows out as three 16-byte stores;
//         else four pixels a workgroup width apart, five u16 loads and three dword stores at consecutive addresses each (normals_device.h
//         normals_narrow_trip, the text the map ICP stage's frame normals run too). All loads of a
//         trip are issued before the first use; a tap outside the plane reads the centre's address. Neighbour rows come through L2: a
//         workgroup's 1024 pixels are a few consecutive rows, read once from HBM and again from the cache by the rows `step` away.
// LIST  (points_normals_kernel): a gather, one point per lane — 4 bytes of pixel, five u16 taps, a 12-byte row out. grid = (chunks of the
//         list) x lists; the counts live on the device, so the x extent is sized from the capacity and capped, a workgroup that starts
//         beyond the clipped range returns at once, a longer range goes through the stride loop (render_splat_kernel's scheme). Masked
//         (sel_list): the keyframe map's launch over the promotion list.
// COUNTS: per-thread integers, added across the wavefront, one LDS sum per workgroup, one global integer atomicAdd per non-zero counter
//         and workgroup into a zeroed array (device_common.h block_counts); compiled out without them. No workgroup waits for
//         another.
#include <algorithm>

#include "normals_device.h"

namespace vors {

struct NormalArgs {
    int seq0;
    NormalCall c;
    int wide;  // plane form: every plane allows four adjacent pixels per thread
};

template <bool COUNTS>
__global__ __launch_bounds__(NORMAL_BLOCK) void depth_normals_kernel(NormalArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? (NORMAL_BLOCK / 64) * VORS_NORMAL_COUNTS : 1];
    const NormalCall& c = a.c;
    const int seq = a.seq0 + blockIdx.y;
    const int plane = c.rows * c.cols;
    const uint16_t* depth = c.depth + (size_t)seq * (size_t)plane;
    float* normals = c.normals ? c.normals + (size_t)seq * (size_t)plane * 3 : nullptr;
    Iso pose = iso_identity();
    if (c.poses) pose = iso_load(c.poses + (size_t)seq * (size_t)c.pose_stride);
    const bool has_pose = c.poses != nullptr;
    const int base = blockIdx.x * (NORMAL_BLOCK * NORMAL_POINTS);
    uint32_t cnt[VORS_NORMAL_COUNTS] = {0u, 0u, 0u};
    if (a.wide) {  // (uniform; cols % 4 == 0: a thread's four pixels share a row and are all inside or all outside)
        const int i = base + NORMAL_POINTS * (int)threadIdx.x;
        if (i < plane) {
            const int y = i / c.cols, x = i - y * c.cols;
            const bool in_u = y - c.step >= 0, in_d = y + c.step < c.rows;
            const ushort4 dc4 = *reinterpret_cast<const ushort4*>(depth + i);
            const ushort4 du4 = *reinterpret_cast<const ushort4*>(depth + (in_u ? i - c.step * c.cols : i));
            const ushort4 dd4 = *reinterpret_cast<const ushort4*>(depth + (in_d ? i + c.step * c.cols : i));
            uint16_t dl[NORMAL_POINTS], dr[NORMAL_POINTS];
#pragma unroll
            for (int j = 0; j < NORMAL_POINTS; ++j) {
                dl[j] = depth[x + j - c.step >= 0 ? i + j - c.step : i + j];
                dr[j] = depth[x + j + c.step < c.cols ? i + j + c.step : i + j];
            }
            DepthNormal o[NORMAL_POINTS];
            const uint16_t dc[NORMAL_POINTS] = {dc4.x, dc4.y, dc4.z, dc4.w}, du[NORMAL_POINTS] = {du4.x, du4.y, du4.z, du4.w},
                           dd[NORMAL_POINTS] = {dd4.x, dd4.y, dd4.z, dd4.w};
#pragma unroll
            for (int j = 0; j < NORMAL_POINTS; ++j) {
                o[j] = depth_normal(c.k, c.depth_scale, c.step, c.jump_m, x + j, y, c.cols, c.rows, dc[j], dl[j], dr[j], du[j], dd[j], has_pose, pose);
                cnt[0] += 1u;
                cnt[1] += o[j].has_depth ? 1u : 0u;
                cnt[2] += o[j].has_normal ? 1u : 0u;
            }
            if (normals) {
                float4* out = reinterpret_cast<float4*>(normals + 3 * (size_t)i);
                out[0] = make_float4(o[0].n.x, o[0].n.y, o[0].n.z, o[1].n.x);
                out[1] = make_float4(o[1].n.y, o[1].n.z, o[2].n.x, o[2].n.y);
                out[2] = make_float4(o[2].n.z, o[3].n.x, o[3].n.y, o[3].n.z);
            }
        }
    } else {
        normals_narrow_trip(c, depth, normals, plane, base, has_pose, pose, cnt);
    }
    if constexpr (COUNTS) block_counts<VORS_NORMAL_COUNTS, NORMAL_BLOCK>(cnt, lds_counts, CountsAdd{c.counts + (size_t)seq * VORS_NORMAL_COUNTS});
}

#define NORMAL_MAX_CHUNKS 1024
template <bool COUNTS>
__global__ __launch_bounds__(NORMAL_BLOCK) void points_normals_kernel(NormalArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? (NORMAL_BLOCK / 64) * VORS_NORMAL_COUNTS : 1];
    const NormalCall& c = a.c;
    int seq = a.seq0 + blockIdx.y;
    if (c.sel_list) {  // masked launch (device_common.h select_pair's rule)
        if (seq >= *c.sel_count) return;
        seq = c.sel_list[seq];
    }
    // the list's range of ranks, clipped to the written prefix (uniform; render_splat_kernel's text)
    const uint32_t n = min(c.list_counts[seq], (uint32_t)c.capacity);
    uint32_t first = 0, last = n;
    if (c.ranges) {
        const uint32_t* r = reinterpret_cast<const uint32_t*>(c.ranges + (size_t)seq * (size_t)c.range_stride);
        first = min(r[0], n);
        last = r[1] > n - first ? n : first + r[1];
    } else if (c.first) {
        first = min(c.first[seq], n);
    }
    // (first <= capacity < 2^31 and the grid spans at most NORMAL_MAX_CHUNKS * NORMAL_BLOCK = 2^18 ranks: nothing below wraps)
    const uint32_t start = first + blockIdx.x * NORMAL_BLOCK;
    if (start >= last) return;  // the whole workgroup
    const int plane = c.rows * c.cols;
    const uint16_t* depth = c.depth + (size_t)seq * (size_t)plane;
    const uint32_t* pixel = c.pixel + (size_t)seq * (size_t)c.capacity;
    float* normals = c.normals ? c.normals + (size_t)seq * (size_t)c.capacity * 3 : nullptr;
    Iso pose = iso_identity();
    if (c.poses) pose = iso_load(c.poses + (size_t)seq * (size_t)c.pose_stride);
    const bool has_pose = c.poses != nullptr;
    uint32_t cnt[VORS_NORMAL_COUNTS] = {0u, 0u, 0u};
    for (uint32_t base = start; base < last; base += gridDim.x * NORMAL_BLOCK) {
        const uint32_t rank = base + threadIdx.x;
        if (rank >= last) continue;
        const uint32_t p = pixel[rank];
        const int x = (int)(p & 0xffffu), y = (int)(p >> 16);
        const bool inside = x < c.cols && y < c.rows;
        const NormalTaps t = inside ? depth_normal_taps(x, y, c.cols, c.rows, c.step) : NormalTaps{0, 0, 0, 0, 0};
        const uint16_t dc = depth[t.c], dl = depth[t.l], dr = depth[t.r], du = depth[t.u], dd = depth[t.d];
        // (a pixel outside the plane: depth_normal returns "no normal" before it looks at a tap)
        const DepthNormal o = depth_normal(c.k, c.depth_scale, c.step, c.jump_m, x, y, c.cols, c.rows, dc, dl, dr, du, dd, has_pose, pose);
        cnt[0] += 1u;
        cnt[1] += o.has_depth ? 1u : 0u;
        cnt[2] += o.has_normal ? 1u : 0u;
        if (normals) {
            float* out = normals + 3 * (size_t)rank;
            out[0] = o.n.x;
            out[1] = o.n.y;
            out[2] = o.n.z;
        }
    }
    if constexpr (COUNTS) block_counts<VORS_NORMAL_COUNTS, NORMAL_BLOCK>(cnt, lds_counts, CountsAdd{c.counts + (size_t)seq * VORS_NORMAL_COUNTS});
}

__global__ void normals_snapshot_kernel(const uint32_t* src, uint32_t* dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

void launch_depth_normals(const NormalCall& c, hipStream_t s) {
    const size_t plane = (size_t)c.rows * (size_t)c.cols;
    if (c.counts) (void)hipMemsetAsync(c.counts, 0, (size_t)c.n * VORS_NORMAL_COUNTS * sizeof(uint32_t), s);
    // (plane % 4 == 0 with cols % 4 == 0, so every plane of the batch starts at the alignment of the first)
    const bool wide = c.cols % 4 == 0 && (uintptr_t)c.depth % 8 == 0 && (uintptr_t)c.normals % 16 == 0;
    NormalArgs a{0, c, wide ? 1 : 0};
    const unsigned blocks = (unsigned)((plane + NORMAL_BLOCK * NORMAL_POINTS - 1) / (NORMAL_BLOCK * NORMAL_POINTS));
    for_pair_slices(c.n, [&](int seq0, int ns) {
        a.seq0 = seq0;
        with_bool(c.counts != nullptr, [&](auto k) {
            hipLaunchKernelGGL(depth_normals_kernel<decltype(k)::value>, dim3(blocks, ns), dim3(NORMAL_BLOCK), 0, s, a);
        });
    });
}

void launch_points_normals(const NormalCall& c, hipStream_t s) {
    if (c.counts) (void)hipMemsetAsync(c.counts, 0, (size_t)c.n * VORS_NORMAL_COUNTS * sizeof(uint32_t), s);
    NormalArgs a{0, c, 0};
    const long long want = ((long long)c.capacity + NORMAL_BLOCK - 1) / NORMAL_BLOCK;
    const unsigned chunks = (unsigned)(want < 1 ? 1 : want > NORMAL_MAX_CHUNKS ? NORMAL_MAX_CHUNKS : want);
    for_pair_slices(c.n, [&](int seq0, int ns) {
        a.seq0 = seq0;
        with_bool(c.counts != nullptr, [&](auto k) {
            hipLaunchKernelGGL(points_normals_kernel<decltype(k)::value>, dim3(chunks, ns), dim3(NORMAL_BLOCK), 0, s, a);
        });
    });
}

void launch_normals_snapshot(const uint32_t* src, uint32_t* dst, int n, hipStream_t s) {
    hipLaunchKernelGGL(normals_snapshot_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n);
}

}  // namespace vors
