// Re-posing of point lists after pose-graph optimisation and the voxel filter of plain point lists (include/vors_hip.h 2i).
// Every per-item text is lie.h's (repose_*, voxel_key, voxel_filter_below) or voxel_table_device.h's (voxel_claim, voxel_owns): the
// host twins in operators.cpp run the same ones. Integer atomics only; no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "engine.h"
#include "lie.h"
#include "voxel_table_device.h"

namespace vors {

// ------------------------------------------------------------------------------------------------------------
// vors_repose_points. POINT PASS: a workgroup owns REPOSE_CHUNK consecutive ranks of one list (grid y), a lane REPOSE_GROUP consecutive
// ranks: three aligned 16-byte loads and stores per array when the list's base is 16-byte aligned and the group lies inside the clipped
// count, per-point access otherwise (the tail, a list at an odd offset). The lane reads its ranks first and writes them last, so that an
// output may be the input. The segment of the chunk's first rank is found ONCE, by a binary search over `first` on values that are the
// same for the whole workgroup; from there the workgroup walks forward over the records that reach into the chunk, reads the two poses
// of each once (addresses uniform over the workgroup) and every lane transforms the ranks of its group that lie in the record's range.
// A list's workgroups stride over its chunks. Counts: per lane across its chunks, a shuffle reduction, the wavefronts' sums through
// LDS, one integer atomic per workgroup and counter.
// RECORD PASS (behind it on the stream, so that segments_out may be segments): one lane per recorded segment.
// ------------------------------------------------------------------------------------------------------------
#define REPOSE_BLOCK 256
#define REPOSE_GROUP 4
#define REPOSE_CHUNK (REPOSE_BLOCK * REPOSE_GROUP)

// A lane's group of an [..][3] f32 list, ranks rb .. rb + 3: whole (three float4) or rank by rank below `end`.
__device__ __forceinline__ void repose_load_group(const float* list, uint32_t rb, uint32_t end, bool whole, float v[3 * REPOSE_GROUP]) {
    if (whole) {
        const float4* s = reinterpret_cast<const float4*>(list + 3 * (size_t)rb);
        const float4 a = s[0], b = s[1], c = s[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < REPOSE_GROUP; ++j) {
        const bool in = rb + (uint32_t)j < end;
        const float* s = list + 3 * (size_t)(rb + (uint32_t)j);
#pragma unroll
        for (int a = 0; a < 3; ++a) v[3 * j + a] = in ? s[a] : 0.0f;
    }
}
__device__ __forceinline__ void repose_store_group(float* list, uint32_t rb, uint32_t end, bool whole, const float v[3 * REPOSE_GROUP]) {
    if (whole) {
        float4* d = reinterpret_cast<float4*>(list + 3 * (size_t)rb);
        d[0] = make_float4(v[0], v[1], v[2], v[3]);
        d[1] = make_float4(v[4], v[5], v[6], v[7]);
        d[2] = make_float4(v[8], v[9], v[10], v[11]);
        return;
    }
#pragma unroll
    for (int j = 0; j < REPOSE_GROUP; ++j) {
        if (rb + (uint32_t)j >= end) continue;
        float* d = list + 3 * (size_t)(rb + (uint32_t)j);
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = v[3 * j + a];
    }
}

// One chunk of list i: the ranks [r0, r0 + REPOSE_CHUNK) below `total`. n4 / shift: the lane's running counters.
template <bool NORMALS>
__device__ __forceinline__ void repose_chunk(const ReposeCall& c, int i, uint32_t total, uint32_t r0, uint32_t n4[4], uint32_t& shift) {
    const uint32_t end = total - r0 < (uint32_t)REPOSE_CHUNK ? total : r0 + (uint32_t)REPOSE_CHUNK;
    const size_t row = (size_t)i * (size_t)c.capacity;
    const float* xin = c.xyz + 3 * row;
    float* xout = c.xyz_out ? c.xyz_out + 3 * row : nullptr;
    const float* nin = NORMALS ? c.normals + 3 * row : nullptr;
    float* nout = NORMALS ? c.normals_out + 3 * row : nullptr;
    const bool aligned = (((uintptr_t)xin | (uintptr_t)xout | (uintptr_t)nin | (uintptr_t)nout) & 15u) == 0u;
    const uint32_t rb = r0 + (uint32_t)REPOSE_GROUP * threadIdx.x;
    const bool whole = aligned && rb < end && end - rb >= (uint32_t)REPOSE_GROUP;

    float p[3 * REPOSE_GROUP], nv[NORMALS ? 3 * REPOSE_GROUP : 1];
    repose_load_group(xin, rb, end, whole, p);
    if constexpr (NORMALS) repose_load_group(nin, rb, end, whole, nv);
    bool pfin[REPOSE_GROUP], nfin[REPOSE_GROUP];
    uint32_t code[REPOSE_GROUP];  // 0 = no record, 1 = kept, 2 = moved
#pragma unroll
    for (int j = 0; j < REPOSE_GROUP; ++j) {
        pfin[j] = repose_finite3(V3{p[3 * j], p[3 * j + 1], p[3 * j + 2]});
        nfin[j] = NORMALS ? repose_finite3(V3{nv[NORMALS ? 3 * j : 0], nv[NORMALS ? 3 * j + 1 : 0], nv[NORMALS ? 3 * j + 2 : 0]}) : false;
        code[j] = 0u;
    }

    // the records that reach into [r0, end): from the last one whose `first` is <= r0 on
    const uint32_t n_seg = c.n_segments[i], n_rec = n_seg < (uint32_t)c.max_keyframes ? n_seg : (uint32_t)c.max_keyframes;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(c.segments + (size_t)i * (size_t)c.max_keyframes);
    const uint32_t* node_of = c.node_of_segment ? c.node_of_segment + (size_t)i * (size_t)c.max_keyframes : nullptr;
    const float* poses = c.poses_new + (size_t)i * (size_t)c.node_capacity * (size_t)c.pose_stride;
    const uint32_t node_count = c.node_counts[i];
    if (n_rec) {
        uint32_t lo = 0, hi = n_rec;  // the last index in [0, n_rec) with first <= r0 (voxel_means_kernel's search)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (words[(size_t)mid * MAP_SEGMENT_WORDS + 1] <= r0) lo = mid;
            else hi = mid;
        }
        for (uint32_t k = lo; k < n_rec; ++k) {
            if (words[(size_t)k * MAP_SEGMENT_WORDS + 1] >= end) break;  // ascending: no later record reaches into the chunk
            uint32_t s_lo, s_hi;
            repose_segment_ranks(words, k, n_rec, total, &s_lo, &s_hi);
            if (s_lo < r0) s_lo = r0;
            if (s_hi > end) s_hi = end;
            if (s_lo >= s_hi) continue;
            float a7[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) a7[q] = __builtin_bit_cast(float, words[(size_t)k * MAP_SEGMENT_WORDS + 3 + q]);
            const uint32_t node = repose_node(k, node_of, node_count, c.node_capacity);
            const float* b7 = node != VORS_REPOSE_NO_NODE ? poses + (size_t)node * (size_t)c.pose_stride : nullptr;
            const bool moved = repose_moves(a7, b7);
            const Iso A = iso_load(a7), B = moved ? iso_load(b7) : A;
#pragma unroll
            for (int j = 0; j < REPOSE_GROUP; ++j) {
                const uint32_t r = rb + (uint32_t)j;
                if (r < s_lo || r >= s_hi) continue;
                code[j] = moved ? 2u : 1u;
                if (!moved) continue;
                if (pfin[j]) {
                    const V3 w{p[3 * j], p[3 * j + 1], p[3 * j + 2]};
                    const V3 m = repose_point(A, B, w);
                    const uint32_t sb = repose_shift_bits(w, m);
                    shift = sb > shift ? sb : shift;
                    p[3 * j] = m.x; p[3 * j + 1] = m.y; p[3 * j + 2] = m.z;
                }
                if constexpr (NORMALS) {
                    if (nfin[j]) {
                        const V3 m = repose_normal(A, B, V3{nv[3 * j], nv[3 * j + 1], nv[3 * j + 2]});
                        nv[3 * j] = m.x; nv[3 * j + 1] = m.y; nv[3 * j + 2] = m.z;
                    }
                }
            }
        }
    }
    if (xout) repose_store_group(xout, rb, end, whole, p);
    if constexpr (NORMALS) repose_store_group(nout, rb, end, whole, nv);

#pragma unroll
    for (int j = 0; j < REPOSE_GROUP; ++j) {
        if (rb + (uint32_t)j >= end) continue;
        const int what = !pfin[j] ? REPOSE_NONFINITE : code[j] == 0u ? REPOSE_NO_RECORD : code[j] == 2u ? REPOSE_MOVED : REPOSE_KEPT;
#pragma unroll
        for (int q = 0; q < 4; ++q) n4[q] += what == q ? 1u : 0u;
    }
}

// The workgroups of a list stride over its chunks (at most REPOSE_MOST_BLOCKS of them per list), so that the counters cost one set of
// integer atomics per workgroup whatever the list's length: thousands of atomics on one word would otherwise outlast the stream.
#define REPOSE_MOST_BLOCKS 1024
template <bool NORMALS>
__global__ __launch_bounds__(REPOSE_BLOCK) void repose_points_kernel(ReposeCall c) {
    __shared__ uint32_t lds[REPOSE_BLOCK / 64][5];
    const int i = blockIdx.y;
    const uint32_t count = c.list_counts[i], total = count < (uint32_t)c.capacity ? count : (uint32_t)c.capacity;
    const uint32_t chunks = total / (uint32_t)REPOSE_CHUNK + (total % (uint32_t)REPOSE_CHUNK ? 1u : 0u);
    uint32_t n4[4] = {0u, 0u, 0u, 0u}, shift = 0u;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x)  // (uniform)
        repose_chunk<NORMALS>(c, i, total, chunk * (uint32_t)REPOSE_CHUNK, n4, shift);
    if (!c.counts_out || blockIdx.x >= chunks) return;  // the whole workgroup
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) n4[q] += __shfl_down(n4[q], off, 64);
        const uint32_t other = __shfl_down(shift, off, 64);
        shift = other > shift ? other : shift;
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) lds[threadIdx.x >> 6][q] = n4[q];
        lds[threadIdx.x >> 6][4] = shift;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        uint32_t v = 0;
        for (int w = 0; w < REPOSE_BLOCK / 64; ++w) v = threadIdx.x < 4 ? v + lds[w][threadIdx.x] : (lds[w][4] > v ? lds[w][4] : v);
        uint32_t* out = c.counts_out + (size_t)i * VORS_REPOSE_COUNTS;
        if (v) {
            if (threadIdx.x < 4) atomicAdd(out + threadIdx.x, v);
            else atomicMax(out + REPOSE_MAX_SHIFT, v);
        }
    }
}

__global__ __launch_bounds__(REPOSE_BLOCK) void repose_segments_kernel(ReposeCall c) {
    const int i = blockIdx.y;
    const uint32_t n_seg = c.n_segments[i], n_rec = n_seg < (uint32_t)c.max_keyframes ? n_seg : (uint32_t)c.max_keyframes;
    const uint32_t k = blockIdx.x * (uint32_t)REPOSE_BLOCK + threadIdx.x;
    if (k >= n_rec) return;
    const size_t at = ((size_t)i * (size_t)c.max_keyframes + k) * MAP_SEGMENT_WORDS;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(c.segments) + at;
    uint32_t w[MAP_SEGMENT_WORDS];
#pragma unroll
    for (int q = 0; q < MAP_SEGMENT_WORDS; ++q) w[q] = in[q];
    float a7[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) a7[q] = __builtin_bit_cast(float, w[3 + q]);
    const uint32_t* node_of = c.node_of_segment ? c.node_of_segment + (size_t)i * (size_t)c.max_keyframes : nullptr;
    const uint32_t node = repose_node(k, node_of, c.node_counts[i], c.node_capacity);
    const float* b7 = node != VORS_REPOSE_NO_NODE
                          ? c.poses_new + ((size_t)i * (size_t)c.node_capacity + node) * (size_t)c.pose_stride : nullptr;
    const bool moved = repose_moves(a7, b7);
    if (moved) {
#pragma unroll
        for (int q = 0; q < 7; ++q) w[3 + q] = repose_bits(b7[q]);
    }
    if (c.segments_out) {
        uint32_t* out = reinterpret_cast<uint32_t*>(c.segments_out) + at;
#pragma unroll
        for (int q = 0; q < MAP_SEGMENT_WORDS; ++q) out[q] = w[q];
    }
    if (c.counts_out && moved) atomicAdd(c.counts_out + (size_t)i * VORS_REPOSE_COUNTS + REPOSE_SEGMENTS_MOVED, 1u);
}

void launch_repose_points(const ReposeCall& c, hipStream_t s) {
    if (c.counts_out) (void)hipMemsetAsync(c.counts_out, 0, (size_t)c.n * VORS_REPOSE_COUNTS * sizeof(uint32_t), s);
    const dim3 grid(std::min(((unsigned)c.capacity + REPOSE_CHUNK - 1) / REPOSE_CHUNK, (unsigned)REPOSE_MOST_BLOCKS), c.n);
    if (c.normals_out) hipLaunchKernelGGL(repose_points_kernel<true>, grid, dim3(REPOSE_BLOCK), 0, s, c);
    else hipLaunchKernelGGL(repose_points_kernel<false>, grid, dim3(REPOSE_BLOCK), 0, s, c);
    if (c.segments_out || c.counts_out)
        hipLaunchKernelGGL(repose_segments_kernel, dim3(((unsigned)c.max_keyframes + REPOSE_BLOCK - 1) / REPOSE_BLOCK, c.n), dim3(REPOSE_BLOCK), 0, s, c);
}

// ------------------------------------------------------------------------------------------------------------
// vors_voxel_filter_points: one point per occupied voxel, the first in the list's order — the keyframe map's filter (product_kernels.hip
// point_cloud_append_voxel_kernel) for a list that already exists, through the same probes with the RANK as the tag.
//   EMPTY     the tables to all ones, the words (occupied, overflow, count) to zero
//   CLAIM     every rank below the clipped count enters its list's table: the owner word of a voxel ends as the minimum rank
//   COUNT     per chunk of VORS_VFILTER_CHUNK ranks, those that own their voxel
//   SCAN      per list, the exclusive prefix of the chunk counts in place and the total
//   WRITE     ordered compaction: a chunk's owners behind the chunk's prefix, in rank order (ballot and popcount per wavefront, the
//             wavefronts' totals through LDS), with the gathers
//   SEGMENTS  one lane per recorded segment: lie.h voxel_filter_below of its two ends
// A chunk is four sweeps of the workgroup's 256 lanes over consecutive ranks, so the order of ranks is sweep, wavefront, lane.
// ------------------------------------------------------------------------------------------------------------
#define VFILTER_BLOCK 256
#define VFILTER_SWEEPS (VORS_VFILTER_CHUNK / VFILTER_BLOCK)
static_assert(VORS_VFILTER_CHUNK % VFILTER_BLOCK == 0, "a chunk is whole sweeps of the workgroup");

__device__ __forceinline__ CloudVox vfilter_vox(const VoxelFilterCall& c, int i) {
    CloudVox v;
    v.table = c.table + 2 * (size_t)i * (size_t)c.table_slots;
    v.occupied = c.occupied + i;
    v.overflow = c.overflow + i;
    v.mask = (uint32_t)c.table_slots - 1u;
    v.voxel_m = c.voxel_m;
    v.tag_hi = 0ull;
    v.pose = iso_identity();
    return v;
}
__device__ __forceinline__ uint32_t vfilter_total(const VoxelFilterCall& c, int i) {
    const uint32_t count = c.list_counts[i];
    return count < (uint32_t)c.capacity ? count : (uint32_t)c.capacity;
}
__device__ __forceinline__ unsigned long long vfilter_key(const VoxelFilterCall& c, size_t row, uint32_t r) {
    const float* w = c.xyz + 3 * (row + r);
    return voxel_key(c.voxel_m, w[0], w[1], w[2]);
}

__global__ __launch_bounds__(VFILTER_BLOCK) void voxel_filter_empty_kernel(VoxelFilterCall c) {
    const size_t entries = (size_t)c.n * (size_t)c.table_slots, step = (size_t)gridDim.x * VFILTER_BLOCK;
    const size_t t = (size_t)blockIdx.x * VFILTER_BLOCK + threadIdx.x;
    ulonglong2* table = reinterpret_cast<ulonglong2*>(c.table);
    for (size_t e = t; e < entries; e += step) table[e] = make_ulonglong2(VOXEL_EMPTY, VOXEL_EMPTY);
    for (size_t i = t; i < (size_t)c.n; i += step) {
        c.occupied[i] = 0u;
        c.overflow[i] = 0u;
        c.counts_out[i] = 0u;
    }
}

template <bool CLAIM>
__global__ __launch_bounds__(VFILTER_BLOCK) void voxel_filter_sweep_kernel(VoxelFilterCall c) {
    __shared__ uint32_t lds[VFILTER_BLOCK / 64];
    const int i = blockIdx.y;
    const uint32_t total = vfilter_total(c, i), r0 = blockIdx.x * (uint32_t)VORS_VFILTER_CHUNK;
    uint32_t owned = 0;
    if (r0 < total) {  // (uniform)
        const CloudVox v = vfilter_vox(c, i);
        const size_t row = (size_t)i * (size_t)c.capacity;
#pragma unroll
        for (int j = 0; j < VFILTER_SWEEPS; ++j) {
            const uint32_t r = r0 + (uint32_t)j * VFILTER_BLOCK + threadIdx.x;
            if (r >= total) continue;
            const unsigned long long key = vfilter_key(c, row, r);
            if constexpr (CLAIM) voxel_claim(v, key, (unsigned long long)r);
            else owned += voxel_owns(v, key, (unsigned long long)r) ? 1u : 0u;
        }
    }
    if constexpr (!CLAIM) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) owned += __shfl_down(owned, off, 64);
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = owned;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t sum = 0;
            for (int w = 0; w < VFILTER_BLOCK / 64; ++w) sum += lds[w];
            c.chunk_counts[(size_t)i * (size_t)c.chunks + blockIdx.x] = sum;
        }
    }
}

__global__ __launch_bounds__(VFILTER_BLOCK) void voxel_filter_scan_kernel(VoxelFilterCall c) {
    __shared__ uint32_t buf[VFILTER_BLOCK];
    const int i = blockIdx.x;
    uint32_t* cc = c.chunk_counts + (size_t)i * (size_t)c.chunks;
    uint32_t run = 0;
    for (int base = 0; base < c.chunks; base += VFILTER_BLOCK) {
        const int at = base + (int)threadIdx.x;
        const uint32_t own = at < c.chunks ? cc[at] : 0u;
        buf[threadIdx.x] = own;
        __syncthreads();
        for (int off = 1; off < VFILTER_BLOCK; off <<= 1) {  // inclusive, in place
            const uint32_t add = (int)threadIdx.x >= off ? buf[threadIdx.x - off] : 0u;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (at < c.chunks) cc[at] = run + buf[threadIdx.x] - own;
        run += buf[VFILTER_BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) c.counts_out[i] = run;
}

__global__ __launch_bounds__(VFILTER_BLOCK) void voxel_filter_write_kernel(VoxelFilterCall c) {
    __shared__ uint32_t lds[VFILTER_BLOCK / 64];
    const int i = blockIdx.y;
    const uint32_t total = vfilter_total(c, i), r0 = blockIdx.x * (uint32_t)VORS_VFILTER_CHUNK;
    if (r0 >= total) return;  // the whole workgroup
    const CloudVox v = vfilter_vox(c, i);
    const size_t row = (size_t)i * (size_t)c.capacity;
    uint32_t at = c.chunk_counts[(size_t)i * (size_t)c.chunks + blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int j = 0; j < VFILTER_SWEEPS; ++j) {
        const uint32_t r = r0 + (uint32_t)j * VFILTER_BLOCK + threadIdx.x;
        const bool own = r < total && voxel_owns(v, vfilter_key(c, row, r), (unsigned long long)r);
        const unsigned long long mask = __ballot(own);
        if (lane == 0) lds[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0, sweep = 0;
#pragma unroll
        for (uint32_t w = 0; w < VFILTER_BLOCK / 64; ++w) {
            before += w < wave ? lds[w] : 0u;
            sweep += lds[w];
        }
        const uint32_t dst = at + before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (own && dst < (uint32_t)c.capacity) {  // (dst < the list's kept total <= capacity; tested all the same)
            c.index[row + dst] = r;
            if (c.xyz_out) {
                const float* s = c.xyz + 3 * (row + r);
                float* d = c.xyz_out + 3 * (row + dst);
                d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
            }
            if (c.pixel_out) c.pixel_out[row + dst] = c.pixel[row + r];
            if (c.gray_out) c.gray_out[row + dst] = c.gray[row + r];
            if (c.normals_out) {
                const float* s = c.normals + 3 * (row + r);
                float* d = c.normals_out + 3 * (row + dst);
                d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
            }
        }
        at += sweep;
        __syncthreads();  // lds is written again by the next sweep
    }
}

__global__ __launch_bounds__(VFILTER_BLOCK) void voxel_filter_segments_kernel(VoxelFilterCall c) {
    const int i = blockIdx.y;
    const uint32_t n_seg = c.n_segments[i], n_rec = n_seg < (uint32_t)c.max_keyframes ? n_seg : (uint32_t)c.max_keyframes;
    const uint32_t k = blockIdx.x * (uint32_t)VFILTER_BLOCK + threadIdx.x;
    if (k >= n_rec) return;
    const size_t at = ((size_t)i * (size_t)c.max_keyframes + k) * MAP_SEGMENT_WORDS;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(c.segments) + at;
    uint32_t* out = reinterpret_cast<uint32_t*>(c.segments_out) + at;
    const uint32_t total = vfilter_total(c, i);
    uint32_t kept = c.counts_out[i];
    if (kept > total) kept = total;  // (never: the searches stay inside the list whatever the word holds)
    const uint32_t* index = c.index + (size_t)i * (size_t)c.capacity;
    const uint32_t first = in[1], count = in[2];
    const uint32_t lo = voxel_filter_below(index, kept, (uint64_t)first), hi = voxel_filter_below(index, kept, (uint64_t)first + (uint64_t)count);
    out[0] = in[0];
    out[1] = lo;
    out[2] = hi - lo;
#pragma unroll
    for (int q = 3; q < MAP_SEGMENT_WORDS; ++q) out[q] = in[q];
}

size_t voxel_filter_workspace_carve(VoxelFilterCall* call, void* workspace, int n, int capacity, int table_slots) {
    const size_t chunks = ((size_t)capacity + VORS_VFILTER_CHUNK - 1) / VORS_VFILTER_CHUNK;
    const size_t table = (size_t)n * (size_t)table_slots * 16, counts = (size_t)n * chunks * sizeof(uint32_t), words = (size_t)n * sizeof(uint32_t);
    if (call && workspace) {
        char* p = static_cast<char*>(workspace);
        call->table = reinterpret_cast<unsigned long long*>(p);
        call->chunk_counts = reinterpret_cast<uint32_t*>(p + table);
        call->occupied = reinterpret_cast<uint32_t*>(p + table + counts);
        call->chunks = (int)chunks;
    }
    return table + counts + words;
}

void launch_voxel_filter_points(const VoxelFilterCall& c, hipStream_t s) {
    const size_t entries = (size_t)c.n * (size_t)c.table_slots;
    const unsigned empty_blocks = (unsigned)std::min<size_t>((entries + VFILTER_BLOCK - 1) / VFILTER_BLOCK, 4096);
    const dim3 grid(c.chunks, c.n), block(VFILTER_BLOCK);
    hipLaunchKernelGGL(voxel_filter_empty_kernel, dim3(empty_blocks), block, 0, s, c);
    hipLaunchKernelGGL(voxel_filter_sweep_kernel<true>, grid, block, 0, s, c);
    hipLaunchKernelGGL(voxel_filter_sweep_kernel<false>, grid, block, 0, s, c);
    hipLaunchKernelGGL(voxel_filter_scan_kernel, dim3(c.n), block, 0, s, c);
    hipLaunchKernelGGL(voxel_filter_write_kernel, grid, block, 0, s, c);
    if (c.segments_out)
        hipLaunchKernelGGL(voxel_filter_segments_kernel, dim3(((unsigned)c.max_keyframes + VFILTER_BLOCK - 1) / VFILTER_BLOCK, c.n), block, 0, s, c);
}

}  // namespace vors
