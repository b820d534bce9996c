// The voxel table of ONE point list as device code sees it, and its two probes: the text the keyframe map's filtered emission
// (product_kernels.hip point_cloud_append_voxel_kernel) and the handle-free filter of point lists (repose_kernels.hip) both compile.
// Device only; the key itself is lie.h voxel_key, host + device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lie.h"

namespace vors {

// Entry e is the two words table[2 e] = voxel key (empty: all ones) and table[2 e + 1] = owner tag (unclaimed: all ones). For the map,
// `tag_hi` is the segment index of the keyframe being emitted << 32; a point's tag is tag_hi | its slot in the level's source, so tags
// ascend in the map's rank order. For a plain list the tag is the rank.
struct CloudVox {
    unsigned long long* table;
    uint32_t* occupied;
    uint32_t* overflow;
    uint32_t mask;  // table_slots - 1
    float voxel_m;
    unsigned long long tag_hi;
    Iso pose;       // the keyframe pose: the key is taken of the world point WRITE stores
};
#define VOXEL_EMPTY 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ uint32_t voxel_hash(unsigned long long key) {  // (the 64-bit finaliser of MurmurHash3)
    key ^= key >> 33;
    key *= 0xff51afd7ed558ccdull;
    key ^= key >> 33;
    key *= 0xc4ceb9fe1a85ec53ull;
    key ^= key >> 33;
    return (uint32_t)key;
}
__device__ __forceinline__ bool voxel_overflowed(const CloudVox& v) { return __hip_atomic_load(v.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0; }
// CLAIM: linear probing from the key's home entry. An empty entry is taken with one compare-and-swap on the key word (a lost race hands
// back the winner's key, which is then compared like any other); on the entry that holds the key, ONE minimum on the owner word. Every
// step either ends the probe or moves on: no thread waits for another. table_slots entries without success — the list has more
// voxels than entries — set the sticky overflow word, which every probe reads at entry and every 64 steps and then gives up.
__device__ __forceinline__ void voxel_claim(const CloudVox& v, unsigned long long key, unsigned long long tag) {
    if (key == VOXEL_EMPTY) return;  // (no key: the point is dropped and not counted)
    uint32_t e = voxel_hash(key) & v.mask;
    for (uint32_t step = 0; step <= v.mask; ++step, e = (e + 1u) & v.mask) {
        if ((step & 63u) == 0u && voxel_overflowed(v)) return;
        unsigned long long* kp = v.table + 2 * (size_t)e;
        unsigned long long k = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == VOXEL_EMPTY) {
            k = atomicCAS(kp, VOXEL_EMPTY, key);
            if (k == VOXEL_EMPTY) {
                atomicAdd(v.occupied, 1u);
                k = key;
            }
        }
        if (k == key) {
            atomicMin(kp + 1, tag);
            return;
        }
    }
    atomicOr(v.overflow, 1u);
}
// COUNT / WRITE: the same probe, reading only (the table does not change during these launches). True iff the voxel's owner is `tag`.
// After an overflow nothing is owned: the list contributes no point, in both sweeps alike.
__device__ __forceinline__ bool voxel_owns(const CloudVox& v, unsigned long long key, unsigned long long tag) {
    if (key == VOXEL_EMPTY) return false;
    uint32_t e = voxel_hash(key) & v.mask;
    for (uint32_t step = 0; step <= v.mask; ++step, e = (e + 1u) & v.mask) {
        if ((step & 63u) == 0u && voxel_overflowed(v)) return false;
        const unsigned long long k = v.table[2 * (size_t)e];
        if (k == key) return v.table[2 * (size_t)e + 1] == tag;
        if (k == VOXEL_EMPTY) return false;  // (never claimed: only after an overflow cut CLAIM short)
    }
    return false;
}

}  // namespace vors
