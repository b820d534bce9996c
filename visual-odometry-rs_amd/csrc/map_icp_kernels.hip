// The map ICP correction at keyframe promotion (vors_trackers_enable_map_icp): what surrounds the robust ICP pass
// (icp_kernels.hip) in a track call. A translation unit of its own. The two
// rules are lie.h map_icp_window / map_icp_verdict, the texts vors_map_icp_window_host / vors_map_icp_verdict_host run.
// ARM    (map_icp_arm_kernel): one thread per sequence. The promotion list holds every promoted sequence once, so a thread finds its own
//        flag by scanning it (at most n entries of 4 bytes, read by every thread from the cache) — no scatter, no second launch, no
//        ordering between threads. It writes the window — (0, 0) for a sequence that is not promoted: its evaluation workgroups then
//        return at once and the first solve freezes it TOO_FEW — copies the keyframe pose into the start pose and resets the record.
// FRAME NORMALS (map_icp_frame_normals_kernel): the plane form of the normals pass for the promoted sequences only. depth_normals_kernel
//        knows no selection; this kernel runs its narrow trip (normals_device.h normals_narrow_trip: four pixels a workgroup width apart,
//        five u16 taps, three dword stores each) under select_pair's rule, without pose and counts: hence vors_depth_normals' bits.
// APPLY  (map_icp_apply_kernel): one thread per entry of the promotion list. The verdict; ACCEPTED: the ICP's pose into the three pose
//        tables; the record; the totals (plain read-modify-write: a sequence is on the list once).
// JOINT  (vors_trackers_enable_map_icp_joint): map_icp_arm_joint_kernel, map_icp_apply_joint_kernel and icp_condition_kernel,
//        described where they stand, behind APPLY.
// Every index is a sequence below n or a pixel below rows * cols; a list entry outside 0..n-1 (there is none) is skipped, not trusted.
#include <cstddef>

#include "normals_device.h"

namespace vors {

static_assert(sizeof(vors_map_segment) == MAP_SEGMENT_WORDS * 4 && offsetof(vors_map_segment, first) == 4,
              "lie.h map_icp_window reads `first` at word 1 of ten");
static_assert(sizeof(vors_map_icp_record) == 112, "vors_map_icp_record is 112 bytes");

__global__ void map_icp_arm_kernel(MapIcpCall c) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= c.n) return;
    const int np = min(max(*c.promo_count, 0), c.n);
    uint32_t promoted = 0u;
    for (int k = 0; k < np; ++k) promoted |= c.promo_list[k] == seq ? 1u : 0u;
    c.promoted[seq] = promoted;
    uint32_t range[2] = {0u, 0u};
    if (promoted)
        map_icp_window(reinterpret_cast<const uint32_t*>(c.segments + (size_t)seq * (size_t)c.max_keyframes), c.n_segments[seq], c.max_keyframes,
                       c.counts[seq], c.capacity, c.last_keyframes, range);
    c.ranges[2 * seq] = range[0];
    c.ranges[2 * seq + 1] = range[1];
    vors_map_icp_record r{};
    r.frame = c.kf_frame[seq];
    r.verdict = VORS_MAP_ICP_NOT_ATTEMPTED;
    r.range_first = range[0];
    r.range_count = range[1];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const float v = c.kf_poses[(size_t)seq * 7 + i];
        c.start_poses[(size_t)seq * 7 + i] = v;
        r.pose_before[i] = v;
        r.pose_after[i] = v;
    }
    c.records[seq] = r;
}

__global__ void map_icp_apply_kernel(MapIcpCall c) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= min(max(*c.promo_count, 0), c.n)) return;
    const int seq = c.promo_list[k];
    if (seq < 0 || seq >= c.n) return;
    vors_map_icp_record& r = c.records[seq];
    const vors_icp_stats st = c.stats[seq];
    float after[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) after[i] = c.result_poses[(size_t)seq * 7 + i];
    const MapIcpVerdict v = map_icp_verdict(c.gates, st.status, st.matched, st.considered, st.rms, r.pose_before, after);
    r.verdict = (uint32_t)v;
    r.stats = st;
#pragma unroll
    for (int g = 0; g < VORS_ICP_GATE_COUNTS; ++g) r.gate_counts[g] = c.gate_counts[(size_t)seq * VORS_ICP_GATE_COUNTS + g];
#pragma unroll
    for (int i = 0; i < 7; ++i) r.pose_after[i] = after[i];
    c.totals[2 * seq] += 1u;
    if (v == MAP_ICP_ACCEPTED) {
        c.totals[2 * seq + 1] += 1u;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            c.kf_poses[(size_t)seq * 7 + i] = after[i];
            c.cur_poses[(size_t)seq * 7 + i] = after[i];
            c.out_poses[(size_t)seq * 7 + i] = after[i];
        }
    }
}

// The joint stage (vors_trackers_enable_map_icp_joint). ARM is map_icp_arm_kernel as it stands, followed by
// map_icp_arm_joint_kernel: one thread per sequence, the joint record reset to zeros. APPLY is replaced by map_icp_apply_joint_kernel:
// map_icp_apply_kernel's index discipline and its writes, word for word, around lie.h icp_condition on the sequence's staged sums and
// lie.h map_icp_verdict_joint; then the joint record. Also here: icp_condition_kernel (vors_icp_condition), one thread per system.
static_assert(sizeof(vors_map_icp_joint_record) == 20, "vors_map_icp_joint_record is 20 bytes");
static_assert(VORS_MAP_ICP_CONDITION == MAP_ICP_CONDITION, "lie.h map_icp_verdict_joint returns the header's value");

__global__ void map_icp_arm_joint_kernel(MapIcpJointCall j) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= j.c.n) return;
    j.joint_records[seq] = vors_map_icp_joint_record{};
}

__global__ void map_icp_apply_joint_kernel(MapIcpJointCall j) {
    const MapIcpCall& c = j.c;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= min(max(*c.promo_count, 0), c.n)) return;
    const int seq = c.promo_list[k];
    if (seq < 0 || seq >= c.n) return;
    vors_map_icp_record& r = c.records[seq];
    const vors_icp_stats st = c.stats[seq];
    float after[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) after[i] = c.result_poses[(size_t)seq * 7 + i];
    float sums[29];
#pragma unroll
    for (int q = 0; q < 29; ++q) sums[q] = j.sums29[(size_t)seq * 29 + q];
    vors_map_icp_joint_record jr{};
    jr.condition_flags = icp_condition(sums, &jr.dilution_t, &jr.dilution_r);
    const uint32_t v = map_icp_verdict_joint(c.gates, j.condition, st.status, st.matched, st.considered, st.rms, r.pose_before, after, jr.dilution_t,
                                             jr.dilution_r);
    r.verdict = v;
    r.stats = st;
#pragma unroll
    for (int g = 0; g < VORS_ICP_GATE_COUNTS; ++g) r.gate_counts[g] = c.gate_counts[(size_t)seq * VORS_ICP_GATE_COUNTS + g];
#pragma unroll
    for (int i = 0; i < 7; ++i) r.pose_after[i] = after[i];
#pragma unroll
    for (int q = 0; q < VORS_ICP_PHOTO_COUNTS; ++q) jr.photo_counts[q] = j.photo_counts[(size_t)seq * VORS_ICP_PHOTO_COUNTS + q];
    j.joint_records[seq] = jr;
    c.totals[2 * seq] += 1u;
    if (v == (uint32_t)MAP_ICP_ACCEPTED) {
        c.totals[2 * seq + 1] += 1u;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            c.kf_poses[(size_t)seq * 7 + i] = after[i];
            c.cur_poses[(size_t)seq * 7 + i] = after[i];
            c.out_poses[(size_t)seq * 7 + i] = after[i];
        }
    }
}

// 29 sums -> dilutions and flags (lie.h icp_condition), one thread per system
__global__ __launch_bounds__(64) void icp_condition_kernel(const float* __restrict__ sums29, int n, float* __restrict__ dilution2,
                                                           int32_t* __restrict__ flags) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    float sums[29];
#pragma unroll
    for (int q = 0; q < 29; ++q) sums[q] = sums29[(size_t)p * 29 + q];
    float dt, dr;
    const int fl = icp_condition(sums, &dt, &dr);
    dilution2[(size_t)p * 2] = dt;
    dilution2[(size_t)p * 2 + 1] = dr;
    if (flags) flags[p] = fl;
}

struct MapIcpNormalArgs {
    int seq0;
    NormalCall c;
};

__global__ __launch_bounds__(NORMAL_BLOCK) void map_icp_frame_normals_kernel(MapIcpNormalArgs a) {
    const NormalCall& c = a.c;
    int seq = a.seq0 + blockIdx.y;
    if (seq >= *c.sel_count) return;  // the whole workgroup (select_pair's rule)
    seq = c.sel_list[seq];
    if (seq < 0 || seq >= c.n) return;
    const int plane = c.rows * c.cols;
    const uint16_t* depth = c.depth + (size_t)seq * (size_t)plane;
    float* normals = c.normals + (size_t)seq * (size_t)plane * 3;
    uint32_t cnt[VORS_NORMAL_COUNTS] = {0u, 0u, 0u};  // (not kept)
    normals_narrow_trip(c, depth, normals, plane, blockIdx.x * (NORMAL_BLOCK * NORMAL_POINTS), false, iso_identity(), cnt);
}

void launch_map_icp_arm(const MapIcpCall& c, hipStream_t s) {
    hipLaunchKernelGGL(map_icp_arm_kernel, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, s, c);
}

void launch_map_icp_apply(const MapIcpCall& c, hipStream_t s) {
    hipLaunchKernelGGL(map_icp_apply_kernel, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, s, c);
}

void launch_map_icp_arm_joint(const MapIcpJointCall& j, hipStream_t s) {
    hipLaunchKernelGGL(map_icp_arm_joint_kernel, dim3((unsigned)((j.c.n + 255) / 256)), dim3(256), 0, s, j);
}

void launch_map_icp_apply_joint(const MapIcpJointCall& j, hipStream_t s) {
    hipLaunchKernelGGL(map_icp_apply_joint_kernel, dim3((unsigned)((j.c.n + 255) / 256)), dim3(256), 0, s, j);
}

void launch_icp_condition(const float* sums29, int n, float* dilution2, int32_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(icp_condition_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, sums29, n, dilution2, flags);
}

void launch_map_icp_frame_normals(const NormalCall& c, hipStream_t s) {
    const size_t plane = (size_t)c.rows * (size_t)c.cols;
    MapIcpNormalArgs a{0, c};
    const unsigned blocks = (unsigned)((plane + NORMAL_BLOCK * NORMAL_POINTS - 1) / (NORMAL_BLOCK * NORMAL_POINTS));
    for_pair_slices(c.n, [&](int seq0, int ns) {
        a.seq0 = seq0;
        hipLaunchKernelGGL(map_icp_frame_normals_kernel, dim3(blocks, ns), dim3(NORMAL_BLOCK), 0, s, a);
    });
}

}  // namespace vors
