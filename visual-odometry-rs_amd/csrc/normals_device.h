// Device text shared by normal_kernels.hip (depth_normals_kernel) and map_icp_kernels.hip (map_icp_frame_normals_kernel).
#pragma once
#include "device_common.h"

namespace vors {

// The narrow trip of the plane form of the normals pass: a thread takes four pixels a workgroup width apart from `base` on — five u16
// taps each, all loads issued before the first use, then per pixel lie.h depth_normal, the three counters and three dword stores at
// consecutive addresses (normals null: no stores). A lane past the end of the plane reads pixel 0, a safe address, and does nothing more.
__device__ __forceinline__ void normals_narrow_trip(const NormalCall& c, const uint16_t* depth, float* normals, int plane, int base, bool has_pose,
                                                    const Iso& pose, uint32_t (&cnt)[VORS_NORMAL_COUNTS]) {
    int xs[NORMAL_POINTS], ys[NORMAL_POINTS];
    uint16_t d[NORMAL_POINTS][5];
    bool valid[NORMAL_POINTS];
#pragma unroll
    for (int j = 0; j < NORMAL_POINTS; ++j) {
        const int i = base + j * NORMAL_BLOCK + (int)threadIdx.x;
        valid[j] = i < plane;
        const int q = valid[j] ? i : 0;
        ys[j] = q / c.cols;
        xs[j] = q - ys[j] * c.cols;
        const NormalTaps t = depth_normal_taps(xs[j], ys[j], c.cols, c.rows, c.step);
        d[j][0] = depth[t.c];
        d[j][1] = depth[t.l];
        d[j][2] = depth[t.r];
        d[j][3] = depth[t.u];
        d[j][4] = depth[t.d];
    }
#pragma unroll
    for (int j = 0; j < NORMAL_POINTS; ++j) {
        if (!valid[j]) continue;
        const int i = base + j * NORMAL_BLOCK + (int)threadIdx.x;
        const DepthNormal o = depth_normal(c.k, c.depth_scale, c.step, c.jump_m, xs[j], ys[j], c.cols, c.rows, d[j][0], d[j][1], d[j][2], d[j][3],
                                           d[j][4], has_pose, pose);
        cnt[0] += 1u;
        cnt[1] += o.has_depth ? 1u : 0u;
        cnt[2] += o.has_normal ? 1u : 0u;
        if (normals) {
            float* out = normals + 3 * (size_t)i;
            out[0] = o.n.x;
            out[1] = o.n.y;
            out[2] = o.n.z;
        }
    }
}

}  // namespace vors
