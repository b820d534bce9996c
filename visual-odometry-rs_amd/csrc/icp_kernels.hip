// vors_icp_points / vors_trackers_icp_map: projective point-to-plane ICP of world-frame point lists with normals against level-0 depth
// planes. Handle-free: no Geom, no records; the per-point rule is lie.h icp_landing / icp_row / icp_products, the round's
// verdict lie.h icp_round, the order of the sums the one lie.h states — the texts vors_icp_points_host runs, bit for bit.
// BEGIN  (icp_begin_kernel): one thread per list copies the start pose into the state in the workspace; from then on the input poses are
//        not read again, so the output poses may alias them.
// EVAL   (icp_eval_kernel): grid = (chunks of the list) x lists, sized from the capacity and capped at ICP_MAX_CHUNKS; a workgroup beyond
//        the clipped range's chunks returns at once, a longer range goes through the stride loop (render_splat_kernel's scheme), and so
//        does every workgroup of a frozen list unless the launch is the final one. A trip is one chunk of 1024 ranks: a thread takes the
//        slots t, t + 256, t + 512, t + 768 — consecutive lanes read consecutive 12-byte rows of points and normals, all loads issued
//        before the first use, then the four depth gathers before the rows. The halving tree: w = 512 and 256 in the thread, (p0 + p2) +
//        (p1 + p3), into ONE set of 28 accumulators (the four rows of seven are what stays live, not four sets of products); w = 128 and
//        64 across the four wavefronts through LDS, [product][lane] so that lanes hit consecutive banks; w = 32..1 inside wavefront 0 by
//        __shfl_down, v[s] + v[s + w]. Lane 0 stores the chunk's 28 sums and its matched count: stored, not accumulated — the
//        workspace needs no clearing and no floating-point atomic exists. No workgroup waits for another.
// SOLVE  (icp_solve_kernel): one wavefront per list. Lanes 0..27 own one sum each and add the chunk partials in ascending order from
//        chunk 0's, eight loads issued ahead of the eight dependent adds; lanes 32..63 add the integer counts. Every lane then holds all
//        28 sums (__shfl) and runs the verdict; lane 0 stores. The final launch writes the outputs instead.
// vors_icp_points_robust / vors_trackers_icp_map_robust run the same launches with icp_eval_robust_kernel in EVAL's place:
// lie.h icp_row_robust / icp_products_robust, a gather of the frame normal beside the depth's, and the gate counts of the final evaluation.
// vors_icp_points_joint / vors_trackers_icp_map_joint run them with icp_eval_joint_kernel there: a photometric row per
// matched point beside the geometric one (lie.h icp_photo_footprint / icp_row_photo), the list's grey byte and four gathered taps of the
// frame's grey plane, and the photo counts of the final evaluation.
#include "device_common.h"

namespace vors {

struct IcpEvalArgs {
    int seq0;
    IcpCall c;
};

__device__ __forceinline__ void icp_list_range(const IcpCall& c, int seq, uint32_t* first, uint32_t* last) {
    const uint32_t* r = c.ranges ? reinterpret_cast<const uint32_t*>(c.ranges + (size_t)seq * (size_t)c.range_stride) : nullptr;
    icp_range(c.list_counts[seq], c.capacity, r, first, last);
}

__global__ void icp_begin_kernel(IcpCall c) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= c.n) return;
    const float* p = c.poses_in + (size_t)seq * (size_t)c.pose_stride;
    IcpState& st = c.state[seq];
#pragma unroll
    for (int i = 0; i < 7; ++i) st.pose[i] = p[i];
    st.status = ICP_ITERATIONS;
    st.iterations = 0u;
    st.frozen = 0u;
    st.last_step_norm = 0.0f;
    st.pad = 0u;
}

template <bool FINAL, bool RESID>
__global__ __launch_bounds__(ICP_BLOCK) void icp_eval_kernel(IcpEvalArgs a) {
    __shared__ float lds[VORS_ICP_SUMS * 128];
    __shared__ uint32_t lds_counts[ICP_BLOCK / 64];
    const IcpCall& c = a.c;
    const int seq = a.seq0 + blockIdx.y;
    const IcpState& st = c.state[seq];
    if (!FINAL && st.frozen) return;  // the whole workgroup
    uint32_t first, last;
    icp_list_range(c, seq, &first, &last);
    // (last - first <= capacity < 2^31: nothing below wraps)
    const uint32_t nchunks = (last - first + (VORS_ICP_CHUNK - 1)) / VORS_ICP_CHUNK;
    if (blockIdx.x >= nchunks) return;  // the whole workgroup
    const size_t cap_chunks = icp_chunks(c.capacity);
    const float* xyz = c.xyz + (size_t)seq * (size_t)c.capacity * 3;
    const float* normals = c.normals + (size_t)seq * (size_t)c.capacity * 3;
    const uint16_t* depth = c.depth + (size_t)seq * (size_t)c.rows * (size_t)c.cols;
    const Iso pose = iso_load(st.pose);
    const unsigned t = threadIdx.x, wave = t >> 6;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint32_t base = first + chunk * VORS_ICP_CHUNK;
        V3 w[4], nw[4];
        bool valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t rank = base + j * ICP_BLOCK + t;
            valid[j] = rank < last;
            const size_t o = 3 * (size_t)(valid[j] ? rank : base);  // (a slot beyond the range reads the chunk's first row: a safe address)
            w[j] = V3{xyz[o], xyz[o + 1], xyz[o + 2]};
            nw[j] = V3{normals[o], normals[o + 1], normals[o + 2]};
        }
        IcpLanding l[4];
        uint16_t d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            l[j] = icp_landing(c.k, pose, w[j], c.cols, c.rows);
            l[j].lands = l[j].lands && valid[j];
            d[j] = depth[l[j].lands ? l[j].y * c.cols + l[j].x : 0];  // (no landing: pixel 0, a safe address; icp_row ignores it)
        }
        float row[4][7];
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool m = icp_row(c.k, c.depth_scale, c.dist_m, pose, l[j], nw[j], d[j], row[j]);
            cnt += m ? 1u : 0u;
            if constexpr (RESID)
                if (valid[j]) c.residuals[(size_t)seq * (size_t)c.capacity + (base + j * ICP_BLOCK + t)] = m ? row[j][0] : __builtin_nanf("");
        }
        // w = 512, 256: (slot t + slot t + 512) + (slot t + 256 + slot t + 768)
        float acc[VORS_ICP_SUMS], p[VORS_ICP_SUMS], q[VORS_ICP_SUMS];
        icp_products(row[0], p);
        icp_products(row[2], q);
#pragma unroll
        for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = p[k] + q[k];
        icp_products(row[1], p);
        icp_products(row[3], q);
#pragma unroll
        for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + (p[k] + q[k]);
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, sh);
        if ((t & 63) == 0) lds_counts[wave] = cnt;
        // w = 128: threads 128..255 hand over
        if (wave >= 2) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) lds[k * 128 + (t - 128)] = acc[k];
        }
        __syncthreads();
        if (wave < 2) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + lds[k * 128 + t];
        }
        __syncthreads();
        // w = 64: threads 64..127 hand over
        if (wave == 1) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) lds[k * 128 + (t - 64)] = acc[k];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + lds[k * 128 + t];
            // w = 32..1: lane s takes lane s + w's (lanes >= w compute values nobody reads)
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) {
#pragma unroll
                for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + __shfl_down(acc[k], sh);
            }
            if (t == 0) {
                float* out = c.partials + ((size_t)seq * cap_chunks + chunk) * VORS_ICP_SUMS;
#pragma unroll
                for (int k = 0; k < VORS_ICP_SUMS; ++k) out[k] = acc[k];
                c.chunk_counts[(size_t)seq * cap_chunks + chunk] = (lds_counts[0] + lds_counts[1]) + (lds_counts[2] + lds_counts[3]);
            }
        }
        __syncthreads();  // (the next trip writes the LDS again)
    }
}

struct IcpRobustEvalArgs {
    int seq0;
    IcpCall c;
    IcpRobust r;
};

// The evaluation of the robust pass (vors_icp_points_robust): icp_eval_kernel's trip, grid, tree and stores with the rule
// lie.h icp_row_robust<NORMALS> / icp_products_robust<HUBER>. A kernel of its own text, not a shared body: with one, the compiler
// scheduled the plain kernels differently, and their code is to stay what it was. The frame normal of a point is gathered together with
// its depth — 12 bytes at the landing pixel, pixel 0 without a landing — ahead of the rows that consume it, not behind the distance
// gate. Gate counts (FINAL, when asked for): a thread counts over its trips; after the last one the workgroup reduces across its
// wavefronts and adds once per counter with an integer atomic. A workgroup without a chunk adds nothing.
template <bool FINAL, bool RESID, bool NORMALS, bool HUBER>
__global__ __launch_bounds__(ICP_BLOCK) void icp_eval_robust_kernel(IcpRobustEvalArgs a) {
    __shared__ float lds[VORS_ICP_SUMS * 128];
    __shared__ uint32_t lds_counts[ICP_BLOCK / 64];
    __shared__ uint32_t lds_gates[VORS_ICP_GATE_COUNTS * (ICP_BLOCK / 64)];
    const IcpCall& c = a.c;
    const IcpRobust& rb = a.r;
    const int seq = a.seq0 + blockIdx.y;
    const IcpState& st = c.state[seq];
    if (!FINAL && st.frozen) return;  // the whole workgroup
    uint32_t first, last;
    icp_list_range(c, seq, &first, &last);
    // (last - first <= capacity < 2^31: nothing below wraps)
    const uint32_t nchunks = (last - first + (VORS_ICP_CHUNK - 1)) / VORS_ICP_CHUNK;
    if (blockIdx.x >= nchunks) return;  // the whole workgroup
    const size_t cap_chunks = icp_chunks(c.capacity);
    const float* xyz = c.xyz + (size_t)seq * (size_t)c.capacity * 3;
    const float* normals = c.normals + (size_t)seq * (size_t)c.capacity * 3;
    const uint16_t* depth = c.depth + (size_t)seq * (size_t)c.rows * (size_t)c.cols;
    const Iso pose = iso_load(st.pose);
    const unsigned t = threadIdx.x, wave = t >> 6;
    const float* frame_normals = nullptr;
    if constexpr (NORMALS) frame_normals = rb.frame_normals + (size_t)seq * (size_t)c.rows * (size_t)c.cols * 3;
    uint32_t gates[VORS_ICP_GATE_COUNTS] = {0u, 0u, 0u, 0u};
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint32_t base = first + chunk * VORS_ICP_CHUNK;
        V3 w[4], nw[4];
        bool valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t rank = base + j * ICP_BLOCK + t;
            valid[j] = rank < last;
            const size_t o = 3 * (size_t)(valid[j] ? rank : base);  // (a slot beyond the range reads the chunk's first row: a safe address)
            w[j] = V3{xyz[o], xyz[o + 1], xyz[o + 2]};
            nw[j] = V3{normals[o], normals[o + 1], normals[o + 2]};
        }
        IcpLanding l[4];
        uint16_t d[4];
        V3 nf[4] = {};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            l[j] = icp_landing(c.k, pose, w[j], c.cols, c.rows);
            l[j].lands = l[j].lands && valid[j];
            const int pixel = l[j].lands ? l[j].y * c.cols + l[j].x : 0;  // (no landing: pixel 0, a safe address; the row ignores it)
            d[j] = depth[pixel];
            if constexpr (NORMALS) {
                const float* f = frame_normals + 3 * (size_t)pixel;
                nf[j] = V3{f[0], f[1], f[2]};
            }
        }
        float row[4][7];
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const IcpGate g = icp_row_robust<NORMALS>(c.k, c.depth_scale, c.dist_m, rb.min_cos, pose, l[j], nw[j], d[j], nf[j], row[j]);
            const bool m = g == ICP_GATE_MATCHED;
            if constexpr (FINAL) {
                gates[0] += g >= ICP_GATE_DEPTH ? 1u : 0u;
                gates[1] += g >= ICP_GATE_DIST ? 1u : 0u;
                gates[2] += m ? 1u : 0u;
            }
            cnt += m ? 1u : 0u;
            if constexpr (RESID)
                if (valid[j]) c.residuals[(size_t)seq * (size_t)c.capacity + (base + j * ICP_BLOCK + t)] = m ? row[j][0] : __builtin_nanf("");
        }
        // w = 512, 256: (slot t + slot t + 512) + (slot t + 256 + slot t + 768)
        float acc[VORS_ICP_SUMS], p[VORS_ICP_SUMS], q[VORS_ICP_SUMS];
        // (a row's products; the final evaluation counts the points that lie on Huber's linear branch)
        auto products = [&](const float* r7, float* o) {
            const bool linear = icp_products_robust<HUBER>(r7, rb.huber_m, o);
            if constexpr (FINAL && HUBER) gates[3] += linear ? 1u : 0u;
        };
        products(row[0], p);
        products(row[2], q);
#pragma unroll
        for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = p[k] + q[k];
        products(row[1], p);
        products(row[3], q);
#pragma unroll
        for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + (p[k] + q[k]);
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, sh);
        if ((t & 63) == 0) lds_counts[wave] = cnt;
        // w = 128: threads 128..255 hand over
        if (wave >= 2) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) lds[k * 128 + (t - 128)] = acc[k];
        }
        __syncthreads();
        if (wave < 2) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + lds[k * 128 + t];
        }
        __syncthreads();
        // w = 64: threads 64..127 hand over
        if (wave == 1) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) lds[k * 128 + (t - 64)] = acc[k];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + lds[k * 128 + t];
            // w = 32..1: lane s takes lane s + w's (lanes >= w compute values nobody reads)
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) {
#pragma unroll
                for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + __shfl_down(acc[k], sh);
            }
            if (t == 0) {
                float* out = c.partials + ((size_t)seq * cap_chunks + chunk) * VORS_ICP_SUMS;
#pragma unroll
                for (int k = 0; k < VORS_ICP_SUMS; ++k) out[k] = acc[k];
                c.chunk_counts[(size_t)seq * cap_chunks + chunk] = (lds_counts[0] + lds_counts[1]) + (lds_counts[2] + lds_counts[3]);
            }
        }
        __syncthreads();  // (the next trip writes the LDS again)
    }
    if constexpr (FINAL) {
        if (!rb.gate_counts) return;  // the whole workgroup
#pragma unroll
        for (int g = 0; g < VORS_ICP_GATE_COUNTS; ++g) {
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) gates[g] += (uint32_t)__shfl_xor((int)gates[g], sh);
            if ((t & 63) == 0) lds_gates[g * (ICP_BLOCK / 64) + wave] = gates[g];
        }
        __syncthreads();
        if (t < VORS_ICP_GATE_COUNTS) {
            const uint32_t* v = lds_gates + t * (ICP_BLOCK / 64);
            atomicAdd(rb.gate_counts + (size_t)seq * VORS_ICP_GATE_COUNTS + t, (v[0] + v[1]) + (v[2] + v[3]));
        }
    }
}

struct IcpJointEvalArgs {
    int seq0;
    IcpCall c;
    IcpRobust r;
    IcpJoint j;
};

// The evaluation of the joint pass (vors_icp_points_joint): icp_eval_robust_kernel's trip, grid, tree and stores, and for
// every matched point whose bilinear footprint lies inside the frame's grey plane a photometric row beside the geometric one (lie.h
// icp_photo_footprint / icp_row_photo), its products under icp_products_robust<PHUBER> added to the point's own before the tree. A text
// of its own for the reason given above the robust kernel. The grey byte of a point is loaded with its row of the list; the four taps —
// two 2-byte loads, rows y0 and y0 + 1, offset 0 without a footprint inside — are gathered with the depth and the frame normal, ahead
// of the rows. photo_scale_m == 0 (or a plane of fewer than two rows or columns, where no footprint fits): workgroup-uniform, no grey
// pointer is read and no point is PHOTO — the robust pass. Photo counts (FINAL, when asked for): as the gate counts.
template <bool FINAL, bool RESID, bool NORMALS, bool HUBER, bool PHUBER>
__global__ __launch_bounds__(ICP_BLOCK) void icp_eval_joint_kernel(IcpJointEvalArgs a) {
    constexpr int COUNTERS = VORS_ICP_GATE_COUNTS + ICP_PHOTO_COUNTS;
    __shared__ float lds[VORS_ICP_SUMS * 128];
    __shared__ uint32_t lds_counts[ICP_BLOCK / 64];
    __shared__ uint32_t lds_gates[COUNTERS * (ICP_BLOCK / 64)];
    const IcpCall& c = a.c;
    const IcpRobust& rb = a.r;
    const IcpJoint& jt = a.j;
    const int seq = a.seq0 + blockIdx.y;
    const IcpState& st = c.state[seq];
    if (!FINAL && st.frozen) return;  // the whole workgroup
    uint32_t first, last;
    icp_list_range(c, seq, &first, &last);
    // (last - first <= capacity < 2^31: nothing below wraps)
    const uint32_t nchunks = (last - first + (VORS_ICP_CHUNK - 1)) / VORS_ICP_CHUNK;
    if (blockIdx.x >= nchunks) return;  // the whole workgroup
    const size_t cap_chunks = icp_chunks(c.capacity);
    const float* xyz = c.xyz + (size_t)seq * (size_t)c.capacity * 3;
    const float* normals = c.normals + (size_t)seq * (size_t)c.capacity * 3;
    const uint16_t* depth = c.depth + (size_t)seq * (size_t)c.rows * (size_t)c.cols;
    const Iso pose = iso_load(st.pose);
    const unsigned t = threadIdx.x, wave = t >> 6;
    const float* frame_normals = nullptr;
    if constexpr (NORMALS) frame_normals = rb.frame_normals + (size_t)seq * (size_t)c.rows * (size_t)c.cols * 3;
    const bool photo_on = jt.photo_scale_m > 0.0f && c.rows >= 2 && c.cols >= 2;  // (uniform)
    const uint8_t* list_gray = photo_on ? jt.list_gray + (size_t)seq * (size_t)c.capacity : nullptr;
    const uint8_t* frame_gray = photo_on ? jt.frame_gray + (size_t)seq * (size_t)c.rows * (size_t)c.cols : nullptr;
    uint32_t gates[COUNTERS] = {0u, 0u, 0u, 0u, 0u, 0u};  // the four gate counts, then photo_used, photo_huber_linear
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const uint32_t base = first + chunk * VORS_ICP_CHUNK;
        V3 w[4], nw[4];
        uint8_t gw[4] = {0, 0, 0, 0};
        bool valid[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t rank = base + j * ICP_BLOCK + t;
            valid[j] = rank < last;
            const size_t r = (size_t)(valid[j] ? rank : base);  // (a slot beyond the range reads the chunk's first row: a safe address)
            const size_t o = 3 * r;
            w[j] = V3{xyz[o], xyz[o + 1], xyz[o + 2]};
            nw[j] = V3{normals[o], normals[o + 1], normals[o + 2]};
            if (photo_on) gw[j] = list_gray[r];
        }
        IcpLanding l[4];
        IcpFootprint fp[4];
        uint16_t d[4], top[4] = {0, 0, 0, 0}, bot[4] = {0, 0, 0, 0};
        V3 nf[4] = {};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            l[j] = icp_landing(c.k, pose, w[j], c.cols, c.rows);
            l[j].lands = l[j].lands && valid[j];
            const int pixel = l[j].lands ? l[j].y * c.cols + l[j].x : 0;  // (no landing: pixel 0, a safe address; the row ignores it)
            d[j] = depth[pixel];
            if constexpr (NORMALS) {
                const float* f = frame_normals + 3 * (size_t)pixel;
                nf[j] = V3{f[0], f[1], f[2]};
            }
            fp[j] = icp_photo_footprint(c.k, l[j].c, c.cols, c.rows);
            if (photo_on) {
                // (no footprint inside: offset 0 — bytes 0, 1, cols, cols + 1 exist in a plane of two rows and two columns)
                const uint8_t* g = frame_gray + (unsigned)fp[j].off;
                __builtin_memcpy(&top[j], g, 2);  // two adjacent bytes per row: one (possibly unaligned) 16-bit load each
                __builtin_memcpy(&bot[j], g + (unsigned)c.cols, 2);
            }
        }
        float row[4][7], prow[4][7];
        bool photo[4];
        uint32_t cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const IcpGate g = icp_row_robust<NORMALS>(c.k, c.depth_scale, c.dist_m, rb.min_cos, pose, l[j], nw[j], d[j], nf[j], row[j]);
            const bool m = g == ICP_GATE_MATCHED;
            photo[j] = m && photo_on && fp[j].inside;
            const float dg = icp_row_photo(c.k, jt.photo_scale_m, l[j].c, fp[j], photo[j], (uint8_t)(top[j] & 0xff), (uint8_t)(top[j] >> 8),
                                           (uint8_t)(bot[j] & 0xff), (uint8_t)(bot[j] >> 8), gw[j], prow[j]);
            if constexpr (FINAL) {
                gates[0] += g >= ICP_GATE_DEPTH ? 1u : 0u;
                gates[1] += g >= ICP_GATE_DIST ? 1u : 0u;
                gates[2] += m ? 1u : 0u;
                gates[4] += photo[j] ? 1u : 0u;
            }
            cnt += m ? 1u : 0u;
            if constexpr (RESID)
                if (valid[j]) {
                    const size_t o = (size_t)seq * (size_t)c.capacity + (base + j * ICP_BLOCK + t);
                    if (c.residuals) c.residuals[o] = m ? row[j][0] : __builtin_nanf("");
                    if (jt.photo_residuals) jt.photo_residuals[o] = photo[j] ? dg : __builtin_nanf("");
                }
        }
        // w = 512, 256: (slot t + slot t + 512) + (slot t + 256 + slot t + 768)
        float acc[VORS_ICP_SUMS], p[VORS_ICP_SUMS], q[VORS_ICP_SUMS];
        // (a point's products: the geometric row's, and for a PHOTO point the photometric row's added to them; the final evaluation
        // counts the points that lie on either Huber's linear branch)
        auto products = [&](int j, float* o) {
            const bool linear = icp_products_robust<HUBER>(row[j], rb.huber_m, o);
            if constexpr (FINAL && HUBER) gates[3] += linear ? 1u : 0u;
            if (photo[j]) {
                float pp[VORS_ICP_SUMS];
                const bool plinear = icp_products_robust<PHUBER>(prow[j], jt.photo_huber_m, pp);
                if constexpr (FINAL && PHUBER) gates[5] += plinear ? 1u : 0u;
#pragma unroll
                for (int k = 0; k < VORS_ICP_SUMS; ++k) o[k] = o[k] + pp[k];
            }
        };
        products(0, p);
        products(2, q);
#pragma unroll
        for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = p[k] + q[k];
        products(1, p);
        products(3, q);
#pragma unroll
        for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + (p[k] + q[k]);
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, sh);
        if ((t & 63) == 0) lds_counts[wave] = cnt;
        // w = 128: threads 128..255 hand over
        if (wave >= 2) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) lds[k * 128 + (t - 128)] = acc[k];
        }
        __syncthreads();
        if (wave < 2) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + lds[k * 128 + t];
        }
        __syncthreads();
        // w = 64: threads 64..127 hand over
        if (wave == 1) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) lds[k * 128 + (t - 64)] = acc[k];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + lds[k * 128 + t];
            // w = 32..1: lane s takes lane s + w's (lanes >= w compute values nobody reads)
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) {
#pragma unroll
                for (int k = 0; k < VORS_ICP_SUMS; ++k) acc[k] = acc[k] + __shfl_down(acc[k], sh);
            }
            if (t == 0) {
                float* out = c.partials + ((size_t)seq * cap_chunks + chunk) * VORS_ICP_SUMS;
#pragma unroll
                for (int k = 0; k < VORS_ICP_SUMS; ++k) out[k] = acc[k];
                c.chunk_counts[(size_t)seq * cap_chunks + chunk] = (lds_counts[0] + lds_counts[1]) + (lds_counts[2] + lds_counts[3]);
            }
        }
        __syncthreads();  // (the next trip writes the LDS again)
    }
    if constexpr (FINAL) {
        if (!rb.gate_counts && !jt.photo_counts) return;  // the whole workgroup
#pragma unroll
        for (int g = 0; g < COUNTERS; ++g) {
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) gates[g] += (uint32_t)__shfl_xor((int)gates[g], sh);
            if ((t & 63) == 0) lds_gates[g * (ICP_BLOCK / 64) + wave] = gates[g];
        }
        __syncthreads();
        if (t < COUNTERS) {
            const uint32_t* v = lds_gates + t * (ICP_BLOCK / 64);
            const uint32_t sum = (v[0] + v[1]) + (v[2] + v[3]);
            if (t < VORS_ICP_GATE_COUNTS) {
                if (rb.gate_counts) atomicAdd(rb.gate_counts + (size_t)seq * VORS_ICP_GATE_COUNTS + t, sum);
            } else if (jt.photo_counts) {
                atomicAdd(jt.photo_counts + (size_t)seq * ICP_PHOTO_COUNTS + (t - VORS_ICP_GATE_COUNTS), sum);
            }
        }
    }
}

template <bool FINAL>
__global__ __launch_bounds__(64) void icp_solve_kernel(IcpCall c) {
    const int seq = blockIdx.x;
    const unsigned lane = threadIdx.x;
    IcpState& st = c.state[seq];
    if (!FINAL && st.frozen) return;  // the whole wavefront
    uint32_t first, last;
    icp_list_range(c, seq, &first, &last);
    const uint32_t nchunks = (last - first + (VORS_ICP_CHUNK - 1)) / VORS_ICP_CHUNK;
    const size_t cap_chunks = icp_chunks(c.capacity);
    const float* part = c.partials + (size_t)seq * cap_chunks * VORS_ICP_SUMS;
    const uint32_t* counts = c.chunk_counts + (size_t)seq * cap_chunks;
    float sum = 0.0f;
    uint32_t matched = 0;
    if (lane < VORS_ICP_SUMS) {
        if (nchunks > 0) sum = part[lane];
        uint32_t ch = 1;
        for (; ch + 8 <= nchunks; ch += 8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(ch + i) * VORS_ICP_SUMS + lane];
#pragma unroll
            for (int i = 0; i < 8; ++i) sum = sum + v[i];
        }
        for (; ch < nchunks; ++ch) sum = sum + part[(size_t)ch * VORS_ICP_SUMS + lane];
    } else if (lane >= 32) {
        for (uint32_t ch = lane - 32; ch < nchunks; ch += 32) matched += counts[ch];
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) matched += (uint32_t)__shfl_xor((int)matched, sh);
    float sums[VORS_ICP_SUMS];
#pragma unroll
    for (int k = 0; k < VORS_ICP_SUMS; ++k) sums[k] = __shfl(sum, k);
    if constexpr (!FINAL) {
        Iso pose = iso_load(st.pose);
        float step_norm = 0.0f;
        const IcpStatus v = icp_round(sums, matched, c.min_points, c.damping, c.step_eps, &pose, &step_norm);
        if (lane == 0) {
            if (v == ICP_ITERATIONS || v == ICP_CONVERGED) {
                iso_store(pose, st.pose);
                st.iterations += 1u;
                st.last_step_norm = step_norm;
            }
            if (v != ICP_ITERATIONS) {
                st.status = (uint32_t)v;
                st.frozen = 1u;
            }
        }
    } else {
        if (lane < 7) c.poses_out[(size_t)seq * 7 + lane] = st.pose[lane];
        if (lane == 0 && c.stats) {
            vors_icp_stats o;
            o.status = st.status;
            o.iterations = st.iterations;
            o.considered = last - first;
            o.matched = matched;
            o.rms = sqrtf(sums[0] / (float)matched);
            o.last_step_norm = st.last_step_norm;
            c.stats[seq] = o;
        }
        if (lane == 0 && c.sums29) icp_sums29(sums, matched, c.sums29 + (size_t)seq * 29);
    }
}

void launch_icp_points(const IcpCall& c, const IcpRobust* robust, hipStream_t s, const IcpJoint* joint) {
    if (robust && robust->gate_counts) (void)hipMemsetAsync(robust->gate_counts, 0, (size_t)c.n * VORS_ICP_GATE_COUNTS * sizeof(uint32_t), s);
    if (joint && joint->photo_counts) (void)hipMemsetAsync(joint->photo_counts, 0, (size_t)c.n * ICP_PHOTO_COUNTS * sizeof(uint32_t), s);
    hipLaunchKernelGGL(icp_begin_kernel, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, s, c);
    const size_t want = icp_chunks(c.capacity);
    const unsigned chunks = (unsigned)(want > ICP_MAX_CHUNKS ? ICP_MAX_CHUNKS : want);
    IcpEvalArgs a{0, c};
    IcpRobustEvalArgs ra{0, c, robust ? *robust : IcpRobust{}};
    IcpJointEvalArgs ja{0, c, ra.r, joint ? *joint : IcpJoint{}};
    auto eval = [&](auto final_, auto resid_) {
        for_pair_slices(c.n, [&](int seq0, int ns) {
            a.seq0 = ra.seq0 = ja.seq0 = seq0;
            if (!robust) {
                hipLaunchKernelGGL((icp_eval_kernel<decltype(final_)::value, decltype(resid_)::value>), dim3(chunks, ns), dim3(ICP_BLOCK), 0, s, a);
                return;
            }
            with_bool(ra.r.frame_normals != nullptr, [&](auto nrm) {
                with_bool(ra.r.huber_m > 0.0f, [&](auto hub) {
                    if (joint) {
                        with_bool(ja.j.photo_huber_m > 0.0f, [&](auto phub) {
                            hipLaunchKernelGGL((icp_eval_joint_kernel<decltype(final_)::value, decltype(resid_)::value, decltype(nrm)::value,
                                                                      decltype(hub)::value, decltype(phub)::value>),
                                               dim3(chunks, ns), dim3(ICP_BLOCK), 0, s, ja);
                        });
                        return;
                    }
                    hipLaunchKernelGGL((icp_eval_robust_kernel<decltype(final_)::value, decltype(resid_)::value, decltype(nrm)::value, decltype(hub)::value>),
                                       dim3(chunks, ns), dim3(ICP_BLOCK), 0, s, ra);
                });
            });
        });
    };
    for (int it = 0; it < c.iters; ++it) {
        eval(std::false_type{}, std::false_type{});
        hipLaunchKernelGGL(icp_solve_kernel<false>, dim3((unsigned)c.n), dim3(64), 0, s, c);
    }
    with_bool(c.residuals != nullptr || (joint && joint->photo_residuals), [&](auto r) { eval(std::true_type{}, r); });
    hipLaunchKernelGGL(icp_solve_kernel<true>, dim3((unsigned)c.n), dim3(64), 0, s, c);
}

}  // namespace vors
