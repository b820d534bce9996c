// vors_pose_graph_optimize: Levenberg-Marquardt over n pose graphs side by side, the inner solve block-Jacobi preconditioned conjugate
// gradients (include/vors_hip.h 2g). Handle-free: the per-edge and per-node rules are lie.h pg_*, the texts
// vors_pose_graph_optimize_host runs, bit for bit. Every grid is (chunk, graph); a graph's state is read through its uniform address (scalar
// loads), and a workgroup of a frozen graph returns at once. No workgroup waits for another; no floating-point atomic exists.
// ONE LANE PER EDGE OR NODE, not a few lanes per block row: a node's product is 6 outputs from 6x6 blocks, 36 + 12 + 6 registers, with no
// cross-lane step at all — the sums of the definition are sequential per node, so lanes of one node could only take turns — and a
// wavefront's 64 nodes keep 64 independent chains of loads in flight. W_e is stored [edge][36] f32, 144 bytes at 16-byte alignment, read
// as nine 16-byte loads: a lane consumes every byte of the (at most three) 64-byte halves of 128-byte lines its block touches, whatever
// the order of its edges, and a wavefront on consecutive edges reads one contiguous run of 9216 bytes.
// BEGIN     per node: the poses into the workspace (the input is not read again: the output may alias it), degrees and vectors cleared.
// EDGES     per edge: valid or skipped (lie.h pg_edge_valid); integer atomics count the degrees of both ends and the valid edges.
// SCAN      one workgroup per graph: exclusive prefix sum of the degrees, the node classes and their counts, VORS_PG_TOO_FEW.
// FILL      per valid edge: a slot in both ends' lists through an integer cursor — the order inside a list depends on the schedule —
// RANK      ... and per valid edge and end, the rank of its key among its node's keys: the list in ascending edge index, whatever FILL did.
// ENERGY    per edge the residual and the energy, the chunk tree, one partial per chunk (stored, not accumulated).
// LINEARISE per valid edge W and the edge's shares of H_ii, H_jj, g_i, g_j (lie.h pg_edge_linearise).
// GATHER    per free node the sums over its list, the damped block and its factor, and the start of the solve: x = 0, r = -g, z = M^-1 r.
// CG A / B  A: p = z + beta p' for the node and, on the fly, for its neighbours (two p buffers: no workgroup reads what another writes),
//           q = A p, the partial p.q. B: alpha, x and r updated, z = M^-1 r, the partials r.z and r.r. The scalars are re-summed from
//           the chunk partials by every workgroup (uniform, f64, ascending).
// CANDIDATE per node T' = renormalize(T exp(delta)); the largest dot6(delta, delta) through an integer maximum of its bits.
// VERDICT   one thread per graph (lie.h pg_accepts / pg_lambda_after).
// FINISH    per node the output pose; one thread the stats.
#include "device_common.h"

namespace vors {

struct PgArgs {
    int g0;
    PgCall c;
};

__device__ __forceinline__ uint32_t pg_clip(uint32_t v, int capacity) { return v < (uint32_t)capacity ? v : (uint32_t)capacity; }

// The chunk tree of vors_icp_points on four slots per thread (t, t + 256, t + 512, t + 768): w = 512 and 256 in the thread, 128 and 64
// through LDS (lds: 128 values), 32..1 by __shfl_down in wavefront 0. Every thread of the workgroup calls it; thread 0 holds the sum.
template <class T>
__device__ __forceinline__ T pg_block_tree(T a0, T a1, T a2, T a3, T* lds) {
    const unsigned t = threadIdx.x, wave = t >> 6;
    T acc = (a0 + a2) + (a1 + a3);
    if (wave >= 2) lds[t - 128] = acc;
    __syncthreads();
    if (wave < 2) acc = acc + lds[t];
    __syncthreads();
    if (wave == 1) lds[t - 64] = acc;
    __syncthreads();
    if (wave == 0) {
        acc = acc + lds[t];
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) acc = acc + __shfl_down(acc, sh);
    }
    __syncthreads();  // (the next trip writes the LDS again)
    return acc;
}

// chunk sums in ascending order from chunk 0's (uniform: scalar loads)
template <class T>
__device__ __forceinline__ T pg_sum_chunks(const T* part, uint32_t nchunks) {
    T s = nchunks > 0 ? part[0] : (T)0;
    for (uint32_t ch = 1; ch < nchunks; ++ch) s = s + part[ch];
    return s;
}

__device__ __forceinline__ void pg_load6(const float* p, float v[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = p[k];
}
__device__ __forceinline__ void pg_store6(float* p, const float v[6]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = v[k];
}

// slots of the dots array of a graph: [6][node chunks]
enum { PG_DOT_PQ = 0, PG_DOT_RZ = 1, PG_DOT_RR = 3, PG_DOT_RR0 = 5 };
__device__ __forceinline__ double* pg_dots(const PgCall& c, int g, int slot) {
    return c.dots + ((size_t)g * 6 + (size_t)slot) * pg_chunks(c.node_capacity);
}

__global__ __launch_bounds__(PG_BLOCK) void pg_begin_kernel(PgArgs a) {
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity);
    const size_t N = (size_t)c.node_capacity, nb = (size_t)g * N;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        PgState st{};
        st.status = PG_ITERATIONS;
        st.lambda = c.lambda0;
        c.state[g] = st;
    }
    for (uint32_t k = blockIdx.x * PG_BLOCK + threadIdx.x; k < nodes; k += gridDim.x * PG_BLOCK) {
        const float* p = c.poses_in + (nb + k) * (size_t)c.pose_stride;
        float* o = c.poses + ((size_t)g * 2 * N + k) * 7;
#pragma unroll
        for (int i = 0; i < 7; ++i) o[i] = p[i];
        c.deg[nb + k] = 0u;
        c.cursor[nb + k] = 0u;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            c.x[(nb + k) * 6 + i] = 0.0f;
            c.z[(nb + k) * 6 + i] = 0.0f;
            c.p[((size_t)g * 2 * N + k) * 6 + i] = 0.0f;
            c.p[((size_t)g * 2 * N + N + k) * 6 + i] = 0.0f;
        }
    }
}

__global__ __launch_bounds__(PG_BLOCK) void pg_edges_kernel(PgArgs a) {
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity), edges = pg_clip(c.edge_counts[g], c.edge_capacity);
    const size_t eb = (size_t)g * (size_t)c.edge_capacity, nb = (size_t)g * (size_t)c.node_capacity;
    // (a uniform trip count, so that every lane reaches the ballot)
    for (uint32_t base = blockIdx.x * PG_BLOCK; base < edges; base += gridDim.x * PG_BLOCK) {
        const uint32_t e = base + threadIdx.x;
        bool ok = false;
        if (e < edges) {
            const uint32_t i = c.edges[(eb + e) * 2], j = c.edges[(eb + e) * 2 + 1];
            const float w = c.weight ? c.weight[eb + e] : 1.0f;
            ok = pg_edge_valid(i, j, nodes, w, c.meas + (eb + e) * 7, c.info ? c.info + (eb + e) * 36 : nullptr);
            c.edge_ok[eb + e] = ok ? 1u : 0u;
            if (ok) {
                atomicAdd(c.deg + nb + i, 1u);
                atomicAdd(c.deg + nb + j, 1u);
            }
        }
        const unsigned long long m = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&c.state[g].valid_edges, (uint32_t)__popcll(m));
    }
}

__global__ __launch_bounds__(PG_BLOCK) void pg_scan_kernel(PgArgs a) {
    __shared__ uint32_t tile[PG_BLOCK];
    __shared__ uint32_t classes[3];
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.x;
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity), edges = pg_clip(c.edge_counts[g], c.edge_capacity);
    const size_t nb = (size_t)g * (size_t)c.node_capacity;
    uint32_t* off = c.off + (size_t)g * ((size_t)c.node_capacity + 1);
    const unsigned t = threadIdx.x;
    if (t < 3) classes[t] = 0u;
    uint32_t running = 0;
    for (uint32_t base = 0; base < nodes; base += PG_BLOCK) {
        const uint32_t k = base + t;
        const uint32_t d = k < nodes ? c.deg[nb + k] : 0u;
        tile[t] = d;
        __syncthreads();
        // inclusive Hillis-Steele scan of the tile
        for (unsigned o = 1; o < PG_BLOCK; o <<= 1) {
            const uint32_t v = t >= o ? tile[t - o] : 0u;
            __syncthreads();
            tile[t] += v;
            __syncthreads();
        }
        if (k < nodes) {
            off[k] = running + tile[t] - d;
            const bool fixed = c.fixed ? c.fixed[nb + k] != 0 : k == 0;
            const uint32_t cls = fixed ? PG_NODE_FIXED : (d == 0u ? PG_NODE_ISOLATED : PG_NODE_FREE);
            c.node_class[nb + k] = cls;
            atomicAdd(&classes[cls], 1u);
        }
        running += tile[PG_BLOCK - 1];
        __syncthreads();
    }
    __syncthreads();
    if (t == 0) {
        off[nodes] = running;
        PgState& st = c.state[g];
        st.free_nodes = classes[PG_NODE_FREE];
        st.fixed_nodes = classes[PG_NODE_FIXED];
        st.isolated_nodes = classes[PG_NODE_ISOLATED];
        st.skipped_edges = edges - st.valid_edges;
        if (st.valid_edges == 0u || classes[PG_NODE_FREE] == 0u) {
            st.status = PG_TOO_FEW;
            st.frozen = 1u;
        }
    }
}

// FILL (RANK = false) and RANK (true)
template <bool RANK>
__global__ __launch_bounds__(PG_BLOCK) void pg_incidence_kernel(PgArgs a) {
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    const uint32_t edges = pg_clip(c.edge_counts[g], c.edge_capacity);
    const size_t eb = (size_t)g * (size_t)c.edge_capacity, nb = (size_t)g * (size_t)c.node_capacity;
    const uint32_t* off = c.off + (size_t)g * ((size_t)c.node_capacity + 1);
    uint32_t* tmp = c.inc_tmp + eb * 2;
    uint32_t* inc = c.inc + eb * 2;
    for (uint32_t e = blockIdx.x * PG_BLOCK + threadIdx.x; e < edges; e += gridDim.x * PG_BLOCK) {
        if (!c.edge_ok[eb + e]) continue;
#pragma unroll
        for (uint32_t side = 0; side < 2; ++side) {
            const uint32_t node = c.edges[(eb + e) * 2 + side], key = (e << 1) | side;
            const uint32_t lo = off[node], hi = off[node + 1];
            if constexpr (!RANK) {
                tmp[lo + atomicAdd(c.cursor + nb + node, 1u)] = key;
            } else {
                uint32_t rank = 0;
                for (uint32_t s = lo; s < hi; ++s) rank += tmp[s] < key ? 1u : 0u;
                inc[lo + rank] = key;
            }
        }
    }
}

// MODE 0: the initial energy, at the kept poses, of every graph; 1: at the candidates, of the graphs still at work; 2: the final one, at the
// kept poses, with the per-edge outputs.
template <int MODE>
__global__ __launch_bounds__(PG_BLOCK) void pg_energy_kernel(PgArgs a) {
    __shared__ float lds[128];
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    const PgState& st = c.state[g];
    if (MODE == 1 && (st.frozen || st.singular)) return;  // the whole workgroup
    const uint32_t edges = pg_clip(c.edge_counts[g], c.edge_capacity);
    const uint32_t nchunks = (edges + (VORS_PG_CHUNK - 1)) / VORS_PG_CHUNK;
    if (blockIdx.x >= nchunks) return;  // the whole workgroup
    const size_t N = (size_t)c.node_capacity, eb = (size_t)g * (size_t)c.edge_capacity;
    const uint32_t which = MODE == 1 ? st.cur ^ 1u : st.cur;
    const float* poses = c.poses + ((size_t)g * 2 + which) * N * 7;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        float en[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t e = chunk * VORS_PG_CHUNK + s * PG_BLOCK + threadIdx.x;
            en[s] = 0.0f;
            if (e >= edges) continue;
            const bool ok = c.edge_ok[eb + e] != 0u;
            float r[6], energy = 0.0f;
            if (ok) {
                const uint32_t i = c.edges[(eb + e) * 2], j = c.edges[(eb + e) * 2 + 1];
                float om[36];
                pg_load_info(c.info ? c.info + (eb + e) * 36 : nullptr, om);
                Iso err;
                pg_edge_error(iso_load(poses + (size_t)i * 7), iso_load(poses + (size_t)j * 7), iso_load(c.meas + (eb + e) * 7), &err, r);
                energy = pg_edge_energy(r, om, c.weight ? c.weight[eb + e] : 1.0f);
                en[s] = energy;
            }
            if constexpr (MODE == 2) {
                const float nan = __builtin_nanf("");
                if (c.edge_residuals) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) c.edge_residuals[(eb + e) * 6 + k] = ok ? r[k] : nan;
                }
                if (c.edge_energy) c.edge_energy[eb + e] = ok ? energy : nan;
            }
        }
        const float sum = pg_block_tree(en[0], en[1], en[2], en[3], lds);
        if (threadIdx.x == 0) c.energy_part[(size_t)g * pg_chunks(c.edge_capacity) + chunk] = sum;
    }
}

__device__ __forceinline__ float pg_graph_energy(const PgCall& c, int g) {
    const uint32_t edges = pg_clip(c.edge_counts[g], c.edge_capacity);
    return pg_sum_chunks(c.energy_part + (size_t)g * pg_chunks(c.edge_capacity), (edges + (VORS_PG_CHUNK - 1)) / VORS_PG_CHUNK);
}

__global__ void pg_start_kernel(PgCall c) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= c.n) return;
    PgState& st = c.state[g];
    st.energy = st.initial_energy = pg_graph_energy(c, g);
}

__global__ __launch_bounds__(PG_BLOCK) void pg_linearise_kernel(PgArgs a) {
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    const PgState& st = c.state[g];
    if (st.frozen || st.lin_ok) return;  // the whole workgroup
    const uint32_t edges = pg_clip(c.edge_counts[g], c.edge_capacity);
    const size_t N = (size_t)c.node_capacity, eb = (size_t)g * (size_t)c.edge_capacity;
    const float* poses = c.poses + ((size_t)g * 2 + st.cur) * N * 7;
    for (uint32_t e = blockIdx.x * PG_BLOCK + threadIdx.x; e < edges; e += gridDim.x * PG_BLOCK) {
        if (!c.edge_ok[eb + e]) continue;
        const uint32_t i = c.edges[(eb + e) * 2], j = c.edges[(eb + e) * 2 + 1];
        float om[36], w[36], lin[VORS_PG_LIN];
        pg_load_info(c.info ? c.info + (eb + e) * 36 : nullptr, om);
        pg_edge_linearise(iso_load(poses + (size_t)i * 7), iso_load(poses + (size_t)j * 7), iso_load(c.meas + (eb + e) * 7), om,
                          c.weight ? c.weight[eb + e] : 1.0f, w, lin);
        float4* wo = reinterpret_cast<float4*>(c.wmat + (eb + e) * 36);
#pragma unroll
        for (int k = 0; k < 9; ++k) wo[k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        float4* lo = reinterpret_cast<float4*>(c.lin + (eb + e) * VORS_PG_LIN);
#pragma unroll
        for (int k = 0; k < VORS_PG_LIN / 4; ++k) lo[k] = make_float4(lin[4 * k], lin[4 * k + 1], lin[4 * k + 2], lin[4 * k + 3]);
    }
}

__global__ __launch_bounds__(PG_BLOCK) void pg_gather_kernel(PgArgs a) {
    __shared__ double lds[128];
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    PgState& st = c.state[g];
    if (st.frozen) return;  // the whole workgroup
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity);
    const uint32_t nchunks = (nodes + (VORS_PG_CHUNK - 1)) / VORS_PG_CHUNK;
    if (blockIdx.x >= nchunks) return;  // the whole workgroup
    const size_t N = (size_t)c.node_capacity, nb = (size_t)g * N, eb = (size_t)g * (size_t)c.edge_capacity;
    const uint32_t* off = c.off + (size_t)g * (N + 1);
    const uint32_t* inc = c.inc + eb * 2;
    const float lambda = st.lambda;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        double rz[4], rr[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t k = chunk * VORS_PG_CHUNK + s * PG_BLOCK + threadIdx.x;
            rz[s] = rr[s] = 0.0;
            if (k >= nodes || c.node_class[nb + k] != PG_NODE_FREE) continue;
            float h[21], gk[6];
            const uint32_t lo = off[k], hi = off[k + 1];  // (a free node has an edge: lo < hi)
            for (uint32_t q = lo; q < hi; ++q) {
                const uint32_t key = inc[q];
                const float* lin = c.lin + (eb + (key >> 1)) * VORS_PG_LIN + (key & 1u) * 21;
                const float* ge = c.lin + (eb + (key >> 1)) * VORS_PG_LIN + 42 + (key & 1u) * 6;
#pragma unroll
                for (int m = 0; m < 21; ++m) h[m] = q == lo ? lin[m] : h[m] + lin[m];
#pragma unroll
                for (int m = 0; m < 6; ++m) gk[m] = q == lo ? ge[m] : gk[m] + ge[m];
            }
            float hd[21], fac[21], r[6], z[6];
            const bool ok = pg_node_factor(h, lambda, hd, fac);
            if (!ok) atomicOr(&st.singular, 1u);
#pragma unroll
            for (int m = 0; m < 21; ++m) {
                c.hd[(nb + k) * 21 + m] = hd[m];
                c.fac[(nb + k) * 21 + m] = fac[m];
            }
#pragma unroll
            for (int m = 0; m < 6; ++m) r[m] = -gk[m];
            pg_factor_solve(fac, r, z);
            pg_store6(c.r + (nb + k) * 6, r);
            pg_store6(c.z + (nb + k) * 6, z);
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                c.x[(nb + k) * 6 + m] = 0.0f;
                c.p[((size_t)g * 2 * N + N + k) * 6 + m] = 0.0f;  // p of "iteration -1", which iteration 0 scales by beta = 0
            }
            rz[s] = pg_dot6(r, z);
            rr[s] = pg_dot6(r, r);
        }
        const double srz = pg_block_tree(rz[0], rz[1], rz[2], rz[3], lds);
        const double srr = pg_block_tree(rr[0], rr[1], rr[2], rr[3], lds);
        if (threadIdx.x == 0) {
            pg_dots(c, g, PG_DOT_RZ)[chunk] = srz;
            pg_dots(c, g, PG_DOT_RR)[chunk] = srr;
            pg_dots(c, g, PG_DOT_RR0)[chunk] = srr;
        }
    }
}

struct PgCgArgs {
    int g0, t;
    PgCall c;
};

__global__ __launch_bounds__(PG_BLOCK) void pg_cg_product_kernel(PgCgArgs a) {
    __shared__ double lds[128];
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y, t = a.t;
    PgState& st = c.state[g];
    if (st.frozen || st.singular) return;  // the whole workgroup
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity);
    const uint32_t nchunks = (nodes + (VORS_PG_CHUNK - 1)) / VORS_PG_CHUNK;
    const size_t nc = pg_chunks(c.node_capacity);
    const uint32_t cur = (uint32_t)t & 1u, prev = cur ^ 1u;
    const double rr = pg_sum_chunks(pg_dots(c, g, PG_DOT_RR) + cur * nc, nchunks), rr0 = pg_sum_chunks(pg_dots(c, g, PG_DOT_RR0), nchunks);
    const bool done = st.cg_done[prev] != 0u || pg_cg_reached(rr, rr0, c.cg_tol);
    if (blockIdx.x == 0 && threadIdx.x == 0) st.cg_done[cur] = done ? 1u : 0u;
    if (done || blockIdx.x >= nchunks) return;  // the whole workgroup
    const float beta = t > 0 ? pg_cg_beta(pg_sum_chunks(pg_dots(c, g, PG_DOT_RZ) + cur * nc, nchunks),
                                          pg_sum_chunks(pg_dots(c, g, PG_DOT_RZ) + prev * nc, nchunks))
                             : 0.0f;
    const size_t N = (size_t)c.node_capacity, nb = (size_t)g * N, eb = (size_t)g * (size_t)c.edge_capacity;
    const uint32_t* off = c.off + (size_t)g * (N + 1);
    const uint32_t* inc = c.inc + eb * 2;
    const float* z = c.z + nb * 6;
    const float* p_prev = c.p + ((size_t)g * 2 + prev) * N * 6;
    float* p_cur = c.p + ((size_t)g * 2 + cur) * N * 6;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        double pq[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t k = chunk * VORS_PG_CHUNK + s * PG_BLOCK + threadIdx.x;
            pq[s] = 0.0;
            if (k >= nodes || c.node_class[nb + k] != PG_NODE_FREE) continue;
            float zk[6], pk[6], p[6], y[6], hd[21];
            pg_load6(z + (size_t)k * 6, zk);
            pg_load6(p_prev + (size_t)k * 6, pk);
#pragma unroll
            for (int m = 0; m < 21; ++m) hd[m] = c.hd[(nb + k) * 21 + m];
            pg_cg_direction(zk, beta, pk, p);
            pg_store6(p_cur + (size_t)k * 6, p);
            pg_matvec_own(hd, p, y);
            const uint32_t lo = off[k], hi = off[k + 1];
            for (uint32_t q = lo; q < hi; ++q) {
                const uint32_t key = inc[q], e = key >> 1, side = key & 1u;
                const uint32_t other = c.edges[(eb + e) * 2 + (side ^ 1u)];
                const float4* w4 = reinterpret_cast<const float4*>(c.wmat + (eb + e) * 36);
                float w[36], zo[6], po[6], d[6];
#pragma unroll
                for (int m = 0; m < 9; ++m) {
                    const float4 v = w4[m];
                    w[4 * m] = v.x; w[4 * m + 1] = v.y; w[4 * m + 2] = v.z; w[4 * m + 3] = v.w;
                }
                pg_load6(z + (size_t)other * 6, zo);
                pg_load6(p_prev + (size_t)other * 6, po);
                pg_cg_direction(zo, beta, po, d);
                if (side == 0u) pg_matvec_edge(w, false, d, y);
                else pg_matvec_edge(w, true, d, y);
            }
            pg_store6(c.q + (nb + k) * 6, y);
            pq[s] = pg_dot6(p, y);
        }
        const double sum = pg_block_tree(pq[0], pq[1], pq[2], pq[3], lds);
        if (threadIdx.x == 0) pg_dots(c, g, PG_DOT_PQ)[chunk] = sum;
    }
}

__global__ __launch_bounds__(PG_BLOCK) void pg_cg_update_kernel(PgCgArgs a) {
    __shared__ double lds[128];
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y, t = a.t;
    PgState& st = c.state[g];
    const uint32_t cur = (uint32_t)t & 1u, next = cur ^ 1u;
    if (st.frozen || st.singular || st.cg_done[cur]) return;  // the whole workgroup
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity);
    const uint32_t nchunks = (nodes + (VORS_PG_CHUNK - 1)) / VORS_PG_CHUNK;
    if (blockIdx.x >= nchunks) return;  // the whole workgroup
    const size_t nc = pg_chunks(c.node_capacity);
    const float alpha = pg_cg_alpha(pg_sum_chunks(pg_dots(c, g, PG_DOT_RZ) + cur * nc, nchunks), pg_sum_chunks(pg_dots(c, g, PG_DOT_PQ), nchunks));
    if (blockIdx.x == 0 && threadIdx.x == 0) st.cg_spent += 1u;
    const size_t N = (size_t)c.node_capacity, nb = (size_t)g * N;
    const float* p_cur = c.p + ((size_t)g * 2 + cur) * N * 6;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        double rz[4], rr[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const uint32_t k = chunk * VORS_PG_CHUNK + s * PG_BLOCK + threadIdx.x;
            rz[s] = rr[s] = 0.0;
            if (k >= nodes || c.node_class[nb + k] != PG_NODE_FREE) continue;
            float x[6], r[6], p[6], q[6], z[6], fac[21];
            pg_load6(c.x + (nb + k) * 6, x);
            pg_load6(c.r + (nb + k) * 6, r);
            pg_load6(p_cur + (size_t)k * 6, p);
            pg_load6(c.q + (nb + k) * 6, q);
#pragma unroll
            for (int m = 0; m < 21; ++m) fac[m] = c.fac[(nb + k) * 21 + m];
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                x[m] = x[m] + alpha * p[m];
                r[m] = r[m] - alpha * q[m];
            }
            pg_factor_solve(fac, r, z);
            pg_store6(c.x + (nb + k) * 6, x);
            pg_store6(c.r + (nb + k) * 6, r);
            pg_store6(c.z + (nb + k) * 6, z);
            rz[s] = pg_dot6(r, z);
            rr[s] = pg_dot6(r, r);
        }
        const double srz = pg_block_tree(rz[0], rz[1], rz[2], rz[3], lds);
        const double srr = pg_block_tree(rr[0], rr[1], rr[2], rr[3], lds);
        if (threadIdx.x == 0) {
            (pg_dots(c, g, PG_DOT_RZ) + next * nc)[chunk] = srz;
            (pg_dots(c, g, PG_DOT_RR) + next * nc)[chunk] = srr;
        }
    }
}

__global__ __launch_bounds__(PG_BLOCK) void pg_candidate_kernel(PgArgs a) {
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    PgState& st = c.state[g];
    if (st.frozen || st.singular) return;  // the whole workgroup
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity);
    const size_t N = (size_t)c.node_capacity, nb = (size_t)g * N;
    const float* from = c.poses + ((size_t)g * 2 + st.cur) * N * 7;
    float* to = c.poses + ((size_t)g * 2 + (st.cur ^ 1u)) * N * 7;
    for (uint32_t base = blockIdx.x * PG_BLOCK; base < nodes; base += gridDim.x * PG_BLOCK) {
        const uint32_t k = base + threadIdx.x;
        uint32_t bits = 0u;
        if (k < nodes) {
            if (c.node_class[nb + k] == PG_NODE_FREE) {
                float d[6];
                pg_load6(c.x + (nb + k) * 6, d);
                iso_store(pg_candidate(iso_load(from + (size_t)k * 7), d), to + (size_t)k * 7);
                const float d2 = pg_step2(d);
                if (d2 == d2) bits = __builtin_bit_cast(uint32_t, d2);  // (d2 >= 0: its bits order as its value; a NaN is left out)
            } else {
#pragma unroll
                for (int i = 0; i < 7; ++i) to[(size_t)k * 7 + i] = from[(size_t)k * 7 + i];
            }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)bits, sh);
            bits = o > bits ? o : bits;
        }
        if ((threadIdx.x & 63) == 0 && bits) atomicMax(&st.step2_bits, bits);
    }
}

__global__ void pg_verdict_kernel(PgCall c) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= c.n) return;
    PgState& st = c.state[g];
    if (st.frozen) return;
    if (st.singular) {
        st.status = PG_SINGULAR;
        st.frozen = 1u;
        return;
    }
    const float energy = pg_graph_energy(c, g);
    const bool accepted = pg_accepts(energy, st.energy);
    st.lambda = pg_lambda_after(accepted, st.lambda);
    if (accepted) {
        const float d2 = __builtin_bit_cast(float, st.step2_bits);
        st.cur ^= 1u;
        st.energy = energy;
        st.accepted += 1u;
        st.last_step_norm = sqrtf(d2);
        st.lin_ok = 0u;
        if (d2 <= c.step_eps * c.step_eps) {
            st.status = PG_CONVERGED;
            st.frozen = 1u;
        }
    } else {
        st.rejected += 1u;
        st.lin_ok = 1u;
    }
    st.step2_bits = 0u;
    st.cg_done[0] = st.cg_done[1] = 0u;
}

__global__ __launch_bounds__(PG_BLOCK) void pg_finish_kernel(PgArgs a) {
    const PgCall& c = a.c;
    const int g = a.g0 + blockIdx.y;
    const PgState& st = c.state[g];
    const uint32_t nodes = pg_clip(c.node_counts[g], c.node_capacity);
    const size_t N = (size_t)c.node_capacity;
    const float* from = c.poses + ((size_t)g * 2 + st.cur) * N * 7;
    for (uint32_t k = blockIdx.x * PG_BLOCK + threadIdx.x; k < nodes; k += gridDim.x * PG_BLOCK) {
#pragma unroll
        for (int i = 0; i < 7; ++i) c.poses_out[((size_t)g * N + k) * 7 + i] = from[(size_t)k * 7 + i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && c.stats) {
        vors_pose_graph_stats o;
        o.status = st.status;
        o.accepted_steps = st.accepted;
        o.rejected_steps = st.rejected;
        o.cg_iterations = st.cg_spent;
        o.valid_edges = st.valid_edges;
        o.skipped_edges = st.skipped_edges;
        o.free_nodes = st.free_nodes;
        o.fixed_nodes = st.fixed_nodes;
        o.isolated_nodes = st.isolated_nodes;
        o.initial_energy = st.initial_energy;
        o.final_energy = pg_graph_energy(c, g);
        o.last_step_norm = st.last_step_norm;
        o.final_lambda = st.lambda;
        c.stats[g] = o;
    }
}

void launch_pose_graph(const PgCall& c, hipStream_t s) {
    const auto extent = [](int capacity, size_t per_block) {
        const size_t want = ((size_t)capacity + per_block - 1) / per_block;
        return (unsigned)(want > PG_MAX_CHUNKS ? PG_MAX_CHUNKS : want);
    };
    const unsigned node_blocks = extent(c.node_capacity, PG_BLOCK), edge_blocks = extent(c.edge_capacity, PG_BLOCK);
    const unsigned node_chunks = extent(c.node_capacity, VORS_PG_CHUNK), edge_chunks = extent(c.edge_capacity, VORS_PG_CHUNK);
    const dim3 per_graph((unsigned)((c.n + 63) / 64));
    PgArgs a{0, c};
    PgCgArgs ca{0, 0, c};
    // kernel(args) on (x, graphs) for every slice of graphs
    auto on_graphs = [&](auto kernel, unsigned x, auto& args) {
        for_pair_slices(c.n, [&](int g0, int ng) {
            args.g0 = g0;
            hipLaunchKernelGGL(kernel, dim3(x, ng), dim3(PG_BLOCK), 0, s, args);
        });
    };
    on_graphs(pg_begin_kernel, node_blocks, a);
    on_graphs(pg_edges_kernel, edge_blocks, a);
    for_pair_slices(c.n, [&](int g0, int ng) {
        a.g0 = g0;
        hipLaunchKernelGGL(pg_scan_kernel, dim3(ng), dim3(PG_BLOCK), 0, s, a);
    });
    on_graphs(pg_incidence_kernel<false>, edge_blocks, a);
    on_graphs(pg_incidence_kernel<true>, edge_blocks, a);
    on_graphs(pg_energy_kernel<0>, edge_chunks, a);
    hipLaunchKernelGGL(pg_start_kernel, per_graph, dim3(64), 0, s, c);
    for (int it = 0; it < c.iters; ++it) {
        on_graphs(pg_linearise_kernel, edge_blocks, a);
        on_graphs(pg_gather_kernel, node_chunks, a);
        for (int t = 0; t < c.cg_iters; ++t) {
            ca.t = t;
            on_graphs(pg_cg_product_kernel, node_chunks, ca);
            on_graphs(pg_cg_update_kernel, node_chunks, ca);
        }
        on_graphs(pg_candidate_kernel, node_blocks, a);
        on_graphs(pg_energy_kernel<1>, edge_chunks, a);
        hipLaunchKernelGGL(pg_verdict_kernel, per_graph, dim3(64), 0, s, c);
    }
    on_graphs(pg_energy_kernel<2>, edge_chunks, a);
    on_graphs(pg_finish_kernel, node_blocks, a);
}

}  // namespace vors
