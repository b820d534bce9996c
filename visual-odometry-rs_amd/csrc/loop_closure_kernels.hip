// Loop closure: vors_loop_signatures, vors_loop_candidates, vors_loop_verify_edges (include/vors_hip.h 2h). Handle-free; the
// rules are lie.h lc_*, the texts the host twins run, bit for bit. No workgroup waits for another; no floating-point atomic exists.
// SIGNATURES  a workgroup per plane. The plane is one run of rows * cols bytes, read once as aligned 16-byte words; a lane walks the 16
//             bytes of a word with the cell of the first byte and the next cell edge in registers and hands a cell's partial sum to an
//             LDS counter (integer atomics: exact, any order) when the run of bytes leaves the cell. Then a lane per cell forms the
//             value, and the two sums of the meta record go through two more LDS counters.
// CANDIDATES  the project's matrix-core kernel. A workgroup per tile of 32 queries and set, four wavefronts; the 32 query signatures
//             stay in LDS (rows padded by 16 bytes), and a wavefront takes every fourth tile of 32 candidates below the diagonal band
//             (i + min_gap <= j): D / 32 steps of v_mfma_i32_32x32x32_i8, A = 16 bytes of a candidate row straight from memory, B = the
//             same 16 k of a query row from LDS. A and B are rows of ONE matrix cut the same way, so whatever order the instruction
//             gives the 16 k of a lane half, both sides agree and the integer dot product is exact. The C map is the one of every
//             32x32 MFMA: column (the query) = lane & 31, row (the candidate) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//             A lane therefore owns ONE query and 16 candidates of the tile: its top-k list lives in registers (lc_topk_insert with
//             constant indices), the candidate rows' root, sum, flat flag and pose are formed once per tile by lanes 0..31 and fetched
//             with ds_bpermute. The gates come first; before the f64 divide an f32 estimate of the score (error < 1e-6) drops what is
//             below min_score by more than 1e-4, which the exact score would drop as well. At the end the eight lists of a query
//             (two lane halves, four wavefronts) are merged by the same insertion: the order is total, the result that of one list.
// VERIFY      ONE workgroup of 1024 lanes over chunks of 1024 candidates in sequence: the verdict per lane (lc_verify), then the ordered
//             compaction — ballot and popcount inside a wavefront, the 16 wavefront totals through LDS, the running base in a register.
#include "device_common.h"

namespace vors {

#define LC_SIG_BLOCK 256
#define LC_CAND_BLOCK 256
#define LC_TILE 32
#define LC_ROW_PAD 16
#define LC_VERIFY_BLOCK 1024

typedef int lc_v4i __attribute__((ext_vector_type(4)));
typedef int lc_v16i __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(LC_SIG_BLOCK) void lc_signature_kernel(LcSigCall c) {
    __shared__ uint32_t cell[1024];
    __shared__ int32_t meta_sum;
    __shared__ uint32_t meta_sumsq;
    const uint32_t rows = (uint32_t)c.rows, cols = (uint32_t)c.cols, tr = (uint32_t)c.tr, tc = (uint32_t)c.tc, d = tr * tc;
    const size_t plane = blockIdx.x;
    for (uint32_t t = threadIdx.x; t < d; t += LC_SIG_BLOCK) cell[t] = 0u;
    if (threadIdx.x == 0) {
        meta_sum = 0;
        meta_sumsq = 0u;
    }
    __syncthreads();
    const uint32_t total = rows * cols;
    const uint8_t* base = c.gray + plane * total;
    // aligned words that hold at least one byte of the plane: word w covers plane offsets [16 w - mis, 16 w - mis + 16)
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u);
    const uint32_t nwords = (total + mis + 15u) / 16u;
    for (uint32_t w = threadIdx.x; w < nwords; w += LC_SIG_BLOCK) {
        const uint4 v = *reinterpret_cast<const uint4*>(base - mis + (size_t)w * 16u);
        const uint32_t word[4] = {v.x, v.y, v.z, v.w};
        const uint32_t b0 = w == 0u ? mis : 0u;                // first byte of the word inside the plane
        const uint32_t off = w * 16u + b0 - mis;               // its offset in the plane
        const uint32_t b1 = b0 + (total - off) < 16u ? b0 + (total - off) : 16u;  // one past its last byte inside the plane
        uint32_t row = off / cols, x = off - row * cols;
        uint32_t cy = lc_cell_of(row, rows, tr), cx = lc_cell_of(x, cols, tc);
        uint32_t next_row = lc_cell_begin(cy + 1u, rows, tr), next_x = lc_cell_begin(cx + 1u, cols, tc);
        uint32_t acc = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 16u; ++b) {
            if (b >= b0 && b < b1) {
                acc += (word[b >> 2] >> (8u * (b & 3u))) & 0xffu;
                ++x;
                if (x == next_x) {  // the run leaves the cell (the last cell of a row ends at cols)
                    atomicAdd(&cell[cy * tc + cx], acc);
                    acc = 0u;
                    if (x == cols) {
                        x = 0u;
                        cx = 0u;
                        ++row;
                        if (row == next_row) {
                            ++cy;
                            next_row = lc_cell_begin(cy + 1u, rows, tr);
                        }
                    } else {
                        ++cx;
                    }
                    next_x = lc_cell_begin(cx + 1u, cols, tc);
                }
            }
        }
        if (acc) atomicAdd(&cell[cy * tc + cx], acc);  // (acc != 0: the run stopped inside a cell, cy < tr)
    }
    __syncthreads();
    int32_t sum = 0;
    uint32_t sumsq = 0u;
    for (uint32_t t = threadIdx.x; t < d; t += LC_SIG_BLOCK) {
        const uint32_t cy = t / tc, cx = t - cy * tc;
        const uint32_t cnt = (lc_cell_begin(cy + 1u, rows, tr) - lc_cell_begin(cy, rows, tr)) * (lc_cell_begin(cx + 1u, cols, tc) - lc_cell_begin(cx, cols, tc));
        const int8_t s = lc_cell_value(cell[t], cnt);
        c.sig[plane * d + t] = s;
        sum += (int32_t)s;
        sumsq += (uint32_t)((int32_t)s * (int32_t)s);
    }
    atomicAdd(&meta_sum, sum);
    atomicAdd(&meta_sumsq, sumsq);
    __syncthreads();
    if (threadIdx.x == 0) c.meta[plane] = LcMeta{meta_sum, meta_sumsq};
}

void launch_loop_signatures(const LcSigCall& c, hipStream_t s) {
    hipLaunchKernelGGL(lc_signature_kernel, dim3((unsigned)c.n), dim3(LC_SIG_BLOCK), 0, s, c);
}

struct LcCandArgs {
    int set0;
    LcCandCall c;
};

// what a lane keeps of one signature for the gates and the score
struct LcRow {
    double root;
    float rootf;
    int32_t sum;
    uint32_t flat;
    float pose[7];
};
__device__ __forceinline__ LcRow lc_row_load(const LcCandCall& c, size_t set, uint32_t row) {
    LcRow r;
    const LcMeta m = c.meta[set * (size_t)c.capacity + row];
    const int64_t va = lc_variance(c.d, m.sum, m.sumsq);
    r.root = lc_root(va);
    r.rootf = (float)r.root;
    r.sum = m.sum;
    r.flat = va == 0 ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < 7; ++k) r.pose[k] = c.poses ? c.poses[(set * (size_t)c.capacity + row) * (size_t)c.pose_stride + k] : 0.0f;
    return r;
}
__device__ __forceinline__ LcRow lc_row_from_lane(const LcRow& r, int lane, bool with_pose) {
    LcRow o;
    o.root = __shfl(r.root, lane);
    o.rootf = __shfl(r.rootf, lane);
    o.sum = __shfl(r.sum, lane);
    o.flat = (uint32_t)__shfl((int)r.flat, lane);
#pragma unroll
    for (int k = 0; k < 7; ++k) o.pose[k] = with_pose ? __shfl(r.pose[k], lane) : 0.0f;
    return o;
}

// LDS: [0, region0) the query tile, 32 rows of d + LC_ROW_PAD bytes — and, after the tiles, the 256 lists of the merge: n[256],
// idx[256][8], score[256][8]
constexpr size_t LC_MERGE_BYTES = (size_t)LC_CAND_BLOCK * 4 + 2 * (size_t)LC_CAND_BLOCK * VORS_LC_MAX_K * 4;
static size_t lc_cand_lds_bytes(int d) {
    const size_t tile = (size_t)LC_TILE * ((size_t)d + LC_ROW_PAD);
    return tile > LC_MERGE_BYTES ? tile : LC_MERGE_BYTES;
}

__global__ __launch_bounds__(LC_CAND_BLOCK) void lc_candidates_kernel(LcCandArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lc_lds[];
    __shared__ uint32_t counts_lds[(LC_CAND_BLOCK / 64) * VORS_LC_COUNTS];
    const LcCandCall& c = a.c;
    const size_t set = (size_t)a.set0 + blockIdx.y;
    const uint32_t cap = (uint32_t)c.capacity, d = (uint32_t)c.d;
    const uint32_t given = c.counts_in[set], count = given < cap ? given : cap;
    const uint32_t first = c.query_first ? c.query_first[set] : 0u;
    const uint32_t j0 = (gridDim.x - 1u - blockIdx.x) * LC_TILE;  // the last query tile has the most candidate tiles: it starts first
    if (j0 >= count || j0 + LC_TILE <= first) return;  // (uniform) no query of this tile is answered
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, q = lane & 31u, h = lane >> 5;
    const int8_t* sig = c.sig + set * (size_t)cap * d;
    const uint32_t row_bytes = d + LC_ROW_PAD, words_per_row = d / 16u;
    // the query tile into LDS; a row beyond the count repeats the last one (it is never answered)
    for (uint32_t w = threadIdx.x; w < LC_TILE * words_per_row; w += LC_CAND_BLOCK) {
        const uint32_t r = w / words_per_row, k = w - r * words_per_row;
        const uint32_t src = j0 + r < count ? j0 + r : count - 1u;
        *reinterpret_cast<uint4*>(lc_lds + r * row_bytes + k * 16u) = *reinterpret_cast<const uint4*>(sig + (size_t)src * d + k * 16u);
    }
    const uint32_t j = j0 + q;
    const bool answered = j >= first && j < count;
    const LcRow rj = lc_row_load(c, set, j < count ? j : count - 1u);
    const bool with_pose = c.poses != nullptr;
    const float score_floor = c.min_score - 1e-4f;
    uint32_t idx[VORS_LC_MAX_K], n = 0u, cnt[VORS_LC_COUNTS];
    float score[VORS_LC_MAX_K];
#pragma unroll
    for (int p = 0; p < VORS_LC_MAX_K; ++p) {
        idx[p] = VORS_LC_EMPTY;
        score[p] = 0.0f;
    }
#pragma unroll
    for (int p = 0; p < VORS_LC_COUNTS; ++p) cnt[p] = 0u;
    __syncthreads();
    // candidate tiles that reach below the band of the tile's last query
    const uint32_t jmax = j0 + LC_TILE - 1u < count - 1u ? j0 + LC_TILE - 1u : count - 1u;
    const uint32_t ntiles = jmax >= c.min_gap ? (jmax - c.min_gap) / LC_TILE + 1u : 0u;
    for (uint32_t it = wave; it < ntiles; it += LC_CAND_BLOCK / 64) {
        const uint32_t i0 = it * LC_TILE;
        const uint32_t arow = i0 + q < count ? i0 + q : count - 1u;
        const LcRow mine = lc_row_load(c, set, arow);  // (lanes 32..63 repeat lanes 0..31)
        const int8_t* ap = sig + (size_t)arow * d + h * 16u;
        const unsigned char* bp = lc_lds + q * row_bytes + h * 16u;
        lc_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t ks = 0; ks < d; ks += 32u) {
            const lc_v4i av = *reinterpret_cast<const lc_v4i*>(ap + ks);
            const lc_v4i bv = *reinterpret_cast<const lc_v4i*>(bp + ks);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t rr = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * h, i = i0 + rr;
            const LcRow ri = lc_row_from_lane(mine, (int)rr, with_pose);
            if (answered && (uint64_t)i + c.min_gap <= (uint64_t)j) {
                cnt[0] += 1u;
                if (ri.flat | rj.flat) {
                    cnt[1] += 1u;
                } else if (with_pose && !lc_pose_passes(ri.pose, rj.pose, c.max_dist_m, c.min_qdot)) {
                    cnt[2] += 1u;
                } else {
                    const int64_t num = lc_numerator((int)d, acc[r], ri.sum, rj.sum);
                    bool passes = !((float)num / (ri.rootf * rj.rootf) < score_floor);
                    float s = 0.0f;
                    if (passes) {
                        s = lc_score(num, ri.root, rj.root);
                        passes = lc_score_passes(s, c.min_score);
                    }
                    if (!passes) {
                        cnt[3] += 1u;
                    } else {
                        cnt[4] += 1u;
                        lc_topk_insert(idx, score, &n, c.k, i, s);
                    }
                }
            }
        }
    }
    __syncthreads();  // every wavefront is done with the query tile: the merge lists take its place
    uint32_t* m_n = reinterpret_cast<uint32_t*>(lc_lds);
    uint32_t* m_idx = m_n + LC_CAND_BLOCK;
    float* m_score = reinterpret_cast<float*>(m_idx + LC_CAND_BLOCK * VORS_LC_MAX_K);
    m_n[threadIdx.x] = n;
#pragma unroll
    for (int p = 0; p < VORS_LC_MAX_K; ++p) {
        m_idx[threadIdx.x * VORS_LC_MAX_K + p] = idx[p];
        m_score[threadIdx.x * VORS_LC_MAX_K + p] = score[p];
    }
    __syncthreads();
    if (threadIdx.x < LC_TILE && answered) {  // (wavefront 0, lane half 0: q == threadIdx.x)
        n = 0u;
#pragma unroll
        for (int p = 0; p < VORS_LC_MAX_K; ++p) {
            idx[p] = VORS_LC_EMPTY;
            score[p] = 0.0f;
        }
#pragma unroll 1
        for (uint32_t list = 0; list < LC_CAND_BLOCK / LC_TILE; ++list) {
            const uint32_t src = list * LC_TILE + q, have = m_n[src];
#pragma unroll 1
            for (uint32_t e = 0; e < have; ++e) lc_topk_insert(idx, score, &n, c.k, m_idx[src * VORS_LC_MAX_K + e], m_score[src * VORS_LC_MAX_K + e]);
        }
        LcCand* out = c.cand + (set * (size_t)cap + j) * c.k;
#pragma unroll
        for (uint32_t p = 0; p < VORS_LC_MAX_K; ++p)
            if (p < c.k) out[p] = LcCand{idx[p], score[p]};
        c.cand_counts[set * (size_t)cap + j] = n;
    }
    if (c.counts) block_counts<VORS_LC_COUNTS, LC_CAND_BLOCK>(cnt, counts_lds, CountsAdd{c.counts + set * VORS_LC_COUNTS});
}

hipError_t launch_loop_candidates(const LcCandCall& c, hipStream_t s) {
    if (c.counts) {  // the atomics add onto zeros: without them no launch
        const hipError_t e = hipMemsetAsync(c.counts, 0, (size_t)c.n * VORS_LC_COUNTS * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
    }
    const unsigned tiles = (unsigned)(((size_t)c.capacity + LC_TILE - 1) / LC_TILE);
    LcCandArgs a{0, c};
    for_pair_slices(c.n, [&](int set0, int nsets) {
        a.set0 = set0;
        hipLaunchKernelGGL(lc_candidates_kernel, dim3(tiles, (unsigned)nsets), dim3(LC_CAND_BLOCK), lc_cand_lds_bytes(c.d), s, a);
    });
    return hipSuccess;
}

__global__ __launch_bounds__(LC_VERIFY_BLOCK) void lc_verify_kernel(LcVerifyCall c) {
    __shared__ uint32_t wave_total[LC_VERIFY_BLOCK / 64];
    __shared__ uint32_t counts[VORS_LC_VERDICTS];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    if (t < VORS_LC_VERDICTS) counts[t] = 0u;
    const uint32_t given = c.edge_count[0];
    uint32_t base = given < c.edge_capacity ? given : c.edge_capacity;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < c.m; c0 += LC_VERIFY_BLOCK) {  // (c.m <= 2^28: no wrap)
        const uint32_t e = c0 + t;
        const bool live = e < c.m;
        uint32_t verdict = LC_STATUS, i = 0u, j = 0u;
        float r12[12];
        const float* fwd = nullptr;
        const float* info = nullptr;
        if (live) {
            i = c.pairs[2 * (size_t)e];
            j = c.pairs[2 * (size_t)e + 1];
            fwd = c.fwd + (size_t)e * c.fwd_stride;
            info = c.info ? c.info + (size_t)e * 36 : nullptr;
            const bool status_ok = c.status_fwd[e] == VORS_TRACK_OK && (!c.status_bwd || c.status_bwd[e] == VORS_TRACK_OK);
            verdict = lc_verify(i, j, status_ok, fwd, c.bwd ? c.bwd + (size_t)e * c.bwd_stride : nullptr, info, c.poses, c.pose_stride, c.node_count,
                                c.max_cycle_trans, c.max_cycle_rot, c.max_prior_trans, c.max_prior_rot, r12);
        }
        const bool accepted = live && verdict == LC_ACCEPTED;
        const unsigned long long ballot = __ballot(accepted);
        if (lane == 0u) wave_total[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (uint32_t w = 0; w < LC_VERIFY_BLOCK / 64; ++w) {
            const uint32_t v = wave_total[w];
            before += w < wave ? v : 0u;
            total += v;
        }
        if (accepted) {
            const uint32_t pos = base + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
            if (pos < c.edge_capacity) {
                c.edges[2 * (size_t)pos] = i;
                c.edges[2 * (size_t)pos + 1] = j;
#pragma unroll
                for (int k = 0; k < 7; ++k) c.meas[(size_t)pos * 7 + k] = fwd[k];
                if (c.info_out)
                    for (int k = 0; k < 36; ++k) c.info_out[(size_t)pos * 36 + k] = info ? info[k] : (k % 7 == 0 ? 1.0f : 0.0f);
                if (c.edge_weight) c.edge_weight[pos] = c.weight;
            } else {
                verdict = LC_CAPACITY;
            }
        }
        if (live) {
            c.verdict[e] = verdict;
            if (c.residuals)
#pragma unroll
                for (int k = 0; k < 12; ++k) c.residuals[(size_t)e * 12 + k] = r12[k];
            atomicAdd(&counts[verdict], 1u);
        }
        base = base + total < c.edge_capacity ? base + total : c.edge_capacity;
        __syncthreads();  // (the next chunk writes the wavefront totals again)
    }
    if (t == 0u) c.edge_count[0] = base;
    if (c.counts && t < VORS_LC_VERDICTS) c.counts[t] = counts[t];
}

void launch_loop_verify(const LcVerifyCall& c, hipStream_t s) { hipLaunchKernelGGL(lc_verify_kernel, dim3(1), dim3(LC_VERIFY_BLOCK), 0, s, c); }

}  // namespace vors
