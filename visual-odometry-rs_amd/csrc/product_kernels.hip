// The batch products of a prepared batch (gfx950 / CDNA4, wave64): residual maps, depth reprojection, depth fusion, point clouds and the
// keyframe-map appends, with their launchers. Per-point outputs of one level at explicit models, made of the EXACT point sources and
// per-point pieces of lm_sources.h — always the reference's per-point arithmetic, whatever the handle's — and cut into chunks like
// lm_eval_pairs_kernel (lm_sources.h level_cut). Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "lm_sources.h"
#include "voxel_table_device.h"

namespace vors {

// ------------------------------------------------------------------------------------------------------------
// vors_batch_residual_maps: what one evaluation of a level is made of, per point instead of summed — the position every usable
// candidate warps to, its raw residual (no Huber weight) where it passes the strict inside test, a 256-bin histogram of |residual| per
// pair and the scale read off it. Grid = (chunks of the level) x pairs with lm_eval_pairs_kernel's cut of a level; the loop is
// eval_accumulate's exact loop (positions -> warp_point -> load_taps -> bilinear_residual) with stores for a sink: no Jacobian, no sums,
// no reduction, no workspace. The planes have the keyframe pixel geometry of the level (row-major) in every candidate mode: a dense pass
// visits every pixel and writes the NaN of a pixel that is no point itself, the candidate lists scatter into planes the launcher has
// filled with NaN. Always the reference's per-point arithmetic (this object), whatever the handle's.
// Histogram (HIST): one sub-histogram per wavefront in LDS (4 x 1 KiB, LDS atomics), added at the end and flushed with one global integer
// atomicAdd per non-empty bin and workgroup into a zeroed array: integer counts, so the result does not depend on the schedule. Without
// HIST the kernel has no LDS and no atomic at all.
// ------------------------------------------------------------------------------------------------------------
#define RMAPS_BLOCK 256
// Pixel index of point g of a group in the level's plane (-1: no point). The dense sources' slot() IS the pixel; a list record carries it.
template <bool LEVEL0>
__device__ __forceinline__ int plane_pixel(const DenseSrc<LEVEL0>& src, const typename DenseSrc<LEVEL0>::Raw& r, int g, int) {
    return src.slot(r, g, 0);
}
template <bool LEVEL0, bool FAST>
__device__ __forceinline__ int plane_pixel(const DenseQuadSrc<LEVEL0, FAST>& src, const typename DenseQuadSrc<LEVEL0, FAST>::Raw& r, int g, int) {
    return src.slot(r, g, 0);
}
__device__ __forceinline__ int plane_pixel(const SlimSrc&, const SlimSrc::Raw& r, int g, int cols) {
    return r.valid[g] ? (int)(r.r[g].xy >> 16) * cols + (int)(r.r[g].xy & 0xffffu) : -1;
}
template <bool HIST, class Src>
__device__ __forceinline__ void residual_maps_sweep(const Src& src, int first, int last, const ImgCtx& c, const Iso& model, float* res, float* uv,
                                                    bool wide, uint32_t* wave_hist) {
    constexpr int G = Src::G;
    const float nan = __builtin_nanf("");
    const unsigned plane = (unsigned)(c.rows * c.cols);
    for (typename Src::Cursor cur = src.template begin<RMAPS_BLOCK>(first); cur.i < last; cur = src.template advance<RMAPS_BLOCK>(cur)) {
        typename Src::Raw raw;
        src.template fetch<RMAPS_BLOCK>(cur, last, raw);
        Pos pos[G];
        src.positions(raw, pos);
        Warped w[G];
#pragma unroll
        for (int g = 0; g < G; ++g) w[g] = warp_point(c, model, pos[g]);
        Taps t[G];
#pragma unroll
        for (int g = 0; g < G; ++g) t[g] = load_taps(c, w[g]);
        float r[G], u[G], v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float r_true = bilinear_residual(pos[g].tmpl, w[g], t[g]);
            const bool usable = pos[g].tmpl >= 0.f;
            r[g] = w[g].inside ? r_true : nan;
            u[g] = usable ? w[g].u : nan;
            v[g] = usable ? w[g].v : nan;
        }
        if constexpr (HIST) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (w[g].inside) atomicAdd(&wave_hist[min((int)fabsf(r[g]), VORS_RESIDUAL_BINS - 1)], 1u);  // (|r| <= 255 up to the rounding of the four products: 255.00002 happens)
        }
        if constexpr (G == 4) {
            if (wide) {  // (uniform) a quad owns four adjacent pixels of one row, 16-byte aligned in both planes
                const unsigned px = (unsigned)plane_pixel(src, raw, 0, c.cols);
                if (res) *reinterpret_cast<float4*>(res + px) = make_float4(r[0], r[1], r[2], r[3]);
                if (uv) {
                    *reinterpret_cast<float4*>(uv + 2 * px) = make_float4(u[0], v[0], u[1], v[1]);
                    *reinterpret_cast<float4*>(uv + 2 * px + 4) = make_float4(u[2], v[2], u[3], v[3]);
                }
                continue;
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int px = plane_pixel(src, raw, g, c.cols);
            if ((unsigned)px >= plane) continue;  // no point (a lane past the end of a list)
            if (res) res[px] = r[g];
            if (uv) {
                if (wide) {
                    *reinterpret_cast<float2*>(uv + 2 * (unsigned)px) = make_float2(u[g], v[g]);
                } else {
                    uv[2 * (unsigned)px] = u[g];
                    uv[2 * (unsigned)px + 1] = v[g];
                }
            }
        }
    }
}
template <bool DENSE, bool HIST>
__global__ __launch_bounds__(RMAPS_BLOCK) void lm_residual_maps_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                       const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                       const uint16_t* __restrict__ kf_depth, Records rec, ResidualMapsArgs a) {
    __shared__ uint32_t lds_hist[HIST ? (RMAPS_BLOCK / 64) * VORS_RESIDUAL_BINS : 1];
    const int pair = a.pair0 + blockIdx.y, chunk = blockIdx.x, n_chunks = gridDim.x;
    const Iso model = iso_uniform(iso_load(a.models + (size_t)pair * a.model_stride));
    const ImgCtx c = level_ctx(g, cur0, curu, pair, a.lvl);
    const size_t plane = (size_t)c.rows * c.cols;
    float* res = a.residuals ? a.residuals + (size_t)pair * plane : nullptr;
    float* uv = a.warp_uv ? a.warp_uv + (size_t)pair * plane * 2 : nullptr;
    if constexpr (HIST) {
#pragma unroll
        for (int k = 0; k < RMAPS_BLOCK / 64; ++k) lds_hist[k * VORS_RESIDUAL_BINS + threadIdx.x] = 0;
        __syncthreads();
    }
    with_exact_source<DENSE, true>(g, a.lvl, pair, kf0, kfu, kf_depth, rec, [&](const auto& src, int n_units) {
        const int chunks = level_chunks(DENSE ? g.lv[a.lvl].n_slots : n_units, a.chunk_points, n_chunks);
        if (chunk >= chunks) return;
        const LevelCut cut = level_cut(n_units, chunk, chunks);
        residual_maps_sweep<HIST>(src, cut.first, cut.last, c, model, res, uv, a.wide_stores != 0, lds_hist + (threadIdx.x >> 6) * VORS_RESIDUAL_BINS);
    });
    if constexpr (HIST) {
        __syncthreads();
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < RMAPS_BLOCK / 64; ++k) n += lds_hist[k * VORS_RESIDUAL_BINS + threadIdx.x];
        if (n) atomicAdd(a.hist + (size_t)pair * VORS_RESIDUAL_BINS + threadIdx.x, n);
    }
}
static_assert(RMAPS_BLOCK == VORS_RESIDUAL_BINS, "one thread per bin clears and flushes the histogram");
// histogram -> (median |r|, 1.4826 median |r|) (lie.h residual_scale_from_hist), one thread per pair
__global__ __launch_bounds__(64) void residual_scale_kernel(const uint32_t* __restrict__ hist, int n, float* __restrict__ scale) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    residual_scale_from_hist(hist + (size_t)p * VORS_RESIDUAL_BINS, scale + 2 * (size_t)p, scale + 2 * (size_t)p + 1, nullptr);
}
void launch_lm_residual_maps(const Geom& g_in, const ResidualMapsCall& call, hipStream_t s) {
    const Geom g = launch_geom(g_in, call);
    const bool dense = g.mode == VORS_CANDIDATES_DENSE;
    const size_t plane = (size_t)g.lv[call.lvl].rows * g.lv[call.lvl].cols, n = (size_t)call.n_pairs;
    if (!dense) {  // the lists scatter their points into planes of NaN
        if (call.residuals) (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(call.residuals), 0x7fc00000, n * plane, s);
        if (call.warp_uv) (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(call.warp_uv), 0x7fc00000, n * plane * 2, s);
    }
    if (call.hist) (void)hipMemsetAsync(call.hist, 0, n * VORS_RESIDUAL_BINS * sizeof(uint32_t), s);
    ResidualMapsArgs a{0, call.lvl, eval_pairs_chunk_points(g), call.models, call.model_stride, call.residuals, call.warp_uv, call.hist,
                       (((uintptr_t)call.residuals | (uintptr_t)call.warp_uv) % 16 == 0) ? 1 : 0};
    const int chunks = eval_pairs_chunks(g, call.lvl);
    for_pair_slices(call.n_pairs, [&](int pair0, int np) {
        a.pair0 = pair0;
        with_bool(dense, [&](auto d) {
            with_bool(call.hist != nullptr, [&](auto h) {
                launch_on_scene(lm_residual_maps_kernel<decltype(d)::value, decltype(h)::value>, dim3(chunks, np), dim3(RMAPS_BLOCK), 0, s, g, call, a);
            });
        });
    });
    if (call.scale && call.hist) hipLaunchKernelGGL(residual_scale_kernel, dim3((call.n_pairs + 63) / 64), dim3(64), 0, s, call.hist, call.n_pairs, call.scale);
}

// ------------------------------------------------------------------------------------------------------------
// vors_batch_reproject_depth: the keyframe's points carried into the CURRENT frame — a forward warp with a z-buffer — and compared with
// a measured current depth map. Grid, cut of a level and sources are lm_residual_maps_kernel's; the loop is positions -> warp_point_z and
// nothing of the current image is read. A point lands at the pixel nearest to (u, v) when P'.z > 0 and that pixel is in the window (all
// compares in float: NaN and huge values fail them, and only a landing point's coordinates are ever converted to integers).
// Z-buffer: a positive float orders as its bit pattern, so the plane is kept as uint32 — filled with +inf (0x7f800000) by the launcher,
// one 32-bit global atomicMin per landing point. A minimum does not depend on the order of arrival: the plane is bitwise reproducible.
// Residual (level 0, needs the current depth): P'.z - cur_depth[q] / depth_scale in KEYFRAME geometry, stored like the residual maps
// (dense: the pass writes the NaN of a non-point itself; lists: scattered into a plane of NaN).
// Counts (COUNTS): per-thread integers through block_counts (device_common.h) into a zeroed array. Without COUNTS the kernel has no LDS.
// ------------------------------------------------------------------------------------------------------------
// warp (lm_optimizer.rs:213-219) as warp_point evaluates it — the same text, so (u, v) have the bits of d_warp_uv — plus the depth P'.z.
struct WarpedZ {
    float u, v, z;
};
__device__ __forceinline__ WarpedZ warp_point_z(const ImgCtx& c, const Iso& model, const Pos& p) {
    WarpedZ w;
    const V3 p2 = iso_transform_point(model, V3{p.X, p.Y, p.Z});
    project_uv(c.k, p2, &w.u, &w.v);
    w.z = p2.z;
    return w;
}
// The landing test of both splats (reprojection and fusion): the pixel nearest to (u, v), when the point is usable, in front of the
// camera and that pixel is in the window. Masked, not branched: a point that does not land addresses pixel 0 (a safe address) and is
// selected away. (fcols, frows: the window as floats, converted once by the caller — converted here, the dense kernels take more SGPRs.)
struct Landing {
    bool lands;
    unsigned q;
};
__device__ __forceinline__ Landing landing_pixel(const WarpedZ& w, bool usable, int cols, float fcols, float frows) {
    const float fu = floorf(w.u + 0.5f), fv = floorf(w.v + 0.5f);
    Landing l;
    l.lands = usable && (w.z > 0.f) && (fu >= 0.f) && (fu < fcols) && (fv >= 0.f) && (fv < frows);
    l.q = (unsigned)(__float2int_rz(l.lands ? fv : 0.f) * cols + __float2int_rz(l.lands ? fu : 0.f));
    return l;
}
// One byte per point of a unit from a byte plane in the level's pixel geometry (weights, keep masks), at the pixels px[] of its points
// (a lane past the end of a list is no point: the caller hands pixel 0): a unit of four — the dense quad source, four adjacent pixels
// of one row — reads them as one dword where the plane allows it (`wide`, uniform: 4-byte aligned), else G byte loads.
template <int G>
__device__ __forceinline__ void unit_bytes(const uint8_t* plane, bool wide, const unsigned (&px)[G], uint32_t (&out)[G]) {
    if constexpr (G == 4) {
        if (wide) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(plane + px[0]);
#pragma unroll
            for (int g = 0; g < G; ++g) out[g] = (w >> (8 * g)) & 0xffu;
            return;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) out[g] = plane[px[g]];
}
template <bool COUNTS, class Src>
__device__ __forceinline__ void reproject_sweep(const Src& src, int first, int last, const ImgCtx& c, const Iso& model, float depth_scale,
                                                uint32_t* zbuf, const uint16_t* cur_depth, float tol_m, float* res, bool wide, uint32_t n[4]) {
    constexpr int G = Src::G;
    const float nan = __builtin_nanf("");
    const unsigned plane = (unsigned)(c.rows * c.cols);
    const float fcols = (float)c.cols, frows = (float)c.rows;
    for (typename Src::Cursor cur = src.template begin<RMAPS_BLOCK>(first); cur.i < last; cur = src.template advance<RMAPS_BLOCK>(cur)) {
        typename Src::Raw raw;
        src.template fetch<RMAPS_BLOCK>(cur, last, raw);
        Pos pos[G];
        src.positions(raw, pos);
        WarpedZ w[G];
#pragma unroll
        for (int g = 0; g < G; ++g) w[g] = warp_point_z(c, model, pos[g]);
        bool usable[G], lands[G];
        unsigned q[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            usable[g] = pos[g].tmpl >= 0.f;
            const Landing l = landing_pixel(w[g], usable[g], c.cols, fcols, frows);
            lands[g] = l.lands;
            q[g] = l.q;
        }
        if (zbuf) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (lands[g]) atomicMin(zbuf + q[g], (uint32_t)__float_as_int(w[g].z));
        }
        float r[G];
        if (cur_depth) {  // (uniform) one 2-byte gather per point
            uint16_t d[G];
#pragma unroll
            for (int g = 0; g < G; ++g) d[g] = cur_depth[q[g]];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bool has = lands[g] && d[g] != 0;
                r[g] = has ? w[g].z - (float)d[g] / depth_scale : nan;
                if constexpr (COUNTS) {
                    n[2] += has ? 1u : 0u;
                    n[3] += (has && fabsf(r[g]) <= tol_m) ? 1u : 0u;
                }
            }
        }
        if constexpr (COUNTS) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                n[0] += usable[g] ? 1u : 0u;
                n[1] += lands[g] ? 1u : 0u;
            }
        }
        if (!res) continue;  // (uniform; res needs cur_depth: r is set)
        if constexpr (G == 4) {
            if (wide) {  // (uniform) a quad owns four adjacent pixels of one row, 16-byte aligned in the plane
                const unsigned px = (unsigned)plane_pixel(src, raw, 0, c.cols);
                *reinterpret_cast<float4*>(res + px) = make_float4(r[0], r[1], r[2], r[3]);
                continue;
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int px = plane_pixel(src, raw, g, c.cols);
            if ((unsigned)px >= plane) continue;  // no point (a lane past the end of a list)
            res[px] = r[g];
        }
    }
}
template <bool DENSE, bool COUNTS>
__global__ __launch_bounds__(RMAPS_BLOCK) void lm_reproject_depth_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                         const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                         const uint16_t* __restrict__ kf_depth, Records rec, ReprojectArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? (RMAPS_BLOCK / 64) * 4 : 1];
    const int pair = a.pair0 + blockIdx.y, chunk = blockIdx.x, n_chunks = gridDim.x;
    const Iso model = iso_uniform(iso_load(a.models + (size_t)pair * a.model_stride));
    ImgCtx c{};  // the level's window and intrinsics; the current image is never read (the pass is legal before any track_current)
    c.rows = g.lv[a.lvl].rows;
    c.cols = g.lv[a.lvl].cols;
    c.k = g.lv[a.lvl].k;
    const size_t plane = (size_t)c.rows * c.cols;
    uint32_t* zbuf = a.pred_z ? a.pred_z + (size_t)pair * plane : nullptr;
    const uint16_t* cur_depth = a.cur_depth ? a.cur_depth + (size_t)pair * g.S0 : nullptr;  // (level 0 only: plane == S0)
    float* res = a.residual ? a.residual + (size_t)pair * plane : nullptr;
    uint32_t n[4] = {0u, 0u, 0u, 0u};
    with_exact_source<DENSE, true>(g, a.lvl, pair, kf0, kfu, kf_depth, rec, [&](const auto& src, int n_units) {
        const int chunks = level_chunks(DENSE ? g.lv[a.lvl].n_slots : n_units, a.chunk_points, n_chunks);
        if (chunk >= chunks) return;
        const LevelCut cut = level_cut(n_units, chunk, chunks);
        reproject_sweep<COUNTS>(src, cut.first, cut.last, c, model, g.depth_scale, zbuf, cur_depth, a.tol_m, res, a.wide_stores != 0, n);
    });
    if constexpr (COUNTS) block_counts<4, RMAPS_BLOCK>(n, lds_counts, CountsAdd{a.counts + (size_t)pair * 4});
}
// z-buffer -> depth map: to_depth(depth_scale, 1 / z) (lie.h, inverse_depth.rs:37-42), 0 where nothing landed. Four pixels per thread
// (16-byte loads, 8-byte stores) where the planes allow it.
__global__ __launch_bounds__(256) void pred_depth_kernel(const float* __restrict__ z, size_t n, float depth_scale, uint16_t* __restrict__ out, int wide) {
    const float inf = __builtin_inff();
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, step = (size_t)gridDim.x * 256;
    const size_t n4 = wide ? n / 4 : 0;
    for (size_t i = t; i < n4; i += step) {
        const float4 zz = reinterpret_cast<const float4*>(z)[i];
        ushort4 d;
        d.x = zz.x == inf ? (uint16_t)0 : to_depth(depth_scale, 1.0f / zz.x);
        d.y = zz.y == inf ? (uint16_t)0 : to_depth(depth_scale, 1.0f / zz.y);
        d.z = zz.z == inf ? (uint16_t)0 : to_depth(depth_scale, 1.0f / zz.z);
        d.w = zz.w == inf ? (uint16_t)0 : to_depth(depth_scale, 1.0f / zz.w);
        reinterpret_cast<ushort4*>(out)[i] = d;
    }
    for (size_t i = 4 * n4 + t; i < n; i += step) out[i] = z[i] == inf ? (uint16_t)0 : to_depth(depth_scale, 1.0f / z[i]);
}
void launch_lm_reproject_depth(const Geom& g_in, const ReprojectCall& call, hipStream_t s) {
    const Geom g = launch_geom(g_in, call);
    const bool dense = g.mode == VORS_CANDIDATES_DENSE;
    const size_t plane = (size_t)g.lv[call.lvl].rows * g.lv[call.lvl].cols, n = (size_t)call.n_pairs;
    if (call.pred_z) (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(call.pred_z), 0x7f800000, n * plane, s);  // +inf: nothing has landed
    if (call.residual && !dense) (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(call.residual), 0x7fc00000, n * plane, s);
    if (call.counts) (void)hipMemsetAsync(call.counts, 0, n * 4 * sizeof(uint32_t), s);
    ReprojectArgs a{0, call.lvl, eval_pairs_chunk_points(g), call.models, call.model_stride, call.cur_depth, call.tol_m,
                    reinterpret_cast<uint32_t*>(call.pred_z), call.residual, call.counts, ((uintptr_t)call.residual % 16 == 0) ? 1 : 0};
    const int chunks = eval_pairs_chunks(g, call.lvl);
    for_pair_slices(call.n_pairs, [&](int pair0, int np) {
        a.pair0 = pair0;
        with_bool(dense, [&](auto d) {
            with_bool(call.counts != nullptr, [&](auto k) {
                launch_on_scene(lm_reproject_depth_kernel<decltype(d)::value, decltype(k)::value>, dim3(chunks, np), dim3(RMAPS_BLOCK), 0, s, g, call, a);
            });
        });
    });
    if (call.pred_depth && call.pred_z) {
        const size_t total = n * plane;
        const int wide = (((uintptr_t)call.pred_z % 16 == 0) && ((uintptr_t)call.pred_depth % 8 == 0)) ? 1 : 0;
        const size_t blocks = std::min<size_t>((total / 4 + 255) / 256 + 1, 8192);
        hipLaunchKernelGGL(pred_depth_kernel, dim3((unsigned)blocks), dim3(256), 0, s, call.pred_z, total, g.depth_scale, call.pred_depth, wide);
    }
}

// ------------------------------------------------------------------------------------------------------------
// vors_batch_fuse_depth: level 0 of the keyframe splatted into the CURRENT frame through a KEYED z-buffer, then merged per current pixel
// with the measured depth. Two launches ordered by the stream. Each pass has ONE body; its kernels are entry points that find the pair —
// index blockIdx.y of a slice of the whole batch, or of the promotion list (the depth filter, below) — and say whether planes may be null.
// SPLAT (fuse_splat_body): lm_reproject_depth_kernel's grid, cut and sources; the sweep is reproject_sweep's up to the landing test
// (landing_pixel). Then one weight byte at the SOURCE pixel (unit_bytes; no plane: weight 1) and, per landing point of non-zero weight,
// one 64-bit global atomicMin of bits(Z') << 32 | src into a plane filled with ones. Z' > 0 orders as its bits, so the nearest surface
// wins and among equal Z' the smallest source index: a minimum, bitwise reproducible whatever the order of arrival. No LDS.
// MERGE (fuse_merge_body): elementwise over current pixels, 1024 per workgroup: lie.h fuse_depth_pixel on (key, weight gathered at src,
// measured depth). Four adjacent pixels per thread where every plane allows it (two 16-byte key loads, one 8-byte depth load, an 8-byte
// and a 4-byte store), else four pixels a workgroup width apart. Counts (COUNTS) follow the reprojection pass (block_counts into a zeroed
// array). Without COUNTS the kernel has no LDS and no atomic.
// ------------------------------------------------------------------------------------------------------------
template <class Src>
__device__ __forceinline__ void fuse_splat_sweep(const Src& src, int first, int last, const ImgCtx& c, const Iso& model, const uint8_t* kf_weight,
                                                 bool wide_weight, unsigned long long* zkey) {
    constexpr int G = Src::G;
    const float fcols = (float)c.cols, frows = (float)c.rows;
    for (typename Src::Cursor cur = src.template begin<RMAPS_BLOCK>(first); cur.i < last; cur = src.template advance<RMAPS_BLOCK>(cur)) {
        typename Src::Raw raw;
        src.template fetch<RMAPS_BLOCK>(cur, last, raw);
        Pos pos[G];
        src.positions(raw, pos);
        WarpedZ w[G];
#pragma unroll
        for (int g = 0; g < G; ++g) w[g] = warp_point_z(c, model, pos[g]);
        Landing l[G];
        unsigned from[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            l[g] = landing_pixel(w[g], pos[g].tmpl >= 0.f, c.cols, fcols, frows);
            from[g] = (unsigned)max(plane_pixel(src, raw, g, c.cols), 0);  // (a lane past the end of a list is no point: pixel 0, selected away)
        }
        uint32_t wb[G];
#pragma unroll
        for (int g = 0; g < G; ++g) wb[g] = 1;
        if (kf_weight) unit_bytes(kf_weight, wide_weight, from, wb);  // (uniform)
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (l[g].lands && wb[g] != 0)
                atomicMin(zkey + l[g].q, ((unsigned long long)(uint32_t)__float_as_int(w[g].z) << 32) | (unsigned long long)from[g]);
    }
}
// OPTIONAL_PLANES: a null kf_weight stands for weight 1 everywhere; without it the plane is required and no null test is kept.
template <bool DENSE, bool OPTIONAL_PLANES>
__device__ __forceinline__ void fuse_splat_body(const Geom& g, int pair, const uint8_t* kf0, const uint8_t* kfu, const uint16_t* kf_depth,
                                                const Records& rec, const FuseSplatArgs& a) {
    const int chunk = blockIdx.x, n_chunks = gridDim.x;
    const Iso model = iso_uniform(iso_load(a.models + (size_t)pair * a.model_stride));
    ImgCtx c{};  // level 0's window and intrinsics; the current image is never read (the pass is legal before any track_current)
    c.rows = g.lv[0].rows;
    c.cols = g.lv[0].cols;
    c.k = g.lv[0].k;
    const uint8_t* kf_weight = (!OPTIONAL_PLANES || a.kf_weight) ? a.kf_weight + (size_t)pair * g.S0 : nullptr;
    unsigned long long* zkey = a.zkey + (size_t)pair * g.S0;
    with_exact_source<DENSE, true>(g, 0, pair, kf0, kfu, kf_depth, rec, [&](const auto& src, int n_units) {
        const int chunks = level_chunks(DENSE ? g.lv[0].n_slots : n_units, a.chunk_points, n_chunks);
        if (chunk >= chunks) return;
        const LevelCut cut = level_cut(n_units, chunk, chunks);
        fuse_splat_sweep(src, cut.first, cut.last, c, model, kf_weight, a.wide_weight != 0, zkey);
    });
}
template <bool DENSE>
__global__ __launch_bounds__(RMAPS_BLOCK) void lm_fuse_splat_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                    const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                    const uint16_t* __restrict__ kf_depth, Records rec, FuseSplatArgs a) {
    fuse_splat_body<DENSE, true>(g, a.pair0 + blockIdx.y, kf0, kfu, kf_depth, rec, a);
}
#define FUSE_BLOCK 256
#define FUSE_PIXELS 4  // per thread
// OPTIONAL_PLANES: kf_weight and the two outputs may be null; without it all planes are required and no null test is kept.
template <bool COUNTS, bool OPTIONAL_PLANES>
__device__ __forceinline__ void fuse_merge_body(int pair, const FuseMergeArgs& a, uint32_t* lds_counts) {
    const size_t off = (size_t)pair * (size_t)a.plane;
    const uint64_t* zkey = a.zkey + off;
    const uint16_t* cur_depth = a.cur_depth + off;
    const uint8_t* kf_weight = (!OPTIONAL_PLANES || a.kf_weight) ? a.kf_weight + off : nullptr;
    uint16_t* fused_depth = (!OPTIONAL_PLANES || a.fused_depth) ? a.fused_depth + off : nullptr;
    uint8_t* fused_weight = (!OPTIONAL_PLANES || a.fused_weight) ? a.fused_weight + off : nullptr;
    const int base = blockIdx.x * (FUSE_BLOCK * FUSE_PIXELS);
    uint32_t n[VORS_FUSE_COUNTS] = {0u, 0u, 0u, 0u, 0u, 0u};
    FusedPixel o[FUSE_PIXELS];
    if (a.wide) {  // (uniform; plane % 4 == 0: a thread's four pixels are all inside or all outside)
        const int i = base + FUSE_PIXELS * (int)threadIdx.x;
        if (i < a.plane) {
            const ulonglong2 k01 = *reinterpret_cast<const ulonglong2*>(zkey + i), k23 = *reinterpret_cast<const ulonglong2*>(zkey + i + 2);
            const ushort4 d = *reinterpret_cast<const ushort4*>(cur_depth + i);
            o[0] = fuse_depth_pixel(a.depth_scale, a.tol_m, a.max_weight, a.fill_min_weight, k01.x, kf_weight, d.x);
            o[1] = fuse_depth_pixel(a.depth_scale, a.tol_m, a.max_weight, a.fill_min_weight, k01.y, kf_weight, d.y);
            o[2] = fuse_depth_pixel(a.depth_scale, a.tol_m, a.max_weight, a.fill_min_weight, k23.x, kf_weight, d.z);
            o[3] = fuse_depth_pixel(a.depth_scale, a.tol_m, a.max_weight, a.fill_min_weight, k23.y, kf_weight, d.w);
            if (!OPTIONAL_PLANES || fused_depth) *reinterpret_cast<ushort4*>(fused_depth + i) = make_ushort4(o[0].depth, o[1].depth, o[2].depth, o[3].depth);
            if (!OPTIONAL_PLANES || fused_weight)
                *reinterpret_cast<uint32_t*>(fused_weight + i) =
                    (uint32_t)o[0].weight | ((uint32_t)o[1].weight << 8) | ((uint32_t)o[2].weight << 16) | ((uint32_t)o[3].weight << 24);
            if constexpr (COUNTS) {
#pragma unroll
                for (int j = 0; j < FUSE_PIXELS; ++j)
#pragma unroll
                    for (int k = 0; k < VORS_FUSE_COUNTS; ++k) n[k] += o[j].kase == k ? 1u : 0u;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < FUSE_PIXELS; ++j) {
            const int i = base + j * FUSE_BLOCK + (int)threadIdx.x;
            if (i >= a.plane) continue;
            o[j] = fuse_depth_pixel(a.depth_scale, a.tol_m, a.max_weight, a.fill_min_weight, zkey[i], kf_weight, cur_depth[i]);
            if (!OPTIONAL_PLANES || fused_depth) fused_depth[i] = o[j].depth;
            if (!OPTIONAL_PLANES || fused_weight) fused_weight[i] = o[j].weight;
            if constexpr (COUNTS) {
#pragma unroll
                for (int k = 0; k < VORS_FUSE_COUNTS; ++k) n[k] += o[j].kase == k ? 1u : 0u;
            }
        }
    }
    if constexpr (COUNTS) block_counts<VORS_FUSE_COUNTS, FUSE_BLOCK>(n, lds_counts, CountsAdd{a.counts + (size_t)pair * VORS_FUSE_COUNTS});
}
template <bool COUNTS>
__global__ __launch_bounds__(FUSE_BLOCK) void fuse_depth_kernel(FuseMergeArgs a) {
    __shared__ uint32_t lds_counts[COUNTS ? (FUSE_BLOCK / 64) * VORS_FUSE_COUNTS : 1];
    fuse_merge_body<COUNTS, true>(a.pair0 + blockIdx.y, a, lds_counts);
}
// What both launchers hand their kernels: the splat's and the merge's arguments (pair0 = 0) and the rule for the wide forms.
static void fuse_depth_args(const Geom& g, const FuseDepthCall& call, uint32_t* counts, FuseSplatArgs* a, FuseMergeArgs* m) {
    const size_t plane = (size_t)g.S0;
    *a = FuseSplatArgs{0, eval_pairs_chunk_points(g), call.models, call.model_stride, call.kf_weight, reinterpret_cast<unsigned long long*>(call.zkey),
                       ((uintptr_t)call.kf_weight % 4 == 0 && plane % 4 == 0) ? 1 : 0};
    const bool wide = plane % 4 == 0 && (uintptr_t)call.zkey % 16 == 0 && (uintptr_t)call.cur_depth % 8 == 0 && (uintptr_t)call.fused_depth % 8 == 0 &&
                      (uintptr_t)call.fused_weight % 4 == 0;
    *m = FuseMergeArgs{0, (int)plane, g.depth_scale, call.tol_m, call.max_weight, call.fill_min_weight, call.zkey, call.cur_depth, call.kf_weight,
                       call.fused_depth, call.fused_weight, counts, wide ? 1 : 0};
}
static unsigned fuse_merge_blocks(const Geom& g) { return (unsigned)(((size_t)g.S0 + FUSE_BLOCK * FUSE_PIXELS - 1) / (FUSE_BLOCK * FUSE_PIXELS)); }
void launch_lm_fuse_depth(const Geom& g_in, const FuseDepthCall& call, hipStream_t s) {
    const Geom g = launch_geom(g_in, call);
    const bool dense = g.mode == VORS_CANDIDATES_DENSE;
    const size_t plane = (size_t)g.S0, n = (size_t)call.n_pairs;
    // all ones = VORS_ZKEY_EMPTY: nothing has landed (a 32-bit fill over twice as many dwords)
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(call.zkey), 0xFFFFFFFF, 2 * n * plane, s);
    if (call.counts) (void)hipMemsetAsync(call.counts, 0, n * VORS_FUSE_COUNTS * sizeof(uint32_t), s);
    FuseSplatArgs a;
    FuseMergeArgs m;
    fuse_depth_args(g, call, call.counts, &a, &m);
    const bool merge = call.fused_depth || call.fused_weight || call.counts;
    const int chunks = eval_pairs_chunks(g, 0);
    for_pair_slices(call.n_pairs, [&](int pair0, int np) {
        a.pair0 = m.pair0 = pair0;
        with_bool(dense, [&](auto d) {
            launch_on_scene(lm_fuse_splat_kernel<decltype(d)::value>, dim3(chunks, np), dim3(RMAPS_BLOCK), 0, s, g, call, a);
        });
        if (merge)
            with_bool(call.counts != nullptr, [&](auto k) {
                hipLaunchKernelGGL(fuse_depth_kernel<decltype(k)::value>, dim3(fuse_merge_blocks(g), np), dim3(FUSE_BLOCK), 0, s, m);
            });
    });
}

// ------------------------------------------------------------------------------------------------------------
// The depth filter of the lock-step trackers (vors_trackers_enable_depth_filter): the pass above as MASKED launches over the promotion
// list (Geom::sel_list) — index k of the pair dimension is sequence select_pair(g, k), a workgroup beyond the selection returns at once.
// The host does not know how many sequences promote, so the grids are sized for all of them. What the masked form adds to the bodies
// above is select_pair in front and a fill of its own; every plane is required and nothing is counted, so SPLAT and MERGE keep no null
// test, no LDS and, the splat's minimum apart, no atomic. The model is the head of the sequence's vors_pair_stats.
// FILL (fuse_fill_selected_kernel): the key planes of the selected sequences to VORS_ZKEY_EMPTY, two keys (16 bytes) per thread.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fuse_fill_selected_kernel(Geom g, unsigned long long* __restrict__ zkey, int vec) {
    const int pair = select_pair(g, blockIdx.y);
    if (pair < 0) return;
    unsigned long long* p = zkey + (size_t)pair * g.S0;
    const int i = 2 * (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= g.S0) return;
    if (vec && i + 2 <= g.S0) {  // (vec: S0 is even, every sequence's plane starts 16-byte aligned)
        *reinterpret_cast<uint4*>(p + i) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    } else {
        p[i] = 0xFFFFFFFFFFFFFFFFull;
        if (i + 1 < g.S0) p[i + 1] = 0xFFFFFFFFFFFFFFFFull;
    }
}
template <bool DENSE>
__global__ __launch_bounds__(RMAPS_BLOCK) void lm_fuse_splat_selected_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                             const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                             const uint16_t* __restrict__ kf_depth, Records rec, FuseSplatArgs a) {
    const int pair = select_pair(g, blockIdx.y);
    if (pair < 0) return;
    fuse_splat_body<DENSE, false>(g, pair, kf0, kfu, kf_depth, rec, a);
}
__global__ __launch_bounds__(FUSE_BLOCK) void fuse_depth_selected_kernel(Geom g, FuseMergeArgs a) {
    const int pair = select_pair(g, blockIdx.y);
    if (pair < 0) return;
    fuse_merge_body<false, false>(pair, a, nullptr);
}
// call.n_pairs: the sequences of the handle (the extent of the pair dimension); g_in.sel_list / sel_count: the ones that take part.
// models, cur_depth, kf_weight, zkey, fused_depth and fused_weight are all required; counts is not written.
void launch_lm_fuse_depth_selected(const Geom& g_in, const FuseDepthCall& call, hipStream_t s) {
    const Geom g = launch_geom(g_in, call);
    const bool dense = g.mode == VORS_CANDIDATES_DENSE;
    const size_t plane = (size_t)g.S0;
    const int n = call.n_pairs;
    FuseSplatArgs a;
    FuseMergeArgs m;
    fuse_depth_args(g, call, nullptr, &a, &m);
    hipLaunchKernelGGL(fuse_fill_selected_kernel, dim3((unsigned)((plane + 511) / 512), n), dim3(256), 0, s, g, a.zkey,
                       (plane % 2 == 0 && (uintptr_t)call.zkey % 16 == 0) ? 1 : 0);
    with_bool(dense, [&](auto d) {
        launch_on_scene(lm_fuse_splat_selected_kernel<decltype(d)::value>, dim3(eval_pairs_chunks(g, 0), n), dim3(RMAPS_BLOCK), 0, s, g, call, a);
    });
    hipLaunchKernelGGL(fuse_depth_selected_kernel, dim3(fuse_merge_blocks(g), n), dim3(FUSE_BLOCK), 0, s, g, m);
}

// ------------------------------------------------------------------------------------------------------------
// vors_batch_point_cloud: the usable points of a level as a LIST per pair — an ordered, deterministic stream compaction — back-projected
// (the Pos the LM kernels warp from, camera.rs:135-140) and carried to the world frame by one pose per pair (iso_transform_point). Grid,
// cut of a level and sources are lm_residual_maps_kernel's. Rank order is ascending SLOT order of the level's source: the dense sources
// give a thread one unit of G adjacent pixels (slots G i .. G i + G - 1 of unit i = first + k BLOCK + t in iteration k), the candidate
// lists give it the slots i and i + BLOCK (i = first + 2 k BLOCK + t) — two interleaved runs, ranked one after the other.
// Two launches, ordered by the stream alone (no workgroup ever waits for another, no atomic anywhere):
//   COUNT  every workgroup STORES the number of kept points of its chunk to ws[pair][chunk] (0 for a chunk the pair does not use);
//   WRITE  every workgroup adds up the counts of the chunks before its own (a uniform loop over at most a few dozen integers; chunk 0
//          also stores the total to d_counts), then repeats the sweep with the loop made UNIFORM over the workgroup — a lane past the end
//          holds no point — and ranks: ballots of the G flags + mbcnt for the wavefront prefix, the four wavefront totals through LDS
//          (two slots used in turn: one barrier per scan), a running base across the iterations. Points of rank < capacity are stored; a
//          workgroup whose base has reached the capacity stops.
// With d_counts alone, COUNT and a one-thread-per-pair sum.
// ------------------------------------------------------------------------------------------------------------
#define PCLOUD_WAVES (RMAPS_BLOCK / 64)
template <bool LEVEL0>
__device__ __forceinline__ uint32_t cloud_xy(const DenseSrc<LEVEL0>&, const typename DenseSrc<LEVEL0>::Raw& r, int) {
    return (uint32_t)r.x | ((uint32_t)r.y << 16);
}
template <bool LEVEL0, bool FAST>
__device__ __forceinline__ uint32_t cloud_xy(const DenseQuadSrc<LEVEL0, FAST>&, const typename DenseQuadSrc<LEVEL0, FAST>::Raw& r, int g) {
    return (uint32_t)(r.x0 + g) | ((uint32_t)r.y << 16);
}
__device__ __forceinline__ uint32_t cloud_xy(const SlimSrc&, const SlimSrc::Raw& r, int g) { return r.r[g].xy; }
// The points of one unit: kept = usable (extract_z's set) and not masked away. A cursor past `last` holds none (and loads nothing).
template <int G>
struct CloudPts {
    V3 P[G];
    uint32_t xy[G];
    float tmpl[G];
    bool kept[G];
    uint32_t entry[G];  // VOX_OWNED_RANK only: the table entry of a kept point's voxel
};
// The voxel table of ONE sequence as the sweeps of its filtered emission see it (point_cloud_append_voxel_kernel, below), CloudVox, and
// its probes voxel_claim / voxel_owns: voxel_table_device.h, the text the filter of plain point lists (repose_kernels.hip) shares.
enum { VOX_OFF = 0, VOX_CLAIM = 1, VOX_OWNED = 2, VOX_OWNED_RANK = 3, VOX_ACCUM = 4 };
// What the two sweeps of the voxel statistics (vors_trackers_enable_map_voxel_stats; point_cloud_append_voxel_stats_kernel) see besides:
// the sequence's rank words, sums and observation records, its list of first points, and the segment index of the keyframe being emitted.
struct CloudVoxStats : CloudVox {
    uint32_t* rank_of;         // [table_slots]
    unsigned long long* sums;  // [capacity][4], two's complement
    uint32_t* obs;             // [capacity][2]
    const float* xyz;          // [capacity][3] the sequence's list
    uint32_t capacity;
    uint32_t segment;
};
#define VOXEL_NO_ENTRY 0xFFFFFFFFu
// voxel_owns' probe, which says WHERE: the entry that holds `key`; VOXEL_NO_ENTRY when none does, the point has no key or the sequence
// has overflowed. Reading only, and it gives up on the overflow word exactly as voxel_owns does.
__device__ __forceinline__ uint32_t voxel_find(const CloudVox& v, unsigned long long key) {
    if (key == VOXEL_EMPTY) return VOXEL_NO_ENTRY;
    uint32_t e = voxel_hash(key) & v.mask;
    for (uint32_t step = 0; step <= v.mask; ++step, e = (e + 1u) & v.mask) {
        if ((step & 63u) == 0u && voxel_overflowed(v)) return VOXEL_NO_ENTRY;
        const unsigned long long k = v.table[2 * (size_t)e];
        if (k == key) return e;
        if (k == VOXEL_EMPTY) return VOXEL_NO_ENTRY;
    }
    return VOXEL_NO_ENTRY;
}
// ACCUMULATE: one observation w (the world point WRITE would store) of grey `gray` into the statistics of its voxel, if the voxel has a
// rank below the capacity. `f`, the list entry at that rank, is final: the WRITE of this or an earlier emission stored it. Integer
// atomics only — three 64-bit additions of lie.h voxel_offset_q, one of the grey, a 32-bit addition and a 32-bit maximum —, so the
// result has the same bits whatever the order of arrival. No thread waits for another.
__device__ __forceinline__ void voxel_accumulate(const CloudVoxStats& v, unsigned long long key, const V3& w, uint32_t gray) {
    const uint32_t e = voxel_find(v, key);
    if (e == VOXEL_NO_ENTRY) return;
    const uint32_t r = v.rank_of[e];
    if (r >= v.capacity) return;  // (all ones included: a voxel without a stored first point accumulates nothing)
    const float* f = v.xyz + 3 * (size_t)r;
    unsigned long long* s = v.sums + 4 * (size_t)r;
    atomicAdd(s + 0, (unsigned long long)voxel_offset_q(v.voxel_m, w.x, f[0]));
    atomicAdd(s + 1, (unsigned long long)voxel_offset_q(v.voxel_m, w.y, f[1]));
    atomicAdd(s + 2, (unsigned long long)voxel_offset_q(v.voxel_m, w.z, f[2]));
    atomicAdd(s + 3, (unsigned long long)gray);
    atomicAdd(v.obs + 2 * (size_t)r, 1u);
    atomicMax(v.obs + 2 * (size_t)r + 1, v.segment);
}
// THRESH (the keyframe map of the trackers, point_cloud_append_kernel): the plane holds weights and a point is kept from `keep_min` on.
// VOX (its voxel filter): after the keep rule, VOX_CLAIM enters every kept point into the table and leaves the flags alone, VOX_OWNED
// keeps a point iff it owns its voxel (VOX_OWNED_RANK: and notes the entry), VOX_ACCUM adds every kept point to the statistics of its
// voxel and leaves the flags alone. Slot of point g of a unit: the candidate lists' i and i + BLOCK, the dense sources' G i + g.
template <bool THRESH, int VOX, class Src>
__device__ __forceinline__ void cloud_fetch(const Src& src, const typename Src::Cursor& cur, int last, int cols, const uint8_t* keep, bool wide_keep,
                                            CloudPts<Src::G>& o, uint32_t keep_min, const CloudVox* vox) {
    constexpr int G = Src::G;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        o.P[g] = V3{0.f, 0.f, 0.f};
        o.xy[g] = 0;
        o.tmpl[g] = -1.f;
        o.kept[g] = false;
    }
    if (cur.i >= last) return;
    typename Src::Raw raw;
    src.template fetch<RMAPS_BLOCK>(cur, last, raw);
    Pos pos[G];
    src.positions(raw, pos);
    uint32_t kb[G];
#pragma unroll
    for (int g = 0; g < G; ++g) kb[g] = 1;
    if (keep) {  // (uniform)
        unsigned px[G];
#pragma unroll
        for (int g = 0; g < G; ++g) px[g] = G == 4 ? (unsigned)plane_pixel(src, raw, g, cols) : (unsigned)max(plane_pixel(src, raw, g, cols), 0);  // (no clamp for a quad: it always holds four pixels, and the clamp costs its kernels VGPRs)
        unit_bytes(keep, wide_keep, px, kb);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        o.P[g] = V3{pos[g].X, pos[g].Y, pos[g].Z};
        o.xy[g] = cloud_xy(src, raw, g);
        o.tmpl[g] = pos[g].tmpl;
        if constexpr (THRESH) o.kept[g] = pos[g].tmpl >= 0.f && kb[g] >= keep_min;
        else o.kept[g] = pos[g].tmpl >= 0.f && kb[g] != 0;
    }
    if constexpr (VOX != VOX_OFF) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (!o.kept[g]) continue;
            const uint32_t slot = G == 2 ? (uint32_t)(cur.i + g * RMAPS_BLOCK) : (uint32_t)(G * cur.i + g);
            const V3 w = iso_transform_point(vox->pose, o.P[g]);  // (cloud_store's expression: the bits the list holds)
            const unsigned long long key = voxel_key(vox->voxel_m, w.x, w.y, w.z);
            if constexpr (VOX == VOX_CLAIM) voxel_claim(*vox, key, vox->tag_hi | slot);
            else if constexpr (VOX == VOX_ACCUM) voxel_accumulate(*static_cast<const CloudVoxStats*>(vox), key, w, (uint32_t)(uint8_t)(int)o.tmpl[g]);
            else if constexpr (VOX == VOX_OWNED_RANK) {
                o.entry[g] = voxel_find(*vox, key);
                o.kept[g] = o.entry[g] != VOXEL_NO_ENTRY && vox->table[2 * (size_t)o.entry[g] + 1] == (vox->tag_hi | slot);
            } else o.kept[g] = voxel_owns(*vox, key, vox->tag_hi | slot);
        }
    }
}
template <bool THRESH, int VOX, class Src>
__device__ __forceinline__ uint32_t cloud_count_sweep(const Src& src, int first, int last, int cols, const uint8_t* keep, bool wide_keep,
                                                      uint32_t keep_min, const CloudVox* vox) {
    constexpr int G = Src::G;
    uint32_t n = 0;
    for (typename Src::Cursor cur = src.template begin<RMAPS_BLOCK>(first); cur.i < last; cur = src.template advance<RMAPS_BLOCK>(cur)) {
        CloudPts<G> pts;
        cloud_fetch<THRESH, VOX>(src, cur, last, cols, keep, wide_keep, pts, keep_min, vox);
#pragma unroll
        for (int g = 0; g < G; ++g) n += pts.kept[g] ? 1u : 0u;
    }
    return n;
}
// Number of set flags before this thread's first one, over the workgroup in thread order (thread t's N flags are adjacent), and the
// workgroup's total. Every thread of the workgroup calls it; `par` alternates between calls (the LDS slot in use).
template <int N>
__device__ __forceinline__ uint32_t cloud_block_rank(const bool* f, uint32_t* lds, int par, uint32_t* total) {
    uint32_t pre = 0, wt = 0;
#pragma unroll
    for (int g = 0; g < N; ++g) {
        const unsigned long long m = __ballot(f[g]);
        pre += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        wt += (uint32_t)__popcll(m);
    }
    const int wave = threadIdx.x >> 6;
    uint32_t* slot = lds + par * PCLOUD_WAVES;
    if ((threadIdx.x & 63) == 0) slot[wave] = wt;
    __syncthreads();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < PCLOUD_WAVES; ++w) {
        const uint32_t c = slot[w];
        pre += w < wave ? c : 0u;
        t += c;
    }
    *total = t;
    return pre;
}
struct CloudOut {
    Iso pose;
    bool has_pose;
    uint32_t capacity;
    float* xyz;
    uint32_t* pixel;
    uint8_t* gray;
};
__device__ __forceinline__ void cloud_store(const CloudOut& o, uint32_t rank, const V3& P, uint32_t xy, float tmpl) {
    if (o.xyz) {  // (uniform) rows of 12 bytes: three dword stores, consecutive ranks are consecutive addresses
        const V3 w = o.has_pose ? iso_transform_point(o.pose, P) : P;
        float* x = o.xyz + 3 * (size_t)rank;
        x[0] = w.x;
        x[1] = w.y;
        x[2] = w.z;
    }
    if (o.pixel) o.pixel[rank] = xy;
    if (o.gray) o.gray[rank] = (uint8_t)(int)tmpl;
}
template <bool THRESH, int VOX, class Src>
__device__ __forceinline__ void cloud_write_sweep(const Src& src, int first, int last, int cols, const uint8_t* keep, bool wide_keep, uint32_t base,
                                                  const CloudOut& out, uint32_t* lds, uint32_t keep_min, const CloudVox* vox) {
    constexpr int G = Src::G;
    static_assert(G != 2 || std::is_same<Src, SlimSrc>::value, "G = 2 is the candidate lists' interleaved pair of slots");
    int par = 0;
    for (typename Src::Cursor cur = src.template begin<RMAPS_BLOCK>(first);
         __builtin_amdgcn_readfirstlane(cur.i - (int)threadIdx.x) < last && base < out.capacity; cur = src.template advance<RMAPS_BLOCK>(cur)) {
        CloudPts<G> pts;
        cloud_fetch<THRESH, VOX>(src, cur, last, cols, keep, wide_keep, pts, keep_min, vox);
        if constexpr (G == 2) {  // slots i and i + BLOCK: the first points of all threads come before the second ones
#pragma unroll
            for (int g = 0; g < G; ++g) {
                uint32_t total;
                const uint32_t rank = base + cloud_block_rank<1>(&pts.kept[g], lds, par, &total);
                par ^= 1;
                if (pts.kept[g] && rank < out.capacity) cloud_store(out, rank, pts.P[g], pts.xy[g], pts.tmpl[g]);
                if constexpr (VOX == VOX_OWNED_RANK)
                    if (pts.kept[g]) static_cast<const CloudVoxStats*>(vox)->rank_of[pts.entry[g]] = rank;
                base += total;
            }
        } else {
            uint32_t total;
            uint32_t rank = base + cloud_block_rank<G>(pts.kept, lds, par, &total);
            par ^= 1;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (pts.kept[g] && rank < out.capacity) cloud_store(out, rank, pts.P[g], pts.xy[g], pts.tmpl[g]);
                if constexpr (VOX == VOX_OWNED_RANK)
                    if (pts.kept[g]) static_cast<const CloudVoxStats*>(vox)->rank_of[pts.entry[g]] = rank;
                rank += pts.kept[g] ? 1u : 0u;
            }
            base += total;
        }
    }
}
// The pass of one workgroup, whoever launched it: the sweep over its chunk of the level — WRITE from `base` into `out`, else the count
// STORED to ws[chunk] (VOX_CLAIM, VOX_ACCUM: nothing is counted) — under the keep rule THRESH and the voxel rule VOX (cloud_fetch). The kernels below
// are its entry points: they find the pair, the planes and, for WRITE, the base and the lists. `ws` is the pair's row of the workspace.
template <bool DENSE, bool WRITE, bool THRESH, int VOX>
__device__ __forceinline__ void point_cloud_body(const Geom& g, int pair, const uint8_t* kf0, const uint8_t* kfu, const uint16_t* kf_depth,
                                                 const Records& rec, int lvl, int chunk_points, const uint8_t* keep, bool wide_keep,
                                                 uint32_t keep_min, uint32_t* ws, uint32_t base, const CloudOut& out, const CloudVox* vox,
                                                 uint32_t* lds) {
    const int chunk = blockIdx.x, n_chunks = gridDim.x;
    const int cols = g.lv[lvl].cols;
    uint32_t n[1] = {0u};
    with_exact_source<DENSE, true>(g, lvl, pair, kf0, kfu, kf_depth, rec, [&](const auto& src, int n_units) {
        const int chunks = level_chunks(DENSE ? g.lv[lvl].n_slots : n_units, chunk_points, n_chunks);
        if (chunk >= chunks) return;
        const LevelCut cut = level_cut(n_units, chunk, chunks);
        if constexpr (WRITE) cloud_write_sweep<THRESH, VOX>(src, cut.first, cut.last, cols, keep, wide_keep, base, out, lds, keep_min, vox);
        else n[0] = cloud_count_sweep<THRESH, VOX>(src, cut.first, cut.last, cols, keep, wide_keep, keep_min, vox);
    });
    if constexpr (!WRITE && VOX != VOX_CLAIM && VOX != VOX_ACCUM) block_counts<1, RMAPS_BLOCK>(n, lds, CountsStore{ws + chunk});
}
template <bool DENSE, bool WRITE>
__global__ __launch_bounds__(RMAPS_BLOCK) void point_cloud_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                  const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                  const uint16_t* __restrict__ kf_depth, Records rec, PointCloudArgs a) {
    __shared__ uint32_t lds[2 * PCLOUD_WAVES];
    const int pair = a.pair0 + blockIdx.y, chunk = blockIdx.x, n_chunks = gridDim.x;
    const size_t plane = (size_t)g.lv[a.lvl].rows * g.lv[a.lvl].cols;
    const uint8_t* keep = a.keep ? a.keep + (size_t)pair * plane : nullptr;
    uint32_t* ws = a.ws + (size_t)pair * a.ws_chunks;
    uint32_t base = 0;
    CloudOut out{};
    if constexpr (WRITE) {  // the whole-batch base: the counts of the chunks before this one
        uint32_t total = 0;
        for (int k = 0; k < n_chunks; ++k) {  // (uniform)
            const uint32_t c = ws[k];
            base += k < chunk ? c : 0u;
            total += c;
        }
        if (chunk == 0 && threadIdx.x == 0 && a.counts) a.counts[pair] = total;
        out.has_pose = a.poses != nullptr;
        out.pose = out.has_pose ? iso_uniform(iso_load(a.poses + (size_t)pair * a.pose_stride)) : iso_identity();
        out.capacity = (uint32_t)a.capacity;
        out.xyz = a.xyz ? a.xyz + (size_t)pair * a.capacity * 3 : nullptr;
        out.pixel = a.pixel ? a.pixel + (size_t)pair * a.capacity : nullptr;
        out.gray = a.gray ? a.gray + (size_t)pair * a.capacity : nullptr;
    }
    point_cloud_body<DENSE, WRITE, false, VOX_OFF>(g, pair, kf0, kfu, kf_depth, rec, a.lvl, a.chunk_points, keep, a.wide_keep != 0, 1u, ws, base, out,
                                                   nullptr, lds);
}
// counts alone: the chunk counts of a pair added up, one thread per pair
__global__ __launch_bounds__(64) void point_cloud_total_kernel(const uint32_t* __restrict__ ws, int ws_chunks, int chunks, int pair0, int n,
                                                               uint32_t* __restrict__ counts) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    uint32_t t = 0;
    for (int k = 0; k < chunks; ++k) t += ws[(size_t)(pair0 + p) * ws_chunks + k];
    counts[pair0 + p] = t;
}
void launch_lm_point_cloud(const Geom& g_in, const PointCloudCall& call, hipStream_t s) {
    const Geom g = launch_geom(g_in, call);
    const bool dense = g.mode == VORS_CANDIDATES_DENSE;
    const bool write = call.xyz || call.pixel || call.gray;
    const size_t plane = (size_t)g.lv[call.lvl].rows * g.lv[call.lvl].cols;
    PointCloudArgs a{0, call.lvl, eval_pairs_chunk_points(g), call.poses, call.pose_stride, call.keep, call.capacity, call.xyz, call.pixel,
                     call.gray, call.counts, call.ws, call.ws_chunks, ((uintptr_t)call.keep % 4 == 0 && plane % 4 == 0) ? 1 : 0};
    const int chunks = std::min(eval_pairs_chunks(g, call.lvl), call.ws_chunks);
    for_pair_slices(call.n_pairs, [&](int pair0, int np) {
        a.pair0 = pair0;
        with_bool(dense, [&](auto d) {
            launch_on_scene(point_cloud_kernel<decltype(d)::value, false>, dim3(chunks, np), dim3(RMAPS_BLOCK), 0, s, g, call, a);
            if (write) launch_on_scene(point_cloud_kernel<decltype(d)::value, true>, dim3(chunks, np), dim3(RMAPS_BLOCK), 0, s, g, call, a);
        });
        if (!write && call.counts)
            hipLaunchKernelGGL(point_cloud_total_kernel, dim3((np + 63) / 64), dim3(64), 0, s, call.ws, call.ws_chunks, chunks, pair0, np, call.counts);
    });
}

// ------------------------------------------------------------------------------------------------------------
// The keyframe map of the lock-step trackers (vors_trackers_enable_map): the pass above as MASKED launches over the promotion list
// (Geom::sel_list; null = every sequence, vors_trackers_init), APPENDING to one list per sequence. What the masked form adds to
// point_cloud_body is select_pair in front, the append base and the keep rule THRESH. The host does not know how many sequences promote,
// so the grids are sized for all of them. Three launches, ordered by the stream alone — no atomic, no flag, no workgroup that waits for
// another:
//   COUNT   the counting sweep on the selected sequence -> ws[seq][chunk]
//   WRITE   the writing sweep with base = counts[seq] (the sequence's running total, still the OLD one) + the counts of the chunks
//           before its own, the lists of the sequence at seq * capacity, and the keyframe pose of the sequence (always applied). A
//           base that has reached the capacity stores nothing.
//   COMMIT  one thread per selected sequence: the segment record {keyframe index, old total, this keyframe's count, pose} if there is
//           room for it, then n_segments += 1 and counts += count (saturating). After WRITE, which reads the old total.
// Keep rule: min_weight <= 1 no plane is read; otherwise `weight` is the depth filter's weight plane (level 0) and a point is kept from
// min_weight on.
// VOXEL FILTER (vors_trackers_enable_map_voxels; point_cloud_append_voxel_kernel): the list keeps ONE point per occupied voxel of a
// world grid, the first in the map's own order. It adds the sequence's table to the same body, and one launch more, in front:
//   CLAIM   the COUNT sweep, whose every kept point enters the sequence's table (voxel_claim): the owner word of a voxel ends as the
//           MINIMUM of the tags (segment index << 32 | slot) of the points that ever fell into it — a value that does not depend on the
//           order of arrival (the keyed z-buffer's argument), that an older keyframe always wins, and that within a keyframe is the
//           point of lowest rank. Nothing is counted or stored besides.
//   COUNT / WRITE  as above, a point kept iff it owns its voxel (voxel_owns, a read-only probe: the table is final when CLAIM has ended).
//   COMMIT  the same kernel.
// The segment index is n_segments[seq], which COMMIT moves on after the three sweeps have read it.
// ------------------------------------------------------------------------------------------------------------
// The append base (saturating; >= capacity: nothing is stored) and the lists of sequence `seq`.
__device__ __forceinline__ CloudOut cloud_out_append(const PointCloudAppendArgs& a, int seq, const uint32_t* ws, int chunk, uint32_t* base) {
    unsigned long long b64 = a.counts[seq];
    for (int k = 0; k < chunk; ++k) b64 += ws[k];  // (uniform)
    *base = b64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b64;
    CloudOut out{};
    out.has_pose = true;
    out.pose = iso_uniform(iso_load(a.kf_poses + 7 * (size_t)seq));
    out.capacity = (uint32_t)a.capacity;
    out.xyz = a.xyz + (size_t)seq * a.capacity * 3;
    out.pixel = a.pixel + (size_t)seq * a.capacity;
    out.gray = a.gray + (size_t)seq * a.capacity;
    return out;
}
// (Two entry points, not one with VOX_OFF among its forms: one __global__ for both moved instructions in the unfiltered kernel.)
template <bool DENSE, bool WRITE>
__global__ __launch_bounds__(RMAPS_BLOCK) void point_cloud_append_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                         const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                         const uint16_t* __restrict__ kf_depth, Records rec, PointCloudAppendArgs a) {
    __shared__ uint32_t lds[2 * PCLOUD_WAVES];
    const int seq = select_pair(g, blockIdx.y);
    if (seq < 0) return;
    const uint8_t* keep = a.weight ? a.weight + (size_t)seq * g.S0 : nullptr;  // (set at level 0 only)
    uint32_t* ws = a.ws + (size_t)seq * a.ws_chunks;
    uint32_t base = 0;
    CloudOut out{};
    if constexpr (WRITE) out = cloud_out_append(a, seq, ws, blockIdx.x, &base);
    point_cloud_body<DENSE, WRITE, true, VOX_OFF>(g, seq, kf0, kfu, kf_depth, rec, a.lvl, a.chunk_points, keep, a.wide_keep != 0, (uint32_t)a.keep_min, ws,
                                                  base, out, nullptr, lds);
}
template <bool DENSE, bool WRITE, int VOX>
__global__ __launch_bounds__(RMAPS_BLOCK) void point_cloud_append_voxel_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                               const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                               const uint16_t* __restrict__ kf_depth, Records rec,
                                                                               PointCloudAppendArgs a, PointCloudVoxelArgs v) {
    static_assert(VOX != VOX_OFF && !(WRITE && VOX == VOX_CLAIM), "CLAIM is a counting sweep");
    __shared__ uint32_t lds[2 * PCLOUD_WAVES];
    const int seq = select_pair(g, blockIdx.y);
    if (seq < 0) return;
    const uint8_t* keep = a.weight ? a.weight + (size_t)seq * g.S0 : nullptr;  // (set at level 0 only)
    uint32_t* ws = a.ws + (size_t)seq * a.ws_chunks;
    uint32_t base = 0;
    CloudOut out{};
    if constexpr (WRITE) out = cloud_out_append(a, seq, ws, blockIdx.x, &base);
    CloudVox vox;
    vox.table = v.table + 2 * (size_t)seq * v.table_slots;
    vox.occupied = v.occupied + seq;
    vox.overflow = v.overflow + seq;
    vox.mask = v.table_slots - 1u;
    vox.voxel_m = v.voxel_m;
    vox.tag_hi = (unsigned long long)a.n_segments[seq] << 32;
    vox.pose = iso_uniform(iso_load(a.kf_poses + 7 * (size_t)seq));
    point_cloud_body<DENSE, WRITE, true, VOX>(g, seq, kf0, kfu, kf_depth, rec, a.lvl, a.chunk_points, keep, a.wide_keep != 0, (uint32_t)a.keep_min, ws,
                                              base, out, &vox, lds);
}
// VOXEL STATISTICS (vors_trackers_enable_map_voxel_stats; a sibling entry point, so that the three kernels above keep their
// arguments and their instructions): per rank of the filtered list, fixed-point sums of every observation of its voxel relative to the
// stored first point, the sum of their greys, their number and the highest segment index among them. The emission becomes
//   CLAIM, COUNT   as above
//   WRITE          <VOX_OWNED_RANK>, in the place of <VOX_OWNED>: the same sweep, which also stores rank_of[entry] = rank for every owned
//                  point it ranks, whether the rank is below the capacity or not. A workgroup whose base has reached the capacity stops
//                  as before, so an entry it never ranks keeps all ones — which reads as a rank beyond every capacity.
//   ACCUMULATE     <VOX_ACCUM>: CLAIM's sweep over the same points; each probes read-only (the table is final), reads its voxel's rank
//                  and adds itself to the rank's statistics (voxel_accumulate). The first point of a voxel counts itself.
//   COMMIT         as above, behind ACCUMULATE: the segment index all sweeps read is still n_segments[seq].
template <bool DENSE, bool WRITE, int VOX>
__global__ __launch_bounds__(RMAPS_BLOCK) void point_cloud_append_voxel_stats_kernel(Geom g, const uint8_t* __restrict__ cur0, const uint8_t* __restrict__ curu,
                                                                                     const uint8_t* __restrict__ kf0, const uint8_t* __restrict__ kfu,
                                                                                     const uint16_t* __restrict__ kf_depth, Records rec,
                                                                                     PointCloudAppendArgs a, PointCloudVoxelArgs v,
                                                                                     PointCloudVoxelStatsArgs st) {
    static_assert((WRITE && VOX == VOX_OWNED_RANK) || (!WRITE && VOX == VOX_ACCUM), "WRITE records ranks, ACCUMULATE is a counting sweep");
    __shared__ uint32_t lds[2 * PCLOUD_WAVES];
    const int seq = select_pair(g, blockIdx.y);
    if (seq < 0) return;
    const uint8_t* keep = a.weight ? a.weight + (size_t)seq * g.S0 : nullptr;  // (set at level 0 only)
    uint32_t* ws = a.ws + (size_t)seq * a.ws_chunks;
    uint32_t base = 0;
    CloudOut out{};
    if constexpr (WRITE) out = cloud_out_append(a, seq, ws, blockIdx.x, &base);
    CloudVoxStats vox;
    vox.table = v.table + 2 * (size_t)seq * v.table_slots;
    vox.occupied = v.occupied + seq;
    vox.overflow = v.overflow + seq;
    vox.mask = v.table_slots - 1u;
    vox.voxel_m = v.voxel_m;
    vox.segment = a.n_segments[seq];
    vox.tag_hi = (unsigned long long)vox.segment << 32;
    vox.pose = iso_uniform(iso_load(a.kf_poses + 7 * (size_t)seq));
    vox.rank_of = st.rank_of + (size_t)seq * v.table_slots;
    vox.sums = reinterpret_cast<unsigned long long*>(st.sums) + 4 * (size_t)seq * a.capacity;
    vox.obs = st.obs + 2 * (size_t)seq * a.capacity;
    vox.xyz = a.xyz + 3 * (size_t)seq * a.capacity;
    vox.capacity = (uint32_t)a.capacity;
    point_cloud_body<DENSE, WRITE, true, VOX>(g, seq, kf0, kfu, kf_depth, rec, a.lvl, a.chunk_points, keep, a.wide_keep != 0, (uint32_t)a.keep_min, ws,
                                              base, out, &vox, lds);
}
__global__ __launch_bounds__(64) void point_cloud_commit_kernel(Geom g, PointCloudAppendArgs a, int n, int chunks) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const int seq = select_pair(g, k);
    if (seq < 0) return;
    uint32_t total = 0;
    for (int c = 0; c < chunks; ++c) total += a.ws[(size_t)seq * a.ws_chunks + c];
    const uint32_t first = a.counts[seq], idx = a.n_segments[seq];
    if (idx < (uint32_t)a.max_keyframes) {
        vors_map_segment* seg = a.segments + (size_t)seq * a.max_keyframes + idx;
        seg->frame = a.kf_frame[seq];
        seg->first = first;
        seg->count = total;
        for (int q = 0; q < 7; ++q) seg->pose7[q] = a.kf_poses[7 * (size_t)seq + q];
    }
    a.n_segments[seq] = idx == 0xFFFFFFFFu ? idx : idx + 1u;
    a.counts[seq] = first + total < first ? 0xFFFFFFFFu : first + total;
}
// call.n_seq: the sequences of the handle (the extent of the pair dimension); g_in.sel_list / sel_count: the ones that get a new segment
// (null: all of them). Every buffer of the call is required but `weight`.
void launch_lm_point_cloud_append(const Geom& g_in, const PointCloudAppendCall& call, hipStream_t s) {
    const Geom g = launch_geom(g_in, call);
    const bool dense = g.mode == VORS_CANDIDATES_DENSE;
    const bool thresh = call.min_weight >= 2 && call.weight != nullptr;
    PointCloudAppendArgs a{call.lvl, eval_pairs_chunk_points(g), call.kf_poses, call.kf_frame, thresh ? call.weight : nullptr,
                           thresh ? call.min_weight : 1, call.capacity, call.max_keyframes, call.xyz, call.pixel, call.gray, call.counts,
                           call.segments, call.n_segments, call.ws, call.ws_chunks,
                           ((uintptr_t)call.weight % 4 == 0 && (size_t)g.S0 % 4 == 0) ? 1 : 0};
    const int chunks = std::min(eval_pairs_chunks(g, call.lvl), call.ws_chunks), n = call.n_seq;
    with_bool(dense, [&](auto d) {
        constexpr bool DENSE = decltype(d)::value;
        if (call.voxels.table) {
            const PointCloudVoxelArgs& v = call.voxels;
            launch_on_scene(point_cloud_append_voxel_kernel<DENSE, false, VOX_CLAIM>, dim3(chunks, n), dim3(RMAPS_BLOCK), 0, s, g, call, a, v);
            launch_on_scene(point_cloud_append_voxel_kernel<DENSE, false, VOX_OWNED>, dim3(chunks, n), dim3(RMAPS_BLOCK), 0, s, g, call, a, v);
            if (call.voxel_stats.rank_of) {
                const PointCloudVoxelStatsArgs& st = call.voxel_stats;
                launch_on_scene(point_cloud_append_voxel_stats_kernel<DENSE, true, VOX_OWNED_RANK>, dim3(chunks, n), dim3(RMAPS_BLOCK), 0, s, g, call, a, v, st);
                launch_on_scene(point_cloud_append_voxel_stats_kernel<DENSE, false, VOX_ACCUM>, dim3(chunks, n), dim3(RMAPS_BLOCK), 0, s, g, call, a, v, st);
            } else {
                launch_on_scene(point_cloud_append_voxel_kernel<DENSE, true, VOX_OWNED>, dim3(chunks, n), dim3(RMAPS_BLOCK), 0, s, g, call, a, v);
            }
        } else {
            launch_on_scene(point_cloud_append_kernel<DENSE, false>, dim3(chunks, n), dim3(RMAPS_BLOCK), 0, s, g, call, a);
            launch_on_scene(point_cloud_append_kernel<DENSE, true>, dim3(chunks, n), dim3(RMAPS_BLOCK), 0, s, g, call, a);
        }
    });
    hipLaunchKernelGGL(point_cloud_commit_kernel, dim3((n + 63) / 64), dim3(64), 0, s, g, a, n, chunks);
}


// ------------------------------------------------------------------------------------------------------------
// vors_voxel_means / vors_trackers_map_voxel_means: the statistics above resolved into an averaged list, rank for rank (lie.h voxel_mean,
// the text vors_voxel_means_host runs). One thread per rank below the clipped count, grid y = list; a rejected rank gets a NaN triple
// and grey 0, nothing is compacted. The first segment of a rank: one word per rank, or a binary search for the last segment whose
// `first` is <= the rank (an empty segment shares its `first` with its successor, which the search prefers; a rank of a keyframe beyond
// max_keyframes has no record and takes the last recorded one), or none. `kept`: a shuffle reduction and one 32-bit atomicAdd per wavefront into
// a cleared word — an integer sum. No LDS.
// WINDOW (the means of the map ICP correction): the ranks [first, first + len) of c.ranges, clipped to the clipped count, in [0, clipped
// count)'s place; the count of passing ranks goes to c.records[i].kept and len to .resolved, both cleared by the launch. A list whose
// window is empty — a sequence that did not promote — is left by the whole workgroup at once. Every store is to a rank below the clipped
// count, hence below capacity, and inside the window.
// ------------------------------------------------------------------------------------------------------------
#define VMEANS_BLOCK 256
template <bool WINDOW>
__global__ __launch_bounds__(VMEANS_BLOCK) void voxel_means_kernel(VoxelMeansCall c) {
    const int i = blockIdx.y;
    uint32_t r0 = 0, len = 0;
    if constexpr (WINDOW) {
        r0 = c.ranges[2 * (size_t)i];
        len = c.ranges[2 * (size_t)i + 1];
        if (len == 0u) return;  // the whole workgroup
    }
    const uint32_t count = c.list_counts[i], total = count < (uint32_t)c.capacity ? count : (uint32_t)c.capacity;
    // (first + len <= total by the window's definition; clipped all the same, without wrapping)
    const uint32_t first = WINDOW ? min(r0, total) : 0u, n = WINDOW ? first + min(len, total - first) : total;
    const size_t row = (size_t)i * (size_t)c.capacity;
    const uint32_t n_seg = c.segments ? min(c.n_segments[i], (uint32_t)c.max_keyframes) : 0u;
    const vors_map_segment* seg = c.segments ? c.segments + (size_t)i * c.max_keyframes : nullptr;
    uint32_t kept = 0;
    for (uint32_t r = first + blockIdx.x * VMEANS_BLOCK + threadIdx.x; r < n; r += gridDim.x * VMEANS_BLOCK) {
        const uint32_t* ob = c.obs + 2 * (row + r);
        uint32_t first_segment = ob[1];  // (no source: span 0)
        if (c.first_segment) first_segment = c.first_segment[row + r];
        else if (n_seg) {
            uint32_t lo = 0, hi = n_seg;  // the last index in [0, n_seg) with first <= r; segment 0 has first 0
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (seg[mid].first <= r) lo = mid;
                else hi = mid;
            }
            first_segment = lo;
        }
        const float* f = c.xyz + 3 * (row + r);
        const long long* sp = c.sums + 4 * (row + r);
        const float f3[3] = {f[0], f[1], f[2]};
        const int64_t s4[4] = {sp[0], sp[1], sp[2], sp[3]};
        const VoxelMean m = voxel_mean(c.voxel_m, f3, s4, ob[0], ob[1], first_segment, c.min_count, c.min_span);
        if (c.xyz_mean) {
            float* o = c.xyz_mean + 3 * (row + r);
            o[0] = m.xyz[0];
            o[1] = m.xyz[1];
            o[2] = m.xyz[2];
        }
        if (c.gray_mean) c.gray_mean[row + r] = m.gray;
        kept += m.kept ? 1u : 0u;
    }
    uint32_t* kept_out = WINDOW ? &c.records[i].kept : (c.kept ? c.kept + i : nullptr);
    if (kept_out) {  // (uniform)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) kept += __shfl_down(kept, off, 64);
        if ((threadIdx.x & 63) == 0 && kept) atomicAdd(kept_out, kept);
    }
    if constexpr (WINDOW)
        if (blockIdx.x == 0 && threadIdx.x == 0) c.records[i].resolved = len;
}
// Workgroups per list: the ranks of the capacity, at most `most` (the loop of the kernel strides over the rest).
static dim3 voxel_means_grid(const VoxelMeansCall& c, long long most) {
    const long long blocks = ((long long)c.capacity + VMEANS_BLOCK - 1) / VMEANS_BLOCK;
    return dim3((unsigned)std::min<long long>(blocks, most), c.n);
}
void launch_voxel_means(const VoxelMeansCall& c, hipStream_t s) {
    if (c.kept) (void)hipMemsetAsync(c.kept, 0, (size_t)c.n * sizeof(uint32_t), s);
    hipLaunchKernelGGL(voxel_means_kernel<false>, voxel_means_grid(c, 4096), dim3(VMEANS_BLOCK), 0, s, c);
}
// 128 workgroups per list, not 4096: in most calls no list has a window, and every workgroup of the grid is then started only to
// return (measured, 64 lists of 2^20 ranks: 0.057 ms per call at 4096). The windows of the promoted lists still fill the device.
void launch_voxel_means_window(const VoxelMeansCall& c, hipStream_t s) {
    (void)hipMemsetAsync(c.records, 0, (size_t)c.n * sizeof(vors_map_icp_means_record), s);
    hipLaunchKernelGGL(voxel_means_kernel<true>, voxel_means_grid(c, 128), dim3(VMEANS_BLOCK), 0, s, c);
}

}  // namespace vors
