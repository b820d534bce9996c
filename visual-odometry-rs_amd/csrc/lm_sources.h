// The EXACT point sources of the direct-alignment kernels and the per-point pieces every pass over a level's points is made of
// (gfx950 / CDNA4, wave64): what lm_kernels.hip (the Levenberg-Marquardt kernels, both arithmetic modes) and product_kernels.hip (the
// batch products) share. Everything here is the reference's per-point arithmetic; the FUSED extensions of the sources live in
// lm_kernels.hip. Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "engine.h"

namespace vors {

// d / 2 with truncation toward zero (Rust's `/` on i16, gradient.rs:28-29,79,92), branch-free.
__device__ __forceinline__ int half_trunc(int d) { return (d + (int)((unsigned)d >> 31)) >> 1; }

// A candidate point ready for warping: back-projected keyframe point + template grey level (< 0 = empty slot).
struct Pos {
    float X, Y, Z;  // camera.rs:135-140 applied to (x, y, 1/_z)
    float tmpl;
};

// Point sources hand out GROUPS of G independent points per thread and iteration (instruction-level parallelism):
//   fetch(cursor, n_units, raw)   issue every load of the group
//   positions(raw, pos[G])        back-projected points (cheap part, needed before the taps can be addressed)
//   jacobians(raw, J[G][6])       warp Jacobians (inverse_compositional.rs:313-341) — evaluated while the taps are in flight
//   slot(raw, g)                  record index of point g (only used when residuals are written, operator level)

// ---- point source: stored record planes (sparse mode, operator level). G = 2 slots (i, i + BLOCK).
struct RecSrc {
    static constexpr bool FUSED = false;
    static constexpr int G = 2;
    static constexpr bool PREFETCH = false;
    static constexpr bool SKIP_EMPTY = true;
    const float4* A;
    const float4* B;
    const float2* C;
    struct Raw {
        float4 a[2], b[2];
        float2 c[2];
        int i[2];
    };
    struct Cursor {
        int i;
    };
    template <int BLOCK>
    __device__ __forceinline__ Cursor begin(int first = 0) const {
        return Cursor{first + (int)threadIdx.x};
    }
    template <int BLOCK>
    __device__ __forceinline__ Cursor advance(const Cursor& c) const {
        return Cursor{c.i + 2 * BLOCK};
    }
    template <int BLOCK>
    __device__ __forceinline__ void fetch(const Cursor& cur, int n, Raw& r) const {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int i = cur.i + g * BLOCK;
            r.i[g] = i;
            r.a[g] = (i < n) ? A[(unsigned)i] : make_float4(0.f, 0.f, 0.f, -1.f);  // 32-bit offsets from the uniform plane bases
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const bool v = r.a[g].w >= 0.f;
            r.b[g] = v ? B[(unsigned)r.i[g]] : make_float4(0.f, 0.f, 0.f, 0.f);
            r.c[g] = v ? C[(unsigned)r.i[g]] : make_float2(0.f, 0.f);
        }
    }
    __device__ __forceinline__ void positions(const Raw& r, Pos p[2]) const {
#pragma unroll
        for (int g = 0; g < 2; ++g) p[g] = Pos{r.a[g].x, r.a[g].y, r.a[g].z, r.a[g].w};
    }
    __device__ __forceinline__ void jacobian(const Raw& r, int g, float J[6]) const {
        J[0] = r.b[g].x; J[1] = r.b[g].y; J[2] = r.b[g].z; J[3] = r.b[g].w;
        J[4] = r.c[g].x; J[5] = r.c[g].y;
    }
    __device__ __forceinline__ int slot(const Raw& r, int g, int n) const { return r.i[g] < n ? r.i[g] : -1; }
};

// ---- point source: compact 12-byte candidate lists (coarse-to-fine and generic-mask modes of the tracker). G = 2 points (i, i + BLOCK).
// The back-projected point (camera.rs:135-140 applied to (x, y, 1/_z)) and the warp Jacobian (inverse_compositional.rs:313-341) are
// recomputed per evaluation with exactly the arithmetic of the reference's precompute: bit-identical values for 12 B of traffic per
// point instead of 40.
struct SlimSrc {
    static constexpr bool FUSED = false;
    static constexpr int G = 2;
    static constexpr bool PREFETCH = false;
    static constexpr bool SKIP_EMPTY = false;
    const SlimRec* S;
    Intr k;
    FastDiv fu, fv;  // the focal lengths as verified fast divisors (lie.h div_uniform; `ok` = 0: IEEE division)
    struct Raw {
        SlimRec r[2];
        bool valid[2];
    };
    struct Cursor {
        int i;
    };
    template <int BLOCK>
    __device__ __forceinline__ Cursor begin(int first = 0) const {
        return Cursor{first + (int)threadIdx.x};
    }
    template <int BLOCK>
    __device__ __forceinline__ Cursor advance(const Cursor& c) const {
        return Cursor{c.i + 2 * BLOCK};
    }
    template <int BLOCK>
    __device__ __forceinline__ void fetch(const Cursor& cur, int n, Raw& r) const {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int i = cur.i + g * BLOCK;
            r.valid[g] = i < n;
            r.r[g] = S[(unsigned)(r.valid[g] ? i : 0)];  // (a lane past the end re-reads record 0 and masks it)
        }
    }
    __device__ __forceinline__ void positions(const Raw& r, Pos p[2]) const {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const V3 P = back_project_rt(IntrFast{k, fu, fv}, (float)(r.r[g].xy & 0xffffu), (float)(r.r[g].xy >> 16), 1.0f / r.r[g].iz);
            p[g] = Pos{P.x, P.y, P.z, r.valid[g] ? (float)(r.r[g].tg & 0xff) : -1.0f};
        }
    }
    __device__ __forceinline__ void jacobian(const Raw& r, int g, float J[6]) const {
        warp_jacobian_at_rt((float)slim_gx(r.r[g].tg), (float)slim_gy(r.r[g].tg), (float)(r.r[g].xy & 0xffffu), (float)(r.r[g].xy >> 16),
                            r.r[g].iz, IntrFast{k, fu, fv}, J);
    }
    __device__ __forceinline__ int slot(const Raw&, int, int) const { return -1; }
};

// ---- point sources for dense mode: NOTHING is stored per point at level 0. Each evaluation recomputes the point from the
// keyframe image (template + integer gradient, gradient.rs:15-33 / 74-93), the depth map (level 0: from_depth,
// inverse_depth.rs:24-29) or the fused inverse-depth plane (levels >= 1), with exactly the arithmetic of the keyframe
// precompute (back_project camera.rs:135-140, warp_jacobian_at inverse_compositional.rs:313-341): bit-identical points
// for ~4 B of HBM traffic per point instead of 40.
//
// DenseSrc: one pixel per unit, any image width (fallback, keyframe test, diagnostics).
template <bool LEVEL0>
struct DenseSrc {
    static constexpr bool FUSED = false;
    static constexpr int G = 1;
    static constexpr bool PREFETCH = false;
    static constexpr bool SKIP_EMPTY = false;
    const uint8_t* kimg;    // keyframe image of this level
    const uint8_t* kfine;   // next finer keyframe level (levels >= 1)
    const uint16_t* depth;  // level 0
    const float* iz;        // levels >= 1: fused inverse depth, NaN = Unknown
    int rows, cols, fcols;
    Intr k;
    float depth_scale;
    struct Cursor {
        int i, x, y;
        __device__ __forceinline__ int& xq() { return x; }
        __device__ __forceinline__ const int& xq() const { return x; }
    };
    struct Raw {
        int i, x, y;
        float izv;
        int gx, gy, tm;
        bool valid;
    };
    template <int BLOCK>
    __device__ __forceinline__ Cursor begin(int first = 0) const {
        const int t = first + (int)threadIdx.x;
        const int y = t / cols;
        return Cursor{t, t - y * cols, y};
    }
    template <int BLOCK>
    __device__ __forceinline__ Cursor advance(const Cursor& c) const {
        const int dy = BLOCK / cols, dx = BLOCK - dy * cols;  // workgroup-uniform
        int x = c.x + dx, y = c.y + dy;
        if (x >= cols) {
            x -= cols;
            y += 1;
        }
        return Cursor{c.i + BLOCK, x, y};
    }
    template <int BLOCK>
    __device__ __forceinline__ void fetch(const Cursor& c, int n, Raw& r) const {
        r.i = c.i;
        r.x = c.x;
        r.y = c.y;
        r.tm = kimg[c.i];
        if (LEVEL0) {
            const bool interior = c.x > 0 && c.y > 0 && c.x < cols - 1 && c.y < rows - 1;
            const uint8_t* p = kimg + c.i;
            const int l = p[interior ? -1 : 0], rr = p[interior ? 1 : 0], u = p[interior ? -cols : 0], d = p[interior ? cols : 0];
            r.gx = (rr - l) / 2;  // borders: the taps alias the centre pixel -> 0, like gradient.rs:15-33
            r.gy = (d - u) / 2;
            const int dz = depth[c.i];
            r.valid = dz != 0;
            r.izv = depth_scale / (float)dz;
        } else {
            const uint8_t* p = kfine + (size_t)(2 * c.y) * fcols + 2 * c.x;
            const int a = p[0], cc = p[1], b = p[fcols], d = p[fcols + 1];
            r.gx = (cc + d - a - b) / 2;
            r.gy = (b - a + d - cc) / 2;
            r.izv = iz[c.i];
            r.valid = !(r.izv != r.izv);
        }
    }
    __device__ __forceinline__ void positions(const Raw& r, Pos p[1]) const {
        const V3 P = back_project(k, (float)r.x, (float)r.y, 1.0f / r.izv);
        p[0] = Pos{P.x, P.y, P.z, r.valid ? (float)r.tm : -1.0f};
    }
    __device__ __forceinline__ void jacobian(const Raw& r, int, float J[6]) const {
        warp_jacobian_at((float)r.gx, (float)r.gy, (float)r.x, (float)r.y, r.izv, k, J);
    }
    __device__ __forceinline__ int slot(const Raw& r, int g, int n) const { return r.i; }
};

// A load of T from any address: the planes of the caller's need not be aligned, and gfx950 global loads take any address.
template <class T>
__device__ __forceinline__ T load_any(const uint8_t* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

// DenseQuadSrc: FOUR horizontally adjacent pixels per unit (cols % 4 == 0). One dword / dwordx2 / dwordx4 load per image
// row and plane instead of ~8 byte loads per pixel: coalesced 256 B - 1 KiB per wavefront instruction, 4-way ILP per lane.
template <bool LEVEL0, bool FAST>
struct DenseQuadSrc {
    static constexpr bool FUSED = false;
    static constexpr int G = 4;
    static constexpr bool PREFETCH = false;
    static constexpr bool SKIP_EMPTY = false;
    const uint8_t* kimg;
    const uint8_t* kfine;
    const uint16_t* depth;
    const float* iz;
    int rows, cols, fcols, qcols;  // qcols = cols / 4
    IntrFast kf;
    const float2* lut;  // level 0: depth -> (inverse depth, 1 / inverse depth), exact table
    struct Cursor {
        int i, qx, y;  // i = quad index
        __device__ __forceinline__ int& xq() { return qx; }
        __device__ __forceinline__ const int& xq() const { return qx; }
    };
    struct Loaded {  // raw words of one quad, straight from memory (kept in flight one iteration ahead)
        uint32_t cw, w1, w2, w3, w4;  // level 0: centre/up/down rows + left/right bytes; levels >= 1: fine rows (2 x uint2) + unused
        uint32_t d0, d1, d2, d3;      // level 0: depth (uint2) ; levels >= 1: inverse depths (float4 bits)
        int x0, y;
    };
    struct Raw {
        int x0, y;
        float izv[4], zv[4];
        int gx[4], gy[4], tm[4];
        bool valid[4];
    };
    template <int BLOCK>
    __device__ __forceinline__ Cursor begin(int first = 0) const {
        const int t = first + (int)threadIdx.x;
        const int y = t / qcols;
        return Cursor{t, t - y * qcols, y};
    }
    template <int BLOCK>
    __device__ __forceinline__ Cursor advance(const Cursor& c) const {
        const int dy = BLOCK / qcols, dx = BLOCK - dy * qcols;  // workgroup-uniform
        int qx = c.qx + dx, y = c.y + dy;
        if (qx >= qcols) {
            qx -= qcols;
            y += 1;
        }
        return Cursor{c.i + BLOCK, qx, y};
    }
    __device__ __forceinline__ void load(const Cursor& c, Loaded& r) const {
        const int x0 = 4 * c.qx, y = c.y;
        r.x0 = x0;
        r.y = y;
        // 32-bit unsigned offsets from workgroup-uniform bases (scalar base + vector offset addressing, no 64-bit VALU arithmetic)
        const unsigned ucols = (unsigned)cols, o = (unsigned)y * ucols + (unsigned)x0;
        // level 0 and the depth map are the CALLER's buffers, which need not be aligned: loads of any address (load_any), the same
        // dword / dwordx2 instructions, so that a pair's source — and with it the order of the sums — does not depend on where
        // the caller's buffers start
        r.cw = load_any<uint32_t>(kimg + o);
        if (LEVEL0) {
            const bool yin = y > 0 && y < rows - 1;
            r.w1 = load_any<uint32_t>(kimg + (o - (yin ? ucols : 0u)));
            r.w2 = load_any<uint32_t>(kimg + (o + (yin ? ucols : 0u)));
            r.w3 = kimg[o - (x0 > 0 ? 1u : 0u)];
            r.w4 = kimg[o + (x0 + 4 < cols ? 4u : 3u)];
            const uint2 dzw = load_any<uint2>(reinterpret_cast<const uint8_t*>(depth) + (o << 1));
            r.d0 = dzw.x;
            r.d1 = dzw.y;
            r.d2 = r.d3 = 0;
        } else {
            const unsigned ufc = (unsigned)fcols, fo = (unsigned)(2 * y) * ufc + (unsigned)(2 * x0);
            const uint2 f0 = load_any<uint2>(kfine + fo);  // (level 1: the finer level is the caller's level 0)
            const uint2 f1 = load_any<uint2>(kfine + (fo + ufc));
            r.w1 = f0.x; r.w2 = f0.y; r.w3 = f1.x; r.w4 = f1.y;
            const uint4 z4 = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(iz) + (o << 2));
            r.d0 = z4.x; r.d1 = z4.y; r.d2 = z4.z; r.d3 = z4.w;
        }
    }
    __device__ __forceinline__ void decode(const Loaded& l, Raw& r) const {
        const int x0 = l.x0, y = l.y;
        r.x0 = x0;
        r.y = y;
#pragma unroll
        for (int j = 0; j < 4; ++j) r.tm[j] = (l.cw >> (8 * j)) & 0xff;
        if (LEVEL0) {
            // centred differences, truncating /2, zero on the 1-px border (gradient.rs:15-33)
            const int yin = (y > 0 && y < rows - 1) ? -1 : 0;
            const int b[6] = {(int)l.w3, r.tm[0], r.tm[1], r.tm[2], r.tm[3], (int)l.w4};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = x0 + j;
                const int in = yin & ((x > 0 && x < cols - 1) ? -1 : 0);  // all-ones inside, 0 on the 1-px border
                const int up = (l.w1 >> (8 * j)) & 0xff, dn = (l.w2 >> (8 * j)) & 0xff;
                r.gx[j] = half_trunc(b[j + 2] - b[j]) & in;  // masks, not branches: keeps the loop one basic block
                r.gy[j] = half_trunc(dn - up) & in;
                const int dz = (j < 2 ? (l.d0 >> (16 * j)) : (l.d1 >> (16 * (j - 2)))) & 0xffff;
                r.valid[j] = dz != 0;
                // (scale / dz, 1 / (scale / dz)): inverse_depth.rs:24-29, lm_optimizer.rs:215
                const float2 zl = *reinterpret_cast<const float2*>(reinterpret_cast<const uint8_t*>(lut) + ((unsigned)dz << 3));
                r.izv[j] = zl.x;
                r.zv[j] = zl.y;
            }
        } else {
            // 2x2 block gradients of the next finer level (gradient.rs:74-93)
            const uint32_t zz[4] = {l.d0, l.d1, l.d2, l.d3};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w0 = j < 2 ? l.w1 : l.w2, w1 = j < 2 ? l.w3 : l.w4;
                const int sh = (j & 1) * 16;
                const int a = (w0 >> sh) & 0xff, cc = (w0 >> (sh + 8)) & 0xff;
                const int bb = (w1 >> sh) & 0xff, d = (w1 >> (sh + 8)) & 0xff;
                r.gx[j] = half_trunc(cc + d - a - bb);
                r.gy[j] = half_trunc(bb - a + d - cc);
                r.izv[j] = __int_as_float((int)zz[j]);
                r.zv[j] = 1.0f / r.izv[j];
                r.valid[j] = !(r.izv[j] != r.izv[j]);
            }
        }
    }
    template <int BLOCK>
    __device__ __forceinline__ void fetch(const Cursor& c, int n, Raw& r) const {
        Loaded l;
        load(c, l);
        decode(l, r);
    }
    __device__ __forceinline__ void positions(const Raw& r, Pos p[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const V3 P = back_project_fast<FAST>(kf, (float)(r.x0 + j), (float)r.y, r.zv[j]);
            p[j] = Pos{P.x, P.y, P.z, r.valid[j] ? (float)r.tm[j] : -1.0f};
        }
    }
    __device__ __forceinline__ void jacobian(const Raw& r, int j, float J[6]) const {
        warp_jacobian_at_fast<FAST>((float)r.gx[j], (float)r.gy[j], (float)(r.x0 + j), (float)r.y, r.izv[j], kf, J);
    }
    __device__ __forceinline__ int slot(const Raw& r, int g, int n) const { return r.y * cols + r.x0 + g; }
};

struct ImgCtx {
    const uint8_t* img;  // current image of this level, row-major
    int rows, cols;
    Intr k;
    float huber;
    double inv_fu_d, inv_fv_d;    // level constants of the fused arithmetic (engine.h LevelGeom), 0 = form them here
    float inv_fu, inv_fv, s_fuv;
    bool force_exact = false;     // FUSED kernels: evaluate this level in the EXACT arithmetic (workgroup-uniform)
    bool exact_warp = false;      // FUSED kernels, candidate lists: (u, v) of this level from the reference's warp chain, the rest fused
    bool exact_step = false;      // FUSED kernels: step() with lm_step instead of lm_step_fast at this level
};

// warp (lm_optimizer.rs:213-219) + interpolate's inside test (lm_optimizer.rs:227-231): tap address or "outside".
struct Warped {
    float u, v, uf, vf;
    int off;      // offset of tap (v0, u0); 0 when outside (a safe address)
    bool inside;  // valid && inside
};
__device__ __forceinline__ Warped warp_point(const ImgCtx& c, const Iso& model, const Pos& p) {
    Warped w;
    const V3 p2 = iso_transform_point(model, V3{p.X, p.Y, p.Z});
    project_uv(c.k, p2, &w.u, &w.v);
    w.uf = floorf(w.u);
    w.vf = floorf(w.v);
    w.inside = (p.tmpl >= 0.f) && (w.uf >= 0.f) && (w.uf < (float)(c.cols - 2)) && (w.vf >= 0.f) && (w.vf < (float)(c.rows - 2));
    // masked, not branched (an outside point reads the safe address 0 and is selected away later)
    w.off = (__float2int_rz(w.vf) * c.cols + __float2int_rz(w.uf)) & (w.inside ? -1 : 0);
    return w;
}
struct Taps {
    uint32_t top, bot;  // (t00 | t01 << 8), (t10 | t11 << 8)
};
__device__ __forceinline__ Taps load_taps(const ImgCtx& c, const Warped& w) {
    const unsigned o = (unsigned)w.off;  // >= 0 by construction; 32-bit offset from the uniform image base
    uint16_t a, b;
    __builtin_memcpy(&a, c.img + o, 2);  // two adjacent bytes per row: one (possibly unaligned) 16-bit load each
    __builtin_memcpy(&b, c.img + (o + (unsigned)c.cols), 2);
    return Taps{a, b};
}
// bilinear (lm_optimizer.rs:236-247, term order as written) + residual: interpolate(u, v) - template, whatever `inside` says. The ONE
// text the sums (accumulate_point) and the per-point outputs (lm_residual_maps_kernel) are made of.
__device__ __forceinline__ float bilinear_residual(float tmpl, const Warped& w, const Taps& t) {
    const float vu_00 = (float)(t.top & 0xff), vu_01 = (float)(t.top >> 8), vu_10 = (float)(t.bot & 0xff), vu_11 = (float)(t.bot >> 8);
    const float fa = w.u - w.uf, fb = w.v - w.vf;
    const float im = (1.0f - fb) * (1.0f - fa) * vu_00 + fb * (1.0f - fa) * vu_10 + (1.0f - fb) * fa * vu_01 + fb * fa * vu_11;
    return im - tmpl;
}

// Values read from LDS are uniform across the workgroup but land in vector registers; readfirstlane moves them to SGPRs.
__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ Iso iso_uniform(const Iso& m) {
    return Iso{V3{uniform_f(m.t.x), uniform_f(m.t.y), uniform_f(m.t.z)}, Quat{uniform_f(m.q.i), uniform_f(m.q.j), uniform_f(m.q.k), uniform_f(m.q.w)}};
}

// Per-level dispatch: build the EXACT point source of a level and run `f(src, n_slots)`.
template <bool DENSE, bool QUADS, class F>
__device__ __forceinline__ void with_exact_source(const Geom& g, int lvl, int pair, const uint8_t* kf0, const uint8_t* kfu,
                                                  const uint16_t* kf_depth, const Records& rec, F&& f) {
    const LevelGeom lg = g.lv[lvl];
    if constexpr (DENSE) {
        const uint8_t* kimg = level_ptr(g, kf0, kfu, pair, lvl);
        const uint8_t* kfine = lvl > 0 ? level_ptr(g, kf0, kfu, pair, lvl - 1) : nullptr;
        const uint16_t* depth = kf_depth + (size_t)pair * g.S0;
        const float* iz = lvl > 0 ? rec.IZ + (size_t)pair * g.slots_total + lg.slot_off : nullptr;
        const int fcols = lvl > 0 ? g.lv[lvl - 1].cols : 0;
        // quads need rows of whole quads in every plane they read (and 16-byte aligned inverse-depth rows)
        const bool quad_ok = QUADS && g.wide_loads_ok && (lg.cols % 4 == 0) && (lvl == 0 ? (g.S0 % 4 == 0) : (fcols % 8 == 0));
        if (lvl == 0) {
            if constexpr (QUADS) {
                if (quad_ok) {
                    if (lg.fu.ok && lg.fv.ok) {  // workgroup-uniform: selects the instantiation, no branch in the hot loop
                        DenseQuadSrc<true, true> src{kimg, kfine, depth, iz, lg.rows, lg.cols, fcols, lg.cols / 4, IntrFast{lg.k, lg.fu, lg.fv}, rec.LUT};
                        f(src, lg.rows * (lg.cols / 4));
                    } else {
                        DenseQuadSrc<true, false> src{kimg, kfine, depth, iz, lg.rows, lg.cols, fcols, lg.cols / 4, IntrFast{lg.k, lg.fu, lg.fv}, rec.LUT};
                        f(src, lg.rows * (lg.cols / 4));
                    }
                    return;
                }
            }
            DenseSrc<true> src{kimg, kfine, depth, iz, lg.rows, lg.cols, fcols, lg.k, g.depth_scale};
            f(src, lg.n_slots);
        } else {
            if constexpr (QUADS) {
                if (quad_ok) {
                    if (lg.fu.ok && lg.fv.ok) {
                        DenseQuadSrc<false, true> src{kimg, kfine, depth, iz, lg.rows, lg.cols, fcols, lg.cols / 4, IntrFast{lg.k, lg.fu, lg.fv}, rec.LUT};
                        f(src, lg.rows * (lg.cols / 4));
                    } else {
                        DenseQuadSrc<false, false> src{kimg, kfine, depth, iz, lg.rows, lg.cols, fcols, lg.cols / 4, IntrFast{lg.k, lg.fu, lg.fv}, rec.LUT};
                        f(src, lg.rows * (lg.cols / 4));
                    }
                    return;
                }
            }
            DenseSrc<false> src{kimg, kfine, depth, iz, lg.rows, lg.cols, fcols, lg.k, g.depth_scale};
            f(src, lg.n_slots);
        }
    } else {
        const SlimRec* S = rec.S + (size_t)pair * g.slots_total + lg.slot_off;
        const int n = __builtin_amdgcn_readfirstlane(rec.n_used[(size_t)pair * VORS_MAX_LEVELS + lvl]);
        SlimSrc src{S, lg.k, lg.fu, lg.fv};
        f(src, n);
    }
}

// The current image of a level and the level's constants (the FUSED exact_* choices are the caller's).
__device__ __forceinline__ ImgCtx level_ctx(const Geom& g, const uint8_t* cur0, const uint8_t* curu, int pair, int lvl) {
    ImgCtx c;
    c.img = level_ptr(g, cur0, curu, pair, lvl);
    c.rows = g.lv[lvl].rows;
    c.cols = g.lv[lvl].cols;
    c.k = g.lv[lvl].k;
    c.huber = g.huber_delta;
    c.inv_fu_d = g.lv[lvl].inv_fu_d; c.inv_fv_d = g.lv[lvl].inv_fv_d;
    c.inv_fu = g.lv[lvl].inv_fu; c.inv_fv = g.lv[lvl].inv_fv; c.s_fuv = g.lv[lvl].s_fuv;
    return c;
}

// The cut of a level: a grid of (chunks of the level) x (pairs or items) gives workgroup `chunk` the units [first, last) of the level's
// source. A pair has level_chunks chunks at this level (a short candidate list needs fewer than the grid has: the rest of the workgroups
// have nothing to do); chunk c of `chunks` holds the units [c * per + min(c, rem), ...): one 32-bit scalar division (the 64-bit
// n * c / chunks costs ~150 scalar instructions apiece, in every workgroup). lm_eval_pairs_kernel and every batch product cut a level
// with these two; lm_split_eval_kernel has its own chunk count. (Two functions with the caller's early return between them: one that
// returns {first, last, mine} changes the instruction stream of most callers.)
struct LevelCut {
    int first, last;
};
__device__ __forceinline__ int level_chunks(int points, int chunk_points, int n_chunks) {
    return min(max((points + chunk_points - 1) / chunk_points, 1), n_chunks);
}
__device__ __forceinline__ LevelCut level_cut(int n_units, int chunk, int chunks) {
    const unsigned per = (unsigned)n_units / (unsigned)chunks, rem = (unsigned)n_units - per * (unsigned)chunks;
    const int first = (int)((unsigned)chunk * per + min((unsigned)chunk, rem));
    const int last = (int)((unsigned)(chunk + 1) * per + min((unsigned)(chunk + 1), rem));
    return LevelCut{first, last};
}

// The geometry of a launch on `call`: wide_loads_ok set iff the handle's own planes are 16-byte aligned (the dense quad source's dwordx4
// loads of the inverse depths). The caller's level 0 and depth map are read with loads of any address (DenseQuadSrc::load): whether a
// pair takes the quad source, and so the order of its sums, is a matter of the shape alone and never of where the caller's buffers start.
static inline Geom launch_geom(const Geom& g_in, const LmScene& call) {
    Geom g = g_in;
    g.wide_loads_ok = (((uintptr_t)call.kf.upper | (uintptr_t)call.rec.IZ) % 16 == 0) ? 1 : 0;
    return g;
}

}  // namespace vors
