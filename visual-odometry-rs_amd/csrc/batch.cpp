// The batch handle (vors_batch_*) and the host-buffer entry built on it (vors_track_pairs): geometry, what a handle allocates, and the
// launches of a step. Owns the device workspaces; the kernels and their launch functions live in the .hip files (engine.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "host_common.h"

using namespace vors;

// ---------------------------------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------------------------------
// FUSED arithmetic: levels of at most this many points are evaluated in the EXACT arithmetic (engine.h Geom::fused_exact_points).
#ifndef VORS_FUSED_EXACT_POINTS_DEFAULT
#define VORS_FUSED_EXACT_POINTS_DEFAULT 2500
#endif
static vors_status build_geom(const vors_config* cfg, int rows, int cols, Geom* g) {
    if (!cfg) return fail(VORS_ERR_INVALID_ARGUMENT, "cfg is NULL");
    if (cfg->nb_levels < 1 || cfg->nb_levels > VORS_MAX_LEVELS)
        return fail(VORS_ERR_INVALID_ARGUMENT, "nb_levels must be in [1, " + std::to_string(VORS_MAX_LEVELS) + "]");
    if (rows < 2 || cols < 2 || rows > 65535 || cols > 65535) return fail(VORS_ERR_INVALID_ARGUMENT, "rows/cols must be in [2, 65535]");
    if ((long long)rows * cols > (1ll << 28))  // the kernels address a level with 32-bit byte offsets
        return fail(VORS_ERR_INVALID_ARGUMENT, "rows * cols must not exceed 2^28 pixels");
    if (cfg->candidates_mode != VORS_CANDIDATES_COARSE_TO_FINE && cfg->candidates_mode != VORS_CANDIDATES_DENSE &&
        cfg->candidates_mode != VORS_CANDIDATES_DSO)
        return fail(VORS_ERR_INVALID_ARGUMENT, "unknown candidates_mode");
    if (cfg->candidates_diff_threshold < 0 || cfg->candidates_diff_threshold > 65535)
        return fail(VORS_ERR_INVALID_ARGUMENT, "candidates_diff_threshold must fit u16");
    std::memset(g, 0, sizeof(*g));
    g->L = cfg->nb_levels;
    if (cfg->arithmetic != VORS_ARITH_EXACT && cfg->arithmetic != VORS_ARITH_FUSED && cfg->arithmetic != VORS_ARITH_REFERENCE)
        return fail(VORS_ERR_INVALID_ARGUMENT, "unknown arithmetic mode");
    g->mode = cfg->candidates_mode;
    g->arith = cfg->arithmetic;
    g->thresh = cfg->candidates_diff_threshold;
    g->depth_scale = cfg->depth_scale;
    g->idepth_variance = cfg->idepth_variance;
    g->huber_delta = cfg->huber_delta;
    g->fused_exact_points = getenv("VORS_FUSED_EXACT_POINTS") ? atoi(getenv("VORS_FUSED_EXACT_POINTS")) : VORS_FUSED_EXACT_POINTS_DEFAULT;
    g->fused_exact_step = getenv("VORS_FUSED_EXACT_STEP") ? atoi(getenv("VORS_FUSED_EXACT_STEP")) : 0;
    g->ref_inflight_x2 = 2;
    g->ref_rank = (getenv("VORS_REF_RANK") && atoi(getenv("VORS_REF_RANK")) == 0) ? 0 : 1;
    g->fused_small_warp = (getenv("VORS_FUSED_SMALL") && std::string(getenv("VORS_FUSED_SMALL")) == "exact") ? 0 : 1;
    g->S0 = rows * cols;
    int r = rows, c = cols;
    Intr k{cfg->cu, cfg->cv, cfg->fu, cfg->fv, cfg->skew};
    int img_off = 0;
    for (int l = 0; l < g->L; ++l) {
        if (l > 0) {
            r /= 2;  // multires.rs:73-77: halve returns None when a half size is 0
            c /= 2;
            if (r == 0 || c == 0)
                return fail(VORS_ERR_PYRAMID_TOO_SHORT,
                            "image too small for nb_levels (the reference panics: inverse_compositional.rs:124-125,183-189)");
            k = intr_half_res(k);  // camera.rs:106-123
        }
        g->lv[l].rows = r;
        g->lv[l].cols = c;
        g->lv[l].k = k;
        g->lv[l].inv_fu_d = 1.0 / (double)k.fu;
        g->lv[l].inv_fv_d = 1.0 / (double)k.fv;
        g->lv[l].inv_fu = (float)g->lv[l].inv_fu_d;
        g->lv[l].inv_fv = (float)g->lv[l].inv_fv_d;
        g->lv[l].s_fuv = (float)((double)k.skew / ((double)k.fu * (double)k.fv));
        if (l == 0) {
            g->lv[l].img_off = -1;
        } else {
            g->lv[l].img_off = img_off;
            img_off += (r * c + 15) & ~15;
        }
    }
    g->upper_stride = std::max(img_off, 16);
    g->root_rows = g->lv[g->L - 1].rows;
    g->root_cols = g->lv[g->L - 1].cols;
    const long n_roots = (long)g->root_rows * g->root_cols;
    long slot_off = 0;
    const bool dense = g->mode == VORS_CANDIDATES_DENSE;
    const bool generic = g->mode == VORS_CANDIDATES_DSO;
    for (int l = 0; l < g->L; ++l) {
        long n = dense ? (long)g->lv[l].rows * g->lv[l].cols : n_roots * (1L << (g->L - 1 - l));
        // generic-mask modes: compacted candidate lists with a fixed capacity per level (the DSO selector aims at 2000 points
        // and re-runs when it gets more than 4x that; 65536 leaves a wide margin, excess candidates would be dropped)
        if (generic) n = std::min((long)g->lv[l].rows * g->lv[l].cols, 65536L);
        if (slot_off + n > 0x7fffffffL) return fail(VORS_ERR_UNSUPPORTED, "too many candidate slots");
        g->lv[l].n_slots = (int)n;
        if (dense && l == 0) {  // dense level 0 stores nothing per point (recomputed on the fly by the LM kernel)
            g->lv[l].slot_off = -1;
            continue;
        }
        g->lv[l].slot_off = (int)slot_off;
        slot_off += (n + 3) & ~3L;
    }
    g->slots_total = (int)std::max(slot_off, 4L);
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// what a handle is made of: pure host decisions from (geometry, max_pairs, environment) ...
// ---------------------------------------------------------------------------------------------------------------
// Threads per frame pair in the LM kernel. Few pairs: one big workgroup per CU (latency); many pairs: 256-thread
// workgroups, several per CU, so that pairs with different iteration counts balance (measured).
// (sparse modes, many pairs: 128 threads — the candidate lists are short, small workgroups waste fewer lanes at the coarse levels and
// more of them are resident: coarse-to-fine LM stage 1.61 -> 1.28 ms per 4096 pairs)
// Round 3: the thresholds below come from tools/speed_sweep.py over 320x240 / 640x480 / 1280x960 x 64 ... 4096 pairs (the round-2 ones
// were fitted at 640x480 with 256 and 4096 pairs and cost 15-25 % at 512 coarse-to-fine pairs, 2.6x at 64 dense 1280x960 pairs):
// the best size depends on the BATCH, hardly on the shape — the chip wants ~100 k resident threads whatever a pair is made of.
static vors_status plan_lm_block(const Geom& g, int max_pairs, int* lm_block) {
    if (g.mode == VORS_CANDIDATES_DENSE) *lm_block = max_pairs >= 512 ? 256 : 1024;
    else if (g.mode == VORS_CANDIDATES_DSO) *lm_block = max_pairs <= 768 ? 512 : 256;  // (lists of ~2000 candidates per level)
    else *lm_block = max_pairs <= 768 ? 512 : (max_pairs < 1536 ? 256 : 128);
    if (const char* e = getenv("VORS_LM_BLOCK")) {  // tuning knob (256 / 512 / 1024)
        const int v = atoi(e);
        if (v != 64 && v != 128 && v != 256 && v != 512 && v != 1024)
            return fail(VORS_ERR_INVALID_ARGUMENT, "VORS_LM_BLOCK must be 64, 128, 256, 512 or 1024");
        *lm_block = v;
    }
    return VORS_OK;
}

// Dense mode, REFERENCE arithmetic: column-major records + current pyramid (engine.h RefDensePlanes). Their index arithmetic (i / rows through
// one multiply-high, lm_reference.hip RefDenseTSrc) is exact while pixels x rows < 2^32 — up to 1920x1080 and beyond; larger frames keep the
// gathering source on the row-major planes (correct, slow).
// A level of ONE row (320x240 with 8 levels, 64x32 with 6) has no multiply-high divisor — floor(2^32 / 1) + 1 wraps to 0 and every
// pixel of the level would decode as (0, i) instead of (i, 0): such pyramids keep the gathering source as well.
static bool plan_ref_dense_planes(const Geom& g) {
    bool one_row_level = false;
    for (int l = 0; l < g.L; ++l) one_row_level = one_row_level || g.lv[l].rows < 2;
    return g.arith == VORS_ARITH_REFERENCE && !one_row_level && (unsigned long long)g.S0 * (unsigned long long)g.lv[0].rows < (1ull << 32);
}

// Generic-mask (DSO) mode: the geometry of the selector's workspace and of the per-pixel planes (the pointers stay null).
struct DsoPlan {
    DsoWs ws{};
    PixelPlanes pp{};
};
static DsoPlan plan_dso(const Geom& g) {
    DsoPlan p;
    const int rr = (g.lv[0].rows + 31) / 32, rc = (g.lv[0].cols + 31) / 32;
    p.ws.n_regions = rr * rc;
    p.ws.max_stride = g.S0 + g.S0 / 4 + g.S0 / 16 + 64;  // worst case: base block size 1
    p.ws.mask_stride = g.S0 + g.S0 / 4 + g.S0 / 16 + 64;
    // picks of one selection round: every block of the first round's three levels at most (a later round with smaller blocks may
    // exceed it: the list then overflows and the pair falls back to the scan of the stamp plane)
    p.ws.list_cap = (g.S0 / 16 + g.S0 / 64 + g.S0 / 256 + 1024 + 3) & ~3;
    int off = 0;
    for (int l = 0; l < g.L; ++l) {  // level 0 is not stored (mask + depth are read instead)
        p.pp.off[l] = off;
        if (l >= 1) off += (g.lv[l].rows * g.lv[l].cols + 3) & ~3;
    }
    p.pp.stride = off > 0 ? off : 4;
    int coff = 0;
    for (int l = 0; l < g.L; ++l) {
        p.pp.chunk_off[l] = coff;
        coff += (g.lv[l].rows * g.lv[l].cols + VORS_CHUNK_PX - 1) / VORS_CHUNK_PX;
    }
    p.pp.chunk_off[g.L] = p.pp.chunks_total = coff;
    return p;
}

// Dense mode: evaluation rounds on the finest levels (engine.h LmSplitWs, lm_kernels.hip).
struct SplitPlan {
    bool present;    // the workspace exists (dense mode unless VORS_LM_SPLIT=0)
    int slots;       // partial-sum slots per pair
    int chunks;      // = slots, or 0: no level is solved by rounds (launch_lm_track then runs the per-pair kernel for every level)
    int n_split, rounds;
    bool side_lane;
    bool predict;    // a level-0 candidate whose step promises a go-on is evaluated in full at once (lm_kernels.hip lm_split_step_kernel)
    float predict_tau;
};
static SplitPlan plan_split(const Geom& g, int max_pairs) {
    SplitPlan p{};
    p.present = g.mode == VORS_CANDIDATES_DENSE && !(getenv("VORS_LM_SPLIT") && atoi(getenv("VORS_LM_SPLIT")) == 0);
    if (!p.present) return p;
    // chunks per pair so that large batches get ~16 workgroups per pair and small ones (down to the single tracker) still spread one
    // evaluation over the chip.
    // `chunks` = partial-sum slots per pair = the late-round cut (at least 512 pixels each); the full rounds use a quarter of it
    // (ONE count for every handle below 512 pairs: the chunk count fixes the order of the f32 partial sums, and a vors_tracker (N = 1)
    // must stay bit-identical to a sequence of a lock-step handle of up to 511 sequences at every image size — the S0 / 2400 cap below
    // only happened to equalise 128 and 256 up to 640x480)
    int chunks = max_pairs >= 1024 ? 64 : (max_pairs >= 512 ? 128 : 256);
    chunks = std::max(4, std::min(chunks, g.S0 / 2400));  // (at least ~2400 pixels per chunk: 320x240 wants 32, not 64-150)
    if (const char* ev = getenv("VORS_LM_CHUNKS")) chunks = std::max(4, atoi(ev));
    p.slots = chunks;
    // levels worth a chip-wide launch per evaluation: at least 64 Ki pixels (640x480: levels 0 and 1; 1280x960: 0, 1, 2)
    int n_split = 0;
    for (int l = 0; l < g.L; ++l)
        if ((long long)g.lv[l].rows * g.lv[l].cols >= 65536) n_split = l + 1;
    p.n_split = getenv("VORS_LM_SPLIT_LEVELS") ? atoi(getenv("VORS_LM_SPLIT_LEVELS")) : std::max(1, n_split);
    p.n_split = std::max(1, std::min(p.n_split, g.L));
    // FUSED: a level of at most fused_exact_points pixels is evaluated in the EXACT arithmetic (include/vors_hip.h) — the per-pair kernel
    // applies that rule, the evaluation rounds do not, so such levels are never solved by rounds (tiny images: no rounds at all)
    if (g.arith == VORS_ARITH_FUSED)
        while (p.n_split > 0 && g.lv[p.n_split - 1].rows * g.lv[p.n_split - 1].cols <= g.fused_exact_points) p.n_split -= 1;
    // rounds before the per-pair finish: a level solved by rounds needs >= 2 of them per evaluation pattern, so the count follows the
    // number of such levels (1280x960 has three: 10 rounds left 64 pairs 2.6x slower than 16)
    const int ns = p.n_split;
    p.rounds = getenv("VORS_LM_SPLIT_ROUNDS") ? atoi(getenv("VORS_LM_SPLIT_ROUNDS")) : (max_pairs >= 512 ? (ns <= 1 ? 12 : 26) : 4 * ns + 8);
    // (a lone dense pair would be 8 % faster with 2 * ns rounds, but a vors_tracker must stay bit-identical to a sequence of a
    // lock-step handle of up to 511 sequences: the same count for every handle below 512 pairs)
    p.chunks = p.n_split == 0 ? 0 : chunks;
    // side lane for the level-1 stragglers of a LARGE batch (engine.h LmSplitWs): two levels solved by rounds, >= 2048 pairs — the rounds
    // of a smaller batch are short enough for the stragglers to keep up (measured: 512 pairs 2.21 -> 2.35 ms, 1024 pairs 3.76 -> 3.81 ms
    // with it, 4096 pairs 12.3 -> 11.9 ms); VORS_LM_SIDE=0 turns it off, VORS_LM_SIDE=1 forces it from 512 pairs on
    const int side_from = (getenv("VORS_LM_SIDE") && atoi(getenv("VORS_LM_SIDE")) == 1) ? 512 : 2048;
    p.side_lane = p.chunks > 0 && p.n_split == 2 && max_pairs >= side_from && !(getenv("VORS_LM_SIDE") && atoi(getenv("VORS_LM_SIDE")) == 0);
    if (p.side_lane && !getenv("VORS_LM_SPLIT_ROUNDS")) p.rounds = 10;  // (the long tail of rounds was theirs; measured 8 / 10 / 12 / 16 / 26 at 4096 pairs)
    // predicted go-ons (profiles/lm_predict_experiments/README.md): FUSED only — the promise is formed from the fast step's delta; the other
    // arithmetics keep the plain schedule. VORS_LM_PREDICT=0 turns it off (development knob; the results are the same bits either way)
    p.predict = p.chunks > 0 && g.arith == VORS_ARITH_FUSED && !(getenv("VORS_LM_PREDICT") && atoi(getenv("VORS_LM_PREDICT")) == 0);
    // VORS_LM_PREDICT_TAU (development knob): the threshold on the promised decrease; tests set it far below and far above the default
    // to make the prediction wrong in either direction
    p.predict_tau = getenv("VORS_LM_PREDICT_TAU") ? (float)atof(getenv("VORS_LM_PREDICT_TAU")) : VORS_LM_PREDICT_TAU;
    return p;
}

// Dense mode, large batches: one vors_batch_track_pairs call as two overlapped slices (host_common.h HalvesPlan). Decided once per handle,
// from max_pairs; everything plan_split and plan_lm_block decide stays a function of the handle's max_pairs and never of a slice's size,
// which is what keeps a pair's bits (tests/test_gpu_large_batches.py pins them against the pair's position and the count of the call).
// Default threshold: measured at 4096 pairs of 640x480 only (profiles/batch_halves/README.md); smaller handles keep the plain path — among
// them, by construction, every handle kind that must stay bit-identical to another: vors_tracker and lock-step handles below 512
// sequences never reach 4096 pairs, and vors_trackers_* never calls vors_batch_track_pairs, the only entry that takes the plan.
// VORS_BATCH_HALVES=0 turns the plan off, =1 forces it from 2 pairs on (development and test knobs, include/vors_hip.h).
#ifndef VORS_BATCH_HALVES_FROM
#define VORS_BATCH_HALVES_FROM 4096
#endif
struct HalvesDecision {
    bool present;
    int from, align, cap;
};
static HalvesDecision plan_halves(const Geom& g, int max_pairs) {
    HalvesDecision p{};
    const char* e = getenv("VORS_BATCH_HALVES");
    p.from = (e && atoi(e) == 1) ? 2 : VORS_BATCH_HALVES_FROM;
    p.present = g.mode == VORS_CANDIDATES_DENSE && !(e && atoi(e) == 0) && max_pairs >= p.from;
    // the kernels choose their wide forms from the alignment of the level-0 buffers (kernels.hip launch_pyramid, launch_keyframe;
    // lm_sources.h launch_geom): a slice that starts h pairs in keeps it when h * S0 is a multiple of 16 (every other per-pair stride is)
    p.align = 1;
    while (p.align < 16 && ((long long)g.S0 * p.align) % 16 != 0) p.align *= 2;
    p.cap = std::max(1, max_pairs / 2);
    return p;
}
// Pairs of the first slice of a call of n_pairs: half of them, rounded up to the alignment; 0 = the call takes the plain path.
static int halves_cut(const HalvesPlan& hp, int n_pairs) {
    if (!hp.present || n_pairs < hp.from) return 0;
    const int h = ((n_pairs + 1) / 2 + hp.align - 1) / hp.align * hp.align;
    return (h >= 1 && h < n_pairs) ? h : 0;
}

// ---------------------------------------------------------------------------------------------------------------
// ... and the allocations: one per buffer, recorded by b->own (host_common.h DeviceResources), checked once by the caller
// ---------------------------------------------------------------------------------------------------------------
static void allocate_workspaces(vors_batch* b, bool allow_halves) {
    const Geom& g = b->g;
    DeviceResources& own = b->own;
    const size_t np = (size_t)b->max_pairs;
    const size_t slots = np * (size_t)g.slots_total;
    own.alloc(&b->kf_upper, np * g.upper_stride);
    own.alloc(&b->cur_upper, np * g.upper_stride);
    if (g.mode == VORS_CANDIDATES_DENSE) {
        own.alloc(&b->rec.IZ, slots);
        own.alloc(&b->rec.V, slots);
        own.alloc(&b->rec.n_used, np * VORS_MAX_LEVELS);
        if (plan_ref_dense_planes(g)) {
            RefDensePlanes& t = b->rec.dense_t;
            own.alloc(&t.recs, np * ((size_t)g.S0 + g.upper_stride));
            own.alloc(&t.n_valid, np * VORS_MAX_LEVELS);
            own.alloc(&t.cur0, np * g.S0);
            own.alloc(&t.curu, np * g.upper_stride);
        }
    } else {  // sparse modes: compact 12-byte candidate lists (+ the keyframe kernel's staging grid in coarse-to-fine mode)
        own.alloc(&b->rec.S, slots);
        own.alloc(&b->rec.n_used, np * VORS_MAX_LEVELS);
        if (g.mode == VORS_CANDIDATES_COARSE_TO_FINE) {
            keyframe_region_geometry(g, &b->rec.kf_r, &b->rec.n_regions);
            own.alloc(&b->rec.stage, slots);
            own.alloc(&b->rec.region_cnt, np * VORS_MAX_LEVELS * (size_t)b->rec.n_regions);
            b->rec.sort_tmp = b->rec.stage;  // (free once the regions have been compacted)
        } else if (g.arith == VORS_ARITH_REFERENCE) {
            own.alloc(&b->rec.sort_tmp, slots);
        }
    }
    if (g.arith == VORS_ARITH_REFERENCE) {  // straggler hand-over of large batches (engine.h RefHandoff)
        own.alloc(&b->rec.handoff.state, np);
        own.alloc(&b->rec.handoff.list, np);
        own.alloc(&b->rec.handoff.counters, 2);
    }
    if (g.mode == VORS_CANDIDATES_DSO) {
        const DsoPlan plan = plan_dso(g);
        b->dso = plan.ws;
        b->pp = plan.pp;
        own.alloc(&b->dso.gmag, np * g.S0);
        own.alloc(&b->dso.median, np * b->dso.n_regions);
        own.alloc(&b->dso.thresh, np * b->dso.n_regions);
        own.alloc(&b->dso.max_g, np * b->dso.max_stride);
        own.alloc(&b->dso.max_pos, np * b->dso.max_stride);
        own.alloc(&b->dso.mask1, np * b->dso.mask_stride);
        own.alloc(&b->dso.picked, np * g.S0);
        own.alloc(&b->dso.state, np);
        if (own.err == hipSuccess) own.err = hipMemset(b->dso.state, 0, np * sizeof(DsoState));  // epoch 0: the first selection clears the stamp plane
        own.alloc(&b->dso.pick_list, np * (size_t)b->dso.list_cap);
        own.alloc(&b->mask0, np * g.S0);
        own.alloc(&b->pp.iz, np * b->pp.stride);
        own.alloc(&b->pp.v, np * b->pp.stride);
        own.alloc(&b->pp.counts, np * b->pp.chunks_total);
    }
    const SplitPlan sp = plan_split(g, b->max_pairs);
    if (sp.present) {
        LmSplitWs& ws = b->split;
        ws.chunks = sp.chunks;
        ws.n_split = sp.n_split;
        ws.rounds = sp.rounds;
        ws.predict = sp.predict ? 1 : 0;
        ws.predict_tau = sp.predict_tau;
        if (sp.predict) own.alloc(&ws.pred_log, np);
        ws.cap = b->max_pairs;
        own.alloc(&ws.state, np);
        own.alloc(&ws.partials, np * sp.slots * 32);
        own.alloc(&ws.list[0], np);
        own.alloc(&ws.list[1], np);
        own.alloc(&ws.count, (size_t)SPLIT_COUNT_INTS);
        ws.side_round = sp.side_lane ? 1 : -1;
        if (sp.side_lane) {
            own.alloc(&ws.side_list, np);
            own.alloc(&ws.join_list, np);
            own.stream(&ws.side_stream, hipStreamNonBlocking);
            own.event(&ws.ev_fork, hipEventDisableTiming);
            own.event(&ws.ev_join, hipEventDisableTiming);
        }
    }
    const HalvesDecision hd = plan_halves(g, b->max_pairs);
    if (hd.present && allow_halves) {  // the second slice's own LM workspace (host_common.h HalvesPlan); with the two side lanes the handle opens three streams
        HalvesPlan& hp = b->halves;
        hp.present = true;
        hp.from = hd.from;
        hp.align = hd.align;
        hp.cap = hd.cap;
        const size_t nb = (size_t)hd.cap;
        if (sp.present) {
            LmSplitWs& ws = hp.split;
            ws = b->split;  // the handle's decisions (chunks, levels, rounds, side round, prediction); pred_log is set per call
            ws.cap = hd.cap;
            own.alloc(&ws.state, nb);
            own.alloc(&ws.partials, nb * sp.slots * 32);
            own.alloc(&ws.list[0], nb);
            own.alloc(&ws.list[1], nb);
            own.alloc(&ws.count, (size_t)SPLIT_COUNT_INTS);
            if (sp.side_lane) {
                own.alloc(&ws.side_list, nb);
                own.alloc(&ws.join_list, nb);
                own.stream(&ws.side_stream, hipStreamNonBlocking);
                own.event(&ws.ev_fork, hipEventDisableTiming);
                own.event(&ws.ev_join, hipEventDisableTiming);
            }
        }
        if (g.arith == VORS_ARITH_REFERENCE) own.alloc(&hp.handoff_counters, 2);
        own.stream(&hp.stream, hipStreamNonBlocking);
        own.event(&hp.ev_fork, hipEventDisableTiming);
        own.event(&hp.ev_join, hipEventDisableTiming);
    }
    if (g.mode == VORS_CANDIDATES_DENSE) {
        float2* lut = nullptr;
        own.alloc(&lut, (size_t)65536);
        b->rec.LUT = lut;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// a step
// ---------------------------------------------------------------------------------------------------------------
vors_status check_stream(const vors_batch* b, hipStream_t s) {
    if (!s) return VORS_OK;  // the default stream of the handle's device (the guard has switched to it)
    hipDevice_t d;
    if (hipStreamGetDevice(s, &d) != hipSuccess) {
        (void)hipGetLastError();
        return VORS_OK;  // cannot tell: let the launch report
    }
    if ((int)d != b->device)
        return fail(VORS_ERR_INVALID_ARGUMENT, "the stream belongs to device " + std::to_string((int)d) + " but the handle lives on device " +
                                                   std::to_string(b->device));
    return VORS_OK;
}
static vors_status check_n(const vors_batch* b, int n_pairs) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL handle");
    if (n_pairs < 1 || n_pairs > b->max_pairs) return fail(VORS_ERR_INVALID_ARGUMENT, "n_pairs out of range for this handle");
    return VORS_OK;
}
vors_status batch_track_current(vors_batch* b, int n_pairs, const uint8_t* d_cur_gray, const float* d_prev_poses7,
                                       const float* d_kf_poses7, float* d_out_poses7, int32_t* d_out_status,
                                       vors_pair_stats* d_out_stats, hipStream_t s) {
    if (b->prepared_pairs <= 0) return fail(VORS_ERR_INVALID_ARGUMENT, "track_current called before prepare_keyframes");
    if (n_pairs > b->prepared_pairs)
        return fail(VORS_ERR_INVALID_ARGUMENT, "track_current: n_pairs (" + std::to_string(n_pairs) + ") exceeds the " +
                                                   std::to_string(b->prepared_pairs) + " keyframes prepared on this handle");
    b->cur_level0 = d_cur_gray;
    b->current_pairs = n_pairs;
    Pyramid cur{d_cur_gray, b->cur_upper};
    STAGE_BEGIN(b, 2, s);
    launch_pyramid(b->g, cur, n_pairs, s);
    if (b->g.arith == VORS_ARITH_REFERENCE) launch_ref_dense_planes_current(b->g, cur, b->rec, n_pairs, s);
    STAGE_END(b, 2, s);
    STAGE_BEGIN(b, 3, s);
    const TrackCall call{{cur, Pyramid{b->kf_level0, b->kf_upper}, b->kf_depth, b->rec}, d_prev_poses7, d_kf_poses7, d_out_poses7, d_out_status, d_out_stats, n_pairs};
    if (b->g.arith == VORS_ARITH_REFERENCE) launch_lm_track_reference(b->g, call, b->ref_device, s);
    else launch_lm_track(b->g, call, b->lm_block, b->split, s);
    STAGE_END(b, 3, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// a step as two overlapped slices (host_common.h HalvesPlan)
// ---------------------------------------------------------------------------------------------------------------
// What one slice of pairs [p0, p0 + n) of a call runs on: the handle's per-pair buffers advanced by p0 pairs, and the LM workspace of
// its own. The launches are the plain path's, with the slice's count: a kernel sees pair k of the slice as pair k.
struct Slice {
    int p0, n;
    hipStream_t s;
    bool second;
    Pyramid kf, cur;
    const uint16_t* kf_depth;
    Records rec;
    LmSplitWs split;
};
static Slice make_slice(const vors_batch* b, int p0, int n, bool second, const uint8_t* kf_gray, const uint16_t* kf_depth, const uint8_t* cur_gray,
                        hipStream_t s) {
    const Geom& g = b->g;
    const size_t p = (size_t)p0;
    Slice v{p0, n, s, second, Pyramid{kf_gray + p * g.S0, b->kf_upper + p * g.upper_stride}, Pyramid{cur_gray + p * g.S0, b->cur_upper + p * g.upper_stride},
            kf_depth + p * g.S0, b->rec, second ? b->halves.split : b->split};
    Records& r = v.rec;
    r.IZ += p * g.slots_total;
    r.V += p * g.slots_total;
    r.n_used += p * VORS_MAX_LEVELS;
    if (r.dense_t.recs) {
        r.dense_t.recs += p * ((size_t)g.S0 + g.upper_stride);
        r.dense_t.n_valid += p * VORS_MAX_LEVELS;
        r.dense_t.cur0 += p * g.S0;
        r.dense_t.curu += p * g.upper_stride;
    }
    if (r.handoff.state) {
        r.handoff.state += p;
        r.handoff.list += p;
        if (second) r.handoff.counters = b->halves.handoff_counters;
    }
    if (second) v.split.pred_log = b->split.pred_log ? b->split.pred_log + p : nullptr;  // the prediction log's slice
    return v;
}
// The stage events of a slice: the first slice's are the plain ring's, the second slice's the ring's second set (StageTimers).
static vors_status slice_stage_mark(vors_batch* b, const Slice& v, int st, bool end) {
    StageTimers& t = b->timers;
    if (t.ring <= 0) return VORS_OK;
    const long idx = t.count[st] % t.ring;
    HIP_TRY(hipEventRecord((v.second ? (end ? t.evb1 : t.evb0) : (end ? t.ev1 : t.ev0))[st][idx], v.s));
    return VORS_OK;
}
static vors_status slice_pre_lm(vors_batch* b, const Slice& v) {
    const Geom& g = b->g;
    vors_status st;
    if ((st = slice_stage_mark(b, v, 0, false)) != VORS_OK) return st;
    launch_pyramid(g, v.kf, v.n, v.s);
    if ((st = slice_stage_mark(b, v, 0, true)) != VORS_OK) return st;
    if ((st = slice_stage_mark(b, v, 1, false)) != VORS_OK) return st;
    launch_keyframe(g, v.kf, v.kf_depth, v.rec, v.n, v.s);
    if (g.arith == VORS_ARITH_REFERENCE) launch_ref_dense_planes_keyframe(g, v.kf, v.kf_depth, v.rec, v.n, v.s);
    if ((st = slice_stage_mark(b, v, 1, true)) != VORS_OK) return st;
    if ((st = slice_stage_mark(b, v, 2, false)) != VORS_OK) return st;
    launch_pyramid(g, v.cur, v.n, v.s);
    if (g.arith == VORS_ARITH_REFERENCE) launch_ref_dense_planes_current(g, v.cur, v.rec, v.n, v.s);
    return slice_stage_mark(b, v, 2, true);
}
static vors_status slice_lm(vors_batch* b, const Slice& v, const float* prev_poses7, float* out_poses7, int32_t* out_status, vors_pair_stats* out_stats) {
    const Geom& g = b->g;
    vors_status st;
    if ((st = slice_stage_mark(b, v, 3, false)) != VORS_OK) return st;
    const TrackCall call{{v.cur, v.kf, v.kf_depth, v.rec}, prev_poses7 ? prev_poses7 + (size_t)v.p0 * 7 : nullptr, nullptr, out_poses7 + (size_t)v.p0 * 7,
                         out_status + v.p0, out_stats ? out_stats + v.p0 : nullptr, v.n};
    if (g.arith == VORS_ARITH_REFERENCE) launch_lm_track_reference(g, call, b->ref_device, v.s);
    else launch_lm_track(g, call, b->lm_block, v.split, v.s);
    return slice_stage_mark(b, v, 3, true);
}
// vors_batch_track_pairs of a handle with the plan, for a call that reaches its threshold: pairs [0, h) on the caller's stream, pairs
// [h, n_pairs) on the plan's stream, forked from the caller's stream at entry and joined back before return — the call stays purely
// stream-ordered for the caller and capturable (the side lane's fork-and-join pattern). Order of issue: A's pyramids and keyframe stage,
// B's, then A's LM stage, then B's.
static vors_status track_pairs_halves(vors_batch* b, int n_pairs, int h, const uint8_t* d_kf_gray, const uint16_t* d_kf_depth, const uint8_t* d_cur_gray,
                                      const float* d_prev_poses7, float* d_out_poses7, int32_t* d_out_status, vors_pair_stats* d_out_stats, hipStream_t s) {
    if (!d_kf_gray || !d_kf_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL image pointer");
    if (!d_cur_gray || !d_out_poses7 || !d_out_status) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL pointer");
    DeviceGuard guard(b->device);
    vors_status st = check_stream(b, s);
    if (st != VORS_OK) return st;
    HalvesPlan& hp = b->halves;
    b->kf_level0 = d_kf_gray;
    b->kf_depth = d_kf_depth;
    b->cur_level0 = d_cur_gray;
    b->prepared_pairs = b->current_pairs = n_pairs;
    const Slice A = make_slice(b, 0, h, false, d_kf_gray, d_kf_depth, d_cur_gray, s);
    const Slice B = make_slice(b, h, n_pairs - h, true, d_kf_gray, d_kf_depth, d_cur_gray, hp.stream);
    HIP_TRY(hipEventRecord(hp.ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(hp.stream, hp.ev_fork, 0));
    // (whatever fails below, the join is enqueued: nothing of this call may still run on the plan's stream behind the caller's back)
    st = slice_pre_lm(b, A);
    if (st == VORS_OK) st = slice_pre_lm(b, B);
    if (st == VORS_OK) st = slice_lm(b, A, d_prev_poses7, d_out_poses7, d_out_status, d_out_stats);
    if (st == VORS_OK) st = slice_lm(b, B, d_prev_poses7, d_out_poses7, d_out_status, d_out_stats);
    HIP_TRY(hipEventRecord(hp.ev_join, hp.stream));
    HIP_TRY(hipStreamWaitEvent(s, hp.ev_join, 0));
    if (st != VORS_OK) return st;
    StageTimers& t = b->timers;
    if (t.ring > 0)
        for (int k = 0; k < 4; ++k) {
            t.two[k][t.count[k] % t.ring] = 1;
            t.count[k] += 1;
        }
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

extern "C" {

vors_status vors_batch_create(const vors_config* cfg, int max_pairs, int rows, int cols, vors_batch** out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = 0;
    }
    return vors_batch_create_on(dev, cfg, max_pairs, rows, cols, out);
}

vors_status vors_batch_create_on(int device, const vors_config* cfg, int max_pairs, int rows, int cols, vors_batch** out) {
    return batch_create_on(device, cfg, max_pairs, rows, cols, true, out);
}

vors_status batch_create_on(int device, const vors_config* cfg, int max_pairs, int rows, int cols, bool allow_halves, vors_batch** out) {
    if (!out) return fail(VORS_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (max_pairs < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "max_pairs must be >= 1");
    Geom g;
    vors_status st = build_geom(cfg, rows, cols, &g);
    if (st != VORS_OK) return st;
    if ((st = require_device()) != VORS_OK) return st;
    if (device < 0 || device >= vors_device_count()) return fail(VORS_ERR_INVALID_ARGUMENT, "device index out of range");
    DeviceGuard guard(device);  // (outlives `b`: a handle that fails below is released on its device)
    if (!guard.ok) return fail(VORS_ERR_HIP, "hipSetDevice failed");
    std::unique_ptr<vors_batch> b(new vors_batch());
    b->device = device;
    b->cfg = *cfg;
    b->g = g;
    b->max_pairs = max_pairs;
    if ((st = plan_lm_block(g, max_pairs, &b->lm_block)) != VORS_OK) return st;
    if (g.arith == VORS_ARITH_REFERENCE) {
        b->ref_device = query_ref_device(device);
        (void)hipGetLastError();  // (an attribute this runtime does not know: the default stands)
    }
    allocate_workspaces(b.get(), allow_halves);
    if (b->own.err != hipSuccess) return fail(VORS_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(b->own.err));
    if (b->rec.LUT) launch_build_depth_lut(g.depth_scale, const_cast<float2*>(b->rec.LUT), nullptr);
    if (g.mode == VORS_CANDIDATES_DENSE) b->g.fast_idepth = (!getenv("VORS_NO_FASTDIV") && verify_fast_idepth(g.depth_scale, nullptr)) ? 1 : 0;
    // Fast exact division by the focal lengths: proven per divisor by exhaustive enumeration on the device, else disabled.
    // Levels halve the focal lengths exactly (camera.rs:119-120), so the level-0 proof covers every level.
    {
        const float fu0 = g.lv[0].k.fu, fv0 = g.lv[0].k.fv;
        const bool ok_u = !getenv("VORS_NO_FASTDIV") && verify_fastdiv(fu0, 1.0f / fu0, nullptr);
        const bool ok_v = !getenv("VORS_NO_FASTDIV") && verify_fastdiv(fv0, 1.0f / fv0, nullptr);
        for (int l = 0; l < g.L; ++l) {
            const float fu = b->g.lv[l].k.fu, fv = b->g.lv[l].k.fv;
            const bool pow2_u = (fu * (float)(1 << l) == fu0), pow2_v = (fv * (float)(1 << l) == fv0);
            b->g.lv[l].fu = FastDiv{fu, 1.0f / fu, (ok_u && pow2_u) ? 1 : 0};
            b->g.lv[l].fv = FastDiv{fv, 1.0f / fv, (ok_v && pow2_v) ? 1 : 0};
        }
    }
    if (hipDeviceSynchronize() != hipSuccess) return fail(VORS_ERR_HIP, "device error while initialising the batch handle");
    *out = b.release();
    return VORS_OK;
}

void vors_batch_destroy(vors_batch* b) {
    if (!b) return;
    DeviceGuard guard(b->device);
    delete b;
}
vors_status vors_batch_device(const vors_batch* b, int* device) {
    if (!b || !device) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    *device = b->device;
    return VORS_OK;
}

vors_status vors_batch_workspace_bytes(const vors_batch* b, uint64_t* bytes) {
    if (!b || !bytes) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    *bytes = b->own.bytes;
    return VORS_OK;
}

vors_status vors_batch_enable_kernel_timing(vors_batch* b, int ring) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL handle");
    if (ring < 0 || ring > 4096) return fail(VORS_ERR_INVALID_ARGUMENT, "ring must be in [0, 4096]");
    DeviceGuard guard(b->device);  // events belong to the device that is current when they are created: the handle's, not the caller's
    if (!guard.ok) return fail(VORS_ERR_HIP, "hipSetDevice failed");
    StageTimers& t = b->timers;
    t.clear();  // stays off if an event cannot be created below
    for (int st = 0; st < 4; ++st) {
        t.ev0[st].assign(ring, nullptr);
        t.ev1[st].assign(ring, nullptr);
        t.two[st].assign(ring, 0);
        for (int k = 0; k < ring; ++k) {
            HIP_TRY(hipEventCreate(&t.ev0[st][k]));
            HIP_TRY(hipEventCreate(&t.ev1[st][k]));
        }
        if (!b->halves.present) continue;
        t.evb0[st].assign(ring, nullptr);
        t.evb1[st].assign(ring, nullptr);
        for (int k = 0; k < ring; ++k) {
            HIP_TRY(hipEventCreate(&t.evb0[st][k]));
            HIP_TRY(hipEventCreate(&t.evb1[st][k]));
        }
    }
    t.ring = ring;
    return VORS_OK;
}

vors_status vors_batch_prepare_keyframes(vors_batch* b, int n_pairs, const uint8_t* d_kf_gray, const uint16_t* d_kf_depth,
                                         void* hip_stream) {
    vors_status st = check_n(b, n_pairs);
    if (st != VORS_OK) return st;
    if (!d_kf_gray || !d_kf_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL image pointer");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, s)) != VORS_OK) return st;
    b->kf_level0 = d_kf_gray;
    b->kf_depth = d_kf_depth;
    b->prepared_pairs = n_pairs;
    Pyramid kf{d_kf_gray, b->kf_upper};
    STAGE_BEGIN(b, 0, s);
    launch_pyramid(b->g, kf, n_pairs, s);
    STAGE_END(b, 0, s);
    STAGE_BEGIN(b, 1, s);
    if (b->g.mode == VORS_CANDIDATES_DSO) {
        launch_keyframe_dso(b->g, kf, d_kf_depth, b->dso, b->mask0, b->pp, b->rec, n_pairs, s);
    } else {
        launch_keyframe(b->g, kf, d_kf_depth, b->rec, n_pairs, s);
    }
    if (b->g.arith == VORS_ARITH_REFERENCE) {  // extract_z's order (inverse_compositional.rs:260-279): sorted lists / column-major planes
        launch_sort_colmajor(b->g, b->rec, n_pairs, s);
        launch_ref_dense_planes_keyframe(b->g, kf, d_kf_depth, b->rec, n_pairs, s);
    }
    STAGE_END(b, 1, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_batch_track_current(vors_batch* b, int n_pairs, const uint8_t* d_cur_gray, const float* d_prev_poses7,
                                     float* d_out_poses7, int32_t* d_out_status, vors_pair_stats* d_out_stats,
                                     void* hip_stream) {
    vors_status st = check_n(b, n_pairs);
    if (st != VORS_OK) return st;
    if (!d_cur_gray || !d_out_poses7 || !d_out_status) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL pointer");
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, static_cast<hipStream_t>(hip_stream))) != VORS_OK) return st;
    return batch_track_current(b, n_pairs, d_cur_gray, d_prev_poses7, nullptr, d_out_poses7, d_out_status, d_out_stats,
                               static_cast<hipStream_t>(hip_stream));
}

vors_status vors_batch_track_pairs(vors_batch* b, int n_pairs, const uint8_t* d_kf_gray, const uint16_t* d_kf_depth,
                                   const uint8_t* d_cur_gray, const float* d_prev_poses7, float* d_out_poses7,
                                   int32_t* d_out_status, vors_pair_stats* d_out_stats, void* hip_stream) {
    if (b && n_pairs >= 1 && n_pairs <= b->max_pairs && halves_cut(b->halves, n_pairs) > 0)
        return track_pairs_halves(b, n_pairs, halves_cut(b->halves, n_pairs), d_kf_gray, d_kf_depth, d_cur_gray, d_prev_poses7, d_out_poses7,
                                  d_out_status, d_out_stats, static_cast<hipStream_t>(hip_stream));
    vors_status st = vors_batch_prepare_keyframes(b, n_pairs, d_kf_gray, d_kf_depth, hip_stream);
    if (st != VORS_OK) return st;
    return vors_batch_track_current(b, n_pairs, d_cur_gray, d_prev_poses7, d_out_poses7, d_out_status, d_out_stats, hip_stream);
}

}  // extern "C"
// Duration of stage `st` of the step in ring entry `idx`. A step that ran as two halves (host_common.h HalvesPlan): the pyramids and the
// keyframe stage are the SUM of the two slices' own intervals; the LM stage runs from the first LM start of either slice to the last LM
// end. The slices overlap, so these figures no longer add up to the step.
static vors_status stage_ms(vors_batch* b, int st, long idx, float* ms) {
    StageTimers& t = b->timers;
    HIP_TRY(hipEventSynchronize(t.ev1[st][idx]));
    HIP_TRY(hipEventElapsedTime(ms, t.ev0[st][idx], t.ev1[st][idx]));
    if (!t.two[st][idx]) return VORS_OK;
    float second = 0.f;
    HIP_TRY(hipEventSynchronize(t.evb1[st][idx]));
    HIP_TRY(hipEventElapsedTime(&second, t.evb0[st][idx], t.evb1[st][idx]));
    if (st != 3) {
        *ms += second;
        return VORS_OK;
    }
    float a_to_b = 0.f, b_to_a = 0.f;
    HIP_TRY(hipEventElapsedTime(&a_to_b, t.ev0[st][idx], t.evb1[st][idx]));
    HIP_TRY(hipEventElapsedTime(&b_to_a, t.evb0[st][idx], t.ev1[st][idx]));
    *ms = std::max(std::max(*ms, second), std::max(a_to_b, b_to_a));
    return VORS_OK;
}
extern "C" {

vors_status vors_batch_kernel_times(vors_batch* b, int stage, float* ms_out, int capacity, int* n_out) {
    if (!b || !n_out || stage < 0 || stage > 3 || (capacity > 0 && !ms_out)) return fail(VORS_ERR_INVALID_ARGUMENT, "bad argument");
    DeviceGuard guard(b->device);
    const int n = (int)std::min<long>(b->timers.count[stage], b->timers.ring);
    *n_out = n;
    for (int k = 0; k < n && k < capacity; ++k) {
        // oldest first
        const long idx = (b->timers.count[stage] - n + k) % b->timers.ring;
        vors_status st = stage_ms(b, stage, idx, &ms_out[k]);
        if (st != VORS_OK) return st;
    }
    return VORS_OK;
}

vors_status vors_batch_last_kernel_ms(vors_batch* b, float* lm_ms, float* keyframe_ms, float* pyramid_ms) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL handle");
    DeviceGuard guard(b->device);
    float v[4] = {-1.f, -1.f, -1.f, -1.f};
    for (int st = 0; st < 4; ++st)
        if (b->timers.ring > 0 && b->timers.count[st] > 0) {
            const long idx = (b->timers.count[st] - 1) % b->timers.ring;
            vors_status rc = stage_ms(b, st, idx, &v[st]);
            if (rc != VORS_OK) return rc;
        }
    if (lm_ms) *lm_ms = v[3];
    if (keyframe_ms) *keyframe_ms = v[1];
    if (pyramid_ms) *pyramid_ms = (v[0] < 0.f && v[2] < 0.f) ? -1.f : std::max(v[0], 0.f) + std::max(v[2], 0.f);
    return VORS_OK;
}

static vors_status get_image(vors_batch* b, const uint8_t* level0, const uint8_t* upper, int pair, int level, uint8_t* out,
                             int* rows, int* cols) {
    if (!b || !out) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (pair < 0 || pair >= b->max_pairs || level < 0 || level >= b->g.L) return fail(VORS_ERR_INVALID_ARGUMENT, "pair/level out of range");
    if (!level0) return fail(VORS_ERR_INVALID_ARGUMENT, "no image has been submitted yet");
    DeviceGuard guard(b->device);
    const LevelGeom& lg = b->g.lv[level];
    const uint8_t* src = level == 0 ? level0 + (size_t)pair * b->g.S0 : upper + (size_t)pair * b->g.upper_stride + lg.img_off;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, src, (size_t)lg.rows * lg.cols, hipMemcpyDeviceToHost));
    if (rows) *rows = lg.rows;
    if (cols) *cols = lg.cols;
    return VORS_OK;
}
vors_status vors_batch_get_keyframe_image(vors_batch* b, int pair, int level, uint8_t* out, int* rows, int* cols) {
    return get_image(b, b ? b->kf_level0 : nullptr, b ? b->kf_upper : nullptr, pair, level, out, rows, cols);
}
vors_status vors_batch_get_current_image(vors_batch* b, int pair, int level, uint8_t* out, int* rows, int* cols) {
    return get_image(b, b ? b->cur_level0 : nullptr, b ? b->cur_upper : nullptr, pair, level, out, rows, cols);
}

vors_status vors_batch_get_points(vors_batch* b, int pair, int level, int capacity, int32_t* xy, float* idepth, float* jac,
                                  uint8_t* tmpl, int* n_out) {
    if (!b || !n_out) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (pair < 0 || pair >= b->max_pairs || level < 0 || level >= b->g.L) return fail(VORS_ERR_INVALID_ARGUMENT, "pair/level out of range");
    const LevelGeom& lg = b->g.lv[level];
    size_t n = (size_t)lg.n_slots;
    DeviceGuard guard(b->device);
    HIP_TRY(hipDeviceSynchronize());
    const bool dense = b->g.mode == VORS_CANDIDATES_DENSE;
    if (!b->kf_level0 || !b->kf_depth)
        return fail(VORS_ERR_INVALID_ARGUMENT, b->prepared_pairs > 0 ? "keyframe inspection is not available on a trackers-owned batch in the candidate-list modes (the handle keeps records, not frames)" : "no keyframe has been prepared yet");
    if (!dense) {  // sparse modes: compact lists
        int used = 0;
        HIP_TRY(hipMemcpy(&used, b->rec.n_used + (size_t)pair * VORS_MAX_LEVELS + level, sizeof(int), hipMemcpyDeviceToHost));
        n = (size_t)std::min(std::max(used, 0), lg.n_slots);
    }
    std::vector<float4> A(n), B(n);
    std::vector<float2> C(n);
    std::vector<uint32_t> XY(n);
    std::vector<float> IZ(n);
    {
        // no mode keeps full records: materialise this level with the exact arithmetic of the reference's precompute
        DevBuf dA, dB, dC, dXY, dIZ;
        HIP_TRY(dA.alloc(n * 16));
        HIP_TRY(dB.alloc(n * 16));
        HIP_TRY(dC.alloc(n * 8));
        HIP_TRY(dXY.alloc(n * 4));
        HIP_TRY(dIZ.alloc(n * 4));
        Records out{dA.as<float4>(), dB.as<float4>(), dC.as<float2>(), dXY.as<uint32_t>(), dIZ.as<float>(), nullptr, nullptr, nullptr};
        if (dense) launch_dense_materialize(b->g, level, pair, Pyramid{b->kf_level0, b->kf_upper}, b->kf_depth, b->rec, out, nullptr);
        else launch_slim_materialize(b->g, level, pair, b->rec, (int)n, out, nullptr);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(A.data(), dA.p, n * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(B.data(), dB.p, n * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(C.data(), dC.p, n * sizeof(float2), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(XY.data(), dXY.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(IZ.data(), dIZ.p, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    int cnt = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!(A[i].w >= 0.f)) continue;
        if (cnt < capacity) {
            if (xy) {
                xy[2 * cnt] = (int32_t)(XY[i] & 0xffffu);
                xy[2 * cnt + 1] = (int32_t)(XY[i] >> 16);
            }
            if (idepth) idepth[cnt] = IZ[i];
            if (jac) {
                jac[6 * cnt] = B[i].x; jac[6 * cnt + 1] = B[i].y; jac[6 * cnt + 2] = B[i].z; jac[6 * cnt + 3] = B[i].w;
                jac[6 * cnt + 4] = C[i].x; jac[6 * cnt + 5] = C[i].y;
            }
            if (tmpl) tmpl[cnt] = (uint8_t)A[i].w;
        }
        ++cnt;
    }
    *n_out = cnt;
    return VORS_OK;
}

// The scene of a batch handle as the products' calls carry it: the keyframe side, and the current frame for the passes that read one.
static LmScene batch_scene(const vors_batch* b, bool with_current) {
    return LmScene{with_current ? Pyramid{b->cur_level0, b->cur_upper} : Pyramid{nullptr, nullptr}, Pyramid{b->kf_level0, b->kf_upper}, b->kf_depth, b->rec};
}

// What a product of the keyframe side alone needs of the handle (reproject_depth, fuse_depth, point_cloud): no current image and no current
// pyramid is read, so the pass is legal before any track_current. A product without a level argument passes 0.
static vors_status check_keyframe_side(const char* who, const vors_batch* b, int n_pairs, int level) {
    if (b->prepared_pairs <= 0 || !b->kf_level0)
        return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + (b->prepared_pairs > 0 ? " is not available on a trackers-owned batch (the handle keeps records, not frames)"
                                                                                         : " needs prepare_keyframes first"));
    if (n_pairs < 1 || n_pairs > b->prepared_pairs)
        return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": n_pairs must be >= 1 and at most the n_pairs of the last prepare_keyframes");
    if (level < 0 || level >= b->g.L) return fail(VORS_ERR_INVALID_ARGUMENT, std::string(who) + ": level out of range");
    return VORS_OK;
}

// What an evaluation at an explicit model needs of the handle (pairs 0 .. last_pair of it) and of the request.
static vors_status check_eval(const vors_batch* b, int last_pair, int level, int arithmetic) {
    if (last_pair < 0 || last_pair >= std::min(b->prepared_pairs, b->current_pairs) || level < 0 || level >= b->g.L)
        return fail(VORS_ERR_INVALID_ARGUMENT, "pair/level out of range (pair must be < the n_pairs of the last prepare_keyframes AND track_current)");
    if (!b->kf_level0 || !b->cur_level0)
        return fail(VORS_ERR_INVALID_ARGUMENT, (b->prepared_pairs > 0 && b->current_pairs > 0 && !b->kf_level0) ? "keyframe inspection is not available on a trackers-owned batch in the candidate-list modes (the handle keeps records, not frames)"
                                                                                                                 : "eval_level needs prepare_keyframes and track_current first");
    if (arithmetic != VORS_ARITH_EXACT && arithmetic != VORS_ARITH_FUSED && arithmetic != VORS_ARITH_REFERENCE)
        return fail(VORS_ERR_INVALID_ARGUMENT, "unknown arithmetic mode");
    return VORS_OK;
}

vors_status vors_batch_eval_level(vors_batch* b, int pair, int level, const float model7[7], int arithmetic, float sums29[29]) {
    if (!b || !model7 || !sums29) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    vors_status st = check_eval(b, pair, level, arithmetic);
    if (st != VORS_OK) return st;
    DeviceGuard guard(b->device);
    DevBuf d_model, d_out;
    HIP_TRY(d_model.alloc(7 * sizeof(float)));
    HIP_TRY(d_out.alloc(32 * sizeof(float)));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(d_model.p, model7, 7 * sizeof(float), hipMemcpyHostToDevice));
    const EvalCall call{batch_scene(b, true), pair, level, d_model.as<float>(), d_out.as<float>()};
    if (arithmetic == VORS_ARITH_REFERENCE)  // sequential sums in the order of the handle's lists (column-major iff the handle itself is REFERENCE)
        launch_lm_eval_level_reference(b->g, call, nullptr);
    else if (arithmetic == VORS_ARITH_FUSED) launch_lm_eval_level_fused(b->g, call, nullptr);
    else launch_lm_eval_level_exact(b->g, call, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(sums29, d_out.p, 29 * sizeof(float), hipMemcpyDeviceToHost));
    return VORS_OK;
}

vors_status vors_batch_lm_predict_log(vors_batch* b, int n_pairs, int32_t* log) {
    if (!b || !log) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_pairs < 0 || n_pairs > b->max_pairs) return fail(VORS_ERR_INVALID_ARGUMENT, "n_pairs out of range");
    DeviceGuard guard(b->device);
    HIP_TRY(hipDeviceSynchronize());
    if (!b->split.pred_log) {  // no prediction on this handle (not dense FUSED, no level solved by rounds, VORS_LM_PREDICT=0)
        for (int i = 0; i < n_pairs; ++i) log[i] = 0;
        return VORS_OK;
    }
    HIP_TRY(hipMemcpy(log, b->split.pred_log, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VORS_OK;
}

// The workspace of the evaluation pass (engine.h EvalPairsWs): created by the first call that needs it and counted by
// vors_batch_workspace_bytes from then on; a handle that only tracks never pays for it.
static vors_status ensure_eval_pairs_ws(vors_batch* b) {
    EvalPairsWs& ws = b->eval_pairs;
    if (ws.items > 0) return VORS_OK;
    const int items = std::min(std::max(b->max_pairs, 256), 32768);  // per slice (also the y extent of a grid)
    int chunks = 1;
    for (int l = 0; l < b->g.L; ++l) chunks = std::max(chunks, eval_pairs_chunks(b->g, l));
    // (a call that failed half-way left what it had allocated in the handle: those buffers are kept and used, not allocated again)
    if (!ws.partials) b->own.alloc(&ws.partials, (size_t)items * chunks * 32);
    if (!ws.fctx) b->own.alloc(&ws.fctx, (size_t)items);
    if (!ws.sums29) b->own.alloc(&ws.sums29, (size_t)b->max_pairs * 29);
    if (b->own.err != hipSuccess) return own_alloc_failed(b, "evaluation workspace");
    ws.items = items;
    ws.chunks = chunks;
    return VORS_OK;
}

static vors_status batch_eval_pairs(vors_batch* b, int n_pairs, int level, int models_per_pair, const void* d_models, size_t model_stride_bytes,
                                    int arithmetic, int what, float* d_sums29, hipStream_t s) {
    vors_status st = ensure_eval_pairs_ws(b);
    if (st != VORS_OK) return st;
    EvalPairsCall call{batch_scene(b, true)};
    call.n_items = n_pairs * models_per_pair;
    call.models_per_pair = models_per_pair;
    call.lvl = level;
    call.models = static_cast<const float*>(d_models);
    call.model_stride = stride_words(model_stride_bytes, 7);
    call.energy_only = what == VORS_EVAL_ENERGY ? 1 : 0;
    call.out29 = d_sums29;
    call.ws = b->eval_pairs;
    if (arithmetic == VORS_ARITH_REFERENCE) launch_lm_eval_pairs_reference(b->g, call, s);
    else if (arithmetic == VORS_ARITH_FUSED) launch_lm_eval_pairs_fused(b->g, call, s);
    else launch_lm_eval_pairs_exact(b->g, call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_batch_eval_pairs(vors_batch* b, int n_pairs, int level, int models_per_pair, const void* d_models, size_t model_stride_bytes,
                                  int arithmetic, int what, float* d_sums29, void* hip_stream) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "eval_pairs: the handle b is NULL");
    if (!d_models) return fail(VORS_ERR_INVALID_ARGUMENT, "eval_pairs: d_models is NULL");
    if (!d_sums29) return fail(VORS_ERR_INVALID_ARGUMENT, "eval_pairs: d_sums29 is NULL");
    if (n_pairs < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "eval_pairs: n_pairs must be >= 1");
    if (models_per_pair < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "eval_pairs: models_per_pair must be >= 1");
    if ((long long)n_pairs * models_per_pair > 0x7fffffffLL / 32) return fail(VORS_ERR_INVALID_ARGUMENT, "eval_pairs: n_pairs * models_per_pair is too large");
    if (what != VORS_EVAL_FULL && what != VORS_EVAL_ENERGY) return fail(VORS_ERR_INVALID_ARGUMENT, "eval_pairs: unknown `what` (VORS_EVAL_FULL or VORS_EVAL_ENERGY)");
    vors_status st = stride_refusal("eval_pairs", "model_stride_bytes", model_stride_bytes, 28, BATCH_STRIDE_LIMIT);
    if (st != VORS_OK) return st;
    if ((st = check_eval(b, n_pairs - 1, level, arithmetic)) != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, s)) != VORS_OK) return st;
    return batch_eval_pairs(b, n_pairs, level, models_per_pair, d_models, model_stride_bytes, arithmetic, what, d_sums29, s);
}

vors_status vors_batch_pose_information(vors_batch* b, int n_pairs, int level, const void* d_models, size_t model_stride_bytes, float* d_info36,
                                        float* d_cov36, float* d_sigma2, int32_t* d_flags, void* hip_stream) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "pose_information: the handle b is NULL");
    if (!d_models) return fail(VORS_ERR_INVALID_ARGUMENT, "pose_information: d_models is NULL");
    if (n_pairs < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "pose_information: n_pairs must be >= 1");
    vors_status st = stride_refusal("pose_information", "model_stride_bytes", model_stride_bytes, 28, BATCH_STRIDE_LIMIT);
    if (st != VORS_OK) return st;
    if ((st = check_eval(b, n_pairs - 1, level, b->g.arith)) != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, s)) != VORS_OK) return st;
    if ((st = ensure_eval_pairs_ws(b)) != VORS_OK) return st;
    if ((st = batch_eval_pairs(b, n_pairs, level, 1, d_models, model_stride_bytes, b->g.arith, VORS_EVAL_FULL, b->eval_pairs.sums29, s)) != VORS_OK) return st;
    launch_pose_information(b->eval_pairs.sums29, n_pairs, d_info36, d_cov36, d_sigma2, d_flags, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_batch_residual_maps(vors_batch* b, int n_pairs, int level, const void* d_models, size_t model_stride_bytes, float* d_residuals,
                                     float* d_warp_uv, uint32_t* d_hist, float* d_scale, void* hip_stream) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "residual_maps: the handle b is NULL");
    if (!d_models) return fail(VORS_ERR_INVALID_ARGUMENT, "residual_maps: d_models is NULL");
    if (!d_residuals && !d_warp_uv && !d_hist && !d_scale)
        return fail(VORS_ERR_INVALID_ARGUMENT, "residual_maps: every output (d_residuals, d_warp_uv, d_hist, d_scale) is NULL");
    if (d_scale && !d_hist) return fail(VORS_ERR_INVALID_ARGUMENT, "residual_maps: d_scale needs d_hist (the pass keeps no histogram of its own)");
    if (n_pairs < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "residual_maps: n_pairs must be >= 1");
    vors_status st = stride_refusal("residual_maps", "model_stride_bytes", model_stride_bytes, 28, BATCH_STRIDE_LIMIT);
    if (st != VORS_OK) return st;
    if ((st = check_eval(b, n_pairs - 1, level, VORS_ARITH_EXACT)) != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, s)) != VORS_OK) return st;
    ResidualMapsCall call{batch_scene(b, true)};
    call.n_pairs = n_pairs;
    call.lvl = level;
    call.models = static_cast<const float*>(d_models);
    call.model_stride = stride_words(model_stride_bytes, 7);
    call.residuals = d_residuals;
    call.warp_uv = d_warp_uv;
    call.hist = d_hist;
    call.scale = d_scale;
    launch_lm_residual_maps(b->g, call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_batch_reproject_depth(vors_batch* b, int n_pairs, int level, const void* d_models, size_t model_stride_bytes,
                                       const uint16_t* d_cur_depth, float tol_m, float* d_pred_z, uint16_t* d_pred_depth, float* d_depth_residual,
                                       uint32_t* d_counts, void* hip_stream) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "reproject_depth: the handle b is NULL");
    if (!d_models) return fail(VORS_ERR_INVALID_ARGUMENT, "reproject_depth: d_models is NULL");
    if (!d_pred_z && !d_pred_depth && !d_depth_residual && !d_counts)
        return fail(VORS_ERR_INVALID_ARGUMENT, "reproject_depth: every output (d_pred_z, d_pred_depth, d_depth_residual, d_counts) is NULL");
    if (d_pred_depth && !d_pred_z)
        return fail(VORS_ERR_INVALID_ARGUMENT, "reproject_depth: d_pred_depth needs d_pred_z (the pass keeps no plane of its own)");
    if (d_depth_residual && !d_cur_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "reproject_depth: d_depth_residual needs d_cur_depth");
    if (d_cur_depth && level != 0)
        return fail(VORS_ERR_INVALID_ARGUMENT, "reproject_depth: d_cur_depth needs level 0 (depth maps exist at full resolution only)");
    if (!(tol_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, "reproject_depth: tol_m must be >= 0 (and not NaN)");
    vors_status st = stride_refusal("reproject_depth", "model_stride_bytes", model_stride_bytes, 28, BATCH_STRIDE_LIMIT);
    if (st != VORS_OK) return st;
    if ((st = check_keyframe_side("reproject_depth", b, n_pairs, level)) != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, s)) != VORS_OK) return st;
    ReprojectCall call{batch_scene(b, false)};
    call.n_pairs = n_pairs;
    call.lvl = level;
    call.models = static_cast<const float*>(d_models);
    call.model_stride = stride_words(model_stride_bytes, 7);
    call.cur_depth = d_cur_depth;
    call.tol_m = tol_m;
    call.pred_z = d_pred_z;
    call.pred_depth = d_pred_depth;
    call.residual = d_depth_residual;
    call.counts = d_counts;
    launch_lm_reproject_depth(b->g, call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

vors_status vors_batch_fuse_depth(vors_batch* b, int n_pairs, const void* d_models, size_t model_stride_bytes, const uint16_t* d_cur_depth,
                                  float tol_m, const uint8_t* d_kf_weight, int max_weight, int fill_min_weight, uint64_t* d_zkey,
                                  uint16_t* d_fused_depth, uint8_t* d_fused_weight, uint32_t* d_counts, void* hip_stream) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: the handle b is NULL");
    if (!d_models) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: d_models is NULL");
    if (!d_cur_depth) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: d_cur_depth is NULL");
    if (!d_zkey) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: d_zkey is NULL (the pass keeps no plane of its own)");
    if ((uintptr_t)d_zkey % 8 != 0) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: d_zkey must be 8-byte aligned");
    if (!(tol_m >= 0.0f)) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: tol_m must be >= 0 (and not NaN)");
    if (max_weight < 1 || max_weight > 255) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: max_weight must be in 1..255");
    if (fill_min_weight < 0 || fill_min_weight > 255) return fail(VORS_ERR_INVALID_ARGUMENT, "fuse_depth: fill_min_weight must be in 0..255");
    vors_status st = stride_refusal("fuse_depth", "model_stride_bytes", model_stride_bytes, 28, BATCH_STRIDE_LIMIT);
    if (st != VORS_OK) return st;
    if ((st = check_keyframe_side("fuse_depth", b, n_pairs, 0)) != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, s)) != VORS_OK) return st;
    FuseDepthCall call{batch_scene(b, false)};
    call.n_pairs = n_pairs;
    call.models = static_cast<const float*>(d_models);
    call.model_stride = stride_words(model_stride_bytes, 7);
    call.cur_depth = d_cur_depth;
    call.tol_m = tol_m;
    call.kf_weight = d_kf_weight;
    call.max_weight = max_weight;
    call.fill_min_weight = fill_min_weight;
    call.zkey = d_zkey;
    call.fused_depth = d_fused_depth;
    call.fused_weight = d_fused_weight;
    call.counts = d_counts;
    launch_lm_fuse_depth(b->g, call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

// The count workspace of the point-cloud pass ([max_pairs][most chunks of a level] integers): created by the first call and counted by
// vors_batch_workspace_bytes from then on, like the evaluation workspace above.
static vors_status ensure_point_cloud_ws(vors_batch* b) {
    if (b->cloud_counts) return VORS_OK;
    int chunks = 1;
    for (int l = 0; l < b->g.L; ++l) chunks = std::max(chunks, eval_pairs_chunks(b->g, l));
    b->own.alloc(&b->cloud_counts, (size_t)b->max_pairs * chunks);
    if (b->own.err != hipSuccess) {
        b->cloud_counts = nullptr;
        return own_alloc_failed(b, "point-cloud workspace");
    }
    b->cloud_chunks = chunks;
    return VORS_OK;
}

vors_status vors_batch_point_cloud(vors_batch* b, int n_pairs, int level, const void* d_poses7, size_t pose_stride_bytes, const uint8_t* d_keep,
                                   int capacity, float* d_xyz, uint32_t* d_pixel, uint8_t* d_gray, uint32_t* d_counts, void* hip_stream) {
    if (!b) return fail(VORS_ERR_INVALID_ARGUMENT, "point_cloud: the handle b is NULL");
    const bool lists = d_xyz || d_pixel || d_gray;
    if (!lists && !d_counts) return fail(VORS_ERR_INVALID_ARGUMENT, "point_cloud: every output (d_xyz, d_pixel, d_gray, d_counts) is NULL");
    if (capacity < 0) return fail(VORS_ERR_INVALID_ARGUMENT, "point_cloud: negative capacity");
    if (lists && capacity == 0) return fail(VORS_ERR_INVALID_ARGUMENT, "point_cloud: d_xyz / d_pixel / d_gray need capacity > 0");
    vors_status st = stride_refusal("point_cloud", "pose_stride_bytes", pose_stride_bytes, 28, BATCH_STRIDE_LIMIT);
    if (st != VORS_OK) return st;
    if ((st = check_keyframe_side("point_cloud", b, n_pairs, level)) != VORS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    DeviceGuard guard(b->device);
    if ((st = check_stream(b, s)) != VORS_OK) return st;
    if ((st = ensure_point_cloud_ws(b)) != VORS_OK) return st;
    PointCloudCall call{batch_scene(b, false)};
    call.n_pairs = n_pairs;
    call.lvl = level;
    call.poses = static_cast<const float*>(d_poses7);
    call.pose_stride = stride_words(pose_stride_bytes, 7);
    call.keep = d_keep;
    call.capacity = capacity;
    call.xyz = d_xyz;
    call.pixel = d_pixel;
    call.gray = d_gray;
    call.counts = d_counts;
    call.ws = b->cloud_counts;
    call.ws_chunks = b->cloud_chunks;
    launch_lm_point_cloud(b->g, call, s);
    HIP_TRY(hipGetLastError());
    return VORS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// host-buffer batch entry
// ---------------------------------------------------------------------------------------------------------------
// Upload an image batch and convert to the row-major device layout when the caller's layout is column-major.
static vors_status upload_u8(const uint8_t* host, int n, int rows, int cols, int layout, DevBuf& dst, DevBuf& tmp, hipStream_t s) {
    const size_t bytes = (size_t)n * rows * cols;
    if (layout == VORS_ROW_MAJOR) {
        HIP_TRY(hipMemcpyAsync(dst.p, host, bytes, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(hipMemcpyAsync(tmp.p, host, bytes, hipMemcpyHostToDevice, s));
        launch_transpose_u8(tmp.as<uint8_t>(), dst.as<uint8_t>(), rows, cols, n, s);
    }
    return VORS_OK;
}
static vors_status upload_u16(const uint16_t* host, int n, int rows, int cols, int layout, DevBuf& dst, DevBuf& tmp, hipStream_t s) {
    const size_t bytes = (size_t)n * rows * cols * 2;
    if (layout == VORS_ROW_MAJOR) {
        HIP_TRY(hipMemcpyAsync(dst.p, host, bytes, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(hipMemcpyAsync(tmp.p, host, bytes, hipMemcpyHostToDevice, s));
        launch_transpose_u16(tmp.as<uint16_t>(), dst.as<uint16_t>(), rows, cols, n, s);
    }
    return VORS_OK;
}

vors_status vors_track_pairs(const vors_config* cfg, int n_pairs, const uint8_t* kf_gray, const uint16_t* kf_depth,
                             const uint8_t* cur_gray, int rows, int cols, int layout, const float* prev_poses7,
                             float* out_poses7, int32_t* out_status, vors_pair_stats* out_stats) {
    if (!kf_gray || !kf_depth || !cur_gray || !out_poses7 || !out_status) return fail(VORS_ERR_INVALID_ARGUMENT, "NULL pointer");
    if (layout != VORS_ROW_MAJOR && layout != VORS_COL_MAJOR) return fail(VORS_ERR_INVALID_ARGUMENT, "bad layout");
    if (n_pairs < 1) return fail(VORS_ERR_INVALID_ARGUMENT, "n_pairs must be >= 1");
    vors_batch* b = nullptr;
    vors_status st = vors_batch_create(cfg, n_pairs, rows, cols, &b);
    if (st != VORS_OK) return st;
    const std::unique_ptr<vors_batch, void (*)(vors_batch*)> guard(b, vors_batch_destroy);
    const size_t S = (size_t)rows * cols, n = (size_t)n_pairs;
    DevBuf d_kf, d_dep, d_cur, d_tmp, d_prev, d_pose, d_stat, d_stats;
    HIP_TRY(d_kf.alloc(n * S));
    HIP_TRY(d_dep.alloc(n * S * 2));
    HIP_TRY(d_cur.alloc(n * S));
    if (layout == VORS_COL_MAJOR) HIP_TRY(d_tmp.alloc(n * S * 2));
    HIP_TRY(d_pose.alloc(n * 7 * sizeof(float)));
    HIP_TRY(d_stat.alloc(n * sizeof(int32_t)));
    HIP_TRY(d_stats.alloc(n * sizeof(vors_pair_stats)));
    hipStream_t s = nullptr;
    if ((st = upload_u8(kf_gray, n_pairs, rows, cols, layout, d_kf, d_tmp, s)) != VORS_OK) return st;
    if ((st = upload_u16(kf_depth, n_pairs, rows, cols, layout, d_dep, d_tmp, s)) != VORS_OK) return st;
    if ((st = upload_u8(cur_gray, n_pairs, rows, cols, layout, d_cur, d_tmp, s)) != VORS_OK) return st;
    if (prev_poses7) {
        HIP_TRY(d_prev.alloc(n * 7 * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(d_prev.p, prev_poses7, n * 7 * sizeof(float), hipMemcpyHostToDevice, s));
    }
    st = vors_batch_track_pairs(b, n_pairs, d_kf.as<uint8_t>(), d_dep.as<uint16_t>(), d_cur.as<uint8_t>(),
                                prev_poses7 ? d_prev.as<float>() : nullptr, d_pose.as<float>(), d_stat.as<int32_t>(),
                                d_stats.as<vors_pair_stats>(), s);
    if (st != VORS_OK) return st;
    HIP_TRY(hipMemcpyAsync(out_poses7, d_pose.p, n * 7 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_status, d_stat.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (out_stats) HIP_TRY(hipMemcpyAsync(out_stats, d_stats.p, n * sizeof(vors_pair_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VORS_OK;
}

}  // extern "C"
