// Internal interface between the HIP kernels and their launch functions (kernels.hip, lm_kernels.hip, product_kernels.hip, lm_reference.hip, dso_kernels.hip)
// and the host engine / C ABI (host_common.h; batch.cpp, trackers.cpp, trackers_map.cpp, pipeline.cpp, operators.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/vors_hip.h"
#include "lie.h"

namespace vors {

// Geometry of one pyramid level.
struct LevelGeom {
    int rows, cols;     // image shape at this level (floor halving, multires.rs:67-88)
    int img_off;        // byte offset of this level inside the per-pair "upper levels" buffer (levels >= 1); -1 for level 0
    int n_slots;        // candidate slots at this level (sparse: roots * 2^(L-1-l); dense: rows*cols)
    int slot_off;       // offset of this level's slots inside the per-pair planes (dense: IZ/V planes hold levels >= 1 only; -1 for level 0)
    Intr k;             // intrinsics of this level (camera.rs:106-123)
    FastDiv fu, fv;     // verified fast exact division by the focal lengths of this level (lie.h)
    // level constants of the FUSED arithmetic, formed once on the host in f64 (the kernels would otherwise redo these divisions in
    // every evaluation): 1 / fu, 1 / fv as f64 (for H = K R K^-1), and as f32 1 / fu, 1 / fv, s / (fu fv) (Jacobian)
    double inv_fu_d, inv_fv_d;
    float inv_fu, inv_fv, s_fuv;
};

// Everything a kernel needs to know about the batch layout. Passed by value.
struct Geom {
    int L;              // nb_levels
    int mode;           // VORS_CANDIDATES_*
    int arith;          // VORS_ARITH_*
    int thresh;         // candidates_diff_threshold (u16)
    float depth_scale, idepth_variance, huber_delta;
    int S0;             // rows*cols of level 0 (pair stride of level-0 images and depth maps)
    int upper_stride;   // bytes per pair of levels 1..L-1
    int slots_total;    // record slots per pair (all levels)
    int root_rows, root_cols;  // shape of the coarsest level (= roots of the selection quad-trees)
    int fast_idepth;    // scale / depth through idepth_of<true> (kernels.hip): proven bit-identical to the division for all 65535 depths
    // FUSED arithmetic: a level of at most this many points (dense: pixels of the level; sparse modes: candidates of the pair at the level)
    // is evaluated in the EXACT arithmetic (lm_kernels.hip lm_track_kernel); fused_exact_step != 0 also takes its step() with lm_step
    int fused_exact_points, fused_exact_step;
    int fused_small_warp;  // candidate-list modes: such a level takes only (u, v) from the reference's warp chain (lm_kernels.hip fused_stage_b<XW>)
    int ref_rank;       // REFERENCE arithmetic, coarse-to-fine: rank the keyframe kernel's staged regions directly (lm_reference.hip); resolved ONCE per
                        // handle from VORS_REF_RANK (development knob) so that the keyframe stage and the sort take the same decision
    int ref_inflight_x2;  // REFERENCE arithmetic, candidate lists: twice the number of steps whose LM stages share the chip (2 = a step on its own;
                          // 3 = a slot of a vors_pipeline ring: the LM stage is ~2/3 of a step, so about 1.5 of them overlap). The workgroup size of
                          // the workgroup-per-pair kernel is chosen for n_pairs x this / 2 RESIDENT pairs (lm_reference.hip refc_waves_per_pair): a
                          // ring wants the thinner workgroups whose LDS lets the LM kernels of consecutive steps share a CU. The sums do not depend on it
    int wide_loads_ok;  // set per launch (lm_sources.h launch_geom): the handle's own planes are 16-byte aligned, so the dense quad source may use wide loads
    // Masked launches of the keyframe stage (vors_trackers: per-sequence keyframe promotion on the device). When sel_list is set, index k
    // of a kernel's pair dimension addresses pair sel_list[k] for k < *sel_count and nothing beyond (device_common.h select_pair).
    const int* sel_list;
    const int* sel_count;
    LevelGeom lv[VORS_MAX_LEVELS];
};

// Candidate record of the coarse-to-fine and generic-mask (DSO) modes: 12 bytes per point, everything else (the back-projected point,
// the warp Jacobian) is recomputed by the LM kernel from it — like the reference's Obs (lm_optimizer.rs:43-58) minus the Jacobians and
// Hessians it precomputes. Per pair and level the records are COMPACT: slots [0, n_used) hold points, nothing else is ever read.
struct SlimRec {
    uint32_t xy;  // x | y << 16
    float iz;     // inverse depth
    uint32_t tg;  // template grey level | (gx & 0x3ff) << 8 | (gy & 0x3ff) << 18   (integer gradients of the level, |g| <= 255)
};
__host__ __device__ inline uint32_t slim_pack_tg(int tmpl, int gx, int gy) {
    return (uint32_t)tmpl | (((uint32_t)gx & 0x3ffu) << 8) | (((uint32_t)gy & 0x3ffu) << 18);
}
__host__ __device__ inline int slim_gx(uint32_t tg) { return ((int)(tg << 14)) >> 22; }
__host__ __device__ inline int slim_gy(uint32_t tg) { return ((int)(tg << 4)) >> 22; }

// Operator-level record planes (explicit observations, vors_lm_eval / vors_lm_solve; also the inspection output of
// vors_batch_get_points). Structure of arrays, one entry per slot:
//   A = (X, Y, Z, tmpl)  back-projected keyframe point (camera.rs:135-140) + template grey level; tmpl < 0 = empty slot
//   B = (J0, J1, J2, J3) C = (J4, J5)   warp Jacobian (inverse_compositional.rs:313-341)
//   XY = x | y << 16     pixel coordinates (keyframe test, inspection)
//   IZ = inverse depth   (inspection only)
// REFERENCE arithmetic, dense mode: everything the LM kernel reads, in COLUMN-MAJOR order. The reference enumerates the pixels of a level
// column by column (DMatrix order, inverse_compositional.rs:260-279), so consecutive points of its order are consecutive ROWS: on the
// row-major planes a wavefront's 64 points touch 64 cache lines per load, here they touch one or two — and point i of the enumeration is
// element i of the level.
//   recs      per pixel of every level, 8 bytes: (inverse depth f32 — scale / depth at level 0 (inverse_depth.rs:24-29), the fused value
//             above, NaN = Unknown — and template | gx | gy packed like SlimRec.tg): the level's Obs entry minus what the LM kernel
//             recomputes (lm_optimizer.rs:43-58), written once per keyframe by lm_reference.hip ref_dense_records_kernel.
//             Pair stride S0 + upper_stride entries; level 0 at 0, level l >= 1 at S0 + img_off.
//   cur0/curu the current frame's pyramid, column-major level by level (laid out like the row-major pyramid).
struct RefDensePlanes {
    uint2* recs;
    int* n_valid;  // [pair][VORS_MAX_LEVELS] pixels with a known inverse depth per level, counted while the records are written (diagnostics)
    uint8_t* cur0;
    uint8_t* curu;
};

// REFERENCE arithmetic, large batches: hand-over of the pairs still iterating when most of the batch has finished (lm_reference.hip).
// One wavefront per pair fills the chip while every pair is alive; the pairs with the most iterations then run alone, one wavefront on a
// SIMD each, at a third of the chip's rate. Once `after` pairs are done, a wavefront that is about to start another evaluation saves its LM
// state instead and queues its pair; a second launch gives each queued pair a whole workgroup (the same chains, bit for bit).
struct RefResume {  // the state of optimizer::State::iterative_solve between two evaluations (lm_reference.hip RefLm) + the level
    float cur_model[7], cand[7];
    float entry[7];  // the model the level started from: lm_model stays it if the level fails (inverse_compositional.rs:195-199)
    float kept[28];
    float cur_energy, lm_coef;
    int nb_iter, n_full, lvl;
};
struct RefHandoff {
    RefResume* state;  // [pairs]
    int* list;         // [pairs] queued pairs
    int* counters;     // [0] pairs queued, [1] pairs finished by the first launch
};

struct Records {
    float4* A;
    float4* B;
    float2* C;
    uint32_t* XY;
    float* IZ;
    float* V;  // dense mode only: fused weight ("variance") plane, < 0 = Unknown
    const float2* LUT;  // dense mode only: depth u16 -> (scale / depth, 1 / (scale / depth)), exact
    int* n_used;  // [pair][VORS_MAX_LEVELS]; sparse modes: slots in use per level (compact, no holes); dense mode: usable points
                  // per level counted by the keyframe stage (level 0 only when L >= 2)
    SlimRec* S;         // coarse-to-fine / generic-mask modes: compact candidate lists, pair stride slots_total, level offset slot_off
    SlimRec* stage;     // coarse-to-fine mode: the keyframe kernel's slot grid (compacted per wavefront region), input of the per-pair compaction
    int* region_cnt;    // coarse-to-fine mode: [pair][level][region] points per wavefront region
    int n_regions;      //   regions per level (= wavefronts of the keyframe kernel per pair)
    int kf_r;           //   roots per wavefront region
    RefDensePlanes dense_t;  // REFERENCE arithmetic, dense mode (all null otherwise)
    RefHandoff handoff;      // REFERENCE arithmetic (null otherwise)
    SlimRec* sort_tmp;  // REFERENCE arithmetic, sparse modes: scratch of the column-major sort (lm_reference.hip), laid out like S; the
                        // coarse-to-fine mode lends its staging grid, which is free once the regions have been compacted
};

// Workspace of the DSO-style selector (dso_kernels.hip), all per pair.
struct DsoState {
    int base_size, iterations_left, done, random_keep, count, final_round;
    int epoch;  // 1 .. 15: the selection this pair's pick stamps belong to (dso_kernels.hip: the stamp plane is cleared when it wraps, not per keyframe)
};
struct DsoWs {
    uint8_t* gmag;      // [S0] gradient magnitude (<= 180)
    uint16_t* median;   // [n_regions]
    uint16_t* thresh;   // [n_regions]
    uint8_t* max_g;     // [max_stride] block maxima of the 3 levels, concatenated
    uint32_t* max_pos;  // [max_stride] their pixel positions (row * cols + col)
    uint8_t* mask1;     // [mask_stride] block masks of levels 1 and 2 (+ the discarded mask after the last level)
    uint8_t* picked;    // [S0] 0 or (round << 2 | level + 1) of the pick
    DsoState* state;    // [1]
    uint32_t* pick_list;  // [list_cap] pixel positions picked in the round in progress (the last round executed = the final one)
    int n_regions, max_stride, mask_stride, list_cap;
};
// Evaluation rounds on the finest levels (dense mode, lm_kernels.hip "split" path): the coarse levels run in the per-pair
// kernel; then every ROUND is one launch that evaluates the energy of each still-active pair at ITS current level and
// candidate over (active pairs x chunks of the image), followed by a tiny per-pair launch that gives the verdict, takes the
// next step or moves the pair to the next level. All CUs stay busy whatever the pairs' iteration counts; the few pairs still
// iterating after `rounds` rounds finish inside the final per-pair kernel.
struct LmSplitState {  // per pair
    float entry[7];    // model on entry to the level: restored when step() fails (the level's progress is discarded)
    float model[7];    // kept model (the level's running estimate)
    float cand[7];     // candidate under evaluation
    float sums[32];    // sums of the kept state (energy sum, n, g[6], H upper triangle[21])
    float cur_energy, lm_coef;
    int nb_iter;
    int n_full;        // initial evaluation + accepted candidates of this level so far (statistics: vors_pair_stats.nb_grad_evals)
    int lvl;           // level being solved
    int phase;         // 0 init evaluation pending (full), 1 candidate's energy pending, 4 accepted candidate's g and H pending (full),
                       // 2 all levels finished
    int pred;          // written by the step kernel with phase 1 / 4, read only then (LmSplitWs::predict). Phase 1: 1 = the candidate was
                       // predicted to go on and is due a FULL evaluation in a round of energy-only ones, its sums 0 and 1 added in the
                       // energy-only kernel's order; 3 = it could have been predicted and was not (bookkeeping of LmSplitWs::pred_log
                       // only). Phase 4: 2 = g and H are in `sums` already (taken from that evaluation): the pair sits
                       // this round out, so that each of its later evaluations falls in the round it has without the prediction
    int went_well;     // 0: a level failed (the pair skips the remaining levels)
    // FUSED arithmetic: the evaluation context (H = K R K^-1, K t: lm_kernels.hip FusedCtx, 21 floats) of the model the NEXT round
    // evaluates at level `lvl` — formed once per pair and round by whoever sets that model (the step kernel, the coarse-level kernel's
    // hand-over) instead of by every thread of every evaluation workgroup — and whether that model is the near-identity case that
    // runs in the exact arithmetic.
    float fctx[21];
    int fctx_exact;
};
#define VORS_SPLIT_MAX_ROUNDS 62
// Threshold of the go-on prediction on the promised decrease of the mean energy, in grey levels squared like the 1.0 of stop_criterion's
// d_energy test (cost-model ESTIMATES from the CPU measurement, profiles/lm_predict_experiments/README.md: 0.75 / 1.0 / 1.25 -> 0.40 / 0.48 /
// 0.42 ms per step)
#define VORS_LM_PREDICT_TAU 1.0f
struct LmSplitWs {
    LmSplitState* state;  // [pairs]
    float* partials;      // [pairs][chunks][32]
    // Active pairs of a round, ping-pong per round. One array holds both kinds: pairs due a FULL evaluation (energy, g, H) fill it
    // from the front, pairs due an ENERGY-only evaluation of a candidate from the back — each kind has its own launch.
    int* list[2];         // [cap]
    int* count;           // [2][VORS_SPLIT_MAX_ROUNDS + 2]: full-kind / energy-kind pairs per round
    int cap;              // capacity of a list = pairs of the handle
    int chunks;           // partial-sum slots per pair = most chunks a pair is cut into; 0 = split path disabled
    int chunks0;          // chunks per pair at level 0 in this launch (level l: chunks0 >> 2l), <= chunks
    int n_split;          // levels 0 .. n_split-1 are solved this way
    int rounds;
    int predict;          // 1: level-0 candidates predicted to go on are evaluated in full at once (LmSplitState::pred); 0: never
    float predict_tau;    // ... those whose step promises a decrease of the mean energy above this (lm_kernels.hip VORS_LM_PREDICT_TAU)
    int* pred_log;        // [cap] what the prediction did with each pair in the last track (VORS_PREDICT_* bits, include/vors_hip.h); null: off
    // SIDE LANE (large dense batches, two levels solved by rounds): the few pairs still iterating at level 1 once everybody else has moved on
    // to level 0 would get ONE cheap evaluation per round while each round lasts milliseconds (level-0 evaluations of 4096 pairs), and then
    // keep ~20 more rounds alive on their own. After round `side_round` the step kernel hands them to a per-pair kernel on a second stream
    // (one 1024-thread workgroup each, all their remaining level-1 iterations back to back, concurrent with the level-0 rounds of the
    // others); they join the rounds again at level 0 (`join_list`, merged into a later round's list).
    int side_round;       // -1: off
    int* side_list;       // [cap] pairs handed to the side lane;  count[SPLIT_SIDE_COUNT] of them
    int* join_list;       // [cap] pairs that finished level 1 there; count[SPLIT_JOIN_COUNT] of them
    hipStream_t side_stream;
    hipEvent_t ev_fork, ev_join;
};
#define SPLIT_SIDE_COUNT (2 * (VORS_SPLIT_MAX_ROUNDS + 2))
#define SPLIT_JOIN_COUNT (2 * (VORS_SPLIT_MAX_ROUNDS + 2) + 1)
#define SPLIT_COUNT_INTS (2 * (VORS_SPLIT_MAX_ROUNDS + 2) + 2)

// Per-pixel inverse-depth planes of the generic-mask keyframe path (all levels).
struct PixelPlanes {
    float* iz;  // NaN = Unknown
    float* v;   // < 0 = Unknown
    int off[VORS_MAX_LEVELS];
    int stride;
    // compaction workspace: usable pixels per chunk of VORS_CHUNK_PX pixels, [pair][chunks_total]; level l owns chunks
    // chunk_off[l] .. chunk_off[l + 1]
    int* counts;
    int chunk_off[VORS_MAX_LEVELS + 1];
    int chunks_total;
};
constexpr int VORS_CHUNK_PX = 4096;  // 256 threads x 16 consecutive pixels

// Image pyramid of a batch: level 0 is the caller's buffer (zero copy), levels >= 1 live in `upper`.
struct Pyramid {
    const uint8_t* level0;  // pair stride S0
    uint8_t* upper;         // pair stride upper_stride
};

void launch_transpose_u8(const uint8_t* src_colmajor, uint8_t* dst_rowmajor, int rows, int cols, int n, hipStream_t s);
void launch_transpose_u16(const uint16_t* src_colmajor, uint16_t* dst_rowmajor, int rows, int cols, int n, hipStream_t s);
void launch_pyramid(const Geom& g, Pyramid pyr, int n_pairs, hipStream_t s);
void launch_zero_ints(const Geom& g, int* base, int stride, int n_pairs, hipStream_t s);  // per-pair counters -> 0 (honours Geom::sel_list)
void launch_keyframe(const Geom& g, Pyramid kf, const uint16_t* depth, Records rec, int n_pairs, hipStream_t s);
void keyframe_region_geometry(const Geom& g, int* kf_r, int* n_regions);  // coarse-to-fine mode: roots per wavefront region, regions per pair
int count_isqrt_u16_mismatches(hipStream_t s);  // dso_kernels.hip: self-check of the gradient-magnitude root (0 = exact for every argument)
void launch_keyframe_dso(const Geom& g, Pyramid kf, const uint16_t* depth, DsoWs ws, uint8_t* mask, PixelPlanes pp, Records rec, int n_pairs,
                         hipStream_t s);
// Inspection: expand the slim records of one level of one pair into record planes (exact arithmetic).
void launch_slim_materialize(const Geom& g, int l, int pair, Records rec, int n, Records out, hipStream_t s);
void launch_dense_materialize(const Geom& g, int l, int pair, Pyramid kf, const uint16_t* depth, Records rec, Records out,
                              hipStream_t s);
// What every LM kernel reads: the two pyramids and the keyframe's records. `kf` and `kf_depth` are read only in dense mode (points are
// recomputed from the keyframe image + depth on the fly).
struct LmScene {
    Pyramid cur, kf;
    const uint16_t* kf_depth;
    Records rec;
};
// One track launch (host side only: the kernels keep their flat argument lists, launch_track below unpacks the record).
struct TrackCall : LmScene {
    const float *prev_poses7, *kf_poses7;
    float* out_poses7;
    int32_t* out_status;
    vors_pair_stats* out_stats;
    int n_pairs;
};
// One evaluation of one level of one pair of a prepared batch at an explicit model -> 29 sums.
struct EvalCall : LmScene {
    int pair, lvl;
    const float* model7;
    float* out29;
};
// One evaluation of one level per (pair, model) of a prepared batch, device-resident (vors_batch_eval_pairs): item i = pair * models_per_pair
// + k reads its model at models + i * model_stride floats and writes out29 + i * 29. The launchers cut the items into slices of at most
// ws.items, the capacity of the handle's workspace; a slice's item `item0 + s` uses slot s of it.
struct EvalPairsCtx {     // FUSED arithmetic: the evaluation context of one item, as LmSplitState keeps it for a pair (same names, same meaning)
    float fctx[21];
    int fctx_exact;
};
struct EvalPairsWs {
    float* partials;      // [items][chunks][32] chunk sums of the levels cut into several workgroups
    EvalPairsCtx* fctx;   // [items]
    float* sums29;        // [max_pairs][29] vors_batch_pose_information's own sums
    int items, chunks;    // capacity: items per slice, chunks per item
};
struct EvalPairsCall : LmScene {
    int n_items, models_per_pair, lvl;
    const float* models;
    int model_stride;     // floats
    int energy_only;      // VORS_EVAL_ENERGY: sums 0 and 1, zeros elsewhere
    float* out29;
    EvalPairsWs ws;
};
// What the kernels of one slice get.
struct EvalPairsArgs {
    int item0, models_per_pair, lvl, chunk_points;
    const float* models;
    int model_stride;
    float* out29;
    float* partials;
    EvalPairsCtx* fctx;
    int ws_chunks;
};
// The per-point quantities of one level per pair of a prepared batch at one model per pair (vors_batch_residual_maps): planes in the
// keyframe pixel geometry of the level, a 256-bin histogram of |residual| and the scale read off it. Every output is nullable.
struct ResidualMapsCall : LmScene {
    int n_pairs, lvl;
    const float* models;
    int model_stride;     // floats
    float* residuals;     // [pair][rows_l * cols_l]
    float* warp_uv;       // [pair][rows_l * cols_l][2]
    uint32_t* hist;       // [pair][VORS_RESIDUAL_BINS]
    float* scale;         // [pair][2] (needs hist)
};
// What the kernel of one slice of pairs gets.
struct ResidualMapsArgs {
    int pair0, lvl, chunk_points;
    const float* models;
    int model_stride;
    float* residuals;
    float* warp_uv;
    uint32_t* hist;
    int wide_stores;      // the planes are 16-byte aligned: a dense quad stores 16 bytes at a time
};
// Depth reprojection of one level per pair of a prepared batch at one model per pair (vors_batch_reproject_depth): the keyframe's points
// warped into the current frame with a z-buffer, and compared with a measured current depth map. Every output is nullable.
struct ReprojectCall : LmScene {
    int n_pairs, lvl;
    const float* models;
    int model_stride;           // floats
    const uint16_t* cur_depth;  // [pair][S0], level 0 only; nullable
    float tol_m;
    float* pred_z;              // [pair][rows_l * cols_l], current frame: min Z' over the points that land, +inf elsewhere
    uint16_t* pred_depth;       // [pair][rows_l * cols_l], current frame (needs pred_z)
    float* residual;            // [pair][rows * cols], keyframe geometry (needs cur_depth)
    uint32_t* counts;           // [pair][4]
};
// What the kernel of one slice of pairs gets.
struct ReprojectArgs {
    int pair0, lvl, chunk_points;
    const float* models;
    int model_stride;
    const uint16_t* cur_depth;
    float tol_m;
    uint32_t* pred_z;           // the plane as bit patterns: Z' > 0 orders as its bits
    float* residual;
    uint32_t* counts;
    int wide_stores;            // the residual plane is 16-byte aligned: a dense quad stores 16 bytes at a time
};
// Point clouds of one level per pair of a prepared batch (vors_batch_point_cloud): the usable points of the level, compacted in ascending
// slot order into lists of `capacity` entries per pair, back-projected and carried to the world frame by one pose per pair. Every output
// is nullable; `ws` is the handle's [pair][ws_chunks] count workspace.
struct PointCloudCall : LmScene {
    int n_pairs, lvl;
    const float* poses;         // camera -> world, nullable = identity (no transform at all)
    int pose_stride;            // floats
    const uint8_t* keep;        // [pair][rows_l * cols_l], nullable = keep everything
    int capacity;
    float* xyz;                 // [pair][capacity][3]
    uint32_t* pixel;            // [pair][capacity] x | y << 16
    uint8_t* gray;              // [pair][capacity]
    uint32_t* counts;           // [pair]
    uint32_t* ws;
    int ws_chunks;
};
// What the kernels of one slice of pairs get.
struct PointCloudArgs {
    int pair0, lvl, chunk_points;
    const float* poses;
    int pose_stride;
    const uint8_t* keep;
    int capacity;
    float* xyz;
    uint32_t* pixel;
    uint8_t* gray;
    uint32_t* counts;
    uint32_t* ws;
    int ws_chunks;
    int wide_keep;              // the mask planes are 4-byte aligned: a dense quad reads its four bytes at once
};
// The voxel filter of that map (vors_trackers_enable_map_voxels): one open-addressing table per sequence, two 64-bit words per entry —
// the voxel key (lie.h voxel_key; empty = all ones) and the tag of the point that owns the voxel (all ones until a point claims it). Only
// the kernels of the filtered emission get this block; the unfiltered ones keep their arguments.
struct PointCloudVoxelArgs {
    float voxel_m = 0.f;
    uint32_t table_slots = 0;       // a power of two
    unsigned long long* table = nullptr;  // [seq][table_slots][2]
    uint32_t* occupied = nullptr;   // [seq] claimed entries
    uint32_t* overflow = nullptr;   // [seq] sticky: a point found no entry in table_slots probes
};
// The statistics of that filter's voxels (vors_trackers_enable_map_voxel_stats), rank-aligned with the lists. Only the two
// kernels the statistics add get this block (the WRITE that also records ranks, and ACCUMULATE); every other kernel keeps its arguments.
struct PointCloudVoxelStatsArgs {
    uint32_t* rank_of = nullptr;    // [seq][table_slots] rank of the voxel of a table entry; all ones: none (yet, or beyond the sweep)
    long long* sums = nullptr;      // [seq][capacity][4] fixed-point offsets x, y, z (lie.h voxel_offset_q) and grey
    uint32_t* obs = nullptr;        // [seq][capacity][2] observations (wraps at 2^32), highest contributing segment index
};
// The keyframe map of the lock-step trackers (vors_trackers_enable_map): the point-cloud pass of one level for the SELECTED sequences
// (Geom::sel_list, null = all), appended to per-sequence lists with one segment record per keyframe. Every buffer is the handle's own.
struct PointCloudAppendCall : LmScene {
    int n_seq, lvl;
    const float* kf_poses;      // [seq][7] keyframe camera -> world, always applied
    const int32_t* kf_frame;    // [seq] keyframe index
    const uint8_t* weight;      // [seq][S0] the depth filter's weights; read only with min_weight >= 2 (level 0)
    int min_weight;
    int capacity, max_keyframes;
    float* xyz;                 // [seq][capacity][3]
    uint32_t* pixel;            // [seq][capacity]
    uint8_t* gray;              // [seq][capacity]
    uint32_t* counts;           // [seq] running total of kept points (saturating)
    vors_map_segment* segments; // [seq][max_keyframes]
    uint32_t* n_segments;       // [seq] keyframes created
    uint32_t* ws;               // [seq][ws_chunks] kept points per chunk of the keyframe being appended
    int ws_chunks;
    PointCloudVoxelArgs voxels; // table == null: no voxel filter, and the launches are exactly the ones above
    PointCloudVoxelStatsArgs voxel_stats;  // rank_of == null: no statistics, and the launches are exactly the filter's
};
// What its kernels get.
struct PointCloudAppendArgs {
    int lvl, chunk_points;
    const float* kf_poses;
    const int32_t* kf_frame;
    const uint8_t* weight;      // null: keep every usable point
    int keep_min;
    int capacity, max_keyframes;
    float* xyz;
    uint32_t* pixel;
    uint8_t* gray;
    uint32_t* counts;
    vors_map_segment* segments;
    uint32_t* n_segments;
    uint32_t* ws;
    int ws_chunks;
    int wide_keep;              // the weight planes are 4-byte aligned: a dense quad reads its four bytes at once
};
// Depth fusion of level 0 of a prepared batch at one model per pair (vors_batch_fuse_depth): the keyframe's points splatted into the
// current frame through a KEYED z-buffer (bits(Z') << 32 | source pixel, one 64-bit minimum per landing point), then merged per current
// pixel with the measured depth (lie.h fuse_depth_pixel). zkey is required; the other outputs are nullable.
struct FuseDepthCall : LmScene {
    int n_pairs;
    const float* models;
    int model_stride;           // floats
    const uint16_t* cur_depth;  // [pair][S0]
    float tol_m;
    const uint8_t* kf_weight;   // [pair][S0], keyframe geometry; nullable = 1 everywhere; 0 removes the point
    int max_weight, fill_min_weight;
    uint64_t* zkey;             // [pair][S0], current frame
    uint16_t* fused_depth;      // [pair][S0], current frame
    uint8_t* fused_weight;      // [pair][S0], current frame
    uint32_t* counts;           // [pair][VORS_FUSE_COUNTS]
};
// What the splat kernel of one slice of pairs gets.
struct FuseSplatArgs {
    int pair0, chunk_points;
    const float* models;
    int model_stride;
    const uint8_t* kf_weight;
    unsigned long long* zkey;
    int wide_weight;            // the weight planes are 4-byte aligned: a dense quad reads its four bytes at once
};
// What the merge kernel of one slice of pairs gets.
struct FuseMergeArgs {
    int pair0, plane;
    float depth_scale, tol_m;
    int max_weight, fill_min_weight;
    const uint64_t* zkey;
    const uint16_t* cur_depth;
    const uint8_t* kf_weight;
    uint16_t* fused_depth;
    uint8_t* fused_weight;
    uint32_t* counts;
    int wide;                   // every plane allows four pixels per thread: 16-byte key loads, 8-byte depth and 4-byte weight accesses
};
// Rendering of world-frame point lists into a camera per sequence (vors_render_points, vors_trackers_render_map; render_kernels.hip): a
// projection-and-splat pass into a KEYED z-buffer (bits(Z') << 32 | rank of the point in its list, one 64-bit minimum per written pixel),
// then an elementwise resolve into a u16 depth map and a u8 grey image (lie.h render_point / render_resolve). Handle-free: everything the
// kernels read is here. zkey is required; the other outputs are nullable.
struct RenderCall {
    int n;                       // sequences
    const float* xyz;            // [n][capacity][3]
    const uint8_t* list_gray;    // [n][capacity]
    const uint32_t* list_counts; // [n]; a count above capacity is clipped to it
    int capacity;
    const uint8_t* ranges;       // nullable = the whole list; (first, count) u32 pairs, range_stride BYTES apart, clipped to the written prefix
    int range_stride;
    Intr k;
    int rows, cols;
    float depth_scale;
    const float* poses;          // camera -> world, nullable = no transform at all
    int pose_stride;             // floats
    int footprint;               // 1, 2 or 3
    uint64_t* zkey;              // [n][rows * cols]
    uint16_t* depth;             // [n][rows * cols]
    uint8_t* gray;               // [n][rows * cols]
    uint32_t* counts;            // [n][VORS_RENDER_COUNTS]
};
// Points per workgroup and trip of the splat, and the cap of its grid's x extent: a longer list goes through the stride loop.
#define RENDER_BLOCK 256
#define RENDER_POINTS 4  // per thread and trip
#define RENDER_MAX_CHUNKS 1024
inline int render_chunks(int capacity) {
    const long long c = ((long long)capacity + RENDER_BLOCK * RENDER_POINTS - 1) / (RENDER_BLOCK * RENDER_POINTS);
    return (int)(c < 1 ? 1 : c > RENDER_MAX_CHUNKS ? RENDER_MAX_CHUNKS : c);
}
// Fill of the key plane, splat, resolve: enqueued on s in this order, not synchronised, no workspace.
void launch_render_points(const RenderCall& call, hipStream_t s);

// Surface normals of level-0 depth planes (vors_depth_normals, vors_points_normals, the keyframe map's normals; normal_kernels.hip): per
// pixel lie.h depth_normal. Handle-free: everything the kernels read is here. The plane form writes every pixel of every plane; the list
// form writes exactly the ranks of each list's clipped range. Each output is nullable (the entries ask for at least one).
struct NormalCall {
    int n;                       // planes / lists
    const uint16_t* depth;       // [n][rows * cols]
    Intr k;
    int rows, cols;
    float depth_scale;
    int step;                    // 1..8
    float jump_m;
    const float* poses;          // camera -> world, nullable = the normal stays in the camera frame; only the rotation is applied
    int pose_stride;             // floats
    float* normals;              // plane form [n][rows * cols][3], list form [n][capacity][3]
    uint32_t* counts;            // [n][VORS_NORMAL_COUNTS]
    // list form only
    const uint32_t* pixel;       // [n][capacity] x | y << 16
    const uint32_t* list_counts; // [n]; a count above capacity is clipped to it
    int capacity;
    const uint8_t* ranges;       // nullable = the whole list; (first, count) u32 pairs, range_stride BYTES apart, clipped to the written prefix
    int range_stride;
    const uint32_t* first;       // nullable; [n] first rank of the range, which then runs to the end of the written prefix (the keyframe map)
    const int* sel_list;         // masked launch (Geom::sel_list): list k of the grid is sel_list[k] for k < *sel_count, nothing beyond
    const int* sel_count;
};
#define NORMAL_BLOCK 256
#define NORMAL_POINTS 4  // pixels per thread of the plane kernel
// The plane form: a memset of the counters when they are asked for, then one kernel; enqueued on s, not synchronised, no workspace.
void launch_depth_normals(const NormalCall& call, hipStream_t s);
// The list form, the same; with sel_list a masked launch whose grid spans all n lists.
void launch_points_normals(const NormalCall& call, hipStream_t s);
// dst[i] = src[i] for the n running totals of the keyframe map (the ranks an emission starts from), honouring nothing: every sequence.
void launch_normals_snapshot(const uint32_t* src, uint32_t* dst, int n, hipStream_t s);

// The sensor front end (vors_undistort_frames, vors_register_depth; frontend_kernels.hip). Handle-free: everything the
// kernels read is here, the cameras, the coefficients and the pose by value. Every output is nullable (the entries ask for what they need).
struct UndistortCall {
    int n;                       // planes
    const uint8_t* gray;         // [n][in_rows * in_cols], nullable
    const uint16_t* depth;       // [n][in_rows * in_cols], nullable
    int in_rows, in_cols;
    Intr k_in;
    Dist5 dist;
    Intr k_out;
    int out_rows, out_cols;
    int border;                  // 0 = zero outside, 1 = edge replicate (grey only)
    uint8_t* gray_out;           // [n][out_rows * out_cols]
    uint16_t* depth_out;         // [n][out_rows * out_cols]
    float* map;                  // [out_rows * out_cols][2], written once (by the first plane's workgroups)
    uint32_t* counts;            // [n][VORS_UNDISTORT_COUNTS]
};
struct RegisterCall {
    int n;                       // planes
    const uint16_t* depth;       // [n][d_rows * d_cols]
    Intr k_d;
    int d_rows, d_cols;
    float scale_in;
    bool has_pose;
    Iso pose;                    // depth camera -> colour camera
    Intr k_c;
    int c_rows, c_cols;
    float scale_out;
    int footprint;               // 1, 2 or 3
    uint64_t* zkey;              // [n][c_rows * c_cols]
    uint16_t* depth_out;         // [n][c_rows * c_cols]
    uint32_t* src_index;         // [n][c_rows * c_cols]
    uint32_t* counts;            // [n][VORS_REGISTER_COUNTS]
};
#define FRONT_BLOCK 256
#define FRONT_POINTS 4  // pixels per thread
// A memset of the counters when they are asked for, then one kernel; enqueued on s, not synchronised, no workspace.
void launch_undistort(const UndistortCall& call, hipStream_t s);
// Fill of the key planes, a memset of the counters when they are asked for, the splat and — with any of depth_out, src_index, counts —
// the resolve: enqueued on s in this order, not synchronised, no workspace.
void launch_register_depth(const RegisterCall& call, hipStream_t s);

// Point-to-plane ICP of world-frame point lists with normals against depth planes (vors_icp_points, vors_trackers_icp_map;
// icp_kernels.hip): per point lie.h icp_landing / icp_row, the sums in lie.h's fixed order, the round's verdict lie.h icp_round.
// Handle-free: everything the kernels read is here; the caller's workspace holds the chunk partials, the chunk counts and the state.
struct IcpState {  // per list, in the workspace
    float pose[7];
    uint32_t status, iterations, frozen;
    float last_step_norm;
    uint32_t pad;
};
struct IcpCall {
    int n;                       // lists
    const float* xyz;            // [n][capacity][3]
    const float* normals;        // [n][capacity][3]
    const uint32_t* list_counts; // [n]; a count above capacity is clipped to it
    int capacity;
    const uint8_t* ranges;       // nullable = the whole list; (first, count) u32 pairs, range_stride BYTES apart, clipped to the written prefix
    int range_stride;
    const float* poses_in;       // camera -> world, required
    int pose_stride;             // floats
    const uint16_t* depth;       // [n][rows * cols]
    Intr k;
    int rows, cols;
    float depth_scale, dist_m, damping, step_eps;
    int iters;
    uint32_t min_points;
    float* partials;             // workspace: [n][icp_chunks(capacity)][VORS_ICP_SUMS]
    uint32_t* chunk_counts;      // workspace: [n][icp_chunks(capacity)]
    IcpState* state;             // workspace: [n]
    float* poses_out;            // [n][7], may alias poses_in
    vors_icp_stats* stats;       // [n], nullable
    float* sums29;               // [n][29], nullable
    float* residuals;            // [n][capacity], nullable
};
#define ICP_BLOCK 256
#define ICP_MAX_CHUNKS 1024  // cap of the evaluation grid's x extent: a longer list goes through the stride loop
constexpr size_t icp_chunks(int capacity) { return ((size_t)capacity + VORS_ICP_CHUNK - 1) / VORS_ICP_CHUNK; }
// The workspace: partials, chunk counts, state, in this order (every part a multiple of 4 bytes): its size, and the three pointers of a call.
inline size_t icp_workspace_bytes(int n, int capacity) {
    return (size_t)n * (icp_chunks(capacity) * (VORS_ICP_SUMS + 1) * 4 + sizeof(IcpState));
}
inline void icp_workspace_carve(IcpCall* call, void* workspace, int n, int capacity) {
    const size_t slots = (size_t)n * icp_chunks(capacity);
    call->partials = static_cast<float*>(workspace);
    call->chunk_counts = reinterpret_cast<uint32_t*>(call->partials + slots * VORS_ICP_SUMS);
    call->state = reinterpret_cast<IcpState*>(call->chunk_counts + slots);
}
// What the robust pass (vors_icp_points_robust; lie.h icp_row_robust / icp_products_robust) reads and writes beyond IcpCall. A record of
// its own: icp_begin_kernel, icp_solve_kernel and the plain evaluation kernels take IcpCall by value, and their arguments stay as they are.
struct IcpRobust {
    const float* frame_normals;  // [n][rows * cols][3], camera frame, three zeros = no normal; nullable = no normal gate
    float min_cos;
    float huber_m;               // 0 = no Huber weight
    uint32_t* gate_counts;       // [n][VORS_ICP_GATE_COUNTS] of the final evaluation, nullable
};
// What the joint pass (vors_icp_points_joint; lie.h icp_photo_footprint / icp_row_photo) reads and writes beyond IcpCall and IcpRobust.
#define ICP_PHOTO_COUNTS VORS_ICP_PHOTO_COUNTS
struct IcpJoint {
    const uint8_t* list_gray;    // [n][capacity]; not read when photo_scale_m == 0
    const uint8_t* frame_gray;   // [n][rows * cols] level 0; not read when photo_scale_m == 0
    float photo_scale_m;         // metres per grey level; 0 = no photometric row: the robust pass
    float photo_huber_m;         // photo_scale_m * photo_huber_grey, taken ONCE on the host; 0 = no Huber weight
    float* photo_residuals;      // [n][capacity] I - grey in grey levels, NaN = not PHOTO, nullable
    uint32_t* photo_counts;      // [n][ICP_PHOTO_COUNTS] of the final evaluation, nullable
};
// The state's start, then per round one evaluation and one solve launch, then the final evaluation and the launch that writes the
// outputs: enqueued on s in this order, not synchronised, no allocation. robust: NULL = the plain pass (vors_icp_points); otherwise the
// robust evaluation kernels, instantiated on (frame normals given, huber_m > 0), after a memset of the gate counts when they are asked for.
// joint (needs robust): the joint evaluation kernels in their place, instantiated on photo_huber_m > 0 as well, after a memset of the
// photo counts when they are asked for.
void launch_icp_points(const IcpCall& call, const IcpRobust* robust, hipStream_t s, const IcpJoint* joint = nullptr);

// Pose-graph optimisation of n graphs side by side (vors_pose_graph_optimize; pose_graph_kernels.hip): the per-edge and
// per-node rules are lie.h pg_*, the order of every sum the one include/vors_hip.h 2g states. Handle-free: everything the kernels read is
// here; the caller's workspace holds the state, the working poses, the incidence lists, the linearisation and the vectors of the solve.
struct PgState {  // per graph, in the workspace
    uint32_t status, frozen, accepted, rejected, cg_spent, valid_edges, skipped_edges, free_nodes, fixed_nodes, isolated_nodes;
    uint32_t cur;         // which of the two pose buffers holds the kept poses
    uint32_t lin_ok;      // the stored linearisation is the kept poses' (the last round was rejected)
    uint32_t singular;    // a block of this round had no factor
    uint32_t cg_done[2];  // slot t & 1: iteration t found the solve ended; written by iteration t's product launch, read by later launches
    uint32_t step2_bits;  // max over the free nodes of dot6(delta, delta) >= 0, as its bits (an integer maximum)
    float lambda, energy, initial_energy, last_step_norm;
};
struct PgCall {
    int n, node_capacity, edge_capacity;
    const float* poses_in;        // [n][node_capacity] poses, pose_stride floats apart
    int pose_stride;
    const uint32_t* node_counts;  // [n]; a count above the capacity is clipped to it
    const uint32_t* edges;        // [n][edge_capacity][2]
    const uint32_t* edge_counts;  // [n], clipped likewise
    const float* meas;            // [n][edge_capacity][7]
    const float* info;            // [n][edge_capacity][36], nullable = identity
    const float* weight;          // [n][edge_capacity], nullable = 1
    const uint8_t* fixed;         // [n][node_capacity], nullable = node 0 of every graph
    float lambda0, step_eps, cg_tol;
    int iters, cg_iters;
    float* poses_out;             // [n][node_capacity][7], may alias poses_in when packed alike
    vors_pose_graph_stats* stats; // [n], nullable
    float* edge_residuals;        // [n][edge_capacity][6], nullable
    float* edge_energy;           // [n][edge_capacity], nullable
    // the workspace, carved by pg_workspace_carve in this order
    double* dots;                 // [n][6][node chunks]: p.q, r.z (two slots), r.r (two slots), r0.r0 chunk sums
    PgState* state;               // [n]
    float* wmat;                  // [n][edge_capacity][36], 16-byte aligned rows
    float* lin;                   // [n][edge_capacity][VORS_PG_LIN]
    float* poses;                 // [n][2][node_capacity][7]
    float *hd, *fac;              // [n][node_capacity][21]
    float *x, *r, *z, *q, *p;     // [n][node_capacity][6]; p: [n][2][node_capacity][6]
    float* energy_part;           // [n][edge chunks]
    uint32_t *edge_ok;            // [n][edge_capacity]
    uint32_t *deg, *cursor, *node_class;  // [n][node_capacity]
    uint32_t* off;                // [n][node_capacity + 1]
    uint32_t *inc_tmp, *inc;      // [n][2 * edge_capacity]: edge << 1 | (0: the node is the edge's i, 1: its j)
};
#define PG_BLOCK 256
#define PG_MAX_CHUNKS 1024  // cap of a grid's x extent: longer graphs go through the stride loop
#define PG_NODE_FREE 0u
#define PG_NODE_FIXED 1u
#define PG_NODE_ISOLATED 2u
constexpr size_t pg_chunks(int capacity) { return ((size_t)capacity + VORS_PG_CHUNK - 1) / VORS_PG_CHUNK; }
// One walk over the workspace's parts for its size and for a call's pointers (call NULL: the size only). Every part is a multiple of 16
// bytes up to `lin`, of 4 bytes after it.
inline size_t pg_workspace_carve(PgCall* call, void* workspace, int n, int node_capacity, int edge_capacity) {
    const size_t g = (size_t)n, N = (size_t)node_capacity, E = (size_t)edge_capacity, nc = pg_chunks(node_capacity), ec = pg_chunks(edge_capacity);
    size_t at = 0;
    auto part = [&](auto** p, size_t bytes) {
        if (call) *p = reinterpret_cast<std::remove_reference_t<decltype(**p)>*>(static_cast<char*>(workspace) + at);
        at += bytes;
    };
    PgCall scratch{};
    PgCall& c = call ? *call : scratch;
    part(&c.dots, g * 6 * nc * sizeof(double));
    part(&c.state, g * sizeof(PgState));
    part(&c.wmat, g * E * 36 * 4);
    part(&c.lin, g * E * VORS_PG_LIN * 4);
    part(&c.poses, g * 2 * N * 7 * 4);
    part(&c.hd, g * N * 21 * 4);
    part(&c.fac, g * N * 21 * 4);
    part(&c.x, g * N * 6 * 4);
    part(&c.r, g * N * 6 * 4);
    part(&c.z, g * N * 6 * 4);
    part(&c.q, g * N * 6 * 4);
    part(&c.p, g * 2 * N * 6 * 4);
    part(&c.energy_part, g * ec * 4);
    part(&c.edge_ok, g * E * 4);
    part(&c.deg, g * N * 4);
    part(&c.cursor, g * N * 4);
    part(&c.node_class, g * N * 4);
    part(&c.off, g * (N + 1) * 4);
    part(&c.inc_tmp, g * 2 * E * 4);
    part(&c.inc, g * 2 * E * 4);
    return at;
}
// The incidence build, the initial energy, per round the linearisation, the gather, 2 cg_iters launches of the solve, the candidates,
// their energy and the verdict, then the final evaluation and the launch that writes the outputs: enqueued on s in this order, every
// launch unconditionally, not synchronised, no allocation.
void launch_pose_graph(const PgCall& call, hipStream_t s);

// Loop closure (vors_loop_signatures, vors_loop_candidates, vors_loop_verify_edges; loop_closure_kernels.hip): the rules are
// lie.h lc_*. Handle-free: everything the kernels read is here. The host twins fill the same records with host pointers.
struct LcMeta {  // vors_loop_sig_meta
    int32_t sum;
    uint32_t sumsq;
};
struct LcCand {  // vors_loop_candidate
    uint32_t i;
    float score;
};
struct LcSigCall {
    int n, rows, cols, tr, tc;
    const uint8_t* gray;  // [n][rows * cols]
    int8_t* sig;          // [n][tr * tc], 16-byte aligned
    LcMeta* meta;         // [n]
};
struct LcCandCall {
    int n, capacity, d;
    const int8_t* sig;          // [n][capacity][d], 16-byte aligned
    const LcMeta* meta;         // [n][capacity]
    const uint32_t* counts_in;  // [n]; a count above the capacity is clipped to it
    const float* poses;         // [n][capacity] poses, pose_stride floats apart; nullable = no pose gate
    int pose_stride;
    const uint32_t* query_first;  // [n], nullable = 0
    uint32_t min_gap, k;
    float min_score, max_dist_m, min_qdot;
    LcCand* cand;           // [n][capacity][k]
    uint32_t* cand_counts;  // [n][capacity]
    uint32_t* counts;       // [n][VORS_LC_COUNTS], nullable; zeroed by the launch
};
struct LcVerifyCall {
    uint32_t m;
    const uint32_t* pairs;  // [m] {i, j}
    const float *fwd, *bwd; // [m] models, fwd_stride / bwd_stride floats apart; bwd nullable
    int fwd_stride, bwd_stride;
    const int32_t *status_fwd, *status_bwd;  // [m]; status_bwd nullable
    const float* info;      // [m][36], nullable = identity rows written
    const float* poses;     // [node_count] poses, pose_stride floats apart; nullable
    int pose_stride;
    uint32_t node_count;
    float max_cycle_trans, max_cycle_rot, max_prior_trans, max_prior_rot, weight;
    uint32_t* edges;        // [edge_capacity] {i, j}
    float* meas;            // [edge_capacity][7]
    float* info_out;        // [edge_capacity][36], nullable
    float* edge_weight;     // [edge_capacity], nullable
    uint32_t* edge_count;   // [1] in / out
    uint32_t edge_capacity;
    uint32_t* verdict;      // [m]
    float* residuals;       // [m][12], nullable
    uint32_t* counts;       // [VORS_LC_VERDICTS], nullable
};
// Each is enqueued on s, not synchronised, no allocation: one launch for the signatures (a workgroup per plane); a memset of the counts
// (when asked for) and one launch for the candidates (a workgroup per tile of 32 queries and set); one launch of ONE workgroup for the
// verification, whose ordered compaction is a scan over chunks of 1024 candidates in sequence. launch_loop_candidates -> the memset's
// error, with nothing launched behind a memset that failed.
void launch_loop_signatures(const LcSigCall& call, hipStream_t s);
hipError_t launch_loop_candidates(const LcCandCall& call, hipStream_t s);
void launch_loop_verify(const LcVerifyCall& call, hipStream_t s);

// The map ICP correction at keyframe promotion (vors_trackers_enable_map_icp; map_icp_kernels.hip): what surrounds
// launch_icp_points there. Handle-free: everything the kernels read is here.
struct MapIcpCall {
    int n;                           // sequences
    const int* promo_list;           // the promotion list of this track call and its length, on the device
    const int* promo_count;
    const int32_t* kf_frame;         // [n] frame index of every sequence's keyframe (the new one for a promoted sequence)
    const uint32_t* counts;          // the map as it stands BEFORE this promotion's emission: running totals, segment records and counts
    const vors_map_segment* segments;
    const uint32_t* n_segments;
    int capacity, max_keyframes, last_keyframes;
    MapIcpGates gates;
    float *kf_poses, *cur_poses, *out_poses;  // [n][7] the tracker's pose tables: read by ARM, written by APPLY for an accepted sequence
    uint32_t* promoted;              // [n] staging: 1 = on the promotion list of this call
    uint32_t* ranges;                // [n][2] the window, (0, 0) for a sequence that is not promoted
    float *start_poses, *result_poses;        // [n][7] the ICP's input and output
    vors_icp_stats* stats;           // [n] staging of the ICP's outputs
    uint32_t* gate_counts;           // [n][VORS_ICP_GATE_COUNTS]
    vors_map_icp_record* records;    // [n]
    uint32_t* totals;                // [n][2] attempted, accepted
};
// ARM: one thread per sequence — promoted flag, window, start pose, the record reset to NOT_ATTEMPTED. Enqueued on s.
void launch_map_icp_arm(const MapIcpCall& call, hipStream_t s);
// APPLY: one thread per entry of the promotion list — the verdict, the write-back of an accepted pose, the record, the totals.
void launch_map_icp_apply(const MapIcpCall& call, hipStream_t s);
// The plane form of the normals pass for the sequences of call.sel_list only (required here), without a pose and without counts: per
// pixel lie.h depth_normal, the text and the bits of launch_depth_normals, whose kernel knows no selection and stays as it is.
void launch_map_icp_frame_normals(const NormalCall& call, hipStream_t s);
// The correction through the joint pass with the condition test (vors_trackers_enable_map_icp_joint): what its two
// kernels read and write beyond MapIcpCall. A record of its own: map_icp_arm_kernel and map_icp_apply_kernel take MapIcpCall by value,
// and their arguments stay as they are.
struct MapIcpJointCall {
    MapIcpCall c;
    MapIcpConditionGates condition;
    const float* sums29;                       // [n][29] staging of the pass's final sums
    const uint32_t* photo_counts;              // [n][VORS_ICP_PHOTO_COUNTS] staging
    vors_map_icp_joint_record* joint_records;  // [n]
};
// ARM's second half: one thread per sequence, the joint record reset to zeros (map_icp_arm_kernel itself is launched by launch_map_icp_arm).
void launch_map_icp_arm_joint(const MapIcpJointCall& call, hipStream_t s);
// APPLY of the joint stage, in launch_map_icp_apply's place: lie.h icp_condition on the staged sums, lie.h map_icp_verdict_joint, the plain
// record exactly as APPLY writes it, the joint record, the totals, the write-back of an accepted pose.
void launch_map_icp_apply_joint(const MapIcpJointCall& call, hipStream_t s);
// [n][29] sums -> [n][2] dilutions and [n] flags (nullable) (lie.h icp_condition), one thread per system; enqueued on s.
void launch_icp_condition(const float* sums29, int n, float* dilution2, int32_t* flags, hipStream_t s);

// Points per workgroup of an evaluation pass: a level of more points is cut into ceil(points / this) chunks of equal size, a function of
// the level's point count alone — never of the batch — so that the order of the additions belongs to the level.
inline int eval_pairs_chunk_points(const Geom& g) { return g.mode == VORS_CANDIDATES_DENSE ? 16384 : 4096; }
// Chunks of the grid at a level. Coarse-to-fine and dense: the level's point count. DSO: n_slots is the capacity of a list (65536), which
// no list comes near: the selector aims at 2000 candidates and runs again with a wider net beyond 4x that, so the grid is sized for
// 8000; a longer list is evaluated whole all the same, cut into that many (larger) chunks by the kernel.
inline int eval_pairs_chunks(const Geom& g, int lvl) {
    const int cp = eval_pairs_chunk_points(g);
    const int points = g.mode == VORS_CANDIDATES_DSO ? (g.lv[lvl].n_slots < 8000 ? g.lv[lvl].n_slots : 8000) : g.lv[lvl].n_slots;
    return points > cp ? (points + cp - 1) / cp : 1;
}
// THE place where the records become kernel arguments: K(g, scene..., extra...), K(g, scene..., poses and outputs..., extra...).
template <class K, class... Extra>
void launch_on_scene(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Geom& g, const LmScene& c, Extra... extra) {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, g, c.cur.level0, c.cur.upper, c.kf.level0, c.kf.upper, c.kf_depth, c.rec, extra...);
}
template <class K, class... Extra>
void launch_track(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Geom& g, const TrackCall& c, Extra... extra) {
    launch_on_scene(kernel, grid, block, lds, s, g, c, c.prev_poses7, c.kf_poses7, c.out_poses7, c.out_status, c.out_stats, extra...);
}
template <class K>
void launch_eval(K kernel, dim3 block, hipStream_t s, const Geom& g, const EvalCall& c) {
    launch_on_scene(kernel, dim3(1), block, 0, s, g, c, c.pair, c.lvl, c.model7, c.out29);
}
inline EvalPairsArgs eval_pairs_args(const Geom& g, const EvalPairsCall& c, int item0) {
    return EvalPairsArgs{item0, c.models_per_pair, c.lvl, eval_pairs_chunk_points(g), c.models, c.model_stride, c.out29, c.ws.partials, c.ws.fctx, c.ws.chunks};
}
template <class K>
void launch_eval_pairs(K kernel, dim3 grid, dim3 block, hipStream_t s, const Geom& g, const EvalPairsCall& c, int item0) {
    launch_on_scene(kernel, grid, block, 0, s, g, c, eval_pairs_args(g, c, item0));
}
// Run-time value -> template argument: f receives a std::integral_constant, `decltype(x)::value` is the compile-time constant.
//   with_bool(huber, [&](auto h) { launch(kernel<decltype(h)::value>); });
template <class F>
void with_bool(bool v, F&& f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}
// f(pair0, np) for every slice of at most 32768 pairs (the y extent of a grid), in index order
template <class F>
void for_pair_slices(int n_pairs, F&& f) {
    for (int pair0 = 0; pair0 < n_pairs; pair0 += 32768) f(pair0, n_pairs - pair0 < 32768 ? n_pairs - pair0 : 32768);
}
// ... the first of the candidates (descending) that v reaches, the last one otherwise
template <int First, int... Rest, class F>
void with_largest_reached(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, First>{});
    else if (v >= First) f(std::integral_constant<int, First>{});
    else with_largest_reached<Rest...>(v, f);
}

void launch_lm_track(const Geom& g, const TrackCall& call, int block, LmSplitWs split, hipStream_t s);
// the two arithmetic modes of the above (lm_kernels.hip compiled with VORS_FUSED = 0 / 1)
void launch_lm_track_exact(const Geom& g, const TrackCall& call, int block, LmSplitWs split, hipStream_t s);
void launch_lm_track_fused(const Geom& g, const TrackCall& call, int block, LmSplitWs split, hipStream_t s);
// REFERENCE arithmetic (lm_reference.hip): the candidate lists of n_pairs pairs into extract_z's column-major order (no-op in dense mode;
// honours Geom::sel_list), and the tracker with the reference's sequential sums.
void launch_sort_colmajor(const Geom& g, Records rec, int n_pairs, hipStream_t s);
bool ref_rank_from_regions(const Geom& g, const Records& rec);  // coarse-to-fine: launch_sort_colmajor ranks the staged regions itself (no compaction first)
// dense mode: the column-major planes of the keyframe side (pyramid, depth map, inverse depths of levels >= 1; honours Geom::sel_list) and
// of the current frame's pyramid -> rec.dense_t
void launch_ref_dense_planes_keyframe(const Geom& g, Pyramid kf, const uint16_t* depth, Records rec, int n_pairs, hipStream_t s);
void launch_ref_dense_planes_current(const Geom& g, Pyramid cur, Records rec, int n_pairs, hipStream_t s);
// What the handle's device offers the workgroup-per-pair kernel: compute units and LDS per CU (MI355X: 256 CUs, 160 KB). Resolved once per
// handle, on its device, when it is created (a process may hold handles on devices of different sizes); host side only.
struct RefDevice {
    int cus = 256;
    size_t lds_per_cu = 64 * 1024;
};
RefDevice query_ref_device(int device);
void launch_lm_track_reference(const Geom& g, const TrackCall& call, const RefDevice& dev, hipStream_t s);
void launch_lm_eval_level_reference(const Geom& g, const EvalCall& call, hipStream_t s);
void launch_lm_eval_obs_reference(Intr k, int rows, int cols, const uint8_t* image, int n, Records rec, float huber_delta, const float* model7,
                                  float* out_energy_n_g_h, float* residuals, hipStream_t s);
void launch_lm_solve_obs_reference(Intr k, int rows, int cols, const uint8_t* image, int n, Records rec, float huber_delta, const float* model7,
                                   float* out, hipStream_t s);
// One evaluation of one level of one pair of a prepared batch at an explicit model, per arithmetic mode -> 29 sums.
void launch_lm_eval_level_exact(const Geom& g, const EvalCall& call, hipStream_t s);
void launch_lm_eval_level_fused(const Geom& g, const EvalCall& call, hipStream_t s);
// One evaluation of one level per (pair, model), per arithmetic mode -> [item][29] sums on the device, enqueued, not synchronised.
void launch_lm_eval_pairs_exact(const Geom& g, const EvalPairsCall& call, hipStream_t s);
void launch_lm_eval_pairs_fused(const Geom& g, const EvalPairsCall& call, hipStream_t s);
void launch_lm_eval_pairs_reference(const Geom& g, const EvalPairsCall& call, hipStream_t s);
// [n][29] sums -> information matrix, covariance, sigma^2, flags (lie.h pose_information), one thread per pair; outputs nullable
void launch_pose_information(const float* sums29, int n, float* info36, float* cov36, float* sigma2, int32_t* flags, hipStream_t s);
// Residuals, warp field, |residual| histogram and its scale of one level per pair, in the reference's per-point arithmetic whatever the
// handle's (product_kernels.hip lm_residual_maps_kernel, residual_scale_kernel): enqueued, not synchronised, no workspace.
void launch_lm_residual_maps(const Geom& g, const ResidualMapsCall& call, hipStream_t s);
// Z-buffered forward warp of the keyframe's depth into the current frame, its u16 depth map, the geometric residual against a measured
// current depth and the four counts, in the reference's per-point arithmetic whatever the handle's (product_kernels.hip
// lm_reproject_depth_kernel, pred_depth_kernel): enqueued, not synchronised, no workspace. Reads no current image.
void launch_lm_reproject_depth(const Geom& g, const ReprojectCall& call, hipStream_t s);
// Keyed z-buffer splat of level 0 and the per-pixel merge with the measured depth, in the reference's per-point arithmetic whatever the
// handle's (product_kernels.hip lm_fuse_splat_kernel, fuse_depth_kernel): enqueued, not synchronised, no workspace. Reads no current image.
void launch_lm_fuse_depth(const Geom& g, const FuseDepthCall& call, hipStream_t s);
// The same pass as MASKED launches (the depth filter of vors_trackers): only the sequences of g.sel_list take part, their key planes
// are filled by a masked launch too; call.n_pairs is the extent of the pair dimension (all sequences). Every plane of the call is
// required, no counts.
void launch_lm_fuse_depth_selected(const Geom& g, const FuseDepthCall& call, hipStream_t s);
// Ordered stream compaction of the usable (and kept) points of one level per pair into point lists in the world frame (product_kernels.hip
// point_cloud_kernel: a counting launch into call.ws, then a ranking and writing launch; no workgroup waits for another): enqueued, not
// synchronised. Reads no current image.
void launch_lm_point_cloud(const Geom& g, const PointCloudCall& call, hipStream_t s);
// The same pass as MASKED launches that APPEND (the keyframe map of vors_trackers; product_kernels.hip point_cloud_append_kernel,
// point_cloud_commit_kernel): count, write behind the sequence's running total, commit the segment record and the totals. call.n_seq is
// the extent of the pair dimension (all sequences); only the sequences of g.sel_list (null: all) are touched. With call.voxels.table set
// the emission is CLAIM, COUNT, WRITE of point_cloud_append_voxel_kernel and the same commit. With call.voxel_stats.rank_of set as well,
// WRITE is point_cloud_append_voxel_stats_kernel's, which records ranks, and its ACCUMULATE follows in front of the commit.
void launch_lm_point_cloud_append(const Geom& g, const PointCloudAppendCall& call, hipStream_t s);
// The resolve of voxel statistics into an averaged list (vors_voxel_means, vors_trackers_map_voxel_means; product_kernels.hip
// voxel_means_kernel): per rank below the clipped count lie.h voxel_mean. Handle-free: everything the kernel reads is here. The first
// segment of a rank comes from `first_segment` (one word per rank), or from `segments` by a binary search over their `first` (the
// handle's own map), or from nowhere (both null: no span test). Each output is nullable.
// The WINDOWED form (launch_voxel_means_window; the means of the map ICP correction, vors_trackers_enable_map_icp_means): the same body
// over the ranks [first, first + len) of `ranges`, clipped to the clipped count, instead of [0, clipped count); `kept` is then not read,
// the count goes into `records`, and a list whose window is empty is left by its workgroups at once.
struct VoxelMeansCall {
    int n;                              // lists
    const float* xyz;                   // [n][capacity][3]
    const uint32_t* list_counts;        // [n]; a count above capacity is clipped to it
    int capacity;
    const long long* sums;              // [n][capacity][4]
    const uint32_t* obs;                // [n][capacity][2]
    float voxel_m;
    uint32_t min_count, min_span;
    const uint32_t* first_segment;      // [n][capacity], nullable
    const vors_map_segment* segments;   // [n][max_keyframes], nullable
    const uint32_t* n_segments;         // [n], with segments
    int max_keyframes;
    float* xyz_mean;                    // [n][capacity][3]
    uint8_t* gray_mean;                 // [n][capacity]
    uint32_t* kept;                     // [n]
    const uint32_t* ranges;             // [n][2] (first, len) per list: the windowed form only
    vors_map_icp_means_record* records; // [n] {resolved = len, kept}: the windowed form only
};
// The clear of `kept` and one launch: enqueued on s, not synchronised, no workspace.
void launch_voxel_means(const VoxelMeansCall& call, hipStream_t s);
// The windowed form: the clear of `records` and one launch over call.n lists; ranges, records, segments, xyz_mean and gray_mean required.
void launch_voxel_means_window(const VoxelMeansCall& call, hipStream_t s);
// Re-posing of point lists after pose-graph optimisation (vors_repose_points, vors_trackers_repose_map; repose_kernels.hip
// repose_points_kernel, repose_segments_kernel): per rank lie.h repose_point / repose_normal with the two poses of its segment.
// Handle-free: everything the kernels read is here. xyz_out / normals_out / segments_out may be exactly xyz / normals / segments.
struct ReposeCall {
    int n;                             // lists
    const float* xyz;                  // [n][capacity][3]
    const float* normals;              // [n][capacity][3], nullable
    const uint32_t* list_counts;       // [n]; a count above capacity is clipped to it
    int capacity;
    const vors_map_segment* segments;  // [n][max_keyframes]
    const uint32_t* n_segments;        // [n]; clipped to max_keyframes
    int max_keyframes;
    const float* poses_new;            // [n][node_capacity] poses, pose_stride floats apart
    int pose_stride, node_capacity;
    const uint32_t* node_counts;       // [n]; clipped to node_capacity
    const uint32_t* node_of_segment;   // [n][max_keyframes], nullable = segment k is node k
    float* xyz_out;                    // nullable
    float* normals_out;                // nullable
    vors_map_segment* segments_out;    // nullable
    uint32_t* counts_out;              // [n][VORS_REPOSE_COUNTS], nullable
};
// The clear of counts_out, the point pass and, with segments_out or counts_out, the record pass behind it: enqueued on s, not
// synchronised, no workspace.
void launch_repose_points(const ReposeCall& call, hipStream_t s);
// The voxel filter of plain point lists (vors_voxel_filter_points; repose_kernels.hip voxel_filter_*_kernel): EMPTY, CLAIM, COUNT, SCAN,
// WRITE and, with segments_out, SEGMENTS, through voxel_table_device.h's probes with the rank as the tag. table / chunk_counts /
// occupied are carved from the caller's workspace (voxel_filter_workspace_carve).
#define VORS_VFILTER_CHUNK 1024
struct VoxelFilterCall {
    int n;
    const float* xyz;                  // [n][capacity][3]
    const uint32_t* list_counts;       // [n]
    int capacity;
    float voxel_m;
    int table_slots;
    unsigned long long* table;         // [n][table_slots][2]
    uint32_t* chunk_counts;            // [n][chunks]
    uint32_t* occupied;                // [n]
    int chunks;                        // ceil(capacity / VORS_VFILTER_CHUNK)
    uint32_t* index;                   // [n][capacity]
    uint32_t* counts_out;              // [n]
    uint32_t* overflow;                // [n]
    const uint32_t* pixel;             // gathers, each pair nullable
    const uint8_t* gray;
    const float* normals;
    float* xyz_out;
    uint32_t* pixel_out;
    uint8_t* gray_out;
    float* normals_out;
    const vors_map_segment* segments;  // [n][max_keyframes], nullable
    const uint32_t* n_segments;
    int max_keyframes;
    vors_map_segment* segments_out;
};
// Bytes of the workspace; with `call` and `workspace` also sets call->table, chunk_counts, occupied and chunks.
size_t voxel_filter_workspace_carve(VoxelFilterCall* call, void* workspace, int n, int capacity, int table_slots);
void launch_voxel_filter_points(const VoxelFilterCall& call, hipStream_t s);
// Operator level on explicit observations of one level (device buffers): eval at `model` -> out29 partial sums layout:
// [0]=sum r^2 (or Huber loss), [1]=n_inside (as float), [2..7]=g, [8..28]=H upper triangle row-wise.
void launch_lm_eval_obs(Intr k, int rows, int cols, const uint8_t* image, int n, Records rec, float huber_delta,
                        const float* model7, float* out_energy_n_g_h /* 44 floats: e, n, g6, H36 */, float* residuals,
                        hipStream_t s);
void launch_lm_solve_obs(Intr k, int rows, int cols, const uint8_t* image, int n, Records rec, float huber_delta,
                         const float* model7, float* out /* model7, nb_iter, energy, lm_coef, status */, hipStream_t s);
// Records from explicit (x, y, idepth, jac, template) arrays: operator-level entry.
void launch_records_from_obs(Intr k, int rows, int cols, const uint8_t* tmpl, int n, const int32_t* xy, const float* iz,
                             const float* jac, Records rec, hipStream_t s);
// Exhaustive device check of div_uniform for divisor d (all 2^23 significands); returns true when it is exact.
bool verify_fastdiv(float d, float r, hipStream_t s);
// Exhaustive device check of idepth_of<true>(scale, d) == scale / d for d = 1 .. 65535.
bool verify_fast_idepth(float scale, hipStream_t s);
// depth -> (inverse depth, its reciprocal) table, 65536 float2 entries (dense mode, level 0).
void launch_build_depth_lut(float depth_scale, float2* lut, hipStream_t s);
void launch_synth_pairs(uint64_t seed0, int n_pairs, int rows, int cols, const double cam5[5], double motion_scale,
                        int invalid_percent, uint8_t* kf_gray, uint16_t* kf_depth, uint8_t* cur_gray, uint16_t* cur_depth,
                        float* gt_models7, hipStream_t s);

// Sequence tooling + the device side of vors_trackers_* (kernels.hip).
void launch_synth_frames(const void* d_frames /* {u64 seed, u64 salt, f64 xi[6]} x n */, int n_frames, int rows, int cols, const double cam5[5],
                         int invalid_percent, uint8_t* gray, uint16_t* depth, hipStream_t s);
void launch_tracker_pack_out(const float* pose7, const int32_t* status, const int32_t* kf_frame, const vors_pair_stats* stats, void* out,
                             hipStream_t s);
void launch_trackers_advance(int n_seq, int* frame_counter, const float* out_poses7, const vors_pair_stats* stats, float* cur_poses7,
                             float* kf_poses7, int32_t* kf_frame, int* promo_list, int* promo_count, hipStream_t s);
void launch_identity_poses(float* a, float* b, int n, hipStream_t s);  // two pose tables -> identity (inverse_compositional.rs:86-99)
void launch_promote_copy(const Geom& g, const void* src, size_t src_stride, void* dst, size_t dst_stride, size_t bytes, int n_pairs,
                         hipStream_t s);
void launch_depth_weight_init(const uint16_t* depth, uint8_t* weight, size_t n, hipStream_t s);  // weight = depth != 0

}  // namespace vors
