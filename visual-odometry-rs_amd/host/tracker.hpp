// C++ host-side mirror of the reference's tracking interface over the C ABI (include/vors_hip.h):
//   vors::Intrinsics                       reference src/core/camera.rs:84-91
//   vors::track::Config / Config::init     src/core/track/inverse_compositional.rs:37-49, 74-100
//   vors::track::Tracker::track / current_frame                      inverse_compositional.rs:170-248
//   vors::track::LMOptimizerState          src/core/track/lm_optimizer.rs:16-193, host-driven through the operator-level
//                                          entry points (eval on the device, step/stop on the host) — the shape a user
//                                          implementing the optimizer trait themselves would follow.
// Same names, argument meaning and error behaviour as the reference: track() returns void (failures keep the pose and
// are logged to stderr like the reference's eprintln!s); programmer errors (image too small for nb_levels) throw, where
// the reference panics.
#pragma once
#include <algorithm>
#include <array>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/vors_hip.h"
#include "optimizer.hpp"

namespace vors {

// Rust `{}` (Display) for floats: the shortest digits that round-trip, positional notation, `1.0` prints as `1`
// (what eprintln!("Optical_flow: {}", ..) and the trajectory writer tum_rgbd.rs:78-85 produce).
template <class T>
inline std::string rust_display(T v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    char buf[512];
    auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

using Float = float;              // src/misc/type_aliases.rs:10
using Iso3 = std::array<float, 7>;  // tx ty tz qx qy qz qw
using Vec6 = std::array<float, 6>;
using Mat6 = std::array<float, 36>;  // row-major

struct Intrinsics {  // camera.rs:84-91
    std::pair<Float, Float> principal_point;
    std::pair<Float, Float> focal;
    Float skew;
};

namespace tum_rgbd {  // src/dataset/tum_rgbd.rs:15-52
constexpr Float DEPTH_SCALE = 5000.0f;
inline Intrinsics INTRINSICS_ICL_NUIM() { return {{319.5f, 239.5f}, {481.20f, -480.00f}, 0.0f}; }
inline Intrinsics INTRINSICS_FR1() { return {{318.643040f, 255.313989f}, {517.306408f, 516.469215f}, 0.0f}; }
inline Intrinsics INTRINSICS_FR2() { return {{325.141442f, 249.701764f}, {520.908620f, 521.007327f}, 0.0f}; }
inline Intrinsics INTRINSICS_FR3() { return {{320.106653f, 247.632132f}, {535.433105f, 539.212524f}, 0.0f}; }
}  // namespace tum_rgbd

inline void check(vors_status st) {
    if (st != VORS_OK) throw std::runtime_error(std::string("vors_hip: ") + vors_last_error());
}

// A row-major or column-major image view (the reference passes nalgebra DMatrix = column-major).
template <class T>
struct ImageView {
    const T* data;
    int rows, cols;
    int layout;  // VORS_ROW_MAJOR / VORS_COL_MAJOR
};

namespace track {

class Tracker;

struct Config {  // inverse_compositional.rs:37-49
    std::size_t nb_levels;
    std::uint16_t candidates_diff_threshold;
    Float depth_scale;
    Intrinsics intrinsics;
    Float idepth_variance;
    // extensions (zero = reference behaviour)
    int candidates_mode = VORS_CANDIDATES_COARSE_TO_FINE;
    Float huber_delta = 0.0f;
    int arithmetic = VORS_ARITH_REFERENCE;  // the reference's arithmetic and summation order (bit-identical poses); VORS_ARITH_FUSED: the fastest, poses within 1e-4 but for a measured tail (include/vors_hip.h)

    vors_config to_c() const {
        return vors_config{(int32_t)nb_levels, (int32_t)candidates_diff_threshold, depth_scale, intrinsics.principal_point.first,
                           intrinsics.principal_point.second, intrinsics.focal.first, intrinsics.focal.second, intrinsics.skew,
                           idepth_variance, candidates_mode, huber_delta, arithmetic};
    }
    // Config::init (inverse_compositional.rs:74-100)
    Tracker init(double keyframe_depth_timestamp, ImageView<std::uint16_t> depth_map, double keyframe_img_timestamp,
                 ImageView<std::uint8_t> img) const;
};

class Tracker {  // inverse_compositional.rs:31-34
   public:
    Tracker(const Tracker&) = delete;
    Tracker& operator=(const Tracker&) = delete;
    Tracker(Tracker&& o) noexcept
        : h_(o.h_), rows_(o.rows_), cols_(o.cols_), layout_(o.layout_), log_(o.log_), map_capacity_(o.map_capacity_),
          map_max_keyframes_(o.map_max_keyframes_) {
        o.h_ = nullptr;
    }
    ~Tracker() { vors_tracker_destroy(h_); }

    // Tracker::track (inverse_compositional.rs:170-240): returns () like the reference.
    void track(double depth_time, ImageView<std::uint16_t> depth_map, double img_time, ImageView<std::uint8_t> img) {
        // the C ABI carries no dimensions after create(): a smaller frame would be read past its end
        if (depth_map.rows != rows_ || depth_map.cols != cols_ || img.rows != rows_ || img.cols != cols_)
            throw std::invalid_argument("Tracker::track: frame shape differs from the keyframe's");
        if (depth_map.layout != layout_ || img.layout != layout_) throw std::invalid_argument("Tracker::track: layout differs from init's");
        int status = 0;
        double keyframe_depth_timestamp = 0;
        Iso3 keyframe_pose_before;
        check(vors_tracker_keyframe(h_, &keyframe_depth_timestamp, keyframe_pose_before.data()));
        check(vors_tracker_track_checked(h_, depth_time, depth_map.data, img_time, img.data, img.rows, img.cols, &status));
        vors_pair_stats s;
        check(vors_tracker_last_stats(h_, &s));
        last_ = s;
        last_status_ = status;
        if (log_) {
            if (status != VORS_TRACK_OK) std::fprintf(stderr, "Error at Cholesky decomposition of hessian\n");  // :196
            // the reference's own lines, with Rust's float Display (inverse_compositional.rs:222,228-229)
            std::fprintf(stderr, "Optical_flow: %s\n", rust_display(s.optical_flow).c_str());
            if (s.change_keyframe)
                std::fprintf(stderr, "Changing keyframe after: %s seconds\n", rust_display(depth_time - keyframe_depth_timestamp).c_str());
        }
    }
    // Tracker::current_frame (inverse_compositional.rs:243-248): (depth timestamp, pose)
    std::pair<double, Iso3> current_frame() const {
        double t = 0;
        Iso3 p;
        check(vors_tracker_current_frame(h_, &t, p.data()));
        return {t, p};
    }
    const vors_pair_stats& last_stats() const { return last_; }
    int last_status() const { return last_status_; }
    void set_logging(bool on) { log_ = on; }
    // Extension: the recursive depth filter across keyframe promotions (vors_tracker_enable_depth_filter). Before the first track().
    void enable_depth_filter(Float tol_m, int max_weight = 255, int fill_min_weight = 0) {
        check(vors_tracker_enable_depth_filter(h_, tol_m, max_weight, fill_min_weight));
    }
    // Extension: the keyframe map (vors_tracker_enable_map): the cloud of every keyframe, appended on the device. Before the first
    // track(), after enable_depth_filter when min_weight >= 2.
    void enable_map(int level, int capacity, int max_keyframes, int min_weight = 0) {
        check(vors_tracker_enable_map(h_, level, capacity, max_keyframes, min_weight));
        map_capacity_ = capacity;
        map_max_keyframes_ = max_keyframes;
    }
    struct Map {
        std::vector<Float> xyz;               // [points][3], keyframe after keyframe
        std::vector<std::uint32_t> pixel;     // x | y << 16
        std::vector<std::uint8_t> gray;
        std::vector<vors_map_segment> segments;
        std::uint32_t count = 0, n_segments = 0;  // the UNCLIPPED totals: count > xyz.size() / 3 means the capacity was exceeded
    };
    // The map so far (vors_tracker_read_map; synchronises): at most `capacity` points and `max_segments` records.
    Map read_map(int capacity = 0x7fffffff, int max_segments = 0x7fffffff) {
        Map m;
        check(vors_tracker_read_map(h_, 0, nullptr, nullptr, nullptr, &m.count, 0, nullptr, &m.n_segments));  // the totals first
        // (nothing beyond the handle's own capacity was ever written)
        const size_t np = std::min<size_t>(m.count, (size_t)std::max(std::min(capacity, map_capacity_), 0));
        const size_t ns = std::min<size_t>(m.n_segments, (size_t)std::max(std::min(max_segments, map_max_keyframes_), 0));
        m.xyz.resize(3 * np);
        m.pixel.resize(np);
        m.gray.resize(np);
        m.segments.resize(ns);
        std::uint32_t count = 0, n_segments = 0;
        check(vors_tracker_read_map(h_, (int)np, m.xyz.data(), m.pixel.data(), m.gray.data(), &count, (int)ns, m.segments.data(), &n_segments));
        return m;
    }

    // Extension: the voxel filter of the keyframe map (vors_tracker_enable_map_voxels): one point per voxel of edge voxel_m, the first in
    // the map's order. After enable_map, before the first track(); empties the map and emits keyframe 0 again, through the filter.
    void enable_map_voxels(Float voxel_m, int table_slots) { check(vors_tracker_enable_map_voxels(h_, voxel_m, table_slots)); }
    struct MapVoxels {
        std::uint32_t occupied = 0, overflow = 0;  // distinct voxels so far; non-zero once they outgrew table_slots
    };
    // The filter's counters (vors_tracker_read_map_voxels; synchronises).
    MapVoxels read_map_voxels() {
        MapVoxels v;
        check(vors_tracker_read_map_voxels(h_, &v.occupied, &v.overflow));
        return v;
    }
    // Extension: statistics of the map's voxels (vors_tracker_enable_map_voxel_stats): per rank fixed-point sums of every observation of
    // its voxel, the sum of their greys, their number and the last segment that saw it. After enable_map_voxels, before
    // enable_map_normals and the first track(); empties the map and emits keyframe 0 again, counted.
    void enable_map_voxel_stats() { check(vors_tracker_enable_map_voxel_stats(h_)); }
    struct MapVoxelMeans {
        std::vector<Float> xyz_mean;          // [ranks][3]; NaN = the rank was rejected
        std::vector<std::uint8_t> gray_mean;  // [ranks]
        std::vector<std::uint32_t> obs;       // [ranks][2] observations, last segment (vors_tracker_read_map_voxel_stats)
        std::uint32_t kept = 0;
    };
    // The averaged map, rank for rank read_map(capacity)'s points (vors_tracker_map_voxel_means; synchronises): centroids and mean grey
    // of the ranks seen at least min_count times over at least min_span segments.
    MapVoxelMeans map_voxel_means(std::uint32_t min_count = 1, std::uint32_t min_span = 0, int capacity = 0x7fffffff) {
        std::uint32_t count = 0, n_segments = 0;
        check(vors_tracker_read_map(h_, 0, nullptr, nullptr, nullptr, &count, 0, nullptr, &n_segments));
        const size_t np = std::min<size_t>(count, (size_t)std::max(std::min(capacity, map_capacity_), 0));
        MapVoxelMeans m;
        m.xyz_mean.resize(3 * np);
        m.gray_mean.resize(np);
        m.obs.resize(2 * np);
        check(vors_tracker_map_voxel_means(h_, min_count, min_span, (int)np, m.xyz_mean.data(), m.gray_mean.data(), &m.kept));
        check(vors_tracker_read_map_voxel_stats(h_, (int)np, nullptr, m.obs.data()));
        return m;
    }
    // Extension: a surface normal per map entry (vors_tracker_enable_map_normals): central differences `step` pixels wide in the
    // keyframe's depth plane, neighbours further than jump_m metres in depth left out. After enable_map (level 0) and enable_map_voxels,
    // before the first track().
    void enable_map_normals(int step, Float jump_m) { check(vors_tracker_enable_map_normals(h_, step, jump_m)); }
    // The normals of read_map(capacity)'s points, rank for rank: [points][3], three zeros = none (vors_tracker_read_map_normals;
    // synchronises).
    std::vector<Float> read_map_normals(int capacity = 0x7fffffff) {
        std::uint32_t count = 0, n_segments = 0;
        check(vors_tracker_read_map(h_, 0, nullptr, nullptr, nullptr, &count, 0, nullptr, &n_segments));
        const size_t np = std::min<size_t>(count, (size_t)std::max(std::min(capacity, map_capacity_), 0));
        std::vector<Float> normals(3 * np + 3);  // (never empty: the entry refuses a NULL buffer)
        check(vors_tracker_read_map_normals(h_, (int)np, normals.data()));
        normals.resize(3 * np);
        return normals;
    }
    // Extension: the ICP correction at keyframe promotion (vors_tracker_enable_map_icp): a promoted frame's pose is refined against the
    // map before its cloud is emitted. After enable_map_normals, before the first track().
    void enable_map_icp(const vors_map_icp_params& params) { check(vors_tracker_enable_map_icp(h_, &params)); }
    // The running totals of the correction: promotions attempted and accepted (vors_tracker_read_map_icp; synchronises).
    std::pair<std::uint32_t, std::uint32_t> read_map_icp_totals() {
        std::uint32_t totals[2] = {0, 0};
        check(vors_tracker_read_map_icp(h_, nullptr, totals));
        return {totals[0], totals[1]};
    }
    // Extension: the same correction through the joint pass with the condition test (vors_tracker_enable_map_icp_joint), INSTEAD of
    // enable_map_icp. read_map_icp_totals() works unchanged.
    void enable_map_icp_joint(const vors_map_icp_joint_params& params) { check(vors_tracker_enable_map_icp_joint(h_, &params)); }
    // The verdict (a VORS_MAP_ICP_*) of the last track() (vors_tracker_read_map_icp; synchronises). What vors_track counts CONDITION
    // verdicts from; works with either correction.
    std::uint32_t read_map_icp_verdict() {
        vors_map_icp_record record{};
        check(vors_tracker_read_map_icp(h_, &record, nullptr));
        return record.verdict;
    }
    // Extension: the averaged map as the correction's model (vors_tracker_enable_map_icp_means): the pass reads the centroid and mean grey
    // of every voxel seen at least min_count times over at least min_span segments in the lists' place. After enable_map_voxel_stats and
    // one of enable_map_icp / enable_map_icp_joint, before the first track().
    void enable_map_icp_means(std::uint32_t min_count = 1, std::uint32_t min_span = 0) {
        check(vors_tracker_enable_map_icp_means(h_, min_count, min_span));
    }
    // The means record of the last track(): the window's length and its passing ranks (vors_tracker_read_map_icp_means; synchronises).
    vors_map_icp_means_record read_map_icp_means() {
        vors_map_icp_means_record record{};
        check(vors_tracker_read_map_icp_means(h_, &record));
        return record;
    }
    // Extension: the map seen from a pose (vors_tracker_render_map; synchronises): a z-buffered depth map and grey image in the geometry
    // of pyramid level `level`, row-major, the arguments of Config::init. pose = nullptr: the current frame's pose; range2 = nullptr: the
    // whole map, else (first, count) of the ranks to render (a vors_map_segment's `first`); footprint: 1, 2 or 3 pixels wide.
    struct Rendering {
        int rows = 0, cols = 0;
        std::vector<std::uint16_t> depth;  // 0 = no point landed
        std::vector<std::uint8_t> gray;
        std::uint32_t counts[VORS_RENDER_COUNTS] = {0, 0, 0, 0};  // considered, in front, landed, covered
    };
    Rendering render_map(int level = 0, const Iso3* pose = nullptr, const std::uint32_t* range2 = nullptr, int footprint = 1) {
        Rendering r;
        if (level < 0 || level >= VORS_MAX_LEVELS) throw std::invalid_argument("Tracker::render_map: level out of range");
        r.rows = rows_ >> level;
        r.cols = cols_ >> level;
        r.depth.resize((size_t)r.rows * r.cols);
        r.gray.resize((size_t)r.rows * r.cols);
        check(vors_tracker_render_map(h_, level, pose ? pose->data() : nullptr, range2, footprint, nullptr, r.depth.data(), r.gray.data(), r.counts));
        return r;
    }

   private:
    friend struct Config;
    Tracker(vors_tracker* h, int rows, int cols, int layout) : h_(h), rows_(rows), cols_(cols), layout_(layout) {}
    vors_tracker* h_ = nullptr;
    int rows_ = 0, cols_ = 0, layout_ = 0;
    bool log_ = true;
    int map_capacity_ = 0, map_max_keyframes_ = 0;  // enable_map's
    vors_pair_stats last_{};
    int last_status_ = 0;
};

inline Tracker Config::init(double keyframe_depth_timestamp, ImageView<std::uint16_t> depth_map, double keyframe_img_timestamp,
                            ImageView<std::uint8_t> img) const {
    if (depth_map.rows != img.rows || depth_map.cols != img.cols || depth_map.layout != img.layout)
        throw std::invalid_argument("Config::init: depth map and image differ in shape or layout");
    vors_config c = to_c();
    vors_tracker* h = nullptr;
    check(vors_tracker_create(&c, keyframe_depth_timestamp, depth_map.data, keyframe_img_timestamp, img.data, img.rows, img.cols,
                              img.layout, &h));
    return Tracker(h, img.rows, img.cols, img.layout);
}

// ---------------------------------------------------------------------------------------------------------------
// lm_optimizer.rs as an implementation of the trait, driven from the host.
// ---------------------------------------------------------------------------------------------------------------
struct EvalData {  // lm_optimizer.rs:31-40
    Mat6 hessian;
    Vec6 gradient;
    Float energy;
    Iso3 model;
};
using EvalState = std::variant<EvalData, Float>;  // Result<EvalData, Float> (lm_optimizer.rs:28)
using Obs = vors_obs;                             // lm_optimizer.rs:43-58

struct LMOptimizerState : optimizer::State<LMOptimizerState, Obs, EvalState, Iso3, std::string> {
    Float lm_coef;
    EvalData eval_data;

    static EvalData full_eval(const Obs& obs, const Iso3& model) {
        EvalData e;
        int32_t n_inside = 0;
        check(vors_lm_eval(&obs, model.data(), &e.energy, &n_inside, e.gradient.data(), e.hessian.data(), nullptr));
        e.model = model;
        return e;
    }
    static LMOptimizerState init(const Obs& obs, Iso3 model) {  // lm_optimizer.rs:113-118
        LMOptimizerState s;
        s.lm_coef = 0.1f;
        s.eval_data = full_eval(obs, model);
        return s;
    }
    bool step(Iso3* out, std::string* err) const {  // lm_optimizer.rs:123-136
        int ok = 0;
        check(vors_lm_step(eval_data.hessian.data(), eval_data.gradient.data(), eval_data.model.data(), lm_coef, out->data(), &ok));
        if (!ok) *err = "Error at Cholesky decomposition of hessian";
        return ok != 0;
    }
    EvalState eval(const Obs& obs, Iso3 model) const {  // lm_optimizer.rs:140-149 (device pass is fused: energy + g + H)
        EvalData e = full_eval(obs, model);
        if (e.energy > eval_data.energy) return EvalState(e.energy);
        return EvalState(e);
    }
    static std::pair<LMOptimizerState, optimizer::Continue> stop_criterion(LMOptimizerState self, std::size_t nb_iter,
                                                                           EvalState eval_state) {  // lm_optimizer.rs:156-192
        using optimizer::Continue;
        const bool too_many_iterations = nb_iter > 20;
        const bool is_err = std::holds_alternative<Float>(eval_state);
        if (is_err && too_many_iterations) return {self, Continue::Stop};
        if (too_many_iterations) {
            self.eval_data = std::get<EvalData>(eval_state);
            return {self, Continue::Stop};
        }
        if (is_err) {
            self.lm_coef *= 10.0f;
            return {self, Continue::Forward};
        }
        const EvalData& e = std::get<EvalData>(eval_state);
        const Float d_energy = self.eval_data.energy - e.energy;
        const Continue c = d_energy > 1.0f ? Continue::Forward : Continue::Stop;
        self.lm_coef = 0.1f * self.lm_coef;
        self.eval_data = e;
        return {self, c};
    }
};

}  // namespace track
}  // namespace vors
