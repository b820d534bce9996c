// vors_track — C++ mirror of the reference's only binary, src/bin/vors_track.rs, on top of libvors_hip.so:
//   Usage: ./vors_track [fr1|fr2|fr3|icl] associations_file          (vors_track.rs:24)
// Reads a TUM RGB-D associations file, initialises the tracker with the first RGB-D frame, tracks every following frame
// and prints one trajectory line `timestamp tx ty tz qx qy qz qw` per tracked frame on stdout (vors_track.rs:46-64).
// Optional trailing flags (not in the reference): `--quiet` silences the per-frame stderr logs; `--arith exact|fused|reference` selects the
// per-point arithmetic (include/vors_hip.h VORS_ARITH_*, default reference); `--candidates c2f|dense|dso` the level-0 mask source
// (default c2f = the reference's coarse-to-fine selection); `--depth-filter TOL_M[,MAX_WEIGHT[,FILL_MIN_WEIGHT]]` switches the recursive
// depth filter across keyframe promotions on (include/vors_hip.h vors_tracker_enable_depth_filter; defaults 255 and 0);
// `--map FILE.ply[,LEVEL[,CAPACITY[,MAX_KEYFRAMES[,MIN_WEIGHT]]]]` collects the cloud of every keyframe on the device
// (vors_tracker_enable_map; defaults level 0, 4 Mi points, 4096 keyframes, min_weight 0) and writes it as a binary PLY after the last frame.
// A malformed --map list, or MIN_WEIGHT >= 2 without --depth-filter, prints the usage and exits with status 2 before any device is touched.
// `--map-voxel SIZE_M[,TABLE_SLOTS]` (needs --map) keeps one point per voxel of edge SIZE_M metres in that map
// (vors_tracker_enable_map_voxels). TABLE_SLOTS, a power of two, defaults to 8 Mi entries — twice the default capacity, so the table is at
// most half full when the list is — and costs 16 x TABLE_SLOTS bytes of device memory (128 MiB at the default). Malformed, or without
// --map: the usage and status 2, before any device is touched. A sequence with more voxels than entries gets a warning after the last frame.
// `--map-voxel-means MIN_COUNT[,MIN_SPAN]` (needs --map-voxel) keeps statistics of every voxel (vors_tracker_enable_map_voxel_stats) and
// writes the AVERAGED map: centroid and mean grey of every voxel seen at least MIN_COUNT times over at least MIN_SPAN keyframes (default 0),
// with an extra `uint obs` property; the other voxels are left out of the file. Malformed or without --map-voxel: the usage and status 2.
// `--map-normals STEP[,JUMP_M]` (needs --map with LEVEL 0) gives every point of that map the surface normal of its pixel in its keyframe's
// depth map (vors_tracker_enable_map_normals; JUMP_M defaults to 0.05 m) and the PLY the properties nx ny nz. Malformed, without --map or
// with another LEVEL: the usage and status 2, before any device is touched.
// `--map-icp DIST_M[,ITERS[,LAST_KEYFRAMES[,MIN_COS[,HUBER_M]]]]` (needs --map and --map-normals) refines the pose of every frame that
// becomes a keyframe against the map before its cloud is appended (vors_tracker_enable_map_icp). Defaults: ITERS 8, LAST_KEYFRAMES 0 (the
// whole map), MIN_COS 0.9 against the frame's own normals, HUBER_M 0 (none); the verdict accepts a correction with at least 0.3 of the
// window matched, an rms of at most 0.01 m, and a step of at most 0.05 m and 0.05 rad. Malformed, or without --map / --map-normals: the
// usage (which repeats these defaults) and status 2, before any device is touched. After the last frame one line on stderr:
// `map-icp: attempted A accepted B`.
// `--map-icp-joint PHOTO_SCALE_M[,PHOTO_HUBER_GREY[,MAX_DILUTION_T[,MAX_DILUTION_R]]]` (needs --map-icp, whose fields become the correction's)
// runs that correction through the joint point-to-plane and photometric pass with a test on the conditioning of the system in the verdict
// (vors_tracker_enable_map_icp_joint). PHOTO_SCALE_M: metres per grey level, 0 = no photometric row; defaults: PHOTO_HUBER_GREY 0 (none),
// both bounds 0 (off). Malformed or without --map-icp: the usage and status 2, before any device is touched. The line after the last
// frame is then `map-icp: attempted A accepted B condition C`, C the corrections the condition test alone rejected.
// `--map-icp-means MIN_COUNT[,MIN_SPAN]` (needs --map-voxel and --map-icp, with or without --map-icp-joint) gives that correction the
// averaged map as its model (vors_tracker_enable_map_icp_means): the centroid and mean grey of every voxel seen at least MIN_COUNT times
// over at least MIN_SPAN keyframes, in the place of the voxel's first point. It switches the voxels' statistics on itself when
// --map-voxel-means has not. Malformed or without --map-voxel / --map-icp: the usage and status 2, before any device is touched. After
// the last frame a second line on stderr: `map-icp-means: attempted A accepted B kept / resolved Q`, Q the mean share of a window's
// ranks that passed, over the corrections with a window that is not empty.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "ply_io.hpp"
#include "png_io.hpp"
#include "tum_rgbd.hpp"

using namespace vors;

static const char* USAGE = "Usage: ./vors_track [fr1|fr2|fr3|icl] associations_file";

static bool create_camera(const std::string& id, Intrinsics& out) {  // vors_track.rs:99-110
    if (id == "fr1") out = tum_rgbd::INTRINSICS_FR1();
    else if (id == "fr2") out = tum_rgbd::INTRINSICS_FR2();
    else if (id == "fr3") out = tum_rgbd::INTRINSICS_FR3();
    else if (id == "icl") out = tum_rgbd::INTRINSICS_ICL_NUIM();
    else return false;
    return true;
}
static std::string parent_of(const std::string& path) {
    const size_t p = path.find_last_of('/');
    return p == std::string::npos ? std::string("") : path.substr(0, p);
}
static std::string join(const std::string& parent, const std::string& rel) {  // Path::join: an absolute `rel` replaces `parent`
    if (!rel.empty() && rel[0] == '/') return rel;
    return parent.empty() ? rel : parent + "/" + rel;
}

// "TOL_M[,MAX_WEIGHT[,FILL_MIN_WEIGHT]]": every field a whole number of its kind, nothing after the last. The VALUES are judged by the library.
static bool parse_depth_filter(const std::string& val, float& tol_m, int& max_weight, int& fill_min_weight) {
    if (val.empty()) return false;
    const char* p = val.c_str();
    char* end = nullptr;
    tol_m = std::strtof(p, &end);
    if (end == p) return false;
    int* ints[2] = {&max_weight, &fill_min_weight};
    for (int k = 0; k < 2 && *end == ','; ++k) {
        p = end + 1;
        const long v = std::strtol(p, &end, 10);
        if (end == p || v < -1000000 || v > 1000000) return false;
        *ints[k] = (int)v;
    }
    return *end == '\0';
}

// "FILE.ply[,LEVEL[,CAPACITY[,MAX_KEYFRAMES[,MIN_WEIGHT]]]]": a non-empty file name, then whole numbers, nothing after the last. The VALUES
// are judged by the library (but for the one rule that needs another flag, checked in main).
static bool parse_map(const std::string& val, std::string& file, int ints[4]) {
    const size_t comma = val.find(',');
    file = val.substr(0, comma);
    if (file.empty() || file.rfind("--", 0) == 0) return false;
    if (comma == std::string::npos) return true;
    const char* p = val.c_str() + comma;
    for (int k = 0; k < 4 && *p == ','; ++k) {
        char* end = nullptr;
        const long v = std::strtol(p + 1, &end, 10);
        if (end == p + 1 || v < -0x7fffffffL || v > 0x7fffffffL) return false;
        ints[k] = (int)v;
        p = end;
    }
    return *p == '\0';
}

// "SIZE_M[,TABLE_SLOTS]": a number, then a whole number, nothing after the last. The VALUES are judged by the library.
static bool parse_map_voxel(const std::string& val, float& voxel_m, int& table_slots) {
    if (val.empty()) return false;
    const char* p = val.c_str();
    char* end = nullptr;
    voxel_m = std::strtof(p, &end);
    if (end == p) return false;
    if (*end == ',') {
        p = end + 1;
        const long v = std::strtol(p, &end, 10);
        if (end == p || v < -0x7fffffffL || v > 0x7fffffffL) return false;
        table_slots = (int)v;
    }
    return *end == '\0';
}

// "MIN_COUNT[,MIN_SPAN]": whole numbers >= 0, nothing after the last.
static bool parse_map_voxel_means(const std::string& val, uint32_t& min_count, uint32_t& min_span) {
    if (val.empty()) return false;
    const char* p = val.c_str();
    char* end = nullptr;
    uint32_t* out[2] = {&min_count, &min_span};
    for (int k = 0; k < 2; ++k) {
        const long long v = std::strtoll(p, &end, 10);
        if (end == p || v < 0 || v > 0xFFFFFFFFll) return false;
        *out[k] = (uint32_t)v;
        if (*end != ',') break;
        p = end + 1;
        if (k == 1) return false;
    }
    return *end == '\0';
}

static const int MAP_VOXEL_DEFAULT_TABLE_SLOTS = 8 << 20;  // 16 bytes each: 128 MiB

// "STEP[,JUMP_M]": a whole number, then a number, nothing after the last. The VALUES are judged by the library.
static bool parse_map_normals(const std::string& val, int& step, float& jump_m) {
    if (val.empty()) return false;
    const char* p = val.c_str();
    char* end = nullptr;
    const long v = std::strtol(p, &end, 10);
    if (end == p || v < -0x7fffffffL || v > 0x7fffffffL) return false;
    step = (int)v;
    if (*end == ',') {
        p = end + 1;
        jump_m = std::strtof(p, &end);
        if (end == p) return false;
    }
    return *end == '\0';
}

// "DIST_M[,ITERS[,LAST_KEYFRAMES[,MIN_COS[,HUBER_M]]]]": a number, two whole numbers, two numbers, nothing after the last. The VALUES are
// judged by the library.
static const char* MAP_ICP_HELP =
    "Malformed --map-icp: expected DIST_M[,ITERS[,LAST_KEYFRAMES[,MIN_COS[,HUBER_M]]]] (defaults: ITERS 8, LAST_KEYFRAMES 0 = the whole map, "
    "MIN_COS 0.9, HUBER_M 0; accepted: >= 0.3 of the window matched, rms <= 0.01 m, step <= 0.05 m and <= 0.05 rad)";
static bool parse_map_icp(const std::string& val, vors_map_icp_params& p) {
    if (val.empty()) return false;
    const char* s = val.c_str();
    char* end = nullptr;
    p.dist_m = std::strtof(s, &end);
    if (end == s) return false;
    int32_t* ints[2] = {&p.iters, &p.last_keyframes};
    for (int k = 0; k < 2 && *end == ','; ++k) {
        s = end + 1;
        const long v = std::strtol(s, &end, 10);
        if (end == s || v < -0x7fffffffL || v > 0x7fffffffL) return false;
        *ints[k] = (int32_t)v;
    }
    float* floats[2] = {&p.min_cos, &p.huber_m};
    for (int k = 0; k < 2 && *end == ','; ++k) {
        s = end + 1;
        *floats[k] = std::strtof(s, &end);
        if (end == s) return false;
    }
    return *end == '\0';
}

// "PHOTO_SCALE_M[,PHOTO_HUBER_GREY[,MAX_DILUTION_T[,MAX_DILUTION_R]]]": up to four numbers, nothing after the last. The VALUES are judged
// by the library.
static const char* MAP_ICP_JOINT_HELP =
    "Malformed --map-icp-joint: expected PHOTO_SCALE_M[,PHOTO_HUBER_GREY[,MAX_DILUTION_T[,MAX_DILUTION_R]]] (metres per grey level, 0 = no "
    "photometric row; defaults: PHOTO_HUBER_GREY 0 = none, MAX_DILUTION_T 0 and MAX_DILUTION_R 0 = that bound is off)";
static bool parse_map_icp_joint(const std::string& val, vors_map_icp_joint_params& p) {
    if (val.empty()) return false;
    const char* s = val.c_str();
    char* end = nullptr;
    p.photo_scale_m = std::strtof(s, &end);
    if (end == s) return false;
    float* floats[3] = {&p.photo_huber_grey, &p.max_dilution_t, &p.max_dilution_r};
    for (int k = 0; k < 3 && *end == ','; ++k) {
        s = end + 1;
        *floats[k] = std::strtof(s, &end);
        if (end == s) return false;
    }
    return *end == '\0';
}

int main(int argc, char** argv) {
    bool map_icp = false, bad_map_icp = false, map_icp_joint = false, bad_map_icp_joint = false;
    vors_map_icp_joint_params joint_params{};
    vors_map_icp_params icp_params{};
    icp_params.step_eps = 1e-5f;
    icp_params.iters = 8;
    icp_params.min_points = 6;
    icp_params.normal_gate = 1;
    icp_params.min_cos = 0.9f;
    icp_params.min_match_ratio = 0.3f;
    icp_params.max_rms = 0.01f;
    icp_params.max_trans_m = 0.05f;
    icp_params.max_rot_rad = 0.05f;
    bool quiet = false, depth_filter = false, map = false, bad_map = false, map_voxel = false, bad_map_voxel = false;
    bool map_normals = false, bad_map_normals = false, map_voxel_means = false, bad_map_voxel_means = false;
    uint32_t means_min_count = 1, means_min_span = 0;
    bool map_icp_means = false, bad_map_icp_means = false;
    uint32_t icp_means_min_count = 1, icp_means_min_span = 0;
    int normals_step = 1;
    float normals_jump_m = 0.05f;
    float voxel_m = 0.0f;
    int voxel_table_slots = MAP_VOXEL_DEFAULT_TABLE_SLOTS;
    std::string map_file;
    int map_ints[4] = {0, 4 << 20, 4096, 0};  // level, capacity, max_keyframes, min_weight
    float filter_tol_m = 0.0f;
    int filter_max_weight = 255, filter_fill_min_weight = 0;
    int arithmetic = VORS_ARITH_REFERENCE, candidates = VORS_CANDIDATES_COARSE_TO_FINE;
    bool bad_flag = false;
    for (int a = 3; a < argc && !bad_flag; ++a) {  // extension flags follow the reference's two positional arguments
        const std::string flag = argv[a], val = a + 1 < argc ? argv[a + 1] : "";
        if (flag == "--quiet") {
            quiet = true;
        } else if (flag == "--arith" && (val == "exact" || val == "fused" || val == "reference")) {
            arithmetic = val == "fused" ? VORS_ARITH_FUSED : (val == "exact" ? VORS_ARITH_EXACT : VORS_ARITH_REFERENCE);
            ++a;
        } else if (flag == "--candidates" && (val == "c2f" || val == "dense" || val == "dso")) {
            candidates = val == "dense" ? VORS_CANDIDATES_DENSE : (val == "dso" ? VORS_CANDIDATES_DSO : VORS_CANDIDATES_COARSE_TO_FINE);
            ++a;
        } else if (flag == "--depth-filter" && parse_depth_filter(val, filter_tol_m, filter_max_weight, filter_fill_min_weight)) {
            depth_filter = true;
            ++a;
        } else if (flag == "--map") {
            map = parse_map(val, map_file, map_ints);
            bad_map = !map;
            ++a;
        } else if (flag == "--map-voxel") {
            map_voxel = parse_map_voxel(val, voxel_m, voxel_table_slots);
            bad_map_voxel = !map_voxel;
            ++a;
        } else if (flag == "--map-voxel-means") {
            map_voxel_means = parse_map_voxel_means(val, means_min_count, means_min_span);
            bad_map_voxel_means = !map_voxel_means;
            ++a;
        } else if (flag == "--map-icp-means") {
            map_icp_means = parse_map_voxel_means(val, icp_means_min_count, icp_means_min_span);
            bad_map_icp_means = !map_icp_means;
            ++a;
        } else if (flag == "--map-normals") {
            map_normals = parse_map_normals(val, normals_step, normals_jump_m);
            bad_map_normals = !map_normals;
            ++a;
        } else if (flag == "--map-icp") {
            map_icp = parse_map_icp(val, icp_params);
            bad_map_icp = !map_icp;
            ++a;
        } else if (flag == "--map-icp-joint") {
            map_icp_joint = parse_map_icp_joint(val, joint_params);
            bad_map_icp_joint = !map_icp_joint;
            ++a;
        } else {
            bad_flag = true;
        }
    }
    if (bad_map || (map && map_ints[3] >= 2 && !depth_filter)) {  // (the new flag's own errors: the usage, and a status a script can test)
        std::fprintf(stderr, "%s\n\"%s\"\n", USAGE,
                     bad_map ? "Malformed --map: expected FILE.ply[,LEVEL[,CAPACITY[,MAX_KEYFRAMES[,MIN_WEIGHT]]]]"
                             : "--map with MIN_WEIGHT >= 2 needs --depth-filter");
        return 2;
    }
    if (bad_map_voxel || (map_voxel && !map)) {
        std::fprintf(stderr, "%s\n\"%s\"\n", USAGE,
                     bad_map_voxel ? "Malformed --map-voxel: expected SIZE_M[,TABLE_SLOTS]" : "--map-voxel needs --map");
        return 2;
    }
    if (bad_map_voxel_means || (map_voxel_means && !map_voxel)) {
        std::fprintf(stderr, "%s\n\"%s\"\n", USAGE,
                     bad_map_voxel_means ? "Malformed --map-voxel-means: expected MIN_COUNT[,MIN_SPAN]" : "--map-voxel-means needs --map-voxel");
        return 2;
    }
    if (bad_map_normals || (map_normals && (!map || map_ints[0] != 0))) {
        std::fprintf(stderr, "%s\n\"%s\"\n", USAGE,
                     bad_map_normals ? "Malformed --map-normals: expected STEP[,JUMP_M]"
                     : !map          ? "--map-normals needs --map"
                                     : "--map-normals needs --map with LEVEL 0");
        return 2;
    }
    if (bad_map_icp || (map_icp && (!map || !map_normals))) {
        std::fprintf(stderr, "%s\n\"%s\"\n", USAGE, bad_map_icp ? MAP_ICP_HELP : !map ? "--map-icp needs --map" : "--map-icp needs --map-normals");
        return 2;
    }
    if (bad_map_icp_joint || (map_icp_joint && !map_icp)) {
        std::fprintf(stderr, "%s\n\"%s\"\n", USAGE, bad_map_icp_joint ? MAP_ICP_JOINT_HELP : "--map-icp-joint needs --map-icp");
        return 2;
    }
    if (bad_map_icp_means || (map_icp_means && (!map_voxel || !map_icp))) {
        std::fprintf(stderr, "%s\n\"%s\"\n", USAGE,
                     bad_map_icp_means ? "Malformed --map-icp-means: expected MIN_COUNT[,MIN_SPAN]"
                     : !map_voxel      ? "--map-icp-means needs --map-voxel"
                                       : "--map-icp-means needs --map-icp");
        return 2;
    }
    if (argc > 3) argc = bad_flag ? 0 : 3;
    if (argc != 3) {  // vors_track.rs:75-96
        std::fprintf(stderr, "%s\n\"Wrong number of arguments\"\n", USAGE);
        return 0;  // the reference's main() only prints the error (vors_track.rs:17-22)
    }
    Intrinsics intrinsics;
    if (!create_camera(argv[1], intrinsics)) {
        std::fprintf(stderr, "%s\n\"Unknown camera id: %s\"\n", USAGE, argv[1]);
        return 0;
    }
    std::ifstream f(argv[2]);
    if (!f.good()) {
        std::fprintf(stderr, "%s\n\"The association file does not exist or is not reachable: %s\"\n", USAGE, argv[2]);
        return 0;
    }
    std::stringstream ss;
    ss << f.rdbuf();
    std::vector<tum_rgbd::Association> associations;
    std::string err;
    if (!tum_rgbd::parse::associations(ss.str(), associations, err)) {
        std::fprintf(stderr, "\"%s\"\n", err.c_str());
        return 0;
    }
    if (associations.empty()) {
        std::fprintf(stderr, "thread 'main' panicked at 'index out of bounds'\n");  // associations[0] (vors_track.rs:43)
        return 101;
    }
    const std::string parent = parent_of(argv[2]);  // vors_track.rs:125-138
    try {
        auto read_images = [&](const tum_rgbd::Association& a, std::vector<uint16_t>& depth, std::vector<uint8_t>& gray, uint32_t& w,
                               uint32_t& h) {  // vors_track.rs:140-145
            uint32_t w2, h2;
            png_io::read_png_16bits(join(parent, a.depth_file_path), w, h, depth);
            png_io::read_luma8(join(parent, a.color_file_path), w2, h2, gray);
            if (w2 != w || h2 != h) throw std::runtime_error("depth and colour images differ in size");
        };
        // vors_track.rs:34-40
        track::Config config{6, 7, tum_rgbd::DEPTH_SCALE, intrinsics, 0.0001f};
        config.arithmetic = arithmetic;
        config.candidates_mode = candidates;
        std::vector<uint16_t> depth;
        std::vector<uint8_t> gray;
        uint32_t w = 0, h = 0;
        read_images(associations[0], depth, gray, w, h);
        track::Tracker tracker = config.init(associations[0].depth_timestamp, {depth.data(), (int)h, (int)w, VORS_ROW_MAJOR},
                                             associations[0].color_timestamp, {gray.data(), (int)h, (int)w, VORS_ROW_MAJOR});
        tracker.set_logging(!quiet);
        if (depth_filter) tracker.enable_depth_filter(filter_tol_m, filter_max_weight, filter_fill_min_weight);
        if (map) tracker.enable_map(map_ints[0], map_ints[1], map_ints[2], map_ints[3]);  // (after the filter: min_weight reads its weights)
        if (map_voxel) tracker.enable_map_voxels(voxel_m, voxel_table_slots);
        if (map_voxel_means || map_icp_means) tracker.enable_map_voxel_stats();  // (in front of the normals: it emits keyframe 0 again, too)
        if (map_normals) tracker.enable_map_normals(normals_step, normals_jump_m);  // (behind the voxel filter, which emits keyframe 0 again)
        std::uint32_t condition = 0;
        if (map_icp_joint) {
            joint_params.icp = icp_params;
            tracker.enable_map_icp_joint(joint_params);
        } else if (map_icp) {
            tracker.enable_map_icp(icp_params);
        }
        if (map_icp_means) tracker.enable_map_icp_means(icp_means_min_count, icp_means_min_span);
        double kept_share = 0.0;
        std::uint32_t windows = 0;
        for (size_t k = 1; k < associations.size(); ++k) {  // vors_track.rs:49-64
            uint32_t w2, h2;
            read_images(associations[k], depth, gray, w2, h2);
            if (w2 != w || h2 != h) throw std::runtime_error("image size changed inside the sequence");
            tracker.track(associations[k].depth_timestamp, {depth.data(), (int)h, (int)w, VORS_ROW_MAJOR}, associations[k].color_timestamp,
                          {gray.data(), (int)h, (int)w, VORS_ROW_MAJOR});
            const auto cf = tracker.current_frame();
            std::printf("%s\n", tum_rgbd::to_string(tum_rgbd::Frame{cf.first, cf.second}).c_str());
            // The handle's totals are (attempted, accepted) and their layout is ABI, so CONDITION is counted here, from the record of each
            // frame: one small read-back and one synchronisation per frame, which exist for this counter alone and only with this flag
            // (the frame has already waited for its promotion: with the correction on, track() reads its results back behind it).
            if (map_icp_joint && tracker.read_map_icp_verdict() == VORS_MAP_ICP_CONDITION) ++condition;
            if (map_icp_means) {  // (the same kind of read-back, for the second line alone and only with this flag)
                const vors_map_icp_means_record r = tracker.read_map_icp_means();
                if (r.resolved) {
                    kept_share += (double)r.kept / (double)r.resolved;
                    ++windows;
                }
            }
        }
        if (map_icp) {
            const auto totals = tracker.read_map_icp_totals();
            if (map_icp_joint)
                std::fprintf(stderr, "map-icp: attempted %u accepted %u condition %u\n", totals.first, totals.second, condition);
            else
                std::fprintf(stderr, "map-icp: attempted %u accepted %u\n", totals.first, totals.second);
            if (map_icp_means)
                std::fprintf(stderr, "map-icp-means: attempted %u accepted %u kept / resolved %.4f\n", totals.first, totals.second,
                             windows ? kept_share / windows : 0.0);
        }
        if (map) {
            if (map_voxel && tracker.read_map_voxels().overflow != 0)
                std::fprintf(stderr, "Warning: more voxels than the %d entries of the voxel table: the map is incomplete (raise TABLE_SLOTS or SIZE_M)\n",
                             voxel_table_slots);
            const track::Tracker::Map m = tracker.read_map();
            if (m.count > (uint32_t)map_ints[1])
                std::fprintf(stderr, "Warning: the map holds %u points but its capacity is %d: the last %u were dropped\n", m.count, map_ints[1],
                             m.count - (uint32_t)map_ints[1]);
            if (m.n_segments > (uint32_t)map_ints[2])
                std::fprintf(stderr, "Warning: %u keyframes but room for %d segment records\n", m.n_segments, map_ints[2]);
            if (map_voxel_means) {  // ranks are aligned: the normals of the map's points go with their voxels' centroids
                const track::Tracker::MapVoxelMeans mm = tracker.map_voxel_means(means_min_count, means_min_span, (int)m.gray.size());
                std::vector<Float> normals;
                if (map_normals) normals = tracker.read_map_normals((int)m.gray.size());
                std::vector<std::uint32_t> obs(m.gray.size());
                for (size_t r = 0; r < obs.size(); ++r) obs[r] = mm.obs[2 * r];
                ply_io::write_map_means(map_file, mm.xyz_mean.data(), map_normals ? normals.data() : nullptr, mm.gray_mean.data(), obs.data(),
                                        obs.size(), m.segments.data(), m.segments.size());
            } else if (map_normals) {
                const std::vector<Float> normals = tracker.read_map_normals((int)m.gray.size());
                ply_io::write_map(map_file, m.xyz.data(), normals.data(), m.gray.data(), m.gray.size(), m.segments.data(), m.segments.size());
            } else {
                ply_io::write_map(map_file, m.xyz.data(), m.gray.data(), m.gray.size(), m.segments.data(), m.segments.size());
            }
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "\"%s\"\n", e.what());
    }
    return 0;
}
