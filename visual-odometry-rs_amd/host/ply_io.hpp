// Binary little-endian PLY writer for the keyframe map of a sequence (vors_tracker_read_map): one vertex per point — x y z float32,
// intensity uchar, 13 bytes — and one comment line per keyframe segment: frame, first, count and the camera -> world pose the points
// were carried through. Header-only, no dependency beyond the standard library; the payload is assembled byte by byte, so the file is
// little-endian on every host. With normals (the overload below; vors_tracker_read_map_normals) a vertex is x y z nx ny nz float32,
// intensity uchar, 25 bytes. The averaged map (write_map_means; vors_tracker_map_voxel_means) adds `obs uint` behind the intensity and
// leaves the rejected ranks out.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vors_hip.h"

namespace vors {
namespace ply_io {

constexpr size_t VERTEX_BYTES = 13;
constexpr size_t VERTEX_NORMAL_BYTES = 25;

inline void put_f32_le(float v, unsigned char* out) {
    std::uint32_t u;
    std::memcpy(&u, &v, 4);
    for (int k = 0; k < 4; ++k) out[k] = (unsigned char)((u >> (8 * k)) & 0xffu);
}

// The header: `n_points` vertices, one "comment segment ..." line per record (%.9g round-trips a float32).
inline std::string header(size_t n_points, const vors_map_segment* segments, size_t n_segments, bool with_normals = false,
                          bool with_obs = false) {
    std::string h = "ply\nformat binary_little_endian 1.0\ncomment vors keyframe map: one segment line per keyframe (frame first count tx ty tz qx qy qz qw)\n";
    char line[256];
    for (size_t k = 0; k < n_segments; ++k) {
        const vors_map_segment& s = segments[k];
        std::snprintf(line, sizeof line, "comment segment %d %u %u %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", (int)s.frame, (unsigned)s.first,
                      (unsigned)s.count, s.pose7[0], s.pose7[1], s.pose7[2], s.pose7[3], s.pose7[4], s.pose7[5], s.pose7[6]);
        h += line;
    }
    h += "element vertex " + std::to_string(n_points) + "\nproperty float x\nproperty float y\nproperty float z\n" +
         (with_normals ? "property float nx\nproperty float ny\nproperty float nz\n" : "") + "property uchar intensity\n" + (with_obs ? "property uint obs\n" : "") + "end_header\n";
    return h;
}

// xyz: [n_points][3], gray: [n_points]. Throws std::runtime_error when the file cannot be written.
inline void write_map(const std::string& path, const float* xyz, const std::uint8_t* gray, size_t n_points, const vors_map_segment* segments,
                      size_t n_segments) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f.good()) throw std::runtime_error("cannot open " + path + " for writing");
    const std::string h = header(n_points, segments, n_segments);
    f.write(h.data(), (std::streamsize)h.size());
    std::vector<unsigned char> buf;
    const size_t block = 65536;  // points per write
    buf.resize(std::min(n_points, block) * VERTEX_BYTES);
    for (size_t p0 = 0; p0 < n_points; p0 += block) {
        const size_t n = std::min(block, n_points - p0);
        for (size_t i = 0; i < n; ++i) {
            unsigned char* o = buf.data() + i * VERTEX_BYTES;
            for (int c = 0; c < 3; ++c) put_f32_le(xyz[3 * (p0 + i) + c], o + 4 * c);
            o[12] = gray[p0 + i];
        }
        f.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)(n * VERTEX_BYTES));
    }
    f.flush();
    if (!f.good()) throw std::runtime_error("error while writing " + path);
}

// The same with one normal per point: normals [n_points][3] (three zeros = the point has none), written after x y z.
inline void write_map(const std::string& path, const float* xyz, const float* normals, const std::uint8_t* gray, size_t n_points,
                      const vors_map_segment* segments, size_t n_segments) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f.good()) throw std::runtime_error("cannot open " + path + " for writing");
    const std::string h = header(n_points, segments, n_segments, true);
    f.write(h.data(), (std::streamsize)h.size());
    std::vector<unsigned char> buf;
    const size_t block = 65536;  // points per write
    buf.resize(std::min(n_points, block) * VERTEX_NORMAL_BYTES);
    for (size_t p0 = 0; p0 < n_points; p0 += block) {
        const size_t n = std::min(block, n_points - p0);
        for (size_t i = 0; i < n; ++i) {
            unsigned char* o = buf.data() + i * VERTEX_NORMAL_BYTES;
            for (int c = 0; c < 3; ++c) put_f32_le(xyz[3 * (p0 + i) + c], o + 4 * c);
            for (int c = 0; c < 3; ++c) put_f32_le(normals[3 * (p0 + i) + c], o + 12 + 4 * c);
            o[24] = gray[p0 + i];
        }
        f.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)(n * VERTEX_NORMAL_BYTES));
    }
    f.flush();
    if (!f.good()) throw std::runtime_error("error while writing " + path);
}

// The averaged map: xyz_mean / gray_mean [n_ranks] as vors_tracker_map_voxel_means resolved them, obs_count [n_ranks] the observations
// of every rank, normals [n_ranks][3] or NULL. A rank whose centroid is NaN (rejected by min_count / min_span) is LEFT OUT of the file,
// so the segment lines' first / count still speak of the map's ranks, not of the file's vertices. Vertex: x y z [nx ny nz] float32,
// intensity uchar, obs uint32. Returns the vertices written.
inline size_t write_map_means(const std::string& path, const float* xyz_mean, const float* normals, const std::uint8_t* gray_mean,
                              const std::uint32_t* obs_count, size_t n_ranks, const vors_map_segment* segments, size_t n_segments) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f.good()) throw std::runtime_error("cannot open " + path + " for writing");
    size_t n_points = 0;
    for (size_t r = 0; r < n_ranks; ++r) n_points += xyz_mean[3 * r] == xyz_mean[3 * r] ? 1 : 0;  // (not NaN)
    const std::string h = header(n_points, segments, n_segments, normals != nullptr, true);
    f.write(h.data(), (std::streamsize)h.size());
    const size_t vertex = (normals ? VERTEX_NORMAL_BYTES : VERTEX_BYTES) + 4;
    std::vector<unsigned char> buf;
    buf.reserve(std::min<size_t>(n_points, 65536) * vertex);
    for (size_t r = 0; r < n_ranks; ++r) {
        if (xyz_mean[3 * r] == xyz_mean[3 * r]) {
            const size_t at = buf.size();
            buf.resize(at + vertex);
            unsigned char* o = buf.data() + at;
            for (int c = 0; c < 3; ++c) put_f32_le(xyz_mean[3 * r + c], o + 4 * c);
            o += 12;
            if (normals) {
                for (int c = 0; c < 3; ++c) put_f32_le(normals[3 * r + c], o + 4 * c);
                o += 12;
            }
            o[0] = gray_mean[r];
            for (int k = 0; k < 4; ++k) o[1 + k] = (unsigned char)((obs_count[r] >> (8 * k)) & 0xffu);
        }
        if (buf.size() >= 65536 * vertex || r + 1 == n_ranks) {
            f.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)buf.size());
            buf.clear();
        }
    }
    f.flush();
    if (!f.good()) throw std::runtime_error("error while writing " + path);
    return n_points;
}

}  // namespace ply_io
}  // namespace vors
