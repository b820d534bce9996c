// Stand-alone check of ply_io.hpp's writer with normals (no device, no library): the same cloud through both overloads of write_map into
// SCRATCH_DIR — plain.ply (x y z intensity, 13 bytes per vertex) and normals.ply (x y z nx ny nz intensity, 25 bytes) — and the header and
// payload of the second parsed back.
//   usage: ply_normals_test SCRATCH_DIR
#include <cstdio>
#include <fstream>
#include <iterator>

#include "ply_io.hpp"

using namespace vors;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: ply_normals_test SCRATCH_DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    const size_t n = 5;
    const float xyz[3 * n] = {1.0f, 2.0f, 3.0f, -0.5f, 0.25f, 8.0f, 0.0f, 0.0f, 1.5f, 4.0f, -4.0f, 2.0f, 1e-3f, 1e3f, 7.0f};
    const float normals[3 * n] = {0.0f, 0.0f, -1.0f, 0.6f, 0.0f, -0.8f, 0.0f, 0.0f, 0.0f, -1.0f, 0.0f, 0.0f, 0.0f, 0.8f, -0.6f};
    const std::uint8_t gray[n] = {0, 17, 128, 200, 255};
    vors_map_segment seg[2] = {{0, 0, 3, {0, 0, 0, 0, 0, 0, 1}}, {7, 3, 2, {0.5f, -1.0f, 2.0f, 0.1f, 0.2f, 0.3f, 0.9f}}};
    ply_io::write_map(dir + "/plain.ply", xyz, gray, n, seg, 2);
    ply_io::write_map(dir + "/normals.ply", xyz, normals, gray, n, seg, 2);
    const std::string plain = slurp(dir + "/plain.ply"), with = slurp(dir + "/normals.ply");
    const std::string end = "end_header\n";
    const size_t hp = plain.find(end), hw = with.find(end);
    CHECK(hp != std::string::npos && hw != std::string::npos);
    if (failures) return 1;
    const std::string extra = "property float nx\nproperty float ny\nproperty float nz\n";
    // the header with normals is the plain one with the three properties between z and intensity
    const size_t at = with.find(extra);
    CHECK(at != std::string::npos);
    CHECK(with.substr(0, at) + with.substr(at + extra.size(), hw + end.size() - at - extra.size()) == plain.substr(0, hp + end.size()));
    CHECK(with.compare(at - std::string("property float z\n").size(), 17, "property float z\n") == 0);
    CHECK(with.compare(at + extra.size(), 24, "property uchar intensity") == 0);
    const unsigned char* pp = reinterpret_cast<const unsigned char*>(plain.data()) + hp + end.size();
    const unsigned char* pw = reinterpret_cast<const unsigned char*>(with.data()) + hw + end.size();
    CHECK(plain.size() - hp - end.size() == n * ply_io::VERTEX_BYTES);
    CHECK(with.size() - hw - end.size() == n * ply_io::VERTEX_NORMAL_BYTES);
    for (size_t i = 0; i < n && !failures; ++i) {
        unsigned char want[12];
        for (int c = 0; c < 3; ++c) ply_io::put_f32_le(normals[3 * i + c], want + 4 * c);
        CHECK(std::memcmp(pw + 25 * i, pp + 13 * i, 12) == 0);      // x y z as without normals
        CHECK(std::memcmp(pw + 25 * i + 12, want, 12) == 0);        // nx ny nz, little-endian
        CHECK(pw[25 * i + 24] == gray[i] && pp[13 * i + 12] == gray[i]);
    }
    // no points: headers only
    ply_io::write_map(dir + "/empty_normals.ply", xyz, normals, gray, 0, seg, 0);
    const std::string empty = slurp(dir + "/empty_normals.ply");
    CHECK(empty.find("element vertex 0\n") != std::string::npos && empty.size() == empty.find(end) + end.size());
    if (failures) return 1;
    std::printf("ply_normals_test: ok\n");
    return 0;
}
