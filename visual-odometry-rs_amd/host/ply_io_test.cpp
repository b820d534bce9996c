// Stand-alone check of ply_io.hpp (no device, no library): writes a cloud with two segments, parses header and payload back, checks byte
// counts, the little-endian floats, the comment lines and the file without points.
//   usage: ply_io_test SCRATCH_DIR
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <sstream>

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
static float f32_le(const unsigned char* p) {
    const std::uint32_t u = (std::uint32_t)p[0] | ((std::uint32_t)p[1] << 8) | ((std::uint32_t)p[2] << 16) | ((std::uint32_t)p[3] << 24);
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
// header lines up to and including end_header; *payload = offset of the first byte after it
static std::vector<std::string> header_lines(const std::string& file, size_t* payload) {
    std::vector<std::string> lines;
    size_t pos = 0;
    while (pos < file.size()) {
        const size_t nl = file.find('\n', pos);
        if (nl == std::string::npos) break;
        lines.push_back(file.substr(pos, nl - pos));
        pos = nl + 1;
        if (lines.back() == "end_header") break;
    }
    *payload = pos;
    return lines;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: ply_io_test SCRATCH_DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    // 5 points in two segments (3 + 2); values whose bytes differ in every position
    const float xyz[15] = {1.0f, -2.5f, 3.25f, 0.1f, 1e-20f, -1e20f, 123456.789f, -0.0f, 7.0f, 0.5f, 0.25f, 0.125f, -1.0f, -2.0f, -3.0f};
    const std::uint8_t gray[5] = {0, 1, 127, 128, 255};
    vors_map_segment seg[2] = {};
    seg[0].frame = 0;
    seg[0].first = 0;
    seg[0].count = 3;
    seg[0].pose7[6] = 1.0f;
    seg[1].frame = 7;
    seg[1].first = 3;
    seg[1].count = 2;
    const float pose1[7] = {0.1f, -0.2f, 0.3f, 0.01f, 0.02f, 0.03f, 0.9993f};
    std::memcpy(seg[1].pose7, pose1, sizeof pose1);
    const std::string path = dir + "/two_segments.ply";
    ply_io::write_map(path, xyz, gray, 5, seg, 2);
    const std::string file = slurp(path);
    size_t payload = 0;
    const std::vector<std::string> lines = header_lines(file, &payload);
    CHECK(lines.size() == 11);
    CHECK(lines.size() >= 3 && lines[0] == "ply" && lines[1] == "format binary_little_endian 1.0" && lines[2].rfind("comment ", 0) == 0);
    CHECK(lines.size() == 11 && lines[5] == "element vertex 5" && lines[6] == "property float x" && lines[7] == "property float y" &&
          lines[8] == "property float z" && lines[9] == "property uchar intensity" && lines[10] == "end_header");
    CHECK(file.size() == payload + 5 * ply_io::VERTEX_BYTES);
    for (int k = 0; k < 2 && lines.size() == 11; ++k) {  // the comment lines carry the records: integers exactly, floats bit for bit
        std::istringstream in(lines[3 + k]);
        std::string w0, w1;
        long frame = -1, first = -1, count = -1;
        float pose[7];
        in >> w0 >> w1 >> frame >> first >> count;
        for (float& v : pose) in >> v;
        CHECK(!in.fail() && w0 == "comment" && w1 == "segment");
        CHECK(frame == seg[k].frame && first == (long)seg[k].first && count == (long)seg[k].count);
        CHECK(std::memcmp(pose, seg[k].pose7, sizeof pose) == 0);
    }
    const unsigned char* p = reinterpret_cast<const unsigned char*>(file.data()) + payload;
    for (int i = 0; i < 5 && file.size() == payload + 5 * ply_io::VERTEX_BYTES; ++i) {
        for (int c = 0; c < 3; ++c) {
            const float v = f32_le(p + i * 13 + 4 * c);
            CHECK(std::memcmp(&v, &xyz[3 * i + c], 4) == 0);
        }
        CHECK(p[i * 13 + 12] == gray[i]);
    }
    // 1.0f is 00 00 80 3f in little-endian order, whatever the host's
    CHECK(file.size() >= payload + 4 && p[0] == 0x00 && p[1] == 0x00 && p[2] == 0x80 && p[3] == 0x3f);
    // more points than one write block
    {
        const size_t n = 65536 + 3;
        std::vector<float> big(3 * n);
        std::vector<std::uint8_t> bg(n);
        for (size_t i = 0; i < n; ++i) {
            big[3 * i] = (float)i;
            big[3 * i + 1] = -(float)i;
            big[3 * i + 2] = 0.5f * (float)i;
            bg[i] = (std::uint8_t)(i * 7);
        }
        const std::string pb = dir + "/blocks.ply";
        ply_io::write_map(pb, big.data(), bg.data(), n, nullptr, 0);
        const std::string fb = slurp(pb);
        size_t off = 0;
        const std::vector<std::string> lb = header_lines(fb, &off);
        CHECK(lb.size() == 9 && lb[3] == "element vertex 65539");
        CHECK(fb.size() == off + n * 13);
        const unsigned char* q = reinterpret_cast<const unsigned char*>(fb.data()) + off + (n - 1) * 13;
        CHECK(fb.size() == off + n * 13 && f32_le(q) == (float)(n - 1) && f32_le(q + 8) == 0.5f * (float)(n - 1) && q[12] == bg[n - 1]);
    }
    // no points, no segments: a header alone
    {
        const std::string pz = dir + "/empty.ply";
        ply_io::write_map(pz, nullptr, nullptr, 0, nullptr, 0);
        const std::string fz = slurp(pz);
        size_t off = 0;
        const std::vector<std::string> lz = header_lines(fz, &off);
        CHECK(lz.size() == 9 && lz[3] == "element vertex 0" && lz.back() == "end_header");
        CHECK(off == fz.size());
    }
    // an unwritable path is an exception, not a silent success
    bool threw = false;
    try {
        ply_io::write_map(dir + "/no/such/dir/x.ply", xyz, gray, 5, seg, 2);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    CHECK(threw);
    if (failures) return 1;
    std::printf("ply_io_test: ok\n");
    return 0;
}
