// Stand-alone check of vors_undistort_frame_host, vors_undistort_source_host and vors_register_depth_host for a sanitizer build of the host
// code (`make frontend_host_check`: operators.cpp and this file with -fsanitize=address,undefined on the host side; runs without a GPU).
// Every plane is a heap block of exactly its size, so a tap or a footprint pixel outside its plane would be reported. The cases of
// tests/test_frontend_host.py at 29x37: identity, integer and half-pixel shifts in both border modes, a strongly distorted camera (most
// coordinates outside, some NaN-free but huge), a crop, depth that is never interpolated; registration: identity, an integer baseline,
// occlusion, the tie-break, holes, the footprints on an up-scaled plane; refusals with sentinel-filled outputs.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/vors_hip.h"

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static const int ROWS = 29, COLS = 37;

struct Out {
    std::vector<uint8_t> gray;
    std::vector<uint16_t> depth;
    std::vector<float> map;
    uint32_t counts[VORS_UNDISTORT_COUNTS];
    Out(int rows, int cols) : gray((size_t)rows * cols, 7), depth((size_t)rows * cols, 7), map((size_t)rows * cols * 2, 7.f), counts{7, 7, 7} {}
    bool untouched() const {
        for (uint8_t g : gray) if (g != 7) return false;
        for (uint16_t d : depth) if (d != 7) return false;
        for (float m : map) if (m != 7.f) return false;
        return counts[0] == 7 && counts[1] == 7 && counts[2] == 7;
    }
};

static void undistortion() {
    std::vector<uint8_t> g((size_t)ROWS * COLS);
    std::vector<uint16_t> d((size_t)ROWS * COLS);
    for (size_t i = 0; i < g.size(); ++i) {
        g[i] = (uint8_t)((i * 37 + 11) % 256);
        d[i] = (i % 13 == 5) ? 0 : (uint16_t)(4000 + 53 * (i % 97));
    }
    const float cam[5] = {COLS / 2.f - 0.5f, ROWS / 2.f - 0.5f, 32.f, 16.f, 0.f};
    for (int border = 0; border <= 1; ++border) {
        {  // identity
            Out o(ROWS, COLS);
            CHECK(vors_undistort_frame_host(g.data(), d.data(), ROWS, COLS, cam, nullptr, cam, ROWS, COLS, border, o.gray.data(), o.depth.data(),
                                            o.map.data(), o.counts) == VORS_OK);
            CHECK(o.gray == g && o.depth == d && o.counts[0] == (uint32_t)(ROWS * COLS) && o.counts[1] == o.counts[0]);
        }
        {  // three columns to the left
            float out[5] = {cam[0] - 3.f, cam[1], cam[2], cam[3], cam[4]};
            Out o(ROWS, COLS);
            CHECK(vors_undistort_frame_host(g.data(), d.data(), ROWS, COLS, cam, nullptr, out, ROWS, COLS, border, o.gray.data(), o.depth.data(),
                                            nullptr, o.counts) == VORS_OK);
            for (int y = 0; y < ROWS; ++y)
                for (int x = 0; x < COLS; ++x) {
                    const size_t i = (size_t)y * COLS + x;
                    if (x + 3 < COLS) CHECK(o.gray[i] == g[i + 3] && o.depth[i] == d[i + 3]);
                    else CHECK(o.depth[i] == 0 && o.gray[i] == (border ? g[(size_t)y * COLS + COLS - 1] : 0));
                }
            CHECK(o.counts[1] == (uint32_t)(ROWS * (COLS - 3)));
        }
        {  // half a pixel, both axes
            float out[5] = {cam[0] - 0.5f, cam[1] - 0.5f, cam[2], cam[3], cam[4]};
            Out o(ROWS, COLS);
            CHECK(vors_undistort_frame_host(g.data(), d.data(), ROWS, COLS, cam, nullptr, out, ROWS, COLS, border, o.gray.data(), o.depth.data(),
                                            nullptr, nullptr) == VORS_OK);
            for (int y = 0; y + 1 < ROWS; ++y)
                for (int x = 0; x + 1 < COLS; ++x) {
                    const size_t i = (size_t)y * COLS + x;
                    const float t0 = g[i] + 0.5f * (g[i + 1] - g[i]), t1 = g[i + COLS] + 0.5f * (g[i + COLS + 1] - g[i + COLS]);
                    CHECK(o.gray[i] == (uint8_t)std::floor(t0 + 0.5f * (t1 - t0) + 0.5f) && o.depth[i] == d[i + COLS + 1]);
                }
        }
        {  // a crop of a strongly distorted camera with a skew and a negative focal, and a larger output than input
            const float in[5] = {0.5f * COLS - 0.5f, 0.5f * ROWS - 0.5f, 0.9f * COLS, -0.95f * COLS, 0.3f};
            const float dist[5] = {0.2f, -0.3f, 0.01f, -0.02f, 0.1f}, wild[5] = {40.f, -300.f, 2.f, -3.f, 1e6f};
            const int shapes[][2] = {{ROWS, COLS}, {23, 31}, {1, 1}, {64, 80}};
            for (const auto& sh : shapes)
                for (const float* k : {dist, wild}) {
                    Out o(sh[0], sh[1]);
                    const float out[5] = {in[0] - 3.f, in[1] - 2.f, in[2] * 0.6f, in[3] * 0.6f, in[4]};
                    CHECK(vors_undistort_frame_host(g.data(), d.data(), ROWS, COLS, in, k, out, sh[0], sh[1], border, o.gray.data(), o.depth.data(),
                                                    o.map.data(), o.counts) == VORS_OK);
                    CHECK(o.counts[0] == (uint32_t)(sh[0] * sh[1]) && o.counts[1] <= o.counts[0] && o.counts[2] <= o.counts[0]);
                    for (uint16_t v : o.depth) {  // never interpolated: a value of the input, or 0
                        bool found = v == 0;
                        for (size_t i = 0; i < d.size() && !found; ++i) found = d[i] == v;
                        CHECK(found);
                    }
                    std::vector<int32_t> xy((size_t)sh[0] * sh[1] * 2);
                    for (int y = 0; y < sh[0]; ++y)
                        for (int x = 0; x < sh[1]; ++x) {
                            xy[2 * ((size_t)y * sh[1] + x)] = x;
                            xy[2 * ((size_t)y * sh[1] + x) + 1] = y;
                        }
                    std::vector<float> uv(xy.size());
                    CHECK(vors_undistort_source_host(in, k, out, sh[0] * sh[1], xy.data(), uv.data()) == VORS_OK);
                    for (size_t i = 0; i < uv.size(); ++i) CHECK(uv[i] == o.map[i] || (uv[i] != uv[i] && o.map[i] != o.map[i]));
                }
        }
    }
    {  // one plane of each kind alone; a 1 x 1 input
        Out o(ROWS, COLS);
        CHECK(vors_undistort_frame_host(g.data(), nullptr, ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, o.counts) == VORS_OK);
        CHECK(o.gray == g && o.counts[2] == 0);
        CHECK(vors_undistort_frame_host(nullptr, d.data(), ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 1, nullptr, o.depth.data(), nullptr, nullptr) == VORS_OK);
        CHECK(o.depth == d);
        std::vector<uint8_t> one(1, 200);
        CHECK(vors_undistort_frame_host(one.data(), nullptr, 1, 1, cam, nullptr, cam, ROWS, COLS, 1, o.gray.data(), nullptr, nullptr, nullptr) == VORS_OK);
        for (uint8_t v : o.gray) CHECK(v == 200);
    }
    {  // refusals: nothing written
        Out o(ROWS, COLS);
        const float nanv = std::nanf(""), bad_fu[5] = {cam[0], cam[1], 0.f, cam[3], 0.f}, bad_nan[5] = {cam[0], nanv, cam[2], cam[3], 0.f},
                    bad_dist[5] = {0.f, 0.f, 0.f, INFINITY, 0.f};
#define REFUSED(...) CHECK(vors_undistort_frame_host(__VA_ARGS__) == VORS_ERR_INVALID_ARGUMENT && o.untouched())
        REFUSED(nullptr, nullptr, ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 0, nullptr, nullptr, o.map.data(), o.counts);
        REFUSED(nullptr, d.data(), ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 0, o.gray.data(), o.depth.data(), nullptr, nullptr);
        REFUSED(g.data(), nullptr, ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 0, o.gray.data(), o.depth.data(), nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 0, nullptr, nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, nullptr, nullptr, cam, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, nullptr, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, bad_fu, nullptr, cam, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, bad_nan, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, bad_dist, cam, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 2, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, cam, ROWS, COLS, -1, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), 0, COLS, cam, nullptr, cam, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, 65536, cam, nullptr, cam, ROWS, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, cam, 0, COLS, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, cam, 32768, 16384, 0, o.gray.data(), nullptr, nullptr, nullptr);
        REFUSED(g.data(), d.data(), ROWS, COLS, cam, nullptr, cam, ROWS, COLS, 0, nullptr,
                reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(o.depth.data()) + 1), nullptr, nullptr);
#undef REFUSED
    }
}

struct Reg {
    std::vector<uint64_t> zkey;
    std::vector<uint16_t> depth;
    std::vector<uint32_t> src;
    uint32_t counts[VORS_REGISTER_COUNTS];
    Reg(int rows, int cols) : zkey((size_t)rows * cols, 7), depth((size_t)rows * cols, 7), src((size_t)rows * cols, 7), counts{7, 7, 7, 7} {}
    bool untouched() const {
        for (size_t i = 0; i < zkey.size(); ++i) if (zkey[i] != 7 || depth[i] != 7 || src[i] != 7) return false;
        return counts[0] == 7 && counts[1] == 7 && counts[2] == 7 && counts[3] == 7;
    }
};

static void registration() {
    const float cam[5] = {COLS / 2.f - 0.5f, ROWS / 2.f - 0.5f, 100.f, 100.f, 0.f};
    std::vector<uint16_t> d((size_t)ROWS * COLS);
    for (size_t i = 0; i < d.size(); ++i) d[i] = (i % 13 == 5) ? 0 : (uint16_t)(1000 + 53 * (i % 97));
    {  // identity: 5 d, holes stay holes
        Reg o(ROWS, COLS);
        CHECK(vors_register_depth_host(d.data(), cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, 5000.f, 1, o.zkey.data(), o.depth.data(),
                                       o.src.data(), o.counts) == VORS_OK);
        for (size_t i = 0; i < d.size(); ++i) CHECK(o.depth[i] == 5 * d[i] && o.src[i] == (d[i] ? (uint32_t)i : 0xFFFFFFFFu));
        CHECK(o.counts[0] == o.counts[3] && o.counts[1] == o.counts[0] && o.counts[2] == o.counts[0]);
    }
    const float pose[7] = {0.05f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    for (int fp = 1; fp <= 3; ++fp) {  // an integer baseline with a near strip in front of a far plane; every footprint at the borders
        std::vector<uint16_t> p((size_t)ROWS * COLS, 10000);
        for (int y = 0; y < ROWS; ++y)
            for (int x = 10; x < 16; ++x) p[(size_t)y * COLS + x] = 5000;
        Reg o(ROWS, COLS);
        CHECK(vors_register_depth_host(p.data(), cam, ROWS, COLS, 5000.f, pose, cam, ROWS, COLS, 5000.f, fp, o.zkey.data(), o.depth.data(),
                                       o.src.data(), o.counts) == VORS_OK);
        for (int y = 0; y < ROWS; ++y)
            for (int x = 15; x < 21; ++x) CHECK(o.depth[(size_t)y * COLS + x] == 5000);
        CHECK(o.counts[0] == (uint32_t)(ROWS * COLS) && o.counts[2] <= o.counts[1]);
        if (fp == 1) CHECK(o.counts[3] < o.counts[2]);
    }
    {  // a rotated pose that throws most points out of the window, points behind the camera, a tiny colour plane
        const float turn[7] = {0.3f, -0.2f, -3.0f, 0.f, 0.7071068f, 0.f, 0.7071068f};
        const int shapes[][2] = {{1, 1}, {3, 50}, {58, 74}};
        for (const auto& sh : shapes)
            for (int fp = 1; fp <= 3; ++fp) {
                Reg o(sh[0], sh[1]);
                CHECK(vors_register_depth_host(d.data(), cam, ROWS, COLS, 1000.f, fp == 2 ? nullptr : turn, cam, sh[0], sh[1], 1000.f, fp, o.zkey.data(),
                                               nullptr, nullptr, o.counts) == VORS_OK);
                CHECK(o.counts[1] <= o.counts[0] && o.counts[2] <= o.counts[1] && o.counts[3] <= (uint32_t)(sh[0] * sh[1]));
            }
    }
    {  // the tie-break: half the focal and half the size, a constant plane
        const int rows = 28, cols = 36;
        const float dcam[5] = {cols / 2.f - 0.5f, rows / 2.f - 0.5f, 64.f, 64.f, 0.f}, ccam[5] = {cols / 4.f - 0.5f, rows / 4.f - 0.5f, 32.f, 32.f, 0.f};
        std::vector<uint16_t> p((size_t)rows * cols, 7500);
        Reg o(rows / 2, cols / 2);
        CHECK(vors_register_depth_host(p.data(), dcam, rows, cols, 5000.f, nullptr, ccam, rows / 2, cols / 2, 5000.f, 1, o.zkey.data(), o.depth.data(),
                                       o.src.data(), o.counts) == VORS_OK);
        CHECK(o.counts[2] == (uint32_t)(rows * cols) && o.counts[3] == (uint32_t)(rows * cols / 4));
        for (size_t q = 0; q < o.src.size(); ++q) {  // the winner is the first source pixel, in index order, that lands on q
            const int sx = (int)(o.src[q] % cols), sy = (int)(o.src[q] / cols);
            const int lx = (int)std::floor(0.5 * (sx - dcam[0]) + ccam[0] + 0.5), ly = (int)std::floor(0.5 * (sy - dcam[1]) + ccam[1] + 0.5);
            CHECK((size_t)ly * (cols / 2) + lx == q);
            if (sx > 0) CHECK((int)std::floor(0.5 * (sx - 1 - dcam[0]) + ccam[0] + 0.5) != lx);
            if (sy > 0) CHECK((int)std::floor(0.5 * (sy - 1 - dcam[1]) + ccam[1] + 0.5) != ly);
        }
    }
    {  // footprint 2 fills a 2x up-scaled plane that footprint 1 leaves with holes
        const float dcam[5] = {COLS / 2.f - 0.5f, ROWS / 2.f - 0.5f, 32.f, 32.f, 0.f}, ccam[5] = {COLS - 0.5f, ROWS - 0.5f, 64.f, 64.f, 0.f};
        std::vector<uint16_t> p((size_t)ROWS * COLS, 6000);
        Reg one(2 * ROWS, 2 * COLS), two(2 * ROWS, 2 * COLS);
        CHECK(vors_register_depth_host(p.data(), dcam, ROWS, COLS, 5000.f, nullptr, ccam, 2 * ROWS, 2 * COLS, 5000.f, 1, one.zkey.data(), one.depth.data(),
                                       nullptr, one.counts) == VORS_OK);
        CHECK(vors_register_depth_host(p.data(), dcam, ROWS, COLS, 5000.f, nullptr, ccam, 2 * ROWS, 2 * COLS, 5000.f, 2, two.zkey.data(), two.depth.data(),
                                       nullptr, two.counts) == VORS_OK);
        CHECK(one.counts[3] == (uint32_t)(ROWS * COLS) && two.counts[3] > 3 * one.counts[3]);
    }
    {  // refusals: nothing written
        Reg o(ROWS, COLS);
#define REFUSED(...) CHECK(vors_register_depth_host(__VA_ARGS__) == VORS_ERR_INVALID_ARGUMENT && o.untouched())
        REFUSED(nullptr, cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, 1000.f, 1, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), nullptr, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, 1000.f, 1, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 1000.f, nullptr, nullptr, ROWS, COLS, 1000.f, 1, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, 1000.f, 1, nullptr, o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, 1000.f, 0, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, 1000.f, 4, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, 0, COLS, 1000.f, nullptr, cam, ROWS, COLS, 1000.f, 1, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, 65536, 1000.f, 1, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 0.f, nullptr, cam, ROWS, COLS, 1000.f, 1, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, std::nanf(""), 1, o.zkey.data(), o.depth.data(), o.src.data(), o.counts);
        REFUSED(d.data(), cam, ROWS, COLS, 1000.f, nullptr, cam, ROWS, COLS, 1000.f, 1,
                reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(o.zkey.data()) + 4), o.depth.data(), o.src.data(), o.counts);
#undef REFUSED
    }
}

int main() {
    undistortion();
    registration();
    if (failures) return 1;
    std::printf("frontend_host_check: ok\n");
    return 0;
}
