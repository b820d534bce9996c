// Stand-alone check of vors_icp_points_joint_host for a sanitizer build of the host code (`make icp_joint_host_check`: operators.cpp and this
// file with -fsanitize=address,undefined on the host side; runs on the CPU, never on a GPU machine). Every list, plane and output is a heap
// block of exactly its size, so a tap outside the grey plane or a grey byte outside the list would be reported. Cases: counts 0, 1, 1025
// and beyond the capacity, ranges, a frame whose border pixels are hit (one point per pixel and per half pixel, so that footprints touch
// the last row and column and the pixels outside), planes of one row and of one column (no footprint fits), the four combinations of the
// two Huber weights with and without frame normals, NULL optionals, NULL grey pointers with photo_scale_m = 0 against
// vors_icp_points_robust_host's bits.
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main() {
    const float tilted[7] = {0.01f, -0.02f, 0.015f, 0.01f, -0.008f, 0.012f, 0.99984f};
    const float identity[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    const int shapes[][2] = {{1, 9}, {9, 1}, {2, 2}, {5, 7}, {12, 16}};
    for (const auto& sh : shapes) {
        const int rows = sh[0], cols = sh[1];
        const float cam[5] = {0.5f * (cols - 1), 0.5f * (rows - 1), 10.0f, 10.5f, 0.1f};
        std::vector<uint16_t> depth((size_t)rows * cols);
        std::vector<uint8_t> frame_gray((size_t)rows * cols);
        std::vector<float> frame_normals((size_t)rows * cols * 3, 0.0f);
        for (size_t i = 0; i < depth.size(); ++i) {
            depth[i] = (i % 7 == 3) ? 0 : (uint16_t)(5000 + 13 * (i % 11));
            frame_gray[i] = (uint8_t)(37 * i + 11);
            if (i % 4 != 1) frame_normals[3 * i + 2] = -1.0f;
        }
        // one point per half pixel of the plane and of a one-pixel frame around it, at 1 m: footprints that touch every border
        std::vector<float> xyz, nrm;
        std::vector<uint8_t> gray;
        for (int y2 = -2; y2 <= 2 * rows; ++y2)
            for (int x2 = -2; x2 <= 2 * cols; ++x2) {
                const float v = 0.5f * (float)y2, u = 0.5f * (float)x2;
                const float py = (v - cam[1]) / cam[3];
                xyz.push_back(((u - cam[0]) - cam[4] * py) / cam[2]);
                xyz.push_back(py);
                xyz.push_back(1.0f);
                nrm.push_back(0.0f);
                nrm.push_back(0.0f);
                nrm.push_back((x2 + y2) % 5 == 0 ? 0.0f : -1.0f);  // some without a normal
                gray.push_back((uint8_t)(x2 * 7 + y2 * 3));
            }
        const float odd[][3] = {{0.f, 0.f, -1.f}, {0.f, 0.f, 0.f}, {1e30f, -1e30f, 1.f}, {NAN, 0.f, 1.f}, {0.f, INFINITY, 1.f}};
        for (const auto& o : odd) {
            for (int q = 0; q < 3; ++q) xyz.push_back(o[q]);
            nrm.push_back(0.6f);
            nrm.push_back(0.0f);
            nrm.push_back(-0.8f);
            gray.push_back(200);
        }
        const int capacity = (int)gray.size();
        const uint32_t range[2] = {3u, 40u};
        for (uint32_t count : {0u, 1u, (uint32_t)capacity, (uint32_t)capacity + 9u})
            for (int combo = 0; combo < 8; ++combo)
                for (const uint32_t* rg : {(const uint32_t*)nullptr, range})
                    for (const float* pose : {identity, tilted}) {
                        const float* fn = (combo & 1) ? frame_normals.data() : nullptr;
                        const float huber_m = (combo & 2) ? 0.004f : 0.0f, photo_huber = (combo & 4) ? 20.0f : 0.0f;
                        std::vector<float> res((size_t)capacity, 42.f), pres((size_t)capacity, 42.f), sums(29), out(7);
                        uint32_t gates[VORS_ICP_GATE_COUNTS] = {9u, 9u, 9u, 9u}, photos[VORS_ICP_PHOTO_COUNTS] = {9u, 9u};
                        vors_icp_stats st;
                        CHECK(vors_icp_points_joint_host(xyz.data(), nrm.data(), gray.data(), count, capacity, rg, pose, depth.data(),
                                                         frame_gray.data(), cam, rows, cols, 5000.f, 0.5f, 0.0f, 1e-6f, 2, 6, fn, 0.9f, huber_m,
                                                         0.0005f, photo_huber, out.data(), &st, sums.data(), res.data(), gates, pres.data(),
                                                         photos) == VORS_OK);
                        const uint32_t n = count < (uint32_t)capacity ? count : (uint32_t)capacity;
                        const uint32_t f = !rg ? 0u : (rg[0] < n ? rg[0] : n), l = !rg ? n : (rg[1] > n - f ? n : f + rg[1]);
                        CHECK(st.considered == l - f && gates[2] == st.matched && photos[0] <= gates[2] && photos[1] <= photos[0]);
                        if (!(combo & 4)) CHECK(photos[1] == 0u);
                        if (rows < 2 || cols < 2) CHECK(photos[0] == 0u);
                        uint32_t finite = 0, pfinite = 0;
                        for (uint32_t r = 0; r < (uint32_t)capacity; ++r) {
                            if (r < f || r >= l) {
                                CHECK(res[r] == 42.f && pres[r] == 42.f);
                                continue;
                            }
                            finite += std::isnan(res[r]) ? 0u : 1u;
                            pfinite += std::isnan(pres[r]) ? 0u : 1u;
                            if (!std::isnan(pres[r])) CHECK(!std::isnan(res[r]) && std::fabs(pres[r]) <= 255.f);
                        }
                        CHECK(finite == st.matched && pfinite == photos[0]);
                    }
        // the identity pose on the largest plane: the points on whole pixels of the last row and column are matched but not PHOTO
        if (rows == 12) {
            std::vector<float> res((size_t)capacity), pres((size_t)capacity), out(7);
            uint32_t photos[VORS_ICP_PHOTO_COUNTS];
            CHECK(vors_icp_points_joint_host(xyz.data(), nrm.data(), gray.data(), (uint32_t)capacity, capacity, nullptr, identity, depth.data(),
                                             frame_gray.data(), cam, rows, cols, 5000.f, 0.5f, 0.0f, 1e-6f, 0, 6, nullptr, 0.0f, 0.0f, 0.0005f, 0.0f,
                                             out.data(), nullptr, nullptr, res.data(), nullptr, pres.data(), photos) == VORS_OK);
            uint32_t border_matched = 0;
            const int w = 2 * cols + 3;
            for (int y2 = 0; y2 <= 2 * (rows - 1); y2 += 2) {
                const size_t r = (size_t)(y2 + 2) * w + (size_t)(2 * (cols - 1) + 2);  // (u, v) = (cols - 1, y)
                if (!std::isnan(res[r])) {
                    ++border_matched;
                    CHECK(std::isnan(pres[r]));
                }
            }
            CHECK(border_matched > 0 && photos[0] > 0);
        }
    }
    // counts around the chunk of 1024 on a small plane, NULL optionals, and the neutral case against the robust twin's bits
    {
        const int rows = 5, cols = 7, capacity = 2500;
        const float cam[5] = {3.0f, 2.0f, 8.f, 8.5f, 0.f};
        std::vector<uint16_t> depth((size_t)rows * cols);
        std::vector<uint8_t> frame_gray((size_t)rows * cols), gray((size_t)capacity);
        for (size_t i = 0; i < depth.size(); ++i) {
            depth[i] = (i % 9 == 4) ? 0 : (uint16_t)(5000 + 7 * (i % 5));
            frame_gray[i] = (uint8_t)(91 * i);
        }
        std::vector<float> xyz((size_t)capacity * 3), nrm((size_t)capacity * 3);
        for (int i = 0; i < capacity; ++i) {  // spread over the plane and a margin around it, at fractions of a pixel
            xyz[3 * i + 2] = 1.0f + 0.002f * (float)(i % 23) - 0.02f;
            xyz[3 * i] = (0.125f * (float)(i % 72) - 1.0f - cam[0]) / cam[2] * xyz[3 * i + 2];
            xyz[3 * i + 1] = (0.125f * (float)((i / 72) % 56) - 1.0f - cam[1]) / cam[3] * xyz[3 * i + 2];
            nrm[3 * i + 2] = (i % 11 == 0) ? 0.0f : -1.0f;
            gray[(size_t)i] = (uint8_t)(i * 13);
        }
        const uint32_t range[2] = {1000u, 1030u};
        for (uint32_t count : {0u, 1u, 1023u, 1024u, 1025u, 2500u, 2600u})
            for (const uint32_t* rg : {(const uint32_t*)nullptr, range})
                for (int iters = 0; iters <= 2; iters += 2) {
                    std::vector<float> res((size_t)capacity, 42.f), sums(29), out(7), res0((size_t)capacity, 42.f), sums0(29), out0(7);
                    uint32_t gates[VORS_ICP_GATE_COUNTS], gates0[VORS_ICP_GATE_COUNTS], photos[VORS_ICP_PHOTO_COUNTS] = {9u, 9u};
                    vors_icp_stats st, st0;
                    CHECK(vors_icp_points_joint_host(xyz.data(), nrm.data(), gray.data(), count, capacity, rg, tilted, depth.data(), frame_gray.data(),
                                                     cam, rows, cols, 5000.f, 0.05f, 0.0f, 1e-6f, iters, 6, nullptr, 0.0f, 0.004f, 0.0005f, 15.0f,
                                                     out.data(), &st, sums.data(), res.data(), gates, nullptr, photos) == VORS_OK);
                    CHECK(photos[0] <= st.matched && gates[2] == st.matched);
                    if (count >= 1023u && !rg) CHECK(photos[0] > 0u);
                    // photo_scale_m = 0 with NULL grey pointers
                    CHECK(vors_icp_points_joint_host(xyz.data(), nrm.data(), nullptr, count, capacity, rg, tilted, depth.data(), nullptr, cam, rows, cols,
                                                     5000.f, 0.05f, 0.0f, 1e-6f, iters, 6, nullptr, 0.0f, 0.004f, 0.0f, 15.0f, out.data(), &st,
                                                     sums.data(), res.data(), gates, nullptr, photos) == VORS_OK);
                    CHECK(vors_icp_points_robust_host(xyz.data(), nrm.data(), count, capacity, rg, tilted, depth.data(), cam, rows, cols, 5000.f, 0.05f,
                                                      0.0f, 1e-6f, iters, 6, nullptr, 0.0f, 0.004f, out0.data(), &st0, sums0.data(), res0.data(),
                                                      gates0) == VORS_OK);
                    CHECK(photos[0] == 0u && photos[1] == 0u && std::memcmp(gates, gates0, sizeof gates) == 0);
                    CHECK(std::memcmp(out.data(), out0.data(), 28) == 0 && std::memcmp(sums.data(), sums0.data(), 116) == 0);
                    CHECK(std::memcmp(res.data(), res0.data(), (size_t)capacity * 4) == 0 && std::memcmp(&st, &st0, sizeof st) == 0);
                }
        // without any optional output
        std::vector<float> out(7);
        CHECK(vors_icp_points_joint_host(xyz.data(), nrm.data(), gray.data(), 2500u, capacity, nullptr, identity, depth.data(), frame_gray.data(), cam,
                                         rows, cols, 5000.f, 0.05f, 0.0f, 1e-6f, 1, 6, nullptr, 0.5f, 0.01f, 0.0005f, 10.0f, out.data(), nullptr, nullptr,
                                         nullptr, nullptr, nullptr, nullptr) == VORS_OK);
    }
    if (failures) return 1;
    std::printf("icp_joint_host_check: ok\n");
    return 0;
}
