// Stand-alone check of vors_icp_points_host for a sanitizer build of the host code (`make icp_host_check`: operators.cpp and this file with
// -fsanitize=address,undefined on the host side; runs without a GPU). Every list, plane and output is a heap block of exactly its size,
// so a gather outside the plane or a rank outside the list would be reported. Cases: lists of count 0 and 1, counts around the chunk of
// 1024, ranges, points that land on the four borders and corners of the plane, points whose pixel lies just outside it, behind the
// camera and far away, a 1 x 1 plane. Then vors_icp_points_robust_host: counts around the chunk, ranges, the four combinations of its two
// options, a plane of frame normals (its own heap block) with zero normals, and the neutral case against vors_icp_points_host's bits.
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
    const float identity[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    const float tilted[7] = {0.01f, -0.02f, 0.015f, 0.01f, -0.008f, 0.012f, 0.99984f};
    const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {5, 7}, {12, 16}};
    for (const auto& sh : shapes) {
        const int rows = sh[0], cols = sh[1];
        const float cam[5] = {0.5f * (cols - 1), 0.5f * (rows - 1), 10.0f, 10.5f, 0.0f};
        std::vector<uint16_t> depth((size_t)rows * cols);
        for (size_t i = 0; i < depth.size(); ++i) depth[i] = (i % 7 == 3) ? 0 : (uint16_t)(5000 + 13 * (i % 11));
        // one point per pixel of the plane and of a one-pixel frame around it, at 1 m: the frame's pixels lie outside the plane
        std::vector<float> xyz, nrm;
        for (int y = -1; y <= rows; ++y)
            for (int x = -1; x <= cols; ++x) {
                xyz.push_back(((float)x - cam[0]) / cam[2]);
                xyz.push_back(((float)y - cam[1]) / cam[3]);
                xyz.push_back(1.0f);
                nrm.push_back(0.0f);
                nrm.push_back(0.0f);
                nrm.push_back((x + y) % 5 == 0 ? 0.0f : -1.0f);  // some without a normal
            }
        // ... and points behind the camera, at the camera, far off axis and not finite
        const float odd[][3] = {{0.f, 0.f, -1.f}, {0.f, 0.f, 0.f}, {1e30f, -1e30f, 1.f}, {NAN, 0.f, 1.f}, {0.f, INFINITY, 1.f}};
        for (const auto& o : odd) {
            for (int q = 0; q < 3; ++q) xyz.push_back(o[q]);
            nrm.push_back(0.6f);
            nrm.push_back(0.0f);
            nrm.push_back(-0.8f);
        }
        const int capacity = (int)(xyz.size() / 3);
        const uint32_t counts[] = {0u, 1u, (uint32_t)capacity, (uint32_t)capacity + 9u};
        for (uint32_t count : counts)
            for (int iters = 0; iters <= 2; ++iters)
                for (const float* pose : {identity, tilted}) {
                    std::vector<float> res((size_t)capacity, 42.f), sums(29), out(7);
                    vors_icp_stats st;
                    CHECK(vors_icp_points_host(xyz.data(), nrm.data(), count, capacity, nullptr, pose, depth.data(), cam, rows, cols, 5000.f, 0.5f,
                                               0.0f, 1e-6f, iters, 6, out.data(), &st, sums.data(), res.data()) == VORS_OK);
                    const uint32_t n = count < (uint32_t)capacity ? count : (uint32_t)capacity;
                    CHECK(st.considered == n && st.matched <= n && st.matched == (uint32_t)sums[1]);
                    uint32_t finite = 0;
                    for (uint32_t r = 0; r < (uint32_t)capacity; ++r) {
                        if (r >= n) CHECK(res[r] == 42.f);
                        else if (!std::isnan(res[r])) ++finite;
                    }
                    if (pose == identity && iters == 0) CHECK(finite == st.matched);
                    if (n == 0) CHECK(st.matched == 0 && sums[0] == 0.f && st.status == (iters ? VORS_ICP_TOO_FEW : VORS_ICP_ITERATIONS));
                    // a range: ranks [3, 3 + 5) clipped to the list, everything else untouched
                    const uint32_t range[2] = {3u, 5u};
                    std::vector<float> r2((size_t)capacity, 42.f);
                    CHECK(vors_icp_points_host(xyz.data(), nrm.data(), count, capacity, range, pose, depth.data(), cam, rows, cols, 5000.f, 0.5f, 0.0f,
                                               1e-6f, iters, 6, out.data(), &st, nullptr, r2.data()) == VORS_OK);
                    const uint32_t f = 3u < n ? 3u : n, l = 5u > n - f ? n : f + 5u;
                    CHECK(st.considered == l - f);
                    for (uint32_t r = 0; r < (uint32_t)capacity; ++r)
                        if (r < f || r >= l) CHECK(r2[r] == 42.f);
                }
    }
    // a list longer than two chunks on the largest plane: every point at the centre pixel
    {
        const int rows = 4, cols = 4, capacity = 2500;
        const float cam[5] = {1.5f, 1.5f, 8.f, 8.f, 0.f};
        std::vector<uint16_t> depth((size_t)rows * cols, 5000);
        std::vector<float> xyz((size_t)capacity * 3), nrm((size_t)capacity * 3);
        for (int i = 0; i < capacity; ++i) {
            xyz[3 * i] = 0.001f * (float)(i % 50);
            xyz[3 * i + 1] = -0.001f * (float)(i % 31);
            xyz[3 * i + 2] = 1.0f + 0.0001f * (float)(i % 17);
            nrm[3 * i] = 0.0f;
            nrm[3 * i + 1] = 0.0f;
            nrm[3 * i + 2] = -1.0f;
        }
        for (uint32_t count : {1023u, 1024u, 1025u, 2500u}) {
            std::vector<float> res((size_t)capacity), sums(29), out(7);
            vors_icp_stats st;
            CHECK(vors_icp_points_host(xyz.data(), nrm.data(), count, capacity, nullptr, identity, depth.data(), cam, rows, cols, 5000.f, 0.5f, 0.0f,
                                       0.0f, 1, 6, out.data(), &st, sums.data(), res.data()) == VORS_OK);
            CHECK(st.considered == count && st.matched > 0);
        }
    }
    // the robust entry: counts around the chunk boundary, ranges, the four option combinations, a frame-normal plane with zero normals.
    // The plane of normals is a heap block of exactly rows * cols * 3 floats: a gather outside it would be reported.
    {
        const int rows = 5, cols = 7, capacity = 2500;
        const float cam[5] = {3.0f, 2.0f, 8.f, 8.5f, 0.f};
        std::vector<uint16_t> depth((size_t)rows * cols);
        std::vector<float> frame_normals((size_t)rows * cols * 3, 0.0f);
        for (size_t i = 0; i < depth.size(); ++i) {
            depth[i] = (i % 9 == 4) ? 0 : (uint16_t)(5000 + 7 * (i % 5));
            if (i % 4 != 1) {  // (every fourth pixel: no frame normal)
                frame_normals[3 * i] = (i % 3 == 0) ? 0.6f : 0.0f;  // (some tilted beyond the gate)
                frame_normals[3 * i + 2] = (i % 3 == 0) ? -0.8f : -1.0f;
            }
        }
        std::vector<float> xyz((size_t)capacity * 3), nrm((size_t)capacity * 3);
        for (int i = 0; i < capacity; ++i) {  // spread over the plane and a margin around it, depths around the plane's
            xyz[3 * i] = ((float)(i % 9) - 1.0f - cam[0]) / cam[2];
            xyz[3 * i + 1] = ((float)((i / 9) % 7) - 1.0f - cam[1]) / cam[3];
            xyz[3 * i + 2] = 1.0f + 0.002f * (float)(i % 23) - 0.02f;
            xyz[3 * i] *= xyz[3 * i + 2];
            xyz[3 * i + 1] *= xyz[3 * i + 2];
            nrm[3 * i + 2] = (i % 11 == 0) ? 0.0f : ((i % 13 == 0) ? 1.0f : -1.0f);  // none / back-facing / facing the camera
        }
        const uint32_t range[2] = {1000u, 1030u};
        for (uint32_t count : {0u, 1u, 1023u, 1024u, 1025u, 2500u, 2600u})
            for (int combo = 0; combo < 4; ++combo)
                for (const uint32_t* rg : {(const uint32_t*)nullptr, range})
                    for (int iters = 0; iters <= 2; iters += 2) {
                        const float* fn = (combo & 1) ? frame_normals.data() : nullptr;
                        const float huber_m = (combo & 2) ? 0.004f : 0.0f;
                        std::vector<float> res((size_t)capacity, 42.f), sums(29), out(7);
                        uint32_t gates[VORS_ICP_GATE_COUNTS] = {9u, 9u, 9u, 9u};
                        vors_icp_stats st;
                        CHECK(vors_icp_points_robust_host(xyz.data(), nrm.data(), count, capacity, rg, tilted, depth.data(), cam, rows, cols, 5000.f,
                                                          0.05f, 0.0f, 1e-6f, iters, 6, fn, 0.9f, huber_m, out.data(), &st, sums.data(), res.data(),
                                                          gates) == VORS_OK);
                        const uint32_t n = count < (uint32_t)capacity ? count : (uint32_t)capacity;
                        const uint32_t f = !rg ? 0u : (rg[0] < n ? rg[0] : n), l = !rg ? n : (rg[1] > n - f ? n : f + rg[1]);
                        CHECK(st.considered == l - f);
                        CHECK(gates[0] <= l - f && gates[1] <= gates[0] && gates[2] <= gates[1] && gates[3] <= gates[2]);
                        CHECK(gates[2] == st.matched && st.matched == (uint32_t)sums[1]);
                        if (!(combo & 1)) CHECK(gates[2] == gates[1]);
                        if (!(combo & 2)) CHECK(gates[3] == 0u);
                        uint32_t finite = 0;
                        for (uint32_t r = 0; r < (uint32_t)capacity; ++r) {
                            if (r < f || r >= l) CHECK(res[r] == 42.f);
                            else if (!std::isnan(res[r])) ++finite;
                        }
                        CHECK(finite == st.matched);
                        if (combo == 0) {  // the neutral case: vors_icp_points_host's bits
                            std::vector<float> res0((size_t)capacity, 42.f), sums0(29), out0(7);
                            vors_icp_stats st0;
                            CHECK(vors_icp_points_host(xyz.data(), nrm.data(), count, capacity, rg, tilted, depth.data(), cam, rows, cols, 5000.f, 0.05f,
                                                       0.0f, 1e-6f, iters, 6, out0.data(), &st0, sums0.data(), res0.data()) == VORS_OK);
                            CHECK(std::memcmp(out.data(), out0.data(), 28) == 0 && std::memcmp(sums.data(), sums0.data(), 116) == 0);
                            CHECK(std::memcmp(res.data(), res0.data(), (size_t)capacity * 4) == 0 && std::memcmp(&st, &st0, sizeof st) == 0);
                        }
                    }
        // without the optional outputs
        std::vector<float> out(7);
        CHECK(vors_icp_points_robust_host(xyz.data(), nrm.data(), 2500u, capacity, nullptr, identity, depth.data(), cam, rows, cols, 5000.f, 0.05f,
                                          0.0f, 1e-6f, 1, 6, frame_normals.data(), 0.5f, 0.01f, out.data(), nullptr, nullptr, nullptr, nullptr) ==
              VORS_OK);
    }
    if (failures) return 1;
    std::printf("icp_host_check: ok\n");
    return 0;
}
