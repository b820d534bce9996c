// Stand-alone check of vors_depth_normals_host for a sanitizer build of the host code (`make normals_host_check`: operators.cpp and this
// file with -fsanitize=address,undefined on the host side; runs without a GPU). Every plane and list is a heap block of exactly its size,
// so a one-sided tap that read outside the plane would be reported. Border cases: 1 x 1, single rows and columns, steps wider than the
// plane, all four borders at every step, list entries on the corners and outside the plane.
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

int main() {
    const float cam[5] = {3.5f, 2.5f, 9.0f, -9.5f, 0.2f};
    const float pose[7] = {1.f, 2.f, 3.f, 0.1f, -0.2f, 0.3f, 0.9273618f};
    const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {2, 2}, {5, 7}, {8, 8}, {17, 3}};
    for (const auto& sh : shapes) {
        const int rows = sh[0], cols = sh[1];
        std::vector<uint16_t> depth((size_t)rows * cols);
        for (size_t i = 0; i < depth.size(); ++i) depth[i] = (i % 7 == 3) ? 0 : (uint16_t)(5000 + 37 * (i % 11));
        for (int step = 1; step <= 8; ++step) {
            std::vector<float> normals(depth.size() * 3);
            uint32_t counts[VORS_NORMAL_COUNTS];
            CHECK(vors_depth_normals_host(depth.data(), cam, rows, cols, 5000.f, step, 0.5f, step & 1 ? pose : nullptr, nullptr, 0, 0, nullptr,
                                          normals.data(), counts) == VORS_OK);
            CHECK(counts[0] == depth.size() && counts[1] <= counts[0] && counts[2] <= counts[1]);
            if (step >= rows || step >= cols) CHECK(counts[2] == 0);
            // the list form on the four corners, the centre and two pixels outside the plane
            const uint32_t pixel[7] = {0u,
                                       (uint32_t)(cols - 1),
                                       (uint32_t)(rows - 1) << 16,
                                       (uint32_t)(cols - 1) | (uint32_t)(rows - 1) << 16,
                                       (uint32_t)(cols / 2) | (uint32_t)(rows / 2) << 16,
                                       (uint32_t)cols,
                                       (uint32_t)rows << 16};
            std::vector<float> ln(7 * 3, 42.f);
            const uint32_t range[2] = {1, 100};
            CHECK(vors_depth_normals_host(depth.data(), cam, rows, cols, 5000.f, step, 0.5f, nullptr, pixel, 9, 7, range, ln.data(), counts) == VORS_OK);
            CHECK(counts[0] == 6 && ln[0] == 42.f && ln[3 * 5] == 0.f && ln[3 * 6 + 2] == 0.f);
        }
    }
    if (failures) return 1;
    std::printf("normals_host_check: ok\n");
    return 0;
}
