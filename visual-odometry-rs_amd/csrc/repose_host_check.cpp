// Stand-alone check of vors_repose_points_host and vors_voxel_filter_points_host for a sanitizer build of the host code (`make
// repose_host_check`: operators.cpp and this file with -fsanitize=address,undefined on the host side; runs without a GPU). Every list,
// record array and output is a heap block of exactly its size, so a rank or record touched outside the clipped count would be reported.
// Cases: empty lists, zero-count segments, counts beyond capacity, segment counts beyond max_keyframes, sentinel and out-of-range nodes,
// non-finite rows and poses, in-place outputs, the overflowing table, an emptied middle segment.
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

static vors_map_segment segment(int frame, uint32_t first, uint32_t count, float tx, float angle) {
    vors_map_segment s{};
    s.frame = frame; s.first = first; s.count = count;
    s.pose7[0] = tx; s.pose7[1] = -0.5f * tx; s.pose7[2] = 0.25f;
    s.pose7[4] = std::sin(0.5f * angle); s.pose7[6] = std::cos(0.5f * angle);
    return s;
}

int main() {
    const float nan = std::nanf("");
    // ---- re-pose ----
    const uint32_t sizes[6] = {0, 3, 0, 5, 1, 4};
    std::vector<vors_map_segment> seg;
    uint32_t first = 0;
    for (int k = 0; k < 6; ++k) {
        seg.push_back(segment(2 * k, first, sizes[k], 0.1f * (float)(k + 1), 0.2f * (float)k));
        first += sizes[k];
    }
    const int cap = 13;
    std::vector<float> xyz((size_t)cap * 3), nrm((size_t)cap * 3);
    for (size_t i = 0; i < xyz.size(); ++i) {
        xyz[i] = 0.37f * (float)(i % 11) - 1.5f;
        nrm[i] = i % 3 == 0 ? 1.0f : 0.0f;
    }
    xyz[3 * 4 + 1] = nan;                   // a NaN row
    nrm[3 * 6] = INFINITY;                  // a non-finite normal
    std::vector<float> poses(5 * 7);
    for (int k = 0; k < 5; ++k) std::memcpy(&poses[7 * k], segment(0, 0, 0, -0.2f * (float)(k + 1), 0.1f * (float)(k + 2)).pose7, 28);
    std::memcpy(&poses[7 * 2], seg[3].pose7, 28);  // node 2 = segment 3's own pose: kept by identical bits
    poses[7 * 4 + 5] = INFINITY;                   // node 4: a non-finite pose
    const uint32_t node_of[6] = {0, 1, 0xFFFFFFFFu, 2, 4, 9};  // a sentinel, a non-finite pose, an index beyond the graph
    const uint32_t counts_in[] = {0, 1, 8, 13, 14, 0xFFFFFFFFu}, nsegs_in[] = {0, 1, 4, 6, 7, 0xFFFFFFFFu};
    for (uint32_t count : counts_in)
        for (uint32_t n_seg : nsegs_in)
            for (int with_table = 0; with_table < 2; ++with_table) {
                std::vector<float> xo((size_t)cap * 3, 7.f), no((size_t)cap * 3, 7.f);
                std::vector<vors_map_segment> so(6);
                uint32_t c[VORS_REPOSE_COUNTS];
                CHECK(vors_repose_points_host(xyz.data(), nrm.data(), count, cap, seg.data(), n_seg, 6, poses.data(), with_table ? 5u : 3u, 5,
                                              with_table ? node_of : nullptr, xo.data(), no.data(), so.data(), c) == VORS_OK);
                const uint32_t total = count < (uint32_t)cap ? count : (uint32_t)cap;
                CHECK(c[0] + c[1] + c[2] + c[3] == total);
                for (size_t i = (size_t)total * 3; i < xo.size(); ++i) CHECK(xo[i] == 7.f && no[i] == 7.f);
                if (total > 4) CHECK(std::memcmp(&xo[12], &xyz[12], 12) == 0 && c[2] == 1);
                if (with_table && n_seg >= 4 && total >= 8)
                    CHECK(std::memcmp(&xo[9], &xyz[9], 15 * 4) == 0);  // segment 3 (ranks 3..7) keeps its bits
                // in place: the same bits
                std::vector<float> xi = xyz, ni = nrm;
                std::vector<vors_map_segment> si = seg;
                CHECK(vors_repose_points_host(xi.data(), ni.data(), count, cap, si.data(), n_seg, 6, poses.data(), with_table ? 5u : 3u, 5,
                                              with_table ? node_of : nullptr, xi.data(), ni.data(), si.data(), nullptr) == VORS_OK);
                CHECK(std::memcmp(xi.data(), xo.data(), (size_t)total * 12) == 0 && std::memcmp(ni.data(), no.data(), (size_t)total * 12) == 0);
                const uint32_t n_rec = n_seg < 6u ? n_seg : 6u;
                CHECK(std::memcmp(si.data(), so.data(), (size_t)n_rec * sizeof(vors_map_segment)) == 0);
            }
    // only normals, only points; refusals with nothing written
    {
        std::vector<float> no((size_t)cap * 3, 7.f);
        CHECK(vors_repose_points_host(xyz.data(), nrm.data(), 13, cap, seg.data(), 6, 6, poses.data(), 5, 5, nullptr, nullptr, no.data(), nullptr, nullptr) == VORS_OK);
        CHECK(vors_repose_points_host(xyz.data(), nullptr, 13, cap, seg.data(), 6, 6, poses.data(), 5, 5, nullptr, nullptr, no.data(), nullptr, nullptr) ==
              VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_repose_points_host(xyz.data(), nrm.data(), 13, cap, seg.data(), 6, 6, poses.data(), 5, 5, nullptr, nullptr, nullptr, nullptr, nullptr) ==
              VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_repose_points_host(xyz.data(), nrm.data(), 13, cap, seg.data(), 6, 6, poses.data(), 5, 5, nullptr, xyz.data() + 3, nullptr, nullptr, nullptr) ==
              VORS_ERR_INVALID_ARGUMENT);
    }
    // ---- filter ----
    for (int n : {1, 2, 63, 64, 65, 200}) {
        std::vector<float> p((size_t)n * 3);
        for (int i = 0; i < n; ++i) {  // voxel i % 65 of a row of voxels: 65 distinct ones from n = 65 on
            p[3 * i] = 0.1f * (float)(i % 65) + 0.05f;
            p[3 * i + 1] = 0.01f * (float)(i / 65);
            p[3 * i + 2] = i % 17 == 5 ? nan : 1.0f;
        }
        std::vector<uint32_t> pixel(n), index(n, 77u), po(n, 77u);
        std::vector<uint8_t> gray(n, 9), go(n, 3);
        for (int i = 0; i < n; ++i) pixel[i] = 1000u + (uint32_t)i;
        std::vector<float> xo((size_t)n * 3, 7.f), no((size_t)n * 3, 7.f);
        const vors_map_segment recs[3] = {segment(0, 0, (uint32_t)n / 2, 0.1f, 0.f), segment(1, (uint32_t)n / 2, 0, 0.2f, 0.f),
                                          segment(2, (uint32_t)n / 2, (uint32_t)n - (uint32_t)n / 2, 0.3f, 0.f)};
        vors_map_segment so[3];
        for (uint32_t count : {0u, (uint32_t)n, (uint32_t)n + 5u}) {
            uint32_t kept = 99, over = 99;
            CHECK(vors_voxel_filter_points_host(p.data(), count, n, 0.1f, 64, pixel.data(), gray.data(), p.data(), recs, 3, 3, index.data(), &kept, &over,
                                                xo.data(), po.data(), go.data(), no.data(), so) == VORS_OK);
            CHECK(kept <= (count < (uint32_t)n ? count : (uint32_t)n) && over == (count && n > 70 ? 1u : 0u));
            CHECK(so[0].first == 0 && so[0].count + so[1].count + so[2].count == kept && so[1].count == 0 && so[2].first == so[0].count);
            for (uint32_t k = 0; k < kept; ++k) CHECK(po[k] == 1000u + index[k] && (k == 0 || index[k] > index[k - 1]));
        }
        uint32_t kept = 0, over = 0;
        CHECK(vors_voxel_filter_points_host(p.data(), (uint32_t)n, n, 0.1f, 48, nullptr, nullptr, nullptr, nullptr, 0, 0, index.data(), &kept, &over,
                                            nullptr, nullptr, nullptr, nullptr, nullptr) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_voxel_filter_points_host(p.data(), (uint32_t)n, n, 0.1f, 64, nullptr, nullptr, nullptr, nullptr, 0, 0, index.data(), &kept, &over,
                                            p.data(), nullptr, nullptr, nullptr, nullptr) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_voxel_filter_points_host(p.data(), (uint32_t)n, n, 0.1f, 64, nullptr, nullptr, nullptr, nullptr, 0, 0, index.data(), &kept, &over,
                                            nullptr, nullptr, nullptr, nullptr, nullptr) == VORS_OK);
    }
    CHECK(vors_voxel_filter_workspace_bytes(2, 1025, 64) == 2u * 64u * 16u + 2u * 2u * 4u + 2u * 4u);
    if (failures) return 1;
    std::printf("repose_host_check: ok\n");
    return 0;
}
