// Stand-alone check of vors_map_icp_window_host and vors_map_icp_verdict_host for a sanitizer build of the host code (`make
// map_icp_host_check`: operators.cpp and this file with -fsanitize=address,undefined; no GPU is used). Every segment array is a heap block
// of exactly the records the rule may read, so a read past the recorded segments is an error here. Window: last_keyframes 0, 1, n_rec,
// n_rec + 1, count above capacity, more keyframes than records, an empty map, against the definition restated. Verdict: every verdict in
// its priority, NaN in every field, equality on every threshold, the rotation test at 0 and pi, and the refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vors_hip.h"

#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            std::printf("map_icp_host_check: %s failed (line %d)\n", #x, __LINE__); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

static bool window_case(uint32_t n_segments, int max_keyframes, uint32_t per_keyframe, int capacity, int last_keyframes) {
    const uint32_t n_rec = n_segments < (uint32_t)max_keyframes ? n_segments : (uint32_t)max_keyframes;
    std::vector<vors_map_segment> seg(n_rec);  // exactly the recorded ones
    for (uint32_t k = 0; k < n_rec; ++k) {
        seg[k] = vors_map_segment{};
        seg[k].frame = (int32_t)k;
        seg[k].first = k * per_keyframe;
        seg[k].count = per_keyframe;
    }
    const uint32_t count = n_segments * per_keyframe;
    const uint32_t total = count < (uint32_t)capacity ? count : (uint32_t)capacity;
    uint32_t want_first = 0;
    if (last_keyframes != 0 && n_rec > (uint32_t)last_keyframes) {
        want_first = seg[n_rec - (uint32_t)last_keyframes].first;
        if (want_first > total) want_first = total;
    }
    uint32_t got[2] = {77u, 77u};
    if (vors_map_icp_window_host(n_rec ? seg.data() : nullptr, n_segments, max_keyframes, count, capacity, last_keyframes, got) != VORS_OK) return false;
    return got[0] == want_first && got[1] == total - want_first;
}

int main() {
    // the window
    for (uint32_t n_segments : {0u, 1u, 2u, 5u, 9u})
        for (int max_keyframes : {1, 4, 16})
            for (uint32_t per : {0u, 1u, 100u})
                for (int capacity : {1, 250, 100000}) {
                    const int n_rec = (int)(n_segments < (uint32_t)max_keyframes ? n_segments : (uint32_t)max_keyframes);
                    for (int last : {0, 1, 2, n_rec, n_rec + 1, 1 << 30}) CHECK(window_case(n_segments, max_keyframes, per, capacity, last));
                }
    uint32_t r2[2];
    CHECK(vors_map_icp_window_host(nullptr, 0, 4, 0, 10, 0, nullptr) == VORS_ERR_INVALID_ARGUMENT);
    CHECK(vors_map_icp_window_host(nullptr, 0, 4, 0, 0, 0, r2) == VORS_ERR_INVALID_ARGUMENT);
    CHECK(vors_map_icp_window_host(nullptr, 0, 0, 0, 10, 0, r2) == VORS_ERR_INVALID_ARGUMENT);
    CHECK(vors_map_icp_window_host(nullptr, 0, 4, 0, 10, -1, r2) == VORS_ERR_INVALID_ARGUMENT);
    CHECK(vors_map_icp_window_host(nullptr, 3, 4, 30, 10, 1, r2) == VORS_ERR_INVALID_ARGUMENT);
    CHECK(vors_map_icp_window_host(nullptr, 3, 4, 30, 10, 0, r2) == VORS_OK && r2[0] == 0 && r2[1] == 10);

    // the verdict
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    vors_map_icp_params p{};
    p.min_match_ratio = 0.5f;
    p.max_rms = 0.01f;
    p.max_trans_m = 0.02f;
    p.max_rot_rad = 0.1f;
    const float before[7] = {0.1f, -0.2f, 0.3f, 0.f, 0.f, 0.f, 1.f};
    vors_icp_stats ok{VORS_ICP_CONVERGED, 3u, 1000u, 500u, 0.01f, 0.f};  // equality on the ratio and on the rms
    auto verdict = [&](const vors_map_icp_params& q, const vors_icp_stats& s, const float* a) {
        uint32_t v = 99u;
        return vors_map_icp_verdict_host(&q, &s, before, a, &v) == VORS_OK ? (int)v : -1;
    };
    float after[7];
    std::memcpy(after, before, sizeof(after));
    CHECK(verdict(p, ok, after) == VORS_MAP_ICP_ACCEPTED);
    after[0] = before[0] + 0.02f;  // (0.1f + 0.02f) - 0.1f rounds; the bound is tested in test_map_icp_host.py on exact values
    CHECK(verdict(p, ok, after) == VORS_MAP_ICP_ACCEPTED || verdict(p, ok, after) == VORS_MAP_ICP_STEP);
    after[0] = before[0] + 0.05f;
    CHECK(verdict(p, ok, after) == VORS_MAP_ICP_STEP);
    for (int i = 0; i < 7; ++i)
        for (float bad : {nan, inf, -inf}) {
            std::memcpy(after, before, sizeof(after));
            after[i] = bad;
            vors_icp_stats worst{VORS_ICP_SINGULAR, 0u, 1000u, 0u, nan, nan};
            CHECK(verdict(p, worst, after) == VORS_MAP_ICP_NONFINITE);
        }
    std::memcpy(after, before, sizeof(after));
    for (uint32_t status : {(uint32_t)VORS_ICP_TOO_FEW, (uint32_t)VORS_ICP_SINGULAR, 17u}) {
        vors_icp_stats s{status, 0u, 1000u, 0u, nan, 0.f};
        CHECK(verdict(p, s, after) == VORS_MAP_ICP_ICP_STATUS);
    }
    {
        vors_icp_stats s = ok;
        s.matched = 499u;
        s.rms = nan;
        CHECK(verdict(p, s, after) == VORS_MAP_ICP_FEW_MATCHES);
        s.matched = 500u;
        CHECK(verdict(p, s, after) == VORS_MAP_ICP_RMS);
        s.rms = 0.0100001f;
        CHECK(verdict(p, s, after) == VORS_MAP_ICP_RMS);
        s.status = VORS_ICP_ITERATIONS;
        s.rms = 0.0f;
        s.considered = 0u;
        s.matched = 0u;
        CHECK(verdict(p, s, after) == VORS_MAP_ICP_ACCEPTED);
    }
    {  // the rotation test: a quarter turn about z
        float turned[7];
        std::memcpy(turned, before, sizeof(turned));
        turned[5] = std::sqrt(0.5f);
        turned[6] = std::sqrt(0.5f);
        vors_map_icp_params q = p;
        q.max_rot_rad = 0.0f;
        CHECK(verdict(q, ok, turned) == VORS_MAP_ICP_STEP);
        CHECK(verdict(q, ok, before) == VORS_MAP_ICP_ACCEPTED);
        q.max_rot_rad = 3.14159265358979323846f;
        CHECK(verdict(q, ok, turned) == VORS_MAP_ICP_ACCEPTED);
        turned[5] = -turned[5];
        turned[6] = -turned[6];  // the same rotation, the other sign of the quaternion
        q.max_rot_rad = 1.6f;
        CHECK(verdict(q, ok, turned) == VORS_MAP_ICP_ACCEPTED);
        q.max_rot_rad = 1.5f;
        CHECK(verdict(q, ok, turned) == VORS_MAP_ICP_STEP);
    }
    for (int field = 0; field < 4; ++field)
        for (float bad : {nan, -1.0f}) {
            vors_map_icp_params q = p;
            (field == 0 ? q.min_match_ratio : field == 1 ? q.max_rms : field == 2 ? q.max_trans_m : q.max_rot_rad) = bad;
            CHECK(verdict(q, ok, before) == -1);
        }
    {
        vors_map_icp_params q = p;
        q.min_match_ratio = 1.5f;
        CHECK(verdict(q, ok, before) == -1);
        uint32_t v;
        CHECK(vors_map_icp_verdict_host(nullptr, &ok, before, before, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_host(&p, nullptr, before, before, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_host(&p, &ok, nullptr, before, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_host(&p, &ok, before, nullptr, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_host(&p, &ok, before, before, nullptr) == VORS_ERR_INVALID_ARGUMENT);
    }
    std::printf("map_icp_host_check: ok\n");
    return 0;
}
