// Stand-alone check of vors_icp_condition_from_sums and vors_map_icp_verdict_joint_host for a sanitizer build of the host code (`make
// map_icp_joint_host_check`: operators.cpp and this file with -fsanitize=address,undefined; no GPU is used). Every sums record is a heap
// block of exactly 29 floats, so a read past slot 28 is an error here. Condition: a diagonal H against the closed form, and hostile
// sums — zeros, NaN in every slot, a negative diagonal, counts 6 and 7, denormals, infinities — for their flags and for NaN outputs
// exactly when a flag is set. Verdict: both bounds off against vors_map_icp_verdict_host, equality on a bound, NaN dilutions, the
// priority of the existing failures, and the refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vors_hip.h"

#define CHECK(x)                                                                    \
    do {                                                                            \
        if (!(x)) {                                                                 \
            std::printf("map_icp_joint_host_check: %s failed (line %d)\n", #x, __LINE__); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

// slot of H[r][c], r <= c, in sums29 (the upper triangle row-wise from slot 8)
static int slot(int r, int c) {
    int k = 8;
    for (int i = 0; i < r; ++i) k += 6 - i;
    return k + (c - r);
}
static std::vector<float> diagonal(float count, const float d[6]) {
    std::vector<float> s(29, 0.0f);  // exactly 29
    s[1] = count;
    for (int i = 0; i < 6; ++i) s[(size_t)slot(i, i)] = d[i];
    return s;
}
struct Cond {
    float t, r;
    int32_t flags;
    bool ok;
};
static Cond condition(const std::vector<float>& s) {
    Cond c{-1.0f, -1.0f, -1, false};
    c.ok = vors_icp_condition_from_sums(s.data(), &c.t, &c.r, &c.flags) == VORS_OK;
    return c;
}
static bool nan_iff_flagged(const Cond& c) {
    const bool nans = std::isnan(c.t) && std::isnan(c.r);
    return c.ok && (c.flags != 0 ? nans : (std::isfinite(c.t) && std::isfinite(c.r)));
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float denorm = std::numeric_limits<float>::denorm_min();
    CHECK(slot(0, 0) == 8 && slot(5, 5) == 28 && slot(0, 5) == 13 && slot(1, 1) == 14);
    CHECK(sizeof(vors_map_icp_joint_record) == 20 && sizeof(vors_map_icp_joint_params) == sizeof(vors_map_icp_params) + 16);

    // a diagonal H: C = diag(1 / d), dilution_t = sqrt(n (1/d0 + 1/d1 + 1/d2)), every step exact in f64 for these powers of two
    {
        const float d[6] = {4.0f, 4.0f, 2.0f, 16.0f, 16.0f, 8.0f};
        const Cond c = condition(diagonal(16.0f, d));
        CHECK(c.ok && c.flags == 0 && c.t == 4.0f && c.r == 2.0f);
        float only_t = -1.0f;
        CHECK(vors_icp_condition_from_sums(diagonal(16.0f, d).data(), &only_t, nullptr, nullptr) == VORS_OK && only_t == 4.0f);
        CHECK(vors_icp_condition_from_sums(diagonal(16.0f, d).data(), nullptr, nullptr, nullptr) == VORS_OK);
        CHECK(vors_icp_condition_from_sums(nullptr, &only_t, nullptr, nullptr) == VORS_ERR_INVALID_ARGUMENT);
    }
    // the count: 6 is too few, 7 is enough; NaN, zero and negative counts are too few
    {
        const float d[6] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f};
        CHECK(condition(diagonal(6.0f, d)).flags == 1 && nan_iff_flagged(condition(diagonal(6.0f, d))));
        CHECK(condition(diagonal(7.0f, d)).flags == 0 && nan_iff_flagged(condition(diagonal(7.0f, d))));
        for (float bad : {nan, 0.0f, -5.0f, -inf}) CHECK(condition(diagonal(bad, d)).flags == 1 && nan_iff_flagged(condition(diagonal(bad, d))));
    }
    // zeros: no pivot; with a count of zero both flags
    {
        std::vector<float> z(29, 0.0f);
        CHECK(condition(z).flags == 3 && nan_iff_flagged(condition(z)));
        z[1] = 100.0f;
        CHECK(condition(z).flags == 2 && nan_iff_flagged(condition(z)));
    }
    // a negative or zero diagonal entry, anywhere
    for (int i = 0; i < 6; ++i)
        for (float bad : {-1.0f, 0.0f, -0.0f, nan, -inf}) {
            float d[6] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f};
            d[i] = bad;
            const Cond c = condition(diagonal(50.0f, d));
            CHECK(c.flags == 2 && nan_iff_flagged(c));
        }
    // NaN and infinities in every slot: no crash, and NaN outputs exactly when flagged (slots 0, 2..7 are not read)
    for (int q = 0; q < 29; ++q)
        for (float bad : {nan, inf, -inf}) {
            const float d[6] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f};
            std::vector<float> s = diagonal(50.0f, d);
            s[(size_t)q] = bad;
            const Cond c = condition(s);
            CHECK(c.ok);
            if (q == 0 || (q >= 2 && q <= 7)) CHECK(c.flags == 0 && std::isfinite(c.t) && std::isfinite(c.r));
            if (q >= 8 && std::isnan(bad)) CHECK(c.flags == 2 && nan_iff_flagged(c));
            if (c.flags != 0) CHECK(std::isnan(c.t) && std::isnan(c.r));
        }
    // denormals: a positive denormal diagonal has a factor in f64; the dilutions are then huge or infinite, never NaN, flags 0
    {
        const float d[6] = {denorm, denorm, denorm, denorm, denorm, denorm};
        const Cond c = condition(diagonal(7.0f, d));
        CHECK(c.ok && c.flags == 0 && !std::isnan(c.t) && !std::isnan(c.r) && c.t > 1e18f && c.r > 1e18f);
        std::vector<float> s = diagonal(7.0f, d);
        for (int q = 8; q < 29; ++q) s[(size_t)q] = 2.0f * denorm;  // every entry 2^-148 (an exact root): rank one, the second pivot is 0
        CHECK(condition(s).flags == 2 && nan_iff_flagged(condition(s)));
    }
    // a rank-deficient H built from five rows: one direction free
    {
        std::vector<float> s(29, 0.0f);
        s[1] = 500.0f;
        const float rows[5][6] = {{1, 0, 0, 0, 0, 0}, {0, 1, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0}, {0, 0, 0, 1, 0, 0}, {0, 0, 0, 0, 1, 0}};
        for (const auto& j : rows)
            for (int r = 0; r < 6; ++r)
                for (int c = r; c < 6; ++c) s[(size_t)slot(r, c)] += j[r] * j[c];
        CHECK(condition(s).flags == 2 && nan_iff_flagged(condition(s)));
    }

    // the verdict
    vors_map_icp_joint_params p{};
    p.icp.min_match_ratio = 0.5f;
    p.icp.max_rms = 0.01f;
    p.icp.max_trans_m = 0.02f;
    p.icp.max_rot_rad = 0.1f;
    const float before[7] = {0.1f, -0.2f, 0.3f, 0.f, 0.f, 0.f, 1.f};
    float far[7], broken[7];
    std::memcpy(far, before, sizeof(far));
    std::memcpy(broken, before, sizeof(broken));
    far[0] += 0.05f;
    broken[3] = nan;
    const vors_icp_stats ok{VORS_ICP_CONVERGED, 3u, 1000u, 500u, 0.01f, 0.f};
    const vors_icp_stats few{VORS_ICP_CONVERGED, 3u, 1000u, 499u, 0.01f, 0.f};
    const vors_icp_stats loud{VORS_ICP_CONVERGED, 3u, 1000u, 500u, 0.02f, 0.f};
    const vors_icp_stats singular{VORS_ICP_SINGULAR, 0u, 1000u, 0u, nan, nan};
    auto verdict = [&](const vors_map_icp_joint_params& q, const vors_icp_stats& s, const float* a, float dt, float dr) {
        uint32_t v = 99u;
        return vors_map_icp_verdict_joint_host(&q, &s, before, a, dt, dr, &v) == VORS_OK ? (int)v : -1;
    };
    auto plain = [&](const vors_icp_stats& s, const float* a) {
        uint32_t v = 99u;
        return vors_map_icp_verdict_host(&p.icp, &s, before, a, &v) == VORS_OK ? (int)v : -1;
    };
    struct Row {
        const vors_icp_stats* s;
        const float* after;
        int want;
    };
    const Row table[] = {{&ok, before, VORS_MAP_ICP_ACCEPTED}, {&ok, broken, VORS_MAP_ICP_NONFINITE}, {&singular, before, VORS_MAP_ICP_ICP_STATUS},
                         {&few, before, VORS_MAP_ICP_FEW_MATCHES}, {&loud, before, VORS_MAP_ICP_RMS}, {&ok, far, VORS_MAP_ICP_STEP}};
    for (const Row& r : table) {
        CHECK(plain(*r.s, r.after) == r.want);
        for (float dt : {0.0f, 1.0f, 1e30f, inf, nan})  // both bounds off: the plain verdict whatever the dilutions
            CHECK(verdict(p, *r.s, r.after, dt, nan) == r.want && verdict(p, *r.s, r.after, nan, dt) == r.want);
        vors_map_icp_joint_params q = p;  // both bounds on and failing: an existing failure keeps its name
        q.max_dilution_t = 1.0f;
        q.max_dilution_r = 1.0f;
        CHECK(verdict(q, *r.s, r.after, 50.0f, 50.0f) == (r.want == VORS_MAP_ICP_ACCEPTED ? VORS_MAP_ICP_CONDITION : r.want));
        CHECK(verdict(q, *r.s, r.after, nan, nan) == (r.want == VORS_MAP_ICP_ACCEPTED ? VORS_MAP_ICP_CONDITION : r.want));
        CHECK(verdict(q, *r.s, r.after, 1.0f, 1.0f) == r.want);  // equality on both bounds holds
    }
    {
        vors_map_icp_joint_params q = p;
        q.max_dilution_t = 20.0f;
        CHECK(verdict(q, ok, before, 20.0f, nan) == VORS_MAP_ICP_ACCEPTED);  // only the translation bound is on
        CHECK(verdict(q, ok, before, 20.000002f, 1.0f) == VORS_MAP_ICP_CONDITION);
        CHECK(verdict(q, ok, before, nan, 1.0f) == VORS_MAP_ICP_CONDITION);
        CHECK(verdict(q, ok, before, inf, 1.0f) == VORS_MAP_ICP_CONDITION);
        q.max_dilution_t = 0.0f;
        q.max_dilution_r = 5.0f;
        CHECK(verdict(q, ok, before, nan, 5.0f) == VORS_MAP_ICP_ACCEPTED);  // only the rotation bound is on
        CHECK(verdict(q, ok, before, 1.0f, 5.5f) == VORS_MAP_ICP_CONDITION);
        CHECK(verdict(q, ok, before, 1.0f, nan) == VORS_MAP_ICP_CONDITION);
        q.max_dilution_r = inf;  // a bound of infinity passes everything but NaN
        CHECK(verdict(q, ok, before, 1.0f, inf) == VORS_MAP_ICP_ACCEPTED && verdict(q, ok, before, 1.0f, nan) == VORS_MAP_ICP_CONDITION);
    }
    // condition and verdict together: a system without a factor fails a bound that is on and passes when both are off
    {
        std::vector<float> z(29, 0.0f);
        z[1] = 100.0f;
        const Cond c = condition(z);
        vors_map_icp_joint_params q = p;
        CHECK(verdict(q, ok, before, c.t, c.r) == VORS_MAP_ICP_ACCEPTED);
        q.max_dilution_t = 1e30f;
        CHECK(verdict(q, ok, before, c.t, c.r) == VORS_MAP_ICP_CONDITION);
    }
    for (int field = 0; field < 6; ++field)
        for (float bad : {nan, -1.0f}) {
            vors_map_icp_joint_params q = p;
            (field == 0 ? q.icp.min_match_ratio : field == 1 ? q.icp.max_rms : field == 2 ? q.icp.max_trans_m : field == 3 ? q.icp.max_rot_rad
             : field == 4 ? q.max_dilution_t : q.max_dilution_r) = bad;
            CHECK(verdict(q, ok, before, 1.0f, 1.0f) == -1);
        }
    {
        uint32_t v;
        CHECK(vors_map_icp_verdict_joint_host(nullptr, &ok, before, before, 1.f, 1.f, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_joint_host(&p, nullptr, before, before, 1.f, 1.f, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_joint_host(&p, &ok, nullptr, before, 1.f, 1.f, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_joint_host(&p, &ok, before, nullptr, 1.f, 1.f, &v) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(vors_map_icp_verdict_joint_host(&p, &ok, before, before, 1.f, 1.f, nullptr) == VORS_ERR_INVALID_ARGUMENT);
    }
    std::printf("map_icp_joint_host_check: ok\n");
    return 0;
}
