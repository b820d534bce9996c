// Stand-alone check of vors_loop_signatures_host, vors_loop_candidates_host and vors_loop_verify_edges_host for a sanitizer build of the
// host code (`make loop_closure_host_check`: operators.cpp and this file with -fsanitize=address,undefined; no GPU is used). Every array
// is a heap block of exactly its size, so a read or write past it is an error here. Signatures: uneven cells, one pixel per cell, the
// largest D. Candidates: a count below the capacity, a flat and a negated signature, both halves of the pose gate, k beyond the
// survivors, a query window. Verification: every verdict code, strided models, a full edge list. And the refusals, which write nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vors_hip.h"

#define CHECK(x)                                                                        \
    do {                                                                                \
        if (!(x)) {                                                                     \
            std::printf("loop_closure_host_check: %s failed (line %d)\n", #x, __LINE__); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

static uint32_t g_seed = 2024u;
static uint32_t next() {
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

static int signature_of(const std::vector<uint8_t>& plane, int rows, int cols, int tr, int tc, std::vector<int8_t>& sig, vors_loop_sig_meta& meta) {
    sig.assign((size_t)tr * tc, 77);
    return vors_loop_signatures_host(plane.data(), rows, cols, tr, tc, sig.data(), &meta);
}

int main() {
    // ---- signatures
    {
        const int shapes[4][4] = {{60, 80, 8, 8}, {61, 83, 12, 16}, {64, 64, 32, 32}, {8, 8, 8, 8}};
        for (const auto& s : shapes) {
            std::vector<uint8_t> plane((size_t)s[0] * s[1]);
            for (uint8_t& p : plane) p = (uint8_t)next();
            std::vector<int8_t> sig;
            vors_loop_sig_meta meta{};
            CHECK(signature_of(plane, s[0], s[1], s[2], s[3], sig, meta) == VORS_OK);
            int64_t sum = 0, sumsq = 0;
            for (int8_t v : sig) {
                sum += v;
                sumsq += (int64_t)v * v;
            }
            CHECK(meta.sum == sum && meta.sumsq == sumsq);
            if (s[0] == 8) {
                for (size_t k = 0; k < plane.size(); ++k) CHECK((int)sig[k] == (int)plane[k] - 128);
            }
            std::fill(plane.begin(), plane.end(), (uint8_t)255);
            CHECK(signature_of(plane, s[0], s[1], s[2], s[3], sig, meta) == VORS_OK && sig[0] == 127 && sig.back() == 127);
        }
        std::vector<uint8_t> plane(64 * 64, 9);
        std::vector<int8_t> sig;
        vors_loop_sig_meta meta{-5, 5u};
        CHECK(signature_of(plane, 64, 64, 8, 7, sig, meta) == VORS_ERR_INVALID_ARGUMENT);   // D = 56
        CHECK(signature_of(plane, 64, 64, 64, 32, sig, meta) == VORS_ERR_INVALID_ARGUMENT);  // D = 2048
        CHECK(signature_of(plane, 4, 64, 8, 8, sig, meta) == VORS_ERR_INVALID_ARGUMENT);     // rows < tr
        CHECK(vors_loop_signatures_host(nullptr, 64, 64, 8, 8, sig.data(), &meta) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(meta.sum == -5 && meta.sumsq == 5u && sig[0] == 77);
    }
    // ---- candidates: 40 random signatures of D = 128 in a capacity of 48, number 5 flat, number 9 the negative of number 2
    {
        const int D = 128, cap = 48, k = 4;
        const uint32_t count = 40;
        std::vector<int8_t> sig((size_t)cap * D);
        std::vector<vors_loop_sig_meta> meta(cap);
        for (int r = 0; r < cap; ++r) {
            int32_t sum = 0;
            uint32_t sumsq = 0;
            for (int c = 0; c < D; ++c) {
                int v = (int)(next() % 255u) - 127;
                if (r == 5) v = 3;
                if (r == 9) v = -sig[(size_t)2 * D + c];
                sig[(size_t)r * D + c] = (int8_t)v;
                sum += v;
                sumsq += (uint32_t)(v * v);
            }
            meta[r] = vors_loop_sig_meta{sum, sumsq};
        }
        std::vector<float> poses((size_t)cap * 7, 0.0f);
        for (int r = 0; r < cap; ++r) {
            poses[(size_t)r * 7] = 0.1f * (float)r;
            poses[(size_t)r * 7 + 6] = 1.0f;
        }
        poses[7 * 7 + 1] = std::numeric_limits<float>::quiet_NaN();
        auto run = [&](const float* p, uint32_t first, uint32_t gap, int kk, float min_score, float dist, float qdot, std::vector<vors_loop_candidate>& cand,
                       std::vector<uint32_t>& cc, uint32_t counts[VORS_LOOP_COUNTS]) {
            cand.assign((size_t)cap * kk, vors_loop_candidate{123u, 7.5f});
            cc.assign(cap, 99u);
            return vors_loop_candidates_host(sig.data(), meta.data(), count, cap, D, p, first, gap, kk, min_score, dist, qdot, cand.data(), cc.data(), counts);
        };
        std::vector<vors_loop_candidate> cand;
        std::vector<uint32_t> cc;
        uint32_t counts[VORS_LOOP_COUNTS];
        CHECK(run(nullptr, 0, 1, k, -2.0f, 0.0f, 0.0f, cand, cc, counts) == VORS_OK);
        CHECK(counts[0] == count * (count - 1) / 2 && counts[1] + counts[2] + counts[3] + counts[4] == counts[0]);
        CHECK(counts[1] == count - 1 && counts[2] == 0 && counts[3] == 0);  // the flat one meets every other once
        CHECK(cc[0] == 0 && cand[0].i == 0xFFFFFFFFu && cc[1] == 1 && cc[39] == (uint32_t)k && cc[40] == 99u && cand[(size_t)40 * k].i == 123u);
        for (uint32_t j = 0; j < count; ++j)
            for (uint32_t p = 0; p + 1 < cc[j]; ++p) {
                const vors_loop_candidate &a = cand[(size_t)j * k + p], &b = cand[(size_t)j * k + p + 1];
                CHECK(a.score > b.score || (a.score == b.score && a.i < b.i));
                CHECK(a.i != 5u && b.i != 5u);
            }
        CHECK(run(nullptr, 0, 1, VORS_LOOP_MAX_K, -2.0f, 0.0f, 0.0f, cand, cc, counts) == VORS_OK);  // query 9: 8 survivors, the negative last
        CHECK(cc[9] == 8u && cand[(size_t)9 * 8 + 7].i == 2u && cand[(size_t)9 * 8 + 7].score == -1.0f);
        CHECK(run(nullptr, 0, 1, k, 0.5f, 0.0f, 0.0f, cand, cc, counts) == VORS_OK && counts[3] > 0);
        CHECK(run(poses.data(), 30, 10, VORS_LOOP_MAX_K, -2.0f, 1.05f, 0.5f, cand, cc, counts) == VORS_OK);
        CHECK(cc[29] == 99u && counts[2] > 0 && counts[0] == counts[1] + counts[2] + counts[3] + counts[4]);
        for (uint32_t j = 30; j < count; ++j)
            for (uint32_t p = 0; p < cc[j]; ++p) CHECK(j - cand[(size_t)j * 8 + p].i == 10u && cand[(size_t)j * 8 + p].i != 7u);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        CHECK(run(nullptr, 0, 0, k, 0.0f, 0.0f, 0.0f, cand, cc, counts) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(nullptr, 0, 1, 0, 0.0f, 0.0f, 0.0f, cand, cc, counts) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(nullptr, 0, 1, 9, 0.0f, 0.0f, 0.0f, cand, cc, counts) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(poses.data(), 0, 1, k, 0.0f, nan, 0.0f, cand, cc, counts) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(poses.data(), 0, 1, k, 0.0f, 0.0f, -1.0f, cand, cc, counts) == VORS_ERR_INVALID_ARGUMENT && cc[3] == 99u && cand[5].i == 123u);
    }
    // ---- verification: models inside vors_pair_stats-like records of 12 floats
    {
        const uint32_t m = 10;
        const int stride = 12, ecap = 6;
        const float xi[6] = {0.05f, -0.02f, 0.03f, 0.01f, 0.02f, -0.015f}, big_t[6] = {0.5f, 0, 0, 0, 0, 0}, big_r[6] = {0, 0, 0, 0.3f, 0, 0};
        float motion[7], inverse[7], off_t[7], off_r[7], id[7] = {0, 0, 0, 0, 0, 0, 1};
        vors_se3_exp(xi, motion);
        vors_iso_inverse(motion, inverse);
        vors_se3_exp(big_t, off_t);
        vors_se3_exp(big_r, off_r);
        std::vector<float> fwd((size_t)m * stride, 0.25f), bwd((size_t)m * stride, 0.25f), info((size_t)m * 36, 0.0f), poses(3 * 7);
        std::vector<uint32_t> pairs(2 * m);
        std::vector<int32_t> sf(m, VORS_TRACK_OK), sb(m, VORS_TRACK_OK);
        // poses consistent with `motion` between nodes 0 and 2: T_2 = T_0 M^-1
        std::memcpy(&poses[0], id, 28);
        std::memcpy(&poses[7], id, 28);
        std::memcpy(&poses[14], inverse, 28);
        for (uint32_t e = 0; e < m; ++e) {
            pairs[2 * e] = 0;
            pairs[2 * e + 1] = 2;
            std::memcpy(&fwd[(size_t)e * stride], motion, 28);
            std::memcpy(&bwd[(size_t)e * stride], inverse, 28);
            for (int d = 0; d < 6; ++d) info[(size_t)e * 36 + d * 7] = 2.0f + (float)e;
        }
        sb[1] = VORS_TRACK_OPTIMIZER_FAILED_POSE_KEPT;                       // STATUS
        pairs[2 * 2 + 1] = 3;                                               // INDEX
        info[3 * 36 + 5] = std::numeric_limits<float>::infinity();          // NONFINITE
        vors_iso_mul(off_t, inverse, &bwd[(size_t)4 * stride]);              // CYCLE_TRANS
        vors_iso_mul(off_r, inverse, &bwd[(size_t)5 * stride]);              // CYCLE_ROT
        vors_iso_mul(motion, off_t, &fwd[(size_t)6 * stride]);               // PRIOR_TRANS (with a backward model that is its inverse)
        vors_iso_inverse(&fwd[(size_t)6 * stride], &bwd[(size_t)6 * stride]);
        vors_iso_mul(motion, off_r, &fwd[(size_t)7 * stride]);               // PRIOR_ROT
        vors_iso_inverse(&fwd[(size_t)7 * stride], &bwd[(size_t)7 * stride]);
        std::vector<uint32_t> edges(2 * ecap, 55u), verdict(m, 55u), counts(VORS_LOOP_VERDICTS, 55u);
        std::vector<float> meas((size_t)ecap * 7, 7.5f), info_out((size_t)ecap * 36, 7.5f), weight(ecap, 7.5f), residuals((size_t)m * 12, 7.5f);
        uint32_t edge_count = 4;
        auto run = [&](uint32_t mm, float bound, float w, int cap) {
            return vors_loop_verify_edges_host(mm, pairs.data(), fwd.data(), stride * 4, bwd.data(), stride * 4, sf.data(), sb.data(), info.data(),
                                               poses.data(), 0, 3, bound, bound, bound, bound, w, edges.data(), meas.data(), info_out.data(),
                                               weight.data(), &edge_count, cap, verdict.data(), residuals.data(), counts.data());
        };
        CHECK(run(m, 0.01f, 0.5f, ecap) == VORS_OK);
        const uint32_t want[m] = {VORS_LOOP_ACCEPTED,    VORS_LOOP_STATUS,      VORS_LOOP_INDEX,     VORS_LOOP_NONFINITE, VORS_LOOP_CYCLE_TRANS,
                                  VORS_LOOP_CYCLE_ROT,   VORS_LOOP_PRIOR_TRANS, VORS_LOOP_PRIOR_ROT, VORS_LOOP_ACCEPTED,  VORS_LOOP_CAPACITY};
        for (uint32_t e = 0; e < m; ++e) CHECK(verdict[e] == want[e]);
        CHECK(edge_count == 6 && edges[6] == 55u && edges[8] == 0u && edges[9] == 2u && edges[10] == 0u && weight[3] == 7.5f && weight[4] == 0.5f);
        CHECK(std::memcmp(&meas[4 * 7], motion, 28) == 0 && info_out[4 * 36] == 2.0f && info_out[5 * 36] == 10.0f && info_out[4 * 36 + 1] == 0.0f);
        CHECK(counts[VORS_LOOP_ACCEPTED] == 2 && counts[VORS_LOOP_CAPACITY] == 1 && counts[VORS_LOOP_STATUS] == 1);
        CHECK(std::isnan(residuals[1 * 12]) && std::isnan(residuals[3 * 12 + 11]) && std::fabs(residuals[0]) < 1e-6f && std::fabs(residuals[4 * 12]) > 0.4f);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        verdict.assign(m, 55u);
        CHECK(run(0, 0.01f, 0.5f, ecap) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(m, nan, 0.5f, ecap) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(m, -1.0f, 0.5f, ecap) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(m, 0.01f, 0.0f, ecap) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(run(m, 0.01f, 0.5f, 0) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(edge_count == 6 && verdict[0] == 55u);
    }
    std::printf("loop_closure_host_check: ok\n");
    return 0;
}
