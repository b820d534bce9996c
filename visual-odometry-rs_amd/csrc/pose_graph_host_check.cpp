// Stand-alone check of vors_pose_graph_optimize_host and vors_pose_graph_jacobians_host for a sanitizer build of the host code (`make
// pose_graph_host_check`: operators.cpp and this file with -fsanitize=address,undefined; no GPU is used). Every array is a heap block of
// exactly its size, so a read or write past a graph's arrays is an error here. Graphs: a ring with chords, a chain with a closing edge, a
// star whose hub has 200 edges, the ring with skipped edges of every kind appended (NaN measurement, zero weight, i == j, an index out of
// range, an infinite information entry), a graph with isolated nodes, an empty graph, counts above the capacities, and the refusals.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/vors_hip.h"

#define CHECK(x)                                                                     \
    do {                                                                             \
        if (!(x)) {                                                                  \
            std::printf("pose_graph_host_check: %s failed (line %d)\n", #x, __LINE__); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

struct Graph {
    std::vector<float> truth, poses, meas, info, weight;
    std::vector<uint32_t> edges;
    size_t nodes() const { return poses.size() / 7; }
    size_t edge_count() const { return edges.size() / 2; }
};

static uint32_t g_seed = 12345u;
static float unit() {  // in [-1, 1)
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)(g_seed >> 8) / 8388608.0f - 1.0f;
}
static void random_pose(float trans, float rot, float out[7]) {
    const float xi[6] = {trans * unit(), trans * unit(), trans * unit(), rot * unit() * 0.5f, rot * unit() * 0.5f, rot * unit() * 0.5f};
    vors_se3_exp(xi, out);
}

// poses from the truth (node 0 exact, the others up to 5 cm / 0.05 rad off) and exact measurements M_ij = T_j^-1 T_i
static void finish(Graph& g) {
    const size_t n = g.truth.size() / 7;
    g.poses = g.truth;
    for (size_t k = 1; k < n; ++k) {
        float d[7];
        random_pose(0.05f, 0.05f, d);
        vors_iso_mul(&g.truth[k * 7], d, &g.poses[k * 7]);
    }
    g.meas.resize(g.edge_count() * 7);
    for (size_t e = 0; e < g.edge_count(); ++e) {
        float inv[7];
        vors_iso_inverse(&g.truth[g.edges[2 * e + 1] * 7], inv);
        vors_iso_mul(inv, &g.truth[g.edges[2 * e] * 7], &g.meas[e * 7]);
    }
}
static Graph random_nodes(size_t n) {
    Graph g;
    g.truth.resize(n * 7);
    const float id[7] = {0, 0, 0, 0, 0, 0, 1};
    std::memcpy(g.truth.data(), id, sizeof id);
    for (size_t k = 1; k < n; ++k) random_pose(1.0f, 1.0f, &g.truth[k * 7]);
    return g;
}
static Graph ring(uint32_t n, uint32_t chords) {
    Graph g = random_nodes(n);
    for (uint32_t k = 0; k < n; ++k) g.edges.insert(g.edges.end(), {k, (k + 1) % n});
    for (uint32_t k = 0; k < chords; ++k) g.edges.insert(g.edges.end(), {k * (n / chords), (k * (n / chords) + n / 2 + 1) % n});
    finish(g);
    return g;
}
static Graph chain(uint32_t n) {
    Graph g = random_nodes(n);
    for (uint32_t k = 0; k + 1 < n; ++k) g.edges.insert(g.edges.end(), {k, k + 1});
    g.edges.insert(g.edges.end(), {n - 1, 0u});
    finish(g);
    return g;
}
static Graph star(uint32_t degree) {
    Graph g = random_nodes(degree + 1);
    g.edges.insert(g.edges.end(), {1u, 0u});
    for (uint32_t k = 2; k <= degree; ++k) g.edges.insert(g.edges.end(), {k % 2 ? 1u : k, k % 2 ? k : 1u});
    for (uint32_t k = 2; k <= degree; k += 4) g.edges.insert(g.edges.end(), {0u, k});
    finish(g);
    return g;
}

struct Result {
    std::vector<float> poses, residuals, energy;
    vors_pose_graph_stats stats;
    vors_status st;
};
static Result run(const Graph& g, uint32_t node_count, uint32_t edge_count, int iters) {
    Result r;
    r.poses.assign(g.poses.size(), 7.5f);
    r.residuals.assign(g.edge_count() * 6, 7.5f);
    r.energy.assign(g.edge_count(), 7.5f);
    std::memset(&r.stats, 0xA5, sizeof r.stats);
    r.st = vors_pose_graph_optimize_host(g.poses.data(), node_count, (int)g.nodes(), g.edges.data(), edge_count, (int)g.edge_count(), g.meas.data(),
                                         g.info.empty() ? nullptr : g.info.data(), g.weight.empty() ? nullptr : g.weight.data(), nullptr, 1e-4f,
                                         1e-6f, 1e-6f, iters, 64, r.poses.data(), &r.stats, r.residuals.data(), r.energy.data());
    return r;
}
static float worst_translation(const Result& r, const Graph& g) {
    float worst = 0.0f;
    for (size_t k = 0; k < g.nodes(); ++k)
        for (int a = 0; a < 3; ++a) worst = std::fmax(worst, std::fabs(r.poses[k * 7 + a] - g.truth[k * 7 + a]));
    return worst;
}

int main() {
    // the three consistent graphs return to the truth
    const Graph graphs[3] = {ring(24, 6), chain(40), star(200)};
    for (const Graph& g : graphs) {
        const Result r = run(g, (uint32_t)g.nodes(), (uint32_t)g.edge_count(), 16);
        CHECK(r.st == VORS_OK && r.stats.status == VORS_PG_CONVERGED);
        CHECK(r.stats.valid_edges == g.edge_count() && r.stats.skipped_edges == 0 && r.stats.free_nodes == g.nodes() - 1);
        CHECK(worst_translation(r, g) < 1e-4f);
        CHECK(std::memcmp(r.poses.data(), g.poses.data(), 28) == 0);
        CHECK(r.stats.final_energy <= r.stats.initial_energy);
    }
    // the evaluator keeps the poses; counts above the capacities are clipped to them
    {
        const Graph& g = graphs[0];
        const Result r = run(g, 1000u, 100000u, 0);
        CHECK(r.st == VORS_OK && std::memcmp(r.poses.data(), g.poses.data(), g.poses.size() * 4) == 0);
        CHECK(r.stats.valid_edges == g.edge_count() && r.stats.initial_energy == r.stats.final_energy);
    }
    // skipped edges of every kind change nothing else
    {
        Graph g = graphs[0];
        const size_t e0 = g.edge_count();
        g.info.assign(e0 * 36, 0.0f);
        for (size_t e = 0; e < e0; ++e)
            for (int d = 0; d < 6; ++d) g.info[e * 36 + d * 7] = 1.0f + 0.1f * (float)d;
        g.weight.assign(e0, 1.0f);
        const Result base = run(g, (uint32_t)g.nodes(), (uint32_t)e0, 4);
        const uint32_t bad[5][2] = {{2, 5}, {2, 5}, {4, 4}, {2, 99}, {2, 5}};
        for (int k = 0; k < 5; ++k) {
            g.edges.insert(g.edges.end(), {bad[k][0], bad[k][1]});
            g.meas.insert(g.meas.end(), g.meas.begin(), g.meas.begin() + 7);
            g.info.insert(g.info.end(), g.info.begin(), g.info.begin() + 36);
            g.weight.push_back(k == 1 ? 0.0f : 1.0f);
        }
        g.meas[e0 * 7 + 4] = std::numeric_limits<float>::quiet_NaN();
        g.info[(e0 + 4) * 36 + 7] = std::numeric_limits<float>::infinity();
        const Result r = run(g, (uint32_t)g.nodes(), (uint32_t)g.edge_count(), 4);
        CHECK(r.st == VORS_OK && r.stats.skipped_edges == 5 && r.stats.valid_edges == e0);
        CHECK(std::memcmp(r.poses.data(), base.poses.data(), r.poses.size() * 4) == 0);
        CHECK(std::memcmp(r.residuals.data(), base.residuals.data(), e0 * 24) == 0 && std::memcmp(r.energy.data(), base.energy.data(), e0 * 4) == 0);
        for (size_t e = e0; e < g.edge_count(); ++e) CHECK(std::isnan(r.energy[e]) && std::isnan(r.residuals[e * 6 + 5]));
        CHECK(r.stats.final_energy == base.stats.final_energy && r.stats.cg_iterations == base.stats.cg_iterations);
    }
    // isolated nodes are counted and kept; an empty graph and a graph without a free node are TOO_FEW
    {
        Graph g = graphs[1];
        for (int k = 0; k < 14; ++k) g.poses.push_back(g.poses[7 + k]);
        g.truth.insert(g.truth.end(), g.poses.end() - 14, g.poses.end());
        const Result r = run(g, (uint32_t)g.nodes(), (uint32_t)g.edge_count(), 16);
        CHECK(r.st == VORS_OK && r.stats.isolated_nodes == 2 && r.stats.status == VORS_PG_CONVERGED);
        CHECK(std::memcmp(&r.poses[r.poses.size() - 14], &g.poses[g.poses.size() - 14], 56) == 0);
        const Result none = run(g, (uint32_t)g.nodes(), 0u, 16);
        CHECK(none.st == VORS_OK && none.stats.status == VORS_PG_TOO_FEW && none.stats.valid_edges == 0 && none.stats.final_energy == 0.0f);
        CHECK(std::memcmp(none.poses.data(), g.poses.data(), g.poses.size() * 4) == 0);
        CHECK(none.energy[0] == 7.5f && none.residuals[0] == 7.5f);  // no edge below the count: nothing written
        const Result one = run(g, 1u, (uint32_t)g.edge_count(), 16);  // every edge refers to a node beyond the count
        CHECK(one.st == VORS_OK && one.stats.status == VORS_PG_TOO_FEW && one.stats.skipped_edges == g.edge_count() && one.poses[7] == 7.5f);
    }
    // the closed-form Jacobians: finite, and J_i = -Ad(E^-1)-shaped (its translational block is minus the identity)
    {
        float r6[6], ji[36], jj[36];
        vors_pose_graph_jacobians_host(&graphs[0].poses[7], &graphs[0].poses[14], &graphs[0].meas[7], r6, ji, jj);
        for (int k = 0; k < 36; ++k) CHECK(std::isfinite(ji[k]) && std::isfinite(jj[k]));
        for (int k = 0; k < 3; ++k) CHECK(std::fabs(ji[k * 6 + k] + 1.0f) < 1e-5f);
    }
    // the refusals write nothing
    {
        const Graph& g = graphs[0];
        float out[7 * 24];
        for (float& v : out) v = 7.5f;
        const int n = (int)g.nodes(), e = (int)g.edge_count();
        const float nan = std::numeric_limits<float>::quiet_NaN();
        auto call = [&](const float* poses, int ncap, int ecap, float lambda0, float step_eps, float cg_tol, int iters, int cg_iters, float* o) {
            return vors_pose_graph_optimize_host(poses, (uint32_t)n, ncap, g.edges.data(), (uint32_t)e, ecap, g.meas.data(), nullptr, nullptr, nullptr,
                                                 lambda0, step_eps, cg_tol, iters, cg_iters, o, nullptr, nullptr, nullptr);
        };
        CHECK(call(nullptr, n, e, 1e-4f, 1e-6f, 1e-6f, 4, 16, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), 0, e, 1e-4f, 1e-6f, 1e-6f, 4, 16, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, 0, 1e-4f, 1e-6f, 1e-6f, 4, 16, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, e, nan, 1e-6f, 1e-6f, 4, 16, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, e, 1e-4f, -1.0f, 1e-6f, 4, 16, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, e, 1e-4f, 1e-6f, nan, 4, 16, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, e, 1e-4f, 1e-6f, 1e-6f, 65, 16, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, e, 1e-4f, 1e-6f, 1e-6f, 4, 0, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, e, 1e-4f, 1e-6f, 1e-6f, 4, 257, out) == VORS_ERR_INVALID_ARGUMENT);
        CHECK(call(g.poses.data(), n, e, 1e-4f, 1e-6f, 1e-6f, 4, 16, nullptr) == VORS_ERR_INVALID_ARGUMENT);
        for (float v : out) CHECK(v == 7.5f);
    }
    std::printf("pose_graph_host_check: ok\n");
    return 0;
}
