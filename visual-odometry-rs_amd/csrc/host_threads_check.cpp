// Stand-alone check of the header's promises about threads for the entries that need no handle (`make host_threads_check`, and
// `make host_threads_check_tsan`: operators.cpp and this file with -fsanitize=thread on the host side). Eight std::threads call the
// host-arithmetic entries concurrently, each on inputs of its own seed, with refused calls in between:
//   vors_lm_step, vors_icp_points_joint_host, vors_render_points_host, vors_voxel_stats_host then vors_voxel_means_host,
//   vors_depth_normals_host, vors_icp_condition_from_sums; vors_lm_solve for its refusals, which come before anything else of it.
// Every thread writes a log: each status, every output byte, and vors_last_error() after every call — after a refused call the
// refusal's message, after a successful one still the message of the thread's own last refusal (a success leaves it alone). The same
// work is done serially first, thread by thread; a concurrent log must equal its serial twin byte for byte. The threads walk the list of
// refusals from different starting points, so at any moment neighbours hold different messages: a last error that was not per thread
// would show as a foreign message in a log.
// vors_lm_solve itself runs on the device (operators.cpp: it uploads the observation), so a valid call of it is made only without
// --host-only: with a GPU that is eight concurrent solves of one small level, without one eight VORS_ERR_NO_DEVICE refusals; either way
// the concurrent results must equal the serial ones. The sanitizer build is run with --host-only and never opens a device.
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/vors_hip.h"

namespace {

constexpr int N_THREADS = 8, ROUNDS = 12, N_REFUSALS = 7;
constexpr int ROWS = 12, COLS = 16, CAPACITY = 320, VOXEL_CAPACITY = 256;

struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0, generation = 0;
    const int n;
    explicit Barrier(int n_) : n(n_) {}
    void wait() {
        std::unique_lock<std::mutex> lock(m);
        const int g = generation;
        if (++waiting == n) {
            waiting = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lock, [&] { return generation != g; });
        }
    }
};

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x5EEDull) {}
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    float unit() { return (float)(next() & 0xFFFFFF) / 16777216.0f; }  // [0, 1)
};

struct Inputs {
    float cam[5], pose[7];
    std::vector<uint16_t> depth;
    std::vector<uint8_t> frame_gray, list_gray, tmpl, image;
    std::vector<float> frame_normals, xyz, normals, iz, jac;
    std::vector<int32_t> coords;
    float H[36], g[6], sums29[29];
};

Inputs make_inputs(int tid) {
    Rng r((uint64_t)tid + 1);
    Inputs in;
    const float cam[5] = {0.5f * (COLS - 1) + 0.1f * tid, 0.5f * (ROWS - 1), 10.0f + tid, 10.5f, 0.05f};
    std::memcpy(in.cam, cam, sizeof cam);
    const float q[3] = {0.01f + 0.002f * tid, -0.008f, 0.012f};
    const float w = std::sqrt(1.0f - (q[0] * q[0] + q[1] * q[1] + q[2] * q[2]));
    const float pose[7] = {0.01f, -0.02f + 0.003f * tid, 0.015f, q[0], q[1], q[2], w};
    std::memcpy(in.pose, pose, sizeof pose);
    const size_t S = (size_t)ROWS * COLS;
    in.depth.resize(S);
    in.frame_gray.resize(S);
    in.tmpl.resize(S);
    in.image.resize(S);
    in.frame_normals.assign(S * 3, 0.0f);
    for (size_t i = 0; i < S; ++i) {
        in.depth[i] = (r.next() % 9 == 0) ? 0 : (uint16_t)(5000 + r.next() % 150);
        in.frame_gray[i] = (uint8_t)r.next();
        in.tmpl[i] = (uint8_t)(8 * (i % COLS) + 5 * (i / COLS) + r.next() % 3);
        in.image[i] = (uint8_t)(8 * (i % COLS) + 5 * (i / COLS) + r.next() % 3);
        if (r.next() % 5) in.frame_normals[3 * i + 2] = -1.0f;
    }
    in.xyz.resize((size_t)CAPACITY * 3);
    in.normals.assign((size_t)CAPACITY * 3, 0.0f);
    in.list_gray.resize(CAPACITY);
    for (int i = 0; i < CAPACITY; ++i) {  // spread over the plane and a margin around it, near 1 m
        const float z = 1.0f + 0.03f * (r.unit() - 0.5f);
        const float u = -1.0f + (COLS + 1.0f) * r.unit(), v = -1.0f + (ROWS + 1.0f) * r.unit();
        const float py = (v - cam[1]) / cam[3];
        in.xyz[3 * i] = ((u - cam[0]) - cam[4] * py) / cam[2] * z;
        in.xyz[3 * i + 1] = py * z;
        in.xyz[3 * i + 2] = z;
        if (r.next() % 11) in.normals[3 * i + 2] = -1.0f;
        in.list_gray[i] = (uint8_t)r.next();
    }
    const int n_obs = 48;
    for (int i = 0; i < n_obs; ++i) {
        in.coords.push_back(2 + (int)(r.next() % (COLS - 4)));
        in.coords.push_back(2 + (int)(r.next() % (ROWS - 4)));
        in.iz.push_back(0.5f + r.unit());
        for (int k = 0; k < 6; ++k) in.jac.push_back(4.0f * (r.unit() - 0.5f));
    }
    for (int a = 0; a < 6; ++a) {  // a symmetric, diagonally dominant H
        for (int b = 0; b <= a; ++b) in.H[6 * a + b] = in.H[6 * b + a] = (a == b) ? 50.0f + 10.0f * r.unit() : r.unit() - 0.5f;
        in.g[a] = r.unit() - 0.5f;
    }
    in.sums29[0] = 0.5f + r.unit();
    in.sums29[1] = 200.0f + (float)tid;
    for (int k = 2; k < 8; ++k) in.sums29[k] = r.unit() - 0.5f;
    int k = 8;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) in.sums29[k++] = (a == b) ? 40.0f + 10.0f * r.unit() : r.unit() - 0.5f;
    return in;
}

struct Log {
    std::vector<uint8_t> bytes;
    std::set<std::string> refusal_messages;
    int refusals_not_refused = 0;
    void raw(const void* p, size_t n) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        bytes.insert(bytes.end(), b, b + n);
    }
    template <class T>
    void vec(const std::vector<T>& v) { raw(v.data(), v.size() * sizeof(T)); }
    void call(vors_status st) {  // the status, then the calling thread's last error as it stands now
        const int32_t s = (int32_t)st;
        raw(&s, sizeof s);
        const char* e = vors_last_error();
        raw(e, std::strlen(e) + 1);
    }
    void refused(vors_status st) {
        if (st == VORS_OK) ++refusals_not_refused;
        refusal_messages.insert(vors_last_error());
        call(st);
    }
};

vors_obs make_obs(const Inputs& in) {
    vors_obs o;
    std::memset(&o, 0, sizeof o);
    o.cu = in.cam[0], o.cv = in.cam[1], o.fu = in.cam[2], o.fv = in.cam[3], o.skew = in.cam[4];
    o.rows = ROWS, o.cols = COLS;
    o.template_ = in.tmpl.data(), o.image = in.image.data();
    o.n = (int32_t)in.iz.size();
    o.coordinates = in.coords.data(), o.jacobians = in.jac.data(), o._z_candidates = in.iz.data();
    o.arithmetic = VORS_ARITH_REFERENCE;
    return o;
}

// One refused call, none of which reaches a device: each has a message of its own.
void refuse(int which, const Inputs& in, Log& log) {
    const float identity[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float out7[7], energy, lm_coef;
    int32_t nb_iter;
    int solve_status;
    vors_obs o = make_obs(in);
    std::vector<uint64_t> zkey((size_t)ROWS * COLS);
    std::vector<float> nrm((size_t)ROWS * COLS * 3);
    std::vector<int64_t> sums((size_t)VOXEL_CAPACITY * 4);
    std::vector<uint32_t> obs((size_t)VOXEL_CAPACITY * 2);
    switch (which % N_REFUSALS) {
    case 0: log.refused(vors_lm_solve(&o, identity, nullptr, &nb_iter, &energy, &lm_coef, &solve_status)); break;
    case 1:
        o.rows = 1;
        log.refused(vors_lm_solve(&o, identity, out7, &nb_iter, &energy, &lm_coef, &solve_status));
        break;
    case 2:
        log.refused(vors_render_points_host(in.xyz.data(), in.list_gray.data(), CAPACITY, CAPACITY, nullptr, in.cam, ROWS, COLS, 5000.f, in.pose, 4,
                                            zkey.data(), nullptr, nullptr, nullptr));
        break;
    case 3:
        log.refused(vors_depth_normals_host(in.depth.data(), in.cam, ROWS, COLS, 5000.f, 9, 0.05f, nullptr, nullptr, 0, 0, nullptr, nrm.data(), nullptr));
        break;
    case 4:
        log.refused(vors_voxel_stats_host(in.xyz.data(), in.list_gray.data(), nullptr, CAPACITY, 0.0f, VOXEL_CAPACITY, nullptr, nullptr, sums.data(),
                                          obs.data()));
        break;
    case 5: log.refused(vors_icp_condition_from_sums(nullptr, nullptr, nullptr, nullptr)); break;
    default:
        log.refused(vors_icp_points_joint_host(in.xyz.data(), in.normals.data(), in.list_gray.data(), CAPACITY, CAPACITY, nullptr, in.pose,
                                               in.depth.data(), in.frame_gray.data(), in.cam, ROWS, COLS, 5000.f, -1.0f, 0.0f, 1e-6f, 2, 6, nullptr,
                                               0.0f, 0.0f, 0.0005f, 0.0f, out7, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        break;
    }
}

void work(int tid, const Inputs& in, bool host_only, Barrier* barrier, Log& log) {
    int next_refusal = tid;  // neighbours start at different refusals
    if (barrier) barrier->wait();
    for (int round = 0; round < ROUNDS; ++round) {
        if (barrier && round % 4 == 0) barrier->wait();
        refuse(next_refusal++, in, log);
        {  // vors_lm_step
            float out7[7] = {0};
            int ok = -1;
            log.call(vors_lm_step(in.H, in.g, in.pose, 0.1f * (float)(round + 1), out7, &ok));
            log.raw(out7, sizeof out7);
            log.raw(&ok, sizeof ok);
        }
        {  // vors_icp_points_joint_host
            std::vector<float> res(CAPACITY, 42.f), pres(CAPACITY, 42.f), sums(29, 0.f), out(7, 0.f);
            uint32_t gates[VORS_ICP_GATE_COUNTS] = {0}, photos[VORS_ICP_PHOTO_COUNTS] = {0};
            vors_icp_stats st;
            std::memset(&st, 0, sizeof st);
            log.call(vors_icp_points_joint_host(in.xyz.data(), in.normals.data(), in.list_gray.data(), CAPACITY, CAPACITY, nullptr, in.pose,
                                                in.depth.data(), in.frame_gray.data(), in.cam, ROWS, COLS, 5000.f, 0.5f, 0.0f, 1e-6f, 1 + round % 3, 6,
                                                in.frame_normals.data(), 0.5f, 0.004f, 0.0005f, 20.0f, out.data(), &st, sums.data(), res.data(), gates,
                                                pres.data(), photos));
            log.vec(out), log.vec(sums), log.vec(res), log.vec(pres);
            log.raw(&st, sizeof st), log.raw(gates, sizeof gates), log.raw(photos, sizeof photos);
        }
        refuse(next_refusal++, in, log);
        {  // vors_render_points_host
            const size_t S = (size_t)ROWS * COLS;
            std::vector<uint64_t> zkey(S, 0);
            std::vector<uint16_t> depth(S, 0);
            std::vector<uint8_t> gray(S, 0);
            uint32_t counts[VORS_RENDER_COUNTS] = {0};
            log.call(vors_render_points_host(in.xyz.data(), in.list_gray.data(), CAPACITY, CAPACITY, nullptr, in.cam, ROWS, COLS, 5000.f, in.pose,
                                             1 + round % 3, zkey.data(), depth.data(), gray.data(), counts));
            log.vec(zkey), log.vec(depth), log.vec(gray), log.raw(counts, sizeof counts);
        }
        {  // vors_voxel_stats_host, then vors_voxel_means_host on the filtered list it describes
            std::vector<int64_t> sums((size_t)VOXEL_CAPACITY * 4, -1);
            std::vector<uint32_t> obs((size_t)VOXEL_CAPACITY * 2, 7u), first(VOXEL_CAPACITY, 0u);
            uint32_t total = 0, kept = 0;
            const float voxel_m = 0.02f + 0.01f * (float)(round % 3);
            log.call(vors_voxel_stats_host(in.xyz.data(), in.list_gray.data(), nullptr, CAPACITY, voxel_m, VOXEL_CAPACITY, &total, first.data(),
                                           sums.data(), obs.data()));
            const uint32_t m = total < (uint32_t)VOXEL_CAPACITY ? total : (uint32_t)VOXEL_CAPACITY;
            std::vector<float> filtered((size_t)VOXEL_CAPACITY * 3, 0.f), mean((size_t)VOXEL_CAPACITY * 3, 0.f);
            std::vector<uint8_t> gray_mean(VOXEL_CAPACITY, 0);
            for (uint32_t k = 0; k < m; ++k) std::memcpy(&filtered[3 * k], &in.xyz[3 * (size_t)first[k]], 12);
            log.call(vors_voxel_means_host(filtered.data(), total, VOXEL_CAPACITY, sums.data(), obs.data(), voxel_m, 1 + (uint32_t)(round % 2), 0, nullptr,
                                           mean.data(), gray_mean.data(), &kept));
            log.raw(&total, sizeof total), log.raw(&kept, sizeof kept);
            log.vec(first), log.vec(sums), log.vec(obs), log.vec(mean), log.vec(gray_mean);
        }
        refuse(next_refusal++, in, log);
        {  // vors_depth_normals_host, plane form
            std::vector<float> nrm((size_t)ROWS * COLS * 3, 9.f);
            uint32_t counts[VORS_NORMAL_COUNTS] = {0};
            log.call(vors_depth_normals_host(in.depth.data(), in.cam, ROWS, COLS, 5000.f, 1 + round % 2, 0.05f, in.pose, nullptr, 0, 0, nullptr,
                                             nrm.data(), counts));
            log.vec(nrm), log.raw(counts, sizeof counts);
        }
        {  // vors_icp_condition_from_sums
            float dt = 0.f, dr = 0.f;
            int32_t flags = -1;
            log.call(vors_icp_condition_from_sums(in.sums29, &dt, &dr, &flags));
            log.raw(&dt, 4), log.raw(&dr, 4), log.raw(&flags, 4);
        }
        if (!host_only) {  // vors_lm_solve of a valid observation: the device's answer, or the refusal of a machine without one
            const float identity[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f};
            float out7[7] = {0}, energy = 0.f, lm_coef = 0.f;
            int32_t nb_iter = 0;
            int solve_status = -1;
            const vors_obs o = make_obs(in);
            log.call(vors_lm_solve(&o, identity, out7, &nb_iter, &energy, &lm_coef, &solve_status));
            log.raw(out7, sizeof out7), log.raw(&nb_iter, 4), log.raw(&energy, 4), log.raw(&lm_coef, 4), log.raw(&solve_status, sizeof solve_status);
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
    int failures = 0;
    std::vector<Inputs> inputs;
    for (int t = 0; t < N_THREADS; ++t) inputs.push_back(make_inputs(t));
    // serially first, each thread's work in a thread of its own (a fresh thread starts with an empty last error, as its twin below will)
    std::vector<Log> serial(N_THREADS), concurrent(N_THREADS);
    for (int t = 0; t < N_THREADS; ++t) {
        std::thread th(work, t, std::cref(inputs[t]), host_only, nullptr, std::ref(serial[t]));
        th.join();
    }
    std::set<std::string> messages;
    for (int t = 0; t < N_THREADS; ++t) {
        if (serial[t].refusals_not_refused) {
            std::fprintf(stderr, "FAILED: thread %d: %d calls meant to be refused were accepted\n", t, serial[t].refusals_not_refused);
            ++failures;
        }
        messages.insert(serial[t].refusal_messages.begin(), serial[t].refusal_messages.end());
        if (t && serial[t].bytes == serial[0].bytes) {
            std::fprintf(stderr, "FAILED: thread %d has the log of thread 0: the inputs do not tell the threads apart\n", t);
            ++failures;
        }
    }
    if ((int)messages.size() != N_REFUSALS || messages.count("")) {
        std::fprintf(stderr, "FAILED: %zu distinct refusal messages, expected %d non-empty ones\n", messages.size(), N_REFUSALS);
        ++failures;
    }
    Barrier barrier(N_THREADS);
    std::vector<std::thread> threads;
    for (int t = 0; t < N_THREADS; ++t) threads.emplace_back(work, t, std::cref(inputs[t]), host_only, &barrier, std::ref(concurrent[t]));
    for (auto& th : threads) th.join();
    for (int t = 0; t < N_THREADS; ++t) {
        if (concurrent[t].bytes != serial[t].bytes) {
            size_t at = 0;
            while (at < concurrent[t].bytes.size() && at < serial[t].bytes.size() && concurrent[t].bytes[at] == serial[t].bytes[at]) ++at;
            std::fprintf(stderr, "FAILED: thread %d: the concurrent log (%zu bytes) differs from the serial one (%zu bytes) at byte %zu\n", t,
                         concurrent[t].bytes.size(), serial[t].bytes.size(), at);
            ++failures;
        }
    }
    if (failures) return 1;
    std::printf("host_threads_check: ok (%d threads x %d rounds, %zu log bytes each, %s)\n", N_THREADS, ROUNDS, serial[0].bytes.size(),
                host_only ? "host only" : "vors_lm_solve included");
    return 0;
}
