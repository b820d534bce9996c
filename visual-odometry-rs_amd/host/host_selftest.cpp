// Compile-and-link check of the C++ host mirror against libvors_hip.so, plus a GPU self-test when a device exists:
// tracks a synthetic 2-frame sequence through vors::track::Config::init / Tracker::track / current_frame and solves one
// level through the optimizer trait (LMOptimizerState::iterative_solve). Exit code 0 = ok, 77 = no GPU (link check only).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../csrc/synth_scene.h"
#include "tracker.hpp"

int main() {
    using namespace vors;
    // the trait skeleton works for any solver: 1-D toy problem (compile-time check of the CRTP contract)
    struct Toy : optimizer::State<Toy, double, std::pair<double, double>, double, int> {
        double x = 0, e = 0;
        static Toy init(const double& target, double m) { Toy t; t.x = m; t.e = (m - target) * (m - target); return t; }
        bool step(double* out, int*) const { *out = 0.5 * (x + 3.0); return true; }
        std::pair<double, double> eval(const double& target, double m) const { return {m, (m - target) * (m - target)}; }
        static std::pair<Toy, optimizer::Continue> stop_criterion(Toy self, std::size_t n, std::pair<double, double> ev) {
            const bool go = self.e - ev.second > 1e-9 && n < 60;
            self.x = ev.first; self.e = ev.second;
            return {self, go ? optimizer::Continue::Forward : optimizer::Continue::Stop};
        }
    };
    auto toy = Toy::iterative_solve(3.0, 11.0);
    if (!toy.ok() || std::fabs(toy.state->x - 3.0) > 1e-3) { std::fprintf(stderr, "trait skeleton failed\n"); return 1; }

    // C-level view of the residual-map entries: the batch entry refuses a NULL handle before it touches a device, and the scale of a
    // histogram is host arithmetic (bins 3 and 4 hold 5 points each, bin 9 ten: the 10th of 20 points ends bin 4 -> median |r| = 5)
    {
        if (vors_batch_residual_maps(nullptr, 1, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != VORS_ERR_INVALID_ARGUMENT) {
            std::fprintf(stderr, "vors_batch_residual_maps accepted a NULL handle\n");
            return 1;
        }
        uint32_t hist[VORS_RESIDUAL_BINS] = {0}, n_inside = 0;
        hist[3] = 5; hist[4] = 5; hist[9] = 10;
        float med = 0, sigma = 0;
        if (vors_residual_scale_from_hist(hist, &med, &sigma, &n_inside) != VORS_OK || med != 5.0f || sigma != (float)(1.4826 * 5.0) || n_inside != 20 ||
            vors_residual_scale_from_hist(nullptr, &med, &sigma, &n_inside) != VORS_ERR_INVALID_ARGUMENT) {
            std::fprintf(stderr, "vors_residual_scale_from_hist failed: median %g sigma %g n %u\n", med, sigma, n_inside);
            return 1;
        }
    }

    // ... and of the depth reprojection: a NULL handle is refused before a device is touched; to_depth / from_depth are host arithmetic
    // (halves round away from zero: 5000 / 0.8 = 6250, 2.5 / 1 -> 3; Unknown <-> 0; the cast saturates)
    {
        if (vors_batch_reproject_depth(nullptr, 1, 0, nullptr, 0, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr) != VORS_ERR_INVALID_ARGUMENT) {
            std::fprintf(stderr, "vors_batch_reproject_depth accepted a NULL handle\n");
            return 1;
        }
        const float idepth[4] = {0.8f, 0.0f, -1.0f, std::nanf("")};
        uint16_t depth[4] = {1, 1, 1, 1}, half = 0;
        const float one = 1.0f;
        float back[4];
        vors_to_depth(5000.0f, idepth, 4, depth);
        vors_to_depth(2.5f, &one, 1, &half);
        vors_from_depth(5000.0f, depth, 4, back);
        if (depth[0] != 6250 || depth[1] != 65535 || depth[2] != 0 || depth[3] != 0 || half != 3 || back[0] != 0.8f || back[2] == back[2]) {
            std::fprintf(stderr, "vors_to_depth / vors_from_depth failed: %u %u %u %u %u %g\n", depth[0], depth[1], depth[2], depth[3], half, back[0]);
            return 1;
        }
    }

    // ... and of the point clouds: a NULL handle is refused before a device is touched; Camera::back_project / project are host arithmetic
    // (pixel (cu, cv) at depth 2 is (0, 0, 2); a NULL pose is the identity; project returns (u w, v w, w))
    {
        if (vors_batch_point_cloud(nullptr, 1, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != VORS_ERR_INVALID_ARGUMENT) {
            std::fprintf(stderr, "vors_batch_point_cloud accepted a NULL handle\n");
            return 1;
        }
        const float cam5[5] = {320.0f, 240.0f, 500.0f, 500.0f, 0.0f}, xy[4] = {320.0f, 240.0f, 820.0f, 240.0f}, depth[2] = {2.0f, 0.5f};
        const float shift[7] = {1.0f, -2.0f, 3.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        float cam_pts[6], world[6], uvw[6];
        vors_camera_back_project(cam5, nullptr, xy, depth, 2, cam_pts);
        vors_camera_back_project(cam5, shift, xy, depth, 2, world);
        vors_camera_project(cam5, shift, world, 2, uvw);
        if (cam_pts[0] != 0.0f || cam_pts[1] != 0.0f || cam_pts[2] != 2.0f || cam_pts[3] != 0.5f || cam_pts[5] != 0.5f || world[0] != 1.0f ||
            world[1] != -2.0f || world[2] != 5.0f || uvw[0] != 640.0f || uvw[2] != 2.0f || uvw[3] != 410.0f || uvw[5] != 0.5f) {
            std::fprintf(stderr, "vors_camera_back_project / vors_camera_project failed: %g %g %g | %g %g %g | %g %g %g\n", cam_pts[3], cam_pts[4], cam_pts[5],
                         world[0], world[1], world[2], uvw[3], uvw[4], uvw[5]);
            return 1;
        }
    }

    // ... and of the depth fusion: a NULL handle is refused before a device is touched; the merge is host arithmetic (1 m of weight 3
    // and 2 m measured agree within 2 m: inverse depths 1 and 0.5, mean 0.875 -> 5714, weight 4; an empty key keeps the measurement)
    {
        if (vors_batch_fuse_depth(nullptr, 1, nullptr, 0, nullptr, 0.f, nullptr, 255, 0, nullptr, nullptr, nullptr, nullptr, nullptr) != VORS_ERR_INVALID_ARGUMENT) {
            std::fprintf(stderr, "vors_batch_fuse_depth accepted a NULL handle\n");
            return 1;
        }
        const uint64_t keys[2] = {0x3f80000000000000ull, VORS_ZKEY_EMPTY};
        const uint16_t cur[2] = {10000, 7000};
        const uint8_t w3 = 3;
        uint16_t depth[2] = {0, 0};
        uint8_t weight[2] = {0, 0};
        uint32_t counts[VORS_FUSE_COUNTS];
        if (vors_fuse_depth_pixels(5000.0f, 2.0f, 255, 0, 2, keys, cur, &w3, 1, depth, weight, counts) != VORS_OK || depth[0] != 5714 ||
            weight[0] != 4 || depth[1] != 7000 || weight[1] != 1 || counts[0] != 1 || counts[3] != 1) {
            std::fprintf(stderr, "vors_fuse_depth_pixels failed: %u %u %u %u\n", depth[0], weight[0], depth[1], weight[1]);
            return 1;
        }
    }

    if (vors_device_count() < 1) { std::printf("host_selftest: link ok, no GPU (skipping device part)\n"); return 77; }
    const int rows = 120, cols = 160;
    const double s = cols / 640.0;
    const vors_synth::CameraD cam{s * (318.643040 + 0.5) - 0.5, s * (255.313989 + 0.5) - 0.5, s * 517.306408, s * 516.469215, 0.0};
    std::vector<uint8_t> g0(rows * cols), g1(rows * cols);
    std::vector<uint16_t> d0(rows * cols), d1(rows * cols);
    double xi[6], zero[6] = {0, 0, 0, 0, 0, 0};
    vors_synth::pair_twist(42, 1.0, xi);
    const auto id = vors_synth::se3_exp_d(zero), m = vors_synth::se3_exp_d(xi);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            vors_synth::render_pixel(42, 0, cam, id, x, y, 2, &g0[y * cols + x], &d0[y * cols + x]);
            vors_synth::render_pixel(42, 1, cam, m, x, y, 2, &g1[y * cols + x], &d1[y * cols + x]);
        }
    track::Config config{4, 7, tum_rgbd::DEPTH_SCALE, Intrinsics{{(float)cam.cu, (float)cam.cv}, {(float)cam.fu, (float)cam.fv}, 0.0f}, 0.0001f};
    track::Tracker tracker = config.init(0.0, {d0.data(), rows, cols, VORS_ROW_MAJOR}, 0.0, {g0.data(), rows, cols, VORS_ROW_MAJOR});
    tracker.set_logging(false);
    tracker.track(1.0, {d1.data(), rows, cols, VORS_ROW_MAJOR}, 1.0, {g1.data(), rows, cols, VORS_ROW_MAJOR});
    auto [t, pose] = tracker.current_frame();
    float gt[7];
    vors_synth::rigid_to_pose7(m, xi, gt);
    float err = 0;
    for (int k = 0; k < 7; ++k) err = std::fmax(err, std::fabs(tracker.last_stats().lm_model[k] - gt[k]));
    std::printf("host_selftest: t=%g pose=[%g %g %g | %g %g %g %g] max|model-gt|=%g status=%d\n", t, pose[0], pose[1], pose[2], pose[3],
                pose[4], pose[5], pose[6], err, tracker.last_status());
    return (t == 1.0 && err < 1e-2 && tracker.last_status() == 0) ? 0 : 1;
}
