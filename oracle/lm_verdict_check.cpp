// TEST INFRASTRUCTURE (tests/test_lm_verdict.py): the device's decision code, vors::lm_verdict of csrc/lie.h compiled for the host,
// against the oracle's LMOptimizerState::eval + stop_criterion (vors_oracle.hpp, Float = float) over a grid of energies, iteration
// counts and damping coefficients. Same decision and same lm_coef BITS everywhere, or exit status 1.
//
// The oracle's side is its own code from end to end: `ok` is what ITS eval() decides for an observation built to have the wanted
// candidate energy — one pixel of grey level a on a black template gives a * a, an empty candidate list gives 0 / 0 = NaN. (An
// infinite CANDIDATE energy cannot come out of 8-bit images, in the oracle or on the device; +inf and -inf appear as kept energies.)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../visual-odometry-rs_amd/csrc/lie.h"
#include "vors_oracle.hpp"

namespace O = vors_oracle;
using O::lm_optimizer::LMOptimizerState;

static uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// An observation whose energy at the identity model is grey * grey (n_points = 1) or NaN (n_points = 0).
struct Scene {
    O::Intrinsics intr{0.f, 0.f, 1.f, 1.f, 0.f};
    O::DMatrix<uint8_t> tmpl, img;
    std::vector<std::pair<size_t, size_t>> coords;
    std::vector<O::Float> iz;
    std::vector<O::Vec6> jac;
    std::vector<O::Mat6> hes;
    Scene(int grey, int n_points) : tmpl(4, 4, 0), img(4, 4, (uint8_t)grey) {
        for (int i = 0; i < n_points; ++i) {
            coords.push_back({0, 0});
            iz.push_back(1.0f);
            jac.push_back(O::Vec6{});
            hes.push_back(O::Mat6{});
        }
    }
    O::lm_optimizer::Obs obs() const {
        O::lm_optimizer::Obs o{};
        o.intrinsics = &intr;
        o.template_ = &tmpl;
        o.image = &img;
        o.coordinates = &coords;
        o._z_candidates = &iz;
        o.jacobians = &jac;
        o.hessians = &hes;
        return o;
    }
};

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float one_below = nextafterf(1.0f, 0.0f), one_above = nextafterf(1.0f, 2.0f);
    const int nb_iters[] = {0, 1, 20, 21, 22};
    const float coefs[] = {0.1f, 1e-8f, 1e8f, 1e-42f /* denormal */, 3e38f /* * 10 overflows */};
    const int greys[] = {0, 2, 255, -1};  // candidate energies 0, 4, 65025, NaN
    const char* names[] = {"rejected, go on", "rejected, stop", "accepted, go on", "accepted, stop"};
    long n_cases = 0, n_bad = 0;
    int seen[4] = {0, 0, 0, 0};
    for (int grey : greys) {
        const Scene scene(grey < 0 ? 0 : grey, grey < 0 ? 0 : 1);
        const O::lm_optimizer::Obs obs = scene.obs();
        const float e = grey < 0 ? nan : (float)(grey * grey);
        // kept energies: below the candidate's (by 1, by one ulp), equal, above (by one ulp, by 0.5, by exactly 1.0f and by its two
        // neighbours — exact for the candidate energy 0 —, by more), infinite, NaN
        std::vector<float> kept = {e - 1.0f, nextafterf(e, -inf), e, nextafterf(e, inf), e + 0.5f, e + one_below, e + 1.0f, e + one_above,
                                   e + 2.0f, e + 1000.0f, inf, -inf, nan};
        if (grey < 0) kept = {0.0f, 1.0f, inf, nan};
        for (float cur_energy : kept)
            for (int nb_iter : nb_iters)
                for (float coef : coefs) {
                    LMOptimizerState st{};
                    st.lm_coef = coef;
                    st.eval_data.energy = cur_energy;
                    st.eval_data.model = O::iso_identity();
                    O::lm_optimizer::EvalState ev = st.eval(obs, O::iso_identity());  // the accept test: lm_optimizer.rs:140-149
                    const bool ok = ev.ok;
                    const float energy = ok ? ev.data.energy : ev.err_energy;
                    const bool stop = LMOptimizerState::stop_criterion(st, (size_t)nb_iter, std::move(ev)) == O::optimizer::Continue::Stop;
                    const int want = (ok ? 2 : 0) | (stop ? 1 : 0);

                    float lm_coef = coef;
                    const int got = (int)vors::lm_verdict(energy, cur_energy, nb_iter, lm_coef);
                    const bool flags_agree = vors::lm_accepted((vors::LmVerdict)got) == ok && vors::lm_stops((vors::LmVerdict)got) == stop;
                    ++n_cases;
                    ++seen[want];
                    if (got != want || !flags_agree || bits(lm_coef) != bits(st.lm_coef) || (!std::isnan(e) && bits(energy) != bits(e))) {
                        ++n_bad;
                        printf("MISMATCH energy %a kept %a nb_iter %d lm_coef %a: oracle '%s' lm_coef %a, lie.h '%s' lm_coef %a\n", energy, cur_energy,
                               nb_iter, coef, names[want], st.lm_coef, names[got & 3], lm_coef);
                    }
                }
    }
    for (int v = 0; v < 4; ++v) {
        printf("%-16s %d cases\n", names[v], seen[v]);
        if (seen[v] == 0) ++n_bad;  // the grid must reach every verdict
    }
    printf("lm_verdict vs oracle: %ld cases, %ld mismatches\n", n_cases, n_bad);
    return n_bad == 0 ? 0 : 1;
}
