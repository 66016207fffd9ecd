// Feedback along the plan for a controller with state limits (x_min / x_max of the model file, the realistic
// configuration: |qdot| limits).  A state-bounded solve is an interior-point solve; its feedback gains are those of the
// barrier problem at the plan, and set_feedback_stages works once the sensitivity barrier is switched on
// (set_sensitivity_barrier; mmpc_set_sensitivity_barrier in include/mmpc.h).
//
//   state_limit_feedback_example <model (path without .json, with finite x_min / x_max)> [n = 3]
// Part 1: one ModelControl.  Prints
//     "refused,<1 if calc_u with feedback stages and the barrier off throws naming the state bounds, else 0>"
//     "status,<solver status>,<feedback_status()>"
//     "g,<i>,G_i published (nu x (nx + nu), row-major)...,G_i of the C-ABI calls on the same inputs..."   for i < n
//     "x0,x_est_0..."     "u0,u_0 of the plan..."
//     "fb,control_at_time(t_0, x_est_0 + 1e-3 (1, -1, 1, -1))..."
// Part 2: one BatchModelControl with B = 5, synchronous calc_u.  Prints
//     "bg,<b>,<i>,<gain status>,G_i published...,G_i of mmpc_feedback_gains_batch_host at the published plans..."
//     "bu,<b>,x_est_0 (nx)...,u_0 (nu)...,controls_at_time at the moved state (nu)..."
#include <Mahi/Mpc.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mmpc.h"

using namespace mahi::mpc;

static std::vector<double> targets(int nx, int N, double h, double phase) {
    const double PI = 3.14159265358979323846;
    std::vector<double> traj;
    double tt = 0.0;
    for (int i = 0; i < N; i++) {  // model_control_example.cpp:58-68 at a fifth of the amplitude, delayed by `phase`
        for (int j = 0; j < nx; j++) {
            if (j < nx / 2) traj.push_back(((j % 2 == 0) ? 0.2 : -0.2) * std::sin(2 * PI * (tt - phase)));
            else traj.push_back((((j - nx / 2) % 2 == 0) ? 0.2 : -0.2) * 2 * PI * std::cos(2 * PI * (tt - phase)));
        }
        tt += h;
    }
    return traj;
}

static void print_values(const std::vector<double>& v) {
    for (double x : v) std::printf(",%.17g", x);
}
static void check(int rc, const char* what) {
    if (rc != MMPC_OK) throw std::runtime_error(std::string(what) + ": " + mmpc_last_error());
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: state_limit_feedback_example model [n]\n");
        return 2;
    }
    const std::string model = argv[1];
    const int n = argc > 2 ? std::atoi(argv[2]) : 3;
    const std::vector<double> Q = {10, 1, 5, 5}, R = {5, 5}, Rm = {0.01, 0.01};
    const double moved[4] = {1e-3, -1e-3, 1e-3, -1e-3};
    std::vector<double> w = Q;
    w.insert(w.end(), R.begin(), R.end());
    w.insert(w.end(), Rm.begin(), Rm.end());

    // the C-ABI handle of the same model file, with the same barrier
    std::ifstream in(model + ".json");
    std::stringstream text;
    text << in.rdbuf();
    mmpc_opts opts;
    mmpc_default_opts(&opts);
    mmpc_handle* h = nullptr;
    check(mmpc_create_from_json(text.str().c_str(), &opts, &h), "mmpc_create_from_json");
    double mu = 0.0, cap = 0.0;
    check(mmpc_sensitivity_barrier_default(&mu, &cap), "mmpc_sensitivity_barrier_default");
    check(mmpc_set_sensitivity_barrier(h, mu, cap), "mmpc_set_sensitivity_barrier");

    {   // ---- part 1: ModelControl ----
        ModelControl mc(model, Q, R, Rm);
        const int nx = mc.model_parameters.num_x, nu = mc.model_parameters.num_u, K = nx + nu;
        const int N = mc.model_parameters.num_shooting_nodes;
        const double hs = mc.model_parameters.step_size.as_seconds();
        if (nx != 4 || nu != 2) {
            std::fprintf(stderr, "state_limit_feedback_example: a model with four states and two controls\n");
            return 2;
        }
        // the velocity targets peak at 0.4 pi = 1.26: a velocity limit below that is active along the plan
        const std::vector<double> tr = targets(nx, N, hs, 0.0);
        const std::vector<double> state = {0.02, -0.01, 0.3, -0.3}, up(nu, 0.0);
        mc.set_feedback_stages(n);
        bool refused = false;
        try {
            mc.calc_u(mahi::util::seconds(0.0), state, up, tr);
        } catch (const std::runtime_error& e) {
            refused = std::string(e.what()).find("state bounds") != std::string::npos;
        }
        std::printf("refused,%d\n", refused ? 1 : 0);
        ModelControl fb(model, Q, R, Rm);
        fb.set_sensitivity_barrier();
        fb.set_feedback_stages(n);
        fb.calc_u(mahi::util::seconds(0.0), state, up, tr);
        std::printf("status,%d,%d\n", fb.last_status(), fb.feedback_status());
        // the same two calls through the C-ABI
        std::vector<double> V(static_cast<size_t>(nx) * (N + 1) + static_cast<size_t>(nu) * N, 0.0);
        std::vector<double> G(static_cast<size_t>(n) * nu * K, 0.0);
        int32_t st = -1, it = 0, gst = -1;
        double kkt = 0.0;
        // the control limits as calc_u passes them
        const std::vector<double>&lo = fb.model_parameters.u_min, &hi = fb.model_parameters.u_max;
        const double* lb = lo.size() == static_cast<size_t>(nu) ? lo.data() : nullptr;
        const double* ub = hi.size() == static_cast<size_t>(nu) ? hi.data() : nullptr;
        check(mmpc_solve_batch_host(h, 1, state.data(), up.data(), tr.data(), w.data(), 0, lb, ub, V.data(),
                                    &st, &it, &kkt),
              "mmpc_solve_batch_host");
        check(mmpc_feedback_gains_batch_host(h, 1, V.data(), up.data(), tr.data(), w.data(), 0, lb, ub, 0, 0,
                                             n, MMPC_HESSIAN_AUTO, MMPC_GAIN_KERNEL_AUTO, G.data(), &gst),
              "mmpc_feedback_gains_batch_host");
        for (int i = 0; i < n; ++i) {
            std::printf("g,%d", i);
            print_values(fb.feedback_gain(i));
            print_values(std::vector<double>(G.begin() + static_cast<size_t>(i) * nu * K,
                                             G.begin() + static_cast<size_t>(i + 1) * nu * K));
            std::printf("\n");
        }
        std::printf("x0");
        print_values(fb.control_results[0].x_est);
        std::printf("\nu0");
        print_values(fb.control_results[0].u);
        std::vector<double> xm = state;
        for (int j = 0; j < nx; ++j) xm[j] += moved[j];
        std::printf("\nfb");
        print_values(fb.control_at_time(mahi::util::seconds(0.0), xm).u);
        std::printf("\n");
    }

    {   // ---- part 2: BatchModelControl ----
        const int64_t B = 5;
        BatchModelControl bc(model, B, Q, R, Rm);
        const int nx = bc.model_parameters.num_x, nu = bc.model_parameters.num_u, K = nx + nu;
        const int N = bc.model_parameters.num_shooting_nodes;
        const double hs = bc.model_parameters.step_size.as_seconds();
        bc.set_sensitivity_barrier();
        bc.set_feedback_stages(n);
        std::vector<double> state(B * nx), control(B * nu, 0.0), trajs;
        for (int64_t b = 0; b < B; ++b) {
            for (int j = 0; j < nx; ++j)
                state[b * nx + j] = 0.05 * std::sin(1.3 * b + 0.7 * j) + (j < nx / 2 ? 0.0 : 0.25);
            const std::vector<double> tr = targets(nx, N, hs, 0.02 * b);
            trajs.insert(trajs.end(), tr.begin(), tr.end());
        }
        bc.calc_u(mahi::util::seconds(0.0), state, control, trajs);
        std::vector<double> xm = state;
        for (int64_t b = 0; b < B; ++b)
            for (int j = 0; j < nx; ++j) xm[b * nx + j] += moved[j];
        const std::vector<double> ub = bc.controls_at_time(mahi::util::seconds(0.0), xm);
        const std::vector<int> gst = bc.feedback_status();
        std::vector<double> V, G(static_cast<size_t>(B) * n * nu * K, 0.0);
        for (int64_t b = 0; b < B; ++b) {
            const std::vector<double> v = bc.solution(b);
            V.insert(V.end(), v.begin(), v.end());
        }
        std::vector<int32_t> st(B, -1);
        check(mmpc_feedback_gains_batch_host(h, B, V.data(), control.data(), trajs.data(), w.data(), 0, nullptr,
                                             nullptr, 0, 0, n, MMPC_HESSIAN_AUTO, MMPC_GAIN_KERNEL_AUTO, G.data(),
                                             st.data()),
              "mmpc_feedback_gains_batch_host");
        for (int64_t b = 0; b < B; ++b) {
            for (int i = 0; i < n; ++i) {
                std::printf("bg,%lld,%d,%d", static_cast<long long>(b), i, gst[b]);
                print_values(bc.feedback_gain(b, i));
                const size_t o = (static_cast<size_t>(b) * n + i) * nu * K;
                print_values(std::vector<double>(G.begin() + o, G.begin() + o + static_cast<size_t>(nu) * K));
                std::printf("\n");
            }
            const ModelControl::ControlResult r0 = bc.control_at_time(b, mahi::util::seconds(0.0));
            std::printf("bu,%lld", static_cast<long long>(b));
            print_values(r0.x_est);
            print_values(r0.u);
            print_values(std::vector<double>(ub.begin() + b * nu, ub.begin() + (b + 1) * nu));
            std::printf("\n");
        }
    }
    mmpc_destroy(h);
    return 0;
}
