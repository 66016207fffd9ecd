// Committed controls through the C++ mirror (set_num_control_inputs_saved): a controller that solves while the plant
// keeps moving publishes a plan whose first controls are already on their way to the actuators, so the next solve
// keeps them and optimises only what can still be decided (the setter the reference's m_num_control_inputs_saved,
// ModelControl.hpp:79 / ModelControl.cpp:165-171, never got).
//
//   committed_controls_example <model (path without .json)> [m = 2] [ticks = 6]
// Part 1: one ModelControl with m controls saved, ticks at t_j = j * step; beside it an object with m = 0 and one that
//   never called the setter, all three fed the same measurements.  Prints per tick
//     "mc,<tick>,<status>,u_0...,u_1...,..,u_m..."        (the first m + 1 controls of the published plan)
//     "m0,<tick>,<1 if the m = 0 object's plan equals the untouched object's bit for bit, else 0>"
// Part 2: one BatchModelControl with B = 5 (synchronous calc_u) against five ModelControl objects, all with m saved:
//     "bc,<tick>,<b>,<status_batch>,<status_single>,u_batch (m + 1 controls)...,u_single (m + 1 controls)..."
//     "max_diff,<max |difference| over those controls>"
#include <Mahi/Mpc.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace mahi::mpc;

static std::vector<double> targets(int nx, int N, double h, double t, double phase) {
    const double PI = 3.14159265358979323846;
    std::vector<double> traj;
    double tt = t;
    for (int i = 0; i < N; i++) {  // model_control_example.cpp:58-68, delayed by `phase`
        for (int j = 0; j < nx; j++) {
            if (j < nx / 2) traj.push_back(((j % 2 == 0) ? 1.0 : -1.0) * std::sin(2 * PI * (tt - phase)));
            else traj.push_back((((j - nx / 2) % 2 == 0) ? 1.0 : -1.0) * 2 * PI * std::cos(2 * PI * (tt - phase)));
        }
        tt += h;
    }
    return traj;
}

static bool same_plan(const std::vector<ModelControl::ControlResult>& a,
                      const std::vector<ModelControl::ControlResult>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].u.size() != b[i].u.size() || a[i].x_est.size() != b[i].x_est.size()) return false;
        if (std::memcmp(a[i].u.data(), b[i].u.data(), a[i].u.size() * sizeof(double)) != 0) return false;
        if (std::memcmp(a[i].x_est.data(), b[i].x_est.data(), a[i].x_est.size() * sizeof(double)) != 0) return false;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: committed_controls_example model [m] [ticks]\n");
        return 2;
    }
    const std::string model = argv[1];
    const int m = argc > 2 ? std::atoi(argv[2]) : 2;
    const int ticks = argc > 3 ? std::atoi(argv[3]) : 6;
    const std::vector<double> Q = {10, 1, 5, 5}, R = {5, 5}, Rm = {0.01, 0.01};

    {   // ---- part 1: ModelControl ----
        ModelControl pinned(model, Q, R, Rm), zero(model, Q, R, Rm), plain(model, Q, R, Rm);
        const int nx = pinned.model_parameters.num_x, nu = pinned.model_parameters.num_u;
        const int N = pinned.model_parameters.num_shooting_nodes;
        const double h = pinned.model_parameters.step_size.as_seconds();
        if (nx != 4 || nu != 2) {
            std::fprintf(stderr, "committed_controls_example: a model with four states and two controls\n");
            return 2;
        }
        pinned.set_num_control_inputs_saved(m);
        zero.set_num_control_inputs_saved(0);
        std::vector<double> state(nx);
        for (int j = 0; j < nx; ++j) state[j] = 0.3 * std::sin(0.7 * j + 0.4);
        std::vector<double> up_pinned(nu, 0.0), up_plain(nu, 0.0);
        for (int tick = 0; tick < ticks; ++tick) {
            const double t = tick * h;
            const std::vector<double> tr = targets(nx, N, h, t, 0.0);
            pinned.calc_u(mahi::util::seconds(t), state, up_pinned, tr);
            zero.calc_u(mahi::util::seconds(t), state, up_plain, tr);
            plain.calc_u(mahi::util::seconds(t), state, up_plain, tr);
            std::printf("mc,%d,%d", tick, pinned.last_status());
            for (int i = 0; i <= m && i < N; ++i)
                for (int c = 0; c < nu; ++c) std::printf(",%.17g", pinned.control_results[i].u[c]);
            std::printf("\n");
            std::printf("m0,%d,%d\n", tick,
                        same_plan(zero.control_results, plain.control_results) &&
                                zero.last_status() == plain.last_status() &&
                                zero.last_iterations() == plain.last_iterations()
                            ? 1
                            : 0);
            // the control in force over the step that follows; the measurement drifts with its velocity
            up_pinned = pinned.control_results[0].u;
            up_plain = plain.control_results[0].u;
            for (int j = 0; j < nx / 2; ++j) state[j] += h * state[nx / 2 + j];
        }
    }

    {   // ---- part 2: BatchModelControl against five ModelControl objects ----
        const int64_t B = 5;
        BatchModelControl bc(model, B, Q, R, Rm);
        std::vector<std::unique_ptr<ModelControl>> mc;
        for (int64_t b = 0; b < B; ++b) mc.emplace_back(new ModelControl(model, Q, R, Rm));
        const int nx = bc.model_parameters.num_x, nu = bc.model_parameters.num_u;
        const int N = bc.model_parameters.num_shooting_nodes;
        const double h = bc.model_parameters.step_size.as_seconds();
        bc.set_num_control_inputs_saved(m);
        for (int64_t b = 0; b < B; ++b) mc[b]->set_num_control_inputs_saved(m);
        std::vector<double> state(B * nx), control(B * nu, 0.0);
        for (int64_t b = 0; b < B; ++b)
            for (int j = 0; j < nx; ++j) state[b * nx + j] = 0.3 * std::sin(1.3 * b + 0.7 * j);
        double diff = 0.0;
        for (int tick = 0; tick < ticks; ++tick) {
            const double t = tick * h;
            std::vector<double> trajs;
            std::vector<std::vector<double>> tr_rows;
            for (int64_t b = 0; b < B; ++b) {
                tr_rows.push_back(targets(nx, N, h, t, 0.1 * b));
                trajs.insert(trajs.end(), tr_rows.back().begin(), tr_rows.back().end());
            }
            bc.calc_u(mahi::util::seconds(t), state, control, trajs);
            const std::vector<int> bst = bc.last_status();
            std::vector<double> next(B * nu);
            for (int64_t b = 0; b < B; ++b) {
                const std::vector<double> xs(state.begin() + b * nx, state.begin() + (b + 1) * nx);
                const std::vector<double> us(control.begin() + b * nu, control.begin() + (b + 1) * nu);
                mc[b]->calc_u(mahi::util::seconds(t), xs, us, tr_rows[b]);
                const std::vector<double> V = bc.solution(b);
                std::printf("bc,%d,%lld,%d,%d", tick, static_cast<long long>(b), bst[b], mc[b]->last_status());
                for (int i = 0; i <= m && i < N; ++i)
                    for (int c = 0; c < nu; ++c) std::printf(",%.17g", V[i * (nx + nu) + nx + c]);
                for (int i = 0; i <= m && i < N; ++i)
                    for (int c = 0; c < nu; ++c) {
                        const double s = mc[b]->control_results[i].u[c];
                        std::printf(",%.17g", s);
                        diff = std::max(diff, std::fabs(s - V[i * (nx + nu) + nx + c]));
                    }
                std::printf("\n");
                // both sides continue from the same inputs: the applied control is the single controllers'
                for (int c = 0; c < nu; ++c) next[b * nu + c] = mc[b]->control_results[0].u[c];
            }
            control = next;
            for (int64_t b = 0; b < B; ++b)
                for (int j = 0; j < nx / 2; ++j) state[b * nx + j] += h * state[b * nx + nx / 2 + j];
        }
        std::printf("max_diff,%.6g\n", diff);
    }
    return 0;
}
