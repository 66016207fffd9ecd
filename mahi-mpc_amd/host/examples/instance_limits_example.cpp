// Per-instance control limits through the C++ mirror: one BatchModelControl with B = 5 instances and three distinct
// limit sets (update_control_limits(b, ...)) against five ModelControl objects that each have their own
// update_control_limits (the reference's one controller per plant, ModelControl.cpp:205-209), over three synchronous
// ticks with the warm start carried along; then the all-instances overload, which returns the batch to one shared box.
// ModelControl::calc_u_batch with a row of limits per instance is compared on the first tick as well.
//
//   instance_limits_example <model (path without .json)>
// prints "tick,<phase>,<tick>,<b>,u_batch...,u_single...,status_batch,status_single" per instance,
//        "calc_u_batch,<b>,u...,status" per instance of the first tick,
//        "max_diff,<per-instance phase>,<shared phase>,<calc_u_batch>" at the end (max |u_0* difference|)
#include <Mahi/Mpc.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
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

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: instance_limits_example model\n");
        return 2;
    }
    const std::string model = argv[1];
    const int64_t B = 5;
    const std::vector<double> Q = {10, 1, 5, 5}, R = {5, 5}, Rm = {0.01, 0.01};
    BatchModelControl bc(model, B, Q, R, Rm);
    std::vector<std::unique_ptr<ModelControl>> mc;
    for (int64_t b = 0; b < B; ++b) mc.emplace_back(new ModelControl(model, Q, R, Rm));
    const int nx = bc.model_parameters.num_x, nu = bc.model_parameters.num_u, N = bc.model_parameters.num_shooting_nodes;
    const double h = bc.model_parameters.step_size.as_seconds();
    if (nu != 2) {
        std::fprintf(stderr, "instance_limits_example: a model with two controls\n");
        return 2;
    }

    // three limit sets over five instances: a derated two-sided box, a one-sided pair, and no limit at all
    const double inf = 10e30;
    const std::vector<std::vector<double>> lo = {{-2.0, -1.6}, {-inf, -1.0}, {-inf, -inf}};
    const std::vector<std::vector<double>> hi = {{1.8, 2.0}, {1.0, inf}, {inf, inf}};
    const int set_of[5] = {0, 1, 2, 1, 0};
    std::vector<std::vector<double>> u_mins, u_maxs;
    for (int64_t b = 0; b < B; ++b) {
        bc.update_control_limits(b, lo[set_of[b]], hi[set_of[b]]);
        mc[b]->update_control_limits(lo[set_of[b]], hi[set_of[b]]);
        u_mins.push_back(lo[set_of[b]]);
        u_maxs.push_back(hi[set_of[b]]);
    }

    std::vector<double> state(B * nx), control(B * nu, 0.0);
    for (int64_t b = 0; b < B; ++b)
        for (int j = 0; j < nx; ++j) state[b * nx + j] = 0.3 * std::sin(1.3 * b + 0.7 * j);
    double diff[2] = {0.0, 0.0}, diff_cub = 0.0;
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1) {   // the all-instances overload: every controller back to one shared box
            bc.update_control_limits({-0.5, -0.5}, {0.5, 0.5});
            for (int64_t b = 0; b < B; ++b) mc[b]->update_control_limits({-0.5, -0.5}, {0.5, 0.5});
        }
        for (int tick = 0; tick < 3; ++tick) {
            const double t = (phase * 3 + tick) * 5 * h;
            std::vector<double> trajs;
            std::vector<std::vector<double>> st_rows, ct_rows, tr_rows;
            for (int64_t b = 0; b < B; ++b) {
                const std::vector<double> r = targets(nx, N, h, t, 0.1 * b);
                trajs.insert(trajs.end(), r.begin(), r.end());
                st_rows.emplace_back(state.begin() + b * nx, state.begin() + (b + 1) * nx);
                ct_rows.emplace_back(control.begin() + b * nu, control.begin() + (b + 1) * nu);
                tr_rows.push_back(r);
            }
            if (phase == 0 && tick == 0) {   // cold start on both sides: calc_u_batch with per-instance limits
                std::vector<int> st;
                const auto V = mc[0]->calc_u_batch(st_rows, ct_rows, tr_rows, u_mins, u_maxs, &st);
                for (int64_t b = 0; b < B; ++b) {
                    std::printf("calc_u_batch,%lld", static_cast<long long>(b));
                    for (int c = 0; c < nu; ++c) std::printf(",%.17g", V[b][nx + c]);
                    std::printf(",%d\n", st[b]);
                }
                // compared below with the five controllers' first tick
                bc.calc_u(mahi::util::seconds(t), state, control, trajs);
                for (int64_t b = 0; b < B; ++b) {
                    const std::vector<double> u = bc.control_at_time(b, mahi::util::seconds(t)).u;
                    for (int c = 0; c < nu; ++c) diff_cub = std::max(diff_cub, std::fabs(u[c] - V[b][nx + c]));
                }
            } else {
                bc.calc_u(mahi::util::seconds(t), state, control, trajs);
            }
            const std::vector<int> bst = bc.last_status();
            std::vector<double> next(B * nu);
            for (int64_t b = 0; b < B; ++b) {
                mc[b]->calc_u(mahi::util::seconds(t), st_rows[b], ct_rows[b], tr_rows[b]);
                const std::vector<double> ub = bc.control_at_time(b, mahi::util::seconds(t)).u;
                const std::vector<double> us = mc[b]->control_at_time(mahi::util::seconds(t)).u;
                std::printf("tick,%d,%d,%lld", phase, tick, static_cast<long long>(b));
                for (int c = 0; c < nu; ++c) std::printf(",%.17g", ub[c]);
                for (int c = 0; c < nu; ++c) std::printf(",%.17g", us[c]);
                std::printf(",%d,%d\n", bst[b], mc[b]->last_status());
                for (int c = 0; c < nu; ++c) {
                    diff[phase] = std::max(diff[phase], std::fabs(ub[c] - us[c]));
                    next[b * nu + c] = us[c];
                }
            }
            // both sides continue from the same measurement: the state drifts a little, the applied control is the
            // single controllers' (so a difference does not feed back into the next tick's inputs)
            control = next;
            for (int64_t b = 0; b < B; ++b)
                for (int j = 0; j < nx / 2; ++j) state[b * nx + j] += 5 * h * state[b * nx + nx / 2 + j];
        }
    }
    std::printf("max_diff,%.6g,%.6g,%.6g\n", diff[0], diff[1], diff_cub);
    return 0;
}
