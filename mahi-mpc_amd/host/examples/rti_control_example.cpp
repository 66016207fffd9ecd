// Closed loops in real-time iteration mode (set_rti_mode): B 2-link arms through BatchModelControl
// (`batch`) or one through ModelControl (`single`, B must be 1), each on the model's own Euler plant (the
// <name>_get_x_dot_init external, as batch_control_example.cpp).  One calc_u per tick of the model's step.
//
//   rti_control_example <model (path without .json)> <B> <ticks> batch|single [jump_tick jump_size] [skip_tick]
//                       [key=value ...]
// jump_tick / jump_size: before the calc_u of that tick, jump_size is added to every entry of every measured state (a
//   disturbance the preparation did not see).  skip_tick: no calc_u at that tick (the plant moves on under the plan's
//   next control), which leaves the preparation stale.  A negative tick number switches the event off.
// key=value, in any position after the mode:
//   step_inf_max=<x>   the fallback threshold of set_rti_mode (default inf)
//   limit=<x>          update_control_limits at -x .. x before the first tick
//   rti=0              leave the mode off: the same loop on full solves
//   pin=<m>            set_num_control_inputs_saved(m)      } with the mode on the first tick throws: the message is
//   feedback=<n>       set_feedback_stages(n)               } printed as {"error": ...} and the exit code is 3
//   quiet=1            no line per tick
//   glitch=<tick>      at that tick entry 0 of the measured state of instance B / 2 handed to calc_u is NaN (a sensor
//                      glitch); the printed state is the measured one, the plant's own state is untouched
// One JSON line per tick: the tick's inputs (state, control, traj), its kind ("full", "rti", "off" or "skipped"), u0,
// step_inf, status, iters and the plan ([B][NV]; `single`: the N published stages x_k, u_k); then one summary line
// with the counters, mean_tick_ms, mean_feedback_latency_ms (`batch`) and the tracking cost
// sum_ticks sum_b |q - q_target|^2.
#include <Mahi/Mpc.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

using namespace mahi::mpc;

static std::vector<double> targets(int nx, int N, double h, double t, double phase) {
    const double PI = 3.14159265358979323846;
    std::vector<double> traj;
    double tt = t;
    for (int i = 0; i < N; i++) {  // batch_control_example.cpp
        for (int j = 0; j < nx; j++) {
            if (j < nx / 2) traj.push_back(((j % 2 == 0) ? 1.0 : -1.0) * std::sin(2 * PI * (tt - phase)));
            else traj.push_back((((j - nx / 2) % 2 == 0) ? 1.0 : -1.0) * 2 * PI * std::cos(2 * PI * (tt - phase)));
        }
        tt += h;
    }
    return traj;
}

static void print_array(const char* key, const std::vector<double>& v) {
    std::printf(",\"%s\":[", key);
    for (size_t i = 0; i < v.size(); ++i) {
        if (std::isfinite(v[i])) std::printf("%s%.17g", i ? "," : "", v[i]);
        else std::printf("%s\"%s\"", i ? "," : "", std::isnan(v[i]) ? "nan" : (v[i] > 0 ? "inf" : "-inf"));
    }
    std::printf("]");
}
static void print_array(const char* key, const std::vector<int>& v) {
    std::printf(",\"%s\":[", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? "," : "", v[i]);
    std::printf("]");
}

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr,
                     "usage: rti_control_example model B ticks batch|single [jump_tick jump_size] [skip_tick] [key=value ...]\n");
        return 2;
    }
    const std::string model = argv[1];
    const int64_t B = std::atoll(argv[2]);
    const int ticks = std::atoi(argv[3]);
    const bool single = !std::strcmp(argv[4], "single");
    double step_inf_max = std::numeric_limits<double>::infinity(), limit = 0.0, jump_size = 0.0;
    int jump_tick = -1, skip_tick = -1, glitch_tick = -1, pin = 0, feedback = 0, npos = 0;
    bool rti = true, quiet = false;
    for (int i = 5; i < argc; ++i) {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) {
            if (npos == 0) jump_tick = std::atoi(argv[i]);
            else if (npos == 1) jump_size = std::atof(argv[i]);
            else skip_tick = std::atoi(argv[i]);
            ++npos;
            continue;
        }
        const std::string key(argv[i], static_cast<size_t>(eq - argv[i]));
        if (key == "step_inf_max") step_inf_max = std::atof(eq + 1);
        else if (key == "limit") limit = std::atof(eq + 1);
        else if (key == "rti") rti = std::atoi(eq + 1) != 0;
        else if (key == "pin") pin = std::atoi(eq + 1);
        else if (key == "feedback") feedback = std::atoi(eq + 1);
        else if (key == "quiet") quiet = std::atoi(eq + 1) != 0;
        else if (key == "glitch") glitch_tick = std::atoi(eq + 1);
        else {
            std::fprintf(stderr, "unknown option %s\n", argv[i]);
            return 2;
        }
    }
    if (single && B != 1) {
        std::fprintf(stderr, "single needs B = 1\n");
        return 2;
    }
    try {
        std::unique_ptr<BatchModelControl> bc;
        std::unique_ptr<ModelControl> mc;
        if (single) mc.reset(new ModelControl(model, {10, 1, 5, 5}, {5, 5}, {0.01, 0.01}));
        else bc.reset(new BatchModelControl(model, B, {10, 1, 5, 5}, {5, 5}, {0.01, 0.01}));
        const ModelParameters& mp = single ? mc->model_parameters : bc->model_parameters;
        const int nx = mp.num_x, nu = mp.num_u, N = mp.num_shooting_nodes;
        const double h = mp.step_size.as_seconds();
        auto ext = external(mp.name + "_get_x_dot_init", model + "_linear_functions.so");
        if (limit > 0.0) {
            const std::vector<double> lo(nu, -limit), hi(nu, limit);
            if (single) mc->update_control_limits(lo, hi);
            else bc->update_control_limits(lo, hi);
        }
        if (pin > 0) single ? mc->set_num_control_inputs_saved(pin) : bc->set_num_control_inputs_saved(pin);
        if (feedback > 0) single ? mc->set_feedback_stages(feedback) : bc->set_feedback_stages(feedback);
        if (rti) single ? mc->set_rti_mode(true, step_inf_max) : bc->set_rti_mode(true, step_inf_max);

        std::vector<double> state(B * nx), control(B * nu, 0.0);
        for (int64_t b = 0; b < B; ++b)
            for (int j = 0; j < nx; ++j) state[b * nx + j] = 0.05 * std::sin(1.3 * b + 0.7 * j);
        double cost = 0.0;
        long long n_rti = 0, n_full = 0;
        for (int tick = 0; tick < ticks; ++tick) {
            const double t = tick * h;
            std::vector<double> tr;
            for (int64_t b = 0; b < B; ++b) {
                const std::vector<double> r = targets(nx, N, h, t, 0.1 * b);
                tr.insert(tr.end(), r.begin(), r.end());
            }
            if (tick == jump_tick)
                for (double& v : state) v += jump_size;
            for (int64_t b = 0; b < B; ++b)
                for (int j = 0; j < nx / 2; ++j) {
                    const double e = state[b * nx + j] - tr[b * N * nx + j];
                    cost += e * e;
                }
            const char* kind = "skipped";
            const std::vector<double> control_in = control;
            std::vector<double> measured = state;   // what the controller sees; the plant keeps `state`
            if (tick == glitch_tick) measured[(B / 2) * nx] = std::numeric_limits<double>::quiet_NaN();
            if (tick != skip_tick) {
                if (single) mc->calc_u(mahi::util::seconds(t), measured, control, tr);
                else bc->calc_u(mahi::util::seconds(t), measured, control, tr);
                const long long r = single ? mc->rti_ticks() : bc->rti_ticks();
                const long long f = single ? mc->full_solve_ticks() : bc->full_solve_ticks();
                kind = r > n_rti ? "rti" : (f > n_full ? "full" : "off");
                n_rti = r, n_full = f;
            }
            std::vector<double> plan, si;
            std::vector<int> st, it;
            if (single) {
                control = mc->control_at_time(mahi::util::seconds(t)).u;
                for (const auto& cr : mc->control_results) {
                    plan.insert(plan.end(), cr.x_est.begin(), cr.x_est.end());
                    plan.insert(plan.end(), cr.u.begin(), cr.u.end());
                }
                si = {mc->last_step_inf()};
                st = {mc->last_status()};
                it = {mc->last_iterations()};
            } else {
                control = bc->controls_at_time(mahi::util::seconds(t));
                for (int64_t b = 0; b < B; ++b) {
                    const std::vector<double> v = bc->solution(b);
                    plan.insert(plan.end(), v.begin(), v.end());
                }
                si = bc->last_step_inf();
                st = bc->last_status();
                it = bc->last_iterations();
            }
            if (!quiet) {
                std::printf("{\"tick\":%d,\"t\":%.17g,\"kind\":\"%s\"", tick, t, kind);
                print_array("state", measured);
                print_array("control", control_in);
                print_array("traj", tr);
                print_array("u0", control);
                print_array("step_inf", si);
                print_array("status", st);
                print_array("iters", it);
                print_array("plan", plan);
                std::printf("}\n");
            }
            for (int64_t b = 0; b < B; ++b) {   // the plant: one Euler step under the control just published
                std::vector<double> x(state.begin() + b * nx, state.begin() + (b + 1) * nx);
                std::vector<double> u(control.begin() + b * nu, control.begin() + (b + 1) * nu);
                const std::vector<double> xd = ext({x, u})[0];
                for (int j = 0; j < nx; ++j) state[b * nx + j] += xd[j] * h;
            }
        }
        std::printf("{\"summary\":1,\"rti_ticks\":%lld,\"full_solve_ticks\":%lld,\"mean_tick_ms\":%.6g,"
                    "\"mean_feedback_latency_ms\":%.6g,\"tracking_cost\":%.17g}\n",
                    n_rti, n_full, single ? 0.0 : bc->mean_tick_ms(), single ? 0.0 : bc->mean_feedback_latency_ms(), cost);
    } catch (const std::exception& e) {
        std::string msg = e.what();
        for (char& c : msg)
            if (c == '"' || c == '\\' || c == '\n') c = ' ';
        std::printf("{\"error\":\"%s\"}\n", msg.c_str());
        return 3;
    }
    return 0;
}
