// Feedback along the plan through the C++ mirror (set_feedback_stages): between two solves the controller has only
// the open-loop plan (ModelControl.cpp:174-197); with the gains G_i = d u_i* / d(x_i, u_{i-1}) of the first n stages
// published beside it, control_at_time(t, x_measured) returns the neighbouring-extremal control
// u_i + G_i[:, :nx] (x_measured - x_est_i).
//
//   feedback_control_example <model (path without .json)> [n = 3] [ticks = 2]
// Part 1: one ModelControl with n feedback stages, one solve.  Prints
//     "plan,<i>,<1 if control_at_time(t_i, x_est_i) is the plan's stage i bit for bit, else 0>"   for i = 0 .. n
//     "status,<solver status>,<feedback_status()>"
//     "g0,G_0 (nu x (nx + nu), row-major)..."     "x0,x_est_0..."     "u0,u_0 of the plan..."
//     "fb,control_at_time(t_0, x_est_0 + 1e-3 (1, -1, 1, -1))..."
//     "resolve,<status>,u_0 of a solve from that moved state..."
// Part 2: an object that never called set_feedback_stages beside one with n stages, `ticks` ticks of the same
//   measurements:  "same,<tick>,<1 if both publish the same plan, status and iteration count bit for bit, else 0>"
//   and "nofb,<1 if the untouched object's control_at_time(t, x_measured) is its plan, else 0>"
// Part 3: one BatchModelControl with B = 5 (synchronous calc_u) against five ModelControl objects, all with n stages:
//     "bg,<b>,<i>,<gain status batch>,<gain status single>,G_i batch...,G_i single..."   for i < n, last tick
//     "bu,<b>,controls_at_time batch (nu)...,control_at_time single (nu)..."   at the moved states, last tick
#include <Mahi/Mpc.hpp>

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

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}
static bool same_result(const ModelControl::ControlResult& a, const ModelControl::ControlResult& b) {
    return a.time.as_seconds() == b.time.as_seconds() && same_bits(a.u, b.u) && same_bits(a.x_est, b.x_est);
}
static bool same_plan(const std::vector<ModelControl::ControlResult>& a,
                      const std::vector<ModelControl::ControlResult>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!same_result(a[i], b[i])) return false;
    return true;
}
static void print_row(const char* tag, const std::vector<double>& v) {
    std::printf("%s", tag);
    for (double x : v) std::printf(",%.17g", x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: feedback_control_example model [n] [ticks]\n");
        return 2;
    }
    const std::string model = argv[1];
    const int n = argc > 2 ? std::atoi(argv[2]) : 3;
    const int ticks = argc > 3 ? std::atoi(argv[3]) : 2;
    const std::vector<double> Q = {10, 1, 5, 5}, R = {5, 5}, Rm = {0.01, 0.01};
    const double moved[4] = {1e-3, -1e-3, 1e-3, -1e-3};

    {   // ---- part 1: ModelControl ----
        ModelControl fb(model, Q, R, Rm), re(model, Q, R, Rm);
        const int nx = fb.model_parameters.num_x, nu = fb.model_parameters.num_u;
        const int N = fb.model_parameters.num_shooting_nodes;
        const double h = fb.model_parameters.step_size.as_seconds();
        if (nx != 4 || nu != 2) {
            std::fprintf(stderr, "feedback_control_example: a model with four states and two controls\n");
            return 2;
        }
        fb.set_feedback_stages(n);
        // a controller in its tracking regime: the arm is on its reference up to a tracking error (the first-order
        // correction is judged against a re-solve below; far from the reference the second-order remainder of the
        // solution map is larger -- from 0.3 sin(0.7 j + 0.4) at rest it is 1 / 43 of the plan's error at this step)
        const std::vector<double> tr = targets(nx, N, h, 0.0, 0.0);
        const double track_err[4] = {0.05, -0.03, 0.2, -0.1};
        std::vector<double> state(nx), up(nu, 0.0);
        for (int j = 0; j < nx; ++j) state[j] = tr[j] + track_err[j];
        fb.calc_u(mahi::util::seconds(0.0), state, up, tr);
        for (int i = 0; i <= n && i < N; ++i) {
            const ModelControl::ControlResult& p = fb.control_results[i];
            // a time just past t_i: the reference's rule returns the last stage whose time is before it
            const ModelControl::ControlResult r = fb.control_at_time(mahi::util::seconds((i + 0.5) * h), p.x_est);
            std::printf("plan,%d,%d\n", i, same_result(r, p) ? 1 : 0);
        }
        std::printf("status,%d,%d\n", fb.last_status(), fb.feedback_status());
        print_row("g0", fb.feedback_gain(0));
        print_row("x0", fb.control_results[0].x_est);
        print_row("u0", fb.control_results[0].u);
        std::vector<double> xm = state;
        for (int j = 0; j < nx; ++j) xm[j] += moved[j];
        print_row("fb", fb.control_at_time(mahi::util::seconds(0.0), xm).u);
        re.calc_u(mahi::util::seconds(0.0), xm, up, tr);
        std::printf("resolve,%d", re.last_status());
        for (double x : re.control_results[0].u) std::printf(",%.17g", x);
        std::printf("\n");
    }

    {   // ---- part 2: feedback does not change what is published ----
        ModelControl plain(model, Q, R, Rm), fb(model, Q, R, Rm);
        const int nx = plain.model_parameters.num_x, nu = plain.model_parameters.num_u;
        const int N = plain.model_parameters.num_shooting_nodes;
        const double h = plain.model_parameters.step_size.as_seconds();
        fb.set_feedback_stages(n);
        std::vector<double> state(nx), up(nu, 0.0);
        for (int j = 0; j < nx; ++j) state[j] = 0.3 * std::sin(0.7 * j + 0.4);
        bool nofb = true;
        for (int tick = 0; tick < ticks; ++tick) {
            const double t = tick * h;
            const std::vector<double> tr = targets(nx, N, h, t, 0.0);
            plain.calc_u(mahi::util::seconds(t), state, up, tr);
            fb.calc_u(mahi::util::seconds(t), state, up, tr);
            std::printf("same,%d,%d\n", tick,
                        same_plan(plain.control_results, fb.control_results) && plain.last_status() == fb.last_status() &&
                                plain.last_iterations() == fb.last_iterations()
                            ? 1
                            : 0);
            std::vector<double> xm = state;
            for (int j = 0; j < nx; ++j) xm[j] += moved[j];
            nofb = nofb && same_result(plain.control_at_time(mahi::util::seconds(t), xm), plain.control_results[0]) &&
                   plain.feedback_status() == -1;
            up = plain.control_results[0].u;
            for (int j = 0; j < nx / 2; ++j) state[j] += h * state[nx / 2 + j];
        }
        std::printf("nofb,%d\n", nofb ? 1 : 0);
    }

    {   // ---- part 3: BatchModelControl against five ModelControl objects ----
        const int64_t B = 5;
        BatchModelControl bc(model, B, Q, R, Rm);
        std::vector<std::unique_ptr<ModelControl>> mc;
        for (int64_t b = 0; b < B; ++b) mc.emplace_back(new ModelControl(model, Q, R, Rm));
        const int nx = bc.model_parameters.num_x, nu = bc.model_parameters.num_u;
        const int N = bc.model_parameters.num_shooting_nodes;
        const double h = bc.model_parameters.step_size.as_seconds();
        bc.set_feedback_stages(n);
        for (int64_t b = 0; b < B; ++b) mc[b]->set_feedback_stages(n);
        std::vector<double> state(B * nx), control(B * nu, 0.0);
        for (int64_t b = 0; b < B; ++b)
            for (int j = 0; j < nx; ++j) state[b * nx + j] = 0.3 * std::sin(1.3 * b + 0.7 * j);
        for (int tick = 0; tick < ticks; ++tick) {
            const double t = tick * h;
            std::vector<double> trajs;
            std::vector<std::vector<double>> tr_rows;
            for (int64_t b = 0; b < B; ++b) {
                tr_rows.push_back(targets(nx, N, h, t, 0.1 * b));
                trajs.insert(trajs.end(), tr_rows.back().begin(), tr_rows.back().end());
            }
            bc.calc_u(mahi::util::seconds(t), state, control, trajs);
            std::vector<double> xm = state;
            for (int64_t b = 0; b < B; ++b)
                for (int j = 0; j < nx; ++j) xm[b * nx + j] += moved[j];
            const std::vector<double> ub = bc.controls_at_time(mahi::util::seconds(t), xm);
            const std::vector<int> gst = bc.feedback_status();
            std::vector<double> next(B * nu);
            for (int64_t b = 0; b < B; ++b) {
                const std::vector<double> xs(state.begin() + b * nx, state.begin() + (b + 1) * nx);
                const std::vector<double> us(control.begin() + b * nu, control.begin() + (b + 1) * nu);
                mc[b]->calc_u(mahi::util::seconds(t), xs, us, tr_rows[b]);
                if (tick == ticks - 1) {
                    for (int i = 0; i < n; ++i) {
                        std::printf("bg,%lld,%d,%d,%d", static_cast<long long>(b), i, gst[b], mc[b]->feedback_status());
                        for (double x : bc.feedback_gain(b, i)) std::printf(",%.17g", x);
                        for (double x : mc[b]->feedback_gain(i)) std::printf(",%.17g", x);
                        std::printf("\n");
                    }
                    const std::vector<double> xmb(xm.begin() + b * nx, xm.begin() + (b + 1) * nx);
                    std::printf("bu,%lld", static_cast<long long>(b));
                    for (int c = 0; c < nu; ++c) std::printf(",%.17g", ub[b * nu + c]);
                    for (double x : mc[b]->control_at_time(mahi::util::seconds(t), xmb).u) std::printf(",%.17g", x);
                    std::printf("\n");
                }
                for (int c = 0; c < nu; ++c) next[b * nu + c] = mc[b]->control_results[0].u[c];
            }
            control = next;
            for (int64_t b = 0; b < B; ++b)
                for (int j = 0; j < nx / 2; ++j) state[b * nx + j] += h * state[b * nx + nx / 2 + j];
        }
    }
    return 0;
}
