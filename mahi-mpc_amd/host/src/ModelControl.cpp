// ModelControl: the reference's online controller (src/Mahi/Mpc/ModelControl.cpp) with the IPOPT call
// replaced by the C-ABI of include/mmpc.h.  Packing follows ModelControl.cpp:116-172; output formatting
// :174-190; control_at_time :192-197; the async thread :75-114.
#include <Mahi/Mpc/ModelControl.hpp>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "../../../include/mmpc.h"
#include "model_library.hpp"
#include "rti_pipeline.hpp"

namespace mahi {
namespace mpc {

using detail::ModelLibrary;

ModelControl::ModelControl(std::string model_name, std::vector<double> Q, std::vector<double> R,
                           std::vector<double> Rm, Dict solver_opts)
    : m_solver_opts(solver_opts), m_Q(Q), m_R(R), m_Rm(Rm) {
    // like the reference, solver_opts are stored but not applied (ModelControl.cpp:7-11 vs :52-62)
    load_model(model_name);
}

ModelControl::~ModelControl() {
    m_stop = true;
    if (m_thread.joinable()) m_thread.join();  // the reference busy-waits on m_done_calcing (:16-19)
    m_rti.reset();                             // before its handle goes
    if (m_handle) m_backend->destroy(m_handle);
}

void ModelControl::load_model(const std::string& model_name) {
    const std::string path = model_name + ".json";  // ModelControl.cpp:24
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::stringstream ss;
    ss << f.rdbuf();
    model_parameters = model_parameters_from_json_string(ss.str());
    std::lock_guard<std::mutex> lk(m_rti_mutex);   // not under a running calc_u
    m_rti.reset();   // the pipeline belongs to the handle: a new model starts with the mode off
    m_rti_mode = false;
    if (m_handle) m_backend->destroy(m_handle);
    m_handle = nullptr;
    m_backend = ModelLibrary::load(model_parameters, path);
    m_backend->check(m_backend->create_from_json(ss.str().c_str(), nullptr, &m_handle), "mmpc_create");
    mmpc_model_info info;
    m_backend->check(m_backend->get_model_info(m_handle, &info), "mmpc_get_model_info");
    m_V.assign(static_cast<size_t>(info.num_v), 0.0);  // v_init = 0 (ModelControl.cpp:29-50)
    // the handle runs on the device that is current when it is used (mmpc_opts.device = -1); the pipeline's buffers
    // go to the one current now, when the handle is made
    if (hipGetDevice(&m_device) != hipSuccess) m_device = -1;
}

std::vector<double> ModelControl::packed_weights() {
    std::lock_guard<std::mutex> lg(m_weights_mutex);
    const size_t nx = model_parameters.num_x, nu = model_parameters.num_u;
    // the reference would hand CasADi a p of the wrong length here
    if (m_Q.size() != nx || m_R.size() != nu || m_Rm.size() != nu)
        throw std::invalid_argument("ModelControl: Q, R, Rm must have num_x, num_u, num_u entries");
    std::vector<double> w;
    w.insert(w.end(), m_Q.begin(), m_Q.end());     // ModelControl.cpp:120
    w.insert(w.end(), m_R.begin(), m_R.end());     // :121
    w.insert(w.end(), m_Rm.begin(), m_Rm.end());   // :122
    return w;
}

void ModelControl::calc_u(mahi::util::Time control_time, const std::vector<double>& state,
                          const std::vector<double>& control, std::vector<double> traj) {
    // calc_u, set_rti_mode and load_model exclude one another: the switch never sees m_V under a running solve
    std::lock_guard<std::mutex> lk(m_rti_mutex);
    curr_time = control_time;
    const size_t nx = model_parameters.num_x, nu = model_parameters.num_u, N = model_parameters.num_shooting_nodes;
    if (state.size() != nx || control.size() != nu || traj.size() != N * nx)
        throw std::invalid_argument("ModelControl::calc_u: state/control/traj size mismatch");
    if (m_rti_mode) return rti_calc_u(control_time, state, control, traj);
    const std::vector<double> w = packed_weights();
    std::vector<double> lb, ub;
    {
        std::lock_guard<std::mutex> lg(m_control_limits_mutex);  // ModelControl.cpp:148-154
        lb = model_parameters.u_min;
        ub = model_parameters.u_max;
    }
    int32_t st = -1, it = 0;
    double kkt = 0.0;
    // committed controls: the previous plan's controls for the first m instants of this horizon (none on the first call)
    std::vector<double> pin;
    if (const int m = m_num_control_inputs_saved.load()) {
        std::lock_guard<std::mutex> lg(m_output_mutex);  // ModelControl.cpp:166
        if (!control_results.empty()) {
            const double dt = control_time.as_seconds() - control_results[0].time.as_seconds();
            const long long k0 = std::llround(dt / model_parameters.step_size.as_seconds());
            for (int i = 0; i < m; ++i) {
                const long long k = std::min<long long>(static_cast<long long>(N) - 1, std::max<long long>(0, k0 + i));
                const std::vector<double>& u = control_results[static_cast<size_t>(k)].u;
                pin.insert(pin.end(), u.begin(), u.end());
            }
        }
    }
    // linear mode: the per-step linearisation at (state, control) of ModelControl.cpp:125-135 happens on the
    // device inside the solve; x_0 is pinned to `state` (ModelControl.cpp:144-145)
    if (pin.empty())
        m_backend->check(m_backend->solve_batch_host(m_handle, 1, state.data(), control.data(), traj.data(), w.data(), 0,
                                    lb.size() == nu ? lb.data() : nullptr, ub.size() == nu ? ub.data() : nullptr,
                                    m_V.data(), &st, &it, &kkt),
              "mmpc_solve_batch_host");
    else
        m_backend->check(m_backend->solve_batch_host_pinned(
                             m_handle, 1, state.data(), control.data(), traj.data(), w.data(), 0,
                             lb.size() == nu ? lb.data() : nullptr, ub.size() == nu ? ub.data() : nullptr, 0, pin.data(),
                             static_cast<int32_t>(pin.size() / nu), m_V.data(), &st, &it, &kkt),
                         "mmpc_solve_batch_host_pinned");
    m_last_status = st;
    m_last_iters = it;
    m_last_kkt = kkt;
    // feedback gains of the first n stages at the published V*, under the limits and pins of this solve
    std::vector<double> gains;
    int32_t gst = -1;
    if (const int n = m_feedback_stages.load()) {
        gains.assign(static_cast<size_t>(n) * nu * (nx + nu), 0.0);
        m_backend->check(m_backend->feedback_gains_batch_host(
                             m_handle, 1, m_V.data(), control.data(), traj.data(), w.data(), 0,
                             lb.size() == nu ? lb.data() : nullptr, ub.size() == nu ? ub.data() : nullptr, 0,
                             static_cast<int32_t>(pin.size() / nu), n, MMPC_HESSIAN_AUTO, MMPC_GAIN_KERNEL_AUTO,
                             gains.data(), &gst),
                         "mmpc_feedback_gains_batch_host");
    }
    format_outputs(m_V, std::move(gains), gst);  // m_V stays as the next warm start (ModelControl.cpp:160-161)
}

void ModelControl::set_rti_mode(bool on, double step_inf_max) {
    std::lock_guard<std::mutex> lg(m_rti_mutex);   // between ticks
    m_step_inf_max = step_inf_max;
    if (on == m_rti_mode) return;
    if (on) {
        if (!m_rti) {
            if (m_device < 0) throw std::runtime_error("set_rti_mode: no HIP device");
            m_rti = std::make_shared<detail::RtiPipeline>(m_backend, m_handle, 1, m_device);
        }
        m_rti->set_plan(m_V.data(), hipMemcpyHostToDevice);   // the warm start goes with the mode
    } else {
        m_rti->get_plan(m_V.data(), hipMemcpyDeviceToHost);
    }
    m_rti_mode = on;
}

double ModelControl::last_step_inf() {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    return m_last_step_inf;
}

// calc_u with the mode on: one tick of detail::RtiPipeline with B = 1
void ModelControl::rti_calc_u(mahi::util::Time time, const std::vector<double>& state,
                              const std::vector<double>& control, const std::vector<double>& traj) {
    const size_t nu = model_parameters.num_u;
    if (model_parameters.is_linear)
        throw std::runtime_error("real-time iteration mode: not available for a linear-mode model");
    for (const std::vector<double>* v : {&model_parameters.x_min, &model_parameters.x_max})
        for (double x : *v)
            if (std::isfinite(x))
                throw std::runtime_error("real-time iteration mode: not available with finite state limits");
    if (m_num_control_inputs_saved.load() > 0)
        throw std::runtime_error("real-time iteration mode: not available with set_num_control_inputs_saved(m > 0)");
    if (m_feedback_stages.load() > 0)
        throw std::runtime_error("real-time iteration mode: not available with set_feedback_stages(n > 0)");
    const std::vector<double> w = packed_weights();
    std::vector<double> lb, ub;
    {
        std::lock_guard<std::mutex> lg(m_control_limits_mutex);
        lb = model_parameters.u_min;
        ub = model_parameters.u_max;
    }
    detail::RtiPipeline::Inputs in;
    in.t = time.as_seconds();
    in.states = state.data();
    in.controls = control.data();
    in.trajs = traj.data();
    in.weights = w.data();
    in.lb = lb.size() == nu ? lb.data() : nullptr;   // as calc_u hands them to the solve
    in.ub = ub.size() == nu ? ub.data() : nullptr;
    in.step_inf_max = m_step_inf_max;
    const bool was_rti = m_rti->tick(in, [] {});
    m_V.assign(m_rti->plan(), m_rti->plan() + m_V.size());
    m_last_status = m_rti->status()[0];
    m_last_iters = m_rti->iterations()[0];
    m_last_kkt = 0.0;
    ++(was_rti ? m_rti_ticks : m_full_ticks);
    {
        std::lock_guard<std::mutex> lg(m_output_mutex);
        m_last_step_inf = m_rti->step_inf()[0];
    }
    format_outputs(m_V);
}

std::vector<std::vector<double>> ModelControl::calc_u_batch(const std::vector<std::vector<double>>& states,
                                                            const std::vector<std::vector<double>>& controls,
                                                            const std::vector<std::vector<double>>& trajs,
                                                            std::vector<int>* status) {
    return calc_u_batch_impl(states, controls, trajs, nullptr, nullptr, status);
}

std::vector<std::vector<double>> ModelControl::calc_u_batch(const std::vector<std::vector<double>>& states,
                                                            const std::vector<std::vector<double>>& controls,
                                                            const std::vector<std::vector<double>>& trajs,
                                                            const std::vector<std::vector<double>>& u_mins,
                                                            const std::vector<std::vector<double>>& u_maxs,
                                                            std::vector<int>* status) {
    return calc_u_batch_impl(states, controls, trajs, &u_mins, &u_maxs, status);
}

std::vector<std::vector<double>> ModelControl::calc_u_batch_impl(const std::vector<std::vector<double>>& states,
                                                                 const std::vector<std::vector<double>>& controls,
                                                                 const std::vector<std::vector<double>>& trajs,
                                                                 const std::vector<std::vector<double>>* u_mins,
                                                                 const std::vector<std::vector<double>>* u_maxs,
                                                                 std::vector<int>* status) {
    const size_t nx = model_parameters.num_x, nu = model_parameters.num_u, N = model_parameters.num_shooting_nodes;
    const size_t B = states.size();
    if (controls.size() != B || trajs.size() != B) throw std::invalid_argument("calc_u_batch: batch size mismatch");
    if (u_mins && (u_mins->size() != B || u_maxs->size() != B))
        throw std::invalid_argument("calc_u_batch: one row of control limits per instance");
    std::vector<double> x0, up, tr, V(B * m_V.size(), 0.0);
    for (size_t b = 0; b < B; ++b) {
        if (states[b].size() != nx || controls[b].size() != nu || trajs[b].size() != N * nx)
            throw std::invalid_argument("calc_u_batch: instance size mismatch");
        x0.insert(x0.end(), states[b].begin(), states[b].end());
        up.insert(up.end(), controls[b].begin(), controls[b].end());
        tr.insert(tr.end(), trajs[b].begin(), trajs[b].end());
    }
    const std::vector<double> w = packed_weights();
    std::vector<double> lb, ub;
    int64_t bounds_stride = 0;
    if (u_mins) {   // instance-major rows, bounds_stride = num_u
        for (size_t b = 0; b < B; ++b) {
            if ((*u_mins)[b].size() != nu || (*u_maxs)[b].size() != nu)
                throw std::invalid_argument("calc_u_batch: control limits need num_u entries per instance");
            lb.insert(lb.end(), (*u_mins)[b].begin(), (*u_mins)[b].end());
            ub.insert(ub.end(), (*u_maxs)[b].begin(), (*u_maxs)[b].end());
        }
        bounds_stride = static_cast<int64_t>(nu);
    } else {
        std::lock_guard<std::mutex> lg(m_control_limits_mutex);  // the limits calc_u enforces (ModelControl.cpp:148-154)
        lb = model_parameters.u_min;
        ub = model_parameters.u_max;
    }
    const size_t nb = u_mins ? B * nu : nu;   // entries a complete set of limits has
    std::vector<int32_t> st(B, -1), it(B, 0);
    std::vector<double> kkt(B, 0.0);
    m_backend->check(m_backend->solve_batch_host_bounds(
                         m_handle, static_cast<int64_t>(B), x0.data(), up.data(), tr.data(), w.data(), 0,
                         lb.size() == nb ? lb.data() : nullptr, ub.size() == nb ? ub.data() : nullptr, bounds_stride,
                         V.data(), st.data(), it.data(), kkt.data()),
                     "mmpc_solve_batch_host_bounds");
    std::vector<std::vector<double>> out(B);
    for (size_t b = 0; b < B; ++b) out[b].assign(V.begin() + b * m_V.size(), V.begin() + (b + 1) * m_V.size());
    if (status) status->assign(st.begin(), st.end());
    return out;
}

void ModelControl::format_outputs(const std::vector<double>& opt_output, std::vector<double> gains, int gain_status) {
    std::vector<ControlResult> local;
    const size_t nx = model_parameters.num_x, nu = model_parameters.num_u;
    for (size_t i = 0; i < static_cast<size_t>(model_parameters.num_shooting_nodes); i++) {
        std::vector<double> x(opt_output.begin() + i * (nx + nu), opt_output.begin() + i * (nx + nu) + nx);
        std::vector<double> u(opt_output.begin() + i * (nx + nu) + nx, opt_output.begin() + i * (nx + nu) + nx + nu);
        local.emplace_back(mahi::util::seconds(curr_time.as_seconds() + model_parameters.step_size.as_seconds() * i),
                           x, u);
    }
    std::lock_guard<std::mutex> lg(m_output_mutex);
    control_results = local;
    m_gains = std::move(gains);   // the gains travel with their plan
    m_gain_status = gain_status;
}

ModelControl::ControlResult ModelControl::control_at_time(mahi::util::Time time) {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    // the reference indexes an empty vector before the first solve (ModelControl.cpp:195); this throws instead
    if (control_results.empty()) throw std::logic_error("control_at_time before the first calc_u");
    size_t i = 0;
    while (i < control_results.size() && control_results[i].time < time) i++;
    return (i == 0) ? control_results[0] : control_results[i - 1];
}

ModelControl::ControlResult ModelControl::control_at_time(mahi::util::Time time, const std::vector<double>& x_measured) {
    const size_t nx = model_parameters.num_x, nu = model_parameters.num_u, K = nx + nu;
    if (x_measured.size() != nx) throw std::invalid_argument("control_at_time: x_measured must have num_x entries");
    std::vector<double> lo, hi;
    {
        std::lock_guard<std::mutex> lg(m_control_limits_mutex);
        lo = model_parameters.u_min;
        hi = model_parameters.u_max;
    }
    std::lock_guard<std::mutex> lg(m_output_mutex);
    if (control_results.empty()) throw std::logic_error("control_at_time before the first calc_u");
    size_t i = 0;   // ModelControl.cpp:192-197
    while (i < control_results.size() && control_results[i].time < time) i++;
    if (i > 0) --i;
    ControlResult r = control_results[i];
    if (m_gain_status == 2 || (i + 1) * nu * K > m_gains.size()) return r;   // no gains for this stage: the plan
    const double* G = m_gains.data() + i * nu * K;
    for (size_t c = 0; c < nu; ++c) {
        double u = r.u[c];
        for (size_t j = 0; j < nx; ++j) u += G[c * K + j] * (x_measured[j] - r.x_est[j]);
        if (lo.size() == nu) u = std::max(u, lo[c]);
        if (hi.size() == nu) u = std::min(u, hi[c]);
        r.u[c] = u;
    }
    return r;
}

void ModelControl::set_feedback_stages(int n) {
    if (n < 0 || n > model_parameters.num_shooting_nodes)
        throw std::invalid_argument("set_feedback_stages: n must be 0 .. num_shooting_nodes");
    m_feedback_stages = n;
}

std::vector<double> ModelControl::feedback_gain(int i) {
    const size_t sz = static_cast<size_t>(model_parameters.num_u) * (model_parameters.num_x + model_parameters.num_u);
    std::lock_guard<std::mutex> lg(m_output_mutex);
    if (i < 0 || (static_cast<size_t>(i) + 1) * sz > m_gains.size())
        throw std::out_of_range("feedback_gain: the published plan carries no gain for this stage");
    return std::vector<double>(m_gains.begin() + i * sz, m_gains.begin() + (i + 1) * sz);
}

int ModelControl::feedback_status() {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    return m_gain_status;
}

void ModelControl::set_state(mahi::util::Time time, const std::vector<double>& state,
                             const std::vector<double>& control, std::vector<double> traj) {
    std::lock_guard<std::mutex> lg(m_state_mutex);
    m_time = time;
    m_state = state;
    m_control = control;
    m_traj = traj;
}

void ModelControl::start_calc() {
    if (m_thread.joinable()) {
        m_stop = true;
        m_thread.join();
    }
    m_stop = false;
    m_done_calcing = false;
    m_thread = std::thread([this] {
        double total_ms = 0.0;
        size_t n = 0;
        while (!m_stop) {
            mahi::util::Time t;
            std::vector<double> s, c, tr;
            {
                std::lock_guard<std::mutex> lg(m_state_mutex);
                t = m_time;
                s = m_state;
                c = m_control;
                tr = m_traj;
            }
            if (s.empty()) {
                std::this_thread::yield();
                continue;
            }
            const auto t0 = std::chrono::steady_clock::now();
            calc_u(t, s, c, tr);
            total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            ++n;
        }
        if (n) std::cout << "Average calc time: " << total_ms / n << " ms" << std::endl;  // ModelControl.cpp:108
        m_done_calcing = true;
    });
}

void ModelControl::stop_calc() {
    m_stop = true;
    if (m_thread.joinable()) m_thread.join();
}

void ModelControl::update_weights(std::vector<double> Q, std::vector<double> R, std::vector<double> Rm) {
    std::lock_guard<std::mutex> lg(m_weights_mutex);
    if (!Q.empty()) m_Q = Q;
    if (!R.empty()) m_R = R;
    if (!Rm.empty()) m_Rm = Rm;
}

void ModelControl::update_control_limits(std::vector<double> u_min, std::vector<double> u_max) {
    std::lock_guard<std::mutex> lg(m_control_limits_mutex);
    model_parameters.u_min = u_min;
    model_parameters.u_max = u_max;
}

void ModelControl::set_num_control_inputs_saved(int m) {
    if (m < 0 || m > model_parameters.num_shooting_nodes - 1)
        throw std::invalid_argument("set_num_control_inputs_saved: m must be 0 .. num_shooting_nodes - 1");
    m_num_control_inputs_saved = m;
}

void ModelControl::set_sensitivity_barrier(double mu, double sigma_cap) {
    double dmu = 0.0, dcap = 0.0;
    m_backend->check(m_backend->sensitivity_barrier_default(&dmu, &dcap), "mmpc_sensitivity_barrier_default");
    m_backend->check(
        m_backend->set_sensitivity_barrier(m_handle, mu < 0.0 ? dmu : mu, sigma_cap > 0.0 ? sigma_cap : dcap),
        "mmpc_set_sensitivity_barrier");
}

void ModelControl::set_barrier_rule(int rule) {
    m_backend->check(m_backend->set_barrier_rule(m_handle, rule), "mmpc_set_barrier_rule");
}

}  // namespace mpc
}  // namespace mahi
