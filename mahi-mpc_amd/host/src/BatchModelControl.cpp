// BatchModelControl: ModelControl's online loop (ModelControl.cpp:75-197) for B instances per GPU solve, with the
// warm start resident in HBM and the host<->device staging double-buffered on a copy stream (see the header).
#include <Mahi/Mpc/BatchModelControl.hpp>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "../../../include/mmpc.h"
#include "model_library.hpp"
#include "rti_pipeline.hpp"

namespace mahi {
namespace mpc {

namespace {
void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPC(call) hip_check((call), #call)
}  // namespace

struct BatchModelControl::Impl {
    std::shared_ptr<detail::ModelLibrary> lib;
    mmpc_handle* h = nullptr;
    int dev = -1;
    hipStream_t compute = nullptr, copy = nullptr;
    int nx = 0, nu = 0, N = 0, NV = 0;
    double step = 0.0;
    int64_t B = 0;
    // per-slot input block (device and pinned host): x0 [B nx] | u_prev [B nu] | traj [B N nx] | Q R Rm | lb | ub |
    // lb table [B nu] | ub table [B nu] (per-instance limits: uploaded, in the same single H2D, only while in use)
    // | committed controls [B m nu], packed right after whatever else the tick uploads (no gap, one H2D)
    size_t off_up = 0, off_tr = 0, off_w = 0, off_lb = 0, off_ub = 0, off_lbt = 0, off_ubt = 0, in_doubles = 0;
    size_t slot_doubles = 0;  // in_doubles + the largest pin table, B (N - 1) nu
    double* d_in[2] = {nullptr, nullptr};
    double* h_in[2] = {nullptr, nullptr};
    bool bounded[2] = {false, false};
    // solution: resident warm start, per-slot copies for the download, per-slot status/iterations
    double* d_V = nullptr;
    double* d_tmp = nullptr;  // warm-start shift
    double* d_Vout[2] = {nullptr, nullptr};
    int32_t* d_st[2] = {nullptr, nullptr};
    int32_t* d_it[2] = {nullptr, nullptr};
    double* h_V[2] = {nullptr, nullptr};
    int32_t* h_st[2] = {nullptr, nullptr};
    int32_t* h_it[2] = {nullptr, nullptr};
    // feedback gains (set_feedback_stages): per-slot device and pinned host buffers for N stages, allocated at the
    // first call that turns feedback on; fb[slot] = stages the slot's tick computed
    double* d_G[2] = {nullptr, nullptr};
    double* h_G[2] = {nullptr, nullptr};
    int32_t* d_gst[2] = {nullptr, nullptr};
    int32_t* h_gst[2] = {nullptr, nullptr};
    int fb[2] = {0, 0};
    hipEvent_t h2d_done[2] = {nullptr, nullptr}, solved[2] = {nullptr, nullptr}, d2h_done[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    mahi::util::Time pend_time[2];
    std::chrono::steady_clock::time_point pend_t0[2];
    int next_slot = 0;
    bool have_prev = false;
    mahi::util::Time prev_time;

    std::unique_ptr<detail::RtiPipeline> rti;   // real-time iteration mode: allocated at the first set_rti_mode(true)

    void check(int rc, const char* what) const { lib->check(rc, what); }
};

BatchModelControl::BatchModelControl(std::string model_name, int64_t B, std::vector<double> Q, std::vector<double> R,
                                     std::vector<double> Rm, Dict solver_opts, int device)
    : m(new Impl), m_B(B), m_Q(std::move(Q)), m_R(std::move(R)), m_Rm(std::move(Rm)) {
    (void)solver_opts;  // stored-but-ignored in the reference (ModelControl.cpp:7-11 vs :52-62)
    if (B < 1) throw std::invalid_argument("BatchModelControl: B must be >= 1");
    const std::string path = model_name + ".json";
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::stringstream ss;
    ss << f.rdbuf();
    model_parameters = model_parameters_from_json_string(ss.str());
    m->lib = detail::ModelLibrary::load(model_parameters, path);
    mmpc_opts o;
    mmpc_default_opts(&o);
    o.device = device;
    m->check(m->lib->create_from_json(ss.str().c_str(), &o, &m->h), "mmpc_create");
    mmpc_model_info info;
    m->check(m->lib->get_model_info(m->h, &info), "mmpc_get_model_info");
    m->nx = info.num_x;
    m->nu = info.num_u;
    m->N = info.num_shooting_nodes;
    m->NV = info.num_v;
    m->step = info.step_size;
    m->B = B;
    if (m_Q.size() != static_cast<size_t>(m->nx) || m_R.size() != static_cast<size_t>(m->nu) ||
        m_Rm.size() != static_cast<size_t>(m->nu))
        throw std::invalid_argument("BatchModelControl: Q, R, Rm must have num_x, num_u, num_u entries");
    if (device >= 0) HIPC(hipSetDevice(device));
    HIPC(hipGetDevice(&m->dev));
    const size_t nx = m->nx, nu = m->nu, N = m->N, NV = m->NV, b = static_cast<size_t>(B);
    m->off_up = b * nx;
    m->off_tr = m->off_up + b * nu;
    m->off_w = m->off_tr + b * N * nx;
    m->off_lb = m->off_w + nx + 2 * nu;
    m->off_ub = m->off_lb + nu;
    m->off_lbt = m->off_ub + nu;
    m->off_ubt = m->off_lbt + b * nu;
    m->in_doubles = m->off_ubt + b * nu;
    m->slot_doubles = m->in_doubles + b * (N > 1 ? N - 1 : 0) * nu;
    HIPC(hipStreamCreateWithFlags(&m->compute, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&m->copy, hipStreamNonBlocking));
    HIPC(hipMalloc(reinterpret_cast<void**>(&m->d_V), b * NV * sizeof(double)));
    HIPC(hipMemset(m->d_V, 0, b * NV * sizeof(double)));  // v_init = 0 (ModelControl.cpp:29-50)
    HIPC(hipMalloc(reinterpret_cast<void**>(&m->d_tmp), b * NV * sizeof(double)));
    for (int s = 0; s < 2; ++s) {
        HIPC(hipMalloc(reinterpret_cast<void**>(&m->d_in[s]), m->slot_doubles * sizeof(double)));
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&m->h_in[s]), m->slot_doubles * sizeof(double), hipHostMallocDefault));
        HIPC(hipMalloc(reinterpret_cast<void**>(&m->d_Vout[s]), b * NV * sizeof(double)));
        HIPC(hipMalloc(reinterpret_cast<void**>(&m->d_st[s]), b * sizeof(int32_t)));
        HIPC(hipMalloc(reinterpret_cast<void**>(&m->d_it[s]), b * sizeof(int32_t)));
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&m->h_V[s]), b * NV * sizeof(double), hipHostMallocDefault));
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&m->h_st[s]), b * sizeof(int32_t), hipHostMallocDefault));
        HIPC(hipHostMalloc(reinterpret_cast<void**>(&m->h_it[s]), b * sizeof(int32_t), hipHostMallocDefault));
        HIPC(hipEventCreateWithFlags(&m->h2d_done[s], hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&m->solved[s], hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&m->d2h_done[s], hipEventDisableTiming));
    }
    // the Riccati solvers' workspace up front: solves never allocate (and never synchronise) inside the loop
    m->check(m->lib->reserve_workspace(m->h, B, nullptr), "mmpc_reserve_workspace");
    m_out_V.assign(b * NV, 0.0);
    m_out_status.assign(b, -1);
    m_out_iters.assign(b, 0);
}

BatchModelControl::~BatchModelControl() {
    stop_calc();
    if (!m) return;
    (void)hipSetDevice(m->dev);
    if (m->compute) (void)hipStreamSynchronize(m->compute);
    if (m->copy) (void)hipStreamSynchronize(m->copy);
    for (int s = 0; s < 2; ++s) {
        (void)hipFree(m->d_in[s]);
        (void)hipHostFree(m->h_in[s]);
        (void)hipFree(m->d_Vout[s]);
        (void)hipFree(m->d_st[s]);
        (void)hipFree(m->d_it[s]);
        (void)hipHostFree(m->h_V[s]);
        (void)hipHostFree(m->h_st[s]);
        (void)hipHostFree(m->h_it[s]);
        (void)hipFree(m->d_G[s]);
        (void)hipHostFree(m->h_G[s]);
        (void)hipFree(m->d_gst[s]);
        (void)hipHostFree(m->h_gst[s]);
        if (m->h2d_done[s]) (void)hipEventDestroy(m->h2d_done[s]);
        if (m->solved[s]) (void)hipEventDestroy(m->solved[s]);
        if (m->d2h_done[s]) (void)hipEventDestroy(m->d2h_done[s]);
    }
    (void)hipFree(m->d_V);
    (void)hipFree(m->d_tmp);
    m->rti.reset();
    if (m->h) m->lib->destroy(m->h);
    if (m->compute) (void)hipStreamDestroy(m->compute);
    if (m->copy) (void)hipStreamDestroy(m->copy);
}

void BatchModelControl::enqueue_tick(int slot, mahi::util::Time time, const double* states, const double* controls,
                                     const double* trajs) {
    Impl& I = *m;
    HIPC(hipSetDevice(I.dev));
    if (I.pending[slot]) publish(slot);  // the slot's pinned buffers are free again
    const size_t nx = I.nx, nu = I.nu, N = I.N, NV = I.NV, b = static_cast<size_t>(I.B);
    double* in = I.h_in[slot];
    std::memcpy(in, states, b * nx * sizeof(double));
    std::memcpy(in + I.off_up, controls, b * nu * sizeof(double));
    std::memcpy(in + I.off_tr, trajs, b * N * nx * sizeof(double));
    {
        std::lock_guard<std::mutex> lg(m_weights_mutex);  // ModelControl.cpp:120-122
        std::copy(m_Q.begin(), m_Q.end(), in + I.off_w);
        std::copy(m_R.begin(), m_R.end(), in + I.off_w + nx);
        std::copy(m_Rm.begin(), m_Rm.end(), in + I.off_w + nx + nu);
    }
    bool finite = false, per_instance = false;
    {
        // the limits of this tick are those in force now, when it is enqueued: a later update_control_limits changes
        // the next tick, never a solve already queued (ModelControl.cpp:148-154 reads them under this mutex per tick)
        std::lock_guard<std::mutex> lg(m_control_limits_mutex);
        per_instance = m_limits_per_instance;
        if (per_instance) {
            std::copy(m_u_min_table.begin(), m_u_min_table.end(), in + I.off_lbt);
            std::copy(m_u_max_table.begin(), m_u_max_table.end(), in + I.off_ubt);
            for (size_t i = 0; i < b * nu; ++i) finite |= m_u_min_table[i] > -1e19 || m_u_max_table[i] < 1e19;
        }
        for (size_t c = 0; c < nu; ++c) {
            const double lo = c < model_parameters.u_min.size() ? model_parameters.u_min[c] : -10e30;
            const double hi = c < model_parameters.u_max.size() ? model_parameters.u_max[c] : 10e30;
            in[I.off_lb + c] = lo;
            in[I.off_ub + c] = hi;
            if (!per_instance) finite |= lo > -1e19 || hi < 1e19;  // IPOPT: |bound| >= 1e19 is infinite
        }
    }
    I.bounded[slot] = finite;
    double* d = I.d_in[slot];
    // one H2D per tick: the per-instance tables lie at the end of the slot and travel only while they are in use
    size_t up_doubles = per_instance ? I.in_doubles : I.off_lbt;
    // committed controls: per instance, the published plan's controls for the first n_pin instants of this horizon
    // (index clamp(round((t - t_published) / step) + i, 0, N - 1), the warm-start shift's rule), packed after the
    // rest of the upload; nothing is pinned before a plan has been published
    const int want_pin = m_num_control_inputs_saved.load();
    int32_t n_pin = 0;
    const size_t off_pin = up_doubles;
    if (want_pin > 0) {
        std::lock_guard<std::mutex> lg(m_output_mutex);
        if (m_ticks > 0) {
            n_pin = want_pin;
            const int64_t k0 = std::llround((time.as_seconds() - m_out_time.as_seconds()) / I.step);
            for (size_t i = 0; i < b; ++i)
                for (int s = 0; s < n_pin; ++s) {
                    const size_t k = static_cast<size_t>(std::min<int64_t>(I.N - 1, std::max<int64_t>(0, k0 + s)));
                    const double* u = m_out_V.data() + i * NV + k * (nx + nu) + nx;
                    std::copy(u, u + nu, in + off_pin + (i * n_pin + s) * nu);
                }
            up_doubles += b * n_pin * nu;
        }
    }
    HIPC(hipMemcpyAsync(d, in, up_doubles * sizeof(double), hipMemcpyHostToDevice, I.copy));
    HIPC(hipEventRecord(I.h2d_done[slot], I.copy));
    HIPC(hipStreamWaitEvent(I.compute, I.h2d_done[slot], 0));
    if (m_shift && I.have_prev) {  // warm start moved k stages earlier (the tail keeps its old values)
        const double dt = time.as_seconds() - I.prev_time.as_seconds();
        const int64_t k = std::min<int64_t>(I.N, std::max<int64_t>(0, std::llround(dt / I.step)));
        if (k > 0) {
            const size_t sh = static_cast<size_t>(k) * (nx + nu), w = (NV - sh) * sizeof(double);
            HIPC(hipMemcpy2DAsync(I.d_tmp, NV * sizeof(double), I.d_V + sh, NV * sizeof(double), w, b,
                                  hipMemcpyDeviceToDevice, I.compute));
            HIPC(hipMemcpy2DAsync(I.d_V, NV * sizeof(double), I.d_tmp, NV * sizeof(double), w, b,
                                  hipMemcpyDeviceToDevice, I.compute));
        }
    }
    I.have_prev = true;
    I.prev_time = time;
    const size_t olb = per_instance ? I.off_lbt : I.off_lb, oub = per_instance ? I.off_ubt : I.off_ub;
    if (n_pin == 0)
        I.check(I.lib->solve_batch_bounds(I.h, I.B, d, d + I.off_up, d + I.off_tr, d + I.off_w, 0,
                                          finite ? d + olb : nullptr, finite ? d + oub : nullptr,
                                          per_instance ? static_cast<int64_t>(nu) : 0, I.d_V, I.d_st[slot],
                                          I.d_it[slot], nullptr, nullptr, I.compute),
                "mmpc_solve_batch_bounds");
    else
        I.check(I.lib->solve_batch_pinned(I.h, I.B, d, d + I.off_up, d + I.off_tr, d + I.off_w, 0,
                                          finite ? d + olb : nullptr, finite ? d + oub : nullptr,
                                          per_instance ? static_cast<int64_t>(nu) : 0, d + off_pin, n_pin, I.d_V,
                                          I.d_st[slot], I.d_it[slot], nullptr, nullptr, I.compute),
                "mmpc_solve_batch_pinned");
    // feedback gains at the solution, behind the solve on the tick's stream, with the tick's limits and pins
    const int n_fb = m_feedback_stages.load();
    I.fb[slot] = n_fb;
    if (n_fb > 0)
        I.check(I.lib->feedback_gains_batch(I.h, I.B, I.d_V, d + I.off_up, d + I.off_tr, d + I.off_w, 0,
                                            finite ? d + olb : nullptr, finite ? d + oub : nullptr,
                                            per_instance ? static_cast<int64_t>(nu) : 0, n_pin, n_fb, MMPC_HESSIAN_AUTO,
                                            MMPC_GAIN_KERNEL_AUTO, I.d_G[slot], I.d_gst[slot], I.compute),
                "mmpc_feedback_gains_batch");
    // the next solve updates d_V in place: download from a per-slot copy
    HIPC(hipMemcpyAsync(I.d_Vout[slot], I.d_V, b * NV * sizeof(double), hipMemcpyDeviceToDevice, I.compute));
    HIPC(hipEventRecord(I.solved[slot], I.compute));
    HIPC(hipStreamWaitEvent(I.copy, I.solved[slot], 0));
    HIPC(hipMemcpyAsync(I.h_V[slot], I.d_Vout[slot], b * NV * sizeof(double), hipMemcpyDeviceToHost, I.copy));
    HIPC(hipMemcpyAsync(I.h_st[slot], I.d_st[slot], b * sizeof(int32_t), hipMemcpyDeviceToHost, I.copy));
    HIPC(hipMemcpyAsync(I.h_it[slot], I.d_it[slot], b * sizeof(int32_t), hipMemcpyDeviceToHost, I.copy));
    if (n_fb > 0) {   // the gains travel in the slot's download with the solution
        HIPC(hipMemcpyAsync(I.h_G[slot], I.d_G[slot], b * n_fb * nu * (nx + nu) * sizeof(double), hipMemcpyDeviceToHost,
                            I.copy));
        HIPC(hipMemcpyAsync(I.h_gst[slot], I.d_gst[slot], b * sizeof(int32_t), hipMemcpyDeviceToHost, I.copy));
    }
    HIPC(hipEventRecord(I.d2h_done[slot], I.copy));
    I.pending[slot] = true;
    I.pend_time[slot] = time;
}

void BatchModelControl::publish(int slot) {
    Impl& I = *m;
    if (!I.pending[slot]) return;
    HIPC(hipEventSynchronize(I.d2h_done[slot]));
    const size_t b = static_cast<size_t>(I.B);
    {
        std::lock_guard<std::mutex> lg(m_output_mutex);  // ModelControl.cpp:174-190
        std::memcpy(m_out_V.data(), I.h_V[slot], b * I.NV * sizeof(double));
        for (size_t i = 0; i < b; ++i) {
            m_out_status[i] = I.h_st[slot][i];
            m_out_iters[i] = I.h_it[slot][i];
        }
        m_out_time = I.pend_time[slot];
        m_out_fb = I.fb[slot];
        if (m_out_fb > 0) {
            m_out_G.assign(I.h_G[slot], I.h_G[slot] + b * m_out_fb * I.nu * (I.nx + I.nu));
            m_out_gst.assign(I.h_gst[slot], I.h_gst[slot] + b);
        } else {
            m_out_G.clear();
            m_out_gst.clear();
        }
    }
    m_tick_ms_sum += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - I.pend_t0[slot]).count();
    I.pending[slot] = false;
    ++m_ticks;
}

void BatchModelControl::calc_u(mahi::util::Time time, const std::vector<double>& states,
                               const std::vector<double>& controls, const std::vector<double>& trajs) {
    const size_t b = static_cast<size_t>(m_B);
    if (states.size() != b * m->nx || controls.size() != b * m->nu || trajs.size() != b * m->N * m->nx)
        throw std::invalid_argument("BatchModelControl::calc_u: states/controls/trajs size mismatch");
    std::lock_guard<std::mutex> lg(m_solve_mutex);
    if (m_rti_mode) return rti_tick(time, states.data(), controls.data(), trajs.data());
    const int slot = m->next_slot;
    m->next_slot ^= 1;
    m->pend_t0[slot] = std::chrono::steady_clock::now();
    enqueue_tick(slot, time, states.data(), controls.data(), trajs.data());
    publish(slot ^ 1);
    publish(slot);
}

void BatchModelControl::set_rti_mode(bool on, double step_inf_max) {
    std::lock_guard<std::mutex> lg(m_solve_mutex);   // between ticks
    Impl& I = *m;
    HIPC(hipSetDevice(I.dev));
    publish(I.next_slot);   // nothing of the pipelined path stays in flight across the switch
    publish(I.next_slot ^ 1);
    HIPC(hipStreamSynchronize(I.compute));
    m_step_inf_max = step_inf_max;
    if (on == m_rti_mode) return;
    if (on) {
        if (!I.rti) I.rti.reset(new detail::RtiPipeline(I.lib, I.h, I.B, I.dev));
        I.rti->set_plan(I.d_V, hipMemcpyDeviceToDevice);   // the warm start goes with the mode
    } else {
        I.rti->get_plan(I.d_V, hipMemcpyDeviceToDevice);
        I.have_prev = false;
    }
    m_rti_mode = on;
}

void BatchModelControl::set_next_targets(const std::vector<double>& trajs_next) {
    if (trajs_next.size() != static_cast<size_t>(m_B) * m->N * m->nx)
        throw std::invalid_argument("set_next_targets: trajs_next must have B * num_shooting_nodes * num_x entries");
    std::lock_guard<std::mutex> lg(m_state_mutex);
    m_next_targets = trajs_next;
    m_have_next_targets = true;
}

std::vector<double> BatchModelControl::last_step_inf() {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    return m_out_step_inf;
}

double BatchModelControl::mean_feedback_latency_ms() const { return m_rti_ticks ? m_fb_ms_sum / m_rti_ticks : 0.0; }

// One tick with the mode on (under m_solve_mutex): detail::RtiPipeline decides between a full and an RTI tick.
void BatchModelControl::rti_tick(mahi::util::Time time, const double* states, const double* controls,
                                 const double* trajs) {
    Impl& I = *m;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t nx = I.nx, nu = I.nu, b = static_cast<size_t>(I.B);
    if (model_parameters.is_linear) throw std::runtime_error("real-time iteration mode: not available for a linear-mode model");
    for (double v : model_parameters.x_min)
        if (std::isfinite(v)) throw std::runtime_error("real-time iteration mode: not available with finite state limits");
    for (double v : model_parameters.x_max)
        if (std::isfinite(v)) throw std::runtime_error("real-time iteration mode: not available with finite state limits");
    if (m_num_control_inputs_saved.load() > 0)
        throw std::runtime_error("real-time iteration mode: not available with set_num_control_inputs_saved(m > 0)");
    if (m_feedback_stages.load() > 0)
        throw std::runtime_error("real-time iteration mode: not available with set_feedback_stages(n > 0)");
    std::vector<double> w, lb, ub, next;
    {
        std::lock_guard<std::mutex> lg(m_weights_mutex);
        w.insert(w.end(), m_Q.begin(), m_Q.end());
        w.insert(w.end(), m_R.begin(), m_R.end());
        w.insert(w.end(), m_Rm.begin(), m_Rm.end());
    }
    bool finite = false, per_instance = false;
    {
        // the limits in force now, by the rules of enqueue_tick
        std::lock_guard<std::mutex> lg(m_control_limits_mutex);
        per_instance = m_limits_per_instance;
        if (per_instance) {
            lb = m_u_min_table;
            ub = m_u_max_table;
            for (size_t i = 0; i < b * nu; ++i) finite |= lb[i] > -1e19 || ub[i] < 1e19;
        } else {
            lb.resize(nu);
            ub.resize(nu);
            for (size_t c = 0; c < nu; ++c) {
                lb[c] = c < model_parameters.u_min.size() ? model_parameters.u_min[c] : -10e30;
                ub[c] = c < model_parameters.u_max.size() ? model_parameters.u_max[c] : 10e30;
                finite |= lb[c] > -1e19 || ub[c] < 1e19;
            }
        }
    }
    {
        std::lock_guard<std::mutex> lg(m_state_mutex);
        if (m_have_next_targets) next.swap(m_next_targets);
        m_have_next_targets = false;
    }
    detail::RtiPipeline::Inputs in;
    in.t = time.as_seconds();
    in.states = states;
    in.controls = controls;
    in.trajs = trajs;
    in.next_trajs = next.empty() ? nullptr : next.data();
    in.weights = w.data();
    in.lb = finite ? lb.data() : nullptr;
    in.ub = finite ? ub.data() : nullptr;
    in.per_instance = per_instance;
    in.step_inf_max = m_step_inf_max;
    double u0_ms = 0.0;
    bool was_rti = false;
    try {
        was_rti = I.rti->tick(in, [&] {
        // u_0 ahead of its plan: control_at_time serves it for the tick's first interval until the plan lands
        std::lock_guard<std::mutex> lg(m_output_mutex);
        m_u0_x.assign(states, states + b * nx);
        m_u0_u.assign(I.rti->u0(), I.rti->u0() + b * nu);
        m_u0_time = time;
        m_u0_ahead = true;
        u0_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        });
    } catch (...) {   // the plan of that u_0 never lands: control_at_time goes back to the last published plan
        std::lock_guard<std::mutex> lg(m_output_mutex);
        m_u0_ahead = false;
        throw;
    }
    {
        std::lock_guard<std::mutex> lg(m_output_mutex);
        std::memcpy(m_out_V.data(), I.rti->plan(), b * I.NV * sizeof(double));
        m_out_status = I.rti->status();
        m_out_iters = I.rti->iterations();
        m_out_step_inf.assign(I.rti->step_inf(), I.rti->step_inf() + b);
        m_out_time = time;
        m_out_fb = 0;
        m_out_G.clear();
        m_out_gst.clear();
        m_u0_ahead = false;
    }
    if (was_rti) {
        m_fb_ms_sum += u0_ms;
        ++m_rti_ticks;
    } else {
        ++m_full_ticks;
    }
    m_tick_ms_sum += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ++m_ticks;
}

void BatchModelControl::set_state(mahi::util::Time time, const std::vector<double>& states,
                                  const std::vector<double>& controls, const std::vector<double>& trajs) {
    const size_t b = static_cast<size_t>(m_B);
    if (states.size() != b * m->nx || controls.size() != b * m->nu || trajs.size() != b * m->N * m->nx)
        throw std::invalid_argument("BatchModelControl::set_state: states/controls/trajs size mismatch");
    {
        std::lock_guard<std::mutex> lg(m_state_mutex);
        m_time = time;
        m_states = states;
        m_controls = controls;
        m_trajs = trajs;
        ++m_state_version;
    }
    m_state_cv.notify_one();
}

void BatchModelControl::worker() {
    uint64_t seen = 0;
    std::vector<double> s, c, tr;
    while (!m_stop) {
        mahi::util::Time t;
        {
            std::unique_lock<std::mutex> lk(m_state_mutex);
            m_state_cv.wait_for(lk, std::chrono::milliseconds(1), [&] { return m_stop || m_state_version != seen; });
            if (m_stop) break;
            if (m_state_version == seen) continue;
            seen = m_state_version;
            t = m_time;
            s = m_states;
            c = m_controls;
            tr = m_trajs;
        }
        std::lock_guard<std::mutex> lg(m_solve_mutex);
        if (m_rti_mode) {
            rti_tick(t, s.data(), c.data(), tr.data());
            continue;
        }
        const int slot = m->next_slot;
        m->next_slot ^= 1;
        m->pend_t0[slot] = std::chrono::steady_clock::now();
        enqueue_tick(slot, t, s.data(), c.data(), tr.data());
        // the previous tick's results are published while this tick's solve is queued behind it on the GPU
        publish(slot ^ 1);
    }
    std::lock_guard<std::mutex> lg(m_solve_mutex);
    publish(m->next_slot ^ 1);
    publish(m->next_slot);
}

void BatchModelControl::start_calc() {
    stop_calc();
    m_stop = false;
    m_thread = std::thread([this] { worker(); });
}

void BatchModelControl::stop_calc() {
    m_stop = true;
    m_state_cv.notify_all();
    if (m_thread.joinable()) m_thread.join();
}

BatchModelControl::ControlResult BatchModelControl::control_at_time(int64_t b, mahi::util::Time time) {
    if (b < 0 || b >= m_B) throw std::out_of_range("control_at_time: instance index");
    std::lock_guard<std::mutex> lg(m_output_mutex);
    const size_t nx = m->nx, nu = m->nu, N = m->N;
    if (m_u0_ahead) {   // an RTI tick's u_0, published before its plan: it serves the tick's first interval
        const bool first = !(mahi::util::seconds(m_u0_time.as_seconds() + m->step) < time);
        if (first || m_ticks == 0)
            return ControlResult(m_u0_time, std::vector<double>(m_u0_x.begin() + b * nx, m_u0_x.begin() + (b + 1) * nx),
                                 std::vector<double>(m_u0_u.begin() + b * nu, m_u0_u.begin() + (b + 1) * nu));
    }
    if (m_ticks == 0) throw std::logic_error("control_at_time before the first solve");
    // ModelControl.cpp:192-197: the last stage whose time is before `time` (the first one if none)
    size_t i = 0;
    while (i < N && mahi::util::seconds(m_out_time.as_seconds() + m->step * i) < time) i++;
    const size_t k = i == 0 ? 0 : i - 1;
    const double* v = m_out_V.data() + static_cast<size_t>(b) * m->NV + k * (nx + nu);
    return ControlResult(mahi::util::seconds(m_out_time.as_seconds() + m->step * k), std::vector<double>(v, v + nx),
                         std::vector<double>(v + nx, v + nx + nu));
}

std::vector<double> BatchModelControl::controls_at_time(mahi::util::Time time) {
    std::vector<double> out;
    out.reserve(static_cast<size_t>(m_B) * m->nu);
    for (int64_t b = 0; b < m_B; ++b) {
        const ControlResult r = control_at_time(b, time);
        out.insert(out.end(), r.u.begin(), r.u.end());
    }
    return out;
}

std::vector<double> BatchModelControl::controls_at_time(mahi::util::Time time, const std::vector<double>& states_measured) {
    const size_t nx = m->nx, nu = m->nu, K = nx + nu, N = m->N, B = static_cast<size_t>(m_B);
    if (states_measured.size() != B * nx)
        throw std::invalid_argument("controls_at_time: states_measured must have B * num_x entries");
    std::vector<double> lo(B * nu, -INFINITY), hi(B * nu, INFINITY);
    {
        std::lock_guard<std::mutex> lg(m_control_limits_mutex);
        for (size_t b = 0; b < B; ++b)
            for (size_t c = 0; c < nu; ++c) {
                if (m_limits_per_instance) {
                    lo[b * nu + c] = m_u_min_table[b * nu + c];
                    hi[b * nu + c] = m_u_max_table[b * nu + c];
                } else {
                    if (c < model_parameters.u_min.size()) lo[b * nu + c] = model_parameters.u_min[c];
                    if (c < model_parameters.u_max.size()) hi[b * nu + c] = model_parameters.u_max[c];
                }
            }
    }
    std::lock_guard<std::mutex> lg(m_output_mutex);
    if (m_ticks == 0) throw std::logic_error("controls_at_time before the first solve");
    size_t i = 0;   // ModelControl.cpp:192-197
    while (i < N && mahi::util::seconds(m_out_time.as_seconds() + m->step * i) < time) i++;
    const size_t k = i == 0 ? 0 : i - 1;
    std::vector<double> out(B * nu);
    for (size_t b = 0; b < B; ++b) {
        const double* v = m_out_V.data() + b * m->NV + k * K;
        const bool fb = k < static_cast<size_t>(m_out_fb) && m_out_gst[b] != 2;
        const double* G = fb ? m_out_G.data() + (b * m_out_fb + k) * nu * K : nullptr;
        for (size_t c = 0; c < nu; ++c) {
            double u = v[nx + c];
            if (fb) {
                for (size_t j = 0; j < nx; ++j) u += G[c * K + j] * (states_measured[b * nx + j] - v[j]);
                u = std::min(std::max(u, lo[b * nu + c]), hi[b * nu + c]);
            }
            out[b * nu + c] = u;
        }
    }
    return out;
}

void BatchModelControl::set_feedback_stages(int n) {
    if (n < 0 || n > m->N) throw std::invalid_argument("set_feedback_stages: n must be 0 .. num_shooting_nodes");
    std::lock_guard<std::mutex> lg(m_solve_mutex);   // between ticks
    Impl& I = *m;
    if (n > 0 && !I.d_G[0]) {
        HIPC(hipSetDevice(I.dev));
        const size_t g = static_cast<size_t>(I.B) * I.N * I.nu * (I.nx + I.nu) * sizeof(double);
        for (int s = 0; s < 2; ++s) {
            HIPC(hipMalloc(reinterpret_cast<void**>(&I.d_G[s]), g));
            HIPC(hipHostMalloc(reinterpret_cast<void**>(&I.h_G[s]), g, hipHostMallocDefault));
            HIPC(hipMalloc(reinterpret_cast<void**>(&I.d_gst[s]), I.B * sizeof(int32_t)));
            HIPC(hipHostMalloc(reinterpret_cast<void**>(&I.h_gst[s]), I.B * sizeof(int32_t), hipHostMallocDefault));
        }
    }
    m_feedback_stages = n;
}

std::vector<double> BatchModelControl::feedback_gain(int64_t b, int i) {
    if (b < 0 || b >= m_B) throw std::out_of_range("feedback_gain: instance index");
    const size_t sz = static_cast<size_t>(m->nu) * (m->nx + m->nu);
    std::lock_guard<std::mutex> lg(m_output_mutex);
    if (i < 0 || i >= m_out_fb) throw std::out_of_range("feedback_gain: the published tick carries no gain for this stage");
    const double* G = m_out_G.data() + (static_cast<size_t>(b) * m_out_fb + i) * sz;
    return std::vector<double>(G, G + sz);
}

std::vector<int> BatchModelControl::feedback_status() {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    return m_out_gst;
}

std::vector<double> BatchModelControl::solution(int64_t b) {
    if (b < 0 || b >= m_B) throw std::out_of_range("solution: instance index");
    std::lock_guard<std::mutex> lg(m_output_mutex);
    const double* v = m_out_V.data() + static_cast<size_t>(b) * m->NV;
    return std::vector<double>(v, v + m->NV);
}

std::vector<int> BatchModelControl::last_status() {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    return m_out_status;
}

std::vector<int> BatchModelControl::last_iterations() {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    return m_out_iters;
}

mahi::util::Time BatchModelControl::last_solve_time() {
    std::lock_guard<std::mutex> lg(m_output_mutex);
    return m_out_time;
}

double BatchModelControl::mean_tick_ms() const { return m_ticks ? m_tick_ms_sum / m_ticks : 0.0; }

void BatchModelControl::update_weights(std::vector<double> Q, std::vector<double> R, std::vector<double> Rm) {
    std::lock_guard<std::mutex> lg(m_weights_mutex);
    if (!Q.empty()) {
        if (Q.size() != m_Q.size()) throw std::invalid_argument("update_weights: Q size");
        m_Q = Q;
    }
    if (!R.empty()) {
        if (R.size() != m_R.size()) throw std::invalid_argument("update_weights: R size");
        m_R = R;
    }
    if (!Rm.empty()) {
        if (Rm.size() != m_Rm.size()) throw std::invalid_argument("update_weights: Rm size");
        m_Rm = Rm;
    }
}

void BatchModelControl::update_control_limits(std::vector<double> u_min, std::vector<double> u_max) {
    std::lock_guard<std::mutex> lg(m_control_limits_mutex);
    model_parameters.u_min = u_min;
    model_parameters.u_max = u_max;
    m_limits_per_instance = false;   // all instances: back to the one shared box
}

void BatchModelControl::update_control_limits(int64_t b, std::vector<double> u_min, std::vector<double> u_max) {
    if (b < 0 || b >= m_B) throw std::out_of_range("update_control_limits: instance index");
    const size_t nu = m->nu;
    if (u_min.size() != nu || u_max.size() != nu)
        throw std::invalid_argument("update_control_limits: u_min, u_max must have num_u entries");
    std::lock_guard<std::mutex> lg(m_control_limits_mutex);
    if (!m_limits_per_instance) {   // every instance starts from the shared limits (ModelControl.cpp:37-50)
        m_u_min_table.resize(static_cast<size_t>(m_B) * nu);
        m_u_max_table.resize(static_cast<size_t>(m_B) * nu);
        for (size_t i = 0; i < static_cast<size_t>(m_B); ++i)
            for (size_t c = 0; c < nu; ++c) {
                m_u_min_table[i * nu + c] = c < model_parameters.u_min.size() ? model_parameters.u_min[c] : -10e30;
                m_u_max_table[i * nu + c] = c < model_parameters.u_max.size() ? model_parameters.u_max[c] : 10e30;
            }
        m_limits_per_instance = true;
    }
    std::copy(u_min.begin(), u_min.end(), m_u_min_table.begin() + static_cast<size_t>(b) * nu);
    std::copy(u_max.begin(), u_max.end(), m_u_max_table.begin() + static_cast<size_t>(b) * nu);
}

void BatchModelControl::set_num_control_inputs_saved(int m_pin) {
    if (m_pin < 0 || m_pin > m->N - 1)
        throw std::invalid_argument("set_num_control_inputs_saved: m must be 0 .. num_shooting_nodes - 1");
    m_num_control_inputs_saved = m_pin;
}

void BatchModelControl::set_sensitivity_barrier(double mu, double sigma_cap) {
    std::lock_guard<std::mutex> lg(m_solve_mutex);   // between ticks
    double dmu = 0.0, dcap = 0.0;
    m->check(m->lib->sensitivity_barrier_default(&dmu, &dcap), "mmpc_sensitivity_barrier_default");
    m->check(m->lib->set_sensitivity_barrier(m->h, mu < 0.0 ? dmu : mu, sigma_cap > 0.0 ? sigma_cap : dcap),
             "mmpc_set_sensitivity_barrier");
}

void BatchModelControl::set_barrier_rule(int rule) {
    std::lock_guard<std::mutex> lg(m_solve_mutex);   // between ticks
    m->check(m->lib->set_barrier_rule(m->h, rule), "mmpc_set_barrier_rule");
}

}  // namespace mpc
}  // namespace mahi
