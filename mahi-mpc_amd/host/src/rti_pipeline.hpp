// rti_pipeline.hpp -- internal: the device state and the tick of the real-time iteration mode of ModelControl (B = 1)
// and BatchModelControl.  It owns
//   * the resident plan and a second plan buffer (the shift writes into the other one, then the two swap);
//   * the RTI workspace of mmpc_rti_workspace_bytes;
//   * the staged inputs: of a tick (x0 | u_prev | traj | weights | lb | ub) and of the next preparation
//     (traj | weights | lb | ub, and the u_prev the shift writes);
//   * mmpc_host_alloc memory for u0, step_inf and status, which the feedback launch writes directly.
// One tick is either a full tick -- all inputs up, mmpc_solve_batch_bounds from the resident plan, everything down --
// or an RTI tick: the measured states up, mmpc_rti_feedback_batch on the stored records, u0 on the host as soon as
// the compute stream is idle, the plan following on the copy stream.  After either, mmpc_rti_shift_batch (n = 1) and
// mmpc_rti_prepare_batch at the shifted plan are queued on the compute stream and not waited for.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "../../../include/mmpc.h"
#include "model_library.hpp"

namespace mahi {
namespace mpc {
namespace detail {

class RtiPipeline {
public:
    // what a tick reads; lb / ub: [nu] shared or [B nu] per instance, either may be null (no bound on that side)
    struct Inputs {
        double t = 0.0;
        const double* states = nullptr;        // [B nx] measured
        const double* controls = nullptr;      // [B nu] previous inputs: a full tick alone reads them
        const double* trajs = nullptr;         // [B N nx] this tick's targets
        const double* next_trajs = nullptr;    // [B N nx] targets of the next preparation, or null: trajs moved one row
        const double* weights = nullptr;       // [nx + 2 nu]
        const double* lb = nullptr;
        const double* ub = nullptr;
        bool per_instance = false;
        double step_inf_max = INFINITY;
    };

    RtiPipeline(std::shared_ptr<ModelLibrary> lib, mmpc_handle* h, int64_t B, int device)
        : m_lib(std::move(lib)), m_h(h), m_B(B), m_dev(device) {
        if (!m_lib->rti_shift_batch || !m_lib->rti_prepare_batch || !m_lib->rti_feedback_batch ||
            !m_lib->rti_workspace_bytes || !m_lib->host_alloc || !m_lib->host_free)
            throw std::runtime_error(
                "the model library lacks the real-time iteration entries (mmpc_rti_*_batch, mmpc_host_alloc): it was "
                "generated before they existed; generate the model again");
        try {
            allocate();
        } catch (...) {   // the destructor does not run for a constructor that throws
            release();
            throw;
        }
    }

    ~RtiPipeline() { release(); }
    RtiPipeline(const RtiPipeline&) = delete;
    RtiPipeline& operator=(const RtiPipeline&) = delete;

private:
    void allocate() {
        const int64_t B = m_B;
        mmpc_model_info info;
        m_lib->check(m_lib->get_model_info(m_h, &info), "mmpc_get_model_info");
        m_nx = info.num_x, m_nu = info.num_u, m_N = info.num_shooting_nodes, m_NV = info.num_v;
        m_step = info.step_size;
        const size_t b = static_cast<size_t>(B), nx = m_nx, nu = m_nu, N = m_N, NV = m_NV;
        m_off_up = b * nx;
        m_off_tr = m_off_up + b * nu;
        m_off_w = m_off_tr + b * N * nx;
        m_off_lb = m_off_w + nx + 2 * nu;
        m_off_ub = m_off_lb + b * nu;
        m_in_doubles = m_off_ub + b * nu;
        m_poff_w = b * N * nx;
        m_poff_lb = m_poff_w + nx + 2 * nu;
        m_poff_ub = m_poff_lb + b * nu;
        m_prep_doubles = m_poff_ub + b * nu;
        hip(hipSetDevice(m_dev), "hipSetDevice");
        hip(hipStreamCreateWithFlags(&m_compute, hipStreamNonBlocking), "hipStreamCreate");
        hip(hipStreamCreateWithFlags(&m_copy, hipStreamNonBlocking), "hipStreamCreate");
        hip(hipEventCreateWithFlags(&m_stepped, hipEventDisableTiming), "hipEventCreate");
        hip(hipEventCreateWithFlags(&m_landed, hipEventDisableTiming), "hipEventCreate");
        for (int s = 0; s < 2; ++s) {
            hip(hipMalloc(reinterpret_cast<void**>(&m_dV[s]), b * NV * sizeof(double)), "hipMalloc");
            hip(hipMemset(m_dV[s], 0, b * NV * sizeof(double)), "hipMemset");
        }
        m_lib->check(m_lib->rti_workspace_bytes(m_h, B, &m_ws_bytes), "mmpc_rti_workspace_bytes");
        hip(hipMalloc(&m_ws, m_ws_bytes), "hipMalloc");
        hip(hipMalloc(reinterpret_cast<void**>(&m_din), m_in_doubles * sizeof(double)), "hipMalloc");
        hip(hipMalloc(reinterpret_cast<void**>(&m_dprep), m_prep_doubles * sizeof(double)), "hipMalloc");
        hip(hipMalloc(reinterpret_cast<void**>(&m_dup), b * nu * sizeof(double)), "hipMalloc");
        hip(hipMalloc(reinterpret_cast<void**>(&m_dst), 3 * b * sizeof(int32_t)), "hipMalloc");   // status | iters | prep
        hip(hipHostMalloc(reinterpret_cast<void**>(&m_hin), m_in_doubles * sizeof(double), hipHostMallocDefault),
            "hipHostMalloc");
        hip(hipHostMalloc(reinterpret_cast<void**>(&m_hprep), m_prep_doubles * sizeof(double), hipHostMallocDefault),
            "hipHostMalloc");
        hip(hipHostMalloc(reinterpret_cast<void**>(&m_hV), b * NV * sizeof(double), hipHostMallocDefault),
            "hipHostMalloc");
        hip(hipHostMalloc(reinterpret_cast<void**>(&m_hst), 2 * b * sizeof(int32_t), hipHostMallocDefault),
            "hipHostMalloc");
        // u0 [B nu] | step_inf [B] | status [B] in memory the feedback kernel stores into directly
        void* hb = nullptr;
        m_lib->check(m_lib->host_alloc((b * nu + b) * sizeof(double) + b * sizeof(int32_t), &hb), "mmpc_host_alloc");
        m_hu0 = static_cast<double*>(hb);
        m_hsi = m_hu0 + b * nu;
        m_hfst = reinterpret_cast<int32_t*>(m_hsi + b);
        m_lib->check(m_lib->reserve_workspace(m_h, B, nullptr), "mmpc_reserve_workspace");
        m_status.assign(b, -1);
        m_iters.assign(b, 0);
    }

    // frees whatever has been created so far: every member starts out null
    void release() {
        (void)hipSetDevice(m_dev);
        if (m_compute) (void)hipStreamSynchronize(m_compute);
        if (m_copy) (void)hipStreamSynchronize(m_copy);
        for (int s = 0; s < 2; ++s) (void)hipFree(m_dV[s]);
        (void)hipFree(m_ws);
        (void)hipFree(m_din);
        (void)hipFree(m_dprep);
        (void)hipFree(m_dup);
        (void)hipFree(m_dst);
        (void)hipHostFree(m_hin);
        (void)hipHostFree(m_hprep);
        (void)hipHostFree(m_hV);
        (void)hipHostFree(m_hst);
        if (m_hu0) (void)m_lib->host_free(m_hu0);
        if (m_stepped) (void)hipEventDestroy(m_stepped);
        if (m_landed) (void)hipEventDestroy(m_landed);
        if (m_compute) (void)hipStreamDestroy(m_compute);
        if (m_copy) (void)hipStreamDestroy(m_copy);
    }

public:
    // The resident plan from / to memory of the caller (host or device); both wait for the queued work.  Taking a
    // plan in drops the preparation: the next tick is a full tick.
    void set_plan(const double* V, hipMemcpyKind kind) {
        hip(hipSetDevice(m_dev), "hipSetDevice");
        hip(hipStreamSynchronize(m_compute), "hipStreamSynchronize");
        hip(hipMemcpy(m_dV[m_cur], V, static_cast<size_t>(m_B) * m_NV * sizeof(double), kind), "hipMemcpy");
        m_prepared = false;
        m_fallback = false;
    }
    void get_plan(double* V, hipMemcpyKind kind) {
        hip(hipSetDevice(m_dev), "hipSetDevice");
        hip(hipStreamSynchronize(m_compute), "hipStreamSynchronize");
        hip(hipMemcpy(V, m_dV[m_cur], static_cast<size_t>(m_B) * m_NV * sizeof(double), kind), "hipMemcpy");
    }

    // One tick.  on_u0() is called when u0(), step_inf() and status() of this tick are on the host -- on an RTI tick
    // before the plan has come down.  When tick() returns plan() holds the tick's plan and the background (shift,
    // preparation) is queued.  Returns true for an RTI tick.
    template <class F>
    bool tick(const Inputs& in, F&& on_u0) {
        hip(hipSetDevice(m_dev), "hipSetDevice");
        const size_t b = static_cast<size_t>(m_B), nx = m_nx, nu = m_nu, N = m_N, NV = m_NV, nw = nx + 2 * nu;
        const size_t nb = in.per_instance ? b * nu : nu;
        const int64_t stride = in.per_instance ? static_cast<int64_t>(nu) : 0;
        const bool stale = m_prepared && std::llround((in.t - m_t_prepared) / m_step) != 0;
        const bool full = !m_prepared || m_fallback || stale;
        if (full) {
            std::memcpy(m_hin, in.states, b * nx * sizeof(double));
            std::memcpy(m_hin + m_off_up, in.controls, b * nu * sizeof(double));
            std::memcpy(m_hin + m_off_tr, in.trajs, b * N * nx * sizeof(double));
            std::memcpy(m_hin + m_off_w, in.weights, nw * sizeof(double));
            if (in.lb) std::memcpy(m_hin + m_off_lb, in.lb, nb * sizeof(double));
            if (in.ub) std::memcpy(m_hin + m_off_ub, in.ub, nb * sizeof(double));
            hip(hipMemcpyAsync(m_din, m_hin, m_in_doubles * sizeof(double), hipMemcpyHostToDevice, m_compute), "H2D");
            m_lib->check(m_lib->solve_batch_bounds(m_h, m_B, m_din, m_din + m_off_up, m_din + m_off_tr, m_din + m_off_w,
                                                   0, in.lb ? m_din + m_off_lb : nullptr,
                                                   in.ub ? m_din + m_off_ub : nullptr, stride, m_dV[m_cur], m_dst,
                                                   m_dst + b, nullptr, nullptr, m_compute),
                         "mmpc_solve_batch_bounds");
            hip(hipMemcpyAsync(m_hV, m_dV[m_cur], b * NV * sizeof(double), hipMemcpyDeviceToHost, m_compute), "D2H");
            hip(hipMemcpyAsync(m_hst, m_dst, 2 * b * sizeof(int32_t), hipMemcpyDeviceToHost, m_compute), "D2H");
            hip(hipStreamSynchronize(m_compute), "hipStreamSynchronize");
            for (size_t i = 0; i < b; ++i) {
                std::memcpy(m_hu0 + i * nu, m_hV + i * NV + nx, nu * sizeof(double));
                m_hsi[i] = 0.0;   // no step: the plan is a solve's
                m_status[i] = m_hst[i];
                m_iters[i] = m_hst[b + i];
            }
            m_fallback = false;
            on_u0();
        } else {
            std::memcpy(m_hin, in.states, b * nx * sizeof(double));
            hip(hipMemcpyAsync(m_din, m_hin, b * nx * sizeof(double), hipMemcpyHostToDevice, m_compute), "H2D");
            // the clamp is the control box the preparation ran under
            m_lib->check(m_lib->rti_feedback_batch(m_h, m_B, m_din, m_prep_lb ? m_dprep + m_poff_lb : nullptr,
                                                   m_prep_ub ? m_dprep + m_poff_ub : nullptr, m_prep_stride,
                                                   m_dV[m_cur], m_hu0, m_hsi, m_hfst, m_ws, m_ws_bytes, m_compute),
                         "mmpc_rti_feedback_batch");
            hip(hipEventRecord(m_stepped, m_compute), "hipEventRecord");
            hip(hipStreamWaitEvent(m_copy, m_stepped, 0), "hipStreamWaitEvent");
            hip(hipMemcpyAsync(m_hV, m_dV[m_cur], b * NV * sizeof(double), hipMemcpyDeviceToHost, m_copy), "D2H");
            hip(hipEventRecord(m_landed, m_copy), "hipEventRecord");
            hip(hipStreamSynchronize(m_compute), "hipStreamSynchronize");
            bool fb = false;
            for (size_t i = 0; i < b; ++i) {
                m_status[i] = m_hfst[i];
                m_iters[i] = 1;
                fb |= m_hfst[i] == 2 || !(m_hsi[i] <= in.step_inf_max);
            }
            m_fallback = fb;
            on_u0();
        }
        // the background: the shift into the other buffer, then the preparation at the shifted plan
        for (size_t i = 0; i < b; ++i)
            for (size_t k = 0; k < N; ++k) {
                const double* src = in.next_trajs ? in.next_trajs + (i * N + k) * nx
                                                  : in.trajs + (i * N + (k + 1 < N ? k + 1 : N - 1)) * nx;
                std::memcpy(m_hprep + (i * N + k) * nx, src, nx * sizeof(double));
            }
        std::memcpy(m_hprep + m_poff_w, in.weights, nw * sizeof(double));
        if (in.lb) std::memcpy(m_hprep + m_poff_lb, in.lb, nb * sizeof(double));
        if (in.ub) std::memcpy(m_hprep + m_poff_ub, in.ub, nb * sizeof(double));
        m_lib->check(m_lib->rti_shift_batch(m_h, m_B, m_dV[m_cur], 1, m_dV[m_cur ^ 1], m_dup, m_compute),
                     "mmpc_rti_shift_batch");
        m_cur ^= 1;
        hip(hipMemcpyAsync(m_dprep, m_hprep, m_prep_doubles * sizeof(double), hipMemcpyHostToDevice, m_compute), "H2D");
        m_prep_lb = in.lb != nullptr, m_prep_ub = in.ub != nullptr, m_prep_stride = stride;
        m_lib->check(m_lib->rti_prepare_batch(m_h, m_B, m_dV[m_cur], m_dup, m_dprep, m_dprep + m_poff_w, 0,
                                              m_prep_lb ? m_dprep + m_poff_lb : nullptr,
                                              m_prep_ub ? m_dprep + m_poff_ub : nullptr, stride, 0, MMPC_HESSIAN_AUTO,
                                              m_dst + 2 * b, m_ws, m_ws_bytes, m_compute),
                     "mmpc_rti_prepare_batch");
        m_prepared = true;
        m_t_prepared = in.t + m_step;
        if (!full) hip(hipEventSynchronize(m_landed), "hipEventSynchronize");   // the plan has come down
        return !full;
    }

    const double* plan() const { return m_hV; }           // [B NV]
    const double* u0() const { return m_hu0; }            // [B nu]
    const double* step_inf() const { return m_hsi; }      // [B]: 0 after a full tick
    const std::vector<int>& status() const { return m_status; }   // solver status (full tick), 0 / 1 / 2 (RTI tick)
    const std::vector<int>& iterations() const { return m_iters; }
    int64_t batch() const { return m_B; }

private:
    static void hip(hipError_t e, const char* what) {
        if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
    }
    std::shared_ptr<ModelLibrary> m_lib;
    mmpc_handle* m_h;
    int64_t m_B;
    int m_dev;
    int m_nx = 0, m_nu = 0, m_N = 0, m_NV = 0;
    double m_step = 0.0;
    size_t m_off_up = 0, m_off_tr = 0, m_off_w = 0, m_off_lb = 0, m_off_ub = 0, m_in_doubles = 0;
    size_t m_poff_w = 0, m_poff_lb = 0, m_poff_ub = 0, m_prep_doubles = 0;
    hipStream_t m_compute = nullptr, m_copy = nullptr;
    hipEvent_t m_stepped = nullptr, m_landed = nullptr;
    double* m_dV[2] = {nullptr, nullptr};
    int m_cur = 0;
    void* m_ws = nullptr;
    uint64_t m_ws_bytes = 0;
    double *m_din = nullptr, *m_dprep = nullptr, *m_dup = nullptr;
    int32_t* m_dst = nullptr;
    double *m_hin = nullptr, *m_hprep = nullptr, *m_hV = nullptr;
    int32_t* m_hst = nullptr;
    double *m_hu0 = nullptr, *m_hsi = nullptr;
    int32_t* m_hfst = nullptr;
    std::vector<int> m_status, m_iters;
    bool m_prepared = false, m_fallback = false;
    double m_t_prepared = 0.0;
    bool m_prep_lb = false, m_prep_ub = false;
    int64_t m_prep_stride = 0;
};

}  // namespace detail
}  // namespace mpc
}  // namespace mahi
