// Mahi/Mpc/BatchModelControl.hpp -- the reference's online controller (ModelControl, ModelControl.cpp:75-197)
// for B independent instances of one model.
//
// Reference semantics kept per instance: set_state() stores the latest measurement snapshot (:93-100 under
// m_state_mutex), the worker thread started by start_calc() solves from the latest snapshot, warm-started with
// the previous solution (:160-161), and publishes control_results (:174-190) that control_at_time() reads
// (:192-197).  Batched and MI355X-side:
//   * one GPU solve per tick for all B instances (mmpc_solve_batch, device pointers, stream-ordered);
//   * the warm start V stays resident in HBM between ticks (never copied back in to the device);
//   * inputs go through two pinned staging slots and a copy stream: the upload of tick i+1 overlaps the solve of
//     tick i, the download of tick i's solution (from a per-slot device copy, so the next solve may overwrite V)
//     overlaps the solve of tick i+1; results are published when their download event completes;
//   * optional warm-start shift (off by default, as the reference): V moved k stages earlier, k = elapsed
//     time / step, by two strided device copies;
//   * control limits for all instances or per instance (update_control_limits): B reference controllers have B limit
//     sets that change independently (ModelControl.cpp:205-209); the per-instance table [B][nu] x 2 is packed into the
//     tick's staging slot and travels in its single H2D (mmpc_solve_batch_bounds, bounds_stride = nu).
#pragma once
#include <atomic>
#include <condition_variable>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <Mahi/Mpc/ModelControl.hpp>
#include <Mahi/Mpc/ModelParameters.hpp>
#include <Mahi/Util/Time.hpp>

namespace mahi {
namespace mpc {

class BatchModelControl {
public:
    using ControlResult = ModelControl::ControlResult;

    // model_name: <model_name>.json (ModelControl.cpp:24); B instances; device -1 = current HIP device
    BatchModelControl(std::string model_name, int64_t B, std::vector<double> Q, std::vector<double> R,
                      std::vector<double> Rm, Dict solver_opts = Dict(), int device = -1);
    ~BatchModelControl();
    BatchModelControl(const BatchModelControl&) = delete;
    BatchModelControl& operator=(const BatchModelControl&) = delete;

    ModelParameters model_parameters;
    int64_t batch() const { return m_B; }

    // synchronous tick: states [B*nx], controls [B*nu] (previous inputs, the Delta-u reference), trajs [B*N*nx]
    void calc_u(mahi::util::Time time, const std::vector<double>& states, const std::vector<double>& controls,
                const std::vector<double>& trajs);

    // asynchronous loop (ModelControl.cpp:75-114)
    void set_state(mahi::util::Time time, const std::vector<double>& states, const std::vector<double>& controls,
                   const std::vector<double>& trajs);
    void start_calc();
    void stop_calc();

    // published results (latest completed tick)
    ControlResult control_at_time(int64_t b, mahi::util::Time time);  // instance b, as ModelControl.cpp:192-197
    std::vector<double> controls_at_time(mahi::util::Time time);      // [B*nu], every instance
    std::vector<double> solution(int64_t b);                          // V* of instance b (reference layout)
    std::vector<int> last_status();                                   // per instance
    std::vector<int> last_iterations();
    mahi::util::Time last_solve_time();                               // time stamp of the published tick
    int64_t ticks_published() const { return m_ticks; }
    double mean_tick_ms() const;                                      // worker: enqueue -> published

    void update_weights(std::vector<double> Q = {}, std::vector<double> R = {}, std::vector<double> Rm = {});
    // the control limits of ALL instances (ModelControl::update_control_limits for every controller of the batch);
    // returns the object to one shared box after per-instance updates
    void update_control_limits(std::vector<double> u_min, std::vector<double> u_max);
    // the control limits of instance b alone -- ModelControl::update_control_limits (ModelControl.cpp:205-209) of that
    // one controller: derated actuators, limits that follow speed or temperature, mixed hardware.  The other instances
    // keep theirs.  The table travels in the tick's single H2D (mmpc_solve_batch_bounds, bounds_stride = nu); a tick
    // uses the limits in force when it is enqueued.  Additive: not part of the reference's interface.
    void update_control_limits(int64_t b, std::vector<double> u_min, std::vector<double> u_max);
    // move the warm start k = round((t - t_prev) / step) stages earlier before each solve (default false)
    void set_warm_start_shift(bool on) { m_shift = on; }
    // barrier rule of the solves with finite state bounds (x_min / x_max of the model file): 0 = IPOPT's monotone rule
    // (default), 1 = Mehrotra's predictor-corrector (mmpc_set_barrier_rule in include/mmpc.h: 16-lane solver, nonlinear
    // mode; a solve it does not cover then throws).  Additive: not part of the reference's interface.
    void set_barrier_rule(int rule);
    // Feedback under state limits.  set_feedback_stages on a controller whose JSON or setters carry state limits needs
    // the sensitivity barrier switched on (mmpc_set_sensitivity_barrier in include/mmpc.h): the gains are then those of
    // the interior point's barrier problem at the plan.  mu < 0: the library's default (the barrier value a
    // monotone-rule solve ends at), mu = 0: off (the state of a new object); sigma_cap <= 0: the library's default
    // (1e12).  Without state limits the setting has no effect.
    void set_sensitivity_barrier(double mu = -1.0, double sigma_cap = 0.0);
    // Committed controls, per instance (ModelControl::set_num_control_inputs_saved for every controller of the batch):
    // from the first tick enqueued after a plan has been published, stage i < m of instance b is pinned to that
    // instance's published control at index clamp(round((t - t_published) / step) + i, 0, N - 1) -- the plan
    // published at enqueue time, which in the pipelined loop is the newest one a user of control_at_time can be
    // applying.  The [B][m][nu] table is packed into the tick's staging slot and travels in its single H2D
    // (mmpc_solve_batch_pinned).  m = 0 (default) pins nothing; m must be 0 .. N - 1.  Additive.
    void set_num_control_inputs_saved(int m);
    // Feedback along the plans (ModelControl::set_feedback_stages for every controller of the batch; include/mmpc.h,
    // "feedback gains"): the gain launch goes onto the tick's stream behind the solve, under that tick's limits and
    // pins, and the gains of the first n stages travel in the slot's download with the solution.  n must be 0 .. N; 0
    // (the default) launches nothing and every published value is what it is without this call.  Additive.
    void set_feedback_stages(int n);
    // G_i of instance b's published plan, num_u x (num_x + num_u) row-major, and the instances' gain status (0 as
    // asked, 1 Gauss-Newton fallback, 2 failed: gains 0; empty when the published tick carries no gains)
    std::vector<double> feedback_gain(int64_t b, int i);
    std::vector<int> feedback_status();
    // controls_at_time with the measured states [B*nx]: per instance clamp(u_i + G_i[:, :nx] (x_measured - x_est_i),
    // u_min, u_max) with that instance's limits; the plan for a stage without gains or an instance with status 2
    std::vector<double> controls_at_time(mahi::util::Time time, const std::vector<double>& states_measured);

    // Real-time iteration mode (include/mmpc.h, "real-time iteration").  Off by default, and with it off
    // every code path, buffer and published value is what it is without these members.  With it on, calc_u and the
    // start_calc worker run one of two ticks:
    //   * a full tick -- all inputs up, one solve from the resident plan, everything down -- when no preparation
    //     exists, when the previous tick raised the fallback flag (an instance with status 2 or step_inf >
    //     step_inf_max; the whole batch re-solves), or when the preparation is stale (made for another instant than
    //     `time`: round((time - t_prepared) / step) != 0);
    //   * an RTI tick otherwise: only the measured states go up, one feedback launch runs on the records the
    //     preparation stored, u_0 is published with the tick's time as soon as that launch is done (u0, step_inf and
    //     status are written by the kernel into host memory), the whole plan follows on the copy stream.  The
    //     `controls` argument is not used: the preparation took the plan's own control in force.  An instance with
    //     status 2 publishes the plan's own u_0.  last_status() of an RTI tick is the step's status (0 as asked, 1
    //     Gauss-Newton fallback, 2 failed), last_iterations() 1.
    // After either tick, without waiting, the plan is shifted by one stage on the device (mmpc_rti_shift_batch: the last
    // control repeated, the terminal state rolled out) and the next preparation is queued at the shifted plan, for
    // time + step, with the weights and control limits in force now and the targets of set_next_targets (else this
    // tick's targets moved one row, the last row repeated).  The clamp of a feedback launch is the control box its
    // preparation ran under.  set_warm_start_shift is not consulted in this mode.
    // The first tick with the mode on throws for a linear-mode model, any finite state limit,
    // set_num_control_inputs_saved(m > 0) or set_feedback_stages(n > 0).  set_rti_mode(true) throws for a generated
    // model library built before the RTI entries existed.  Additive: not part of the reference's interface.
    void set_rti_mode(bool on, double step_inf_max = std::numeric_limits<double>::infinity());
    // targets [B*N*nx] of the next preparation (the horizon starting at the next tick); consumed by one tick
    void set_next_targets(const std::vector<double>& trajs_next);
    int64_t rti_ticks() const { return m_rti_ticks; }
    int64_t full_solve_ticks() const { return m_full_ticks; }   // full ticks with the mode on
    std::vector<double> last_step_inf();                         // [B] max |dV| of the published RTI tick; 0 after a full tick
    double mean_feedback_latency_ms() const;                     // tick entry -> u_0 published, RTI ticks only

private:
    struct Impl;
    std::unique_ptr<Impl> m;
    int64_t m_B;
    std::atomic<bool> m_shift{false};
    std::atomic<int> m_num_control_inputs_saved{0};
    std::atomic<int64_t> m_ticks{0};
    std::atomic<bool> m_stop{true};
    std::thread m_thread;

    std::mutex m_state_mutex;  // snapshot (ModelControl.hpp:71)
    std::condition_variable m_state_cv;
    uint64_t m_state_version = 0;
    mahi::util::Time m_time;
    std::vector<double> m_states, m_controls, m_trajs;

    std::mutex m_output_mutex;  // published results (ModelControl.hpp:72)
    mahi::util::Time m_out_time;
    std::vector<double> m_out_V;
    std::vector<int> m_out_status, m_out_iters;
    int m_out_fb = 0;                 // stages the published tick carries gains for
    std::vector<double> m_out_G;      // [B][m_out_fb][nu][nx + nu]
    std::vector<int> m_out_gst;       // [B]
    std::atomic<int> m_feedback_stages{0};

    std::mutex m_weights_mutex;
    std::vector<double> m_Q, m_R, m_Rm;
    std::mutex m_control_limits_mutex;
    bool m_limits_per_instance = false;               // under m_control_limits_mutex, as the two tables
    std::vector<double> m_u_min_table, m_u_max_table;  // [B*nu] while per-instance limits are in use

    std::mutex m_solve_mutex;  // one tick pipeline at a time (calc_u vs the worker)
    double m_tick_ms_sum = 0.0;

    // real-time iteration mode
    std::atomic<bool> m_rti_mode{false};
    double m_step_inf_max = std::numeric_limits<double>::infinity();   // under m_solve_mutex
    std::vector<double> m_next_targets;                                // under m_state_mutex, as m_have_next_targets
    bool m_have_next_targets = false;
    std::atomic<int64_t> m_rti_ticks{0}, m_full_ticks{0};
    double m_fb_ms_sum = 0.0;
    std::vector<double> m_out_step_inf;   // under m_output_mutex, as the u_0 published ahead of its plan:
    bool m_u0_ahead = false;              // u_0 of a tick whose plan has not landed yet
    mahi::util::Time m_u0_time;
    std::vector<double> m_u0_x, m_u0_u;   // [B nx] measured states, [B nu]
    void rti_tick(mahi::util::Time time, const double* states, const double* controls, const double* trajs);

    void enqueue_tick(int slot, mahi::util::Time time, const double* states, const double* controls,
                      const double* trajs);
    void publish(int slot);
    void worker();
};

}  // namespace mpc
}  // namespace mahi
