// Mahi/Mpc/ModelControl.hpp -- drop-in for the reference class (include/Mahi/Mpc/ModelControl.hpp:13-80).
// Same public members and method signatures; the IPOPT call of calc_u (ModelControl.cpp:159) is replaced by
// the MI355X batched SQP behind include/mmpc.h.  casadi::Dict is replaced by mahi::mpc::Dict.
#pragma once
#include <atomic>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <Mahi/Mpc/External.hpp>
#include <Mahi/Mpc/ModelParameters.hpp>
#include <Mahi/Mpc/SX.hpp>
#include <Mahi/Util/Time.hpp>

struct mmpc_handle;

namespace mahi {
namespace mpc {
namespace detail {
struct ModelLibrary;
class RtiPipeline;
}

using Dict = std::map<std::string, double>;

class ModelControl {
public:
    struct ControlResult {
        ControlResult(mahi::util::Time time_, std::vector<double> x_est_, std::vector<double> u_)
            : time(time_), x_est(x_est_), u(u_) {}
        mahi::util::Time time;
        std::vector<double> x_est;
        std::vector<double> u;
    };

    ModelControl(std::string model_name, std::vector<double> Q = {}, std::vector<double> R = {},
                 std::vector<double> Rm = {}, Dict solver_opts = Dict());
    ~ModelControl();
    ModelControl(const ModelControl&) = delete;
    ModelControl& operator=(const ModelControl&) = delete;

    ModelParameters model_parameters;
    std::vector<ControlResult> control_results;

    void calc_u(mahi::util::Time time, const std::vector<double>& state, const std::vector<double>& control,
                std::vector<double> traj);
    void load_model(const std::string& model_name);

    ControlResult control_at_time(mahi::util::Time time);

    void start_calc();
    void stop_calc();

    void set_state(mahi::util::Time time, const std::vector<double>& state, const std::vector<double>& control,
                   std::vector<double> traj);

    void update_weights(std::vector<double> Q = {}, std::vector<double> R = {}, std::vector<double> Rm = {});
    void update_control_limits(std::vector<double> u_min, std::vector<double> u_max);
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
    // Committed controls (delay compensation): the setter the reference's private m_num_control_inputs_saved
    // (ModelControl.hpp:79) never got.  From the second calc_u on, the first m controls of the horizon are pinned to the
    // controls the previous plan holds for those instants: stage i < m gets the previous plan's control at index
    // clamp(round((t - t_prev) / step) + i, 0, N - 1), read under m_output_mutex as ModelControl.cpp:166 does; the
    // first call pins nothing.  The solve then optimises only what can still be decided (mmpc_solve_batch_host_pinned).
    // Departure from the reference's stub (ModelControl.cpp:165-171), which is dead: it copies index for index (no
    // shift by the elapsed time) into lbx / ubx, and the next calc_u overwrites those with u_min / u_max (:150-153)
    // before solving.  m = 0 (the default) is the reference's behaviour; m must be 0 .. N - 1; linear-mode models
    // throw at the first pinned solve.  Additive: not part of the reference's interface.
    void set_num_control_inputs_saved(int m);
    // Feedback along the plan (include/mmpc.h, "feedback gains"): after each solve the gains G_i = d u_i* / d(x_i,
    // u_{i-1}) of the first n stages are computed from the published V*, under the control limits in force (a control
    // on a limit has a zero row) and with the committed controls of that solve held, and published with the plan.
    // n must be 0 .. N; 0 (the default) computes nothing, and every published value is what it is without this call.
    // A linear-mode model or finite state bounds make the next calc_u throw.  Additive: not part of the reference's
    // interface (ModelControl.cpp:174-197 publishes and reads the open-loop plan only).
    void set_feedback_stages(int n);
    // G_i of the published plan, num_u x (num_x + num_u) row-major (columns 0 .. num_x - 1: d u_i / d x_i); i must be
    // below the number of stages the published plan carries gains for
    std::vector<double> feedback_gain(int i);
    // 0 as asked (the exact Hessian where the model has second derivatives), 1 Gauss-Newton fallback, 2 failed (the
    // gains are 0: pure feed-forward); -1 when the published plan carries no gains
    int feedback_status();
    // control_at_time with the measured state: the stage i of the reference's index rule (ModelControl.cpp:192-197),
    // and ControlResult{time_i, x_est_i, clamp(u_i + G_i[:, :nx] (x_measured - x_est_i), u_min, u_max)} -- the
    // neighbouring-extremal control.  For a stage without gains (i >= n, or feedback_status() == 2): the plan.
    ControlResult control_at_time(mahi::util::Time time, const std::vector<double>& x_measured);

    // Real-time iteration mode (include/mmpc.h, "real-time iteration"): BatchModelControl's mode for
    // this one controller, through the same device pipeline with B = 1 -- see BatchModelControl::set_rti_mode for the
    // tick rule (full tick / RTI tick, fallback flag, stale preparation) and the refusals, which are the same.  The
    // next preparation's targets are this tick's `traj` moved one row (the last row repeated).  An RTI tick steps the
    // plan with one feedback launch on the measured state (`control` is not used) and fills control_results from the
    // stepped plan; last_status() is then the step's status (0 / 1 / 2), last_iterations() 1.  Off by default, and
    // with it off nothing changes.  Additive: not part of the reference's interface.
    void set_rti_mode(bool on, double step_inf_max = std::numeric_limits<double>::infinity());
    long long rti_ticks() const { return m_rti_ticks; }
    long long full_solve_ticks() const { return m_full_ticks; }   // full ticks with the mode on
    double last_step_inf();                                        // max |dV| of the last RTI tick; 0 after a full tick

    // ---- build extensions (not in the reference) ----
    // solver status of the last calc_u (the reference ignores IPOPT's status, ModelControl.cpp:159-161)
    int last_status() const { return m_last_status; }
    int last_iterations() const { return m_last_iters; }
    double last_kkt_residual() const { return m_last_kkt; }
    // B independent instances in one GPU call (states/controls/trajs instance-major); returns V* per instance
    std::vector<std::vector<double>> calc_u_batch(const std::vector<std::vector<double>>& states,
                                                  const std::vector<std::vector<double>>& controls,
                                                  const std::vector<std::vector<double>>& trajs,
                                                  std::vector<int>* status = nullptr);
    // the same with the control limits of each instance: u_mins / u_maxs hold B rows of num_u entries (what B
    // controllers would each have set with update_control_limits); this object's own limits are not used
    std::vector<std::vector<double>> calc_u_batch(const std::vector<std::vector<double>>& states,
                                                  const std::vector<std::vector<double>>& controls,
                                                  const std::vector<std::vector<double>>& trajs,
                                                  const std::vector<std::vector<double>>& u_mins,
                                                  const std::vector<std::vector<double>>& u_maxs,
                                                  std::vector<int>* status = nullptr);

private:
    std::shared_ptr<detail::ModelLibrary> m_backend;  // C-ABI of the model's library (dll_filepath)
    Dict m_solver_opts;
    mahi::util::Time curr_time;
    mmpc_handle* m_handle = nullptr;
    std::vector<double> m_V;  // warm start = previous solution (ModelControl.cpp:160-161)

    std::vector<double> m_Q, m_R, m_Rm;

    std::atomic<bool> m_stop{true};
    std::atomic<bool> m_done_calcing{true};
    std::thread m_thread;

    mahi::util::Time m_time;
    std::vector<double> m_state, m_control, m_traj;

    std::mutex m_state_mutex;
    std::mutex m_output_mutex;
    std::mutex m_control_limits_mutex;
    std::mutex m_weights_mutex;

    std::atomic<int> m_num_control_inputs_saved{0};  // ModelControl.hpp:79 (there an int without a setter)
    std::atomic<int> m_feedback_stages{0};
    std::vector<double> m_gains;   // [n][nu][nx + nu] of the published plan (under m_output_mutex, as m_gain_status)
    int m_gain_status = -1;

    std::atomic<bool> m_rti_mode{false};   // real-time iteration mode
    double m_step_inf_max = std::numeric_limits<double>::infinity();
    std::shared_ptr<detail::RtiPipeline> m_rti;
    std::mutex m_rti_mutex;                // calc_u (either mode), set_rti_mode and load_model exclude one another
    int m_device = -1;                     // the device current when the handle was made: the pipeline's
    std::atomic<long long> m_rti_ticks{0}, m_full_ticks{0};
    double m_last_step_inf = 0.0;          // under m_output_mutex
    void rti_calc_u(mahi::util::Time time, const std::vector<double>& state, const std::vector<double>& control,
                    const std::vector<double>& traj);

    int m_last_status = -1;
    int m_last_iters = 0;
    double m_last_kkt = 0.0;

    void format_outputs(const std::vector<double>& opt_output, std::vector<double> gains = {}, int gain_status = -1);
    std::vector<double> packed_weights();
    // calc_u_batch with this object's limits (u_mins == nullptr) or a row of limits per instance
    std::vector<std::vector<double>> calc_u_batch_impl(const std::vector<std::vector<double>>& states,
                                                       const std::vector<std::vector<double>>& controls,
                                                       const std::vector<std::vector<double>>& trajs,
                                                       const std::vector<std::vector<double>>* u_mins,
                                                       const std::vector<std::vector<double>>* u_maxs,
                                                       std::vector<int>* status);
};

}  // namespace mpc
}  // namespace mahi

namespace casadi {
using mahi::mpc::Dict;   // the solver_opts type of the reference's constructor (ModelControl.hpp:26)
}  // namespace casadi
