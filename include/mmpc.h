/*
 * mmpc.h -- C-ABI of the MI355X-native batched nonlinear-MPC solve path.
 *
 * This is the drop-in boundary for mahi-mpc's hot path.  Each entry point names
 * the reference interface it replaces (paths relative to the mahi-mpc tree):
 *
 *   mmpc_create / mmpc_create_from_json
 *       replaces ModelControl::load_model  (src/Mahi/Mpc/ModelControl.cpp:21-73):
 *       reads the <name>.json written by ModelGenerator::save_param_file
 *       (src/Mahi/Mpc/ModelGenerator.cpp:261-270; schema ModelParameters.cpp:37-72)
 *       instead of dlopen'ing the CasADi-generated <name>.so via nlpsol(...).
 *   mmpc_solve_batch / mmpc_solve_batch_host
 *       replaces `m_solver_result = m_solver(m_solver_args);`
 *       (src/Mahi/Mpc/ModelControl.cpp:159) -- the IPOPT call over the CasADi NLP
 *       evaluators -- for B independent instances at once, including the
 *       per-step linearisation of ModelControl.cpp:125-135 in linear mode.
 *   mmpc_linearize_batch
 *       replaces the CasADi externals <name>_get_A / _get_B / _get_x_dot_init
 *       (ModelGenerator.cpp:51-53, loaded at ModelControl.cpp:70-72; used by the
 *       examples' plant model, examples/model_control_example.cpp:81-82).
 *       A and B are returned COLUMN-major, as CasADi DM -> std::vector does.
 *   mmpc_nlp_eval_batch
 *       replaces the nlp_f / nlp_g evaluators of the generated <name>.so
 *       (ModelGenerator.cpp:206-222, generated at :238).
 *
 * Conventions.
 *   - All sizes are int64_t, all arithmetic fp64.
 *   - Layouts are instance-major ("array of instances"), reference order inside:
 *       x0[B][nx], u_prev[B][nu], traj[B][N][nx]   (traj row k = target of F(x_k,u_k),
 *       ModelGenerator.cpp:207-211), weights = (Q[nx] | R[nu] | Rm[nu]) shared
 *       (weights_stride 0) or per instance (weights_stride = nx+2nu),
 *       V[B][NV] with V = [x0,u0,x1,u1,...,x_{N-1},u_{N-1},x_N] (ModelGenerator.cpp:61-112).
 *   - V_inout is the primal warm start on entry (the reference keeps the previous
 *     solution as x0 for the next call, ModelControl.cpp:160-161; first call = zeros,
 *     ModelControl.cpp:29-50) and the solution on exit.  V[b][0:nx] is pinned to x0[b]
 *     as the reference pins x_0 through lbx = ubx = state (ModelControl.cpp:144-145).
 *   - mmpc_solve_batch takes DEVICE pointers and is stream-ordered on `stream`
 *     (a hipStream_t; NULL = default stream) and never synchronises.  The condensed
 *     solver never allocates; the Riccati solver uses a per-handle device workspace
 *     that grows (synchronously) when a larger B arrives -- call
 *     mmpc_reserve_workspace first to keep solves allocation-free (hipGraph capture).
 *     mmpc_solve_batch_host takes host pointers and is synchronous.
 *   - Functions return MMPC_OK (0) or a negative mmpc_result and never throw.
 *     Non-convergence is NOT an API error: it is reported per instance in
 *     status[] (the reference silently uses non-converged IPOPT output,
 *     ModelControl.cpp:159-163; callers here can see it).
 *   - A handle may be used from several threads only on distinct streams and only
 *     for the device-pointer entry points of the condensed solver (the Riccati
 *     workspace is per handle: use one handle per concurrent stream); the _host
 *     entry points serialise on an internal mutex.
 */
#ifndef MMPC_H
#define MMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMPC_ABI_VERSION 6

typedef struct mmpc_handle mmpc_handle;

/* API result codes (return values) */
enum mmpc_result {
    MMPC_OK = 0,
    MMPC_ERR_INVALID_ARG = -1,
    MMPC_ERR_IO = -2,
    MMPC_ERR_PARSE = -3,
    MMPC_ERR_UNSUPPORTED = -4,
    MMPC_ERR_HIP = -5,
    MMPC_ERR_NO_DEVICE = -6
};

/* per-instance solver status (status[] outputs).  Under state bounds (the interior-point variant) non-finite input
   data may surface as LINESEARCH_FAILED, NONFINITE or FACTORIZATION_FAILED (2, 3 or 4): which test meets the NaN/Inf
   first depends on where it enters the barrier terms; the instance's neighbours in the batch are unaffected. */
enum mmpc_status {
    MMPC_STATUS_CONVERGED = 0,            /* ||grad||_inf <= tol_grad and ||g||_inf <= tol_defect */
    MMPC_STATUS_MAX_ITER = 1,             /* opts.max_iter SQP iterations without convergence */
    MMPC_STATUS_LINESEARCH_FAILED = 2,    /* no sufficient merit decrease after 30 halvings */
    MMPC_STATUS_NONFINITE = 3,            /* NaN/Inf in the iterate or the KKT residual */
    MMPC_STATUS_FACTORIZATION_FAILED = 4, /* condensed Hessian not positive definite */
    MMPC_STATUS_BOUNDS_VIOLATED = 5       /* reserved (ABI 1 reported violated u bounds); u bounds are
                                             now enforced and this status is never produced */
};

/* built-in dynamics (device code; see DESIGN.md "Models") */
enum mmpc_model_id {
    MMPC_MODEL_TWO_LINK_ARM = 0, /* examples/ex_model_generate.cpp:24-43, nx=4 nu=2 */
    MMPC_MODEL_EXO_ARM = 1,      /* 4-DoF exo, nx=8 nu=4: M(q) of src/inverseTest.cpp:59-74 with the
                                    build-defined parameters of tests/golden/exo_params.json */
    MMPC_MODEL_USER = 2          /* dynamics given as SX expressions to mahi::mpc::ModelGenerator
                                    (ModelGenerator.hpp:23; examples/ex_model_generate.cpp:36-43), compiled by
                                    compile_model() into the model's own <name>.so, which exports this same
                                    C-ABI for that one model (the JSON's dll_filepath, ModelGenerator.cpp:255) */
};

/* KKT solve of each SQP iteration (both solve the same Gauss-Newton QP exactly) */
enum mmpc_kkt_solver {
    MMPC_KKT_AUTO = 0,      /* by shape and batch: 2-link arm -- CONDENSED for N*nu <= 64 and
                               B <= 2560, RICCATI_GROUP up to B*N = 1e6, else RICCATI; exo -- RICCATI_GROUP
                               for B <= 4096 when two workgroups fit a CU's LDS, else RICCATI */
    MMPC_KKT_CONDENSED = 1, /* one wavefront per instance, condensed Hessian row per lane (N*nu <= 64) */
    MMPC_KKT_RICCATI = 2,   /* one lane per instance, Riccati recursion, any N (needs a workspace).  Unbounded
                               nonlinear solves of models with nx+nu < 16 hand instances still unconverged after
                               iteration 4 (or once at most 8 lanes of their wave are left) to a 16-lane resume
                               launch on the same stream that continues the same iterates; with
                               factor_fp32 that tail runs the fp64 factor; bounded solves hand over by the wave
                               rule alone (4 lanes), with their duals and barrier parameter (state bounds) or the
                               lane kernel's active-set rule (control bounds).  Policy: opts.tail_* (ABI 6) */
    MMPC_KKT_RICCATI_GROUP = 3 /* 16 lanes per instance: stage-parallel model evaluations and line search,
                                  serial Riccati sweeps from LDS (stage data of 4 instances <= 160 KB LDS) */
};

/* how a solve starts from V_inout (the converged KKT point does not depend on it) */
enum mmpc_init_states {
    MMPC_INIT_AS_GIVEN = 0, /* the reference: V as given (first call zeros, ModelControl.cpp:29-50; later the
                               previous solution, :160-161), x_0 pinned to the measured state */
    MMPC_INIT_HOLD_X0 = 1,  /* x_1..x_N start at the measured state x_0 (controls as given): a consistent-ish
                               state trajectory for cold starts, fewer SQP iterations */
    MMPC_INIT_ZERO = 2      /* the reference's first call, V = 0 with x_0 pinned (ModelControl.cpp:29-50), without
                               reading V_inout: a cold start needs no zeroed input (same iterates as AS_GIVEN on a
                               zero V) */
};

/* Hessian of each SQP subproblem.  The reference's IPOPT uses the exact Lagrangian Hessian by default
 * (hessian_approximation = exact; opts at ModelControl.cpp:54-59, nlp_hess_l generated at ModelGenerator.cpp:238).
 * Both choices converge to the same KKT point; they differ in the path and the iteration count. */
enum mmpc_hessian {
    MMPC_HESSIAN_AUTO = 0,         /* EXACT where supported and the model enables it by default (the built-in 2-link
                                      arm and SX-generated models; the exo keeps Gauss-Newton, whose small-residual
                                      fits converge in 3-5 iterations), else GAUSS_NEWTON */
    MMPC_HESSIAN_GAUSS_NEWTON = 1, /* J_F^T Q J_F + R terms: positive semidefinite, linear convergence for large
                                      tracking residuals */
    MMPC_HESSIAN_EXACT = 2         /* + h sum_r lam_{k+1,r} d^2 f_r/d(x_k,u_k)^2 per stage (lam: the QP adjoint);
                                      an iteration whose KKT matrix is not positive definite on the null space takes
                                      the Gauss-Newton step.  Supported: nonlinear solves of models with second
                                      derivatives (the built-in 2-link arm and exo, SX-generated models) on the
                                      RICCATI_GROUP solver (nx+nu < 16) and the RICCATI (lane) solver with its fp64
                                      factor, unbounded or with control bounds (the held controls are fixed in the
                                      exact QP; AUTO keeps Gauss-Newton for bounded solves); AUTO keeps Gauss-Newton
                                      for the exo and on the lane solver.  State bounds, linear mode, the fp32
                                      factor and any other solve return MMPC_ERR_UNSUPPORTED */
};

typedef struct mmpc_opts {
    int32_t max_iter;   /* SQP iteration cap. default 200 (the reference IPOPT option, ModelControl.cpp:55) */
    int32_t device;     /* HIP device ordinal; -1 = the calling thread's current device. default -1 */
    double tol_grad;    /* ||grad_u J_reduced||_inf stop tolerance. default 1e-8 */
    double tol_defect;  /* ||g||_inf stop tolerance. default 1e-10 */
    int32_t kkt_solver; /* enum mmpc_kkt_solver. default MMPC_KKT_AUTO */
    int32_t factor_fp32; /* 1: Riccati factor/solve in fp32, residuals/merit/iterates in fp64 (SURVEY 8d
                            cfg#5; each SQP iteration refines the fp32 step). Riccati solver only. default 0 */
    int32_t init_states; /* enum mmpc_init_states. default MMPC_INIT_AS_GIVEN */
    int32_t hessian;     /* enum mmpc_hessian. default MMPC_HESSIAN_AUTO (ABI 4) */
    /* Iteration-tail hand-over of the RICCATI (lane) solver (ABI 6; -1 = the default policy; the
     * environment variables MMPC_TAIL_CAP / MMPC_TAIL_WAVE / MMPC_TAIL_ROUNDS, read at mmpc_create, override them for
     * tests and A/B runs).  An instance still unconverged at the stop test of iteration tail_cap, or from iteration 2
     * on once at most tail_wave_max lanes of its 64-instance wave are still iterating, continues in a 16-lane resume
     * launch on the same stream, from the same iterate with the same algorithm.  The two kernels round differently,
     * so an instance's bits (and, within the stop test's roundoff, its iteration count) depend on whether it was
     * handed over -- which the wave rule decides by its wave-mates: the same instance solved alone (B = 1, the
     * calc_u case), inside another batch or in another shard of a multi-device solve agrees to 1e-10 relative in V*
     * (tests/test_gpu_tail.py), not bit for bit.  tail_cap = 0 turns the hand-over off: results then depend only on
     * the instance's own data. */
    int32_t tail_cap;      /* -1: 4 for unbounded solves, none (the wave rule alone) for bounded ones; 0: off */
    int32_t tail_wave_max; /* -1: 8 lanes (unbounded), 4 (bounded); 0: no wave rule; <= 64 */
    int32_t tail_rounds;   /* resume slots in rounds of up to 4 one-wave workgroups per CU; -1: 4 */
} mmpc_opts;

typedef struct mmpc_model_info {
    char name[128];
    int32_t model_id;           /* enum mmpc_model_id */
    int32_t num_x, num_u;       /* nx, nu */
    int32_t num_shooting_nodes; /* N */
    int32_t num_v;              /* NV = nx(N+1) + nu N */
    int32_t num_g;              /* NG = nx N */
    int32_t is_linear;
    double step_size;           /* h [s] */
    int64_t timespan_us;        /* h N in microseconds, as serialised */
    int64_t step_size_us;
    double u_min[16], u_max[16], x_min[16], x_max[16]; /* first nu / nx entries valid */
} mmpc_model_info;

int mmpc_abi_version(void);
void mmpc_default_opts(mmpc_opts* opts);

/* load <name>.json (ModelParameters schema); opts may be NULL (defaults) */
int mmpc_create(const char* model_json_path, const mmpc_opts* opts, mmpc_handle** out);
int mmpc_create_from_json(const char* json_text, const mmpc_opts* opts, mmpc_handle** out);
int mmpc_destroy(mmpc_handle* h);
int mmpc_get_model_info(const mmpc_handle* h, mmpc_model_info* info);
int mmpc_set_opts(mmpc_handle* h, const mmpc_opts* opts);
/* State bounds x_lb <= x_k <= x_ub for k = 1..N ([nx] host arrays, NULL = unbounded; |b| >= 1e19 is infinite),
 * the lbx/ubx IPOPT receives for the states (ModelControl.cpp:37-50,146-157).  A handle starts with the JSON's
 * x_min/x_max (ModelParameters.cpp:66-69: +-10e30 -> +-inf).  Finite state bounds make the solves run the
 * primal-dual interior-point variant (IPOPT-style barrier on the same Gauss-Newton model), which
 * then also handles u_lb/u_ub; it needs a Riccati solver (AUTO never picks CONDENSED for it). */
int mmpc_set_state_bounds(mmpc_handle* h, const double* x_lb, const double* x_ub);
int mmpc_get_state_bounds(const mmpc_handle* h, double* x_lb, double* x_ub);

/* Barrier-parameter rule of the interior point, i.e. of the solves with finite state bounds; every other solve ignores
 * it.  MONOTONE (the default): IPOPT's monotone rule, mu lowered when the barrier problem's error falls under
 * 10 mu.  MEHROTRA: Mehrotra's predictor-corrector -- each iteration solves its stage QPs twice with one set of
 * matrices (affine predictor, then a corrector with mu_t = (mu_aff / mu)^3 mu and the second-order terms), reaching the
 * same KKT points in about a third fewer iterations (cfg#2 shape, |qdot| <= 1.5, B = 4096: 9.1 mean / 20 max against
 * 13.4 / 29).  Measured on one MI355X it is nevertheless the SLOWER rule on that line: 2.11 ms against 1.50 ms per
 * batch with the Gauss-Newton Hessian (1.41x), 1.83 against 1.61 ms with the exact Hessian (1.14x) -- each iteration
 * costs about 1.5x.  MONOTONE is the faster rule on every line measured; MEHROTRA is opt-in.
 * Scope of MEHROTRA: the 16-lane solver (MMPC_KKT_RICCATI_GROUP, models with nx + nu < 16) in nonlinear mode, both
 * Hessians.  A state-bounded solve that resolves to the lane solver (MMPC_KKT_RICCATI, asked for or picked by AUTO)
 * or runs a linear-mode model returns MMPC_ERR_UNSUPPORTED; it is never run under the other rule.  The rule does not
 * change what MMPC_KKT_AUTO picks.  mmpc_reserve_workspace reserves for either rule, so setting the rule after a
 * reservation never makes a solve allocate.  An unknown value: MMPC_ERR_INVALID_ARG (mmpc_last_error names `rule`).
 * The environment variable MMPC_BARRIER_RULE (0 or 1), read when a handle is created, sets its initial rule
 * (measurement aid).  Handles of an mmpc_multi: through mmpc_multi_handle. */
enum mmpc_barrier_rule { MMPC_BARRIER_MONOTONE = 0, MMPC_BARRIER_MEHROTRA = 1 };
int mmpc_set_barrier_rule(mmpc_handle* h, int32_t rule);
int mmpc_get_barrier_rule(const mmpc_handle* h, int32_t* rule);

/* Pre-allocate the Riccati solvers' device workspace for batches up to B (so that later
 * stream-ordered solves allocate nothing; the workspace grows on demand otherwise; it includes the iteration-tail
 * hand-over list).  *bytes (may be NULL) receives the workspace size. */
int mmpc_reserve_workspace(mmpc_handle* h, int64_t B, uint64_t* bytes);

/* The KKT solver (enum mmpc_kkt_solver) a solve of B instances runs under the handle's options:
 * opts.kkt_solver, or what MMPC_KKT_AUTO picks for this model, horizon and B. */
int mmpc_resolve_kkt_solver(const mmpc_handle* h, int64_t B, int32_t* solver);

/* The Hessian (MMPC_HESSIAN_GAUSS_NEWTON or MMPC_HESSIAN_EXACT) a solve of B instances runs under the handle's
 * options; u_bounded = whether the solve passes control bounds (AUTO resolves control-bounded solves to
 * Gauss-Newton; an explicit EXACT is honoured with control bounds on RICCATI_GROUP and RICCATI).
 * MMPC_ERR_UNSUPPORTED when opts.hessian = EXACT cannot be honoured (CONDENSED, fp32 factor); state bounds: yes. */
int mmpc_resolve_hessian(const mmpc_handle* h, int64_t B, int32_t u_bounded, int32_t* hessian);

/* Batched SQP solve, DEVICE pointers, stream-ordered.  u_lb/u_ub: device [nu] or NULL
 * (unbounded; |bound| >= 1e19 is unbounded as in IPOPT).  Finite bounds are enforced (the lbx/ubx
 * of ModelControl.cpp:146-157): projected Gauss-Newton SQP, every returned u_k inside [u_lb, u_ub],
 * kkt_res = max(||U - P(U - grad)||_inf, ||g||_inf).  status/iters/kkt_res: device
 * [B] outputs, each may be NULL. */
int mmpc_solve_batch(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                     const double* traj, const double* weights, int64_t weights_stride,
                     const double* u_lb, const double* u_ub, double* V_inout, int32_t* status,
                     int32_t* iters, double* kkt_res, void* stream);

/* mmpc_solve_batch that also writes u_0* [B][nu] -- the control calc_u returns, V[b][nx:nx+nu]
 * (ModelControl.cpp:174-190) -- to u0_out (NULL = not written).  u0_out, status and iters may point into
 * memory from mmpc_host_alloc: the kernel then stores the per-tick results straight into host memory and they
 * are on the host when the stream's work completes (no copy kernel, no D2H; a controller loop reads them after
 * synchronising the stream).  Since ABI 5. */
int mmpc_solve_batch_u0(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                        const double* traj, const double* weights, int64_t weights_stride,
                        const double* u_lb, const double* u_ub, double* V_inout, int32_t* status,
                        int32_t* iters, double* kkt_res, double* u0_out, void* stream);

/* Pinned host memory mapped into every device's address space at the same address (hipHostMalloc mapped |
 * portable | coherent), for the outputs of mmpc_solve_batch_u0.  bytes = 0 gives *out = NULL.  Since ABI 5. */
int mmpc_host_alloc(uint64_t bytes, void** out);
int mmpc_host_free(void* p);

/* Same contract with HOST pointers; synchronous (H2D, solve, D2H on an internal stream). */
int mmpc_solve_batch_host(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                          const double* traj, const double* weights, int64_t weights_stride,
                          const double* u_lb, const double* u_ub, double* V_inout, int32_t* status,
                          int32_t* iters, double* kkt_res);

/* ---- per-instance control bounds (additive to ABI 6, as mmpc_set_barrier_rule was) ----
 * The reference's control limits belong to one controller: ModelControl::update_control_limits
 * (ModelControl.cpp:205-209) replaces that controller's u_min / u_max at run time and calc_u writes them into its own
 * lbx / ubx every tick (:147-157).  The *_bounds entry points carry B such limit sets through one launch: each is the
 * entry point above of the same name plus `bounds_stride` after u_ub, and the entry points above forward to them with
 * bounds_stride 0.
 *   bounds_stride == 0    u_lb / u_ub are [nu], shared by the batch (the meaning above).
 *   bounds_stride >= nu   instance b's row starts at b * bounds_stride in both arrays (one stride serves both); a
 *                         buffer of (B - 1) bounds_stride + nu doubles is enough and is never read past that (the
 *                         rule of the RCCL path's per-instance weights); columns nu .. bounds_stride - 1 are padding
 *                         that no kernel or scan reads.
 *   any other value       MMPC_ERR_INVALID_ARG, mmpc_last_error names `bounds_stride`; checked before any device call
 *                         (and, in the RCCL entry, before anything is sent).  The kernels take the stride as 32
 *                         bits: above 2^31 - 1 it is MMPC_ERR_UNSUPPORTED.
 * Shared-bounds solves run the kernels they ran before, unchanged; bounds_stride != 0 selects per-instance variants of
 * the bounded Riccati kernels (compiled separately: as per-lane values the bounds cost the shared-bounds solves
 * 3-10 %), the condensed kernel reads its row through a run-time stride.
 * Either pointer may be NULL as above (the RCCL entry keeps its "both or neither" rule).  |b| >= 1e19 is infinite per
 * element; an instance whose row is all infinite is solved by the bounded kernel with infinite bounds -- the kernel
 * is chosen per batch from the pointers, as above.  The host entries keep their "all infinite -> unbounded kernels"
 * rule over all B rows (a multi-device solve: over each shard's rows).  Every kernel reads the row of the INSTANCE,
 * also in the lane solver's resume launch (the hand-over list's slots are not instances).  State bounds stay per
 * handle. */
int mmpc_solve_batch_bounds(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                            const double* traj, const double* weights, int64_t weights_stride,
                            const double* u_lb, const double* u_ub, int64_t bounds_stride, double* V_inout,
                            int32_t* status, int32_t* iters, double* kkt_res, double* u0_out, void* stream);
/* HOST pointers, synchronous; stages (B - 1) bounds_stride + nu doubles per array when the bounds are strided */
int mmpc_solve_batch_host_bounds(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                                 const double* traj, const double* weights, int64_t weights_stride,
                                 const double* u_lb, const double* u_ub, int64_t bounds_stride, double* V_inout,
                                 int32_t* status, int32_t* iters, double* kkt_res);

/* ---- committed controls: pin the leading controls of the horizon (additive to ABI 6) ----
 * A controller that solves while the plant keeps moving (ModelControl::start_calc, ModelControl.cpp:83-112) publishes a
 * plan whose first controls have already been applied.  The reference began the cure -- ModelControl.hpp:79 keeps
 * m_num_control_inputs_saved and ModelControl.cpp:165-171 writes the first m controls of the last solution into lbx and
 * ubx -- but m is 0 without a setter and the next calc_u overwrites those bounds (:150-153).  The *_pinned entry points
 * pose what it meant: the same NLP with u_k = u_pin[b][k] for k < n_pin (lbx = ubx on those entries).  Each is the
 * *_bounds entry point of the same name plus `u_pin, n_pin` after bounds_stride.
 *   u_pin    [B][n_pin][nu], dense, instance-major (DEVICE memory for mmpc_solve_batch_pinned, host memory for the
 *            host entries): B controllers have B plans.  May be NULL when n_pin == 0.
 *   n_pin    0 .. N - 1.  0 forwards to the *_bounds entry point (the same bits as without pins).  n_pin < 0,
 *            n_pin > N - 1, or n_pin > 0 with u_pin == NULL: MMPC_ERR_INVALID_ARG, mmpc_last_error names `n_pin` /
 *            `u_pin`.  A linear-mode model (is_linear) with n_pin > 0: MMPC_ERR_UNSUPPORTED -- the reference linearises
 *            at the measured (x_0, u_prev), the reduced problem below would linearise at x_m; it is not run under the
 *            other meaning.  All checked from the arguments alone, before any device call, as bounds_stride is.
 * The pins override the control box as lbx = ubx would: a pinned value outside [u_lb, u_ub] is kept, not projected, and
 * gets no barrier slack.
 * How it is solved: with u_0..u_{m-1} fixed, x_1..x_m follow from x_0 by m Euler steps, and the rest is
 * the horizon-(N - m) problem from x_m with u_prev' = u_pin[b][m-1] and the targets traj[b][m:], solved by the same
 * kernels (the KKT solver and Hessian are resolved for the handle's own N; weights, control and state bounds, barrier
 * rule, init_states -- applied to the tail: HOLD_X0 holds at x_m -- tail_* and factor_fp32 act as on any solve).
 * What is written where: V_inout[b] = [x_0, u_pin_0, x_1, .., u_pin_{m-1}, x_m | the tail solution]; the warm start is
 * read from V_inout[b] from offset m (nx + nu) on; u0_out[b] = u_pin[b][0], the control in force now
 * (V[b][nx : nx + nu]); status / iters / kkt_res are those of the tail solve.  The x_1..x_m implied by the pins are NOT
 * checked against the state bounds (they are no decision of this solve); with finite state bounds an x_{m+1} that
 * cannot reach the box reports failure per instance, as an x_0 outside a position box does.  A non-finite pin gives
 * its own instance a non-converged status and leaves the others untouched.
 * Staging: B (nx + nu + (N - 1) nx + NV(N - 1)) doubles of the handle's workspace; mmpc_reserve_workspace(B) includes
 * them (whether or not pins are ever used), after which a pinned solve allocates nothing and can be captured in a
 * hipGraph.  The staging is per handle like the Riccati workspace -- also under MMPC_KKT_CONDENSED, whose unpinned
 * solves use no workspace: pinned solves of one handle go to one stream at a time.  The RCCL entry and mmpc/dist.py
 * take no pins (out of scope). */
int mmpc_solve_batch_pinned(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                            const double* traj, const double* weights, int64_t weights_stride,
                            const double* u_lb, const double* u_ub, int64_t bounds_stride, const double* u_pin,
                            int32_t n_pin, double* V_inout, int32_t* status, int32_t* iters, double* kkt_res,
                            double* u0_out, void* stream);
/* HOST pointers, synchronous; the pins travel with the other inputs */
int mmpc_solve_batch_host_pinned(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                                 const double* traj, const double* weights, int64_t weights_stride,
                                 const double* u_lb, const double* u_ub, int64_t bounds_stride, const double* u_pin,
                                 int32_t n_pin, double* V_inout, int32_t* status, int32_t* iters, double* kkt_res);

/* ---- feedback gains along the plan (additive to ABI 6) ----
 * A solve returns an open-loop plan: V*, published by the reference as control_results[i] = (time_i, x_est_i, u_i) and
 * read through ModelControl::control_at_time (ModelControl.cpp:174-197).  When the plant is not at x_est_i when u_i is
 * applied, the published control is off by (d u_i / d x_i) (x - x_est_i).  These entry points return the quantity that repairs it
 * to first order, the time-varying feedback gain at V:  u_i + G_i[:, :nx] (x_meas - x_est_i)  is the
 * neighbouring-extremal control (what RTI-style MPC applies between solves).
 *
 * Definition.  Take the tail problem from stage k: the stages k..N-1 of the NLP of ModelGenerator.cpp:191-222, from
 * x_k = x with u_{k-1} = v.  G_k in R^{nu x (nx+nu)} is d u_k / d(x, v) of its solution at (x_k*, u*_{k-1}), with
 * u*_{-1} = u_prev; by optimality the solution of the tail problem there is the plan's own tail.  With s = (dx, dv),
 * K = nx + nu and P_N = 0 (K x K), the recursion runs backward over k = N-1..0:
 *   A_k = I + h f_x, B_k = h f_u, e_k = F(x_k, u_k) - r_k;
 *   nu_k = 2 Q e_k + lam_k, with lam_{N-1} = 0 and lam_{k-1} = A_k^T nu_k (the multipliers of the defects);
 *   S_k = 2 [A_k|B_k]^T Q [A_k|B_k] on (x_k, u_k); with the exact Hessian, plus W_k = sum_r h nu_k[r] d^2 f_r/d(x,u)^2
 *   (the dynamics part of nlp_hess_l, ModelGenerator.cpp:238, as mmpc_nlp_hess_batch forms it);
 *   M = T^T P_{k+1} T + S_k placed on (dx, du) + 2R [[I, -I], [-I, I]] on (dv, du) + 2Rm on (du, du), where T maps
 *   (dx, dv, du) to s' = (A_k dx + B_k du, du).  The Delta-u term's further +2R on u_k for k + 1 < N (in
 *   mmpc_nlp_hess_batch's block) arrives through P_{k+1} and is not added twice;
 *   G_k = -M_uu^-1 M_us and P_k = M_ss - M_su M_uu^-1 M_us.
 * A control counts as held when u_k[c] equals its lower or upper bound bit for bit (the projected SQP returns exact
 * bound values; |b| >= 1e19 is infinite) or when k < n_pin (the committed controls of mmpc_solve_batch_pinned).  For a
 * held control its row and column of M_uu become identity, its row of M_us becomes zero, and G_k's row is exactly 0.
 * M_uu on the free controls is factorised by Cholesky.  A pivot that is <= 0 or non-finite at any stage under the exact
 * Hessian redoes the whole instance with Gauss-Newton, so no instance gets mixed Hessians.  Per instance:
 *   gain_status 0   as asked
 *               1   Gauss-Newton fallback
 *               2   failed (non-finite input, or not positive definite even with Gauss-Newton): all gains are written
 *                   as 0, i.e. pure feed-forward; neighbours in the batch are untouched
 * V need not be a solution: the gains are those of the quadratic model at the V given.
 *
 * Arguments.  V [B][NV], u_prev, traj, weights / weights_stride as for the solves.  u_lb, u_ub, bounds_stride follow
 * the mmpc_solve_batch_bounds rules exactly, stride validation included (either pointer may be NULL).
 *   n_pin     0 .. N - 1: stages k < n_pin are held.
 *   n_gain    1 .. N: the sweep always runs all N stages, n_gain only limits what is written.
 *   G_out     [B][n_gain][nu][nx+nu] row-major; columns 0..nx-1 are d u_k / d x_k, columns nx.. are d u_k / d u_{k-1}.
 *   hessian   enum mmpc_hessian.  AUTO means EXACT wherever the model has second derivatives -- the true derivative is
 *             wanted whatever Hessian the solve ran, so this is NOT mmpc_resolve_hessian.  GAUSS_NEWTON gives the
 *             iLQR / RTI gain.  EXACT on a model without second derivatives: MMPC_ERR_UNSUPPORTED.
 *   kernel    enum mmpc_gain_kernel.  LANE: one lane per instance, a single fused backward sweep without any workspace.
 *             GROUP: 16 lanes per instance (stage-parallel model evaluations, column j of the Riccati matrices on lane
 *             j), needs nx + nu < 16 and one instance's stage records within 160 KB of LDS -- MMPC_ERR_UNSUPPORTED
 *             otherwise.  AUTO: GROUP where it is available and its workgroups (up to 4 instances each, fewer when the
 *             LDS admits fewer) are at most two per compute unit, else LANE (measured).  The two kernels
 *             run the same operations per instance and agree to rounding, not bit for bit.
 *   gain_status   [B] or NULL.
 * Refused with MMPC_ERR_UNSUPPORTED, never run under another meaning: a linear-mode model; a handle with any finite
 * state bound whose sensitivity barrier is off (mmpc_set_sensitivity_barrier below; off is the state of every new
 * handle).  n_gain outside 1..N, n_pin outside 0..N-1, a bad
 * bounds_stride, an unknown hessian or kernel: MMPC_ERR_INVALID_ARG, mmpc_last_error names the argument.  Everything is
 * checked from the arguments alone before any device call; B = 0 is a no-op success.
 * mmpc_feedback_gains_batch takes DEVICE pointers, is stream-ordered on `stream`, never synchronises and never
 * allocates: neither kernel uses the handle's workspace (mmpc_reserve_workspace's sizes do not include anything for
 * it), so a gain launch can be captured in a hipGraph.  mmpc_feedback_gains_batch_host takes host pointers and is
 * synchronous.  Multi-device and RCCL entries: out of scope. */
enum mmpc_gain_kernel { MMPC_GAIN_KERNEL_AUTO = 0, MMPC_GAIN_KERNEL_LANE = 1, MMPC_GAIN_KERNEL_GROUP = 2 };
int mmpc_feedback_gains_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                              const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                              int64_t bounds_stride, int32_t n_pin, int32_t n_gain, int32_t hessian, int32_t kernel,
                              double* G_out, int32_t* gain_status, void* stream);
int mmpc_feedback_gains_batch_host(mmpc_handle* h, int64_t B, const double* V, const double* u_prev,
                                   const double* traj, const double* weights, int64_t weights_stride,
                                   const double* u_lb, const double* u_ub, int64_t bounds_stride, int32_t n_pin,
                                   int32_t n_gain, int32_t hessian, int32_t kernel, double* G_out,
                                   int32_t* gain_status);

/* ---- differentiable solve: reverse-mode products of the solution map (additive to ABI 6) ----
 * V* is a function of theta = (x0, u_prev, traj, weights).  Given a cotangent V_bar [NV] these entry points return
 * theta_bar = (d V* / d theta)^T V_bar for all of theta from one backward Riccati sweep with a vector part and one
 * forward sweep at V -- about the cost of one SQP iteration -- where finite differences take one solve per input.
 *
 * Definition.  Notation as for the feedback gains above: V = (x_0, u_0, .., x_N), K = nx + nu, A_k = I + h f_x,
 * B_k = h f_u, e_k = F(x_k, u_k) - r_k, C_k = [[A_k, B_k], [0, I]]; the stage blocks S_k (+ W_k with the exact Hessian),
 * the multipliers nu_k, lam_k and the held mask (bit-equal to a finite bound, or k < n_pin) are those of the gains.
 * Let z be the free entries of V (x_1..x_N and the controls not held), L = J + sum_k lam_k^T (F(x_k, u_k) - x_{k+1})
 * and g the defects.  (a, b) solves the symmetric system
 *     L_zz a + g_z^T b = V_bar_z,   g_z a = 0      (a = 0 on x_0 and on held controls),
 * the equality-constrained QP min 1/2 a^T L_VV a - V_bar^T a over the linearised dynamics from a_{x,0} = 0.  With
 * a_{x,k}, a_{u,k} its stage parts and a_{u,-1} = 0:
 *   traj_bar[k] = 2 Q o a_{x,k+1}
 *   Q_bar       = -2 sum_k e_k o a_{x,k+1}
 *   R_bar       = -2 sum_k (u_k - u_{k-1}) o (a_{u,k} - a_{u,k-1}),  u_{-1} = u_prev
 *   Rm_bar      = -2 sum_k u_k o a_{u,k}
 *   (x0_bar | u_prev_bar) = p_0 of the recursion below: 2 R o a_{u,0} for u_prev, V_bar_{x_0} minus the stage-0 cross
 *   terms for x0.
 * Recursion on s = (dx_k, dv = du_{k-1}), P_N = 0, p_N = (V_bar_{x_N}; 0), backward over k = N-1..0: M_uu, M_us, M_ss
 * and G_k exactly as in the gain definition;  q = C_k^T p_{k+1} + (V_bar_{x_k}; V_bar_{u_k});  q_u of a held control
 * is 0;  kff_k = M_uu^-1 q_u;  p_k = (q_x; 0) + G_k^T q_u;  P_k = M_ss + M_su G_k.  Forward from s_0 = 0:
 * a_{u,k} = G_k s_k + kff_k,  s_{k+1} = (A_k a_{x,k} + B_k a_{u,k}; a_{u,k}).
 * V_bar entries on held controls are ignored (derivatives with respect to the bounds and the pins are another
 * feature).  V need not be a solution: the outputs are those of the quadratic model at the V given.  Per instance:
 *   vjp_status 0   as asked
 *              1   Gauss-Newton fallback: a pivot <= 0 or non-finite under EXACT redoes the whole instance, both sweeps,
 *                  with Gauss-Newton
 *              2   failed (non-finite input, or not positive definite even with Gauss-Newton): every output row of the
 *                  instance is written as 0; neighbours in the batch are untouched
 *
 * Arguments.  V, u_prev, traj, weights / weights_stride, u_lb, u_ub, bounds_stride, n_pin: as for
 * mmpc_feedback_gains_batch, validation included.  V_bar [B][NV].
 *   hessian      enum mmpc_hessian.  AUTO means EXACT wherever the model has second derivatives, as for the gains;
 *                GAUSS_NEWTON is available and is NOT the true derivative.
 *   x0_bar       [B][nx]          u_prev_bar  [B][nu]          traj_bar  [B][N][nx]
 *   weights_bar  [B][nx+2nu], always per instance: a caller with shared weights sums the rows
 *   adj_V        [B][NV], the direction a
 *   vjp_status   [B]
 *   Every output and vjp_status may be NULL.
 *   workspace    DEVICE memory of mmpc_solve_vjp_workspace_bytes(h, B) bytes for the per-stage records G_k | kff_k
 *                (nu (K + 1) doubles per stage; ceil(B / 64) blocks of N nu (K + 1) x 64 doubles, lane-interleaved).  The
 *                kernel evaluates [A_k | B_k] again in the forward sweep, it is not stored.
 * Backward-only mode: when traj_bar, weights_bar and adj_V are all NULL no record is stored, no forward sweep runs and
 * workspace may be NULL; x0_bar and u_prev_bar are bit for bit those of the full call.  Otherwise a workspace that is
 * NULL or smaller than the query: MMPC_ERR_INVALID_ARG naming `workspace` / `workspace_bytes`.
 * Refused with MMPC_ERR_UNSUPPORTED: a linear-mode model; a handle with any finite state bound whose sensitivity
 * barrier is off (mmpc_set_sensitivity_barrier below).  n_pin outside 0..N-1,
 * a bad bounds_stride or weights_stride, an unknown hessian, a NULL V_bar: MMPC_ERR_INVALID_ARG, mmpc_last_error names
 * the argument.  Everything is checked from the arguments alone before any device call; B = 0 is a no-op success.
 * mmpc_solve_vjp_batch takes DEVICE pointers and is one stream-ordered launch on `stream` that never synchronises and
 * never allocates (the handle's workspace is not used; mmpc_reserve_workspace's sizes are unchanged), so it can be
 * captured in a hipGraph.  mmpc_solve_vjp_batch_host takes host pointers, stages them, brings its own workspace and is
 * synchronous.  Multi-device and RCCL entries, a 16-lane kernel: out of scope. */
int mmpc_solve_vjp_workspace_bytes(const mmpc_handle* h, int64_t B, uint64_t* bytes);
int mmpc_solve_vjp_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                         const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                         int64_t bounds_stride, int32_t n_pin, const double* V_bar, int32_t hessian, double* x0_bar,
                         double* u_prev_bar, double* traj_bar, double* weights_bar, double* adj_V, int32_t* vjp_status,
                         void* workspace, uint64_t workspace_bytes, void* stream);
int mmpc_solve_vjp_batch_host(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                              const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                              int64_t bounds_stride, int32_t n_pin, const double* V_bar, int32_t hessian,
                              double* x0_bar, double* u_prev_bar, double* traj_bar, double* weights_bar, double* adj_V,
                              int32_t* vjp_status);

/* ---- forward sensitivity of the solve: the first-order plan update (solve JVP; additive to ABI 6) ----
 * The forward-mode product dV = (d V* / d theta) d theta for theta = (x0, u_prev, traj, weights): when the measured
 * state, the applied control and the targets have all moved a little since the plan was computed, V* + dV is the plan
 * updated to first order (the feedback step of real-time iteration), and the best warm start of the next solve.
 *
 * Definition.  Notation of the gain and VJP comments above: A_k, B_k, J_k = [A_k | B_k], e_k = F(x_k, u_k) - r_k,
 * C_k, S_k (+ W_k), nu_k, lam_k, the held mask (bit-equal to a finite bound, or k < n_pin), M_uu, M_us, M_ss, G_k.
 * Tangents: dx0 [nx], du_prev [nu], dtraj [N][nx], dweights = (dQ | dR | dRm) [nx+2nu]; a missing tangent is zero.
 * Right-hand side, per stage on y_k = (x_k, u_k):
 *   rho_k = J_k^T (2 Q o dtraj_k - 2 dQ o e_k),
 *   plus on the u rows  - 2 dR o ((u_k - u_{k-1}) - (u_{k+1} - u_k)) - 2 dRm o u_k,
 *   with u_{-1} = u_prev and the (u_{k+1} - u_k) term absent at k = N-1;
 * rho is -d(grad_V L)/d theta d theta for traj and the weights; rho on x_N is 0.
 * Recursion: backward over k = N-1..0 from P_N = 0, p_N = 0, with P_k, M_*, G_k exactly as in the gains (with the
 * sensitivity barrier's terms when it is on):  q = C_k^T p_{k+1} + rho_k;  q_u of a held control is 0;
 * kff_k = M_uu^-1 q_u;  p_k = (q_x; 0) + G_k^T q_u.  Forward from s_0 = (dx0, du_prev):  du_k = G_k s_k + kff_k,
 * dx_{k+1} = A_k dx_k + B_k du_k,  s_{k+1} = (dx_{k+1}, du_k).  dV = (dx0, du_0, dx_1, .., dx_N).
 * Held controls have du = 0: the active set and the pins are assumed unchanged (the VJP's "V_bar on held controls is
 * ignored").  V need not be a solution: the result is that of the quadratic model at the V given.  Per instance:
 *   jvp_status 0   as asked
 *              1   Gauss-Newton fallback: a pivot <= 0 or non-finite under EXACT redoes the whole instance, both sweeps,
 *                  with Gauss-Newton
 *              2   failed (non-finite input, or not positive definite even with Gauss-Newton): every output row of the
 *                  instance is written as 0; neighbours in the batch are untouched
 *
 * Arguments.  V, u_prev, traj, weights / weights_stride, u_lb, u_ub, bounds_stride, n_pin: as for
 * mmpc_solve_vjp_batch, validation included.
 *   dx0 [B][nx]   du_prev [B][nu]   dtraj [B][N][nx]   dweights [B][nx+2nu], always per instance.
 *                Each may be NULL (zero); all four NULL: MMPC_ERR_INVALID_ARG.
 *   hessian      enum mmpc_hessian.  AUTO means EXACT wherever the model has second derivatives; GAUSS_NEWTON is
 *                available and is NOT the true derivative.
 *   dV           [B][NV] or NULL      du0  [B][nu] or NULL: du_0, the correction of the control about to be applied, for
 *                a state error and a target change together.  Both NULL: MMPC_ERR_INVALID_ARG.  With dV given, du0 is
 *                bit for bit the u_0 entries of dV.
 *   jvp_status   [B] or NULL.
 *   workspace    DEVICE memory of mmpc_solve_jvp_workspace_bytes(h, B) bytes for the records G_k | kff_k: the layout
 *                and the size of mmpc_solve_vjp_workspace_bytes.
 * Forward-free mode: when dV is NULL no record is stored, no forward sweep runs and workspace may be NULL; du0 is bit
 * for bit the full call's wherever both report status 0 or 1.  Otherwise a workspace that is NULL or smaller than the
 * query: MMPC_ERR_INVALID_ARG naming `workspace` / `workspace_bytes`.
 * Refused with MMPC_ERR_UNSUPPORTED: a linear-mode model; a handle with any finite state bound whose sensitivity
 * barrier is off.  The remaining rules, codes and argument names are the VJP's.  Everything is checked from the
 * arguments alone before any device call; B = 0 is a no-op success.
 * mmpc_solve_jvp_batch takes DEVICE pointers and is one stream-ordered launch on `stream` that never synchronises and
 * never allocates (the handle's workspace is not used; mmpc_reserve_workspace's sizes are unchanged), so it can be
 * captured in a hipGraph.  mmpc_solve_jvp_batch_host takes host pointers, stages them, brings its own workspace and is
 * synchronous.  Multi-device and RCCL entries, a 16-lane kernel, tangents of the bounds and the pins: out of scope. */
int mmpc_solve_jvp_workspace_bytes(const mmpc_handle* h, int64_t B, uint64_t* bytes);
int mmpc_solve_jvp_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                         const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                         int64_t bounds_stride, int32_t n_pin, const double* dx0, const double* du_prev,
                         const double* dtraj, const double* dweights, int32_t hessian, double* dV, double* du0,
                         int32_t* jvp_status, void* workspace, uint64_t workspace_bytes, void* stream);
int mmpc_solve_jvp_batch_host(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                              const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                              int64_t bounds_stride, int32_t n_pin, const double* dx0, const double* du_prev,
                              const double* dtraj, const double* dweights, int32_t hessian, double* dV, double* du0,
                              int32_t* jvp_status);

/* ---- real-time iteration: a prepare launch and a feedback launch per tick (additive to ABI 6) ----
 * One full-step SQP iteration at a plan V^ that is NOT a solution -- typically the previous solution shifted by one
 * stage -- split in two.  The preparation runs while the plant still moves towards the next sampling instant: it
 * linearises at V^, forms the gradient and the defects, runs the backward Riccati sweep and stores the stage records.
 * The feedback runs when x_0 is measured: one forward sweep over the records, no model, no factor.  (The solve JVP
 * above is the sensitivity of a converged plan: its right-hand side has no gradient residual and no defects.)
 *
 * Definition.  Notation of the gain, VJP and JVP comments, all at V^ = (x^_0, u^_0, x^_1, .., x^_N).  u_prev is the
 * control in force over the coming interval; it is known at prepare time.  With c_k = F(x^_k, u^_k) - x^_{k+1} the
 * step dV solves
 *   min 1/2 dV^T H dV + grad J(V^)^T dV
 *   s.t. dx_{k+1} = A_k dx_k + B_k du_k + c_k,   dx_0 = x0_meas - x^_0,   du_k = 0 on held controls,
 * H the Hessian of the Lagrangian (S_k, + W_k under EXACT, the -2R couplings) with the multipliers of the gain
 * recursion (lam_{N-1} = 0, lam_{k-1} = A_k^T nu_k, nu_k = 2 Q e_k + lam_k).  On the feasible set grad J^T dV and
 * grad L^T dV differ by a constant, and with these multipliers the x rows of grad L vanish; the u rows are
 *   r_{u,k} = B_k^T nu_k + 2R((u_k - u_{k-1}) - (u_{k+1} - u_k)) + 2Rm u_k,
 * u_{-1} = u_prev, the (u_{k+1} - u_k) term absent at k = N-1.  The held mask is the sensitivities': bit-equal to a
 * finite bound, or k < n_pin.
 * Recursion, with the cost-to-go written 1/2 s^T P_k s - p_k^T s (p has the sign of the JVP's p, so the recursion is the
 * JVP's with rho_k = -(0; r_{u,k}) - C_k^T P_{k+1} (c_k; 0)): backward over k = N-1..0 from P_N = 0, p_N = 0, with
 * P_k, M_*, G_k exactly as in the gains,
 *   q = C_k^T (p_{k+1} - P_{k+1} (c_k; 0)) - (0; r_{u,k});  q_u of a held control is 0;
 *   kff_k = M_uu^-1 q_u;  p_k = (q_x; 0) + G_k^T q_u.
 * Forward from s_0 = (dx_0; 0):  du_k = G_k s_k + kff_k,  dx_{k+1} = A_k dx_k + B_k du_k + c_k,  s_{k+1} = (dx_{k+1}; du_k).
 * Control box: with u_lb / u_ub given to the feedback call the forward sweep forms u_k+ = clamp(u^_k + du_k, lb, ub)
 * and propagates du_k = u_k+ - u^_k (the projected forward pass of box-iLQR); every returned control is inside the box
 * bit for bit.  A du_k that is exactly 0 -- a held control has a zero row of G_k and kff 0 -- leaves the control as it
 * is, so a pinned control keeps its value whatever the box.
 * Output: V_inout = V^ + dV with V[0:nx] bit for bit x0_meas; u0_out = u_0+, bit for bit V_inout's u_0; step_inf =
 * max |V_inout - V^| over the entries as stored.  The step is the full step: no line search.  Per instance:
 *   status 0   as asked
 *          1   Gauss-Newton fallback: a pivot <= 0 or non-finite under EXACT redoes the whole preparation of the instance
 *              with Gauss-Newton
 *          2   failed: decided at prepare time for a non-finite input or a step that is not positive definite even with
 *              Gauss-Newton, at feedback time for a non-finite x0_meas or a non-finite step.  V_inout is left bit for
 *              bit as given, u0_out is the plan's own u^_0, step_inf is +inf (no step was taken; a caller that
 *              thresholds step_inf alone falls back to a full solve); neighbours in the batch are untouched.
 *   prep_status reports 0 / 1 / 2 as far as the preparation knows; the feedback call's status carries it on.
 *
 * Arguments.  V, u_prev, traj, weights / weights_stride, u_lb, u_ub, bounds_stride, n_pin, hessian: as for
 * mmpc_solve_jvp_batch, validation (codes and the argument names in mmpc_last_error) included.  x0_meas [B][nx];
 * V_inout [B][NV], holding the plan the preparation was given; u0_out [B][nu], step_inf [B], status [B], prep_status [B]
 * may each be NULL.  u0_out, step_inf and status may point into mmpc_host_alloc memory, as for mmpc_solve_batch_u0.
 * The feedback call takes no model inputs: the preparation's status, n_pin and the held mask reach it through the
 * workspace.  Its u_lb / u_ub / bounds_stride are the box of the clamp (normally the preparation's).
 *   workspace    caller-provided DEVICE memory of mmpc_rti_workspace_bytes(h, B) bytes, K = nx + nu:
 *                  ceil(B / 64) * 64 * ((N K (K + 1) + NV) * 8 + 4)  bytes:
 *                per stage the record G_k | kff_k (nu rows of K + 1) and A_k | B_k | c_k (nx rows of K + 1), K (K + 1)
 *                doubles (156 N per instance for the exo), lane-interleaved in blocks of 64 instances in the layout of
 *                the VJP's record; then NV doubles per instance in which the feedback launch keeps the plan entries it
 *                overwrites, so that a failed step can be undone; then one int32 status word per instance.  The stored
 *                A | B | c are the price of a feedback sweep that evaluates no model.
 *                NULL or smaller than the query: MMPC_ERR_INVALID_ARG naming `workspace` / `workspace_bytes`.
 * A feedback call on a workspace that no prepare call of the same handle and B has filled, or with a V_inout that is
 * not the plan that prepare call was given, is the caller's error and is not detected.  One preparation serves one
 * feedback call on that plan.
 * Refused with MMPC_ERR_UNSUPPORTED: a linear-mode model; a handle with any finite state bound, whether the sensitivity
 * barrier is on or off (a one-step interior point is not computed).  Everything is checked from the arguments alone
 * before any device call; B = 0 is a no-op success.
 * mmpc_rti_prepare_batch and mmpc_rti_feedback_batch take DEVICE pointers; each is one stream-ordered launch on
 * `stream` that never synchronises and never allocates (the handle's workspace is not used; mmpc_reserve_workspace's
 * sizes are unchanged), so both can be captured in a hipGraph.  mmpc_rti_step_batch_host takes host pointers, runs
 * preparation and feedback back to back, brings its own workspace and is synchronous.  State-bounded handles,
 * inequality constraints beyond the clamp, multi-device and RCCL entries, a 16-lane kernel, globalisation: out of
 * scope. */
int mmpc_rti_workspace_bytes(const mmpc_handle* h, int64_t B, uint64_t* bytes);
int mmpc_rti_prepare_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                           const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                           int64_t bounds_stride, int32_t n_pin, int32_t hessian, int32_t* prep_status,
                           void* workspace, uint64_t workspace_bytes, void* stream);
int mmpc_rti_feedback_batch(mmpc_handle* h, int64_t B, const double* x0_meas, const double* u_lb, const double* u_ub,
                            int64_t bounds_stride, double* V_inout, double* u0_out, double* step_inf, int32_t* status,
                            void* workspace, uint64_t workspace_bytes, void* stream);
int mmpc_rti_step_batch_host(mmpc_handle* h, int64_t B, double* V_inout, const double* x0_meas, const double* u_prev,
                             const double* traj, const double* weights, int64_t weights_stride, const double* u_lb,
                             const double* u_ub, int64_t bounds_stride, int32_t n_pin, int32_t hessian, double* u0_out,
                             double* step_inf, int32_t* status);

/* ---- the shift between two ticks of a real-time iteration loop (additive to ABI 6) ----
 * V_out is V_in moved n = n_shift stages earlier, per instance, K = nx + nu:
 *   stages k = 0 .. N-n-1 of V_out (x_k, u_k) and the state x_{N-n} are stages k + n of V_in and its x_N, bit for bit;
 *   every later control is the old u_{N-1}, bit for bit;
 *   every later state is rolled out, x_{k+1} = F(x_k, u_{N-1}) = x_k + h f(x_k, u_{N-1}): the Euler step of the NLP's
 *   defects, evaluated by the model's own device function.
 * u_prev_out [B][nu] (may be NULL) receives the old u_{n-1}, the control in force over the new first interval, which
 * is the u_prev of a preparation at V_out.  With n = 0 V_out is a copy of V_in and u_prev_out is not written.
 * V_in and V_out [B][NV] are DEVICE pointers and may not overlap (V_out == V_in is refused; a partial overlap is the
 * caller's error).  One stream-ordered launch on `stream` that never synchronises, never allocates and uses no
 * workspace, so it can be captured in a hipGraph.  A non-finite entry propagates into its own row only.
 * MMPC_ERR_INVALID_ARG: n_shift outside 0 .. N (mmpc_last_error names `n_shift`), a NULL V_in or V_out (named),
 * V_out == V_in.  MMPC_ERR_UNSUPPORTED: a linear-mode model, as for the entries above.  Everything is checked from the
 * arguments alone before any device call.  n_shift and the model's mode are properties of the call, not of the data, and
 * are checked first: B = 0 with a valid n_shift on a nonlinear model is a no-op success whatever the pointers are, B = 0
 * with a bad n_shift or a linear-mode model is still the error above.  A state-bounded handle is accepted, since the
 * shifted plan is also the warm start of a solve; the rolled-out states are NOT checked against any state bound and
 * may lie outside the box. */
int mmpc_rti_shift_batch(mmpc_handle* h, int64_t B, const double* V_in, int32_t n_shift, double* V_out,
                         double* u_prev_out, void* stream);

/* ---- feedback gains and solve VJP of a state-bounded handle: the sensitivity barrier (additive to ABI 6) ----
 * A state-bounded solve is an interior-point solve: the V it returns lies strictly inside every bound, near the
 * central path of its last barrier value.  Its sensitivity is the recursion of the two definitions above with the
 * barrier's Hessian on the diagonal of the bounded rows and the barrier's gradient in the multiplier recursion.
 *
 * Definition.  Notation of the gain and VJP comments; for a handle with at least one finite state bound and the
 * sensitivity barrier switched on, with parameters mu_s > 0 and sigma_cap > 0:
 *   Bounded variables are those the interior-point solve bounds: x_{k+1} for k = 0..N-1 under the handle's state
 *   bounds, u_k under u_lb / u_ub / bounds_stride of the call; |b| >= 1e19 is infinite.  x_0 has no term.  Controls of
 *   stages k < n_pin are held exactly as above and get no term.  No control is held by bit-equality on such a handle:
 *   the interior point never returns a control on its bound.
 *   Per bounded entry y with slacks s_l = y - l, s_u = u - y (a side whose bound is infinite contributes nothing):
 *     beta = 2 mu_s (1 / s_u - 1 / s_l),   D = min(2 mu_s (1 / s_l^2 + 1 / s_u^2), sigma_cap)
 *   (the J scale: the barrier objective is J - 2 mu sum log s).
 *   Multipliers: lam_{N-1} = beta(x_N), lam_{k-1} = A_k^T nu_k + beta(x_k), nu_k = 2 Q e_k + lam_k; W_k uses these
 *   nu_k; Gauss-Newton ignores beta.
 *   Recursion: P_{k+1}[x, x] += diag D(x_{k+1}) before T^T P_{k+1} T is formed; M_uu += diag D(u_k) on the controls
 *   not pinned; everything else is as written above.  The VJP's q, kff, p, its forward sweep and its output formulas
 *   are unchanged: the barrier term does not depend on theta.
 *   Status: a bounded entry with a slack that is <= 0 or not finite gives the instance status 2, with the all-zero /
 *   neighbours-untouched rules above.  The Gauss-Newton fallback (status 1) is unchanged.
 * Meaning: the derivative of the mu_s-barrier problem's solution at the V given.  With mu_s the barrier value the solve
 * ended at, that is the derivative of the solve's own map.  mmpc_sensitivity_barrier_default returns the value the
 * monotone rule reaches first with 2 mu <= its complementarity tolerance (2.5e-9, computed from the solver's
 * schedule) and sigma_cap = 1e12.  Caveat: an instance that needed a further decrease of mu ends at the floor 5e-10,
 * and Mehrotra's rule ends at a per-instance value; for those the multipliers in W_k are an estimate, and mu_s is the
 * caller's to set.  sigma_cap bounds the condition of the recursion (the slacks of an active bound reach 1e-12, D
 * 1e16) and is part of the meaning: against central differences of the solve the gains agree to 5e-7 at 1e12 and
 * without a cap, to 5e-5 at 1e10, and not at all at 1e6, a value for checking the arithmetic only.
 *
 * mmpc_set_sensitivity_barrier: mu = 0 switches the barrier off (the state of every new handle: the gain and VJP calls
 * refuse a state-bounded handle), mu > 0 switches it on.  A non-finite or negative mu, a sigma_cap that is <= 0 or NaN:
 * MMPC_ERR_INVALID_ARG naming the argument; sigma_cap = +inf is allowed (no cap).  On a handle without a finite state
 * bound the setting has no effect at all.  With it on, mmpc_feedback_gains_batch[_host] and
 * mmpc_solve_vjp_batch[_host] accept the handle with the same signatures and launch rules (no allocation, no
 * synchronisation, hipGraph capture; mmpc_solve_vjp_workspace_bytes and mmpc_reserve_workspace unchanged); the
 * 16-lane gain kernel's stage records grow by 2 nx + nu doubles, and its availability and the AUTO rule are evaluated
 * with that size.  mmpc_solve_jvp_batch[_host] accept it on the same terms: its right-hand side does not depend on
 * the barrier.  Gradients with respect to the bounds, a per-instance mu_s: out of scope. */
int mmpc_sensitivity_barrier_default(double* mu, double* sigma_cap);
int mmpc_set_sensitivity_barrier(mmpc_handle* h, double mu, double sigma_cap);
int mmpc_get_sensitivity_barrier(const mmpc_handle* h, double* mu, double* sigma_cap);

/* Continuous-time linearisation at (x[b], u[b]): A = df/dx [nx*nx], B = df/du [nx*nu]
 * column-major, xdot = f(x,u) [nx].  DEVICE pointers; any output may be NULL. */
int mmpc_linearize_batch(mmpc_handle* h, int64_t B, const double* x, const double* u,
                         double* A_colmajor, double* B_colmajor, double* xdot, void* stream);
int mmpc_linearize_batch_host(mmpc_handle* h, int64_t B, const double* x, const double* u,
                              double* A_colmajor, double* B_colmajor, double* xdot);

/* NLP value at V: J (ModelGenerator.cpp:208-222) and max |g| (g of :206).  DEVICE pointers. */
int mmpc_nlp_eval_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev,
                        const double* traj, const double* weights, int64_t weights_stride,
                        double* J, double* defect_inf, void* stream);

/* nlp_grad_f / nlp_jac_g of the reference's generated NLP (ModelGenerator.cpp:238; CasADi generate_dependencies)
 * at V: J [B], dJ/dV [B][NV] (V layout) and the nonzero Jacobian blocks of the defects g_k = F(x_k,u_k) - x_{k+1},
 * [dg_k/dx_k | dg_k/du_k] = [I + h df/dx | h df/du] as [B][N][nx][nx+nu] row-major (dg_k/dx_{k+1} = -I).
 * DEVICE pointers; any output may be NULL. */
int mmpc_nlp_derivs_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev,
                          const double* traj, const double* weights, int64_t weights_stride,
                          double* J, double* grad, double* jac_blocks, void* stream);

/* nlp_hess_l of the reference's generated NLP (ModelGenerator.cpp:238; CasADi generate_dependencies): the Hessian of
 * the Lagrangian lam_f J + lam_g^T g at V.  Output: the nonzero stage blocks on (x_k, u_k), [B][N][K][K] row-major
 * (K = nx + nu, symmetric); the remaining nonzeros are constant, d^2 L / du_k du_{k-1} = -2 lam_f R, and x_N enters
 * L linearly.  lam_g: DEVICE [B][N*nx] (g order, ModelGenerator.cpp:206) or NULL (zeros).  Needs second derivatives
 * of the dynamics (built-in 2-link arm, SX-generated models; linear mode always): MMPC_ERR_UNSUPPORTED otherwise. */
int mmpc_nlp_hess_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev,
                        const double* traj, const double* weights, int64_t weights_stride, double lam_f,
                        const double* lam_g, double* hess_blocks, void* stream);

/* Synthetic instances: cfg#2 recipe for the 2-link arm, cfg#3 recipe for the exo;
 * counter-based splitmix64(seed, first_index + b), so shards generate identical instances
 * whatever the GPU count.  DEVICE pointers. */
int mmpc_synth_batch(mmpc_handle* h, uint64_t seed, int64_t first_index, int64_t B, double* x0,
                     double* u_prev, double* traj, void* stream);

/* ---- one process, several devices (the reference's per-instance worker loop of
 *      ModelControl.cpp:75-112, batched and sharded) ----
 * Contiguous split of B instances over n shards: shard i = [floor(i B / n), floor((i+1) B / n)) (first, count);
 * the same partition as the multi-process path (mmpc/dist.py shard_strong).  Pure arithmetic, no device. */
int mmpc_shard(int64_t B, int32_t n, int32_t i, int64_t* first, int64_t* count);

typedef struct mmpc_multi mmpc_multi;
/* One handle per listed device ordinal (each with its own stream, workspace and staging; a device may be listed
 * more than once: its shards then run on concurrent streams).  opts.device is ignored. */
int mmpc_multi_create(const char* model_json_path, const mmpc_opts* opts, const int32_t* devices, int32_t n_devices,
                      mmpc_multi** out);
int mmpc_multi_destroy(mmpc_multi* m);
int mmpc_multi_num_devices(const mmpc_multi* m, int32_t* n);
/* the handle of shard g (to reserve workspace, set state bounds or options device by device) */
int mmpc_multi_handle(mmpc_multi* m, int32_t g, mmpc_handle** h);
/* mmpc_solve_batch_host contract for the whole batch: shard g = mmpc_shard(B, n_devices, g) is solved on device g
 * (H2D, solve, D2H on that device's stream, all devices concurrently) straight from/into the caller's arrays;
 * synchronous.  Results equal a single-device solve of each shard bit for bit; against a single-device solve of the
 * whole batch they are bit for bit except where the RICCATI solver's iteration-tail hand-over decides differently
 * for a different wave composition (opts.tail_cap: 1e-10 relative in V*, tests/test_gpu_multi.py). */
int mmpc_multi_solve_batch_host(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                const double* traj, const double* weights, int64_t weights_stride,
                                const double* u_lb, const double* u_ub, double* V_inout, int32_t* status,
                                int32_t* iters, double* kkt_res);

/* The same solve through RCCL (SURVEY.md 8e's single-process design; replaces the per-tick m_solver call of
 * ModelControl.cpp:159 for a batch resident on one GPU): DEVICE pointers on the multi handle's FIRST device; shard g
 * (mmpc_shard) of every input goes to device g by ncclSend/ncclRecv, shared weights and u_lb/u_ub (device [nu] or
 * NULL) by ncclBroadcast, every device solves its shard, and V / status / iters / kkt_res come back to the first
 * device by ncclSend/ncclRecv (ncclCommInitAll over the listed devices at the first call).  The devices must be
 * distinct (RCCL refuses a device listed twice: MMPC_ERR_UNSUPPORTED); RCCL is loaded with dlopen at the first call
 * (MMPC_ERR_UNSUPPORTED when librccl is absent).  `stream` (hipStream_t on the first device, NULL = the null
 * stream): the call's first RCCL operation is ordered after the work already queued there, and work queued there
 * later sees the results.  Per-instance weights (weights_stride >= nx + 2 nu) need (B - 1) weights_stride + nx + 2 nu
 * doubles.  Every RCCL operation's result is checked; after an error every stream of the call is drained before the
 * call returns.  Synchronous; results as mmpc_multi_solve_batch_host's.  `stream` must belong to the first device
 * (MMPC_ERR_INVALID_ARG otherwise). */
int mmpc_multi_solve_batch_rccl(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                const double* traj, const double* weights, int64_t weights_stride,
                                const double* u_lb, const double* u_ub, double* V_inout, int32_t* status,
                                int32_t* iters, double* kkt_res, void* stream);
/* The two multi-device solves with per-instance control bounds (bounds_stride: see mmpc_solve_batch_bounds).  The host
 * entry gives shard g the rows from first * bounds_stride on.  The RCCL entry sends each shard's rows by
 * ncclSend/ncclRecv (the last row up to its nu entries, so (B - 1) bounds_stride + nu doubles are never over-read), as
 * it does for per-instance weights, and keeps ncclBroadcast for bounds_stride 0. */
int mmpc_multi_solve_batch_host_bounds(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                       const double* traj, const double* weights, int64_t weights_stride,
                                       const double* u_lb, const double* u_ub, int64_t bounds_stride, double* V_inout,
                                       int32_t* status, int32_t* iters, double* kkt_res);
int mmpc_multi_solve_batch_rccl_bounds(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                       const double* traj, const double* weights, int64_t weights_stride,
                                       const double* u_lb, const double* u_ub, int64_t bounds_stride, double* V_inout,
                                       int32_t* status, int32_t* iters, double* kkt_res, void* stream);
/* mmpc_multi_solve_batch_host_bounds with committed controls (u_pin [B][n_pin][nu] host memory, n_pin: see
 * mmpc_solve_batch_pinned): shard g gets the rows from first * n_pin * nu on.  The RCCL entry takes no pins. */
int mmpc_multi_solve_batch_host_pinned(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                       const double* traj, const double* weights, int64_t weights_stride,
                                       const double* u_lb, const double* u_ub, int64_t bounds_stride,
                                       const double* u_pin, int32_t n_pin, double* V_inout, int32_t* status,
                                       int32_t* iters, double* kkt_res);
/* the version of the RCCL library the RCCL entries load (ncclGetVersion, e.g. 22606), MMPC_ERR_UNSUPPORTED if none */
int mmpc_rccl_version(int32_t* version);

const char* mmpc_status_string(int32_t status);
/* thread-local description of the last API error on this thread ("" if none) */
const char* mmpc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MMPC_H */
