// mmpc.hip -- C-ABI (include/mmpc.h) of the MI355X batched NMPC solve path.
//
// Host side of the drop-in boundary: loads the reference's <name>.json model file
// (src/Mahi/Mpc/ModelParameters.cpp:52-72 semantics), validates every launch shape on
// the host, and launches the gfx950 kernels of sqp_wave.h / below.  No CPU fallback
// exists: every compute entry point runs on the GPU or returns an error.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <thread>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only: RCCL itself is loaded with dlopen at the first RCCL call

#include "../../include/mmpc.h"
#include "json_lite.h"
#include "adjoint_sweep.h"
#include "tangent_sweep.h"
#include "rti_sweep.h"
#include "gain_sweep.h"
#include "group_launch.h"
#include "lane_launch.h"
#include "models.h"
#include "sqp_group.h"
#include "sqp_lane.h"
#include "sqp_wave.h"

// A library built by ModelGenerator::compile_model for SX-defined dynamics (mahi-mpc's <name>.so,
// ModelGenerator.cpp:254-259) compiles this same file with -DMMPC_USER_MODEL_HEADER="<name>_model.h", which
// defines mmpc::UserModel; it then serves that one model (MMPC_MODEL_USER) and none of the built-in ones.
#ifdef MMPC_USER_MODEL_HEADER
#include MMPC_USER_MODEL_HEADER
#define MMPC_BUILTIN_MODELS 0
#else
#define MMPC_BUILTIN_MODELS 1
#endif

using namespace mmpc;

// ---------------------------------------------------------------- errors
namespace {
thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
int hip_fail(hipError_t e, const char* where) {
    return fail(MMPC_ERR_HIP, std::string(where) + ": " + hipGetErrorString(e));
}
#define MMPC_HIP(call)                                    \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)
}  // namespace

// ---------------------------------------------------------------- handle
struct mmpc_handle {
    mmpc_model_info info;
    int nq = 0;  // kinematic rows of the model's dynamics (sqp_lane.h a_mul)
    mmpc_opts opts;
    std::mutex host_mu;  // serialises the *_host entry points
    hipStream_t host_stream = nullptr;
    int host_dev = -1;
    // device staging for the *_host entry points (grown on demand)
    double* d_buf = nullptr;
    size_t d_buf_bytes = 0;
    // Riccati solver workspace (SoA, sqp_lane.h LaneLayout), grown on demand
    std::mutex ws_mu;
    double* ws = nullptr;
    size_t ws_bytes = 0;
    int ws_dev = -1;
    // iteration-tail hand-over: cap override from MMPC_TAIL_CAP at creation (-1: the default policy),
    // compute units of the device (slots of the resume launch)
    int tail_cap_env = -1;      // MMPC_TAIL_CAP (test / A/B override of opts.tail_cap; -1: not set)
    int tail_wave_env = -1;     // MMPC_TAIL_WAVE (override of opts.tail_wave_max)
    int tail_rounds_env = -1;   // MMPC_TAIL_ROUNDS (override of opts.tail_rounds)
    int cu_count = 0;
    // state bounds of x_1..x_N (JSON x_min/x_max, or mmpc_set_state_bounds); copied into each launch's arguments
    double x_lb[16], x_ub[16];
    bool x_bounded = false;
    // barrier rule of the interior point (mmpc_set_barrier_rule, MMPC_BARRIER_RULE at creation); read with the bounds
    int barrier_rule = MMPC_BARRIER_MONOTONE;
    // sensitivity barrier of the gain and VJP calls (mmpc_set_sensitivity_barrier): sens_mu = 0 is off; read with the
    // bounds
    double sens_mu = 0.0, sens_cap = 1e12;
    std::mutex xb_mu;
};

namespace {

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    int err = 0;
    // A failed call here is reported by the entry point (MMPC_ERR_NO_DEVICE); HIP also keeps it as the thread's last
    // error, where the hipGetLastError() after a later, healthy kernel launch of this thread would find it: cleared.
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) {
            (void)hipGetLastError();
            err = 1;
            return;
        }
        if (dev >= 0 && dev != prev) {
            if (hipSetDevice(dev) != hipSuccess) {
                (void)hipGetLastError();
                err = 1;
                return;
            }
            changed = true;
        }
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

int parse_model(const std::string& text, mmpc_model_info* info) {
    json::Value root;
    try {
        root = json::parse(text);
    } catch (const std::exception& ex) {
        return fail(MMPC_ERR_PARSE, ex.what());
    }
    const json::Value* m = root.get("model");  // ModelGenerator.cpp:264 writes j["model"]
    if (!m) m = &root;
    if (m->kind != json::Value::Object) return fail(MMPC_ERR_PARSE, "model entry is not an object");
    auto num = [&](const char* k, double* out) -> bool {
        const json::Value* v = m->get(k);
        if (!v || v->kind != json::Value::Number) return false;
        *out = v->num;
        return true;
    };
    std::memset(info, 0, sizeof(*info));
    const json::Value* nm = m->get("name");
    if (!nm || nm->kind != json::Value::String) return fail(MMPC_ERR_PARSE, "missing \"name\"");
    std::snprintf(info->name, sizeof(info->name), "%s", nm->str.c_str());
    double nx, nu, N, step_us, span_us = 0.0;
    if (!num("num_x", &nx) || !num("num_u", &nu) || !num("num_shooting_nodes", &N) || !num("step_size", &step_us))
        return fail(MMPC_ERR_PARSE, "missing num_x / num_u / num_shooting_nodes / step_size");
    num("timespan", &span_us);
    info->num_x = static_cast<int32_t>(nx);
    info->num_u = static_cast<int32_t>(nu);
    info->num_shooting_nodes = static_cast<int32_t>(N);
    if (info->num_x < 1 || info->num_x > 16 || info->num_u < 1 || info->num_u > 16 || info->num_shooting_nodes < 1)
        return fail(MMPC_ERR_PARSE, "num_x / num_u / num_shooting_nodes out of range");
    info->step_size_us = static_cast<int64_t>(std::llround(step_us));
    info->timespan_us = static_cast<int64_t>(std::llround(span_us));
    info->step_size = step_us * 1e-6;  // mahi::util::microseconds(j.at("step_size"))
    info->num_v = info->num_x * (info->num_shooting_nodes + 1) + info->num_u * info->num_shooting_nodes;
    info->num_g = info->num_x * info->num_shooting_nodes;
    const json::Value* lin = m->get("is_linear");
    info->is_linear = (lin && lin->kind == json::Value::Bool && lin->b) ? 1 : 0;
    // bounds: default +-10e30 (ModelParameters.cpp:21-24); x bounds of exactly +-10e30 become +-inf on
    // load (ModelParameters.cpp:66-69); nlohmann writes +-inf as null, read back here as unbounded.
    auto bounds = [&](const char* k, double* out, int n, double dflt, bool inf_map) -> int {
        for (int i = 0; i < n; ++i) out[i] = dflt;
        const json::Value* v = m->get(k);
        if (!v || v->kind == json::Value::Null) return 0;
        if (v->kind != json::Value::Array) return fail(MMPC_ERR_PARSE, std::string(k) + " is not an array");
        if (static_cast<int>(v->arr.size()) != n && !v->arr.empty())
            return fail(MMPC_ERR_PARSE, std::string(k) + " has the wrong length");
        for (size_t i = 0; i < v->arr.size(); ++i) {
            const json::Value& e = v->arr[i];
            if (e.kind == json::Value::Null) out[i] = dflt;
            else if (e.kind == json::Value::Number) out[i] = e.num;
            else return fail(MMPC_ERR_PARSE, std::string(k) + " has a non-number entry");
            if (inf_map && std::fabs(out[i]) == 10e30) out[i] = std::copysign(INFINITY, out[i]);
        }
        return 0;
    };
    int rc;
    if ((rc = bounds("x_min", info->x_min, info->num_x, -INFINITY, true))) return rc;
    if ((rc = bounds("x_max", info->x_max, info->num_x, INFINITY, true))) return rc;
    if ((rc = bounds("u_min", info->u_min, info->num_u, -10e30, false))) return rc;
    if ((rc = bounds("u_max", info->u_max, info->num_u, 10e30, false))) return rc;
    // dynamics: explicit "mmpc_model" key, else the only built-in model with these dimensions
    const json::Value* mdl = m->get("mmpc_model");
#if !MMPC_BUILTIN_MODELS
    // a generated library serves exactly its own model
    if (mdl && mdl->kind == json::Value::String && mdl->str != UserModel::kName)
        return fail(MMPC_ERR_UNSUPPORTED, "this library was generated for model \"" + std::string(UserModel::kName) +
                                              "\", not \"" + mdl->str + "\"");
    if (info->num_x != UserModel::NX || info->num_u != UserModel::NU)
        return fail(MMPC_ERR_PARSE, "num_x / num_u differ from the generated model's dimensions");
    info->model_id = MMPC_MODEL_USER;
    return MMPC_OK;
#endif
    if (mdl && mdl->kind == json::Value::String) {
        if (mdl->str == "two_link_arm" || mdl->str == "double_pendulum") info->model_id = MMPC_MODEL_TWO_LINK_ARM;
        else if (mdl->str == "exo_arm" || mdl->str == "exo") info->model_id = MMPC_MODEL_EXO_ARM;
        else return fail(MMPC_ERR_UNSUPPORTED, "unknown mmpc_model \"" + mdl->str + "\"");
    } else if (info->num_x == 4 && info->num_u == 2) {
        info->model_id = MMPC_MODEL_TWO_LINK_ARM;
    } else if (info->num_x == 8 && info->num_u == 4) {
        info->model_id = MMPC_MODEL_EXO_ARM;
    } else {
        return fail(MMPC_ERR_UNSUPPORTED, "no built-in dynamics for these dimensions (set \"mmpc_model\")");
    }
    if (info->model_id == MMPC_MODEL_TWO_LINK_ARM && (info->num_x != 4 || info->num_u != 2))
        return fail(MMPC_ERR_PARSE, "two_link_arm needs num_x = 4, num_u = 2");
    if (info->model_id == MMPC_MODEL_EXO_ARM && (info->num_x != 8 || info->num_u != 4))
        return fail(MMPC_ERR_PARSE, "exo_arm needs num_x = 8, num_u = 4");
    return MMPC_OK;
}

int validate_opts(const mmpc_opts* o) {
    if (o->max_iter < 0 || o->max_iter > 100000) return fail(MMPC_ERR_INVALID_ARG, "max_iter out of range");
    if (!(o->tol_grad > 0.0) || !(o->tol_defect > 0.0)) return fail(MMPC_ERR_INVALID_ARG, "tolerances must be > 0");
    if (o->kkt_solver < MMPC_KKT_AUTO || o->kkt_solver > MMPC_KKT_RICCATI_GROUP)
        return fail(MMPC_ERR_INVALID_ARG, "unknown kkt_solver");
    if (o->factor_fp32 != 0 && o->factor_fp32 != 1) return fail(MMPC_ERR_INVALID_ARG, "factor_fp32 must be 0 or 1");
    if (o->init_states != MMPC_INIT_AS_GIVEN && o->init_states != MMPC_INIT_HOLD_X0 && o->init_states != MMPC_INIT_ZERO)
        return fail(MMPC_ERR_INVALID_ARG, "unknown init_states");
    if (o->hessian < MMPC_HESSIAN_AUTO || o->hessian > MMPC_HESSIAN_EXACT)
        return fail(MMPC_ERR_INVALID_ARG, "unknown hessian");
    if (o->tail_cap < -1 || o->tail_cap >= 1000) return fail(MMPC_ERR_INVALID_ARG, "tail_cap must be -1 .. 999");
    if (o->tail_wave_max < -1 || o->tail_wave_max > 64)
        return fail(MMPC_ERR_INVALID_ARG, "tail_wave_max must be -1 .. 64");
    if (o->tail_rounds < -1 || o->tail_rounds == 0 || o->tail_rounds >= 1000)
        return fail(MMPC_ERR_INVALID_ARG, "tail_rounds must be -1 or 1 .. 999");
    return MMPC_OK;
}

int resolve_device(mmpc_handle* h, int* dev) {
    if (h->opts.device >= 0) {
        *dev = h->opts.device;
        return MMPC_OK;
    }
    int d = -1;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess) return fail(MMPC_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    *dev = d;
    return MMPC_OK;
}

// ---------------------------------------------------------------- auxiliary kernels
template <class Model>
__global__ __launch_bounds__(256) void linearize_kernel(int64_t B, const double* __restrict__ x,
                                                        const double* __restrict__ u, double* A, double* Bm,
                                                        double* xdot) {
    constexpr int NX = Model::NX, NU = Model::NU;
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= B) return;
    double xv[NX], uv[NU], xd[NX], fx[NX * NX], fu[NX * NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) xv[i] = x[b * NX + i];
#pragma unroll
    for (int i = 0; i < NU; ++i) uv[i] = u[b * NU + i];
    model_eval_jac<Model>(xv, uv, xd, fx, fu);
    // column-major, as CasADi DM -> std::vector (ModelControl.cpp:127-129)
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        if (xdot) xdot[b * NX + r] = xd[r];
#pragma unroll
        for (int c = 0; c < NX; ++c)
            if (A) A[b * NX * NX + c * NX + r] = fx[r * NX + c];
#pragma unroll
        for (int c = 0; c < NU; ++c)
            if (Bm) Bm[b * NX * NU + c * NX + r] = fu[r * NU + c];
    }
}

template <class Model>
__global__ __launch_bounds__(256) void nlp_eval_kernel(int64_t B, int N, double h, int is_linear,
                                                       const double* __restrict__ V, const double* __restrict__ u_prev,
                                                       const double* __restrict__ traj,
                                                       const double* __restrict__ weights, int64_t w_stride,
                                                       double* J, double* ginf) {
    constexpr int NX = Model::NX, NU = Model::NU, ND = NX + NU;
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int NV = NX * (N + 1) + NU * N;
    const double* v = V + b * NV;
    const double* w = weights + b * w_stride;
    const double* up = u_prev + b * NU;
    const double* tr = traj + b * (int64_t)N * NX;
    double lin[NX * NX + NX * NU + NX];
    if (is_linear) {  // F_lin at (x*, u*) = (x_0, u_prev), ModelGenerator.cpp:47-48
        double xd[NX], fx[NX * NX], fu[NX * NU];
        model_eval_jac<Model>(v, up, xd, fx, fu);
        for (int i = 0; i < NX * NX; ++i) lin[i] = fx[i];
        for (int i = 0; i < NX * NU; ++i) lin[NX * NX + i] = fu[i];
        for (int i = 0; i < NX; ++i) lin[NX * NX + NX * NU + i] = xd[i];
    }
    double Jv = 0.0, gm = 0.0;
    for (int k = 0; k < N; ++k) {
        const double* xk = v + k * ND;
        const double* uk = xk + NX;
        double xd[NX];
        if (!is_linear) {
            model_eval<Model>(xk, uk, xd);
        } else {
            for (int r = 0; r < NX; ++r) {
                double s = lin[NX * NX + NX * NU + r];
                for (int c = 0; c < NX; ++c) s += lin[r * NX + c] * (xk[c] - v[c]);
                for (int c = 0; c < NU; ++c) s += lin[NX * NX + r * NU + c] * (uk[c] - up[c]);
                xd[r] = s;
            }
        }
        for (int r = 0; r < NX; ++r) {
            const double F = xk[r] + h * xd[r];
            const double e = F - tr[k * NX + r];
            Jv += e * w[r] * e;
            const double gk = F - v[(k + 1) * ND + r];
            gm = (std::fabs(gk) > gm || gk != gk) ? std::fabs(gk) : gm;
        }
        for (int c = 0; c < NU; ++c) {
            const double um = (k == 0) ? up[c] : v[(k - 1) * ND + NX + c];
            const double du = uk[c] - um;
            Jv += du * w[NX + c] * du + uk[c] * w[NX + NU + c] * uk[c];
        }
    }
    if (J) J[b] = Jv;
    if (ginf) ginf[b] = gm;
}

// ---- committed controls (mmpc_solve_batch_pinned) ----
// With u_0..u_{m-1} fixed to the caller's values (the lbx = ubx = u the reference's ModelControl.cpp:165-171 meant to
// pose), x_1..x_m are fixed too and the rest is the horizon-(N - m) problem from x_m with u_prev' = u_{m-1} and the
// targets traj[m:].  The three kernels below reduce a batch to that problem in a staging area and put its solution
// back; the solver kernels run unchanged on the staging arrays with SolveParams::N = N - m.
//
// Prologue 1: one lane per instance, m serial Euler steps x_{k+1} = x_k + h f(x_k, u_k) with the model's value
// evaluation (as nlp_eval_kernel forms F).  Writes x_0..x_m and the pins into the head of V[b], and x_m / u_{m-1} as
// the tail problem's x0' / u_prev'.
template <class Model>
__global__ __launch_bounds__(256) void pin_rollout_kernel(int64_t B, int N, int m, double h,
                                                          const double* __restrict__ x0,
                                                          const double* __restrict__ u_pin, double* __restrict__ V,
                                                          double* __restrict__ x0s, double* __restrict__ ups) {
    constexpr int NX = Model::NX, NU = Model::NU, ND = NX + NU;
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    double* v = V + b * NV;
    const double* pin = u_pin + b * (int64_t)m * NU;
    double xk[NX], uk[NU] = {}, xd[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) xk[r] = x0[b * NX + r];
    for (int k = 0; k < m; ++k) {
#pragma unroll
        for (int c = 0; c < NU; ++c) uk[c] = pin[k * NU + c];
#pragma unroll
        for (int r = 0; r < NX; ++r) v[k * ND + r] = xk[r];
#pragma unroll
        for (int c = 0; c < NU; ++c) v[k * ND + NX + c] = uk[c];
        model_eval<Model>(xk, uk, xd);
#pragma unroll
        for (int r = 0; r < NX; ++r) xk[r] = xk[r] + h * xd[r];
    }
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        v[m * ND + r] = xk[r];
        x0s[b * NX + r] = xk[r];
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) ups[b * NU + c] = uk[c];   // m >= 1: the last pin
}

// Prologue 2: elementwise, consecutive lanes on consecutive doubles of the destination.  trajs [B][N - m][nx] =
// traj[b][m:], Vs [B][NV(N - m)] = V[b] from offset m (nx + nu) on (its first nx entries are the x_m of prologue 1:
// same stream, launched after it).  Vs == nullptr (MMPC_INIT_ZERO: the solver does not read V) skips the V part.
__global__ __launch_bounds__(256) void pin_gather_kernel(int64_t B, int N, int m, int nx, int nu,
                                                         const double* __restrict__ traj, const double* __restrict__ V,
                                                         double* __restrict__ trajs, double* __restrict__ Vs) {
    const int64_t Np = N - m;
    const int64_t nt = Np * nx, ntf = (int64_t)N * nx;
    const int64_t nvs = nx * (Np + 1) + nu * Np, nvf = (int64_t)nx * (N + 1) + (int64_t)nu * N;
    const int64_t row = nt + (Vs ? nvs : 0);
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= B * row) return;
    const int64_t b = t / row, i = t - b * row;
    if (i < nt) trajs[b * nt + i] = traj[b * ntf + (int64_t)m * nx + i];
    else Vs[b * nvs + (i - nt)] = V[b * nvf + (int64_t)m * (nx + nu) + (i - nt)];
}

// Epilogue: the tail solution back into V[b] from offset m (nx + nu) on, and u0_out[b] = the first pin -- the control
// in force now, V[b][nx : nx + nu] (u0_out may be nullptr or host-mapped memory).
__global__ __launch_bounds__(256) void pin_scatter_kernel(int64_t B, int N, int m, int nx, int nu,
                                                          const double* __restrict__ Vs,
                                                          const double* __restrict__ u_pin, double* __restrict__ V,
                                                          double* __restrict__ u0_out) {
    const int64_t Np = N - m;
    const int64_t nvs = nx * (Np + 1) + nu * Np, nvf = (int64_t)nx * (N + 1) + (int64_t)nu * N;
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= B * nvs) return;
    const int64_t b = t / nvs, i = t - b * nvs;
    V[b * nvf + (int64_t)m * (nx + nu) + i] = Vs[t];
    if (u0_out && i < nu) u0_out[b * nu + i] = u_pin[b * (int64_t)m * nu + i];
}

// nlp_grad_f / nlp_jac_g of the generated NLP (ModelGenerator.cpp:238, CasADi generate_dependencies): per
// instance J, dJ/dV [NV] (V layout) and the nonzero blocks of dg/dV, [dg_k/dx_k | dg_k/du_k] = [I + h f_x | h f_u]
// (row-major nx x (nx+nu) per stage; dg_k/dx_{k+1} = -I).  Linear mode: F_lin with A*, B* at (x_0, u_prev).
template <class Model>
__global__ __launch_bounds__(256) void nlp_derivs_kernel(int64_t B, int N, double h, int is_linear,
                                                         const double* __restrict__ V, const double* __restrict__ u_prev,
                                                         const double* __restrict__ traj,
                                                         const double* __restrict__ weights, int64_t w_stride,
                                                         double* J, double* grad, double* jac_blocks) {
    constexpr int NX = Model::NX, NU = Model::NU, ND = NX + NU;
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int NV = NX * (N + 1) + NU * N;
    const double* v = V + b * NV;
    const double* w = weights + b * w_stride;
    const double* up = u_prev + b * NU;
    const double* tr = traj + b * (int64_t)N * NX;
    double* gr = grad ? grad + b * NV : nullptr;
    double lin[NX * NX + NX * NU + NX];
    if (is_linear) {
        double xd[NX], fx[NX * NX], fu[NX * NU];
        model_eval_jac<Model>(v, up, xd, fx, fu);
        for (int i = 0; i < NX * NX; ++i) lin[i] = fx[i];
        for (int i = 0; i < NX * NU; ++i) lin[NX * NX + i] = fu[i];
        for (int i = 0; i < NX; ++i) lin[NX * NX + NX * NU + i] = xd[i];
    }
    double Jv = 0.0;
    if (gr)
        for (int r = 0; r < NX; ++r) gr[N * ND + r] = 0.0;  // x_N does not enter J
    for (int k = 0; k < N; ++k) {
        const double* xk = v + k * ND;
        const double* uk = xk + NX;
        double xd[NX], fx[NX * NX], fu[NX * NU];
        if (!is_linear) {
            model_eval_jac<Model>(xk, uk, xd, fx, fu);
        } else {
            for (int r = 0; r < NX; ++r) {
                double s = lin[NX * NX + NX * NU + r];
                for (int c = 0; c < NX; ++c) s += lin[r * NX + c] * (xk[c] - v[c]);
                for (int c = 0; c < NU; ++c) s += lin[NX * NX + r * NU + c] * (uk[c] - up[c]);
                xd[r] = s;
            }
            for (int i = 0; i < NX * NX; ++i) fx[i] = lin[i];
            for (int i = 0; i < NX * NU; ++i) fu[i] = lin[NX * NX + i];
        }
        double qe[NX];
        for (int r = 0; r < NX; ++r) {
            const double e = xk[r] + h * xd[r] - tr[k * NX + r];
            Jv += e * w[r] * e;
            qe[r] = 2.0 * w[r] * e;
        }
        if (jac_blocks) {
            double* jb = jac_blocks + (b * N + k) * (int64_t)(NX * ND);
            for (int r = 0; r < NX; ++r) {
                for (int c = 0; c < NX; ++c) jb[r * ND + c] = (r == c ? 1.0 : 0.0) + h * fx[r * NX + c];
                for (int c = 0; c < NU; ++c) jb[r * ND + NX + c] = h * fu[r * NU + c];
            }
        }
        for (int c = 0; c < NU; ++c) {
            const double um = (k == 0) ? up[c] : v[(k - 1) * ND + NX + c];
            const double du = uk[c] - um;
            Jv += du * w[NX + c] * du + uk[c] * w[NX + NU + c] * uk[c];
        }
        if (gr) {
            for (int c = 0; c < NX; ++c) {  // dJ/dx_k = 2 (I + h f_x)^T Q e_k
                double t = qe[c];
                for (int r = 0; r < NX; ++r) t += h * fx[r * NX + c] * qe[r];
                gr[k * ND + c] = t;
            }
            for (int c = 0; c < NU; ++c) {  // dJ/du_k = 2 h f_u^T Q e_k + Delta-u and Rm terms
                double t = 0.0;
                for (int r = 0; r < NX; ++r) t += h * fu[r * NU + c] * qe[r];
                const double um = (k == 0) ? up[c] : v[(k - 1) * ND + NX + c];
                t += 2.0 * w[NX + c] * (uk[c] - um) + 2.0 * w[NX + NU + c] * uk[c];
                if (k + 1 < N) t -= 2.0 * w[NX + c] * (v[(k + 1) * ND + NX + c] - uk[c]);
                gr[k * ND + NX + c] = t;
            }
        }
    }
    if (J) J[b] = Jv;
}

// nlp_hess_l of the generated NLP (ModelGenerator.cpp:238; CasADi's Hessian of the Lagrangian
// lam_f J + lam_g^T g): the nonzero stage blocks, one thread per (instance, stage).  Block k on (x_k, u_k) [K x K]:
//   lam_f [2 J_Fk^T Q J_Fk + blkdiag(0, 2R + 2Rm (+ 2R for k + 1 < N))] + h sum_r nu_r d^2 f_r/d(x_k,u_k)^2,
//   nu = 2 lam_f Q e_k + lam_g,k,  J_Fk = [I + h f_x | h f_u],  e_k = F(x_k,u_k) - r_k;
// the other nonzeros are constant (d^2/du_k du_{k-1} = -2 lam_f R) and x_N enters L linearly.
template <class Model>
__global__ __launch_bounds__(256) void nlp_hess_kernel(int64_t B, int N, double h, int is_linear,
                                                       const double* __restrict__ V, const double* __restrict__ u_prev,
                                                       const double* __restrict__ traj,
                                                       const double* __restrict__ weights, int64_t w_stride,
                                                       double lam_f, const double* __restrict__ lam_g, double* blocks) {
    constexpr int NX = Model::NX, NU = Model::NU, ND = NX + NU, NQ = Model::NQ, NA = NX - NQ;
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= B * N) return;
    const int64_t b = t / N;
    const int k = static_cast<int>(t - b * N);
    const int NV = NX * (N + 1) + NU * N;
    const double* v = V + b * NV;
    const double* w = weights + b * w_stride;
    const double* up = u_prev + b * NU;
    const double* xk = v + k * ND;
    const double* uk = xk + NX;
    double xd[NX], fx[NX * NX], fu[NX * NU];
    if (!is_linear) {
        model_eval_jac<Model>(xk, uk, xd, fx, fu);
    } else {   // F_lin: A*, B*, xdot* at (x_0, u_prev)
        double xs[NX], fxs[NX * NX], fus[NX * NU];
        model_eval_jac<Model>(v, up, xs, fxs, fus);
        for (int r = 0; r < NX; ++r) {
            double s = xs[r];
            for (int c = 0; c < NX; ++c) s += fxs[r * NX + c] * (xk[c] - v[c]);
            for (int c = 0; c < NU; ++c) s += fus[r * NU + c] * (uk[c] - up[c]);
            xd[r] = s;
        }
        for (int i = 0; i < NX * NX; ++i) fx[i] = fxs[i];
        for (int i = 0; i < NX * NU; ++i) fu[i] = fus[i];
    }
    double JF[NX][ND], nu[NX];
    for (int r = 0; r < NX; ++r) {
        for (int c = 0; c < NX; ++c) JF[r][c] = (r == c ? 1.0 : 0.0) + h * fx[r * NX + c];
        for (int c = 0; c < NU; ++c) JF[r][NX + c] = h * fu[r * NU + c];
        const double e = xk[r] + h * xd[r] - traj[(b * N + k) * NX + r];
        nu[r] = 2.0 * lam_f * w[r] * e + (lam_g ? lam_g[b * (int64_t)N * NX + k * NX + r] : 0.0);
    }
    double W[ND * ND];
    for (int i = 0; i < ND * ND; ++i) W[i] = 0.0;
    if constexpr (HasHess<Model>::value) {
        if (!is_linear) {
            double la[NA];
            for (int s2 = 0; s2 < NA; ++s2) la[s2] = h * nu[NQ + s2];
            Model::eval_hess(xk, uk, la, W);
        }
    }
    double* out = blocks + t * (int64_t)(ND * ND);
    for (int i = 0; i < ND; ++i)
        for (int j = i; j < ND; ++j) {   // upper triangle, mirrored: the block is symmetric bit for bit
            double s = W[i * ND + j];
            for (int r = 0; r < NX; ++r) s += 2.0 * lam_f * w[r] * JF[r][i] * JF[r][j];
            if (i == j && i >= NX) {
                const int c = i - NX;
                s += lam_f * (2.0 * w[NX + c] + 2.0 * w[NX + NU + c] + (k + 1 < N ? 2.0 * w[NX + c] : 0.0));
            }
            out[i * ND + j] = s;
            out[j * ND + i] = s;
        }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double unit_draw(uint64_t seed, int64_t index, int j) {
    const uint64_t v = splitmix64(seed ^ splitmix64((uint64_t)index * 16ull + (uint64_t)j));
    return (double)(v >> 11) * 0x1.0p-53;
}

// lo + span*u with an unfused product (bit-identical to the oracle's and make_golden.py's generator)
__device__ __forceinline__ double affine_draw(double lo, double span, double u) {
#pragma clang fp contract(off)
    const double p = span * u;
    return lo + p;
}

// SURVEY.md 8d instance generators (identical recipes in oracle/mmpc_oracle.c and tests/golden/).  bench.py generates
// every step's instances inside its clock, so they are built for throughput: a 256-thread block takes
// I = max(1, 256 / N) instances; its threads first form the instances' unit draws (each exactly once, into LDS; the
// x0 / u_prev draws go straight to memory), then one thread per (instance, stage) forms that stage's targets (sin /
// cos of the phase, stores contiguous across the block).  Round 4 ran one thread per instance (30-50 sin / cos in
// series, strided stores, 16 CUs busy at cfg#2: 12.3 us per batch); a first round-5 version redrew every instance's
// parameters in each stage's thread (5.2 us at cfg#2 but 165 us at cfg#3: the 64-bit multiplies of splitmix64).
// The phase argument is formed without FMA contraction, as the C oracle.
// Round 6: the block's target rows (I N nx doubles, contiguous in traj) are staged in LDS and written out with
// consecutive lanes on consecutive doubles: one thread per stage wrote its row with nx stores of 8 bytes at a 64-byte
// lane stride (8 cache-line segments per store instruction; 131 us per cfg#3 batch).  N <= 256 always fits (I N <= 256).
constexpr int kSynthThreads = 256;
constexpr int kSynthStaged = 2048;   // doubles of LDS for the staged rows

// cfg#2: q ~ U[-pi/4, pi/4], qdot ~ U[-1, 1], u_prev ~ U[-5, 5]; a ~ U[0.5, 1], f ~ U[0.25, 1] Hz, phase ~ U[0, 2 pi];
// r_k = [a sin(2 pi f t_k + phase), -a sin(.), 2 pi f a cos(.), -2 pi f a cos(.)], t_k = k h
__global__ __launch_bounds__(kSynthThreads) void synth_two_link_kernel(uint64_t seed, int64_t first, int64_t B, int N,
                                                                       double h, double* x0, double* u_prev,
                                                                       double* traj) {
    constexpr int ND = 9;   // draws per instance: x0 (4), u_prev (2), a, f, phase
    __shared__ double dr[kSynthThreads][3];
    const int I = N < kSynthThreads ? kSynthThreads / N : 1;
    const int64_t b0 = (int64_t)blockIdx.x * I;
    const double PI = 3.14159265358979323846;
    for (int t = threadIdx.x; t < I * ND; t += kSynthThreads) {
        const int i = t / ND, j = t - i * ND;
        const int64_t b = b0 + i;
        if (b >= B) continue;
        const double u = unit_draw(seed, first + b, j);
        if (j < 2) x0[b * 4 + j] = affine_draw(-PI / 4, PI / 2, u);
        else if (j < 4) x0[b * 4 + j] = affine_draw(-1.0, 2.0, u);
        else if (j < 6) u_prev[b * 2 + j - 4] = affine_draw(-5.0, 10.0, u);
        else if (j == 6) dr[i][0] = affine_draw(0.5, 0.5, u);
        else if (j == 7) dr[i][1] = affine_draw(0.25, 0.75, u);
        else dr[i][2] = affine_draw(0.0, 2.0 * PI, u);
    }
    __syncthreads();
    __shared__ double so[kSynthStaged];
    const bool staged = I * N * 4 <= kSynthStaged;
    for (int t = threadIdx.x; t < I * N; t += kSynthThreads) {
        const int i = t / N, k = t - i * N;
        const int64_t b = b0 + i;
        if (b >= B) continue;
        const double a = dr[i][0], f = dr[i][1], ph = dr[i][2];
        double arg, cs;
        {
#pragma clang fp contract(off)
            arg = 2.0 * PI * f * (k * h) + ph;
            cs = 2.0 * PI * f * a;
        }
        double sn, cn;
        sincos(arg, &sn, &cn);   // one argument reduction for both (the device library's sin and cos values)
        const double sv = a * sn, cv = cs * cn;
        double* r = staged ? so + t * 4 : traj + (b * N + k) * 4;
        r[0] = sv;
        r[1] = -sv;
        r[2] = cv;
        r[3] = -cv;
    }
    if (staged) {   // the block's rows are contiguous in traj: coalesced copy-out
        __syncthreads();
        const int64_t nb = B - b0 < I ? B - b0 : I;
        double* const dst = traj + b0 * N * 4;
        for (int t = threadIdx.x; t < nb * N * 4; t += kSynthThreads) dst[t] = so[t];
    }
}

// cfg#3: q, qd ~ U[-0.5, 0.5], tau_prev ~ U[-1, 1], per joint a ~ U[0.1, 0.4], f ~ U[0.25, 1] Hz, phase ~ U[0, 2 pi];
// r_k = [a sin(2 pi f t_k + phase); 2 pi f a cos(2 pi f t_k + phase)], t_k = k h
__device__ __forceinline__ double unit_draw_exo(uint64_t seed, int64_t index, int j) {
    const uint64_t v = splitmix64((seed + 0x3C6EF372FE94F82Aull) ^ splitmix64((uint64_t)index * 32ull + (uint64_t)j));
    return (double)(v >> 11) * 0x1.0p-53;
}
__global__ __launch_bounds__(kSynthThreads) void synth_exo_kernel(uint64_t seed, int64_t first, int64_t B, int N,
                                                                  double h, double* x0, double* u_prev, double* traj) {
    constexpr int ND = 24;   // draws per instance: x0 (8), u_prev (4), per joint a, f, phase (12)
    __shared__ double dr[kSynthThreads][12];
    const int I = N < kSynthThreads ? kSynthThreads / N : 1;
    const int64_t b0 = (int64_t)blockIdx.x * I;
    const double PI = 3.14159265358979323846;
    for (int t = threadIdx.x; t < I * ND; t += kSynthThreads) {
        const int i = t / ND, j = t - i * ND;
        const int64_t b = b0 + i;
        if (b >= B) continue;
        const double u = unit_draw_exo(seed, first + b, j);
        if (j < 8) x0[b * 8 + j] = affine_draw(-0.5, 1.0, u);
        else if (j < 12) u_prev[b * 4 + j - 8] = affine_draw(-1.0, 2.0, u);
        else if (j < 16) dr[i][j - 12] = affine_draw(0.1, 0.3, u);
        else if (j < 20) dr[i][j - 12] = affine_draw(0.25, 0.75, u);
        else dr[i][j - 12] = affine_draw(0.0, 2.0 * PI, u);
    }
    __syncthreads();
    __shared__ double so[kSynthStaged];
    const bool staged = I * N * 8 <= kSynthStaged;
    for (int t = threadIdx.x; t < I * N; t += kSynthThreads) {
        const int i = t / N, k = t - i * N;
        const int64_t b = b0 + i;
        if (b >= B) continue;
        double* r = staged ? so + t * 8 : traj + (b * N + k) * 8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double a = dr[i][j], f = dr[i][4 + j], ph = dr[i][8 + j];
            double arg, cs;
            {
#pragma clang fp contract(off)
                arg = 2.0 * PI * f * (k * h) + ph;
                cs = 2.0 * PI * f * a;
            }
            double sn, cn;
            sincos(arg, &sn, &cn);
            r[j] = a * sn;
            r[4 + j] = cs * cn;
        }
    }
    if (staged) {   // the block's rows are contiguous in traj: coalesced copy-out
        __syncthreads();
        const int64_t nb = B - b0 < I ? B - b0 : I;
        double* const dst = traj + b0 * N * 8;
        for (int t = threadIdx.x; t < nb * N * 8; t += kSynthThreads) dst[t] = so[t];
    }
}

inline unsigned grid1d(int64_t B, int threads) { return static_cast<unsigned>((B + threads - 1) / threads); }
// blocks of the instance generators: I = max(1, kSynthThreads / N) instances per block
inline unsigned synth_blocks(int64_t B, int N) {
    const int64_t I = N < kSynthThreads ? kSynthThreads / N : 1;
    return static_cast<unsigned>((B + I - 1) / I);
}

// Calls f((Model*)nullptr) for the model compiled into this library under model_id.
template <class F>
int with_model(int model_id, F&& f) {
#if MMPC_BUILTIN_MODELS
    if (model_id == MMPC_MODEL_TWO_LINK_ARM) return f(static_cast<TwoLinkArm*>(nullptr));
    if (model_id == MMPC_MODEL_EXO_ARM) return f(static_cast<ExoArm*>(nullptr));
#else
    if (model_id == MMPC_MODEL_USER) return f(static_cast<UserModel*>(nullptr));
#endif
    return fail(MMPC_ERR_UNSUPPORTED, "model not compiled into this library");
}
int model_nq(int model_id) {
    int nq = 0;
    with_model(model_id, [&](auto* m) {
        nq = std::remove_pointer_t<decltype(m)>::NQ;
        return MMPC_OK;
    });
    return nq;
}

// the model at another horizon: a pinned solve (mmpc_solve_batch_pinned) runs the handle's model with N - n_pin
// shooting nodes, and every host-side size below follows the horizon of the launch (SolveParams::N), not the handle's
mmpc_model_info with_horizon(const mmpc_model_info& mi, int N) {
    mmpc_model_info r = mi;
    r.num_shooting_nodes = N;
    r.num_v = mi.num_x * (N + 1) + mi.num_u * N;
    r.num_g = mi.num_x * N;
    return r;
}

// Sizes by key (kernel_variant.h): the kernels stride their LDS and workspace by their own template flags (sqp_group.h
// group_lds / group_ws_doubles, sqp_lane.h lane_ws_doubles), and these are the host's only calls of those
// functions, each flag taken from the key's member of the same meaning.
// per-instance doubles of the 16-lane kernel's workspace (the host never counts on the on-chip W record)
int group_ws_doubles(const mmpc_model_info& mi, const KernelVariant& v) {
    return mmpc::group_ws_doubles(mi.num_x, mi.num_u, mi.num_shooting_nodes, v.ub, v.xb, false, v.mehr);
}
int lane_ws_doubles(const mmpc_model_info& mi, int nq, const KernelVariant& v) {
    return mmpc::lane_ws_doubles(mi.num_x, mi.num_u, nq, mi.num_shooting_nodes, v.xb);
}
// LDS of one instance group of the 16-lane kernel, and of a full workgroup of kGroupsPerWave of them
size_t group_lds_instance_bytes(const mmpc_model_info& mi, int nq, const KernelVariant& v) {
    // the constant block of the model's kernels (sqp_group.h GroupLaneOps; generated models: none)
    const int kc = mi.model_id == MMPC_MODEL_TWO_LINK_ARM ? mmpc::GroupLaneOps<TwoLinkArm>::doubles
                   : mi.model_id == MMPC_MODEL_EXO_ARM    ? mmpc::GroupLaneOps<ExoArm>::doubles
                                                          : 0;
    // the head block of the gain record: the unbounded kernels of a model with a constant block
    const int kh = kc > 0 && !v.ub && !v.xb ? mmpc::group_head_doubles(mi.num_x, mi.num_u) : 0;
    return static_cast<size_t>(mmpc::group_lds(mi.num_x, mi.num_u, nq, mi.num_shooting_nodes, v.ub, mi.is_linear != 0,
                                               kc, kh).doubles) * sizeof(double);
}
size_t group_lds_bytes(const mmpc_model_info& mi, int nq, const KernelVariant& v) {
    return group_lds_instance_bytes(mi, nq, v) * kGroupsPerWave;
}
constexpr size_t kMaxGroupLds = 160 * 1024;  // gfx950: 160 KB of LDS per workgroup (attribute raised above 64 KB)

// Solver workspace of B instances, whichever kernel and variant runs them: the lane kernels' with the interior point's
// stage fields, or the largest of the 16-lane kernels' -- control bounds, or state bounds under Mehrotra's rule, counted
// whichever barrier rule the handle has now, so that mmpc_set_barrier_rule after a reservation never makes a solve
// grow it
size_t solver_workspace_bytes(const mmpc_model_info& mi, int nq, int64_t B) {
    const size_t lane = static_cast<size_t>(lane_ws_doubles(mi, nq, kVariantXb)) * 64u *
                        static_cast<size_t>((B + 63) / 64) * sizeof(double);
    const size_t group = static_cast<size_t>(std::max(group_ws_doubles(mi, kVariantUb),
                                                      group_ws_doubles(mi, kVariantXbMehrotra))) *
                         static_cast<size_t>(B) * sizeof(double);
    return (std::max(lane, group) + 255) / 256 * 256;
}

// opts.kkt_solver, or the AUTO choice before state bounds are considered
int resolve_kkt_solver_base(const mmpc_handle* h, int64_t B) {
    const mmpc_model_info& mi = h->info;
    if (h->opts.kkt_solver != MMPC_KKT_AUTO) return h->opts.kkt_solver;
    if (h->opts.factor_fp32) return MMPC_KKT_RICCATI;
    // measured on one MI355X (tools/solver_sweep.py): 2-link arm -- condensed for small batches
    // (B <= 2560 at N*nu <= 64), the 16-lane Riccati kernel up to B*N = 1e6, one lane per instance beyond;
    // exo -- the 16-lane kernel while at least two of its workgroups fit a CU's LDS and B <= 4096
    const int N = mi.num_shooting_nodes;
    // LDS of the layout launch_kernel will use: the interior-point fields with state bounds, else the bounded
    // solves' hold targets (the larger of the two control-bound variants)
    const size_t glds = group_lds_bytes(mi, h->nq, h->x_bounded ? kVariantXb : kVariantUb);
    if (mi.model_id == MMPC_MODEL_USER) {  // SX-generated dynamics: no condensed kernel (it is 2-link specific)
        if (glds <= kMaxGroupLds / 2 && B * static_cast<int64_t>(N) <= 1000000) return MMPC_KKT_RICCATI_GROUP;
        return MMPC_KKT_RICCATI;
    }
    if (mi.model_id == MMPC_MODEL_TWO_LINK_ARM) {
        // the condensed kernel is Gauss-Newton only: with the exact Hessian (AUTO) the 16-lane kernel takes the
        // small batches too (fewer SQP iterations outweigh its higher per-iteration cost)
        if (N * TwoLinkArm::NU <= 64 && B <= 2560 && (h->opts.hessian == MMPC_HESSIAN_GAUSS_NEWTON || mi.is_linear))
            return MMPC_KKT_CONDENSED;
        if (glds <= kMaxGroupLds && B * static_cast<int64_t>(N) <= 1000000) return MMPC_KKT_RICCATI_GROUP;
        return MMPC_KKT_RICCATI;
    }
    if (glds <= kMaxGroupLds / 2 && B <= 4096) return MMPC_KKT_RICCATI_GROUP;
    return MMPC_KKT_RICCATI;
}
// the KKT solver a solve of B instances runs
int resolve_kkt_solver(const mmpc_handle* h, int64_t B) {
    const int s = resolve_kkt_solver_base(h, B);
    // state bounds (interior-point variant): the Riccati solvers only; the group kernel when its LDS layout fits
    if (h->x_bounded && h->opts.kkt_solver == MMPC_KKT_AUTO && s == MMPC_KKT_CONDENSED)
        return group_lds_bytes(h->info, h->nq, kVariantXb) <= kMaxGroupLds ? MMPC_KKT_RICCATI_GROUP : MMPC_KKT_RICCATI;
    return s;
}

// Exact-Hessian support of a model / solve (mmpc_opts.hessian): second derivatives, the lane-distributed path
// of the group kernel (nx + nu < 16, no bounds), nonlinear dynamics.  AUTO also needs the model's default
// (kExactDefault: the exo keeps Gauss-Newton -- its small-residual fits converge in 3-5 Gauss-Newton
// iterations and the exact Hessian did not cut them in the prototype sweep).
template <class M>
constexpr bool exact_capable() {
    return HasHess<M>::value && (M::NX + M::NU < kGroupLanes);
}
template <class M, class = void>
struct ExactDefault {
    static constexpr bool value = true;
};
template <class M>
struct ExactDefault<M, std::enable_if_t<!M::kExactDefault || M::kExactDefault>> {
    static constexpr bool value = M::kExactDefault;
};
// MMPC_HESSIAN_GAUSS_NEWTON / _EXACT for a solve under solver with/without control bounds; <0 = error
int resolve_hessian(const mmpc_handle* h, int solver, bool u_bounded) {
    const int want = h->opts.hessian;
    if (want == MMPC_HESSIAN_GAUSS_NEWTON) return MMPC_HESSIAN_GAUSS_NEWTON;
    bool group_capable = false, lane_capable = false, dflt = false;
    with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        group_capable = exact_capable<M>();
        lane_capable = HasHess<M>::value;
        dflt = ExactDefault<M>::value;
        return MMPC_OK;
    });
    // control bounds (the projected SQP): EXACT fixes the held controls in the exact QP as in the Gauss-Newton one
    // (group kernel; lane kernel since round 5); AUTO keeps Gauss-Newton there -- measured faster at cfg#2 with +-2 Nm
    // (0.77 vs 0.91 ms: the exact solves take fewer iterations, but every re-solve after a hold repeats the costlier
    // exact Riccati sweep).  The lane kernel (round 4) takes EXACT on request; AUTO there stays
    // Gauss-Newton (its backward sweep evaluates the model's Hessian per stage).
    // state bounds (round 6): EXACT on request (IPOPT's exact Hessian under the barrier, ModelGenerator.cpp:232,238);
    // AUTO keeps Gauss-Newton for state-bounded solves like for control-bounded ones
    const bool common = !h->info.is_linear && !h->opts.factor_fp32;
    const bool group_ok = common && group_capable && solver == MMPC_KKT_RICCATI_GROUP;
    const bool lane_ok = common && lane_capable && solver == MMPC_KKT_RICCATI;
    if (want == MMPC_HESSIAN_EXACT) {
        if (!group_ok && !lane_ok)
            return fail(MMPC_ERR_UNSUPPORTED, "exact Hessian: needs a model with second derivatives, a Riccati "
                                              "solver (RICCATI_GROUP or RICCATI, fp64 factor) and a nonlinear solve");
        return MMPC_HESSIAN_EXACT;
    }
    return group_ok && dflt && !u_bounded && !h->x_bounded ? MMPC_HESSIAN_EXACT : MMPC_HESSIAN_GAUSS_NEWTON;
}

// the 16-lane kernels this unit instantiates for model M: every canonical fp64 variant, the exact Hessian for
// exact_capable models, Mehrotra's rule on the lane-distributed path (nx + nu < 16).  None for the built-in 2-link arm:
// its kernels live in the units of group_launch.h.
template <class M>
constexpr bool has_group_kernel(const KernelVariant& v) {
    return !std::is_same<M, TwoLinkArm>::value && canonical(v) && !v.fp32 && (!v.exact || exact_capable<M>()) &&
           (!v.mehr || M::NX + M::NU < kGroupLanes);
}
// launches the 16-lane kernel of model M for the key v; `what` names the launch in an error text
template <class M>
int launch_group_of(const KernelVariant& v, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                    const SolveParams& p, const GroupWork& gwk, const char* what) {
    if (v.mehr && M::NX + M::NU >= kGroupLanes)
        return fail(MMPC_ERR_UNSUPPORTED, "barrier rule MEHROTRA: the 16-lane solver runs it for models with "
                                          "nx + nu < 16 only");
    hipError_t e;
    if constexpr (std::is_same<M, TwoLinkArm>::value) {
        e = (v.ub || v.xb) ? launch_group_two_link_bounded(v, grid, block, lds, stream, p, gwk)
                           : launch_group_two_link(v, grid, block, lds, stream, p, gwk);
    } else {
        e = with_variant(v, [&](auto sv) {
            if constexpr (has_group_kernel<M>(decltype(sv)::value))
                return launch_group_kernel<M>(sv, grid, block, lds, stream, p, gwk);
            else
                return hipErrorInvalidValue;   // a key with no kernel (resolve_hessian never asks for one)
        });
    }
    return e == hipSuccess ? MMPC_OK : fail(MMPC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Riccati workspace (sqp_lane.h / sqp_group.h layouts), grown on demand.  Growth is synchronous:
// hipFree waits for the kernels still using the old buffer.
int ensure_workspace_bytes(mmpc_handle* h, size_t bytes, double** out) {
    int dev = -1;
    MMPC_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(h->ws_mu);
    if (h->ws && h->ws_dev != dev) return fail(MMPC_ERR_INVALID_ARG, "handle used on two devices");
    if (bytes > h->ws_bytes) {
        if (h->ws) MMPC_HIP(hipFree(h->ws));
        h->ws = nullptr;
        h->ws_bytes = 0;
        MMPC_HIP(hipMalloc(reinterpret_cast<void**>(&h->ws), bytes));
        h->ws_bytes = bytes;
        h->ws_dev = dev;
    }
    *out = h->ws;
    return MMPC_OK;
}
// iteration-tail hand-over list after the solver workspace: [count | pad][idx: slots x i32][it: slots x i32][mu][mub]
// (a state-bounded solve's resume workspace follows it: its duals stay in the lane launch's workspace)
constexpr int kTailMaxSlots = 65536;
constexpr size_t kTailBytes = 256 + static_cast<size_t>(kTailMaxSlots) * 24;

// Iteration-tail hand-over of a lane-kernel solve: the lane kernel's wave runs until its slowest lane
// converges (cfg#3: 1 % of the instances need a 5th iteration, and the waves holding them set the kernel time), so
// instances still unconverged at the stop test of iteration `cap` continue in a 16-lane resume launch, whose
// per-iteration latency is ~5x lower (exo N = 24, B = 256: 0.30 vs 1.68 ms). Unbounded nonlinear solves of models
// the 16-lane kernel runs (nx + nu < 16), without the diagnostic trace; a solve with the fp32 Riccati factor continues
// its tail with the fp64 factor (precision escalation: same stop test, same iterate). cap: 4 (Gauss-Newton and exact
// Hessian; 3 hands over too many: cfg#3 12.8 ms), MMPC_TAIL_CAP overrides (0 = off). slots: four rounds of resume
// workgroups (groups per workgroup gpw with <= 64 KB of LDS, up to 4 one-wave workgroups per CU per round),
// MMPC_TAIL_ROUNDS overrides.
// Bounded solves hand over by the wave rule alone (their counts spread: no common cap). State bounds: the duals are
// read from the lane launch's workspace by the resume launch, whose own workspace then lies after the hand-over list
// (xb_ws_bytes). Control bounds: the resume launch runs the lane kernel's active-set rule (no_release) from the
// handed-over hold epsilon (tail_mub).
struct TailPlan {
    int cap = 0, wave_max = 0, slots = 0, gpw = 1;
    size_t lds = 0, xb_ws_bytes = 0;
};
// mi: the model at the horizon of the launch; v: the lane launch's key; cu <= 0 (no device queried, or a solve that must
// stay in the lane kernel: the diagnostic trace): no hand-over
TailPlan tail_plan(const mmpc_handle* h, const mmpc_model_info& mi, int64_t B, const KernelVariant& v, int cu) {
    TailPlan t;
    if (mi.is_linear || cu <= 0) return t;
    if (mi.num_x + mi.num_u >= kGroupLanes) return t;
    constexpr int kNoCap = 1 << 20;
    // bounded solves (state: interior point; control: projected SQP with its QP re-solves) hand over by the wave rule
    // alone: their counts spread (exo |u| <= 0.5: 4.3 mean, 12 max), and a cap either hands over too many or none
    const bool spread = v.xb || v.ub;
    const int max_iter = h->opts.max_iter;
    // opts.tail_* (ABI 6), the MMPC_TAIL_* environment overriding them (A/B and tests); -1: the default policy
    const int cap_o = h->tail_cap_env >= 0 ? h->tail_cap_env : h->opts.tail_cap;
    const int wave_o = h->tail_wave_env >= 0 ? h->tail_wave_env : h->opts.tail_wave_max;
    const int rounds_o = h->tail_rounds_env > 0 ? h->tail_rounds_env : h->opts.tail_rounds;
    const int cap = cap_o >= 0 ? cap_o : (spread ? kNoCap : 4);
    if (cap <= 0 || (cap >= max_iter && !spread)) return t;
    // wave rule threshold: 8 lanes (unbounded: only the thin tails of loose tolerances use it), 4 for bounded solves,
    // whose handed-over instances need several more iterations (exo at cfg#3 size, ms without / with 4: |qdot| <= 1.5
    // 65.3 / 60.5 (1 / 2 / 3 / 6 lanes: 62.2 / 61.0 / 61.0 / 67.6, profiles/r05/xbwave); |u| <= 0.5 36.9 / 30.1, |u| <= 2
    // 22.7 / 22.2 (8 lanes: 38.4 / 21.0; caps 4-8 beside it, profiles/r05/ubsweep))
    const int wave_max = wave_o >= 0 ? wave_o : (spread ? 4 : 8);
    if (spread && cap >= max_iter && wave_max <= 0) return t;
    const size_t inst = group_lds_instance_bytes(mi, h->nq, v);
    if (inst > 64 * 1024) return t;
    const int gpw = static_cast<int>(std::max<size_t>(1, std::min<size_t>(kGroupsPerWave, (64 * 1024) / inst)));
    const int per_cu = static_cast<int>(std::min<size_t>(4, (160 * 1024) / (gpw * inst)));
    t.cap = cap;
    t.wave_max = wave_max;
    t.gpw = gpw;
    t.lds = gpw * inst;
    // up to four rounds of resume workgroups (slots nobody claimed exit at once, so spare slots cost nothing)
    const int rounds = rounds_o > 0 ? rounds_o : 4;
    t.slots = static_cast<int>(std::min<int64_t>({B, kTailMaxSlots, (int64_t)rounds * per_cu * cu * gpw}));
    if (v.xb) t.xb_ws_bytes = static_cast<size_t>(group_ws_doubles(mi, v)) * static_cast<size_t>(t.slots) * sizeof(double);
    return t;
}
// the device's compute units (the resume launch's slots scale with them), queried once per handle
int query_cu_count(mmpc_handle* h) {
    if (h->cu_count == 0) {
        int dev = 0, n = 0;
        MMPC_HIP(hipGetDevice(&dev));
        MMPC_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        h->cu_count = n;
    }
    return MMPC_OK;
}

// The handle's workspace, byte offsets:
//   [solver workspace | hand-over list | resume workspace]  (one launch, horizon N)  ...  | staging
// The first three are what one launch at horizon N under the key v uses; `end` is what that launch needs allocated.
// A pinned solve (mmpc_solve_batch_pinned) runs the solver at horizon N - m, where those regions end at an offset that
// depends on m (the resume slots grow as the stage data shrink), so its staging area -- x0' [B][nx], u_prev' [B][nu],
// traj' [B][N - m][nx], V' [B][NV(N - m)], sized for m = 1, the worst case -- lies after the largest end over every
// horizon 1..N (reserved_layout, which alone fills the second row; what mmpc_reserve_workspace reserves is `total`).
struct WorkspaceLayout {
    TailPlan tail;
    size_t solver = 0, tail_list = 0, resume = 0, end = 0;
    size_t max_end = 0, staging = 0, total = 0;
};
WorkspaceLayout workspace_layout(const mmpc_handle* h, const mmpc_model_info& mi, int64_t B, const KernelVariant& v,
                                 int cu) {
    WorkspaceLayout L;
    L.tail = tail_plan(h, mi, B, v, cu);
    L.tail_list = L.solver + solver_workspace_bytes(mi, h->nq, B);
    L.resume = L.tail_list + kTailBytes;
    L.end = L.resume + L.tail.xb_ws_bytes;
    return L;
}
// every horizon under the key with the largest end (state bounds: the only one with a resume workspace), reserved
// whether or not the handle has state bounds or pins now: neither mmpc_set_state_bounds nor a pinned solve may make a
// later solve grow the workspace (a hipFree / hipMalloc inside a stream-ordered solve, or under a captured hipGraph
// that still points at the old buffer)
WorkspaceLayout reserved_layout(const mmpc_handle* h, int64_t B, int cu) {
    const mmpc_model_info& mi = h->info;
    WorkspaceLayout L;   // ends as the handle's own horizon's
    size_t max_end = 0;
    for (int n = 1; n <= mi.num_shooting_nodes; ++n) {
        L = workspace_layout(h, with_horizon(mi, n), B, kVariantXb, cu);
        max_end = std::max(max_end, L.end);
    }
    L.max_end = max_end;
    const size_t nx = mi.num_x, nu = mi.num_u, N1 = mi.num_shooting_nodes > 1 ? mi.num_shooting_nodes - 1 : 0;
    L.staging = (L.max_end + 255) / 256 * 256;
    L.total = L.staging + static_cast<size_t>(B) * (nx + nu + N1 * nx + nx * (N1 + 1) + nu * N1) * sizeof(double);
    return L;
}

// u_lb / u_ub rows of the *_bounds entry points: 0 = one shared [nu] row, >= nu = a row per instance.
int check_bounds_stride(const mmpc_model_info& mi, int64_t b_stride) {
    if (b_stride != 0 && b_stride < mi.num_u)
        return fail(MMPC_ERR_INVALID_ARG, "bounds_stride must be 0 (shared) or >= nu (" + std::to_string(mi.num_u) +
                                              "), got " + std::to_string(b_stride));
    if (b_stride > 0x7fffffffLL)   // the kernels take it as 32 bits (SolveParams::b_stride)
        return fail(MMPC_ERR_UNSUPPORTED, "bounds_stride above 2^31 - 1 is not supported");
    return MMPC_OK;
}
// u_pin / n_pin of the *_pinned entry points
int check_pins(const mmpc_model_info& mi, const double* u_pin, int32_t n_pin) {
    const int N = mi.num_shooting_nodes;
    if (n_pin < 0 || n_pin > N - 1)
        return fail(MMPC_ERR_INVALID_ARG, "n_pin must be 0 .. N - 1 (" + std::to_string(N - 1) + "), got " +
                                              std::to_string(n_pin));
    if (n_pin > 0 && !u_pin)
        return fail(MMPC_ERR_INVALID_ARG, "u_pin is NULL with n_pin = " + std::to_string(n_pin));
    if (n_pin > 0 && mi.is_linear)   // the reference linearises at the measured (x_0, u_prev), the reduction would at x_m
        return fail(MMPC_ERR_UNSUPPORTED, "n_pin > 0 is not available in linear mode: the model is linearised at the "
                                          "measured (x_0, u_prev), the reduced problem would linearise at x_m");
    return MMPC_OK;
}

// One solve as the C-ABI describes it, in the order of the entry points' parameters (device or host pointers, as the
// entry point takes them).
struct SolveArgs {
    int64_t B = 0;
    const double *x0 = nullptr, *u_prev = nullptr, *traj = nullptr, *weights = nullptr;
    int64_t weights_stride = 0;
    const double *u_lb = nullptr, *u_ub = nullptr;
    int64_t bounds_stride = 0;
    const double* u_pin = nullptr;
    int32_t n_pin = 0;
    double* V = nullptr;
    int32_t *status = nullptr, *iters = nullptr;
    double *kkt = nullptr, *u0_out = nullptr;
    hipStream_t stream = nullptr;
    double* trace = nullptr;
};
// The one check of a solve's arguments.  Pure arithmetic on the arguments and the model (info: null for a null handle):
// every solve entry point calls it first, before any device call, copy or send, and returns at once when B == 0.
int check_solve_args(const mmpc_model_info* info, const SolveArgs& a, const char* null_handle = "null handle") {
    if (!info) return fail(MMPC_ERR_INVALID_ARG, null_handle);
    if (int rc = check_pins(*info, a.u_pin, a.n_pin)) return rc;
    if (a.B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    if (int rc = check_bounds_stride(*info, a.bounds_stride)) return rc;
    if (a.B == 0) return MMPC_OK;
    if (!a.x0 || !a.u_prev || !a.traj || !a.weights || !a.V) return fail(MMPC_ERR_INVALID_ARG, "null input pointer");
    // rows of weights_stride are read (and, by the host and RCCL entries, copied and sent) for every instance
    if (a.weights_stride != 0 && a.weights_stride < info->num_x + 2 * info->num_u)
        return fail(MMPC_ERR_INVALID_ARG, "weights_stride must be 0 or >= nx+2nu");
    if (a.B > 0x7fffffffLL) return fail(MMPC_ERR_INVALID_ARG, "B exceeds the grid limit (2^31-1)");
    return MMPC_OK;
}

int launch_kernel(mmpc_handle* h, int solver, const SolveParams& p, int barrier_rule, hipStream_t stream);

// a solve whose arguments check_solve_args has passed, B > 0, device pointers, on the current device
int launch_solve(mmpc_handle* h, const SolveArgs& a) {
    const mmpc_model_info& mi = h->info;
    const int64_t B = a.B;
    SolveParams p{};
    p.B = B;
    p.N = mi.num_shooting_nodes;
    p.max_iter = h->opts.max_iter;
    p.h = mi.step_size;
    p.tol_grad = h->opts.tol_grad;
    p.tol_defect = h->opts.tol_defect;
    p.is_linear = mi.is_linear;
    p.x0 = a.x0;
    p.u_prev = a.u_prev;
    p.traj = a.traj;
    p.weights = a.weights;
    p.w_stride = a.weights_stride;
    // any bound pointer selects a bounded kernel (launch_kernel); host entry points pass NULL for bounds that are all
    // infinite
    p.u_lb = a.u_lb;
    p.u_ub = a.u_ub;
    p.b_stride = static_cast<int32_t>(a.bounds_stride);
    p.V = a.V;
    p.status = a.status;
    p.iters = a.iters;
    p.kkt = a.kkt;
    p.trace = a.trace;
    p.u0_out = a.u0_out;
    p.init_hold = h->opts.init_states == MMPC_INIT_HOLD_X0;
    p.init_zero = h->opts.init_states == MMPC_INIT_ZERO;
    p.gpw = kGroupsPerWave;
    int barrier_rule;
    {  // state bounds: the interior-point variant (sqp_wave.h "state bounds"), by value in the launch arguments
        std::lock_guard<std::mutex> lk(h->xb_mu);
        barrier_rule = h->barrier_rule;
        p.x_bounded = h->x_bounded;
        for (int i = 0; i < 16; ++i) {
            p.x_lb[i] = i < mi.num_x ? h->x_lb[i] : -INFINITY;
            p.x_ub[i] = i < mi.num_x ? h->x_ub[i] : INFINITY;
        }
    }
    const int solver = resolve_kkt_solver(h, B);   // for the handle's own N, pinned or not
    if (a.n_pin == 0) return launch_kernel(h, solver, p, barrier_rule, a.stream);
    // committed controls: prologue (rollout of the pins, gather of the tail problem), the solve of the staged
    // horizon-(N - m) problem, epilogue (its solution back into V, u0_out = the first pin)
    if (int rc = query_cu_count(h)) return rc;
    const int m = a.n_pin, N = mi.num_shooting_nodes, Np = N - m, nx = mi.num_x, nu = mi.num_u;
    const WorkspaceLayout L = reserved_layout(h, B, h->cu_count);
    double* ws = nullptr;
    if (int rc = ensure_workspace_bytes(h, L.total, &ws)) return rc;
    const int64_t nvs = static_cast<int64_t>(nx) * (Np + 1) + static_cast<int64_t>(nu) * Np;
    double* const x0s = ws + L.staging / sizeof(double);
    double* const ups = x0s + B * nx;
    double* const trajs = ups + B * nu;
    double* const Vs = trajs + B * Np * nx;
    const int64_t n_gather = B * (static_cast<int64_t>(Np) * nx + (p.init_zero ? 0 : nvs)), n_scatter = B * nvs;
    if (std::max(n_gather, n_scatter) > 0x7fffffffLL * 256) return fail(MMPC_ERR_INVALID_ARG, "B*N too large");
    int rc = with_model(mi.model_id, [&](auto* mp) {
        using M = std::remove_pointer_t<decltype(mp)>;
        pin_rollout_kernel<M><<<grid1d(B, 256), 256, 0, a.stream>>>(B, N, m, mi.step_size, a.x0, a.u_pin, a.V, x0s, ups);
        return static_cast<int>(MMPC_OK);
    });
    if (rc) return rc;
    pin_gather_kernel<<<grid1d(n_gather, 256), 256, 0, a.stream>>>(B, N, m, nx, nu, a.traj, a.V, trajs,
                                                                    p.init_zero ? nullptr : Vs);
    MMPC_HIP(hipGetLastError());
    p.N = Np;
    p.x0 = x0s;
    p.u_prev = ups;
    p.traj = trajs;
    p.V = Vs;
    p.u0_out = nullptr;
    if ((rc = launch_kernel(h, solver, p, barrier_rule, a.stream))) return rc;
    pin_scatter_kernel<<<grid1d(n_scatter, 256), 256, 0, a.stream>>>(B, N, m, nx, nu, Vs, a.u_pin, a.V, a.u0_out);
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
}

// The three launches of launch_kernel.  Every size follows the horizon of the launch, p.N: the handle's, or N - n_pin of a
// pinned solve (the kernels lay their LDS and workspace out from p.N, and host and kernel must agree on one horizon).
int launch_condensed(mmpc_handle* h, const SolveParams& p, const KernelVariant& v, hipStream_t stream) {
    if (v.xb) return fail(MMPC_ERR_UNSUPPORTED, "state bounds need a Riccati solver (MMPC_KKT_RICCATI[_GROUP])");
    if (v.fp32) return fail(MMPC_ERR_UNSUPPORTED, "factor_fp32 is a Riccati-solver option");
#if MMPC_BUILTIN_MODELS
    // host-side shape checks: the kernel holds one condensed-Hessian row per lane
    // (supported or not by the handle's own N: a pinned solve runs the size class of its shorter horizon)
    if (h->info.model_id != MMPC_MODEL_TWO_LINK_ARM || h->info.num_shooting_nodes * TwoLinkArm::NU > 64)
        return fail(MMPC_ERR_UNSUPPORTED, "condensed solver needs the 2-link arm and N*nu <= 64");
    const int N = p.N;
    dim3 grid(static_cast<unsigned>(p.B)), block(64);
    if (v.ub) {
        if (N <= 16) sqp_wave_kernel<TwoLinkArm, 16, true><<<grid, block, 0, stream>>>(p);
        else if (N <= 30) sqp_wave_kernel<TwoLinkArm, 30, true><<<grid, block, 0, stream>>>(p);
        else sqp_wave_kernel<TwoLinkArm, 32, true><<<grid, block, 0, stream>>>(p);
    } else {
        if (N <= 16) sqp_wave_kernel<TwoLinkArm, 16><<<grid, block, 0, stream>>>(p);
        else if (N <= 30) sqp_wave_kernel<TwoLinkArm, 30><<<grid, block, 0, stream>>>(p);
        else sqp_wave_kernel<TwoLinkArm, 32><<<grid, block, 0, stream>>>(p);
    }
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
#else
    return fail(MMPC_ERR_UNSUPPORTED, "condensed solver needs the built-in 2-link arm");
#endif
}

int launch_group(mmpc_handle* h, const SolveParams& p, const KernelVariant& v, hipStream_t stream) {
    const mmpc_model_info mi = with_horizon(h->info, p.N);
    if (v.fp32) return fail(MMPC_ERR_UNSUPPORTED, "factor_fp32 needs the lane Riccati solver");
    const size_t lds = group_lds_bytes(mi, h->nq, v);
    if (lds > kMaxGroupLds) return fail(MMPC_ERR_UNSUPPORTED, "group Riccati solver: stage data exceeds 160 KB LDS");
    const WorkspaceLayout L = workspace_layout(h, mi, p.B, v, 0);   // cu = 0: nothing is handed over
    double* ws = nullptr;
    if (int rc = ensure_workspace_bytes(h, L.end, &ws)) return rc;
    const GroupWork gwk{ws + L.solver / sizeof(double)};
    const dim3 grid(grid1d(p.B, kGroupsPerWave)), block(64);
    return with_model(mi.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        return launch_group_of<M>(v, grid, block, lds, stream, p, gwk, "group kernel launch");
    });
}

// the lane launch, then (TailPlan) the 16-lane resume launch over the instances it handed over
int launch_lane(mmpc_handle* h, const SolveParams& p, const KernelVariant& v, hipStream_t stream) {
    const mmpc_model_info mi = with_horizon(h->info, p.N);
    if (int rc = query_cu_count(h)) return rc;
    // the diagnostic trace keeps every instance in the lane kernel
    const WorkspaceLayout L = workspace_layout(h, mi, p.B, v, p.trace ? 0 : h->cu_count);
    const TailPlan& tp = L.tail;
    double* ws = nullptr;
    if (int rc = ensure_workspace_bytes(h, L.end, &ws)) return rc;
    char* const base = reinterpret_cast<char*>(ws);
    const LaneWork lw{reinterpret_cast<double*>(base + L.solver)};
    SolveParams pl = p;
    if (tp.cap > 0) {   // the lane kernel hands instances still unconverged at iteration cap to a 16-lane launch
        pl.tail_cap = tp.cap;
        pl.tail_wave_max = tp.wave_max;
        pl.tail_slots = tp.slots;
        pl.tail_count = reinterpret_cast<int32_t*>(base + L.tail_list);
        pl.tail_idx = reinterpret_cast<int32_t*>(base + L.tail_list + 256);
        pl.tail_it = pl.tail_idx + kTailMaxSlots;
        pl.tail_mu = reinterpret_cast<double*>(pl.tail_it + kTailMaxSlots);
        pl.tail_mub = pl.tail_mu + kTailMaxSlots;
        MMPC_HIP(hipMemsetAsync(pl.tail_count, 0, sizeof(int32_t), stream));
    }
    // lane kernels: their own translation unit (lane_kernels.hip, lane_launch.h)
    const int lrc = launch_lane_kernels(mi.model_id, v, dim3(grid1d(p.B, 64)), dim3(64), stream, pl, lw);
    if (lrc == -1) return fail(MMPC_ERR_UNSUPPORTED, "model not compiled into this library");
    if (lrc != 0) return fail(MMPC_ERR_UNSUPPORTED, "lane Riccati solver: no kernel of this model for the solve's variant");
    MMPC_HIP(hipGetLastError());
    if (tp.cap <= 0) return MMPC_OK;
    // resume launch over the hand-over list (slots the lane kernel did not claim exit at once), with the fp64 factor
    SolveParams pr = pl;
    pr.tail_cap = 0;
    pr.gpw = tp.gpw;
    pr.init_hold = pr.init_zero = 0;   // the handed-over iterate is in V
    pr.no_release = 1;                 // control bounds: the lane kernel's active-set rule
    KernelVariant rv = v;
    rv.fp32 = false;
    GroupWork gwk{lw.ws};
    if (v.xb) {   // duals from the lane workspace; the resume workspace after the hand-over list
        pr.tail_lws = lw.ws;
        pr.tail_lws_block = static_cast<int64_t>(lane_ws_doubles(mi, h->nq, v)) * 64;
        pr.tail_lws_ss = lane_stage_stride(mi.num_x, mi.num_u, v.xb);
        pr.tail_lws_zl = lane_zl_offset(mi.num_x, mi.num_u);
        gwk.ws = reinterpret_cast<double*>(base + L.resume);
    }
    const dim3 rgrid(static_cast<unsigned>((tp.slots + tp.gpw - 1) / tp.gpw)), rblock(64);
    return with_model(mi.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        return launch_group_of<M>(rv, rgrid, rblock, tp.lds, stream, pr, gwk, "resume launch");
    });
}

// The key of a solve (kernel_variant.h), built here and nowhere else, in canonical form: the interior point takes the
// control bounds of a state-bounded solve, per-instance rows matter to bounded kernels only, the barrier rule to the
// interior point only, and the fp32 factor runs Gauss-Newton.  <0: resolve_hessian's error.
int kernel_variant(const mmpc_handle* h, int solver, const SolveParams& p, int barrier_rule, KernelVariant* v) {
    const bool u_bounded = p.u_lb || p.u_ub;
    const int hess = resolve_hessian(h, solver, u_bounded);   // EXACT requested on an unsupported solver: error
    if (hess < 0) return hess;
    v->xb = p.x_bounded != 0;
    v->ub = u_bounded && !v->xb;
    v->fp32 = h->opts.factor_fp32 != 0;
    v->exact = hess == MMPC_HESSIAN_EXACT && !v->fp32;
    v->instb = p.b_stride != 0 && (v->ub || v->xb);
    v->mehr = v->xb && barrier_rule == MMPC_BARRIER_MEHROTRA;
    return MMPC_OK;
}

// one solve of p.B instances with solver (not AUTO): the condensed launch, the 16-lane launch, or the lane launch with
// its resume launch
int launch_kernel(mmpc_handle* h, int solver, const SolveParams& p, int barrier_rule, hipStream_t stream) {
    KernelVariant v;
    if (int rc = kernel_variant(h, solver, p, barrier_rule, &v)) return rc;
    // the barrier rule matters to the interior point alone (finite state bounds); Mehrotra's rule is built into the
    // 16-lane kernel for nonlinear solves -- anything else is refused, never run under the other rule
    if (v.mehr && h->info.is_linear)
        return fail(MMPC_ERR_UNSUPPORTED, "barrier rule MEHROTRA: not available in linear mode "
                                          "(use MMPC_BARRIER_MONOTONE)");
    if (v.mehr && solver != MMPC_KKT_RICCATI_GROUP)
        return fail(MMPC_ERR_UNSUPPORTED,
                    std::string("barrier rule MEHROTRA: needs the 16-lane solver (MMPC_KKT_RICCATI_GROUP), this solve ") +
                        (h->opts.kkt_solver == MMPC_KKT_AUTO ? "resolves to" : "asks for") +
                        (solver == MMPC_KKT_RICCATI ? " the lane solver (MMPC_KKT_RICCATI)" : " the condensed solver"));
    switch (solver) {
        case MMPC_KKT_RICCATI_GROUP: return launch_group(h, p, v, stream);
        case MMPC_KKT_CONDENSED: return launch_condensed(h, p, v, stream);
        default: return launch_lane(h, p, v, stream);
    }
}

int ensure_host_ctx(mmpc_handle* h, size_t bytes) {
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    if (h->host_stream && h->host_dev != dev) return fail(MMPC_ERR_INVALID_ARG, "handle used on two devices");
    if (!h->host_stream) {
        MMPC_HIP(hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking));
        h->host_dev = dev;
    }
    if (bytes > h->d_buf_bytes) {
        if (h->d_buf) MMPC_HIP(hipFree(h->d_buf));
        h->d_buf = nullptr;
        h->d_buf_bytes = 0;
        MMPC_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_buf), bytes));
        h->d_buf_bytes = bytes;
    }
    return MMPC_OK;
}

// ---- sensitivity barrier of the gain and VJP calls (mmpc_set_sensitivity_barrier) ----
constexpr double kSensCapDefault = 1e12;
// the barrier value the monotone schedule of sqp_wave.h reaches first with 2 mu <= kIpTolCompl: where a state-bounded
// solve under the monotone rule ends unless an instance needed one more decrease
double sens_mu_default() {
    double mu = kIpMu0;
    while (2.0 * mu > kIpTolCompl)
        mu = std::fmax(kIpTolCompl / 20.0, std::fmin(kIpKappaMu * mu, std::pow(mu, kIpThetaMu)));
    return mu;
}
// What a gain or VJP call does about the handle's state bounds, read under their lock: xb->mu = 0 without a finite
// state bound (the setting has no effect there), the bounds and the barrier with one and the barrier on; with one
// and the barrier off the call is refused.
int read_sens_barrier(mmpc_handle* h, const char* what, XbTail* xb) {
    std::lock_guard<std::mutex> lk(h->xb_mu);
    *xb = XbTail{};
    if (!h->x_bounded) return MMPC_OK;
    if (!(h->sens_mu > 0.0))
        return fail(MMPC_ERR_UNSUPPORTED, std::string(what) + " not available with finite state bounds "
                                          "(barrier-smoothed sensitivities are not computed) unless the sensitivity "
                                          "barrier is switched on (mmpc_set_sensitivity_barrier)");
    for (int i = 0; i < 16; ++i) {
        xb->x_lb[i] = i < h->info.num_x ? h->x_lb[i] : -INFINITY;
        xb->x_ub[i] = i < h->info.num_x ? h->x_ub[i] : INFINITY;
    }
    xb->mu = h->sens_mu;
    xb->cap = h->sens_cap;
    return MMPC_OK;
}

// ---- what the gain and VJP calls share: arguments, check, kernel parameters, variant, staging ----
struct SensArgs {
    int64_t B = 0;
    const double *V = nullptr, *u_prev = nullptr, *traj = nullptr, *weights = nullptr;
    int64_t weights_stride = 0;
    const double *u_lb = nullptr, *u_ub = nullptr;
    int64_t bounds_stride = 0;
    int32_t n_pin = 0, hessian = 0;
    int32_t* status = nullptr;
    hipStream_t stream = nullptr;
};
// Where a call's own rules stand among the shared ones of check_sens_args: each after the shared rule it followed when
// the two checks were written out, so that of two bad arguments the one reported stays the same.
enum class SensRule { kAfterPin, kAfterHessian, kAfterVariant, kAfterInputs };
// The shared rules of a gain or VJP call's arguments: pure arithmetic on the arguments and the handle, before any
// device call.  what: the call as the refusals name it ("feedback gains are").  own(SensRule): the call's own rules.
// *exact: the Hessian the call runs (AUTO: exact wherever the model has second derivatives -- the true derivative is
// wanted whatever Hessian the solve ran, so this is not resolve_hessian).  *xb: read_sens_barrier's answer.
template <class Own>
int check_sens_args(mmpc_handle* h, const SensArgs& a, const char* what, bool* exact, XbTail* xb, Own own) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    const mmpc_model_info& mi = h->info;
    const int N = mi.num_shooting_nodes;
    if (a.n_pin < 0 || a.n_pin > N - 1)
        return fail(MMPC_ERR_INVALID_ARG, "n_pin must be 0 .. N - 1 (" + std::to_string(N - 1) + "), got " +
                                              std::to_string(a.n_pin));
    if (int rc = own(SensRule::kAfterPin)) return rc;
    if (a.B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    if (int rc = check_bounds_stride(mi, a.bounds_stride)) return rc;
    if (a.hessian < MMPC_HESSIAN_AUTO || a.hessian > MMPC_HESSIAN_EXACT)
        return fail(MMPC_ERR_INVALID_ARG, "hessian: not an mmpc_hessian value (" + std::to_string(a.hessian) + ")");
    if (int rc = own(SensRule::kAfterHessian)) return rc;
    if (mi.is_linear)
        return fail(MMPC_ERR_UNSUPPORTED, std::string(what) + " not available for a linear-mode model");
    if (int rc = read_sens_barrier(h, what, xb)) return rc;
    bool has_hess = false;
    with_model(mi.model_id, [&](auto* m) {
        has_hess = HasHess<std::remove_pointer_t<decltype(m)>>::value;
        return MMPC_OK;
    });
    if (a.hessian == MMPC_HESSIAN_EXACT && !has_hess)
        return fail(MMPC_ERR_UNSUPPORTED, "hessian = EXACT: the model has no second derivatives");
    *exact = a.hessian != MMPC_HESSIAN_GAUSS_NEWTON && has_hess;
    if (int rc = own(SensRule::kAfterVariant)) return rc;
    if (a.B == 0) return MMPC_OK;
    if (!a.V || !a.u_prev || !a.traj || !a.weights) return fail(MMPC_ERR_INVALID_ARG, "null input pointer");
    if (int rc = own(SensRule::kAfterInputs)) return rc;
    if (a.weights_stride != 0 && a.weights_stride < mi.num_x + 2 * mi.num_u)
        return fail(MMPC_ERR_INVALID_ARG, "weights_stride must be 0 or >= nx+2nu");
    if (a.B > 0x7fffffffLL) return fail(MMPC_ERR_INVALID_ARG, "B exceeds the grid limit (2^31-1)");
    return MMPC_OK;
}
// the head of a sensitivity kernel's parameters (SensParams, gain_sweep.h) and the barrier's tail
template <class Params>
void fill_sens_params(const mmpc_handle* h, const SensArgs& a, const XbTail& xb, Params& p) {
    p.xb = xb;
    p.B = a.B;
    p.N = h->info.num_shooting_nodes;
    p.h = h->info.step_size;
    p.V = a.V;
    p.u_prev = a.u_prev;
    p.traj = a.traj;
    p.weights = a.weights;
    p.w_stride = a.weights_stride;
    p.u_lb = a.u_lb;
    p.u_ub = a.u_ub;
    p.b_stride = static_cast<int32_t>(a.bounds_stride);
    p.n_pin = a.n_pin;
}
// f(EXACT, BOUNDED, XB) with the three flags of a call lifted to std::bool_constant's: the one place that knows the
// kernels of a model -- the exact Hessian only where the model has one, and XB implies BOUNDED.
template <class M, class F>
int with_sens_variant(bool exact, bool bounded, bool xb, F f) {
    const auto lift = [&](auto ex) {
        if (xb) return f(ex, std::true_type{}, std::true_type{});
        return bounded ? f(ex, std::true_type{}, std::false_type{}) : f(ex, std::false_type{}, std::false_type{});
    };
    if constexpr (HasHess<M>::value) {
        if (exact) return lift(std::true_type{});
    }
    return lift(std::false_type{});
}
// f() on the handle's device, which is the current one for the call's duration
template <class F>
int on_handle_device(mmpc_handle* h, F f) {
    int dev;
    if (int rc = resolve_device(h, &dev)) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    return f();
}
// The staging of a *_host sensitivity entry, in doubles of the handle's buffer:
//   V | (extra) | u_prev | traj | weights | u_lb | u_ub | (own) | status,
// extra and own being the entry's own regions.  Sizes the buffer, copies the six shared inputs to the device on the
// host stream and points a's inputs, status and stream at the staged copies.  *d: the buffer;  *off_extra, *off_own:
// where the entry's regions start.  The caller holds the host lock and has the handle's device current.
int stage_sens_inputs(mmpc_handle* h, SensArgs& a, size_t extra, size_t own, double** d, size_t* off_extra,
                      size_t* off_own) {
    const mmpc_model_info& mi = h->info;
    const size_t B = static_cast<size_t>(a.B), nx = mi.num_x, nu = mi.num_u, N = mi.num_shooting_nodes, NV = mi.num_v;
    const size_t nW = a.weights_stride ? B * static_cast<size_t>(a.weights_stride) : nx + 2 * nu;
    // staged bound doubles: the caller's buffer holds (B - 1) stride + nu of them and is never read past that
    const size_t nB = (a.bounds_stride ? B - 1 : 0) * static_cast<size_t>(a.bounds_stride) + nu;
    const size_t off_V = 0, off_x = off_V + B * NV, off_up = off_x + extra, off_tr = off_up + B * nu;
    const size_t off_w = off_tr + B * N * nx, off_lb = off_w + nW, off_ub = off_lb + nB, off_o = off_ub + nB;
    const size_t off_st = off_o + own, total = off_st + (B + 1) / 2;
    if (int rc = ensure_host_ctx(h, total * sizeof(double))) return rc;
    double* const b = h->d_buf;
    hipStream_t s = h->host_stream;
    MMPC_HIP(hipMemcpyAsync(b + off_V, a.V, B * NV * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(b + off_up, a.u_prev, B * nu * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(b + off_tr, a.traj, B * N * nx * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(b + off_w, a.weights, nW * sizeof(double), hipMemcpyHostToDevice, s));
    if (a.u_lb) MMPC_HIP(hipMemcpyAsync(b + off_lb, a.u_lb, nB * sizeof(double), hipMemcpyHostToDevice, s));
    if (a.u_ub) MMPC_HIP(hipMemcpyAsync(b + off_ub, a.u_ub, nB * sizeof(double), hipMemcpyHostToDevice, s));
    a.V = b + off_V;
    a.u_prev = b + off_up;
    a.traj = b + off_tr;
    a.weights = b + off_w;
    a.u_lb = a.u_lb ? b + off_lb : nullptr;
    a.u_ub = a.u_ub ? b + off_ub : nullptr;
    a.status = reinterpret_cast<int32_t*>(b + off_st);
    a.stream = s;
    *d = b;
    *off_extra = off_x;
    *off_own = off_o;
    return MMPC_OK;
}

// ---- feedback gains (mmpc_feedback_gains_batch; gain_sweep.h) ----
struct GainArgs : SensArgs {
    int32_t n_gain = 0, kernel = 0;
    double* G = nullptr;
};
// instances per workgroup of the 16-lane gain kernel: as many as fit 160 KB of LDS, 0 when one does not
int gain_group_gpw(const mmpc_model_info& mi, bool exact, bool xb) {
    const size_t inst =
        static_cast<size_t>(gain_group_lds_doubles(mi.num_x, mi.num_u, mi.num_shooting_nodes, exact, xb)) *
        sizeof(double);
    return static_cast<int>(std::min<size_t>(kGroupsPerWave, kMaxGroupLds / inst));
}
// The one check of a gain call's arguments: check_sens_args with the rules of n_gain, kernel and G_out.
int check_gain_args(mmpc_handle* h, const GainArgs& a, bool* exact, XbTail* xb) {
    return check_sens_args(h, a, "feedback gains are", exact, xb, [&](SensRule at) -> int {
        const mmpc_model_info& mi = h->info;
        const int N = mi.num_shooting_nodes;
        if (at == SensRule::kAfterPin && (a.n_gain < 1 || a.n_gain > N))
            return fail(MMPC_ERR_INVALID_ARG, "n_gain must be 1 .. N (" + std::to_string(N) + "), got " +
                                                  std::to_string(a.n_gain));
        if (at == SensRule::kAfterHessian && (a.kernel < MMPC_GAIN_KERNEL_AUTO || a.kernel > MMPC_GAIN_KERNEL_GROUP))
            return fail(MMPC_ERR_INVALID_ARG,
                        "kernel: not an mmpc_gain_kernel value (" + std::to_string(a.kernel) + ")");
        if (at == SensRule::kAfterVariant && a.kernel == MMPC_GAIN_KERNEL_GROUP) {
            if (mi.num_x + mi.num_u >= kGroupLanes)
                return fail(MMPC_ERR_UNSUPPORTED, "kernel = 2 (the 16-lane kernel) needs nx + nu < 16");
            if (gain_group_gpw(mi, *exact, xb->mu > 0.0) < 1)
                return fail(MMPC_ERR_UNSUPPORTED, "kernel = 2 (the 16-lane kernel): the stage records of one instance "
                                                  "exceed 160 KB of LDS at this horizon");
        }
        if (at == SensRule::kAfterInputs && !a.G) return fail(MMPC_ERR_INVALID_ARG, "G_out is NULL");
        return MMPC_OK;
    });
}
// The kernel a gain call of B instances runs (measured on one MI355X, tools/feedback_gains_cost.py): the
// 16-lane kernel while its workgroups are at most two per compute unit -- B <= 2 gpw CUs, gpw = the instances per
// workgroup the LDS admits -- where the model has nx + nu < 16 and an instance's records fit the LDS; one lane per
// instance beyond.  The two kernels cross between two and four workgroups per CU on both built-in models (cfg#2 shape:
// 59 against 68 us at B = 2048, 118 against 69 at 4096; exo N = 50, one instance per workgroup: 0.30 against 1.07 ms at
// B = 256, 1.21 against 1.08 at 1024): the lane kernel's time is flat in B up to 16384 instances, the 16-lane kernel's
// grows with the workgroups a CU has to take.  (The first rule, 16 B lanes within four waves per SIMD, was B <= 64 per
// CU.)
int resolve_gain_kernel(const mmpc_handle* h, int64_t B, bool exact, bool xb, int kernel) {
    if (kernel != MMPC_GAIN_KERNEL_AUTO) return kernel;
    const mmpc_model_info& mi = h->info;
    const int gpw = mi.num_x + mi.num_u < kGroupLanes ? gain_group_gpw(mi, exact, xb) : 0;
    return gpw >= 1 && B <= 2LL * gpw * h->cu_count ? MMPC_GAIN_KERNEL_GROUP : MMPC_GAIN_KERNEL_LANE;
}
template <class M, bool EXACT, bool BOUNDED, bool XB = false>
int launch_gain_kernels(int kernel, const GainParamsOf<XB>& p, size_t lds, hipStream_t stream) {
    if (kernel == MMPC_GAIN_KERNEL_LANE) {
        gain_lane_kernel<M, EXACT, BOUNDED, XB><<<grid1d(p.B, 64), 64, 0, stream>>>(p);
    } else if constexpr (M::NX + M::NU < kGroupLanes) {
        auto* const k = &gain_group_kernel<M, EXACT, BOUNDED, XB>;
        if (lds > 64 * 1024)   // gfx950: up to 160 KB per workgroup once the attribute is raised
            MMPC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         static_cast<int>(lds)));
        k<<<grid1d(p.B, p.gpw), 64, lds, stream>>>(p);
    } else {
        return fail(MMPC_ERR_UNSUPPORTED, "kernel = 2 (the 16-lane kernel) needs nx + nu < 16");
    }
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
}
// a gain call whose arguments check_gain_args has passed, B > 0, device pointers, on the current device: one launch,
// stream-ordered, no allocation, no synchronisation
int launch_gains(mmpc_handle* h, const GainArgs& a, bool exact, const XbTail& xb) {
    const mmpc_model_info& mi = h->info;
    if (a.kernel == MMPC_GAIN_KERNEL_AUTO)
        if (int rc = query_cu_count(h)) return rc;
    const bool xbv = xb.mu > 0.0;
    const int kernel = resolve_gain_kernel(h, a.B, exact, xbv, a.kernel);
    GainXbParams p{};
    fill_sens_params(h, a, xb, p);
    p.n_gain = a.n_gain;
    p.G = a.G;
    p.status = a.status;
    p.gpw = kernel == MMPC_GAIN_KERNEL_GROUP ? gain_group_gpw(mi, exact, xbv) : 1;
    const size_t lds = kernel == MMPC_GAIN_KERNEL_GROUP
                           ? static_cast<size_t>(gain_group_lds_doubles(mi.num_x, mi.num_u, p.N, exact, xbv)) * p.gpw *
                                 sizeof(double)
                           : 0;
    return with_model(mi.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        return with_sens_variant<M>(exact, a.u_lb || a.u_ub, xbv, [&](auto ex, auto bd, auto x) {
            return launch_gain_kernels<M, decltype(ex)::value, decltype(bd)::value, decltype(x)::value>(kernel, p, lds,
                                                                                                         a.stream);
        });
    });
}

// ---- reverse-mode product of the solve (mmpc_solve_vjp_batch; adjoint_sweep.h) ----
struct VjpArgs : SensArgs {
    const double* V_bar = nullptr;
    double *x0_bar = nullptr, *u_prev_bar = nullptr, *traj_bar = nullptr, *weights_bar = nullptr, *adj_V = nullptr;
    void* workspace = nullptr;
    uint64_t workspace_bytes = 0;
    bool forward() const { return traj_bar || weights_bar || adj_V; }   // else backward-only: no record, no workspace
};
// bytes of the record workspace of B instances: ceil(B / 64) blocks of (doubles per lane) x 64, lane-interleaved
uint64_t vjp_workspace_bytes(const mmpc_model_info& mi, int64_t B) {
    const uint64_t blocks = (static_cast<uint64_t>(B) + 63) / 64;
    return blocks * static_cast<uint64_t>(adjoint_lane_doubles(mi.num_x, mi.num_u, mi.num_shooting_nodes)) * 64 *
           sizeof(double);
}
// The one check of a VJP call's arguments: check_sens_args with the rules of V_bar and the workspace (the host entry
// brings its own workspace and passes check_workspace = false).
int check_vjp_args(mmpc_handle* h, const VjpArgs& a, bool check_workspace, bool* exact, XbTail* xb) {
    const int rc = check_sens_args(h, a, "the solve VJP is", exact, xb, [&](SensRule at) -> int {
        if (at == SensRule::kAfterInputs && !a.V_bar) return fail(MMPC_ERR_INVALID_ARG, "V_bar is NULL");
        return MMPC_OK;
    });
    if (rc || a.B == 0) return rc;
    if (check_workspace && a.forward()) {
        const uint64_t need = vjp_workspace_bytes(h->info, a.B);
        if (!a.workspace)
            return fail(MMPC_ERR_INVALID_ARG, "workspace is NULL: traj_bar, weights_bar and adj_V need " +
                                                  std::to_string(need) + " bytes (mmpc_solve_vjp_workspace_bytes)");
        if (a.workspace_bytes < need)
            return fail(MMPC_ERR_INVALID_ARG, "workspace_bytes is " + std::to_string(a.workspace_bytes) + ", needs " +
                                                  std::to_string(need) + " (mmpc_solve_vjp_workspace_bytes)");
    }
    return MMPC_OK;
}
// a VJP call whose arguments check_vjp_args has passed, B > 0, device pointers, on the current device: one launch,
// stream-ordered, no allocation, no synchronisation
int launch_vjp(mmpc_handle* h, const VjpArgs& a, bool exact, const XbTail& xb) {
    AdjointXbParams p{};
    fill_sens_params(h, a, xb, p);
    p.V_bar = a.V_bar;
    p.x0_bar = a.x0_bar;
    p.u_prev_bar = a.u_prev_bar;
    p.traj_bar = a.traj_bar;
    p.weights_bar = a.weights_bar;
    p.adj_V = a.adj_V;
    p.status = a.status;
    p.ws = a.forward() ? static_cast<double*>(a.workspace) : nullptr;
    return with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        return with_sens_variant<M>(exact, a.u_lb || a.u_ub, xb.mu > 0.0, [&](auto ex, auto bd, auto x) -> int {
            adjoint_lane_kernel<M, decltype(ex)::value, decltype(bd)::value, decltype(x)::value>
                <<<grid1d(p.B, 64), 64, 0, a.stream>>>(p);
            MMPC_HIP(hipGetLastError());
            return MMPC_OK;
        });
    });
}

// ---- forward-mode product of the solve (mmpc_solve_jvp_batch; tangent_sweep.h) ----
struct JvpArgs : SensArgs {
    const double *dx0 = nullptr, *du_prev = nullptr, *dtraj = nullptr, *dweights = nullptr;
    double *dV = nullptr, *du0 = nullptr;
    void* workspace = nullptr;
    uint64_t workspace_bytes = 0;
    bool forward() const { return dV != nullptr; }   // else forward-free: no record, no workspace
};
// The one check of a JVP call's arguments: check_sens_args with the rules of the tangents, the outputs and the
// workspace (the host entry brings its own workspace and passes check_workspace = false).  The record is the VJP's,
// and so is the workspace's size.
int check_jvp_args(mmpc_handle* h, const JvpArgs& a, bool check_workspace, bool* exact, XbTail* xb) {
    const int rc = check_sens_args(h, a, "the solve JVP is", exact, xb, [&](SensRule at) -> int {
        if (at != SensRule::kAfterInputs) return MMPC_OK;
        if (!a.dx0 && !a.du_prev && !a.dtraj && !a.dweights)
            return fail(MMPC_ERR_INVALID_ARG, "dx0, du_prev, dtraj and dweights are all NULL: no tangent");
        if (!a.dV && !a.du0) return fail(MMPC_ERR_INVALID_ARG, "dV and du0 are both NULL: no output");
        return MMPC_OK;
    });
    if (rc || a.B == 0) return rc;
    if (check_workspace && a.forward()) {
        const uint64_t need = vjp_workspace_bytes(h->info, a.B);
        if (!a.workspace)
            return fail(MMPC_ERR_INVALID_ARG, "workspace is NULL: dV needs " + std::to_string(need) +
                                                  " bytes (mmpc_solve_jvp_workspace_bytes)");
        if (a.workspace_bytes < need)
            return fail(MMPC_ERR_INVALID_ARG, "workspace_bytes is " + std::to_string(a.workspace_bytes) + ", needs " +
                                                  std::to_string(need) + " (mmpc_solve_jvp_workspace_bytes)");
    }
    return MMPC_OK;
}
// a JVP call whose arguments check_jvp_args has passed, B > 0, device pointers, on the current device: one launch,
// stream-ordered, no allocation, no synchronisation
int launch_jvp(mmpc_handle* h, const JvpArgs& a, bool exact, const XbTail& xb) {
    TangentXbParams p{};
    fill_sens_params(h, a, xb, p);
    p.dx0 = a.dx0;
    p.du_prev = a.du_prev;
    p.dtraj = a.dtraj;
    p.dweights = a.dweights;
    p.dV = a.dV;
    p.du0 = a.du0;
    p.status = a.status;
    p.ws = a.forward() ? static_cast<double*>(a.workspace) : nullptr;
    return with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        return with_sens_variant<M>(exact, a.u_lb || a.u_ub, xb.mu > 0.0, [&](auto ex, auto bd, auto x) -> int {
            tangent_lane_kernel<M, decltype(ex)::value, decltype(bd)::value, decltype(x)::value>
                <<<grid1d(p.B, 64), 64, 0, a.stream>>>(p);
            MMPC_HIP(hipGetLastError());
            return MMPC_OK;
        });
    });
}

// ---- real-time iteration (mmpc_rti_prepare_batch / mmpc_rti_feedback_batch; rti_sweep.h) ----
struct RtiArgs : SensArgs {   // the preparation's arguments are the head; the rest is the feedback launch's
    const double* x0_meas = nullptr;
    double *V_inout = nullptr, *u0 = nullptr, *step_inf = nullptr;
    int32_t* fb_status = nullptr;
    void* workspace = nullptr;
    uint64_t workspace_bytes = 0;
};
uint64_t rti_ws_bytes(const mmpc_model_info& mi, int64_t B) {
    return rti_workspace_bytes(mi.num_x, mi.num_u, mi.num_shooting_nodes, B);
}
// the two refusals every RTI entry shares, before the sensitivity barrier is looked at: a state-bounded handle is
// refused with the barrier on or off
int check_rti_handle(mmpc_handle* h) {
    if (h->info.is_linear)
        return fail(MMPC_ERR_UNSUPPORTED, "real-time iteration is not available for a linear-mode model");
    std::lock_guard<std::mutex> lk(h->xb_mu);
    if (h->x_bounded)
        return fail(MMPC_ERR_UNSUPPORTED, "real-time iteration is not available with finite state bounds, whether the "
                                          "sensitivity barrier is on or off (a one-step interior point is not computed)");
    return MMPC_OK;
}
int check_rti_workspace(mmpc_handle* h, const RtiArgs& a) {
    const uint64_t need = rti_ws_bytes(h->info, a.B);
    if (!a.workspace)
        return fail(MMPC_ERR_INVALID_ARG,
                    "workspace is NULL: needs " + std::to_string(need) + " bytes (mmpc_rti_workspace_bytes)");
    if (a.workspace_bytes < need)
        return fail(MMPC_ERR_INVALID_ARG, "workspace_bytes is " + std::to_string(a.workspace_bytes) + ", needs " +
                                              std::to_string(need) + " (mmpc_rti_workspace_bytes)");
    return MMPC_OK;
}
// The one check of a preparation's arguments: check_sens_args with the RTI refusals (the host entry brings its own
// workspace and passes check_workspace = false).
int check_rti_prepare_args(mmpc_handle* h, const RtiArgs& a, bool check_workspace, bool* exact) {
    XbTail xb;
    const int rc = check_sens_args(h, a, "real-time iteration is", exact, &xb, [&](SensRule at) -> int {
        return at == SensRule::kAfterHessian ? check_rti_handle(h) : MMPC_OK;
    });
    if (rc || a.B == 0 || !check_workspace) return rc;
    return check_rti_workspace(h, a);
}
// The one check of a feedback launch's arguments (it has no model inputs, so check_sens_args does not apply).
int check_rti_feedback_args(mmpc_handle* h, const RtiArgs& a) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (a.B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    if (int rc = check_bounds_stride(h->info, a.bounds_stride)) return rc;
    if (int rc = check_rti_handle(h)) return rc;
    if (a.B == 0) return MMPC_OK;
    if (!a.x0_meas) return fail(MMPC_ERR_INVALID_ARG, "x0_meas is NULL");
    if (!a.V_inout) return fail(MMPC_ERR_INVALID_ARG, "V_inout is NULL");
    if (a.B > 0x7fffffffLL) return fail(MMPC_ERR_INVALID_ARG, "B exceeds the grid limit (2^31-1)");
    return check_rti_workspace(h, a);
}
// the three regions of an RTI workspace of B instances: records | undo log | status words
struct RtiRegions {
    double *rec, *undo;
    int32_t* status;
};
RtiRegions rti_regions(const mmpc_model_info& mi, int64_t B, void* workspace) {
    const uint64_t blocks = (static_cast<uint64_t>(B) + 63) / 64;
    RtiRegions r;
    r.rec = static_cast<double*>(workspace);
    r.undo = r.rec + blocks * rti_rec_block_doubles(mi.num_x, mi.num_u, mi.num_shooting_nodes);
    r.status = reinterpret_cast<int32_t*>(r.undo +
                                          blocks * rti_undo_block_doubles(mi.num_x, mi.num_u, mi.num_shooting_nodes));
    return r;
}
// a preparation whose arguments check_rti_prepare_args has passed, B > 0, device pointers, on the current device: one
// launch, stream-ordered, no allocation, no synchronisation
int launch_rti_prepare(mmpc_handle* h, const RtiArgs& a, bool exact) {
    RtiPrepareXbParams px{};   // fill_sens_params writes the barrier's tail; the kernels take the head alone
    fill_sens_params(h, a, XbTail{}, px);
    const RtiRegions r = rti_regions(h->info, a.B, a.workspace);
    px.status = a.status;
    px.rec = r.rec;
    px.ws_status = r.status;
    const RtiPrepareParams p = px;
    return with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        return with_sens_variant<M>(exact, a.u_lb || a.u_ub, false, [&](auto ex, auto bd, auto) -> int {
            rti_prepare_lane_kernel<M, decltype(ex)::value, decltype(bd)::value><<<grid1d(p.B, 64), 64, 0, a.stream>>>(p);
            MMPC_HIP(hipGetLastError());
            return MMPC_OK;
        });
    });
}
// a feedback launch whose arguments check_rti_feedback_args has passed, on the same terms
int launch_rti_feedback(mmpc_handle* h, const RtiArgs& a) {
    const RtiRegions r = rti_regions(h->info, a.B, a.workspace);
    RtiFeedbackParams p{};
    p.B = a.B;
    p.N = h->info.num_shooting_nodes;
    p.x0 = a.x0_meas;
    p.u_lb = a.u_lb;
    p.u_ub = a.u_ub;
    p.b_stride = static_cast<int32_t>(a.bounds_stride);
    p.V = a.V_inout;
    p.u0 = a.u0;
    p.step_inf = a.step_inf;
    p.status = a.fb_status;
    p.rec = r.rec;
    p.undo = r.undo;
    p.ws_status = r.status;
    return with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        return with_sens_variant<M>(false, a.u_lb || a.u_ub, false, [&](auto, auto bd, auto) -> int {
            rti_feedback_lane_kernel<M::NX, M::NU, decltype(bd)::value><<<grid1d(p.B, 64), 64, 0, a.stream>>>(p);
            MMPC_HIP(hipGetLastError());
            return MMPC_OK;
        });
    });
}

// The one check of a shift's arguments.  State bounds are not looked at: the shift is also the warm start of a solve.
int check_rti_shift_args(mmpc_handle* h, int64_t B, const double* V_in, int32_t n_shift, const double* V_out) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    const int N = h->info.num_shooting_nodes;
    if (n_shift < 0 || n_shift > N)
        return fail(MMPC_ERR_INVALID_ARG,
                    "n_shift is " + std::to_string(n_shift) + ": must be 0 .. " + std::to_string(N));
    if (h->info.is_linear)
        return fail(MMPC_ERR_UNSUPPORTED, "real-time iteration is not available for a linear-mode model");
    if (B == 0) return MMPC_OK;
    if (!V_in) return fail(MMPC_ERR_INVALID_ARG, "V_in is NULL");
    if (!V_out) return fail(MMPC_ERR_INVALID_ARG, "V_out is NULL");
    if (V_out == V_in) return fail(MMPC_ERR_INVALID_ARG, "V_out is V_in: the two plans may not overlap");
    if (rti_shift_copy_blocks(B, h->info.num_v) + rti_shift_roll_blocks(B, n_shift) > 0x7fffffffULL)
        return fail(MMPC_ERR_INVALID_ARG, "B exceeds the grid limit of the shift (2^31-1 blocks)");
    return MMPC_OK;
}
// a shift whose arguments check_rti_shift_args has passed, B > 0, on the same terms as the launches above
int launch_rti_shift(mmpc_handle* h, int64_t B, const double* V_in, int32_t n_shift, double* V_out, double* u_prev_out,
                     hipStream_t stream) {
    RtiShiftParams p{};
    p.B = B;
    p.N = h->info.num_shooting_nodes;
    p.n = n_shift;
    p.h = h->info.step_size;
    p.V_in = V_in;
    p.V_out = V_out;
    p.u_prev = n_shift > 0 ? u_prev_out : nullptr;
    p.copy_blocks = static_cast<uint32_t>(rti_shift_copy_blocks(B, h->info.num_v));
    const unsigned grid = p.copy_blocks + static_cast<unsigned>(rti_shift_roll_blocks(B, n_shift));
    return with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        rti_shift_kernel<M><<<grid, kRtiShiftThreads, 0, stream>>>(p);
        MMPC_HIP(hipGetLastError());
        return static_cast<int>(MMPC_OK);
    });
}

}  // namespace

// ---------------------------------------------------------------- C-ABI
extern "C" {

int mmpc_abi_version(void) { return MMPC_ABI_VERSION; }

void mmpc_default_opts(mmpc_opts* o) {
    if (!o) return;
    o->max_iter = 200;  // reference IPOPT option, ModelControl.cpp:55
    o->device = -1;
    o->tol_grad = 1e-8;
    o->tol_defect = 1e-10;
    o->kkt_solver = MMPC_KKT_AUTO;
    o->factor_fp32 = 0;
    o->init_states = MMPC_INIT_AS_GIVEN;
    o->hessian = MMPC_HESSIAN_AUTO;
    o->tail_cap = -1;   // the iteration-tail hand-over's default policy
    o->tail_wave_max = -1;
    o->tail_rounds = -1;
}

int mmpc_create_from_json(const char* json_text, const mmpc_opts* opts, mmpc_handle** out) {
    if (!json_text || !out) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    mmpc_opts o;
    mmpc_default_opts(&o);
    if (opts) o = *opts;
    int rc = validate_opts(&o);
    if (rc) return rc;
    mmpc_model_info info;
    rc = parse_model(json_text, &info);
    if (rc) return rc;
    mmpc_handle* h = new (std::nothrow) mmpc_handle();
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "out of memory");
    h->info = info;
    h->nq = model_nq(info.model_id);
    for (int i = 0; i < info.num_x; ++i) {  // x_min/x_max of the JSON (ModelControl.cpp:37-50)
        h->x_lb[i] = info.x_min[i];
        h->x_ub[i] = info.x_max[i];
        h->x_bounded |= info.x_min[i] > -1e19 || info.x_max[i] < 1e19;
    }
    h->opts = o;
    if (const char* e = std::getenv("MMPC_TAIL_CAP")) {   // A/B and tests: the tail hand-over's cap (0 = off)
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && v >= 0 && v < 1000) h->tail_cap_env = static_cast<int>(v);
    }
    if (const char* e = std::getenv("MMPC_TAIL_WAVE")) {
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && v >= 0 && v <= 64) h->tail_wave_env = static_cast<int>(v);
    }
    if (const char* e = std::getenv("MMPC_BARRIER_RULE")) {   // measurement: the rule without a change of the caller
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && (v == MMPC_BARRIER_MONOTONE || v == MMPC_BARRIER_MEHROTRA)) h->barrier_rule = static_cast<int>(v);
    }
    if (const char* e = std::getenv("MMPC_TAIL_ROUNDS")) {
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && v > 0 && v < 1000) h->tail_rounds_env = static_cast<int>(v);
    }
    *out = h;
    g_last_error.clear();
    return MMPC_OK;
}

int mmpc_create(const char* path, const mmpc_opts* opts, mmpc_handle** out) {
    if (!path || !out) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    std::ifstream f(path);  // ModelControl.cpp:24 reads <model_name>.json
    if (!f) return fail(MMPC_ERR_IO, std::string("cannot open ") + path);
    std::stringstream ss;
    ss << f.rdbuf();
    return mmpc_create_from_json(ss.str().c_str(), opts, out);
}

int mmpc_destroy(mmpc_handle* h) {
    if (!h) return MMPC_OK;
    if (h->host_stream || h->d_buf) {
        DeviceGuard g(h->host_dev);
        if (h->d_buf) (void)hipFree(h->d_buf);
        if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    }
    if (h->ws) {
        DeviceGuard g(h->ws_dev);
        (void)hipFree(h->ws);
    }
    delete h;
    return MMPC_OK;
}

int mmpc_get_model_info(const mmpc_handle* h, mmpc_model_info* info) {
    if (!h || !info) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *info = h->info;
    return MMPC_OK;
}

int mmpc_set_opts(mmpc_handle* h, const mmpc_opts* opts) {
    if (!h || !opts) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    int rc = validate_opts(opts);
    if (rc) return rc;
    h->opts = *opts;
    return MMPC_OK;
}

int mmpc_set_state_bounds(mmpc_handle* h, const double* x_lb, const double* x_ub) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    std::lock_guard<std::mutex> lk(h->xb_mu);
    bool any = false;
    for (int i = 0; i < h->info.num_x; ++i) {
        const double l = x_lb ? x_lb[i] : -INFINITY, u = x_ub ? x_ub[i] : INFINITY;
        if (l != l || u != u || l > u) return fail(MMPC_ERR_INVALID_ARG, "state bounds: NaN or lower > upper");
        h->x_lb[i] = l;
        h->x_ub[i] = u;
        any |= l > -1e19 || u < 1e19;
    }
    h->x_bounded = any;
    return MMPC_OK;
}

int mmpc_get_state_bounds(const mmpc_handle* h, double* x_lb, double* x_ub) {
    if (!h || !x_lb || !x_ub) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < h->info.num_x; ++i) {
        x_lb[i] = h->x_lb[i];
        x_ub[i] = h->x_ub[i];
    }
    return MMPC_OK;
}

int mmpc_set_barrier_rule(mmpc_handle* h, int32_t rule) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (rule != MMPC_BARRIER_MONOTONE && rule != MMPC_BARRIER_MEHROTRA)
        return fail(MMPC_ERR_INVALID_ARG, "rule: not an mmpc_barrier_rule value (" + std::to_string(rule) + ")");
    std::lock_guard<std::mutex> lk(h->xb_mu);
    h->barrier_rule = rule;
    return MMPC_OK;
}

int mmpc_get_barrier_rule(const mmpc_handle* h, int32_t* rule) {
    if (!h || !rule) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *rule = h->barrier_rule;
    return MMPC_OK;
}

int mmpc_sensitivity_barrier_default(double* mu, double* sigma_cap) {
    if (!mu || !sigma_cap) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *mu = sens_mu_default();
    *sigma_cap = kSensCapDefault;
    return MMPC_OK;
}

int mmpc_set_sensitivity_barrier(mmpc_handle* h, double mu, double sigma_cap) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (!(mu >= 0.0) || !std::isfinite(mu))
        return fail(MMPC_ERR_INVALID_ARG, "mu must be finite and >= 0 (0 switches the barrier off), got " +
                                              std::to_string(mu));
    if (!(sigma_cap > 0.0))
        return fail(MMPC_ERR_INVALID_ARG, "sigma_cap must be > 0 (+inf: no cap), got " + std::to_string(sigma_cap));
    std::lock_guard<std::mutex> lk(h->xb_mu);
    h->sens_mu = mu;
    h->sens_cap = sigma_cap;
    return MMPC_OK;
}

int mmpc_get_sensitivity_barrier(const mmpc_handle* h, double* mu, double* sigma_cap) {
    if (!h || !mu || !sigma_cap) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *mu = h->sens_mu;
    *sigma_cap = h->sens_cap;
    return MMPC_OK;
}

int mmpc_reserve_workspace(mmpc_handle* h, int64_t B, uint64_t* bytes) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    // reserved_layout: every horizon's solver workspace, hand-over list and resume workspace (sized by the device's CUs:
    // 256 until a device was queried), then the pinned solves' staging area
    auto total = [&]() { return reserved_layout(h, B, h->cu_count > 0 ? h->cu_count : 256).total; };
    if (bytes) *bytes = B == 0 ? 0 : total();
    if (B == 0) return MMPC_OK;
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    if ((rc = query_cu_count(h))) return rc;
    if (bytes) *bytes = total();
    double* ws = nullptr;
    return ensure_workspace_bytes(h, total(), &ws);
}

int mmpc_solve_batch(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev, const double* traj,
                     const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                     double* V_inout, int32_t* status, int32_t* iters, double* kkt_res, void* stream) {
    return mmpc_solve_batch_u0(h, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, V_inout, status, iters,
                               kkt_res, nullptr, stream);
}

int mmpc_solve_batch_u0(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev, const double* traj,
                        const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                        double* V_inout, int32_t* status, int32_t* iters, double* kkt_res, double* u0_out,
                        void* stream) {
    return mmpc_solve_batch_bounds(h, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, 0, V_inout, status,
                                   iters, kkt_res, u0_out, stream);
}

int mmpc_solve_batch_bounds(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev, const double* traj,
                            const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                            int64_t bounds_stride, double* V_inout, int32_t* status, int32_t* iters, double* kkt_res,
                            double* u0_out, void* stream) {
    return mmpc_solve_batch_pinned(h, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, nullptr,
                                   0, V_inout, status, iters, kkt_res, u0_out, stream);
}

// the device-pointer entry of every solve
int mmpc_solve_batch_pinned(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev, const double* traj,
                            const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                            int64_t bounds_stride, const double* u_pin, int32_t n_pin, double* V_inout,
                            int32_t* status, int32_t* iters, double* kkt_res, double* u0_out, void* stream) {
    const SolveArgs a{B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, u_pin, n_pin, V_inout,
                      status, iters, kkt_res, u0_out, reinterpret_cast<hipStream_t>(stream)};
    if (int rc = check_solve_args(h ? &h->info : nullptr, a)) return rc;
    if (B == 0) return MMPC_OK;
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    return launch_solve(h, a);
}

int mmpc_host_alloc(uint64_t bytes, void** out) {
    if (!out) return fail(MMPC_ERR_INVALID_ARG, "null output pointer");
    *out = nullptr;
    if (bytes == 0) return MMPC_OK;
    // pinned, mapped into every device's address space at the same address, coherent (uncached on the device
    // side): a kernel's stores land in host memory, visible to the host once the stream's work has completed
    if (hipHostMalloc(out, bytes, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess) {
        *out = nullptr;
        return fail(MMPC_ERR_HIP, "hipHostMalloc failed");
    }
    return MMPC_OK;
}

int mmpc_host_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) return fail(MMPC_ERR_HIP, "hipHostFree failed");
    return MMPC_OK;
}

int mmpc_solve_batch_host(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev, const double* traj,
                          const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                          double* V_inout, int32_t* status, int32_t* iters, double* kkt_res) {
    return mmpc_solve_batch_host_bounds(h, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, 0, V_inout,
                                        status, iters, kkt_res);
}

int mmpc_solve_batch_host_bounds(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                                 const double* traj, const double* weights, int64_t weights_stride,
                                 const double* u_lb, const double* u_ub, int64_t bounds_stride, double* V_inout,
                                 int32_t* status, int32_t* iters, double* kkt_res) {
    return mmpc_solve_batch_host_pinned(h, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride,
                                        nullptr, 0, V_inout, status, iters, kkt_res);
}

// the host entry of every solve: n_pin = 0 stages and launches exactly what mmpc_solve_batch_host_bounds always did
int mmpc_solve_batch_host_pinned(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev,
                                 const double* traj, const double* weights, int64_t weights_stride,
                                 const double* u_lb, const double* u_ub, int64_t bounds_stride, const double* u_pin,
                                 int32_t n_pin, double* V_inout, int32_t* status, int32_t* iters, double* kkt_res) {
    SolveArgs a{B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, u_pin, n_pin, V_inout,
                status, iters, kkt_res};
    // before the bound rows are scanned and weights_stride sizes a copy
    if (int rc = check_solve_args(h ? &h->info : nullptr, a)) return rc;
    if (B == 0) return MMPC_OK;
    std::lock_guard<std::mutex> lk(h->host_mu);
    const mmpc_model_info& mi = h->info;
    const size_t nx = mi.num_x, nu = mi.num_u, N = mi.num_shooting_nodes, NV = mi.num_v;
    // bounds that are all infinite (|b| >= 1e19, the reference's +-1e31 defaults) select the unbounded kernels:
    // every row of per-instance bounds is scanned, its nu entries only (not the padding of a wider stride)
    const size_t bst = static_cast<size_t>(bounds_stride), brows = bst ? static_cast<size_t>(B) : 1;
    bool lb_finite = false, ub_finite = false;
    for (size_t b = 0; b < brows; ++b)
        for (size_t c = 0; c < nu; ++c) {
            lb_finite |= u_lb && u_lb[b * bst + c] > -1e19;
            ub_finite |= u_ub && u_ub[b * bst + c] < 1e19;
        }
    if (!lb_finite && !ub_finite) u_lb = u_ub = nullptr;
    const size_t nw = nx + 2 * nu;
    const size_t nW = weights_stride ? (size_t)B * (size_t)weights_stride : nw;
    // staged bound doubles: the caller's buffer holds (B - 1) stride + nu of them and is never read past that
    const size_t nB = (brows - 1) * bst + nu;
    // doubles: x0, u_prev, traj, weights, lb, ub, V, kkt ; ints: status, iters (as doubles' room)
    const size_t off_x0 = 0, off_up = off_x0 + B * nx, off_tr = off_up + B * nu, off_w = off_tr + B * N * nx;
    const size_t off_lb = off_w + nW, off_ub = off_lb + nB, off_V = off_ub + nB, off_kkt = off_V + B * NV;
    const size_t off_st = off_kkt + B, off_it = off_st + (B + 1) / 2, off_pin = off_it + (B + 1) / 2;
    const size_t nP = static_cast<size_t>(B) * static_cast<size_t>(n_pin) * nu, total = off_pin + nP;   // pins last
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    rc = ensure_host_ctx(h, total * sizeof(double));
    if (rc) return rc;
    double* d = h->d_buf;
    hipStream_t s = h->host_stream;
    MMPC_HIP(hipMemcpyAsync(d + off_x0, x0, B * nx * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(d + off_up, u_prev, B * nu * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(d + off_tr, traj, B * N * nx * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(d + off_w, weights, nW * sizeof(double), hipMemcpyHostToDevice, s));
    if (u_lb) MMPC_HIP(hipMemcpyAsync(d + off_lb, u_lb, nB * sizeof(double), hipMemcpyHostToDevice, s));
    if (u_ub) MMPC_HIP(hipMemcpyAsync(d + off_ub, u_ub, nB * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(d + off_V, V_inout, B * NV * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_pin > 0) MMPC_HIP(hipMemcpyAsync(d + off_pin, u_pin, nP * sizeof(double), hipMemcpyHostToDevice, s));
    int32_t* dst = reinterpret_cast<int32_t*>(d + off_st);
    int32_t* dit = reinterpret_cast<int32_t*>(d + off_it);
    a = SolveArgs{B, d + off_x0, d + off_up, d + off_tr, d + off_w, weights_stride, u_lb ? d + off_lb : nullptr,
                  u_ub ? d + off_ub : nullptr, bounds_stride, n_pin > 0 ? d + off_pin : nullptr, n_pin, d + off_V, dst,
                  dit, d + off_kkt, nullptr, s};   // the staged copies
    if ((rc = launch_solve(h, a))) return rc;
    MMPC_HIP(hipMemcpyAsync(V_inout, d + off_V, B * NV * sizeof(double), hipMemcpyDeviceToHost, s));
    if (status) MMPC_HIP(hipMemcpyAsync(status, dst, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (iters) MMPC_HIP(hipMemcpyAsync(iters, dit, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (kkt_res) MMPC_HIP(hipMemcpyAsync(kkt_res, d + off_kkt, B * sizeof(double), hipMemcpyDeviceToHost, s));
    MMPC_HIP(hipStreamSynchronize(s));
    return MMPC_OK;
}

int mmpc_feedback_gains_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                              const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                              int64_t bounds_stride, int32_t n_pin, int32_t n_gain, int32_t hessian, int32_t kernel,
                              double* G_out, int32_t* gain_status, void* stream) {
    const GainArgs a{{B, V, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin, hessian,
                      gain_status, reinterpret_cast<hipStream_t>(stream)}, n_gain, kernel, G_out};
    bool exact = false;
    XbTail xb;
    if (int rc = check_gain_args(h, a, &exact, &xb)) return rc;
    if (B == 0) return MMPC_OK;
    return on_handle_device(h, [&] { return launch_gains(h, a, exact, xb); });
}

int mmpc_feedback_gains_batch_host(mmpc_handle* h, int64_t B, const double* V, const double* u_prev,
                                   const double* traj, const double* weights, int64_t weights_stride,
                                   const double* u_lb, const double* u_ub, int64_t bounds_stride, int32_t n_pin,
                                   int32_t n_gain, int32_t hessian, int32_t kernel, double* G_out,
                                   int32_t* gain_status) {
    GainArgs a{{B, V, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin, hessian}, n_gain,
               kernel, G_out};
    bool exact = false;
    XbTail xb;
    if (int rc = check_gain_args(h, a, &exact, &xb)) return rc;   // before weights_stride and bounds_stride size a copy
    if (B == 0) return MMPC_OK;
    std::lock_guard<std::mutex> lk(h->host_mu);
    return on_handle_device(h, [&]() -> int {
        const mmpc_model_info& mi = h->info;
        const size_t nu = mi.num_u, nG = static_cast<size_t>(B) * static_cast<size_t>(n_gain) * nu * (mi.num_x + nu);
        double* d;
        size_t off_x, off_G;
        if (int rc = stage_sens_inputs(h, a, 0, nG, &d, &off_x, &off_G)) return rc;
        a.G = d + off_G;
        if (int rc = launch_gains(h, a, exact, xb)) return rc;
        hipStream_t s = a.stream;
        MMPC_HIP(hipMemcpyAsync(G_out, d + off_G, nG * sizeof(double), hipMemcpyDeviceToHost, s));
        if (gain_status)
            MMPC_HIP(hipMemcpyAsync(gain_status, a.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        MMPC_HIP(hipStreamSynchronize(s));
        return MMPC_OK;
    });
}

int mmpc_solve_vjp_workspace_bytes(const mmpc_handle* h, int64_t B, uint64_t* bytes) {
    if (!h || !bytes || B < 0) return fail(MMPC_ERR_INVALID_ARG, "null argument or B < 0");
    *bytes = vjp_workspace_bytes(h->info, B);
    return MMPC_OK;
}

int mmpc_solve_vjp_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                         const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                         int64_t bounds_stride, int32_t n_pin, const double* V_bar, int32_t hessian, double* x0_bar,
                         double* u_prev_bar, double* traj_bar, double* weights_bar, double* adj_V, int32_t* vjp_status,
                         void* workspace, uint64_t workspace_bytes, void* stream) {
    const VjpArgs a{{B, V, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin, hessian,
                     vjp_status, reinterpret_cast<hipStream_t>(stream)},
                    V_bar, x0_bar, u_prev_bar, traj_bar, weights_bar, adj_V, workspace, workspace_bytes};
    bool exact = false;
    XbTail xb;
    if (int rc = check_vjp_args(h, a, true, &exact, &xb)) return rc;
    if (B == 0) return MMPC_OK;
    return on_handle_device(h, [&] { return launch_vjp(h, a, exact, xb); });
}

int mmpc_solve_vjp_batch_host(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                              const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                              int64_t bounds_stride, int32_t n_pin, const double* V_bar, int32_t hessian,
                              double* x0_bar, double* u_prev_bar, double* traj_bar, double* weights_bar, double* adj_V,
                              int32_t* vjp_status) {
    VjpArgs a{{B, V, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin, hessian},
              V_bar, x0_bar, u_prev_bar, traj_bar, weights_bar, adj_V};
    bool exact = false;
    XbTail xb;
    if (int rc = check_vjp_args(h, a, false, &exact, &xb)) return rc;   // before the strides size a copy
    if (B == 0) return MMPC_OK;
    std::lock_guard<std::mutex> lk(h->host_mu);
    return on_handle_device(h, [&]() -> int {
        const mmpc_model_info& mi = h->info;
        const size_t nx = mi.num_x, nu = mi.num_u, N = mi.num_shooting_nodes, NV = mi.num_v, nw = nx + 2 * nu;
        const size_t nWs = a.forward() ? vjp_workspace_bytes(mi, B) / sizeof(double) : 0;
        // own regions: V_bar after V;  x0_bar | u_prev_bar | traj_bar | weights_bar | adj_V | the records after u_ub
        double* d;
        size_t off_Vb, off_x0b;
        const size_t n_own = B * nx + B * nu + B * N * nx + B * nw + B * NV + nWs;
        if (int rc = stage_sens_inputs(h, a, B * NV, n_own, &d, &off_Vb, &off_x0b)) return rc;
        const size_t off_upb = off_x0b + B * nx, off_trb = off_upb + B * nu, off_wb = off_trb + B * N * nx;
        const size_t off_a = off_wb + B * nw, off_ws = off_a + B * NV;
        hipStream_t s = a.stream;
        MMPC_HIP(hipMemcpyAsync(d + off_Vb, V_bar, B * NV * sizeof(double), hipMemcpyHostToDevice, s));
        a.V_bar = d + off_Vb;
        a.x0_bar = x0_bar ? d + off_x0b : nullptr;
        a.u_prev_bar = u_prev_bar ? d + off_upb : nullptr;
        a.traj_bar = traj_bar ? d + off_trb : nullptr;
        a.weights_bar = weights_bar ? d + off_wb : nullptr;
        a.adj_V = adj_V ? d + off_a : nullptr;
        a.workspace = nWs ? d + off_ws : nullptr;
        a.workspace_bytes = nWs * sizeof(double);
        if (int rc = launch_vjp(h, a, exact, xb)) return rc;
        const auto back = [&](double* dst_host, size_t off, size_t n) {
            return dst_host ? hipMemcpyAsync(dst_host, d + off, n * sizeof(double), hipMemcpyDeviceToHost, s)
                            : hipSuccess;
        };
        MMPC_HIP(back(x0_bar, off_x0b, B * nx));
        MMPC_HIP(back(u_prev_bar, off_upb, B * nu));
        MMPC_HIP(back(traj_bar, off_trb, B * N * nx));
        MMPC_HIP(back(weights_bar, off_wb, B * nw));
        MMPC_HIP(back(adj_V, off_a, B * NV));
        if (vjp_status) MMPC_HIP(hipMemcpyAsync(vjp_status, a.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        MMPC_HIP(hipStreamSynchronize(s));
        return MMPC_OK;
    });
}

int mmpc_solve_jvp_workspace_bytes(const mmpc_handle* h, int64_t B, uint64_t* bytes) {
    if (!h || !bytes || B < 0) return fail(MMPC_ERR_INVALID_ARG, "null argument or B < 0");
    *bytes = vjp_workspace_bytes(h->info, B);
    return MMPC_OK;
}

int mmpc_solve_jvp_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                         const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                         int64_t bounds_stride, int32_t n_pin, const double* dx0, const double* du_prev,
                         const double* dtraj, const double* dweights, int32_t hessian, double* dV, double* du0,
                         int32_t* jvp_status, void* workspace, uint64_t workspace_bytes, void* stream) {
    JvpArgs a;
    static_cast<SensArgs&>(a) = SensArgs{B, V, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin,
                                         hessian, jvp_status, reinterpret_cast<hipStream_t>(stream)};
    a.dx0 = dx0, a.du_prev = du_prev, a.dtraj = dtraj, a.dweights = dweights;
    a.dV = dV, a.du0 = du0, a.workspace = workspace, a.workspace_bytes = workspace_bytes;
    bool exact = false;
    XbTail xb;
    if (int rc = check_jvp_args(h, a, true, &exact, &xb)) return rc;
    if (B == 0) return MMPC_OK;
    return on_handle_device(h, [&] { return launch_jvp(h, a, exact, xb); });
}

int mmpc_solve_jvp_batch_host(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                              const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                              int64_t bounds_stride, int32_t n_pin, const double* dx0, const double* du_prev,
                              const double* dtraj, const double* dweights, int32_t hessian, double* dV, double* du0,
                              int32_t* jvp_status) {
    JvpArgs a;
    static_cast<SensArgs&>(a) =
        SensArgs{B, V, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin, hessian};
    a.dx0 = dx0, a.du_prev = du_prev, a.dtraj = dtraj, a.dweights = dweights;
    a.dV = dV, a.du0 = du0;
    bool exact = false;
    XbTail xb;
    if (int rc = check_jvp_args(h, a, false, &exact, &xb)) return rc;   // before the strides size a copy
    if (B == 0) return MMPC_OK;
    std::lock_guard<std::mutex> lk(h->host_mu);
    return on_handle_device(h, [&]() -> int {
        const mmpc_model_info& mi = h->info;
        const size_t nx = mi.num_x, nu = mi.num_u, N = mi.num_shooting_nodes, NV = mi.num_v, nw = nx + 2 * nu;
        const size_t nWs = a.forward() ? vjp_workspace_bytes(mi, B) / sizeof(double) : 0;
        // own regions, after u_ub: dx0 | du_prev | dtraj | dweights | dV | du0 | the records
        double* d;
        size_t off_none, off_dx0;
        const size_t n_own = B * nx + B * nu + B * N * nx + B * nw + B * NV + B * nu + nWs;
        if (int rc = stage_sens_inputs(h, a, 0, n_own, &d, &off_none, &off_dx0)) return rc;
        const size_t off_dup = off_dx0 + B * nx, off_dtr = off_dup + B * nu, off_dw = off_dtr + B * N * nx;
        const size_t off_dV = off_dw + B * nw, off_du0 = off_dV + B * NV, off_ws = off_du0 + B * nu;
        hipStream_t s = a.stream;
        const auto in = [&](const double*& src, size_t off, size_t n) {
            if (!src) return hipSuccess;
            const hipError_t e = hipMemcpyAsync(d + off, src, n * sizeof(double), hipMemcpyHostToDevice, s);
            src = d + off;
            return e;
        };
        MMPC_HIP(in(a.dx0, off_dx0, B * nx));
        MMPC_HIP(in(a.du_prev, off_dup, B * nu));
        MMPC_HIP(in(a.dtraj, off_dtr, B * N * nx));
        MMPC_HIP(in(a.dweights, off_dw, B * nw));
        a.dV = dV ? d + off_dV : nullptr;
        a.du0 = du0 ? d + off_du0 : nullptr;
        a.workspace = nWs ? d + off_ws : nullptr;
        a.workspace_bytes = nWs * sizeof(double);
        if (int rc = launch_jvp(h, a, exact, xb)) return rc;
        if (dV) MMPC_HIP(hipMemcpyAsync(dV, d + off_dV, B * NV * sizeof(double), hipMemcpyDeviceToHost, s));
        if (du0) MMPC_HIP(hipMemcpyAsync(du0, d + off_du0, B * nu * sizeof(double), hipMemcpyDeviceToHost, s));
        if (jvp_status) MMPC_HIP(hipMemcpyAsync(jvp_status, a.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        MMPC_HIP(hipStreamSynchronize(s));
        return MMPC_OK;
    });
}

int mmpc_rti_workspace_bytes(const mmpc_handle* h, int64_t B, uint64_t* bytes) {
    if (!h || !bytes || B < 0) return fail(MMPC_ERR_INVALID_ARG, "null argument or B < 0");
    *bytes = rti_ws_bytes(h->info, B);
    return MMPC_OK;
}

int mmpc_rti_prepare_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                           const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                           int64_t bounds_stride, int32_t n_pin, int32_t hessian, int32_t* prep_status,
                           void* workspace, uint64_t workspace_bytes, void* stream) {
    RtiArgs a;
    static_cast<SensArgs&>(a) = SensArgs{B, V, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin,
                                         hessian, prep_status, reinterpret_cast<hipStream_t>(stream)};
    a.workspace = workspace, a.workspace_bytes = workspace_bytes;
    bool exact = false;
    if (int rc = check_rti_prepare_args(h, a, true, &exact)) return rc;
    if (B == 0) return MMPC_OK;
    return on_handle_device(h, [&] { return launch_rti_prepare(h, a, exact); });
}

int mmpc_rti_feedback_batch(mmpc_handle* h, int64_t B, const double* x0_meas, const double* u_lb, const double* u_ub,
                            int64_t bounds_stride, double* V_inout, double* u0_out, double* step_inf, int32_t* status,
                            void* workspace, uint64_t workspace_bytes, void* stream) {
    RtiArgs a;
    a.B = B, a.u_lb = u_lb, a.u_ub = u_ub, a.bounds_stride = bounds_stride;
    a.stream = reinterpret_cast<hipStream_t>(stream);
    a.x0_meas = x0_meas, a.V_inout = V_inout, a.u0 = u0_out, a.step_inf = step_inf, a.fb_status = status;
    a.workspace = workspace, a.workspace_bytes = workspace_bytes;
    if (int rc = check_rti_feedback_args(h, a)) return rc;
    if (B == 0) return MMPC_OK;
    return on_handle_device(h, [&] { return launch_rti_feedback(h, a); });
}

int mmpc_rti_shift_batch(mmpc_handle* h, int64_t B, const double* V_in, int32_t n_shift, double* V_out,
                         double* u_prev_out, void* stream) {
    if (int rc = check_rti_shift_args(h, B, V_in, n_shift, V_out)) return rc;
    if (B == 0) return MMPC_OK;
    return on_handle_device(h, [&] {
        return launch_rti_shift(h, B, V_in, n_shift, V_out, u_prev_out, reinterpret_cast<hipStream_t>(stream));
    });
}

int mmpc_rti_step_batch_host(mmpc_handle* h, int64_t B, double* V_inout, const double* x0_meas, const double* u_prev,
                             const double* traj, const double* weights, int64_t weights_stride, const double* u_lb,
                             const double* u_ub, int64_t bounds_stride, int32_t n_pin, int32_t hessian, double* u0_out,
                             double* step_inf, int32_t* status) {
    RtiArgs a;
    static_cast<SensArgs&>(a) =
        SensArgs{B, V_inout, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, n_pin, hessian};
    bool exact = false;
    if (int rc = check_rti_prepare_args(h, a, false, &exact)) return rc;   // before the strides size a copy
    if (B == 0) return MMPC_OK;
    if (!x0_meas) return fail(MMPC_ERR_INVALID_ARG, "x0_meas is NULL");
    std::lock_guard<std::mutex> lk(h->host_mu);
    return on_handle_device(h, [&]() -> int {
        const mmpc_model_info& mi = h->info;
        const size_t nx = mi.num_x, nu = mi.num_u, NV = mi.num_v;
        const size_t nWs = rti_ws_bytes(mi, B) / sizeof(double);
        // own regions, after u_ub: x0_meas | u0 | step_inf | the workspace
        double* d;
        size_t off_none, off_x0;
        if (int rc = stage_sens_inputs(h, a, 0, B * nx + B * nu + B + nWs, &d, &off_none, &off_x0)) return rc;
        const size_t off_u0 = off_x0 + B * nx, off_si = off_u0 + B * nu, off_ws = off_si + B;
        hipStream_t s = a.stream;
        MMPC_HIP(hipMemcpyAsync(d + off_x0, x0_meas, B * nx * sizeof(double), hipMemcpyHostToDevice, s));
        a.x0_meas = d + off_x0;
        a.V_inout = d;   // the staged V, first in the buffer
        a.u0 = d + off_u0;
        a.step_inf = d + off_si;
        a.fb_status = a.status;
        a.status = nullptr;   // the feedback launch's status carries the preparation's
        a.workspace = d + off_ws;
        a.workspace_bytes = nWs * sizeof(double);
        if (int rc = launch_rti_prepare(h, a, exact)) return rc;
        if (int rc = launch_rti_feedback(h, a)) return rc;
        MMPC_HIP(hipMemcpyAsync(V_inout, d, B * NV * sizeof(double), hipMemcpyDeviceToHost, s));
        if (u0_out) MMPC_HIP(hipMemcpyAsync(u0_out, d + off_u0, B * nu * sizeof(double), hipMemcpyDeviceToHost, s));
        if (step_inf) MMPC_HIP(hipMemcpyAsync(step_inf, d + off_si, B * sizeof(double), hipMemcpyDeviceToHost, s));
        if (status) MMPC_HIP(hipMemcpyAsync(status, a.fb_status, B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        MMPC_HIP(hipStreamSynchronize(s));
        return MMPC_OK;
    });
}

int mmpc_resolve_kkt_solver(const mmpc_handle* h, int64_t B, int32_t* solver) {
    if (!h || !solver || B < 0) return fail(MMPC_ERR_INVALID_ARG, "bad argument");
    *solver = resolve_kkt_solver(h, B);
    return MMPC_OK;
}

int mmpc_resolve_hessian(const mmpc_handle* h, int64_t B, int32_t u_bounded, int32_t* hessian) {
    if (!h || !hessian || B < 0) return fail(MMPC_ERR_INVALID_ARG, "null argument or B < 0");
    const int r = resolve_hessian(h, resolve_kkt_solver(h, B), u_bounded != 0);
    if (r < 0) return r;
    *hessian = r;
    return MMPC_OK;
}

int mmpc_linearize_batch(mmpc_handle* h, int64_t B, const double* x, const double* u, double* A_colmajor,
                         double* B_colmajor, double* xdot, void* stream) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    if (B == 0) return MMPC_OK;
    if (!x || !u) return fail(MMPC_ERR_INVALID_ARG, "null input pointer");
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    rc = with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        linearize_kernel<M><<<grid1d(B, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
            B, x, u, A_colmajor, B_colmajor, xdot);
        return MMPC_OK;
    });
    if (rc) return rc;
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
}

int mmpc_linearize_batch_host(mmpc_handle* h, int64_t B, const double* x, const double* u, double* A_colmajor,
                              double* B_colmajor, double* xdot) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    if (B == 0) return MMPC_OK;
    if (!x || !u) return fail(MMPC_ERR_INVALID_ARG, "null input pointer");
    std::lock_guard<std::mutex> lk(h->host_mu);
    const size_t nx = h->info.num_x, nu = h->info.num_u;
    const size_t off_x = 0, off_u = B * nx, off_A = off_u + B * nu, off_B = off_A + B * nx * nx,
                 off_f = off_B + B * nx * nu, total = off_f + B * nx;
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    rc = ensure_host_ctx(h, total * sizeof(double));
    if (rc) return rc;
    double* d = h->d_buf;
    hipStream_t s = h->host_stream;
    MMPC_HIP(hipMemcpyAsync(d + off_x, x, B * nx * sizeof(double), hipMemcpyHostToDevice, s));
    MMPC_HIP(hipMemcpyAsync(d + off_u, u, B * nu * sizeof(double), hipMemcpyHostToDevice, s));
    rc = mmpc_linearize_batch(h, B, d + off_x, d + off_u, d + off_A, d + off_B, d + off_f, s);
    if (rc) return rc;
    if (A_colmajor) MMPC_HIP(hipMemcpyAsync(A_colmajor, d + off_A, B * nx * nx * sizeof(double), hipMemcpyDeviceToHost, s));
    if (B_colmajor) MMPC_HIP(hipMemcpyAsync(B_colmajor, d + off_B, B * nx * nu * sizeof(double), hipMemcpyDeviceToHost, s));
    if (xdot) MMPC_HIP(hipMemcpyAsync(xdot, d + off_f, B * nx * sizeof(double), hipMemcpyDeviceToHost, s));
    MMPC_HIP(hipStreamSynchronize(s));
    return MMPC_OK;
}

int mmpc_nlp_eval_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                        const double* weights, int64_t weights_stride, double* J, double* defect_inf, void* stream) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    if (B == 0) return MMPC_OK;
    if (!V || !u_prev || !traj || !weights) return fail(MMPC_ERR_INVALID_ARG, "null input pointer");
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    rc = with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        nlp_eval_kernel<M><<<grid1d(B, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
            B, h->info.num_shooting_nodes, h->info.step_size, h->info.is_linear, V, u_prev, traj, weights,
            weights_stride, J, defect_inf);
        return MMPC_OK;
    });
    if (rc) return rc;
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
}

int mmpc_nlp_derivs_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                          const double* weights, int64_t weights_stride, double* J, double* grad, double* jac_blocks,
                          void* stream) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (B < 0) return fail(MMPC_ERR_INVALID_ARG, "B < 0");
    if (B == 0) return MMPC_OK;
    if (!V || !u_prev || !traj || !weights) return fail(MMPC_ERR_INVALID_ARG, "null input pointer");
    const int nw = h->info.num_x + 2 * h->info.num_u;
    if (weights_stride != 0 && weights_stride < nw) return fail(MMPC_ERR_INVALID_ARG, "weights_stride must be 0 or >= nx+2nu");
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    rc = with_model(h->info.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        nlp_derivs_kernel<M><<<grid1d(B, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
            B, h->info.num_shooting_nodes, h->info.step_size, h->info.is_linear, V, u_prev, traj, weights,
            weights_stride, J, grad, jac_blocks);
        return MMPC_OK;
    });
    if (rc) return rc;
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
}

int mmpc_nlp_hess_batch(mmpc_handle* h, int64_t B, const double* V, const double* u_prev, const double* traj,
                        const double* weights, int64_t weights_stride, double lam_f, const double* lam_g,
                        double* hess_blocks, void* stream) {
    if (!h || B < 0) return fail(MMPC_ERR_INVALID_ARG, "null handle or B < 0");
    if (B == 0) return MMPC_OK;
    if (!V || !u_prev || !traj || !weights || !hess_blocks) return fail(MMPC_ERR_INVALID_ARG, "null pointer");
    const mmpc_model_info& mi = h->info;
    if (weights_stride != 0 && weights_stride < mi.num_x + 2 * mi.num_u)
        return fail(MMPC_ERR_INVALID_ARG, "weights_stride must be 0 or >= nx+2nu");
    const int64_t n = B * mi.num_shooting_nodes;
    if (n > 0x7fffffffLL * 256) return fail(MMPC_ERR_INVALID_ARG, "B*N too large");
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    rc = with_model(mi.model_id, [&](auto* m) {
        using M = std::remove_pointer_t<decltype(m)>;
        if (!HasHess<M>::value && !mi.is_linear)
            return fail(MMPC_ERR_UNSUPPORTED, "nlp_hess: the model has no second derivatives");
        nlp_hess_kernel<M><<<grid1d(n, 256), 256, 0, reinterpret_cast<hipStream_t>(stream)>>>(
            B, mi.num_shooting_nodes, mi.step_size, mi.is_linear, V, u_prev, traj, weights, weights_stride, lam_f,
            lam_g, hess_blocks);
        return static_cast<int>(MMPC_OK);
    });
    if (rc) return rc;
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
}

int mmpc_synth_batch(mmpc_handle* h, uint64_t seed, int64_t first_index, int64_t B, double* x0, double* u_prev,
                     double* traj, void* stream) {
    if (!h) return fail(MMPC_ERR_INVALID_ARG, "null handle");
    if (B < 0 || first_index < 0) return fail(MMPC_ERR_INVALID_ARG, "negative B / first_index");
    if (B == 0) return MMPC_OK;
    if (!x0 || !u_prev || !traj) return fail(MMPC_ERR_INVALID_ARG, "null output pointer");
    if (h->info.model_id == MMPC_MODEL_USER)
        return fail(MMPC_ERR_UNSUPPORTED, "no synthetic-instance recipe for generated models");
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    if (g.err) return fail(MMPC_ERR_NO_DEVICE, "cannot select device");
    if (h->info.model_id == MMPC_MODEL_EXO_ARM)
        synth_exo_kernel<<<synth_blocks(B, h->info.num_shooting_nodes), kSynthThreads, 0,
                           reinterpret_cast<hipStream_t>(stream)>>>(
            seed, first_index, B, h->info.num_shooting_nodes, h->info.step_size, x0, u_prev, traj);
    else
        synth_two_link_kernel<<<synth_blocks(B, h->info.num_shooting_nodes), kSynthThreads, 0,
                                reinterpret_cast<hipStream_t>(stream)>>>(
            seed, first_index, B, h->info.num_shooting_nodes, h->info.step_size, x0, u_prev, traj);
    MMPC_HIP(hipGetLastError());
    return MMPC_OK;
}

// ---------------------------------------------------------------- multi-device (one process, G devices)
int mmpc_shard(int64_t B, int32_t n, int32_t i, int64_t* first, int64_t* count) {
    if (B < 0 || n < 1 || i < 0 || i >= n || !first || !count) return fail(MMPC_ERR_INVALID_ARG, "bad shard arguments");
    if (B > (int64_t(1) << 40)) return fail(MMPC_ERR_INVALID_ARG, "B too large");
    const int64_t lo = (static_cast<int64_t>(i) * B) / n, hi = (static_cast<int64_t>(i + 1) * B) / n;
    *first = lo;
    *count = hi - lo;
    return MMPC_OK;
}

}  // extern "C"

namespace {
// RCCL entry points, resolved from librccl at the first RCCL call (no link-time dependency of libmmpc.so on it)
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclBroadcast) broadcast = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    decltype(&ncclGetVersion) get_version = nullptr;
};
const RcclApi* rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (a.lib) break;
        }
        if (!a.lib) return a;
        bool ok = true;
        auto sym = [&](auto& fn, const char* n) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(a.lib, n));
            ok &= fn != nullptr;
        };
        sym(a.comm_init_all, "ncclCommInitAll");
        sym(a.comm_destroy, "ncclCommDestroy");
        sym(a.group_start, "ncclGroupStart");
        sym(a.group_end, "ncclGroupEnd");
        sym(a.send, "ncclSend");
        sym(a.recv, "ncclRecv");
        sym(a.broadcast, "ncclBroadcast");
        sym(a.error_string, "ncclGetErrorString");
        sym(a.get_version, "ncclGetVersion");
        if (!ok) a.lib = nullptr;
        return a;
    }();
    return api.lib ? &api : nullptr;
}
}  // namespace

struct mmpc_multi {
    std::vector<mmpc_handle*> h;  // one handle (own stream, workspace, staging) per listed device
    std::vector<int32_t> dev;
    std::mutex mu;                // one multi-device solve at a time
    // RCCL path (mmpc_multi_solve_batch_rccl): one communicator and stream per device, grown-only shard buffers
    std::vector<ncclComm_t> comm;
    std::vector<hipStream_t> st;
    std::vector<char*> buf;
    std::vector<size_t> buf_bytes;
};

extern "C" {

int mmpc_multi_create(const char* model_json_path, const mmpc_opts* opts, const int32_t* devices, int32_t n_devices,
                      mmpc_multi** out) {
    if (!model_json_path || !devices || n_devices < 1 || n_devices > 1024 || !out)
        return fail(MMPC_ERR_INVALID_ARG, "bad multi-device arguments");
    *out = nullptr;
    std::unique_ptr<mmpc_multi> m(new mmpc_multi());
    mmpc_opts o;
    mmpc_default_opts(&o);
    if (opts) o = *opts;
    for (int32_t g = 0; g < n_devices; ++g) {
        if (devices[g] < 0) {
            for (mmpc_handle* x : m->h) mmpc_destroy(x);
            return fail(MMPC_ERR_INVALID_ARG, "device ordinals must be >= 0");
        }
        o.device = devices[g];
        mmpc_handle* h = nullptr;
        const int rc = mmpc_create(model_json_path, &o, &h);
        if (rc) {
            for (mmpc_handle* x : m->h) mmpc_destroy(x);
            return rc;
        }
        m->h.push_back(h);
        m->dev.push_back(devices[g]);
    }
    *out = m.release();
    return MMPC_OK;
}

int mmpc_multi_destroy(mmpc_multi* m) {
    if (!m) return MMPC_OK;
    if (const RcclApi* R = rccl_api())
        for (ncclComm_t c : m->comm)
            if (c) R->comm_destroy(c);
    for (size_t g = 0; g < m->st.size(); ++g) {
        DeviceGuard dg(m->dev[g]);
        if (m->st[g]) (void)hipStreamDestroy(m->st[g]);
        if (m->buf[g]) (void)hipFree(m->buf[g]);
    }
    for (mmpc_handle* h : m->h) mmpc_destroy(h);
    delete m;
    return MMPC_OK;
}

int mmpc_multi_num_devices(const mmpc_multi* m, int32_t* n) {
    if (!m || !n) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *n = static_cast<int32_t>(m->h.size());
    return MMPC_OK;
}

int mmpc_multi_handle(mmpc_multi* m, int32_t g, mmpc_handle** h) {
    if (!m || !h || g < 0 || g >= static_cast<int32_t>(m->h.size())) return fail(MMPC_ERR_INVALID_ARG, "bad device index");
    *h = m->h[static_cast<size_t>(g)];
    return MMPC_OK;
}

int mmpc_multi_solve_batch_host(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev, const double* traj,
                                const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                                double* V_inout, int32_t* status, int32_t* iters, double* kkt_res) {
    return mmpc_multi_solve_batch_host_bounds(m, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, 0, V_inout,
                                              status, iters, kkt_res);
}

int mmpc_multi_solve_batch_host_bounds(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                       const double* traj, const double* weights, int64_t weights_stride,
                                       const double* u_lb, const double* u_ub, int64_t bounds_stride, double* V_inout,
                                       int32_t* status, int32_t* iters, double* kkt_res) {
    return mmpc_multi_solve_batch_host_pinned(m, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub,
                                              bounds_stride, nullptr, 0, V_inout, status, iters, kkt_res);
}

int mmpc_multi_solve_batch_host_pinned(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                       const double* traj, const double* weights, int64_t weights_stride,
                                       const double* u_lb, const double* u_ub, int64_t bounds_stride,
                                       const double* u_pin, int32_t n_pin, double* V_inout, int32_t* status,
                                       int32_t* iters, double* kkt_res) {
    const SolveArgs a{B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, u_pin, n_pin, V_inout,
                      status, iters, kkt_res};
    // before any shard starts
    if (int rc = check_solve_args(m ? &m->h[0]->info : nullptr, a, "null multi-device handle")) return rc;
    if (B == 0) return MMPC_OK;
    std::lock_guard<std::mutex> lk(m->mu);
    const mmpc_model_info& mi = m->h[0]->info;
    const int64_t nx = mi.num_x, nu = mi.num_u, N = mi.num_shooting_nodes, NV = mi.num_v;
    const int32_t G = static_cast<int32_t>(m->h.size());
    std::vector<int> rcs(static_cast<size_t>(G), MMPC_OK);
    std::vector<std::string> errs(static_cast<size_t>(G));
    // each device solves its contiguous shard of the host arrays on its own thread (H2D, solve, D2H on the
    // handle's stream); shards are disjoint, so the results land in place without any assembly copy
    auto work = [&](int32_t g) {
        int64_t first = 0, count = 0;
        mmpc_shard(B, G, g, &first, &count);
        if (count == 0) return;
        // per-instance bounds: the shard's rows start at first * bounds_stride (stride 0: the shared row)
        // the pins of the shard: rows from first * n_pin * nu on
        const int rc = mmpc_solve_batch_host_pinned(
            m->h[static_cast<size_t>(g)], count, x0 + first * nx, u_prev + first * nu, traj + first * N * nx,
            weights_stride ? weights + first * weights_stride : weights, weights_stride,
            u_lb ? u_lb + first * bounds_stride : nullptr, u_ub ? u_ub + first * bounds_stride : nullptr, bounds_stride,
            n_pin > 0 ? u_pin + first * n_pin * nu : nullptr, n_pin, V_inout + first * NV,
            status ? status + first : nullptr, iters ? iters + first : nullptr,
            kkt_res ? kkt_res + first : nullptr);
        rcs[static_cast<size_t>(g)] = rc;
        if (rc) errs[static_cast<size_t>(g)] = g_last_error;   // thread-local: carried back to the caller
    };
    if (G == 1) {
        work(0);
    } else {
        std::vector<std::thread> th;
        th.reserve(static_cast<size_t>(G));
        for (int32_t g = 0; g < G; ++g) th.emplace_back(work, g);
        for (std::thread& t : th) t.join();
    }
    for (int32_t g = 0; g < G; ++g)
        if (rcs[static_cast<size_t>(g)])
            return fail(rcs[static_cast<size_t>(g)], "device " + std::to_string(m->dev[static_cast<size_t>(g)]) + ": " +
                                                         errs[static_cast<size_t>(g)]);
    return MMPC_OK;
}

int mmpc_rccl_version(int32_t* version) {
    if (!version) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *version = 0;
    const RcclApi* R = rccl_api();
    if (!R) return fail(MMPC_ERR_UNSUPPORTED, "librccl not loadable");
    int v = 0;
    if (R->get_version(&v) != ncclSuccess) return fail(MMPC_ERR_UNSUPPORTED, "ncclGetVersion failed");
    *version = v;
    return MMPC_OK;
}

int mmpc_multi_solve_batch_rccl(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev, const double* traj,
                                const double* weights, int64_t weights_stride, const double* u_lb, const double* u_ub,
                                double* V_inout, int32_t* status, int32_t* iters, double* kkt_res, void* stream) {
    return mmpc_multi_solve_batch_rccl_bounds(m, B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, 0, V_inout,
                                              status, iters, kkt_res, stream);
}

int mmpc_multi_solve_batch_rccl_bounds(mmpc_multi* m, int64_t B, const double* x0, const double* u_prev,
                                       const double* traj, const double* weights, int64_t weights_stride,
                                       const double* u_lb, const double* u_ub, int64_t bounds_stride, double* V_inout,
                                       int32_t* status, int32_t* iters, double* kkt_res, void* stream) {
    const SolveArgs a{B, x0, u_prev, traj, weights, weights_stride, u_lb, u_ub, bounds_stride, nullptr, 0, V_inout,
                      status, iters, kkt_res, nullptr, reinterpret_cast<hipStream_t>(stream)};
    // checked before anything is sent: the scatter reads rows of bounds_stride and of weights_stride
    if (int rc = check_solve_args(m ? &m->h[0]->info : nullptr, a, "null multi-device handle")) return rc;
    if (B == 0) return MMPC_OK;
    if ((u_lb == nullptr) != (u_ub == nullptr)) return fail(MMPC_ERR_INVALID_ARG, "u_lb and u_ub go together");
    std::lock_guard<std::mutex> lk(m->mu);
    const mmpc_model_info& mi = m->h[0]->info;
    const int64_t nx = mi.num_x, nu = mi.num_u, N = mi.num_shooting_nodes, NV = mi.num_v, nw = nx + 2 * nu;
    const int32_t G = static_cast<int32_t>(m->h.size());
    for (int32_t a = 0; a < G; ++a)
        for (int32_t b = 0; b < a; ++b)
            if (m->dev[a] == m->dev[b])
                return fail(MMPC_ERR_UNSUPPORTED, "RCCL needs distinct devices (device " + std::to_string(m->dev[a]) +
                                                      " listed twice); mmpc_multi_solve_batch_host shares a device");
    const RcclApi* R = rccl_api();
    if (!R) return fail(MMPC_ERR_UNSUPPORTED, "librccl not loadable");
    auto nccl = [&](ncclResult_t r, const char* what) {
        return r == ncclSuccess ? MMPC_OK : fail(MMPC_ERR_HIP, std::string(what) + ": " + R->error_string(r));
    };
    if (m->comm.empty()) {   // one communicator per device, in the listed order (rank g = device g of the handle)
        std::vector<ncclComm_t> comm(static_cast<size_t>(G), nullptr);
        std::vector<int> devs(m->dev.begin(), m->dev.end());
        if (int rc = nccl(R->comm_init_all(comm.data(), G, devs.data()), "ncclCommInitAll")) return rc;
        m->comm = comm;
        m->st.assign(static_cast<size_t>(G), nullptr);
        m->buf.assign(static_cast<size_t>(G), nullptr);
        m->buf_bytes.assign(static_cast<size_t>(G), 0);
        for (int32_t g = 0; g < G; ++g) {
            DeviceGuard dg(m->dev[g]);
            MMPC_HIP(hipStreamCreateWithFlags(&m->st[g], hipStreamNonBlocking));
        }
    }
    const bool shared_w = weights_stride == 0;
    const int64_t wst = shared_w ? 0 : weights_stride;
    struct Shard {
        int64_t first = 0, count = 0;
        double *x0, *up, *tr, *w, *lb, *ub, *V, *kkt;
        int32_t *st, *it;
    };
    std::vector<Shard> sh(static_cast<size_t>(G));
    // bound doubles of a shard of c instances: the shared row, or c rows of which the last ends after its nu entries
    const int64_t bst = bounds_stride;
    auto nbs = [&](int64_t c) { return bst ? (c > 0 ? (c - 1) * bst + nu : 0) : nu; };
    for (int32_t g = 0; g < G; ++g) {   // shard buffers on device g (grown only)
        Shard& s = sh[static_cast<size_t>(g)];
        mmpc_shard(B, G, g, &s.first, &s.count);
        const int64_t c = s.count;
        const int64_t nd = c * (nx + nu + N * nx + NV + 1) + (shared_w ? nw : c * wst) + 2 * nbs(c);
        const size_t bytes = static_cast<size_t>(nd) * sizeof(double) + static_cast<size_t>(2 * c) * sizeof(int32_t) + 64;
        DeviceGuard dg(m->dev[g]);
        if (bytes > m->buf_bytes[g]) {
            if (m->buf[g]) MMPC_HIP(hipFree(m->buf[g]));
            m->buf[g] = nullptr;
            m->buf_bytes[g] = 0;
            MMPC_HIP(hipMalloc(&m->buf[g], bytes));
            m->buf_bytes[g] = bytes;
        }
        double* p = reinterpret_cast<double*>(m->buf[g]);
        s.x0 = p; p += c * nx;
        s.up = p; p += c * nu;
        s.tr = p; p += c * N * nx;
        s.V = p; p += c * NV;
        s.kkt = p; p += c;
        s.w = p; p += shared_w ? nw : c * wst;
        s.lb = p; p += nbs(c);
        s.ub = p; p += nbs(c);
        s.st = reinterpret_cast<int32_t*>(p);
        s.it = s.st + c;
    }
    // the caller's inputs on the first device are complete before RCCL reads them: the first device's stream waits
    // for the caller's stream (no device-wide synchronisation); at the end the caller's stream waits for the results
    hipStream_t caller = reinterpret_cast<hipStream_t>(stream);
    if (caller) {   // the bridges below record on and wait with the caller's stream from the first device
        hipDevice_t sd = -1;
        MMPC_HIP(hipStreamGetDevice(caller, &sd));
        if (sd != m->dev[0])
            return fail(MMPC_ERR_INVALID_ARG, "stream belongs to device " + std::to_string(sd) +
                                                  ", not to the multi handle's first device " + std::to_string(m->dev[0]));
    }
    {
        DeviceGuard dg(m->dev[0]);
        hipEvent_t ev;
        MMPC_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, caller);
        if (e == hipSuccess) e = hipStreamWaitEvent(m->st[0], ev, 0);
        (void)hipEventDestroy(ev);
        MMPC_HIP(e);
    }
    // every stream of the call drained before an error after the first enqueue is returned (no RCCL operation or
    // solve of this call is still running when the caller sees the error)
    auto drain = [&](int rc) {
        for (int32_t g = 0; g < G; ++g) {
            DeviceGuard dg(m->dev[g]);
            (void)hipStreamSynchronize(m->st[static_cast<size_t>(g)]);
        }
        return rc;
    };
    // a group is always closed (ncclGroupEnd) even when an operation inside it failed; the first failure is reported
    int grp_rc = MMPC_OK;
    auto op = [&](ncclResult_t r, const char* what, int32_t g) {
        if (r != ncclSuccess && grp_rc == MMPC_OK)
            grp_rc = fail(MMPC_ERR_HIP, std::string(what) + " (shard " + std::to_string(g) + "): " + R->error_string(r));
    };
    // scatter: shard g of every input from rank 0 to rank g (rank 0 included: its shard goes through RCCL as well),
    // shared weights and the bounds by broadcast.  Per-instance weights: the last row of a shard is sent up to its
    // nx + 2 nu entries, so a caller's buffer of (B - 1) weights_stride + nx + 2 nu doubles is never over-read.
    const ncclDataType_t f64 = ncclFloat64, i32 = ncclInt32;
    if (int rc = nccl(R->group_start(), "ncclGroupStart")) return drain(rc);
    for (int32_t g = 0; g < G; ++g) {
        const Shard& s = sh[static_cast<size_t>(g)];
        ncclComm_t c0 = m->comm[0], cg = m->comm[static_cast<size_t>(g)];
        hipStream_t s0 = m->st[0], sg = m->st[static_cast<size_t>(g)];
        if (s.count > 0) {
            const size_t c = static_cast<size_t>(s.count);
            op(R->send(x0 + s.first * nx, c * nx, f64, g, c0, s0), "ncclSend x0", g);
            op(R->recv(s.x0, c * nx, f64, 0, cg, sg), "ncclRecv x0", g);
            op(R->send(u_prev + s.first * nu, c * nu, f64, g, c0, s0), "ncclSend u_prev", g);
            op(R->recv(s.up, c * nu, f64, 0, cg, sg), "ncclRecv u_prev", g);
            op(R->send(traj + s.first * N * nx, c * N * nx, f64, g, c0, s0), "ncclSend traj", g);
            op(R->recv(s.tr, c * N * nx, f64, 0, cg, sg), "ncclRecv traj", g);
            op(R->send(V_inout + s.first * NV, c * NV, f64, g, c0, s0), "ncclSend V", g);
            op(R->recv(s.V, c * NV, f64, 0, cg, sg), "ncclRecv V", g);
            if (!shared_w) {
                const size_t nwc = (c - 1) * static_cast<size_t>(wst) + static_cast<size_t>(nw);
                op(R->send(weights + s.first * wst, nwc, f64, g, c0, s0), "ncclSend weights", g);
                op(R->recv(s.w, nwc, f64, 0, cg, sg), "ncclRecv weights", g);
            }
            if (u_lb && bst) {   // per-instance bounds: the shard's rows, the last one up to its nu entries
                const size_t nbc = static_cast<size_t>(nbs(s.count));
                op(R->send(u_lb + s.first * bst, nbc, f64, g, c0, s0), "ncclSend u_lb", g);
                op(R->recv(s.lb, nbc, f64, 0, cg, sg), "ncclRecv u_lb", g);
                op(R->send(u_ub + s.first * bst, nbc, f64, g, c0, s0), "ncclSend u_ub", g);
                op(R->recv(s.ub, nbc, f64, 0, cg, sg), "ncclRecv u_ub", g);
            }
        }
        // collectives run on every rank, shards of count 0 included (the broadcast lands in its unused buffer)
        if (shared_w) op(R->broadcast(weights, s.w, static_cast<size_t>(nw), f64, 0, cg, sg), "ncclBroadcast weights", g);
        if (u_lb && !bst) {
            op(R->broadcast(u_lb, s.lb, static_cast<size_t>(nu), f64, 0, cg, sg), "ncclBroadcast u_lb", g);
            op(R->broadcast(u_ub, s.ub, static_cast<size_t>(nu), f64, 0, cg, sg), "ncclBroadcast u_ub", g);
        }
    }
    if (int rc = nccl(R->group_end(), "ncclGroupEnd (scatter)")) return drain(rc);
    if (grp_rc) return drain(grp_rc);
    // solve: every device its shard, on its stream after its receives
    for (int32_t g = 0; g < G; ++g) {
        const Shard& s = sh[static_cast<size_t>(g)];
        if (s.count == 0) continue;
        const int rc = mmpc_solve_batch_bounds(m->h[static_cast<size_t>(g)], s.count, s.x0, s.up, s.tr, s.w, wst,
                                               u_lb ? s.lb : nullptr, u_lb ? s.ub : nullptr, bst, s.V, s.st, s.it,
                                               s.kkt, nullptr, m->st[static_cast<size_t>(g)]);
        if (rc) {
            const std::string err = "device " + std::to_string(m->dev[static_cast<size_t>(g)]) + ": " + g_last_error;
            return drain(fail(rc, err));
        }
    }
    // gather: V, status, iters, kkt_res of shard g back to rank 0 at the shard's offset
    if (int rc = nccl(R->group_start(), "ncclGroupStart")) return drain(rc);
    for (int32_t g = 0; g < G; ++g) {
        const Shard& s = sh[static_cast<size_t>(g)];
        if (s.count == 0) continue;
        const size_t c = static_cast<size_t>(s.count);
        ncclComm_t c0 = m->comm[0], cg = m->comm[static_cast<size_t>(g)];
        hipStream_t s0 = m->st[0], sg = m->st[static_cast<size_t>(g)];
        op(R->send(s.V, c * NV, f64, 0, cg, sg), "ncclSend V (gather)", g);
        op(R->recv(V_inout + s.first * NV, c * NV, f64, g, c0, s0), "ncclRecv V (gather)", g);
        if (status) {
            op(R->send(s.st, c, i32, 0, cg, sg), "ncclSend status", g);
            op(R->recv(status + s.first, c, i32, g, c0, s0), "ncclRecv status", g);
        }
        if (iters) {
            op(R->send(s.it, c, i32, 0, cg, sg), "ncclSend iters", g);
            op(R->recv(iters + s.first, c, i32, g, c0, s0), "ncclRecv iters", g);
        }
        if (kkt_res) {
            op(R->send(s.kkt, c, f64, 0, cg, sg), "ncclSend kkt", g);
            op(R->recv(kkt_res + s.first, c, f64, g, c0, s0), "ncclRecv kkt", g);
        }
    }
    if (int rc = nccl(R->group_end(), "ncclGroupEnd (gather)")) return drain(rc);
    if (grp_rc) return drain(grp_rc);
    {   // later work on the caller's stream sees the gathered results
        DeviceGuard dg(m->dev[0]);
        hipEvent_t ev;
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return drain(fail(MMPC_ERR_HIP, std::string("event: ") + hipGetErrorString(e)));
        e = hipEventRecord(ev, m->st[0]);
        if (e == hipSuccess) e = hipStreamWaitEvent(caller, ev, 0);
        (void)hipEventDestroy(ev);
        if (e != hipSuccess) return drain(fail(MMPC_ERR_HIP, std::string("event: ") + hipGetErrorString(e)));
    }
    for (int32_t g = 0; g < G; ++g) {
        DeviceGuard dg(m->dev[g]);
        MMPC_HIP(hipStreamSynchronize(m->st[static_cast<size_t>(g)]));
    }
    return MMPC_OK;
}

const char* mmpc_status_string(int32_t s) {
    switch (s) {
        case MMPC_STATUS_CONVERGED: return "converged";
        case MMPC_STATUS_MAX_ITER: return "max_iter";
        case MMPC_STATUS_LINESEARCH_FAILED: return "linesearch_failed";
        case MMPC_STATUS_NONFINITE: return "nonfinite";
        case MMPC_STATUS_FACTORIZATION_FAILED: return "factorization_failed";
        case MMPC_STATUS_BOUNDS_VIOLATED: return "bounds_violated";
        default: return "unknown";
    }
}

const char* mmpc_last_error(void) { return g_last_error.c_str(); }

// Internal diagnostic: per-phase s_memtime cycle totals of the SQP kernel (all zero unless the library
// was built with -DMMPC_PHASE_TIMING, i.e. lib/libmmpc_timing.so).  out[15] = number of waves.
// sums, except slots 10-12 (latest end, ~earliest start, longest wave: sqp_wave.h MMPC_PHASE_FLUSH), which are maxima;
// the per-wave slots 16.. are written by one unit only per launch (the others hold zeros after a reset)
static void merge_phase_tables(unsigned long long* out, const unsigned long long* t, int n) {
    for (int i = 0; i < n; ++i) out[i] = (i >= 10 && i <= 12) ? std::max(out[i], t[i]) : out[i] + t[i];
}
// the first n slots of the merged tables of every translation unit (kPhaseTableSlots: kPhaseSlots in the timing build,
// 16 otherwise)
int mmpc_debug_phase_table(unsigned long long* out, int n, int reset) {
    if (!out || n < 16 || n > kPhaseTableSlots)
        return fail(MMPC_ERR_INVALID_ARG, "null or n out of 16 .. the table's size (16 outside the timing build)");
    MMPC_HIP(phase_table_read(out, n, reset != 0));   // this unit's table
    std::vector<unsigned long long> t(static_cast<size_t>(n));
    MMPC_HIP(lane_phase_cycles(t.data(), n, reset != 0));   // the lane kernels' unit (lane_launch.h)
    merge_phase_tables(out, t.data(), n);
#if MMPC_BUILTIN_MODELS
    MMPC_HIP(group_two_link_phase_cycles(t.data(), n, reset != 0));   // the 2-link group kernels' units (group_launch.h)
    merge_phase_tables(out, t.data(), n);
    MMPC_HIP(group_two_link_bounded_phase_cycles(t.data(), n, reset != 0));
    merge_phase_tables(out, t.data(), n);
#endif
    return MMPC_OK;
}
int mmpc_debug_phase_cycles(unsigned long long* out16, int reset) { return mmpc_debug_phase_table(out16, 16, reset); }

// Internal diagnostic (not part of include/mmpc.h): the handle's Riccati workspace (device pointer and size), e.g. to
// read the gains [K_k | kff_k] a solve left there (tools/xb_diag.py)
int mmpc_debug_workspace(mmpc_handle* h, void** ptr, uint64_t* bytes) {
    if (!h || !ptr || !bytes) return fail(MMPC_ERR_INVALID_ARG, "null argument");
    *ptr = h->ws;
    *bytes = h->ws_bytes;
    return MMPC_OK;
}

// Internal diagnostic (not part of include/mmpc.h): as mmpc_solve_batch, plus a per-iteration trace
// [B][max_iter+1][8] = (||2g||, ||c||, alpha, dphi, phi0, mu, ||du||, accepted).  Device pointers.
int mmpc_debug_solve_trace(mmpc_handle* h, int64_t B, const double* x0, const double* u_prev, const double* traj,
                           const double* weights, int64_t weights_stride, double* V_inout, int32_t* status,
                           int32_t* iters, double* kkt_res, double* trace, void* stream) {
    if (!h || B < 0 || !trace) return fail(MMPC_ERR_INVALID_ARG, "bad argument");
    const SolveArgs a{B, x0, u_prev, traj, weights, weights_stride, nullptr, nullptr, 0, nullptr, 0, V_inout, status,
                      iters, kkt_res, nullptr, reinterpret_cast<hipStream_t>(stream), trace};
    if (int rc = check_solve_args(&h->info, a)) return rc;
    if (B == 0) return MMPC_OK;
    int dev;
    int rc = resolve_device(h, &dev);
    if (rc) return rc;
    DeviceGuard g(dev);
    return launch_solve(h, a);
}

}  // extern "C"
