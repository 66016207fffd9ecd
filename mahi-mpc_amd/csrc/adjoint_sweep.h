// adjoint_sweep.h -- reverse-mode product of the solve: (d V* / d theta)^T V_bar for theta = x0, u_prev, traj and the
// weights, from one backward Riccati sweep with a vector part and one forward sweep at V
// (mmpc_solve_vjp_batch, include/mmpc.h).
//
// With the stage quantities of gain_sweep.h (A_k, B_k, e_k, nu_k, lam_k, S_k (+ W_k), M_uu, M_us, M_ss, G_k, the held
// mask) the direction a solves  min 1/2 a^T L_VV a - V_bar^T a  over the linearised dynamics from a_{x,0} = 0, a = 0 on
// held controls.  On s = (dx_k, dv = du_{k-1}), P_N = 0, p_N = (V_bar_{x_N}; 0), backward over k = N-1..0:
//   q = C_k^T p_{k+1} + (V_bar_{x_k}; V_bar_{u_k}),  q_u of a held control 0,
//   kff_k = M_uu^-1 q_u,  p_k = (q_x; 0) + G_k^T q_u,  P_k = M_ss + M_su G_k;
// forward from s_0 = 0:  a_{u,k} = G_k s_k + kff_k,  s_{k+1} = (A_k a_{x,k} + B_k a_{u,k}; a_{u,k}).
// Outputs: (x0_bar | u_prev_bar) = p_0;  traj_bar[k] = 2 Q o a_{x,k+1};  Q_bar = -2 sum e_k o a_{x,k+1};
// R_bar = -2 sum (u_k - u_{k-1}) o (a_{u,k} - a_{u,k-1});  Rm_bar = -2 sum u_k o a_{u,k};  adj_V = a.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "gain_sweep.h"

namespace mmpc {

struct AdjointParams : SensParams {   // the head: gain_sweep.h
    const double* V_bar;    // [B][NV]
    double* x0_bar;         // [B][nx] or null
    double* u_prev_bar;     // [B][nu] or null
    double* traj_bar;       // [B][N][nx] or null
    double* weights_bar;    // [B][nx + 2 nu] or null
    double* adj_V;          // [B][NV] or null
    int32_t* status;        // [B] or null: 0 as asked, 1 Gauss-Newton fallback, 2 failed (every output row 0)
    double* ws;             // the records; null in backward-only mode (traj_bar, weights_bar and adj_V all null)
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(AdjointParams) == 152 && offsetof(AdjointParams, V_bar) == 88, "kernel argument layout");
#pragma clang diagnostic pop

// workspace doubles per lane: the record G_k | kff_k of every stage
__host__ __device__ constexpr int64_t adjoint_rec_doubles(int nx, int nu) { return (int64_t)nu * (nx + nu + 1); }
__host__ __device__ constexpr int64_t adjoint_lane_doubles(int nx, int nu, int N) {
    return (int64_t)N * adjoint_rec_doubles(nx, nu);
}

// the XB instantiations' parameters: AdjointParams plus the sensitivity barrier's tail (gain_sweep.h); AdjointParams
// itself, and with it the other instantiations' kernel arguments, keeps its layout
struct AdjointXbParams : AdjointParams {
    XbTail xb;
};
template <bool XB>
using AdjointParamsOf = std::conditional_t<XB, AdjointXbParams, AdjointParams>;

// One lane per instance, both sweeps in one launch.  The backward sweep is gain_lane_kernel's fused stage -- one text
// for both kernels, sens_lane_stage.inc: part 1 through G_k, then q, kff and p here, then part 2 (P_k) -- and the
// prologue is that file's part 0; with a workspace it stores G_k | kff_k per stage, element i of
// lane l of workgroup g at ws[(g * doubles per lane + i) * 64 + l], so a wave's store of one element is one 512-byte
// line.  The forward sweep evaluates value and Jacobian again per stage (nothing of [A | B] is stored), reads the
// record back, writes adj_V and traj_bar per stage and keeps the nx + 2 nu weight sums in registers.  A second pass
// over both sweeps runs only for the Gauss-Newton fallback.  XB: the sensitivity barrier's terms join the backward
// stage inside the shared text (XbTail, gain_sweep.h); q, kff, p, the forward sweep and the outputs are the same text
// with and without XB, the barrier does not depend on theta.
template <class Model, bool EXACT, bool BOUNDED, bool XB = false>
__global__ __launch_bounds__(64) void adjoint_lane_kernel(const AdjointParamsOf<XB> p) {
    constexpr int NX = Model::NX, NU = Model::NU, K = NX + NU, NQ = Model::NQ, NA = NX - NQ, NP = K * (K + 1) / 2;
    constexpr int RD = NU * (K + 1);
    static_assert(!EXACT || HasHess<Model>::value, "the exact adjoint needs Model::eval_hess");
    static_assert(!XB || BOUNDED, "the XB instantiations read the control bounds");
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N;
    const double h = p.h;
    const int64_t NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    const double* v = p.V + b * NV;
    const double* vb = p.V_bar + b * NV;
    const double* w = p.weights + b * p.w_stride;
    const double* tr = p.traj + b * (int64_t)N * NX;
    const bool full = p.ws != nullptr;
    double* const rec = full ? p.ws + (int64_t)blockIdx.x * ((int64_t)N * RD * 64) + threadIdx.x : nullptr;
    double* const trb = p.traj_bar ? p.traj_bar + b * (int64_t)N * NX : nullptr;
    double* const av = p.adj_V ? p.adj_V + b * NV : nullptr;
#define MMPC_SENS_PART 0   // Q, R, Rm, lb, ub, up, fin
#include "sens_lane_stage.inc"
    bool ok = false;
    int st = 0;
    double pv[K], wb[NX + 2 * NU];   // p_k; the weight sums (Q_bar | R_bar | Rm_bar)
#pragma unroll
    for (int i = 0; i < NX + 2 * NU; ++i) wb[i] = 0.0;
    for (int pass = 0; pass < (EXACT ? 2 : 1) && !ok; ++pass) {
        const bool exact = EXACT && pass == 0;
        st = pass;
        ok = fin == 0.0;
        // ---- backward: P_k, p_k, the record ----
        double P[NP], lam[NX];
#pragma unroll
        for (int i = 0; i < NP; ++i) P[i] = 0.0;
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            lam[r] = 0.0;
            pv[r] = vb[(int64_t)N * K + r];
        }
#pragma unroll
        for (int c = 0; c < NU; ++c) pv[NX + c] = 0.0;
        for (int k = N - 1; k >= 0 && ok; --k) {
#define MMPC_SENS_PART 1   // the model, nu_k / lam, M_yy (+ W_k), the held rows, the factor of M_uu, G_k
#include "sens_lane_stage.inc"
            // q = C_k^T p_{k+1} + V_bar_{y_k}; kff_k = M_uu^-1 q_u; p_k = (q_x; 0) + G_k^T q_u
            double q[K], mq[NU], kff[NU];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double s = (j >= NX ? pv[j] : 0.0) + vb[k * K + j];
#pragma unroll
                for (int r = 0; r < NX; ++r) s += J[r][j] * pv[r];
                q[j] = s;
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                q[NX + c] = held[c] ? 0.0 : q[NX + c];
                mq[c] = -q[NX + c];
            }
            gain_solve<NU>(Muu, il, mq, kff);
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                kff[c] = held[c] ? 0.0 : kff[c];
                chk += gain_nonfinite(kff[c]);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double s = j < NX ? q[j] : 0.0;
#pragma unroll
                for (int c = 0; c < NU; ++c) s += G[c][j] * q[NX + c];
                pv[j] = s;
                chk += gain_nonfinite(s);
            }
#define MMPC_SENS_PART 2   // P_k = M_ss + M_su G_k
#include "sens_lane_stage.inc"
            ok = ok && chk == 0.0;
            if (ok && full) {
                double* const rk = rec + (int64_t)k * (RD * 64);
#pragma unroll
                for (int c = 0; c < NU; ++c) {
#pragma unroll
                    for (int j = 0; j < K; ++j) rk[(c * (K + 1) + j) * 64] = G[c][j];
                    rk[(c * (K + 1) + K) * 64] = kff[c];
                }
            }
        }
        // ---- forward: a, traj_bar, the weight sums ----
        if (ok && full) {
            double ax[NX], aup[NU], ul[NU], fbad = 0.0;   // s_k = (a_{x,k}; a_{u,k-1}); u_{k-1}
#pragma unroll
            for (int r = 0; r < NX; ++r) ax[r] = 0.0;
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                aup[c] = 0.0;
                ul[c] = up[c];
            }
#pragma unroll
            for (int i = 0; i < NX + 2 * NU; ++i) wb[i] = 0.0;
            for (int k = 0; k < N; ++k) {
                double x[NX], u[NU], xd[NX], fx[NX * NX], fu[NX * NU], au[NU], an[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) x[r] = v[k * K + r];
#pragma unroll
                for (int c = 0; c < NU; ++c) u[c] = v[k * K + NX + c];
                model_eval_jac<Model>(x, u, xd, fx, fu);
                const double* const rk = rec + (int64_t)k * (RD * 64);
#pragma unroll
                for (int c = 0; c < NU; ++c) {   // a_{u,k} = G_k s_k + kff_k (a held control: a zero row and kff 0)
                    double s = rk[(c * (K + 1) + K) * 64];
#pragma unroll
                    for (int j = 0; j < NX; ++j) s += rk[(c * (K + 1) + j) * 64] * ax[j];
#pragma unroll
                    for (int d = 0; d < NU; ++d) s += rk[(c * (K + 1) + NX + d) * 64] * aup[d];
                    au[c] = s;
                }
                if (av) {
#pragma unroll
                    for (int r = 0; r < NX; ++r) av[k * K + r] = ax[r];
#pragma unroll
                    for (int c = 0; c < NU; ++c) av[k * K + NX + c] = au[c];
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) {   // a_{x,k+1} = A_k a_{x,k} + B_k a_{u,k}
                    double s = ax[r];
#pragma unroll
                    for (int c = 0; c < NX; ++c) s += h * fx[r * NX + c] * ax[c];
#pragma unroll
                    for (int c = 0; c < NU; ++c) s += h * fu[r * NU + c] * au[c];
                    an[r] = s;
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    const double e = x[r] + h * xd[r] - tr[k * NX + r];
                    wb[r] -= 2.0 * e * an[r];
                    const double t = 2.0 * Q[r] * an[r];
                    fbad += gain_nonfinite(t);
                    if (trb) trb[k * NX + r] = t;
                    ax[r] = an[r];
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    wb[NX + c] -= 2.0 * (u[c] - ul[c]) * (au[c] - aup[c]);
                    wb[NX + NU + c] -= 2.0 * u[c] * au[c];
                    aup[c] = au[c];
                    ul[c] = u[c];
                }
            }
#pragma unroll
            for (int i = 0; i < NX + 2 * NU; ++i) fbad += gain_nonfinite(wb[i]);
            if (av) {
#pragma unroll
                for (int r = 0; r < NX; ++r) av[(int64_t)N * K + r] = ax[r];
            }
            ok = fbad == 0.0;
        }
    }
    if (!ok) {   // every output row of the instance 0
        st = 2;
#pragma unroll
        for (int j = 0; j < K; ++j) pv[j] = 0.0;
#pragma unroll
        for (int i = 0; i < NX + 2 * NU; ++i) wb[i] = 0.0;
        if (trb)
            for (int i = 0; i < N * NX; ++i) trb[i] = 0.0;
        if (av)
            for (int64_t i = 0; i < NV; ++i) av[i] = 0.0;
    }
    if (p.x0_bar) {
#pragma unroll
        for (int r = 0; r < NX; ++r) p.x0_bar[b * NX + r] = pv[r];
    }
    if (p.u_prev_bar) {
#pragma unroll
        for (int c = 0; c < NU; ++c) p.u_prev_bar[b * NU + c] = pv[NX + c];
    }
    if (p.weights_bar) {
#pragma unroll
        for (int i = 0; i < NX + 2 * NU; ++i) p.weights_bar[b * (NX + 2 * NU) + i] = wb[i];
    }
    if (p.status) p.status[b] = st;
}

}  // namespace mmpc
