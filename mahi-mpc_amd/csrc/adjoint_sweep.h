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

#include <cstdint>

#include "gain_sweep.h"

namespace mmpc {

struct AdjointParams {
    int64_t B;
    int N;
    double h;
    const double* V;        // [B][NV]
    const double* u_prev;   // [B][nu]
    const double* traj;     // [B][N][nx]
    const double* weights;  // (Q | R | Rm), row b at b * w_stride
    int64_t w_stride;
    const double* u_lb;     // BOUNDED kernels: [nu] (b_stride 0) or row b at b * b_stride; either may be null
    const double* u_ub;
    int32_t b_stride;
    int32_t n_pin;          // stages k < n_pin are held (committed controls)
    const double* V_bar;    // [B][NV]
    double* x0_bar;         // [B][nx] or null
    double* u_prev_bar;     // [B][nu] or null
    double* traj_bar;       // [B][N][nx] or null
    double* weights_bar;    // [B][nx + 2 nu] or null
    double* adj_V;          // [B][NV] or null
    int32_t* status;        // [B] or null: 0 as asked, 1 Gauss-Newton fallback, 2 failed (every output row 0)
    double* ws;             // the records; null in backward-only mode (traj_bar, weights_bar and adj_V all null)
};

// workspace doubles per lane: the record G_k | kff_k of every stage
__host__ __device__ constexpr int64_t adjoint_rec_doubles(int nx, int nu) { return (int64_t)nu * (nx + nu + 1); }
__host__ __device__ constexpr int64_t adjoint_lane_doubles(int nx, int nu, int N) {
    return (int64_t)N * adjoint_rec_doubles(nx, nu);
}

// the XB instantiations' parameters: AdjointParams plus the sensitivity barrier's tail (gain_sweep.h); AdjointParams
// itself, and with it the other instantiations' kernel arguments, stays as it is
struct AdjointXbParams : AdjointParams {
    XbTail xb;
};
template <bool XB>
using AdjointParamsOf = std::conditional_t<XB, AdjointXbParams, AdjointParams>;

// One lane per instance, both sweeps in one launch.  The backward sweep is gain_lane_kernel's fused stage (restated
// here, that kernel is left as it is) plus q, kff and p; with a workspace it stores G_k | kff_k per stage, element i of
// lane l of workgroup g at ws[(g * doubles per lane + i) * 64 + l], so a wave's store of one element is one 512-byte
// line.  The forward sweep evaluates value and Jacobian again per stage (nothing of [A | B] is stored), reads the
// record back, writes adj_V and traj_bar per stage and keeps the nx + 2 nu weight sums in registers.  A second pass
// over both sweeps runs only for the Gauss-Newton fallback.  XB: the sensitivity barrier's terms join the backward
// stage as in gain_lane_kernel (XbTail, gain_sweep.h); q, kff, p, the forward sweep and the outputs are the same text,
// the barrier does not depend on theta.
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
    double Q[NX], R[NU], Rm[NU], lb[NU], ub[NU], up[NU];
    // inputs the backward sweep never multiplies into a pivot: x_N, u_prev
    double fin = 0.0;
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        Q[r] = w[r];
        fin += gain_nonfinite(v[(int64_t)N * K + r]) + gain_nonfinite(Q[r]);
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        R[c] = w[NX + c];
        Rm[c] = w[NX + NU + c];
        up[c] = p.u_prev[b * NU + c];
        fin += gain_nonfinite(up[c]) + gain_nonfinite(R[c]) + gain_nonfinite(Rm[c]);
        lb[c] = (BOUNDED && p.u_lb) ? p.u_lb[b * p.b_stride + c] : -INFINITY;
        ub[c] = (BOUNDED && p.u_ub) ? p.u_ub[b * p.b_stride + c] : INFINITY;
    }
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
            double x[NX], u[NU], xd[NX], fx[NX * NX], fu[NX * NU];
#pragma unroll
            for (int r = 0; r < NX; ++r) x[r] = v[k * K + r];
#pragma unroll
            for (int c = 0; c < NU; ++c) u[c] = v[k * K + NX + c];
            model_eval_jac<Model>(x, u, xd, fx, fu);
            double J[NX][K], nuk[NX], chk = 0.0;   // J = [A_k | B_k]
            [[maybe_unused]] double Du[NU];
            if constexpr (XB) {   // lam_k gets beta(x_{k+1}), P_{k+1} gets D(x_{k+1}) in place; D(u_k) for M_uu
                bool in = true;
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    double be, D;
                    in = xb_terms(v[(k + 1) * K + r], p.xb.x_lb[r], p.xb.x_ub[r], p.xb.mu, p.xb.cap, be, D) && in;
                    lam[r] += be;
                    P[gain_sym(r, r, K)] += D;
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    double be;
                    Du[c] = 0.0;
                    if (k >= p.n_pin) in = xb_terms(u[c], lb[c], ub[c], p.xb.mu, p.xb.cap, be, Du[c]) && in;
                }
                chk += in ? 0.0 : NAN;
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) {
#pragma unroll
                for (int c = 0; c < NX; ++c) J[r][c] = (r == c ? 1.0 : 0.0) + h * fx[r * NX + c];
#pragma unroll
                for (int c = 0; c < NU; ++c) J[r][NX + c] = h * fu[r * NU + c];
                const double e = x[r] + h * xd[r] - tr[k * NX + r];
                nuk[r] = 2.0 * Q[r] * e + lam[r];
                chk += gain_nonfinite(nuk[r]);   // a non-finite target fails the instance under either Hessian
            }
#pragma unroll
            for (int c = 0; c < NX; ++c) {   // lam_{k-1} = A_k^T nu_k
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < NX; ++r) s += J[r][c] * nuk[r];
                lam[c] = s;
            }
            // M_yy = C^T P C + S_k, column by column of P C
            double M[NP];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double t[K];
#pragma unroll
                for (int a = 0; a < K; ++a) {
                    double s = j >= NX ? P[gain_sym(a, j, K)] : 0.0;
#pragma unroll
                    for (int q = 0; q < NX; ++q) s += P[gain_sym(a, q, K)] * J[q][j];
                    t[a] = s;
                }
#pragma unroll
                for (int i = 0; i <= j; ++i) {
                    double s = i >= NX ? t[i] : 0.0;
#pragma unroll
                    for (int a = 0; a < NX; ++a) s += J[a][i] * t[a];
#pragma unroll
                    for (int r = 0; r < NX; ++r) s += 2.0 * Q[r] * J[r][i] * J[r][j];
                    M[gain_sym(i, j, K)] = s;
                }
            }
            if constexpr (EXACT) {
                if (exact) {
                    double la[NA], W[K * K];
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) la[s2] = h * nuk[NQ + s2];
                    Model::eval_hess(x, u, la, W);
#pragma unroll
                    for (int i = 0; i < K; ++i)
#pragma unroll
                        for (int j = i; j < K; ++j) M[gain_sym(i, j, K)] += W[i * K + j];
                }
            }
            double Muu[NU][NU], Mus[NU][K], il[NU];
            bool held[NU];
#pragma unroll
            for (int c = 0; c < NU; ++c) held[c] = gain_held<BOUNDED && !XB>(k, p.n_pin, u[c], lb[c], ub[c]);
#pragma unroll
            for (int c = 0; c < NU; ++c) {
#pragma unroll
                for (int d = 0; d < NU; ++d) {
                    double m = M[gain_sym(NX + c, NX + d, K)] + (c == d ? 2.0 * R[c] + 2.0 * Rm[c] : 0.0);
                    if constexpr (XB) m += c == d ? Du[c] : 0.0;
                    Muu[c][d] = (held[c] || held[d]) ? (c == d ? 1.0 : 0.0) : m;
                }
#pragma unroll
                for (int j = 0; j < NX; ++j) Mus[c][j] = held[c] ? 0.0 : M[gain_sym(j, NX + c, K)];
#pragma unroll
                for (int d = 0; d < NU; ++d) Mus[c][NX + d] = (c == d && !held[c]) ? -2.0 * R[c] : 0.0;
            }
            ok = gain_chol<NU>(Muu, il);
            double G[NU][K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double m[NU], g[NU];
#pragma unroll
                for (int c = 0; c < NU; ++c) m[c] = Mus[c][j];
                gain_solve<NU>(Muu, il, m, g);
#pragma unroll
                for (int c = 0; c < NU; ++c) G[c][j] = held[c] ? 0.0 : g[c];
            }
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
            // P_k = M_ss + M_su G_k
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = i; j < K; ++j) {
                    double s = (j < NX) ? M[gain_sym(i, j, K)] : ((i == j) ? 2.0 * R[i - (i >= NX ? NX : 0)] : 0.0);
#pragma unroll
                    for (int c = 0; c < NU; ++c) s += Mus[c][i] * G[c][j];
                    P[gain_sym(i, j, K)] = s;
                    chk += gain_nonfinite(s);
                }
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
