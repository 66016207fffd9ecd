// tangent_sweep.h -- forward-mode product of the solve: dV = (d V* / d theta) d theta for theta = x0, u_prev, traj and
// the weights, from one backward Riccati sweep with a vector part and one forward sweep at V
// (mmpc_solve_jvp_batch, include/mmpc.h).
//
// The KKT matrix of the solution map is symmetric, so the sweeps are those of adjoint_sweep.h with another right-hand
// side and a non-zero start.  With the stage quantities of gain_sweep.h (A_k, B_k, J_k = [A_k | B_k], e_k, nu_k,
// lam_k, S_k (+ W_k), M_uu, M_us, M_ss, G_k, the held mask) and the tangents dx0, du_prev, dtraj, dweights =
// (dQ | dR | dRm), per stage on y_k = (x_k, u_k):
//   rho_k = J_k^T (2 Q o dtraj_k - 2 dQ o e_k),  and on the u rows
//           - 2 dR o ((u_k - u_{k-1}) - (u_{k+1} - u_k)) - 2 dRm o u_k      (u_{-1} = u_prev; no u_{k+1} term at k = N-1).
// On s = (dx_k, dv = du_{k-1}), P_N = 0, p_N = 0, backward over k = N-1..0:
//   q = C_k^T p_{k+1} + rho_k,  q_u of a held control 0,
//   kff_k = M_uu^-1 q_u,  p_k = (q_x; 0) + G_k^T q_u,  P_k = M_ss + M_su G_k;
// forward from s_0 = (dx0; du_prev):  du_k = G_k s_k + kff_k,  dx_{k+1} = A_k dx_k + B_k du_k,  s_{k+1} = (dx_{k+1}; du_k).
// Output: dV = (dx0, du_0, dx_1, .., dx_N);  du0 = du_0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "adjoint_sweep.h"

namespace mmpc {

struct TangentParams : SensParams {   // the head: gain_sweep.h
    const double* dx0;        // [B][nx] or null (zero)
    const double* du_prev;    // [B][nu] or null
    const double* dtraj;      // [B][N][nx] or null
    const double* dweights;   // [B][nx + 2 nu] or null
    double* dV;               // [B][NV] or null
    double* du0;              // [B][nu] or null
    int32_t* status;          // [B] or null: 0 as asked, 1 Gauss-Newton fallback, 2 failed (every output row 0)
    double* ws;               // the records; null in forward-free mode (dV null)
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(TangentParams) == 152 && offsetof(TangentParams, dx0) == 88, "kernel argument layout");
#pragma clang diagnostic pop

// the XB instantiations' parameters: TangentParams plus the sensitivity barrier's tail (gain_sweep.h)
struct TangentXbParams : TangentParams {
    XbTail xb;
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(TangentXbParams, xb) == 152 && sizeof(TangentXbParams) == 152 + sizeof(XbTail),
              "kernel argument layout");
#pragma clang diagnostic pop
template <bool XB>
using TangentParamsOf = std::conditional_t<XB, TangentXbParams, TangentParams>;

// du_k[c] = kff + row c of G_k times s = (dx; dv), as one chain of fused multiply-adds in a fixed order: the record's
// reader (the forward sweep) and the registers' reader (forward-free mode) get the same bits.  g: row c of G_k.
template <int NX, int NU>
__device__ __forceinline__ double tangent_control(double kff, const double* g, const double* dx, const double* dv) {
    double s = kff;
#pragma unroll
    for (int j = 0; j < NX; ++j) s = fma(g[j], dx[j], s);
#pragma unroll
    for (int d = 0; d < NU; ++d) s = fma(g[NX + d], dv[d], s);
    return s;
}

// One lane per instance, both sweeps in one launch, built as adjoint_lane_kernel is: the prologue and the backward
// stage are parts 0, 1 and 2 of sens_lane_stage.inc, with rho_k, q, kff and p between parts 1 and 2; the record
// G_k | kff_k has the adjoint's layout (element i of lane l of workgroup g at ws[(g * doubles per lane + i) * 64 + l],
// adjoint_lane_doubles per lane).  e_k comes from part 1's x, xd and tr; u_{k+1} is carried in registers from the
// trip before, u_{k-1} is read from V (u_prev at k = 0).  The forward sweep evaluates value and Jacobian again per
// stage and writes dV.  Forward-free mode (dV null): no record, no forward sweep, du_0 = G_0 s_0 + kff_0 from the
// registers of stage 0.  A second pass over both sweeps runs only for the Gauss-Newton fallback.  XB: the barrier's
// terms join the backward stage inside the shared text; rho, q, kff, p and the forward sweep are the same text with
// and without it, the barrier does not depend on theta.
template <class Model, bool EXACT, bool BOUNDED, bool XB = false>
__global__ __launch_bounds__(64) void tangent_lane_kernel(const TangentParamsOf<XB> p) {
    constexpr int NX = Model::NX, NU = Model::NU, K = NX + NU, NQ = Model::NQ, NA = NX - NQ, NP = K * (K + 1) / 2;
    constexpr int RD = NU * (K + 1);
    static_assert(RD == adjoint_rec_doubles(NX, NU), "the record is the adjoint's");
    static_assert(!EXACT || HasHess<Model>::value, "the exact tangent needs Model::eval_hess");
    static_assert(!XB || BOUNDED, "the XB instantiations read the control bounds");
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N;
    const double h = p.h;
    const int64_t NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    const double* v = p.V + b * NV;
    const double* w = p.weights + b * p.w_stride;
    const double* tr = p.traj + b * (int64_t)N * NX;
    const double* const dtr = p.dtraj ? p.dtraj + b * (int64_t)N * NX : nullptr;
    const bool full = p.dV != nullptr;
    double* const rec = full ? p.ws + (int64_t)blockIdx.x * ((int64_t)N * RD * 64) + threadIdx.x : nullptr;
    double* const dv = full ? p.dV + b * NV : nullptr;
#define MMPC_SENS_PART 0   // Q, R, Rm, lb, ub, up, fin
#include "sens_lane_stage.inc"
    // the tangents that are not per stage; a null tangent is zero and runs the same arithmetic
    double dx0[NX], dup[NU], dQ[NX], dR[NU], dRm[NU], du0[NU];
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        dx0[r] = p.dx0 ? p.dx0[b * NX + r] : 0.0;
        dQ[r] = p.dweights ? p.dweights[b * (NX + 2 * NU) + r] : 0.0;
        fin += gain_nonfinite(dx0[r]) + gain_nonfinite(dQ[r]);
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        dup[c] = p.du_prev ? p.du_prev[b * NU + c] : 0.0;
        dR[c] = p.dweights ? p.dweights[b * (NX + 2 * NU) + NX + c] : 0.0;
        dRm[c] = p.dweights ? p.dweights[b * (NX + 2 * NU) + NX + NU + c] : 0.0;
        fin += gain_nonfinite(dup[c]) + gain_nonfinite(dR[c]) + gain_nonfinite(dRm[c]);
        du0[c] = 0.0;
    }
    bool ok = false;
    int st = 0;
    for (int pass = 0; pass < (EXACT ? 2 : 1) && !ok; ++pass) {
        const bool exact = EXACT && pass == 0;
        st = pass;
        ok = fin == 0.0;
        // ---- backward: P_k, p_k, the record ----
        double P[NP], lam[NX], pv[K], un[NU];   // un: u_{k+1}
#pragma unroll
        for (int i = 0; i < NP; ++i) P[i] = 0.0;
#pragma unroll
        for (int r = 0; r < NX; ++r) lam[r] = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) pv[j] = 0.0;
#pragma unroll
        for (int c = 0; c < NU; ++c) un[c] = 0.0;
        for (int k = N - 1; k >= 0 && ok; --k) {
#define MMPC_SENS_PART 1   // the model, nu_k / lam, M_yy (+ W_k), the held rows, the factor of M_uu, G_k
#include "sens_lane_stage.inc"
            // rho_k;  q = C_k^T p_{k+1} + rho_k;  kff_k = M_uu^-1 q_u;  p_k = (q_x; 0) + G_k^T q_u
            double q[K], mq[NU], kff[NU], g[NX];   // g = 2 Q o dtraj_k - 2 dQ o e_k
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                const double e = x[r] + h * xd[r] - tr[k * NX + r];
                g[r] = 2.0 * Q[r] * (dtr ? dtr[k * NX + r] : 0.0) - 2.0 * dQ[r] * e;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double s = j >= NX ? pv[j] : 0.0;
#pragma unroll
                for (int r = 0; r < NX; ++r) s += J[r][j] * (pv[r] + g[r]);
                q[j] = s;
            }
            const bool last = k + 1 == N;
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                const double um = k > 0 ? v[(k - 1) * K + NX + c] : up[c];   // u_{k-1}
                const double t = (u[c] - um) - (last ? 0.0 : un[c] - u[c]);
                const double qu = q[NX + c] - 2.0 * dR[c] * t - 2.0 * dRm[c] * u[c];
                un[c] = u[c];
                q[NX + c] = held[c] ? 0.0 : qu;
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
            if (ok && !full && k == 0) {   // forward-free: du_0 from the registers of stage 0
                double bad = 0.0;
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    du0[c] = tangent_control<NX, NU>(kff[c], G[c], dx0, dup);
                    bad += gain_nonfinite(du0[c]);
                }
                ok = bad == 0.0;
            }
        }
        // ---- forward: dV ----
        if (ok && full) {
            double dx[NX], dum[NU], fbad = 0.0;   // s_k = (dx_k; du_{k-1})
#pragma unroll
            for (int r = 0; r < NX; ++r) dx[r] = dx0[r];
#pragma unroll
            for (int c = 0; c < NU; ++c) dum[c] = dup[c];
            for (int k = 0; k < N; ++k) {
                double x[NX], u[NU], xd[NX], fx[NX * NX], fu[NX * NU], du[NU], dn[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) x[r] = v[k * K + r];
#pragma unroll
                for (int c = 0; c < NU; ++c) u[c] = v[k * K + NX + c];
                model_eval_jac<Model>(x, u, xd, fx, fu);
                const double* const rk = rec + (int64_t)k * (RD * 64);
#pragma unroll
                for (int c = 0; c < NU; ++c) {   // du_k = G_k s_k + kff_k (a held control: a zero row and kff 0)
                    double gr[K];
#pragma unroll
                    for (int j = 0; j < K; ++j) gr[j] = rk[(c * (K + 1) + j) * 64];
                    du[c] = tangent_control<NX, NU>(rk[(c * (K + 1) + K) * 64], gr, dx, dum);
                    fbad += gain_nonfinite(du[c]);
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) dv[k * K + r] = dx[r];
#pragma unroll
                for (int c = 0; c < NU; ++c) dv[k * K + NX + c] = du[c];
                if (k == 0) {
#pragma unroll
                    for (int c = 0; c < NU; ++c) du0[c] = du[c];
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) {   // dx_{k+1} = A_k dx_k + B_k du_k
                    double s = dx[r];
#pragma unroll
                    for (int c = 0; c < NX; ++c) s += h * fx[r * NX + c] * dx[c];
#pragma unroll
                    for (int c = 0; c < NU; ++c) s += h * fu[r * NU + c] * du[c];
                    dn[r] = s;
                    fbad += gain_nonfinite(s);
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) dx[r] = dn[r];
#pragma unroll
                for (int c = 0; c < NU; ++c) dum[c] = du[c];
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) dv[(int64_t)N * K + r] = dx[r];
            ok = fbad == 0.0;
        }
    }
    if (!ok) {   // every output row of the instance 0
        st = 2;
#pragma unroll
        for (int c = 0; c < NU; ++c) du0[c] = 0.0;
        if (full)
            for (int64_t i = 0; i < NV; ++i) dv[i] = 0.0;
    }
    if (p.du0) {
#pragma unroll
        for (int c = 0; c < NU; ++c) p.du0[b * NU + c] = du0[c];
    }
    if (p.status) p.status[b] = st;
}

}  // namespace mmpc
