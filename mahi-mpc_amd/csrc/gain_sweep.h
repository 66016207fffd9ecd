// gain_sweep.h -- feedback gains along a plan: G_k = d u_k* / d(x_k, u_{k-1}) from one Riccati sweep
// (mmpc_feedback_gains_batch, include/mmpc.h).
//
// The tail problem from stage k is the stages k..N-1 of the NLP of ModelGenerator.cpp:191-222 from x_k = x with
// u_{k-1} = v; G_k [nu x (nx + nu)] is the derivative of its solution's first control with respect to (x, v) at the
// plan's own (x_k, u_{k-1}).  With s = (dx, dv), K = nx + nu and P_N = 0 (K x K), backward over k = N-1..0:
//   A_k = I + h f_x, B_k = h f_u, e_k = F(x_k, u_k) - r_k,
//   nu_k = 2 Q e_k + lam_k, lam_{N-1} = 0, lam_{k-1} = A_k^T nu_k            (the multipliers of the defects),
//   S_k = 2 [A_k | B_k]^T Q [A_k | B_k]  (+ W_k = Model::eval_hess(x_k, u_k, h nu_k[NQ:]) with the exact Hessian),
//   M_yy = C^T P_{k+1} C + S_k (+ W_k) on y = (dx, du), C = [[A_k, B_k], [0, I]]  (s' = (A dx + B du, du)),
//   M_uu = M_yy[u, u] + 2R + 2Rm,  M_us = [M_yy[u, x] | -2R],  M_ss = blkdiag(M_yy[x, x], 2R),
//   G_k = -M_uu^-1 M_us,  P_k = M_ss + M_su G_k.
// The Delta-u term's second +2R on u_k (for k + 1 < N) arrives through P_{k+1}'s v-v block; it is not added again.
// A held control (on a bound bit for bit, or k < n_pin) gets an identity row and column in M_uu and a zero row in
// M_us: its row of G_k is exactly 0.  M_uu is factorised by Cholesky; a pivot that is <= 0 or not finite under the
// exact Hessian redoes the whole instance with Gauss-Newton (status 1), and under Gauss-Newton fails it (status 2, all
// gains written as 0).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "models.h"
#include "sqp_group.h"

namespace mmpc {

// The head of every sensitivity kernel's parameters (the gain kernels here, the adjoint kernel of adjoint_sweep.h): the
// plan and the problem it solved.  The shared kernel text (sens_lane_stage.inc) reads only these and, with XB, the tail.
struct SensParams {
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
};
struct GainParams : SensParams {
    int32_t n_gain;         // stages written
    double* G;              // [B][n_gain][nu][nx + nu]
    int32_t* status;        // [B] or null: 0 as asked, 1 Gauss-Newton fallback, 2 failed (gains 0)
    int gpw;                // 16-lane kernel: instances per workgroup (<= kGroupsPerWave)
};
// the kernel arguments' layout is the one the structs had with the head written out member by member (offsetof of a
// struct with a base is conditionally supported; the compiler of HIP supports it and says so with a warning)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(SensParams) == 88 && sizeof(GainParams) == 120, "kernel argument layout");
static_assert(offsetof(GainParams, n_gain) == 88, "kernel argument layout");
#pragma clang diagnostic pop

// The sensitivity barrier of a state-bounded handle (mmpc_set_sensitivity_barrier, include/mmpc.h): the
// XB instantiations take GainParams plus this tail, so the kernel arguments of every other instantiation stay as
// they are.  With y a bounded entry (x_{k+1} under x_lb / x_ub, u_k of a stage k >= n_pin under u_lb / u_ub), slacks
// s_l = y - l, s_u = u - y:  beta = 2 mu (1 / s_u - 1 / s_l),  D = min(2 mu (1 / s_l^2 + 1 / s_u^2), cap);  then
//   lam_{N-1} = beta(x_N), lam_{k-1} = A_k^T nu_k + beta(x_k),  P_{k+1}[x, x] += diag D(x_{k+1}) before M_yy is formed,
//   M_uu += diag D(u_k);  no control is held by bit-equality (the interior point returns none on its bound).
struct XbTail {
    double x_lb[16], x_ub[16];   // |b| >= 1e19 is infinite
    double mu, cap;
};
struct GainXbParams : GainParams {
    XbTail xb;
};
template <bool XB>
using GainParamsOf = std::conditional_t<XB, GainXbParams, GainParams>;

// beta and D of one entry y under (l, u); false when a slack of a finite side is <= 0 or not finite
__device__ __forceinline__ bool xb_terms(double y, double l, double u, double mu, double cap, double& beta, double& D) {
    bool ok = true;
    double d = 0.0;
    beta = 0.0;
    if (u < 1e19) {
        const double s = u - y;
        ok = ok && s > 0.0 && s < INFINITY;
        beta += 2.0 * mu / s;
        d += 2.0 * mu / (s * s);
    }
    if (l > -1e19) {
        const double s = y - l;
        ok = ok && s > 0.0 && s < INFINITY;
        beta -= 2.0 * mu / s;
        d += 2.0 * mu / (s * s);
    }
    D = fmin(d, cap);
    return ok;
}

// index of (i, j) in the packed upper triangle of a symmetric n x n matrix
__host__ __device__ constexpr int gain_sym(int i, int j, int n) {
    return i <= j ? i * n - i * (i - 1) / 2 + (j - i) : j * n - j * (j - 1) / 2 + (i - j);
}
// NaN when v is not finite, else 0: summed into a flag that must stay == 0
__device__ __forceinline__ double gain_nonfinite(double v) { return v * 0.0; }

// Cholesky of the nu x nu matrix a (lower factor in place, il = 1 / diagonal); false when a pivot is <= 0 or not finite
template <int NU>
__device__ __forceinline__ bool gain_chol(double (*a)[NU], double* il) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        double d = a[c][c];
#pragma unroll
        for (int e = 0; e < c; ++e) d -= a[c][e] * a[c][e];
        ok = ok && d > 0.0 && d < INFINITY;
        const double l = sqrt(d);
        a[c][c] = l;
        il[c] = 1.0 / l;
#pragma unroll
        for (int r = c + 1; r < NU; ++r) {
            double s = a[r][c];
#pragma unroll
            for (int e = 0; e < c; ++e) s -= a[r][e] * a[c][e];
            a[r][c] = s * il[c];
        }
    }
    return ok;
}
// g = -(L L^T)^-1 m
template <int NU>
__device__ __forceinline__ void gain_solve(const double (*l)[NU], const double* il, const double* m, double* g) {
    double y[NU];
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        double s = -m[c];
#pragma unroll
        for (int e = 0; e < c; ++e) s -= l[c][e] * y[e];
        y[c] = s * il[c];
    }
#pragma unroll
    for (int c = NU - 1; c >= 0; --c) {
        double s = y[c];
#pragma unroll
        for (int e = c + 1; e < NU; ++e) s -= l[e][c] * g[e];
        g[c] = s * il[c];
    }
}
// control c of stage k is held: committed (k < n_pin) or on a finite bound bit for bit (the projected SQP returns
// exact bound values; |b| >= 1e19 is infinite)
template <bool BOUNDED>
__device__ __forceinline__ bool gain_held(int k, int n_pin, double u, double lb, double ub) {
    bool held = k < n_pin;
    if constexpr (BOUNDED) held = held || (lb > -1e19 && u == lb) || (ub < 1e19 && u == ub);
    return held;
}

// One lane per instance: a single fused backward sweep -- Jacobian, nu / lam, W_k, the stage step and the store of
// G_k for k < n_gain per stage.  No workspace: the only traffic is V, the targets and G.  A second pass runs only
// for the Gauss-Newton fallback.  XB: the sensitivity barrier's terms join the stage (XbTail).  The prologue and the
// stage are the text of sens_lane_stage.inc, which adjoint_lane_kernel (adjoint_sweep.h) compiles in too: parts 0, 1, 2.
template <class Model, bool EXACT, bool BOUNDED, bool XB = false>
__global__ __launch_bounds__(64) void gain_lane_kernel(const GainParamsOf<XB> p) {
    constexpr int NX = Model::NX, NU = Model::NU, K = NX + NU, NQ = Model::NQ, NA = NX - NQ, NP = K * (K + 1) / 2;
    static_assert(!EXACT || HasHess<Model>::value, "exact gains need Model::eval_hess");
    static_assert(!XB || BOUNDED, "the XB instantiations read the control bounds");
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N;
    const double h = p.h;
    const int64_t NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    const double* v = p.V + b * NV;
    const double* w = p.weights + b * p.w_stride;
    const double* tr = p.traj + b * (int64_t)N * NX;
    double* Gb = p.G + b * (int64_t)p.n_gain * (NU * K);
#define MMPC_SENS_PART 0   // Q, R, Rm, lb, ub, up, fin
#include "sens_lane_stage.inc"
    bool ok = false;
    int st = 0;
    for (int pass = 0; pass < (EXACT ? 2 : 1) && !ok; ++pass) {
        const bool exact = EXACT && pass == 0;
        st = pass;
        ok = fin == 0.0;
        double P[NP], lam[NX];
#pragma unroll
        for (int i = 0; i < NP; ++i) P[i] = 0.0;
#pragma unroll
        for (int r = 0; r < NX; ++r) lam[r] = 0.0;
        for (int k = N - 1; k >= 0 && ok; --k) {
#define MMPC_SENS_PART 1   // the model, nu_k / lam, M_yy (+ W_k), the held rows, the factor of M_uu, G_k
#include "sens_lane_stage.inc"
#define MMPC_SENS_PART 2   // P_k = M_ss + M_su G_k
#include "sens_lane_stage.inc"
            ok = ok && chk == 0.0;
            if (ok && k < p.n_gain) {
#pragma unroll
                for (int c = 0; c < NU; ++c)
#pragma unroll
                    for (int j = 0; j < K; ++j) Gb[(int64_t)k * (NU * K) + c * K + j] = G[c][j];
            }
        }
    }
    if (!ok) {   // pure feed-forward: every gain of the instance 0
        st = 2;
        for (int i = 0; i < p.n_gain * (NU * K); ++i) Gb[i] = 0.0;
    }
    if (p.status) p.status[b] = st;
}

// ---- 16 lanes per instance ----
// LDS doubles per stage record: [A_k | B_k] (nx x K), nu_k (nx; 2 Q e_k until the lam recursion has passed), the held
// controls of the stage as a bit mask, with the exact Hessian W_k (K x K), and with the sensitivity barrier
// beta(x_{k+1}) (nx), D(x_{k+1}) (nx) and D(u_k) (nu)
__host__ __device__ constexpr int gain_group_rec_doubles(int nx, int nu, bool exact, bool xb = false) {
    return nx * (nx + nu) + nx + 1 + (exact ? (nx + nu) * (nx + nu) : 0) + (xb ? 2 * nx + nu : 0);
}
// LDS doubles per instance: N stage records, then the exchange area of the Riccati sweep (the rows of P C, K x K, and
// the u rows of M_yy, nu x K)
__host__ __device__ constexpr int gain_group_lds_doubles(int nx, int nu, int N, bool exact, bool xb = false) {
    return N * gain_group_rec_doubles(nx, nu, exact, xb) + (nx + nu) * (nx + nu) + nu * (nx + nu);
}

// 16 lanes per instance, p.gpw (<= kGroupsPerWave) instances per one-wave workgroup: the partition of the 16-lane
// solver, for batches that do not fill the device with one lane each (nx + nu < 16).
//   A. stage-parallel (lane = stage mod 16): [A_k | B_k], 2 Q e_k and the held mask of every stage, into LDS (XB: and
//      the barrier terms of x_{k+1} and u_k; a slack that is <= 0 or not finite fails the instance);
//   B. the serial lam recursion, component r on lane r: one nx x nx mat-vec per stage through LDS;
//   C. stage-parallel: W_k (exact Hessian);
//   D. the serial Riccati sweep, column j of P, M_yy and G on lane j < K.  Lane j forms row j of P C; the rows are
//      exchanged through LDS (each lane reads its column), as are the u rows of M_yy; the nu x nu factor of M_uu is
//      computed redundantly on every lane, so the pivot test is uniform over the group.
// The stage records live in LDS (dynamic, gain_group_lds_doubles per instance): the launch takes as many instances per
// workgroup as fit 160 KB, and a horizon whose single instance does not fit is refused by the host (no HBM scratch).
// Lanes of a group run in lock step within their wave, so the LDS exchanges need only the compiler-level wave barrier,
// as in sqp_group.h.  The instance prologue is part 0 of sens_lane_stage.inc; the phases are this kernel's own.
extern __shared__ double gain_group_lds[];
template <class Model, bool EXACT, bool BOUNDED, bool XB = false>
__global__ __launch_bounds__(64) void gain_group_kernel(const GainParamsOf<XB> p) {
    constexpr int NX = Model::NX, NU = Model::NU, K = NX + NU, NQ = Model::NQ, NA = NX - NQ, G = kGroupLanes;
    static_assert(K < G, "the 16-lane gain kernel holds one column of P per lane");
    static_assert(!EXACT || HasHess<Model>::value, "exact gains need Model::eval_hess");
    static_assert(!XB || BOUNDED, "the XB instantiations read the control bounds");
    constexpr int RS = gain_group_rec_doubles(NX, NU, EXACT, XB), OJ = 0, ONU = NX * K, OH = ONU + NX, OW = OH + 1;
    [[maybe_unused]] constexpr int OBE = OW + (EXACT ? K * K : 0), ODX = OBE + NX, ODU = ODX + NX;
    const int grp = threadIdx.x / G, l = threadIdx.x % G;
    const int64_t b = blockIdx.x * (int64_t)p.gpw + grp;
    if (grp >= p.gpw || b >= p.B) return;
    const int N = p.N;
    const double h = p.h;
    double* const rec = gain_group_lds + (size_t)grp * gain_group_lds_doubles(NX, NU, N, EXACT, XB);
    double* const sX = rec + (size_t)N * RS;
    double* const sMu = sX + K * K;
    const int64_t NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    const double* v = p.V + b * NV;
    const double* w = p.weights + b * p.w_stride;
    const double* tr = p.traj + b * (int64_t)N * NX;
    double* Gb = p.G + b * (int64_t)p.n_gain * (NU * K);
#define MMPC_SENS_PART 0   // Q, R, Rm, lb, ub, up, fin
#include "sens_lane_stage.inc"
    // ---- A ----
    for (int k = l; k < N; k += G) {
        double x[NX], u[NU], xd[NX], fx[NX * NX], fu[NX * NU];
#pragma unroll
        for (int r = 0; r < NX; ++r) x[r] = v[k * K + r];
#pragma unroll
        for (int c = 0; c < NU; ++c) u[c] = v[k * K + NX + c];
        model_eval_jac<Model>(x, u, xd, fx, fu);
        double* const rk = rec + (size_t)k * RS;
#pragma unroll
        for (int r = 0; r < NX; ++r) {
#pragma unroll
            for (int c = 0; c < NX; ++c) rk[OJ + r * K + c] = (r == c ? 1.0 : 0.0) + h * fx[r * NX + c];
#pragma unroll
            for (int c = 0; c < NU; ++c) rk[OJ + r * K + NX + c] = h * fu[r * NU + c];
            rk[ONU + r] = 2.0 * Q[r] * (x[r] + h * xd[r] - tr[k * NX + r]);
        }
        int hm = 0;
#pragma unroll
        for (int c = 0; c < NU; ++c) hm |= gain_held<BOUNDED && !XB>(k, p.n_pin, u[c], lb[c], ub[c]) ? (1 << c) : 0;
        rk[OH] = static_cast<double>(hm);
        if constexpr (XB) {
            bool in = true;
#pragma unroll
            for (int r = 0; r < NX; ++r)
                in = xb_terms(v[(k + 1) * K + r], p.xb.x_lb[r], p.xb.x_ub[r], p.xb.mu, p.xb.cap, rk[OBE + r],
                              rk[ODX + r]) && in;
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                double be;
                rk[ODU + c] = 0.0;
                if (k >= p.n_pin) in = xb_terms(u[c], lb[c], ub[c], p.xb.mu, p.xb.cap, be, rk[ODU + c]) && in;
            }
            fin += in ? 0.0 : NAN;
        }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- B ----
    {
        const int r0 = l < NX ? l : NX - 1;   // lanes past nx repeat the last component and write nothing
        double lam = 0.0;
        for (int k = N - 1; k >= 0; --k) {
            double* const rk = rec + (size_t)k * RS;
            if (l < NX) {
                if constexpr (XB) lam += rk[OBE + l];   // lam_k = A_{k+1}^T nu_{k+1} + beta(x_{k+1})
                rk[ONU + l] += lam;
                fin += gain_nonfinite(rk[ONU + l]);   // a non-finite target fails the instance under either Hessian
            }
            __builtin_amdgcn_wave_barrier();
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < NX; ++r) s += rk[OJ + r * K + r0] * rk[ONU + r];
            lam = s;
        }
        fin = group_max(fin == 0.0 ? 0.0 : 1.0);
    }
    __builtin_amdgcn_wave_barrier();
    // ---- C ----
    if constexpr (EXACT) {
        for (int k = l; k < N; k += G) {
            double x[NX], u[NU], la[NA], W[K * K];
            double* const rk = rec + (size_t)k * RS;
#pragma unroll
            for (int r = 0; r < NX; ++r) x[r] = v[k * K + r];
#pragma unroll
            for (int c = 0; c < NU; ++c) u[c] = v[k * K + NX + c];
#pragma unroll
            for (int s2 = 0; s2 < NA; ++s2) la[s2] = h * rk[ONU + NQ + s2];
            Model::eval_hess(x, u, la, W);
#pragma unroll
            for (int i = 0; i < K * K; ++i) rk[OW + i] = W[i];
        }
        __builtin_amdgcn_wave_barrier();
    }
    // ---- D ----
    const bool act = l < K;
    const int j = act ? l : K - 1;   // lanes past K repeat the last column and write nothing
    bool ok = false;
    int st = 0;
    for (int pass = 0; pass < (EXACT ? 2 : 1) && !ok; ++pass) {
        const bool exact = EXACT && pass == 0;
        st = pass;
        ok = fin == 0.0;
        double P[K], bad = 0.0;   // row j (= column j) of P
#pragma unroll
        for (int i = 0; i < K; ++i) P[i] = 0.0;
        for (int k = N - 1; k >= 0 && ok; --k) {
            const double* const rk = rec + (size_t)k * RS;
            const double* const J = rk + OJ;
            if constexpr (XB) {   // P_{k+1}[x, x] += diag D(x_{k+1}), in place before the products
#pragma unroll
                for (int i = 0; i < NX; ++i) P[i] += i == j ? rk[ODX + i] : 0.0;
            }
            __builtin_amdgcn_wave_barrier();   // the exchange area is free: every lane has read the last stage's
#pragma unroll
            for (int c = 0; c < K; ++c) {      // row j of P C
                double s = c >= NX ? P[c] : 0.0;
#pragma unroll
                for (int q = 0; q < NX; ++q) s += P[q] * J[q * K + c];
                if (act) sX[j * K + c] = s;
            }
            __builtin_amdgcn_wave_barrier();
            double t[K], M[K];   // column j of P C and of M_yy
#pragma unroll
            for (int a = 0; a < K; ++a) t[a] = sX[a * K + j];
#pragma unroll
            for (int i = 0; i < K; ++i) {
                double s = i >= NX ? t[i] : 0.0;
#pragma unroll
                for (int a = 0; a < NX; ++a) s += J[a * K + i] * t[a];
#pragma unroll
                for (int r = 0; r < NX; ++r) s += 2.0 * Q[r] * J[r * K + i] * J[r * K + j];
                if constexpr (EXACT) {
                    if (exact) s += rk[OW + i * K + j];
                }
                M[i] = s;
            }
#pragma unroll
            for (int c = 0; c < NU; ++c)
                if (act) sMu[c * K + j] = M[NX + c];
            __builtin_amdgcn_wave_barrier();
            const int hm = static_cast<int>(rk[OH]);
            double Muu[NU][NU], m[NU], g[NU], il[NU];
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                const bool hc = (hm >> c) & 1;
#pragma unroll
                for (int d = 0; d < NU; ++d) {
                    double e = sMu[c * K + NX + d] + (c == d ? 2.0 * R[c] + 2.0 * Rm[c] : 0.0);
                    if constexpr (XB) e += c == d ? rk[ODU + c] : 0.0;
                    Muu[c][d] = (hc || ((hm >> d) & 1)) ? (c == d ? 1.0 : 0.0) : e;
                }
                m[c] = hc ? 0.0 : (j < NX ? M[NX + c] : (j == NX + c ? -2.0 * R[c] : 0.0));
            }
            ok = gain_chol<NU>(Muu, il);
            gain_solve<NU>(Muu, il, m, g);
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                g[c] = ((hm >> c) & 1) ? 0.0 : g[c];
                bad += gain_nonfinite(g[c]);
            }
            // column j of P_k = M_ss + M_su G_k
#pragma unroll
            for (int i = 0; i < K; ++i) {
                double s = i < NX ? (j < NX ? M[i] : 0.0) : (i == j ? 2.0 * R[i - (i >= NX ? NX : 0)] : 0.0);
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    const double mus = ((hm >> c) & 1) ? 0.0 : (i < NX ? sMu[c * K + i] : (i == NX + c ? -2.0 * R[c] : 0.0));
                    s += mus * g[c];
                }
                P[i] = s;
            }
            if (ok && act && k < p.n_gain) {
#pragma unroll
                for (int c = 0; c < NU; ++c) Gb[(int64_t)k * (NU * K) + c * K + j] = g[c];
            }
        }
#pragma unroll
        for (int i = 0; i < K; ++i) bad += gain_nonfinite(P[i]);
        ok = ok && group_max(bad == 0.0 ? 0.0 : 1.0) == 0.0;
    }
    if (!ok) {
        st = 2;
        for (int i = l; i < p.n_gain * (NU * K); i += G) Gb[i] = 0.0;
    }
    if (p.status && l == 0) p.status[b] = st;
}

}  // namespace mmpc
