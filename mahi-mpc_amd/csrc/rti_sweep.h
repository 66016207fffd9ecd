// rti_sweep.h -- real-time iteration: one full-step SQP iteration at a plan that is NOT a solution, split into a
// preparation launch (everything that does not depend on the measured state) and a feedback launch (one forward sweep
// over stored records, no model inside) (mmpc_rti_prepare_batch / mmpc_rti_feedback_batch, include/mmpc.h).
// The shift of the plan between two ticks (mmpc_rti_shift_batch) is at the end of the file.
//
// The step dV at the plan V^ solves
//   min 1/2 dV^T H dV + grad J(V^)^T dV   s.t.  dx_{k+1} = A_k dx_k + B_k du_k + c_k,  dx_0 = x0_meas - x^_0,
//   du_k = 0 on held controls,            c_k = F(x^_k, u^_k) - x^_{k+1},
// with H, the multipliers nu_k / lam_k, the held mask, P_k, M_*, G_k those of gain_sweep.h.  On the feasible set
// grad J^T dV differs from grad L^T dV by a constant, and with the multipliers of the gain recursion the x rows of
// grad L vanish; what is left is on the u rows,
//   r_{u,k} = B_k^T nu_k + 2R((u_k - u_{k-1}) - (u_{k+1} - u_k)) + 2Rm u_k   (u_{-1} = u_prev; no u_{k+1} term at k = N-1).
// The cost-to-go 1/2 s^T P_k s - p_k^T s on s = (dx_k, du_{k-1}) -- the sign of p is the one tangent_sweep.h uses, so
// the vector part is that file's recursion with rho_k = -(0; r_{u,k}) - C_k^T P_{k+1} (c_k; 0):
//   q = C_k^T (p_{k+1} - P_{k+1} (c_k; 0)) - (0; r_{u,k}),  q_u of a held control 0,
//   kff_k = M_uu^-1 q_u,  p_k = (q_x; 0) + G_k^T q_u,  P_k = M_ss + M_su G_k,  p_N = 0;
// forward from s_0 = (dx_0; 0) (u_prev is known when the preparation runs):
//   du_k = G_k s_k + kff_k,  dx_{k+1} = A_k dx_k + B_k du_k + c_k,  s_{k+1} = (dx_{k+1}; du_k).
// With control bounds the forward sweep is the projected one of box-iLQR: u_k+ = clamp(u^_k + du_k, lb, ub) and
// du_k = u_k+ - u^_k is what is propagated; a du_k that is exactly 0 (a held control: zero row of G_k, kff 0) leaves
// the control as it is, so a pinned control outside the box stays pinned.
//
// The record of stage k is a K x (K + 1) matrix, rows 0..nu-1 = [G_k | kff_k] (the record of adjoint_sweep.h), rows
// nu..K-1 = [A_k | B_k | c_k]: K (K + 1) doubles.  Element i of stage k of lane l of workgroup g is at
// rec[((g N + k) K (K + 1) + i) 64 + l].  The workspace is  records | undo log (NV doubles per lane, lane-interleaved
// the same way) | one int32 status word per lane:  rti_workspace_bytes below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "tangent_sweep.h"

namespace mmpc {

__host__ __device__ constexpr int rti_rec_doubles(int nx, int nu) { return (nx + nu) * (nx + nu + 1); }
// doubles of the record region and of the undo log, per block of 64 lanes
__host__ __device__ constexpr uint64_t rti_rec_block_doubles(int nx, int nu, int N) {
    return static_cast<uint64_t>(N) * rti_rec_doubles(nx, nu) * 64;
}
__host__ __device__ constexpr uint64_t rti_undo_block_doubles(int nx, int nu, int N) {
    return (static_cast<uint64_t>(nx) * (N + 1) + static_cast<uint64_t>(nu) * N) * 64;
}
// ceil(B / 64) blocks of 64 lanes, each (N K (K + 1) + NV) doubles and one int32 per lane
__host__ __device__ constexpr uint64_t rti_workspace_bytes(int nx, int nu, int N, int64_t B) {
    const uint64_t blocks = (static_cast<uint64_t>(B) + 63) / 64;
    return blocks * ((rti_rec_block_doubles(nx, nu, N) + rti_undo_block_doubles(nx, nu, N)) * sizeof(double) +
                     64 * sizeof(int32_t));
}

struct RtiPrepareParams : SensParams {   // the head: gain_sweep.h
    int32_t* status;      // [B] or null: 0 as asked, 1 Gauss-Newton fallback, 2 failed
    double* rec;          // the records
    int32_t* ws_status;   // the workspace's status words: what the feedback launch reads
};
// sens_lane_stage.inc names p.xb under `if constexpr (XB)`, which discards it only while p's type depends on XB: the
// kernel keeps the template parameter, is instantiated with XB = false alone, and the host fills this struct
struct RtiPrepareXbParams : RtiPrepareParams {
    XbTail xb;
};
template <bool XB>
using RtiPrepareParamsOf = std::conditional_t<XB, RtiPrepareXbParams, RtiPrepareParams>;
struct RtiFeedbackParams {
    int64_t B;
    int N;
    const double* x0;       // [B][nx], the measured state
    const double* u_lb;     // BOUNDED kernels: [nu] (b_stride 0) or row b at b * b_stride; either may be null
    const double* u_ub;
    int32_t b_stride;
    double* V;              // [B][NV], in: the plan of the preparation, out: V^ + dV
    double* u0;             // [B][nu] or null
    double* step_inf;       // [B] or null
    int32_t* status;        // [B] or null
    const double* rec;      // the records
    double* undo;           // the undo log
    const int32_t* ws_status;
};

// Preparation: one lane per instance, built as tangent_lane_kernel is -- parts 0, 1 and 2 of sens_lane_stage.inc with
// this kernel's block between parts 1 and 2: r_{u,k}, c_k, q, kff, p, and the store of the record.  A second pass over
// the sweep runs only for the Gauss-Newton fallback and writes the whole record again.  u_{k+1} is carried in
// registers from the trip before, u_{k-1} and x_{k+1} are read from V.
template <class Model, bool EXACT, bool BOUNDED, bool XB = false>
__global__ __launch_bounds__(64) void rti_prepare_lane_kernel(const RtiPrepareParamsOf<XB> p) {
    constexpr int NX = Model::NX, NU = Model::NU, K = NX + NU, NQ = Model::NQ, NA = NX - NQ, NP = K * (K + 1) / 2;
    constexpr int RD = rti_rec_doubles(NX, NU);
    static_assert(!XB, "a state-bounded handle is refused by the host");
    static_assert(!EXACT || HasHess<Model>::value, "the exact step needs Model::eval_hess");
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N;
    const double h = p.h;
    const int64_t NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    const double* v = p.V + b * NV;
    const double* w = p.weights + b * p.w_stride;
    const double* tr = p.traj + b * (int64_t)N * NX;
    double* const rec = p.rec + (int64_t)blockIdx.x * ((int64_t)N * RD * 64) + threadIdx.x;
#define MMPC_SENS_PART 0   // Q, R, Rm, lb, ub, up, fin
#include "sens_lane_stage.inc"
    bool ok = false;
    int st = 0;
    for (int pass = 0; pass < (EXACT ? 2 : 1) && !ok; ++pass) {
        const bool exact = EXACT && pass == 0;
        st = pass;
        ok = fin == 0.0;
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
            // c_k;  t = p_{k+1} - P_{k+1} (c_k; 0);  q = C_k^T t - (0; r_{u,k});  kff_k = M_uu^-1 q_u;
            // p_k = (q_x; 0) + G_k^T q_u
            double ck[NX], t[K], q[K], mq[NU], kff[NU];
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                ck[r] = (x[r] + h * xd[r]) - v[(k + 1) * K + r];
                chk += gain_nonfinite(ck[r]);
            }
#pragma unroll
            for (int a = 0; a < K; ++a) {
                double s = pv[a];
#pragma unroll
                for (int r = 0; r < NX; ++r) s -= P[gain_sym(a, r, K)] * ck[r];
                t[a] = s;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                double s = j >= NX ? t[j] : 0.0;
#pragma unroll
                for (int r = 0; r < NX; ++r) s += J[r][j] * t[r];
                q[j] = s;
            }
            const bool last = k + 1 == N;
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                const double um = k > 0 ? v[(k - 1) * K + NX + c] : up[c];   // u_{k-1}
                double ru = 2.0 * R[c] * ((u[c] - um) - (last ? 0.0 : un[c] - u[c])) + 2.0 * Rm[c] * u[c];
#pragma unroll
                for (int r = 0; r < NX; ++r) ru += J[r][NX + c] * nuk[r];
                un[c] = u[c];
                q[NX + c] = held[c] ? 0.0 : q[NX + c] - ru;
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
            if (ok) {
                double* const rk = rec + (int64_t)k * (RD * 64);
#pragma unroll
                for (int c = 0; c < NU; ++c) {
#pragma unroll
                    for (int j = 0; j < K; ++j) rk[(c * (K + 1) + j) * 64] = G[c][j];
                    rk[(c * (K + 1) + K) * 64] = kff[c];
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) {
#pragma unroll
                    for (int j = 0; j < K; ++j) rk[((NU + r) * (K + 1) + j) * 64] = J[r][j];
                    rk[((NU + r) * (K + 1) + K) * 64] = ck[r];
                }
            }
        }
    }
    if (!ok) st = 2;
    p.ws_status[b] = st;
    if (p.status) p.status[b] = st;
}

// Stages of the record the feedback kernel keeps in registers: a ring of D slots, each K (K + 1) record doubles and
// the K plan entries of its stage.  The loads of a slot do not depend on the sweep's chain; a slot is loaded again,
// for the stage D later, as soon as its stage has used it, so the load of a stage is issued D - 1 stages of
// multiply-adds before its first use.  160 doubles (320 of the 512 registers a one-wave workgroup can have) are the
// budget: D = 3 for the 2-link arm (K = 6), 4 for K <= 5, 1 for the exo (K = 12, one record is 156 doubles), where the
// rows [G | kff] of the next stage are asked for while [A | B | c] of this one are multiplied, and no earlier.
// A model whose one slot is over the budget still gets D = 1 (mass_chain, K = 16: 272 + 16 = 288 doubles).  The
// unbounded kernel then takes 256 + 23 registers and no scratch -- the rows of a record are loaded as the sweep consumes
// them, the slot never stands in registers whole -- and the bounded one spills 175 registers to 632 B of scratch.
__host__ __device__ constexpr int rti_ring_slots(int nx, int nu) {
    const int per = rti_rec_doubles(nx, nu) + nx + nu, d = 160 / per;
    return d < 1 ? 1 : (d > 4 ? 4 : d);
}

// Feedback: one lane per instance, the forward sweep over the records; no model, no factor, no trig.  Per stage the
// dependent chain is K multiply-adds for du_k (tangent_control's fixed order), the clamp, and nu multiply-adds per row
// of dx_{k+1} (c_k + A_k dx_k comes first in the row's fixed order and does not wait for du_k).  The plan is read from
// V and overwritten stage by stage; what is overwritten goes into the undo log first, so that a step that turns out
// non-finite leaves V bit for bit as given.  step_inf is the maximum of |new - old| over the entries as stored.
template <int NX, int NU, bool BOUNDED, int D = rti_ring_slots(NX, NU)>
__global__ __launch_bounds__(64) void rti_feedback_lane_kernel(const RtiFeedbackParams p) {
    constexpr int K = NX + NU, RD = rti_rec_doubles(NX, NU);
    static_assert(D >= 1, "the ring has at least the slot of the stage at work");
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N;
    const int64_t NV = (int64_t)NX * (N + 1) + (int64_t)NU * N;
    double* const v = p.V + b * NV;
    const double* const rec = p.rec + (int64_t)blockIdx.x * ((int64_t)N * RD * 64) + threadIdx.x;
    double* const undo = p.undo + (int64_t)blockIdx.x * (NV * 64) + threadIdx.x;
    int st = p.ws_status[b];
    double lb[NU], ub[NU], u0[NU], dx[NX], dum[NU], x0m[NX], xN[NX], bad = 0.0;
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        lb[c] = (BOUNDED && p.u_lb) ? p.u_lb[b * p.b_stride + c] : -INFINITY;
        ub[c] = (BOUNDED && p.u_ub) ? p.u_ub[b * p.b_stride + c] : INFINITY;
        u0[c] = v[NX + c];
        dum[c] = 0.0;
    }
#pragma unroll
    for (int r = 0; r < NX; ++r) {
        x0m[r] = p.x0[b * NX + r];
        xN[r] = v[(int64_t)N * K + r];
        dx[r] = x0m[r] - v[r];
        bad += gain_nonfinite(dx[r]);
    }
    bool ok = st != 2 && bad == 0.0;
    double smax = 0.0;
    if (ok) {
        double rg[D][RD], y[D][K], fbad = 0.0;   // the ring: record and plan entries of stage k in slot k mod D
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int kn = j < N ? j : N - 1;
            const double* const rk = rec + (int64_t)kn * (RD * 64);
#pragma unroll
            for (int i = 0; i < RD; ++i) rg[j][i] = rk[i * 64];
#pragma unroll
            for (int i = 0; i < K; ++i) y[j][i] = v[kn * K + i];
        }
        for (int k0 = 0; k0 < N; k0 += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const int k = k0 + j;
                const int kn = k + D < N ? k + D : N - 1;   // the stage this slot holds next (in bounds past the end)
                const double* const rn = rec + (int64_t)kn * (RD * 64);
                if (k < N) {
                    double du[NU], unew[NU], dn[NX];
#pragma unroll
                    for (int c = 0; c < NU; ++c) {   // du_k = G_k s_k + kff_k (a held control: a zero row and kff 0)
                        const double uh = y[j][NX + c];
                        const double d = tangent_control<NX, NU>(rg[j][c * (K + 1) + K], &rg[j][c * (K + 1)], dx, dum);
                        fbad += gain_nonfinite(d);
                        double un = uh + d;
                        if constexpr (BOUNDED) {
                            un = d == 0.0 ? uh : fmin(fmax(un, lb[c]), ub[c]);
                            du[c] = un - uh;
                        } else {
                            du[c] = d;
                        }
                        unew[c] = un;
                        smax = fmax(smax, fabs(un - uh));
                    }
#pragma unroll
                    for (int r = 0; r < NX; ++r) {   // x_k as stored: x0_meas at k = 0
                        const double xh = y[j][r];
                        const double xn = k == 0 ? x0m[r] : xh + dx[r];
                        undo[((int64_t)k * K + r) * 64] = xh;
                        v[k * K + r] = xn;
                        smax = fmax(smax, fabs(xn - xh));
                    }
#pragma unroll
                    for (int c = 0; c < NU; ++c) {
                        undo[((int64_t)k * K + NX + c) * 64] = y[j][NX + c];
                        v[k * K + NX + c] = unew[c];
                        if (k == 0) u0[c] = unew[c];
                    }
#pragma unroll
                    for (int r = 0; r < NX; ++r) {   // dx_{k+1} = c_k + A_k dx_k + B_k du_k, in this order
                        const double* const row = &rg[j][(NU + r) * (K + 1)];
                        double s = row[K];
#pragma unroll
                        for (int c = 0; c < NX; ++c) s = fma(row[c], dx[c], s);
#pragma unroll
                        for (int c = 0; c < NU; ++c) s = fma(row[NX + c], du[c], s);
                        dn[r] = s;
                        fbad += gain_nonfinite(s);
                    }
#pragma unroll
                    for (int r = 0; r < NX; ++r) dx[r] = dn[r];
#pragma unroll
                    for (int c = 0; c < NU; ++c) dum[c] = du[c];
                }
#pragma unroll
                for (int i = 0; i < RD; ++i) rg[j][i] = rn[i * 64];
#pragma unroll
                for (int i = 0; i < K; ++i) y[j][i] = v[kn * K + i];
            }
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            const double xn = xN[r] + dx[r];
            undo[((int64_t)N * K + r) * 64] = xN[r];
            v[(int64_t)N * K + r] = xn;
            smax = fmax(smax, fabs(xn - xN[r]));
        }
        ok = fbad == 0.0;
        if (!ok) {   // V bit for bit as given
            for (int64_t i = 0; i < NV; ++i) v[i] = undo[i * 64];
#pragma unroll
            for (int c = 0; c < NU; ++c) u0[c] = undo[(int64_t)(NX + c) * 64];
        }
    }
    if (!ok) st = 2;
    if (p.u0) {
#pragma unroll
        for (int c = 0; c < NU; ++c) p.u0[b * NU + c] = u0[c];
    }
    if (p.step_inf) p.step_inf[b] = ok ? smax : INFINITY;
    if (p.status) p.status[b] = st;
}

// ---- the shift between two ticks (mmpc_rti_shift_batch) ----
// V_out is V_in moved n stages earlier: entries 0 .. (N - n) K + nx - 1 of a row are entries n K .. of the old row, the
// later controls are the old u_{N-1}, the later states are rolled out by x_{k+1} = x_k + h f(x_k, u_{N-1}).
struct RtiShiftParams {
    int64_t B;
    int N, n;               // 0 <= n <= N
    double h;
    const double* V_in;     // [B][NV]
    double* V_out;          // [B][NV], no overlap with V_in
    double* u_prev;         // [B][nu] or null: the old u_{n-1} (n >= 1)
    uint32_t copy_blocks;   // blocks 0 .. copy_blocks-1 copy, the rest roll out
};
constexpr int kRtiShiftThreads = 256, kRtiShiftPerThread = 4;
// blocks of the copy part (kRtiShiftThreads * kRtiShiftPerThread entries each) and of the roll-out (one lane per
// instance; none for n = 0)
inline uint64_t rti_shift_copy_blocks(int64_t B, int64_t NV) {
    const uint64_t per = kRtiShiftThreads * kRtiShiftPerThread;
    return (static_cast<uint64_t>(B) * NV + per - 1) / per;
}
inline uint64_t rti_shift_roll_blocks(int64_t B, int n) {
    return n > 0 ? (static_cast<uint64_t>(B) + kRtiShiftThreads - 1) / kRtiShiftThreads : 0;
}

// One launch, two kinds of block, which write disjoint entries of V_out and read V_in alone, so no order between
// them is needed.
// * Copy blocks: the B NV entries of V_out as one flat array, consecutive lanes on consecutive entries, so a wave
//   reads and writes whole cache lines whatever NV is (one lane per instance would stride by NV).  Each entry is
//   the old entry n K later in its own row, or the old u_{N-1}'s; the rolled-out states are skipped.  No FP64
//   arithmetic: the doubles move through registers bit for bit.
// * Roll-out blocks (n >= 1): one lane per instance, the serial chain of n Euler steps from the old x_N under the
//   old u_{N-1}, by the model's own device function; it also stores u_prev.  n nx doubles written per instance.
// A non-finite entry stays in its own row: no lane reads another instance's entries.
template <class Model>
__global__ __launch_bounds__(kRtiShiftThreads) void rti_shift_kernel(const RtiShiftParams p) {
    constexpr int NX = Model::NX, NU = Model::NU, K = NX + NU;
    const int N = p.N, n = p.n;
    const uint32_t NV = (uint32_t)NX * (N + 1) + (uint32_t)NU * N;
    const uint32_t kept = (uint32_t)(N - n) * K + NX;   // entries of a row that are old entries n K later
    if (blockIdx.x < p.copy_blocks) {
        const uint64_t total = (uint64_t)p.B * NV;
        const uint64_t base = (uint64_t)blockIdx.x * (kRtiShiftThreads * kRtiShiftPerThread) + threadIdx.x;
#pragma unroll
        for (int e = 0; e < kRtiShiftPerThread; ++e) {
            const uint64_t i = base + (uint64_t)e * kRtiShiftThreads;
            if (i >= total) break;
            uint64_t b;
            uint32_t j;
            if (total <= 0xffffffffull) {   // uniform: the 32-bit division is a fraction of the 64-bit one
                const uint32_t q = (uint32_t)i / NV;
                b = q;
                j = (uint32_t)i - q * NV;
            } else {
                b = i / NV;
                j = (uint32_t)(i - b * NV);
            }
            const double* const row = p.V_in + b * NV;
            if (j < kept) {
                p.V_out[i] = row[j + (uint32_t)n * K];
            } else {
                const uint32_t r = (j - kept) % K;   // kept = a stage's x done: r < NU is a control, the rest x
                if (r < NU) p.V_out[i] = row[(uint32_t)(N - 1) * K + NX + r];
            }
        }
        return;
    }
    const int64_t b = (int64_t)(blockIdx.x - p.copy_blocks) * kRtiShiftThreads + threadIdx.x;
    if (b >= p.B) return;
    const double* const row = p.V_in + b * NV;
    double* const out = p.V_out + b * NV;
    double x[NX], u[NU], xd[NX];
#pragma unroll
    for (int r = 0; r < NX; ++r) x[r] = row[(int64_t)N * K + r];
#pragma unroll
    for (int c = 0; c < NU; ++c) u[c] = row[(int64_t)(N - 1) * K + NX + c];
    if (p.u_prev) {
#pragma unroll
        for (int c = 0; c < NU; ++c) p.u_prev[b * NU + c] = row[(int64_t)(n - 1) * K + NX + c];
    }
    for (int k = N - n + 1; k <= N; ++k) {
        model_eval<Model>(x, u, xd);
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            x[r] = x[r] + p.h * xd[r];
            out[(int64_t)k * K + r] = x[r];
        }
    }
}

}  // namespace mmpc
