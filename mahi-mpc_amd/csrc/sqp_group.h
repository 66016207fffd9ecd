// sqp_group.h -- batched GN-SQP with a Riccati KKT solve, SIXTEEN LANES PER INSTANCE (four instances per wave).
//
// The condensed kernel (sqp_wave.h) spends O(N^2 nu^2 nx + (N nu)^3) flops per SQP iteration (288 kflop at
// cfg#2); a Riccati recursion solves the same GN QP exactly in O(N (nx+nu)^3) (~15 kflop at
// cfg#2).  The lane-per-instance Riccati kernel (sqp_lane.h) cannot fill the GPU at cfg#2's B = 4096 (64 waves),
// so here one instance owns a 16-lane DPP row and the work splits by its shape:
//   * stage-parallel (all 16 lanes, stage k on lane k mod 16): model + Jacobian evaluations, defects, merit
//     terms, line-search trial evaluations, iterate updates, loads and stores;
//   * O(N) recursions (one lane per instance): defect propagation d, adjoint + reduced gradient + Riccati
//     backward sweep, forward step sweep -- reading the stage blocks the other lanes left in LDS.
// Group reductions (J, |c|_1, max|c|, merit) are 16-lane butterflies; the NLP, merit, line search and stop test
// are those of sqp_wave.h / sqp_lane.h / oracle.  B = 4096 gives 1024 waves = one per SIMD.
//
// LDS per instance (fp64): x_k, u_k, d_k (then lam_k), dx_k, du_k, F_k, c_k, hFq_k, hFqd_k, hFu_k, the targets r_k
// (cross-lane data).  The gains K_k | kff_k go through a per-instance HBM workspace.  The exact-Hessian blocks W_k go
// there too, except in the unbounded solve of a model with a packed W record (WPack; the 2-link arm, cfg#2): its
// records stay in LDS, over d / lam, dx and du, which are dead from the W pass to the step sweep.
// This header includes itself once: the kernel body below is one text compiled into two __global__ templates (the
// kernels of the monotone barrier rule and sqp_group_mehrotra_kernel, at the end of the file), so that the former keep
// exactly the code they had before the second existed.  MMPC_GROUP_PASS: 1 = the whole header (first include), 2 = the
// body alone (the include inside sqp_group_mehrotra_kernel), 0 = a repeated include (nothing).
#undef MMPC_GROUP_PASS
#if defined(MMPC_GROUP_BODY_ONLY)
#define MMPC_GROUP_PASS 2
#elif !defined(MMPC_SQP_GROUP_H)
#define MMPC_SQP_GROUP_H
#define MMPC_GROUP_PASS 1
#else
#define MMPC_GROUP_PASS 0
#endif
#if MMPC_GROUP_PASS == 1
#include <type_traits>

#include "models.h"
#include "sqp_lane.h"
#include "sqp_wave.h"

namespace mmpc {

// Entries of W_k's x rows that Model::eval_hess always leaves 0 (structural zeros): on the workspace path a launch
// stores them in its first W pass only (round 6); the on-chip record (WPack) has no slot for them.  2-link arm
// (two_link_fast.h eval_hess: q_A enters only through gravity, the torques linearly): row 0 is zero in columns 2..5,
// rows 2 and 3 in columns 0, 4 and 5.
template <class Model>
__host__ __device__ constexpr bool w_struct_zero(int, int) { return false; }
template <>
__host__ __device__ constexpr bool w_struct_zero<TwoLinkArm>(int r, int j) { return (r == 0 && j >= 2) || (r >= 2 && (j == 0 || j >= 4)); }
// Packed record of the x rows of W_k for the on-chip W path of the unbounded exact-Hessian kernel (sqp_group_kernel,
// WLDS): PK doubles per stage, idx(r, j) = slot of W_k[r][j] (x row r, column j of (x, u)), -1 for a structural zero.
// PK = 0: the model has no packing and keeps the workspace path.  2-link arm: eval_hess writes W[i][j] and W[j][i]
// from one variable, so the 14 non-zero entries of the x rows are 10 distinct values.  The slot of W[r][j] is
// col(r) + col(j) with col = (0, 1, 2, 4, 6, 8): distinct over the 10 values, and a lane's row is then ONE address,
// record + col(r), plus the immediate offsets col(j) -- one address register for the sweep's six loads:
//   slot  0     1     2     3     4     5     6     7     8     9
//   W     [0][0] [0][1] [1][1] [1][2] [2][2] [1][3] [2][3] [1][4] [3][3] [1][5]
// A structural zero W[r][j] has no slot; read at col(r) + col(j) all the same (under a factor 0, sqp_group_kernel) it
// lands on another entry's slot or up to OVER = col(NX - 1) + col(NX + NU - 1) - (PK - 1) doubles past the record.
template <class Model>
struct WPack {
    static constexpr int PK = 0, OVER = 0;
    __host__ __device__ static constexpr int col(int) { return 0; }
    __host__ __device__ static constexpr int idx(int, int) { return -1; }
};
template <>
struct WPack<TwoLinkArm> {
    static constexpr int PK = 10, OVER = 3;
    __host__ __device__ static constexpr int col(int i) { return i < 3 ? i : 2 * (i - 1); }
    __host__ __device__ static constexpr int idx(int r, int j) {
        if (w_struct_zero<TwoLinkArm>(r, j)) return -1;
        return col(r) + col(j);
    }
};
// the additive slots are a packing: inside the record, and shared only by W[r][j] and W[j][r]
template <class Model>
__host__ __device__ constexpr bool wpack_valid() {
    using P = WPack<Model>;
    constexpr int NX = Model::NX, KZ = Model::NX + Model::NU;
    for (int r = 0; r < NX; ++r)
        for (int j = 0; j < KZ; ++j) {
            if (P::idx(r, j) < 0) continue;
            if (P::idx(r, j) >= P::PK || P::idx(r, j) != P::col(r) + P::col(j)) return false;
            for (int r2 = 0; r2 < NX; ++r2)
                for (int j2 = 0; j2 < KZ; ++j2)
                    if (P::idx(r2, j2) == P::idx(r, j) && !((r2 == r && j2 == j) || (r2 == j && j2 == r))) return false;
        }
    return P::OVER == P::col(NX - 1) + P::col(KZ - 1) - (P::PK - 1);
}
static_assert(wpack_valid<TwoLinkArm>(), "W record of the 2-link arm");
// first column whose structural zeros sit in the same x rows as column j's (j itself when there is none before it)
template <class Model>
__host__ __device__ constexpr int wpack_col_rep(int j) {
    for (int q = 0; q < j; ++q) {
        bool same = true;
        for (int r = 0; r < Model::NX; ++r) same = same && ((WPack<Model>::idx(r, q) < 0) == (WPack<Model>::idx(r, j) < 0));
        if (same) return q;
    }
    return j;
}
constexpr int kGroupLanes = 16;
constexpr int kGroupsPerWave = 4;

// LDS doubles per instance.  The hold targets (bounded solves) and the linear-mode block are only allocated
// when used: at cfg#2 that keeps a 4-instance workgroup at 40,384 B (bounded: 40,960 B), so 4 workgroups (one per
// SIMD) fit a CU's 160 KB.  nq = kinematic rows of the model (sqp_lane.h a_mul); the stage blocks are h da/dq,
// h da/dz, h da/du.  xb (the interior-point variant) adds nothing here since round 5: its per-stage z_l, z_u, Sigma,
// b, z_u - z_l live in the HBM workspace (group_ws_doubles) -- in LDS they made 67.8 KB per workgroup at cfg#2, two
// workgroups per CU, half the SIMDs idle and a 4096-instance batch in two rounds.
// The d recursion prefetches two stages ahead without a clamp (d_recursion_dist): its reads of stages N and N + 1 of
// sC, sFq and sFqd land in the arrays that follow each of them.  When the arrays after sFqd (sFu, sR, ...) are
// shorter than sFqd's overreach of 2 (nx - nq)^2 doubles (exo shapes at N = 1), a tail pad of that size keeps the read
// inside the instance's own block, never in the next group's block or past the end of the dynamic LDS; otherwise no
// pad (round 4 always padded: the control-bounded cfg#2 layout was then 40,960 B per workgroup).  The prefetched
// values are never used.  (A lane that reads the constant block below does so with stage stride 0 and overreaches
// nothing; the block sits last, after the pad, so the overreach of the other lanes still lands in front of it.)
// kc: doubles of the constant block that closes the instance's LDS in the kernels of a model with per-lane sweep
// operands (GroupLaneOps, below), [nx - 1 zeros | h | max(nx, nu) zeros].  Their serial sweeps read "this lane's row or
// column of A_k" through a per-lane address and a per-lane stage stride: a lane with the role points into the stage
// blocks, a q-lane's row h e_{nq+r} and the zero row of a lane without the role point here with stride 0 (cfg#2: 8
// doubles).
__host__ __device__ constexpr int group_const_doubles(int nx, int nu) {
    return nx + nu < kGroupLanes ? nx + (nx > nu ? nx : nu) : 0;
}
// kh: doubles of the head block in front of the constant block, K_k | kff_k of stages 0 .. 2 ([3][nu][nx + nu + 1]) in
// the unbounded kernels of a model with per-lane sweep operands: the step sweep opens with these rows a few hundred
// cycles after the Riccati sweep's last stages formed them, and from the workspace they came back at the latency of
// a load behind a store to the same line (cfg#2: 42 doubles, 40,384 B per workgroup).  The constant block stays last.
__host__ __device__ constexpr int group_head_doubles(int nx, int nu) { return 3 * nu * (nx + nu + 1); }
__host__ __device__ constexpr int group_lds_doubles(int nx, int nu, int nq, int N, bool bounded = true,
                                                   bool linear = true, bool xb = false, int kc = 0, int kh = 0) {
    return N * (3 * nx + (nx - nq) * (nq + (nx - nq) + nu) + 2 * nu) + 3 * (N + 1) * nx + (bounded ? N * nu : 0) +
           (linear ? (nx - nq) * (nq + (nx - nq) + nu) + nx : 0) +
           (N * ((nx - nq) * nu + nx) >= 2 * (nx - nq) * (nx - nq) ? 0 : 2 * (nx - nq) * (nx - nq)) + kh + kc;
}
// Models whose 16-lane kernels take the sweeps' lane operands through per-lane addresses, at the price of the constant
// block: the 2-link arm (cfg#2, whose kernel is bound by the issue slots of one wave).  The other models keep the
// FP64 blends against the lane-role factors and their LDS layout to the byte: the exo's block would be 16 doubles per
// instance, and LDS is what sizes its launches -- three of its groups share a 64 KB resume workgroup at N = 26 with 21
// bytes to spare (mmpc.hip tail_plan), and its kernels spill registers, so they are not bound by issue slots.
template <class Model>
struct GroupLaneOps {
    static constexpr int doubles = 0;
};
template <>
struct GroupLaneOps<TwoLinkArm> {
    static constexpr int doubles = group_const_doubles(TwoLinkArm::NX, TwoLinkArm::NU);
};
// exact Hessian (EXACT): per stage the x rows of W_k = h sum_s lam_{k+1,NQ+s} d^2 acc_s/d(x,u)^2 (nx x (nx+nu))
// and its u-u block (nu x nu), written stage-parallel and read by the lane-distributed Riccati sweep
__host__ __device__ constexpr int group_hess_doubles(int nx, int nu) { return nx * (nx + nu) + nu * nu; }
// HBM workspace doubles per instance: K_k | kff_k per stage, then the W_k blocks per stage, then (control-bounded
// solves only) the un-held rows [H_wx | -R | H_ww | h_w] of each stage QP, for the multipliers of the held controls.
// The kernel strides instances by its own variant's size (unbounded solves: 1020 instead of 1560 doubles at cfg#2);
// the host reserves the bounded size, the largest.
// xb (the interior-point variant, never with `bounded`): the per-stage z_l, z_u, Sigma, b, z_u - z_l of
// (x_{k+1} | u_k) after the W blocks, in place of the bounded solves' rows.
// w_onchip (the unbounded exact-Hessian kernel of a model with a packed W record, WPack): the W blocks stay in LDS, so
// the kernel strides instances by K | kff alone (420 doubles at cfg#2).
// The unbounded kernels of a model with per-lane sweep operands keep K | kff of stages 0 .. 2 in LDS (group_lds_doubles,
// kh) and leave those rows of the workspace unwritten; the control-bounded kernels (their LDS is at the budget), the
// interior-point kernels and the exo and generated models keep the workspace path for all rows.  The layout and what
// the host reserves are the same either way.
// mehr (the xb variant under Mehrotra's predictor-corrector rule): the per-bound corrector terms of (x_{k+1} | u_k),
// lower and upper, follow the xb fields; then per stage the record the predictor's Riccati sweep leaves for the
// corrector's vector-only sweep: 2 + nu doubles per lane (P~_x c, the b-independent part of p~, L^-1 [H_wx | -R]) and
// the Cholesky factor of H_ww with the b-independent part of h_w, once.
__host__ __device__ constexpr int group_ws_doubles(int nx, int nu, int N, bool bounded = true, bool xb = false,
                                                  bool w_onchip = false, bool mehr = false) {
    return N * nu * (nx + nu + 1) + (w_onchip ? 0 : N * group_hess_doubles(nx, nu)) +
           (bounded ? N * nu * (nx + 2 * nu + 1) : 0) + (xb ? 5 * N * (nx + nu) : 0) +
           (mehr ? 2 * N * (nx + nu) + N * ((2 + nu) * kGroupLanes + nu * (nu + 1) / 2 + nu) : 0);
}
// the cfg#2 shape (2-link arm, N = 30, unbounded): four instances per workgroup within 40,960 B of LDS, so that four
// workgroups (one per SIMD) fit a CU -- the on-chip W record lives in arrays that are dead while it is alive and adds
// nothing to this
static_assert(kGroupsPerWave * group_lds_doubles(4, 2, 2, 30, false, false, false, GroupLaneOps<TwoLinkArm>::doubles,
                                                 group_head_doubles(4, 2)) * 8 <= 40960,
              "cfg#2 LDS budget");

struct GroupWork {
    double* ws;
};

// Reductions over one 16-lane row (= one instance group): a butterfly of DPP row rotations by 8, 4, 2, 1 (two
// v_mov_b32_dpp row_ror and the FP64 operation per step; no LDS access -- the __shfl_xor butterfly they replace was two
// ds_bpermute_b32 and an LDS round trip per step).  Values: after the step with offset o every lane's value has period
// 2 o over the row, so the lane o places round holds what lane i ^ o holds, and each lane forms op(own, partner) with
// the xor butterfly's operands in the xor butterfly's order: the results are its results bit for bit.
// Every call is group-uniform: all 16 lanes of the row are active (bound_ctrl would hand an inactive lane's partner a
// zero).  Checked at every call site of sqp_group.h and gain_sweep.h: each sits under conditions on template flags,
// launch parameters, the iteration count and values that are themselves group reductions or computed redundantly on
// every lane (evalA / fwd_ready, resolve, fact_ok, the line search's tests), never under a lane or stage test; groups
// of one wave may diverge from each other, which a row operation does not see.
template <int O>
__device__ __forceinline__ double row_ror(double v) {
    static_assert(O >= 1 && O < 16, "row rotation");
    return __builtin_amdgcn_update_dpp(v, v, 0x120 + O, 0xf, 0xf, true);
}
__device__ __forceinline__ double group_sum(double v) {
    v += row_ror<8>(v);
    v += row_ror<4>(v);
    v += row_ror<2>(v);
    v += row_ror<1>(v);
    return v;
}
__device__ __forceinline__ double group_min(double v) {
    v = fmin(v, row_ror<8>(v));
    v = fmin(v, row_ror<4>(v));
    v = fmin(v, row_ror<2>(v));
    v = fmin(v, row_ror<1>(v));
    return v;
}
__device__ __forceinline__ double group_max(double v) {
    v = fmax(v, row_ror<8>(v));
    v = fmax(v, row_ror<4>(v));
    v = fmax(v, row_ror<2>(v));
    v = fmax(v, row_ror<1>(v));
    return v;
}
__device__ __forceinline__ double group_bcast(double v, int base) { return __shfl(v, base); }
__device__ __forceinline__ int group_bcast_i(int v, int base) { return __shfl(v, base); }

// Lane L of every 16-lane row (= one instance group) to the whole row: one v_mov_b64_dpp row_newbcast:L
// (gfx950 DPP64).  Measured on MI355X (tools/ubench/f64_latency.hip): a dependent FMA through it costs
// 17 cycles against 11 for a plain dependent FMA and ~80 through __shfl (ds_bpermute) or an LDS round trip,
// so the lane-distributed Riccati sweep below exchanges data with it.
template <int L>
__device__ __forceinline__ double row_bcast(double v) {
    static_assert(L >= 0 && L < 16, "row lane");
    // bound_ctrl with full row/bank masks: every lane is written, so the old value is dead (no copy)
    return __builtin_amdgcn_update_dpp(v, v, 0x150 + L, 0xf, 0xf, true);
}
// compile-time loop: f(std::integral_constant<int, I>) for I = B .. E-1 (row_bcast needs a constant lane)
template <int B, int E, class F>
__device__ __forceinline__ void sfor(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        sfor<B + 1, E>(static_cast<F&&>(f));
    }
}

// xd = f(x, u); with jac also the acceleration partials (unscaled).  Linear mode (ModelGenerator.cpp:47-48):
// F_lin with the acceleration Jacobians lFq, lFqd, lFu and xdot lxd taken at (lxs, lus).
template <class Model>
__device__ __forceinline__ void group_model(bool lin, const double* lFq, const double* lFqd, const double* lFu,
                                            const double* lxd, const double* lxs, const double* lus, const double* x,
                                            const double* u, double* xd, double* Fq, double* Fqd, double* Fu,
                                            bool jac) {
    constexpr int NQ = Model::NQ, NU = Model::NU, NA = Model::NX - NQ;
    if (!lin) {
        if (jac) {
            Model::eval_acc_jac(x, u, xd + NQ, Fq, Fqd, Fu);
#pragma unroll
            for (int i = 0; i < NQ; ++i) xd[i] = x[NQ + i];
        } else {
            Model::eval(x, u, xd);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) xd[i] = lxd[i] + (x[NQ + i] - lxs[NQ + i]);
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        double t = lxd[NQ + i];
#pragma unroll
        for (int s = 0; s < (NQ > NA ? NQ : NA); ++s) {
            if (s < NA) t = fma(lFqd[i * NA + s], x[NQ + s] - lxs[NQ + s], t);
            if (s < NQ) t = fma(lFq[i * NQ + s], x[s] - lxs[s], t);
        }
#pragma unroll
        for (int c = 0; c < NU; ++c) t = fma(lFu[i * NU + c], u[c] - lus[c], t);
        xd[NQ + i] = t;
    }
    if (jac) {
#pragma unroll
        for (int i = 0; i < NA * NQ; ++i) Fq[i] = lFq[i];
#pragma unroll
        for (int i = 0; i < NA * NA; ++i) Fqd[i] = lFqd[i];
#pragma unroll
        for (int i = 0; i < NA * NU; ++i) Fu[i] = lFu[i];
    }
}

// The model at the W stages of a pair (PAIR, sqp_group_kernel): x, u, xd and the blocks per stage [e].  W = 1 is
// group_model itself, with its run-time `lin` (LM < 0).  W > 1 takes `lin` as the constant LM, hoisted out of the stage
// loop by the caller (as a branch inside the body it would split the pair's block and keep the chains apart): LM = 0
// evaluates the model once on dpack<W> values, so the W chains alternate operation by operation (two_link_fast.h);
// LM = 1 is the linear-mode branch of group_model per stage.  Stage e gets group_model's values bit for bit.
template <class Model, int W, int LM, bool JAC, int SQ, int FD, int FU>
__device__ __forceinline__ void group_model_w(bool lin, const double* lFq, const double* lFqd, const double* lFu,
                                              const double* lxd, const double* lxs, const double* lus,
                                              const double (*x)[Model::NX], const double (*u)[Model::NU],
                                              double (*xd)[Model::NX], double (*Fq)[SQ], double (*Fqd)[FD],
                                              double (*Fu)[FU]) {
    constexpr int NX = Model::NX, NQ = Model::NQ, NU = Model::NU, NA = NX - NQ;
    if constexpr (W == 1 || LM != 0) {
#pragma unroll
        for (int e = 0; e < W; ++e)
            group_model<Model>(W == 1 ? lin : true, lFq, lFqd, lFu, lxd, lxs, lus, x[e], u[e], xd[e], JAC ? Fq[e] : nullptr,
                               JAC ? Fqd[e] : nullptr, JAC ? Fu[e] : nullptr, JAC);
    } else {
        using T = dpack<W>;
        T xw[NX], uw[NU], xdw[NX];
#pragma unroll
        for (int e = 0; e < W; ++e) {
#pragma unroll
            for (int i = 0; i < NX; ++i) xw[i].v[e] = x[e][i];
#pragma unroll
            for (int i = 0; i < NU; ++i) uw[i].v[e] = u[e][i];
        }
        if constexpr (JAC) {
            T fq[SQ], fqd[FD], fu[FU];
            Model::eval_acc_jac(xw, uw, xdw + NQ, fq, fqd, fu);
#pragma unroll
            for (int e = 0; e < W; ++e) {
#pragma unroll
                for (int i = 0; i < NQ; ++i) xd[e][i] = x[e][NQ + i];
#pragma unroll
                for (int i = 0; i < NA; ++i) xd[e][NQ + i] = xdw[NQ + i].v[e];
#pragma unroll
                for (int i = 0; i < NA * NQ; ++i) Fq[e][i] = fq[i].v[e];
#pragma unroll
                for (int i = 0; i < FD; ++i) Fqd[e][i] = fqd[i].v[e];
#pragma unroll
                for (int i = 0; i < FU; ++i) Fu[e][i] = fu[i].v[e];
            }
        } else {
            Model::eval(xw, uw, xdw);
#pragma unroll
            for (int e = 0; e < W; ++e)
#pragma unroll
                for (int i = 0; i < NX; ++i) xd[e][i] = xdw[i].v[e];
        }
    }
}

// XB: state bounds (oracle solve_one_ip), the primal-dual interior-point variant for state AND control bounds;
// BOUNDED: control bounds only (projected GN-SQP).  At most one of them.
// EXACT: exact Hessian of the Lagrangian (mmpc_opts.hessian; oracle ORACLE_HESS_EXACT) -- solves of models with
// second derivatives on the lane-distributed path: unbounded, control-bounded (held controls fixed in the exact QP)
// and, round 6, state-bounded (W_k joins the barrier-augmented stage blocks; oracle solve_one_ip with the exact
// Hessian).
// MEHR (XB only): Mehrotra's predictor-corrector barrier rule (mmpc_set_barrier_rule; oracle solve_one_ip, rule 1) in
// place of the monotone update.  Each iteration solves the stage QPs twice with one set of matrices: the affine
// predictor (barrier gradient b = 0) gives the step to the boundary, from which the target mu_t = sigma mu with
// sigma = (mu_aff / mu)^3 and the per-bound second-order terms -ds_aff dz_aff follow; the corrector solves with
// b = -(mu_t - ds dz)_l / s_l + (mu_t - ds dz)_u / s_u.  Dual steps, merit and the kappa_Sigma safeguard use mu_t and
// the corrected terms; there is no lagged update.  Every MEHR statement sits behind `if constexpr`, and the kernels
// of the monotone rule are sqp_group_kernel's, with their names and code unchanged.
// The body is shared with sqp_group_mehrotra_kernel (end of the file), which sets BOUNDED = false, XB = true, MEHR = true.
template <class Model, bool BOUNDED = false, bool XB = false, bool EXACT = false>
__global__ __launch_bounds__(64) void sqp_group_kernel(SolveParams p, GroupWork gw) {
    constexpr bool MEHR = false;
    constexpr bool IB = false;   // shared control bounds; per-instance rows: sqp_group_instb_kernel (end of the file)
#endif  // MMPC_GROUP_PASS == 1
#if MMPC_GROUP_PASS != 0   // ---- the kernel body: Model, BOUNDED, XB, EXACT, MEHR, p, gw in scope ----
    static_assert(!(BOUNDED && XB), "the interior-point variant handles the control bounds itself");
    static_assert(!MEHR || XB, "the barrier rule belongs to the interior-point variant");
    constexpr int NX = Model::NX, NU = Model::NU, NQ = Model::NQ, NA = NX - NQ, NS = NX + NU, ND = NX + NU;
    constexpr int SQ = NA * NQ > 0 ? NA * NQ : 1;  // extent of the h da/dq block (empty for NQ = 0)
    constexpr int FQ = NA * NQ, FD = NA * NA, FU = NA * NU;  // stage block sizes (sqp_lane.h a_mul)
    static_assert(NQ >= 0 && NA >= NQ, "x = [q; z] with qdot = z[0:NQ]");
    constexpr int G = kGroupLanes;
    extern __shared__ double shm[];
    const int gl = threadIdx.x & (G - 1);
    const int gi = threadIdx.x / G;
    [[maybe_unused]] const int lane0 = threadIdx.x;
    MMPC_PHASE_DECL
    const int gbase = gi * G;  // first lane of this instance's group
    // slot of this group in the launch: the instance itself, or (resume launch, p.tail_idx) an entry of the lane
    // kernel's hand-over list
    const int64_t slot = (int64_t)blockIdx.x * p.gpw + gi;
    const bool resume = p.tail_idx != nullptr;
    const bool valid = gi < p.gpw && slot < (resume ? (int64_t)min(*p.tail_count, p.tail_slots) : p.B);
    // a group past the end of the batch (the last wave of a B not divisible by 4) leaves at once: no group reads
    // another group's lanes (row_bcast and the group reductions stay inside the 16-lane row) or LDS block, so
    // nothing else in the wave needs it, and it issues no memory access at all (round 4 had those groups run on
    // aliased to instance 0 and masked by `done`, which made every store's masking a correctness condition)
    if (!valid) return;
    const int64_t inst = resume ? (int64_t)p.tail_idx[slot] : slot;
    const int64_t ii = inst;
    const int N = p.N;
    const int NV = NX * (N + 1) + NU * N;
    const double h = p.h;

    // ---- LDS views of this instance ----
    // constant block of the per-lane sweep operands (LOPS, below): the models with GroupLaneOps, lane-distributed path
    constexpr int KC = NX + NU < kGroupLanes ? GroupLaneOps<Model>::doubles : 0;
    // head block of the gain record (group_lds_doubles): the unbounded kernels of those models
    constexpr int KH = (KC > 0 && !BOUNDED && !XB) ? group_head_doubles(NX, NU) : 0;
    double* const sX = shm + gi * group_lds_doubles(NX, NU, NQ, N, BOUNDED, p.is_linear != 0, XB, KC, KH);  // [N+1][NX]
    // sD | sDX | sDU are contiguous: between the W pass and the step sweep of an iteration all three are dead (d / lam
    // in sD: the W pass is its last reader; sDX, sDU: the previous step, consumed by the update) and, on the on-chip W
    // path (WLDS), sD + NX .. holds the packed W records (sW) -- d_0 = 0 in sD[0..NX) stays
    double* const sU = sX + (N + 1) * NX;                          // [N][NU]
    double* const sD = sU + N * NU;                                // [N+1][NX]
    double* const sDX = sD + (N + 1) * NX;                         // [N+1][NX]
    double* const sDU = sDX + (N + 1) * NX;                        // [N][NU]
    double* const sF = sDU + N * NU;                               // [N][NX]
    double* const sC = sF + N * NX;                                // [N][NX]
    double* const sFq = sC + N * NX;                               // [N][NA*NQ]   h da/dq
    double* const sFqd = sFq + N * FQ;                             // [N][NA*NA]   h da/dz
    double* const sFu = sFqd + N * FD;                             // [N][NA*NU]   h da/du
    double* const sR = sFu + N * FU;                               // [N][NX]      targets r_k
    double* const sHold = sR + N * NX;                             // [N][NU]      bound a control is held at
    double* const sLin = sHold + (BOUNDED ? N * NU : 0);           // linear mode: Fq | Fqd | Fu | xdot
    constexpr int NY = NX + NU;
    // On-chip W path: the unbounded exact-Hessian solve of a control-affine model with a packed W record that fits the
    // dead arrays (PK <= 2 NX + NU per stage; PK >= NX for the W pass's write order, below).  It solves the QP once per
    // iteration, with no step sweep between the W pass and the Riccati sweep; the control-bounded and interior-point
    // variants solve it again after step sweeps that rewrite sDX, sD and sDU, and keep W in the workspace.
    constexpr int PK = WPack<Model>::PK;
    constexpr bool WLDS = EXACT && !BOUNDED && !XB && IsControlAffine<Model>::value && PK >= NX && PK <= 2 * NX + NU;
    double* const wK = gw.ws + slot * (int64_t)group_ws_doubles(NX, NU, N, BOUNDED, XB, WLDS, MEHR);  // [N][NU][NS+1]
    constexpr int KZ = NX + NU, HW = group_hess_doubles(NX, NU);
    double* const wH = wK + N * NU * (NS + 1);  // EXACT: [N][HW] = W_k x rows [NX][KZ] | W_k uu block [NU][NU]
    double* const sW = sD + NX;                 // WLDS: [N][PK] packed W_k x rows, over sD[1..], sDX and sDU
    // WLDS: the sweep's loads of the last record's structural zeros reach the OVER doubles behind it (WPack).  Those
    // lie inside sDX | sDU (OVER <= NX and PK <= 2 NX + NU): zeroed here for the first iteration, and from then on a
    // step of the previous iteration, finite whenever the iteration goes on to its Riccati sweep -- the line search
    // accepts a non-finite step only into an iterate that the next stop test leaves with ST_NONFINITE.
    static_assert(!WLDS || WPack<Model>::OVER <= NX, "the over-read of the last W record stays inside sDU");
    if constexpr (WLDS) {
        if (gl < WPack<Model>::OVER) sW[N * PK + gl] = 0.0;
    }
    constexpr int NR = NS + NU + 1;             // BOUNDED: [N][NU][NR] = un-held [H_wx | -R | H_ww | h_w] rows
    double* const wRel = wH + N * HW;
    bool w_zeros_stored = false;   // W_k's structural zeros are in the workspace (this launch's first W pass stored them)
    // interior point (XB): per stage k, y = (x_{k+1} | u_k) [NY]: duals z_l, z_u, Sigma, b, z_u - z_l -- in the HBM
    // workspace after the W blocks (group_lds_doubles); the stage-parallel phases write them, the serial sweeps read
    // them on other lanes after a workgroup fence
    double* const sZl = wRel;  // [N][NY]
    double* const sZu = sZl + N * NY;
    double* const sSg = sZu + N * NY;
    double* const sBb = sSg + N * NY;
    double* const sZg = sBb + N * NY;
    // MEHR: corrector terms mu_t - ds_aff dz_aff of the lower / upper bounds, written and read by the stage's own lane
    [[maybe_unused]] double* const sCl = sZg + N * NY;   // [N][NY]
    [[maybe_unused]] double* const sCu = sCl + N * NY;
    // MEHR: what the predictor's Riccati sweep (backward_dist) leaves per stage for the corrector's vector-only sweep
    // (backward_vec).  Per lane r [VL][G]: pc = P~_{k+1,x} row r . c_k, pn0 = the b-independent part of row r of p~_k,
    // Ytil[NU] = column r of L^-1 [H_wx | -R]; once [VS]: L row by row with 1 / L_aa on the diagonal, then the
    // b-independent part of h_w (bit-identical on every lane: each lane stores and reads them)
    constexpr int VL = 2 + NU, VC = NU * (NU + 1) / 2, VS = VC + NU, VR = VL * G + VS;
    [[maybe_unused]] double* const sVr = sCu + N * NY;   // [N][VR]
    const double* const trg = p.traj + ii * (int64_t)N * NX;

    // two stages per lane in the stage-parallel phases (at FUSE_FWD, below)
    constexpr bool PAIR = HasWideEval<Model>::value && !BOUNDED && !XB;
    constexpr int WD = PAIR ? 2 : 1;
    // width of phase A, of the fused trial and of the W pass (1 takes one of them back to its one-stage loop)
    constexpr int WA = WD, WJ = WD, WW = WD;
    const double* w = p.weights + ii * p.w_stride;
    double Q[NX], R[NU], Rm[NU], up[NU];
#pragma unroll
    for (int r = 0; r < NX; ++r) Q[r] = w[r];
#pragma unroll
    for (int c = 0; c < NU; ++c) {
        R[c] = w[NX + c];
        Rm[c] = w[NX + NU + c];
        up[c] = p.u_prev[ii * NU + c];
    }
    double lbv[NU], ubv[NU];
    load_bounds<NU, BOUNDED, IB>(p, inst, lbv, ubv);
    // PAIR: the prologue in one round trip.  Every global load of the lane is issued here, behind the weights and u_prev
    // and before anything waits for one of them: x_0, and for the lane's first pair of stages (gl and gl + G: the whole
    // horizon up to N = 2 G - 1) the targets and, unless the start is zero, V.  The LDS stores and the per-lane
    // constants derived from the weights follow.  The uniform init_zero test is taken once, around the loads; a stage
    // index past the horizon is clamped (k to the lane's first stage, the u / target row of k = N to N - 1), so the
    // loads need no lane test and a repeated store writes the value already there.
    [[maybe_unused]] double px0[NX], pxv[WD][NX], puv[WD][NU], prv[WD][NX];
    // (a lane past the end of a short horizon, gl > N, loads stage N's values and stores nothing)
    [[maybe_unused]] auto pro_k = [&](int k0, int e) { return k0 + e * G <= N ? k0 + e * G : (k0 <= N ? k0 : N); };
    [[maybe_unused]] auto pro_load = [&](int k0, double (*xv)[NX], double (*uv)[NU], double (*rv)[NX]) {
        const double* Vin = p.V + ii * (int64_t)NV;
#pragma unroll
        for (int e = 0; e < WD; ++e) {
            const int k = pro_k(k0, e), ku = k < N ? k : N - 1;
#pragma unroll
            for (int r = 0; r < NX; ++r) rv[e][r] = trg[ku * NX + r];
        }
        if (p.init_zero) {
#pragma unroll
            for (int e = 0; e < WD; ++e) {
#pragma unroll
                for (int r = 0; r < NX; ++r) xv[e][r] = 0.0;
#pragma unroll
                for (int c = 0; c < NU; ++c) uv[e][c] = 0.0;
            }
        } else {
#pragma unroll
            for (int e = 0; e < WD; ++e) {
                const int k = pro_k(k0, e), ku = k < N ? k : N - 1;
#pragma unroll
                for (int r = 0; r < NX; ++r) xv[e][r] = Vin[k * ND + r];
#pragma unroll
                for (int c = 0; c < NU; ++c) uv[e][c] = Vin[ku * ND + NX + c];
            }
        }
    };
    if constexpr (PAIR) {
#pragma unroll
        for (int r = 0; r < NX; ++r) px0[r] = p.x0[ii * NX + r];
        pro_load(gl, pxv, puv, prv);
    }
    // ---- lane-distributed Riccati (DIST): lane r of the group owns row r of the augmented value function
    //      P~ (NS x NS) and of every per-row quantity; small per-stage quantities are computed redundantly on
    //      all lanes; rows are exchanged with row_bcast.  Control bounds (BOUNDED) run the same
    //      sweeps with the held controls of the projected SQP folded into the per-stage quantities; state bounds
    //      (XB) add the barrier terms and use the Cholesky (Y^T Y) form of the stage update.  Models with
    //      nx + nu >= 16 keep the one-lane sweep below. ----
    constexpr bool DIST = (NS < G);
    static_assert(!MEHR || DIST, "Mehrotra's rule: lane-distributed path");
    // control-affine model: the u-u block of the exact-Hessian W_k is zero -- neither stored, loaded nor added
    constexpr bool CAFF = IsControlAffine<Model>::value;
    static_assert(!EXACT || (DIST && HasHess<Model>::value), "exact Hessian: lane-distributed path, model eval_hess");
    const int r = gl;
    const bool lx = r < NX, lu = r >= NX && r < NS, la = r >= NQ && r < NX;
    const int rx = lx ? r : 0;                        // x row of this lane (clamped for address arithmetic)
    const int ru = lu ? r - NX : 0;                   // u row
    const int ta = la ? r - NQ : 0;                   // row of the a-blocks (hFq, hFqd, hFu) of an a-lane
    const double Qr = lx ? w[rx] : 0.0;               // Q of this lane's x row
    // lane-role masks as blend factors, for the models whose row / column of A is not a per-lane load (LOPS, ACOLP,
    // below): their DIST loops blend loaded values with FMAs instead of selects (a select of an LDS load becomes a
    // branch or a pointer select)
    [[maybe_unused]] const double lqd = r < NQ ? 1.0 : 0.0, lad = la ? 1.0 : 0.0;
    // x-lane factor for the sweeps' per-stage masking: one FP64 multiply where a 64-bit select is two cndmasks (the
    // masked values are finite sums of this instance's own data, so 0 * v == 0)
    const double lxf = lx ? 1.0 : 0.0;
    // WLDS: W_k[r][j] sits at slot wrow + col(j) of the packed record, wrow = col(r) this lane's one row offset (a lane
    // without an x row: row 0), and wm[j] is its blend factor.  A structural zero, and every column of a lane without
    // an x row, reads its additive slot all the same -- another entry of this record, or up to OVER doubles past it, all
    // finite (sW, below) -- under a factor 0; the factor takes the place of the x-lane factor at the uses of W, so the
    // sweep gains no select; columns with the same zero pattern share one factor.
    int wrow = 0;
#pragma unroll
    for (int r2 = 0; r2 < NX; ++r2)
        if (lx && r == r2) wrow = WPack<Model>::col(r2);
    double wm[KZ];
#pragma unroll
    for (int j = 0; j < KZ; ++j) {
        bool nz = false;
#pragma unroll
        for (int r2 = 0; r2 < NX; ++r2)
            if (lx && r == r2 && WPack<Model>::idx(r2, j) >= 0) nz = true;
        wm[j] = wpack_col_rep<Model>(j) < j ? wm[wpack_col_rep<Model>(j)] : (nz ? 1.0 : 0.0);
    }
    const int rq = r < NQ ? r : 0;                    // q column of a q-lane (clamped)
    const double Rr = lu ? w[NX + ru] : 0.0;          // R of this lane's u row
    double dgx[NS];                                    // XB: this x-lane's diagonal entry of P~ (barrier Sigma)
#pragma unroll
    for (int j = 0; j < NS; ++j) dgx[j] = (lx && j == r) ? 1.0 : 0.0;
    double lbr = -INFINITY, ubr = INFINITY;            // bounds of this u-lane's control (BOUNDED)
#pragma unroll
    for (int c = 0; c < NU; ++c)
        if (lu && ru == c) {
            lbr = lbv[c];
            ubr = ubv[c];
        }
    double hq[NQ > 0 ? NQ : 1], hrow[NX], qoh[NX], rdg[NU];
#pragma unroll
    for (int z = 0; z < NQ; ++z) hq[z] = (r == NQ + z) ? h : 0.0;   // column r of A holds h in row z (kinematics)
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        hrow[j] = (r < NQ && j == NQ + r) ? h : 0.0;  // row r of A of a q-lane (besides the identity); blended where !LOPS
        qoh[j] = (j == r) ? Qr : 0.0;
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) rdg[c] = (r == NX + c) ? R[c] : 0.0;
    // LOPS (models with GroupLaneOps): this lane's row and column of A_k as LDS operands of the serial sweeps -- an address and a stage stride
    // (bytes) per operand, both fixed for the launch.  A lane with the role reads the stage blocks (stride = block size);
    // a q-lane's row h e_{NQ+r} and the zero row / column of a lane without the role are read from the constant block
    // sKc = [NX - 1 zeros | h | max(NX, NU) zeros] with stride 0.  The loads are unconditional and deliver what the
    // blends fma(lad, v, hrow) / lad v + lqd v' delivered (1 v + 0, or 0 v + h with v finite), without the FP64
    // instructions -- the same idiom as the W slots (wrow): per-lane addresses, never a select of a loaded value.
    constexpr bool LOPS = KC > 0;
    double* const sKc = sX + group_lds_doubles(NX, NU, NQ, N, BOUNDED, p.is_linear != 0, XB, KC, KH) - KC;
    [[maybe_unused]] double* const sKh = sKc - KH;   // [3][NU][NS+1]: K_k | kff_k of stages 0 .. 2
    // (the addresses are LDS pointers, so that the base of the dynamic LDS is added here once and not at every load)
    using LdsB = const __attribute__((address_space(3))) char*;
    using LdsD = const __attribute__((address_space(3))) double*;
    const LdsB shb = (LdsB)shm;
    auto lds = [](LdsB b) { return *(LdsD)b; };
    // a running address, opaque to the loop optimiser: one add per stage and immediate offsets from it (left alone,
    // strength reduction gives every unrolled copy of a load its own induction variable)
    auto pin = [](LdsB& b) { asm volatile("" : "+v"(b)); };
    [[maybe_unused]] const LdsB iKc = shb + 8 * (int)(sKc - shm), iKz = iKc + 8 * NX;   // the block; its zero row (max(NX, NU) zeros)
    // row r of [A - I | B]: a-lanes [hFq | hFqd | hFu] row r - NQ, q-lanes h e_{NQ+r} | 0.
    // MIRROR: a lane without an x row takes row 0's operands (rx = 0: the addresses of lane 0, a q-lane) in the d
    // recursion, the adjoint and the step sweep, so it carries lane 0's chain bit for bit (same instructions, same
    // operands, same broadcasts) and the sweeps store without a lane mask: its stores go to lane 0's address with lane
    // 0's value.  It never reaches another group: every address is this instance's own.  (The u-lanes of the step sweep
    // keep their own chain; see there.)  Without MIRROR such a lane reads the zero row and its stores stay masked.
    constexpr bool MIRROR = LOPS && NQ > 0 && NQ == NA && (NA - 1) * NA < KC;   // (= ACOLP, below)
    [[maybe_unused]] const double Qa = MIRROR ? w[rx] : Qr;   // Q of the x row whose chain the lane carries in the adjoint
    [[maybe_unused]] const LdsB iAq =
        la ? shb + 8 * ((int)(sFq - shm) + ta * NQ) : ((r < NQ || MIRROR) ? iKc + 8 * ((NX - 1) - (NQ + rq)) : iKz);
    [[maybe_unused]] const int zAq = la ? 8 * FQ : 0, zAd = la ? 8 * FD : 0, zBr = la ? 8 * FU : 0;
    [[maybe_unused]] const LdsB iAd = la ? shb + 8 * ((int)(sFqd - shm) + ta * NA) : ((r < NQ || MIRROR) ? iAq + 8 * NQ : iKz);
    [[maybe_unused]] const LdsB iBr = la ? shb + 8 * ((int)(sFu - shm) + ta * NU) : iKz;
    // column r of A's a-rows: a-lanes hFqd[:, r - NQ], q-lanes hFq[:, r], other lanes 0.  With NQ == NA both kinds of
    // column have the element stride NA, an immediate; a lane without the role reads the block from its start, where
    // the offsets t NA (t < NA) are zeros (they never meet h at NX - 1 = 2 NA - 1).  Other shapes keep the blend.
    constexpr bool ACOLP = LOPS && NQ == NA && (NA - 1) * NA < KC;
    static_assert(!MIRROR || ACOLP, "a mirrored lane reads row 0's column through the per-lane column address");
    [[maybe_unused]] const int zAc = (la || r < NQ) ? 8 * FD : 0;
    [[maybe_unused]] const LdsB iAc = la ? shb + 8 * ((int)(sFqd - shm) + ta) : (r < NQ ? shb + 8 * ((int)(sFq - shm) + rq) : iKc),
                                iAcN = iAc + (N - 1) * zAc;   // ... at the last stage
    if constexpr (LOPS) {
        for (int i = gl; i < KC; i += G) sKc[i] = (i == NX - 1) ? h : 0.0;
    }
    // ---- load: V (reference layout) -> LDS, x_0 pinned (ModelControl.cpp:144-145) ----
    if constexpr (PAIR) {
        // the first pair's values are in flight since the top (pro_load); a horizon of more than two rounds loads its
        // further pairs here, one round trip each
        const bool hold = p.init_hold != 0;
        for (int k0 = gl; k0 <= N; k0 += WD * G) {
            if (k0 != gl) pro_load(k0, pxv, puv, prv);
#pragma unroll
            for (int e = 0; e < WD; ++e) {
                const int k = pro_k(k0, e), ku = k < N ? k : N - 1;
#pragma unroll
                for (int r = 0; r < NX; ++r) sX[k * NX + r] = (k == 0 || hold) ? px0[r] : pxv[e][r];
#pragma unroll
                for (int c = 0; c < NU; ++c) sU[ku * NU + c] = puv[e][c];
#pragma unroll
                for (int r = 0; r < NX; ++r) sR[ku * NX + r] = prv[e][r];
            }
        }
    } else {
        const double* Vin = p.V + ii * (int64_t)NV;
        for (int k = gl; k <= N; k += G) {
#pragma unroll
            for (int r = 0; r < NX; ++r)
                sX[k * NX + r] = (k == 0 || p.init_hold) ? p.x0[ii * NX + r] : (p.init_zero ? 0.0 : Vin[k * ND + r]);
            if (k < N) {
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    const double v = p.init_zero ? 0.0 : Vin[k * ND + NX + c];
                    sU[k * NU + c] = BOUNDED ? proj(v, lbv[c], ubv[c]) : v;
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) sR[k * NX + r] = trg[k * NX + r];
            }
        }
    }
    const double* const tr = sR;
    double yl[XB ? NY : 1], yu[XB ? NY : 1];
    double mub = (XB && resume) ? p.tail_mub[slot] : kIpMu0;  // barrier parameter (f = J/2 scale)
    if constexpr (XB) {
        load_ip_bounds<NX, NU, IB>(p, inst, yl, yu);
        __builtin_amdgcn_wave_barrier();
        if (resume) {   // the handed-over duals, from the lane launch's workspace (the iterate is interior already)
            const double* const lz = p.tail_lws + (inst >> 6) * p.tail_lws_block + (inst & 63);
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NY; ++j) {
                    sZl[k * NY + j] = lz[((int64_t)k * p.tail_lws_ss + p.tail_lws_zl + j) * 64];
                    sZu[k * NY + j] = lz[((int64_t)k * p.tail_lws_ss + p.tail_lws_zl + NY + j) * 64];
                }
            }
        } else {
            // y pushed into the interior, z = 1 on finite bounds (oracle solve_one_ip)
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NY; ++j) {
                    double& y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    y = ip_push(y, yl[j], yu[j]);
                    sZl[k * NY + j] = yl[j] > -INFINITY ? 1.0 : 0.0;
                    sZu[k * NY + j] = yu[j] < INFINITY ? 1.0 : 0.0;
                }
            }
        }
    }
    // linear mode: acceleration Jacobians and xdot at (x_0, u_prev) (ModelControl.cpp:125-135), in LDS (keeps
    // 20-64 VGPRs free for the serial Riccati sweep); the linearisation point x_0 is sX[0..NX) (pinned)
    const bool lin = p.is_linear != 0;
    double* const lFq = sLin;
    double* const lFqd = lFq + FQ;
    double* const lFu = lFqd + FD;
    double* const lxd = lFu + FU;
    const double* const lxs = sX;
    if (lin && gl == 0) {
        double acc[NA], x[NX], Fq[SQ], Fqd[FD], Fu[FU];
#pragma unroll
        for (int r = 0; r < NX; ++r) x[r] = p.x0[ii * NX + r];
        Model::eval_acc_jac(x, up, acc, Fq, Fqd, Fu);
#pragma unroll
        for (int i = 0; i < FQ; ++i) lFq[i] = Fq[i];
#pragma unroll
        for (int i = 0; i < FD; ++i) lFqd[i] = Fqd[i];
#pragma unroll
        for (int i = 0; i < FU; ++i) lFu[i] = Fu[i];
#pragma unroll
        for (int i = 0; i < NQ; ++i) lxd[i] = x[NQ + i];
#pragma unroll
        for (int i = 0; i < NA; ++i) lxd[NQ + i] = acc[i];
    }
    __builtin_amdgcn_wave_barrier();
    int status = ST_MAX_ITER;
    int it = 0;
    double kkt = 0.0, mu = resume ? p.tail_mu[slot] : 0.0, pg_prev = (BOUNDED && resume) ? p.tail_mub[slot] : INFINITY;
    bool done = !valid;
    // FUSE_FWD: the line search's alpha = 1 trial evaluates the model with its Jacobian and writes everything phase A
    // computes at that point (F_k, c_k, the stage blocks; J, |c|_1, max|c|); when the full step is accepted (every
    // cfg#2 iteration, tools/alpha_stats.py) the next iteration skips phase A.  The trial point fma(1, d, v) is the
    // update's iterate and the sums run in phase A's order, so the values are phase A's bit for bit.  The old stage
    // blocks are dead once the directional derivative is formed; a rejected full step recomputes them in phase A.
    // XB (round 5): the first trial is at alpha = alpha_max (fraction to the boundary) and the update's y is the same
    // fma(alpha, dy, y) (ip_update), so the fused evaluation is again phase A's; the barrier terms (ip_terms) of phase
    // A still run every iteration, after the dual update.
    constexpr bool FUSE_FWD = true;
    // PAIR: the stage-parallel phases take TWO stages per lane in one straight-line body, k and k + G (the unbounded
    // solves of a model whose functions take dpack values, HasWideEval: the 2-link arm, cfg#2).  A lane's stage
    // evaluation is one dependent FP64 chain (two range reductions, four Horner polynomials, a division, the quotient
    // rule) that issues every ~8 cycles where the wave could issue every 4; the second stage is an independent chain
    // in the same block, interleaved in the source (group_model_w).  A lane without a second stage (k + G >= N) repeats
    // its own stage k: it stores the same values to the same addresses, the max and non-finite accumulators are
    // idempotent, and the sums (J, |c|_1, dJ) keep their value after the first stage by one select each.  Per stage
    // every operation keeps its operands and order, and every per-lane sum its order (k, then k + G).  For N > 2 G the
    // loops run over pairs of rounds.  WD = 1 (every other kernel) is the one-stage loop as it was.  (PAIR and WD are
    // defined at the prologue, which takes the pairs too.)
    // the stage loops' body with `lin` hoisted (PAIR) or as group_model's run-time argument (LM = -1)
    auto with_lin = [&](auto wd_c, auto&& body) {
        if constexpr (decltype(wd_c)::value == 1) body(std::integral_constant<int, -1>{});
        else if (p.is_linear != 0) body(std::integral_constant<int, 1>{});
        else body(std::integral_constant<int, 0>{});
    };
    bool fwd_ready = false;
    double J0n = 0.0, c1n = 0.0, cmaxn = 0.0;
    int nfn = 0;
    MMPC_PHASE(0);
    for (it = resume ? p.tail_it[slot] : 0; !done; ++it) {
        MMPC_PHASE(8);
        __builtin_amdgcn_wave_barrier();
        // ---- A. stage-parallel: F_k, A_k/B_k blocks, defects, merit value ----
        double J0 = J0n, c1 = c1n, cmax = cmaxn;
        int nonfinite = nfn;
        const bool evalA = !(FUSE_FWD && fwd_ready);
        if (evalA) {
            J0 = 0.0;
            c1 = 0.0;
            cmax = 0.0;
            nonfinite = 0;
            with_lin(std::integral_constant<int, WA>{}, [&](auto lm_c) {
                constexpr int LM = decltype(lm_c)::value;
                for (int k0 = gl; k0 < N; k0 += WA * G) {
                    int kk[WA];
                    double x[WA][NX], u[WA][NU], xd[WA][NX], Fq[WA][SQ], Fqd[WA][FD], Fu[WA][FU];
#pragma unroll
                    for (int e = 0; e < WA; ++e) {
                        kk[e] = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
#pragma unroll
                        for (int r = 0; r < NX; ++r) x[e][r] = sX[kk[e] * NX + r];
#pragma unroll
                        for (int c = 0; c < NU; ++c) u[e][c] = sU[kk[e] * NU + c];
                    }
                    group_model_w<Model, WA, LM, true, SQ, FD, FU>(lin, lFq, lFqd, lFu, lxd, lxs, up, x, u, xd, Fq, Fqd, Fu);
                    double cd[WA][NX], er[WA][NX];
#pragma unroll
                    for (int e = 0; e < WA; ++e) {
                        const int k = kk[e];
#pragma unroll
                        for (int i = 0; i < FQ; ++i) sFq[k * FQ + i] = h * Fq[e][i];
#pragma unroll
                        for (int i = 0; i < FD; ++i) sFqd[k * FD + i] = h * Fqd[e][i];
#pragma unroll
                        for (int i = 0; i < FU; ++i) sFu[k * FU + i] = h * Fu[e][i];
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double F = fma(h, xd[e][r], x[e][r]);
                            sF[k * NX + r] = F;
                            cd[e][r] = F - sX[(k + 1) * NX + r];
                            sC[k * NX + r] = cd[e][r];
                            er[e][r] = F - tr[k * NX + r];
                        }
                    }
                    // the sums in stage order; a repeated stage leaves them as they were
#pragma unroll
                    for (int e = 0; e < WA; ++e) {
                        const int k = kk[e];
                        double Js = J0, cs = c1;
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double c = cd[e][r];
                            cmax = fmax(cmax, fabs(c));
                            cs += fabs(c);
                            nonfinite |= !isfinite(c);
                            Js = fma(er[e][r] * Q[r], er[e][r], Js);
                        }
#pragma unroll
                        for (int c = 0; c < NU; ++c) {
                            const double um = (k == 0) ? up[c] : sU[(k - 1) * NU + c];
                            const double dif = u[e][c] - um;
                            Js = fma(dif * R[c], dif, fma(u[e][c] * Rm[c], u[e][c], Js));
                        }
                        const bool on = e == 0 || k0 + e * G < N;
                        J0 = on ? Js : J0;
                        c1 = on ? cs : c1;
                    }
                }
            });
        }
        double lsum = 0.0, cmpl0 = 0.0, cmplmu = 0.0;  // interior point: sum log s, max |s z|, max |s z - mu|
        if constexpr (XB) {
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NY; ++j) {
                    const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    double sg, bb, zg;
                    ip_terms(y, yl[j], yu[j], sZl[k * NY + j], sZu[k * NY + j], mub, sg, bb, zg, cmpl0, cmplmu, lsum);
                    sSg[k * NY + j] = sg;
                    if constexpr (MEHR) sBb[k * NY + j] = 0.0;   // the affine predictor's barrier gradient
                    else sBb[k * NY + j] = bb;
                    sZg[k * NY + j] = zg;
                }
            }
            lsum = group_sum(lsum);
            cmpl0 = group_max(cmpl0);
            cmplmu = group_max(cmplmu);
            nonfinite |= !isfinite(lsum);
            // Sigma, b, z_u - z_l of every stage (HBM workspace) visible to the other lanes' serial sweeps
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        if (evalA) {
            J0 = group_sum(J0);
            c1 = group_sum(c1);
            cmax = group_max(cmax);
        }
        fwd_ready = false;
        __builtin_amdgcn_wave_barrier();
        MMPC_PHASE(1);

        // ---- B. one lane: d recursion, then adjoint + gradient + Riccati backward sweep (the 6x6 / 12x12
        //      Riccati step of one stage is too small to pay for lane-parallel exchanges: measured slower) ----
        double gmax = 0.0, lmax = 0.0;
        int fact_ok = 1;
        const double beps = BOUNDED ? fmin(kBoundEps, pg_prev) : 0.0;
        // backward sweep of QP solve `pass` (gradient and stop-test quantities are the same in every pass)
        auto backward = [&](int pass) {
            // P~ (symmetric, upper triangle used) and p~ on s = [dx_k; du_{k-1}]; P~_N = blkdiag(Q, 0)
            double P[NS][NS], pv[NS], lam[NX], unext[NU];
#define Ps(i, j) ((i) <= (j) ? P[(i)][(j)] : P[(j)][(i)])
#pragma unroll
            for (int a = 0; a < NS; ++a) {
                pv[a] = 0.0;
#pragma unroll
                for (int b = a; b < NS; ++b) P[a][b] = (a == b && a < NX) ? Q[a] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                const double eb = sX[N * NX + r] - tr[(N - 1) * NX + r];  // x_N - r_{N-1}
                pv[r] = Q[r] * eb;
                lam[r] = Q[r] * (sD[N * NX + r] + eb);  // lam_N = Q e_{N-1}
                if constexpr (XB) {  // barrier at x_N: Sigma, b in the value function, z_u - z_l in the adjoint
                    P[r][r] += sSg[(N - 1) * NY + r];
                    pv[r] += sBb[(N - 1) * NY + r];
                    lam[r] += sZg[(N - 1) * NY + r];
                }
                lmax = fmax(lmax, fabs(lam[r]));
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) unext[c] = 0.0;
            for (int k = N - 1; k >= 0; --k) {
                const double* hFq = sFq + k * FQ;
                const double* hFqd = sFqd + k * FD;
                double hFu[FU], x[NX], u[NU], um[NU], cc[NX], tg[NU];
#pragma unroll
                for (int i = 0; i < FU; ++i) hFu[i] = sFu[k * FU + i];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    x[r] = sX[k * NX + r];
                    cc[r] = sC[k * NX + r];
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    u[c] = sU[k * NU + c];
                    um[c] = (k == 0) ? up[c] : sU[(k - 1) * NU + c];
                }
                // reduced gradient g_k = B_k^T lam_{k+1} + R/Rm terms
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    double g = 0.0;
#pragma unroll
                    for (int s = 0; s < NA; ++s) g = fma(hFu[s * NU + c], lam[NQ + s], g);
                    g = fma(R[c], u[c] - um[c], fma(Rm[c], u[c], g));
                    if (k + 1 < N) g -= R[c] * (unext[c] - u[c]);
                    if (XB) g += sZg[k * NY + NX + c];  // reduced Lagrangian gradient
                    if (!BOUNDED) {
                        gmax = fmax(gmax, fabs(2.0 * g));
                    } else {  // projected gradient; hold rule (pass 0) or the holds of the previous solve
                        gmax = fmax(gmax, fabs(u[c] - proj(u[c] - 2.0 * g, lbv[c], ubv[c])));
                        if (pass == 0) {
                            tg[c] = (u[c] <= lbv[c] + beps && g > 0.0)   ? lbv[c]
                                    : (u[c] >= ubv[c] - beps && g < 0.0) ? ubv[c]
                                                                          : NAN;
                            sHold[k * NU + c] = tg[c];
                        } else {
                            tg[c] = sHold[k * NU + c];
                        }
                    }
                    nonfinite |= !isfinite(g);
                    unext[c] = u[c];
                }
                // adjoint lam_k = Q e_{k-1} + A_k^T lam_{k+1},  e_{k-1} = d_k + x_k - r_{k-1}
                if (k >= 1) {
                    double ln[NX];
                    at_mul<NQ, NA, double>(h, hFq, hFqd, lam, ln);
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        lam[r] = fma(Q[r], sD[k * NX + r] + x[r] - tr[(k - 1) * NX + r], ln[r]);
                        if (XB) lam[r] += sZg[(k - 1) * NY + r];
                        lmax = fmax(lmax, fabs(lam[r]));
                    }
                }
                // Riccati step (sqp_lane.h): G = P_xx B + P_xu, H_ww, h_w, Y = L^-1 [H_wx | -R | h_w]
                double Gm[NX][NU];
#pragma unroll
                for (int r = 0; r < NX; ++r)
#pragma unroll
                    for (int c = 0; c < NU; ++c) {
                        double t = Ps(r, NX + c);
#pragma unroll
                        for (int s = 0; s < NA; ++s) t = fma(Ps(r, NQ + s), hFu[s * NU + c], t);
                        Gm[r][c] = t;
                    }
                double mv[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    double t = pv[r];
#pragma unroll
                    for (int q = 0; q < NX; ++q) t = fma(Ps(r, q), cc[q], t);
                    mv[r] = t;
                }
                double Hww[NU][NU], Y[NU][NS + 1];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
#pragma unroll
                    for (int b = a; b < NU; ++b) {
                        double t = Ps(NX + a, NX + b);
#pragma unroll
                        for (int s = 0; s < NA; ++s)
                            t = fma(hFu[s * NU + a], Gm[NQ + s][b], fma(Ps(NQ + s, NX + a), hFu[s * NU + b], t));
                        if (a == b) t += R[a] + Rm[a];
                        if (XB && a == b) t += sSg[k * NY + NX + a];
                        Hww[a][b] = t;
                    }
                    double t = fma(R[a], u[a] - um[a], fma(Rm[a], u[a], pv[NX + a]));
                    if (XB) t += sBb[k * NY + NX + a];
#pragma unroll
                    for (int s = 0; s < NA; ++s) t = fma(hFu[s * NU + a], mv[NQ + s], t);
#pragma unroll
                    for (int r = 0; r < NX; ++r) t = fma(Ps(r, NX + a), cc[r], t);
                    Y[a][NS] = t;
                    double ga[NX];
#pragma unroll
                    for (int r = 0; r < NX; ++r) ga[r] = Gm[r][a];
                    at_mul<NQ, NA, double>(h, hFq, hFqd, ga, &Y[a][0]);
#pragma unroll
                    for (int c = 0; c < NU; ++c) Y[a][NX + c] = (a == c) ? -R[a] : 0.0;
                }
                // held controls (bounded): w_A = target - u fixed in the stage QP, as sqp_lane.h
                double pex[NS];
                if (BOUNDED) {
                    bool hd[NU], any = false;
                    double dl[NU];
#pragma unroll
                    for (int j = 0; j < NS; ++j) pex[j] = 0.0;
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        hd[a] = tg[a] == tg[a];
                        dl[a] = hd[a] ? tg[a] - u[a] : 0.0;
                        any |= hd[a];
                    }
                    if (any) {
#pragma unroll
                        for (int a = 0; a < NU; ++a)
#pragma unroll
                            for (int j = 0; j < NS; ++j) pex[j] = fma(Y[a][j], dl[a], pex[j]);
#pragma unroll
                        for (int b = 0; b < NU; ++b) {
                            double t = Y[b][NS];
#pragma unroll
                            for (int a = 0; a < NU; ++a) t = fma(Hww[a < b ? a : b][a < b ? b : a], dl[a], t);
                            Y[b][NS] = hd[b] ? -dl[b] : t;
                        }
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
#pragma unroll
                            for (int b = a; b < NU; ++b)
                                if (hd[a] || hd[b]) Hww[a][b] = (a == b) ? 1.0 : 0.0;
                            if (hd[a])
#pragma unroll
                                for (int j = 0; j < NS; ++j) Y[a][j] = 0.0;
                        }
                    }
                }
                // P~_k x block A^T P_xx A + Q and p~_k x part A^T mv + Q (x_k - r_{k-1}), before P is overwritten
                double Pn[NX][NX], pn[NS];
                if (k >= 1) {
#pragma unroll
                    for (int b = 0; b < NX; ++b) {
                        double row[NX], tcol[NX];
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            double t;
                            if (b < NQ) {
                                t = Ps(r, b);
#pragma unroll
                                for (int s = 0; s < NA; ++s) t = fma(hFq[s * NQ + b], Ps(r, NQ + s), t);
                            } else {
                                t = (b - NQ < NQ) ? fma(h, Ps(r, b - NQ), Ps(r, b)) : Ps(r, b);
#pragma unroll
                                for (int s = 0; s < NA; ++s) t = fma(hFqd[s * NA + b - NQ], Ps(r, NQ + s), t);
                            }
                            tcol[r] = t;
                        }
                        at_mul<NQ, NA, double>(h, hFq, hFqd, tcol, row);
#pragma unroll
                        for (int a = 0; a <= b; ++a)
                            Pn[a][b] = row[a] + ((a == b) ? Q[a] + (XB ? sSg[(k - 1) * NY + a] : 0.0) : 0.0);
                    }
                    double t[NX];
                    at_mul<NQ, NA, double>(h, hFq, hFqd, mv, t);
#pragma unroll
                    for (int q = 0; q < NX; ++q) {
                        pn[q] = fma(Q[q], x[q] - tr[(k - 1) * NX + q], t[q]);
                        if (XB) pn[q] += sBb[(k - 1) * NY + q];
                    }
#pragma unroll
                    for (int c = 0; c < NU; ++c) pn[NX + c] = -R[c] * (u[c] - um[c]);
                }
                // [K_k | kff_k] = -H_ww^-1 [H_wx | -R | h_w] (into wK) and Y with Y^T Y = Z^T H_ww^-1 Z for the
                // update of P~ and p~.  nu = 2: explicit inverse (one reciprocal; no square roots -- the serial
                // sweep is latency-bound); otherwise Cholesky, Y = L^-1 Z.
                double Kt[NU][NS + 1];
                if constexpr (NU == 2 && !XB) {  // XB: Cholesky (Y^T Y stays PSD with the large barrier Sigma)
                    const double det = fma(Hww[0][0], Hww[1][1], -Hww[0][1] * Hww[0][1]);
                    fact_ok &= (Hww[0][0] > 0.0) && (det > 0.0) && isfinite(det);
                    const double idet = rcp_nr(det);  // two Newton steps: ~1 ulp, off the division's long chain
                    const double i00 = Hww[1][1] * idet, i11 = Hww[0][0] * idet, i01 = -Hww[0][1] * idet;
#pragma unroll
                    for (int j = 0; j <= NS; ++j) {
                        Kt[0][j] = fma(i00, Y[0][j], i01 * Y[1][j]);
                        Kt[1][j] = fma(i01, Y[0][j], i11 * Y[1][j]);
                    }
                } else {
                    double Ld[NU][NU], il[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        double sd = Hww[a][a];
#pragma unroll
                        for (int q = 0; q < a; ++q) sd = fma(-Ld[a][q], Ld[a][q], sd);
                        fact_ok &= (sd > 0.0) && isfinite(sd);
                        // 1/sqrt by v_rsq + two Newton steps (no square root and division on the serial chain)
                        const double sp = fmax(sd, 1e-300);
                        double r = __builtin_amdgcn_rsq(sp);
                        r = r * fma(-0.5 * sp * r, r, 1.5);
                        r = r * fma(-0.5 * sp * r, r, 1.5);
                        Ld[a][a] = sp * r;
                        il[a] = r;
#pragma unroll
                        for (int b = a + 1; b < NU; ++b) {
                            double t = Hww[a][b];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[b][q], Ld[a][q], t);
                            Ld[b][a] = t * il[a];
                        }
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a)
#pragma unroll
                        for (int j = 0; j <= NS; ++j) {
                            double t = Y[a][j];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[a][q], Y[q][j], t);
                            Y[a][j] = t * il[a];
                        }
#pragma unroll
                    for (int a = NU - 1; a >= 0; --a)
#pragma unroll
                        for (int j = 0; j <= NS; ++j) {
                            double t = Y[a][j];
#pragma unroll
                            for (int q = a + 1; q < NU; ++q) t = fma(-Ld[q][a], Kt[q][j], t);
                            Kt[a][j] = t * il[a];
                        }
                }
#pragma unroll
                for (int a = 0; a < NU; ++a)
#pragma unroll
                    for (int j = 0; j <= NS; ++j) wK[(k * NU + a) * (NS + 1) + j] = -Kt[a][j];
                if (k == 0) break;
                // P~_k = blkdiag(A^T P_xx A + Q, R) - Z^T H_ww^-1 Z, p~_k = pn - Z^T H_ww^-1 h_w:
                // nu = 2 as Y^T Kt (Y = Z, Kt = H_ww^-1 Z), Cholesky as Y^T Y (Y = L^-1 Z)
                const double(&YB)[NU][NS + 1] = (NU == 2 && !XB) ? Kt : Y;
#pragma unroll
                for (int a = 0; a < NS; ++a) {
                    double t = pn[a];
#pragma unroll
                    for (int q = 0; q < NU; ++q) t = fma(-Y[q][a], YB[q][NS], t);
                    if (BOUNDED) t += pex[a];
                    pv[a] = t;
#pragma unroll
                    for (int b = a; b < NS; ++b) {
                        double v = (b < NX) ? Pn[a][b] : ((a == b) ? R[a - NX] : 0.0);
#pragma unroll
                        for (int q = 0; q < NU; ++q) v = fma(-Y[q][a], YB[q][b], v);
                        P[a][b] = v;
                    }
                }
            }
#undef Ps
        };
        // ---- C. one lane: step sweep du = K s + kff, dx, directional derivative ----
        double dJ = 0.0;
        bool resolve = false;
        auto step_sweep = [&](int pass) {
            dJ = 0.0;
            double dx[NX], dup[NU], um[NU];
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                dx[r] = 0.0;
                sDX[r] = 0.0;
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                dup[c] = 0.0;
                um[c] = up[c];
            }
            // software pipeline: K_{k+1} (HBM) and the LDS operands of step k+1 are loaded during step k
            constexpr int NK = NU * (NS + 1);
            double nK[NK], nFq[SQ], nFqd[FD], nFu[FU], nF[NX], nc[NX], nr[NX], nu_[NU];
#define GROUP_LOAD_STEP(k_)                                                                        \
        do {                                                                                           \
            const int kk_ = (k_);                                                                      \
            _Pragma("unroll") for (int i_ = 0; i_ < NK; ++i_) nK[i_] = wK[kk_ * NK + i_];              \
            _Pragma("unroll") for (int i_ = 0; i_ < FQ; ++i_) nFq[i_] = sFq[kk_ * FQ + i_];             \
            _Pragma("unroll") for (int i_ = 0; i_ < FD; ++i_) nFqd[i_] = sFqd[kk_ * FD + i_];           \
            _Pragma("unroll") for (int i_ = 0; i_ < FU; ++i_) nFu[i_] = sFu[kk_ * FU + i_];             \
            _Pragma("unroll") for (int r_ = 0; r_ < NX; ++r_) {                                        \
            nF[r_] = sF[kk_ * NX + r_];                                                            \
            nc[r_] = sC[kk_ * NX + r_];                                                            \
            nr[r_] = sR[kk_ * NX + r_];                                                            \
            }                                                                                          \
            _Pragma("unroll") for (int c_ = 0; c_ < NU; ++c_) nu_[c_] = sU[kk_ * NU + c_];             \
        } while (0)
            GROUP_LOAD_STEP(0);
            // unrolled by two so that the prefetch buffers are renamed instead of copied (2-link only: the exo
            // step spills when unrolled)
            constexpr int kStepUnroll = NX <= 4 ? 2 : 1;
#pragma unroll kStepUnroll
            for (int k = 0; k < N; ++k) {
                double K[NK], hFq[SQ], hFqd[FD], hFu[FU], Fk[NX], ck[NX], rk[NX], uk[NU];
#pragma unroll
                for (int i = 0; i < NK; ++i) K[i] = nK[i];
#pragma unroll
                for (int i = 0; i < FQ; ++i) hFq[i] = nFq[i];
#pragma unroll
                for (int i = 0; i < FD; ++i) hFqd[i] = nFqd[i];
#pragma unroll
                for (int i = 0; i < FU; ++i) hFu[i] = nFu[i];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    Fk[r] = nF[r];
                    ck[r] = nc[r];
                    rk[r] = nr[r];
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) uk[c] = nu_[c];
                if (k + 1 < N) GROUP_LOAD_STEP(k + 1);
                double du[NU];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
                    double t = K[a * (NS + 1) + NS];
#pragma unroll
                    for (int q = 0; q < NX; ++q) t = fma(K[a * (NS + 1) + q], dx[q], t);
#pragma unroll
                    for (int c = 0; c < NU; ++c) t = fma(K[a * (NS + 1) + NX + c], dup[c], t);
                    du[a] = t;
                    sDU[k * NU + a] = t;
                }
                if (BOUNDED && pass + 1 < kBoundPasses) {  // a free control whose step crosses a bound: hold it
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        const double hv = sHold[k * NU + a], t = uk[a] + du[a];
                        if (hv != hv && (t < lbv[a] || t > ubv[a])) {
                            sHold[k * NU + a] = t < lbv[a] ? lbv[a] : ubv[a];
                            resolve = true;
                        }
                    }
                }
                double ad[NX];
                a_mul<NQ, NA, double>(h, hFq, hFqd, dx, ad);
#pragma unroll
                for (int s = 0; s < NA; ++s)
#pragma unroll
                    for (int c = 0; c < NU; ++c) ad[NQ + s] = fma(hFu[s * NU + c], du[c], ad[NQ + s]);
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    const double qe = 2.0 * Q[r] * (Fk[r] - rk[r]);
                    dJ = fma(qe, ad[r], dJ);
                    dx[r] = ad[r] + ck[r];
                    sDX[(k + 1) * NX + r] = dx[r];
                }
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    const double dif = uk[c] - um[c];
                    dJ = fma(2.0 * R[c] * dif, du[c] - dup[c], fma(2.0 * Rm[c] * uk[c], du[c], dJ));
                    um[c] = uk[c];
                    dup[c] = du[c];
                }
            }
#undef GROUP_LOAD_STEP
        };
        // ---- DIST: the same recursions with row r of every quantity on lane r of the group ----
        // column r of A (x-lanes): own row (identity) + h in row z for r = NQ + z + acol[t] in row NQ + t, where
        // acol = hFq[:, r] (q-lanes) or hFqd[:, r - NQ] (a-lanes); so (A^T v)[r] = colA(v_r, vb) with vb = all v.
        auto colA = [&](double own, const double* acol, const double* vb) {
            double t = lxf * own;
#pragma unroll
            for (int z = 0; z < NQ; ++z) t = fma(hq[z], vb[z], t);
#pragma unroll
            for (int s2 = 0; s2 < NA; ++s2) t = fma(acol[s2], vb[NQ + s2], t);
            return t;
        };
        // row r of [A - I | B] (x-lanes) at stage k: q-lanes h e_{NQ+r}, a-lanes [hFq, hFqd | hFu] row r - NQ
        // (unconditional loads through the lane's own index and stage stride, iAq / iAd / iBr above: a conditional LDS
        // load becomes a branch, and a select between a loaded value and a register a flat load through a selected
        // LDS-or-scratch pointer)
        auto load_arow = [&](int k, double* arow, double* brow) {
#pragma unroll
            for (int s2 = 0; s2 < NQ; ++s2)
                arow[s2] = LOPS ? lds(iAq + __mul24(k, zAq) + 8 * s2) : fma(lad, sFq[k * FQ + ta * NQ + s2], hrow[s2]);
#pragma unroll
            for (int s2 = 0; s2 < NA; ++s2)
                arow[NQ + s2] = LOPS ? lds(iAd + __mul24(k, zAd) + 8 * s2) : fma(lad, sFqd[k * FD + ta * NA + s2], hrow[NQ + s2]);
#pragma unroll
            for (int c = 0; c < NU; ++c) brow[c] = LOPS ? lds(iBr + __mul24(k, zBr) + 8 * c) : lad * sFu[k * FU + ta * NU + c];
        };
        // d_{k+1} = A_k d_k + c_k (d_0 = 0): lane r holds d_k[r]
        // The recursions below are latency-bound (a few FMAs per stage on the dependency chain): every stage's
        // LDS operands are loaded one stage ahead and the dot products split into two partial sums.
        auto d_recursion_dist = [&]() {
            double dr = 0.0;
            if (MIRROR || lx) sD[rx] = 0.0;   // (also what re-zeroes the step sweep's dump doubles, see step_dist)
            // stage operands (row r of A - I through the lane's own address, used as loaded; the wait for a load sits a
            // full stage after its issue): two buffers, each refilled two stages ahead.  MIRROR: a buffer is refilled
            // after its last use in program order (the refill closes the stage, behind a scheduling barrier), so the
            // old and the new contents are never live together and the unroll by two renames the buffers without a copy.
            struct Op {
                double q[NQ > 0 ? NQ : 1], d[NA], c;
            };
            // (the lane's two row addresses run along with the fetches, one add each per stage: fetch k is the k-th call)
            LdsB jq = iAq, jd = iAd;
            auto fetch = [&](int k, Op& o) {
#pragma unroll
                for (int s2 = 0; s2 < NQ; ++s2) o.q[s2] = LOPS ? lds(jq + 8 * s2) : sFq[k * FQ + ta * NQ + s2];
#pragma unroll
                for (int s2 = 0; s2 < NA; ++s2) o.d[s2] = LOPS ? lds(jd + 8 * s2) : sFqd[k * FD + ta * NA + s2];
                o.c = sC[k * NX + rx];
                if constexpr (LOPS) {
                    jq += zAq;
                    jd += zAd;
                    pin(jq);
                    pin(jd);
                }
            };
            auto stage = [&](int k, Op& o) {
                double db[NX], arow[NX];
#pragma unroll
                for (int s2 = 0; s2 < NQ; ++s2) arow[s2] = LOPS ? o.q[s2] : fma(lad, o.q[s2], hrow[s2]);
#pragma unroll
                for (int s2 = 0; s2 < NA; ++s2) arow[NQ + s2] = LOPS ? o.d[s2] : fma(lad, o.d[s2], hrow[NQ + s2]);
                const double cr = o.c;
                // unconditional and unclamped (static wait counts; the address is a strength-reduced increment): past
                // the last stage the loads read the next arrays of this instance's LDS block (sFq -> sFqd -> sFu,
                // sC -> sFq), values never used
                if constexpr (!MIRROR) fetch(k + 2, o);
                sfor<0, NX>([&](auto I) { db[I] = row_bcast<I>(dr); });
                double t0 = dr + cr, t1 = 0.0;
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    if (j & 1) t1 = fma(arow[j], db[j], t1);
                    else t0 = fma(arow[j], db[j], t0);
                }
                // no lane-role mask on the chain: only the x-lanes' d is broadcast.  MIRROR: the other lanes carry lane 0's
                // d and store it again over lane 0's (same address, same bits), so the store needs no exec mask;
                // otherwise their finite leftovers (a sum of c_k[0]) are never read or stored
                dr = t0 + t1;
                if (MIRROR || lx) sD[(k + 1) * NX + rx] = dr;
                if constexpr (MIRROR) {
                    __builtin_amdgcn_sched_barrier(0);   // the refill stays behind the last use of o
                    fetch(k + 2, o);
                }
            };
            Op o0, o1;
            fetch(0, o0);
            fetch(LOPS || N > 1 ? 1 : 0, o1);   // LOPS: the second call, stage 1 (N = 1: stage N, as the prefetches below)
            int k = 0;
            for (; k + 1 < N; k += 2) {
                stage(k, o0);
                stage(k + 1, o1);
            }
            if (k < N) stage(k, o0);
        };
        // adjoint + reduced gradient + Riccati backward sweep; lane r: row r of P~ (Prow) and p~ (pvr), lam[r]
        // column r of the a-rows of A at stage k: hFq[:, r] (q-lanes), hFqd[:, r - NQ] (a-lanes), 0 otherwise
        // (ACOLP: jc = the lane's column address at stage k, kept by the caller, which takes the stages N - 1 .. 0 in order:
        // it leaves here one stage down, one add per stage)
        auto load_acol = [&](int k, [[maybe_unused]] LdsB& jc, double* acol) {
            if constexpr (ACOLP) {
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) acol[t2] = lds(jc + 8 * t2 * NA);
                jc -= zAc;
                pin(jc);
            } else {
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) {
                    double v = lad * sFqd[k * FD + t2 * NA + ta];
                    if constexpr (NQ > 0) v = fma(lqd, sFq[k * FQ + t2 * NQ + rq], v);
                    acol[t2] = v;
                }
            }
        };
        // adjoint lam_k = Q e_{k-1} + A_k^T lam_{k+1} (lam_N = Q e_{N-1}, e_{k-1} = d_k + x_k - r_{k-1}), lane r holds
        // lam[r] (x-lanes) and writes it over d_k in sD (d_k is read one stage earlier); then, stage-parallel, the
        // reduced gradient g_k = B_k^T lam_{k+1} + R (u_k - u_{k-1}) + Rm u_k - R (u_{k+1} - u_k) from the stored
        // lam (the serial sweep carries only the lam chain: the gradient's loads and arithmetic were a quarter of
        // its instructions).  gmax, lmax are per-lane maxima (reduced by the caller).
        // Runs before the stop test, so a converged wave skips the Riccati sweep.
        auto adjoint_dist = [&]() {
            double lamr;
            // MIRROR: a lane without an x row carries lane 0's lam (Q, column, operands and stores of row 0), so the
            // stores need no exec mask and lmax no lane factor (the maximum over the group sees lane 0's value twice);
            // Qa is the Q of the row the lane carries (without MIRROR: Qr)
            {
                const double eb = (MIRROR || lx) ? sX[N * NX + rx] - tr[(N - 1) * NX + rx] : 0.0;   // x_N - r_{N-1}
                lamr = Qa * (sD[N * NX + rx] + eb);
                if constexpr (XB) lamr += (MIRROR ? 1.0 : lxf) * sZg[(N - 1) * NY + rx];   // z_u - z_l of x_N's bounds
                lmax = fmax(lmax, fabs(lamr));
                if (MIRROR || lx) sD[N * NX + rx] = lamr;   // lam_k replaces d_k (read one stage earlier)
            }
            // stage operands as loaded, two buffers refilled two stages ahead (d_k is read before stage k writes lam_k
            // over it): column r of A's a-rows and the pieces of Q (d_k + x_k - r_{k-1})[r], combined at the use
            struct Op {
                double fd[NA], fq[NA], xk, trm, dk, zg;
            };
            // ACOLP: the lane's column address runs down with the fetches, one add per stage and no clamp: fetch number
            // i reads stage N - 1 - i, and the two fetches past stage 1 (values never used) read stages 0 and -1 of the
            // lane's array -- the end of the array in front of it (sC, sFq), inside the instance's block
            [[maybe_unused]] LdsB jc = (!MIRROR || lx) ? iAcN : shb + 8 * ((int)(sFq - shm) + (N - 1) * FD);
            [[maybe_unused]] const int zc = MIRROR ? 8 * FD : zAc;   // (every x-lane is a q- or an a-lane)
            auto fetch = [&](int k, Op& o) {   // k >= 1
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) {
                    if constexpr (ACOLP) {
                        o.fd[t2] = lds(jc + 8 * t2 * NA);
                    } else {
                        o.fd[t2] = sFqd[k * FD + t2 * NA + ta];
                        if constexpr (NQ > 0) o.fq[t2] = sFq[k * FQ + t2 * NQ + rq];
                    }
                }
                if constexpr (ACOLP) {
                    jc -= zc;
                    pin(jc);
                }
                o.xk = sX[k * NX + rx];
                o.trm = tr[(k - 1) * NX + rx];
                o.dk = sD[k * NX + rx];
                if constexpr (XB) o.zg = sZg[(k - 1) * NY + rx];   // z_u - z_l of x_k's bounds
            };
            // stage k >= 1: lam_k from lam_{k+1}; then refill o with stage k - 2 (k >= 3; MIRROR: where `more` says so)
            auto stage = [&](int k, Op& o, [[maybe_unused]] bool more = true) {
                double acol[NA];
#pragma unroll
                for (int t2 = 0; t2 < NA; ++t2) {
                    if constexpr (ACOLP) {
                        acol[t2] = o.fd[t2];
                    } else {
                        double v = lad * o.fd[t2];
                        if constexpr (NQ > 0) v = fma(lqd, o.fq[t2], v);
                        acol[t2] = v;
                    }
                }
                double qe = Qa * (o.dk + (o.xk - o.trm));
                if constexpr (XB) qe += o.zg;
                if constexpr (!MIRROR) fetch(k >= 3 ? k - 2 : 1, o);   // unconditional: static wait counts
                double lamb[NX];
                sfor<0, NX>([&](auto I) { lamb[I] = row_bcast<I>(lamr); });
                // (A^T lam)[r] + Q e_{k-1}[r], two partial sums
                // unmasked chain: a lane without an x row carries lane 0's lam (MIRROR), stored again over lane 0's;
                // otherwise it has Qr = 0, acol = 0 and hq = 0, so it carries 0 (XB: a finite sum of another row's z
                // gaps) -- never broadcast or stored, and masked out of lmax
                double t0 = lamr + qe, t1 = 0.0;
#pragma unroll
                for (int z = 0; z < NQ; ++z) t1 = fma(hq[z], lamb[z], t1);
#pragma unroll
                for (int s2 = 0; s2 < NA; ++s2) {
                    if (s2 & 1) t1 = fma(acol[s2], lamb[NQ + s2], t1);
                    else t0 = fma(acol[s2], lamb[NQ + s2], t0);
                }
                lamr = t0 + t1;
                lmax = fmax(lmax, fabs(MIRROR ? lamr : lxf * lamr));
                if (MIRROR || lx) sD[k * NX + rx] = lamr;
                if constexpr (MIRROR) {   // the refill closes the stage, behind the last use of o (no buffer copies)
                    __builtin_amdgcn_sched_barrier(0);
                    if (more) fetch(k - 2, o);
                }
            };
            if (N >= 2) {
                Op o0, o1;
                fetch(N - 1, o0);
                fetch(N >= 3 ? N - 2 : 1, o1);
                int k = N - 1;
                if constexpr (MIRROR) {
                    // no clamp: the pair loop takes the stages whose refills (k - 2, k - 3) exist, unconditionally
                    // (static wait counts at its top); the two or three stages left run apart, stage 3 with its refill
                    for (; k >= 4; k -= 2) {
                        stage(k, o0);
                        stage(k - 1, o1);
                    }
                    if (k == 3) {
                        stage(3, o0);
                        stage(2, o1, false);
                        stage(1, o0, false);
                    } else if (k == 2) {
                        stage(2, o0, false);
                        stage(1, o1, false);
                    } else {
                        stage(1, o0, false);
                    }
                } else {
                    for (; k >= 2; k -= 2) {
                        stage(k, o0);
                        stage(k - 1, o1);
                    }
                    if (k == 1) stage(1, o0);
                }
            }
            // the lam rows of the other lanes of this wave must be visible to the gradient pass
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    double g = 0.0;
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) g = fma(sFu[k * FU + s2 * NU + c], sD[(k + 1) * NX + NQ + s2], g);
                    const double uk = sU[k * NU + c], um = k == 0 ? up[c] : sU[(k - 1) * NU + c];
                    g = fma(R[c], uk - um, fma(Rm[c], uk, g));
                    if (k < N - 1) g -= R[c] * (sU[(k + 1) * NU + c] - uk);
                    if constexpr (XB) g += sZg[k * NY + NX + c];   // reduced Lagrangian gradient
                    if constexpr (!BOUNDED) {
                        gmax = fmax(gmax, fabs(2.0 * g));
                    } else {   // projected gradient; epsilon-active holds of the first QP solve (oracle solve_one)
                        gmax = fmax(gmax, fabs(uk - proj(uk - 2.0 * g, lbv[c], ubv[c])));
                        sHold[k * NU + c] = (uk <= lbv[c] + beps && g > 0.0)   ? lbv[c]
                                            : (uk >= ubv[c] - beps && g < 0.0) ? ubv[c]
                                                                                : NAN;
                    }
                    nonfinite |= !isfinite(g);
                }
            }
        };
        auto backward_dist = [&](bool useW) {
            if constexpr (BOUNDED) {   // the hold targets (sHold) the gradient pass stored on every lane of this wave
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            double Prow[NS], pvr;
            [[maybe_unused]] LdsB jcol = iAcN;   // load_acol's running address
            const double lxm = lx ? 1.0 : 0.0;
            // W_k row rx and uu block, loaded one stage ahead into one buffer: from the workspace, or (WLDS) row rx of
            // the packed record in LDS at this lane's row offset wrow + col(j), a structural zero under wm = 0;
            // the records were written by the other lanes of this wave, and LDS serves a wave's accesses in order.
            // (Round 2 used two
            // buffers two stages ahead; once the control-affine sweep dropped the uu block, the second buffer's
            // registers cost more than the load latency it hid: 0.1875 -> 0.1808 ms with one buffer)
            struct Wb {
                double r[KZ], u[NU * NU];
            };
            Wb w0;
            auto load_w = [&](int k, Wb& b) {
#pragma unroll
                for (int j = 0; j < KZ; ++j)   // row rx; masked at its uses
                    b.r[j] = WLDS ? sW[k * PK + wrow + WPack<Model>::col(j)] : wH[k * HW + rx * KZ + j];
                if constexpr (!CAFF) {
#pragma unroll
                    for (int j = 0; j < NU * NU; ++j) b.u[j] = wH[k * HW + NX * KZ + j];
                }
            };
            if (EXACT && useW) {
                load_w(N - 1, w0);
            }
#pragma unroll
            for (int j = 0; j < NS; ++j) Prow[j] = j < NX ? qoh[j] : 0.0;   // P~_N = blkdiag(Q, 0)
            pvr = Qr * (lx ? sX[N * NX + rx] - tr[(N - 1) * NX + rx] : 0.0);   // Q (x_N - r_{N-1})
            if constexpr (XB) {   // barrier at x_N: Sigma on the diagonal, b in p~
                const double sgN = sSg[(N - 1) * NY + rx], bbN = sBb[(N - 1) * NY + rx];
#pragma unroll
                for (int j = 0; j < NX; ++j) Prow[j] = fma(dgx[j], sgN, Prow[j]);
                pvr = fma(lxm, bbN, pvr);
            }
            // The stage's first FMAs (T, mv) need P~'s row, which is in registers, and h da/du and c of the stage: LDS
            // returns a wave's reads in order and the wave has nothing else to issue at the stage's top, so whatever
            // is queued in front of those two is waited for in full.  LOPS: the two are handed over from the stage
            // before (Hb, loaded in the middle of that stage's P~ update, as the W row one stage ahead), and the stage's
            // other operands are read in place in the order of first use, those of colA / at_mul last.  (A buffer for
            // all of a stage's operands spills to AGPRs; the sweep is otherwise bound by issue slots.)
            struct Hb {
                double fu[FU], c[NX];
            };
            Hb h0;
            auto load_head = [&](int k, Hb& b) {
#pragma unroll
                for (int i = 0; i < FU; ++i) b.fu[i] = sFu[k * FU + i];
#pragma unroll
                for (int q = 0; q < NX; ++q) b.c[q] = sC[k * NX + q];
            };
            if constexpr (LOPS) load_head(N - 1, h0);
            // stage k; LAST = (k == 0), peeled so that the stages k >= 1 carry no k == 0 selects or branches
            // HEADK: a stage k <= 2 of a kernel with the head block, which takes its K | kff columns
            auto stage = [&](int k, auto last_c, auto head_c, Wb& wb, Hb& hb) {
                constexpr bool LAST = decltype(last_c)::value, HEADK = decltype(head_c)::value;
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                const unsigned long long st_top = __builtin_amdgcn_s_memtime();
                __builtin_amdgcn_sched_barrier(0);
#endif
                double hFq[SQ], hFqd[FD], hFu[FU], cc[NX], u[NU], um[NU], acol[NA];
                if constexpr (!LOPS) {
#pragma unroll
                    for (int i = 0; i < FQ; ++i) hFq[i] = sFq[k * FQ + i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) hFqd[i] = sFqd[k * FD + i];
                    load_head(k, hb);
                }
#pragma unroll
                for (int i = 0; i < FU; ++i) hFu[i] = hb.fu[i];
#pragma unroll
                for (int q = 0; q < NX; ++q) cc[q] = hb.c[q];
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                // the stamp behind the arrival of the operands of T and mv (s_memtime's own result needs lgkmcnt(0):
                // in the order of the other models it also waits for the reads queued behind them)
#pragma unroll
                for (int i = 0; i < FU; ++i) asm volatile("" ::"v"(hFu[i]));
#pragma unroll
                for (int q = 0; q < NX; ++q) asm volatile("" ::"v"(cc[q]));
                __builtin_amdgcn_sched_barrier(0);
                if (gl == 0 && blockIdx.x < kPhaseWavePhases && k < 32) {
                    g_mmpc_phase_cycles[kPhaseStageLog + 128 * blockIdx.x + 32 * gi + k] = st_top;
                    g_mmpc_phase_cycles[kPhaseWaitLog + 128 * blockIdx.x + 32 * gi + k] = __builtin_amdgcn_s_memtime();
                }
                __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
                for (int c = 0; c < NU; ++c) {
                    u[c] = sU[k * NU + c];
                    um[c] = LAST ? up[c] : sU[(k - 1) * NU + c];
                }
                load_acol(k, jcol, acol);
                if constexpr (LOPS) {
#pragma unroll
                    for (int i = 0; i < FQ; ++i) hFq[i] = sFq[k * FQ + i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) hFqd[i] = sFqd[k * FD + i];
                }
                // XB: the barrier pieces of this stage (u_k) and of x_k (stage k-1), loaded with the stage operands:
                // read at their uses, deep in the stage, their HBM latency was exposed
                double xsgu[XB ? NU : 1], xbbu[XB ? NU : 1], xsgx = 0.0, xbbx = 0.0;
                if constexpr (XB) {
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        xsgu[a] = sSg[k * NY + NX + a];
                        xbbu[a] = sBb[k * NY + NX + a];
                    }
                    if constexpr (!LAST) {
                        xsgx = sSg[(k - 1) * NY + rx];
                        xbbx = sBb[(k - 1) * NY + rx];
                    }
                }
                double exr = 0.0, duu = 0.0;
                if constexpr (!LAST) {
                    const double xk = sX[k * NX + rx], trm = tr[(k - 1) * NX + rx];
                    exr = xk - trm;   // non-x lanes: finite leftovers of the clamped row, masked by lxm in pn
                    duu = sU[k * NU + ru] - sU[(k - 1) * NU + ru];
                }
                double wr[KZ], wu[NU * NU];
                if constexpr (EXACT) {
#pragma unroll
                    for (int j = 0; j < KZ; ++j) wr[j] = useW ? wb.r[j] : 0.0;
#pragma unroll
                    for (int j = 0; j < NU * NU; ++j) wu[j] = (useW && !CAFF) ? wb.u[j] : 0.0;
                    if (!LAST && useW) load_w(k - 1, wb);
                }
                // T = P~ [B; I] (row r), mv = P~_x. c + p~ (row r)
                double T[NU], mv = pvr;
#pragma unroll
                for (int b = 0; b < NU; ++b) {
                    double t = Prow[NX + b];
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) t = fma(Prow[NQ + s2], hFu[s2 * NU + b], t);
                    T[b] = t;
                }
#pragma unroll
                for (int q = 0; q < NX; ++q) mv = fma(Prow[q], cc[q], mv);
                double Tb[NS][NU], mvb[NS];
                sfor<0, NS>([&](auto I) {
#pragma unroll
                    for (int b = 0; b < NU; ++b) Tb[I][b] = row_bcast<I>(T[b]);
                    mvb[I] = row_bcast<I>(mv);
                });
                // H_ww = B^T P_xx B + B^T P_xu + P_ux B + P_uu + R + Rm, h_w (redundant)
                double Hww[NU][NU], hw[NU];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
#pragma unroll
                    for (int b = a; b < NU; ++b) {
                        double t = Tb[NX + a][b];
#pragma unroll
                        for (int s2 = 0; s2 < NA; ++s2) t = fma(hFu[s2 * NU + a], Tb[NQ + s2][b], t);
                        if (a == b) t += R[a] + Rm[a];
                        if constexpr (EXACT && !CAFF) t += wu[a * NU + b];
                        if constexpr (XB) {
                            if (a == b) t += xsgu[a];   // barrier Sigma of u_k
                        }
                        Hww[a][b] = t;
                        Hww[b][a] = t;
                    }
                    double t = fma(R[a], u[a] - um[a], fma(Rm[a], u[a], mvb[NX + a]));
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) t = fma(hFu[s2 * NU + a], mvb[NQ + s2], t);
                    if constexpr (XB) t += xbbu[a];   // barrier gradient b of u_k
                    hw[a] = t;
                }
                // column r of Y = [H_wx | -R | .]: x-lanes (A^T T)[r], u-lanes -R e_{r-NX}
                double Ycol[NU];
#pragma unroll
                for (int a = 0; a < NU; ++a) {
                    double tb[NX];
#pragma unroll
                    for (int q = 0; q < NX; ++q) tb[q] = Tb[q][a];
                    Ycol[a] = colA(T[a], acol, tb) - rdg[a];
                    // H_wx[a][r] += W_ux[a][r] (x-lanes; WLDS: the x-lanes whose entry is not a structural zero)
                    if constexpr (EXACT) Ycol[a] = fma(WLDS ? wm[NX + a] : lxm, wr[NX + a], Ycol[a]);
                }
                // BOUNDED: the un-held stage rows [H_wx | -R | H_ww | h_w] (lane j < NS: column j; lanes NS.. the H_ww
                // columns and h_w, the idle lanes duplicating h_w) -- the step sweep forms the multiplier of a held
                // control from them (primal-dual active set: release a hold whose multiplier points into the box)
                if constexpr (BOUNDED) {
#pragma unroll
                    for (int c0 = 0; c0 < NR; c0 += G) {   // column c0 + r; lanes past the row rewrite its last entry
                        const int col = c0 + r < NR ? c0 + r : NR - 1;
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
                            double v = hw[a];
#pragma unroll
                            for (int b = 0; b < NU; ++b)
                                if (col == NS + b) v = Hww[a][b];
                            wRel[(k * NU + a) * NR + col] = col < NS ? Ycol[a] : v;
                        }
                    }
                }
                // held controls (BOUNDED, sHold of this QP solve): du_a = target - u_a fixed in the stage QP, as the
                // one-lane sweep -- p~ gains [H_wx | -R]^T delta, h_w the coupling H_ww delta, the held rows and
                // columns of H_ww become the identity and the held rows of [H_wx | -R] zero, so that K_a = 0 and
                // kff_a = delta_a exactly; Rk: the -R columns of the u-lanes with the held rows removed
                double pexr = 0.0, Rk[NU];
#pragma unroll
                for (int c = 0; c < NU; ++c) Rk[c] = R[c];
                if constexpr (BOUNDED) {
                    bool hd[NU];
                    double dl[NU], hw2[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        const double tg = sHold[k * NU + a];
                        hd[a] = tg == tg;
                        dl[a] = hd[a] ? tg - u[a] : 0.0;
                        pexr = fma(Ycol[a], dl[a], pexr);
                    }
#pragma unroll
                    for (int b = 0; b < NU; ++b) {
                        double t = hw[b];
#pragma unroll
                        for (int a = 0; a < NU; ++a) t = fma(Hww[a][b], dl[a], t);
                        hw2[b] = hd[b] ? -dl[b] : t;
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        hw[a] = hw2[a];
#pragma unroll
                        for (int b = 0; b < NU; ++b)
                            if (hd[a] || hd[b]) Hww[a][b] = (a == b) ? 1.0 : 0.0;
                        if (hd[a]) {
                            Ycol[a] = 0.0;
                            Rk[a] = 0.0;
                        }
                    }
                }
                // Kcol = H_ww^-1 Ycol (this lane's column of K~), kff = H_ww^-1 h_w (redundant)
                double Kcol[NU], kff[NU], Ku[NU][NU];
                // XB: Cholesky H_ww = L L^T, Ytil = L^-1 Ycol (this lane's column of L^-1 [H_wx | -R]), htil = L^-1 h_w;
                // the update P~ -= Ytil^T Ytil stays positive semidefinite under the barrier's large Sigma
                double Ytil[NU], htil[NU];
                if constexpr (XB) {
                    double Ld[NU][NU], il[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        double sd = Hww[a][a];
#pragma unroll
                        for (int q = 0; q < a; ++q) sd = fma(-Ld[a][q], Ld[a][q], sd);
                        fact_ok &= (sd > 0.0) && isfinite(sd);
                        const double sp = fmax(sd, 1e-300);
                        double rr = __builtin_amdgcn_rsq(sp);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        Ld[a][a] = sp * rr;
                        il[a] = rr;
#pragma unroll
                        for (int b = a + 1; b < NU; ++b) {
                            double t = Hww[a][b];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[b][q], Ld[a][q], t);
                            Ld[b][a] = t * il[a];
                        }
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a) {   // forward substitutions
                        double t = Ycol[a], th = hw[a];
#pragma unroll
                        for (int q = 0; q < a; ++q) {
                            t = fma(-Ld[a][q], Ytil[q], t);
                            th = fma(-Ld[a][q], htil[q], th);
                        }
                        Ytil[a] = t * il[a];
                        htil[a] = th * il[a];
                    }
#pragma unroll
                    for (int a = NU - 1; a >= 0; --a) {   // back substitutions: K~ column, kff
                        double t = Ytil[a], th = htil[a];
#pragma unroll
                        for (int q = a + 1; q < NU; ++q) {
                            t = fma(-Ld[q][a], Kcol[q], t);
                            th = fma(-Ld[q][a], kff[q], th);
                        }
                        Kcol[a] = t * il[a];
                        kff[a] = th * il[a];
                    }
                    if constexpr (MEHR) {   // the record of this stage for backward_vec
                        double* const rec = sVr + k * VR;
                        double pc = 0.0;
#pragma unroll
                        for (int q = 0; q < NX; ++q) pc = fma(Prow[q], cc[q], pc);
                        rec[r] = pc;
                        rec[G + r] = fma(-Rr, duu, lxm * (Qr * exr));
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
                            rec[(2 + a) * G + r] = Ytil[a];
#pragma unroll
                            for (int q = 0; q < a; ++q) rec[VL * G + a * (a + 1) / 2 + q] = Ld[a][q];
                            rec[VL * G + a * (a + 1) / 2 + a] = il[a];
                            rec[VL * G + VC + a] = fma(R[a], u[a] - um[a], Rm[a] * u[a]);
                        }
                    }
                } else if constexpr (NU == 2) {
                    const double det = fma(Hww[0][0], Hww[1][1], -Hww[0][1] * Hww[0][1]);
                    fact_ok &= (Hww[0][0] > 0.0) && (det > 0.0) && isfinite(det);
                    const double idet = rcp_nr(det);
                    const double i00 = Hww[1][1] * idet, i11 = Hww[0][0] * idet, i01 = -Hww[0][1] * idet;
                    Kcol[0] = fma(i00, Ycol[0], i01 * Ycol[1]);
                    Kcol[1] = fma(i01, Ycol[0], i11 * Ycol[1]);
                    kff[0] = fma(i00, hw[0], i01 * hw[1]);
                    kff[1] = fma(i01, hw[0], i11 * hw[1]);
                    Ku[0][0] = -i00 * Rk[0];
                    Ku[0][1] = -i01 * Rk[1];
                    Ku[1][0] = -i01 * Rk[0];
                    Ku[1][1] = -i11 * Rk[1];
                } else {   // Cholesky H_ww = L L^T (rsq + Newton), solves with L and L^T
                    double Ld[NU][NU], il[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        double sd = Hww[a][a];
#pragma unroll
                        for (int q = 0; q < a; ++q) sd = fma(-Ld[a][q], Ld[a][q], sd);
                        fact_ok &= (sd > 0.0) && isfinite(sd);
                        const double sp = fmax(sd, 1e-300);
                        double rr = __builtin_amdgcn_rsq(sp);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        rr = rr * fma(-0.5 * sp * rr, rr, 1.5);
                        Ld[a][a] = sp * rr;
                        il[a] = rr;
#pragma unroll
                        for (int b = a + 1; b < NU; ++b) {
                            double t = Hww[a][b];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[b][q], Ld[a][q], t);
                            Ld[b][a] = t * il[a];
                        }
                    }
                    auto chol_solve = [&](const double* rhs, double* out) {
                        double y[NU];
#pragma unroll
                        for (int a = 0; a < NU; ++a) {
                            double t = rhs[a];
#pragma unroll
                            for (int q = 0; q < a; ++q) t = fma(-Ld[a][q], y[q], t);
                            y[a] = t * il[a];
                        }
#pragma unroll
                        for (int a = NU - 1; a >= 0; --a) {
                            double t = y[a];
#pragma unroll
                            for (int q = a + 1; q < NU; ++q) t = fma(-Ld[q][a], out[q], t);
                            out[a] = t * il[a];
                        }
                    };
                    chol_solve(Ycol, Kcol);
                    chol_solve(hw, kff);
#pragma unroll
                    for (int c = 0; c < NU; ++c) {   // column NX + c of K~: H_ww^-1 (-R_c e_c)
                        double e[NU], o[NU];
#pragma unroll
                        for (int a = 0; a < NU; ++a) e[a] = (a == c) ? -Rk[c] : 0.0;
                        chol_solve(e, o);
#pragma unroll
                        for (int a = 0; a < NU; ++a) Ku[a][c] = o[a];
                    }
                }
                // [K_k | kff_k] = -[K~ | kff~] (lane j < NS stores column j, lanes >= NS the feed-forward column: kff
                // is computed redundantly, bit-identical on every lane of the group, so the duplicate stores of the
                // idle lanes write the same value -- no exec-mask branch in the sweep)
                {
                    const int col = r < NS ? r : NS;
#pragma unroll
                    for (int a = 0; a < NU; ++a)
                        (HEADK ? sKh : wK)[(k * NU + a) * (NS + 1) + col] = -(r < NS ? Kcol[a] : kff[a]);
                }
                if constexpr (LAST) return;
                // A^T P_xx A (row r) from the broadcast P_xx, p~_x = A^T mv + Q (x_k - r_{k-1})
                double Pb[NX][NX];
                sfor<0, NX>([&](auto I) {
#pragma unroll
                    for (int j = I; j < NX; ++j) {
                        Pb[I][j] = row_bcast<I>(Prow[j]);
                        Pb[j][I] = Pb[I][j];
                    }
                });
                double Ur[NX], Pn[NX];
#pragma unroll
                for (int j = 0; j < NX; ++j) {
                    double pc[NX];
#pragma unroll
                    for (int q = 0; q < NX; ++q) pc[q] = Pb[q][j];
                    Ur[j] = colA(Prow[j], acol, pc);
                }
                at_mul<NQ, NA, double>(h, hFq, hFqd, Ur, Pn);
                // the next stage's h da/du and c: T, mv, H_ww and h_w of this stage are formed, so the buffer is free, and
                // the rest of the P~ update (some 60 instructions) covers the reads.  Left alone, the scheduler sinks
                // them to their uses at the next stage's top; the barrier further up in the stage (in front of the
                // P~ update, or of Y) made the unbounded exact kernel spill.
                if constexpr (LOPS) {
                    load_head(k - 1, hb);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // x-lanes A^T mv + Q (x_k - r_{k-1}), u-lanes -R (u_k - u_{k-1}), idle lanes 0 -- blended with the
                // lane-role factor (Rr = 0 off the u-lanes) instead of a branch
                double pn = fma(-Rr, duu, lxm * fma(Qr, exr, colA(mv, acol, mvb)));
                double sgk = 0.0;   // XB: barrier Sigma and b of x_k (stage k-1's y)
                if constexpr (XB) {
                    sgk = xsgx;
                    pn = fma(lxm, xbbx, pn);
                }
                if constexpr (XB) {   // P~_k = blkdiag(A^T P_xx A + Q + Sigma, R) - Ytil^T Ytil, p~_k = pn - Ytil^T htil
                    double Yb[NU][NS];
                    sfor<0, NS>([&](auto I) {
#pragma unroll
                        for (int a = 0; a < NU; ++a) Yb[a][I] = row_bcast<I>(Ytil[a]);
                    });
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        double v = j < NX ? fma(dgx[j], sgk, Pn[j] + qoh[j]) : rdg[j - NX];
                        if constexpr (EXACT) {
                            if (j < NX) v = fma(lxm, wr[j], v);   // + W_xx row r (round 6: the exact Hessian under bounds)
                        }
#pragma unroll
                        for (int a = 0; a < NU; ++a) v = fma(-Ytil[a], Yb[a][j], v);
                        Prow[j] = v;
                    }
                    double pv2 = pn;
#pragma unroll
                    for (int a = 0; a < NU; ++a) pv2 = fma(-Ytil[a], htil[a], pv2);
                    pvr = pv2;
                    return;
                }
                // K~ columns of the other lanes
                double Kb[NU][NX];
                sfor<0, NX>([&](auto I) {
#pragma unroll
                    for (int a = 0; a < NU; ++a) Kb[a][I] = row_bcast<I>(Kcol[a]);
                });
                // P~_k = blkdiag(A^T P_xx A + Q, R) - Y^T K~, p~_k = pn - Y^T kff (row r)
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double v = j < NX ? Pn[j] + qoh[j] : rdg[j - NX];
                    if constexpr (EXACT) {
                        if (j < NX) v = fma(WLDS ? wm[j] : lxm, wr[j], v);   // W_xx row r (x-lanes; the mask folded into the add)
                    }
#pragma unroll
                    for (int a = 0; a < NU; ++a) v = fma(-Ycol[a], j < NX ? Kb[a][j] : Ku[a][j - NX], v);
                    Prow[j] = v;
                }
                double pv2 = pn;
#pragma unroll
                for (int a = 0; a < NU; ++a) pv2 = fma(-Ycol[a], kff[a], pv2);
                if constexpr (BOUNDED) pv2 += pexr;
                pvr = pv2;
            };
            // inner stages N-1 .. 1 by unconditional pairs (an odd count peels stage N-1 in front), as the step sweep;
            // the control-bounded sweep one stage per trip (its hold logic and relaxation rows fill the registers: two
            // stages in flight spilled to scratch inside the loop)
            using F_ = std::false_type;
            using T_ = std::true_type;
            if constexpr (BOUNDED || (XB && EXACT)) {
                for (int k = N - 1; k >= 1; --k) stage(k, F_{}, F_{}, w0, h0);
                stage(0, T_{}, F_{}, w0, h0);
            } else if constexpr (KH > 0) {
                // head block: the pair loop ends at stage 3 (an odd count of stages N - 1 .. 3 peels stage N - 1), and
                // the stages 2, 1 (one more pair body) and 0 that store there follow as straight-line code -- a store
                // address chosen per stage inside the loop would cost every stage what these three save.  (Stages
                // 2 and 1 each under a test of their own made the exact kernel spill four registers.)
                int k = N - 1;
                if (N >= 4 && ((N - 3) & 1)) stage(k--, F_{}, F_{}, w0, h0);
                for (; k >= 4; k -= 2) {
                    stage(k, F_{}, F_{}, w0, h0);
                    stage(k - 1, F_{}, F_{}, w0, h0);
                }
                if (N >= 3) {
                    stage(2, F_{}, T_{}, w0, h0);
                    stage(1, F_{}, T_{}, w0, h0);
                } else if (N == 2) {
                    stage(1, F_{}, T_{}, w0, h0);
                }
                stage(0, T_{}, T_{}, w0, h0);
            } else if ((N - 1) & 1) {
                stage(N - 1, F_{}, F_{}, w0, h0);
                for (int k = N - 2; k >= 2; k -= 2) {
                    stage(k, F_{}, F_{}, w0, h0);
                    stage(k - 1, F_{}, F_{}, w0, h0);
                }
                stage(0, T_{}, F_{}, w0, h0);
            } else {
                for (int k = N - 1; k >= 2; k -= 2) {
                    stage(k, F_{}, F_{}, w0, h0);
                    stage(k - 1, F_{}, F_{}, w0, h0);
                }
                stage(0, T_{}, F_{}, w0, h0);
            }
        };
        // MEHR corrector: the vector part (p~, kff) of the Riccati recursion for the barrier gradient now in sBb, on the
        // matrices of the sweep that just ran (its per-stage record sVr): mv = p~ + P~_x c, h_w, kff = H_ww^-1 h_w through
        // the stored factor, p~_k = pn - Ytil^T L^-1 h_w.  Only the kff column of the gains is rewritten.
        [[maybe_unused]] auto backward_vec = [&]() {
            if constexpr (MEHR) {
                const double lxm = lx ? 1.0 : 0.0;
                [[maybe_unused]] LdsB jcol = iAcN;   // load_acol's running address
                double pvr = Qr * (lx ? sX[N * NX + rx] - tr[(N - 1) * NX + rx] : 0.0);   // Q (x_N - r_{N-1})
                pvr = fma(lxm, sBb[(N - 1) * NY + rx], pvr);
                struct Rec {
                    double pc, pn0, yt[NU], sh[VS], bbu[NU], bbx;
                };
                auto fetch = [&](int k, Rec& o) {
                    const double* const rec = sVr + k * VR;
                    o.pc = rec[r];
                    o.pn0 = rec[G + r];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {
                        o.yt[a] = rec[(2 + a) * G + r];
                        o.bbu[a] = sBb[k * NY + NX + a];
                    }
#pragma unroll
                    for (int i = 0; i < VS; ++i) o.sh[i] = rec[VL * G + i];
                    o.bbx = sBb[(k > 0 ? k - 1 : 0) * NY + rx];   // b of x_k (stage k - 1's y); unused at k = 0
                };
                auto stage = [&](int k, const Rec& o) {
                    double hFu[FU], acol[NA];
#pragma unroll
                    for (int i = 0; i < FU; ++i) hFu[i] = sFu[k * FU + i];
                    load_acol(k, jcol, acol);
                    const double mv = pvr + o.pc;
                    double mvb[NS];
                    sfor<0, NS>([&](auto I) { mvb[I] = row_bcast<I>(mv); });
                    double htil[NU], kff[NU];
#pragma unroll
                    for (int a = 0; a < NU; ++a) {   // h_w, then L^-1 h_w
                        double t = o.sh[VC + a] + mvb[NX + a];
#pragma unroll
                        for (int s2 = 0; s2 < NA; ++s2) t = fma(hFu[s2 * NU + a], mvb[NQ + s2], t);
                        t += o.bbu[a];
#pragma unroll
                        for (int q = 0; q < a; ++q) t = fma(-o.sh[a * (a + 1) / 2 + q], htil[q], t);
                        htil[a] = t * o.sh[a * (a + 1) / 2 + a];
                    }
#pragma unroll
                    for (int a = NU - 1; a >= 0; --a) {
                        double t = htil[a];
#pragma unroll
                        for (int q = a + 1; q < NU; ++q) t = fma(-o.sh[q * (q + 1) / 2 + a], kff[q], t);
                        kff[a] = t * o.sh[a * (a + 1) / 2 + a];
                    }
                    // bit-identical on every lane: duplicate stores, no exec-mask branch (as backward_dist)
#pragma unroll
                    for (int a = 0; a < NU; ++a) wK[(k * NU + a) * (NS + 1) + NS] = -kff[a];
                    if (k == 0) return;
                    double pv2 = fma(lxm, colA(mv, acol, mvb) + o.bbx, o.pn0);
#pragma unroll
                    for (int a = 0; a < NU; ++a) pv2 = fma(-o.yt[a], htil[a], pv2);
                    pvr = pv2;
                };
                // two buffers, each refilled one stage ahead of its use
                Rec o0, o1;
                fetch(N - 1, o0);
                int k = N - 1;
                for (; k >= 1; k -= 2) {
                    fetch(k - 1, o1);
                    stage(k, o0);
                    fetch(k >= 2 ? k - 2 : 0, o0);
                    stage(k - 1, o1);
                }
                if (k == 0) stage(0, o0);
            }
        };
        if constexpr (DIST) {
            d_recursion_dist();
            adjoint_dist();
            lmax = group_max(lmax);
            gmax = group_max(gmax);
        } else if (gl == 0) {
            {
                double d[NX];
#pragma unroll
                for (int r = 0; r < NX; ++r) {
                    d[r] = 0.0;
                    sD[r] = 0.0;
                }
                // the operands of step k+1 are loaded during step k (the recursion is latency-bound)
                double aq[SQ], ad[FD], ac[NX];
#pragma unroll
                for (int i = 0; i < FQ; ++i) aq[i] = sFq[i];
#pragma unroll
                for (int i = 0; i < FD; ++i) ad[i] = sFqd[i];
#pragma unroll
                for (int r = 0; r < NX; ++r) ac[r] = sC[r];
                constexpr int kDUnroll = NX <= 4 ? 2 : 1;
#pragma unroll kDUnroll
                for (int k = 0; k < N; ++k) {
                    double fq[SQ], fd[FD], cc[NX], dn[NX];
#pragma unroll
                    for (int i = 0; i < FQ; ++i) fq[i] = aq[i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) fd[i] = ad[i];
#pragma unroll
                    for (int r = 0; r < NX; ++r) cc[r] = ac[r];
                    const int kn = k + 1 < N ? k + 1 : k;
#pragma unroll
                    for (int i = 0; i < FQ; ++i) aq[i] = sFq[kn * FQ + i];
#pragma unroll
                    for (int i = 0; i < FD; ++i) ad[i] = sFqd[kn * FD + i];
#pragma unroll
                    for (int r = 0; r < NX; ++r) ac[r] = sC[kn * NX + r];
                    a_mul<NQ, NA, double>(h, fq, fd, d, dn);
#pragma unroll
                    for (int r = 0; r < NX; ++r) {
                        d[r] = dn[r] + cc[r];
                        sD[(k + 1) * NX + r] = d[r];
                    }
                }
            }
            backward(0);
        }
        if constexpr (!DIST) {
            gmax = group_bcast(gmax, gbase);
            lmax = group_bcast(lmax, gbase);
            fact_ok = group_bcast_i(fact_ok, gbase);
        }
        MMPC_PHASE(2);
        nonfinite = (group_max((double)nonfinite) != 0.0);
        kkt = fmax(gmax, cmax);
        if (XB) kkt = fmax(kkt, 2.0 * cmpl0);  // J-scale complementarity
        double* trc = p.trace && valid ? p.trace + (inst * (p.max_iter + 1) + it) * 8 : nullptr;
        if (trc && gl == 0) {
            trc[0] = gmax;
            trc[1] = cmax;
            trc[2] = J0;
            trc[3] = c1;
            trc[7] = lmax;
        }
        if (nonfinite || !isfinite(kkt)) {
            status = ST_NONFINITE;
            break;
        }
        if (gmax <= p.tol_grad && cmax <= p.tol_defect && (!XB || 2.0 * cmpl0 <= kIpTolCompl)) {
            status = ST_CONVERGED;
            break;
        }
        if (it == p.max_iter) {
            status = ST_MAX_ITER;
            break;
        }
        MMPC_PHASE(9);
        if constexpr (EXACT) {
            // stage-parallel: W_k = h sum_s lam_{k+1,NQ+s} d^2 acc_s/d(x_k,u_k)^2 (lam from the adjoint, in sD)
            __builtin_amdgcn_wave_barrier();
            // W_k of stage k on lane k mod 16.  WLDS: the packed record goes to sW[k], over sD[1..] | sDX | sDU.  Record k
            // starts at double NX + PK k of sD and lam_{k'+1} ends at NX (k' + 2), so with PK >= NX writing record k can
            // only overwrite the lam operands of stages k' >= k.  The stages are therefore taken in rounds of 16 from the
            // last round down, for every N: the stages above a round are done, and within a round every lane's lam loads
            // precede every lane's stores in program order (one wave; LDS serves its accesses in order).
            // PAIR: a lane takes the stages k0 + gl and k0 + G + gl of two rounds together (kk[0], kk[1]; the first again when
            // the second is past the horizon), from the last pair of rounds down.  The argument holds for the pair as for
            // the round: the pairs of rounds above are done; inside the pair every lane's lam loads of BOTH stages precede
            // every lane's stores in program order, and the stores reach only lam operands of stages >= the pair's lowest,
            // all of them loaded or done.  A repeated stage stores its record twice, with the same values.
            auto w_stages = [&](const int (&kk)[WW]) {
                double x[WW][NX], u[WW][NU], la[WW][NA], W[WW][KZ * KZ];
#pragma unroll
                for (int e = 0; e < WW; ++e) {
                    const int k = kk[e];
#pragma unroll
                    for (int r2 = 0; r2 < NX; ++r2) x[e][r2] = sX[k * NX + r2];
#pragma unroll
                    for (int c = 0; c < NU; ++c) u[e][c] = sU[k * NU + c];
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) la[e][s2] = h * sD[(k + 1) * NX + NQ + s2];
                }
                if constexpr (WLDS) __builtin_amdgcn_wave_barrier();   // (compiler: no store of this round above a load)
                if constexpr (WW == 1) {
                    Model::eval_hess(x[0], u[0], la[0], W[0]);
                } else {   // the WW evaluations with their chains in turn (two_link_fast.h)
                    using T = dpack<WW>;
                    T xw[NX], uw[NU], lw[NA], Ww[KZ * KZ];
#pragma unroll
                    for (int e = 0; e < WW; ++e) {
#pragma unroll
                        for (int i = 0; i < NX; ++i) xw[i].v[e] = x[e][i];
#pragma unroll
                        for (int i = 0; i < NU; ++i) uw[i].v[e] = u[e][i];
#pragma unroll
                        for (int i = 0; i < NA; ++i) lw[i].v[e] = la[e][i];
                    }
                    Model::eval_hess(xw, uw, lw, Ww);
#pragma unroll
                    for (int e = 0; e < WW; ++e)
#pragma unroll
                        for (int i = 0; i < KZ * KZ; ++i) W[e][i] = Ww[i].v[e];
                }
#pragma unroll
                for (int e = 0; e < WW; ++e) {
                    const int k = kk[e];
                    if constexpr (WLDS) {
                        static_assert(!WLDS || PK >= NX, "write order of the W pass");
#pragma unroll
                        for (int r2 = 0; r2 < NX; ++r2)
#pragma unroll
                            for (int j = r2; j < KZ; ++j)
                                if (WPack<Model>::idx(r2, j) >= 0) sW[k * PK + WPack<Model>::idx(r2, j)] = W[e][r2 * KZ + j];
                    } else {
                        double* const dst = wH + k * HW;
#pragma unroll
                        for (int r2 = 0; r2 < NX; ++r2)
#pragma unroll
                            for (int j = 0; j < KZ; ++j)
                                if (!w_struct_zero<Model>(r2, j) || !w_zeros_stored) dst[r2 * KZ + j] = W[e][r2 * KZ + j];
                        if constexpr (!CAFF) {
#pragma unroll
                            for (int a = 0; a < NU; ++a)
#pragma unroll
                                for (int b = 0; b < NU; ++b) dst[NX * KZ + a * NU + b] = W[e][(NX + a) * KZ + NX + b];
                        }
                    }
                }
            };
            auto w_pair = [&](int k0) {   // the lane's stages of the WW rounds from k0 (= its stage of the first)
                int kk[WW];
#pragma unroll
                for (int e = 0; e < WW; ++e) kk[e] = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
                w_stages(kk);
            };
            if constexpr (WLDS) {
                for (int k0 = ((N - 1) / (WW * G)) * (WW * G); k0 >= 0; k0 -= WW * G)
                    if (k0 + gl < N) w_pair(k0 + gl);
                MMPC_PHASE(9);   // (timing build: "check" = the stop test and this W pass)
                // the records of the other lanes of this wave are in LDS before the sweep's loads: program order
                __builtin_amdgcn_wave_barrier();
            } else {
                for (int k = gl; k < N; k += WW * G) w_pair(k);
                w_zeros_stored = true;
                MMPC_PHASE(9);   // (timing build: "check" = the stop test and this W pass up to its fence)
                // the stores of the other lanes of this wave must be visible to the sweep's loads
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
        }
        // exact Hessian in this iteration's QP solves (false after a Gauss-Newton fallback)
        bool use_w = EXACT;
        if constexpr (DIST) {   // Riccati sweep (fact_ok is uniform over the group)
            backward_dist(use_w);
            // exact KKT matrix not positive definite on the null space: this iteration takes the Gauss-Newton step
            // (oracle solve_one: Cholesky of the exact condensed Hessian fails -> Gauss-Newton)
            if (EXACT && !fact_ok) {
                fact_ok = 1;
                use_w = false;
                backward_dist(false);
            }
        }
        if (!fact_ok) {
            status = ST_FACT_FAILED;
            break;
        }
        if (BOUNDED) pg_prev = gmax;
        // barrier update for the next iteration (IPOPT monotone rule, lagged; oracle solve_one_ip)
        const double mub_next = (XB && fmax(fmax(0.5 * gmax, cmax), cmplmu) <= kIpKappaEps * mub)
                                    ? fmax(kIpTolCompl / 20.0, fmin(kIpKappaMu * mub, pow(mub, kIpThetaMu)))
                                    : mub;

        MMPC_PHASE(3);
        if constexpr (DIST) {
            // step sweep: lane r holds s_k[r], s = [dx_k; du_{k-1}]; u-lanes du_k = K_k s_k + kff_k (row r - NX of
            // K from the workspace), x-lanes dx_{k+1} = A dx + B du + c.  A dx_k + B du_k goes to sD[k+1] (d is
            // dead after the backward sweep) for the directional derivative below.
            // check: a free control whose step crosses a bound is held there (sHold) and the QP solved again (BOUNDED)
            auto step_dist = [&](bool check) {
                // K_k columns were stored by the other lanes of this wave in the backward sweep
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                constexpr bool RUN = MIRROR;   // running addresses, unmasked stores, no clamped prefetch (below)
                double sr = 0.0;
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                if (gl == 0 && blockIdx.x < kPhaseWavePhases)
                    g_mmpc_phase_cycles[kPhaseStepLog + 8 * blockIdx.x + 2 * gi] = __builtin_amdgcn_s_memtime();
#endif
                if (RUN || lx) sDX[rx] = 0.0;
                constexpr int NK = NS + 1;
                const double* const Kp = wK + ru * NK;   // row ru of K_k | kff_k at Kp + k NU NK
                // the stage operands of a buffer: the K row from the HBM/L2 workspace, row r of [A - I | B] and c_k[r]
                // from LDS
                struct Ops {
                    double K[NK], a[NX], b[NU], c, Rw[BOUNDED ? NR : 1];
                };
                const double* const Rp = wRel + ru * NR;   // BOUNDED: un-held row ru at Rp + k NU NR
                // RUN: every address of the sweep runs along it, one add per stage, opaque to the loop optimiser -- the
                // lane's three row addresses and its c address (the stage of the next refill), the K (and un-held) row
                // pointer, and two store addresses:
                //   js: where the lane's s goes -- x-lanes dx_{k+1}[r] in sDX (stride NX), u-lanes du_k in sDU (stride NU);
                //       the stored value is the lane's next s, so one store serves both roles and s needs one select
                //   jt: where A dx_k + B du_k goes -- x-lanes sD[k+1][r] (stride NX).  A u-lane has no such row; its sum
                //       (finite: its own du_{k-1} plus row 0's products) goes to sD[ru] with stride 0.  sD[0 .. NX) is
                //       d_0: no sweep or pass of the lane-distributed kernels reads it (they start at sD[NX]), and the d
                //       recursion zeroes it again at the start of the next iteration.
                // A lane without a role carries lane 0's chain (rows, c and K row 0 as lane 0) and stores lane 0's
                // values to lane 0's addresses.
                using LdsW = __attribute__((address_space(3))) double*;
                [[maybe_unused]] LdsB ja = iAq, jd = iAd, jb = iBr, jcs = shb + 8 * ((int)(sC - shm) + rx);
                [[maybe_unused]] LdsB js = shb + 8 * (lu ? (int)(sDU - shm) + ru : (int)(sDX - shm) + NX + rx);
                [[maybe_unused]] LdsB jt = shb + 8 * (lu ? (int)(sD - shm) + ru : (int)(sD - shm) + NX + rx);
                [[maybe_unused]] const int zs = lu ? 8 * NU : 8 * NX, zt = lu ? 0 : 8 * NX;
                using GlbD = const __attribute__((address_space(1))) double*;   // (stays a global load behind the pin)
                [[maybe_unused]] GlbD jK = (GlbD)Kp;
                [[maybe_unused]] GlbD jR = (GlbD)Rp;
                // (hs: -1, or the stage 0 .. 2 whose K row the head block holds -- the opening's refills)
                [[maybe_unused]] auto refill = [&](Ops& o, int hs = -1) {   // the next stage in order
#pragma unroll
                    for (int j = 0; j < NK; ++j) o.K[j] = (KH > 0 && hs >= 0) ? sKh[(hs * NU + ru) * NK + j] : jK[j];
#pragma unroll
                    for (int s2 = 0; s2 < NQ; ++s2) o.a[s2] = lds(ja + 8 * s2);
#pragma unroll
                    for (int s2 = 0; s2 < NA; ++s2) o.a[NQ + s2] = lds(jd + 8 * s2);
#pragma unroll
                    for (int c = 0; c < NU; ++c) o.b[c] = lds(jb + 8 * c);
                    o.c = lds(jcs);
                    if constexpr (BOUNDED) {
#pragma unroll
                        for (int j = 0; j < NR; ++j) o.Rw[j] = jR[j];
                    }
                };
                [[maybe_unused]] auto advance = [&]() {
                    ja += zAq;
                    jd += zAd;
                    jb += zBr;
                    jcs += 8 * NX;
                    jK += NU * NK;
                    pin(ja);
                    pin(jd);
                    pin(jb);
                    pin(jcs);
                    asm volatile("" : "+v"(jK));
                    if constexpr (BOUNDED) {
                        jR += NU * NR;
                        asm volatile("" : "+v"(jR));
                    }
                };
                auto fetch = [&](int k, Ops& o) {
#pragma unroll
                    for (int j = 0; j < NK; ++j) o.K[j] = Kp[k * NU * NK + j];
                    load_arow(k, o.a, o.b);
                    o.c = sC[k * NX + rx];
                    if constexpr (BOUNDED) {
#pragma unroll
                        for (int j = 0; j < NR; ++j) o.Rw[j] = Rp[k * NU * NR + j];
                    }
                };
                // (more: RUN, whether the stage refills its buffer with the stage three ahead)
                auto stage = [&](int k, Ops& o, [[maybe_unused]] bool more = true) {
                    double sb[NS];
                    sfor<0, NS>([&](auto I) { sb[I] = row_bcast<I>(sr); });
                    double du0 = o.K[NS], du1 = 0.0;
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        if (j & 1) du1 = fma(o.K[j], sb[j], du1);
                        else du0 = fma(o.K[j], sb[j], du0);
                    }
                    const double du = du0 + du1;
                    double ad = sr;
#pragma unroll
                    for (int j = 0; j < NX; ++j) ad = fma(o.a[j], sb[j], ad);
                    double dub[NU];
                    sfor<0, NU>([&](auto I) { dub[I] = row_bcast<NX + I>(du); });
#pragma unroll
                    for (int c = 0; c < NU; ++c) ad = fma(o.b[c], dub[c], ad);
                    const double dxn = ad + o.c;
                    if constexpr (RUN) {   // unmasked stores through the lane's running store addresses
                        sr = lu ? du : dxn;
                        *(LdsW)js = sr;
                        *(LdsW)jt = ad;
                        js += zs;
                        jt += zt;
                        pin(js);
                        pin(jt);
                    } else {
                        if (lx) {
                            sDX[(k + 1) * NX + rx] = dxn;
                            sD[(k + 1) * NX + rx] = ad;
                        }
                        if (lu) sDU[k * NU + ru] = du;
                    }
                    if constexpr (BOUNDED) {
                        if (check && lu) {
                            const double hv = sHold[k * NU + ru], t = sU[k * NU + ru] + du;
                            if (hv != hv) {   // free: hold it where its step crosses a bound
                                if (t < lbr || t > ubr) {
                                    sHold[k * NU + ru] = t < lbr ? lbr : ubr;
                                    resolve = true;
                                }
                            } else if (!p.no_release) {   // held: release it when its multiplier H_ww du + [H_wx | -R] s + h_w points inward
                                double m = o.Rw[NR - 1];
#pragma unroll
                                for (int j = 0; j < NS; ++j) m = fma(o.Rw[j], sb[j], m);
#pragma unroll
                                for (int b = 0; b < NU; ++b) m = fma(o.Rw[NS + b], dub[b], m);
                                if ((hv == lbr && m < 0.0) || (hv == ubr && m > 0.0)) {
                                    sHold[k * NU + ru] = NAN;
                                    resolve = true;
                                }
                            }
                        }
                    }
#if defined(MMPC_PHASE_TIMING) && defined(MMPC_PHASE_STAGES)
                    asm volatile("" ::"v"(sr), "v"(ad));
                    if (k == 0 && gl == 0 && blockIdx.x < kPhaseWavePhases)
                        g_mmpc_phase_cycles[kPhaseStepLog + 8 * blockIdx.x + 2 * gi + 1] = __builtin_amdgcn_s_memtime();
#endif
                    if constexpr (RUN) {
                        if (more) {
                            refill(o);
                            advance();
                        }
                    } else {
                        sr = lx ? dxn : (lu ? du : 0.0);
                        fetch(k + 3 < N ? k + 3 : N - 1, o);   // unconditional: static wait counts
                    }
                };
                // three buffers, refilled three stages ahead: the K rows come from L2/MALL (the workspace of a
                // 512-instance XCD exceeds its 4 MB L2) and one stage of the sweep (~300 cycles) did not cover that
                // latency -- with two buffers every stage waited for the loads issued one stage earlier
                Ops o0, o1, o2;
                if constexpr (RUN) {
                    // No clamp and no read past stage N - 1.  The N - 3 stages that have a stage three ahead refill their
                    // buffer: the three-stage body takes them three at a time (the same outstanding loads on every path
                    // at its top: the wait before stage k's operands is vmcnt(#loads of stages k + 1, k + 2)), the one
                    // or two left over follow it; the last three stages run without a refill, from the buffers the
                    // rotation has reached.  The opening loads of a horizon shorter than three read its last stage
                    // again (values never used) instead of moving on.
                    // With the head block (KH) the opening's K rows are LDS reads, under one uniform test for the
                    // horizons that have three stages (the form with a test between the refills makes the exact kernel
                    // spill two registers); the K pointer runs along, so that the first refill of a stage finds row 3
                    // of the workspace.  Where the K rows come from the workspace the test sits between the refills:
                    // the uniform form measured slower there.
                    if (KH == 0 || N < 3) {
                        refill(o0, 0);
                        if (N > 1) advance();
                        refill(o1, N > 1 ? 1 : 0);
                        if (N > 2) advance();
                        refill(o2, N > 2 ? 2 : N - 1);
                        advance();
                    } else {
                        refill(o0, 0);
                        advance();
                        refill(o1, 1);
                        advance();
                        refill(o2, 2);
                        advance();
                    }
                    int k = 0;
                    for (; k + 5 < N; k += 3) {
                        stage(k, o0, true);
                        stage(k + 1, o1, true);
                        stage(k + 2, o2, true);
                    }
                    const int left = N - 3 - k;   // refilling stages left: 0, 1 or 2 (negative: N < 3)
                    if (left == 1) {
                        stage(k, o0, true);
                        stage(k + 1, o1, false);
                        stage(k + 2, o2, false);
                        stage(k + 3, o0, false);
                    } else if (left == 2) {
                        stage(k, o0, true);
                        stage(k + 1, o1, true);
                        stage(k + 2, o2, false);
                        stage(k + 3, o0, false);
                        stage(k + 4, o1, false);
                    } else {
                        stage(k, o0, false);
                        if (N >= 2) stage(k + 1, o1, false);
                        if (N >= 3) stage(k + 2, o2, false);
                    }
                    return;
                }
                // (the other models: the clamped prefetch, N mod 3 stages peeled in front)
                fetch(0, o0);
                fetch(N > 1 ? 1 : 0, o1);
                fetch(N > 2 ? 2 : 0, o2);
                // all three stages of the unrolled body unconditional (N mod 3 stages peeled in front, the buffers
                // rotate roles): the loop top then has the same outstanding loads on every path, so the wait before
                // stage k's operands is vmcnt(#loads of stages k+1, k+2), not vmcnt(0)
                if (N % 3 == 1) {
                    stage(0, o0);
                    for (int k = 1; k < N; k += 3) {
                        stage(k, o1);
                        stage(k + 1, o2);
                        stage(k + 2, o0);
                    }
                } else if (N % 3 == 2) {
                    stage(0, o0);
                    stage(1, o1);
                    for (int k = 2; k < N; k += 3) {
                        stage(k, o2);
                        stage(k + 1, o0);
                        stage(k + 2, o1);
                    }
                } else {
                    for (int k = 0; k < N; k += 3) {
                        stage(k, o0);
                        stage(k + 1, o1);
                        stage(k + 2, o2);
                    }
                }
            };
            if constexpr (MEHR) {
                // affine predictor step (the sweep above ran with b = 0): dy_aff in sDX | sDU
                step_dist(false);
                __builtin_amdgcn_wave_barrier();
                // stage-parallel: steps to the boundary without tau, mu = avg(s z), mu_aff at the end of those steps
                double ap = 1.0, ad = 1.0, sz = 0.0;
                for (int k = gl; k < N; k += G) {
#pragma unroll
                    for (int j = 0; j < NY; ++j) {
                        const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                        const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                        ip_aff_limits(y, dy, yl[j], yu[j], sZl[k * NY + j], sZu[k * NY + j], ap, ad, sz);
                    }
                }
                ap = group_min(ap);
                ad = group_min(ad);
                sz = group_sum(sz);
                double saff = 0.0;
                for (int k = gl; k < N; k += G) {
#pragma unroll
                    for (int j = 0; j < NY; ++j) {
                        const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                        const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                        saff += ip_aff_compl(y, dy, yl[j], yu[j], sZl[k * NY + j], sZu[k * NY + j], ap, ad);
                    }
                }
                saff = group_sum(saff);
                int nb = 0;   // finite bounds of one stage
#pragma unroll
                for (int j = 0; j < NY; ++j) nb += (yl[j] > -INFINITY) + (yu[j] < INFINITY);
                const double mbnd = (double)nb * (double)N;
                const double muc = sz / mbnd, mua = saff / mbnd;   // XB: at least one finite bound
                const double sig = muc > 0.0 ? pow(mua / muc, 3.0) : 0.0;
                // the target mu_t replaces the barrier parameter of this iteration (merit, duals, safeguard, trace)
                mub = fmax(kIpTolCompl / 20.0, fmin(sig * muc, kIpMu0));
                for (int k = gl; k < N; k += G) {
#pragma unroll
                    for (int j = 0; j < NY; ++j) {
                        const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                        const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                        double ccl, ccu, bb;
                        ip_corrector(y, dy, yl[j], yu[j], sZl[k * NY + j], sZu[k * NY + j], mub, ccl, ccu, bb);
                        sCl[k * NY + j] = ccl;
                        sCu[k * NY + j] = ccu;
                        sBb[k * NY + j] = bb;
                    }
                }
                // the corrected b of every stage visible to the other lanes' sweep
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                // corrector: the same stage matrices and factors with the corrected b -- only the vector part of the
                // recursion changes (backward_vec); the usual step sweep follows
                backward_vec();
            }
            for (int pass = 0;; ++pass) {
                if (pass > 0) {   // BOUNDED: controls held after the previous step -- solve the QP again
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    backward_dist(use_w);
                    if (EXACT && use_w && !fact_ok) {   // the held exact QP not positive definite: Gauss-Newton
                        fact_ok = 1;
                        use_w = false;
                        backward_dist(false);
                    }
                    if (!fact_ok) break;
                }
                resolve = false;
                // QP solves of this iteration: two at the first (the cold start's active set moves most there, and a
                // wave pays its slowest instance's solves), kBoundPasses later (oracle bound_release)
                const int passes = (it == 0 && !p.no_release) ? 2 : kBoundPasses;
                step_dist(BOUNDED && pass + 1 < passes);
                if constexpr (!BOUNDED) {
                    break;
                } else {
                    resolve = group_max(resolve ? 1.0 : 0.0) != 0.0;
                    if (!resolve || pass + 1 >= passes) break;
                }
            }
            __builtin_amdgcn_wave_barrier();
            // directional derivative of J along (dx, du), stage-parallel:
            // sum_k 2Q(F_k - r_k).(A dx_k + B du_k) + 2R(u_k - u_{k-1})(du_k - du_{k-1}) + 2Rm u_k du_k
            double dj = 0.0;
            for (int k0 = gl; k0 < N; k0 += WD * G) {   // (PAIR: the loads of two stages in flight together)
                double ef[WD][NX], ad[WD][NX], uk[WD][NU], duk[WD][NU], um[WD][NU], dum[WD][NU];
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
#pragma unroll
                    for (int q = 0; q < NX; ++q) {
                        ef[e][q] = sF[k * NX + q] - tr[k * NX + q];
                        ad[e][q] = sD[(k + 1) * NX + q];
                    }
#pragma unroll
                    for (int c = 0; c < NU; ++c) {
                        uk[e][c] = sU[k * NU + c];
                        duk[e][c] = sDU[k * NU + c];
                        um[e][c] = (k == 0) ? up[c] : sU[(k - 1) * NU + c];
                        dum[e][c] = (k == 0) ? 0.0 : sDU[(k - 1) * NU + c];
                    }
                }
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    double ds = dj;
#pragma unroll
                    for (int q = 0; q < NX; ++q) ds = fma(2.0 * Q[q] * ef[e][q], ad[e][q], ds);
#pragma unroll
                    for (int c = 0; c < NU; ++c)
                        ds = fma(2.0 * R[c] * (uk[e][c] - um[e][c]), duk[e][c] - dum[e][c], fma(2.0 * Rm[c] * uk[e][c], duk[e][c], ds));
                    dj = (e == 0 || k0 + e * G < N) ? ds : dj;
                }
            }
            dJ = group_sum(dj);
        } else {
            if (gl == 0) {
                for (int pass = 0;; ++pass) {
                    if (pass > 0) backward(pass);
                    if (!fact_ok) break;
                    resolve = false;
                    step_sweep(pass);
                    if (!BOUNDED || !resolve || pass + 1 >= kBoundPasses) break;
                }
            }
            fact_ok = group_bcast_i(fact_ok, gbase);
            dJ = group_bcast(dJ, gbase);
        }
        if (!fact_ok) {
            status = ST_FACT_FAILED;
            break;
        }
        __builtin_amdgcn_wave_barrier();
        MMPC_PHASE(4);
        // interior point: fraction to the boundary (primal alpha_max, dual alpha_z), barrier directional derivative
        double amax = 1.0, az = 1.0, dbar = 0.0;
        if constexpr (XB) {
            const double tau = kIpTau;
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NY; ++j) {
                    const double y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                    if constexpr (MEHR)
                        ip_step_limits_pc(y, dy, yl[j], yu[j], sZl[k * NY + j], sZu[k * NY + j], mub, tau,
                                          sCl[k * NY + j], sCu[k * NY + j], amax, az, dbar);
                    else
                        ip_step_limits(y, dy, yl[j], yu[j], sZl[k * NY + j], sZu[k * NY + j], mub, tau, sBb[k * NY + j],
                                       amax, az, dbar);
                }
            }
            amax = group_min(amax);
            az = group_min(az);
            dbar = group_sum(dbar);
        }

        // ---- D. stage-parallel l1-merit Armijo line search (noise-aware, as sqp_wave.h), update ----
        mu = fmax(mu, 4.0 * lmax + 1.0);
        const double phi0 = XB ? fma(mu, c1, fma(-2.0 * mub, lsum, J0)) : fma(mu, c1, J0);
        const double dphi = XB ? dJ + dbar - mu * c1 : dJ - mu * c1;
        double alpha = amax;
        bool accepted = false;
        // the alpha = 1 trial with the Jacobian (FUSE_FWD): ctm, nft are phase A's max|c| and nonfinite flag there
        double ctm = 0.0;
        int nft = 0;
        auto trial = [&](auto jac_c, double& Jt, double& ct, double& lt) {
            constexpr bool JAC = decltype(jac_c)::value;
            // two stages per lane in the fused trial; the trials after a rejected full step keep the one-stage loop (no
            // cfg#2 iteration runs them, and with nothing to store the compiler puts a pair's second evaluation behind a
            // branch on "the lane has a second stage" anyway)
            constexpr int WT = JAC ? WJ : 1;
            with_lin(std::integral_constant<int, WT>{}, [&](auto lm_c) {
                constexpr int LM = decltype(lm_c)::value;
                for (int k0 = gl; k0 < N; k0 += WT * G) {
                    int kk[WT];
                    double x[WT][NX], u[WT][NU], xd[WT][NX];
                    [[maybe_unused]] double Fq[WT][SQ], Fqd[WT][FD], Fu[WT][FU];
#pragma unroll
                    for (int e = 0; e < WT; ++e) {
                        const int k = kk[e] = (e == 0 || k0 + e * G < N) ? k0 + e * G : k0;
#pragma unroll
                        for (int r = 0; r < NX; ++r) x[e][r] = fma(alpha, sDX[k * NX + r], sX[k * NX + r]);
#pragma unroll
                        for (int c = 0; c < NU; ++c) {
                            u[e][c] = fma(alpha, sDU[k * NU + c], sU[k * NU + c]);
                            if (BOUNDED) u[e][c] = proj(u[e][c], lbv[c], ubv[c]);  // projected trial point
                        }
                    }
                    group_model_w<Model, WT, LM, JAC, SQ, FD, FU>(lin, lFq, lFqd, lFu, lxd, lxs, up, x, u, xd, Fq, Fqd, Fu);
                    double cd[WT][NX], er[WT][NX];
#pragma unroll
                    for (int e = 0; e < WT; ++e) {
                        const int k = kk[e];
                        if constexpr (JAC) {   // = phase A at the trial point (stored for the next iteration)
#pragma unroll
                            for (int i = 0; i < FQ; ++i) sFq[k * FQ + i] = h * Fq[e][i];
#pragma unroll
                            for (int i = 0; i < FD; ++i) sFqd[k * FD + i] = h * Fqd[e][i];
#pragma unroll
                            for (int i = 0; i < FU; ++i) sFu[k * FU + i] = h * Fu[e][i];
                        }
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double F = fma(h, xd[e][r], x[e][r]);
                            if constexpr (JAC) sF[k * NX + r] = F;
                            if constexpr (JAC) {
                                cd[e][r] = F - fma(alpha, sDX[(k + 1) * NX + r], sX[(k + 1) * NX + r]);
                                sC[k * NX + r] = cd[e][r];
                                er[e][r] = F - tr[k * NX + r];
                            } else {
                                er[e][r] = F - tr[k * NX + r];
                                cd[e][r] = F - fma(alpha, sDX[(k + 1) * NX + r], sX[(k + 1) * NX + r]);
                            }
                        }
                    }
                    // the sums in stage order; a repeated stage leaves them as they were
#pragma unroll
                    for (int e = 0; e < WT; ++e) {
                        const int k = kk[e];
                        double Js = Jt, cs = ct, ls = lt;
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            if constexpr (JAC) {
                                ctm = fmax(ctm, fabs(cd[e][r]));
                                cs += fabs(cd[e][r]);
                                nft |= !isfinite(cd[e][r]);
                                Js = fma(er[e][r] * Q[r], er[e][r], Js);
                            } else {
                                Js = fma(er[e][r] * Q[r], er[e][r], Js);
                                cs += fabs(cd[e][r]);
                            }
                        }
#pragma unroll
                        for (int c = 0; c < NU; ++c) {
                            double um = (k == 0) ? up[c] : fma(alpha, sDU[(k - 1) * NU + c], sU[(k - 1) * NU + c]);
                            if (BOUNDED && k > 0) um = proj(um, lbv[c], ubv[c]);
                            const double dif = u[e][c] - um;
                            Js = fma(dif * R[c], dif, fma(u[e][c] * Rm[c], u[e][c], Js));
                        }
                        if constexpr (XB) {
#pragma unroll
                            for (int j = 0; j < NY; ++j) {
                                const double y = j < NX ? fma(alpha, sDX[(k + 1) * NX + j], sX[(k + 1) * NX + j]) : u[e][j - NX];
                                ls += ip_log_slacks(y, yl[j], yu[j]);
                            }
                        }
                        const bool on = e == 0 || k0 + e * G < N;
                        Jt = on ? Js : Jt;
                        ct = on ? cs : ct;
                        lt = on ? ls : lt;
                    }
                }
            });
        };
        bool jac_trial = false;
        const FirstIterSwitch fsw = first_iter_switch(!XB && it == 0, c1, dJ);
        for (int ls = 0; ls < 30; ++ls) {
            double Jt = 0.0, ct = 0.0, lt = 0.0;
            jac_trial = FUSE_FWD && ls == 0;   // alpha = amax (1 without state bounds)
            if (jac_trial) trial(std::true_type{}, Jt, ct, lt);
            else trial(std::false_type{}, Jt, ct, lt);
            Jt = group_sum(Jt);
            ct = group_sum(ct);
            if (XB) lt = group_sum(lt);
            const double phit = XB ? fma(mu, ct, fma(-2.0 * mub, lt, Jt)) : fma(mu, ct, Jt);
            const double noise = 1.0 + fabs(phi0);
            if (dphi >= -1e-11 * noise || phit <= phi0 + 1e-4 * alpha * dphi + 1e-13 * noise ||
                (!XB && it == 0 && first_iter_filter_accepts(J0, c1, Jt, ct, alpha, fsw))) {
                accepted = true;
                if (FUSE_FWD && jac_trial) {   // the next iteration starts after phase A
                    fwd_ready = true;
                    J0n = Jt;
                    c1n = ct;
                    cmaxn = group_max(ctm);
                    nfn = nft;
                }
                break;
            }
            alpha *= 0.5;
        }
        if (trc && gl == 0) {
            trc[4] = XB ? amax : dJ;
            trc[5] = alpha;
            trc[6] = XB ? mub : mu;
            if (XB) trc[3] = cmpl0;
        }
        MMPC_PHASE(5);
        if (!accepted) {
            status = ST_LS_FAILED;
            break;
        }
        __builtin_amdgcn_wave_barrier();
        if constexpr (XB) {  // y and the duals of stage k's (x_{k+1} | u_k), as oracle solve_one_ip
            for (int k = gl; k < N; k += G) {
#pragma unroll
                for (int j = 0; j < NY; ++j) {
                    double& y = j < NX ? sX[(k + 1) * NX + j] : sU[k * NU + j - NX];
                    const double dy = j < NX ? sDX[(k + 1) * NX + j] : sDU[k * NU + j - NX];
                    double zl = sZl[k * NY + j], zu = sZu[k * NY + j], yn;
                    if constexpr (MEHR)
                        ip_update_pc(y, dy, yl[j], yu[j], zl, zu, mub, sCl[k * NY + j], sCu[k * NY + j], alpha, az, yn);
                    else
                        ip_update(y, dy, yl[j], yu[j], zl, zu, mub, alpha, az, yn);
                    y = yn;
                    sZl[k * NY + j] = zl;
                    sZu[k * NY + j] = zu;
                }
            }
            if constexpr (!MEHR) mub = mub_next;   // MEHR: no lagged update, mu_t is set in every iteration
        } else {
            // (PAIR: all loads of the two stages before their stores -- a repeated stage forms its new value from the old
            // one both times and stores it twice)
            for (int k0 = gl; k0 <= N; k0 += WD * G) {
                int kk[WD], ku[WD];
                double xn[WD][NX], un[WD][NU];
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = kk[e] = (e == 0 || k0 + e * G <= N) ? k0 + e * G : k0;
                    if constexpr (WD == 1) {
                        ku[e] = k;
                        if (k > 0) {
#pragma unroll
                            for (int r = 0; r < NX; ++r) xn[e][r] = fma(alpha, sDX[k * NX + r], sX[k * NX + r]);
                        }
                        if (k < N) {
#pragma unroll
                            for (int c = 0; c < NU; ++c) un[e][c] = fma(alpha, sDU[k * NU + c], sU[k * NU + c]);
                        }
                    } else {   // loads without lane tests: x_0 keeps its bytes by a select, k = N reads the u row of N - 1
                        ku[e] = k < N ? k : N - 1;
#pragma unroll
                        for (int r = 0; r < NX; ++r) {
                            const double xo = sX[k * NX + r];
                            xn[e][r] = k > 0 ? fma(alpha, sDX[k * NX + r], xo) : xo;
                        }
#pragma unroll
                        for (int c = 0; c < NU; ++c) un[e][c] = fma(alpha, sDU[ku[e] * NU + c], sU[ku[e] * NU + c]);
                    }
                }
                if constexpr (WD > 1) __builtin_amdgcn_wave_barrier();   // (compiler: no store of the pair above a load)
#pragma unroll
                for (int e = 0; e < WD; ++e) {
                    const int k = kk[e];
                    if (WD > 1 || k > 0) {
#pragma unroll
                        for (int r = 0; r < NX; ++r) sX[k * NX + r] = xn[e][r];
                    }
                    if (k < N) {   // (never the u row of another lane's stage: that lane updates it itself)
#pragma unroll
                        for (int c = 0; c < NU; ++c) sU[ku[e] * NU + c] = BOUNDED ? proj(un[e][c], lbv[c], ubv[c]) : un[e][c];
                    }
                }
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    MMPC_PHASE(6);
    if (!valid) return;
    // ---- write back V (reference layout), stage-parallel ----
    double* Vout = p.V + inst * (int64_t)NV;
    for (int k = gl; k <= N; k += G) {
#pragma unroll
        for (int r = 0; r < NX; ++r) Vout[k * ND + r] = sX[k * NX + r];
        if (k < N) {
#pragma unroll
            for (int c = 0; c < NU; ++c) Vout[k * ND + NX + c] = sU[k * NU + c];
        }
    }
    if (p.u0_out && gl < NU) p.u0_out[inst * NU + gl] = sU[gl];
    if (gl == 0) {
        if (p.status) p.status[inst] = status;
        if (p.iters) p.iters[inst] = it;
        if (p.kkt) p.kkt[inst] = kkt;
    }
    MMPC_PHASE(7);
    MMPC_PHASE_FLUSH
#endif  // MMPC_GROUP_PASS != 0
#if MMPC_GROUP_PASS == 1
}

// the interior-point variant under Mehrotra's predictor-corrector rule (state-bounded solves, nonlinear mode): the
// body above once more
template <class Model, bool EXACT = false>
__global__ __launch_bounds__(64) void sqp_group_mehrotra_kernel(SolveParams p, GroupWork gw) {
    constexpr bool BOUNDED = false, XB = true, MEHR = true;
    constexpr bool IB = false;
#define MMPC_GROUP_BODY_ONLY
#include "sqp_group.h"
#undef MMPC_GROUP_BODY_ONLY
}

// The bounded variants with PER-INSTANCE control bounds (mmpc_solve_batch_bounds, bounds_stride >= nu): the body once
// more with IB = true, where load_bounds / load_ip_bounds read row `inst` of u_lb / u_ub -- the instance, never the
// launch slot of a resume launch.  A kernel of its own and not a run-time stride in the kernels above: their bounds
// are wave-uniform scalar loads, and as per-lane values they cost the shared-bounds solves 3-10 %.
template <class Model, bool BOUNDED, bool XB, bool EXACT = false, bool MEHR = false>
__global__ __launch_bounds__(64) void sqp_group_instb_kernel(SolveParams p, GroupWork gw) {
    static_assert(BOUNDED || XB, "per-instance bounds: the bounded variants only");
    constexpr bool IB = true;
#define MMPC_GROUP_BODY_ONLY
#include "sqp_group.h"
#undef MMPC_GROUP_BODY_ONLY
}

}  // namespace mmpc
#endif  // MMPC_GROUP_PASS == 1
