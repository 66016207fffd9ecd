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
// This header holds the declarations and the three __global__ templates (end of the file).  The kernel body is one
// text, sqp_group_body.inc and the phase files it includes (kernel text, not headers), compiled into each of them by
// inclusion, so that the kernels of the monotone barrier rule keep exactly the code they had before the others existed.
#ifndef MMPC_SQP_GROUP_H
#define MMPC_SQP_GROUP_H
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
    constexpr int NX = Model::NX, NS = Model::NX + Model::NU;
    for (int r = 0; r < NX; ++r)
        for (int j = 0; j < NS; ++j) {
            if (P::idx(r, j) < 0) continue;
            if (P::idx(r, j) >= P::PK || P::idx(r, j) != P::col(r) + P::col(j)) return false;
            for (int r2 = 0; r2 < NX; ++r2)
                for (int j2 = 0; j2 < NS; ++j2)
                    if (P::idx(r2, j2) == P::idx(r, j) && !((r2 == r && j2 == j) || (r2 == j && j2 == r))) return false;
        }
    return P::OVER == P::col(NX - 1) + P::col(NS - 1) - (P::PK - 1);
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
// The layout itself: offsets in doubles from the instance's block (sX), in the order of the arrays; `doubles` is the
// size of the block and the stride from one group's block to the next.  The host's launch size (mmpc.hip
// group_lds_instance_bytes), the cfg#2 budget below and tests/test_group_lds_layout.py read this function.
struct GroupLds {
    int U, D, DX, DU, F, C, Fq, Fqd, Fu, R, Hold, Lin, Kh, Kc, doubles;
};
__host__ __device__ constexpr GroupLds group_lds(int nx, int nu, int nq, int N, bool bounded, bool linear, int kc,
                                                 int kh) {
    const int na = nx - nq;
    GroupLds L{};
    L.U = (N + 1) * nx;              // sX [N+1][nx]
    L.D = L.U + N * nu;              // sU [N][nu]
    L.DX = L.D + (N + 1) * nx;       // sD [N+1][nx]
    L.DU = L.DX + (N + 1) * nx;      // sDX [N+1][nx]
    L.F = L.DU + N * nu;             // sDU [N][nu]
    L.C = L.F + N * nx;              // sF [N][nx]
    L.Fq = L.C + N * nx;             // sC [N][nx]
    L.Fqd = L.Fq + N * na * nq;      // sFq [N][na nq]
    L.Fu = L.Fqd + N * na * na;      // sFqd [N][na na]
    L.R = L.Fu + N * na * nu;        // sFu [N][na nu]
    L.Hold = L.R + N * nx;           // sR [N][nx]
    L.Lin = L.Hold + (bounded ? N * nu : 0);   // sHold [N][nu], bounded solves only
    // the linear-mode block (Fq | Fqd | Fu | xdot), then the tail pad where the arrays behind sFqd are shorter than
    // the d recursion's over-read of it (above)
    L.Kh = L.Lin + (linear ? na * (nq + na + nu) + nx : 0) + (N * (na * nu + nx) >= 2 * na * na ? 0 : 2 * na * na);
    L.Kc = L.Kh + kh;
    L.doubles = L.Kc + kc;
    return L;
}
// The kernel body (sqp_group_body.inc) does not read the struct: formed from it, the views changed the instruction
// streams of every 16-lane kernel.  It keeps its pointer chain sX -> sU -> ... -> sLin, takes the group
// stride from this closed formula and sKc, sKh from the block's end.  group_lds_chain_ok checks group_lds against the
// closed forms of that chain as typed below, not against the chain's text in the kernel: whoever edits the chain
// edits both.
__host__ __device__ constexpr int group_lds_doubles(int nx, int nu, int nq, int N, bool bounded, bool linear, int kc,
                                                   int kh) {
    return N * (3 * nx + (nx - nq) * (nq + (nx - nq) + nu) + 2 * nu) + 3 * (N + 1) * nx + (bounded ? N * nu : 0) +
           (linear ? (nx - nq) * (nq + (nx - nq) + nu) + nx : 0) +
           (N * ((nx - nq) * nu + nx) >= 2 * (nx - nq) * (nx - nq) ? 0 : 2 * (nx - nq) * (nx - nq)) + kh + kc;
}
// the closed forms of what the kernel's chain reaches (its anchors sU, sF, sFq, sR, sLin), its stride, sKc = end - kc and
// sKh = sKc - kh, against the struct
__host__ __device__ constexpr bool group_lds_chain_ok(int nx, int nu, int nq, int N, bool bounded, bool linear, int kc,
                                                     int kh) {
    const GroupLds L = group_lds(nx, nu, nq, N, bounded, linear, kc, kh);
    const int na = nx - nq, total = group_lds_doubles(nx, nu, nq, N, bounded, linear, kc, kh);
    return L.U == (N + 1) * nx && L.F == 3 * (N + 1) * nx + 2 * N * nu && L.Fq == L.F + 2 * N * nx &&
           L.R == L.Fq + N * na * (nq + na + nu) && L.Lin == L.R + N * nx + (bounded ? N * nu : 0) &&
           L.doubles == total && L.Kc == total - kc && L.Kh == total - kc - kh && L.Kh >= L.Lin;
}
static_assert(group_lds_chain_ok(4, 2, 2, 30, false, false, 8, 42) && group_lds_chain_ok(4, 2, 2, 30, true, false, 8, 0) &&
                  group_lds_chain_ok(4, 2, 2, 30, false, true, 8, 42) && group_lds_chain_ok(4, 2, 2, 1, true, true, 8, 0),
              "cfg#2 shapes: the kernel's chain and group_lds");
static_assert(group_lds_chain_ok(8, 4, 4, 50, false, false, 0, 0) && group_lds_chain_ok(8, 4, 4, 26, true, false, 0, 0) &&
                  group_lds_chain_ok(8, 4, 4, 1, false, true, 0, 0) && group_lds_chain_ok(8, 4, 4, 1, true, false, 0, 0),
              "exo shapes (N = 1: padded): the kernel's chain and group_lds");
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
// The unbounded kernels of a model with per-lane sweep operands keep K | kff of stages 0 .. 2 in LDS (group_lds,
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
static_assert(kGroupsPerWave * group_lds(4, 2, 2, 30, false, false, GroupLaneOps<TwoLinkArm>::doubles,
                                         group_head_doubles(4, 2)).doubles * 8 <= 40960,
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
#include "sqp_group_body.inc"
}

// the interior-point variant under Mehrotra's predictor-corrector rule (state-bounded solves, nonlinear mode): the
// body once more
template <class Model, bool EXACT = false>
__global__ __launch_bounds__(64) void sqp_group_mehrotra_kernel(SolveParams p, GroupWork gw) {
    constexpr bool BOUNDED = false, XB = true, MEHR = true;
    constexpr bool IB = false;
#include "sqp_group_body.inc"
}

// The bounded variants with PER-INSTANCE control bounds (mmpc_solve_batch_bounds, bounds_stride >= nu): the body once
// more with IB = true, where load_bounds / load_ip_bounds read row `inst` of u_lb / u_ub -- the instance, never the
// launch slot of a resume launch.  A kernel of its own and not a run-time stride in the kernels above: their bounds
// are wave-uniform scalar loads, and as per-lane values they cost the shared-bounds solves 3-10 %.
template <class Model, bool BOUNDED, bool XB, bool EXACT = false, bool MEHR = false>
__global__ __launch_bounds__(64) void sqp_group_instb_kernel(SolveParams p, GroupWork gw) {
    static_assert(BOUNDED || XB, "per-instance bounds: the bounded variants only");
    constexpr bool IB = true;
#include "sqp_group_body.inc"
}

}  // namespace mmpc
#endif  // MMPC_SQP_GROUP_H
