"""CPU: the definition of the feedback gains and the solve VJP under the sensitivity barrier of a state-bounded handle
(mmpc_set_sensitivity_barrier; include/mmpc.h).

This module is the numpy restatement of the definition (xb_recursion); its dense reference (the other names below)
lives in tests/sens_reference.py; the GPU tests import both.

* barrier_terms: beta = 2 mu (1 / s_u - 1 / s_l) and D = min(2 mu (1 / s_l^2 + 1 / s_u^2), cap) of x_{k+1} and u_k;
* xb_stage_data: stage_data of tests/sens_reference.py with beta in the multiplier recursion
  (lam_{N-1} = beta(x_N), lam_{k-1} = A_k^T nu_k + beta(x_k); Gauss-Newton ignores beta);
* xb_recursion: the recursion of the header, term for term (P_{k+1}[x, x] += diag D(x_{k+1}) in place before C^T P C,
  M_uu += diag D(u_k)), the gains and every VJP output -- what the kernels run;
* xb_dense_gains: the tail system (tail_system) with Su_{j+1}^T D Su_{j+1} / Su_{j+1}^T D Sp_{j+1} added per stage and
  D_u on the control diagonal; xb_dense_vjp: the dense KKT solve (dense_vjp) with D added to L_zz.  No control is held by bit-equality; stages k < n_pin are held.

Inputs: oracle.synth(20250213, 0, B, N, 0.002) with the x0 velocities clipped (XB of test_gpu_bounded_shapes.py),
WEIGHTS_CFG / W_EXO, V* from oracle.solve_batch(x_lb=, x_ub=) with the exact Hessian at tol_grad 1e-11, tol_defect 1e-12.
Cases: 2-link (N, B) = (1, 5) (2, 3) (3, 9) (17, 9) (33, 9) under `box` (|qdot| <= 0.5), (17, 9) under `mixed+u`
(one-sided velocity bounds, u_1 >= -1, u_2 <= 1), exo (1, 5) (7, 9) under |qdot| <= 0.3.

1. arithmetic pin at sigma_cap = 1e6, mu_s default: recursion against dense <= 1e-10 max(1, |ref|) for the gains and
   every VJP output, both Hessians.  Every case with N >= 3 has an entry whose uncapped D >= 1e6 and a bounded entry
   with D < 1.
2. the test can tell: at the same cap the gains differ from the bound-free recursion by >= 1 in absolute value.
3. default settings (mu_f, 1e12): a measured floor, asserted at 10 x the value measured here (FLOOR below; the two
   sides are reorderings of the same ill-conditioned arithmetic, the factor covers a change of BLAS).
4. central path: on the N = 17 `box` batch the bound multipliers recovered from stationarity alone (the u rows give
   B_k^T nu_k, propagated backward) against 2 mu_f (1 / s_u - 1 / s_l) on every entry with a slack < 1e-6, asserted at
   10 x the worst relative deviation measured here (CENTRAL_PATH below).
5. derivative of the solve: central differences of cold oracle solves (delta = 1e-5, N = 17 `box`, six instances) against
   G_0 and against x0_bar / u_prev_bar for V_bar = e_{u_0, c}, asserted at 20 x the worst value measured here (FD below;
   the finite difference's own error is a comparable term).

Measured values (this module's prints) are recorded beside the constants they bound."""
import numpy as np
import pytest

import oracle_lib as oracle
from conftest import WEIGHTS_CFG
from sens_reference import (CAP_DEFAULT, OUT, _residuals, _weight_sums, barrier_terms, mu_f, xb_dense_gains,
                            stage_data, xb_dense_vjp, xb_stage_data)
from test_gpu_bounded_shapes import XB

H = 0.002
SEED = 20250213
W_2L = np.array(WEIGHTS_CFG)
W_EXO = np.array([10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4)
NAME = {oracle.TWO_LINK: "two_link_arm", oracle.EXO: "exo_arm"}
WEIGHTS = {oracle.TWO_LINK: W_2L, oracle.EXO: W_EXO}
CAP_PIN = 1e6
# (model, pattern, N, B)
CASES = [(oracle.TWO_LINK, "box", 1, 5), (oracle.TWO_LINK, "box", 2, 3), (oracle.TWO_LINK, "box", 3, 9),
         (oracle.TWO_LINK, "box", 17, 9), (oracle.TWO_LINK, "box", 33, 9), (oracle.TWO_LINK, "mixed+u", 17, 9),
         (oracle.EXO, "box", 1, 5), (oracle.EXO, "box", 7, 9)]
# the further shapes of the GPU tests, for their floors (3.)
FLOOR_CASES = CASES + [(oracle.TWO_LINK, "mixed+u", 1, 5), (oracle.TWO_LINK, "mixed+u", 2, 3),
                       (oracle.TWO_LINK, "mixed+u", 3, 9), (oracle.TWO_LINK, "mixed+u", 33, 9), (oracle.EXO, "box", 21, 9)]
# 3. recursion against dense at the default settings, worst err / max(1, |ref|) over gains and VJP outputs, both
# Hessians, as measured on the CPU by test_default_settings_floor (asserted at 10 x)
FLOOR = {
    (oracle.TWO_LINK, "box", 1): 1.46e-10,
    (oracle.TWO_LINK, "box", 2): 9.12e-10,
    (oracle.TWO_LINK, "box", 3): 6.05e-09,
    (oracle.TWO_LINK, "box", 17): 1.99e-08,
    (oracle.TWO_LINK, "box", 33): 9.79e-09,
    (oracle.TWO_LINK, "mixed+u", 17): 1.37e-08,
    (oracle.EXO, "box", 1): 1.08e-08,
    (oracle.EXO, "box", 7): 2.32e-08,
    (oracle.TWO_LINK, "mixed+u", 1): 7.02e-10,
    (oracle.TWO_LINK, "mixed+u", 2): 1.35e-09,
    (oracle.TWO_LINK, "mixed+u", 3): 1.31e-09,
    (oracle.TWO_LINK, "mixed+u", 33): 8.12e-09,
    (oracle.EXO, "box", 21): 3.73e-08,
}
# 4. worst |z - beta| / |beta| measured over the 68 entries with a slack < 1e-6: 0.574, at the first active entry of
# instance 0 (slack 1.0e-8).  64 of the 68 agree within 1 %, 51 within 1e-4: the interior point ends a barrier problem
# at E_mu <= 10 mu, so single multipliers may sit that far off mu / s while the plan's derivative (5.) agrees
CENTRAL_PATH = 0.574
# 5. worst err / max(1, |ref|) measured, G_0 and x0_bar | u_prev_bar alike: 5.381e-7
FD = 5.39e-7


def _id(case):
    return "-".join([NAME[case[0]]] + [str(v) for v in case[1:]])


def arr(v):
    return None if v is None else np.array(v, dtype=np.float64)


# ---------------------------------------------------------------- the definition
def xb_recursion(model, N, h, V, up, tr, w, Vbar, exact, xl, xu, ul=None, uu=None, n_pin=0, mu=None, cap=CAP_DEFAULT,
                 barrier=True):
    """the recursion of the definition, one instance: G [N, nu, K] and the VJP outputs for Vbar (None: zeros);
    barrier=False: the bound-free recursion at the same V"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = np.asarray(w, dtype=np.float64)
    mu = mu_f() if mu is None else mu
    Vbar = np.zeros(V.size) if Vbar is None else Vbar
    Q, R, Rm = w[:nx], w[nx:nx + nu], w[nx + nu:]
    bx, Dx, Du, _, _ = barrier_terms(model, N, V, xl, xu, ul, uu, n_pin, mu, cap)
    if not barrier:
        bx, Dx, Du = np.zeros_like(bx), np.zeros_like(Dx), np.zeros_like(Du)
    A, B, blocks = xb_stage_data(model, N, h, V, up, tr, w, exact, bx)
    P = np.zeros((K, K))
    p = np.concatenate([Vbar[N * K:], np.zeros(nu)])
    G, kff = np.zeros((N, nu, K)), np.zeros((N, nu))
    for k in range(N - 1, -1, -1):
        C = np.block([[A[k], B[k]], [np.zeros((nu, nx)), np.eye(nu)]])
        S = blocks[k].copy()   # S_k (+ W_k): the stage block without its Delta-u and Rm terms
        S[nx:, nx:] -= np.diag(2 * R + 2 * Rm + (2 * R if k + 1 < N else 0))
        P[np.arange(nx), np.arange(nx)] += Dx[k]
        Myy = C.T @ P @ C + S
        Muu = Myy[nx:, nx:] + np.diag(2 * R + 2 * Rm + Du[k])
        Mus = np.hstack([Myy[nx:, :nx], -np.diag(2 * R)])
        Mss = np.zeros((K, K))
        Mss[:nx, :nx] = Myy[:nx, :nx]
        Mss[nx:, nx:] = np.diag(2 * R)
        q = C.T @ p + Vbar[k * K:(k + 1) * K]
        if k < n_pin:
            Muu, Mus = np.eye(nu), np.zeros((nu, K))
            q[nx:] = 0.0
        L = np.linalg.cholesky(Muu)
        G[k] = -np.linalg.solve(L.T, np.linalg.solve(L, Mus))
        kff[k] = np.linalg.solve(L.T, np.linalg.solve(L, q[nx:]))
        p = np.concatenate([q[:nx], np.zeros(nu)]) + G[k].T @ q[nx:]
        P = Mss + Mus.T @ G[k]
    a = np.zeros(V.size)
    s = np.zeros(K)
    ax_next = np.zeros((N, nx))
    for k in range(N):
        au = G[k] @ s + kff[k]
        a[k * K + nx:(k + 1) * K] = au
        ax_next[k] = A[k] @ s[:nx] + B[k] @ au
        a[(k + 1) * K:(k + 1) * K + nx] = ax_next[k]
        s = np.concatenate([ax_next[k], au])
    e = _residuals(model, N, h, V, tr)
    return dict(G=G, x0_bar=p[:nx], u_prev_bar=p[nx:], traj_bar=2 * Q[None, :] * ax_next,
                weights_bar=_weight_sums(model, N, V, up, e, a, ax_next), adj_V=a)


# ---------------------------------------------------------------- the cases
_solved = {}


def case_inputs(model, pat, N, B):
    """(xl, xu, ul, uu), (x0, up, tr) of a case: the synth batch with the x0 velocities clipped"""
    nx, _ = oracle.DIMS[model]
    xl, xu, ul, uu, clip = XB[NAME[model]][pat]
    x0, up, tr = oracle.synth(SEED, 0, B, N, H, model=model)
    x0[:, nx // 2:] = np.clip(x0[:, nx // 2:], -clip, clip)
    return (arr(xl), arr(xu), arr(ul), arr(uu)), (x0, up, tr)


def tight_solve(model, N, x0, up, tr, bounds, **kw):
    xl, xu, ul, uu = bounds
    return oracle.solve_batch(N, H, x0, up, tr, WEIGHTS[model], u_lb=ul, u_ub=uu, x_lb=xl, x_ub=xu, model=model,
                              hessian=oracle.HESS_EXACT, tol_grad=1e-11, tol_defect=1e-12, **kw)


def solved(case):
    """bounds, inputs, the oracle's V* [B, NV] and a random V_bar of a case, computed once and left unchanged"""
    if case not in _solved:
        model, pat, N, B = case
        bounds, (x0, up, tr) = case_inputs(model, pat, N, B)
        o = tight_solve(model, N, x0, up, tr, bounds)
        assert (o["status"] == 0).all(), o["status"]
        Vbar = np.random.default_rng(SEED + N).standard_normal(o["V"].shape)
        for a in (x0, up, tr, o["V"], Vbar):
            a.setflags(write=False)
        _solved[case] = (bounds, x0, up, tr, o["V"], Vbar)
    return _solved[case]


def recursion_against_dense(case, cap):
    """worst err / max(1, |ref|) over the instances, both Hessians, the gains and every VJP output"""
    model, pat, N, B = case
    (xl, xu, ul, uu), x0, up, tr, V, Vbar = solved(case)
    w = WEIGHTS[model]
    worst = {}
    for b in range(B):
        for exact in (True, False):
            r = xb_recursion(model, N, H, V[b], up[b], tr[b], w, Vbar[b], exact, xl, xu, ul, uu, cap=cap)
            d = xb_dense_vjp(model, N, H, V[b], up[b], tr[b], w, Vbar[b], exact, xl, xu, ul, uu, cap=cap)
            d["G"] = xb_dense_gains(model, N, H, V[b], up[b], tr[b], w, exact, xl, xu, ul, uu, cap=cap)
            for k in ("G",) + OUT:
                worst[k] = max(worst.get(k, 0.0), np.abs(d[k] - r[k]).max() / max(1.0, np.abs(d[k]).max()))
    return worst


# ---------------------------------------------------------------- 1. the arithmetic pin
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_recursion_matches_dense_at_cap_1e6(case):
    model, pat, N, B = case
    (xl, xu, ul, uu), x0, up, tr, V, Vbar = solved(case)
    if N >= 3:
        raw = np.concatenate([barrier_terms(model, N, V[b], xl, xu, ul, uu, 0, mu_f(), CAP_PIN)[3] for b in range(B)])
        print(f"{_id(case)}: {int((raw >= CAP_PIN).sum())} capped entries of {raw.size}, {int((raw < 1).sum())} with "
              f"D < 1, largest D {raw.max():.2e}")
        assert (raw >= CAP_PIN).any() and (raw < 1.0).any()
    worst = recursion_against_dense(case, CAP_PIN)
    print(f"{_id(case)} cap 1e6: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-10, worst


# ---------------------------------------------------------------- 2. the test can tell
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == oracle.TWO_LINK and c[1] == "box" and c[2] >= 3], ids=_id)
def test_gains_differ_from_the_bound_free_recursion(case):
    model, pat, N, B = case
    (xl, xu, ul, uu), x0, up, tr, V, Vbar = solved(case)
    gap = 0.0
    for b in range(B):
        on = xb_recursion(model, N, H, V[b], up[b], tr[b], W_2L, None, True, xl, xu, ul, uu, cap=CAP_PIN)["G"]
        off = xb_recursion(model, N, H, V[b], up[b], tr[b], W_2L, None, True, xl, xu, ul, uu, barrier=False)["G"]
        gap = max(gap, np.abs(on - off).max())
    print(f"{_id(case)}: barrier against bound-free gains, largest difference {gap:.1f}")
    assert gap >= 1.0


# ---------------------------------------------------------------- 3. the default settings
@pytest.mark.parametrize("case", FLOOR_CASES, ids=_id)
def test_default_settings_floor(case):
    worst = recursion_against_dense(case, CAP_DEFAULT)
    print(f"{_id(case)} defaults: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 10 * FLOOR[case[:3]], worst


# ---------------------------------------------------------------- 4. the central path
def stationarity_multipliers(model, N, h, V, up, tr, w, bounded):
    """z(x_{k+1}) [N, nx] on the `bounded` components from stationarity alone: the u rows,
    B_k^T nu_k + dJ/du_k = 0 with nu_k = 2 Q e_k + A_{k+1}^T nu_{k+1} + z(x_{k+1}), backward from k = N - 1
    (no control bound; as many bounded components as controls, the rows of B_k they select invertible)"""
    nx, nu = oracle.DIMS[model]
    Q, R, Rm = w[:nx], w[nx:nx + nu], w[nx + nu:]
    A, B, _ = stage_data(model, N, h, V, up, tr, w, False)
    e = _residuals(model, N, h, V, tr)
    U = V[:-nx].reshape(N, nx + nu)[:, nx:]
    Uprev = np.vstack([up[None, :], U[:-1]])
    z = np.zeros((N, nx))
    nu_next = None
    for k in range(N - 1, -1, -1):
        gu = 2 * R * (U[k] - Uprev[k]) + 2 * Rm * U[k] - (2 * R * (U[k + 1] - U[k]) if k + 1 < N else 0.0)
        t = 2 * Q * e[k] + (A[k + 1].T @ nu_next if nu_next is not None else 0.0)
        z[k, bounded] = np.linalg.solve(B[k][bounded].T, -gu - B[k].T @ t)
        nu_next = t + z[k]
    return z


def test_returned_plan_is_on_the_central_path_of_mu_f():
    case = (oracle.TWO_LINK, "box", 17, 9)
    model, pat, N, B = case
    (xl, xu, ul, uu), x0, up, tr, V, Vbar = solved(case)
    bounded = np.isfinite(xl) | np.isfinite(xu)
    worst, n = 0.0, 0
    for b in range(B):
        z = stationarity_multipliers(model, N, H, V[b], up[b], tr[b], W_2L, bounded)
        X = np.stack([V[b][(k + 1) * 6:(k + 1) * 6 + 4] for k in range(N)])
        sl, su = X - xl[None, :], xu[None, :] - X
        beta = 2 * mu_f() * (1 / su - 1 / sl)
        act = np.minimum(sl, su) < 1e-6
        n += int(act.sum())
        if act.any():
            worst = max(worst, (np.abs(z - beta)[act] / np.abs(beta)[act]).max())
    print(f"central path: {n} entries with a slack < 1e-6, worst |z - beta| / |beta| = {worst:.3e}")
    assert n >= 10
    assert worst <= 10 * CENTRAL_PATH


# ---------------------------------------------------------------- 5. the derivative of the solve
def fd_of_solves(solve, x0, up, nx, nu, delta=1e-5):
    """central differences of u_0* of cold solves in every direction of (x0, u_prev): [B, nu, nx + nu]"""
    fd = np.zeros((x0.shape[0], nu, nx + nu))
    for i in range(nx + nu):
        u0 = []
        for sign in (1.0, -1.0):
            xs, us = x0.copy(), up.copy()
            (xs if i < nx else us)[:, i if i < nx else i - nx] += sign * delta
            u0.append(solve(xs, us)[:, nx:nx + nu])
        fd[:, :, i] = (u0[0] - u0[1]) / (2 * delta)
    return fd


def fd_errors(fd, G0, bars):
    """worst err / max(1, |ref|) of the central differences against G_0 [B, nu, K] and against
    bars[c] = (x0_bar | u_prev_bar) [B, K] for V_bar = e_{u_0, c}"""
    eg = (np.abs(fd - G0).max(axis=(1, 2)) / np.maximum(1.0, np.abs(G0).max(axis=(1, 2)))).max()
    eb = max((np.abs(fd[:, c] - bars[c]).max(axis=1) / np.maximum(1.0, np.abs(bars[c]).max(axis=1))).max()
             for c in range(fd.shape[1]))
    return eg, eb


def test_recursion_is_the_derivative_of_the_oracles_solve():
    model, pat, N, B = oracle.TWO_LINK, "box", 17, 6
    nx, nu = 4, 2
    bounds, (x0, up, tr) = case_inputs(model, pat, N, B)
    xl, xu, ul, uu = bounds

    def solve(xs, us):
        o = tight_solve(model, N, xs, us, tr, bounds)
        assert (o["status"] == 0).all(), o["status"]
        return o["V"]

    V = solve(x0, up)
    G0 = np.zeros((B, nu, nx + nu))
    bars = np.zeros((nu, B, nx + nu))
    for b in range(B):
        G0[b] = xb_recursion(model, N, H, V[b], up[b], tr[b], W_2L, None, True, xl, xu)["G"][0]
        for c in range(nu):
            Vbar = np.zeros(V.shape[1])
            Vbar[nx + c] = 1.0
            r = xb_recursion(model, N, H, V[b], up[b], tr[b], W_2L, Vbar, True, xl, xu)
            bars[c, b] = np.concatenate([r["x0_bar"], r["u_prev_bar"]])
    eg, eb = fd_errors(fd_of_solves(solve, x0, up, nx, nu), G0, bars)
    print(f"central differences of cold oracle solves: against G_0 {eg:.3e}, against x0_bar | u_prev_bar {eb:.3e}")
    assert max(eg, eb) <= 20 * FD
