"""CPU: the definition of the solve's forward-mode product (mmpc_solve_jvp_batch; include/mmpc.h).

dV = (d V* / d theta) d theta for theta = (x0, u_prev, traj, weights): the first-order update of the plan.  This
module is the numpy restatement of the definition, on stage_data / held_mask of tests/sens_reference.py:

* dense_jvp (tests/jvp_reference.py): the dense KKT solve with the definition's right-hand side (the reference of the
  GPU tests);
* riccati_jvp: the recursion of the header, term for term, and its forward sweep from s_0 = (dx0, du_prev) (what the
  kernel runs).

Setup: the four cases of tests/test_solve_vjp_reference.py (its `solved`: two instances each, oracle exact-Hessian
solves at tol_grad 1e-11 and tol_defect 1e-12; 2-link N = 1, 5 unbounded, N = 17 under +-2 Nm with 1 and 24 held
controls, exo N = 7) and standard normal tangents in all four inputs from default_rng(SEED + 101 N + b).

1. recursion against dense: 1e-12 max(1, |ref|), both Hessians, n_pin 0 and 1, du exactly 0 on held controls (two
   orderings of the same fp64 arithmetic; measured <= 3.3e-14).
2. the adjoint identity <V_bar, dV> = <x0_bar, dx0> + <u_prev_bar, du_prev> + <traj_bar, dtraj> + <weights_bar,
   dweights> against dense_vjp with the VJP module's V_bar: 1e-12 max(1, sum |V_bar o dV|), both Hessians, n_pin 0 and
   1 (two solves with one symmetric matrix; measured <= 5.9e-15 relative).
3. the oracle's own map: V* + t dV against warm-started re-solves at theta + t d theta, t = 2e-3, 1e-3, 5e-4, with
   dweights scaled to the weights' own sizes (relative_weight_tangent below).  The
   remainder is quadratic in t: the error's ratio per halving lies in [3, 5] (measured 3.98 - 4.00), and at t = 1e-3
   the error is at most 1e-2 of what the unchanged plan is off by (measured <= 9.0e-4; N = 17: 1.40e-6, 3.51e-7,
   8.76e-8 against a plan off by 1.8e-3 at t = 1e-3)."""
import numpy as np
import pytest

import oracle_lib as oracle
from jvp_reference import dense_jvp, rho, tangents
from sens_reference import dense_vjp, held_mask, stage_data
from test_solve_vjp_reference import CASES, SEED, H, solved


def riccati_jvp(model, N, h, V, up, tr, w, dx0, du_prev, dtraj, dweights, exact, lb=None, ub=None, n_pin=0):
    """dV by the recursion of the definition and its forward sweep, one instance"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = np.asarray(w, dtype=np.float64)
    R, Rm = w[nx:nx + nu], w[nx + nu:]
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, None if lb is None else np.asarray(lb, dtype=np.float64),
                     None if ub is None else np.asarray(ub, dtype=np.float64), n_pin)
    rh = rho(model, N, h, V, up, tr, w, A, B, dtraj, dweights)
    P = np.zeros((K, K))
    p = np.zeros(K)
    G, kff = np.zeros((N, nu, K)), np.zeros((N, nu))
    for k in range(N - 1, -1, -1):
        C = np.block([[A[k], B[k]], [np.zeros((nu, nx)), np.eye(nu)]])
        S = blocks[k].copy()   # S_k (+ W_k): the stage block without its Delta-u and Rm terms
        S[nx:, nx:] -= np.diag(2 * R + 2 * Rm + (2 * R if k + 1 < N else 0))
        Myy = C.T @ P @ C + S
        Muu = Myy[nx:, nx:] + np.diag(2 * R + 2 * Rm)
        Mus = np.hstack([Myy[nx:, :nx], -np.diag(2 * R)])
        Mss = np.zeros((K, K))
        Mss[:nx, :nx] = Myy[:nx, :nx]
        Mss[nx:, nx:] = np.diag(2 * R)
        q = C.T @ p + rh[k * K:(k + 1) * K]
        for c in np.flatnonzero(held[k]):
            Muu[c, :] = 0.0
            Muu[:, c] = 0.0
            Muu[c, c] = 1.0
            Mus[c, :] = 0.0
            q[nx + c] = 0.0
        G[k] = -np.linalg.solve(Muu, Mus)
        kff[k] = np.linalg.solve(Muu, q[nx:])
        p = np.concatenate([q[:nx], np.zeros(nu)]) + G[k].T @ q[nx:]
        P = Mss + Mus.T @ G[k]
    dV = np.zeros(V.size)
    s = np.concatenate([dx0, du_prev])
    dV[:nx] = dx0
    for k in range(N):
        du = G[k] @ s + kff[k]
        dV[k * K + nx:(k + 1) * K] = du
        dxn = A[k] @ s[:nx] + B[k] @ du
        dV[(k + 1) * K:(k + 1) * K + nx] = dxn
        s = np.concatenate([dxn, du])
    return dV


def case_tangents(model, N, b):
    return tangents(model, N, np.random.default_rng(SEED + 101 * N + b))


def pins(N):
    return sorted({0, min(1, N - 1)})


@pytest.mark.parametrize("model,N,bounds,n_held", CASES)
def test_recursion_matches_the_dense_kkt_solve(model, N, bounds, n_held):
    nx, nu = oracle.DIMS[model]
    w, lb, ub, x0, up, tr, V, _ = solved(model, N, bounds)
    worst = 0.0
    for b in range(2):
        assert int(held_mask(model, N, V[b], lb, ub, 0).sum()) == n_held[b]
        t = case_tangents(model, N, b)
        for exact in (True, False):
            for n_pin in pins(N):
                d = dense_jvp(model, N, H, V[b], up[b], tr[b], w, *t, exact, lb, ub, n_pin)
                r = riccati_jvp(model, N, H, V[b], up[b], tr[b], w, *t, exact, lb, ub, n_pin)
                err = np.abs(d - r).max()
                worst = max(worst, err / max(1.0, np.abs(d).max()))
                assert err <= 1e-12 * max(1.0, np.abs(d).max()), (b, exact, n_pin, err)
                held = held_mask(model, N, V[b], lb, ub, n_pin)
                for dv in (d, r):
                    assert (dv[:-nx].reshape(N, -1)[:, nx:][held] == 0.0).all()
                    assert np.array_equal(dv[:nx], t[0])
    print(f"recursion against dense, worst relative error: {worst:.3e}")


@pytest.mark.parametrize("model,N,bounds,n_held", CASES)
def test_adjoint_identity_against_the_dense_vjp(model, N, bounds, n_held):
    w, lb, ub, x0, up, tr, V, Vbar = solved(model, N, bounds)
    worst = 0.0
    for b in range(2):
        t = case_tangents(model, N, b)
        for exact in (True, False):
            for n_pin in pins(N):
                dV = riccati_jvp(model, N, H, V[b], up[b], tr[b], w, *t, exact, lb, ub, n_pin)
                v = dense_vjp(model, N, H, V[b], up[b], tr[b], w, Vbar[b], exact, lb, ub, n_pin)
                lhs = (Vbar[b] * dV).sum()
                rhs = sum((v[k] * d).sum() for k, d in zip(("x0_bar", "u_prev_bar", "traj_bar", "weights_bar"), t))
                scale = max(1.0, np.abs(Vbar[b] * dV).sum())
                worst = max(worst, abs(lhs - rhs) / scale)
                assert abs(lhs - rhs) <= 1e-12 * scale, (b, exact, n_pin, lhs, rhs)
    print(f"adjoint identity against dense_vjp, worst relative error: {worst:.3e}")


STEPS = (2e-3, 1e-3, 5e-4)


def relative_weight_tangent(t, w):
    """the tangents with dweights scaled entry by entry to the weights' own sizes, as fd_delta of
    tests/sens_reference.py scales a weight's step: V* depends on the weights through their ratios, and a unit tangent
    on Rm = 0.01 at t = 1e-3 would be a 10 % step, outside the range a first-order update is for"""
    return t[0], t[1], t[2], t[3] * w


@pytest.mark.parametrize("model,N,bounds,n_held", CASES)
def test_first_order_update_follows_the_oracles_resolves(model, N, bounds, n_held):
    nx, nu = oracle.DIMS[model]
    w, lb, ub, x0, up, tr, V, _ = solved(model, N, bounds)
    t4 = [relative_weight_tangent(case_tangents(model, N, b), w) for b in range(2)]
    dx0, dup, dtr, dw = (np.stack([t4[b][i] for b in range(2)]) for i in range(4))
    dV = np.stack([riccati_jvp(model, N, H, V[b], up[b], tr[b], w, *t4[b], True, lb, ub) for b in range(2)])
    err, off = [], []
    for t in STEPS:
        o = oracle.solve_batch(N, H, x0 + t * dx0, up + t * dup, tr + t * dtr, np.tile(w, (2, 1)) + t * dw, V=V,
                               u_lb=lb, u_ub=ub, model=model, hessian=oracle.HESS_EXACT, tol_grad=1e-11,
                               tol_defect=1e-12)
        assert (o["status"] == 0).all(), (t, o["status"])
        err.append(np.abs(o["V"] - (V + t * dV)).max(axis=1))
        off.append(np.abs(o["V"] - V).max(axis=1))
    err, off = np.array(err), np.array(off)
    for b in range(2):
        ratios = err[:-1, b] / err[1:, b]
        print(f"instance {b}: error of V* + t dV at t = {STEPS}: {err[:, b]}, ratios per halving {ratios}; "
              f"the unchanged plan is off by {off[:, b]}; update / plan at t = 1e-3: {err[1, b] / off[1, b]:.3e}")
        assert ((ratios >= 3.0) & (ratios <= 5.0)).all(), (b, err[:, b], ratios)
        assert err[1, b] <= 1e-2 * off[1, b], (b, err[1, b], off[1, b])
