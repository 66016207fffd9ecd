"""CPU: the definition of the solve's reverse-mode product (mmpc_solve_vjp_batch; include/mmpc.h).

This module is the numpy restatement of the definition, on stage_data / held_mask of tests/sens_reference.py:

* dense_vjp: the dense KKT solve for (a, b) -- L_zz a + g_z^T b = V_bar_z, g_z a = 0 with a = 0 on x_0 and on held
  controls -- and every output by the implicit function theorem from the dense blocks (the reference of the GPU tests);
* riccati_vjp: the recursion of the header, term for term, and its forward sweep (what the kernel runs).

Setup: two instances each of oracle.synth(20250213, 0, 2, N, 0.002), oracle exact-Hessian solves at tol_grad 1e-11 and
tol_defect 1e-12, a random normal V_bar; 2-link N = 1, 5 unbounded, N = 17 under +-2 Nm (1 and 24 held controls), exo
N = 7.

1. recursion against dense: 1e-12 max(1, |ref|) per output array, both Hessians, and with one committed stage
   (two orderings of the same fp64 arithmetic; measured <= 2.9e-14).
2. the solver's own map: central differences of the oracle's solves in 3 entries of each of x0, u_prev, traj and the
   weights (2 of u_prev on the 2-link arm, which has no more), delta = 1e-4 relative (fd_delta), warm-started from V*,
   against the exact recursion at 1e-6 max(1, |ref|) (DESIGN.md 3i item 5's tolerance; measured <= 8.1e-10)."""
import numpy as np
import pytest

import oracle_lib as oracle
from conftest import WEIGHTS_CFG
from sens_reference import OUT, _residuals, _weight_sums, dense_vjp, fd_delta, held_mask, stage_data

H = 0.002
SEED = 20250213
W_2L = np.array(WEIGHTS_CFG)
W_EXO = np.array([10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4)


def riccati_vjp(model, N, h, V, up, tr, w, Vbar, exact, lb=None, ub=None, n_pin=0):
    """every output by the recursion of the definition and its forward sweep, one instance"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = np.asarray(w, dtype=np.float64)
    Q, R, Rm = w[:nx], w[nx:nx + nu], w[nx + nu:]
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, None if lb is None else np.asarray(lb, dtype=np.float64),
                     None if ub is None else np.asarray(ub, dtype=np.float64), n_pin)
    P = np.zeros((K, K))
    p = np.concatenate([Vbar[N * K:], np.zeros(nu)])
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
        q = C.T @ p + Vbar[k * K:(k + 1) * K]
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
    return dict(x0_bar=p[:nx], u_prev_bar=p[nx:], traj_bar=2 * Q[None, :] * ax_next,
                weights_bar=_weight_sums(model, N, V, up, e, a, ax_next), adj_V=a)


# ---------------------------------------------------------------- the cases
PM2 = (np.array([-2.0, -2.0]), np.array([2.0, 2.0]))
CASES = [(oracle.TWO_LINK, 1, None, (0, 0)), (oracle.TWO_LINK, 5, None, (0, 0)), (oracle.TWO_LINK, 17, PM2, (1, 24)),
         (oracle.EXO, 7, None, (0, 0))]
_solved = {}


def solved(model, N, bounds):
    """the inputs, the oracle's V* [2, NV] and V_bar of a case, computed once"""
    key = (model, N, bounds is not None)
    if key not in _solved:
        w = W_EXO if model == oracle.EXO else W_2L
        lb, ub = bounds if bounds else (None, None)
        x0, up, tr = oracle.synth(SEED, 0, 2, N, H, model=model)
        o = oracle.solve_batch(N, H, x0, up, tr, w, u_lb=lb, u_ub=ub, model=model, hessian=oracle.HESS_EXACT,
                               tol_grad=1e-11, tol_defect=1e-12)
        assert (o["status"] == 0).all(), o["status"]
        Vbar = np.random.default_rng(SEED + N).standard_normal(o["V"].shape)
        for arr in (x0, up, tr, o["V"], Vbar):
            arr.setflags(write=False)
        _solved[key] = (w, lb, ub, x0, up, tr, o["V"], Vbar)
    return _solved[key]


@pytest.mark.parametrize("model,N,bounds,n_held", CASES)
def test_recursion_matches_the_dense_kkt_solve(model, N, bounds, n_held):
    w, lb, ub, x0, up, tr, V, Vbar = solved(model, N, bounds)
    worst = 0.0
    for b in range(2):
        assert int(held_mask(model, N, V[b], lb, ub, 0).sum()) == n_held[b]
        for exact in (True, False):
            for n_pin in sorted({0, min(1, N - 1)}):
                d = dense_vjp(model, N, H, V[b], up[b], tr[b], w, Vbar[b], exact, lb, ub, n_pin)
                r = riccati_vjp(model, N, H, V[b], up[b], tr[b], w, Vbar[b], exact, lb, ub, n_pin)
                for k in OUT:
                    err = np.abs(d[k] - r[k]).max()
                    worst = max(worst, err / max(1.0, np.abs(d[k]).max()))
                    assert err <= 1e-12 * max(1.0, np.abs(d[k]).max()), (k, b, exact, n_pin, err)
                held = held_mask(model, N, V[b], lb, ub, n_pin)
                aU = r["adj_V"][:-oracle.DIMS[model][0]].reshape(N, -1)[:, oracle.DIMS[model][0]:]
                assert (aU[held] == 0.0).all()
                if n_pin:
                    assert (r["u_prev_bar"] == 0.0).all() and (d["u_prev_bar"] == 0.0).all()
    print(f"recursion against dense, worst relative error: {worst:.3e}")


@pytest.mark.parametrize("model,N,bounds,n_held", CASES)
def test_recursion_is_the_derivative_of_the_oracles_solve(model, N, bounds, n_held):
    nx, nu = oracle.DIMS[model]
    w, lb, ub, x0, up, tr, V, Vbar = solved(model, N, bounds)
    ref = [riccati_vjp(model, N, H, V[b], up[b], tr[b], w, Vbar[b], True, lb, ub) for b in range(2)]
    pick = lambda n: sorted({0, n // 2, n - 1})  # noqa: E731
    # stage 0's position targets do not move V* (x_1's positions follow from x_0 alone): start at a velocity target
    tpick = sorted({nx // 2, N * nx // 2, N * nx - 1})
    inputs = {"x0_bar": (x0, pick(nx)), "u_prev_bar": (up, pick(nu)), "traj_bar": (tr.reshape(2, -1), tpick),
              "weights_bar": (np.tile(w, (2, 1)), [1, nx, nx + 2 * nu - 1])}
    worst = 0.0
    for name, (theta, idx) in inputs.items():
        for i in idx:
            delta = fd_delta(name, theta[:, i])
            Vs = []
            for sign in (1.0, -1.0):
                args = dict(x0_bar=x0, u_prev_bar=up, traj_bar=tr.reshape(2, -1), weights_bar=np.tile(w, (2, 1)))
                t = args[name].copy()
                t[:, i] += sign * delta
                args[name] = t
                o = oracle.solve_batch(N, H, args["x0_bar"], args["u_prev_bar"], args["traj_bar"].reshape(2, N, nx),
                                       args["weights_bar"], V=V, u_lb=lb, u_ub=ub, model=model,
                                       hessian=oracle.HESS_EXACT, tol_grad=1e-11, tol_defect=1e-12)
                assert (o["status"] == 0).all(), (name, i, o["status"])
                Vs.append(o["V"])
            fd = ((Vs[0] - Vs[1]) * Vbar).sum(1) / (2 * delta)
            for b in range(2):
                got = ref[b][name].reshape(-1)[i]
                err = abs(fd[b] - got) / max(1.0, np.abs(ref[b][name]).max())
                worst = max(worst, err)
                assert err <= 1e-6, (name, i, b, fd[b], got)
    print(f"central differences of the oracle's solves against the recursion, worst relative error: {worst:.3e}")
