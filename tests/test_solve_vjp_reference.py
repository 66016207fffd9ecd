"""CPU: the definition of the solve's reverse-mode product (mmpc_solve_vjp_batch; include/mmpc.h).

This module is the numpy restatement of the definition, on stage_data / held_mask of tests/test_gpu_feedback_gains.py:

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
from test_gpu_feedback_gains import _jac, held_mask, stage_data

H = 0.002
SEED = 20250213
W_2L = np.array(WEIGHTS_CFG)
W_EXO = np.array([10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4)
OUT = ("x0_bar", "u_prev_bar", "traj_bar", "weights_bar", "adj_V")


def _residuals(model, N, h, V, tr):
    """e_k = F(x_k, u_k) - r_k [N, nx]"""
    nx, nu = oracle.DIMS[model]
    Vs = V[:-nx].reshape(N, nx + nu)
    return np.stack([Vs[k, :nx] + h * _jac(model, Vs[k, :nx], Vs[k, nx:])[2] - tr[k] for k in range(N)])


def _weight_sums(model, N, V, up, e, a, ax_next):
    """(Q_bar | R_bar | Rm_bar) from the direction a [NV] and a_{x,k+1} [N, nx]"""
    nx, nu = oracle.DIMS[model]
    U = V[:-nx].reshape(N, nx + nu)[:, nx:]
    aU = a[:-nx].reshape(N, nx + nu)[:, nx:]
    dU = U - np.vstack([up[None, :], U[:-1]])
    daU = aU - np.vstack([np.zeros((1, nu)), aU[:-1]])
    return np.concatenate([-2 * (e * ax_next).sum(0), -2 * (dU * daU).sum(0), -2 * (U * aU).sum(0)])


def dense_vjp(model, N, h, V, up, tr, w, Vbar, exact, lb=None, ub=None, n_pin=0):
    """every output of the definition for one instance, from one dense KKT solve"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    NV = V.size
    w = np.asarray(w, dtype=np.float64)
    Q, R = w[:nx], w[nx:nx + nu]
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, None if lb is None else np.asarray(lb, dtype=np.float64),
                     None if ub is None else np.asarray(ub, dtype=np.float64), n_pin)
    Hm = np.zeros((NV, NV))   # L_VV: the stage blocks and the -2R couplings of consecutive controls
    Gz = np.zeros((N * nx, NV))   # the defects' Jacobian: F(x_k, u_k) - x_{k+1}
    for k in range(N):
        Hm[k * K:(k + 1) * K, k * K:(k + 1) * K] = blocks[k]
        Gz[k * nx:(k + 1) * nx, k * K:(k + 1) * K] = np.hstack([A[k], B[k]])
        Gz[k * nx + np.arange(nx), (k + 1) * K + np.arange(nx)] = -1.0
        if k >= 1:
            i, j = k * K + nx + np.arange(nu), (k - 1) * K + nx + np.arange(nu)
            Hm[i, j] -= 2 * R
            Hm[j, i] -= 2 * R
    free = np.ones(NV, bool)
    free[:nx] = False
    for k in range(N):
        free[k * K + nx:(k + 1) * K] = ~held[k]
    nf, ng = int(free.sum()), N * nx
    KKT = np.zeros((nf + ng, nf + ng))
    KKT[:nf, :nf] = Hm[np.ix_(free, free)]
    KKT[nf:, :nf] = Gz[:, free]
    KKT[:nf, nf:] = Gz[:, free].T
    sol = np.linalg.solve(KKT, np.concatenate([Vbar[free], np.zeros(ng)]))
    a = np.zeros(NV)
    a[free] = sol[:nf]
    b = sol[nf:]
    # theta_bar = V_bar_theta - (d grad_z L / d theta)^T a - (d g / d theta)^T b
    x0_bar = Vbar[:nx] - Hm[:, :nx].T @ a - Gz[:, :nx].T @ b
    u_prev_bar = 2 * R * a[nx:K]
    ax_next = np.stack([np.hstack([A[k], B[k]]) @ a[k * K:(k + 1) * K] for k in range(N)])   # J_k a_{y,k}
    e = _residuals(model, N, h, V, tr)
    return dict(x0_bar=x0_bar, u_prev_bar=u_prev_bar, traj_bar=2 * Q[None, :] * ax_next,
                weights_bar=_weight_sums(model, N, V, up, e, a, ax_next), adj_V=a)


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


def dense_vjp_batch(model, N, h, V, up, tr, w, Vbar, exact, lb=None, ub=None, n_pin=0):
    """dense_vjp for every instance, stacked; w [nw] shared or [B, nw], lb / ub [nu] shared or [B, nu]"""
    row = lambda a, b: None if a is None else (np.asarray(a, dtype=np.float64)[b] if np.ndim(a) == 2 else a)  # noqa: E731
    rows = [dense_vjp(model, N, h, V[b], up[b], tr[b], row(w, b), Vbar[b], exact, row(lb, b), row(ub, b), n_pin)
            for b in range(V.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in OUT}


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


def fd_delta(name, theta):
    """the step of a central difference in an input entry, 1e-4 relative: to the entry's own size for a weight (V*
    depends on the weights through their ratios, and Rm = 0.01 moved by 1e-4 would be a 1 % step with a visible
    third-order term), to max(1, |theta|) for x0, u_prev and traj (physical quantities of order 1, some of them 0)"""
    return 1e-4 * (np.abs(theta) if name == "weights_bar" else np.maximum(1.0, np.abs(theta)))


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
