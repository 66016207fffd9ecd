"""The numpy reference of the solve's forward-mode product (mmpc_solve_jvp_batch; include/mmpc.h), shared
by its CPU and GPU test modules.  No test lives here.

dV = (d V* / d theta) d theta for theta = (x0, u_prev, traj, weights) from one dense KKT solve on stage_data /
held_mask of tests/sens_reference.py.  With z the free entries of V (x_1..x_N and the controls not held), L_VV the
Hessian of the Lagrangian and g the defects, differentiating the stationarity and the defects at fixed active set gives
    L_zz dz + g_z^T dlam = rho_z - L_{z, x0} dx0 + (2 R o du_prev on u_0),    g_z dz = -g_{x0} dx0,
with dV = dx0 on x_0 and 0 on held controls, and rho = -d(grad_V L)/d theta d theta for traj and the weights:
    rho_k = J_k^T (2 Q o dtraj_k - 2 dQ o e_k), on the u rows - 2 dR o ((u_k - u_{k-1}) - (u_{k+1} - u_k)) - 2 dRm o u_k,
    u_{-1} = u_prev, no u_{k+1} term at k = N - 1, rho on x_N = 0.
xb_dense_jvp is the same under the sensitivity barrier of a state-bounded handle (xb_stage_data / barrier_terms: D on
the diagonal of L_zz, beta in the multipliers; the barrier does not depend on theta), solved with refined_solve as
xb_dense_vjp is."""
import numpy as np

import oracle_lib as oracle
from sens_reference import (CAP_DEFAULT, _residuals, barrier_terms, held_mask, mu_f, refined_solve, stage_data,
                            xb_stage_data)


def tangents(model, N, rng, B=None):
    """standard normal (dx0, du_prev, dtraj, dweights) for one instance, or for B of them"""
    nx, nu = oracle.DIMS[model]
    lead = () if B is None else (B,)
    return tuple(rng.standard_normal(lead + s) for s in ((nx,), (nu,), (N, nx), (nx + 2 * nu,)))


def rho(model, N, h, V, up, tr, w, A, B, dtraj, dweights):
    """the right-hand side of the definition in V's layout [NV]; a tangent that is None is zero"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    Q = w[:nx]
    dtraj = np.zeros((N, nx)) if dtraj is None else dtraj
    dQ, dR, dRm = np.split(np.zeros(nx + 2 * nu) if dweights is None else dweights, [nx, nx + nu])
    e = _residuals(model, N, h, V, tr)
    U = V[:-nx].reshape(N, K)[:, nx:]
    out = np.zeros(V.size)
    for k in range(N):
        r = np.hstack([A[k], B[k]]).T @ (2 * Q * dtraj[k] - 2 * dQ * e[k])
        t = U[k] - (U[k - 1] if k else up)
        if k + 1 < N:
            t = t - (U[k + 1] - U[k])
        r[nx:] += -2 * dR * t - 2 * dRm * U[k]
        out[k * K:(k + 1) * K] = r
    return out


def _lagrangian(model, N, A, B, blocks, R):
    """L_VV [NV, NV] (the stage blocks and the -2R couplings of consecutive controls) and the defects' Jacobian"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    NV = N * K + nx
    Hm = np.zeros((NV, NV))
    Gz = np.zeros((N * nx, NV))
    for k in range(N):
        Hm[k * K:(k + 1) * K, k * K:(k + 1) * K] = blocks[k]
        Gz[k * nx:(k + 1) * nx, k * K:(k + 1) * K] = np.hstack([A[k], B[k]])
        Gz[k * nx + np.arange(nx), (k + 1) * K + np.arange(nx)] = -1.0
        if k >= 1:
            i, j = k * K + nx + np.arange(nu), (k - 1) * K + nx + np.arange(nu)
            Hm[i, j] -= 2 * R
            Hm[j, i] -= 2 * R
    return Hm, Gz


def _solve_kkt(Hm, Gz, free, rhs_V, dx0, nx, solve):
    """dV from the KKT system on the free entries; rhs_V: rho plus the u_prev term, in V's layout"""
    NV = Hm.shape[0]
    dx0 = np.zeros(nx) if dx0 is None else dx0
    nf, ng = int(free.sum()), Gz.shape[0]
    KKT = np.zeros((nf + ng, nf + ng))
    KKT[:nf, :nf] = Hm[np.ix_(free, free)]
    KKT[nf:, :nf] = Gz[:, free]
    KKT[:nf, nf:] = Gz[:, free].T
    rhs = np.concatenate([rhs_V[free] - Hm[np.ix_(free, np.arange(nx))] @ dx0, -Gz[:, :nx] @ dx0])
    dV = np.zeros(NV)
    dV[:nx] = dx0
    dV[free] = solve(KKT, rhs)[:nf]
    return dV


def dense_jvp(model, N, h, V, up, tr, w, dx0, du_prev, dtraj, dweights, exact, lb=None, ub=None, n_pin=0):
    """dV [NV] of the definition for one instance, from one dense KKT solve; a tangent that is None is zero"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = np.asarray(w, dtype=np.float64)
    R = w[nx:nx + nu]
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, None if lb is None else np.asarray(lb, dtype=np.float64),
                     None if ub is None else np.asarray(ub, dtype=np.float64), n_pin)
    Hm, Gz = _lagrangian(model, N, A, B, blocks, R)
    free = np.ones(V.size, bool)
    free[:nx] = False
    for k in range(N):
        free[k * K + nx:(k + 1) * K] = ~held[k]
    rhs = rho(model, N, h, V, up, tr, w, A, B, dtraj, dweights)
    if du_prev is not None:
        rhs[nx:K] += 2 * R * du_prev
    return _solve_kkt(Hm, Gz, free, rhs, dx0, nx, np.linalg.solve)


def xb_dense_jvp(model, N, h, V, up, tr, w, dx0, du_prev, dtraj, dweights, exact, xl, xu, ul=None, uu=None, n_pin=0,
                 mu=None, cap=CAP_DEFAULT):
    """dense_jvp under the sensitivity barrier: D on the diagonal of L_zz, no control held by bit-equality"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = np.asarray(w, dtype=np.float64)
    R = w[nx:nx + nu]
    mu = mu_f() if mu is None else mu
    bx, Dx, Du, _, _ = barrier_terms(model, N, V, xl, xu, ul, uu, n_pin, mu, cap)
    A, B, blocks = xb_stage_data(model, N, h, V, up, tr, w, exact, bx)
    Hm, Gz = _lagrangian(model, N, A, B, blocks, R)
    for k in range(N):
        iu, ix = k * K + nx + np.arange(nu), (k + 1) * K + np.arange(nx)
        Hm[iu, iu] += Du[k]
        Hm[ix, ix] += Dx[k]
    free = np.ones(V.size, bool)
    free[:nx] = False
    for k in range(n_pin):
        free[k * K + nx:(k + 1) * K] = False
    rhs = rho(model, N, h, V, up, tr, w, A, B, dtraj, dweights)
    if du_prev is not None:
        rhs[nx:K] += 2 * R * du_prev
    return _solve_kkt(Hm, Gz, free, rhs, dx0, nx, refined_solve)


def _row(a, b, shared_ndim):
    """row b of a per-instance array, the array itself when shared, None when absent"""
    return None if a is None else (np.asarray(a, dtype=np.float64)[b] if np.ndim(a) > shared_ndim else a)


def dense_jvp_batch(model, N, h, V, up, tr, w, dx0, du_prev, dtraj, dweights, exact, lb=None, ub=None, n_pin=0):
    """dense_jvp for every instance [B, NV]; w [nw] shared or [B, nw], lb / ub [nu] shared or [B, nu]; the tangents
    are per instance or None"""
    return np.stack([dense_jvp(model, N, h, V[b], up[b], tr[b], _row(w, b, 1), _row(dx0, b, 0), _row(du_prev, b, 0),
                               _row(dtraj, b, 0), _row(dweights, b, 0), exact, _row(lb, b, 1), _row(ub, b, 1), n_pin)
                     for b in range(V.shape[0])])


def xb_dense_jvp_batch(model, N, h, V, up, tr, w, dx0, du_prev, dtraj, dweights, exact, xl, xu, ul=None, uu=None, **kw):
    return np.stack([xb_dense_jvp(model, N, h, V[b], up[b], tr[b], w, _row(dx0, b, 0), _row(du_prev, b, 0),
                                  _row(dtraj, b, 0), _row(dweights, b, 0), exact, xl, xu, _row(ul, b, 1),
                                  _row(uu, b, 1), **kw) for b in range(V.shape[0])])
