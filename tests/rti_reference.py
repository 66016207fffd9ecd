"""The numpy reference of the real-time iteration step (mmpc_rti_prepare_batch / mmpc_rti_feedback_batch;
include/mmpc.h), shared by its CPU and GPU test modules.  No test lives here.

At a plan V^ that need not be a solution, with c_k = F(x^_k, u^_k) - x^_{k+1} and dx0 = x0_meas - x^_0, the step solves
    min 1/2 dV^T H dV + grad J(V^)^T dV   s.t.  dx_{k+1} = A_k dx_k + B_k du_k + c_k,  dx_0 = dx0,  du = 0 on held controls,
H = L_VV of jvp_reference._lagrangian on stage_data of tests/sens_reference.py.

* dense_rti_step: one dense KKT solve on the free entries z (x_1..x_N and the controls not held),
      [H_zz G_z^T; G_z 0] [dz; lam+] = [-grad J_z - H_{z,x0} dx0; -c - G_{x0} dx0],
  with the gradient of the objective itself, so no multiplier convention enters.  The unclamped reference.
* riccati_rti_step: the recursion of the header, term for term, and its forward sweep, with the clamp of the control
  box when clamp=True.  The reference where a clamp acts.
* shift_plan / plant_step: what a controller does between two ticks, for the tests that need it.
* exact_qp_ratio: the sign that decides between status 0 and the Gauss-Newton fallback's 1; overflow_growth /
  first_nonfinite_stage: how far the forward sweep grows dx_0, for the tests that make it overflow."""
import numpy as np

import oracle_lib as oracle
from jvp_reference import _lagrangian
from sens_reference import _jac, _residuals, gains, held_mask, stage_data, tail_system  # noqa: F401


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def objective_gradient(model, N, h, V, up, tr, w, A, B):
    """grad J(V) in V's layout and the residuals e_k [N, nx]"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    Q, R, Rm = w[:nx], w[nx:nx + nu], w[nx + nu:]
    e = _residuals(model, N, h, V, tr)
    U = V[:-nx].reshape(N, K)[:, nx:]
    g = np.zeros(V.size)
    for k in range(N):
        g[k * K:(k + 1) * K] = np.hstack([A[k], B[k]]).T @ (2 * Q * e[k])
        t = U[k] - (U[k - 1] if k else up)
        if k + 1 < N:
            t = t - (U[k + 1] - U[k])
        g[k * K + nx:(k + 1) * K] += 2 * R * t + 2 * Rm * U[k]
    return g, e


def defects(model, N, V, tr, e):
    """c_k = F(x_k, u_k) - x_{k+1} [N, nx]"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    return np.stack([e[k] + tr[k] - V[(k + 1) * K:(k + 1) * K + nx] for k in range(N)])


def dense_rti_step(model, N, h, V, up, tr, w, x0_meas, exact, lb=None, ub=None, n_pin=0):
    """dV [NV] of the definition for one instance, from one dense KKT solve; no clamp"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = _f64(w)
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, _f64(lb), _f64(ub), n_pin)
    Hm, Gz = _lagrangian(model, N, A, B, blocks, w[nx:nx + nu])
    g, e = objective_gradient(model, N, h, V, up, tr, w, A, B)
    c = defects(model, N, V, tr, e).ravel()
    dx0 = _f64(x0_meas) - V[:nx]
    free = np.ones(V.size, bool)
    free[:nx] = False
    for k in range(N):
        free[k * K + nx:(k + 1) * K] = ~held[k]
    nf, ng = int(free.sum()), N * nx
    KKT = np.zeros((nf + ng, nf + ng))
    KKT[:nf, :nf] = Hm[np.ix_(free, free)]
    KKT[nf:, :nf] = Gz[:, free]
    KKT[:nf, nf:] = Gz[:, free].T
    rhs = np.concatenate([-g[free] - Hm[np.ix_(free, np.arange(nx))] @ dx0, -c - Gz[:, :nx] @ dx0])
    dV = np.zeros(V.size)
    dV[:nx] = dx0
    dV[free] = np.linalg.solve(KKT, rhs)[:nf]
    return dV


def riccati_rti_step(model, N, h, V, up, tr, w, x0_meas, exact, lb=None, ub=None, n_pin=0, clamp=False, info=None):
    """dV [NV] by the recursion of the definition and its forward sweep, one instance.  clamp: the forward sweep
    projects u^_k + du_k onto [lb, ub] and propagates the projected du_k (a du_k that is exactly 0 is left alone).
    info: a dict that receives `clamped` [N, nu] bool (where the projection moved a control) and `V_new`, the plan
    with the controls stored as clamped (bit for bit inside the box) rather than as V + dV."""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = _f64(w)
    R, Rm = w[nx:nx + nu], w[nx + nu:]
    lb, ub = _f64(lb), _f64(ub)
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, lb, ub, n_pin)
    g, e = objective_gradient(model, N, h, V, up, tr, w, A, B)
    c = defects(model, N, V, tr, e)
    # r_{u,k}: the u rows of grad L with the multipliers of the gain recursion; its x rows vanish
    Q = w[:nx]
    lam = np.zeros(nx)
    ru = np.zeros((N, nu))
    for k in range(N - 1, -1, -1):
        nuk = 2 * Q * e[k] + lam
        ru[k] = g[k * K + nx:(k + 1) * K] + B[k].T @ lam
        lam = A[k].T @ nuk
    P = np.zeros((K, K))
    p = np.zeros(K)
    G, kff = np.zeros((N, nu, K)), np.zeros((N, nu))
    min_ratio = np.inf
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
        q = C.T @ (p - P @ np.concatenate([c[k], np.zeros(nu)]))
        q[nx:] -= ru[k]
        for i in np.flatnonzero(held[k]):
            Muu[i, :] = 0.0
            Muu[:, i] = 0.0
            Muu[i, i] = 1.0
            Mus[i, :] = 0.0
            q[nx + i] = 0.0
        ev = np.linalg.eigvalsh(0.5 * (Muu + Muu.T))
        min_ratio = min(min_ratio, ev.min() / np.abs(ev).max())
        G[k] = -np.linalg.solve(Muu, Mus)
        kff[k] = np.linalg.solve(Muu, q[nx:])
        G[k][held[k]] = 0.0
        kff[k][held[k]] = 0.0
        p = np.concatenate([q[:nx], np.zeros(nu)]) + G[k].T @ q[nx:]
        P = Mss + Mus.T @ G[k]
    dx0 = _f64(x0_meas) - V[:nx]
    dV = np.zeros(V.size)
    Vn = V.copy()
    dV[:nx] = dx0
    Vn[:nx] = x0_meas
    s = np.concatenate([dx0, np.zeros(nu)])
    clamped = np.zeros((N, nu), bool)
    for k in range(N):
        du = G[k] @ s + kff[k]
        uh = V[k * K + nx:(k + 1) * K]
        un = uh + du
        if clamp:
            lo = np.full(nu, -np.inf) if lb is None else lb
            hi = np.full(nu, np.inf) if ub is None else ub
            proj = np.where(du == 0.0, uh, np.minimum(np.maximum(un, lo), hi))
            clamped[k] = proj != un
            un = proj
            du = un - uh
        dV[k * K + nx:(k + 1) * K] = du
        Vn[k * K + nx:(k + 1) * K] = un
        dxn = A[k] @ s[:nx] + B[k] @ du + c[k]
        dV[(k + 1) * K:(k + 1) * K + nx] = dxn
        s = np.concatenate([dxn, du])
    for k in range(1, N + 1):
        Vn[k * K:k * K + nx] = V[k * K:k * K + nx] + dV[k * K:k * K + nx]
    if info is not None:
        info["clamped"] = clamped
        info["V_new"] = Vn
        info["min_ratio"] = min_ratio
    return dV


def exact_qp_ratio(model, N, h, V, up, tr, w, lb=None, ub=None, n_pin=0):
    """the smallest over the stages of (smallest / largest-magnitude eigenvalue of M_uu) of the exact-Hessian recursion,
    held rows replaced by the identity: positive exactly when every pivot of the exact sweep is, i.e. when the exact QP
    is positive definite on the free controls, which is what decides between status 0 and the fallback's 1"""
    info = {}
    riccati_rti_step(model, N, h, V, up, tr, w, V[:oracle.DIMS[model][0]], True, lb, ub, n_pin, False, info)
    return info["min_ratio"]


def overflow_growth(model, N, h, V, up, tr, w, exact, lb=None, ub=None, clamp=False, big=1e300):
    """g = max |dV| / big of the reference step at x0_meas = x^_0 + big on every entry (big = 1e300: nothing
    overflows, and the step is linear in dx_0 up to 1e-300).  With g >= 1.2 the same sweep at dx_0 = 1.7e308 passes
    DBL_MAX = 1.797e308 by 13 % or more, whatever the order of its sums: the step must be reported as failed."""
    nx, _ = oracle.DIMS[model]
    dV = riccati_rti_step(model, N, h, V, up, tr, w, V[:nx] + big, exact, lb, ub, 0, clamp)
    assert np.isfinite(dV).all()
    return np.abs(dV).max() / big


def first_nonfinite_stage(model, N, h, V, up, tr, w, exact, lb=None, ub=None, clamp=False, big=1.7e308):
    """the first stage k at which (du_k, dx_{k+1}) of the reference's forward sweep at x0_meas = big is not finite"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    with np.errstate(all="ignore"):
        dV = riccati_rti_step(model, N, h, V, up, tr, w, np.full(nx, big), exact, lb, ub, 0, clamp)
    for k in range(N):
        if not np.isfinite(dV[k * K + nx:(k + 1) * K + nx]).all():
            return k
    return None


def _row(a, b, shared_ndim):
    """row b of a per-instance array, the array itself when shared, None when absent"""
    return None if a is None else (np.asarray(a, dtype=np.float64)[b] if np.ndim(a) > shared_ndim else a)


def dense_rti_step_batch(model, N, h, V, up, tr, w, x0_meas, exact, lb=None, ub=None, n_pin=0):
    """dense_rti_step for every instance [B, NV]; w [nw] shared or [B, nw], lb / ub [nu] shared or [B, nu]"""
    return np.stack([dense_rti_step(model, N, h, V[b], up[b], tr[b], _row(w, b, 1), x0_meas[b], exact, _row(lb, b, 1),
                                    _row(ub, b, 1), n_pin) for b in range(V.shape[0])])


def riccati_rti_step_batch(model, N, h, V, up, tr, w, x0_meas, exact, lb=None, ub=None, n_pin=0, clamp=False):
    """riccati_rti_step for every instance: (dV [B, NV], V_new [B, NV], clamped [B, N, nu])"""
    dV, Vn, cl = [], [], []
    for b in range(V.shape[0]):
        info = {}
        dV.append(riccati_rti_step(model, N, h, V[b], up[b], tr[b], _row(w, b, 1), x0_meas[b], exact, _row(lb, b, 1),
                                   _row(ub, b, 1), n_pin, clamp, info))
        Vn.append(info["V_new"])
        cl.append(info["clamped"])
    return np.stack(dV), np.stack(Vn), np.stack(cl)


def plant_step(model, h, x, u):
    """F(x, u) = x + h f(x, u): the explicit Euler step the NLP's defects use"""
    return x + h * _jac(model, x, u)[2]


def shift_plan(model, N, h, V):
    """the plan shifted by one stage, one instance: (x_1, u_1, .., x_{N-1}, u_{N-1}, x_N, u_{N-1}, F(x_N, u_{N-1})),
    and the control that is in force over the new first interval (the old u_0)"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    ulast = V[(N - 1) * K + nx:N * K]
    xN = V[N * K:]
    return np.concatenate([V[K:], ulast, plant_step(model, h, xN, ulast)]), V[nx:K].copy()
