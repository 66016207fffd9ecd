"""The numpy reference of the sensitivity calls (feedback gains, solve VJP, and both under the sensitivity barrier of a
state-bounded handle), shared by their CPU and GPU test modules.  No test lives here.

* gains / gains_batch: the DENSE sensitivity of the tail problems (stage_data, held_mask, tail_system); the derivation
  is in tests/test_gpu_feedback_gains.py's docstring.
* dense_vjp / dense_vjp_batch: the dense KKT solve of tests/test_solve_vjp_reference.py's docstring; fd_delta is the
  step of the central differences taken against it.
* xb_dense_gains / xb_dense_vjp and their batches: the same two with the barrier's terms (barrier_terms,
  xb_stage_data), assembled or refined in extended precision; tests/test_xb_sensitivity_reference.py's docstring.
* model = oracle.USER: a generated model (use_user_model of this module registers it; _jac reads the host build of its
  generated header and raises when the oracle's one USER slot holds another model by then)."""
import math

import numpy as np

import oracle_lib as oracle

OUT = ("x0_bar", "u_prev_bar", "traj_bar", "weights_bar", "adj_V")
CAP_DEFAULT = 1e12


# ---------------------------------------------------------------- feedback gains: the dense tail sensitivity
_user_name = None   # the generated model use_user_model of this module registered last


def use_user_model(name):
    """Register generated model `name` as the oracle's USER model for the references of this module; returns
    oracle.USER.  The oracle has one USER slot: call this before every reference or oracle solve of that model."""
    global _user_name
    _user_name = name
    return oracle.use_user_model(name)


def _jac(model, x, u):
    if model == oracle.USER:   # raises if the slot was never filled through this module or holds another model since
        assert _user_name is not None, "sens_reference.use_user_model(name) comes first"
        return oracle.active_user_model(_user_name).jac(x, u)
    return (oracle.exo_jac if model == oracle.EXO else oracle.two_link_jac)(x, u)


def stage_data(model, N, h, V, up, tr, w, exact):
    """A_k, B_k and the (x_k, u_k) Hessian blocks of the Lagrangian at V, exact or Gauss-Newton"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    Q, R, Rm = w[:nx], w[nx:nx + nu], w[nx + nu:]
    Vs = V[:-nx].reshape(N, K)
    A, B, e = [], [], []
    for k in range(N):
        Ac, Bc, xd = _jac(model, Vs[k, :nx], Vs[k, nx:])
        A.append(np.eye(nx) + h * Ac)
        B.append(h * Bc)
        e.append(Vs[k, :nx] + h * xd - tr[k])
    if exact:
        lam = np.zeros((N, nx))   # lam_k = A_{k+1}^T (2 Q e_{k+1} + lam_{k+1}), lam_{N-1} = 0
        for k in range(N - 2, -1, -1):
            lam[k] = A[k + 1].T @ (2 * Q * e[k + 1] + lam[k + 1])
        blocks = oracle.nlp_hess(N, h, V, up, tr, w, 1.0, lam, model=model)
    else:
        blocks = np.zeros((N, K, K))
        for k in range(N):
            JF = np.hstack([A[k], B[k]])
            blocks[k] = 2 * JF.T @ (Q[:, None] * JF)
            blocks[k, nx:, nx:] += np.diag(2 * R + 2 * Rm + (2 * R if k + 1 < N else 0))
    return A, B, blocks


def held_mask(model, N, V, lb, ub, n_pin):
    """[N, nu] bool: control on a finite bound bit for bit, or committed"""
    nx, nu = oracle.DIMS[model]
    U = V[:-nx].reshape(N, nx + nu)[:, nx:]
    held = np.zeros((N, nu), bool)
    held[:n_pin] = True
    if lb is not None:
        held |= (np.abs(lb) < 1e19)[None, :] & (U == lb[None, :])
    if ub is not None:
        held |= (np.abs(ub) < 1e19)[None, :] & (U == ub[None, :])
    return held


def tail_system(model, N, k, A, B, blocks, w):
    """H_UU [(N-k) nu]^2 and H_Up [(N-k) nu, K] of the tail problem from stage k, no control removed"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    R = w[nx:nx + nu]
    n = (N - k) * nu
    Su = np.zeros((nx, n))
    Sp = np.eye(nx)
    HUU = np.zeros((n, n))
    HUp = np.zeros((n, K))
    for j in range(k, N):
        Yu = np.zeros((K, n))    # (dx_j, du_j) as functions of dU and of dx
        Yu[:nx] = Su
        Yu[nx + np.arange(nu), (j - k) * nu + np.arange(nu)] = 1.0
        Yp = np.zeros((K, nx))
        Yp[:nx] = Sp
        HUU += Yu.T @ blocks[j] @ Yu
        HUp[:, :nx] += Yu.T @ blocks[j] @ Yp
        Su, Sp = A[j] @ Su + B[j] @ Yu[nx:], A[j] @ Sp
    for j in range(k + 1, N):
        for c in range(nu):
            a, b = (j - k) * nu + c, (j - 1 - k) * nu + c
            HUU[a, b] -= 2 * R[c]
            HUU[b, a] -= 2 * R[c]
    for c in range(nu):
        HUp[c, nx + c] -= 2 * R[c]
    return 0.5 * (HUU + HUU.T), HUp


def gains(model, N, h, V, up, tr, w, exact, lb=None, ub=None, n_pin=0, stages=None, min_eig=None):
    """G_k [nu, nx + nu] for k in stages (default all N), one instance.  min_eig: a list that receives, per stage,
    the smallest eigenvalue of the free part of H_UU over its largest."""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = np.asarray(w, dtype=np.float64)
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, None if lb is None else np.asarray(lb, dtype=np.float64),
                     None if ub is None else np.asarray(ub, dtype=np.float64), n_pin)
    stages = range(N) if stages is None else stages
    out = np.zeros((len(stages), nu, K))
    for i, k in enumerate(stages):
        HUU, HUp = tail_system(model, N, k, A, B, blocks, w)
        free = ~held[k:].ravel()
        dU = np.zeros((free.size, K))
        if free.any():
            Hf = HUU[np.ix_(free, free)]
            dU[free] = -np.linalg.solve(Hf, HUp[free])
            if min_eig is not None:
                ev = np.linalg.eigvalsh(Hf)
                min_eig.append(ev.min() / ev.max())
        out[i] = dU[:nu]
    return out


def gains_batch(model, N, h, V, up, tr, w, exact, lb=None, ub=None, n_pin=0, stages=None):
    """gains() for every instance: [B, len(stages), nu, nx + nu]; w [nw] shared, lb / ub [nu] shared or [B, nu]"""
    row = lambda a, b: None if a is None else (np.asarray(a, dtype=np.float64)[b] if np.ndim(a) == 2 else a)  # noqa: E731
    return np.stack([gains(model, N, h, V[b], up[b], tr[b], w, exact, row(lb, b), row(ub, b), n_pin, stages)
                     for b in range(V.shape[0])])


# ---------------------------------------------------------------- solve VJP: the dense KKT solve
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


def dense_vjp_batch(model, N, h, V, up, tr, w, Vbar, exact, lb=None, ub=None, n_pin=0):
    """dense_vjp for every instance, stacked; w [nw] shared or [B, nw], lb / ub [nu] shared or [B, nu]"""
    row = lambda a, b: None if a is None else (np.asarray(a, dtype=np.float64)[b] if np.ndim(a) == 2 else a)  # noqa: E731
    rows = [dense_vjp(model, N, h, V[b], up[b], tr[b], row(w, b), Vbar[b], exact, row(lb, b), row(ub, b), n_pin)
            for b in range(V.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in OUT}


def fd_delta(name, theta):
    """the step of a central difference in an input entry, 1e-4 relative: to the entry's own size for a weight (V*
    depends on the weights through their ratios, and Rm = 0.01 moved by 1e-4 would be a 1 % step with a visible
    third-order term), to max(1, |theta|) for x0, u_prev and traj (physical quantities of order 1, some of them 0)"""
    return 1e-4 * (np.abs(theta) if name == "weights_bar" else np.maximum(1.0, np.abs(theta)))


# ---------------------------------------------------------------- the same two under the sensitivity barrier
def mu_f():
    """the barrier value the monotone schedule of csrc/sqp_wave.h reaches first with 2 mu <= 1e-8"""
    mu, tol = 0.1, 1e-8
    while 2.0 * mu > tol:
        mu = max(tol / 20.0, min(0.2 * mu, math.pow(mu, 1.5)))
    return mu


def barrier_terms(model, N, V, xl, xu, ul, uu, n_pin, mu, cap):
    """beta(x_{k+1}) [N, nx], D(x_{k+1}) [N, nx], D(u_k) [N, nu] (0 for k < n_pin), the uncapped D of every bounded
    entry and the smallest slack; a bound that is None or |b| >= 1e19 is infinite"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    X = np.stack([V[(k + 1) * K:(k + 1) * K + nx] for k in range(N)])
    U = V[:-nx].reshape(N, K)[:, nx:]

    def side(b, n, sign):
        b = np.full(n, sign * np.inf) if b is None else np.asarray(b, dtype=np.float64).copy()
        b[np.abs(b) >= 1e19] = sign * np.inf
        return b

    def terms(Y, lo, hi):
        sl, su = Y - lo[None, :], hi[None, :] - Y
        with np.errstate(divide="ignore"):
            beta = 2 * mu * (1 / su - 1 / sl)
            D = 2 * mu * (1 / sl ** 2 + 1 / su ** 2)
        return beta, D, np.minimum(sl, su)

    bx, Dx, sx = terms(X, side(xl, nx, -1), side(xu, nx, 1))
    _, Du, su = terms(U, side(ul, nu, -1), side(uu, nu, 1))
    Du[:n_pin] = 0.0
    su[:n_pin] = np.inf
    raw = np.concatenate([Dx[np.isfinite(sx)], Du[np.isfinite(su)]])
    return bx, np.minimum(Dx, cap), np.minimum(Du, cap), raw, min(sx.min(), su.min())


def xb_stage_data(model, N, h, V, up, tr, w, exact, bx):
    """A_k, B_k and the stage blocks of stage_data with beta(x_{k+1}) = bx[k] in the multipliers"""
    nx, nu = oracle.DIMS[model]
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, False)
    if exact:
        Q = w[:nx]
        e = _residuals(model, N, h, V, tr)
        lam = np.zeros((N, nx))
        lam[N - 1] = bx[N - 1]
        for k in range(N - 2, -1, -1):
            lam[k] = A[k + 1].T @ (2 * Q * e[k + 1] + lam[k + 1]) + bx[k]
        blocks = oracle.nlp_hess(N, h, V, up, tr, w, 1.0, lam, model=model)
    return A, B, blocks


def refined_solve(A, b):
    """A^-1 b by LU in double with iterative refinement on extended-precision residuals (A and b may be extended
    themselves); returned in double.  With D up to the cap on the diagonal the plain solve's own error (measured
    1.6e-10 on weights_bar at N = 33, cap 1e6, where the recursion agrees with the refined solve to 3e-14) would
    otherwise be charged to the code under test."""
    LD = np.longdouble
    A64, Al, bl = A.astype(np.float64), A.astype(LD), b.astype(LD)
    x = np.linalg.solve(A64, bl.astype(np.float64)).astype(LD)
    for _ in range(4):
        x = x + np.linalg.solve(A64, (bl - Al @ x).astype(np.float64)).astype(LD)
    return x.astype(np.float64)


def xb_dense_gains(model, N, h, V, up, tr, w, exact, xl, xu, ul=None, uu=None, n_pin=0, mu=None, cap=CAP_DEFAULT,
                   stages=None):
    """G_k [nu, K] for k in stages (default all N) from the dense tail problems, one instance.  The tail systems of
    tail_system with the barrier added, assembled in extended precision (the double
    assembly of sums with D = 1e6 beside entries of order 1 carries 7e-11 at exo N = 7, three times the recursion's
    own error): H_UU of the tail from stage k is the trailing block of stage 0's, since no state depends on a later
    control, and H_Up's state columns follow backward from T_k = Yu_k^T S_k[:, x] + (T_{k+1} + Su_{k+1}^T D_k) A_k."""
    LD = np.longdouble
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    w = np.asarray(w, dtype=np.float64)
    R = w[nx:nx + nu]
    mu = mu_f() if mu is None else mu
    bx, Dx, Du, _, _ = barrier_terms(model, N, V, xl, xu, ul, uu, n_pin, mu, cap)
    A, B, blocks = xb_stage_data(model, N, h, V, up, tr, w, exact, bx)
    A, B, blocks = [a.astype(LD) for a in A], [b.astype(LD) for b in B], blocks.astype(LD)
    Dx, Du = Dx.astype(LD), Du.astype(LD)
    n = N * nu
    Su, HUU = np.zeros((nx, n), LD), np.zeros((n, n), LD)
    Yus, Sus = [], []
    for j in range(N):
        cols = j * nu + np.arange(nu)
        Yu = np.zeros((K, n), LD)    # (dx_j, du_j) as functions of dU
        Yu[:nx] = Su
        Yu[nx + np.arange(nu), cols] = 1.0
        HUU += Yu.T @ (blocks[j] @ Yu)
        HUU[cols, cols] += Du[j]
        Su = A[j] @ Su + B[j] @ Yu[nx:]
        HUU += Su.T @ (Dx[j][:, None] * Su)      # the barrier of x_{j+1}
        Yus.append(Yu)
        Sus.append(Su)
    for j in range(1, N):
        for c in range(nu):
            HUU[j * nu + c, (j - 1) * nu + c] -= 2 * R[c]
            HUU[(j - 1) * nu + c, j * nu + c] -= 2 * R[c]
    HUU = (HUU + HUU.T) / 2
    T = np.zeros((n, nx), LD)
    Ts = [None] * N
    for k in range(N - 1, -1, -1):
        T = Yus[k].T @ blocks[k][:, :nx] + (Sus[k].T * Dx[k][None, :] + T) @ A[k]
        Ts[k] = T
    stages = range(N) if stages is None else stages
    out = np.zeros((len(stages), nu, K))
    for i, k in enumerate(stages):
        r0 = k * nu
        HUp = np.zeros((n - r0, K), LD)
        HUp[:, :nx] = Ts[k][r0:]
        for c in range(nu):
            HUp[c, nx + c] -= 2 * R[c]
        free = np.repeat(np.arange(k, N) >= n_pin, nu)
        dU = np.zeros((n - r0, K))
        if free.any():
            dU[free] = -refined_solve(HUU[r0:, r0:][np.ix_(free, free)], HUp[free])
        out[i] = dU[:nu]
    return out


def xb_dense_vjp(model, N, h, V, up, tr, w, Vbar, exact, xl, xu, ul=None, uu=None, n_pin=0, mu=None, cap=CAP_DEFAULT):
    """every VJP output for one instance from one dense KKT solve with D on the diagonal of L_zz"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    NV = V.size
    w = np.asarray(w, dtype=np.float64)
    Q, R = w[:nx], w[nx:nx + nu]
    mu = mu_f() if mu is None else mu
    bx, Dx, Du, _, _ = barrier_terms(model, N, V, xl, xu, ul, uu, n_pin, mu, cap)
    A, B, blocks = xb_stage_data(model, N, h, V, up, tr, w, exact, bx)
    Hm = np.zeros((NV, NV))
    Gz = np.zeros((N * nx, NV))
    for k in range(N):
        Hm[k * K:(k + 1) * K, k * K:(k + 1) * K] += blocks[k]
        iu, ix = k * K + nx + np.arange(nu), (k + 1) * K + np.arange(nx)
        Hm[iu, iu] += Du[k]
        Hm[ix, ix] += Dx[k]
        Gz[k * nx:(k + 1) * nx, k * K:(k + 1) * K] = np.hstack([A[k], B[k]])
        Gz[k * nx + np.arange(nx), ix] = -1.0
        if k >= 1:
            j = iu - K
            Hm[iu, j] -= 2 * R
            Hm[j, iu] -= 2 * R
    free = np.ones(NV, bool)
    free[:nx] = False
    for k in range(n_pin):
        free[k * K + nx:(k + 1) * K] = False
    nf, ng = int(free.sum()), N * nx
    KKT = np.zeros((nf + ng, nf + ng))
    KKT[:nf, :nf] = Hm[np.ix_(free, free)]
    KKT[nf:, :nf] = Gz[:, free]
    KKT[:nf, nf:] = Gz[:, free].T
    sol = refined_solve(KKT, np.concatenate([Vbar[free], np.zeros(ng)]))
    a = np.zeros(NV)
    a[free] = sol[:nf]
    b = sol[nf:]
    x0_bar = Vbar[:nx] - Hm[:, :nx].T @ a - Gz[:, :nx].T @ b
    ax_next = np.stack([np.hstack([A[k], B[k]]) @ a[k * K:(k + 1) * K] for k in range(N)])
    e = _residuals(model, N, h, V, tr)
    return dict(x0_bar=x0_bar, u_prev_bar=2 * R * a[nx:K], traj_bar=2 * Q[None, :] * ax_next,
                weights_bar=_weight_sums(model, N, V, up, e, a, ax_next), adj_V=a)


def xb_dense_gains_batch(model, N, h, V, up, tr, w, exact, xl, xu, ul=None, uu=None, **kw):
    """xb_dense_gains for every instance [B, n, nu, K]; ul / uu [nu] shared or [B, nu]"""
    row = lambda a, b: None if a is None else (np.asarray(a, dtype=np.float64)[b] if np.ndim(a) == 2 else a)  # noqa: E731
    return np.stack([xb_dense_gains(model, N, h, V[b], up[b], tr[b], w, exact, xl, xu, row(ul, b), row(uu, b), **kw)
                     for b in range(V.shape[0])])


def xb_dense_vjp_batch(model, N, h, V, up, tr, w, Vbar, exact, xl, xu, ul=None, uu=None, **kw):
    row = lambda a, b: None if a is None else (np.asarray(a, dtype=np.float64)[b] if np.ndim(a) == 2 else a)  # noqa: E731
    rows = [xb_dense_vjp(model, N, h, V[b], up[b], tr[b], w, Vbar[b], exact, xl, xu, row(ul, b), row(uu, b), **kw)
            for b in range(V.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in OUT}
