"""CPU: the recursion that defines the feedback gains (include/mmpc.h) against the dense reference.

The kernels of csrc/gain_sweep.h run the Riccati recursion of the definition; the GPU tests hold them to the dense tail
sensitivity of tests/test_gpu_feedback_gains.py.  This module restates the recursion in numpy, term for term as the
header gives it, and checks it against that dense reference at CPU-oracle solutions, so that definition and reference
are known to agree without a GPU: 2-link arm at N = 1, 2, 17 and the exo at N = 7, both Hessians, unbounded, under
+-2 Nm (held controls) and with one committed stage.  Tolerance 1e-12 max(1, |G|): two orderings of the same fp64
arithmetic (measured <= 5e-15)."""
import numpy as np
import pytest

import oracle_lib as oracle
from conftest import WEIGHTS_CFG
from sens_reference import gains, held_mask, stage_data

H = 0.002
W_2L = np.array(WEIGHTS_CFG)
W_EXO = np.array([10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4)


def riccati_gains(model, N, h, V, up, tr, w, exact, lb=None, ub=None, n_pin=0):
    """G_k [N, nu, nx + nu] by the recursion of the definition"""
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    R, Rm = w[nx:nx + nu], w[nx + nu:]
    A, B, blocks = stage_data(model, N, h, V, up, tr, w, exact)
    held = held_mask(model, N, V, lb, ub, n_pin)
    P = np.zeros((K, K))
    G = np.zeros((N, nu, K))
    for k in range(N - 1, -1, -1):
        # T maps (dx, dv, du) to s' = (A dx + B du, du); on y = (dx, du) it is C
        C = np.block([[A[k], B[k]], [np.zeros((nu, nx)), np.eye(nu)]])
        S = blocks[k].copy()   # S_k (+ W_k): the stage block without its Delta-u and Rm terms
        S[nx:, nx:] -= np.diag(2 * R + 2 * Rm + (2 * R if k + 1 < N else 0))
        Myy = C.T @ P @ C + S
        Muu = Myy[nx:, nx:] + np.diag(2 * R + 2 * Rm)   # the further +2R of k + 1 < N came through P
        Mus = np.hstack([Myy[nx:, :nx], -np.diag(2 * R)])
        Mss = np.zeros((K, K))
        Mss[:nx, :nx] = Myy[:nx, :nx]
        Mss[nx:, nx:] = np.diag(2 * R)
        for c in np.flatnonzero(held[k]):
            Muu[c, :] = 0.0
            Muu[:, c] = 0.0
            Muu[c, c] = 1.0
            Mus[c, :] = 0.0
        np.linalg.cholesky(Muu)   # positive definite at a solution
        G[k] = -np.linalg.solve(Muu, Mus)
        P = Mss + Mus.T @ G[k]
    return G


CASES = [(oracle.TWO_LINK, 1, 2, False), (oracle.TWO_LINK, 2, 2, False), (oracle.TWO_LINK, 17, 3, False),
         (oracle.TWO_LINK, 17, 4, True), (oracle.EXO, 7, 2, False)]


@pytest.mark.parametrize("model,N,B,bounded", CASES)
def test_recursion_matches_the_dense_tail_sensitivity(model, N, B, bounded):
    w = W_EXO if model == oracle.EXO else W_2L
    lb, ub = (np.array([-2.0, -2.0]), np.array([2.0, 2.0])) if bounded else (None, None)
    x0, up, tr = oracle.synth(20250213, 0, B, N, H, model=model)
    o = oracle.solve_batch(N, H, x0, up, tr, w, u_lb=lb, u_ub=ub, model=model,
                           hessian=oracle.HESS_GAUSS_NEWTON if bounded else oracle.HESS_EXACT)
    assert (o["status"] == 0).all()
    n_held = 0
    for b in range(B):
        n_pin = 1 if (b == 1 and N > 1) else 0
        n_held += int(held_mask(model, N, o["V"][b], lb, ub, 0).sum())
        for exact in (True, False):
            Gd = gains(model, N, H, o["V"][b], up[b], tr[b], w, exact, lb, ub, n_pin)
            Gr = riccati_gains(model, N, H, o["V"][b], up[b], tr[b], w, exact, lb, ub, n_pin)
            assert np.abs(Gd - Gr).max() <= 1e-12 * max(1.0, np.abs(Gd).max())
            if n_pin:
                assert (Gd[0] == 0.0).all() and (Gr[0] == 0.0).all()
    assert (n_held > 0) == bounded


def test_exact_and_gauss_newton_gains_differ():
    """what lets a test tell the two Hessians apart: 0.2 at N = 17 on the first synthetic instance"""
    N = 17
    x0, up, tr = oracle.synth(20250213, 0, 1, N, H)
    o = oracle.solve_batch(N, H, x0, up, tr, W_2L, hessian=oracle.HESS_EXACT)
    Ge = gains(oracle.TWO_LINK, N, H, o["V"][0], up[0], tr[0], W_2L, True)
    Gg = gains(oracle.TWO_LINK, N, H, o["V"][0], up[0], tr[0], W_2L, False)
    assert np.abs(Ge - Gg).max() >= 1e-2
