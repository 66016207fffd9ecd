"""CPU: the definition of the real-time iteration step (mmpc_rti_prepare_batch / mmpc_rti_feedback_batch;
include/mmpc.h), restated in numpy by tests/rti_reference.py.

Setup: the four cases of tests/test_solve_jvp_reference.py (`solved` of tests/test_solve_vjp_reference.py: two
instances each, oracle exact-Hessian solves at 1e-11 / 1e-12; 2-link N = 1, 5 unbounded, N = 17 under +-2 Nm with 1 and
24 held controls, exo N = 7).  The linearisation point is NOT a solution: it is the plan shifted by one stage
(shift_plan: the last control repeated, x_N = F(x_N, u_{N-1}); u_prev the old u_0), and x0_meas = x^_0 + 1e-2 times a
standard normal from default_rng(SEED + 101 N + b).

1. recursion against the dense KKT solve wherever no clamp acts: 1e-10 max(1, max |ref|), both Hessians, n_pin 0 and 1
   (measured <= 5.2e-14); du exactly 0 on held controls, the x_0 entries of dV exactly x0_meas - x^_0.
2. the clamped forward pass: with a box that no control of the unclamped step leaves, clamp=True is the unclamped step
   up to the rounding of u + du - u; with a tight box some free controls are clamped and not all, every new control is
   inside the box bit for bit, held controls keep du = 0, and the new states satisfy the linearised dynamics with the
   clamped du.
3. the Newton property, 2-link N = 17, five instances (the inputs of the GPU test, oracle.synth(SEED, 0, 5, 17, H)):
   V* from the oracle at (x0, traj); x0 moved by delta with |delta|_inf = 1e-2 (default_rng(SEED + 7 N + B), scaled);
   the reference step iterated at the new x0 from V*, against the oracle's re-solve V*_new.  Measured, per instance
   (|V_n - V*_new|_inf for n = 0..4):
       1.12e-02 7.55e-05 2.10e-11 1.91e-12 1.94e-12
       2.63e-02 2.02e-04 6.37e-12 6.66e-12 6.63e-12
       4.81e-02 5.32e-06 9.95e-14 3.02e-14 5.33e-14
       1.34e-02 2.69e-05 1.95e-12 4.68e-12 4.87e-12
       1.15e-02 1.04e-05 1.32e-13 3.62e-14 6.39e-14
   The error stops falling after n* = 3 steps (2 for two of the five), at <= 6.7e-12 -- the oracle's own convergence
   at 1e-11 / 1e-12, not the step -- and every step before that contracts by at least 130 (quadratically: 130, then
   3e6).  No instance needed a smaller delta than 1e-2.  N_STAR and ERR_REACHED below are these two numbers; the GPU
   test of the Newton iteration (tests/test_gpu_rti.py) takes its step count and its bound from them."""
import numpy as np
import pytest

import oracle_lib as oracle
from rti_reference import dense_rti_step, riccati_rti_step, shift_plan
from sens_reference import _jac, held_mask
from test_solve_vjp_reference import CASES, SEED, H, W_2L, solved

TOL = 1e-10
N_STAR = 3              # steps after which the error of the iterated reference step stops falling (item 3)
ERR_REACHED = 6.8e-12   # the error it reaches, all five instances
CONTRACTION = 10.0      # what every step before n* must contract by at |delta|_inf = 1e-2
DELTA = 1e-2


def shifted(model, N, b, bounds):
    """(w, lb, ub, V^, u_prev, traj, x0_meas) of instance b of a case at its shifted plan"""
    nx, _ = oracle.DIMS[model]
    w, lb, ub, _, _, tr, V, _ = solved(model, N, bounds)
    Vh, up = shift_plan(model, N, H, V[b])
    x0m = Vh[:nx] + 1e-2 * np.random.default_rng(SEED + 101 * N + b).standard_normal(nx)
    return w, lb, ub, Vh, up, tr[b], x0m


def pins(N):
    return sorted({0, min(1, N - 1)})


@pytest.mark.parametrize("model,N,bounds,n_held", CASES)
def test_recursion_matches_the_dense_kkt_solve(model, N, bounds, n_held):
    nx, nu = oracle.DIMS[model]
    worst = 0.0
    for b in range(2):
        w, lb, ub, Vh, up, tr, x0m = shifted(model, N, b, bounds)
        for exact in (True, False):
            for n_pin in pins(N):
                d = dense_rti_step(model, N, H, Vh, up, tr, w, x0m, exact, lb, ub, n_pin)
                r = riccati_rti_step(model, N, H, Vh, up, tr, w, x0m, exact, lb, ub, n_pin)
                err, scale = np.abs(d - r).max(), max(1.0, np.abs(d).max())
                worst = max(worst, err / scale)
                assert err <= TOL * scale, (b, exact, n_pin, err)
                held = held_mask(model, N, Vh, lb, ub, n_pin)
                for dv in (d, r):
                    assert (dv[:-nx].reshape(N, -1)[:, nx:][held] == 0.0).all()
                    assert np.array_equal(dv[:nx], x0m - Vh[:nx])
                assert np.abs(d).max() > 1e-3, "the shifted plan is no solution: the step must not vanish"
    print(f"recursion against dense, worst relative error: {worst:.3e}")


def test_the_step_of_a_solution_at_its_own_state_is_the_residual_of_the_solve():
    """at V* with x0_meas = x0 the right-hand side is the KKT residual the solve stopped at"""
    model, N = oracle.TWO_LINK, 5
    w, lb, ub, x0, up, tr, V, _ = solved(model, N, None)
    for b in range(2):
        d = dense_rti_step(model, N, H, V[b], up[b], tr[b], w, x0[b], True)
        assert np.abs(d).max() <= 1e-9, np.abs(d).max()


@pytest.mark.parametrize("exact", [True, False])
def test_clamped_forward_pass(exact):
    model, N, bounds = CASES[2][0], CASES[2][1], CASES[2][2]
    nx, nu = oracle.DIMS[model]
    K = nx + nu
    some, not_all = False, False
    for b in range(2):
        w, lb, ub, Vh, up, tr, x0m = shifted(model, N, b, bounds)
        lb, ub = np.asarray(lb, float), np.asarray(ub, float)
        free = riccati_rti_step(model, N, H, Vh, up, tr, w, x0m, exact, lb, ub)
        Uh = Vh[:-nx].reshape(N, K)[:, nx:]
        # the case's own box: wherever the unclamped step stays inside it the clamp is the identity
        info = {}
        cl = riccati_rti_step(model, N, H, Vh, up, tr, w, x0m, exact, lb, ub, clamp=True, info=info)
        if not info["clamped"].any():
            assert np.abs(cl - free).max() <= 1e-14 * max(1.0, np.abs(free).max())
        # a tight box around the plan's own controls: half of the largest free step
        dU = free[:-nx].reshape(N, K)[:, nx:]
        half = 0.5 * np.abs(dU).max()
        tl, tu = np.maximum(lb, Uh.min(0) - half), np.minimum(ub, Uh.max(0) + half)
        held = held_mask(model, N, Vh, tl, tu, 0)
        info = {}
        cl = riccati_rti_step(model, N, H, Vh, up, tr, w, x0m, exact, tl, tu, clamp=True, info=info)
        Un = info["V_new"][:-nx].reshape(N, K)[:, nx:]
        assert ((Un >= tl) & (Un <= tu)).all(), "every new control inside the box bit for bit"
        assert (cl[:-nx].reshape(N, K)[:, nx:][held] == 0.0).all()
        some |= bool(info["clamped"][~held].any())
        not_all |= not info["clamped"][~held].all()
        for k in range(N):   # the linearised dynamics with the clamped du
            Ac, Bc, xd = _jac(model, Vh[k * K:k * K + nx], Vh[k * K + nx:(k + 1) * K])
            c = Vh[k * K:k * K + nx] + H * xd - Vh[(k + 1) * K:(k + 1) * K + nx]
            want = (np.eye(nx) + H * Ac) @ cl[k * K:k * K + nx] + H * Bc @ cl[k * K + nx:(k + 1) * K] + c
            assert np.abs(cl[(k + 1) * K:(k + 1) * K + nx] - want).max() <= TOL * max(1.0, np.abs(want).max())
    assert some and not_all, "the tight box must clamp some free controls and not all"


def newton_errors(model, N, B, delta, steps):
    """|V_n - V*_new|_inf [B, steps + 1] of the iterated reference step from V* at x0 + delta"""
    nx, _ = oracle.DIMS[model]
    x0, up, tr = oracle.synth(SEED, 0, B, N, H, model=model)
    kw = dict(model=model, hessian=oracle.HESS_EXACT, tol_grad=1e-11, tol_defect=1e-12)
    o = oracle.solve_batch(N, H, x0, up, tr, W_2L, **kw)
    assert (o["status"] == 0).all()
    r = np.random.default_rng(SEED + 7 * N + B).standard_normal((B, nx))
    x1 = x0 + delta * r / np.abs(r).max(axis=1, keepdims=True)
    o2 = oracle.solve_batch(N, H, x1, up, tr, W_2L, V=o["V"], **kw)
    assert (o2["status"] == 0).all()
    errs = np.zeros((B, steps + 1))
    for b in range(B):
        V = o["V"][b].copy()
        errs[b, 0] = np.abs(V - o2["V"][b]).max()
        for n in range(steps):
            V = V + dense_rti_step(model, N, H, V, up[b], tr[b], W_2L, x1[b], True)
            errs[b, n + 1] = np.abs(V - o2["V"][b]).max()
    return errs


def test_iterated_step_is_newtons_method():
    errs = newton_errors(oracle.TWO_LINK, 17, 5, DELTA, N_STAR + 2)
    for b, e in enumerate(errs):
        print(f"instance {b}: " + " ".join(f"{v:.2e}" for v in e))
    falling = errs[:, 1:] < 0.5 * errs[:, :-1]
    n_star = [int(np.argmin(f)) if not f.all() else f.size for f in falling]   # steps until it stops falling
    print(f"n* per instance {n_star}, error reached {errs[:, N_STAR:].max():.2e}")
    assert max(n_star) == N_STAR, n_star
    assert errs[:, N_STAR:].max() <= ERR_REACHED, errs[:, N_STAR:].max()
    for b in range(errs.shape[0]):
        ratios = errs[b, :n_star[b]] / errs[b, 1:n_star[b] + 1]
        assert (ratios[:-1] >= CONTRACTION).all() and ratios[0] >= CONTRACTION, (b, ratios)
