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
   test of the Newton iteration (tests/test_gpu_rti.py) takes its step count and its bound from them.
4. the generated models: every zoo case of tests/test_gpu_rti_edges.py (ZOO_FREE, ZOO_CLAMPED) at the oracle's plan of
   tests/test_user_model_sens_reference.py shifted by one stage, x0_meas as the GPU module draws it: recursion against
   the dense KKT solve at 1e-10 max(1, max |ref|), both Hessians (measured <= 1.7e-12, cart_pole (33, 65)); the step
   does not vanish (max |dV| >= 2.9e-2); the exact QP is positive definite on every instance, the M_uu eigenvalue ratio
   of exact_qp_ratio at least 0.54.  The two ubound cases: the clamp tests' tight box (tight_box) acts on 16 and 7 of
   37 instances.  The shapes that module has no seed for, cart_pole (4, 5) (6, 5) (7, 5), take seed 0, the first at
   which the oracle converges on every instance (ZOO_SEEDS).
5. the growth g = overflow_growth of the forward sweep (the reference step at x^_0 + 1e300, over 1e300), instance 0,
   exact Hessian: 2-link N = 17 2.2410 (clamped at +-2: 1.3330), exo N = 7 1.4137, 2-link N = 5 1.0100.  The first three
   are >= 1.2, so at x0_meas = 1.7e308 the sweep passes DBL_MAX by 13 % or more; the reference's own sweep there is
   first non-finite at stage 3, 4 and 2: after the plan's first stages have been overwritten.  The undo-log test of
   tests/test_gpu_rti_edges.py rests on this."""
import numpy as np
import pytest

import oracle_lib as oracle
import test_user_model_sens_reference as zoo
from rti_reference import (dense_rti_step, exact_qp_ratio, first_nonfinite_stage, overflow_growth, riccati_rti_step,
                           riccati_rti_step_batch, shift_plan)
from sens_reference import _jac, held_mask
from test_solve_vjp_reference import CASES, PM2, SEED, H, W_2L, solved

TOL = 1e-10
# 4. the zoo's cases of tests/test_gpu_rti_edges.py.  The shapes tests/test_user_model_sens_reference.py has no seed
# for take the first seed from 0 at which the oracle converges on every instance (its rule; asserted below)
ZOO_SEEDS = {("free", "cart_pole", 4, 5): 0, ("free", "cart_pole", 6, 5): 0, ("free", "cart_pole", 7, 5): 0}
ZOO_FREE = ([("free", "cart_pole", N, B) for (N, B) in [(1, 5), (2, 3), (3, 9), (33, 65), (4, 5), (6, 5), (7, 5)]]
            + [("free", model, N, B) for model in ("motor_pendulum", "unicycle") for (N, B) in [(1, 5), (3, 9), (17, 37)]]
            + [("free", "mass_chain", 1, 5), ("free", "mass_chain", 5, 9)])
ZOO_CLAMPED = [("ubound", "cart_pole", 17, 37), ("ubound", "unicycle", 17, 37)]
# 5. name: (model, N, bounds of the plan, clamp, relied on by the GPU's undo-log test, g as measured)
G_MIN = 1.2
GROWTH = {"2-link N=17": (oracle.TWO_LINK, 17, PM2, False, True, 2.24),
          "2-link N=17 clamped": (oracle.TWO_LINK, 17, PM2, True, True, 1.33),
          "exo N=7": (oracle.EXO, 7, None, False, True, 1.41),
          "2-link N=5": (oracle.TWO_LINK, 5, None, False, False, 1.010)}
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


# ---------------------------------------------------------------- 4. the generated models (the zoo)
def zoo_seed(case):
    return ZOO_SEEDS[case] if case in ZOO_SEEDS else zoo.SEEDS[case]


def zoo_shifted(case):
    """(model id, w, lb, ub, V^ [B, NV], u_prev [B, nu], traj, x0_meas [B, nx]) of a zoo case at the oracle's plans
    shifted by one stage; x0_meas as tests/test_gpu_rti.py draws it"""
    _, model, N, B = case
    nx, nu = zoo.DIMS[model]
    x0, up, tr, o = zoo.solved(case, zoo_seed(case))
    assert (o["status"] == 0).all(), "the oracle must converge on every instance"
    mid = zoo.use(model)
    rows = [shift_plan(mid, N, zoo.H, o["V"][b]) for b in range(B)]
    Vh, uph = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    x0m = Vh[:, :nx] + 1e-2 * np.random.default_rng(SEED + 13 * N + B).standard_normal((B, nx))
    lb, ub, _, _ = zoo.case_bounds(case)
    return mid, zoo.weights(nx, nu), lb, ub, Vh, uph, tr, x0m


def tight_box(lb, ub, Uh, free_dU):
    """the per-instance box of the clamp tests: around the plan's own controls [B, N, nu], half of the largest free
    step wide, intersected with (lb, ub) [nu]; a side of (lb, ub) that is no bound (|.| >= 1e19) stays as it is"""
    half = 0.5 * np.abs(free_dU).max(axis=(1, 2))[:, None]
    tl, tu = np.maximum(lb[None, :], Uh.min(1) - half), np.minimum(ub[None, :], Uh.max(1) + half)
    return np.where(np.abs(lb) < 1e19, tl, lb[None, :]), np.where(np.abs(ub) < 1e19, tu, ub[None, :])


@pytest.mark.parametrize("case", ZOO_FREE + ZOO_CLAMPED, ids=zoo._id)
def test_zoo_recursion_matches_the_dense_kkt_solve(case):
    kind, model, N, B = case
    nx, nu = zoo.DIMS[model]
    mid, w, lb, ub, Vh, up, tr, x0m = zoo_shifted(case)
    worst, big, ratios = 0.0, 0.0, []
    for b in range(B):
        ratios.append(exact_qp_ratio(mid, N, zoo.H, Vh[b], up[b], tr[b], w, lb, ub))
        for exact in (True, False):
            d = dense_rti_step(mid, N, zoo.H, Vh[b], up[b], tr[b], w, x0m[b], exact, lb, ub)
            r = riccati_rti_step(mid, N, zoo.H, Vh[b], up[b], tr[b], w, x0m[b], exact, lb, ub)
            err, scale = np.abs(d - r).max(), max(1.0, np.abs(d).max())
            worst, big = max(worst, err / scale), max(big, np.abs(d).max())
            assert err <= TOL * scale, (b, exact, err)
    print(f"{zoo._id(case)} seed {zoo_seed(case)}: recursion against dense {worst:.3e}, max |dV| {big:.3e}, exact M_uu "
          f"eigenvalue ratio {min(ratios):.3e} .. {max(ratios):.3e}, {sum(r <= 0 for r in ratios)} instances not definite")
    assert big > 1e-3, "the shifted plan is no solution: the step must not vanish"
    assert min(abs(r) for r in ratios) > 1e-9, "status 0 or 1 must not hang on rounding"
    if kind != "ubound":
        return
    # the clamp tests' tight box: it must act on some instances' free controls and not on all of them
    K = nx + nu
    Uh = Vh[:, :-nx].reshape(B, N, K)[:, :, nx:]
    for exact in (True, False):
        free, _, _ = riccati_rti_step_batch(mid, N, zoo.H, Vh, up, tr, w, x0m, exact, lb, ub)
        tl, tu = tight_box(lb, ub, Uh, free[:, :-nx].reshape(B, N, K)[:, :, nx:])
        held = np.stack([held_mask(mid, N, Vh[b], tl[b], tu[b], 0) for b in range(B)])
        _, _, clamped = riccati_rti_step_batch(mid, N, zoo.H, Vh, up, tr, w, x0m, exact, tl, tu, clamp=True)
        acts = np.array([clamped[b][~held[b]].any() for b in range(B)])
        print(f"{zoo._id(case)} exact={exact}: the tight box acts on {int(acts.sum())} of {B} instances")
        assert acts.any() and not acts.all()


def test_new_zoo_seeds_are_the_first_at_which_the_oracle_converges():
    for case, seed in ZOO_SEEDS.items():
        for s in range(seed + 1):
            conv = bool((zoo.solved(case, s)[3]["status"] == 0).all())
            assert conv == (s == seed), (case, s, conv)


# ---------------------------------------------------------------- 5. the growth that makes 1.7e308 overflow
def growth_case(name):
    """(the arguments of overflow_growth after h, as a tuple) of a GROWTH case, instance 0, exact Hessian"""
    model, N, bounds, clamp = GROWTH[name][:4]
    w, lb, ub, Vh, up, tr, _ = shifted(model, N, 0, bounds)
    if not clamp:
        lb = ub = None
    return (model, N, H, Vh, up, tr, w, True, lb, ub, clamp)


@pytest.mark.parametrize("name", GROWTH)
def test_growth_of_the_forward_sweep(name):
    """g of rti_reference.overflow_growth and the first stage at which the sweep at x0_meas = 1.7e308 is not finite;
    the undo-log test of tests/test_gpu_rti_edges.py relies on g >= 1.2 for the cases marked so"""
    args = growth_case(name)
    g, k = overflow_growth(*args), first_nonfinite_stage(*args)
    print(f"{name}: g = {g:.4f}, first non-finite stage at 1.7e308: {k}")
    relied_on, recorded = GROWTH[name][4:]
    assert abs(g - recorded) <= 0.01 * recorded, "the recorded value is the measured one"
    if relied_on:
        assert g >= G_MIN
        assert k is not None and k >= 1, "the plan has been overwritten when the overflow shows"
