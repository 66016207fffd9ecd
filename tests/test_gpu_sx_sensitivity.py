"""GPU: the sensitivity kernels of GENERATED models' libraries (gain_lane_kernel, gain_group_kernel,
adjoint_lane_kernel and their state-bounded instantiations, compiled into every lib/user/<name>.so from
csrc/gain_sweep.h, csrc/adjoint_sweep.h and csrc/sens_lane_stage.inc) against the dense references of
tests/sens_reference.py.

The built-in models are second order with NQ = NA = nx / 2, an even K = nx + nu and nu >= 2.  The zoo's models
(host/examples/sx_model_zoo.cpp) reach the instantiations they do not: cart_pole (nx 4, nu 1, NQ 2: a 1 x 1 factor, a
one-bit held mask, odd K = 5), unicycle (4, 2, NQ 0: NA = NX, no kinematic rows), motor_pendulum (3, 1, NQ 1: NA = 2,
K = 4) and mass_chain (12, 4, NQ 6: K = 16, the lane kernels only).

Solvers: the generated library at the test's own horizon, through a JSON written with dll_filepath = the absolute
lib/user/<name>.so; h = 0.01.  Inputs: test_gpu_sx_models.instances(nx, nu, B, N, h, seed) and weights(nx, nu).  Plans:
V* of the GPU solve, status 0 everywhere (asserted).  References: dense, with the model's Jacobians from the host build
of the generated header (pinned to sympy in tests/test_sx_models.py) and W_k from the oracle.  Tolerance of every
comparison with the dense reference: 1e-10 max(1, max |ref|), per stage for the gains, per instance and output array
for the VJP -- the project's standing GPU-versus-reference tolerance.

Cases, seeds and what was checked on the CPU before fixing them are those of tests/test_user_model_sens_reference.py
(its docstring: for every case the first seed from 0 upward at which the oracle converges on every instance, the free
part of every tail H_UU under the exact Hessian is positive definite with min / max eigenvalue > 1e-9, so that status
0 is what the definition gives, and the CPU recursion agrees with the dense reference to 1e-12; seed 0 everywhere but
cart_pole (33, 65): 60 and motor_pendulum (17, 37): 1).  No seed was chosen from a GPU result.

Shapes (N, B): cart_pole (1, 5) (2, 3) (3, 9) (17, 37) (33, 65), unicycle and motor_pendulum (1, 5) (3, 9) (17, 37),
mass_chain (1, 5) (5, 9) -- N = 1 has no recursion, 17 and 33 are one stage past the rounds of 16, 5 and 37 leave a
partial workgroup and a partial wave, 65 starts a second wave and a second block of the adjoint records.

a. gain parity: lane and 16-lane kernel, both Hessians, n_gain in {1, N}, status 0.  mass_chain: the lane kernel, and
   kernel = AUTO returns its gains bit for bit (kernel = 2 is refused: tests/test_feedback_gains_api.py).
b. VJP parity: all five outputs, both Hessians, vjp_status 0; the workspace is ceil(B / 64) N nu (K + 1) 64 doubles.
c. the test can tell: per model at its largest case the dense G_exact and G_GN differ by >= 1000 x the tolerance of a
   (asserted on the reference; CPU values in GGAP of the reference module: 0.63, 6.9e-2, 1.8e-2, 2.4e-4, no target was
   scaled), and the GPU's GAUSS_NEWTON gains match the Gauss-Newton reference and miss the exact one.
d. control bounds at (17, 37): cart_pole under +-1.5 N with the targets times 4, unicycle with the acceleration
   bounded from above only (the other three entries -inf, -1e30, +inf); shared and as a [B, nu] table at a padded
   stride with NaN in the padding and buffers of the exact size.  At least one held and one free control per case (on
   cart_pole that is a stage with its only control held and one with it free); held rows of G and held entries of
   adj_V exactly 0, the rest at the tolerance.  Both gain kernels and the VJP.
e. pins: cart_pole (17, 37), n_pin = 2: G_0, G_1, adj_V on u_0, u_1 and u_prev_bar exactly 0, the rest at the tolerance.
f. state bounds under the sensitivity barrier: cart_pole under XL / XU of test_gpu_sx_variants.py at (3, 9) and (17, 9),
   the plan from the 16-lane interior-point solve with the Hessian the library resolves.  At sigma_cap = 1e6 both gain
   kernels and the VJP at the tolerance; at the defaults within 10 x the CPU floor (FLOOR of the reference module; at
   (3, 9) no state is near its bound and the floor is plain roundoff, at (17, 9) one entry is over the cap).  An instance
   with a state outside its box reports 2 with zeros; its workgroup-mates are bit for bit those of the clean batch.
g. the solver's own map: cart_pole (17, 5), 16-lane solves at tol_grad 1e-11 / tol_defect 1e-12, central differences at
   delta = 1e-4 in each of the nx + nu directions, warm-started from V*, against the exact G_0 at 1e-6 max(1, |G_0|)
   (the same experiment with the oracle on the CPU: 5.3e-9).
h. failure isolation and bits, motor_pendulum (17, 37): a NaN in V gives status 2 and zeros for that instance, its
   workgroup- and wave-mates bit for bit unchanged; host entries equal the device entries; B = 1; run-to-run
   determinism.

Measured on one MI355X, worst err / bound: gains (lane | 16-lane) cart_pole 6.2e-5 | 6.2e-5, unicycle 3.4e-5 | 3.7e-5,
motor_pendulum 2.8e-5 | 2.6e-5, mass_chain 2.7e-5; VJP 9.1e-3, 4.3e-4, 7.5e-3, 5.0e-5 (weights_bar and x0_bar at the long
horizons, where the CPU recursion is as far from the dense solve); d: gains 3.6e-5, VJP 1.0e-3; e: 3.1e-5 and 7.6e-4;
f at cap 1e6: 7.6e-4; at the defaults 0.11 and 0.25 of 10 x the floor; g: 1.4e-8 against the bound of 1e-6.

The tests skip only when a generated library is missing (as test_gpu_sx_models.solver does)."""
import os

import numpy as np
import pytest

from sens_reference import (CAP_DEFAULT, OUT, dense_vjp_batch, gains_batch, xb_dense_gains_batch, xb_dense_vjp_batch)
from test_gpu_feedback_gains import gpu_gains, hess_id
from test_gpu_solve_vjp import gpu_vjp
from test_gpu_sx_models import USER, weights
from test_gpu_xb_sensitivity import worst_gain, worst_vjp
from test_user_model_sens_reference import (DIMS, FLOOR, H, LARGEST, SHAPES, UBOUND, case_bounds, case_inputs,
                                            fd_of_u0, held_controls, use, vbar)
from test_xb_sensitivity_reference import CAP_PIN

pytestmark = pytest.mark.gpu

TOL = 1e-10
KERNELS = {"lane": 1, "group": 2}


def kernels_of(model):
    """the gain kernels a model's library runs: the 16-lane kernel holds one column per lane, K <= 15"""
    return ["lane"] if sum(DIMS[model]) >= 16 else list(KERNELS)


def _id(v):
    return "-".join(str(x) for x in v)


PARITY = [(model, N, B) for model, shapes in SHAPES.items() for (N, B) in shapes]
GAIN_PARITY = [(model, N, B, kernel, hess) for (model, N, B) in PARITY for kernel in kernels_of(model)
               for hess in ("exact", "gn")]
VJP_PARITY = [(model, N, B, hess) for (model, N, B) in PARITY for hess in ("exact", "gn")]
XB_CASES = [("xb", "cart_pole", 3, 9), ("xb", "cart_pole", 17, 9)]


class Ctx:
    """the module's shared state: inputs, GPU plans and dense references, each computed once and left unchanged"""

    def __init__(self, m, d):
        self.m, self.dir = m, d
        self.inputs_, self.plans_, self.refs_ = {}, {}, {}

    def solver(self, case, cap=None, **kw):
        """the generated library of the case's model at the case's horizon, with the case's state bounds; cap: the
        sensitivity barrier at (mu_f, cap), None: off"""
        kind, model, N, _ = case
        so = os.path.join(USER, f"{model}.so")
        if not os.path.exists(so):
            pytest.skip(f"{model} not generated")
        nx, nu = DIMS[model]
        p = self.m.write_model_json(os.path.join(self.dir, f"{model}_{N}.json"), model, nx, nu, 10000, N,
                                    dll_filepath=so, model=model)
        kw.setdefault("max_iter", 100)
        s = self.m.Solver(p, **kw)
        assert s.info.model_id == self.m.MODEL_USER and (s.nx, s.nu, s.N) == (nx, nu, N) and abs(s.h - H) < 1e-15
        if kind == "xb":
            s.set_state_bounds(*case_bounds(case)[2:])
        if cap is not None:
            s.set_sensitivity_barrier(sigma_cap=cap)
        return s

    def inputs(self, case):
        """(x0, up, tr, V_bar)"""
        if case not in self.inputs_:
            arrs = case_inputs(case) + (vbar(case),)
            for a in arrs:
                a.setflags(write=False)
            self.inputs_[case] = arrs
        return self.inputs_[case]

    def plan(self, case):
        """V* of the GPU solve [B, NV]; xb cases: the 16-lane interior-point solve"""
        if case not in self.plans_:
            kind, model, N, B = case
            x0, up, tr, _ = self.inputs(case)
            lb, ub, _, _ = case_bounds(case)
            s = self.solver(case, **(dict(kkt_solver=self.m.KKT_RICCATI_GROUP) if kind == "xb" else {}))
            g = s.solve_batch_host(x0, up, tr, weights(*DIMS[model]), u_lb=lb, u_ub=ub)
            s.close()
            assert (g["status"] == 0).all(), g["status"]
            g["V"].setflags(write=False)
            self.plans_[case] = g["V"]
        return self.plans_[case]

    def ref(self, case, exact, n_pin=0, cap=None):
        """the dense references at the plan: (G [B, N, nu, K], the VJP outputs)"""
        key = (case, exact, n_pin, cap)
        if key not in self.refs_:
            kind, model, N, B = case
            _, up, tr, Vbar = self.inputs(case)
            lb, ub, xl, xu = case_bounds(case)
            V, w = self.plan(case), weights(*DIMS[model])
            mid = use(model)   # the oracle has one USER slot: before every reference
            if kind == "xb":
                G = xb_dense_gains_batch(mid, N, H, V, up, tr, w, exact, xl, xu, n_pin=n_pin, cap=cap)
                r = xb_dense_vjp_batch(mid, N, H, V, up, tr, w, Vbar, exact, xl, xu, n_pin=n_pin, cap=cap)
            else:
                G = gains_batch(mid, N, H, V, up, tr, w, exact, lb, ub, n_pin)
                r = dense_vjp_batch(mid, N, H, V, up, tr, w, Vbar, exact, lb, ub, n_pin)
            for a in (G,) + tuple(r.values()):
                a.setflags(write=False)
            self.refs_[key] = (G, r)
        return self.refs_[key]


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return Ctx(mmpc_mod, str(tmp_path_factory.mktemp("sx_sensitivity")))


def controls(case, adj_V):
    """[B, N, nu] view of the control entries of adj_V"""
    _, model, N, _ = case
    nx, nu = DIMS[model]
    return adj_V[:, :-nx].reshape(adj_V.shape[0], N, nx + nu)[:, :, nx:]


def table(rows, stride):
    """[B, nu] rows at a padded stride in a buffer of the exact size, NaN in the padding"""
    B, nu = rows.shape
    t = np.full((B - 1) * stride + nu, np.nan)
    for b in range(B):
        t[b * stride:b * stride + nu] = rows[b]
    return t


# ---------------------------------------------------------------- a. gain parity
@pytest.mark.parametrize("par", GAIN_PARITY, ids=_id)
def test_gains_match_the_dense_reference(par, ctx):
    model, N, B, kernel, hess = par
    case = ("free", model, N, B)
    _, up, tr, _ = ctx.inputs(case)
    V = ctx.plan(case)
    Gref, _ = ctx.ref(case, hess == "exact")
    s = ctx.solver(case)
    worst = 0.0
    for n_gain in sorted({1, N}):
        G, st = gpu_gains(s, V, up, tr, weights(*DIMS[model]), n_gain=n_gain, hessian=hess_id(ctx.m, hess),
                          kernel=KERNELS[kernel])
        assert (st == 0).all(), st
        worst = max(worst, worst_gain(G, Gref[:, :n_gain]))
    s.close()
    print(f"gains {_id(par)}: worst err / max(1, |ref|) = {worst:.3e}, over the bound = {worst / TOL:.3e}")
    assert worst <= TOL


@pytest.mark.parametrize("shape", SHAPES["mass_chain"], ids=_id)
def test_auto_is_the_lane_kernel_at_sixteen_columns(shape, ctx):
    case = ("free", "mass_chain") + shape
    _, up, tr, _ = ctx.inputs(case)
    V = ctx.plan(case)
    s = ctx.solver(case)
    for hess in ("exact", "gn"):
        Gl, stl = gpu_gains(s, V, up, tr, weights(12, 4), hessian=hess_id(ctx.m, hess), kernel=ctx.m.GAIN_KERNEL_LANE)
        Ga, sta = gpu_gains(s, V, up, tr, weights(12, 4), hessian=hess_id(ctx.m, hess), kernel=ctx.m.GAIN_KERNEL_AUTO)
        assert (stl == 0).all() and np.array_equal(sta, stl)
        assert np.array_equal(Ga, Gl), "AUTO must resolve to the lane kernel"
    s.close()


# ---------------------------------------------------------------- b. VJP parity
@pytest.mark.parametrize("par", VJP_PARITY, ids=_id)
def test_vjp_outputs_match_the_dense_reference(par, ctx):
    model, N, B, hess = par
    nx, nu = DIMS[model]
    case = ("free", model, N, B)
    _, up, tr, Vbar = ctx.inputs(case)
    _, vref = ctx.ref(case, hess == "exact")
    s = ctx.solver(case)
    assert s.solve_vjp_workspace_bytes(B) == -(-B // 64) * N * nu * (nx + nu + 1) * 64 * 8
    r = gpu_vjp(s, ctx.plan(case), up, tr, weights(nx, nu), Vbar, hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["vjp_status"] == 0).all(), r["vjp_status"]
    worst = worst_vjp(r, vref)
    print(f"vjp {_id(par)}: worst err / max(1, |ref|) = {worst:.3e}, over the bound = {worst / TOL:.3e}")
    assert worst <= TOL


# ---------------------------------------------------------------- c. the test can tell
@pytest.mark.parametrize("model", SHAPES)
def test_gauss_newton_is_the_other_gain(model, ctx):
    N, B = LARGEST[model]
    case = ("free", model, N, B)
    _, up, tr, _ = ctx.inputs(case)
    V = ctx.plan(case)
    Ge, Gg = ctx.ref(case, True)[0], ctx.ref(case, False)[0]
    gap = np.abs(Ge - Gg).max()
    print(f"{model} ({N}, {B}): dense max |G_exact - G_GN| = {gap:.3e}, max |G_exact| = {np.abs(Ge).max():.3e}")
    assert gap >= 1000 * TOL * max(1.0, np.abs(Ge).max()), "the reference must tell the two Hessians apart"
    s = ctx.solver(case)
    for kernel in kernels_of(model):
        Gn, st = gpu_gains(s, V, up, tr, weights(*DIMS[model]), hessian=ctx.m.HESSIAN_GAUSS_NEWTON,
                           kernel=KERNELS[kernel])
        Ga, sta = gpu_gains(s, V, up, tr, weights(*DIMS[model]), hessian=ctx.m.HESSIAN_AUTO, kernel=KERNELS[kernel])
        assert (st == 0).all() and (sta == 0).all()
        assert worst_gain(Gn, Gg) <= TOL and worst_gain(Ga, Ge) <= TOL, kernel
        assert np.abs(Gn - Ge).max() >= 0.5 * gap and worst_gain(Gn, Ge) > 100 * TOL, kernel
    s.close()


# ---------------------------------------------------------------- d. control bounds
@pytest.mark.parametrize("form", ["shared", "table"])
@pytest.mark.parametrize("model", list(UBOUND))
def test_held_controls_get_zeros_and_the_rest_matches(model, form, ctx):
    case = ("ubound", model, 17, 37)
    _, _, N, B = case
    nx, nu = DIMS[model]
    w = weights(nx, nu)
    _, up, tr, Vbar = ctx.inputs(case)
    V = ctx.plan(case)
    lb, ub, _, _ = case_bounds(case)
    use(model)
    held = held_controls(case, V)
    print(f"{_id(case)}: {int(held.sum())} held controls of {held.size}")
    assert held.any() and not held.all(), "the case needs at least one held and one free control"
    if nu == 1:
        assert held.all(axis=2).any() and (~held).all(axis=2).any(), "a stage with its only control held, one with it free"
    if form == "shared":
        bl, bu, stride = lb, ub, 0
    else:
        stride = nu + 3
        bl, bu = table(np.tile(lb, (B, 1)), stride), table(np.tile(ub, (B, 1)), stride)
    s = ctx.solver(case)
    for hess in ("exact", "gn"):
        Gref, vref = ctx.ref(case, hess == "exact")
        assert (Gref[held] == 0.0).all() and (controls(case, vref["adj_V"])[held] == 0.0).all()
        for kernel in KERNELS:
            G, st = gpu_gains(s, V, up, tr, w, bl, bu, stride, hessian=hess_id(ctx.m, hess), kernel=KERNELS[kernel])
            assert (st == 0).all(), st
            assert (G[held] == 0.0).all(), "a held control's row of G_k must be exactly 0"
            worst = worst_gain(G, Gref)
            print(f"bounded gains {_id(case)} {form} {kernel} {hess}: over the bound = {worst / TOL:.3e}")
            assert worst <= TOL
        r = gpu_vjp(s, V, up, tr, w, Vbar, bl, bu, bounds_stride=stride, hessian=hess_id(ctx.m, hess))
        assert (r["vjp_status"] == 0).all(), r["vjp_status"]
        assert (controls(case, r["adj_V"])[held] == 0.0).all(), "adj_V must be exactly 0 on a held control"
        worst = worst_vjp(r, vref)
        print(f"bounded vjp {_id(case)} {form} {hess}: over the bound = {worst / TOL:.3e}")
        assert worst <= TOL
    s.close()


# ---------------------------------------------------------------- e. pins
def test_pinned_stages_get_zeros(ctx):
    case = ("free", "cart_pole", 17, 37)
    w = weights(4, 1)
    _, up, tr, Vbar = ctx.inputs(case)
    V = ctx.plan(case)
    Gref, vref = ctx.ref(case, True, n_pin=2)
    assert (Gref[:, :2] == 0.0).all() and (vref["u_prev_bar"] == 0.0).all()
    s = ctx.solver(case)
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr, w, n_pin=2, kernel=KERNELS[kernel])
        assert (st == 0).all(), st
        assert (G[:, :2] == 0.0).all() and np.abs(G[:, 2:]).max() > 0.1
        worst = worst_gain(G, Gref)
        print(f"pins gains {kernel}: over the bound = {worst / TOL:.3e}")
        assert worst <= TOL
    r = gpu_vjp(s, V, up, tr, w, Vbar, n_pin=2)
    s.close()
    assert (r["vjp_status"] == 0).all(), r["vjp_status"]
    aU = controls(case, r["adj_V"])
    assert (aU[:, :2] == 0.0).all() and (r["u_prev_bar"] == 0.0).all()
    assert np.abs(aU[:, 2:]).max() > 1e-3 and np.abs(r["x0_bar"]).max() > 1e-3
    worst = worst_vjp(r, vref)
    print(f"pins vjp: over the bound = {worst / TOL:.3e}")
    assert worst <= TOL


# ---------------------------------------------------------------- f. state bounds under the sensitivity barrier
def xb_run_all(ctx, case, hess, cap):
    """{what: worst err / max(1, |ref|)} of both gain kernels and the VJP of a state-bounded case against dense"""
    _, model, N, B = case
    w = weights(*DIMS[model])
    _, up, tr, Vbar = ctx.inputs(case)
    V = ctx.plan(case)
    Gref, vref = ctx.ref(case, hess == "exact", cap=cap)
    s = ctx.solver(case, cap=cap)
    out = {}
    for kernel in KERNELS:
        for n_gain in sorted({1, N}):
            G, st = gpu_gains(s, V, up, tr, w, n_gain=n_gain, hessian=hess_id(ctx.m, hess), kernel=KERNELS[kernel])
            assert (st == 0).all(), (kernel, st)
            out[f"{kernel} n_gain={n_gain}"] = worst_gain(G, Gref[:, :n_gain])
    r = gpu_vjp(s, V, up, tr, w, Vbar, hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["vjp_status"] == 0).all(), r["vjp_status"]
    out["vjp"] = worst_vjp(r, vref)
    print(f"barrier {_id(case)} {hess} cap {cap:.0e}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()))
    return out


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("case", XB_CASES, ids=_id)
def test_state_bounded_parity_at_cap_1e6(case, hess, ctx):
    out = xb_run_all(ctx, case, hess, CAP_PIN)
    assert max(out.values()) <= TOL, out


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("case", XB_CASES, ids=_id)
def test_state_bounded_defaults_within_ten_times_the_cpu_floor(case, hess, ctx):
    out = xb_run_all(ctx, case, hess, CAP_DEFAULT)
    print(f"barrier {_id(case)} {hess} defaults: worst over 10 x floor = {max(out.values()) / (10 * FLOOR[case]):.3e}")
    assert max(out.values()) <= 10 * FLOOR[case], out


def test_state_outside_its_box_fails_alone(ctx):
    case, bad = ("xb", "cart_pole", 17, 9), 5
    _, _, N, B = case
    w = weights(4, 1)
    _, up, tr, Vbar = ctx.inputs(case)
    V = ctx.plan(case)
    V2 = V.copy()
    V2[bad, 3 * 5 + 0] = 0.25   # the cart position of x_3, bounded by +-0.2
    others = np.arange(B) != bad
    s = ctx.solver(case, cap=CAP_DEFAULT)
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr, w, kernel=KERNELS[kernel])
        G2, st2 = gpu_gains(s, V2, up, tr, w, kernel=KERNELS[kernel])
        assert (st == 0).all()
        assert st2[bad] == 2 and (G2[bad] == 0.0).all(), (kernel, st2[bad])
        assert (st2[others] == 0).all()
        assert np.array_equal(G2[others], G[others]), "the neighbours of a failed instance must not change"
    r = gpu_vjp(s, V, up, tr, w, Vbar)
    r2 = gpu_vjp(s, V2, up, tr, w, Vbar)
    s.close()
    assert (r["vjp_status"] == 0).all() and r2["vjp_status"][bad] == 2 and (r2["vjp_status"][others] == 0).all()
    for k in OUT:
        assert (r2[k][bad] == 0.0).all(), k
        assert np.array_equal(r2[k][others], r[k][others]), k


# ---------------------------------------------------------------- g. the solver's own map
def test_exact_gain_is_the_derivative_of_the_solve(ctx):
    case = ("free", "cart_pole", 17, 5)
    _, model, N, B = case
    nx, nu = DIMS[model]
    m, w = ctx.m, weights(nx, nu)
    x0, up, tr, _ = ctx.inputs(case)
    s = ctx.solver(case, kkt_solver=m.KKT_RICCATI_GROUP, tol_grad=1e-11, tol_defect=1e-12)
    assert s.hessian_for(B) == m.HESSIAN_EXACT
    g = s.solve_batch_host(x0, up, tr, w)
    assert (g["status"] == 0).all()
    V = g["V"]
    G0, st = s.feedback_gains_host(V, up, tr, w, n_gain=1, hessian=m.HESSIAN_EXACT)
    assert (st == 0).all()
    G0 = G0[:, 0]

    def solve(xs, us):
        r = s.solve_batch_host(xs, us, tr, w, V=V)
        assert (r["status"] == 0).all(), r["status"]
        return r["V"]

    fd = fd_of_u0(solve, x0, up, nx, nu, delta=1e-4)
    s.close()
    err = np.abs(fd - G0).max(axis=(1, 2))
    bound = 1e-6 * np.maximum(1.0, np.abs(G0).max(axis=(1, 2)))
    print(f"central differences of the solve against G_0: max {err.max():.3e} (bound {bound.min():.1e})")
    assert (err <= bound).all(), (err, bound)


# ---------------------------------------------------------------- h. failure isolation and bits
def test_nan_instance_fails_alone(ctx):
    case, bad = ("free", "motor_pendulum", 17, 37), 5
    _, model, N, B = case
    w = weights(*DIMS[model])
    _, up, tr, Vbar = ctx.inputs(case)
    V = ctx.plan(case)
    V2 = V.copy()
    V2[bad, 3 * 4 + 1] = np.nan   # a rate of x_3
    others = np.arange(B) != bad
    s = ctx.solver(case)
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr, w, kernel=KERNELS[kernel])
        G2, st2 = gpu_gains(s, V2, up, tr, w, kernel=KERNELS[kernel])
        assert (st == 0).all()
        assert st2[bad] == 2 and (G2[bad] == 0.0).all(), (kernel, st2[bad])
        assert (st2[others] == 0).all()
        assert np.array_equal(G2[others], G[others]), "the neighbours of a failed instance must not change"
    r = gpu_vjp(s, V, up, tr, w, Vbar)
    r2 = gpu_vjp(s, V2, up, tr, w, Vbar)
    s.close()
    assert (r["vjp_status"] == 0).all() and r2["vjp_status"][bad] == 2 and (r2["vjp_status"][others] == 0).all()
    for k in OUT:
        assert (r2[k][bad] == 0.0).all(), k
        assert np.array_equal(r2[k][others], r[k][others]), k


def test_host_entries_single_instance_and_determinism(ctx):
    case = ("free", "motor_pendulum", 17, 37)
    _, model, N, B = case
    w = weights(*DIMS[model])
    _, up, tr, Vbar = ctx.inputs(case)
    V = ctx.plan(case)
    Gref, vref = ctx.ref(case, True)
    s = ctx.solver(case)
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr, w, kernel=KERNELS[kernel])
        Gr, str_ = gpu_gains(s, V, up, tr, w, kernel=KERNELS[kernel])
        assert np.array_equal(G, Gr) and np.array_equal(st, str_), "run to run"
        Gh, sth = s.feedback_gains_host(V, up, tr, w, kernel=KERNELS[kernel])
        assert np.array_equal(Gh, G) and np.array_equal(sth, st), "host entry against the device entry"
        G1, st1 = s.feedback_gains_host(V[3:4], up[3:4], tr[3:4], w, n_gain=8, kernel=KERNELS[kernel])
        assert st1.tolist() == [0] and worst_gain(G1, Gref[3:4, :8]) <= TOL
    r = gpu_vjp(s, V, up, tr, w, Vbar)
    again = gpu_vjp(s, V, up, tr, w, Vbar)
    host = s.solve_vjp_host(V, up, tr, w, Vbar)
    one = s.solve_vjp_host(V[3:4], up[3:4], tr[3:4], w, Vbar[3:4])
    s.close()
    for k in OUT + ("vjp_status",):
        assert np.array_equal(r[k], again[k]), f"{k}: run to run"
        assert np.array_equal(r[k], host[k]), f"{k}: host entry against the device entry"
    assert one["vjp_status"].tolist() == [0] and worst_vjp(one, {k: v[3:4] for k, v in vref.items()}) <= TOL
