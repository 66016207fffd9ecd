"""GPU: the real-time iteration kernels (csrc/rti_sweep.h) where tests/test_gpu_rti.py does not
reach: the undo log's restore path, the clamped forward pass beyond one block of the 2-link arm, the ring depths
D = rti_ring_slots(nx, nu) in {1, 3, 4} at every horizon edge, and every generated model of the zoo.

Helpers, linearisation points and the tolerance are those of tests/test_gpu_rti.py: the GPU plan shifted one stage by
rti_reference.shift_plan, x0_meas = x^_0 + 1e-2 N(0, 1) from default_rng(SEED + 13 N + B), every numeric comparison
per instance at 1e-10 max(1, max |ref|).  Built-in models through test_gpu_rti.RCtx, the zoo through
test_gpu_sx_sensitivity.Ctx with the inputs, bounds and step of tests/test_user_model_sens_reference.py.  The CPU
preconditions of every reference used here are in tests/test_rti_reference.py (items 4 and 5).

A1. the undo log.  One instance gets x0_meas = 1.7e308 in every entry: finite, so dx_0 is finite and the early exit
    does not fire; the sweep overflows after V has been overwritten, and the restore loop is what keeps V.  The instance
    is the first of the batch (the first with b >= 64 in the two-block case) whose growth g = overflow_growth (the
    reference step at x^_0 + 1e300, over 1e300) reaches 1.2 at the GPU's own V^: at 1.7e308 the sweep then passes
    DBL_MAX by 13 % or more, whatever the order of its sums.  Cases: 2-link (17, 37) unbounded and clamped at +-2,
    exo (7, 9), 2-link (4, 130) with the instance in the second block (short horizons grow little: at the oracle's
    plans instance 104 is the first of 64..129 to reach 1.2, with g = 1.2153, which puts 1.7e308 g = 2.07e308 15 % past
    DBL_MAX).  Asserted: prep_status 0 everywhere, status 2 / V bit for bit V^ / u0 the plan's own / step_inf inf for the
    instance, every other instance bit for bit the clean batch's; then a second feedback launch on the same workspace
    and the same V tensor with the clean x0_meas is bit for bit the clean batch, the failed instance included (the
    feedback steps V in place, so the rows of the instances that succeeded are set back to V^ before it; the failed
    instance's row is what the restore loop left).
    The instances used and their g are in the test's docstring.
A2. the clamped forward pass (the construction of test_gpu_rti.test_clamped_forward_pass: a per-instance box around
    the plan's own controls, half the largest free step wide, to both launches as a per-instance table, both
    Hessians): exo (7, 70) (D = 1, two blocks, the last partial) and (21, 9); 2-link (4, 130) at stride nu + 3 with
    NaN padding in a buffer of the exact size (three blocks, two lanes in the last; the boxes differ per instance, so
    a row read at the wrong instance leaves its box) and (2, 64) (one full block); cart_pole and unicycle (17, 37)
    under UBOUND intersected with the tight box, unicycle's -inf / -1e30 / +inf sides kept as they are.
A3. ring depth and the zoo, unclamped, both Hessians, against dense_rti_step: cart_pole (D = 4) at (1, 5) (2, 3) (3, 9)
    (33, 65) and N = 4, 6, 7 with B = 5 (N < D and every residue N mod 4); motor_pendulum and unicycle (1, 5) (3, 9)
    (17, 37); mass_chain (K = 16: D = 1, the record of 272 doubles) (1, 5) (5, 9); 2-link (4, 5) (5, 5) (the residues
    of D = 3 the other module leaves).  Where the reference's exact QP is not positive definite for an instance (the
    sign of rti_reference.exact_qp_ratio, which must be 1e-9 away from 0) the instance is held to the Gauss-Newton
    reference with status 1.  mass_chain's shift at (5, 9), n = 1 and n = 5.
    Seeds of the new cart_pole shapes (4, 5) (6, 5) (7, 5): 0, 0, 0 -- the first seed from 0 at which the oracle
    converges on every instance (tests/test_rti_reference.py: ZOO_SEEDS, asserted there on the CPU).
A4. isolation on the D = 1 and scratch kernels: a NaN in one instance's V^ and in its x0_meas, exo (7, 70) with the
    instance at b = 66 (clamped at the exo's box) and mass_chain (5, 9); the assertions of
    test_gpu_rti.test_nan_instance_fails_alone.

The tests skip only when a generated library is missing (as the zoo's modules do)."""
import numpy as np
import pytest

from rti_reference import (dense_rti_step, exact_qp_ratio, overflow_growth, riccati_rti_step_batch, shift_plan)
from sens_reference import _jac, held_mask
from test_gpu_feedback_gains import DIMS, H, OMODEL, SEED, WEIGHTS, dev, hess_id
from test_gpu_rti import RCtx, check, check_outputs, gpu_rti, table
from test_gpu_rti_shift import check_shift, gpu_shift
from test_gpu_rti_shift import reference as shift_reference
from test_gpu_sx_models import weights as sx_weights
from test_gpu_sx_sensitivity import Ctx as SxCtx
from test_rti_reference import G_MIN, ZOO_SEEDS, tight_box
from test_user_model_sens_reference import DIMS as ZDIMS
from test_user_model_sens_reference import H as H_SX
from test_user_model_sens_reference import case_bounds, case_inputs, use

pytestmark = pytest.mark.gpu

TOL = 1e-10
BIG = 1.7e308


def _id(case):
    return "-".join(str(v) for v in case)


class ZCtx(SxCtx):
    """test_gpu_sx_sensitivity's shared state, with the inputs of the shapes that module has no seed for"""

    def inputs(self, case):
        if case in ZOO_SEEDS and case not in self.inputs_:
            arrs = case_inputs(case, seed=ZOO_SEEDS[case])
            for a in arrs:
                a.setflags(write=False)
            self.inputs_[case] = arrs + (None,)
        return super().inputs(case)


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return RCtx(mmpc_mod, str(tmp_path_factory.mktemp("rti_edges")))


@pytest.fixture(scope="module")
def zctx(mmpc_mod, tmp_path_factory):
    z = ZCtx(mmpc_mod, str(tmp_path_factory.mktemp("rti_edges_sx")))
    z.hats_ = {}
    return z


class Prob:
    """one case: its dimensions, step, weights, bounds (lb, ub: [nu] or None), the shifted GPU plans V^ [B, NV] with
    u_prev and x0_meas, the targets; om() is the oracle's model id (a zoo model is registered again by every call: the
    oracle has one USER slot), solver() a new solver at the case's horizon"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.K = self.nx + self.nu

    def U(self, V):
        """[B, N, nu] view of the control entries of V"""
        return V[:, :-self.nx].reshape(V.shape[0], self.N, self.K)[:, :, self.nx:]


def builtin(ctx, model, N, B, bounded=False):
    nx, nu = DIMS[model]
    _, _, tr = ctx.inputs(model, N, B)
    Vh, up, x0m = ctx.hat(model, N, B, bounded)
    lb, ub = ctx.bounds(model, bounded)
    return Prob(name=_id((model, N, B)), nx=nx, nu=nu, N=N, B=B, h=H, w=WEIGHTS[model], lb=lb, ub=ub, Vh=Vh, up=up,
                x0m=x0m, tr=tr, om=lambda: OMODEL[model], solver=lambda: ctx.solver(model, N))


def zoo(zctx, case):
    _, model, N, B = case
    nx, nu = ZDIMS[model]
    zctx.solver(case).close()   # skips when the library is not generated
    if case not in zctx.hats_:
        V = zctx.plan(case)
        om = use(model)
        rows = [shift_plan(om, N, H_SX, V[b]) for b in range(B)]
        Vh, up = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        x0m = Vh[:, :nx] + 1e-2 * np.random.default_rng(SEED + 13 * N + B).standard_normal((B, nx))
        for a in (Vh, up, x0m):
            a.setflags(write=False)
        zctx.hats_[case] = (Vh, up, x0m)
    Vh, up, x0m = zctx.hats_[case]
    lb, ub, _, _ = case_bounds(case)
    return Prob(name=_id(case), nx=nx, nu=nu, N=N, B=B, h=H_SX, w=sx_weights(nx, nu), lb=lb, ub=ub, Vh=Vh, up=up,
                x0m=x0m, tr=zctx.inputs(case)[2], om=lambda: use(model), solver=lambda: zctx.solver(case))


def problem(case, ctx, zctx):
    return builtin(ctx, *case[:3]) if case[0] in DIMS else zoo(zctx, case)


def assert_failed_alone(r, clean, bad, V_given, u0_plan, B):
    """what a failed instance guarantees, and that it fails alone"""
    others = np.arange(B) != bad
    assert r["status"][bad] == 2 and (r["status"][others] == 0).all(), r["status"]
    assert np.array_equal(r["V"][bad], V_given, equal_nan=True), "V of a failed instance is bit for bit as given"
    assert np.array_equal(r["u0"][bad], u0_plan) and np.isinf(r["step_inf"][bad]) and r["step_inf"][bad] > 0
    for k in ("V", "u0", "step_inf", "status"):
        assert np.array_equal(r[k][others], clean[k][others]), f"{k}: the neighbours of a failed instance must not change"


# ---------------------------------------------------------------- A1. the undo log
UNDO = [("two_link_arm", 17, 37, False, 0), ("two_link_arm", 17, 37, True, 0), ("exo_arm", 7, 9, False, 0),
        ("two_link_arm", 4, 130, False, 64)]


@pytest.mark.parametrize("case", UNDO, ids=_id)
def test_overflowing_step_restores_the_plan(case, ctx):
    """Instances used (per case the first candidate with g >= 1.2) and their g, as printed on one MI355X:
    2-link (17, 37): 0, g = 1.6819; clamped at +-2: 0, g = 1.3330; exo (7, 9): 0, g = 1.4137; 2-link (4, 130): 104 (the
    first of 64..129), g = 1.2153."""
    import torch
    model, N, B, clamped, first = case
    p = builtin(ctx, model, N, B, clamped)
    lb, ub = (p.lb, p.ub) if clamped else (None, None)
    m = ctx.m
    bad, g = None, 0.0
    for b in range(first, B):   # the precondition, from the reference alone
        g = overflow_growth(p.om(), N, p.h, p.Vh[b], p.up[b], p.tr[b], p.w, True, lb, ub, clamped)
        if g >= G_MIN:
            bad = b
            break
    assert bad is not None, "no instance of the case grows by 1.2"
    print(f"{_id(case)}: instance {bad}, g = {g:.4f}")
    s = p.solver()
    kw = dict(hessian=m.HESSIAN_EXACT)
    clean = gpu_rti(s, p.Vh, p.up, p.tr, p.w, p.x0m, lb, ub, clamp=(lb, ub) if clamped else None, **kw)
    assert (clean["prep_status"] == 0).all() and (clean["status"] == 0).all(), (clean["prep_status"], clean["status"])
    x2 = p.x0m.copy()
    x2[bad] = BIG
    V = dev(p.Vh)
    pr = s.rti_prepare(B, V, dev(p.up), dev(p.tr), dev(p.w), u_lb=dev(lb), u_ub=dev(ub), **kw)
    cl = dict(u_lb=dev(lb), u_ub=dev(ub))
    f = s.rti_feedback(B, dev(x2), V, pr["workspace"], **cl)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in f.items()}
    assert (pr["prep_status"].cpu().numpy() == 0).all()
    assert_failed_alone(r, clean, bad, p.Vh[bad], p.Vh[bad, p.nx:p.K], B)
    # the records and the restored plan are intact: the same workspace and V tensor, the clean measurement.  The
    # feedback steps V in place, so the rows of the instances that succeeded are put back to V^ first; the failed
    # instance's row stays exactly what the restore loop left
    others = torch.tensor(np.flatnonzero(np.arange(B) != bad), device="cuda")
    V[others] = dev(p.Vh)[others]
    f2 = s.rti_feedback(B, dev(p.x0m), V, pr["workspace"], **cl)
    torch.cuda.synchronize()
    s.close()
    for k in ("V", "u0", "step_inf", "status"):
        assert np.array_equal(f2[k].cpu().numpy(), clean[k]), f"{k}: the second launch against the clean batch"


# ---------------------------------------------------------------- A2. the clamped forward pass
CLAMPED = [("exo_arm", 7, 70, 0), ("exo_arm", 21, 9, 0), ("two_link_arm", 4, 130, 3), ("two_link_arm", 2, 64, 0),
           ("ubound", "cart_pole", 17, 37), ("ubound", "unicycle", 17, 37)]


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("case", CLAMPED, ids=_id)
def test_clamped_forward_pass_on_every_ring(case, hess, ctx, zctx):
    p = builtin(ctx, *case[:3], bounded=True) if case[0] in DIMS else zoo(zctx, case)
    pad = case[3] if case[0] in DIMS else 0
    nx, nu, N, B, K = p.nx, p.nu, p.N, p.B, p.K
    exact = hess == "exact"
    free, _, _ = riccati_rti_step_batch(p.om(), N, p.h, p.Vh, p.up, p.tr, p.w, p.x0m, exact, p.lb, p.ub)
    Uh = p.U(p.Vh)
    tl, tu = tight_box(p.lb, p.ub, Uh, p.U(free))
    om = p.om()
    held = np.stack([held_mask(om, N, p.Vh[b], tl[b], tu[b], 0) for b in range(B)])
    ref, Vn, clamped = riccati_rti_step_batch(om, N, p.h, p.Vh, p.up, p.tr, p.w, p.x0m, exact, tl, tu, clamp=True)
    acts = np.array([clamped[b][~held[b]].any() for b in range(B)])
    print(f"{p.name} {hess}: the clamp acts on {int(acts.sum())} of {B} instances")
    assert acts.any() and not acts.all(), "the clamp must act on at least one instance and not on all"
    s = p.solver()
    tabs = (table(tl, nu + pad), table(tu, nu + pad))
    r = gpu_rti(s, p.Vh, p.up, p.tr, p.w, p.x0m, *tabs, clamp=tabs, bounds_stride=nu + pad, hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["status"] == 0).all() and (r["prep_status"] == 0).all(), (r["status"], r["prep_status"])
    check_outputs(r, p.Vh, p.x0m, nx, nu)
    Un = p.U(r["V"])
    assert ((Un >= tl[:, None, :]) & (Un <= tu[:, None, :])).all(), "every returned control inside its own box bit for bit"
    assert np.array_equal(Un[held], Uh[held])
    moved = (Un == tl[:, None, :]) | (Un == tu[:, None, :])
    assert (moved & ~held).any(), "the GPU's clamp acted"
    check(r["V"], Vn, f"A2 {p.name} {hess}: V_out")
    check(r["V"] - p.Vh, ref, f"A2 {p.name} {hess}: dV")
    dV = r["V"] - p.Vh
    for b in range(B):   # the linearised dynamics with the clamped du
        for k in range(N):
            Ac, Bc, xd = _jac(om, p.Vh[b, k * K:k * K + nx], p.Vh[b, k * K + nx:(k + 1) * K])
            c = p.Vh[b, k * K:k * K + nx] + p.h * xd - p.Vh[b, (k + 1) * K:(k + 1) * K + nx]
            want = (np.eye(nx) + p.h * Ac) @ dV[b, k * K:k * K + nx] + p.h * Bc @ dV[b, k * K + nx:(k + 1) * K] + c
            assert np.abs(dV[b, (k + 1) * K:(k + 1) * K + nx] - want).max() <= TOL * max(1.0, np.abs(want).max()), (b, k)


# ---------------------------------------------------------------- A3. ring depth and the zoo
PARITY = ([("free", "cart_pole", N, B) for (N, B) in [(1, 5), (2, 3), (3, 9), (33, 65), (4, 5), (6, 5), (7, 5)]]
          + [("free", model, N, B) for model in ("motor_pendulum", "unicycle") for (N, B) in [(1, 5), (3, 9), (17, 37)]]
          + [("free", "mass_chain", 1, 5), ("free", "mass_chain", 5, 9), ("two_link_arm", 4, 5), ("two_link_arm", 5, 5)])


@pytest.mark.parametrize("case", PARITY, ids=_id)
def test_step_matches_the_dense_reference_on_every_ring(case, ctx, zctx):
    p = problem(case, ctx, zctx)
    N, B = p.N, p.B
    ratio = np.array([exact_qp_ratio(p.om(), N, p.h, p.Vh[b], p.up[b], p.tr[b], p.w) for b in range(B)])
    print(f"{p.name}: exact M_uu eigenvalue ratio {ratio.min():.3e} .. {ratio.max():.3e}")
    assert (np.abs(ratio) > 1e-9).all(), "status 0 or 1 must not hang on rounding"
    s = p.solver()
    for hess in ("exact", "gn"):
        r = gpu_rti(s, p.Vh, p.up, p.tr, p.w, p.x0m, hessian=hess_id(ctx.m, hess))
        ex = (ratio > 0) & (hess == "exact")   # the instances the exact reference judges
        want = np.where((hess == "exact") & ~ex, 1, 0)
        assert np.array_equal(r["prep_status"], want) and np.array_equal(r["status"], want), (r["prep_status"], want)
        check_outputs(r, p.Vh, p.x0m, p.nx, p.nu)
        ref = np.stack([dense_rti_step(p.om(), N, p.h, p.Vh[b], p.up[b], p.tr[b], p.w, p.x0m[b], bool(ex[b]))
                        for b in range(B)])
        assert np.abs(ref).max() > 1e-3, "the shifted plan is no solution"
        check(r["V"] - p.Vh, ref, f"A3 {p.name} {hess}")
    s.close()


@pytest.mark.parametrize("n", [1, 5])
def test_mass_chain_shift(n, zctx):
    case = ("free", "mass_chain", 5, 9)
    _, model, N, B = case
    nx, nu = ZDIMS[model]
    s = zctx.solver(case)
    V = zctx.plan(case)
    got, up = gpu_shift(s, V, n)
    s.close()
    ref, up_ref = shift_reference(use(model), N, H_SX, V, n)
    check_shift(got, up, V, ref, up_ref, nx, nu, N, n, f"mass_chain-5-9-{n}")


# ---------------------------------------------------------------- A4. isolation on the D = 1 and scratch kernels
@pytest.mark.parametrize("where", ["plan", "x0_meas"])
@pytest.mark.parametrize("case", [("exo_arm", 7, 70, 66), ("free", "mass_chain", 5, 9, 5)], ids=_id)
def test_nan_instance_fails_alone_on_the_deep_records(case, where, ctx, zctx):
    bad = case[-1]
    p = builtin(ctx, *case[:3], bounded=True) if case[0] in DIMS else zoo(zctx, case[:4])
    clamp = (p.lb, p.ub) if p.lb is not None else None
    s = p.solver()
    clean = gpu_rti(s, p.Vh, p.up, p.tr, p.w, p.x0m, p.lb, p.ub, clamp=clamp)
    assert (clean["status"] == 0).all() and (clean["prep_status"] == 0).all()
    V2, x2 = p.Vh.copy(), p.x0m.copy()
    if where == "plan":
        V2[bad, 3 * p.K + 1] = np.nan
    else:
        x2[bad, 2] = np.nan
    r = gpu_rti(s, V2, p.up, p.tr, p.w, x2, p.lb, p.ub, clamp=clamp)
    s.close()
    others = np.arange(p.B) != bad
    assert r["prep_status"][bad] == (2 if where == "plan" else 0) and (r["prep_status"][others] == 0).all()
    assert_failed_alone(r, clean, bad, V2[bad], p.Vh[bad, p.nx:p.K], p.B)
