"""GPU: real-time iteration, a prepare launch and a feedback launch per tick (mmpc_rti_prepare_batch /
mmpc_rti_feedback_batch).

Inputs, shapes and fixtures are those of tests/test_gpu_feedback_gains.py.  The linearisation point is NOT a solution:
it is the GPU plan shifted by one stage (rti_reference.shift_plan: the last control repeated, x_N = F(x_N, u_{N-1});
u_prev the old u_0), and x0_meas = x^_0 + 1e-2 times a standard normal from default_rng(SEED + 13 N + B).  The
references are tests/rti_reference.py: dense_rti_step (one dense KKT solve with the objective's own gradient) where no
clamp acts, riccati_rti_step where one does.  Every comparison is per instance at 1e-10 max(1, max |ref|).

1. parity, both Hessians, every shape: V_out - V^ against dense_rti_step; prep_status and status 0; V_out[:, :nx] bit
   for bit x0_meas, u0 bit for bit V_out's u_0, step_inf equal to max |V_out - V^| recomputed from the arrays.
2. control bounds without clamping (the bounds reach the preparation alone): the BOUNDED cases, shared and as a padded
   table with NaN in the padding; dV exactly 0 on held controls, the rest matches.
3. the clamped forward pass: a per-instance box around the plan's own controls, half the largest free step wide: some
   free controls are clamped and not all, every returned control is inside the box bit for bit, V_out matches
   riccati_rti_step(clamp=True), the new states satisfy the linearised dynamics with the clamped du.
4. pins: n_pin = 2 at (17, 37): u_0 and u_1 unchanged bit for bit.
5. agreement with the JVP at a solution (16-lane solves at 1e-11 / 1e-12): the step with dx0 minus solve_jvp's dV for
   dx0 alone is the step at dx0 = 0 -- the step V*'s own residual produces -- which is computed in the same run.
6. fallback: the indefinite-exact instance of tests/test_gpu_solve_vjp.py: status 1 with the Gauss-Newton reference, the
   instance beside it 0 with the exact one.
7. non-finite input, three runs: NaN in V^ (decided by the preparation), NaN in x0_meas (decided by the feedback), NaN
   in the padding of a strided bounds table (no effect).  A failed instance has status 2, V bit for bit as given, u0
   the plan's own, step_inf inf; its wave- and workgroup-mates are bit for bit the clean batch's.
8. Newton iteration, 2-link (17, 5): prepare + feedback iterated at fixed data from V* at x0 + delta, |delta|_inf =
   1e-2; after N_STAR + 1 steps |V - V*_new|_inf against the GPU's own tight re-solve is within 10 ERR_REACHED, the
   two numbers tests/test_rti_reference.py measured on the CPU (3 steps, 6.8e-12).
9. a loop of 5 ticks, shift -> prepare -> plant step with a disturbance -> feedback, the shift done in torch: each
   tick's step against the dense reference at the GPU's own V^ of that tick; a captured graph of one (feedback, shift,
   prepare) tick replays the direct calls bit for bit.
10. the host entry, B = 1, determinism run to run, u0 / status in mmpc_host_alloc memory.
11. a generated model (cart_pole: nu = 1, odd K = 5) at (17, 37) through its own library."""
import numpy as np
import pytest

from rti_reference import dense_rti_step, dense_rti_step_batch, plant_step, riccati_rti_step_batch, shift_plan
from sens_reference import _jac, held_mask
from test_gpu_feedback_gains import BOUNDED, DIMS, H, OMODEL, SEED, SHAPES, W_2L, WEIGHTS, Ctx, _id, dev, hess_id
from test_rti_reference import DELTA, ERR_REACHED, N_STAR

pytestmark = pytest.mark.gpu

TOL = 1e-10
PARITY = [(model, N, B, hess) for model, shapes in SHAPES.items() for (N, B) in shapes for hess in ("exact", "gn")]


def shift_batch(om, N, V):
    rows = [shift_plan(om, N, H, V[b]) for b in range(V.shape[0])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


class RCtx(Ctx):
    """test_gpu_feedback_gains's shared state (inputs, GPU plans) plus the shifted plans and the measured states"""

    def __init__(self, m, d):
        super().__init__(m, d)
        self.hats_ = {}

    def hat(self, model, N, B, bounded=False):
        """(V^ [B, NV], u_prev [B, nu], x0_meas [B, nx])"""
        key = (model, N, B, bounded)
        if key not in self.hats_:
            nx, _ = DIMS[model]
            Vh, up = shift_batch(OMODEL[model], N, self.plan(model, N, B, bounded))
            x0m = Vh[:, :nx] + 1e-2 * np.random.default_rng(SEED + 13 * N + B).standard_normal((B, nx))
            for a in (Vh, up, x0m):
                a.setflags(write=False)
            self.hats_[key] = (Vh, up, x0m)
        return self.hats_[key]


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return RCtx(mmpc_mod, str(tmp_path_factory.mktemp("rti")))


def gpu_rti(s, Vh, up, tr, w, x0m, lb=None, ub=None, clamp=None, bounds_stride=0, **kw):
    """one prepare and one feedback launch on fresh tensors; lb / ub go to the preparation (the held mask), clamp =
    (lb, ub) to the feedback (None: no clamp).  The outputs as numpy."""
    import torch
    B = Vh.shape[0]
    V = dev(Vh)
    p = s.rti_prepare(B, V, dev(up), dev(tr), dev(w), u_lb=dev(lb), u_ub=dev(ub), bounds_stride=bounds_stride, **kw)
    cl, cu = clamp if clamp else (None, None)
    f = s.rti_feedback(B, dev(x0m), V, p["workspace"], u_lb=dev(cl), u_ub=dev(cu),
                       bounds_stride=bounds_stride if clamp else 0)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in f.items()}
    out["prep_status"] = p["prep_status"].cpu().numpy()
    return out


def check(dV, ref, what=""):
    """per instance: max |dV - ref| <= TOL max(1, max |ref|)"""
    assert dV.shape == ref.shape, (dV.shape, ref.shape)
    err = np.abs(dV - ref).max(axis=1)
    bound = TOL * np.maximum(1.0, np.abs(ref).max(axis=1))
    print(f"{what}: max |dV - ref| = {err.max():.3e}, worst err / bound = {(err / bound).max():.3e}")
    assert np.isfinite(dV).all() and (err <= bound).all(), (what, err.max(), np.argwhere(err > bound)[:5])


def check_outputs(r, Vh, x0m, nx, nu):
    """what every successful step guarantees bit for bit"""
    assert np.array_equal(r["V"][:, :nx], x0m), "V[:, :nx] is x0_meas bit for bit"
    assert np.array_equal(r["u0"], r["V"][:, nx:nx + nu]), "u0 is V's u_0 bit for bit"
    assert np.array_equal(r["step_inf"], np.abs(r["V"] - Vh).max(axis=1)), "step_inf from the arrays as stored"


def controls(model, N, V):
    """[B, N, nu] view of the control entries of V"""
    nx, nu = DIMS[model]
    return V[:, :-nx].reshape(V.shape[0], N, nx + nu)[:, :, nx:]


def table(rows, stride):
    """[B, nu] rows at a padded stride in a buffer of the exact size, NaN in the padding"""
    B, nu = rows.shape
    t = np.full((B - 1) * stride + nu, np.nan)
    for b in range(B):
        t[b * stride:b * stride + nu] = rows[b]
    return t


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", PARITY, ids=_id)
def test_step_matches_the_dense_reference(case, ctx):
    model, N, B, hess = case
    nx, nu = DIMS[model]
    _, _, tr = ctx.inputs(model, N, B)
    Vh, up, x0m = ctx.hat(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_rti(s, Vh, up, tr, WEIGHTS[model], x0m, hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["prep_status"] == 0).all() and (r["status"] == 0).all(), (r["prep_status"], r["status"])
    check_outputs(r, Vh, x0m, nx, nu)
    ref = dense_rti_step_batch(OMODEL[model], N, H, Vh, up, tr, WEIGHTS[model], x0m, hess == "exact")
    assert np.abs(ref).max() > 1e-3, "the shifted plan is no solution"
    check(r["V"] - Vh, ref, _id(case))


# ---------------------------------------------------------------- 2. control bounds, no clamp
@pytest.mark.parametrize("case", BOUNDED, ids=_id)
def test_held_controls_stay_and_the_rest_matches(case, ctx):
    model, N, B, form = case
    nx, nu = DIMS[model]
    _, _, tr = ctx.inputs(model, N, B)
    Vh, up, x0m = ctx.hat(model, N, B, True)
    lb, ub = ctx.bounds(model, True)
    held = np.stack([held_mask(OMODEL[model], N, Vh[b], lb, ub, 0) for b in range(B)])
    assert held.any() and not held.all(), "the case needs at least one held and one free control"
    s = ctx.solver(model, N)
    for hess in ("exact", "gn"):
        ref, _, _ = riccati_rti_step_batch(OMODEL[model], N, H, Vh, up, tr, WEIGHTS[model], x0m, hess == "exact", lb, ub)
        if form == "shared":
            r = gpu_rti(s, Vh, up, tr, WEIGHTS[model], x0m, lb, ub, hessian=hess_id(ctx.m, hess))
        else:
            r = gpu_rti(s, Vh, up, tr, WEIGHTS[model], x0m, table(np.tile(lb, (B, 1)), nu + 3),
                        table(np.tile(ub, (B, 1)), nu + 3), bounds_stride=nu + 3, hessian=hess_id(ctx.m, hess))
        assert (r["prep_status"] == 0).all() and (r["status"] == 0).all(), (r["prep_status"], r["status"])
        check_outputs(r, Vh, x0m, nx, nu)
        assert np.array_equal(controls(model, N, r["V"])[held], controls(model, N, Vh)[held]), "held controls stay"
        assert (controls(model, N, ref)[held] == 0.0).all()
        check(r["V"] - Vh, ref, f"{_id(case)} {hess}")
    s.close()


# ---------------------------------------------------------------- 3. the clamped forward pass
@pytest.mark.parametrize("hess", ["exact", "gn"])
def test_clamped_forward_pass(hess, ctx):
    model, N, B = "two_link_arm", 17, 37
    om = OMODEL[model]
    nx, nu = DIMS[model]
    K = nx + nu
    _, _, tr = ctx.inputs(model, N, B)
    Vh, up, x0m = ctx.hat(model, N, B, True)
    lb, ub = ctx.bounds(model, True)
    free, _, _ = riccati_rti_step_batch(om, N, H, Vh, up, tr, W_2L, x0m, hess == "exact", lb, ub)
    Uh = controls(model, N, Vh)
    half = 0.5 * np.abs(controls(model, N, free)).max(axis=(1, 2))[:, None]
    tl, tu = np.maximum(lb[None, :], Uh.min(1) - half), np.minimum(ub[None, :], Uh.max(1) + half)
    held = np.stack([held_mask(om, N, Vh[b], tl[b], tu[b], 0) for b in range(B)])
    ref, Vn, clamped = riccati_rti_step_batch(om, N, H, Vh, up, tr, W_2L, x0m, hess == "exact", tl, tu, clamp=True)
    acts = np.array([clamped[b][~held[b]].any() for b in range(B)])
    assert acts.any() and not acts.all(), "the clamp must act on at least one instance and not on all"
    s = ctx.solver(model, N)
    r = gpu_rti(s, Vh, up, tr, W_2L, x0m, table(tl, nu), table(tu, nu), clamp=(table(tl, nu), table(tu, nu)),
                bounds_stride=nu, hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["status"] == 0).all(), r["status"]
    check_outputs(r, Vh, x0m, nx, nu)
    Un = controls(model, N, r["V"])
    assert ((Un >= tl[:, None, :]) & (Un <= tu[:, None, :])).all(), "every returned control inside the box bit for bit"
    assert np.array_equal(Un[held], Uh[held])
    moved = (Un == tl[:, None, :]) | (Un == tu[:, None, :])
    assert (moved & ~held).any(), "the GPU's clamp acted"
    check(r["V"], Vn, f"clamped {hess}: V_out")
    check(r["V"] - Vh, ref, f"clamped {hess}: dV")
    dV = r["V"] - Vh
    for b in range(B):   # the linearised dynamics with the clamped du
        for k in range(N):
            Ac, Bc, xd = _jac(om, Vh[b, k * K:k * K + nx], Vh[b, k * K + nx:(k + 1) * K])
            c = Vh[b, k * K:k * K + nx] + H * xd - Vh[b, (k + 1) * K:(k + 1) * K + nx]
            want = (np.eye(nx) + H * Ac) @ dV[b, k * K:k * K + nx] + H * Bc @ dV[b, k * K + nx:(k + 1) * K] + c
            assert np.abs(dV[b, (k + 1) * K:(k + 1) * K + nx] - want).max() <= TOL * max(1.0, np.abs(want).max()), (b, k)


# ---------------------------------------------------------------- 4. pins
def test_pinned_stages_stay(ctx):
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    _, _, tr = ctx.inputs(model, N, B)
    Vh, up, x0m = ctx.hat(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_rti(s, Vh, up, tr, W_2L, x0m, n_pin=2)
    box = gpu_rti(s, Vh, up, tr, W_2L, x0m, n_pin=2, clamp=(np.full(nu, 1e-3), np.full(nu, 2e-3)))
    s.close()
    assert (r["status"] == 0).all(), r["status"]
    check_outputs(r, Vh, x0m, nx, nu)
    U, Uh = controls(model, N, r["V"]), controls(model, N, Vh)
    assert np.array_equal(U[:, :2], Uh[:, :2]) and np.abs(U[:, 2:] - Uh[:, 2:]).max() > 1e-3
    check(r["V"] - Vh, dense_rti_step_batch(OMODEL[model], N, H, Vh, up, tr, W_2L, x0m, True, n_pin=2), "pins")
    Ub = controls(model, N, box["V"])   # a pinned control keeps its value whatever the box, the others are inside it
    assert np.array_equal(Ub[:, :2], Uh[:, :2]) and ((Ub[:, 2:] >= 1e-3) & (Ub[:, 2:] <= 2e-3)).all()


# ---------------------------------------------------------------- 5. agreement with the JVP at a solution
def test_step_at_a_solution_is_the_jvp_plus_the_residuals_step(ctx):
    import torch
    model, N, B = "two_link_arm", 17, 5
    nx, nu = DIMS[model]
    m = ctx.m
    x0, up, tr = ctx.inputs(model, N, B)
    s = ctx.solver(model, N, kkt_solver=m.KKT_RICCATI_GROUP, tol_grad=1e-11, tol_defect=1e-12)
    g = s.solve_batch_host(x0, up, tr, W_2L)
    assert (g["status"] == 0).all()
    V = g["V"]
    dx0 = 1e-2 * np.random.default_rng(SEED + 13 * N + B).standard_normal((B, nx))
    r = gpu_rti(s, V, up, tr, W_2L, V[:, :nx] + dx0, hessian=m.HESSIAN_EXACT)
    r0 = gpu_rti(s, V, up, tr, W_2L, V[:, :nx], hessian=m.HESSIAN_EXACT)
    j = s.solve_jvp(B, dev(V), dev(up), dev(tr), dev(W_2L), dx0=dev(dx0), hessian=m.HESSIAN_EXACT)
    torch.cuda.synchronize()
    s.close()
    jv = j["dV"].cpu().numpy()
    assert (r["status"] == 0).all() and (r0["status"] == 0).all() and (j["jvp_status"].cpu().numpy() == 0).all()
    # V[:, :nx] + dx0 - V[:, :nx] is dx0 up to one rounding, which the tolerance covers
    gap = np.abs((r["V"] - V) - jv).max(axis=1)
    bound = r0["step_inf"] + TOL * np.maximum(1.0, np.abs(jv).max(axis=1))
    print(f"|rti - jvp| = {gap}, the step of V*'s own residual = {r0['step_inf']}")
    assert np.abs(jv).max() > 1e-3 and (r0["step_inf"] <= 1e-8).all() and (gap <= bound).all(), (gap, bound)


# ---------------------------------------------------------------- 6. fallback
def test_indefinite_exact_model_falls_back_to_gauss_newton(ctx):
    model, N, B = "two_link_arm", 17, 2
    om = OMODEL[model]
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    nx, _ = DIMS[model]
    x0m = V[:, :nx] + 1e-2 * np.random.default_rng(SEED + 13 * N + B).standard_normal((B, nx))
    tr2 = tr.copy()   # V is no solution for these targets: velocity targets of instance 0 moved by 1000 (1, -1)
    tr2[0, :, 2] += 1000.0
    tr2[0, :, 3] -= 1000.0
    s = ctx.solver(model, N)
    r = gpu_rti(s, V, up, tr2, W_2L, x0m, hessian=ctx.m.HESSIAN_EXACT)
    s.close()
    assert r["prep_status"].tolist() == [1, 0] and r["status"].tolist() == [1, 0], (r["prep_status"], r["status"])
    check((r["V"] - V)[:1], dense_rti_step_batch(om, N, H, V[:1], up[:1], tr2[:1], W_2L, x0m[:1], False), "fallback")
    check((r["V"] - V)[1:], dense_rti_step_batch(om, N, H, V[1:], up[1:], tr2[1:], W_2L, x0m[1:], True), "neighbour")


# ---------------------------------------------------------------- 7. non-finite input
@pytest.mark.parametrize("where", ["plan", "x0_meas", "padding"])
def test_nan_instance_fails_alone(where, ctx):
    model, N, B, bad = "two_link_arm", 17, 37, 5
    nx, nu = DIMS[model]
    _, _, tr = ctx.inputs(model, N, B)
    Vh, up, x0m = ctx.hat(model, N, B, True)
    lb, ub = ctx.bounds(model, True)
    stride = nu + 3
    tl, tu = table(np.tile(lb, (B, 1)), stride), table(np.tile(ub, (B, 1)), stride)
    s = ctx.solver(model, N)
    clean = gpu_rti(s, Vh, up, tr, W_2L, x0m, lb, ub, clamp=(lb, ub))
    assert (clean["status"] == 0).all()
    V2, x2 = Vh.copy(), x0m.copy()
    if where == "plan":
        V2[bad, 3 * 6 + 1] = np.nan
    elif where == "x0_meas":
        x2[bad, 2] = np.nan
    if where == "padding":
        r = gpu_rti(s, Vh, up, tr, W_2L, x0m, tl, tu, clamp=(tl, tu), bounds_stride=stride)
    else:
        r = gpu_rti(s, V2, up, tr, W_2L, x2, lb, ub, clamp=(lb, ub))
    s.close()
    if where == "padding":
        for k in ("V", "u0", "step_inf", "status", "prep_status"):
            assert np.array_equal(r[k], clean[k]), k
        return
    others = np.arange(B) != bad
    assert r["prep_status"][bad] == (2 if where == "plan" else 0) and (r["prep_status"][others] == 0).all()
    assert r["status"][bad] == 2 and (r["status"][others] == 0).all(), r["status"]
    assert np.array_equal(r["V"][bad], V2[bad], equal_nan=True), "V of a failed instance is bit for bit as given"
    assert np.array_equal(r["u0"][bad], Vh[bad, nx:nx + nu]) and np.isinf(r["step_inf"][bad])
    for k in ("V", "u0", "step_inf"):
        assert np.array_equal(r[k][others], clean[k][others]), f"{k}: the neighbours of a failed instance must not change"


# ---------------------------------------------------------------- 8. Newton iteration
def test_iterated_step_reaches_the_resolve(ctx):
    model, N, B = "two_link_arm", 17, 5
    nx, nu = DIMS[model]
    m = ctx.m
    x0, up, tr = ctx.inputs(model, N, B)
    rn = np.random.default_rng(SEED + 7 * N + B).standard_normal((B, nx))
    x1 = x0 + DELTA * rn / np.abs(rn).max(axis=1, keepdims=True)
    s = ctx.solver(model, N, kkt_solver=m.KKT_RICCATI_GROUP, tol_grad=1e-11, tol_defect=1e-12)
    g = s.solve_batch_host(x0, up, tr, W_2L)
    g2 = s.solve_batch_host(x1, up, tr, W_2L, V=g["V"])
    assert (g["status"] == 0).all() and (g2["status"] == 0).all()
    V = g["V"]
    errs = [np.abs(V - g2["V"]).max(axis=1)]
    for _ in range(N_STAR + 1):
        r = gpu_rti(s, V, up, tr, W_2L, x1, hessian=m.HESSIAN_EXACT)
        assert (r["status"] == 0).all(), r["status"]
        V = r["V"]
        errs.append(np.abs(V - g2["V"]).max(axis=1))
    s.close()
    for b in range(B):
        print(f"instance {b}: " + " ".join(f"{e[b]:.2e}" for e in errs))
    assert (errs[-1] <= 10.0 * ERR_REACHED).all(), (errs[-1], 10.0 * ERR_REACHED)


# ---------------------------------------------------------------- 9. a loop
def torch_shift(s, V, tmp, xdot, up, u0, nx, nu, N, stream=None):
    """V (holding the plan after a feedback) becomes the shifted plan, up the control just applied: all on `stream`"""
    K = nx + nu
    NV = V.shape[1]
    tmp.copy_(V)
    xN, uL = tmp[:, N * K:].contiguous(), tmp[:, (N - 1) * K + nx:N * K].contiguous()
    s.linearize(V.shape[0], xN, uL, None, None, xdot, stream=stream)
    V[:, :NV - K].copy_(tmp[:, K:])
    V[:, NV - K:NV - nx].copy_(uL)
    V[:, NV - nx:].copy_(xN + H * xdot)
    up.copy_(u0)


def test_five_ticks_and_a_captured_tick(ctx):
    import torch
    model, N, B = "two_link_arm", 17, 5
    om = OMODEL[model]
    nx, nu = DIMS[model]
    x0, up0, tr = ctx.inputs(model, N, B)
    rng = np.random.default_rng(SEED + 17 * N + B)
    s = ctx.solver(model, N)
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    V, tmp, xdot, up, xm = dev(ctx.plan(model, N, B)), f64(B, s.NV), f64(B, nx), dev(up0), f64(B, nx)
    dtr, dw = dev(tr), dev(W_2L)
    out = dict(u0=f64(B, nu), step_inf=f64(B), status=torch.full((B,), -1, dtype=torch.int32, device="cuda"))
    out["u0"].copy_(V[:, nx:nx + nu])
    ws = f64(s.rti_workspace_bytes(B) // 8)
    pst = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    x = V[:, :nx].cpu().numpy()
    for tick in range(5):
        u_applied = out["u0"].cpu().numpy()
        torch_shift(s, V, tmp, xdot, up, out["u0"], nx, nu, N)
        s.rti_prepare(B, V, up, dtr, dw, workspace=ws, prep_status=pst)
        torch.cuda.synchronize()
        Vh, uph = V.cpu().numpy(), up.cpu().numpy()
        x = np.stack([plant_step(om, H, x[b], u_applied[b]) for b in range(B)]) + 1e-3 * rng.standard_normal((B, nx))
        xm.copy_(dev(x))
        s.rti_feedback(B, xm, V, ws, **out)
        torch.cuda.synchronize()
        Vn = V.cpu().numpy()
        assert (pst.cpu().numpy() == 0).all() and (out["status"].cpu().numpy() == 0).all()
        assert np.array_equal(Vn[:, :nx], x) and np.array_equal(out["u0"].cpu().numpy(), Vn[:, nx:nx + nu])
        check(Vn - Vh, dense_rti_step_batch(om, N, H, Vh, uph, tr, W_2L, x, True), f"tick {tick}")
    # one (feedback, shift, prepare) tick: the direct calls, then the same from a captured graph on the same start
    s.rti_prepare(B, V, up, dtr, dw, workspace=ws, prep_status=pst)
    start = (V.clone(), up.clone(), ws.clone())

    def one_tick(stream=None):
        s.rti_feedback(B, xm, V, ws, stream=stream, **out)
        torch_shift(s, V, tmp, xdot, up, out["u0"], nx, nu, N, stream=stream)
        s.rti_prepare(B, V, up, dtr, dw, workspace=ws, prep_status=pst, stream=stream)

    one_tick()
    torch.cuda.synchronize()
    want = [t.clone() for t in (V, up, ws, out["u0"], out["step_inf"], out["status"], pst)]
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        one_tick(cs.cuda_stream)
    for t, v in zip((V, up, ws), start):   # the graph reads the live buffers
        t.copy_(v)
    for t in (out["u0"], out["step_inf"]):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for name, t, w in zip(("V", "u_prev", "workspace", "u0", "step_inf", "status", "prep_status"),
                          (V, up, ws, out["u0"], out["step_inf"], out["status"], pst), want):
        assert torch.equal(t, w), f"{name}: the replayed tick against the direct calls"
    s.close()


# ---------------------------------------------------------------- 10. remaining paths
def test_host_entry_single_instance_host_memory_and_determinism(ctx):
    import torch
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    _, _, tr = ctx.inputs(model, N, B)
    Vh, up, x0m = ctx.hat(model, N, B, True)
    lb, ub = ctx.bounds(model, True)
    s = ctx.solver(model, N)
    r = gpu_rti(s, Vh, up, tr, W_2L, x0m, lb, ub, clamp=(lb, ub))
    again = gpu_rti(s, Vh, up, tr, W_2L, x0m, lb, ub, clamp=(lb, ub))
    host = s.rti_step_host(Vh, x0m, up, tr, W_2L, u_lb=lb, u_ub=ub)
    for k in ("V", "u0", "step_inf", "status"):
        assert np.array_equal(r[k], again[k]), f"{k}: run to run"
        assert np.array_equal(r[k], host[k]), f"{k}: host entry against the device entries"
    one = s.rti_step_host(Vh[3:4], x0m[3:4], up[3:4], tr[3:4], W_2L, u_lb=lb, u_ub=ub)
    assert one["status"].tolist() == [0]
    for k in ("V", "u0", "step_inf"):
        assert np.array_equal(one[k], r[k][3:4]), f"{k}: B = 1"
    # u0, step_inf and status straight into mmpc_host_alloc memory
    hb = ctx.m.HostBuffer(B * nu * 8 + B * 8 + B * 4)
    V = dev(Vh)
    p = s.rti_prepare(B, V, dev(up), dev(tr), dev(W_2L), u_lb=dev(lb), u_ub=dev(ub))
    s.rti_feedback(B, dev(x0m), V, p["workspace"], u0=hb.ptr, step_inf=hb.ptr + B * nu * 8,
                   status=hb.ptr + B * nu * 8 + B * 8, u_lb=dev(lb), u_ub=dev(ub))
    torch.cuda.synchronize()
    assert np.array_equal(hb.view(0, np.float64, B * nu).reshape(B, nu), r["u0"])
    assert np.array_equal(hb.view(B * nu * 8, np.float64, B), r["step_inf"])
    assert np.array_equal(hb.view(B * nu * 8 + B * 8, np.int32, B), r["status"])
    assert np.array_equal(V.cpu().numpy(), r["V"])
    hb.close()
    s.close()


# ---------------------------------------------------------------- 11. a generated model
def test_generated_model_matches_the_dense_reference(mmpc_mod, tmp_path_factory):
    from test_gpu_sx_models import weights as sx_weights
    from test_gpu_sx_sensitivity import Ctx as SxCtx
    from test_user_model_sens_reference import H as H_SX
    from test_user_model_sens_reference import use
    case = ("free", "cart_pole", 17, 37)
    _, model, N, B = case
    nx, nu = 4, 1
    x = SxCtx(mmpc_mod, str(tmp_path_factory.mktemp("rti_sx")))
    s = x.solver(case)   # skips when the library is not generated
    assert (s.nx, s.nu) == (nx, nu)
    _, _, tr, _ = x.inputs(case)
    V, w = x.plan(case), sx_weights(nx, nu)
    om = use(model)
    rows = [shift_plan(om, N, H_SX, V[b]) for b in range(B)]
    Vh, up = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    x0m = Vh[:, :nx] + 1e-2 * np.random.default_rng(SEED + 13 * N + B).standard_normal((B, nx))
    for hess in ("exact", "gn"):
        r = gpu_rti(s, Vh, up, tr, w, x0m, hessian=hess_id(mmpc_mod, hess))
        assert (r["prep_status"] == 0).all() and (r["status"] == 0).all()
        check_outputs(r, Vh, x0m, nx, nu)
        om = use(model)   # the oracle has one USER slot: before every reference
        ref = np.stack([dense_rti_step(om, N, H_SX, Vh[b], up[b], tr[b], w, x0m[b], hess == "exact") for b in range(B)])
        assert np.abs(ref).max() > 1e-3
        check(r["V"] - Vh, ref, f"cart_pole {hess}")
    s.close()
