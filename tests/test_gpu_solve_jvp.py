"""GPU: the forward-mode product of the solve, dV = (d V* / d theta) d theta (mmpc_solve_jvp_batch).

V* comes from the GPU solve, the tangents (dx0, du_prev, dtraj, dweights) are standard normal from a fixed seed
(jvp_reference.tangents with default_rng(SEED + 11 N + B)), the reference is the dense KKT solve of
tests/jvp_reference.py (dense_jvp), not a second Riccati recursion.  Inputs, shapes and fixtures are those of
tests/test_gpu_feedback_gains.py.  Every comparison with the reference is per instance at 1e-10 max(1, max |ref|), the
project's standing GPU-versus-reference tolerance.

1. parity, both Hessians: 2-link (N, B) = (1, 5) (2, 3) (3, 9) (17, 37) (33, 65) and the exo (1, 5) (7, 9) (21, 9) --
   N = 1 has no recursion, 5 and 37 leave a partial wave, 65 makes a second workgroup of one lane; jvp_status 0
   everywhere, du0 bit for bit the u_0 entries of dV, the x_0 entries of dV bit for bit dx0.
2. control bounds: the BOUNDED cases (shared and as a padded table): dV exactly 0 on held controls.
3. pins: n_pin = 2 at (17, 37): du_0 and du_1 exactly 0, the rest matches the reference, and du_prev has no effect on a
   bit of the result.
4. the adjoint identity against the GPU's own solve_vjp on the same plans, per instance:
   |<V_bar, dV> - sum <theta_bar, d theta>| <= 1e-10 max(1, sum |V_bar o dV| + sum |theta_bar o d theta|) -- each
   side's entries are within 1e-10 max(1, |ref|) of one symmetric system's two solutions.
5. forward-free mode: du0 bit for bit the full call's, with a NULL workspace, both Hessians.
6. each tangent alone with the others NULL equals the call with explicit zeros bit for bit; the four single-tangent
   results add up to the joint call at the tolerance.
7. per-instance weights with a padded stride and NaN in the padding, at (17, 37).
8. the solver's own map: 2-link (17, 5), 16-lane solves with tol_grad 1e-11 and tol_defect 1e-12; V* + t dV against
   warm-started re-solves at theta + t d theta, t = 2e-3, 1e-3, 5e-4, dweights scaled to the weights' own sizes
   (relative_weight_tangent of the CPU module): the error's ratio per halving in [3, 5], and at t = 1e-3 the error at
   most 1e-2 of what the unchanged plan is off by.
9. fallback: the indefinite-exact instance of tests/test_gpu_solve_vjp.py item 7: jvp_status 1 with the Gauss-Newton
   reference, the instance beside it 0 with the exact one; forward-free agrees.
10. non-finite input: a NaN in V gives status 2 and zero rows; wave- and workgroup-mates bit for bit the clean batch's.
11. the host entry, B = 1, a captured-graph replay bit for bit the direct call, determinism run to run.
12. a state-bounded handle under the sensitivity barrier at cap 1e6 against xb_dense_jvp: 2-link (3, 9) (17, 37) `box`,
    exo (7, 9) `box`, both Hessians.
13. autograd: torch.autograd.forward_ad and torch.func.jvp through DifferentiableSolver equal a direct solve_jvp bit
    for bit (a shared weights tangent is every row's), and .backward() in the same process still equals solve_vjp.
14. a generated model (cart_pole: nu = 1, odd K = 5) at (17, 37) through the identity of 4 against its library's VJP."""
import numpy as np
import pytest

from jvp_reference import dense_jvp_batch, tangents, xb_dense_jvp_batch
from sens_reference import held_mask
from test_gpu_feedback_gains import BOUNDED, DIMS, H, OMODEL, SEED, SHAPES, W_2L, WEIGHTS, _id, dev, hess_id
from test_gpu_solve_vjp import VCtx, gpu_vjp
from test_solve_jvp_reference import STEPS, relative_weight_tangent

pytestmark = pytest.mark.gpu

TOL = 1e-10
PARITY = [(model, N, B, hess) for model, shapes in SHAPES.items() for (N, B) in shapes for hess in ("exact", "gn")]
NAMES = ("dx0", "du_prev", "dtraj", "dweights")
BARS = ("x0_bar", "u_prev_bar", "traj_bar", "weights_bar")


class JCtx(VCtx):
    """test_gpu_solve_vjp's shared state (inputs, GPU plans, V_bar) plus the tangents and the dense JVP references"""

    def __init__(self, m, d):
        super().__init__(m, d)
        self.tans_, self.jrefs_ = {}, {}

    def tan(self, model, N, B):
        key = (model, N, B)
        if key not in self.tans_:
            t = tangents(OMODEL[model], N, np.random.default_rng(SEED + 11 * N + B), B)
            for a in t:
                a.setflags(write=False)
            self.tans_[key] = t
        return self.tans_[key]

    def jref(self, model, N, B, exact, bounded=False, n_pin=0):
        key = (model, N, B, exact, bounded, n_pin)
        if key not in self.jrefs_:
            _, up, tr = self.inputs(model, N, B)
            lb, ub = self.bounds(model, bounded)
            r = dense_jvp_batch(OMODEL[model], N, H, self.plan(model, N, B, bounded), up, tr, WEIGHTS[model],
                                *self.tan(model, N, B), exact, lb, ub, n_pin)
            r.setflags(write=False)
            self.jrefs_[key] = r
        return self.jrefs_[key]


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return JCtx(mmpc_mod, str(tmp_path_factory.mktemp("solve_jvp")))


def gpu_jvp(s, V, up, tr, w, t, lb=None, ub=None, **kw):
    """one device-pointer JVP call on fresh tensors, t = (dx0, du_prev, dtraj, dweights) with None for a NULL tangent:
    the outputs as numpy"""
    import torch
    r = s.solve_jvp(V.shape[0], dev(V), dev(up), dev(tr), dev(w), *(dev(a) for a in t), u_lb=dev(lb), u_ub=dev(ub), **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def check(dV, ref, what=""):
    """per instance: max |dV - ref| <= TOL max(1, max |ref|)"""
    assert dV.shape == ref.shape, (dV.shape, ref.shape)
    err = np.abs(dV - ref).max(axis=1)
    bound = TOL * np.maximum(1.0, np.abs(ref).max(axis=1))
    print(f"{what}: max |dV - ref| = {err.max():.3e}, worst err / bound = {(err / bound).max():.3e}")
    assert np.isfinite(dV).all() and (err <= bound).all(), (what, err.max(), np.argwhere(err > bound)[:5])


def controls(model, N, dV):
    """[B, N, nu] view of the control entries of dV"""
    nx, nu = DIMS[model]
    return dV[:, :-nx].reshape(dV.shape[0], N, nx + nu)[:, :, nx:]


def identity_gap(Vbar, dV, bars, t):
    """per instance: |<V_bar, dV> - sum <theta_bar, d theta>| and the sum of the absolute products of both sides"""
    B = Vbar.shape[0]
    lhs = (Vbar * dV).sum(1)
    rhs = sum((bars[k].reshape(B, -1) * d.reshape(B, -1)).sum(1) for k, d in zip(BARS, t))
    scale = np.abs(Vbar * dV).sum(1) + sum(np.abs(bars[k].reshape(B, -1) * d.reshape(B, -1)).sum(1)
                                           for k, d in zip(BARS, t))
    return np.abs(lhs - rhs), scale


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", PARITY, ids=_id)
def test_plan_update_matches_the_dense_reference(case, ctx):
    model, N, B, hess = case
    nx, nu = DIMS[model]
    _, up, tr = ctx.inputs(model, N, B)
    t = ctx.tan(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_jvp(s, ctx.plan(model, N, B), up, tr, WEIGHTS[model], t, hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["jvp_status"] == 0).all(), r["jvp_status"]
    assert np.array_equal(r["du0"], r["dV"][:, nx:nx + nu]) and np.array_equal(r["dV"][:, :nx], t[0])
    check(r["dV"], ctx.jref(model, N, B, hess == "exact"), _id(case))


# ---------------------------------------------------------------- 2. control bounds
@pytest.mark.parametrize("case", BOUNDED, ids=_id)
def test_held_controls_stay_and_the_rest_matches(case, ctx):
    model, N, B, form = case
    nx, nu = DIMS[model]
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B, True)
    lb, ub = ctx.bounds(model, True)
    held = np.stack([held_mask(OMODEL[model], N, V[b], lb, ub, 0) for b in range(B)])
    assert held.any() and not held.all(), "the case needs at least one held and one free control"
    s = ctx.solver(model, N)
    for hess in ("exact", "gn"):
        ref = ctx.jref(model, N, B, hess == "exact", True)
        if form == "shared":
            r = gpu_jvp(s, V, up, tr, WEIGHTS[model], ctx.tan(model, N, B), lb, ub, hessian=hess_id(ctx.m, hess))
        else:   # a row per instance at a padded stride, NaN in the padding, buffers of the exact size
            stride = nu + 3
            tl = np.full((B - 1) * stride + nu, np.nan)
            tu = np.full((B - 1) * stride + nu, np.nan)
            for b in range(B):
                tl[b * stride:b * stride + nu], tu[b * stride:b * stride + nu] = lb, ub
            r = gpu_jvp(s, V, up, tr, WEIGHTS[model], ctx.tan(model, N, B), tl, tu, bounds_stride=stride,
                        hessian=hess_id(ctx.m, hess))
        assert (r["jvp_status"] == 0).all(), r["jvp_status"]
        assert (controls(model, N, r["dV"])[held] == 0.0).all(), "dV must be exactly 0 on a held control"
        assert (controls(model, N, ref)[held] == 0.0).all()
        check(r["dV"], ref, f"{_id(case)} {hess}")
    s.close()


# ---------------------------------------------------------------- 3. pins
def test_pinned_stages_stay(ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    V, t = ctx.plan(model, N, B), ctx.tan(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_jvp(s, V, up, tr, W_2L, t, n_pin=2)
    other = gpu_jvp(s, V, up, tr, W_2L, (t[0], 3.0 - 2.0 * t[1], t[2], t[3]), n_pin=2)
    s.close()
    assert (r["jvp_status"] == 0).all(), r["jvp_status"]
    dU = controls(model, N, r["dV"])
    assert (dU[:, :2] == 0.0).all() and (r["du0"] == 0.0).all() and np.abs(dU[:, 2:]).max() > 1e-3
    assert np.array_equal(other["dV"], r["dV"]), "du_prev acts through u_0 alone, and u_0 is pinned"
    check(r["dV"], ctx.jref(model, N, B, True, n_pin=2), "pins")


# ---------------------------------------------------------------- 4. the adjoint identity
@pytest.mark.parametrize("case", [("two_link_arm", 17, 37, False), ("two_link_arm", 17, 37, True),
                                  ("two_link_arm", 33, 65, False), ("exo_arm", 7, 9, True), ("exo_arm", 21, 9, False)],
                         ids=_id)
def test_adjoint_identity_against_the_gpu_vjp(case, ctx):
    model, N, B, bounded = case
    _, up, tr = ctx.inputs(model, N, B)
    V, t, Vbar = ctx.plan(model, N, B, bounded), ctx.tan(model, N, B), ctx.vbar(model, N, B)
    lb, ub = ctx.bounds(model, bounded)
    s = ctx.solver(model, N)
    for hess in ("exact", "gn"):
        j = gpu_jvp(s, V, up, tr, WEIGHTS[model], t, lb, ub, hessian=hess_id(ctx.m, hess))
        v = gpu_vjp(s, V, up, tr, WEIGHTS[model], Vbar, lb, ub, hessian=hess_id(ctx.m, hess))
        assert (j["jvp_status"] == 0).all() and (v["vjp_status"] == 0).all()
        gap, scale = identity_gap(Vbar, j["dV"], v, t)
        print(f"{_id(case)} {hess}: worst gap / bound = {(gap / (TOL * np.maximum(1.0, scale))).max():.3e}")
        assert (gap <= TOL * np.maximum(1.0, scale)).all(), (hess, gap.max())
    s.close()


# ---------------------------------------------------------------- 5. forward-free mode
@pytest.mark.parametrize("hess", ["exact", "gn"])
def test_forward_free_is_bit_for_bit_the_full_call(hess, ctx):
    for model, N, B, bounded in (("two_link_arm", 17, 37, False), ("two_link_arm", 17, 37, True),
                                 ("exo_arm", 7, 9, False)):
        _, up, tr = ctx.inputs(model, N, B)
        V, t = ctx.plan(model, N, B, bounded), ctx.tan(model, N, B)
        lb, ub = ctx.bounds(model, bounded)
        s = ctx.solver(model, N)
        full = gpu_jvp(s, V, up, tr, WEIGHTS[model], t, lb, ub, hessian=hess_id(ctx.m, hess))
        free = gpu_jvp(s, V, up, tr, WEIGHTS[model], t, lb, ub, hessian=hess_id(ctx.m, hess), forward_free=True)
        s.close()
        assert free["dV"] is None and (full["jvp_status"] == 0).all() and (free["jvp_status"] == 0).all()
        assert np.array_equal(free["du0"], full["du0"]) and np.abs(free["du0"]).max() > 1e-3, (model, bounded)


# ---------------------------------------------------------------- 6. single tangents
@pytest.mark.parametrize("model,N,B", [("two_link_arm", 17, 37), ("exo_arm", 7, 9)])
def test_null_tangents_are_zeros_and_the_map_is_linear(model, N, B, ctx):
    _, up, tr = ctx.inputs(model, N, B)
    V, t = ctx.plan(model, N, B), ctx.tan(model, N, B)
    s = ctx.solver(model, N)
    joint = gpu_jvp(s, V, up, tr, WEIGHTS[model], t)
    total = np.zeros_like(joint["dV"])
    for i, name in enumerate(NAMES):
        alone = gpu_jvp(s, V, up, tr, WEIGHTS[model], tuple(a if j == i else None for j, a in enumerate(t)))
        zeros = gpu_jvp(s, V, up, tr, WEIGHTS[model], tuple(a if j == i else np.zeros_like(a) for j, a in enumerate(t)))
        assert (alone["jvp_status"] == 0).all() and (zeros["jvp_status"] == 0).all()
        assert np.array_equal(alone["dV"], zeros["dV"]) and np.array_equal(alone["du0"], zeros["du0"]), name
        assert np.abs(alone["dV"]).max() > 1e-3, name
        total += alone["dV"]
    s.close()
    check(total, joint["dV"], f"{model}: the sum of the single tangents against the joint call")


# ---------------------------------------------------------------- 7. per-instance weights
def test_per_instance_weights_at_a_padded_stride(ctx):
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    nw = nx + 2 * nu
    _, up, tr = ctx.inputs(model, N, B)
    V, t = ctx.plan(model, N, B), ctx.tan(model, N, B)
    wi = W_2L[None, :] * np.random.default_rng(SEED).uniform(0.5, 2.0, (B, nw))   # V is no solution for these
    stride = nw + 5
    wt = np.full((B - 1) * stride + nw, np.nan)   # NaN in the padding, a buffer of the exact size
    for b in range(B):
        wt[b * stride:b * stride + nw] = wi[b]
    s = ctx.solver(model, N)
    r = gpu_jvp(s, V, up, tr, wt, t, weights_stride=stride)
    s.close()
    assert (r["jvp_status"] == 0).all(), r["jvp_status"]
    check(r["dV"], dense_jvp_batch(OMODEL[model], N, H, V, up, tr, wi, *t, True), "per-instance weights")


# ---------------------------------------------------------------- 8. the solver's own map
def test_first_order_update_follows_the_gpu_resolves(ctx):
    model, N, B = "two_link_arm", 17, 5
    m = ctx.m
    x0, up, tr = ctx.inputs(model, N, B)
    t = ctx.tan(model, N, B)
    dx0, dup, dtr, dw = relative_weight_tangent(t, W_2L)
    s = ctx.solver(model, N, kkt_solver=m.KKT_RICCATI_GROUP, tol_grad=1e-11, tol_defect=1e-12)
    assert s.hessian_for(B) == m.HESSIAN_EXACT
    g = s.solve_batch_host(x0, up, tr, W_2L)
    assert (g["status"] == 0).all()
    V = g["V"]
    r = s.solve_jvp_host(V, up, tr, W_2L, dx0, dup, dtr, dw, hessian=m.HESSIAN_EXACT)
    assert (r["jvp_status"] == 0).all()
    err, off = [], []
    for step in STEPS:
        o = s.solve_batch_host(x0 + step * dx0, up + step * dup, tr + step * dtr, np.tile(W_2L, (B, 1)) + step * dw,
                               V=V)
        assert (o["status"] == 0).all(), (step, o["status"])
        err.append(np.abs(o["V"] - (V + step * r["dV"])).max(axis=1))
        off.append(np.abs(o["V"] - V).max(axis=1))
    s.close()
    err, off = np.array(err), np.array(off)
    ratios = err[:-1] / err[1:]
    for b in range(B):
        print(f"instance {b}: error of V* + t dV at t = {STEPS}: {err[:, b]}, ratios per halving {ratios[:, b]}; the "
              f"unchanged plan is off by {off[:, b]}; update / plan at t = 1e-3: {err[1, b] / off[1, b]:.3e}")
    assert ((ratios >= 3.0) & (ratios <= 5.0)).all(), ratios
    assert (err[1] <= 1e-2 * off[1]).all(), (err[1], off[1])


# ---------------------------------------------------------------- 9. fallback
def test_indefinite_exact_model_falls_back_to_gauss_newton(ctx):
    model, N, B = "two_link_arm", 17, 2
    om = OMODEL[model]
    _, up, tr = ctx.inputs(model, N, B)
    V, t = ctx.plan(model, N, B), ctx.tan(model, N, B)
    tr2 = tr.copy()   # V is no solution for these targets: velocity targets of instance 0 moved by 1000 (1, -1)
    tr2[0, :, 2] += 1000.0
    tr2[0, :, 3] -= 1000.0
    s = ctx.solver(model, N)
    r = gpu_jvp(s, V, up, tr2, W_2L, t, hessian=ctx.m.HESSIAN_EXACT)
    f = gpu_jvp(s, V, up, tr2, W_2L, t, hessian=ctx.m.HESSIAN_EXACT, forward_free=True)
    s.close()
    assert r["jvp_status"].tolist() == [1, 0] and f["jvp_status"].tolist() == [1, 0], (r["jvp_status"], f["jvp_status"])
    assert np.array_equal(f["du0"], r["du0"])
    one = lambda b: tuple(a[b:b + 1] for a in t)  # noqa: E731
    check(r["dV"][:1], dense_jvp_batch(om, N, H, V[:1], up[:1], tr2[:1], W_2L, *one(0), False), "fallback instance")
    check(r["dV"][1:], dense_jvp_batch(om, N, H, V[1:], up[1:], tr2[1:], W_2L, *one(1), True), "its neighbour")


# ---------------------------------------------------------------- 10. non-finite input
@pytest.mark.parametrize("where", ["state", "x_N"])
def test_nan_instance_fails_alone(where, ctx):
    model, N, B, bad = "two_link_arm", 17, 37, 5
    _, up, tr = ctx.inputs(model, N, B)
    V, t = ctx.plan(model, N, B), ctx.tan(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_jvp(s, V, up, tr, W_2L, t)
    V2 = V.copy()
    V2[bad, 3 * 6 + 1 if where == "state" else V.shape[1] - 1] = np.nan
    r2 = gpu_jvp(s, V2, up, tr, W_2L, t)
    f2 = gpu_jvp(s, V2, up, tr, W_2L, t, forward_free=True)
    s.close()
    others = np.arange(B) != bad
    assert (r["jvp_status"] == 0).all()
    for got in (r2, f2):
        assert got["jvp_status"][bad] == 2 and (got["jvp_status"][others] == 0).all(), got["jvp_status"]
        assert (got["du0"][bad] == 0.0).all() and np.array_equal(got["du0"][others], r["du0"][others])
    assert (r2["dV"][bad] == 0.0).all()
    assert np.array_equal(r2["dV"][others], r["dV"][others]), "the neighbours of a failed instance must not change"


# ---------------------------------------------------------------- 11. remaining paths
def test_host_entry_single_instance_and_determinism(ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    V, t = ctx.plan(model, N, B), ctx.tan(model, N, B)
    ref = ctx.jref(model, N, B, True)
    s = ctx.solver(model, N)
    r = gpu_jvp(s, V, up, tr, W_2L, t)
    again = gpu_jvp(s, V, up, tr, W_2L, t)
    host = s.solve_jvp_host(V, up, tr, W_2L, *t)
    hfree = s.solve_jvp_host(V, up, tr, W_2L, *t, forward_free=True)
    honly = s.solve_jvp_host(V, up, tr, W_2L, dtraj=t[2])
    donly = gpu_jvp(s, V, up, tr, W_2L, (None, None, t[2], None))
    for k in ("dV", "du0", "jvp_status"):
        assert np.array_equal(r[k], again[k]), f"{k}: run to run"
        assert np.array_equal(r[k], host[k]), f"{k}: host entry against the device entry"
        assert np.array_equal(honly[k], donly[k]), f"{k}: host entry with NULL tangents"
    assert hfree["dV"] is None and np.array_equal(hfree["du0"], r["du0"])
    one = s.solve_jvp_host(V[3:4], up[3:4], tr[3:4], W_2L, *(a[3:4] for a in t))
    s.close()
    assert one["jvp_status"].tolist() == [0]
    check(one["dV"], ref[3:4], "B = 1")


def test_jvp_launch_replays_from_a_graph(ctx):
    import torch
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    _, up, tr = ctx.inputs(model, N, B)
    V, t = ctx.plan(model, N, B), ctx.tan(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_jvp(s, V, up, tr, W_2L, t)
    dVin, dup, dtr, dw = (dev(a) for a in (np.zeros_like(V), up, tr, W_2L))
    dt = [dev(a) for a in t]
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    out = dict(dV=f64(B, V.shape[1]), du0=f64(B, nu), jvp_status=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
               workspace=f64(s.solve_jvp_workspace_bytes(B) // 8))
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):   # one launch on the capture stream before capturing (module load)
        s.solve_jvp(B, dVin, dup, dtr, dw, *dt, stream=cs.cuda_stream, **out)
    torch.cuda.current_stream().wait_stream(cs)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        s.solve_jvp(B, dVin, dup, dtr, dw, *dt, stream=cs.cuda_stream, **out)
    dVin.copy_(dev(V))   # the graph reads the live buffers
    out["dV"].zero_()
    out["du0"].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in ("dV", "du0", "jvp_status"):
        assert np.array_equal(out[k].cpu().numpy(), r[k]), k
    s.close()


# ---------------------------------------------------------------- 12. state bounds under the sensitivity barrier
@pytest.mark.parametrize("case", [("two_link_arm", 3, 9), ("two_link_arm", 17, 37), ("exo_arm", 7, 9)], ids=_id)
def test_state_bounded_handle_matches_the_dense_reference(case, mmpc_mod, tmp_path_factory):
    from test_gpu_xb_sensitivity import Ctx as XCtx
    from test_xb_sensitivity_reference import CAP_PIN
    model, N, B = case
    pat = "box"
    x = XCtx(mmpc_mod, str(tmp_path_factory.mktemp("solve_jvp_xb")))
    _, up, tr, _ = x.inputs(model, pat, N, B)
    xl, xu, ul, uu = x.bounds(model, pat)
    V = x.plan(model, pat, N, B)
    t = tangents(OMODEL[model], N, np.random.default_rng(SEED + 11 * N + B), B)
    s = x.solver(model, N, pat, CAP_PIN)
    for hess in ("exact", "gn"):
        r = gpu_jvp(s, V, up, tr, WEIGHTS[model], t, ul, uu, hessian=hess_id(mmpc_mod, hess))
        assert (r["jvp_status"] == 0).all(), r["jvp_status"]
        ref = xb_dense_jvp_batch(OMODEL[model], N, H, V, up, tr, WEIGHTS[model], *t, hess == "exact", xl, xu, ul, uu,
                                 cap=CAP_PIN)
        check(r["dV"], ref, f"state-bounded {_id(case)} {hess}")
    s.close()


# ---------------------------------------------------------------- 13. autograd
@pytest.mark.parametrize("weights", ["shared", "rows"])
def test_autograd_forward_mode_is_one_jvp_call(weights, ctx):
    import torch
    import torch.autograd.forward_ad as fwAD
    from mmpc.autograd import DifferentiableSolver
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    K = nx + nu
    x0, up, tr = ctx.inputs(model, N, B)
    t = ctx.tan(model, N, B)
    w = W_2L if weights == "shared" else np.tile(W_2L, (B, 1))
    dw = t[3][0] if weights == "shared" else t[3]
    dw_rows = np.tile(t[3][0], (B, 1)) if weights == "shared" else t[3]
    s = ctx.solver(model, N)
    ds = DifferentiableSolver(s)
    with fwAD.dual_level():
        duals = [fwAD.make_dual(dev(p), dev(d)) for p, d in ((x0, t[0]), (up, t[1]), (tr, t[2]), (w, dw))]
        V, status, _ = ds(*duals)
        Vp, Vt = fwAD.unpack_dual(V)
        Vp, Vt = Vp.clone(), Vt.clone()
    assert (status == 0).all() and ds.last_jvp_status is not None and (ds.last_jvp_status == 0).all()
    direct = s.solve_jvp(B, Vp, dev(up), dev(tr), dev(w), dev(t[0]), dev(t[1]), dev(t[2]), dev(dw_rows),
                         weights_stride=0 if w.ndim == 1 else nx + 2 * nu)
    torch.cuda.synchronize()
    assert torch.equal(Vt, direct["dV"]) and Vt.abs().max() > 1e-3
    # torch.func.jvp, tangents in x0 and traj alone
    _, ft = torch.func.jvp(lambda a, b: ds(a, dev(up), b, dev(w))[0], (dev(x0), dev(tr)), (dev(t[0]), dev(t[2])))
    fd = s.solve_jvp(B, Vp, dev(up), dev(tr), dev(w), dx0=dev(t[0]), dtraj=dev(t[2]),
                     weights_stride=0 if w.ndim == 1 else nx + 2 * nu)
    torch.cuda.synchronize()
    assert torch.equal(ft, fd["dV"])
    # reverse mode in the same process: still one solve_vjp call
    tx0, tup, ttr, tw = (dev(a).requires_grad_() for a in (x0, up, tr, w))
    V, status, _ = ds(tx0, tup, ttr, tw)
    loss = ((V[:, nx:K] - 0.25) ** 2).sum() + (V[:, N * K:] ** 2).sum()
    loss.backward()
    Vn = V.detach()
    Vbar = torch.zeros_like(Vn)
    Vbar[:, nx:K] = 2 * (Vn[:, nx:K] - 0.25)
    Vbar[:, N * K:] = 2 * Vn[:, N * K:]
    back = s.solve_vjp(B, Vn, dev(up), dev(tr), dev(w), Vbar, weights_stride=0 if w.ndim == 1 else nx + 2 * nu)
    torch.cuda.synchronize()
    wb = back["weights_bar"].sum(0) if weights == "shared" else back["weights_bar"]
    for grad, want in ((tx0.grad, back["x0_bar"]), (tup.grad, back["u_prev_bar"]), (ttr.grad, back["traj_bar"]),
                       (tw.grad, wb)):
        assert grad is not None and grad.shape == want.shape and torch.equal(grad, want)
    s.close()


# ---------------------------------------------------------------- 14. a generated model
def test_generated_model_satisfies_the_adjoint_identity(mmpc_mod, tmp_path_factory):
    from test_gpu_sx_sensitivity import Ctx as SxCtx
    from test_gpu_sx_models import weights as sx_weights
    case = ("free", "cart_pole", 17, 37)
    _, model, N, B = case
    nx, nu = 4, 1
    x = SxCtx(mmpc_mod, str(tmp_path_factory.mktemp("solve_jvp_sx")))
    s = x.solver(case)   # skips when the library is not generated
    assert (s.nx, s.nu) == (nx, nu)
    _, up, tr, Vbar = x.inputs(case)
    V, w = x.plan(case), sx_weights(nx, nu)
    rng = np.random.default_rng(SEED + 11 * N + B)
    t = tuple(rng.standard_normal((B,) + sh) for sh in ((nx,), (nu,), (N, nx), (nx + 2 * nu,)))
    for hess in ("exact", "gn"):
        j = gpu_jvp(s, V, up, tr, w, t, hessian=hess_id(mmpc_mod, hess))
        v = gpu_vjp(s, V, up, tr, w, Vbar, hessian=hess_id(mmpc_mod, hess))
        f = gpu_jvp(s, V, up, tr, w, t, hessian=hess_id(mmpc_mod, hess), forward_free=True)
        assert (j["jvp_status"] == 0).all() and (v["vjp_status"] == 0).all()
        assert np.array_equal(j["du0"], j["dV"][:, nx:nx + nu]) and np.array_equal(f["du0"], j["du0"])
        gap, scale = identity_gap(Vbar, j["dV"], v, t)
        print(f"cart_pole {hess}: worst gap / bound = {(gap / (TOL * np.maximum(1.0, scale))).max():.3e}")
        assert np.abs(j["dV"]).max() > 1e-3 and (gap <= TOL * np.maximum(1.0, scale)).all(), (hess, gap.max())
    s.close()
