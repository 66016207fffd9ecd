"""GPU: reverse-mode products of the solve, theta_bar = (d V* / d theta)^T V_bar (mmpc_solve_vjp_batch).

V* comes from the GPU solve, V_bar is standard normal from a fixed seed, the reference is the dense KKT solve of
tests/sens_reference.py (dense_vjp), not a second Riccati recursion.  Inputs as in
tests/test_gpu_feedback_gains.py: oracle.synth(20250213, 0, B, N, 0.002), WEIGHTS_CFG and W_EXO.  Every comparison with
the reference is per instance and per output array (x0_bar, u_prev_bar, traj_bar, weights_bar, adj_V) at
1e-10 max(1, max |ref|), the project's standing GPU-versus-reference tolerance.

1. parity, both Hessians, all five outputs: 2-link (N, B) = (1, 5) (2, 3) (3, 9) (17, 37) (33, 65) and the exo (1, 5)
   (7, 9) (21, 9) -- N = 1 has no recursion and a one-stage forward sweep, 5 and 37 leave a partial wave, 65 makes a
   second workgroup of one lane; vjp_status 0 everywhere.
2. control bounds: 2-link (3, 9) and (17, 37) under +-2 Nm, shared and as a [B, nu] table with a padded stride, the exo
   (7, 9) under test_gpu_bounded_shapes's box: at least one held and one free control per case, adj_V exactly 0 on
   held controls, everything else at the tolerance.
3. pins: n_pin = 2 at (17, 37): adj_V on u_0, u_1 and u_prev_bar exactly 0, x0_bar and the rest match the reference
   with those stages held.
4. backward-only mode at (17, 37): x0_bar and u_prev_bar bit for bit the full call's, with a NULL workspace.
5. per-instance weights with a padded stride and NaN in the padding, at (17, 37).
6. the solver's own map: 2-link (17, 5), 16-lane solves with tol_grad 1e-11 and tol_defect 1e-12, central differences
   at delta = 1e-4 (relative, fd_delta of the CPU module) in three entries of each input (two of u_prev), warm-started
   from V*, against the exact outputs at 1e-6 max(1, |ref|) (the CPU value of the same experiment is 8.1e-10).
7. fallback: instance 0 gets its velocity targets moved by 1000 (1, -1) (test_gpu_feedback_gains item 6: the exact
   model is then indefinite): vjp_status 1 and the Gauss-Newton reference's outputs; the instance beside it keeps
   status 0 and the exact outputs.
8. non-finite input: an instance with a NaN in V reports 2 with all-zero rows; its workgroup- and wave-mates are bit
   for bit those of the clean batch.
9. the host entry, B = 1, a captured-graph replay bit for bit the direct call, and determinism run to run.
10. autograd (mmpc/autograd.py), 2-link (17, 37): loss = sum |u_0* - c|^2 + sum |x_N*|^2; .backward() gives x0.grad,
    u_prev.grad, traj.grad and weights.grad (shared and [B, nw]) bit for bit a direct solve_vjp with V_bar =
    d loss / d V (the shared case its sum over the batch), and they match the dense reference at the tolerance."""
import numpy as np
import pytest

from sens_reference import OUT, dense_vjp_batch, fd_delta, held_mask
from test_gpu_feedback_gains import BOUNDED, DIMS, H, OMODEL, SEED, SHAPES, W_2L, WEIGHTS, Ctx, _id, dev, hess_id

pytestmark = pytest.mark.gpu

TOL = 1e-10
PARITY = [(model, N, B, hess) for model, shapes in SHAPES.items() for (N, B) in shapes for hess in ("exact", "gn")]


class VCtx(Ctx):
    """test_gpu_feedback_gains's shared state (inputs, GPU plans) plus V_bar and the dense VJP references"""

    def __init__(self, m, d):
        super().__init__(m, d)
        self.vbars_, self.vrefs_ = {}, {}

    def vbar(self, model, N, B):
        key = (model, N, B)
        if key not in self.vbars_:
            nx, nu = DIMS[model]
            vb = np.random.default_rng(SEED + 7 * N + B).standard_normal((B, nx * (N + 1) + nu * N))
            vb.setflags(write=False)
            self.vbars_[key] = vb
        return self.vbars_[key]

    def vref(self, model, N, B, exact, bounded=False, n_pin=0):
        key = (model, N, B, exact, bounded, n_pin)
        if key not in self.vrefs_:
            _, up, tr = self.inputs(model, N, B)
            lb, ub = self.bounds(model, bounded)
            r = dense_vjp_batch(OMODEL[model], N, H, self.plan(model, N, B, bounded), up, tr, WEIGHTS[model],
                                self.vbar(model, N, B), exact, lb, ub, n_pin)
            for a in r.values():
                a.setflags(write=False)
            self.vrefs_[key] = r
        return self.vrefs_[key]


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return VCtx(mmpc_mod, str(tmp_path_factory.mktemp("solve_vjp")))


def gpu_vjp(s, V, up, tr, w, Vbar, lb=None, ub=None, **kw):
    """one device-pointer VJP call on fresh tensors: the outputs as numpy"""
    import torch
    r = s.solve_vjp(V.shape[0], dev(V), dev(up), dev(tr), dev(w), dev(Vbar), u_lb=dev(lb), u_ub=dev(ub), **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def check(got, ref, what="", keys=OUT):
    """per instance and per output array: max |got - ref| <= TOL max(1, max |ref|)"""
    worst = 0.0
    for k in keys:
        g, r = got[k].reshape(got[k].shape[0], -1), ref[k].reshape(ref[k].shape[0], -1)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        err = np.abs(g - r).max(axis=1)
        bound = TOL * np.maximum(1.0, np.abs(r).max(axis=1))
        worst = max(worst, (err / bound).max())
        assert np.isfinite(g).all() and (err <= bound).all(), (what, k, err.max(), np.argwhere(err > bound)[:5])
    print(f"{what}: worst err / bound = {worst:.3e}")


def controls(model, N, adj_V):
    """[B, N, nu] view of the control entries of adj_V"""
    nx, nu = DIMS[model]
    return adj_V[:, :-nx].reshape(adj_V.shape[0], N, nx + nu)[:, :, nx:]


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", PARITY, ids=_id)
def test_outputs_match_the_dense_reference(case, ctx):
    model, N, B, hess = case
    _, up, tr = ctx.inputs(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_vjp(s, ctx.plan(model, N, B), up, tr, WEIGHTS[model], ctx.vbar(model, N, B), hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["vjp_status"] == 0).all(), r["vjp_status"]
    check(r, ctx.vref(model, N, B, hess == "exact"), _id(case))


# ---------------------------------------------------------------- 2. control bounds
@pytest.mark.parametrize("case", BOUNDED, ids=_id)
def test_held_controls_get_zero_and_the_rest_matches(case, ctx):
    model, N, B, form = case
    nx, nu = DIMS[model]
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B, True)
    lb, ub = ctx.bounds(model, True)
    held = np.stack([held_mask(OMODEL[model], N, V[b], lb, ub, 0) for b in range(B)])
    print(f"{_id(case)}: {int(held.sum())} held controls of {held.size}")
    assert held.any() and not held.all(), "the case needs at least one held and one free control"
    s = ctx.solver(model, N)
    for hess in ("exact", "gn"):
        ref = ctx.vref(model, N, B, hess == "exact", True)
        if form == "shared":
            r = gpu_vjp(s, V, up, tr, WEIGHTS[model], ctx.vbar(model, N, B), lb, ub, hessian=hess_id(ctx.m, hess))
        else:   # a row per instance at a padded stride, NaN in the padding, buffers of the exact size
            stride = nu + 3
            tl = np.full((B - 1) * stride + nu, np.nan)
            tu = np.full((B - 1) * stride + nu, np.nan)
            for b in range(B):
                tl[b * stride:b * stride + nu], tu[b * stride:b * stride + nu] = lb, ub
            r = gpu_vjp(s, V, up, tr, WEIGHTS[model], ctx.vbar(model, N, B), tl, tu, bounds_stride=stride,
                        hessian=hess_id(ctx.m, hess))
        assert (r["vjp_status"] == 0).all(), r["vjp_status"]
        assert (controls(model, N, r["adj_V"])[held] == 0.0).all(), "adj_V must be exactly 0 on a held control"
        assert (controls(model, N, ref["adj_V"])[held] == 0.0).all()
        check(r, ref, f"{_id(case)} {hess}")
    s.close()


# ---------------------------------------------------------------- 3. pins
def test_pinned_stages_get_zero(ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    ref = ctx.vref(model, N, B, True, n_pin=2)
    s = ctx.solver(model, N)
    r = gpu_vjp(s, ctx.plan(model, N, B), up, tr, W_2L, ctx.vbar(model, N, B), n_pin=2)
    s.close()
    assert (r["vjp_status"] == 0).all(), r["vjp_status"]
    aU = controls(model, N, r["adj_V"])
    assert (aU[:, :2] == 0.0).all() and (r["u_prev_bar"] == 0.0).all() and (ref["u_prev_bar"] == 0.0).all()
    assert np.abs(aU[:, 2:]).max() > 1e-3 and np.abs(r["x0_bar"]).max() > 1e-3
    check(r, ref, "pins")


# ---------------------------------------------------------------- 4. backward-only mode
@pytest.mark.parametrize("hess", ["exact", "gn"])
def test_backward_only_is_bit_for_bit_the_full_call(hess, ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    V, Vbar = ctx.plan(model, N, B), ctx.vbar(model, N, B)
    s = ctx.solver(model, N)
    full = gpu_vjp(s, V, up, tr, W_2L, Vbar, hessian=hess_id(ctx.m, hess))
    back = gpu_vjp(s, V, up, tr, W_2L, Vbar, hessian=hess_id(ctx.m, hess), backward_only=True)   # workspace NULL
    s.close()
    assert back["traj_bar"] is None and back["weights_bar"] is None and back["adj_V"] is None
    assert (full["vjp_status"] == 0).all() and (back["vjp_status"] == 0).all()
    assert np.array_equal(back["x0_bar"], full["x0_bar"]) and np.array_equal(back["u_prev_bar"], full["u_prev_bar"])
    check(back, ctx.vref(model, N, B, hess == "exact"), f"backward-only {hess}", keys=("x0_bar", "u_prev_bar"))


# ---------------------------------------------------------------- 5. per-instance weights
def test_per_instance_weights_at_a_padded_stride(ctx):
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    nw = nx + 2 * nu
    _, up, tr = ctx.inputs(model, N, B)
    V, Vbar = ctx.plan(model, N, B), ctx.vbar(model, N, B)
    wi = W_2L[None, :] * np.random.default_rng(SEED).uniform(0.5, 2.0, (B, nw))   # V is no solution for these
    stride = nw + 5
    wt = np.full((B - 1) * stride + nw, np.nan)   # NaN in the padding, a buffer of the exact size
    for b in range(B):
        wt[b * stride:b * stride + nw] = wi[b]
    s = ctx.solver(model, N)
    r = gpu_vjp(s, V, up, tr, wt, Vbar, weights_stride=stride)
    s.close()
    assert (r["vjp_status"] == 0).all(), r["vjp_status"]
    check(r, dense_vjp_batch(OMODEL[model], N, H, V, up, tr, wi, Vbar, True), "per-instance weights")


# ---------------------------------------------------------------- 6. the solver's own map
def test_outputs_are_the_derivative_of_the_solve(ctx):
    model, N, B = "two_link_arm", 17, 5
    nx, nu = DIMS[model]
    m = ctx.m
    x0, up, tr = ctx.inputs(model, N, B)
    Vbar = ctx.vbar(model, N, B)
    s = ctx.solver(model, N, kkt_solver=m.KKT_RICCATI_GROUP, tol_grad=1e-11, tol_defect=1e-12)
    assert s.hessian_for(B) == m.HESSIAN_EXACT
    g = s.solve_batch_host(x0, up, tr, W_2L)
    assert (g["status"] == 0).all()
    V = g["V"]
    r = s.solve_vjp_host(V, up, tr, W_2L, Vbar, hessian=m.HESSIAN_EXACT)
    assert (r["vjp_status"] == 0).all()
    wt = np.tile(W_2L, (B, 1))
    pick = lambda n: sorted({0, n // 2, n - 1})  # noqa: E731
    base = dict(x0_bar=x0, u_prev_bar=up, traj_bar=tr.reshape(B, -1), weights_bar=wt)
    # stage 0's position targets do not move V* (x_1's positions follow from x_0 alone): start at a velocity target
    idx = dict(x0_bar=pick(nx), u_prev_bar=pick(nu), traj_bar=sorted({nx // 2, N * nx // 2, N * nx - 1}),
               weights_bar=[1, nx, nx + 2 * nu - 1])
    worst = 0.0
    for name in base:
        for i in idx[name]:
            delta = fd_delta(name, base[name][:, i])
            Vs = []
            for sign in (1.0, -1.0):
                a = dict(base)
                t = a[name].copy()
                t[:, i] += sign * delta
                a[name] = t
                o = s.solve_batch_host(a["x0_bar"], a["u_prev_bar"], a["traj_bar"].reshape(B, N, nx), a["weights_bar"],
                                       V=V)
                assert (o["status"] == 0).all(), (name, i, o["status"])
                Vs.append(o["V"])
            fd = ((Vs[0] - Vs[1]) * Vbar).sum(1) / (2 * delta)
            got = r[name].reshape(B, -1)
            err = np.abs(fd - got[:, i]) / np.maximum(1.0, np.abs(got).max(axis=1))
            print(f"{name}[{i}]: central differences against the VJP, max relative error {err.max():.3e}")
            worst = max(worst, err.max())
            assert (err <= 1e-6).all(), (name, i, fd, got[:, i])
    s.close()
    print(f"central differences of the solve against the VJP: worst {worst:.3e}")


# ---------------------------------------------------------------- 7. fallback
def test_indefinite_exact_model_falls_back_to_gauss_newton(ctx):
    model, N, B = "two_link_arm", 17, 2
    om = OMODEL[model]
    _, up, tr = ctx.inputs(model, N, B)
    V, Vbar = ctx.plan(model, N, B), ctx.vbar(model, N, B)
    tr2 = tr.copy()   # V is no solution for these targets: velocity targets of instance 0 moved by 1000 (1, -1)
    tr2[0, :, 2] += 1000.0
    tr2[0, :, 3] -= 1000.0
    s = ctx.solver(model, N)
    r = gpu_vjp(s, V, up, tr2, W_2L, Vbar, hessian=ctx.m.HESSIAN_EXACT)
    b = gpu_vjp(s, V, up, tr2, W_2L, Vbar, hessian=ctx.m.HESSIAN_EXACT, backward_only=True)
    s.close()
    assert r["vjp_status"].tolist() == [1, 0] and b["vjp_status"].tolist() == [1, 0], (r["vjp_status"], b["vjp_status"])
    assert np.array_equal(b["x0_bar"], r["x0_bar"]) and np.array_equal(b["u_prev_bar"], r["u_prev_bar"])
    first = {k: v[:1] for k, v in r.items()}
    second = {k: v[1:] for k, v in r.items()}
    check(first, dense_vjp_batch(om, N, H, V[:1], up[:1], tr2[:1], W_2L, Vbar[:1], False), "fallback instance")
    check(second, dense_vjp_batch(om, N, H, V[1:], up[1:], tr2[1:], W_2L, Vbar[1:], True), "its neighbour")


# ---------------------------------------------------------------- 8. non-finite input
@pytest.mark.parametrize("where", ["state", "x_N"])
def test_nan_instance_fails_alone(where, ctx):
    model, N, B, bad = "two_link_arm", 17, 37, 5
    _, up, tr = ctx.inputs(model, N, B)
    V, Vbar = ctx.plan(model, N, B), ctx.vbar(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar)
    V2 = V.copy()
    V2[bad, 3 * 6 + 1 if where == "state" else V.shape[1] - 1] = np.nan
    r2 = gpu_vjp(s, V2, up, tr, W_2L, Vbar)
    s.close()
    others = np.arange(B) != bad
    assert (r["vjp_status"] == 0).all()
    assert r2["vjp_status"][bad] == 2 and (r2["vjp_status"][others] == 0).all(), r2["vjp_status"]
    for k in OUT:
        assert (r2[k][bad] == 0.0).all(), k
        assert np.array_equal(r2[k][others], r[k][others]), f"{k}: the neighbours of a failed instance must not change"


# ---------------------------------------------------------------- 9. remaining paths
def test_host_entry_single_instance_and_determinism(ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    V, Vbar = ctx.plan(model, N, B), ctx.vbar(model, N, B)
    ref = ctx.vref(model, N, B, True)
    s = ctx.solver(model, N)
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar)
    again = gpu_vjp(s, V, up, tr, W_2L, Vbar)
    host = s.solve_vjp_host(V, up, tr, W_2L, Vbar)
    hback = s.solve_vjp_host(V, up, tr, W_2L, Vbar, backward_only=True)
    for k in OUT + ("vjp_status",):
        assert np.array_equal(r[k], again[k]), f"{k}: run to run"
        assert np.array_equal(r[k], host[k]), f"{k}: host entry against the device entry"
    assert np.array_equal(hback["x0_bar"], r["x0_bar"]) and np.array_equal(hback["u_prev_bar"], r["u_prev_bar"])
    one = s.solve_vjp_host(V[3:4], up[3:4], tr[3:4], W_2L, Vbar[3:4])
    s.close()
    assert one["vjp_status"].tolist() == [0]
    check(one, {k: v[3:4] for k, v in ref.items()}, "B = 1")


def test_vjp_launch_replays_from_a_graph(ctx):
    import torch
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    _, up, tr = ctx.inputs(model, N, B)
    V, Vbar = ctx.plan(model, N, B), ctx.vbar(model, N, B)
    s = ctx.solver(model, N)
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar)
    dV, dup, dtr, dw, dvb = (dev(a) for a in (np.zeros_like(V), up, tr, W_2L, Vbar))
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    out = dict(x0_bar=f64(B, nx), u_prev_bar=f64(B, nu), traj_bar=f64(B, N, nx), weights_bar=f64(B, nx + 2 * nu),
               adj_V=f64(B, V.shape[1]), vjp_status=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
               workspace=f64(s.solve_vjp_workspace_bytes(B) // 8))
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):   # one launch on the capture stream before capturing (module load)
        s.solve_vjp(B, dV, dup, dtr, dw, dvb, stream=cs.cuda_stream, **out)
    torch.cuda.current_stream().wait_stream(cs)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        s.solve_vjp(B, dV, dup, dtr, dw, dvb, stream=cs.cuda_stream, **out)
    dV.copy_(dev(V))   # the graph reads the live buffers
    for k in OUT:
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in OUT + ("vjp_status",):
        assert np.array_equal(out[k].cpu().numpy(), r[k]), k
    s.close()


# ---------------------------------------------------------------- 10. autograd
@pytest.mark.parametrize("weights", ["shared", "rows"])
def test_autograd_backward_is_one_vjp_call(weights, ctx):
    import torch
    from mmpc.autograd import DifferentiableSolver
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    K = nx + nu
    x0, up, tr = ctx.inputs(model, N, B)
    w = W_2L if weights == "shared" else np.tile(W_2L, (B, 1))
    s = ctx.solver(model, N)
    ds = DifferentiableSolver(s)
    tx0, tup, ttr, tw = (dev(a).requires_grad_() for a in (x0, up, tr, w))
    c = dev(np.full(nu, 0.25))
    V, status, iters = ds(tx0, tup, ttr, tw)
    assert not status.requires_grad and not iters.requires_grad and V.requires_grad
    assert (status == 0).all()
    loss = ((V[:, nx:K] - c) ** 2).sum() + (V[:, N * K:] ** 2).sum()
    loss.backward()
    torch.cuda.synchronize()
    Vn = V.detach().cpu().numpy()
    Vbar = np.zeros_like(Vn)
    Vbar[:, nx:K] = 2 * (Vn[:, nx:K] - 0.25)
    Vbar[:, N * K:] = 2 * Vn[:, N * K:]
    assert ds.last_vjp_status is not None and (ds.last_vjp_status == 0).all()
    direct = s.solve_vjp(B, V.detach(), dev(up), dev(tr), dev(w), dev(Vbar),
                         weights_stride=0 if w.ndim == 1 else nx + 2 * nu)
    torch.cuda.synchronize()
    wb = direct["weights_bar"].sum(0) if weights == "shared" else direct["weights_bar"]
    for grad, want in ((tx0.grad, direct["x0_bar"]), (tup.grad, direct["u_prev_bar"]), (ttr.grad, direct["traj_bar"]),
                       (tw.grad, wb)):
        assert grad is not None and grad.shape == want.shape and torch.equal(grad, want)
    s.close()
    ref = dense_vjp_batch(OMODEL[model], N, H, Vn, up, tr, W_2L, Vbar, True)
    got = dict(x0_bar=tx0.grad.cpu().numpy(), u_prev_bar=tup.grad.cpu().numpy(), traj_bar=ttr.grad.cpu().numpy())
    check(got, ref, f"autograd {weights}", keys=("x0_bar", "u_prev_bar", "traj_bar"))
    gw = tw.grad.cpu().numpy()
    if weights == "shared":   # the sum over the batch against the sum of the reference's rows: the rows' bounds add
        rw = ref["weights_bar"].sum(0)
        assert np.abs(gw - rw).max() <= (TOL * np.maximum(1.0, np.abs(ref["weights_bar"]).max(axis=1))).sum()
    else:
        check(dict(weights_bar=gw), ref, "autograd rows: weights", keys=("weights_bar",))
