"""GPU: feedback gains and the solve VJP of a state-bounded handle under its sensitivity barrier
(mmpc_set_sensitivity_barrier; include/mmpc.h).

The references are those of tests/test_xb_sensitivity_reference.py: the dense tail systems and the dense KKT solve with
the barrier's D on the diagonal and beta in the multipliers.  V* comes from the GPU interior-point solve (16-lane
solver, exact Hessian).  Inputs: oracle.synth(20250213, 0, B, N, 0.002) with the x0 velocities clipped, WEIGHTS_CFG and
W_EXO, the patterns of test_gpu_bounded_shapes.XB: 2-link `box` (|qdot| <= 0.5) and `mixed+u` (one-sided velocity
bounds, u_1 >= -1, u_2 <= 1), exo `box` (|qdot| <= 0.3).

1. parity at sigma_cap = 1e6 against dense, 1e-10 max(1, max |ref|): lane and 16-lane gain kernels (n_gain in {1, N})
   and the VJP, both Hessians; 2-link (N, B) = (1, 5) (2, 3) (3, 9) (17, 37) (33, 65), exo (1, 5) (7, 9) (21, 9); status
   0 everywhere.
2. defaults (mu_f, 1e12): the same cases against dense at 10 x the CPU floor of that case (FLOOR of the reference
   module).
3. derivative of the GPU solver's own map: 2-link (17, 5), cold 16-lane solves at tol_grad 1e-11 / tol_defect 1e-12,
   central differences at delta = 1e-5 against G_0 and against the VJP's x0_bar / u_prev_bar for V_bar = e_{u_0, c}, at
   the bound of the CPU experiment (20 x FD of the reference module).
4. pins: n_pin = 2 at (17, 37): G_0 and G_1 exactly 0, the rest at the tolerance of 1.
5. per-instance control bounds: a [B, nu] table at a padded stride with NaN in the padding; instance b equals, bit for
   bit, the shared-bounds call with its row.
6. failure isolation: an instance with a state outside its box and one with a NaN report 2 and zeros, their
   workgroup- and wave-mates are bit for bit those of the clean batch; velocity targets moved by 1000 (1, -1) make
   the exact model of an instance without an active bound indefinite: status 1 and the Gauss-Newton reference's
   gains, the neighbour untouched.
7. bits: the VJP's backward-only mode against the full call, the host entries against the device entries, B = 1, a
   captured-graph replay, run-to-run determinism.
8. a handle without a finite state bound: switching the barrier on changes no bit of gains or VJP.
9. autograd: DifferentiableSolver on a state-bounded solver, the gradient of sum u_0 with respect to x0 and Q against
   central differences of the solve, at the bound of 3.
10. the C++ mirror (mahi-mpc_amd/host/examples/state_limit_feedback_example.cpp, 2-link N = 17 with |qdot| <= 0.5 in
   the model file): a ModelControl with feedback stages and the barrier off refuses to solve; with it on the published
   gains are bit for bit those of the C-ABI calls on the same inputs (ModelControl) and at the published plans
   (BatchModelControl, B = 5), and control_at_time(t, x) / controls_at_time(t, x) equal u_0 + G_0[:, :nx] (x - x_est_0)
   to 1e-15 max(1, |u|) (the mirror's own order of summation)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as oracle
from conftest import ROOT
from sens_reference import CAP_DEFAULT, OUT, xb_dense_gains_batch, xb_dense_vjp_batch
from test_gpu_bounded_shapes import XB
from test_gpu_feedback_gains import DIMS, OMODEL, WEIGHTS, W_2L, dev, gpu_gains, hess_id
from test_gpu_solve_vjp import gpu_vjp
from test_xb_sensitivity_reference import CAP_PIN, FD, FLOOR, H, SEED, arr, fd_errors, fd_of_solves, xb_recursion

pytestmark = pytest.mark.gpu

TOL = 1e-10
SHAPES = {"two_link_arm": [(1, 5), (2, 3), (3, 9), (17, 37), (33, 65)], "exo_arm": [(1, 5), (7, 9), (21, 9)]}
PATTERNS = {"two_link_arm": ["box", "mixed+u"], "exo_arm": ["box"]}
KERNELS = {"lane": 1, "group": 2}
CASES = [(model, pat, N, B, hess) for model, shapes in SHAPES.items() for pat in PATTERNS[model] for (N, B) in shapes
         for hess in ("exact", "gn")]


def _id(case):
    return "-".join(str(v) for v in case)


class Ctx:
    """the module's shared state: inputs, GPU plans and dense references, each computed once and left unchanged"""

    def __init__(self, m, d):
        self.m, self.dir = m, d
        self.inputs_, self.plans_, self.refs_ = {}, {}, {}

    def solver(self, model, N, pat=None, cap=None, **kw):
        """a solver with the pattern's state bounds; cap: the sensitivity barrier at (mu_f, cap), None: off"""
        nx, nu = DIMS[model]
        p = self.m.write_model_json(os.path.join(self.dir, f"{model}_{N}.json"), f"{model}_{N}", nx, nu, 2000, N,
                                    model=model)
        kw.setdefault("max_iter", 100)
        s = self.m.Solver(p, **kw)
        if pat is not None:
            s.set_state_bounds(arr(XB[model][pat][0]), arr(XB[model][pat][1]))
        if cap is not None:
            s.set_sensitivity_barrier(sigma_cap=cap)
        return s

    def bounds(self, model, pat):
        return tuple(arr(v) for v in XB[model][pat][:4])

    def inputs(self, model, pat, N, B):
        key = (model, pat, N, B)
        if key not in self.inputs_:
            nx, nu = DIMS[model]
            clip = XB[model][pat][4]
            x0, up, tr = oracle.synth(SEED, 0, B, N, H, model=OMODEL[model])
            x0[:, nx // 2:] = np.clip(x0[:, nx // 2:], -clip, clip)
            Vbar = np.random.default_rng(SEED + N).standard_normal((B, nx * (N + 1) + nu * N))
            for a in (x0, up, tr, Vbar):
                a.setflags(write=False)
            self.inputs_[key] = (x0, up, tr, Vbar)
        return self.inputs_[key]

    def plan(self, model, pat, N, B):
        """V* of the GPU interior-point solve [B, NV]"""
        key = (model, pat, N, B)
        if key not in self.plans_:
            x0, up, tr, _ = self.inputs(model, pat, N, B)
            _, _, ul, uu = self.bounds(model, pat)
            s = self.solver(model, N, pat, kkt_solver=self.m.KKT_RICCATI_GROUP, hessian=self.m.HESSIAN_EXACT)
            g = s.solve_batch_host(x0, up, tr, WEIGHTS[model], u_lb=ul, u_ub=uu)
            s.close()
            assert (g["status"] == 0).all(), g["status"]
            g["V"].setflags(write=False)
            self.plans_[key] = g["V"]
        return self.plans_[key]

    def ref(self, model, pat, N, B, exact, cap, n_pin=0):
        """the dense references at the plan: (G [B, N, nu, K], the VJP outputs)"""
        key = (model, pat, N, B, exact, cap, n_pin)
        if key not in self.refs_:
            _, up, tr, Vbar = self.inputs(model, pat, N, B)
            xl, xu, ul, uu = self.bounds(model, pat)
            V = self.plan(model, pat, N, B)
            kw = dict(n_pin=n_pin, cap=cap)
            G = xb_dense_gains_batch(OMODEL[model], N, H, V, up, tr, WEIGHTS[model], exact, xl, xu, ul, uu, **kw)
            r = xb_dense_vjp_batch(OMODEL[model], N, H, V, up, tr, WEIGHTS[model], Vbar, exact, xl, xu, ul, uu, **kw)
            G.setflags(write=False)
            self.refs_[key] = (G, r)
        return self.refs_[key]


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return Ctx(mmpc_mod, str(tmp_path_factory.mktemp("xb_sensitivity")))


def worst_gain(G, Gref):
    """max over instances and stages of err / max(1, max |ref|)"""
    assert G.shape == Gref.shape and np.isfinite(G).all(), (G.shape, Gref.shape)
    err = np.abs(G - Gref).max(axis=(2, 3))
    return (err / np.maximum(1.0, np.abs(Gref).max(axis=(2, 3)))).max()


def worst_vjp(got, ref):
    worst = 0.0
    for k in OUT:
        g, r = got[k].reshape(got[k].shape[0], -1), ref[k].reshape(ref[k].shape[0], -1)
        assert g.shape == r.shape and np.isfinite(g).all(), k
        worst = max(worst, (np.abs(g - r).max(axis=1) / np.maximum(1.0, np.abs(r).max(axis=1))).max())
    return worst


def run_all(ctx, case, cap):
    """{what: worst err / max(1, |ref|)} of the lane and 16-lane gain kernels and the VJP of a case against dense"""
    model, pat, N, B, hess = case
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    _, _, ul, uu = ctx.bounds(model, pat)
    V = ctx.plan(model, pat, N, B)
    Gref, vref = ctx.ref(model, pat, N, B, hess == "exact", cap)
    s = ctx.solver(model, N, pat, cap)
    out = {}
    for kernel in KERNELS:
        for n_gain in sorted({1, N}):
            G, st = gpu_gains(s, V, up, tr, WEIGHTS[model], ul, uu, n_gain=n_gain, hessian=hess_id(ctx.m, hess),
                              kernel=KERNELS[kernel])
            assert (st == 0).all(), (kernel, st)
            out[f"{kernel} n_gain={n_gain}"] = worst_gain(G, Gref[:, :n_gain])
    r = gpu_vjp(s, V, up, tr, WEIGHTS[model], Vbar, ul, uu, hessian=hess_id(ctx.m, hess))
    s.close()
    assert (r["vjp_status"] == 0).all(), r["vjp_status"]
    out["vjp"] = worst_vjp(r, vref)
    print(f"{_id(case)} cap {cap:.0e}: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()))
    return out


# ---------------------------------------------------------------- 1. parity at the pinned cap
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity_with_dense_at_cap_1e6(case, ctx):
    out = run_all(ctx, case, CAP_PIN)
    assert max(out.values()) <= TOL, out


# ---------------------------------------------------------------- 2. the default settings
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_defaults_within_ten_times_the_cpu_floor(case, ctx):
    model, pat, N, B, hess = case
    out = run_all(ctx, case, CAP_DEFAULT)
    assert max(out.values()) <= 10 * FLOOR[(OMODEL[model], pat, N)], out


# ---------------------------------------------------------------- 3. the derivative of the solver's own map
def test_gain_and_vjp_are_the_derivative_of_the_gpu_solve(ctx):
    model, pat, N, B = "two_link_arm", "box", 17, 5
    nx, nu = DIMS[model]
    m = ctx.m
    x0, up, tr, _ = ctx.inputs(model, pat, N, B)
    s = ctx.solver(model, N, pat, CAP_DEFAULT, kkt_solver=m.KKT_RICCATI_GROUP, hessian=m.HESSIAN_EXACT, tol_grad=1e-11,
                   tol_defect=1e-12)

    def solve(xs, us):
        g = s.solve_batch_host(xs, us, tr, W_2L)
        assert (g["status"] == 0).all(), g["status"]
        return g["V"]

    V = solve(x0, up)
    G0, st = s.feedback_gains_host(V, up, tr, W_2L, n_gain=1, hessian=m.HESSIAN_EXACT)
    assert (st == 0).all(), st
    bars = np.zeros((nu, B, nx + nu))
    for c in range(nu):
        Vbar = np.zeros_like(V)
        Vbar[:, nx + c] = 1.0
        r = s.solve_vjp_host(V, up, tr, W_2L, Vbar, hessian=m.HESSIAN_EXACT, backward_only=True)
        assert (r["vjp_status"] == 0).all()
        bars[c] = np.hstack([r["x0_bar"], r["u_prev_bar"]])
    fd = fd_of_solves(solve, x0, up, nx, nu)
    s.close()
    eg, eb = fd_errors(fd, G0[:, 0], bars)
    print(f"central differences of cold GPU solves: against G_0 {eg:.3e}, against x0_bar | u_prev_bar {eb:.3e}")
    assert max(eg, eb) <= 20 * FD


# ---------------------------------------------------------------- 4. pins
@pytest.mark.parametrize("kernel", KERNELS)
def test_pinned_stages_have_zero_gains(kernel, ctx):
    model, pat, N, B = "two_link_arm", "box", 17, 37
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    V = ctx.plan(model, pat, N, B)
    Gref, vref = ctx.ref(model, pat, N, B, True, CAP_PIN, n_pin=2)
    s = ctx.solver(model, N, pat, CAP_PIN)
    G, st = gpu_gains(s, V, up, tr, W_2L, n_pin=2, kernel=KERNELS[kernel])
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar, n_pin=2)
    s.close()
    assert (st == 0).all() and (r["vjp_status"] == 0).all()
    assert (G[:, :2] == 0.0).all() and (Gref[:, :2] == 0.0).all()
    assert np.abs(G[:, 2:]).max() > 0.1
    assert (r["u_prev_bar"] == 0.0).all()
    wg, wv = worst_gain(G, Gref), worst_vjp(r, vref)
    print(f"pins {kernel}: gains {wg:.2e}, vjp {wv:.2e}")
    assert max(wg, wv) <= TOL


# ---------------------------------------------------------------- 5. per-instance control bounds
def test_control_bound_table_rows_equal_the_shared_calls(ctx):
    model, pat, N, B = "two_link_arm", "mixed+u", 17, 37
    nx, nu = DIMS[model]
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    _, _, ul, uu = ctx.bounds(model, pat)
    V = ctx.plan(model, pat, N, B)
    rows = [(np.where(np.isfinite(ul), ul - 0.125 * i, ul), np.where(np.isfinite(uu), uu + 0.125 * i, uu))
            for i in range(3)]
    stride = nu + 3
    tl = np.full((B - 1) * stride + nu, np.nan)
    tu = np.full((B - 1) * stride + nu, np.nan)
    for b in range(B):
        tl[b * stride:b * stride + nu], tu[b * stride:b * stride + nu] = rows[b % 3]
    s = ctx.solver(model, N, pat, CAP_DEFAULT)
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr, W_2L, tl, tu, stride, kernel=KERNELS[kernel])
        assert (st == 0).all(), st
        shared = [gpu_gains(s, V, up, tr, W_2L, lo, hi, kernel=KERNELS[kernel])[0] for lo, hi in rows]
        assert not np.array_equal(shared[0], shared[1]), "the rows must matter"
        for b in range(B):
            assert np.array_equal(G[b], shared[b % 3][b]), (kernel, b)
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar, tl, tu, bounds_stride=stride)
    shared = [gpu_vjp(s, V, up, tr, W_2L, Vbar, lo, hi) for lo, hi in rows]
    s.close()
    assert (r["vjp_status"] == 0).all()
    for k in OUT:
        for b in range(B):
            assert np.array_equal(r[k][b], shared[b % 3][k][b]), (k, b)


# ---------------------------------------------------------------- 6. failure isolation
@pytest.mark.parametrize("what", ["outside", "on_bound", "nan"])
def test_bad_instance_fails_alone(what, ctx):
    model, pat, N, B, bad = "two_link_arm", "box", 17, 37, 5
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    V = ctx.plan(model, pat, N, B)
    V2 = V.copy()
    V2[bad, 3 * 6 + 2] = {"outside": 0.625, "on_bound": 0.5, "nan": np.nan}[what]   # the first velocity of x_3
    others = np.arange(B) != bad
    s = ctx.solver(model, N, pat, CAP_DEFAULT)
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr, W_2L, kernel=KERNELS[kernel])
        G2, st2 = gpu_gains(s, V2, up, tr, W_2L, kernel=KERNELS[kernel])
        assert (st == 0).all()
        assert st2[bad] == 2 and (G2[bad] == 0.0).all(), (kernel, st2[bad])
        assert (st2[others] == 0).all()
        assert np.array_equal(G2[others], G[others]), "the neighbours of a failed instance must not change"
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar)
    r2 = gpu_vjp(s, V2, up, tr, W_2L, Vbar)
    s.close()
    assert (r["vjp_status"] == 0).all() and r2["vjp_status"][bad] == 2 and (r2["vjp_status"][others] == 0).all()
    for k in OUT:
        assert (r2[k][bad] == 0.0).all(), k
        assert np.array_equal(r2[k][others], r[k][others]), k


def test_indefinite_exact_model_falls_back_to_gauss_newton(ctx):
    model, pat, N, B = "two_link_arm", "box", 17, 37
    om = OMODEL[model]
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    xl, xu, ul, uu = ctx.bounds(model, pat)
    V, up, Vbar = ctx.plan(model, pat, N, B)[:2], up[:2], Vbar[:2]
    # V is no solution for these targets: velocity targets of instance 1 moved by 1000 (1, -1).  (Instance 0, which
    # the unbounded test moves, stays positive definite here: the barrier's D on its active velocity bounds outweighs
    # the negative curvature; instance 1 has no active bound.)
    tr2 = tr[:2].copy()
    tr2[1, :, 2] += 1000.0
    tr2[1, :, 3] -= 1000.0
    with pytest.raises(np.linalg.LinAlgError):   # some M_uu of the exact recursion is not positive definite
        xb_recursion(om, N, H, V[1], up[1], tr2[1], W_2L, None, True, xl, xu, cap=CAP_PIN)
    s = ctx.solver(model, N, pat, CAP_PIN)
    gref = [xb_dense_gains_batch(om, N, H, V[b:b + 1], up[b:b + 1], tr2[b:b + 1], W_2L, b == 0, xl, xu, cap=CAP_PIN)
            for b in range(2)]
    vref = [xb_dense_vjp_batch(om, N, H, V[b:b + 1], up[b:b + 1], tr2[b:b + 1], W_2L, Vbar[b:b + 1], b == 0, xl, xu,
                               cap=CAP_PIN) for b in range(2)]
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr2, W_2L, hessian=ctx.m.HESSIAN_EXACT, kernel=KERNELS[kernel])
        assert st.tolist() == [0, 1], (kernel, st)
        assert max(worst_gain(G[b:b + 1], gref[b]) for b in range(2)) <= TOL
    r = gpu_vjp(s, V, up, tr2, W_2L, Vbar, hessian=ctx.m.HESSIAN_EXACT)
    s.close()
    assert r["vjp_status"].tolist() == [0, 1]
    assert max(worst_vjp({k: r[k][b:b + 1] for k in OUT}, vref[b]) for b in range(2)) <= TOL


# ---------------------------------------------------------------- 7. bits
def test_backward_only_host_entries_single_instance_and_determinism(ctx):
    model, pat, N, B = "two_link_arm", "mixed+u", 17, 37
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    _, _, ul, uu = ctx.bounds(model, pat)
    V = ctx.plan(model, pat, N, B)
    Gref, vref = ctx.ref(model, pat, N, B, True, CAP_DEFAULT)
    floor = 10 * FLOOR[(OMODEL[model], pat, N)]
    s = ctx.solver(model, N, pat, CAP_DEFAULT)
    for kernel in KERNELS:
        G, st = gpu_gains(s, V, up, tr, W_2L, ul, uu, kernel=KERNELS[kernel])
        Gr, str_ = gpu_gains(s, V, up, tr, W_2L, ul, uu, kernel=KERNELS[kernel])
        assert np.array_equal(G, Gr) and np.array_equal(st, str_), "run to run"
        Gh, sth = s.feedback_gains_host(V, up, tr, W_2L, u_lb=ul, u_ub=uu, kernel=KERNELS[kernel])
        assert np.array_equal(Gh, G) and np.array_equal(sth, st), "host entry against the device entry"
        G1, st1 = s.feedback_gains_host(V[3:4], up[3:4], tr[3:4], W_2L, u_lb=ul, u_ub=uu, n_gain=8,
                                        kernel=KERNELS[kernel])
        assert st1.tolist() == [0] and worst_gain(G1, Gref[3:4, :8]) <= floor
    Ga, sta = s.feedback_gains_host(V, up, tr, W_2L, u_lb=ul, u_ub=uu)   # AUTO picks a kernel by B
    assert (sta == 0).all() and worst_gain(Ga, Gref) <= floor
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar, ul, uu)
    rr = gpu_vjp(s, V, up, tr, W_2L, Vbar, ul, uu)
    rb = gpu_vjp(s, V, up, tr, W_2L, Vbar, ul, uu, backward_only=True)
    rh = s.solve_vjp_host(V, up, tr, W_2L, Vbar, u_lb=ul, u_ub=uu)
    r1 = s.solve_vjp_host(V[3:4], up[3:4], tr[3:4], W_2L, Vbar[3:4], u_lb=ul, u_ub=uu)
    s.close()
    for k in OUT + ("vjp_status",):
        assert np.array_equal(r[k], rr[k]), ("run to run", k)
        assert np.array_equal(r[k], rh[k]), ("host entry", k)
    for k in ("x0_bar", "u_prev_bar", "vjp_status"):
        assert np.array_equal(r[k], rb[k]), ("backward-only", k)
    assert rb["traj_bar"] is None and rb["adj_V"] is None
    assert r1["vjp_status"].tolist() == [0] and worst_vjp(r1, {k: v[3:4] for k, v in vref.items()}) <= floor


@pytest.mark.parametrize("kernel", KERNELS)
def test_launches_replay_from_a_graph(kernel, ctx):
    import torch
    model, pat, N, B = "two_link_arm", "box", 17, 37
    nx, nu = DIMS[model]
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    V = ctx.plan(model, pat, N, B)
    s = ctx.solver(model, N, pat, CAP_DEFAULT)
    G, st = gpu_gains(s, V, up, tr, W_2L, kernel=KERNELS[kernel])
    r = gpu_vjp(s, V, up, tr, W_2L, Vbar)
    dV, dup, dtr, dw, dvb = (dev(a) for a in (np.full_like(V, 0.1), up, tr, W_2L, Vbar))
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    Gg, sg = f64(B, N, nu, nx + nu), torch.full((B,), -1, dtype=torch.int32, device="cuda")
    out = dict(x0_bar=f64(B, nx), u_prev_bar=f64(B, nu), traj_bar=f64(B, N, nx), weights_bar=f64(B, nx + 2 * nu),
               adj_V=f64(B, V.shape[1]), vjp_status=torch.full((B,), -1, dtype=torch.int32, device="cuda"),
               workspace=f64(s.solve_vjp_workspace_bytes(B) // 8))

    def launch(stream):
        s.feedback_gains(B, dV, dup, dtr, dw, G=Gg, gain_status=sg, kernel=KERNELS[kernel], stream=stream)
        s.solve_vjp(B, dV, dup, dtr, dw, dvb, stream=stream, **out)

    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):   # one launch on the capture stream before capturing (module load)
        launch(cs.cuda_stream)
    torch.cuda.current_stream().wait_stream(cs)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        launch(cs.cuda_stream)
    dV.copy_(dev(V))   # the graph reads the live buffers
    Gg.zero_()
    for k in OUT:
        out[k].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(Gg.cpu().numpy(), G) and np.array_equal(sg.cpu().numpy(), st)
    for k in OUT + ("vjp_status",):
        assert np.array_equal(out[k].cpu().numpy(), r[k]), k
    s.close()


# ---------------------------------------------------------------- 8. a handle without state bounds
def test_unbounded_handle_is_untouched_by_the_setting(ctx):
    model, pat, N, B = "two_link_arm", "mixed+u", 17, 37
    _, up, tr, Vbar = ctx.inputs(model, pat, N, B)
    _, _, ul, uu = ctx.bounds(model, pat)
    V = ctx.plan(model, pat, N, B)
    s = ctx.solver(model, N)
    res = []
    for on in (False, True):
        if on:
            s.set_sensitivity_barrier(1e-3, 10.0)
        res.append([gpu_gains(s, V, up, tr, W_2L, ul, uu, kernel=KERNELS[k]) for k in KERNELS]
                   + [gpu_vjp(s, V, up, tr, W_2L, Vbar, ul, uu)])
    s.close()
    for off, on in zip(res[0][:2], res[1][:2]):
        assert np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1])
    for k in OUT + ("vjp_status",):
        assert np.array_equal(res[0][2][k], res[1][2][k]), k


# ---------------------------------------------------------------- 9. autograd
def test_autograd_on_a_state_bounded_solver(ctx):
    import torch
    from mmpc.autograd import DifferentiableSolver
    model, pat, N, B = "two_link_arm", "box", 17, 5
    nx, nu = DIMS[model]
    m = ctx.m
    x0, up, tr, _ = ctx.inputs(model, pat, N, B)
    s = ctx.solver(model, N, pat, kkt_solver=m.KKT_RICCATI_GROUP, hessian=m.HESSIAN_EXACT, tol_grad=1e-11,
                   tol_defect=1e-12)
    ds = DifferentiableSolver(s)
    tx0, tw = dev(x0).requires_grad_(), dev(np.tile(W_2L, (B, 1))).requires_grad_()
    V, status, _ = ds(tx0, dev(up), dev(tr), tw)
    assert (status == 0).all()
    with pytest.raises(m.MmpcError, match="state bounds"):   # the barrier is off
        V[:, nx:nx + nu].sum().backward(retain_graph=True)
    s.set_sensitivity_barrier()
    V[:, nx:nx + nu].sum().backward()
    torch.cuda.synchronize()
    assert (ds.last_vjp_status == 0).all()
    gx, gq = tx0.grad.cpu().numpy(), tw.grad.cpu().numpy()[:, :nx]

    def u0_sum(xs, w):
        g = s.solve_batch_host(xs, up, tr, w)
        assert (g["status"] == 0).all(), g["status"]
        return g["V"][:, nx:nx + nu].sum(1)

    fx, fq = np.zeros_like(gx), np.zeros_like(gq)
    wrows = np.tile(W_2L, (B, 1))
    for i in range(nx):
        d = np.zeros(nx)
        d[i] = 1e-5
        fx[:, i] = (u0_sum(x0 + d, wrows) - u0_sum(x0 - d, wrows)) / 2e-5
        dq = np.zeros(nx + 2 * nu)
        dq[i] = 1e-5 * W_2L[i]   # relative to the weight's own size (fd_delta of sens_reference.py)
        fq[:, i] = (u0_sum(x0, wrows + dq) - u0_sum(x0, wrows - dq)) / (2 * dq[i])
    s.close()
    ex = (np.abs(fx - gx).max(1) / np.maximum(1.0, np.abs(gx).max(1))).max()
    eq = (np.abs(fq - gq).max(1) / np.maximum(1.0, np.abs(gq).max(1))).max()
    print(f"autograd against central differences of the solve: x0 {ex:.3e}, Q {eq:.3e}")
    assert max(ex, eq) <= 20 * FD


# ---------------------------------------------------------------- 10. the C++ mirror
def test_cpp_mirror_publishes_the_c_abi_gains_and_applies_them(mmpc_mod, tmp_path):
    exe = os.path.join(ROOT, "mahi-mpc_amd", "host", "bin", "state_limit_feedback_example")
    assert os.path.exists(exe), "build() makes the example"
    N, n, B, nx, nu = 17, 3, 5, 4, 2
    K = nx + nu
    model = str(tmp_path / "arm17_limits")
    mmpc_mod.write_model_json(model + ".json", "arm17_limits", nx, nu, 2000, N, model="two_link_arm",
                              x_min=[-10e30, -10e30, -0.5, -0.5], x_max=[10e30, 10e30, 0.5, 0.5])
    r = subprocess.run([exe, model, str(n)], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split(",") for l in r.stdout.splitlines()]
    rows = lambda tag: [l for l in lines if l[0] == tag]   # noqa: E731
    vec = lambda tag: np.array(rows(tag)[0][1:], dtype=float)   # noqa: E731
    delta = 1e-3 * np.array([1.0, -1.0, 1.0, -1.0])

    def corrected(u0, G0, x0):
        dx = (x0 + delta) - x0   # the measured state the example passes, minus x_est_0
        want = u0.copy()
        for j in range(nx):      # the mirror's own order of summation
            want += G0[:, j] * dx[j]
        return want

    assert int(rows("refused")[0][1]) == 1
    assert [int(v) for v in rows("status")[0][1:]] == [0, 0]
    g = rows("g")
    assert [int(row[1]) for row in g] == list(range(n))
    for row in g:
        pair = np.array(row[2:], dtype=float).reshape(2, nu, K)
        assert np.array_equal(pair[0], pair[1]), ("ModelControl against the C-ABI", row[1])
    G0 = np.array(g[0][2:], dtype=float).reshape(2, nu, K)[0]
    assert np.abs(G0[:, :nx]).max() > 0.1
    fb, want = vec("fb"), corrected(vec("u0"), G0, vec("x0"))
    assert np.abs(fb - want).max() <= 1e-15 * max(1.0, np.abs(want).max()), (fb, want)
    bg = rows("bg")
    assert len(bg) == B * n
    first = {}
    for row in bg:
        assert int(row[3]) == 0, row[:4]
        pair = np.array(row[4:], dtype=float).reshape(2, nu, K)
        assert np.array_equal(pair[0], pair[1]), ("BatchModelControl against the C-ABI", row[1:3])
        if int(row[2]) == 0:
            first[int(row[1])] = pair[0]
    bu = rows("bu")
    assert len(bu) == B
    for row in bu:
        v = np.array(row[2:], dtype=float)
        x0, u0, got = v[:nx], v[nx:nx + nu], v[nx + nu:]
        want = corrected(u0, first[int(row[1])], x0)
        assert np.abs(got - want).max() <= 1e-15 * max(1.0, np.abs(want).max()), (row[1], got, want)
