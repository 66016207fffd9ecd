"""GPU: feedback gains along the plan, G_k = d u_k* / d(x_k, u_{k-1}) (mmpc_feedback_gains_batch).

The reference (tests/sens_reference.py, numpy over oracle_lib's Jacobians and oracle_nlp_hess) is the DENSE sensitivity
of the tail problem, not a second Riccati recursion.  Tail problem from stage k: the stages k..N-1 of the NLP from x_k = x with
u_{k-1} = v.  Linearised at the plan, dx_{j+1} = A_j dx_j + B_j du_j, so every (dx_j, du_j) is linear in the parameters
p = (dx, dv) and the unknowns dU = (du_k .. du_{N-1}); the Lagrangian's Hessian in these variables is the sum of the
stage blocks (nlp_hess_l with the multipliers of tests/test_kkt_certificate.py::_certify, or their Gauss-Newton part)
and the constant -2R couplings of consecutive controls, the first of them between du_k and dv.  Held controls (on a
bound bit for bit, or k < n_pin) are removed from the unknowns.  dU = -H_UU^-1 H_Up; its first nu rows are G_k.

Inputs: oracle.synth(20250213, 0, B, N, 0.002), WEIGHTS_CFG and W_EXO; V* comes from the GPU solve.  Tolerance of every
comparison with the reference: max |G_k - G_ref,k| <= 1e-10 max(1, max |G_ref,k|) at every stage written, the project's
standing GPU-versus-oracle tolerance (the CPU floor of Riccati against dense is 1.5e-14).

1. parity per kernel (lane, 16-lane) and Hessian: 2-link (N, B) = (1, 5) (2, 3) (3, 9) (17, 37) (33, 65) -- N = 1 has no
   recursion, 17 and 33 are one stage past the rounds of 16, 5 and 37 leave a partial workgroup, 65 a partial wave --
   and the exo (1, 5) (7, 9) (21, 9); n_gain in {1, N} and 8 at N = 17; gain_status 0 everywhere.
2. control bounds: 2-link (3, 9) and (17, 37) under +-2 Nm, shared and as a [B, nu] table with a padded stride, the exo
   (7, 9) under test_gpu_bounded_shapes's box: held rows exactly 0, free rows at the tolerance, at least one held and
   one free control per case.
3. pins: n_pin = 2 at (17, 37): G_0 and G_1 exactly zero, G_2.. match the reference with those stages held.
4. Hessian selection: an explicit GAUSS_NEWTON matches the Gauss-Newton reference and differs from the exact gain by
   >= 1e-2 on the 2-link arm at N = 17.
5. derivative of the solver's own map: 2-link (17, 5), 16-lane solves with tol_grad 1e-11 and tol_defect 1e-12, central
   differences at delta = 1e-4 in each of the nx + nu directions, warm-started from V*, against the exact G_0 at
   1e-6 max(1, |G_0|) (the CPU value of the same experiment is 7.6e-9).
6. fallback: instance 0 gets its velocity targets moved by 1000 (1, -1): the dense reference's free H_UU then has an
   eigenvalue below -1e-3 of its largest (asserted here), so some pivot of the exact sweep is not positive: status 1
   and the Gauss-Newton reference's gains; the instance beside it keeps status 0 and the exact gains.
7. non-finite input: an instance with a NaN in V reports 2 with all-zero gains; its workgroup- and wave-mates are bit
   for bit those of the clean batch.
8. the host entry, B = 1, a captured-graph replay bit for bit the direct call, and determinism run to run."""
import os

import numpy as np
import pytest

import oracle_lib as oracle
from conftest import WEIGHTS_CFG
from sens_reference import gains, gains_batch, held_mask
from test_gpu_bounded_shapes import UB, W_EXO

pytestmark = pytest.mark.gpu

H = 0.002
SEED = 20250213
W_2L = np.array(WEIGHTS_CFG)
DIMS = {"two_link_arm": (4, 2), "exo_arm": (8, 4)}
OMODEL = {"two_link_arm": oracle.TWO_LINK, "exo_arm": oracle.EXO}
WEIGHTS = {"two_link_arm": W_2L, "exo_arm": W_EXO}
TOL = 1e-10




# ---------------------------------------------------------------- the cases
SHAPES = {"two_link_arm": [(1, 5), (2, 3), (3, 9), (17, 37), (33, 65)], "exo_arm": [(1, 5), (7, 9), (21, 9)]}
KERNELS = {"lane": 1, "group": 2}
PARITY = [(model, N, B, kernel, hess) for model, shapes in SHAPES.items() for (N, B) in shapes
          for kernel in KERNELS for hess in ("exact", "gn")]
PM2 = ([-2.0, -2.0], [2.0, 2.0])
BOUNDED = [("two_link_arm", 3, 9, "shared"), ("two_link_arm", 3, 9, "table"), ("two_link_arm", 17, 37, "shared"),
           ("two_link_arm", 17, 37, "table"), ("exo_arm", 7, 9, "shared")]


def _id(case):
    return "-".join(str(v) for v in case)


class Ctx:
    """the module's shared state: inputs, GPU plans and references, each computed once and left unchanged"""

    def __init__(self, m, d):
        self.m, self.dir = m, d
        self.inputs_, self.plans_, self.refs_ = {}, {}, {}

    def solver(self, model, N, **kw):
        nx, nu = DIMS[model]
        p = self.m.write_model_json(os.path.join(self.dir, f"{model}_{N}.json"), f"{model}_{N}", nx, nu, 2000, N,
                                    model=model)
        kw.setdefault("max_iter", 100)
        return self.m.Solver(p, **kw)

    def inputs(self, model, N, B):
        key = (model, N, B)
        if key not in self.inputs_:
            arrs = oracle.synth(SEED, 0, B, N, H, model=OMODEL[model])
            for a in arrs:
                a.setflags(write=False)
            self.inputs_[key] = arrs
        return self.inputs_[key]

    def bounds(self, model, bounded):
        """(lb, ub) [nu] of a case, or (None, None)"""
        if not bounded:
            return None, None
        lb, ub = PM2 if model == "two_link_arm" else UB["exo_arm"]["box"]
        return np.array(lb, dtype=np.float64), np.array(ub, dtype=np.float64)

    def plan(self, model, N, B, bounded=False):
        """V* of the GPU solve [B, NV]"""
        key = (model, N, B, bounded)
        if key not in self.plans_:
            x0, up, tr = self.inputs(model, N, B)
            lb, ub = self.bounds(model, bounded)
            s = self.solver(model, N)
            g = s.solve_batch_host(x0, up, tr, WEIGHTS[model], u_lb=lb, u_ub=ub)
            s.close()
            assert (g["status"] == 0).all(), g["status"]
            g["V"].setflags(write=False)
            self.plans_[key] = g["V"]
        return self.plans_[key]

    def ref(self, model, N, B, exact, bounded=False, n_pin=0):
        """the dense reference at the plan, every stage: [B, N, nu, nx + nu]"""
        key = (model, N, B, exact, bounded, n_pin)
        if key not in self.refs_:
            _, up, tr = self.inputs(model, N, B)
            lb, ub = self.bounds(model, bounded)
            G = gains_batch(OMODEL[model], N, H, self.plan(model, N, B, bounded), up, tr, WEIGHTS[model], exact, lb, ub,
                            n_pin)
            G.setflags(write=False)
            self.refs_[key] = G
        return self.refs_[key]


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return Ctx(mmpc_mod, str(tmp_path_factory.mktemp("feedback_gains")))


def dev(a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def gpu_gains(s, V, up, tr, w, lb=None, ub=None, bounds_stride=0, **kw):
    """one device-pointer gain call on fresh tensors: (G, gain_status) as numpy"""
    import torch
    B = V.shape[0]
    args = [dev(a) for a in (V, up, tr, w)]
    dl, du = dev(lb), dev(ub)
    G, st = s.feedback_gains(B, *args, u_lb=dl, u_ub=du, bounds_stride=bounds_stride, **kw)
    torch.cuda.synchronize()
    return G.cpu().numpy(), st.cpu().numpy()


def check(G, Gref, what=""):
    """G, Gref [B, n, nu, K]: the tolerance at every stage written"""
    assert G.shape == Gref.shape, (G.shape, Gref.shape)
    err = np.abs(G - Gref).max(axis=(2, 3))
    bound = TOL * np.maximum(1.0, np.abs(Gref).max(axis=(2, 3)))
    worst = (err / bound).max() if err.size else 0.0
    print(f"{what}: max |G - G_ref| = {err.max():.3e}, worst err / bound = {worst:.3e}")
    assert np.isfinite(G).all() and (err <= bound).all(), (what, err.max(), np.argwhere(err > bound)[:5])


def hess_id(m, hess):
    return m.HESSIAN_EXACT if hess == "exact" else m.HESSIAN_GAUSS_NEWTON


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", PARITY, ids=_id)
def test_gains_match_the_dense_reference(case, ctx):
    model, N, B, kernel, hess = case
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    ref = ctx.ref(model, N, B, hess == "exact")
    s = ctx.solver(model, N)
    for n_gain in sorted({1, N} | ({8} if N == 17 else set())):
        G, st = gpu_gains(s, V, up, tr, WEIGHTS[model], n_gain=n_gain, hessian=hess_id(ctx.m, hess),
                          kernel=KERNELS[kernel])
        assert (st == 0).all(), st
        check(G, ref[:, :n_gain], f"{_id(case)} n_gain={n_gain}")
    s.close()


# ---------------------------------------------------------------- 2. control bounds
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", BOUNDED, ids=_id)
def test_held_rows_are_zero_and_free_rows_match(case, kernel, ctx):
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
        ref = ctx.ref(model, N, B, hess == "exact", True)
        if form == "shared":
            G, st = gpu_gains(s, V, up, tr, WEIGHTS[model], lb, ub, hessian=hess_id(ctx.m, hess), kernel=KERNELS[kernel])
        else:   # a row per instance at a padded stride, NaN in the padding, buffers of the exact size
            stride = nu + 3
            tl = np.full((B - 1) * stride + nu, np.nan)
            tu = np.full((B - 1) * stride + nu, np.nan)
            for b in range(B):
                tl[b * stride:b * stride + nu], tu[b * stride:b * stride + nu] = lb, ub
            G, st = gpu_gains(s, V, up, tr, WEIGHTS[model], tl, tu, stride, hessian=hess_id(ctx.m, hess),
                              kernel=KERNELS[kernel])
        assert (st == 0).all(), st
        assert (G[held] == 0.0).all(), "a held control's row of G_k must be exactly 0"
        assert (ref[held] == 0.0).all()
        check(G, ref, f"{_id(case)} {kernel} {hess}")
    s.close()


# ---------------------------------------------------------------- 3. pins
@pytest.mark.parametrize("kernel", KERNELS)
def test_pinned_stages_have_zero_gains(kernel, ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    ref = ctx.ref(model, N, B, True, n_pin=2)
    s = ctx.solver(model, N)
    G, st = gpu_gains(s, V, up, tr, W_2L, n_pin=2, kernel=KERNELS[kernel])
    s.close()
    assert (st == 0).all(), st
    assert (G[:, :2] == 0.0).all() and (ref[:, :2] == 0.0).all()
    assert np.abs(G[:, 2:]).max() > 0.1
    check(G, ref, f"pins {kernel}")


# ---------------------------------------------------------------- 4. Hessian selection
@pytest.mark.parametrize("kernel", KERNELS)
def test_gauss_newton_is_the_other_gain(kernel, ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    s = ctx.solver(model, N)
    Gn, st = gpu_gains(s, V, up, tr, W_2L, hessian=ctx.m.HESSIAN_GAUSS_NEWTON, kernel=KERNELS[kernel])
    Ga, sta = gpu_gains(s, V, up, tr, W_2L, hessian=ctx.m.HESSIAN_AUTO, kernel=KERNELS[kernel])
    s.close()
    assert (st == 0).all() and (sta == 0).all()
    check(Gn, ctx.ref(model, N, B, False), f"explicit Gauss-Newton {kernel}")
    check(Ga, ctx.ref(model, N, B, True), f"AUTO is exact {kernel}")
    gap = np.abs(Gn - Ga).max()
    print(f"exact against Gauss-Newton gain: {gap:.3e}")
    assert gap >= 1e-2


# ---------------------------------------------------------------- 5. derivative of the solver's own map
def test_exact_gain_is_the_derivative_of_the_solve(ctx):
    model, N, B, delta = "two_link_arm", 17, 5, 1e-4
    nx, nu = DIMS[model]
    m = ctx.m
    x0, up, tr = ctx.inputs(model, N, B)
    s = ctx.solver(model, N, kkt_solver=m.KKT_RICCATI_GROUP, tol_grad=1e-11, tol_defect=1e-12)
    assert s.hessian_for(B) == m.HESSIAN_EXACT
    g = s.solve_batch_host(x0, up, tr, W_2L)
    assert (g["status"] == 0).all()
    V = g["V"]
    G0, st = s.feedback_gains_host(V, up, tr, W_2L, n_gain=1, hessian=m.HESSIAN_EXACT)
    assert (st == 0).all()
    G0 = G0[:, 0]
    fd = np.zeros_like(G0)
    for i in range(nx + nu):
        u0 = []
        for sign in (1.0, -1.0):
            xs, us = x0.copy(), up.copy()
            (xs if i < nx else us)[:, i if i < nx else i - nx] += sign * delta
            r = s.solve_batch_host(xs, us, tr, W_2L, V=V)
            assert (r["status"] == 0).all(), r["status"]
            u0.append(r["V"][:, nx:nx + nu])
        fd[:, :, i] = (u0[0] - u0[1]) / (2 * delta)
    s.close()
    err = np.abs(fd - G0).max(axis=(1, 2))
    bound = 1e-6 * np.maximum(1.0, np.abs(G0).max(axis=(1, 2)))
    print(f"central differences of the solve against G_0: max {err.max():.3e} (bound {bound.min():.1e})")
    assert (err <= bound).all(), (err, bound)


# ---------------------------------------------------------------- 6. fallback
@pytest.mark.parametrize("kernel", KERNELS)
def test_indefinite_exact_model_falls_back_to_gauss_newton(kernel, ctx):
    model, N, B = "two_link_arm", 17, 2
    om = OMODEL[model]
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    tr2 = tr.copy()   # V is no solution for these targets: velocity targets of instance 0 moved by 1000 (1, -1)
    tr2[0, :, 2] += 1000.0
    tr2[0, :, 3] -= 1000.0
    ratios = []
    gains(om, N, H, V[0], up[0], tr2[0], W_2L, True, min_eig=ratios)
    print(f"smallest eigenvalue of H_UU over its largest, worst stage: {min(ratios):.3e}")
    assert min(ratios) < -1e-3
    s = ctx.solver(model, N)
    G, st = gpu_gains(s, V, up, tr2, W_2L, hessian=ctx.m.HESSIAN_EXACT, kernel=KERNELS[kernel])
    s.close()
    assert st.tolist() == [1, 0], st
    check(G[:1], gains_batch(om, N, H, V[:1], up[:1], tr2[:1], W_2L, False), f"fallback instance {kernel}")
    check(G[1:], gains_batch(om, N, H, V[1:], up[1:], tr2[1:], W_2L, True), f"its neighbour {kernel}")


# ---------------------------------------------------------------- 7. non-finite input
@pytest.mark.parametrize("where", ["state", "x_N"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_nan_instance_fails_alone(kernel, where, ctx):
    model, N, B, bad = "two_link_arm", 17, 37, 5
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    s = ctx.solver(model, N)
    G, st = gpu_gains(s, V, up, tr, W_2L, kernel=KERNELS[kernel])
    V2 = V.copy()
    V2[bad, 3 * 6 + 1 if where == "state" else V.shape[1] - 1] = np.nan
    G2, st2 = gpu_gains(s, V2, up, tr, W_2L, kernel=KERNELS[kernel])
    s.close()
    assert (st == 0).all()
    assert st2[bad] == 2 and (G2[bad] == 0.0).all()
    others = np.arange(B) != bad
    assert (st2[others] == 0).all()
    assert np.array_equal(G2[others], G[others]), "the neighbours of a failed instance must not change"


# ---------------------------------------------------------------- 8. remaining paths
@pytest.mark.parametrize("kernel", KERNELS)
def test_host_entry_single_instance_and_determinism(kernel, ctx):
    model, N, B = "two_link_arm", 17, 37
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    ref = ctx.ref(model, N, B, True)
    s = ctx.solver(model, N)
    G, st = gpu_gains(s, V, up, tr, W_2L, kernel=KERNELS[kernel])
    Gr, str_ = gpu_gains(s, V, up, tr, W_2L, kernel=KERNELS[kernel])
    assert np.array_equal(G, Gr) and np.array_equal(st, str_), "run to run"
    Gh, sth = s.feedback_gains_host(V, up, tr, W_2L, kernel=KERNELS[kernel])
    assert np.array_equal(Gh, G) and np.array_equal(sth, st), "host entry against the device entry"
    G1, st1 = s.feedback_gains_host(V[3:4], up[3:4], tr[3:4], W_2L, n_gain=8, kernel=KERNELS[kernel])
    assert st1.tolist() == [0]
    check(G1, ref[3:4, :8], f"B = 1 {kernel}")
    Ga, sta = s.feedback_gains_host(V, up, tr, W_2L)   # AUTO picks a kernel by B
    assert (sta == 0).all()
    check(Ga, ref, "AUTO kernel")
    s.close()


@pytest.mark.parametrize("kernel", KERNELS)
def test_gain_launch_replays_from_a_graph(kernel, ctx):
    import torch
    model, N, B = "two_link_arm", 17, 37
    nx, nu = DIMS[model]
    _, up, tr = ctx.inputs(model, N, B)
    V = ctx.plan(model, N, B)
    s = ctx.solver(model, N)
    G, st = gpu_gains(s, V, up, tr, W_2L, kernel=KERNELS[kernel])
    dV, dup, dtr, dw = (dev(a) for a in (np.zeros_like(V), up, tr, W_2L))
    Gg = torch.zeros((B, N, nu, nx + nu), dtype=torch.float64, device="cuda")
    sg = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):   # one launch on the capture stream before capturing (module load)
        s.feedback_gains(B, dV, dup, dtr, dw, G=Gg, gain_status=sg, kernel=KERNELS[kernel], stream=cs.cuda_stream)
    torch.cuda.current_stream().wait_stream(cs)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        s.feedback_gains(B, dV, dup, dtr, dw, G=Gg, gain_status=sg, kernel=KERNELS[kernel], stream=cs.cuda_stream)
    dV.copy_(dev(V))   # the graph reads the live buffers
    Gg.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(Gg.cpu().numpy(), G) and np.array_equal(sg.cpu().numpy(), st)
    s.close()
