"""GPU: the first iteration's switching condition where it can decide (csrc/sqp_wave.h first_iter_switch).

The two powers of IPOPT's switching condition alpha (-dJ)^2.3 > theta_0^1.1 are formed behind a branch that only a lane
with a nearly feasible first iterate and a descent step takes, once in front of the search loop, in the 16-lane and the
condensed kernel; the lane kernel keeps the one-expression form.  In all three the condition is READ only by a
first-iteration trial of such a lane whose Armijo test failed.

* the decision itself: the converged plan as the start of a solve whose targets are 100 (N = 17) or 40 (N = 30) times
  further away.  theta_0 is at roundoff (asserted <= 1e-4 through oracle.nlp_eval), dJ is large and negative, and
  the Armijo test fails at alpha = 1 -- asserted from the solver's own trace, alpha < 1 in iteration 0 on every instance -- so the filter is
  asked with the precondition true, the switching condition holds, it refuses, and the search backtracks (an f-type
  iteration).  A wrong exponent, swapped powers or a reversed comparison accepts the full step there and leaves the
  oracle's iterates.  N = 17 and 30, B = 1, 4 and 7, exact and Gauss-Newton Hessian, kkt_solver 3, 2 and 1 (the
  condensed kernel has no exact Hessian), the whole solve and max_iter = 1.  (Horizons and factors: the merit has to
  be nonlinear enough along the step for the Armijo test to fail.  At N = 5, 10 ms of motion, the full step is
  accepted at every factor up to 1000; at N = 17 and a factor of 40 one Gauss-Newton instance of seven still accepts
  it, at 100 none does and the oracle converges in at most 41 iterations; at N = 30 a factor of 40 is enough);
* one wave in which only instances 0 and 2 reach the decision (1 and 3 accept alpha = 1 by the Armijo test): every
  instance's bytes are the bytes of that instance solved alone;
* warm starts as in tests/test_gpu_parity.py test_warm_start_perturbed_state: the converged plan with x_0 moved by at
  most 1e-7, theta_0 <= 1e-4 asserted; the precondition holds (the 16-lane and condensed kernels form the powers), the
  Armijo test accepts and nothing reads them; N = 5 and 17, B = 1, 4 and 7, the whole solve and max_iter = 1;
* cold starts at the same shapes (the precondition fails);
* one wave that holds warm and cold instances: every instance's bytes are the bytes of that instance solved alone.

Every oracle comparison: the oracle's status and iteration counts on every instance, V within 1e-10 relative to max|V|
(tests/test_gpu_group_sweep_shapes.py: the same algorithm on both sides)."""
import ctypes as C

import numpy as np
import pytest

from conftest import WEIGHTS_CFG
from test_gpu_group_sweep_shapes import H, SEED, _oracle_hess, _same_as_oracle

pytestmark = pytest.mark.gpu

BMAX = 7
# (kkt_solver, hessian): the condensed kernel (1) is Gauss-Newton only
VARIANTS = [(3, "exact"), (3, "gn"), (2, "exact"), (2, "gn"), (1, "gn")]


def _w():
    return np.array(WEIGHTS_CFG)


def _solver(m, model_json, N, kkt, hess, **kw):
    h = m.HESSIAN_EXACT if hess == "exact" else m.HESSIAN_GAUSS_NEWTON
    s = m.Solver(model_json(N=N), kkt_solver=kkt, hessian=h, **kw)
    return s


def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def starts(oracle):
    """per (N, hess) at B = 7, computed once: inputs, the warm-start plan (theta_0 <= 1e-4 asserted) and the oracle's
    solutions of the warm and the cold start, whole and with max_iter = 1; smaller batches are the leading rows"""
    memo = {}

    def get(N, hess):
        if (N, hess) in memo:
            return memo[(N, hess)]
        oh = _oracle_hess(oracle, hess)
        x0, up, tr = oracle.synth(SEED, 300, BMAX, N, H)
        first = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=oh)
        assert (first["status"] == 0).all(), first["status"]
        x0p = x0 + np.random.default_rng(5).uniform(-1e-7, 1e-7, x0.shape)
        Vw = first["V"].copy()
        Vw[:, :4] = x0p
        for b in range(BMAX):   # nearly feasible: the switching condition is what the first iteration tests
            _, c0 = oracle.nlp_eval(N, H, Vw[b], up[b], tr[b], _w())
            theta0 = np.abs(c0).sum()
            assert 0.0 < theta0 <= 1e-4, theta0
        d = dict(x0=x0p, up=up, tr=tr, Vw=Vw)
        for name, V in (("warm", Vw), ("cold", None)):
            for mi in (200, 1):
                o = oracle.solve_batch(N, H, x0p, up, tr, _w(), V=None if V is None else V.copy(), hessian=oh,
                                       max_iter=mi)
                _freeze(*o.values())
                d[(name, mi)] = o
        assert (d[("warm", 200)]["status"] == 0).all() and (d[("cold", 200)]["status"] == 0).all()
        assert (d[("warm", 200)]["iters"] >= 1).all()          # the moved x_0 costs at least one iteration
        assert (d[("cold", 200)]["iters"] > d[("warm", 200)]["iters"]).any()
        _freeze(*d.values())
        memo[(N, hess)] = d
        return d
    return get


def _rows(o, B):
    return {k: o[k][:B] for k in ("V", "status", "iters")}


def _c(a, B):
    return np.ascontiguousarray(a[:B])


@pytest.mark.parametrize("kkt,hess", VARIANTS)
@pytest.mark.parametrize("B", [1, 4, 7])
@pytest.mark.parametrize("N", [5, 17])
@pytest.mark.parametrize("start", ["warm", "cold"])
def test_first_iteration_vs_oracle(start, N, B, kkt, hess, starts, model_json, mmpc_mod):
    d = starts(N, hess)
    V0 = _c(d["Vw"], B).copy() if start == "warm" else None
    for mi in (200, 1):
        s = _solver(mmpc_mod, model_json, N, kkt, hess, max_iter=mi)
        assert s.kkt_solver_for(B) == kkt
        g = s.solve_batch_host(_c(d["x0"], B), _c(d["up"], B), _c(d["tr"], B), _w(),
                               V=None if V0 is None else V0.copy())
        s.close()
        _same_as_oracle(g, _rows(d[(start, mi)], B), f"{start} N={N} B={B} kkt={kkt} {hess} max_iter={mi}")


@pytest.mark.parametrize("kkt,hess", [v for v in VARIANTS if v[0] != 1])
@pytest.mark.parametrize("N", [5, 17])
def test_warm_and_cold_instances_in_one_wave(N, kkt, hess, starts, model_json, mmpc_mod):
    """instances 0 and 2 start warm, 1 and 3 cold (a zero plan): the groups (16-lane kernel) or lanes (lane kernel) of
    one wave disagree on the branch; each instance is then solved alone from the same start"""
    d = starts(N, hess)
    B = 4
    V0 = _c(d["Vw"], B).copy()
    V0[1::2] = 0.0
    s = _solver(mmpc_mod, model_json, N, kkt, hess)
    x0, up, tr = _c(d["x0"], B), _c(d["up"], B), _c(d["tr"], B)
    g = s.solve_batch_host(x0, up, tr, _w(), V=V0.copy())
    assert (g["status"] == 0).all(), g["status"]
    for b in range(B):
        a = s.solve_batch_host(x0[b:b + 1], up[b:b + 1], tr[b:b + 1], _w(), V=V0[b:b + 1].copy())
        assert a["V"][0].tobytes() == g["V"][b].tobytes(), (N, kkt, hess, b)
        assert a["status"][0] == g["status"][b] and a["iters"][0] == g["iters"][b], (N, kkt, hess, b)
    s.close()
    # the warm ones are the oracle's warm solves, the cold ones its cold solves
    for b in range(B):
        o = d[("warm" if b % 2 == 0 else "cold", 200)]
        _same_as_oracle({k: g[k][b:b + 1] for k in ("V", "status", "iters")},
                        {k: o[k][b:b + 1] for k in ("V", "status", "iters")},
                        f"mixed wave N={N} kkt={kkt} {hess} b={b}")


# ---------------------------------------------------------------------------------------------- the decision itself
TARGET_SCALE = {17: 100.0, 30: 40.0}   # per horizon: every instance's Armijo test fails at alpha = 1 (module docstring)


@pytest.fixture(scope="module")
def far_targets(oracle):
    """per (N, hess) at B = 7, computed once: the converged plan of the synthetic instances as the start of a solve
    towards targets TARGET_SCALE[N] times further away, and the oracle's solutions, whole and with max_iter = 1"""
    memo = {}

    def get(N, hess):
        if (N, hess) in memo:
            return memo[(N, hess)]
        oh = _oracle_hess(oracle, hess)
        x0, up, tr = oracle.synth(SEED, 300, BMAX, N, H)
        first = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=oh)
        assert (first["status"] == 0).all(), first["status"]
        Vw = first["V"].copy()
        far = np.ascontiguousarray(tr * TARGET_SCALE[N])
        for b in range(BMAX):
            _, c0 = oracle.nlp_eval(N, H, Vw[b], up[b], far[b], _w())
            assert np.abs(c0).sum() <= 1e-4      # theta_0 <= theta_min: the precondition's first half
        d = dict(x0=x0, up=up, tr=tr, far=far, Vw=Vw)
        for mi in (200, 1):
            o = oracle.solve_batch(N, H, x0, up, far, _w(), V=Vw.copy(), hessian=oh, max_iter=mi)
            _freeze(*o.values())
            d[mi] = o
        assert (d[200]["status"] == 0).all(), d[200]["status"]
        assert (d[200]["iters"] >= 2).all()
        _freeze(*d.values())
        memo[(N, hess)] = d
        return d
    return get


def _trace_solve(s, kkt, x0, up, tr, w, V0, max_iter):
    """the solve through mmpc_debug_solve_trace: (result dict, alpha accepted in iteration 0 per instance)"""
    import torch
    B = x0.shape[0]
    f64 = dict(dtype=torch.float64, device="cuda")
    t = [torch.tensor(np.ascontiguousarray(a), **f64) for a in (x0, up, tr, w)]
    V = torch.tensor(np.ascontiguousarray(V0), **f64)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    kk = torch.zeros(B, **f64)
    trace = torch.zeros((B, max_iter + 1, 8), **f64)
    L = s._L
    L.mmpc_debug_solve_trace.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 6
    rc = L.mmpc_debug_solve_trace(s._h, B, *(a.data_ptr() for a in t), 0, V.data_ptr(), st.data_ptr(), it.data_ptr(),
                                  kk.data_ptr(), trace.data_ptr(), None)
    assert rc == 0, L.mmpc_last_error()
    torch.cuda.synchronize()
    col = 2 if kkt == 1 else 5      # the condensed kernel's trace keeps alpha in column 2, the Riccati kernels' in 5
    g = {"V": V.cpu().numpy(), "status": st.cpu().numpy(), "iters": it.cpu().numpy()}
    return g, trace[:, 0, col].cpu().numpy()


@pytest.mark.parametrize("kkt,hess", VARIANTS)
@pytest.mark.parametrize("B", [1, 4, 7])
@pytest.mark.parametrize("N", [17, 30])
def test_switching_condition_refuses_the_full_step(N, B, kkt, hess, far_targets, model_json, mmpc_mod):
    d = far_targets(N, hess)
    x0, up, far, V0 = _c(d["x0"], B), _c(d["up"], B), _c(d["far"], B), _c(d["Vw"], B)
    for mi in (200, 1):
        s = _solver(mmpc_mod, model_json, N, kkt, hess, max_iter=mi)
        assert s.kkt_solver_for(B) == kkt
        g = s.solve_batch_host(x0, up, far, _w(), V=V0.copy())
        gt, alpha0 = _trace_solve(s, kkt, x0, up, far, _w(), V0, mi)
        s.close()
        print(f"N={N} B={B} kkt={kkt} {hess} max_iter={mi}: alpha of iteration 0 {alpha0.tolist()}")
        # the Armijo test failed at alpha = 1, so the filter was asked and the switching condition decided
        assert ((alpha0 > 0.0) & (alpha0 < 1.0)).all(), alpha0
        # the traced solve is the solve: the same bytes -- except in the lane kernel, whose launch hands the instances
        # that iterate longest to a 16-lane launch and does not when it writes a trace; both are held to the oracle
        if kkt != mmpc_mod.KKT_RICCATI:
            assert gt["V"].tobytes() == g["V"].tobytes() and np.array_equal(gt["iters"], g["iters"])
        else:
            _same_as_oracle(gt, _rows(d[mi], B), f"far targets, traced, N={N} B={B} kkt={kkt} {hess} max_iter={mi}")
        _same_as_oracle(g, _rows(d[mi], B), f"far targets N={N} B={B} kkt={kkt} {hess} max_iter={mi}")


@pytest.mark.parametrize("kkt,hess", [v for v in VARIANTS if v[0] != 1])
@pytest.mark.parametrize("N", [17, 30])
def test_decision_in_some_instances_of_a_wave(N, kkt, hess, far_targets, model_json, mmpc_mod, oracle):
    """instances 0 and 2 head for the far targets (the filter is asked and refuses), 1 and 3 for their own targets from
    the same plan with x_0 moved by <= 1e-7 (the Armijo test accepts alpha = 1): the groups (16-lane kernel) or lanes
    (lane kernel) of one wave disagree at the decision; each instance is then solved alone (traced like the wave, so
    that the lane kernel takes the same launch path both times)"""
    d = far_targets(N, hess)
    B = 4
    x0, up, V0 = _c(d["x0"], B).copy(), _c(d["up"], B), _c(d["Vw"], B).copy()
    tr = _c(d["far"], B).copy()
    tr[1::2] = d["tr"][1:B:2]
    x0[1::2] += np.random.default_rng(5).uniform(-1e-7, 1e-7, x0[1::2].shape)
    V0[1::2, :4] = x0[1::2]
    s = _solver(mmpc_mod, model_json, N, kkt, hess)
    g, alpha0 = _trace_solve(s, kkt, x0, up, tr, _w(), V0, 200)
    print(f"N={N} kkt={kkt} {hess}: alpha of iteration 0 {alpha0.tolist()}")
    assert (alpha0[0::2] < 1.0).all() and (alpha0[1::2] == 1.0).all(), alpha0
    assert (g["status"] == 0).all(), g["status"]
    for b in range(B):
        a, _ = _trace_solve(s, kkt, x0[b:b + 1], up[b:b + 1], tr[b:b + 1], _w(), V0[b:b + 1], 200)
        assert a["V"][0].tobytes() == g["V"][b].tobytes(), (N, kkt, hess, b)
        assert a["status"][0] == g["status"][b] and a["iters"][0] == g["iters"][b], (N, kkt, hess, b)
    s.close()
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), V=V0.copy(), hessian=_oracle_hess(oracle, hess))
    _same_as_oracle(g, o, f"decision in instances 0 and 2, N={N} kkt={kkt} {hess}")
