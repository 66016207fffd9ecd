"""GPU: the parts of a 16-lane kernel iteration outside the serial sweeps -- the group reductions, the accepted full
step and the prologue (csrc/sqp_group.h).

Reductions: group_sum / group_max / group_min are butterflies of DPP row rotations inside the 16-lane row of one
instance.  The variants that run the most of them per iteration (control bounds, state bounds, Mehrotra's rule,
per-instance bounds) at N = 5 and 17 in partly filled waves (B = 1, 3, 5), the exo kernels at N = 3, and one instance
alone and as group 0 .. 3 of a wave among different neighbours (same bytes: a row operation never sees another group).

Line search and update: the fused alpha = 1 trial of the unbounded 2-link kernels and the update pass after it form
the same iterate; a trial that stores it in place (tried and measured) has to get the cross-lane reads
x_{k+1}, u_{k-1} right at the round boundaries, x_N, and put the old iterate back after a rejected step.  These cases
pin what any such change must keep: horizons 1, 2, 16, 17, 32, 33 (one round, a full round, each round boundary,
x_N); a non-zero start; max_iter = 1 and 2 (the iterate written back is the oracle's at that point); and rejected full
steps, where the alpha / 2 trials go on from the old iterate.

Prologue: the three init_states modes at N = 1, 17, 33, per-instance weights, and an exo lane-kernel batch that hands
its tail to the 16-lane resume launch.

Every oracle comparison uses the criterion of tests/test_gpu_group_sweep_shapes.py: identical status and iteration
counts on every instance, V within 1e-10 relative to max|V| (same algorithm on both sides)."""
import ctypes as C

import numpy as np
import pytest

from conftest import WEIGHTS_CFG
from test_gpu_group_sweep_shapes import H, INF, SEED, W_EXO, _oracle_hess, _same_as_oracle, _two_link

pytestmark = pytest.mark.gpu

VEL = (np.array([-INF, -INF, -1.5, -1.5]), np.array([INF, INF, 1.5, 1.5]))
UB = (np.array([-2.0, -2.0]), np.array([2.0, 2.0]))


def _w():
    return np.array(WEIGHTS_CFG)


# ---------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N", [5, 17])
def test_control_bounds_partly_filled_wave(N, B, model_json, mmpc_mod, oracle):
    s = mmpc_mod.Solver(model_json(N=N), kkt_solver=mmpc_mod.KKT_RICCATI_GROUP)
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    g = s.solve_batch_host(x0, up, tr, _w(), u_lb=UB[0], u_ub=UB[1])
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), u_lb=UB[0], u_ub=UB[1], solver=s)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"control bounds N={N} B={B}")


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N", [5, 17])
def test_state_bounds_partly_filled_wave(N, B, model_json, mmpc_mod, oracle):
    xl, xu = VEL
    s = mmpc_mod.Solver(model_json(N=N), max_iter=100, kkt_solver=mmpc_mod.KKT_RICCATI_GROUP)
    s.set_state_bounds(xl, xu)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    g = s.solve_batch_host(x0, up, tr, _w())
    hess = {1: oracle.HESS_GAUSS_NEWTON, 2: oracle.HESS_EXACT}[s.hessian_for(B, False)]
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), x_lb=xl, x_ub=xu, max_iter=100, hessian=hess)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"state bounds N={N} B={B}")


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N", [5, 17])
def test_mehrotra_partly_filled_wave(N, B, model_json, mmpc_mod, oracle):
    """the rule and the inputs of tests/test_gpu_barrier_rule.py (small shapes)"""
    m = mmpc_mod
    xl, xu = VEL
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    x0[:, 2:] = np.clip(x0[:, 2:], -1.4, 1.4)
    s = m.Solver(model_json(N=N), max_iter=100, kkt_solver=m.KKT_RICCATI_GROUP, hessian=None,
                 barrier_rule=m.BARRIER_MEHROTRA)
    s.set_state_bounds(xl, xu)
    g = s.solve_batch_host(x0, up, tr, _w())
    try:
        oracle.set_ip_rule(1)
        o = oracle.solve_batch(N, H, x0, up, tr, _w(), x_lb=xl, x_ub=xu, max_iter=100)
    finally:
        oracle.set_ip_rule(0)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"Mehrotra N={N} B={B}")


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N", [5, 17])
def test_per_instance_bounds_partly_filled_wave(N, B, model_json, mmpc_mod, oracle):
    """[B, nu] bounds, one row per instance, against one oracle solve per instance with that instance's bounds and the
    16-lane kernel's hold-release rule (as tests/test_gpu_group_vector_sweeps.py)"""
    m = mmpc_mod
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    c = np.array([1.0, 1.5, 2.0, 3.0, INF])[:B]
    lb, ub = -np.stack([c, 0.5 * c], 1), np.stack([0.75 * c, c], 1)
    s = m.Solver(model_json(N=N), kkt_solver=m.KKT_RICCATI_GROUP, hessian=m.HESSIAN_GAUSS_NEWTON)
    assert s.kkt_solver_for(B) == m.KKT_RICCATI_GROUP
    g = s.solve_batch_host(x0, up, tr, _w(), u_lb=lb, u_ub=ub)
    s.close()
    res = [oracle.solve_batch(N, H, x0[b:b + 1], up[b:b + 1], tr[b:b + 1], _w(), u_lb=lb[b], u_ub=ub[b],
                              hessian=oracle.HESS_GAUSS_NEWTON, bound_release=True) for b in range(B)]
    o = {k: np.concatenate([r[k] for r in res]) for k in ("V", "status", "iters")}
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"per-instance bounds N={N} B={B}")


@pytest.mark.parametrize("variant", ["exact", "gn", "u-bounds"])
def test_exo_short_horizon(variant, mmpc_mod, oracle, tmp_path):
    N, B = 3, 5
    p = mmpc_mod.write_model_json(str(tmp_path / f"exo_{N}.json"), "exo_arm", 8, 4, 2000, N, model="exo_arm")
    h = mmpc_mod.HESSIAN_EXACT if variant == "exact" else mmpc_mod.HESSIAN_GAUSS_NEWTON
    s = mmpc_mod.Solver(p, kkt_solver=mmpc_mod.KKT_RICCATI_GROUP, hessian=h)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H, model=oracle.EXO)
    if variant == "u-bounds":
        lb, ub = np.full(4, -0.5), np.full(4, 0.5)
        g = s.solve_batch_host(x0, up, tr, W_EXO, u_lb=lb, u_ub=ub)
        o = oracle.solve_batch(N, H, x0, up, tr, W_EXO, model=oracle.EXO, u_lb=lb, u_ub=ub, solver=s)
    else:
        g = s.solve_batch_host(x0, up, tr, W_EXO)
        o = oracle.solve_batch(N, H, x0, up, tr, W_EXO, model=oracle.EXO, hessian=_oracle_hess(oracle, variant))
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"exo N={N} {variant}")


@pytest.mark.parametrize("variant", ["exact", "u-bounds", "x-bounds"])
def test_placement_in_the_wave(variant, model_json, mmpc_mod, oracle):
    """instance 0 of the batch alone, then as group 0, 1, 2, 3 of one wave with three other instances around it (a
    different set for every place): V, status and iteration count of the instance are the same bytes every time"""
    m, N = mmpc_mod, 17
    x0, up, tr = oracle.synth(SEED, 0, 16, N, H)
    kw = {}
    if variant == "exact":
        s = _two_link(m, model_json, N, variant)
    else:
        s = m.Solver(model_json(N=N), max_iter=100, kkt_solver=m.KKT_RICCATI_GROUP)
        if variant == "u-bounds":
            kw = dict(u_lb=UB[0], u_ub=UB[1])
        else:
            s.set_state_bounds(*VEL)
    alone = s.solve_batch_host(x0[:1], up[:1], tr[:1], _w(), **kw)
    assert alone["status"][0] == 0
    for place in range(4):
        others = [1 + 3 * place + j for j in range(3)]
        idx = others[:place] + [0] + others[place:]
        g = s.solve_batch_host(np.ascontiguousarray(x0[idx]), np.ascontiguousarray(up[idx]),
                               np.ascontiguousarray(tr[idx]), _w(), **kw)
        assert g["V"][place].tobytes() == alone["V"][0].tobytes(), (variant, place)
        assert g["status"][place] == alone["status"][0] and g["iters"][place] == alone["iters"][0], (variant, place)
    s.close()


# ---------------------------------------------------------------------------------------------- line search, update
@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N", [1, 2, 16, 17, 32, 33])
def test_round_boundaries_vs_oracle(N, hess, model_json, mmpc_mod, oracle):
    B = 5
    s = _two_link(mmpc_mod, model_json, N, hess)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    g = s.solve_batch_host(x0, up, tr, _w())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=_oracle_hess(oracle, hess))
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"N={N} {hess}")


def _seeded_V(B, N, x0):
    """a start away from zero: states near x_0, controls of a few units (every entry non-zero)"""
    rng = np.random.default_rng(SEED + N)
    V = np.zeros((B, N + 1, 6))
    V[:, :, :4] = x0[:, None, :] + 0.05 * rng.standard_normal((B, N + 1, 4))
    V[:, :, 4:] = 2.0 * rng.standard_normal((B, N + 1, 2))
    return np.ascontiguousarray(V.reshape(B, -1)[:, :4 * (N + 1) + 2 * N])


@pytest.mark.parametrize("hess", ["exact", "gn"])
def test_start_as_given_vs_oracle(hess, model_json, mmpc_mod, oracle):
    N, B = 17, 5
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    V0 = _seeded_V(B, N, x0)
    s = _two_link(mmpc_mod, model_json, N, hess, max_iter=100)
    g = s.solve_batch_host(x0, up, tr, _w(), V=V0.copy())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), V=V0.copy(), hessian=_oracle_hess(oracle, hess), max_iter=100)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"as given N={N} {hess}")


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("max_iter", [1, 2])
def test_iterate_at_max_iter_vs_oracle(max_iter, hess, model_json, mmpc_mod, oracle):
    """stopped at the iteration limit: the iterate written back is the one the accepted steps left"""
    N, B = 17, 5
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    s = _two_link(mmpc_mod, model_json, N, hess, max_iter=max_iter)
    g = s.solve_batch_host(x0, up, tr, _w())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=_oracle_hess(oracle, hess), max_iter=max_iter)
    s.close()
    assert (g["status"] == mmpc_mod.STATUS_MAX_ITER).all(), g["status"]
    assert (g["iters"] == max_iter).all(), g["iters"]
    assert np.abs(g["V"][:, 4:]).max() > 0.0   # (the iterate moved)
    _same_as_oracle(g, o, f"max_iter={max_iter} {hess}")


REJECT_SCALE = {17: 40.0, 33: 20.0}


@pytest.mark.parametrize("N", [17, 33])
def test_rejected_full_step_vs_oracle(N, model_json, mmpc_mod, oracle):
    """the recipe of tests/test_gpu_group_sweep_shapes.py test_rejected_full_step_vs_oracle (targets x 20, Delta-u
    weight / 100, B = 8) at a horizon of two rounds and of three: some instance rejects alpha = 1 after its first
    iteration (asserted from the solver's own trace, column 5), so the alpha / 2 trials start from the old iterate
    after the fused trial has run.  Target factor (REJECT_SCALE): 20 at N = 33 (instance 4
    rejects once); at N = 17 no instance rejects a step at 20 or 30, so the factor there is 40 (instances 3 and 7 reject
    once each); the oracle converges on all eight instances at both."""
    import torch
    B = 8
    w = _w()
    w[4:6] *= 0.01
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    tr = np.ascontiguousarray(tr * REJECT_SCALE[N])
    s = _two_link(mmpc_mod, model_json, N, "exact", init_states=mmpc_mod.INIT_ZERO, max_iter=60)
    g = s.solve_batch_host(x0, up, tr, w)
    o = oracle.solve_batch(N, H, x0, up, tr, w, hessian=oracle.HESS_EXACT, init_states=2, max_iter=60)
    f64 = dict(dtype=torch.float64, device="cuda")
    t = [torch.tensor(a, **f64) for a in (x0, up, tr, w)]
    V = torch.zeros((B, s.NV), **f64)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    kk = torch.zeros(B, **f64)
    trace = torch.zeros((B, 61, 8), **f64)
    L = s._L
    L.mmpc_debug_solve_trace.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 6
    rc = L.mmpc_debug_solve_trace(s._h, B, *(a.data_ptr() for a in t), 0, V.data_ptr(), st.data_ptr(), it.data_ptr(),
                                  kk.data_ptr(), trace.data_ptr(), None)
    assert rc == 0, L.mmpc_last_error()
    torch.cuda.synchronize()
    iters = it.cpu().numpy()
    alpha = trace[:, :, 5].cpu().numpy()
    live = np.arange(61)[None, :] < iters[:, None]
    short = (alpha < 1.0) & live
    print(f"N={N}: iterations with alpha < 1 per instance:", short.sum(1).tolist())
    s.close()
    assert short[:, 1:].any(), "no full step was rejected after the first iteration: the case proves nothing"
    assert np.array_equal(V.cpu().numpy(), g["V"]) and np.array_equal(iters, g["iters"])   # the trace solve: same iterates
    _same_as_oracle(g, o, f"rejected full step N={N}")


# ---------------------------------------------------------------------------------------------- prologue
@pytest.mark.parametrize("init", ["as_given", "hold_x0", "zero"])
@pytest.mark.parametrize("N", [1, 17, 33])
def test_init_modes_vs_oracle(N, init, model_json, mmpc_mod, oracle):
    m, B = mmpc_mod, 5
    mode = {"as_given": m.INIT_AS_GIVEN, "hold_x0": m.INIT_HOLD_X0, "zero": m.INIT_ZERO}[init]
    omode = {"as_given": 0, "hold_x0": 1, "zero": 2}[init]
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    V0 = _seeded_V(B, N, x0)
    s = _two_link(m, model_json, N, "exact", init_states=mode, max_iter=100)
    g = s.solve_batch_host(x0, up, tr, _w(), V=V0.copy())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), V=V0.copy(), hessian=oracle.HESS_EXACT, init_states=omode,
                           max_iter=100)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"init {init} N={N}")


def test_per_instance_weights_vs_oracle(model_json, mmpc_mod, oracle):
    """weights_stride = nx + 2 nu: one row of weights per instance"""
    N, B = 17, 5
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    rng = np.random.default_rng(SEED)
    w = _w()[None, :] * rng.uniform(0.5, 2.0, size=(B, 8))
    s = _two_link(mmpc_mod, model_json, N, "exact")
    g = s.solve_batch_host(x0, up, tr, w)
    o = oracle.solve_batch(N, H, x0, up, tr, w, hessian=oracle.HESS_EXACT)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    assert not np.array_equal(g["V"][0], g["V"][1])
    _same_as_oracle(g, o, "per-instance weights")


def test_exo_tail_handover_resume_launch(mmpc_mod, oracle, tmp_path, monkeypatch):
    """the smallest batch at which tests/test_gpu_tail.py test_tail_handover_vs_oracle hands a lane-kernel tail to the
    16-lane resume launch (exo, N = 50, B = 512, cap 4, exact Hessian), with that test's criteria: the resume launch's
    prologue and reductions, against the oracle and against the same solve without hand-over"""
    from test_gpu_parity import _compare, _rel
    N, B, cap, hess = 50, 512, 4, 2
    x0, up, tr = oracle.synth(SEED, 0, B, N, H, model=oracle.EXO)
    p = mmpc_mod.write_model_json(str(tmp_path / "exo_tail.json"), "exo", 8, 4, 2000, N, model="exo_arm")
    monkeypatch.setenv("MMPC_TAIL_CAP", str(cap))
    s = mmpc_mod.Solver(p, kkt_solver=2, init_states=mmpc_mod.INIT_ZERO, hessian=hess)
    monkeypatch.delenv("MMPC_TAIL_CAP")
    r = s.solve_batch_host(x0, up, tr, W_EXO)
    s.close()
    off = mmpc_mod.Solver(p, kkt_solver=2, init_states=mmpc_mod.INIT_ZERO, hessian=hess, tail_cap=0)
    f = off.solve_batch_host(x0, up, tr, W_EXO)
    off.close()
    o = oracle.solve_batch(N, H, x0, up, tr, W_EXO, model=oracle.EXO, kkt=oracle.KKT_RICCATI, init_states=2,
                           hessian=oracle.HESS_EXACT)
    assert (r["status"] == 0).all() and (o["status"] == 0).all()
    print("instances past the cap:", int((r["iters"] > cap).sum()))
    assert (r["iters"] > cap).sum() > 0   # some instances did continue in the resume launch
    _compare(r, o)
    same = f["iters"] == r["iters"]
    assert same.mean() >= 0.99
    assert _rel(r["V"][same], f["V"][same]).max() <= 1e-10
