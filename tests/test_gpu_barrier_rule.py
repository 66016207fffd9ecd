"""GPU: Mehrotra's predictor-corrector barrier rule in the 16-lane interior-point kernel (sqp_group_mehrotra_kernel;
mmpc_set_barrier_rule(MMPC_BARRIER_MEHROTRA)) -- the same algorithm as the oracle's rule 1
(oracle_set_ip_rule(1), mmpc_oracle.c solve_one_ip).

All solves: kkt_solver = RICCATI_GROUP, max_iter = 100, seed 20250213, the cfg#2 weights (exo: those of
test_gpu_xbounds.py).  Parity criterion: `compare` of test_gpu_xbounds.py (identical converged sets, identical
iteration counts on >= 90 % of the converged instances, V* within 1e-10 relative on those, 1e-6 on all converged)."""
import numpy as np
import pytest

from conftest import WEIGHTS_CFG, load_golden
from test_gpu_xbounds import CASES, compare, states

pytestmark = pytest.mark.gpu
INF = np.inf
SEED = 20250213
W_EXO = [10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4
VEL = (np.array([-INF, -INF, -1.5, -1.5]), np.array([INF, INF, 1.5, 1.5]))


def oracle_rule1(oracle, *a, **kw):
    try:
        oracle.set_ip_rule(1)
        return oracle.solve_batch(*a, **kw)
    finally:
        oracle.set_ip_rule(0)


def group_solver(m, path, rule, hessian=None, **kw):
    s = m.Solver(path, max_iter=100, kkt_solver=m.KKT_RICCATI_GROUP, hessian=hessian, barrier_rule=rule, **kw)
    return s


@pytest.fixture(scope="module")
def velocity_inputs(oracle):
    """the velocity case's inputs (N = 30, B = 128), shared and never modified"""
    x0, up, tr = oracle.synth(SEED, 0, 128, 30, 0.002)
    for a in (x0, up, tr):
        a.setflags(write=False)
    return x0, up, tr


# ---- 1. parity with the oracle's rule 1 ----
@pytest.mark.parametrize("case,hess", [("velocity", "gn"), ("velocity", "exact"), ("velocity+u", "gn"),
                                       ("position", "gn")])
def test_mehrotra_matches_oracle_rule1(case, hess, model_json, mmpc_mod, oracle, velocity_inputs):
    m = mmpc_mod
    xl, xu, ul, uu = (None if v is None else np.array(v) for v in CASES[case])
    N, h, B = 30, 0.002, 128
    exact = hess == "exact"
    s = group_solver(m, model_json(N=N), m.BARRIER_MEHROTRA, m.HESSIAN_EXACT if exact else m.HESSIAN_GAUSS_NEWTON)
    s.set_state_bounds(xl, xu)
    assert s.kkt_solver_for(B) == m.KKT_RICCATI_GROUP and s.hessian_for(B) == (2 if exact else 1)
    x0, up, tr = velocity_inputs
    w = np.array(WEIGHTS_CFG)
    g = s.solve_batch_host(x0, up, tr, w, u_lb=ul, u_ub=uu)
    o = oracle_rule1(oracle, N, h, x0, up, tr, w, u_lb=ul, u_ub=uu, x_lb=xl, x_ub=xu, max_iter=100,
                     hessian=oracle.HESS_EXACT if exact else oracle.HESS_GAUSS_NEWTON)
    ok = g["status"] == 0
    print(f"{case} {hess}: GPU iterations mean {g['iters'][ok].mean():.2f} max {g['iters'][ok].max()}, oracle rule 1 "
          f"mean {o['iters'][o['status'] == 0].mean():.2f}; same count on {(g['iters'] == o['iters'])[ok].sum()} of "
          f"{ok.sum()} converged")
    compare(g, o)
    X = states(g["V"][ok], N, 4, 2)
    assert (X >= xl - 1e-12).all() and (X <= xu + 1e-12).all()
    if ul is not None:
        U = np.stack([g["V"][ok][:, k * 6 + 4:k * 6 + 6] for k in range(N)], 1)
        assert (U >= ul - 1e-12).all() and (U <= uu + 1e-12).all()
    if case == "position":
        assert (~ok).sum() > 0 and (o["status"] != 0).sum() > 0   # infeasible instances fail under the rule too
        s.set_barrier_rule(m.BARRIER_MONOTONE)                      # ... as they do under the monotone rule
        g0 = s.solve_batch_host(x0, up, tr, w, u_lb=ul, u_ub=uu)
        assert (g0["status"] != 0).sum() > 0
    else:
        assert ok.all()


# ---- 2. small and awkward shapes ----
SHAPES = [(5, False), (16, False), (31, False), (17, True)]


@pytest.mark.parametrize("N,ub", SHAPES)
def test_mehrotra_small_shapes_two_link(N, ub, model_json, mmpc_mod, oracle):
    """N = 5: fewer stages than lanes, N mod 3 = 2 (no bound active: the barrier path alone); 16: one lane round,
    N mod 3 = 1; 31: two rounds; 17 with |u| <= 4"""
    m = mmpc_mod
    h, B = 0.002, 32
    xl, xu = VEL
    ul, uu = (np.array([-4.0, -4.0]), np.array([4.0, 4.0])) if ub else (None, None)
    x0, up, tr = oracle.synth(SEED, 0, B, N, h)
    x0[:, 2:] = np.clip(x0[:, 2:], -1.4, 1.4)
    w = np.array(WEIGHTS_CFG)
    s = group_solver(m, model_json(N=N), m.BARRIER_MEHROTRA)
    s.set_state_bounds(xl, xu)
    g = s.solve_batch_host(x0, up, tr, w, u_lb=ul, u_ub=uu)
    o = oracle_rule1(oracle, N, h, x0, up, tr, w, u_lb=ul, u_ub=uu, x_lb=xl, x_ub=xu, max_iter=100)
    assert (o["status"] == 0).all()
    compare(g, o)
    assert np.abs(states(g["V"], N, 4, 2)[:, :, 2:]).max() <= 1.5 + 1e-12


@pytest.mark.parametrize("hess", ["gn", "exact"])
def test_mehrotra_exo(hess, mmpc_mod, oracle, tmp_path):
    """exo N = 20, |qdot| <= 0.3, B = 70 (the last wave holds two instances), both Hessians"""
    m = mmpc_mod
    N, h, B = 20, 0.002, 70
    xl = np.array([-INF] * 4 + [-0.3] * 4)
    xu = np.array([INF] * 4 + [0.3] * 4)
    exact = hess == "exact"
    p = m.write_model_json(str(tmp_path / "exo20.json"), "exo20", 8, 4, 2000, N, model="exo_arm")
    s = group_solver(m, p, m.BARRIER_MEHROTRA, m.HESSIAN_EXACT if exact else m.HESSIAN_GAUSS_NEWTON)
    s.set_state_bounds(xl, xu)
    assert s.kkt_solver_for(B) == m.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, h, model=oracle.EXO)
    x0[:, 4:] = np.clip(x0[:, 4:], -0.25, 0.25)
    w = np.array(W_EXO)
    g = s.solve_batch_host(x0, up, tr, w)
    o = oracle_rule1(oracle, N, h, x0, up, tr, w, x_lb=xl, x_ub=xu, max_iter=100, model=oracle.EXO,
                     hessian=oracle.HESS_EXACT if exact else oracle.HESS_GAUSS_NEWTON)
    assert (o["status"] == 0).all()
    compare(g, o)
    assert np.abs(states(g["V"], N, 8, 4)[:, :, 4:]).max() <= 0.3 + 1e-12


# ---- 3. fewer iterations ----
def test_mehrotra_takes_fewer_iterations(model_json, mmpc_mod, velocity_inputs):
    m = mmpc_mod
    x0, up, tr = velocity_inputs
    w = np.array(WEIGHTS_CFG)
    it = {}
    for rule in (m.BARRIER_MONOTONE, m.BARRIER_MEHROTRA):
        s = group_solver(m, model_json(N=30, name=f"r{rule}"), rule, m.HESSIAN_GAUSS_NEWTON)
        s.set_state_bounds(*VEL)
        g = s.solve_batch_host(x0, up, tr, w)
        assert (g["status"] == 0).all()
        it[rule] = g["iters"]
        wave = g["iters"].reshape(-1, 4).max(1).mean()
        print(f"rule {rule}: iterations {np.bincount(g['iters']).tolist()} mean {g['iters'].mean():.2f} "
              f"max {g['iters'].max()}, wave-max mean over groups of 4: {wave:.2f}")
    assert it[m.BARRIER_MEHROTRA].mean() < 0.85 * it[m.BARRIER_MONOTONE].mean()


# ---- 4. the same KKT points as the scipy golden vectors ----
@pytest.mark.parametrize("hess", ["gn", "exact"])
def test_mehrotra_reaches_the_golden_kkt_points(hess, mmpc_mod, tmp_path):
    m = mmpc_mod
    gold = load_golden("xbounds_golden.json")
    h = gold["h"]
    for i, case in enumerate(gold["cases"]):
        exo = case["model"] == "exo_arm"
        nx, nu = (8, 4) if exo else (4, 2)
        path = m.write_model_json(str(tmp_path / f"g{i}.json"), f"g{i}", nx, nu, int(h * 1e6), case["N"],
                                  x_min=case["x_lb"], x_max=case["x_ub"], model="exo_arm" if exo else "two_link_arm")
        s = m.Solver(path, max_iter=200, kkt_solver=m.KKT_RICCATI_GROUP, barrier_rule=m.BARRIER_MEHROTRA,
                     hessian=m.HESSIAN_EXACT if hess == "exact" else m.HESSIAN_GAUSS_NEWTON)
        ul, uu = np.array(case["u_lb"]), np.array(case["u_ub"])
        g = s.solve_batch_host(np.array(case["x0"])[None], np.array(case["u_prev"])[None],
                               np.array(case["traj"])[None], np.array(case["weights"]),
                               u_lb=None if np.isinf(ul).all() else ul, u_ub=None if np.isinf(uu).all() else uu)
        assert g["status"][0] == 0, (i, g["status"], g["iters"])
        Vg = np.array(case["V"])
        assert np.abs(g["V"][0] - Vg).max() / np.abs(Vg).max() < 1e-6, i
        s.close()


# ---- 5. independence of batch composition ----
def test_mehrotra_batch_composition(model_json, mmpc_mod, oracle):
    m = mmpc_mod
    N, B = 30, 32
    x0, up, tr = oracle.synth(SEED, 0, B, N, 0.002)
    w = np.array(WEIGHTS_CFG)
    s = group_solver(m, model_json(N=N), m.BARRIER_MEHROTRA)
    s.set_state_bounds(*VEL)
    full = s.solve_batch_host(x0, up, tr, w)
    for b in (1, 5):
        part = s.solve_batch_host(x0[:b], up[:b], tr[:b], w)
        for k in ("V", "status", "iters"):
            assert np.array_equal(part[k], full[k][:b]), (b, k)


# ---- 6. refusals ----
def test_mehrotra_refusals(model_json, mmpc_mod, tmp_path):
    m = mmpc_mod
    w = np.array(WEIGHTS_CFG)

    def refused(s, nx, nu, N, weights):
        with pytest.raises(m.MmpcError) as e:
            s.solve_batch_host(np.zeros((4, nx)), np.zeros((4, nu)), np.zeros((4, N, nx)), weights)
        assert e.value.code == -4 and "MEHROTRA" in str(e.value), str(e.value)

    s = m.Solver(model_json(N=30), kkt_solver=m.KKT_RICCATI, barrier_rule=m.BARRIER_MEHROTRA)   # the lane solver
    s.set_state_bounds(*VEL)
    refused(s, 4, 2, 30, w)
    s.set_barrier_rule(m.BARRIER_MONOTONE)   # the same handle is served under the monotone rule
    s.solve_batch_host(np.zeros((4, 4)), np.zeros((4, 2)), np.zeros((4, 30, 4)), w)
    p = m.write_model_json(str(tmp_path / "exo50.json"), "exo50", 8, 4, 2000, 50, model="exo_arm",
                           x_min=[-1e31] * 4 + [-0.3] * 4, x_max=[1e31] * 4 + [0.3] * 4)
    s = m.Solver(p, barrier_rule=m.BARRIER_MEHROTRA)            # AUTO resolves to the lane solver
    assert s.kkt_solver_for(4) == m.KKT_RICCATI
    refused(s, 8, 4, 50, np.array(W_EXO))
    s = m.Solver(model_json(N=30, name="lin", is_linear=True, x_min=[-1e31, -1e31, -1.5, -1.5],
                            x_max=[1e31, 1e31, 1.5, 1.5]),
                 kkt_solver=m.KKT_RICCATI_GROUP, barrier_rule=m.BARRIER_MEHROTRA)   # linear mode
    refused(s, 4, 2, 30, w)
    # without finite state bounds the rule is ignored
    s = m.Solver(model_json(N=30, name="free"), kkt_solver=m.KKT_RICCATI, barrier_rule=m.BARRIER_MEHROTRA)
    assert (s.solve_batch_host(np.zeros((4, 4)), np.zeros((4, 2)), np.zeros((4, 30, 4)), w)["status"] == 0).all()


# ---- 7. the default path is untouched ----
def test_monotone_after_mehrotra_is_the_default_solve(model_json, mmpc_mod, velocity_inputs):
    m = mmpc_mod
    x0, up, tr = velocity_inputs
    w = np.array(WEIGHTS_CFG)
    a = group_solver(m, model_json(N=30, name="a"), None)
    a.set_state_bounds(*VEL)
    ref = a.solve_batch_host(x0, up, tr, w)
    b = group_solver(m, model_json(N=30, name="b"), m.BARRIER_MEHROTRA)
    b.set_state_bounds(*VEL)
    mid = b.solve_batch_host(x0, up, tr, w)
    assert not np.array_equal(mid["iters"], ref["iters"])
    b.set_barrier_rule(m.BARRIER_MONOTONE)
    back = b.solve_batch_host(x0, up, tr, w)
    for k in ("V", "status", "iters"):
        assert np.array_equal(back[k], ref[k]), k


# ---- 8. graph safety ----
def test_mehrotra_solve_replays_from_a_graph(model_json, mmpc_mod):
    import torch
    m = mmpc_mod
    N, B = 30, 256
    s = group_solver(m, model_json(N=N), None, init_states=m.INIT_ZERO)
    s.set_state_bounds(*VEL)
    s.reserve_workspace(B)
    s.set_barrier_rule(m.BARRIER_MEHROTRA)   # after the reservation: no solve may allocate
    f = dict(dtype=torch.float64, device="cuda")
    x0 = torch.empty((B, 4), **f)
    up = torch.empty((B, 2), **f)
    tr = torch.empty((B, N, 4), **f)
    wt = torch.tensor(WEIGHTS_CFG, **f)
    s.synth(SEED, 0, B, x0, up, tr)
    torch.cuda.synchronize()

    def outputs():
        return (torch.zeros((B, s.NV), **f), torch.full((B,), -1, dtype=torch.int32, device="cuda"),
                torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, **f))

    ref = outputs()
    s.solve_batch(B, x0, up, tr, wt, *ref)
    torch.cuda.synchronize()
    assert (ref[1] == 0).all()
    g_out = outputs()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):   # one eager solve on the capture stream before capturing
        s.solve_batch(B, x0, up, tr, wt, *g_out, stream=cs.cuda_stream)
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        s.solve_batch(B, x0, up, tr, wt, *g_out, stream=cs.cuda_stream)
    for t in g_out:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(g_out, ref):
        assert torch.equal(a, b)
