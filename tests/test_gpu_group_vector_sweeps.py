"""GPU: the vector sweeps of the 16-lane kernel (d recursion, adjoint, step sweep) at the shapes where their loops
change form, and with lanes that carry another lane's row.

In the 2-link kernels a lane without an x row carries row 0's chain in these sweeps and stores it again over lane 0's
value, so the stores have no lane mask; the d recursion and the adjoint refill a buffer after its last use; the step
sweep runs its addresses along the horizon, takes the stages that have a stage three ahead three at a time plus one or
two left over, and ends with three stages that fetch nothing (csrc/sqp_group.h).  Every case is the GPU solve against
the CPU oracle running the same algorithm, with the criterion of tests/test_gpu_group_sweep_shapes.py: identical
status and iteration counts on every instance, V* within 1e-10 relative to max|V|; the oracle converges on every case.

Horizons: N = 5 .. 9 (with 1 .. 4 of the other file every N mod 6: the pair loops' peel x the step sweep's left-over
stages), N = 2, 3 alone in a wave (no loop trip at all, three absent groups), N = 7 with a full wave and with a wave
and a half.  Variants at N = 6, 7: control bounds, state bounds; at N = 7: Mehrotra's rule, per-instance control
bounds; the exo arm (which keeps masked stores and the clamped prefetch) at N = 3 and 7.

Placement: one instance solved alone and as group 0, 1, 2, 3 of a wave among different neighbours gives the same bytes
-- the lanes that mirror row 0 stay inside their own instance."""
import numpy as np
import pytest

from conftest import WEIGHTS_CFG
from test_gpu_group_sweep_shapes import H, INF, SEED, W_EXO, _oracle_hess, _same_as_oracle, _two_link

pytestmark = pytest.mark.gpu

VEL = (np.array([-INF, -INF, -1.5, -1.5]), np.array([INF, INF, 1.5, 1.5]))


def _w():
    return np.array(WEIGHTS_CFG)


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N", [5, 6, 7, 8, 9])
def test_horizons_mod_six_vs_oracle(N, hess, model_json, mmpc_mod, oracle):
    B = 5
    s = _two_link(mmpc_mod, model_json, N, hess)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    g = s.solve_batch_host(x0, up, tr, _w())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=_oracle_hess(oracle, hess))
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"N={N} {hess}")


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N,B", [(2, 1), (3, 1), (7, 4), (7, 6)])
def test_wave_fill_vs_oracle(N, B, hess, model_json, mmpc_mod, oracle):
    s = _two_link(mmpc_mod, model_json, N, hess)
    x0, up, tr = oracle.synth(SEED, 40, B, N, H)
    g = s.solve_batch_host(x0, up, tr, _w())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=_oracle_hess(oracle, hess))
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"N={N} B={B} {hess}")


@pytest.mark.parametrize("N", [6, 7])
def test_control_bounds_vs_oracle(N, model_json, mmpc_mod, oracle):
    B = 5
    lb, ub = np.array([-2.0, -2.0]), np.array([2.0, 2.0])
    s = mmpc_mod.Solver(model_json(N=N), kkt_solver=mmpc_mod.KKT_RICCATI_GROUP)
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    g = s.solve_batch_host(x0, up, tr, _w(), u_lb=lb, u_ub=ub)
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), u_lb=lb, u_ub=ub, solver=s)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    U = np.stack([g["V"][:, k * 6 + 4:k * 6 + 6] for k in range(N)], 1)
    print(f"N={N}: {int((np.abs(U) >= 2.0 - 1e-12).sum())} of {U.size} controls at a bound")
    _same_as_oracle(g, o, f"control bounds N={N}")


@pytest.mark.parametrize("N", [6, 7])
def test_state_bounds_vs_oracle(N, model_json, mmpc_mod, oracle):
    B = 5
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
    _same_as_oracle(g, o, f"state bounds N={N}")


def test_mehrotra_vs_oracle(model_json, mmpc_mod, oracle):
    """the rule and the inputs of tests/test_gpu_barrier_rule.py (small shapes), at N = 7"""
    m, N, B = mmpc_mod, 7, 5
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
    _same_as_oracle(g, o, "Mehrotra N=7")


def test_per_instance_bounds_vs_oracle(model_json, mmpc_mod, oracle):
    """[B, nu] bounds, one row per instance (the host entry of tests/test_gpu_instance_bounds.py), against one oracle
    solve per instance with that instance's bounds and the 16-lane kernel's hold-release rule"""
    m, N, B = mmpc_mod, 7, 5
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    c = np.array([1.0, 1.5, 2.0, 3.0, INF])
    lb, ub = -np.stack([c, 0.5 * c], 1), np.stack([0.75 * c, c], 1)
    s = m.Solver(model_json(N=N), kkt_solver=m.KKT_RICCATI_GROUP, hessian=m.HESSIAN_GAUSS_NEWTON)
    assert s.kkt_solver_for(B) == m.KKT_RICCATI_GROUP
    g = s.solve_batch_host(x0, up, tr, _w(), u_lb=lb, u_ub=ub)
    s.close()
    res = [oracle.solve_batch(N, H, x0[b:b + 1], up[b:b + 1], tr[b:b + 1], _w(), u_lb=lb[b], u_ub=ub[b],
                              hessian=oracle.HESS_GAUSS_NEWTON, bound_release=True) for b in range(B)]
    o = {k: np.concatenate([r[k] for r in res]) for k in ("V", "status", "iters")}
    assert (o["status"] == 0).all(), o["status"]
    U = np.stack([g["V"][:, k * 6 + 4:k * 6 + 6] for k in range(N)], 1)
    nact = int(((U == lb[:, None, :]) | (U == ub[:, None, :])).sum())
    print(f"per-instance bounds: {nact} of {U.size} controls on a bound")
    assert nact >= 1
    _same_as_oracle(g, o, "per-instance bounds N=7")


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N", [3, 7])
def test_exo_vs_oracle(N, hess, mmpc_mod, oracle, tmp_path):
    B = 5
    p = mmpc_mod.write_model_json(str(tmp_path / f"exo_{N}.json"), "exo_arm", 8, 4, 2000, N, model="exo_arm")
    h = mmpc_mod.HESSIAN_EXACT if hess == "exact" else mmpc_mod.HESSIAN_GAUSS_NEWTON
    s = mmpc_mod.Solver(p, kkt_solver=mmpc_mod.KKT_RICCATI_GROUP, hessian=h)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H, model=oracle.EXO)
    g = s.solve_batch_host(x0, up, tr, W_EXO)
    o = oracle.solve_batch(N, H, x0, up, tr, W_EXO, model=oracle.EXO, hessian=_oracle_hess(oracle, hess))
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"exo N={N} {hess}")


@pytest.mark.parametrize("variant", ["exact", "gn", "u-bounds", "x-bounds"])
def test_placement_in_the_wave(variant, model_json, mmpc_mod, oracle):
    """instance 0 of the batch alone, then as group 0, 1, 2, 3 of one wave with three other instances around it (a
    different set for every place): V, status and iteration count of the instance are the same bytes every time"""
    m, N = mmpc_mod, 7
    x0, up, tr = oracle.synth(SEED, 0, 16, N, H)
    kw = {}
    if variant in ("exact", "gn"):
        s = _two_link(m, model_json, N, variant)
    else:
        s = m.Solver(model_json(N=N), max_iter=100, kkt_solver=m.KKT_RICCATI_GROUP)
        if variant == "u-bounds":
            kw = dict(u_lb=np.array([-2.0, -2.0]), u_ub=np.array([2.0, 2.0]))
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
