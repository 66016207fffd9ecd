"""GPU: where the serial sweeps of the 2-link 16-lane kernels issue their loads (csrc/sqp_group.h).

The Riccati sweep (backward_dist) hands h da/du and c of stage k - 1 over from stage k, loaded one stage ahead into one
buffer; its peeled first stage loads its own pair and the last stage loads nothing ahead.  The step sweep (step_dist)
opens with three refills issued back to back when the horizon has three stages, and with a block of its own for
N < 3.  No operand, operation or stored value changes, so every case here is a plain comparison with the oracle at the
shapes where an off-by-one stage, a read of the neighbour group's block or a wrong branch of the opening would show:

* N = 1, 2, 3 (the opening covers the whole horizon), 4, 5, 6 (zero, one or two refilling stages behind it), 7, 8 (both
  parities of the Riccati pair loop); exact and Gauss-Newton; unbounded and |u| <= 2 (the control-bounded kernels run
  the sweep one stage per trip and load the un-held rows in the same refills); the whole solve and max_iter = 1;
* one instance alone and as each group of a wave among different neighbours, N = 5 and 17: same bytes;
* ragged batches (B = 5, 7: a last wave with one and with three valid groups);
* N = 16, 17, 30, 33 (the stage-parallel phases' round boundaries; N > 32 loops over pairs of rounds);
* the state-bounded solve at N = 5 and 17, whose sweep takes the same loads.

Criterion of tests/test_gpu_group_iteration_trims.py: identical status and iteration counts on every instance, V within
1e-10 relative to max|V| (same algorithm on both sides)."""
import numpy as np
import pytest

from conftest import WEIGHTS_CFG
from test_gpu_group_sweep_shapes import H, INF, SEED, _oracle_hess, _same_as_oracle, _two_link

pytestmark = pytest.mark.gpu

UB = (np.array([-2.0, -2.0]), np.array([2.0, 2.0]))
VEL = (np.array([-INF, -INF, -1.5, -1.5]), np.array([INF, INF, 1.5, 1.5]))


def _w():
    return np.array(WEIGHTS_CFG)


def _solve_both(m, oracle, model_json, N, B, hess, bounded, max_iter=None, first=0):
    kw = {} if max_iter is None else dict(max_iter=max_iter)
    s = _two_link(m, model_json, N, hess, **kw)
    assert s.kkt_solver_for(B) == m.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, first, B, N, H)
    bk = dict(u_lb=UB[0], u_ub=UB[1]) if bounded else {}
    g = s.solve_batch_host(x0, up, tr, _w(), **bk)
    # solver=s: the Hessian the solver resolves for this solve (asserted: the one asked for) and, with bounds, the
    # 16-lane kernel's hold-release rule
    assert {1: oracle.HESS_GAUSS_NEWTON, 2: oracle.HESS_EXACT}[s.hessian_for(B, bounded)] == _oracle_hess(oracle, hess)
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), solver=s, **bk, **kw)
    s.close()
    return g, o


@pytest.mark.parametrize("max_iter", [None, 1])
@pytest.mark.parametrize("bounded", [False, True], ids=["free", "u-bounds"])
@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 8])
def test_horizon_edges_vs_oracle(N, hess, bounded, max_iter, model_json, mmpc_mod, oracle):
    g, o = _solve_both(mmpc_mod, oracle, model_json, N, 5, hess, bounded, max_iter)
    if max_iter is None:
        assert (o["status"] == 0).all(), o["status"]
    else:
        assert (g["iters"] == 1).all(), g["iters"]
    _same_as_oracle(g, o, f"N={N} {hess} {'u-bounds' if bounded else 'free'} max_iter={max_iter}")


@pytest.mark.parametrize("N", [5, 17])
def test_instance_alone_and_in_every_group(N, model_json, mmpc_mod, oracle):
    """instance 0 alone (B = 1), then as group 0, 1, 2, 3 of one wave with three other instances around it (a different
    set for every place): V, status and iteration count are the same bytes in all five solves"""
    x0, up, tr = oracle.synth(SEED, 0, 16, N, H)
    s = _two_link(mmpc_mod, model_json, N, "exact")
    alone = s.solve_batch_host(x0[:1], up[:1], tr[:1], _w())
    assert alone["status"][0] == 0
    for place in range(4):
        others = [1 + 3 * place + j for j in range(3)]
        idx = others[:place] + [0] + others[place:]
        g = s.solve_batch_host(np.ascontiguousarray(x0[idx]), np.ascontiguousarray(up[idx]),
                               np.ascontiguousarray(tr[idx]), _w())
        assert g["V"][place].tobytes() == alone["V"][0].tobytes(), (N, place)
        assert g["status"][place] == alone["status"][0] and g["iters"][place] == alone["iters"][0], (N, place)
    s.close()


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("B", [5, 7])
def test_ragged_batch_vs_oracle(B, hess, model_json, mmpc_mod, oracle):
    g, o = _solve_both(mmpc_mod, oracle, model_json, 6, B, hess, False, first=40)
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"ragged B={B} {hess}")


@pytest.mark.parametrize("N", [16, 17, 30, 33])
def test_round_shapes_vs_oracle(N, model_json, mmpc_mod, oracle):
    g, o = _solve_both(mmpc_mod, oracle, model_json, N, 5, "exact", False)
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"N={N} exact")


@pytest.mark.parametrize("N", [5, 17])
def test_state_bounded_vs_oracle(N, model_json, mmpc_mod, oracle):
    m, B = mmpc_mod, 5
    s = m.Solver(model_json(N=N), max_iter=100, kkt_solver=m.KKT_RICCATI_GROUP)
    s.set_state_bounds(*VEL)
    assert s.kkt_solver_for(B) == m.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    g = s.solve_batch_host(x0, up, tr, _w())
    hess = {1: oracle.HESS_GAUSS_NEWTON, 2: oracle.HESS_EXACT}[s.hessian_for(B, False)]
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), x_lb=VEL[0], x_ub=VEL[1], max_iter=100, hessian=hess)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"state bounds N={N}")
