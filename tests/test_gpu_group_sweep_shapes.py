"""GPU: the serial sweeps of the 16-lane kernel at the shapes where their loops change form.

The sweeps read "this lane's row / column of A_k" through a per-lane LDS address with a per-lane stage stride (a lane
without the role reads the instance's constant block with stride 0) and a lane's W_k row through one row offset plus
immediate column offsets (csrc/sqp_group.h).  Every case is the GPU solve against the CPU oracle running the same
algorithm: identical status and identical iteration counts on every instance, V* within 1e-10 relative to max|V|
(same algorithm; the bound of tests/test_gpu_group_w_onchip.py and of smoke()).

Horizons: N = 1, 2, 3, 4 (the peels of the pair loops of the d recursion, the adjoint and the Riccati sweep -- N
parity -- and of the three-buffer step loop -- N mod 3; the prefetches two and three stages ahead run past the arrays'
ends from the first stage on), 15 / 16 / 17 (one round of the stage-parallel passes and of the W pass against two), 30
(cfg#2), 31, 33 (two rounds against three).  B = 1, 3, 5: a partly filled wave, whose absent groups must touch
nothing, alone and after a full wave.  Variants: the 2-link arm with the exact Hessian (packed W record on chip) and
Gauss-Newton, with control bounds and with state bounds (their kernels share the sweeps and keep W in the workspace),
and the exo arm (8 states: the constant block is 16 doubles, its column reads start at the block's first double).

A rejected full step: targets 20 x further away and a Delta-u weight / 100 (the recipe of tests/test_gpu_lazy_steps.py)
make instances 3 and 7 of the batch reject alpha = 1 in their second and third iterations under the exact Hessian, so the
line search goes on from the old iterate after the fused alpha = 1 trial has run; asserted from the solver's
own per-iteration trace."""
import ctypes as C

import numpy as np
import pytest

from conftest import WEIGHTS_CFG

pytestmark = pytest.mark.gpu

H = 0.002
SEED = 20250213
W_EXO = np.array([10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4)
INF = np.inf


def _rel(a, b):
    return np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1e-300)


def _same_as_oracle(g, o, tag):
    rel = _rel(g["V"], o["V"])
    print(f"{tag}: status {g['status'].tolist()} iters gpu {g['iters'].tolist()} oracle {o['iters'].tolist()} "
          f"max rel diff {rel.max():.3e}")
    np.testing.assert_array_equal(g["status"], o["status"])
    np.testing.assert_array_equal(g["iters"], o["iters"])
    assert rel.max() <= 1e-10, rel.max()


def _two_link(mmpc_mod, model_json, N, hess, **kw):
    h = mmpc_mod.HESSIAN_EXACT if hess == "exact" else mmpc_mod.HESSIAN_GAUSS_NEWTON
    return mmpc_mod.Solver(model_json(N=N), kkt_solver=mmpc_mod.KKT_RICCATI_GROUP, hessian=h, **kw)


def _oracle_hess(oracle, hess):
    return oracle.HESS_EXACT if hess == "exact" else oracle.HESS_GAUSS_NEWTON


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 15, 16, 17, 30, 31, 33])
def test_horizons_vs_oracle(N, hess, model_json, mmpc_mod, oracle):
    B = 5
    s = _two_link(mmpc_mod, model_json, N, hess)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    w = np.array(WEIGHTS_CFG)
    g = s.solve_batch_host(x0, up, tr, w)
    o = oracle.solve_batch(N, H, x0, up, tr, w, hessian=_oracle_hess(oracle, hess))
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"N={N} {hess}")


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [17, 30])
def test_partly_filled_wave_vs_oracle(N, B, hess, model_json, mmpc_mod, oracle):
    s = _two_link(mmpc_mod, model_json, N, hess)
    x0, up, tr = oracle.synth(SEED, 40, B, N, H)
    w = np.array(WEIGHTS_CFG)
    g = s.solve_batch_host(x0, up, tr, w)
    o = oracle.solve_batch(N, H, x0, up, tr, w, hessian=_oracle_hess(oracle, hess))
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"N={N} B={B} {hess}")


@pytest.mark.parametrize("N", [5, 17])
def test_control_bounds_vs_oracle(N, model_json, mmpc_mod, oracle):
    B = 5
    lb, ub = np.array([-2.0, -2.0]), np.array([2.0, 2.0])
    s = mmpc_mod.Solver(model_json(N=N), kkt_solver=mmpc_mod.KKT_RICCATI_GROUP)
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    w = np.array(WEIGHTS_CFG)
    g = s.solve_batch_host(x0, up, tr, w, u_lb=lb, u_ub=ub)
    o = oracle.solve_batch(N, H, x0, up, tr, w, u_lb=lb, u_ub=ub, solver=s)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    U = np.stack([g["V"][:, k * 6 + 4:k * 6 + 6] for k in range(N)], 1)
    print(f"N={N}: {int((np.abs(U) >= 2.0 - 1e-12).sum())} of {U.size} controls at a bound")
    _same_as_oracle(g, o, f"control bounds N={N}")


@pytest.mark.parametrize("N", [5, 17])
def test_state_bounds_vs_oracle(N, model_json, mmpc_mod, oracle):
    B = 5
    xl, xu = np.array([-INF, -INF, -1.5, -1.5]), np.array([INF, INF, 1.5, 1.5])
    s = mmpc_mod.Solver(model_json(N=N), max_iter=100, kkt_solver=mmpc_mod.KKT_RICCATI_GROUP)
    s.set_state_bounds(xl, xu)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    w = np.array(WEIGHTS_CFG)
    g = s.solve_batch_host(x0, up, tr, w)
    hess = {1: oracle.HESS_GAUSS_NEWTON, 2: oracle.HESS_EXACT}[s.hessian_for(B, False)]
    o = oracle.solve_batch(N, H, x0, up, tr, w, x_lb=xl, x_ub=xu, max_iter=100, hessian=hess)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"state bounds N={N}")


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N", [3, 17])
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


def test_rejected_full_step_vs_oracle(model_json, mmpc_mod, oracle):
    import torch
    B, N = 8, 30
    w = np.array(WEIGHTS_CFG)
    w[4:6] *= 0.01
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    tr = np.ascontiguousarray(tr * 20.0)
    s = _two_link(mmpc_mod, model_json, N, "exact", init_states=mmpc_mod.INIT_ZERO, max_iter=60)
    g = s.solve_batch_host(x0, up, tr, w)
    oracle.exact_fallbacks()
    o = oracle.solve_batch(N, H, x0, up, tr, w, hessian=oracle.HESS_EXACT, init_states=2, max_iter=60)
    print("oracle Gauss-Newton fallbacks:", oracle.exact_fallbacks())
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, "rejected full step")
    # the same solve with the per-iteration trace: column 5 is the accepted step length of the iteration
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
    print("iterations with alpha < 1 per instance:", short.sum(1).tolist())
    s.close()
    assert short[:, 1:].any(), "no full step was rejected after the first iteration: the case proves nothing"
    assert np.array_equal(V.cpu().numpy(), g["V"]) and np.array_equal(iters, g["iters"])   # the trace solve: same iterates
