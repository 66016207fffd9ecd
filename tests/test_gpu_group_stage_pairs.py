"""GPU: two stages per lane in the stage-parallel phases of the unbounded 2-link 16-lane kernels (csrc/sqp_group.h,
PAIR): the fused alpha = 1 trial, phase A and the W pass take stage k and stage k + 16 of a lane in one body, the model
evaluated on both at once (csrc/two_link_fast.h, dpack); a lane whose second stage is past the horizon repeats its
first.

* horizons at every pairing edge: N = 1, 2; 15, 16 (no lane has a second stage); 17 (lane 0 only); 31, 32 (every lane);
  33 (a second pair of rounds, one stage in it); 47, 48, 49 -- exact Hessian and Gauss-Newton, B = 1, 3, 5;
* one instance alone and in each of the four places of a wave, N = 17 and 33: identical bytes;
* rejected full steps (the one-stage trials and phase A after a rejection), asserted from the trace;
* the prologue: the three init_states modes at N = 1, 17, 33 with a non-zero V, per-instance weights, a batch that is
  no multiple of four, u0 written to host memory;
* the linear-mode model at N = 17 (the `lin` test is hoisted out of the paired loops);
* one control-bounded and one state-bounded solve at N = 17 (kernels that keep the one-stage loops).

Every oracle comparison: the oracle's status and iteration counts on every instance, V within 1e-10 relative to max|V|
(tests/test_gpu_group_sweep_shapes.py: the same algorithm on both sides)."""
import ctypes as C

import numpy as np
import pytest

from conftest import WEIGHTS_CFG
from test_gpu_group_iteration_trims import REJECT_SCALE, UB, VEL, _seeded_V
from test_gpu_group_sweep_shapes import H, SEED, _oracle_hess, _same_as_oracle, _two_link

pytestmark = pytest.mark.gpu

EDGES = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49]


def _w():
    return np.array(WEIGHTS_CFG)


@pytest.fixture(scope="module")
def edge_case(oracle):
    """inputs and oracle solutions per (N, hess) at B = 5, computed once; smaller batches are their leading rows"""
    memo = {}

    def get(N, hess):
        if (N, hess) not in memo:
            x0, up, tr = oracle.synth(SEED, 0, 5, N, H)
            o = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=_oracle_hess(oracle, hess))
            for a in (x0, up, tr, *o.values()):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            memo[(N, hess)] = (x0, up, tr, o)
        return memo[(N, hess)]
    return get


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("N", EDGES)
def test_pairing_edges_vs_oracle(N, B, hess, edge_case, model_json, mmpc_mod):
    x0, up, tr, o = edge_case(N, hess)
    s = _two_link(mmpc_mod, model_json, N, hess)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    g = s.solve_batch_host(np.ascontiguousarray(x0[:B]), np.ascontiguousarray(up[:B]), np.ascontiguousarray(tr[:B]), _w())
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    ob = {k: o[k][:B] for k in ("V", "status", "iters")}   # (instances are independent: the oracle's first B rows)
    _same_as_oracle(g, ob, f"N={N} B={B} {hess}")


@pytest.mark.parametrize("hess", ["exact", "gn"])
@pytest.mark.parametrize("N", [17, 33])
def test_placement_in_the_wave(N, hess, model_json, mmpc_mod, oracle):
    """instance 0 alone, then as group 0, 1, 2, 3 of one wave among three other instances (another set for every place):
    the same bytes every time"""
    x0, up, tr = oracle.synth(SEED, 0, 16, N, H)
    s = _two_link(mmpc_mod, model_json, N, hess)
    alone = s.solve_batch_host(x0[:1], up[:1], tr[:1], _w())
    assert alone["status"][0] == 0
    for place in range(4):
        others = [1 + 3 * place + j for j in range(3)]
        idx = others[:place] + [0] + others[place:]
        g = s.solve_batch_host(np.ascontiguousarray(x0[idx]), np.ascontiguousarray(up[idx]),
                               np.ascontiguousarray(tr[idx]), _w())
        assert g["V"][place].tobytes() == alone["V"][0].tobytes(), (N, hess, place)
        assert g["status"][place] == alone["status"][0] and g["iters"][place] == alone["iters"][0], (N, hess, place)
    s.close()


@pytest.mark.parametrize("N", [17, 33])
def test_rejected_full_step_vs_oracle(N, model_json, mmpc_mod, oracle):
    """the recipe of tests/test_gpu_group_iteration_trims.py (targets x 40 at N = 17, x 20 at N = 33, Delta-u weight /
    100, B = 8): some instance rejects alpha = 1 after its first iteration (asserted from the trace, column 5), so the
    one-stage alpha / 2 trials run after the paired fused trial, and the next iteration's phase A is evaluated"""
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
    assert np.array_equal(V.cpu().numpy(), g["V"]) and np.array_equal(iters, g["iters"])
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
    assert np.all(V0 != 0.0)
    s = _two_link(m, model_json, N, "exact", init_states=mode, max_iter=100)
    g = s.solve_batch_host(x0, up, tr, _w(), V=V0.copy())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), V=V0.copy(), hessian=oracle.HESS_EXACT, init_states=omode,
                           max_iter=100)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"init {init} N={N}")


@pytest.mark.parametrize("B", [6, 7])
def test_per_instance_weights_batch_not_a_multiple_of_four(B, model_json, mmpc_mod, oracle):
    """one row of weights per instance (weights_stride = nx + 2 nu) in a batch whose last wave is partly filled"""
    N = 33
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    rng = np.random.default_rng(SEED + B)
    w = _w()[None, :] * rng.uniform(0.5, 2.0, size=(B, 8))
    s = _two_link(mmpc_mod, model_json, N, "exact")
    g = s.solve_batch_host(x0, up, tr, w)
    o = oracle.solve_batch(N, H, x0, up, tr, w, hessian=oracle.HESS_EXACT)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    assert not np.array_equal(g["V"][0], g["V"][1])
    _same_as_oracle(g, o, f"per-instance weights B={B}")


def test_u0_into_host_memory(model_json, mmpc_mod, oracle):
    """u0, status and iteration counts written by the kernel straight into host memory, B = 7, N = 17: u0 is V's u_0 bit
    for bit and V is the oracle's"""
    import torch
    N, B, nx, nu = 17, 7, 4, 2
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), hessian=oracle.HESS_EXACT)
    s = _two_link(mmpc_mod, model_json, N, "exact")
    f64 = dict(dtype=torch.float64, device="cuda")
    dx0, dup, dtr, dw = (torch.tensor(a, **f64) for a in (x0, up, tr, _w()))
    V = torch.zeros((B, s.NV), **f64)
    hb = mmpc_mod.HostBuffer(B * (8 * nu + 8))
    u0h = hb.view(0, np.float64, B * nu)
    sth = hb.view(B * nu * 8, np.int32, B)
    ith = hb.view(B * nu * 8 + 4 * B, np.int32, B)
    u0h[:] = np.nan
    sth[:] = -1
    ith[:] = -1
    s.solve_batch(B, dx0, dup, dtr, dw, V, sth, ith, u0=u0h)
    torch.cuda.synchronize()
    g = {"V": V.cpu().numpy(), "status": np.array(sth), "iters": np.array(ith)}
    u0 = np.array(u0h).reshape(B, nu)
    hb.close()
    s.close()
    assert np.array_equal(u0, g["V"][:, nx:nx + nu])
    _same_as_oracle(g, o, "u0 into host memory")


# ---------------------------------------------------------------------------------------------- other paths
def test_linear_mode_vs_oracle(model_json, mmpc_mod, oracle):
    N, B = 17, 5
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    s = mmpc_mod.Solver(model_json(N=N, name="linear_double_pendulum", is_linear=True),
                        kkt_solver=mmpc_mod.KKT_RICCATI_GROUP)
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP
    g = s.solve_batch_host(x0, up, tr, _w())
    o = oracle.solve_batch(N, H, x0, up, tr, _w(), is_linear=True, solver=s)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, "linear mode N=17")


@pytest.mark.parametrize("variant", ["u-bounds", "x-bounds"])
def test_bounded_variants_vs_oracle(variant, model_json, mmpc_mod, oracle):
    m, N, B = mmpc_mod, 17, 5
    x0, up, tr = oracle.synth(SEED, 0, B, N, H)
    s = m.Solver(model_json(N=N), max_iter=100, kkt_solver=m.KKT_RICCATI_GROUP)
    if variant == "u-bounds":
        g = s.solve_batch_host(x0, up, tr, _w(), u_lb=UB[0], u_ub=UB[1])
        o = oracle.solve_batch(N, H, x0, up, tr, _w(), u_lb=UB[0], u_ub=UB[1], max_iter=100, solver=s)
    else:
        s.set_state_bounds(*VEL)
        g = s.solve_batch_host(x0, up, tr, _w())
        hess = {1: oracle.HESS_GAUSS_NEWTON, 2: oracle.HESS_EXACT}[s.hessian_for(B, False)]
        o = oracle.solve_batch(N, H, x0, up, tr, _w(), x_lb=VEL[0], x_ub=VEL[1], max_iter=100, hessian=hess)
    s.close()
    assert (o["status"] == 0).all(), o["status"]
    _same_as_oracle(g, o, f"{variant} N=17")
