"""GPU: the lane kernel's lean backward sweep (csrc/sqp_lane.h "(2') lean sweep") against its full sweep (2).  When every
lane of a wave leaves at an iteration's stop test, the backward sweep forms only the adjoint, the reduced gradient and
the stop test's quantities, and promises the full sweep's values bit for bit.  With the iteration-tail hand-over off the
lean sweep runs exactly at it == max_iter, so the same batch solved with max_iter = M (lean sweep at iteration M) and
with max_iter = M + 1 (full sweep at iteration M) must agree bitwise: in the iterates (trace rows 0 .. M-1, all columns)
and in what the lean sweep writes at row M (||2g||, ||c||, J, |c|_1, ||lam||), and run A's final residual is the
stop-test maximum of run B's row M.  B = 70 is one full wave and a 6-lane one; N >= 3 runs both arms (k >= 1, k = 0)
of a sweep that reads stages N-1 and N."""
import ctypes as C

import numpy as np
import pytest

from conftest import WEIGHTS_CFG

pytestmark = pytest.mark.gpu

H = 0.002
B = 70
M = 2
INF = np.inf
W_EXO = np.array([10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4)
ST_MAX_ITER = 1

# model, N, hessian, factor_fp32, state bounds
CASES = {
    "two_link-gn": ("two_link_arm", 3, "gn", 0, None),
    "two_link-xb": ("two_link_arm", 8, "gn", 0, ([-INF, -INF, -1.5, -1.5], [INF, INF, 1.5, 1.5])),
    "exo-gn": ("exo_arm", 4, "gn", 0, None),
    "exo-exact": ("exo_arm", 5, "exact", 0, None),
    "exo-fp32": ("exo_arm", 4, "gn", 1, None),
}


def _trace_solve(mmpc_mod, path, hess, fp32, xb, max_iter, x0, up, tr, w):
    import torch
    s = mmpc_mod.Solver(path, kkt_solver=2, hessian=hess, factor_fp32=fp32, init_states=mmpc_mod.INIT_ZERO,
                        max_iter=max_iter, tail_cap=0)
    if xb is not None:
        s.set_state_bounds(np.array(xb[0]), np.array(xb[1]))
    f64 = dict(dtype=torch.float64, device="cuda")
    t = [torch.tensor(a, **f64) for a in (x0, up, tr, w)]
    V = torch.zeros((B, s.NV), **f64)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    kk = torch.zeros(B, **f64)
    trace = torch.zeros((B, max_iter + 1, 8), **f64)
    L = s._L
    L.mmpc_debug_solve_trace.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 6
    rc = L.mmpc_debug_solve_trace(s._h, B, *(a.data_ptr() for a in t), 0, V.data_ptr(), st.data_ptr(),
                                  it.data_ptr(), kk.data_ptr(), trace.data_ptr(), None)
    assert rc == 0, L.mmpc_last_error()
    torch.cuda.synchronize()
    return dict(status=st.cpu().numpy(), iters=it.cpu().numpy(), kkt=kk.cpu().numpy(), trace=trace.cpu().numpy())


@pytest.mark.parametrize("case", list(CASES))
def test_lean_sweep_equals_full_sweep_bitwise(case, mmpc_mod, oracle, tmp_path):
    model, N, hess, fp32, xb = CASES[case]
    exo = model == "exo_arm"
    nx, nu = (8, 4) if exo else (4, 2)
    w = W_EXO if exo else np.array(WEIGHTS_CFG)
    x0, up, tr = oracle.synth(20250213, 0, B, N, H, model=oracle.EXO if exo else oracle.TWO_LINK)
    tr = np.ascontiguousarray(tr * 20.0)   # far targets: no instance converges within M iterations (asserted below)
    path = mmpc_mod.write_model_json(str(tmp_path / f"{model}_{N}.json"), model, nx, nu, 2000, N, model=model)
    h = mmpc_mod.HESSIAN_EXACT if hess == "exact" else mmpc_mod.HESSIAN_GAUSS_NEWTON
    a = _trace_solve(mmpc_mod, path, h, fp32, xb, M, x0, up, tr, w)       # lean sweep at iteration M
    b = _trace_solve(mmpc_mod, path, h, fp32, xb, M + 1, x0, up, tr, w)   # full sweep (2) at iteration M
    # the comparison leaves no instance out: every one reaches iteration M's stop test and stops there by the limit
    assert (a["status"] == ST_MAX_ITER).all(), np.bincount(a["status"])
    assert (a["iters"] == M).all() and (b["iters"] >= M).all()
    ta, tb = a["trace"], b["trace"]
    assert np.array_equal(ta[:, :M, :], tb[:, :M, :])   # the same iterates
    # ||2g||, ||c||, J, |c|_1, ||lam||: what the lean sweep writes.  A state-bounded solve's iteration goes on to put
    # the complementarity max |s z| into column 3 (trc[3] = cmpl0 after the line search), so run B's row M no longer
    # holds |c|_1 there: that column is compared through the stop test's residual below instead
    cols = [0, 1, 2, 3, 7] if xb is None else [0, 1, 2, 7]
    assert np.array_equal(ta[:, M, cols], tb[:, M, cols])
    assert np.isfinite(ta[:, M, cols]).all() and (ta[:, M, 0] > 0).all()
    kkt_b = np.maximum(tb[:, M, 0], tb[:, M, 1])
    if xb is not None:   # the lean stop test's residual includes the J-scale complementarity 2 max |s z|
        kkt_b = np.maximum(kkt_b, 2.0 * tb[:, M, 3])
    assert np.array_equal(a["kkt"], kkt_b)
