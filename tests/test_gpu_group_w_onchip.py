"""On-chip W path of the 16-lane kernel: the unbounded exact-Hessian solve of the 2-link arm keeps the packed W_k
records in LDS, in the arrays (d / lam, dx, du) that are dead between the W pass and the step sweep.

Every case is the GPU solve against the CPU oracle running the same algorithm (the Hessian the solver resolves):
identical status and identical iteration counts on every instance, V* within 1e-10 relative to max|V|
(same algorithm).  The horizons are those at which the W pass and the Riccati reader change shape:
N = 1 (the peeled last stage alone), 2, 16 / 17 (one round of stages per lane against two), 30 (cfg#2), 32 / 33 (two
rounds against three: the W pass writes its records over lam of later stages, in rounds from the last one down) and
48 (three full rounds).  B = 6 is one full wave and one half-filled wave; groups with different iteration counts
share wave 0 (oracle: 3/3/3/4/3/3 iterations for N = 15..33, 4/3/3/4/4/4 at N = 48)."""
import numpy as np
import pytest

from conftest import WEIGHTS_CFG

pytestmark = pytest.mark.gpu

H = 0.002
SEED = 20250213
ITERS = {16: [3, 3, 3, 4, 3, 3], 17: [3, 3, 3, 4, 3, 3], 30: [3, 3, 3, 4, 3, 3], 32: [3, 3, 3, 4, 3, 3],
         33: [3, 3, 3, 4, 3, 3], 48: [4, 3, 3, 4, 4, 4]}


def _rel(a, b):
    return np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1e-300)


def _solver(mmpc_mod, model_json, N):
    s = mmpc_mod.Solver(model_json(N=N), kkt_solver=mmpc_mod.KKT_RICCATI_GROUP, hessian=mmpc_mod.HESSIAN_EXACT)
    return s


def _check(s, mmpc_mod, oracle, first, B, N, iters=None):
    assert s.kkt_solver_for(B) == mmpc_mod.KKT_RICCATI_GROUP and s.hessian_for(B, False) == mmpc_mod.HESSIAN_EXACT
    x0, up, tr = oracle.synth(SEED, first, B, N, H)
    w = np.array(WEIGHTS_CFG)
    g = s.solve_batch_host(x0, up, tr, w)
    oracle.exact_fallbacks()
    o = oracle.solve_batch(N, H, x0, up, tr, w, solver=s)
    assert oracle.exact_fallbacks() == 0 and (o["status"] == 0).all(), o["status"]
    if iters is not None:
        np.testing.assert_array_equal(o["iters"], iters)
    rel = _rel(g["V"], o["V"])
    print(f"N={N} B={B} first={first}: gpu iters {g['iters'].tolist() if B <= 8 else (g['iters'].min(), g['iters'].max())}"
          f" max rel diff {rel.max():.3e}")
    np.testing.assert_array_equal(g["status"], o["status"])
    np.testing.assert_array_equal(g["iters"], o["iters"])
    assert rel.max() <= 1e-10, rel.max()


@pytest.mark.parametrize("N", [1, 2, 16, 17, 30, 32, 33, 48])
def test_w_onchip_vs_oracle(N, model_json, mmpc_mod, oracle):
    s = _solver(mmpc_mod, model_json, N)
    _check(s, mmpc_mod, oracle, 0, 6, N, ITERS.get(N))
    s.close()


def test_w_onchip_repeated_launches(model_json, mmpc_mod, oracle):
    """Two launches on one handle with different instance blocks: the second must not depend on what the first left
    in the workspace (LDS is not kept between launches; the workspace stride of this variant is K | kff alone)."""
    s = _solver(mmpc_mod, model_json, 30)
    _check(s, mmpc_mod, oracle, 0, 64, 30)
    _check(s, mmpc_mod, oracle, 64, 64, 30)
    s.close()
