"""GPU: a generated model's library (cart-pole, lib/user/cart_pole.so) on the kernel variants it reaches only through
its own dispatcher: per-instance control bounds and Mehrotra's barrier rule.  B = 5: a partial 16-lane workgroup (four
instances per workgroup) and a partial lane wave.

1. pick test (the rule of tests/test_gpu_instance_bounds.py; needs no oracle): a batch solved with a [B, 1] array of
   bounds whose rows alternate between two boxes equals, instance by instance and bit for bit in V, status and
   iterations, the batch solved with that instance's box as shared bounds.  On the 16-lane and on the lane solver (the
   latter with the hand-over off, so that an instance's result depends on its own data alone).
2. Mehrotra's rule on the 16-lane solver under the state box of test_generated_model_state_bounds, max_iter = 100,
   against the oracle's rule 1: identical iteration counts, V* within 1e-10 relative (test_gpu_barrier_rule.py's
   tolerances); the lane solver refuses the rule.  Instance seed 0: the first of the seeds 0..19 of
   test_gpu_sx_models.instances at which the oracle alone converges on all five instances under both rules (all twenty
   do; checked on the CPU)."""
import numpy as np
import pytest

from test_gpu_sx_models import instances, solver, weights

pytestmark = pytest.mark.gpu
B = 5
BOXES = [(-1.5, 1.5), (-0.8, 2.5)]


@pytest.mark.parametrize("kkt", ["group", "riccati"])
def test_per_instance_bounds_pick_the_instances_own_box(kkt, mmpc_mod):
    m = mmpc_mod
    kw = dict(kkt_solver=m.KKT_RICCATI_GROUP) if kkt == "group" else dict(kkt_solver=m.KKT_RICCATI, tail_cap=0,
                                                                           tail_wave_max=0)
    s = solver(m, "cart_pole", **kw)
    x0, up, tr = instances(s.nx, s.nu, B, s.N, s.h, seed=11)
    tr *= 4.0   # targets the force bounds keep out of reach (test_generated_model_bounded)
    w = weights(s.nx, s.nu)
    lb = np.array([[BOXES[b % 2][0]] for b in range(B)])
    ub = np.array([[BOXES[b % 2][1]] for b in range(B)])
    g = s.solve_batch_host(x0, up, tr, w, u_lb=lb, u_ub=ub)
    shared = [s.solve_batch_host(x0, up, tr, w, u_lb=np.array([lo]), u_ub=np.array([hi])) for lo, hi in BOXES]
    s.close()
    assert (g["status"] == 0).all(), g["status"]
    U = g["V"][:, :-s.nx].reshape(B, s.N, s.nx + s.nu)[:, :, s.nx:]
    for b in range(B):
        lo, hi = BOXES[b % 2]
        assert U[b].min() >= lo and U[b].max() <= hi
        # its own box is active (on the CPU oracle too: instances 0, 3 at the lower bound, 1, 2, 4 at the upper)
        assert (np.abs(U[b] - lo) < 1e-12).any() or (np.abs(U[b] - hi) < 1e-12).any(), b
        for k in ("V", "status", "iters"):
            assert np.array_equal(g[k][b], shared[b % 2][k][b]), (b, k)
    assert not np.array_equal(shared[0]["V"], shared[1]["V"])   # the two boxes give different solves


def _state_bounded_inputs(s):
    x0, up, tr = instances(s.nx, s.nu, B, s.N, s.h, seed=0)
    x0[:, 0] = np.clip(x0[:, 0], -0.15, 0.15)
    x0[:, 3] = np.clip(x0[:, 3], -0.9, 0.9)
    return x0, up, tr * 3.0


XL, XU = np.array([-0.2, -np.inf, -np.inf, -1.0]), np.array([0.2, np.inf, np.inf, 1.0])


def test_mehrotra_on_the_group_solver_matches_oracle_rule1(mmpc_mod, oracle):
    m = mmpc_mod
    s = solver(m, "cart_pole", kkt_solver=m.KKT_RICCATI_GROUP, max_iter=100, barrier_rule=m.BARRIER_MEHROTRA)
    mid = oracle.use_user_model("cart_pole")
    s.set_state_bounds(XL, XU)
    x0, up, tr = _state_bounded_inputs(s)
    w = weights(s.nx, s.nu)
    g = s.solve_batch_host(x0, up, tr, w)
    o = {}
    for rule in (0, 1):
        try:
            oracle.set_ip_rule(rule)
            o[rule] = oracle.solve_batch(s.N, s.h, x0, up, tr, w, model=mid, x_lb=XL, x_ub=XU, max_iter=100)
        finally:
            oracle.set_ip_rule(0)
        assert (o[rule]["status"] == 0).all(), (rule, o[rule]["status"])   # what the seed was chosen for
    s.close()
    assert (g["status"] == 0).all(), g["status"]
    rel = np.abs(g["V"] - o[1]["V"]).max(axis=1) / np.abs(o[1]["V"]).max()
    print(f"iterations GPU {g['iters'].tolist()} oracle rule 1 {o[1]['iters'].tolist()} rule 0 {o[0]['iters'].tolist()}, "
          f"max rel diff {rel.max():.2e}")
    assert np.array_equal(g["iters"], o[1]["iters"])
    assert rel.max() < 1e-10, rel
    assert (o[1]["iters"] < o[0]["iters"]).all()   # the rule ran: the monotone rule takes about twice as many
    X = np.stack([g["V"][:, k * 5:k * 5 + 4] for k in range(1, s.N + 1)], 1)
    assert (X >= XL - 1e-12).all() and (X <= XU + 1e-12).all()
    assert (np.abs(np.abs(X[:, :, 0]) - 0.2) < 1e-6).any()   # the position bound is active somewhere


def test_mehrotra_on_the_lane_solver_is_refused(mmpc_mod):
    m = mmpc_mod
    s = solver(m, "cart_pole", kkt_solver=m.KKT_RICCATI, max_iter=100, barrier_rule=m.BARRIER_MEHROTRA)
    s.set_state_bounds(XL, XU)
    x0, up, tr = _state_bounded_inputs(s)
    with pytest.raises(m.MmpcError, match="MEHROTRA") as e:
        s.solve_batch_host(x0, up, tr, weights(s.nx, s.nu))
    assert e.value.code == -4   # MMPC_ERR_UNSUPPORTED
    s.close()
