"""GPU: committed controls (mmpc_solve_batch_pinned) -- the first m controls of every instance fixed to
the caller's values, solved as the horizon-(N - m) problem from x_m.

Inputs throughout: oracle.synth(20250213, 0, B, N, 0.002), the weights of conftest.WEIGHTS_CFG (2-link arm) and of
test_gpu_xbounds.py (exo), pins u[b, k, j] = u_prev[b, j] + a (-1)^j (-1)^k with a = 0.25 (2-link arm) / 0.1 (exo).

Per shape (N, B, m), kernel and Hessian:
 1. the reduction, bit for bit: a second handle created with N' = N - m and the same options, solving x_m (as the pinned
    solve wrote it into V), u_{m-1}, traj[:, m:] and the same tail warm start, returns the tail of V, status, iters and
    kkt_res bit for bit;
 2. the oracle on those same inputs agrees with the tail by test_gpu_parity._compare (1e-10 where the iteration counts
    agree);
 3. the head: V[:, 0:nx] = x0, u_k = pin_k for k < m and u0_out = pin_0 bit for bit; the defects of the whole V are
    <= tol_defect by the oracle's nlp_eval (the head rows) and by the device nlp_eval;
 4. the full NLP, independent of the reduction: oracle.reduced_gradient on the full horizon at the returned controls
    is <= 1e-7 on every row k >= m (ten times tol_grad: the margin between the multiple-shooting iterate with defects
    <= 1e-10 and its single-shooting rollout; the CPU value of the same check is 9.5e-9) and its largest entry over
    the rows k < m is >= 0.5 on every instance (the pins bind: 0.69 .. 149 on the CPU).  A wrong u_prev', a traj
    shift off by one or a dropped pin moves a free row to O(1).
Then, once each: n_pin = 0, control bounds (shared and per instance; pins outside the box are kept), state bounds,
the lane kernel's hand-over, init_states, a NaN pin, the host and multi-device entries, a captured graph."""
import os

import numpy as np
import pytest

import oracle_lib as oracle
from conftest import WEIGHTS_CFG
from test_gpu_bounded_shapes import W_EXO, compare_xb, controls
from test_gpu_instance_bounds import rows
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

H = 0.002
SEED = 20250213
TOL_DEFECT = 1e-10
DIMS = {"two_link_arm": (4, 2), "exo_arm": (8, 4)}
OMODEL = {"two_link_arm": oracle.TWO_LINK, "exo_arm": oracle.EXO}
WEIGHTS = {"two_link_arm": np.array(WEIGHTS_CFG), "exo_arm": W_EXO}
AMP = {"two_link_arm": 0.25, "exo_arm": 0.1}

S_2L = [(3, 9, 1), (3, 9, 2), (17, 37, 1), (17, 37, 2), (17, 37, 16), (33, 65, 1), (33, 37, 32)]
S_EXO = [(7, 9, 1), (7, 9, 6), (21, 9, 2)]
CASES = (
    [("two_link_arm", N, B, m, "group", hess) for (N, B, m) in S_2L for hess in ("gn", "exact")]
    + [("two_link_arm", N, B, m, "lane", hess) for (N, B, m) in S_2L if N != 3 for hess in ("gn", "exact")]
    + [("two_link_arm", N, B, m, "condensed", "gn") for (N, B, m) in [(17, 37, 1), (17, 37, 16), (32, 6, 2)]]
    + [("exo_arm", N, B, m, kernel, hess) for kernel in ("group", "lane") for (N, B, m) in S_EXO
       for hess in ("gn", "exact")])
BASE = ("two_link_arm", 17, 37, 2)


def _id(case):
    return "-".join(str(v) for v in case)


def pins(model, up, m):
    """u[b, k, j] = u_prev[b, j] + a (-1)^j (-1)^k"""
    nu = up.shape[1]
    sj = (-1.0) ** np.arange(nu)
    sk = (-1.0) ** np.arange(m)
    return np.ascontiguousarray(up[:, None, :] + AMP[model] * sk[None, :, None] * sj[None, None, :])


def warm_start(x0, up, N):
    """a warm start that is nonzero and different at every index: the measured state and the previous control held over
    the horizon, plus 0.01 sin(i + b)"""
    B, nx = x0.shape
    nu = up.shape[1]
    V = np.concatenate([np.tile(np.concatenate([x0, up], 1), (1, N)), x0], 1)
    i = np.arange(V.shape[1])[None, :] + np.arange(B)[:, None]
    return V + 0.01 * np.sin(i)


class Ctx:
    def __init__(self, m, d):
        self.m, self.dir = m, d
        self.inputs_ = {}

    def inputs(self, model, N, B, clip=None):
        key = (model, N, B, clip)
        if key not in self.inputs_:
            nx, _ = DIMS[model]
            x0, up, tr = oracle.synth(SEED, 0, B, N, H, model=OMODEL[model])
            if clip is not None:
                x0[:, nx // 2:] = np.clip(x0[:, nx // 2:], -clip, clip)
            for a in (x0, up, tr):
                a.setflags(write=False)
            self.inputs_[key] = (x0, up, tr)
        return self.inputs_[key]

    def solver(self, model, N, kernel, hess, tail="off", **kw):
        m = self.m
        nx, nu = DIMS[model]
        p = m.write_model_json(os.path.join(self.dir, f"{model}_{N}.json"), f"{model}_{N}", nx, nu, 2000, N, model=model)
        ks = {"group": m.KKT_RICCATI_GROUP, "lane": m.KKT_RICCATI, "condensed": m.KKT_CONDENSED}[kernel]
        hs = {"gn": m.HESSIAN_GAUSS_NEWTON, "exact": m.HESSIAN_EXACT}[hess]
        if kernel == "lane" and tail == "off":
            kw.update(tail_cap=0, tail_wave_max=0)
        return m.Solver(p, kkt_solver=ks, hessian=hs, **kw)


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return Ctx(mmpc_mod, str(tmp_path_factory.mktemp("pinned")))


def dev(a, dtype=None):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def dev_solve(s, x0, up, tr, w, V0, pin=None, lb=None, ub=None, stride=0, entry="python"):
    """a device-pointer solve through mmpc_solve_batch_pinned (pin given) or Solver.solve_batch, from V0 into fresh
    outputs; entry = "pinned0": mmpc_solve_batch_pinned with n_pin = 0 and a NULL u_pin"""
    import torch
    B = x0.shape[0]
    V, st, it = dev(V0), dev(np.full(B, -1), torch.int32), dev(np.zeros(B), torch.int32)
    kk, u0 = dev(np.zeros(B)), dev(np.full((B, s.nu), -7.0))
    d = lambda a: None if a is None else dev(a)   # noqa: E731
    dx0, dup, dtr, dw, dlb, dub = dev(x0), dev(up), dev(tr), dev(w), d(lb), d(ub)
    if entry == "pinned0":
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        s._check(s._L.mmpc_solve_batch_pinned(s._h, B, p(dx0), p(dup), p(dtr), p(dw), 0, p(dlb), p(dub), stride, None,
                                              0, p(V), p(st), p(it), p(kk), p(u0), None))
    elif pin is None:
        s.solve_batch(B, dx0, dup, dtr, dw, V, st, it, kk, u_lb=dlb, u_ub=dub, bounds_stride=stride, u0=u0)
    else:
        s.solve_batch(B, dx0, dup, dtr, dw, V, st, it, kk, u_lb=dlb, u_ub=dub, bounds_stride=stride, u0=u0,
                      u_pin=dev(pin), n_pin=pin.shape[1])
    torch.cuda.synchronize()
    return dict(V=V.cpu().numpy(), status=st.cpu().numpy(), iters=it.cpu().numpy(), kkt=kk.cpu().numpy(),
                u0=u0.cpu().numpy())


def same_bits(a, b, keys=("V", "status", "iters", "kkt"), idx=slice(None), msg=""):
    for k in keys:
        np.testing.assert_array_equal(a[k][idx], b[k][idx], err_msg=f"{msg} {k}")


def tail_of(g, m, nd):
    return dict(V=g["V"][:, m * nd:], status=g["status"], iters=g["iters"], kkt=g["kkt"])


def check_head(g, x0, pin, nx, nu):
    m = pin.shape[1]
    nd = nx + nu
    np.testing.assert_array_equal(g["V"][:, :nx], x0)
    for k in range(m):
        np.testing.assert_array_equal(g["V"][:, k * nd + nx:(k + 1) * nd], pin[:, k])
    np.testing.assert_array_equal(g["u0"], pin[:, 0])


def check_full_nlp(name, g, model, N, m, x0, up, tr, w):
    """property 4 of the module docstring, and the head defects by the oracle"""
    nx, nu = DIMS[model]
    U = controls(g["V"], N, nx, nu)
    free = pinned = None
    for b in range(x0.shape[0]):
        _, gd = oracle.nlp_eval(N, H, g["V"][b], up[b], tr[b], w, model=OMODEL[model])
        assert np.abs(gd[:m * nx]).max() <= TOL_DEFECT, (name, b, np.abs(gd[:m * nx]).max())
        r = np.abs(oracle.reduced_gradient(N, H, x0[b], U[b], up[b], tr[b], w, model=OMODEL[model])).reshape(N, nu)
        fb, pb = r[m:].max(), r[:m].max()
        free = fb if free is None else max(free, fb)
        pinned = pb if pinned is None else min(pinned, pb)
        assert fb <= 1e-7, (name, b, fb)
        assert pb >= 0.5, (name, b, pb)
    print(f"{name}: reduced gradient: free rows <= {free:.2e}, pinned rows >= {pinned:.2f}")


def device_defects(s, g, up, tr, w):
    import torch
    B = up.shape[0]
    J, gi = dev(np.zeros(B)), dev(np.full(B, 9.0))
    s.nlp_eval(B, dev(g["V"]), dev(up), dev(tr), dev(w), J, gi)
    torch.cuda.synchronize()
    return gi.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pinned_solve(case, ctx):
    model, N, B, m, kernel, hess = case
    name = _id(case)
    nx, nu = DIMS[model]
    nd = nx + nu
    x0, up, tr = ctx.inputs(model, N, B)
    w = WEIGHTS[model]
    pin = pins(model, up, m)
    V0 = warm_start(x0, up, N)
    s = ctx.solver(model, N, kernel, hess)
    g = dev_solve(s, x0, up, tr, w, V0, pin)
    print(f"{name}: iterations {g['iters'].min()}-{g['iters'].max()}, status {np.unique(g['status'])}")
    assert (g["status"] == 0).all(), (name, g["status"])
    # 3. the head
    check_head(g, x0, pin, nx, nu)
    gi = device_defects(s, g, up, tr, w)
    assert gi.max() <= TOL_DEFECT, (name, gi.max())
    # 1. the reduction, bit for bit
    xm = np.ascontiguousarray(g["V"][:, m * nd:m * nd + nx])
    upm = np.ascontiguousarray(pin[:, m - 1])
    trm = np.ascontiguousarray(tr[:, m:])
    V0m = np.ascontiguousarray(V0[:, m * nd:])
    s2 = ctx.solver(model, N - m, kernel, hess)
    g2 = dev_solve(s2, xm, upm, trm, w, V0m)
    same_bits(tail_of(g, m, nd), g2, msg=name)
    # 2. the oracle on the same inputs
    o = oracle.solve_batch(N - m, H, xm, upm, trm, w, V=V0m, model=OMODEL[model], solver=s2)
    _compare(tail_of(g, m, nd), o)
    # 4. the full NLP
    check_full_nlp(name, g, model, N, m, x0, up, tr, w)
    s.close()
    s2.close()


@pytest.fixture(scope="module")
def base(ctx):
    """the once-each tests' shape, 2-link (17, 37, 2): inputs, pins, warm start"""
    model, N, B, m = BASE
    x0, up, tr = ctx.inputs(model, N, B)
    return dict(model=model, N=N, B=B, m=m, x0=x0, up=up, tr=tr, w=WEIGHTS[model], pin=pins(model, up, m),
                V0=warm_start(x0, up, N))


def test_n_pin_zero_is_the_bounds_entry(ctx, base):
    b = base
    lb, ub = np.array([-2.0, -2.0]), np.array([2.0, 2.0])
    for kw in (dict(), dict(lb=lb, ub=ub)):
        s = ctx.solver(b["model"], b["N"], "group", "gn")
        a = dev_solve(s, b["x0"], b["up"], b["tr"], b["w"], b["V0"], entry="pinned0", **kw)
        r = dev_solve(s, b["x0"], b["up"], b["tr"], b["w"], b["V0"], **kw)
        same_bits(a, r, keys=("V", "status", "iters", "kkt", "u0"))
        assert (r["status"] == 0).all()
        s.close()


def tail_inputs(b, g):
    nx, nu = DIMS[b["model"]]
    nd, m = nx + nu, b["m"]
    return (np.ascontiguousarray(g["V"][:, m * nd:m * nd + nx]), np.ascontiguousarray(b["pin"][:, m - 1]),
            np.ascontiguousarray(b["tr"][:, m:]), np.ascontiguousarray(b["V0"][:, m * nd:]))


@pytest.mark.parametrize("table", ["shared", "per_instance"])
def test_control_bounds_keep_the_pins_outside_the_box(table, ctx, base):
    """shared +-2 Nm, and a [B, nu] table of pattern b % 4 (test_gpu_instance_bounds.rows): the tail against the oracle
    (per instance for the table, as that module does); the pins run outside the box and are kept"""
    b = base
    model, N, B, m = b["model"], b["N"], b["B"], b["m"]
    nx, nu = DIMS[model]
    nd = nx + nu
    if table == "shared":
        lb, ub, stride = np.array([-2.0, -2.0]), np.array([2.0, 2.0]), 0
        lbr, ubr = np.tile(lb, (B, 1)), np.tile(ub, (B, 1))
    else:
        lb, ub = rows(model, False, B)
        lbr, ubr, stride = lb, ub, nu
    s = ctx.solver(model, N, "group", "gn")
    g = dev_solve(s, b["x0"], b["up"], b["tr"], b["w"], b["V0"], b["pin"], lb=lb, ub=ub, stride=stride)
    assert (g["status"] == 0).all(), g["status"]
    check_head(g, b["x0"], b["pin"], nx, nu)
    outside = (b["pin"] < lbr[:, None, :]) | (b["pin"] > ubr[:, None, :])
    assert outside.any(), "the pins were meant to lie outside the box"
    U = controls(g["V"], N, nx, nu)
    assert (U[:, m:] >= lbr[:, None, :]).all() and (U[:, m:] <= ubr[:, None, :]).all()
    xm, upm, trm, V0m = tail_inputs(b, g)
    s2 = ctx.solver(model, N - m, "group", "gn")
    if table == "shared":
        o = oracle.solve_batch(N - m, H, xm, upm, trm, b["w"], V=V0m, u_lb=lb, u_ub=ub, solver=s2)
    else:
        o = dict(V=np.zeros_like(V0m), status=np.zeros(B, np.int32), iters=np.zeros(B, np.int32))
        for i in range(B):
            oi = oracle.solve_batch(N - m, H, xm[i:i + 1], upm[i:i + 1], trm[i:i + 1], b["w"], V=V0m[i:i + 1],
                                    u_lb=lb[i], u_ub=ub[i], solver=s2, hessian=oracle.HESS_GAUSS_NEWTON)
            for k in ("V", "status", "iters"):
                o[k][i] = oi[k][0]
    _compare(tail_of(g, m, nd), o)
    on = int(((U[:, m:] == lbr[:, None, :]) | (U[:, m:] == ubr[:, None, :])).sum())
    print(f"{table}: {on} free controls on a bound, pins {b['pin'].min():.2f} .. {b['pin'].max():.2f}")
    assert on >= 1
    s.close()
    s2.close()


def xb_case(ctx, model, N, B, m, kernel, xl, xu, clip, ul=None, uu=None):
    """a pinned solve under state (and control) bounds against the oracle's interior point on the tail problem"""
    nx, nu = DIMS[model]
    nd = nx + nu
    x0, up, tr = ctx.inputs(model, N, B, clip)
    w = WEIGHTS[model]
    pin = pins(model, up, m)
    V0 = warm_start(x0, up, N)
    s = ctx.solver(model, N, kernel, "gn", max_iter=100)
    if xl is not None:
        s.set_state_bounds(np.array(xl), np.array(xu))
    arr = lambda v: None if v is None else np.array(v, dtype=np.float64)   # noqa: E731
    g = dev_solve(s, x0, up, tr, w, V0, pin, lb=arr(ul), ub=arr(uu))
    check_head(g, x0, pin, nx, nu)
    xm = np.ascontiguousarray(g["V"][:, m * nd:m * nd + nx])
    o = oracle.solve_batch(N - m, H, xm, pin[:, m - 1], tr[:, m:], w, V=V0[:, m * nd:], x_lb=arr(xl), x_ub=arr(xu),
                           u_lb=arr(ul), u_ub=arr(uu), max_iter=100, model=OMODEL[model],
                           hessian=oracle.HESS_GAUSS_NEWTON, bound_release=(kernel == "group"))
    s.close()
    return tail_of(g, m, nd), o


@pytest.mark.parametrize("kernel", ["group", "lane"])
def test_state_bounds(kernel, ctx):
    """|qdot| <= 0.5 with the measured velocities clipped to 0.45, both Riccati kernels"""
    model, N, B, m = BASE
    inf = np.inf
    g, o = xb_case(ctx, model, N, B, m, kernel, [-inf, -inf, -0.5, -0.5], [inf, inf, 0.5, 0.5], 0.45)
    compare_xb(f"xb-{kernel}", g, o)


@pytest.mark.parametrize("bounds", ["u_box", "qdot"])
def test_exo_bounds(bounds, ctx):
    """exo (7, 9, 1) with its control box, and with |qdot| <= 0.3 (velocities clipped to 0.25)"""
    inf = np.inf
    if bounds == "u_box":
        g, o = xb_case(ctx, "exo_arm", 7, 9, 1, "group", None, None, None, [-0.5, -1.0, -0.5, -0.3],
                       [0.6, 0.5, 1.0, 0.3])
        _compare(g, o)
    else:
        g, o = xb_case(ctx, "exo_arm", 7, 9, 1, "group", [-inf] * 4 + [-0.3] * 4, [inf] * 4 + [0.3] * 4, 0.25)
        compare_xb("exo-qdot", g, o)
    assert (g["status"] == 0).all()


def test_lane_default_hand_over_policy(ctx, base):
    """the lane kernel under the default hand-over policy (memset, lane launch, resume launch at horizon N - m) against
    tail_cap = 0: the same solutions to 1e-10"""
    b = base
    off = ctx.solver(b["model"], b["N"], "lane", "gn")
    on = ctx.solver(b["model"], b["N"], "lane", "gn", tail="default")
    a = dev_solve(off, b["x0"], b["up"], b["tr"], b["w"], b["V0"], b["pin"])
    c = dev_solve(on, b["x0"], b["up"], b["tr"], b["w"], b["V0"], b["pin"])
    assert (a["status"] == 0).all() and (c["status"] == 0).all()
    rel = np.abs(a["V"] - c["V"]).max(1) / np.abs(a["V"]).max(1)
    assert rel.max() <= 1e-10, rel.max()
    off.close()
    on.close()


@pytest.mark.parametrize("init", ["hold_x0", "zero"])
def test_init_states_apply_to_the_tail(init, ctx, base, mmpc_mod):
    """HOLD_X0 holds the tail at x_m, ZERO zeroes it (V is not read: NaN there changes nothing): the same KKT point as
    the given warm start to 1e-7 (tests/test_gpu_init.py), and bit for bit the second handle's solve"""
    b = base
    model, N, m = b["model"], b["N"], b["m"]
    nx, nu = DIMS[model]
    nd = nx + nu
    mode = mmpc_mod.INIT_HOLD_X0 if init == "hold_x0" else mmpc_mod.INIT_ZERO
    ref = ctx.solver(model, N, "group", "gn")
    r = dev_solve(ref, b["x0"], b["up"], b["tr"], b["w"], b["V0"], b["pin"])
    s = ctx.solver(model, N, "group", "gn", init_states=mode)
    V0 = np.full_like(b["V0"], np.nan) if init == "zero" else b["V0"]
    g = dev_solve(s, b["x0"], b["up"], b["tr"], b["w"], V0, b["pin"])
    assert (g["status"] == 0).all() and (r["status"] == 0).all()
    assert np.abs(g["V"] - r["V"]).max() / np.abs(r["V"]).max() < 1e-7
    check_head(g, b["x0"], b["pin"], nx, nu)
    xm, upm, trm, V0m = tail_inputs(b, g)
    s2 = ctx.solver(model, N - m, "group", "gn", init_states=mode)
    g2 = dev_solve(s2, xm, upm, trm, b["w"], np.full_like(V0m, np.nan) if init == "zero" else V0m)
    same_bits(tail_of(g, m, nd), g2, msg=init)
    for x in (ref, s, s2):
        x.close()


def test_nan_pin_stays_in_its_instance(ctx, base):
    b = base
    bad = 5
    s = ctx.solver(b["model"], b["N"], "group", "gn")
    clean = dev_solve(s, b["x0"], b["up"], b["tr"], b["w"], b["V0"], b["pin"])
    pin = b["pin"].copy()
    pin[bad, 0, 1] = np.nan
    g = dev_solve(s, b["x0"], b["up"], b["tr"], b["w"], b["V0"], pin)
    assert g["status"][bad] != 0, g["status"][bad]
    others = np.arange(b["B"]) != bad
    same_bits(g, clean, keys=("V", "status", "iters", "kkt", "u0"), idx=others)
    assert (clean["status"] == 0).all()
    s.close()


def test_host_entry(ctx, base):
    b = base
    s = ctx.solver(b["model"], b["N"], "group", "gn")
    d = dev_solve(s, b["x0"], b["up"], b["tr"], b["w"], b["V0"], b["pin"])
    hst = s.solve_batch_host(b["x0"], b["up"], b["tr"], b["w"], V=b["V0"], u_pin=b["pin"])
    same_bits(hst, d)
    assert (hst["status"] == 0).all()
    s.close()


def test_two_shards_on_one_device(ctx, base, mmpc_mod):
    """devices [0, 0], B = 5 (shards of 2 and 3): each shard gets its own rows of the pins; bit for bit the single
    handle's solve"""
    b = base
    B = 5
    s = ctx.solver(b["model"], b["N"], "group", "gn")
    args = [b[k][:B] for k in ("x0", "up", "tr")] + [b["w"]]
    one = s.solve_batch_host(*args, V=b["V0"][:B], u_pin=b["pin"][:B])
    path = os.path.join(ctx.dir, f"{b['model']}_{b['N']}.json")
    ms = mmpc_mod.MultiSolver(path, [0, 0], kkt_solver=mmpc_mod.KKT_RICCATI_GROUP,
                              hessian=mmpc_mod.HESSIAN_GAUSS_NEWTON)
    two = ms.solve_batch_host(*args, V=b["V0"][:B], u_pin=b["pin"][:B])
    same_bits(two, one)
    assert (one["status"] == 0).all()
    nx, nu = DIMS[b["model"]]
    np.testing.assert_array_equal(two["V"][:, nx:nx + nu], b["pin"][:B, 0])
    s.close()
    ms.close()


def test_pinned_solve_replays_from_a_graph(ctx, base):
    """after reserve_workspace(B) a pinned solve allocates nothing: captured, it replays bit for bit, and with new pins
    written into the same buffer it solves the new pins"""
    import torch
    b = base
    B, m = b["B"], b["m"]
    s = ctx.solver(b["model"], b["N"], "group", "gn")
    s.reserve_workspace(B)
    x0, up, tr, w, pin = (dev(b[k]) for k in ("x0", "up", "tr", "w", "pin"))
    V0 = dev(b["V0"])

    def outputs():
        return (V0.clone(), dev(np.full(B, -1), torch.int32), dev(np.zeros(B), torch.int32), dev(np.zeros(B)))

    u0e, u0g = dev(np.zeros((B, s.nu))), dev(np.zeros((B, s.nu)))

    def eager():
        o = outputs()
        s.solve_batch(B, x0, up, tr, w, *o, u0=u0e, u_pin=pin, n_pin=m)
        torch.cuda.synchronize()
        return [t.clone() for t in o] + [u0e.clone()]

    ref = eager()
    assert (ref[1] == 0).all()
    g_out = outputs()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):   # one solve on the capture stream before capturing (module load)
        s.solve_batch(B, x0, up, tr, w, *g_out, u0=u0g, u_pin=pin, n_pin=m, stream=cs.cuda_stream)
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    g_out[0].copy_(V0)
    with torch.cuda.graph(g, stream=cs):
        s.solve_batch(B, x0, up, tr, w, *g_out, u0=u0g, u_pin=pin, n_pin=m, stream=cs.cuda_stream)

    def replay():
        g_out[0].copy_(V0)
        for t in g_out[1:]:
            t.fill_(0)
        u0g.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        return list(g_out) + [u0g]

    for _ in range(2):
        for a, r in zip(replay(), ref):
            assert torch.equal(a, r)
    pin.copy_(dev(-b["pin"]))   # new pins in the same buffer
    torch.cuda.synchronize()
    ref2 = eager()
    assert not torch.equal(ref2[0], ref[0])
    for a, r in zip(replay(), ref2):
        assert torch.equal(a, r)
    s.close()
