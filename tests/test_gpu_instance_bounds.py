"""GPU: per-instance control bounds (mmpc_*_bounds, bounds_stride) through the kernels, the lane-to-16-lane hand-over,
the host and multi-device entries and a captured graph.

Inputs follow tests/test_gpu_bounded_shapes.py: seed 20250213, oracle.synth(first = 500) for the 2-link arm and 900 for
the exo in the control-bound cases, first = 0 with that module's velocity clips in the state-bound cases, h = 0.002,
that module's weights, max_iter = 100.  Instance b gets bound pattern b % 4.

1. pick test (needs no oracle): a batch solved once with per-instance bounds must equal, instance by instance and bit
   for bit in V, status, iterations and kkt_res, the batch solved with pattern b % 4 as SHARED bounds through the old
   entry point.  The kernels' results depend only on the instance's own data (lane solves run with the hand-over off),
   so any difference is an indexing or staging defect.  Shapes: partial workgroups (B = 5, 9, 37 at four instances per
   workgroup), a second and a partial wave on the lane kernel (B = 65, 37).  Also a padded stride with NaN padding in
   an exact-size buffer, B equal rows against the shared solve, and u_ub = NULL against u_ub = +inf.
2. hand-over: 2-link lane solves at (N, B) = (17, 5) under the default tail policy, where the wave rule hands the
   instances that outlast the first to converge (four, three under state bounds) to the resume launch, with bounds
   that differ from instance to instance: 1e-10 relative in V* against the
   same solve with the hand-over off (the hand-over's documented agreement).  A resume launch that indexes the bounds
   by its slot fails this.
3. oracle: per-instance batches against the CPU oracle called once per instance with that instance's bounds, under
   test_gpu_bounded_shapes.py's parity criterion unchanged; every control inside its own instance's box exactly.
4. other layers: solve_batch_host with [B, nu] bounds, MultiSolver over device 0 listed twice (shard offsets), the RCCL
   entry at one rank with a strided exact-size buffer, and a captured graph."""
import numpy as np
import pytest

import oracle_lib as oracle
from test_gpu_bounded_shapes import (DIMS, H, INF, OMODEL, SEED, UB_FIRST, WEIGHTS, XB, Ctx, arr, compare_ub,
                                     compare_xb, controls)
from test_gpu_parity import _rel

pytestmark = pytest.mark.gpu

BIG = 1e31   # |b| >= 1e19 is infinite: the reference's default limits
# control-bound patterns (instance b: pattern b % 4)
CB = {
    "two_link_arm": [([-2.0, -1.6], [1.8, 2.0]), ([-INF, -1.0], [1.0, INF]), ([-0.5] * 2, [0.5] * 2),
                     ([-BIG] * 2, [BIG] * 2)],
    "exo_arm": [([-0.5, -1.0, -0.5, -0.3], [0.6, 0.5, 1.0, 0.3]), ([-INF, -0.5, -INF, -0.3], [0.5, INF, 0.5, INF]),
                ([-0.2] * 4, [0.2] * 4), ([-BIG] * 4, [BIG] * 4)],
}
# control patterns under state bounds: one-sided boxes for the 2-link arm's `mixed` state box (two-sided control boxes
# leave the interior point at max_iter there, on the oracle as well); the exo keeps its four under `one_sided`
XCB = {
    "two_link_arm": [([-1.0, -INF], [INF, 1.0]), ([-1.5, -INF], [INF, 1.5]), ([-BIG] * 2, [BIG] * 2),
                     ([-1.0, -INF], [INF, 1.0])],
    "exo_arm": CB["exo_arm"],
}
XPAT = {"two_link_arm": "mixed", "exo_arm": "one_sided"}

SHAPES_2L_GROUP = [(1, 5), (3, 9), (17, 37), (33, 37)]
SHAPES_2L_LANE = [(2, 65), (17, 37)]
SHAPES_EXO = [(1, 5), (7, 9)]
# (model, N, B, kernel, hessian, state-bounded, barrier rule)
PICK = (
    [("two_link_arm", N, B, "condensed", "auto", False, 0) for (N, B) in SHAPES_2L_GROUP if N <= 32]
    + [("two_link_arm", N, B, "lane", "gn", xb, 0) for xb in (False, True) for (N, B) in SHAPES_2L_LANE]
    + [("exo_arm", N, B, "lane", "gn", xb, 0) for xb in (False, True) for (N, B) in SHAPES_EXO]
    + [(model, N, B, "group", hess, False, 0) for hess in ("gn", "exact")
       for model, shapes in (("two_link_arm", SHAPES_2L_GROUP), ("exo_arm", SHAPES_EXO)) for (N, B) in shapes]
    + [(model, N, B, "group", "gn", True, rule) for rule in (0, 1)
       for model, shapes in (("two_link_arm", SHAPES_2L_GROUP), ("exo_arm", SHAPES_EXO)) for (N, B) in shapes])


def _id(case):
    model, N, B, kernel, hess, xb, rule = case
    return f"{model}-{N}-{B}-{kernel}-{hess}" + ("-xb" if xb else "") + ("-mehrotra" if rule else "")


def patterns(model, xb):
    return (XCB if xb else CB)[model]


def rows(model, xb, B):
    """[B, nu] bounds: instance b gets pattern b % 4"""
    pats = patterns(model, xb)
    lb = np.array([pats[b % 4][0] for b in range(B)], dtype=np.float64)
    ub = np.array([pats[b % 4][1] for b in range(B)], dtype=np.float64)
    return lb, ub


class Dev:
    """device-pointer solves of one case: inputs uploaded once, every solve from a zero V into fresh outputs"""

    def __init__(self, ctx, case, tail="off", **kw):
        import torch
        self.torch = torch
        model, N, B, kernel, hess, xb, rule = case
        self.model, self.N, self.B, self.xb = model, N, B, xb
        clip = XB[model][XPAT[model]][4] if xb else None
        self.inputs = ctx.inputs(model, 0 if xb else UB_FIRST[model], N, B, clip)
        self.s = ctx.solver(model, N, kernel, hess, tail, **kw)
        if xb:
            xl, xu = XB[model][XPAT[model]][:2]
            self.s.set_state_bounds(arr(xl), arr(xu))
            self.s.set_barrier_rule(rule)
        ctx.check_resolved(self.s, kernel, "gn" if hess == "auto" else hess, B, True)
        self.x0, self.up, self.tr = (self.d(a) for a in self.inputs)
        self.w = self.d(WEIGHTS[model])

    def d(self, a):
        return self.torch.tensor(np.ascontiguousarray(a), dtype=self.torch.float64, device="cuda")

    def solve(self, lb, ub, stride=0, stream=None, out=None):
        """lb / ub: device tensors or None"""
        t, B = self.torch, self.B
        if out is None:
            out = (t.zeros((B, self.s.NV), dtype=t.float64, device="cuda"),
                   t.full((B,), -1, dtype=t.int32, device="cuda"), t.zeros(B, dtype=t.int32, device="cuda"),
                   t.zeros(B, dtype=t.float64, device="cuda"))
        self.s.solve_batch(B, self.x0, self.up, self.tr, self.w, *out, u_lb=lb, u_ub=ub, bounds_stride=stride,
                           stream=stream)
        if stream is None:
            t.cuda.synchronize()
        return out

    def result(self, out):
        V, st, it, kk = (o.cpu().numpy() for o in out)
        return dict(V=V, status=st, iters=it, kkt=kk)

    def close(self):
        self.s.close()


def assert_same_bits(a, b, idx=slice(None), jdx=None, msg=""):
    jdx = idx if jdx is None else jdx
    for k in ("V", "status", "iters", "kkt"):
        np.testing.assert_array_equal(a[k][idx], b[k][jdx], err_msg=f"{msg} {k}")


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return Ctx(mmpc_mod, str(tmp_path_factory.mktemp("instance_bounds")))


# ---- 1. pick test ----
@pytest.mark.parametrize("case", PICK, ids=_id)
def test_per_instance_solve_picks_the_shared_solves(case, ctx):
    model, N, B, kernel, hess, xb, rule = case
    dv = Dev(ctx, case)
    lb, ub = rows(model, xb, B)
    per = dv.result(dv.solve(dv.d(lb), dv.d(ub), stride=DIMS[model][1]))
    nact = 0
    for p, (pl, pu) in enumerate(patterns(model, xb)):
        shared = dv.result(dv.solve(dv.d(pl), dv.d(pu)))   # the old entry point, device [nu]
        idx = np.arange(p, B, 4)
        assert_same_bits(per, shared, idx, msg=f"{_id(case)} pattern {p}")
        U = controls(shared["V"], N, *DIMS[model])[idx]
        nact += int(((U == arr(pl)) | (U == arr(pu))).sum())
    dv.close()
    print(f"{_id(case)}: statuses {np.bincount(per['status'])}, iterations {per['iters'].min()}-{per['iters'].max()}, "
          f"{nact} controls on a bound")
    assert (per["status"] >= 0).all() and (per["iters"] >= 1).all()   # every instance was written by the solve


EDGE = [("two_link_arm", 17, 37, "condensed", "auto", False, 0), ("two_link_arm", 17, 37, "lane", "gn", False, 0),
        ("two_link_arm", 17, 37, "group", "gn", False, 0), ("two_link_arm", 17, 37, "group", "exact", False, 0),
        ("two_link_arm", 17, 37, "lane", "gn", True, 0), ("exo_arm", 7, 9, "group", "gn", True, 0),
        ("exo_arm", 7, 9, "group", "gn", True, 1)]


@pytest.mark.parametrize("case", EDGE, ids=_id)
def test_stride_padding_equal_rows_and_null_upper(case, ctx):
    model, N, B, kernel, hess, xb, rule = case
    nu = DIMS[model][1]
    dv = Dev(ctx, case)
    t = dv.torch
    lb, ub = rows(model, xb, B)
    per = dv.result(dv.solve(dv.d(lb), dv.d(ub), stride=nu))
    # bounds_stride = nu + 1, NaN in the padding column, buffers of exactly (B - 1) stride + nu doubles
    st = nu + 1
    pad = []
    for a in (lb, ub):
        full = np.full((B, st), np.nan)
        full[:, :nu] = a
        pad.append(dv.d(full.reshape(-1)[:(B - 1) * st + nu]))
        assert pad[-1].numel() == (B - 1) * st + nu
    assert_same_bits(per, dv.result(dv.solve(pad[0], pad[1], stride=st)), msg="padded stride")
    # B equal rows reproduce the shared solve
    pl, pu = patterns(model, xb)[0]
    shared = dv.result(dv.solve(dv.d(pl), dv.d(pu)))
    eq = dv.result(dv.solve(dv.d(np.tile(arr(pl), (B, 1))), dv.d(np.tile(arr(pu), (B, 1))), stride=nu))
    assert_same_bits(eq, shared, msg="equal rows")
    # u_ub = NULL with per-instance u_lb equals u_ub = +inf
    null = dv.result(dv.solve(dv.d(lb), None, stride=nu))
    infu = dv.result(dv.solve(dv.d(lb), t.full((B, nu), BIG, dtype=t.float64, device="cuda"), stride=nu))
    assert_same_bits(null, infu, msg="null upper")
    dv.close()


# ---- 2. hand-over ----
def handover_rows(xb, B):
    """instance 0 on pattern 0, the rest on pattern 1 shifted a little per instance: no two rows are equal, so a row
    picked by the resume launch's slot instead of the instance is a different box whatever the claim order"""
    pats = patterns("two_link_arm", xb)
    lb = np.array([pats[0][0]] + [pats[1][0]] * (B - 1), dtype=np.float64)
    ub = np.array([pats[0][1]] + [pats[1][1]] * (B - 1), dtype=np.float64)
    for b in range(1, B):
        lb[b] -= 0.01 * b    # infinite entries stay infinite
        ub[b] += 0.01 * b
    return lb, ub


@pytest.mark.parametrize("xb", [False, True], ids=["control", "state+control"])
def test_handed_over_instances_keep_their_own_bounds(xb, ctx):
    case = ("two_link_arm", 17, 5, "lane", "gn", xb, 0)
    lb, ub = handover_rows(xb, 5)
    off_dv = Dev(ctx, case)
    off = off_dv.result(off_dv.solve(off_dv.d(lb), off_dv.d(ub), stride=2))
    off_dv.close()
    on_dv = Dev(ctx, case, tail="default")
    on = on_dv.result(on_dv.solve(on_dv.d(lb), on_dv.d(ub), stride=2))
    on_dv.close()
    print(f"hand-over {'state+control' if xb else 'control'}: iterations off {off['iters']}, on {on['iters']}, "
          f"V* {_rel(on['V'], off['V']).max():.2e} apart")
    assert (off["status"] == 0).all() and (on["status"] == 0).all(), (off["status"], on["status"])
    # the wave rule (at most 4 lanes of the wave still iterating) hands over those that outlast the first to converge:
    # four under control bounds, three under state bounds, where two instances share the lowest count (on the oracle
    # 5 3 6 4 4 and 20 12 12 19 18 iterations)
    assert 3 <= (off["iters"] > off["iters"].min()).sum() <= 4 and off["iters"].min() >= 2, off["iters"]
    assert _rel(on["V"], off["V"]).max() <= 1e-10
    U = controls(on["V"], 17, 4, 2)
    assert (U >= lb[:, None, :]).all() and (U <= ub[:, None, :]).all()


# ---- 3. against the oracle, one instance at a time ----
ORACLE_SHAPE = {"two_link_arm": (17, 37), "exo_arm": (7, 9)}
ORACLE_CASES = [(model, *ORACLE_SHAPE[model], kernel, hess, xb, 0) for model in ORACLE_SHAPE
                for kernel in ("lane", "group") for hess in ("gn", "exact") for xb in (False, True)]
_oracle_cache = {}


def oracle_per_instance(ctx, model, N, B, hess, xb, release):
    """B oracle solves of one instance each, with that instance's bounds, the Hessian and the hold-release rule given
    explicitly (solve_batch(solver=...) would resolve them for the B it is handed)"""
    key = (model, N, B, hess, xb, release)
    if key not in _oracle_cache:
        clip = XB[model][XPAT[model]][4] if xb else None
        x0, up, tr = ctx.inputs(model, 0 if xb else UB_FIRST[model], N, B, clip)
        lb, ub = rows(model, xb, B)
        xl, xu = (arr(v) for v in XB[model][XPAT[model]][:2]) if xb else (None, None)
        hs = oracle.HESS_EXACT if hess == "exact" else oracle.HESS_GAUSS_NEWTON
        res = [oracle.solve_batch(N, H, x0[b:b + 1], up[b:b + 1], tr[b:b + 1], WEIGHTS[model], u_lb=lb[b], u_ub=ub[b],
                                  x_lb=xl, x_ub=xu, max_iter=100, model=OMODEL[model], hessian=hs,
                                  bound_release=release) for b in range(B)]
        _oracle_cache[key] = {k: np.concatenate([r[k] for r in res]) for k in ("V", "status", "iters", "kkt")}
    return _oracle_cache[key]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=_id)
def test_per_instance_batch_matches_the_oracle_per_instance(case, ctx):
    model, N, B, kernel, hess, xb, rule = case
    nx, nu = DIMS[model]
    lb, ub = rows(model, xb, B)
    dv = Dev(ctx, case)
    g = dv.result(dv.solve(dv.d(lb), dv.d(ub), stride=nu))
    dv.close()
    # the 16-lane kernel also releases holds whose multiplier points into the box (oracle_lib.solve_batch)
    o = oracle_per_instance(ctx, model, N, B, hess, xb, release=(kernel == "group" and not xb))
    (compare_xb if xb else compare_ub)(_id(case), g, o)
    U = controls(g["V"], N, nx, nu)
    lo = np.where(np.abs(lb) >= 1e19, -INF, lb)[:, None, :]
    hi = np.where(np.abs(ub) >= 1e19, INF, ub)[:, None, :]
    assert (U >= lo).all() and (U <= hi).all()
    nact = int(((U == lo) | (U == hi)).sum())
    print(f"{_id(case)}: oracle iterations {o['iters'].min()}-{o['iters'].max()}, {nact} controls on a bound")
    if not xb:
        assert nact >= 1


# ---- 4. other layers ----
LAYER = ("two_link_arm", 17, 37, "group", "gn", False, 0)


def test_host_entry_with_2d_bounds_equals_the_device_solve(ctx):
    model, N, B = LAYER[:3]
    lb, ub = rows(model, False, B)
    dv = Dev(ctx, LAYER)
    dev = dv.result(dv.solve(dv.d(lb), dv.d(ub), stride=2))
    host = dv.s.solve_batch_host(*dv.inputs, WEIGHTS[model], u_lb=lb, u_ub=ub)
    assert_same_bits(host, dev, msg="host entry")
    # one-sided: a 2-D lower bound alone
    assert_same_bits(dv.s.solve_batch_host(*dv.inputs, WEIGHTS[model], u_lb=lb), dv.result(dv.solve(dv.d(lb), None, 2)),
                     msg="host entry, lower bounds only")
    # every row infinite: the host entry scans all B rows and runs the unbounded kernels
    inf_rows = np.full((B, 2), BIG)
    assert_same_bits(dv.s.solve_batch_host(*dv.inputs, WEIGHTS[model], u_lb=-inf_rows, u_ub=inf_rows),
                     dv.s.solve_batch_host(*dv.inputs, WEIGHTS[model]), msg="all rows infinite")
    dv.close()


def test_multi_host_entry_offsets_the_shards(ctx, mmpc_mod):
    """device 0 listed twice: the second shard's rows start at first * bounds_stride"""
    import os
    model, N, B = LAYER[:3]
    lb, ub = rows(model, False, B)
    dv = Dev(ctx, LAYER)
    single = dv.s.solve_batch_host(*dv.inputs, WEIGHTS[model], u_lb=lb, u_ub=ub)
    dv.close()
    path = os.path.join(ctx.dir, f"{model}_{N}.json")
    m = mmpc_mod.MultiSolver(path, [0, 0], kkt_solver=mmpc_mod.KKT_RICCATI_GROUP,
                             hessian=mmpc_mod.HESSIAN_GAUSS_NEWTON, max_iter=100)
    multi = m.solve_batch_host(*dv.inputs, WEIGHTS[model], u_lb=lb, u_ub=ub)
    m.close()
    assert_same_bits(multi, single, msg="two shards on one device")
    assert (multi["status"] == 0).all()


def test_rccl_entry_sends_strided_bounds_not_over_read(ctx, mmpc_mod):
    """one rank: the shard's bound rows go through ncclSend / ncclRecv at bounds_stride 3 > nu = 2 from buffers of
    exactly (B - 1) 3 + 2 doubles (NaN padding); bit for bit the single-handle device solve"""
    import os
    if not mmpc_mod.rccl_version():
        pytest.skip("librccl is not loadable")
    import torch
    model, N, B = LAYER[:3]
    lb, ub = rows(model, False, B)
    dv = Dev(ctx, LAYER)
    single = dv.result(dv.solve(dv.d(lb), dv.d(ub), stride=2))
    st = 3
    bufs = []
    for a in (lb, ub):
        full = np.full((B, st), np.nan)
        full[:, :2] = a
        bufs.append(dv.d(full.reshape(-1)[:(B - 1) * st + 2]))
    path = os.path.join(ctx.dir, f"{model}_{N}.json")
    m = mmpc_mod.MultiSolver(path, [0], kkt_solver=mmpc_mod.KKT_RICCATI_GROUP, hessian=mmpc_mod.HESSIAN_GAUSS_NEWTON,
                             max_iter=100)
    V = torch.zeros((B, dv.s.NV), dtype=torch.float64, device="cuda")
    sts = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    it, kk = torch.zeros_like(sts), torch.zeros(B, dtype=torch.float64, device="cuda")
    m.solve_batch_rccl(dv.x0, dv.up, dv.tr, dv.w, V, sts, it, kk, u_lb=bufs[0], u_ub=bufs[1], bounds_stride=st)
    torch.cuda.synchronize()
    with pytest.raises(mmpc_mod.MmpcError, match="bounds_stride"):
        m.solve_batch_rccl(dv.x0, dv.up, dv.tr, dv.w, V.clone(), u_lb=bufs[0], u_ub=bufs[1], bounds_stride=1)
    m.close()
    dv.close()
    assert_same_bits(dv.result((V, sts, it, kk)), single, msg="RCCL entry")


def test_per_instance_solve_replays_from_a_graph(ctx):
    import torch
    model, N, B = LAYER[:3]
    lb, ub = rows(model, False, B)
    dv = Dev(ctx, LAYER)
    dv.s.reserve_workspace(B)
    dlb, dub = dv.d(lb), dv.d(ub)
    ref = dv.result(dv.solve(dlb, dub, stride=2))
    out = dv.solve(dlb, dub, stride=2)
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs):   # one solve on the capture stream before capturing
        dv.solve(dlb, dub, stride=2, stream=cs.cuda_stream, out=out)
    torch.cuda.current_stream().wait_stream(cs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        dv.solve(dlb, dub, stride=2, stream=cs.cuda_stream, out=out)
    for _ in range(2):
        for t in out:
            t.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        assert_same_bits(dv.result(out), ref, msg="graph replay")
    # the graph reads the live bound rows: swap two instances' rows in place and replay
    dlb[[0, 1]] = dlb[[1, 0]]
    dub[[0, 1]] = dub[[1, 0]]
    torch.cuda.synchronize()
    ref2 = dv.result(dv.solve(dlb, dub, stride=2))
    assert not np.array_equal(ref2["V"][:2], ref["V"][:2])
    for t in out:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert_same_bits(dv.result(out), ref2, msg="graph replay after new bounds")
    dv.close()
