"""GPU: the shift between two ticks of a real-time iteration loop, mmpc_rti_shift_batch (include/mmpc.h).

Plans are the GPU solves of oracle.synth(20250213, ...) that tests/test_gpu_feedback_gains.py and tests/test_gpu_rti.py
share.  The reference of every comparison is rti_reference.shift_plan applied n_shift times.

1. shapes (N, B, n_shift): 2-link (1, 5, 0) (1, 5, 1) (2, 3, 2) (3, 9, 1) (17, 37, 1) (17, 37, 3) (17, 37, 17)
   (33, 65, 1); exo (7, 9, 1) (7, 9, 7) (21, 9, 1); cart_pole's generated library (17, 5, 1).  n = 0 is the copy, n = N
   keeps the old x_N alone; 37 and 65 instances put several instances and a row boundary into one wave of the copy.
   Copied entries and u_prev_out bit for bit; with n = 0 u_prev_out is not written.  Rolled-out states within
   1e-12 max(1, max |ref|): the GPU and the oracle agree to 2.2e-15 on whole solves, and at most 33 compounded Euler
   steps of an O(1) state stay far inside that.
2. NaN: a NaN in one instance's plan (its x_N, so that the roll-out sees it) changes no bit of the other instances', the
   wave-mates of the copy and of the roll-out included; the instance's own copied entries are still the old ones.
3. B = 1 agrees bit for bit with the instance inside a batch; the result is the same from run to run.
4. a captured graph of one tick (feedback, shift, prepare) replays to the bits of the direct calls; it is captured from
   one stream, so its three launches form one chain: a graph with a single branch."""
import numpy as np
import pytest

from rti_reference import shift_plan
from test_gpu_feedback_gains import DIMS, H, OMODEL, W_2L, Ctx, dev

pytestmark = pytest.mark.gpu

TOL = 1e-12
SHAPES = [("two_link_arm", 1, 5, 0), ("two_link_arm", 1, 5, 1), ("two_link_arm", 2, 3, 2), ("two_link_arm", 3, 9, 1),
          ("two_link_arm", 17, 37, 1), ("two_link_arm", 17, 37, 3), ("two_link_arm", 17, 37, 17),
          ("two_link_arm", 33, 65, 1), ("exo_arm", 7, 9, 1), ("exo_arm", 7, 9, 7), ("exo_arm", 21, 9, 1)]


def _id(case):
    return "-".join(str(v) for v in case)


@pytest.fixture(scope="module")
def ctx(mmpc_mod, tmp_path_factory):
    return Ctx(mmpc_mod, str(tmp_path_factory.mktemp("rti_shift")))


def reference(om, N, h, V, n):
    """shift_plan applied n times to every row: (V_ref [B, NV], u_prev_ref [B, nu] or None for n = 0)"""
    out, ups = [], []
    for b in range(V.shape[0]):
        v, up = V[b], None
        for _ in range(n):
            v, up = shift_plan(om, N, h, v)
        out.append(v)
        ups.append(up)
    return np.stack(out), (np.stack(ups) if n else None)


def rolled_mask(nx, nu, N, n):
    """True on the entries of a row the roll-out computes: x_k for k > N - n"""
    K = nx + nu
    m = np.zeros(nx * (N + 1) + nu * N, bool)
    for k in range(N - n + 1, N + 1):
        m[k * K:k * K + nx] = True
    return m


def gpu_shift(s, V, n):
    """one shift on fresh tensors: (V_out, u_prev_out) as numpy; both outputs start as a sentinel"""
    import torch
    B = V.shape[0]
    Vo = torch.full((B, s.NV), -7.0, dtype=torch.float64, device="cuda")
    up = torch.full((B, s.nu), -7.0, dtype=torch.float64, device="cuda")
    Vi = dev(V)
    r = s.rti_shift(B, Vi, n, V_out=Vo, u_prev_out=up)
    torch.cuda.synchronize()
    assert np.array_equal(Vi.cpu().numpy(), V, equal_nan=True), "V_in is read only"
    return r["V"].cpu().numpy(), r["u_prev"].cpu().numpy()


def check_shift(got, up, V, ref, up_ref, nx, nu, N, n, what):
    roll = rolled_mask(nx, nu, N, n)
    assert np.array_equal(got[:, ~roll], ref[:, ~roll]), f"{what}: copied entries bit for bit"
    if n == 0:
        assert np.array_equal(got, V) and (up == -7.0).all(), f"{what}: n = 0 is a copy and writes no u_prev"
        return
    assert np.array_equal(up, up_ref), f"{what}: u_prev_out bit for bit"
    err = np.abs(got[:, roll] - ref[:, roll]).max(axis=1)
    bound = TOL * np.maximum(1.0, np.abs(ref).max(axis=1))
    print(f"{what}: rolled-out states, max err {err.max():.3e}, worst err / bound {(err / bound).max():.3e}")
    assert np.isfinite(got).all() and (err <= bound).all(), (what, err.max())


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("case", SHAPES, ids=_id)
def test_shift_matches_the_reference(case, ctx):
    model, N, B, n = case
    nx, nu = DIMS[model]
    V = ctx.plan(model, N, B)
    ref, up_ref = reference(OMODEL[model], N, H, V, n)
    s = ctx.solver(model, N)
    got, up = gpu_shift(s, V, n)
    s.close()
    check_shift(got, up, V, ref, up_ref, nx, nu, N, n, _id(case))


def test_generated_model_shift(mmpc_mod, tmp_path_factory):
    from test_gpu_sx_sensitivity import Ctx as SxCtx
    from test_user_model_sens_reference import H as H_SX
    from test_user_model_sens_reference import use
    case = ("free", "cart_pole", 17, 5)
    _, model, N, B = case
    nx, nu = 4, 1
    import os

    from test_gpu_sx_models import USER
    # the build generates the model libraries: without this one the compile_model instantiation is not covered
    assert os.path.exists(os.path.join(USER, f"{model}.so")), "cart_pole's generated library is not built"
    x = SxCtx(mmpc_mod, str(tmp_path_factory.mktemp("rti_shift_sx")))
    s = x.solver(case)
    V = x.plan(case)
    got, up = gpu_shift(s, V, 1)
    s.close()
    ref, up_ref = reference(use(model), N, H_SX, V, 1)
    check_shift(got, up, V, ref, up_ref, nx, nu, N, 1, "cart_pole-17-5-1")


# ---------------------------------------------------------------- 2. NaN
@pytest.mark.parametrize("n", [1, 3])
def test_nan_stays_in_its_row(n, ctx):
    model, N, B, bad = "two_link_arm", 17, 130, 5   # 130: instances in the roll-out's first, second and third wave
    nx, nu = DIMS[model]
    K = nx + nu
    V = np.tile(ctx.plan(model, N, 37), (4, 1))[:B]
    s = ctx.solver(model, N)
    clean, up_clean = gpu_shift(s, V, n)
    V2 = V.copy()
    V2[bad, N * K + 1] = np.nan   # in x_N: copied to x_{N-n} and the start of the roll-out
    got, up = gpu_shift(s, V2, n)
    s.close()
    others = np.arange(B) != bad
    assert np.array_equal(got[others], clean[others]) and np.array_equal(up[others], up_clean[others])
    roll = rolled_mask(nx, nu, N, n)
    ref, _ = reference(OMODEL[model], N, H, V2[bad:bad + 1], n)
    assert np.array_equal(got[bad, ~roll], ref[0, ~roll], equal_nan=True), "the row's own copied entries"
    assert np.isnan(got[bad, (N - n) * K + 1]) and np.isnan(got[bad, roll]).any()
    assert np.array_equal(up[bad], up_clean[bad])


# ---------------------------------------------------------------- 3. repeatability
def test_single_instance_and_run_to_run(ctx):
    model, N, B = "two_link_arm", 17, 37
    V = ctx.plan(model, N, B)
    s = ctx.solver(model, N)
    for n in (1, 3, 17):
        a, ua = gpu_shift(s, V, n)
        b, ub = gpu_shift(s, V, n)
        assert np.array_equal(a, b) and np.array_equal(ua, ub), f"n = {n}: run to run"
        for i in (0, 36):
            one, uo = gpu_shift(s, V[i:i + 1], n)
            assert np.array_equal(one[0], a[i]) and np.array_equal(uo[0], ua[i]), f"n = {n}: B = 1 against row {i}"
    s.close()


# ---------------------------------------------------------------- 4. a captured tick
def test_captured_tick_replays_the_direct_calls(ctx):
    import torch
    model, N, B = "two_link_arm", 17, 5
    nx, nu = DIMS[model]
    _, up0, tr = ctx.inputs(model, N, B)
    s = ctx.solver(model, N)
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    Va, Vb, up = dev(ctx.plan(model, N, B)), f64(B, s.NV), dev(up0)
    dtr, dw = dev(tr), dev(W_2L)
    xm = dev(ctx.plan(model, N, B)[:, :nx] + 1e-3 * np.random.default_rng(5).standard_normal((B, nx)))
    out = dict(u0=f64(B, nu), step_inf=f64(B), status=torch.full((B,), -1, dtype=torch.int32, device="cuda"))
    ws = f64(s.rti_workspace_bytes(B) // 8)
    pst = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    s.rti_prepare(B, Va, up, dtr, dw, workspace=ws, prep_status=pst)
    torch.cuda.synchronize()
    start = (Va.clone(), Vb.clone(), up.clone(), ws.clone())

    def one_tick(stream=None):
        s.rti_feedback(B, xm, Va, ws, stream=stream, **out)
        s.rti_shift(B, Va, 1, V_out=Vb, u_prev_out=up, stream=stream)
        s.rti_prepare(B, Vb, up, dtr, dw, workspace=ws, prep_status=pst, stream=stream)

    one_tick()
    torch.cuda.synchronize()
    live = (Va, Vb, up, ws, out["u0"], out["step_inf"], out["status"], pst)
    want = [t.clone() for t in live]
    assert (want[6].cpu().numpy() == 0).all() and (want[7].cpu().numpy() == 0).all()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        one_tick(cs.cuda_stream)
    for t, v in zip((Va, Vb, up, ws), start):   # the graph reads the live buffers
        t.copy_(v)
    for t in (out["u0"], out["step_inf"]):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for name, t, w in zip(("V", "V_shifted", "u_prev", "workspace", "u0", "step_inf", "status", "prep_status"), live,
                          want):
        assert torch.equal(t, w), f"{name}: the replayed tick against the direct calls"
    s.close()
