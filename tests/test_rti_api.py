"""CPU: the real-time iteration entry points of include/mmpc.h (mmpc_rti_prepare_batch, mmpc_rti_feedback_batch,
mmpc_rti_step_batch_host, mmpc_rti_workspace_bytes; additive to ABI 6).

The handles ask for a device index no machine has (as tests/test_solve_jvp_api.py does), so every answer below comes
from the arguments alone, before any device call, and the test is the same with and without a GPU:

* the header declares the four functions, the library exports them and the Python layer has their prototypes, the
  Solver methods and the RTI_FAILED constant; the ABI version stays 6 and sizeof(mmpc_opts) stays 56;
* prepare and host entry: n_pin in {-1, N}, a bounds_stride in 1 .. nu - 1, a weights_stride in 1 .. nx + 2 nu - 1, an
  unknown hessian and a NULL input are MMPC_ERR_INVALID_ARG with the argument's name in mmpc_last_error;
* feedback: a bad bounds_stride, a NULL x0_meas and a NULL V_inout are MMPC_ERR_INVALID_ARG naming them; every output
  may be NULL;
* a workspace that is NULL or one byte short is MMPC_ERR_INVALID_ARG naming `workspace` on the two device entries (the
  host entry brings its own);
* a linear-mode model, and a state-bounded handle with the sensitivity barrier off AND on, are MMPC_ERR_UNSUPPORTED on
  all three entries;
* the workspace query: ceil(B / 64) 64 ((N K (K + 1) + NV) 8 + 4) bytes, K = nx + nu;
* B = 0 returns MMPC_OK."""
import ctypes as C

import numpy as np
import pytest

NEW = ["mmpc_rti_workspace_bytes", "mmpc_rti_prepare_batch", "mmpc_rti_feedback_batch", "mmpc_rti_step_batch_host"]
MODELS = [("two_link_arm", 4, 2), ("exo_arm", 8, 4)]
NO_SUCH_DEVICE = 4096   # mmpc_create touches no device
a = lambda v: None if v is None else v.ctypes.data   # noqa: E731


def test_header_declares_and_library_exports(mmpc_mod):
    names = mmpc_mod.header_functions()
    L = mmpc_mod.lib()
    for fn in NEW:
        assert fn in names, fn
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes is not None, fn
    assert len(L.mmpc_rti_prepare_batch.argtypes) == 16 and len(L.mmpc_rti_feedback_batch.argtypes) == 13
    assert len(L.mmpc_rti_step_batch_host.argtypes) == 16
    for meth in ("rti_workspace_bytes", "rti_prepare", "rti_feedback", "rti_step_host"):
        assert hasattr(mmpc_mod.Solver, meth), meth
    assert mmpc_mod.RTI_FAILED == 2


def test_abi_version_and_opts_size_unchanged(mmpc_mod):
    assert mmpc_mod.lib().mmpc_abi_version() == 6
    assert C.sizeof(mmpc_mod.Opts) == 56


def _solver(mmpc_mod, tmp_path, model, nx, nu, N, **kw):
    p = mmpc_mod.write_model_json(str(tmp_path / f"{model}_{N}.json"), model, nx, nu, 2000, N, model=model, **kw)
    return mmpc_mod.Solver(p, device=NO_SUCH_DEVICE)


class Args:
    """one tick's arguments: host arrays of the right sizes, every output given, a workspace of the queried size"""

    def __init__(self, s, B):
        nx, nu, N, NV = s.nx, s.nu, s.N, s.NV
        n = max(B, 1)
        self.B = B
        self.V, self.up, self.tr = np.zeros((n, NV)), np.zeros((n, nu)), np.zeros((n, N, nx))
        self.x0 = np.zeros((n, nx))
        self.w, self.w_stride = np.ones(n * (nx + 2 * nu + 3)), 0
        self.lb, self.ub, self.stride = -np.ones(nu), np.ones(nu), 0
        self.n_pin, self.hessian = 0, 0
        self.u0, self.si, self.st, self.pst = np.zeros((n, nu)), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.ws_bytes = s.rti_workspace_bytes(n)
        self.ws = np.zeros(self.ws_bytes // 8)

    def call(self, s, which, **change):
        """(rc, mmpc_last_error) of one entry (`prepare`, `feedback` or `host`), with some attributes replaced"""
        v = dict(vars(self), **change)
        L = s._L
        if which == "prepare":
            rc = L.mmpc_rti_prepare_batch(s._h, v["B"], a(v["V"]), a(v["up"]), a(v["tr"]), a(v["w"]), v["w_stride"],
                                          a(v["lb"]), a(v["ub"]), v["stride"], v["n_pin"], v["hessian"], a(v["pst"]),
                                          a(v["ws"]), v["ws_bytes"], None)
        elif which == "feedback":
            rc = L.mmpc_rti_feedback_batch(s._h, v["B"], a(v["x0"]), a(v["lb"]), a(v["ub"]), v["stride"], a(v["V"]),
                                           a(v["u0"]), a(v["si"]), a(v["st"]), a(v["ws"]), v["ws_bytes"], None)
        else:
            rc = L.mmpc_rti_step_batch_host(s._h, v["B"], a(v["V"]), a(v["x0"]), a(v["up"]), a(v["tr"]), a(v["w"]),
                                            v["w_stride"], a(v["lb"]), a(v["ub"]), v["stride"], v["n_pin"],
                                            v["hessian"], a(v["u0"]), a(v["si"]), a(v["st"]))
        return rc, L.mmpc_last_error().decode()


ALL = ("prepare", "feedback", "host")


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_bad_arguments_are_refused_before_any_device_call(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, B)
    bad = [("n_pin", dict(n_pin=-1)), ("n_pin", dict(n_pin=N)), ("bounds_stride", dict(stride=nu - 1)),
           ("bounds_stride", dict(stride=-1)), ("weights_stride", dict(w_stride=nx + 2 * nu - 1)),
           ("weights_stride", dict(w_stride=-1)), ("hessian", dict(hessian=3)), ("hessian", dict(hessian=-1)),
           ("null input pointer", dict(V=None)), ("null input pointer", dict(up=None)),
           ("null input pointer", dict(tr=None)), ("null input pointer", dict(w=None))]
    for name, change in bad:
        for which in ("prepare", "host"):
            rc, msg = g.call(s, which, **change)
            assert rc == -1 and name in msg, (which, name, change, rc, msg)
    for name, change in [("bounds_stride", dict(stride=nu - 1)), ("bounds_stride", dict(stride=-1)),
                         ("x0_meas", dict(x0=None)), ("V_inout", dict(V=None))]:
        rc, msg = g.call(s, "feedback", **change)
        assert rc == -1 and name in msg, (name, change, rc, msg)
    rc, msg = g.call(s, "host", x0=None)
    assert rc == -1 and "x0_meas" in msg, (rc, msg)
    for which in ALL:   # the arguments pass: the call goes on to look for its device
        rc, msg = g.call(s, which)
        assert rc in (-5, -6), (which, rc, msg)
        rc, msg = g.call(s, which, lb=None, ub=None, u0=None, si=None, st=None, pst=None)
        assert rc in (-5, -6), (which, rc, msg)
    with pytest.raises(mmpc_mod.MmpcError, match="n_pin") as e:
        s.rti_step_host(g.V, g.x0, g.up, g.tr, np.ones(nx + 2 * nu), n_pin=N)
    assert e.value.code == -1
    with pytest.raises(mmpc_mod.MmpcError, match="hessian") as e:
        s.rti_prepare(B, a(g.V), a(g.up), a(g.tr), a(g.w), workspace=a(g.ws), workspace_bytes=g.ws_bytes,
                      prep_status=a(g.pst), hessian=7)
    assert e.value.code == -1
    with pytest.raises(mmpc_mod.MmpcError, match="workspace") as e:
        s.rti_feedback(B, a(g.x0), a(g.V), a(g.ws), workspace_bytes=8, u0=a(g.u0), step_inf=a(g.si), status=a(g.st))
    assert e.value.code == -1
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_the_device_entries_need_the_workspace(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, B)
    for change in (dict(ws=None), dict(ws=None, ws_bytes=0), dict(ws_bytes=g.ws_bytes - 1), dict(ws_bytes=0)):
        for which in ("prepare", "feedback"):
            rc, msg = g.call(s, which, **change)
            assert rc == -1 and "workspace" in msg, (which, change, rc, msg)
            if "ws" not in change:
                assert "workspace_bytes" in msg and str(g.ws_bytes) in msg, msg
        rc, msg = g.call(s, "host", **change)
        assert rc in (-5, -6), (rc, msg)   # the host entry allocates its own
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_workspace_query(model, nx, nu, mmpc_mod, tmp_path):
    N = 5
    K, NV = nx + nu, nx * (N + 1) + nu * N
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    last = 0
    for B in (1, 2, 63, 64, 65, 128, 129, 4096, 65536):
        n = s.rti_workspace_bytes(B)
        assert n > 0 and n >= last and n % 8 == 0, (B, n, last)
        assert n == -(-B // 64) * 64 * ((N * K * (K + 1) + NV) * 8 + 4), (B, n)
        last = n
    assert s.rti_workspace_bytes(0) == 0
    n = C.c_uint64(7)
    assert s._L.mmpc_rti_workspace_bytes(s._h, -1, C.byref(n)) == -1
    assert s._L.mmpc_rti_workspace_bytes(s._h, 1, None) == -1
    assert s._L.mmpc_rti_workspace_bytes(None, 1, C.byref(n)) == -1
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_zero_instances_is_a_no_op(model, nx, nu, mmpc_mod, tmp_path):
    N = 3
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, 0)
    for which in ALL:
        assert g.call(s, which)[0] == 0, which
        assert g.call(s, which, ws=None, ws_bytes=0)[0] == 0, which
    L = s._L
    assert L.mmpc_rti_prepare_batch(s._h, 0, None, None, None, None, 0, None, None, 0, 0, 0, None, None, 0, None) == 0
    assert L.mmpc_rti_feedback_batch(s._h, 0, None, None, None, 0, None, None, None, None, None, 0, None) == 0
    assert L.mmpc_rti_step_batch_host(s._h, 0, None, None, None, None, None, 0, None, None, 0, 0, 0, None, None,
                                      None) == 0
    s.close()


def test_linear_mode_is_unsupported(mmpc_mod, model_json):
    N, B = 3, 2
    s = mmpc_mod.Solver(model_json(N=N, is_linear=True, name="linear_double_pendulum"), device=NO_SUCH_DEVICE)
    g = Args(s, B)
    for which in ALL:
        rc, msg = g.call(s, which, lb=None, ub=None)
        assert rc == -4 and "linear" in msg, (which, rc, msg)
    s.close()


def test_state_bounds_are_refused_with_the_barrier_on_or_off(mmpc_mod, tmp_path):
    N, B, nx, nu = 3, 2, 4, 2
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N)
    g = Args(s, B)
    s.set_state_bounds(None, np.array([np.inf, np.inf, 1.5, np.inf]))
    for barrier in ("off", "on", "off again"):
        if barrier == "on":
            s.set_sensitivity_barrier()
        elif barrier == "off again":
            s.set_sensitivity_barrier(mu=0.0)
        for which in ALL:
            rc, msg = g.call(s, which)
            assert rc == -4 and "state bounds" in msg and "real-time iteration" in msg, (barrier, which, rc, msg)
    s.set_state_bounds(None, None)   # infinite again
    for which in ALL:
        rc, msg = g.call(s, which)
        assert rc in (-5, -6), (which, rc, msg)
    s.close()
