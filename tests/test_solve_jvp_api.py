"""CPU: the solve-JVP entry points of include/mmpc.h (mmpc_solve_jvp_batch[_host], mmpc_solve_jvp_workspace_bytes;
additive to ABI 6).

The handles ask for a device index no machine has (as tests/test_solve_vjp_api.py does), so every answer below comes
from the arguments alone, before any device call, and the test is the same with and without a GPU:

* the header declares the three functions, the library exports them and the Python layer has their prototypes, the
  Solver methods and the JVP_FAILED constant; the ABI version stays 6 and sizeof(mmpc_opts) stays 56;
* n_pin in {-1, N}, a bounds_stride in 1 .. nu - 1, a weights_stride in 1 .. nx + 2 nu - 1 and an unknown hessian are
  MMPC_ERR_INVALID_ARG with the argument's name in mmpc_last_error, on the device and on the host entry;
* all four tangents NULL, and dV and du0 both NULL, are MMPC_ERR_INVALID_ARG naming them; each tangent alone passes;
* a workspace that is NULL or one byte short with dV asked for is MMPC_ERR_INVALID_ARG naming `workspace` on the
  device entry (the host entry brings its own); with dV NULL (forward-free) a NULL workspace passes the arguments;
* a linear-mode model and a state-bounded handle whose sensitivity barrier is off are MMPC_ERR_UNSUPPORTED; with the
  barrier on the arguments pass;
* the workspace query is the VJP's: ceil(B / 64) 64 N nu (nx + nu + 1) doubles;
* B = 0 returns MMPC_OK."""
import ctypes as C

import numpy as np
import pytest

NEW = ["mmpc_solve_jvp_batch", "mmpc_solve_jvp_batch_host", "mmpc_solve_jvp_workspace_bytes"]
MODELS = [("two_link_arm", 4, 2), ("exo_arm", 8, 4)]
NO_SUCH_DEVICE = 4096   # mmpc_create touches no device
TANGENTS = ("dx0", "dup", "dtr", "dw")
a = lambda v: None if v is None else v.ctypes.data   # noqa: E731


def test_header_declares_and_library_exports(mmpc_mod):
    names = mmpc_mod.header_functions()
    L = mmpc_mod.lib()
    for fn in NEW:
        assert fn in names, fn
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes is not None, fn
    assert len(L.mmpc_solve_jvp_batch.argtypes) == 22 and len(L.mmpc_solve_jvp_batch_host.argtypes) == 19
    for meth in ("solve_jvp", "solve_jvp_host", "solve_jvp_workspace_bytes"):
        assert hasattr(mmpc_mod.Solver, meth), meth
    assert mmpc_mod.JVP_FAILED == 2


def test_abi_version_and_opts_size_unchanged(mmpc_mod):
    assert mmpc_mod.lib().mmpc_abi_version() == 6
    assert C.sizeof(mmpc_mod.Opts) == 56


def _solver(mmpc_mod, tmp_path, model, nx, nu, N, **kw):
    p = mmpc_mod.write_model_json(str(tmp_path / f"{model}_{N}.json"), model, nx, nu, 2000, N, model=model, **kw)
    return mmpc_mod.Solver(p, device=NO_SUCH_DEVICE)


class Args:
    """one call's arguments: host arrays of the right sizes, every tangent and output given, a workspace of the
    queried size"""

    def __init__(self, s, B):
        nx, nu, N, NV = s.nx, s.nu, s.N, s.NV
        n = max(B, 1)
        self.B = B
        self.V, self.up, self.tr = np.zeros((n, NV)), np.zeros((n, nu)), np.zeros((n, N, nx))
        self.w, self.w_stride = np.ones(n * (nx + 2 * nu + 3)), 0
        self.lb, self.ub, self.stride = -np.ones(nu), np.ones(nu), 0
        self.n_pin, self.hessian = 0, 0
        self.dx0, self.dup, self.dtr = np.zeros((n, nx)), np.zeros((n, nu)), np.zeros((n, N, nx))
        self.dw = np.zeros((n, nx + 2 * nu))
        self.dV, self.du0, self.st = np.zeros((n, NV)), np.zeros((n, nu)), np.zeros(n, np.int32)
        self.ws_bytes = s.solve_jvp_workspace_bytes(n)
        self.ws = np.zeros(self.ws_bytes // 8)

    def call_both(self, s, **change):
        """(rc, mmpc_last_error) of the device entry and of the host entry, with some attributes replaced"""
        v = dict(vars(self), **change)
        pre = (s._h, v["B"], a(v["V"]), a(v["up"]), a(v["tr"]), a(v["w"]), v["w_stride"], a(v["lb"]), a(v["ub"]),
               v["stride"], v["n_pin"], a(v["dx0"]), a(v["dup"]), a(v["dtr"]), a(v["dw"]), v["hessian"], a(v["dV"]),
               a(v["du0"]), a(v["st"]))
        L = s._L
        out = []
        for fn, args in ((L.mmpc_solve_jvp_batch, pre + (a(v["ws"]), v["ws_bytes"], None)),
                         (L.mmpc_solve_jvp_batch_host, pre)):
            rc = fn(*args)
            out.append((rc, L.mmpc_last_error().decode()))
        return out


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_bad_arguments_are_refused_before_any_device_call(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, B)
    bad = [("n_pin", dict(n_pin=-1)), ("n_pin", dict(n_pin=N)), ("bounds_stride", dict(stride=nu - 1)),
           ("bounds_stride", dict(stride=-1)), ("weights_stride", dict(w_stride=nx + 2 * nu - 1)),
           ("weights_stride", dict(w_stride=-1)), ("hessian", dict(hessian=3)), ("hessian", dict(hessian=-1)),
           ("null input pointer", dict(V=None))]
    for name, change in bad:
        for rc, msg in g.call_both(s, **change):
            assert rc == -1, (name, change, rc, msg)
            assert name in msg, (name, change, msg)
    for rc, msg in g.call_both(s):   # the arguments pass: the call goes on to look for its device
        assert rc in (-5, -6), (rc, msg)
    with pytest.raises(mmpc_mod.MmpcError, match="n_pin") as e:
        s.solve_jvp_host(g.V, g.up, g.tr, np.ones(nx + 2 * nu), dx0=g.dx0, n_pin=N)
    assert e.value.code == -1
    with pytest.raises(mmpc_mod.MmpcError, match="hessian") as e:
        s.solve_jvp(B, a(g.V), a(g.up), a(g.tr), a(g.w), dx0=a(g.dx0), du0=a(g.du0), jvp_status=a(g.st),
                    forward_free=True, hessian=7)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        s.solve_jvp(B, a(g.V), a(g.up), a(g.tr), a(g.w), dx0=a(g.dx0), dV=a(g.dV), forward_free=True)
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_the_two_all_null_rules(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, B)
    none = {k: None for k in TANGENTS}
    for rc, msg in g.call_both(s, **none):
        assert rc == -1 and all(n in msg for n in ("dx0", "du_prev", "dtraj", "dweights")), (rc, msg)
    for keep in TANGENTS:   # each tangent alone is a call
        for rc, msg in g.call_both(s, **{k: None for k in TANGENTS if k != keep}):
            assert rc in (-5, -6), (keep, rc, msg)
    for rc, msg in g.call_both(s, dV=None, du0=None):
        assert rc == -1 and "dV" in msg and "du0" in msg, (rc, msg)
    for change in (dict(dV=None), dict(du0=None), dict(st=None)):
        for rc, msg in g.call_both(s, **change):
            assert rc in (-5, -6), (change, rc, msg)
    with pytest.raises(mmpc_mod.MmpcError, match="dweights") as e:
        s.solve_jvp_host(g.V, g.up, g.tr, np.ones(nx + 2 * nu))
    assert e.value.code == -1
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_the_plan_update_needs_the_workspace(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, B)
    for change in (dict(ws=None), dict(ws=None, ws_bytes=0), dict(ws_bytes=g.ws_bytes - 1), dict(ws_bytes=0)):
        for more in ({}, dict(du0=None)):
            (rc, msg), (rch, msgh) = g.call_both(s, **change, **more)
            assert rc == -1 and "workspace" in msg, (change, rc, msg)
            assert rch in (-5, -6), (rch, msgh)   # the host entry allocates its own
    for change in (dict(ws=None, ws_bytes=0), dict(ws_bytes=0), {}):   # forward-free: no workspace needed
        for rc, msg in g.call_both(s, dV=None, **change):
            assert rc in (-5, -6), (change, rc, msg)
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_workspace_query(model, nx, nu, mmpc_mod, tmp_path):
    N = 5
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    last = 0
    for B in (1, 2, 63, 64, 65, 128, 129, 4096, 65536):
        n = s.solve_jvp_workspace_bytes(B)
        assert n > 0 and n >= last, (B, n, last)
        assert n == -(-B // 64) * 64 * N * nu * (nx + nu + 1) * 8, (B, n)
        assert n == s.solve_vjp_workspace_bytes(B), (B, n)
        last = n
    assert s.solve_jvp_workspace_bytes(0) == 0
    n = C.c_uint64(7)
    assert s._L.mmpc_solve_jvp_workspace_bytes(s._h, -1, C.byref(n)) == -1
    assert s._L.mmpc_solve_jvp_workspace_bytes(s._h, 1, None) == -1
    assert s._L.mmpc_solve_jvp_workspace_bytes(None, 1, C.byref(n)) == -1
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_zero_instances_is_a_no_op(model, nx, nu, mmpc_mod, tmp_path):
    N = 3
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, 0)
    for rc, msg in g.call_both(s):
        assert rc == 0, (rc, msg)
    for rc, msg in g.call_both(s, ws=None, ws_bytes=0):
        assert rc == 0, (rc, msg)
    assert s._L.mmpc_solve_jvp_batch(s._h, 0, None, None, None, None, 0, None, None, 0, 0, None, None, None, None, 0,
                                     None, None, None, None, 0, None) == 0
    assert s._L.mmpc_solve_jvp_batch_host(s._h, 0, None, None, None, None, 0, None, None, 0, 0, None, None, None, None,
                                          0, None, None, None) == 0
    s.close()


def test_linear_mode_is_unsupported(mmpc_mod, model_json):
    N, B = 3, 2
    s = mmpc_mod.Solver(model_json(N=N, is_linear=True, name="linear_double_pendulum"), device=NO_SUCH_DEVICE)
    g = Args(s, B)
    for rc, msg in g.call_both(s, lb=None, ub=None):
        assert rc == -4 and "linear" in msg, (rc, msg)
    s.close()


def test_state_bounds_need_the_sensitivity_barrier(mmpc_mod, tmp_path):
    N, B, nx, nu = 3, 2, 4, 2
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N)
    g = Args(s, B)
    s.set_state_bounds(None, np.array([np.inf, np.inf, 1.5, np.inf]))
    for rc, msg in g.call_both(s):
        assert rc == -4 and "state bounds" in msg and "JVP" in msg, (rc, msg)
    s.set_sensitivity_barrier()   # on: the arguments pass, the call goes on to look for its device
    for rc, msg in g.call_both(s):
        assert rc in (-5, -6), (rc, msg)
    s.set_sensitivity_barrier(mu=0.0)
    for rc, msg in g.call_both(s):
        assert rc == -4 and "state bounds" in msg, (rc, msg)
    s.set_state_bounds(None, None)   # infinite again
    for rc, msg in g.call_both(s):
        assert rc in (-5, -6), (rc, msg)
    s.close()
