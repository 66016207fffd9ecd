"""CPU: the solve-VJP entry points of include/mmpc.h (mmpc_solve_vjp_batch[_host], mmpc_solve_vjp_workspace_bytes;
additive to ABI 6).

The handles ask for a device index no machine has (as tests/test_feedback_gains_api.py does), so every answer below
comes from the arguments alone, before any device call, and the test is the same with and without a GPU:

* the header declares the three functions, the library exports them and the Python layer has their prototypes;
  mmpc/autograd.py exists and `import mmpc` does not import it; the ABI version stays 6 and sizeof(mmpc_opts) stays 56;
* n_pin in {-1, N}, a bounds_stride in 1 .. nu - 1, a weights_stride in 1 .. nx + 2 nu - 1, an unknown hessian and a
  NULL V_bar are MMPC_ERR_INVALID_ARG with the argument's name in mmpc_last_error, on the device and on the host entry;
* a workspace that is NULL or one byte short, with any one of traj_bar / weights_bar / adj_V asked for, is
  MMPC_ERR_INVALID_ARG naming `workspace` on the device entry (the host entry brings its own); with none of the three
  asked for (backward-only) a NULL workspace passes the arguments;
* a linear-mode model and a handle with a finite state bound are MMPC_ERR_UNSUPPORTED;
* the workspace query is positive, non-decreasing in B and ceil(B / 64) 64 N nu (nx + nu + 1) doubles;
* B = 0 returns MMPC_OK."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

NEW = ["mmpc_solve_vjp_batch", "mmpc_solve_vjp_batch_host", "mmpc_solve_vjp_workspace_bytes"]
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
    for meth in ("solve_vjp", "solve_vjp_host", "solve_vjp_workspace_bytes"):
        assert hasattr(mmpc_mod.Solver, meth), meth
    assert os.path.exists(os.path.join(mmpc_mod.PKG_DIR, "autograd.py"))
    with open(os.path.join(mmpc_mod.PKG_DIR, "__init__.py")) as fh:
        assert "autograd" not in fh.read(), "mmpc/__init__.py must not import the torch module"


def test_abi_version_and_opts_size_unchanged(mmpc_mod):
    assert mmpc_mod.lib().mmpc_abi_version() == 6
    assert C.sizeof(mmpc_mod.Opts) == 56


def _solver(mmpc_mod, tmp_path, model, nx, nu, N, **kw):
    p = mmpc_mod.write_model_json(str(tmp_path / f"{model}_{N}.json"), model, nx, nu, 2000, N, model=model, **kw)
    return mmpc_mod.Solver(p, device=NO_SUCH_DEVICE)


class Args:
    """one call's arguments: host arrays of the right sizes, every output asked for, a workspace of the queried size"""

    def __init__(self, s, B):
        nx, nu, N, NV = s.nx, s.nu, s.N, s.NV
        n = max(B, 1)
        self.B = B
        self.V, self.up, self.tr = np.zeros((n, NV)), np.zeros((n, nu)), np.zeros((n, N, nx))
        self.w, self.w_stride = np.ones(n * (nx + 2 * nu + 3)), 0
        self.lb, self.ub, self.stride = -np.ones(nu), np.ones(nu), 0
        self.n_pin, self.hessian = 0, 0
        self.Vbar = np.zeros((n, NV))
        self.x0b, self.upb, self.trb = np.zeros((n, nx)), np.zeros((n, nu)), np.zeros((n, N, nx))
        self.wb, self.adj, self.st = np.zeros((n, nx + 2 * nu)), np.zeros((n, NV)), np.zeros(n, np.int32)
        self.ws_bytes = s.solve_vjp_workspace_bytes(n)
        self.ws = np.zeros(self.ws_bytes // 8)

    def call_both(self, s, **change):
        """(rc, mmpc_last_error) of the device entry and of the host entry, with some attributes replaced"""
        v = dict(vars(self), **change)
        pre = (s._h, v["B"], a(v["V"]), a(v["up"]), a(v["tr"]), a(v["w"]), v["w_stride"], a(v["lb"]), a(v["ub"]),
               v["stride"], v["n_pin"], a(v["Vbar"]), v["hessian"], a(v["x0b"]), a(v["upb"]), a(v["trb"]), a(v["wb"]),
               a(v["adj"]), a(v["st"]))
        L = s._L
        out = []
        for fn, args in ((L.mmpc_solve_vjp_batch, pre + (a(v["ws"]), v["ws_bytes"], None)),
                         (L.mmpc_solve_vjp_batch_host, pre)):
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
           ("V_bar", dict(Vbar=None))]
    for name, change in bad:
        for rc, msg in g.call_both(s, **change):
            assert rc == -1, (name, change, rc, msg)
            assert name in msg, (name, change, msg)
    for rc, msg in g.call_both(s):   # the arguments pass: the call goes on to look for its device
        assert rc in (-5, -6), (rc, msg)
    with pytest.raises(mmpc_mod.MmpcError, match="n_pin") as e:
        s.solve_vjp_host(g.V, g.up, g.tr, np.ones(nx + 2 * nu), g.Vbar, n_pin=N)
    assert e.value.code == -1
    with pytest.raises(mmpc_mod.MmpcError, match="hessian") as e:
        s.solve_vjp(B, a(g.V), a(g.up), a(g.tr), a(g.w), a(g.Vbar), x0_bar=a(g.x0b), u_prev_bar=a(g.upb),
                    vjp_status=a(g.st), backward_only=True, hessian=7)
    assert e.value.code == -1
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_forward_outputs_need_the_workspace(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    g = Args(s, B)
    none = dict(trb=None, wb=None, adj=None)
    for keep in ("trb", "wb", "adj"):
        only = {k: v for k, v in none.items() if k != keep}
        for change in (dict(ws=None), dict(ws=None, ws_bytes=0), dict(ws_bytes=g.ws_bytes - 1), dict(ws_bytes=0)):
            (rc, msg), (rch, msgh) = g.call_both(s, **only, **change)
            assert rc == -1 and "workspace" in msg, (keep, change, rc, msg)
            assert rch in (-5, -6), (rch, msgh)   # the host entry allocates its own
    for change in (dict(ws=None, ws_bytes=0), dict(ws_bytes=0), {}):   # backward-only: no workspace needed
        for rc, msg in g.call_both(s, **none, **change):
            assert rc in (-5, -6), (change, rc, msg)
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_workspace_query(model, nx, nu, mmpc_mod, tmp_path):
    N = 5
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    last = 0
    for B in (1, 2, 63, 64, 65, 128, 129, 4096, 65536):
        n = s.solve_vjp_workspace_bytes(B)
        assert n > 0 and n >= last, (B, n, last)
        assert n == -(-B // 64) * 64 * N * nu * (nx + nu + 1) * 8, (B, n)
        last = n
    assert s.solve_vjp_workspace_bytes(0) == 0
    n = C.c_uint64(7)
    assert s._L.mmpc_solve_vjp_workspace_bytes(s._h, -1, C.byref(n)) == -1
    assert s._L.mmpc_solve_vjp_workspace_bytes(s._h, 1, None) == -1
    assert s._L.mmpc_solve_vjp_workspace_bytes(None, 1, C.byref(n)) == -1
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
    assert s._L.mmpc_solve_vjp_batch(s._h, 0, None, None, None, None, 0, None, None, 0, 0, None, 0, None, None, None,
                                     None, None, None, None, 0, None) == 0
    assert s._L.mmpc_solve_vjp_batch_host(s._h, 0, None, None, None, None, 0, None, None, 0, 0, None, 0, None, None,
                                          None, None, None, None) == 0
    s.close()


def test_linear_mode_is_unsupported(mmpc_mod, model_json):
    N, B = 3, 2
    s = mmpc_mod.Solver(model_json(N=N, is_linear=True, name="linear_double_pendulum"), device=NO_SUCH_DEVICE)
    g = Args(s, B)
    for rc, msg in g.call_both(s, lb=None, ub=None):
        assert rc == -4 and "linear" in msg, (rc, msg)
    s.close()


def test_finite_state_bounds_are_unsupported(mmpc_mod, tmp_path):
    N, B, nx, nu = 3, 2, 4, 2
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N)
    g = Args(s, B)
    s.set_state_bounds(None, np.array([np.inf, np.inf, 1.5, np.inf]))
    for rc, msg in g.call_both(s):
        assert rc == -4 and "state bounds" in msg, (rc, msg)
    s.set_state_bounds(None, None)   # infinite again: the arguments pass, the call goes on to look for its device
    for rc, msg in g.call_both(s):
        assert rc in (-5, -6), (rc, msg)
    s.close()
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N, x_max=[10e30, 10e30, 2.0, 10e30])
    for rc, msg in g.call_both(s):
        assert rc == -4 and "state bounds" in msg, (rc, msg)
    s.close()
