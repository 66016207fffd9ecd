"""CPU: the feedback-gain entry points of include/mmpc.h (mmpc_feedback_gains_batch[_host], additive to ABI 6).

The handles ask for a device index no machine has (as tests/test_workspace_layout.py does), so every answer below comes
from the arguments alone, before any device call, and the test is the same with and without a GPU:

* the header declares the two functions, the library exports them and the Python layer has their prototypes; the ABI
  version stays 6 and sizeof(mmpc_opts) stays 56;
* n_gain in {0, N + 1}, n_pin in {-1, N}, a bounds_stride in 1 .. nu - 1, an unknown hessian and an unknown kernel are
  MMPC_ERR_INVALID_ARG with the argument's name in mmpc_last_error, on the device and on the host entry;
* a linear-mode model and a handle with a finite state bound are MMPC_ERR_UNSUPPORTED;
* the 16-lane kernel (kernel = 2) is MMPC_ERR_UNSUPPORTED for a model with nx + nu = 16 (the generated mass_chain of
  host/examples/sx_model_zoo.cpp, served by its own library) and at a horizon whose stage records exceed the LDS;
* B = 0 returns MMPC_OK."""
import ctypes as C
import os

import numpy as np
import pytest

NEW = ["mmpc_feedback_gains_batch", "mmpc_feedback_gains_batch_host"]
MODELS = [("two_link_arm", 4, 2), ("exo_arm", 8, 4)]
NO_SUCH_DEVICE = 4096   # mmpc_create touches no device
a = lambda v: v.ctypes.data   # noqa: E731


def test_header_declares_and_library_exports(mmpc_mod):
    names = mmpc_mod.header_functions()
    L = mmpc_mod.lib()
    for fn in NEW:
        assert fn in names, fn
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes is not None, fn
    assert hasattr(mmpc_mod.Solver, "feedback_gains") and hasattr(mmpc_mod.Solver, "feedback_gains_host")


def test_abi_version_and_opts_size_unchanged(mmpc_mod):
    assert mmpc_mod.lib().mmpc_abi_version() == 6
    assert C.sizeof(mmpc_mod.Opts) == 56


def _solver(mmpc_mod, tmp_path, model, nx, nu, N, **kw):
    p = mmpc_mod.write_model_json(str(tmp_path / f"{model}_{N}.json"), model, nx, nu, 2000, N, model=model, **kw)
    return mmpc_mod.Solver(p, device=NO_SUCH_DEVICE)


def _arrays(nx, nu, N, B, NV):
    return (np.zeros((B, NV)), np.zeros((B, nu)), np.zeros((B, N, nx)), np.ones(nx + 2 * nu), -np.ones(nu),
            np.ones(nu), np.zeros((B, N, nu, nx + nu)), np.zeros(B, np.int32))


def _call_both(s, B, V, up, tr, w, lb, ub, stride, n_pin, n_gain, hessian, kernel, G, st):
    """(rc, mmpc_last_error) of the device entry and of the host entry"""
    L = s._L
    pre = (s._h, B, a(V), a(up), a(tr), a(w), 0, None if lb is None else a(lb), None if ub is None else a(ub), stride,
           n_pin, n_gain, hessian, kernel, a(G), a(st))
    out = []
    for fn, args in ((L.mmpc_feedback_gains_batch, pre + (None,)), (L.mmpc_feedback_gains_batch_host, pre)):
        rc = fn(*args)
        out.append((rc, L.mmpc_last_error().decode()))
    return out


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_bad_arguments_are_refused_before_any_device_call(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)
    good = dict(stride=0, n_pin=0, n_gain=N, hessian=0, kernel=0)
    bad = [("n_gain", dict(n_gain=0)), ("n_gain", dict(n_gain=N + 1)), ("n_pin", dict(n_pin=-1)),
           ("n_pin", dict(n_pin=N)), ("bounds_stride", dict(stride=nu - 1)), ("bounds_stride", dict(stride=-1)),
           ("hessian", dict(hessian=3)), ("hessian", dict(hessian=-1)), ("kernel", dict(kernel=3)),
           ("kernel", dict(kernel=-1))]
    for name, change in bad:
        kw = dict(good, **change)
        for rc, msg in _call_both(s, B, V, up, tr, w, lb, ub, kw["stride"], kw["n_pin"], kw["n_gain"], kw["hessian"],
                                  kw["kernel"], G, st):
            assert rc == -1, (name, change, rc, msg)
            assert name in msg, (name, change, msg)
        with pytest.raises(mmpc_mod.MmpcError, match=name) as e:
            if "stride" in change:
                s.feedback_gains(B, a(V), a(up), a(tr), a(w), G=a(G), gain_status=a(st), u_lb=a(lb), u_ub=a(ub),
                                 bounds_stride=kw["stride"])
            else:
                s.feedback_gains_host(V, up, tr, w, u_lb=lb, u_ub=ub, n_pin=kw["n_pin"], n_gain=kw["n_gain"],
                                      hessian=kw["hessian"], kernel=kw["kernel"])
        assert e.value.code == -1
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_zero_instances_is_a_no_op(model, nx, nu, mmpc_mod, tmp_path):
    N = 3
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, 1, s.NV)
    for kernel in (0, 1, 2):
        for rc, msg in _call_both(s, 0, V, up, tr, w, lb, ub, 0, 0, N, 0, kernel, G, st):
            assert rc == 0, (rc, msg)
    assert s._L.mmpc_feedback_gains_batch(s._h, 0, None, None, None, None, 0, None, None, 0, 0, 1, 0, 0, None, None,
                                          None) == 0
    s.close()


def test_linear_mode_is_unsupported(mmpc_mod, model_json):
    N, B, nx, nu = 3, 2, 4, 2
    s = mmpc_mod.Solver(model_json(N=N, is_linear=True, name="linear_double_pendulum"), device=NO_SUCH_DEVICE)
    V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)
    for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, 0, G, st):
        assert rc == -4 and "linear" in msg, (rc, msg)
    s.close()


def test_finite_state_bounds_are_unsupported(mmpc_mod, tmp_path):
    N, B, nx, nu = 3, 2, 4, 2
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N)
    V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)
    s.set_state_bounds(None, np.array([np.inf, np.inf, 1.5, np.inf]))
    for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, 0, G, st):
        assert rc == -4 and "state bounds" in msg, (rc, msg)
    s.set_state_bounds(None, None)   # infinite again: the arguments pass, the call goes on to look for its device
    for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, 0, G, st):
        assert rc in (-5, -6), (rc, msg)
    s.close()
    # x_max of the JSON (ModelParameters.cpp:66-69) bounds the handle from its creation
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N, x_max=[10e30, 10e30, 2.0, 10e30])
    for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, 0, G, st):
        assert rc == -4 and "state bounds" in msg, (rc, msg)
    s.close()


def test_group_kernel_needs_fewer_than_sixteen_columns(mmpc_mod):
    """kernel = 2 holds one column of P per lane of its 16: nx + nu = 16 is refused, the lane kernel and AUTO are not"""
    path = os.path.join(mmpc_mod.USER_LIB_DIR, "mass_chain.json")
    assert os.path.exists(path), "build() generates the models of sx_model_zoo.cpp"
    s = mmpc_mod.Solver(path, device=NO_SUCH_DEVICE)
    nx, nu, N, B = s.nx, s.nu, s.N, 2
    assert (nx, nu) == (12, 4) and s.info.model_id == mmpc_mod.MODEL_USER
    V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)
    for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, 2, G, st):
        assert rc == -4 and "kernel" in msg and "nx + nu < 16" in msg, (rc, msg)
    for kernel in (0, 1):   # the arguments pass: the call goes on to look for its device
        for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, kernel, G, st):
            assert rc in (-5, -6), (kernel, rc, msg)
    s.close()


def test_group_kernel_needs_its_records_in_lds(mmpc_mod, tmp_path):
    """kernel = 2 keeps an instance's stage records in LDS: 160 KB hold 81 exact-Hessian stages of the exo
    (249 doubles each, 192 for the exchange area); AUTO never picks the 16-lane kernel there"""
    nx, nu, B = 8, 4, 2
    for N, rc_want in ((81, (-5, -6)), (82, (-4,))):
        s = _solver(mmpc_mod, tmp_path, "exo_arm", nx, nu, N)
        V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)
        for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, 1, 0, 2, G[:, :1].copy(), st):
            assert rc in rc_want, (N, rc, msg)
            if rc == -4:
                assert "kernel" in msg and "LDS" in msg, msg
        s.close()
