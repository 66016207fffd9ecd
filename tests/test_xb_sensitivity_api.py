"""CPU: the sensitivity barrier of a state-bounded handle (mmpc_set_sensitivity_barrier, include/mmpc.h).

The handles ask for a device index no machine has (as tests/test_feedback_gains_api.py does), so every answer comes
from the arguments and the handle alone, before any device call:

* the header declares the three functions, the library and the generated model libraries export them, the Python layer
  has their prototypes; ABI 6, sizeof(mmpc_opts) 56;
* the defaults are (mu_f, 1e12), mu_f recomputed here from the monotone schedule mu <- max(tol / 20, min(0.2 mu,
  mu^1.5)) from 0.1 until 2 mu <= tol = 1e-8 (the constants of csrc/sqp_wave.h);
* a negative, infinite or NaN mu and a sigma_cap that is <= 0 or NaN are MMPC_ERR_INVALID_ARG naming the argument and
  change nothing; sigma_cap = +inf is allowed;
* off by default: a state-bounded handle is refused by the gain and VJP entries with -4 and "state bounds"; on: the same
  calls pass the argument check and go on to look for their device (-5 / -6), as an unbounded handle does; off again:
  refused again;
* the 16-lane gain kernel's LDS rule is evaluated with the grown stage record: the exo's exact-Hessian horizon limit
  moves from 81 to 75 stages (249 + 20 doubles a stage, 192 for the exchange area)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_feedback_gains_api import NO_SUCH_DEVICE, _arrays, _call_both, _solver

NEW = ["mmpc_sensitivity_barrier_default", "mmpc_set_sensitivity_barrier", "mmpc_get_sensitivity_barrier"]
a = lambda v: v.ctypes.data   # noqa: E731


def mu_f():
    mu, tol = 0.1, 1e-8
    while 2.0 * mu > tol:
        mu = max(tol / 20.0, min(0.2 * mu, math.pow(mu, 1.5)))
    return mu


def test_header_declares_and_libraries_export(mmpc_mod):
    names = mmpc_mod.header_functions()
    L = mmpc_mod.lib()
    for fn in NEW:
        assert fn in names, fn
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes is not None, fn
    assert hasattr(mmpc_mod.Solver, "set_sensitivity_barrier") and hasattr(mmpc_mod.Solver, "sensitivity_barrier")
    user = os.path.join(mmpc_mod.USER_LIB_DIR, "mass_chain.json")
    assert os.path.exists(user), "build() generates the models of sx_model_zoo.cpp"
    U = mmpc_mod.lib(mmpc_mod.model_library(user))
    for fn in NEW:
        assert hasattr(U, fn), fn


def test_abi_version_and_opts_size_unchanged(mmpc_mod):
    assert mmpc_mod.lib().mmpc_abi_version() == 6
    assert C.sizeof(mmpc_mod.Opts) == 56


def test_defaults_are_the_schedules_last_value_and_1e12(mmpc_mod):
    mu, cap = C.c_double(), C.c_double()
    assert mmpc_mod.lib().mmpc_sensitivity_barrier_default(C.byref(mu), C.byref(cap)) == 0
    assert abs(mu_f() - 2.5059035596800618e-09) <= 1e-22
    assert mu.value == pytest.approx(mu_f(), rel=1e-14, abs=0.0)
    assert cap.value == 1e12
    assert mmpc_mod.lib().mmpc_sensitivity_barrier_default(None, C.byref(cap)) == -1


def test_setter_validation_and_round_trip(mmpc_mod, tmp_path):
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", 4, 2, 3)
    L = s._L
    assert s.sensitivity_barrier == (0.0, 1e12), "a new handle has the barrier off"
    s.set_sensitivity_barrier()
    assert s.sensitivity_barrier == (pytest.approx(mu_f(), rel=1e-14), 1e12)
    s.set_sensitivity_barrier(1e-7, 1e6)
    assert s.sensitivity_barrier == (1e-7, 1e6)
    for name, mu, cap in (("mu", -1e-9, 1e6), ("mu", np.inf, 1e6), ("mu", np.nan, 1e6), ("sigma_cap", 1e-9, 0.0),
                          ("sigma_cap", 1e-9, -1.0), ("sigma_cap", 1e-9, np.nan)):
        rc = L.mmpc_set_sensitivity_barrier(s._h, mu, cap)
        assert rc == -1 and name in L.mmpc_last_error().decode(), (name, mu, cap, rc, L.mmpc_last_error())
        with pytest.raises(mmpc_mod.MmpcError, match=name):
            s.set_sensitivity_barrier(mu, cap)
        assert s.sensitivity_barrier == (1e-7, 1e6), "a refused call changes nothing"
    s.set_sensitivity_barrier(1e-9, np.inf)
    assert s.sensitivity_barrier == (1e-9, np.inf)
    s.set_sensitivity_barrier(mu=0)
    assert s.sensitivity_barrier[0] == 0.0
    assert L.mmpc_set_sensitivity_barrier(None, 1e-9, 1e6) == -1
    s.close()
    p = mmpc_mod.write_model_json(str(tmp_path / "ctor.json"), "two_link_arm", 4, 2, 2000, 3, model="two_link_arm")
    for arg, want in ((True, (pytest.approx(mu_f(), rel=1e-14), 1e12)), (1e-8, (1e-8, 1e12)),
                      ((1e-8, 1e5), (1e-8, 1e5)), (False, (0.0, 1e12))):
        s = mmpc_mod.Solver(p, device=NO_SUCH_DEVICE, sensitivity_barrier=arg)
        assert s.sensitivity_barrier == want, arg
        s.close()


def _vjp_both(s, B, V, up, tr, w, N):
    L = s._L
    nx, nu = s.nx, s.nu
    Vb, x0b, st = np.zeros_like(V), np.zeros((B, nx)), np.zeros(B, np.int32)
    pre = (s._h, B, a(V), a(up), a(tr), a(w), 0, None, None, 0, 0, a(Vb), 0, a(x0b), None, None, None, None, a(st))
    out = []
    for fn, args in ((L.mmpc_solve_vjp_batch, pre + (None, 0, None)), (L.mmpc_solve_vjp_batch_host, pre)):
        rc = fn(*args)
        out.append((rc, L.mmpc_last_error().decode()))
    return out


@pytest.mark.parametrize("how", ["setter", "json"])
def test_switch_admits_and_refuses_a_state_bounded_handle(how, mmpc_mod, tmp_path):
    N, B, nx, nu = 3, 2, 4, 2
    if how == "json":   # x_max of the JSON (ModelParameters.cpp:66-69) bounds the handle from its creation
        s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N, x_max=[10e30, 10e30, 2.0, 10e30])
    else:
        s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N)
        s.set_state_bounds(None, np.array([np.inf, np.inf, 1.5, np.inf]))
    V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)

    def calls():
        return (_call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, 0, G, st)
                + _call_both(s, B, V, up, tr, w, lb, ub, 0, 0, N, 0, 2, G, st) + _vjp_both(s, B, V, up, tr, w, N))

    for rc, msg in calls():   # off is the state of a new handle
        assert rc == -4 and "state bounds" in msg and "mmpc_set_sensitivity_barrier" in msg, (rc, msg)
    s.set_sensitivity_barrier()
    for rc, msg in calls():   # the arguments pass: the call goes on to look for its device
        assert rc in (-5, -6), (rc, msg)
    for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N + 1, 0, 0, G, st):
        assert rc == -1 and "n_gain" in msg, (rc, msg)   # the other checks are as before
    s.set_sensitivity_barrier(mu=0)
    for rc, msg in calls():
        assert rc == -4 and "state bounds" in msg, (rc, msg)
    s.close()


def test_unbounded_handle_ignores_the_setting(mmpc_mod, tmp_path):
    N, B, nx, nu = 3, 2, 4, 2
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N)
    V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)
    for on in (False, True):
        if on:
            s.set_sensitivity_barrier()
        for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, N, 0, 0, G, st) + _vjp_both(s, B, V, up, tr,
                                                                                                       w, N):
            assert rc in (-5, -6), (on, rc, msg)
    s.close()


def test_group_kernel_lds_rule_uses_the_grown_record(mmpc_mod, tmp_path):
    """exact-Hessian exo: 81 stages of 249 doubles fit 160 KB beside the 192 of the exchange area, 75 of 269 do"""
    nx, nu, B = 8, 4, 2
    xmax = [10e30] * 4 + [0.3] * 4
    for N, bounded, rc_want in ((81, False, (-5, -6)), (75, True, (-5, -6)), (76, True, (-4,)), (81, True, (-4,))):
        s = _solver(mmpc_mod, tmp_path, "exo_arm", nx, nu, N, **(dict(x_max=xmax) if bounded else {}))
        s.set_sensitivity_barrier()
        V, up, tr, w, lb, ub, G, st = _arrays(nx, nu, N, B, s.NV)
        for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, 1, 0, 2, G[:, :1].copy(), st):
            assert rc in rc_want, (N, bounded, rc, msg)
            if rc == -4:
                assert "kernel" in msg and "LDS" in msg, msg
        for rc, msg in _call_both(s, B, V, up, tr, w, None, None, 0, 0, 1, 0, 0, G[:, :1].copy(), st):
            assert rc in (-5, -6), (N, bounded, rc, msg)   # AUTO never picks a kernel that does not fit
        s.close()
