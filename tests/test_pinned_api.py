"""CPU: the committed-controls entry points of include/mmpc.h (mmpc_*_pinned, additive to ABI 6).

* the header declares the three functions and the library exports them;
* the ABI version stays 6 and sizeof(mmpc_opts) stays 56;
* n_pin in {-1, N, N + 3}, and n_pin = 1 with a NULL u_pin, are MMPC_ERR_INVALID_ARG with the argument's name in
  mmpc_last_error on handles created without a device, on the device-pointer, the host and the multi-device entry:
  the pins are validated from the arguments alone, before any device call;
* weights_stride < 0 or in 1 .. nx + 2 nu - 1 is MMPC_ERR_INVALID_ARG with `weights_stride` in mmpc_last_error on the
  five solve entry points (the one check of a solve's arguments, check_solve_args in mmpc.hip), likewise before any
  device call;
* a linear-mode model with n_pin = 1 is MMPC_ERR_UNSUPPORTED;
* the Python wrappers refuse a wrongly shaped u_pin with ValueError before the library is called."""
import ctypes as C

import numpy as np
import pytest

NEW = ["mmpc_solve_batch_pinned", "mmpc_solve_batch_host_pinned", "mmpc_multi_solve_batch_host_pinned"]
MODELS = [("two_link_arm", 4, 2), ("exo_arm", 8, 4)]
a = lambda v: v.ctypes.data   # noqa: E731


def test_header_declares_and_library_exports(mmpc_mod):
    names = mmpc_mod.header_functions()
    L = mmpc_mod.lib()
    for fn in NEW:
        assert fn in names, fn
        assert hasattr(L, fn), fn
        assert getattr(L, fn).argtypes is not None, fn


def test_abi_version_and_opts_size_unchanged(mmpc_mod):
    assert mmpc_mod.lib().mmpc_abi_version() == 6
    assert C.sizeof(mmpc_mod.Opts) == 56


def _arrays(nx, nu, N, B, NV):
    return (np.zeros((B, nx)), np.zeros((B, nu)), np.zeros((B, N, nx)), np.ones(nx + 2 * nu), np.zeros((B, NV)),
            np.zeros((B, N + 3, nu)))


def _bad_pins(N, pin):
    """(u_pin, n_pin, the argument mmpc_last_error must name)"""
    return [(a(pin), -1, "n_pin"), (a(pin), N, "n_pin"), (a(pin), N + 3, "n_pin"), (None, 1, "u_pin")]


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_bad_pins_are_refused_before_any_device_call(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    p = mmpc_mod.write_model_json(str(tmp_path / f"{model}.json"), model, nx, nu, 2000, N, model=model)
    s = mmpc_mod.Solver(p)   # mmpc_create touches no device
    L = s._L
    x0, up, tr, w, V, pin = _arrays(nx, nu, N, B, s.NV)
    for u_pin, n_pin, name in _bad_pins(N, pin):
        rc = L.mmpc_solve_batch_host_pinned(s._h, B, a(x0), a(up), a(tr), a(w), 0, None, None, 0, u_pin, n_pin, a(V),
                                            None, None, None)
        assert rc == -1, (n_pin, rc)
        assert name in L.mmpc_last_error().decode(), (n_pin, L.mmpc_last_error())
        rc = L.mmpc_solve_batch_pinned(s._h, B, a(x0), a(up), a(tr), a(w), 0, None, None, 0, u_pin, n_pin, a(V), None,
                                       None, None, None, None)
        assert rc == -1, (n_pin, rc)
        assert name in L.mmpc_last_error().decode(), (n_pin, L.mmpc_last_error())
        with pytest.raises(mmpc_mod.MmpcError, match=name) as e:
            s.solve_batch(B, a(x0), a(up), a(tr), a(w), a(V), u_pin=u_pin, n_pin=n_pin)
        assert e.value.code == -1
    s.close()


def test_bad_pins_are_refused_by_the_multi_device_entry(mmpc_mod, tmp_path):
    """mmpc_multi_create opens no device either: the pins are refused before a shard starts"""
    nx, nu, N, B = 4, 2, 3, 5
    p = mmpc_mod.write_model_json(str(tmp_path / "m.json"), "two_link_arm", nx, nu, 2000, N, model="two_link_arm")
    m = mmpc_mod.MultiSolver(p, [0, 0])
    L = m._L
    x0, up, tr, w, V, pin = _arrays(nx, nu, N, B, m.NV)
    for u_pin, n_pin, name in _bad_pins(N, pin):
        rc = L.mmpc_multi_solve_batch_host_pinned(m._m, B, a(x0), a(up), a(tr), a(w), 0, None, None, 0, u_pin, n_pin,
                                                  a(V), None, None, None)
        assert rc == -1 and name in L.mmpc_last_error().decode(), (n_pin, rc, L.mmpc_last_error())
    m.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_bad_weights_stride_is_refused_by_every_solve_entry(model, nx, nu, mmpc_mod, tmp_path):
    """weights_stride < 0 or in 1 .. nx + 2 nu - 1 is MMPC_ERR_INVALID_ARG naming the argument, from the arguments
    alone (handles created without a device), on the five solve entry points: no entry sizes a copy or a send by it, or
    goes to a device, before it is checked"""
    N, B = 3, 5
    p = mmpc_mod.write_model_json(str(tmp_path / f"{model}.json"), model, nx, nu, 2000, N, model=model)
    s = mmpc_mod.Solver(p)
    m = mmpc_mod.MultiSolver(p, [0, 0])
    L = s._L
    x0, up, tr, _, V, _ = _arrays(nx, nu, N, B, s.NV)
    w = np.ones((B, nx + 2 * nu))
    lb, ub = -np.ones(nu), np.ones(nu)
    pre = (B, a(x0), a(up), a(tr), a(w))
    for ws in (-1, 1, nx + 2 * nu - 1):
        calls = {
            "mmpc_solve_batch_bounds": (s._h, *pre, ws, a(lb), a(ub), 0, a(V), None, None, None, None, None),
            "mmpc_solve_batch_pinned": (s._h, *pre, ws, a(lb), a(ub), 0, None, 0, a(V), None, None, None, None, None),
            "mmpc_solve_batch_host_pinned": (s._h, *pre, ws, a(lb), a(ub), 0, None, 0, a(V), None, None, None),
            "mmpc_multi_solve_batch_host_pinned": (m._m, *pre, ws, a(lb), a(ub), 0, None, 0, a(V), None, None, None),
            "mmpc_multi_solve_batch_rccl_bounds": (m._m, *pre, ws, a(lb), a(ub), 0, a(V), None, None, None, None),
        }
        for fn, args in calls.items():
            rc = getattr(L, fn)(*args)
            assert rc == -1, (fn, ws, rc, L.mmpc_last_error())
            assert "weights_stride" in L.mmpc_last_error().decode(), (fn, ws, L.mmpc_last_error())
    s.close()
    m.close()


def test_linear_mode_with_pins_is_unsupported(mmpc_mod, model_json):
    """the reference linearises at the measured (x_0, u_prev); the reduction would linearise at x_m"""
    N, B, nx, nu = 3, 2, 4, 2
    s = mmpc_mod.Solver(model_json(N=N, is_linear=True, name="linear_double_pendulum"))
    L = s._L
    x0, up, tr, w, V, pin = _arrays(nx, nu, N, B, s.NV)
    rc = L.mmpc_solve_batch_host_pinned(s._h, B, a(x0), a(up), a(tr), a(w), 0, None, None, 0, a(pin), 1, a(V), None,
                                        None, None)
    assert rc == -4, rc
    assert "linear" in L.mmpc_last_error().decode()
    rc = L.mmpc_solve_batch_pinned(s._h, B, a(x0), a(up), a(tr), a(w), 0, None, None, 0, a(pin), 1, a(V), None, None,
                                   None, None, None)
    assert rc == -4, rc
    with pytest.raises(mmpc_mod.MmpcError) as e:
        s.solve_batch_host(x0, up, tr, w, u_pin=np.zeros((B, 1, nu)))
    assert e.value.code == -4
    s.close()
    m = mmpc_mod.MultiSolver(model_json(N=N, is_linear=True, name="linear_double_pendulum"), [0, 0])
    rc = m._L.mmpc_multi_solve_batch_host_pinned(m._m, B, a(x0), a(up), a(tr), a(w), 0, None, None, 0, a(pin), 1,
                                                 a(V), None, None, None)
    assert rc == -4, rc
    m.close()


def test_host_pins_shapes(mmpc_mod):
    """[B, m, nu] with m from the shape, 0 <= m <= N - 1; anything else raises before the library is called"""
    hp = mmpc_mod._host_pins
    assert hp(None, 3, 2, 5) == (None, 0)
    pin, m = hp(np.arange(12.0).reshape(3, 2, 2)[:, :, ::-1], 3, 2, 5)
    assert m == 2 and pin.shape == (3, 2, 2) and pin.flags.c_contiguous and pin.dtype == np.float64
    assert hp(np.zeros((3, 0, 2)), 3, 2, 5) == (None, 0)
    assert hp(np.zeros((3, 4, 2)), 3, 2, 5)[1] == 4
    for bad in (np.zeros((3, 2)), np.zeros((4, 2, 2)), np.zeros((3, 2, 3)), np.zeros((3, 5, 2)), np.zeros(6)):
        with pytest.raises(ValueError):
            hp(bad, 3, 2, 5)


def test_wrappers_refuse_a_wrong_shape_before_the_library(mmpc_mod, tmp_path):
    nx, nu, N, B = 4, 2, 3, 5
    p = mmpc_mod.write_model_json(str(tmp_path / "m.json"), "two_link_arm", nx, nu, 2000, N, model="two_link_arm")
    x0, up, tr, w, _, _ = _arrays(nx, nu, N, B, 0)
    s = mmpc_mod.Solver(p)
    m = mmpc_mod.MultiSolver(p, [0, 0])
    for obj in (s, m):
        for bad in (np.zeros((B, nu)), np.zeros((B + 1, 1, nu)), np.zeros((B, 1, nu + 1)), np.zeros((B, N, nu))):
            with pytest.raises(ValueError, match="u_pin"):
                obj.solve_batch_host(x0, up, tr, w, u_pin=bad)
    s.close()
    m.close()
