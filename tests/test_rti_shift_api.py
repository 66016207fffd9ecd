"""CPU: the shift between two ticks of a real-time iteration loop, mmpc_rti_shift_batch (include/mmpc.h; additive to ABI
6).

The handles ask for a device index no machine has (as tests/test_rti_api.py does), so every answer below comes from the
arguments alone, before any device call, and the test is the same with and without a GPU:

* the header declares the function, the library exports it, the Python layer has its prototype and Solver.rti_shift;
  the ABI version stays 6;
* n_shift outside 0 .. N is MMPC_ERR_INVALID_ARG naming `n_shift`; a NULL V_in or V_out is MMPC_ERR_INVALID_ARG naming
  the argument; V_out == V_in is MMPC_ERR_INVALID_ARG naming both; u_prev_out may be NULL;
* a valid call goes on to look for its device (-5 or -6), for every n_shift in 0 .. N;
* a linear-mode model is MMPC_ERR_UNSUPPORTED; a state-bounded handle is accepted;
* B = 0 is a no-op success, B < 0 and a NULL handle are refused."""
import numpy as np
import pytest

MODELS = [("two_link_arm", 4, 2), ("exo_arm", 8, 4)]
NO_SUCH_DEVICE = 4096   # mmpc_create touches no device
a = lambda v: None if v is None else v.ctypes.data   # noqa: E731


def _solver(mmpc_mod, tmp_path, model, nx, nu, N, **kw):
    p = mmpc_mod.write_model_json(str(tmp_path / f"{model}_{N}.json"), model, nx, nu, 2000, N, model=model, **kw)
    return mmpc_mod.Solver(p, device=NO_SUCH_DEVICE)


def call(s, B, V_in, n, V_out, up):
    rc = s._L.mmpc_rti_shift_batch(s._h, B, a(V_in), n, a(V_out), a(up), None)
    return rc, s._L.mmpc_last_error().decode()


def test_header_declares_and_library_exports(mmpc_mod):
    L = mmpc_mod.lib()
    assert "mmpc_rti_shift_batch" in mmpc_mod.header_functions()
    assert hasattr(L, "mmpc_rti_shift_batch") and len(L.mmpc_rti_shift_batch.argtypes) == 7
    assert hasattr(mmpc_mod.Solver, "rti_shift")
    assert L.mmpc_abi_version() == 6


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_argument_rules(model, nx, nu, mmpc_mod, tmp_path):
    N, B = 3, 2
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, N)
    Vi, Vo, up = np.zeros((B, s.NV)), np.zeros((B, s.NV)), np.zeros((B, nu))
    for n in (-1, N + 1, 1 << 20):
        rc, msg = call(s, B, Vi, n, Vo, up)
        assert rc == -1 and "n_shift" in msg, (n, rc, msg)
    rc, msg = call(s, B, None, 1, Vo, up)
    assert rc == -1 and "V_in" in msg and "V_out" not in msg, (rc, msg)
    rc, msg = call(s, B, Vi, 1, None, up)
    assert rc == -1 and "V_out" in msg and "V_in" not in msg, (rc, msg)
    rc, msg = call(s, B, Vi, 1, Vi, up)
    assert rc == -1 and "V_out" in msg and "V_in" in msg, (rc, msg)
    for n in range(N + 1):   # the arguments pass: the call goes on to look for its device
        for u in (up, None):
            rc, msg = call(s, B, Vi, n, Vo, u)
            assert rc in (-5, -6), (n, rc, msg)
    with pytest.raises(mmpc_mod.MmpcError, match="n_shift") as e:
        s.rti_shift(B, a(Vi), N + 1, V_out=a(Vo), u_prev_out=a(up))
    assert e.value.code == -1
    s.close()


@pytest.mark.parametrize("model,nx,nu", MODELS)
def test_zero_instances_is_a_no_op(model, nx, nu, mmpc_mod, tmp_path):
    s = _solver(mmpc_mod, tmp_path, model, nx, nu, 3)
    assert s._L.mmpc_rti_shift_batch(s._h, 0, None, 1, None, None, None) == 0
    assert s._L.mmpc_rti_shift_batch(s._h, 0, None, 0, None, None, None) == 0
    V = np.zeros((1, s.NV))
    assert call(s, 0, V, 3, V, None)[0] == 0
    assert call(s, -1, V, 1, np.zeros((1, s.NV)), None)[0] == -1
    assert s._L.mmpc_rti_shift_batch(None, 1, a(V), 1, a(np.zeros((1, s.NV))), None, None) == -1
    s.close()


def test_linear_mode_is_unsupported(mmpc_mod, model_json):
    N, B = 3, 2
    s = mmpc_mod.Solver(model_json(N=N, is_linear=True, name="linear_double_pendulum"), device=NO_SUCH_DEVICE)
    rc, msg = call(s, B, np.zeros((B, s.NV)), 1, np.zeros((B, s.NV)), None)
    assert rc == -4 and "linear" in msg, (rc, msg)
    s.close()


def test_state_bounded_handle_is_accepted(mmpc_mod, tmp_path):
    N, B, nx, nu = 3, 2, 4, 2
    s = _solver(mmpc_mod, tmp_path, "two_link_arm", nx, nu, N)
    s.set_state_bounds(None, np.array([np.inf, np.inf, 1.5, np.inf]))
    for barrier in ("off", "on"):
        if barrier == "on":
            s.set_sensitivity_barrier()
        rc, msg = call(s, B, np.zeros((B, s.NV)), 1, np.zeros((B, s.NV)), np.zeros((B, nu)))
        assert rc in (-5, -6), (barrier, rc, msg)
    s.close()
