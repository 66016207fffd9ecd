"""CPU: the barrier-rule entry points of the C-ABI (include/mmpc.h mmpc_set_barrier_rule / mmpc_get_barrier_rule,
enum mmpc_barrier_rule) and their Python binding -- host-only logic, no solve is launched here.  The rule selects
Mehrotra's predictor-corrector for the interior point of state-bounded solves; it arrives as additive
entry points, so the ABI version and mmpc_opts stay as they are."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_and_exported(mmpc_mod):
    names = mmpc_mod.header_functions()
    assert "mmpc_set_barrier_rule" in names and "mmpc_get_barrier_rule" in names
    L = mmpc_mod.lib()
    assert hasattr(L, "mmpc_set_barrier_rule") and hasattr(L, "mmpc_get_barrier_rule")
    assert (mmpc_mod.BARRIER_MONOTONE, mmpc_mod.BARRIER_MEHROTRA) == (0, 1)
    header = open(mmpc_mod.HEADER_PATH).read()
    assert "MMPC_BARRIER_MONOTONE = 0" in header and "MMPC_BARRIER_MEHROTRA = 1" in header


def test_abi_version_unchanged(mmpc_mod):
    assert mmpc_mod.lib().mmpc_abi_version() == 6
    assert C.sizeof(mmpc_mod.Opts) == 56   # mmpc_opts of ABI 6 (9 int32 + 2 double, padded): the rule is no option field


def test_default_set_get(model_json, mmpc_mod):
    m = mmpc_mod
    s = m.Solver(model_json(N=30))
    assert s.barrier_rule() == m.BARRIER_MONOTONE
    s.set_barrier_rule(m.BARRIER_MEHROTRA)
    assert s.barrier_rule() == m.BARRIER_MEHROTRA
    s.set_barrier_rule(m.BARRIER_MONOTONE)
    assert s.barrier_rule() == m.BARRIER_MONOTONE
    s.close()
    s = m.Solver(model_json(N=30, name="ctor"), barrier_rule=m.BARRIER_MEHROTRA)
    assert s.barrier_rule() == m.BARRIER_MEHROTRA
    s.close()


def test_invalid_rule_names_the_argument(model_json, mmpc_mod):
    s = mmpc_mod.Solver(model_json(N=30))
    L = mmpc_mod.lib()
    for bad in (2, -1, 7):
        assert L.mmpc_set_barrier_rule(s._h, bad) == -1   # MMPC_ERR_INVALID_ARG
        assert "rule" in L.mmpc_last_error().decode()
        assert s.barrier_rule() == mmpc_mod.BARRIER_MONOTONE
    assert L.mmpc_set_barrier_rule(None, 0) == -1
    assert L.mmpc_get_barrier_rule(s._h, None) == -1
    s.close()


def test_rule_does_not_change_auto(tmp_path, model_json, mmpc_mod):
    """MMPC_KKT_AUTO and the Hessian resolution are those of the monotone rule (the rule refuses what it cannot run)"""
    m = mmpc_mod
    s = m.Solver(model_json(N=30))
    s.set_state_bounds([-np.inf, -np.inf, -1.5, -1.5], [np.inf, np.inf, 1.5, 1.5])
    before = [(s.kkt_solver_for(B), s.hessian_for(B)) for B in (1, 64, 4096, 65536)]
    s.set_barrier_rule(m.BARRIER_MEHROTRA)
    assert [(s.kkt_solver_for(B), s.hessian_for(B)) for B in (1, 64, 4096, 65536)] == before
    assert before[-1][0] == m.KKT_RICCATI and before[0][0] == m.KKT_RICCATI_GROUP


def test_reserved_bytes_do_not_depend_on_the_rule(tmp_path, model_json, mmpc_mod):
    """mmpc_reserve_workspace reserves for either rule (the size is reported before a device is touched), so setting
    the rule after a reservation never makes a solve grow the workspace under a captured graph"""
    m = mmpc_mod
    exo = m.write_model_json(str(tmp_path / "exo20.json"), "exo20", 8, 4, 2000, 20, model="exo_arm")
    for path, nx, nu, N in ((model_json(N=30), 4, 2, 30), (exo, 8, 4, 20)):
        s = m.Solver(path)
        b = C.c_uint64(0)
        B = 4096
        s._L.mmpc_reserve_workspace(s._h, B, C.byref(b))
        plain = b.value
        # at least the Mehrotra variant's 16-lane workspace (group_ws_doubles): K | kff, W blocks, z_l z_u Sigma b
        # z_u-z_l, ccl ccu, and the corrector sweep's per-stage record
        per = (N * nu * (nx + nu + 1) + N * (nx * (nx + nu) + nu * nu) + 7 * N * (nx + nu)
               + N * ((2 + nu) * 16 + nu * (nu + 1) // 2 + nu))
        assert plain >= per * B * 8
        s.set_barrier_rule(m.BARRIER_MEHROTRA)
        s._L.mmpc_reserve_workspace(s._h, B, C.byref(b))
        assert b.value == plain
        s.set_state_bounds([-1.0] * nx, [1.0] * nx)
        s._L.mmpc_reserve_workspace(s._h, B, C.byref(b))
        assert b.value == plain
        s.set_barrier_rule(m.BARRIER_MONOTONE)
        s._L.mmpc_reserve_workspace(s._h, B, C.byref(b))
        assert b.value == plain
        s.close()


def test_environment_override_in_a_fresh_process(tmp_path, model_json):
    """MMPC_BARRIER_RULE (0 or 1) is read when a handle is created; anything else leaves the default"""
    path = model_json(N=30)
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import mmpc; "
            "s = mmpc.Solver(sys.argv[2]); print(s.barrier_rule())")
    for val, want in (("1", 1), (None, 0), ("2", 0)):
        env = {k: v for k, v in os.environ.items() if k != "MMPC_BARRIER_RULE"}
        if val is not None:
            env["MMPC_BARRIER_RULE"] = val
        out = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "mahi-mpc_amd"), path], env=env,
                             capture_output=True, text=True, check=True).stdout
        assert int(out.strip().splitlines()[-1]) == want, (val, out)
