"""GPU: a plain ``bench.py`` run (no --full) prints the headline line alone, and ``--dump-outputs`` writes what the
last timed step returned: the same arrays from run to run, u_0* (stored by the kernel into host memory) equal to its
slice of V, and the solution of block 0 that Solver.solve_batch_host computes for the same instances."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, WEIGHTS_CFG

pytestmark = pytest.mark.gpu

B = 300   # no multiple of the 16-lane kernel's instances per block; more than one block


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", str(B), *args],
                       capture_output=True, text=True, timeout=110, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step(tmp_path, mmpc_mod, oracle):
    outs = [_bench("--steps", str(k), "--warmup", "1", "--dump-outputs", str(tmp_path / d))
            for k, d in ((3, "a"), (2, "b"))]
    for out, k in zip(outs, (3, 2)):
        assert out["steps"] == k and out["converged"] == B and out["gathered_results_match"] is True
        assert out["value"] == pytest.approx(B * 1e3 / out["ms_per_step"], rel=1e-9)
        for key in ("value_solve_only", "kernel_ms", "roofline", "secondary", "tolerance_sweep", "cpu_baseline"):
            assert key not in out
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("V", "u0", "status", "iters")}
    assert sorted(os.listdir(tmp_path / "a")) == ["V.npy", "iters.npy", "status.npy", "u0.npy"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["V"].shape == (B, 184) and a["u0"].shape == (B, 2) and a["status"].shape == a["iters"].shape == (B,)
    # the last step solves block 0 whatever K is: both runs dump the same arrays, bit for bit
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy")), n
    assert np.array_equal(a["u0"], a["V"][:, 4:6]) and not a["status"].any() and (a["iters"] >= 1).all()
    # the same instances through the host API (cold start V = 0, the library's AUTO choices as the bench)
    path = mmpc_mod.write_model_json(str(tmp_path / "m.json"), "two_link_arm", 4, 2, 2000, 30, model="two_link_arm")
    s = mmpc_mod.Solver(path, tol_grad=1e-8, tol_defect=1e-10, init_states=mmpc_mod.INIT_ZERO)
    x0, up, tr = oracle.synth(20250213, 0, B, 30, 0.002)
    ref = s.solve_batch_host(x0, up, tr, np.array(WEIGHTS_CFG))
    s.close()
    # same algorithm, same iteration counts: V* within the 1e-10 relative of SURVEY.md A9 (the bound of smoke())
    assert np.array_equal(ref["iters"], a["iters"]) and not ref["status"].any()
    rel = np.abs(a["V"] - ref["V"]).max(1) / np.abs(ref["V"]).max(1)
    print("max rel diff of the dumped V against solve_batch_host:", rel.max())
    assert rel.max() <= 1e-10
