"""GPU: committed controls through the C++ mirror (mahi-mpc_amd/host/examples/committed_controls_example.cpp).

ModelControl, built-in 2-link arm with N = 17, set_num_control_inputs_saved(2), six ticks at t_j = j * step: from tick 1
on the first two controls of the published plan are the previous plan's controls 1 and 2, bit for bit (the index rule
clamp(round((t - t_prev) / step) + i, 0, N - 1) with one step elapsed), every solve converges, and an object with m = 0
publishes bit for bit what an object that never called the setter publishes.

BatchModelControl with B = 5 and synchronous calc_u, m = 2, against five ModelControl objects with m = 2: the first
three controls of every plan agree to 1e-7, the tolerance of tests/test_gpu_instance_limits_control.py (the batch of 5
and the single controllers may run different kernels: both reach the same KKT point to the stop test's accuracy), and
the batch's pinned controls are its own previous plan's, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "mahi-mpc_amd", "host", "bin", "committed_controls_example")
N, M, TICKS, B, NU = 17, 2, 6, 5, 2


def test_committed_controls_example(mmpc_mod, tmp_path):
    assert os.path.exists(EXE), "build() makes the example"
    model = str(tmp_path / "arm17")
    mmpc_mod.write_model_json(model + ".json", "arm17", 4, NU, 2000, N, model="two_link_arm")
    r = subprocess.run([EXE, model, str(M), str(TICKS)], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split(",") for l in r.stdout.splitlines()]
    # ---- ModelControl ----
    mc = [l for l in lines if l[0] == "mc"]
    assert len(mc) == TICKS
    plans = []
    for j, row in enumerate(mc):
        assert int(row[1]) == j and int(row[2]) == 0, row   # last_status() == 0 at every tick
        plans.append(np.array(row[3:], dtype=float).reshape(M + 1, NU))
    for j in range(1, TICKS):
        np.testing.assert_array_equal(plans[j][:M], plans[j - 1][1:M + 1], err_msg=f"tick {j}")
    assert not np.array_equal(plans[1][M], plans[0][M])   # the free controls do move
    m0 = [l for l in lines if l[0] == "m0"]
    assert len(m0) == TICKS and all(int(row[2]) == 1 for row in m0), m0
    # ---- BatchModelControl against five ModelControl objects ----
    bc = [l for l in lines if l[0] == "bc"]
    assert len(bc) == TICKS * B
    prev = {}
    for row in bc:
        tick, b = int(row[1]), int(row[2])
        assert int(row[3]) == 0 and int(row[4]) == 0, row
        v = np.array(row[5:], dtype=float).reshape(2, M + 1, NU)
        np.testing.assert_allclose(v[0], v[1], rtol=0, atol=1e-7, err_msg=f"tick {tick} instance {b}")
        if tick > 0:
            np.testing.assert_array_equal(v[0][:M], prev[b][1:M + 1], err_msg=f"tick {tick} instance {b}")
        prev[b] = v[0]
    d = float([l for l in lines if l[0] == "max_diff"][0][1])
    print(f"max |control difference| batch vs single controllers: {d:.2e}")
    assert d <= 1e-7, d
