"""GPU: per-instance control limits through the C++ mirror (mahi-mpc_amd/host/examples/instance_limits_example.cpp).

One BatchModelControl with B = 5 and three distinct limit sets, set through update_control_limits(b, ...), against five
ModelControl objects that each have their own update_control_limits, over three synchronous ticks with the warm start
carried along: agreement in u_0* to 1e-7, the tolerance of the closed-loop comparison of tests/test_gpu_batch_control.py
(the batch of 5 and the single controllers may run different kernels: both reach the same KKT point to the stop test's
accuracy).  The all-instances overload afterwards restores shared behaviour: three more ticks against the five
controllers, all given the same box.  ModelControl::calc_u_batch with a row of limits per instance is compared with the
batch controller's first tick (the same cold start, the same kernel choice: bit-level agreement is not asserted, 1e-7
is)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "mahi-mpc_amd", "host")
EXE = os.path.join(HOST, "bin", "instance_limits_example")
MODEL = os.path.join(ROOT, "mahi-mpc_amd", "lib", "user", "nonlinear_double_pendulum")

INF = 10e30
LO = [[-2.0, -1.6], [-INF, -1.0], [-INF, -INF]]
HI = [[1.8, 2.0], [1.0, INF], [INF, INF]]
SET_OF = [0, 1, 2, 1, 0]


def test_batch_controller_with_per_instance_limits_matches_five_controllers():
    assert os.path.exists(EXE) and os.path.exists(MODEL + ".so"), "build() makes the example and the generated model"
    r = subprocess.run([EXE, MODEL], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    ticks = [l.split(",") for l in r.stdout.splitlines() if l.startswith("tick,")]
    assert len(ticks) == 2 * 3 * 5
    on_bound = [0, 0]
    for row in ticks:
        phase, tick, b = int(row[1]), int(row[2]), int(row[3])
        ub, us = np.array(row[4:6], dtype=float), np.array(row[6:8], dtype=float)
        assert int(row[8]) == 0 and int(row[9]) == 0, row
        np.testing.assert_allclose(ub, us, rtol=0, atol=1e-7, err_msg=f"phase {phase} tick {tick} instance {b}")
        lo, hi = (LO[SET_OF[b]], HI[SET_OF[b]]) if phase == 0 else ([-0.5, -0.5], [0.5, 0.5])
        assert (ub >= lo).all() and (ub <= hi).all(), (row, lo, hi)   # inside the instance's own box exactly
        on_bound[phase] += int(((ub == lo) | (ub == hi)).sum())
    # the limits are active in both phases, and instance 2 (no limits) leaves the other instances' boxes in phase 0
    assert on_bound[0] >= 4 and on_bound[1] >= 8, on_bound
    free = np.array([row[4:6] for row in ticks if int(row[1]) == 0 and int(row[3]) == 2], dtype=float)
    assert np.abs(free).max() > 2.0
    cub = [l.split(",") for l in r.stdout.splitlines() if l.startswith("calc_u_batch,")]
    assert len(cub) == 5 and all(int(row[4]) == 0 for row in cub)
    d = [float(v) for v in [l for l in r.stdout.splitlines() if l.startswith("max_diff,")][0].split(",")[1:]]
    print(f"max |u_0* difference|: per-instance limits {d[0]:.2e}, shared again {d[1]:.2e}, calc_u_batch {d[2]:.2e}")
    assert max(d) <= 1e-7, d
