"""GPU: feedback along the plan through the C++ mirror (mahi-mpc_amd/host/examples/feedback_control_example.cpp).

ModelControl, built-in 2-link arm with N = 17, set_feedback_stages(3):
* control_at_time with x_measured = x_est_i returns the plan's stage i bit for bit, for the stages with gains and for the
  first one without (i = 3).  The example asks at t_i + step / 2: the reference's index rule (ModelControl.cpp:192-197)
  returns the last stage whose time is BEFORE the argument, so t_i itself would select stage i - 1;
* with x_measured = x_est_0 + 1e-3 (1, -1, 1, -1) the returned control equals u_0 + G_0[:, :nx] delta recomputed here
  from feedback_gain(0), to 1e-15;
* its distance to a re-solve from the moved state is at most 1 / 100 of the plan's distance (on the CPU the worst
  ratio was 1 / 450 over 13 instances at N = 17 and 30; the margin covers the GPU solve's own 1e-8 stop tolerance).
  The example's controller is in its tracking regime (the arm on its reference up to a tracking error of
  (0.05, -0.03, 0.2, -0.1)): the CPU oracle and the dense reference give 1 / 885 there.  The correction is first
  order: far from the reference the remainder grows (1 / 43 from the rest state the other examples start from, on
  the CPU and on the GPU alike, falling as delta^2).
An object that never enabled feedback publishes, tick after tick, bit for bit what an object with feedback publishes
(plan, status, iteration count: the solve path does not see the gains), and its control_at_time(t, x_measured) is its
plan.
BatchModelControl with B = 5 and synchronous calc_u against five ModelControl objects, all with three stages: gains and
corrected controls to 1e-7, the tolerance of the other batch-versus-single tests."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "mahi-mpc_amd", "host", "bin", "feedback_control_example")
N, NFB, TICKS, B, NX, NU = 17, 3, 2, 5, 4, 2
K = NX + NU
DELTA = 1e-3 * np.array([1.0, -1.0, 1.0, -1.0])


def test_feedback_control_example(mmpc_mod, tmp_path):
    assert os.path.exists(EXE), "build() makes the example"
    model = str(tmp_path / "arm17")
    mmpc_mod.write_model_json(model + ".json", "arm17", NX, NU, 2000, N, model="two_link_arm")
    r = subprocess.run([EXE, model, str(NFB), str(TICKS)], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split(",") for l in r.stdout.splitlines()]
    rows = lambda tag: [l for l in lines if l[0] == tag]   # noqa: E731
    vec = lambda tag: np.array(rows(tag)[0][1:], dtype=float)   # noqa: E731
    # ---- ModelControl ----
    plan = rows("plan")
    assert [int(p[1]) for p in plan] == list(range(NFB + 1)) and all(int(p[2]) == 1 for p in plan), plan
    assert [int(v) for v in rows("status")[0][1:]] == [0, 0]
    G0, u0, fb = vec("g0").reshape(NU, K), vec("u0"), vec("fb")
    assert np.abs(G0[:, :NX]).max() > 0.1   # the gains are there
    x0 = vec("x0")
    dx = (x0 + DELTA) - x0   # the measured state the example passes, minus x_est_0
    want = u0.copy()
    for j in range(NX):      # the mirror's own order of summation
        want += G0[:, j] * dx[j]
    err = np.abs(fb - want).max()
    print(f"control_at_time against u_0 + G_0 delta: {err:.2e}")
    assert err <= 1e-15
    re = rows("resolve")[0]
    assert int(re[1]) == 0
    u_re = np.array(re[2:], dtype=float)
    d_fb, d_plan = np.abs(fb - u_re).max(), np.abs(u0 - u_re).max()
    print(f"distance to the re-solve: corrected {d_fb:.3e}, plan {d_plan:.3e}, ratio 1 / {d_plan / d_fb:.0f}")
    assert d_fb <= d_plan / 100
    # ---- feedback off ----
    same = rows("same")
    assert len(same) == TICKS and all(int(s[2]) == 1 for s in same), same
    assert int(rows("nofb")[0][1]) == 1
    # ---- BatchModelControl against five ModelControl objects ----
    bg = rows("bg")
    assert len(bg) == B * NFB
    worst = 0.0
    for row in bg:
        assert int(row[3]) == 0 and int(row[4]) == 0, row[:5]
        g = np.array(row[5:], dtype=float).reshape(2, NU, K)
        worst = max(worst, np.abs(g[0] - g[1]).max())
    bu = rows("bu")
    assert len(bu) == B
    worst_u = max(np.abs(np.diff(np.array(row[2:], dtype=float).reshape(2, NU), axis=0)).max() for row in bu)
    print(f"batch against single controllers: gains {worst:.2e}, corrected controls {worst_u:.2e}")
    assert worst <= 1e-7 and worst_u <= 1e-7
