#!/usr/bin/env python3
"""Cost of per-instance control bounds: cfg#2 (2-link arm, N = 30, B = 4096) at +-2 Nm, solved with the box as shared
bounds (bounds_stride 0) and as a [B, nu] array holding the same box in every row (bounds_stride nu).  The iterates are
the same, so the time difference is what the per-instance kernels cost.  Timed as bench.py times its kernels: HIP events
around K back-to-back launches on one stream, after a warm-up; the median of R such blocks is reported.

    python3 tools/instance_bounds_cost.py [--kkt group|riccati|condensed] [--x-bound 1.5] [--launches 20] [--blocks 7]

Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mahi-mpc_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kkt", choices=["auto", "group", "riccati", "condensed"], default="auto")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--u-bound", type=float, default=2.0)
    ap.add_argument("--x-bound", type=float, default=None, help="|qdot| <= this: the interior-point variant")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    import torch

    import mmpc
    B, N, nx, nu = a.batch, a.horizon, 4, 2
    path = mmpc.write_model_json(os.path.join(tempfile.mkdtemp(), "m.json"), "two_link_arm", nx, nu, 2000, N,
                                 model="two_link_arm")
    kkt = {"auto": None, "group": mmpc.KKT_RICCATI_GROUP, "riccati": mmpc.KKT_RICCATI,
           "condensed": mmpc.KKT_CONDENSED}[a.kkt]
    s = mmpc.Solver(path, kkt_solver=kkt, init_states=mmpc.INIT_ZERO)
    if a.x_bound is not None:
        s.set_state_bounds([-np.inf, -np.inf, -a.x_bound, -a.x_bound], [np.inf, np.inf, a.x_bound, a.x_bound])
    s.reserve_workspace(B)
    f = dict(dtype=torch.float64, device="cuda")
    x0, up, tr = torch.empty((B, nx), **f), torch.empty((B, nu), **f), torch.empty((B, N, nx), **f)
    s.synth(20250213, 0, B, x0, up, tr)
    if a.x_bound is not None:   # measured velocities inside the box (x_1 one Euler step from x_0 must be feasible)
        x0[:, 2:].clamp_(-0.99 * a.x_bound, 0.99 * a.x_bound)
    w = torch.tensor([10.0, 1.0, 5.0, 5.0, 5.0, 5.0, 0.01, 0.01], **f)
    lb1, ub1 = torch.full((nu,), -a.u_bound, **f), torch.full((nu,), a.u_bound, **f)
    lbB, ubB = lb1.repeat(B, 1).contiguous(), ub1.repeat(B, 1).contiguous()
    V = torch.zeros((B, s.NV), **f)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    it = torch.zeros_like(st)
    kk = torch.zeros(B, **f)

    def launch(per_instance):
        if per_instance:
            s.solve_batch(B, x0, up, tr, w, V, st, it, kk, u_lb=lbB, u_ub=ubB, bounds_stride=nu)
        else:
            s.solve_batch(B, x0, up, tr, w, V, st, it, kk, u_lb=lb1, u_ub=ub1)

    out = {"config": f"cfg#2 shape: 2-link arm, N = {N}, B = {B}, |u| <= {a.u_bound}"
                     + (f", |qdot| <= {a.x_bound}" if a.x_bound is not None else ""),
           "kkt_solver": s.kkt_solver_for(B), "launches_per_block": a.launches, "blocks": a.blocks}
    res = {}
    for per_instance in (False, True):
        for _ in range(3):
            launch(per_instance)
        torch.cuda.synchronize()
        res[per_instance] = (V.clone(), st.clone(), it.clone())
    out["same_bits"] = all(torch.equal(x, y) for x, y in zip(res[False], res[True]))
    out["converged"] = int((res[True][1] == 0).sum())
    out["mean_iters"] = float(res[True][2].double().mean())
    times = {False: [], True: []}
    for _ in range(a.blocks):   # alternating blocks: drift hits both alike
        for per_instance in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch(per_instance)
            e1.record()
            torch.cuda.synchronize()
            times[per_instance].append(e0.elapsed_time(e1) / a.launches)
    out["shared_ms"] = float(np.median(times[False]))
    out["per_instance_ms"] = float(np.median(times[True]))
    out["shared_ms_runs"] = times[False]
    out["per_instance_ms_runs"] = times[True]
    out["per_instance_over_shared"] = out["per_instance_ms"] / out["shared_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
