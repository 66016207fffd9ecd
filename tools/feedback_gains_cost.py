#!/usr/bin/env python3
"""Cost of the feedback gains (mmpc_feedback_gains_batch) beside the unchanged solve of the same batch.

A gain sweep is one model-and-Hessian pass plus one Riccati sweep, with no step sweep and no line search, so its budget
is one SQP iteration of the solve: the solve's time divided by its mean iteration count, measured in the same run.
Per line three or four timings: the solve (init_states = ZERO, every launch from the same iterate; the handle's own
AUTO solver and Hessian) and the gain launch at the solve's V* on the lane kernel, the 16-lane kernel (where it is
available) and whatever AUTO picks.  Timed as tools/pinned_controls_cost.py times its kernels: HIP events around K
back-to-back launches on one stream after a warm-up; the median of R alternating blocks.

    python3 tools/feedback_gains_cost.py [--model two_link_arm|exo_arm] [--batch 4096] [--horizon 30]
                                         [--hessian exact|gn] [--n-gain N] [--launches 20] [--blocks 7]

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
    ap.add_argument("--model", choices=["two_link_arm", "exo_arm"], default="two_link_arm")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--hessian", choices=["exact", "gn"], default="exact")
    ap.add_argument("--n-gain", type=int, default=0, help="stages written (0: all N)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    import torch

    import mmpc
    B, N = a.batch, a.horizon
    nx, nu = (8, 4) if a.model == "exo_arm" else (4, 2)
    n_gain = a.n_gain or N
    d = tempfile.mkdtemp()
    p = mmpc.write_model_json(os.path.join(d, "m.json"), a.model, nx, nu, 2000, N, model=a.model)
    s = mmpc.Solver(p, init_states=mmpc.INIT_ZERO)
    s.reserve_workspace(B)
    f = dict(dtype=torch.float64, device="cuda")
    x0, up, tr = torch.empty((B, nx), **f), torch.empty((B, nu), **f), torch.empty((B, N, nx), **f)
    s.synth(20250213, 0, B, x0, up, tr)
    wv = [10.0, 1.0, 5.0, 5.0, 5.0, 5.0, 0.01, 0.01] if nx == 4 else [10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4
    w = torch.tensor(wv, **f)
    V = torch.zeros((B, s.NV), **f)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    it = torch.zeros_like(st)
    kk = torch.zeros(B, **f)
    G = torch.zeros((B, n_gain, nu, nx + nu), **f)
    gst = torch.zeros(B, dtype=torch.int32, device="cuda")
    hess = mmpc.HESSIAN_EXACT if a.hessian == "exact" else mmpc.HESSIAN_GAUSS_NEWTON

    def solve():
        s.solve_batch(B, x0, up, tr, w, V, st, it, kk)

    def gains(kernel):
        return lambda: s.feedback_gains(B, V, up, tr, w, G=G, gain_status=gst, n_gain=n_gain, hessian=hess,
                                        kernel=kernel)

    sides = {"solve": solve, "gains_lane": gains(mmpc.GAIN_KERNEL_LANE)}
    try:   # the 16-lane kernel where it is available (nx + nu < 16 and an instance's records within the LDS)
        gains(mmpc.GAIN_KERNEL_GROUP)()
        sides["gains_group"] = gains(mmpc.GAIN_KERNEL_GROUP)
    except mmpc.MmpcError as e:
        if e.code != -4:
            raise
    sides["gains_auto"] = gains(mmpc.GAIN_KERNEL_AUTO)
    out = {"config": f"{a.model}, N = {N}, B = {B}", "kkt_solver": s.kkt_solver_for(B), "solve_hessian": s.hessian_for(B),
           "gain_hessian": a.hessian, "n_gain": n_gain, "launches_per_block": a.launches, "blocks": a.blocks}
    for name, launch in sides.items():
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        if name == "solve":
            out["solve_converged"] = int((st == 0).sum())
            out["solve_mean_iters"] = float(it.double().mean())
        else:
            out[name + "_status_counts"] = [int((gst == v).sum()) for v in (0, 1, 2)]
    times = {name: [] for name in sides}
    for _ in range(a.blocks):   # alternating blocks: drift hits all sides alike
        for name, launch in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches)
    for name in sides:
        out[name + "_ms"] = float(np.median(times[name]))
        out[name + "_ms_runs"] = times[name]
    out["budget_ms"] = out["solve_ms"] / out["solve_mean_iters"]   # one SQP iteration of this solve
    for name in sides:
        if name != "solve":
            out[name + "_over_budget"] = out[name + "_ms"] / out["budget_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
