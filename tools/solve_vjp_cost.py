#!/usr/bin/env python3
"""Cost of the solve's reverse-mode product (mmpc_solve_vjp_batch) beside the gain sweep and the solve of one batch.

A VJP is one backward Riccati sweep with a vector part plus one forward sweep at the solution, so it is measured beside
(a) the feedback-gain launch on the lane kernel (the same backward sweep without the vector part, storing G instead of
the record) and (b) one SQP iteration of the solve: the solve's time divided by its mean iteration count in the same
run.  Per line four timings: the solve (init_states = ZERO, every launch from the same iterate; the handle's own AUTO
solver and Hessian), the gain launch, the full VJP (all five outputs, the record workspace) and the backward-only VJP
(x0_bar and u_prev_bar, no workspace), all at the solve's V* with a standard normal V_bar.  Timed as
tools/feedback_gains_cost.py times its kernels: HIP events around K back-to-back launches on one stream after a warm-up;
the median of R alternating blocks.

    python3 tools/solve_vjp_cost.py [--model two_link_arm|exo_arm] [--batch 4096] [--horizon 30] [--hessian exact|gn]
                                    [--launches 20] [--blocks 7]

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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    import torch

    import mmpc
    B, N = a.batch, a.horizon
    nx, nu = (8, 4) if a.model == "exo_arm" else (4, 2)
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
    G = torch.zeros((B, N, nu, nx + nu), **f)
    gst = torch.zeros(B, dtype=torch.int32, device="cuda")
    Vbar = torch.randn((B, s.NV), generator=torch.Generator(device="cuda").manual_seed(20250213), **f)
    ws_bytes = s.solve_vjp_workspace_bytes(B)
    outs = dict(x0_bar=torch.zeros((B, nx), **f), u_prev_bar=torch.zeros((B, nu), **f),
                traj_bar=torch.zeros((B, N, nx), **f), weights_bar=torch.zeros((B, nx + 2 * nu), **f),
                adj_V=torch.zeros((B, s.NV), **f), workspace=torch.zeros(ws_bytes // 8, **f))
    vst = torch.zeros(B, dtype=torch.int32, device="cuda")
    hess = mmpc.HESSIAN_EXACT if a.hessian == "exact" else mmpc.HESSIAN_GAUSS_NEWTON

    def solve():
        s.solve_batch(B, x0, up, tr, w, V, st, it, kk)

    def gains():
        s.feedback_gains(B, V, up, tr, w, G=G, gain_status=gst, hessian=hess, kernel=mmpc.GAIN_KERNEL_LANE)

    def vjp_full():
        s.solve_vjp(B, V, up, tr, w, Vbar, vjp_status=vst, hessian=hess, **outs)

    def vjp_backward():
        s.solve_vjp(B, V, up, tr, w, Vbar, x0_bar=outs["x0_bar"], u_prev_bar=outs["u_prev_bar"], vjp_status=vst,
                    hessian=hess, backward_only=True)

    sides = {"solve": solve, "gains_lane": gains, "vjp_full": vjp_full, "vjp_backward": vjp_backward}
    out = {"config": f"{a.model}, N = {N}, B = {B}", "kkt_solver": s.kkt_solver_for(B),
           "solve_hessian": s.hessian_for(B), "vjp_hessian": a.hessian, "workspace_bytes": ws_bytes,
           "launches_per_block": a.launches, "blocks": a.blocks}
    for name, launch in sides.items():
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        if name == "solve":
            out["solve_converged"] = int((st == 0).sum())
            out["solve_mean_iters"] = float(it.double().mean())
        else:
            status = gst if name == "gains_lane" else vst
            out[name + "_status_counts"] = [int((status == v).sum()) for v in (0, 1, 2)]
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
    out["iteration_ms"] = out["solve_ms"] / out["solve_mean_iters"]   # one SQP iteration of this solve
    for name in ("vjp_full", "vjp_backward"):
        out[name + "_over_gains_lane"] = out[name + "_ms"] / out["gains_lane_ms"]
        out[name + "_over_iteration"] = out[name + "_ms"] / out["iteration_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
