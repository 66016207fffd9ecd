#!/usr/bin/env python3
"""Cost of the solve's forward-mode product (mmpc_solve_jvp_batch) beside the VJP and the gain sweep of one batch.

A JVP runs the VJP's two sweeps with the same record and another right-hand side, so the expectation it is measured
against is the VJP's time in the same run.  Per line five timings at the solve's V*: the full JVP (dV and du0, the
record workspace), the forward-free JVP (du0 alone, no workspace), the full VJP (all five outputs), the backward-only
VJP and the feedback-gain launch on the lane kernel; standard normal tangents in all four inputs and a standard normal
V_bar.  The protocol is tools/solve_vjp_cost.py's: HIP events around K back-to-back launches on one stream after a
warm-up; the median of R alternating blocks.

    python3 tools/solve_jvp_cost.py [--model two_link_arm|exo_arm] [--batch 4096] [--horizon 30] [--hessian exact|gn]
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
    s.solve_batch(B, x0, up, tr, w, V, st, it, torch.zeros(B, **f))
    torch.cuda.synchronize()
    gen = torch.Generator(device="cuda").manual_seed(20250213)
    rnd = lambda *shape: torch.randn(shape, generator=gen, **f)  # noqa: E731
    G = torch.zeros((B, N, nu, nx + nu), **f)
    Vbar = rnd(B, s.NV)
    tang = dict(dx0=rnd(B, nx), du_prev=rnd(B, nu), dtraj=rnd(B, N, nx), dweights=rnd(B, nx + 2 * nu))
    ws_bytes = s.solve_jvp_workspace_bytes(B)
    ws = torch.zeros(ws_bytes // 8, **f)
    vouts = dict(x0_bar=torch.zeros((B, nx), **f), u_prev_bar=torch.zeros((B, nu), **f),
                 traj_bar=torch.zeros((B, N, nx), **f), weights_bar=torch.zeros((B, nx + 2 * nu), **f),
                 adj_V=torch.zeros((B, s.NV), **f), workspace=ws)
    dV, du0 = torch.zeros((B, s.NV), **f), torch.zeros((B, nu), **f)
    status = {k: torch.zeros(B, dtype=torch.int32, device="cuda")
              for k in ("jvp_full", "jvp_forward_free", "vjp_full", "vjp_backward", "gains_lane")}
    hess = mmpc.HESSIAN_EXACT if a.hessian == "exact" else mmpc.HESSIAN_GAUSS_NEWTON

    def jvp_full():
        s.solve_jvp(B, V, up, tr, w, dV=dV, du0=du0, jvp_status=status["jvp_full"], workspace=ws, hessian=hess, **tang)

    def jvp_forward_free():
        s.solve_jvp(B, V, up, tr, w, du0=du0, jvp_status=status["jvp_forward_free"], hessian=hess, forward_free=True,
                    **tang)

    def vjp_full():
        s.solve_vjp(B, V, up, tr, w, Vbar, vjp_status=status["vjp_full"], hessian=hess, **vouts)

    def vjp_backward():
        s.solve_vjp(B, V, up, tr, w, Vbar, x0_bar=vouts["x0_bar"], u_prev_bar=vouts["u_prev_bar"],
                    vjp_status=status["vjp_backward"], hessian=hess, backward_only=True)

    def gains():
        s.feedback_gains(B, V, up, tr, w, G=G, gain_status=status["gains_lane"], hessian=hess,
                         kernel=mmpc.GAIN_KERNEL_LANE)

    sides = {"jvp_full": jvp_full, "vjp_full": vjp_full, "jvp_forward_free": jvp_forward_free,
             "vjp_backward": vjp_backward, "gains_lane": gains}
    out = {"config": f"{a.model}, N = {N}, B = {B}", "solve_converged": int((st == 0).sum()),
           "solve_mean_iters": float(it.double().mean()), "hessian": a.hessian, "workspace_bytes": ws_bytes,
           "launches_per_block": a.launches, "blocks": a.blocks}
    for name, launch in sides.items():
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        out[name + "_status_counts"] = [int((status[name] == v).sum()) for v in (0, 1, 2)]
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
    out["jvp_full_over_vjp_full"] = out["jvp_full_ms"] / out["vjp_full_ms"]
    out["jvp_forward_free_over_vjp_backward"] = out["jvp_forward_free_ms"] / out["vjp_backward_ms"]
    out["jvp_forward_free_over_gains_lane"] = out["jvp_forward_free_ms"] / out["gains_lane_ms"]
    out["vjp_full_spread"] = (max(times["vjp_full"]) - min(times["vjp_full"])) / out["vjp_full_ms"]
    out["vjp_backward_spread"] = (max(times["vjp_backward"]) - min(times["vjp_backward"])) / out["vjp_backward_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
