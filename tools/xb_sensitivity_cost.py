#!/usr/bin/env python3
"""Cost of the feedback gains and the solve VJP under the sensitivity barrier of a state-bounded handle
(mmpc_set_sensitivity_barrier): the XB instantiations beside the unbounded ones on the same batch.

Two handles of one model file: one with |qdot| <= --qdot-max on every velocity state and the barrier at its defaults,
one without state bounds.  The plan V* is the state-bounded handle's own interior-point solve (init_states = ZERO);
both handles then run the gain launch (lane kernel and, where it is available, the 16-lane kernel) and the VJP (full
and backward-only) at that V* with a standard normal V_bar -- the unbounded kernels on a V they did not produce, which
costs them the same arithmetic.  Timed with the protocol of tools/solve_vjp_cost.py: HIP events around K back-to-back
launches on one stream after a warm-up, the median of R alternating blocks.

    python3 tools/xb_sensitivity_cost.py [--model two_link_arm|exo_arm] [--batch 4096] [--horizon 30]
                                         [--qdot-max 1.5] [--launches 20] [--blocks 7]

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
    ap.add_argument("--qdot-max", type=float, default=1.5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    import torch

    import mmpc
    B, N = a.batch, a.horizon
    nx, nu = (8, 4) if a.model == "exo_arm" else (4, 2)
    K = nx + nu
    d = tempfile.mkdtemp()
    p = mmpc.write_model_json(os.path.join(d, "m.json"), a.model, nx, nu, 2000, N, model=a.model)
    xb = mmpc.Solver(p, init_states=mmpc.INIT_ZERO, max_iter=100, sensitivity_barrier=True)
    lim = np.concatenate([np.full(nx // 2, np.inf), np.full(nx // 2, a.qdot_max)])
    xb.set_state_bounds(-lim, lim)
    free = mmpc.Solver(p)
    xb.reserve_workspace(B)
    f = dict(dtype=torch.float64, device="cuda")
    x0, up, tr = torch.empty((B, nx), **f), torch.empty((B, nu), **f), torch.empty((B, N, nx), **f)
    xb.synth(20250213, 0, B, x0, up, tr)
    x0[:, nx // 2:].clamp_(-0.99 * a.qdot_max, 0.99 * a.qdot_max)   # x_1 is one Euler step from x_0
    wv = [10.0, 1.0, 5.0, 5.0, 5.0, 5.0, 0.01, 0.01] if nx == 4 else [10.0] * 4 + [1.0] * 4 + [1.0] * 4 + [0.01] * 4
    w = torch.tensor(wv, **f)
    V = torch.zeros((B, xb.NV), **f)
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    it = torch.zeros_like(st)
    xb.solve_batch(B, x0, up, tr, w, V, st, it, torch.zeros(B, **f))
    torch.cuda.synchronize()
    X = torch.stack([V[:, k * K + nx // 2:k * K + nx] for k in range(1, N + 1)], 1)
    G = torch.zeros((B, N, nu, K), **f)
    gst = torch.zeros(B, dtype=torch.int32, device="cuda")
    Vbar = torch.randn((B, xb.NV), generator=torch.Generator(device="cuda").manual_seed(20250213), **f)
    ws_bytes = xb.solve_vjp_workspace_bytes(B)
    outs = dict(x0_bar=torch.zeros((B, nx), **f), u_prev_bar=torch.zeros((B, nu), **f),
                traj_bar=torch.zeros((B, N, nx), **f), weights_bar=torch.zeros((B, nx + 2 * nu), **f),
                adj_V=torch.zeros((B, xb.NV), **f), workspace=torch.zeros(ws_bytes // 8, **f))
    vst = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = {"config": f"{a.model}, N = {N}, B = {B}, |qdot| <= {a.qdot_max}", "sensitivity_barrier": xb.sensitivity_barrier,
           "solve_converged": int((st == 0).sum()), "solve_mean_iters": float(it.double().mean()),
           "slacks_below_1e-6": int(((a.qdot_max - X.abs()) < 1e-6).sum()), "workspace_bytes": ws_bytes,
           "launches_per_block": a.launches, "blocks": a.blocks}

    sides = {}
    for tag, s in (("xb", xb), ("unbounded", free)):
        kernels = [("lane", mmpc.GAIN_KERNEL_LANE)]
        try:   # the 16-lane kernel where the model and the horizon admit it (the XB record is larger)
            s.feedback_gains(B, V, up, tr, w, G=G, gain_status=gst, kernel=mmpc.GAIN_KERNEL_GROUP)
            kernels.append(("group", mmpc.GAIN_KERNEL_GROUP))
        except mmpc.MmpcError as e:
            out[f"{tag}_gains_group"] = f"unavailable: {e}"
        for name, kid in kernels:
            sides[f"{tag}_gains_{name}"] = (lambda s=s, kid=kid: s.feedback_gains(B, V, up, tr, w, G=G, gain_status=gst,
                                                                                 kernel=kid), gst)
        sides[f"{tag}_vjp_full"] = (lambda s=s: s.solve_vjp(B, V, up, tr, w, Vbar, vjp_status=vst, **outs), vst)
        sides[f"{tag}_vjp_backward"] = (lambda s=s: s.solve_vjp(B, V, up, tr, w, Vbar, x0_bar=outs["x0_bar"],
                                                                u_prev_bar=outs["u_prev_bar"], vjp_status=vst,
                                                                backward_only=True), vst)
    for name, (launch, status) in sides.items():
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        out[name + "_status_counts"] = [int((status == v).sum()) for v in (0, 1, 2)]
    times = {name: [] for name in sides}
    for _ in range(a.blocks):   # alternating blocks: drift hits all sides alike
        for name, (launch, _) in sides.items():
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
    for name in sides:
        if name.startswith("xb_") and "unbounded_" + name[3:] in sides:
            out[name + "_over_unbounded"] = out[name + "_ms"] / out["unbounded_" + name[3:] + "_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
