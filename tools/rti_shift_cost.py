#!/usr/bin/env python3
"""Cost of the shift between two ticks (mmpc_rti_shift_batch) beside the feedback launch of the same batch.

The plan is the solve's V* from the zero start; the shift reads it and writes a second buffer, so nothing needs
restoring between launches.  The feedback launch (on a preparation at the shifted plan) is timed in the same alternating
blocks as the yardstick tools/rti_cost.py reports.  The protocol is that tool's: HIP events around K back-to-back
launches on one stream after a warm-up; the median of R alternating blocks, max - min beside it.

    python3 tools/rti_shift_cost.py [--model two_link_arm|exo_arm] [--batch 4096] [--horizon 30] [--n-shift 1]
                                    [--launches 20] [--blocks 7]

Prints one JSON line; bytes_moved is what the copy part reads plus what it writes."""
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
    ap.add_argument("--n-shift", type=int, default=1)
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
    kkt = torch.zeros(B, **f)
    s.solve_batch(B, x0, up, tr, w, V, st, it, kkt)
    torch.cuda.synchronize()
    Vh, uph = torch.zeros((B, s.NV), **f), torch.zeros((B, nu), **f)
    s.rti_shift(B, V, 1, V_out=Vh, u_prev_out=uph)
    Vo, upo = torch.zeros((B, s.NV), **f), torch.zeros((B, nu), **f)
    ws = torch.zeros(s.rti_workspace_bytes(B) // 8, **f)
    s.rti_prepare(B, Vh, uph, tr, w, workspace=ws)
    xm = Vh[:, :nx] + 1e-2 * torch.randn((B, nx), generator=torch.Generator(device="cuda").manual_seed(20250213), **f)
    Vt = Vh.clone()
    u0, si = torch.zeros((B, nu), **f), torch.zeros(B, **f)
    fst = torch.zeros(B, dtype=torch.int32, device="cuda")

    def shift():
        s.rti_shift(B, V, a.n_shift, V_out=Vo, u_prev_out=upo)

    def feedback():
        s.rti_feedback(B, xm, Vt, ws, u0=u0, step_inf=si, status=fst)

    sides = {"shift": shift, "feedback": feedback}
    out = {"config": f"{a.model}, N = {N}, B = {B}", "n_shift": a.n_shift, "solve_converged": int((st == 0).sum()),
           "bytes_moved": 2 * B * s.NV * 8, "launches_per_block": a.launches, "blocks": a.blocks}
    for launch in sides.values():
        for _ in range(3):
            Vt.copy_(Vh)
            launch()
    torch.cuda.synchronize()
    out["shifted_plan_finite"] = bool(torch.isfinite(Vo).all())
    times = {name: [] for name in sides}
    for _ in range(a.blocks):   # alternating blocks: drift hits both sides alike
        for name, launch in sides.items():
            Vt.copy_(Vh)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches)
    for name in sides:
        out[name + "_ms"] = float(np.median(times[name]))
        out[name + "_ms_max_minus_min"] = max(times[name]) - min(times[name])
        out[name + "_ms_runs"] = times[name]
    out["shift_GBps"] = out["bytes_moved"] / (out["shift_ms"] * 1e-3) / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
