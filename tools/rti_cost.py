#!/usr/bin/env python3
"""Cost of a real-time iteration tick (mmpc_rti_prepare_batch, mmpc_rti_feedback_batch) beside the solve JVP and one
solve of the same batch.

The quantity of interest is the feedback launch -- what runs between the measurement and the actuation -- against the
forward-free JVP (what a controller had before for that moment) and against a full solve.  Per line five timings at
the solve's V* shifted by one stage in time (the plan a tick linearises at; x0_meas = x^_0 + 1e-2 standard normal): the
preparation, the feedback, the full JVP, the forward-free JVP (tangent dx0) and one mmpc_solve_batch of the batch from
the zero start (the solve the benchmark times).  The feedback launch overwrites its plan, so the plan is restored
before every block, outside the timed region; its time does not depend on the data.  The protocol is
tools/solve_jvp_cost.py's: HIP events around K back-to-back launches on one stream after a warm-up; the median of R
alternating blocks, max - min beside it.

    python3 tools/rti_cost.py [--model two_link_arm|exo_arm] [--batch 4096] [--horizon 30] [--hessian exact|gn]
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
    K = nx + nu
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
    conv, iters = int((st == 0).sum()), float(it.double().mean())
    # the plan shifted by one stage: the last control repeated, x_N = F(x_N, u_{N-1}); u_prev the old u_0
    xd = torch.zeros((B, nx), **f)
    xN, uL = V[:, N * K:].contiguous(), V[:, (N - 1) * K + nx:N * K].contiguous()
    s.linearize(B, xN, uL, None, None, xd)
    Vh = torch.cat([V[:, K:], uL, xN + s.h * xd], dim=1).contiguous()
    uph = V[:, nx:K].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(20250213)
    dx0 = 1e-2 * torch.randn((B, nx), generator=gen, **f)
    xm = Vh[:, :nx] + dx0
    ws_bytes = s.rti_workspace_bytes(B)
    ws = torch.zeros(ws_bytes // 8, **f)
    jws = torch.zeros(s.solve_jvp_workspace_bytes(B) // 8, **f)
    Vt, Vs = Vh.clone(), Vh.clone()
    u0, si = torch.zeros((B, nu), **f), torch.zeros(B, **f)
    dV, du0 = torch.zeros((B, s.NV), **f), torch.zeros((B, nu), **f)
    status = {k: torch.zeros(B, dtype=torch.int32, device="cuda")
              for k in ("prepare", "feedback", "jvp_full", "jvp_forward_free", "solve")}
    hess = mmpc.HESSIAN_EXACT if a.hessian == "exact" else mmpc.HESSIAN_GAUSS_NEWTON

    def prepare():
        s.rti_prepare(B, Vh, uph, tr, w, workspace=ws, prep_status=status["prepare"], hessian=hess)

    def feedback():
        s.rti_feedback(B, xm, Vt, ws, u0=u0, step_inf=si, status=status["feedback"])

    def jvp_full():
        s.solve_jvp(B, Vh, uph, tr, w, dx0=dx0, dV=dV, du0=du0, jvp_status=status["jvp_full"], workspace=jws,
                    hessian=hess)

    def jvp_forward_free():
        s.solve_jvp(B, Vh, uph, tr, w, dx0=dx0, du0=du0, jvp_status=status["jvp_forward_free"], hessian=hess,
                    forward_free=True)

    def solve():
        s.solve_batch(B, x0, up, tr, w, Vs, status["solve"], it, kkt)

    def restore():
        Vt.copy_(Vh)
        Vs.copy_(Vh)

    sides = {"prepare": prepare, "feedback": feedback, "jvp_full": jvp_full, "jvp_forward_free": jvp_forward_free,
             "solve": solve}
    out = {"config": f"{a.model}, N = {N}, B = {B}", "solve_converged": conv, "solve_mean_iters": iters,
           "hessian": a.hessian, "workspace_bytes": ws_bytes,
           "feedback_record_bytes_read": B * N * K * (K + 1) * 8, "launches_per_block": a.launches, "blocks": a.blocks}
    prepare()
    for name, launch in sides.items():
        for _ in range(3):
            restore()
            launch()
        torch.cuda.synchronize()
        out[name + "_status_counts"] = [int((status[name] == v).sum()) for v in (0, 1, 2)]
    times = {name: [] for name in sides}
    for _ in range(a.blocks):   # alternating blocks: drift hits all sides alike
        for name, launch in sides.items():
            restore()
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
    out["feedback_over_jvp_forward_free"] = out["feedback_ms"] / out["jvp_forward_free_ms"]
    out["feedback_over_solve"] = out["feedback_ms"] / out["solve_ms"]
    out["prepare_over_jvp_forward_free"] = out["prepare_ms"] / out["jvp_forward_free_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
