#!/usr/bin/env python3
"""Cost of committed controls (mmpc_solve_batch_pinned): cfg#2 shape (2-link arm, N = 30, B = 4096), m = 0 against
m in {1, 2, 5} pinned controls (pins u[b, k, j] = u_prev[b, j] + 0.25 (-1)^j (-1)^k).

A pinned solve is the horizon-(N - m) solve plus a prologue (rollout of the pins, gather of the tail problem) and an
epilogue (scatter).  Per m three timings: the full-horizon solve without pins (m = 0: the path every solve took before
pins existed), the pinned solve, and the same tail problem solved directly on a second handle created with N - m (same
bits, so the same solver time): pinned - tail is what the prologue and epilogue cost.  Timed as
tools/instance_bounds_cost.py times its kernels: HIP events around K back-to-back launches on one stream, after a
warm-up; the median of R alternating blocks.

    python3 tools/pinned_controls_cost.py [--kkt auto|group|riccati|condensed] [--warm] [--launches 20] [--blocks 7]

Default: init_states = ZERO (every launch starts from the same iterate; the prologue then skips the gather of V').
--warm: init_states = AS_GIVEN from a fixed warm start that a device copy restores before every launch, on all three
sides alike (the copy is inside the timed region and cancels in the differences).  Prints one JSON line."""
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
    ap.add_argument("--pins", type=int, nargs="+", default=[1, 2, 5])
    ap.add_argument("--warm", action="store_true")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    import torch

    import mmpc
    B, N, nx, nu = a.batch, a.horizon, 4, 2
    nd = nx + nu
    d = tempfile.mkdtemp()
    kkt = {"auto": None, "group": mmpc.KKT_RICCATI_GROUP, "riccati": mmpc.KKT_RICCATI,
           "condensed": mmpc.KKT_CONDENSED}[a.kkt]
    init = mmpc.INIT_AS_GIVEN if a.warm else mmpc.INIT_ZERO

    def solver(n, kk, hs=None):
        p = mmpc.write_model_json(os.path.join(d, f"m{n}.json"), "two_link_arm", nx, nu, 2000, n, model="two_link_arm")
        s = mmpc.Solver(p, kkt_solver=kk, init_states=init, hessian=hs)
        s.reserve_workspace(B)
        return s

    full = solver(N, kkt)
    # the tail handles run the kernel family the full handle resolves (a pinned solve never changes it)
    family, hess = full.kkt_solver_for(B), full.hessian_for(B)
    f = dict(dtype=torch.float64, device="cuda")
    x0, up, tr = torch.empty((B, nx), **f), torch.empty((B, nu), **f), torch.empty((B, N, nx), **f)
    full.synth(20250213, 0, B, x0, up, tr)
    w = torch.tensor([10.0, 1.0, 5.0, 5.0, 5.0, 5.0, 0.01, 0.01], **f)
    # warm start: the measured state and the previous control held over the horizon
    V0 = torch.cat([torch.cat([x0, up], 1).repeat(1, N), x0], 1).contiguous()
    st = torch.zeros(B, dtype=torch.int32, device="cuda")
    it = torch.zeros_like(st)
    kk = torch.zeros(B, **f)
    torch.cuda.synchronize()

    sides = {}   # name -> (launch, V, iters holder)

    def add(name, s, V, V_start, args, **kw):
        def launch():
            if a.warm:
                V.copy_(V_start)
            s.solve_batch(B, *args, w, V, st, it, kk, **kw)
        sides[name] = (launch, V)

    add("m0", full, torch.zeros((B, full.NV), **f), V0, (x0, up, tr))
    keep = [full]
    for m in a.pins:
        sj = torch.tensor([(-1.0) ** j for j in range(nu)], **f)
        sk = torch.tensor([(-1.0) ** k for k in range(m)], **f)
        pin = (up[:, None, :] + 0.25 * sk[None, :, None] * sj[None, None, :]).contiguous()
        Vp = torch.zeros((B, full.NV), **f)
        add(f"pinned_m{m}", full, Vp, V0, (x0, up, tr), u_pin=pin, n_pin=m)
        sides[f"pinned_m{m}"][0]()
        torch.cuda.synchronize()
        tail = solver(N - m, family, hess)
        keep.append(tail)
        xm = Vp[:, m * nd:m * nd + nx].contiguous()
        add(f"tail_m{m}", tail, torch.zeros((B, tail.NV), **f), V0[:, m * nd:].contiguous(),
            (xm, pin[:, m - 1].contiguous(), tr[:, m:].contiguous()))

    out = {"config": f"cfg#2 shape: 2-link arm, N = {N}, B = {B}", "kkt_solver": family, "hessian": hess,
           "init_states": "as_given (restored per launch)" if a.warm else "zero",
           "launches_per_block": a.launches, "blocks": a.blocks, "pins": a.pins}
    for name, (launch, V) in sides.items():
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        out[name + "_converged"] = int((st == 0).sum())
        out[name + "_mean_iters"] = float(it.double().mean())
        sides[name] = (launch, V.clone())
    for m in a.pins:   # the reduction: the pinned solve's tail is the tail handle's solve, bit for bit
        out[f"same_bits_m{m}"] = bool(torch.equal(sides[f"pinned_m{m}"][1][:, m * nd:], sides[f"tail_m{m}"][1]))
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
    for m in a.pins:
        out[f"prologue_epilogue_ms_m{m}"] = out[f"pinned_m{m}_ms"] - out[f"tail_m{m}_ms"]
        out[f"pinned_over_m0_m{m}"] = out[f"pinned_m{m}_ms"] / out["m0_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
