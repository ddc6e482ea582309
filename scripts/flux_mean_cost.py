#!/usr/bin/env python3
"""flux_mean_cost.py — what the flux means (picles_flux_mean_*) cost per step on one GPU, at the BASELINE box (4096², winds (10,10), DP5).

Legs, alternated over --rounds rounds on ONE context (re-seeded before every leg, clocks conditioned once as bench.py does):

    none       no set                                        (the run the others are compared with)
    mean44     a mean set at coarsening (4, 4), every = 1     K steps in one picles_run_steps call: the steps stay fused
    mean11     a mean set at coarsening (1, 1), every = 1
    export44   the route without a mean set, at (4, 4): picles_time_step + picles_flux_export after every step, summed in torch
    export11   the same at (1, 1)

The run_steps legs are timed inside ONE event pair (picles_enable_timing(ctx, 2)): ms per step = region / K.  The export legs leave
the fused path (every export completes the pending step), so they are timed with torch events around the whole loop: the same K
steps, the torch additions included — that sum is what the route delivers.  The `none` leg is timed both ways.

    python scripts/flux_mean_cost.py [--grid-n 4096] [--steps 40] [--warmup 5] [--rounds 3] [--legs ...] [--out FILE]

Prints one JSON line per leg and round, then the memory of the set at both coarsenings and a summary line; --out appends them to a
file.  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python scripts/flux_mean_cost.py --legs mean44
--rounds 1` in a run of its own: k_flux_mean_update stands beside k_stat<true> (the same pull; scripts/stat_cost.py) and k_flux (the
same arithmetic; the export legs).
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

LEGS = {"none": None, "mean44": ("mean", (4, 4)), "mean11": ("mean", (1, 1)), "export44": ("export", (4, 4)), "export11": ("export", (1, 1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid-n", dest="n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="none,mean44,mean11,export44,export11")
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import torch
    from picles_amd import configs, _capi as K
    from picles_amd.parallel import SlabModel

    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    cfg = configs.box4096(n=args.n, U10=10.0, V10=10.0)
    cfg.model["ODEsets"].solver = "DP5"
    model = SlabModel(cfg.model, 0, 1, device=0, halo_rows=1 if args.warmup + args.steps <= 40 else 2)
    b = model.backend
    model.seed()
    pre = int(min(4000, max(5, math.ceil(60e-3 * 6.5e9 / (args.n * args.n)))))      # clock conditioning, as bench.py
    left = pre
    while left > 0:
        model.run_steps(cfg.Δt, min(left, 40))
        left -= 40
        model.seed()
    scales = (1025.0 * 9.81, 1025.0)
    per_leg, memory = {}, {}
    for rnd in range(args.rounds):
        for leg in args.legs.split(","):
            kind, pair = LEGS[leg] if LEGS[leg] is not None else (None, None)
            model.seed()
            if kind:
                b.flux_init(pair, K.FLUX_FIELDS, *scales, 1)
            if kind == "mean":
                b.flux_mean_init(every=1, first=1)
                memory[leg] = b.flux_mean_shape()[2]
            model.run_steps(cfg.Δt, args.warmup)
            extra = {}
            if kind == "export":
                nxc, nyc, nf, npart, _ = b.flux_shape()
                planes = torch.zeros((nf, nyc, nxc), dtype=torch.float32, device="cuda")
                total = torch.zeros((nf, nyc, nxc), dtype=torch.float64, device="cuda")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.sync()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.steps):
                    b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
                    b.flux_export(planes)
                    total += planes
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / args.steps
                extra = {"timed": "torch events around the loop", "mean_phi_in": float(total[0].mean()) / args.steps}
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b.enable_timing(2)
                b.sync()
                torch.cuda.synchronize()
                e0.record()
                model.run_steps(cfg.Δt, args.steps)
                b.sync()
                e1.record()
                torch.cuda.synchronize()
                t = b.get_timing()
                b.enable_timing(0)
                ms = t["advance_ms"] / args.steps
                extra = {"timed": "one event pair around picles_run_steps", "launches": t["advance_launches"],
                         "ms_per_step_torch_events": e0.elapsed_time(e1) / args.steps}
                if kind == "mean":
                    n, t0, t1 = b.flux_mean_scalars()
                    extra["n_samples"] = n
            if kind:
                b.flux_free()                                # the mean set goes with it
            per_leg.setdefault(leg, []).append(ms)
            emit({"leg": leg, "round": rnd, "n": args.n, "steps": args.steps, "ms_per_step": ms, **extra})
    emit({"memory_bytes": memory, "cells": {k: v // 88 for k, v in memory.items()}})
    base = statistics.median(per_leg["none"]) if "none" in per_leg else None
    emit({"summary": {k: {"median_ms": statistics.median(v), "all_ms": v, "over_none_ms": (statistics.median(v) - base) if base is not None else None}
                      for k, v in per_leg.items()}})
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
