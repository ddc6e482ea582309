#!/usr/bin/env python3
"""stat_cost.py — what the run statistics (picles_stat_*) cost per step on one GPU, at the BASELINE box (4096², winds (10,10), DP5).

Legs, alternated over --rounds rounds on ONE context (re-seeded before every leg, clocks conditioned once as bench.py does):

    none     no statistics set                        (the run the others are compared with)
    peak1    PICLES_STAT_PEAK alone, updated every step
    all1     every group, four thresholds, updated every step
    all10    every group, four thresholds, every = 10

Each leg: seed, W warm-up steps, then K steps in one picles_run_steps call inside ONE event pair (picles_enable_timing(ctx, 2)):
ms per step = region / K.  The yardstick is the stand-alone k_scatter (scatter + remesh of a step completed by somebody looking:
picles_time_step + picles_sync per step, events around every launch), timed in the same process.

    python scripts/stat_cost.py [--grid-n 4096] [--steps 40] [--warmup 5] [--rounds 3] [--legs none,peak1,all1,all10] [--out FILE]
    python scripts/stat_cost.py --tree OTHER_CHECKOUT --legs none        # the yardstick of another checkout (no picles_stat_*)

Prints one JSON line per leg and round, then a summary line; --out appends them to a file.  For the kernel's own time run it under
`rocprofv3 --kernel-trace --stats -- python scripts/stat_cost.py --legs all1 --rounds 1` in a run of its own.
"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

LEGS = {"none": None, "peak1": (1, (), 1), "all1": (7, (1.0, 2.0, 3.0, 4.0), 1), "all10": (7, (1.0, 2.0, 3.0, 4.0), 10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid-n", dest="n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="none,peak1,all1,all10")
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-yardstick", action="store_true")
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
    per_leg = {}
    for rnd in range(args.rounds):
        for leg in args.legs.split(","):
            model.seed()
            if LEGS[leg] is not None:
                mask, thr, every = LEGS[leg]
                b.stat_init(mask, thr, every=every, first=1)
            model.run_steps(cfg.Δt, args.warmup)
            b.enable_timing(2)
            torch.cuda.synchronize()
            model.run_steps(cfg.Δt, args.steps)
            torch.cuda.synchronize()
            t = b.get_timing()
            b.enable_timing(0)
            ms = t["advance_ms"] / args.steps
            extra = {}
            if LEGS[leg] is not None:
                acc = b.stat_get(0)
                extra = {"n_samples": acc["n_samples"], "wet_share": float((acc["n_wet"] > 0).mean())}
                b.stat_free()
            per_leg.setdefault(leg, []).append(ms)
            emit({"leg": leg, "round": rnd, "n": args.n, "steps": args.steps, "ms_per_step": ms, "launches": t["advance_launches"], **extra})
    if not args.no_yardstick:
        # the stand-alone scatter + remesh: every step completed by a picles_sync, events around every launch
        model.seed()
        model.run_steps(cfg.Δt, args.warmup)
        b.sync()
        b.enable_timing(1)
        for _ in range(10):
            b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
            b.sync()
        t = b.get_timing()
        s = b.get_timing_samples(1)
        emit({"leg": "k_scatter_standalone", "n": args.n, "launches": t["scatter_launches"], "ms_mean": t["scatter_ms"] / max(1, t["scatter_launches"]),
              "ms_median": float(statistics.median(s)) if len(s) else None, "ms_min": float(min(s)) if len(s) else None})
    base = statistics.median(per_leg["none"]) if "none" in per_leg else None
    emit({"summary": {k: {"median_ms": statistics.median(v), "all_ms": v, "over_none_ms": (statistics.median(v) - base) if base is not None else None}
                      for k, v in per_leg.items()}})
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
