"""Cost of the open-boundary forcing: the 4096^2 non-periodic box (DP5, winds (10,10)) with its whole rim forced
(16,380 nodes) against the same box without a set, 20 steps per round inside one event pair, four alternated rounds in one process.
Two forcings: swell at 8 m/s (2.4 cells per step) and at 2 m/s (0.6 cells per step).  One JSON line on stdout.
--profile: a short forced run and nothing else, for `rocprofv3 --kernel-trace --stats -- python scripts/bforce_cost.py --profile`.
--width W[,W...]: the cost of a band instead — the whole rim forced W nodes deep with swell at 8 m/s, unweighted and
with the "linear" ramp, against "no set", four alternated rounds in one process; with --profile the first width alone (add --linear
for the blend flavour)."""
import json
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from picles_amd import configs, models
from picles_amd.boundary_forcing import band_nodes, linear_weights, rim_nodes
from picles_amd.simulations import Simulation, initialize_simulation

N, K, W = 4096, 20, 5
profile = "--profile" in sys.argv


widths = [int(x) for x in sys.argv[sys.argv.index("--width") + 1].split(",")] if "--width" in sys.argv else []


def build(forced, cb=8.0, width=None, linear=False):
    cfg = configs.box4096(n=N, periodic_grid=False)
    m = models.WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    if forced:
        e, th = 1.0, math.pi / 4
        if width is None:
            rim = rim_nodes(m.grid, "rim")
            m.backend.bforce_init(rim)
        else:
            rim, d = band_nodes(m.grid, "rim", width)
            m.backend.bforce_init_band(rim, linear_weights(d, width) if linear else None)
        v = np.tile([e, e / (2 * cb) * math.cos(th), e / (2 * cb) * math.sin(th)], (len(rim), 1))
        m.backend.bforce_set_levels(0.0, v, 1e9, 1.5 * v)
        print("forced nodes:", len(rim), file=sys.stderr)
    return m, cfg.Δt


def timed(m, dt):
    b = m.backend
    b.enable_timing(2)
    b.run_steps(dt, K)
    t = b.get_timing()
    b.enable_timing(0)
    return t["advance_ms"] / K


if profile:
    m, dt = build(True, width=widths[0], linear="--linear" in sys.argv) if widths else build(True)
    m.backend.run_steps(dt, W + 10)
    m.backend.sync()
    sys.exit(0)

if widths:
    plain, dt = build(False)
    sets = {f"width{w}{'_linear' if lin else ''}": build(True, width=w, linear=lin)[0] for w in widths for lin in (False, True)}
    for m in [plain] + list(sets.values()):
        m.backend.run_steps(dt, W)
        m.backend.sync()
    ms = {k: [] for k in ["no_set"] + list(sets)}
    for r in range(4):
        ms["no_set"].append(timed(plain, dt))
        for k, m in sets.items():
            ms[k].append(timed(m, dt))
        print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.4f}" for k, v in ms.items()) + " ms/step", file=sys.stderr)
    print(json.dumps({"n": N, "steps_per_round": K, "swell_cells_per_step": 8.0 * dt / 2000.0, "ms_per_step": ms,
                      "median_ms_per_step": {k: float(np.median(v)) for k, v in ms.items()},
                      "forced_nodes": {k: m.backend.bforce_info()[0] for k, m in sets.items()},
                      "counters": {k: m.backend.get_counters() for k, m in [("no_set", plain)] + list(sets.items())}}))
    sys.exit(0)

plain, dt = build(False)
forced, _ = build(True)
slow, _ = build(True, cb=2.0)          # 0.6 cells per step: the scatter reach stays 1
for m in (plain, forced, slow):
    m.backend.run_steps(dt, W)
    m.backend.sync()
rows, slows = [], []
for r in range(4):
    a = timed(plain, dt)
    b = timed(forced, dt)
    s_ = timed(slow, dt)
    rows.append((a, b))
    slows.append(s_)
    print(f"round {r}: unforced {a:.4f} ms/step, forced (2.4 cells/step) {b:.4f}, forced (0.6 cells/step) {s_:.4f}", file=sys.stderr)
c = forced.backend.get_counters()
out = {"n": N, "steps_per_round": K, "unforced_ms": [x for x, _ in rows], "forced_ms": [y for _, y in rows],
       "median_unforced_ms": float(np.median([x for x, _ in rows])), "median_forced_ms": float(np.median([y for _, y in rows])),
       "unforced_counters": plain.backend.get_counters(), "forced_counters": c, "slow_forced_ms": slows, "median_slow_forced_ms": float(np.median(slows)),
       "slow_counters": slow.backend.get_counters()}
print(json.dumps(out))
