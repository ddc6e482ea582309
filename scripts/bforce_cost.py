"""Cost of the open-boundary forcing: the 4096^2 non-periodic box (DP5, winds (10,10)) with its whole rim forced
(16,380 nodes) against the same box without a set, 20 steps per round inside one event pair, four alternated rounds in one process.
Two forcings: swell at 8 m/s (2.4 cells per step) and at 2 m/s (0.6 cells per step).  One JSON line on stdout.
--profile: a short forced run and nothing else, for `rocprofv3 --kernel-trace --stats -- python scripts/bforce_cost.py --profile`."""
import json
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from picles_amd import configs, models
from picles_amd.boundary_forcing import rim_nodes
from picles_amd.simulations import Simulation, initialize_simulation

N, K, W = 4096, 20, 5
profile = "--profile" in sys.argv


def build(forced, cb=8.0):
    cfg = configs.box4096(n=N, periodic_grid=False)
    m = models.WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    if forced:
        rim = rim_nodes(m.grid, "rim")
        e, th = 1.0, math.pi / 4
        v = np.tile([e, e / (2 * cb) * math.cos(th), e / (2 * cb) * math.sin(th)], (len(rim), 1))
        m.backend.bforce_init(rim)
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
    m, dt = build(True)
    m.backend.run_steps(dt, W + 10)
    m.backend.sync()
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
