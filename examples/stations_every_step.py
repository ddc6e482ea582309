#!/usr/bin/env python3
"""Station output at every step: the sea state at five points of a 512² periodic box — significant wave height, peak period, group
velocity and direction — written once per model step, while the run itself stays on the fused `picles_run_steps` path.

What the reference's scripts plot out of full `cash_store` snapshots (`State[i, j, :]` against time, tests/T04_2D_reg_test.jl) is
sampled on the device behind each step, for the stations' corner nodes only (picles_probe_*, include/picles_hip.h): twenty nodes
instead of 3 float64 planes of 512².  Needs a HIP device."""
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import StationWriter, read_station_output

out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="picles_stations_"))
n = 512
L = 2000.0 * n
cfg = configs.bench06_box(n=n, winds=configs.smooth_winds(10.0, 10.0, L, L))
model = WaveGrowth2D(**cfg.model)
sim = Simulation(model, Δt=cfg.Δt, stop_time=cfg.Δt * 59)          # 60 steps: run! takes one step past stop_time
points = [(0.1 * L, 0.1 * L), (0.25 * L, 0.75 * L), (0.5 * L, 0.5 * L), (0.75 * L, 0.25 * L), (L - 1000.0, L - 1000.0)]   # the last one: the wrap cell
sim.output_writers["stations"] = StationWriter(model, points=points, names=["SW", "NW", "centre", "SE", "wrap"], schedule=1,
                                               path=out_dir, format="npy")
run(sim)

out = read_station_output(out_dir)
data, var = out["data"], list(out["var_names"])                      # [time, station, var]
print(f"{model.clock.iteration} steps in {sim.run_wall_time:.3f} s, {data.shape[0]} records of {data.shape[1]} stations in {out_dir}")
hs, tp, direction = data[..., var.index("hs")], data[..., var.index("tp")], np.degrees(data[..., var.index("dir")])
for k in range(0, data.shape[0], 10):
    row = "   ".join(f"{name} Hs {hs[k, s]:.3f} m Tp {tp[k, s]:.2f} s {direction[k, s]:5.1f} deg" for s, name in enumerate(out["names"]))
    print(f"t = {out['time'][k] / 3600:5.2f} h   {row}")
