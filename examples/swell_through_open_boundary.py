#!/usr/bin/env python3
"""Swell through an open boundary: a 256 x 128 regional box under a light local wind, with a swell train — significant wave height
rising from 1 m to 3 m over six hours, peak period 11 s, heading east-north-east — prescribed along its west side, and a line of
stations watching it cross the box.  The run stays on the fused `picles_run_steps` path: behind each step one small kernel bears
the rim's particles from the prescribed sea state (picles_bforce_*, include/picles_hip.h), and the time levels are uploaded a pair
at a time between chunks.  Needs a HIP device."""
import math
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.boundary_forcing import BoundaryForcing, sea_state
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import StationWriter, read_station_output

out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="picles_swell_"))
nx, ny, dx = 256, 128, 2000.0
cfg = configs.bench06_box(n=16, dx=dx, U10=4.0, V10=3.0, periodic_grid=False)          # periodic_boundary = false: an open rim
cfg.model["grid"] = TwoDCartesianGridMesh(dx * (nx - 1), nx, dx * (ny - 1), ny, periodic_boundary=(False, False))
model = WaveGrowth2D(**cfg.model)
n_steps = 72                                                                           # twelve hours of ten-minute steps
sim = Simulation(model, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1))

hours = np.arange(0.0, 13.0)                                                           # one level per hour
hs = np.where(hours < 6.0, 1.0 + hours / 3.0, 3.0)


def level(t):
    """(e, m_x, m_y) on the west column at time t: the swell is weaker towards the corners of the side"""
    taper = np.sin(np.linspace(0.0, math.pi, ny)) ** 2
    e, mx, my = sea_state(np.interp(t / 3600.0, hours, hs) * np.sqrt(taper), 11.0, math.radians(20.0), model)
    return np.stack([e, mx, my], axis=1)          # a node whose value falls under the model's minimal state bears no particle


sim.output_writers["boundary_forcing"] = BoundaryForcing(model, side="west", times=3600.0 * hours, values=level, Δt=cfg.Δt)
line = [(i, ny // 2) for i in (1, 16, 64, 128, 240)]
sim.output_writers["stations"] = StationWriter(model, nodes=line, names=[f"{i * dx / 1000:.0f} km" for i, _ in line], schedule=6,
                                               path=out_dir, format="npy")
run(sim)

out = read_station_output(out_dir)
data, var = out["data"], list(out["var_names"])
print(f"{model.clock.iteration} steps in {sim.run_wall_time:.3f} s; {sim.output_writers['boundary_forcing'].uploads} level pairs uploaded; files in {out_dir}")
for k in range(data.shape[0]):
    row = "   ".join(f"{name}: Hs {data[k, s, var.index('hs')]:.2f} m Tp {data[k, s, var.index('tp')]:.1f} s" for s, name in enumerate(out["names"]))
    print(f"t = {out['time'][k] / 3600:5.2f} h   {row}")
