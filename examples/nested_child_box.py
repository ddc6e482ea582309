#!/usr/bin/env python3
"""A nested child box: a coarse periodic box (96 x 64 at 6 km) under smooth winds, and inside it a regional box at a third of the
spacing (120 x 90 at 2 km) whose whole rim is forced by the coarse model while both run — one-way nesting on the device.  The parent
takes one ten-minute step for every three steps of the child and stays one step ahead of it; behind each of its steps two small
kernels take the sea state at the parent nodes around the child's rim and mix it onto the rim nodes (picles_nest_*,
include/picles_hip.h).  Neither model leaves the fused `picles_run_steps` path and no State crosses PCIe.  The parent writes its own
stations as it would alone.  Needs a HIP device."""
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.nesting import NestForcing
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import StationWriter, read_station_output

out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="picles_nest_"))
PNX, PNY, PDX = 96, 64, 6000.0
CNX, CNY, CDX, X0, Y0 = 120, 90, 2000.0, 151000.0, 97000.0          # 238 km x 178 km, well inside the 576 km x 384 km parent
RATIO, DT = 3, 600.0
winds = configs.smooth_winds(10.0, 6.0, PNX * PDX, PNY * PDX)         # one wind field in the common frame, periodic with the parent


def box(grid, periodic):
    cfg = configs.bench06_box(n=16, dx=PDX, periodic_grid=periodic)
    cfg.model["grid"] = grid
    cfg.model["winds"] = winds
    cfg.model["ODEsys"] = particle_equations(winds.u, winds.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=True, dissipation=True)
    return WaveGrowth2D(**cfg.model)


parent = box(TwoDCartesianGridMesh(PDX * (PNX - 1), PNX, PDX * (PNY - 1), PNY, periodic_boundary=(True, True)), True)
child = box(TwoDCartesianGridMesh(X0, X0 + CDX * (CNX - 1), CNX, Y0, Y0 + CDX * (CNY - 1), CNY, periodic_boundary=(False, False)), False)

n_parent = 36                                                         # six hours
parent_sim = Simulation(parent, Δt=DT, stop_time=DT * (n_parent - 1))
child_sim = Simulation(child, Δt=DT / RATIO, stop_time=DT / RATIO * (n_parent * RATIO - 1))
centre = (X0 + CDX * (CNX // 2), Y0 + CDX * (CNY // 2))
parent_sim.output_writers["stations"] = StationWriter(parent, points=[centre], names=["parent at the child's centre"], schedule=6,
                                                      path=out_dir, name="parent", format="npy")
child_sim.output_writers["stations"] = StationWriter(child, points=[centre], names=["child centre"], schedule=6 * RATIO,
                                                     path=out_dir, name="child", format="npy")
nest = child_sim.output_writers["boundary_forcing"] = NestForcing(child, parent=parent_sim, side="rim", ratio=RATIO)
run(child_sim)

print(f"child: {child.clock.iteration} steps of {child_sim.Δt:.0f} s, parent: {parent.clock.iteration} steps of {DT:.0f} s, in {child_sim.run_wall_time:.3f} s; "
      f"{len(nest.nodes)} rim nodes fed from {len(nest.corner_nodes)} parent nodes, {nest.uploads} levels taken; files in {out_dir}")
p, c = read_station_output(out_dir, "parent"), read_station_output(out_dir, "child")
hs = list(p["var_names"]).index("hs")
for k in range(min(len(p["time"]), len(c["time"]))):
    print(f"t = {p['time'][k] / 3600:4.1f} h   Hs at the child's centre: parent {p['data'][k, 0, hs]:.3f} m, child {c['data'][k, 0, hs]:.3f} m")
S = child.State.copy()
print(f"child rim mean Hs {4 * np.sqrt(np.mean(S[0, :, 0])):.3f} m (west), interior mean Hs {4 * np.sqrt(np.mean(S[1:-1, 1:-1, 0])):.3f} m")
