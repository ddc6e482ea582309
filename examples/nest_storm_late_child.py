#!/usr/bin/env python3
"""A child switched on late, under a storm: a coarse periodic box (96 x 64 at 6 km) runs alone for three hours under gridded winds
that vary in time — a vortex crossing the box, handed to the device once as an (x, y, t) lattice and sampled there every step — and
writes its own stations.  Then a regional box at a third of the spacing (120 x 90 at 2 km), placed where the storm is heading, is
started from the spun-up parent (`nesting.start_from_parent`: the parent's State prolonged onto the child's nodes on the device, the
child's particles made from it under its own winds at that time) and runs nested to the end, forced through a band three nodes deep
(`NestForcing(width=3)`), with a track of events — a ship crossing the box — sampled on the child.  Both models stay on
`picles_run_steps` throughout; the spin-up's output and the nested leg's go to different directories, because NestForcing begins
the parent's writers for the nested leg as a second run(parent_sim) would.  Needs a HIP device.
python examples/nest_storm_late_child.py [out_dir]"""
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.nesting import NestForcing, start_from_parent
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import StationWriter, read_station_output
from picles_amd.track_output import TrackWriter, read_track_output
from picles_amd.wind_emulator import IdealizedWindGrid, wind_interpolator

out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="picles_late_child_"))
PNX, PNY, PDX = 96, 64, 6000.0
CNX, CNY, CDX, X0, Y0 = 120, 90, 2000.0, 301000.0, 103000.0          # 238 km x 178 km, east of the box's centre
RATIO, DT = 3, 600.0
N_SPIN, N_NESTED = 18, 18                                             # three hours alone, three hours nested
LX, LY = PNX * PDX, PNY * PDX


def storm(x, y, t):
    """a vortex of 90 km radius (8 m/s at its wall) that travels east through the box, in a (12, 4) m/s flow: the wind stays well
    above the growth parameterisation's 2 m/s gate; periodic with the parent through the distance to the nearest image"""
    xc, yc = 0.15 * LX + 0.6 * LX * t / (DT * (N_SPIN + N_NESTED)), 0.5 * LY
    ddx, ddy = (x - xc + 0.5 * LX) % LX - 0.5 * LX, (y - yc + 0.5 * LY) % LY - 0.5 * LY
    r = np.hypot(ddx, ddy) + 1.0
    vt = 8.0 * (r / 9e4) * np.exp(1.0 - r / 9e4)
    return -vt * ddy / r + 12.0, vt * ddx / r + 4.0


lattice = IdealizedWindGrid(lambda x, y, t: storm(x, y, t)[0], lambda x, y, t: storm(x, y, t)[1],
                            dict(Lx=LX, Ly=LY, T=DT * (N_SPIN + N_NESTED + 2)), dict(dx=LX / 48, dy=LY / 32, dt=1800.0))
winds = wind_interpolator(lattice)                                    # piecewise linear in time: a knot every third parent step


def box(grid, periodic):
    cfg = configs.bench06_box(n=16, dx=PDX, periodic_grid=periodic)
    cfg.model["grid"] = grid
    cfg.model["winds"] = winds                                        # one lattice for both: each model samples it at its own nodes
    cfg.model["winds_static"] = False
    cfg.model["ODEsys"] = particle_equations(winds.u, winds.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=True, dissipation=True)
    return WaveGrowth2D(**cfg.model)


parent = box(TwoDCartesianGridMesh(PDX * (PNX - 1), PNX, PDX * (PNY - 1), PNY, periodic_boundary=(True, True)), True)
child = box(TwoDCartesianGridMesh(X0, X0 + CDX * (CNX - 1), CNX, Y0, Y0 + CDX * (CNY - 1), CNY, periodic_boundary=(False, False)), False)
centre = (X0 + CDX * (CNX // 2), Y0 + CDX * (CNY // 2))

# ---- the spin-up: the parent alone, chunked under the lattice ----
parent_sim = Simulation(parent, Δt=DT, stop_time=DT * (N_SPIN - 1))
parent_sim.output_writers["stations"] = StationWriter(parent, points=[centre], names=["parent at the child's centre"], schedule=3,
                                                      path=out_dir / "spin_up", name="parent", format="npy")
run(parent_sim)
t_on = parent.clock.time
print(f"spin-up: {parent.clock.iteration} parent steps in {parent_sim.run_wall_time:.3f} s; the child is switched on at t = {t_on / 3600:.1f} h")

# ---- the child, started from the parent, nested to the end ----
child_sim = Simulation(child, Δt=DT / RATIO, stop_time=t_on + DT / RATIO * (N_NESTED * RATIO - 1))
start_from_parent(child_sim, parent_sim)
S0 = child.State.copy()
print(f"child started: mean Hs {4 * np.sqrt(np.mean(S0[..., 0])):.3f} m over {CNX} x {CNY} nodes, {int(child.ParticleCollection.on.sum())} particles")
parent_sim.stop_time = t_on + DT * (N_NESTED - 1)
parent_sim.output_writers["stations"].path = out_dir / "nested"     # the same writer (it owns the parent's probe set), another directory
child_sim.output_writers["stations"] = StationWriter(child, points=[centre], names=["child centre"], schedule=3 * RATIO,
                                                     path=out_dir / "nested", name="child", format="npy")
n_events = 24                                                         # a ship crossing the child from south-west to north-east
ship_t = t_on + np.linspace(300.0, DT * N_NESTED - 300.0, n_events)
ship_xy = [(X0 + CDX * (4 + (CNX - 9) * k / (n_events - 1)), Y0 + CDX * (4 + (CNY - 9) * k / (n_events - 1))) for k in range(n_events)]
child_sim.output_writers["tracks"] = TrackWriter(child, times=ship_t, points=ship_xy, path=out_dir / "nested", name="ship", format="npy")
nest = child_sim.output_writers["boundary_forcing"] = NestForcing(child, parent=parent_sim, side="rim", ratio=RATIO, width=3)
run(child_sim)

print(f"nested leg: child {child.clock.iteration} steps of {child_sim.Δt:.0f} s, parent {nest.parent_steps} steps of {DT:.0f} s, in {child_sim.run_wall_time:.3f} s; "
      f"{len(nest.nodes)} band nodes fed from {len(nest.corner_nodes)} parent nodes, {nest.uploads} levels taken; files in {out_dir}")
p, c = read_station_output(out_dir / "nested", "parent"), read_station_output(out_dir / "nested", "child")
hs = list(p["var_names"]).index("hs")
for k in range(min(len(p["time"]), len(c["time"]))):
    print(f"t = {p['time'][k] / 3600:4.1f} h   Hs at the child's centre: parent {p['data'][k, 0, hs]:.3f} m, child {c['data'][k, 0, hs]:.3f} m")
ship = read_track_output(out_dir / "nested", "ship")
ship_hs = np.asarray(ship["data"])[list(ship["var_names"]).index("hs")]
print("Hs along the ship's track [m]: " + " ".join(f"{v:.2f}" for v in ship_hs[::3]))
