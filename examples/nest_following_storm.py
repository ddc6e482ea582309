#!/usr/bin/env python3
"""A child box that follows the storm: a coarse periodic box (96 x 64 at 6 km) runs under gridded winds that vary in time — a vortex
crossing the box, handed to the device once as an (x, y, t) lattice and sampled there every step.  After a spin-up a fine box at a
third of the spacing (90 x 72 at 2 km: 178 km x 142 km, far smaller than the storm's track) is started from the parent where the
wind is strongest and then FOLLOWS the wind maximum across the parent (`nesting.run_following`): every two parent steps the box is
moved by whole child nodes (`nesting.move_child`, picles_nest_relocate) — where the old and the new box overlap the child keeps the
sea it has resolved, the freshly exposed strip takes the parent's, and the lattice is sampled at the new nodes without being uploaded
again.  A fixed child would have to cover the whole track at the fine spacing.  Nothing crosses PCIe in a move.  Needs a HIP device.
python examples/nest_following_storm.py"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.nesting import run_following, start_from_parent
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, run
from picles_amd.wind_emulator import IdealizedWindGrid, wind_interpolator

PNX, PNY, PDX = 96, 64, 6000.0
CNX, CNY, CDX = 90, 72, 2000.0
RATIO, DT, EVERY = 3, 600.0, 2
N_SPIN, N_LEGS = 12, 9                                                # two hours alone, three hours followed
LX, LY = PNX * PDX, PNY * PDX
T_END = DT * (N_SPIN + EVERY * N_LEGS)


def storm(x, y, t):
    """a vortex of 60 km radius (10 m/s at its wall) that travels east and a little north through the box, in a (9, 3) m/s flow"""
    xc, yc = 0.2 * LX + 0.55 * LX * t / T_END, 0.4 * LY + 0.15 * LY * t / T_END
    ddx, ddy = (x - xc + 0.5 * LX) % LX - 0.5 * LX, (y - yc + 0.5 * LY) % LY - 0.5 * LY
    r = np.hypot(ddx, ddy) + 1.0
    vt = 10.0 * (r / 6e4) * np.exp(1.0 - r / 6e4)
    return -vt * ddy / r + 9.0, vt * ddx / r + 3.0


lattice = IdealizedWindGrid(lambda x, y, t: storm(x, y, t)[0], lambda x, y, t: storm(x, y, t)[1],
                            dict(Lx=LX, Ly=LY, T=T_END + 2 * DT), dict(dx=LX / 48, dy=LY / 32, dt=1800.0))
winds = wind_interpolator(lattice)


def box(grid, periodic):
    cfg = configs.bench06_box(n=16, dx=PDX, periodic_grid=periodic)
    cfg.model["grid"] = grid
    cfg.model["winds"] = winds                                        # one lattice for both: each model samples it at its own nodes
    cfg.model["winds_static"] = False
    cfg.model["ODEsys"] = particle_equations(winds.u, winds.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=True, dissipation=True)
    return WaveGrowth2D(**cfg.model)


parent = box(TwoDCartesianGridMesh(PDX * (PNX - 1), PNX, PDX * (PNY - 1), PNY, periodic_boundary=(True, True)), True)
PX, PY = parent.grid.data.x, parent.grid.data.y


def wind_maximum(t):
    """where the wind is strongest on the parent's nodes at time t: what the box follows"""
    k = np.unravel_index(np.argmax(np.hypot(winds.u(PX, PY, t), winds.v(PX, PY, t))), PX.shape)
    return float(PX[k]), float(PY[k])


# ---- the spin-up: the parent alone ----
parent_sim = Simulation(parent, Δt=DT, stop_time=DT * (N_SPIN - 1))
run(parent_sim)
t_on = parent.clock.time
parent_sim.stop_time = 1e12

# ---- the child, started where the wind is strongest, on whole child nodes ----
cx, cy = wind_maximum(t_on)
X0 = CDX * round((cx - 0.5 * CDX * (CNX - 1)) / CDX) + 1000.0         # (off the parent's nodes: every weight is non-trivial)
Y0 = CDX * round((cy - 0.5 * CDX * (CNY - 1)) / CDX) + 1000.0
child = box(TwoDCartesianGridMesh(X0, X0 + CDX * (CNX - 1), CNX, Y0, Y0 + CDX * (CNY - 1), CNY, periodic_boundary=(False, False)), False)
child_sim = Simulation(child, Δt=DT / RATIO, stop_time=0.0)
start_from_parent(child_sim, parent_sim)
print(f"spin-up: {parent.clock.iteration} parent steps; the child ({CNX} x {CNY} at {CDX / 1e3:.0f} km) is switched on at t = {t_on / 3600:.1f} h "
      f"with its origin at ({X0 / 1e3:.0f}, {Y0 / 1e3:.0f}) km")


def report(k, sim):
    S = np.asarray(sim.model.State)
    g = sim.model.grid
    print(f"leg {k}: t = {sim.model.clock.time / 3600:4.2f} h   box x {g.stats.xmin / 1e3:5.0f}..{g.stats.xmax / 1e3:5.0f} km, y {g.stats.ymin / 1e3:5.0f}..{g.stats.ymax / 1e3:5.0f} km   "
          f"max Hs in the box {4 * np.sqrt(np.nanmax(S[..., 0])):.3f} m")


boxes = run_following(child_sim, parent_sim, wind_maximum, stop_time=t_on + DT * EVERY * N_LEGS, every=EVERY,
                      nest=dict(side="rim", ratio=RATIO, width=3), on_leg=report)
report(N_LEGS, child_sim)
moved = sum(a[1:] != b[1:] for a, b in zip(boxes, boxes[1:]))
print(f"{N_LEGS} legs of {EVERY} parent steps, {moved} moves; the box travelled {(boxes[-1][1] - boxes[0][1]) / 1e3:.0f} km east and "
      f"{(boxes[-1][2] - boxes[0][2]) / 1e3:.0f} km north while the child covers {CDX * (CNX - 1) / 1e3:.0f} km x {CDX * (CNY - 1) / 1e3:.0f} km; "
      f"child {child.clock.iteration} steps, parent {parent.clock.iteration}")
assert np.isfinite(np.asarray(child.State)).all() and moved > 0
