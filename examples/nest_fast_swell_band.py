#!/usr/bin/env python3
"""Fast swell through a nest, with and without a forcing band.  A calm 128 x 16 box at 2 km, every source term off, with swell at
8 m/s forced through its west column; the child is the parent's own sub-box (rows 2..10, columns 8..77), same spacing, same
ten-minute step — 2.4 cells a step.  With a one-node rim the swell crosses the child's rim column between two parent levels and
never enters; with a band as deep as the swell travels (`NestForcing(..., width=3)`, picles_bforce_init_band) the child outside its
band is the parent, to the bit.  A third child relaxes towards the parent over the same band (`weights="linear"`): its inner
band nodes carry two thirds of the child's own, still incomplete, state, so it trades the exact entry for a smooth seam — the
choice for a child whose own sea differs from the parent's, not for this one.  Needs a HIP device."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.boundary_forcing import BoundaryForcing
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.nesting import NestForcing
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, run

DX, DT, N_STEPS = 2000.0, 600.0, 10
PNX, PNY, CNX, CNY, COL0, ROW0 = 128, 16, 70, 9, 8, 2
CBAR, THETA = 8.0, 0.15
WIDTH = int(np.ceil(CBAR * DT / DX))          # cells the swell travels in a step, rounded up: 3


def calm_box(grid):
    cfg = configs.bench06_box(n=16, dx=DX, periodic_grid=False)
    w = configs.const_winds(0.0, 0.0)
    cfg.model["grid"], cfg.model["winds"] = grid, w
    cfg.model["ODEsys"] = particle_equations(w.u, w.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=False,
                                             dissipation=False, peak_shift=False, direction=False)
    return WaveGrowth2D(**cfg.model)


def nested(width, weights=None):
    parent = calm_box(TwoDCartesianGridMesh(DX * (PNX - 1), PNX, DX * (PNY - 1), PNY, periodic_boundary=(False, False)))
    psim = Simulation(parent, Δt=DT, stop_time=DT * (N_STEPS - 1))
    swell = np.tile([1.0, np.cos(THETA) / (2.0 * CBAR), np.sin(THETA) / (2.0 * CBAR)], (PNY, 1))
    psim.output_writers["boundary_forcing"] = BoundaryForcing(parent, side="west", times=[0.0], values=swell[None])
    child = calm_box(TwoDCartesianGridMesh(COL0 * DX, (COL0 + CNX - 1) * DX, CNX, ROW0 * DX, (ROW0 + CNY - 1) * DX, CNY,
                                           periodic_boundary=(False, False)))
    csim = Simulation(child, Δt=DT, stop_time=DT * (N_STEPS - 1))
    nest = csim.output_writers["boundary_forcing"] = NestForcing(child, parent=psim, side="rim", ratio=1, width=width, weights=weights)
    run(csim)
    inner = slice(WIDTH, CNX - WIDTH), slice(WIDTH, CNY - WIDTH)
    ec = child.backend.get_state()[inner][..., 0]
    ep = parent.backend.get_state()[COL0 + WIDTH:COL0 + CNX - WIDTH, ROW0 + WIDTH:ROW0 + CNY - WIDTH, 0]
    return len(nest.nodes), float(np.abs(ec - ep).max() / ep.max()), int((ec == ep).sum()), ec.size


print(f"swell at {CBAR} m/s, Δt = {DT:.0f} s, dx = {DX:.0f} m: {CBAR * DT / DX:.1f} cells a step; band width {WIDTH}")
for label, width, weights in (("one-node rim", 1, None), (f"band of {WIDTH}", WIDTH, None), (f"band of {WIDTH}, linear ramp", WIDTH, "linear")):
    n, off, same, size = nested(width, weights)
    print(f"{label:28s} {n:4d} forced nodes: child off by {off:.3e} of the parent's largest energy outside the band; "
          f"{same} of {size} nodes equal to the bit")
