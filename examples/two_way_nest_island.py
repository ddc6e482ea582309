#!/usr/bin/env python3
"""Two-way nesting: an island only the child resolves casts its shadow into the parent.  A calm 128 x 16 box at 2 km, every
source term off, with a pulse of swell at 8 m/s on its western half (2.4 cells a step); the child is the parent's own sub-box (rows
2..10, columns 40..109), same spacing and step, forced over a three-deep band — and carries a land block of 4 x 3 nodes that the
parent's mask lacks.  One-way (`NestForcing(...)`) the parent never learns of it and equals the parent alone to the bit.  Two-way
(`NestForcing(..., feedback=True)`, picles_nest_feedback_*) the child's State is restricted onto the parent's ocean nodes under it
before every parent step: where the child is calm the parent's node bears no particle, and the parent's energy drops in the lee.
The parent of a fed model carries no forcing set of its own, so the swell starts in the box.  Needs a HIP device."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.nesting import NestForcing
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, initialize_simulation, run

DX, DT, N_STEPS = 2000.0, 600.0, 10
PNX, PNY, CNX, CNY, COL0, ROW0 = 128, 16, 70, 9, 40, 2
CBAR, THETA = 8.0, 0.15
WIDTH = int(np.ceil(CBAR * DT / DX))          # cells the swell travels in a step, rounded up: 3
ISLAND = (slice(30, 34), slice(3, 6))         # child nodes: parent columns 70..73, rows 5..7


def calm_box(grid):
    cfg = configs.bench06_box(n=16, dx=DX, periodic_grid=False)
    w = configs.const_winds(0.0, 0.0)
    cfg.model["grid"], cfg.model["winds"] = grid, w
    cfg.model["ODEsys"] = particle_equations(w.u, w.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=False,
                                             dissipation=False, peak_shift=False, direction=False)
    return WaveGrowth2D(**cfg.model)


def start(model, sim, state):
    """the model holds `state` and the particles of it"""
    initialize_simulation(sim)
    model.backend.set_state(state)
    model.backend.remesh(DT)


def parent_after(mode):
    """the parent's energy after ten steps: mode None — alone; False — beside a one-way child; True — fed by it"""
    swell = np.zeros((PNX, PNY, 3))
    swell[1:61, 1:PNY - 1] = (1.0, np.cos(THETA) / (2.0 * CBAR), np.sin(THETA) / (2.0 * CBAR))
    parent = calm_box(TwoDCartesianGridMesh(DX * (PNX - 1), PNX, DX * (PNY - 1), PNY, periodic_boundary=(False, False)))
    psim = Simulation(parent, Δt=DT, stop_time=DT * (N_STEPS - 1))
    start(parent, psim, swell)
    if mode is None:
        run(psim)
        return parent.backend.get_state()[..., 0], None
    sea = np.ones((CNX, CNY), dtype=bool)
    sea[ISLAND] = False
    child = calm_box(TwoDCartesianGridMesh(COL0 * DX, (COL0 + CNX - 1) * DX, CNX, ROW0 * DX, (ROW0 + CNY - 1) * DX, CNY, mask=sea,
                                           periodic_boundary=(False, False)))
    csim = Simulation(child, Δt=DT, stop_time=DT * (N_STEPS - 1))
    start(child, csim, np.where(sea[..., None], swell[COL0:COL0 + CNX, ROW0:ROW0 + CNY], 0.0))
    nest = csim.output_writers["boundary_forcing"] = NestForcing(child, parent=psim, side="rim", ratio=1, width=WIDTH, feedback=mode)
    run(csim)
    return parent.backend.get_state()[..., 0], nest


alone, _ = parent_after(None)
one_way, _ = parent_after(False)
two_way, nest = parent_after(True)
row = nest.fb_nodes[0, 1]
print(f"swell at {CBAR} m/s, Δt = {DT:.0f} s, dx = {DX:.0f} m: {CBAR * DT / DX:.1f} cells a step; band width {WIDTH}; "
      f"{len(nest.fb_nodes)} parent nodes fed (row {row}, columns {nest.fb_nodes[0, 0]}..{nest.fb_nodes[-1, 0]}, margin {nest.feedback_margin}), "
      f"{nest.feedbacks} levels taken")
print(f"one-way: the parent equals the parent alone at {int((one_way == alone).sum())} of {alone.size} nodes")
print(f"two-way: the parent differs from the parent alone at {int((two_way != alone).sum())} nodes, none of them upwind of the child: "
      f"{bool((two_way[:COL0] == alone[:COL0]).all())}")
cols = np.arange(COL0 + 28, COL0 + 44)
print("parent energy on the fed row, columns", cols[0], "..", cols[-1], "(the island is on 70..73)")
print("  alone  ", np.array2string(alone[cols, row], precision=2, floatmode="fixed", max_line_width=200))
print("  two-way", np.array2string(two_way[cols, row], precision=2, floatmode="fixed", max_line_width=200))
