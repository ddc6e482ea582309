#!/usr/bin/env python3
"""A nested pair stopped and picked up: the boxes of examples/nested_child_box.py — a coarse periodic box (96 x 64 at 6 km) and a
regional box inside it at a third of the spacing (120 x 90 at 2 km), whole rim forced — with a Checkpointer on the child.  A
three-hour job writes a pair checkpoint every 20 child steps: the child's file, the parent's at the parent's own clock (the parent is
a step ahead between its levels) and the pair of parent levels the child held (`<child file>.nest.npz`).  The job ends; a second
program builds both models again and `run(child_sim, pickup=True)` continues to six hours from the latest complete trio.  A third run
goes through the six hours without a stop: both models of the picked-up run equal it to the bit.  Needs a HIP device."""
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.checkpointing import Checkpointer, list_checkpoints
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.nesting import NestForcing, link_path, parent_checkpoint_path
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, run

out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="picles_nest_restart_"))
PNX, PNY, PDX = 96, 64, 6000.0
CNX, CNY, CDX, X0, Y0 = 120, 90, 2000.0, 151000.0, 97000.0
RATIO, DT = 3, 600.0
winds = configs.smooth_winds(10.0, 6.0, PNX * PDX, PNY * PDX)


def box(grid, periodic):
    cfg = configs.bench06_box(n=16, dx=PDX, periodic_grid=periodic)
    cfg.model["grid"] = grid
    cfg.model["winds"] = winds
    cfg.model["ODEsys"] = particle_equations(winds.u, winds.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=True, dissipation=True)
    return WaveGrowth2D(**cfg.model)


def nested_pair(n_child, ckdir):
    """what every program of the cycle builds from its script: both models, the nest, the child's Checkpointer"""
    parent = box(TwoDCartesianGridMesh(PDX * (PNX - 1), PNX, PDX * (PNY - 1), PNY, periodic_boundary=(True, True)), True)
    child = box(TwoDCartesianGridMesh(X0, X0 + CDX * (CNX - 1), CNX, Y0, Y0 + CDX * (CNY - 1), CNY, periodic_boundary=(False, False)), False)
    parent_sim = Simulation(parent, Δt=DT, stop_time=1e9)             # the parent's steps are counted from the child's
    child_sim = Simulation(child, Δt=DT / RATIO, stop_time=DT / RATIO * (n_child - 1))
    child_sim.output_writers["boundary_forcing"] = NestForcing(child, parent=parent_sim, side="rim", ratio=RATIO)
    child_sim.output_writers["checkpointer"] = Checkpointer(child, schedule=20, dir=ckdir, prefix="nest")
    return parent, child, child_sim


SIX_HOURS = 36 * RATIO
# the job that is stopped after three hours and a bit: 56 child steps, the last pair checkpoint at 40 — one step past a parent level
parent, child, sim = nested_pair(56, out_dir / "job")
run(sim)
found = list_checkpoints(out_dir / "job", "nest")
latest = found[max(found)]
print(f"stopped at child iteration {child.clock.iteration}; pair checkpoints at {sorted(found)}: {latest.name}, {parent_checkpoint_path(latest).name}, "
      f"{link_path(latest).name}")

# the program that continues: new models, the same script, pickup=True
parent2, child2, sim2 = nested_pair(SIX_HOURS, out_dir / "job")
run(sim2, pickup=True)
print(f"picked up at child iteration {max(found)}, ran on to {child2.clock.iteration} (parent: {parent2.clock.iteration} steps)")

# and the run nobody stopped
parent3, child3, sim3 = nested_pair(SIX_HOURS, out_dir / "whole")
run(sim3)
same = [np.array_equal(np.ascontiguousarray(a.State).view(np.uint64), np.ascontiguousarray(b.State).view(np.uint64))
        for a, b in ((child2, child3), (parent2, parent3))]
print(f"child equal to the uninterrupted run, bit for bit: {same[0]}; parent: {same[1]}; "
      f"child interior mean Hs {4 * np.sqrt(np.mean(np.asarray(child2.State)[1:-1, 1:-1, 0])):.3f} m; files in {out_dir}")
if not all(same):
    raise SystemExit("the picked-up pair differs from the uninterrupted run")
