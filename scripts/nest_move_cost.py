"""Cost of a moving nest.  One JSON line on stdout; host wall time between synchronisations of both contexts.

default: the pair of scripts/nest_cost.py (§18) under static winds — parent the 1024^2 periodic bench06 box (dx = 2000 m, Δt = 600 s),
child 1024^2 at a quarter of the spacing (Δt = 150 s, ratio 4):
  one move:   picles_nest_relocate (shift (8, 4), margin 1) between two synchronisations, five times; picles_nest_prolong on the same
              pair in the same session, five times; one child step, five times
  in a run:   host wall time per parent step of `run_following(every=1)` whose centre jumps 8 child nodes to and fro (a move behind
              every parent step) against one whose centre stands still (the same legs, no move) and against one plain nested
              `run()` of as many parent steps; four alternated rounds after one that is dropped
--differ:   a child at the parent's spacing (48 x 48 in a 128 x 128 periodic box at 2 km, ratio 1, band of width 3) moved one node
            east behind every step for ten steps, against the same child standing still: the largest relative difference in e
            between each and the parent at the same nodes, outside the band
--profile:  four picles_nest_relocate calls and two picles_nest_prolong calls on the 1024^2 pair and nothing else, for
            `rocprofv3 --kernel-trace --stats -- python scripts/nest_move_cost.py --profile`."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from picles_amd import configs, models
from picles_amd.grids import TwoDCartesianGridMesh, translated
from picles_amd.nesting import NestForcing, prolong_tables, run_following, start_from_parent
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, run

N, RATIO, DT, PDX = 1024, 4, 600.0, 2000.0
CDX, X0, Y0 = PDX / RATIO, 300.25 * PDX, 300.25 * PDX
STEPS, ROUNDS = 8, 4                    # parent steps per round, rounds


def model(grid, periodic, dx, winds):
    cfg = configs.bench06_box(n=16, dx=dx, periodic_grid=periodic)
    cfg.model["grid"] = grid
    cfg.model["winds"] = winds
    cfg.model["winds_static"] = True
    cfg.model["ODEsys"] = particle_equations(winds.u, winds.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=True, dissipation=True)
    return models.WaveGrowth2D(**cfg.model)


def pair(n_par=N, n_child=N, cdx=CDX, x0=X0, y0=Y0, ratio=RATIO, spin=2):
    """a parent spun up `spin` steps and a child started from it, under smooth static winds of the parent's period"""
    winds = configs.smooth_winds(10.0, 10.0, n_par * PDX, n_par * PDX)
    pm = model(TwoDCartesianGridMesh(PDX * (n_par - 1), n_par, PDX * (n_par - 1), n_par, periodic_boundary=(True, True)), True, PDX, winds)
    cm = model(TwoDCartesianGridMesh(x0, x0 + cdx * (n_child - 1), n_child, y0, y0 + cdx * (n_child - 1), n_child, periodic_boundary=(False, False)), False, cdx, winds)
    psim, csim = Simulation(pm, Δt=DT, stop_time=DT * (spin - 1)), Simulation(cm, Δt=DT / ratio, stop_time=0.0)
    run(psim)
    psim.stop_time = 1e12
    start_from_parent(csim, psim)
    return pm, psim, cm, csim


def wall(fn, contexts, per=1):
    for b in contexts:
        b.sync()
    t0 = time.perf_counter()
    fn()
    for b in contexts:
        b.sync()
    return 1e3 * (time.perf_counter() - t0) / per


def box_centre(g):
    return 0.5 * (g.stats.xmin + g.stats.xmax), 0.5 * (g.stats.ymin + g.stats.ymax)


if "--differ" in sys.argv:
    n_par, n_child, steps, width = 128, 48, 10, 3
    out = {"parent": f"{n_par}^2 periodic at {PDX:.0f} m", "child": f"{n_child}^2 at the parent's spacing, on its nodes, ratio 1, band width {width}", "steps": steps}
    for kind, drift in (("moved_one_node_per_step", 1.0), ("standing", 0.0)):
        pm, psim, cm, csim = pair(n_par, n_child, PDX, 20 * PDX, 40 * PDX, 1, spin=6)
        c0, t0 = box_centre(cm.grid), pm.clock.time
        boxes = run_following(csim, psim, lambda t: (c0[0] + drift * PDX * (t - t0) / DT, c0[1]), stop_time=t0 + steps * DT,
                              nest=dict(side="rim", ratio=1, width=width))
        i0, j0 = int(round(boxes[-1][1] / PDX)), int(round(boxes[-1][2] / PDX))
        Sc, Sp = cm.backend.get_state(), pm.backend.get_state()[i0:i0 + n_child, j0:j0 + n_child]
        inner = (slice(width, n_child - width),) * 2
        rel = np.abs(Sc[inner][..., 0] - Sp[inner][..., 0]) / Sp[inner][..., 0]
        out[kind] = {"moves": sum(a[1:] != b[1:] for a, b in zip(boxes, boxes[1:])), "max_rel_diff_e": float(rel.max()), "median_rel_diff_e": float(np.median(rel))}
    print(json.dumps(out))
    sys.exit(0)

pm, psim, cm, csim = pair()
pb, cb = pm.backend, cm.backend
both = (pb, cb)
tables_here = prolong_tables(pm.grid, cm.grid)
tables_there = prolong_tables(pm.grid, translated(cm.grid, 8, 4))

if "--profile" in sys.argv:
    for k in range(4):                  # to and fro: the tables of the place the box goes to
        s = 1 if k % 2 == 0 else -1
        cb.nest_relocate(pb, 8 * s, 4 * s, 1, *(tables_there if s > 0 else tables_here), DT / RATIO)
    for _ in range(2):
        cb.nest_prolong(pb, *tables_here, DT / RATIO)
    pb.sync(); cb.sync()
    sys.exit(0)

out = {"n": N, "ratio": RATIO, "unit": "ms (host wall time between synchronisations)"}
cb.run_steps(DT / RATIO, 2)             # conditioning; the child's clock leaves the parent's, so it is put back by a prolong
cb.nest_prolong(pb, *tables_here, DT / RATIO)
moves, prolongs, steps = [], [], []
for k in range(5):
    moves.append(wall(lambda: cb.nest_relocate(pb, 8, 4, 1, *tables_there, DT / RATIO), both))
    moves.append(wall(lambda: cb.nest_relocate(pb, -8, -4, 1, *tables_here, DT / RATIO), both))
    prolongs.append(wall(lambda: cb.nest_prolong(pb, *tables_here, DT / RATIO), both))
out["relocate_ms"], out["prolong_ms"] = moves, prolongs
for k in range(5):
    steps.append(wall(lambda: cb.run_steps(DT / RATIO, 1), both))
out["child_step_ms"] = steps
out.update({f"median_{k}_ms": float(np.median(out[f"{k}_ms"])) for k in ("relocate", "prolong", "child_step")})
pb.close(); cb.close()

# inside a run: a move behind every parent step, against the same legs without one, against one plain nested run
pm, psim, cm, csim = pair()
c0 = box_centre(cm.grid)
nest = dict(side="rim", ratio=RATIO)
flip = [0]


def to_and_fro(t):
    flip[0] ^= 1
    return c0[0] + 8 * CDX * flip[0], c0[1]


def plain():
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, **nest)
    csim.stop_time = cm.clock.time + (STEPS * RATIO - 0.5) * DT / RATIO
    run(csim)


legs = {"moving": lambda: run_following(csim, psim, to_and_fro, stop_time=cm.clock.time + STEPS * DT, nest=nest),
        "standing": lambda: run_following(csim, psim, lambda t: box_centre(cm.grid), stop_time=cm.clock.time + STEPS * DT, nest=nest),
        "plain_run": plain}
rows = {k: [] for k in legs}
for r in range(ROUNDS + 1):             # round 0 conditions and is dropped
    for k, fn in legs.items():
        ms = wall(fn, (pm.backend, cm.backend), per=STEPS)
        if r:
            rows[k].append(ms)
    print(f"round {r}: " + "; ".join(f"{k} {v[-1]:.3f}" for k, v in rows.items() if v), file=sys.stderr)
out["run_parent_steps_per_round"] = STEPS
out.update({f"run_{k}_ms_per_parent_step": v for k, v in rows.items()})
out.update({f"median_run_{k}_ms_per_parent_step": float(np.median(v)) for k, v in rows.items()})
print(json.dumps(out))
