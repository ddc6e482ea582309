"""Cost of nests and chunked runs under a device-sampled wind lattice, and of a child started from its parent.
One JSON line on stdout; host wall time with a final synchronisation of the contexts involved, alternated rounds in one process
after un-timed conditioning steps.

default: the pair of scripts/nest_cost.py — parent the 1024^2 periodic bench06 box (dx = 2000 m, Δt = 600 s), child 1024^2 at a
quarter of the spacing (Δt = 150 s, ratio 4), whole rim forced — once under one wind lattice over the parent (65 x 65 x 1 h knots: a
vortex crossing the box in a (10, 10) m/s flow) on both models and once under static winds (the lattice at t = 0), per parent step:
  nested:  four child steps, parent step, picles_nest_sample;   parts: the parent alone, the child alone under a constant level
then picles_nest_prolong for that child: the call between two synchronisations, five times, under both kinds of wind.
--stations: config 5's box (2048^2, its forcing as a SMOOTH3 device lattice) with a StationWriter of 64 stations every step,
  run(sim) — chunked — against the per-step loop the same run took before lattices were chunked, ms per step, alternated.
--profile: a short nested run under the lattice and two picles_nest_prolong calls and nothing else, for
  `rocprofv3 --kernel-trace --stats -- python scripts/nest_lattice_cost.py --profile`."""
import json
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from picles_amd import configs, models
from picles_amd.boundary_forcing import rim_nodes
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import locate_in_parent, prolong_tables, rim_points
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter
from picles_amd.wind_emulator import IdealizedWindGrid, wind_interpolator

N, RATIO, DT, PDX = 1024, 4, 600.0, 2000.0
CDX, X0, Y0 = PDX / RATIO, 300.25 * PDX, 300.25 * PDX
STEPS, WARM, ROUNDS = 50, 5, 4          # parent steps per round, un-timed parent steps first, rounds
LP = N * PDX


def stations_leg():
    n_steps, rounds = 20, 4
    rows = {"chunked": [], "per_step": []}
    for r in range(rounds + 1):
        for leg in rows:
            cfg = configs.growing_decaying_winds_lattice(n=2048, n_steps=n_steps)
            m = models.WaveGrowth2D(**cfg.model)
            if leg == "per_step":
                m.runs_chunked = lambda *a, **k: False            # run()'s choice before lattices were chunked
            sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1))
            L = float(m.grid.data.x[-1, 0])
            pts = [(L * (0.52 + 0.45 * (k % 8) / 8), L * (0.05 + 0.9 * (k // 8) / 8)) for k in range(64)]
            with tempfile.TemporaryDirectory() as d:
                sim.output_writers["stations"] = StationWriter(m, points=pts, path=d, format="npy")
                initialize_simulation(sim)
                m.backend.sync()
                t0 = time.perf_counter()
                run(sim)
                ms = 1e3 * (time.perf_counter() - t0) / n_steps
            print(f"round {r}: {leg} {ms:.4f} ms per step", file=sys.stderr)
            if r:
                rows[leg].append(ms)
            m.backend.close()
    out = {"box": "config 5 at 2048^2, SMOOTH3 device lattice, 64 stations every step", "steps": n_steps, "unit": "ms per step (host wall time of run())"}
    out.update({k + "_ms": v for k, v in rows.items()})
    out.update({"median_" + k + "_ms": float(np.median(v)) for k, v in rows.items()})
    print(json.dumps(out))


if "--stations" in sys.argv:
    stations_leg()
    sys.exit(0)


def storm(x, y, t):
    T = DT * (WARM + (ROUNDS + 1) * STEPS + 8)
    xc, yc = 0.2 * LP + 0.6 * LP * t / T, 0.5 * LP
    ddx, ddy = (x - xc + 0.5 * LP) % LP - 0.5 * LP, (y - yc + 0.5 * LP) % LP - 0.5 * LP
    r = np.hypot(ddx, ddy) + 1.0
    vt = 6.0 * (r / 3e5) * np.exp(1.0 - r / 3e5)
    return -vt * ddy / r + 10.0, vt * ddx / r + 10.0


n_knots = int(np.ceil(DT * (WARM + (ROUNDS + 1) * STEPS + 8) / 3600.0)) + 1
LATTICE = wind_interpolator(IdealizedWindGrid(lambda x, y, t: storm(x, y, t)[0], lambda x, y, t: storm(x, y, t)[1],
                                              dict(Lx=LP, Ly=LP, T=3600.0 * n_knots), dict(dx=LP / 64, dy=LP / 64, dt=3600.0)))
STATIC = SimpleNamespace(u=lambda x, y, t: LATTICE.u(x, y, 0.0), v=lambda x, y, t: LATTICE.v(x, y, 0.0))


def model(kind, who):
    w = LATTICE if kind == "lattice" else STATIC
    if who == "parent":
        cfg = configs.bench06_box(n=N, dx=PDX)
        dt = DT
    else:
        cfg = configs.bench06_box(n=16, dx=CDX, periodic_grid=False)
        cfg.model["grid"] = TwoDCartesianGridMesh(X0, X0 + CDX * (N - 1), N, Y0, Y0 + CDX * (N - 1), N, periodic_boundary=(False, False))
        dt = DT / RATIO
    cfg.model["winds"] = w
    cfg.model["winds_static"] = kind != "lattice"
    cfg.model["ODEsys"] = particle_equations(w.u, w.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=True, dissipation=True)
    m = models.WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=dt, stop_time=1.0))
    m.upload_winds(0.0, dt)
    return m


def wall(fn, contexts, per=STEPS):
    for b in contexts:
        b.sync()
    t0 = time.perf_counter()
    fn()
    for b in contexts:
        b.sync()
    return 1e3 * (time.perf_counter() - t0) / per


def legs(kind):
    pa, ca = model(kind, "parent"), model(kind, "child")
    rim = rim_nodes(ca.grid, "rim")
    corner_nodes, index, weights = locate_in_parent(pa.grid, rim_points(ca, side="rim"))
    ca.backend.bforce_init(rim)
    ca.backend.nest_init(pa.backend, corner_nodes, index, weights)
    ca.backend.nest_sample()
    pa.backend.run_steps(DT, 1)
    ca.backend.nest_sample()

    def nested(n=STEPS):
        for _ in range(n):
            ca.backend.run_steps(DT / RATIO, RATIO)
            pa.backend.run_steps(DT, 1)
            ca.backend.nest_sample()

    nested(WARM)
    pb, cb = model(kind, "parent"), model(kind, "child")
    cb.backend.bforce_init(rim)
    cb.backend.bforce_set_levels(0.0, ca.backend.bforce_get_levels()[1])
    pb.backend.run_steps(DT, WARM + 1)
    cb.backend.run_steps(DT / RATIO, RATIO * WARM)
    return dict(nested=(nested, (pa.backend, ca.backend)), parent_alone=(lambda: pb.backend.run_steps(DT, STEPS), (pb.backend,)),
                child_alone=(lambda: cb.backend.run_steps(DT / RATIO, RATIO * STEPS), (cb.backend,))), (pa, ca)


if "--profile" in sys.argv:
    L, (pa, ca) = legs("lattice")
    L["nested"][0](10)
    tables = prolong_tables(pa.grid, ca.grid)
    ca.backend.nest_free(); ca.backend.bforce_free()
    for _ in range(2):
        ca.backend.nest_prolong(pa.backend, *tables, DT / RATIO)
    pa.backend.sync(); ca.backend.sync()
    sys.exit(0)

all_legs, pairs = {}, {}
for kind in ("lattice", "static"):
    all_legs[kind], pairs[kind] = legs(kind)
rows = {f"{kind}_{leg}": [] for kind in all_legs for leg in all_legs[kind]}
for r in range(ROUNDS + 1):              # round 0 conditions the clocks and is dropped
    line = []
    for kind in all_legs:
        for leg, (fn, ctx) in all_legs[kind].items():
            ms = wall(fn, ctx)
            line.append(f"{kind} {leg} {ms:.4f}")
            if r:
                rows[f"{kind}_{leg}"].append(ms)
    print(f"round {r}: " + "; ".join(line), file=sys.stderr)
out = {"n": N, "ratio": RATIO, "parent_steps_per_round": STEPS, "lattice": [65, 65, n_knots + 1], "lattice_time_spacing_s": 3600.0,
       "unit": "ms per parent step (host wall time)"}
out.update({k + "_ms": v for k, v in rows.items()})
out.update({"median_" + k + "_ms": float(np.median(v)) for k, v in rows.items()})
for kind in all_legs:
    out[f"median_{kind}_parts_sum_ms"] = out[f"median_{kind}_parent_alone_ms"] + out[f"median_{kind}_child_alone_ms"]
# picles_nest_prolong for that child: the call between two synchronisations
for kind, (pa, ca) in pairs.items():
    tables = prolong_tables(pa.grid, ca.grid)
    ca.backend.nest_free(); ca.backend.bforce_free()
    out[f"prolong_{kind}_ms"] = [wall(lambda: ca.backend.nest_prolong(pa.backend, *tables, DT / RATIO), (pa.backend, ca.backend), per=1) for _ in range(5)]
    S = ca.backend.get_state()
    out[f"prolong_{kind}_zeroed_nodes"] = int((S == 0.0).all(axis=-1).sum())
print(json.dumps(out))
