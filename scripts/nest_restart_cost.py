"""Cost of a pair checkpoint and of a resume on §18's pair.  Parent: the 1024^2 periodic bench06 box (dx = 2000 m,
Δt = 600 s).  Child: 1024^2 at a quarter of the spacing (dx = 500 m, Δt = 150 s, ratio 4), its whole rim forced (4092 nodes).
run(child_sim) with a NestForcing and Checkpointer(schedule=6) over 18 child steps: three pair checkpoints, at child iteration 6 (the
first of the contexts: the snapshot buffers are allocated; a chunk of 2 child steps runs behind it), 12 (a chunk of 4 child steps and
a parent step behind it) and 18 (the run's last iteration: nothing behind it).  Host wall time from the entry of Checkpointer.begin
to the link side-car's rename — the child's snapshot, the parent's, the pair read back, whatever the loop did in between, the two
blobs fetched and the three files written to --dir (default: a temporary directory).  Then two new models pick the pair up from
iteration 12: wall time from the entry of run(child_sim, pickup=...) to the child's first picles_run_steps — three files read,
two blobs loaded, the set and the nest made, the pair put back — and the picked-up run's final State held against the
uninterrupted run's.  One process, one pass, no repetition: these are orders of magnitude, not a benchmark.  One JSON line on stdout."""
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from picles_amd import configs, models
from picles_amd.checkpointing import Checkpointer, checkpoint_path
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import NestForcing, link_path, parent_checkpoint_path
from picles_amd.simulations import Simulation, run

N, RATIO, DT, PDX = 1024, 4, 600.0, 2000.0
CDX, X0, Y0 = PDX / RATIO, 300.25 * PDX, 300.25 * PDX
N_CHILD, EVERY, PICK = 18, 6, 12


def pair(ckdir):
    pm = models.WaveGrowth2D(**configs.bench06_box(n=N, dx=PDX).model)
    cfg = configs.bench06_box(n=16, dx=CDX, periodic_grid=False)
    cfg.model["grid"] = TwoDCartesianGridMesh(X0, X0 + CDX * (N - 1), N, Y0, Y0 + CDX * (N - 1), N, periodic_boundary=(False, False))
    cm = models.WaveGrowth2D(**cfg.model)
    psim = Simulation(pm, Δt=DT, stop_time=1e9)
    csim = Simulation(cm, Δt=DT / RATIO, stop_time=(N_CHILD - 1) * DT / RATIO)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=RATIO)
    ck = csim.output_writers["checkpointer"] = Checkpointer(cm, schedule=EVERY, dir=ckdir, prefix="pair")
    return pm, cm, csim, f, ck


def main():
    given = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--dir=")]
    with tempfile.TemporaryDirectory(dir=given[0] if given else None) as d:
        pm, cm, csim, f, ck = pair(d)
        began, spans = {}, []
        ck_begin, pair_finish = ck.begin, f._pair_finish

        def begin(backend, time_, iteration):
            began["t"], began["it"] = time.perf_counter(), int(iteration)
            ck_begin(backend, time_, iteration)

        def finish():
            busy = f._pair is not None
            pair_finish()
            if busy:
                spans.append({"child_iteration": began["it"], "ms": 1e3 * (time.perf_counter() - began["t"])})

        ck.begin, f._pair_finish = begin, finish
        run(csim)
        S = np.ascontiguousarray(cm.backend.get_state())
        cf = checkpoint_path(d, "pair", PICK)
        sizes = {"child_file": cf.stat().st_size, "parent_file": parent_checkpoint_path(cf).stat().st_size, "link_side_car": link_path(cf).stat().st_size}

        pm2, cm2, csim2, f2, _ = pair(Path(d) / "again")
        first, steps = {}, cm2.backend.run_steps

        def run_steps(dt, n):
            if not first:
                pm2.backend.sync(); cm2.backend.sync()
                first["t"] = time.perf_counter()
            steps(dt, n)

        cm2.backend.run_steps = run_steps
        t0 = time.perf_counter()
        run(csim2, pickup=cf)
        out = {"pair": f"{N}^2 parent, {N}^2 child, ratio {RATIO}, {len(f.nodes)} forced nodes", "checkpoints": spans, "bytes": sizes,
               "resume_ms": 1e3 * (first["t"] - t0), "resumed_at_child_iteration": PICK,
               "final_state_equal_to_uninterrupted": bool(np.array_equal(np.ascontiguousarray(cm2.backend.get_state()).view(np.uint64), S.view(np.uint64)))}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
