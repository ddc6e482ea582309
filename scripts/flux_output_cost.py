"""Cost of the coupling fluxes on the BASELINE box: the k_flux kernel beside k_diag at the same coarsening, and the
wall time of run(sim) with a FluxWriter against the same run without one.

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/flux_output_cost.py --kernel-only     # the kernels, one trace
    python scripts/flux_output_cost.py [--n 4096] [--rounds 5] [--out profiles/flux_output_cost.json]  # the writer

--kernel-only: two contexts, coarsening (4,4) and (1,1), each with a diagnostics set (four planes, as §12 measured it) and a flux set
(nine planes); a few steps, then `--launches` times k_diag and k_flux on each.  The default mode alternates run(sim) over 100 steps
with and without a FluxWriter(schedule=10, coarsen=(4, 4), format="npy") after bench.py-style clock conditioning, and prints one
JSON document."""
import argparse
import json
import math
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from picles_amd import _capi as K, configs  # noqa: E402
from picles_amd.flux_output import FluxWriter  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation, run  # noqa: E402

DIAG_FIELDS = ("hs", "tp", "cg_x", "cg_y")


def make(n):
    cfg = configs.box4096(n=n)
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    m.upload_winds(0.0, cfg.Δt)
    return m, cfg.Δt


def kernel_only(n, launches):
    for pair in ((4, 4), (1, 1)):
        m, dt = make(n)
        b = m.backend
        b.diag_init(pair, DIAG_FIELDS, 1)
        b.flux_init(pair, K.FLUX_FIELDS, 1025.0 * 9.81, 1025.0, 1)
        b.run_steps(dt, 5)
        for _ in range(launches):
            b.diag_push(); b.diag_pop()
            b.flux_push(); b.flux_pop()
        b.close()
    print(json.dumps({"launches_per_pair": launches, "grid": [n, n]}))


def timed(m, dt, steps, writer):
    """wall time [ms] of run(sim) over `steps` steps from a fresh seed, ending in a sync"""
    sim = Simulation(m, Δt=dt, stop_time=dt * (steps - 1))
    if writer is not None:
        sim.output_writers["fluxes"] = writer
    m.backend.sync()
    t0 = time.perf_counter()
    run(sim)
    m.backend.sync()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--prewarm-ms", type=float, default=1500.0)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "flux_output_cost.json"))
    a = ap.parse_args()
    if a.kernel_only:
        kernel_only(a.n, a.launches)
        return
    m, dt = make(a.n)
    b = m.backend
    # clock conditioning as bench.py: the same steps, un-timed, in cycles of at most 40 with a re-seed after each
    left = int(min(4000, max(5, math.ceil(a.prewarm_ms * 1e-3 * 6.5e9 / b.N))))
    while left > 0:
        b.run_steps(dt, min(left, 40))
        left -= 40
        b.seed(0.0)
    runs = {"a_no_writer": [], "b_flux_writer_4x4": []}
    with tempfile.TemporaryDirectory() as tmp:
        fw = FluxWriter(m, schedule=a.every, path=tmp, coarsen=(4, 4), format="npy")
        timed(m, dt, a.every, fw)              # un-timed: the ring's set-up and the first launch of the kernel
        for _ in range(a.rounds):
            runs["a_no_writer"].append(timed(m, dt, a.steps, None))
            runs["b_flux_writer_4x4"].append(timed(m, dt, a.steps, fw))
    med = {k: statistics.median(v) for k, v in runs.items()}
    outputs = a.steps // a.every + 1
    shape = b.flux_shape()
    out = {"grid": [a.n, a.n], "steps_per_run": a.steps, "outputs_per_run": outputs, "rounds": a.rounds,
           "bytes_per_output": shape[4] + shape[3] * 88,
           "wall_ms": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in runs.items()},
           "added_ms_per_output": (med["b_flux_writer_4x4"] - med["a_no_writer"]) / outputs}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
