"""Cost of exact restart on the BASELINE box: bytes per checkpoint, the pack kernel, begin -> end wall time, and the
ms/step of a run with a checkpoint every `--every` steps against one without, alternated, after bench.py-style clock conditioning.

    python scripts/checkpoint_cost.py [--n 4096] [--steps 200] [--every 50] [--pairs 2]

Prints one JSON line.  The pack kernel's time here comes from the library's own HIP events (picles_enable_timing: `other_ms`);
a `rocprofv3 --kernel-trace --stats -- python scripts/checkpoint_cost.py --pack-only` run gives the trace's view of k_ckpt."""
import argparse
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from picles_amd import configs  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--prewarm-ms", type=float, default=1500.0)
    ap.add_argument("--pack-only", action="store_true", help="seed, a few steps, three checkpoints: for a kernel trace")
    a = ap.parse_args()
    cfg = configs.box4096(n=a.n)
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    m.upload_winds(0.0, cfg.Δt)
    b, dt, N = m.backend, cfg.Δt, m.backend.N
    nbytes = b.checkpoint_size()
    if a.pack_only:
        b.run_steps(dt, 5)
        for _ in range(3):
            b.checkpoint_begin()
            b.checkpoint_end()
        print(json.dumps({"bytes": nbytes}))
        return
    # clock conditioning as bench.py: the same steps, un-timed, in cycles of at most 40 with a re-seed after each
    left = int(min(4000, max(5, math.ceil(a.prewarm_ms * 1e-3 * 6.5e9 / N))))
    while left > 0:
        b.run_steps(dt, min(left, 40))
        left -= 40
        b.seed(0.0)
    b.run_steps(dt, 5)
    # begin -> end of one checkpoint with nothing behind it; the pack kernel from the library's events
    b.sync()
    b.enable_timing(1)
    t0 = time.perf_counter()
    b.checkpoint_begin()
    t1 = time.perf_counter()
    blob = b.checkpoint_end()
    t2 = time.perf_counter()
    pack_ms = b.get_timing()["other_ms"]
    b.enable_timing(0)
    assert blob.size == nbytes

    def leg(with_ckpt):
        b.seed(0.0)
        b.run_steps(dt, 5)
        b.sync()
        t0 = time.perf_counter()
        inflight = False
        done = 0
        end_s = 0.0
        while done < a.steps:
            k = min(a.every, a.steps - done)
            b.run_steps(dt, k)
            if inflight:
                te = time.perf_counter()
                b.checkpoint_end()           # its copy-out ran beside the chunk just enqueued
                end_s += time.perf_counter() - te
                inflight = False
            done += k
            if with_ckpt and done < a.steps:
                b.checkpoint_begin()
                inflight = True
        if inflight:
            b.checkpoint_end()
        b.sync()
        return 1e3 * (time.perf_counter() - t0) / a.steps, 1e3 * end_s
    rows = []
    for _ in range(a.pairs):
        off, _e = leg(False)
        on, end_ms = leg(True)
        rows.append({"none_ms_per_step": off, "ckpt_ms_per_step": on, "end_ms_in_loop": end_ms})
    none = float(np.median([r["none_ms_per_step"] for r in rows]))
    ck = float(np.median([r["ckpt_ms_per_step"] for r in rows]))
    print(json.dumps({"n": a.n, "particles": N, "bytes_per_checkpoint": nbytes, "bytes_per_particle": nbytes / N,
                      "pack_kernel_ms_events": pack_ms, "begin_ms": 1e3 * (t1 - t0), "begin_to_end_ms": 1e3 * (t2 - t0),
                      "steps": a.steps, "every": a.every, "pairs": rows, "median_none_ms_per_step": none, "median_ckpt_ms_per_step": ck,
                      "ckpt_overhead_per_checkpoint_ms": (ck - none) * a.steps / max(1, (a.steps - 1) // a.every)}))


if __name__ == "__main__":
    main()
