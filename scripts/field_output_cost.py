"""Cost of device-side wave diagnostics on the BASELINE box: the k_diag kernel, and the wall time of a run that
takes an output every ten steps — none, the State ring (picles_store_*), coarse fields (picles_diag_*) at (4,4) and at (1,1) —
alternated in one process after bench.py-style clock conditioning.

    python scripts/field_output_cost.py [--n 4096] [--rounds 5] [--out profiles/field_output_cost.json]

Writes one JSON document (and prints it).  The kernel's time here comes from the library's own HIP events (picles_enable_timing:
`other_ms` around each k_diag launch); `rocprofv3 --kernel-trace --stats -- python scripts/field_output_cost.py --kernel-only`
gives the trace's view of the same launches."""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from picles_amd import configs  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation  # noqa: E402

FIELDS = ("hs", "tp", "cg_x", "cg_y")


def make(n):
    cfg = configs.box4096(n=n)
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    m.upload_winds(0.0, cfg.Δt)
    return m, cfg.Δt


def kernel_ms(b, launches):
    """mean device time of one k_diag launch, from the library's events around it"""
    b.diag_push()            # un-timed: the first launch of a kernel carries the runtime's one-off set-up between the two events
    b.diag_pop()
    b.sync()
    b.enable_timing(1)
    for _ in range(launches):
        b.diag_push()
        b.diag_pop()
    t = b.get_timing()
    b.enable_timing(0)
    return t["other_ms"] / launches


def timed_run(b, dt, chunks, per_chunk, mode, slots):
    """wall time [ms], ending in a sync, of chunks x run_steps(per_chunk) from a fresh seed with an output after every chunk"""
    b.seed(0.0)
    b.sync()
    t0 = time.perf_counter()
    for _ in range(chunks):
        b.run_steps(dt, per_chunk)
        if mode == "store":
            if b.store_pending == slots:
                b.store_pop()
            b.store_push()
        elif mode == "diag":
            if b.diag_pending == slots:
                b.diag_pop()
            b.diag_push()
    if mode == "store":
        while b.store_pending:
            b.store_pop()
    elif mode == "diag":
        while b.diag_pending:
            b.diag_pop()
    b.sync()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=10)
    ap.add_argument("--per-chunk", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--prewarm-ms", type=float, default=1500.0)
    ap.add_argument("--kernel-only", action="store_true", help="seed, a few steps, the k_diag launches of both factor pairs: for a kernel trace")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "field_output_cost.json"))
    a = ap.parse_args()
    slots = 3
    # a ring is set up once per context: one context carries the State ring and the (4,4) diagnostics, a second one the (1,1)
    m4, dt = make(a.n)
    m1, _ = make(a.n)
    b4, b1 = m4.backend, m1.backend
    b4.store_init(slots)
    b4.diag_init((4, 4), FIELDS, slots)
    b1.diag_init((1, 1), FIELDS, slots)
    N = b4.N
    shape4, shape1 = b4.diag_shape(), b1.diag_shape()
    for b in (b4, b1):
        b.run_steps(dt, 5)
    if a.kernel_only:
        for b in (b4, b1):
            for _ in range(a.launches):
                b.diag_push()
                b.diag_pop()
        print(json.dumps({"launches_per_pair": a.launches}))
        return
    # clock conditioning as bench.py: the same steps, un-timed, in cycles of at most 40 with a re-seed after each
    left = int(min(4000, max(5, math.ceil(a.prewarm_ms * 1e-3 * 6.5e9 / N))))
    while left > 0:
        b4.run_steps(dt, min(left, 40))
        left -= 40
        b4.seed(0.0)
    b4.run_steps(dt, 5)
    read_bytes = 24 * N
    k4, k1 = kernel_ms(b4, a.launches), kernel_ms(b1, a.launches)
    variants = {"a_no_output": (b4, None), "b_state_ring": (b4, "store"), "c_diag_4x4": (b4, "diag"), "d_diag_1x1": (b1, "diag")}
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, (b, mode) in variants.items():
            runs[name].append(timed_run(b, dt, a.chunks, a.per_chunk, mode, slots))
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {
        "grid": [a.n, a.n], "steps_per_run": a.chunks * a.per_chunk, "outputs_per_run": a.chunks, "rounds": a.rounds, "ring_slots": slots,
        "fields": list(FIELDS),
        "bytes_per_output": {"state_snapshot": 24 * N, "diag_4x4": shape4[4] + shape4[3] * 56, "diag_1x1": shape1[4] + shape1[3] * 56},
        "k_diag": {
            "launches": a.launches, "state_bytes_read": read_bytes,
            "4x4": {"device_ms": k4, "read_GBps": read_bytes / (k4 * 1e-3) / 1e9},
            "1x1": {"device_ms": k1, "read_GBps": read_bytes / (k1 * 1e-3) / 1e9},
        },
        "wall_ms": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in runs.items()},
        "added_ms_per_output": {k: (med[k] - med["a_no_output"]) / a.chunks for k in variants if k != "a_no_output"},
        "diag_4x4_share_of_state_ring_cost": (med["c_diag_4x4"] - med["a_no_output"]) / (med["b_state_ring"] - med["a_no_output"]),
    }
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
