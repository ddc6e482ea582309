"""Driver of tests/test_gpu_run_stats_ring.py (run as a fresh process with PICLES_CCL_LIB pointing at the loopback communicator):
`world` threads, one slab context each on the one GPU, joined into the library's NATIVE ring (picles_slab_run_steps), every rank
holding a statistics set over its own rows — the update of a fused step runs on the ring's side stream behind the interior launch
and the delivered exchange.  Prints one JSON line: how many planes of the rank-ordered concatenation differ from
tests/_stats_numpy.py applied to the States of a whole-grid twin observed after every step."""
import json
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

import _stats_numpy as SN  # noqa: E402
from picles_amd.driver import stat_concat  # noqa: E402
from picles_amd.parallel import SlabModel  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation  # noqa: E402
from picles_amd.timesteppers import time_step  # noqa: E402
from loopback_ring_driver import _NoExchange, box  # noqa: E402


def main():
    world, case, solver, steps = int(sys.argv[1]), sys.argv[2], sys.argv[3], int(sys.argv[4])
    chunks = [int(c) for c in sys.argv[5].split(",")]
    every, first, halo = int(sys.argv[6]), int(sys.argv[7]), int(sys.argv[8])
    assert sum(chunks) == steps
    cfg0 = box(case, solver)
    due = [s for s in range(1, steps + 1) if s >= first and (s - first) % every == 0]
    plain = WaveGrowth2D(**cfg0.model)
    initialize_simulation(Simulation(plain, Δt=cfg0.Δt, stop_time=1.0))
    twin = []
    for _ in range(steps):                      # observed after every step: the unfused twin
        time_step(plain, cfg0.Δt, zero_first=True)
        twin.append((plain.backend.get_state(), plain.backend.clock))
    e = twin[-1][0][..., 0]
    thr = tuple(float(x) for x in np.quantile(4.0 * np.sqrt(e[e > 0]), [0.25, 0.5, 0.75]))
    want = SN.accumulate([twin[s - 1] for s in due], 7, thr)

    uid, out, errs = {}, [None] * world, []
    bar = threading.Barrier(world)

    def rank_main(rank):
        try:
            cfg = box(case, solver)
            sm = SlabModel(cfg.model, rank, world, device=0, halo_rows=halo, native_ring=False, exchange=_NoExchange())
            b = sm.backend
            if rank == 0:
                uid["id"] = b.slab_unique_id()
            bar.wait()
            b.slab_comm_init(uid["id"], rank, world)
            sm.native, sm.ex, sm.use_streams = True, None, False
            sm.seed()
            sm.stat_init(7, thr, every=every, first=first)
            for c in chunks:
                sm.run_steps(cfg.Δt, c)
            out[rank] = sm.stat_get()
            bar.wait()
            b.slab_comm_destroy()
        except BaseException as e:  # noqa: BLE001
            errs.append(f"rank {rank}: {e!r}")
            bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th: t.start()
    for t in th: t.join(timeout=600)
    if errs or any(t.is_alive() for t in th):
        print(json.dumps({"error": errs or "timeout"}))
        sys.exit(1)
    got = stat_concat(out)
    bad = [n for n in SN.plane_names(7) if np.ascontiguousarray(got[n]).tobytes() != np.ascontiguousarray(want[n]).tobytes()]
    print(json.dumps({"world": world, "case": case, "planes_that_differ": bad, "n_samples": [int(o["n_samples"]) for o in out],
                      "want_samples": len(due), "t_first": [o["t_first"] for o in out], "t_last": [o["t_last"] for o in out],
                      "want_t": [want["t_first"], want["t_last"]], "wet_share": float((got["n_wet"] > 0).mean()),
                      "exceeding_share": float((got["n_exc"][..., 1] > 0).mean())}))


if __name__ == "__main__":
    main()
