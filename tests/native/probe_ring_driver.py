"""Driver of tests/test_gpu_probe_slabs.py (run as a fresh process with PICLES_CCL_LIB pointing at the loopback communicator):
`world` threads, one slab context each on the one GPU, joined into the library's NATIVE ring (picles_slab_run_steps), every rank
probing the nodes of its own rows — first and last owned row of every slab among them, which ghost records feed.  Prints one JSON
line: the bitwise mismatch count of the gathered samples against a whole-grid context's samples and against its State."""
import json
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from picles_amd.parallel import SlabModel, assemble_probes, slab_rows  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation  # noqa: E402
from picles_amd.timesteppers import time_step  # noqa: E402
from picles_amd.wind_emulator import GriddedWinds  # noqa: E402
from loopback_ring_driver import _NoExchange, box  # noqa: E402


def slab_nodes(Nx, Ny, world, seed=7):
    """60 random nodes + for every slab of the decomposition a spread of columns in its first two and last two rows"""
    rng = np.random.default_rng(seed)
    nodes = [(int(rng.integers(Nx)), int(rng.integers(Ny))) for _ in range(60)]
    for r in range(world):
        j0, j1 = slab_rows(Ny, world, r)
        for j in (j0, j0 + 1, j1 - 2, j1 - 1):
            nodes += [(int(i), j) for i in (0, 1, Nx // 3, Nx // 2 + 1, Nx - 2, Nx - 1)]
    return np.array(nodes, dtype=np.int64)


def main():
    world, case, solver, steps = int(sys.argv[1]), sys.argv[2], sys.argv[3], int(sys.argv[4])
    chunks = [int(c) for c in sys.argv[5].split(",")]
    every, first, halo = int(sys.argv[6]), int(sys.argv[7]), int(sys.argv[8])
    assert sum(chunks) == steps
    cfg0 = box(case, solver)
    g = cfg0.model["grid"]
    Nx, Ny = int(g.stats.Nx), int(g.stats.Ny)
    nodes = slab_nodes(Nx, Ny, world)
    due = [s for s in range(1, steps + 1) if s >= first and (s - first) % every == 0]
    plain = WaveGrowth2D(**cfg0.model)
    initialize_simulation(Simulation(plain, Δt=cfg0.Δt, stop_time=1.0))
    plain.backend.probe_init(nodes, every=every, first=first, capacity=len(due) + 1)
    plain.backend.probe_sample()
    states = []
    for _ in range(steps):                      # observed after every step: the unfused twin
        time_step(plain, cfg0.Δt, zero_first=True)
        states.append(plain.backend.get_state())
    want = plain.backend.probe_pop()

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
            sm.probe_init(nodes, every=every, first=first, capacity=len(due) + 1)
            sm.probe_sample()
            for c in chunks:
                sm.run_steps(cfg.Δt, c)
            out[rank] = sm.pop_probes()
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
    v, t, s = assemble_probes(len(nodes), out)
    bad = int((v.view(np.uint64) != want[0].view(np.uint64)).sum()) if v.shape == want[0].shape else -1
    for k, step in enumerate(s):
        if step > 0:
            ref = np.ascontiguousarray(states[step - 1][nodes[:, 0], nodes[:, 1], :].T)
            bad += int((v[k].view(np.uint64) != ref.view(np.uint64)).sum())
    print(json.dumps({"world": world, "case": case, "mismatches": bad, "steps": [int(x) for x in s], "want_steps": [0] + due,
                      "times_equal": bool(np.array_equal(t, want[1])), "wet_share": float((v[-1][0] > 0).mean()),
                      "ranks_with_nodes": sum(1 for q in out if len(q[0]))}))


if __name__ == "__main__":
    main()
