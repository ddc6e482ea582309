"""Driver of tests/test_gpu_pull_class_ring.py (a fresh process with PICLES_CCL_LIB pointing at the loopback communicator): two slab
contexts on the one GPU, joined into the library's native ring, stepped ONE model step per call so that the class-path counters of
every rank can be read after every step (picles_get_pull_class_counts does not complete the pending step).  192 x 32 periodic box
under uniform winds, 16 rows per rank, halo of 2 rows, DP5 under static winds in the default PICLES_WAVEROW mode: the edge launch
(rows 0, 1, 14, 15: two row ranges) is k_step on one stream, the interior launch (rows 2 .. 13) k_step_waverow on the other.
Prints one JSON line: per rank and step the (class, EMPTY) wave counts, and the bitwise mismatches against the whole-grid context."""
import json
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from picles_amd import configs  # noqa: E402
from picles_amd.grids import TwoDCartesianGridMesh  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.parallel import SlabModel  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation  # noqa: E402

NX, NY, DX, WORLD = 192, 32, 2000.0, 2


def box():
    cfg = configs.bench06_box(n=8)
    cfg.model["grid"] = TwoDCartesianGridMesh(DX * (NX - 1), NX, DX * (NY - 1), NY, periodic_boundary=(True, True))
    return cfg


class _NoExchange:
    def start(self): raise RuntimeError("unused")
    def finish(self, w): raise RuntimeError("unused")


def main():
    steps = int(sys.argv[1])
    cfg0 = box()
    plain = WaveGrowth2D(**cfg0.model)
    initialize_simulation(Simulation(plain, Δt=cfg0.Δt, stop_time=1.0))
    plain.upload_winds(0.0, cfg0.Δt)
    plain.backend.run_steps(cfg0.Δt, steps)
    S = np.asarray(plain.State).copy()
    zp, onp, _, stp = plain.backend.get_particles()
    reach = plain.backend.get_counters()["max_reach_seen"]

    uid, out, errs = {}, [None] * WORLD, []
    bar = threading.Barrier(WORLD)

    def rank_main(rank):
        try:
            cfg = box()
            sm = SlabModel(cfg.model, rank, WORLD, device=0, halo_rows=2, native_ring=False, exchange=_NoExchange())
            b = sm.backend
            if rank == 0:
                uid["id"] = b.slab_unique_id()
            bar.wait()
            b.slab_comm_init(uid["id"], rank, WORLD)
            sm.native, sm.ex, sm.use_streams = True, None, False
            sm.seed()
            counts, last = [], (0, 0)
            for _ in range(steps):
                sm.run_steps(cfg.Δt, 1)
                now = b.get_pull_class_counts()
                counts.append([now[0] - last[0], now[1] - last[1]])
                last = now
            st = sm.get_state()
            z, on, _, status = b.get_particles()
            out[rank] = (sm.j0, sm.j1, st, z, on, status, counts)
            bar.wait()
            b.slab_comm_destroy()
        except BaseException as e:  # noqa: BLE001
            errs.append(f"rank {rank}: {e!r}")
            bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(WORLD)]
    for t in th: t.start()
    for t in th: t.join(timeout=300)
    if errs or any(t.is_alive() for t in th):
        print(json.dumps({"error": errs or "timeout"}))
        sys.exit(1)
    bad = 0
    for j0, j1, st, z, on, status, _ in out:
        bad += int((st.view(np.uint64) != np.ascontiguousarray(S[:, j0:j1]).view(np.uint64)).sum())
        bad += int((on != onp[:, j0:j1]).sum()) + int((status != stp[:, j0:j1]).sum())
        live = ((stp[:, j0:j1] & 1) == 1) & (onp[:, j0:j1] == 1)
        for k in range(5):
            bad += int((z[..., k][live].view(np.uint64) != zp[:, j0:j1, k][live].view(np.uint64)).sum())
    print(json.dumps({"mismatches": bad, "counts": [o[6] for o in out], "rows": [[o[0], o[1]] for o in out], "max_reach": int(reach),
                      "nonzero_state": int((S != 0).sum()), "state_crc": int(np.bitwise_xor.reduce(S.view(np.uint64).ravel()) & 0xffffffff)}))


if __name__ == "__main__":
    main()
