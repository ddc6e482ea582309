"""Driver of tests/test_gpu_checkpoint.py::test_native_ring_over_the_loopback_communicator (a fresh process with PICLES_CCL_LIB
pointing at the loopback communicator): `world` threads, one slab context each, joined into the library's native ring; k steps,
every rank checkpoints (after growing its halo by one row), a NEW set of ranks joins a new ring and loads, N - k steps.  Prints one
JSON line: the mismatch count against the single whole-grid context and the halo rows of the new ranks."""
import json
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from picles_amd import configs  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.parallel import SlabModel  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation  # noqa: E402


def cfg():
    n, dx = 64, 1500.0
    P = n * dx
    return configs.bench06_box(n=n, dx=dx, winds=configs.smooth_winds(10.0, 7.0, P, P))


class _NoExchange:
    def start(self): raise RuntimeError("unused")
    def finish(self, w): raise RuntimeError("unused")


def main():
    world, N, k = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    c0 = cfg()
    plain = WaveGrowth2D(**c0.model)
    initialize_simulation(Simulation(plain, Δt=c0.Δt, stop_time=1.0))
    plain.upload_winds(0.0, c0.Δt)
    plain.backend.run_steps(c0.Δt, N)
    S = plain.backend.get_state()
    zp, onp, _, stp = plain.backend.get_particles()

    uid, blobs, out, errs = {}, [None] * world, [None] * world, []
    bar = threading.Barrier(world)

    def ring(rank, key):
        sm = SlabModel(cfg().model, rank, world, device=0, halo_rows=2, native_ring=False, exchange=_NoExchange())
        b = sm.backend
        if rank == 0:
            uid[key] = b.slab_unique_id()
        bar.wait()
        b.slab_comm_init(uid[key], rank, world)
        sm.native, sm.ex, sm.use_streams = True, None, False
        return sm

    def rank_main(rank):
        try:
            sm = ring(rank, "a")
            sm.seed()
            sm.run_steps(c0.Δt, k)
            sm.sync()
            sm.backend.set_halo_rows(3)               # a halo grown during the run, on every rank
            sm.checkpoint_begin()
            blobs[rank] = (sm.checkpoint_end(), sm.clock)
            bar.wait()
            sm.backend.slab_comm_destroy()
            sm2 = ring(rank, "b")
            sm2.checkpoint_load(*blobs[rank])
            sm2.run_steps(c0.Δt, N - k)
            st = sm2.get_state()
            z, on, _, status = sm2.backend.get_particles()
            out[rank] = (sm2.j0, sm2.j1, st, z, on, status, sm2.backend.halo_rows)
            bar.wait()
            sm2.backend.slab_comm_destroy()
        except BaseException as e:  # noqa: BLE001
            errs.append(f"rank {rank}: {e!r}")
            bar.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in th: t.start()
    for t in th: t.join(timeout=240)
    if errs or any(t.is_alive() for t in th):
        print(json.dumps({"error": errs or "timeout"}))
        sys.exit(1)
    bad = 0
    for j0, j1, st, z, on, status, _ in out:
        bad += int((st.view(np.uint64) != np.ascontiguousarray(S[:, j0:j1]).view(np.uint64)).sum())
        bad += int((on != onp[:, j0:j1]).sum()) + int((status != stp[:, j0:j1]).sum())
        bad += int((z.view(np.uint64) != np.ascontiguousarray(zp[:, j0:j1]).view(np.uint64)).sum())
    print(json.dumps({"world": world, "steps": N, "k": k, "mismatches": bad, "halo_rows": [o[6] for o in out]}))


if __name__ == "__main__":
    main()
