"""Driver of tests/test_gpu_flux_mean_ring.py (run as a fresh process with PICLES_CCL_LIB pointing at the loopback communicator):
`world` threads, one slab context each on the one GPU, joined into the library's NATIVE ring (picles_slab_run_steps), every rank
holding a flux set and a mean set over the coarse cells of its own rows — the update of a fused step runs on the ring's side stream
behind the interior launch and the delivered exchange, and under a wind lattice the context stream, on which the next windows are
sampled, waits for it.  Prints one JSON line: which accumulator planes of the rank-ordered concatenation differ from those of a
whole-grid context that took the same chunks through picles_run_steps, and whether the totals do."""
import json
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from picles_amd import _capi as K  # noqa: E402
from picles_amd.driver import flux_mean_concat  # noqa: E402
from picles_amd.parallel import SlabModel  # noqa: E402
from loopback_ring_driver import _NoExchange, box  # noqa: E402

NAMES = K.FLUX_FIELDS + ("n_active", "n_bad")


def main():
    world, case, solver, steps = int(sys.argv[1]), sys.argv[2], sys.argv[3], int(sys.argv[4])
    chunks = [int(c) for c in sys.argv[5].split(",")]
    every, first, halo = int(sys.argv[6]), int(sys.argv[7]), int(sys.argv[8])
    pair = (int(sys.argv[9]), int(sys.argv[10]))
    assert sum(chunks) == steps
    scales = (1025.0 * 9.81, 1025.0)
    cfg0 = box(case, solver)
    due = [s for s in range(1, steps + 1) if s >= first and (s - first) % every == 0]
    one = SlabModel(cfg0.model, 0, 1, device=0)
    one.flux_init(pair, K.FLUX_FIELDS, *scales, 2)
    one.seed()
    one.flux_mean_init(every=every, first=first)
    for c in chunks:
        one.run_steps(cfg0.Δt, c)
    want = one.gather_flux_means()
    state = one.get_state()

    uid, out, states, errs = {}, [None] * world, [None] * world, []
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
            sm.flux_init(pair, K.FLUX_FIELDS, *scales, 2)
            sm.seed()
            sm.flux_mean_init(every=every, first=first)
            for c in chunks:
                sm.run_steps(cfg.Δt, c)
            out[rank] = sm.flux_mean_get()
            states[rank] = sm.get_state()
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
    got = flux_mean_concat(out)
    same = lambda a, b: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()      # noqa: E731
    bad = [n for k, n in enumerate(NAMES) if got["acc"].shape != want["acc"].shape or not same(got["acc"][k], want["acc"][k])]
    print(json.dumps({"world": world, "case": case, "planes_that_differ": bad,
                      "totals_that_differ": [k for k in want["totals"] if not same(np.float64(got["totals"][k]), np.float64(want["totals"][k]))],
                      "state_equal": same(np.concatenate(states, axis=1), state),
                      "n_samples": [int(o["n_samples"]) for o in out], "want_samples": len(due),
                      "t_first": [o["t_first"] for o in out], "t_last": [o["t_last"] for o in out],
                      "want_t": [want["t_first"], want["t_last"]], "whole_grid_samples": want["n_samples"],
                      "active_share": float(want["totals"]["n_active"] / (state.shape[0] * state.shape[1])),
                      "phi_in_positive": bool((want["acc"][0] > 0).all())}))


if __name__ == "__main__":
    main()
