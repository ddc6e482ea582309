"""Driver of tests/test_gpu_track.py::test_init_is_refused_on_the_native_ring (run as a fresh process with PICLES_CCL_LIB pointing at
the loopback communicator): a whole-grid context joins the library's NATIVE ring as a ring of one; picles_track_init is refused
there and leaves no set, the ring steps afterwards, and once the ring has gone the same init succeeds and the context samples.
Prints one JSON line."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from picles_amd import _capi as K  # noqa: E402
from picles_amd import configs  # noqa: E402
from picles_amd.models import WaveGrowth2D  # noqa: E402
from picles_amd.simulations import Simulation, initialize_simulation  # noqa: E402


def main():
    cfg = configs.bench06_box(n=32)
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    m.upload_winds(m.clock.time, cfg.Δt)
    b, dt = m.backend, cfg.Δt
    t = np.array([0.5 * dt, 1.5 * dt, 2.5 * dt])
    ij = np.array([[3, 4, 5], [4, 5, 6], [3, 4, 5], [4, 5, 6], [7, 7, 7], [7, 7, 7], [8, 8, 8], [8, 8, 8]])
    w = np.full((4, 3), 0.25)
    out = {}
    b.slab_comm_init(b.slab_unique_id(), 0, 1)
    try:
        b.track_init(t, ij, w, dt)
        out["refusal"] = None
    except K.PiclesError as e:
        out["refusal"] = str(e)
    out["set_after_refusal"] = b.lib.picles_track_info(b.h, None, None, None) == 0
    b.slab_run_steps(dt, 2)
    out["clock_after_ring_steps"] = b.clock
    b.slab_comm_destroy()
    b.track_init(t, ij, w, dt)
    b.time_step(dt, K.STEP_ZERO_FIRST)
    out["info"] = list(b.track_info())
    b.track_fetch_begin(0, 3)
    tab = b.track_fetch_end()
    out["t_before"], out["t_after"] = [None if np.isnan(x) else float(x) for x in tab[3]], [None if np.isnan(x) else float(x) for x in tab[7]]
    out["state_finite"] = bool(np.isfinite(b.get_state()).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
