"""Child process of tests/test_gpu_checkpoint.py::test_run_with_checkpointer_and_pickup_in_a_fresh_process: builds the same model as
the parent with a later stop_time, run(sim, pickup=True) from the parent's checkpoint directory, saves State and the iteration."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from picles_amd import configs  # noqa: E402

DT = 600.0
STOP = 19 * DT


def cfg():
    return configs.bench06_box(n=40)


def main(ckdir, out):
    from picles_amd.checkpointing import Checkpointer
    from picles_amd.models import WaveGrowth2D
    from picles_amd.simulations import Simulation, run
    m = WaveGrowth2D(**cfg().model)
    sim = Simulation(m, Δt=DT, stop_time=STOP)
    sim.output_writers["checkpointer"] = Checkpointer(m, schedule=4, dir=ckdir, prefix="box")
    run(sim, pickup=True)
    np.savez(out, State=m.backend.get_state(), iteration=m.clock.iteration)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
