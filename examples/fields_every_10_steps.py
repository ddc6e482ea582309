#!/usr/bin/env python3
"""Coarse wave fields every 10 steps: Hs, Tp and the group velocity of a 512² periodic box, averaged over 4×4 node blocks on the
device and written on a schedule, while the run itself stays on the fused `picles_run_steps` path between the outputs.

What `PartitionOutput` / `GetGroupVelocity` / `mean_of_state` of the reference derive from State on the host afterwards is formed
where the data is (picles_diag_*, include/picles_hip.h): an output is 4 float32 planes of 128² instead of 3 float64 planes of 512².
Needs a HIP device."""
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.field_output import FieldWriter, read_field_output
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, run

out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="picles_fields_"))
n = 512
cfg = configs.bench06_box(n=n, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * n, 2000.0 * n))
model = WaveGrowth2D(**cfg.model)
sim = Simulation(model, Δt=cfg.Δt, stop_time=cfg.Δt * 59)          # 60 steps: run! takes one step past stop_time
sim.output_writers["fields"] = FieldWriter(model, schedule=10, path=out_dir, coarsen=(4, 4), fields=("hs", "tp", "cg_x", "cg_y"),
                                           format="npy")
run(sim)

out = read_field_output(out_dir)
data, scalars = out["data"], out["scalars"]                          # [time, x, y, field], [time, 8]
print(f"{model.clock.iteration} steps in {sim.run_wall_time:.3f} s, {data.shape[0]} records of {data.shape[1]}x{data.shape[2]} cells "
      f"x {data.shape[3]} fields in {out_dir}")
hs, tp = data[..., out["var_names"].index("hs")], data[..., out["var_names"].index("tp")]
direction = np.degrees(np.arctan2(data[..., 3], data[..., 2]))       # the host takes atan2 of the coarse cg planes
for k, t in enumerate(out["time"]):
    s = dict(zip(out["scalar_names"], scalars[k]))
    print(f"t = {t / 3600:5.2f} h   Hs mean {np.nanmean(hs[k]):.3f} m  max {np.nanmax(hs[k]):.3f} m   Tp mean {np.nanmean(tp[k]):.2f} s   "
          f"dir {np.nanmean(direction[k]):.1f} deg   mean_of_state {s['mean_of_state']:.4e}   max_e {s['max_e']:.4e}")
