#!/usr/bin/env python3
"""Track output: three altimeter passes over a 512² storm box, sampled where and when the satellite was.

A pass crosses the box along a diagonal at 6.9 km/s ground speed and measures once a second: some 200 observations, each with its
own time and place.  The library samples, behind every model step, only the observations whose time lies next to the clock — their
four corner nodes, mixed on the device into a table that stays in device memory (picles_track_*, include/picles_hip.h "track
samples") — and the writer interpolates between the sample before and the sample after each observation.  The run itself stays on
the fused `picles_run_steps` path; State never crosses PCIe.  Needs a HIP device."""
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, run
from picles_amd.track_output import TrackWriter, read_track_output

out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(tempfile.mkdtemp(prefix="picles_tracks_"))
n = 512
L = 2000.0 * n
cfg = configs.bench06_box(n=n, winds=configs.smooth_winds(14.0, 6.0, L, L, a=0.6, b=0.4))      # a storm: the wind varies by half across the box
model = WaveGrowth2D(**cfg.model)
sim = Simulation(model, Δt=cfg.Δt, stop_time=cfg.Δt * 59)          # 60 steps of ten minutes

speed = 6900.0                                                      # ground speed [m/s]
seconds = np.arange(0.0, 0.98 * L * np.sqrt(2.0) / speed, 1.0)      # 1 Hz
along = seconds * speed / np.sqrt(2.0)
times, points, names = [], [], []
for p, (start, ascending) in enumerate(((2.1 * 3600.0, True), (5.3 * 3600.0, False), (9.6 * 3600.0, True))):
    times += list(start + seconds)
    points += [(0.01 * L + s, 0.01 * L + s if ascending else 0.99 * L - s) for s in along]
    names += [f"pass{p}_{k:03d}" for k in range(len(seconds))]
sim.output_writers["tracks"] = TrackWriter(model, times=times, points=points, names=names, path=out_dir, format="npy")
run(sim)

out = read_track_output(out_dir)
data, var = out["data"], list(out["var_names"])                     # (var, event), the order given above
hs, tp = data[var.index("hs")], data[var.index("tp")]
print(f"{model.clock.iteration} steps in {sim.run_wall_time:.3f} s, {data.shape[1]} observations in {out_dir}")
for p in range(3):
    sel = slice(p * len(seconds), (p + 1) * len(seconds))
    print(f"pass {p} at t = {out['time'][sel][0] / 3600:.2f} h, between the samples at {out['t_before'][sel][0] / 3600:.2f} h and "
          f"{out['t_after'][sel][0] / 3600:.2f} h:  Hs {np.nanmin(hs[sel]):.2f} .. {np.nanmax(hs[sel]):.2f} m,  Tp {np.nanmin(tp[sel]):.2f} .. "
          f"{np.nanmax(tp[sel]):.2f} s along the track")
