#!/usr/bin/env python3
"""The storm-peak map of a moving storm: the vortex of examples/gridded_winds_storm.py crosses a box under gridded, time-varying
winds sampled on the device, and a StatisticsWriter keeps — per node, on the device, behind every step — the largest significant
wave height and when it occurred, the period and direction at that peak, the mean sea state and the share of the time with
Hs above 1 m and 2 m.  State never leaves the GPU; the file holds one record for the whole run (window=None) and is read back
with read_statistics.  Needs a HIP device.  python examples/storm_peak_map.py [n_steps] [out_dir]"""
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np

from picles_amd import configs
from picles_amd.models import WaveGrowth2D
from picles_amd.run_statistics import StatisticsWriter, read_statistics, variable
from picles_amd.simulations import Simulation, run
from picles_amd.wind_emulator import IdealizedWindGrid, wind_interpolator

n, dx, DT = int(__import__("os").environ.get("STORM_N", "512")), 2000.0, 600.0
L = dx * (n - 1)
n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 72
out_dir = Path(sys.argv[2]) if len(sys.argv) > 2 else Path("storm_peak_out")


def storm(x, y, t):
    """a vortex of 150 km radius (8 m/s at its wall) crossing the box in 12 hours, embedded in a (12, 4) m/s flow (the wind speed
    stays well above the 2 m/s gate of the growth parameterisation everywhere)"""
    xc, yc = 0.2 * L + 0.6 * L * t / 43200.0, 0.5 * L
    r = np.hypot(x - xc, y - yc) + 1.0
    vt = 8.0 * (r / 1.5e5) * np.exp(1.0 - r / 1.5e5)
    return -vt * (y - yc) / r + 12.0, vt * (x - xc) / r + 4.0


lattice = IdealizedWindGrid(lambda x, y, t: storm(x, y, t)[0], lambda x, y, t: storm(x, y, t)[1],
                            dict(Lx=L, Ly=L, T=DT * (n_steps + 1)), dict(dx=L / 64, dy=L / 64, dt=1800.0))
cfg = configs.bench06_box(n=n, dx=dx, periodic_grid=False)
cfg.model["winds"] = wind_interpolator(lattice)
cfg.model["winds_static"] = False
model = WaveGrowth2D(**cfg.model)
sim = Simulation(model, Δt=DT, stop_time=DT * (n_steps - 1))          # run() takes one step past stop_time
sim.output_writers["statistics"] = StatisticsWriter(model, fields=("peak", "mean", "exceed"), thresholds=(1.0, 2.0), schedule=1,
                                                    window=None, path=out_dir, name="storm")
t0 = time.perf_counter()
run(sim)
wall = time.perf_counter() - t0

out = read_statistics(out_dir, name="storm")
hs_max = variable(out, "hs_max")[:, :, 0]                              # (y, x) of the run's only window
t_of_max = variable(out, "t_of_max")[:, :, 0]
j, i = np.unravel_index(np.nanargmax(hs_max), hs_max.shape)
print(f"{n_steps} steps of {n}x{n} in {wall:.2f} s ({1e3 * wall / n_steps:.2f} ms/step), {int(out['n_samples'][0])} samples per node; "
      f"largest Hs of the run {hs_max[j, i]:.2f} m at x = {out['x'][i] / 1e3:.0f} km, y = {out['y'][j] / 1e3:.0f} km, "
      f"{t_of_max[j, i] / 3600.0:.1f} h into the run; mean Hs {np.nanmean(variable(out, 'hs_mean')):.2f} m; "
      f"Hs >= 2 m for {100.0 * np.mean(variable(out, 'exceed_1')):.1f} % of the node-hours; written to {out_dir}")
