#!/usr/bin/env python3
"""PiCLES as the wave component of a coupled system, both directions on the device: a toy torch "atmosphere" produces
the 10 m winds of each coupling interval from the significant wave height the wave model exported at the end of the previous one —
rougher sea, more drag, weaker wind — and pushes them as one time level of a wind stream (picles_amd/coupling.py); the wave model
runs the interval as one chunk of fused steps and exports its coarse Hs plane into a torch tensor (picles_diag_export).  Every hand-over
is ordered by events against torch's stream; nothing is copied to the host inside the loop, and the host waits for nothing.
Needs a HIP device.  python examples/coupled_atmosphere_torch.py [n_intervals]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from picles_amd import configs
from picles_amd.coupling import StreamedWinds
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, initialize_simulation

n, dx, DT = int(os.environ.get("COUPLED_N", "512")), 2000.0, 600.0
STEPS = 3                                   # model steps per coupling interval
n_intervals = int(sys.argv[1]) if len(sys.argv) > 1 else 12
L = dx * (n - 1)
NX = NY = 65                                # the atmosphere's grid
dev = torch.device("cuda")
xa = torch.linspace(0.0, L, NX, device=dev, dtype=torch.float64)
ya = torch.linspace(0.0, L, NY, device=dev, dtype=torch.float64)
Y, X = torch.meshgrid(ya, xa, indexing="ij")          # (ny, nx): x fastest, the layout a level is pushed in


def atmosphere(k, hs):
    """the winds at the start of interval k: a jet that swings with time, slowed where the sea is rough (hs: the wave model's coarse
    Hs plane [nyc, nxc] on the device, or None before the first export)"""
    t = k * STEPS * DT
    u = 11.0 + 3.0 * torch.sin(2 * np.pi * (Y / L) + t / 7e3)
    v = 3.0 + 2.0 * torch.cos(2 * np.pi * (X / L) - t / 9e3)
    if hs is not None:
        rough = torch.nn.functional.interpolate(torch.nan_to_num(hs)[None, None], size=(NY, NX), mode="bilinear", align_corners=True)[0, 0]
        drag = 1.0 / (1.0 + 0.08 * rough.double())
        u, v = u * drag, v * drag
    return u.contiguous(), v.contiguous()


cfg = configs.bench06_box(n=n, dx=dx, periodic_grid=False)
winds = StreamedWinds(xa.cpu().numpy(), ya.cpu().numpy(), t0=0.0, dt=STEPS * DT, slots=3)
cfg.model["winds"] = winds
cfg.model["winds_static"] = False
model = WaveGrowth2D(**cfg.model)
b = model.backend
winds.attach(model)
winds.push(0, *atmosphere(0, None))                  # the seed reads the winds at t = 0
initialize_simulation(Simulation(model, Δt=DT, stop_time=1.0))
b.diag_init(coarsen=(4, 4), fields=("hs",), n_slots=1)
nxc, nyc, nf, npart, _ = b.diag_shape()
hs = torch.zeros((nf, nyc, nxc), device=dev, dtype=torch.float32)
partials = torch.zeros((npart, 7), device=dev, dtype=torch.float64)
b.diag_export(hs, partials)
peak = torch.zeros((), device=dev, dtype=torch.float32)

t0 = time.perf_counter()
for k in range(1, n_intervals + 1):
    winds.push(k, *atmosphere(k, hs[0]))             # level k closes interval k - 1: the atmosphere has seen the sea state at its start
    b.run_steps(DT, STEPS)                           # refused with a text if a level were missing
    b.diag_export(hs, partials)                      # Hs at the end of the interval, for the next winds
    peak = torch.maximum(peak, torch.nan_to_num(hs[0]).max())
b.sync()
torch.cuda.synchronize()
wall = time.perf_counter() - t0
slots, oldest, newest, pushes = b.wind_stream_info()
print(f"{n_intervals} coupling intervals of {STEPS} steps on {n}x{n} in {wall:.2f} s ({1e3 * wall / (n_intervals * STEPS):.2f} ms/step): "
      f"{pushes} levels pushed from the device (ring of {slots}: levels {oldest} .. {newest} held), "
      f"peak Hs {float(peak):.2f} m, mean energy {float(partials[:, 0].sum()) / (n * n):.4g}")
