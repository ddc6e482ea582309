#!/usr/bin/env python3
"""PiCLES as the wave component of a coupled system that exchanges INTERVAL MEANS: the loop of
examples/coupled_fluxes_torch.py with six wave steps per coupling interval.  A toy torch "atmosphere" pushes the 10 m winds of each
interval as one time level of a wind stream; the wave model runs the interval as ONE chunk of fused steps, the device adds the
coupling fluxes of every step to its accumulators behind the step (picles_flux_mean_*), and at the end of the interval the mean over
the six steps is written into torch tensors (picles_flux_mean_export, which also empties the accumulators):
    to the atmosphere  tq_in   the momentum the waves took out of the wind over the interval [N m-2]
    to the ocean       tq_dis, phi_dis   the momentum and energy the breaking waves handed down [N m-2, W m-2]; us, the Stokes drift
What the partners receive is what crossed the surface over the interval, not the state of its last instant.
Needs a HIP device.  python examples/coupled_flux_means_torch.py [n_intervals]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

from picles_amd import configs
from picles_amd.coupling import FluxMeanExport, StreamedWinds
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, initialize_simulation

n, dx, DT = int(os.environ.get("COUPLED_N", "512")), 2000.0, 600.0
STEPS = 6                                   # ten-minute wave steps against an hourly exchange
n_intervals = int(sys.argv[1]) if len(sys.argv) > 1 else 6
L = dx * (n - 1)
NX = NY = 65                                # the atmosphere's grid
RHO_AIR, RHO_WATER, MIXED_LAYER = 1.225, 1025.0, 20.0
dev = torch.device("cuda")
xa = torch.linspace(0.0, L, NX, device=dev, dtype=torch.float64)
ya = torch.linspace(0.0, L, NY, device=dev, dtype=torch.float64)
Y, X = torch.meshgrid(ya, xa, indexing="ij")          # (ny, nx): x fastest, the layout a level is pushed in


def to_atmosphere(plane):
    return torch.nn.functional.interpolate(plane[None, None], size=(NY, NX), mode="bilinear", align_corners=True)[0, 0].double()


def atmosphere(k, taw):
    """the winds at the start of interval k: a jet that swings with time, slowed by the mean stress the waves took out of it over
    the last interval (taw: (tq_in_x, tq_in_y) planes [nyc, nxc] on the device, or None before the first exchange)"""
    t = k * STEPS * DT
    u = 11.0 + 3.0 * torch.sin(2 * np.pi * (Y / L) + t / 7e3)
    v = 3.0 + 2.0 * torch.cos(2 * np.pi * (X / L) - t / 9e3)
    if taw is not None:      # a 500 m boundary layer loses the wave-supported momentum flux of the interval
        u = u - to_atmosphere(taw[0]) * (STEPS * DT) / (RHO_AIR * 500.0)
        v = v - to_atmosphere(taw[1]) * (STEPS * DT) / (RHO_AIR * 500.0)
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
means = FluxMeanExport(model, coarsen=(4, 4), rho_water=RHO_WATER)
current, heat, taw = None, torch.zeros((), device=dev, dtype=torch.float64), None

t0 = time.perf_counter()
for k in range(1, n_intervals + 1):
    winds.push(k, *atmosphere(k, taw))               # level k closes interval k - 1
    b.run_steps(DT, STEPS)                           # one fused chunk; the accumulators take a sample behind every step
    assert means.n_samples == STEPS
    F = means()                                      # the means of the interval; the accumulators start afresh
    taw = (F["tq_in_x"].clone(), F["tq_in_y"].clone())
    if current is None:
        current = torch.zeros((2,) + tuple(F["tq_dis_x"].shape), device=dev, dtype=torch.float32)
    current[0] += F["tq_dis_x"] * (STEPS * DT) / (RHO_WATER * MIXED_LAYER)      # the "ocean": stress into a mixed layer
    current[1] += F["tq_dis_y"] * (STEPS * DT) / (RHO_WATER * MIXED_LAYER)
    heat += F["phi_dis"].double().mean() * (STEPS * DT)
b.sync()
torch.cuda.synchronize()
wall = time.perf_counter() - t0
tot = means.partials.sum(dim=0).cpu().numpy() / means.exported["n_samples"]
print(f"{n_intervals} coupling intervals of {STEPS} steps on {n}x{n} in {wall:.2f} s ({1e3 * wall / (n_intervals * STEPS):.2f} ms/step); "
      f"means of the last interval [{means.exported['t_first']:.0f} s, {means.exported['t_last']:.0f} s]: "
      f"wave-supported stress {float(torch.hypot(F['tq_in_x'], F['tq_in_y']).mean()):.3f} N m-2, "
      f"stress to the ocean {float(torch.hypot(F['tq_dis_x'], F['tq_dis_y']).mean()):.3f} N m-2, "
      f"dissipation {float(F['phi_dis'].mean()):.3f} W m-2 ({float(heat):.3g} J m-2 over the run), "
      f"Stokes drift {float(torch.hypot(F['us_x'], F['us_y']).mean()):.3f} m s-1, surface current {float(current.abs().max()):.3f} m s-1; "
      f"{int(round(tot[9]))} active and {int(round(tot[10]))} bad nodes per sample")
