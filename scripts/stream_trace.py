"""per-push and export cost, for a kernel trace (rocprofv3 --kernel-trace --memory-copy-trace --stats -- python scripts/stream_trace.py): a 4096^2 box under a wind stream (65 x 65 lattice), 20 steps with a float64 device
push each (a device-to-device copy pair), 20 with a float32 push each (k_wind_ingest), and 20 picles_diag_export at (4, 4)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from picles_amd import configs
from picles_amd.coupling import StreamedWinds
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, initialize_simulation

N, DT, dx = 4096, 600.0, 2000.0
L = dx * (N - 1)
xa = np.linspace(0.0, L, 65)
Y, X = np.meshgrid(xa, xa, indexing="ij")
def level(k, dtype):
    t = k * DT
    u = 10.0 + 2.0 * np.sin(2 * np.pi * X / L) * np.cos(t / 5e3)
    v = 10.0 + 2.0 * np.cos(2 * np.pi * Y / L) * np.sin(t / 7e3)
    return tuple(torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).cuda() for a in (u, v))
cfg = configs.bench06_box(n=N, dx=dx)
sw = StreamedWinds(xa, xa, 0.0, DT, slots=3)
cfg.model["winds"], cfg.model["winds_static"] = sw, False
m = WaveGrowth2D(**cfg.model)
b = m.backend
sw.attach(m)
sw.push(0, *level(0, np.float64))
initialize_simulation(Simulation(m, Δt=DT, stop_time=1.0))
lev = [level(k, np.float64 if k <= 25 else np.float32) for k in range(47)]
for s in range(45):
    b.wind_stream_push(s + 1, *lev[s + 1])
    b.run_steps(DT, 1)
b.diag_init(coarsen=(4, 4), fields=("hs", "tp", "cg_x", "cg_y"), n_slots=1)
nxc, nyc, nf, npart, _ = b.diag_shape()
f = torch.zeros((nf, nyc, nxc), device="cuda", dtype=torch.float32)
p = torch.zeros((npart, 7), device="cuda", dtype=torch.float64)
for _ in range(20):
    b.diag_export(f, p)
b.sync()
torch.cuda.synchronize()
print("trace run done: Hs max", float(torch.nan_to_num(f[0]).max()))
