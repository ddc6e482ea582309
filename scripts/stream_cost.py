"""4096^2 box, DP5, winds varying in time: ms per step of (a) host levels through picles_set_winds every step, (b) a wind stream with one
device push per step (coupling interval = the step), (c) the same lattice uploaded whole.  Four alternated rounds of 20 steps after a
warm-up of 5; every route steps through run_steps(dt, 1) / time_step once per step so that the call pattern is the same."""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from picles_amd import configs, _capi as K
from picles_amd.coupling import StreamedWinds
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.wind_emulator import IdealizedWindGrid, wind_interpolator

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS, WARM, ROUNDS = 20, 5, 4
DT, dx = 600.0, 2000.0
L = dx * (N - 1)
u = lambda x, y, t: 10.0 + 2.0 * np.sin(2 * np.pi * x / L) * np.cos(t / 5e3) + 0 * y
v = lambda x, y, t: 10.0 + 2.0 * np.cos(2 * np.pi * y / L) * np.sin(t / 7e3) + 0 * x
NLEV = WARM + ROUNDS * STEPS + 4
lat = IdealizedWindGrid(u, v, dict(Lx=L, Ly=L, T=DT * (NLEV - 1)), dict(dx=L / 64, dy=L / 64, dt=DT))
assert lat["t"].size == NLEV


def model_of(winds):
    cfg = configs.bench06_box(n=N, dx=dx)
    cfg.model["winds"] = winds
    cfg.model["winds_static"] = False
    m = WaveGrowth2D(**cfg.model)
    return m


out = {"n": N, "steps": STEPS, "warmup": WARM, "rounds": ROUNDS, "lattice": [int(lat["x"].size), int(lat["y"].size), NLEV]}

# (c) the lattice uploaded whole
mc = model_of(wind_interpolator(lat))
initialize_simulation(Simulation(mc, Δt=DT, stop_time=1.0))
mc.upload_winds(0.0, DT)

# (b) the stream: levels as device tensors, made before the clock starts
lev = [tuple(torch.from_numpy(np.ascontiguousarray(lat[c][:, :, k].T)).cuda() for c in ("u", "v")) for k in range(NLEV)]
sw = StreamedWinds(lat["x"], lat["y"], 0.0, DT, slots=3)
mb = model_of(sw)
sw.attach(mb)
sw.push(0, *lev[0])
initialize_simulation(Simulation(mb, Δt=DT, stop_time=1.0))

# (a) host levels at node resolution: the closures sampled at the step's ends by NumPy beforehand (two alternating pairs would hide
# nothing: the cost measured is the library's route, two planes of N^2 doubles per level over PCIe), set every step
ma = model_of(wind_interpolator(lat))
ma.backend  # the same lattice object only names the winds of the seed; the steps below set host levels
initialize_simulation(Simulation(ma, Δt=DT, stop_time=1.0))
X, Y = ma.grid.data.x, ma.grid.data.y
PA = np.ascontiguousarray((2.0 * np.sin(2 * np.pi * X / L)).reshape(-1, order="F"))
PB = np.ascontiguousarray((2.0 * np.cos(2 * np.pi * Y / L)).reshape(-1, order="F"))
planes = {}
def node_level(t):
    """the closures at the mesh nodes (the lattice tabulates the same closures; the spatial factors are formed once)"""
    if t not in planes:
        planes[t] = (10.0 + PA * np.cos(t / 5e3), 10.0 + PB * np.sin(t / 7e3))
    return planes[t]


def steps_a(k0, n):
    b = ma.backend
    for s in range(k0, k0 + n):
        t = s * DT
        u0, v0 = node_level(t)
        u1, v1 = node_level(t + DT)
        rc = b.lib.picles_set_winds(b.h, K.dptr(u0), K.dptr(v0), t, K.dptr(u1), K.dptr(v1), t + DT)
        assert rc == 0
        b.time_step(DT, K.STEP_ZERO_FIRST)
        planes.pop(t, None)
    b.sync()


def steps_b(k0, n):
    b = mb.backend
    for s in range(k0, k0 + n):
        b.wind_stream_push(s + 1, *lev[s + 1])
        b.run_steps(DT, 1)
    b.sync()


def steps_c(k0, n):
    b = mc.backend
    for s in range(k0, k0 + n):
        b.run_steps(DT, 1)
    b.sync()


routes = {"a_host_levels": steps_a, "b_stream": steps_b, "c_lattice": steps_c}
for f in routes.values():
    f(0, WARM)
res = {k: [] for k in routes}
for r in range(ROUNDS):
    k0 = WARM + r * STEPS
    for name, f in routes.items():
        if name == "a_host_levels":
            for s in range(k0, k0 + STEPS + 1):      # the NumPy sampling is not the route's cost: done before the clock starts
                node_level(s * DT)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f(k0, STEPS)
        res[name].append(1e3 * (time.perf_counter() - t0) / STEPS)
        print(name, r, f"{res[name][-1]:.3f} ms/step", flush=True)
out["ms_per_step"] = res
out["median"] = {k: float(np.median(x)) for k, x in res.items()}
out["spread"] = {k: float(max(x) - min(x)) for k, x in res.items()}
# (b) against (c): bit for bit only where no sampled time lies inside the snapping slack of a level without being one — with
# 600-second steps on 600-second levels t (1/600) misses the whole number by an ulp or two at some steps, the lattice then blends
# with a weight of 1e-15 and the stream reads the level alone: the difference is reported
sb, sc, sa = mb.backend.get_state(), mc.backend.get_state(), ma.backend.get_state()
out["b_equals_c_bitwise"] = bool(np.array_equal(sb, sc, equal_nan=True))
out["b_vs_c_max_abs_e"] = float(np.nanmax(np.abs(sb[..., 0] - sc[..., 0])))
out["a_vs_c_max_abs_e"] = float(np.nanmax(np.abs(sa[..., 0] - sc[..., 0])))      # (node-sampled closures vs their 65 x 65 lattice)
out["c_max_e"] = float(np.nanmax(sc[..., 0]))
print(json.dumps(out))
