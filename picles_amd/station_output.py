"""StationWriter: point output — the time series of the sea state at a list of stations (buoys, platforms, validation points),
one record per scheduled model step, without leaving the fused stepping path.  The third product of a wave model beside restart
files (picles_amd/checkpointing.py) and gridded fields (picles_amd/field_output.py).  The reference's scripts cut the same
series out of full `cash_store` snapshots (`State[i, j, :]` against time: tests/T04_2D_reg_test.jl and the B0x regressions).

The library samples the State values of the stations' nodes on the device behind each step (picles_probe_*, include/picles_hip.h
"station probes": from the records of the pending fused step, which stays pending) and carries them to the host through a ring;
`run(sim)` stays on `picles_run_steps`, in chunks that end where the next checkpoint or field output falls or where the probe ring
would fill, and the writer pops the samples of EARLIER chunks while the latest one runs.

Attach like the other writers: `sim.output_writers["stations"] = StationWriter(model, points=[(x, y), ...], schedule=1, path="out")`.

POINTS -> NODES.  A point (x, y) is given in mesh coordinates.  Per axis, with x_0 the first node's coordinate, N the number of
nodes and dx = (x_{N-1} - x_0) / (N - 1):

    ξ = (x - x_0) / dx,   i0 = floor(ξ),   w_x = ξ - i0

* open axis: 0 <= ξ <= N - 1 is required (ValueError otherwise); ξ == N - 1 uses i0 = N - 2, w_x = 1.0
* periodic axis: 0 <= ξ < N is required; i0 + 1 wraps to 0
* tripolar y axis: as an open axis, and points in the top cell row (ξ_y >= N_y - 2) are refused (their corners fold)

The four corners are visited in the order (i0, j0), (i0+1, j0), (i0, j0+1), (i0+1, j0+1) with the weights

    (1.0 - w_x) * (1.0 - w_y),   w_x * (1.0 - w_y),   (1.0 - w_x) * w_y,   w_x * w_y

The writer probes the distinct corner nodes of all stations.  `nodes=[(i, j), ...]` (0-based) skips the interpolation: one corner,
the node itself, with weight 1.0.

PER STATION AND SAMPLE, in NumPy fp64, every operation one IEEE operation in the order written:

    a corner is WET when e, m_x, m_y are finite, e > 0 and m_x*m_x + m_y*m_y > 0        (the rule of picles_diag_*)
    W = SE = SX = SY = +0.0;  for each corner in the order above, if it is wet:
        W = W + w;  SE = SE + w * e;  SX = SX + w * m_x;  SY = SY + w * m_y
    E = SE / W;  MX = SX / W;  MY = SY / W;  M2 = MX * MX + MY * MY
    the station is VALID when W > 0 and M2 > 0;  otherwise every variable of the record is NaN
    hs   = 4.0 * sqrt(E)
    cg_x = (MX * E) / (2.0 * M2)          cg_y = (MY * E) / (2.0 * M2)
    cbar = E / (2.0 * sqrt(M2))
    tp   = (FOUR_PI * max(cbar / r_g, 0.1)) / g          FOUR_PI = 12.566370614359172
    dir  = atan2(MY, MX)
    e, m_x, m_y = E, MX, MY        (for `nodes=` stations: the node's State values themselves, bit for bit: w = 1.0)

with g, r_g of the model's ODE parameters — the expressions of the header's diagnostics definition applied to the station's means.

FILE, following picles_amd/field_output.py: where a libhdf5 loads `<name>.h5` with

    /stations/data        float64 (var, station, time)       /stations/var_names = e, m_x, m_y, hs, tp, cg_x, cg_y, dir
    /stations/x, y        float64 (NaN for `nodes=` stations: their coordinates are the nodes')      /stations/names
    /stations/time        float64                             /stations/iteration  float64 (whole numbers)

else `<name>.stations.data.npy` [time, station, var] + `<name>.json` (the same logical layout).  The record of the run's first
iteration (the seeded state, or the state a pickup restored) is written too, as FieldWriter writes it.  `read_station_output(path)`
reads either form.
"""
from __future__ import annotations

import json
import math
from pathlib import Path

import numpy as np

from .checkpointing import IterationInterval
from .output_writers import OutputWriter
from .storing import H5File, choose_format, read_h5_group

VAR_NAMES = ("e", "m_x", "m_y", "hs", "tp", "cg_x", "cg_y", "dir")
FOUR_PI = 12.566370614359172


def peak_period(cbar, g, r_g):
    """the header's tp of a mean phase-speed scale cbar = E / (2 sqrt(M2)), with its slow-wave floor; these IEEE operations in
    this order, for station records (below) and the run statistics' tp_at_max (picles_amd/run_statistics.py) alike"""
    return (FOUR_PI * np.maximum(cbar / r_g, 0.1)) / g


def _axis(x, x0, xN, N, kind, what):
    """(i0, i1, w) of one coordinate on one axis; kind: "open", "periodic" or "tripolar" """
    dx = (xN - x0) / (N - 1)
    xi = (x - x0) / dx
    if kind == "periodic":
        if not (0.0 <= xi < N):
            raise ValueError(f"station {what} = {x!r} outside the periodic axis [{x0!r}, {x0 + N * dx!r})")
        i0 = int(math.floor(xi))
        return i0, (i0 + 1) % N, xi - i0
    if not (0.0 <= xi <= N - 1):
        raise ValueError(f"station {what} = {x!r} outside the mesh [{x0!r}, {xN!r}]")
    if kind == "tripolar" and xi >= N - 2:
        raise ValueError(f"station {what} = {x!r} lies in the top cell row of a tripolar mesh (its corners fold over the seam)")
    i0 = int(math.floor(xi))
    if i0 == N - 1:
        return N - 2, N - 1, 1.0
    return i0, i0 + 1, xi - i0


def _kind(n):
    name = type(n).__name__
    return "periodic" if name == "N_Periodic" else ("tripolar" if name == "N_TripolarNorth" else "open")


def locate_points(grid, points):
    """points (x, y) in mesh coordinates -> (corners int64 [n, 4, 2] in the visiting order, weights float64 [n, 4])"""
    xs, ys = np.asarray(grid.data.x)[:, 0], np.asarray(grid.data.y)[0, :]
    Nx, Ny = int(grid.stats.Nx), int(grid.stats.Ny)
    kx, ky = _kind(grid.stats.Nx), _kind(grid.stats.Ny)
    corners = np.empty((len(points), 4, 2), dtype=np.int64)
    weights = np.empty((len(points), 4))
    for k, (x, y) in enumerate(points):
        i0, i1, wx = _axis(float(x), float(xs[0]), float(xs[-1]), Nx, kx, "x")
        j0, j1, wy = _axis(float(y), float(ys[0]), float(ys[-1]), Ny, ky, "y")
        corners[k] = [(i0, j0), (i1, j0), (i0, j1), (i1, j1)]
        weights[k] = [(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy]
    return corners, weights


def wet_means(values, index, weights):
    """the accumulation of the module docstring, from the wet test to the means: values float64 [..., 3, n_nodes], index int
    [n, n_entries] into the node axis, weights [n, n_entries] -> E, MX, MY, valid, each [..., n] (not yet NaN where not valid).
    The mix and the restrict of a nest (k_nest.h, picles_amd/nesting.py) are this too; an entry of weight 0.0 needs no skipping:
    W + 0.0 = W, and a sum that started at +0.0 keeps its bits when +-0.0 is added"""
    W = SE = SX = SY = np.zeros(values.shape[:-2] + index.shape[:1])
    with np.errstate(all="ignore"):
        for c in range(index.shape[1]):
            e, mx, my = values[..., 0, index[:, c]], values[..., 1, index[:, c]], values[..., 2, index[:, c]]
            w = weights[:, c]
            wet = np.isfinite(e) & np.isfinite(mx) & np.isfinite(my) & (e > 0.0) & (mx * mx + my * my > 0.0)
            W = np.where(wet, W + w, W)
            SE = np.where(wet, SE + w * e, SE)
            SX = np.where(wet, SX + w * mx, SX)
            SY = np.where(wet, SY + w * my, SY)
        E, MX, MY = SE / W, SX / W, SY / W
        return E, MX, MY, (W > 0.0) & (MX * MX + MY * MY > 0.0)


def station_records(values, index, weights, g, r_g):
    """values [samples, 3, n_nodes] (probe samples), index int [n_stations, n_corners] into the node axis, weights
    [n_stations, n_corners] -> float64 [samples, n_stations, 8] in the order of VAR_NAMES (the module docstring's arithmetic)"""
    E, MX, MY, valid = wet_means(np.asarray(values, dtype=np.float64), index, weights)
    with np.errstate(all="ignore"):
        M2 = MX * MX + MY * MY
        hs = 4.0 * np.sqrt(E)
        cgx = (MX * E) / (2.0 * M2)
        cgy = (MY * E) / (2.0 * M2)
        cbar = E / (2.0 * np.sqrt(M2))
        tp = peak_period(cbar, g, r_g)
        dr = np.arctan2(MY, MX)
    out = np.stack([E, MX, MY, hs, tp, cgx, cgy, dr], axis=-1)
    out[~valid] = np.nan
    return out


class NpyStationStore:
    format = "npy"

    def __init__(self, path, name, nt, x, y, names):
        self.dir = Path(path)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.path = self.dir / f"{name}.stations.data.npy"
        self.data = np.lib.format.open_memmap(self.path, mode="w+", dtype=np.float64, shape=(nt, len(names), len(VAR_NAMES)))
        self.data[:] = np.nan
        self.json = self.dir / f"{name}.json"
        self.meta = {"group": "stations", "dims": ["time", "station", "var"], "var_names": list(VAR_NAMES), "names": list(names),
                     "x": [float(v) for v in x], "y": [float(v) for v in y], "time": [float("nan")] * nt, "iteration": [float("nan")] * nt}

    def write(self, i, rec, time, iteration):
        self.data[i] = rec
        self.meta["time"][i] = float(time)
        self.meta["iteration"][i] = float(iteration)

    def close(self):
        self.data.flush()
        self.json.write_text(json.dumps(self.meta))


class H5StationStore:
    """the HDF5 form, through the file layer of picles_amd/storing.py; the records are kept in memory (stations x 8 doubles
    per record) and written when the file is closed"""

    format = "hdf5"

    def __init__(self, path, name, nt, x, y, names):
        h = self.h5 = H5File(path, name, "stations")
        self.dir, self.path = h.dir, h.path
        self.x, self.y, self.names = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), list(names)
        self.data = np.full((len(VAR_NAMES), len(names), nt), np.nan)
        self.time = np.full(nt, np.nan)
        self.iteration = np.full(nt, np.nan)

    def write(self, i, rec, time, iteration):
        self.data[:, :, i] = np.asarray(rec).T
        self.time[i] = time
        self.iteration[i] = iteration

    def close(self):
        h = self.h5
        if h.file is None:
            return
        h.f64("data", self.data)
        h.strings("dims", ["time", "station", "var"], attribute=True)
        h.strings("var_names", list(VAR_NAMES))
        h.strings("names", self.names)
        for k, a in (("x", self.x), ("y", self.y), ("time", self.time), ("iteration", self.iteration)):
            h.f64(k, a)
        h.close()


def make_station_store(path, name, nt, x, y, names, format="auto"):
    return choose_format(format, "station output", lambda: H5StationStore(path, name, nt, x, y, names),
                         lambda: NpyStationStore(path, name, nt, x, y, names))


class StationWriter(OutputWriter):
    """StationWriter(model, points=[(x, y), ...] | nodes=[(i, j), ...], names=None, schedule=1, path=..., name="stations",
    capacity=64)"""

    kind = "stations"
    needs = "probe_init"
    refusal = "a StationWriter needs a backend with probe_init / probe_sample / probe_pop (the HIP library)"
    sized_for_run = True

    def __init__(self, model=None, *, points=None, nodes=None, names=None, schedule=1, path=".", name="stations", capacity=64,
                 format="auto"):
        if (points is None) == (nodes is None):
            raise ValueError("StationWriter needs either points=[(x, y), ...] or nodes=[(i, j), ...]")
        self.model = model
        self.schedule = IterationInterval.of(schedule)
        self.path, self.name, self.format = Path(path), name, format
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("StationWriter: capacity must be >= 1")
        self.points = None if points is None else [(float(x), float(y)) for x, y in points]
        self.station_nodes = None if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1, 2)
        n = len(self.points) if points is not None else len(self.station_nodes)
        if n < 1:
            raise ValueError("StationWriter: no station given")
        self.names = [f"station_{k}" for k in range(n)] if names is None else [str(s) for s in names]
        if len(self.names) != n:
            raise ValueError("StationWriter: one name per station")
        self.store = None
        self.written = 0
        self.iterations = []          # the iteration of every record written, in order
        self._set_on = None           # the backend that holds this writer's probe set
        if model is not None:
            self._locate(model.grid)

    def _locate(self, grid):
        """corners and weights of the stations, and the distinct nodes to probe"""
        if self.points is not None:
            corners, self.weights = locate_points(grid, self.points)
        else:
            Nx, Ny = int(grid.stats.Nx), int(grid.stats.Ny)
            sn = self.station_nodes
            if sn.min() < 0 or sn[:, 0].max() >= Nx or sn[:, 1].max() >= Ny:
                raise ValueError(f"StationWriter: node outside [0, {Nx}) x [0, {Ny})")
            corners, self.weights = sn[:, None, :], np.ones((len(sn), 1))
        flat = corners.reshape(-1, 2)
        self.probe_nodes, inv = np.unique(flat, axis=0, return_inverse=True)
        self.index = np.asarray(inv).reshape(corners.shape[:2])
        self._grid = grid

    # ---- the cadence in iterations and in probe steps ----
    def first_step(self, it0: int) -> int:
        return self.schedule.first_step(it0)

    def allowance(self, backend, iteration: int) -> int:
        """how many steps may be enqueued from `iteration` without asking the ring for more than it holds: the samples of one
        chunk stay within half the ring (at least one), so that the samples of the chunk before can be popped while it runs.
        0: pop first"""
        N = self.schedule.interval
        allowance = min(self.capacity - backend.probe_pending, max(1, self.capacity // 2))
        if allowance <= 0:
            return 0
        return (iteration // N + allowance + 1) * N - 1 - iteration

    def steps_allowed(self, backend, iteration: int) -> int:
        """the ring's allowance, after making room where there is none; what is pending now are the samples of the chunks
        before the next one: after_chunk pops them while that chunk runs"""
        if self.allowance(backend, iteration) < 1:
            self.drain(backend)
        self._earlier = backend.probe_pending
        return self.allowance(backend, iteration)

    def after_chunk(self, backend):
        self.drain(backend, self._earlier)

    def begin_run(self, model, n_steps: int):
        """(re)create the probe set with the cadence continued from the model's iteration — a picked-up run goes on where the
        run that wrote the checkpoint would have —, open the file and take the record of the current iteration"""
        b = model.backend
        if getattr(self, "_grid", None) is not model.grid:
            self._locate(model.grid)
        if self._set_on is b:
            b.probe_free()
        it0 = int(model.clock.iteration)
        b.probe_init(self.probe_nodes, every=self.schedule.interval, first=self.first_step(it0), capacity=self.capacity)
        self._set_on = b
        self._it0 = it0
        P = model.ODEsettings.Parameters
        self._g, self._r_g = P.get("g", 9.81), P["r_g"]
        ns = len(self.names)
        if self.points is not None:
            x, y = [p[0] for p in self.points], [p[1] for p in self.points]
        else:
            x, y = [float("nan")] * ns, [float("nan")] * ns
        self.store = make_station_store(self.path, self.name, self.schedule.records_of(it0, n_steps), x, y, self.names, format=self.format)
        self.written = 0
        self.iterations = []
        b.probe_sample()

    def drain(self, backend, count=None):
        """pop and write `count` samples (all that are pending when None)"""
        pending = backend.probe_pending
        m = pending if count is None else min(int(count), pending)
        if m <= 0:
            return
        v, t, s = backend.probe_pop(m)
        rec = station_records(v, self.index, self.weights, self._g, self._r_g)
        for k in range(len(s)):
            it = self._it0 + int(s[k])
            self.store.write(self.written, rec[k], t[k], it)
            self.iterations.append(it)
            self.written += 1

    def before_step(self, backend):
        """the per-step loop: the library samples inside time_step and refuses a full ring; it gives up its older half first"""
        if backend.probe_pending >= self.capacity:
            self.drain(backend, max(1, self.capacity // 2))

    def finish(self, backend, iteration=None):
        if self.store is None:
            return
        self.drain(backend)
        self.store.close()
        self.last_store, self.store = self.store, None


def read_station_output(path, name="stations"):
    """either form: dict with `data` [time, station, var], `var_names`, `names`, `x`, `y`, `time`, `iteration` (arrays)"""
    d = Path(path)
    if (d / f"{name}.json").exists():
        out = json.loads((d / f"{name}.json").read_text())
        out["data"] = np.load(d / f"{name}.stations.data.npy")
        for k in ("x", "y", "time", "iteration"):
            out[k] = np.asarray(out[k], dtype=np.float64)
        return out
    out = read_h5_group(d / f"{name}.h5", "stations", f64=("data", "x", "y", "time", "iteration"), strings=("var_names", "names"),
                        attrs=("dims",))
    out["data"] = out["data"].transpose(2, 1, 0)        # file (var, station, time) -> [time, station, var]
    return out
