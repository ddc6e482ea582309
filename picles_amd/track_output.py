"""TrackWriter: track output — the sea state along moving platforms (altimeter passes, ships, drifting buoys), one record per
observation, without leaving the fused stepping path.  The fourth output beside gridded fields (picles_amd/field_output.py), fixed
stations (picles_amd/station_output.py) and per-node statistics (picles_amd/run_statistics.py).

Every observation is an EVENT with its own time and place (t_k, x_k, y_k).  The library samples, behind each step, only the events
whose time lies next to the clock, mixes their four corner nodes on the device and keeps, per event, the latest sample taken at a
clock <= t_k (BEFORE) and the earliest taken at a clock >= t_k (AFTER) in a table in device memory (picles_track_*,
include/picles_hip.h "track samples"); `run(sim)` stays on `picles_run_steps`, and this writer never ends a chunk.  The writer
fetches the slots of the events a chunk has completed while the next chunk runs, and interpolates linearly in time.

Attach like the other writers:
    sim.output_writers["tracks"] = TrackWriter(model, times=[t, ...], points=[(x, y), ...], path="out")

EVENTS -> CORNERS.  A point (x, y) is located as a station is (picles_amd/station_output.py, "POINTS -> NODES": the same ξ, i0, w_x
per axis, the same visiting order of the four corners, the same weights), here for all events at once in NumPy: `locate_points_fast`
gives the bits of `station_output.locate_points`.  The events are handed to the library sorted by time (a stable sort); the file
keeps the caller's order.

PER EVENT, in NumPy fp64, every operation one IEEE operation in the order written, with (E_b, MX_b, MY_b, t_b) the before slot and
(E_a, MX_a, MY_a, t_a) the after slot (each the station definition over the four corners at that sample's clock, NaN where the
point was not valid then):

    if any of the eight is NaN:     every variable of the record is NaN
    else if t_a == t_b:             V = V_b                                    for V = E, MX, MY
    else (t_a > t_b):               s = (t_k - t_b) / (t_a - t_b);   V = V_b + s * (V_a - V_b)
    M2 = MX * MX + MY * MY;   the record is NaN too when not M2 > 0
    hs   = 4.0 * sqrt(E)
    cg_x = (MX * E) / (2.0 * M2)          cg_y = (MY * E) / (2.0 * M2)
    cbar = E / (2.0 * sqrt(M2))
    tp   = (FOUR_PI * max(cbar / r_g, 0.1)) / g
    dir  = atan2(MY, MX)
    e, m_x, m_y = E, MX, MY

— `station_output.station_records`' expressions applied to the interpolated means.  An event outside the span of the run's sample
clocks (before the first, after the last) has one slot empty and a NaN record; `t_before` and `t_after` in the file say which.

FILE, through the file layer of picles_amd/storing.py: where a libhdf5 loads `<name>.h5` with

    /tracks/data        float64 (var, event), the caller's order       /tracks/var_names = e, m_x, m_y, hs, tp, cg_x, cg_y, dir
    /tracks/time, x, y  float64 (event)                                  /tracks/names
    /tracks/t_before, t_after   float64 (event): the clocks of the two samples (NaN: none)

else `<name>.tracks.data.npy` [event, var] + `<name>.json` (the same logical layout).  `read_track_output(path)` reads either form.

PICKUP.  The table is not checkpointed.  Under `run(sim, pickup=...)` the set is made anew at the restored clock: events before that
clock have no before slot and are NaN; from the restored clock on the records are those of the straight run.
Not for slabs (`SlabModel`): the corners of an event may lie on two ranks.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from .output_writers import NO_LIMIT, OutputWriter
from .station_output import VAR_NAMES, _kind, peak_period
from .storing import H5File, choose_format, read_h5_group


def _axis_fast(x, x0, xN, N, kind, what):
    """station_output._axis for an array of coordinates: (i0, i1, w), the same IEEE operations per element"""
    x = np.asarray(x, dtype=np.float64)
    dx = (xN - x0) / (N - 1)
    xi = (x - x0) / dx
    if kind == "periodic":
        bad = ~((0.0 <= xi) & (xi < N))
    else:
        bad = ~((0.0 <= xi) & (xi <= N - 1))
        if kind == "tripolar":
            bad |= xi >= N - 2
    if bad.any():
        k = int(np.argmax(bad))
        raise ValueError(f"track event {k}: {what} = {float(x[k])!r} outside the mesh (or in the top cell row of a tripolar mesh)")
    f = np.floor(xi)
    i0 = f.astype(np.int64)
    w = xi - f
    if kind == "periodic":
        return i0, (i0 + 1) % N, w
    last = i0 == N - 1
    i0 = np.where(last, N - 2, i0)
    return i0, i0 + 1, np.where(last, 1.0, w)


def locate_points_fast(grid, points):
    """station_output.locate_points, vectorised: points [n, 2] -> (corners int64 [n, 4, 2], weights float64 [n, 4]), bit for bit"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    xs, ys = np.asarray(grid.data.x)[:, 0], np.asarray(grid.data.y)[0, :]
    Nx, Ny = int(grid.stats.Nx), int(grid.stats.Ny)
    i0, i1, wx = _axis_fast(p[:, 0], float(xs[0]), float(xs[-1]), Nx, _kind(grid.stats.Nx), "x")
    j0, j1, wy = _axis_fast(p[:, 1], float(ys[0]), float(ys[-1]), Ny, _kind(grid.stats.Ny), "y")
    corners = np.stack([np.stack([i0, j0], -1), np.stack([i1, j0], -1), np.stack([i0, j1], -1), np.stack([i1, j1], -1)], axis=1)
    weights = np.stack([(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy], axis=1)
    return corners.astype(np.int64), weights


def track_records(table, times, g, r_g):
    """table float64 [8, n] (planes e_b, mx_b, my_b, t_b, e_a, mx_a, my_a, t_a), times [n] -> float64 [n, 8] in the order of
    VAR_NAMES: the module docstring's arithmetic"""
    T = np.asarray(table, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64)
    tb, ta = T[3], T[7]
    with np.errstate(all="ignore"):
        valid = ~np.isnan(T).any(axis=0)
        same = ta == tb
        s = (t - tb) / (ta - tb)
        E, MX, MY = (np.where(same, T[k], T[k] + s * (T[4 + k] - T[k])) for k in range(3))
        M2 = MX * MX + MY * MY
        valid &= M2 > 0.0
        hs = 4.0 * np.sqrt(E)
        cgx = (MX * E) / (2.0 * M2)
        cgy = (MY * E) / (2.0 * M2)
        cbar = E / (2.0 * np.sqrt(M2))
        tp = peak_period(cbar, g, r_g)
        dr = np.arctan2(MY, MX)
    out = np.stack([E, MX, MY, hs, tp, cgx, cgy, dr], axis=-1)
    out[~valid] = np.nan
    return out


class NpyTrackStore:
    format = "npy"

    def __init__(self, path, name):
        self.dir = Path(path)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.path = self.dir / f"{name}.tracks.data.npy"
        self.json = self.dir / f"{name}.json"

    def close(self, data, time, x, y, t_before, t_after, names):
        np.save(self.path, np.ascontiguousarray(data))
        lst = lambda a: [float(v) for v in a]      # noqa: E731
        self.json.write_text(json.dumps({"group": "tracks", "dims": ["event", "var"], "var_names": list(VAR_NAMES), "names": list(names),
                                         "time": lst(time), "x": lst(x), "y": lst(y), "t_before": lst(t_before), "t_after": lst(t_after)}))


class H5TrackStore:
    format = "hdf5"

    def __init__(self, path, name):
        h = self.h5 = H5File(path, name, "tracks")
        self.dir, self.path = h.dir, h.path

    def close(self, data, time, x, y, t_before, t_after, names):
        h = self.h5
        if h.file is None:
            return
        h.f64("data", np.ascontiguousarray(np.asarray(data).T))        # (var, event)
        h.strings("dims", ["event", "var"], attribute=True)
        h.strings("var_names", list(VAR_NAMES))
        h.strings("names", list(names))
        for k, a in (("time", time), ("x", x), ("y", y), ("t_before", t_before), ("t_after", t_after)):
            h.f64(k, np.asarray(a, dtype=np.float64))
        h.close()


def make_track_store(path, name, format="auto"):
    return choose_format(format, "track output", lambda: H5TrackStore(path, name), lambda: NpyTrackStore(path, name))


class TrackWriter(OutputWriter):
    """TrackWriter(model, times=[t, ...], points=[(x, y), ...], names=None, path=".", name="tracks", format="auto")"""

    kind = "tracks"
    needs = "track_init"
    refusal = "a TrackWriter needs a backend with track_init / track_sample / track_fetch_begin / track_fetch_end (the HIP library, ABI 14)"

    def __init__(self, model=None, *, times, points, names=None, path=".", name="tracks", format="auto"):
        if type(model).__name__ == "SlabModel":
            raise NotImplementedError("TrackWriter: slabs do not carry a track set (the corners of an event may lie on two ranks): "
                                      "use a whole-grid model")
        self.model = model
        self.times = np.asarray(times, dtype=np.float64).reshape(-1)
        self.points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        n = len(self.times)
        if n < 1 or len(self.points) != n:
            raise ValueError("TrackWriter: times and points must name the same events, at least one")
        if not np.isfinite(self.times).all():
            raise ValueError("TrackWriter: event times must be finite")
        self.names = [f"event_{k}" for k in range(n)] if names is None else [str(s) for s in names]
        if len(self.names) != n:
            raise ValueError("TrackWriter: one name per event")
        self.path, self.name, self.format = Path(path), name, format
        # the library's order: by time, ties in the caller's order; order[k] = the caller's index of sorted event k
        self.order = np.argsort(self.times, kind="stable")
        self.sorted_times = self.times[self.order]
        self.store = None
        self._set_on = None
        self._grid = None
        self.H = None
        if model is not None:
            self._locate(model.grid)

    def _locate(self, grid):
        corners, weights = locate_points_fast(grid, self.points[self.order])
        # the library's planes: ij[c m + k] = i, ij[(4 + c) m + k] = j of corner c of sorted event k; w[c m + k]
        self.corners_ij = np.ascontiguousarray(np.concatenate([corners[:, :, 0].T, corners[:, :, 1].T], axis=0))
        self.weights = np.ascontiguousarray(weights.T)
        self._grid = grid

    def check_run(self, sim, writers, store=False, cash_store=False, pickup=False):
        if type(sim.model).__name__ == "SlabModel":
            raise NotImplementedError("TrackWriter: slabs do not carry a track set (the corners of an event may lie on two ranks): "
                                      "use a whole-grid model")
        self.H = float(sim.Δt)          # the longest step run() will take

    def begin_run(self, model, n_steps: int):
        """(re)create the set, open the file and take the sample of the current state (the seeded one, or what a pickup restored)"""
        b = model.backend
        if self._grid is not model.grid:
            self._locate(model.grid)
        if self._set_on is b:
            b.track_free()
        if self.H is None:
            raise ValueError("TrackWriter: begin_run before check_run (the horizon is the run's Δt)")
        b.track_init(self.sorted_times, self.corners_ij, self.weights, self.H)
        self._set_on = b
        P = model.ODEsettings.Parameters
        self._g, self._r_g = P.get("g", 9.81), P["r_g"]
        self.store = make_track_store(self.path, self.name, format=self.format)
        self.table = np.full((8, len(self.times)), np.nan)      # in the library's (sorted) order
        self.begun = 0          # events [0, begun) have been asked for; [fetched, begun) are in flight
        self.fetched = 0
        self._turned_at = None   # the library clock at which the latest turn was taken
        b.track_sample()

    # ---- the two things, in this order: end the fetch begun a chunk earlier, begin the one of the events completed since ----
    def _turn(self, backend, clock=None):
        if self.store is None:
            return
        self._turned_at = clock
        if self.begun > self.fetched:
            self.table[:, self.fetched:self.begun] = backend.track_fetch_end()
            self.fetched = self.begun
        done = len(self.times) if clock is None else int(np.searchsorted(self.sorted_times, clock, side="right"))
        if done > self.begun:
            backend.track_fetch_begin(self.begun, done - self.begun)
            self.begun = done

    def steps_allowed(self, backend, iteration: int) -> int:
        return NO_LIMIT          # the table is no ring: this writer never ends a chunk

    def after_chunk(self, backend):
        """a chunk has been enqueued: the library's clock shows where it ends"""
        self._turn(backend, backend.clock)

    def at_iteration(self, model, writers):
        """the per-step path; on the chunked path after_chunk has taken this clock's turn already"""
        clock = model.backend.clock
        if clock != self._turned_at:
            self._turn(model.backend, clock)

    def finish(self, backend, iteration=None):
        if self.store is None:
            return
        self._turn(backend)          # ends the open fetch, begins the rest ...
        self._turn(backend)          # ... and ends that
        backend.track_free()
        self._set_on = None
        rec = track_records(self.table, self.sorted_times, self._g, self._r_g)
        n = len(self.times)
        data, tb, ta = np.empty((n, len(VAR_NAMES))), np.empty(n), np.empty(n)
        data[self.order], tb[self.order], ta[self.order] = rec, self.table[3], self.table[7]      # back to the caller's order
        self.store.close(data, self.times, self.points[:, 0], self.points[:, 1], tb, ta, self.names)
        self.last_store, self.store = self.store, None


def read_track_output(path, name="tracks"):
    """either form: dict with `data` [var, event], `var_names`, `names`, `time`, `x`, `y`, `t_before`, `t_after` (arrays)"""
    d = Path(path)
    keys = ("time", "x", "y", "t_before", "t_after")
    if (d / f"{name}.json").exists():
        out = json.loads((d / f"{name}.json").read_text())
        out["data"] = np.ascontiguousarray(np.load(d / f"{name}.tracks.data.npy").T)
        for k in keys:
            out[k] = np.asarray(out[k], dtype=np.float64)
        return out
    return read_h5_group(d / f"{name}.h5", "tracks", f64=("data",) + keys, strings=("var_names", "names"), attrs=("dims",))
