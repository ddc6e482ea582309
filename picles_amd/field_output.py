"""FieldWriter: coarse wave fields (Hs, Tp, group velocity, ...) and global scalars on a schedule — the output a user of a wave
model takes home, formed on the device (picles_diag_*, include/picles_hip.h) instead of from full State snapshots on the host.
The reference derives the same quantities from `State` afterwards: Hs = 4 sqrt(e) (visualization/movie_2D.jl:49,162), the group
velocity of GetGroupVelocity (Operators/core_2D.jl:138-147) / PartitionOutput (examples/example_00_minimal_state_vector.jl:21-57),
mean_of_state and max_energy / max_cgx / max_cgy (Operators/TimeSteppers.jl:15-29).

Attach like the Checkpointer: `sim.output_writers["fields"] = FieldWriter(model, schedule=10, path="out", coarsen=(4, 4))`.
`run(sim)` then stays on the `picles_run_steps` path between outputs: a snapshot is pushed into the library's ring at every output
iteration and popped — waited for and written — only when the ring is full or the run ends, so the copy to the host and the file
write of output k run beside the steps that follow it.  The record of the run's first iteration (the seeded state) is written too,
as `run(sim, store=True)` writes it.

File, following the conventions of picles_amd/storing.py (HDF5 datasets are row-major, i.e. the reverse of the Julia order):

    /waves/data           float32 (field, y, x, time)         NaN where a coarse cell holds no wet node
    /waves/x, /waves/y    float64: mean coordinate of the nodes a coarse cell covers;  /waves/time float64
    /waves/var_names      the fields, in plane order (a subset of hs, tp, cg_x, cg_y, e, m_x, m_y)
    /waves/scalars        float64 (time, 8);  /waves/scalar_names = sum_e, sum_mx, sum_my, n_wet, max_e, max_mx, max_my, mean_of_state

written as `<name>.h5` where a libhdf5 loads, else as `<name>.waves.data.npy` [time, x, y, field] + `<name>.waves.scalars.npy`
[time, 8] + `<name>.json` (the same logical layout, like NpyStateStore).
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from . import _capi as K
from .checkpointing import IterationInterval
from .driver import SCALAR_NAMES, combine_partials, diag_field_mask
from .output_writers import OutputWriter
from .storing import H5File, choose_format


def coarse_coordinate(x, c: int):
    """mean coordinate of the nodes each coarse cell covers (the last cell may cover fewer than c)"""
    x = np.asarray(x, dtype=np.float64)
    return np.array([x[k:k + c].mean() for k in range(0, len(x), c)])


class NpyFieldStore:
    """group, scalar_names: what a sibling product (picles_amd/flux_output.py) changes; `extra`: further entries of the side-car"""

    format = "npy"
    group = "waves"
    scalar_names = SCALAR_NAMES

    def __init__(self, path, name, time, x, y, var_names, extra=None):
        self.dir = Path(path)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.shape = (len(time), len(x), len(y), len(var_names))
        self.path = self.dir / f"{name}.{self.group}.data.npy"
        self.data = np.lib.format.open_memmap(self.path, mode="w+", dtype=np.float32, shape=self.shape)
        self.scalars = np.lib.format.open_memmap(self.dir / f"{name}.{self.group}.scalars.npy", mode="w+", dtype=np.float64,
                                                 shape=(len(time), len(self.scalar_names)))
        self.data[:] = np.nan
        self.scalars[:] = np.nan
        self.json = self.dir / f"{name}.json"
        self.meta = {"group": self.group, "dims": ["time", "x", "y", "field"], "var_names": list(var_names),
                     "scalar_names": list(self.scalar_names), "time": [float("nan")] * len(time), "x": list(map(float, x)),
                     "y": list(map(float, y))}
        self.meta.update(extra or {})

    def write(self, i, fields, scalars, time):
        self.data[i] = np.moveaxis(fields, 0, -1)
        self.scalars[i] = scalars
        self.meta["time"][i] = float(time)

    def close(self):
        self.data.flush()
        self.scalars.flush()
        self.json.write_text(json.dumps(self.meta))


class H5FieldStore:
    """the HDF5 form, through the file layer of picles_amd/storing.py"""

    format = "hdf5"
    group = "waves"
    scalar_names = SCALAR_NAMES

    def __init__(self, path, name, time, x, y, var_names, extra=None):
        h = self.h5 = H5File(path, name, self.group)
        self.dir, self.path = h.dir, h.path
        nt, nx, ny, nf = self.shape = (len(time), len(x), len(y), len(var_names))
        self.data = h.sliced("data", (nf, ny, nx, nt), np.float32)
        self.data.fill(np.nan)
        h.strings("dims", ["time", "x", "y", "field"], attribute=True)
        h.f64("x", x)
        h.f64("y", y)
        h.strings("var_names", list(var_names))
        h.strings("scalar_names", list(self.scalar_names))
        for k, v in (extra or {}).items():          # lists of strings become string datasets, numbers float64 datasets
            if isinstance(v, (list, tuple)) and v and isinstance(v[0], str):
                h.strings(k, list(v))
            else:
                h.f64(k, np.atleast_1d(np.asarray(v, dtype=np.float64)))
        self.times = np.full(nt, np.nan)
        self.scalars = np.full((nt, len(self.scalar_names)), np.nan)

    def write(self, i, fields, scalars, time):
        # (field, y, x): a no-op for the planes as popped
        self.data.write(i, np.ascontiguousarray(np.asarray(fields, dtype=np.float32).transpose(0, 2, 1)))
        self.scalars[i] = scalars
        self.times[i] = time

    def close(self):
        if self.h5.file is None:
            return
        self.h5.f64("time", self.times)
        self.h5.f64("scalars", self.scalars)
        self.h5.close()


def make_field_store(path, name, time, x, y, var_names, format="auto"):
    return choose_format(format, "field output", lambda: H5FieldStore(path, name, time, x, y, var_names),
                         lambda: NpyFieldStore(path, name, time, x, y, var_names))


class FieldWriter(OutputWriter):
    """FieldWriter(model, schedule=IterationInterval(N) | N, path=..., coarsen=(cx, cy), fields=("hs", "tp", "cg_x", "cg_y"))"""

    kind = "fields"
    needs = "diag_init"
    refusal = "a FieldWriter needs a backend with diag_init / diag_push / diag_pop (the HIP library)"
    sized_for_run = True

    def __init__(self, model=None, *, schedule=None, path=".", name="fields", coarsen=(4, 4), fields=("hs", "tp", "cg_x", "cg_y"),
                 format="auto", slots=3):
        if schedule is None:
            raise ValueError("FieldWriter needs a schedule (IterationInterval(N) or N)")
        self.model = model
        self.schedule = IterationInterval.of(schedule)
        self.path, self.name, self.format = Path(path), name, format
        self.coarsen = (int(coarsen), int(coarsen)) if np.isscalar(coarsen) else (int(coarsen[0]), int(coarsen[1]))
        mask = diag_field_mask(fields)
        self.fields = tuple(f for f in K.DIAG_FIELDS if mask & K.DIAG_BITS[f])      # plane order
        self.slots = int(slots)
        self.store = None
        self.written = 0              # records in the file so far
        self.iterations = []          # the iteration of every record pushed, in order
        self._initialised = None      # the backend whose ring was set up

    def begin_run(self, model, n_steps: int):
        """set the ring up (once per backend), open the file for this run and push the record of the current iteration"""
        b = model.backend
        if self._initialised is not b:
            b.diag_init(self.coarsen, self.fields, self.slots)
            self._initialised = b
        g = model.grid
        self.Nx, self.Ny = int(g.stats.Nx), int(g.stats.Ny)
        nt = self.schedule.records_of(model.clock.iteration, n_steps)
        x, y = coarse_coordinate(g.data.x[:, 0], self.coarsen[0]), coarse_coordinate(g.data.y[0, :], self.coarsen[1])
        self.store = make_field_store(self.path, self.name, np.zeros(nt), x, y, self.fields, format=self.format)
        self.written = 0
        self.iterations = []
        self.push(b, model.clock.iteration)

    def steps_allowed(self, backend, iteration: int) -> int:
        return self.schedule.next_after(iteration) - iteration

    def at_iteration(self, model, writers):
        if self.schedule(model.clock.iteration):
            self.push(model.backend, model.clock.iteration)

    def push(self, backend, iteration: int):
        """snapshot now; a full ring first gives up its oldest snapshot (waited for and written)"""
        if backend.diag_pending >= self.slots:
            self.drain(backend, 1)
        backend.diag_push()
        self.iterations.append(int(iteration))

    def drain(self, backend, count=None):
        """pop and write `count` snapshots (all that are pending when None)"""
        while backend.diag_pending > 0 and (count is None or count > 0):
            f, p, t = backend.diag_pop()
            s = combine_partials([p], self.Nx, self.Ny)
            self.store.write(self.written, f, [s[k] for k in SCALAR_NAMES], t)
            self.written += 1
            if count is not None:
                count -= 1

    def finish(self, backend, iteration=None):
        """end of the run: write what is pending and close the file"""
        if self.store is None:
            return
        self.drain(backend)
        self.store.close()
        self.last_store, self.store = self.store, None


def read_field_output(path, name="fields"):
    """read the .npy + .json form back: dict with `data` [time, x, y, field], `scalars` [time, 8] and the side-car's entries"""
    d = Path(path)
    out = json.loads((d / f"{name}.json").read_text())
    out["data"] = np.load(d / f"{name}.waves.data.npy")
    out["scalars"] = np.load(d / f"{name}.waves.scalars.npy")
    return out
