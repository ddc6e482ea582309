"""FluxWriter: the coupling fluxes on a schedule — what the partner models of a coupled system consume, formed on the device
(picles_flux_*, include/picles_hip.h "coupling fluxes"): the energy and momentum the waves take out of the wind (phi_in, tq_in: the
wave-supported stress, WAVEWATCH III's taw), what the breaking waves hand down to the ocean (phi_dis, tq_dis: phioc, two) and the
surface Stokes drift of the peak wave (us: uss), as area means over coarse cells, with the area totals of the grid.

Attach like the FieldWriter: `sim.output_writers["fluxes"] = FluxWriter(model, schedule=10, path="out", coarsen=(4, 4))`.  It sits on
the writer protocol and the file layer the FieldWriter sits on: `run(sim)` stays on the `picles_run_steps` path
between outputs, a snapshot is pushed into the library's ring at every output iteration and popped — waited for and written — only
when the ring is full or the run ends.  The record of the run's first iteration is written too; a picked-up run writes the record of
the iteration it picks up at and continues the schedule, which is counted in model iterations.

`rho_water` sets the scales of the planes: the three phi planes come in W m-2 (scale_phi = rho_water * g), the four tq planes in
N m-2 (scale_tau = rho_water); the Stokes drift is in m s-1.  Land and calm nodes count as zero in a cell's mean: the partner model
applies its own sea fraction.  The planes hold no NaN.

File (HDF5 datasets are row-major, i.e. the reverse of the Julia order):

    /fluxes/data            float32 (field, y, x, time)
    /fluxes/x, /fluxes/y    float64: mean coordinate of the nodes a coarse cell covers;  /fluxes/time float64
    /fluxes/var_names       the planes, in plane order (a subset of phi_in, phi_dis, phi_shift, tq_in_x, tq_in_y, tq_dis_x, tq_dis_y,
                            us_x, us_y);  /fluxes/units  one entry per plane
    /fluxes/scalars         float64 (time, 11);  /fluxes/scalar_names = sum_<plane> x 9 (UNSCALED node sums of the whole grid:
                            times the node's area and the plane's scale for the integrated flux), n_active, n_bad
    /fluxes/rho_water, scale_phi, scale_tau

written as `<name>.h5` where a libhdf5 loads, else as `<name>.fluxes.data.npy` [time, x, y, field] + `<name>.fluxes.scalars.npy`
[time, 11] + `<name>.json` (the same logical layout).  `read_flux_output` reads either form back.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

from . import _capi as K
from .checkpointing import IterationInterval
from .driver import combine_flux_partials, flux_field_mask
from .field_output import FieldWriter, H5FieldStore, NpyFieldStore, coarse_coordinate
from .storing import choose_format, read_h5_group

G0 = 9.81                                  # the g of the right-hand side (physics.h PK_G0)
SCALAR_NAMES = K.FLUX_PARTIAL
UNITS = {f: "W m-2" if f.startswith("phi") else "N m-2" if f.startswith("tq") else "m s-1" for f in K.FLUX_FIELDS}


class NpyFluxStore(NpyFieldStore):
    group = "fluxes"
    scalar_names = SCALAR_NAMES


class H5FluxStore(H5FieldStore):
    group = "fluxes"
    scalar_names = SCALAR_NAMES


def make_flux_store(path, name, time, x, y, var_names, extra, format="auto"):
    return choose_format(format, "flux output", lambda: H5FluxStore(path, name, time, x, y, var_names, extra),
                         lambda: NpyFluxStore(path, name, time, x, y, var_names, extra))


class FluxWriter(FieldWriter):
    """FluxWriter(model, schedule=IterationInterval(N) | N, path=..., coarsen=(cx, cy), fields=(...), rho_water=1025.0)"""

    kind = "fluxes"
    needs = "flux_init"
    refusal = "a FluxWriter needs a backend with flux_init / flux_push / flux_pop (the HIP library)"
    sized_for_run = True

    def __init__(self, model=None, *, schedule=None, path=".", name="fluxes", coarsen=(4, 4), fields=K.FLUX_FIELDS, rho_water=1025.0,
                 format="auto", slots=3):
        if schedule is None:
            raise ValueError("FluxWriter needs a schedule (IterationInterval(N) or N)")
        if not (np.isfinite(rho_water) and rho_water > 0.0):
            raise ValueError("FluxWriter: rho_water must be finite and positive")
        self.model = model
        self.schedule = IterationInterval.of(schedule)
        self.path, self.name, self.format = Path(path), name, format
        self.coarsen = (int(coarsen), int(coarsen)) if np.isscalar(coarsen) else (int(coarsen[0]), int(coarsen[1]))
        mask = flux_field_mask(fields)
        self.fields = tuple(f for f in K.FLUX_FIELDS if mask & K.FLUX_BITS[f])      # plane order
        self.rho_water = float(rho_water)
        self.scale_phi, self.scale_tau = self.rho_water * G0, self.rho_water
        self.slots = int(slots)
        self.store = None
        self.written = 0
        self.iterations = []
        self._initialised = None
        self._dt = None

    def check_run(self, sim, writers, store=False, cash_store=False, pickup=False):
        self._dt = float(sim.Δt)          # begin_run hands the model the window of the step to come

    def begin_run(self, model, n_steps: int):
        """set the ring up (once per backend), open the file for this run and push the record of the current iteration"""
        b = model.backend
        # the first record reads the wind level at the clock.  A run picked up under wind closures that vary in time restores a context
        # whose window is an earlier step's: the window of the step to come — the one the first time_step uploads, kept by the model —
        # starts at the clock.  (Static winds, a lattice and a stream: nothing is uploaded twice.)
        if self._dt is not None and hasattr(model, "upload_winds"):
            model.upload_winds(model.clock.time, self._dt)
        if self._initialised is not b:
            b.flux_init(self.coarsen, self.fields, self.scale_phi, self.scale_tau, self.slots)
            self._initialised = b
        g = model.grid
        nt = self.schedule.records_of(model.clock.iteration, n_steps)
        x, y = coarse_coordinate(g.data.x[:, 0], self.coarsen[0]), coarse_coordinate(g.data.y[0, :], self.coarsen[1])
        extra = {"units": [UNITS[f] for f in self.fields], "rho_water": self.rho_water, "scale_phi": self.scale_phi, "scale_tau": self.scale_tau}
        self.store = make_flux_store(self.path, self.name, np.zeros(nt), x, y, self.fields, extra, format=self.format)
        self.written = 0
        self.iterations = []
        self.push(b, model.clock.iteration)

    def push(self, backend, iteration: int):
        """snapshot now; a full ring first gives up its oldest snapshot (waited for and written)"""
        if backend.flux_pending >= self.slots:
            self.drain(backend, 1)
        backend.flux_push()
        self.iterations.append(int(iteration))

    def drain(self, backend, count=None):
        """pop and write `count` snapshots (all that are pending when None)"""
        while backend.flux_pending > 0 and (count is None or count > 0):
            f, p, t = backend.flux_pop()
            s = combine_flux_partials([p])
            self.store.write(self.written, f, [s[k] for k in SCALAR_NAMES], t)
            self.written += 1
            if count is not None:
                count -= 1


MEAN_SIDECAR_SUFFIX = ".fluxmeans.npz"


class MeanFluxWriter(FluxWriter):
    """MeanFluxWriter(model, schedule=N, every=1, path=..., name="flux_means", coarsen=(cx, cy), fields=(...), rho_water=1025.0):
    the coupling fluxes as INTERVAL MEANS (picles_flux_mean_*, include/picles_hip.h "flux means"), which is what a coupler exchanges.
    The device adds the cell sums of the fluxes to its accumulators behind every `every`-th model step — iterations that are
    multiples of `every`; N % every == 0 is required — while run() stays on the fused picles_run_steps path; at every iteration that
    is a multiple of N the mean over the samples of the N steps before it is pushed into the flux ring and the accumulators start
    afresh (picles_flux_mean_push with reset = 1).  The chunks of run() end there, as a FieldWriter's do; the copy-out and the
    file write overlap the next chunk.  There is NO record at the starting iteration, and samples left over when the run ends — a
    run whose last iteration is no multiple of N — are DISCARDED: no record is written for an interval that did not complete.

    The file layout is FluxWriter's, with `averaged = true` and `samples_per_record = N / every`; `scalars` are the combined tile
    partials divided by the number of samples: the interval means of the unscaled node sums (and of n_active, n_bad).
    read_flux_output(path, name="flux_means") reads it.  A record's time is the clock at the end of its interval.

    Restart: a Checkpointer's checkpoint gets the raw accumulators and n_samples, t_first, t_last as a side-car next to it
    (`<file>.fluxmeans.npz`); a picked-up run uploads them (picles_flux_mean_set) and writes the records of the uninterrupted run bit
    for bit.  A missing or foreign side-car starts the open interval afresh with a warning.

    A FluxWriter and a MeanFluxWriter on one model would share one ring and pop each other's records: run() refuses the pair."""

    kind = "flux_means"
    needs = "flux_mean_init"
    refusal = "a MeanFluxWriter needs a backend with flux_mean_init / flux_mean_push / flux_pop (the HIP library)"

    def __init__(self, model=None, *, schedule=None, every=1, path=".", name="flux_means", coarsen=(4, 4), fields=K.FLUX_FIELDS,
                 rho_water=1025.0, format="auto", slots=3):
        if schedule is None:
            raise ValueError("MeanFluxWriter needs a schedule (IterationInterval(N) or N)")
        super().__init__(model, schedule=schedule, path=path, name=name, coarsen=coarsen, fields=fields, rho_water=rho_water,
                         format=format, slots=slots)
        self.every = int(every)
        if self.every < 1 or self.schedule.interval % self.every != 0:
            raise ValueError(f"MeanFluxWriter: every = {every} must be >= 1 and divide the schedule ({self.schedule.interval}): "
                             "a record is the mean over whole sampling intervals")
        self.samples_per_record = self.schedule.interval // self.every
        self._set_on = None           # the backend that holds this writer's mean set
        self._restore = None          # accumulators a pickup handed over, uploaded by begin_run
        self._samples = []            # n_samples of every record pushed and not yet written

    def check_run(self, sim, writers, store=False, cash_store=False, pickup=False):
        if any(getattr(w, "kind", None) == "fluxes" for w in writers):
            raise ValueError("a FluxWriter and a MeanFluxWriter on one model share the one flux ring of the library and would pop each "
                             "other's records: attach one of them (snapshots and means side by side are not supported)")
        super().check_run(sim, writers, store=store, cash_store=cash_store, pickup=pickup)

    def records_of(self, it0: int, n_steps: int) -> int:
        N = self.schedule.interval
        return (it0 + n_steps) // N - it0 // N

    def begin_run(self, model, n_steps: int):
        """set the ring up (once per backend), (re)create the mean set with the cadence continued from the model's iteration, open
        the file and, after a pickup, upload the open interval.  No record is pushed here"""
        b = model.backend
        if self._initialised is not b:
            b.flux_init(self.coarsen, self.fields, self.scale_phi, self.scale_tau, self.slots)
            self._initialised = b
        if self._set_on is b:
            b.flux_mean_free()
        it0 = int(model.clock.iteration)
        b.flux_mean_init(every=self.every, first=self.every - it0 % self.every)
        self._set_on = b
        g = model.grid
        x, y = coarse_coordinate(g.data.x[:, 0], self.coarsen[0]), coarse_coordinate(g.data.y[0, :], self.coarsen[1])
        extra = {"units": [UNITS[f] for f in self.fields], "rho_water": self.rho_water, "scale_phi": self.scale_phi, "scale_tau": self.scale_tau,
                 "averaged": True, "samples_per_record": self.samples_per_record}
        self.store = make_flux_store(self.path, self.name, np.zeros(self.records_of(it0, n_steps)), x, y, self.fields, extra, format=self.format)
        self.written = 0
        self.iterations = []
        self._samples = []
        if self._restore is not None:
            # (a checkpoint taken AT a record's iteration is taken before the record is pushed: its interval was written by the
            # run that stopped, and the open interval of this one is empty)
            if it0 % self.schedule.interval != 0:
                b.flux_mean_set(self._restore)
            self._restore = None

    def push(self, backend, iteration: int):
        """the mean of the interval that ends here, then zero; an interval without a sample leaves no record"""
        n = backend.flux_mean_scalars()[0]
        if n == 0:
            return
        if backend.flux_pending >= self.slots:
            self.drain(backend, 1)
        backend.flux_mean_push(reset=True)
        self.iterations.append(int(iteration))
        self._samples.append(n)

    def drain(self, backend, count=None):
        while backend.flux_pending > 0 and (count is None or count > 0):
            f, p, t = backend.flux_pop()
            s, n = combine_flux_partials([p]), self._samples.pop(0)
            self.store.write(self.written, f, [s[k] / n for k in SCALAR_NAMES], t)
            self.written += 1
            if count is not None:
                count -= 1

    def finish(self, backend, iteration=None):
        super().finish(backend, iteration)
        if self._set_on is not None:      # samples of an interval that did not complete go with the set
            backend.flux_mean_free()
            self._set_on = None

    # ---- pickup ----
    def checkpoint_begun(self, backend, checkpoint_file):
        """the raw accumulators of the open interval next to a checkpoint file (atomic, like the file itself)"""
        import os
        acc = backend.flux_mean_get()
        path = Path(str(checkpoint_file) + MEAN_SIDECAR_SUFFIX)
        path.parent.mkdir(parents=True, exist_ok=True)
        tmp = path.with_name(f".{path.name}.tmp-{os.getpid()}.npz")
        np.savez(tmp, acc=np.asarray(acc["acc"]), n_samples=np.int64(acc["n_samples"]), t_first=np.float64(acc["t_first"]),
                 t_last=np.float64(acc["t_last"]), coarsen=np.asarray(self.coarsen, dtype=np.int64), every=np.int64(self.every),
                 schedule=np.int64(self.schedule.interval))
        os.replace(tmp, path)
        return path

    def load_pickup(self, checkpoint_file):
        """remember the accumulators stored next to `checkpoint_file` for begin_run; a missing or foreign side-car starts the open
        interval afresh with a warning"""
        import warnings
        path = Path(str(checkpoint_file) + MEAN_SIDECAR_SUFFIX)
        self._restore = None
        if not path.exists():
            warnings.warn(f"MeanFluxWriter: no flux-mean side-car {path.name} next to the checkpoint: the open interval starts afresh")
            return False
        with np.load(path) as z:
            acc = {k: z[k] for k in z.files}
        same = (tuple(int(v) for v in acc.get("coarsen", ())) == self.coarsen and int(acc.get("every", -1)) == self.every
                and int(acc.get("schedule", -1)) == self.schedule.interval and np.ndim(acc.get("acc")) == 3)
        if not same:
            warnings.warn(f"MeanFluxWriter: the side-car {path.name} was written with another coarsening, sampling or schedule: "
                          "the open interval starts afresh")
            return False
        self._restore = dict(acc=acc["acc"], n_samples=int(acc["n_samples"]), t_first=float(acc["t_first"]), t_last=float(acc["t_last"]))
        return True


def read_flux_output(path, name="fluxes"):
    """read either form back: dict with `data` [time, x, y, field], `scalars` [time, 11], `time`, `x`, `y`, `var_names`, `units`,
    `scalar_names`, `dims`, `rho_water`, `scale_phi`, `scale_tau`; a MeanFluxWriter's file (name="flux_means") also has `averaged`
    and `samples_per_record`"""
    d = Path(path)
    if (d / f"{name}.json").exists():
        out = json.loads((d / f"{name}.json").read_text())
        out["data"] = np.load(d / f"{name}.fluxes.data.npy")
        out["scalars"] = np.load(d / f"{name}.fluxes.scalars.npy")
        return out
    out = read_h5_group(d / f"{name}.h5", "fluxes", f64=("data", "time", "x", "y", "scalars", "rho_water", "scale_phi", "scale_tau"),
                        strings=("var_names", "units", "scalar_names"), attrs=("dims",),
                        optional_f64=("averaged", "samples_per_record"))      # the two entries a MeanFluxWriter adds
    out["data"] = out["data"].transpose(3, 2, 1, 0).astype(np.float32)       # file (field, y, x, time) -> [time, x, y, field]
    for k in ("time", "x", "y"):
        out[k] = out[k].tolist()
    for k in ("rho_water", "scale_phi", "scale_tau"):
        out[k] = float(out[k][0])
    if "averaged" in out:
        out["averaged"], out["samples_per_record"] = bool(out["averaged"][0]), int(out["samples_per_record"][0])
    return out
