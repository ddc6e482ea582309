"""StatisticsWriter: run statistics — per-node maps of the storm peak, the mean sea state and the share of time above height
thresholds, over the whole run or over windows of it, without leaving the fused stepping path.  The fourth product of a wave model
beside restart files (picles_amd/checkpointing.py), gridded fields (picles_amd/field_output.py) and station series
(picles_amd/station_output.py).

The library folds the State value of every node into per-node accumulators on the device behind each scheduled step
(picles_stat_*, include/picles_hip.h "run statistics": from the records of the pending fused step, which stays pending); State
never crosses PCIe.  `run(sim)` stays on `picles_run_steps`, in chunks that end where a window, a checkpoint or another writer's
output falls.  At the end of a window the writer gets the accumulators, derives the record, and resets them.

Attach like the other writers:
`sim.output_writers["statistics"] = StatisticsWriter(model, fields=("peak", "mean", "exceed"), thresholds=(2.0, 4.0), schedule=1,
window=None, path="out")`.  `schedule` is the sampling cadence in iterations (a sample at every iteration that is a multiple of
it); `window` the number of iterations per output record (records end at the iterations that are multiples of it; None: one
record at the end of the run).  A window that is still open when the run ends is written as the last record.

THE ACCUMULATORS are those of the header: per node and WET sample (e, m_x, m_y finite, e > 0, m_x*m_x + m_y*m_y > 0)
n_wet += 1; "peak": (e_peak, mx_peak, my_peak, t_peak) replaced by the sample and its clock on the first wet sample or when
e > e_peak; "mean": sum_e, sum_mx, sum_my, sum_hs with hs = 4.0 * sqrt(e); "exceed": n_exc[k] += 1 when hs >= thresholds[k].
n_samples counts the samples of the window, wet or not.

DERIVED VARIABLES, per node, in NumPy fp64, every operation one IEEE operation in the order written (`derive`), with n = n_wet as
a double, N = n_samples as a double, and g, r_g of the model's ODE parameters:

    "peak":    hs_max     = 4.0 * sqrt(e_peak)
               M2 = mx_peak * mx_peak + my_peak * my_peak;  cbar = e_peak / (2.0 * sqrt(M2))
               tp_at_max  = (FOUR_PI * max(cbar / r_g, 0.1)) / g          FOUR_PI = 12.566370614359172  (the header's tp)
               dir_at_max = atan2(my_peak, mx_peak)
               t_of_max   = t_peak
    "mean":    e_mean = sum_e / n;  hs_mean = sum_hs / n;  mx_mean = sum_mx / n;  my_mean = sum_my / n
               dir_mean   = atan2(sum_my, sum_mx)
    always:    wet_fraction = n / N
    "exceed":  exceed_k   = n_exc[k] / N          (k = 0 ... number of thresholds - 1)

Where n_wet == 0 the values are NaN and the fractions 0.0 (also when N == 0).  The variables come in the order above.

FILE, following picles_amd/field_output.py: where a libhdf5 loads `<name>.h5` with

    /stats/data          float64 (var, y, x, window)        /stats/names = the variable names
    /stats/x, y          float64 node coordinates           /stats/thresholds   float64
    /stats/t_start, t_end  float64: the clocks of the first and the last sample of each window
    /stats/iteration     float64 (whole numbers): the iteration each window ended at      /stats/n_samples  float64

else `<name>.stats.data.npy` (the same array) + `<name>.json` (the same logical layout).  `read_statistics(path)` reads either.

PICKUP.  When the Checkpointer writes iteration i the writer stores its raw accumulators next to that file
(`<checkpoint file>.stats.npz`); `run(sim, pickup=True)` uploads them again (picles_stat_set), so that a picked-up run continues
its open window.  A missing side-car starts a fresh window with a warning.
"""
from __future__ import annotations

import json
import math
import os
import warnings
from pathlib import Path

import numpy as np

from .checkpointing import IterationInterval
from .output_writers import NO_LIMIT, OutputWriter
from .station_output import FOUR_PI, peak_period          # noqa: F401  (FOUR_PI: the docstring's constant, importable from here)
from .storing import H5File, check_format, choose_format, read_h5_group

GROUPS = ("peak", "mean", "exceed")
GROUP_BITS = {"peak": 1, "mean": 2, "exceed": 4}
PEAK_VARS = ("hs_max", "tp_at_max", "dir_at_max", "t_of_max")
MEAN_VARS = ("e_mean", "hs_mean", "mx_mean", "my_mean", "dir_mean")
SIDECAR_SUFFIX = ".stats.npz"


def check_arguments(fields, thresholds, schedule, window):
    """what the library would refuse, refused before it is reached: -> (fields in canonical order, thresholds, schedule, window)"""
    if isinstance(fields, str):
        fields = (fields,)
    fields = tuple(fields)
    unknown = [f for f in fields if f not in GROUPS]
    if unknown or not fields:
        raise ValueError(f"StatisticsWriter: fields must be a non-empty selection of {GROUPS}, got {fields}")
    fields = tuple(g for g in GROUPS if g in fields)
    thr = tuple(float(t) for t in thresholds)
    if "exceed" in fields:
        if not 1 <= len(thr) <= 4:
            raise ValueError("StatisticsWriter: 'exceed' takes 1 ... 4 thresholds")
        if any(not math.isfinite(t) or not t > 0.0 for t in thr) or any(not b > a for a, b in zip(thr, thr[1:])):
            raise ValueError("StatisticsWriter: thresholds must be finite, positive and strictly ascending")
    elif thr:
        raise ValueError("StatisticsWriter: thresholds given without 'exceed'")
    return fields, thr, IterationInterval.of(schedule), (None if window is None else IterationInterval.of(window))


def var_names(fields, n_thresholds):
    return ((PEAK_VARS if "peak" in fields else ()) + (MEAN_VARS if "mean" in fields else ()) + ("wet_fraction",)
            + (tuple(f"exceed_{k}" for k in range(n_thresholds)) if "exceed" in fields else ()))


def derive(acc, g, r_g):
    """the accumulators of stat_get -> {variable: plane shaped like the accumulators}, by the module docstring's arithmetic"""
    nw = acc["n_wet"]
    dry = nw == 0
    n = nw.astype(np.float64)
    N = np.float64(acc["n_samples"])
    out = {}
    with np.errstate(all="ignore"):
        if "e_peak" in acc:
            e, mx, my = acc["e_peak"], acc["mx_peak"], acc["my_peak"]
            out["hs_max"] = 4.0 * np.sqrt(e)
            M2 = mx * mx + my * my
            cbar = e / (2.0 * np.sqrt(M2))
            out["tp_at_max"] = peak_period(cbar, g, r_g)
            out["dir_at_max"] = np.arctan2(my, mx)
            out["t_of_max"] = acc["t_peak"].copy()
        if "sum_e" in acc:
            out["e_mean"] = acc["sum_e"] / n
            out["hs_mean"] = acc["sum_hs"] / n
            out["mx_mean"] = acc["sum_mx"] / n
            out["my_mean"] = acc["sum_my"] / n
            out["dir_mean"] = np.arctan2(acc["sum_my"], acc["sum_mx"])
        for v in out.values():
            v[dry] = np.nan
        out["wet_fraction"] = np.where(dry, 0.0, n / N)
        if "n_exc" in acc:
            for k in range(acc["n_exc"].shape[-1]):
                c = acc["n_exc"][..., k]
                out[f"exceed_{k}"] = np.where(c == 0, 0.0, c.astype(np.float64) / N)
    return out


def _write_files(path, name, format, data, meta):
    """data (var, y, x, window); meta: names, x, y, thresholds, t_start, t_end, iteration, n_samples -> the path written"""
    d = Path(path)
    d.mkdir(parents=True, exist_ok=True)
    keys = ("x", "y", "thresholds", "t_start", "t_end", "iteration", "n_samples")

    def hdf5_form():
        h = H5File(d, name, "stats")
        h.f64("data", data)
        h.strings("dims", ["var", "y", "x", "window"], attribute=True)
        h.strings("names", list(meta["names"]))
        for k in keys:
            h.f64(k, np.asarray(meta[k], dtype=np.float64))
        h.close()
        return h.path, "hdf5"

    def npy_form():
        np.save(d / f"{name}.stats.data.npy", np.ascontiguousarray(data))
        js = {"group": "stats", "dims": ["var", "y", "x", "window"], "names": list(meta["names"])}
        for k in keys:
            js[k] = [float(v) for v in np.asarray(meta[k], dtype=np.float64)]
        (d / f"{name}.json").write_text(json.dumps(js))
        return d / f"{name}.json", "npy"

    return choose_format(format, "statistics output", hdf5_form, npy_form)


def read_statistics(path, name="statistics"):
    """either form: dict with `data` float64 (var, y, x, window), `names`, `x`, `y`, `thresholds`, `t_start`, `t_end`, `iteration`,
    `n_samples`; `path` is the writer's directory (or the file it wrote)"""
    d = Path(path)
    if d.is_file():
        name = d.name[:-len(".json")] if d.name.endswith(".json") else d.stem
        d = d.parent
    keys = ("x", "y", "thresholds", "t_start", "t_end", "iteration", "n_samples")
    if (d / f"{name}.json").exists():
        out = json.loads((d / f"{name}.json").read_text())
        out["data"] = np.load(d / f"{name}.stats.data.npy")
        for k in keys:
            out[k] = np.asarray(out[k], dtype=np.float64)
        return out
    out = read_h5_group(d / f"{name}.h5", "stats", f64=("data",) + keys, strings=("names",), attrs=("dims",))
    out["names"] = list(out["names"])
    return out


def variable(out, var):
    """the (y, x, window) block of one variable of read_statistics' result"""
    return out["data"][list(out["names"]).index(var)]


class StatisticsWriter(OutputWriter):
    """StatisticsWriter(model, fields=("peak", "mean", "exceed"), thresholds=(...), schedule=1, window=None | N, path=...,
    name="statistics")"""

    kind = "statistics"
    needs = "stat_init"
    refusal = "a StatisticsWriter needs a backend with stat_init / stat_get / stat_reset (the HIP library)"
    sized_for_run = True

    def __init__(self, model=None, *, fields=GROUPS, thresholds=(), schedule=1, window=None, path=".", name="statistics", format="auto"):
        self.fields, self.thresholds, self.schedule, self.window = check_arguments(fields, thresholds, schedule, window)
        check_format(format, "statistics output")
        self.model = model
        self.dir, self.name, self.format = Path(path), name, format
        self.path = self.dir
        self.mask = sum(GROUP_BITS[f] for f in self.fields)
        self.names = var_names(self.fields, len(self.thresholds))
        self.records = []             # (planes [var, y, x], t_start, t_end, iteration, n_samples) of every window written
        self._set_on = None           # the backend that holds this writer's statistics set
        self._restore = None          # accumulators a pickup handed over, uploaded by begin_run

    # ---- the cadence ----
    def steps_allowed(self, backend, iteration: int) -> int:
        """the distance to the iteration the open window ends at (where run() must end a chunk); a run without windows never ends one"""
        return self.window.next_after(iteration) - iteration if self.window is not None else NO_LIMIT

    # ---- the run ----
    def begin_run(self, model, n_steps: int):
        """(re)create the set with the cadence continued from the model's iteration and, after a pickup, upload the open window"""
        b = model.backend
        if self._set_on is b:
            b.stat_free()
        it0 = int(model.clock.iteration)
        b.stat_init(self.fields, self.thresholds, every=self.schedule.interval, first=self.schedule.first_step(it0))
        self._set_on = b
        P = model.ODEsettings.Parameters
        self._g, self._r_g = P.get("g", 9.81), P["r_g"]
        g = model.grid
        self._x, self._y = np.asarray(g.data.x)[:, 0].astype(np.float64), np.asarray(g.data.y)[0, :].astype(np.float64)
        self.records = []
        if self._restore is not None:
            b.stat_set(self._restore)
            self._restore = None

    def end_window(self, backend, iteration: int):
        """get, derive and keep the record, reset; a window without a sample leaves no record"""
        acc = backend.stat_get()
        if acc["n_samples"] == 0:
            return
        d = derive(acc, self._g, self._r_g)
        planes = np.stack([np.ascontiguousarray(d[n].T) for n in self.names])          # [var, y, x]
        self.records.append((planes, acc["t_first"], acc["t_last"], int(iteration), acc["n_samples"]))
        backend.stat_reset()

    def at_iteration(self, model, writers):
        """a window that ends here: get, write, reset"""
        if self.window is not None and self.window(model.clock.iteration):
            self.end_window(model.backend, model.clock.iteration)

    def finish(self, backend, iteration: int):
        if self._set_on is None:
            return
        self.end_window(backend, iteration)          # the window still open (the whole run when there are no windows)
        nv = len(self.names)
        if self.records:
            data = np.stack([r[0] for r in self.records], axis=-1)
        else:
            data = np.empty((nv, len(self._y), len(self._x), 0))
        meta = dict(names=self.names, x=self._x, y=self._y, thresholds=self.thresholds, t_start=[r[1] for r in self.records],
                    t_end=[r[2] for r in self.records], iteration=[r[3] for r in self.records], n_samples=[r[4] for r in self.records])
        self.file, self.written_format = _write_files(self.dir, self.name, self.format, data, meta)
        backend.stat_free()
        self._set_on = None

    # ---- pickup ----
    def checkpoint_begun(self, backend, checkpoint_file):
        """the raw accumulators of the open window next to a checkpoint file (atomic, like the file itself)"""
        acc = backend.stat_get()
        path = Path(str(checkpoint_file) + SIDECAR_SUFFIX)
        path.parent.mkdir(parents=True, exist_ok=True)
        tmp = path.with_name(f".{path.name}.tmp-{os.getpid()}.npz")
        arrays = {k: v for k, v in acc.items() if isinstance(v, np.ndarray)}
        np.savez(tmp, n_samples=np.int64(acc["n_samples"]), t_first=np.float64(acc["t_first"]), t_last=np.float64(acc["t_last"]),
                 mask=np.int64(self.mask), schedule=np.int64(self.schedule.interval), **arrays)
        os.replace(tmp, path)
        return path

    def load_pickup(self, checkpoint_file):
        """remember the accumulators stored next to `checkpoint_file` for begin_run; a missing or foreign side-car starts a fresh
        window with a warning"""
        path = Path(str(checkpoint_file) + SIDECAR_SUFFIX)
        self._restore = None
        if not path.exists():
            warnings.warn(f"StatisticsWriter: no statistics side-car {path.name} next to the checkpoint: the window starts afresh")
            return False
        with np.load(path) as z:
            acc = {k: z[k] for k in z.files}
        same = (int(acc["mask"]) == self.mask and int(acc["schedule"]) == self.schedule.interval
                and tuple(float(t) for t in acc["thresholds"]) == self.thresholds)
        if not same:
            warnings.warn(f"StatisticsWriter: the side-car {path.name} was written with other fields, thresholds or schedule: "
                          "the window starts afresh")
            return False
        for k in ("n_samples", "mask"):
            acc[k] = int(acc[k])
        for k in ("t_first", "t_last"):
            acc[k] = float(acc[k])
        self._restore = acc
        return True
