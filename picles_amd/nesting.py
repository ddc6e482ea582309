"""NestForcing: one-way nesting — a fine child box forced at its open rim by a coarser parent model that runs beside it, all on
the device.  The parent's State is sampled behind its step at the corner nodes that surround the child's forced nodes, mixed onto
them with the station definition of picles_amd/station_output.py and written into the level block of the child's forcing set in
stream order (picles_nest_*, include/picles_hip.h "one-way nesting"; the mix kernel is picles_amd/csrc/k_nest.h).  Nothing crosses
PCIe, the host waits for nothing, and both models stay on `picles_run_steps`.

Attach in the place of a BoundaryForcing (picles_amd/boundary_forcing.py):

    child_sim.output_writers["boundary_forcing"] = NestForcing(child_model, parent=parent_sim, side="rim", ratio=3)
    run(child_sim)

`run(child_sim)` drives both: the parent takes one step of `parent_sim.Δt` for every `ratio` steps of the child and stays one
step ahead of it, so that the child always steps between two parent levels.  The value a child step sees is BoundaryForcing's —
linear in t between the levels that bracket the step's start time, the later pair at a level itself; the window logic is that
class's own (`window_of`, `steps_allowed`), applied to the parent's clock values.  The parent's FieldWriter, StationWriter and
StatisticsWriter are driven through their hooks as run(parent_sim) would drive them, one step per chunk.

GEOMETRY.  The child's forced nodes are located in the parent from the child grid's own node coordinates with
`station_output.locate_points` (a node outside the parent is its ValueError); the distinct corner nodes are found on the host.
TIME.  `ratio` is an integer r >= 1 with |r Δt_child - Δt_parent| <= 1e-12 Δt_parent, and both clocks agree when the run begins.

THE OFFLINE ROUTE gives the same bits: run the parent alone with `StationWriter(points=rim_points(child_model, side=...))`, then the
child under `boundary_forcing.from_station_output(child_model, path, side=...)`.

Not for slabs, not together with a Checkpointer or `pickup=` (a restart of a pair whose parent is a step ahead is not defined yet),
and only where run() takes its chunked path on both models: static winds, no `store`, no `cash_store`.
"""
from __future__ import annotations

import numpy as np

from .boundary_forcing import BoundaryForcing, node_points, rim_nodes
from .output_writers import PHASE_ORDER, in_phase, writers_of
from .station_output import locate_points

RATIO_EPS = 1e-12          # |r Δt_child - Δt_parent| may be this fraction of Δt_parent


def rim_points(model, side=None, *, nodes=None, width=1):
    """the (x, y) of a model's forced nodes, in the order of its forcing set: the `points` of the StationWriter that records, in a
    parent run, what a NestForcing would hand the model (width > 1: the band of boundary_forcing.band_nodes)"""
    if (nodes is None) == (side is None):
        raise ValueError("rim_points needs either nodes=[(i, j), ...] or side=...")
    return node_points(model.grid, rim_nodes(model.grid, side, width) if nodes is None else nodes)


def locate_in_parent(parent_grid, points):
    """(corner_nodes int64 [n_corner, 2] distinct, index int64 [n, 4] into them, weights float64 [n, 4]) of points in the parent"""
    corners, weights = locate_points(parent_grid, points)
    corner_nodes, inv = np.unique(corners.reshape(-1, 2), axis=0, return_inverse=True)
    return corner_nodes, np.asarray(inv).reshape(corners.shape[:2]), weights


def _whole(ratio):
    if not (isinstance(ratio, (int, float, np.integer, np.floating)) and ratio == int(ratio) and ratio >= 1):
        raise ValueError(f"NestForcing: ratio must be an integer >= 1, not {ratio!r}")
    return int(ratio)


def check_ratio(ratio, dt_child, dt_parent):
    r = _whole(ratio)
    if not abs(r * dt_child - dt_parent) <= RATIO_EPS * dt_parent:
        raise ValueError(f"NestForcing: {r} child steps of {dt_child!r} s do not make one parent step of {dt_parent!r} s")
    return r


def _chunked(model, dt):
    """would run() take picles_run_steps on this model?  (time-constant winds; evaluated on the host, nothing is uploaded)"""
    return hasattr(model.backend, "run_steps") and bool(model._is_static(dt))


class NestForcing(BoundaryForcing):
    """NestForcing(child_model, parent=<Simulation>, nodes=[(i, j), ...] | side="west" | ... | "rim", ratio=r, Δt=None, width=1,
    weights=None | "linear" | array(n))
    Δt: the child's step, where it is not parent.Δt / ratio to the last bit; width, weights: BoundaryForcing's — a band as deep as
    the parent's fastest swell travels in a child step lets it enter"""

    kind = "boundary_forcing"
    needs = "nest_init"
    refusal = "a NestForcing needs a backend with nest_init / nest_sample (the HIP library)"

    def __init__(self, model, *, parent, nodes=None, side=None, ratio=1, Δt=None, width=1, weights=None):
        if type(model).__name__ == "SlabModel" or type(parent.model).__name__ == "SlabModel":
            raise NotImplementedError("NestForcing: slabs do not nest: use whole-grid models")
        if (nodes is None) == (side is None):
            raise ValueError("NestForcing needs either nodes=[(i, j), ...] or side=...")
        if parent.model is model:
            raise ValueError("NestForcing: the parent must be another model")
        self.model, self.parent = model, parent
        self._take_nodes(model, nodes, side, width, weights)
        self.dt = float(parent.Δt) / _whole(ratio) if Δt is None else float(Δt)
        self.ratio = check_ratio(ratio, self.dt, float(parent.Δt))
        self.corner_nodes, self.index, self.weights = locate_in_parent(parent.model.grid, node_points(model.grid, self.nodes))
        self.times = np.zeros(0)      # the parent's clock at every level taken, and behind them the time of the level to come
        self.values = None
        self.uploads = 0              # levels taken from the parent
        self.parent_steps = 0
        self._have = -1               # index into times of the latest level the library holds
        self._set_on = None
        self._k = None
        self._mark = None

    # ---- before anything is seeded ----
    def check_run(self, sim, writers, store=False, cash_store=False, pickup=False):
        super().check_run(sim, writers, store=store, cash_store=cash_store, pickup=pickup)
        pw = writers_of(self.parent)
        if pickup or any(w.kind == "checkpointer" for w in list(writers) + pw):
            raise NotImplementedError("NestForcing: a nested pair cannot be checkpointed or picked up yet (the parent is a step ahead of the "
                                      "child): run without a Checkpointer and without pickup=")
        if store or cash_store:
            raise NotImplementedError("NestForcing: run(child, store=True / cash_store=True) takes the per-step loop; a nest needs the chunked path")
        if sim.stop_time == float("inf"):
            raise ValueError("NestForcing needs a finite stop_time (the parent's steps are counted from the child's)")
        check_ratio(self.ratio, float(sim.Δt), float(self.parent.Δt))
        for m, dt, who in ((sim.model, sim.Δt, "child"), (self.parent.model, self.parent.Δt, "parent")):
            if not _chunked(m, dt):
                raise NotImplementedError(f"NestForcing: the {who} model would leave picles_run_steps (winds that vary in time, or a backend "
                                          "without run_steps): a nest needs static winds on both models")
        for w in pw:
            if not hasattr(self.parent.model.backend, w.needs):
                raise NotImplementedError(w.refusal)
        self.dt = float(sim.Δt)

    # ---- the parent, driven as run(parent) would drive it, one step per chunk ----
    def _parent_begin(self, n_parent):
        from .simulations import initialize_simulation
        ps, pm = self.parent, self.parent.model
        if not ps.initialized:
            initialize_simulation(ps)
        self._pw = writers_of(ps)
        self._pphase = {p: in_phase(self._pw, p) for p in PHASE_ORDER}
        pm.upload_winds(pm.clock.time, ps.Δt)
        self._ptime0, self._pit0, self.parent_steps = pm.clock.time, int(pm.clock.iteration), 0
        for w in self._pphase["begin_run"]:
            w.begin_run(pm, n_parent)

    def _parent_step(self, child_backend):
        """one fused step of the parent, which stays pending, and the level behind it"""
        ps, pm = self.parent, self.parent.model
        pb = pm.backend
        for w in self._pw:
            if w.steps_allowed(pb, self._pit0 + self.parent_steps) < 1:
                raise RuntimeError(f"NestForcing: the parent's {w.kind} writer allows no step")
        pb.run_steps(ps.Δt, 1)
        child_backend.nest_sample()
        for w in self._pphase["after_chunk"]:
            w.after_chunk(pb)
        self.parent_steps += 1
        pm.clock.time = self._ptime0 + self.parent_steps * ps.Δt
        pm.clock.iteration = self._pit0 + self.parent_steps
        for w in self._pphase["at_iteration"]:
            w.at_iteration(pm, self._pw)

    def _took_level(self, backend):
        """the library holds a new level: its time is the parent's clock, and the level to come is one parent step later"""
        _, levels, t0, t1 = backend.bforce_info()
        self._have += 1
        self.uploads += 1
        self.times = np.concatenate([self.times[:self._have], [t1 if levels == 2 else t0, (t1 if levels == 2 else t0) + float(self.parent.Δt)]])

    # ---- BoundaryForcing's hooks ----
    def level(self, k):
        raise NotImplementedError("NestForcing: the levels live on the device (backend.bforce_get_levels reads the pair held)")

    def _apply(self, backend, t, force=False):
        """the library holds the pair that brackets t: window_of names it; where its later level has not been taken yet the parent
        steps and is sampled"""
        k = self.window_of(t)
        while k + 1 > self._have:
            self._parent_step(backend)
            self._took_level(backend)
        if k + 1 != self._have:
            raise ValueError(f"NestForcing: a step would start at t = {t!r}, before the pair of parent levels the library holds "
                             f"[{self.times[self._have - 1]!r}, {self.times[self._have]!r}]")
        self._k = k
        return k

    def begin_run(self, model, n_steps: int):
        b = model.backend
        ps, pm = self.parent, self.parent.model
        n_parent = max(1, -(-int(n_steps) // self.ratio))
        self._parent_begin(n_parent)
        if float(pm.clock.time) != float(model.clock.time):
            raise ValueError(f"NestForcing: the child's clock ({model.clock.time!r}) and the parent's ({pm.clock.time!r}) differ")
        if self._set_on is b:
            b.bforce_free()
        self._init_set(b)
        b.nest_init(pm.backend, self.corner_nodes, self.index, self.weights)
        self._set_on = b
        self.times, self._have, self._k = np.zeros(0), -1, None
        self._mark = (self._time(b), int(model.clock.iteration))
        b.nest_sample()                   # level 0: the parent at the common clock
        self._took_level(b)
        self._parent_step(b)              # the parent is one step ahead from here on
        self._took_level(b)

    def load_pickup(self, checkpoint_file):
        raise NotImplementedError("NestForcing: a nested pair cannot be picked up yet")

    def before_step(self, backend):
        raise NotImplementedError("NestForcing: run() left its chunked path (store=True, cash_store=True or winds that vary in time)")

    def at_iteration(self, model, writers):
        """the step actually taken is held against the ratio once it can be read off the clock; the next pair is steps_allowed's
        business (no step of the parent is taken that no step of the child needs)"""
        b = model.backend
        t, it = self._time(b), int(model.clock.iteration)
        if self._mark is not None and it > self._mark[1]:
            check_ratio(self.ratio, (t - self._mark[0]) / (it - self._mark[1]), float(self.parent.Δt))
            self._mark = None

    def finish(self, backend, iteration=None):
        """the parent's writers finish with the child's; the nest and the set go with the run"""
        if getattr(self, "_pw", None) is not None:
            pm = self.parent.model
            for w in self._pphase["finish"]:
                w.finish(pm.backend, pm.clock.iteration)
            self._pw = None
        if self._set_on is backend:
            backend.nest_free()
            backend.bforce_free()
            self._set_on = None
            self._k = None
