"""BoundaryForcing: sea state coming in through an open boundary — swell from a parent model, a storm outside the box, a buoy
spectrum at the mouth of a basin — prescribed at rim nodes as (e, m_x, m_y)(t), without leaving the fused stepping path.

On a model with `periodic_boundary=False` the grid-boundary nodes (mask class 3) carry no particle: what reaches the rim is
dropped and nothing enters (the reference's rim is equally dead).  With a forcing set the library bears a particle at every forced
node behind each step's launch, from the prescribed value at the step's start time, advances it with the model's own solver under
the local wind and scatters it with all others (picles_bforce_*, include/picles_hip.h "open-boundary forcing"; the kernel is
picles_amd/csrc/k_bforce.hip).  A forced node needs no memory between steps: its particle is reborn every step.

Attach like the output writers, `sim.output_writers["boundary_forcing"] = BoundaryForcing(model, side="west", times=..., values=...)`:
`run(sim)` stays on `picles_run_steps`, in chunks that end where the clock would leave the pair of time levels the library holds;
the next pair is uploaded between the chunks (a step that starts at a time level takes the later pair: s = 0, the level itself).
On the per-step loop the pair is checked before every step.

THE VALUE at a step that starts at t, with the levels (t_k, V_k), (t_{k+1}, V_{k+1}) that bracket t, per node and component, each
operation one IEEE operation (NumPy reproduces the bits: `lerp` below):

    s = (t - t_k) / (t_{k+1} - t_k);    v = V_k + s * (V_{k+1} - V_k)

One time level: constant.  THE BIRTH is NodeToParticle!'s branch A (`born_particles` below restates it): e, m_x, m_y finite,
e >= minimal_state[0] and m_x² + m_y² >= minimal_state[1]; otherwise the node bears no particle that step.

BANDS (`width=`, `weights=`).  Sea that travels more than one cell a step crosses a one-node rim between two levels
and never enters.  `width=w` forces every node within w nodes of the side that can bear a particle (`band_nodes`), ocean nodes
included: the library takes those out of the step kernels' hands while the set lives (picles_bforce_init_band).  With weights the
band is a relaxation zone: per node and component v = m + w (p - m), p the prescribed value above, m the model's own State at the
step's start (`blend` reproduces the bits); w = 1 is p itself.  `"linear"`: w = (width - d) / width, d the node distance to the side.

`sea_state(hs, tp, direction, model)` turns a significant wave height, a peak period and a propagation direction into
(e, m_x, m_y): the exact inverse of the definitions of picles_amd/station_output.py.

Not for slabs (`SlabModel`): the edge rows' records are exchanged before a kernel behind the launch could run.
"""
from __future__ import annotations

import math

import numpy as np

from .output_writers import NO_LIMIT, OutputWriter
from .station_output import FOUR_PI

SIDES = ("west", "east", "south", "north", "rim")
WINDOW_EPS = 1e-9          # a time closer to an end of a level window than this fraction of its length is that end (the library's rule)


def sea_state(hs, tp, direction, model):
    """(e, m_x, m_y) of waves of significant height `hs` [m], peak period `tp` [s], travelling towards `direction` [rad, atan2(m_y, m_x)]:
    e = (hs / 4)², c̄ = r_g g tp / FOUR_PI, |m| = e / (2 c̄) — StationWriter's hs, tp and dir of that state are the arguments again"""
    P = model.ODEsettings.Parameters
    g, r_g = P.get("g", 9.81), P["r_g"]
    hs, tp, direction = np.asarray(hs, dtype=np.float64), np.asarray(tp, dtype=np.float64), np.asarray(direction, dtype=np.float64)
    e = (hs / 4.0) * (hs / 4.0)
    cbar = ((r_g * g) * tp) / FOUR_PI
    m = e / (2.0 * cbar)
    return e, m * np.cos(direction), m * np.sin(direction)


def lerp(t, t0, v0, t1, v1):
    """the library's value at a step that starts at t, bit for bit"""
    s = (np.float64(t) - np.float64(t0)) / (np.float64(t1) - np.float64(t0))
    v0, v1 = np.asarray(v0, dtype=np.float64), np.asarray(v1, dtype=np.float64)
    return v0 + s * (v1 - v0)


def born_particles(values, minimal_state):
    """NodeToParticle!'s branch A and GetVariablesAtVertex on (n, 3) values: (born [n] bool, z [n, 3] = lne, c̄_x, c̄_y; NaN rows
    where no particle is born).  The kernel forms |m|² with one fused multiply-add and its own log: equal to rounding, not to the bit"""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 3)
    e, mx, my = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        m2 = mx * mx + my * my
        born = np.isfinite(e) & np.isfinite(mx) & np.isfinite(my) & (e >= minimal_state[0]) & (m2 >= minimal_state[1])
        q = e / (2.0 * m2)
        z = np.stack([np.log(e), mx * q, my * q], axis=1)
    z[~born] = np.nan
    return born, z


def side_distance(grid, side):
    """(Nx, Ny) int array: the distance in nodes of every node to the forced side (to the nearest of the four for "rim"), 0 on it"""
    Nx, Ny = int(grid.stats.Nx), int(grid.stats.Ny)
    i, j = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
    if side not in SIDES:
        raise ValueError(f"BoundaryForcing: side must be one of {SIDES}, not {side!r}")
    d = {"west": i, "east": Nx - 1 - i, "south": j, "north": Ny - 1 - j}
    return np.minimum(np.minimum(d["west"], d["east"]), np.minimum(d["south"], d["north"])) if side == "rim" else d[side]


def band_nodes(grid, side, width):
    """the nodes within `width` nodes of a side (or of the whole rim) that can bear a particle — mask class 3 (grid boundary) or 1
    (ocean); land and coast (0, 2) are skipped — row by row, i running fastest, and their distance d to the forced side"""
    if not (isinstance(width, (int, np.integer)) and width >= 1):
        raise ValueError(f"BoundaryForcing: width must be an integer >= 1, not {width!r}")
    d = side_distance(grid, side)
    mask = np.asarray(grid.data.mask)
    keep = (d < int(width)) & ((mask == 1) | (mask == 3))
    j, i = np.nonzero(keep.T)                     # rows in order, i fastest within a row
    return [(int(a), int(b)) for a, b in zip(i, j)], d[i, j]


def linear_weights(d, width):
    """the "linear" ramp of a relaxation zone: w = (width - d) / width — 1 on the forced side, 1 / width on the band's last node"""
    return (np.float64(width) - np.asarray(d, dtype=np.float64)) / np.float64(width)


def blend(m, p, w):
    """the library's blend of a prescribed value p into the model's own State m at weight w, bit for bit: v = m + w (p - m)"""
    m, p, w = (np.asarray(a, dtype=np.float64) for a in (m, p, w))
    return m + w * (p - m)


def rim_nodes(grid, side, width=1):
    """the 0-based (i, j) nodes of one side of the mesh (corners included) or of the whole rim, i running fastest; width > 1: the
    band of every node within `width` nodes of it that can bear a particle (band_nodes), in the same order"""
    if width != 1:
        return band_nodes(grid, side, width)[0]
    Nx, Ny = int(grid.stats.Nx), int(grid.stats.Ny)
    if side == "west":
        return [(0, j) for j in range(Ny)]
    if side == "east":
        return [(Nx - 1, j) for j in range(Ny)]
    if side == "south":
        return [(i, 0) for i in range(Nx)]
    if side == "north":
        return [(i, Ny - 1) for i in range(Nx)]
    if side == "rim":
        return [(i, j) for j in range(Ny) for i in range(Nx) if i in (0, Nx - 1) or j in (0, Ny - 1)]
    raise ValueError(f"BoundaryForcing: side must be one of {SIDES}, not {side!r}")


def node_points(grid, nodes):
    """the mesh coordinates (x, y) of 0-based (i, j) nodes, as a list of float pairs"""
    x, y = np.asarray(grid.data.x), np.asarray(grid.data.y)
    return [(float(x[i, j]), float(y[i, j])) for i, j in np.asarray(nodes, dtype=np.int64).reshape(-1, 2)]


def from_station_output(model, path, name="stations", *, nodes=None, side=None, Δt=None, width=1, weights=None):
    """the offline route of a nest: a BoundaryForcing for `model` from the file a StationWriter wrote in a parent run at the
    model's forced nodes (`points=nesting.rim_points(model, side=... | nodes=...)`): `times` are /stations/time, `values` the
    e, m_x, m_y of every record — NaN rows included: a station without a wet corner bears no particle.  The file's stations must
    be the forced nodes in order"""
    from .station_output import VAR_NAMES, read_station_output
    if (nodes is None) == (side is None):
        raise ValueError("from_station_output needs either nodes=[(i, j), ...] or side=...")
    forced = np.asarray(rim_nodes(model.grid, side, width) if nodes is None else nodes, dtype=np.int64).reshape(-1, 2)
    out = read_station_output(path, name)
    data = np.asarray(out["data"], dtype=np.float64)
    pts = np.asarray(node_points(model.grid, forced))
    fx, fy = np.asarray(out["x"], dtype=np.float64), np.asarray(out["y"], dtype=np.float64)
    if data.shape[1] != len(forced) or not (np.array_equal(fx, pts[:, 0]) and np.array_equal(fy, pts[:, 1])):
        raise ValueError(f"from_station_output: the {data.shape[1]} stations of {name!r} are not the model's {len(forced)} forced nodes in order "
                         "(write the file with StationWriter(points=nesting.rim_points(model, ...)))")
    times = np.asarray(out["time"], dtype=np.float64)
    keep = np.isfinite(times)                     # records a shorter run never wrote
    names = [str(v) for v in out.get("var_names", VAR_NAMES)]
    cols = [names.index(v) for v in ("e", "m_x", "m_y")]
    if isinstance(weights, str):                   # a ramp needs the side the distances are counted from
        return BoundaryForcing(model, side=side, width=width, weights=weights, times=times[keep], values=data[keep][:, :, cols], Δt=Δt)
    return BoundaryForcing(model, nodes=forced, weights=weights, times=times[keep], values=data[keep][:, :, cols], Δt=Δt)


class BoundaryForcing(OutputWriter):
    """BoundaryForcing(model, nodes=[(i, j), ...] | side="west" | "east" | "south" | "north" | "rim", times=[...],
    values=array(time, node, 3) | callable(t) -> (n, 3), Δt=None, width=1, weights=None | "linear" | array(n))

    width > 1 (with side=), or an ocean node among nodes=: a BAND set (picles_bforce_init_band) — the forced ocean nodes are not
    stepped while the set lives.  Choose the width as deep as the fastest swell travels in a step (cells per step, rounded up): sea
    that crosses a one-node rim between two levels never enters.  weights: the prescribed value p is blended into the model's own
    State m at the step's start, v = m + w (p - m) (`blend`); "linear": w = (width - d) / width, d the node distance to the
    forced side — a relaxation zone."""

    kind = "boundary_forcing"
    needs = "bforce_init"
    refusal = "a BoundaryForcing needs a backend with bforce_init / bforce_set_levels (the HIP library)"

    def __init__(self, model, *, nodes=None, side=None, times, values, Δt=None, width=1, weights=None):
        if type(model).__name__ == "SlabModel":
            raise NotImplementedError("BoundaryForcing: slabs do not carry a boundary forcing (the edge rows' records are exchanged "
                                      "before the forced nodes' could be added): use a whole-grid model")
        if (nodes is None) == (side is None):
            raise ValueError("BoundaryForcing needs either nodes=[(i, j), ...] or side=...")
        self.model = model
        self._take_nodes(model, nodes, side, width, weights)
        n = len(self.nodes)
        self.times = np.asarray(times, dtype=np.float64).reshape(-1)
        if self.times.size < 1 or not np.isfinite(self.times).all() or (np.diff(self.times) <= 0.0).any():
            raise ValueError("BoundaryForcing: times must be finite and strictly increasing")
        if callable(values):
            self.values = values
        else:
            self.values = np.asarray(values, dtype=np.float64)
            if self.values.shape != (self.times.size, n, 3):
                raise ValueError(f"BoundaryForcing: values must have the shape (time, node, 3) = {(self.times.size, n, 3)}, "
                                 f"not {self.values.shape}")
        self.dt = None if Δt is None else float(Δt)
        self.uploads = 0              # level pairs handed to the library
        self._set_on = None           # the backend that holds this forcing's set
        self._k = None                # the window [times[k], times[k + 1]] it holds
        self._mark = None             # (time, iteration) of the last visit: Δt is read off two of them when it was not given

    # ---- the set ----
    def _take_nodes(self, model, nodes, side, width, weights):
        """self.nodes, self.node_weights (None: every node 1.0) and self.band: does the set go through bforce_init_band?"""
        who = type(self).__name__
        if nodes is not None and width != 1:
            raise ValueError(f"{who}: width= goes with side=; with nodes= the list is the band")
        dist = None
        if nodes is None and width != 1:
            listed, dist = band_nodes(model.grid, side, width)
        else:
            listed = rim_nodes(model.grid, side) if nodes is None else nodes
        self.nodes = np.asarray(listed, dtype=np.int64).reshape(-1, 2)
        n = len(self.nodes)
        if n < 1:
            raise ValueError(f"{who}: no node given")
        if len(np.unique(self.nodes, axis=0)) != n:
            raise ValueError(f"{who}: a node is given twice")
        self.width = int(width)
        if weights is None:
            self.node_weights = None
        elif isinstance(weights, str):
            if weights != "linear" or nodes is not None:
                raise ValueError(f"{who}: weights must be None, \"linear\" (with side=) or an array of one weight per node, not {weights!r}")
            self.node_weights = linear_weights(np.zeros(n, dtype=np.int64) if dist is None else dist, self.width)
        else:
            self.node_weights = np.asarray(weights, dtype=np.float64).reshape(-1)
            if self.node_weights.shape != (n,):
                raise ValueError(f"{who}: {self.node_weights.size} weights for {n} nodes")
        if self.node_weights is not None and not (np.isfinite(self.node_weights).all() and (self.node_weights > 0.0).all() and (self.node_weights <= 1.0).all()):
            raise ValueError(f"{who}: weights must be finite and in (0, 1]")
        mask = np.asarray(model.grid.data.mask)
        inside = (self.nodes >= 0).all(axis=1) & (self.nodes[:, 0] < mask.shape[0]) & (self.nodes[:, 1] < mask.shape[1])
        ocean = np.zeros(n, dtype=bool)
        ocean[inside] = mask[self.nodes[inside, 0], self.nodes[inside, 1]] == 1
        self.band = bool(self.width != 1 or ocean.any() or self.node_weights is not None)

    BAND_REFUSAL = ("a forcing band (width > 1, an ocean node among the forced nodes, or weights) needs a backend with "
                    "bforce_init_band (the HIP library, ABI 12)")

    def check_run(self, sim, writers, store=False, cash_store=False, pickup=False):
        if self.band and not hasattr(sim.model.backend, "bforce_init_band"):
            raise NotImplementedError(self.BAND_REFUSAL)

    def _init_set(self, backend):
        """width = 1 on rim nodes without weights: bforce_init as ever; anything else is a band set"""
        if self.band:
            backend.bforce_init_band(self.nodes, self.node_weights)
        else:
            backend.bforce_init(self.nodes)

    # ---- the levels ----
    def level(self, k):
        v = self.values(float(self.times[k])) if callable(self.values) else self.values[k]
        v = np.asarray(v, dtype=np.float64)
        if v.shape != (len(self.nodes), 3):
            raise ValueError(f"BoundaryForcing: values(t) must return an ({len(self.nodes)}, 3) array, not {v.shape}")
        return v

    def _snaps(self, k, t):
        """does a step that starts at t, at or below times[k + 1], belong to the window behind that level?  Within that window's own
        slack of the level — the library's rule for the pair it holds, so the pair chosen here is one it accepts at t"""
        T = self.times
        return k + 2 < T.size and t >= T[k + 1] - WINDOW_EPS * (T[k + 2] - T[k + 1])

    def window_of(self, t):
        """k of the window [times[k], times[k + 1]] a step that starts at t takes its value from: the later one at a time level"""
        T = self.times
        if T.size == 1:
            return 0
        if not (T[0] - WINDOW_EPS * (T[1] - T[0]) <= t <= T[-1] + WINDOW_EPS * (T[-1] - T[-2])):
            raise ValueError(f"BoundaryForcing: a step would start at t = {t!r}, outside the forcing's times [{T[0]!r}, {T[-1]!r}]: "
                             "give levels that cover the run")
        k = min(max(int(np.searchsorted(T, t, side="right")) - 1, 0), T.size - 2)
        return k + 1 if self._snaps(k, t) else k

    def _time(self, backend):
        t = getattr(backend, "clock", None)
        return float(self.model.clock.time if t is None else t)

    def _apply(self, backend, t, force=False):
        """the library holds the pair that brackets t"""
        k = self.window_of(t)
        if not force and self._k == k and self._set_on is backend:
            return k
        if self.times.size == 1:
            backend.bforce_set_levels(float(self.times[0]), self.level(0))
        else:
            backend.bforce_set_levels(float(self.times[k]), self.level(k), float(self.times[k + 1]), self.level(k + 1))
        self.uploads += 1
        self._k = k
        return k

    # ---- the hooks of run() ----
    def begin_run(self, model, n_steps: int):
        b = model.backend
        if self._set_on is b:
            b.bforce_free()
        self._init_set(b)
        self._set_on = b
        self._k = None
        self._mark = (self._time(b), int(model.clock.iteration))
        self._apply(b, self._mark[0], force=True)

    def load_pickup(self, checkpoint_file):
        """the checkpoint holds nothing of the forcing (a forced particle carries nothing across a step): the pair that brackets
        the restored clock is uploaded again — here where the set exists already, in begin_run otherwise"""
        self._k = None
        b = getattr(self.model, "backend", None)
        if b is not None and self._set_on is b:
            self._apply(b, self._time(b), force=True)

    def steps_allowed(self, backend, iteration: int) -> int:
        """the steps of the next chunk whose start times lie inside the pair's window (the library checks the same, with the same
        arithmetic, before it enqueues anything); one step while Δt is not known yet"""
        if self.times.size == 1:
            return NO_LIMIT
        t = self._time(backend)
        k = self._apply(backend, t)
        if self.dt is None:
            return 1
        t0, t1 = float(self.times[k]), float(self.times[k + 1])
        # a step that starts at the window's end belongs to the next window where there is one (s = 0 there: the level itself)
        slack = WINDOW_EPS * (t1 - t0)
        n, tt = 0, t
        most = int(math.floor((t1 + slack - t) / self.dt)) + 2
        while n < most and tt <= t1 + slack and not self._snaps(k, tt):
            n += 1
            tt += self.dt
        return max(n, 1)

    def before_step(self, backend):
        self._apply(backend, self._time(backend))

    def at_iteration(self, model, writers):
        """first among the writers: the pair for the next chunk is in place before anything else looks at the iteration.  A clock
        beyond the last level is left to the next step, if there is one (steps_allowed / before_step name the remedy)"""
        b = model.backend
        t, it = self._time(b), int(model.clock.iteration)
        if self.dt is None and self._mark is not None and it > self._mark[1]:
            self.dt = (t - self._mark[0]) / (it - self._mark[1])
        if self.times.size > 1 and t <= self.times[-1] + WINDOW_EPS * (self.times[-1] - self.times[-2]):
            self._apply(b, t)

    def finish(self, backend, iteration=None):
        """the set goes with the run, as a StatisticsWriter's does: a later run on the same model without this forcing is not forced
        by its last levels.  (The library completes the last step first; the forced nodes' particles are switched off.)"""
        if self._set_on is backend:
            backend.bforce_free()
            self._set_on = None
            self._k = None
