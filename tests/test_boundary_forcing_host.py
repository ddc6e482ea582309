"""BoundaryForcing on the CPU box: window selection and the chunking of run() across time levels over a backend that records its
calls (the pattern of tests/test_station_output_host.py), sea_state against the station formulas, the refusals, the pickup
re-upload, and the NumPy restatement of the birth test against hand values."""
import math

import numpy as np
import pytest

from picles_amd import configs, models
from picles_amd.boundary_forcing import BoundaryForcing, born_particles, lerp, rim_nodes, sea_state
from picles_amd.output_writers import NO_LIMIT, PHASE_ORDER
from picles_amd.parallel import SlabModel
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import station_records
from test_field_output_host import FakeBackend

G, RG = 9.81, 0.85


class ForcingBackend(FakeBackend):
    """FakeBackend + the forcing set: it refuses what the library refuses — a step that starts outside the level pair's window"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.bf = None
        self.seeded_before_init = None

    def seed(self, t0=0.0):
        super().seed(t0)
        if self.bf is None:
            self.seeded_before_init = True

    def bforce_init(self, nodes):
        assert self.bf is None, "second bforce_init without bforce_free"
        self.bf = dict(nodes=np.asarray(nodes), levels=None)
        self.log.append(("bforce_init", len(nodes)))

    def bforce_free(self):
        self.bf = None
        self.log.append(("bforce_free",))

    def bforce_set_levels(self, t0, v0, t1=None, v1=None):
        assert self.bf is not None and np.asarray(v0).shape == (len(self.bf["nodes"]), 3)
        self.bf["levels"] = (t0, np.array(v0), t1, None if v1 is None else np.array(v1))
        self.log.append(("bforce_set_levels", t0, t1))

    def _inside(self, dt, n):
        if self.bf is None:
            return
        t0, _, t1, v1 = self.bf["levels"]
        if v1 is None:
            return
        slack, t = 1e-9 * (t1 - t0), self.clock
        for _ in range(n):
            assert t0 - slack <= t <= t1 + slack, f"a step starts at {t}, outside [{t0}, {t1}]"
            t += dt

    def run_steps(self, dt, n):
        self._inside(dt, n)
        t = self.clock
        for _ in range(n):          # the library's clock: one addition per step
            t += dt
        self.log.append(("run_steps", n))
        self.clock = t

    def time_step(self, dt, flags=0):
        self._inside(dt, 1)
        super().time_step(dt, flags)

    def get_state(self):
        return np.zeros((self.Nx, self.Ny, 3))


def _sim(n_steps, n=12, backend=ForcingBackend):
    cfg = configs.bench06_box(n=n, periodic_grid=False)
    m = models.WaveGrowth2D(**cfg.model, backend_factory=backend)
    return m, Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1)), cfg.Δt


def _values(times, n):
    v = np.empty((len(times), n, 3))
    v[..., 0] = 1.0 + np.arange(len(times))[:, None]
    v[..., 1] = 0.1
    v[..., 2] = 0.0
    return v


def test_sides_and_rim_nodes():
    m, _, _ = _sim(3, n=5)
    assert rim_nodes(m.grid, "west") == [(0, j) for j in range(5)]
    assert rim_nodes(m.grid, "north") == [(i, 4) for i in range(5)]
    rim = rim_nodes(m.grid, "rim")
    assert len(rim) == 16 and len(set(rim)) == 16 and rim[:6] == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (0, 1)]
    with pytest.raises(ValueError, match="side must be"):
        rim_nodes(m.grid, "up")


def test_window_selection_at_and_between_levels():
    m, _, _ = _sim(3)
    times = [0.0, 1800.0, 3600.0, 9000.0]
    f = BoundaryForcing(m, side="west", times=times, values=_values(times, 12))
    assert [f.window_of(t) for t in (0.0, 1.0, 1799.0, 1800.0, 1800.0 - 1e-9, 3599.0, 3600.0, 8999.0, 9000.0)] == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    for t in (-1.0, 9000.1):
        with pytest.raises(ValueError, match="outside the forcing's times"):
            f.window_of(t)
    one = BoundaryForcing(m, side="west", times=[0.0], values=_values([0.0], 12))
    assert one.window_of(1e9) == 0 and one.steps_allowed(m.backend, 0) == NO_LIMIT


def test_run_chunks_end_where_the_clock_leaves_the_window():
    """600-second steps against levels every 1800 s: a chunk ends before the step that starts at the next level, and the next pair
    is uploaded before the next chunk; the fake backend refuses, as the library does, a start time outside the pair it holds"""
    m, sim, dt = _sim(10)
    times = np.arange(0.0, 7201.0, 1800.0)
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="rim", times=times, values=_values(times, 44), Δt=dt)
    run(sim)
    log = [e for e in m.backend.log if e[0] in ("bforce_init", "bforce_set_levels", "run_steps", "seed")]
    assert log[0][0] == "seed" and log[1] == ("bforce_init", 44)
    assert [e for e in log if e[0] == "run_steps"] == [("run_steps", 3), ("run_steps", 3), ("run_steps", 3), ("run_steps", 1)]
    assert [e[1:] for e in log if e[0] == "bforce_set_levels"] == [(0.0, 1800.0), (1800.0, 3600.0), (3600.0, 5400.0), (5400.0, 7200.0)]
    # every pair is in place before the chunk that needs it
    k = [i for i, e in enumerate(log) if e[0] == "bforce_set_levels"]
    r = [i for i, e in enumerate(log) if e[0] == "run_steps"]
    assert all(a < b for a, b in zip(k, r)) and f.uploads == 4
    assert m.clock.iteration == 10


def test_step_length_is_read_off_the_run_when_not_given():
    m, sim, dt = _sim(7)
    times = [0.0, 1800.0, 3600.0]
    sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", times=times, values=_values(times, 12))
    run(sim)
    assert [e[1] for e in m.backend.log if e[0] == "run_steps"] == [1, 2, 4]        # one step until Δt is known; the last window takes the step at its end


def test_callable_values_and_the_per_step_loop():
    m, sim, dt = _sim(5)
    seen = []

    def values(t):
        seen.append(t)
        return np.tile([1.0 + t, 0.1, 0.0], (12, 1))
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="east", times=[0.0, 1200.0, 2400.0], values=values)
    run(sim, cash_store=True)              # the per-step loop: before_step keeps the pair in place
    assert [e[1] for e in m.backend.log if e[0] in ("time_step",)] == [1] * 5
    assert [e[1:] for e in m.backend.log if e[0] == "bforce_set_levels"] == [(0.0, 1200.0), (1200.0, 2400.0)]
    assert seen == [0.0, 1200.0, 1200.0, 2400.0] and f.uploads == 2


def test_a_run_past_the_last_level_is_refused_with_the_remedy():
    m, sim, dt = _sim(8)
    sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", times=[0.0, 1800.0], values=_values([0.0, 1800.0], 12), Δt=dt)
    with pytest.raises(ValueError, match="give levels that cover the run"):
        run(sim)
    assert sum(e[1] for e in m.backend.log if e[0] == "run_steps") == 4          # the steps that start at 0 ... 1800 were taken


def test_refusals_come_before_anything_is_seeded():
    m, sim, dt = _sim(3, backend=FakeBackend)               # a backend without bforce_init
    sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", times=[0.0], values=_values([0.0], 12))
    with pytest.raises(NotImplementedError, match="bforce_init"):
        run(sim)
    assert m.backend.log == []
    m2, _, _ = _sim(3)
    for kw, what in ((dict(side="west", nodes=[(0, 0)]), "either"), (dict(), "either"), (dict(nodes=[(0, 1), (0, 1)]), "twice"),
                     (dict(side="west", times=[0.0, 0.0]), "strictly increasing"), (dict(side="west", times=[0.0, np.inf]), "finite"),
                     (dict(side="west", values=np.zeros((1, 3, 3))), "shape")):
        a = dict(times=[0.0], values=_values([0.0], 12))
        a.update(kw)
        if "nodes" in kw and "values" not in kw:
            a["values"] = _values(a["times"], len(kw["nodes"]))
        if "times" in kw and "values" not in kw:
            a["values"] = _values(a["times"], 12)
        with pytest.raises(ValueError, match=what):
            BoundaryForcing(m2, **a)
    slab = object.__new__(SlabModel)
    with pytest.raises(NotImplementedError, match="slabs"):
        BoundaryForcing(slab, side="west", times=[0.0], values=np.zeros((1, 1, 3)))


def test_pickup_uploads_the_pair_that_brackets_the_restored_clock():
    m, sim, dt = _sim(4)
    times = np.arange(0.0, 7201.0, 1800.0)
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", times=times, values=_values(times, 12), Δt=dt)
    f.begin_run(m, 4)                      # a set that exists (run() frees it when it ends: a set made by hand, as a pickup into a
    b = m.backend                          # model that holds one finds it)
    n0 = f.uploads
    b.clock = 4200.0                       # what a checkpoint load restores
    f.load_pickup("ignored")
    assert f.uploads == n0 + 1 and b.bf["levels"][0] == 3600.0 and b.bf["levels"][2] == 5400.0
    assert b.log[-1] == ("bforce_set_levels", 3600.0, 5400.0)
    # a fresh model: nothing to upload to yet — begin_run creates the set and uploads
    m2, sim2, _ = _sim(4)
    f2 = BoundaryForcing(m2, side="west", times=times, values=_values(times, 12), Δt=dt)
    f2.load_pickup("ignored")
    assert f2.uploads == 0 and m2.backend.log == []
    m2.backend.clock = 4200.0
    f2.begin_run(m2, 3)
    assert [e for e in m2.backend.log if e[0].startswith("bforce")] == [("bforce_init", 12), ("bforce_set_levels", 3600.0, 5400.0)]


def test_forcing_is_visited_first():
    assert PHASE_ORDER["begin_run"][0] == "boundary_forcing" and PHASE_ORDER["at_iteration"][0] == "boundary_forcing"


def test_sea_state_is_inverted_by_the_station_formulas():
    m, _, _ = _sim(3)
    rng = np.random.default_rng(5)
    hs, tp, dr = rng.uniform(0.2, 9.0, 50), rng.uniform(3.0, 20.0, 50), rng.uniform(-math.pi, math.pi, 50)
    e, mx, my = sea_state(hs, tp, dr, m)
    v = np.stack([e, mx, my])[None]                                   # one sample, 3 planes, 50 nodes
    r = station_records(v, np.arange(50)[:, None], np.ones((50, 1)), G, RG)[0]
    # hs = 4 sqrt(e) of e = (hs / 4)²: one rounding each way; tp and dir: a handful of operations
    assert np.allclose(r[:, 3], hs, rtol=4e-16, atol=0) and np.allclose(r[:, 4], tp, rtol=1e-14, atol=0)
    assert np.allclose(r[:, 7], dr, rtol=0, atol=1e-14)
    # hand values: hs = 4 m -> e = 1; tp such that c̄ = 10 m/s -> |m| = 0.05, towards +x
    e1, mx1, my1 = sea_state(4.0, 10.0 * 12.566370614359172 / (RG * G), 0.0, m)
    assert e1 == 1.0 and my1 == 0.0 and mx1 == pytest.approx(0.05, rel=1e-15)


def test_birth_restatement_hand_values():
    min_e, min_m2 = 1e-3, 1e-8
    v = np.array([[1.0, 0.03, 0.04],            # born: |m|² = 0.0025, q = 200, c̄ = (6, 8)
                  [4.0, 0.0, -0.5],             # born: q = 8, c̄ = (0, -4)
                  [np.nan, 0.1, 0.1], [1.0, np.inf, 0.1], [1.0, 0.1, -np.inf],
                  [0.0, 0.1, 0.1], [-1.0, 0.1, 0.1], [1.0, 0.0, 0.0], [9e-4, 0.1, 0.1], [1.0, 9e-5, 0.0]])
    born, z = born_particles(v, (min_e, min_m2))
    assert born.tolist() == [True, True] + [False] * 8
    assert z[0].tolist() == [0.0, pytest.approx(6.0, rel=1e-15), pytest.approx(8.0, rel=1e-15)]
    assert z[1].tolist() == [math.log(4.0), 0.0, -4.0]
    assert np.isnan(z[2:]).all()
    # the thresholds themselves are accepted (>=)
    assert born_particles([[min_e, 1e-4, 0.0]], (min_e, min_m2))[0].tolist() == [True]


def test_lerp_is_three_operations():
    v0, v1 = np.array([[1.0, 0.1, 0.3]]), np.array([[2.5, -0.2, 0.7]])
    s = (700.0 - 600.0) / (1800.0 - 600.0)
    assert np.array_equal(lerp(700.0, 600.0, v0, 1800.0, v1), v0 + s * (v1 - v0))
    assert np.array_equal(lerp(600.0, 600.0, v0, 1800.0, v1), v0)


def test_window_slack_is_that_of_the_window_behind_the_level():
    """strongly uneven levels: a clock just below a level snaps to it only within the slack of the window BEHIND it, the one the
    library will hold (1e-9 of that window's length); any farther and the step belongs to the window in front, which accepts it"""
    m, _, _ = _sim(3)
    times = [0.0, 1e6, 1e6 + 1.0, 2e6]
    f = BoundaryForcing(m, side="west", times=times, values=_values(times, 12), Δt=1.0)
    for t, k in ((1e6 - 1e-4, 0), (1e6 - 5e-10, 1), (1e6, 1), (1e6 + 1.0 - 1e-2, 1), (1e6 + 1.0 - 1e-4, 2), (1e6 + 1.0, 2)):
        got = f.window_of(t)
        assert got == k, (t, got, k)
        t0, t1 = times[got], times[got + 1]          # the library's test of the pair it is then given
        assert t0 - 1e-9 * (t1 - t0) <= t <= t1 + 1e-9 * (t1 - t0), (t, got)
    # steps_allowed ends the chunk by the same rule: from 1e6 - 2.0001 with 1-second steps, the steps that start at
    # 1e6 - 2.0001 and 1e6 - 1.0001 and the one 1e-4 s short of the level stay with window 0
    m.backend.bforce_init(f.nodes)
    f._set_on = m.backend
    m.backend.clock = 1e6 - 2.0001
    assert f.steps_allowed(m.backend, 0) == 3


def test_finish_frees_the_set():
    m, sim, dt = _sim(4)
    times = [0.0, 7200.0]
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", times=times, values=_values(times, 12), Δt=dt)
    run(sim)
    assert ("bforce_free",) in m.backend.log
    assert m.backend.bf is None and f._set_on is None
    assert "boundary_forcing" not in PHASE_ORDER["finish"]          # visited behind the writers the phase lists: the last output sees the set
    # a second run on the same model makes its set again
    sim.stop_time = dt * 7
    run(sim)
    assert [e[0] for e in m.backend.log].count("bforce_init") == 2 and m.backend.bf is None
