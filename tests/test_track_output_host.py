"""TrackWriter on the CPU box: the vectorised locate against station_output.locate_points bit for bit, the sort and the caller's
order, the interpolation and record arithmetic on hand-made tables and against the scalar restatement (tests/_track_numpy.py), the
writer + run() over a backend that records its calls (the pattern of tests/test_station_output_host.py), the file layout in both
formats."""
import math

import numpy as np
import pytest

import _track_numpy as TN
from picles_amd import configs, models
from picles_amd.checkpointing import Checkpointer
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.output_writers import NO_LIMIT, PHASE_ORDER
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import VAR_NAMES, locate_points
from picles_amd.track_output import TrackWriter, locate_points_fast, read_track_output, track_records
from test_field_output_host import FakeBackend

G, RG = 9.81, 0.85


def _grid(per, nx=23, ny=17):
    return TwoDCartesianGridMesh(-300.0, -300.0 + 700.0 * (nx - 1), nx, 100.0, 100.0 + 450.0 * (ny - 1), ny, periodic_boundary=per)


@pytest.mark.parametrize("per", [(False, False), (True, True), (True, "tripolar_north")], ids=["open", "periodic", "tripolar"])
def test_vectorised_locate_equals_locate_points_bitwise(per):
    g = _grid(per)
    nx, ny = 23, 17
    xs, ys = g.data.x[:, 0], g.data.y[0, :]
    rng = np.random.default_rng(17)
    x = xs[0] + rng.uniform(0.0, 1.0, 2000) * 700.0 * (nx if per[0] else nx - 1)
    y = ys[0] + rng.uniform(0.0, 1.0, 2000) * 450.0 * (ny if per[1] is True else ny - 3 if per[1] else ny - 1)
    # nodes, edges, the first and the last node of every axis, the last representable point of a periodic one
    x[:nx], y[:nx] = xs, ys[3]
    y[nx:nx + ny - 3], x[nx:nx + ny - 3] = ys[:ny - 3], xs[5]
    x[100], y[101] = xs[-1], (ys[-1] if per[1] is False else ys[0])
    if per[0]:
        x[102] = np.nextafter(xs[0] + 700.0 * nx, -np.inf)
    pts = np.stack([x, y], axis=1)
    c0, w0 = locate_points(g, [tuple(p) for p in pts])
    c1, w1 = locate_points_fast(g, pts)
    assert c1.dtype == np.int64 and w1.dtype == np.float64
    assert np.array_equal(c0, c1)
    assert np.array_equal(w0.view(np.uint64), w1.view(np.uint64))
    assert (w0.max(axis=1) == 1.0).sum() >= nx and c0[:, :, 0].max() == nx - 1 and c0[:, :, 0].min() == 0
    for bad in ([(xs[0] - 1.0, ys[2])], [(xs[2], ys[0] - 0.5)], [(xs[0] + 700.0 * (nx if per[0] else nx - 1) + (0.0 if per[0] else 0.5), ys[2])],
                [(xs[2], ys[-1] + (450.0 if per[1] is True else 0.5))]):
        with pytest.raises(ValueError):
            locate_points(g, bad)
        with pytest.raises(ValueError, match="outside"):
            locate_points_fast(g, bad)
    if per[1] == "tripolar_north":
        with pytest.raises(ValueError):
            locate_points_fast(g, [(xs[2], ys[ny - 2])])


def test_interpolation_and_records_hand_values():
    #            e_b  mx_b  my_b   t_b   e_a  mx_a  my_a   t_a
    rows = [(4.0, 3.0, 4.0, 100.0, 8.0, 1.0, 2.0, 300.0),      # a quarter of the way
            (4.0, 3.0, 4.0, 200.0, 9.0, 9.0, 9.0, 200.0),      # on a clock: t_a == t_b, V = V_b
            (np.nan, np.nan, np.nan, np.nan, 8.0, 1.0, 2.0, 300.0),      # no before slot
            (4.0, 3.0, 4.0, 100.0, np.nan, np.nan, np.nan, np.nan),      # no after slot
            (np.nan, np.nan, np.nan, 100.0, 8.0, 1.0, 2.0, 300.0),       # the before sample was not valid
            (4.0, 3.0, 4.0, 100.0, np.nan, np.nan, np.nan, 300.0),       # the after sample was not valid
            (1.0, 1.0, -2.0, 100.0, 1.0, -1.0, 2.0, 300.0)]              # means that cancel half-way: M2 == 0
    tab = np.array(rows).T
    t = np.array([150.0, 200.0, 250.0, 150.0, 150.0, 150.0, 200.0])
    r = track_records(tab, t, G, RG)
    s = (150.0 - 100.0) / (300.0 - 100.0)
    E, MX, MY = 4.0 + s * (8.0 - 4.0), 3.0 + s * (1.0 - 3.0), 4.0 + s * (2.0 - 4.0)
    M2 = MX * MX + MY * MY
    assert r[0, :3].tolist() == [E, MX, MY] == [5.0, 2.5, 3.5]
    assert r[0, 3] == 4.0 * math.sqrt(E)
    assert r[0, 4] == (12.566370614359172 * max((E / (2.0 * math.sqrt(M2))) / RG, 0.1)) / G
    assert r[0, 5] == (MX * E) / (2.0 * M2) and r[0, 6] == (MY * E) / (2.0 * M2) and r[0, 7] == math.atan2(MY, MX)
    assert r[1, :3].tolist() == [4.0, 3.0, 4.0] and r[1, 3] == 8.0
    assert np.isnan(r[2:]).all() and np.isfinite(r[:2]).all()
    # and the scalar restatement, bit for bit, on random tables with empty and invalid slots
    rng = np.random.default_rng(23)
    n = 400
    tab = rng.normal(size=(8, n)) * np.array([1.0, 0.3, 0.3, 0.0, 1.0, 0.3, 0.3, 0.0])[:, None]
    tab[0], tab[4] = np.abs(tab[0]) + 0.01, np.abs(tab[4]) + 0.01
    tab[3] = 600.0 * rng.integers(0, 5, n)
    tab[7] = tab[3] + 600.0 * rng.integers(0, 2, n)
    t = tab[3] + rng.uniform(0.0, 1.0, n) * (tab[7] - tab[3])
    tab[:4, rng.integers(n, size=30)] = np.nan
    tab[4:, rng.integers(n, size=30)] = np.nan
    tab[0:3, rng.integers(n, size=20)] = np.nan
    got, want = track_records(tab, t, G, RG), TN.records(tab, t, G, RG)
    assert np.array_equal(got.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any(axis=1).sum() >= 50 and np.isfinite(want).all(axis=1).sum() >= 250


# ---- TrackWriter + run() over a backend that records its calls ----
class TrackBackend(FakeBackend):
    """FakeBackend + the track table: a sample's means are (1 + T / 1000, 0.5, 0.25) at every event, the rule is the header's"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.trk = None
        self.open = None

    def track_init(self, times, corners_ij, weights, horizon):
        assert self.trk is None, "second track_init without track_free"
        t = np.asarray(times, dtype=np.float64)
        assert (np.diff(t) >= 0).all() and np.asarray(corners_ij).shape == (8, len(t)) and np.asarray(weights).shape == (4, len(t))
        self.trk = dict(t=t, H=horizon, tab=np.full((8, len(t)), np.nan), samples=0)
        self.log.append(("track_init", len(t), horizon))

    def _sample(self):
        k, T = self.trk, self.clock
        near = (k["t"] > T - k["H"]) & (k["t"] < T + k["H"])
        v = np.array([1.0 + T / 1000.0, 0.5, 0.25, T])
        before = near & (k["t"] >= T)
        after = near & (k["t"] <= T) & np.isnan(k["tab"][7])
        k["tab"][0:4, before] = v[:, None]
        k["tab"][4:8, after] = v[:, None]
        k["samples"] += 1

    def track_sample(self, stream=None):
        self._sample()
        self.log.append(("track_sample", self.clock))

    def _stepped(self, dt, n):
        for _ in range(n):
            assert self.trk is None or dt <= self.trk["H"]
            self.clock += dt
            if self.trk is not None:
                self._sample()

    def run_steps(self, dt, n):
        self._stepped(dt, n)
        self.log.append(("run_steps", n))

    def time_step(self, dt, flags=0):
        self._stepped(dt, 1)
        self.log.append(("time_step", 1))

    def track_fetch_begin(self, k0, n):
        assert self.open is None, "fetch_begin with a fetch open"
        assert 0 <= k0 and n >= 1 and k0 + n <= len(self.trk["t"])
        self.open = self.trk["tab"][:, k0:k0 + n].copy()
        self.log.append(("track_fetch_begin", k0, n, self.clock))

    def track_fetch_end(self):
        assert self.open is not None, "fetch_end without fetch_begin"
        out, self.open = self.open, None
        self.log.append(("track_fetch_end", out.shape[1]))
        return out

    def track_info(self):
        return len(self.trk["t"]), self.trk["H"], self.trk["samples"]

    def track_free(self):
        self.trk = None
        self.log.append(("track_free",))


def _fake_sim(n_steps, n=12):
    cfg = configs.bench06_box(n=n)
    m = models.WaveGrowth2D(**cfg.model, backend_factory=TrackBackend)
    return m, Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1)), cfg.Δt


def _events(m, dt, n_steps, n=60, seed=2):
    rng = np.random.default_rng(seed)
    x = m.grid.data.x[:, 0]
    t = rng.uniform(-1.5 * dt, (n_steps + 1.5) * dt, n)
    t[:4] = [0.0, 3 * dt, n_steps * dt, 3 * dt]          # on clocks, two of them equal
    pts = np.stack([rng.uniform(x[0], x[-1], n), rng.uniform(x[0], x[-1], n)], axis=1)
    return t, pts


def test_sort_and_the_callers_order():
    m, sim, dt = _fake_sim(5)
    t = np.array([50.0, 10.0, 30.0, 10.0, 20.0])
    pts = [(1000.0 * k, 2000.0 * k) for k in range(5)]
    tw = TrackWriter(m, times=t, points=pts)
    assert tw.order.tolist() == [1, 3, 4, 2, 0]          # stable: equal times keep the caller's order
    assert tw.sorted_times.tolist() == [10.0, 10.0, 20.0, 30.0, 50.0]
    c, w = locate_points(m.grid, [pts[k] for k in tw.order])
    assert np.array_equal(tw.corners_ij, np.concatenate([c[:, :, 0].T, c[:, :, 1].T])) and np.array_equal(tw.weights, w.T)
    assert tw.corners_ij.shape == (8, 5) and tw.weights.shape == (4, 5)
    assert tw.names == [f"event_{k}" for k in range(5)]
    for kw, text in ((dict(times=[1.0], points=pts), "same events"), (dict(times=[], points=[]), "same events"),
                     (dict(times=[np.nan], points=pts[:1]), "finite"), (dict(times=t, points=pts, names=["a"]), "one name per event"),
                     (dict(times=[1.0], points=[(-5000.0, 0.0)]), "outside")):
        with pytest.raises(ValueError, match=text):
            TrackWriter(m, **kw)


@pytest.mark.parametrize("fmt", ["npy", "hdf5"])
@pytest.mark.parametrize("with_ckpt", [False, True])
def test_hooks_fetches_and_the_file(tmp_path, fmt, with_ckpt):
    if fmt == "hdf5":
        from picles_amd import storing
        try:
            storing.hdf5()
        except OSError:
            pytest.skip("no libhdf5 on this machine")
    n_steps = 12
    m, sim, dt = _fake_sim(n_steps)
    t, pts = _events(m, dt, n_steps)
    names = [f"pass_{k}" for k in range(len(t))]
    if with_ckpt:
        sim.output_writers["checkpointer"] = Checkpointer(m, schedule=5, dir=tmp_path / "ck")
    tw = sim.output_writers["tracks"] = TrackWriter(m, times=t, points=pts, names=names, path=tmp_path, format=fmt)
    assert tw.kind == "tracks" and tw.needs == "track_init" and all(order[-1] == "tracks" for order in PHASE_ORDER.values())
    assert tw.steps_allowed(m.backend, 0) == NO_LIMIT
    run(sim)
    log = m.backend.log
    calls = [c for c in log if c[0].startswith("track_") or c[0] in ("run_steps", "time_step")]
    chunks = [5, 5, 2] if with_ckpt else [12]          # this writer ends no chunk: the checkpointer's iterations do
    assert [c[1] for c in calls if c[0] == "run_steps"] == chunks and not [c for c in calls if c[0] == "time_step"]
    # the hook order: the set and the sample of the initial state, then per chunk fetch_end (of the chunk before) and ONE fetch_begin
    assert calls[0] == ("track_init", len(t), dt) and calls[1] == ("track_sample", 0.0) and calls[2][0] == "run_steps"
    assert calls[-1] == ("track_free",)
    st = np.sort(t)
    k, begun, fetched, clock = 2, 0, 0, 0.0
    for n in chunks:
        assert calls[k] == ("run_steps", n)
        k += 1
        for _ in range(n):
            clock += dt
        if begun > fetched:          # first the end of the fetch begun a chunk earlier ...
            assert calls[k] == ("track_fetch_end", begun - fetched)
            k, fetched = k + 1, begun
        done = int(np.searchsorted(st, clock, side="right"))
        assert done > begun          # ... then ONE begin, of the events completed since
        assert calls[k] == ("track_fetch_begin", begun, done - begun, clock)
        k, begun = k + 1, done
    # finish: the open fetch, then the rest, then the set goes
    assert calls[k] == ("track_fetch_end", begun - fetched)
    assert calls[k + 1] == ("track_fetch_begin", begun, len(t) - begun, clock) and calls[k + 2] == ("track_fetch_end", len(t) - begun)
    assert calls[k + 3] == ("track_free",) and len(calls) == k + 4
    assert len([c for c in calls if c[0] == "track_fetch_begin"]) == len(chunks) + 1
    # the file: the caller's order, (var, event)
    out = read_track_output(tmp_path)
    assert out["data"].shape == (8, len(t)) and list(out["var_names"]) == list(VAR_NAMES) and list(out["names"]) == names
    assert out["time"].tolist() == t.tolist() and out["x"].tolist() == pts[:, 0].tolist() and out["y"].tolist() == pts[:, 1].tolist()
    clocks = np.array([0.0])
    for _ in range(n_steps):
        clocks = np.append(clocks, clocks[-1] + dt)
    for k in range(len(t)):
        inside = clocks[0] <= t[k] <= clocks[-1]
        if not inside:
            assert np.isnan(out["data"][:, k]).all()
            assert np.isnan(out["t_before"][k]) or np.isnan(out["t_after"][k])
            continue
        tb, ta = clocks[clocks <= t[k]].max(), clocks[clocks >= t[k]].min()
        assert out["t_before"][k] == tb and out["t_after"][k] == ta
        eb, ea = 1.0 + tb / 1000.0, 1.0 + ta / 1000.0
        e = eb if ta == tb else eb + ((t[k] - tb) / (ta - tb)) * (ea - eb)
        assert out["data"][0, k] == e and out["data"][1, k] == 0.5 and out["data"][2, k] == 0.25 and out["data"][3, k] == 4.0 * math.sqrt(e)
    assert (fmt == "npy") == (tmp_path / "tracks.json").exists() and (fmt == "hdf5") == (tmp_path / "tracks.h5").exists()


def test_per_step_loop_fetches_at_every_iteration(tmp_path):
    m, sim, dt = _fake_sim(6)
    m.backend.get_state = lambda: np.zeros((12, 12, 3))
    m.backend.state_gen = 0
    t, pts = _events(m, dt, 6, n=30)
    sim.output_writers["tracks"] = TrackWriter(m, times=t, points=pts, path=tmp_path, format="npy")
    run(sim, cash_store=True)
    calls = [c[0] for c in m.backend.log if c[0].startswith("track_fetch") or c[0] == "time_step"]
    assert calls.count("time_step") == 6 and calls.count("track_fetch_begin") == calls.count("track_fetch_end")
    for a, b in zip(calls, calls[1:]):
        assert not (a == b == "track_fetch_begin")          # never two begins without the end between them
    out = read_track_output(tmp_path)
    assert np.isfinite(out["data"][0, (t >= 0.0) & (t <= 6 * dt)]).all()


def test_refusals():
    m, sim, dt = _fake_sim(3)
    # a backend without track_init
    cfg = configs.bench06_box(n=12)
    plain = models.WaveGrowth2D(**cfg.model, backend_factory=FakeBackend)
    s2 = Simulation(plain, Δt=cfg.Δt, stop_time=cfg.Δt)
    s2.output_writers["tracks"] = TrackWriter(plain, times=[10.0], points=[(1000.0, 1000.0)])
    with pytest.raises(NotImplementedError, match="TrackWriter needs a backend with track_init"):
        run(s2)
    assert not [c for c in plain.backend.log if c[0] in ("seed", "run_steps")]
    # a SlabModel, at construction and at run()
    SlabModel = type("SlabModel", (), {})
    with pytest.raises(NotImplementedError, match="slabs do not carry a track set"):
        TrackWriter(SlabModel(), times=[10.0], points=[(0.0, 0.0)])
    tw = TrackWriter(None, times=[10.0], points=[(0.0, 0.0)])
    fake = type("S", (), {"model": SlabModel(), "Δt": 600.0})()
    with pytest.raises(NotImplementedError, match="slabs do not carry a track set"):
        tw.check_run(fake, [tw])
