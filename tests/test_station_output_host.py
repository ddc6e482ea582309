"""StationWriter on the CPU box: points -> corners and weights and the per-station arithmetic against hand values and against
the scalar restatement (tests/_station_numpy.py), the writer + run() over a backend that records its calls (the pattern of
tests/test_field_output_host.py), the file round trip in both formats, the cadence after a pickup."""
import itertools
import math

import numpy as np
import pytest

import _station_numpy as R
from picles_amd import configs, models
from picles_amd.checkpointing import Checkpointer
from picles_amd.field_output import FieldWriter
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import (VAR_NAMES, StationWriter, locate_points, read_station_output, station_records)
from test_field_output_host import FakeBackend

G, RG = 9.81, 0.85


def _grid(per=(False, False), nx=6, ny=5):
    return TwoDCartesianGridMesh(0.0, 1000.0 * (nx - 1), nx, 100.0, 100.0 + 500.0 * (ny - 1), ny, periodic_boundary=per)


def test_points_to_corners_hand_values():
    g = _grid()
    c, w = locate_points(g, [(2000.0, 1100.0), (2500.0, 1350.0), (5000.0, 2100.0), (0.0, 100.0), (4250.0, 225.0)])
    assert c[0].tolist() == [[2, 2], [3, 2], [2, 3], [3, 3]] and w[0].tolist() == [1.0, 0.0, 0.0, 0.0]           # on a node
    assert c[1].tolist() == [[2, 2], [3, 2], [2, 3], [3, 3]] and w[1].tolist() == [0.25, 0.25, 0.25, 0.25]       # a cell centre
    assert c[2].tolist() == [[4, 3], [5, 3], [4, 4], [5, 4]] and w[2].tolist() == [0.0, 0.0, 0.0, 1.0]           # the last node of both open axes
    assert c[3].tolist() == [[0, 0], [1, 0], [0, 1], [1, 1]] and w[3].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert c[4].tolist() == [[4, 0], [5, 0], [4, 1], [5, 1]] and w[4].tolist() == [0.75 * 0.75, 0.25 * 0.75, 0.75 * 0.25, 0.25 * 0.25]
    for bad in [(-1.0, 500.0), (5000.5, 500.0), (100.0, 99.0), (100.0, 2100.5)]:
        with pytest.raises(ValueError, match="outside"):
            locate_points(g, [bad])
    # across the periodic wrap: the cell between the last node and the first
    gp = _grid(per=(True, True))
    c, w = locate_points(gp, [(5500.0, 2350.0)])
    assert c[0].tolist() == [[5, 4], [0, 4], [5, 0], [0, 0]] and w[0].tolist() == [0.25, 0.25, 0.25, 0.25]
    with pytest.raises(ValueError, match="outside"):
        locate_points(gp, [(6000.0, 500.0)])
    gt = _grid(per=(True, "tripolar_north"))
    locate_points(gt, [(5500.0, 1599.0)])
    with pytest.raises(ValueError, match="top cell row"):
        locate_points(gt, [(100.0, 1600.0)])
    # and the scalar restatement agrees on corners and weights, bit for bit
    xs, ys = g.data.x[:, 0], g.data.y[0, :]
    rng = np.random.default_rng(3)
    pts = [(float(rng.uniform(0, 5000)), float(rng.uniform(100, 2100))) for _ in range(50)]
    for grid, per in ((g, (False, False)), (gp, (True, True))):
        c, w = locate_points(grid, pts)
        for k, p in enumerate(pts):
            want = R.corners_of(p, xs, ys, periodic=per)
            assert [tuple(x) for x in c[k].tolist()] == [ij for ij, _ in want]
            assert w[k].tolist() == [float(x) for _, x in want]


def test_station_arithmetic_hand_values():
    # one sample, four nodes: e, m_x, m_y
    v = np.zeros((1, 3, 4))
    v[0, :, 0] = [4.0, 3.0, 4.0]
    v[0, :, 1] = [1.0, 0.0, 2.0]
    v[0, :, 2] = [9.0, -1.0, 0.0]
    v[0, :, 3] = [2.0, 1.0, 1.0]
    idx = np.array([[0, 1, 2, 3]])
    w = np.array([[0.25, 0.25, 0.25, 0.25]])
    r = station_records(v, idx, w, G, RG)[0, 0]
    E, MX, MY = 16.0 * 0.25 / 1.0, 3.0 * 0.25, 7.0 * 0.25
    assert r[0] == 4.0 and r[1] == 0.75 and r[2] == 1.75
    M2 = MX * MX + MY * MY
    assert r[3] == 4.0 * math.sqrt(E) == 8.0
    assert r[5] == (MX * E) / (2.0 * M2) and r[6] == (MY * E) / (2.0 * M2)
    assert r[4] == (12.566370614359172 * max((E / (2.0 * math.sqrt(M2))) / RG, 0.1)) / G
    assert r[7] == math.atan2(MY, MX)
    # one dry corner (land: zeros): the mean over the three wet ones, normalised by their weight
    v1 = v.copy(); v1[0, :, 1] = 0.0
    r1 = station_records(v1, idx, w, G, RG)[0, 0]
    assert r1[0] == (0.25 * 4.0 + 0.25 * 9.0 + 0.25 * 2.0) / 0.75 and r1[1] == (0.75 - 0.25 + 0.25) / 0.75
    # a NaN corner and an e > 0, m = 0 corner are dry too
    v2 = v.copy(); v2[0, 0, 1] = np.nan; v2[0, 1:, 3] = 0.0
    r2 = station_records(v2, idx, w, G, RG)[0, 0]
    assert r2[0] == (0.25 * 4.0 + 0.25 * 9.0) / 0.5
    # four dry corners: every variable NaN; so is a station whose only wet corner has weight zero
    assert np.isnan(station_records(np.zeros((1, 3, 4)), idx, w, G, RG)).all()
    v3 = np.zeros((1, 3, 4)); v3[0, :, 1] = [1.0, 1.0, 1.0]
    assert np.isnan(station_records(v3, idx, np.array([[1.0, 0.0, 0.0, 0.0]]), G, RG)).all()
    # means that cancel: M2 == 0
    v4 = np.zeros((1, 3, 2)); v4[0, :, 0] = [1.0, 1.0, 2.0]; v4[0, :, 1] = [1.0, -1.0, -2.0]
    assert np.isnan(station_records(v4, np.array([[0, 1]]), np.array([[0.5, 0.5]]), G, RG)).all()
    # nodes=: weight 1 on the node — its values come back bit for bit
    x = np.array([0.1 + 0.2, 1.0 / 3.0, -2.0 / 7.0])
    v5 = np.zeros((1, 3, 1)); v5[0, :, 0] = x
    assert station_records(v5, np.array([[0]]), np.ones((1, 1)), G, RG)[0, 0, :3].tolist() == x.tolist()


def test_vectorised_records_equal_the_scalar_restatement_bitwise():
    rng = np.random.default_rng(11)
    nn, ns, S = 40, 25, 6
    v = rng.normal(size=(S, 3, nn)) * np.array([1.0, 0.3, 0.3])[None, :, None]
    v[:, 0] = np.abs(v[:, 0])
    v[:, :, rng.integers(nn, size=8)] = 0.0          # dry nodes
    v[2, 1, 5] = np.nan
    idx = rng.integers(nn, size=(ns, 4))
    v[:, :, 0] = 0.0
    idx[0, :] = 0                                    # a station with four dry corners
    w = rng.uniform(size=(ns, 2))
    w = np.stack([(1 - w[:, 0]) * (1 - w[:, 1]), w[:, 0] * (1 - w[:, 1]), (1 - w[:, 0]) * w[:, 1], w[:, 0] * w[:, 1]], axis=1)
    got = station_records(v, idx, w, G, RG)
    for k in range(S):
        for s in range(ns):
            want = R.record([(tuple(v[k, :, idx[s, c]]), w[s, c]) for c in range(4)], G, RG)
            assert np.array_equal(got[k, s], want, equal_nan=True), (k, s, got[k, s], want)
    assert np.isnan(got).any() and np.isfinite(got).any()


# ---- StationWriter + run() over a backend that records its calls ----
class ProbeBackend(FakeBackend):
    """FakeBackend + the probe ring: a sample's values are its step number, the ring refuses what the library refuses"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.probe = None
        self.max_pending = 0

    def probe_init(self, nodes, every=1, first=1, capacity=64):
        assert self.probe is None, "second probe_init without probe_free"
        self.probe = dict(nodes=np.asarray(nodes), every=every, first=first, cap=capacity, s=0, ring=[])
        self.log.append(("probe_init", len(nodes), every, first, capacity))

    def probe_free(self):
        self.probe = None
        self.log.append(("probe_free",))

    def _take(self):
        p = self.probe
        assert len(p["ring"]) < p["cap"], "a sample was asked for with the ring full"
        p["ring"].append((p["s"], self.clock))
        self.max_pending = max(self.max_pending, len(p["ring"]))

    def probe_sample(self, stream=None):
        self._take()
        self.log.append(("probe_sample", self.clock))

    def _stepped(self, dt, n):
        p = self.probe
        for _ in range(n):
            self.clock += dt
            if p is not None:
                p["s"] += 1
                if p["s"] >= p["first"] and (p["s"] - p["first"]) % p["every"] == 0:
                    self._take()

    def run_steps(self, dt, n):
        self._stepped(dt, n)
        self.log.append(("run_steps", n))

    def time_step(self, dt, flags=0):
        self._stepped(dt, 1)
        self.log.append(("time_step", 1))

    @property
    def probe_pending(self):
        return len(self.probe["ring"]) if self.probe else 0

    def probe_pop(self, max_samples=None):
        p = self.probe
        m = len(p["ring"]) if max_samples is None else min(max_samples, len(p["ring"]))
        assert m > 0
        got, p["ring"] = p["ring"][:m], p["ring"][m:]
        n = len(p["nodes"])
        v = np.empty((m, 3, n))
        for k, (s, _) in enumerate(got):
            v[k, 0], v[k, 1], v[k, 2] = 1.0 + s, 0.5 * (1 + s), np.arange(n) + 1.0
        self.log.append(("probe_pop", [s for s, _ in got]))
        return v, np.array([t for _, t in got]), np.array([s for s, _ in got], dtype=np.int64)


def _fake_sim(n_steps, n=12):
    cfg = configs.bench06_box(n=n)
    m = models.WaveGrowth2D(**cfg.model, backend_factory=ProbeBackend)
    return m, Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1)), cfg.Δt


@pytest.mark.parametrize("fmt", ["npy", "hdf5"])
def test_writer_alone_and_the_file_round_trip(tmp_path, fmt):
    if fmt == "hdf5":
        from picles_amd import storing
        try:
            storing.hdf5()
        except OSError:
            pytest.skip("no libhdf5 on this machine")
    m, sim, dt = _fake_sim(23)
    x = m.grid.data.x[:, 0]
    sw = sim.output_writers["stations"] = StationWriter(m, points=[(x[3], x[4]), (0.5 * (x[3] + x[4]), x[7])], names=["buoy", "rig"],
                                                        schedule=1, path=tmp_path, capacity=8, format=fmt)
    run(sim)
    b = m.backend
    log = b.log
    assert [c[0] for c in log if c[0] in ("time_step", "run_steps")] == ["run_steps"] * len([c for c in log if c[0] == "run_steps"])
    assert sum(c[1] for c in log if c[0] == "run_steps") == 23
    assert max(c[1] for c in log if c[0] == "run_steps") <= 4 and b.max_pending <= 8          # half the ring per chunk
    assert [c for c in log if c[0] == "probe_init"] == [("probe_init", len(sw.probe_nodes), 1, 1, 8)]
    popped = [s for c in log if c[0] == "probe_pop" for s in c[1]]
    assert popped == list(range(24))                                                          # the seeded state and every step, in order
    out = read_station_output(tmp_path)
    assert out["data"].shape == (24, 2, 8) and list(out["var_names"]) == list(VAR_NAMES) and list(out["names"]) == ["buoy", "rig"]
    assert out["time"].tolist() == [k * dt for k in range(24)] and out["iteration"].tolist() == list(range(24))
    assert out["x"].tolist() == [x[3], 0.5 * (x[3] + x[4])] and out["y"].tolist() == [x[4], x[7]]
    assert out["data"][:, 0, 0].tolist() == [1.0 + k for k in range(24)]                       # e of the sample = 1 + its step
    assert sw.iterations == list(range(24)) and m.clock.iteration == 23


@pytest.mark.parametrize("with_ckpt,with_fw,cap,sched", list(itertools.product([False, True], [False, True], [1, 2, 5, 64], [1, 3])))
def test_fast_branch_chunks_never_overrun_the_ring(tmp_path, with_ckpt, with_fw, cap, sched):
    m, sim, dt = _fake_sim(40)
    if with_ckpt:
        sim.output_writers["checkpointer"] = Checkpointer(m, schedule=7, dir=tmp_path / "ck")
    if with_fw:
        sim.output_writers["fields"] = FieldWriter(m, schedule=5, path=tmp_path, format="npy")
    sw = sim.output_writers["stations"] = StationWriter(m, nodes=[(1, 2), (3, 4), (1, 2)], schedule=sched, path=tmp_path, capacity=cap,
                                                        format="npy")
    run(sim)            # (ProbeBackend asserts on every sample that the ring has room)
    b = m.backend
    assert all(c[0] != "time_step" for c in b.log) and sum(c[1] for c in b.log if c[0] == "run_steps") == 40
    assert b.max_pending <= cap
    want = [0] + [k for k in range(1, 41) if k % sched == 0]
    assert sw.iterations == want
    out = read_station_output(tmp_path)
    assert out["iteration"].tolist() == want and out["data"].shape == (len(want), 3, 8)
    if with_ckpt:
        assert [c[1] for c in b.log if c[0] == "checkpoint_begin"] == [k * dt for k in (7, 14, 21, 28, 35)]
    if with_fw:
        assert [c[1] for c in b.log if c[0] == "diag_push"] == [k * dt for k in range(0, 41, 5)]
    # chunk ends: every checkpoint and output iteration is one
    ends = np.cumsum([c[1] for c in b.log if c[0] == "run_steps"]).tolist()
    for k in ([7, 14, 21, 28, 35] if with_ckpt else []) + (list(range(5, 41, 5)) if with_fw else []):
        assert k in ends


def test_per_step_loop_pops_before_the_ring_fills(tmp_path):
    m, sim, dt = _fake_sim(9)
    m.backend.get_state = lambda: np.zeros((12, 12, 3))
    m.backend.state_gen = 0
    sw = sim.output_writers["stations"] = StationWriter(m, nodes=[(0, 0)], schedule=2, path=tmp_path, capacity=2, format="npy")
    run(sim, cash_store=True)
    assert [c[0] for c in m.backend.log if c[0] in ("time_step", "run_steps")] == ["time_step"] * 9
    assert sw.iterations == [0, 2, 4, 6, 8] and m.backend.max_pending <= 2


def test_cadence_continues_after_a_pickup_off_the_schedule(tmp_path):
    """the probe step counter starts at the restored iteration: `first` is the distance to the next scheduled iteration"""
    m, sim, dt = _fake_sim(10)
    sw = sim.output_writers["stations"] = StationWriter(m, nodes=[(2, 2)], schedule=4, path=tmp_path, capacity=4, format="npy")
    assert [sw.first_step(it) for it in (0, 1, 3, 4, 10, 12)] == [4, 3, 1, 4, 2, 4]
    m.clock.iteration, m.clock.time = 10, 10 * dt                   # as load_checkpoint leaves the clock
    m.backend.clock = 10 * dt
    sim.initialized = True
    sim.stop_time = dt * 24
    run(sim)
    assert [c for c in m.backend.log if c[0] == "probe_init"] == [("probe_init", 1, 4, 2, 4)]
    assert sw.iterations == [10, 12, 16, 20, 24]
    out = read_station_output(tmp_path)
    assert out["time"].tolist() == [k * dt for k in (10, 12, 16, 20, 24)]
    # a second run on the same backend replaces the set
    sim.stop_time = dt * 30
    run(sim)
    assert [c[0] for c in m.backend.log if c[0] in ("probe_init", "probe_free")] == ["probe_init", "probe_free", "probe_init"]
    assert sw.iterations == [25, 28]


def test_argument_checks(tmp_path):
    m, sim, dt = _fake_sim(3)
    with pytest.raises(ValueError, match="either points"):
        StationWriter(m)
    with pytest.raises(ValueError, match="either points"):
        StationWriter(m, points=[(0.0, 0.0)], nodes=[(0, 0)])
    with pytest.raises(ValueError, match="one name per station"):
        StationWriter(m, nodes=[(0, 0)], names=["a", "b"])
    with pytest.raises(ValueError, match="node outside"):
        StationWriter(m, nodes=[(12, 0)])
    with pytest.raises(ValueError, match="outside"):
        StationWriter(m, points=[(-5.0, 0.0)])
    from helpers import make_model
    cfg = configs.example_00_minimal(n=9, L=16e3)
    mo = make_model(cfg, ("pmath", 1))
    s2 = Simulation(mo, Δt=cfg.Δt, stop_time=cfg.Δt)
    s2.output_writers["stations"] = StationWriter(mo, nodes=[(1, 1)], path=tmp_path)
    with pytest.raises(NotImplementedError, match="StationWriter needs a backend"):
        run(s2)
