"""Nests and chunked runs under a gridded wind that varies in time, and a child started from its parent, on the CPU box
(picles_amd/nesting.py, picles_amd/simulations.py): `prolong_state` against a brute-force scalar restatement on hostile values; the
chunk logic of run() and NestForcing over the recording backends of tests/test_nesting_host.py, extended here with a `set_wind_grid`
that records; the refusals, before anything is seeded.

The lattices of tests/test_gpu_nest_lattice.py and tests/test_gpu_nest_prolong.py are built here (`lattice_winds`), so that the
files speak of the same winds."""
import math

import numpy as np
import pytest

from picles_amd import configs, models
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import NestForcing, prolong_state, prolong_tables, start_from_parent
from picles_amd.run_statistics import StatisticsWriter
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter, locate_points
from picles_amd.wind_emulator import GriddedWinds, IdealizedWindGrid, wind_interpolator
from test_nesting_host import C_DX, C_X0, C_Y0, K_SHAPE, LAND, LX, LY, P_DX, P_SHAPE, W_SHAPE, NestBackend, _winds, child_cfg, parent_cfg
from test_run_stats_host import StatBackend
from test_station_output_host import ProbeBackend

WRAP_X0 = 241000.0                  # a K child whose last column (x = 379 km) lies in P's periodic wrap cell (378 km, 384 km): corners 63 and 0
LATTICE_T = 9000.0                  # the lattices' last time knot: a multiple of both spacings, behind every run here


def lattice_winds(spacing):
    """L900 / L250: smooth_winds(10, 10, LX, LY) times (1 + 0.3 sin(2 pi t / 5400)) tabulated over P's period at 12 km and `spacing`
    seconds, piecewise linear in time"""
    w = configs.smooth_winds(10.0, 10.0, LX, LY)
    f = lambda t: 1.0 + 0.3 * np.sin(2.0 * np.pi * t / 5400.0)
    lat = IdealizedWindGrid(lambda x, y, t: w.u(x, y, t) * f(t), lambda x, y, t: w.v(x, y, t) * f(t),
                            dict(Lx=LX, Ly=LY, T=LATTICE_T), dict(dx=12000.0, dy=12000.0, dt=float(spacing)))
    return wind_interpolator(lat, time_mode="linear")


def under(cfg, winds):
    """the config under these winds, declared as varying in time"""
    cfg = _winds(cfg, winds)
    cfg.model["winds_static"] = False
    return cfg


# ---- prolong_state against a scalar restatement ----
def _hostile_parent_state():
    rng = np.random.default_rng(23)
    nx, ny = P_SHAPE
    S = np.stack([np.exp(rng.uniform(-6, 2, P_SHAPE)), rng.normal(0, 0.05, P_SHAPE), rng.normal(0, 0.05, P_SHAPE)], axis=-1)
    S[LAND] = 0.0                                   # the 3 x 3 dry block: x 60..72 km, y 6..18 km
    S[20, 5] = (np.nan, 0.1, 0.1)
    S[21, 5] = (1.0, np.inf, 0.1)
    S[22, 5] = (1.0, 0.1, -np.inf)
    S[23, 5] = (0.0, 0.1, 0.1)
    S[24, 5] = (-1.0, 0.1, 0.1)
    S[25, 5] = (1.0, 0.0, 0.0)
    S[26, 5] = (1e-300, 1e-170, 1e-170)             # m² underflows to zero: dry
    S[63, 8] = (np.nan, np.nan, np.nan)             # a corner of the wrap cell
    S[0, 9] = (2.0, -np.inf, 0.0)
    S[50:53, 2:5] = 0.0                             # a second 3 x 3 dry block, under the child across the wrap cell
    S[50:53, 2:5, 0] = 1.0                          # ... with energy and zero momentum
    return S


def _wet(e, mx, my):
    return math.isfinite(e) and math.isfinite(mx) and math.isfinite(my) and e > 0.0 and mx * mx + my * my > 0.0


def _prolong_scalar(S, pg, cg):
    """k_nest_prolong, node by node, in Python floats (IEEE doubles, one rounding per operation); corners and weights from
    locate_points, point by point.  Returns the State and, per node, the number of wet corners"""
    cx, cy = np.asarray(cg.data.x)[:, 0], np.asarray(cg.data.y)[0, :]
    out = np.empty((len(cx), len(cy), 3))
    wet_corners = np.empty((len(cx), len(cy)), dtype=np.int64)
    for i, x in enumerate(cx):
        for j, y in enumerate(cy):
            corners, weights = locate_points(pg, [(float(x), float(y))])
            W = SE = SX = SY = 0.0
            nwet = 0
            for c in range(4):
                e, mx, my = (float(v) for v in S[corners[0, c, 0], corners[0, c, 1]])
                w = float(weights[0, c])
                if _wet(e, mx, my):
                    nwet += 1
                    W = W + w
                    SE = SE + w * e
                    SX = SX + w * mx
                    SY = SY + w * my
            ok = False
            if W > 0.0:
                E, MX, MY = SE / W, SX / W, SY / W
                ok = MX * MX + MY * MY > 0.0
            out[i, j] = (E, MX, MY) if ok else (0.0, 0.0, 0.0)
            wet_corners[i, j] = nwet
    return out, wet_corners


@pytest.mark.parametrize("x0", [C_X0, WRAP_X0], ids=["K70x9", "K70x9-across-the-wrap-cell"])
def test_prolong_state_equals_the_scalar_restatement_bit_for_bit(x0):
    pg, cg = parent_cfg(land=True).model["grid"], child_cfg(K_SHAPE, x0=x0).model["grid"]
    S = _hostile_parent_state()
    got = prolong_state(S, pg, cg)
    want, wet_corners = _prolong_scalar(S, pg, cg)
    assert got.shape == K_SHAPE + (3,) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    zeroed = (got == 0.0).all(axis=-1)
    assert np.array_equal(zeroed, wet_corners == 0)          # (random weights and values: no momentum cancels to zero)
    assert zeroed.any() and (~zeroed).any() and np.isfinite(got).all()
    assert ((wet_corners > 0) & (wet_corners < 4)).any()     # and nodes that lose some of their corners
    ix0, ix1, wx, iy0, iy1, wy = prolong_tables(pg, cg)
    assert [a.dtype for a in (ix0, ix1, wx, iy0, iy1, wy)] == [np.int32, np.int32, np.float64] * 2
    assert [a.shape for a in (ix0, ix1, wx, iy0, iy1, wy)] == [(K_SHAPE[0],)] * 3 + [(K_SHAPE[1],)] * 3
    assert (0.0 <= wx).all() and (wx <= 1.0).all() and (0.0 <= wy).all() and (wy <= 1.0).all()
    if x0 == WRAP_X0:
        assert (ix0[-1], ix1[-1]) == (63, 0) and ((ix0 == 63) & (ix1 == 0)).sum() >= 1 and wx[-1] > 0.0 and ix0[0] < 63
    else:
        assert (ix1 == ix0 + 1).all()


# ---- chunk logic over the recording backends ----
class LatticeNestBackend(NestBackend):
    """NestBackend + a device that samples a wind lattice itself: the upload is recorded"""

    def set_wind_grid(self, lat, mesh_x0, mesh_y0, time_mode="linear"):
        self.log.append(("set_wind_grid", int(lat["nt"]), time_mode))

    def time_step(self, dt, flags=0):
        raise AssertionError("the per-step loop was entered")


def _pair(shape, n_child, child_winds, parent_winds, backend=LatticeNestBackend, ratio=3, parent_dt=600.0):
    pc, cc = parent_cfg(), child_cfg(shape)
    if parent_winds is not None:
        under(pc, parent_winds)
    if child_winds is not None:
        under(cc, child_winds)
    pm = models.WaveGrowth2D(**pc.model, backend_factory=backend)
    cm = models.WaveGrowth2D(**cc.model, backend_factory=backend)
    journal = []
    for m, name in ((pm, "parent"), (cm, "child")):
        m.backend.journal, m.backend.name = journal, name
    dt = parent_dt / ratio
    psim = Simulation(pm, Δt=parent_dt, stop_time=parent_dt * 1000)
    csim = Simulation(cm, Δt=dt, stop_time=dt * (n_child - 1))
    return pm, psim, cm, csim, journal


@pytest.mark.parametrize("which", ["both-one-lattice", "both-two-lattices", "child-only", "parent-only"])
def test_a_nest_under_lattices_journals_what_it_journals_under_static_winds(which):
    L900, L250 = lattice_winds(900.0), lattice_winds(250.0)
    cw, pw = {"both-one-lattice": (L900, L900), "both-two-lattices": (L900, L250), "child-only": (L900, None), "parent-only": (None, L250)}[which]
    journals, uploads = [], []
    for child_winds, parent_winds in ((None, None), (cw, pw)):
        pm, psim, cm, csim, journal = _pair(W_SHAPE, 11, child_winds, parent_winds)
        f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
        run(csim)
        assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps) == (11, 4, 4)
        journals.append(journal)
        uploads.append([[e for e in m.backend.log if e[0] in ("set_wind_grid", "set_winds")] for m in (cm, pm)])
    assert journals[0] == journals[1] and len(journals[0]) > 8
    assert {e[1] for e in journals[0]} == {"run_steps", "nest_sample"}
    for winds, log in zip((cw, pw), uploads[1]):          # each lattice once, and no host-sampled level beside it
        assert log == ([("set_wind_grid", len(winds.t), "linear")] if winds is not None else [("set_winds", 0.0)])


class OutputBackend(ProbeBackend, StatBackend):
    """the probe ring and the statistics set on one recording backend that samples its lattice itself"""

    def set_wind_grid(self, lat, mesh_x0, mesh_y0, time_mode="linear"):
        self.log.append(("set_wind_grid", int(lat["nt"]), time_mode))

    def _stepped(self, dt, n):
        for _ in range(n):
            before = self.clock
            ProbeBackend._stepped(self, dt, 1)
            self.clock = before
            StatBackend._stepped(self, dt, 1)


def test_a_plain_run_under_a_lattice_is_chunked(tmp_path):
    cfg = under(parent_cfg(), lattice_winds(250.0))
    m = models.WaveGrowth2D(**cfg.model, backend_factory=OutputBackend)
    sim = Simulation(m, Δt=600.0, stop_time=600.0 * 9)
    sw = sim.output_writers["stations"] = StationWriter(m, points=[(30000.0, 30000.0), (100000.0, 40000.0)], path=tmp_path, format="npy")
    st = sim.output_writers["statistics"] = StatisticsWriter(m, fields=("mean",), schedule=1, window=3, path=tmp_path, format="npy")
    assert m.runs_chunked(600.0) and not m._winds_static
    run(sim)
    log = m.backend.log
    assert sum(e[1] for e in log if e[0] == "run_steps") == 10 and not [e for e in log if e[0] == "time_step"]
    assert [e for e in log if e[0] in ("set_wind_grid", "set_winds")] == [("set_wind_grid", 37, "linear")]
    assert sw.iterations == list(range(11)) and [r[3] for r in st.records] == [3, 6, 9, 10]      # (the last window is cut by the run's end)
    # the same writers under closures that vary in time keep the per-step loop
    w = configs.smooth_winds(10.0, 10.0, LX, LY)
    tv = type(w)(u=lambda x, y, t: w.u(x, y, t) * (1.0 + 1e-4 * t), v=lambda x, y, t: w.v(x, y, t) * (1.0 + 1e-4 * t))
    m2 = models.WaveGrowth2D(**under(parent_cfg(), tv).model, backend_factory=OutputBackend)
    sim2 = Simulation(m2, Δt=600.0, stop_time=600.0 * 2)
    sim2.output_writers["stations"] = StationWriter(m2, points=[(30000.0, 30000.0)], path=tmp_path / "tv", format="npy")
    assert not m2.runs_chunked(600.0) and not m2.runs_chunked(600.0, detect=True)
    run(sim2)
    assert [e[0] for e in m2.backend.log if e[0] in ("run_steps", "time_step")] == ["time_step"] * 3


# ---- refusals, before anything is seeded ----
def _time_varying_closures():
    w = configs.smooth_winds(10.0, 10.0, LX, LY)
    return type(w)(u=lambda x, y, t: w.u(x, y, t) * (1.0 + 1e-4 * t), v=lambda x, y, t: w.v(x, y, t) * (1.0 + 1e-4 * t))


def _seeds(*ms):
    return [e for m in ms for e in m.backend.log if e[0] == "seed"]


@pytest.mark.parametrize("who", ["child", "parent"])
def test_closures_that_vary_in_time_stay_refused(who):
    tv = _time_varying_closures()
    pm, psim, cm, csim, _ = _pair(K_SHAPE, 6, tv if who == "child" else None, tv if who == "parent" else lattice_winds(900.0))
    (cm if who == "child" else pm)._winds_static = None          # not declared: found out by sampling
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
    with pytest.raises(NotImplementedError, match=f"the {who} model.*static winds.*GriddedWinds lattice"):
        run(csim)
    assert not _seeds(cm, pm)


@pytest.mark.parametrize("who", ["child", "parent"])
def test_a_lattice_on_a_backend_that_cannot_sample_it_is_refused(who):
    L = lattice_winds(900.0)
    pm, psim, cm, csim, _ = _pair(K_SHAPE, 6, L if who == "child" else None, L if who == "parent" else None, backend=NestBackend)
    assert not hasattr(cm.backend, "set_wind_grid")
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
    with pytest.raises(NotImplementedError, match=f"the {who} model.*static winds"):
        run(csim)
    assert not _seeds(cm, pm)
    # and run() alone takes the per-step loop there: the host samples the lattice
    m = cm if who == "child" else pm
    assert isinstance(m.winds, GriddedWinds) and not m.runs_chunked(600.0)


class ProlongBackend(LatticeNestBackend):
    def nest_prolong(self, parent, *tables_and_dt):
        self.clock = parent.clock
        self.log.append(("nest_prolong", parent.clock))


def test_start_from_parent_refusals_and_clocks():
    # a parent that was never run
    pm, psim, cm, csim, _ = _pair(K_SHAPE, 6, None, None, backend=ProlongBackend)
    with pytest.raises(ValueError, match="the parent was never run"):
        start_from_parent(csim, psim)
    # a child node outside the parent (an open parent: rows up to y = 96 km > 90 km)
    pc = parent_cfg()
    pc.model["grid"] = TwoDCartesianGridMesh(P_DX * 63, 64, P_DX * 15, 16, periodic_boundary=(False, False))
    om = models.WaveGrowth2D(**{**pc.model, "periodic_boundary": False}, backend_factory=ProlongBackend)
    osim = Simulation(om, Δt=600.0, stop_time=600.0)
    initialize_simulation(osim)
    far = models.WaveGrowth2D(**child_cfg(K_SHAPE, y0=80000.0).model, backend_factory=ProlongBackend)
    fsim = Simulation(far, Δt=200.0, stop_time=1000.0)
    with pytest.raises(ValueError, match="outside the mesh"):
        start_from_parent(fsim, osim)
    # the child's closures vary in time: the sentence of the nest
    tvm = models.WaveGrowth2D(**under(child_cfg(K_SHAPE), _time_varying_closures()).model, backend_factory=ProlongBackend)
    with pytest.raises(NotImplementedError, match="static winds"):
        start_from_parent(Simulation(tvm, Δt=200.0, stop_time=1000.0), osim)
    # the same model twice, and a backend without the call
    with pytest.raises(ValueError, match="another model"):
        start_from_parent(osim, osim)
    initialize_simulation(psim)
    plain = models.WaveGrowth2D(**child_cfg(K_SHAPE).model, backend_factory=NestBackend)
    with pytest.raises(NotImplementedError, match="nest_prolong"):
        start_from_parent(Simulation(plain, Δt=200.0, stop_time=1000.0), psim)
    for m, s in ((cm, csim), (far, fsim), (tvm, None), (plain, None)):
        assert not _seeds(m) and not [e for e in m.backend.log if e[0] == "nest_prolong"] and (s is None or not s.initialized)
    # and the start itself: the parent run to t = 1800, the child's clocks afterwards, the nested run behind it
    psim.stop_time = 1200.0
    run(psim)
    assert pm.clock.time == 1800.0 and pm.clock.iteration == 3
    csim.stop_time = 1800.0 + 200.0 * 5
    start_from_parent(csim, psim)
    assert csim.initialized and (cm.clock.time, cm.clock.iteration, cm.backend.clock) == (1800.0, 0, 1800.0)
    assert [e for e in cm.backend.log if e[0] in ("seed", "set_winds", "nest_prolong")] == [("set_winds", 1800.0), ("nest_prolong", 1800.0)]
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
    psim.stop_time = 1e9
    run(csim)
    assert not _seeds(cm) and (cm.clock.iteration, cm.clock.time, f.parent_steps, pm.clock.iteration) == (6, 3000.0, 2, 5)
    assert np.array_equal(f.times[:-1], [1800.0, 2400.0, 3000.0])
