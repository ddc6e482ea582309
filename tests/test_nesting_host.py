"""One-way nesting on the CPU box (picles_amd/nesting.py): the geometry of the two test children in the test parent against a
brute-force restatement, the time rule, the chunk logic of NestForcing over backends that record their calls and refuse what the
library refuses (the pattern of tests/test_boundary_forcing_host.py), the offline route's file reader, the Checkpointer and pickup
refusals, and the arithmetic of the mix kernel as a scalar restatement against station_records on hostile corners.

The cases of tests/test_gpu_nesting.py are built here (`parent_cfg`, `child_cfg`), so that both files speak of the same boxes."""
import math

import numpy as np
import pytest

from picles_amd import configs, models
from picles_amd.boundary_forcing import BoundaryForcing, from_station_output, rim_nodes
from picles_amd.checkpointing import Checkpointer
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import NestForcing, check_ratio, locate_in_parent, rim_points
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import NpyStationStore, StationWriter, VAR_NAMES, station_records
from test_boundary_forcing_host import ForcingBackend

P_SHAPE, W_SHAPE, K_SHAPE = (64, 16), (128, 12), (70, 9)
P_DX, C_DX = 6000.0, 2000.0
C_X0, C_Y0 = 31000.0, 17000.0           # no child node coincides with a parent node: every weight is non-trivial
LX, LY = P_SHAPE[0] * P_DX, P_SHAPE[1] * P_DX
LAND = (slice(10, 13), slice(1, 4))     # the 3 x 3 land block of P-land: x 60..72 km, y 6..18 km — under the child's south rim


def _winds(cfg, w):
    cfg.model["winds"] = w
    cfg.model["ODEsys"] = particle_equations(w.u, w.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=True, dissipation=True)
    return cfg


def parent_cfg(land=False, solver="DP5"):
    """(P): 64 x 16, fully periodic, dx = 6000 m, bench06_box's physics under smooth winds of the box's period"""
    nx, ny = P_SHAPE
    cfg = configs.bench06_box(n=16, dx=P_DX, periodic_grid=True)
    mask = np.ones(P_SHAPE, dtype=bool)
    if land:
        mask[LAND] = False
    cfg.model["grid"] = TwoDCartesianGridMesh(P_DX * (nx - 1), nx, P_DX * (ny - 1), ny, mask=mask, periodic_boundary=(True, True))
    cfg.model["ODEsets"].solver = solver
    return _winds(cfg, configs.smooth_winds(10.0, 10.0, LX, LY))


def child_cfg(shape, solver="DP5", x0=C_X0, y0=C_Y0, dx=C_DX):
    """(W) 128 x 12 / (K) 70 x 9: open boxes at dx = 2000 m inside P, under the same wind closure in the common frame"""
    nx, ny = shape
    cfg = configs.bench06_box(n=16, dx=dx, periodic_grid=False)
    cfg.model["grid"] = TwoDCartesianGridMesh(x0, x0 + dx * (nx - 1), nx, y0, y0 + dx * (ny - 1), ny, periodic_boundary=(False, False))
    cfg.model["ODEsets"].solver = solver
    cfg.Δt = 200.0
    return _winds(cfg, configs.smooth_winds(10.0, 10.0, LX, LY))


# ---- backends that record and refuse ----
class NestBackend(ForcingBackend):
    """ForcingBackend + the nest: levels come from a parent backend's clock; refuses what the library refuses"""

    journal = None
    name = "?"

    def run_steps(self, dt, n):
        super().run_steps(dt, n)
        if self.journal is not None:
            self.journal.append((self.name, "run_steps", n, self.clock))

    def bforce_init(self, nodes):
        super().bforce_init(nodes)
        self.nest = None

    def bforce_free(self):
        super().bforce_free()
        self.nest = None

    def bforce_set_levels(self, *a, **k):
        assert getattr(self, "nest", None) is None, "bforce_set_levels on a nested child"
        super().bforce_set_levels(*a, **k)

    def bforce_info(self):
        t0, _, t1, v1 = self.bf["levels"] or (0.0, None, 0.0, None)
        levels = 0 if self.bf["levels"] is None else (1 if v1 is None else 2)
        return len(self.bf["nodes"]), levels, t0, (t0 if levels < 2 else t1)

    def nest_init(self, parent, corner_nodes, index, weights):
        assert self.bf is not None and self.nest is None and parent is not self
        assert np.asarray(index).shape == (len(self.bf["nodes"]), 4) and np.asarray(index).max() < len(corner_nodes)
        self.nest = dict(parent=parent, samples=0)
        self.bf["levels"] = None
        self.log.append(("nest_init", len(corner_nodes)))

    def nest_sample(self):
        N, p = self.nest, self.nest["parent"]
        lv = self.bf["levels"]
        if lv is None:
            self.bf["levels"] = (p.clock, 0, p.clock, None)
        else:
            t0, _, t1, v1 = lv
            assert p.clock > t1, "nest_sample while the parent's clock has not moved past t1"
            self.bf["levels"] = (t0 if v1 is None else t1, 0, p.clock, 1)
        N["samples"] += 1
        self.log.append(("nest_sample", p.clock))
        if self.journal is not None:
            self.journal.append((self.name, "nest_sample", N["samples"], p.clock))

    def nest_free(self):
        self.nest = None
        self.log.append(("nest_free",))


def _pair(shape, n_child_steps, ratio=3, parent_dt=600.0, backend=NestBackend):
    pc, cc = parent_cfg(), child_cfg(shape)
    pm = models.WaveGrowth2D(**pc.model, backend_factory=backend)
    cm = models.WaveGrowth2D(**cc.model, backend_factory=backend)
    dt = parent_dt / ratio
    journal = []
    for m, name in ((pm, "parent"), (cm, "child")):
        m.backend.journal, m.backend.name = journal, name
    psim = Simulation(pm, Δt=parent_dt, stop_time=parent_dt * 1000)
    csim = Simulation(cm, Δt=dt, stop_time=dt * (n_child_steps - 1))
    return pm, psim, cm, csim, journal


# ---- geometry ----
def _brute(parent_grid, pts):
    """corners and weights per point, from the coordinates alone (periodic parent)"""
    xs, ys = parent_grid.data.x[:, 0], parent_grid.data.y[0, :]
    Nx, Ny = len(xs), len(ys)
    out = []
    for x, y in pts:
        i0 = max(i for i in range(Nx) if xs[i] <= x)
        j0 = max(j for j in range(Ny) if ys[j] <= y)
        wx, wy = (x - xs[0]) / P_DX - i0, (y - ys[0]) / P_DX - j0
        out.append(([(i0, j0), ((i0 + 1) % Nx, j0), (i0, (j0 + 1) % Ny), ((i0 + 1) % Nx, (j0 + 1) % Ny)],
                    [(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy]))
    return out


@pytest.mark.parametrize("shape", [W_SHAPE, K_SHAPE], ids=["W128x12", "K70x9"])
def test_corners_weights_and_deduplication(shape):
    pg, cg = parent_cfg().model["grid"], child_cfg(shape).model["grid"]
    rim = rim_nodes(cg, "rim")
    assert len(rim) == 2 * (shape[0] + shape[1]) - 4
    pts = [(C_X0 + C_DX * i, C_Y0 + C_DX * j) for i, j in rim]
    m = type("M", (), {"grid": cg})
    assert rim_points(m, side="rim") == pts
    corner_nodes, index, weights = locate_in_parent(pg, pts)
    assert len(np.unique(corner_nodes, axis=0)) == len(corner_nodes) < 4 * len(rim)
    for k, (cs, ws) in enumerate(_brute(pg, pts)):
        assert [tuple(corner_nodes[q]) for q in index[k]] == cs, k
        assert np.array_equal(weights[k], np.array(ws)), k
        assert 0.0 < weights[k].min() and abs(weights[k].sum() - 1.0) < 1e-15        # no child node coincides with a parent node
    assert set(map(tuple, corner_nodes)) == {c for cs, _ in _brute(pg, pts) for c in cs}


def test_a_child_that_reaches_outside_the_parent_is_refused():
    pc = parent_cfg()
    pc.model["grid"] = TwoDCartesianGridMesh(P_DX * 63, 64, P_DX * 15, 16, periodic_boundary=(False, False))
    pm = models.WaveGrowth2D(**{**pc.model, "periodic_boundary": False}, backend_factory=NestBackend)
    cm = models.WaveGrowth2D(**child_cfg(K_SHAPE, y0=80000.0).model, backend_factory=NestBackend)      # rows up to y = 96 km > 90 km
    with pytest.raises(ValueError, match="outside the mesh"):
        NestForcing(cm, parent=Simulation(pm, Δt=600.0, stop_time=6000.0), side="rim", ratio=3)


# ---- the time rule ----
def test_ratio_and_clock_rules():
    pm, psim, cm, csim, _ = _pair(K_SHAPE, 6)
    for bad in (2.5, 0, -1, "3"):
        with pytest.raises(ValueError, match="integer >= 1"):
            NestForcing(cm, parent=psim, side="rim", ratio=bad)
    with pytest.raises(ValueError, match="do not make one parent step"):
        NestForcing(cm, parent=psim, side="rim", ratio=3, Δt=200.0 * (1.0 + 1e-6))
    NestForcing(cm, parent=psim, side="rim", ratio=3, Δt=200.0 * (1.0 + 1e-15))
    assert check_ratio(3.0, 200.0, 600.0) == 3
    # the simulation's own step is held against the ratio before anything is seeded
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=2)
    with pytest.raises(ValueError, match="do not make one parent step"):
        run(csim)
    assert not [e for e in cm.backend.log if e[0] == "seed"]
    # clocks that differ when the run begins
    pm, psim, cm, csim, _ = _pair(K_SHAPE, 6)
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
    from picles_amd.simulations import initialize_simulation
    initialize_simulation(psim)
    pm.clock.time = 600.0
    with pytest.raises(ValueError, match="clock"):
        run(csim)


# ---- chunk logic ----
@pytest.mark.parametrize("ratio,n_child", [(3, 12), (1, 4), (3, 11), (4, 9)])
def test_parent_steps_once_per_ratio_child_steps_and_one_step_ahead(ratio, n_child):
    pm, psim, cm, csim, journal = _pair(W_SHAPE, n_child, ratio=ratio)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=ratio)
    run(csim)
    n_parent = -(-n_child // ratio)
    steps = [e for e in journal if e[1] == "run_steps"]
    assert [e[2] for e in steps if e[0] == "parent"] == [1] * n_parent and f.parent_steps == n_parent
    assert sum(e[2] for e in steps if e[0] == "child") == n_child and max(e[2] for e in steps if e[0] == "child") <= ratio
    assert [e[2] for e in journal if e[1] == "nest_sample"] == list(range(1, n_parent + 2)) and f.uploads == n_parent + 1
    # every parent step is followed by its sample before anybody steps again, and the parent is one step ahead: when a child chunk
    # is enqueued at clock t the parent's clock is the level behind t
    pclock = 0.0
    for k, e in enumerate(journal):
        if e[0] == "parent" and e[1] == "run_steps":
            assert journal[k + 1][:2] == ("child", "nest_sample") and journal[k + 1][3] == e[3]
            pclock = e[3]
        if e[0] == "child" and e[1] == "run_steps":
            start = e[3] - e[2] * csim.Δt
            assert pclock - psim.Δt - 1e-6 <= start and e[3] <= pclock + 1e-6, (e, pclock)
    assert pm.clock.iteration == n_parent and cm.clock.iteration == n_child
    log = cm.backend.log
    assert [e[0] for e in log if e[0] in ("seed", "bforce_init", "nest_init")] == ["seed", "bforce_init", "nest_init"]
    assert [e[0] for e in log][-2:] == ["nest_free", "bforce_free"]
    assert len(f.times) == n_parent + 2 and np.array_equal(f.times[:-1], 600.0 * np.arange(n_parent + 1))


def test_the_parents_writers_are_driven_one_step_per_chunk(tmp_path):
    from test_station_output_host import ProbeBackend

    class B(NestBackend, ProbeBackend):
        def run_steps(self, dt, n):
            before = self.clock
            self._stepped(dt, n)                 # the probe ring's samples
            self.clock = before
            NestBackend.run_steps(self, dt, n)   # the window check, the clock, the journal

    pm, psim, cm, csim, journal = _pair(K_SHAPE, 12, backend=B)
    sw = psim.output_writers["stations"] = StationWriter(pm, points=rim_points(cm, side="west"), path=tmp_path, format="npy")
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="west", ratio=3)
    run(csim)
    assert sw.iterations == [0, 1, 2, 3, 4] and sw.store is None          # every parent step recorded, the file closed


def test_per_step_paths_and_restarts_are_refused(tmp_path):
    pm, psim, cm, csim, _ = _pair(K_SHAPE, 6)
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
    with pytest.raises(NotImplementedError, match="picked up"):
        run(csim, pickup=str(tmp_path / "nothing.ckpt"))
    with pytest.raises(NotImplementedError, match="chunked path"):
        run(csim, cash_store=True)
    csim.output_writers["checkpointer"] = Checkpointer(cm, schedule=2, dir=tmp_path, prefix="c")
    with pytest.raises(NotImplementedError, match="Checkpointer"):
        run(csim)
    del csim.output_writers["checkpointer"]
    psim.output_writers["checkpointer"] = Checkpointer(pm, schedule=2, dir=tmp_path, prefix="p")
    with pytest.raises(NotImplementedError, match="Checkpointer"):
        run(csim)
    del psim.output_writers["checkpointer"]
    pm._winds_static = False
    with pytest.raises(NotImplementedError, match="static winds"):
        run(csim)
    assert not [e for e in cm.backend.log + pm.backend.log if e[0] == "seed"]        # nothing was seeded by any of them


# ---- the offline route's reader ----
def test_from_station_output_round_trip(tmp_path):
    cm = models.WaveGrowth2D(**child_cfg(K_SHAPE).model, backend_factory=NestBackend)
    pts = rim_points(cm, side="west")
    n, nt = len(pts), 4
    rng = np.random.default_rng(3)
    rec = rng.uniform(0.1, 2.0, (nt, n, len(VAR_NAMES)))
    rec[2, 5, :] = np.nan                         # a station without a wet corner
    st = NpyStationStore(tmp_path, "stations", nt + 1, [p[0] for p in pts], [p[1] for p in pts], [f"s{k}" for k in range(n)])
    for k in range(nt):
        st.write(k, rec[k], 600.0 * k, k)
    st.close()                                    # (the last record was never written: a shorter run)
    f = from_station_output(cm, tmp_path, side="west")
    assert isinstance(f, BoundaryForcing) and np.array_equal(f.times, 600.0 * np.arange(nt))
    assert np.array_equal(f.nodes, np.array(rim_nodes(cm.grid, "west")))
    assert np.array_equal(f.values, rec[:, :, :3], equal_nan=True) and np.isnan(f.values[2, 5]).all() and np.isnan(f.values).sum() == 3
    with pytest.raises(ValueError, match="forced nodes in order"):
        from_station_output(cm, tmp_path, side="east")
    with pytest.raises(ValueError, match="either nodes"):
        from_station_output(cm, tmp_path)


# ---- the mix arithmetic ----
def _mix_scalar(corner, index, weight):
    """k_nest_mix, lane by lane, in Python floats (IEEE doubles, one rounding per operation)"""
    n = len(index)
    out = np.empty((n, 3))
    for p in range(n):
        W = SE = SX = SY = 0.0
        for c in range(4):
            e, mx, my = (float(v) for v in corner[:, index[p][c]])
            w = float(weight[p][c])
            if math.isfinite(e) and math.isfinite(mx) and math.isfinite(my) and e > 0.0 and mx * mx + my * my > 0.0:
                W = W + w
                SE = SE + w * e
                SX = SX + w * mx
                SY = SY + w * my
        if W > 0.0:
            E, MX, MY = SE / W, SX / W, SY / W
            ok = MX * MX + MY * MY > 0.0
        else:
            ok = False
        out[p] = (E, MX, MY) if ok else (math.nan,) * 3
    return out


def test_mix_arithmetic_on_hostile_corners():
    rng = np.random.default_rng(11)
    nc, n = 40, 300
    corner = np.stack([np.exp(rng.uniform(-6, 2, nc)), rng.normal(0, 0.05, nc), rng.normal(0, 0.05, nc)])
    corner[:, 0] = (np.nan, 0.1, 0.1)
    corner[:, 1] = (1.0, np.inf, 0.1)
    corner[:, 2] = (0.0, 0.1, 0.1)
    corner[:, 3] = (1.0, 0.0, 0.0)
    corner[:, 4] = (-1.0, 0.1, 0.1)
    corner[:, 5] = (1.0, 0.1, -np.inf)
    corner[:, 6] = (1e-300, 1e-170, 1e-170)       # m² underflows to zero: dry
    index = rng.integers(0, nc, (n, 4))
    index[:8] = rng.integers(0, 7, (8, 4))        # all dry
    weight = rng.uniform(0.0, 1.0, (n, 4))
    weight[8:16, 1:] = 0.0                        # one corner carries everything
    weight[16:20] = 0.0                           # W = 0 with wet corners
    got = _mix_scalar(corner, index, weight)
    want = station_records(corner[None], index, weight, 9.81, 0.85)[0, :, :3]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)])
    assert np.isnan(got[:8]).all() and np.isnan(got[16:20]).all() and 8 < np.isnan(got[:, 0]).sum() < n // 2
