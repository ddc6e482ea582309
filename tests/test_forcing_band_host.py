"""Forcing bands on the CPU box (picles_amd/boundary_forcing.py, nesting.py): the band geometry and its order, the
"linear" ramp, which of bforce_init / bforce_init_band a forcing takes over backends that record their calls, the refusals before a
run, and the blend restated in scalar arithmetic."""
import struct

import numpy as np
import pytest

from picles_amd import configs, models
from picles_amd.boundary_forcing import SIDES, BoundaryForcing, band_nodes, blend, linear_weights, rim_nodes, side_distance
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import rim_points
from picles_amd.simulations import Simulation, run
from test_boundary_forcing_host import ForcingBackend, _values


class BandBackend(ForcingBackend):
    """ForcingBackend + the band entry point, recorded"""

    def bforce_init_band(self, nodes, weights=None):
        assert self.bf is None, "second bforce_init without bforce_free"
        self.bf = dict(nodes=np.asarray(nodes), levels=None, weights=None if weights is None else np.array(weights))
        self.log.append(("bforce_init_band", len(nodes), weights is not None))


def _sim(n_steps, shape=(12, 12), backend=BandBackend, mask=None):
    cfg = configs.bench06_box(n=16, periodic_grid=False)
    nx, ny = shape
    cfg.model["grid"] = TwoDCartesianGridMesh(2000.0 * (nx - 1), nx, 2000.0 * (ny - 1), ny, mask=mask, periodic_boundary=(False, False))
    m = models.WaveGrowth2D(**cfg.model, backend_factory=backend)
    return m, Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1)), cfg.Δt


def _old_rim_nodes(Nx, Ny, side):
    """the lists rim_nodes gave before it had a width"""
    return {"west": [(0, j) for j in range(Ny)], "east": [(Nx - 1, j) for j in range(Ny)], "south": [(i, 0) for i in range(Nx)],
            "north": [(i, Ny - 1) for i in range(Nx)],
            "rim": [(i, j) for j in range(Ny) for i in range(Nx) if i in (0, Nx - 1) or j in (0, Ny - 1)]}[side]


def test_width_one_is_the_list_of_old_for_every_side():
    m, _, _ = _sim(3, shape=(7, 5))
    for side in SIDES:
        assert rim_nodes(m.grid, side) == rim_nodes(m.grid, side, 1) == rim_nodes(m.grid, side, width=1) == _old_rim_nodes(7, 5, side)
        assert band_nodes(m.grid, side, 1)[0] == sorted(_old_rim_nodes(7, 5, side), key=lambda n: (n[1], n[0]))
        assert rim_points(m, side) == rim_points(m, side=side) == rim_points(m, side, width=1)
    with pytest.raises(ValueError, match="side must be"):
        rim_nodes(m.grid, "up", 2)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="width must be an integer >= 1"):
            rim_nodes(m.grid, "rim", bad)


def test_band_geometry_and_order_with_land_in_the_band():
    nx, ny = 9, 8
    mask = np.ones((nx, ny), dtype=bool)
    mask[1:4, 2:5] = False                                       # a land block inside a three-deep west band: its centre class 0, coast around
    m, _, _ = _sim(3, shape=(nx, ny), mask=mask)
    total = np.asarray(m.grid.data.mask)
    assert total[2, 3] == 0 and total[1, 2] == 2 and (np.isin(total[1:4, 2:5], (0, 2))).all() and total[0, 3] == 3
    west, d = band_nodes(m.grid, "west", 3)
    want = [(i, j) for j in range(ny) for i in range(3) if total[i, j] in (1, 3)]
    assert west == want == rim_nodes(m.grid, "west", 3)          # rows in order, i fastest; land (0) and coast (2) skipped
    assert not any(total[i, j] in (0, 2) for i, j in west) and len(west) < 3 * ny
    assert d.tolist() == [i for i, _ in west]
    rim, dr = band_nodes(m.grid, "rim", 2)
    assert rim == [(i, j) for j in range(ny) for i in range(nx) if min(i, nx - 1 - i, j, ny - 1 - j) < 2 and total[i, j] in (1, 3)]
    assert dr.tolist() == [min(i, nx - 1 - i, j, ny - 1 - j) for i, j in rim]
    assert side_distance(m.grid, "north")[4].tolist() == list(range(ny - 1, -1, -1))
    east, de = band_nodes(m.grid, "east", 2)
    assert east == [(i, j) for j in range(ny) for i in (nx - 2, nx - 1)] and de.tolist() == [1, 0] * ny
    # a band wider than the box is the whole box
    assert len(band_nodes(m.grid, "rim", 50)[0]) == int(np.isin(total, (1, 3)).sum())
    pts = rim_points(m, "west", width=3)
    x, y = np.asarray(m.grid.data.x), np.asarray(m.grid.data.y)
    assert pts == [(float(x[i, j]), float(y[i, j])) for i, j in west]


def test_linear_ramp():
    m, _, _ = _sim(3, shape=(12, 10))
    for width in (1, 2, 3, 4):
        f = BoundaryForcing(m, side="rim", width=width, weights="linear", times=[0.0], values=lambda t: None)
        nodes, d = band_nodes(m.grid, "rim", width)
        assert np.array_equal(f.nodes, np.asarray(nodes))
        want = np.array([(width - int(k)) / width for k in d])
        assert np.array_equal(f.node_weights, want) and np.array_equal(linear_weights(d, width), want)
        assert f.node_weights.max() == 1.0 and f.node_weights.min() == 1.0 / width and f.band
        assert (f.node_weights[np.asarray(d) == 0] == 1.0).all()
    with pytest.raises(ValueError, match="weights must be None"):
        BoundaryForcing(m, side="rim", width=3, weights="cosine", times=[0.0], values=lambda t: None)
    with pytest.raises(ValueError, match="weights must be None"):
        BoundaryForcing(m, nodes=[(0, 1), (1, 1)], weights="linear", times=[0.0], values=lambda t: None)
    with pytest.raises(ValueError, match="width= goes with side="):
        BoundaryForcing(m, nodes=[(0, 1), (1, 1)], width=2, times=[0.0], values=lambda t: None)
    with pytest.raises(ValueError, match="3 weights for 2 nodes"):
        BoundaryForcing(m, nodes=[(0, 1), (1, 1)], weights=[1.0, 0.5, 0.5], times=[0.0], values=lambda t: None)
    for bad in (0.0, 1.5, float("nan"), -0.1):
        with pytest.raises(ValueError, match="finite and in \\(0, 1\\]"):
            BoundaryForcing(m, nodes=[(0, 1), (1, 1)], weights=[1.0, bad], times=[0.0], values=lambda t: None)


def _inits(m):
    return [e for e in m.backend.log if e[0].startswith("bforce_init")]


def test_which_entry_point_a_forcing_takes():
    times = [0.0, 7200.0]
    # width 1 on the rim: bforce_init, as ever — also over a backend that has nothing else
    for backend in (ForcingBackend, BandBackend):
        m, sim, dt = _sim(4, backend=backend)
        f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="rim", times=times, values=_values(times, 44), Δt=dt)
        assert not f.band and f.node_weights is None
        run(sim)
        assert _inits(m) == [("bforce_init", 44)]
    # a band by width, by an ocean node among nodes=, and by weights
    m, sim, dt = _sim(4)
    n = len(rim_nodes(m.grid, "rim", 3))
    assert n == 144 - 36
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="rim", width=3, times=times, values=_values(times, n), Δt=dt)
    assert f.band
    run(sim)
    assert _inits(m) == [("bforce_init_band", n, False)] and m.backend.log[-1] == ("bforce_free",)
    m, sim, dt = _sim(4)
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, nodes=[(0, 3), (1, 3), (2, 3)], times=times, values=_values(times, 3), Δt=dt)
    assert f.band
    run(sim)
    assert _inits(m) == [("bforce_init_band", 3, False)]
    m, sim, dt = _sim(4)
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", width=2, weights="linear", times=times,
                                                                 values=_values(times, 24), Δt=dt)
    run(sim)
    assert _inits(m) == [("bforce_init_band", 24, True)]
    m, sim, dt = _sim(4)
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", weights=np.full(12, 0.5), times=times,
                                                                 values=_values(times, 12), Δt=dt)
    run(sim)
    assert _inits(m) == [("bforce_init_band", 12, True)]


def test_check_run_refuses_a_band_over_a_backend_without_the_entry_point():
    times = [0.0, 7200.0]
    for kw, n in ((dict(side="rim", width=2), 144 - 64), (dict(nodes=[(0, 3), (1, 3)]), 2), (dict(side="west", weights=np.full(12, 0.5)), 12)):
        m, sim, dt = _sim(4, backend=ForcingBackend)
        sim.output_writers["boundary_forcing"] = BoundaryForcing(m, times=times, values=_values(times, n), Δt=dt, **kw)
        with pytest.raises(NotImplementedError, match="needs a backend with bforce_init_band"):
            run(sim)
        assert not _inits(m) and not any(e[0] == "run_steps" for e in m.backend.log)          # refused before anything ran


def _bits(x):
    return struct.pack("<d", float(x))


def test_blend_is_three_rounded_operations():
    """v = m + w (p - m): the difference, the product and the sum each round once — Python floats do exactly that"""
    rng = np.random.default_rng(3)
    m = rng.uniform(0.0, 3.0, (200, 3))
    p = rng.uniform(0.0, 3.0, (200, 3))
    w = rng.choice([1.0 / 3.0, 2.0 / 3.0, 0.5, 0.1, 1.0], 200)
    v = blend(m, p, w[:, None])
    for k in range(200):
        for c in range(3):
            mk, pk, wk = float(m[k, c]), float(p[k, c]), float(w[k])
            diff = pk - mk
            prod = wk * diff
            assert _bits(v[k, c]) == _bits(mk + prod)
    # the arithmetic does not return p at w = 1 in general (m + (p - m) rounds twice) — which is why a lane with w == 1.0 skips it
    assert (blend(m, p, 1.0) != p).any()
    m1, p1 = np.float64(0.1), np.float64(0.7)
    assert blend(0.0, p1, 1.0) == p1 and blend(m1, m1, 0.25) == m1
    # a hostile prescribed value stays hostile under any weight, and a hostile State poisons the blend: the birth test sees both
    assert np.isnan(blend(1.0, np.nan, 0.5)) and np.isnan(blend(np.nan, 1.0, 0.5)) and np.isinf(blend(1.0, np.inf, 1.0 / 3.0))
