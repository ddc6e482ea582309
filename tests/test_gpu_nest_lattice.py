"""Nests and chunked runs under a gridded wind that varies in time, on the GPU (picles_amd/nesting.py, picles_amd/simulations.py;
the device samples its own copy of the lattice every step: picles_set_wind_grid, k_wind_sample): a child run beside its parent under
a lattice equals, bit for bit, the child run afterwards from the parent's station file; a two-way nest under a lattice equals the host
route through the public API; run() on its chunked path equals the per-step loop, in the model and in every output file.

The boxes are those of tests/test_nesting_host.py — (P) 64 x 16 periodic at 6 km, (W) 128 x 12 and (K) 70 x 9 at 2 km — and (F) 70 x 21
of tests/test_gpu_nest_feedback.py; parent step 600 s, ratio 3.  The lattices are those of tests/test_nest_lattice_host.py:
L900 — a parent step holds one time knot or none, a child step likewise, 1800 s is a knot on a step boundary of both — and L250 —
every parent step holds two or three knots (a polyline window: plain phases, the step is not pending when it is sampled), a child
step one or none."""
import numpy as np
import pytest

from picles_amd.boundary_forcing import from_station_output, node_points, rim_nodes
from picles_amd.field_output import FieldWriter, read_field_output
from picles_amd.nesting import NestForcing, locate_in_parent, restrict_records, restriction_stencil, rim_points
from picles_amd.run_statistics import StatisticsWriter, read_statistics
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter, read_station_output
from picles_amd.track_output import TrackWriter, read_track_output
from helpers import assert_same_bits, make_model
from test_gpu_boundary_forcing import _assert_same_model, _everything
from test_gpu_nest_feedback import F_SHAPE, pn_cfg
from test_gpu_nesting import DEFAULT_SOLVER
from test_nest_lattice_host import lattice_winds, under
from test_nesting_host import K_SHAPE, LX, LY, W_SHAPE, child_cfg, parent_cfg

pytestmark = pytest.mark.gpu

DT = 600.0
_LATTICES = {}


def L(spacing):
    if spacing not in _LATTICES:
        _LATTICES[spacing] = lattice_winds(float(spacing))
    return _LATTICES[spacing]


def same_files(a, b, what):
    """two read_*_output dictionaries: every array equal, floats in bits"""
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype in (np.float32, np.float64):
            assert_same_bits(x, y, f"{what}: {k}")
        else:
            assert x.shape == y.shape and (x == y).all(), (what, k)


# ---- 1. the nested route against the offline route ----
def _parent_sim(tmp, shape, spacing, width):
    pm = make_model(under(parent_cfg(), L(spacing)), "hip")
    psim = Simulation(pm, Δt=DT, stop_time=3 * DT)           # run(psim): four steps
    child_like = type("M", (), {"grid": child_cfg(shape).model["grid"]})
    psim.output_writers["stations"] = StationWriter(pm, points=rim_points(child_like, side="rim", width=width), path=tmp, format="npy")
    psim.output_writers["fields"] = FieldWriter(pm, schedule=2, path=tmp, coarsen=(4, 4), format="npy")
    return pm, psim


def _child(shape, solver, spacing):
    cm = make_model(under(child_cfg(shape, solver), L(spacing)), "hip")
    return cm, Simulation(cm, Δt=DT / 3, stop_time=11 * DT / 3)


CASES = [(W_SHAPE, 900, "DP5", 1, None), (K_SHAPE, 900, DEFAULT_SOLVER, 1, None), (K_SHAPE, 250, "DP5", 1, None), (W_SHAPE, 900, "DP5", 3, "linear")]
IDS = ["W128x12-L900", "K70x9-L900-default-solver", "K70x9-L250", "W128x12-L900-width3-linear"]


@pytest.mark.parametrize("shape,spacing,solver,width,weights", CASES, ids=IDS)
def test_nested_route_equals_offline_route_under_a_lattice(shape, spacing, solver, width, weights, tmp_path):
    band = dict(width=width, weights=weights) if width > 1 else {}
    # A: NestForcing beside the parent
    dirA = tmp_path / "nested"
    pm, psim = _parent_sim(dirA, shape, spacing, width)
    cm, csim = _child(shape, solver, spacing)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3, **band)
    run(csim)
    assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps, f.uploads) == (12, 4, 4, 5) and cm.backend.clock == pm.backend.clock
    A, parentA = _everything(cm), _everything(pm)
    # B: the parent alone, then the child from its station file
    dirB = tmp_path / "offline"
    pm2, psim2 = _parent_sim(dirB, shape, spacing, width)
    run(psim2)
    cm2, csim2 = _child(shape, solver, spacing)
    csim2.output_writers["boundary_forcing"] = from_station_output(cm2, dirB, side="rim", **band)
    run(csim2)
    _assert_same_model(A, _everything(cm2), "the child: NestForcing vs from_station_output under a lattice")
    _assert_same_model(parentA, _everything(pm2), "the parent beside a child vs the parent alone under a lattice")
    same_files(read_station_output(dirA), read_station_output(dirB), "the parent's station file")
    same_files(read_field_output(dirA), read_field_output(dirB), "the parent's field file")
    assert read_station_output(dirA)["iteration"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    # the winds did vary, and the forcing did enter: the child alone differs in its interior
    u0, _, u1, _ = cm.backend.get_winds()
    assert not np.array_equal(u0, u1)
    cm3, csim3 = _child(shape, solver, spacing)
    run(csim3)
    S0 = cm3.backend.get_state()
    w = width
    assert not np.array_equal(A[0][w:-w, w:-w], S0[w:-w, w:-w])
    assert np.isfinite(A[0]).all()


# ---- 2. two-way under a lattice ----
def test_two_way_nest_under_a_lattice_equals_the_host_route():
    """the host route of tests/test_gpu_nest_feedback.py (get_state(child), restrict_records, bforce_set_levels on a band set of the
    parent), both models under the same lattice object"""
    dt, wind = DT / 3, L(900)

    def pair():
        return make_model(under(pn_cfg(), wind), "hip"), make_model(under(child_cfg(F_SHAPE), wind), "hip")

    # the device route
    pm, cm = pair()
    psim, csim = Simulation(pm, Δt=DT, stop_time=3 * DT), Simulation(cm, Δt=dt, stop_time=11 * dt)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3, width=2, feedback=True)
    run(csim)
    assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps, f.feedbacks) == (12, 4, 4, 5) and len(f.fb_nodes) == 57
    # the host route
    pm2, cm2 = pair()
    for mdl, step in ((cm2, dt), (pm2, DT)):
        initialize_simulation(Simulation(mdl, Δt=step, stop_time=1.0))
        mdl.upload_winds(mdl.clock.time, step)
    pb, cb = pm2.backend, cm2.backend
    nodes = np.asarray(rim_nodes(cm2.grid, "rim", 2))
    corner_nodes, cindex, cweights = locate_in_parent(pm2.grid, node_points(cm2.grid, nodes))
    fb, src, index, weight = restriction_stencil(pm2.grid, cm2.grid, 2)
    cb.bforce_init_band(nodes)
    cb.nest_init(pb, corner_nodes, cindex, cweights)
    cb.nest_sample()
    pb.bforce_init_band(fb)
    for _ in range(4):
        S = cb.get_state()
        pb.bforce_set_levels(pb.clock, restrict_records(S[src[:, 0], src[:, 1]], index, weight))
        pb.run_steps(DT, 1)
        cb.nest_sample()
        cb.run_steps(dt, 3)
    pb.bforce_free()
    cb.nest_free()
    cb.bforce_free()
    parentA = _everything(pm)
    _assert_same_model(parentA, _everything(pm2), "the parent: NestForcing(feedback=True) vs the host route under a lattice")
    _assert_same_model(_everything(cm), _everything(cm2), "the child: NestForcing(feedback=True) vs the host route under a lattice")
    # the feedback is seen: the parent alone differs at a fed node
    pm3 = make_model(under(pn_cfg(), wind), "hip")
    run(Simulation(pm3, Δt=DT, stop_time=3 * DT))
    i, j = f.fb_nodes[:, 0], f.fb_nodes[:, 1]
    assert not np.array_equal(pm3.backend.get_state()[i, j], parentA[0][i, j])
    assert np.isfinite(parentA[0]).all() and (parentA[0][i, j, 0] > 0.0).all()


# ---- 3. run() chunked against the per-step loop ----
def _with_writers(tmp, spacing):
    m = make_model(under(parent_cfg(), L(spacing)), "hip")
    sim = Simulation(m, Δt=DT, stop_time=7 * DT)             # eight steps
    pts = [(30000.0 + 17000.0 * k, 9000.0 + 11000.0 * (k % 7)) for k in range(9)]
    sim.output_writers["stations"] = StationWriter(m, points=pts, path=tmp, format="npy")
    sim.output_writers["fields"] = FieldWriter(m, schedule=2, path=tmp, coarsen=(4, 4), format="npy")
    sim.output_writers["statistics"] = StatisticsWriter(m, fields=("peak", "mean"), schedule=1, window=3, path=tmp, format="npy")
    times = [37.0 + 233.0 * k for k in range(20)]            # 20 events along a track that crosses the box, inside the eight steps
    track = [((5000.0 + 18500.0 * k) % LX, (3000.0 + 4100.0 * k) % LY) for k in range(20)]
    sim.output_writers["tracks"] = TrackWriter(m, times=times, points=track, path=tmp, format="npy")
    calls = dict(run_steps=0, time_step=0)
    b = m.backend
    for name in calls:
        def wrapped(*a, _f=getattr(b, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        setattr(b, name, wrapped)
    return m, sim, calls


@pytest.mark.parametrize("spacing", [900, 250], ids=["L900", "L250"])
def test_chunked_run_equals_the_per_step_loop_under_a_lattice(spacing, tmp_path):
    a, asim, acalls = _with_writers(tmp_path / "chunked", spacing)
    run(asim)
    b, bsim, bcalls = _with_writers(tmp_path / "per-step", spacing)
    run(bsim, cash_store=True)
    assert acalls["run_steps"] >= 1 and acalls["time_step"] == 0, acalls
    assert bcalls == dict(run_steps=0, time_step=8), bcalls
    assert a.clock.iteration == b.clock.iteration == 8 and a.backend.clock == b.backend.clock
    for x, y, name in zip(_everything(a)[:4], _everything(b)[:4], ("State", "z", "on", "status")):
        assert_same_bits(x, y, f"run(sim) vs run(sim, cash_store=True) under a lattice: {name}") if x.dtype == np.float64 else np.testing.assert_array_equal(x, y)
    for read in (read_station_output, read_field_output, read_statistics, read_track_output):
        same_files(read(tmp_path / "chunked"), read(tmp_path / "per-step"), read.__name__)
    assert read_station_output(tmp_path / "chunked")["iteration"].tolist() == [float(k) for k in range(9)]
    assert np.isfinite(np.asarray(read_track_output(tmp_path / "chunked")["data"])[:3]).any()
