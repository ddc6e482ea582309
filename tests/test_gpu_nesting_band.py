"""Nests with a forcing band on the GPU (NestForcing(width=), picles_bforce_init_band): a band as deep as the swell
travels in a step closes the hole a one-node rim leaves — the coincident child outside its band IS the parent — and the device
route of a banded nest equals the offline route through a station file, bit for bit.

The coincident nest is that of tests/test_gpu_nesting.py (_coincident), restated here with a width."""
import numpy as np
import pytest

from picles_amd.boundary_forcing import BoundaryForcing, from_station_output, rim_nodes
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import NestForcing, rim_points
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import StationWriter
from helpers import make_model
from test_gpu_boundary_forcing import _assert_same_model, _box, _everything
from test_nesting_host import C_DX, K_SHAPE, child_cfg, parent_cfg

pytestmark = pytest.mark.gpu

COINCIDENT_PARENT = (128, 16)
COL0, ROW0 = 8, 2
CBAR, DT, THETA, N_STEPS = 8.0, 600.0, 0.15, 10          # 2.4 cells a step


def _coincident(width):
    """Calm 128 x 16 box, every source term off, swell at 8 m/s and 0.15 rad through the west column; the child is the parent's own
    sub-box on rows 2..10 and columns 8..77, same dx, same Δt = 600 s, ratio 1, ten steps.  Returns (e_child, e_parent) over the
    child's columns 3..66 and rows 3..5 — outside a three-deep band — and max e_parent there"""
    nx, ny = COINCIDENT_PARENT
    pm = make_model(_box(COINCIDENT_PARENT, calm=True), "hip")
    psim = Simulation(pm, Δt=DT, stop_time=(N_STEPS - 1) * DT)
    e = 1.0
    v = np.tile(np.array([e, e / (2.0 * CBAR) * np.cos(THETA), e / (2.0 * CBAR) * np.sin(THETA)]), (ny, 1))
    psim.output_writers["boundary_forcing"] = BoundaryForcing(pm, side="west", times=[0.0], values=v[None])
    cfg = _box(K_SHAPE, calm=True)
    cfg.model["grid"] = TwoDCartesianGridMesh(COL0 * C_DX, (COL0 + 69) * C_DX, 70, ROW0 * C_DX, (ROW0 + 8) * C_DX, 9, periodic_boundary=(False, False))
    cm = make_model(cfg, "hip")
    csim = Simulation(cm, Δt=DT, stop_time=(N_STEPS - 1) * DT)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=1, width=width)
    assert len(f.nodes) == len(rim_nodes(cm.grid, "rim", width)) and f.band == (width > 1)
    assert np.array_equal(f.corner_nodes[f.index[:, 0]], f.nodes + [COL0, ROW0])          # every node sits on a parent node, weight 1.0
    run(csim)
    assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps) == (N_STEPS,) * 3
    ec = cm.backend.get_state()[3:67, 3:6, 0]
    ep = pm.backend.get_state()[COL0 + 3:COL0 + 67, ROW0 + 3:ROW0 + 6, 0]
    return ec, ep, float(ep.max())


def test_a_band_as_deep_as_the_swell_travels_lets_it_enter():
    """Swell at 2.4 cells a step.  With width = 3 the expected difference is zero, to the bit: at ratio 1 every child step starts at
    a level (s = 0), every band particle is charge_to_particle of the parent's own State, with the sources off the controller
    memory does not show, and a particle from parent column 7 lands at child column 1.4 and touches band columns only.  Should the
    GPU show otherwise the bound is 1e-4, by the position-rounding argument of test_coincident_nest_deeper_into_the_child
    (tests/test_gpu_nesting.py).  The same child at width = 1 stays off by more than half of the parent's largest energy (the commit
    before bands measured 9.872e-01 over all non-rim nodes; over the nodes compared here it is 6.219e-01).
    Measured on an MI355X: width 3 off by 0.000e+00, all 192 nodes equal to the bit; max e_parent 4.230478e-01."""
    ec, ep, scale = _coincident(3)
    rel3 = float(np.abs(ec - ep).max()) / scale
    print(f"width 3: max e_parent {scale:.6e}; child off by {rel3:.3e}; bitwise equal nodes {int((ec == ep).sum())} of {ec.size}")
    ec1, ep1, scale1 = _coincident(1)
    rel1 = float(np.abs(ec1 - ep1).max()) / scale1
    print(f"width 1: max e_parent {scale1:.6e}; child off by {rel1:.3e}")
    assert scale > 0.1 and scale1 == scale                       # the swell has arrived, and the parent is the same parent
    assert rel3 <= 1e-4
    assert rel1 > 0.5


def _stations_parent(tmp, width):
    pm = make_model(parent_cfg(), "hip")
    psim = Simulation(pm, Δt=600.0, stop_time=3 * 600.0)         # four parent steps
    child_like = type("M", (), {"grid": child_cfg(K_SHAPE).model["grid"]})
    psim.output_writers["stations"] = StationWriter(pm, points=rim_points(child_like, "rim", width=width), path=tmp, format="npy")
    return pm, psim


def test_banded_nest_equals_the_offline_route(tmp_path_factory):
    """NestForcing(width=2) on (K) under winds, twelve child steps at ratio 3, against the parent alone with a StationWriter at
    rim_points(child, "rim", width=2) and then the child under from_station_output(..., width=2): State, particles and counters"""
    ratio, width = 3, 2
    dt, n = 600.0 / ratio, 4 * ratio
    dirA, dirB = tmp_path_factory.mktemp("nested"), tmp_path_factory.mktemp("offline")
    pm, psim = _stations_parent(dirA, width)
    cm = make_model(child_cfg(K_SHAPE), "hip")
    csim = Simulation(cm, Δt=dt, stop_time=dt * (n - 1))
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=ratio, width=width)
    cm.backend.enable_timing(True)
    run(csim)
    timing = cm.backend.get_timing()
    assert timing["advance_launches"] == n and timing["scatter_launches"] <= 1, timing
    assert (cm.clock.iteration, pm.clock.iteration) == (n, 4) and f.band
    A = _everything(cm)
    pm2, psim2 = _stations_parent(dirB, width)
    run(psim2)
    cm2 = make_model(child_cfg(K_SHAPE), "hip")
    csim2 = Simulation(cm2, Δt=dt, stop_time=dt * (n - 1))
    g = csim2.output_writers["boundary_forcing"] = from_station_output(cm2, dirB, side="rim", width=width)
    assert np.array_equal(g.nodes, f.nodes) and len(g.nodes) == 2 * 2 * 70 + 2 * 2 * 5
    run(csim2)
    _assert_same_model(A, _everything(cm2), "NestForcing(width=2) vs from_station_output(width=2)")
    S, on = A[0], A[2]
    assert not on[f.nodes[:, 0], f.nodes[:, 1]].any()            # the set went with the run: its particles are switched off
    assert (S[f.nodes[:, 0], f.nodes[:, 1], 0] > 0.0).any() and np.isfinite(S).all()
