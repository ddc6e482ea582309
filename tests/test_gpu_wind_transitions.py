"""The wind window changes form at every model step: 12 steps on a fixed schedule that takes it through every ordered pair of
neighbouring forms — static, two levels, parabola, knot, polyline and back, from levels the caller uploads — and then over to a
lattice the device samples itself, whose 900-second knots put none, one and two of them into the last three steps (600, 600 and 2000
seconds long: a two-level window from a stand-alone advance, a knot window that a fused launch follows by rotating the level planes,
a polyline through the plain phases that reuses the level the step before left behind).  The oracle is driven through the same
schedule with host-sampled levels (the NumPy interpolant of tests/test_wind_grid.py, models.gridded_wind_window); State and the
particles are compared bit for bit where the host-level walk ends and at the end of the run, with nobody looking in between.

Shapes: 64 x 8, whose fused launches qualify for the wave-per-row kernel (run with PICLES_WAVEROW unset and =require, DP5 and the
auto-switching solver), and 24 x 10, whose launches do not."""
import functools

import numpy as np
import pytest

from picles_amd import _capi as K
from picles_amd.models import apply_wind_window, gridded_wind_window
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.wind_emulator import wind_interpolator
from helpers import assert_bitwise, make_model
from test_gpu_fullsize import _same_particles
from test_gpu_waverow import _box
from test_wind_grid import _lattice

DT = 600.0
# (source, form, step length); the host walk visits S T P K L K P T S: every ordered pair of neighbours among the five forms
SCHEDULE = [("host", f, DT) for f in ("static", "two", "parabola", "knot", "polyline", "knot", "parabola", "two", "static")] + \
           [("lattice", 0, DT), ("lattice", 1, DT), ("lattice", 2, 2000.0)]
HOST_END = 9


def _models(nx, ny, solver, backend):
    w = wind_interpolator(_lattice()[0])
    cfg = _box(nx, ny, solver=solver, winds=w)
    cfg.model["winds_static"] = False
    cfg.model["ODEsys"].u, cfg.model["ODEsys"].v = w.u, w.v
    m = make_model(cfg, backend)
    initialize_simulation(Simulation(m, Δt=DT, stop_time=1.0))      # seeds under the lattice's level at t = 0
    return m, w


def _walk(m, w, device_lattice):
    """the schedule on one model's backend; yields after the host walk and at the end"""
    b, grid = m.backend, m.grid
    X, Y = grid.data.x, grid.data.y
    lv = lambda t: (w.u(X, Y, t), w.v(X, Y, t))
    t, on_lattice = 0.0, device_lattice
    for k, (src, form, dt) in enumerate(SCHEDULE, 1):
        if src == "host":
            on_lattice = False
            (u0, v0), (u1, v1) = lv(t), lv(t + dt)
            if form == "static":
                b.set_winds(u0, v0, t)
            elif form == "two":
                b.set_winds(u0, v0, t, u1, v1, t + dt)
            elif form == "parabola":
                um, vm = lv(t + 0.5 * dt)
                b.set_winds(u0, v0, t, u1, v1, t + dt, um=um, vm=vm)
            elif form == "knot":
                um, vm = lv(t + 0.375 * dt)
                b.set_winds(u0, v0, t, u1, v1, t + dt, um=um, vm=vm, tk=t + 0.375 * dt)
            else:      # the most a window carries: PICLES_MAX_KNOTS knots, unevenly spaced
                times = [t + dt * (j * j) / 81.0 for j in range(10)]
                b.set_winds_polyline([lv(x)[0] for x in times], [lv(x)[1] for x in times], times)
        elif device_lattice:
            if not on_lattice:
                b.set_wind_grid(w.lattice(), float(X[0, 0]), float(Y[0, 0]), time_mode="linear")
                on_lattice = True
        else:
            win = gridded_wind_window(w, grid, t, dt)
            tk = win[-1]
            assert (0 if tk is None else len(tk) if isinstance(tk, list) else 1) == form, (k, tk)
            apply_wind_window(b, t, dt, *win)
        b.time_step(dt, K.STEP_ZERO_FIRST)
        t += dt
        if k in (HOST_END, len(SCHEDULE)):
            yield k


@functools.lru_cache(maxsize=None)
def _oracle(nx, ny, solver):
    """the oracle's run, once per shape and solver: the model (for the particles and counters at the end) and State at both stops"""
    o, w = _models(nx, ny, solver, ("pmath", 1))
    states = {k: np.array(o.backend.get_state()) for k in _walk(o, w, False)}
    return o, states


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,solver,waverow", [(64, 8, "DP5", None), (64, 8, "DP5", "require"), (64, 8, "AutoTsit5", None),
                                                  (64, 8, "AutoTsit5", "require"), (24, 10, "DP5", None)])
def test_every_transition_between_window_forms_matches_the_oracle(nx, ny, solver, waverow, monkeypatch):
    if waverow is None:
        monkeypatch.delenv("PICLES_WAVEROW", raising=False)
    else:
        monkeypatch.setenv("PICLES_WAVEROW", waverow)
    o, states = _oracle(nx, ny, solver)
    g, w = _models(nx, ny, solver, "hip")
    for k in _walk(g, w, True):
        s = g.backend.get_state()
        assert np.abs(s).max() > 0
        assert_bitwise(s, states[k], f"State after step {k}")
    _same_particles(g, o)
