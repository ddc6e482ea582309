"""The fused step after its RK loop stopped waiting at the loads (the exponential's table read leaves early and is
consumed late, the tableau's address is pc-relative, the constants of a plain RHS evaluation are asked for ahead of the reciprocal
square root).  No fp64 operation, operand order or rounding changed, so everything here is bitwise against oracle B.

64 x 4 (one workgroup) and 128 x 8 are the smallest grids that still launch k_step_waverow; three fused steps — the first is the
stand-alone advance (nothing to scatter yet), the second and third are fused launches — and then an observer, whose flush writes the
State.  All six flavours of the fused kernel (DP5, Tsit5, the default solver; static and time-varying winds) under
PICLES_WAVEROW=require (k_step_waverow) and PICLES_WAVEROW=0 (k_step).  Oracle B runs once per case and is shared by both."""
from types import SimpleNamespace

import numpy as np
import pytest

from picles_amd import configs
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.timesteppers import time_step
from picles_amd.wind_emulator import wind_interpolator
from helpers import assert_bitwise, make_model
from test_gpu_waverow import DX, _box

pytestmark = pytest.mark.gpu
STEPS = 3
SHAPES = [(64, 4), (128, 8)]
_REF = {}


def _two_level(nx, ny, solver):
    """winds that turn and freshen linearly in time, carried as a device lattice with one time knot per model step: no knot falls
    inside a step, every window has two levels (the straight line) — the time-varying flavours of the fused kernel"""
    c = _box(nx, ny, solver=solver)
    s = configs.smooth_winds(10.0, 10.0, DX * (nx - 1), DX * (ny - 1))
    T = (STEPS + 3) * c.Δt

    def u(x, y, t):
        return s.u(x, y, t) * (1.0 + 0.3 * t / T)

    def v(x, y, t):
        return s.v(x, y, t) * (1.0 - 0.4 * t / T)
    g = c.model["grid"]
    x, y, t = g.data.x[:, 0], g.data.y[0, :], np.arange(0.0, T + 0.5 * c.Δt, c.Δt)
    X, Y, TT = np.meshgrid(x, y, t, indexing="ij")
    w = wind_interpolator(dict(x=x, y=y, t=t, u=u(X, Y, TT), v=v(X, Y, TT)))
    c.model["winds"] = w
    c.model["ODEsys"].u, c.model["ODEsys"].v = w.u, w.v
    c.model["winds_static"] = False
    return c


def _cfg(shape, solver, wind):
    if wind == "two_level":
        return _two_level(*shape, solver)
    U10, V10 = wind
    return _box(*shape, solver=solver, U10=U10, V10=V10)


def _snapshot(m):
    z, on, bnd, st = m.backend.get_particles()
    c = m.backend.get_counters()
    return dict(State=np.array(m.State, copy=True), z=z, on=on, bnd=bnd, st=st,
                counters={k: c[k] for k in ("rhs_evals", "steps_accepted", "steps_rejected", "reseeds", "clamps", "particles_advanced", "max_reach")})


def _run(make, backend, prepare=None, watch=None):
    cfg = make()
    m = make_model(cfg, backend)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    if prepare is not None:
        prepare(m)
    seen = []
    if backend == "hip":
        m.backend.enable_timing(True)
    for _ in range(STEPS):
        time_step(m, cfg.Δt, zero_first=True)
        if watch is not None:
            seen.append(watch(m))
    if backend == "hip" and watch is None:      # nobody looked in between: every step was a fused launch, one flush at the end
        t = m.backend.get_timing()
        assert t["advance_launches"] == STEPS and t["scatter_launches"] <= 1, t
    out = _snapshot(m)
    out["seen"] = seen
    return out


def _reference(key, make, prepare=None, watch=None):
    """oracle B's run of a case: computed once, shared by the two kernels, never written to"""
    if key not in _REF:
        _REF[key] = _run(make, ("pmath", 1), prepare, watch)
        for a in _REF[key].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[key]


def _hold(got, ref, what):
    assert_bitwise(got["State"], ref["State"], f"{what}: State after {STEPS} fused steps")
    assert_bitwise(got["on"], ref["on"], f"{what}: on flags")
    assert_bitwise(got["bnd"], ref["bnd"], f"{what}: boundary flags")
    assert_bitwise(got["st"], ref["st"], f"{what}: status")
    live = ((ref["st"] & 1) == 1) & (ref["on"] == 1)        # the state vector of a switched-off particle is dead storage
    for c in range(5):
        assert_bitwise(got["z"][..., c][live], ref["z"][..., c][live], f"{what}: particle z[{c}]")
    assert got["counters"] == ref["counters"], (what, got["counters"], ref["counters"])
    assert ref["counters"]["particles_advanced"] > 0 and ref["counters"]["rhs_evals"] > 0


@pytest.mark.parametrize("mode", ["require", "0"], ids=["waverow", "k_step"])
@pytest.mark.parametrize("wind", [(10.0, 10.0), (10.0, 3.0), "two_level"], ids=["winds_10_10", "winds_10_3", "two_level_window"])
@pytest.mark.parametrize("solver", ["DP5", "Tsit5", "AutoTsit5"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_flavour_against_the_oracle(shape, solver, wind, mode, monkeypatch):
    monkeypatch.setenv("PICLES_WAVEROW", mode)
    make = lambda: _cfg(shape, solver, wind)      # noqa: E731
    _hold(_run(make, "hip"), _reference((shape, solver, wind), make), f"{shape} {solver} {wind} PICLES_WAVEROW={mode}")


# ---- the early table read meets the rare side of the exponential in one wave -------------------------------------------------------
# rhs3 evaluates exp(2 ln e) behind a wave-uniform range test (pm_exp_sat: |2 ln e| <= 700 in every lane, or the clamps first).  A
# band of eight columns carries e = exp(-352): its lanes are on the rare side, the other lanes of the same wave are plain.  A
# fused step re-meshes its particles from the node values of the step before, so the band has to survive a scatter: the remesh
# thresholds are lowered to nothing (an energy of 1e-153 stays a particle), the model step is one minute (a particle moves 0.15
# cells) and only the band's downwind edge takes energy from plain neighbours — one column per step, five are left at the third.
BAND = slice(40, 48)
LNE_RARE = -352.0


def _rare_cfg():
    c = _box(128, 8, dt=60.0)
    c.model["minimal_state"] = [0.0, 0.0]
    return c


def _rare_prepare(m):
    z, on, _, _ = m.backend.get_particles()
    z = z.copy()
    z[BAND, :, 0] = LNE_RARE
    m.backend.set_particles(z, on)


def _rare_watch(m):
    z, on, _, st = m.backend.get_particles()
    return z[..., 0].copy(), (on == 1) & ((st & 1) == 1)


@pytest.mark.parametrize("mode", ["require", "0"], ids=["waverow", "k_step"])
def test_rare_side_of_the_exponential_in_some_lanes_of_a_wave(mode, monkeypatch):
    monkeypatch.setenv("PICLES_WAVEROW", mode)
    ref = _reference("rare", _rare_cfg, _rare_prepare, _rare_watch)
    for k, (lne, live) in enumerate(ref["seen"][:STEPS - 1]):      # what the fused launches of steps 2 and 3 start from
        rare = live & (np.abs(2.0 * lne) > 700.0)
        plain = live & (np.abs(2.0 * lne) < 100.0)
        for j in range(lne.shape[1]):          # every row holds both kinds in the band's column block (one wave)
            assert rare[0:64, j].sum() >= 3 and plain[0:64, j].sum() >= 32, (k, j, int(rare[:, j].sum()), int(plain[:, j].sum()))
    _hold(_run(_rare_cfg, "hip", _rare_prepare), ref, f"rare exponential PICLES_WAVEROW={mode}")


# ---- particles that are not plain: y = 1/|c̄| above ymax = 10/r_g ------------------------------------------------------------------------
# (the guarded forms of rhs3 keep their own loads behind the wave-uniform test; the other lanes of the wave are plain.)  Same
# construction: in a band of eight columns the wind is a tenth of its neighbours' (1.4 m/s) and the particles are the slow, faint
# ones such a wind seeds, |c̄| = 0.009 m/s against the floor r_g/10 = 0.085; they stay what they are from step to step.
SLOW = [-16.5, 0.0065, 0.006, 0.0, 0.0]


def _slow_cfg():
    nx, ny = 128, 8
    s = configs.smooth_winds(10.0, 10.0, DX * (nx - 1), DX * (ny - 1))

    def band(x):
        return np.where((x >= DX * BAND.start) & (x < DX * BAND.stop), 0.1, 1.0)
    c = _box(nx, ny, winds=SimpleNamespace(u=lambda x, y, t: s.u(x, y, t) * band(x), v=lambda x, y, t: s.v(x, y, t) * band(x)), dt=60.0)
    c.model["minimal_state"] = [0.0, 0.0]
    return c


def _slow_prepare(m):
    z, on, _, _ = m.backend.get_particles()
    z, on = z.copy(), on.copy()
    z[BAND, :, :] = SLOW
    on[BAND, :] = 1
    m.backend.set_particles(z, on)


def _slow_watch(m):
    z, on, _, st = m.backend.get_particles()
    return np.hypot(z[..., 1], z[..., 2]), (on == 1) & ((st & 1) == 1)


@pytest.mark.parametrize("mode", ["require", "0"], ids=["waverow", "k_step"])
def test_particles_that_are_not_plain(mode, monkeypatch):
    monkeypatch.setenv("PICLES_WAVEROW", mode)
    ref = _reference("slow", _slow_cfg, _slow_prepare, _slow_watch)
    assert np.isfinite(ref["State"]).all()
    for k, (c, live) in enumerate(ref["seen"][:STEPS - 1]):
        slow = live & (c < 0.5 * 0.085)
        plain = live & (c > 2.0 * 0.085)
        for j in range(c.shape[1]):
            assert slow[0:64, j].sum() >= 3 and plain[0:64, j].sum() >= 32, (k, j, int(slow[:, j].sum()), int(plain[:, j].sum()))
    _hold(_run(_slow_cfg, "hip", _slow_prepare), ref, f"non-plain particles PICLES_WAVEROW={mode}")
