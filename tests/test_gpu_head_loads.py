"""The head of k_step_waverow after its loads left the serial chain: the static four-wave flavours (DP5, Tsit5) fetch
u0, v0 and ln q_old straight into LDS when the wave's index is known and read them there behind the pull; every wave-per-row flavour
asks for the rows of the reach and class maps in one round trip at reach 1 and 2.  No fp64 operation, candidate order or summation
order changed, so everything is bitwise: against oracle B, and against the same run through k_step (PICLES_WAVEROW=0).  The runs under
test go through PICLES_WAVEROW=require, which hands every flavour to k_step_waverow — the two staged ones and the four whose text is
the old one (time-varying winds, the default solver), which share the map rows.

What a stage can get wrong and the bits would show: a lane reading another lane's value (the winds differ from node to node:
configs.smooth_winds), a wave reading another wave's (four rows per workgroup, their winds differ), a value read before it landed,
ln q_old not following the controller from step to step, the re-seed branch (it reads the planes through the global pointers), lanes
that are not stepped (their staged values are fetched and never read).

Grids: 64 x 4 and 128 x 8 hold only edge waves (every window wraps or leaves the grid: the per-lane pull); 192 x 12 is the smallest
with a wave whose windows lie inside (middle column block, rows 4 - 7: the written-out map rows).  192 x 24 where reach 2 needs
interior rows.  Six steps: the first is the stand-alone advance, five are fused launches.

The planes of a context are the library's own allocations (hipMalloc: 256-byte aligned) and the C ABI takes no plane pointer, so the
host's fall-back to k_step for a plane that is not 16-byte aligned (picles_hip.hip, launch_step_rows) cannot be reached from here."""
import numpy as np
import pytest

from picles_amd import configs
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.timesteppers import time_step
from helpers import assert_bitwise, make_model
from test_gpu_fullsize import _same_particles
from test_gpu_pull_class import _box as _class_box, _hip, _want, _winds
from test_gpu_waverow import _box, _calm_patch, _same, _snap

pytestmark = pytest.mark.gpu
STEPS = 6
_REF = {}


def _oracle(key, make, n_steps, event=None):
    """oracle B's run of a case, stepped as the models under test are: computed once, shared, never written to"""
    if key not in _REF:
        cfg = make()
        mo = make_model(cfg, ("pmath", 1))
        initialize_simulation(Simulation(mo, Δt=cfg.Δt, stop_time=1.0))
        for k in range(1, n_steps + 1):
            time_step(mo, cfg.Δt, zero_first=True)
            if event is not None:
                event(k, mo)
        _REF[key] = mo
    return _REF[key]


def _fused(make, mode, monkeypatch, n_steps, event=None):
    monkeypatch.setenv("PICLES_WAVEROW", mode)
    cfg = make()
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    mid = None
    for k in range(1, n_steps + 1):
        time_step(m, cfg.Δt, zero_first=True)
        if event is not None:
            event(k, m)
        if k == n_steps - 2:
            mid = _snap(m)
    return m, mid, _snap(m)


def _three_ways(key, make, monkeypatch, n_steps=STEPS, event=None, oracle=True):
    """k_step_waverow against k_step (two steps before the end and at the end) and against oracle B (at the end)"""
    mw, w_mid, w_end = _fused(make, "require", monkeypatch, n_steps, event)
    m0, o_mid, o_end = _fused(make, "0", monkeypatch, n_steps, event)
    _same(w_mid, o_mid, f"{key}: after {n_steps - 2} steps")
    _same(w_end, o_end, f"{key}: after {n_steps} steps")
    assert w_end["counters"]["particles_advanced"] > 0
    if oracle:
        mo = _oracle(key, make, n_steps, event)
        assert_bitwise(mw.State, mo.State, f"{key}: State against oracle B")
        _same_particles(mw, mo)
    return w_end


@pytest.mark.parametrize("solver", ["DP5", "Tsit5"])
@pytest.mark.parametrize("wind", [(10.0, 10.0), (10.0, 3.0)], ids=["winds_10_10", "winds_10_3"])
@pytest.mark.parametrize("shape", [(64, 4), (128, 8), (192, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_staged_flavours(shape, wind, solver, monkeypatch):
    _three_ways((shape, wind, solver), lambda: _box(*shape, solver=solver, U10=wind[0], V10=wind[1]), monkeypatch)


@pytest.mark.parametrize("case", ["AutoTsit5_static", "DP5_lattice", "Tsit5_lattice", "AutoTsit5_lattice"])
def test_flavours_that_keep_their_text(case, monkeypatch):
    """the default solver under static winds and the three time-varying flavours: their node loads are the old ones, their map rows
    the new ones"""
    solver, kind = case.split("_")
    make = (lambda: _box(192, 12, solver=solver)) if kind == "static" else (lambda: _calm_patch(192, 12, solver=solver, n_steps=STEPS + 2))
    _three_ways(case, make, monkeypatch, oracle=kind == "static")      # (test_wind_grid.py holds the lattice against the oracle)


@pytest.mark.parametrize("solver", ["DP5", "Tsit5"])
@pytest.mark.parametrize("klass", [True, False], ids=["class_map_on", "class_map_off"])
def test_reach_two_takes_the_five_rows(klass, solver, monkeypatch):
    """dx = 900 m: the grid's reach gets from 1 to 2 within a few steps (asserted on the oracle), so the interior waves read three
    rows of the class map, then five of both maps — with the class map off, five of the reach map alone.  The number of waves that took
    the class path is an equality against the model of the map built from the oracle's particles (test_gpu_pull_class.py)"""
    def make():
        c = _class_box(24, 900.0)
        c.model["ODEsets"].solver = solver
        return c
    n = 9
    m1, counts = _hip(make, monkeypatch, klass, n)
    mo, want, reach = _want(make, n)
    print("class/EMPTY waves per step:", counts, "expected:", want, "reach:", reach)
    assert {1, 2} <= set(reach) and reach[-2] == 2, reach
    assert counts == (want if klass else [(0, 0)] * n)
    assert_bitwise(m1.State, mo.State, "State against oracle B")
    _same_particles(m1, mo)
    monkeypatch.setenv("PICLES_WAVEROW", "0")
    cfg = make()
    m0 = make_model(cfg, "hip")
    initialize_simulation(Simulation(m0, Δt=cfg.Δt, stop_time=1.0))
    for _ in range(n):
        time_step(m0, cfg.Δt, zero_first=True)
    _same(_snap(m1), _snap(m0), "reach 2 against k_step")


CALM_BAND = _winds(lambda i, j: (np.where(j < 12, 10.0, 0.05), np.where(j < 12, 10.0, 0.05)))


@pytest.mark.parametrize("solver", ["DP5", "Tsit5"])
def test_calm_band_on_off_and_on_again(solver, monkeypatch):
    """rows 12 .. 23 start below wind_min: their particles are off.  Behind step 3 the band gets wind: step 4 is a stand-alone advance
    (the event completed the pending step) and the fused launch of step 5, which re-meshes step 4, re-seeds the band — the branch that
    reads u0 and v0 through the global pointers and resets ln q_old.  Behind step 5 the band falls calm and is switched off, behind
    step 7 it gets its wind back: the fused launch of step 9 re-seeds it again.  The flags and the re-seed counter are looked at only
    where an event completes the step anyway; the class-path counts are held against the oracle's model of the map"""
    seen = {}

    def ev(k, m):
        if k not in (3, 5, 7):
            return False
        b = m.backend
        u = np.full((192, 24), 10.0)
        if k == 5:
            u[:, 12:] = 0.05
            z, on, _, _ = b.get_particles()
            on = on.copy()
            on[:, 12:] = 0
            b.set_particles(z, on)
        b.set_winds(u, u.copy(), m.clock.time)
        return True

    def watch(k, m):
        if k in (5, 7):
            seen[k] = (m.backend.get_particles()[1].copy(), m.backend.get_counters()["reseeds"])
        return ev(k, m)

    def make():
        c = _class_box(24, 2000.0, CALM_BAND)
        c.model["ODEsets"].solver = solver
        return c
    n = 10
    m1, counts = _hip(make, monkeypatch, True, n, watch)
    assert seen[5][0][:, 16:22].all() and seen[5][1] >= 192 * 6, "the fused launch of step 5 re-seeded the band"
    assert not seen[7][0][:, 16:22].any(), "the band is off behind step 7"
    assert m1.backend.get_particles()[1][:, 16:22].all() and m1.backend.get_counters()["reseeds"] > seen[7][1], "and on again"
    mo, want, _ = _want(make, n, ev)
    print("class/EMPTY waves per step:", counts, "expected:", want)
    assert counts == want
    assert counts[2][1] > 0 and counts[-1][0] > 0, counts
    assert_bitwise(m1.State, mo.State, "State against oracle B")
    _same_particles(m1, mo)
    monkeypatch.setenv("PICLES_WAVEROW", "0")
    cfg = make()
    m0 = make_model(cfg, "hip")
    initialize_simulation(Simulation(m0, Δt=cfg.Δt, stop_time=1.0))
    for k in range(1, n + 1):
        time_step(m0, cfg.Δt, zero_first=True)
        ev(k, m0)
    _same(_snap(m1), _snap(m0), "calm band against k_step")


@pytest.mark.parametrize("solver", ["DP5", "Tsit5"])
def test_land_block_and_boundary_nodes(solver, monkeypatch):
    """a land patch inside the middle column block (lanes 6 .. 35 of rows 4 .. 7 are not stepped: their stage is fetched and never
    read) and the grid-boundary ring stepped as the second list (the model's periodic flag on an open mesh)"""
    mask = np.ones((192, 12), dtype=bool)
    mask[70:100, 4:8] = False
    _three_ways(("land", solver), lambda: _box(192, 12, periodic=(False, False), mask=mask, model_periodic=True, solver=solver), monkeypatch)


@pytest.mark.parametrize("solver", ["DP5", "Tsit5"])
def test_reseed_set_particles_and_checkpoint_between_fused_steps(solver, monkeypatch):
    """whoever rewrites the planes between two fused launches is seen by the next one: the stage is filled anew in every launch"""
    blob = {}

    def ev(k, m):
        b = m.backend
        if k == 2:
            b.checkpoint_begin()
            blob[id(m)] = b.checkpoint_end()
        elif k == 3:
            b.seed(m.clock.time)
        elif k == 5:
            z, on, _, _ = b.get_particles()
            z = z.copy()
            z[..., 0] += 0.125
            b.set_particles(z, on)
        elif k == 7:
            b.checkpoint_load(blob[id(m)])
            m.clock.time = b.clock
    end = _three_ways(("events", solver), lambda: _box(192, 12, solver=solver), monkeypatch, n_steps=9, event=ev, oracle=False)
    assert end["counters"]["particles_advanced"] > 0
