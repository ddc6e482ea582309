"""k_step_waverow (k_step.inc, WROW) against k_step: the same model runs twice in fresh contexts, once with PICLES_WAVEROW=require
(every fused launch goes through the wave-per-row kernel, or the step is refused) and once with PICLES_WAVEROW=0 (never), fused steps
with nobody looking in between.  No fp64 operation differs between the two kernels, so everything is compared bit for bit: State, the
particles, the status words, the controller memory (ln q_old, dt_next, the auto-switch word), the counters, the reach maps — and, a few
steps later, what the reach maps and the reach counter of the compared step led to.

Shapes: the smallest that hold every path of the kernel.  64 x 4: one workgroup, its column block is both the first and the last of
its row and every row's window wraps or leaves the grid (nothing takes the scalar-addressed pull).  128 x 8: two column blocks, both
edges.  192 x 12: one interior column block, rows 1 .. 10 interior at reach 1, the top and bottom rows wrap."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from picles_amd import _capi as K, configs
from picles_amd import fetch_relations as FetchRelations
from picles_amd.driver import HipModel
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D, build_structs
from picles_amd.particle_waves_v5 import ODEParameters, ODESettings, particle_equations
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.timesteppers import time_step
from helpers import assert_bitwise, make_model
from test_gpu_checkpoint import _segment
from test_gpu_fullsize import _same_particles

pytestmark = pytest.mark.gpu
DX = 2000.0
REFUSAL = "PICLES_WAVEROW=require"


def _box(nx, ny, periodic=(True, True), solver="DP5", winds=None, mask=None, model_periodic=None, U10=10.0, V10=10.0, dt=None):
    """bench06's physics (configs.bench06_box) on an nx x ny mesh, smoothly perturbed winds: neighbouring nodes differ"""
    Lx, Ly = DX * (nx - 1), DX * (ny - 1)
    c = configs.bench06_box(n=8, U10=U10, V10=V10, winds=configs.smooth_winds(U10, V10, Lx, Ly) if winds is None else winds)
    c.model["grid"] = TwoDCartesianGridMesh(Lx, nx, Ly, ny, mask=mask, periodic_boundary=periodic)
    c.model["periodic_boundary"] = all(periodic) if model_periodic is None else model_periodic
    c.model["ODEsets"].solver = solver
    if dt is not None:
        c.Δt = dt
    return c


def _calm_patch(nx, ny, solver="AutoTsit5", lattice=True, n_steps=32):
    """config 5's forcing (configs.growing_decaying_winds: calm half, ramp, u times a cosine in time) on an nx x ny mesh; lattice: the
    closures carried as a SMOOTH3 device lattice — fused launches of the time-varying flavours"""
    DT = 20 * configs.MINUTES
    Lx, Ly = DX * (nx - 1), DX * (ny - 1)
    x0 = Lx / 2

    def u(x, y, t):
        return np.where(x < x0, 0.1, 10.0 * (x - x0) / (Lx - x0)) * np.cos(t * 3 / (3600 * 2 * np.pi))

    def v(x, y, t):
        return np.where(x < x0, 0.1, 10.0 * (x - x0) / (Lx - x0)) + 0 * t
    grid = TwoDCartesianGridMesh(Lx, nx, Ly, ny)
    ODEpars, Const_ID, _ = ODEParameters(r_g=0.85)
    psys = particle_equations(u, v, γ=Const_ID.γ, q=Const_ID.q, IDConstants=Const_ID)
    ws = FetchRelations.MinimalWindsea(10.0, 10.0, DT)
    sets = ODESettings(Parameters=ODEpars, log_energy_minimum=ws["lne"], log_energy_maximum=math.log(27), saving_step=DT, timestep=DT,
                       total_time=6 * configs.DAYS, dt=1e-3, dtmin=1e-4, force_dtmin=True)
    sets.solver = solver
    c = SimpleNamespace(model=dict(grid=grid, winds=SimpleNamespace(u=u, v=v), ODEsys=psys, ODEsets=sets, ODEinit_type="wind_sea",
                                   periodic_boundary=False, boundary_type="same",
                                   minimal_particle=FetchRelations.MinimalParticle(10.0, 10.0, DT), movie=False, winds_static=False),
                        Δt=DT, n_steps=n_steps, mode="run")
    return configs.closure_lattice(c, n_steps, y=np.array([0.0, float(grid.data.y[0, -1])])) if lattice else c


def _snap(m):
    b = m.backend
    b.checkpoint_begin()
    blob = b.checkpoint_end()
    z, on, bnd, st = b.get_particles()
    seg = {k: _segment(blob, k, t) for k, t in (("qold", np.float64), ("dtn", np.float64), ("asw", np.int32), ("status", np.int32),
                                                  ("on", np.uint8), ("pflags", np.uint8), ("reach_maps", np.int32))}
    return dict(State=b.get_state(), z=z, on=on, bnd=bnd, st=st, counters=b.get_counters(), seg=seg)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, what):
    for k in ("State", "on", "bnd", "st"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k}: {int((_bits(a[k]) != _bits(b[k])).sum())} values differ"
    live = ((a["st"] & 1) == 1) & (a["on"] == 1)        # the state vector and the controller memory of a switched-off particle are dead storage
    assert np.array_equal(_bits(a["z"][live]), _bits(b["z"][live])), f"{what}: particle state"
    flat = live.reshape(-1, order="F")
    for k in ("qold", "dtn", "asw"):
        assert np.array_equal(_bits(a["seg"][k][flat]), _bits(b["seg"][k][flat])), f"{what}: controller memory {k}"
    for k in ("status", "on", "pflags", "reach_maps"):
        assert np.array_equal(a["seg"][k], b["seg"][k]), f"{what}: {k}"
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])      # max_reach_seen and wave_attempt_slots among them


def _run(make, mode, monkeypatch, n_steps, later, reseed_at=None):
    """n_steps fused steps unobserved -> snapshot -> `later` more -> snapshot"""
    monkeypatch.setenv("PICLES_WAVEROW", mode)
    cfg = make()
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    out = []
    for k in range(1, n_steps + later + 1):
        time_step(m, cfg.Δt, zero_first=True)
        if k == reseed_at:
            m.backend.seed(m.clock.time)
        if k == n_steps or k == n_steps + later:
            out.append(_snap(m))
    return m, out


def _both(make, monkeypatch, n_steps=25, later=3, reseed_at=None):
    mw, w = _run(make, "require", monkeypatch, n_steps, later, reseed_at)
    m0, o = _run(make, "0", monkeypatch, n_steps, later, reseed_at)
    _same(w[0], o[0], f"after {n_steps} fused steps")
    _same(w[1], o[1], f"{later} steps later")
    assert w[0]["counters"]["particles_advanced"] > 0
    return w[1]["counters"], w


@pytest.mark.parametrize("periodic", [(True, True), (True, False), (False, False)], ids=["periodic", "periodic_x", "open"])
@pytest.mark.parametrize("shape", [(64, 4), (128, 8), (192, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_boundaries(shape, periodic, monkeypatch):
    _both(lambda: _box(*shape, periodic=periodic), monkeypatch)


@pytest.mark.parametrize("solver", ["DP5", "Tsit5", "AutoTsit5"])
def test_solvers_static_winds(solver, monkeypatch):
    _both(lambda: _box(192, 12, solver=solver), monkeypatch)


@pytest.mark.parametrize("solver", ["DP5", "Tsit5", "AutoTsit5"])
def test_calm_patch_device_lattice(solver, monkeypatch):
    """the time-varying flavours (SMOOTH3 lattice).  Half the mesh is calm: some particles are off at the snapshot and others were
    re-seeded on the way (both asserted).  Whether a reach-map tile stayed empty or a dispatch order was followed is not asserted here."""
    c, w = _both(lambda: _calm_patch(192, 12, solver=solver), monkeypatch, n_steps=28, later=4)
    on = w[0]["on"]
    assert 0 < int(on.sum()) < on.size
    assert c["reseeds"] > 0


def test_land_mask_and_boundary_list(monkeypatch):
    """a land patch and stepped grid-boundary particles (the model's periodic flag on an open mesh): records of both lists"""
    mask = np.ones((192, 12), dtype=bool)
    mask[70:100, 4:8] = False
    _both(lambda: _box(192, 12, periodic=(False, False), mask=mask, model_periodic=True), monkeypatch)


def test_reach_grows_to_two_and_three(monkeypatch):
    """strong winds and a long step: the scatter reach passes 2 (the two-phase window of reach 2) and 3 (a row at a time)"""
    c, _ = _both(lambda: _box(192, 16, U10=18.0, V10=14.0, dt=45 * configs.MINUTES), monkeypatch, n_steps=30, later=3)
    assert c["max_reach_seen"] >= 3, c


def test_reseed_in_the_middle(monkeypatch):
    _both(lambda: _box(192, 12), monkeypatch, n_steps=25, later=3, reseed_at=12)


def test_against_the_oracle(monkeypatch):
    """192 x 12 periodic, DP5, through k_step_waverow: State and particles equal oracle B's"""
    monkeypatch.setenv("PICLES_WAVEROW", "require")
    pair = [make_model(_box(192, 12), b) for b in ("hip", ("pmath", 1))]
    cfg = _box(192, 12)
    for m in pair:
        initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
        for _ in range(25):
            time_step(m, cfg.Δt, zero_first=True)
    assert_bitwise(pair[0].State, pair[1].State, "State after 25 fused steps")
    _same_particles(*pair)


@pytest.mark.parametrize("shape", [(96, 8), (64, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry_that_does_not_qualify(shape, monkeypatch):
    """`require` refuses the fused step with its text and leaves the context as it was and usable; the default mode gives the bits of
    PICLES_WAVEROW=0"""
    make = lambda: _box(*shape)      # noqa: E731
    monkeypatch.setenv("PICLES_WAVEROW", "require")
    cfg = make()
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    before = _snap(m)
    with pytest.raises(K.PiclesError, match=REFUSAL):
        m.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    _same(_snap(m), before, "after the refusal")
    assert m.backend.clock == 0.0
    m.backend.time_step(cfg.Δt, 0)                    # the plain phases are not fused launches: the context steps on
    monkeypatch.setenv("PICLES_WAVEROW", "0")
    ref = WaveGrowth2D(**make().model)
    initialize_simulation(Simulation(ref, Δt=cfg.Δt, stop_time=1.0))
    ref.backend.time_step(cfg.Δt, 0)
    _same(_snap(m), _snap(ref), "a plain step after the refusal")
    monkeypatch.delenv("PICLES_WAVEROW")
    _, d = _run(make, "1", monkeypatch, 25, 3)
    _, o = _run(make, "0", monkeypatch, 25, 3)
    _same(d[0], o[0], "default mode")
    _same(d[1], o[1], "default mode, later")


def _slab(mode, monkeypatch):
    """rows 0 .. 15 of a 64 x 32 periodic box as one rank of two holds them (halo of 2 rows)"""
    monkeypatch.setenv("PICLES_WAVEROW", mode)
    cfg = configs.bench06_box(n=8)
    cfg.model["grid"] = TwoDCartesianGridMesh(DX * 63, 64, DX * 31, 32, periodic_boundary=(True, True))
    ms = FetchRelations.MinimalState(2, 2, cfg.model["ODEsets"].timestep)
    g, p, o, mm = build_structs(cfg.model["grid"], cfg.model["ODEsys"], cfg.model["ODEsets"], None, ms, True, j_begin=0, j_end=16)
    hm = HipModel(g, p, o, mm, mask=cfg.model["grid"].data.mask[:, 0:16], device=0, halo_rows=2)
    x = np.arange(64)[:, None] + 0.0 * np.arange(16)[None, :]
    hm.set_winds(10.0 + np.sin(x / 7.0), 9.0 + np.cos(x / 5.0) + 0.0 * x, 0.0)
    hm.seed(0.0)
    return hm, cfg.Δt


def test_slab_edge_launch_does_not_qualify(monkeypatch):
    """a slab's edge launch covers two row ranges: `require` refuses the fused step; in the default mode the interior rows (12 rows
    of 64) take the wave-per-row kernel, the edge rows the old one, and the bits are those of PICLES_WAVEROW=0"""
    hm, dt = _slab("require", monkeypatch)
    with pytest.raises(K.PiclesError, match=REFUSAL):
        hm.begin_fused_step(dt)
    assert hm.clock == 0.0
    hm.begin_step(dt, K.STEP_ZERO_FIRST)              # usable: a plain step
    hm.advance_rows(K.ROWS_ALL)
    hm.scatter_remesh()
    assert np.isfinite(hm.get_state()).all()
    got = []
    for mode in ("1", "0"):
        hm, dt = _slab(mode, monkeypatch)
        for _ in range(8):
            assert hm.begin_fused_step(dt)
            hm.step_rows(K.ROWS_EDGE)
            hm.step_rows(K.ROWS_INTERIOR)
            hm.end_fused_step()
        z, on, bnd, st = hm.get_particles()
        got.append((hm.get_state(), z[((st & 1) == 1) & (on == 1)], on, st, hm.get_counters()))
    for a, b in zip(got[0][:4], got[1][:4]):
        assert np.array_equal(_bits(a), _bits(b))
    assert got[0][4] == got[1][4]
