"""The tile class map of the pull scatter (kernels.h: class_map, pull_class_waverow): a wave of k_step_waverow whose whole
neighbourhood carries one record code skips the candidate codes and goes to its four value fetches, or to nothing where nobody left a
record.  The map changes speed, never results — and a test of it passes vacuously when the path is never taken, so every case holds
two things:

  * the bits: State and particles against oracle B, and everything test_gpu_waverow compares against a run with PICLES_PULL_CLASS=0
    (which must count no class wave at all);
  * the counts: after every step, the number of waves that took the class path and the number that found it EMPTY, as an EQUALITY
    against a model of the map built from oracle B's particles.  The oracle is stepped by phases; behind its advance the positions of
    its particles give every record code, the codes give the entry of every 64-node tile (all 64 stepped and of one code), and the
    entries give the waves that qualify: interior column block, window rows inside the grid, (2 Rg + 1) x 3 entries equal and not 0,
    Rg = the largest reach of that advance.  A fused step counts what the step BEFORE it filed, and only if that one was fused too.

Shapes: 192 columns = three column blocks, one of them interior (more where a border or the boundary ring would leave no wave with a
uniform neighbourhood); 16 or 24 rows (24 where reach 3 needs interior rows).  dx is chosen so that the reach gets from 1 to 2 and from
2 to 3 within a few steps (the oracle's reach is asserted, not assumed)."""
from types import SimpleNamespace

import numpy as np
import pytest

from picles_amd import _capi as K, configs
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.timesteppers import time_step
from helpers import assert_bitwise, make_model
from test_gpu_fullsize import _same_particles
from test_gpu_waverow import _same, _snap

pytestmark = pytest.mark.gpu
EMPTY = -1


def _winds(f):
    """winds from f(i, j) -> (u, v) on node indices (the closures get coordinates: x = dx * i)"""
    def mk(dx):
        def u(x, y, t):
            return f(np.rint(x / dx).astype(int), np.rint(y / dx).astype(int))[0] + 0.0 * x

        def v(x, y, t):
            return f(np.rint(x / dx).astype(int), np.rint(y / dx).astype(int))[1] + 0.0 * x
        return SimpleNamespace(u=u, v=v)
    return mk


UNIFORM = _winds(lambda i, j: (10.0 + 0 * i, 10.0 + 0 * i))


def _box(ny, dx, winds=UNIFORM, periodic=(True, True), mask=None, model_periodic=None, NX=192):
    c = configs.bench06_box(n=8, winds=winds(dx))
    c.model["grid"] = TwoDCartesianGridMesh(dx * (NX - 1), NX, dx * (ny - 1), ny, mask=mask, periodic_boundary=periodic)
    c.model["periodic_boundary"] = all(periodic) if model_periodic is None else model_periodic
    return c


# ---- the model of the map, from oracle B's particles behind its advance ----
def _entries(mo, model_periodic):
    """(entry of every tile [3, ny], Rg of the next step's pull) from the oracle's particles as its advance left them"""
    z, on, _, _ = mo.backend.get_particles()
    mk = mo.backend.get_mask()
    grp2 = (mk == 3) & bool(model_periodic)
    stepped = (mk == 1) | grp2
    bx, by = np.floor(z[..., 3]).astype(int), np.floor(z[..., 4]).astype(int)
    code = np.where(stepped & (on == 1), np.where(grp2, 2, 1) + 4 * (bx + 2048) + 16384 * (by + 2048), 0)
    reach = np.where(code > 0, np.maximum(np.where(bx < 0, -bx, bx + 1), np.where(by < 0, -by, by + 1)), 0)
    ny = code.shape[1]
    nb = code.shape[0] // 64
    ent = np.zeros((nb, ny), dtype=np.int64)
    for b in range(nb):
        cb, sb = code[64 * b:64 * b + 64], stepped[64 * b:64 * b + 64]
        one = sb.all(axis=0) & (cb == cb[0]).all(axis=0)
        ent[b] = np.where(one, np.where(cb[0] == 0, EMPTY, cb[0]), 0)
    return ent, max(1, int(reach.max()))


def _expect(ent, Rg, ny):
    """(class waves, EMPTY waves) of a fused step that reads these entries at grid reach Rg: the interior column blocks"""
    cls = emp = 0
    for b, jl in ((b, jl) for b in range(1, ent.shape[0] - 1) for jl in range(Rg, ny - Rg)):
        w = ent[b - 1:b + 2, jl - Rg:jl + Rg + 1]
        c0 = w[1, 0]
        if c0 == 0 or not (w == c0).all():
            continue
        if c0 > 0:
            bx, by = ((c0 >> 2) & 4095) - 2048, (c0 >> 14) - 2048
            if max(-bx if bx < 0 else bx + 1, -by if by < 0 else by + 1) > Rg:
                continue
        cls += 1
        emp += int(c0 == EMPTY)
    return cls, emp


def _oracle_step(mo, dt):
    """one run!-style step of the oracle by phases; returns what its advance left, for the model above"""
    mo.upload_winds(mo.clock.time, dt)
    b = mo.backend
    b.begin_step(dt, K.STEP_ZERO_FIRST)
    b.advance_rows(K.ROWS_ALL)
    got = _entries(mo, mo.periodic_boundary)
    t0 = b.clock
    b.scatter_remesh()
    if b.clock == t0:
        b.tick(dt)
    mo.clock.time = b.clock
    return got


def _hip(make, monkeypatch, klass, n_steps, event=None):
    """n_steps fused steps through k_step_waverow; per step the (class, EMPTY) wave counts; event(k, model) runs behind step k"""
    monkeypatch.setenv("PICLES_WAVEROW", "require")
    monkeypatch.setenv("PICLES_PULL_CLASS", "1" if klass else "0")
    cfg = make()
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    counts, last = [], (0, 0)
    for k in range(1, n_steps + 1):
        time_step(m, cfg.Δt, zero_first=True)
        now = m.backend.get_pull_class_counts()
        counts.append((now[0] - last[0], now[1] - last[1]))
        last = now
        if event is not None:
            event(k, m)
            last = m.backend.get_pull_class_counts()
    return m, counts


def _case(make, monkeypatch, n_steps, event=None, oracle_event=None):
    """class path on, class path off, the oracle; returns (counts per step, expected per step, reach per step)"""
    m1, counts = _hip(make, monkeypatch, True, n_steps, event)
    m0, none = _hip(make, monkeypatch, False, n_steps, event)
    assert all(c == (0, 0) for c in none), none
    _same(_snap(m1), _snap(m0), "PICLES_PULL_CLASS=1 against 0")
    mo, want, reach = _want(make, n_steps, oracle_event)
    assert_bitwise(m1.State, mo.State, f"State after {n_steps} fused steps")
    _same_particles(m1, mo)
    print("class/EMPTY waves per step:", counts, "expected:", want, "reach:", reach)
    return counts, want, reach


def _want(make, n_steps, oracle_event=None):
    cfg = make()
    mo = make_model(cfg, ("pmath", 1))
    initialize_simulation(Simulation(mo, Δt=cfg.Δt, stop_time=1.0))
    ny = cfg.model["grid"].data.mask.shape[1]
    want, reach, prev = [], [], None
    fused = [False, False]                    # was the step before this one a fused launch, is this one?  Step 1 is a stand-alone advance
    for k in range(1, n_steps + 1):
        got = _oracle_step(mo, cfg.Δt)
        want.append(_expect(prev[0], prev[1], ny) if all(fused) else (0, 0))
        reach.append(got[1])
        prev, fused = got, [fused[1], True]
        if oracle_event is not None and oracle_event(k, mo):
            fused[1] = False                      # the event completed the pending step: the next one is a stand-alone advance again
    return mo, want, reach


def _fix_after_event(want, at):
    """an event behind step `at` completes the pending step: step at + 1 is a stand-alone advance and step at + 2 reads what it
    filed — nothing"""
    for k in (at + 1, at + 2):
        if k <= len(want):
            want[k - 1] = (0, 0)
    return want


@pytest.mark.parametrize("dx,reaches", [(900.0, {1, 2}), (500.0, {2, 3})], ids=["reach_1_to_2", "reach_2_to_3"])
def test_uniform_box_through_reach_1_2_3(dx, reaches, monkeypatch):
    """every tile carries the one code of the step: from the second fused step on, every interior wave takes the class path"""
    ny = 24
    counts, want, reach = _case(lambda: _box(ny, dx), monkeypatch, 12)
    assert counts == want
    assert reaches == set(reach), reach
    assert counts[0] == counts[1] == (0, 0)
    for k in range(3, 13):
        assert counts[k - 1] == (ny - 2 * reach[k - 2], 0), (k, counts, reach)


def test_two_wind_regimes(monkeypatch):
    """384 columns, four interior column blocks.  The border cuts through the tiles of a block (column 100) in the lower rows, runs along
    a tile edge (column 256) in the upper ones and between rows 11 and 12: waves at the border take the old path, waves inside a
    regime the class path"""
    def f(i, j):
        a = ((j < 12) & (i < 100)) | ((j >= 12) & (i < 256))
        return np.where(a, 10.0, 10.0), np.where(a, 10.0, -10.0)
    counts, want, _ = _case(lambda: _box(24, 2000.0, _winds(f), NX=384), monkeypatch, 8)
    assert counts == want
    assert all(0 < c[0] < 4 * 22 for c in counts[2:]), counts


def test_calm_band_switched_on(monkeypatch):
    """rows 12 .. 23 below wind_min: their particles are off, their tiles EMPTY; waves whose window reaches the active rows are not.
    Behind step 5 the band is switched on."""
    def f(i, j):
        return np.where(j < 12, 10.0, 0.05), np.where(j < 12, 10.0, 0.05)

    def on(k, m):
        if k == 5:
            m.backend.set_winds(np.full((192, 24), 10.0), np.full((192, 24), 10.0), m.clock.time)
            return True
        return False
    counts, want, _ = _case(lambda: _box(24, 2000.0, _winds(f)), monkeypatch, 9, event=on, oracle_event=on)
    assert counts == want
    assert all(c[1] > 0 for c in counts[2:5]), counts       # rows 13 .. 22 at reach 1: the window stays inside the band
    assert counts[5] == counts[6] == (0, 0) and counts[8][1] == 0 and counts[8][0] > 0, counts


def test_calm_grid_is_empty_everywhere(monkeypatch):
    """no wind above wind_min anywhere: nobody leaves a record, the reach counter reads 0 and the pull's reach is clamped to 1 — every
    interior wave finds its neighbourhood EMPTY and loads nothing"""
    calm = _winds(lambda i, j: (0.05 + 0 * i, 0.05 + 0 * i))
    counts, want, reach = _case(lambda: _box(16, 2000.0, calm), monkeypatch, 5)
    assert counts == want
    assert counts[2:] == [(14, 14)] * 3 and set(reach) == {1}, (counts, reach)


def test_land_inside_a_tile(monkeypatch):
    """land nodes are not stepped: their tiles keep 0 and every wave whose window touches them takes the old path"""
    mask = np.ones((192, 16), dtype=bool)
    mask[70:100, 6:9] = False
    counts, want, _ = _case(lambda: _box(16, 2000.0, mask=mask), monkeypatch, 7)
    assert counts == want
    assert all(0 < c[0] < 14 for c in counts[2:]), counts


def test_open_grid_with_both_lists(monkeypatch):
    """a non-periodic mesh under the model's periodic flag: the grid-boundary ring is stepped as the second list (code group 2): the tiles
    of the first and last row are of that list, those of the first and last column block are mixed.  320 columns: the block in the
    middle sees neither"""
    counts, want, _ = _case(lambda: _box(16, 2000.0, periodic=(False, False), model_periodic=True, NX=320), monkeypatch, 7)
    assert counts == want
    assert all(c[0] > 0 for c in counts[2:]), counts


def test_one_node_with_another_code(monkeypatch):
    """the wind over one node of the interior block blows the other way: while its particle carries another code than its neighbours
    its tile, and with it the rows of waves around it, leave the class path"""
    def f(i, j):
        odd = (i == 90) & (j == 8)
        return np.where(odd, -10.0, 10.0), np.where(odd, -10.0, 10.0)
    counts, want, _ = _case(lambda: _box(16, 2000.0, _winds(f)), monkeypatch, 7)
    assert counts == want
    assert 0 < min(c[0] for c in counts[2:]) < 14, counts


@pytest.mark.parametrize("kind", ["plain_step", "reseed", "checkpoint", "set_particles", "set_halo_rows"])
def test_stale_entries_are_never_followed(kind, monkeypatch):
    """whatever writes records or particles by other means than the fused step zeroes the map: the next step counts no class wave,
    and the bits are those of PICLES_PULL_CLASS=0 — for the plain steps, which the oracle can follow, its bits too"""
    blob = {}

    def ev(k, m):
        b = m.backend
        if kind == "plain_step" and k in (4, 6):
            b.zero_state()                 # (completes the pending step) ... and a run!-style step by the plain phases
            b.time_step(600.0, 0)
            m.clock.time = b.clock
        elif kind == "reseed" and k == 5:
            b.seed(m.clock.time)
        elif kind == "checkpoint" and k == 3:
            b.checkpoint_begin()
            blob["b"] = b.checkpoint_end()
        elif kind == "checkpoint" and k == 6:
            b.checkpoint_load(blob["b"])
            m.clock.time = b.clock
        elif kind == "set_particles" and k == 5:
            z, on, _, _ = b.get_particles()
            b.set_particles(z, on)
        elif kind == "set_halo_rows" and k == 5:
            b.set_halo_rows(3)             # re-packs both record buffers into a new ghost-row geometry
        else:
            return False
        return True
    make = lambda: _box(16, 2000.0)      # noqa: E731
    m1, counts = _hip(make, monkeypatch, True, 9, ev)
    m0, none = _hip(make, monkeypatch, False, 9, ev)
    assert all(c == (0, 0) for c in none), none
    _same(_snap(m1), _snap(m0), kind)
    print(kind, counts)
    if kind == "plain_step":
        mo = make_model(make(), ("pmath", 1))
        initialize_simulation(Simulation(mo, Δt=600.0, stop_time=1.0))
        for k in range(1, 10):
            time_step(mo, 600.0, zero_first=True)
            ev(k, mo)
        assert_bitwise(m1.State, mo.State, "State against the oracle")
        _same_particles(m1, mo)
    at = {"plain_step": (4, 6), "reseed": (5,), "checkpoint": (3, 6), "set_particles": (5,), "set_halo_rows": (5,)}[kind]
    want = [(0, 0), (0, 0)] + [(14, 0)] * 7            # 16 rows at reach 1: 14 interior waves
    for a in at:
        _fix_after_event(want, a)
    assert counts == want, (counts, want)
