"""k_wind_sample over lattice geometry (tests/_wind_cases.py): origins offset in both signs, meshes that leave the lattice by several
periods and meshes strictly inside it, lattices finer and coarser than the mesh, spacings that are not exact in binary, nodes on
knots, on the last knot and on whole multiples of the period, two-knot axes, times before, on the last knot of and several periods
past the lattice, a knot inside the step, SMOOTH3, node counts that are not multiples of 256, a slab with j_begin > 0.

The levels are read with get_winds() / get_winds_mid() after the public calls that make the library sample a window: picles_seed
(levels at 0 and at the seed time scale) and one picles_time_step from a chosen clock (levels at t, t + Δt and, with a lattice knot
inside the step or in SMOOTH3 mode, the middle one).  The State is not under test.

Two assertions per case:
  (a) the device levels have the same bits as the NumPy mirror GriddedWinds.u / .v at the mesh nodes — the whole mesh, every case;
  (b) device and mirror are within the rounding bound u (16 max|F| + 8 Σ_a c_a Δ_a) of the exact rational interpolant
      (tests/_wind_exact.py) on about a hundred nodes per level; tests/_wind_cases.py derives the bound and states the seam rule for
      data that is not periodic.  Measured on the CPU (tests/test_aux_references.py): the mirror's worst error over the 18
      geometries is 0.19 of the bound."""
import ctypes as C

import numpy as np
import pytest

import _wind_cases as W
from helpers import assert_same_bits
from picles_amd import _capi as K, configs, fetch_relations
from picles_amd.driver import HipModel
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import build_structs
from picles_amd.wind_emulator import GriddedWinds

pytestmark = pytest.mark.gpu


def _context(c, rows=None):
    """a context on the case's mesh (rows: a slab of it) with the case's lattice uploaded"""
    cfg = configs.example_00_minimal(n=9, L=16e3)          # physics and solver settings; its seed time scale is W.SEED_STEP
    assert cfg.model["ODEsets"].timestep == W.SEED_STEP
    xmin, xmax, ymin, ymax = c.mesh
    grid = TwoDCartesianGridMesh(xmin, xmax, c.Nx, ymin, ymax, c.Ny)
    w = GriddedWinds(*c.knots, c.u, c.v, time_mode=c.mode)
    ms = fetch_relations.MinimalState(2, 2, W.SEED_STEP)
    j0, j1 = rows if rows else (0, None)
    g, p, o, m = build_structs(grid, cfg.model["ODEsys"], cfg.model["ODEsets"], None, ms, False, j_begin=j0, j_end=j1)
    b = HipModel(g, p, o, m, mask=grid.data.mask, device=0, halo_rows=2)
    b.set_wind_grid(w.lattice(), float(grid.data.x[0, 0]), float(grid.data.y[0, 0]), time_mode=c.mode)      # the global mesh origin
    return b, grid, w


def _check_level(c, grid, w, name, t, got_u, got_v, nodes, rows=None):
    """(a) and (b) for one level; returns the device's worst error / bound"""
    j0, j1 = rows if rows else (0, c.Ny)
    X, Y = grid.data.x[:, j0:j1], grid.data.y[:, j0:j1]
    xs, ys = grid.data.x[:, 0], grid.data.y[0, :]
    lat = w.lattice()
    worst = 0.0
    for comp, F, f, got in (("u", c.u, w.u, got_u), ("v", c.v, w.v, got_v)):
        assert got.shape == X.shape
        assert_same_bits(got, f(X, Y, t), f"{c.name}: {comp} at {name} = {t}: device against the mirror")
        for who, vals in (("device", got), ("mirror", f(X, Y, t))):
            r, checked = W.worst_ratio(c, lat, F, xs, ys, t, vals, [ij for ij in nodes if j0 <= ij[1] < j1], j_off=j0)
            assert checked >= 10 and r <= 1.0, (c.name, name, comp, who, r, checked)
            if who == "device":
                worst = max(worst, r)
    return worst


@pytest.mark.parametrize("c", W.all_cases(), ids=lambda c: c.name)
def test_device_levels_equal_the_mirror_and_meet_the_exact_interpolant(c):
    b, grid, w = _context(c)
    xs, ys = W.mesh_axes(c)
    assert_same_bits(grid.data.x[:, 0], xs, "mesh x"); assert_same_bits(grid.data.y[0, :], ys, "mesh y")
    assert W.excluded_share(c, w.lattice(), xs, ys) <= W.SEAM_CAP
    T = W.level_times(c)
    nodes = W.sample_nodes(c)
    b.seed(c.clock)
    u0, v0, u1, v1 = b.get_winds()
    worst = _check_level(c, grid, w, "seed0", T["seed0"], u0, v0, nodes)
    worst = max(worst, _check_level(c, grid, w, "seed1", T["seed1"], u1, v1, nodes))
    seed_levels = (u0, v0, u1, v1)
    # the library's own view of the step's window agrees with the case's
    tk = C.c_double(-1.0)
    lat = w.lattice()
    nk = K.load().picles_lattice_knots(lat["t0"], lat["dt"], c.clock, c.step, C.byref(tk))
    assert nk <= 1 and (nk == 1) == (W.knot_inside(c) is not None) and (nk == 0 or tk.value == W.knot_inside(c))
    b.time_step(c.step, K.STEP_ZERO_FIRST)
    assert b.clock == c.clock + c.step
    u0, v0, u1, v1 = b.get_winds()
    worst = max(worst, _check_level(c, grid, w, "step0", T["step0"], u0, v0, nodes))
    worst = max(worst, _check_level(c, grid, w, "step1", T["step1"], u1, v1, nodes))
    mid = b.get_winds_mid()
    assert (mid is None) == (T["mid"] is None), (c.name, T)
    if mid is not None:
        worst = max(worst, _check_level(c, grid, w, "mid", T["mid"], mid[0], mid[1], nodes))
    S = b.get_state()
    assert np.isfinite(S).all() and S[..., 0].max() > 0.0           # an ordinary step
    b.close()
    print(f"{c.name}: device vs exact, worst error / bound = {worst:.3f}")
    if c.slab:
        # the slab's rows are the same rows of the whole-grid sample: the sampler adds j_begin to the node's row
        sb, _, _ = _context(c, c.slab)
        assert (sb.j_begin, sb.ny_loc) == (c.slab[0], c.slab[1] - c.slab[0]) and sb.j_begin > 0
        sb.seed(c.clock)
        got = sb.get_winds()
        for name, a, whole in zip(("u0", "v0", "u1", "v1"), got, seed_levels):
            assert_same_bits(a, np.ascontiguousarray(whole[:, c.slab[0]:c.slab[1]]), f"{c.name}: slab {name} against the whole grid's rows")
        _check_level(c, grid, w, "seed0", T["seed0"], got[0], got[1], nodes, rows=c.slab)
        _check_level(c, grid, w, "seed1", T["seed1"], got[2], got[3], nodes, rows=c.slab)
        sb.close()
