"""Lattice geometries for the gridded-wind sampler (k_wind_sample on the device in tests/test_gpu_wind_sampler.py, the NumPy mirror
picles_amd/wind_emulator.py on the CPU in tests/test_aux_references.py), the rounding bound both are held to against the exact
rational interpolant of tests/_wind_exact.py, and the bookkeeping of the nodes near a seam.

THE BOUND.  With u = 2^-53, F the lattice data, c_a the largest |lattice coordinate| a case reaches on axis a (x, y, t) and Δ_a the
largest difference between neighbouring knots along that axis,

    |computed - exact|  <=  u (K1 max|F| + K2 Σ_a c_a Δ_a),        K1 = 16,  K2 = 8.

Coordinate: c = (x - x0) * (1 / dx) is three roundings (the difference, the reciprocal, the product), a relative error of 3u to
first order, so the coordinate is off by at most 3u |c|.  The wrap c - floor(c / per) per adds nothing: the floor and the product of
two integers below 2^53 are exact, and the difference of c and an integer no larger than it is a multiple of ulp(c) of smaller
magnitude, so it is exact as well (if c / per rounds across an integer the point lands one period away, a hair outside the first or
last cell, which for a continuous periodic interpolant is the same function).  The exact interpolant is continuous and piecewise
linear in every coordinate with slope at most Δ_a; a computed point that falls into the neighbouring cell extrapolates that
cell's line instead, which differs by at most another slope: 2 Δ_a 3u c_a = 6u c_a Δ_a per axis.
Lerp: fl(a + fl(fl(b - a) f)) with |a|, |b| <= M and f in [0, 1] errs by at most 2u |b - a| f + u |result| <= 5u M; a lerp is a
convex combination, so errors of its inputs pass with weight at most one; three nested levels (x, then y, then t): 15u M.
First order therefore gives K1 = 15 and K2 = 6; 16 and 8 cover the second-order terms and weights a hair outside [0, 1].
The constants come from this count, not from what any implementation returns.

SEAMS.  Data that is not periodic along an axis (first plane != last plane) makes the periodic continuation jump at every whole
multiple of the period, and a coordinate one ulp off may legitimately land on either side.  The bound is therefore asserted on
every node where the data is periodic along each axis the case leaves, and otherwise only on nodes farther than SEAM_EPS lattice
units from a seam of a non-periodic axis — at most SEAM_CAP of a case's nodes may be excluded that way, counted on the exact
coordinates."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import _wind_exact as X

U = 2.0 ** -53
K1, K2 = 16.0, 8.0
SEAM_EPS = 1e-6
SEAM_CAP = 0.02
SEED_STEP = 600.0            # the seed window's second level: ODESettings.timestep of the configuration the tests build


def _case(name, Nx, Ny, mesh, lat, clock, step=600.0, mode="linear", periodic=True, seed=0, slab=None):
    """mesh = (xmin, xmax, ymin, ymax): Nx x Ny nodes, ends included;  lat = (x0, dx, nx, y0, dy, ny, t0, dt, nt)"""
    x0, dx, nx, y0, dy, ny, t0, dt, nt = lat
    rng = np.random.default_rng(1000 + seed)
    # physical winds, |U| <= 30 m/s: smooth part plus knot-to-knot noise
    u = 10.0 + 8.0 * rng.uniform(-1.0, 1.0, (nx, ny, nt))
    v = -4.0 + 8.0 * rng.uniform(-1.0, 1.0, (nx, ny, nt))
    c = SimpleNamespace(name=name, Nx=Nx, Ny=Ny, mesh=tuple(float(a) for a in mesh), clock=float(clock), step=float(step), mode=mode,
                        periodic=periodic, seed=seed, slab=slab,
                        knots=(x0 + dx * np.arange(nx), y0 + dy * np.arange(ny), t0 + dt * np.arange(nt)), u=u, v=v)
    if periodic:
        for axis, left in enumerate(axes_left(c)):
            if left:
                for F in (c.u, c.v):
                    idx = [slice(None)] * 3
                    idx[axis] = -1
                    first = [slice(None)] * 3
                    first[axis] = 0
                    F[tuple(idx)] = F[tuple(first)]
    return c


def mesh_axes(c):
    """node coordinates as the mesh (picles_amd.grids.TwoDCartesianGridMesh) and the device form them: xmin + dx i"""
    xmin, xmax, ymin, ymax = c.mesh
    return xmin + ((xmax - xmin) / (c.Nx - 1)) * np.arange(c.Nx), ymin + ((ymax - ymin) / (c.Ny - 1)) * np.arange(c.Ny)


def knot_inside(c):
    """time of the first lattice knot strictly inside (clock, clock + step), or None; the cases keep knots well away from the ends"""
    t0, dt = float(c.knots[2][0]), float(c.knots[2][1] - c.knots[2][0])
    k = math.floor((c.clock - t0) / dt) + 1.0
    tk = t0 + k * dt
    return tk if c.clock < tk < c.clock + c.step else None


def level_times(c):
    """the times the library samples: at the seed (0 and the seed time scale), then for one step from `clock`"""
    tm = c.clock + 0.5 * c.step if c.mode == "smooth3" else knot_inside(c)
    return dict(seed0=0.0, seed1=SEED_STEP, step0=c.clock, step1=c.clock + c.step, mid=tm)


def _coords(c):
    xs, ys = mesh_axes(c)
    ts = np.array([t for t in level_times(c).values() if t is not None])
    out = []
    for pts, k in zip((xs, ys, ts), c.knots):
        out.append((pts - k[0]) / (k[1] - k[0]))
    return out


def axes_left(c):
    """per axis: does a node or a sampled time lie outside the lattice (or within SEAM_EPS of its ends)?"""
    return [bool(((cc < SEAM_EPS) | (cc > k.size - 1 - SEAM_EPS)).any()) for cc, k in zip(_coords(c), c.knots)]


def bound(c, F):
    s = sum(float(np.abs(cc).max()) * (float(np.abs(np.diff(F, axis=a)).max()) if F.shape[a] > 1 else 0.0) for a, cc in enumerate(_coords(c)))
    return U * (K1 * float(np.abs(F).max()) + K2 * s)


def _jumps(F):
    """per axis: is the data NOT periodic (first plane != last plane)?"""
    return [not np.array_equal(np.take(F, 0, axis=a), np.take(F, -1, axis=a)) for a in range(3)]


def near_seam(c, lat, F, xs, ys, t):
    """boolean [len(xs), len(ys)]: nodes closer than SEAM_EPS to a seam of an axis along which F jumps, on the exact coordinates"""
    jx, jy, jt = _jumps(F)
    bx = np.array([jx and X.seam_distance(X.coord(x, lat["x0"], lat["dx"]), F.shape[0]) < SEAM_EPS for x in xs])
    by = np.array([jy and X.seam_distance(X.coord(y, lat["y0"], lat["dy"]), F.shape[1]) < SEAM_EPS for y in ys])
    bt = bool(jt and X.seam_distance(X.coord(t, lat["t0"], lat["dt"]), F.shape[2]) < SEAM_EPS)
    return bx[:, None] | by[None, :] | bt


def sample_nodes(c, n=96):
    """(i, j) pairs checked against the exact interpolant: the corners, the edges' middles and n seeded random nodes"""
    rng = np.random.default_rng(77 + c.seed)
    ij = {(0, 0), (c.Nx - 1, 0), (0, c.Ny - 1), (c.Nx - 1, c.Ny - 1), (c.Nx // 2, 0), (0, c.Ny // 2)}
    ij |= {(int(a), int(b)) for a, b in zip(rng.integers(0, c.Nx, n), rng.integers(0, c.Ny, n))}
    return sorted(ij)


def worst_ratio(c, lat, F, xs, ys, t, values, nodes, j_off=0):
    """max over `nodes` (outside the seam exclusion) of |values[i, j - j_off] - exact| / bound, and the number of nodes checked"""
    skip = near_seam(c, lat, F, xs, ys, t)
    b = bound(c, F)
    worst, checked = 0.0, 0
    for i, j in nodes:
        if skip[i, j]:
            continue
        err = abs(X.Fraction(float(values[i, j - j_off])) - X.at(F, lat, xs[i], ys[j], t))
        worst = max(worst, float(err / X.Fraction(b)))
        checked += 1
    return worst, checked


def excluded_share(c, lat, xs, ys):
    """share of (node, level, component) values the seam rule excludes"""
    tot = exc = 0
    for t in level_times(c).values():
        if t is None:
            continue
        for F in (c.u, c.v):
            m = near_seam(c, lat, F, xs, ys, t)
            tot += m.size
            exc += int(m.sum())
    return exc / tot


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases.  Lattice units: c = (x - x0) / dx; "leaves by" in periods of (n - 1) dx
# ------------------------------------------------------------------------------------------------------------------------------------
def directed():
    C = []
    # lattice origin to the right of / above the mesh origin, coarser than the mesh (2 km nodes, 3 and 4 km knots); the mesh leaves it
    # by 3.3 periods on the left and 5.5 on the right; the times leave it on both sides too (lattice 5000 ... 6800 s): 0 and 600 s lie
    # before its first knot, 12000 and 12600 four periods past its last, and the knot 12200 s (a whole multiple of the period,
    # c = 8 -> 0) falls inside the step: a mid level
    C.append(_case("coarse_offset_pos_several_periods", 41, 29, (0.0, 80e3, 0.0, 56e3), (30e3, 3e3, 4, 25e3, 4e3, 3, 5000.0, 900.0, 3), 12000.0, seed=1))
    # lattice origin to the left of / below the mesh origin, finer than the mesh (700 and 900 m knots), the mesh and every time
    # strictly inside: no wrap anywhere; 32 x 24 = 3 x 256 nodes; data not periodic
    C.append(_case("fine_offset_neg_mesh_inside", 32, 24, (0.0, 62e3, 0.0, 46e3), (-10e3, 700.0, 120, -7e3, 900.0, 70, -3000.0, 2500.0, 4), 1200.0, periodic=False, seed=2))
    # every node ON a knot (2 km nodes over 4 km knots from 8 km: every other node), on the last knot (x = 24 km: c = 4 = per) and
    # on whole multiples of the period in both directions (c = -12, -8, -4, 0, 4, 8); times (knots at -1200, -600, 0, 600 s): 600 s = the last
    # knot (c = 3 = per), 0 s on a knot, 4200 s = three periods (c = 9), 3600 s
    C.append(_case("nodes_on_knots_and_period_multiples", 41, 31, (-40e3, 40e3, -30e3, 30e3), (8e3, 4e3, 5, 6e3, 4e3, 4, -1200.0, 600.0, 4), 3600.0, seed=3))
    # two knots on one axis at a time: that axis spans the mesh (so its two planes differ), the others are left
    C.append(_case("nx2", 37, 23, (0.0, 64e3, 0.0, 40e3), (-5e3, 75e3, 2, 11e3, 3.3e3, 4, 100.0, 1300.0, 3), 2400.0, seed=4))
    C.append(_case("ny2", 37, 23, (0.0, 64e3, 0.0, 40e3), (9e3, 5.1e3, 5, -1e3, 43e3, 2, 100.0, 1300.0, 3), 2400.0, seed=5))
    C.append(_case("nt2", 37, 23, (0.0, 64e3, 0.0, 40e3), (9e3, 5.1e3, 5, 11e3, 3.3e3, 4, -1000.0, 9000.0, 2), 1200.0, seed=6))
    # mesh spacing that is not exact in binary (64 km / 36, 40 km / 22), lattice spacing neither; a knot inside the step
    C.append(_case("inexact_spacings_knot_inside", 37, 23, (1e3 / 3, 1e3 / 3 + 64e3, -0.7e3, 39.3e3), (7e3 / 3, 1e4 / 7, 9, 1e3 / 9, 1.7e3, 7, 50.0, 700.0, 5), 3000.0, seed=7))
    # SMOOTH3: three levels, the middle one at clock + step / 2
    C.append(_case("smooth3", 33, 27, (0.0, 64e3, 0.0, 52e3), (-3e3, 6.5e3, 6, 2e3, 5.5e3, 5, 0.0, 300.0, 9), 4800.0, mode="smooth3", seed=8))
    # data that is NOT periodic under a mesh and times that leave the lattice: same bits everywhere, the bound away from the seams
    C.append(_case("non_periodic_left", 37, 23, (1e3 / 3, 1e3 / 3 + 64e3, -0.7e3, 39.3e3), (7e3 / 3, 1e4 / 7, 9, 1e3 / 9, 1.7e3, 7, 50.0, 700.0, 5), 7250.0, periodic=False, seed=9))
    # a slab: rows 8 ... 23 of 32 (j_begin > 0); its levels must equal the same rows of the whole grid's
    C.append(_case("slab_rows_8_24", 37, 32, (0.0, 64e3, 0.0, 55e3), (20e3, 3.7e3, 5, 30e3, 2.9e3, 4, 200.0, 450.0, 4), 0.0, seed=10, slab=(8, 24)))
    return C


def random_cases(n=8, seed0=100):
    C = []
    for k in range(n):
        rng = np.random.default_rng(seed0 + k)
        Nx, Ny = int(rng.integers(17, 48)), int(rng.integers(9, 40))
        dxm, dym = float(rng.uniform(1.5e3, 3e3)), float(rng.uniform(1.5e3, 3e3))
        xmin, ymin = float(rng.uniform(-50e3, 50e3)), float(rng.uniform(-50e3, 50e3))
        nx, ny, nt = (int(a) for a in rng.integers(2, 9, 3))
        # knots from 0.3 to 3 mesh spacings apart; origin anywhere within a few mesh widths of the mesh, on either side
        dx, dy = dxm * float(2.0 ** rng.uniform(-1.7, 1.6)), dym * float(2.0 ** rng.uniform(-1.7, 1.6))
        x0 = xmin + float(rng.uniform(-2.0, 2.0)) * dxm * Nx
        y0 = ymin + float(rng.uniform(-2.0, 2.0)) * dym * Ny
        dt = float(rng.uniform(700.0, 3000.0))
        t0 = float(rng.uniform(-20e3, 20e3))
        clock = 600.0 * int(rng.integers(0, 60))
        C.append(_case(f"random_{seed0 + k}", Nx, Ny, (xmin, xmin + dxm * (Nx - 1), ymin, ymin + dym * (Ny - 1)),
                       (x0, dx, nx, y0, dy, ny, t0, dt, nt), clock, mode="smooth3" if k % 4 == 3 else "linear", periodic=(k % 3 != 2),
                       seed=seed0 + k))
    return C


def all_cases():
    return directed() + random_cases()
