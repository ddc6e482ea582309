"""Exact rational evaluation of the gridded-wind interpolant, written from include/picles_hip.h (picles_set_wind_grid: "tri-linear,
periodic continuation", the period of an axis being its last knot minus its first) and from the definition of a periodic
piecewise-linear interpolant — NOT from the kernel or from picles_amd/wind_emulator.py, and importing nothing from picles_amd/.
Every input is a double and is taken at its exact value (fractions.Fraction); nothing is rounded anywhere.

An axis has n >= 2 knots at x0 + k dx, k = 0 ... n - 1.  In lattice units c = (x - x0) / dx the knots sit at the integers 0 ... n - 1
and the period is per = n - 1.  A point inside [0, per] is interpolated where it lies (c = per belongs to the last cell, weight 1);
a point outside is moved by a whole number of periods into [0, per) first."""
from __future__ import annotations

import math
from fractions import Fraction


def coord(x, x0, dx):
    """exact lattice coordinate of the double x on an axis with the doubles x0, dx"""
    return (Fraction(float(x)) - Fraction(float(x0))) / Fraction(float(dx))


def cell_of(c, n):
    """(i0, f): the cell [i0, i0 + 1] with 0 <= i0 <= n - 2 and the weight f in [0, 1] of the exact lattice coordinate c"""
    per = n - 1
    if c < 0 or c > per:
        c = c - math.floor(c / per) * per          # into [0, per)
    i0 = min(math.floor(c), n - 2)
    return i0, c - i0


def seam_distance(c, n):
    """distance, in lattice units, of the exact coordinate c from the nearest whole multiple of the period (0 and per included):
    where the continuation of data that is not periodic jumps"""
    per = n - 1
    r = c - math.floor(c / per) * per
    return min(r, per - r)


def interp(F, cx, cy, ct):
    """the tri-linear interpolant of the lattice F[nx, ny, nt] (doubles) at the exact lattice coordinates (cx, cy, ct)"""
    nx, ny, nt = F.shape
    (ix, fx), (iy, fy), (it, ft) = cell_of(cx, nx), cell_of(cy, ny), cell_of(ct, nt)
    g = lambda a, b, c: Fraction(float(F[ix + a, iy + b, it + c]))
    lerp = lambda p, q, f: p + (q - p) * f
    c0 = lerp(lerp(g(0, 0, 0), g(1, 0, 0), fx), lerp(g(0, 1, 0), g(1, 1, 0), fx), fy)
    c1 = lerp(lerp(g(0, 0, 1), g(1, 0, 1), fx), lerp(g(0, 1, 1), g(1, 1, 1), fx), fy)
    return lerp(c0, c1, ft)


def at(F, lat, x, y, t):
    """the interpolant at the doubles (x, y, t); lat: dict with x0, dx, y0, dy, t0, dt (doubles)"""
    return interp(F, coord(x, lat["x0"], lat["dx"]), coord(y, lat["y0"], lat["dy"]), coord(t, lat["t0"], lat["dt"]))
