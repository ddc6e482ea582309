"""An independent restatement of picles_amd/station_output.py's definition (its module docstring): points -> corners and weights,
and the per-station arithmetic — written station by station and corner by corner with NumPy fp64 scalars, no vectorisation,
so that the writer's vectorised form is held against the text rather than against itself."""
import math

import numpy as np

VAR_NAMES = ("e", "m_x", "m_y", "hs", "tp", "cg_x", "cg_y", "dir")
FOUR_PI = np.float64(12.566370614359172)


def axis(x, coords, periodic=False, tripolar=False):
    """(i0, i1, w) on one axis; raises ValueError outside"""
    N = len(coords)
    x0, xN = np.float64(coords[0]), np.float64(coords[-1])
    dx = (xN - x0) / np.float64(N - 1)
    xi = (np.float64(x) - x0) / dx
    if periodic:
        if xi < 0 or xi >= N:
            raise ValueError("outside")
        i0 = int(np.floor(xi))
        return i0, (i0 + 1) % N, np.float64(xi - i0)
    if xi < 0 or xi > N - 1:
        raise ValueError("outside")
    if tripolar and xi >= N - 2:
        raise ValueError("top cell row")
    i0 = int(np.floor(xi))
    if i0 == N - 1:
        return N - 2, N - 1, np.float64(1.0)
    return i0, i0 + 1, np.float64(xi - i0)


def corners_of(point, xs, ys, periodic=(False, False), tripolar=False):
    """[((i, j), weight)] x 4 in the visiting order"""
    i0, i1, wx = axis(point[0], xs, periodic[0])
    j0, j1, wy = axis(point[1], ys, periodic[1], tripolar)
    one = np.float64(1.0)
    return [((i0, j0), (one - wx) * (one - wy)), ((i1, j0), wx * (one - wy)), ((i0, j1), (one - wx) * wy), ((i1, j1), wx * wy)]


def record(corner_values, g, r_g):
    """corner_values: [((e, m_x, m_y), weight)] in the visiting order -> the eight variables of one station and sample"""
    W = SE = SX = SY = np.float64(0.0)
    for (e, mx, my), w in corner_values:
        e, mx, my, w = np.float64(e), np.float64(mx), np.float64(my), np.float64(w)
        if np.isfinite(e) and np.isfinite(mx) and np.isfinite(my) and e > 0 and mx * mx + my * my > 0:
            W = W + w
            SE = SE + w * e
            SX = SX + w * mx
            SY = SY + w * my
    if not W > 0:
        return np.full(8, np.nan)
    E, MX, MY = SE / W, SX / W, SY / W
    M2 = MX * MX + MY * MY
    if not M2 > 0:
        return np.full(8, np.nan)
    hs = np.float64(4.0) * np.sqrt(E)
    cgx = (MX * E) / (np.float64(2.0) * M2)
    cgy = (MY * E) / (np.float64(2.0) * M2)
    cbar = E / (np.float64(2.0) * np.sqrt(M2))
    tp = (FOUR_PI * max(cbar / np.float64(r_g), np.float64(0.1))) / np.float64(g)
    return np.array([E, MX, MY, hs, tp, cgx, cgy, np.arctan2(MY, MX)])


def series_from_states(states, stations, g, r_g):
    """states: list of State arrays [Nx, Ny, 3]; stations: list of corner lists [((i, j), weight)] -> [time, station, 8]"""
    out = np.empty((len(states), len(stations), 8))
    for k, S in enumerate(states):
        for s, corners in enumerate(stations):
            out[k, s] = record([(tuple(S[i, j, :]), w) for (i, j), w in corners], g, r_g)
    return out
