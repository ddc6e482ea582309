"""Checkers of the flux means (picles_flux_mean_*, include/picles_hip.h "flux means").  Test infrastructure, never imported by
picles_amd/.  The accumulation itself is the per-step host route of the tests (State and winds through the public API, flux_node on
the host, _flux_numpy.cell_sums, then acc = acc + S in NumPy); this file restates what comes behind it:

  cover       the number of nodes each coarse cell covers
  finalise    plane_q = float32(((acc_q / (n_cover * n)) * scale_q)): the product in fp64, one division, the scale last
  tile_tree   eleven doubles per tile of 256 coarse columns: the accumulator plane through the halving tree inside each group of 64
              lanes, then the four groups in ascending order; unscaled, undivided
  totals      the partials combined sequentially from +0.0 (rank order, then (J, tile) ascending), divided by n
"""
from __future__ import annotations

import numpy as np

FIELDS = ("phi_in", "phi_dis", "phi_shift", "tq_in_x", "tq_in_y", "tq_dis_x", "tq_dis_y", "us_x", "us_y")
NACC = 11
TILE = 256


def cover(Nx, ny, cx, cy):
    """[Nxc, nyc]: cx cy, fewer in a ragged last column or row of cells"""
    nxc, nyc = -(-Nx // cx), -(-ny // cy)
    wx = np.minimum(cx, Nx - cx * np.arange(nxc))
    wy = np.minimum(cy, ny - cy * np.arange(nyc))
    return (wx[:, None] * wy[None, :]).astype(np.float64)


def finalise(acc, ncov, n, scale_phi=1.0, scale_tau=1.0, names=FIELDS):
    """float32 planes [len(names), Nxc, nyc] in the order of FIELDS"""
    assert n >= 1
    scale = [scale_phi] * 3 + [scale_tau] * 4 + [1.0] * 2
    den = ncov * np.float64(n)
    with np.errstate(over="ignore"):
        return np.stack([((acc[k] / den) * np.float64(scale[k])).astype(np.float32) for k, f in enumerate(FIELDS) if f in names])


def tile_tree(acc):
    """[nyc * tiles_per_row, 11], index J tiles_per_row + T"""
    _, nxc, nyc = acc.shape
    tpr = -(-nxc // TILE)
    out = np.zeros((nyc * tpr, NACC))
    for q in range(NACC):
        for J in range(nyc):
            for T in range(tpr):
                lanes = np.zeros(TILE)
                seg = acc[q, T * TILE:(T + 1) * TILE, J]
                lanes[:seg.size] = seg
                waves = []
                for w in range(4):
                    v = lanes[64 * w:64 * (w + 1)].copy()
                    s = 32
                    while s >= 1:
                        v = v[:s] + v[s:2 * s]
                        s //= 2
                    waves.append(v[0])
                out[J * tpr + T, q] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    return out


def totals(partials_list, n):
    """the eleven interval-mean totals: the combined partials divided by n"""
    a = [0.0] * NACC
    for p in partials_list:
        for row in np.asarray(p).reshape(-1, NACC):
            for k in range(NACC):
                a[k] = a[k] + float(row[k])
    return [x / float(n) for x in a]
