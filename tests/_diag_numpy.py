"""Independent NumPy restatement of the coarse wave diagnostics as include/picles_hip.h defines them ("THE DEFINITION" of the
picles_diag_* section).  Test infrastructure: the checker of tests/test_field_output_host.py and tests/test_gpu_field_output.py,
never imported by picles_amd/.  Vectorised over the coarse cells, with the per-cell order of the definition (j outer, i inner)
kept as the order of the two Python loops."""
from __future__ import annotations

import math

import numpy as np

FIELDS = ("hs", "tp", "cg_x", "cg_y", "e", "m_x", "m_y")
TILE = 256
FOUR_PI = 4.0 * math.pi


def fmax(a, b):
    """the fmax of the definition: a NaN — quiet or signalling — is skipped; NaN only when both are.  (np.fmax hands a signalling NaN
    to the C library, which answers NaN or the number depending on the loop NumPy happens to take.)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.where(np.isnan(b), a, np.where(np.isnan(a), b, np.maximum(a, b)))


def coarse_shape(Nx, ny, cx, cy):
    return -(-Nx // cx), -(-ny // cy)


def cell_sums(state, cx, cy):
    """per coarse cell: Σe, Σm_x, Σm_y, n over the wet nodes (from +0.0, j outer, i inner) and the fmax of the three planes over all
    nodes (from -inf).  state: [Nx, ny, 3] (the context's own rows; its first row must be a multiple of cy in global indices)"""
    Nx, ny = state.shape[:2]
    nxc, nyc = coarse_shape(Nx, ny, cx, cy)
    S = [np.zeros((nxc, nyc)) for _ in range(4)]
    X = [np.full((nxc, nyc), -np.inf) for _ in range(3)]
    with np.errstate(all="ignore"):
        for jj in range(cy):
            for ii in range(cx):
                sub = state[ii::cx, jj::cy]
                a, b = sub.shape[:2]
                if a == 0 or b == 0:
                    continue
                e, mx, my = sub[..., 0], sub[..., 1], sub[..., 2]
                m2 = mx * mx + my * my
                wet = np.isfinite(e) & np.isfinite(mx) & np.isfinite(my) & (e > 0.0) & (m2 > 0.0)
                for acc, v in zip(S, (e, mx, my, np.ones_like(e))):
                    acc[:a, :b] = np.where(wet, acc[:a, :b] + np.where(wet, v, 0.0), acc[:a, :b])
                for acc, v in zip(X, (e, mx, my)):
                    acc[:a, :b] = fmax(acc[:a, :b], v)
    return S, X


def fields_of(state, cx, cy, g, r_g, names=FIELDS):
    """float32 planes [len(names), Nxc, nyc] in the order of FIELDS (whatever the order of `names`); NaN where a cell is not valid"""
    (se, sx, sy, n), _ = cell_sums(state, cx, cy)
    with np.errstate(all="ignore"):
        E, MX, MY = se / n, sx / n, sy / n
        M2 = MX * MX + MY * MY
        valid = (n > 0.0) & (M2 > 0.0)
        cbar = E / (2.0 * np.sqrt(M2))
        planes = {
            "hs": 4.0 * np.sqrt(E),
            "tp": (FOUR_PI * fmax(cbar / r_g, 0.1)) / g,
            "cg_x": (MX * E) / (2.0 * M2),
            "cg_y": (MY * E) / (2.0 * M2),
            "e": E, "m_x": MX, "m_y": MY}
        out = [np.where(valid, planes[f], np.nan).astype(np.float32) for f in FIELDS if f in names]
    return np.stack(out), valid


def _tree(v, op):
    """v: [tiles, 256, nyc] -> [tiles, nyc]: halving tree inside each group of 64 lanes, then the four groups in ascending order"""
    t, _, nyc = v.shape
    v = v.reshape(t, 4, 64, nyc)
    s = 32
    while s >= 1:
        v = op(v[:, :, :s], v[:, :, s:2 * s])
        s //= 2
    w = v[:, :, 0]
    return op(op(op(w[:, 0], w[:, 1]), w[:, 2]), w[:, 3])


def partials_of(state, cx, cy):
    """[n_partials, 7]: sum_e, sum_mx, sum_my, n_wet, max_e, max_mx, max_my per tile of 256 coarse columns, index J tiles_per_row + T"""
    S, X = cell_sums(state, cx, cy)
    nxc, nyc = S[0].shape
    tpr = -(-nxc // TILE)
    cols = []
    with np.errstate(all="ignore"):
        for a, fillv, op in [(s, 0.0, np.add) for s in S] + [(x, -np.inf, fmax) for x in X]:
            pad = np.full((tpr * TILE, nyc), fillv)
            pad[:nxc] = a
            r = _tree(pad.reshape(tpr, TILE, nyc), op)          # [tiles, nyc]
            if op is fmax:
                r = r + 0.0
            cols.append(r.T.reshape(-1))                        # J outer, tile inner
    return np.stack(cols, axis=1)


def combine(partials_list, Nx, Ny):
    """the eight scalars: sequential over the partials in the order given (rank order, then (J, tile) ascending)"""
    acc = [0.0, 0.0, 0.0, 0.0, -math.inf, -math.inf, -math.inf]
    for p in partials_list:
        for row in np.asarray(p).reshape(-1, 7):
            for k in range(4):
                acc[k] = acc[k] + float(row[k])
            for k in range(4, 7):
                acc[k] = float(fmax(acc[k], row[k]))
    names = ("sum_e", "sum_mx", "sum_my", "n_wet", "max_e", "max_mx", "max_my")
    out = dict(zip(names, acc))
    out["mean_of_state"] = out["sum_e"] / (float(Nx) * float(Ny))
    return out
