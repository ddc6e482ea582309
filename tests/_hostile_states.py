"""Seeded generators of hostile States for the diagnostics kernel and the copies out of State (tests/test_gpu_diag_hostile.py on
the device, tests/test_aux_references.py on the CPU), and a scalar, cell-by-cell restatement of the coarse wave diagnostics written
from the text of include/picles_hip.h ("THE DEFINITION") that keeps the vectorised tests/_diag_numpy.py honest.  Test
infrastructure: imports nothing from picles_amd/.

Hostile means hostile VALUES: every shape, index and size stays valid."""
from __future__ import annotations

import math

import numpy as np

import _diag_numpy as D

F32_TINY = float(np.finfo(np.float32).tiny)          # smallest normal float32
F32_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------------------------------------------------
# values
# ------------------------------------------------------------------------------------------------------------------------------------
def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _pow2(rng, n, lo, hi):
    """magnitudes 2**U(lo, hi): log-uniform, every binade equally likely"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(rng.uniform(lo, hi, n))


def _nans(rng, n):
    """NaNs with non-default payloads, quiet and signalling, both signs"""
    payload = rng.integers(1, 1 << 51, n, dtype=np.uint64)
    quiet = np.where(rng.random(n) < 0.7, np.uint64(1 << 51), np.uint64(0))
    sign = np.where(rng.random(n) < 0.5, np.uint64(1 << 63), np.uint64(0))
    return (np.uint64(0x7FF0000000000000) | quiet | payload | sign).view(np.float64)


def _sea(rng, n):
    """an ordinary sea: e of order 1e-4 ... 30 m², |m| a few per cent of e, any direction"""
    e = 10.0 ** rng.uniform(-4.0, 1.5, n)
    m = e * rng.uniform(0.02, 0.3, n)
    th = rng.uniform(0.0, 2.0 * math.pi, n)
    return np.stack([e, m * np.cos(th), m * np.sin(th)], axis=1)


WET_KINDS = 9


WET_P = [0.28, 0.12, 0.12, 0.08, 0.08, 0.08, 0.08, 0.08, 0.08]


def _wet(rng, n, kind=None):
    """wet nodes (finite, e > 0, m2 > 0) of every kind the planes can trip over; kind: per node, drawn when not given"""
    v = _sea(rng, n)
    if kind is None:
        kind = rng.choice(WET_KINDS, n, p=WET_P)
    sx, sy = _sign(rng, n), _sign(rng, n)
    def put(k, e=None, mx=None, my=None):
        w = kind == k
        for col, a in ((0, e), (1, mx), (2, my)):
            if a is not None:
                v[w, col] = a[w]
    put(1, e=_pow2(rng, n, -149.0, -127.0))                                       # E in the float32 subnormal range
    put(2, e=_pow2(rng, n, -302.0, -258.0))                                       # hs = 4 sqrt(E) in the float32 subnormal range
    put(3, e=_pow2(rng, n, 128.0, 250.0))                                         # E past FLT_MAX
    put(4, e=_pow2(rng, n, 260.0, 1000.0))                                        # hs past FLT_MAX as well
    put(5, mx=sx * _pow2(rng, n, -400.0, -160.0), my=sy * _pow2(rng, n, -400.0, -160.0))     # m2 tiny but > 0; float32 m is ±0
    put(6, mx=sx * _pow2(rng, n, 513.0, 1000.0), my=sy * _pow2(rng, n, 400.0, 1000.0))       # m2 = inf: wet, M2 = inf
    put(7, e=_pow2(rng, n, 700.0, 1023.9), mx=sx * _pow2(rng, n, 520.0, 1023.9), my=sy * _pow2(rng, n, 520.0, 1023.9))   # inf / inf
    put(8, e=rng.uniform(0.9e308, 1.7e308, n), mx=sx * rng.uniform(0.9e308, 1.7e308, n))     # several of them: Σ overflows
    return v


DRY_KINDS = 9


def _dry(rng, n):
    """nodes that are not wet, one reason each"""
    v = _sea(rng, n)
    kind = rng.integers(0, DRY_KINDS, n)
    col = rng.integers(0, 3, n)
    rows = np.arange(n)
    z = np.where(rng.random((n, 3)) < 0.5, -0.0, 0.0)
    w = kind == 0; v[w] = z[w]                                                    # land: zeros of either sign
    w = kind == 1; v[w, 0] = -v[w, 0]                                             # negative e
    w = kind == 2; v[w, 0] = z[w, 0]                                              # e = ±0 over an ordinary m
    w = kind == 3; v[w, 1:] = (_sign(rng, (n, 2)) * _pow2(rng, (n, 2), -1074.0, -540.0))[w]      # m2 underflows to 0
    w = kind == 4; v[rows[w], col[w]] = _nans(rng, n)[w]                          # a NaN in one plane
    w = kind == 5; v[rows[w], col[w]] = (_sign(rng, n) * np.inf)[w]               # ±Inf in one plane
    w = kind == 6; v[w, 1:] = (_sign(rng, (n, 2)) * 5e-324)[w]                    # the smallest subnormal: its square is 0
    w = kind == 7; v[w] = (_sign(rng, (n, 3)) * _pow2(rng, (n, 3), -1074.0, 1024.0))[w]; v[w, 0] = -np.abs(v[w, 0])   # whole range, e < 0
    w = kind == 8; v[w] = _nans(rng, 3 * n).reshape(n, 3)[w]                      # NaN everywhere
    return v


def _any(rng, n):
    """the per-node mix of a free cell: half an ordinary sea, the rest wet oddities, dry nodes and the whole double range"""
    v = _sea(rng, n)
    k = rng.choice(4, n, p=[0.5, 0.15, 0.2, 0.15])
    w = k == 1; v[w] = _wet(rng, n)[w]
    w = k == 2; v[w] = _dry(rng, n)[w]
    w = k == 3; v[w] = (_sign(rng, (n, 3)) * _pow2(rng, (n, 3), -1074.0, 1024.0))[w]
    return v


# ------------------------------------------------------------------------------------------------------------------------------------
# States
# ------------------------------------------------------------------------------------------------------------------------------------
CELL_FREE, CELL_DRY, CELL_ONE, CELL_TWO, CELL_ALL = range(5)
CELL_P = [0.40, 0.30, 0.10, 0.08, 0.12]


def hostile_state(Nx, ny, cx, cy, seed):
    """[Nx, ny, 3] float64.  Every coarse cell of the (cx, cy) coarsening is given a plan: FREE (the per-node mix), DRY (no wet
    node), ONE and TWO (exactly that many wet nodes among dry ones; half the pairs are m next to -m), ALL (every node wet; one kind
    of wet node per cell).  The
    last tile (256 coarse columns, or the whole row on a narrower grid) of the last coarse row is dry when there are three rows
    or more."""
    rng = np.random.default_rng(seed)
    nxc, nyc = D.coarse_shape(Nx, ny, cx, cy)
    n = Nx * ny
    plan = rng.choice(5, (nxc, nyc), p=CELL_P)
    if nyc >= 3:
        plan[256 * ((nxc - 1) // 256):, nyc - 1] = CELL_DRY
    I, J = np.meshgrid(np.arange(Nx) // cx, np.arange(ny) // cy, indexing="ij")
    node_plan = plan[I, J].reshape(-1)
    cell_id = (I * nyc + J).reshape(-1)
    S = _any(rng, n)
    # the wet nodes of an ALL or TWO cell are of one kind, so that the cell's averages stay where the kind puts them
    cell_kind = rng.choice(WET_KINDS, (nxc, nyc), p=WET_P)[I, J].reshape(-1)
    themed = (node_plan == CELL_ALL) | (node_plan == CELL_TWO)
    dry, wet = _dry(rng, n), _wet(rng, n, np.where(themed, cell_kind, rng.choice(WET_KINDS, n, p=WET_P)))
    w = node_plan != CELL_FREE
    S[w] = dry[w]
    w = node_plan == CELL_ALL
    S[w] = wet[w]
    # ONE / TWO: the wet nodes are the first one / two of a random order of the cell's nodes
    order = np.lexsort((rng.random(n), cell_id))
    sorted_cell = cell_id[order]
    first = np.r_[True, sorted_cell[1:] != sorted_cell[:-1]]
    rank = np.arange(n) - np.maximum.accumulate(np.where(first, np.arange(n), 0))
    rank_of = np.empty(n, dtype=np.int64)
    rank_of[order] = rank
    w = ((node_plan == CELL_ONE) & (rank_of == 0)) | ((node_plan == CELL_TWO) & (rank_of <= 1))
    S[w] = wet[w]
    # half the pairs cancel: the second node carries the first one's m negated (one plane or both), under an e of its own
    second = np.flatnonzero((node_plan == CELL_TWO) & (rank_of == 1))
    first_of = {int(c): int(k) for k, c in zip(np.flatnonzero((node_plan == CELL_TWO) & (rank_of == 0)), cell_id[(node_plan == CELL_TWO) & (rank_of == 0)])}
    for k in second[rng.random(second.size) < 0.5]:
        a = first_of[int(cell_id[k])]
        S[k, 1] = -S[a, 1]
        if rng.random() < 0.5:
            S[k, 2] = -S[a, 2]
    # the dry tile holds nothing above -0.0: negative zeros, NaNs and negative numbers, so that each of its three maxima is the
    # zero fmax keeps — a negative one — and only the x + 0.0 of the definition makes it +0.0
    t = dry_tile_nodes(Nx, ny, cx, cy).reshape(-1)
    if t.any():
        k = rng.choice(3, (int(t.sum()), 3), p=[0.6, 0.2, 0.2])
        S[t] = np.where(k == 0, -0.0, np.where(k == 1, _nans(rng, k.size).reshape(k.shape), -_pow2(rng, k.shape, -1074.0, 1024.0)))
        S[np.flatnonzero(t)[0]] = -0.0                 # however small the tile: a negative zero in every plane
    return np.ascontiguousarray(S.reshape(Nx, ny, 3))


def dry_tile_nodes(Nx, ny, cx, cy):
    """boolean [Nx, ny]: the nodes of the dry tile of hostile_state (none when there are fewer than three coarse rows)"""
    nxc, nyc = D.coarse_shape(Nx, ny, cx, cy)
    I, J = np.meshgrid(np.arange(Nx) // cx, np.arange(ny) // cy, indexing="ij")
    return (I >= 256 * ((nxc - 1) // 256)) & (J == nyc - 1) & (nyc >= 3)


def all_nan_state(Nx, ny, seed):
    return _nans(np.random.default_rng(seed), Nx * ny * 3).reshape(Nx, ny, 3)


def sweep_state(Nx, ny, seed):
    """the large sweep: planes log-uniform over the exponent range in which e, m2 and the float32 planes stay finite (e over
    2^-140 ... 2^100, which takes E and m into the float32 subnormal range; |m| / e over 2^±20, any direction), a band of subnormal
    operands (e subnormal, m2 subnormal), and dry nodes (e = 0) from one in fifty at the left edge to forty-nine in fifty at the
    right, so that the cells of a (4, 4) coarsening divide by every n from 1 to 16"""
    rng = np.random.default_rng(seed)
    n = Nx * ny
    e = _pow2(rng, n, -140.0, 100.0)
    m = e * _pow2(rng, n, -20.0, 20.0)
    band = rng.random(n) < 0.05
    e[band] = _pow2(rng, n, -1074.0, -1022.0)[band]
    m[band] = _pow2(rng, n, -537.0, -511.5)[band]
    th = rng.uniform(0.0, 2.0 * math.pi, n)
    e[rng.random(n) < np.repeat(np.linspace(0.02, 0.98, Nx), ny)] = 0.0
    return np.ascontiguousarray(np.stack([e, m * np.cos(th), m * np.sin(th)], axis=1).reshape(Nx, ny, 3))


# ------------------------------------------------------------------------------------------------------------------------------------
# what a State exercises: counted on the restatement's output, so that a test cannot pass empty
# ------------------------------------------------------------------------------------------------------------------------------------
def classes_of(S, cx, cy, g, r_g):
    (_, _, _, n), _ = D.cell_sums(S, cx, cy)
    f, valid = D.fields_of(S, cx, cy, g, r_g)
    neg_zero = ((f == 0.0) & np.signbit(f)).any(axis=0)
    sub = ((np.abs(f) > 0.0) & (np.abs(f) < np.float32(F32_TINY))).any(axis=0)
    return dict(cells=int(valid.size), valid_share=float(valid.mean()), n0=int((n == 0.0).sum()), n1=int((n == 1.0).sum()),
                valid_nan=int((valid & np.isnan(f).any(axis=0)).sum()), neg_zero=int(neg_zero.sum()), f32_subnormal=int(sub.sum()),
                f32_inf=int(np.isinf(f).any(axis=0).sum()))


CLASS_KEYS = ("n0", "n1", "valid_nan", "neg_zero", "f32_subnormal", "f32_inf")


def assert_classes(c, what):
    """the conditions every mixed case meets: 20 % ... 80 % of the coarse cells valid, and five cells or more of every class"""
    assert 0.2 <= c["valid_share"] <= 0.8, (what, c)
    for k in CLASS_KEYS:
        assert c[k] >= 5, (what, k, c)


# ------------------------------------------------------------------------------------------------------------------------------------
# the scalar restatement: one coarse cell, one tile, one operation at a time, as the header words it
# ------------------------------------------------------------------------------------------------------------------------------------
def _fmax(a, b):
    """fmax as the header means it: a NaN of any kind is skipped"""
    if b != b:
        return a
    if a != a:
        return b
    return a if a >= b else b


def scalar_cell(S, I, J, cx, cy, g, r_g):
    """(the seven float32 planes of cell (I, J), [Σe, Σm_x, Σm_y, n], [max e, max m_x, max m_y]) of S [Nx, ny, 3]"""
    Nx, ny = S.shape[:2]
    f64, zero = np.float64, np.float64(0.0)
    se = sx = sy = n = zero
    xe = xx = xy = f64(-np.inf)
    for j in range(J * cy, min((J + 1) * cy, ny)):            # j outer
        for i in range(I * cx, min((I + 1) * cx, Nx)):        # i inner
            e, mx, my = S[i, j]
            xe, xx, xy = _fmax(xe, e), _fmax(xx, mx), _fmax(xy, my)
            m2 = mx * mx + my * my
            if np.isfinite(e) and np.isfinite(mx) and np.isfinite(my) and e > 0.0 and m2 > 0.0:
                se, sx, sy, n = se + e, sx + mx, sy + my, n + f64(1.0)
    E, MX, MY = se / n, sx / n, sy / n
    M2 = MX * MX + MY * MY
    if n > 0.0 and M2 > 0.0:
        hs = f64(4.0) * np.sqrt(E)
        cg_x = (MX * E) / (f64(2.0) * M2)
        cg_y = (MY * E) / (f64(2.0) * M2)
        cbar = E / (f64(2.0) * np.sqrt(M2))
        tp = (f64(12.566370614359172) * _fmax(cbar / f64(r_g), f64(0.1))) / f64(g)
        planes = [np.float32(x) for x in (hs, tp, cg_x, cg_y, E, MX, MY)]
    else:
        planes = [np.float32(np.nan)] * 7
    return planes, [se, sx, sy, n], [xe, xx, xy]


def scalar_diag(S, cx, cy, g, r_g):
    """fields [7, Nxc, nyc] float32 and partials [nyc tiles_per_row, 7] of the whole State, cell by cell and tile by tile"""
    Nx, ny = S.shape[:2]
    nxc, nyc = D.coarse_shape(Nx, ny, cx, cy)
    tpr = -(-nxc // 256)
    fields = np.empty((7, nxc, nyc), dtype=np.float32)
    partials = np.empty((nyc * tpr, 7))
    with np.errstate(all="ignore"):
        for J in range(nyc):
            for T in range(tpr):
                lanes = [[np.float64(0.0)] * 4 + [np.float64(-np.inf)] * 3 for _ in range(256)]
                for l in range(256):
                    I = 256 * T + l
                    if I < nxc:
                        p, sums, maxs = scalar_cell(S, I, J, cx, cy, g, r_g)
                        fields[:, I, J] = p
                        lanes[l] = sums + maxs
                for q in range(7):
                    op = (lambda a, b: a + b) if q < 4 else _fmax
                    groups = []
                    for w in range(4):
                        v = [lanes[64 * w + l][q] for l in range(64)]
                        s = 32
                        while s >= 1:
                            for l in range(s):
                                v[l] = op(v[l], v[l + s])
                            s //= 2
                        groups.append(v[0])
                    a = op(op(op(groups[0], groups[1]), groups[2]), groups[3])
                    partials[J * tpr + T, q] = a if q < 4 else a + np.float64(0.0)
    return fields, partials
