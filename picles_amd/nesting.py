"""NestForcing: one-way nesting — a fine child box forced at its open rim by a coarser parent model that runs beside it, all on
the device.  The parent's State is sampled behind its step at the corner nodes that surround the child's forced nodes, mixed onto
them with the station definition of picles_amd/station_output.py and written into the level block of the child's forcing set in
stream order (picles_nest_*, include/picles_hip.h "one-way nesting"; the mix kernel is picles_amd/csrc/k_nest.h).  Nothing crosses
PCIe, the host waits for nothing, and both models stay on `picles_run_steps`.

Attach in the place of a BoundaryForcing (picles_amd/boundary_forcing.py):

    child_sim.output_writers["boundary_forcing"] = NestForcing(child_model, parent=parent_sim, side="rim", ratio=3)
    run(child_sim)

`run(child_sim)` drives both: the parent takes one step of `parent_sim.Δt` for every `ratio` steps of the child and stays one
step ahead of it, so that the child always steps between two parent levels.  The value a child step sees is BoundaryForcing's —
linear in t between the levels that bracket the step's start time, the later pair at a level itself; the window logic is that
class's own (`window_of`, `steps_allowed`), applied to the parent's clock values.  The parent's FieldWriter, StationWriter and
StatisticsWriter are driven through their hooks as run(parent_sim) would drive them, one step per chunk.

GEOMETRY.  The child's forced nodes are located in the parent from the child grid's own node coordinates with
`station_output.locate_points` (a node outside the parent is its ValueError); the distinct corner nodes are found on the host.
TIME.  `ratio` is an integer r >= 1 with |r Δt_child - Δt_parent| <= 1e-12 Δt_parent, and both clocks agree when the run begins.

THE OFFLINE ROUTE gives the same bits: run the parent alone with `StationWriter(points=rim_points(child_model, side=...))`, then the
child under `boundary_forcing.from_station_output(child_model, path, side=...)`.

TWO-WAY (`feedback=True`).  The parent learns what the child resolved: its ocean nodes under the child, a margin
inside the child's band, become a forcing set of the parent whose one level is the child's State restricted onto them
(`restriction_stencil`, `restrict_records`; picles_nest_feedback_*, the kernel is k_nest_restrict in picles_amd/csrc/k_nest.h).  A
feedback is taken exactly when a parent step is taken, with both clocks equal, in front of that step.  Not for a parent that carries a
BoundaryForcing of its own.

RESTART.  A Checkpointer in the CHILD's output_writers checkpoints the pair: next to every child file the parent's
file at the parent's own clock — t1 of the pair of levels the child holds; between two levels the parent is a step ahead —
(`parent_checkpoint_path`, loadable on its own) and the pair itself with the counters and a hash of the geometry (`link_path`,
`<child file>.nest.npz`), the link last.  `run(child_sim, pickup=True)` takes the latest child iteration whose three files are
complete (`pickup=<path>` names the child's file), loads both models, makes the set and the nest and puts the pair back
(picles_nest_set_levels) without a seed sample or a seed feedback; the ordinary loop follows, and both models continue with the bits
of the uninterrupted run.  A Checkpointer on the parent stays refused, and so does a backend without nest_set_levels.

Not for slabs, and only where run() takes its chunked path on both models: no `store`, no `cash_store`, and winds that are static or a
GriddedWinds lattice the device samples itself (`WaveGrowth2D.runs_chunked`).  Either model, or both, may run under a lattice, the
same object or different ones: each context samples its own copy at its own node coordinates, in stream order on its own stream,
so a level taken from the parent and a step of the child see the winds their clocks name.  Wind closures that vary in time are
sampled by the host in front of every step and stay refused.

A CHILD SWITCHED ON LATE (`start_from_parent(child_sim, parent_sim)`).  A hindcast spins the parent up alone and
switches the child on when the storm nears: the parent's State at its clock t is prolonged onto every node of the child on the
device (`prolong_state` is the definition, picles_nest_prolong the call, k_nest_prolong in picles_amd/csrc/k_nest.h the kernel),
the child's particles are remeshed from it under the child's wind at t, and both clocks read t: `run(child_sim)` with a
NestForcing then proceeds as from a common cold start.

A CHILD THAT FOLLOWS THE STORM (`move_child`, `run_following`).  Between two legs of `run(child_sim)` the child's box is
translated by whole child nodes (`grids.translated`): where the old and the new box overlap the child keeps the sea it resolved, the
freshly exposed nodes take the parent's State prolonged (`relocate_state` is the definition, picles_nest_relocate the call,
k_nest_relocate the kernel), and the particles are remade under the wind at the new nodes.  `run_following` runs legs under a fresh
NestForcing each and moves the box behind every leg so that its centre follows a track.  An open Cartesian box without land, under
static winds or a device-sampled lattice; restart of `run_following` itself is not carried.
"""
from __future__ import annotations

import hashlib
import math
import os
import re
from pathlib import Path

import numpy as np

from ._capi import CheckpointError
from .boundary_forcing import BoundaryForcing, node_points, rim_nodes
from .checkpointing import _HEAD, load_checkpoint, write_checkpoint_file
from .output_writers import PHASE_ORDER, in_phase, writers_of
from .station_output import _axis, _kind, locate_points, wet_means

RATIO_EPS = 1e-12          # |r Δt_child - Δt_parent| may be this fraction of Δt_parent
LINK_SUFFIX = ".nest.npz"   # the link side-car of a pair checkpoint, next to the child's file


def parent_checkpoint_path(child_file):
    """the parent's file of a pair checkpoint, next to the child's `{prefix}_iteration{i}.picles`: `{prefix}_parent_iteration{i}.picles`
    (a name `list_checkpoints(dir, prefix)` does not match); a child file of another name gets `<stem>_parent<suffix>`"""
    f = Path(child_file)
    m = re.fullmatch(r"(.*)_iteration(\d+)(\.[^.]+)", f.name)
    return f.with_name(f"{m.group(1)}_parent_iteration{m.group(2)}{m.group(3)}" if m else f"{f.stem}_parent{f.suffix}")


def link_path(child_file):
    """the link side-car of a pair checkpoint: `<child file>.nest.npz`"""
    return Path(str(child_file) + LINK_SUFFIX)


def _write_link(path, **arrays):
    """atomic, like the checkpoint files: temporary name, flush + fsync, rename"""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(f".{path.name}.tmp-{os.getpid()}")
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **arrays)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    return path


def rim_points(model, side=None, *, nodes=None, width=1):
    """the (x, y) of a model's forced nodes, in the order of its forcing set: the `points` of the StationWriter that records, in a
    parent run, what a NestForcing would hand the model (width > 1: the band of boundary_forcing.band_nodes)"""
    if (nodes is None) == (side is None):
        raise ValueError("rim_points needs either nodes=[(i, j), ...] or side=...")
    return node_points(model.grid, rim_nodes(model.grid, side, width) if nodes is None else nodes)


def locate_in_parent(parent_grid, points):
    """(corner_nodes int64 [n_corner, 2] distinct, index int64 [n, 4] into them, weights float64 [n, 4]) of points in the parent"""
    corners, weights = locate_points(parent_grid, points)
    corner_nodes, inv = np.unique(corners.reshape(-1, 2), axis=0, return_inverse=True)
    return corner_nodes, np.asarray(inv).reshape(corners.shape[:2]), weights


SNAP = 1e-9               # a child node closer to a parent node, or to the end of its hat, than this fraction of a parent cell is on it


def _axis_hat(pc, cc, D):
    """per parent coordinate pc[k] the child coordinates inside its hat (|cc - pc| < D): (index int64 [n, mx], weight [n, mx]),
    ascending in the child index, padded with weight 0.0; w = 1 - |cc - pc| / D from the coordinates alone"""
    t = np.abs(np.asarray(cc, dtype=np.float64)[None, :] - np.asarray(pc, dtype=np.float64)[:, None]) / np.float64(D)
    t = np.where(t < SNAP, 0.0, np.where(t > 1.0 - SNAP, 1.0, t))
    w = np.maximum(0.0, 1.0 - t)
    mx = max(int((w > 0.0).sum(axis=1).max(initial=0)), 1)
    order = np.argsort(w == 0.0, axis=1, kind="stable")[:, :mx]          # the entries of the hat first, in child order
    return order, np.take_along_axis(w, order, axis=1)


def restriction_stencil(parent_grid, child_grid, margin=1):
    """(fb_nodes int64 [n_fb, 2], src_nodes int64 [n_src, 2], index int64 [n_fb, m], weight float64 [n_fb, m]) of a two-way nest.

    The feedback nodes are the parent's ocean nodes (mask class 1) whose one-cell neighbourhood lies inside the child's grid and
    which lie at least `margin` parent cells inside the child's outermost nodes, row by row, i fastest.  The weights are the
    adjoint of the bilinear interpolation the child's rim uses: for a child node at (xc, yc) and a parent node at (xp, yp),
    w = max(0, 1 - |xc - xp| / Dx) max(0, 1 - |yc - yp| / Dy), from the coordinates alone (a distance within 1e-9 of a cell of 0 or
    of Dx is that).  Per node the entries with w > 0, in row order of the child, i fastest, padded to m with weight 0.0 (the
    padding repeats the node's first index); src_nodes are the distinct child nodes used, in row order, and index points into them.
    A child at the parent's spacing gives m = 1 with weight 1.0 (injection), an aligned child at spacing ratio rs (2 rs - 1)²."""
    if not (isinstance(margin, (int, np.integer)) and margin >= 0):
        raise ValueError(f"restriction_stencil: margin must be an integer >= 0, not {margin!r}")
    px, py = np.asarray(parent_grid.data.x)[:, 0], np.asarray(parent_grid.data.y)[0, :]
    cx, cy = np.asarray(child_grid.data.x)[:, 0], np.asarray(child_grid.data.y)[0, :]
    Dx, Dy = float(parent_grid.stats.dx), float(parent_grid.stats.dy)
    reach = max(int(margin), 1)
    okx = (px - reach * Dx >= cx[0] - SNAP * Dx) & (px + reach * Dx <= cx[-1] + SNAP * Dx)
    oky = (py - reach * Dy >= cy[0] - SNAP * Dy) & (py + reach * Dy <= cy[-1] + SNAP * Dy)
    keep = okx[:, None] & oky[None, :] & (np.asarray(parent_grid.data.mask) == 1)
    j, i = np.nonzero(keep.T)                     # rows in order, i fastest within a row
    fb_nodes = np.stack([i, j], axis=1).astype(np.int64)
    if len(fb_nodes) == 0:
        return fb_nodes, np.zeros((0, 2), dtype=np.int64), np.zeros((0, 1), dtype=np.int64), np.zeros((0, 1))
    ix, wx = _axis_hat(px, cx, Dx)
    iy, wy = _axis_hat(py, cy, Dy)
    # entry (b, a) of node (i, j): child node (ix[i, a], iy[j, b]), a fastest — the child's row order
    ci = np.repeat(ix[i][:, None, :], iy.shape[1], axis=1).reshape(len(i), -1)
    cj = np.repeat(iy[j][:, :, None], ix.shape[1], axis=2).reshape(len(i), -1)
    w = (wy[j][:, :, None] * wx[i][:, None, :]).reshape(len(i), -1)
    m = int((w > 0.0).sum(axis=1).max())
    order = np.argsort(w == 0.0, axis=1, kind="stable")[:, :m]
    ci, cj, w = (np.take_along_axis(a, order, axis=1) for a in (ci, cj, w))
    ci, cj = np.where(w > 0.0, ci, ci[:, :1]), np.where(w > 0.0, cj, cj[:, :1])
    Ncx = len(cx)
    flat, inv = np.unique(cj * Ncx + ci, return_inverse=True)
    src_nodes = np.stack([flat % Ncx, flat // Ncx], axis=1).astype(np.int64)
    return fb_nodes, src_nodes, np.asarray(inv).reshape(ci.shape).astype(np.int64), np.ascontiguousarray(w)


def restrict_records(values, index, weight):
    """k_nest_restrict in NumPy, bit for bit: values float64 [n_src, 3] (e, m_x, m_y of the source nodes), index int [n_fb, m]
    into them, weight [n_fb, m] -> float64 [n_fb, 3], NaN rows where no entry is wet.  The station definition of
    picles_amd/station_output.py (wet_means) over m entries in order; an entry whose weight is 0.0 is padding: it adds no bit"""
    v = np.asarray(values, dtype=np.float64).reshape(-1, 3)
    E, MX, MY, valid = wet_means(v.T, np.asarray(index, dtype=np.int64), np.asarray(weight, dtype=np.float64))
    out = np.stack([E, MX, MY], axis=1)
    out[~valid] = np.nan
    return out


def prolong_tables(parent_grid, child_grid):
    """(ix0, ix1 int32 [Ncx], wx float64 [Ncx], iy0, iy1 int32 [Ncy], wy float64 [Ncy]): per child column and per child row the two
    parent columns / rows around it and the weight of the second — `station_output._axis` of the child's node coordinates on the
    parent's axes, which is what `locate_points(parent_grid, [(x, y)])` does per point: the bilinear stencil is separable.  The
    tables picles_nest_prolong takes.  A child node outside the parent is locate_points' ValueError"""
    xs, ys = np.asarray(parent_grid.data.x)[:, 0], np.asarray(parent_grid.data.y)[0, :]
    cx, cy = np.asarray(child_grid.data.x)[:, 0], np.asarray(child_grid.data.y)[0, :]
    out = []
    for pc, cc, N, what in ((xs, cx, parent_grid.stats.Nx, "x"), (ys, cy, parent_grid.stats.Ny, "y")):
        rows = [_axis(float(c), float(pc[0]), float(pc[-1]), int(N), _kind(N), what) for c in cc]
        out += [np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32),
                np.array([r[2] for r in rows], dtype=np.float64)]
    return tuple(out)


def prolong_state(S_parent, parent_grid, child_grid):
    """k_nest_prolong in NumPy, bit for bit: the parent's State float64 [Npx, Npy, 3] onto every node of the child -> float64
    [Ncx, Ncy, 3].  Per child node the four parent corners in locate_points' visiting order with its weights (1-wx)(1-wy),
    wx(1-wy), (1-wx)wy, wx wy, and over them the station definition (wet_means); a node that is not valid — no wet corner, or zero
    momentum — is (0, 0, 0): a calm node, whose particle the remesh makes from the local wind.  No case depends on a mask"""
    S = np.asarray(S_parent, dtype=np.float64)
    ix0, ix1, wx, iy0, iy1, wy = prolong_tables(parent_grid, child_grid)
    Npx = S.shape[0]
    ncx, ncy = len(wx), len(wy)
    gx, gy = 1.0 - wx, 1.0 - wy
    I0, I1, J0, J1 = (a.astype(np.int64) for a in (ix0[:, None], ix1[:, None], iy0[None, :], iy1[None, :]))
    index = np.stack([J0 * Npx + I0, J0 * Npx + I1, J1 * Npx + I0, J1 * Npx + I1], axis=-1).reshape(ncx * ncy, 4)
    weight = np.stack([gx[:, None] * gy[None, :], wx[:, None] * gy[None, :], gx[:, None] * wy[None, :], wx[:, None] * wy[None, :]],
                      axis=-1).reshape(ncx * ncy, 4)
    values = S.reshape(-1, 3, order="F").T                  # [3, n_nodes], node j Npx + i
    E, MX, MY, valid = wet_means(values, index, weight)
    out = np.where(valid[:, None], np.stack([E, MX, MY], axis=1), 0.0)
    return out.reshape(ncx, ncy, 3)


def start_from_parent(child_sim, parent_sim):
    """A child started from its spun-up parent, before `run(child_sim)`: the parent has been run to some clock t; afterwards the
    child's State is the parent's prolonged onto the child's nodes (`prolong_state`), its particles are what the library's remesh
    makes of that State under the child's wind at t with the step `child_sim.Δt` and fresh controller memory, the library's clock
    for the child is t, `child.clock.time = t`, `child.clock.iteration = 0` and `child_sim.initialized` is true: `run(child_sim)`
    with a `NestForcing(parent=parent_sim, ...)` finds equal clocks and proceeds.  All on the device (picles_nest_prolong,
    DESIGN.md §23).  The child's winds are static or a lattice the device samples; the parent's pending step is completed.
    A run begun this way is checkpointed and picked up like any nested pair: the picked-up program builds both
    models and calls `run(child_sim, pickup=...)` — neither the spin-up nor this call is repeated."""
    cm, pm = child_sim.model, parent_sim.model
    if type(cm).__name__ == "SlabModel" or type(pm).__name__ == "SlabModel":
        raise NotImplementedError("start_from_parent: slabs do not nest: use whole-grid models")
    if cm is pm:
        raise ValueError("start_from_parent: the parent must be another model")
    if not parent_sim.initialized:
        raise ValueError("start_from_parent: the parent was never run: it holds no sea state to start a child from "
                         "(run(parent_sim) to the clock at which the child is switched on first)")
    if not cm.runs_chunked(child_sim.Δt, detect=True):
        raise NotImplementedError(f"start_from_parent: the child's wind closures vary in time: {WINDS_REFUSAL}")
    tables = prolong_tables(pm.grid, cm.grid)             # a child node outside the parent: ValueError, nothing touched
    if not hasattr(cm.backend, "nest_prolong"):
        raise NotImplementedError("start_from_parent needs a backend with nest_prolong (the HIP library, ABI 15)")
    t = float(pm.clock.time)
    cm._wind_window = None
    cm.upload_winds(t, child_sim.Δt, seeding=True)        # static: the level at t; a lattice: uploaded once, sampled by the library at t
    cm.backend.nest_prolong(pm.backend, *tables, float(child_sim.Δt))
    st = getattr(cm, "_state", None)
    if st is not None:
        st.after_step()                  # the device field was replaced: no host mirror, no recorded write survives the start
    cm.clock.time, cm.clock.iteration = t, 0
    child_sim.initialized = True
    child_sim.running = False


def _whole_shift(shift, keep_margin, who):
    si, sj = shift
    for v in (si, sj):
        if not isinstance(v, (int, np.integer)):
            raise ValueError(f"{who}: the shift is whole child nodes (si, sj), not {shift!r}")
    if not (isinstance(keep_margin, (int, np.integer)) and keep_margin >= 0):
        raise ValueError(f"{who}: keep_margin must be an integer >= 0, not {keep_margin!r}")
    return int(si), int(sj), int(keep_margin)


def kept_box(shape, shift, keep_margin):
    """the new nodes that keep the child's own State under a move by `shift` = (si, sj): (i0, i1, j0, j1), the half-open ranges of
    new i and j with keep_margin <= i + si < Ncx - keep_margin and likewise in j (empty ranges have i1 == i0): kx ky nodes,
    kx = max(0, Ncx - max(m, si) - max(m, -si))"""
    (ncx, ncy), (si, sj), m = shape, shift, keep_margin
    i0, j0 = max(0, m - si), max(0, m - sj)
    return i0, max(i0, min(ncx, ncx - m - si)), j0, max(j0, min(ncy, ncy - m - sj))


def relocate_state(S_child, S_parent, parent_grid, new_child_grid, shift, keep_margin):
    """k_nest_relocate in NumPy, bit for bit: the State of a child whose box has been translated by `shift` = (si, sj) of its own
    nodes, so that new node (i, j) lies where old node (i + si, j + sj) lay.  S_child float64 [Ncx, Ncy, 3] is the child's State
    before the move, `new_child_grid` the translated grid (`grids.translated`).  Where keep_margin <= i + si < Ncx - keep_margin and
    keep_margin <= j + sj < Ncy - keep_margin the new node takes the bits of S_child[i + si, j + sj] as they stand, calm (0, 0, 0)
    nodes and NaN payloads included; any other node takes `prolong_state(S_parent, parent_grid, new_child_grid)[i, j]`.
    keep_margin drops the old box's rim and band, whose State is prescribed rather than resolved"""
    si, sj, m = _whole_shift(shift, keep_margin, "relocate_state")
    Sc = np.ascontiguousarray(S_child, dtype=np.float64)
    out = prolong_state(S_parent, parent_grid, new_child_grid)
    if Sc.shape != out.shape:
        raise ValueError(f"relocate_state: the child's State is {Sc.shape}, the new grid's {out.shape}: a move keeps the box's shape")
    i0, i1, j0, j1 = kept_box(Sc.shape[:2], (si, sj), m)
    if i1 > i0 and j1 > j0:
        out.view(np.uint64)[i0:i1, j0:j1] = Sc.view(np.uint64)[i0 + si:i1 + si, j0 + sj:j1 + sj]
    return out


def move_child(child_sim, parent_sim, shift, keep_margin=None):
    """A child box moved across its parent, between two legs of `run(child_sim)` (a vortex-following nest): the box
    is translated by `shift` = (si, sj) whole child nodes.  Where the old and the new box overlap, `keep_margin` nodes inside the old
    one, the child keeps the sea it resolved; the freshly exposed nodes take the parent's State prolonged (`relocate_state` is the
    definition, picles_nest_relocate the call, k_nest_relocate in picles_amd/csrc/k_nest.h the kernel: nothing crosses PCIe).  The
    particles are remade from that State under the child's wind at the new nodes with fresh controller memory.  Afterwards
    `child.grid` is the translated grid (`grids.translated`); clock time and iteration are kept.
    keep_margin: default the `width` of the NestForcing still in child_sim.output_writers, at least 1.
    The leg before must have ended (NestForcing.finish frees the link), both clocks must agree, and the child is an open Cartesian
    box without land under static winds or a lattice the device samples.  A new box that leaves the parent is prolong_tables'
    ValueError; like every refusal here it comes before anything is touched.
    A NestForcing holds geometry from its constructor: THE NEXT LEG TAKES A NEW ONE, built after the move.  Writers that carry node
    coordinates (FieldWriter and its kin) keep those of their construction: point them at a per-leg path.  Not carried across a
    move: statistics accumulators, a track table, StreamedWinds, a checkpoint's origin."""
    from .grids import TwoDCartesianGridMesh, translated
    cm, pm = child_sim.model, parent_sim.model
    if type(cm).__name__ == "SlabModel" or type(pm).__name__ == "SlabModel":
        raise NotImplementedError("move_child: slabs do not nest: use whole-grid models")
    if cm is pm:
        raise ValueError("move_child: the parent must be another model")
    if not parent_sim.initialized or not child_sim.initialized:
        raise ValueError("move_child: both models must have been run: a box moves between two legs of a nested run")
    if keep_margin is None:
        f = getattr(child_sim, "output_writers", {}).get("boundary_forcing")
        keep_margin = max(1, int(getattr(f, "width", 1)))
    si, sj, m = _whole_shift(shift, keep_margin, "move_child")
    from .coupling import StreamedWinds
    if isinstance(getattr(cm, "winds", None), StreamedWinds):
        raise NotImplementedError("move_child: the child runs under StreamedWinds: a streamed child does not move")
    if not cm.runs_chunked(child_sim.Δt, detect=True):
        raise NotImplementedError(f"move_child: the child's wind closures vary in time: {WINDS_REFUSAL}")
    if not isinstance(cm.grid, TwoDCartesianGridMesh):
        raise NotImplementedError("move_child: only a child on a Cartesian grid moves (no spherical child)")
    if float(cm.clock.time) != float(pm.clock.time):
        raise ValueError(f"move_child: the child's clock ({cm.clock.time!r}) and the parent's ({pm.clock.time!r}) differ: a box moves "
                         "between two legs, on a common clock")
    new_grid = translated(cm.grid, si, sj)                 # land or a periodic axis: NotImplementedError, nothing touched
    tables = prolong_tables(pm.grid, new_grid)             # a node of the new box outside the parent: ValueError, nothing touched
    if not hasattr(cm.backend, "nest_relocate"):
        raise NotImplementedError("move_child needs a backend with nest_relocate (the HIP library, ABI 18)")
    t, dt = float(cm.clock.time), float(child_sim.Δt)
    old_grid = cm.grid
    lattice = cm._wind_window == "device-lattice"
    cm.grid = new_grid
    try:
        if not lattice:
            cm._wind_window = None
            cm.upload_winds(t, dt, seeding=True)           # static: the level at the new nodes; a lattice stays on the device
        cm.backend.nest_relocate(pm.backend, si, sj, m, *tables, dt, float(new_grid.data.x[0, 0]), float(new_grid.data.y[0, 0]))
    except BaseException:
        cm.grid = old_grid
        if not lattice:
            cm._wind_window = None
            cm.upload_winds(t, dt, seeding=True)           # the winds of the old nodes again
        raise
    st = getattr(cm, "_state", None)
    if st is not None:
        st.after_step()                  # the device field was replaced: no host mirror, no recorded write survives the move
    child_sim.running = False


def _box_shift(child_grid, parent_grid, target, snap):
    """the whole-node shift (si, sj) that brings the centre of the child's box closest to `target` = (x, y): rounded to whole child
    nodes, or (snap="parent") to whole parent cells; clamped on every non-periodic parent axis so that all child nodes stay inside"""
    out = []
    cs, ps = child_grid.stats, parent_grid.stats
    for c, lo, hi, d, D, N, plo, phi, what in ((target[0], cs.xmin, cs.xmax, cs.dx, ps.dx, ps.Nx, ps.xmin, ps.xmax, "x"),
                                               (target[1], cs.ymin, cs.ymax, cs.dy, ps.dy, ps.Ny, ps.ymin, ps.ymax, "y")):
        unit = 1
        if snap == "parent":
            unit = int(round(D / d))
            if unit < 1 or abs(unit * d - D) > 1e-9 * D:
                raise ValueError(f"run_following: snap='parent' needs a parent spacing that is a whole multiple of the child's; in {what} "
                                 f"they are {D!r} and {d!r}")
        s = int(round((float(c) - 0.5 * (lo + hi)) / (unit * d))) * unit
        if _kind(N) == "open":
            smin = -int(math.floor((lo - plo) / d + 1e-9))           # the shifts that keep [lo, hi] inside [plo, phi]
            smax = int(math.floor((phi - hi) / d + 1e-9))
            smin, smax = -((-smin) // unit) * unit, (smax // unit) * unit
            s = min(max(s, smin), smax)
        out.append(s)
    return tuple(out)


def run_following(child_sim, parent_sim, centre, *, stop_time, nest, every=1, snap="child", keep_margin=None, on_leg=None):
    """A nested run whose child box follows `centre(t) -> (x, y)` — a storm's wind maximum, a best-track position — across the
    parent.  The run is a sequence of LEGS of `every` parent steps: each leg is `run(child_sim)` under a fresh
    `NestForcing(child_model, parent=parent_sim, **nest)` (`nest` names at least `ratio` and `side` or `nodes`; `feedback=True` with
    snap="parent" keeps an aligned two-way child aligned), with `child_sim.stop_time` set so that run() takes `every * ratio` child
    steps; legs are run until the child's clock has reached `stop_time` (whole legs: the last one may end behind it).  After a leg,
    at the common clock t, the box centre goes to `centre(t)` rounded to whole child nodes (snap="child") or whole parent cells
    (snap="parent"), clamped on a non-periodic parent axis so that every child node stays inside the parent (a periodic axis does
    not wrap a box: leaving the period is move_child's ValueError); a zero shift calls nothing, any other `move_child`.
    keep_margin: move_child's, default max(1, nest["width"]).
    on_leg(k, child_sim) runs in front of leg k = 0, 1, ...: point FieldWriter and similar writers of either model at a per-leg path
    there — their files carry the coordinates of their construction, and every leg begins them anew.
    Returns [(t, x0, y0), ...]: the box origin (node (0, 0)) at the start and behind every leg.
    The child must be started (`start_from_parent`, or a common cold start: both clocks equal).  RESTART inside run_following is
    not carried: a Checkpointer in a leg writes pair checkpoints as in any nested run, and a checkpoint is picked up by a program
    that builds the child at THAT LEG's origin and runs on from there — the link side-car's geometry hash refuses any other origin."""
    from .simulations import run
    if snap not in ("child", "parent"):
        raise ValueError(f"run_following: snap must be 'child' or 'parent', not {snap!r}")
    if not (isinstance(every, (int, np.integer)) and every >= 1):
        raise ValueError(f"run_following: every must be an integer >= 1, not {every!r}")
    if "ratio" not in nest:
        raise ValueError("run_following: nest=dict(ratio=r, side=... | nodes=..., ...) must name the ratio")
    cm, pm = child_sim.model, parent_sim.model
    ratio = _whole(nest["ratio"])
    m = max(1, int(nest.get("width", 1))) if keep_margin is None else keep_margin
    dt = float(child_sim.Δt)
    n = int(every) * ratio
    origin = lambda: (float(cm.clock.time), float(cm.grid.data.x[0, 0]), float(cm.grid.data.y[0, 0]))
    boxes = [origin()]
    k = 0
    while cm.clock.time < stop_time - 1e-9 * dt:
        if on_leg is not None:
            on_leg(k, child_sim)
        child_sim.output_writers["boundary_forcing"] = NestForcing(cm, parent=parent_sim, **nest)
        child_sim.stop_time = float(cm.clock.time) + (n - 0.5) * dt          # run() steps while stop_time >= clock.time: n steps
        run(child_sim)
        shift = _box_shift(cm.grid, pm.grid, centre(float(cm.clock.time)), snap)
        if shift != (0, 0):
            move_child(child_sim, parent_sim, shift, keep_margin=m)
        boxes.append(origin())
        k += 1
    return boxes


def default_feedback_margin(width, dx_child, dx_parent):
    """1 + ceil(width dx_child / dx_parent) parent cells: no node of the child's band is among the sources"""
    return 1 + int(math.ceil(float(width) * float(dx_child) / float(dx_parent) - 1e-12))


def _whole(ratio):
    if not (isinstance(ratio, (int, float, np.integer, np.floating)) and ratio == int(ratio) and ratio >= 1):
        raise ValueError(f"NestForcing: ratio must be an integer >= 1, not {ratio!r}")
    return int(ratio)


def check_ratio(ratio, dt_child, dt_parent):
    r = _whole(ratio)
    if not abs(r * dt_child - dt_parent) <= RATIO_EPS * dt_parent:
        raise ValueError(f"NestForcing: {r} child steps of {dt_child!r} s do not make one parent step of {dt_parent!r} s")
    return r


def _chunked(model, dt):
    """would run() take picles_run_steps on this model?  (WaveGrowth2D.runs_chunked: time-constant winds, or a lattice the device
    samples itself; evaluated on the host, nothing is uploaded)"""
    return hasattr(model.backend, "run_steps") and bool(model.runs_chunked(dt, detect=True))


WINDS_REFUSAL = ("a nest needs static winds on both models, or a GriddedWinds lattice on a backend that samples it on the device "
                 "(set_wind_grid)")


class NestForcing(BoundaryForcing):
    """NestForcing(child_model, parent=<Simulation>, nodes=[(i, j), ...] | side="west" | ... | "rim", ratio=r, Δt=None, width=1,
    weights=None | "linear" | array(n), feedback=False, feedback_margin=None)
    feedback=True: two-way — the child's State is restricted onto the parent's ocean nodes under it, feedback_margin parent cells
    inside the child's outermost nodes (default 1 + ceil(width dx_child / dx_parent): no band node of the child is fed back)
    Δt: the child's step, where it is not parent.Δt / ratio to the last bit; width, weights: BoundaryForcing's — a band as deep as
    the parent's fastest swell travels in a child step lets it enter"""

    kind = "boundary_forcing"
    needs = "nest_init"
    refusal = "a NestForcing needs a backend with nest_init / nest_sample (the HIP library)"

    FEEDBACK_REFUSAL = "a NestForcing with feedback=True needs a backend with nest_feedback_init / nest_feedback (the HIP library, ABI 13)"

    def __init__(self, model, *, parent, nodes=None, side=None, ratio=1, Δt=None, width=1, weights=None, feedback=False, feedback_margin=None):
        if type(model).__name__ == "SlabModel" or type(parent.model).__name__ == "SlabModel":
            raise NotImplementedError("NestForcing: slabs do not nest: use whole-grid models")
        if (nodes is None) == (side is None):
            raise ValueError("NestForcing needs either nodes=[(i, j), ...] or side=...")
        if parent.model is model:
            raise ValueError("NestForcing: the parent must be another model")
        self.model, self.parent = model, parent
        self._take_nodes(model, nodes, side, width, weights)
        self.dt = float(parent.Δt) / _whole(ratio) if Δt is None else float(Δt)
        self.ratio = check_ratio(ratio, self.dt, float(parent.Δt))
        self.corner_nodes, self.index, self.weights = locate_in_parent(parent.model.grid, node_points(model.grid, self.nodes))
        self.feedback = bool(feedback)
        self.feedbacks = 0            # levels handed to the parent
        self._fb_on = None
        if self.feedback:
            self.needs, self.refusal = "nest_feedback_init", self.FEEDBACK_REFUSAL
            pg, cg = parent.model.grid, model.grid
            self.feedback_margin = (default_feedback_margin(self.width, cg.stats.dx, pg.stats.dx) if feedback_margin is None
                                    else feedback_margin)
            self.fb_nodes, self.src_nodes, self.fb_index, self.fb_weights = restriction_stencil(pg, cg, self.feedback_margin)
            if len(self.fb_nodes) == 0:
                raise ValueError(f"NestForcing: feedback=True, but no ocean node of the parent lies {self.feedback_margin} parent cell(s) "
                                 "inside the child: a larger child or a smaller feedback_margin is needed")
        self.times = np.zeros(0)      # the parent's clock at every level taken, and behind them the time of the level to come
        self.values = None
        self.uploads = 0              # levels taken from the parent
        self.parent_steps = 0
        self._have = -1               # index into times of the latest level the library holds
        self._set_on = None
        self._k = None
        self._mark = None
        self._pair = None             # the pair checkpoint whose parent blob is being copied out: (parent file, link file, clock, iteration, link)
        self._link = None             # the link side-car check_pickup read
        self._resume = None           # ... handed to begin_run by load_pickup: the run resumes instead of starting cold
        self.pairs_written = []       # the child files whose companions were completed

    def geometry_hash(self):
        """what a link side-car is held against: the forcing set's nodes and weights, the corner geometry and, two-way, the feedback's"""
        h = hashlib.sha256()
        parts = [self.nodes, np.zeros(0) if self.node_weights is None else self.node_weights, self.corner_nodes, self.index, self.weights]
        if self.feedback:
            parts += [self.fb_nodes, self.src_nodes, self.fb_index, self.fb_weights]
        for a in parts:
            a = np.ascontiguousarray(a)
            h.update(f"{a.dtype.str}{a.shape}".encode())
            h.update(a.tobytes())
        return h.hexdigest()

    # ---- before anything is seeded ----
    def check_run(self, sim, writers, store=False, cash_store=False, pickup=False):
        super().check_run(sim, writers, store=store, cash_store=cash_store, pickup=pickup)
        from .coupling import StreamedWinds
        if any(isinstance(getattr(mm, "winds", None), StreamedWinds) for mm in (sim.model, self.parent.model)):
            raise NotImplementedError("NestForcing: the child or the parent runs under StreamedWinds: streamed nests are not carried "
                                      "(a GriddedWinds lattice or static winds on both models)")
        pw = writers_of(self.parent)
        if any(w.kind == "checkpointer" for w in pw):
            raise NotImplementedError("NestForcing: a Checkpointer in the parent's output_writers: a nested pair is checkpointed through the "
                                      "child's Checkpointer, which writes the parent's file next to the child's")
        ck = any(w.kind == "checkpointer" for w in writers)
        if ck or pickup:
            b, pb = sim.model.backend, self.parent.model.backend
            if not (hasattr(b, "nest_set_levels") and hasattr(pb, "checkpoint_begin") and hasattr(pb, "checkpoint_load")):
                raise NotImplementedError("NestForcing: " + " and ".join((["a Checkpointer is attached"] if ck else []) + (["the run is to be picked up"] if pickup else []))
                                          + ", but a nested pair is checkpointed and picked up only on a backend with nest_set_levels and checkpoint_begin / "
                                          "checkpoint_load on both models (the HIP library, ABI 16)")
        if self.feedback:
            if not hasattr(self.parent.model.backend, "bforce_init_band"):
                raise NotImplementedError(self.FEEDBACK_REFUSAL)
            if any(w.kind == "boundary_forcing" for w in pw):
                raise NotImplementedError("NestForcing: feedback=True on a parent that carries a BoundaryForcing of its own: a model holds one "
                                          "forcing set, and the feedback is one (not supported together)")
        if store or cash_store:
            raise NotImplementedError("NestForcing: run(child, store=True / cash_store=True) takes the per-step loop; a nest needs the chunked path")
        if sim.stop_time == float("inf"):
            raise ValueError("NestForcing needs a finite stop_time (the parent's steps are counted from the child's)")
        check_ratio(self.ratio, float(sim.Δt), float(self.parent.Δt))
        for m, dt, who in ((sim.model, sim.Δt, "child"), (self.parent.model, self.parent.Δt, "parent")):
            if not _chunked(m, dt):
                raise NotImplementedError(f"NestForcing: the {who} model would leave picles_run_steps (wind closures that vary in time, or a "
                                          f"backend without run_steps): {WINDS_REFUSAL}")
        for w in pw:
            if not hasattr(self.parent.model.backend, w.needs):
                raise NotImplementedError(w.refusal)
        self.dt = float(sim.Δt)

    # ---- the parent, driven as run(parent) would drive it, one step per chunk ----
    def _parent_begin(self, n_parent):
        """the parent's side of begin_run.  A parent that has not been initialised is seeded; one that has been run already (a
        spin-up in front of `start_from_parent`) goes on from its clock, and its writers are begun for the nested leg as a second
        `run(parent_sim)` would begin them: files sized for `n_parent` steps, the record of the parent's current iteration first.
        Point them at another path for the nested leg (`writer.path = ...` on the same objects: a
        StationWriter owns the parent's probe set), or they overwrite what the spin-up wrote"""
        from .simulations import initialize_simulation
        ps, pm = self.parent, self.parent.model
        if not ps.initialized:
            initialize_simulation(ps)
        self._pw = writers_of(ps)
        self._pphase = {p: in_phase(self._pw, p) for p in PHASE_ORDER}
        pm.upload_winds(pm.clock.time, ps.Δt)
        self._ptime0, self._pit0, self.parent_steps = pm.clock.time, int(pm.clock.iteration), 0
        for w in self._pphase["begin_run"]:
            w.begin_run(pm, n_parent)

    def _parent_step(self, child_backend):
        """one fused step of the parent, which stays pending, and the level behind it"""
        ps, pm = self.parent, self.parent.model
        pb = pm.backend
        for w in self._pw:
            if w.steps_allowed(pb, self._pit0 + self.parent_steps) < 1:
                raise RuntimeError(f"NestForcing: the parent's {w.kind} writer allows no step")
        if self.feedback:
            self._feed(child_backend)         # both clocks stand at the parent's: what the child resolved goes into this step
        pb.run_steps(ps.Δt, 1)
        child_backend.nest_sample()
        for w in self._pphase["after_chunk"]:
            w.after_chunk(pb)
        self.parent_steps += 1
        pm.clock.time = self._ptime0 + self.parent_steps * ps.Δt
        pm.clock.iteration = self._pit0 + self.parent_steps
        for w in self._pphase["at_iteration"]:
            w.at_iteration(pm, self._pw)

    def _feed(self, child_backend):
        child_backend.nest_feedback()
        self.feedbacks += 1

    def _took_level(self, backend):
        """the library holds a new level: its time is the parent's clock, and the level to come is one parent step later"""
        _, levels, t0, t1 = backend.bforce_info()
        self._have += 1
        self.uploads += 1
        self.times = np.concatenate([self.times[:self._have], [t1 if levels == 2 else t0, (t1 if levels == 2 else t0) + float(self.parent.Δt)]])

    # ---- BoundaryForcing's hooks ----
    def level(self, k):
        raise NotImplementedError("NestForcing: the levels live on the device (backend.bforce_get_levels reads the pair held)")

    def _apply(self, backend, t, force=False):
        """the library holds the pair that brackets t: window_of names it; where its later level has not been taken yet the parent
        steps and is sampled"""
        k = self.window_of(t)
        while k + 1 > self._have:
            self._parent_step(backend)
            self._took_level(backend)
        if k + 1 != self._have:
            raise ValueError(f"NestForcing: a step would start at t = {t!r}, before the pair of parent levels the library holds "
                             f"[{self.times[self._have - 1]!r}, {self.times[self._have]!r}]")
        self._k = k
        return k

    def begin_run(self, model, n_steps: int):
        if self._resume is not None:
            return self._begin_resumed(model, n_steps)
        b = model.backend
        ps, pm = self.parent, self.parent.model
        n_parent = max(1, -(-int(n_steps) // self.ratio))
        self._parent_begin(n_parent)
        if float(pm.clock.time) != float(model.clock.time):
            raise ValueError(f"NestForcing: the child's clock ({model.clock.time!r}) and the parent's ({pm.clock.time!r}) differ")
        if self._set_on is b:
            b.bforce_free()               # (a feedback left behind goes with it)
            self._fb_on = None
        self._init_set(b)
        b.nest_init(pm.backend, self.corner_nodes, self.index, self.weights)
        self._set_on = b
        self.times, self._have, self._k = np.zeros(0), -1, None
        self._mark = (self._time(b), int(model.clock.iteration))
        self._cit0 = int(model.clock.iteration)
        b.nest_sample()                   # level 0: the parent at the common clock
        self._took_level(b)
        if self.feedback:
            b.nest_feedback_init(self.fb_nodes, self.src_nodes, self.fb_index, self.fb_weights)
            self._fb_on = b
            self.feedbacks = 0
            self._feed(b)                 # the seed: State in memory at the common clock — the parent's set holds a level from here on
        self._parent_step(b)              # the parent is one step ahead from here on
        self._took_level(b)

    # ---- a pair checkpoint: the child's file, the parent's at ITS clock — t1 of the pair held — and the pair ----
    def checkpoint_begun(self, backend, checkpoint_file):
        """the child's Checkpointer has taken the child's snapshot: the parent's is taken now, at the parent's clock, the pair is read
        as the child holds it, and the parent's writers hear of the parent's file; the blob is fetched one chunk later"""
        self._pair_finish()
        pm = self.parent.model
        pb = pm.backend
        pb.checkpoint_begin()
        _, levels, t0, t1 = backend.bforce_info()
        if levels != 2 or float(pm.clock.time) != t1:
            raise CheckpointError(0, f"NestForcing: the child holds {levels} level(s) up to {t1!r} and the parent's clock is {pm.clock.time!r}: "
                                     "a pair checkpoint needs the pair whose later level is the parent's State at its clock")
        v0, v1 = backend.bforce_get_levels()
        pfile = parent_checkpoint_path(checkpoint_file)
        for w in self._pw:
            w.checkpoint_begun(pb, pfile)
        link = dict(t0=np.float64(t0), t1=np.float64(t1), v0=v0, v1=v1, ratio=np.int64(self.ratio), feedback=np.bool_(self.feedback),
                    child_time=np.float64(self.model.clock.time), child_iteration=np.int64(self.model.clock.iteration),
                    parent_time=np.float64(pm.clock.time), parent_iteration=np.int64(pm.clock.iteration),
                    uploads=np.int64(self.uploads), parent_steps=np.int64(self.parent_steps), feedbacks=np.int64(self.feedbacks),
                    times=np.asarray(self.times, dtype=np.float64), have=np.int64(self._have),
                    parent_time0=np.float64(self._ptime0), parent_iteration0=np.int64(self._pit0), child_iteration0=np.int64(self._cit0),
                    hash=np.str_(self.geometry_hash()))
        self._pair = (pfile, link_path(checkpoint_file), float(pm.clock.time), int(pm.clock.iteration), link, Path(checkpoint_file))

    def _pair_finish(self):
        """the parent's blob, whose copy-out ran beside the chunk, then the link: the side-car is the last of the three files"""
        if self._pair is None:
            return
        pfile, lfile, time, iteration, link, cfile = self._pair
        self._pair = None
        write_checkpoint_file(pfile, self.parent.model.backend.checkpoint_end(), time, iteration)
        _write_link(lfile, **link)
        self.pairs_written.append(cfile)

    def after_chunk(self, backend):
        self._pair_finish()

    def pickup_companions(self, checkpoint_file):
        return (parent_checkpoint_path(checkpoint_file), link_path(checkpoint_file))

    def check_pickup(self, checkpoint_file):
        """the parent's file and the link side-car are there and were written under this NestForcing; nothing is loaded"""
        for f in (Path(checkpoint_file),) + tuple(self.pickup_companions(checkpoint_file)):
            if not f.is_file():
                raise CheckpointError(0, f"NestForcing: {f} is missing: a nested pair is picked up from the child's file, the parent's file and the "
                                         "link side-car next to it")
        pfile, lfile = self.pickup_companions(checkpoint_file)
        try:
            with np.load(lfile) as z:
                link = {k: z[k] for k in z.files}
            have = {"t0", "t1", "v0", "v1", "ratio", "feedback", "hash", "times", "have", "child_time", "child_iteration", "parent_time",
                    "parent_iteration", "uploads", "parent_steps", "feedbacks", "parent_time0", "parent_iteration0", "child_iteration0"} <= set(link)
        except Exception as e:
            raise CheckpointError(0, f"NestForcing: {lfile} is not a link side-car ({e})") from None
        if not have:
            raise CheckpointError(0, f"NestForcing: {lfile} is not a link side-car (entries are missing)")
        for what, got, want in (("ratio", int(link["ratio"]), self.ratio), ("feedback", bool(link["feedback"]), self.feedback),
                                ("geometry hash", str(link["hash"]), self.geometry_hash())):
            if got != want:
                raise CheckpointError(0, f"NestForcing: {lfile} was written by another nest: its {what} is {got!r}, this NestForcing's {want!r}")
        n = len(self.nodes)
        if link["v0"].shape != (n, 3) or link["v1"].shape != (n, 3):
            raise CheckpointError(0, f"NestForcing: {lfile}: the pair's levels are not ({n}, 3) arrays")
        with open(pfile, "rb") as f:
            head = f.read(_HEAD.size)
        if len(head) == _HEAD.size:
            _, _, _, it, time, _ = _HEAD.unpack(head)
            if it != int(link["parent_iteration"]) or time != float(link["parent_time"]):
                raise CheckpointError(0, f"NestForcing: {pfile} holds the parent at iteration {it}, t = {time!r}; the side-car {lfile.name} names "
                                         f"iteration {int(link['parent_iteration'])}, t = {float(link['parent_time'])!r}")
        self._link = (Path(checkpoint_file), link)

    def load_pickup(self, checkpoint_file):
        """the child has been loaded: the parent is loaded from its file next to the child's, its writers take what they stored next
        to that, and the pair is remembered for begin_run"""
        if self._link is None or self._link[0] != Path(checkpoint_file):
            self.check_pickup(checkpoint_file)
        link, self._link = self._link[1], None
        ps = self.parent
        pfile = parent_checkpoint_path(checkpoint_file)
        load_checkpoint(ps.model, pfile, ps.Δt)
        ps.initialized = True
        ps.running = False
        for w in writers_of(ps):
            w.load_pickup(pfile)
        self._resume = link

    def _begin_resumed(self, model, n_steps: int):
        """begin_run after a pickup: the set and the nest are made again and the pair is put back (nest_set_levels) — no seed sample
        and no seed feedback: the ordinary loop steps the parent where the uninterrupted run would have, its feedback in front"""
        link, self._resume = self._resume, None
        b = model.backend
        ps, pm = self.parent, self.parent.model
        done = int(model.clock.iteration) - int(link["child_iteration0"])          # child steps since the nest began
        n_parent = max(0, -(-(done + int(n_steps)) // self.ratio) - int(link["parent_steps"]))
        self._parent_begin(n_parent)
        for who, m, tag in (("child", model, "child"), ("parent", pm, "parent")):
            if float(m.clock.time) != float(link[tag + "_time"]) or int(m.clock.iteration) != int(link[tag + "_iteration"]):
                raise CheckpointError(0, f"NestForcing: the {who}'s clock ({m.clock.time!r}, iteration {m.clock.iteration}) is not the link side-car's "
                                         f"({float(link[tag + '_time'])!r}, iteration {int(link[tag + '_iteration'])})")
        if self._set_on is b:
            b.bforce_free()
            self._fb_on = None
        self._init_set(b)
        b.nest_init(pm.backend, self.corner_nodes, self.index, self.weights)
        self._set_on = b
        b.nest_set_levels(float(link["t0"]), link["v0"], float(link["t1"]), link["v1"])
        self.times, self._have, self._k = np.asarray(link["times"], dtype=np.float64), int(link["have"]), None
        self.uploads, self.parent_steps, self.feedbacks = int(link["uploads"]), int(link["parent_steps"]), int(link["feedbacks"])
        self._ptime0, self._pit0, self._cit0 = float(link["parent_time0"]), int(link["parent_iteration0"]), int(link["child_iteration0"])
        self._mark = (self._time(b), int(model.clock.iteration))
        if self.feedback:
            b.nest_feedback_init(self.fb_nodes, self.src_nodes, self.fb_index, self.fb_weights)
            self._fb_on = b

    def before_step(self, backend):
        raise NotImplementedError("NestForcing: run() left its chunked path (store=True, cash_store=True or wind closures that vary in time)")

    def at_iteration(self, model, writers):
        """the step actually taken is held against the ratio once it can be read off the clock; the next pair is steps_allowed's
        business (no step of the parent is taken that no step of the child needs)"""
        b = model.backend
        t, it = self._time(b), int(model.clock.iteration)
        if self._mark is not None and it > self._mark[1]:
            check_ratio(self.ratio, (t - self._mark[0]) / (it - self._mark[1]), float(self.parent.Δt))
            self._mark = None

    def finish(self, backend, iteration=None):
        """the parent's writers finish with the child's; the nest and the set go with the run"""
        self._pair_finish()
        if getattr(self, "_pw", None) is not None:
            pm = self.parent.model
            for w in self._pphase["finish"]:
                w.finish(pm.backend, pm.clock.iteration)
            self._pw = None
        if self._fb_on is backend:
            backend.nest_feedback_free()
            self._fb_on = None
        if self._set_on is backend:
            backend.nest_free()
            backend.bforce_free()
            self._set_on = None
            self._k = None
