"""Moving nests on the CPU box (picles_amd/nesting.py: relocate_state, move_child, run_following; picles_amd/grids.py: translated;
DESIGN.md §26): `relocate_state` against a scalar per-node restatement on hostile values, the translated grid against a grid built
at the new place, and the leg logic of `run_following` and the refusals of `move_child` over the recording backends of
tests/test_nesting_host.py, extended here with a `nest_relocate` that records and refuses what the library refuses.

The boxes are those of tests/test_nesting_host.py, so that tests/test_gpu_nest_move.py speaks of the same ones."""
import numpy as np
import pytest

from picles_amd import models
from picles_amd.grids import TwoDCartesianGridMesh, translated
from picles_amd.nesting import NestForcing, kept_box, move_child, prolong_state, relocate_state, run_following
from picles_amd.simulations import Simulation, run
from test_nest_lattice_host import _hostile_parent_state, _prolong_scalar
from test_nesting_host import C_DX, C_X0, C_Y0, K_SHAPE, P_DX, W_SHAPE, NestBackend, child_cfg, parent_cfg

SHIFTS = [(9, 2), (-7, -3), (0, 1), (0, 0), (70, 0)]
MARGINS = [0, 1, 3]


def kept_count(shape, shift, m):
    """the issue's formula: kx ky, kx = max(0, Ncx - max(m, si) - max(m, -si))"""
    (ncx, ncy), (si, sj) = shape, shift
    return max(0, ncx - max(m, si) - max(m, -si)) * max(0, ncy - max(m, sj) - max(m, -sj))


# ---- 1. relocate_state against a scalar restatement ----
def _hostile_child_state():
    rng = np.random.default_rng(41)
    S = np.stack([np.exp(rng.uniform(-6, 2, K_SHAPE)), rng.normal(0, 0.05, K_SHAPE), rng.normal(0, 0.05, K_SHAPE)], axis=-1)
    S[3, 3] = (np.nan, 0.1, 0.1)
    S[12, 4] = (1.0, np.inf, 0.1)
    S[13, 4] = (1.0, 0.1, -np.inf)
    S[14, 5] = (1.0, 0.0, 0.0)                       # zero momentum
    S[20:24, 3:6] = 0.0                              # calm nodes: copied as they stand, not filled from the parent
    S[40, 6] = (-0.0, -0.0, 0.0)                     # ... and the sign of a zero is bits too
    S[41, 2].view(np.uint64)[0] = 0x7FF8000000000123  # a NaN payload
    S[60, 4] = (-np.inf, np.nan, 1e-300)
    return S


@pytest.fixture(scope="module")
def prolonged():
    """per shift: the new grid and the scalar restatement of the prolong there (k_nest_prolong node by node in Python floats)"""
    pg, Sp = parent_cfg(land=True).model["grid"], _hostile_parent_state()
    out = {}
    for si, sj in SHIFTS:
        ng = child_cfg(K_SHAPE, x0=C_X0 + si * C_DX, y0=C_Y0 + sj * C_DX).model["grid"]
        out[(si, sj)] = (ng, _prolong_scalar(Sp, pg, ng)[0])
    return pg, Sp, out


@pytest.mark.parametrize("m", MARGINS)
@pytest.mark.parametrize("shift", SHIFTS, ids=[f"{a}_{b}" for a, b in SHIFTS])
def test_relocate_state_equals_the_scalar_restatement_bit_for_bit(prolonged, shift, m):
    pg, Sp, per_shift = prolonged
    ng, P = per_shift[shift]
    Sc = _hostile_child_state()
    si, sj = shift
    ncx, ncy = K_SHAPE
    want = np.empty(K_SHAPE + (3,))
    kept = np.zeros(K_SHAPE, dtype=bool)
    for i in range(ncx):
        for j in range(ncy):
            kept[i, j] = m <= i + si < ncx - m and m <= j + sj < ncy - m
            want[i, j].view(np.uint64)[:] = (Sc[i + si, j + sj] if kept[i, j] else P[i, j]).view(np.uint64)
    got = relocate_state(Sc, Sp, pg, ng, shift=shift, keep_margin=m)
    assert got.shape == K_SHAPE + (3,) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert int(kept.sum()) == kept_count(K_SHAPE, shift, m)
    i0, i1, j0, j1 = kept_box(K_SHAPE, shift, m)
    box = np.zeros(K_SHAPE, dtype=bool)
    box[i0:i1, j0:j1] = True
    assert np.array_equal(box, kept)
    if shift == (70, 0):
        assert not kept.any() and np.array_equal(got.view(np.uint64), prolong_state(Sp, pg, ng).view(np.uint64))
    if shift == (0, 0) and m == 0:
        assert kept.all() and np.array_equal(got.view(np.uint64), Sc.view(np.uint64))
    if shift in ((9, 2), (-7, -3)):
        assert kept.any() and (~kept).any()
    # the inputs are not written
    assert np.array_equal(Sc.view(np.uint64), _hostile_child_state().view(np.uint64))


def test_relocate_state_refuses_what_is_no_shift():
    pg, cg = parent_cfg().model["grid"], child_cfg(K_SHAPE).model["grid"]
    Sp, Sc = _hostile_parent_state(), _hostile_child_state()
    for bad in (-1, 1.0, None):
        with pytest.raises(ValueError, match="keep_margin"):
            relocate_state(Sc, Sp, pg, cg, shift=(0, 0), keep_margin=bad)
    with pytest.raises(ValueError, match="whole child nodes"):
        relocate_state(Sc, Sp, pg, cg, shift=(1.5, 0), keep_margin=1)
    with pytest.raises(ValueError, match="keeps the box's shape"):
        relocate_state(Sc[:-1], Sp, pg, cg, shift=(0, 0), keep_margin=1)


# ---- 2. translated ----
@pytest.mark.parametrize("shape", [K_SHAPE, W_SHAPE], ids=["K70x9", "W128x12"])
@pytest.mark.parametrize("shift", SHIFTS + [(105, 0), (-13, 29)], ids=lambda s: f"{s[0]}_{s[1]}")
def test_translated_grid_has_the_bits_of_a_grid_built_there(shape, shift):
    si, sj = shift
    g = translated(child_cfg(shape).model["grid"], si, sj)
    ref = child_cfg(shape, x0=C_X0 + si * C_DX, y0=C_Y0 + sj * C_DX).model["grid"]
    for a, b in ((g.data.x, ref.data.x), (g.data.y, ref.data.y)):
        assert a.shape == b.shape and np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))
    assert np.array_equal(g.data.mask, ref.data.mask)
    assert (g.stats.dx, g.stats.dy, type(g.stats.Nx), type(g.stats.Ny)) == (ref.stats.dx, ref.stats.dy, type(ref.stats.Nx), type(ref.stats.Ny))


def test_translated_refuses_land_periodic_axes_and_half_nodes():
    with pytest.raises(NotImplementedError, match="periodic"):
        translated(parent_cfg().model["grid"], 1, 0)
    mask = np.ones(K_SHAPE, dtype=bool)
    mask[30, 4] = False
    land = TwoDCartesianGridMesh(C_X0, C_X0 + C_DX * 69, 70, C_Y0, C_Y0 + C_DX * 8, 9, mask=mask)
    with pytest.raises(NotImplementedError, match="land"):
        translated(land, 1, 0)
    with pytest.raises(ValueError, match="whole nodes"):
        translated(child_cfg(K_SHAPE).model["grid"], 0.5, 0)


# ---- 3. run_following and move_child over recording backends ----
class MoveBackend(NestBackend):
    """NestBackend + the move: refuses what the library refuses of a child's state"""

    def bforce_init_band(self, nodes, weights=None):
        self.bforce_init(nodes)

    def nest_relocate(self, parent, si, sj, keep_margin, ix0, ix1, wx, iy0, iy1, wy, dt, mesh_x0, mesh_y0):
        assert self.bf is None and getattr(self, "nest", None) is None, "nest_relocate on a child that still holds its set or its nest"
        assert self.clock == parent.clock and keep_margin >= 0 and dt > 0
        assert len(ix0) == len(ix1) == len(wx) == self.Nx and len(iy0) == len(iy1) == len(wy) == self.Ny
        self.log.append(("nest_relocate", si, sj, keep_margin, mesh_x0, mesh_y0))
        if self.journal is not None:
            self.journal.append((self.name, "nest_relocate", (si, sj), self.clock))


def _open_parent_cfg():
    pc = parent_cfg()
    pc.model["grid"] = TwoDCartesianGridMesh(P_DX * 63, 64, P_DX * 15, 16, periodic_boundary=(False, False))
    pc.model["periodic_boundary"] = False
    return pc


def _pair(pc=None, cc=None, child_cls=models.WaveGrowth2D):
    pc, cc = pc or parent_cfg(), cc or child_cfg(K_SHAPE)
    pm = models.WaveGrowth2D(**pc.model, backend_factory=MoveBackend)
    cm = child_cls(**cc.model, backend_factory=MoveBackend)
    journal = []
    for m, name in ((pm, "parent"), (cm, "child")):
        m.backend.journal, m.backend.name = journal, name
    return pm, Simulation(pm, Δt=600.0, stop_time=1e9), cm, Simulation(cm, Δt=200.0, stop_time=0.0), journal


def _drift(t):
    """the box centre of K (100 km, 25 km) drifting east by 2.4 child nodes per parent step"""
    return 100000.0 + 2.4 * C_DX * t / 600.0, 25000.0


def _legs(journal):
    """the journal cut at the moves and leg ends: per leg (child steps, parent steps)"""
    legs, c, p = [], 0, 0
    for e in journal:
        if e[1] == "run_steps":
            c, p = (c + e[2], p) if e[0] == "child" else (c, p + e[2])
        if e[1] == "leg":
            legs.append((c, p))
            c, p = 0, 0
    return legs


@pytest.mark.parametrize("snap,every,want_shifts", [("child", 1, [(2, 0), (3, 0), (2, 0)]), ("parent", 1, [(3, 0), (3, 0), (0, 0)]),
                                                    ("child", 2, [(5, 0), (5, 0)])])
def test_run_following_legs_snapping_and_fresh_forcings(snap, every, want_shifts):
    pm, psim, cm, csim, journal = _pair()
    seen, forcings = [], []

    def on_leg(k, sim):
        assert sim is csim
        seen.append((k, cm.clock.time))

    def centre(t):
        forcings.append(csim.output_writers["boundary_forcing"])
        journal.append(("-", "leg", None, t))
        return _drift(t)

    n_legs = len(want_shifts)
    boxes = run_following(csim, psim, centre, stop_time=600.0 * every * n_legs, every=every, snap=snap, on_leg=on_leg,
                          nest=dict(side="rim", ratio=3, width=2))
    assert _legs(journal) == [(3 * every, every)] * n_legs
    assert seen == [(k, 600.0 * every * k) for k in range(n_legs)]
    assert len(forcings) == n_legs and len({id(f) for f in forcings}) == n_legs and all(isinstance(f, NestForcing) and f.width == 2 for f in forcings)
    assert [e[0] for e in cm.backend.log].count("nest_init") == n_legs
    moves = [e for e in cm.backend.log if e[0] == "nest_relocate"]
    cum = np.cumsum([(0, 0)] + want_shifts, axis=0)
    assert [(e[1], e[2]) for e in moves] == [s for s in want_shifts if s != (0, 0)]          # a zero shift makes no call
    assert all(e[3] == 2 for e in moves)                                                   # keep_margin: max(1, width)
    assert boxes == [(600.0 * every * k, C_X0 + C_DX * cum[k][0], C_Y0 + C_DX * cum[k][1]) for k in range(n_legs + 1)]
    assert [(e[4], e[5]) for e in moves] == [b[1:] for b, s in zip(boxes[1:], want_shifts) if s != (0, 0)]
    assert (cm.clock.time, cm.clock.iteration, pm.clock.iteration) == (600.0 * every * n_legs, 3 * every * n_legs, every * n_legs)
    assert float(cm.grid.data.x[0, 0]) == boxes[-1][1] and cm.backend.clock == pm.backend.clock
    # every forcing was built on the grid of its leg: its corner geometry differs from leg to leg where the box moved
    hashes = [f.geometry_hash() for f in forcings]
    assert len(set(hashes)) == 1 + sum(s != (0, 0) for s in want_shifts[:-1])
    # static winds were uploaded at the new nodes in front of every move, and only there
    assert [e[0] for e in cm.backend.log if e[0] in ("set_winds", "nest_relocate")] == ["set_winds"] + ["set_winds", "nest_relocate"] * len(moves)


@pytest.mark.parametrize("snap,want", [("child", (104, -8)), ("parent", (102, -6))])
def test_run_following_clamps_at_a_non_periodic_parent_edge(snap, want):
    pm, psim, cm, csim, _ = _pair(pc=_open_parent_cfg())
    boxes = run_following(csim, psim, lambda t: (1e9, -1e9), stop_time=1200.0, snap=snap, nest=dict(side="rim", ratio=3))
    moves = [e for e in cm.backend.log if e[0] == "nest_relocate"]
    assert [(e[1], e[2]) for e in moves] == [want]                                          # the second leg finds the box at the edge: no call
    assert boxes[1][1:] == boxes[2][1:] == (C_X0 + C_DX * want[0], C_Y0 + C_DX * want[1])
    x, y = cm.grid.data.x, cm.grid.data.y
    assert 0.0 <= x.min() and x.max() <= P_DX * 63 and 0.0 <= y.min() and y.max() <= P_DX * 15
    if snap == "child":                                                                     # the last whole node inside
        assert x.max() + C_DX > P_DX * 63 and y.min() - C_DX < 0.0


def test_run_following_refuses_bad_arguments_before_anything_runs():
    pm, psim, cm, csim, _ = _pair()
    for kw, match in ((dict(snap="nearest"), "snap"), (dict(every=0), "every"), (dict(nest=dict(side="rim")), "ratio")):
        args = dict(stop_time=600.0, nest=dict(side="rim", ratio=3))
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            run_following(csim, psim, _drift, **args)
    assert not cm.backend.log or not [e for e in cm.backend.log if e[0] in ("seed", "run_steps")]


class SlabModel(models.WaveGrowth2D):
    """(only the name is looked at: slabs do not nest)"""


def test_move_child_refusals_leave_grid_and_clocks_untouched():
    def after_a_leg(**kw):
        pm, psim, cm, csim, _ = _pair(**kw)
        csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
        csim.stop_time = 500.0
        run(csim)
        assert (cm.clock.time, pm.clock.time) == (600.0, 600.0)
        return pm, psim, cm, csim

    def refused(exc, match, pm, psim, cm, csim, shift=(2, 1), **kw):
        grid, clocks, n_log = cm.grid, (cm.clock.time, cm.clock.iteration, pm.clock.time, pm.clock.iteration, cm.backend.clock), len(cm.backend.log)
        with pytest.raises(exc, match=match):
            move_child(csim, psim, shift, **kw)
        assert cm.grid is grid and clocks == (cm.clock.time, cm.clock.iteration, pm.clock.time, pm.clock.iteration, cm.backend.clock)
        assert len(cm.backend.log) == n_log                                                 # no upload, no call

    # a child with land
    mask = np.ones(K_SHAPE, dtype=bool)
    mask[30:32, 4] = False
    cc = child_cfg(K_SHAPE)
    cc.model["grid"] = TwoDCartesianGridMesh(C_X0, C_X0 + C_DX * 69, 70, C_Y0, C_Y0 + C_DX * 8, 9, mask=mask)
    refused(NotImplementedError, "land", *after_a_leg(cc=cc))
    # unequal clocks
    pm, psim, cm, csim = after_a_leg()
    pm.clock.time += 600.0
    refused(ValueError, "clock", pm, psim, cm, csim)
    pm.clock.time -= 600.0
    # shifts and margins that are none
    refused(ValueError, "whole child nodes", pm, psim, cm, csim, shift=(0.5, 0))
    refused(ValueError, "keep_margin", pm, psim, cm, csim, keep_margin=-1)
    # a child that was never run
    pm2, psim2, cm2, csim2, _ = _pair()
    refused(ValueError, "must have been run", pm, psim, cm2, csim2)
    # leaving the parent: an open parent's north edge (rows up to y = 33 km + 60 km > 90 km), and a periodic axis does not wrap a box
    refused(ValueError, "outside the mesh", *after_a_leg(pc=_open_parent_cfg()), shift=(0, 30))
    refused(ValueError, "outside the periodic axis", pm, psim, cm, csim, shift=(0, 40))
    # slabs
    refused(NotImplementedError, "slabs", *_pair(child_cls=SlabModel)[:4])                 # (a slab child never had a leg: NestForcing refuses it too)
    # a backend without the call
    pm3 = models.WaveGrowth2D(**parent_cfg().model, backend_factory=NestBackend)
    cm3 = models.WaveGrowth2D(**child_cfg(K_SHAPE).model, backend_factory=NestBackend)
    psim3, csim3 = Simulation(pm3, Δt=600.0, stop_time=1e9), Simulation(cm3, Δt=200.0, stop_time=500.0)
    csim3.output_writers["boundary_forcing"] = NestForcing(cm3, parent=psim3, side="rim", ratio=3)
    run(csim3)
    refused(NotImplementedError, "nest_relocate", pm3, psim3, cm3, csim3)
    # and the move itself goes through afterwards: default margin from the forcing still attached, the grid replaced, the clocks kept
    move_child(csim, psim, (2, 1))
    assert cm.backend.log[-1] == ("nest_relocate", 2, 1, 1, C_X0 + 2 * C_DX, C_Y0 + C_DX) and cm.backend.log[-2][0] == "set_winds"
    assert float(cm.grid.data.x[0, 0]) == C_X0 + 2 * C_DX and (cm.clock.time, cm.clock.iteration) == (600.0, 3)
