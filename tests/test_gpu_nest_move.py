"""A child box moved across its parent, on the GPU (picles_nest_relocate, k_nest_relocate in picles_amd/csrc/k_nest.h,
nesting.move_child / run_following): the moved child's State is `relocate_state` bit for bit; its particles, flags,
controller memory and counters are those of a child built at the new origin through the public API as seed(t), set_state(relocated),
remesh(dt), and stay so through a further nested leg; under a lattice the child's window is the lattice at the NEW node coordinates;
a two-way pair and `run_following` equal their hand-driven twins; the refusals leave two usable contexts.

The boxes are those of tests/test_nesting_host.py: (P-land) 64 x 16 periodic at 6 km with its 3 x 3 land block; the children (K)
70 x 9 — 630 nodes: ragged rows and a ragged last workgroup — and (W) 128 x 12 — six full workgroups — at 2 km; parent step 600 s,
ratio 3.  The two-way case takes (F) 70 x 21 of tests/test_gpu_nest_feedback.py in P's non-periodic twin: K and W are too thin to
hold a feedback node at the default margin."""
import numpy as np
import pytest

from picles_amd import _capi as K
from picles_amd.grids import TwoDCartesianGridMesh, translated
from picles_amd.nesting import NestForcing, kept_box, move_child, prolong_state, prolong_tables, relocate_state, run_following, start_from_parent
from picles_amd.simulations import Simulation, initialize_simulation, run
from helpers import assert_same_bits, make_model
from test_gpu_boundary_forcing import _assert_same_model, _everything
from test_gpu_nest_feedback import F_SHAPE, pn_cfg
from test_gpu_nest_prolong import _blob, _by_hand, _spun_up
from test_gpu_nesting import _geometry
from test_nest_lattice_host import lattice_winds, under
from test_nest_move_host import kept_count
from test_nesting_host import C_DX, C_X0, C_Y0, K_SHAPE, W_SHAPE, child_cfg, parent_cfg

pytestmark = pytest.mark.gpu

DT = 600.0
DTC = DT / 3


def _assert_same_blob(a, b, what):
    """the restart blobs of two models, bit for bit; a failure names the header bytes and the payload segments that differ
    (picles_hip.hip: CkptHeader — segment offsets at byte 80, lengths at byte 160, ten of each)"""
    A, B = _blob(a), _blob(b)
    if A.shape == B.shape and np.array_equal(A, B):
        return
    assert A.shape == B.shape, f"{what}: blobs of {A.size} and {B.size} bytes"
    off, length = A[80:160].view(np.uint64), A[160:240].view(np.uint64)
    head = np.flatnonzero(A[:256] != B[:256]).tolist()
    segs = [k for k in range(10) if not np.array_equal(A[256 + int(off[k]):256 + int(off[k] + length[k])], B[256 + int(off[k]):256 + int(off[k] + length[k])])]
    raise AssertionError(f"{what}: restart blobs differ: header bytes {head}, payload segments {segs}")


def _at(shape, si=0, sj=0):
    return child_cfg(shape, x0=C_X0 + si * C_DX, y0=C_Y0 + sj * C_DX)


def _leg(csim, psim, n_parent, **nest):
    """one nested leg of n_parent parent steps under a fresh NestForcing"""
    cm = csim.model
    psim.stop_time = 1e9
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, **{"side": "rim", "ratio": 3, **nest})
    csim.stop_time = cm.clock.time + (3 * n_parent - 0.5) * DTC
    run(csim)
    return f


def _started_and_nested(cfg, parent, n_spin, n_parent):
    """a parent spun up alone, a child started from it and nested beside it for n_parent parent steps: the child holds sea of its own"""
    pm, psim = _spun_up(parent, n_spin)
    cm = make_model(cfg, "hip")
    csim = Simulation(cm, Δt=DTC, stop_time=0.0)
    start_from_parent(csim, psim)
    _leg(csim, psim, n_parent)
    assert cm.clock.time == pm.clock.time == (n_spin + n_parent) * DT and cm.backend.clock == pm.backend.clock
    return pm, psim, cm, csim


# ---- 4. the device route is the definition ----
@pytest.mark.parametrize("shape,shift,m", [(K_SHAPE, (9, 2), 1), (K_SHAPE, (-7, -3), 1), (K_SHAPE, (70, 0), 1), (K_SHAPE, (105, 0), 1), (W_SHAPE, (9, 2), 3)],
                         ids=["K-9_2", "K-m7_m3", "K-70_0-nothing-kept", "K-105_0-across-the-wrap-cell", "W-9_2-margin3"])
def test_moved_child_is_the_definition_and_stays_equal_to_the_child_built_at_the_new_origin(shape, shift, m):
    si, sj = shift
    # twins: the first pair is moved on the device with its last steps still pending; the old State is read off the second
    pm, psim, cm, csim = _started_and_nested(_at(shape), parent_cfg(land=True), 6, 2)
    pm2, psim2, old2, _ = _started_and_nested(_at(shape), parent_cfg(land=True), 6, 2)
    t = pm.clock.time
    Sc, Sp = old2.backend.get_state(), pm2.backend.get_state()
    new_grid = translated(cm.grid, si, sj)
    want = relocate_state(Sc, Sp, pm.grid, new_grid, shift=shift, keep_margin=m)
    P = prolong_state(Sp, pm.grid, new_grid)
    move_child(csim, psim, shift, keep_margin=m)
    assert (cm.clock.time, cm.clock.iteration, cm.backend.clock) == (t, 6, pm.backend.clock) and cm.grid is not new_grid
    assert_same_bits(np.asarray(cm.grid.data.x), np.asarray(new_grid.data.x), "the child's grid after the move")
    got = cm.backend.get_state()
    assert_same_bits(got, want, "the moved child's State against relocate_state", nan_payload=True)
    assert_same_bits(np.asarray(cm.State), want, "the lazy view re-read")
    assert_same_bits(cm.backend.get_movie_state(), want, "MovieState holds the relocated State")
    assert_same_bits(pm.backend.get_state(), Sp, "the parent is not touched")
    # both classes of node, with the formula's counts; the kept sea is the child's own, not the parent's
    i0, i1, j0, j1 = kept_box(shape, shift, m)
    kept = np.zeros(shape, dtype=bool)
    kept[i0:i1, j0:j1] = True
    differs = (want.view(np.uint64) != P.view(np.uint64)).any(axis=-1)
    print(f"{shape} by {shift}, margin {m}: {int(kept.sum())} kept, {int((~kept).sum())} exposed; {int(differs[kept].sum())} kept nodes differ from the prolonged parent")
    assert int(kept.sum()) == kept_count(shape, shift, m)
    if abs(si) < shape[0] - 2 * m:
        assert kept.any() and (~kept).any() and differs[kept].sum() >= 0.5 * kept.sum()
        assert_same_bits(got[~kept], P[~kept], "the exposed nodes are the prolonged parent")
        assert_same_bits(got[kept], Sc[i0 + si:i1 + si, j0 + sj:j1 + sj].reshape(-1, 3), "the kept nodes are the child's own", nan_payload=True)
    else:                                                     # nothing kept: start_from_parent at the new place
        assert not kept.any()
        assert_same_bits(got, P, "nothing kept: the prolonged parent")
    if shift == (105, 0):
        ix0, ix1 = prolong_tables(pm.grid, cm.grid)[:2]
        assert (ix0[-1], ix1[-1]) == (63, 0)
    # the second child, built at the new origin through the public API
    stop = t + 5 * DTC
    cm2, csim2 = _by_hand(_at(shape, si, sj), DTC, t, want, stop)
    A, B = _everything(cm), _everything(cm2)
    _assert_same_model(A, B, "move_child vs seed, set_state, remesh at the new origin")
    assert (A[2][1:-1, 1:-1] != 0).all()                      # every interior node bears a particle
    _assert_same_blob(cm, cm2, "move_child vs seed, set_state, remesh at the new origin (controller memory included)")
    # six further child steps, nested
    for cs, ps in ((csim, psim), (csim2, psim2)):
        _leg(cs, ps, 2)
    assert (cm.clock.iteration, cm2.clock.iteration, pm.clock.iteration, cm.clock.time) == (12, 6, 10, t + 6 * DTC)
    _assert_same_model(_everything(cm), _everything(cm2), "after six nested steps: the child")
    _assert_same_model(_everything(pm), _everything(pm2), "after six nested steps: the parent")
    _assert_same_blob(cm, cm2, "after six nested steps")
    assert np.isfinite(cm.backend.get_state()).all()


# ---- 5. under a lattice: the mesh origin moves with the box ----
def test_moved_child_under_a_lattice_samples_it_at_the_new_nodes():
    wind = lattice_winds(900.0)
    shift = (9, 2)
    pm, psim, cm, csim = _started_and_nested(under(_at(K_SHAPE), wind), under(parent_cfg(), wind), 3, 1)
    pm2, psim2, old2, _ = _started_and_nested(under(_at(K_SHAPE), wind), under(parent_cfg(), wind), 3, 1)
    t = pm.clock.time
    assert t == 2400.0                                        # between two time knots of the lattice
    Xo, Yo = np.array(cm.grid.data.x), np.array(cm.grid.data.y)
    want = relocate_state(old2.backend.get_state(), pm2.backend.get_state(), pm.grid, translated(cm.grid, *shift), shift=shift, keep_margin=1)
    move_child(csim, psim, shift, keep_margin=1)
    assert_same_bits(cm.backend.get_state(), want, "the moved child's State against relocate_state", nan_payload=True)
    X, Y = cm.grid.data.x, cm.grid.data.y
    assert X[0, 0] == C_X0 + 9 * C_DX and Y[0, 0] == C_Y0 + 2 * C_DX
    u0, v0, u1, v1 = cm.backend.get_winds()
    for got, ref, what in ((u0, wind.u(X, Y, t), "u(t)"), (v0, wind.v(X, Y, t), "v(t)"), (u1, wind.u(X, Y, t + DTC), "u(t + dt)"),
                           (v1, wind.v(X, Y, t + DTC), "v(t + dt)")):
        assert_same_bits(got, ref, f"the window of the moved child, at the new nodes: {what}")
    assert not np.array_equal(u0, wind.u(Xo, Yo, t))          # a stale mesh origin would give this
    # a child built at the new origin under the same lattice: started from the twin parent there, then the relocated State
    cm2 = make_model(under(_at(K_SHAPE, *shift), wind), "hip")
    csim2 = Simulation(cm2, Δt=DTC, stop_time=0.0)
    start_from_parent(csim2, psim2)
    cm2.backend.set_state(want)
    cm2.backend.remesh(DTC)
    _assert_same_model(_everything(cm), _everything(cm2), "moved under the lattice vs built at the new origin")
    for a, b in zip(cm.backend.get_winds(), cm2.backend.get_winds()):
        assert_same_bits(a, b, "the wind window of both")
    for cs, ps in ((csim, psim), (csim2, psim2)):
        _leg(cs, ps, 2, width=3)
    _assert_same_model(_everything(cm), _everything(cm2), "after a nested leg under the lattice: the child")
    _assert_same_model(_everything(pm), _everything(pm2), "after a nested leg under the lattice: the parent")
    assert np.isfinite(cm.backend.get_state()).all()


# ---- 6. two-way ----
def test_two_way_pair_followed_equals_its_twin_driven_by_hand():
    nest = dict(side="rim", ratio=3, width=2, feedback=True)
    centre = lambda t: (C_X0 + C_DX * 34.5 + 8000.0, C_Y0 + C_DX * 10.0 + 5000.0)      # 1.33 and 0.83 parent cells off the box centre
    # by run_following: a leg, a move, a leg
    pm, cm = make_model(pn_cfg(), "hip"), make_model(_at(F_SHAPE), "hip")
    psim, csim = Simulation(pm, Δt=DT, stop_time=1e9), Simulation(cm, Δt=DTC, stop_time=0.0)
    boxes = run_following(csim, psim, centre, stop_time=2 * DT, every=1, nest=nest, snap="parent")
    assert boxes == [(0.0, C_X0, C_Y0), (DT, C_X0 + 3 * C_DX, C_Y0 + 3 * C_DX), (2 * DT, C_X0 + 3 * C_DX, C_Y0 + 3 * C_DX)]
    # by hand: run, move_child, a new NestForcing, run
    pm2, cm2 = make_model(pn_cfg(), "hip"), make_model(_at(F_SHAPE), "hip")
    psim2, csim2 = Simulation(pm2, Δt=DT, stop_time=1e9), Simulation(cm2, Δt=DTC, stop_time=0.0)
    f = _leg(csim2, psim2, 1, **nest)
    assert f.feedbacks == 2 and len(f.fb_nodes) > 0
    move_child(csim2, psim2, (3, 3), keep_margin=2)
    g = _leg(csim2, psim2, 1, **nest)
    assert g is not f and g.geometry_hash() != f.geometry_hash() and len(g.fb_nodes) > 0
    assert (cm.clock.iteration, pm.clock.iteration, cm.clock.time) == (cm2.clock.iteration, pm2.clock.iteration, cm2.clock.time) == (6, 2, 2 * DT)
    _assert_same_model(_everything(cm), _everything(cm2), "two-way, followed vs by hand: the child")
    _assert_same_model(_everything(pm), _everything(pm2), "two-way, followed vs by hand: the parent")
    _assert_same_blob(cm, cm2, "two-way, the child")
    _assert_same_blob(pm, pm2, "two-way, the parent")
    assert np.isfinite(cm.backend.get_state()).all() and np.isfinite(pm.backend.get_state()).all()
    # the feedback is seen behind the move: the parent differs from a parent beside a one-way child that moves the same way
    pm1, cm1 = make_model(pn_cfg(), "hip"), make_model(_at(F_SHAPE), "hip")
    psim1, csim1 = Simulation(pm1, Δt=DT, stop_time=1e9), Simulation(cm1, Δt=DTC, stop_time=0.0)
    run_following(csim1, psim1, centre, stop_time=2 * DT, nest=dict(side="rim", ratio=3, width=2), snap="parent")
    assert not np.array_equal(pm1.backend.get_state(), pm.backend.get_state())


# ---- 7. run_following ----
def test_run_following_equals_the_hand_written_sequence():
    x_c, y_c = C_X0 + C_DX * 34.5, C_Y0 + C_DX * 4.0            # K's box centre
    pairs = []
    for _ in range(2):
        pm, psim = _spun_up(parent_cfg(land=True), 3)
        cm = make_model(_at(K_SHAPE), "hip")
        csim = Simulation(cm, Δt=DTC, stop_time=0.0)
        start_from_parent(csim, psim)
        psim.stop_time = 1e9
        pairs.append((pm, psim, cm, csim))
    (pm, psim, cm, csim), (pm2, psim2, cm2, csim2) = pairs
    t0 = pm.clock.time
    centre = lambda t: (x_c + 2.0 * C_DX * (t - t0) / DT, y_c - 1.0 * C_DX * (t - t0) / DT)      # two child nodes east, one south per parent step
    legs = []
    boxes = run_following(csim, psim, centre, stop_time=t0 + 3 * DT, nest=dict(side="rim", ratio=3), on_leg=lambda k, s: legs.append((k, s.model.clock.time)))
    assert legs == [(k, t0 + k * DT) for k in range(3)]
    assert boxes == [(t0 + k * DT, C_X0 + 2 * k * C_DX, C_Y0 - k * C_DX) for k in range(4)]
    for k in range(3):
        _leg(csim2, psim2, 1)
        move_child(csim2, psim2, (2, -1), keep_margin=1)
    assert (cm.clock.iteration, cm2.clock.iteration, pm.clock.iteration, pm2.clock.iteration) == (9, 9, 6, 6)
    assert_same_bits(np.asarray(cm.grid.data.x), np.asarray(cm2.grid.data.x), "both boxes stand at the same place")
    _assert_same_model(_everything(cm), _everything(cm2), "run_following vs run and move_child by hand: the child")
    _assert_same_model(_everything(pm), _everything(pm2), "run_following vs run and move_child by hand: the parent")
    _assert_same_blob(cm, cm2, "run_following vs by hand")
    for m in (cm, pm):
        assert np.isfinite(m.backend.get_state()).all()


# ---- 8. refusals ----
def test_refusals_leave_both_contexts_usable():
    def seeded(cfg):
        m = make_model(cfg, "hip")
        initialize_simulation(Simulation(m, Δt=DT, stop_time=1.0))
        return m

    mask = np.ones(K_SHAPE, dtype=bool)
    mask[30:32, 4] = False
    land_cfg = _at(K_SHAPE)
    land_cfg.model["grid"] = TwoDCartesianGridMesh(C_X0, C_X0 + C_DX * 69, 70, C_Y0, C_Y0 + C_DX * 8, 9, mask=mask)
    pm, cm, pm2, cm2, land, late, held = (seeded(c) for c in (parent_cfg(), _at(K_SHAPE), parent_cfg(), _at(K_SHAPE), land_cfg, _at(K_SHAPE), _at(K_SHAPE)))
    for m in (pm, cm, pm2, cm2, land, held):
        m.backend.run_steps(DT, 2)
    late.backend.run_steps(DT, 1)
    tables = prolong_tables(pm.grid, translated(cm.grid, 2, 1))
    steps = [0]

    def refused(match, code, *args, child=cm, step=True):
        with pytest.raises(K.PiclesError, match=match) as e:
            child.backend.nest_relocate(pm.backend, *args)
        assert e.value.code == code
        if step:
            for m in (pm, cm):
                m.backend.run_steps(DT, 1)
            steps[0] += 1
            late.backend.run_steps(DT, 1)
            land.backend.run_steps(DT, 1)

    def bad(k, at, value):
        t2 = [a.copy() for a in tables]
        t2[k][at] = value
        return t2

    # a child that still holds a forcing set, and one that holds a nest on it (a context of its own: a set that comes and goes
    # leaves the rim's particles to the forcing, which is no business of this call)
    nodes, corner_nodes, index, weights = _geometry(pm, held)
    held.backend.bforce_init(nodes)
    refused("still holds a forcing set", -5, 2, 1, 1, *tables, DTC, child=held, step=False)
    held.backend.nest_init(pm.backend, corner_nodes, index, weights)
    refused("still holds a nest", -5, 2, 1, 1, *tables, DTC, child=held, step=False)
    held.backend.nest_free()
    held.backend.bforce_free()
    held.backend.nest_relocate(pm.backend, 2, 1, 1, *tables, DTC)          # the leg ended: the same call goes through
    held.backend.run_steps(DT, 1)
    refused("dt must be positive", -2, 2, 1, 1, *tables, 0.0)
    refused("lies outside the parent's grid", -2, 2, 1, 1, *bad(0, 3, 64), DTC)
    refused("lies outside the parent's grid", -2, 2, 1, 1, *bad(4, 8, -1), DTC)
    refused("not finite or lies outside", -2, 2, 1, 1, *bad(2, 5, np.nan), DTC)
    refused("keep_margin must be >= 0", -2, 2, 1, -1, *tables, DTC)
    refused("land nodes", -5, 2, 1, 1, *tables, DTC, child=land)
    refused("clock.*differ", -2, 2, 1, 1, *tables, DTC, child=late)
    with pytest.raises(ValueError, match="must hold"):
        cm.backend.nest_relocate(pm.backend, 2, 1, 1, tables[0][:-1], *tables[1:], DTC)
    with pytest.raises(ValueError, match="integer of 32 bits"):
        cm.backend.nest_relocate(pm.backend, 2 ** 31, 1, 1, *tables, DTC)
    for m in (pm2, cm2):
        m.backend.run_steps(DT, steps[0])
    _assert_same_model(_everything(cm), _everything(cm2), "the child after the refusals vs an untouched twin")
    _assert_same_model(_everything(pm), _everything(pm2), "the parent after the refusals vs an untouched twin")
    for m in (land, late, held):
        assert np.isfinite(m.backend.get_state()).all()
    # and the call itself goes through afterwards, twice, with shifts far beyond the box included
    for shift in ((2, 1), (2 ** 31 - 1, -2 ** 31)):
        Sc, Sp = cm.backend.get_state(), pm.backend.get_state()
        cm.backend.nest_relocate(pm.backend, *shift, 1, *tables, DTC)
        assert cm.backend.clock == pm.backend.clock
        new_grid = translated(_at(K_SHAPE).model["grid"], 2, 1)
        assert_same_bits(cm.backend.get_state(), relocate_state(Sc, Sp, pm.grid, new_grid, shift=shift, keep_margin=1), "after the refusals", nan_payload=True)
        for m in (pm, cm):
            m.backend.run_steps(DT, 1)
