"""A child started from its spun-up parent, on the GPU (picles_nest_prolong, k_nest_prolong in picles_amd/csrc/k_nest.h,
nesting.start_from_parent): the child's State is `prolong_state` of the parent's bit for bit; its particles, flags,
controller memory and counters are those of a child built through the public API as seed(t), set_state(prolonged), remesh(dt), and
stay so through a nested run; under a lattice the child's particles are those under static winds set to the lattice at t; the late
nest equals its offline route; the refusals leave two usable contexts.

The boxes are those of tests/test_nesting_host.py: (P-land) 64 x 16 periodic at 6 km with its 3 x 3 land block; the children (W)
128 x 12 — 1536 nodes, six full workgroups of the kernel — and (K) 70 x 9 — 630 nodes: ragged rows and a ragged last workgroup — at
2 km, and (K) once more across the parent's periodic wrap cell; parent step 600 s, ratio 3."""
from types import SimpleNamespace

import numpy as np
import pytest

from picles_amd import _capi as K
from picles_amd.boundary_forcing import from_station_output
from picles_amd.nesting import NestForcing, prolong_state, prolong_tables, rim_points, start_from_parent
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter
from helpers import assert_same_bits, make_model
from test_gpu_boundary_forcing import _assert_same_model, _everything
from test_nest_lattice_host import WRAP_X0, lattice_winds, under
from test_nesting_host import C_X0, K_SHAPE, W_SHAPE, _winds, child_cfg, parent_cfg

pytestmark = pytest.mark.gpu

DT = 600.0
DTC = DT / 3


def _wet(S):
    with np.errstate(all="ignore"):
        return np.isfinite(S).all(axis=-1) & (S[..., 0] > 0.0) & (S[..., 1] * S[..., 1] + S[..., 2] * S[..., 2] > 0.0)


def _wet_corners(pm, cm):
    """per child node, how many of its four parent corners are wet in the parent's State as it stands"""
    ix0, ix1, _, iy0, iy1, _ = prolong_tables(pm.grid, cm.grid)
    wet = _wet(pm.backend.get_state())
    return sum(wet[a[:, None], b[None, :]].astype(int) for a in (ix0, ix1) for b in (iy0, iy1))


def _blob(m):
    """the restart blob: every prognostic plane of the context — particles, controller memory (dtn, qold, the auto-switch word),
    flags, State, the clock — in one array"""
    m.backend.checkpoint_begin()
    return np.array(m.backend.checkpoint_end())


def _spun_up(cfg, n_steps):
    pm = make_model(cfg, "hip")
    psim = Simulation(pm, Δt=DT, stop_time=(n_steps - 1) * DT)
    run(psim)
    assert pm.clock.iteration == n_steps and pm.clock.time == n_steps * DT
    return pm, psim


def _by_hand(cfg, csim_dt, t, S, stop_time):
    """the second child, through the public API: seed(t), set_state(prolonged), remesh(dt)"""
    cm = make_model(cfg, "hip")
    csim = Simulation(cm, Δt=csim_dt, stop_time=stop_time)
    cm._wind_window = None
    cm.upload_winds(t, csim_dt, seeding=True)
    cm.backend.seed(t)
    cm.backend.set_state(S)
    cm.backend.remesh(csim_dt)
    cm.clock.time, cm.clock.iteration = t, 0
    csim.initialized = True
    return cm, csim


# ---- 4. the device route is the definition ----
@pytest.mark.parametrize("shape,x0", [(K_SHAPE, C_X0), (W_SHAPE, C_X0), (K_SHAPE, WRAP_X0)], ids=["K70x9", "W128x12", "K70x9-across-the-wrap-cell"])
def test_started_child_is_the_definition_and_stays_equal_to_the_child_built_by_hand(shape, x0):
    (pm, psim), (pm2, psim2) = _spun_up(parent_cfg(land=True), 6), _spun_up(parent_cfg(land=True), 6)
    t = pm.clock.time
    stop = t + 5 * DTC                                        # six further child steps: two parent steps
    cm = make_model(child_cfg(shape, x0=x0), "hip")
    csim = Simulation(cm, Δt=DTC, stop_time=stop)
    start_from_parent(csim, psim)
    assert csim.initialized and (cm.clock.time, cm.clock.iteration, cm.backend.clock) == (t, 0, pm.backend.clock)
    Sp = pm.backend.get_state()
    want = prolong_state(Sp, pm.grid, cm.grid)
    got = cm.backend.get_state()
    assert_same_bits(got, want, "the child's State against prolong_state")
    assert_same_bits(np.asarray(cm.State), want, "the lazy view re-read")
    zeroed, nwet = (got == 0.0).all(axis=-1), _wet_corners(pm, cm)
    print(f"{shape} at x0 = {x0}: {int(zeroed.sum())} zeroed nodes, {int((~zeroed).sum())} valid; by wet corners {np.bincount(nwet.ravel(), minlength=5).tolist()}")
    assert np.array_equal(zeroed, nwet == 0) and (~zeroed).sum() > 0.9 * zeroed.size
    if x0 == C_X0:                                            # the land block lies under the child's south rim
        assert zeroed.sum() >= 3 and ((nwet > 0) & (nwet < 4)).any()
    else:
        ix0, ix1 = prolong_tables(pm.grid, cm.grid)[:2]
        assert (ix0[-1], ix1[-1]) == (63, 0) and not zeroed.any()
    # the second child
    assert_same_bits(pm2.backend.get_state(), Sp, "the twin parent")
    cm2, csim2 = _by_hand(child_cfg(shape, x0=x0), DTC, t, want, stop)
    A, B = _everything(cm), _everything(cm2)
    _assert_same_model(A, B, "start_from_parent vs seed, set_state, remesh")
    print(f"particles on: {int((A[2] != 0).sum())} of {A[2].size}; at zeroed nodes {int((A[2][zeroed] != 0).sum())} of {int(zeroed.sum())}")
    assert (A[2][1:-1, 1:-1] != 0).all()                      # every interior node bears a particle: from its State, or from the local wind
    assert np.array_equal(_blob(cm), _blob(cm2)), "restart blobs (controller memory included) differ"
    # six further child steps, nested
    for c, cs, ps in ((cm, csim, psim), (cm2, csim2, psim2)):
        ps.stop_time = 1e9
        cs.output_writers["boundary_forcing"] = NestForcing(c, parent=ps, side="rim", ratio=3)
        run(cs)
    assert (cm.clock.iteration, pm.clock.iteration, cm.clock.time) == (6, 8, t + 6 * DTC) and cm.backend.clock == pm.backend.clock
    _assert_same_model(_everything(cm), _everything(cm2), "after six nested steps: the child")
    _assert_same_model(_everything(pm), _everything(pm2), "after six nested steps: the parent")
    assert np.array_equal(_blob(cm), _blob(cm2)), "restart blobs after six nested steps differ"
    assert np.isfinite(cm.backend.get_state()).all()


# ---- 5. under a lattice ----
@pytest.mark.parametrize("n_spin", [3, 4], ids=["t1800-a-knot", "t2400-between-knots"])
def test_child_started_under_a_lattice_and_the_late_nest(n_spin, tmp_path):
    wind = lattice_winds(900.0)
    pm, psim = _spun_up(under(parent_cfg(), wind), n_spin)
    t = pm.clock.time
    stop = t + 5 * DTC
    cm = make_model(under(child_cfg(K_SHAPE), wind), "hip")
    csim = Simulation(cm, Δt=DTC, stop_time=stop)
    start_from_parent(csim, psim)
    want = prolong_state(pm.backend.get_state(), pm.grid, cm.grid)
    assert_same_bits(cm.backend.get_state(), want, "the child's State against prolong_state")
    X, Y = cm.grid.data.x, cm.grid.data.y
    u0, v0, u1, v1 = cm.backend.get_winds()
    for got, ref, what in ((u0, wind.u(X, Y, t), "u(t)"), (v0, wind.v(X, Y, t), "v(t)"), (u1, wind.u(X, Y, t + DTC), "u(t + dt)")):
        assert_same_bits(got, ref, f"the window the child was started under: {what}")
    # the second child: static winds, the lattice evaluated on the host at t
    frozen = SimpleNamespace(u=lambda x, y, _t: wind.u(x, y, t), v=lambda x, y, _t: wind.v(x, y, t))
    cfg2 = _winds(child_cfg(K_SHAPE), frozen)
    cfg2.model["winds_static"] = True
    cm2, _ = _by_hand(cfg2, DTC, t, want, stop)
    A, B = _everything(cm), _everything(cm2)
    for x, y, name in zip(A[:4], B[:4], ("State", "z", "on", "status")):
        x, y = (np.where(A[2][..., None] != 0, x, 0.0), np.where(B[2][..., None] != 0, y, 0.0)) if name == "z" else (x, y)
        assert_same_bits(x, y, f"under the lattice at t = {t} vs under static winds of that time: {name}") if x.dtype == np.float64 else np.testing.assert_array_equal(x, y)
    assert A[2].any()
    # the late nest: two parent steps beside the parent ...
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3, width=3)
    psim.stop_time = 1e9
    run(csim)
    assert (cm.clock.iteration, f.parent_steps, pm.clock.iteration) == (6, 2, n_spin + 2)
    # ... against the offline route from the same prolonged state: a twin parent run to t, the child started, the parent's nested leg
    # alone with stations at the child's band, the child from that file
    pm3, psim3 = _spun_up(under(parent_cfg(), wind), n_spin)
    cm3 = make_model(under(child_cfg(K_SHAPE), wind), "hip")
    csim3 = Simulation(cm3, Δt=DTC, stop_time=stop)
    start_from_parent(csim3, psim3)
    psim3.output_writers["stations"] = StationWriter(pm3, points=rim_points(cm3, side="rim", width=3), path=tmp_path, format="npy")
    psim3.stop_time = t + DT
    run(psim3)
    g = csim3.output_writers["boundary_forcing"] = from_station_output(cm3, tmp_path, side="rim", width=3)
    assert np.array_equal(g.times, [t, t + DT, t + 2 * DT])
    run(csim3)
    _assert_same_model(_everything(cm), _everything(cm3), "the late nest vs its offline route: the child")
    _assert_same_model(_everything(pm), _everything(pm3), "the late nest vs its offline route: the parent")
    alone = make_model(under(child_cfg(K_SHAPE), wind), "hip")
    asim = Simulation(alone, Δt=DTC, stop_time=stop)
    start_from_parent(asim, psim3)                            # (the parent has moved on: another state; it only has to differ)
    assert not np.array_equal(alone.backend.get_state(), want)


# ---- 6. refusals ----
def test_refusals_leave_both_contexts_usable():
    def seeded(cfg, dt):
        m = make_model(cfg, "hip")
        initialize_simulation(Simulation(m, Δt=dt, stop_time=1.0))
        return m

    pm, cm, pm2, cm2 = (seeded(parent_cfg(), DT), seeded(child_cfg(K_SHAPE), DT), seeded(parent_cfg(), DT), seeded(child_cfg(K_SHAPE), DT))
    for m in (pm, pm2):
        m.backend.run_steps(DT, 2)
    tables = prolong_tables(pm.grid, cm.grid)
    steps = [0]

    def refused(match, code, *args, child=cm.backend, parent=pm.backend):
        with pytest.raises(K.PiclesError, match=match) as e:
            child.nest_prolong(parent, *args)
        assert e.value.code == code
        for m in (pm, cm):
            m.backend.run_steps(DT, 1)
        steps[0] += 1

    def bad(k, at, value):
        t2 = [a.copy() for a in tables]
        t2[k][at] = value
        return t2

    refused("same context", -2, *tables, DTC, parent=cm.backend)
    slab = make_model(parent_cfg(), "hip")
    slab.backend.set_slab_mode(True)
    refused("slab", -5, *tables, DTC, parent=slab.backend)
    slab.backend.close()
    refused("lies outside the parent's grid", -2, *bad(0, 3, 64), DTC)
    refused("lies outside the parent's grid", -2, *bad(1, 69, -1), DTC)
    refused("lies outside the parent's grid", -2, *bad(4, 8, 16), DTC)
    refused("not finite or lies outside", -2, *bad(2, 5, np.nan), DTC)
    refused("not finite or lies outside", -2, *bad(5, 0, 1.5), DTC)
    refused("not finite or lies outside", -2, *bad(5, 0, np.inf), DTC)
    refused("dt must be positive", -2, *tables, 0.0)
    with pytest.raises(ValueError, match="must hold"):
        cm.backend.nest_prolong(pm.backend, tables[0][:-1], *tables[1:], DTC)
    for m in (pm2, cm2):
        m.backend.run_steps(DT, steps[0])
    _assert_same_model(_everything(cm), _everything(cm2), "the child after the refusals vs an untouched twin")
    _assert_same_model(_everything(pm), _everything(pm2), "the parent after the refusals vs an untouched twin")
    # and the call itself goes through afterwards, twice
    for _ in range(2):
        cm.backend.nest_prolong(pm.backend, *tables, DTC)
        assert cm.backend.clock == pm.backend.clock
        assert_same_bits(cm.backend.get_state(), prolong_state(pm.backend.get_state(), pm.grid, cm.grid), "after the refusals")
        pm.backend.run_steps(DT, 1)
