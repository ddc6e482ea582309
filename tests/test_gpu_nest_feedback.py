"""Two-way nesting on the GPU (picles_nest_feedback_*, k_nest_restrict in picles_amd/csrc/k_nest.h, NestForcing(feedback=True)): the
level the parent's set holds is `restrict_records` of the child's State bit for bit, from a pending step's records and from State in
memory alike; the device route equals a host route through the public API; neither model leaves the fused path; feedback is neutral
where the child adds nothing and lowers the parent's energy in the lee of land only the child sees; the parent's writers see what
get_state shows; the refusals leave two usable contexts.

The boxes are those of tests/test_gpu_nesting.py: (P) 64 x 16 periodic at 6 km and (Pn) its non-periodic twin; children at 2 km
placed at (31 km, 17 km): (F) 70 x 21, ragged rows, k_step — 57 feedback nodes at margin 2; (V) 128 x 24, k_step_waverow — 152;
(B) 88 x 37 — 270 at margin 1: two workgroups of the restrict stage and a ragged tail (270 = 4 * 64 + 14), 36 entries per node."""
import math

import numpy as np
import pytest

from picles_amd import _capi as K
from picles_amd.boundary_forcing import node_points, rim_nodes
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import NestForcing, locate_in_parent, restrict_records, restriction_stencil
from picles_amd.run_statistics import StatisticsWriter
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter, read_station_output
from helpers import assert_same_bits, make_model
from test_gpu_boundary_forcing import _assert_same_model, _box, _everything
from test_gpu_nesting import DEFAULT_SOLVER, _geometry, _seeded
from test_nesting_host import C_DX, C_X0, C_Y0, P_DX, P_SHAPE, child_cfg, parent_cfg

pytestmark = pytest.mark.gpu

DT = 600.0
F_SHAPE, V_SHAPE, B_SHAPE = (70, 21), (128, 24), (88, 37)
CHILD_LAND = (slice(20, 40), slice(10, 24))          # child nodes x 71..109 km, y 37..63 km: ten parent nodes lose every entry


def pn_cfg():
    """(Pn): P's non-periodic twin"""
    cfg = parent_cfg()
    cfg.model["grid"] = TwoDCartesianGridMesh(P_DX * (P_SHAPE[0] - 1), P_SHAPE[0], P_DX * (P_SHAPE[1] - 1), P_SHAPE[1], periodic_boundary=(False, False))
    cfg.model["periodic_boundary"] = False
    return cfg


def child_land_cfg(shape, land):
    cfg = child_cfg(shape)
    nx, ny = shape
    mask = np.ones(shape, dtype=bool)
    mask[land] = False
    cfg.model["grid"] = TwoDCartesianGridMesh(C_X0, C_X0 + C_DX * (nx - 1), nx, C_Y0, C_Y0 + C_DX * (ny - 1), ny, mask=mask, periodic_boundary=(False, False))
    return cfg


def _wet(S):
    with np.errstate(all="ignore"):
        return np.isfinite(S).all(axis=-1) & (S[..., 0] > 0.0) & (S[..., 1] * S[..., 1] + S[..., 2] * S[..., 2] > 0.0)


# ---- 1. the level is the definition ----
@pytest.mark.parametrize("land", [False, True], ids=["P", "P-child-land"])
def test_level_is_restrict_records_bit_for_bit(land):
    pm = _seeded(parent_cfg(), DT)
    cm = _seeded(child_land_cfg(B_SHAPE, CHILD_LAND) if land else child_cfg(B_SHAPE), DT / 3)
    pb, cb = pm.backend, cm.backend
    nodes, corner_nodes, cindex, cweights = _geometry(pm, cm)
    cb.bforce_init(nodes)
    cb.nest_init(pb, corner_nodes, cindex, cweights)
    cb.nest_sample()
    fb, src, index, weight = restriction_stencil(pm.grid, cm.grid, 1)
    n_fb, m = index.shape
    assert n_fb == 270 and n_fb > 256 and n_fb % 64 != 0 and m == 36
    cb.nest_feedback_init(fb, src, index, weight)
    assert cb.nest_feedback_info() == (n_fb, len(src), m, 0) and pb.bforce_info()[:2] == (n_fb, 0)
    with pytest.raises(K.PiclesError, match="no levels yet"):
        pb.run_steps(DT, 1)                       # the parent's set has no level before the first feedback

    def check(what):
        got = pb.bforce_get_levels()[0]           # behind the restrict's event; completes nobody's step
        assert pb.bforce_info()[1:] == (1, cb.clock, cb.clock)
        S = cb.get_state()                        # (completes the child's step: after the level was read back)
        want = restrict_records(S[src[:, 0], src[:, 1]], index, weight)
        assert_same_bits(got, np.ascontiguousarray(want), what)
        assert np.array_equal(np.isnan(got).any(axis=1), np.isnan(got).all(axis=1))
        dry = ((~_wet(S[src[:, 0], src[:, 1]]))[index] & (weight > 0.0)).sum(axis=1)
        return got, dry, (weight > 0.0).sum(axis=1)

    nan_nodes = []
    for rnd in range(4):
        if rnd:                                   # the seed is taken from State in memory, the others with the child's step pending
            pb.run_steps(DT, 1)
            cb.nest_sample()
            cb.run_steps(DT / 3, 3)
        cb.nest_feedback()
        got, dry, full = check(f"level {rnd} against restrict_records")
        nan_nodes.append(int(np.isnan(got[:, 0]).sum()))
        assert cb.nest_feedback_info()[3] == rnd + 1
    print(f"land={land}: NaN nodes per level {nan_nodes}; feedback nodes that lose some / all entries {int(((dry > 0) & (dry < full)).sum())} / {int((dry == full).sum())}")
    if land:
        assert ((dry > 0) & (dry < full)).any() and (dry == full).sum() >= 1 and nan_nodes[-1] == int((dry == full).sum()) >= 1
    else:
        assert not dry.any() and nan_nodes == [0, 0, 0, 0]
    # once more from State in memory (get_state completed the child's step): the other slot, the same bits
    cb.nest_feedback()
    again, _, _ = check("taken from State in memory")
    assert_same_bits(again, got, "pending records vs State in memory")
    assert cb.nest_feedback_info()[3] == 5
    pb.run_steps(DT, 1)                           # and the parent steps under it
    assert np.isfinite(pb.get_state()).all()


# ---- 2. the device route against the host route ----
def _host_route(shape, solver):
    """the public API only: a twin of Pn with a band set on the feedback nodes whose level is uploaded per parent step from the child's
    State read back, the child under nest_init / nest_sample against that twin"""
    dt = DT / 3
    pm, cm = make_model(pn_cfg(), "hip"), make_model(child_cfg(shape, solver), "hip")
    for mdl, step in ((cm, dt), (pm, DT)):
        initialize_simulation(Simulation(mdl, Δt=step, stop_time=1.0))
        mdl.upload_winds(mdl.clock.time, step)
    pb, cb = pm.backend, cm.backend
    nodes = np.asarray(rim_nodes(cm.grid, "rim", 2))
    corner_nodes, cindex, cweights = locate_in_parent(pm.grid, node_points(cm.grid, nodes))
    fb, src, index, weight = restriction_stencil(pm.grid, cm.grid, 2)
    cb.bforce_init_band(nodes)
    cb.nest_init(pb, corner_nodes, cindex, cweights)
    cb.nest_sample()
    pb.bforce_init_band(fb)
    for _ in range(4):
        S = cb.get_state()
        pb.bforce_set_levels(pb.clock, restrict_records(S[src[:, 0], src[:, 1]], index, weight))
        pb.run_steps(DT, 1)
        cb.nest_sample()
        cb.run_steps(dt, 3)
    pb.bforce_free()
    cb.nest_free()
    cb.bforce_free()
    return _everything(cm), _everything(pm), len(fb)


def _device_route(shape, solver, timing=False):
    dt = DT / 3
    pm, cm = make_model(pn_cfg(), "hip"), make_model(child_cfg(shape, solver), "hip")
    psim, csim = Simulation(pm, Δt=DT, stop_time=3 * DT), Simulation(cm, Δt=dt, stop_time=11 * dt)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3, width=2, feedback=True)
    if timing:
        pm.backend.enable_timing(True)
        cm.backend.enable_timing(True)
    run(csim)
    return pm, cm, f


@pytest.mark.parametrize("shape,solver,n_fb", [(F_SHAPE, "DP5", 57), (V_SHAPE, "DP5", 152), (F_SHAPE, DEFAULT_SOLVER, 57)],
                         ids=["F70x21-k_step", "V128x24-waverow", "F70x21-default-solver"])
def test_device_route_equals_host_route(shape, solver, n_fb):
    pm, cm, f = _device_route(shape, solver)
    assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps, f.feedbacks) == (12, 4, 4, 5) and len(f.fb_nodes) == n_fb
    childA, parentA = _everything(cm), _everything(pm)
    childB, parentB, n = _host_route(shape, solver)
    assert n == n_fb
    _assert_same_model(parentA, parentB, "the parent: NestForcing(feedback=True) vs the host route")
    _assert_same_model(childA, childB, "the child: NestForcing(feedback=True) vs the host route")
    # the feedback is seen: the parent differs from the parent beside a one-way child
    pm1, cm1 = make_model(pn_cfg(), "hip"), make_model(child_cfg(shape, solver), "hip")
    csim1 = Simulation(cm1, Δt=DT / 3, stop_time=11 * DT / 3)
    csim1.output_writers["boundary_forcing"] = NestForcing(cm1, parent=Simulation(pm1, Δt=DT, stop_time=3 * DT), side="rim", ratio=3, width=2)
    run(csim1)
    i, j = f.fb_nodes[:, 0], f.fb_nodes[:, 1]
    assert not np.array_equal(pm1.backend.get_state()[i, j], parentA[0][i, j])
    assert np.isfinite(parentA[0]).all() and (parentA[0][i, j, 0] > 0.0).all()


# ---- 3. nobody left the fused path ----
def test_nobody_left_the_fused_path():
    """counted as tests/test_gpu_nesting.py counts: one fused launch per step, and at most the one stand-alone scatter that completes
    the last step when the sets are freed.  A nest_feedback that waited for the host or completed a step would show as a scatter
    launch per parent step"""
    pm, cm, f = _device_route(V_SHAPE, "DP5", timing=True)
    child, parent = cm.backend.get_timing(), pm.backend.get_timing()
    print(child, parent)
    assert child["advance_launches"] == 12 and child["scatter_launches"] <= 1, child
    assert parent["advance_launches"] == 4 and parent["scatter_launches"] <= 1, parent
    assert f.parent_steps == 4 and f.uploads == 5 and f.feedbacks == 5


# ---- 4, 5. the coincident nest: swell through a calm box, every source term off ----
CP_SHAPE = (128, 16)
COL0, ROW0 = 40, 2
CBAR, THETA, N_STEPS = 8.0, 0.15, 10                 # 2.4 cells a step at Δt = 600 s
TX, TY = CBAR * DT / C_DX * math.cos(THETA), CBAR * DT / C_DX * math.sin(THETA)
BLOCK = (slice(30, 34), slice(3, 6))                 # child land, 4 x 3 nodes: parent columns 70..73, rows 5..7
_SWELL = {}


def _swell(kind):
    """The box of tests/test_gpu_nesting_band.py (_coincident): 128 x 16 calm, sources off; the child the parent's own sub-box of
    70 x 9 nodes, same dx and Δt, ratio 1, width 3, ten steps.  The parent of a fed model cannot carry a forcing set of its own, so
    the swell is not forced through the west column but starts in the box: e = 1 at 8 m/s and 0.15 rad on columns 1..60, whose front
    crosses the feedback nodes (row 6, columns 44..105) during the run.  The child sits on rows 2..10 and columns 40..109, not 8..77:
    the swell's trailing edge travels 24 columns in ten steps and must not reach the child's band — a band node bears no particle
    while the LATER level of its pair is NaN (include/picles_hip.h, "the birth"), which is what a node the trailing edge has just
    left shows, so a one-way child loses the tail, measured: off by 3.7e-01 of the parent behind it after six steps.  kind: "alone" (the parent alone), "one-way" / "two-way"
    (the child with BLOCK as land), "neutral" (two-way, the child without land).  Returns the parent's final State; computed once"""
    if kind in _SWELL:
        return _SWELL[kind]
    nx, ny = CP_SHAPE
    S0 = np.zeros((nx, ny, 3))
    S0[1:61, 1:ny - 1] = (1.0, 1.0 / (2.0 * CBAR) * math.cos(THETA), 1.0 / (2.0 * CBAR) * math.sin(THETA))
    pm = make_model(_box(CP_SHAPE, calm=True), "hip")
    psim = Simulation(pm, Δt=DT, stop_time=(N_STEPS - 1) * DT)
    initialize_simulation(psim)
    pm.backend.set_state(S0)
    pm.backend.remesh(DT)                             # the particles of that State (branch A)
    info = None
    if kind == "alone":
        run(psim)
    else:
        cfg = _box((70, 9), calm=True)
        mask = np.ones((70, 9), dtype=bool)
        if kind != "neutral":
            mask[BLOCK] = False
        cfg.model["grid"] = TwoDCartesianGridMesh(COL0 * C_DX, (COL0 + 69) * C_DX, 70, ROW0 * C_DX, (ROW0 + 8) * C_DX, 9, mask=mask,
                                                  periodic_boundary=(False, False))
        cm = make_model(cfg, "hip")
        csim = Simulation(cm, Δt=DT, stop_time=(N_STEPS - 1) * DT)
        initialize_simulation(csim)
        Sc = S0[COL0:COL0 + 70, ROW0:ROW0 + 9].copy()
        Sc[~mask] = 0.0
        cm.backend.set_state(Sc)
        cm.backend.remesh(DT)
        f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=1, width=3, feedback=kind != "one-way")
        if f.feedback:
            assert f.feedback_margin == 4 and f.fb_index.shape[1] == 1 and (f.fb_weights == 1.0).all()
            assert np.array_equal(f.fb_nodes, np.stack([np.arange(COL0 + 4, COL0 + 66), np.full(62, 6)], axis=1))
            assert np.array_equal(f.src_nodes[f.fb_index[:, 0]] + [COL0, ROW0], f.fb_nodes)
        run(csim)
        assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps) == (N_STEPS,) * 3
        info = f.feedbacks
    _SWELL[kind] = (pm.backend.get_state(), info)
    return _SWELL[kind]


# largest |e_two-way - e_alone| / max e_alone over the parent's columns 44..127 of the test below, measured on an MI355X: all 1176
# nodes agree to the bit (max e_parent 1.000000e+00, the front at column 83, 11 levels taken)
NEUTRAL_MEASURED = 0.0
# e_two-way / e_alone at the parent's lee nodes (76, 6) and (77, 6) of the test after it, measured on an MI355X: 0.2917 against 0.8945
LEE_MEASURED = 0.326


def test_feedback_is_neutral_where_the_child_adds_nothing():
    """The child is the parent's own sub-box: what it hands back on row 6, columns 44..105 is the parent's own State, and with the
    sources off the fresh controller memory of a reborn particle does not show.  Zero is expected; the bound is 1e-4, by the
    position-rounding argument of test_coincident_nest_deeper_into_the_child (tests/test_gpu_nesting.py).  A level that arrives a
    step late, or lands in the slot the parent does not read, hands the front back 2.4 columns behind where it is"""
    (Sa, _), (St, taken) = _swell("alone"), _swell("neutral")
    ea, et = Sa[COL0 + 4:, 1:-1, 0], St[COL0 + 4:, 1:-1, 0]
    scale = ea.max()
    rel = float(np.abs(et - ea).max()) / scale
    front = int((Sa[:, 6, 0] > 0.5).nonzero()[0].max())
    print(f"neutral feedback: max e_parent {scale:.6e}; two-way off by {rel:.3e}; bitwise equal nodes {int((et == ea).sum())} of {ea.size}; "
          f"front at column {front}; levels taken {taken}")
    assert taken == N_STEPS + 1 and scale > 0.5 and COL0 + 4 < front < COL0 + 65          # the front stands among the feedback nodes
    assert rel <= 1e-4


def test_feedback_matters_where_the_child_sees_more():
    """The child carries a land block of 4 x 3 nodes — parent columns 70..73, rows 5..7 — that the parent's mask lacks.
    One-way the parent is the parent alone, to the bit.  Two-way the parent loses energy in the lee.  The fraction, from the block's
    width and the travel alone: a particle moves TX = 2.37 columns and TY = 0.36 rows a step, so what a node (c, 6) holds after a step
    was deposited by the particles of columns floor(c - TX) and floor(c - TX) + 1, on row 5 (share TY) and row 6 (share 1 - TY).
    State is what was deposited, on land too, so the wet rule sees the child's land nodes that upstream particles reach (columns
    70..72) as sea; the level is NaN where the child's State is zero: on the block's last column, whose sources are land (73), and on
    the child's lee columns whose two source columns lie on the block (74, 75: width 4 > TX + 1).  Those parent nodes bear no
    particle, so the parent's nodes whose two row-6 sources are among them — c = 76, 77 — keep the row-5 share alone: at most TY =
    0.36 of what the parent alone holds there (row 5 holds no more than row 6: the box is eroded from the south).  Asserted: less
    than half.  Upwind of the child's footprint nothing changes, to the bit.
    Measured on an MI355X: LEE_MEASURED"""
    (Sa, _), (S1, _), (S2, taken) = _swell("alone"), _swell("one-way"), _swell("two-way")
    assert_same_bits(S1, Sa, "the parent beside a one-way child vs the parent alone")
    first, last = COL0 + BLOCK[0].start, COL0 + BLOCK[0].stop - 1
    src = lambda c: {math.floor(c - TX), math.floor(c - TX) + 1}
    block = set(range(first, last + 1))
    empty = {c for c in block if src(c) <= block} | {c for c in range(last + 1, last + 5) if src(c) <= block}
    lee = [c for c in range(last + 1, last + 9) if src(c) <= empty]
    assert sorted(empty) == [73, 74, 75] and lee == [76, 77] and TY < 0.4
    assert np.isnan(S2[sorted(empty), 6, 0]).sum() == 0 and (S2[[74, 75], 6, 0] < Sa[[74, 75], 6, 0]).all()
    ea, e2 = Sa[lee, 6, 0], S2[lee, 6, 0]
    print(f"lee columns {lee}: parent alone {ea.tolist()}, two-way {e2.tolist()}, ratio {(e2 / ea).tolist()} (derived: at most {TY:.3f}); levels taken {taken}")
    assert (ea > 0.1).all()
    assert (e2 <= 0.5 * ea).all()
    assert_same_bits(S2[:COL0], Sa[:COL0], "the parent's columns upwind of the child's footprint")
    assert np.isfinite(S2).all()


# ---- 6. the parent's writers ----
def test_the_parents_writers_see_the_fed_parent(tmp_path):
    pm, cm = make_model(pn_cfg(), "hip"), make_model(child_cfg(F_SHAPE), "hip")
    psim, csim = Simulation(pm, Δt=DT, stop_time=3 * DT), Simulation(cm, Δt=DT / 3, stop_time=11 * DT / 3)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3, width=2, feedback=True)
    fed = set(map(tuple, f.fb_nodes))
    nodes = [tuple(f.fb_nodes[0]), tuple(f.fb_nodes[len(fed) // 2]), (int(f.fb_nodes[0, 0]) - 1, int(f.fb_nodes[0, 1])), (3, 3)]
    assert [p in fed for p in nodes] == [True, True, False, False]
    psim.output_writers["stations"] = StationWriter(pm, points=node_points(pm.grid, nodes), path=tmp_path, format="npy")
    sw = psim.output_writers["statistics"] = StatisticsWriter(pm, fields=("mean",), schedule=1, window=1, path=tmp_path, format="npy")
    run(csim)
    S = pm.backend.get_state()
    want = np.array([S[i, j] for i, j in nodes])
    assert np.isfinite(want).all() and (want[:, 0] > 0.0).all()
    out = read_station_output(tmp_path)
    assert out["iteration"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert_same_bits(np.ascontiguousarray(np.asarray(out["data"])[-1, :, :3]), want, "the last station record vs get_state")
    assert [r[3] for r in sw.records] == [1, 2, 3, 4]
    planes = sw.records[-1][0]                    # [var, y, x]: a window of one sample is that sample
    for k, name in enumerate(("e_mean", "mx_mean", "my_mean")):
        got = np.array([planes[sw.names.index(name), j, i] for i, j in nodes])
        assert_same_bits(got, np.ascontiguousarray(want[:, k]), f"statistics {name} vs get_state")


# ---- 7. refusals ----
def _nested_pair(shape=F_SHAPE):
    pm, cm = _seeded(pn_cfg(), DT), _seeded(child_cfg(shape), DT)          # (Pn: a set of the parent's own needs an open rim or a band)
    nodes, corner_nodes, cindex, cweights = _geometry(pm, cm)
    return pm, cm, (nodes, corner_nodes, cindex, cweights), restriction_stencil(pm.grid, cm.grid, 2)


def _step_both(pb, cb):
    """both by DT: the clocks stay equal, and the child stays inside the pair its nest holds"""
    pb.run_steps(DT, 1)
    cb.nest_sample()
    cb.run_steps(DT, 1)
    assert np.isfinite(pb.get_state()).all() and np.isfinite(cb.get_state()).all()


def test_refusals_leave_both_contexts_usable():
    import torch
    pm, cm, (nodes, corner_nodes, cindex, cweights), (fb, src, index, weight) = _nested_pair()
    pb, cb = pm.backend, cm.backend
    n_fb, m = index.shape

    def refused(match, *args):
        with pytest.raises(K.PiclesError, match=match) as e:
            cb.nest_feedback_init(*args)
        assert e.value.code in (-2, -5)
        with pytest.raises(K.PiclesError):
            cb.nest_feedback_info()
        with pytest.raises(K.PiclesError):
            pb.bforce_info()                      # no set was left on the parent
        _step_both(pb, cb)

    with pytest.raises(K.PiclesError, match="holds no nest"):
        cb.nest_feedback_init(fb, src, index, weight)
    with pytest.raises(K.PiclesError, match="picles_nest_feedback_init first"):
        cb.nest_feedback()
    cb.bforce_init(nodes)
    cb.nest_init(pb, corner_nodes, cindex, cweights)
    cb.nest_sample()
    _step_both(pb, cb)
    # a parent with a forcing set of its own
    pb.bforce_init_band([(5, 5)])
    pb.bforce_set_levels(pb.clock, np.array([[0.5, 0.02, 0.02]]))
    with pytest.raises(K.PiclesError, match="forcing set of its own.*not supported together"):
        cb.nest_feedback_init(fb, src, index, weight)
    _step_both(pb, cb)
    pb.bforce_free()
    refused("n_src and m must be >= 1", fb, np.zeros((0, 2), dtype=np.int64), np.zeros_like(index), weight)
    refused("n_src and m must be >= 1", fb, src, index[:, :0], weight[:, :0])
    for far in ((F_SHAPE[0], 0), (0, F_SHAPE[1]), (-1, 3)):
        s2 = src.copy(); s2[-1] = far
        refused("outside the child's grid", fb, s2, index, weight)
    for bad_at, bad in (((n_fb // 2, m - 1), len(src)), ((0, 0), -1)):
        i2 = index.copy(); i2[bad_at] = bad
        refused("lies outside \\[0, n_src", fb, src, i2, weight)
    for hostile in (np.nan, np.inf, -0.25):
        w2 = weight.copy(); w2[n_fb - 1, 2] = hostile
        refused("not finite or is negative", fb, src, index, w2)
    w2 = weight.copy(); w2[3] = 0.0
    refused("every weight of node 3 is zero", fb, src, index, w2)
    # what the parent's set refuses: a node twice, off the grid, not an ocean node (the rim is class 3)
    f2 = fb.copy(); f2[1] = f2[0]
    refused("given twice", f2, src, index, weight)
    f2 = fb.copy(); f2[0] = (P_SHAPE[0], 2)
    refused("lies outside", f2, src, index, weight)
    f2 = fb.copy(); f2[0] = (0, 0)
    refused("no ocean node of the parent", f2, src, index, weight)
    # the feedback itself; a second one; uploads to the parent's set are refused while it lives
    cb.nest_feedback_init(fb, src, index, weight)
    with pytest.raises(K.PiclesError, match="feeds back already"):
        cb.nest_feedback_init(fb, src, index, weight)
    with pytest.raises(K.PiclesError, match="no levels yet"):
        pb.run_steps(DT, 1)
    cb.nest_feedback()
    const = np.tile([0.5, 0.02, 0.02], (n_fb, 1))
    with pytest.raises(K.PiclesError, match="nest feedback"):
        pb.bforce_set_levels(pb.clock, const)
    for b in (pb, cb):                            # slab mode stays refused on both
        with pytest.raises(K.PiclesError):
            b.set_slab_mode(True)
    _step_both(pb, cb)
    # clocks that differ: refused, nothing changed
    pb.run_steps(DT, 1)
    before = pb.bforce_info(), pb.bforce_get_levels()[0], cb.nest_feedback_info()
    with pytest.raises(K.PiclesError, match="differ") as e:
        cb.nest_feedback()
    assert e.value.code == -2
    after = pb.bforce_info(), pb.bforce_get_levels()[0], cb.nest_feedback_info()
    assert before[0] == after[0] and before[2] == after[2] == (n_fb, len(src), m, 1)
    assert_same_bits(before[1], after[1], "the level after a refused feedback", nan_payload=True)
    cb.nest_sample(); cb.run_steps(DT, 1)
    cb.nest_feedback()
    _step_both(pb, cb)
    # dropped from the child: the parent's set goes, its nodes are stepped again and carry a particle within two steps
    i, j = fb[:, 0], fb[:, 1]
    cb.nest_feedback_free()
    with pytest.raises(K.PiclesError):
        pb.bforce_info()
    with pytest.raises(K.PiclesError):
        cb.nest_feedback_info()
    assert cb.nest_info()[0] == len(corner_nodes)                 # the one-way nest stays
    _step_both(pb, cb)
    _step_both(pb, cb)
    assert (pb.get_particles()[1][i, j] == 1).all()
    # dropped from the parent, with the set
    cb.nest_feedback_init(fb, src, index, weight)
    cb.nest_feedback()
    _step_both(pb, cb)
    pb.bforce_free()
    with pytest.raises(K.PiclesError):
        cb.nest_feedback_info()
    with pytest.raises(K.PiclesError, match="picles_nest_feedback_init first"):
        cb.nest_feedback()
    _step_both(pb, cb)
    # nest_free and bforce_free on the child release the feedback first
    for drop in (cb.nest_free, cb.bforce_free):
        cb.nest_feedback_init(fb, src, index, weight)
        cb.nest_feedback()
        _step_both(pb, cb)
        drop()
        with pytest.raises(K.PiclesError):
            pb.bforce_info()
        with pytest.raises(K.PiclesError):
            cb.nest_feedback_info()
        if drop == cb.nest_free:
            cb.nest_init(pb, corner_nodes, cindex, cweights)
            cb.nest_sample()
    pb.run_steps(DT, 1)
    assert np.isfinite(pb.get_state()).all()
    # a parent that has run on a caller's stream
    xp, xc = _seeded(parent_cfg(), DT), _seeded(child_cfg(F_SHAPE), DT)
    xc.backend.bforce_init(nodes)
    xc.backend.nest_init(xp.backend, corner_nodes, cindex, cweights)
    xc.backend.nest_sample()
    s = torch.cuda.Stream()
    xp.backend.begin_step(DT, K.STEP_ZERO_FIRST)
    xp.backend.advance_rows(K.ROWS_ALL, s.cuda_stream)
    torch.cuda.synchronize()
    xp.backend.scatter_remesh()
    with pytest.raises(K.PiclesError, match="caller-provided streams"):
        xc.backend.nest_feedback_init(fb, src, index, weight)
    xp.backend.run_steps(DT, 1)
    xc.backend.run_steps(DT, 1)
    assert np.isfinite(xp.backend.get_state()).all() and np.isfinite(xc.backend.get_state()).all()


def test_destroying_the_parent_detaches_the_feedback():
    pm, cm, (nodes, corner_nodes, cindex, cweights), (fb, src, index, weight) = _nested_pair()
    pb, cb = pm.backend, cm.backend
    cb.bforce_init(nodes)
    cb.nest_init(pb, corner_nodes, cindex, cweights)
    cb.nest_sample()
    cb.nest_feedback_init(fb, src, index, weight)
    cb.nest_feedback()
    _step_both(pb, cb)
    cb.run_steps(DT, 1)                           # a step pending, and a restrict in flight behind it
    with pytest.raises(K.PiclesError, match="differ"):
        cb.nest_feedback()
    pb.run_steps(DT, 1)
    cb.nest_sample()
    cb.nest_feedback()
    pb.close()                                    # picles_destroy(parent) with the feedback attached
    with pytest.raises(K.PiclesError, match="parent context was destroyed"):
        cb.nest_feedback()
    assert cb.nest_feedback_info() == (len(fb), len(src), index.shape[1], 2)
    cb.run_steps(DT, 1)                           # under the levels the nest kept
    assert np.isfinite(cb.get_state()).all()
    cb.nest_feedback_free()
    cb.nest_free()
    cb.bforce_set_levels(cb.clock, np.tile([0.5, 0.02, 0.02], (len(nodes), 1)))
    cb.run_steps(DT, 1)
    assert np.isfinite(cb.get_state()).all()
