"""One-way nesting on the GPU (picles_nest_*, picles_amd/csrc/k_nest.h, picles_amd/nesting.py): a level taken from the parent is the
station definition bit for bit, from a pending step's records and from State in memory alike; a child run beside its parent equals,
bit for bit, the child run afterwards from the parent's station file; neither model leaves the fused path; the parent's own output
is what it writes alone; a coincident nest reproduces the parent's propagation; the refusals leave two usable contexts.

The boxes are those of tests/test_nesting_host.py: (P) 64 x 16 periodic at 6 km, which qualifies for k_step_waverow; the children
(W) 128 x 12 — a rim of 276 nodes: two workgroups of the mix kernel, no multiple of 64 — and (K) 70 x 9 with ragged rows, at 2 km."""
import numpy as np
import pytest

from picles_amd import _capi as K
from picles_amd.boundary_forcing import BoundaryForcing, from_station_output, rim_nodes
from picles_amd.field_output import FieldWriter, read_field_output
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import NestForcing, locate_in_parent, rim_points
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter, read_station_output, station_records
from helpers import assert_same_bits, make_model
from test_gpu_boundary_forcing import _assert_same_model, _box, _everything
from test_nesting_host import C_DX, K_SHAPE, P_SHAPE, W_SHAPE, child_cfg, parent_cfg

pytestmark = pytest.mark.gpu

DT = 600.0
DEFAULT_SOLVER = "AutoTsit5(Rosenbrock23())"


def _seeded(cfg, dt):
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=dt, stop_time=1.0))
    return m


def _geometry(pm, cm, side="rim"):
    nodes = rim_nodes(cm.grid, side)
    return (nodes,) + locate_in_parent(pm.grid, rim_points(cm, side=side))


def _dry_corners(pm, corner_nodes, index):
    """per child node, how many of its four corners the wet test refuses in the parent's State as it stands"""
    S = pm.backend.get_state()[corner_nodes[:, 0], corner_nodes[:, 1]]
    with np.errstate(all="ignore"):
        wet = np.isfinite(S).all(axis=1) & (S[:, 0] > 0.0) & (S[:, 1] * S[:, 1] + S[:, 2] * S[:, 2] > 0.0)
    return (~wet[index]).sum(axis=1)


# ---- 1. the level is the station definition ----
@pytest.mark.parametrize("land", [False, True], ids=["P", "P-land"])
def test_level_is_the_station_definition_bit_for_bit(land):
    pm, cm = _seeded(parent_cfg(land=land), DT), _seeded(child_cfg(W_SHAPE), DT / 3)
    nodes, corner_nodes, index, weights = _geometry(pm, cm)
    assert len(nodes) == 276
    P = pm.ODEsettings.Parameters
    pb, cb = pm.backend, cm.backend
    cb.bforce_init(nodes)
    cb.nest_init(pb, corner_nodes, index, weights)
    assert cb.nest_info() == (len(corner_nodes), 0) and cb.bforce_info()[1] == 0
    nan_nodes = []
    for step in range(4):
        if step:
            pb.run_steps(DT, 1)                   # fused: the step stays pending while it is sampled
        cb.nest_sample()
        n, levels, t0, t1 = cb.bforce_info()
        assert (levels, t1) == (min(step + 1, 2), pb.clock) and t0 == (0.0 if step < 2 else pb.clock - DT)
        v0, v1 = cb.bforce_get_levels()
        got = v0 if step == 0 else v1
        S = pb.get_state()                        # (completes the parent's step: after the level was read back)
        want = station_records(S[corner_nodes[:, 0], corner_nodes[:, 1]].T[None], index, weights, P.get("g", 9.81), P["r_g"])[0, :, :3]
        assert_same_bits(got, np.ascontiguousarray(want), f"level {step} against station_records")
        if step >= 1:                             # the level before it: kept as level 0, from step 2 on moved there by pointer
            assert_same_bits(v0, previous, f"level 0 at step {step}")
        previous = got
        nan_nodes.append(int(np.isnan(got[:, 0]).sum()))
        assert np.array_equal(np.isnan(got).any(axis=1), np.isnan(got).all(axis=1))
    dry = _dry_corners(pm, corner_nodes, index)
    print(f"land={land}: NaN nodes per level {nan_nodes}; child nodes by dry corners {np.bincount(dry, minlength=5).tolist()}")
    if land:
        # (the seeded State of level 0 is written at every node, land included: the dry corners show from the first step on)
        assert ((dry >= 1) & (dry <= 3)).any() and (dry == 4).any()
        assert min(nan_nodes[1:]) >= 1 and nan_nodes[-1] == int((dry == 4).sum())
    else:
        assert not dry.any() and nan_nodes == [0, 0, 0, 0]
    # once more from State in memory: no step is pending now (get_state completed it), and the parent's clock has to move first
    with pytest.raises(K.PiclesError, match="has not moved past"):
        cb.nest_sample()
    cb.nest_free()
    cb.nest_init(pb, corner_nodes, index, weights)
    cb.nest_sample()
    assert_same_bits(cb.bforce_get_levels()[0], previous, "sampled from State in memory")
    assert cb.nest_info() == (len(corner_nodes), 1)


# ---- 2..4. the device route against the host route ----
def _parent_sim(tmp, shape, side, fields=True):
    """the parent with the writers both routes give it: stations at the child's forced nodes, and coarse fields"""
    pm = make_model(parent_cfg(), "hip")
    psim = Simulation(pm, Δt=DT, stop_time=3 * DT)           # run(psim): four steps
    cgrid = child_cfg(shape).model["grid"]
    child_like = type("M", (), {"grid": cgrid})
    psim.output_writers["stations"] = StationWriter(pm, points=rim_points(child_like, side=side), path=tmp, format="npy")
    if fields:
        psim.output_writers["fields"] = FieldWriter(pm, schedule=2, path=tmp, coarsen=(4, 4), format="npy")
    return pm, psim


_ROUTES = {}


def _routes(shape, ratio, solver, tmp_factory):
    """run A (NestForcing beside the parent) and run B (the parent alone, then the child from its station file), 4 parent steps;
    computed once per case and shared by the tests below, which leave it unchanged"""
    if (shape, ratio, solver) in _ROUTES:
        return _ROUTES[shape, ratio, solver]
    dt, n = DT / ratio, 4 * ratio
    out = {}
    # A
    dirA = tmp_factory.mktemp("nested")
    pm, psim = _parent_sim(dirA, shape, "rim")
    cm = make_model(child_cfg(shape, solver), "hip")
    csim = Simulation(cm, Δt=dt, stop_time=dt * (n - 1))
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=ratio)
    run(csim)
    out["A"], out["parentA"], out["nest"] = _everything(cm), _everything(pm), f
    out["clocks"] = (cm.clock.iteration, pm.clock.iteration, cm.backend.clock, pm.backend.clock)
    out["filesA"] = (read_station_output(dirA), read_field_output(dirA))
    # B
    dirB = tmp_factory.mktemp("offline")
    pm2, psim2 = _parent_sim(dirB, shape, "rim")
    run(psim2)
    out["parentB"] = _everything(pm2)
    out["filesB"] = (read_station_output(dirB), read_field_output(dirB))
    cm2 = make_model(child_cfg(shape, solver), "hip")
    csim2 = Simulation(cm2, Δt=dt, stop_time=dt * (n - 1))
    csim2.output_writers["boundary_forcing"] = from_station_output(cm2, dirB, side="rim")
    run(csim2)
    out["B"] = _everything(cm2)
    # and the child alone: what the forcing has to change
    cm3 = make_model(child_cfg(shape, solver), "hip")
    run(Simulation(cm3, Δt=dt, stop_time=dt * (n - 1)))
    out["alone"] = _everything(cm3)
    _ROUTES[shape, ratio, solver] = out
    return out


CASES = [(W_SHAPE, 3, "DP5"), (K_SHAPE, 3, "DP5"), (K_SHAPE, 1, "DP5"), (K_SHAPE, 3, DEFAULT_SOLVER)]
IDS = ["W128x12-r3", "K70x9-r3", "K70x9-r1", "K70x9-r3-default-solver"]


@pytest.mark.parametrize("shape,ratio,solver", CASES, ids=IDS)
def test_device_route_equals_host_route(shape, ratio, solver, tmp_path_factory):
    R = _routes(shape, ratio, solver, tmp_path_factory)
    assert R["clocks"][:2] == (4 * ratio, 4) and R["clocks"][2] == R["clocks"][3]
    assert np.isfinite(R["filesB"][0]["data"][..., :3]).all()         # (no land in P: every level is a value)
    _assert_same_model(R["A"], R["B"], "NestForcing vs from_station_output")
    # the forcing enters: the upwind rim columns bear particles that deposit on the rim and on the interior next to it, where the
    # child alone has an empty rim and less energy behind it
    SA, S0 = R["A"][0], R["alone"][0]
    print(f"{shape} r={ratio} {solver}: e on the west rim {SA[0, 1:-1, 0].min():.3e}..{SA[0, 1:-1, 0].max():.3e} (alone {S0[0, 1:-1, 0].max():.3e}); "
          f"next to it {SA[1, 1:-1, 0].min():.3e} (alone {S0[1, 1:-1, 0].min():.3e}..{S0[1, 1:-1, 0].max():.3e})")
    assert (S0[0, 1:-1, 0] == 0.0).all() and (SA[0, 1:-1, 0] > 0.0).all()
    assert (SA[1, 1:-1, 0] > S0[1, 1:-1, 0]).all()


def test_nobody_left_the_fused_path(tmp_path):
    """counted as test_fused_run_equals_single_steps_and_plain_phases counts: one fused launch per step, and at most the one
    stand-alone scatter that completes the last step when somebody looks.  The parent takes 4 steps: the look-ahead step behind the
    child's last window is not taken (no step of the child would read its level).  The parent writes stations, which leave a step
    pending; a FieldWriter completes the step it records, with or without a nest (picles_diag_push), so it has none here"""
    pm, psim = _parent_sim(tmp_path, W_SHAPE, "rim", fields=False)
    cm = make_model(child_cfg(W_SHAPE), "hip")
    csim = Simulation(cm, Δt=DT / 3, stop_time=11 * DT / 3)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
    pm.backend.enable_timing(True)
    cm.backend.enable_timing(True)
    run(csim)
    child, parent = cm.backend.get_timing(), pm.backend.get_timing()
    print(child, parent)
    assert child["advance_launches"] == 12 and child["scatter_launches"] <= 1, child
    assert parent["advance_launches"] == 4 and parent["scatter_launches"] <= 1, parent
    assert f.parent_steps == 4 and f.uploads == 5
    assert read_station_output(tmp_path)["iteration"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


def test_parent_is_not_disturbed(tmp_path_factory):
    R = _routes(W_SHAPE, 3, "DP5", tmp_path_factory)
    (sa, fa), (sb, fb) = R["filesA"], R["filesB"]
    assert list(sa["iteration"]) == list(sb["iteration"]) == [0.0, 1.0, 2.0, 3.0, 4.0]
    for k in ("data", "time"):
        assert_same_bits(np.asarray(sa[k]), np.asarray(sb[k]), f"stations {k}")
    assert fa["data"].shape == fb["data"].shape and fa["data"].shape[0] == 3
    assert_same_bits(np.asarray(fa["data"]), np.asarray(fb["data"]), "fields data")
    assert_same_bits(np.asarray(fa["scalars"]), np.asarray(fb["scalars"]), "fields scalars")
    _assert_same_model(R["parentA"], R["parentB"], "the parent beside a child vs the parent alone")


# ---- 5. coincident nest, propagation only ----
COINCIDENT_PARENT = (128, 16)


def _coincident(col0, cbar, dt, n_steps=10):
    """Calm box, every source term off.  The parent's west column is forced with swell of group speed `cbar`; the child is the
    parent's own sub-box, rows 2..10 and columns col0..col0+69, same dx and Δt = dt, ratio 1: every weight is 1.0 on one corner.
    Returns the largest |e_child - e_parent| / max e_parent over the child's non-rim nodes after n_steps, for the nested child and
    for the child alone"""
    nx, ny = COINCIDENT_PARENT
    pm = make_model(_box(COINCIDENT_PARENT, calm=True), "hip")
    psim = Simulation(pm, Δt=dt, stop_time=(n_steps - 1) * dt)
    e, th = 1.0, 0.15
    v = np.tile(np.array([e, e / (2.0 * cbar) * np.cos(th), e / (2.0 * cbar) * np.sin(th)]), (ny, 1))
    psim.output_writers["boundary_forcing"] = BoundaryForcing(pm, side="west", times=[0.0], values=v[None])

    def child():
        cfg = _box(K_SHAPE, calm=True)
        cfg.model["grid"] = TwoDCartesianGridMesh(col0 * C_DX, (col0 + 69) * C_DX, 70, 2 * C_DX, 10 * C_DX, 9, periodic_boundary=(False, False))
        m = make_model(cfg, "hip")
        return m, Simulation(m, Δt=dt, stop_time=(n_steps - 1) * dt)

    cm, csim = child()
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=1)
    assert np.array_equal(f.weights, np.tile([1.0, 0.0, 0.0, 0.0], (len(f.nodes), 1)))
    assert np.array_equal(f.corner_nodes[f.index[:, 0]], f.nodes + [col0, 2])
    run(csim)
    assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps) == (n_steps,) * 3
    um, usim = child()
    run(usim)
    ep = pm.backend.get_state()[col0 + 1:col0 + 69, 3:10, 0]
    ec, eu = cm.backend.get_state()[1:-1, 1:-1, 0], um.backend.get_state()[1:-1, 1:-1, 0]
    scale = ep.max()
    rel, blind = np.abs(ec - ep).max() / scale, np.abs(eu - ep).max() / scale
    print(f"coincident nest, columns {col0}..{col0 + 69}, swell at {cbar} m/s, Δt = {dt} s ({cbar * dt / C_DX:.1f} cells a step): max e_parent "
          f"{scale:.6e}; nested child off by {rel:.3e}, child alone off by {blind:.3e}; bitwise equal nodes {int((ec == ep).sum())} of "
          f"{ec.size}; columns the swell has reached {int((ep.max(axis=1) > 1e-3 * scale).sum())}")
    assert scale > 0.1 * e                    # the swell has arrived in the sub-box
    return rel, blind


# largest |e_child - e_parent| / max e_parent of the test below, measured on an MI355X: all 476 nodes agree to the bit (the parent's
# largest energy there 3.492951e-01, the child alone off by 1.000e+00).  The bound is ten times the measured value: equality
COINCIDENT_MEASURED = 0.0


def test_coincident_nest_reproduces_the_parents_propagation():
    """Swell at 8 m/s through the parent's west column; the child is the parent's sub-box on rows 2..10 and columns 8..77, same dx
    (2000 m) and Δt, ratio 1; ten steps; the child's non-rim nodes against the parent's.  The bound is ten times the difference
    measured on the GPU (COINCIDENT_MEASURED), and the child alone must miss the parent by more than a thousand times the bound —
    and, since it has no sea of its own in a calm box, by more than half of the parent's largest energy.
    (The parent is 128 x 16, not the 64 x 16 of the other tests: columns 8..77 do not fit into 64.)

    Δt is 200 s, the child step of the other tests at this spacing: 0.8 cells a step.  A forcing set bears particles at rim nodes
    only (mask class 3: the contract of picles_bforce_init), so a nest carries what is found AT a rim node at a level time.  Below
    a cell a step that is everything that enters.  At Δt = 600 s the same swell travels 2.4 cells a step: the parent's columns 9
    and 10 are then fed by particles that start on columns 6 and 7, outside the child, and cross the rim column within one step —
    measured there: nested child off by 9.872e-01 of the parent's largest energy, child alone by 1.000e+00 (DESIGN.md §18 has the
    table).  That is a limit of rim-only forcing, not of the nest, and the reason for the step chosen here."""
    rel, blind = _coincident(8, 8.0, 200.0)
    bound = 10.0 * COINCIDENT_MEASURED
    assert rel <= bound
    assert blind > 1000.0 * bound and blind > 0.5


def test_coincident_nest_deeper_into_the_child():
    """The same box with swell at 3 m/s and Δt = 600 s — 0.9 cells a step — and the child on columns 2..71, which the swell enters
    eight columns deep within ten steps.  Propagation alone has a constant right-hand side for the position, which every step size
    integrates to rounding; what can differ between a reborn rim particle and the parent's own is the rounding of a particle
    position to six digits (a weight off by at most 1e-6 per step and contribution).  Ten steps and at most four contributions per
    node stay inside 4e-5, and a difference of 1e-4 would want an explanation: that is the bound.  The child alone misses the
    parent by all of its energy: more than a thousand times the bound."""
    rel, blind = _coincident(2, 3.0, 600.0)
    bound = 1e-4
    assert rel <= bound
    assert blind > 1000.0 * bound


# ---- 6. refusals ----
def _step_both(pb, cb, dt_child):
    pb.run_steps(DT, 1)
    cb.run_steps(dt_child, 1)
    assert np.isfinite(pb.get_state()).all() and np.isfinite(cb.get_state()).all()


def test_refusals_leave_both_contexts_usable():
    import torch
    pm, cm = _seeded(parent_cfg(), DT), _seeded(child_cfg(K_SHAPE), DT)
    pb, cb = pm.backend, cm.backend
    nodes, corner_nodes, index, weights = _geometry(pm, cm)
    n, dtc = len(nodes), DT                      # both step by DT: the child's clock stays inside the pair the nest holds
    const = np.tile([0.5, 0.02, 0.02], (n, 1))

    def refused(match, *args, parent=pb, child=cb):
        with pytest.raises(K.PiclesError, match=match) as e:
            child.nest_init(parent, *args)
        assert e.value.code in (-2, -5)
        _step_both(pb, cb, dtc)

    refused("no boundary forcing set", corner_nodes, index, weights)
    cb.bforce_init(nodes)
    cb.bforce_set_levels(0.0, const)
    refused("same context", corner_nodes, index, weights, parent=cb)
    refused("n_corner must be >= 1", np.zeros((0, 2), dtype=np.int64), np.zeros_like(index), weights)
    bad = index.copy(); bad[n // 2, 3] = len(corner_nodes)
    refused("lies outside \\[0, n_corner", corner_nodes, bad, weights)
    bad = index.copy(); bad[0, 0] = -1
    refused("lies outside \\[0, n_corner", corner_nodes, bad, weights)
    for far in ((P_SHAPE[0], 0), (0, P_SHAPE[1]), (-1, 3)):
        c2 = corner_nodes.copy(); c2[-1] = far
        refused("outside the parent's grid", c2, index, weights)
    for hostile in (np.nan, np.inf):
        w2 = weights.copy(); w2[n - 1, 2] = hostile
        refused("is not finite", corner_nodes, index, w2)
    slab = make_model(parent_cfg(), "hip")
    slab.backend.set_slab_mode(True)
    refused("slab", corner_nodes, index, weights, parent=slab.backend)
    slab.backend.close()
    if torch.cuda.device_count() >= 2:
        far = make_model(parent_cfg(), "hip", device=1)
        refused("one device", corner_nodes, index, weights, parent=far.backend)
        far.backend.close()
    assert cb.bforce_info()[1] == 1              # every refusal left the uploaded level in place
    # the nest itself; a second one; uploads are refused while it exists
    cb.nest_init(pb, corner_nodes, index, weights)
    with pytest.raises(K.PiclesError, match="holds a nest"):
        cb.nest_init(pb, corner_nodes, index, weights)
    with pytest.raises(K.PiclesError, match="no levels yet"):
        cb.run_steps(dtc, 1)                      # the uploaded level went with nest_init
    cb.nest_sample()
    with pytest.raises(K.PiclesError, match="picles_nest_free first"):
        cb.bforce_set_levels(0.0, const)
    _step_both(pb, cb, dtc)
    # twice without a parent step: the second is refused and changes nothing
    cb.nest_sample()
    before = cb.bforce_info(), cb.bforce_get_levels(), cb.nest_info()
    with pytest.raises(K.PiclesError, match="has not moved past"):
        cb.nest_sample()
    after = cb.bforce_info(), cb.bforce_get_levels(), cb.nest_info()
    assert before[0] == after[0] and before[2] == after[2] == (len(corner_nodes), 2)
    for a, b in zip(before[1], after[1]):
        assert_same_bits(a, b, "levels after a refused sample", nan_payload=True)
    _step_both(pb, cb, dtc)
    # bforce_free on a nested child releases the nest; both can be made again
    cb.bforce_free()
    with pytest.raises(K.PiclesError):
        cb.nest_info()
    cb.bforce_init(nodes)
    cb.nest_init(pb, corner_nodes, index, weights)
    cb.nest_sample()
    _step_both(pb, cb, dtc)
    cb.nest_sample()
    # nest_free keeps the pair, wherever the rotation had left it, and uploads work again
    pb.run_steps(DT, 1)
    cb.nest_sample()
    pair, info = cb.bforce_get_levels(), cb.bforce_info()
    cb.nest_free()
    assert cb.bforce_info() == info
    for a, b in zip(pair, cb.bforce_get_levels()):
        assert_same_bits(a, b, "levels kept by nest_free", nan_payload=True)
    cb.bforce_set_levels(cb.clock, const)
    _step_both(pb, cb, dtc)


def test_destroying_the_parent_detaches_its_children():
    pm = _seeded(parent_cfg(), DT)
    kids = [_seeded(child_cfg(K_SHAPE), DT / 3), _seeded(child_cfg(W_SHAPE), DT / 3)]        # a parent may serve several children
    for cm in kids:
        nodes, corner_nodes, index, weights = _geometry(pm, cm, "west")
        cm.backend.bforce_init(nodes)
        cm.backend.nest_init(pm.backend, corner_nodes, index, weights)
        cm.backend.nest_sample()
    pm.backend.run_steps(DT, 1)
    for cm in kids:
        cm.backend.nest_sample()
        cm.backend.run_steps(DT / 3, 2)
    kept = [cm.backend.bforce_get_levels() for cm in kids]
    pm.backend.close()                           # picles_destroy(parent) with two children attached
    for cm, lv in zip(kids, kept):
        b = cm.backend
        b.run_steps(DT / 3, 1)                   # under the kept levels
        S = b.get_state()
        assert np.isfinite(S).all() and (S[0, 1:-1, 0] > 0.0).all()
        for a, c in zip(lv, b.bforce_get_levels()):
            assert_same_bits(a, c, "levels kept after the parent went", nan_payload=True)
        with pytest.raises(K.PiclesError, match="parent context was destroyed"):
            b.nest_sample()
        with pytest.raises(K.PiclesError, match="picles_nest_free first"):
            b.bforce_set_levels(0.0, lv[0])
        b.nest_free()
        b.bforce_set_levels(b.clock, lv[0])
        b.run_steps(DT / 3, 1)
        assert np.isfinite(b.get_state()).all()
