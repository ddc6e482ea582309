"""Exact restart of a nested pair on the GPU (picles_nest_set_levels, NestForcing under a Checkpointer and `pickup=`):
a pair stopped one step past a parent level, two steps past one and exactly on one and picked up into fresh contexts equals the
uninterrupted run bit for bit, both models; the pair comes back to the bit, NaN levels included; the parent's writers continue their
series; nobody leaves the fused path; the contract of the new call.

The boxes are those of tests/test_nesting_host.py: parent (P) 64 x 16 periodic at 6 km (P-land: with its 3 x 3 land block, Pn: open),
children (W) 128 x 12, (K) 70 x 9 and (F) 70 x 21 at 2 km; parent step 600 s, ratio 3; 14 child steps, a checkpoint every 4."""
import numpy as np
import pytest

from picles_amd import _capi as K
from picles_amd.checkpointing import Checkpointer, checkpoint_path, list_checkpoints, read_checkpoint_file
from picles_amd.nesting import NestForcing, link_path, parent_checkpoint_path, rim_points, start_from_parent
from picles_amd.output_writers import OutputWriter
from picles_amd.run_statistics import StatisticsWriter, read_statistics
from picles_amd.simulations import Simulation, run
from picles_amd.station_output import StationWriter, read_station_output
from helpers import assert_same_bits, make_model
from test_gpu_boundary_forcing import _assert_same_model, _everything
from test_gpu_nest_feedback import F_SHAPE, pn_cfg
from test_gpu_nest_lattice import L
from test_gpu_nesting import DEFAULT_SOLVER, _dry_corners, _geometry, _seeded
from test_nest_lattice_host import under
from test_nesting_host import K_SHAPE, W_SHAPE, child_cfg, parent_cfg

pytestmark = pytest.mark.gpu

DT, RATIO = 600.0, 3
DTC = DT / RATIO
N_CHILD, EVERY = 14, 4
STOPS = (4, 8, 12)          # one step past a parent level, two steps past one, exactly on one
SPIN = 6                    # parent steps in front of a child started late

# name -> (parent configuration, child configuration, NestForcing's keywords, parent steps in front of start_from_parent)
CASES = {
    "W-DP5": (lambda: parent_cfg(), lambda: child_cfg(W_SHAPE), {}, 0),
    "K-default-solver": (lambda: parent_cfg(), lambda: child_cfg(K_SHAPE, DEFAULT_SOLVER), {}, 0),
    "W-width3-linear": (lambda: parent_cfg(), lambda: child_cfg(W_SHAPE), dict(width=3, weights="linear"), 0),
    "F-two-way": (lambda: pn_cfg(), lambda: child_cfg(F_SHAPE), dict(width=2, feedback=True), 0),
    "K-lattice-on-both": (lambda: under(parent_cfg(), L(900)), lambda: under(child_cfg(K_SHAPE), L(900)), {}, 0),
    "K-started-late": (lambda: parent_cfg(land=True), lambda: child_cfg(K_SHAPE), {}, SPIN),
}


def _pair(case, ckdir, n_child=N_CHILD, fresh=True):
    """fresh contexts of a case with the NestForcing attached and the child's Checkpointer; fresh=False: the cold start of the
    case — for a child started late the parent's spin-up and start_from_parent (a picked-up pair needs neither)"""
    pcfg, ccfg, kw, spin = CASES[case]
    pm, cm = make_model(pcfg(), "hip"), make_model(ccfg(), "hip")
    psim = Simulation(pm, Δt=DT, stop_time=(spin - 1) * DT)
    csim = Simulation(cm, Δt=DTC, stop_time=spin * DT + (n_child - 1) * DTC)
    if spin and not fresh:
        run(psim)
        start_from_parent(csim, psim)
    psim.stop_time = 1e9
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=RATIO, **kw)
    csim.output_writers["checkpointer"] = Checkpointer(cm, schedule=EVERY, dir=ckdir, prefix="c")
    return pm, psim, cm, csim, f


# ---- 1. stopped and picked up equals uninterrupted ----
@pytest.mark.parametrize("case", list(CASES))
def test_stopped_and_picked_up_equals_uninterrupted(case, tmp_path):
    spin = CASES[case][3]
    pm, psim, cm, csim, f = _pair(case, tmp_path, fresh=False)
    run(csim)
    n_parent = -(-N_CHILD // RATIO)
    assert (cm.clock.iteration, pm.clock.iteration, f.parent_steps, f.uploads) == (N_CHILD, spin + n_parent, n_parent, n_parent + 1)
    child, parent = _everything(cm), _everything(pm)
    assert sorted(list_checkpoints(tmp_path, "c")) == list(STOPS) and len(f.pairs_written) == 3
    assert np.isfinite(child[0]).all() and (child[0][..., 0] > 0.0).any()          # a child with a sea state
    for it in STOPS:
        cf = checkpoint_path(tmp_path, "c", it)
        _, ptime, pit, _ = read_checkpoint_file(parent_checkpoint_path(cf))
        assert (pit, ptime) == (spin + -(-it // RATIO), (spin + -(-it // RATIO)) * DT)       # the parent's own clock: t1 of the pair
        pm2, psim2, cm2, csim2, f2 = _pair(case, tmp_path / f"again{it}")          # new contexts; its own later checkpoints go elsewhere
        run(csim2, pickup=cf)
        what = f"{case}, picked up at child iteration {it}"
        assert (cm2.clock.iteration, pm2.clock.iteration, cm2.clock.time, pm2.clock.time) == (cm.clock.iteration, pm.clock.iteration, cm.clock.time, pm.clock.time), what
        assert (f2.parent_steps, f2.uploads, f2.feedbacks) == (f.parent_steps, f.uploads, f.feedbacks), what
        _assert_same_model(_everything(cm2), child, what + ": the child")
        _assert_same_model(_everything(pm2), parent, what + ": the parent")
        assert cm2.backend.clock == cm.backend.clock and pm2.backend.clock == pm.backend.clock


# ---- 2. the pair comes back to the bit, NaN included ----
class _Spy(OutputWriter):
    """reads the pair the child holds: at the run's begin (behind the forcing's begin_run) and at the iterations asked for
    (behind the Checkpointer); bforce_get_levels completes no step"""

    kind = "spy"
    needs = "bforce_get_levels"

    def __init__(self, at=()):
        self.at, self.seen, self.begun = set(at), {}, None

    def _read(self, b):
        return b.bforce_info(), b.bforce_get_levels(), b.nest_info()

    def begin_run(self, model, n_steps):
        self.begun = self._read(model.backend)

    def at_iteration(self, model, writers):
        if model.clock.iteration in self.at:
            self.seen[model.clock.iteration] = self._read(model.backend)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_pair_comes_back_to_the_bit_nan_included(tmp_path):
    CASES["W-under-P-land"] = (lambda: parent_cfg(land=True), lambda: child_cfg(W_SHAPE), {}, 0)
    try:
        pm, psim, cm, csim, f = _pair("W-under-P-land", tmp_path)
        spy = csim.output_writers["spy"] = _Spy(STOPS)
        run(csim)
        for it in STOPS:
            cf = checkpoint_path(tmp_path, "c", it)
            pm2, psim2, cm2, csim2, f2 = _pair("W-under-P-land", tmp_path / f"again{it}", n_child=it + 1)
            spy2 = csim2.output_writers["spy"] = _Spy()

            class Dry(OutputWriter):          # the parent as loaded, before anybody steps: its State is level 1's source
                kind, needs = "dry", "get_state"
                def begin_run(self, model, n_steps, pm2=pm2, f2=f2):
                    self.dry = _dry_corners(pm2, f2.corner_nodes, f2.index)
            dry = csim2.output_writers["dry"] = Dry()
            run(csim2, pickup=cf)
            (info, (v0, v1), nest), (info0, (u0, u1), nest0) = spy2.begun, spy.seen[it]
            p_it = -(-it // RATIO)
            assert info == info0 == (len(f.nodes), 2, (p_it - 1) * DT, p_it * DT) and nest == (len(f.corner_nodes), 2)
            with np.load(link_path(cf)) as z:
                assert (float(z["t0"]), float(z["t1"])) == info[2:]
                for got, kept, ran, name in ((v0, z["v0"], u0, "level 0"), (v1, z["v1"], u1, "level 1")):
                    assert np.array_equal(_bits(got), _bits(kept)), f"iteration {it}: {name} against the side-car"
                    assert np.array_equal(_bits(got), _bits(ran)), f"iteration {it}: {name} against the uninterrupted run's"
            nan0, nan1 = np.isnan(v0).all(axis=1), np.isnan(v1).all(axis=1)
            print(f"iteration {it}: NaN rows {int(nan0.sum())} / {int(nan1.sum())}; child nodes by dry corners {np.bincount(dry.dry, minlength=5).tolist()}")
            assert nan0.any() and nan1.any()                                   # without a NaN level nothing is shown about NaN payloads
            assert np.array_equal(nan1, dry.dry == 4) and np.array_equal(np.isnan(v1).any(axis=1), nan1)
    finally:
        del CASES["W-under-P-land"]


# ---- 3. the parent's writers continue ----
def _written_pair(d, ckdir, n_child, window):
    pm, psim, cm, csim, f = _pair("K-default-solver", ckdir, n_child=n_child)
    psim.output_writers["stations"] = StationWriter(pm, points=rim_points(cm, side="west"), path=d, format="npy")
    psim.output_writers["statistics"] = StatisticsWriter(pm, fields=("peak", "mean"), window=window, path=d, format="npy")
    return pm, psim, cm, csim, f


@pytest.mark.parametrize("window", [2, None], ids=["windows-of-2", "one-open-window"])
def test_the_parents_writers_continue(window, tmp_path):
    stop = 8                                                 # two steps past a level: the parent stands at iteration 3
    *_, csim, f = _written_pair(tmp_path / "whole", tmp_path / "whole", N_CHILD, window)
    run(csim)
    *_, csim, f = _written_pair(tmp_path / "parts", tmp_path / "parts", stop, window)
    run(csim)
    pm2, psim2, cm2, csim2, f2 = _written_pair(tmp_path / "parts2", tmp_path / "parts2", N_CHILD, window)
    cf = checkpoint_path(tmp_path / "parts", "c", stop)
    assert (tmp_path / "parts" / (parent_checkpoint_path(cf).name + ".stats.npz")).is_file()      # the side-car lands next to the parent's file
    run(csim2, pickup=cf)
    assert (cm2.clock.iteration, pm2.clock.iteration) == (N_CHILD, 5)
    whole, first, second = (read_station_output(tmp_path / d) for d in ("whole", "parts", "parts2"))
    assert whole["iteration"].tolist() == [0, 1, 2, 3, 4, 5] and first["iteration"].tolist() == [0, 1, 2, 3]
    assert second["iteration"].tolist() == [3, 4, 5]          # the restored state's record, then the series continued
    keep = second["iteration"] > 3
    assert_same_bits(np.concatenate([first["data"], second["data"][keep]]), np.asarray(whole["data"]), "stations: stopped + picked up vs uninterrupted")
    assert np.concatenate([first["time"], second["time"][keep]]).tolist() == whole["time"].tolist()
    assert_same_bits(np.asarray(second["data"][0]), np.asarray(first["data"][3]), "the record of the restored parent")
    whole, first, second = (read_statistics(tmp_path / d) for d in ("whole", "parts", "parts2"))
    if window is None:
        # the window open at the checkpoint went through the side-car: the picked-up run's one record is the uninterrupted run's
        assert whole["iteration"].tolist() == second["iteration"].tolist() == [5.0] and first["iteration"].tolist() == [3.0]
        for k in ("data", "t_start", "t_end", "n_samples"):
            assert_same_bits(np.asarray(second[k]), np.asarray(whole[k]), f"statistics {k}: the open window, picked up")
        assert not np.array_equal(first["data"], whole["data"])
    else:
        assert whole["iteration"].tolist() == [2.0, 4.0, 5.0] and first["iteration"].tolist() == [2.0, 3.0] and second["iteration"].tolist() == [4.0, 5.0]
        done = first["iteration"] < 3                        # (the stopped run's last record is its open window, cut short by the stop)
        assert_same_bits(np.concatenate([first["data"][..., done], second["data"]], axis=-1), np.asarray(whole["data"]), "statistics: stopped + picked up")
        for k in ("t_start", "t_end", "n_samples"):
            assert np.concatenate([first[k][done], second[k]]).tolist() == whole[k].tolist(), k


# ---- 4. nobody left the fused path ----
def test_nobody_left_the_fused_path_across_checkpoints(tmp_path):
    """counted as tests/test_gpu_nesting.py counts.  12 child steps, 4 parent steps, checkpoints at child iterations 4, 8 and 12: one
    fused launch per step as without a Checkpointer, and per checkpoint the two flushes picles_checkpoint_begin makes — the stand-alone
    scatter that completes the child's pending step, and the parent's (the parent stands one fused step ahead at each of the three).
    The last step of either model is completed by the checkpoint at 12: no further scatter when the run ends.  Reading the pair
    (picles_bforce_get_levels) completes nothing"""
    pm, psim, cm, csim, f = _pair("W-DP5", tmp_path, n_child=12)
    psim.output_writers["stations"] = StationWriter(pm, points=rim_points(cm, side="rim"), path=tmp_path, format="npy")
    pm.backend.enable_timing(True)
    cm.backend.enable_timing(True)
    run(csim)
    child, parent = cm.backend.get_timing(), pm.backend.get_timing()
    print(child, parent)
    assert child["advance_launches"] == 12 and child["scatter_launches"] == 3, child
    assert parent["advance_launches"] == 4 and parent["scatter_launches"] == 3, parent
    assert f.parent_steps == 4 and f.uploads == 5 and len(f.pairs_written) == 3
    assert read_station_output(tmp_path)["iteration"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


# ---- 5. the new call's contract ----
def _step_both(pb, cb, const):
    """a step of both contexts; a child whose nest holds no pair takes it under an uploaded level"""
    pb.run_steps(DT, 1)
    if cb.bforce_info()[1] == 0:
        cb.nest_free()
        cb.bforce_set_levels(cb.clock, const)
    cb.run_steps(DTC, 1)
    assert np.isfinite(pb.get_state()).all() and np.isfinite(cb.get_state()).all()


def test_nest_set_levels_contract():
    import torch
    pm, cm = _seeded(parent_cfg(land=True), DT), _seeded(child_cfg(K_SHAPE), DTC)
    pb, cb = pm.backend, cm.backend
    nodes, corner_nodes, index, weights = _geometry(pm, cm)
    n = len(nodes)
    const = np.tile([0.5, 0.02, 0.02], (n, 1))
    geometry = (corner_nodes, index, weights)

    def fresh_nest():
        cb.bforce_free()
        cb.bforce_init(nodes)
        cb.nest_init(pb, *geometry)

    # a real pair to put back: two samples around a parent step
    cb.bforce_init(nodes)
    cb.nest_init(pb, *geometry)
    cb.nest_sample()
    pb.run_steps(DT, 1)
    cb.nest_sample()
    (_, _, t0, t1), (v0, v1) = cb.bforce_info(), cb.bforce_get_levels()
    assert (t0, t1) == (0.0, DT) and cb.nest_info() == (len(corner_nodes), 2)

    def refused(match, *args, child=cb, parent=pb):
        before = child.bforce_info()
        with pytest.raises(K.PiclesError, match=match) as e:
            child.nest_set_levels(*args)
        assert e.value.code == -2 and child.bforce_info() == before
        _step_both(parent, child, const)

    refused("has taken 2 sample", t0, v0, t1, v1)                     # a nest that has sampled already
    cb.nest_free()
    refused("picles_nest_init first", t0, v0, t1, v1)                 # a child without a nest
    # (the parent's clock moves with every refusal's step: the pair that fits a fresh nest is named by it)
    def pair_now():
        fresh_nest()
        return pb.clock - DT, v0, pb.clock, v1
    a0, _, a1, _ = pair_now()
    for hostile in (np.nan, np.inf, -np.inf):
        refused("must be finite", hostile, v0, a1, v1)
        a0, _, a1, _ = pair_now()
    refused("must be finite", a0, v0, np.nan, v1)
    a0, _, a1, _ = pair_now()
    refused("needs t1 > t0", a1, v0, a1, v1)
    a0, _, a1, _ = pair_now()
    refused("needs t1 > t0", a1 + DT, v0, a1, v1)
    a0, _, a1, _ = pair_now()
    refused("is not t1", a0, v0, a1 + DT, v1)                          # level 1 is the parent's State at ITS clock
    a0, _, a1, _ = pair_now()
    refused("is not t1", a0 - DT, v0, a1 - DT, v1)
    a0, _, a1, _ = pair_now()
    planes = np.ascontiguousarray(v0.T)
    for args in ((None, K.dptr(planes)), (K.dptr(planes), None)):      # a level missing: below the binding, which always passes two
        rc = cb.lib.picles_nest_set_levels(cb.h, a0, args[0], a1, args[1])
        with pytest.raises(K.PiclesError, match="both levels must be given") as e:
            cb._ck(rc, "picles_nest_set_levels")
        assert rc == e.value.code == -2 and cb.bforce_info()[1] == 0
        _step_both(pb, cb, const)
        a0, _, a1, _ = pair_now()
    with pytest.raises(K.PiclesError, match="picles_nest_free first"):  # uploads stay refused with a nest
        cb.bforce_set_levels(a0, const)

    # the call itself: the pair verbatim, NaN payloads included; two samples; the next sample waits for the parent and rotates
    w0, w1 = v0.copy(), v1.copy()
    w0.view(np.uint64)[3] = 0x7FF8_0000_DEAD_BEEF                     # a NaN with a payload, and a negative one
    w1.view(np.uint64)[5] = 0xFFF0_0000_0000_0001
    assert np.isnan(v1).all(axis=1).any()                              # (P-land: real NaN rows too)
    cb.nest_set_levels(a0, w0, a1, w1)
    assert cb.bforce_info() == (n, 2, a0, a1) and cb.nest_info() == (len(corner_nodes), 2)
    g0, g1 = cb.bforce_get_levels()
    assert np.array_equal(_bits(g0), _bits(w0)) and np.array_equal(_bits(g1), _bits(w1))
    with pytest.raises(K.PiclesError, match="has taken 2 sample"):
        cb.nest_set_levels(a0, w0, a1, w1)
    with pytest.raises(K.PiclesError, match="has not moved past"):
        cb.nest_sample()
    cb.nest_free()
    fresh_nest()
    cb.nest_set_levels(a0, v0, a1, v1)
    # the child's clock lies far behind the parent's by now: it steps inside the pair once its clock is there
    pb.run_steps(DT, 1)
    cb.nest_sample()                                                   # the third sample: rotates
    assert cb.bforce_info() == (n, 2, a1, a1 + DT) and cb.nest_info() == (len(corner_nodes), 3)
    r0, r1 = cb.bforce_get_levels()
    assert np.array_equal(_bits(r0), _bits(v1))                        # level 1 became level 0 by pointer
    pb.run_steps(DT, 1)
    cb.nest_sample()                                                   # the fourth writes the slot the put-back level 0 lay in
    q0, q1 = cb.bforce_get_levels()
    assert np.array_equal(_bits(q0), _bits(r1)) and cb.nest_info()[1] == 4
    assert np.isfinite(pb.get_state()).all()

    # a nest whose parent was destroyed
    xp, xc = _seeded(parent_cfg(), DT), _seeded(child_cfg(K_SHAPE), DTC)
    xc.backend.bforce_init(nodes)
    xc.backend.nest_init(xp.backend, *geometry)
    xp.backend.close()
    with pytest.raises(K.PiclesError, match="parent context was destroyed") as e:
        xc.backend.nest_set_levels(-DT, v0, 0.0, v1)
    assert e.value.code == -2
    xc.backend.nest_free()
    xc.backend.bforce_set_levels(0.0, const)
    xc.backend.run_steps(DTC, 1)
    assert np.isfinite(xc.backend.get_state()).all()
    # a parent that has run on a caller's stream
    xp, xc = _seeded(parent_cfg(), DT), _seeded(child_cfg(K_SHAPE), DTC)
    xc.backend.bforce_init(nodes)
    xc.backend.nest_init(xp.backend, *geometry)
    s = torch.cuda.Stream()
    xp.backend.begin_step(DT, K.STEP_ZERO_FIRST)
    xp.backend.advance_rows(K.ROWS_ALL, s.cuda_stream)
    torch.cuda.synchronize()
    xp.backend.scatter_remesh()
    with pytest.raises(K.PiclesError, match="caller-provided streams") as e:
        xc.backend.nest_set_levels(0.0, v0, DT, v1)
    assert e.value.code == -2
    _step_both(xp.backend, xc.backend, const)
