"""The restart of a nested pair on the CPU box (picles_amd/nesting.py): over backends that keep a journal and refuse
what the library refuses (the pattern of tests/test_nesting_host.py) — the order of calls on pickup, the chunk lengths after a resume
one step past a parent level, two steps past one and exactly on one, pickup's choice among half-written trios, the side-car
refusals, and the refusals that stay."""
import struct

import numpy as np
import pytest

from picles_amd import _capi as K, models
from picles_amd.checkpointing import Checkpointer, checkpoint_path, list_checkpoints, read_checkpoint_file
from picles_amd.nesting import NestForcing, link_path, parent_checkpoint_path
from picles_amd.simulations import Simulation, run
from test_nest_feedback_host import F_SHAPE, FeedbackBackend
from test_nesting_host import K_SHAPE, NestBackend, child_cfg, parent_cfg

N_CHILD, EVERY = 14, 4
CHUNKS = [3, 1, 2, 2, 1, 3, 2]          # child chunks end on a parent level (every 3) or on a checkpoint (every 4)


class RestartBackend(FeedbackBackend):
    """FeedbackBackend + what a pair checkpoint needs: blobs that carry the clock, levels that are arrays (level k of the parent's
    clock t is t everywhere, node 1 NaN), and nest_set_levels with the library's refusals as assertions"""

    def _j(self, *e):
        if self.journal is not None:
            self.journal.append((self.name,) + e)

    def bforce_init(self, nodes):
        super().bforce_init(nodes)
        self._j("bforce_init", len(nodes))

    def nest_init(self, parent, corner_nodes, index, weights):
        super().nest_init(parent, corner_nodes, index, weights)
        self._j("nest_init")

    def nest_feedback_init(self, *a):
        super().nest_feedback_init(*a)
        self._j("nest_feedback_init")

    def _level(self, t):
        v = np.full((len(self.bf["nodes"]), 3), float(t))
        v[1] = np.nan
        return v

    def nest_sample(self):
        super().nest_sample()
        t0, _, t1, v1 = self.bf["levels"]
        self.bf["levels"] = (t0, self._level(t0), t1, None if v1 is None else self._level(t1))

    def bforce_get_levels(self):
        _, v0, _, v1 = self.bf["levels"]
        return v0, v1

    def nest_set_levels(self, t0, v0, t1, v1):
        N = self.nest
        assert N is not None and N["samples"] == 0, "nest_set_levels needs a fresh nest"
        assert np.isfinite([t0, t1]).all() and t1 > t0 and N["parent"].clock == t1, (t0, t1, N["parent"].clock)
        assert np.asarray(v0).shape == np.asarray(v1).shape == (len(self.bf["nodes"]), 3)
        self.bf["levels"] = (t0, np.array(v0), t1, np.array(v1))
        N["samples"] = 2
        self._j("nest_set_levels", t0, t1)

    def checkpoint_begin(self):
        self._snap = self.clock
        self._j("checkpoint_begin", self.clock)

    def checkpoint_end(self):
        blob = np.zeros(K.CKPT_HEADER_BYTES + 8, dtype=np.uint8)
        blob[:8] = np.frombuffer(struct.pack("<Q", K.CKPT_MAGIC), dtype=np.uint8)
        blob[48:56] = np.frombuffer(struct.pack("<d", self._snap), dtype=np.uint8)
        return blob

    def checkpoint_load(self, blob):
        self.clock = struct.unpack_from("<d", bytes(blob), 48)[0]
        self._j("checkpoint_load", self.clock)


def _pair(tmp_path, shape=K_SHAPE, ratio=3, parent_dt=600.0, backend=RestartBackend, checkpointer=True, **nest):
    pm = models.WaveGrowth2D(**parent_cfg().model, backend_factory=backend)
    cm = models.WaveGrowth2D(**child_cfg(shape).model, backend_factory=backend)
    journal = []
    for m, name in ((pm, "parent"), (cm, "child")):
        m.backend.journal, m.backend.name = journal, name
    dt = parent_dt / ratio
    psim = Simulation(pm, Δt=parent_dt, stop_time=parent_dt * 1000)
    csim = Simulation(cm, Δt=dt, stop_time=dt * (N_CHILD - 1))
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, **{"side": "rim", "ratio": ratio, **nest})
    if checkpointer:
        csim.output_writers["checkpointer"] = Checkpointer(cm, schedule=EVERY, dir=tmp_path, prefix="c")
    return pm, psim, cm, csim, f, journal


def _child_chunks(journal):
    return [e[2] for e in journal if e[:2] == ("child", "run_steps")]


@pytest.fixture()
def written(tmp_path):
    pm, psim, cm, csim, f, journal = _pair(tmp_path)
    run(csim)
    return tmp_path, f, journal


def test_a_pair_checkpoint_is_three_files_and_the_parents_stands_alone(written):
    d, f, journal = written
    assert _child_chunks(journal) == CHUNKS
    assert sorted(list_checkpoints(d, "c")) == [4, 8, 12]               # the parent's files are not seen
    assert f.pairs_written == [checkpoint_path(d, "c", i) for i in (4, 8, 12)]
    for i, p_it in ((4, 2), (8, 3), (12, 4)):          # one step past a level, two steps past one, on one: the parent's clock is t1
        cf = checkpoint_path(d, "c", i)
        pf, lf = parent_checkpoint_path(cf), link_path(cf)
        assert pf.name == f"c_parent_iteration{i}.picles" and lf.name == f"c_iteration{i}.picles.nest.npz"
        _, time, it, _ = read_checkpoint_file(pf)      # an ordinary checkpoint file with the parent's own clock and iteration
        assert (time, it) == (600.0 * p_it, p_it)
        with np.load(lf) as z:
            assert (float(z["t0"]), float(z["t1"])) == (600.0 * (p_it - 1), 600.0 * p_it)
            assert (float(z["child_time"]), int(z["child_iteration"]), float(z["parent_time"]), int(z["parent_iteration"])) == (200.0 * i, i, 600.0 * p_it, p_it)
            assert (int(z["ratio"]), bool(z["feedback"]), int(z["uploads"]), int(z["parent_steps"]), int(z["feedbacks"])) == (3, False, p_it + 1, p_it, 0)
            assert str(z["hash"]) == f.geometry_hash()
            for v, t in ((z["v0"], float(z["t0"])), (z["v1"], float(z["t1"]))):
                assert np.isnan(v[1]).all() and (np.delete(v, 1, axis=0) == t).all()
    assert not [p for p in d.iterdir() if ".tmp-" in p.name]


@pytest.mark.parametrize("it,done", [(4, 2), (8, 4), (12, 6)], ids=["one-past", "two-past", "on-level"])
def test_the_order_of_calls_on_pickup_and_the_chunks_after_it(written, it, done):
    d, f0, journal0 = written
    pm, psim, cm, csim, f, journal = _pair(d)
    run(csim, pickup=checkpoint_path(d, "c", it))
    first_parent_step = next(k for k, e in enumerate(journal) if e[:2] == ("parent", "run_steps"))
    head = [e[:2] for e in journal[:first_parent_step]]
    assert head == [("child", "checkpoint_load"), ("parent", "checkpoint_load"), ("child", "bforce_init"), ("child", "nest_init"),
                    ("child", "nest_set_levels")] + [("child", "run_steps")] * (len(head) - 5)
    assert journal[0][2] == 200.0 * it and journal[1][2] == journal[4][3] == 600.0 * (-(-it // 3))
    assert not [e for e in cm.backend.log + pm.backend.log if e[0] == "seed"]
    assert _child_chunks(journal) == CHUNKS[done:]
    # the parent steps where the uninterrupted run stepped it, and every counter ends where that run's ended
    tail = lambda j, t: [e for e in j if e[:2] == ("parent", "run_steps") and e[3] > t]
    assert tail(journal, 600.0 * (-(-it // 3))) == tail(journal0, 600.0 * (-(-it // 3)))
    assert (f.uploads, f.parent_steps, f.feedbacks) == (f0.uploads, f0.parent_steps, f0.feedbacks) == (6, 5, 0)
    assert np.array_equal(f.times, f0.times) and f._have == f0._have
    assert (cm.clock.iteration, pm.clock.iteration, pm.clock.time) == (N_CHILD, 5, 3000.0)
    # the picked-up run checkpoints on: its later trios are the uninterrupted run's
    assert sorted(list_checkpoints(d, "c")) == [4, 8, 12] and f.pairs_written == [checkpoint_path(d, "c", i) for i in (4, 8, 12) if i > it]


@pytest.mark.parametrize("it", [4, 8, 12])
def test_two_way_no_seed_feedback_and_none_before_the_first_parent_step(tmp_path, it):
    kw = dict(shape=F_SHAPE, width=2, feedback=True)
    _, _, _, csim0, f0, journal0 = _pair(tmp_path, **kw)
    run(csim0)
    pm, psim, cm, csim, f, journal = _pair(tmp_path, **kw)
    run(csim, pickup=checkpoint_path(tmp_path, "c", it))
    kinds = [e[:2] for e in journal]
    k_set, k_fb, k_step = (kinds.index(e) for e in (("child", "nest_set_levels"), ("child", "nest_feedback_init"), ("parent", "run_steps")))
    assert k_set < k_fb < k_step
    assert not [e for e in journal[:k_step - 1] if e[1] in ("nest_sample", "nest_feedback")]
    assert journal[k_step - 1][:2] == ("child", "nest_feedback") and journal[k_step + 1][:2] == ("child", "nest_sample")
    assert journal[k_step - 1][3] == journal[k_step][3] - 600.0          # on a common clock, at the step's start time
    assert (f.uploads, f.parent_steps, f.feedbacks) == (f0.uploads, f0.parent_steps, f0.feedbacks) == (6, 5, 6)


@pytest.mark.parametrize("gone", ["child", "parent", "link"])
def test_pickup_passes_over_a_half_written_trio(written, gone):
    d, _, _ = written
    cf = checkpoint_path(d, "c", 12)
    victim = {"child": cf, "parent": parent_checkpoint_path(cf), "link": link_path(cf)}[gone]
    victim.unlink()
    pm, psim, cm, csim, f, journal = _pair(d)
    run(csim, pickup=True)
    assert journal[0] == ("child", "checkpoint_load", 1600.0) and journal[1] == ("parent", "checkpoint_load", 1800.0)
    assert cm.clock.iteration == N_CHILD
    if gone != "child":          # named outright, the incomplete trio is refused with the file's name, and nothing is loaded
        victim.unlink(missing_ok=True)
        pm, psim, cm, csim, f, journal = _pair(d)
        cf.touch(exist_ok=True)
        with pytest.raises(K.CheckpointError, match=victim.name.replace(".", r"\.")):
            run(csim, pickup=cf)
        assert not journal


def test_no_complete_trio_at_all(written):
    d, _, _ = written
    for i in (4, 8, 12):
        link_path(checkpoint_path(d, "c", i)).unlink()
    *_, csim, f, journal = _pair(d)
    with pytest.raises(K.CheckpointError, match="complete"):
        run(csim, pickup=True)
    assert not journal


def test_a_sidecar_of_another_nest_is_refused_before_anything_is_loaded(written):
    d, _, _ = written
    cf = checkpoint_path(d, "c", 8)
    for what, kw in (("ratio", dict(ratio=4, parent_dt=800.0)), ("feedback", dict(feedback=True, width=2, shape=K_SHAPE)),
                     ("geometry hash", dict(side="west")), ("geometry hash", dict(width=2))):
        shape = kw.pop("shape", K_SHAPE)
        try:
            *_, csim, f, journal = _pair(d, shape=shape, **kw)
        except ValueError:
            assert what == "feedback"          # (no feedback node under the small child: the larger one then)
            *_, csim, f, journal = _pair(d, shape=F_SHAPE, **kw)
        with pytest.raises(K.CheckpointError, match=what):
            run(csim, pickup=cf)
        assert not journal, what
    # a side-car that is no side-car, and a parent's file of another iteration
    *_, csim, f, journal = _pair(d)
    good = link_path(cf).read_bytes()
    link_path(cf).write_bytes(b"not an archive")
    with pytest.raises(K.CheckpointError, match="not a link side-car"):
        run(csim, pickup=cf)
    link_path(cf).write_bytes(good)
    parent_checkpoint_path(cf).write_bytes(parent_checkpoint_path(checkpoint_path(d, "c", 4)).read_bytes())
    with pytest.raises(K.CheckpointError, match="holds the parent at iteration 2"):
        run(csim, pickup=cf)
    assert not journal


def test_the_refusals_that_stay(tmp_path):
    # a Checkpointer on the parent: the pair is checkpointed through the child's
    pm, psim, cm, csim, f, journal = _pair(tmp_path)
    psim.output_writers["checkpointer"] = Checkpointer(pm, schedule=2, dir=tmp_path, prefix="p")
    with pytest.raises(NotImplementedError, match="Checkpointer"):
        run(csim)
    del psim.output_writers["checkpointer"]
    # a backend without nest_set_levels: both texts, before anything is loaded or seeded
    pm, psim, cm, csim, f, journal = _pair(tmp_path, backend=NestBackend)
    with pytest.raises(NotImplementedError, match="Checkpointer.*picked up"):
        run(csim, pickup=str(tmp_path / "nothing.picles"))
    with pytest.raises(NotImplementedError, match="Checkpointer"):
        run(csim)
    del csim.output_writers["checkpointer"]
    with pytest.raises(NotImplementedError, match="picked up"):
        run(csim, pickup=str(tmp_path / "nothing.picles"))
    # the per-step paths stay refused with a Checkpointer that could be served
    pm, psim, cm, csim, f, journal = _pair(tmp_path)
    with pytest.raises(NotImplementedError, match="chunked path"):
        run(csim, cash_store=True)
    pm._winds_static = False
    with pytest.raises(NotImplementedError, match="static winds"):
        run(csim)
    assert not [e for e in cm.backend.log + pm.backend.log if e[0] == "seed"] and not list(tmp_path.iterdir())
