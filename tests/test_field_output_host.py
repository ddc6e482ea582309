"""Coarse wave diagnostics, host side (no GPU): the NumPy restatement of the definition in include/picles_hip.h against hand
values, and FieldWriter + run() over a fake backend that records the calls it receives."""
import math

import numpy as np
import pytest

import _diag_numpy as D
from picles_amd import configs, models
from picles_amd.checkpointing import Checkpointer, IterationInterval
from picles_amd.driver import HipModel, SCALAR_NAMES, combine_partials, diag_field_mask
from picles_amd.field_output import FieldWriter, coarse_coordinate, read_field_output
from picles_amd.simulations import Simulation, run

G, RG = 9.81, 0.85


def _state(Nx, Ny):
    return np.zeros((Nx, Ny, 3))


# ---- the restatement against hand values ----
def test_one_wet_node_hand_values():
    s = _state(1, 1)
    s[0, 0] = (1.0, 0.05, 0.0)
    f, valid = D.fields_of(s, 1, 1, G, RG)
    assert valid.all() and f.dtype == np.float32 and f.shape == (7, 1, 1)
    hs, tp, cgx, cgy, e, mx, my = (float(v) for v in f[:, 0, 0])
    assert hs == 4.0 and cgy == 0.0 and e == 1.0 and my == 0.0
    assert cgx == pytest.approx(10.0, rel=1e-6)          # (0.05 * 1) / (2 * 0.0025)
    assert mx == np.float32(0.05)
    assert tp == pytest.approx(4 * math.pi * (10 / 0.85) / 9.81, rel=1e-6) and tp == pytest.approx(15.07, abs=0.01)
    # the slow-wave floor of the peak frequency: cbar / r_g below 0.1 is held at 0.1
    s[0, 0] = (1e-4, 0.05, 0.0)
    f, _ = D.fields_of(s, 1, 1, G, RG, names=("tp",))
    assert f.shape == (1, 1, 1) and float(f[0, 0, 0]) == np.float32(4 * math.pi * 0.1 / 9.81)


def test_block_with_one_land_node_averages_over_three():
    s = _state(2, 2)
    s[0, 0] = (1.0, 0.1, 0.0)
    s[1, 0] = (2.0, 0.1, 0.0)
    s[1, 1] = (3.0, 0.1, 0.0)          # (0, 1) stays land: zeros
    (se, sx, sy, n), (xe, xx, xy) = D.cell_sums(s, 2, 2)
    assert n[0, 0] == 3.0 and se[0, 0] == 6.0 and xe[0, 0] == 3.0 and xy[0, 0] == 0.0
    f, valid = D.fields_of(s, 2, 2, G, RG, names=("e", "hs"))
    assert valid.all()
    assert float(f[1, 0, 0]) == 2.0 and float(f[0, 0, 0]) == np.float32(4.0 * math.sqrt(2.0))     # planes in FIELDS order: hs, e


def test_all_land_block_is_nan_in_every_plane():
    s = _state(4, 2)
    s[2:, :, 0] = 1.0
    s[2:, :, 1] = 0.02
    s[0, 0] = (np.nan, 1.0, 1.0)        # not finite: not wet
    s[1, 1] = (1.0, 0.0, 0.0)           # m2 == 0: not wet
    f, valid = D.fields_of(s, 2, 2, G, RG)
    assert not valid[0, 0] and valid[1, 0]
    assert np.isnan(f[:, 0, 0]).all() and np.isfinite(f[:, 1, 0]).all()
    p = D.partials_of(s, 2, 2)
    assert p.shape == (1, 7)
    assert p[0, 3] == 4.0 and p[0, 0] == 4.0 and p[0, 4] == 1.0      # n_wet, sum_e; max_e skips the NaN
    assert p[0, 5] == 1.0                                             # max_mx is over ALL nodes, the non-wet one included


def test_ragged_axis_33_nodes_by_4():
    assert D.coarse_shape(33, 33, 4, 4) == (9, 9)
    s = _state(33, 5)
    s[..., 0] = np.arange(33)[:, None] + 1.0
    s[..., 1] = 0.01
    (se, _, _, n), _ = D.cell_sums(s, 4, 5)
    assert n.shape == (9, 1) and n[8, 0] == 5.0 and n[0, 0] == 20.0       # the last cell covers one node column
    assert se[8, 0] == 5 * 33.0
    xc = coarse_coordinate(np.arange(33.0), 4)
    assert len(xc) == 9 and xc[0] == 1.5 and xc[8] == 32.0


def test_tile_tree_and_combination():
    rng = np.random.default_rng(5)
    s = _state(600, 3)
    s[..., 0] = rng.uniform(0.1, 2.0, (600, 3))
    s[..., 1] = rng.uniform(-0.1, 0.1, (600, 3))
    s[..., 2] = rng.uniform(-0.1, 0.1, (600, 3))
    p = D.partials_of(s, 1, 1)
    assert p.shape == (3 * 3, 7)                                       # 600 columns: two full tiles and one of 88
    # the tree's result is a sum of the same numbers: equal to rounding, and the integer count exactly
    assert p[:, 3].sum() == 1800 and p[2, 3] == 88
    np.testing.assert_allclose(p[:, 0].sum(), s[..., 0].sum(), rtol=1e-13)
    assert p[:, 4].max() == s[..., 0].max()
    # restated by hand for tile 0 of row 0: groups of 64 lanes, strides 32 ... 1, then the four groups in order
    v = s[:256, 0, 0].reshape(4, 64).copy()
    w = 32
    while w >= 1:
        v = v[:, :w] + v[:, w:2 * w]
        w //= 2
    assert p[0, 0] == ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]
    mine, theirs = combine_partials([p[:4], p[4:]], 600, 3), D.combine([p], 600, 3)
    assert tuple(mine) == SCALAR_NAMES
    for k in SCALAR_NAMES:
        assert mine[k] == theirs[k], k
    assert mine["mean_of_state"] == mine["sum_e"] / 1800.0
    # a zero maximum is +0.0
    z = _state(2, 2)
    z[..., 1] = -0.0
    assert not np.signbit(D.partials_of(z, 1, 1)[0, 5])


def test_field_mask_and_set_winds_tk():
    assert diag_field_mask(("hs", "tp", "cg_x", "cg_y")) == 15 and diag_field_mask("m_y") == 64 and diag_field_mask(5) == 5
    with pytest.raises(ValueError):
        diag_field_mask(("hs", "dir"))
    m = object.__new__(HipModel)           # no context: the argument check comes before any call into the library
    m.N, m.h = 4, None
    with pytest.raises(ValueError, match="tk"):
        m.set_winds(np.ones(4), np.ones(4), 0.0, np.ones(4), np.ones(4), 600.0, tk=300.0)


# ---- FieldWriter + run() over a backend that records its calls ----
class FakeBackend:
    """the surface run() uses on its fast path; every call is logged"""

    def __init__(self, g, p, o, m, mask, **kw):
        self.Nx, self.Ny = g.Nx, g.Ny
        self.log = []
        self.clock = 0.0
        self.ring = []
        self.slots = 0
        self.ckpt = None

    def set_winds(self, u0, v0, t0=0.0, *a, **k):
        self.log.append(("set_winds", t0))

    def seed(self, t0=0.0):
        self.clock = t0
        self.log.append(("seed", t0))

    def run_steps(self, dt, n):
        self.clock += n * dt
        self.log.append(("run_steps", n))

    def time_step(self, dt, flags=0):
        self.clock += dt
        self.log.append(("time_step", 1))

    def sync(self):
        pass

    def get_counters(self):
        return {"halo_overflow": 0, "dropped_nonfinite": 0}

    def diag_init(self, coarsen, fields, n_slots):
        assert self.slots == 0
        self.coarsen, self.fields, self.slots = coarsen, fields, n_slots
        self.log.append(("diag_init", coarsen, fields, n_slots))

    def diag_shape(self):
        nxc, nyc = D.coarse_shape(self.Nx, self.Ny, *self.coarsen)
        return nxc, nyc, len(self.fields), nyc, 4 * nxc * nyc * len(self.fields)

    def diag_push(self):
        assert len(self.ring) < self.slots, "push into a full ring"
        self.ring.append(self.clock)
        self.log.append(("diag_push", self.clock))

    def diag_pop(self):
        t = self.ring.pop(0)
        nxc, nyc, nf, npart, _ = self.diag_shape()
        p = np.zeros((npart, 7))
        p[0, 0] = t
        self.log.append(("diag_pop", t))
        return np.full((nf, nxc, nyc), t, dtype=np.float32), p, t

    @property
    def diag_pending(self):
        return len(self.ring)

    def checkpoint_begin(self):
        self.log.append(("checkpoint_begin", self.clock))

    def checkpoint_end(self):
        self.log.append(("checkpoint_end", self.clock))
        return np.zeros(300, dtype=np.uint8)


def _fake_sim(n_steps, n=12):
    cfg = configs.bench06_box(n=n)
    m = models.WaveGrowth2D(**cfg.model, backend_factory=FakeBackend)
    return m, Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1)), cfg.Δt


def test_run_chunks_end_on_output_iterations(tmp_path):
    m, sim, dt = _fake_sim(23)
    fw = sim.output_writers["fields"] = FieldWriter(m, schedule=IterationInterval(5), path=tmp_path, coarsen=(4, 4), format="npy")
    run(sim)
    log = m.backend.log
    assert [c[1] for c in log if c[0] == "run_steps"] == [5, 5, 5, 5, 3]
    assert [c for c in log if c[0] == "diag_init"] == [("diag_init", (4, 4), ("hs", "tp", "cg_x", "cg_y"), 3)]
    times = [k * 5 * dt for k in range(5)]
    assert [c[1] for c in log if c[0] == "diag_push"] == times
    assert [c[1] for c in log if c[0] == "diag_pop"] == times                    # in order
    # nothing is popped before the ring is full: the first pop comes directly before the fourth push
    kinds = [c[0] for c in log if c[0] in ("diag_push", "diag_pop")]
    assert kinds == ["diag_push"] * 3 + ["diag_pop", "diag_push", "diag_pop", "diag_push"] + ["diag_pop"] * 3
    assert m.clock.iteration == 23 and m.clock.time == 23 * dt and fw.iterations == [0, 5, 10, 15, 20]
    out = read_field_output(tmp_path)
    assert out["data"].shape == (23 // 5 + 1, 3, 3, 4) and out["data"].dtype == np.float32
    assert out["time"] == times and out["var_names"] == ["hs", "tp", "cg_x", "cg_y"] and out["scalar_names"] == list(SCALAR_NAMES)
    for k, t in enumerate(times):
        assert (out["data"][k] == np.float32(t)).all() and out["scalars"][k, 0] == t
        assert out["scalars"][k, 7] == t / 144.0                                 # mean_of_state = sum_e / (Nx Ny)
    x = m.grid.data.x[:, 0]
    assert out["x"] == [x[0:4].mean(), x[4:8].mean(), x[8:12].mean()]


def test_run_chunks_end_on_output_or_checkpoint_whichever_is_first(tmp_path):
    m, sim, dt = _fake_sim(20)
    sim.output_writers["checkpointer"] = Checkpointer(m, schedule=3, dir=tmp_path / "ck")
    sim.output_writers["fields"] = FieldWriter(m, schedule=5, path=tmp_path, coarsen=(2, 3), fields=("hs", "e"), format="npy", slots=2)
    run(sim)
    log = m.backend.log
    assert [c[1] for c in log if c[0] == "run_steps"] == [3, 2, 1, 3, 1, 2, 3, 3, 2]
    assert [c[1] for c in log if c[0] == "checkpoint_begin"] == [k * dt for k in (3, 6, 9, 12, 15, 18)]
    assert [c[1] for c in log if c[0] == "diag_push"] == [k * dt for k in (0, 5, 10, 15, 20)]
    out = read_field_output(tmp_path)
    assert out["data"].shape == (5, 6, 4, 2) and out["time"] == [k * dt for k in (0, 5, 10, 15, 20)]
    assert len(list((tmp_path / "ck").glob("*.picles"))) == 6


def test_run_without_a_writer_takes_the_calls_it_took(tmp_path):
    m, sim, dt = _fake_sim(7)
    run(sim)
    assert [c for c in m.backend.log if c[0] not in ("set_winds", "seed")] == [("run_steps", 7)]


def test_per_step_loop_pushes_on_schedule(tmp_path):
    """a run that cannot take the fast path (here: cash_store observes every step) pushes when schedule(iteration)"""
    m, sim, dt = _fake_sim(6)
    m.backend.get_state = lambda: np.zeros((12, 12, 3))
    m.backend.state_gen = 0
    sim.output_writers["fields"] = FieldWriter(m, schedule=2, path=tmp_path, format="npy")
    run(sim, cash_store=True)
    log = m.backend.log
    assert [c[0] for c in log if c[0] in ("time_step", "run_steps")] == ["time_step"] * 6
    assert [c[1] for c in log if c[0] == "diag_push"] == [0.0, 2 * dt, 4 * dt, 6 * dt]
    assert read_field_output(tmp_path)["data"].shape[0] == 4


def test_oracle_backend_is_refused(tmp_path):
    from helpers import make_model
    cfg = configs.example_00_minimal(n=9, L=16e3)
    m = make_model(cfg, ("pmath", 1))
    sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt)
    sim.output_writers["fields"] = FieldWriter(m, schedule=1, path=tmp_path)
    with pytest.raises(NotImplementedError, match="FieldWriter"):
        run(sim)
