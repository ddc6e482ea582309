"""Two-way nesting on the CPU box (picles_amd/nesting.py): the geometry of the restriction stencil against a brute-force restatement
from the coordinates, `restrict_records` against a scalar restatement of k_nest_restrict on hostile values, the call order of
NestForcing(feedback=True) over backends that record their calls, and the refusals made before anything is seeded.

The boxes are those of tests/test_nesting_host.py, with children tall enough to hold feedback nodes."""
import math

import numpy as np
import pytest

from picles_amd import models
from picles_amd.boundary_forcing import BoundaryForcing, band_nodes
from picles_amd.checkpointing import Checkpointer
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import NestForcing, default_feedback_margin, restrict_records, restriction_stencil
from picles_amd.simulations import Simulation, run
from test_nesting_host import C_DX, C_X0, C_Y0, P_DX, NestBackend, child_cfg, parent_cfg

F_SHAPE = (70, 21)          # 57 feedback nodes at margin 2
B_SHAPE = (88, 37)          # 270 at margin 1: two workgroups of the restrict stage and a ragged tail


# ---- geometry ----
def _hat_brute(pg, cg, margin):
    """feedback nodes and, per node, [(child i, child j, weight)] in the child's row order, from the coordinates alone"""
    px, py = pg.data.x[:, 0], pg.data.y[0, :]
    cx, cy = cg.data.x[:, 0], cg.data.y[0, :]
    reach = max(margin, 1)
    out = []
    for j in range(len(py)):
        for i in range(len(px)):
            if pg.data.mask[i, j] != 1:
                continue
            if not (px[i] - reach * P_DX >= cx[0] and px[i] + reach * P_DX <= cx[-1] and py[j] - reach * P_DX >= cy[0] and py[j] + reach * P_DX <= cy[-1]):
                continue
            ent = []
            for b in range(len(cy)):
                for a in range(len(cx)):
                    w = max(0.0, 1.0 - abs(cx[a] - px[i]) / P_DX) * max(0.0, 1.0 - abs(cy[b] - py[j]) / P_DX)
                    if w > 0.0:
                        ent.append((a, b, w))
            out.append(((i, j), ent))
    return out


@pytest.mark.parametrize("shape,margin,n_fb", [(F_SHAPE, 2, 57), (F_SHAPE, 1, 21 * 5), (B_SHAPE, 1, 270)], ids=["F70x21-m2", "F70x21-m1", "B88x37-m1"])
def test_hat_weights_against_the_coordinates(shape, margin, n_fb):
    pg, cg = parent_cfg().model["grid"], child_cfg(shape).model["grid"]
    fb, src, index, weight = restriction_stencil(pg, cg, margin)
    want = _hat_brute(pg, cg, margin)
    assert len(fb) == n_fb == len(want) and index.shape == weight.shape == (n_fb, index.shape[1])
    assert [tuple(p) for p in fb] == [p for p, _ in want]                      # row by row, i fastest
    assert len(np.unique(src, axis=0)) == len(src) and np.array_equal(src, src[np.lexsort((src[:, 0], src[:, 1]))])
    m = max(len(e) for _, e in want)
    assert index.shape[1] == m and index.min() >= 0 and index.max() < len(src)
    used = set()
    for k, (_, ent) in enumerate(want):
        n = len(ent)
        assert [tuple(src[q]) for q in index[k, :n]] == [(a, b) for a, b, _ in ent], k
        assert np.array_equal(weight[k, :n], np.array([w for _, _, w in ent])), k
        assert (weight[k, n:] == 0.0).all() and (index[k, n:] == index[k, 0]).all()
        assert abs(weight[k].sum() - 9.0) < 1e-12                               # the hat of a 3:1 child sums to rs² wherever it sits
        used.update((a, b) for a, b, _ in ent)
    assert used == set(map(tuple, src))


def _grid(x0, nx, y0, ny, dx):
    return TwoDCartesianGridMesh(x0, x0 + dx * (nx - 1), nx, y0, y0 + dx * (ny - 1), ny, periodic_boundary=(False, False))


def test_coincident_child_is_injection():
    pg = _grid(0.0, 128, 0.0, 16, C_DX)
    cg = _grid(8 * C_DX, 70, 2 * C_DX, 9, C_DX)
    fb, src, index, weight = restriction_stencil(pg, cg, 1)
    assert index.shape == (len(fb), 1) and (weight == 1.0).all()
    assert np.array_equal(src[index[:, 0]] + [8, 2], fb)
    # the parent's rim (class 3) is never fed, the child's outermost nodes are never a source
    assert fb[:, 0].min() == 9 and fb[:, 0].max() == 76 and fb[:, 1].min() == 3 and fb[:, 1].max() == 9
    fb4, _, _, _ = restriction_stencil(pg, cg, 4)
    assert fb4[:, 0].min() == 12 and fb4[:, 0].max() == 73 and sorted(set(fb4[:, 1])) == [6]


@pytest.mark.parametrize("rs", [2, 3, 4])
def test_aligned_child_has_2rs_minus_1_squared_entries(rs):
    D = 6000.0
    pg = _grid(0.0, 20, 0.0, 12, D)
    cg = _grid(3 * D, 8 * rs + 1, 2 * D, 6 * rs + 1, D / rs)
    fb, src, index, weight = restriction_stencil(pg, cg, 1)
    assert len(fb) == 7 * 5 and index.shape[1] == (2 * rs - 1) ** 2 and (weight > 0.0).all()
    hat = np.array([1.0 - abs(k) / rs for k in range(-(rs - 1), rs)])
    assert np.allclose(weight[0].reshape(2 * rs - 1, 2 * rs - 1), np.outer(hat, hat), rtol=0, atol=1e-15)
    k = [tuple(p) for p in fb].index((5, 4))
    ci = src[index[k]]
    assert ci[:, 0].min() == 2 * rs - (rs - 1) and ci[:, 0].max() == 2 * rs + (rs - 1) and np.array_equal(np.unique(ci[:, 1]), np.arange(2 * rs - (rs - 1), 2 * rs + rs))


def test_margin_rule_and_the_childs_band():
    pg = parent_cfg().model["grid"]
    px, py = pg.data.x[:, 0], pg.data.y[0, :]
    for shape, width in ((F_SHAPE, 1), (F_SHAPE, 2), (B_SHAPE, 3), (B_SHAPE, 6)):
        cg = child_cfg(shape).model["grid"]
        cx, cy = cg.data.x[:, 0], cg.data.y[0, :]
        margin = default_feedback_margin(width, C_DX, P_DX)
        assert margin == 1 + math.ceil(width * C_DX / P_DX)
        fb, src, index, weight = restriction_stencil(pg, cg, margin)
        assert len(fb) > 0
        x, y = px[fb[:, 0]], py[fb[:, 1]]
        assert (x - margin * P_DX >= cx[0]).all() and (x + margin * P_DX <= cx[-1]).all()
        assert (y - margin * P_DX >= cy[0]).all() and (y + margin * P_DX <= cy[-1]).all()
        # one cell less of margin takes more nodes: the rule is sharp
        assert len(restriction_stencil(pg, cg, margin - 1)[0]) > len(fb) or margin == 1
        band = set(band_nodes(cg, "rim", width)[0])
        assert not band & set(map(tuple, src)), (shape, width)
    assert default_feedback_margin(3, 2000.0, 6000.0) == 2 and default_feedback_margin(1, 6000.0, 6000.0) == 2
    with pytest.raises(ValueError, match="margin"):
        restriction_stencil(pg, cg, -1)


def test_land_in_the_parent_is_not_fed():
    cg = child_cfg(B_SHAPE).model["grid"]
    mask = np.ones((64, 16), dtype=bool)
    mask[20:22, 8:10] = False                     # four parent nodes under the child
    pg = TwoDCartesianGridMesh(P_DX * 63, 64, P_DX * 15, 16, mask=mask, periodic_boundary=(True, True))
    fb = restriction_stencil(pg, cg, 1)[0]
    assert (np.asarray(pg.data.mask)[fb[:, 0], fb[:, 1]] == 1).all() and len(fb) <= 270 - 4
    assert not {(20, 8), (21, 9)} & set(map(tuple, fb))


# ---- the restrict arithmetic ----
def _restrict_scalar(values, index, weight):
    """k_nest_restrict, lane by lane, in Python floats (IEEE doubles, one rounding per operation)"""
    n, m = index.shape
    out = np.empty((n, 3))
    for p in range(n):
        W = SE = SX = SY = 0.0
        for c in range(m):
            w = float(weight[p, c])
            if w == 0.0:
                continue
            e, mx, my = (float(v) for v in values[index[p, c]])
            if math.isfinite(e) and math.isfinite(mx) and math.isfinite(my) and e > 0.0 and mx * mx + my * my > 0.0:
                W = W + w
                SE = SE + w * e
                SX = SX + w * mx
                SY = SY + w * my
        ok = False
        if W > 0.0:
            E, MX, MY = SE / W, SX / W, SY / W
            ok = MX * MX + MY * MY > 0.0
        out[p] = (E, MX, MY) if ok else (math.nan,) * 3
    return out


@pytest.mark.parametrize("m", [1, 4, 25])
def test_restrict_records_on_hostile_values(m):
    rng = np.random.default_rng(20 + m)
    ns, n = 60, 300
    v = np.stack([np.exp(rng.uniform(-6, 2, ns)), rng.normal(0, 0.05, ns), rng.normal(0, 0.05, ns)], axis=1)
    v[0] = (np.nan, 0.1, 0.1)
    v[1] = (1.0, np.inf, 0.1)
    v[2] = (0.0, 0.1, 0.1)
    v[3] = (1.0, 0.0, 0.0)
    v[4] = (-1.0, 0.1, 0.1)
    v[5] = (1.0, 0.1, -np.inf)
    v[6] = (1e-300, 1e-170, 1e-170)               # m² underflows to zero: dry
    v[7] = (-np.inf, 0.0, -0.0)
    index = rng.integers(0, ns, (n, m))
    index[:8] = rng.integers(0, 8, (8, m))        # all dry
    weight = rng.uniform(0.0, 1.0, (n, m))
    weight[rng.uniform(size=(n, m)) < 0.3] = 0.0  # padding anywhere
    weight[8:16, 1:] = 0.0                        # one entry carries everything
    weight[:, 0] = np.where((weight == 0.0).all(axis=1), 0.5, weight[:, 0])
    index[16:24, 0] = rng.integers(0, 8, 8)       # padding that names a hostile value next to wet entries
    weight[16:24, 0] = 0.0
    if m > 1:
        weight[16:24, 1] = 0.25
        index[16:24, 1] = rng.integers(8, ns, 8)
    got = restrict_records(v, index, weight)
    want = _restrict_scalar(v, index, weight)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)])
    assert np.isnan(got[:8]).all() and np.array_equal(np.isnan(got).any(axis=1), np.isnan(got).all(axis=1))
    if m > 1:
        assert np.isfinite(got[16:24]).all()
    # a single wet entry is that value: w e / w rounds back only where the product was exact, so the test is on the definition
    one = restrict_records(v[8:9], np.zeros((1, 1), dtype=np.int64), np.ones((1, 1)))
    assert np.array_equal(one[0], v[8])


# ---- call order ----
class FeedbackBackend(NestBackend):
    """NestBackend + the feedback: refuses what the library refuses, and tells the parent's fake that it holds a level"""

    fb = None

    def nest_feedback_init(self, fb_nodes, src_nodes, index, weights):
        assert self.nest is not None and self.fb is None
        p = self.nest["parent"]
        assert p.bf is None, "the parent holds a forcing set of its own"
        assert np.asarray(index).shape == np.asarray(weights).shape == (len(fb_nodes), np.asarray(index).shape[1])
        assert np.asarray(index).max() < len(src_nodes)
        self.fb = dict(taken=0)
        self.log.append(("nest_feedback_init", len(fb_nodes)))

    def nest_feedback(self):
        assert self.fb is not None
        p = self.nest["parent"]
        assert abs(self.clock - p.clock) <= 1e-9 * 200.0, (self.clock, p.clock)
        self.fb["taken"] += 1
        self.log.append(("nest_feedback", self.clock))
        self.journal.append((self.name, "nest_feedback", self.fb["taken"], self.clock))

    def nest_feedback_info(self):
        return 0, 0, 0, self.fb["taken"]

    def nest_feedback_free(self):
        assert self.nest is not None, "the feedback is freed before the nest"
        self.fb = None
        self.log.append(("nest_feedback_free",))

    def nest_free(self):
        assert self.fb is None, "nest_free with the feedback alive"
        super().nest_free()

    def bforce_init_band(self, nodes, weights=None):
        self.bforce_init(nodes)


def _pair(shape, n_child_steps, ratio=3, backend=FeedbackBackend):
    pm = models.WaveGrowth2D(**parent_cfg().model, backend_factory=backend)
    cm = models.WaveGrowth2D(**child_cfg(shape).model, backend_factory=backend)
    journal = []
    for m, name in ((pm, "parent"), (cm, "child")):
        m.backend.journal, m.backend.name = journal, name
    dt = 600.0 / ratio
    return pm, Simulation(pm, Δt=600.0, stop_time=600.0 * 1000), cm, Simulation(cm, Δt=dt, stop_time=dt * (n_child_steps - 1)), journal


@pytest.mark.parametrize("ratio,n_child", [(3, 12), (1, 4), (3, 11)])
def test_one_feedback_in_front_of_every_parent_step(ratio, n_child):
    pm, psim, cm, csim, journal = _pair(F_SHAPE, n_child, ratio=ratio)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=ratio, width=2, feedback=True)
    assert f.feedback_margin == 2 and len(f.fb_nodes) == 57
    run(csim)
    n_parent = -(-n_child // ratio)
    assert f.parent_steps == n_parent and f.feedbacks == 1 + n_parent
    assert [e[2] for e in journal if e[1] == "nest_feedback"] == list(range(1, n_parent + 2))
    for k, e in enumerate(journal):
        if e[0] == "parent" and e[1] == "run_steps":
            before = journal[k - 1]
            assert before[:2] == ("child", "nest_feedback") and before[3] == e[3] - 600.0, (before, e)      # at the step's start time
            assert journal[k + 1][:2] == ("child", "nest_sample")
    # the seed stands between level 0 and the first parent step
    kinds = [e[:2] for e in journal[:5]]
    assert kinds == [("child", "nest_sample"), ("child", "nest_feedback"), ("child", "nest_feedback"), ("parent", "run_steps"), ("child", "nest_sample")]
    log = [e[0] for e in cm.backend.log]
    assert [e for e in log if e in ("seed", "bforce_init", "nest_init", "nest_feedback_init")] == ["seed", "bforce_init", "nest_init", "nest_feedback_init"]
    assert log[-3:] == ["nest_feedback_free", "nest_free", "bforce_free"]
    assert sum(e[2] for e in journal if e[:2] == ("child", "run_steps")) == n_child


def test_one_way_stays_as_it_was():
    pm, psim, cm, csim, journal = _pair(F_SHAPE, 6)
    f = csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3)
    assert f.needs == "nest_init" and not f.feedback
    run(csim)
    assert not [e for e in journal if e[1] == "nest_feedback"] and not [e for e in cm.backend.log if e[0].startswith("nest_feedback")]


# ---- refusals, before anything is seeded ----
def test_feedback_refusals(tmp_path):
    pm, psim, cm, csim, _ = _pair(F_SHAPE, 6)
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3, feedback=True)
    # a parent with a forcing of its own
    psim.output_writers["boundary_forcing"] = BoundaryForcing(pm, nodes=[(3, 3)], times=[0.0], values=np.ones((1, 1, 3)))
    with pytest.raises(NotImplementedError, match="BoundaryForcing of its own"):
        run(csim)
    del psim.output_writers["boundary_forcing"]
    # the refusals of a one-way nest still hold
    with pytest.raises(NotImplementedError, match="picked up"):
        run(csim, pickup=str(tmp_path / "nothing.ckpt"))
    with pytest.raises(NotImplementedError, match="chunked path"):
        run(csim, cash_store=True)
    csim.output_writers["checkpointer"] = Checkpointer(cm, schedule=2, dir=tmp_path, prefix="c")
    with pytest.raises(NotImplementedError, match="Checkpointer"):
        run(csim)
    del csim.output_writers["checkpointer"]
    pm._winds_static = False
    with pytest.raises(NotImplementedError, match="static winds"):
        run(csim)
    assert not [e for e in cm.backend.log + pm.backend.log if e[0] == "seed"]
    # a backend without nest_feedback_init
    pm, psim, cm, csim, _ = _pair(F_SHAPE, 6, backend=NestBackend)
    csim.output_writers["boundary_forcing"] = NestForcing(cm, parent=psim, side="rim", ratio=3, feedback=True)
    with pytest.raises(NotImplementedError, match="nest_feedback_init"):
        run(csim)
    assert not [e for e in cm.backend.log + pm.backend.log if e[0] == "seed"]
    # a child too small to hold a feedback node
    pm, psim, cm, csim, _ = _pair((70, 9), 6)
    with pytest.raises(ValueError, match="no ocean node of the parent"):
        NestForcing(cm, parent=psim, side="rim", ratio=3, feedback=True)
