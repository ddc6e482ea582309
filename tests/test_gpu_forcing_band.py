"""Forcing bands on the GPU (picles_bforce_init_band, k_bforce.hip): a forcing set that holds ocean nodes, with an
optional blend weight per node.  A forced ocean node's particle is the interior particle of the same value, bit for bit; the node
is not stepped while the set lives and is counted once; fused steps, single steps and the plain phases agree; the blend equals the
host route that forms v = m + w (p - m) in NumPy, from State in memory and from a pending step's records alike; hostile values bear
no particle; the flags come back when the set goes and a checkpoint never carries them into another context; the refusals leave a
usable context.

The shapes are those of tests/test_gpu_boundary_forcing.py: (W) 128 x 12 qualifies for k_step_waverow and its three-deep rim band
has 804 nodes — four workgroups of k_bforce, no multiple of 64 —, (K) 70 x 9 has ragged rows, takes k_step, and its band has 438;
the 46 x 31 sphere has the per-node metric."""
import numpy as np
import pytest

from picles_amd import configs, _capi as K
from picles_amd.boundary_forcing import BoundaryForcing, band_nodes, blend, born_particles, lerp, linear_weights, rim_nodes
from picles_amd.checkpointing import Checkpointer
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.simulations import Simulation, run
from helpers import assert_bitwise, make_model
from test_gpu_boundary_forcing import DOWNWIND, DX, K_SHAPE, W_SHAPE, _assert_same_model, _box, _everything, _model, _values

pytestmark = pytest.mark.gpu

WIDTH = 3
SOLVERS = ["DP5", "Tsit5", "AutoTsit5(Rosenbrock23())"]


def _band(grid, width=WIDTH, side="rim"):
    """(nodes [n, 2], d [n], ocean [n] bool: mask class 1) of the band"""
    nodes, d = band_nodes(grid, side, width)
    nodes = np.asarray(nodes)
    return nodes, np.asarray(d), np.asarray(grid.data.mask)[nodes[:, 0], nodes[:, 1]] == 1


def _particles_equal(a, b, what):
    """(z, on, boundary, status) of two get_particles calls: on and status everywhere, z where a particle is on"""
    assert np.array_equal(a[1], b[1]), f"{what}: on"
    assert np.array_equal(a[3], b[3]), f"{what}: status"
    assert_bitwise(np.where(a[1][..., None] != 0, a[0], 0.0), np.where(b[1][..., None] != 0, b[0], 0.0), f"{what}: z")


# ---- 1. birth identity, moved inward ----
@pytest.mark.parametrize("solver", SOLVERS)
def test_forced_ocean_particle_is_the_interior_particle_of_the_same_value(solver):
    cfg = _box(K_SHAPE, solver)
    nodes, _, ocean = _band(cfg.model["grid"])
    assert len(nodes) == 2 * 3 * 70 + 2 * 3 * 3 and ocean.sum() == len(nodes) - (2 * 70 + 2 * 7)
    v = _values(len(nodes), 7)
    A, B = _model(cfg), _model(_box(K_SHAPE, solver))
    assert born_particles(v, A.minimal_state)[0].all()
    A.backend.bforce_init_band(nodes)
    A.backend.bforce_set_levels(0.0, v)
    A.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    zA, onA, _, stA = A.backend.get_particles()
    oi, oj = nodes[ocean].T
    S = np.zeros(K_SHAPE + (3,))
    S[oi, oj] = v[ocean]
    B.backend.set_state(S)
    B.backend.remesh(cfg.Δt)                 # branch A at those nodes, on a context without a set
    B.backend.advance(cfg.Δt, 0)
    zB, onB, _, stB = B.backend.get_particles()
    print(f"{solver}: {int(onA[oi, oj].sum())} of {int(ocean.sum())} forced ocean particles on; largest |x|, |y| = "
          f"{np.abs(zA[oi, oj, 3]).max():.3f}, {np.abs(zA[oi, oj, 4]).max():.3f} cells")
    assert onA[oi, oj].all() and np.array_equal(onA[oi, oj], onB[oi, oj])
    assert np.array_equal(stA[oi, oj], stB[oi, oj])
    assert_bitwise(zA[oi, oj], zB[oi, oj], "forced ocean particle vs interior particle")
    assert np.abs(zA[oi, oj, 3:]).max() > 1.0


# ---- 2. fused == single steps == plain phases ----
def _three_paths(cfg, nodes, weights, times, values, n_steps=12):
    out = []
    for path in range(3):
        m = _model(cfg())
        b = m.backend
        b.bforce_init_band(nodes, weights)
        b.bforce_set_levels(times[0], values[0], times[1], values[1])
        dt = cfg().Δt
        if path == 0:
            b.enable_timing(True)
            b.run_steps(dt, n_steps)
            timing = b.get_timing()
        elif path == 1:
            for _ in range(n_steps):
                b.time_step(dt, K.STEP_ZERO_FIRST)
                b.get_state()
        else:
            for _ in range(n_steps):
                b.advance(dt, K.STEP_ZERO_FIRST)
                b.remesh(dt)
                b.tick(dt)
        out.append(_everything(m))
    return out, timing


@pytest.mark.parametrize("case", ["W128x12", "K70x9", "sphere46x31"])
def test_fused_run_equals_single_steps_and_plain_phases_under_a_band(case):
    cfg = {"W128x12": lambda: _box(W_SHAPE), "K70x9": lambda: _box(K_SHAPE), "sphere46x31": lambda: configs.sphere_aqua(nx=46, ny=31)}[case]
    nodes, _, ocean = _band(cfg().model["grid"])
    assert ocean.any() and not ocean.all()
    dt = cfg().Δt
    th = (-np.pi, np.pi) if case == "sphere46x31" else DOWNWIND
    values = (_values(len(nodes), 1, c=(3.0, 8.0), th=th), _values(len(nodes), 2, c=(3.0, 8.0), th=th))
    (fused, single, phases), timing = _three_paths(cfg, nodes, None, (0.0, 12 * dt), values)
    print(case, len(nodes), timing, fused[4])
    if case == "W128x12":
        assert len(nodes) == 804
    assert timing["advance_launches"] == 12 and timing["scatter_launches"] <= 1, timing
    _assert_same_model(fused, single, f"{case}: run_steps vs observed single steps")
    _assert_same_model(fused, phases, f"{case}: run_steps vs advance + remesh + tick")
    # every forced node of the boxes bears a particle; on the sphere the south row does, as in tests/test_gpu_boundary_forcing.py
    assert fused[2][:, 0].all() if case == "sphere46x31" else fused[2][nodes[:, 0], nodes[:, 1]].all()


# ---- 3. a forced node is counted once ----
def test_forced_ocean_nodes_are_counted_once():
    """particles_advanced grows per step by the stepped nodes that carry a particle plus the forced nodes that bear one.  Under the
    box's wind every ocean node carries a particle from the seed on.  A set that overrode stepped particles instead of taking the
    nodes out of the step kernels' hands would count its ocean nodes twice"""
    cfg = _box(K_SHAPE)
    nx, ny = K_SHAPE
    nodes, _, ocean = _band(cfg.model["grid"])
    v = _values(len(nodes), 11, th=DOWNWIND)
    refused = [5, 100, 300]                                      # list positions that bear nothing
    v[refused] = (0.0, 0.0, 0.0)
    m = _model(cfg)
    b = m.backend
    mask = np.asarray(m.grid.data.mask)
    in_band = np.zeros((nx, ny), dtype=bool)
    in_band[nodes[:, 0], nodes[:, 1]] = True
    stepped = (mask == 1) & ~in_band
    b.bforce_init_band(nodes)
    b.bforce_set_levels(0.0, v)
    before = b.get_counters()["particles_advanced"]
    for step in range(3):
        on = b.get_particles()[1]
        assert on[stepped].all()                                 # (every one of them runs the ODE)
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        now = b.get_counters()["particles_advanced"]
        print(f"step {step + 1}: particles_advanced +{now - before}; stepped nodes {int(stepped.sum())}, born forced nodes {len(nodes) - len(refused)}")
        assert now - before == int(stepped.sum()) + len(nodes) - len(refused)
        before = now
    on = b.get_particles()[1]
    assert not on[nodes[refused, 0], nodes[refused, 1]].any()


# ---- 4. the blend against the host route ----
def test_linear_blend_equals_the_host_route_from_state_and_from_pending_records():
    cfg = _box(W_SHAPE)
    dt = cfg.Δt
    nodes, d, ocean = _band(cfg.model["grid"])
    w = linear_weights(d, WIDTH)
    assert sorted(set(w.tolist())) == [1.0 / 3.0, 2.0 / 3.0, 1.0] and (w[~ocean] == 1.0).all()
    times = (0.0, 4 * dt)
    p0, p1 = _values(len(nodes), 21, th=DOWNWIND), _values(len(nodes), 22, th=DOWNWIND)
    A, B, C = _model(cfg), _model(_box(W_SHAPE)), _model(_box(W_SHAPE))
    f = BoundaryForcing(A, side="rim", width=WIDTH, weights="linear", times=times, values=np.stack([p0, p1]))
    assert np.array_equal(f.nodes, nodes) and np.array_equal(f.node_weights, w) and f.band
    A.backend.bforce_init_band(f.nodes, f.node_weights)
    A.backend.bforce_set_levels(times[0], p0, times[1], p1)
    B.backend.bforce_init_band(nodes)
    C.backend.bforce_init_band(nodes, w)
    C.backend.bforce_set_levels(times[0], p0, times[1], p1)
    C.backend.enable_timing(True)
    C.backend.run_steps(dt, 4)                                   # nobody looks: steps 2..4 blend into the pull over pending records
    moved = 0.0
    for step in range(4):
        t = step * dt
        m = B.backend.get_state()[nodes[:, 0], nodes[:, 1]]      # the model's own State at the step's start
        p = lerp(t, times[0], p0, times[1], p1)
        v = np.where((w == 1.0)[:, None], p, blend(m, p, w[:, None]))
        moved = max(moved, float(np.abs(v - p)[w < 1.0].max()))
        B.backend.bforce_set_levels(t, v)
        for x in (A, B):
            x.backend.time_step(dt, K.STEP_ZERO_FIRST)
        assert_bitwise(A.backend.get_state(), B.backend.get_state(), f"step {step + 1}: State, device blend vs host blend")
        _particles_equal(A.backend.get_particles(), B.backend.get_particles(), f"step {step + 1}: device blend vs host blend")
    print(f"largest |v - p| on a blended node: {moved:.3e}")
    assert moved > 1e-3                                          # the blend did something
    timing = C.backend.get_timing()
    assert timing["advance_launches"] == 4 and timing["scatter_launches"] <= 1, timing
    assert_bitwise(C.backend.get_state(), B.backend.get_state(), "four fused steps, records pending throughout, vs the host route")
    _particles_equal(C.backend.get_particles(), B.backend.get_particles(), "four fused steps vs the host route")


# ---- 5. hostile values on forced ocean nodes ----
def test_hostile_values_on_ocean_nodes_bear_no_particle():
    """as tests/test_gpu_boundary_forcing.py: two good steps fill both record buffers, then thirteen hostile values go onto ocean
    nodes of the band.  The twin keeps the same band — the nodes stay unstepped in both — with values under the minimal state there"""
    cfg = _box(W_SHAPE)
    nodes, _, ocean = _band(cfg.model["grid"])
    good = _values(len(nodes), 5, th=DOWNWIND)
    nan, inf = float("nan"), float("inf")
    hostile = [(nan, 0.1, 0.1), (1.0, nan, 0.1), (1.0, 0.1, nan), (inf, 0.1, 0.1), (1.0, -inf, 0.1), (1.0, 0.1, inf), (-inf, 0.1, 0.1),
               (0.0, 0.1, 0.1), (0.0, 0.0, 0.0), (-1.0, 0.1, 0.1), (1.0, 0.0, 0.0), (1e-9, 0.1, 0.1), (1.0, 1e-6, 0.0)]
    wet = np.flatnonzero(ocean)
    refused = [int(wet[k]) for k in np.linspace(2, len(wet) - 2, len(hostile)).astype(int)]
    assert len(set(refused)) == len(hostile) and max(refused) >= 512 and ocean[refused].all()
    vA, vB = good.copy(), good.copy()
    for k, h in zip(refused, hostile):
        vA[k] = h
        vB[k] = (1e-300, 0.0, 0.0)
    A, B = _model(cfg), _model(_box(W_SHAPE))
    assert not born_particles(vA[refused], A.minimal_state)[0].any() and not born_particles(vB[refused], A.minimal_state)[0].any()
    for m in (A, B):
        m.backend.bforce_init_band(nodes)
        m.backend.bforce_set_levels(0.0, good)
        for _ in range(2):
            m.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert A.backend.get_particles()[1][nodes[:, 0], nodes[:, 1]].all()
    A.backend.bforce_set_levels(0.0, vA)
    B.backend.bforce_set_levels(0.0, vB)
    for step in range(3):
        for m in (A, B):
            m.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        SA = A.backend.get_state()
        assert np.isfinite(SA).all(), f"step {step + 1}"
        assert_bitwise(SA, B.backend.get_state(), f"step {step + 1} after the hostile values were set")
    _, on, _, st = A.backend.get_particles()
    keep = np.setdiff1d(np.arange(len(nodes)), refused)
    assert not on[nodes[refused, 0], nodes[refused, 1]].any() and not st[nodes[refused, 0], nodes[refused, 1]].any()
    assert on[nodes[keep, 0], nodes[keep, 1]].all()
    assert A.backend.get_counters() == B.backend.get_counters()


# ---- 6. free and checkpoint ----
def test_free_hands_the_ocean_nodes_back_to_the_step_kernels():
    cfg = _box(K_SHAPE)
    nodes, _, ocean = _band(cfg.model["grid"])
    oi, oj = nodes[ocean].T
    m = _model(cfg)
    b = m.backend
    boundary0 = b.get_particles()[2].copy()
    b.bforce_init_band(nodes)
    b.bforce_set_levels(0.0, np.tile([1e-300, 0.0, 0.0], (len(nodes), 1)))      # nothing is born: the band goes empty
    for _ in range(2):
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    on = b.get_particles()[1]
    assert not on[nodes[:, 0], nodes[:, 1]].any()               # not stepped, not re-seeded from the wind, while the set lives
    b.bforce_free()
    _, on, boundary, _ = b.get_particles()
    assert np.array_equal(boundary, boundary0) and not on[oi, oj].any()
    for _ in range(2):
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    _, on, boundary, st = b.get_particles()
    assert np.array_equal(boundary, boundary0)
    assert on[oi, oj].all() and (st[oi, oj] & K.ST_STEPPED).all()          # stepped again within two steps of the windy box
    assert not on[nodes[~ocean, 0], nodes[~ocean, 1]].any()      # the rim is dead again


def test_pickup_continues_a_band_run_bit_for_bit(tmp_path):
    times = np.arange(0.0, 5401.0, 1800.0)

    def sim_of(n_steps, ckpt):
        cfg = _box(K_SHAPE)
        m = make_model(cfg, "hip")
        n = len(rim_nodes(m.grid, "rim", WIDTH))
        values = np.stack([_values(n, 20 + k, th=DOWNWIND) for k in range(len(times))])
        sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1))
        sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="rim", width=WIDTH, weights="linear", times=times, values=values)
        if ckpt:
            sim.output_writers["checkpointer"] = Checkpointer(m, schedule=3, dir=tmp_path)
        return m, sim
    a, sim_a = sim_of(6, False)
    run(sim_a)
    b, sim_b = sim_of(3, True)
    run(sim_b)
    assert b.clock.iteration == 3
    c, sim_c = sim_of(6, True)
    run(sim_c, pickup=True)
    assert c.clock.iteration == 6
    _assert_same_model(_everything(a), _everything(c), "six steps straight vs three + checkpoint + fresh model + pickup, under a band set")


def test_blob_written_under_a_band_steps_the_band_in_a_context_without_one():
    cfg = _box(K_SHAPE)
    nodes, _, ocean = _band(cfg.model["grid"])
    oi, oj = nodes[ocean].T
    A, D, E = _model(cfg), _model(_box(K_SHAPE)), _model(_box(K_SHAPE))
    A.backend.bforce_init_band(nodes)
    A.backend.bforce_set_levels(0.0, np.tile([1e-300, 0.0, 0.0], (len(nodes), 1)))
    for _ in range(3):
        A.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    A.backend.checkpoint_begin()
    blob = A.backend.checkpoint_end()
    assert not A.backend.get_particles()[1][oi, oj].any()
    D.backend.checkpoint_load(blob)                              # same fingerprint: the set is no part of it
    assert not D.backend.get_particles()[1][oi, oj].any()
    for _ in range(2):
        D.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert D.backend.get_particles()[1][oi, oj].all()
    # and the other way round: a blob of a context without a set, loaded under a band set, leaves the band unstepped
    E.backend.checkpoint_begin()
    plain = E.backend.checkpoint_end()
    A.backend.checkpoint_load(plain)
    assert A.backend.get_particles()[1][oi, oj].all()            # the seeded particles of the blob
    A.backend.bforce_set_levels(0.0, np.tile([1e-300, 0.0, 0.0], (len(nodes), 1)))
    A.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert not A.backend.get_particles()[1][oi, oj].any()        # k_bforce wrote the slots: nothing born, and nobody else stepped them


# ---- 7. refusals ----
def test_band_refusals_leave_a_usable_context():
    nx, ny = K_SHAPE
    land = np.ones(K_SHAPE, dtype=bool)
    land[1:4, 3:6] = False                                       # a land block inside the three-deep band
    cfg = _box(K_SHAPE)
    cfg.model["grid"] = TwoDCartesianGridMesh(DX * (nx - 1), nx, DX * (ny - 1), ny, mask=land, periodic_boundary=(False, False))
    m = _model(cfg)
    b = m.backend
    mask = np.asarray(m.grid.data.mask)
    cls0, cls2 = [tuple(int(x) for x in np.argwhere(mask == c)[0]) for c in (0, 2)]
    helper = rim_nodes(m.grid, "rim", WIDTH)
    assert not any(mask[i, j] in (0, 2) for i, j in helper) and len(helper) < 438

    def step():
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        assert np.isfinite(b.get_state()).all()
        with pytest.raises(K.PiclesError, match="bforce_init first"):
            b.bforce_info()

    for node, text in ((cls0, "mask class 0"), (cls2, "mask class 2")):
        with pytest.raises(K.PiclesError, match=text):
            b.bforce_init_band([(0, 1), node])
        step()
    with pytest.raises(K.PiclesError, match="given twice"):
        b.bforce_init_band([(5, 5), (0, 1), (5, 5)])
    step()
    with pytest.raises(K.PiclesError, match="outside"):
        b.bforce_init_band([(5, ny)])
    step()
    for bad in (0.0, 1.5, float("nan"), -0.5, float("inf")):
        with pytest.raises(K.PiclesError, match="weight must be finite and in \\(0, 1\\]"):
            b.bforce_init_band([(0, 1), (6, 6)], [1.0, bad])
        step()
    with pytest.raises(K.PiclesError, match="is no grid-boundary node \\(mask class 1, 3 is needed\\): only the open rim can be forced"):
        b.bforce_init([(0, 1), (6, 6)])
    step()
    b.bforce_init_band(helper, np.ones(len(helper)))
    with pytest.raises(K.PiclesError, match="a boundary forcing set exists"):
        b.bforce_init_band(helper)
    with pytest.raises(K.PiclesError, match="a boundary forcing set exists"):
        b.bforce_init(rim_nodes(m.grid, "rim"))
    b.bforce_set_levels(0.0, _values(len(helper), 3, th=DOWNWIND))
    b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert np.isfinite(b.get_state()).all()
    b.bforce_free()
    step()
    per = _model(configs.bench06_box(n=16))
    with pytest.raises(K.PiclesError, match="periodic_boundary"):
        per.backend.bforce_init_band([(0, 1)])
    per.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert np.isfinite(per.backend.get_state()).all()
    slab = make_model(_box(K_SHAPE), "hip")
    slab.backend.set_slab_mode(True)
    with pytest.raises(K.PiclesError, match="slabs"):
        slab.backend.bforce_init_band([(0, 1)])
