"""Open-boundary forcing on the GPU (picles_bforce_*, k_bforce.hip, picles_amd/boundary_forcing.py): a forced rim node's particle
is the interior particle NodeToParticle! would bear from the same value, bit for bit; fused steps, single steps and the plain phases
agree; the value follows the level pair linearly in time; what enters is conserved by the scatter; hostile values bear no particle;
probes, statistics and checkpoints see the forced particles; the refusals leave a usable context.

The shapes are the smallest that reach each launch path: (W) 128 x 12 qualifies for k_step_waverow, (K) 70 x 9 has ragged rows and
runs on k_step; the rim of (W) has 276 nodes — more than one workgroup of k_bforce and no multiple of 64."""
import math

import numpy as np
import pytest

from picles_amd import configs, _capi as K
from picles_amd.boundary_forcing import BoundaryForcing, born_particles, lerp, rim_nodes
from picles_amd.checkpointing import Checkpointer
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.particle_waves_v5 import IDConstants, particle_equations
from picles_amd.run_statistics import StatisticsWriter
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter, read_station_output
from helpers import assert_bitwise, make_model

pytestmark = pytest.mark.gpu

W_SHAPE, K_SHAPE = (128, 12), (70, 9)
DX = 2000.0


def _box(shape, solver="DP5", calm=False):
    """the physics and ODE settings of configs.bench06_box on a non-periodic nx x ny mesh, periodic_boundary = false; calm: no wind
    and every source term off — particles only propagate"""
    nx, ny = shape
    cfg = configs.bench06_box(n=16, dx=DX, periodic_grid=False)
    cfg.model["grid"] = TwoDCartesianGridMesh(DX * (nx - 1), nx, DX * (ny - 1), ny, periodic_boundary=(False, False))
    cfg.model["ODEsets"].solver = solver
    if calm:
        w = configs.const_winds(0.0, 0.0)
        cfg.model["winds"] = w
        cfg.model["ODEsys"] = particle_equations(w.u, w.v, γ=0.88, q=IDConstants.make().q, IDConstants=IDConstants.make(), input=False,
                                                 dissipation=False, peak_shift=False, direction=False)
    return cfg


def _model(cfg):
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    return m


INTO_THE_BOX = (-1.2, 1.2)          # directions of travel for a west column [rad]
DOWNWIND = (0.2, 1.3)               # ... for a whole rim under the (10, 10) wind: in through the west and south sides, out through the others


def _values(n, seed, c=(3.0, 12.0), th=(-math.pi, math.pi)):
    """(n, 3) sea states branch A accepts: e in [0.05, 4] m², |c̄| in c [m/s] — up to four cells per step —, direction in th"""
    rng = np.random.default_rng(seed)
    e = np.exp(rng.uniform(math.log(0.05), math.log(4.0), n))
    cb, th = rng.uniform(c[0], c[1], n), rng.uniform(th[0], th[1], n)
    mm = e / (2.0 * cb)
    return np.stack([e, mm * np.cos(th), mm * np.sin(th)], axis=1)


def _everything(m):
    b = m.backend
    S = b.get_state()
    z, on, _, st = b.get_particles()
    return S, z, on, st, b.get_counters()


def _assert_same_model(a, b, what):
    for x, y, name in zip(a[:4], b[:4], ("State", "z", "on", "status")):
        assert_bitwise(np.where(a[2][..., None] != 0, x, 0.0) if name == "z" else x,
                       np.where(b[2][..., None] != 0, y, 0.0) if name == "z" else y, f"{what}: {name}")     # (the z of an off particle is dead storage)
    assert a[4] == b[4], (what, a[4], b[4])


# ---- 1. birth identity ----
@pytest.mark.parametrize("solver", ["DP5", "Tsit5", "AutoTsit5(Rosenbrock23())"])
def test_forced_rim_particle_is_the_interior_particle_of_the_same_value(solver):
    cfg = _box(K_SHAPE, solver)
    nx, ny = K_SHAPE
    rim = rim_nodes(cfg.model["grid"], "rim")
    v = _values(len(rim), 7)
    A, B = _model(cfg), _model(_box(K_SHAPE, solver))
    assert born_particles(v, A.minimal_state)[0].all()
    A.backend.bforce_init(rim)
    A.backend.bforce_set_levels(0.0, v)
    A.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    zA, onA, _, stA = A.backend.get_particles()
    inner = [(i, j) for j in range(1, ny - 1) for i in range(1, nx - 1)][:len(rim)]
    S = np.zeros((nx, ny, 3))
    for k, (i, j) in enumerate(inner):
        S[i, j] = v[k]
    B.backend.set_state(S)
    B.backend.remesh(cfg.Δt)                 # branch A at those nodes
    B.backend.advance(cfg.Δt, 0)
    zB, onB, _, stB = B.backend.get_particles()
    ri, rj = np.array(rim).T
    ii, ij = np.array(inner).T
    print(f"{solver}: {int(onA[ri, rj].sum())} of {len(rim)} rim particles on; largest |x|, |y| = "
          f"{np.abs(zA[ri, rj, 3]).max():.3f}, {np.abs(zA[ri, rj, 4]).max():.3f} cells")
    assert onA[ri, rj].all() and np.array_equal(onA[ri, rj], onB[ii, ij])
    assert np.array_equal(stA[ri, rj], stB[ii, ij])
    assert_bitwise(zA[ri, rj], zB[ii, ij], "rim particle vs interior particle")
    assert np.abs(zA[ri, rj, 3:]).max() > 1.0          # some of them travel more than a cell


# ---- 2. fused == single steps == plain phases ----
def _three_paths(cfg, nodes, times, values, n_steps=12):
    """final (State, z, on, status, counters) of one run_steps call, of single steps observed after each, and of advance + remesh +
    tick; the timing counts of the first"""
    out = []
    for path in range(3):
        m = _model(cfg)
        b = m.backend
        b.bforce_init(nodes)
        b.bforce_set_levels(times[0], values[0], times[1], values[1])
        if path == 0:
            b.enable_timing(True)
            b.run_steps(cfg.Δt, n_steps)
            timing = b.get_timing()          # (flushes the last step: one stand-alone scatter + remesh)
        elif path == 1:
            for _ in range(n_steps):
                b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
                b.get_state()
        else:
            for _ in range(n_steps):
                b.advance(cfg.Δt, K.STEP_ZERO_FIRST)
                b.remesh(cfg.Δt)
                b.tick(cfg.Δt)
        out.append(_everything(m))
    return out, timing


@pytest.mark.parametrize("shape", [W_SHAPE, K_SHAPE], ids=["W128x12", "K70x9"])
def test_fused_run_equals_single_steps_and_plain_phases(shape):
    cfg = _box(shape)
    west = rim_nodes(cfg.model["grid"], "west")
    times = (0.0, 12 * cfg.Δt)
    values = (_values(len(west), 1, th=INTO_THE_BOX), _values(len(west), 2, th=INTO_THE_BOX))
    (fused, single, phases), timing = _three_paths(cfg, west, times, values)
    print(shape, timing, fused[4])
    assert timing["advance_launches"] == 12 and timing["scatter_launches"] <= 1, timing
    _assert_same_model(fused, single, "run_steps vs observed single steps")
    _assert_same_model(fused, phases, "run_steps vs advance + remesh + tick")
    assert fused[2][0, :].all() and fused[0][1, 1:-1, 0].min() > 0.0       # the west column bears particles, and they arrive


def test_fused_run_equals_plain_phases_on_the_sphere():
    """the per-node-metric flavour, under the reference's default solver: the south rim of the lon/lat mesh"""
    cfg = configs.sphere_aqua(nx=46, ny=31)
    south = rim_nodes(cfg.model["grid"], "south")
    assert (np.asarray(cfg.model["grid"].data.mask)[:, 0] == 3).all()
    th = np.linspace(0.2, math.pi - 0.2, len(south))          # heading north, fanned out
    def level(e):
        mm = e / (2.0 * 6.0)
        return np.stack([np.full(len(south), e), mm * np.cos(th), mm * np.sin(th)], axis=1)
    (fused, single, phases), timing = _three_paths(cfg, south, (0.0, 12 * cfg.Δt), (level(0.4), level(1.1)))
    print(timing, fused[4])
    assert timing["advance_launches"] == 12 and timing["scatter_launches"] <= 1, timing
    _assert_same_model(fused, single, "sphere: run_steps vs observed single steps")
    _assert_same_model(fused, phases, "sphere: run_steps vs advance + remesh + tick")
    assert fused[2][:, 0].all()


# ---- 3. time interpolation ----
def test_level_pair_is_followed_linearly_in_time():
    cfg = _box(K_SHAPE)
    rim = rim_nodes(cfg.model["grid"], "rim")
    v0, v1 = _values(len(rim), 3, th=DOWNWIND), _values(len(rim), 4, th=DOWNWIND)
    t0, t1 = -1000.0, 5000.0                  # the first step starts at 0, strictly inside
    A, B = _model(cfg), _model(_box(K_SHAPE))
    A.backend.bforce_init(rim)
    A.backend.bforce_set_levels(t0, v0, t1, v1)
    B.backend.bforce_init(rim)
    B.backend.bforce_set_levels(0.0, lerp(0.0, t0, v0, t1, v1))
    for m in (A, B):
        m.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    _assert_same_model(_everything(A), _everything(B), "level pair vs the NumPy lerp as a constant")
    assert A.backend.bforce_info() == (len(rim), 2, t0, t1) and B.backend.bforce_info()[:2] == (len(rim), 1)


# ---- 4. conservation ----
def test_what_enters_is_conserved_and_spreads_no_faster_than_its_reach():
    cfg = _box(K_SHAPE, calm=True)
    nx, ny = K_SHAPE
    west = [(0, j) for j in range(1, ny - 1)]
    e, cb = 1.0, 2.0                          # 1200 m per step on a 2000 m mesh, straight into the box
    v = np.tile([e, e / (2.0 * cb), 0.0], (len(west), 1))
    ref = _model(cfg)
    ref.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert not ref.backend.get_state().any()          # without a forcing the calm box stays empty
    m = _model(_box(K_SHAPE, calm=True))
    b = m.backend
    b.bforce_init(west)
    b.bforce_set_levels(0.0, v)
    b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    S = b.get_state()
    z, on, _, _ = b.get_particles()
    assert on[0, 1:ny - 1].all() and not on[0, 0] and not on[0, ny - 1]
    born = math.fsum(np.exp(z[0, 1:ny - 1, 0]).tolist())
    got = math.fsum(S[..., 0].ravel().tolist())
    print(f"sum State[e] = {got!r}, sum exp(lne) = {born!r}, relative difference {abs(got - born) / born:.3e}; x = {z[0, 1, 3]!r}")
    assert abs(got - born) <= 1e-12 * born          # the four corner weights of a particle sum to one
    assert np.isfinite(S).all() and S[..., 0].min() >= 0.0
    n = 3
    for _ in range(n - 1):
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    S = b.get_state()
    reach = b.get_counters()["max_reach_seen"]
    print(f"after {n} steps: max_reach_seen = {reach}, last non-zero column = {int(np.flatnonzero(S[..., 0].any(axis=1)).max())}")
    assert reach >= 1 and S[..., 0].any()
    assert not S[n * (reach + 1) + 1:].any()
    # the set goes, and its records with it: nothing enters any more (a record left behind would be scattered again every step)
    b.bforce_free()
    prev = math.fsum(S[..., 0].ravel().tolist())
    for _ in range(2):
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        cur = math.fsum(b.get_state()[..., 0].ravel().tolist())
        print(f"after the set was freed: sum State[e] {prev!r} -> {cur!r}")
        assert 0.0 < cur <= prev * (1.0 + 1e-12)
        prev = cur


# ---- 5. hostile values ----
def test_hostile_values_bear_no_particle_and_leave_an_empty_record():
    """Two steps with good values everywhere first: the record buffers are a rotating pair, and after two steps both hold a record
    of every rim node.  Then the hostile values are set.  From there on State must be, bit for bit, that of a twin whose set no longer
    holds the refused nodes (its old set freed — which empties their records — and a new one made without them): a refused lane that
    did not write its empty record would leave the record of two steps ago in the buffer, and it would be scattered again."""
    cfg = _box(W_SHAPE)                      # 276 rim nodes: two workgroups of k_bforce, behind k_step_waverow
    rim = rim_nodes(cfg.model["grid"], "rim")
    good = _values(len(rim), 5, th=DOWNWIND)
    lne_max = cfg.model["ODEsets"].log_energy_maximum
    nan, inf = float("nan"), float("inf")
    hostile = [(nan, 0.1, 0.1), (1.0, nan, 0.1), (1.0, 0.1, nan), (inf, 0.1, 0.1), (1.0, -inf, 0.1), (1.0, 0.1, inf), (-inf, 0.1, 0.1),
               (0.0, 0.1, 0.1), (0.0, 0.0, 0.0), (-1.0, 0.1, 0.1), (1.0, 0.0, 0.0), (1e-9, 0.1, 0.1), (1.0, 1e-6, 0.0)]
    refused = [int(k) for k in np.linspace(2, len(rim) - 2, len(hostile))]          # spread over both workgroups and all four sides
    v = good.copy()
    for k, h in zip(refused, hostile):
        v[k] = h
    big = 100                                                   # far more energy than the cap allows: born, then clamped by the guard
    v[big] = (10.0 * math.exp(lne_max), 10.0 * math.exp(lne_max) / (2.0 * 8.0), 0.0)
    assert not born_particles(v[refused], _model(cfg).minimal_state)[0].any()
    keep = [k for k in range(len(rim)) if k not in refused]
    assert len(set(refused)) == len(hostile) and big not in refused and max(refused) >= 256
    ri, rj = np.array(rim).T
    A, B = _model(cfg), _model(_box(W_SHAPE))
    for m in (A, B):
        m.backend.bforce_init(rim)
        m.backend.bforce_set_levels(0.0, good)
        for _ in range(2):
            m.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert_bitwise(A.backend.get_state(), B.backend.get_state(), "two steps with good values")
    assert A.backend.get_particles()[1][ri, rj].all() and A.backend.get_counters()["clamps"] == 0
    A.backend.bforce_set_levels(0.0, v)                          # the refused nodes stay in A's list ...
    B.backend.bforce_free()                                      # ... and leave B's, records and all
    B.backend.bforce_init([rim[k] for k in keep])
    B.backend.bforce_set_levels(0.0, v[keep])
    for step in range(3):
        for m in (A, B):
            m.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        SA, SB = A.backend.get_state(), B.backend.get_state()
        assert np.isfinite(SA).all(), f"step {step + 1}"
        assert_bitwise(SA, SB, f"step {step + 1} after the hostile values were set: a refused lane left something in its record")
    z, on, _, st = A.backend.get_particles()
    zB, onB, _, stB = B.backend.get_particles()
    assert not on[ri[refused], rj[refused]].any() and on[ri[keep], rj[keep]].all()
    assert not st[ri[refused], rj[refused]].any()
    assert np.array_equal(on, onB) and np.array_equal(st, stB)
    cA, cB = A.backend.get_counters(), B.backend.get_counters()
    print(cA, f"status of the over-energetic particle: {int(st[ri[big], rj[big]])}, lne {z[ri[big], rj[big], 0]!r} (cap {lne_max!r})")
    # a refused lane counts nothing (wave_attempt_slots is a per-wave figure: B's shorter list groups the lanes differently)
    assert {k: x for k, x in cA.items() if k != "wave_attempt_slots"} == {k: x for k, x in cB.items() if k != "wave_attempt_slots"}
    # the over-energetic particle is born and advanced like any other.  Under this wind the dissipation takes ten times the cap below
    # the cap within the step (measured: lne 3.182 against the cap's 3.296, status ST_STEPPED alone), so the energy guard finds
    # nothing to clamp here; the test below has the case where it must
    assert st[ri[big], rj[big]] & K.ST_STEPPED and z[ri[big], rj[big], 0] <= lne_max and np.isfinite(z[ri[big], rj[big]]).all()
    assert cA["dropped_nonfinite"] == 0


def test_over_energetic_value_is_clamped_and_counted():
    """The energy guard on forced particles, where it must act: in the calm box with every source term off a particle's lne does not
    change over a step (the conservation test above rests on the same fact), so a particle born with ten times exp(log_energy_maximum)
    arrives above the cap, and advance_guards sets it to the cap, flags ST_CLAMPED and counts one clamp per particle — as for any
    particle (tests/test_host_api.py, test_energy_clamp_guard).  Its neighbours with ordinary values are left alone."""
    cfg = _box(K_SHAPE, calm=True)
    nx, ny = K_SHAPE
    lne_max = cfg.model["ODEsets"].log_energy_maximum
    west = [(0, j) for j in range(1, ny - 1)]
    over = [1, 4]                                               # list positions of the over-energetic nodes
    e = np.ones(len(west))
    e[over] = 10.0 * math.exp(lne_max)
    v = np.stack([e, e / (2.0 * 2.0), np.zeros(len(west))], axis=1)          # c̄ = 2 m/s straight into the box: 0.6 cells per step
    m = _model(cfg)
    b = m.backend
    b.bforce_init(west)
    b.bforce_set_levels(0.0, v)
    b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    S = b.get_state()
    z, on, _, st = b.get_particles()
    c = b.get_counters()
    col = np.array([j for _, j in west])
    print(c, f"status {st[0, col].tolist()}, lne {z[0, col, 0].tolist()} (cap {lne_max!r})")
    assert on[0, col].all() and (st[0, col] & K.ST_STEPPED).all()
    clamped = (st[0, col] & K.ST_CLAMPED) != 0
    assert np.flatnonzero(clamped).tolist() == over
    assert (z[0, col[over], 0] == lne_max).all() and (z[0, col[~clamped], 0] == 0.0).all()
    assert c["clamps"] == len(over) and c["reseeds"] == 0 and c["dropped_nonfinite"] == 0
    assert np.isfinite(S).all()
    born = math.fsum(np.exp(z[0, col, 0]).tolist())             # what is scattered is the clamped particle
    got = math.fsum(S[..., 0].ravel().tolist())
    assert abs(got - born) <= 1e-12 * born


# ---- 6. probes and statistics ----
def test_station_and_statistics_writers_see_the_forced_particles(tmp_path):
    cfg = _box(K_SHAPE)
    nx, ny = K_SHAPE
    west = rim_nodes(cfg.model["grid"], "west")
    times = np.array([0.0, 1800.0, 3600.0])
    values = np.stack([_values(len(west), 10 + k, c=(1.0, 6.0), th=INTO_THE_BOX) for k in range(3)])      # some stay within the first cell
    n_steps = 6
    watch = [(0, 3), (1, 3), (2, 3), (1, 1), (1, ny - 2), (0, 0), (5, 4)]          # on, beside and away from forced nodes
    m = make_model(cfg, "hip")
    sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1))
    f = sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", times=times, values=values, Δt=cfg.Δt)
    sim.output_writers["stations"] = StationWriter(m, nodes=watch, schedule=1, path=tmp_path, format="npy")
    sw = sim.output_writers["statistics"] = StatisticsWriter(m, fields=("peak", "mean"), schedule=1, path=tmp_path, format="npy")
    m.backend.enable_timing(True)
    run(sim)
    timing = m.backend.get_timing()
    assert timing["advance_launches"] == n_steps and timing["scatter_launches"] <= 1, timing          # the run stayed fused
    assert f.uploads == 2
    # the same run by hand, observed after every step
    ref = _model(_box(K_SHAPE))
    b = ref.backend
    b.bforce_init(west)
    states = [b.get_state()]
    for s in range(n_steps):
        k = min(int(s * cfg.Δt // 1800.0), 1)
        b.bforce_set_levels(times[k], values[k], times[k + 1], values[k + 1])
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        states.append(b.get_state())
    out = read_station_output(tmp_path)
    seen_wet = set()
    assert out["iteration"].tolist() == list(range(n_steps + 1))
    for it in range(n_steps + 1):
        for s, (i, j) in enumerate(watch):
            e, mx, my = states[it][i, j]
            if e > 0.0 and mx * mx + my * my > 0.0:
                assert_bitwise(out["data"][it, s, :3], states[it][i, j], f"station {s} at iteration {it}")
                seen_wet.add(s)
            else:          # a dry node's record is NaN (picles_amd/station_output.py)
                assert np.isnan(out["data"][it, s]).all(), f"station {s} at iteration {it}"
    assert seen_wet >= {0, 1, 2, 3, 4, 6}                       # the forced node itself among them
    assert np.all(out["data"][1:, 1, 0] > 0.0)                  # the node beside the forced column receives
    planes, _, _, _, n_samples = sw.records[0]
    assert n_samples == n_steps
    # the accumulators of picles_amd/run_statistics.py restated over the observed states, wet mask and all, on every node of the
    # grid — the forced column and the rest of the rim included (k_stat pulls a rim node's State like any other node's)
    E = np.stack([S[..., 0] for S in states[1:]])               # [sample, i, j]
    wet = np.isfinite(E) & (E > 0.0) & (np.stack([S[..., 1] * S[..., 1] + S[..., 2] * S[..., 2] for S in states[1:]]) > 0.0)
    assert wet[:, 1:-1, 1:-1].all()
    assert wet[:, 0, 1:-1].any(axis=0).all(), "every forced node of the west column is wet in some sample"
    n_wet, e_peak, sum_e = np.zeros((nx, ny)), np.zeros((nx, ny)), np.zeros((nx, ny))
    for k in range(n_steps):
        e_peak = np.where(wet[k] & ((n_wet == 0.0) | (E[k] > e_peak)), E[k], e_peak)
        sum_e = np.where(wet[k], sum_e + E[k], sum_e)
        n_wet = n_wet + wet[k]
    with np.errstate(all="ignore"):
        hs_max = np.where(n_wet > 0.0, 4.0 * np.sqrt(e_peak), np.nan)
        e_mean = np.where(n_wet > 0.0, sum_e / n_wet, np.nan)
    names = list(sw.names)
    print(f"wet samples of the west column: {n_wet[0].tolist()}; never-wet nodes: {int((n_wet == 0.0).sum())}")
    assert_bitwise(planes[names.index("hs_max")].T, hs_max, "hs_max")
    assert_bitwise(planes[names.index("e_mean")].T, e_mean, "e_mean")
    assert_bitwise(planes[names.index("wet_fraction")].T, n_wet / float(n_steps), "wet_fraction")


# ---- 7. restart ----
def test_pickup_continues_a_forced_run_bit_for_bit(tmp_path):
    times = np.arange(0.0, 5401.0, 1800.0)

    def sim_of(n_steps, ckpt):
        cfg = _box(K_SHAPE)
        m = make_model(cfg, "hip")
        west = rim_nodes(m.grid, "west")
        values = np.stack([_values(len(west), 20 + k, th=INTO_THE_BOX) for k in range(len(times))])
        sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1))
        sim.output_writers["boundary_forcing"] = BoundaryForcing(m, side="west", times=times, values=values)
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
    assert c.clock.iteration == 6 and sim_c.output_writers["boundary_forcing"].uploads >= 1
    _assert_same_model(_everything(a), _everything(c), "six steps straight vs three + checkpoint + pickup + three")


# ---- 8. refusals ----
def test_refusals_leave_a_usable_context():
    cfg = _box(K_SHAPE)
    nx, ny = K_SHAPE
    m = _model(cfg)
    b = m.backend
    for nodes, text in (([(0, 1), (5, 4)], "no grid-boundary node"), ([(0, 1), (3, 0), (0, 1)], "given twice"), ([(nx, 0)], "outside")):
        with pytest.raises(K.PiclesError, match=text):
            b.bforce_init(nodes)
        with pytest.raises(K.PiclesError, match="bforce_init first"):
            b.bforce_info()
    per = _model(configs.bench06_box(n=16))
    with pytest.raises(K.PiclesError, match="periodic_boundary"):
        per.backend.bforce_init([(0, 1)])
    per.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert np.isfinite(per.backend.get_state()).all()
    from test_gpu_probe import _tripolar
    tcfg = _tripolar()
    tri = _model(tcfg)
    with pytest.raises(K.PiclesError, match="tripolar"):
        tri.backend.bforce_init([(0, 0)])
    tri.backend.time_step(tcfg.Δt, K.STEP_ZERO_FIRST)
    assert np.isfinite(tri.backend.get_state()).all()
    # slabs, either way round
    fresh = make_model(_box(K_SHAPE), "hip")
    fresh.backend.bforce_init([(0, 1)])
    with pytest.raises(K.PiclesError, match="boundary forcing set"):
        fresh.backend.set_slab_mode(True)
    with pytest.raises(K.PiclesError, match="boundary forcing set"):
        fresh.backend.begin_step(cfg.Δt, 0)
    # ... a launch of less than all rows launches nothing, and the step that was opened is completed by one of all rows: the
    # context then stands where a twin stands after a plain time_step
    initialize_simulation(Simulation(fresh, Δt=cfg.Δt, stop_time=1.0))
    twin = _model(_box(K_SHAPE))
    v1 = _values(1, 32, th=INTO_THE_BOX)
    twin.backend.bforce_init([(0, 1)])
    for m_ in (fresh, twin):
        m_.backend.bforce_set_levels(0.0, v1)
        m_.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert fresh.backend.begin_fused_step(cfg.Δt)
    with pytest.raises(K.PiclesError, match="boundary forcing set"):
        fresh.backend.step_rows(K.ROWS_EDGE)
    fresh.backend.step_rows(K.ROWS_ALL)
    fresh.backend.end_fused_step()
    twin.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    _assert_same_model(_everything(fresh)[:4] + ({},), _everything(twin)[:4] + ({},), "after the refused launch of the edge rows")
    slab = make_model(_box(K_SHAPE), "hip")
    slab.backend.set_slab_mode(True)
    with pytest.raises(K.PiclesError, match="slabs"):
        slab.backend.bforce_init([(0, 1)])
    slab.backend.set_slab_mode(False)        # the refusal left the context as it was: out of slab mode it steps like any other
    initialize_simulation(Simulation(slab, Δt=cfg.Δt, stop_time=1.0))
    slab.backend.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert np.isfinite(slab.backend.get_state()).all() and slab.backend.get_state()[..., 0].max() > 0.0
    # a step without levels, and a run that would leave the window: nothing is enqueued, the clock stands
    west = rim_nodes(m.grid, "west")
    v0, v1 = _values(len(west), 30, th=INTO_THE_BOX), _values(len(west), 31, th=INTO_THE_BOX)
    b.bforce_init(west)
    with pytest.raises(K.PiclesError, match="picles_bforce_set_levels first"):
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    with pytest.raises(K.PiclesError, match="t1 > t0"):
        b.bforce_set_levels(100.0, v0, 100.0, v1)
    b.bforce_set_levels(0.0, v0, 1800.0, v1)
    b.enable_timing(True)
    with pytest.raises(K.PiclesError, match="call picles_bforce_set_levels with the pair that brackets that time first"):
        b.run_steps(cfg.Δt, 5)               # the fifth step would start at 2400 s
    assert b.clock == 0.0 and b.get_timing()["advance_launches"] == 0
    b.run_steps(cfg.Δt, 4)                   # 0, 600, 1200, 1800: inside
    assert b.clock == 4 * cfg.Δt
    with pytest.raises(K.PiclesError, match="outside the window"):
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    b.bforce_set_levels(1800.0, v1, 3600.0, v0)
    b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    S = b.get_state()
    assert np.isfinite(S).all() and S[1, 1:-1, 0].min() > 0.0
    # and the set can go
    b.bforce_free()
    b.bforce_free()                          # (nothing to free: no error)
    b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    assert np.isfinite(b.get_state()).all()
