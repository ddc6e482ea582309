"""Run statistics (picles_stat_*, include/picles_hip.h "run statistics"): per-node peak / mean / exceedance accumulators kept on the
device, updated behind every step without completing the pending fused step.

Everything is bitwise (tobytes) against tests/_stats_numpy.py applied to the samples of a TWIN context built from the same config,
stepped one step at a time and read with get_state() after each step (existing behaviour).

Grids — the smallest on which the kernel can go wrong: 24x20 periodic x / open y with the land block and the calm band of the
step2d fixtures (rows shorter than a wave), 70x9 (a row crosses a wave boundary, the last workgroup is ragged), 300x5 (a row
crosses a 256-lane workgroup), 3x3 doubly periodic (the pull aliases), one small tripolar-north mesh."""
import numpy as np
import pytest

from picles_amd import configs, _capi as K
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.timesteppers import time_step
from helpers import assert_bitwise, make_model
import _stats_numpy as SN

pytestmark = pytest.mark.gpu

N_STEPS = 12
ALL = K.STAT_ALL


def _ready(cfg):
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    return m


def _box(nx, ny, per=(True, True)):
    c = configs.bench06_box(n=8, dx=2000.0, winds=configs.smooth_winds(10.0, 8.0, 2000.0 * nx, 2000.0 * ny))
    c.model["grid"] = TwoDCartesianGridMesh(0.0, 2000.0 * (nx - 1), nx, 0.0, 2000.0 * (ny - 1), ny, periodic_boundary=per)
    return c


def _make(grid, solver):
    if grid == "24x20":
        from test_step2d_fixture import _cfg
        return _cfg("full_stiff", solver)
    if grid == "3x3":
        from test_gpu_probe import _box_far
        c = _box_far(3, 3)
    elif grid == "tripolar":
        from test_gpu_probe import _tripolar
        c = _tripolar()
    else:
        nx, ny = (int(x) for x in grid.split("x"))
        c = _box(nx, ny)
    c.model["ODEsets"].solver = solver
    return c


_twins = {}


def _twin(grid, solver):
    """(State, clock) after each of N_STEPS steps, observed after every step (the unfused path); computed once, never changed"""
    key = (grid, solver)
    if key not in _twins:
        cfg = _make(grid, solver)
        a = _ready(cfg)
        out = []
        for _ in range(N_STEPS):
            time_step(a, cfg.Δt, zero_first=True)
            S = a.backend.get_state()
            S.setflags(write=False)
            out.append((S, a.backend.clock))
        _twins[key] = out
    return _twins[key]


def _thresholds(twin):
    """four ascending Hs thresholds inside the range the twin's last State spans: every n_exc plane is neither empty nor full"""
    e = twin[-1][0][..., 0]
    hs = 4.0 * np.sqrt(e[e > 0])
    return tuple(float(x) for x in np.quantile(hs, [0.2, 0.4, 0.6, 0.8]))


def _due(every, first, n=N_STEPS, s0=0):
    return [s for s in range(s0 + 1, s0 + n + 1) if s >= first and (s - first) % every == 0]


def _snapshot(b):
    return b.get_state(), b.get_particles(), b.get_counters(), b.clock


def _assert_same_model(a, b, what):
    (Sa, Pa, Ca, ta), (Sb, Pb, Cb, tb) = a, b
    assert_bitwise(Sa, Sb, f"{what}: State")
    on = Pa[1].astype(bool)
    for x, y, name in zip(Pa, Pb, ("z", "on", "boundary", "status")):
        if name == "z":        # (the state vector of a switched-off particle is dead storage)
            assert_bitwise(x[on], y[on], f"{what}: {name}")
        else:
            assert_bitwise(x, y, f"{what}: {name}")
    assert Ca == Cb and ta == tb, (what, Ca, Cb, ta, tb)


GRIDS = ["24x20", "70x9", "300x5", "3x3", "tripolar"]
SOLVERS = ["DP5", "AutoTsit5"]        # AutoTsit5(Rosenbrock23()) is the default solver of ODESettings


# ---- 1. the fused path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("grid", GRIDS)
def test_fused_run_accumulates_what_the_twin_shows(grid, solver):
    twin = _twin(grid, solver)
    thr = _thresholds(twin)
    wet_share = float(SN.wet(twin[-1][0]).mean())
    print(f"{grid} {solver}: wet share of the last State {wet_share:.3f}, thresholds {thr}")
    assert wet_share >= 0.3
    # the run without a set, through the same chunks
    cfg = _make(grid, solver)
    plain = _ready(cfg)
    plain.upload_winds(0.0, cfg.Δt)
    for c in (1, 4, 7):
        plain.backend.run_steps(cfg.Δt, c)
    plain_end = _snapshot(plain.backend)
    for every, first in ((1, 1), (3, 2)):
        cfg = _make(grid, solver)
        m = _ready(cfg)
        b = m.backend
        b.stat_init(ALL, thr, every=every, first=first)
        assert b.stat_shape() == (ALL, thr, every, 13, b.N * 84)
        b.enable_timing(True)
        m.upload_winds(0.0, cfg.Δt)
        for c in (1, 4, 7):
            b.run_steps(cfg.Δt, c)
        got = b.stat_get()              # the last step is still pending here
        t = b.get_timing()              # (flushes the last step: at most one stand-alone scatter + remesh)
        assert t["advance_launches"] == N_STEPS and t["scatter_launches"] <= 1, t
        want = SN.accumulate([twin[s - 1] for s in _due(every, first)], ALL, thr)
        SN.assert_equal(got, want, ALL, f"{grid} {solver} every {every} first {first}")
        assert got["n_samples"] == len(_due(every, first))
        if every == 1:
            assert 0 < got["n_exc"][..., 0].sum() and got["n_exc"][..., 3].sum() < got["n_wet"].sum()
        _assert_same_model(_snapshot(b), plain_end, f"{grid} {solver} every {every}: the model with a set vs without")
    if grid == "3x3":
        c = b.get_counters()
        assert 2 * c["max_reach_seen"] + 1 > 3, c


# ---- 2. the State path ------------------------------------------------------------------------------------------------------------
def test_state_path_seeded_plain_movie_atomic_and_hostile_planes():
    import _hostile_states as H
    cfg = _make("24x20", "DP5")
    m = _ready(cfg)
    b = m.backend
    S0 = b.get_state()
    thr = (0.05, 0.5, 1.0, 3.0)
    b.stat_init(("peak", "mean", "exceed"), thr)
    b.stat_update()                                                   # freshly seeded
    samples = [(S0, 0.0)]
    SN.assert_equal(b.stat_get(), SN.accumulate(samples, ALL, thr), ALL, "seeded state")
    m.upload_winds(0.0, cfg.Δt)
    for k in range(2):                                                # accumulating steps of the plain phases
        b.time_step(cfg.Δt, 0)
        samples.append((b.get_state(), b.clock))
    SN.assert_equal(b.stat_get(), SN.accumulate(samples, ALL, thr), ALL, "plain-phase steps")
    before = b.stat_get()
    for k in range(2):                                                # MOVIE: State reads zeros — only n_samples moves
        b.zero_state()
        b.time_step(cfg.Δt, K.STEP_MOVIE)
        samples.append((b.get_state(), b.clock))
        assert not samples[-1][0].any()
    after = b.stat_get()
    for name in SN.plane_names(ALL):
        assert after[name].tobytes() == before[name].tobytes(), name
    assert after["n_samples"] == before["n_samples"] + 2 and after["t_last"] == b.clock and after["t_first"] == 0.0
    for k in range(2):                                                # ATOMIC: not reproducible across contexts — own get_state
        b.zero_state()
        b.time_step(cfg.Δt, K.STEP_ATOMIC)
        samples.append((b.get_state(), b.clock))
    SN.assert_equal(b.stat_get(), SN.accumulate(samples, ALL, thr), ALL, "movie and atomic steps")
    assert float(SN.wet(samples[-1][0]).mean()) >= 0.3
    # hostile planes: the device's half of the hostile-value check of tests/test_run_stats_host.py
    b.stat_reset()
    hostile = H_samples(H, 24, 20)
    for S, clock in hostile:
        b.set_state(S)
        b.stat_update()
    got = b.stat_get()
    want = SN.accumulate([(S, b.clock) for S, _ in hostile], ALL, thr)
    SN.assert_equal(got, want, ALL, "hostile planes")
    assert 0 < int((got["n_wet"] > 0).sum()) < got["n_wet"].size and np.isinf(got["sum_e"]).any()


def H_samples(H, Nx, ny):
    """the hostile samples shared with the CPU test: three hostile States, the large sweep, all NaN, the first one again (a
    repeated maximum)"""
    S = [H.hostile_state(Nx, ny, 2, 2, seed) for seed in (11, 12, 13)]
    S += [H.sweep_state(Nx, ny, 14), H.all_nan_state(Nx, ny, 15), S[0]]
    return [(s, 600.0 * (k + 1)) for k, s in enumerate(S)]


# ---- 3. get, reset, set -----------------------------------------------------------------------------------------------------------
def test_get_and_reset_in_the_middle_of_a_fused_run():
    grid, solver = "24x20", "DP5"
    twin = _twin(grid, solver)
    thr = _thresholds(twin)
    cfg = _make(grid, solver)
    m = _ready(cfg)
    b = m.backend
    b.stat_init(ALL, thr)
    b.enable_timing(True)
    m.upload_winds(0.0, cfg.Δt)
    b.run_steps(cfg.Δt, 5)
    mid = b.stat_get()                                                # step 5 stays pending
    SN.assert_equal(mid, SN.accumulate(twin[:5], ALL, thr), ALL, "get after 5 steps")
    only = b.stat_get("peak")
    assert sorted(k for k, v in only.items() if isinstance(v, np.ndarray) and v.ndim >= 2) == sorted(SN.PEAK_PLANES + ("n_wet",))
    assert only["e_peak"].tobytes() == mid["e_peak"].tobytes() and only["n_wet"].tobytes() == mid["n_wet"].tobytes()
    b.stat_reset()
    b.run_steps(cfg.Δt, 7)
    got = b.stat_get()
    t = b.get_timing()
    assert t["advance_launches"] == N_STEPS and t["scatter_launches"] <= 1, t          # neither get nor reset completed a step
    SN.assert_equal(got, SN.accumulate(twin[5:], ALL, thr), ALL, "after a reset: the later samples only")
    assert_bitwise(b.get_state(), twin[-1][0], "final State")


def test_set_continues_a_run_picked_up_from_a_checkpoint():
    grid, solver = "24x20", "DP5"
    twin = _twin(grid, solver)
    thr = _thresholds(twin)
    cfg = _make(grid, solver)
    m = _ready(cfg)
    b = m.backend
    b.stat_init(ALL, thr)
    m.upload_winds(0.0, cfg.Δt)
    b.run_steps(cfg.Δt, 6)
    b.checkpoint_begin()
    blob = b.checkpoint_end()
    acc = b.stat_get()
    SN.assert_equal(b.stat_get(), acc, ALL, "the checkpoint left the set as it was")
    cfg2 = _make(grid, solver)
    m2 = _ready(cfg2)
    b2 = m2.backend
    b2.stat_init(ALL, thr)
    b2.stat_update()                                                  # something to overwrite
    b2.checkpoint_load(blob)
    b2.stat_set(acc)
    SN.assert_equal(b2.stat_get(), acc, ALL, "set then get")
    m2.upload_winds(b2.clock, cfg2.Δt)
    b2.run_steps(cfg2.Δt, 6)
    SN.assert_equal(b2.stat_get(), SN.accumulate(twin, ALL, thr), ALL, "6 + 6 steps across a checkpoint vs 12 uninterrupted")
    assert_bitwise(b2.get_state(), twin[-1][0], "final State")


# ---- 4. slabs in one process (the native ring: tests/test_gpu_run_stats_ring.py) -------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_in_process_slabs_gather_the_whole_grid_planes(world):
    from picles_amd.driver import stat_concat
    from picles_amd.parallel import SlabModel
    from test_gpu_slab_fuzz import _NoExchange, _step_all
    grid, solver = "24x20", "DP5"
    twin = _twin(grid, solver)
    thr = _thresholds(twin)
    n, dt = 8, _make(grid, solver).Δt
    slabs = [SlabModel(_make(grid, solver).model, r, world, device=0, halo_rows=2, exchange=_NoExchange()) for r in range(world)]
    for s in slabs:
        s._comm_warm = True
        s.seed()
        s.stat_init(ALL, thr, every=2, first=1)
    for k in range(n):
        _step_all(slabs, dt, slabs[0].periodic_y, fused_ok=True)
        for s in slabs:
            s._stat_after_steps(1, split_phase=True)                  # what SlabModel.time_step does behind its halo exchange
    got = stat_concat([s.stat_get() for s in slabs])
    assert sum(s.backend.get_counters()["halo_overflow"] for s in slabs) == 0
    want = SN.accumulate([twin[s - 1] for s in _due(2, 1, n)], ALL, thr)
    SN.assert_equal(got, want, ALL, f"{world} slabs")
    assert_bitwise(np.concatenate([s.get_state() for s in slabs], axis=1), twin[n - 1][0], "State")


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    cfg = _make("24x20", "DP5")
    m = _ready(cfg)
    b = m.backend
    lib, h = b.lib, b.h
    import ctypes as C
    buf = np.zeros(b.N * 84, dtype=np.uint8)
    vp = buf.ctypes.data_as(C.c_void_p)
    thr4 = (C.c_double * 4)(0.5, 1.0, 2.0, 3.0)
    n, t0, t1 = C.c_int64(), C.c_double(), C.c_double()

    def refused(rc, text):
        assert rc == -2, (rc, text)
        assert text in lib.picles_last_error(h).decode(), (text, lib.picles_last_error(h))

    # without a set
    refused(lib.picles_stat_update(h, None), "picles_stat_init first")
    refused(lib.picles_stat_get(h, 0, vp, C.byref(n), C.byref(t0), C.byref(t1)), "picles_stat_init first")
    refused(lib.picles_stat_set(h, 0, vp, 0, 0.0, 0.0), "picles_stat_init first")
    refused(lib.picles_stat_reset(h), "picles_stat_init first")
    assert lib.picles_stat_shape(h, None, None, None, None, None, None) == -1
    assert lib.picles_stat_free(h) == 0
    # init
    bad = lambda *v: (C.c_double * 4)(*v)      # noqa: E731
    for args, text in (((0, 0, None, 1, 1), "empty or unknown group mask"), ((8, 0, None, 1, 1), "empty or unknown group mask"),
                       ((-1, 0, None, 1, 1), "empty or unknown group mask"),
                       ((7, 0, None, 1, 1), "takes 1 ... 4 thresholds"), ((7, 5, thr4, 1, 1), "takes 1 ... 4 thresholds"),
                       ((4, 2, None, 1, 1), "takes 1 ... 4 thresholds"),
                       ((7, 2, bad(1.0, 1.0), 1, 1), "strictly ascending"), ((7, 2, bad(2.0, 1.0), 1, 1), "strictly ascending"),
                       ((7, 1, bad(0.0), 1, 1), "strictly ascending"), ((7, 1, bad(-1.0), 1, 1), "strictly ascending"),
                       ((7, 2, bad(1.0, np.inf), 1, 1), "strictly ascending"), ((7, 1, bad(np.nan), 1, 1), "strictly ascending"),
                       ((3, 1, thr4, 1, 1), "without PICLES_STAT_EXCEED"),
                       ((7, 4, thr4, 0, 1), "must be >= 1"), ((7, 4, thr4, 1, 0), "must be >= 1")):
        refused(lib.picles_stat_init(h, *args), text)
        assert lib.picles_stat_shape(h, None, None, None, None, None, None) == -1      # the context is unchanged: still no set
    with pytest.raises(ValueError):
        b.stat_init(("peak", "median"))
    b.stat_init(("peak", "exceed"), (0.5, 1.0))
    assert b.stat_shape() == (5, (0.5, 1.0), 1, 7, b.N * (32 + 12))
    refused(lib.picles_stat_init(h, 1, 0, None, 1, 1), "a statistics set exists")
    refused(lib.picles_stat_get(h, 5, None, C.byref(n), C.byref(t0), C.byref(t1)), "planes must be given")
    refused(lib.picles_stat_set(h, 5, None, 0, 0.0, 0.0), "planes must be given")
    refused(lib.picles_stat_get(h, 2, vp, None, None, None), "no subset")
    refused(lib.picles_stat_set(h, 7, vp, 0, 0.0, 0.0), "no subset")
    refused(lib.picles_stat_set(h, 5, vp, -1, 0.0, 0.0), "n_samples must be >= 0")
    # ... and the context goes on as if nothing had been asked
    twin = _twin("24x20", "DP5")
    m.upload_winds(0.0, cfg.Δt)
    b.run_steps(cfg.Δt, 3)
    SN.assert_equal(b.stat_get(), SN.accumulate(twin[:3], 5, (0.5, 1.0)), 5, "after the refusals")
    b.stat_free()
    refused(lib.picles_stat_update(h, None), "picles_stat_init first")
    b.stat_init("mean", every=2, first=1)                             # a new set after free; s counts from here
    b.run_steps(cfg.Δt, 3)
    SN.assert_equal(b.stat_get(), SN.accumulate([twin[3], twin[5]], 2), 2, "a new set after free")
    assert_bitwise(b.get_state(), twin[5][0], "State")


# ---- 6. the writer end to end -------------------------------------------------------------------------------------------------------
def test_statistics_writer_end_to_end(tmp_path):
    from picles_amd.run_statistics import StatisticsWriter, derive, read_statistics
    from picles_amd.simulations import run
    grid, solver = "24x20", "DP5"
    twin = _twin(grid, solver)
    thr = _thresholds(twin)[1:3]
    cfg = _make(grid, solver)
    m = make_model(cfg, "hip")
    sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * 9)
    initialize_simulation(sim)
    w = StatisticsWriter(m, fields=("peak", "mean", "exceed"), thresholds=thr, schedule=1, window=5, path=tmp_path / "stats")
    sim.output_writers["statistics"] = w
    m.backend.enable_timing(True)
    run(sim)
    t = m.backend.get_timing()
    assert t["advance_launches"] == 10 and t["scatter_launches"] <= 1, t
    out = read_statistics(w.path)
    assert out["data"].shape == (len(out["names"]), 20, 24, 2) and list(out["thresholds"]) == list(thr)
    P = m.ODEsettings.Parameters
    for k, part in enumerate((twin[:5], twin[5:10])):
        acc = SN.accumulate(part, ALL, thr)
        want = derive(acc, g=P.get("g", 9.81), r_g=P["r_g"])
        assert out["t_start"][k] == part[0][1] and out["t_end"][k] == part[-1][1]
        for i, name in enumerate(out["names"]):
            a, b_ = np.ascontiguousarray(out["data"][i, :, :, k]), np.ascontiguousarray(want[name].T)
            assert a.tobytes() == b_.tobytes(), (k, name)
        hs_max = out["data"][list(out["names"]).index("hs_max"), :, :, k]
        assert np.isfinite(hs_max).mean() >= 0.3 and np.array_equal(np.isnan(hs_max), (acc["n_wet"] == 0).T)


# ---- 7. all four writers at once: every product equals that of a run with that writer alone ---------------------------------------
def test_four_writers_at_once_write_what_each_writes_alone(tmp_path):
    """tests/test_run_call_sequence.py pins the ORDER of run()'s calls with several writers attached; this shows the library
    agrees that the order gives the same products: bench06_box(n=48) (no multiple of the 64-node tile), 23 steps, the schedules
    of that test; every .npy file and every checkpoint file, byte for byte, against four runs with one writer each"""
    from picles_amd.checkpointing import Checkpointer
    from picles_amd.field_output import FieldWriter
    from picles_amd.run_statistics import StatisticsWriter
    from picles_amd.simulations import run
    from picles_amd.station_output import StationWriter
    make = {"ck": lambda m, d: Checkpointer(m, schedule=7, dir=d / "ck"),
            "fields": lambda m, d: FieldWriter(m, schedule=5, path=d / "fields", slots=2, format="npy"),
            "stations": lambda m, d: StationWriter(m, nodes=[(1, 2), (3, 4)], schedule=1, path=d / "stations", capacity=3, format="npy"),
            "statistics": lambda m, d: StatisticsWriter(m, thresholds=(0.25,), window=10, path=d / "statistics", format="npy")}

    def products(kinds, d):
        cfg = configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * 48, 2000.0 * 48))
        m = make_model(cfg, "hip")
        sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * 22)
        for k in kinds:
            sim.output_writers[k] = make[k](m, d)
        run(sim)
        assert m.clock.iteration == 23
        return {p.relative_to(d).as_posix(): p.read_bytes() for p in sorted(d.rglob("*")) if p.suffix in (".npy", ".picles")}

    together = products(tuple(make), tmp_path / "together")
    assert sorted(together) == ["ck/checkpoint_iteration14.picles", "ck/checkpoint_iteration21.picles", "ck/checkpoint_iteration7.picles",
                                "fields/fields.waves.data.npy", "fields/fields.waves.scalars.npy", "stations/stations.stations.data.npy",
                                "statistics/statistics.stats.data.npy"]
    alone = {}
    for k in make:
        alone.update(products((k,), tmp_path / k))
    assert sorted(alone) == sorted(together)
    for name, data in together.items():
        assert data == alone[name], f"{name}: with all four writers attached it differs from the run with this writer alone"
