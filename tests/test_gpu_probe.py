"""Station probes (picles_probe_*, include/picles_hip.h "station probes"): a sample is, bit for bit, what picles_get_state would
return for the probed nodes at that moment — taken without completing the pending fused step, without a host synchronisation and
without touching anything of the model.

The reference for every value is a TWIN context built from the same config, stepped with picles_time_step and read with
get_state() after every step (existing behaviour, which the existing tests hold bitwise equal to the fused run)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from picles_amd import configs, _capi as K
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.timesteppers import time_step
from helpers import assert_bitwise, make_model

pytestmark = pytest.mark.gpu


def _ready(cfg):
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    return m


def probe_nodes(grid, extra=(), seed=20240607):
    """200 nodes drawn with a fixed seed, the four grid corners, ten land nodes where there is a mask, and `extra`"""
    Nx, Ny = int(grid.stats.Nx), int(grid.stats.Ny)
    rng = np.random.default_rng(seed)
    nodes = [(int(rng.integers(Nx)), int(rng.integers(Ny))) for _ in range(200)]
    nodes += [(0, 0), (Nx - 1, 0), (0, Ny - 1), (Nx - 1, Ny - 1)]
    land = np.argwhere(np.asarray(grid.data.mask) == 0)
    nodes += [(int(i), int(j)) for i, j in land[:10]]
    nodes += list(extra)
    return np.array(nodes, dtype=np.int64)


def _at(S, nodes):
    """[3, n] of a State array [Nx, Ny, 3]"""
    return np.ascontiguousarray(S[nodes[:, 0], nodes[:, 1], :].T)


def _twin_series(cfg, n, flags=K.STEP_ZERO_FIRST):
    """the existing way: step, look, step, look"""
    a = _ready(cfg)
    out = []
    for _ in range(n):
        if flags == K.STEP_ZERO_FIRST:
            time_step(a, cfg.Δt, zero_first=True)
        else:
            a.upload_winds(a.clock.time, cfg.Δt)
            a.backend.time_step(cfg.Δt, flags)
            a.clock.time += cfg.Δt
        out.append((a.backend.get_state(), a.backend.clock))
    return a, out


def _check_series(v, t, s, nodes, twin, steps, wet_min, what):
    assert list(s) == list(steps), (what, list(s))
    for k, step in enumerate(steps):
        S, clock = twin[step - 1]
        assert t[k] == clock, (what, step, t[k], clock)
        assert_bitwise(v[k], _at(S, nodes), f"{what}: sample of step {step}")
    wet = float((v[-1][0] > 0).mean())
    print(f"{what}: share of probed nodes with e > 0 at the last step: {wet:.3f} (bound {wet_min})")
    assert wet >= wet_min, (what, wet)


def _tv(P):
    """winds that change in space and time (period P in space)"""
    u = lambda x, y, t: 9.0 * (1 + 0.2 * np.sin(2 * np.pi * x / P)) * (1 + t / 14400.0) + 0 * y        # noqa: E731
    v = lambda x, y, t: 6.0 * (1 + 0.2 * np.cos(2 * np.pi * y / P)) * (1 - 0.3 * t / 14400.0) + 0 * x  # noqa: E731
    return SimpleNamespace(u=u, v=v)


def _box_tv(n=40):
    c = configs.bench06_box(n=n, winds=_tv(2000.0 * n))
    c.model["winds_static"] = False
    return c


def _box_lattice_smooth3():
    return configs.closure_lattice(_box_tv(40), 8)


def _box_polyline():
    from picles_amd.wind_emulator import GriddedWinds
    c = configs.bench06_box(n=40)
    P = 2000.0 * 39
    x = np.linspace(0.0, P, 9)
    t = np.arange(0.0, 10 * 600.0 + 1.0, 250.0)        # two or three knots inside every 600 s step: polyline windows
    X, Y, T = np.meshgrid(x, x, t, indexing="ij")
    c.model["winds"] = GriddedWinds(x, x, t, 9.0 * (1 + 0.2 * np.sin(2 * np.pi * X / P)) * (1 + T / 7200.0),
                                    6.0 * (1 + 0.2 * np.cos(2 * np.pi * Y / P)) * (1 - 0.3 * T / 7200.0))
    c.model["winds_static"] = False
    return c


def _box_auto():
    c = configs.bench06_box(n=40, U10=10.0, V10=3.0, periodic_grid=False)
    n, dx = 40, 2000.0
    mask = np.ones((n, n), dtype=bool)
    mask[12:20, 22:30] = False
    c.model["grid"] = TwoDCartesianGridMesh(dx * (n - 1), n, dx * (n - 1), n, mask=mask, periodic_boundary=(False, False))
    c.model["periodic_boundary"] = False
    c.model["ODEsets"].solver = "AutoTsit5"
    return c


def _box_far(nx=64, ny=64, per=(True, True)):
    """500 m cells and 30-minute steps: particles travel several cells per step"""
    c = configs.bench06_box(n=8, dx=500.0, U10=9.0, V10=-4.0)
    c.Δt = 1800.0
    c.model["grid"] = TwoDCartesianGridMesh(0.0, 500.0 * (nx - 1), nx, 0.0, 500.0 * (ny - 1), ny, periodic_boundary=per)
    u0 = lambda x, y, t: 9.0 + 5.0 * np.sin(x / 700.0) * np.cos(y / 900.0)      # noqa: E731
    v0 = lambda x, y, t: -4.0 + 6.0 * np.cos(x / 500.0 + y / 1100.0)             # noqa: E731
    c.model["winds"] = SimpleNamespace(u=u0, v=v0)
    c.model["ODEsys"].u, c.model["ODEsys"].v = u0, v0
    return c


def _tripolar(nx=18, ny=14):
    c = configs.bench06_box(n=8, dx=1200.0, U10=6.0, V10=11.0)
    c.Δt = 1200.0
    c.model["grid"] = TwoDCartesianGridMesh(0.0, 1200.0 * (nx - 1), nx, 0.0, 1200.0 * (ny - 1), ny,
                                            periodic_boundary=(True, "tripolar_north"))
    return c


# name: (config, steps, "run" = picles_run_steps in one call | "step" = the model layer's time_step per step, wet bound, reach asserted)
CASES = {
    "bench06_48_fused_static": (lambda: configs.bench06_box(n=48), 6, "run", 0.5, 0),
    "example_00_33_open_edges": (lambda: configs.example_00_minimal(n=33, L=64e3), 5, "run", 0.5, 0),
    "T04_32": (lambda: configs.T04_2D_reg_test(n=32), 6, "run", 0.5, 0),
    "sphere_92x60_metric": (lambda: configs.sphere_aqua(nx=92, ny=60), 4, "run", 0.1, 0),
    "box_40_solver2_masked": (_box_auto, 6, "run", 0.5, 0),
    "box_40_lattice_smooth3": (_box_lattice_smooth3, 6, "run", 0.5, 0),
    "box_40_host_closures_plain_phases": (_box_tv, 5, "step", 0.5, 0),
    "box_40_polyline_window": (_box_polyline, 5, "run", 0.5, 0),
    "box_64_reach_2": (_box_far, 6, "run", 0.5, 2),
    "tripolar_18x14_top_rows": (_tripolar, 8, "run", 0.5, 0),
    "box_100_nx_not_multiple_of_64": (lambda: configs.bench06_box(n=100, dx=1000.0), 4, "run", 0.5, 0),
    "box_7x6_aliased_pull": (lambda: _box_far(7, 6), 6, "run", 0.5, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_samples_equal_get_state_of_the_twin_bitwise(name):
    make, n, mode, wet_min, reach = CASES[name]
    cfg = make()
    g = cfg.model["grid"]
    Nx, Ny = int(g.stats.Nx), int(g.stats.Ny)
    extra = [(i, j) for j in (Ny - 1, Ny - 2) for i in range(Nx)] if "tripolar" in name else []
    nodes = probe_nodes(g, extra)
    _, twin = _twin_series(make(), n)
    m = _ready(cfg)
    b = m.backend
    b.probe_init(nodes, every=1, first=1, capacity=n)
    assert b.probe_shape() == (len(nodes), 1, n) and b.probe_pending == 0
    if mode == "run":
        m.upload_winds(m.clock.time, cfg.Δt)
        b.run_steps(cfg.Δt, n)
    else:
        for _ in range(n):
            time_step(m, cfg.Δt, zero_first=True)
    assert b.probe_pending == n
    v, t, s = b.probe_pop()
    assert v.shape == (n, 3, len(nodes)) and b.probe_pending == 0
    _check_series(v, t, s, nodes, twin, range(1, n + 1), wet_min, name)
    # and the model itself went where the twin went
    assert_bitwise(b.get_state(), twin[-1][0], f"{name}: final State")
    c = b.get_counters()
    if reach:
        assert c["max_reach_seen"] >= reach, c
    if "aliased" in name:
        assert 2 * c["max_reach_seen"] + 1 > min(Nx, Ny), c


@pytest.mark.parametrize("flags", [K.STEP_MOVIE, K.STEP_ATOMIC, 0])
def test_samples_of_movie_atomic_and_accumulating_steps(flags):
    """State is in memory after these: a MOVIE step leaves zeros (as picles_get_state shows); the atomic push is not reproducible
    across contexts, so its samples are held against the same context's own get_state"""
    cfg = configs.bench06_box(n=48)
    nodes = probe_nodes(cfg.model["grid"])
    m = _ready(cfg)
    b = m.backend
    b.probe_init(nodes, capacity=1)
    m.upload_winds(0.0, cfg.Δt)
    for k in range(4):
        if flags != 0:
            b.zero_state()
        b.time_step(cfg.Δt, flags)
        assert b.probe_pending == 1
        own = _at(b.get_state(), nodes)
        v, t, s = b.probe_pop()
        assert list(s) == [k + 1] and t[0] == b.clock
        assert_bitwise(v[0], own, f"flags {flags} step {k + 1}")
        if flags == K.STEP_MOVIE:
            assert not v.any()
        else:
            wet = float((v[0][0] > 0).mean())
            print(f"flags {flags}: wet share {wet:.3f}")
            assert wet >= 0.5
    if flags == 0:       # the accumulating steps are reproducible: the twin agrees too
        _, twin = _twin_series(configs.bench06_box(n=48), 4, flags=0)
        assert_bitwise(own, _at(twin[-1][0], nodes), "accumulating steps vs the twin")


def test_seeded_state_set_state_and_checkpoint_sources():
    """picles_probe_sample: the freshly seeded State, a State written by the caller, and the State of a loaded checkpoint"""
    cfg = configs.bench06_box(n=48)
    nodes = probe_nodes(cfg.model["grid"])
    m = _ready(cfg)
    b = m.backend
    b.probe_init(nodes, capacity=4)
    b.probe_sample()
    S0 = b.get_state()
    b.set_state(2.0 * S0)
    b.probe_sample()
    m.upload_winds(0.0, cfg.Δt)
    b.run_steps(cfg.Δt, 2)
    v, t, s = b.probe_pop()
    assert list(s) == [0, 0, 1, 2] and list(t) == [0.0, 0.0, cfg.Δt, 2 * cfg.Δt]
    assert_bitwise(v[0], _at(S0, nodes), "seeded state")
    assert_bitwise(v[1], _at(2.0 * S0, nodes), "after set_state")
    b.checkpoint_begin()
    blob = b.checkpoint_end()
    S2 = b.get_state()
    b.run_steps(cfg.Δt, 1)
    with pytest.raises(K.CheckpointError) as e:
        b.checkpoint_load(blob)
    assert e.value.code == K.CKPT_E_BUSY and "probe samples" in str(e.value)
    b.probe_pop()
    b.checkpoint_load(blob)
    b.probe_sample()
    v, t, s = b.probe_pop()
    assert_bitwise(v[0], _at(S2, nodes), "after a checkpoint load")
    assert t[0] == 2 * cfg.Δt


def test_probes_have_no_side_effect():
    make = lambda: configs.bench06_box(n=256, winds=configs.smooth_winds(10.0, 8.0, 256 * 2000.0, 256 * 2000.0))      # noqa: E731
    nodes = probe_nodes(make().model["grid"])
    out = []
    for probed in (True, False):
        m = _ready(make())
        b = m.backend
        if probed:
            b.probe_init(nodes, every=1, first=1, capacity=12)
        m.upload_winds(0.0, 600.0)
        b.run_steps(600.0, 12)
        order = (C.c_int32 * 4096)()
        nord = b.lib.picles_get_dispatch_order(b.h, order, 4096)
        out.append((b.get_state(), b.get_particles(), b.get_counters(), (nord, list(order)), b.clock))
    (Sa, Pa, Ca, Oa, ta), (Sb, Pb, Cb, Ob, tb) = out
    assert_bitwise(Sa, Sb, "State")
    for x, y, what in zip(Pa, Pb, ("z", "on", "boundary", "status")):
        on = Pa[1].astype(bool)
        if what == "z":        # (the state vector of a switched-off particle is dead storage)
            assert_bitwise(x[on], y[on], what)
        else:
            assert_bitwise(x, y, what)
    assert Ca == Cb and Oa == Ob and ta == tb


@pytest.mark.parametrize("through", ["time_step", "run_steps"])
def test_fused_path_is_kept_with_probes_on(through):
    """the set-up and the assertion of tests/test_gpu_lazy_state.py::test_unobserved_run_loop_stays_fused_and_off_pcie with a probe
    set sampled every step"""
    cfg = configs.bench06_box(n=256, winds=configs.smooth_winds(10.0, 8.0, 256 * 2000.0, 256 * 2000.0))
    m = _ready(cfg)
    b = m.backend
    b.probe_init(probe_nodes(cfg.model["grid"]), capacity=10)
    b.enable_timing(True)
    if through == "time_step":
        for _ in range(10):
            m.State.fill(0.0)
            time_step(m, cfg.Δt)
    else:
        m.upload_winds(0.0, cfg.Δt)
        b.run_steps(cfg.Δt, 10)
    assert b.probe_pending == 10
    t = b.get_timing()
    assert t["advance_launches"] == 10 and t["scatter_launches"] <= 1, t


def test_ring_pops_in_order_while_steps_are_enqueued():
    """as tests/test_gpu_field_output.py shows it for the diagnostics ring: the oldest samples are handed out — with the right
    values — while later steps are enqueued behind them; pop waits for the copies of the samples it hands out, nothing else"""
    cfg = configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * 48, 2000.0 * 48))
    nodes = probe_nodes(cfg.model["grid"])
    _, twin = _twin_series(configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * 48, 2000.0 * 48)), 12)
    m = _ready(cfg)
    b = m.backend
    b.probe_init(nodes, capacity=8)
    m.upload_winds(0.0, cfg.Δt)
    b.run_steps(cfg.Δt, 8)                        # eight steps and their samples enqueued; nothing waited for
    got = [b.probe_pop(2)]                        # the first two, while the rest is in flight
    b.run_steps(cfg.Δt, 2)                        # more steps behind the samples still pending
    got.append(b.probe_pop(3))
    b.run_steps(cfg.Δt, 2)
    assert b.probe_pending == 7
    got.append(b.probe_pop())
    v = np.concatenate([g[0] for g in got]); t = np.concatenate([g[1] for g in got]); s = np.concatenate([g[2] for g in got])
    _check_series(v, t, s, nodes, twin, range(1, 13), 0.5, "pops between enqueued steps")
    assert [len(g[2]) for g in got] == [2, 3, 7]


@pytest.mark.parametrize("every,first", [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_cadence(every, first):
    cfg = configs.bench06_box(n=48)
    nodes = probe_nodes(cfg.model["grid"])
    n = 11
    _, twin = _twin_series(configs.bench06_box(n=48), n)
    want = [s for s in range(1, n + 1) if s >= first and (s - first) % every == 0]
    for split in (None, 4):
        m = _ready(cfg)
        b = m.backend
        b.probe_init(nodes, every=every, first=first, capacity=len(want))
        m.upload_winds(0.0, cfg.Δt)
        if split is None:
            b.run_steps(cfg.Δt, n)
        else:
            b.run_steps(cfg.Δt, split)
            for _ in range(n - split):
                b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        v, t, s = b.probe_pop()
        _check_series(v, t, s, nodes, twin, want, 0.5, f"every {every} first {first} split {split}")


def test_full_ring_refuses_and_nothing_is_lost():
    cfg = configs.bench06_box(n=48)
    nodes = probe_nodes(cfg.model["grid"])
    _, twin = _twin_series(configs.bench06_box(n=48), 9)
    m = _ready(cfg)
    b = m.backend
    b.probe_init(nodes, every=1, first=1, capacity=3)
    m.upload_winds(0.0, cfg.Δt)
    with pytest.raises(K.PiclesError, match="probe ring full") as e:
        b.run_steps(cfg.Δt, 4)                    # would overrun: refused up front, not after three steps
    assert e.value.code == K.PROBE_E_FULL and b.clock == 0.0 and b.probe_pending == 0
    b.run_steps(cfg.Δt, 3)
    clock = b.clock
    for call in (lambda: b.time_step(cfg.Δt, K.STEP_ZERO_FIRST), lambda: b.run_steps(cfg.Δt, 1), lambda: b.probe_sample()):
        with pytest.raises(K.PiclesError, match="probe ring full") as e:
            call()
        assert e.value.code == K.PROBE_E_FULL and b.clock == clock and b.probe_pending == 3
    got = [b.probe_pop(1)]                        # one slot free: the same call succeeds
    b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
    got.append(b.probe_pop())                     # samples 2, 3, 4: across the ring's wrap, oldest first
    b.run_steps(cfg.Δt, 3)
    got.append(b.probe_pop(2))
    b.run_steps(cfg.Δt, 2)
    got.append(b.probe_pop())
    v = np.concatenate([g[0] for g in got]); t = np.concatenate([g[1] for g in got]); s = np.concatenate([g[2] for g in got])
    _check_series(v, t, s, nodes, twin, range(1, 10), 0.5, "ring of three over nine steps")
    assert_bitwise(b.get_state(), twin[-1][0], "final State equals the unprobed twin's")


def test_refusals():
    cfg = configs.bench06_box(n=48)
    m = _ready(cfg)
    b = m.backend
    ok = np.array([[1, 2], [3, 4]])
    for call, text in ((lambda: b.probe_pop(), "probe_init first"), (lambda: b.probe_sample(), "picles_probe_init first")):
        with pytest.raises(K.PiclesError, match=text):
            call()
    assert b.probe_pending == 0
    for kw, text in ((dict(nodes=np.zeros((0, 2), dtype=int)), "n must be >= 1"),
                     (dict(nodes=np.array([[48, 0]])), r"node 0 = \(48, 0\) lies outside"),
                     (dict(nodes=np.array([[0, 0], [0, 48]])), r"node 1 = \(0, 48\) lies outside"),
                     (dict(nodes=np.array([[-1, 0]])), "lies outside"),
                     (dict(nodes=ok, every=0), "must be >= 1"), (dict(nodes=ok, first=0), "must be >= 1"),
                     (dict(nodes=ok, capacity=0), "must be >= 1")):
        with pytest.raises(K.PiclesError, match=text):
            b.probe_init(**kw)
        with pytest.raises(K.PiclesError):
            b.probe_shape()                       # the context is unchanged: still no set
    b.probe_init(ok)
    with pytest.raises(K.PiclesError, match="a probe set exists"):
        b.probe_init(ok)
    with pytest.raises(K.PiclesError, match="no probe sample pending") as e:
        b.probe_pop()
    assert e.value.code == -3
    b.probe_sample()
    b.probe_free()                                # with a sample pending
    with pytest.raises(K.PiclesError, match="picles_probe_init first"):
        b.probe_sample()
    b.probe_init(np.array([[5, 5], [5, 5]]), every=2, first=3, capacity=2)      # duplicates are allowed; a new set after free
    assert b.probe_shape() == (2, 2, 2)
    m.upload_winds(0.0, cfg.Δt)
    b.run_steps(cfg.Δt, 5)
    v, t, s = b.probe_pop()
    assert list(s) == [3, 5] and np.array_equal(v[:, :, 0], v[:, :, 1])
    # a slab context refuses nodes outside its own rows
    from picles_amd.parallel import SlabModel
    sl = SlabModel(cfg.model, rank=1, world=2, exchange=SimpleNamespace(start=lambda: None, finish=lambda w: None))
    with pytest.raises(K.PiclesError, match=r"node 0 = \(3, 23\) lies outside"):
        sl.backend.probe_init(np.array([[3, 23]]))
    sl.backend.probe_init(np.array([[3, 24], [3, 47]]))
