"""Streamed winds on the GPU: a run whose wind levels are pushed one at a time into the ring of picles_wind_stream_*
against the same model under wind_interpolator with the whole lattice uploaded first (picles_set_wind_grid, the route
tests/test_wind_grid.py holds against NumPy and the oracle) — bit for bit: the sampler's planes, State, particles and counters over
every window form, whenever a level is pushed, from host and device memory in float64 and float32, through run(sim) with writers
and a restart; the refusals change nothing; picles_diag_export against push + pop.
The reference lattice always holds levels beyond the last time a run samples: its LAST level is evaluated as f = 1 of the interval
before, which is not the stream's form (a level alone)."""
import numpy as np
import pytest

from picles_amd import configs
from picles_amd import _capi as K
from picles_amd.coupling import StreamedWinds
from picles_amd.wind_emulator import wind_interpolator, IdealizedWindGrid
from picles_amd.simulations import Simulation, initialize_simulation, run
from helpers import make_model, assert_bitwise
from test_wind_grid import _lattice

pytestmark = pytest.mark.gpu

NSTEPS = 8


def _lat(interval, n_levels, f32=False):
    """the 13 x 11 spatial lattice and the smooth u, v of tests/test_wind_grid.py, n_levels time levels `interval` apart"""
    _, u, v = _lattice()
    lat = IdealizedWindGrid(u, v, dict(Lx=60e3, Ly=45e3, T=interval * (n_levels - 1)), dict(dx=5e3, dy=4.5e3, dt=interval))
    assert lat["x"].size == 13 and lat["y"].size == 11 and lat["t"].size == n_levels
    if f32:
        lat["u"], lat["v"] = (lat[k].astype(np.float32).astype(np.float64) for k in ("u", "v"))
    return lat


def _level(lat, k, dtype=np.float64):
    """level k as the push takes it: (ny, nx), x fastest"""
    return tuple(np.ascontiguousarray(lat[c][:, :, k].T.astype(dtype)) for c in ("u", "v"))


def _cfg(winds, solver="DP5"):
    cfg = configs.example_00_minimal(n=33, L=64e3)
    cfg.model["winds"] = winds
    cfg.model["winds_static"] = False
    cfg.model["ODEsets"].solver = solver
    return cfg


def _n_levels(dt, interval, slots=3):
    return int(np.ceil(NSTEPS * dt / interval)) + slots + 3


def _reference(lat, dt, solver="DP5", mode="linear", n=NSTEPS):
    m = make_model(_cfg(wind_interpolator(lat, time_mode=mode), solver), "hip")
    initialize_simulation(Simulation(m, Δt=dt, stop_time=1.0))
    m.upload_winds(0.0, dt)
    if n:
        m.backend.run_steps(dt, n)
    return m


def _streamed(lat, dt, slots, solver="DP5", mode="linear", level=None, source=None):
    """a model under StreamedWinds, seeded (level 0 pushed first: the seed reads the winds at t = 0)"""
    sw = StreamedWinds(lat["x"], lat["y"], float(lat["t"][0]), float(lat["t"][1] - lat["t"][0]), slots=slots, time_mode=mode, source=source)
    m = make_model(_cfg(sw, solver), "hip")
    if source is None:
        sw.attach(m)
        sw.push(0, *(level or (lambda k: _level(lat, k)))(0))
    initialize_simulation(Simulation(m, Δt=dt, stop_time=1.0))
    return m, sw


def _advance(m, sw, level, dt, n, early=False, ahead=2, max_chunk=3):
    """n steps through run_steps in chunks.  late: before a chunk only the levels its next `ahead` steps read are pushed, as far as the
    ring admits them (the slot of the clock's own level is kept); early: every level the ring admits.  Returns the chunk sizes"""
    b, done, chunks = m.backend, 0, []
    while done < n:
        t = b.clock
        slots, _, newest, _ = b.wind_stream_info()
        top = sw.coord(t)[0] + slots - 1
        want = top if early else min(top, sw.levels_of(t, t + min(ahead, n - done) * dt)[1])
        for k in range(newest + 1, want + 1):
            b.wind_stream_push(k, *level(k))
        newest = max(newest, want)
        c, tt = 0, t
        while c < min(max_chunk, n - done) and sw.levels_of(tt, tt + dt)[1] <= newest:
            c, tt = c + 1, tt + dt
        assert c >= 1, (t, newest)
        b.run_steps(dt, c)
        done += c
        chunks.append(c)
    return chunks


def _same_run(a, b, what):
    """State, particles, `on` and the counters rhs_evals and max_reach"""
    assert_bitwise(a.backend.get_state(), b.backend.get_state(), f"{what}: State")
    za, ona, _, sta = a.backend.get_particles()
    zb, onb, _, stb = b.backend.get_particles()
    assert_bitwise(ona, onb, f"{what}: on"); assert_bitwise(sta, stb, f"{what}: status")
    live = ((stb & 1) == 1) & (onb == 1)       # the state vector of a switched-off particle is dead storage
    for c in range(5):
        assert_bitwise(za[..., c][live], zb[..., c][live], f"{what}: z[{c}]")
    ca, cb = a.backend.get_counters(), b.backend.get_counters()
    for key in ("rhs_evals", "max_reach", "particles_advanced", "steps_accepted"):
        assert ca[key] == cb[key], (what, key, ca[key], cb[key])
    assert np.abs(b.backend.get_state()).max() > 0 and cb["rhs_evals"] > 0


_REF = {}


def _ref_of(dt, interval, solver="DP5", mode="linear", f32=False):
    """the lattice route's run of a case, made once and left alone"""
    key = (dt, interval, solver, mode, f32)
    if key not in _REF:
        lat = _lat(interval, _n_levels(dt, interval, 5), f32)
        _REF[key] = (lat, _reference(lat, dt, solver, mode))
    return _REF[key]


# ---- 1. the sampler ----
def test_sampler_planes_equal_the_lattice_routes():
    lat = _lat(900.0, 6)
    m, sw = _streamed(lat, 600.0, 3)
    r = _reference(lat, 600.0, n=0)
    for a, b, what in zip(m.backend.get_winds()[:2], r.backend.get_winds()[:2], ("u0", "v0")):
        assert_bitwise(a, b, f"seed window {what}")
    for k in (1, 2):
        sw.push(k, *_level(lat, k))
    assert m.backend.wind_stream_info() == (3, 0, 2, 3)
    for mm in (m, r):
        mm.backend.run_steps(600.0, 2)                     # [0, 600]: two levels; [600, 1200]: the knot at 900
    for a, b, what in zip(m.backend.get_winds(), r.backend.get_winds(), ("u0", "v0", "u1", "v1")):
        assert_bitwise(a, b, f"window [600, 1200] {what}")
    for a, b, what in zip(m.backend.get_winds_mid(), r.backend.get_winds_mid(), ("um", "vm")):
        assert_bitwise(a, b, f"knot level {what}")
    for mm in (m, r):
        mm.backend.run_steps(600.0, 1)                     # [1200, 1800] ends exactly ON the newest level, which is read alone
    assert m.backend.get_winds_mid() is None and r.backend.get_winds_mid() is None
    for a, b, what in zip(m.backend.get_winds(), r.backend.get_winds(), ("u0", "v0", "u1", "v1")):
        assert_bitwise(a, b, f"window [1200, 1800] {what}")
    # and it is the interpolant AT the level (NumPy, on a lattice that goes on beyond it)
    w = wind_interpolator(lat)
    assert_bitwise(m.backend.get_winds()[2], w.u(m.grid.data.x, m.grid.data.y, 1800.0), "u1 on the newest level vs NumPy")
    _same_run(m, r, "after three steps")


# ---- 2. runs, bit for bit, each level pushed just in time ----
@pytest.mark.parametrize("dt,interval,slots,solver,mode", [
    (512.0, 512.0, 2, "DP5", "linear"),           # TWO only
    (768.0, 512.0, 3, "DP5", "linear"),           # KNOT, or ends on knots
    (600.0, 900.0, 3, "DP5", "linear"),           # step ends on levels or clear of them
    (2048.0, 512.0, 5, "DP5", "linear"),          # three interior knots: POLYLINE, plain phases
    (512.0, 256.0, 3, "DP5", "smooth3"),          # SMOOTH3
    (768.0, 512.0, 3, "AutoTsit5", "linear"),
])
def test_streamed_run_equals_the_lattice_run(dt, interval, slots, solver, mode):
    lat, r = _ref_of(dt, interval, solver, mode)
    m, sw = _streamed(lat, dt, slots, solver, mode)
    chunks = _advance(m, sw, lambda k: _level(lat, k), dt, NSTEPS)
    assert sum(chunks) == NSTEPS
    assert m.backend.clock == r.backend.clock
    _same_run(m, r, f"dt {dt}, interval {interval}, {slots} slots, {solver}, {mode}")
    n_slots, oldest, newest, pushes = m.backend.wind_stream_info()
    assert n_slots == slots and pushes == newest + 1 and oldest == newest - slots + 1


def test_a_step_with_three_knots_is_refused_in_a_ring_of_four():
    lat, r = _ref_of(2048.0, 512.0)
    m, sw = _streamed(lat, 2048.0, 4)
    for k in (1, 2, 3):
        sw.push(k, *_level(lat, k))
    with pytest.raises(K.PiclesError, match=r"n_slots >= nk \+ 2"):
        m.backend.run_steps(2048.0, 1)
    with pytest.raises(K.PiclesError, match="still needs"):
        sw.push(4, *_level(lat, 4))
    assert m.backend.wind_stream_info() == (4, 0, 3, 4) and m.backend.clock == 0.0


# ---- 3. push timing ----
@pytest.mark.parametrize("dt,interval,slots", [(768.0, 512.0, 4), (600.0, 900.0, 3)])
def test_results_do_not_depend_on_when_a_level_is_pushed(dt, interval, slots):
    lat, r = _ref_of(dt, interval)
    level = lambda k: _level(lat, k)
    early, swe = _streamed(lat, dt, slots)
    late, swl = _streamed(lat, dt, slots)
    ce = _advance(early, swe, level, dt, NSTEPS, early=True)
    cl = _advance(late, swl, level, dt, NSTEPS, ahead=1, max_chunk=1)
    assert cl == [1] * NSTEPS and max(ce) > 1 and early.backend.wind_stream_info()[2] >= late.backend.wind_stream_info()[2]
    _same_run(early, late, "pushed early vs at the last moment")
    _same_run(early, r, "pushed early vs the lattice")


# ---- 4. sources ----
def test_host_and_device_pushes_in_both_precisions_give_the_same_bits():
    import torch
    dt, interval, slots = 768.0, 512.0, 3
    lat, r = _ref_of(dt, interval)
    dev = lambda k: tuple(torch.from_numpy(a).cuda() for a in _level(lat, k))
    m, sw = _streamed(lat, dt, slots, level=dev)
    _advance(m, sw, dev, dt, NSTEPS)
    _same_run(m, r, "device float64 tensors")
    flat = lambda k: tuple(a.reshape(-1) for a in dev(k))
    m, sw = _streamed(lat, dt, slots, level=flat)
    _advance(m, sw, flat, dt, NSTEPS)
    _same_run(m, r, "flat device float64 tensors")
    # float32: against a lattice built from the same float32 values widened (exact)
    lat32, r32 = _ref_of(dt, interval, f32=True)
    for what, lv in (("device float32 tensors", lambda k: tuple(torch.from_numpy(a).cuda() for a in _level(lat32, k, np.float32))),
                     ("host float32 arrays", lambda k: _level(lat32, k, np.float32)),
                     ("host float64 arrays of the widened values", lambda k: _level(lat32, k))):
        m, sw = _streamed(lat32, dt, slots, level=lv)
        _advance(m, sw, lv, dt, NSTEPS)
        _same_run(m, r32, what)
    with pytest.raises(ValueError, match="contiguous"):
        m.backend.wind_stream_push(99, dev(1)[0].T, dev(1)[1].T)
    with pytest.raises(ValueError, match="a level is 11 x 13"):
        m.backend.wind_stream_push(99, np.zeros(5), np.zeros(5))


def test_a_push_from_a_side_stream_waits_for_its_producer():
    """the planes are produced on a side torch stream behind a large matrix product that is still queued when the push is made, and
    overwritten on that stream right after it: the first proves the event into the context's stream, the second the event out of it"""
    import torch
    dt, interval, slots = 768.0, 512.0, 3
    lat, r = _ref_of(dt, interval)
    side = torch.cuda.Stream()
    big = torch.ones(4096, 4096, device="cuda", dtype=torch.float32)
    torch.cuda.synchronize()

    def level(k):
        u, v = (torch.from_numpy(a).cuda() for a in _level(lat, k))
        side.wait_stream(torch.cuda.current_stream())
        u.record_stream(side); v.record_stream(side)         # (read on the side stream long after this function has dropped them)
        with torch.cuda.stream(side):
            z = big
            for _ in range(6):
                z = (z @ big) * (1.0 / 4096.0)
            zero = (z[0, 0] * 0.0).double()                  # 0.0, known only once the products are done
            pu, pv = u + zero, v + zero
            m.backend.wind_stream_push(k, pu, pv)
            pu.fill_(1e9); pv.fill_(-1e9)                    # the caller reuses its buffers in stream order
        return None

    sw = StreamedWinds(lat["x"], lat["y"], 0.0, interval, slots=slots)
    m = make_model(_cfg(sw), "hip")
    sw.attach(m)
    level(0)
    initialize_simulation(Simulation(m, Δt=dt, stop_time=1.0))
    done = 0
    while done < NSTEPS:
        newest = m.backend.wind_stream_info()[2]
        for k in range(newest + 1, sw.levels_of(m.backend.clock, m.backend.clock + dt)[1] + 1):
            level(k)
        m.backend.run_steps(dt, 1)
        done += 1
    torch.cuda.synchronize()
    _same_run(m, r, "pushed from a side stream")


# ---- 5. refusals: nothing changed afterwards ----
def test_refusals_change_nothing():
    dt, interval = 768.0, 512.0
    lat, r = _ref_of(dt, interval)
    level = lambda k: _level(lat, k)
    # slab mode and a stream exclude each other, either way round
    sw = StreamedWinds(lat["x"], lat["y"], 0.0, interval, slots=2)
    m = make_model(_cfg(sw), "hip")
    sw.attach(m)
    with pytest.raises(K.PiclesError, match="holds a wind stream"):
        m.backend.set_slab_mode(True)
    s = make_model(_cfg(StreamedWinds(lat["x"], lat["y"], 0.0, interval)), "hip")
    s.backend.set_slab_mode(True)
    with pytest.raises(K.PiclesError, match="whole-grid context"):
        s.winds.attach(s)
    # the seed reads level 0
    with pytest.raises(K.PiclesError, match="level k = 0"):
        initialize_simulation(Simulation(m, Δt=dt, stop_time=1.0))
    m, sw = _streamed(lat, dt, 3)
    b = m.backend
    with pytest.raises(K.PiclesError, match=r"reads level k = 1 \(t = 512\)"):        # a step past the newest level
        b.run_steps(dt, 1)
    with pytest.raises(K.PiclesError, match="reads level k = 1"):
        b.time_step(dt, K.STEP_ZERO_FIRST)
    with pytest.raises(K.PiclesError, match="out of order"):                          # a push out of order
        sw.push(2, *level(2))
    with pytest.raises(K.PiclesError, match="out of order"):
        sw.push(0, *level(0))
    sw.push(1, *level(1)); sw.push(2, *level(2))
    with pytest.raises(K.PiclesError, match="still needs"):                           # a push onto a needed slot
        sw.push(3, *level(3))
    with pytest.raises(K.PiclesError, match="step 2 of this call"):
        b.run_steps(dt, 2)
    assert b.wind_stream_info() == (3, 0, 2, 3) and b.clock == 0.0
    b.run_steps(dt, 1)
    with pytest.raises(K.PiclesError, match="reads level k = 3"):
        b.run_steps(dt, 1)
    _advance(m, sw, level, dt, NSTEPS - 1)
    _same_run(m, r, "after the refusals")


# ---- 6. run(sim) ----
def test_run_with_a_source_and_writers_equals_the_lattice_run(tmp_path):
    from picles_amd.station_output import StationWriter, read_station_output
    from picles_amd.checkpointing import Checkpointer
    dt, interval, slots, n = 768.0, 512.0, 3, 8
    lat = _lat(interval, _n_levels(dt, interval, slots))
    nodes = [(3, 4), (16, 16), (29, 30)]
    asked = []

    def source(k):
        asked.append(k)
        return _level(lat, k)

    def sim_of(winds, d, stop_it, ck=None):
        m = make_model(_cfg(winds), "hip")
        sim = Simulation(m, Δt=dt, stop_time=dt * (stop_it - 1))
        sim.output_writers["stations"] = StationWriter(m, nodes=nodes, schedule=1, path=tmp_path / d, capacity=6, format="npy")
        if ck:
            sim.output_writers["checkpointer"] = Checkpointer(m, schedule=3, dir=tmp_path / ck)
        return m, sim
    stream = lambda: StreamedWinds(lat["x"], lat["y"], 0.0, interval, slots=slots, source=source)
    r, rsim = sim_of(wind_interpolator(lat), "lattice", n)
    run(rsim)
    m, sim = sim_of(stream(), "stream", n)
    run(sim)
    assert asked == sorted(set(asked)) and asked[0] == 0 and m.clock.iteration == n == r.clock.iteration
    a, b = read_station_output(tmp_path / "stream"), read_station_output(tmp_path / "lattice")
    assert a["iteration"].tolist() == b["iteration"].tolist() == list(range(n + 1))
    assert_bitwise(a["data"], b["data"], "station series")
    _same_run(m, r, "run(sim) with a source")
    # stopped after 5 steps (checkpoints at 3), picked up in a fresh model: the source is asked again for the levels around the clock
    m1, sim1 = sim_of(stream(), "part1", 5, ck="ck")
    run(sim1)
    del asked[:]
    m2, sim2 = sim_of(stream(), "part2", n, ck="ck")
    run(sim2, pickup=True)
    assert m2.clock.iteration == n and asked[0] == m2.winds.coord(3 * dt)[0]
    assert_bitwise(m2.backend.get_state(), m.backend.get_state(), "picked up vs uninterrupted: State")
    z2, on2, _, st2 = m2.backend.get_particles()
    z, on, _, st = m.backend.get_particles()
    assert_bitwise(on2, on, "picked up: on"); assert_bitwise(st2, st, "picked up: status")
    c = read_station_output(tmp_path / "part2")
    keep = c["iteration"] > 3
    assert_bitwise(c["data"][keep], a["data"][a["iteration"] > 3], "picked up: station series")
    # without a source a run that reaches a missing level raises the library's text
    sw = StreamedWinds(lat["x"], lat["y"], 0.0, interval, slots=slots)
    m3 = make_model(_cfg(sw), "hip")
    sw.attach(m3)
    sw.push(0, *_level(lat, 0)); sw.push(1, *_level(lat, 1))
    with pytest.raises(K.PiclesError, match="reads level k = 2"):
        run(Simulation(m3, Δt=dt, stop_time=dt * 3))


# ---- 7. the diagnostics into device tensors ----
@pytest.mark.parametrize("coarsen", [(4, 4), (1, 1)])
def test_diag_export_equals_push_and_pop(coarsen):
    import torch
    dt, interval = 768.0, 512.0
    lat, _ = _ref_of(dt, interval)
    m = _reference(lat, dt, n=3)
    b = m.backend
    b.diag_init(coarsen=coarsen, fields=K.DIAG_FIELDS, n_slots=1)
    nxc, nyc, nf, npart, _ = b.diag_shape()
    b.diag_push()
    f, p, _ = b.diag_pop()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ft = torch.full((nf, nyc, nxc), -1.0, device="cuda", dtype=torch.float32)
        pt = torch.full((npart, 7), -1.0, device="cuda", dtype=torch.float64)
        b.diag_export(ft, pt)
        total = ft[0].double().nansum()                        # a torch op on the caller's stream right behind the export sees the data
    ft0 = torch.zeros(nf * nyc * nxc, device="cuda", dtype=torch.float32)
    b.diag_export(ft0)                                       # flat, no partials, torch's default stream
    hs_sum = ft0[:nyc * nxc].double().nansum()
    torch.cuda.synchronize()
    want_f = np.ascontiguousarray(f.transpose(0, 2, 1))      # diag_pop's planes back in memory order: [n_fields, nyc, nxc]
    assert np.array_equal(ft.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    assert np.array_equal(pt.cpu().numpy().view(np.uint64), p.view(np.uint64))
    assert np.array_equal(ft0.cpu().numpy().view(np.uint32), ft.cpu().numpy().reshape(-1).view(np.uint32))
    want = float(np.nansum(f[0].astype(np.float64)))
    assert abs(float(total) - want) <= 1e-9 * max(abs(want), 1.0) and abs(float(hs_sum) - want) <= 1e-9 * max(abs(want), 1.0)
    assert np.nanmax(f[0]) > 0 and b.diag_pending == 0
    with pytest.raises(ValueError, match="contiguous float32 device tensor"):
        b.diag_export(torch.zeros(3, device="cuda"))
