"""Track samples on the GPU (picles_track_*, k_track.h; the contract: include/picles_hip.h "track samples"), through
HipModel.backend.  Every comparison is bit for bit (NaN equals NaN): the reference is the HOST ROUTE — a twin model stepped with
picles_time_step and read with get_state() after every step — put through the NumPy restatement of the sample rule in
tests/_track_numpy.py (the station definition of tests/_station_numpy.py over the four corners; before = the latest sample at a
clock <= t_k, after = the earliest at a clock >= t_k).

Grids: (P) 64 x 16 periodic; (K) 70 x 9 open with a 10 x 3 land block, ragged rows on k_step; (W) 128 x 12 open, which qualifies
for k_step_waverow; the 46 x 31 sphere.  DP5, winds (10, 3) on the boxes.  About 300 events per grid (tests/_track_numpy.py,
make_events).  The test counts, from the host route, the events with both slots valid (>= 150 asserted on every grid), those
sampled with one to three wet corners (>= 5) and those with none (>= 3).  A dry node needs land, coast or an open rim: (P) has
none, so there the last two counts are asserted to be zero; (W) has a rim and no land — a cell always has an interior corner —, so
there partly wet events are asserted and all-dry ones are not possible."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import _track_numpy as TN
from picles_amd import configs, _capi as K
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.station_output import locate_points
from helpers import assert_bitwise, make_model

pytestmark = pytest.mark.gpu

DX = 2000.0
N_STEPS = 6


def _box(shape, periodic, land=None):
    nx, ny = shape
    cfg = configs.bench06_box(n=16, dx=DX, U10=10.0, V10=3.0, periodic_grid=periodic)
    mask = None
    if land is not None:
        mask = np.ones(shape, dtype=bool)
        mask[land] = False
    cfg.model["grid"] = TwoDCartesianGridMesh(DX * (nx - 1), nx, DX * (ny - 1), ny, mask=mask, periodic_boundary=(periodic, periodic))
    assert cfg.model["ODEsets"].solver == "DP5"
    return cfg


GRIDS = {
    "P64x16": lambda: _box((64, 16), True),
    "K70x9": lambda: _box((70, 9), False, land=(slice(30, 40), slice(3, 6))),
    "W128x12": lambda: _box((128, 12), False),
    "sphere46x31": lambda: configs.sphere_aqua(nx=46, ny=31),
}
# (partly wet, all dry) events the host route must show, at least; None: none can exist on that grid (module docstring)
DRY_BOUNDS = {"P64x16": (None, None), "K70x9": (5, 3), "W128x12": (5, None), "sphere46x31": (5, 3)}


def _model(cfg, seeded=True):
    m = make_model(cfg, "hip")
    if seeded:
        initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
        m.upload_winds(m.clock.time, cfg.Δt)
    return m


def _everything(m):
    b = m.backend
    S = b.get_state()
    z, on, _, st = b.get_particles()
    return S, z, on, st, b.get_counters(), b.clock


def _assert_same_model(a, b, what):
    for x, y, name in zip(a[:4], b[:4], ("State", "z", "on", "status")):
        assert_bitwise(np.where(a[2][..., None] != 0, x, 0.0) if name == "z" else x,
                       np.where(b[2][..., None] != 0, y, 0.0) if name == "z" else y, f"{what}: {name}")     # (the z of an off particle is dead storage)
    assert a[4] == b[4], (what, a[4], b[4])
    assert a[5] == b[5], (what, a[5], b[5])


_ROUTES = {}


def _route(name, steps=None):
    """the host route of a grid, computed once: cfg maker, the sorted events with corners and weights, [(clock, State)] after the
    seed and after every step, and the final (State, particles, counters, clock) of that model — which never had a set"""
    key = (name, tuple(steps) if steps else None)
    if key in _ROUTES:
        return _ROUTES[key]
    cfg = GRIDS[name]()
    dts = list(steps) if steps else [cfg.Δt] * N_STEPS
    a = _model(cfg)
    b = a.backend
    samples = [(b.clock, b.get_state())]
    for dt in dts:
        b.time_step(dt, K.STEP_ZERO_FIRST)
        samples.append((b.clock, b.get_state()))
    clocks = [c for c, _ in samples]
    wets = [np.isfinite(S).all(axis=-1) & (S[..., 0] > 0) & (S[..., 1] ** 2 + S[..., 2] ** 2 > 0) for _, S in samples]
    wet, never = np.logical_and.reduce(wets), ~(wets[1] | wets[2])
    t, p = TN.make_events(cfg.model["grid"], bool(cfg.model.get("periodic_boundary", True)), clocks if not steps else
                          [clocks[0] + k * cfg.Δt for k in range(7)], cfg.Δt, wet=wet, never=never)
    order = np.argsort(t, kind="stable")
    corners, weights = locate_points(cfg.model["grid"], [tuple(q) for q in p[order]])
    ev = dict(t=t[order], corners=corners, weights=weights,
              ij=np.concatenate([corners[:, :, 0].T, corners[:, :, 1].T], axis=0), w=np.ascontiguousarray(weights.T))
    _ROUTES[key] = (cfg, ev, samples, _everything(a))
    return _ROUTES[key]


def _expected(ev, samples, H):
    tab = TN.Table(ev["t"], ev["corners"], ev["weights"], H)
    for T, S in samples:
        tab.sample(T, S)
    return tab


def _fetch(b, k0=0, n=None):
    b.track_fetch_begin(k0, b.track_info()[0] - k0 if n is None else n)
    return b.track_fetch_end()


def _with_set(name, ev, H):
    m = _model(GRIDS[name]())
    m.backend.track_init(ev["t"], ev["ij"], ev["w"], H)
    return m


# ---- 1. the table against the host route; 2. nothing perturbed ----
@pytest.mark.parametrize("name", list(GRIDS))
def test_table_equals_the_host_route_and_the_model_is_untouched(name):
    cfg, ev, samples, never = _route(name)
    dt = cfg.Δt
    want = _expected(ev, samples, dt)
    # the inputs have not degenerated: counted on the host route
    both = int((~np.isnan(want.tab).any(axis=0)).sum())
    seen = want.n_wet >= 0
    partly, dry = int(((want.n_wet > 0) & (want.n_wet < 4)).sum()), int((want.n_wet[seen] == 0).sum())
    sizes = [len(v) for v in want.visits]
    t, clocks = ev["t"], [c for c, _ in samples]
    print(f"{name}: {len(t)} events; both slots valid {both}, partly wet {partly}, all dry {dry}; visited per sample {sizes}")
    assert both >= 150
    lo_partly, lo_dry = DRY_BOUNDS[name]
    assert partly >= lo_partly if lo_partly is not None else partly == 0
    assert dry >= lo_dry if lo_dry is not None else dry == 0
    assert ((t > clocks[2]) & (t < clocks[3])).sum() > 64 and ((t > clocks[4]) & (t < clocks[5])).sum() == 0
    assert all((t == c).sum() >= 4 for c in (clocks[0], clocks[3], clocks[6])) and (np.diff(t) == 0).sum() >= 10
    assert (ev["weights"].max(axis=1) == 1.0).any() and ((ev["weights"] == 0.0).sum(axis=1) == 2).any()      # on a node, on a cell edge
    Nx = int(cfg.model["grid"].stats.Nx)
    assert ((ev["corners"][:, 0, 0] == Nx - 1) & (ev["corners"][:, 1, 0] == 0)).any() or ((ev["corners"][:, 1, 0] == Nx - 1) & (ev["weights"][:, 1] + ev["weights"][:, 3] == 1.0)).any()
    m = _with_set(name, ev, dt)
    b = m.backend
    assert b.track_info() == (len(t), dt, 0)
    assert_bitwise(_fetch(b), np.full((8, len(t)), np.nan), "the table after init")
    b.track_sample()
    b.enable_timing(True)
    b.run_steps(dt, N_STEPS)
    got = _fetch(b)
    # get_timing completes the pending step itself (one stand-alone scatter + remesh), so `<= 1` here shows only that no SAMPLE
    # completed a step (seven samples would be seven scatters); that a FETCH completes none is shown where fetches lie between
    # steps: test_fetch_hands_out_the_table_as_it_was_at_begin
    timing = b.get_timing()
    print(name, timing)
    assert timing["advance_launches"] == N_STEPS and timing["scatter_launches"] <= 1, timing
    assert b.track_info() == (len(t), dt, N_STEPS + 1)
    assert_bitwise(got, want.tab, f"{name}: table after the initial sample and run_steps({N_STEPS})")
    _assert_same_model(_everything(m), never, f"{name}: a model with a track set vs one that never had one")
    b.track_free()
    with pytest.raises(K.PiclesError, match="track_init first"):
        b.track_info()


# ---- 3. State in memory ----
def test_state_in_memory_is_gathered_and_follows_the_wet_rule():
    name = "K70x9"
    cfg, ev, _, _ = _route(name)
    dt = cfg.Δt
    m = _with_set(name, ev, dt)
    b = m.backend
    nx, ny = 70, 9
    rng = np.random.default_rng(5)
    e = np.exp(rng.uniform(np.log(0.05), np.log(4.0), (nx, ny)))
    th = rng.uniform(-np.pi, np.pi, (nx, ny))
    S = np.stack([e, e / 16.0 * np.cos(th), e / 16.0 * np.sin(th)], axis=-1)
    # hostile values at corners of events the first sample visits
    c = ev["corners"]
    ocean = np.asarray(cfg.model["grid"].data.mask) == 1
    k = [q for q in range(len(ev["t"])) if 0.0 <= ev["t"][q] - b.clock < dt and (ev["weights"][q] > 0).all()
         and all(ocean[i, j] for i, j in c[q])]          # events whose before slot the first sample writes, in all-ocean cells
    hostile = [(np.nan, 0), (np.inf, 0), (-np.inf, 1), (-1.0, 0), (np.nan, 2)]
    for q, (v, comp) in zip(k[:5], hostile):
        S[c[q, 0, 0], c[q, 0, 1], comp] = v
    S[c[k[5], 3, 0], c[k[5], 3, 1], 1:] = 0.0           # zero momentum
    S[c[k[6], 1, 0], c[k[6], 1, 1], 0] = 0.0            # zero energy
    b.set_state(S)
    b.remesh(dt)
    b.track_sample()
    S1, T1 = b.get_state(), b.clock
    want = _expected(ev, [(T1, S1)], dt)
    assert ((want.n_wet > 0) & (want.n_wet < 4)).sum() >= 7
    assert_bitwise(_fetch(b), want.tab, "sample of a State in memory (set_state + remesh)")
    b.advance(dt, K.STEP_ZERO_FIRST)
    b.remesh(dt)
    b.tick(dt)
    assert b.track_info()[2] == 1          # no automatic sample on this path
    b.track_sample()
    S2, T2 = b.get_state(), b.clock
    assert T2 > T1
    want.sample(T2, S2)
    assert_bitwise(_fetch(b), want.tab, "sample after advance + remesh + tick")


# ---- 4. uneven steps, and the horizon ----
def test_uneven_steps_and_a_step_beyond_the_horizon():
    name = "P64x16"
    dt = GRIDS[name]().Δt
    steps = [dt, dt / 2, dt / 2, dt, dt]
    cfg, ev, samples, _ = _route(name, steps)
    m = _with_set(name, ev, dt)
    b = m.backend
    b.track_sample()
    for s in steps[:4]:
        b.time_step(s, K.STEP_ZERO_FIRST)
    want = _expected(ev, samples[:5], dt)
    inside = (ev["t"] >= samples[0][0]) & (ev["t"] <= samples[4][0])
    clocks = np.array([c for c, _ in samples[:5]])
    for q in np.flatnonzero(inside):          # before is the latest, after the earliest sample clock around the event
        assert want.tab[3, q] == clocks[clocks <= ev["t"][q]].max() and want.tab[7, q] == clocks[clocks >= ev["t"][q]].min()
    assert_bitwise(_fetch(b), want.tab, "steps of dt, dt/2, dt/2, dt")
    clock = b.clock
    b.enable_timing(True)
    for call in (lambda: b.time_step(2 * dt, K.STEP_ZERO_FIRST), lambda: b.run_steps(2 * dt, 3)):
        with pytest.raises(K.PiclesError, match="longer than the horizon"):
            call()
    assert b.clock == clock and b.track_info()[2] == 5
    assert_bitwise(_fetch(b), want.tab, "the table after the refused steps")
    b.time_step(dt, K.STEP_ZERO_FIRST)      # a legal step succeeds, from records that are as they were
    got = _fetch(b)
    assert b.get_timing()["advance_launches"] == 1
    assert_bitwise(b.get_state(), samples[5][1], "State after the refused steps and a legal one")
    assert_bitwise(got, want.sample(*samples[5]).tab, "the table after the legal step")


# ---- 5. fetch overlap ----
def test_fetch_hands_out_the_table_as_it_was_at_begin():
    name = "W128x12"
    cfg, ev, samples, _ = _route(name)
    dt = cfg.Δt
    m = _with_set(name, ev, dt)
    b = m.backend
    b.enable_timing(True)
    b.track_sample()
    b.run_steps(dt, 3)
    at_begin = _expected(ev, samples[:4], dt)
    n_done = int(np.searchsorted(ev["t"], samples[3][0], side="right"))
    b.track_fetch_begin(0, len(ev["t"]))      # the completed events and the open ones behind them
    b.run_steps(dt, 2)                        # two more steps enqueued: they rewrite slots of the open events
    got = b.track_fetch_end()
    later = at_begin.copy().sample(*samples[4]).sample(*samples[5])
    changed = ~((later.tab == at_begin.tab) | (np.isnan(later.tab) & np.isnan(at_begin.tab))).all(axis=0)
    assert changed.sum() >= 20 and not changed[:n_done].any()
    assert_bitwise(got, at_begin.tab, "fetch_end: the values at fetch_begin")
    b.run_steps(dt, 1)                        # a step behind the completed fetch: had the fetch (or a sample) completed the pending step,
    later.sample(*samples[6])                 # that stand-alone scatter and the one get_timing launches below would make two
    assert_bitwise(_fetch(b, 0, n_done), later.tab[:, :n_done], "a later fetch of the completed events")
    assert_bitwise(_fetch(b, n_done), later.tab[:, n_done:], "a later fetch of the rest: the later table")
    timing = b.get_timing()                   # (completes the last step: the one stand-alone scatter there may be)
    assert timing["advance_launches"] == 6 and timing["scatter_launches"] <= 1, timing


# ---- 6. refusals ----
def test_refusals_leave_a_usable_context():
    name = "K70x9"
    cfg, ev, _, _ = _route(name)
    dt = cfg.Δt
    m = _model(GRIDS[name]())
    b = m.backend
    t, ij, w = ev["t"][:40].copy(), np.ascontiguousarray(ev["ij"][:, :40]), np.ascontiguousarray(ev["w"][:, :40])

    def step():
        b.time_step(dt, K.STEP_ZERO_FIRST)

    def raw_init(mm, H=dt):
        return b.lib.picles_track_init(b.h, mm, K.dptr(t), ij.astype(np.int32).ctypes.data_as(K.c_int32_p), K.dptr(w), H)

    def bad(text, tt=t, iij=ij, ww=w, H=dt):
        with pytest.raises(K.PiclesError, match=text):
            b.track_init(tt, iij, ww, H)
        with pytest.raises(K.PiclesError, match="track_init first"):
            b.track_info()
        step()

    assert raw_init(0) == -2 and b"m must be >= 1" in b.lib.picles_last_error(b.h)
    step()
    assert raw_init(2**28) == -2 and b"INT32_MAX" in b.lib.picles_last_error(b.h)      # refused before any array is read
    step()
    for q, v in ((3, t[2] - 1.0), (0, np.nan), (39, np.inf)):
        tt = t.copy(); tt[q] = v
        bad("finite and nondecreasing", tt=tt)
    for plane, v in ((0, 70), (2, -1), (4, 9), (7, -1)):
        iij = ij.copy(); iij[plane, 7] = v
        bad("outside the grid", iij=iij)
    for v in (-1e-300, np.nan, np.inf):
        ww = w.copy(); ww[1, 5] = v
        bad("finite and >= 0", ww=ww)
    for H in (0.0, -dt, np.inf, np.nan):
        bad("horizon must be finite and positive", H=H)
    with pytest.raises(K.PiclesError, match="track_init first"):
        b.track_sample()
    step()
    with pytest.raises(K.PiclesError, match="track_init first"):
        b.track_fetch_begin(0, 1)
    step()
    b.track_init(t, ij, w, dt)
    with pytest.raises(K.PiclesError, match="a track set exists"):
        b.track_init(t, ij, w, dt)
    step()
    with pytest.raises(K.PiclesError, match="no fetch is open"):
        b.track_fetch_end()
    step()
    for k0, n in ((-1, 2), (0, 0), (0, 41), (40, 1), (39, 2)):
        with pytest.raises(K.PiclesError, match="outside"):
            b.track_fetch_begin(k0, n)
        step()
    b.track_fetch_begin(0, 40)
    with pytest.raises(K.PiclesError, match="a fetch is open"):
        b.track_fetch_begin(0, 1)
    step()
    assert b.track_fetch_end().shape == (8, 40)
    # the native ring with a set: refused before the communicator library is looked for (the other way round:
    # test_init_is_refused_on_the_native_ring)
    with pytest.raises(K.PiclesError, match="track set"):
        b.slab_comm_init(bytes(K.SLAB_ID_BYTES), 0, 1)
    step()
    b.track_free()
    b.track_free()                                          # (nothing to free: no error)
    b.track_init(t, ij, w, dt)                              # a second init after the free works
    b.track_sample()
    step()
    assert b.track_info()[0] == 40 and b.track_info()[2] == 2 and np.isfinite(b.get_state()).all()
    b.track_fetch_begin(5, 20)
    b.close()                                               # destroy with a set and an open fetch
    # slab mode, either way round (before the seed, where the mode can change)
    fresh = _model(GRIDS[name](), seeded=False)
    fresh.backend.track_init(t, ij, w, dt)
    with pytest.raises(K.PiclesError, match="track set"):
        fresh.backend.set_slab_mode(True)
    fresh.backend.track_free()
    fresh.backend.set_slab_mode(True)
    with pytest.raises(K.PiclesError, match="whole-grid context"):
        fresh.backend.track_init(t, ij, w, dt)
    fresh.backend.set_slab_mode(False)                      # the refusal left the context as it was
    fresh.backend.track_init(t, ij, w, dt)
    initialize_simulation(Simulation(fresh, Δt=dt, stop_time=1.0))
    fresh.backend.time_step(dt, K.STEP_ZERO_FIRST)
    assert fresh.backend.track_info()[2] == 1 and fresh.backend.get_state()[..., 0].max() > 0.0
    # a slab context
    from picles_amd import fetch_relations as FR
    from picles_amd.driver import HipModel
    from picles_amd.models import build_structs
    c2 = GRIDS[name]()
    ms = FR.MinimalState(2, 2, c2.model["ODEsets"].timestep)
    g, p, o, mo = build_structs(c2.model["grid"], c2.model["ODEsys"], c2.model["ODEsets"], None, ms, False, j_begin=2, j_end=7)      # rows 2 .. 6
    slab = HipModel(g, p, o, mo, mask=c2.model["grid"].data.mask, device=0, halo_rows=2)
    with pytest.raises(K.PiclesError, match="whole-grid context"):
        slab.track_init(t, ij, w, dt)
    slab.close()


def test_init_is_refused_on_the_native_ring(tmp_path):
    """a whole-grid context on a ring of one, through the thread loopback communicator of tests/test_gpu_loopback_ring.py, in a fresh
    process (the communicator library is bound once per process): the init is refused and leaves no set, the ring steps, and with the
    ring gone the same init succeeds and the context samples"""
    root = Path(__file__).resolve().parent.parent
    so = tmp_path / "libloopback_ccl.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include",
                    str(root / "tests" / "native" / "loopback_ccl.cpp"), "-o", str(so)], check=True)
    r = subprocess.run([sys.executable, str(root / "tests" / "native" / "track_ring_driver.py")], capture_output=True, text=True,
                       env=dict(os.environ, PICLES_CCL_LIB=str(so)), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    dt = 600.0
    assert res["refusal"] and "whole-grid context" in res["refusal"] and "native ring" in res["refusal"], res
    assert res["set_after_refusal"] is False and res["clock_after_ring_steps"] == 2 * dt, res
    assert res["info"] == [3, dt, 1], res
    assert res["t_before"] == [None, None, None] and res["t_after"] == [None, None, 3 * dt] and res["state_finite"], res


# ---- 7. checkpoint ----
def test_checkpoint_load_keeps_the_table_and_a_sample_follows_the_restored_clock():
    name = "P64x16"
    cfg, ev, samples, _ = _route(name)
    dt = cfg.Δt
    m = _with_set(name, ev, dt)
    b = m.backend
    b.track_sample()
    b.run_steps(dt, 3)
    b.checkpoint_begin()
    blob = b.checkpoint_end()
    b.run_steps(dt, 2)
    want = _expected(ev, samples[:6], dt)
    assert_bitwise(_fetch(b), want.tab, "before the load")
    b.checkpoint_load(blob)
    assert b.clock == samples[3][0]
    assert_bitwise(_fetch(b), want.tab, "checkpoint_load leaves the table alone")
    b.track_sample()                       # at the restored clock, of the restored State
    assert_bitwise(_fetch(b), want.sample(*samples[3]).tab, "a fresh sample follows the restored clock")
    b.run_steps(dt, 1)
    assert_bitwise(b.get_state(), samples[4][1], "the restored model steps as before")
