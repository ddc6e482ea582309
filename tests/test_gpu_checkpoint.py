"""Exact restart on the GPU (picles_checkpoint_*, picles_amd/checkpointing.py): N steps in one go equal k steps -> checkpoint ->
load into a NEW context built from the same configuration -> N - k steps, bit for bit (State, particles, counters)."""
import json
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from picles_amd import _capi as K, configs
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import WaveGrowth2D
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.timesteppers import time_step

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    if a.dtype.kind == "f":
        a, b = a.view(np.uint64), b.view(np.uint64)
    bad = int((a != b).sum())
    assert bad == 0, f"{what}: {bad} of {a.size} values differ"


def _model(cfg):
    m = WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    return m


def _steps(m, cfg, k, fused):
    if k <= 0:
        return
    if fused:                              # run!-style: picles_run_steps, one fused launch per step
        m.upload_winds(m.clock.time, cfg.Δt)
        m.backend.run_steps(cfg.Δt, k)
        m.clock.time += k * cfg.Δt
        m.clock.iteration += k
    else:
        for _ in range(k):
            time_step(m, cfg.Δt, zero_first=True)


def _snap(m):
    z, on, bnd, st = m.backend.get_particles()
    return dict(State=m.backend.get_state(), z=z, on=on, boundary=bnd, status=st, counters=m.backend.get_counters())


def _check(a, b, what):
    for key in ("State", "z", "on", "boundary", "status"):
        _same(a[key], b[key], f"{what}: {key}")
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])


def _pickup(cfg, blob, t, it):
    """a new context from the same configuration, loaded as run(sim, pickup=...) loads it"""
    m = WaveGrowth2D(**cfg.model)
    m._wind_window = None
    m.upload_winds(t, cfg.Δt)
    m.backend.checkpoint_load(blob)
    m.clock.time, m.clock.iteration = t, it
    return m


def _save(m):
    m.backend.checkpoint_begin()
    return m.backend.checkpoint_end()


def _restart(make, N, k, fused):
    ref = _model(make())
    _steps(ref, make(), N, fused)
    want = _snap(ref)
    a = _model(make())
    _steps(a, make(), k, fused)
    blob = _save(a)
    b = _pickup(make(), blob, a.clock.time, a.clock.iteration)
    _check(_snap(a), _snap(b), "right after the load")
    _steps(b, make(), N - k, fused)
    _check(_snap(b), want, "after the restart")
    return blob, a


def _segment(blob, name, dtype):
    off = K.CKPT_HEADER_BYTES
    i = K.CKPT_SEGMENTS.index(name)
    so, sl = struct.unpack_from("<Q", blob, 80 + 8 * i)[0], struct.unpack_from("<Q", blob, 160 + 8 * i)[0]
    return np.frombuffer(bytes(blob[off + so: off + so + sl]), dtype=dtype)


def test_bench06_box_dp5_fused():
    _restart(lambda: configs.bench06_box(n=48), N=9, k=4, fused=True)


def _masked_generic():
    c = configs.bench06_box(n=40, U10=10.0, V10=3.0, periodic_grid=False)
    n, dx = 40, 2000.0
    mask = np.ones((n, n), dtype=bool)
    mask[12:20, 22:30] = False
    c.model["grid"] = TwoDCartesianGridMesh(dx * (n - 1), n, dx * (n - 1), n, mask=mask, periodic_boundary=(False, False))
    c.model["periodic_boundary"] = False
    c.model["ODEsets"].solver = "AutoTsit5"
    return c


def test_default_solver_carries_the_autoswitch_state():
    blob, a = _restart(_masked_generic, N=8, k=4, fused=False)
    asw = _segment(blob, "asw", np.int32)
    on = _segment(blob, "on", np.uint8)
    assert asw.size == a.backend.N
    assert int(((asw & 1) == 1)[(on == 1)].sum()) > 0, "no particle has Rosenbrock23 active at the checkpoint"


def test_time_varying_winds_with_a_calm_region():
    blob, a = _restart(lambda: configs.growing_decaying_winds(n=64, n_steps=10), N=8, k=3, fused=False)
    on = _segment(blob, "on", np.uint8)
    assert 0 < int(on.sum()) < on.size           # particles off in the calm half carried across


def test_wind_lattice_knot_inside_the_first_step_after_the_restart():
    def make():
        c = configs.bench06_box(n=40)
        from picles_amd.wind_emulator import GriddedWinds
        P = 2000.0 * 39
        x = np.linspace(0.0, P, 9)
        t = np.arange(0.0, 12 * 600.0 + 1.0, 900.0)        # knots every 1.5 steps: the step after k = 4 ([2400, 3000]) holds 2700
        X, Y, T = np.meshgrid(x, x, t, indexing="ij")
        c.model["winds"] = GriddedWinds(x, x, t, 9.0 * (1 + 0.2 * np.sin(2 * np.pi * X / P)) * (1 + T / 7200.0),
                                        6.0 * (1 + 0.2 * np.cos(2 * np.pi * Y / P)) * (1 - 0.3 * T / 7200.0))
        c.model["winds_static"] = False
        return c
    k = 4
    tk = K.load().picles_lattice_knots(0.0, 900.0, k * 600.0, 600.0, None)
    assert tk == 1
    _restart(make, N=8, k=k, fused=False)


def test_spherical_metric():
    _restart(lambda: configs.sphere_aqua(nx=46, ny=31, n_steps=6), N=6, k=2, fused=True)


def test_saving_does_not_perturb_the_run():
    make = lambda: configs.bench06_box(n=48)         # noqa: E731
    ref, a = _model(make()), _model(make())
    _steps(ref, make(), 8, True)
    _steps(a, make(), 3, True)                       # a fused step is pending here
    a.backend.checkpoint_begin()
    _steps(a, make(), 5, True)                       # enqueued while the copy-out runs
    a.backend.checkpoint_end()
    _check(_snap(a), _snap(ref), "with a checkpoint at step 3")


def test_begin_then_steps_then_end_gives_the_blob_of_step_k():
    make = lambda: configs.bench06_box(n=48)         # noqa: E731
    a, b = _model(make()), _model(make())
    for m in (a, b):
        _steps(m, make(), 4, True)
    want = _save(a)
    b.backend.checkpoint_begin()
    _steps(b, make(), 3, True)
    got = b.backend.checkpoint_end()
    _same(got, want, "blob")


def test_refusals_leave_the_context_as_it_was():
    make = lambda: configs.bench06_box(n=32)         # noqa: E731
    a = _model(make())
    _steps(a, make(), 3, True)
    blob = _save(a)
    ref = _model(make())
    _steps(ref, make(), 6, True)
    want = _snap(ref)

    def other(**kw):
        c = make()
        if "n" in kw:
            c = configs.bench06_box(n=kw["n"])
        if "mask" in kw:
            mask = np.ones((32, 32), dtype=bool); mask[5:9, 5:9] = False
            c.model["grid"] = TwoDCartesianGridMesh(2000.0 * 31, 32, 2000.0 * 31, 32, mask=mask, periodic_boundary=(True, True))
        if "solver" in kw:
            c.model["ODEsets"].solver = "Tsit5"
        if "r_g" in kw:
            c.model["ODEsets"].Parameters = dict(c.model["ODEsets"].Parameters, r_g=0.9)
        return WaveGrowth2D(**c.model)
    for kw in (dict(n=33), dict(mask=1), dict(solver=1), dict(r_g=1)):
        m = other(**kw)
        with pytest.raises(K.CheckpointError) as e:
            m.backend.checkpoint_load(blob)
        assert e.value.code == K.CKPT_E_CONFIG, (kw, e.value)
    # the loaded context first tries a truncated blob, a damaged one and a foreign one, then the real one
    b = _pickup(make(), blob, a.clock.time, a.clock.iteration)
    _steps(a, make(), 1, True)
    _steps(b, make(), 1, True)
    bad = blob.copy(); bad[K.CKPT_HEADER_BYTES + 1000] ^= 0x10
    foreign = blob.copy(); foreign[:8] = 0
    codes = []
    for buf in (blob[:-7], blob[:100], bad, foreign):
        with pytest.raises(K.CheckpointError) as e:
            b.backend.checkpoint_load(buf)
        codes.append(e.value.code)
    assert codes == [K.CKPT_E_SHORT, K.CKPT_E_SHORT, K.CKPT_E_CHECKSUM, K.CKPT_E_MAGIC]
    _steps(b, make(), 2, True)                        # continues bitwise as if no load had been tried
    _steps(a, make(), 2, True)
    _check(_snap(b), _snap(a), "after the refused loads")
    _check(_snap(b), want, "against the uninterrupted run")
    # in flight: refused too
    b.backend.checkpoint_begin()
    with pytest.raises(K.CheckpointError) as e:
        b.backend.checkpoint_load(blob)
    assert e.value.code == K.CKPT_E_BUSY
    b.backend.checkpoint_end()


def test_run_with_checkpointer_and_pickup_in_a_fresh_process(tmp_path):
    drv = ROOT / "tests" / "native" / "checkpoint_pickup_driver.py"
    from picles_amd.checkpointing import Checkpointer, list_checkpoints
    from picles_amd.simulations import run
    sys.path.insert(0, str(drv.parent))
    import checkpoint_pickup_driver as D
    m = WaveGrowth2D(**D.cfg().model)
    sim = Simulation(m, Δt=D.DT, stop_time=11 * D.DT)
    sim.output_writers["checkpointer"] = Checkpointer(m, schedule=4, dir=tmp_path, prefix="box")
    run(sim)
    assert m.clock.iteration == 12
    assert sorted(list_checkpoints(tmp_path, "box")) == [4, 8, 12]
    out = tmp_path / "picked.npz"
    r = subprocess.run([sys.executable, str(drv), str(tmp_path), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    ref = WaveGrowth2D(**D.cfg().model)
    sim = Simulation(ref, Δt=D.DT, stop_time=D.STOP)
    run(sim)
    assert int(got["iteration"]) == ref.clock.iteration == 20
    _same(got["State"], ref.backend.get_state(), "State after pickup")


def test_slabs_in_lock_step():
    from picles_amd.parallel import SlabModel
    import test_gpu_slab_fuzz as F
    make = lambda: configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 7.0, 96e3, 96e3))   # noqa: E731
    cfg = make()
    one = SlabModel(cfg.model, 0, 1, device=0)
    one.seed()
    one.run_steps(cfg.Δt, 8)
    S = one.get_state()
    z1, on1, _, st1 = one.backend.get_particles()
    world = 2
    slabs = [SlabModel(make().model, r, world, device=0, halo_rows=2, exchange=F._NoExchange()) for r in range(world)]
    for s in slabs:
        s.seed()
    for _ in range(3):
        F._step_all(slabs, cfg.Δt, True, True)
    for s in slabs:
        s.backend.set_halo_rows(3)                   # as grow_halo_if_needed does, collectively
    blobs = []
    for s in slabs:
        s.checkpoint_begin()
    for s in slabs:
        blobs.append((s.checkpoint_end(), s.clock))
    new = [SlabModel(make().model, r, world, device=0, halo_rows=2, exchange=F._NoExchange()) for r in range(world)]
    for s, (blob, clock) in zip(new, blobs):
        s.checkpoint_load(blob, clock)
        assert s.backend.halo_rows == 3
    for _ in range(5):
        F._step_all(new, cfg.Δt, True, True)
    for s in new:
        _same(s.get_state(), S[:, s.j0:s.j1], f"rank {s.rank} State")
        z, on, _, st = s.backend.get_particles()
        _same(on, on1[:, s.j0:s.j1], f"rank {s.rank} on")
        _same(st, st1[:, s.j0:s.j1], f"rank {s.rank} status")
        _same(z, z1[:, s.j0:s.j1], f"rank {s.rank} z")


def test_native_ring_over_the_loopback_communicator(tmp_path):
    so = tmp_path / "libloopback_ccl.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include",
                    str(ROOT / "tests" / "native" / "loopback_ccl.cpp"), "-o", str(so)], check=True, timeout=300)
    env = dict(os.environ, PICLES_CCL_LIB=str(so))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "native" / "checkpoint_ring_driver.py"), "2", "8", "3"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["mismatches"] == 0 and res["halo_rows"] == [3, 3], res
