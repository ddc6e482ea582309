"""Coupling fluxes on the device (picles_flux_*, k_flux): planes and tile partials BIT FOR BIT against the host build of flux_node
(tests/native/flux_host.cpp: the same header, compiled for the CPU) with NumPy doing the coarsening, the scale, the float32 rounding
and the tile tree in the stated order (tests/_flux_numpy.py) — on a smooth-winds box after six fused steps with the last step still
pending, and on the hostile planes of tests/_hostile_states.py.  Bitwise equality with the host build proves the device runs the same
source; that something physical is compared is held by the literal restatement of the reference's formulas, within one float32 unit
in the last place on the smooth case.  Then: mask subsets, export into torch tensors, no side effect on the model, the wind rule
(host-set windows, a lattice, a wind stream), slabs, a sphere, FluxWriter through run(), coupling.FluxExport and the example on it.

Which shape reaches which instantiation of k_flux<CX, VEC> (VEC: Nx even):
    70 x 37 (4, 3)    <4, true>, ragged last cell in both directions (2 columns, 1 row)
    520 x 9 (2, 1)    <2, true>, Nxc = 260: two tiles per row, the second with four lanes
    64 x 16 (1, 1)    <1, false>, no coarsening
    96 x 24 (16, 16)  <0, false>, the largest factor, ragged in y (24 = 16 + 8)
    45 x 28 (2, 3), 61 x 33 (4, 2)   <2, false>, <4, false> (odd Nx; hostile planes only), the last cell one column wide"""
import numpy as np
import pytest

import _flux_numpy as F
import _hostile_states as H
from helpers import assert_bitwise, assert_same_bits, bits_of, make_model
from picles_amd import _capi as K, configs, fetch_relations
from picles_amd.driver import HipModel, combine_flux_partials
from picles_amd.flux_output import G0, SCALAR_NAMES, FluxWriter, read_flux_output
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import build_structs
from picles_amd.parallel import SlabModel, slab_rows
from picles_amd.simulations import Simulation, initialize_simulation, run

pytestmark = pytest.mark.gpu

SHAPES = {"70x37_4x3": (70, 37, 4, 3), "520x9_2x1": (520, 9, 2, 1), "64x16_1x1": (64, 16, 1, 1), "96x24_16x16": (96, 24, 16, 16)}
ODD = {"45x28_2x3": (45, 28, 2, 3), "61x33_4x2": (61, 33, 4, 2)}
SCALES = (1025.0 * G0, 1025.0)          # W m-2 and N m-2 at rho_water = 1025
DX = 2000.0


def _box(nx, ny, winds="smooth"):
    """the periodic bench06 box on an nx x ny mesh, under smooth winds (None: the constant ones)"""
    cfg = configs.bench06_box(n=nx, winds=configs.smooth_winds(10.0, 10.0, DX * nx, DX * ny) if winds == "smooth" else None)
    cfg.model["grid"] = TwoDCartesianGridMesh(DX * (nx - 1), nx, DX * (ny - 1), ny, periodic_boundary=(True, True))
    return cfg


def _ready(cfg):
    """a seeded model whose backend can be driven directly (winds uploaded for run_steps)"""
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    m.upload_winds(0.0, cfg.Δt)
    return m


def _structs(m):
    _, p, _, _ = build_structs(m.grid, m.ODEsystem, m.ODEsettings, m.ODEdefaults, m.minimal_state, m.periodic_boundary)
    return p, list(m.minimal_state)


def _reference(phys, ms, S, u, v, pair, names=K.FLUX_FIELDS, scales=SCALES, nodes=F.host_nodes):
    """planes and partials of State S under the wind planes (u, v): flux_node per node on the host, the rest in NumPy"""
    with np.errstate(all="ignore"):
        vals, st = nodes(phys, ms, S[..., 0], S[..., 1], S[..., 2], u, v)
        return F.planes_of(vals, st, *pair, *scales, names=names), F.partials_of(vals, st, *pair), st


def _snapshot(b):
    b.flux_push()
    return b.flux_pop()


def _ulps(a, b):
    """distance of two float32 arrays in units in the last place (same sign or zero)"""
    ia, ib = bits_of(a).astype(np.int64), bits_of(b).astype(np.int64)
    assert ((ia >> 31) == (ib >> 31)).all() or ((a == 0) | (b == 0) | (np.sign(a) == np.sign(b))).all()
    return np.abs((ia & 0x7FFFFFFF) - (ib & 0x7FFFFFFF))


# ---- planes and partials, bit for bit ----
@pytest.mark.parametrize("case", list(SHAPES))
def test_smooth_box_bitwise_with_the_last_step_pending(case):
    import torch
    nx, ny, cx, cy = SHAPES[case]
    m = _ready(_box(nx, ny))
    b, dt = m.backend, 600.0
    phys, ms = _structs(m)
    b.flux_init((cx, cy), K.FLUX_FIELDS, *SCALES, 2)
    nxc, nyc = F.coarse_shape(nx, ny, cx, cy)
    assert b.flux_shape() == (nxc, nyc, 9, nyc * -(-nxc // 256), 4 * nxc * nyc * 9)
    b.run_steps(dt, 6)                                   # six fused steps: the scatter and remesh of the sixth are still pending
    f, p, t = _snapshot(b)
    assert t == b.clock == 6 * dt and b.flux_pending == 0
    S = b.get_state()
    u0, v0, _, _ = b.get_winds()                         # a static window: its only level
    want_f, want_p, st = _reference(phys, ms, S, u0, v0, (cx, cy))
    assert f.dtype == np.float32 and f.shape == want_f.shape == (9, nxc, nyc) and p.shape == want_p.shape
    assert_same_bits(f, want_f, f"{case}: planes")
    assert_same_bits(p, want_p, f"{case}: partials")
    assert (st == 1).all() and p[:, 9].sum() == nx * ny and p[:, 10].sum() == 0
    assert np.isfinite(f).all() and (f[:2] > 0).all() and (np.abs(f).max(axis=(1, 2)) > 0).all()
    # something physical: within one float32 unit in the last place of the reference's formulas in their literal order
    lit_f, _, _ = _reference(phys, ms, S, u0, v0, (cx, cy), nodes=F.literal_nodes)
    d = _ulps(f, lit_f)
    print(f"{case}: planes against the literal restatement: {int((d > 0).sum())} of {d.size} values differ, by at most {int(d.max())} float32 ulp")
    assert d.max() <= 1
    tot = combine_flux_partials(p)
    assert tot == F.combine([want_p]) and tuple(tot) == SCALAR_NAMES
    # a wind sea under the wind that raised it takes energy in and spends a part of it; the stress points down the wind
    assert 0 < tot["sum_phi_dis"] < tot["sum_phi_in"] and tot["sum_tq_in_x"] > 0 and tot["sum_tq_in_y"] > 0 and tot["sum_us_x"] > 0
    # export into torch tensors: the bits of push + pop
    tf = torch.full((9, nyc, nxc), -1.0, dtype=torch.float32, device="cuda")
    tp = torch.full((p.shape[0], 11), -1.0, dtype=torch.float64, device="cuda")
    b.flux_export(tf, tp)
    torch.cuda.current_stream().synchronize()
    assert_same_bits(tf.cpu().numpy().transpose(0, 2, 1), f, f"{case}: exported planes")
    assert_same_bits(tp.cpu().numpy(), p, f"{case}: exported partials")
    tf.fill_(-1.0)
    b.flux_export(tf)                                    # without a partials buffer
    torch.cuda.current_stream().synchronize()
    assert_same_bits(tf.cpu().numpy().transpose(0, 2, 1), f, f"{case}: exported planes, no partials")
    # a subset mask gives the same planes, and the same partials, as the full mask
    names = ("us_y", "phi_dis", "tq_in_x", "phi_shift")
    b.flux_free()
    b.flux_init((cx, cy), names, *SCALES, 1)
    assert b.flux_fields == ("phi_dis", "phi_shift", "tq_in_x", "us_y") and b.flux_shape()[2] == 4
    f4, p4, _ = _snapshot(b)
    assert_same_bits(f4, f[[1, 2, 3, 8]], f"{case}: subset mask")
    assert_same_bits(p4, p, f"{case}: subset mask, partials")
    # unit scales: the planes are the unscaled area means
    b.flux_free()
    b.flux_init((cx, cy), K.FLUX_FIELDS, 1.0, 1.0, 1)
    f1, _, _ = _snapshot(b)
    assert_same_bits(f1, _reference(phys, ms, S, u0, v0, (cx, cy), scales=(1.0, 1.0))[0], f"{case}: unit scales")
    assert_same_bits(f1[7:], f[7:], f"{case}: the Stokes drift carries no scale")
    b.close()


def _bare(Nx, Ny, rows=None):
    """a bare context on an Nx x Ny mesh (rows = (j_begin, j_end): a slab of it), with the C structs the host build takes"""
    cfg = configs.example_00_minimal(n=9, L=16e3)
    grid = TwoDCartesianGridMesh(DX * (Nx - 1), Nx, DX * (Ny - 1), Ny)
    ms = fetch_relations.MinimalState(2, 2, cfg.model["ODEsets"].timestep)
    j0, j1 = rows if rows else (0, None)
    g, p, o, mm = build_structs(grid, cfg.model["ODEsys"], cfg.model["ODEsets"], None, ms, False, j_begin=j0, j_end=j1)
    return HipModel(g, p, o, mm, mask=grid.data.mask, device=0, halo_rows=2), p, list(ms)


def _hostile_winds(Nx, Ny, seed):
    """ordinary winds with calm nodes, vanishing, huge, infinite and NaN entries among them"""
    rng = np.random.default_rng(seed)
    u, v = rng.normal(0.0, 9.0, (Nx, Ny)), rng.normal(0.0, 9.0, (Nx, Ny))
    k = rng.choice(8, (Nx, Ny), p=[0.72, 0.08, 0.04, 0.04, 0.04, 0.03, 0.03, 0.02])
    u[k == 1] = 0.0; v[k == 1] = 0.0
    u[k == 2] = 1e-160; v[k == 2] = -1e-170
    u[k == 3] = 3e3; v[k == 4] = -1e200
    u[k == 5] = np.inf; v[k == 6] = np.nan
    u[k == 7] = -0.0
    return u, v


@pytest.mark.parametrize("case", list(SHAPES) + list(ODD))
def test_hostile_planes_bitwise(case):
    nx, ny, cx, cy = {**SHAPES, **ODD}[case]
    b, phys, ms = _bare(nx, ny)
    # (the 16 x 16 case has twelve coarse cells: a seed whose cell plans leave a third of the nodes active)
    S = H.hostile_state(nx, ny, cx, cy, seed=801 if case == "96x24_16x16" else 700 + len(case) + nx)
    u, v = _hostile_winds(nx, ny, seed=nx + ny)
    b.set_winds(u, v, 0.0)
    b.set_state(S)
    names = K.FLUX_FIELDS if case != "61x33_4x2" else ("phi_in", "tq_dis_y", "us_x")
    b.flux_init((cx, cy), names, *SCALES, 2)
    b.flux_push()
    b.flux_push()
    f, p, _ = b.flux_pop()
    f2, p2, _ = b.flux_pop()
    assert_same_bits(f2, f, "second slot: planes"); assert_same_bits(p2, p, "second slot: partials")
    assert_same_bits(b.get_state(), S, f"{case}: State as set", nan_payload=True)
    want_f, want_p, st = _reference(phys, ms, S, u, v, (cx, cy), names=names)
    assert_same_bits(f, want_f, f"{case}: planes")
    assert_same_bits(p, want_p, f"{case}: partials")
    # the case is not empty: active, inactive and bad nodes, cells with no active node, and never a NaN or an infinity of the
    # kernel's own making in a plane (a float32 overflow of a finite mean is the rounding the definition asks for)
    n = np.bincount(st.reshape(-1), minlength=3)
    print(f"{case}: {n[1]} active, {n[0]} inactive, {n[2]} bad nodes")
    assert n[0] > 0.1 * st.size and n[1] > 0.1 * st.size and n[2] >= 3
    assert not np.isnan(f).any() and (f == 0).any()
    assert p[:, 9].sum() == n[1] and p[:, 10].sum() == n[2]
    b.close()


# ---- no side effect ----
def test_a_push_leaves_the_model_as_a_flush_does():
    def go(with_flux):
        b = _ready(_box(48, 24)).backend
        if with_flux:
            b.flux_init((4, 4), K.FLUX_FIELDS, *SCALES, 3)
        for k in (2, 3, 1):
            b.run_steps(600.0, k)
            if with_flux:
                b.flux_push()
            else:
                b.get_state()                            # the twin only flushes
        b.checkpoint_begin()
        blob = b.checkpoint_end()
        b.time_step(600.0, K.STEP_ZERO_FIRST)
        if with_flux:
            while b.flux_pending:
                b.flux_pop()
        z, on, bnd, st = b.get_particles()
        return b.get_state(), np.where(on[..., None] != 0, z, 0.0), on, bnd, st, blob, b.get_counters(), b.clock
    A, B = go(True), go(False)
    for x, y, what in zip(A[:6], B[:6], ("State", "particles", "on", "boundary", "status", "restart blob")):
        assert_bitwise(x, y, what)
    assert A[6] == B[6] and A[7] == B[7]


# ---- the wind rule ----
def _levels(nx, ny):
    x, y = np.meshgrid(np.arange(nx) / nx, np.arange(ny) / ny, indexing="ij")
    u0, v0 = 9.0 + 2.0 * np.sin(2 * np.pi * x), 4.0 + np.cos(2 * np.pi * y)
    return u0, v0, u0 + 3.0 * np.cos(2 * np.pi * y), v0 - 2.5 * np.sin(2 * np.pi * x)


def test_wind_rule_host_window_end_level_and_refusal_inside():
    nx, ny, dt = 48, 24, 600.0
    def make():
        m = _ready(_box(nx, ny, winds=None))
        b = m.backend
        u0, v0, u1, v1 = _levels(nx, ny)
        b.set_winds(u0, v0, 0.0, u1, v1, dt)             # a host two-level window over the first step
        return m, b
    (m, b), (_, twin) = make(), make()
    phys, ms = _structs(m)
    b.flux_init((4, 3), K.FLUX_FIELDS, *SCALES, 2)
    # the clock at the window's start: level 0
    f, p, _ = _snapshot(b)
    w = b.get_winds()
    assert_same_bits(f, _reference(phys, ms, b.get_state(), w[0], w[1], (4, 3))[0], "clock at the window's start: (u0, v0)")
    # ... at its end, with the step still pending: the planes used are (u1, v1)
    b.time_step(dt, K.STEP_ZERO_FIRST); twin.time_step(dt, K.STEP_ZERO_FIRST)
    f, p, t = _snapshot(b)
    assert t == dt
    w, S = b.get_winds(), b.get_state()
    assert_same_bits(f, _reference(phys, ms, S, w[2], w[3], (4, 3))[0], "clock at the window's end: (u1, v1)")
    assert not np.array_equal(f, _reference(phys, ms, S, w[0], w[1], (4, 3))[0])
    # a clock moved inside the window is refused, with the remedy, before anything is launched ...
    b.tick(-0.25 * dt); twin.tick(-0.25 * dt)
    import torch
    with pytest.raises(K.PiclesError, match=r"picles_flux_push.*holds no level at the clock 450.*step to a level.*set the window"):
        b.flux_push()
    with pytest.raises(K.PiclesError, match=r"picles_flux_export.*step to a level"):
        b.flux_export(torch.zeros((9, 8, 12), dtype=torch.float32, device="cuda"))
    assert b.flux_pending == 0
    # ... and the context steps on equal to the twin nobody asked
    b.tick(0.25 * dt); twin.tick(0.25 * dt)
    for x in (b, twin):
        u0, v0, u1, v1 = _levels(nx, ny)
        x.set_winds(u1, v1, dt, u0, v0, 2 * dt)
        x.time_step(dt, K.STEP_ZERO_FIRST)
    assert b.clock == twin.clock == 2 * dt
    assert_bitwise(b.get_state(), twin.get_state(), "State after the refusal")
    f, _, _ = _snapshot(b)
    w = b.get_winds()
    assert_same_bits(f, _reference(phys, ms, b.get_state(), w[2], w[3], (4, 3))[0], "the next window's end")
    b.close(); twin.close()


def test_wind_rule_lattice_through_run_steps_and_between_levels():
    make = lambda: configs.growing_decaying_winds_lattice(n=48, n_steps=8)      # noqa: E731
    m, m2 = _ready(make()), _ready(make())
    b, twin, dt = m.backend, m2.backend, make().Δt
    phys, ms = _structs(m)
    b.flux_init((4, 4), K.FLUX_FIELDS, *SCALES, 2)
    b.run_steps(dt, 3); twin.run_steps(dt, 3)
    f, p, t = _snapshot(b)
    assert t == 3 * dt
    w, S = b.get_winds(), b.get_state()
    assert not np.array_equal(w[0], w[2])                                       # the wind does vary over the step
    assert_same_bits(f, _reference(phys, ms, S, w[2], w[3], (4, 4))[0], "lattice: the level the last step's window ends on")
    # a clock between the window's levels: the level is sampled at the clock — the twin's next step starts its window there
    b.tick(0.25 * dt); twin.tick(0.25 * dt)
    f, p, t = _snapshot(b)
    assert t == 3.25 * dt
    twin.get_state()                                     # (completes the pending step: its successor does not start where it ended)
    twin.time_step(dt, K.STEP_ZERO_FIRST)
    tw = twin.get_winds()
    assert not np.array_equal(tw[0], w[2])
    assert_same_bits(f, _reference(phys, ms, S, tw[0], tw[1], (4, 4))[0], "lattice: sampled at the clock")
    # and the context that was asked steps on as the twin does
    b.time_step(dt, K.STEP_ZERO_FIRST)
    assert_bitwise(b.get_state(), twin.get_state(), "State after the sampled snapshot")
    b.close(); twin.close()


# ---- refusals ----
def test_refusals_leave_the_context_usable():
    m = _ready(_box(48, 24))
    b = m.backend
    b.run_steps(600.0, 2)
    with pytest.raises(K.PiclesError, match="picles_flux_init first"):
        b.flux_push()
    with pytest.raises(K.PiclesError, match="picles_flux_init first"):
        b.flux_free()
    with pytest.raises(K.PiclesError):
        b.flux_shape()
    for bad in ((0, 2), (17, 2), (2, 0), (2, 17)):
        with pytest.raises(K.PiclesError, match="1 ... 16"):
            b.flux_init(bad, ("phi_in",), 1.0, 1.0, 2)
    for mask in (0, 512, 1 << 20, -1):
        with pytest.raises(K.PiclesError, match="field mask"):
            b.flux_init((2, 2), mask, 1.0, 1.0, 2)
    for sp, st in ((0.0, 1.0), (1.0, -1.0), (np.inf, 1.0), (1.0, np.nan)):
        with pytest.raises(K.PiclesError, match="finite and positive"):
            b.flux_init((2, 2), ("phi_in",), sp, st, 2)
    with pytest.raises(K.PiclesError, match="n_slots"):
        b.flux_init((2, 2), ("phi_in",), 1.0, 1.0, 0)
    assert b.flux_pending == 0
    b.flux_init((2, 2), ("phi_in", "us_x"), 1.0, 1.0, 2)
    with pytest.raises(K.PiclesError, match="already initialised"):
        b.flux_init((2, 2), ("phi_in",), 1.0, 1.0, 2)
    with pytest.raises(K.PiclesError, match="no flux snapshot"):
        b.flux_pop()
    b.flux_push(); b.flux_push()
    with pytest.raises(K.PiclesError, match="ring full"):
        b.flux_push()
    assert b.flux_pending == 2
    # a load is refused beside a flux snapshot in flight as it is beside a store snapshot; the diagnostics mask knows no flux bit
    b.checkpoint_begin()
    blob = b.checkpoint_end()
    with pytest.raises(K.CheckpointError) as e:
        b.checkpoint_load(blob)
    assert e.value.code == K.CKPT_E_BUSY
    b.flux_pop(); b.flux_pop()
    b.checkpoint_load(blob)
    with pytest.raises(K.PiclesError, match="field mask"):
        b.diag_init((2, 2), 128, 2)
    # a slab whose first row is not a multiple of cy
    hm, _, _ = _bare(48, 48, rows=(8, 24))
    with pytest.raises(K.PiclesError, match="multiple of cy"):
        hm.flux_init((2, 3), ("phi_in",), 1.0, 1.0, 2)
    hm.flux_init((2, 4), ("phi_in",), 1.0, 1.0, 2)
    assert hm.flux_shape()[:2] == (24, 4)
    hm.close(); b.close()


# ---- slabs ----
@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_whole_grid_planes_and_totals(world):
    from test_gpu_slab_fuzz import _NoExchange, _step_all
    make = lambda: _box(64, 48)      # noqa: E731
    cfg = make()
    pair = (2, 4)
    assert all(slab_rows(48, world, r)[0] % pair[1] == 0 for r in range(world))
    one = SlabModel(cfg.model, 0, 1, device=0)
    one.flux_init(pair, K.FLUX_FIELDS, *SCALES, 2)
    one.seed()
    for _ in range(4):
        one.time_step(cfg.Δt)
    one.flux_push()
    f1, s1, t1 = one.gather_fluxes()
    slabs = [SlabModel(make().model, r, world, device=0, halo_rows=2, exchange=_NoExchange()) for r in range(world)]
    for s in slabs:
        s._comm_warm = True
        s.flux_init(pair, K.FLUX_FIELDS, *SCALES, 2)
        s.seed()
    for _ in range(4):
        _step_all(slabs, cfg.Δt, slabs[0].periodic_y, fused_ok=True)
    for s in slabs:
        s.flux_push()
    pops = [s.flux_pop() for s in slabs]
    assert_bitwise(np.concatenate([s.get_state() for s in slabs], axis=1), one.get_state(), "slab State")
    j = 0
    for r, (f, _, t) in enumerate(pops):                # row block after row block
        assert_same_bits(f, f1[:, :, j:j + f.shape[2]], f"{world} slabs: planes of rank {r}")
        j += f.shape[2]
        assert t == t1
    assert j == f1.shape[2]
    s2 = combine_flux_partials([p for _, p, _ in pops])
    for k in SCALAR_NAMES:
        assert_same_bits(np.array([s2[k]]), np.array([s1[k]]), f"{world} slabs: total {k}")
    assert s1["n_active"] == 64 * 48 and s1["n_bad"] == 0


# ---- a sphere ----
def test_sphere_context_agrees_with_the_host_build():
    cfg = configs.sphere_aqua(nx=46, ny=31, n_steps=3)
    m = _ready(cfg)
    b = m.backend
    phys, ms = _structs(m)
    b.flux_init((3, 2), K.FLUX_FIELDS, *SCALES, 1)
    b.run_steps(cfg.Δt, 3)
    f, p, t = _snapshot(b)
    S = b.get_state()
    u0, v0, _, _ = b.get_winds()
    want_f, want_p, st = _reference(phys, ms, S, u0, v0, (3, 2))
    assert_same_bits(f, want_f, "sphere: planes")
    assert_same_bits(p, want_p, "sphere: partials")
    n = np.bincount(st.reshape(-1), minlength=3)
    assert n[1] > 0.2 * st.size and n[0] > 0 and (f[1] > 0).any()          # sea under the wind blob, land and calm elsewhere
    b.close()


# ---- FluxWriter through run() ----
def test_run_with_a_flux_writer_equals_the_hand_written_loop(tmp_path):
    make = lambda: _box(64, 48)      # noqa: E731
    cfg = make()
    n, dt = 10, cfg.Δt
    m = make_model(cfg, "hip")
    sim = Simulation(m, Δt=dt, stop_time=dt * (n - 1))
    sim.output_writers["fluxes"] = FluxWriter(m, schedule=3, path=tmp_path, coarsen=(4, 4), format="npy")
    run(sim)
    assert m.clock.iteration == n
    out = read_flux_output(tmp_path)
    assert out["data"].shape == (n // 3 + 1, 16, 12, 9) and out["var_names"] == list(K.FLUX_FIELDS)
    ref = _ready(make()).backend
    ref.flux_init((4, 4), K.FLUX_FIELDS, *SCALES, 4)
    ref.flux_push()
    for _ in range(n // 3):
        ref.run_steps(dt, 3)
        ref.flux_push()
    ref.run_steps(dt, n % 3)
    for k in range(n // 3 + 1):
        f, p, t = ref.flux_pop()
        assert out["time"][k] == t == 3 * k * dt
        assert_bitwise(out["data"][k], np.moveaxis(f, 0, -1), f"record {k}")
        s = combine_flux_partials(p)
        assert_bitwise(out["scalars"][k], np.array([s[q] for q in SCALAR_NAMES]), f"totals of record {k}")
    assert np.isfinite(out["data"]).all() and (out["data"][..., 0] > 0).all()
    assert_bitwise(np.asarray(m.State), ref.get_state(), "final State of run() and of the loop")
    # and the run itself is the run without the writer
    plain = make_model(make(), "hip")
    run(Simulation(plain, Δt=dt, stop_time=dt * (n - 1)))
    assert_bitwise(np.asarray(m.State), np.asarray(plain.State), "final State with and without the writer")


# ---- the wind rule under a wind stream (picles_wind_stream_*): WindWindow::sample_spare's ring branch ----
def test_wind_rule_streamed_context_samples_at_the_clock_and_names_the_missing_level():
    """each sampled snapshot is held against the planes a window STARTING at that clock holds in (u0, v0): a twin's next step"""
    from test_gpu_wind_stream import _lat, _level, _streamed
    dt, interval = 600.0, 1800.0
    lat = _lat(interval, 8)
    (m, sw), (m2, sw2) = _streamed(lat, dt, 3), _streamed(lat, dt, 3)      # seeded under level 0; the seed invalidates the planes
    b, twin = m.backend, m2.backend
    phys, ms = _structs(m)
    b.flux_init((3, 2), K.FLUX_FIELDS, *SCALES, 2)
    # the clock AT a level (f == 0), directly behind the seed: the level itself, from one slot
    f, p, t = _snapshot(b)
    assert t == 0.0
    S = b.get_state()
    for s in (sw, sw2):
        s.push(1, *_level(lat, 1))
    twin.time_step(dt, K.STEP_ZERO_FIRST)                 # its window starts at 0: (u0, v0) = the stream at the clock
    tw = twin.get_winds()
    want = _reference(phys, ms, S, tw[0], tw[1], (3, 2))
    assert_same_bits(f, want[0], "stream: sampled at level 0"); assert_same_bits(p, want[1], "stream: partials at level 0")
    # a step: the clock at the window's end, the planes the step left
    b.time_step(dt, K.STEP_ZERO_FIRST)
    f, _, t = _snapshot(b)
    w, S = b.get_winds(), b.get_state()
    assert t == dt
    assert_same_bits(f, _reference(phys, ms, S, w[2], w[3], (3, 2))[0], "stream: the level the step ended on")
    # the clock BETWEEN levels (900 s: f = 1/2 between levels 0 and 1): two slots, sampled at the clock
    twin.get_state()                                      # (completes the twin's pending step: its successor starts elsewhere)
    b.tick(0.5 * dt); twin.tick(0.5 * dt)
    f, p, t = _snapshot(b)
    assert t == 1.5 * dt
    twin.time_step(dt, K.STEP_ZERO_FIRST)
    tw = twin.get_winds()
    assert not np.array_equal(tw[0], w[2]) and not np.array_equal(tw[0], w[0])
    want = _reference(phys, ms, S, tw[0], tw[1], (3, 2))
    assert_same_bits(f, want[0], "stream: sampled between levels"); assert_same_bits(p, want[1], "stream: partials between levels")
    # a level that is not held: refused, naming the level to push, before anything is launched
    import torch
    b.tick(interval)                                      # 2700 s: between levels 1 and 2; 2 was never pushed
    with pytest.raises(K.PiclesError, match=r"picles_flux_push.*needs level k = 2 \(t = 3600\).*not held.*levels held: 0 \.\. 1.*picles_wind_stream_push"):
        b.flux_push()
    with pytest.raises(K.PiclesError, match=r"picles_flux_export.*level k = 2"):
        b.flux_export(torch.zeros((9, 17, 11), dtype=torch.float32, device="cuda"))
    sw.push(2, *_level(lat, 2))
    f2, _, t = _snapshot(b)                               # once it is held the same call goes through
    assert t == 1.5 * dt + interval and np.isfinite(f2).all() and not np.array_equal(f2, f)
    # a clock before the stream's first level
    b.tick(-(1.5 * dt + interval) - 300.0)
    with pytest.raises(K.PiclesError, match=r"clock -300 lies before the first time level of the wind stream \(t0 = 0\)"):
        b.flux_push()
    assert b.flux_pending == 0
    b.close(); twin.close()


# ---- FluxExport (picles_amd/coupling.py) and the example built on it ----
def test_flux_export_helper_gives_the_planes_of_push_and_pop():
    import torch
    from picles_amd.coupling import FluxExport
    m, m2 = _ready(_box(48, 24)), _ready(_box(48, 24))
    names = ("tq_in_x", "tq_in_y", "phi_dis", "us_x")
    fx = FluxExport(m, coarsen=(4, 3), fields=names, rho_water=1000.0)
    assert fx.fields == ("phi_dis", "tq_in_x", "tq_in_y", "us_x") and tuple(fx.planes.shape) == (4, 8, 12) and fx.planes.is_cuda
    m2.backend.flux_init((4, 3), names, 1000.0 * G0, 1000.0, 1)
    for k in (0, 3, 2):                                   # the seeded sea, then twice behind fused steps that are still pending
        for x in (m, m2):
            if k:
                x.backend.run_steps(600.0, k)
        planes = fx()
        torch.cuda.current_stream().synchronize()
        f, p, t = _snapshot(m2.backend)
        assert set(planes) == set(fx.fields) and t == m.backend.clock
        for q, name in enumerate(fx.fields):
            assert planes[name].dtype == torch.float32 and tuple(planes[name].shape) == (8, 12)
            assert_same_bits(planes[name].cpu().numpy().T, f[q], f"FluxExport after {k} steps: {name}")
        assert_same_bits(fx.partials.cpu().numpy(), p, f"FluxExport after {k} steps: partials")
    assert_bitwise(m.backend.get_state(), m2.backend.get_state(), "State under FluxExport and under push + pop")
    with pytest.raises(ValueError, match="rho_water"):
        FluxExport(m2, rho_water=-1.0)
    m.backend.close(); m2.backend.close()


def test_coupled_fluxes_example_runs():
    """examples/coupled_fluxes_torch.py on a small box: streamed winds in, FluxExport out, its first export directly behind the seed"""
    import os
    import re
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "examples" / "coupled_fluxes_torch.py"), "3"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, COUPLED_N="96"))
    assert r.returncode == 0, r.stderr[-2000:]
    mo = re.search(r"wave-supported stress ([\d.]+) N m-2, stress to the ocean ([\d.]+) N m-2.* (\d+) active and (\d+) bad nodes", r.stdout)
    assert mo, r.stdout
    assert 0.0 < float(mo.group(1)) < 5.0 and 0.0 < float(mo.group(2)) < 5.0          # N m-2: the order of a wind stress
    assert int(mo.group(3)) > 0.8 * 96 * 96 and int(mo.group(4)) == 0
