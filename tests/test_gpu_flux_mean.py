"""Flux means on the device (picles_flux_mean_*, k_flux_mean_update / k_flux_mean_final): the fp64 accumulators BIT FOR BIT against
the per-step host route through the existing public API — a second model of the same configuration takes the steps one time_step at
a time; after each step get_state() and get_winds() give State and the end level, the host build of flux_node
(tests/native/flux_host.cpp) the node values, _flux_numpy.cell_sums the cell sums S, and NumPy does acc = acc + S.  Finalisation and
the tile tree are restated in tests/_flux_mean_numpy.py.

Which shape reaches which instance of k_flux_mean_update<FROM_REC, CX>:
    70 x 37 (4, 3)    groups of four; ragged last cell in x (two columns) and in y
    520 x 9 (2, 1)    three workgroups per row, the last with eight live lanes
    64 x 16 (1, 1)    every lane its own leader
    96 x 24 (16, 16)  four groups per wave, ragged in y
    45 x 28 (2, 3)    odd Nx, the last cell one column wide
    66 x 20 (3, 5)    the generic instance
    67 x 22 (3, 5)    the generic instance with a ragged last cell in x (one column) and in y (two rows): lanes of a wave leave the
                      node loop at different times while the pull ballots"""
import numpy as np
import pytest

import _flux_mean_numpy as FM
import _flux_numpy as F
import _hostile_states as H
from helpers import assert_bitwise, assert_same_bits, make_model
from picles_amd import _capi as K, configs
from picles_amd.driver import combine_flux_partials
from picles_amd.simulations import Simulation, initialize_simulation
from test_gpu_flux import SCALES, _bare, _box, _hostile_winds, _levels, _ready, _structs

pytestmark = pytest.mark.gpu

SHAPES = {"70x37_4x3": (70, 37, 4, 3), "520x9_2x1": (520, 9, 2, 1), "64x16_1x1": (64, 16, 1, 1), "96x24_16x16": (96, 24, 16, 16),
          "45x28_2x3": (45, 28, 2, 3), "66x20_3x5": (66, 20, 3, 5), "67x22_3x5": (67, 22, 3, 5)}
DT = 600.0


def _sums(phys, ms, S, u, v, pair):
    with np.errstate(all="ignore"):
        vals, st = F.host_nodes(phys, ms, S[..., 0], S[..., 1], S[..., 2], u, v)
        return F.cell_sums(vals, st, *pair)[0]


def _host_route(b, phys, ms, dt, n_steps, pair, due, level, before_step=None):
    """the checker: b takes n_steps single steps; behind every step s in `due`, acc = acc + S from State and the wind level
    (level 0: a static window's only level; 1: the end level)"""
    acc = None
    for s in range(1, n_steps + 1):
        if before_step:
            before_step(b, s)
        b.time_step(dt, K.STEP_ZERO_FIRST)
        if s in due:
            w = b.get_winds()
            S = _sums(phys, ms, b.get_state(), w[2 * level], w[2 * level + 1], pair)
            acc = S if acc is None else acc + S
    return acc


# ---- 1. the accumulators after run_steps(dt, 6) in one call, the sixth step still pending ----
@pytest.mark.parametrize("case", list(SHAPES))
def test_accumulators_bitwise_after_six_fused_steps(case):
    nx, ny, cx, cy = SHAPES[case]
    m, twin = _ready(_box(nx, ny)), _ready(_box(nx, ny))
    b = m.backend
    phys, ms = _structs(m)
    b.flux_init((cx, cy), K.FLUX_FIELDS, *SCALES, 2)
    b.flux_mean_init(every=1, first=1)
    nxc, nyc = F.coarse_shape(nx, ny, cx, cy)
    assert b.flux_mean_shape() == (1, 11, 88 * nxc * nyc)
    assert_same_bits(b.flux_mean_get()["acc"], np.zeros((11, nxc, nyc)), f"{case}: all zero at init")
    b.run_steps(DT, 6)
    got = b.flux_mean_get()
    assert (got["n_samples"], got["t_first"], got["t_last"]) == (6, DT, 6 * DT)
    want = _host_route(twin.backend, phys, ms, DT, 6, (cx, cy), range(1, 7), 0)
    assert got["acc"].shape == want.shape == (11, nxc, nyc)
    assert_same_bits(got["acc"], want, f"{case}: accumulators")
    # the smooth box leaves every node active in every sample
    assert got["acc"][9].sum() == 6 * nx * ny and got["acc"][10].sum() == 0
    assert (got["acc"][:2] > 0).all()
    assert_bitwise(b.get_state(), twin.backend.get_state(), f"{case}: State of the run with the set and of the per-step twin")
    b.close(); twin.backend.close()


# ---- 2. a wind that differs at every step end ----
def test_lattice_winds_through_chunked_run_steps():
    make = lambda: configs.growing_decaying_winds_lattice(n=48, n_steps=8)      # noqa: E731
    m, twin = _ready(make()), _ready(make())
    b, dt = m.backend, make().Δt
    phys, ms = _structs(m)
    b.flux_init((4, 3), K.FLUX_FIELDS, *SCALES, 2)
    b.flux_mean_init()
    for c in (1, 3, 2):
        b.run_steps(dt, c)
    got = b.flux_mean_get()
    seen = []
    want = _host_route(twin.backend, phys, ms, dt, 6, (4, 3), range(1, 7), 1, before_step=lambda x, s: seen.append(x.get_winds()[2].copy()) if s > 1 else None)
    assert not np.array_equal(seen[0], seen[-1])                                # the end level does change from step to step
    assert got["n_samples"] == 6 and got["t_last"] == 6 * dt
    assert_same_bits(got["acc"], want, "lattice: accumulators")
    b.close(); twin.backend.close()


def test_host_set_levels_through_the_per_step_loop():
    nx, ny = 48, 24
    u0, v0, u1, v1 = _levels(nx, ny)
    def window(b, s):      # the window of step s: its levels swing between the two pairs, scaled by the step number
        a, c = (u0, v0) if s % 2 else (u1, v1), (u1, v1) if s % 2 else (u0, v0)
        f0, f1 = 1.0 + 0.05 * (s - 1), 1.0 + 0.05 * s
        b.set_winds(f0 * a[0], f0 * a[1], (s - 1) * DT, f1 * c[0], f1 * c[1], s * DT)
    m, twin = _ready(_box(nx, ny, winds=None)), _ready(_box(nx, ny, winds=None))
    b = m.backend
    phys, ms = _structs(m)
    b.flux_init((2, 4), K.FLUX_FIELDS, *SCALES, 2)
    b.flux_mean_init()
    for s in range(1, 6):
        window(b, s)
        b.time_step(DT, K.STEP_ZERO_FIRST)
    got = b.flux_mean_get()
    want = _host_route(twin.backend, phys, ms, DT, 5, (2, 4), range(1, 6), 1, before_step=window)
    assert got["n_samples"] == 5
    assert_same_bits(got["acc"], want, "host-set levels: accumulators")
    # a clock inside the window: the wind rule refuses a manual update before anything is launched, and nothing is counted
    b.tick(-0.25 * DT)
    with pytest.raises(K.PiclesError, match=r"picles_flux_mean_update.*holds no level at the clock.*step to a level"):
        b.flux_mean_update()
    b.tick(0.25 * DT)
    again = b.flux_mean_get()
    assert again["n_samples"] == 5
    assert_same_bits(again["acc"], want, "accumulators after the refusal")
    b.close(); twin.backend.close()


# ---- 3. developed sea, land and an open edge: scatter reach >= 2 in the pending step ----
def test_large_reach_land_block_and_open_edge():
    from test_gpu_more import _masked_cfg
    def ready():
        cfg = _masked_cfg()
        m = make_model(cfg, "hip")
        initialize_simulation(Simulation(m, Δt=1200.0, stop_time=1.0))
        m.upload_winds(0.0, 1200.0)
        return m
    m, twin = ready(), ready()
    b = m.backend
    phys, ms = _structs(m)
    b.flux_init((4, 2), K.FLUX_FIELDS, *SCALES, 2)
    b.flux_mean_init(every=1, first=9)                   # the samples of the developed sea: steps 9 ... 12
    b.enable_timing(True)
    b.run_steps(1200.0, 12)
    got = b.flux_mean_get()
    t = b.get_timing()
    assert t["advance_launches"] == 12 and t["scatter_launches"] <= 1, t      # the twelfth step was pending under the last update
    assert b.get_counters()["max_reach"] >= 2
    want = _host_route(twin.backend, phys, ms, 1200.0, 12, (4, 2), range(9, 13), 0)
    assert got["n_samples"] == 4 and got["t_first"] == 9 * 1200.0
    assert_same_bits(got["acc"], want, "large reach, land, open edge: accumulators")
    assert 0 < got["acc"][9].sum() < 4 * 32 * 32         # land and rim nodes are not active
    b.close(); twin.backend.close()


# ---- 4. hostile planes, nothing pending: the FROM_REC = false instances ----
@pytest.mark.parametrize("case", ["70x37_4x3", "45x28_2x3", "66x20_3x5", "67x22_3x5", "96x24_16x16"])
def test_hostile_planes_two_manual_updates(case):
    nx, ny, cx, cy = SHAPES[case]
    b, phys, ms = _bare(nx, ny)
    S = H.hostile_state(nx, ny, cx, cy, seed=801 if case == "96x24_16x16" else 700 + len(case) + nx)
    u, v = _hostile_winds(nx, ny, seed=nx + ny)
    b.set_winds(u, v, 0.0)
    b.set_state(S)
    b.flux_init((cx, cy), K.FLUX_FIELDS, *SCALES, 2)
    b.flux_mean_init()
    b.flux_mean_update()
    b.flux_mean_update()
    got = b.flux_mean_get()
    one = _sums(phys, ms, S, u, v, (cx, cy))
    assert got["n_samples"] == 2 and got["t_first"] == got["t_last"] == 0.0
    assert_same_bits(got["acc"], one + one, f"{case}: S + S")
    assert got["acc"][10].sum() > 0 and got["acc"][9].sum() > 0 and not np.isnan(got["acc"]).any()
    assert_same_bits(b.get_state(), S, f"{case}: State as set", nan_payload=True)
    b.close()


# ---- 5. push + pop and export into torch tensors ----
def test_push_pop_and_export_against_the_numpy_finalisation():
    import torch
    nx, ny, cx, cy = 70, 37, 4, 3
    b = _ready(_box(nx, ny)).backend
    b.flux_init((cx, cy), K.FLUX_FIELDS, *SCALES, 2)
    b.flux_mean_init()
    with pytest.raises(K.PiclesError, match="holds no sample"):
        b.flux_mean_push()
    b.run_steps(DT, 4)
    got = b.flux_mean_get()
    ncov = FM.cover(nx, ny, cx, cy)
    nxc, nyc = ncov.shape
    want_f, want_p = FM.finalise(got["acc"], ncov, 4, *SCALES), FM.tile_tree(got["acc"])
    b.flux_mean_push(reset=False)
    assert b.flux_pending == 1
    f, p, t = b.flux_pop()
    assert t == b.clock == 4 * DT
    assert_same_bits(f, want_f, "planes of push + pop"); assert_same_bits(p, want_p, "partials of push + pop")
    assert np.isfinite(f).all() and (f[:2] > 0).all()
    tot = combine_flux_partials(p)
    assert [tot[k] / 4 for k in tot] == FM.totals([want_p], 4) and tot["n_active"] == 4 * nx * ny
    # the ring refuses when full and works again after a pop
    b.flux_mean_push(reset=False); b.flux_mean_push(reset=False)
    with pytest.raises(K.PiclesError, match="ring full"):
        b.flux_mean_push(reset=False)
    f2, p2, _ = b.flux_pop()
    b.flux_mean_push(reset=False)
    for _ in range(2):
        f3, p3, _ = b.flux_pop()
        assert_same_bits(f3, f, "a later slot: planes"); assert_same_bits(p3, p, "a later slot: partials")
    assert_same_bits(f2, f, "second slot")
    # export into torch tensors, with and without a partials buffer
    tf = torch.full((9, nyc, nxc), -1.0, dtype=torch.float32, device="cuda")
    tp = torch.full((p.shape[0], 11), -1.0, dtype=torch.float64, device="cuda")
    b.flux_mean_export(tf, tp, reset=False)
    torch.cuda.current_stream().synchronize()
    assert_same_bits(tf.cpu().numpy().transpose(0, 2, 1), f, "exported planes"); assert_same_bits(tp.cpu().numpy(), p, "exported partials")
    tf.fill_(-1.0)
    b.flux_mean_export(tf, reset=True)
    torch.cuda.current_stream().synchronize()
    assert_same_bits(tf.cpu().numpy().transpose(0, 2, 1), f, "exported planes, no partials")
    # reset = 1 leaves zeros and no sample
    z = b.flux_mean_get()
    assert (z["n_samples"], z["t_first"], z["t_last"]) == (0, 0.0, 0.0)
    assert_same_bits(z["acc"], np.zeros_like(got["acc"]), "accumulators after reset")
    with pytest.raises(K.PiclesError, match="holds no sample"):
        b.flux_mean_export(tf)
    # a subset mask and unit scales, on the same accumulators (the flux set goes, and the mean set with it)
    names = ("us_y", "phi_dis", "tq_in_x", "phi_shift")
    b.flux_free()
    with pytest.raises(K.PiclesError):
        b.flux_mean_shape()
    with pytest.raises(K.PiclesError, match="picles_flux_init first"):
        b.flux_mean_init()
    b.flux_init((cx, cy), names, 1.0, 1.0, 1)
    b.flux_mean_init()
    b.flux_mean_set(got)
    b.flux_mean_push(reset=True)
    f4, p4, _ = b.flux_pop()
    assert_same_bits(f4, FM.finalise(got["acc"], ncov, 4, names=names), "subset mask, unit scales")
    assert_same_bits(p4, p, "subset mask: partials")
    assert b.flux_mean_get()["n_samples"] == 0
    b.close()


# ---- 6. cadence, round trip, refusals ----
def test_cadence_and_get_free_init_set_round_trip():
    nx, ny, pair = 48, 24, (4, 4)
    m, twin, twin2 = _ready(_box(nx, ny)), _ready(_box(nx, ny)), _ready(_box(nx, ny))
    b = m.backend
    phys, ms = _structs(m)
    with pytest.raises(K.PiclesError, match="picles_flux_init first"):
        b.flux_mean_init()
    with pytest.raises(K.PiclesError, match="picles_flux_mean_init first"):
        b.flux_mean_update()
    b.flux_init(pair, K.FLUX_FIELDS, *SCALES, 2)
    for ev, fi in ((0, 1), (1, 0), (-3, 2)):
        with pytest.raises(K.PiclesError, match="every and first"):
            b.flux_mean_init(ev, fi)
    b.flux_mean_init(every=3, first=2)
    with pytest.raises(K.PiclesError, match="a mean set exists"):
        b.flux_mean_init()
    b.run_steps(DT, 5)
    b.time_step(DT, K.STEP_ZERO_FIRST)
    b.run_steps(DT, 2)
    got = b.flux_mean_get()
    want = _host_route(twin.backend, phys, ms, DT, 8, pair, (2, 5, 8), 0)
    assert (got["n_samples"], got["t_first"], got["t_last"]) == (3, 2 * DT, 8 * DT)
    assert_same_bits(got["acc"], want, "every 3 from step 2 over eight steps")
    # get -> free -> init -> set -> more steps: the uninterrupted accumulators (every = 1 from here: steps 9 ... 11)
    b.flux_mean_free()
    b.flux_mean_free()                                   # without a set: nothing to drop
    b.flux_mean_init()
    b.flux_mean_set(got)
    b.run_steps(DT, 3)
    more = b.flux_mean_get()
    want2 = _host_route(twin2.backend, phys, ms, DT, 11, pair, (2, 5, 8, 9, 10, 11), 0)
    assert (more["n_samples"], more["t_first"], more["t_last"]) == (6, 2 * DT, 11 * DT)
    assert_same_bits(more["acc"], want2, "continued after free, init, set")
    # reset: zero, the step count goes on
    b.flux_mean_reset()
    assert b.flux_mean_get()["n_samples"] == 0 and not b.flux_mean_get()["acc"].any()
    for x in (m, twin, twin2):
        x.backend.close()


# ---- 7. no side effect; the last step stays pending ----
def test_a_run_with_the_set_is_the_run_without_it():
    def go(with_set):
        b = _ready(_box(48, 24)).backend
        b.enable_timing(True)
        if with_set:
            b.flux_init((4, 4), K.FLUX_FIELDS, *SCALES, 3)
            b.flux_mean_init()
        for k in (2, 3, 1):
            b.run_steps(DT, k)
        if with_set:
            b.flux_mean_get()
            b.flux_mean_push(reset=True)
        t = b.get_timing()                               # (flushes the last step: at most one stand-alone scatter + remesh)
        assert t["advance_launches"] == 6 and t["scatter_launches"] <= 1, t
        b.checkpoint_begin()
        blob = b.checkpoint_end()
        b.time_step(DT, K.STEP_ZERO_FIRST)
        if with_set:
            b.flux_pop()
        z, on, bnd, st = b.get_particles()
        return b.get_state(), np.where(on[..., None] != 0, z, 0.0), on, bnd, st, blob, b.get_counters(), b.clock
    A, B = go(True), go(False)
    for x, y, what in zip(A[:6], B[:6], ("State", "particles", "on", "boundary", "status", "restart blob")):
        assert_bitwise(x, y, what)
    assert A[6] == B[6] and A[7] == B[7]


# ---- 11. something physical ----
def test_interval_mean_against_the_average_of_six_snapshots():
    """At (1, 1) with unit scales every snapshot plane is the correctly rounded float32 of the node's value x_k (relative error at
    most u = 2^-24), so the fp64 average of six snapshots differs from accumulator / 6 by rounding only.  At EVERY node of ALL nine
    planes, whatever the signs: |mean(fl(x_k)) - mean(x_k)| <= u mean(|x_k|) <= u (1 + u) mean(|fl(x_k)|); the fp64 operations add
    some 1e-16 relative to the same norm.  Asserted: |difference| <= 2 u mean_k(|snapshot_k|), node by node, plane by plane; the
    largest ratio is printed per plane (in units of u).  Measured on an MI355X: see DESIGN.md §28."""
    nx, ny = 64, 16
    m, m2 = _ready(_box(nx, ny)), _ready(_box(nx, ny))
    b, s = m.backend, m2.backend
    for x in (b, s):
        x.flux_init((1, 1), K.FLUX_FIELDS, 1.0, 1.0, 2)
    b.flux_mean_init()
    b.run_steps(DT, 6)
    acc = b.flux_mean_get()["acc"]
    snaps = []
    for _ in range(6):
        s.time_step(DT, K.STEP_ZERO_FIRST)
        s.flux_push()
        snaps.append(s.flux_pop()[0].astype(np.float64))
    u = 2.0 ** -24
    avg, mean, norm = sum(snaps) / 6.0, acc[:9] / 6.0, sum(np.abs(x) for x in snaps) / 6.0
    assert (norm[[0, 1, 3, 4, 5, 6, 7, 8]] > 0).all()     # every node carries a flux in the planes no switch turns off
    diff = np.abs(avg - mean)
    ratio = [float(np.max(np.where(norm[k] > 0, diff[k] / np.where(norm[k] > 0, norm[k], 1.0), 0.0))) / u for k in range(9)]
    print("snapshot average against accumulator / 6, largest |difference| / mean|snapshot| per plane, in u (float32): "
          + ", ".join(f"{f} {r:.3f}" for f, r in zip(K.FLUX_FIELDS, ratio)))
    assert (diff <= 2.0 * u * norm).all(), ratio
    assert max(ratio) > 0.01                              # the two routes do differ: the snapshots were rounded
    b.close(); s.close()


# ---- 8. slabs in one process ----
@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_whole_grid_accumulators_and_totals(world):
    from picles_amd.driver import flux_mean_concat
    from picles_amd.parallel import SlabModel, slab_rows
    from test_gpu_slab_fuzz import _NoExchange, _step_all
    make = lambda: _box(64, 48)      # noqa: E731
    cfg, pair = make(), (2, 4)
    assert all(slab_rows(48, world, r)[0] % pair[1] == 0 for r in range(world))
    one = SlabModel(cfg.model, 0, 1, device=0)
    one.flux_init(pair, K.FLUX_FIELDS, *SCALES, 2)
    one.flux_mean_init(every=2, first=1)
    one.seed()
    for _ in range(5):
        one.time_step(cfg.Δt)
    want = one.gather_flux_means()
    assert want["n_samples"] == 3 and want["acc"].shape == (11, 32, 12) and want["totals"]["n_active"] == 64 * 48
    slabs = [SlabModel(make().model, r, world, device=0, halo_rows=2, exchange=_NoExchange()) for r in range(world)]
    for s in slabs:
        s._comm_warm = True
        s.flux_init(pair, K.FLUX_FIELDS, *SCALES, 2)
        s.flux_mean_init(every=2, first=1)
        s.seed()
    for _ in range(5):
        _step_all(slabs, cfg.Δt, slabs[0].periodic_y, fused_ok=True)
        for s in slabs:
            s._flux_mean_after_steps(1, split_phase=True)             # what SlabModel.time_step does behind its halo exchange
    got = flux_mean_concat([s.flux_mean_get() for s in slabs])
    assert sum(s.backend.get_counters()["halo_overflow"] for s in slabs) == 0
    assert (got["n_samples"], got["t_first"], got["t_last"]) == (want["n_samples"], want["t_first"], want["t_last"])
    assert_same_bits(got["acc"], want["acc"], f"{world} slabs: accumulators, row block after row block")
    for k in want["totals"]:
        assert_same_bits(np.array([got["totals"][k]]), np.array([want["totals"][k]]), f"{world} slabs: total {k}")
    # the host's tile tree is the finalising kernel's: the partials of a push, combined, are the totals times n
    one.backend.flux_mean_push(reset=False)
    _, p, _ = one.backend.flux_pop()
    tot = combine_flux_partials(p)
    assert all(tot[k] / 3 == want["totals"][k] for k in tot)


# ---- 10. FluxMeanExport (picles_amd/coupling.py) and the example built on it ----
def test_flux_mean_export_helper_against_push_and_pop():
    import torch
    from picles_amd.coupling import FluxMeanExport
    from picles_amd.flux_output import G0
    m, m2 = _ready(_box(48, 24)), _ready(_box(48, 24))
    names = ("tq_in_x", "tq_in_y", "phi_dis", "us_x")
    fx = FluxMeanExport(m, coarsen=(4, 3), fields=names, rho_water=1000.0)
    assert fx.fields == ("phi_dis", "tq_in_x", "tq_in_y", "us_x") and tuple(fx.planes.shape) == (4, 8, 12) and fx.n_samples == 0
    m2.backend.flux_init((4, 3), names, 1000.0 * G0, 1000.0, 1)
    m2.backend.flux_mean_init()
    with pytest.raises(K.PiclesError, match="holds no sample"):
        fx()
    t = 0.0
    for k in (3, 2):                                      # two intervals, each behind fused steps that are still pending
        for x in (m, m2):
            x.backend.run_steps(DT, k)
        assert (fx.n_samples, fx.t_first, fx.t_last) == (k, t + DT, t + k * DT)
        planes = fx()
        torch.cuda.current_stream().synchronize()
        assert fx.exported == dict(n_samples=k, t_first=t + DT, t_last=t + k * DT) and fx.n_samples == 0
        t += k * DT
        m2.backend.flux_mean_push(reset=True)
        f, p, tp = m2.backend.flux_pop()
        assert tp == t
        for q, name in enumerate(fx.fields):
            assert_same_bits(planes[name].cpu().numpy().T, f[q], f"FluxMeanExport over {k} steps: {name}")
        assert_same_bits(fx.partials.cpu().numpy(), p, f"FluxMeanExport over {k} steps: partials")
    assert_bitwise(m.backend.get_state(), m2.backend.get_state(), "State under FluxMeanExport and under push + pop")
    m.backend.close(); m2.backend.close()


def test_coupled_flux_means_example_runs():
    """examples/coupled_flux_means_torch.py on a small box: streamed winds in, six steps per interval, interval means out"""
    import os
    import re
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    r = subprocess.run([sys.executable, str(root / "examples" / "coupled_flux_means_torch.py"), "2"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, COUPLED_N="96"))
    assert r.returncode == 0, r.stderr[-2000:]
    mo = re.search(r"wave-supported stress ([\d.]+) N m-2, stress to the ocean ([\d.]+) N m-2.* (\d+) active and (\d+) bad nodes", r.stdout)
    assert mo, r.stdout
    assert 0.0 < float(mo.group(1)) < 5.0 and 0.0 < float(mo.group(2)) < 5.0          # N m-2: the order of a wind stress
    assert int(mo.group(3)) > 0.8 * 96 * 96 and int(mo.group(4)) == 0


# ---- 9. MeanFluxWriter through run() ----
def test_run_with_a_mean_flux_writer_and_a_picked_up_run(tmp_path):
    from picles_amd.checkpointing import Checkpointer
    from picles_amd.flux_output import SCALAR_NAMES, FluxWriter, MeanFluxWriter, read_flux_output
    from picles_amd.simulations import run
    make = lambda: _box(64, 48)      # noqa: E731
    dt = make().Δt
    def sim_of(d, stop_it, ck=None):
        m = make_model(make(), "hip")
        sim = Simulation(m, Δt=dt, stop_time=dt * (stop_it - 1))
        sim.output_writers["flux_means"] = MeanFluxWriter(m, schedule=3, path=tmp_path / d, coarsen=(4, 4), format="npy")
        if ck:
            sim.output_writers["checkpointer"] = Checkpointer(m, schedule=4, dir=tmp_path / ck / "ck")
        return m, sim
    m, sim = sim_of("whole", 9)
    run(sim)
    assert m.clock.iteration == 9
    out = read_flux_output(tmp_path / "whole", name="flux_means")
    assert out["data"].shape == (3, 16, 12, 9) and out["averaged"] is True and out["samples_per_record"] == 3
    # a hand-written loop over the backend calls
    ref = _ready(make()).backend
    ref.flux_init((4, 4), K.FLUX_FIELDS, *SCALES, 4)
    ref.flux_mean_init()
    for k in range(3):
        ref.run_steps(dt, 3)
        ref.flux_mean_push(reset=True)
    for k in range(3):
        f, p, t = ref.flux_pop()
        assert out["time"][k] == t == 3 * (k + 1) * dt
        assert_bitwise(out["data"][k], np.moveaxis(f, 0, -1), f"record {k}")
        s = combine_flux_partials(p)
        assert_bitwise(out["scalars"][k], np.array([s[q] / 3 for q in SCALAR_NAMES]), f"interval-mean totals of record {k}")
    assert np.isfinite(out["data"]).all() and (out["data"][..., 0] > 0).all()
    assert_bitwise(np.asarray(m.State), ref.get_state(), "final State of run() and of the loop")
    # stopped by a Checkpointer at iteration 4 and picked up in a fresh model: the records of the uninterrupted run
    m1, sim1 = sim_of("part1", 4, ck="part1")
    run(sim1)
    first = read_flux_output(tmp_path / "part1", name="flux_means")
    assert first["data"].shape[0] == 1                    # iteration 3; the sample of step 4 went into the side-car
    assert len(list((tmp_path / "part1" / "ck").glob("*.fluxmeans.npz"))) == 1
    m2, sim2 = sim_of("part2", 9, ck="part1")
    run(sim2, pickup=True)
    assert m2.clock.iteration == 9
    second = read_flux_output(tmp_path / "part2", name="flux_means")
    assert second["time"] == out["time"][1:]
    assert_bitwise(np.concatenate([first["data"], second["data"]]), out["data"], "stopped + picked up vs uninterrupted: planes")
    assert_bitwise(np.concatenate([first["scalars"], second["scalars"]]), out["scalars"], "stopped + picked up vs uninterrupted: totals")
    # a FluxWriter next to it is refused before anything is seeded
    m3, sim3 = sim_of("pair", 9)
    sim3.output_writers["fluxes"] = FluxWriter(m3, schedule=3, path=tmp_path / "pair", format="npy")
    with pytest.raises(ValueError, match="share the one flux ring.*pop each other's records"):
        run(sim3)
    assert m3.clock.iteration == 0 and not (tmp_path / "pair").exists()
