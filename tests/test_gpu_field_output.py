"""Coarse wave diagnostics on the device (picles_diag_*, k_diag): fields, tile partials and global scalars BITWISE against the
NumPy restatement of the definition (tests/_diag_numpy.py) applied to get_state() of the same context; ring semantics; no side
effect on the model; refusals; slabs; FieldWriter through run()."""
import numpy as np
import pytest

import _diag_numpy as D
from helpers import assert_bitwise, assert_same_bits, make_model
from picles_amd import _capi as K, configs, fetch_relations
from picles_amd.checkpointing import Checkpointer
from picles_amd.driver import HipModel, SCALAR_NAMES, combine_partials
from picles_amd.field_output import FieldWriter, read_field_output
from picles_amd.models import build_structs
from picles_amd.parallel import SlabModel, slab_rows
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.timesteppers import time_step

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (2, 2), (4, 4), (3, 5), (16, 16)]
CASES = {
    "bench06_48": (lambda: configs.bench06_box(n=48), 4, PAIRS, (0.9, 1.0)),
    "example_00_33": (lambda: configs.example_00_minimal(n=33, L=64e3), 3, PAIRS, (0.9, 1.0)),
    "T04_32": (lambda: configs.T04_2D_reg_test(n=32), 6, PAIRS, (0.9, 1.0)),
    "sphere_92x60": (lambda: configs.sphere_aqua(nx=92, ny=60), 4, PAIRS, (0.2, 0.5)),
    "bench06_1100": (lambda: configs.bench06_box(n=1100), 2, [(1, 1), (4, 4)], (0.9, 1.0)),      # 275 coarse columns at cx = 4: a full tile and 19
}


def _phys(cfg):
    P = cfg.model["ODEsets"].Parameters
    return P.get("g", 9.81), P["r_g"]


def _ready(cfg):
    """a seeded model whose backend can be driven directly (winds uploaded for run_steps)"""
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    m.upload_winds(0.0, cfg.Δt)
    return m


def _same_scalars(got, want, what):
    """the scalars by bit pattern (a zero's sign counts; two NaNs are the same)"""
    for k in want:
        assert_same_bits(np.array([got[k]], dtype=np.float64), np.array([want[k]], dtype=np.float64), f"{what}: scalar {k}")


def _check_snapshot(b, cfg, pair, names, f, p, what):
    """fields and partials of one pop against the restatement of the State the same context holds"""
    S = b.get_state()
    g, r_g = _phys(cfg)
    want_f, valid = D.fields_of(S, pair[0], pair[1], g, r_g, names=names)
    want_p = D.partials_of(S, pair[0], pair[1])
    assert f.dtype == np.float32 and f.shape == want_f.shape, (what, f.shape, want_f.shape)
    assert_same_bits(f, want_f, f"{what}: fields")
    assert_same_bits(p, want_p, f"{what}: partials")
    got, want = combine_partials(p, b.Nx, b.Ny), D.combine([want_p], b.Nx, b.Ny)
    _same_scalars(got, want, what)
    with np.errstate(all="ignore"):
        _same_scalars({"max_e": got["max_e"], "max_my": got["max_my"]},
                      {"max_e": np.fmax.reduce(S[..., 0], axis=None) + 0.0, "max_my": np.fmax.reduce(S[..., 2], axis=None) + 0.0}, what)
    return float(valid.mean())


@pytest.mark.parametrize("case", list(CASES))
def test_fields_partials_and_scalars_bitwise(case):
    make, n_steps, pairs, (lo, hi) = CASES[case]
    cfg = make()
    m = _ready(cfg)
    for _ in range(n_steps):
        time_step(m, cfg.Δt, zero_first=True)
    S = m.backend.get_state()
    for pair in pairs:
        # a context of its own per factor pair (a ring is set up once per context), holding the same State
        b = make_model(make(), "hip").backend
        b.set_state(S)
        names = K.DIAG_FIELDS if pair != (2, 2) else ("hs", "tp", "cg_x", "cg_y")
        b.diag_init(pair, names, 2)
        nxc, nyc, nf, npart, nbytes = b.diag_shape()
        assert (nxc, nyc) == D.coarse_shape(b.Nx, b.Ny, *pair) and nf == len(names)
        assert npart == nyc * -(-nxc // 256) and nbytes == 4 * nxc * nyc * nf
        b.diag_push()
        assert b.diag_pending == 1
        f, p, t = b.diag_pop()
        assert b.diag_pending == 0 and t == b.clock
        share = _check_snapshot(b, cfg, pair, names, f, p, f"{case} {pair}")
        print(f"{case} {pair}: share of valid coarse cells {share:.3f}")
        assert lo <= share <= hi, (case, pair, share)
        assert np.isfinite(f[:, np.isfinite(f[0])]).all()          # a valid cell is valid in every plane
        b.close()


def test_ring_pops_in_order_while_steps_are_enqueued():
    cfg = configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * 48, 2000.0 * 48))
    dt = cfg.Δt
    a, twin = _ready(cfg).backend, _ready(configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * 48, 2000.0 * 48))).backend
    a.diag_init((2, 3), K.DIAG_FIELDS, 3)
    chunks, want = [2, 3, 1], []
    for k in chunks:
        a.run_steps(dt, k)
        a.diag_push()
        twin.run_steps(dt, k)
        want.append((twin.get_state(), twin.clock))
    a.run_steps(dt, 2)                     # more steps enqueued behind the last push, before anything is popped
    assert a.diag_pending == 3
    g, r_g = _phys(cfg)
    for k, (S, t) in enumerate(want):
        f, p, tt = a.diag_pop()
        assert tt == t == sum(chunks[:k + 1]) * dt
        assert_same_bits(f, D.fields_of(S, 2, 3, g, r_g)[0], f"snapshot {k}: fields")
        assert_same_bits(p, D.partials_of(S, 2, 3), f"snapshot {k}: partials")
    assert a.diag_pending == 0
    twin.run_steps(dt, 2)
    assert_bitwise(a.get_state(), twin.get_state(), "State after the ring run")


def test_pushes_leave_the_model_untouched():
    def go(with_diag):
        b = _ready(configs.example_00_minimal(n=33, L=64e3)).backend
        if with_diag:
            b.diag_init((4, 4), ("hs", "tp", "cg_x", "cg_y"), 3)
        for k in (2, 3, 1):
            b.run_steps(600.0, k)
            if with_diag:
                b.diag_push()
        b.time_step(600.0, K.STEP_ZERO_FIRST)
        if with_diag:
            while b.diag_pending:
                b.diag_pop()
        z, on, bnd, st = b.get_particles()
        return b.get_state(), np.where(on[..., None] != 0, z, 0.0), on, bnd, st, b.get_counters(), b.clock
    A, B = go(True), go(False)
    for x, y, what in zip(A[:5], B[:5], ("State", "particles", "on", "boundary", "status")):
        assert_bitwise(x, y, what)
    assert A[5] == B[5] and A[6] == B[6]


def test_refusals_leave_the_context_usable():
    cfg = configs.bench06_box(n=48)
    b = _ready(cfg).backend
    b.run_steps(cfg.Δt, 2)
    with pytest.raises(K.PiclesError, match="picles_diag_init first"):
        b.diag_push()
    with pytest.raises(K.PiclesError):
        b.diag_shape()
    for bad in ((0, 2), (17, 2), (2, 0), (2, 17)):
        with pytest.raises(K.PiclesError, match="1 ... 16"):
            b.diag_init(bad, ("hs",), 2)
    for mask in (0, 128, 1 << 20):
        with pytest.raises(K.PiclesError, match="field mask"):
            b.diag_init((2, 2), mask, 2)
    assert b.diag_pending == 0
    b.diag_init((2, 2), ("hs", "e"), 2)
    with pytest.raises(K.PiclesError, match="already initialised"):
        b.diag_init((2, 2), ("hs", "e"), 2)
    with pytest.raises(K.PiclesError, match="no diagnostics snapshot"):
        b.diag_pop()
    b.diag_push()
    b.diag_push()
    with pytest.raises(K.PiclesError, match="ring full"):
        b.diag_push()
    assert b.diag_pending == 2
    b.diag_pop()
    b.run_steps(cfg.Δt, 1)
    b.diag_push()
    b.diag_pop()
    f, p, t = b.diag_pop()
    assert t == 3 * cfg.Δt
    _check_snapshot(b, cfg, (2, 2), ("hs", "e"), f, p, "after the refusals")
    # a checkpoint may begin beside a diagnostics snapshot in flight; a load is refused as it is beside a store snapshot
    b.diag_push()
    b.checkpoint_begin()
    blob = b.checkpoint_end()
    with pytest.raises(K.CheckpointError) as e:
        b.checkpoint_load(blob)
    assert e.value.code == K.CKPT_E_BUSY
    b.diag_pop()
    b.checkpoint_load(blob)
    # a slab whose first row is not a multiple of cy
    ms = fetch_relations.MinimalState(2, 2, cfg.model["ODEsets"].timestep)
    g, p_, o, m_ = build_structs(cfg.model["grid"], cfg.model["ODEsys"], cfg.model["ODEsets"], None, ms, True, j_begin=8, j_end=24)
    hm = HipModel(g, p_, o, m_, mask=cfg.model["grid"].data.mask, device=0, halo_rows=2)
    with pytest.raises(K.PiclesError, match="multiple of cy"):
        hm.diag_init((2, 3), ("hs",), 2)
    hm.diag_init((2, 4), ("hs",), 2)
    assert hm.diag_shape()[:2] == (24, 4)
    hm.close()


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_give_the_single_context_fields_and_sums(world):
    from test_gpu_slab_fuzz import _NoExchange, _step_all
    make = lambda: configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * 48, 2000.0 * 48))      # noqa: E731
    cfg = make()
    pair, names = (3, 4), ("hs", "tp", "cg_x", "cg_y", "e")
    assert all(slab_rows(48, world, r)[0] % pair[1] == 0 for r in range(world))
    one = SlabModel(cfg.model, 0, 1, device=0)
    one.diag_init(pair, names, 2)
    one.seed()
    for _ in range(4):
        one.time_step(cfg.Δt)
    one.diag_push()
    f1, s1, t1 = one.gather_fields()
    S1 = one.get_state()
    g, r_g = _phys(cfg)
    assert_same_bits(f1, D.fields_of(S1, *pair, g, r_g, names=names)[0], "single context against the restatement")
    slabs = [SlabModel(make().model, r, world, device=0, halo_rows=2, exchange=_NoExchange()) for r in range(world)]
    for s in slabs:
        s._comm_warm = True
        s.diag_init(pair, names, 2)
        s.seed()
    for _ in range(4):
        _step_all(slabs, cfg.Δt, slabs[0].periodic_y, fused_ok=True)
    for s in slabs:
        s.diag_push()
    pops = [s.diag_pop() for s in slabs]
    assert_bitwise(np.concatenate([s.get_state() for s in slabs], axis=1), S1, "slab State")
    assert_same_bits(np.concatenate([f for f, _, _ in pops], axis=2), f1, f"{world} slabs: gathered fields")
    s2 = combine_partials([p for _, p, _ in pops], 48, 48)
    _same_scalars(s2, {k: s1[k] for k in SCALAR_NAMES}, f"{world} slabs")
    assert all(t == t1 for _, _, t in pops) and s1["n_wet"] == 48 * 48


@pytest.mark.parametrize("with_checkpointer", [False, True])
def test_run_with_field_writer(tmp_path, with_checkpointer):
    make = lambda: configs.bench06_box(n=64, winds=configs.smooth_winds(10.0, 10.0, 2000.0 * 64, 2000.0 * 64))      # noqa: E731
    cfg = make()
    n = 20
    m = make_model(cfg, "hip")
    sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n - 1))
    sim.output_writers["fields"] = FieldWriter(m, schedule=5, path=tmp_path, coarsen=(4, 4), format="npy")
    if with_checkpointer:
        sim.output_writers["checkpointer"] = Checkpointer(m, schedule=3, dir=tmp_path / "ck")
    run(sim)
    assert m.clock.iteration == n
    out = read_field_output(tmp_path)
    assert out["data"].shape == (n // 5 + 1, 16, 16, 4) and out["var_names"] == ["hs", "tp", "cg_x", "cg_y"]
    # the same model stepped through time_step, a push every 5
    ref = make_model(make(), "hip")
    initialize_simulation(Simulation(ref, Δt=cfg.Δt, stop_time=1.0))
    ref.backend.diag_init((4, 4), ("hs", "tp", "cg_x", "cg_y"), 8)
    ref.backend.diag_push()
    for it in range(1, n + 1):
        time_step(ref, cfg.Δt, zero_first=True)
        if it % 5 == 0:
            ref.backend.diag_push()
    for k in range(n // 5 + 1):
        f, p, t = ref.backend.diag_pop()
        assert out["time"][k] == t == 5 * k * cfg.Δt
        assert_bitwise(out["data"][k], np.moveaxis(f, 0, -1), f"record {k}")
        s = combine_partials(p, 64, 64)
        assert_bitwise(out["scalars"][k], np.array([s[q] for q in SCALAR_NAMES]), f"scalars of record {k}")
    assert np.isfinite(out["data"]).mean() >= 0.9
    # and the run itself is the run without the writer
    plain = make_model(make(), "hip")
    run(Simulation(plain, Δt=cfg.Δt, stop_time=cfg.Δt * (n - 1)))
    assert_bitwise(np.asarray(m.State), np.asarray(plain.State), "final State with and without the writer")
    if with_checkpointer:
        assert len(list((tmp_path / "ck").glob("*.picles"))) == 6
