"""k_diag on synthetic, hostile States — set_state(S) -> diag_init / diag_push / diag_pop — against the NumPy restatement of the
definition (tests/_diag_numpy.py, itself held to a scalar loop in tests/test_aux_references.py) in TRUE bits: the sign of a zero
counts, NaNs compare by class.  The States (tests/_hostile_states.py) hold what a healthy sea never does: the whole double range,
signed zeros, NaNs with payloads, infinities, subnormals, squares that underflow and overflow, sums that overflow and cancel,
float32 results in the subnormal range and past FLT_MAX, cells with exactly 0, 1, 2 and all nodes wet, a dry tile whose maxima
are negative zeros, a grid of NaN.  Hostile means hostile values: every shape, index and size is valid.

And the four plain copies out of State (get_state, the store ring, the plain-gather probe, a checkpoint round trip) hand back
the 64-bit patterns they were given, NaN payloads included.

Which case reaches which instantiation of k_diag<CX, VEC> (picles_diag_push: VEC when Nx is even) and which boundary:

    <1, false>  1x1_40x30, tile_255 / tile_256 / tile_257 / tile_513 (cy = 2), sweep (1, 1), smallest_2x2
    <2, true>   2x2_even (ragged cy)
    <2, false>  2x3_odd (ragged last cell in x: 1 node; ragged cy), tile_257_cx2 (the lane of the second tile is the ragged cell)
    <4, true>   4x4_whole, 4x4_even_ragged (last cell 2 nodes), tile_257_cx4 (ditto, alone in its tile), sweep (4, 4),
                nx_below_cx_even (Nx = 2 < 4: the only cell is ragged), slab
    <4, false>  4x2_odd_ragged (last cell 1 node; ragged cy), nx_below_cx_odd
    <0, false>  rt_3x5, rt_5x3, rt_8x2, rt_16x16; ny_below_cy (one coarse row), one_cell (3 x 3 under 16 x 16)
    tiles       255: one tile, a lane short; 256: a full tile; 257: a tile of one lane; 513: three tiles
    slab        rows 8 ... 26 of 40 under cy = 4: j_begin a multiple of cy, ragged ny_loc = 19"""
import numpy as np
import pytest

import _diag_numpy as D
import _hostile_states as H
from helpers import assert_same_bits, bits_of, make_model
from picles_amd import _capi as K, configs, fetch_relations
from picles_amd.driver import HipModel, SCALAR_NAMES, combine_partials
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.models import build_structs
from picles_amd.simulations import Simulation, initialize_simulation

pytestmark = pytest.mark.gpu

_CFG = configs.example_00_minimal(n=9, L=16e3)          # the physics (g, r_g) and the solver settings of every context below
G, R_G = _CFG.model["ODEsets"].Parameters.get("g", 9.81), _CFG.model["ODEsets"].Parameters["r_g"]


def _ctx(Nx, Ny, rows=None):
    """a bare context on an Nx x Ny mesh (rows = (j_begin, j_end): a slab of it), as test_refusals_leave_the_context_usable builds one"""
    grid = TwoDCartesianGridMesh(2000.0 * (Nx - 1), Nx, 2000.0 * (Ny - 1), Ny)
    ms = fetch_relations.MinimalState(2, 2, _CFG.model["ODEsets"].timestep)
    j0, j1 = rows if rows else (0, None)
    g, p, o, m = build_structs(grid, _CFG.model["ODEsys"], _CFG.model["ODEsets"], None, ms, False, j_begin=j0, j_end=j1)
    return HipModel(g, p, o, m, mask=grid.data.mask, device=0, halo_rows=2)


def _same_scalars(got, want, what):
    for k in SCALAR_NAMES:
        assert_same_bits(np.array([got[k]], dtype=np.float64), np.array([want[k]], dtype=np.float64), f"{what}: scalar {k}")


def _diag_of(b, S, pair, names=K.DIAG_FIELDS):
    """fields, partials of State S through the device: a ring of two, the snapshot pushed twice (both slots must agree)"""
    b.set_state(S)
    b.diag_init(pair, names, 2)
    nxc, nyc = D.coarse_shape(S.shape[0], S.shape[1], *pair)
    assert b.diag_shape()[:4] == (nxc, nyc, len(names), nyc * -(-nxc // 256))
    b.diag_push()
    b.diag_push()
    f, p, _ = b.diag_pop()
    f2, p2, _ = b.diag_pop()
    assert_same_bits(f2, f, "second slot: fields"); assert_same_bits(p2, p, "second slot: partials")
    return f, p


def _check(b, S, pair, what, names=K.DIAG_FIELDS, Ny=None):
    f, p = _diag_of(b, S, pair, names)
    assert_same_bits(b.get_state(), S, f"{what}: State as set", nan_payload=True)
    with np.errstate(all="ignore"):
        want_f, _ = D.fields_of(S, *pair, G, R_G, names=names)
        want_p = D.partials_of(S, *pair)
    assert_same_bits(f, want_f, f"{what}: fields")
    assert_same_bits(p, want_p, f"{what}: partials")
    Ny = S.shape[1] if Ny is None else Ny
    _same_scalars(combine_partials(p, S.shape[0], Ny), D.combine([want_p], S.shape[0], Ny), what)
    return want_p


# name: (Nx, Ny, cx, cy, seed, fields).  Seeds: those for which the generator meets the class conditions (asserted below and, for the
# scalar loop's cases, in tests/test_aux_references.py)
MIXED = {
    "1x1_40x30":        (40, 30, 1, 1, 11, K.DIAG_FIELDS),
    "2x2_even":         (48, 27, 2, 2, 12, K.DIAG_FIELDS),
    "2x3_odd":          (45, 28, 2, 3, 13, ("hs", "cg_x", "m_y")),
    "4x4_whole":        (64, 40, 4, 4, 114, K.DIAG_FIELDS),
    "4x4_even_ragged":  (70, 44, 4, 4, 15, K.DIAG_FIELDS),
    "4x2_odd_ragged":   (61, 33, 4, 2, 15, K.DIAG_FIELDS),
    "rt_3x5":           (70, 38, 3, 5, 16, K.DIAG_FIELDS),
    "rt_5x3":           (90, 36, 5, 3, 17, ("tp", "cg_y", "e", "m_x")),
    "rt_8x2":           (120, 40, 8, 2, 18, K.DIAG_FIELDS),
    "rt_16x16":         (480, 160, 16, 16, 19, K.DIAG_FIELDS),
    "tile_255":         (255, 8, 1, 2, 20, K.DIAG_FIELDS),
    "tile_256":         (256, 8, 1, 2, 21, K.DIAG_FIELDS),
    "tile_257":         (257, 8, 1, 2, 22, K.DIAG_FIELDS),
    "tile_513":         (513, 6, 1, 2, 23, K.DIAG_FIELDS),
    "tile_257_cx2":     (513, 6, 2, 2, 24, K.DIAG_FIELDS),
    "tile_257_cx4":     (1026, 12, 4, 4, 25, K.DIAG_FIELDS),
}
# too few coarse cells for the class conditions; the point is the shape: the smallest grids the library accepts
TINY = {
    "nx_below_cx_odd":  (3, 9, 4, 2, 31),
    "nx_below_cx_even": (2, 7, 4, 3, 32),
    "ny_below_cy":      (9, 3, 2, 5, 33),
    "one_cell":         (3, 3, 16, 16, 34),
    "smallest_2x2":     (2, 2, 1, 1, 35),
}


@pytest.mark.parametrize("case", list(MIXED))
def test_hostile_states_bit_for_bit(case):
    Nx, Ny, cx, cy, seed, names = MIXED[case]
    S = H.hostile_state(Nx, Ny, cx, cy, seed)
    c = H.classes_of(S, cx, cy, G, R_G)
    print(case, c)
    H.assert_classes(c, case)
    b = _ctx(Nx, Ny)
    want_p = _check(b, S, (cx, cy), case, names)
    b.close()
    # the dry tile: nothing above -0.0 in it, so its three maxima are zeros that only the x + 0.0 of the definition makes positive
    t = H.dry_tile_nodes(Nx, Ny, cx, cy)
    v = S[t]
    assert t.any() and (np.isnan(v) | np.signbit(v)).all() and all(((v[:, k] == 0.0) & np.signbit(v[:, k])).any() for k in range(3))
    assert_same_bits(want_p[-1], np.zeros(7), f"{case}: the dry tile's partial")


@pytest.mark.parametrize("case", list(TINY))
def test_smallest_grids(case):
    Nx, Ny, cx, cy, seed = TINY[case]
    b = _ctx(Nx, Ny)
    _check(b, H.hostile_state(Nx, Ny, cx, cy, seed), (cx, cy), case)
    b.close()
    # and a healthy sea of the same shape, so that the few cells there are hold numbers
    b = _ctx(Nx, Ny)
    S = H._sea(np.random.default_rng(seed), Nx * Ny).reshape(Nx, Ny, 3)
    _check(b, S, (cx, cy), case + ", sea")
    assert np.isfinite(D.fields_of(S, cx, cy, G, R_G)[0]).all()
    b.close()


def test_slab_context_with_ragged_rows():
    Nx, Ny, rows, pair = 200, 40, (8, 27), (4, 4)
    S = H.hostile_state(Nx, rows[1] - rows[0], *pair, 41)
    H.assert_classes(H.classes_of(S, *pair, G, R_G), "slab")
    b = _ctx(Nx, Ny, rows)
    assert (b.j_begin, b.ny_loc) == (8, 19)
    _check(b, S, pair, "slab rows 8 ... 26", Ny=Ny)
    assert b.diag_shape()[:2] == (50, 5)
    b.close()


@pytest.mark.parametrize("pair", [(1, 1), (4, 4), (3, 5)])
def test_a_grid_of_nan(pair):
    S = H.all_nan_state(40, 30, 51)
    b = _ctx(40, 30)
    f, p = _diag_of(b, S, pair)
    b.close()
    assert np.isnan(f).all()
    assert_same_bits(p, np.tile(np.array([0.0, 0.0, 0.0, 0.0, -np.inf, -np.inf, -np.inf]), (p.shape[0], 1)), "every sum +0.0, every maximum -inf")
    assert_same_bits(p, D.partials_of(S, *pair), "the restatement says the same")
    s = combine_partials(p, 40, 30)
    _same_scalars(s, dict(sum_e=0.0, sum_mx=0.0, sum_my=0.0, n_wet=0.0, max_e=-np.inf, max_mx=-np.inf, max_my=-np.inf, mean_of_state=0.0), "NaN grid")


@pytest.mark.parametrize("pair", [(1, 1), (4, 4)])
def test_two_million_nodes_every_sqrt_and_division_to_the_last_bit(pair):
    """2048 x 1024 nodes, planes log-uniform over the exponent range in which e, m2 and the float32 planes stay finite, a band of
    subnormal operands, dry nodes from one in fifty on the left to nearly all on the right.  At (1, 1) every wet node is one fp64 sqrt of E, one of M2 and four divisions; at
    (4, 4) the three divisions by n = 1 ... 16 come on top.  An inexact sqrt or division sequence, or a flushed subnormal, shows here."""
    Nx, Ny = 2048, 1024
    S = H.sweep_state(Nx, Ny, 61)
    b = _ctx(Nx, Ny)
    f, p = _diag_of(b, S, pair)
    b.close()
    with np.errstate(all="ignore"):
        want_f, valid = D.fields_of(S, *pair, G, R_G)
        want_p = D.partials_of(S, *pair)
        (_, _, _, n), _ = D.cell_sums(S, *pair)
    # what the sweep holds, on the restatement: valid cells, all of them finite, float32 subnormals among them, every divisor
    assert 0.4 <= valid.mean() and np.isfinite(want_f[:, valid]).all() and np.isnan(want_f[:, ~valid]).all()
    assert ((np.abs(want_f) > 0) & (np.abs(want_f) < np.float32(H.F32_TINY))).sum() >= (1000 if pair == (1, 1) else 0)
    assert set(np.unique(n).tolist()) >= (set(range(1, 17)) if pair == (4, 4) else {0.0, 1.0})
    assert_same_bits(f, want_f, f"sweep {pair}: fields")
    assert_same_bits(p, want_p, f"sweep {pair}: partials")
    _same_scalars(combine_partials(p, Nx, Ny), D.combine([want_p], Nx, Ny), f"sweep {pair}")


def _seeded():
    """a seeded model as a run leaves it before its first step: no fused step pending"""
    cfg = configs.example_00_minimal(n=33, L=64e3)
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    return m.backend


def test_copies_out_of_state_keep_every_bit():
    """set_state -> get_state, the store ring, the plain gather of the station probes (no step pending) and a checkpoint loaded
    into a second context: identical 64-bit patterns, NaN payloads (quiet and signalling, both signs) and -0.0 included"""
    S = H.hostile_state(33, 33, 4, 2, 71)
    bits = bits_of(S)
    nan = np.isnan(S)
    assert nan.sum() > 100 and np.unique(bits[nan]).size > 100 and ((S == 0.0) & np.signbit(S)).sum() > 20 and np.isinf(S).sum() > 20
    assert ((bits[nan] >> np.uint64(51)) & np.uint64(1) == 0).sum() > 10          # signalling ones among them
    b = _seeded()
    b.set_state(S)
    assert_same_bits(b.get_state(), S, "get_state", nan_payload=True)
    b.store_init(2)
    b.store_push()
    b.store_push()
    for k in range(2):
        got, t = b.store_pop()
        assert_same_bits(got, S, f"store slot {k}", nan_payload=True)
    rng = np.random.default_rng(72)
    nodes = np.stack([rng.integers(0, 33, 300), rng.integers(0, 33, 300)], axis=1)
    b.probe_init(nodes, every=1, first=1, capacity=4)
    b.probe_sample()
    v, _, _ = b.probe_pop()
    assert v.shape == (1, 3, 300)
    assert_same_bits(v[0], np.ascontiguousarray(S[nodes[:, 0], nodes[:, 1], :].T), "probe, plain gather", nan_payload=True)
    b.probe_free()
    b.checkpoint_begin()
    blob = b.checkpoint_end()
    b2 = _seeded()
    b2.checkpoint_load(blob)
    assert_same_bits(b2.get_state(), S, "State of the context that loaded the checkpoint", nan_payload=True)
    assert_same_bits(b.get_state(), S, "State of the context that wrote it", nan_payload=True)
    b.close(); b2.close()
