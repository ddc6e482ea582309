"""The checkers of the hostile-value and lattice-geometry GPU tests, held on the CPU (no test here needs a GPU):

  * the vectorised restatement of the coarse diagnostics (tests/_diag_numpy.py) against a scalar, cell-by-cell loop written from
    the header text (tests/_hostile_states.py), in true bits, on the hostile generator — and the classes that generator must
    contain for tests/test_gpu_diag_hostile.py to mean anything;
  * the NumPy mirror of the wind sampler (picles_amd/wind_emulator.py) against the exact rational interpolant
    (tests/_wind_exact.py) within the rounding bound of tests/_wind_cases.py, over the geometries of
    tests/test_gpu_wind_sampler.py, and the cap on the nodes the seam rule may exclude.

Measured here (CPU, the 18 geometries, 102 nodes each, every level, u and v): the mirror's worst error is 0.19 of the bound."""
import numpy as np
import pytest

import _diag_numpy as D
import _hostile_states as H
import _wind_cases as W
import _wind_exact as X
from helpers import assert_same_bits, bits_of
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.wind_emulator import GriddedWinds

G, R_G = 9.81, 0.85

# (Nx, ny, cx, cy, seed): one per kernel path, small enough for the Python loop
SCALAR_CASES = [(40, 30, 1, 1, 11), (48, 27, 2, 2, 12), (45, 28, 2, 3, 13), (66, 40, 4, 4, 14), (61, 33, 4, 2, 15), (70, 38, 3, 5, 16),
                (300, 9, 1, 2, 17)]


@pytest.mark.parametrize("case", SCALAR_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_vectorised_restatement_equals_the_scalar_loop_on_hostile_states(case):
    Nx, ny, cx, cy, seed = case
    S = H.hostile_state(Nx, ny, cx, cy, seed)
    f, p = H.scalar_diag(S, cx, cy, G, R_G)
    assert_same_bits(D.fields_of(S, cx, cy, G, R_G)[0], f, f"{case}: fields")
    assert_same_bits(D.partials_of(S, cx, cy), p, f"{case}: partials")
    c = H.classes_of(S, cx, cy, G, R_G)
    print(case, c)
    H.assert_classes(c, case)


def test_scalar_loop_on_the_all_nan_grid_and_on_hand_values():
    S = H.all_nan_state(20, 9, 5)
    for cx, cy in ((1, 1), (4, 2), (3, 5)):
        f, p = H.scalar_diag(S, cx, cy, G, R_G)
        assert np.isnan(f).all()
        assert_same_bits(p, np.tile(np.array([0.0, 0.0, 0.0, 0.0, -np.inf, -np.inf, -np.inf]), (p.shape[0], 1)), "all-NaN partials")
        assert_same_bits(D.partials_of(S, cx, cy), p, "all-NaN partials, vectorised")
    # one cell by hand: two wet nodes whose m_x cancel -> MX = +0.0, cg_x = +0.0; a land node with negative zeros: the maximum of
    # m_y over (0.25, 0.25, -0.0) is 0.25; a cell of negative zeros alone has the maximum +0.0 after x + 0.0
    S = np.zeros((2, 2, 3))
    S[0, 0] = (1.0, 0.5, 0.25)
    S[1, 0] = (3.0, -0.5, 0.25)
    S[0, 1] = (-0.0, -0.0, -0.0)
    S[1, 1] = (-0.0, -0.0, -0.0)
    f, p = H.scalar_diag(S, 2, 1, G, R_G)
    assert f[4, 0, 0] == 2.0 and f[6, 0, 0] == 0.25 and f[0, 0, 0] == np.float32(4.0 * np.sqrt(2.0))
    assert f[5, 0, 0] == 0.0 and not np.signbit(f[5, 0, 0]) and f[2, 0, 0] == 0.0 and not np.signbit(f[2, 0, 0])
    assert np.isnan(f[:, 0, 1]).all()
    assert_same_bits(p, np.array([[4.0, 0.0, 0.5, 2.0, 3.0, 0.5, 0.25], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]), "hand partials")
    assert_same_bits(D.partials_of(S, 2, 1), p, "hand partials, vectorised")


def test_generators_are_seeded_and_keep_their_payloads_through_the_host_layer():
    from picles_amd.driver import _col
    a, b = H.hostile_state(33, 21, 4, 4, 3), H.hostile_state(33, 21, 4, 4, 3)
    assert_same_bits(a, b, "same seed", nan_payload=True)
    assert not np.array_equal(bits_of(a), bits_of(H.hostile_state(33, 21, 4, 4, 4)))
    # the Fortran-order flattening in front of picles_set_state is a plain copy: NaN payloads (signalling ones too) survive it
    flat = _col(a, a.size)
    assert_same_bits(flat.reshape(a.shape, order="F"), a, "driver._col", nan_payload=True)
    nan = np.isnan(a)
    payloads = np.unique(bits_of(a)[nan] & np.uint64((1 << 51) - 1))
    assert nan.sum() > 50 and payloads.size > 40 and (bits_of(a)[nan] >> np.uint64(63)).any()
    sw = H.sweep_state(64, 64, 1)
    assert np.isfinite(sw).all() and (sw[..., 0] == 0.0).mean() > 0.4
    f, valid = D.fields_of(sw, 1, 1, G, R_G)
    assert np.isfinite(f[:, valid]).all() and valid.mean() > 0.4


def test_assert_same_bits_sees_what_assert_bitwise_does_not():
    z, nz = np.array([0.0, 1.0]), np.array([-0.0, 1.0])
    with pytest.raises(AssertionError, match="bit patterns differ"):
        assert_same_bits(z, nz, "zeros")
    q = np.array([0x7FF8000000000001, 0xFFF8000000000002], dtype=np.uint64).view(np.float64)
    assert_same_bits(q, q[::-1].copy(), "NaNs by class")
    with pytest.raises(AssertionError, match="bit patterns differ"):
        assert_same_bits(q, q[::-1].copy(), "NaN payloads", nan_payload=True)
    with pytest.raises(AssertionError, match="dtype"):
        assert_same_bits(z, z.astype(np.float32), "dtype")
    with pytest.raises(AssertionError, match="shape"):
        assert_same_bits(z, z[:1], "shape")
    assert_same_bits(np.float32([-0.0, np.nan]), np.float32([-0.0, -np.nan]), "float32")


# ------------------------------------------------------------------------------------------------------------------------------------
# the wind mirror against the exact interpolant
# ------------------------------------------------------------------------------------------------------------------------------------
def _mirror(c):
    xmin, xmax, ymin, ymax = c.mesh
    grid = TwoDCartesianGridMesh(xmin, xmax, c.Nx, ymin, ymax, c.Ny)
    w = GriddedWinds(*c.knots, c.u, c.v, time_mode=c.mode)
    return grid, w


@pytest.mark.parametrize("c", W.all_cases(), ids=lambda c: c.name)
def test_numpy_mirror_is_within_the_bound_of_the_exact_interpolant(c):
    grid, w = _mirror(c)
    xs, ys = grid.data.x[:, 0], grid.data.y[0, :]
    mx, my = W.mesh_axes(c)
    assert_same_bits(xs, mx, "mesh x"); assert_same_bits(ys, my, "mesh y")
    lat = w.lattice()
    nodes = W.sample_nodes(c)
    worst = 0.0
    for name, t in W.level_times(c).items():
        if t is None:
            continue
        for F, f in ((c.u, w.u), (c.v, w.v)):
            vals = f(grid.data.x, grid.data.y, t)
            assert np.abs(vals).max() <= 30.0
            r, checked = W.worst_ratio(c, lat, F, xs, ys, t, vals, nodes)
            assert checked >= 0.9 * len(nodes), (c.name, name, checked)
            worst = max(worst, r)
    print(f"{c.name}: mirror vs exact, worst error / bound = {worst:.3f}")
    assert worst <= 1.0, (c.name, worst)
    share = W.excluded_share(c, lat, xs, ys)
    assert share <= W.SEAM_CAP, (c.name, share)
    if c.periodic:
        assert share == 0.0, (c.name, share)


def test_the_geometries_cover_what_they_claim():
    cases = {c.name: c for c in W.all_cases()}
    assert len(cases) == 18
    def coords(c):
        return W._coords(c)
    # negative coordinates, several periods on both sides, every axis
    c = cases["coarse_offset_pos_several_periods"]
    for cc, k in zip(coords(c), c.knots):
        per = k.size - 1
        assert cc.min() < -2.0 * per / 3 and cc.max() > 3 * per
    assert W.knot_inside(c) == 12200.0
    # a mesh strictly inside
    c = cases["fine_offset_neg_mesh_inside"]
    assert W.axes_left(c) == [False, False, False] and (c.Nx * c.Ny) % 256 == 0 and W.knot_inside(c) is None
    assert c.knots[0][1] - c.knots[0][0] < (c.mesh[1] - c.mesh[0]) / (c.Nx - 1)
    # nodes exactly on knots, on w = per, on whole multiples of the period, negative ones included; a time on the last knot
    c = cases["nodes_on_knots_and_period_multiples"]
    cx, cy, ct = coords(c)
    assert {-12.0, -8.0, -4.0, 0.0, 4.0, 8.0} <= set(cx.tolist()) and (cx == np.floor(cx)).sum() >= 20
    assert {2.0, 3.0, 8.0, 9.0} == set(ct.tolist())
    for name, axis in (("nx2", 0), ("ny2", 1), ("nt2", 2)):
        c = cases[name]
        assert c.knots[axis].size == 2 and not W.axes_left(c)[axis] and all(W.axes_left(c)[a] for a in range(3) if a != axis)
    c = cases["inexact_spacings_knot_inside"]
    dxm = (c.mesh[1] - c.mesh[0]) / (c.Nx - 1)
    assert dxm * 2.0 ** 40 != np.floor(dxm * 2.0 ** 40) and W.knot_inside(c) is not None
    assert cases["smooth3"].mode == "smooth3" and cases["slab_rows_8_24"].slab == (8, 24)
    c = cases["non_periodic_left"]
    assert not c.periodic and all(W.axes_left(c)) and all(W._jumps(c.u))
    assert sum((c.Nx * c.Ny) % 256 != 0 for c in cases.values()) >= 15
    assert sum(not c.periodic for c in cases.values()) >= 4 and sum(c.mode == "smooth3" for c in cases.values()) >= 3
    assert sum(W.knot_inside(c) is not None and c.mode == "linear" for c in cases.values()) >= 4
    # lattices finer and coarser than the mesh among the random ones
    ratio = [(c.knots[0][1] - c.knots[0][0]) / ((c.mesh[1] - c.mesh[0]) / (c.Nx - 1)) for c in W.random_cases()]
    assert min(ratio) < 0.8 and max(ratio) > 1.5


def test_lattice_coord_mutations_are_caught_by_the_exact_interpolant(monkeypatch):
    """the two mutations of lattice_coord that may not run on a device (one reads out of bounds), applied to the mirror: n as the
    period instead of n - 1 breaks the bound; without the i0 > n - 2 clamp a node on the last knot indexes past the lattice"""
    from picles_amd import wind_emulator as WE
    c = {k.name: k for k in W.directed()}["nodes_on_knots_and_period_multiples"]
    grid, w = _mirror(c)
    xs, ys = grid.data.x[:, 0], grid.data.y[0, :]

    def period_n(cc, n):
        per = float(n)
        cc = np.asarray(cc, dtype=np.float64)
        ww = np.where((cc < 0.0) | (cc > per), cc - np.floor(cc / per) * per, cc)
        i0 = np.maximum(np.minimum(np.floor(ww).astype(np.int64), n - 2), 0)
        return i0, ww - i0.astype(np.float64)

    def no_clamp(cc, n):
        per = float(n - 1)
        cc = np.asarray(cc, dtype=np.float64)
        ww = np.where((cc < 0.0) | (cc > per), cc - np.floor(cc / per) * per, cc)
        i0 = np.maximum(np.floor(ww).astype(np.int64), 0)
        return i0, ww - i0.astype(np.float64)

    monkeypatch.setattr(WE, "_lattice_coord", period_n)
    r, _ = W.worst_ratio(c, w.lattice(), c.u, xs, ys, 3600.0, w.u(grid.data.x, grid.data.y, 3600.0), W.sample_nodes(c))
    assert r > 1e6
    monkeypatch.setattr(WE, "_lattice_coord", no_clamp)
    with pytest.raises(IndexError):
        w.u(grid.data.x, grid.data.y, 1800.0)
