"""Flux means, the host side (no GPU): the NumPy finalisation and tile tree of tests/_flux_mean_numpy.py and the host tile tree of
picles_amd/driver.py against hand-computed tiny cases; MeanFluxWriter's argument checks, record schedule and side-car round trip
with a fake backend."""
import warnings

import numpy as np
import pytest

import _flux_mean_numpy as FM
from picles_amd import _capi as K
from picles_amd.driver import combine_flux_partials, flux_mean_concat, flux_mean_tile_partials
from picles_amd.flux_output import MEAN_SIDECAR_SUFFIX, FluxWriter, MeanFluxWriter
from picles_amd.output_writers import PHASE_ORDER


def test_cover_counts_the_nodes_of_ragged_cells():
    c = FM.cover(7, 5, 4, 3)
    assert c.tolist() == [[12.0, 8.0], [9.0, 6.0]]
    assert FM.cover(6, 4, 1, 1).tolist() == np.ones((6, 4)).tolist()


def test_finalise_by_hand():
    acc = np.zeros((11, 2, 1))
    acc[0, :, 0] = [6.0, 1.0]          # phi_in
    acc[3, :, 0] = [-3.0, 0.5]         # tq_in_x
    acc[7, :, 0] = [1.0, 1e300]        # us_x
    ncov = np.array([[4.0], [2.0]])
    f = FM.finalise(acc, ncov, 3, scale_phi=2.0, scale_tau=10.0, names=("phi_in", "tq_in_x", "us_x"))
    assert f.dtype == np.float32 and f.shape == (3, 2, 1)
    assert f[0, :, 0].tolist() == [np.float32((6.0 / 12.0) * 2.0), np.float32((1.0 / 6.0) * 2.0)]
    assert f[1, :, 0].tolist() == [np.float32((-3.0 / 12.0) * 10.0), np.float32((0.5 / 6.0) * 10.0)]
    assert f[2, 0, 0] == np.float32(1.0 / 12.0) and np.isinf(f[2, 1, 0])      # a finite mean beyond float32 rounds to inf
    # the division is by the product, not two divisions: 1 / (3 * 3) is not (1 / 3) / 3 in fp64 for every numerator
    a = np.zeros((11, 1, 1)); a[8] = 7.0
    assert FM.finalise(a, np.array([[3.0]]), 3, names=("us_y",))[0, 0, 0] == np.float32(7.0 / 9.0)
    with pytest.raises(AssertionError):
        FM.finalise(acc, ncov, 0)


def test_tile_tree_by_hand_and_against_the_host_layer():
    # one tile, three live columns: ((a0 + 0) ... ) the halving tree pairs lane k with lane k + 32, 16, 8, 4, 2, 1
    acc = np.zeros((11, 3, 2))
    acc[0, :, 0] = [1.0, 2.0 ** -60, -1.0]
    acc[9, :, 1] = [5.0, 6.0, 7.0]
    t = FM.tile_tree(acc)
    assert t.shape == (2, 11)
    # lanes 0..2 of wave 0: the tree ends with ((l0 + l2) + (l1 + l3)) = ((1 + -1) + (2^-60 + 0))
    assert t[0, 0] == (1.0 + -1.0) + 2.0 ** -60 and t[0, 0] != (1.0 + 2.0 ** -60) + -1.0
    assert t[1, 9] == 18.0 and t[0, 9] == 0.0
    # 300 columns: two tiles per row; the waves of a tile are added in ascending order
    rng = np.random.default_rng(3)
    acc = rng.normal(size=(11, 300, 3)) * 10.0 ** rng.integers(-8, 8, size=(11, 300, 3))
    t = FM.tile_tree(acc)
    assert t.shape == (6, 11)
    assert np.array_equal(t, flux_mean_tile_partials(acc))
    w = [FM.tile_tree(np.pad(acc[:, 64 * k:64 * (k + 1), :1], ((0, 0), (0, 0), (0, 0))))[0, 4] for k in range(4)]
    assert t[0, 4] == ((w[0] + w[1]) + w[2]) + w[3]
    # totals: sequential over (J, tile), divided by n
    tot = FM.totals([t], 4)
    c = combine_flux_partials(t)
    assert tot == [c[k] / 4 for k in K.FLUX_PARTIAL]


def test_concat_stacks_row_blocks_and_combines_in_rank_order():
    rng = np.random.default_rng(5)
    whole = rng.normal(size=(11, 5, 6))
    parts = [dict(acc=whole[:, :, :2], n_samples=2, t_first=1.0, t_last=2.0), dict(acc=whole[:, :, 2:], n_samples=2, t_first=1.0, t_last=2.0)]
    got = flux_mean_concat(parts)
    assert np.array_equal(got["acc"], whole) and got["n_samples"] == 2
    one = flux_mean_concat([dict(acc=whole, n_samples=2, t_first=1.0, t_last=2.0)])
    assert got["totals"] == one["totals"]                 # coarse rows are whole on every rank: the same (J, tile) order
    assert flux_mean_concat([dict(acc=whole, n_samples=0, t_first=0.0, t_last=0.0)])["totals"] is None


class _Clock:
    def __init__(self, it):
        self.iteration, self.time = it, 600.0 * it


class _Grid:
    class data:
        x = np.arange(8.0)[:, None] * np.ones((1, 6))
        y = np.ones((8, 1)) * np.arange(6.0)[None, :]


class _FakeBackend:
    """records the calls; one sample per step, the accumulator counts them"""
    def __init__(self):
        self.calls, self.ring, self.acc, self.n, self.t, self.set_on = [], [], np.zeros((11, 2, 2)), 0, 0.0, False
    def flux_init(self, *a): self.calls.append(("flux_init",) + a)
    def flux_mean_init(self, every=1, first=1): self.calls.append(("flux_mean_init", every, first)); self.set_on = True
    def flux_mean_free(self): self.calls.append(("flux_mean_free",)); self.set_on = False; self.n = 0; self.acc = np.zeros((11, 2, 2))
    def flux_mean_scalars(self): return self.n, 0.0, self.t
    def flux_mean_get(self): return dict(acc=self.acc.copy(), n_samples=self.n, t_first=0.0, t_last=self.t)
    def flux_mean_set(self, a): self.acc, self.n, self.t = np.array(a["acc"]), a["n_samples"], a["t_last"]; self.calls.append(("flux_mean_set", a["n_samples"]))
    def step(self): self.acc = self.acc + 1.0; self.n += 1; self.t += 600.0
    @property
    def flux_pending(self): return len(self.ring)
    def flux_mean_push(self, reset=True):
        self.ring.append((np.full((9, 2, 2), self.acc[0, 0, 0] / self.n, dtype=np.float32), np.tile(self.acc.sum(axis=(1, 2)), (1, 1)), self.t))
        if reset:
            self.acc, self.n = np.zeros((11, 2, 2)), 0
    def flux_pop(self): return self.ring.pop(0)


class _Model:
    def __init__(self, it=0):
        self.backend, self.clock, self.grid = _FakeBackend(), _Clock(it), _Grid()


def test_writer_argument_checks_and_phase_order():
    with pytest.raises(ValueError, match="needs a schedule"):
        MeanFluxWriter(None)
    for every in (0, 2, 4, -1):
        with pytest.raises(ValueError, match="must be >= 1 and divide the schedule"):
            MeanFluxWriter(None, schedule=3, every=every)
    with pytest.raises(ValueError, match="rho_water"):
        MeanFluxWriter(None, schedule=3, rho_water=0.0)
    w = MeanFluxWriter(None, schedule=6, every=2, fields=("us_x", "phi_in"))
    assert w.kind == "flux_means" and w.name == "flux_means" and w.samples_per_record == 3 and w.fields == ("phi_in", "us_x")
    assert "DISCARDED" in MeanFluxWriter.__doc__
    for phase, order in PHASE_ORDER.items():
        if "fluxes" in order:
            assert order.index("flux_means") == order.index("fluxes") + 1, phase
    # the pair is refused, with a text that says why
    class Sim: Δt = 600.0
    with pytest.raises(ValueError, match="share the one flux ring.*pop each other's records"):
        w.check_run(Sim(), [w, FluxWriter(None, schedule=3)])
    w.check_run(Sim(), [w])


def test_record_schedule_no_record_at_the_start_and_leftovers_discarded(tmp_path):
    w = MeanFluxWriter(None, schedule=3, path=tmp_path, coarsen=(4, 3), format="npy")
    assert [w.records_of(0, n) for n in (2, 3, 8, 9)] == [0, 1, 2, 3] and w.records_of(4, 5) == 2 and w.records_of(3, 2) == 0
    m = _Model()
    b = m.backend
    w.begin_run(m, 8)
    assert ("flux_mean_init", 1, 1) in b.calls and b.flux_pending == 0 and w.iterations == []      # nothing at the starting iteration
    assert w.steps_allowed(b, 0) == 3 and w.steps_allowed(b, 4) == 2
    for it in range(1, 9):
        b.step()
        m.clock = _Clock(it)
        w.at_iteration(m, [w])
    assert w.iterations == [3, 6] and b.n == 2                                                     # two samples left over
    w.finish(b, 8)
    assert not b.set_on and b.calls[-1] == ("flux_mean_free",)
    from picles_amd.flux_output import read_flux_output
    out = read_flux_output(tmp_path, name="flux_means")
    assert out["averaged"] is True and out["samples_per_record"] == 3 and out["time"] == [1800.0, 3600.0]
    assert out["data"].shape == (2, 2, 2, 9) and (out["data"] == 1.0).all()
    assert (out["scalars"] == 4.0).all()                  # the combined partials (4 cells x 3) divided by the three samples
    # a cadence continued from a model's iteration: every = 2 from iteration 5 samples step 1 (iteration 6)
    w2 = MeanFluxWriter(None, schedule=4, every=2, path=tmp_path / "b", format="npy")
    m2 = _Model(5)
    w2.begin_run(m2, 4)
    assert ("flux_mean_init", 2, 1) in m2.backend.calls


def test_side_car_round_trip_missing_and_foreign(tmp_path):
    w = MeanFluxWriter(None, schedule=3, path=tmp_path, format="npy")
    m = _Model()
    w.begin_run(m, 9)
    for _ in range(4):
        m.backend.step()
    m.backend.flux_mean_push(reset=True); m.backend.step()             # as after iteration 3, with the sample of step 4 held
    ck = tmp_path / "ck" / "run_iteration4.picles"
    path = w.checkpoint_begun(m.backend, ck)
    assert path.name == ck.name + MEAN_SIDECAR_SUFFIX and path.exists()
    held = m.backend.flux_mean_get()
    w2 = MeanFluxWriter(None, schedule=3, path=tmp_path / "second", format="npy")
    assert w2.load_pickup(ck) is True
    m2 = _Model(4)
    w2.begin_run(m2, 5)
    got = m2.backend.flux_mean_get()
    assert ("flux_mean_init", 1, 1) in m2.backend.calls and ("flux_mean_set", 1) in m2.backend.calls
    assert np.array_equal(got["acc"], held["acc"]) and got["n_samples"] == held["n_samples"] == 1 and got["t_last"] == held["t_last"]
    # picked up AT a record's iteration: that interval was written by the run that stopped
    w3 = MeanFluxWriter(None, schedule=3, path=tmp_path / "third", format="npy")
    assert w3.load_pickup(ck) is True
    m3 = _Model(6)
    w3.begin_run(m3, 3)
    assert not any(c[0] == "flux_mean_set" for c in m3.backend.calls)
    # a missing and a foreign side-car: a warning, and the open interval starts afresh
    with pytest.warns(UserWarning, match="no flux-mean side-car"):
        assert MeanFluxWriter(None, schedule=3).load_pickup(tmp_path / "ck" / "other.picles") is False
    with pytest.warns(UserWarning, match="another coarsening, sampling or schedule"):
        assert MeanFluxWriter(None, schedule=6).load_pickup(ck) is False
    with pytest.warns(UserWarning, match="another coarsening"):
        assert MeanFluxWriter(None, schedule=3, coarsen=(2, 2)).load_pickup(ck) is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert MeanFluxWriter(None, schedule=3).load_pickup(ck) is True


def _has_hdf5():
    try:
        from picles_amd.storing import hdf5
        hdf5()
        return True
    except OSError:
        return False


@pytest.mark.skipif(not _has_hdf5(), reason="no libhdf5 loads here (the .npy form is tested above)")
def test_hdf5_form_carries_the_two_entries_and_a_snapshot_file_reads_without_them(tmp_path):
    from picles_amd.flux_output import make_flux_store, read_flux_output
    w = MeanFluxWriter(None, schedule=2, path=tmp_path, coarsen=(4, 3), format="hdf5")
    m = _Model()
    b = m.backend
    w.begin_run(m, 4)
    for it in range(1, 5):
        b.step()
        m.clock = _Clock(it)
        w.at_iteration(m, [w])
    w.finish(b, 4)
    assert (tmp_path / "flux_means.h5").exists()
    out = read_flux_output(tmp_path, name="flux_means")
    assert out["averaged"] is True and out["samples_per_record"] == 2 and out["time"] == [1200.0, 2400.0]
    assert out["data"].shape == (2, 2, 2, 9) and (out["data"] == 1.0).all() and (out["scalars"] == 4.0).all()
    # a FluxWriter's file has neither entry: read as before, and no key is invented
    st = make_flux_store(tmp_path / "snap", "fluxes", np.zeros(1), [0.0, 1.0], [0.0, 1.0], K.FLUX_FIELDS,
                         {"units": ["x"] * 9, "rho_water": 1025.0, "scale_phi": 2.0, "scale_tau": 3.0}, format="hdf5")
    st.write(0, np.zeros((9, 2, 2), dtype=np.float32), [0.0] * 11, 5.0)
    st.close()
    snap = read_flux_output(tmp_path / "snap")
    assert "averaged" not in snap and "samples_per_record" not in snap and snap["time"] == [5.0] and snap["scale_tau"] == 3.0
