"""Run statistics on the CPU box: the vectorised restatement of the contract (tests/_stats_numpy.py, which the device planes are
held against) against a scalar pure-Python restatement written from the header's text that shares no code with it — on the hostile
States of tests/_hostile_states.py and on constructed cases —, and StatisticsWriter + run() over a backend that records its calls
(the pattern of tests/test_station_output_host.py): windows, reset, chunking of run(), the file round trip in both forms, the
side-car and the pickup of an open window, refusal of bad arguments before the library is reached."""
import math
import struct
import warnings

import numpy as np
import pytest

import _hostile_states as H
import _stats_numpy as SN
from picles_amd import _capi as K, configs, models
from picles_amd.checkpointing import Checkpointer
from picles_amd.field_output import FieldWriter
from picles_amd.run_statistics import (FOUR_PI, StatisticsWriter, check_arguments, derive, read_statistics, var_names, variable)
from picles_amd.simulations import Simulation, run
from test_field_output_host import FakeBackend

G, RG = 9.81, 0.85


# ---- the scalar restatement: one node, one sample, one operation at a time, as the header words it ---------------------------------
def scalar_stats(samples, mask, thr):
    Nx, ny = samples[0][0].shape[:2]
    out = {}
    for i in range(Nx):
        for j in range(ny):
            n_wet, peak, sums, n_exc = 0, [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0] * len(thr)
            for S, clock in samples:
                e, mx, my = float(S[i, j, 0]), float(S[i, j, 1]), float(S[i, j, 2])
                if not (math.isfinite(e) and math.isfinite(mx) and math.isfinite(my)):
                    continue
                if not e > 0.0:
                    continue
                try:
                    m2 = mx * mx + my * my
                except OverflowError:          # (Python raises where IEEE gives +inf)
                    m2 = math.inf
                if not m2 > 0.0:
                    continue
                if n_wet == 0 or e > peak[0]:
                    peak = [e, mx, my, float(clock)]
                n_wet += 1
                hs = 4.0 * math.sqrt(e)
                sums = [sums[0] + e, sums[1] + mx, sums[2] + my, sums[3] + hs]
                for k, t in enumerate(thr):
                    if hs >= t:
                        n_exc[k] += 1
            out[i, j] = (n_wet, peak, sums, n_exc)
    return out


def _same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def assert_vector_equals_scalar(samples, thr, what):
    acc = SN.accumulate(samples, 7, thr)
    ref = scalar_stats(samples, 7, thr)
    for (i, j), (n_wet, peak, sums, n_exc) in ref.items():
        assert int(acc["n_wet"][i, j]) == n_wet, (what, i, j)
        for name, v in zip(SN.PEAK_PLANES, peak):
            assert _same_bits(float(acc[name][i, j]), v), (what, name, i, j, acc[name][i, j], v)
        for name, v in zip(SN.MEAN_PLANES, sums):
            assert _same_bits(float(acc[name][i, j]), v), (what, name, i, j, acc[name][i, j], v)
        assert acc["n_exc"][i, j].tolist() == n_exc, (what, i, j)
    assert acc["n_samples"] == len(samples) and acc["t_first"] == samples[0][1] and acc["t_last"] == samples[-1][1]
    return acc


def hostile_samples(Nx, ny):
    """(the samples tests/test_gpu_run_stats.py uploads to the device)"""
    S = [H.hostile_state(Nx, ny, 2, 2, seed) for seed in (11, 12, 13)]
    S += [H.sweep_state(Nx, ny, 14), H.all_nan_state(Nx, ny, 15), S[0]]
    return [(s, 600.0 * (k + 1)) for k, s in enumerate(S)]


def test_vectorised_restatement_equals_the_scalar_one_on_hostile_states():
    thr = (0.05, 0.5, 1.0, 3.0)
    acc = assert_vector_equals_scalar(hostile_samples(24, 20), thr, "hostile")
    # the inputs exercise what they are meant to: dry and wet nodes, overflowing sums, every threshold met somewhere and missed elsewhere
    assert 0 < int((acc["n_wet"] == 0).sum()) and int(acc["n_wet"].max()) >= 4
    assert np.isinf(acc["sum_e"]).any() and np.isinf(acc["sum_hs"]).sum() == 0
    for k in range(4):
        c = acc["n_exc"][..., k]
        assert 0 < int(c.sum()) < int(acc["n_wet"].sum())


def _one(*triples):
    """samples of a 1 x 1 grid"""
    return [(np.array(t, dtype=np.float64).reshape(1, 1, 3), 100.0 * (k + 1)) for k, t in enumerate(triples)]


def test_constructed_cases():
    thr = (1.0, 2.0)
    sub = 5e-324
    cases = {
        "nan": [(math.nan, 1.0, 1.0), (1.0, math.nan, 0.0), (1.0, 0.0, math.nan)],
        "inf": [(math.inf, 1.0, 1.0), (1.0, -math.inf, 0.0), (-math.inf, 1.0, 1.0)],
        "negative zero": [(-0.0, 1.0, 1.0), (1.0, -0.0, -0.0), (0.0, 0.0, 0.0)],
        "negative e": [(-1.0, 0.5, 0.5)],
        "e > 0 with zero momentum": [(2.0, 0.0, 0.0)],
        "subnormal momentum squares to zero": [(1.0, sub, -sub), (1.0, 1e-170, 1e-170)],
    }
    for what, triples in cases.items():
        acc = assert_vector_equals_scalar(_one(*triples), thr, what)
        assert acc["n_wet"][0, 0] == 0 and acc["n_samples"] == len(triples), what
        for name in SN.PEAK_PLANES + SN.MEAN_PLANES:
            assert acc[name][0, 0] == 0.0, (what, name)
    # subnormal e is wet; a momentum whose square overflows is wet
    acc = assert_vector_equals_scalar(_one((sub, 1.0, 0.0), (1.0, 1e200, 1e200)), thr, "subnormal e, huge m")
    assert acc["n_wet"][0, 0] == 2 and acc["e_peak"][0, 0] == 1.0 and acc["t_peak"][0, 0] == 200.0
    # a repeated maximum: the first time is kept (and its momentum)
    acc = assert_vector_equals_scalar(_one((1.0, 0.1, 0.0), (3.0, 0.2, 0.0), (2.0, 0.3, 0.0), (3.0, 0.4, 0.0)), thr, "repeated maximum")
    assert (acc["e_peak"][0, 0], acc["mx_peak"][0, 0], acc["t_peak"][0, 0]) == (3.0, 0.2, 200.0)
    # a first wet sample below the zero the planes start from cannot happen (e > 0), but the first one always takes the peak
    acc = assert_vector_equals_scalar(_one((0.0, 0.0, 0.0), (sub, 0.0, 1.0)), thr, "first wet sample")
    assert acc["e_peak"][0, 0] == sub and acc["t_peak"][0, 0] == 200.0
    # hs exactly equal to a threshold counts: e = 0.0625 -> hs = 1.0, e = 0.25 -> hs = 2.0; the next double below does not
    below = math.nextafter(0.25, 0.0)
    assert 4.0 * math.sqrt(below) < 2.0
    acc = assert_vector_equals_scalar(_one((0.0625, 0.1, 0.0), (0.25, 0.1, 0.0), (below, 0.1, 0.0)), thr, "hs == threshold")
    assert acc["n_exc"][0, 0].tolist() == [3, 1] and acc["n_wet"][0, 0] == 3
    # a continued accumulation (what picles_stat_set is for) equals the uninterrupted one
    s = hostile_samples(6, 4)
    a = SN.accumulate(s[3:], 7, thr, acc=SN.accumulate(s[:3], 7, thr))
    SN.assert_equal(a, SN.accumulate(s, 7, thr), 7, "continued")


def test_derived_variables_hand_values():
    acc = SN.accumulate(_one((4.0, 3.0, 4.0), (1.0, 1.0, 0.0), (0.0, 0.0, 0.0)), 7, (2.0, 8.0))
    d = derive(acc, G, RG)
    assert d["hs_max"][0, 0] == 8.0 and d["t_of_max"][0, 0] == 100.0 and d["dir_at_max"][0, 0] == math.atan2(4.0, 3.0)
    assert d["tp_at_max"][0, 0] == (FOUR_PI * max((4.0 / (2.0 * math.sqrt(25.0))) / RG, 0.1)) / G
    assert d["e_mean"][0, 0] == 2.5 and d["hs_mean"][0, 0] == (8.0 + 4.0) / 2.0 and d["mx_mean"][0, 0] == 2.0 and d["my_mean"][0, 0] == 2.0
    assert d["dir_mean"][0, 0] == math.atan2(4.0, 4.0)
    assert d["wet_fraction"][0, 0] == 2.0 / 3.0 and d["exceed_0"][0, 0] == 2.0 / 3.0 and d["exceed_1"][0, 0] == 1.0 / 3.0
    dry = derive(SN.accumulate(_one((0.0, 0.0, 0.0)), 7, (2.0, 8.0)), G, RG)
    for name in var_names(("peak", "mean", "exceed"), 2):
        v = dry[name][0, 0]
        assert (v == 0.0) if name in ("wet_fraction", "exceed_0", "exceed_1") else math.isnan(v), name
    none = derive(SN.zeros((2, 2), 7, (2.0, 8.0)), G, RG)           # no sample at all
    assert not none["wet_fraction"].any() and np.isnan(none["hs_max"]).all()


# ---- StatisticsWriter + run() over a backend that records its calls ----------------------------------------------------------------
def synthetic_state(Nx, Ny, s):
    """the State of the fake backend after its step s: e grows and falls with s differently at every node, column 0 is land"""
    i, j = np.meshgrid(np.arange(Nx), np.arange(Ny), indexing="ij")
    e = 0.0625 * (1.0 + ((3 * i + 5 * j + 7 * s) % 11))
    S = np.stack([e, 0.125 * e * np.cos(0.3 * s + i), -0.25 * e * np.sin(0.2 * s + j)], axis=-1)
    S[0] = 0.0
    return S


class StatBackend(FakeBackend):
    """FakeBackend + the statistics set: the accumulators are those of tests/_stats_numpy.py over synthetic_state"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.stat = None
        self.step = 0                  # model steps since the seed

    def stat_init(self, groups, thresholds=(), every=1, first=1):
        assert self.stat is None, "second stat_init without stat_free"
        mask = sum({"peak": 1, "mean": 2, "exceed": 4}[g] for g in groups)
        self.stat = dict(mask=mask, thr=tuple(thresholds), every=every, first=first, s=0, acc=SN.zeros((self.Nx, self.Ny), mask, thresholds))
        self.log.append(("stat_init", mask, tuple(thresholds), every, first))

    def stat_free(self):
        self.stat = None
        self.log.append(("stat_free",))

    def _stepped(self, dt, n):
        for _ in range(n):
            self.clock += dt
            self.step += 1
            p = self.stat
            if p is not None:
                p["s"] += 1
                if p["s"] >= p["first"] and (p["s"] - p["first"]) % p["every"] == 0:
                    SN.update(p["acc"], synthetic_state(self.Nx, self.Ny, self.step), self.clock, p["mask"], p["thr"])

    def run_steps(self, dt, n):
        self._stepped(dt, n)
        self.log.append(("run_steps", n))

    def time_step(self, dt, flags=0):
        self._stepped(dt, 1)
        self.log.append(("time_step", 1))

    def stat_get(self, groups=None):
        self.log.append(("stat_get", self.step))
        out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.stat["acc"].items()}
        out.update(thresholds=np.asarray(self.stat["thr"]), mask=self.stat["mask"])
        return out

    def stat_set(self, acc):
        self.log.append(("stat_set", int(acc["n_samples"])))
        for k in self.stat["acc"]:
            v = acc[k]
            self.stat["acc"][k] = v.copy() if isinstance(v, np.ndarray) else v

    def stat_reset(self):
        self.log.append(("stat_reset", self.step))
        self.stat["acc"] = SN.zeros((self.Nx, self.Ny), self.stat["mask"], self.stat["thr"])

    # a blob the checkpoint file reader accepts, with what this backend needs to go on
    def checkpoint_end(self):
        self.log.append(("checkpoint_end", self.clock))
        blob = np.zeros(K.CKPT_HEADER_BYTES + 16, dtype=np.uint8)
        blob[:8] = np.frombuffer(struct.pack("<Q", K.CKPT_MAGIC), dtype=np.uint8)
        blob[-16:] = np.frombuffer(struct.pack("<dq", self._ck[0], self._ck[1]), dtype=np.uint8)
        return blob

    def checkpoint_begin(self):
        self._ck = (self.clock, self.step)
        self.log.append(("checkpoint_begin", self.clock))

    def checkpoint_load(self, blob):
        self.clock, self.step = struct.unpack("<dq", bytes(blob[-16:]))
        self.log.append(("checkpoint_load", self.step))


def _fake_sim(n_steps, n=12):
    cfg = configs.bench06_box(n=n)
    m = models.WaveGrowth2D(**cfg.model, backend_factory=StatBackend)
    return m, Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1)), cfg.Δt


def _expected(n, dt, steps, thr, mask=7):
    return SN.accumulate([(synthetic_state(n, n, s), s * dt) for s in steps], mask, thr)


def _check_record(out, k, acc, names):
    d = derive(acc, G, RG)
    for name in names:
        a, b = np.ascontiguousarray(variable(out, name)[:, :, k]), np.ascontiguousarray(d[name].T)
        assert a.tobytes() == b.tobytes(), (k, name)


@pytest.mark.parametrize("fmt", ["npy", "hdf5"])
def test_windows_reset_chunks_and_the_file_round_trip(tmp_path, fmt):
    if fmt == "hdf5":
        from picles_amd import storing
        try:
            storing.hdf5()
        except OSError:
            pytest.skip("no libhdf5 on this machine")
    thr = (0.25, 0.5)
    m, sim, dt = _fake_sim(23)
    w = sim.output_writers["statistics"] = StatisticsWriter(m, thresholds=thr, schedule=1, window=5, path=tmp_path, format=fmt)
    sim.output_writers["fields"] = FieldWriter(m, schedule=4, path=tmp_path, format="npy")
    run(sim)
    log = m.backend.log
    assert all(c[0] != "time_step" for c in log) and sum(c[1] for c in log if c[0] == "run_steps") == 23
    ends = np.cumsum([c[1] for c in log if c[0] == "run_steps"]).tolist()
    assert ends == sorted(set(range(5, 24, 5)) | set(range(4, 24, 4)) | {23})          # chunks end on windows and field outputs only
    assert [c for c in log if c[0] == "stat_init"] == [("stat_init", 7, thr, 1, 1)]
    assert [c[1] for c in log if c[0] == "stat_get"] == [5, 10, 15, 20, 23] == [c[1] for c in log if c[0] == "stat_reset"]
    assert log[-1] == ("stat_free",) or ("stat_free",) in log
    out = read_statistics(tmp_path)
    names = var_names(("peak", "mean", "exceed"), 2)
    assert list(out["names"]) == list(names) and out["data"].shape == (len(names), 12, 12, 5) and out["data"].dtype == np.float64
    assert out["thresholds"].tolist() == list(thr) and out["iteration"].tolist() == [5.0, 10.0, 15.0, 20.0, 23.0]
    assert out["t_start"].tolist() == [dt * k for k in (1, 6, 11, 16, 21)] and out["t_end"].tolist() == [dt * k for k in (5, 10, 15, 20, 23)]
    assert out["n_samples"].tolist() == [5.0, 5.0, 5.0, 5.0, 3.0]
    assert out["x"].tolist() == m.grid.data.x[:, 0].tolist() and out["y"].tolist() == m.grid.data.y[0, :].tolist()
    for k, (a, b) in enumerate(((1, 5), (6, 10), (11, 15), (16, 20), (21, 23))):
        _check_record(out, k, _expected(12, dt, range(a, b + 1), thr), names)
    hs = variable(out, "hs_max")
    assert np.isnan(hs[:, 0, :]).all() and np.isfinite(hs[:, 1:, :]).all()                  # column 0 is land: (y, x, window)
    assert (variable(out, "wet_fraction")[:, 0, :] == 0.0).all() and (variable(out, "wet_fraction")[:, 1:, :] == 1.0).all()


def test_one_record_at_the_end_and_a_sampling_cadence(tmp_path):
    m, sim, dt = _fake_sim(17)
    sim.output_writers["statistics"] = StatisticsWriter(m, fields=("mean", "peak"), schedule=3, path=tmp_path, format="npy")
    run(sim)
    log = m.backend.log
    assert [c for c in log if c[0] == "run_steps"] == [("run_steps", 17)]                       # nothing ends a chunk
    assert [c for c in log if c[0] == "stat_init"] == [("stat_init", 3, (), 3, 3)]
    out = read_statistics(tmp_path)
    names = var_names(("peak", "mean"), 0)
    assert list(out["names"]) == list(names) == ["hs_max", "tp_at_max", "dir_at_max", "t_of_max", "e_mean", "hs_mean", "mx_mean", "my_mean",
                                                  "dir_mean", "wet_fraction"]
    assert out["data"].shape[-1] == 1 and out["n_samples"].tolist() == [5.0] and out["thresholds"].size == 0
    _check_record(out, 0, _expected(12, dt, (3, 6, 9, 12, 15), (), mask=3), names)
    # the per-step loop (cash_store observes State after every step): the library updates inside time_step
    m2, sim2, _ = _fake_sim(9)
    m2.backend.get_state = lambda: np.zeros((12, 12, 3))
    m2.backend.state_gen = 0
    sim2.output_writers["statistics"] = StatisticsWriter(m2, fields="peak", window=4, path=tmp_path / "loop", format="npy")
    run(sim2, cash_store=True)
    assert [c[0] for c in m2.backend.log if c[0] in ("time_step", "run_steps")] == ["time_step"] * 9
    out2 = read_statistics(tmp_path / "loop")
    assert out2["iteration"].tolist() == [4.0, 8.0, 9.0] and out2["n_samples"].tolist() == [4.0, 4.0, 1.0]
    _check_record(out2, 1, _expected(12, dt, range(5, 9), (), mask=1), var_names(("peak",), 0))


def test_sidecar_and_pickup_of_an_open_window(tmp_path):
    thr = (0.25,)
    kw = dict(fields=("peak", "mean", "exceed"), thresholds=thr, schedule=1, window=10, format="npy")
    # the uninterrupted run
    m0, sim0, dt = _fake_sim(24)
    sim0.output_writers["statistics"] = StatisticsWriter(m0, path=tmp_path / "whole", **kw)
    run(sim0)
    whole = read_statistics(tmp_path / "whole")
    # the same run stopped after 17 steps with a checkpoint every 7 ...
    m1, sim1, _ = _fake_sim(17)
    sim1.output_writers["checkpointer"] = Checkpointer(m1, schedule=7, dir=tmp_path / "ck")
    sim1.output_writers["statistics"] = StatisticsWriter(m1, path=tmp_path / "first", **kw)
    run(sim1)
    side = sorted(p.name for p in (tmp_path / "ck").iterdir())
    assert side == ["checkpoint_iteration14.picles", "checkpoint_iteration14.picles.stats.npz", "checkpoint_iteration7.picles",
                    "checkpoint_iteration7.picles.stats.npz"]
    with np.load(tmp_path / "ck" / "checkpoint_iteration14.picles.stats.npz") as z:
        assert int(z["n_samples"]) == 4 and float(z["t_first"]) == 11 * dt and z["e_peak"].shape == (12, 12)
    # ... and picked up from iteration 14: the open window (iterations 11 ... 20) continues
    m2, sim2, _ = _fake_sim(24)
    sim2.output_writers["checkpointer"] = Checkpointer(m2, schedule=7, dir=tmp_path / "ck")
    sim2.output_writers["statistics"] = StatisticsWriter(m2, path=tmp_path / "second", **kw)
    run(sim2, pickup=True)
    log = m2.backend.log
    assert ("checkpoint_load", 14) in log and ("stat_set", 4) in log
    assert [c for c in log if c[0] == "stat_init"] == [("stat_init", 7, thr, 1, 1)]
    assert log.index(("stat_set", 4)) > [k for k, c in enumerate(log) if c[0] == "stat_init"][0]
    second = read_statistics(tmp_path / "second")
    assert second["iteration"].tolist() == [20.0, 24.0] and second["n_samples"].tolist() == [10.0, 4.0]
    assert second["t_start"].tolist() == [11 * dt, 21 * dt]
    assert second["data"].tobytes() == whole["data"][..., 1:].tobytes()
    # a missing side-car: a fresh window, with a warning
    (tmp_path / "ck" / "checkpoint_iteration14.picles.stats.npz").unlink()
    m3, sim3, _ = _fake_sim(24)
    sim3.output_writers["checkpointer"] = Checkpointer(m3, schedule=7, dir=tmp_path / "ck2")
    sim3.output_writers["statistics"] = StatisticsWriter(m3, path=tmp_path / "third", **kw)
    with pytest.warns(UserWarning, match="starts afresh"):
        run(sim3, pickup=tmp_path / "ck" / "checkpoint_iteration14.picles")
    assert not [c for c in m3.backend.log if c[0] == "stat_set"]
    third = read_statistics(tmp_path / "third")
    assert third["iteration"].tolist() == [20.0, 24.0] and third["n_samples"].tolist() == [6.0, 4.0] and third["t_start"][0] == 15 * dt
    # a side-car written with other thresholds is not uploaded either
    m4, sim4, _ = _fake_sim(24)
    sim4.output_writers["statistics"] = StatisticsWriter(m4, path=tmp_path / "fourth", **dict(kw, thresholds=(0.5,)))
    with pytest.warns(UserWarning, match="other fields, thresholds or schedule"):
        run(sim4, pickup=tmp_path / "ck" / "checkpoint_iteration7.picles")
    assert not [c for c in m4.backend.log if c[0] == "stat_set"]


def test_bad_arguments_are_refused_before_the_library_is_reached(tmp_path):
    m, sim, dt = _fake_sim(3)
    for kw, text in ((dict(fields=()), "non-empty selection"), (dict(fields=("peak", "median")), "non-empty selection"),
                     (dict(fields=("exceed",)), "1 ... 4 thresholds"), (dict(thresholds=(1, 2, 3, 4, 5)), "1 ... 4 thresholds"),
                     (dict(thresholds=(1.0, 1.0)), "strictly ascending"), (dict(thresholds=(2.0, 1.0)), "strictly ascending"),
                     (dict(thresholds=(0.0, 1.0)), "strictly ascending"), (dict(thresholds=(-1.0,)), "strictly ascending"),
                     (dict(thresholds=(1.0, math.inf)), "strictly ascending"), (dict(thresholds=(math.nan,)), "strictly ascending"),
                     (dict(fields=("peak",), thresholds=(1.0,)), "without 'exceed'"),
                     (dict(fields="mean", schedule=0), "interval >= 1"), (dict(fields="mean", window=0), "interval >= 1"),
                     (dict(fields="mean", format="netcdf"), "unknown statistics output format")):
        with pytest.raises(ValueError, match=text):
            StatisticsWriter(m, path=tmp_path, **kw)
    assert m.backend.log == [] or all(c[0] not in ("stat_init",) for c in m.backend.log)
    assert check_arguments(("exceed", "peak"), (1, 2), 2, None)[:2] == (("peak", "exceed"), (1.0, 2.0))
    # the driver layer refuses unknown groups before the library is reached, too
    from picles_amd.driver import stat_layout, stat_mask, stat_pack, stat_unpack
    with pytest.raises(ValueError, match="unknown statistics groups"):
        stat_mask(("peak", "median"))
    for bad in (0, 8, -1):
        with pytest.raises(ValueError, match="empty or unknown"):
            stat_mask(bad)
    assert stat_mask(("exceed", "peak")) == 5 and stat_mask(0, allow_empty=True) == 0
    # the plane block: pack and unpack are inverse, the fp64 planes first
    lay = stat_layout(7, 2)
    assert [n for n, _, _ in lay] == list(SN.PEAK_PLANES + SN.MEAN_PLANES) + ["n_wet", "n_exc"]
    acc = SN.accumulate(hostile_samples(6, 4), 7, (0.5, 1.0))
    buf = stat_pack(acc, lay, 6, 4)
    assert buf.size == 6 * 4 * (64 + 4 + 8)
    assert buf[:6 * 4 * 8].tobytes() == np.ascontiguousarray(acc["e_peak"].reshape(-1, order="F")).tobytes()
    back = stat_unpack(buf, lay, 6, 4)
    back.update(n_samples=acc["n_samples"], t_first=acc["t_first"], t_last=acc["t_last"])
    SN.assert_equal(back, acc, 7, "pack / unpack")
    # a backend without the entry points
    from helpers import make_model
    cfg = configs.example_00_minimal(n=9, L=16e3)
    mo = make_model(cfg, ("pmath", 1))
    s2 = Simulation(mo, Δt=cfg.Δt, stop_time=cfg.Δt)
    s2.output_writers["statistics"] = StatisticsWriter(mo, fields="peak", path=tmp_path)
    with pytest.raises(NotImplementedError, match="StatisticsWriter needs a backend"):
        run(s2)
