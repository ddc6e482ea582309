"""TrackWriter on the GPU (picles_amd/track_output.py): `run(sim)` with the writer attached gives, event by event and bit for bit, the
records of the NumPy restatement (tests/_track_numpy.py) fed from a second run's get_state() after every step; the other writers'
files do not notice it; a picked-up run is NaN before the restored clock and the straight run from there.  Grid (K) of
tests/test_gpu_track.py — 70 x 9, open, a 10 x 3 land block —, twelve steps."""
import json

import numpy as np
import pytest

import _track_numpy as TN
from picles_amd import _capi as K
from picles_amd.checkpointing import Checkpointer
from picles_amd.field_output import FieldWriter
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter, VAR_NAMES, locate_points
from picles_amd.track_output import TrackWriter, read_track_output
from helpers import assert_bitwise, make_model
from test_gpu_track import GRIDS

pytestmark = pytest.mark.gpu

N = 12
_REF = {}


def _reference():
    """once: the events in the caller's order, and the records the host route gives for them, [var, event]"""
    if _REF:
        return _REF
    cfg = GRIDS["K70x9"]()
    a = make_model(cfg, "hip")
    initialize_simulation(Simulation(a, Δt=cfg.Δt, stop_time=1.0))
    a.upload_winds(a.clock.time, cfg.Δt)
    b = a.backend
    samples = [(b.clock, b.get_state())]
    for _ in range(N):
        b.time_step(cfg.Δt, K.STEP_ZERO_FIRST)
        samples.append((b.clock, b.get_state()))
    wets = [np.isfinite(S).all(axis=-1) & (S[..., 0] > 0) & (S[..., 1] ** 2 + S[..., 2] ** 2 > 0) for _, S in samples]
    t, p = TN.make_events(a.grid, False, [c for c, _ in samples], cfg.Δt, seed=77, wet=np.logical_and.reduce(wets), never=~(wets[1] | wets[2]))
    order = np.argsort(t, kind="stable")
    corners, weights = locate_points(a.grid, [tuple(q) for q in p[order]])
    P = a.ODEsettings.Parameters
    g, r_g = P.get("g", 9.81), P["r_g"]

    def records(first=0):
        tab = TN.Table(t[order], corners, weights, cfg.Δt)
        for T, S in samples[first:]:
            tab.sample(T, S)
        rec = np.empty((len(t), 8))
        rec[order] = TN.records(tab.tab, t[order], g, r_g)
        tb, ta = np.empty(len(t)), np.empty(len(t))
        tb[order], ta[order] = tab.tab[3], tab.tab[7]
        return rec.T, tb, ta
    _REF.update(cfg=cfg, t=t, p=p, samples=samples, records=records)
    return _REF


def _sim(tmp, n_steps=N, tracks=None, others=False, ckpt=None):
    R = _reference()
    cfg = GRIDS["K70x9"]()
    m = make_model(cfg, "hip")
    sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1))
    if others:
        x, y = m.grid.data.x[:, 0], m.grid.data.y[0, :]
        sim.output_writers["fields"] = FieldWriter(m, schedule=4, path=tmp, coarsen=(2, 2), format="npy")
        sim.output_writers["stations"] = StationWriter(m, points=[(x[3] + 300.0, y[2] + 100.0), (x[29] + 1500.0, y[3] + 900.0), (x[60], y[7])],
                                                       schedule=1, path=tmp, capacity=8, format="npy")
    if ckpt is not None:
        sim.output_writers["checkpointer"] = Checkpointer(m, schedule=6, dir=ckpt)
    if tracks:
        sim.output_writers["tracks"] = TrackWriter(m, times=R["t"], points=R["p"], path=tmp, format=tracks)
    return m, sim


@pytest.mark.parametrize("fmt", ["npy", "hdf5"])
def test_file_equals_the_numpy_restatement_of_a_second_run(tmp_path, fmt):
    if fmt == "hdf5":
        from picles_amd import storing
        try:
            storing.hdf5()
        except OSError:
            pytest.skip("no libhdf5 on this machine")
    R = _reference()
    m, sim = _sim(tmp_path, tracks=fmt)
    m.backend.enable_timing(True)
    run(sim)
    timing = m.backend.get_timing()
    # the run stayed fused: twelve step launches, and no sample completed a step (the one scatter allowed is the one that run()'s
    # closing sync, or get_timing, launches; that a fetch completes none: tests/test_gpu_track.py, the fetch test)
    assert timing["advance_launches"] == N and timing["scatter_launches"] <= 1, timing
    out = read_track_output(tmp_path)
    want, tb, ta = R["records"]()
    valid = int(np.isfinite(want).all(axis=0).sum())
    print(f"{fmt}: {len(R['t'])} events, {valid} with a record, {int(np.isnan(want).all(axis=0).sum())} NaN")
    assert valid >= 150 and np.isnan(want).all(axis=0).sum() >= 10
    assert list(out["var_names"]) == list(VAR_NAMES) and out["data"].shape == (8, len(R["t"]))
    assert_bitwise(out["data"], want, "records, (var, event) in the caller's order")
    assert_bitwise(out["t_before"], tb, "t_before")
    assert_bitwise(out["t_after"], ta, "t_after")
    assert_bitwise(out["time"], R["t"], "time")
    assert_bitwise(np.stack([out["x"], out["y"]], axis=1), R["p"], "x, y")
    assert m.clock.iteration == N
    assert_bitwise(m.backend.get_state(), R["samples"][N][1], "State at the end of the run")
    with pytest.raises(K.PiclesError, match="track_init first"):
        m.backend.track_info()          # finish freed the set


def test_other_writers_files_do_not_notice_the_track_writer(tmp_path):
    R = _reference()
    for sub, tracks in (("without", None), ("with", "npy")):
        _, sim = _sim(tmp_path / sub, tracks=tracks, others=True)
        run(sim)
    names = sorted(f.name for f in (tmp_path / "without").iterdir())
    assert len(names) >= 4 and any("stations" in n for n in names) and any("fields" in n for n in names), names
    for n in names:
        a, b = (tmp_path / "without" / n), (tmp_path / "with" / n)
        if n.endswith(".json"):
            assert json.loads(a.read_text()) == json.loads(b.read_text()) or a.read_text() == b.read_text(), n
        else:
            assert a.read_bytes() == b.read_bytes(), n
    assert_bitwise(read_track_output(tmp_path / "with")["data"], R["records"]()[0], "the track file beside the other writers")


def test_pickup_is_nan_before_the_restored_clock_and_the_straight_run_from_there(tmp_path):
    R = _reference()
    _, first = _sim(tmp_path / "first", n_steps=6, tracks="npy", ckpt=tmp_path / "ck")
    run(first)
    m, sim = _sim(tmp_path / "second", tracks="npy", ckpt=tmp_path / "ck")
    run(sim, pickup=True)
    assert m.clock.iteration == N
    out = read_track_output(tmp_path / "second")
    straight = R["records"]()[0]
    T6 = R["samples"][6][0]
    late = R["t"] >= T6
    assert np.isnan(out["data"][:, ~late]).all() and (~late).sum() >= 50
    assert_bitwise(out["data"][:, late], straight[:, late], "events from the restored clock on")
    assert np.isfinite(out["data"][:, late]).all(axis=0).sum() >= 40
    assert_bitwise(out["data"], R["records"](first=6)[0], "the restatement fed from the restored clock on")
