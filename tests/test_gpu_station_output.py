"""StationWriter through run() on the GPU: the station file equals the NumPy restatement (tests/_station_numpy.py) applied to
the per-step State of a twin that is observed after every step — bit for bit, raw and derived variables —, alone and together
with a Checkpointer and a FieldWriter of co-prime schedules, whose files do not change by the writer's presence; a run stopped
and picked up continues the series."""
import numpy as np
import pytest

import _station_numpy as R
from picles_amd import configs
from picles_amd.checkpointing import Checkpointer
from picles_amd.field_output import FieldWriter, read_field_output
from picles_amd.simulations import Simulation, initialize_simulation, run
from picles_amd.station_output import StationWriter, read_station_output
from picles_amd.timesteppers import time_step
from helpers import assert_bitwise, make_model

pytestmark = pytest.mark.gpu


def _make():
    return configs.bench06_box(n=48, winds=configs.smooth_winds(10.0, 7.0, 96e3, 96e3))


def _phys(cfg):
    P = cfg.model["ODEsets"].Parameters
    return P.get("g", 9.81), P["r_g"]


def _twin_states(n):
    """State at iteration 0 ... n of the observed twin"""
    cfg = _make()
    m = make_model(cfg, "hip")
    initialize_simulation(Simulation(m, Δt=cfg.Δt, stop_time=1.0))
    out = [m.backend.get_state()]
    for _ in range(n):
        time_step(m, cfg.Δt, zero_first=True)
        out.append(m.backend.get_state())
    return out


def _points(cfg):
    x = cfg.model["grid"].data.x[:, 0]
    rng = np.random.default_rng(5)
    pts = [(float(rng.uniform(x[0], x[-1] + 1999.0)), float(rng.uniform(x[0], x[-1] + 1999.0))) for _ in range(30)]
    return pts + [(float(x[7]), float(x[9])), (float(x[-1]) + 1000.0, float(x[-1]) + 500.0)]       # a node; the wrap cell


def _stations_of(cfg, pts):
    g = cfg.model["grid"]
    return [R.corners_of(p, g.data.x[:, 0], g.data.y[0, :], periodic=(True, True)) for p in pts]


def test_station_writer_alone_points_and_nodes(tmp_path):
    n = 12
    S = _twin_states(n)
    for kind in ("points", "nodes"):
        cfg = _make()
        m = make_model(cfg, "hip")
        sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n - 1))
        if kind == "points":
            pts = _points(cfg)
            sw = StationWriter(m, points=pts, schedule=1, path=tmp_path / kind, capacity=6)
            stations = _stations_of(cfg, pts)
        else:
            rng = np.random.default_rng(9)
            nodes = [(int(rng.integers(48)), int(rng.integers(48))) for _ in range(40)]
            sw = StationWriter(m, nodes=nodes, schedule=1, path=tmp_path / kind, capacity=6)
            stations = [[(ij, 1.0)] for ij in nodes]
        sim.output_writers["stations"] = sw
        m.backend.enable_timing(True)
        run(sim)
        t = m.backend.get_timing()
        assert t["advance_launches"] == n and t["scatter_launches"] <= 1, t              # the fused path is kept
        out = read_station_output(tmp_path / kind)
        assert out["iteration"].tolist() == list(range(n + 1)) and out["time"].tolist() == [k * cfg.Δt for k in range(n + 1)]
        want = R.series_from_states(S, stations, *_phys(cfg))
        assert_bitwise(out["data"], want, f"{kind}: station file vs the restatement on the twin's State")
        if kind == "nodes":
            raw = np.stack([np.stack([Sk[i, j, :] for (i, j) in nodes]) for Sk in S])
            assert_bitwise(out["data"][:, :, :3], raw, "nodes=: raw e, m_x, m_y")
        wet = float(np.isfinite(out["data"][-1, :, 0]).mean())
        print(f"{kind}: share of valid stations at the last record {wet:.3f}")
        assert wet >= 0.5


def test_with_checkpointer_and_field_writer_and_their_files_unchanged(tmp_path):
    n = 30
    S = _twin_states(n)
    files = {}
    for with_sw in (False, True):
        cfg = _make()
        m = make_model(cfg, "hip")
        sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n - 1))
        d = tmp_path / ("with" if with_sw else "without")
        sim.output_writers["checkpointer"] = Checkpointer(m, schedule=7, dir=d / "ck")
        sim.output_writers["fields"] = FieldWriter(m, schedule=5, path=d, coarsen=(4, 4), format="npy")
        if with_sw:
            pts = _points(cfg)
            sim.output_writers["stations"] = StationWriter(m, points=pts, schedule=1, path=d, capacity=5, format="npy")
        run(sim)
        f = read_field_output(d)
        files[with_sw] = (f["data"], f["scalars"], {p.name: p.read_bytes() for p in sorted((d / "ck").glob("*.picles"))}, m.backend.get_state())
        if with_sw:
            out = read_station_output(d)
            assert out["iteration"].tolist() == list(range(n + 1))
            assert_bitwise(out["data"], R.series_from_states(S, _stations_of(cfg, pts), *_phys(cfg)), "station file beside the other writers")
    a, b = files[False], files[True]
    assert_bitwise(a[0], b[0], "field planes"); assert_bitwise(a[1], b[1], "field scalars"); assert_bitwise(a[3], b[3], "final State")
    assert list(a[2]) == list(b[2]) and len(a[2]) == 4 and all(a[2][k] == b[2][k] for k in a[2]), "checkpoint files changed"


def test_stopped_and_picked_up_run_continues_the_series(tmp_path):
    sched = 3
    def sim_of(d, stop_it):
        cfg = _make()
        m = make_model(cfg, "hip")
        sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (stop_it - 1))
        sim.output_writers["checkpointer"] = Checkpointer(m, schedule=10, dir=tmp_path / d / "ck")
        sim.output_writers["stations"] = StationWriter(m, points=_points(cfg), schedule=sched, path=tmp_path / d, capacity=4, format="npy")
        return cfg, m, sim
    cfg, m, sim = sim_of("whole", 25)
    run(sim)
    whole = read_station_output(tmp_path / "whole")
    assert whole["iteration"].tolist() == [0] + list(range(3, 26, 3))
    cfg, m, sim = sim_of("parts", 10)
    run(sim)                                              # stops at iteration 10: not a multiple of the schedule
    first = read_station_output(tmp_path / "parts")
    assert first["iteration"].tolist() == [0, 3, 6, 9]
    cfg, m2, sim2 = sim_of("parts2", 25)
    sim2.output_writers["checkpointer"] = Checkpointer(m2, schedule=10, dir=tmp_path / "parts" / "ck")
    run(sim2, pickup=True)
    assert m2.clock.iteration == 25
    second = read_station_output(tmp_path / "parts2")
    assert second["iteration"].tolist() == [10, 12, 15, 18, 21, 24]       # the restored state's record, then the cadence continued
    keep = second["iteration"] > 10
    assert_bitwise(np.concatenate([first["data"], second["data"][keep]]), whole["data"], "stopped + picked up vs uninterrupted")
    assert np.concatenate([first["time"], second["time"][keep]]).tolist() == whole["time"].tolist()
