"""run() with several output products attached at once, against a recording: what the backend is asked for, call by call, and
what lands in the files.  tests/golden/run_call_sequences.json was recorded with this file's `--record` from the tree BEFORE
run()'s writers were put behind one protocol; the comparison is equality — the log entry by entry, the files by
their hashes, JSON as parsed objects, arrays bitwise.

Per case the fixture holds `log` (the backend's whole call log) and `files`: for every `.npy` and `.picles` file the sha256 of
its bytes, for every `.json` file its parsed content, for every `.npz` file its loaded arrays (the scalars and short vectors as
values, and one sha256 over every array's name, dtype, shape and bytes — an `.npz` itself is a zip archive and carries times).

    python tests/test_run_call_sequence.py --record        # writes the fixture anew: only ever from a tree known to be right
"""
import hashlib
import itertools
import json
import sys
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden" / "run_call_sequences.json"
KINDS = ("checkpointer", "fields", "stations", "statistics")
STEPS = 23


def _sim(n_steps, n=12):
    from _recording_backend import RecordingBackend
    from picles_amd import configs, models
    from picles_amd.simulations import Simulation
    cfg = configs.bench06_box(n=n)
    m = models.WaveGrowth2D(**cfg.model, backend_factory=RecordingBackend)
    return m, Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * (n_steps - 1)), cfg.Δt


def _attach(sim, kinds, d):
    from picles_amd.checkpointing import Checkpointer
    from picles_amd.field_output import FieldWriter
    from picles_amd.run_statistics import StatisticsWriter
    from picles_amd.station_output import StationWriter
    m = sim.model
    make = {"checkpointer": lambda: Checkpointer(m, schedule=7, dir=d / "ck"),
            "fields": lambda: FieldWriter(m, schedule=5, path=d / "fields", slots=2, format="npy"),
            "stations": lambda: StationWriter(m, nodes=[(1, 2), (3, 4)], schedule=1, path=d / "stations", capacity=3, format="npy"),
            "statistics": lambda: StatisticsWriter(m, thresholds=(0.25,), window=10, path=d / "statistics", format="npy")}
    for k in KINDS:                 # attached in one order; run() visits by kind, not by the dict's order
        if k in kinds:
            sim.output_writers[k] = make[k]()


def _arrays(z):
    """the arrays of an .npz: the scalars and short vectors as values, and one sha256 over every array's name, dtype, shape and bytes"""
    h = hashlib.sha256()
    small = {}
    for k in sorted(z.files):
        a = np.ascontiguousarray(z[k])
        h.update(f"{k}|{a.dtype}|{a.shape}|".encode())
        h.update(a.tobytes())
        if a.size <= 4:
            small[k] = a.reshape(-1).tolist()
    return {"values": small, "sha256": h.hexdigest()}


def _files(d):
    out = {}
    for p in sorted(q for q in d.rglob("*") if q.is_file()):
        key = p.relative_to(d).as_posix()
        if p.suffix in (".npy", ".picles"):
            out[key] = hashlib.sha256(p.read_bytes()).hexdigest()
        elif p.suffix == ".json":
            out[key] = json.loads(p.read_text())
        elif p.suffix == ".npz":
            with np.load(p) as z:
                out[key] = _arrays(z)
        else:
            raise AssertionError(f"a file of a kind the fixture does not hold: {key}")
    return out


def _result(d, *models):
    from _recording_backend import jsonable
    logs = [jsonable(m.backend.log) for m in models]
    return {"log": logs[0] if len(logs) == 1 else logs, "files": _files(d)}


def _subset(kinds, per_step):
    def case(d):
        from picles_amd.simulations import run
        m, sim, dt = _sim(STEPS)
        _attach(sim, kinds, d)
        run(sim, cash_store=per_step)
        return _result(d, m)
    return case


def _pickup(d):
    """17 steps with a checkpoint every 7, then run(sim, pickup=True) from iteration 14 in a model of its own"""
    from picles_amd.simulations import run
    m1, sim1, dt = _sim(17)
    _attach(sim1, ("checkpointer", "statistics"), d / "first")
    run(sim1)
    m2, sim2, _ = _sim(24)
    _attach(sim2, ("checkpointer", "statistics"), d / "second")
    sim2.output_writers["checkpointer"].dir = sim1.output_writers["checkpointer"].dir
    run(sim2, pickup=True)
    return _result(d, m1, m2)


def _second_run(d):
    """a second run() of the same simulation: the probe and statistics sets are freed and made again, the diag ring stays"""
    from picles_amd.simulations import run
    m, sim, dt = _sim(STEPS)
    _attach(sim, KINDS, d)
    run(sim)
    sim.stop_time = dt * 30
    run(sim)
    return _result(d, m)


def _store(kinds):
    def case(d):
        from picles_amd.simulations import init_state_store, run
        m, sim, dt = _sim(STEPS)
        _attach(sim, kinds, d)
        init_state_store(sim, d / "store", format="npy")
        run(sim, store=True)
        return _result(d, m)
    return case


CASES = {}
for _r in range(len(KINDS) + 1):
    for _kinds in itertools.combinations(KINDS, _r):
        for _per_step in (False, True):
            CASES["+".join(_kinds or ("none",)) + ("/per-step" if _per_step else "/fast")] = _subset(_kinds, _per_step)
CASES["pickup"] = _pickup
CASES["second-run"] = _second_run
CASES["store"] = _store(())
CASES["store+all"] = _store(KINDS)


def _canonical(obj):
    return json.dumps(obj, sort_keys=True)          # NaN compares equal to NaN this way


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_fixture_holds_these_cases_and_no_others(golden):
    assert sorted(golden) == sorted(CASES) and len(CASES) == 36


@pytest.mark.parametrize("name", list(CASES))
def test_calls_and_files_equal_the_recording(name, tmp_path, golden):
    got = json.loads(json.dumps(CASES[name](tmp_path)))          # as the fixture went through JSON
    want = golden[name]
    logs = [(got["log"], want["log"])] if name != "pickup" else list(zip(got["log"], want["log"]))
    for g, w in logs:
        for k, (a, b) in enumerate(zip(g, w)):
            assert a == b, f"{name}: call {k} is {a}, the recording has {b} (after {g[max(0, k - 3):k]})"
        assert len(g) == len(w), f"{name}: {len(g)} calls, the recording has {len(w)}"
    assert sorted(got["files"]) == sorted(want["files"])
    for key, w in want["files"].items():
        assert _canonical(got["files"][key]) == _canonical(w), f"{name}: {key} differs from the recording"


def test_a_refused_run_has_asked_the_backend_for_nothing(tmp_path):
    """every writer's backend check comes before pickup and seeding: a refused run leaves the model as it was"""
    from picles_amd import configs, models
    from picles_amd.simulations import Simulation, run
    from picles_amd.station_output import StationWriter
    from test_field_output_host import FakeBackend
    cfg = configs.bench06_box(n=12)
    m = models.WaveGrowth2D(**cfg.model, backend_factory=FakeBackend)          # no probe ring
    sim = Simulation(m, Δt=cfg.Δt, stop_time=cfg.Δt * 3)
    sim.output_writers["stations"] = StationWriter(m, nodes=[(1, 2)], path=tmp_path, format="npy")
    with pytest.raises(NotImplementedError, match="a StationWriter needs a backend with probe_init / probe_sample / probe_pop"):
        run(sim)
    assert m.backend.log == [] and not sim.initialized and m.clock.iteration == 0 and not list(tmp_path.iterdir())


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        raise SystemExit(__doc__)
    import tempfile
    sys.path[:0] = [str(Path(__file__).resolve().parent.parent), str(Path(__file__).resolve().parent)]
    rec = {}
    for name, case in CASES.items():
        with tempfile.TemporaryDirectory() as t:
            rec[name] = case(Path(t))
    GOLDEN.write_text(json.dumps(rec, sort_keys=True, separators=(",", ":")) + "\n")
    print(f"{len(rec)} cases, {GOLDEN.stat().st_size} bytes -> {GOLDEN}")
