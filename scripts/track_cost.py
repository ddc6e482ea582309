"""Cost of track output.  The 4096^2 periodic box (DP5, winds (10, 10), dx = 2000 m, Δt = 600 s), with two passes
of 1,200 events in every step — 2,400 events per step, evenly spaced in time, one pass along a diagonal of the box and one along an
anti-diagonal, each step's pair shifted in x against the last as an orbit's ground track is —, against the same box without a set.
Four alternated rounds of 20 steps after un-timed conditioning steps; round 0 is dropped.  Two figures per round: the device time
inside one event pair (picles_enable_timing(2): the launches of a picles_run_steps call back to back, the track samples among
them), and the host wall time of the round with the writer's fetch behind it — fetch_end of the range begun a round earlier, then
fetch_begin of the events the round completed: eight device-to-device copies on the context stream and one copy to the host, which
the event pair does not see — and a synchronisation (so the copy to the host is waited for here, where the writer overlaps it).
One JSON line on stdout, with the figure for the same events served as fixed stations: the number of distinct corner nodes and the
memory a probe ring of them would take.
--profile: a short run with a set and nothing else, for `rocprofv3 --kernel-trace --stats -- python scripts/track_cost.py --profile`."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from picles_amd import configs, models
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.track_output import locate_points_fast

N, DT = 4096, 600.0
PER_PASS, STEPS, WARM, ROUNDS = 1200, 20, 5, 4
profile = "--profile" in sys.argv
n_steps = WARM + (10 if profile else (ROUNDS + 1) * STEPS)


def box():
    cfg = configs.box4096(n=N)
    m = models.WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=DT, stop_time=1.0))
    m.upload_winds(m.clock.time, DT)
    return m


with_set = box()
x = np.asarray(with_set.grid.data.x)[:, 0]
L = float(x[-1] - x[0]) + float(x[1] - x[0])          # the periodic box's length
k = np.arange(n_steps * PER_PASS)
frac = (k % PER_PASS + 0.5) / PER_PASS                  # a pass crosses the box in one step
shift = (0.37 * (k // PER_PASS)) % 1.0                  # ... and the next one lies elsewhere
t1 = (k + 0.25) * (DT / PER_PASS)
t2 = (k + 0.75) * (DT / PER_PASS)
times = np.concatenate([t1, t2])
px = x[0] + ((frac + shift) % 1.0) * L * 0.999
points = np.concatenate([np.stack([px, x[0] + frac * L * 0.999], axis=1), np.stack([px, x[0] + (1.0 - frac) * L * 0.999], axis=1)])
order = np.argsort(times, kind="stable")
corners, weights = locate_points_fast(with_set.grid, points[order])
ij = np.ascontiguousarray(np.concatenate([corners[:, :, 0].T, corners[:, :, 1].T], axis=0))
b = with_set.backend
b.track_init(times[order], ij, np.ascontiguousarray(weights.T), DT)
b.track_sample()
if profile:
    b.run_steps(DT, n_steps)
    b.sync()
    sys.exit(0)

without = box()
a = without.backend
for q in (a, b):
    q.run_steps(DT, WARM)
    q.enable_timing(2)


sorted_times = times[order]
fetch = {"begun": 0, "fetched": 0, "ranges": []}


def turn(q):
    """TrackWriter's turn behind a chunk: end the fetch begun a chunk earlier, begin the one of the events completed since"""
    if fetch["begun"] > fetch["fetched"]:
        q.track_fetch_end()
        fetch["fetched"] = fetch["begun"]
    done = int(np.searchsorted(sorted_times, q.clock, side="right"))
    if done > fetch["begun"]:
        q.track_fetch_begin(fetch["begun"], done - fetch["begun"])
        fetch["ranges"].append(done - fetch["begun"])
        fetch["begun"] = done


def round_ms(q, fetching):
    """(device ms per step inside the event pair, host wall ms per step with the fetch turn and a synchronisation behind the steps)"""
    t0 = q.get_timing()["advance_ms"]          # (completes the pending step and synchronises: the wall clock starts on an idle device)
    w0 = time.perf_counter()
    q.run_steps(DT, STEPS)
    if fetching:
        turn(q)
    q.sync()
    w1 = time.perf_counter()
    return (q.get_timing()["advance_ms"] - t0) / STEPS, 1e3 * (w1 - w0) / STEPS


rows = {"with_set": [], "without": [], "wall_with_set_and_fetch": [], "wall_without": []}
for r in range(ROUNDS + 1):
    (w, ww), (o, wo) = round_ms(b, True), round_ms(a, False)
    print(f"round {r}: with a set {w:.4f} ms per step (wall, fetch included: {ww:.4f}), without {o:.4f} (wall {wo:.4f})", file=sys.stderr)
    if r:
        for k_, x in zip(rows, (w, o, ww, wo)):
            rows[k_].append(x)
if fetch["begun"] > fetch["fetched"]:
    b.track_fetch_end()
m_events, _, samples = b.track_info()
b.track_fetch_begin(0, m_events)
table = b.track_fetch_end()
distinct = int(len(np.unique(corners.reshape(-1, 2), axis=0)))
per_step = int(len(np.unique(corners[: 2 * PER_PASS].reshape(-1, 2), axis=0)))
out = {"n": N, "events": int(m_events), "events_per_step": 2 * PER_PASS, "steps_per_round": STEPS, "unit": "ms per step (one event pair around 20 steps)",
       "samples_taken": int(samples), "events_with_both_slots": int((~np.isnan(table).any(axis=0)).sum())}
out.update({k_ + "_ms": v for k_, v in rows.items()})
out.update({"median_" + k_ + "_ms": float(np.median(v)) for k_, v in rows.items()})
out["median_cost_ms"] = out["median_with_set_ms"] - out["median_without_ms"]
out["median_wall_cost_with_fetch_ms"] = out["median_wall_with_set_and_fetch_ms"] - out["median_wall_without_ms"]
out["events_per_fetch"] = fetch["ranges"]
out["table_bytes"] = int(8 * 8 * m_events)
out["as_stations"] = {"distinct_corner_nodes": distinct, "distinct_corner_nodes_of_one_step": per_step, "bytes_per_sample": 24 * distinct,
                      "ring_bytes_device_and_pinned_each_at_capacity_64": 64 * 24 * distinct}
print(json.dumps(out))
