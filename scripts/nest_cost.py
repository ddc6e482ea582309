"""Cost of one-way nesting.  Parent: the 1024^2 periodic bench06 box (dx = 2000 m, Δt = 600 s).  Child: 1024^2 at a
quarter of the spacing (dx = 500 m, Δt = 150 s, ratio 4), covering 256^2 parent cells, its whole rim forced (4092 nodes).
Per parent step, host wall time around the whole loop with a final synchronisation of both contexts, alternated rounds in one
process after un-timed conditioning steps:
  (a) nested:  parent step, picles_nest_sample, four child steps
  (b) parts:   the parent alone; the child alone under a constant level taken from the nest — each separately
  (c) host route run together: the parent's probe of the corner nodes popped (blocking) after every parent step, the NumPy mix,
      picles_bforce_set_levels, four child steps
One JSON line on stdout.  --profile: a short nested run and nothing else, for
`rocprofv3 --kernel-trace --stats -- python scripts/nest_cost.py --profile`.

--feedback: the cost of two-way nesting instead, on the same pair: the parent's ocean nodes under the child, two
parent cells inside its rim, are fed from the child (picles_nest_feedback_*: (2 * 4 - 1)^2 = 49 entries per node).  Per parent
step, alternated rounds as above:
  (t) two-way: four child steps, picles_nest_feedback, parent step, picles_nest_sample
  (o) one-way: four child steps, parent step, picles_nest_sample
  (b) parts:   the parent alone; the child alone under a constant level
--feedback --profile: a short two-way run and nothing else, for rocprofv3 as above."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from picles_amd import configs, models
from picles_amd.boundary_forcing import rim_nodes
from picles_amd.grids import TwoDCartesianGridMesh
from picles_amd.nesting import default_feedback_margin, locate_in_parent, restriction_stencil, rim_points
from picles_amd.simulations import Simulation, initialize_simulation
from picles_amd.station_output import station_records

N, RATIO, DT, PDX = 1024, 4, 600.0, 2000.0
CDX, X0, Y0 = PDX / RATIO, 300.25 * PDX, 300.25 * PDX
STEPS, WARM, ROUNDS = 50, 5, 4          # parent steps per round, un-timed parent steps first, rounds
profile = "--profile" in sys.argv


def parent():
    cfg = configs.bench06_box(n=N, dx=PDX)
    m = models.WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=DT, stop_time=1.0))
    return m


def child():
    cfg = configs.bench06_box(n=16, dx=CDX, periodic_grid=False)
    cfg.model["grid"] = TwoDCartesianGridMesh(X0, X0 + CDX * (N - 1), N, Y0, Y0 + CDX * (N - 1), N, periodic_boundary=(False, False))
    m = models.WaveGrowth2D(**cfg.model)
    initialize_simulation(Simulation(m, Δt=DT / RATIO, stop_time=1.0))
    return m


def wall(fn, contexts):
    for b in contexts:
        b.sync()
    t0 = time.perf_counter()
    fn()
    for b in contexts:
        b.sync()
    return 1e3 * (time.perf_counter() - t0) / STEPS


def feedback_cost():
    def pair():
        p, c = parent(), child()
        rim = rim_nodes(c.grid, "rim")
        corner_nodes, index, weights = locate_in_parent(p.grid, rim_points(c, side="rim"))
        c.backend.bforce_init(rim)
        c.backend.nest_init(p.backend, corner_nodes, index, weights)
        c.backend.nest_sample()
        return p, c, rim

    po, co, rim = pair()
    pt, ct, _ = pair()
    fb, src, index, weight = restriction_stencil(pt.grid, ct.grid, default_feedback_margin(1, CDX, PDX))
    print(f"feedback nodes: {len(fb)}, child source nodes: {len(src)}, entries per node: {index.shape[1]}", file=sys.stderr)
    ct.backend.nest_feedback_init(fb, src, index, weight)
    ct.backend.nest_feedback()                  # the seed
    for p, c in ((po, co), (pt, ct)):
        p.backend.run_steps(DT, 1)
        c.backend.nest_sample()

    def one_way(n=STEPS):
        for _ in range(n):
            co.backend.run_steps(DT / RATIO, RATIO)
            po.backend.run_steps(DT, 1)
            co.backend.nest_sample()

    def two_way(n=STEPS):
        for _ in range(n):
            ct.backend.run_steps(DT / RATIO, RATIO)
            ct.backend.nest_feedback()
            pt.backend.run_steps(DT, 1)
            ct.backend.nest_sample()

    one_way(WARM)
    two_way(WARM)
    if profile:
        two_way(10)
        pt.backend.sync(); ct.backend.sync()
        return
    pb, cb = parent(), child()
    cb.backend.bforce_init(rim)
    cb.backend.bforce_set_levels(0.0, co.backend.bforce_get_levels()[1])
    pb.backend.run_steps(DT, WARM + 1)
    cb.backend.run_steps(DT / RATIO, RATIO * WARM)
    rows = {"two_way": [], "one_way": [], "parent_alone": [], "child_alone": []}
    for r in range(ROUNDS + 1):          # round 0 conditions the clocks and is dropped
        t = wall(two_way, (pt.backend, ct.backend))
        o = wall(one_way, (po.backend, co.backend))
        bp = wall(lambda: pb.backend.run_steps(DT, STEPS), (pb.backend,))
        bc = wall(lambda: cb.backend.run_steps(DT / RATIO, RATIO * STEPS), (cb.backend,))
        print(f"round {r}: two-way {t:.4f} ms per parent step; one-way {o:.4f}; parent alone {bp:.4f} + child alone {bc:.4f} = {bp + bc:.4f}", file=sys.stderr)
        if r:
            for k, x in zip(rows, (t, o, bp, bc)):
                rows[k].append(x)
    out = {"n": N, "ratio": RATIO, "forced_nodes": len(rim), "feedback_nodes": int(len(fb)), "source_nodes": int(len(src)), "entries_per_node": int(index.shape[1]),
           "parent_steps_per_round": STEPS, "unit": "ms per parent step (host wall time)", "levels_taken": ct.backend.nest_feedback_info()[3]}
    out.update({k + "_ms": v for k, v in rows.items()})
    out.update({"median_" + k + "_ms": float(np.median(v)) for k, v in rows.items()})
    out["median_parts_sum_ms"] = out["median_parent_alone_ms"] + out["median_child_alone_ms"]
    out["median_feedback_cost_ms"] = out["median_two_way_ms"] - out["median_one_way_ms"]
    out["one_way_overlap_ms"] = out["median_parts_sum_ms"] - out["median_one_way_ms"]
    level = pt.backend.bforce_get_levels()[0]
    out["nan_feedback_nodes"] = int(np.isnan(level[:, 0]).sum())
    print(json.dumps(out))


if "--feedback" in sys.argv:
    feedback_cost()
    sys.exit(0)

# (a) the nested pair
pa, ca = parent(), child()
rim = rim_nodes(ca.grid, "rim")
corner_nodes, index, weights = locate_in_parent(pa.grid, rim_points(ca, side="rim"))
print(f"forced nodes: {len(rim)}, parent corner nodes: {len(corner_nodes)}", file=sys.stderr)
ca.backend.bforce_init(rim)
ca.backend.nest_init(pa.backend, corner_nodes, index, weights)
ca.backend.nest_sample()
pa.backend.run_steps(DT, 1)
ca.backend.nest_sample()


def nested(n=STEPS):
    for _ in range(n):
        ca.backend.run_steps(DT / RATIO, RATIO)
        pa.backend.run_steps(DT, 1)
        ca.backend.nest_sample()


nested(WARM)
if profile:
    nested(10)
    pa.backend.sync(); ca.backend.sync()
    sys.exit(0)

# (b) the parts
pb, cb = parent(), child()
v0, v1 = ca.backend.bforce_get_levels()
cb.backend.bforce_init(rim)
cb.backend.bforce_set_levels(0.0, v1)          # constant: the sea the nest carried in at this moment
pb.backend.run_steps(DT, WARM + 1)
cb.backend.run_steps(DT / RATIO, RATIO * WARM)

# (c) the host route, both run together
pc, cc = parent(), child()
P = pc.ODEsettings.Parameters
g, r_g = P.get("g", 9.81), P["r_g"]
pc.backend.probe_init(corner_nodes, every=1, first=1, capacity=4)
cc.backend.bforce_init(rim)


def host_level():
    v, t, _ = pc.backend.probe_pop(1)           # blocking: the host waits for the parent's step
    return float(t[0]), station_records(v, index, weights, g, r_g)[0, :, :3]


pc.backend.probe_sample()
t_prev, lv_prev = host_level()
pc.backend.run_steps(DT, 1)
t_next, lv_next = host_level()


def host_route(n=STEPS):
    global t_prev, lv_prev, t_next, lv_next
    for _ in range(n):
        cc.backend.bforce_set_levels(t_prev, lv_prev, t_next, lv_next)
        cc.backend.run_steps(DT / RATIO, RATIO)
        pc.backend.run_steps(DT, 1)
        t_prev, lv_prev = t_next, lv_next
        t_next, lv_next = host_level()


host_route(WARM)

rows = {"nested": [], "parent_alone": [], "child_alone": [], "host_route": []}
for r in range(ROUNDS + 1):          # round 0 conditions the clocks and is dropped
    a = wall(nested, (pa.backend, ca.backend))
    bp = wall(lambda: pb.backend.run_steps(DT, STEPS), (pb.backend,))
    bc = wall(lambda: cb.backend.run_steps(DT / RATIO, RATIO * STEPS), (cb.backend,))
    c = wall(host_route, (pc.backend, cc.backend))
    print(f"round {r}: nested {a:.4f} ms per parent step; parent alone {bp:.4f} + child alone {bc:.4f} = {bp + bc:.4f}; host route {c:.4f}", file=sys.stderr)
    if r:
        for k, x in zip(rows, (a, bp, bc, c)):
            rows[k].append(x)
# the two routes took the same levels: the child of (c) equals the child of (a) while their clocks agree
same = bool(np.array_equal(ca.backend.get_state(), cc.backend.get_state())) if ca.backend.clock == cc.backend.clock else None
out = {"n": N, "ratio": RATIO, "forced_nodes": len(rim), "corner_nodes": int(len(corner_nodes)), "parent_steps_per_round": STEPS, "unit": "ms per parent step (host wall time)"}
out.update({k + "_ms": v for k, v in rows.items()})
out.update({"median_" + k + "_ms": float(np.median(v)) for k, v in rows.items()})
out["median_parts_sum_ms"] = out["median_parent_alone_ms"] + out["median_child_alone_ms"]
out["child_state_equal_nested_vs_host_route"] = same
out["counters"] = {"nested_child": ca.backend.get_counters(), "child_alone": cb.backend.get_counters(), "host_route_child": cc.backend.get_counters()}
print(json.dumps(out))
