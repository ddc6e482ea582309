"""Ledger of the VALU instructions of a fused step kernel OUTSIDE its Runge-Kutta loop, by phase, from the compiler's assembly: the unit
is compiled with line tables (which leave the code as it is), every instruction carries the chain of inlined source lines it came from,
and that chain names the phase.  Two columns per kernel: every path, and the common path of the BASELINE box — reach 1, interior nodes,
a wave whose lanes all match the same candidates, no re-seed, no guard firing — which leaves out what the chain shows to lie on other
paths (wider reaches, wrapped / aliased / tripolar windows, the per-lane walk, re-seeding).  The counts are STATIC: an instruction in a
block that a wave runs twice (the statistics' ballot ladders) or skips counts once, and both sides of every branch that the chain
cannot rule out count, so a column is several times what a wave executes.  The split is indicative — where the instruction text
shrank — and no prediction of the executed count, which comes from the counters (profiles/waverow_pmc.md).

    python scripts/valu_ledger.py k_step_explicit.hip _Z6k_stepILb1ELb0ELb1ELb0ELb0E _Z14k_step_waverowILb1ELb0ELb1ELb0ELb0E
"""
import re
import sys
from collections import Counter, OrderedDict
from pathlib import Path

import isa_budget

SRC = isa_budget.SRC
PHASES = ["index", "node loads", "reach", "pull: codes", "pull: values", "pull: other paths", "remesh", "first RHS + init dt",
          "charge + record", "statistics", "other"]
GROUPS = OrderedDict([
    ("reach", {"pull_reach", "pull_reach_local", "pull_reach_early", "pull_reach_local_waverow"}),
    ("pull", {"pull_window_2p", "pull_window_waverow", "pull_walk_lanes", "pull_candidate", "pull_node", "pull_node_aliased",
              "pull_node_tripolar", "pull_any", "pull_waverow", "floor_div", "floor_mod"}),
    ("index", {"rows_index", "rows_index_waverow", "waverow_of", "ordered_block", "order_counts", "order_entry", "xcd_block",
               "rmap_clear_ahead", "rmap_clear_ahead_waverow", "arrays_at", "order_sign_init", "order_sign", "kargs_reload"}),
    ("node loads", {"load_wind"}),
    ("statistics", {"flush_stats", "wave_sum_u64", "wave_max_i32", "order_file", "order_wanted", "order_buf", "reach_counters"}),
    ("charge + record", {"write_record", "write_record_at", "particle_to_charge", "index_weight", "rec_encode", "advance_guards",
                         "rec_row_out"}),
    ("remesh", {"remesh_regs_lazy", "charge_to_particle"}),
])
RARE = {"pull_node_aliased", "pull_node_tripolar", "pull_candidate", "pull_walk_lanes", "reseed", "floor_div", "floor_mod"}
_SRC, _FUN = {}, {}


def source(name):
    if name not in _SRC:
        p = SRC / name
        _SRC[name] = p.read_text().split("\n") if p.exists() else []
        starts = []
        for k, l in enumerate(_SRC[name], 1):
            m = re.search(r"(\w+)\s*\(KParams", l) if l.startswith("__global__") else \
                re.match(r"^(?:static |inline )*__device__[^;{]*?\b(\w+)\s*\(", l)
            if m:
                starts.append((k, m.group(1)))
        _FUN[name] = starts
    return _SRC[name]


def function_of(name, line):
    source(name)
    f = None
    for k, n in _FUN[name]:
        if k > line:
            break
        f = n
    return f


def marker(name, fun, text):
    """line of the first occurrence of `text` inside function `fun` of file `name`"""
    lines = source(name)
    start = next(k for k, n in _FUN[name] if n == fun)
    return next(k for k in range(start, len(lines) + 1) if text in lines[k - 1])


def phase_of(chain):
    """chain: [(file, line), ...] innermost first -> (phase, on the common path)"""
    if not chain:
        return "other", True
    funs = [function_of(f, l) for f, l in chain]
    texts = [(source(f)[l - 1] if 0 < l <= len(source(f)) else "") for f, l in chain]
    common = not (set(funs) & RARE)
    for (f, l), fun, t in zip(chain, funs, texts):
        if fun == "pull_any" and "pull_node<" in t and "pull_node<1>" not in t:
            common = False
        if fun == "pull_waverow" and ("pull_window_waverow<2>" in t or "pull_any(" in t):
            common = False
        if fun == "pull_node" and l >= marker("kernels.h", "pull_node", "int shx = 0"):
            common = False
        if fun == "pull_window_2p" and l >= marker("kernels.h", "pull_window_2p", "while (__ballot(m != 0u))"):
            common = False
        if fun == "pull_window_waverow" and marker("kernels.h", "pull_window_waverow", "if constexpr (R >= 2)") <= l < \
                marker("kernels.h", "pull_window_waverow", "unsigned int mu = m0"):
            common = False
    for group, names in GROUPS.items():
        hit = next((k for k, fun in enumerate(funs) if fun in names), None)
        if hit is None:
            continue
        if group != "pull":
            return group, common
        (f, l), fun = chain[hit], funs[hit]
        if fun == "pull_window_2p":
            return ("pull: codes" if l < marker("kernels.h", "pull_window_2p", "readfirstlane") else "pull: values"), common
        if fun == "pull_window_waverow":
            return ("pull: codes" if l < marker("kernels.h", "pull_window_waverow", "if constexpr (R >= 2)") else "pull: values"), common
        return ("pull: codes" if common else "pull: other paths"), common       # the reach dispatch and the interior test
    if any(f in ("physics.h", "pmath.h") for f, _ in chain) or "advance_core" in funs:
        return "first RHS + init dt", common
    f, l = chain[-1]
    if f == "k_step.inc":
        if l >= marker("k_step.inc", "K_STEP_NAME", "flush_stats<"):
            return "statistics", common
        if l > marker("k_step.inc", "K_STEP_NAME", "else status = advance_core<"):
            return "charge + record", common
        if l >= marker("k_step.inc", "K_STEP_NAME", "unsigned char pf = PREFETCH"):
            return "remesh", common
        return "index", common
    return "other", common


def ledger(unit, prefix):
    asm = isa_budget.assembly(unit)
    name, rk, _, _ = isa_budget.budget(unit, prefix)
    body = asm[asm.index("\n" + name + ":"):].split(".Lfunc_end")[0].split("\n")
    tot, com = Counter(), Counter()
    in_rk, chain = False, []
    for k, l in enumerate(body):
        m = re.match(r"^\.(LBB\d+_\d+):", l)
        if m:
            in_rk = m.group(1)[1:] == rk
            for q in range(k, min(k + 8, len(body))):
                if q > k and not body[q].strip().startswith(";"):
                    break
                h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth", body[q])
                if h and h.group(1) == rk:
                    in_rk = True
            continue
        t = l.strip()
        if t.startswith(".loc"):
            frames = re.findall(r"([\w.]+):(\d+):\d+", t.split(";", 1)[1]) if ";" in t else []
            if frames and int(frames[0][1]) > 0:
                chain = [(Path(f).name, int(n)) for f, n in frames]
            continue
        if in_rk or not t or t.startswith((";", ".", "//")):
            continue
        c = isa_budget.classify(t.split(";")[0].strip())
        if not (c.split(" ")[0] in ("fp64", "cvt", "mov", "select", "lane", "int") or c.startswith("other:v_")):
            continue
        ph, common = phase_of(chain)
        tot[ph] += 1
        if common:
            com[ph] += 1
    return name, tot, com


def main():
    unit, prefixes = sys.argv[1], sys.argv[2:]
    isa_budget.FLAGS.insert(0, "-gline-tables-only")
    cols = [ledger(unit, p) for p in prefixes]
    for name, _, _ in cols:
        print(name)
    print(f"{'VALU outside the RK loop (static)':36s}" + "".join(f"{'all paths':>12s}{'common':>10s}" for _ in cols))
    for ph in PHASES:
        print(f"{ph:36s}" + "".join(f"{tot[ph]:12d}{com[ph]:10d}" for _, tot, com in cols))
    print(f"{'total':36s}" + "".join(f"{sum(tot.values()):12d}{sum(com.values()):10d}" for _, tot, com in cols))


if __name__ == "__main__":
    main()
