#!/usr/bin/env python3
"""trace_diff.py A B — compare two traces of the fake HIP runtime (fake_hip.cpp, PICLES_FAKE_HIP_TRACE=<file>) taken from the same
harness run against two builds of the library's host side.

What must agree, line for line: every call that enqueues on, waits on, records on or synchronises a stream, an event or the device
(launches, copies, memsets, hipEventRecord, hipStreamWaitEvent, every *Synchronize, hipStreamQuery).  What may differ and is only
counted: hipMalloc / hipHostMalloc / hipFree / hipHostFree and the creation and destruction of streams and events.  The blocks that
threads other than the main one append when they end ("thread {" ... "}": the ranks of a loopback ring) are compared as a sorted
group, since only their order among each other is left to chance.  The "window ..." lines a harness's launch hook appends (wind_harness.cpp: what a launch was handed)
are no calls: they are compared on their own, one for one, and must be identical too.  Exit status 0: the ordering calls and the window
lines are identical.
TEST INFRASTRUCTURE ONLY."""
import re
import sys
from collections import Counter

MAY_DIFFER = re.compile(r"^(hipMalloc|hipHostMalloc|hipFree|hipHostFree|hipEventCreate|hipEventDestroy|hipStreamCreate|hipStreamDestroy)\b")


def load(path):
    out, block, waiting = [], None, []

    def flush():
        for b in sorted(waiting):
            out.extend(("thread {",) + b + ("}",))
        waiting.clear()
    for line in open(path):
        line = line.rstrip("\n")
        if line == "thread {":
            block = []
        elif line == "}" and block is not None:
            waiting.append(tuple(block))
            block = None
        elif block is not None:
            block.append(line)
        else:
            flush()
            out.append(line)
    flush()
    return out


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    wa, wb = [x for x in a if x.startswith("window ")], [x for x in b if x.startswith("window ")]
    a, b = [x for x in a if not x.startswith("window ")], [x for x in b if not x.startswith("window ")]
    fa, fb = [x for x in a if not MAY_DIFFER.match(x)], [x for x in b if not MAY_DIFFER.match(x)]
    ca, cb = (Counter(x.split()[0] for x in t if MAY_DIFFER.match(x)) for t in (a, b))
    print(f"{len(a)} and {len(b)} lines; ordering calls {len(fa)} and {len(fb)}; "
          f"may differ: {({k: (ca[k], cb[k]) for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]})}")
    if fa != fb:
        k = next((k for k, (x, y) in enumerate(zip(fa, fb)) if x != y), min(len(fa), len(fb)))
        print(f"ordering calls differ from call {k}:\n  A: {fa[max(0, k - 2):k + 3]}\n  B: {fb[max(0, k - 2):k + 3]}")
        return 1
    print("ordering calls identical")
    if wa != wb:
        k = next((k for k, (x, y) in enumerate(zip(wa, wb)) if x != y), min(len(wa), len(wb)))
        print(f"{len(wa)} and {len(wb)} window lines, which differ from line {k}:\n  A: {wa[k:k + 1]}\n  B: {wb[k:k + 1]}")
        return 1
    print(f"window lines identical ({len(wa)})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
