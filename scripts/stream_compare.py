"""Compare the instruction streams of the step kernels in two assembly files (hipcc -S --cuda-device-only of the same translation unit
at two commits), mnemonic by mnemonic: a refactoring that must leave a kernel's code alone shows here whether it did.

    python scripts/stream_compare.py OLD.s NEW.s [name-prefix ...]        # default prefixes: _Z6k_stepI _Z9k_advanceI
"""
import re
import sys


def streams(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*;", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        t = line.strip()
        if cur is None or not t or t.startswith((";", ".", "//")):
            continue
        cur.append(t.split()[0])
    return out


def main():
    old, new = streams(sys.argv[1]), streams(sys.argv[2])
    prefixes = tuple(sys.argv[3:]) or ("_Z6k_stepI", "_Z9k_advanceI")
    bad = 0
    for name in sorted(old):
        if not name.startswith(prefixes):
            continue
        if name not in new:
            print(f"MISSING  {name}")
            bad += 1
            continue
        a, b = old[name], new[name]
        if a == b:
            print(f"same     {name}  ({len(a)} instructions)")
        else:
            k = next((q for q, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"DIFFERS  {name}  ({len(a)} -> {len(b)} instructions, first difference at #{k})")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
