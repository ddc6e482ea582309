"""The head of k_step_waverow, from the compiler's assembly (hipcc cross-compiles gfx950 without a GPU; DESIGN.md §10, "The head's
loads").  For the two staged flavours, `k_step_waverow<1,0,1,0,0>` (DP5) and `<1,1,1,0,0>` (Tsit5), static winds:

 - u0, v0 and ln q_old are asked for by three `global_load_lds` (no destination register) ahead of the first load of a record value;
 - behind the pull they are read from LDS behind a wait for the vector-memory counter alone, and from there to the header of the RK
   loop the path every stepped lane takes holds no `global_load` (what is left reads the two wind planes through the global pointers
   inside an exec-masked stretch that a wave without a lane to re-seed jumps over, and the rare paths);
 - the rows of the reach and class maps are written out, one straight line per reach: at reach 1 the three rows of the class map, at
   reach 2 the five rows of each map, and no wait for the vector-memory counter between the first and the last load of either.

k_step and k_advance are not meant to change: their instruction streams, mnemonic by mnemonic (scripts/stream_compare.py's reading
of the assembly), are held against the digests recorded from the tree before this change (tests/golden/step_kernel_streams.json;
a change that means to touch them records new ones with `python tests/test_kernel_head_loads.py --record`)."""
import hashlib
import json
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
sys.path.insert(0, str(ROOT / "scripts"))

pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="no hipcc")
ARGS = "EEv7KParams5GridP6Arraysddddiiii"
UNIT = "k_step_explicit.hip"
UNITS = ("k_step_explicit.hip", "k_step_auto.hip", "k_advance.hip")
STAGED = {"DP5": "_Z14k_step_waverowILb1ELb0ELb1ELb0ELb0" + ARGS, "Tsit5": "_Z14k_step_waverowILb1ELb1ELb1ELb0ELb0" + ARGS}
DIGESTS = ROOT / "tests" / "golden" / "step_kernel_streams.json"
VM_WAIT = re.compile(r"s_waitcnt\b.*vmcnt")
ROW_LOAD = re.compile(r"global_load_dwordx[23] v\[\d+:\d+\], v\d+, s\[\d+:\d+\] offset:-4$")      # three ints from tile - 1 on, uniform base
_ASM = {}


def _assembly(units):
    """the assembly of the units (each compiled once per process, the missing ones side by side), also handed to isa_budget"""
    import isa_budget
    src = ROOT / "picles_amd" / "csrc"

    def one(unit):
        r = subprocess.run([HIPCC, *isa_budget.FLAGS, "-S", str(src / unit), "-o", "-"], capture_output=True, text=True, cwd=src, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    todo = [u for u in units if u not in _ASM]
    with ThreadPoolExecutor(max_workers=3) as ex:
        for u, text in zip(todo, ex.map(one, todo)):
            _ASM[u] = isa_budget._ASM[u] = text
    return isa_budget


def _blocks(name):
    """(basic blocks of the kernel in program order, index of the RK loop's header)"""
    isa_budget = _assembly([UNIT])
    _, rk, blocks = isa_budget._walk(UNIT, name)
    hdr = next(k for k, b in enumerate(blocks) if b["label"] == "L" + rk)
    return blocks, hdr


@pytest.mark.parametrize("flavour", list(STAGED))
def test_node_planes_are_asked_for_ahead_of_the_records(flavour):
    blocks, _ = _blocks(STAGED[flavour])
    ins = [i for b in blocks for i in b["ins"]]
    first_record = next(k for k, i in enumerate(ins) if i.startswith("global_load_dwordx4"))
    ahead = ins[:first_record]
    assert sum(i.startswith("global_load_lds_dwordx4") for i in ahead) >= 3, [i for i in ahead if i.startswith("global_load")]
    assert sum(i.startswith("global_load_ubyte") for i in ahead) == 1          # the flags byte, into one register
    assert not [i for i in ins[first_record:] if i.startswith("global_load_lds")]


@pytest.mark.parametrize("flavour", list(STAGED))
def test_no_node_plane_is_loaded_between_the_pull_and_the_rk_loop(flavour):
    blocks, hdr = _blocks(STAGED[flavour])
    # the stage is read where a block waits for vmcnt alone (the wait written through the builtin) and reads LDS right behind it
    at = None
    for k in range(hdr):
        ins = blocks[k]["ins"]
        for q, i in enumerate(ins):
            if i == "s_waitcnt vmcnt(0)" and blocks[k]["hdr"] is None and sum(x.startswith("ds_read") for x in ins[q + 1:q + 16]) >= 2:
                at = (k, q)
    assert at is not None, "no LDS read stands behind a wait for the vector-memory counter ahead of the RK loop"
    k0, q0 = at
    reads = [i for i in blocks[k0]["ins"][q0 + 1:q0 + 16] if i.startswith("ds_read")]
    assert sum(2 if i.startswith("ds_read2") else 1 for i in reads) >= 3, reads      # u0, v0, ln q_old
    # from there to the loop header: program order, rare blocks left out, exec-masked stretches that a wave may jump over left out
    order = {b["label"]: k for k, b in enumerate(blocks)}
    path, skip_to = [], -1
    for k in range(k0, hdr):
        b = blocks[k]
        if k < skip_to or b["rare"]:
            continue
        for q, i in enumerate(b["ins"][q0 + 1:] if k == k0 else b["ins"]):
            path.append(i)
            m = re.match(r"s_cbranch_execz\s+\.(LBB\d+_\d+)", i)
            if m and order.get(m.group(1), -1) > k:
                skip_to = order[m.group(1)]
                break
    assert len(path) >= 20, len(path)
    assert not [i for i in path if i.startswith("global_load")], [i for i in path if i.startswith("global_load")]
    jumped = [i for k in range(k0, hdr) for i in blocks[k]["ins"] if i.startswith("global_load_dwordx2")]
    assert len(jumped) >= 2, jumped          # the re-seed branch still reads u0 and v0 through the global pointers


@pytest.mark.parametrize("flavour", list(STAGED))
def test_map_rows_are_in_flight_together(flavour):
    blocks, _ = _blocks(STAGED[flavour])
    flat = [(b["hdr"], i) for b in blocks for i in b["ins"]]
    # the row loads outside any loop, in program order, cut into runs wherever the stream waits for the vector-memory counter
    runs = [0]
    for h, i in flat:
        if VM_WAIT.match(i):
            runs.append(0)
        elif h is None and ROW_LOAD.match(i):
            runs[-1] += 1
    runs = sorted(r for r in runs if r)
    assert runs == [3, 10], runs          # reach 1: three rows of the class map; reach 2: five rows of each map; no wait inside either
    # larger reaches keep the counted loop
    assert [i for h, i in flat if h is not None and ROW_LOAD.match(i)]


def _digests():
    from stream_compare import streams
    import tempfile
    _assembly(UNITS)
    out = {}
    for u in UNITS:
        with tempfile.NamedTemporaryFile("w", suffix=".s") as f:
            f.write(_ASM[u])
            f.flush()
            for name, mnem in streams(f.name).items():
                if name.startswith(("_Z6k_stepI", "_Z9k_advanceI")):
                    out[name] = {"unit": u, "instructions": len(mnem), "sha256": hashlib.sha256("\n".join(mnem).encode()).hexdigest()}
    return out


def test_k_step_and_k_advance_keep_their_streams():
    want = json.loads(DIGESTS.read_text())["kernels"]
    got = _digests()
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    differ = [(n, want[n]["instructions"], got[n]["instructions"]) for n in want if got[n]["sha256"] != want[n]["sha256"]]
    assert not differ, differ


if __name__ == "__main__" and "--record" in sys.argv:
    DIGESTS.write_text(json.dumps({"what": "mnemonic streams of the k_step and k_advance kernels (scripts/stream_compare.py's reading of hipcc -S)",
                                   "kernels": _digests()}, indent=1, sort_keys=True) + "\n")
    print("recorded", DIGESTS)
