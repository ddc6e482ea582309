"""Where the RK loop of the fused DP5 step waits, from the compiler's assembly (hipcc cross-compiles gfx950 without a GPU): the common
path of the loop of `k_step_waverow<1,0,1,0,0>` and of `k_step<1,0,1,0,0>`, walked block by block with scripts/isa_budget.py.

Scalar loads and LDS reads share one counter (lgkmcnt), scalar loads return out of order, so every wait for either is
`s_waitcnt lgkmcnt(0)` and a wave sleeps through the round trip of whatever is still in flight.  What this file holds:
 - the exponential's table read (pm_exp_plain) leaves ahead of the polynomial and is consumed behind it: no wait stands within the
   polynomial's six fp64 instructions of a `ds_read_b64`;
 - the tableau's address is formed on the scalar unit (pc-relative), not fetched from the GOT: no `gotpcrel` relocation in the loop;
 - the number of waits in the loop body: 38 before the three changes, 27 with them — written here as the ceiling;
 - none of it was bought with registers: the resource line and the loop's spill classes are those of the kernel before."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
sys.path.insert(0, str(ROOT / "scripts"))

pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="no hipcc")
LANE = "lane moves (readlane / writelane / readfirstlane / dpp / permute)"
SCRATCH = "scratch (spill traffic)"
ARGS = "EEv7KParams5GridP6Arraysddddiiii"
UNIT = "k_step_explicit.hip"
WAVEROW = "_Z14k_step_waverowILb1ELb0ELb1ELb0ELb0" + ARGS
OLD = "_Z6k_stepILb1ELb0ELb1ELb0ELb0" + ARGS
POLY = 6                                   # r (two fma), r², Estrin's three: what needs neither the table's address nor its entry
WAITS = {WAVEROW: 27, OLD: 29}             # s_waitcnt in the loop body, common path (before: 38 and 30)
_CACHE = {}


def _compiled():
    """(resource usage by kernel, isa_budget primed with the same compile's assembly) — one compile for the whole file"""
    import isa_budget
    if not _CACHE:
        src = ROOT / "picles_amd" / "csrc"
        r = subprocess.run([HIPCC, *isa_budget.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-S", str(src / UNIT), "-o", "-"],
                           capture_output=True, text=True, cwd=src, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        isa_budget._ASM[UNIT] = r.stdout
        usage = {}
        for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
            get = lambda key: int(re.search(key + r": (\d+)", b).group(1))      # noqa: E731
            usage[b.split()[0]] = dict(vgpr=get(r"VGPRs"), scratch=get(r"ScratchSize \[bytes/lane\]"), occ=get(r"Occupancy \[waves/SIMD\]"),
                                       vspill=get(r"VGPRs Spill"), sspill=get(r"SGPRs Spill"))
        _CACHE["usage"] = usage
    return _CACHE["usage"], isa_budget


def _stream(name):
    """the loop's common path as one instruction list, in program order"""
    _, isa_budget = _compiled()
    _, _, tot, _ = isa_budget.budget(UNIT, name)
    assert tot["fp64 fma"] + tot["fp64 mul"] > 500, (name, tot)      # the loop that was found is the RK loop
    return [i for _, ins in isa_budget.rk_common_path(UNIT, name) for i in ins], tot


@pytest.mark.parametrize("name", [WAVEROW, OLD], ids=["k_step_waverow", "k_step"])
def test_table_reads_run_under_the_polynomial(name):
    ins, _ = _stream(name)
    reads = [k for k, i in enumerate(ins) if i.startswith("ds_read_b64")]
    assert len(reads) == 14, len(reads)      # two per RHS evaluation of the attempt, the controller's on either side of its branch
    for k in reads:
        nxt = next(q for q in range(k + 1, len(ins)) if ins[q].startswith("s_waitcnt"))
        between = sum(bool(re.match(r"v_\w+_f64", i)) for i in ins[k + 1:nxt])
        assert between >= POLY, (name, k, between, ins[k:nxt + 1])


@pytest.mark.parametrize("name", [WAVEROW, OLD], ids=["k_step_waverow", "k_step"])
def test_no_address_comes_from_the_got_inside_the_loop(name):
    ins, _ = _stream(name)
    assert not [i for i in ins if "gotpcrel" in i]
    assert [i for i in ins if "DPTAB_C@rel32" in i]      # the tableau is still read stage by stage from a pc-relative address


@pytest.mark.parametrize("name", [WAVEROW, OLD], ids=["k_step_waverow", "k_step"])
def test_waits_in_the_loop_body(name):
    ins, _ = _stream(name)
    waits = [i for i in ins if i.startswith("s_waitcnt")]
    print(name, len(waits), "s_waitcnt in the loop body")
    assert len(waits) <= WAITS[name], (name, len(waits))


def test_resources_are_those_of_the_kernel_before():
    usage, _ = _compiled()
    u = usage[WAVEROW]
    assert u["vgpr"] <= 128 and u["occ"] == 4 and u["sspill"] <= 15 and u["vspill"] <= 2 and u["scratch"] <= 12, u
    _, tot = _stream(WAVEROW)
    assert tot.get(LANE, 0) <= 4 and tot.get(SCRATCH, 0) == 0, tot
    valu = sum(v for k, v in tot.items() if k.split(" ")[0] in ("fp64", "cvt", "mov", "select", "lane", "int") or k.startswith("other:v_"))
    assert valu <= 846, valu                 # no instruction was meant to leave, none may come


def test_no_wait_is_written_by_hand():
    """every s_waitcnt is the compiler's: the sources hold none, and no load is issued from inline assembly"""
    src = ROOT / "picles_amd" / "csrc"
    for f in ("pmath.h", "physics.h", "kernels.h", "k_step.inc"):
        text = (src / f).read_text()
        for m in re.finditer(r"__asm__\s*(?:volatile)?\s*\(\s*\"([^\"]*)\"", text):
            assert not re.search(r"s_waitcnt|s_load|ds_read|global_load|buffer_load", m.group(1)), (f, m.group(1))
