"""Register, scratch and RK-loop budget of k_step_waverow (k_step.inc, WROW), from the compiler's resource report and assembly (hipcc
cross-compiles gfx950 without a GPU).  The wave-per-row form moves index and address arithmetic outside the RK loop to the scalar unit;
the scalar register file is full inside the loop (tests/test_kernel_budget.py), so what that costs shows here before it shows as time:
more spilled scalars are lane moves inside the loop.  The loop of `k_step_waverow<1,0,1,0,0>` is held against the loop of
`k_step<1,0,1,0,0>` compiled in the same run — the unchanged old kernel is the reference, not a literal."""
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
_UNITS = {}


def _unit(unit):
    """(resource usage by kernel, isa_budget primed with the same compile's assembly)"""
    import isa_budget
    if unit not in _UNITS:
        src = ROOT / "picles_amd" / "csrc"
        r = subprocess.run([HIPCC, *isa_budget.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-S", str(src / unit), "-o", "-"],
                           capture_output=True, text=True, cwd=src, timeout=1200)
        assert r.returncode == 0, r.stderr[-2000:]
        isa_budget._ASM[unit] = r.stdout
        usage = {}
        for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
            get = lambda key: int(re.search(key + r": (\d+)", b).group(1))      # noqa: E731
            usage[b.split()[0]] = dict(vgpr=get(r"VGPRs"), scratch=get(r"ScratchSize \[bytes/lane\]"), occ=get(r"Occupancy \[waves/SIMD\]"),
                                       vspill=get(r"VGPRs Spill"), sspill=get(r"SGPRs Spill"))
        _UNITS[unit] = usage
    return _UNITS[unit], isa_budget


def _loop(isa_budget, unit, name):
    _, _, tot, _ = isa_budget.budget(unit, name)
    assert tot["fp64 fma"] + tot["fp64 mul"] > 500, (name, tot)      # the loop that was found is the RK loop
    valu = sum(v for k, v in tot.items() if k.split(" ")[0] in ("fp64", "cvt", "mov", "select", "lane", "int") or k.startswith("other:v_"))
    return valu, tot.get(SCRATCH, 0), tot.get(LANE, 0)


def test_baseline_flavour_keeps_the_budget_of_the_old_kernel():
    usage, isa_budget = _unit("k_step_explicit.hip")
    new, old = "_Z14k_step_waverowILb1ELb0ELb1ELb0ELb0" + ARGS, "_Z6k_stepILb1ELb0ELb1ELb0ELb0" + ARGS
    u = usage[new]
    assert u["occ"] == 4 and u["vgpr"] <= 128 and u["vspill"] <= 10 and u["scratch"] <= 48 and u["sspill"] <= 24, u
    valu, scr, lane = _loop(isa_budget, "k_step_explicit.hip", new)
    valu_old, _, _ = _loop(isa_budget, "k_step_explicit.hip", old)
    assert scr == 0 and lane <= 4, (scr, lane)
    assert valu <= valu_old, (valu, valu_old)


def test_every_explicit_flavour_reaches_four_waves():
    usage, isa_budget = _unit("k_step_explicit.hip")
    names = isa_budget.waverow_kernels("k_step_explicit.hip")
    want = [f"_Z14k_step_waverowILb1ELb{t}ELb{s}ELb0ELb0" + ARGS for t in (0, 1) for s in (0, 1)]
    assert sorted(names) == sorted(want), names
    for n in names:      # DP5 and Tsit5, static and time-varying winds
        assert usage[n]["occ"] == 4, (n, usage[n])


def test_auto_flavours_reach_three_waves_within_the_bounds_of_their_twins():
    """the bounds tests/test_kernel_budget.py::test_rk_loops_stay_clear_of_spill_code states for k_step<1,1,S,0,1>"""
    usage, isa_budget = _unit("k_step_auto.hip")
    names = isa_budget.waverow_kernels("k_step_auto.hip")
    assert len(names) == 2, names
    for n in names:
        assert usage[n]["occ"] >= 3, (n, usage[n])
        static = n.startswith("_Z14k_step_waverowILb1ELb1ELb1E")
        _, scr, lane = _loop(isa_budget, "k_step_auto.hip", n)
        assert scr <= (8 if static else 32) and lane <= 72, (n, scr, lane)
