"""Whole integrations by integrate_dp5 on the device against the same function compiled for the host, bit for bit."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.gpu
def test_explicit_integrations_device_equal_host_bitwise(tmp_path):
    """physics.h integrate_dp5 over one DT in seven instantiations (tests/native/gpu_explicit_check.hip) — DP5 fast / static with the
    tables through scalar loads and through LDS, Tsit5 under a parabola window, the auto-switching solver in both table forms, the
    general flavour of k_bforce under a knot window, one metric variant — 64 x 64 + 37 states each, compared on z, lq, dtn, asw, rhs,
    acc, rej and status.  The states are ordered so that the device decides per wave what the host decides per state: waves whose
    lanes all take the same attempts, waves where one lane alone rejects, waves whose lanes need very different attempt counts (dtn
    over three decades), waves where only lane 0 or only lane 63 enters with Rosenbrock23 active, waves with lanes whose counter
    crosses 10 inside the integration, and a last wave of 37 live lanes.  The program checks that layout itself (exit status 3 if the
    states are not what it says).  The host side of the comparison is what tests/test_explicit_reference.py holds against the
    60-digit reference."""
    exe = tmp_path / "gpu_explicit_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                    "-I", str(ROOT / "picles_amd" / "csrc"), str(ROOT / "tests" / "native" / "gpu_explicit_check.hip"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" 0 mismatches") == 7, r.stdout
