"""The Rosenbrock23 attempt and the initial step on the device against the same functions compiled for the host, bit for bit."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.gpu
def test_rosenbrock_attempt_and_initial_step_device_equal_host_bitwise(tmp_path):
    """physics.h ros23_try in four instantiations and init_dt in two (tests/native/gpu_ros_check.hip), 64 x 256 + 37 states per variant,
    ordered so that the wave-uniform branches — the forward-mode Jacobian and its `mine` selection, 1/det, pm_exp_sat, W.ymaxw — are
    decided per wave on the device where the host decides per state: waves all plain, all non-plain, with one non-plain lane at lane 0
    and at lane 63, with |det| beyond 1e290 next to ordinary ones, and a last wave of 37 live lanes.  The program checks that layout
    itself (exit status 3 if the states are not what it says)."""
    exe = tmp_path / "gpu_ros_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                    "-I", str(ROOT / "picles_amd" / "csrc"), str(ROOT / "tests" / "native" / "gpu_ros_check.hip"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" 0 mismatches") == 6, r.stdout
