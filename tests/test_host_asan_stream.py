"""The host side of the wind stream (picles_wind_stream_*: the ring's bookkeeping, the time rule, the checks of the step entry points,
the seed, the checkpoint fingerprint) and of picles_diag_export under AddressSanitizer + UBSan on the CPU box: the translation units
host-only against the fake HIP runtime, as tests/test_host_asan_wind.py builds them (same objects; tests/native/host_asan/stream.mk
adds the program), driven by the stand-alone program tests/native/host_asan/stream_harness.cpp — every level is pushed as planes
filled with its own time and the launch hook plays k_wind_sample_ring on one element, so every window that reaches a step launch is
held against its own times: init, pushes around the ring from host and "device" memory, every window form, each refusal."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not (Path(HIPCC).exists() and Path(CXX).exists()), reason="no hipcc")
def test_wind_stream_host_code_is_clean_under_asan_and_samples_the_times_it_means(tmp_path_factory):
    d = ROOT / "tests" / "native" / "host_asan"
    OUT = Path(os.environ.get("PICLES_HOST_ASAN_OUT") or tmp_path_factory.mktemp("host_asan_stream"))
    exe = OUT / "stream_harness"
    r = subprocess.run(["make", "-s", "-j4", "-f", "stream.mk", f"OUT={OUT}", str(exe)], cwd=d, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("PICLES_FAKE_HIP_TRACE", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
