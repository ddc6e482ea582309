"""The host side of the wind window (struct WindWindow of picles_hip.hip: host-set levels and the device-sampled lattice behind one
publisher) under AddressSanitizer + UBSan on the CPU box: the translation units host-only against the fake HIP runtime, as
tests/test_host_asan_nest.py builds them (same Makefile, same objects), driven by the stand-alone program
tests/native/host_asan/wind_harness.cpp — one context, then a two-slab pair through the split phases, walked through every form of a
window and every transition between neighbouring forms, from host levels and from a lattice; then every creation inside the lazily
made plane pairs failed in turn: the call fails, the same call then succeeds, and no launch behind it is handed half a pair.
Then what the kernels are handed: the same program, without the failed creations, traced (PICLES_FAKE_HIP_TRACE) and compared by
trace_diff.py with tests/golden/wind_host_trace_parent.txt, the trace of the host code as it was before the window had one owner:
every launch, copy, event record, stream wait and synchronisation must be the same call in the same place (allocation and creation
lines may differ), and the "window" lines of the harness's launch hook — the nine wind fields of KParams at every launch that takes
them, bit for bit, and which level each live plane holds — must be identical one for one."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
GOLDEN = ROOT / "tests" / "golden" / "wind_host_trace_parent.txt"


@pytest.mark.skipif(not (Path(HIPCC).exists() and Path(CXX).exists()), reason="no hipcc")
def test_wind_host_code_is_clean_under_asan_and_hands_the_kernels_what_it_did(tmp_path_factory):
    d = ROOT / "tests" / "native" / "host_asan"
    OUT = Path(os.environ.get("PICLES_HOST_ASAN_OUT") or tmp_path_factory.mktemp("host_asan_wind"))
    exe = OUT / "wind_harness"
    r = subprocess.run(["make", "-s", "-j4", f"OUT={OUT}", str(exe)], cwd=d, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("PICLES_FAKE_HIP_TRACE", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert " 0 creations failed" not in r.stdout, r.stdout[-500:]

    trace = OUT / "wind_host_trace.txt"
    trace.unlink(missing_ok=True)
    r = subprocess.run([str(exe), "trace"], capture_output=True, text=True, timeout=600, env=dict(env, PICLES_FAKE_HIP_TRACE=str(trace)))
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([sys.executable, str(d / "trace_diff.py"), str(GOLDEN), str(trace)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ordering calls identical" in r.stdout, r.stdout[-3000:]
    assert "window lines identical (0)" not in r.stdout and "window lines identical" in r.stdout, r.stdout[-3000:]
