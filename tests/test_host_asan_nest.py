"""The host side of the boundary forcing and of both directions of a nest (picles_bforce_*, picles_nest_*, picles_nest_feedback_*)
under AddressSanitizer + UBSan on the CPU box: the translation units host-only against the fake HIP runtime, as
tests/test_host_asan_stat.py builds them (same Makefile, same objects, and k_bforce.hip, without whose launcher no forcing set can be
made), driven by the stand-alone program tests/native/host_asan/nest_harness.cpp — every entry point, every refusal, exact-size
buffers, the lifetimes from either end, the slot rotation of both directions, and every creation of the three inits failed in turn.
Then the ordering: the same program, without the failed creations, traced (PICLES_FAKE_HIP_TRACE) and compared by trace_diff.py with
tests/golden/nest_host_trace_parent.txt, the trace of the host code as it was before both directions sat on one link: every launch,
copy, event record, stream wait and synchronisation must be the same call in the same place; allocation and creation lines may differ."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SAN = "-fsanitize=address,undefined -fno-sanitize=function,vptr -fno-omit-frame-pointer -g -O1".split()
UNITS = ("picles_hip", "k_step_explicit", "k_step_auto", "k_advance", "k_bforce")
GOLDEN = ROOT / "tests" / "golden" / "nest_host_trace_parent.txt"


@pytest.mark.skipif(not (Path(HIPCC).exists() and Path(CXX).exists()), reason="no hipcc")
def test_nest_host_code_is_clean_under_asan_and_orders_as_before(tmp_path_factory):
    d = ROOT / "tests" / "native" / "host_asan"
    OUT = Path(os.environ.get("PICLES_HOST_ASAN_OUT") or tmp_path_factory.mktemp("host_asan_nest"))
    r = subprocess.run(["make", "-s", "-j4", f"OUT={OUT}", f"{OUT}/fatbin_stub.c"], cwd=d, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    objs = [str(OUT / f"{u}.host.o") for u in UNITS]
    exe = OUT / "nest_harness"
    r = subprocess.run([CXX, "-std=c++17", *SAN, "-I/opt/rocm/include", "-rdynamic", "nest_harness.cpp", "fake_hip.cpp",
                        str(OUT / "fatbin_stub.c"), "-x", "none", *objs, "-o", str(exe), "-ldl", "-lpthread"],
                       cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("PICLES_FAKE_HIP_TRACE", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert " 0 inits failed by a creation" not in r.stdout, r.stdout[-500:]

    trace = OUT / "nest_host_trace.txt"
    trace.unlink(missing_ok=True)
    r = subprocess.run([str(exe), "trace"], capture_output=True, text=True, timeout=600, env=dict(env, PICLES_FAKE_HIP_TRACE=str(trace)))
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([sys.executable, str(d / "trace_diff.py"), str(GOLDEN), str(trace)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ordering calls identical" in r.stdout, r.stdout[-3000:]
