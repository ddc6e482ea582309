"""The host side of picles_nest_set_levels (a nested pair resumed from a checkpoint) under AddressSanitizer + UBSan on the CPU box: the
translation units host-only against the fake HIP runtime, as tests/test_host_asan_nest_restart.py builds them (same Makefile, same objects),
driven by the stand-alone program tests/native/host_asan/nest_restart_harness.cpp — pairs saved one, two and three child steps past a
parent level, their blobs and their pair in heap blocks of exactly the contract's size, resumed in new contexts one-way and with
feedback and run on through the third and fourth sample; every refusal of the call with its text and a step of both contexts behind
it; and the destroy orders after a resume.  Nothing is loaded into Python."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SAN = "-fsanitize=address,undefined -fno-sanitize=function,vptr -fno-omit-frame-pointer -g -O1".split()
UNITS = ("picles_hip", "k_step_explicit", "k_step_auto", "k_advance", "k_bforce")


@pytest.mark.skipif(not (Path(HIPCC).exists() and Path(CXX).exists()), reason="no hipcc")
def test_nest_restart_host_code_is_clean_under_asan(tmp_path_factory):
    d = ROOT / "tests" / "native" / "host_asan"
    OUT = Path(os.environ.get("PICLES_HOST_ASAN_OUT") or tmp_path_factory.mktemp("host_asan_nest_restart"))
    r = subprocess.run(["make", "-s", "-j4", f"OUT={OUT}", f"{OUT}/fatbin_stub.c"], cwd=d, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    objs = [str(OUT / f"{u}.host.o") for u in UNITS]
    exe = OUT / "nest_restart_harness"
    r = subprocess.run([CXX, "-std=c++17", *SAN, "-I/opt/rocm/include", "-rdynamic", "nest_restart_harness.cpp", "fake_hip.cpp",
                        str(OUT / "fatbin_stub.c"), "-x", "none", *objs, "-o", str(exe), "-ldl", "-lpthread"],
                       cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("PICLES_FAKE_HIP_TRACE", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert " 0 pairs resumed" not in r.stdout and " 0 refused as documented" not in r.stdout and " 0 contexts destroyed" not in r.stdout, r.stdout[-500:]
