"""The host side of the flux means (picles_flux_mean_*) under AddressSanitizer + UBSan on the CPU box: the translation units host-only
against the fake HIP runtime, as tests/test_host_asan_flux.py builds them (same Makefile, same objects), driven by the stand-alone
program tests/native/host_asan/flux_mean_harness.cpp — exact-size buffers for every get, set, pop and export, every new entry point
and every refusal of the header (the wind rule among them), whole-grid, slab and lattice contexts, free with samples held, the mean
set dropped with its flux set, destroy with a mean push pending.  Nothing is preloaded."""
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
def test_flux_mean_host_code_is_clean_under_asan(tmp_path_factory):
    d = ROOT / "tests" / "native" / "host_asan"
    OUT = Path(os.environ.get("PICLES_HOST_ASAN_OUT") or tmp_path_factory.mktemp("host_asan_flux_mean"))
    r = subprocess.run(["make", "-s", "-j4", f"OUT={OUT}", f"{OUT}/fatbin_stub.c"], cwd=d, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    objs = [str(OUT / f"{u}.host.o") for u in UNITS]
    exe = OUT / "flux_mean_harness"
    r = subprocess.run([CXX, "-std=c++17", *SAN, "-I/opt/rocm/include", "-rdynamic", "flux_mean_harness.cpp", "fake_hip.cpp",
                        str(OUT / "fatbin_stub.c"), "-x", "none", *objs, "-o", str(exe), "-ldl", "-lpthread"],
                       cwd=d, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("PICLES_FAKE_HIP_TRACE", None)
    r = subprocess.run([str(exe), "0", "400"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "no sanitizer report" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
