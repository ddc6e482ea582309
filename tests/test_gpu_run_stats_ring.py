"""Run statistics in the NATIVE slab ring over the loopback communicator (2 ranks): every rank accumulates over its own rows, the
update of a fused step on the ring's side stream behind the interior launch and the delivered exchange; the rank-ordered
concatenation of the planes equals tests/_stats_numpy.py over a whole-grid twin's States bit for bit.  (Slabs in one process:
tests/test_gpu_run_stats.py.)"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def loopback(tmp_path_factory):
    so = tmp_path_factory.mktemp("loopback") / "libloopback_ccl.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include",
                    str(ROOT / "tests" / "native" / "loopback_ccl.cpp"), "-o", str(so)], check=True)
    return so


@pytest.mark.parametrize("world,case,solver,steps,chunks,every,first,halo", [
    (2, "smooth", "DP5", 9, "2,7", 1, 1, 2),          # two ranks on a periodic axis, every step
    (2, "open", "DP5", 8, "3,5", 3, 2, 1),            # open y axis, land across the slab boundary, a cadence with gaps, halo 1
])
def test_native_ring_statistics_through_the_loopback_communicator(loopback, world, case, solver, steps, chunks, every, first, halo):
    env = dict(os.environ, PICLES_CCL_LIB=str(loopback))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "native" / "stat_ring_driver.py"), str(world), case, solver, str(steps), chunks,
                        str(every), str(first), str(halo)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    assert res["planes_that_differ"] == [], res
    assert res["n_samples"] == [res["want_samples"]] * world, res
    assert res["t_first"] == [res["want_t"][0]] * world and res["t_last"] == [res["want_t"][1]] * world, res
    assert res["wet_share"] >= 0.5 and res["exceeding_share"] > 0.0, res
