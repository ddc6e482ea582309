"""Flux means in the NATIVE slab ring over the loopback communicator (2 ranks): every rank accumulates over the coarse cells of its
own rows, the update of a fused step on the ring's side stream behind the interior launch and the delivered exchange; the
rank-ordered concatenation of the accumulator planes, and the totals, equal a whole-grid context's bit for bit.  Under a wind
lattice the update reads wind planes that the sampler of a later window rewrites on the context stream: the context stream waits
for the update.  (Slabs in one process: tests/test_gpu_flux_mean.py.)"""
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


@pytest.mark.parametrize("world,case,solver,steps,chunks,every,first,halo,cx,cy", [
    (2, "smooth", "DP5", 9, "2,7", 1, 1, 2, 4, 4),         # two ranks on a periodic axis, every step, groups of four
    (2, "lattice", "DP5", 8, "3,5", 1, 1, 2, 2, 3),        # device-sampled winds that change with every step; 48 rows per rank, cy = 3
    (2, "open", "DP5", 8, "3,5", 3, 2, 1, 3, 4),           # open y axis, land across the slab boundary, a cadence with gaps, the generic instance
])
def test_native_ring_flux_means_through_the_loopback_communicator(loopback, world, case, solver, steps, chunks, every, first, halo, cx, cy):
    env = dict(os.environ, PICLES_CCL_LIB=str(loopback))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "native" / "flux_mean_ring_driver.py"), str(world), case, solver, str(steps), chunks,
                        str(every), str(first), str(halo), str(cx), str(cy)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    assert res["planes_that_differ"] == [] and res["totals_that_differ"] == [] and res["state_equal"], res
    assert res["n_samples"] == [res["want_samples"]] * world and res["whole_grid_samples"] == res["want_samples"], res
    assert res["t_first"] == [res["want_t"][0]] * world and res["t_last"] == [res["want_t"][1]] * world, res
    assert res["active_share"] >= 0.5, res
