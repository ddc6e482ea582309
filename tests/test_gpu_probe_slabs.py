"""Station probes over slabs: every rank samples the nodes of its own rows, `gather_probes()` puts them back into the caller's
order, and the result equals the whole-grid context's samples bit for bit whatever the decomposition — in the Python-driven
split-phase loop (2, 3, 4 ranks sharing the GPU over gloo; picles_probe_sample behind the halo exchange), in the NATIVE ring over
the loopback communicator (2 and 4 ranks; the probe runs on a side stream that waits for the interior launch and the exchange),
and in the ring of one.  The node sets hold nodes in the first and last owned rows of every slab, which ghost records feed."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import assert_bitwise, spawn_ranks

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
sys.path.insert(0, str(ROOT / "tests" / "native"))


def _cfg():
    from picles_amd import configs
    return configs.bench06_box(n=64, dx=1500.0, winds=configs.smooth_winds(10.0, 8.0, 64 * 1500.0, 64 * 1500.0))


def _whole_grid(cfg, nodes, n_steps, every=1, first=1):
    """the whole-grid context's samples (seeded state first) and its State after every step"""
    from picles_amd.parallel import SlabModel
    one = SlabModel(cfg.model, 0, 1, device=0)
    one.seed()
    one.probe_init(nodes, every=every, first=first, capacity=n_steps + 1)
    one.probe_sample()
    states = []
    for _ in range(n_steps):
        one.time_step(cfg.Δt)
        states.append(one.get_state())
    return one.gather_probes(), states


def _worker(rank, world, port, n_steps, halo, outdir):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "tests" / "native"))
    from picles_amd.parallel import SlabModel
    from probe_ring_driver import slab_nodes
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg = _cfg()
    nodes = slab_nodes(64, 64, world)
    model = SlabModel(cfg.model, rank, world, device=0, halo_rows=halo)
    model.seed()
    model.probe_init(nodes, capacity=n_steps + 1)
    model.probe_sample()
    for _ in range(n_steps):
        model.time_step(cfg.Δt)
    v, t, s = model.gather_probes()
    if rank == 0:
        np.savez(os.path.join(outdir, "probes.npz"), v=v, t=t, s=s)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,halo", [(2, 1), (3, 2), (4, 1)])
@pytest.mark.timeout(300)
def test_python_driven_slabs_gather_the_whole_grid_samples(tmp_path, world, halo):
    from probe_ring_driver import slab_nodes
    n_steps = 5
    spawn_ranks(_worker, lambda port: (world, port, n_steps, halo, str(tmp_path)), world)
    got = np.load(tmp_path / "probes.npz")
    nodes = slab_nodes(64, 64, world)
    (v, t, s), states = _whole_grid(_cfg(), nodes, n_steps)
    assert list(got["s"]) == list(s) == list(range(n_steps + 1)) and np.array_equal(got["t"], t)
    assert_bitwise(got["v"], v, f"{world} slabs, halo {halo}: gathered samples vs the whole-grid context's")
    for k in range(1, n_steps + 1):
        assert_bitwise(got["v"][k], np.ascontiguousarray(states[k - 1][nodes[:, 0], nodes[:, 1], :].T), f"step {k} vs State")
    wet = float((got["v"][-1][0] > 0).mean())
    print(f"{world} slabs: wet share {wet:.3f}")
    assert wet >= 0.5


@pytest.fixture(scope="module")
def loopback(tmp_path_factory):
    so = tmp_path_factory.mktemp("loopback") / "libloopback_ccl.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include",
                    str(ROOT / "tests" / "native" / "loopback_ccl.cpp"), "-o", str(so)], check=True)
    return so


@pytest.mark.parametrize("world,case,solver,steps,chunks,every,first,halo", [
    (2, "smooth", "DP5", 9, "9", 1, 1, 2),            # two ranks on a periodic axis, every step, one call
    (4, "open", "DP5", 8, "3,5", 1, 1, 1),            # open y axis, land across a slab boundary, two calls, halo 1
    (4, "smooth", "AutoTsit5", 9, "4,5", 3, 2, 2),    # a cadence with gaps: the buffer hand-over flags of un-sampled steps
    (3, "lattice", "DP5", 6, "2,4", 1, 1, 2),         # device-sampled time-varying winds: fused and plain steps mixed
])
def test_native_ring_probes_through_the_loopback_communicator(loopback, world, case, solver, steps, chunks, every, first, halo):
    env = dict(os.environ, PICLES_CCL_LIB=str(loopback))
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "native" / "probe_ring_driver.py"), str(world), case, solver, str(steps), chunks,
                        str(every), str(first), str(halo)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(res)
    assert res["mismatches"] == 0 and res["steps"] == res["want_steps"] and res["times_equal"], res
    assert res["ranks_with_nodes"] == world and res["wet_share"] >= 0.5, res


def test_ring_of_one():
    from picles_amd.parallel import SlabModel
    from probe_ring_driver import slab_nodes
    n_steps = 6
    cfg = _cfg()
    nodes = slab_nodes(64, 64, 1)
    (v, t, s), states = _whole_grid(_cfg(), nodes, n_steps)
    ring = SlabModel(cfg.model, 0, 1, device=0, halo_rows=2, ring_of_one=True)
    assert ring.native
    ring.seed()
    ring.probe_init(nodes, capacity=n_steps + 1)
    ring.probe_sample()
    ring.run_steps(cfg.Δt, 2)
    for _ in range(n_steps - 2):
        ring.time_step(cfg.Δt)
    got = ring.gather_probes()
    assert list(got[2]) == list(s) and np.array_equal(got[1], t)
    assert_bitwise(got[0], v, "ring of one vs the whole-grid context")
    assert float((got[0][-1][0] > 0).mean()) >= 0.5
