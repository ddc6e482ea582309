#!/usr/bin/env python3
"""bench.py — particle-steps/s of the PiCLES 2D particle-in-cell time step on N MI355X.

A "step" is one model time step (advance + scatter + remesh) of the BASELINE.json metric
workload: the 4096×4096 periodic Cartesian box, 1 particle per cell, constant winds (10,10),
bench06 physics (configs.box4096), slab-partitioned over the N GPUs (strong scaling).
Prints ONE JSON line on rank 0.  A plain run sets up, conditions the clocks, warms up, times the K
steps and prints the headline; --full adds the CPU baseline, the secondary measurements, the
per-launch spread, the ring's phase diagnosis and the state check.  --dump-outputs DIR writes what
the timed steps computed (State and particles, float64 .npy).

    python bench.py --gpus 1 --steps 10 --warmup 2 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import math
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

B_ALG = 64.0          # algorithmic HBM bytes per particle-step (SURVEY §8d / DESIGN.md)
HBM_PEAK_GBPS = 8000.0
FP64_PEAK_TFLOPS = 78.6
FLOP_PER_RHS = 175.0  # executed fp64 flops per RHS evaluation, all-in: static count of the RK loop of k_step<FAST,DP5> (332 FMA, 352 MUL, 34 ADD per attempt of 6 evaluations)


def usable_cores():
    """host cores this process may actually use: min(cpu_count, affinity mask, cgroup CPU quota)"""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def cpu_baseline(args, W, K):
    """time the CPU oracle (kind 'port': our C restatement, OpenMP over particles) on a bounded
    sample of the same workload: an n×n periodic sub-box with identical physics and winds —
    in a homogeneous periodic box every particle does the same work at step k as in the
    4096² box — for the same W warm-up + K timed steps."""
    sys.path.insert(0, str(ROOT / "tests"))
    import _oracle as O
    from picles_amd import configs
    from picles_amd.parallel import SlabModel
    cores = usable_cores()
    threads = args.cpu_threads if args.cpu_threads else cores

    def fac(g, p, o, m, mask, **kw):
        # pull=True: the node-parallel (OpenMP) scatter; bitwise equal to the sequential push
        return O.OracleModel(g, p, o, m, kind="pmath", order=1, threads=threads, mask=mask, pull=True)

    def run(n):
        cfg = configs.box4096(n=n, U10=args.winds[0], V10=args.winds[1])
        cfg.model["ODEsys"].dir_deadband = getattr(args, "deadband", 0.0)
        cfg.model["ODEsets"].solver = getattr(args, "solver", "DP5")
        m = SlabModel(cfg.model, 0, 1, backend_factory=fac)
        m.seed()
        for _ in range(W):
            m.time_step(cfg.Δt)
        t0 = time.perf_counter()
        for _ in range(K):
            m.time_step(cfg.Δt)
        dt = time.perf_counter() - t0
        return m.n_stepped * K / dt, dt

    run(64)                      # spin up the OpenMP team (256-thread pools take ~1 s to start)
    n = 512
    rate, dt = run(n)
    for _ in range(3):           # grow the sample towards ~cpu_seconds of work (bounded at 3072²)
        if dt >= 0.5 * args.cpu_seconds or n >= 3072:
            break
        n = int(min(3072, max(n + 8, n * (args.cpu_seconds / max(dt, 1e-3)) ** 0.5)))
        n -= n % 8
        rate, dt = run(n)
    return {"value": rate, "unit": "particle-steps/s", "cores": threads, "kind": "port",
            "sample": f"{n}x{n} periodic sub-box, same physics/winds, same {W}+{K} steps, {dt:.1f} s of CPU work "
                      f"(C oracle: OpenMP advance + node-parallel pull scatter, {threads} threads on the {cores} host cores this process may use)"}


KERNEL_SOURCES = ("kernels.h", "physics.h", "pmath.h", "pm_exp_tab.h", "k_step.inc", "k_step_explicit.hip")


def kernel_stamp():
    """sha256 over the sources of the dominant kernel: a PMC profile is only quoted for the kernel it was taken on"""
    import hashlib
    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        h.update((ROOT / "picles_amd" / "csrc" / f).read_bytes())
    return h.hexdigest()[:16]


def measured_traffic(args, world):
    """HBM bytes per launch of the dominant kernel from the committed PMC profile (rocprofv3 --pmc
    FETCH_SIZE / WRITE_SIZE in separate passes, FETCH doubled: profiles/*_pmc_summary.md) — only when
    the profile was taken on this exact workload AND on this exact kernel (the profile carries a hash of the
    kernel's sources: an edited kernel reports null until the PMC passes are collected again); PMC counters
    cannot be read live in a timed run."""
    f = next((q for q in (ROOT / "profiles" / "r4_pmc_traffic.json", ROOT / "profiles" / "r3_pmc_traffic.json") if q.exists()), None)
    try:
        d = json.loads(f.read_text())
        if (world == 1 and d["config"]["n"] == args.n and tuple(d["config"]["winds"]) == tuple(args.winds)
                and d.get("kernel_stamp") == kernel_stamp()
                and args.solver == "DP5" and args.deadband == 0.0 and not args.atomic):
            k = d["kernels"][d["dominant"]]
            return k["hbm_read_bytes"] + k["hbm_write_bytes"], k.get("valu_busy"), k.get("valu_insts_per_wave_steady", k.get("valu_insts_per_wave"))
    except Exception:
        pass
    return None, None, None


DUMP_NODES = 1 << 19     # nodes --dump-outputs writes at most: (3 + 5) float64 per node = 32 MB


def dump_outputs(model, out_dir, dist=None):
    """what the timed path computed in its last step, as a caller of it receives the model: the node State and the particle state,
    one row per node (global index i + Nx j), every node up to DUMP_NODES, above that a fixed, seeded sample of the nodes (sorted).
    Collective over the ranks of a slab run; rank 0 writes."""
    Nx, Ny = int(model.grid.stats.Nx), int(model.grid.stats.Ny)
    n = Nx * Ny
    idx = np.arange(n) if n <= DUMP_NODES else np.sort(np.random.default_rng(12345).choice(n, DUMP_NODES, replace=False))
    lo, hi = Nx * model.j0, Nx * model.j1
    sel = idx[(idx >= lo) & (idx < hi)] - lo
    s = model.get_state()                                   # completes the last step (picles_sync)
    z = model.backend.get_particles()[0]
    part = (s.reshape(-1, 3, order="F")[sel], z.reshape(-1, 5, order="F")[sel])
    parts = [part]
    if dist is not None:
        parts = [None] * model.world
        dist.all_gather_object(parts, part)
    if model.rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "state.npy"), np.concatenate([p[0] for p in parts]).astype(np.float64))
        np.save(os.path.join(out_dir, "particles.npy"), np.concatenate([p[1] for p in parts]).astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)      # the first launches after seeding take six and five RK attempts per particle; from the fifth on the step is steady
    ap.add_argument("--grid-n", dest="n", type=int, default=4096, help="grid nodes per side")
    ap.add_argument("--winds", type=lambda s: tuple(float(x) for x in s.split(",")), default=(10.0, 10.0))
    ap.add_argument("--halo", type=int, default=0,
                    help="halo rows = scatter reach the slabs cover; 0 = automatic: 1 while the run (clock conditioning cycles of <= 40 steps, "
                         "warm-up + timed steps) stays inside the ~45 steps for which the box's reach is 1 cell, else 2 (a particle beyond the halo "
                         "is counted and fails the run: halo overflow check); ignored for one GPU")
    ap.add_argument("--atomic", action="store_true", help="LDS-tiled atomic push scatter instead of the pull")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-events", action="store_true", help="diagnostic: no HIP events at all (roofline fields become meaningless)")
    ap.add_argument("--launch-events", action="store_true",
                    help="HIP events around EVERY launch inside the timed region (default on one GPU: one pair around the whole "
                         "region — an event between two dependent launches idles the GPU for about half a microsecond)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary measurements (generic wind direction, default solver)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--prewarm-ms", type=float, default=60.0,
                    help="GPU clock conditioning before the warm-up: about this many milliseconds of the same model steps, then a "
                         "re-seed (the model is back at t = 0 in its initial state), then the W warm-up and the K timed steps as "
                         "always.  A GPU that has idled needs tens of milliseconds of load before its waves run at full speed "
                         "(measured: a 4096 x 512 slab 0.341 -> 0.313 ms per step; DESIGN.md section 7.0): 5 warm-up steps of a "
                         "third of a millisecond each end long before that.  0 = off.")
    ap.add_argument("--deadband", type=float, default=0.0,
                    help="opt-in picles_phys.dir_deadband (0 = reference-exact RHS; the headline number uses 0)")
    ap.add_argument("--solver", default="DP5", choices=["DP5", "Tsit5", "AutoTsit5"],
                    help="ODE solver of the workload (the BASELINE box is quoted on DP5, as benchmarks/bench06 sets it)")
    ap.add_argument("--ring-of-one", action="store_true",
                    help="rehearsal on ONE GPU of the N > 1 host loop over the real transport: a one-rank RCCL group, edge / "
                         "interior launches on two streams, the halo blocks sent to ourselves every step")
    ap.add_argument("--python-loop", action="store_true",
                    help="drive the slab exchange from Python (torch.distributed P2P per step) instead of the native ring")
    ap.add_argument("--native-ring", action="store_true",
                    help="with --backend gloo: the library's own step loop (picles_slab_run_steps) over whatever communicator "
                         "PICLES_CCL_LIB names — the rehearsal of the N > 1 launch path on one GPU (tests/native/shm_ccl.cpp)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo = rehearsal of the N>1 path with all ranks on ONE GPU (halo staged through the host)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the CPU baseline (--no-cpu drops it), the secondary measurements "
                         "(--no-secondary drops them), the instrumented pass behind the timed region (min / median launch), the ring's "
                         "phase diagnosis and the state check.  Off: set up, warm up, time the K steps, dump, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what they computed as DIR/state.npy (node State: energy, momentum x, y) and "
                         f"DIR/particles.npy (the 5 particle components), float64, one row per node in global x-fastest order; above "
                         f"{DUMP_NODES} nodes a fixed, seeded sample of the nodes")
    args = ap.parse_args()

    # stdout carries the ONE JSON line and nothing else: whatever the runtime libraries print (RCCL's version banner and
    # warnings go to stdout by default) is sent to stderr by pointing fd 1 there for the duration of the run
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run for --gpus > 1")
        args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the product has no CPU path")
    if args.backend == "gloo":
        local_rank = 0            # rehearsal: every rank on the one GPU (RCCL itself refuses two ranks per device)
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        fallback = None
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
            # (SlabModel can fall back to host-staged halos over a second gloo group — fallback_group — if the in-place
            # exchange raises at warm-up; not opened here: RCCL send/recv straight from the library's record memory is
            # exercised on this stack by the ring-of-one test, and a second rendezvous is one more thing that can stall)
        else:
            dist.init_process_group("gloo")

    if world == 1 and args.ring_of_one and args.python_loop:
        import socket
        import torch.distributed as dist
        sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                                device_id=torch.device("cuda", local_rank))

    from picles_amd import configs, _capi as K
    from picles_amd.parallel import SlabModel

    PHASE_PASS = 3 + min(args.steps, 10)      # steps of the ring's phase diagnosis, run behind the timed region (ring_phase_pass)
    if args.halo <= 0:
        args.halo = 1 if (args.warmup + args.steps + PHASE_PASS) <= 40 else 2
    use_dist = world > 1
    flags = K.STEP_ZERO_FIRST | (K.STEP_ATOMIC if args.atomic else 0)
    W, Ksteps = args.warmup, args.steps

    def barrier(model):
        # device-wide synchronisation on both sides of the timed region, WITHOUT picles_sync: that call also completes ("flushes")
        # the scatter + remesh of the last step with a stand-alone launch.  In a run of fused steps launch k does the scatter +
        # remesh of step k-1 and the advance of step k; the region between two non-flushing barriers therefore holds exactly K
        # launches = K scatters + K remeshes + K advances — the same work as K steps, with nothing extra and nothing skipped.
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def measure(winds, solver, deadband, K_, W_, cfg=None, ring_of_one=None, halo=None):
        """seed, W_ warm-up steps, then EXACTLY K_ timed steps between barriers.  The timed region is ONE call into the
        library (picles_run_steps on one GPU, picles_slab_run_steps on a slab ring): no interpreter between the steps.
        `cfg`: another workload than the BASELINE box (the secondary legs)."""
        if cfg is None:
            cfg = configs.box4096(n=args.n, U10=winds[0], V10=winds[1])
            cfg.model["ODEsys"].dir_deadband = deadband
            cfg.model["ODEsets"].solver = solver
        ring1 = args.ring_of_one if ring_of_one is None else ring_of_one
        model = SlabModel(cfg.model, rank, world, device=local_rank, halo_rows=args.halo if halo is None else halo,
                          ring_of_one=ring1,
                          native_ring=True if args.native_ring else (None if (args.backend == "nccl" and not args.python_loop) else False))
        model.seed()
        # clock conditioning (--prewarm-ms): the same steps, un-timed, in cycles of at most 40 (the scatter reach of the box stays 1 that
        # long: no halo grows, nothing overflows), each followed by a re-seed — after the last one the model is exactly where
        # model.seed() left it.  The number of steps is a function of the grid alone: every rank runs the same.
        pre_steps = 0
        if args.prewarm_ms > 0:
            per_rank = int(model.grid.stats.Nx) * (model.j1 - model.j0)
            pre_steps = int(min(4000, max(5, math.ceil(args.prewarm_ms * 1e-3 * 6.5e9 / per_rank))))
            left = pre_steps
            while left > 0:
                model.run_steps(cfg.Δt, min(left, 40), flags)
                left -= 40
                model.seed()
        model.prewarm_steps = pre_steps
        model.run_steps(cfg.Δt, W_, flags)
        model.backend.reset_counters()
        # one GPU: the K launches are back to back on one stream — ONE event pair around them (mean launch = region / K).
        # Slabs (native ring): ONE pair as well, on the stream of the interior launches, into which every step's edge launch is
        # ordered — pairs around every launch plus the five phase events of the diagnosis cost a 2 M-particle slab 9 % of its step
        # (ring of one at 1448^2: 0.306 ms without events, 0.333 with): the diagnosis has a pass of its own (ring_phase_pass)
        region_ok = (not args.atomic and not args.launch_events and
                     ((world == 1 and not ring1) or getattr(model, "native", False)))
        model.backend.enable_timing(0 if args.no_events else (2 if region_ok else 1))
        model.timing_region = bool(region_ok) and not args.no_events
        barrier(model)
        t0 = time.perf_counter()
        model.run_steps(cfg.Δt, K_, flags)
        model.host_enqueue_s = time.perf_counter() - t0      # host side of the step loop (the launches are asynchronous)
        barrier(model)
        return model, time.perf_counter() - t0

    model, elapsed = measure(args.winds, args.solver, args.deadband, Ksteps, W)

    cnt = model.backend.get_counters()
    tim = model.backend.get_timing()
    if args.dump_outputs:
        dump_outputs(model, args.dump_outputs, dist if use_dist else None)
    # where each rank's ring steps went (edge launch / exchange / interior launch, and whether the exchange was hidden behind the
    # interior launch): one line of diagnosis per rank for the multi-GPU run, from events the ring records itself
    def ring_phase_pass(m, dt):
        """where a ring step goes (edge launch / exchange / interior launch, was the exchange hidden): events around every launch and
        phase, in a pass of min(K, 10) steps BEHIND the timed region (three un-instrumented steps first: reading the timers completed
        the pending step with a stand-alone launch, the ring is fused again from the second step on)"""
        if getattr(m, "timing_region", False):
            m.run_steps(dt, 3, flags)
            m.backend.enable_timing(1)
            m.run_steps(dt, min(Ksteps, 10), flags)
        return m.backend.slab_phases()

    slab_phases = None
    if args.full and model.native and not args.no_events:
        ph = ring_phase_pass(model, configs.box4096(n=args.n).Δt)
        row = torch.tensor([float(rank), float(ph["steps"]), float(ph["exchange_hidden_steps"]), ph["edge_ms"], ph["exchange_ms"],
                            ph["interior_ms"], ph["slack_ms"], ph["span_ms"]], dtype=torch.float64,
                           device="cuda" if args.backend == "nccl" else "cpu")
        rows = [row]
        if use_dist:
            rows = [torch.zeros_like(row) for _ in range(world)]
            dist.all_gather(rows, row)
        slab_phases = [{"rank": int(r[0]), "steps": int(r[1]), "exchange_hidden_steps": int(r[2]), "edge_ms": float(r[3]),
                        "exchange_ms": float(r[4]), "interior_ms": float(r[5]), "exchange_end_to_interior_end_ms": float(r[6]),
                        "step_span_ms": float(r[7])} for r in rows]
    launch_samples = None
    if (args.full and world == 1 and not args.no_events and not args.launch_events and not args.ring_of_one and not args.atomic):
        # spread of the launch durations: a SEPARATE instrumented pass (events around every launch) right behind the timed region —
        # a few un-timed launches first, so that the pass does not start on a GPU that idled (and clocked down) during the readback
        model.run_steps(configs.box4096(n=args.n).Δt, 3, flags)
        model.backend.enable_timing(1)
        model.run_steps(configs.box4096(n=args.n).Δt, min(Ksteps, 10), flags)
        torch.cuda.synchronize()
        model.backend.get_timing()
        launch_samples = np.sort(model.backend.get_timing_samples(0))
    n_local = model.n_stepped
    vals = torch.tensor([elapsed, float(n_local), float(cnt["rhs_evals"]), float(cnt["halo_overflow"]),
                         float(cnt["steps_accepted"]), float(cnt["steps_rejected"])], dtype=torch.float64,
                        device="cuda" if args.backend == "nccl" else "cpu")
    if use_dist:
        mx = vals.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        dist.all_reduce(vals, op=dist.ReduceOp.SUM)
        elapsed = float(mx[0])
    n_total = float(vals[1])
    rhs_total = float(vals[2])
    overflow = float(vals[3])
    if overflow > 0:
        raise SystemExit(f"halo overflow ({overflow} particles travelled beyond --halo {args.halo}): result invalid")
    # result check outside the timed region: the BASELINE box is homogeneous and periodic, so after any number of steps the
    # energy plane must be one value on every node of every slab (a lost or doubled halo row, a wrong neighbour across a slab
    # seam or a stale ghost row breaks it at the seams)
    state_check = None
    # (not for --atomic: the atomic push sums in run-dependent order, and that last-bit noise is amplified by the stiff direction
    # mode to the solver tolerance — DESIGN.md §3; the headline path is the deterministic pull)
    if args.full and (args.winds[0] == args.winds[1] or world > 1) and not args.atomic:
        e = model.get_state()[..., 0]
        ext = torch.tensor([float(e.min()), -float(e.max())], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        if use_dist:
            dist.all_reduce(ext, op=dist.ReduceOp.MIN)
        emin, emax = float(ext[0]), -float(ext[1])
        state_check = {"e_min": emin, "e_max": emax, "rel_spread": (emax - emin) / emax}
        if not (emin > 0 and state_check["rel_spread"] < 1e-6):
            raise SystemExit(f"State check failed: the homogeneous periodic box is not uniform across the {world} slab(s): {state_check}")
        del e

    if rank == 0:
        value = n_total * Ksteps / elapsed
        adv_ms = tim["advance_ms"] / max(tim["advance_launches"], 1)
        launches_per_step = max(tim["advance_launches"], 1) / Ksteps
        # dominant kernel: k_advance.  algorithmic bytes per launch = B_ALG × particles a launch advances
        per_launch = n_local / launches_per_step
        achieved = B_ALG * per_launch / (adv_ms * 1e-3) / 1e9 if adv_ms > 0 else 0.0
        rhs_per_ps = rhs_total / (n_total * Ksteps)
        tflops = rhs_total * FLOP_PER_RHS / elapsed / 1e12
        traffic, valu_busy, valu_per_wave = measured_traffic(args, world)
        out = {
            "metric": "particle_steps_per_sec",
            "value": value,
            "unit": "particle-steps/s",
            "n_gpus": world,
            "steps": Ksteps,
            "warmup": W,
            "ms_per_step": 1e3 * elapsed / Ksteps,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": f"box{args.n}: {args.n}x{args.n} TwoDCartesianGridMesh, periodic, 1 particle/cell, "
                            f"constant winds ({args.winds[0]:g},{args.winds[1]:g}), dx=2000 m, dt=600 s, bench06 physics "
                            f"(C_phi=0.04, gamma=0.88, {args.solver} abstol 1e-4 reltol 1e-3, lne_max=log 27)",
                "grid": [args.n, args.n],
                "particles": int(n_total),
                "parallelism": f"y-slabs x{world}, forward halo of scatter records ({args.halo} row) over "
                               + ("RCCL send/recv" if not (world > 1 and model.ex is not None and model.ex.staged) else "host-staged gloo send/recv (fallback)"),
                "scatter": "atomic-push" if args.atomic else "deterministic-pull",
                "dir_deadband": args.deadband,
            },
            "hbm_GBps_path": B_ALG * value / 1e9,
            "roofline": {
                "kernel": "k_step (fused scatter+remesh+advance, one launch per model step; per row range for slabs)",
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBPS,
                "traffic": traffic,
                "avg_launch_ms": adv_ms,
                "note": "the fused RK advance is fp64-VALU bound, not HBM bound (DESIGN.md): see fp64",
            },
            "fp64": {
                "rhs_evals_per_particle_step": rhs_per_ps,
                "flop_per_rhs": FLOP_PER_RHS,
                "achieved_tflops": tflops,
                "peak_tflops": FP64_PEAK_TFLOPS * world,
                "frac": tflops / (FP64_PEAK_TFLOPS * world),
                # from the committed PMC profile of this exact workload (profiles/r4_pmc_traffic.json, quoted only while its kernel stamp matches the tree), null otherwise
                "valu_issue_busy": valu_busy,
                "valu_insts_per_wave": valu_per_wave,
            },
            "kernel_ms_per_step": {"step_or_advance": tim["advance_ms"] / Ksteps, "scatter_remesh": tim["scatter_ms"] / Ksteps,
                                   "remesh": tim["remesh_ms"] / Ksteps},
        }
        samples = np.sort(model.backend.get_timing_samples(0)) if launch_samples is None else launch_samples
        out["roofline"]["launches"] = int(tim["advance_launches"])
        out["roofline"]["events"] = ("one pair around the timed region" if (launch_samples is not None or getattr(model, "timing_region", False))
                                     else "one pair per launch")
        if getattr(model, "timing_region", False) and model.native:
            out["roofline"]["events"] += (" on the interior stream of the ring; avg_launch_ms = region / launches (edge + interior launch of a "
                                          "step overlap: two launches per step)"
                                          + ("; phase diagnosis in a separate pass behind it" if slab_phases is not None else ""))
        if launch_samples is not None:
            samples = launch_samples
            out["roofline"]["launch_samples"] = (f"separate pass of {samples.size} launches with per-launch events, right behind the timed region "
                                                 "(the GPU kept busy in between)")
        if samples.size:
            out["roofline"]["min_launch_ms"] = float(samples[0])
            out["roofline"]["median_launch_ms"] = float(np.median(samples))
        out["state_check"] = state_check
        if slab_phases is not None:
            out["slab_phases"] = {"per_rank": slab_phases,
                                  "note": "per-step means [ms] from the ring's own events: edge launch (stream E), end of the edge launch -> "
                                          "end of the RCCL send/recv group (stream E), interior launch (stream M); "
                                          "exchange_end_to_interior_end > 0 = the exchange had completed before the interior launch ended (hidden)"}
        out["config"]["host_enqueue_us_per_step"] = 1e6 * model.host_enqueue_s / Ksteps
        out["config"]["clock_prewarm"] = {"target_ms": args.prewarm_ms, "untimed_steps": model.prewarm_steps,
                                          "note": "un-timed steps of the same model followed by a re-seed, before the W warm-up steps "
                                                  "(GPU clock conditioning; 0 = off: --prewarm-ms 0)"}
        out["config"]["step_loop"] = ("native: picles_slab_run_steps (RCCL send/recv issued from C)" if model.native else
                                      ("native: picles_run_steps" if (world == 1 and not args.atomic and model.ex is None) else
                                       "python: one C call per step" + ("" if world == 1 else ", torch.distributed P2P")))
        if args.full and world == 1 and not args.no_secondary and not args.atomic and not args.ring_of_one:
            # the honest spread: the BASELINE winds (10,10) are the best case of the explicit pair; a generic
            # wind direction and the reference's DEFAULT solver, same box, same process
            del model
            sec = []
            K2 = max(3, min(Ksteps, 10))
            for winds, solver in (((10.0, 3.0), "DP5"), ((10.0, 3.0), "AutoTsit5"), ((10.0, 10.0), "AutoTsit5")):
                if tuple(winds) == tuple(args.winds) and solver == args.solver:
                    continue
                m2, el2 = measure(winds, solver, 0.0, K2, W)          # the same warm-up as the headline: past the ramp-up launches
                c2 = m2.backend.get_counters()
                t2 = m2.backend.get_timing()
                sm = np.sort(m2.backend.get_timing_samples(0))
                rate = m2.n_stepped * K2 / el2
                rps = c2["rhs_evals"] / max(m2.n_stepped * K2, 1)
                tf = c2["rhs_evals"] * FLOP_PER_RHS / el2 / 1e12
                sec.append({"winds": list(winds), "solver": solver, "steps": K2, "warmup": W, "ms_per_step": 1e3 * el2 / K2, "value": rate,
                            "rhs_evals_per_particle_step": rps, "fp64_frac": tf / FP64_PEAK_TFLOPS,
                            "hbm_frac": B_ALG * rate / 1e9 / HBM_PEAK_GBPS,
                            "kernel_ms_mean": t2["advance_ms"] / max(t2["advance_launches"], 1),
                            "kernel_ms_min_median": [float(sm[0]), float(np.median(sm))] if sm.size else None,
                            "halo_overflow": int(c2["halo_overflow"])})
                del m2
            out["secondary"] = sec
            # what rounds 3-4 optimised and the 5+20-step window of the headline never reaches: each leg on its own,
            # a failure is recorded in its place and never touches the headline
            ext = {}

            def leg(name, fn):
                try:
                    ext[name] = fn()
                except BaseException as e:       # noqa: BLE001 (SystemExit from a check included)
                    ext[name] = {"error": repr(e)}

            def summary(m2, el2, K_, W_):
                c2, t2 = m2.backend.get_counters(), m2.backend.get_timing()
                att = c2["steps_accepted"] + c2["steps_rejected"]
                kms = t2["advance_ms"] / max(t2["advance_launches"], 1)
                return {"steps": K_, "warmup": W_, "ms_per_step": 1e3 * el2 / K_, "value": c2["particles_advanced"] / el2,
                        "kernel_ms_mean": kms, "launches": int(t2["advance_launches"]),
                        "particles_on_per_step": c2["particles_advanced"] / K_,
                        "rhs_evals_per_particle_step": c2["rhs_evals"] / max(c2["particles_advanced"], 1),
                        "rhs_per_s": c2["rhs_evals"] / el2,
                        "lane_efficiency": att / max(c2.get("wave_attempt_slots", 0), 1),
                        "max_reach": int(c2["max_reach_seen"]), "halo_overflow": int(c2["halo_overflow"]), "reseeds": int(c2["reseeds"])}

            def cfg5():
                # BASELINE config 5 (2048², growing / decaying winds x cos(3t/(3600·2π)), 20-minute steps, the reference's default
                # solver) on its CONFORMANT device path: the forcing as a lattice with time knots at dt/2, three levels sampled on the
                # device per step (SMOOTH3) — the path tests/test_step2d_fixture.py::test_config5_forcing_through_a_smooth3_lattice
                # holds to the stage-time fixture at 1e-3; no host closure evaluation in the loop
                K5, W5 = 58, 2
                m5, el5 = measure(None, None, 0.0, K5, W5, cfg=configs.growing_decaying_winds_lattice(n=2048, n_steps=K5 + W5 + 42))
                r5 = summary(m5, el5, K5, W5)
                del m5
                def bx2():
                    b_ = configs.box4096(n=2048)
                    b_.model["ODEsets"].solver = "AutoTsit5"
                    return b_
                bx = bx2()
                mb, elb = measure(None, None, 0.0, 20, 5, cfg=bx)
                rb = summary(mb, elb, 20, 5)
                del mb
                r5["workload"] = "cfg5: 2048x2048 non-periodic, winds ramp(x) x cos(3t/(3600 2pi)) as a device lattice (SMOOTH3, knots at dt/2), dt = 1200 s, AutoTsit5"
                r5["homogeneous_box_2048_AutoTsit5"] = {k: rb[k] for k in ("ms_per_step", "rhs_per_s", "rhs_evals_per_particle_step", "lane_efficiency")}
                r5["rhs_rate_over_homogeneous_box"] = r5["rhs_per_s"] / rb["rhs_per_s"]
                # ... and the same box through config 5's own kernel flavour and wind path (its constant winds as a SMOOTH3 device lattice:
                # three device-sampled levels per step, stage winds interpolated in time): "same solver and kernel flavour" 
                bl = configs.closure_lattice(bx2(), 20 + 5 + 2, x=[0.0, 2000.0 * 2047], y=[0.0, 2000.0 * 2047])
                ml, ell = measure(None, None, 0.0, 20, 5, cfg=bl)
                rl = summary(ml, ell, 20, 5)
                del ml
                r5["homogeneous_box_2048_same_flavour"] = {k: rl[k] for k in ("ms_per_step", "rhs_per_s", "rhs_evals_per_particle_step", "lane_efficiency")}
                r5["rhs_rate_over_same_flavour_box"] = r5["rhs_per_s"] / rl["rhs_per_s"]
                return r5

            def reach2():
                # the developed sea: from step ~45 on the scatter reach of the BASELINE box is 2 cells (25 pull candidates per node)
                m3, el3 = measure(args.winds, args.solver, 0.0, 10, 60)
                r3 = summary(m3, el3, 10, 60)
                r3["workload"] = f"the headline box, steps 61-70 after seeding (scatter reach {r3['max_reach']})"
                del m3
                return r3

            def slab_shape(ring1):
                # the per-rank work of the 8-GPU run: a 4096 x 512 box of the same physics (the homogeneous box is homogeneous at any
                # size), plain and as a ring of one (edge / interior launches on two streams, the halo blocks sent to ourselves by RCCL)
                from picles_amd.grids import TwoDCartesianGridMesh
                cs = configs.box4096(n=4096, U10=args.winds[0], V10=args.winds[1])
                cs.model["ODEsets"].solver = args.solver
                cs.model["grid"] = TwoDCartesianGridMesh(0.0, 2000.0 * 4095, 4096, 0.0, 2000.0 * 511, 512, periodic_boundary=(True, True))
                ms, els = measure(None, None, 0.0, Ksteps, W, cfg=cs, ring_of_one=ring1, halo=1)
                rs = summary(ms, els, Ksteps, W)
                rs["workload"] = "4096 x 512 periodic box (one rank's slab of the 8-GPU run)" + (", ring of one over RCCL" if ring1 else ", plain context")
                rs["frac_of_linear"] = (1e3 * elapsed / Ksteps / 8) / rs["ms_per_step"]
                if ring1 and ms.native:
                    rs["slab_phases"] = ring_phase_pass(ms, cs.Δt)
                del ms
                return rs

            if args.n == 4096:
                leg("cfg5_conformant_device_lattice", cfg5)
                leg("box_reach2", reach2)
                leg("slab_4096x512", lambda: slab_shape(False))
                leg("slab_4096x512_ring_of_one", lambda: slab_shape(True))
            out["secondary_legs"] = ext
        if args.full and world == 1 and not args.no_cpu:
            try:
                out["cpu_baseline"] = cpu_baseline(args, W, Ksteps)
            except Exception as e:  # the baseline is reported, never required for the GPU number
                out["cpu_baseline"] = {"value": None, "error": repr(e)}
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
