"""Simulation / run! / init_particles! (reference: src/Simulations/simulation.jl:11-98,
src/Simulations/run.jl:36-146,199-247; CashStore: storing.jl:7-25; the HDF5 StateStore is picles_amd/storing.py)."""
from __future__ import annotations

import math
import time

import numpy as np

from .checkpointing import load_checkpoint, resolve_pickup
from .output_writers import PHASE_ORDER, in_phase, writers_of
from .storing import NpyStateStore, StateStore, make_state_store
from .timesteppers import time_step


class CashStore:
    def __init__(self):
        self.store = []
        self.iteration = 1


def init_state_store(sim, save_path, name="state", format="auto"):
    """init_state_store!(sim, save_path) (storing.jl:83-104): `time` runs to stop_time + Δt (run! takes one step past stop_time).
    format "hdf5" = the reference's file (picles_amd/storing.py), "npy" = the same layout as a NumPy memory map, "auto" = hdf5
    where a libhdf5 loads"""
    g = sim.model.grid
    times = np.arange(0.0, sim.stop_time + sim.Δt + 0.5 * sim.Δt, sim.Δt)
    sim.store = make_state_store(save_path, times, g.data.x[:, 0], g.data.y[0, :], name=name, format=format)
    return sim.store


def push_state_to_storage(sim, i=None):
    """push_state_to_storage!(sim; i) (storing.jl:109-119)"""
    sim.store.write(sim.model.State, i=i)


def reset_state_store(sim, value=0.0):
    """reset_state_store!(sim; value) (storing.jl:127-131)"""
    sim.store.reset(value)


def close_store(sim):
    """close_store!(sim) (storing.jl:178-180)"""
    sim.store.close()


class Simulation:
    def __init__(self, model, Δt: float, verbose=False, stop_iteration=float("inf"),
                 stop_time=float("inf"), wall_time_limit=float("inf")):
        self.model, self.Δt = model, float(Δt)
        self.stop_iteration, self.stop_time, self.wall_time_limit = stop_iteration, stop_time, wall_time_limit
        self.run_wall_time = 0.0
        self.running = False
        self.initialized = False
        self.verbose = verbose
        self.store = None
        self.output_writers = {}      # Oceananigans' output_writers; run() drives a Checkpointer found here (picles_amd/checkpointing.py)


def init_particles(model, defaults=None, verbose=False):
    """init_particles!(model) (run.jl:199-247): seed every node from the winds at t = 0 with the
    time scale ODEsettings.timestep, write the seeds' (e, m_x, m_y) into State."""
    model._wind_window = None
    model.upload_winds(0.0, model.ODEsettings.timestep, seeding=True)
    model.backend.seed(model.clock.time)


def initialize_simulation(sim: Simulation):
    """run.jl:130-146"""
    init_particles(sim.model, defaults=sim.model.ODEdefaults, verbose=sim.verbose)
    if sim.model.clock.iteration != 0:
        sim.model.clock.iteration = 0
        sim.model.clock.time = 0.0
        sim.model.backend.seed(0.0)
    sim.initialized = True


def reset_simulation(sim: Simulation):
    """reset_simulation!(sim) (run.jl:154-181): clock to zero, particles re-seeded, **State cleared** (so a following run!
    stores zeros as its initial state — the reference's behaviour), the state store reset"""
    sim.running = False
    sim.run_wall_time = 0.0
    sim.model.clock.time = 0.0
    sim.model.clock.iteration = 0
    init_particles(sim.model, defaults=sim.model.ODEdefaults, verbose=sim.verbose)
    sim.model.State.fill(0.0)
    sim.initialized = True
    if isinstance(sim.store, (StateStore, NpyStateStore)):
        sim.store.reset()


def run(sim: Simulation, store=False, pickup=False, cash_store=False, debug=False):
    """run!(sim) (run.jl:36-122): note `stop_time >= clock.time`, i.e. one step past stop_time.
    pickup=True: continue from the latest file of the Checkpointer in sim.output_writers; pickup=<path>: from that file (the seeding of
    initialize_simulation is skipped, the clock restored; the reference accepts the keyword and ignores it, run.jl:36).  A Checkpointer
    in sim.output_writers writes a file every `schedule` iterations.
    The entries of sim.output_writers are driven through the hooks of picles_amd/output_writers.py, each phase in its own order
    (DESIGN.md §16); a writer the backend cannot serve is refused before anything is loaded or seeded."""
    t0 = time.perf_counter_ns()
    if store and not isinstance(sim.store, (StateStore, NpyStateStore)):
        raise ValueError("call init_state_store(sim, path) before run(sim, store=True)")
    m = sim.model
    ring = store and hasattr(m.backend, "store_init")
    writers = writers_of(sim)
    picked = resolve_pickup(sim, pickup) if pickup is not False and pickup is not None else None     # which file: nothing is loaded yet
    for w in writers:
        if not hasattr(m.backend, w.needs):
            raise NotImplementedError(w.refusal)
    for w in writers:
        w.check_run(sim, writers, store=store, cash_store=cash_store, pickup=picked is not None)
    phase = {p: in_phase(writers, p) for p in PHASE_ORDER}
    if picked is not None:
        for w in writers:
            w.check_pickup(picked)             # e.g. the parent's file and the link side-car of a nested pair: nothing is loaded yet
        load_checkpoint(m, picked, sim.Δt)
        sim.initialized = True
        for w in writers:
            w.load_pickup(picked)              # e.g. the open statistics window of the run that wrote the checkpoint
    if not sim.initialized:
        initialize_simulation(sim)
    sim.run_wall_time = 0.0
    sim.running = sim.stop_time >= m.clock.time
    if cash_store:
        sim.store = CashStore()
        sim.store.iteration += 1
        sim.store.store.append(m.State.copy())
    if store:
        sim.store.write(m.State)          # initial state (run.jl:62-69)
        if ring and not getattr(m.backend, "_store_ready", False):
            m.backend.store_init(3)
            m.backend._store_ready = True
    # steps to take (run.jl:113 loops while `stop_time >= clock.time`: one step past stop_time); None without a finite stop_time
    n = 0 if not sim.running else None if sim.stop_time == float("inf") else int(math.floor((sim.stop_time - m.clock.time) / sim.Δt)) + 1
    # nothing observes State between the steps: enqueue the whole loop from C, in one call or in chunks between the writers' iterations
    # (static winds, a lattice the device samples or levels streamed into its ring: WaveGrowth2D.runs_chunked; closures that vary in
    # time take the per-step loop)
    chunk_winds = m.runs_chunked(sim.Δt) if hasattr(m, "runs_chunked") else getattr(m, "_winds_static", False)
    chunked = not store and not cash_store and hasattr(m.backend, "run_steps") and chunk_winds and n is not None
    if chunked and n > 0:
        m.upload_winds(m.clock.time, sim.Δt)
    if writers and sim.running:
        if n is None and any(w.sized_for_run for w in writers):
            raise ValueError("a FieldWriter, StationWriter or StatisticsWriter needs a finite stop_time (its file is sized for the run)")
        for w in phase["begin_run"]:
            w.begin_run(m, n)                 # the files are sized for the run; the record of the first iteration
    if chunked:
        # chunks that end on the next output, checkpoint or statistics-window iteration or where the probe ring would fill, whichever is first:
        # the snapshot of chunk k is copied out and written — and the station samples of chunk k-1 are — while chunk k+1 runs
        time0, it0, done = m.clock.time, m.clock.iteration, 0
        while done < n:
            k = min([n - done] + [w.steps_allowed(m.backend, it0 + done) for w in writers])
            if hasattr(m, "wind_steps_allowed"):
                k = m.wind_steps_allowed(sim.Δt, k)      # streamed winds: the steps the levels held on the device cover
            m.backend.run_steps(sim.Δt, k)
            for w in phase["after_chunk"]:
                w.after_chunk(m.backend)
            done += k
            m.clock.time = time0 + done * sim.Δt
            m.clock.iteration = it0 + done
            for w in phase["at_iteration"]:
                w.at_iteration(m, writers)
        sim.running = False
    while sim.running:                     # the per-step loop (time-varying winds, stores)
        for w in writers:
            w.before_step(m.backend)       # the library samples inside time_step
        m.State.fill(0.0)                  # State .= 0 (run.jl:75-79): recorded by the lazy view, fused into the scatter's store
        time_step(m, sim.Δt, debug=debug)
        if store:
            if ring:   # asynchronous: D2H of step k overlaps the kernels of steps k+1, k+2
                if m.backend.store_pending == 3:
                    sim.store.write(m.backend.store_pop()[0])
                m.backend.store_push()
            else:
                sim.store.write(m.State)
        if cash_store:
            sim.store.store.append(m.State.copy())
            sim.store.iteration += 1
        for w in phase["at_iteration"]:
            w.at_iteration(m, writers)
        sim.running = sim.stop_time >= m.clock.time
    for w in phase["finish"]:
        w.finish(m.backend, m.clock.iteration)
    if store:
        if ring:
            while m.backend.store_pending:
                sim.store.write(m.backend.store_pop()[0])
        sim.store.close()
    m.backend.sync() if hasattr(m.backend, "sync") else None
    if hasattr(m, "check_counters"):
        m.check_counters()         # particles beyond the reach cap / with non-finite positions were not scattered: say so
    sim.run_wall_time += 1e-9 * (time.perf_counter_ns() - t0)
