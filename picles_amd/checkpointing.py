"""Checkpointer / pickup: exact restart of a run (the Oceananigans surface the reference's `run!(sim; pickup)` is modelled on,
src/Simulations/run.jl:36, where the keyword is accepted and ignored).

A checkpoint file holds the library's blob (picles_checkpoint_*: the prognostic state of the model at a step boundary)
plus the host clock.  The configuration is not in it: the restoring script builds the same model and `run(sim, pickup=True)`
loads the latest file into it; the library refuses a blob written by a model of another configuration.

File layout (little-endian):  8 bytes magic b"PICLESCF" | u32 version | i32 rank (-1: a whole-grid model) | i64 iteration |
f64 clock time | u64 blob bytes | the blob.  Name: `{prefix}_iteration{i}.picles`, `{prefix}_iteration{i}_rank{r}.picles` for a slab.
Every file is written to a temporary name, flushed, fsync'ed and renamed: a job killed mid-write leaves no file that pickup would
choose.
"""
from __future__ import annotations

import os
import re
import struct
from pathlib import Path

import numpy as np

from . import _capi as K
from .output_writers import OutputWriter, find_writer, writers_of

FILE_MAGIC = b"PICLESCF"
FILE_VERSION = 1
_HEAD = struct.Struct("<8sIiqdQ")          # 40 bytes
SUFFIX = ".picles"


class IterationInterval:
    """schedule: every `interval` iterations (Oceananigans.IterationInterval)"""

    def __init__(self, interval: int):
        if int(interval) < 1:
            raise ValueError("IterationInterval needs interval >= 1")
        self.interval = int(interval)

    def __call__(self, iteration: int) -> bool:
        return iteration > 0 and iteration % self.interval == 0

    @classmethod
    def of(cls, schedule):
        """a schedule given as an IterationInterval or as an int (every that many iterations)"""
        return schedule if isinstance(schedule, cls) else cls(int(schedule))

    def next_after(self, iteration: int) -> int:
        return (iteration // self.interval + 1) * self.interval

    def records_of(self, it0: int, n_steps: int) -> int:
        """records a run of n_steps from iteration it0 writes: the first iteration's and one per scheduled iteration after it"""
        return 1 + (it0 + n_steps) // self.interval - it0 // self.interval

    def first_step(self, it0: int) -> int:
        """the library's step counter (steps since a set was created at iteration it0) of the first scheduled iteration"""
        return self.interval - it0 % self.interval


def checkpoint_path(dir, prefix: str, iteration: int, rank=None) -> Path:
    name = f"{prefix}_iteration{int(iteration)}" + (f"_rank{int(rank)}" if rank is not None else "") + SUFFIX
    return Path(dir) / name


def write_checkpoint_file(path, blob, time: float, iteration: int, rank=None) -> Path:
    """atomic: temporary file in the same directory, flush + fsync, rename, fsync of the directory"""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob, dtype=np.uint8)
    tmp = path.with_name(f".{path.name}.tmp-{os.getpid()}")
    try:
        with open(tmp, "wb") as f:
            f.write(_HEAD.pack(FILE_MAGIC, FILE_VERSION, -1 if rank is None else int(rank), int(iteration), float(time), blob.size))
            f.write(memoryview(blob))
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    try:
        fd = os.open(path.parent, os.O_RDONLY)
        try:
            os.fsync(fd)
        finally:
            os.close(fd)
    except OSError:
        pass
    return path


def read_checkpoint_file(path):
    """-> (blob: np.uint8 array, time, iteration, rank); refuses a truncated or foreign file before it reaches the library"""
    path = Path(path)
    raw = path.read_bytes()
    if len(raw) < _HEAD.size:
        raise K.CheckpointError(0, f"{path}: not a checkpoint file (only {len(raw)} bytes)")
    magic, version, rank, iteration, time, nblob = _HEAD.unpack_from(raw)
    if magic != FILE_MAGIC:
        raise K.CheckpointError(0, f"{path}: not a checkpoint file (bad magic)")
    if version != FILE_VERSION:
        raise K.CheckpointError(0, f"{path}: checkpoint file version {version}, this reader knows {FILE_VERSION}")
    if len(raw) - _HEAD.size != nblob:
        raise K.CheckpointError(0, f"{path}: truncated or padded checkpoint file ({len(raw) - _HEAD.size} blob bytes, header says {nblob})")
    blob = np.frombuffer(raw, dtype=np.uint8, offset=_HEAD.size)
    if nblob < K.CKPT_HEADER_BYTES or struct.unpack_from("<Q", raw, _HEAD.size)[0] != K.CKPT_MAGIC:
        raise K.CheckpointError(0, f"{path}: the file does not hold a checkpoint blob")
    return blob, time, iteration, (None if rank < 0 else rank)


def list_checkpoints(dir, prefix: str = "checkpoint", rank=None):
    """{iteration: path} of the finished checkpoint files of `prefix` (and `rank`) in dir; temporary files do not match"""
    d = Path(dir)
    if not d.is_dir():
        return {}
    pat = re.compile(re.escape(prefix) + r"_iteration(\d+)" + (rf"_rank{int(rank)}" if rank is not None else "") + re.escape(SUFFIX) + "$")
    out = {}
    for f in d.iterdir():
        m = pat.fullmatch(f.name)
        if m and f.is_file():
            out[int(m.group(1))] = f
    return out


def latest_checkpoint(dir, prefix: str = "checkpoint", rank=None, world=None):
    """the file with the highest iteration; for the ranks of a slab run (world given) the highest iteration ALL ranks have a
    file for, so that every rank picks the same one.  None if there is none."""
    if world is None:
        found = list_checkpoints(dir, prefix, rank)
        return found[max(found)] if found else None
    per = [list_checkpoints(dir, prefix, r) for r in range(int(world))]
    common = set(per[0]).intersection(*per[1:]) if per else set()
    return per[int(rank)][max(common)] if common else None


class Checkpointer(OutputWriter):
    """Checkpointer(model; schedule, dir, prefix) of Oceananigans: attach with `sim.output_writers["checkpointer"] = ...`.
    `schedule` is an IterationInterval or an int (every that many iterations).  `rank`: a slab model's rank (file per rank)."""

    kind = "checkpointer"
    needs = "checkpoint_begin"
    refusal = "a Checkpointer needs a backend with checkpoint_begin / checkpoint_end (the HIP library)"

    def __init__(self, model=None, *, schedule=None, dir=".", prefix: str = "checkpoint", rank=None):
        if schedule is None:
            raise ValueError("Checkpointer needs a schedule (IterationInterval(N) or N)")
        self.model = model
        self.schedule = IterationInterval.of(schedule)
        self.dir = Path(dir)
        self.prefix = prefix
        self.rank = rank
        self._inflight = None            # (path, time, iteration) of the checkpoint whose copy-out is running
        self.written = []

    @property
    def interval(self) -> int:
        return self.schedule.interval

    def begin(self, backend, time: float, iteration: int):
        """snapshot now; the file is written by finish(), after the next steps have been enqueued"""
        self.finish(backend)
        backend.checkpoint_begin()
        self._inflight = (checkpoint_path(self.dir, self.prefix, iteration, self.rank), float(time), int(iteration))

    def steps_allowed(self, backend, iteration: int) -> int:
        return self.schedule.next_after(iteration) - iteration

    def at_iteration(self, model, writers):
        """the file of the previous snapshot, then — on a scheduled iteration — the next snapshot, and word of it to every writer"""
        it = model.clock.iteration
        self.finish(model.backend)
        if self.schedule(it):
            self.begin(model.backend, model.clock.time, it)
            for w in writers:
                w.checkpoint_begun(model.backend, self._inflight[0])

    def finish(self, backend, iteration=None):
        if self._inflight is None:
            return None
        path, time, iteration = self._inflight
        self._inflight = None
        blob = backend.checkpoint_end()
        write_checkpoint_file(path, blob, time, iteration, self.rank)
        self.written.append(path)
        return path

    after_chunk = finish                 # the snapshot taken before the chunk: its copy-out ran beside the chunk's kernels

    def latest(self, world=None):
        return latest_checkpoint(self.dir, self.prefix, self.rank, world)


def resolve_pickup(sim, pickup):
    """pickup=True: the latest file of the simulation's Checkpointer; a path: that file"""
    if pickup is True:
        ck = find_writer(sim, Checkpointer)
        if ck is None:
            raise K.CheckpointError(0, "run(sim, pickup=True) needs a Checkpointer in sim.output_writers (or pass pickup=<path>)")
        others = [w for w in writers_of(sim) if w is not ck]
        found = list_checkpoints(ck.dir, ck.prefix, ck.rank)
        if not found:
            raise K.CheckpointError(0, f"run(sim, pickup=True): no checkpoint file '{ck.prefix}_iteration*{SUFFIX}' in {ck.dir}")
        # the latest file whose companions (the parent's file and the link side-car of a nested pair) are complete: a job killed
        # between two of them leaves a file that is passed over
        for it in sorted(found, reverse=True):
            if all(Path(f).is_file() for w in others for f in w.pickup_companions(found[it])):
                return found[it]
        lacking = [str(f) for w in others for f in w.pickup_companions(found[max(found)]) if not Path(f).is_file()]
        raise K.CheckpointError(0, f"run(sim, pickup=True): no checkpoint of '{ck.prefix}' in {ck.dir} is complete (the latest lacks {', '.join(lacking)})")
    return Path(pickup)


def load_checkpoint(model, path, Δt: float):
    """restore a WaveGrowth2D from a checkpoint file: its clock, then the library state.  The wind source is handed to the
    library first (a device-resident lattice is part of the configuration the blob is checked against)."""
    blob, time, iteration, _ = read_checkpoint_file(path)
    model._wind_window = None
    model.upload_winds(time, Δt)
    model.backend.checkpoint_load(blob)
    st = getattr(model, "_state", None)
    if st is not None:
        st.after_step()                  # the device field was replaced: no host mirror, no recorded write survives the load
    model.clock.time = time
    model.clock.iteration = iteration
    return time, iteration
