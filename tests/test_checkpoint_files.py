"""The file layer of exact restart (picles_amd/checkpointing.py), no GPU: atomic writes, which file pickup chooses, the clock
round trip, refusals of truncated or foreign files before they reach the library, pickup with nothing to pick up."""
import os
import struct

import numpy as np
import pytest

from picles_amd import _capi as K
from picles_amd import checkpointing as CK
from picles_amd.simulations import Simulation, run


def _blob(n=64, fill=7):
    b = np.full(K.CKPT_HEADER_BYTES + n, fill, dtype=np.uint8)
    b[:8] = np.frombuffer(struct.pack("<Q", K.CKPT_MAGIC), dtype=np.uint8)
    return b


def test_clock_and_iteration_round_trip(tmp_path):
    p = CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "ck", 12), _blob(), 7200.000000000001, 12)
    blob, t, it, rank = CK.read_checkpoint_file(p)
    assert p.name == "ck_iteration12.picles"
    assert (t, it, rank) == (7200.000000000001, 12, None)
    assert np.array_equal(blob, _blob())
    p2 = CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "ck", 3, rank=1), _blob(), 1.5, 3, rank=1)
    assert p2.name == "ck_iteration3_rank1.picles" and CK.read_checkpoint_file(p2)[3] == 1


def test_crash_before_the_rename_leaves_no_pickable_file(tmp_path, monkeypatch):
    CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "ck", 4), _blob(), 1.0, 4)

    def crash(*a, **k):
        raise KeyboardInterrupt("killed")
    monkeypatch.setattr(os, "replace", crash)
    with pytest.raises(KeyboardInterrupt):
        CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "ck", 8), _blob(), 2.0, 8)
    monkeypatch.undo()
    assert CK.latest_checkpoint(tmp_path, "ck").name == "ck_iteration4.picles"
    # a temporary file left by a job killed mid-write (no cleanup at all) is not chosen either
    (tmp_path / ".ck_iteration12.picles.tmp-999").write_bytes(b"PICLESCF")
    assert CK.latest_checkpoint(tmp_path, "ck").name == "ck_iteration4.picles"


def test_pickup_chooses_the_highest_iteration_of_its_prefix(tmp_path):
    for i in (4, 12, 8):
        CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "ck", i), _blob(), float(i), i)
    CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "other", 40), _blob(), 40.0, 40)
    CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "ck", 16, rank=0), _blob(), 16.0, 16, rank=0)
    (tmp_path / "ck_iteration99.picles.bak").write_bytes(b"x")
    assert sorted(CK.list_checkpoints(tmp_path, "ck")) == [4, 8, 12]
    assert CK.latest_checkpoint(tmp_path, "ck").name == "ck_iteration12.picles"
    sim = Simulation(model=None, Δt=1.0)
    sim.output_writers["checkpointer"] = CK.Checkpointer(schedule=4, dir=tmp_path, prefix="ck")
    assert CK.resolve_pickup(sim, True).name == "ck_iteration12.picles"
    # slab ranks: the highest iteration every rank has a file for
    for r, its in ((0, (4, 8)), (1, (4,))):
        for i in its:
            CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "slab", i, rank=r), _blob(), float(i), i, rank=r)
    assert CK.latest_checkpoint(tmp_path, "slab", rank=0, world=2).name == "slab_iteration4_rank0.picles"


def test_truncated_or_foreign_files_are_refused(tmp_path):
    p = CK.write_checkpoint_file(CK.checkpoint_path(tmp_path, "ck", 4), _blob(), 1.0, 4)
    raw = p.read_bytes()
    bad = tmp_path / "cut.picles"
    for data in (raw[:-1], raw[:20], b"", b"NOTACKPT" + raw[8:], raw + b"\0"):
        bad.write_bytes(data)
        with pytest.raises(K.CheckpointError):
            CK.read_checkpoint_file(bad)
    other = _blob(); other[:8] = 0          # a file of the right shape around something that is not a library blob
    p2 = CK.write_checkpoint_file(tmp_path / "x.picles", other, 1.0, 4)
    with pytest.raises(K.CheckpointError, match="blob"):
        CK.read_checkpoint_file(p2)


def test_pickup_with_an_empty_directory_raises(tmp_path):
    sim = Simulation(model=None, Δt=1.0, stop_time=10.0)
    sim.output_writers["checkpointer"] = CK.Checkpointer(schedule=4, dir=tmp_path / "none")
    with pytest.raises(K.CheckpointError, match="no checkpoint"):
        run(sim, pickup=True)
    bare = Simulation(model=None, Δt=1.0, stop_time=10.0)
    with pytest.raises(K.CheckpointError, match="Checkpointer"):
        run(bare, pickup=True)


def test_schedule():
    s = CK.IterationInterval(4)
    assert [i for i in range(13) if s(i)] == [4, 8, 12]
    assert s.next_after(0) == 4 and s.next_after(4) == 8 and s.next_after(5) == 8
