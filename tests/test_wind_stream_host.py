"""Streamed winds, the host side: the time rule `coupling.stream_coord` against the library's picles_wind_stream_coord
and, clear of the snapping slack, against the lattice sampler's own coordinate (wind_emulator._lattice_coord on a longer lattice), to
the bit; StreamedWinds' argument checks and the refusals of backends that carry no wind stream.  No device work."""
import ctypes as C

import numpy as np
import pytest

from picles_amd import configs
from picles_amd import _capi as K
from picles_amd.coupling import StreamedWinds, stream_coord, REFUSAL
from picles_amd.wind_emulator import _lattice_coord
from helpers import make_model


def _c_coord(lib, t0, dt, t):
    k, f = C.c_int64(-7), C.c_double(-7.0)
    rc = lib.picles_wind_stream_coord(t0, dt, t, C.byref(k), C.byref(f))
    return rc, k.value, f.value


def _cases():
    rng = np.random.default_rng(23)
    cases = []
    for _ in range(300):
        t0, dt = float(rng.uniform(-1e4, 1e4)), float(rng.uniform(50, 5e3))
        cases.append((t0, dt, t0 + float(rng.uniform(0, 1e5))))
    cases += [(0.0, 512.0, 512.0 * k) for k in range(20)] + [(-300.0, 700.0, -300.0 + 700.0 * k) for k in range(20)]      # aligned
    cases += [(0.0, 900.0, 600.0 * k) for k in range(13)]                                                                # 600 s steps, 900 s knots
    cases += [(0.0, 0.1 * 9000, 0.1 * 6000 * k) for k in range(13)]
    for t0, dt in ((0.0, 900.0), (125.0, 512.0), (-40.0, 3600.0)):        # 1e-10 and 1e-8 of an interval either side of a knot
        for k in (1, 2, 7, 40):
            for off in (1e-10, -1e-10, 1e-8, -1e-8):
                cases.append((t0, dt, t0 + (k + off) * dt))
    return cases


def test_stream_coord_python_and_c_agree():
    lib = K.load()
    snapped = unsnapped = 0
    for t0, dt, t in _cases():
        rc, k, f = _c_coord(lib, t0, dt, t)
        assert rc == 0, (t0, dt, t)
        assert (k, f) == stream_coord(t0, dt, t), (t0, dt, t)
        assert 0.0 <= f < 1.0 and k >= 0
        c = (t - t0) * (1.0 / dt)
        if c != np.rint(c) and abs(c - np.rint(c)) <= 1e-9:
            assert f == 0.0 and k == int(np.rint(c))
            snapped += 1
        elif f != 0.0:
            unsnapped += 1
    assert snapped >= 12 and unsnapped >= 300
    # either side of a knot: 1e-10 of an interval is the knot, 1e-8 is not
    assert stream_coord(0.0, 900.0, 900.0 * (2 + 1e-10)) == (2, 0.0) and stream_coord(0.0, 900.0, 900.0 * (2 - 1e-10)) == (2, 0.0)
    k, f = stream_coord(0.0, 900.0, 900.0 * (2 + 1e-8))
    assert k == 2 and 0.0 < f < 2e-8
    k, f = stream_coord(0.0, 900.0, 900.0 * (2 - 1e-8))
    assert k == 1 and 1.0 - 2e-8 < f < 1.0
    # 600-second steps against 900-second levels: every step end is a level or clear of one
    assert [stream_coord(0.0, 900.0, 600.0 * s)[0] for s in range(7)] == [0, 0, 1, 2, 2, 3, 4]
    assert stream_coord(0.0, 900.0, 1800.0) == (2, 0.0)
    # refused: a time before the first level, a non-positive interval
    assert _c_coord(lib, 100.0, 50.0, 0.0)[0] == -2 and _c_coord(lib, 0.0, 0.0, 10.0)[0] == -2
    assert lib.picles_wind_stream_coord(0.0, 10.0, 25.0, None, None) == 0
    with pytest.raises(ValueError, match="before the stream's first level"):
        stream_coord(100.0, 50.0, 0.0)
    with pytest.raises(ValueError, match="positive"):
        stream_coord(0.0, -1.0, 0.0)


def test_stream_coord_is_the_lattice_samplers_coordinate_clear_of_the_knots():
    """for a time not within the slack of a level, (k, f) is what k_wind_sample's arithmetic (wind_emulator._lattice_coord) gives on a
    lattice that reaches beyond that time: the streamed sample then blends the same two levels with the same weight"""
    n = 0
    for t0, dt, t in _cases():
        c = (t - t0) * (1.0 / dt)
        if abs(c - np.rint(c)) <= 1e-9:
            continue
        k, f = stream_coord(t0, dt, t)
        it, ft = _lattice_coord(np.float64(c), k + 3)
        assert (int(it), float(ft)) == (k, f), (t0, dt, t)
        n += 1
    assert n >= 300
    # ON a level the two differ in form only: the lattice reads (k, 0) as well while the level is not its last
    for k in range(5):
        it, ft = _lattice_coord(np.float64(k), 7)
        assert (int(it), float(ft)) == stream_coord(0.0, 512.0, 512.0 * k) == (k, 0.0)
    it, ft = _lattice_coord(np.float64(6.0), 7)      # its last level is f = 1 of the interval before: not the stream's form
    assert (int(it), float(ft)) == (5, 1.0)


def test_streamed_winds_argument_checks():
    x, y = np.arange(13) * 5e3, np.arange(11) * 4.5e3
    w = StreamedWinds(x, y, 0.0, 900.0)
    assert (w.slots, w.time_mode, w.source) == (3, "linear", None) and w.coord(1350.0) == (1, 0.5)
    assert w.levels_of(600.0, 1200.0) == (0, 2) and w.levels_of(1200.0, 1800.0) == (1, 2) and w.levels_of(0.0, 0.0) == (0, 0)
    with pytest.raises(ValueError, match="regular"):
        StreamedWinds([0.0, 1.0, 3.0], y, 0.0, 900.0)
    with pytest.raises(ValueError, match="regular"):
        StreamedWinds(x, [4.0], 0.0, 900.0)
    with pytest.raises(ValueError, match="positive"):
        StreamedWinds(x, y, 0.0, 0.0)
    with pytest.raises(ValueError, match="slots"):
        StreamedWinds(x, y, 0.0, 900.0, slots=1)
    with pytest.raises(ValueError, match="time_mode"):
        StreamedWinds(x, y, 0.0, 900.0, time_mode="cubic")
    with pytest.raises(TypeError, match="callable"):
        StreamedWinds(x, y, 0.0, 900.0, source=3)
    with pytest.raises(K.PiclesError, match="not attached"):
        w.push(0, np.zeros((11, 13)), np.zeros((11, 13)))


def _streamed_cfg():
    cfg = configs.example_00_minimal(n=33, L=64e3)
    cfg.model["winds"] = StreamedWinds(np.arange(13) * 5e3, np.arange(11) * 4.5e3, 0.0, 900.0)
    cfg.model["winds_static"] = False
    return cfg


def test_backends_without_a_wind_stream_refuse_streamed_winds():
    with pytest.raises(NotImplementedError, match="StreamedWinds are carried by the HIP library"):
        make_model(_streamed_cfg(), ("pmath", 1))
    from picles_amd.parallel import SlabModel
    with pytest.raises(NotImplementedError, match="SlabModel: StreamedWinds"):
        SlabModel(_streamed_cfg().model, 0, 1)
    assert "slabs" in REFUSAL


def test_nest_forcing_refuses_streamed_winds():
    from types import SimpleNamespace
    from picles_amd.nesting import NestForcing
    from picles_amd.boundary_forcing import BoundaryForcing
    child = SimpleNamespace(model=SimpleNamespace(winds=_streamed_cfg().model["winds"]))
    parent = SimpleNamespace(model=SimpleNamespace(winds=None), output_writers={})
    nf = NestForcing.__new__(NestForcing)
    nf.parent = parent
    saved = BoundaryForcing.check_run
    BoundaryForcing.check_run = lambda self, *a, **k: None
    try:
        with pytest.raises(NotImplementedError, match="streamed nests are not carried"):
            nf.check_run(child, [])
        child.model.winds, parent.model.winds = None, _streamed_cfg().model["winds"]
        with pytest.raises(NotImplementedError, match="streamed nests are not carried"):
            nf.check_run(child, [])
    finally:
        BoundaryForcing.check_run = saved
