"""The tile class map in a slab ring: two ranks over the loopback communicator (tests/native/loopback_ccl.cpp), default
PICLES_WAVEROW mode.  A slab's edge launch has two row ranges and stays on k_step, on the ring's edge stream; its interior launch takes
k_step_waverow on the other stream.  This is the mixed step: the host clears the class-map entries of the edge rows ahead of the k_step
launch (class_map_clear_rows) while the interior launch files its tiles, the reader meets G.Rp > 0, edge rows and ghost rows.

Counts from the geometry: 192 x 32 periodic, 16 rows per rank, halo 2, reach 1.  Rows 0, 1, 14, 15 of a slab are edge rows: they never
take the class path and their tiles keep 0.  Of the interior rows 2 .. 13 those whose window (one row up and down) stays off the edge
rows do: rows 3 .. 12 of the one interior column block, 10 waves per rank and step — from the third step on (the first is the
stand-alone advance, the second reads what that one filed: nothing).  PICLES_PULL_CLASS=0 counts nothing; both give the bits of the
whole-grid context."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
STEPS = 6


@pytest.fixture(scope="module")
def loopback(tmp_path_factory):
    so = tmp_path_factory.mktemp("loopback") / "libloopback_ccl.so"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-I/opt/rocm/include",
                    str(ROOT / "tests" / "native" / "loopback_ccl.cpp"), "-o", str(so)], check=True)
    return so


def _run(loopback, klass):
    env = dict(os.environ, PICLES_CCL_LIB=str(loopback), PICLES_PULL_CLASS="1" if klass else "0")
    env.pop("PICLES_WAVEROW", None)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "native" / "pull_class_ring_driver.py"), str(STEPS)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_two_slabs_edge_rows_never_take_the_class_path(loopback):
    on, off = _run(loopback, True), _run(loopback, False)
    print(on, off)
    for res in (on, off):
        assert res["mismatches"] == 0 and res["nonzero_state"] > 0 and res["max_reach"] == 1, res
        assert res["rows"] == [[0, 16], [16, 32]], res
    assert on["state_crc"] == off["state_crc"]
    want = [[0, 0], [0, 0]] + [[10, 0]] * (STEPS - 2)
    assert on["counts"] == [want, want], on
    assert off["counts"] == [[[0, 0]] * STEPS] * 2, off
