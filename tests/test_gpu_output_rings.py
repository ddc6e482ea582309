"""Every output path on ONE context, sharing its one store stream: a snapshot ring, a diagnostics ring, a probe set, run statistics
and a checkpoint in flight while nine fused-style steps run (picles_time_step).  The rings are small and the pops lag, so each ring
wraps more than twice and each is once found full — refused by its code, nothing lost afterwards.  A twin context runs the same
steps with nothing attached and reads get_state after every step; everything the observers hand out is compared with the twin's
States bit for bit, and so is the observed context's own final State (the observers have no side effect).

Two grids, the smallest that take the two fused kernels: 64 x 8, periodic in x and y (k_step_waverow by default), and 24 x 10,
open on every side (a row that is no multiple of 64: k_step, with boundary particles)."""
import numpy as np
import pytest

import _diag_numpy as D
import _stats_numpy as ST
from helpers import assert_bitwise, assert_same_bits, make_model
from picles_amd import _capi as K
from test_gpu_field_output import _phys, _ready
from test_gpu_waverow import _box

pytestmark = pytest.mark.gpu

N_STEPS = 9
PUSH_AFTER = (1, 2, 3, 5, 7, 9)        # six pushes into two slots: slot 0, 1, 0, 1, 0, 1; the third finds the ring full
COARSEN = (2, 2)
THRESHOLDS = (0.05, 0.2)


def _refused(call, code):
    with pytest.raises(K.PiclesError) as e:
        call()
    assert e.value.code == code, (e.value.code, code, str(e.value))


@pytest.mark.parametrize("nx,ny,periodic", [(64, 8, (True, True)), (24, 10, (False, False))])
def test_all_output_paths_on_one_context_agree_with_an_unobserved_twin(nx, ny, periodic):
    make = lambda: _box(nx, ny, periodic=periodic)
    cfg = make()
    dt = cfg.Δt
    a, twin = _ready(cfg).backend, _ready(make()).backend
    nodes = np.array([(0, 0), (nx - 1, ny - 1), (nx // 2, ny // 2), (1, ny - 2), (nx - 2, 0)])
    a.store_init(2)
    a.diag_init(COARSEN, K.DIAG_FIELDS, 2)
    a.probe_init(nodes, every=1, first=1, capacity=3)
    a.stat_init(K.STAT_ALL, thresholds=THRESHOLDS, every=1)
    g, r_g = _phys(cfg)

    states = {}                          # the twin's State after step s
    snaps, diags, samples = [], [], []   # what the rings handed out, in order
    full = dict(store=0, diag=0, probe=0)
    blob = None

    def pop_store():
        snaps.append(a.store_pop())

    def pop_diag():
        diags.append(a.diag_pop())

    def pop_probe(k):
        v, t, s = a.probe_pop(k)
        assert len(v) == k
        samples.extend(zip(v, t, s))

    for s in range(1, N_STEPS + 1):
        if a.probe_pending == 3 and full["probe"] == 0:
            clock = a.clock
            _refused(lambda: a.time_step(dt, K.STEP_ZERO_FIRST), K.PROBE_E_FULL)      # refused before anything has changed
            assert a.clock == clock and a.probe_pending == 3
            full["probe"] += 1
        if a.probe_pending == 3:
            pop_probe(1)                 # the oldest sample alone: the ring stays two deep
        a.time_step(dt, K.STEP_ZERO_FIRST)
        twin.time_step(dt, K.STEP_ZERO_FIRST)
        states[s] = twin.get_state()
        assert a.clock == twin.clock == s * dt
        if s in PUSH_AFTER:
            if a.store_pending == 2:
                if full["store"] == 0:
                    _refused(a.store_push, -3)
                    assert a.store_pending == 2
                    full["store"] += 1
                pop_store()
            a.store_push()
            if a.diag_pending == 2:
                if full["diag"] == 0:
                    _refused(a.diag_push, -3)
                    assert a.diag_pending == 2
                    full["diag"] += 1
                pop_diag()
            a.diag_push()
        if s == 4:
            a.checkpoint_begin()
        if s == 6:
            blob = a.checkpoint_end()
    assert full == dict(store=1, diag=1, probe=1), full
    while a.store_pending:
        pop_store()
    while a.diag_pending:
        pop_diag()
    pop_probe(a.probe_pending)
    stats = a.stat_get()
    final = a.get_state()

    assert [t for _, t in snaps] == [s * dt for s in PUSH_AFTER]
    for (S, _), s in zip(snaps, PUSH_AFTER):
        assert_bitwise(S, states[s], f"snapshot of step {s}")
    assert [t for _, _, t in diags] == [s * dt for s in PUSH_AFTER]
    for (f, p, _), s in zip(diags, PUSH_AFTER):
        assert_same_bits(f, D.fields_of(states[s], *COARSEN, g, r_g, names=K.DIAG_FIELDS)[0], f"diagnostics of step {s}: fields")
        assert_same_bits(p, D.partials_of(states[s], *COARSEN), f"diagnostics of step {s}: partials")
    assert [int(k) for _, _, k in samples] == list(range(1, N_STEPS + 1))
    assert [float(t) for _, t, _ in samples] == [s * dt for s in range(1, N_STEPS + 1)]
    for v, _, s in samples:
        assert_bitwise(v, states[int(s)][nodes[:, 0], nodes[:, 1], :].T, f"probe sample of step {s}")
    want = ST.accumulate([(states[s], s * dt) for s in range(1, N_STEPS + 1)], K.STAT_ALL, THRESHOLDS)
    ST.assert_equal(stats, want, K.STAT_ALL, "statistics")
    assert_bitwise(final, states[N_STEPS], "the observed context's own final State")

    # the checkpoint taken at step 4, while the rings were in flight, continues to the twin's final State
    m = make_model(make(), "hip")
    m._wind_window = None
    m.upload_winds(4 * dt, dt)
    b = m.backend
    b.checkpoint_load(blob)
    assert b.clock == 4 * dt
    assert_bitwise(b.get_state(), states[4], "State right after the load")
    for _ in range(N_STEPS - 4):
        b.time_step(dt, K.STEP_ZERO_FIRST)
    assert_bitwise(b.get_state(), states[N_STEPS], "the restarted run's final State")
    for x in (a, twin, b):
        x.close()
