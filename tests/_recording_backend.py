"""One recording backend for run() with every output product attached at once: the diag ring of FakeBackend, the probe ring of
ProbeBackend, the statistics set and the checkpoint calls of StatBackend, and a state-store ring.  Built from those fakes, not
written again: every call they log is logged here in the order run() makes it (tests/test_run_call_sequence.py)."""
import numpy as np

from test_run_stats_host import StatBackend, synthetic_state
from test_station_output_host import ProbeBackend


class RecordingBackend(ProbeBackend):
    """ProbeBackend + StatBackend's statistics set and checkpoint blob + the three-slot ring of run(sim, store=True)"""

    stat_init, stat_free = StatBackend.stat_init, StatBackend.stat_free
    stat_get, stat_set, stat_reset = StatBackend.stat_get, StatBackend.stat_set, StatBackend.stat_reset
    checkpoint_begin, checkpoint_end, checkpoint_load = (StatBackend.checkpoint_begin, StatBackend.checkpoint_end,
                                                         StatBackend.checkpoint_load)

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.stat = None
        self.step = 0                  # model steps since the seed (StatBackend's counter)
        self.state_gen = 0             # LazyState: the mirror is re-read after every step
        self.store_ring, self.store_slots = [], 0

    def _stepped(self, dt, n):
        """the probe step, then the statistics step, of each model step (both fakes advance the clock: by the same addition)"""
        for _ in range(n):
            clock = self.clock
            ProbeBackend._stepped(self, dt, 1)
            self.clock = clock
            StatBackend._stepped(self, dt, 1)

    def get_state(self):
        self.log.append(("get_state", self.step))
        return synthetic_state(self.Nx, self.Ny, self.step)

    # ---- the state-store ring (picles_store_*) ----
    def store_init(self, n_slots=3):
        assert self.store_slots == 0, "second store_init"
        self.store_slots = n_slots
        self.log.append(("store_init", n_slots))

    def store_push(self):
        assert len(self.store_ring) < self.store_slots, "push into a full store ring"
        self.store_ring.append((self.step, self.clock))
        self.log.append(("store_push", self.step))

    def store_pop(self):
        s, t = self.store_ring.pop(0)
        self.log.append(("store_pop", s))
        return synthetic_state(self.Nx, self.Ny, s), t

    @property
    def store_pending(self):
        return len(self.store_ring)


def jsonable(v):
    """a log entry as JSON holds it: tuples as lists, NumPy scalars and arrays as Python numbers and lists"""
    if isinstance(v, (tuple, list)):
        return [jsonable(x) for x in v]
    if isinstance(v, np.ndarray):
        return jsonable(v.tolist())
    if isinstance(v, np.generic):
        return v.item()
    return v
