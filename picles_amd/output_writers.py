"""OutputWriter: what run() (picles_amd/simulations.py) asks of the entries of `sim.output_writers` — Checkpointer, FieldWriter, FluxWriter, MeanFluxWriter,
StationWriter, StatisticsWriter, TrackWriter — and of the one input that is driven the same way, BoundaryForcing (picles_amd/boundary_forcing.py:
visited first, so that the level pair of the next chunk is in place before anything else looks at the iteration; NestForcing of
picles_amd/nesting.py takes its place where the levels come from a parent model, and drives that model's writers through the same
hooks).  run() names none of them: it calls the hooks below, each phase in the order PHASE_ORDER gives
(by kind of writer, not by the dict's order), and a writer overrides the hooks it has work for.  DESIGN.md §16 says why the
orders are what they are."""
from __future__ import annotations

NO_LIMIT = 2**62          # steps_allowed of a writer that ends no chunk

# the visiting order of each phase, by `kind`; a kind a phase does not list has no work in it (and is visited last)
PHASE_ORDER = {
    "begin_run": ("boundary_forcing", "fields", "fluxes", "flux_means", "stations", "statistics", "tracks"),
    "after_chunk": ("stations", "checkpointer", "tracks"),
    "at_iteration": ("boundary_forcing", "statistics", "checkpointer", "fields", "fluxes", "flux_means", "tracks"),
    "finish": ("checkpointer", "fields", "fluxes", "flux_means", "stations", "statistics", "tracks"),
}


class OutputWriter:
    kind = None             # the name PHASE_ORDER knows the class by
    needs = None            # a backend method the writer cannot do without ...
    refusal = None          # ... and what run() says of a backend that lacks it
    sized_for_run = False   # begin_run sizes a file for the run: a finite stop_time is needed

    def check_run(self, sim, writers, store=False, cash_store=False, pickup=False):
        """run(sim, ...) is about to start with these arguments and these writers: raise for a combination this writer cannot
        serve — nothing has been loaded or seeded yet"""

    def pickup_companions(self, checkpoint_file):
        """the files this writer cannot continue without next to `checkpoint_file`: run(sim, pickup=True) takes the latest
        checkpoint for which every writer's companions are complete"""
        return ()

    def check_pickup(self, checkpoint_file):
        """run(sim, pickup=...) has chosen `checkpoint_file` and every check_run has passed: raise a CheckpointError for
        companions that are missing or were written by another configuration — nothing has been loaded yet"""

    def load_pickup(self, checkpoint_file):
        """run(sim, pickup=...) has loaded `checkpoint_file`: take what this writer stored next to it"""

    def begin_run(self, model, n_steps: int):
        """`n_steps` steps from the model's iteration are about to run"""

    def steps_allowed(self, backend, iteration: int) -> int:
        """how many steps the next chunk of picles_run_steps may take from `iteration`"""
        return NO_LIMIT

    def after_chunk(self, backend):
        """the chunked path only: a chunk has been enqueued (the clock does not show it yet)"""

    def before_step(self, backend):
        """the per-step loop only: a time_step is about to be taken"""

    def at_iteration(self, model, writers):
        """the clock has reached an iteration, on either path; `writers` are all the writers run() drives"""

    def checkpoint_begun(self, backend, checkpoint_file):
        """the Checkpointer has taken the snapshot that will become `checkpoint_file`"""

    def finish(self, backend, iteration=None):
        """the run is over"""


def writers_of(sim):
    """the writers run() drives: the first of each kind in sim.output_writers (what is no OutputWriter is left alone)"""
    found = {}
    for w in getattr(sim, "output_writers", {}).values():
        if isinstance(w, OutputWriter):
            found.setdefault(w.kind, w)
    return list(found.values())


def find_writer(sim, kind):
    """the writer of that kind (a class attribute `kind`, or the class itself), or None"""
    kind = getattr(kind, "kind", kind)
    return next((w for w in writers_of(sim) if w.kind == kind), None)


def in_phase(writers, phase):
    order = PHASE_ORDER[phase]
    return sorted(writers, key=lambda w: order.index(w.kind) if w.kind in order else len(order))
