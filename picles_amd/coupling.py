"""Coupling: winds that arrive one time level at a time, from device memory, while the model runs.

PiCLES as the wave component of a coupled system: an atmosphere hands over the 10 m winds of one coupling interval, knows nothing of
the next, and wants the sea state back.  `StreamedWinds` is the wind source for that — a lattice with regular (x, y) axes like
`wind_emulator.GriddedWinds`, whose time levels t_k = t0 + k dt are pushed into a ring on the device (`picles_wind_stream_*`) — and
`HipModel.diag_export` the way back: Hs / Tp / cg planes written into the caller's device tensors.  Beside it, `FluxExport` hands back
what the partner models consume rather than a description of the sea (`picles_flux_*`): the momentum and energy the
waves take out of the wind (the wave-supported stress), what the breaking waves hand down to the ocean, and the surface Stokes drift.
All directions are ordered against torch's current stream with events; none copies to the host.

    winds = StreamedWinds(x, y, t0=0.0, dt=3600.0, slots=3)
    model = WaveGrowth2D(winds=winds, winds_static=False, ...)
    initialize... ; winds.push(0, u0, v0); winds.push(1, u1, v1)      # NumPy arrays or torch CUDA tensors, (ny, nx) or flat
    model.backend.run_steps(dt, n)                                   # refused with a text if a level the steps read is missing
    fluxes = FluxExport(model, coarsen=(4, 4), rho_water=1025.0)     # once
    planes = fluxes()                                                # dict of [nyc, nxc] float32 CUDA tensors: tq_in_x, phi_dis, us_x, ...

With `source=callable(k) -> (u, v)` run(sim) pulls the levels itself, a chunk at a time, as far as the ring admits.
"""
from __future__ import annotations

import math

import numpy as np

from . import _capi as K

SNAP = 1e-9          # a time closer to a level than this many intervals IS that level (the slack of picles_lattice_knots)

REFUSAL = ("StreamedWinds are carried by the HIP library's wind stream on a whole-grid model (picles_wind_stream_*): this backend has none "
           "— CPU backends and slabs take a GriddedWinds lattice or wind closures")


def stream_coord(t0, dt, t):
    """the time rule of a wind stream, (k, f) with t = t0 + (k + f) dt: the host mirror of picles_wind_stream_coord (the tests hold
    the two against each other).  c = (t - t0) * (1 / dt) as the lattice sampler forms it, snapped to the whole number it is within
    1e-9 of; k = floor(c), f = c - k"""
    t0, dt, t = float(t0), float(dt), float(t)
    if not dt > 0.0:
        raise ValueError("stream_coord: dt must be positive")
    c = (t - t0) * (1.0 / dt)
    r = float(np.rint(c))
    if abs(c - r) <= SNAP:
        c = r
    if not (0.0 <= c < 9.0e15):
        raise ValueError(f"stream_coord: t = {t} lies before the stream's first level t0 = {t0} (a stream has no periodic continuation in t)")
    k = math.floor(c)
    return int(k), c - float(k)


class StreamedWinds:
    """StreamedWinds(x, y, t0, dt, slots=3, time_mode="linear", source=None), handed to WaveGrowth2D(winds=...).
    x, y: the lattice's regular space axes (>= 2 knots each; periodic continuation outside, as GriddedWinds); level k holds the winds
    at t0 + k dt; `slots` levels are held at a time (a step with nk levels strictly inside needs nk + 2).  time_mode as GriddedWinds.
    source: callable(k) -> (u, v), asked by run(sim) for the levels a chunk needs and not before the ring admits them."""

    def __init__(self, x, y, t0, dt, slots=3, time_mode="linear", source=None):
        if time_mode not in ("linear", "smooth3"):
            raise ValueError("time_mode must be 'linear' or 'smooth3'")
        self.x, self.y = (np.asarray(a, dtype=np.float64) for a in (x, y))
        for a, name in ((self.x, "x"), (self.y, "y")):
            if a.ndim != 1 or a.size < 2 or not np.allclose(np.diff(a), a[1] - a[0], rtol=1e-12, atol=0) or not a[1] > a[0]:
                raise ValueError(f"wind stream axis {name} must be regular and increasing with >= 2 knots")
        self.t0, self.dt = float(t0), float(dt)
        if not self.dt > 0.0:
            raise ValueError("the coupling interval dt must be positive (irregular intervals are not carried)")
        if int(slots) != slots or int(slots) < 2:
            raise ValueError("slots must be an integer >= 2 (two levels bracket a time)")
        if source is not None and not callable(source):
            raise TypeError("source must be callable(k) -> (u, v)")
        self.slots, self.time_mode, self.source = int(slots), time_mode, source
        self.dx, self.dy = float(self.x[1] - self.x[0]), float(self.y[1] - self.y[0])
        self._backend = None

    # ---- the time axis ----
    def coord(self, t):
        return stream_coord(self.t0, self.dt, t)

    def levels_of(self, t_a, t_b):
        """(first, last) level a window over [t_a, t_b] reads"""
        k0, _ = self.coord(t_a)
        k1, f1 = self.coord(t_b)
        return k0, k1 + (1 if f1 != 0.0 else 0)

    # ---- the device side ----
    def attach(self, model):
        """once per backend: the ring (picles_wind_stream_init); replaces whatever winds the backend had"""
        b = model.backend
        if not hasattr(b, "wind_stream_init"):
            raise NotImplementedError(REFUSAL)
        if self._backend is not b:
            g = model.grid
            b.wind_stream_init(self.x.size, self.y.size, self.x[0], self.dx, self.y[0], self.dy, self.t0, self.dt,
                               float(g.data.x[0, 0]), float(g.data.y[0, 0]), n_slots=self.slots, time_mode=self.time_mode)
            self._backend = b
        return b

    def _bound(self):
        if self._backend is None:
            raise K.PiclesError("StreamedWinds: not attached to a model yet (WaveGrowth2D(winds=...), then initialize_simulation or upload_winds)")
        return self._backend

    def push(self, k, u, v):
        """level k: NumPy arrays or torch CUDA tensors of (ny, nx) values, or flat with x fastest (HipModel.wind_stream_push)"""
        self._bound().wind_stream_push(k, u, v)

    def info(self):
        return self._bound().wind_stream_info()

    def reset(self):
        self._bound().wind_stream_reset()

    def ensure(self, t_a, t_b):
        """with a source: push what the window over [t_a, t_b] reads and the ring does not hold.  A window that starts before the
        oldest level held, or beyond the newest, starts the ring afresh (a restored clock).  Without a source nothing happens: the
        library names the missing level when a step needs it"""
        if self.source is None:
            return
        b = self._bound()
        k0, k1 = self.levels_of(t_a, t_b)
        _, oldest, newest, _ = b.wind_stream_info()
        if newest >= 0 and (k0 < oldest or k0 > newest + 1):
            b.wind_stream_reset()
            newest = -1
        nxt = k0 if newest < 0 else newest + 1
        for k in range(nxt, k1 + 1):
            b.wind_stream_push(k, *self.source(k))

    def steps_allowed(self, dt, k_max):
        """how many of the next k_max steps of length dt the held levels cover, from the backend's clock; a source is first asked for
        the levels those steps read, as far as the ring admits them (the slot of the clock's own level is kept).  At least 1: a step
        whose level is missing is refused by the library, with its text"""
        b = self._bound()
        t = float(b.clock)
        slots, _, newest, _ = b.wind_stream_info()
        if self.source is not None:
            self.ensure(t, t + dt)
            newest = b.wind_stream_info()[2]
            top = min(self.coord(t)[0] + slots - 1, self.levels_of(t, t + k_max * dt)[1])
            for k in range(newest + 1, top + 1):
                b.wind_stream_push(k, *self.source(k))
            newest = max(newest, top)
        n = 0
        while n < k_max:
            if self.levels_of(t, t + dt)[1] > newest:
                break
            n += 1
            t += dt
        return max(n, 1)


class FluxExport:
    """FluxExport(model, coarsen=(4, 4), fields=_capi.FLUX_FIELDS, rho_water=1025.0): the coupling fluxes of the model's current
    step boundary in device tensors of its own (`picles_flux_export`).  Calling it runs the kernel behind the model's steps and orders
    torch's current stream behind the kernel; it returns {plane name: float32 CUDA tensor [nyc, nxc]} — views of one block that the
    next call overwrites — the phi planes in W m-2 (rho_water * g), the tq planes in N m-2 (rho_water), the Stokes drift in m s-1, as
    area means over the coarse cells (land and calm nodes count as zero).  `partials` holds the tile partials ([n_partials, 11]
    float64, on the device; driver.combine_flux_partials of its host copy gives the area totals).  The wind is the level the wind
    window holds at the clock — after a step, the step's end level; a lattice or streamed model samples it where its planes hold
    none (include/picles_hip.h, "coupling fluxes")."""

    def __init__(self, model, coarsen=(4, 4), fields=K.FLUX_FIELDS, rho_water=1025.0, device=None):
        import torch
        b = self.backend = model.backend
        if not hasattr(b, "flux_export"):
            raise NotImplementedError("FluxExport needs the HIP library's flux set (picles_flux_*): this backend has none")
        if not (np.isfinite(rho_water) and rho_water > 0.0):
            raise ValueError("FluxExport: rho_water must be finite and positive")
        b.flux_init(coarsen, fields, scale_phi=float(rho_water) * 9.81, scale_tau=float(rho_water), n_slots=1)
        self.fields = b.flux_fields
        nxc, nyc, nf, npart, _ = b.flux_shape()
        dev = torch.device("cuda", getattr(b, "device", 0)) if device is None else device
        self.planes = torch.zeros((nf, nyc, nxc), dtype=torch.float32, device=dev)
        self.partials = torch.zeros((npart, K.FLUX_NPARTIAL), dtype=torch.float64, device=dev)

    def __call__(self):
        self.backend.flux_export(self.planes, self.partials)
        return {f: self.planes[k] for k, f in enumerate(self.fields)}


class FluxMeanExport(FluxExport):
    """FluxMeanExport(model, coarsen=(4, 4), fields=_capi.FLUX_FIELDS, rho_water=1025.0, every=1): the coupling fluxes as the MEAN over
    the model steps since the last call, which is what a coupler exchanges (`picles_flux_mean_*`; include/picles_hip.h, "flux means").
    The device accumulates the cell sums behind every `every`-th model step — the steps stay fused — and calling the object finalises
    them into the device tensors of FluxExport (`picles_flux_mean_export` with reset = 1: the next interval starts empty) and returns
    {plane name: float32 CUDA tensor [nyc, nxc]}.  `n_samples`, `t_first`, `t_last` describe the samples held now (after a call: the
    interval that call exported is in `exported`).  `partials` holds the unscaled, undivided tile partials of the interval: the
    host divides their combination by the number of samples.  A call with no sample held is refused by the library."""

    def __init__(self, model, coarsen=(4, 4), fields=K.FLUX_FIELDS, rho_water=1025.0, every=1, device=None):
        super().__init__(model, coarsen, fields, rho_water, device)
        if not hasattr(self.backend, "flux_mean_export"):
            raise NotImplementedError("FluxMeanExport needs the HIP library's mean set (picles_flux_mean_*): this backend has none")
        self.backend.flux_mean_init(every=every, first=every)
        self.exported = dict(n_samples=0, t_first=0.0, t_last=0.0)

    def _scalars(self):
        return self.backend.flux_mean_scalars()           # host-side values: no device work

    n_samples = property(lambda self: self._scalars()[0])
    t_first = property(lambda self: self._scalars()[1])
    t_last = property(lambda self: self._scalars()[2])

    def __call__(self):
        n, t0, t1 = self._scalars()
        self.backend.flux_mean_export(self.planes, self.partials, reset=True)
        self.exported = dict(n_samples=n, t_first=t0, t_last=t1)
        return {f: self.planes[k] for k, f in enumerate(self.fields)}
