"""HipModel: thin object wrapper over one `picles_ctx*` (one GPU, one y-slab).

All compute happens in libpicles_hip.so (hand-written HIP kernels).  This module only moves
host arrays across the C ABI.  If the library is missing or no HIP device exists, construction
raises — there is no CPU path in the product.
"""
from __future__ import annotations

import atexit
import ctypes as C
import weakref

import numpy as np

from . import _capi as K


def _check(lib, h, rc, what):
    if rc != 0:
        msg = lib.picles_last_error(h)
        e = K.PiclesError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
        e.code = rc          # (e.g. K.PROBE_E_FULL: the caller pops and repeats the call)
        raise e


def _col(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, order="F"))
    if a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


def _int32_planes(a, who, what="index", pairs=False):
    """an integer array, nodes or stencil rows along axis 0 -> its columns as contiguous int32 planes, the layout of the C ABI's
    node lists and stencils; pairs: the array must be (n, 2), a list of (i, j)"""
    a = np.asarray(a, dtype=np.int64)
    if pairs and (a.ndim != 2 or a.shape[1] != 2):
        raise ValueError(f"{who}: nodes must be an (n, 2) array of (i, j)")
    if a.size and np.abs(a).max() > 2**31 - 1:
        raise ValueError(f"{who}: {what} out of the int32 range")
    return np.ascontiguousarray(a.T.astype(np.int32))


def _p32(planes):
    return planes.ctypes.data_as(K.c_int32_p)


def diag_field_mask(fields) -> int:
    """field names (or a ready bit mask) -> PICLES_DIAG_* bit mask"""
    if isinstance(fields, (int, np.integer)):
        return int(fields)
    if isinstance(fields, str):
        fields = (fields,)
    unknown = [f for f in fields if f not in K.DIAG_BITS]
    if unknown:
        raise ValueError(f"unknown diagnostic fields {unknown}: choose from {K.DIAG_FIELDS}")
    mask = 0
    for f in fields:
        mask |= K.DIAG_BITS[f]
    return mask


def combine_partials(list_of_partials, Nx, Ny) -> dict:
    """the eight global scalars from the tile partials of picles_diag_pop — one [n_partials, 7] array, or a list of them in rank
    order for a slab run: combined sequentially in ascending (J, tile) order, sums from +0.0 and maxima (fmax) from -inf, so the
    result does not depend on the decomposition.  mean_of_state = sum_e / (Nx Ny) (TimeSteppers.jl:15-19)."""
    if isinstance(list_of_partials, np.ndarray) and list_of_partials.ndim == 2:
        list_of_partials = [list_of_partials]
    acc = [0.0, 0.0, 0.0, 0.0, -np.inf, -np.inf, -np.inf]
    for part in list_of_partials:
        for row in np.asarray(part, dtype=np.float64).reshape(-1, 7).tolist():
            for k in range(4):
                acc[k] = acc[k] + row[k]
            for k in range(4, 7):
                b = row[k]
                if b == b and (acc[k] != acc[k] or b > acc[k]):
                    acc[k] = b
    out = dict(zip(K.DIAG_PARTIAL, acc))
    out["mean_of_state"] = out["sum_e"] / (float(Nx) * float(Ny))
    return out


SCALAR_NAMES = K.DIAG_PARTIAL + ("mean_of_state",)


def flux_field_mask(fields) -> int:
    """plane names (or a ready bit mask) -> PICLES_FLUX_* bit mask"""
    if isinstance(fields, (int, np.integer)):
        return int(fields)
    if isinstance(fields, str):
        fields = (fields,)
    unknown = [f for f in fields if f not in K.FLUX_BITS]
    if unknown:
        raise ValueError(f"unknown flux planes {unknown}: choose from {K.FLUX_FIELDS}")
    mask = 0
    for f in fields:
        mask |= K.FLUX_BITS[f]
    return mask


def combine_flux_partials(list_of_partials) -> dict:
    """the eleven area totals from the tile partials of picles_flux_pop — one [n_partials, 11] array, or a list of them in rank
    order for a slab run — combined sequentially in ascending (J, tile) order from +0.0: the same bits whatever the decomposition.
    The nine sums are UNSCALED node sums (multiply by the cell area and the set's scale for an integrated flux)."""
    if isinstance(list_of_partials, np.ndarray) and list_of_partials.ndim == 2:
        list_of_partials = [list_of_partials]
    acc = [0.0] * K.FLUX_NPARTIAL
    for part in list_of_partials:
        for row in np.asarray(part, dtype=np.float64).reshape(-1, K.FLUX_NPARTIAL).tolist():
            for k in range(K.FLUX_NPARTIAL):
                acc[k] = acc[k] + row[k]
    return dict(zip(K.FLUX_PARTIAL, acc))


def flux_mean_tile_partials(acc) -> np.ndarray:
    """the tile partials of a mean (include/picles_hip.h "flux means") from accumulator planes [11, Nxc, nyc] on the host: each plane
    through the halving tree inside each group of 64 coarse columns, then the four groups of a tile of 256 in ascending order;
    [nyc * tiles_per_row, 11], index J tiles_per_row + T — the bits k_flux_mean_final writes"""
    acc = np.asarray(acc, dtype=np.float64)
    _, nxc, nyc = acc.shape
    tpr = -(-nxc // 256)
    v = np.zeros((K.FLUX_NPARTIAL, tpr * 256, nyc))
    v[:, :nxc] = acc
    v = v.reshape(K.FLUX_NPARTIAL, tpr, 4, 64, nyc)
    s = 32
    while s >= 1:
        v = v[:, :, :, :s] + v[:, :, :, s:2 * s]
        s //= 2
    w = v[:, :, :, 0]
    t = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]              # [11, tpr, nyc]
    return np.ascontiguousarray(t.transpose(2, 1, 0).reshape(nyc * tpr, K.FLUX_NPARTIAL))


def flux_mean_concat(parts) -> dict:
    """what flux_mean_get returned on every rank, in rank order, as one whole-grid result: the planes row block after row block, the
    scalars of rank 0 (the ranks step together), and "totals": the eleven sums over all cells — every rank's tile partials combined
    in rank order as combine_flux_partials does — divided by n_samples (None without a sample)"""
    n = int(parts[0]["n_samples"])
    tot = combine_flux_partials([flux_mean_tile_partials(p["acc"]) for p in parts])
    return dict(acc=np.concatenate([np.asarray(p["acc"]) for p in parts], axis=2), n_samples=n, t_first=parts[0]["t_first"],
                t_last=parts[0]["t_last"], totals={k: v / n for k, v in tot.items()} if n else None)


# ---- run statistics: the plane block of picles_stat_get / picles_stat_set (include/picles_hip.h "run statistics") ----
STAT_GROUPS = {"peak": K.STAT_PEAK, "mean": K.STAT_MEAN, "exceed": K.STAT_EXCEED}
STAT_PEAK_PLANES = ("e_peak", "mx_peak", "my_peak", "t_peak")
STAT_MEAN_PLANES = ("sum_e", "sum_mx", "sum_my", "sum_hs")


def stat_mask(groups, allow_empty=False) -> int:
    """group names (or a ready bit mask) -> PICLES_STAT_* bit mask; refuses what the library would refuse"""
    if isinstance(groups, (int, np.integer)):
        mask = int(groups)
    else:
        if isinstance(groups, str):
            groups = (groups,)
        unknown = [g for g in groups if g not in STAT_GROUPS]
        if unknown:
            raise ValueError(f"unknown statistics groups {unknown}: choose from {tuple(STAT_GROUPS)}")
        mask = 0
        for g in groups:
            mask |= STAT_GROUPS[g]
    if mask < 0 or (mask & ~K.STAT_ALL) or (mask == 0 and not allow_empty):
        raise ValueError(f"empty or unknown statistics group mask {mask}")
    return mask


def stat_layout(mask, n_thresholds):
    """[(name, dtype, planes)] of the plane block for `mask`, in its order: the fp64 planes first, then the uint32 ones"""
    lay = []
    if mask & K.STAT_PEAK:
        lay += [(n, np.float64, 1) for n in STAT_PEAK_PLANES]
    if mask & K.STAT_MEAN:
        lay += [(n, np.float64, 1) for n in STAT_MEAN_PLANES]
    lay.append(("n_wet", np.uint32, 1))
    if mask & K.STAT_EXCEED:
        lay.append(("n_exc", np.uint32, int(n_thresholds)))
    return lay


def stat_mask_of(acc) -> int:
    return ((K.STAT_PEAK if "e_peak" in acc else 0) | (K.STAT_MEAN if "sum_e" in acc else 0) | (K.STAT_EXCEED if "n_exc" in acc else 0))


def stat_unpack(buf, lay, Nx, ny):
    """plane block (bytes) -> {name: (Nx, ny) plane, "n_exc": (Nx, ny, n_thresholds)}, column-major like State"""
    out, at, N = {}, 0, Nx * ny
    for name, dt, k in lay:
        nb = np.dtype(dt).itemsize * N * k
        a = np.frombuffer(buf, dtype=dt, count=N * k, offset=at).copy()
        out[name] = a.reshape((Nx, ny) + ((k,) if name == "n_exc" else ()), order="F")
        at += nb
    return out


def stat_pack(acc, lay, Nx, ny):
    parts = []
    for name, dt, k in lay:
        a = np.asarray(acc[name], dtype=dt)
        if a.shape != (Nx, ny) + ((k,) if name == "n_exc" else ()):
            raise ValueError(f"statistics plane {name}: shape {a.shape}, expected {(Nx, ny) + ((k,) if name == 'n_exc' else ())}")
        parts.append(np.ascontiguousarray(a.reshape(-1, order="F")).view(np.uint8))
    return np.ascontiguousarray(np.concatenate(parts))


def stat_concat(list_of_acc):
    """the accumulators of the whole grid from those of its slabs, in rank order: per-node values do not depend on the
    decomposition, so the gather is a concatenation of row blocks; the scalars are every slab's (taken from the first)"""
    first = list_of_acc[0]
    out = {}
    for k, v in first.items():
        out[k] = np.concatenate([a[k] for a in list_of_acc], axis=1) if isinstance(v, np.ndarray) and v.ndim >= 2 else v
    return out

_live = weakref.WeakSet()


@atexit.register
def _close_all():
    """contexts still alive at interpreter exit are destroyed HERE, while the HIP runtime and RCCL are intact —
    not from __del__ during module teardown, after other libraries' exit handlers may have run"""
    for m in list(_live):
        try:
            m.close()
        except Exception:
            pass


class HipModel:
    def __init__(self, grid: K.PiclesGrid, phys: K.PiclesPhys, ode: K.PiclesOde, model: K.PiclesModel,
                 mask=None, device: int = 0, halo_rows: int = 2, lib_path=None):
        self.lib = K.load(lib_path)
        self._mask = None
        if mask is not None:
            self._mask = np.ascontiguousarray(np.asarray(mask, dtype=np.int8).reshape(-1, order="F"))
            grid.mask = self._mask.ctypes.data_as(K.c_int8_p)
        if grid.j_end == 0 and grid.j_begin == 0:
            grid.j_end = grid.Ny
        self.Nx, self.Ny = grid.Nx, grid.Ny
        self.j_begin, self.j_end = grid.j_begin, grid.j_end
        self.ny_loc = self.j_end - self.j_begin
        self.N = self.Nx * self.ny_loc
        h = C.c_void_p()
        rc = self.lib.picles_create(C.byref(grid), C.byref(phys), C.byref(ode), C.byref(model),
                                    device, halo_rows, C.byref(h))
        if rc != 0:
            msg = self.lib.picles_last_error(None)
            raise K.PiclesError(f"picles_create failed (rc={rc}): {msg.decode() if msg else '?'}")
        self.h = h
        self.gen = 0          # bumped by every call that changes anything on the device
        self.state_gen = 0    # bumped by the calls that write the device State field — and only those: LazyState validates its
                              # mirror and a recorded `State .= 0` against it (set_particles, halo resizing, advance_rows, remesh
                              # leave State alone and must not cancel a recorded zero-fill)
        _live.add(self)

    # ---- lifetime ----
    def close(self):
        if getattr(self, "h", None):
            self.lib.picles_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        _check(self.lib, self.h, rc, what)

    # ---- inputs ----
    def set_winds(self, u0, v0, t0=0.0, u1=None, v1=None, t1=0.0, um=None, vm=None, tk=None):
        """node winds of the window [t0, t1]: one level (static), two (linear in t) or three — (um, vm) at (t0+t1)/2: the parabola;
        with `tk`: (um, vm) at the knot tk of a gridded wind, two straight segments (picles_set_winds_knot)"""
        u0, v0 = _col(u0, self.N), _col(v0, self.N)
        if u1 is not None:
            u1, v1 = _col(u1, self.N), _col(v1, self.N)
        if tk is not None and um is None:
            raise ValueError("set_winds: tk names the time of the level (um, vm); it was given without one")
        if um is not None:
            um, vm = _col(um, self.N), _col(vm, self.N)
            if tk is not None:
                self._ck(self.lib.picles_set_winds_knot(self.h, K.dptr(u0), K.dptr(v0), t0, K.dptr(um), K.dptr(vm), float(tk),
                                                        K.dptr(u1), K.dptr(v1), t1), "picles_set_winds_knot")
                return
            self._ck(self.lib.picles_set_winds3(self.h, K.dptr(u0), K.dptr(v0), t0, K.dptr(um), K.dptr(vm), K.dptr(u1), K.dptr(v1), t1),
                     "picles_set_winds3")
            return
        self._ck(self.lib.picles_set_winds(self.h, K.dptr(u0), K.dptr(v0), t0, K.dptr(u1), K.dptr(v1), t1),
                 "picles_set_winds")

    def set_winds_polyline(self, us, vs, times):
        """node winds at len(times) >= 2 strictly increasing times: the piecewise-linear wind through them (picles_set_winds_polyline) —
        a gridded wind sampled at every one of its time knots inside the step and at the step's ends"""
        import ctypes as C
        n = len(times)
        us = [_col(a, self.N) for a in us]
        vs = [_col(a, self.N) for a in vs]
        assert len(us) == n and len(vs) == n
        PP = C.POINTER(C.c_double) * n
        pu = PP(*[K.dptr(a) for a in us])
        pv = PP(*[K.dptr(a) for a in vs])
        tt = (C.c_double * n)(*[float(x) for x in times])
        self._ck(self.lib.picles_set_winds_polyline(self.h, n, pu, pv, tt), "picles_set_winds_polyline")

    def set_metric(self, m11, m22, pc):
        """per-node projection diag(m11, m22) and great-circle coefficient (picles_set_metric)"""
        a = [_col(x, self.N) for x in (m11, m22, pc)]
        self._ck(self.lib.picles_set_metric(self.h, K.dptr(a[0]), K.dptr(a[1]), K.dptr(a[2])), "picles_set_metric")

    def set_wind_grid(self, lat: dict, mesh_x0: float, mesh_y0: float, time_mode: str = "linear"):
        """upload an (x,y,t) wind lattice; the device samples it every step (picles_set_wind_grid).  time_mode "linear": the
        interpolant itself, time knots inside a step included (PICLES_LATTICE_LINEAR); "smooth3": the parabola through the lattice
        sampled at t, t+Δt/2, t+Δt — for a lattice that tabulates a smooth closure (PICLES_LATTICE_SMOOTH3)"""
        self._wg = (lat["u"], lat["v"])
        self._ck(self.lib.picles_set_wind_grid(self.h, lat["nx"], lat["ny"], lat["nt"], lat["x0"], lat["dx"], lat["y0"],
                                               lat["dy"], lat["t0"], lat["dt"], K.dptr(lat["u"]), K.dptr(lat["v"]),
                                               mesh_x0, mesh_y0), "picles_set_wind_grid")
        mode = {"linear": K.LATTICE_LINEAR, "smooth3": K.LATTICE_SMOOTH3}[time_mode]
        if mode != K.LATTICE_LINEAR:
            self._ck(self.lib.picles_set_wind_grid_mode(self.h, mode), "picles_set_wind_grid_mode")

    # ---- streamed winds (picles_wind_stream_*: a lattice whose time levels arrive one at a time, from device memory) ----
    def wind_stream_init(self, nx, ny, x0, dx, y0, dy, t0, dt, mesh_x0, mesh_y0, n_slots=3, time_mode="linear"):
        """a ring of n_slots >= 2 (u, v) levels on an (nx, ny) lattice, level k at t0 + k dt; replaces whatever winds the model had"""
        mode = {"linear": K.LATTICE_LINEAR, "smooth3": K.LATTICE_SMOOTH3}[time_mode]
        self._ck(self.lib.picles_wind_stream_init(self.h, int(nx), int(ny), float(x0), float(dx), float(y0), float(dy), float(t0), float(dt),
                                                  float(mesh_x0), float(mesh_y0), int(n_slots)), "picles_wind_stream_init")
        self._stream_shape = (int(nx), int(ny))
        if mode != K.LATTICE_LINEAR:
            self._ck(self.lib.picles_set_wind_grid_mode(self.h, mode), "picles_set_wind_grid_mode")

    def wind_stream_push(self, k, u, v):
        """level k: NumPy arrays (host; float32 or float64, anything else is converted to float64) or torch CUDA tensors (float32 /
        float64, contiguous), shape (ny, nx) or flat — nx * ny values, x fastest.  A tensor is handed over by pointer on torch's
        current stream: the library orders its copy behind what that stream holds, and the stream behind the copy"""
        nx, ny = getattr(self, "_stream_shape", (0, 0))
        n = nx * ny
        if hasattr(u, "data_ptr"):
            import torch
            for a in (u, v):
                if not a.is_cuda or a.dtype not in (torch.float32, torch.float64) or not a.is_contiguous():
                    raise ValueError("wind_stream_push: tensors must live on the device, be float32 or float64 and contiguous")
                if a.numel() != n or (a.dim() != 1 and tuple(a.shape) != (ny, nx)):
                    raise ValueError(f"wind_stream_push: a level is {ny} x {nx} values (shape (ny, nx) or flat), got {tuple(a.shape)}")
            if u.dtype != v.dtype:
                raise ValueError("wind_stream_push: u and v must have one dtype")
            dtype = K.WIND_F32 if u.dtype == torch.float32 else K.WIND_F64
            cur = torch.cuda.current_stream(u.device)
            if cur.cuda_stream:
                self._ck(self.lib.picles_wind_stream_push(self.h, int(k), u.data_ptr(), v.data_ptr(), dtype, K.WIND_DEVICE, cur.cuda_stream),
                         "picles_wind_stream_push")
                return
            # torch's default stream is the null stream, which the C ABI reads as "already synchronised": the hand-over goes through
            # a side stream ordered behind and in front of it, so the host still does not wait
            side = getattr(self, "_stream_side", None)
            if side is None:
                side = self._stream_side = torch.cuda.Stream(u.device)
            side.wait_stream(cur)
            try:
                self._ck(self.lib.picles_wind_stream_push(self.h, int(k), u.data_ptr(), v.data_ptr(), dtype, K.WIND_DEVICE, side.cuda_stream),
                         "picles_wind_stream_push")
            finally:
                cur.wait_stream(side)
            return
        f32 = all(getattr(a, "dtype", None) == np.float32 for a in (u, v))
        dt = np.float32 if f32 else np.float64
        u, v = (np.ascontiguousarray(np.asarray(a, dtype=dt)) for a in (u, v))
        for a in (u, v):
            if a.size != n or (a.ndim != 1 and a.shape != (ny, nx)):
                raise ValueError(f"wind_stream_push: a level is {ny} x {nx} values (shape (ny, nx) or flat), got {a.shape}")
        self._ck(self.lib.picles_wind_stream_push(self.h, int(k), u.ctypes.data, v.ctypes.data, K.WIND_F32 if f32 else K.WIND_F64,
                                                  K.WIND_HOST, None), "picles_wind_stream_push")

    def wind_stream_info(self):
        """(n_slots, oldest level held, newest level held, pushes so far); oldest = newest = -1: the ring is empty.  No device work"""
        s = C.c_int32()
        a = [C.c_int64() for _ in range(3)]
        if self.lib.picles_wind_stream_info(self.h, C.byref(s), *[C.byref(x) for x in a]) != 0:
            raise K.PiclesError("picles_wind_stream_info failed: wind_stream_init first")
        return (s.value,) + tuple(x.value for x in a)

    def wind_stream_reset(self):
        self._ck(self.lib.picles_wind_stream_reset(self.h), "picles_wind_stream_reset")

    def get_winds(self):
        out = [np.empty(self.N) for _ in range(4)]
        self._ck(self.lib.picles_get_winds(self.h, *[K.dptr(a) for a in out]), "picles_get_winds")
        return [a.reshape((self.Nx, self.ny_loc), order="F") for a in out]

    def get_winds_mid(self):
        """the mid-window level of three-level winds, or None when the current winds have two levels"""
        out = [np.empty(self.N) for _ in range(2)]
        rc = self.lib.picles_get_winds_mid(self.h, *[K.dptr(a) for a in out])
        if rc == 1:
            return None
        self._ck(rc, "picles_get_winds_mid")
        return [a.reshape((self.Nx, self.ny_loc), order="F") for a in out]

    def seed(self, t0=0.0):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_seed(self.h, t0), "picles_seed")

    # ---- stepping ----
    def time_step(self, dt, flags=0):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_time_step(self.h, dt, flags), "picles_time_step")

    def run_steps(self, dt, n):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_run_steps(self.h, dt, n), "picles_run_steps")

    def advance(self, dt, flags=0):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_advance(self.h, dt, flags), "picles_advance")

    def remesh(self, dt):
        self.gen += 1
        self._ck(self.lib.picles_remesh(self.h, dt), "picles_remesh")

    def tick(self, dt):
        self._ck(self.lib.picles_tick(self.h, dt), "picles_tick")

    def zero_state(self):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_zero_state(self.h), "picles_zero_state")

    def sync(self):
        self._ck(self.lib.picles_sync(self.h), "picles_sync")

    @property
    def clock(self):
        return self.lib.picles_clock(self.h)

    # ---- split phases (slab-partitioned step) ----
    def begin_step(self, dt, flags=0):
        self.gen += 1
        self._ck(self.lib.picles_begin_step(self.h, dt, flags), "picles_begin_step")

    def advance_rows(self, which, stream=None):
        self.gen += 1
        self._ck(self.lib.picles_advance_rows(self.h, which, stream), "picles_advance_rows")

    def scatter_remesh(self, stream=None):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_scatter_remesh(self.h, stream), "picles_scatter_remesh")

    def begin_fused_step(self, dt) -> bool:
        """True if the step runs as fused k_step launches (step_rows / end_fused_step)"""
        rc = self.lib.picles_begin_fused_step(self.h, dt)
        if rc < 0:
            self._ck(rc, "picles_begin_fused_step")
        return rc == 0

    def step_rows(self, which, stream=None):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_step_rows(self.h, which, stream), "picles_step_rows")

    def end_fused_step(self):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_end_fused_step(self.h), "picles_end_fused_step")

    def halo_send(self, side):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self.lib.picles_halo_send_dev(self.h, side, C.byref(p), C.byref(n)), "picles_halo_send_dev")
        return p.value, n.value

    def halo_recv(self, side):
        p, n = C.c_void_p(), C.c_size_t()
        self._ck(self.lib.picles_halo_recv_dev(self.h, side, C.byref(p), C.byref(n)), "picles_halo_recv_dev")
        return p.value, n.value

    @property
    def halo_rows(self):
        return self.lib.picles_halo_rows(self.h)

    def set_halo_rows(self, r):
        self.gen += 1
        self._ck(self.lib.picles_set_halo_rows(self.h, r), "picles_set_halo_rows")

    def set_slab_mode(self, on=True):
        """a whole-grid context behaves as a slab: the periodic y wrap goes through the ghost rows (ring of one)"""
        self._ck(self.lib.picles_set_slab_mode(self.h, int(on)), "picles_set_slab_mode")

    # ---- native slab ring (RCCL send/recv driven from C) ----
    def slab_unique_id(self) -> bytes:
        buf = C.create_string_buffer(K.SLAB_ID_BYTES)
        rc = self.lib.picles_slab_unique_id(buf)
        if rc != 0:
            msg = self.lib.picles_last_error(None)
            raise K.PiclesError(f"picles_slab_unique_id failed (rc={rc}): {msg.decode() if msg else '?'}")
        return buf.raw

    def slab_comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == K.SLAB_ID_BYTES
        buf = C.create_string_buffer(unique_id, K.SLAB_ID_BYTES)
        self._ck(self.lib.picles_slab_comm_init(self.h, buf, rank, world), "picles_slab_comm_init")

    def slab_run_steps(self, dt, n, flags=K.STEP_ZERO_FIRST):
        self.gen += 1
        self.state_gen += 1
        self._ck(self.lib.picles_slab_run_steps(self.h, dt, n, flags), "picles_slab_run_steps")

    def slab_exchange(self):
        self._ck(self.lib.picles_slab_exchange(self.h), "picles_slab_exchange")

    def slab_streams(self):
        e, m = C.c_void_p(), C.c_void_p()
        self._ck(self.lib.picles_slab_streams(self.h, C.byref(e), C.byref(m)), "picles_slab_streams")
        return e.value, m.value

    def slab_phases(self):
        """where the ring steps' time went since the last call (picles_slab_get_phases; needs enable_timing(1)): per-step means
        [ms] of the edge launch, the exchange behind it and the interior launch, and how often the exchange was hidden"""
        p = K.PiclesSlabPhases()
        self._ck(self.lib.picles_slab_get_phases(self.h, C.byref(p)), "picles_slab_get_phases")
        d = p.as_dict()
        n = max(d["steps"], 1)
        return {"steps": d["steps"], "exchange_hidden_steps": d["exchange_hidden"], "edge_ms": d["edge_ms"] / n,
                "exchange_ms": d["exchange_ms"] / n, "interior_ms": d["interior_ms"] / n, "slack_ms": d["slack_ms"] / n,
                "span_ms": d["span_ms"] / n}

    def slab_comm_destroy(self):
        self._ck(self.lib.picles_slab_comm_destroy(self.h), "picles_slab_comm_destroy")

    # ---- outputs ----
    def get_state(self):
        s = np.empty(3 * self.N)
        self._ck(self.lib.picles_get_state(self.h, K.dptr(s)), "picles_get_state")
        return s.reshape((self.Nx, self.ny_loc, 3), order="F")

    def set_state(self, s):
        self.gen += 1
        self.state_gen += 1
        s = _col(s, 3 * self.N)
        self._ck(self.lib.picles_set_state(self.h, K.dptr(s)), "picles_set_state")

    def get_movie_state(self):
        s = np.empty(3 * self.N)
        self._ck(self.lib.picles_get_movie_state(self.h, K.dptr(s)), "picles_get_movie_state")
        return s.reshape((self.Nx, self.ny_loc, 3), order="F")

    # ---- snapshot ring ----
    def store_init(self, n_slots=3):
        self._ck(self.lib.picles_store_init(self.h, n_slots), "picles_store_init")

    def store_push(self):
        self._ck(self.lib.picles_store_push(self.h), "picles_store_push")

    def store_pop(self):
        s = np.empty(3 * self.N)
        t = C.c_double()
        self._ck(self.lib.picles_store_pop(self.h, K.dptr(s), C.byref(t)), "picles_store_pop")
        return s.reshape((self.Nx, self.ny_loc, 3), order="F"), t.value

    @property
    def store_pending(self):
        return self.lib.picles_store_pending(self.h)

    # ---- coarse wave diagnostics (picles_diag_*: Hs / Tp / group velocity planes + global sums, reduced on the device) ----
    def diag_init(self, coarsen=(4, 4), fields=("hs", "tp", "cg_x", "cg_y"), n_slots=3):
        """coarsen = (cx, cy), each 1 ... 16; fields: names out of _capi.DIAG_FIELDS (the planes come in that order, whatever the
        order given here) or the bit mask itself"""
        cx, cy = (coarsen, coarsen) if np.isscalar(coarsen) else coarsen
        mask = diag_field_mask(fields)
        self._ck(self.lib.picles_diag_init(self.h, int(cx), int(cy), mask, int(n_slots)), "picles_diag_init")
        self.diag_fields = tuple(f for f in K.DIAG_FIELDS if mask & K.DIAG_BITS[f])
        self.diag_coarsen = (int(cx), int(cy))

    def diag_shape(self):
        """(Nxc, nyc_loc, n_fields, n_partials, bytes of the float32 field block); no device work"""
        a = [C.c_int32() for _ in range(4)]
        b = C.c_size_t()
        rc = self.lib.picles_diag_shape(self.h, *[C.byref(x) for x in a], C.byref(b))
        if rc != 0:
            raise K.PiclesError("picles_diag_shape failed: diag_init first")
        return tuple(x.value for x in a) + (b.value,)

    def diag_push(self):
        self._ck(self.lib.picles_diag_push(self.h), "picles_diag_push")

    def diag_pop(self):
        """the oldest snapshot: (fields float32 [n_fields, Nxc, nyc_loc] — each plane Fortran-ordered, i.e. [I + Nxc J] in memory —,
        partials float64 [n_partials, 7], model time)"""
        nxc, nyc, nf, npart, _ = self.diag_shape()
        f = np.empty(nf * nxc * nyc, dtype=np.float32)
        p = np.empty((npart, 7))
        t = C.c_double()
        self._ck(self.lib.picles_diag_pop(self.h, f.ctypes.data, K.dptr(p), C.byref(t)), "picles_diag_pop")
        return f.reshape((nf, nyc, nxc)).transpose(0, 2, 1), p, t.value

    def diag_export(self, fields, partials=None):
        """the snapshot of diag_push, written into torch CUDA tensors instead of a ring slot (picles_diag_export): `fields` float32,
        contiguous, n_fields * Nxc * nyc_loc values (the memory layout of diag_pop: [n_fields, nyc_loc, Nxc]); `partials` float64
        [n_partials, 7] or None.  Nothing is copied to the host; torch's current stream is ordered behind the kernel"""
        import torch
        nxc, nyc, nf, npart, _ = self.diag_shape()
        if not (fields.is_cuda and fields.dtype == torch.float32 and fields.is_contiguous() and fields.numel() == nf * nxc * nyc):
            raise ValueError(f"diag_export: fields must be a contiguous float32 device tensor of {nf} x {nyc} x {nxc} values")
        if partials is not None and not (partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
                                         and partials.numel() == npart * 7):
            raise ValueError(f"diag_export: partials must be a contiguous float64 device tensor of {npart} x 7 values")
        cur = torch.cuda.current_stream(fields.device)
        s = cur
        if not cur.cuda_stream:          # torch's default stream is the null stream: ordered through a side stream (wind_stream_push)
            s = getattr(self, "_stream_side", None)
            if s is None:
                s = self._stream_side = torch.cuda.Stream(fields.device)
            s.wait_stream(cur)
        try:
            self._ck(self.lib.picles_diag_export(self.h, fields.data_ptr(), None if partials is None else C.cast(partials.data_ptr(), K.c_double_p),
                                                 s.cuda_stream), "picles_diag_export")
        finally:
            if s is not cur:
                cur.wait_stream(s)

    @property
    def diag_pending(self):
        return self.lib.picles_diag_pending(self.h)

    # ---- coupling fluxes (picles_flux_*: wind input, dissipation, stress and Stokes drift planes + area totals, on the device) ----
    def flux_init(self, coarsen=(4, 4), fields=K.FLUX_FIELDS, scale_phi=1.0, scale_tau=1.0, n_slots=3):
        """coarsen = (cx, cy), each 1 ... 16; fields: names out of _capi.FLUX_FIELDS (the planes come in that order, whatever the
        order given here) or the bit mask itself; scale_phi multiplies the three phi planes (rho_water * g: W m^-2), scale_tau the
        four tq planes (rho_water: N m^-2)"""
        cx, cy = (coarsen, coarsen) if np.isscalar(coarsen) else coarsen
        mask = flux_field_mask(fields)
        self._ck(self.lib.picles_flux_init(self.h, int(cx), int(cy), mask, float(scale_phi), float(scale_tau), int(n_slots)), "picles_flux_init")
        self.flux_fields = tuple(f for f in K.FLUX_FIELDS if mask & K.FLUX_BITS[f])
        self.flux_coarsen = (int(cx), int(cy))

    def flux_shape(self):
        """(Nxc, nyc_loc, n_fields, n_partials, bytes of the float32 field block); no device work"""
        a = [C.c_int32() for _ in range(4)]
        b = C.c_size_t()
        rc = self.lib.picles_flux_shape(self.h, *[C.byref(x) for x in a], C.byref(b))
        if rc != 0:
            raise K.PiclesError("picles_flux_shape failed: flux_init first")
        return tuple(x.value for x in a) + (b.value,)

    def flux_push(self):
        self._ck(self.lib.picles_flux_push(self.h), "picles_flux_push")

    def flux_pop(self):
        """the oldest snapshot: (planes float32 [n_fields, Nxc, nyc_loc] — each plane Fortran-ordered, i.e. [I + Nxc J] in memory —,
        partials float64 [n_partials, 11], model time)"""
        nxc, nyc, nf, npart, _ = self.flux_shape()
        f = np.empty(nf * nxc * nyc, dtype=np.float32)
        p = np.empty((npart, K.FLUX_NPARTIAL))
        t = C.c_double()
        self._ck(self.lib.picles_flux_pop(self.h, f.ctypes.data, K.dptr(p), C.byref(t)), "picles_flux_pop")
        return f.reshape((nf, nyc, nxc)).transpose(0, 2, 1), p, t.value

    def flux_export(self, fields, partials=None):
        """the snapshot of flux_push, written into torch CUDA tensors instead of a ring slot (picles_flux_export): `fields` float32,
        contiguous, n_fields * Nxc * nyc_loc values (the memory layout of flux_pop: [n_fields, nyc_loc, Nxc]); `partials` float64
        [n_partials, 11] or None.  Nothing is copied to the host; torch's current stream is ordered behind the kernel"""
        import torch
        nxc, nyc, nf, npart, _ = self.flux_shape()
        if not (fields.is_cuda and fields.dtype == torch.float32 and fields.is_contiguous() and fields.numel() == nf * nxc * nyc):
            raise ValueError(f"flux_export: fields must be a contiguous float32 device tensor of {nf} x {nyc} x {nxc} values")
        if partials is not None and not (partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
                                         and partials.numel() == npart * K.FLUX_NPARTIAL):
            raise ValueError(f"flux_export: partials must be a contiguous float64 device tensor of {npart} x {K.FLUX_NPARTIAL} values")
        cur = torch.cuda.current_stream(fields.device)
        s = cur
        if not cur.cuda_stream:          # torch's default stream is the null stream: ordered through a side stream (diag_export)
            s = getattr(self, "_stream_side", None)
            if s is None:
                s = self._stream_side = torch.cuda.Stream(fields.device)
            s.wait_stream(cur)
        try:
            self._ck(self.lib.picles_flux_export(self.h, fields.data_ptr(), None if partials is None else C.cast(partials.data_ptr(), K.c_double_p),
                                                 s.cuda_stream), "picles_flux_export")
        finally:
            if s is not cur:
                cur.wait_stream(s)

    def flux_free(self):
        self._ck(self.lib.picles_flux_free(self.h), "picles_flux_free")
        self.flux_fields = ()

    @property
    def flux_pending(self):
        return self.lib.picles_flux_pending(self.h)

    # ---- flux means (picles_flux_mean_*: the coupling fluxes accumulated behind every step, exported as interval means) ----
    def flux_mean_init(self, every=1, first=1):
        """a mean set over the flux set's cells (flux_init first): an update follows every model step s (counted from here) with
        s >= first and (s - first) % every == 0; a pending fused step stays pending"""
        self._ck(self.lib.picles_flux_mean_init(self.h, int(every), int(first)), "picles_flux_mean_init")

    def flux_mean_shape(self):
        """(every, n_planes = 11, bytes of the accumulator planes); no device work"""
        ev, npl = C.c_int32(), C.c_int32()
        b = C.c_size_t()
        if self.lib.picles_flux_mean_shape(self.h, C.byref(ev), C.byref(npl), C.byref(b)) != 0:
            raise K.PiclesError("picles_flux_mean_shape failed: flux_mean_init first")
        return ev.value, npl.value, b.value

    def flux_mean_update(self, stream=None):
        """one update now (callers of the split-phase API, on the stream their step is ordered on)"""
        self._ck(self.lib.picles_flux_mean_update(self.h, stream), "picles_flux_mean_update")

    def flux_mean_push(self, reset=True):
        """the mean over the samples held into the next slot of the flux ring (flux_pop serves it); reset: zero behind it"""
        self._ck(self.lib.picles_flux_mean_push(self.h, 1 if reset else 0), "picles_flux_mean_push")

    def flux_mean_export(self, fields, partials=None, reset=True):
        """the mean of flux_mean_push written into torch CUDA tensors (picles_flux_mean_export): the arguments of flux_export"""
        import torch
        nxc, nyc, nf, npart, _ = self.flux_shape()
        if not (fields.is_cuda and fields.dtype == torch.float32 and fields.is_contiguous() and fields.numel() == nf * nxc * nyc):
            raise ValueError(f"flux_mean_export: fields must be a contiguous float32 device tensor of {nf} x {nyc} x {nxc} values")
        if partials is not None and not (partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
                                         and partials.numel() == npart * K.FLUX_NPARTIAL):
            raise ValueError(f"flux_mean_export: partials must be a contiguous float64 device tensor of {npart} x {K.FLUX_NPARTIAL} values")
        cur = torch.cuda.current_stream(fields.device)
        s = cur
        if not cur.cuda_stream:          # torch's default stream is the null stream: ordered through a side stream (flux_export)
            s = getattr(self, "_stream_side", None)
            if s is None:
                s = self._stream_side = torch.cuda.Stream(fields.device)
            s.wait_stream(cur)
        try:
            self._ck(self.lib.picles_flux_mean_export(self.h, fields.data_ptr(), None if partials is None else C.cast(partials.data_ptr(), K.c_double_p),
                                                      s.cuda_stream, 1 if reset else 0), "picles_flux_mean_export")
        finally:
            if s is not cur:
                cur.wait_stream(s)

    def flux_mean_get(self):
        """the raw accumulators: {"acc": float64 [11, Nxc, nyc_loc] (each plane [I + Nxc J] in memory: the nine sums in plane order,
        n_active, n_bad), "n_samples", "t_first", "t_last"}; waits for the latest operation on them alone"""
        nxc, nyc, _, _, _ = self.flux_shape()
        buf = np.empty(K.FLUX_NPARTIAL * nxc * nyc)
        n, t0, t1 = C.c_int64(), C.c_double(), C.c_double()
        self._ck(self.lib.picles_flux_mean_get(self.h, K.dptr(buf), C.byref(n), C.byref(t0), C.byref(t1)), "picles_flux_mean_get")
        return dict(acc=buf.reshape((K.FLUX_NPARTIAL, nyc, nxc)).transpose(0, 2, 1), n_samples=int(n.value), t_first=float(t0.value),
                    t_last=float(t1.value))

    def flux_mean_scalars(self):
        """(n_samples, t_first, t_last) of the mean set: host-side values, no device work"""
        n, t0, t1 = C.c_int64(), C.c_double(), C.c_double()
        self._ck(self.lib.picles_flux_mean_get(self.h, None, C.byref(n), C.byref(t0), C.byref(t1)), "picles_flux_mean_get")
        return int(n.value), float(t0.value), float(t1.value)

    def flux_mean_set(self, acc):
        """upload what flux_mean_get returned: how a picked-up run continues an open interval"""
        nxc, nyc, _, _, _ = self.flux_shape()
        a = np.asarray(acc["acc"], dtype=np.float64)
        if a.shape != (K.FLUX_NPARTIAL, nxc, nyc):
            raise ValueError(f"flux_mean_set: acc must be {K.FLUX_NPARTIAL} x {nxc} x {nyc}, got {a.shape}")
        buf = np.ascontiguousarray(a.transpose(0, 2, 1))
        self._ck(self.lib.picles_flux_mean_set(self.h, K.dptr(buf), int(acc["n_samples"]), float(acc["t_first"]), float(acc["t_last"])),
                 "picles_flux_mean_set")

    def flux_mean_reset(self):
        self._ck(self.lib.picles_flux_mean_reset(self.h), "picles_flux_mean_reset")

    def flux_mean_free(self):
        self._ck(self.lib.picles_flux_mean_free(self.h), "picles_flux_mean_free")

    # ---- station probes (picles_probe_*: the State value of chosen nodes behind every step, the fused path kept) ----
    def probe_init(self, nodes, every=1, first=1, capacity=64):
        """nodes: (n, 2) global 0-based (i, j), j inside this context's rows; a sample is taken after every model step s (counted
        from here) with s >= first and (s - first) % every == 0; `capacity` samples may wait for probe_pop"""
        ij = np.asarray(nodes, dtype=np.int64)
        if ij.ndim != 2 or ij.shape[1] != 2:
            raise ValueError("probe_init: nodes must be an (n, 2) array of (i, j)")
        if ij.size and (np.abs(ij).max() > 2**31 - 1):
            raise ValueError("probe_init: node index out of the int32 range")
        planes = np.ascontiguousarray(ij.T.astype(np.int32))
        self._ck(self.lib.picles_probe_init(self.h, int(ij.shape[0]), planes.ctypes.data_as(K.c_int32_p), int(every), int(first),
                                            int(capacity)), "picles_probe_init")

    def probe_shape(self):
        """(n, every, capacity) of the probe set; no device work"""
        a = [C.c_int32() for _ in range(3)]
        if self.lib.picles_probe_shape(self.h, *[C.byref(x) for x in a]) != 0:
            raise K.PiclesError("picles_probe_shape failed: probe_init first")
        return tuple(x.value for x in a)

    def probe_sample(self, stream=None):
        """one sample now (the seeded state; callers of the split-phase API, on the stream their step is ordered on)"""
        self._ck(self.lib.picles_probe_sample(self.h, stream), "picles_probe_sample")

    def probe_pop(self, max_samples=None):
        """the oldest samples, up to max_samples (all pending when None): (values [samples, 3, n], times [samples], steps [samples])"""
        n, _, cap = self.probe_shape()
        m = cap if max_samples is None else int(max_samples)
        m = max(1, min(m, max(self.probe_pending, 1)))
        v = np.empty((m, 3, n))
        t = np.empty(m)
        s = np.empty(m, dtype=np.int64)
        got = C.c_int32()
        self._ck(self.lib.picles_probe_pop(self.h, m, K.dptr(v), K.dptr(t), s.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(got)),
                 "picles_probe_pop")
        return v[:got.value], t[:got.value], s[:got.value]

    @property
    def probe_pending(self):
        return self.lib.picles_probe_pending(self.h)

    def probe_free(self):
        self._ck(self.lib.picles_probe_free(self.h), "picles_probe_free")

    # ---- track samples (picles_track_*: sea state at events along moving platforms, kept in a table on the device) ----
    def track_init(self, times, corners_ij, weights, horizon):
        """times: (m,) nondecreasing; corners_ij: (8, m) int, the i of the four corners then their j (global, 0-based, in the
        visiting order of station_output.locate_points); weights: (4, m), finite and >= 0; horizon: the longest step to come"""
        t = np.ascontiguousarray(times, dtype=np.float64)
        ij = np.asarray(corners_ij, dtype=np.int64)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        m = t.shape[0] if t.ndim == 1 else -1
        if m < 0 or ij.shape != (8, m) or w.shape != (4, m):
            raise ValueError("track_init: times (m,), corners_ij (8, m) and weights (4, m) are needed")
        if ij.size and np.abs(ij).max() > 2**31 - 1:
            raise ValueError("track_init: node index out of the int32 range")
        if m > (2**31 - 1) // 8:
            raise ValueError("track_init: 8 m must not exceed INT32_MAX")
        planes = np.ascontiguousarray(ij.astype(np.int32))
        self._ck(self.lib.picles_track_init(self.h, int(m), K.dptr(t), planes.ctypes.data_as(K.c_int32_p), K.dptr(w), float(horizon)),
                 "picles_track_init")

    def track_info(self):
        """(m, horizon, samples taken) of the track set; no device work"""
        m, h, s = C.c_int32(), C.c_double(), C.c_int64()
        if self.lib.picles_track_info(self.h, C.byref(m), C.byref(h), C.byref(s)) != 0:
            raise K.PiclesError("picles_track_info failed: track_init first")
        return m.value, h.value, s.value

    def track_sample(self, stream=None):
        """one sample now, at the model clock (the seeded state; callers of the split-phase API, on the stream their step is ordered on)"""
        self._ck(self.lib.picles_track_sample(self.h, stream), "picles_track_sample")

    def track_fetch_begin(self, k0, n):
        """start the copy of the table's 8 planes of the events [k0, k0 + n), as they are behind the work enqueued so far"""
        self._ck(self.lib.picles_track_fetch_begin(self.h, int(k0), int(n)), "picles_track_fetch_begin")
        self._track_fetch_n = int(n)

    def track_fetch_end(self):
        """wait for that copy alone: (8, n) float64, rows e_b, mx_b, my_b, t_b, e_a, mx_a, my_a, t_a"""
        out = np.empty((8, getattr(self, "_track_fetch_n", 0) or 1))
        self._ck(self.lib.picles_track_fetch_end(self.h, K.dptr(out)), "picles_track_fetch_end")
        self._track_fetch_n = 0
        return out

    def track_free(self):
        self._track_fetch_n = 0
        self._ck(self.lib.picles_track_free(self.h), "picles_track_free")

    # ---- run statistics (picles_stat_*: per-node peak / mean / exceedance accumulators kept on the device, the fused path kept) ----
    def stat_init(self, groups=K.STAT_ALL, thresholds=(), every=1, first=1):
        """groups: PICLES_STAT_* bits or names ("peak", "mean", "exceed"); thresholds: 1 ... 4 ascending Hs values with "exceed";
        an update follows every model step s (counted from here) with s >= first and (s - first) % every == 0"""
        mask = stat_mask(groups)
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).ravel())
        self._ck(self.lib.picles_stat_init(self.h, mask, int(thr.size), K.dptr(thr) if thr.size else None, int(every), int(first)),
                 "picles_stat_init")

    def stat_shape(self):
        """(mask, thresholds, every, n_planes, bytes) of the statistics set; no device work"""
        m, nt, ev, npl = (C.c_int32() for _ in range(4))
        thr = (C.c_double * 4)()
        b = C.c_size_t()
        if self.lib.picles_stat_shape(self.h, C.byref(m), C.byref(nt), thr, C.byref(ev), C.byref(npl), C.byref(b)) != 0:
            raise K.PiclesError("picles_stat_shape failed: stat_init first")
        return m.value, tuple(thr[k] for k in range(nt.value)), ev.value, npl.value, b.value

    def stat_update(self, stream=None):
        """one update now (the seeded state; callers of the split-phase API, on the stream their step is ordered on)"""
        self._ck(self.lib.picles_stat_update(self.h, stream), "picles_stat_update")

    def stat_get(self, groups=None):
        """the accumulators of the selected groups (all of the set's when None) as a dict of (Nx, ny_loc) planes — "n_exc" is
        (Nx, ny_loc, n_thresholds) — with "n_samples", "t_first", "t_last"; a pending fused step stays pending"""
        set_mask, thr, _, _, _ = self.stat_shape()
        mask = set_mask if groups is None else stat_mask(groups, allow_empty=True)
        lay = stat_layout(mask, len(thr))
        buf = np.empty(sum(np.dtype(dt).itemsize * k for _, dt, k in lay) * self.N, dtype=np.uint8)
        n, t0, t1 = C.c_int64(), C.c_double(), C.c_double()
        self._ck(self.lib.picles_stat_get(self.h, mask, buf.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(t0), C.byref(t1)),
                 "picles_stat_get")
        out = stat_unpack(buf, lay, self.Nx, self.ny_loc)
        out.update(n_samples=int(n.value), t_first=float(t0.value), t_last=float(t1.value), thresholds=np.asarray(thr), mask=mask)
        return out

    def stat_set(self, acc):
        """upload what stat_get returned (the groups it holds): how a picked-up run continues its open window"""
        _, thr, _, _, _ = self.stat_shape()
        mask = int(acc["mask"]) if "mask" in acc else stat_mask_of(acc)
        buf = stat_pack(acc, stat_layout(mask, len(thr)), self.Nx, self.ny_loc)
        self._ck(self.lib.picles_stat_set(self.h, mask, buf.ctypes.data_as(C.c_void_p), int(acc["n_samples"]), float(acc["t_first"]),
                                          float(acc["t_last"])), "picles_stat_set")

    def stat_reset(self):
        self._ck(self.lib.picles_stat_reset(self.h), "picles_stat_reset")

    def stat_free(self):
        self._ck(self.lib.picles_stat_free(self.h), "picles_stat_free")

    # ---- open-boundary forcing (picles_bforce_*: prescribed sea state at rim nodes, born and advanced behind every step's launch) ----
    def bforce_init(self, nodes, weights=None):
        """nodes: (n, 2) global 0-based (i, j), each a grid-boundary node (mask class 3) of a model without periodic_boundary, each once.
        With weights the call is bforce_init_band's (ocean nodes are taken there too)"""
        if weights is not None:
            return self.bforce_init_band(nodes, weights)
        planes = _int32_planes(nodes, "bforce_init", "node index", pairs=True)
        self._ck(self.lib.picles_bforce_init(self.h, planes.shape[1], _p32(planes)), "picles_bforce_init")

    def bforce_init_band(self, nodes, weights=None):
        """a band set: nodes as for bforce_init, of mask class 3 or 1 (ocean: not stepped while the set lives); weights: None
        (every node 1.0) or n values in (0, 1] — the prescribed value is blended into the model's own State, v = m + w (p - m)"""
        planes = _int32_planes(nodes, "bforce_init_band", "node index", pairs=True)
        n, w = planes.shape[1], None
        if weights is not None:
            w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
            if w.shape != (n,):
                raise ValueError(f"bforce_init_band: expected {n} weights, got {w.shape[0]}")
        self._ck(self.lib.picles_bforce_init_band(self.h, n, _p32(planes), K.dptr(w)), "picles_bforce_init_band")

    def bforce_set_levels(self, t0, v0, t1=None, v1=None):
        """v0 (and v1): (n, 3) values (e, m_x, m_y) per forced node at t0 (and t1 > t0); one level: constant in time"""
        n = self.bforce_info()[0]
        def planes(v):
            v = np.asarray(v, dtype=np.float64)
            if v.shape != (n, 3):
                raise ValueError(f"bforce_set_levels: expected an ({n}, 3) array of (e, m_x, m_y), got {v.shape}")
            return np.ascontiguousarray(v.T)
        a = planes(v0)
        b = None if v1 is None else planes(v1)
        self._ck(self.lib.picles_bforce_set_levels(self.h, float(t0), K.dptr(a), float(t0 if t1 is None else t1), K.dptr(b)),
                 "picles_bforce_set_levels")

    def bforce_info(self):
        """(n, levels held: 0, 1 or 2, t0, t1) of the forcing set; no device work"""
        n, lv = C.c_int32(), C.c_int32()
        t0, t1 = C.c_double(), C.c_double()
        if self.lib.picles_bforce_info(self.h, C.byref(n), C.byref(lv), C.byref(t0), C.byref(t1)) != 0:
            raise K.PiclesError("picles_bforce_info failed: bforce_init first")
        return n.value, lv.value, t0.value, t1.value

    def bforce_free(self):
        self.gen += 1
        self._feedback_goes()
        self._ck(self.lib.picles_bforce_free(self.h), "picles_bforce_free")

    def bforce_get_levels(self):
        """the levels as the device holds them: (v0, v1), each (n, 3) of (e, m_x, m_y) or None where the set does not hold it;
        stream-ordered behind whatever wrote them, completes no pending step"""
        n, lv, _, _ = self.bforce_info()
        a = np.empty((3, n)) if lv >= 1 else None
        b = np.empty((3, n)) if lv >= 2 else None
        self._ck(self.lib.picles_bforce_get_levels(self.h, K.dptr(a), K.dptr(b)), "picles_bforce_get_levels")
        return (None if a is None else np.ascontiguousarray(a.T)), (None if b is None else np.ascontiguousarray(b.T))

    # ---- one-way nesting (picles_nest_*: this model's forcing set takes its levels from a parent model's State, on the device) ----
    def nest_init(self, parent, corner_nodes, index, weights):
        """parent: the HipModel to sample; corner_nodes (n_corner, 2): distinct 0-based (i, j) in the parent; index (n, 4) into
        corner_nodes and weights (n, 4), per node of this model's forcing set in the set's order (one to four columns: missing
        corners repeat the first with weight 0.0, which adds nothing)"""
        cn = np.asarray(corner_nodes, dtype=np.int64).reshape(-1, 2)
        ph = getattr(parent, "h", parent)
        if self.lib.picles_bforce_info(self.h, None, None, None, None) != 0:      # no set: the library says what is missing
            self._ck(self.lib.picles_nest_init(self.h, ph, 0, None, None, None), "picles_nest_init")
        n = self.bforce_info()[0]
        ix, w = np.asarray(index, dtype=np.int64), np.asarray(weights, dtype=np.float64)
        if ix.ndim != 2 or ix.shape != w.shape or ix.shape[0] != n or not 1 <= ix.shape[1] <= 4:
            raise ValueError(f"nest_init: index and weights must both be ({n}, 1..4) arrays, got {ix.shape} and {w.shape}")
        if ix.shape[1] < 4:
            pad = 4 - ix.shape[1]
            ix = np.concatenate([ix, np.repeat(ix[:, :1], pad, axis=1)], axis=1)
            w = np.concatenate([w, np.zeros((n, pad))], axis=1)
        cplanes, iplanes, wplanes = _int32_planes(cn, "nest_init"), _int32_planes(ix, "nest_init"), np.ascontiguousarray(w.T)
        self._ck(self.lib.picles_nest_init(self.h, ph, cplanes.shape[1], _p32(cplanes), _p32(iplanes), K.dptr(wplanes)), "picles_nest_init")
        self._nest_parent = parent if hasattr(parent, "gen") else None

    def nest_sample(self):
        """rotate the levels and take a new one from the parent as it stands now; returns after enqueueing"""
        self._ck(self.lib.picles_nest_sample(self.h), "picles_nest_sample")

    def nest_set_levels(self, t0, v0, t1, v1):
        """a nest resumed: the pair a checkpointed child held — v0, v1 (n, 3) as bforce_get_levels gave them, NaN rows included,
        over [t0, t1] — put back into a fresh nest as if two samples had been taken; the parent's clock must be t1"""
        n = self.bforce_info()[0]
        def planes(v):
            v = np.asarray(v, dtype=np.float64)
            if v.shape != (n, 3):
                raise ValueError(f"nest_set_levels: expected an ({n}, 3) array of (e, m_x, m_y), got {v.shape}")
            return np.ascontiguousarray(v.T)
        a, b = planes(v0), planes(v1)
        self._ck(self.lib.picles_nest_set_levels(self.h, float(t0), K.dptr(a), float(t1), K.dptr(b)), "picles_nest_set_levels")

    def nest_info(self):
        """(n_corner, samples taken) of this model's nest"""
        nc, s = C.c_int32(), C.c_int64()
        if self.lib.picles_nest_info(self.h, C.byref(nc), C.byref(s)) != 0:
            raise K.PiclesError("picles_nest_info failed: nest_init first")
        return nc.value, s.value

    def nest_free(self):
        self._feedback_goes()
        self._ck(self.lib.picles_nest_free(self.h), "picles_nest_free")

    def _prolong_tables(self, who, ix0, ix1, wx, iy0, iy1, wy):
        """the six per-axis tables of nest_prolong / nest_relocate, shapes checked, as the library takes them: (a0, a1, wx, b0, b1, wy)"""
        ints = [np.ascontiguousarray(a, dtype=np.int64) for a in (ix0, ix1, iy0, iy1)]
        w = [np.ascontiguousarray(a, dtype=np.float64) for a in (wx, wy)]
        for a, b, n, axis in ((ints[0], ints[1], self.Nx, "x"), (ints[2], ints[3], self.ny_loc, "y")):
            if not (a.shape == b.shape == (n,)):
                raise ValueError(f"{who}: the {axis} index tables must hold {n} entries each, got {a.shape} and {b.shape}")
        if w[0].shape != (self.Nx,) or w[1].shape != (self.ny_loc,):
            raise ValueError(f"{who}: the weight tables must hold {self.Nx} and {self.ny_loc} entries, got {w[0].shape} and {w[1].shape}")
        a0, a1, b0, b1 = (_int32_planes(a.reshape(-1, 1), who).reshape(-1) for a in ints)
        return a0, a1, w[0], b0, b1, w[1]

    def nest_prolong(self, parent, ix0, ix1, wx, iy0, iy1, wy, dt):
        """this model started from `parent` (a HipModel) at the parent's clock: the parent's State prolonged onto every node of this
        model, and the particles the remesh makes of it with step `dt` (picles_nest_prolong; nesting.prolong_tables gives the six
        per-axis tables: 0-based parent columns / rows and weights in [0, 1] per child column / row)"""
        ph = getattr(parent, "h", parent)
        a0, a1, fx, b0, b1, fy = self._prolong_tables("nest_prolong", ix0, ix1, wx, iy0, iy1, wy)
        # (State is replaced too: the model layer resets its lazy view after the start — nesting.start_from_parent — as after a step)
        self.gen += 1
        self._ck(self.lib.picles_nest_prolong(self.h, ph, _p32(a0), _p32(a1), K.dptr(fx), _p32(b0), _p32(b1), K.dptr(fy), float(dt)),
                 "picles_nest_prolong")

    def nest_relocate(self, parent, si, sj, keep_margin, ix0, ix1, wx, iy0, iy1, wy, dt, mesh_x0=0.0, mesh_y0=0.0):
        """this model's box moved by (si, sj) of its own nodes across `parent` (a HipModel), between two legs of a nested run: new
        node (i, j) keeps the State of old node (i + si, j + sj) where that lies `keep_margin` nodes inside the old box and takes the
        parent's prolonged State elsewhere; the particles are remade with step `dt` (picles_nest_relocate; nesting.relocate_state is
        the definition).  The tables are nesting.prolong_tables(parent_grid, NEW child grid); (mesh_x0, mesh_y0): the new
        coordinates of node (0, 0), for a wind lattice this model holds.  Static winds are uploaded at the new nodes before the call"""
        ph = getattr(parent, "h", parent)
        for v, name in ((si, "si"), (sj, "sj"), (keep_margin, "keep_margin")):
            if not (isinstance(v, (int, np.integer)) and -2 ** 31 <= int(v) < 2 ** 31):
                raise ValueError(f"nest_relocate: {name} must be an integer of 32 bits, not {v!r}")
        a0, a1, fx, b0, b1, fy = self._prolong_tables("nest_relocate", ix0, ix1, wx, iy0, iy1, wy)
        self.gen += 1
        self._ck(self.lib.picles_nest_relocate(self.h, ph, int(si), int(sj), int(keep_margin), _p32(a0), _p32(a1), K.dptr(fx), _p32(b0), _p32(b1),
                                               K.dptr(fy), float(dt), float(mesh_x0), float(mesh_y0)), "picles_nest_relocate")

    # ---- two-way nesting (picles_nest_feedback_*: this nested model's State restricted onto ocean nodes of its parent, on the device) ----
    def nest_feedback_init(self, fb_nodes, src_nodes, index, weights):
        """fb_nodes (n_fb, 2): 0-based (i, j) of the parent's ocean nodes to feed; src_nodes (n_src, 2): distinct 0-based (i, j) of
        this model; index (n_fb, m) into src_nodes and weights (n_fb, m) >= 0, 0.0 marking padding
        (picles_amd/nesting.py: restriction_stencil).  The library makes the forcing set on the parent of this model's nest"""
        fb = np.asarray(fb_nodes, dtype=np.int64).reshape(-1, 2)
        sn = np.asarray(src_nodes, dtype=np.int64).reshape(-1, 2)
        ix, w = np.asarray(index, dtype=np.int64), np.asarray(weights, dtype=np.float64)
        if ix.ndim != 2 or ix.shape != w.shape or ix.shape[0] != fb.shape[0]:
            raise ValueError(f"nest_feedback_init: index and weights must both be ({fb.shape[0]}, m) arrays, got {ix.shape} and {w.shape}")
        fplanes, splanes, iplanes = (_int32_planes(a, "nest_feedback_init") for a in (fb, sn, ix))
        wplanes = np.ascontiguousarray(w.T)
        self._ck(self.lib.picles_nest_feedback_init(self.h, fplanes.shape[1], _p32(fplanes), splanes.shape[1], _p32(splanes), iplanes.shape[0],
                                                    _p32(iplanes), K.dptr(wplanes)), "picles_nest_feedback_init")

    def nest_feedback(self):
        """take one level at this model's clock into the parent's set; returns after enqueueing"""
        self._ck(self.lib.picles_nest_feedback(self.h), "picles_nest_feedback")

    def nest_feedback_info(self):
        """(n_fb, n_src, m, levels taken) of this model's feedback"""
        a, b, m, t = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        if self.lib.picles_nest_feedback_info(self.h, C.byref(a), C.byref(b), C.byref(m), C.byref(t)) != 0:
            raise K.PiclesError("picles_nest_feedback_info failed: nest_feedback_init first")
        return a.value, b.value, m.value, t.value

    def _feedback_goes(self):
        """this model's feedback, if it has one, is about to be released: the parent's set goes with it, and the parent's pending
        step is completed on the way"""
        p = getattr(self, "_nest_parent", None)
        if p is not None and self.lib.picles_nest_feedback_info(self.h, None, None, None, None) == 0:
            p.gen += 1

    def nest_feedback_free(self):
        self._feedback_goes()
        self._ck(self.lib.picles_nest_feedback_free(self.h), "picles_nest_feedback_free")

    # ---- exact restart (picles_checkpoint_*) ----
    def checkpoint_size(self) -> int:
        n = C.c_size_t()
        self._ck(self.lib.picles_checkpoint_size(self.h, C.byref(n)), "picles_checkpoint_size")
        return n.value

    def checkpoint_begin(self):
        """snapshot the model at the current step boundary; the copy to the host runs beside the steps enqueued next"""
        self._ck(self.lib.picles_checkpoint_begin(self.h), "picles_checkpoint_begin")

    def checkpoint_end(self) -> np.ndarray:
        """wait for the snapshot of checkpoint_begin: the blob (uint8 array)"""
        buf = np.empty(self.checkpoint_size(), dtype=np.uint8)
        self._ck(self.lib.picles_checkpoint_end(self.h, buf.ctypes.data, buf.size), "picles_checkpoint_end")
        return buf

    def checkpoint_load(self, blob):
        """load a blob written by a model of the same configuration; raises CheckpointError (its .code says why) and leaves the
        model unchanged on a refusal"""
        a = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob, dtype=np.uint8)
        # (State is replaced too: the model layer resets its lazy view after a load — checkpointing.load_checkpoint — as after a step)
        self.gen += 1
        rc = self.lib.picles_checkpoint_load(self.h, a.ctypes.data if a.size else None, a.size)
        if rc != 0:
            msg = self.lib.picles_last_error(self.h)
            raise K.CheckpointError(rc, f"picles_checkpoint_load failed (rc={rc}): {msg.decode() if msg else '?'}")

    def get_particles(self):
        z = np.empty(5 * self.N)
        on = np.empty(self.N, dtype=np.uint8)
        bnd = np.empty(self.N, dtype=np.uint8)
        st = np.empty(self.N, dtype=np.int32)
        self._ck(self.lib.picles_get_particles(self.h, K.dptr(z), on.ctypes.data_as(K.c_uint8_p),
                                               bnd.ctypes.data_as(K.c_uint8_p), st.ctypes.data_as(K.c_int32_p)),
                 "picles_get_particles")
        sh = (self.Nx, self.ny_loc)
        return (z.reshape(sh + (5,), order="F"), on.reshape(sh, order="F"),
                bnd.reshape(sh, order="F"), st.reshape(sh, order="F"))

    def set_particles(self, z, on):
        self.gen += 1
        z = _col(z, 5 * self.N)
        on = np.ascontiguousarray(np.asarray(on, dtype=np.uint8).reshape(-1, order="F"))
        self._ck(self.lib.picles_set_particles(self.h, K.dptr(z), on.ctypes.data_as(K.c_uint8_p)),
                 "picles_set_particles")

    def scatter_particles(self, ij, xy, charge):
        """generic push_to_grid! of a particle list (ij: (n,2) int, xy: (n,2), charge: (n,3))"""
        self.gen += 1
        self.state_gen += 1
        ij = np.ascontiguousarray(np.asarray(ij, dtype=np.int32).T)
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).T)
        ch = np.ascontiguousarray(np.asarray(charge, dtype=np.float64).T)
        n = ij.shape[1]
        self._ck(self.lib.picles_scatter_particles(self.h, n, ij.ctypes.data_as(K.c_int32_p), K.dptr(xy), K.dptr(ch)),
                 "picles_scatter_particles")

    def get_counters(self):
        c = K.PiclesCounters()
        self._ck(self.lib.picles_get_counters(self.h, C.byref(c)), "picles_get_counters")
        return c.as_dict()

    def get_pull_class_counts(self):
        """(class_waves, empty_waves): waves of the wave-per-row fused step whose pull followed the tile class map, and those among them
        whose neighbourhood held no record, since the seed / reset_counters"""
        out = (C.c_int64 * 2)()
        self._ck(self.lib.picles_get_pull_class_counts(self.h, out), "picles_get_pull_class_counts")
        return int(out[0]), int(out[1])

    def reset_counters(self):
        self._ck(self.lib.picles_reset_counters(self.h), "picles_reset_counters")

    def enable_timing(self, on=True):
        self._ck(self.lib.picles_enable_timing(self.h, int(on)), "picles_enable_timing")

    def get_timing_samples(self, kind=0):
        """per-launch device durations [ms] of the step/advance (0), scatter (1) or remesh (2) kernels"""
        n = self.lib.picles_get_timing_samples(self.h, kind, None, 0)
        if n < 0:
            self._ck(n, "picles_get_timing_samples")
        out = np.empty(max(n, 1))
        n = self.lib.picles_get_timing_samples(self.h, kind, K.dptr(out), n)
        return out[:max(n, 0)]

    def get_dispatch_order(self):
        """(busy, calm, order) filed by the latest whole-grid fused step for its successor, or None when no complete order exists"""
        n = self.lib.picles_get_dispatch_order(self.h, None, 0)
        if n < 0:
            self._ck(n, "picles_get_dispatch_order")
        if n == 0:
            return None
        out = np.empty(2 + n, dtype=np.int32)
        n2 = self.lib.picles_get_dispatch_order(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size)
        if n2 != n:
            return None
        return int(out[0]), int(out[1]), out[2:].copy()

    def get_timing(self):
        t = K.PiclesTiming()
        self._ck(self.lib.picles_get_timing(self.h, C.byref(t)), "picles_get_timing")
        return t.as_dict()
