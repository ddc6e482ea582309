"""StateStore: the HDF5 file `run!(sim; store=true)` writes (reference: src/Simulations/storing.jl:36-62 `state_store`,
:83-104 `init_state_store!`, :109-119 `push_state_to_storage!`, :127-131 `reset_state_store!`, :172-180 `close_store!`).

File layout, as HDF5.jl produces it for the reference (Julia arrays are column-major, HDF5 datasets row-major: HDF5.jl
reverses the dimension order, so the Julia array `data[time, x, y, state]` is the HDF5 dataset of shape
`(state, y, x, time)` — which is how h5py, h5dump or xarray see a file written by the reference):

    /waves                      group, attribute "dims" = ["time", "x", "y", "state"]   (variable-length UTF-8 strings)
    /waves/data                 float64 (3, Ny, Nx, Nt)
    /waves/time, /waves/x, /waves/y        float64 coordinate vectors
    /waves/state, /waves/var_names         variable-length strings ["e", "m_x", "m_y"]

The host side of this row is plain file IO: the snapshots arrive from the library's device-side ring
(`picles_store_push` / `picles_store_pop`, asynchronous D2H) already in the column-major order `[i + Nx (j + Ny k)]`
the dataset wants, so one hyperslab write per snapshot and no transposition.  libhdf5 is bound with ctypes (there is no
h5py for this interpreter); where no libhdf5 can be found, `NpyStateStore` keeps the same logical layout in a `.npy`
memory map with a JSON side-car.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import json
import os
import warnings
from pathlib import Path

import numpy as np

VAR_NAMES = ["e", "m_x", "m_y"]

_hid = C.c_int64
_H5F_ACC_RDONLY, _H5F_ACC_TRUNC = 0, 2
_H5S_SELECT_SET = 0
_H5T_VARIABLE = C.c_size_t(-1).value
_H5T_CSET_UTF8 = 1
_lib = None


def _find_hdf5():
    cand = [os.environ.get("PICLES_HDF5_LIB"), ctypes.util.find_library("hdf5"), "libhdf5.so", "libhdf5_serial.so",
            "/opt/conda/lib/libhdf5.so"]
    errs = []
    for c in cand:
        if not c:
            continue
        try:
            return C.CDLL(c)
        except OSError as e:
            errs.append(f"{c}: {e}")
    raise OSError("no libhdf5 found (set PICLES_HDF5_LIB): " + "; ".join(errs))


def hdf5():
    """the bound library (loaded once); raises OSError when there is none"""
    global _lib
    if _lib is not None:
        return _lib
    L = _find_hdf5()
    sig = {
        "H5open": (C.c_int, []),
        "H5Fcreate": (_hid, [C.c_char_p, C.c_uint, _hid, _hid]),
        "H5Fopen": (_hid, [C.c_char_p, C.c_uint, _hid]),
        "H5Fflush": (C.c_int, [_hid, C.c_int]),
        "H5Fclose": (C.c_int, [_hid]),
        "H5Gcreate2": (_hid, [_hid, C.c_char_p, _hid, _hid, _hid]),
        "H5Gopen2": (_hid, [_hid, C.c_char_p, _hid]),
        "H5Gclose": (C.c_int, [_hid]),
        "H5Screate_simple": (_hid, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "H5Sselect_hyperslab": (C.c_int, [_hid, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
        "H5Sget_simple_extent_ndims": (C.c_int, [_hid]),
        "H5Sget_simple_extent_dims": (C.c_int, [_hid, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "H5Sclose": (C.c_int, [_hid]),
        "H5Dcreate2": (_hid, [_hid, C.c_char_p, _hid, _hid, _hid, _hid, _hid]),
        "H5Dopen2": (_hid, [_hid, C.c_char_p, _hid]),
        "H5Dget_space": (_hid, [_hid]),
        "H5Dwrite": (C.c_int, [_hid, _hid, _hid, _hid, _hid, C.c_void_p]),
        "H5Dread": (C.c_int, [_hid, _hid, _hid, _hid, _hid, C.c_void_p]),
        "H5Dvlen_reclaim": (C.c_int, [_hid, _hid, _hid, C.c_void_p]),
        "H5Dclose": (C.c_int, [_hid]),
        "H5Tcopy": (_hid, [_hid]),
        "H5Tset_size": (C.c_int, [_hid, C.c_size_t]),
        "H5Tset_cset": (C.c_int, [_hid, C.c_int]),
        "H5Tclose": (C.c_int, [_hid]),
        "H5Lexists": (C.c_int, [_hid, C.c_char_p, _hid]),
        "H5Acreate2": (_hid, [_hid, C.c_char_p, _hid, _hid, _hid, _hid]),
        "H5Aopen": (_hid, [_hid, C.c_char_p, _hid]),
        "H5Aget_space": (_hid, [_hid]),
        "H5Awrite": (C.c_int, [_hid, _hid, C.c_void_p]),
        "H5Aread": (C.c_int, [_hid, _hid, C.c_void_p]),
        "H5Aclose": (C.c_int, [_hid]),
        "H5Eset_auto2": (C.c_int, [_hid, C.c_void_p, C.c_void_p]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    if L.H5open() < 0:
        raise OSError("H5open failed")
    L.H5Eset_auto2(0, None, None)          # errors come back as negative ids / return codes, checked below; no stderr stack dumps
    L.NATIVE_DOUBLE = _hid.in_dll(L, "H5T_NATIVE_DOUBLE_g").value
    L.NATIVE_FLOAT = _hid.in_dll(L, "H5T_NATIVE_FLOAT_g").value
    L.C_S1 = _hid.in_dll(L, "H5T_C_S1_g").value
    _lib = L
    return L


def _ok(v, what):
    if v < 0:
        raise OSError(f"HDF5: {what} failed")
    return v


def _dims(shape):
    return (C.c_uint64 * len(shape))(*shape)


def _vlen_str_type(L):
    t = _ok(L.H5Tcopy(L.C_S1), "H5Tcopy")
    _ok(L.H5Tset_size(t, _H5T_VARIABLE), "H5Tset_size")
    _ok(L.H5Tset_cset(t, _H5T_CSET_UTF8), "H5Tset_cset")
    return t


class H5Sliced:
    """a dataset written one slice of its last axis at a time (H5File.sliced): one hyperslab write per slice"""

    def __init__(self, L, loc, name, dims, dtype):
        self.L, self.name, self.dims, self.dtype = L, name, tuple(dims), np.dtype(dtype)
        self.type = L.NATIVE_DOUBLE if self.dtype == np.float64 else L.NATIVE_FLOAT
        self.fspace = _ok(L.H5Screate_simple(len(dims), _dims(self.dims), None), "H5Screate_simple")
        self.data = _ok(L.H5Dcreate2(loc, name.encode(), self.type, self.fspace, 0, 0, 0), f"H5Dcreate2({name})")
        self.mspace = _ok(L.H5Screate_simple(len(dims), _dims(self.dims[:-1] + (1,)), None), "H5Screate_simple")

    def write(self, i, plane):
        """`plane`: a contiguous array of the dataset's element type, shaped like the dataset without its last axis"""
        L, nd = self.L, len(self.dims)
        _ok(L.H5Sselect_hyperslab(self.fspace, _H5S_SELECT_SET, _dims((0,) * (nd - 1) + (i,)), None, _dims(self.dims[:-1] + (1,)), None),
            "H5Sselect_hyperslab")
        _ok(L.H5Dwrite(self.data, self.type, self.mspace, self.fspace, 0, plane.ctypes.data), f"H5Dwrite({self.name})")

    def fill(self, value):
        full = np.full(self.dims, value, dtype=self.dtype)
        _ok(self.L.H5Dwrite(self.data, self.type, 0, 0, 0, full.ctypes.data), f"H5Dwrite({self.name})")

    def close(self):
        self.L.H5Sclose(self.mspace); self.L.H5Sclose(self.fspace); self.L.H5Dclose(self.data)


class H5File:
    """`<dir>/<name>.h5` with one group, as every product here writes its HDF5 form: the directory is made, a file of that name
    replaced (the reference's replace=true: rm(...; force=true)), the file and the group created.  Datasets and attributes go
    into the group (or into `loc`, another group of the file: add_winds_forcing).  OSError where no libhdf5 loads or a call fails."""

    def __init__(self, dir, name, group):
        L = self.L = hdf5()
        self.dir = Path(dir)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.path = self.dir / f"{name}.h5"
        if self.path.exists():
            self.path.unlink()
        self.file = _ok(L.H5Fcreate(str(self.path).encode(), _H5F_ACC_TRUNC, 0, 0), f"H5Fcreate({self.path})")
        self.group = _ok(L.H5Gcreate2(self.file, group.encode(), 0, 0, 0), f"H5Gcreate2({group})")
        self._sliced = []

    def sliced(self, name, dims, dtype=np.float64):
        """a float64 or float32 dataset of shape `dims`, to be written slice by slice of its last axis; closed with the file"""
        self._sliced.append(H5Sliced(self.L, self.group, name, dims, dtype))
        return self._sliced[-1]

    def f64(self, name, a, loc=None):
        L = self.L
        a = np.ascontiguousarray(a, dtype=np.float64)
        sp = _ok(L.H5Screate_simple(a.ndim, _dims(a.shape), None), "H5Screate_simple")
        d = _ok(L.H5Dcreate2(self.group if loc is None else loc, name.encode(), L.NATIVE_DOUBLE, sp, 0, 0, 0), f"H5Dcreate2({name})")
        _ok(L.H5Dwrite(d, L.NATIVE_DOUBLE, 0, 0, 0, a.ctypes.data), f"H5Dwrite({name})")
        L.H5Dclose(d); L.H5Sclose(sp)

    def strings(self, name, strings, attribute=False, loc=None):
        """a dataset, or an attribute of the group, of variable-length UTF-8 strings"""
        L, loc = self.L, (self.group if loc is None else loc)
        t = _vlen_str_type(L)
        sp = _ok(L.H5Screate_simple(1, _dims((len(strings),)), None), "H5Screate_simple")
        keep = [s.encode("utf-8") for s in strings]
        buf = (C.c_char_p * len(keep))(*keep)
        if attribute:
            a = _ok(L.H5Acreate2(loc, name.encode(), t, sp, 0, 0), f"H5Acreate2({name})")
            _ok(L.H5Awrite(a, t, buf), f"H5Awrite({name})")
            L.H5Aclose(a)
        else:
            d = _ok(L.H5Dcreate2(loc, name.encode(), t, sp, 0, 0, 0), f"H5Dcreate2({name})")
            _ok(L.H5Dwrite(d, t, 0, 0, 0, buf), f"H5Dwrite({name})")
            L.H5Dclose(d)
        L.H5Sclose(sp); L.H5Tclose(t)

    def flush(self):
        if self.file is not None:
            self.L.H5Fflush(self.file, 1)

    def close(self):
        """idempotent; an H5Fclose that fails is an OSError (the file may not be whole)"""
        if self.file is None:
            return
        for d in self._sliced:
            d.close()
        self.L.H5Gclose(self.group)
        _ok(self.L.H5Fclose(self.file), "H5Fclose")
        self.file = None


def check_format(format, product):
    if format not in ("auto", "hdf5", "npy"):
        raise ValueError(f"unknown {product} format {format!r}")


def choose_format(format, product, hdf5_form, npy_form, warn=None):
    """the one "auto" | "hdf5" | "npy" choice: `hdf5_form()` unless "npy" is asked for; its OSError (no libhdf5, a failing call)
    is re-raised for "hdf5" and answered with `npy_form()` — after the warning `warn`, if given — for "auto" """
    check_format(format, product)
    if format != "npy":
        try:
            return hdf5_form()
        except OSError:
            if format == "hdf5":
                raise
            if warn:
                warnings.warn(warn)
    return npy_form()


class StateStore:
    """state_store(path, coords; name="state", replace=true) (storing.jl:36-62) + push_state_to_storage! (:109-119)"""

    format = "hdf5"

    def __init__(self, path, time, x, y, name="state", state=VAR_NAMES):
        h = self.h5 = H5File(path, name, "waves")
        self.dir, self.path = h.dir, h.path
        self.shape = (len(time), len(x), len(y), len(state))     # the reference's (Julia-order) shape
        nt, nx, ny, ns = self.shape
        self.data = h.sliced("data", (ns, ny, nx, nt))
        h.strings("dims", ["time", "x", "y", "state"], attribute=True)
        h.f64("time", time)
        h.f64("x", x)
        h.f64("y", y)
        h.strings("state", list(state))
        h.strings("var_names", VAR_NAMES)
        self.iteration = 0

    def write(self, state, i=None):
        """`store["data"][ii, :, :, :] = State`: one time plane.  `state` is the (Nx, Ny, 3) view the host API hands out
        (Fortran order underneath, i.e. already (3, Ny, Nx) in the file's row-major terms)"""
        if self.h5.file is None:
            raise ValueError("StateStore is closed")
        ii = self.iteration if i is None else int(i)
        nt, nx, ny, ns = self.shape
        if not 0 <= ii < nt:
            raise IndexError(f"store iteration {ii} outside the {nt} time slots")
        a = np.asarray(state, dtype=np.float64)
        if a.shape != (nx, ny, ns):
            raise ValueError(f"state of shape {a.shape}, store expects {(nx, ny, ns)}")
        self.data.write(ii, np.ascontiguousarray(a.transpose(2, 1, 0)))          # a no-op for the column-major State
        if i is None:
            self.iteration += 1

    def reset(self, value=0.0):
        """reset_state_store!(sim; value) (storing.jl:127-131)"""
        self.data.fill(float(value))
        self.iteration = 0

    def add_winds_forcing(self, forcing, coords):
        """add_winds_forcing_to_store!(store, forcing, coords) (storing.jl:142-176): a root-level group `forcing` with one float64
        dataset per forcing field (`forcing` = {"u": array[time, x, y], "v": ...}; None entries are skipped), the attribute
        `dims` and the coordinate vectors (`coords` = {"time": ..., "x": ..., "y": ...}, in the fields' index order).  The
        reference creates the field datasets with `create_dataset` and never writes them (:155-157); here they are filled."""
        h, L = self.h5, self.h5.L
        g = _ok(L.H5Gcreate2(h.file, b"forcing", 0, 0, 0), "H5Gcreate2(forcing)")
        for name, f in forcing.items():
            if f is None:
                continue
            f = np.asarray(f, dtype=np.float64)
            h.f64(str(name), np.ascontiguousarray(f.transpose(*range(f.ndim - 1, -1, -1))), loc=g)
        h.strings("dims", [str(k) for k in coords], attribute=True, loc=g)
        for k, v in coords.items():
            h.f64(str(k), np.asarray(v, dtype=np.float64), loc=g)
        L.H5Gclose(g)

    def flush(self):
        self.h5.flush()

    def close(self):
        """close_store!(store) (storing.jl:172-180)"""
        self.h5.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_state_store(path):
    """read a StateStore file back (tests, post-processing): dict with `data` in the reference's index order
    [time, x, y, state], the coordinate vectors, `var_names`, `state` and the group's `dims` attribute"""
    out = read_h5_group(path, "waves", f64=("data", "time", "x", "y"), strings=("var_names", "state"), attrs=("dims",))
    out["data"] = out["data"].transpose(3, 2, 1, 0)       # file (state, y, x, time) -> [time, x, y, state]
    return out


def read_h5_group(path, group, f64=(), strings=(), attrs=(), optional_f64=()):
    """the named float64 datasets (arrays in the file's row-major shape), string datasets and string attributes of one group;
    optional_f64: float64 datasets that are read where the group has a link of that name (H5Lexists) and left out where it has none"""
    L = hdf5()
    f = _ok(L.H5Fopen(str(path).encode(), _H5F_ACC_RDONLY, 0), f"H5Fopen({path})")
    g = _ok(L.H5Gopen2(f, group.encode(), 0), f"H5Gopen2({group})")
    out = {}

    def shape_of(space):
        nd = L.H5Sget_simple_extent_ndims(space)
        d = (C.c_uint64 * nd)()
        L.H5Sget_simple_extent_dims(space, d, None)
        return tuple(int(v) for v in d)

    for name in tuple(f64) + tuple(n for n in optional_f64 if _ok(L.H5Lexists(g, n.encode(), 0), f"H5Lexists({n})") > 0):
        d = _ok(L.H5Dopen2(g, name.encode(), 0), f"H5Dopen2({name})")
        sp = L.H5Dget_space(d)
        a = np.empty(shape_of(sp), dtype=np.float64)
        _ok(L.H5Dread(d, L.NATIVE_DOUBLE, 0, 0, 0, a.ctypes.data), f"H5Dread({name})")
        L.H5Sclose(sp); L.H5Dclose(d)
        out[name] = a
    for name, attribute in [(n, False) for n in strings] + [(n, True) for n in attrs]:
        t = _vlen_str_type(L)
        h = _ok((L.H5Aopen(g, name.encode(), 0) if attribute else L.H5Dopen2(g, name.encode(), 0)), f"open({name})")
        sp = L.H5Aget_space(h) if attribute else L.H5Dget_space(h)
        n = shape_of(sp)[0]
        buf = (C.c_char_p * n)()
        _ok(L.H5Aread(h, t, buf) if attribute else L.H5Dread(h, t, 0, 0, 0, buf), f"read({name})")
        out[name] = [b.decode("utf-8") for b in buf]
        L.H5Dvlen_reclaim(t, sp, 0, buf)
        L.H5Sclose(sp)
        (L.H5Aclose if attribute else L.H5Dclose)(h)
        L.H5Tclose(t)
    L.H5Gclose(g); L.H5Fclose(f)
    return out


class NpyStateStore:
    """the same logical layout without libhdf5: `<name>.waves.data.npy` [time, x, y, state] + `<name>.json`"""

    format = "npy"

    def __init__(self, path, time, x, y, name="state", state=VAR_NAMES):
        self.dir = Path(path)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.shape = (len(time), len(x), len(y), len(state))
        self.path = self.dir / f"{name}.waves.data.npy"
        self.data = np.lib.format.open_memmap(self.path, mode="w+", dtype=np.float64, shape=self.shape)
        (self.dir / f"{name}.json").write_text(json.dumps(
            {"group": "waves", "dims": ["time", "x", "y", "state"], "var_names": VAR_NAMES, "state": list(state),
             "time": list(map(float, time)), "x": list(map(float, x)), "y": list(map(float, y))}))
        self.iteration = 0

    def write(self, state, i=None):
        ii = self.iteration if i is None else int(i)
        self.data[ii] = state
        if i is None:
            self.iteration += 1

    def reset(self, value=0.0):
        self.data[:] = value
        self.iteration = 0

    def flush(self):
        self.data.flush()

    def close(self):
        self.data.flush()


def make_state_store(path, time, x, y, name="state", format="auto"):
    """format: "hdf5" (the reference's file; OSError without a libhdf5), "npy", or "auto" = hdf5 where a libhdf5 loads"""
    return choose_format(format, "store", lambda: StateStore(path, time, x, y, name=name),
                         lambda: NpyStateStore(path, time, x, y, name=name),
                         warn="no libhdf5 found: the state store is written as .npy + .json (same layout); set PICLES_HDF5_LIB")
