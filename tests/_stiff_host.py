"""The HOST build of the stiff half of the default solver (tests/native/stiff_host.cpp, the oracle's flags) through ctypes.
Test infrastructure, never imported by picles_amd/."""
from __future__ import annotations

import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from _flux_numpy import ORACLE_FLAGS
from picles_amd import _capi as K

ROOT = Path(__file__).resolve().parent.parent
ROS_VARIANTS = {(True, True, False): 0, (True, False, False): 1, (True, False, True): 2, (False, False, False): 3}   # (FAST, STATIC, METRIC)

_lib = None
_tmp = None


def host_lib():
    """compiled once per process into a temporary directory"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="picles_stiff_host_")
        so = Path(_tmp.name) / "libstiff_host.so"
        subprocess.run(["g++", "-std=gnu++17", *ORACLE_FLAGS, str(ROOT / "tests" / "native" / "stiff_host.cpp"), "-o", str(so)], check=True)
        _lib = C.CDLL(str(so))
        P, O, D, I32, I64 = C.POINTER(K.PiclesPhys), C.POINTER(K.PiclesOde), K.c_double_p, C.c_int32, C.c_int64
        for name, res, args in (("stiff_rhs3", None, [P, I32, I32, I64] + [D] * 4),
                                ("stiff_jac_plain", None, [P, I32, I32, I64] + [D] * 7),
                                ("stiff_jvp", None, [P, I32, I32, I64] + [D] * 6),
                                ("stiff_ros23", I32, [P, O, I32, I64] + [D] * 12),
                                ("stiff_init_dt", None, [P, O, I32, I64] + [D] * 7),
                                ("stiff_init_dt_f0", None, [P, O, I64] + [D] * 6)):
            f = getattr(_lib, name)
            f.restype, f.argtypes = res, args
    return _lib


def _a(x, n, k=None):
    shape = (n,) if k is None else (n, k)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), shape))


def rhs3(phys, z3, uv, pc=None, fast=True):
    z3 = np.atleast_2d(np.asarray(z3, dtype=np.float64))
    n = len(z3)
    z3, uv, pcs, f = _a(z3, n, 3), _a(uv, n, 2), _a(0.0 if pc is None else pc, n), np.empty((n, 3))
    host_lib().stiff_rhs3(C.byref(phys), int(fast), int(pc is not None), n, K.dptr(z3), K.dptr(uv), K.dptr(pcs), K.dptr(f))
    return f


def jac_plain(phys, z3, uv, pc=None, duv=None):
    """(J [n, 3, 3], dT [n, 3], y [n]) of rhs3_jac_plain<METRIC = pc given, TV = duv given>"""
    z3 = np.atleast_2d(np.asarray(z3, dtype=np.float64))
    n = len(z3)
    z3, uv, pcs, d = _a(z3, n, 3), _a(uv, n, 2), _a(0.0 if pc is None else pc, n), _a(0.0 if duv is None else duv, n, 2)
    J, dT, y = np.empty((n, 9)), np.empty((n, 3)), np.empty(n)
    host_lib().stiff_jac_plain(C.byref(phys), int(pc is not None), int(duv is not None), n, K.dptr(z3), K.dptr(uv), K.dptr(pcs), K.dptr(d),
                               K.dptr(J), K.dptr(dT), K.dptr(y))
    return J.reshape(n, 3, 3), dT, y


def jvp(phys, z3, uv, pc=None, duv=None, fast=True):
    """(J [n, 3, 3], dT [n, 3]) of rhs3_jvp<FAST, METRIC = pc given, 4>"""
    z3 = np.atleast_2d(np.asarray(z3, dtype=np.float64))
    n = len(z3)
    z3, uv, pcs, d = _a(z3, n, 3), _a(uv, n, 2), _a(0.0 if pc is None else pc, n), _a(0.0 if duv is None else duv, n, 2)
    J, dT = np.empty((n, 9)), np.empty((n, 3))
    host_lib().stiff_jvp(C.byref(phys), int(fast), int(pc is not None), n, K.dptr(z3), K.dptr(uv), K.dptr(pcs), K.dptr(d), K.dptr(J), K.dptr(dT))
    return J.reshape(n, 3, 3), dT


def ros23(phys, ode, variant, z5, wind, win, t, h, ipx, ipy, pc=0.0):
    """ros23_try<FAST, STATIC, METRIC> (variant: the triple): un [n, 5], f2 [n, 3], EEst² [n], eig [n]"""
    z5 = np.atleast_2d(np.asarray(z5, dtype=np.float64))
    n = len(z5)
    a = [_a(z5, n, 5), _a(wind, n, 6), _a(win, n, 3)] + [_a(x, n) for x in (t, h, ipx, ipy, pc)]
    un, f2, ee2, eig = np.empty((n, 5)), np.empty((n, 3)), np.empty(n), np.empty(n)
    rc = host_lib().stiff_ros23(C.byref(phys), C.byref(ode), ROS_VARIANTS[tuple(variant)], n, *[K.dptr(x) for x in a],
                                K.dptr(un), K.dptr(f2), K.dptr(ee2), K.dptr(eig))
    assert rc == 0
    return un, f2, ee2, eig


def init_dt(phys, ode, static, z5, wind, win, t, ipx, ipy):
    z5 = np.atleast_2d(np.asarray(z5, dtype=np.float64))
    n = len(z5)
    a = [_a(z5, n, 5), _a(wind, n, 6), _a(win, n, 3)] + [_a(x, n) for x in (t, ipx, ipy)]
    dt = np.empty(n)
    host_lib().stiff_init_dt(C.byref(phys), C.byref(ode), int(static), n, *[K.dptr(x) for x in a], K.dptr(dt))
    return dt


def init_dt_f0(phys, ode, z5, uv, f0, ipx, ipy):
    """init_dt<true, true, false> with the tendency f0 [n, 5] given"""
    z5 = np.atleast_2d(np.asarray(z5, dtype=np.float64))
    n = len(z5)
    a = [_a(z5, n, 5), _a(uv, n, 2), _a(f0, n, 5), _a(ipx, n), _a(ipy, n)]
    dt = np.empty(n)
    host_lib().stiff_init_dt_f0(C.byref(phys), C.byref(ode), n, *[K.dptr(x) for x in a], K.dptr(dt))
    return dt


def order_ratios(phys, ode, z5, uv, h, ipx=0.0, ipy=0.0, substeps=400):
    """the order of one Rosenbrock23 attempt under a static wind, from the pair (h, h/2): the factors by which the local error of un
    (against the exact solution: classical RK4 in mpmath, `substeps` steps) and sqrt(EEst²) fall — 8 for a second-order method with a
    local error O(h³).  Returns ((reference's two factors), (the code's two factors), h ||J||_inf)"""
    import _stiff_mp as R
    wind, win = [uv[0], uv[1], 0.0, 0.0, 0.0, 0.0], (0.0, 0.0, 0.0)
    node = R.Node(R.MP, phys, wind, win, 0.0, ipx, ipy)
    err_ref, est_ref, err_code, est_code = [], [], [], []
    hJ = None
    for hh in (h, 0.5 * h):
        exact = R.rk4_exact(node, z5, 0.0, hh, substeps)
        a = R.ros23_attempt(node, z5, 0.0, hh, ode.abstol, ode.reltol)
        if hJ is None:
            hJ = float(hh * max(sum(abs(a["J"][r, c]) for c in range(5)) for r in range(5)))
        un, _, ee2, _ = ros23(phys, ode, (True, True, False), z5, wind, win, 0.0, hh, ipx, ipy)
        sc = a["scale"]
        norm = lambda v: float(max(abs(R.mpf(float(x)) - e) / s for x, e, s in zip(v, exact, sc)))
        err_ref.append(float(max(abs(x - e) / s for x, e, s in zip(a["un"], exact, sc))))
        est_ref.append(float(R.mp.sqrt(a["EE2"])))
        err_code.append(norm(un[0]))
        est_code.append(float(np.sqrt(ee2[0])))
    return (err_ref[0] / err_ref[1], est_ref[0] / est_ref[1]), (err_code[0] / err_code[1], est_code[0] / est_code[1]), hJ
