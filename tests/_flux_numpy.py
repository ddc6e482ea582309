"""Checkers of the coupling fluxes (picles_flux_*, include/picles_hip.h "coupling fluxes").  Test infrastructure, never imported by
picles_amd/.  Three independent pieces:

  literal_nodes   the nine node values restated from the REFERENCE's formulas in their literal order with libm (NumPy) —
                  GetVariablesAtVertex (core_2D.jl:121-128), c_g_conversions_vector, α_func, αₚ, H_β, Δ_β, Ĩ_func, D̃_func_lne, S_cg
                  (particle_waves_v5.jl:212-335) and the first line of particle_system (:479-556) — independent of physics.h
  host_nodes      the HOST build of flux_node (tests/native/flux_host.cpp, compiled here with the oracle's flags): what the kernel
                  is held against bit for bit
  planes_of / partials_of / combine   the coarsening, the scale, the float32 rounding and the tile tree of the header's
                  definition, in NumPy, applied to per-node values
"""
from __future__ import annotations

import ctypes as C
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from picles_amd import _capi as K

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ("phi_in", "phi_dis", "phi_shift", "tq_in_x", "tq_in_y", "tq_dis_x", "tq_dis_y", "us_x", "us_y")
TILE = 256
NPART = 11
ORACLE_FLAGS = "-O2 -fPIC -shared -ffp-contract=off -fno-fast-math -mfma -fvisibility=hidden -w".split()      # oracle/Makefile's CFLAGS

_lib = None
_tmp = None


def host_lib():
    """the host build of flux_node, compiled once per process into a temporary directory"""
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="picles_flux_host_")
        so = Path(_tmp.name) / "libflux_host.so"
        subprocess.run(["g++", "-std=gnu++17", *ORACLE_FLAGS, str(ROOT / "tests" / "native" / "flux_host.cpp"), "-o", str(so)], check=True)
        _lib = C.CDLL(str(so))
        _lib.flux_host_nodes.restype = None
        _lib.flux_host_nodes.argtypes = [C.POINTER(K.PiclesPhys), K.c_double_p, C.c_int64] + [K.c_double_p] * 5 + [K.c_double_p, K.c_int32_p]
    return _lib


def host_nodes(phys, minimal_state, e, mx, my, u, v):
    """flux_node per node: (values [..., 9], status [...]) for arrays of any (common) shape"""
    shape = np.shape(e)
    a = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), shape).reshape(-1)) for x in (e, mx, my, u, v)]
    n = a[0].size
    out, st = np.empty(9 * n), np.empty(n, dtype=np.int32)
    ms = np.array([minimal_state[0], minimal_state[1]], dtype=np.float64)
    host_lib().flux_host_nodes(C.byref(phys), K.dptr(ms), n, *[K.dptr(x) for x in a], K.dptr(out), st.ctypes.data_as(K.c_int32_p))
    return out.reshape(shape + (9,)), st.reshape(shape)


def literal_nodes(phys, minimal_state, e, mx, my, u, v):
    """the reference's formulas in their literal order (libm through NumPy); the same return as host_nodes.  BAD nodes are judged on
    these values (status 2), so a status may differ from the host build's only where a value is at the edge of the fp64 range"""
    e, mx, my, u, v = [np.asarray(x, dtype=np.float64) for x in np.broadcast_arrays(e, mx, my, u, v)]
    g = 9.81
    r_g, C_alpha, C_e, q, gamma = phys.r_g, phys.C_alpha, phys.C_e, phys.q, phys.gamma
    p = (-1 - 10 * q) / 2                                                    # magic_fractions
    n = 2 * q / (p + 4 * q)
    e_T = np.sqrt(phys.c_e * phys.c_alpha ** (-p / q) / (gamma * phys.c_beta * phys.c_D) ** (1 / n))      # e_T_func
    with np.errstate(all="ignore"):
        active = np.isfinite(e) & np.isfinite(mx) & np.isfinite(my) & (e >= minimal_state[0]) & (mx * mx + my * my >= minimal_state[1])
        m_amp = np.sqrt(mx ** 2 + my ** 2)                                   # GetVariablesAtVertex
        cx = mx * e / (2 * m_amp ** 2)
        cy = my * e / (2 * m_amp ** 2)
        lne = np.log(e)
        cbar = np.sqrt(cx ** 2 + cy ** 2)                                    # speed
        u_speed = np.sqrt(u ** 2 + v ** 2)
        c_gp = np.abs(cbar) / r_g                                            # c_g_conversions_vector
        kp = g / (4.0 * np.maximum(c_gp ** 2, 1e-2))
        wp = g / (2.0 * np.maximum(np.abs(c_gp), 0.1))
        cgx, cgy = cx / r_g, cy / r_g
        a = u_speed / (2.0 * c_gp)                                           # α_func
        alpha = np.where(a > 500, 500.0, a)
        alpha_p = (u * cgx + v * cgy) / (2 * np.maximum(np.sqrt(cgx ** 2 + cgy ** 2), 1e-4) ** 2)      # αₚ
        H = 0.5 * (1.0 + np.tanh(p * (alpha_p - 0.85)))                      # H_β
        Delta = 1.0 - 1.25 * (1.0 / np.cosh(10.0 * (alpha_p - 0.85))) ** 2   # Δ_β
        zero = np.zeros_like(e)
        It = C_e * H * alpha ** 2 if phys.input else zero                    # Ĩ_func
        Dt = np.exp(n * lne) * (kp / e_T) ** (2 * n) if phys.dissipation else zero      # D̃_func_lne
        Scg = C_alpha * Delta * kp ** 4 * np.exp(2 * lne) if phys.peak_shift else zero   # S_cg
        dx, dy = cx / cbar, cy / cbar
        phi_in, phi_dis, phi_shift = e * wp * It, e * wp * Dt, e * (wp * r_g * Scg)
        vals = np.stack([phi_in, phi_dis, phi_shift, wp * phi_in * dx, wp * phi_in * dy, wp * phi_dis * dx, wp * phi_dis * dy,
                         2 * e * wp * kp * dx, 2 * e * wp * kp * dy], axis=-1)
        bad = active & ~np.isfinite(vals).all(axis=-1)
        good = active & ~bad
    return np.where(good[..., None], vals, 0.0), np.where(good, 1, np.where(bad, 2, 0)).astype(np.int32)


# ---- coarsening, scale, rounding, tile tree: the header's definition applied to per-node values ----
def coarse_shape(Nx, ny, cx, cy):
    return -(-Nx // cx), -(-ny // cy)


def cell_sums(vals, status, cx, cy):
    """per coarse cell: the nine sums over the ACTIVE nodes (status 1), n_active, n_bad — from +0.0, j outer, i inner — and the
    number of nodes the cell covers.  vals [Nx, ny, 9], status [Nx, ny]: the context's own rows"""
    Nx, ny = status.shape
    nxc, nyc = coarse_shape(Nx, ny, cx, cy)
    S = np.zeros((NPART, nxc, nyc))
    cover = np.zeros((nxc, nyc))
    for jj in range(cy):
        for ii in range(cx):
            st = status[ii::cx, jj::cy]
            a, b = st.shape
            if a == 0 or b == 0:
                continue
            on = st == 1
            for k in range(9):
                S[k, :a, :b] = np.where(on, S[k, :a, :b] + np.where(on, vals[ii::cx, jj::cy, k], 0.0), S[k, :a, :b])
            S[9, :a, :b] += on
            S[10, :a, :b] += st == 2
            cover[:a, :b] += 1.0
    return S, cover


def planes_of(vals, status, cx, cy, scale_phi=1.0, scale_tau=1.0, names=FIELDS):
    """float32 planes [len(names), Nxc, nyc] in the order of FIELDS: ((sum / n_cover) * scale) rounded to nearest even"""
    S, cover = cell_sums(vals, status, cx, cy)
    scale = [scale_phi] * 3 + [scale_tau] * 4 + [1.0] * 2
    return np.stack([((S[k] / cover) * scale[k]).astype(np.float32) for k, f in enumerate(FIELDS) if f in names])


def _tree(v):
    """v: [tiles, 256, nyc] -> [tiles, nyc]: halving tree inside each group of 64 lanes, then the four groups in ascending order"""
    t, _, nyc = v.shape
    v = v.reshape(t, 4, 64, nyc)
    s = 32
    while s >= 1:
        v = v[:, :, :s] + v[:, :, s:2 * s]
        s //= 2
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def partials_of(vals, status, cx, cy):
    """[n_partials, 11]: the nine unscaled sums, n_active, n_bad per tile of 256 coarse columns, index J tiles_per_row + T"""
    S, _ = cell_sums(vals, status, cx, cy)
    _, nxc, nyc = S.shape
    tpr = -(-nxc // TILE)
    cols = []
    for k in range(NPART):
        pad = np.zeros((tpr * TILE, nyc))
        pad[:nxc] = S[k]
        cols.append(_tree(pad.reshape(tpr, TILE, nyc)).T.reshape(-1))       # J outer, tile inner
    return np.stack(cols, axis=1)


def combine(partials_list):
    """the eleven totals: sequential over the partials in the order given (rank order, then (J, tile) ascending), from +0.0"""
    acc = [0.0] * NPART
    for p in partials_list:
        for row in np.asarray(p).reshape(-1, NPART):
            for k in range(NPART):
                acc[k] = acc[k] + float(row[k])
    return dict(zip(tuple("sum_" + f for f in FIELDS) + ("n_active", "n_bad"), acc))
