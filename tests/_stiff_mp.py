"""The independent reference of the stiff half of the default solver.  Test infrastructure, never imported by picles_amd/.

Everything here is written from formulas, in three arithmetics that share ONE statement of each formula:

  MP   mpmath at 60 digits                          the reference values
  FP   Python floats with libm                      the same literal formulas in fp64: their distance from MP is `fp64_noise`,
  CS   Python complex numbers with libm             the yardstick of every tolerance in tests/test_stiff_reference.py.  CS carries
                                                    a derivative in the imaginary part (complex step, h = 1e-200): the Jacobian of
                                                    the literal formulas in fp64 without a difference quotient

  rhs5           the reference's right-hand side in its literal order: particle_system with c_g_conversions_vector, α_func, αₚ, H_β,
                 Δ_β, Ĩ_func, D̃_func_lne, S_cg, S_dir, sin2_a_min_b (max / min guards, tanh, sech), the metric term c̄x·pc riding on
                 S_dir, and ẋ = ipx·c̄x, ẏ = ipy·c̄y.  Constants: mpf(float(...)) of the C struct the shim receives.
  wind_at        the node wind over the window, parabola and knot form (static: level 0)
  jac_mp         J (5 × 5) and ∂f/∂t by central differences, step 1e-22 at 60 digits (truncation below 1e-40)
  ros23_attempt  ONE Rosenbrock23 attempt as Shampine–Reichelt / OrdinaryDiffEq state it (d = 1/(2+√2), e32 = 6+√2 from mpmath)
  init_dt_ref    Hairer–Wanner's initial step as OrdinaryDiffEq states it (true log10 and sqrt; the exponent divides by the order of
                 the explicit pair, 5)
  rk4_exact      the exact solution over one step: classical RK4 in mpmath
"""
from __future__ import annotations

import cmath
import math

import numpy as np
from mpmath import mp, mpf

mp.dps = 60
G = 9.81
FD = mpf(10) ** -22
CSTEP = 1e-200


class _Arith:
    def __init__(self, name, num, sqrt, tanh, cosh, exp, log10, re):
        self.name, self.num, self.sqrt, self.tanh, self._cosh, self.exp, self.log10, self.re = name, num, sqrt, tanh, cosh, exp, log10, re

    def sech(self, x):
        try:
            return 1 / self._cosh(x)
        except OverflowError:          # libm's cosh beyond 710: sech is 0 to every digit of fp64
            return self.num(0.0)

    def max(self, a, b):
        return a if self.re(a) >= self.re(b) else b

    def abs(self, a):
        return a if self.re(a) >= 0 else -a


MP = _Arith("mp", mpf, mp.sqrt, mp.tanh, mp.cosh, mp.exp, mp.log10, lambda x: x)
FP = _Arith("fp64", float, math.sqrt, math.tanh, math.cosh, math.exp, math.log10, lambda x: x)
CS = _Arith("fp64 complex step", complex, cmath.sqrt, cmath.tanh, cmath.cosh, cmath.exp, cmath.log10, lambda x: x.real)


def consts(A, phys):
    """the physical constants of the C struct as numbers of arithmetic A; p, n, e_T as magic_fractions / e_T_func derive them"""
    f = lambda name: A.num(float(getattr(phys, name)))
    C = {k: f(k) for k in ("r_g", "C_alpha", "C_phi", "C_e", "gamma", "q", "c_beta", "c_D", "c_e", "c_alpha")}
    q = C["q"]
    C["p"] = (-1 - 10 * q) / 2
    C["n"] = 2 * q / (C["p"] + 4 * q)
    C["e_T"] = A.sqrt(C["c_e"] * C["c_alpha"] ** (-C["p"] / q) / (C["gamma"] * C["c_beta"] * C["c_D"]) ** (1 / C["n"]))
    C["g"] = A.num(G)
    for k in ("input", "dissipation", "peak_shift", "direction", "propagation"):
        C[k] = bool(getattr(phys, k))
    return C


def _speed(A, a, b):
    return A.sqrt(a ** 2 + b ** 2)


def alpha_p(A, C, cx, cy, u, v):
    cgx, cgy = cx / C["r_g"], cy / C["r_g"]
    return (u * cgx + v * cgy) / (2 * A.max(_speed(A, cgx, cgy), A.num(1e-4)) ** 2)


def rhs5(A, C, z, u, v, pc=0, ipx=0, ipy=0, parts=None):
    """particle_system(dz, z, params, t) with the wind (u, v) of the node at t: the five tendencies.  `parts`, a dict, receives the
    intermediate values the tests place their regimes with"""
    lne, cx, cy = z[0], z[1], z[2]
    r_g, g = C["r_g"], C["g"]
    cbar = _speed(A, cx, cy)
    u_speed = _speed(A, u, v)
    c_gp = A.abs(cbar) / r_g                                   # c_g_conversions_vector
    kp = g / (4 * A.max(c_gp ** 2, A.num(1e-2)))
    wp = g / (2 * A.max(A.abs(c_gp), A.num(0.1)))
    cgx, cgy = cx / r_g, cy / r_g
    a = u_speed / (2 * c_gp)                                   # α_func
    alpha = A.num(500.0) if A.re(a) > 500 else a
    ap = (u * cgx + v * cgy) / (2 * A.max(_speed(A, cgx, cgy), A.num(1e-4)) ** 2)      # αₚ
    H = 0.5 * (1 + A.tanh(C["p"] * (ap - 0.85)))               # H_β
    D = 1 - 1.25 * A.sech(10 * (ap - 0.85)) ** 2               # Δ_β
    zero = A.num(0.0)
    It = C["C_e"] * H * alpha ** 2 if C["input"] else zero
    Dt = A.exp(C["n"] * lne) * (kp / C["e_T"]) ** (2 * C["n"]) if C["dissipation"] else zero
    Scg = C["C_alpha"] * D * kp ** 4 * A.exp(2 * lne) if C["peak_shift"] else zero
    Sdir = zero
    if C["direction"]:
        su, sc = _speed(A, u, v), _speed(A, cgx, cgy)          # sin2_a_min_b(u, v, c_gp_x, c_gp_y)
        if A.re(su * sc) == 0:
            s2 = zero
        else:
            s2 = (2 / (su * sc) ** 2) * (u * v * (2 * cgy ** 2 - sc ** 2) - cgx * cgy * (2 * v ** 2 - su ** 2))
        a2 = su / (2 * sc)
        a2 = A.num(500.0) if A.re(a2) > 500 else a2
        Sdir = a2 ** 2 * C["C_phi"] * H * s2
    Ssph = cx * pc
    if parts is not None:
        parts.update(c_gp=c_gp, a=a, ap=ap, H=H, D=D, It=It, Dt=Dt, Scg=Scg, Sdir=Sdir, wp=wp, kp=kp, U=u_speed)
    out = [wp * r_g * Scg + wp * (It - Dt),
           -cx * wp * r_g * Scg + cy * Sdir + cy * Ssph,
           -cy * wp * r_g * Scg - cx * Sdir - cx * Ssph]
    if C["propagation"]:
        out += [ipx * cx, ipy * cy]
    else:
        out += [zero, zero]
    return out


def one_minus_H(C, z, u, v):
    """1 - H_β of the reference at 60 digits, in the complementary form (no cancellation where H_β saturates)"""
    ap = alpha_p(MP, C, z[1], z[2], u, v)
    return 1 / (1 + mp.exp(2 * C["p"] * (ap - 0.85)))


def wind_at(A, wind, win, t):
    """the node wind at time t: wind = (u0, v0, du, dv, bu, bv), win = (tw0, dtw, sk).  dtw <= 0: static, level 0.
    sk == 0: u(s) = u0 + s (du + (s - 1) bu);  0 < sk < 1: u(s) = u0 + s du + max(s - sk, 0) bu;  s = (t - tw0)/dtw"""
    u0, v0, du, dv, bu, bv = wind
    tw0, dtw, sk = win
    if not A.re(dtw) > 0:
        return u0, v0
    s = (t - tw0) / dtw
    if A.re(sk) > 0:
        sp = A.max(s - sk, A.num(0.0))
        return u0 + s * du + sp * bu, v0 + s * dv + sp * bv
    return u0 + s * (du + (s - 1) * bu), v0 + s * (dv + (s - 1) * bv)


class Node:
    """what one particle's ODE holds fixed: constants, window wind, metric coefficient, projection"""

    def __init__(self, A, phys, wind, win=(0.0, 0.0, 0.0), pc=0.0, ipx=0.0, ipy=0.0):
        self.A, self.C = A, consts(A, phys)
        self.wind, self.win = [A.num(float(x)) for x in wind], [A.num(float(x)) for x in win]
        self.pc, self.ipx, self.ipy = A.num(float(pc)), A.num(float(ipx)), A.num(float(ipy))

    def f(self, z, t, parts=None):
        u, v = wind_at(self.A, self.wind, self.win, t)
        return rhs5(self.A, self.C, z, u, v, self.pc, self.ipx, self.ipy, parts)


def jac_mp(node, z, t):
    """(J [5][5], dT [5]) of node.f at (z, t): central differences at 60 digits"""
    z, t = [mpf(x) for x in z], mpf(t)
    J = mp.zeros(5, 5)
    for c in range(5):
        zp, zm = list(z), list(z)
        zp[c] += FD
        zm[c] -= FD
        fp, fm = node.f(zp, t), node.f(zm, t)
        for r in range(5):
            J[r, c] = (fp[r] - fm[r]) / (2 * FD)
    fp, fm = node.f(z, t + FD), node.f(z, t - FD)
    return J, [(a - b) / (2 * FD) for a, b in zip(fp, fm)]


def jac_cs(phys, z, wind, win, t, pc=0.0, ipx=0.0, ipy=0.0):
    """the same in fp64 by the complex step: (J [5, 5], dT [5]) as float arrays"""
    node = Node(CS, phys, wind, win, pc, ipx, ipy)
    J = np.zeros((5, 5))
    for c in range(5):
        zc = [complex(float(x)) for x in z]
        zc[c] += 1j * CSTEP
        J[:, c] = [x.imag / CSTEP for x in node.f(zc, complex(float(t)))]
    dT = np.array([x.imag / CSTEP for x in node.f([complex(float(x)) for x in z], complex(float(t), CSTEP))])
    return J, dT


def _solve(A, W, b):
    if A is MP:
        return list(mp.lu_solve(W, mp.matrix(b)))
    return list(np.linalg.solve(np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)))


def ros23_attempt(node, z, t, h, abstol, reltol, J=None, dT=None):
    """one Rosenbrock23 attempt on the five-vector in node's arithmetic (MP, or FP with J and dT given).  Returns a dict: un, f2, EE2,
    k1, k2, k3, the error vector's terms, and cond = Σ|terms| / |sum| of k1 - 2 k2 + k3 weighted as the mean square weighs it"""
    A = node.A
    z, t, h = [A.num(x) for x in z], A.num(t), A.num(h)
    if J is None:
        J, dT = jac_mp(node, z, t)
    two = A.num(2)
    d = 1 / (two + A.sqrt(two))
    e32 = 6 + A.sqrt(two)
    n = 5
    W = [[(1 if r == c else 0) - h * d * A.num(J[r, c]) for c in range(n)] for r in range(n)]
    if A is MP:
        W = mp.matrix(W)
    dT = [A.num(x) for x in dT]
    f0 = node.f(z, t)
    k1 = _solve(A, W, [f0[i] + h * d * dT[i] for i in range(n)])
    f1 = node.f([z[i] + h / 2 * k1[i] for i in range(n)], t + h / 2)
    k2 = _solve(A, W, [f1[i] - k1[i] for i in range(n)])
    k2 = [k2[i] + k1[i] for i in range(n)]
    un = [z[i] + h * k2[i] for i in range(n)]
    f2 = node.f(un, t + h)
    k3 = _solve(A, W, [f2[i] - e32 * (k2[i] - f1[i]) - 2 * (k1[i] - f0[i]) + h * dT[i] for i in range(n)])
    absf = (lambda x: abs(x))
    sc = [abstol + max(absf(z[i]), absf(un[i])) * reltol for i in range(n)]
    err = [h / 6 * (k1[i] - 2 * k2[i] + k3[i]) / sc[i] for i in range(n)]
    mag = [h / 6 * (absf(k1[i]) + 2 * absf(k2[i]) + absf(k3[i])) / sc[i] for i in range(n)]
    EE2 = sum(e ** 2 for e in err) / n
    # d(EE2)/EE2 for a relative perturbation ε of each term: 2 Σ_i |err_i| mag_i ε / Σ_i err_i²
    cond = 2 * sum(absf(e) * m for e, m in zip(err, mag)) / (n * EE2) if EE2 != 0 else A.num(0)
    return dict(un=un, f2=f2, EE2=EE2, k1=k1, k2=k2, k3=k3, f0=f0, f1=f1, J=J, dT=dT, cond=cond, scale=sc)


def _rms(A, v):
    return A.sqrt(sum(x ** 2 for x in v) / len(v))


def init_dt_ref(node, z, t, abstol, reltol, dtmin, f0=None):
    """ode_determine_initdt in node's arithmetic (MP or FP): sk = abstol + |u0| reltol; d0 = ‖u0/sk‖, d1 = ‖f0/sk‖ (RMS);
    dt0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 d0/d1; u1 = u0 + dt0 f0; d2 = ‖(f(u1, t + dt0) - f0)/sk‖/dt0;
    dt1 = max(1e-6, 1e-3 dt0) if max(d1, d2) <= 1e-15 else 10^(-(2 + log10 max(d1, d2))/5); dt = max(dtmin, min(100 dt0, dt1)).
    Returns (dt, the branch taken, the intermediate values)"""
    A = node.A
    z, t = [A.num(x) for x in z], A.num(t)
    f0 = node.f(z, t) if f0 is None else [A.num(x) for x in f0]
    sk = [abstol + abs(x) * reltol for x in z]
    d0, d1 = _rms(A, [a / s for a, s in zip(z, sk)]), _rms(A, [a / s for a, s in zip(f0, sk)])
    small = d0 < 1e-5 or d1 < 1e-5
    dt0 = A.num(1e-6) if small else A.num(0.01) * d0 / d1
    u1 = [a + dt0 * b for a, b in zip(z, f0)]
    f1 = node.f(u1, t + dt0)
    d2 = _rms(A, [(a - b) / s for a, b, s in zip(f1, f0, sk)]) / dt0
    m = max(d1, d2)
    flat = m <= 1e-15
    dt1 = max(A.num(1e-6), dt0 * A.num(1e-3)) if flat else A.num(10) ** (-(2 + A.log10(m)) / 5)
    dt = min(100 * dt0, dt1)
    branch = ("small" if small else "plain") + ("/flat" if flat else "") + ("/dt0" if 100 * dt0 < dt1 else "/dt1")
    if dtmin > dt:
        dt, branch = A.num(dtmin), branch + "/dtmin"
    return dt, branch, dict(d0=d0, d1=d1, d2=d2, m=m, dt0=dt0, dt1=dt1)


def rk4_exact(node, z, t, h, substeps=400):
    """the solution of the five-vector ODE at t + h: classical RK4, `substeps` steps (error ∝ (h/substeps)⁴)"""
    z, t = [mpf(x) for x in z], mpf(t)
    dt = mpf(h) / substeps
    for _ in range(substeps):
        k1 = node.f(z, t)
        k2 = node.f([a + dt / 2 * b for a, b in zip(z, k1)], t + dt / 2)
        k3 = node.f([a + dt / 2 * b for a, b in zip(z, k2)], t + dt / 2)
        k4 = node.f([a + dt * b for a, b in zip(z, k3)], t + dt)
        z = [a + dt / 6 * (p + 2 * q + 2 * r + s) for a, p, q, r, s in zip(z, k1, k2, k3, k4)]
        t += dt
    return z


def fp64_noise(ref, fp, scale=None):
    """distance of the fp64 evaluation of the literal formulas from their 60-digit values, |fp - ref| / scale elementwise (scale
    defaults to |ref|; a zero reference with a zero fp64 value counts 0)"""
    ref = [mpf(x) for x in ref]
    scale = [abs(r) for r in ref] if scale is None else [mpf(s) for s in scale]
    out = []
    for r, f, s in zip(ref, fp, scale):
        dlt = abs(mpf(float(f)) - r)
        out.append(0.0 if dlt == 0 else float(dlt / s) if s != 0 else float("inf"))
    return np.array(out)
