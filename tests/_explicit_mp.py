"""The independent reference of the explicit half of the default solver: one embedded Runge–Kutta attempt, the PI controller and the
composite's stiffness detector, written from formulas.  Test infrastructure, never imported by picles_amd/; it reads neither the
kernels' sources nor the oracle.

The right-hand side, the window wind and the three arithmetics (MP: mpmath at 60 digits, the reference values; FP: the same literal
formulas in Python floats, whose distance from MP is the yardstick of every tolerance; CS is not needed here: nothing is
differentiated) are those of tests/_stiff_mp.py.

  tableau           Dormand–Prince 5(4) from exact rationals (Dormand & Prince 1980; Hairer, Nørsett & Wanner II.5, with the error
                    weights e = b - b̂).  Tsitouras 5(4) has no rational form: its table is OrdinaryDiffEq's doubles as
                    tests/test_tableaux.TSIT5 holds them, and what holds THOSE values is the 17 + 8 order conditions of
                    tests/test_tableaux.py and the full-table equality of tests/test_explicit_reference.py (every compiled entry
                    against that table).
  explicit_attempt  the textbook embedded attempt on the five-vector: full Butcher sums, stage times t + c_i h,
                    err = h Σ e_i k_i, scale_i = abstol + max(|z_i|, |u_new,i|) reltol, EEst = sqrt(mean((err/scale)²)), and the
                    composite's estimate eigen_est = ‖k7 − k6‖ / ‖u_new − g6‖ (RMS over the five components on both sides)
  pi_accept, pi_reject   the PI controller as OrdinaryDiffEq states it: q = EEst^β1 / qold^β2, the accepted factor
                    clamp(γ/q, qmin, qmax) with qold ← max(EEst, 1e-4); the rejected factor max(qmin, γ / EEst^β1)
  is_stiff          |eigen_est · dt_next / 3.5068| > 0.9
  asw_step          the AutoSwitch counters: more than 10 successive positives switch to Rosenbrock23 and double dt, more than 3
                    successive negatives switch back and halve dt
"""
from __future__ import annotations

import math
from fractions import Fraction as Fr

from mpmath import mp, mpf

import _stiff_mp as R
from _stiff_mp import FP, MP, Node, fp64_noise, rk4_exact  # noqa: F401  (one namespace for the tests)

# ---- the controller's and the detector's constants: OrdinaryDiffEq's defaults, as rationals ----
BETA = {"dp5": (Fr(17, 100), Fr(1, 25)), "tsit5": (Fr(7, 50), Fr(2, 25))}          # (β1, β2): DP5 β2 = 4//100, β1 = 1//5 − 3β2/4
GAMMA, QMIN, QMAX = Fr(9, 10), Fr(1, 5), Fr(10)
QOLD_INIT = Fr(1, 10000)
STABILITY = Fr(35068, 10000)          # alg_stability_size(Tsit5())
STIFF_TOL = Fr(9, 10)
MAX_STIFF, MAX_NONSTIFF = 10, 3

_DP5 = dict(
    c=[Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)],
    A=[[], [Fr(1, 5)], [Fr(3, 40), Fr(9, 40)], [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
       [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
       [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)],
       [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)]],
    e=[Fr(-71, 57600), Fr(0), Fr(71, 16695), Fr(-71, 1920), Fr(17253, 339200), Fr(-22, 525), Fr(1, 40)])


def num(A, x):
    """a rational or a double as a number of arithmetic A (a rational is divided in A: correctly rounded in fp64)"""
    if isinstance(x, Fr):
        return A.num(x.numerator) / A.num(x.denominator)
    return A.num(float(x))


def tableau_exact(name):
    """{c, A, e} of "dp5" (Fractions) or "tsit5" (doubles)"""
    if name == "dp5":
        return _DP5
    from test_tableaux import TSIT5
    return TSIT5


def tableau(A, name):
    t = tableau_exact(name)
    return dict(c=[num(A, x) for x in t["c"]], A=[[num(A, x) for x in row] for row in t["A"]], e=[num(A, x) for x in t["e"]])


def explicit_attempt(node, tab, z, t, h, abstol, reltol):
    """one embedded attempt in node's arithmetic (MP or FP).  Returns a dict: un, k [7][5], g [7][5] (the stage states), err, scale,
    EEst, eig (the composite's estimate) and cond = Σ|e_i k_i| / |Σ e_i k_i| weighted as the mean square weighs it"""
    A = node.A
    z, t, h = [A.num(x) for x in z], A.num(t), A.num(h)
    n = 5
    k, g = [], []
    for i in range(7):
        gi = [z[j] + h * sum((tab["A"][i][s] * k[s][j] for s in range(i)), A.num(0)) for j in range(n)] if i else list(z)
        g.append(gi)
        k.append(node.f(gi, t + tab["c"][i] * h))
    un = g[6]
    err = [h * sum((tab["e"][i] * k[i][j] for i in range(7)), A.num(0)) for j in range(n)]
    sc = [abstol + max(abs(z[j]), abs(un[j])) * reltol for j in range(n)]
    EE2 = sum((err[j] / sc[j]) ** 2 for j in range(n)) / n
    EEst = A.sqrt(EE2)
    nu = A.sqrt(sum((k[6][j] - k[5][j]) ** 2 for j in range(n)) / n)
    nd = A.sqrt(sum((un[j] - g[5][j]) ** 2 for j in range(n)) / n)
    eig = nu / nd if nd != 0 else A.num(0)
    return dict(un=un, k=k, g=g, err=err, scale=sc, EEst=EEst, eig=eig)


def _log(A, x):
    return mp.log(x) if A is MP else math.log(x)


def pi_accept(A, solver, EEst, qold):
    """(factor, the new qold) of an accepted attempt"""
    b1, b2 = (num(A, x) for x in BETA[solver])
    q = EEst ** b1 / qold ** b2
    f = num(A, GAMMA) / q
    f = min(max(f, num(A, QMIN)), num(A, QMAX))
    return f, max(EEst, num(A, QOLD_INIT))


def pi_reject(A, solver, EEst):
    b1 = num(A, BETA[solver][0])
    return max(num(A, QMIN), num(A, GAMMA) / EEst ** b1)


def clamp_thresholds(solver, qold):
    """the values of EEst (60 digits) at which a branch or a clamp changes, for a carried qold: accept / reject, the floor of the new
    qold, the accepted factor meeting qmax, the rejected factor meeting qmin"""
    b1, b2 = (num(MP, x) for x in BETA[solver])
    at_qmax = (num(MP, GAMMA) / num(MP, QMAX) * mpf(qold) ** b2) ** (1 / b1)
    at_qmin = (num(MP, GAMMA) / num(MP, QMIN)) ** (1 / b1)
    return dict(one=mpf(1), floor=num(MP, QOLD_INIT), qmax=at_qmax, qmin=at_qmin)


def stiff_ratio(A, eig, dt_next):
    """|eigen_est · dt_next / 3.5068| / 0.9: the composite counts the attempt as stiff where this exceeds 1"""
    return abs(eig * dt_next / num(A, STABILITY)) / num(A, STIFF_TOL)


def asw_step(count, stiff, positive, dt):
    """one AutoSwitch test: (count, stiff, dt) afterwards.  The counter runs up over successive positives and down over successive
    negatives, restarting at ±1 when the sign turns"""
    count = (1 if count < 0 else count + 1) if positive else (-1 if count > 0 else count - 1)
    if not stiff and count > MAX_STIFF:
        return count, True, dt * 2
    if stiff and count < -MAX_NONSTIFF:
        return count, False, dt / 2
    return count, stiff, dt
