"""The stiff half of the default solver against an independent 60-digit reference (no GPU).

The HOST build of physics.h's rhs3, rhs3_jac_plain, rhs3_jvp, ros23_try and init_dt (tests/native/stiff_host.cpp, the oracle's flags)
against tests/_stiff_mp.py: the reference's formulas in their literal order in mpmath at 60 digits, differentiated there, one textbook
Rosenbrock23 attempt and the textbook initial step.  What is pinned: the derivatives, the W-method, the initial step.  What is not:
OrdinaryDiffEq's controller and its AutoSwitch semantics.

TOLERANCES.  None is chosen: for each compared quantity and regime the bound is 16 x the largest distance of the reference's OWN literal
formulas, evaluated in fp64 (libm; derivatives by the complex step), from their 60-digit values over the same seeded sample
(_stiff_mp.fp64_noise) — the margin covers a different operation order of comparable conditioning.  The bound is computed from the
reference alone, in the run; RECORDED keeps what the development machine (glibc 2.39 libm, x86-64) measured, (noise, the code's error)
in the units of the comparison, and the run's noise may not leave [1/4, 4] x the recorded one (a yardstick that moved is a finding).
Two derived terms are added:
  * where H_β saturates (reference H_β > 1/2) the code's dH/dα_p = 2p H (1 - H) loses the bits of 1 - H by cancellation: relative
    2^-52 / (1 - H_ref) on the part of an entry that carries dH.  Conditioning of the form, not a wrong formula; physics.h keeps it
    (every bit is mirrored by the oracle), and it is harmless to a W-method, whose order does not depend on the Jacobian's accuracy;
  * init_dt routes the second-derivative term through pm_log_coarse (2e-9 absolute, tests/test_pmath.py), times 0.1 in the exponent.
"""
import functools
import math

import numpy as np
import pytest
from mpmath import mpf

import _stiff_host as S
import _stiff_mp as R
from helpers import make_model
from picles_amd import _capi as K, configs
from picles_amd.models import build_structs

MARGIN = 16.0
EPS52 = 2.0 ** -52
LOG_COARSE = 0.1 * 2e-9

# (largest fp64 noise of the literal formulas, largest error of the code): measured on the development machine, see above
RECORDED = {
    "rhs3 plain cartesian": (4.7e-11, 1.7e-13), "rhs3 plain metric": (4.7e-11, 6.5e-14), "rhs3 young cartesian": (4.2e-11, 6.2e-14),
    "rhs3 young metric": (4.2e-11, 6.2e-14), "rhs3 floored cartesian": (3.7e-12, 8.0e-15), "rhs3 floored metric": (3.7e-12, 9.2e-15),
    "rhs3 capped cartesian": (4.0e-11, 5.6e-15), "rhs3 capped metric": (4.0e-11, 5.6e-15), "rhs3 opposing cartesian": (1.1e-09, 9.0e-14),
    "rhs3 opposing metric": (3.1e-10, 9.0e-14), "rhs3 calm cartesian": (2.2e-15, 2.1e-15), "rhs3 calm metric": (3.8e-15, 2.4e-15),
    "J plain cartesian": (9.3e-12, 5.2e-15), "dT plain cartesian": (1.4e-02, 1.1e-14), "J plain metric": (9.3e-12, 2.1e-14),
    "dT plain metric": (1.4e-02, 1.1e-14), "J young cartesian": (6.4e-12, 2.1e-14), "dT young cartesian": (9.7e-12, 3.2e-14),
    "J young metric": (6.4e-12, 2.1e-14), "dT young metric": (9.7e-12, 3.2e-14), "J floored cartesian": (6.1e-11, 4.4e-15),
    "dT floored cartesian": (3.4e-01, 1.0e-08), "J floored metric": (6.1e-11, 4.4e-15), "dT floored metric": (3.4e-01, 1.0e-08),
    "J capped cartesian": (1.1e-12, 1.8e-14), "dT capped cartesian": (4.6e-03, 3.9e-10), "J capped metric": (1.1e-12, 1.8e-14),
    "dT capped metric": (4.6e-03, 3.9e-10), "J opposing cartesian": (1.3e-10, 1.1e-14), "dT opposing cartesian": (1.5e-10, 7.3e-15),
    "J opposing metric": (7.0e-11, 4.6e-15), "dT opposing metric": (1.5e-10, 7.3e-15), "J calm cartesian": (2.6e-15, 2.9e-15),
    "dT calm cartesian": (0.0e+00, 0.0e+00), "J calm metric": (2.6e-15, 2.4e-15), "dT calm metric": (0.0e+00, 0.0e+00),
    "rhs3 only input": (1.0e-15, 7.1e-16), "J only input": (1.4e-15, 1.1e-15), "dT only input": (8.1e-16, 1.4e-15),
    "rhs3 only dissipation": (2.2e-15, 1.8e-15), "J only dissipation": (2.8e-15, 2.1e-15), "dT only dissipation": (0.0e+00, 0.0e+00),
    "rhs3 only peak_shift": (9.6e-15, 2.3e-14), "J only peak_shift": (5.8e-15, 8.0e-15), "dT only peak_shift": (1.2e-09, 1.2e-09),
    "rhs3 only direction": (1.3e-14, 1.4e-14), "J only direction": (1.9e-14, 3.7e-15), "dT only direction": (1.2e-15, 1.8e-15),
    "ros23 fast/static un": (2.5e-12, 5.2e-12), "ros23 fast/static f2": (9.5e-14, 5.0e-14), "ros23 fast/static EEst2/cond": (1.0e-14, 5.4e-14),
    "ros23 fast/static eig": (3.3e-15, 9.6e-15), "ros23 fast/tvar un": (3.1e-12, 4.4e-12), "ros23 fast/tvar f2": (2.2e-13, 2.9e-13),
    "ros23 fast/tvar EEst2/cond": (7.8e-15, 1.4e-14), "ros23 fast/tvar eig": (1.1e-14, 2.1e-14), "ros23 fast/tvar/metric un": (2.1e-12, 9.1e-12),
    "ros23 fast/tvar/metric f2": (9.1e-14, 6.0e-14), "ros23 fast/tvar/metric EEst2/cond": (1.5e-14, 1.7e-14), "ros23 fast/tvar/metric eig": (8.5e-15, 1.3e-14),
    "ros23 general/tvar un": (6.5e-12, 1.4e-11), "ros23 general/tvar f2": (1.1e-11, 3.1e-12), "ros23 general/tvar EEst2/cond": (1.0e-14, 1.8e-14),
    "ros23 general/tvar eig": (1.2e-14, 8.7e-15),
    "ros23 general/tvar/no peak_shift un": (7.7e-13, 5.9e-13), "ros23 general/tvar/no peak_shift f2": (7.0e-14, 5.9e-14),
    "ros23 general/tvar/no peak_shift EEst2/cond": (1.5e-14, 1.7e-14), "ros23 general/tvar/no peak_shift eig": (8.5e-15, 5.4e-15), "init_dt static": (7.5e-15, 7.1e-11), "init_dt tvar": (6.3e-15, 7.1e-11),
}


@functools.lru_cache(maxsize=None)
def structs():
    cfg = configs.example_00_minimal(n=9, L=16e3)
    m = make_model(cfg, ("libm", 0))
    _, p, o, _ = build_structs(m.grid, m.ODEsystem, m.ODEsettings, m.ODEdefaults, m.minimal_state, m.periodic_boundary)
    return p, o


def phys_with(**kw):
    q = K.PiclesPhys.from_buffer_copy(structs()[0])
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def ode_with(**kw):
    q = K.PiclesOde.from_buffer_copy(structs()[1])
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def check(key, noise, err, extra=0.0):
    """print both figures, hold the run's yardstick against the recorded one, and the code's error against MARGIN x noise (+ extra, a
    derived allowance per element)"""
    noise, err = np.asarray(noise, dtype=np.float64), np.asarray(err, dtype=np.float64)
    per = noise.max(axis=0)                    # one yardstick per compared quantity (component, matrix entry): the largest over the sample
    noise_max, worst = float(per.max()), float(np.max(err))
    ratio = float(np.max((err - extra) / np.where(per > 0, per, np.inf))) if per.any() else 0.0
    print(f"{key}: fp64 noise of the literal formulas {noise_max:.2e}, the code's error {worst:.2e}, at most {max(ratio, 0.0):.2f} x its own yardstick")
    assert np.isfinite(per).all() and np.isfinite(err).all(), key
    if key in RECORDED:
        rec = RECORDED[key][0]
        assert rec / 4 <= noise_max <= rec * 4, (key, "the yardstick moved", noise_max, rec)
    assert (err <= MARGIN * per + extra).all(), (key, worst, noise_max)


# ---- regimes: each strictly inside one branch of every guard ----
REGIMES = ("plain", "young", "floored", "capped", "opposing", "calm")
ALL_REGIMES = REGIMES + ("aligned",)          # aligned: plain states under a wind within ±0.6 rad (the one-term tests)
N_STATES = {"plain": 300}


def regime_states(name, seed=20261021):
    """(z3 [n, 3], uv [n, 2], duv [n, 2], pc [n]) of the regime, seeded"""
    n = N_STATES.get(name, 200)
    rng = np.random.default_rng([seed, ALL_REGIMES.index(name)])
    r_g = structs()[0].r_g
    th = rng.uniform(-np.pi, np.pi, n)
    dth = np.where(rng.random(n) < 0.75, rng.uniform(-0.6, 0.6, n), rng.uniform(-np.pi, np.pi, n))
    L = rng.uniform(-18.0, 3.0, n)
    if name in ("plain", "calm", "aligned"):
        c, U = rng.uniform(0.2, 12.0, n), rng.uniform(0.05, 30.0, n)
        if name == "aligned":
            dth = rng.uniform(-0.6, 0.6, n)
        if name == "calm":
            U = np.zeros(n)
    elif name == "young":
        c, U, L = rng.uniform(0.086, 0.4, n), 10.0 ** rng.uniform(-6.0, 1.0, n), rng.uniform(-20.0, -8.0, n)
    elif name == "floored":
        c = rng.uniform(0.01, 0.08, n)
        U, L = rng.uniform(0.05, np.minimum(30.0, 0.9 * 990.0 * c / r_g)), rng.uniform(-20.0, -8.0, n)
    elif name == "capped":
        c, U, L = rng.uniform(0.002, 0.008, n), rng.uniform(12.0, 30.0, n), rng.uniform(-20.0, -8.0, n)
    elif name == "opposing":
        c = rng.uniform(0.3, 2.0, n)
        dth = np.pi + rng.uniform(-0.6, 0.6, n)
        U = rng.uniform(1.1, 2.0, n) * 10.1 * (c / r_g) / np.abs(np.cos(dth))
    else:
        raise KeyError(name)
    z3 = np.stack([L, c * np.cos(th), c * np.sin(th)], axis=1)
    uv = np.stack([U * np.cos(th + dth), U * np.sin(th + dth)], axis=1)
    duv = rng.uniform(-1e-3, 1e-3, (n, 2)) * (0.0 if name == "calm" else 1.0)
    pc = rng.uniform(1e-7, 5e-7, n) * rng.choice([-1.0, 1.0], n)
    return z3, uv, duv, pc


def assert_inside(name, parts):
    """regime membership on the reference side, at least 1 % from every kink"""
    c_gp, a, U = parts["c_gp"], parts["a"], parts["U"]
    assert c_gp > 1.01e-4                                               # the floor of αₚ's denominator is never met
    if name in ("plain", "young", "opposing", "calm", "aligned"):
        assert c_gp > 0.101 and c_gp ** 2 > 1.01e-2 and a < 495
    elif name == "floored":
        assert c_gp < 0.099 and c_gp ** 2 < 0.99e-2 and a < 495
    elif name == "capped":
        assert c_gp < 0.099 and a > 505
    if name == "opposing":
        assert parts["ap"] < -5
    assert (U == 0) == (name == "calm")


class Ref:
    """the reference of one regime under one physics: computed once, shared by the tests, never changed"""

    def __init__(self, name, metric, switches=()):
        z3, uv, duv, pc = regime_states(name)
        self.name, self.z3, self.uv, self.duv = name, z3, uv, duv
        self.pc = pc if metric else None
        self.phys = phys_with(**{k: int(k in switches) for k in ("input", "dissipation", "peak_shift", "direction")}) if switches else structs()[0]
        n = len(z3)
        self.f, self.J, self.dT, self.dT_scale = [None] * n, [None] * n, [None] * n, [None] * n
        self.f_noise, self.J_noise, self.dT_noise = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3))
        self.JH, self.dTH = np.zeros((n, 3, 3)), np.zeros((n, 3))
        win = (0.0, 1.0, 0.0)                   # u(t) = u + t du: the slope per second at t = 0 is (du, dv)
        for k in range(n):
            wind = [uv[k, 0], uv[k, 1], duv[k, 0], duv[k, 1], 0.0, 0.0]
            pck = pc[k] if metric else 0.0
            node = R.Node(R.MP, self.phys, wind, win, pck)
            z5 = [*z3[k], 0.0, 0.0]
            parts = {}
            self.f[k] = node.f([mpf(x) for x in z5], mpf(0), parts)[:3]
            assert_inside(name, parts)
            J, dT = R.jac_mp(node, z5, 0.0)
            self.J[k] = [[J[r, c] for c in range(3)] for r in range(3)]
            self.dT[k] = dT[:3]
            ff = R.Node(R.FP, self.phys, wind, win, pck).f([float(x) for x in z5], 0.0)
            self.f_noise[k] = R.fp64_noise(self.f[k], ff[:3])
            Jc, dTc = R.jac_cs(self.phys, z5, wind, win, 0.0, pck)
            for r in range(3):
                self.J_noise[k, r] = R.fp64_noise(self.J[k][r], Jc[r, :3], [self.row_scale(k, r)] * 3)
            # ∂f/∂t = f_u du + f_v dv: each component is held relative to |f_u du| + |f_v dv|, the row of terms it sums (below
            # 1e-30 |f| the 60-digit difference quotient resolves nothing: an H_β that is 0 to 60 digits leaves an exact 0)
            zm5 = [mpf(x) for x in z5]
            d_uv = []
            for du_, dv_ in ((R.FD, 0), (0, R.FD)):
                fp_ = R.rhs5(R.MP, node.C, zm5, mpf(uv[k, 0]) + du_, mpf(uv[k, 1]) + dv_, node.pc)
                fm_ = R.rhs5(R.MP, node.C, zm5, mpf(uv[k, 0]) - du_, mpf(uv[k, 1]) - dv_, node.pc)
                d_uv.append([(a - b) / (2 * R.FD) for a, b in zip(fp_, fm_)])
            self.dT_scale[k] = [max(abs(d_uv[0][r] * mpf(duv[k, 0])) + abs(d_uv[1][r] * mpf(duv[k, 1])), mpf(1e-30) * abs(self.f[k][r]))
                                for r in range(3)]
            self.dT_noise[k] = R.fp64_noise(self.dT[k], dTc[:3], self.dT_scale[k])
            # the part of each entry that carries dH = 2p H (1 - H) dα_p, and 1 - H_β in its complementary form
            if parts["H"] > 0.5:
                C = node.C
                omH = R.one_minus_H(C, z5, mpf(uv[k, 0]), mpf(uv[k, 1]))
                # relative 2^-52 / (1 - H_ref) of the dH part; at most all of it (1 - H below 2^-52: the code's H rounds to 1, dH to 0)
                gH = 2 * C["p"] * parts["H"] * omH * min(mpf(EPS52) / omH, mpf(1))
                f_H = [parts["wp"] * parts["It"] / parts["H"], mpf(z5[2]) * parts["Sdir"] / parts["H"], -mpf(z5[1]) * parts["Sdir"] / parts["H"]]
                dap = []
                for c in (1, 2):
                    zp, zm = [mpf(x) for x in z5], [mpf(x) for x in z5]
                    zp[c] += R.FD
                    zm[c] -= R.FD
                    dap.append((R.alpha_p(R.MP, C, zp[1], zp[2], mpf(uv[k, 0]), mpf(uv[k, 1]))
                                - R.alpha_p(R.MP, C, zm[1], zm[2], mpf(uv[k, 0]), mpf(uv[k, 1]))) / (2 * R.FD))
                ap_t = (R.alpha_p(R.MP, C, mpf(z5[1]), mpf(z5[2]), mpf(uv[k, 0]) + R.FD * mpf(duv[k, 0]), mpf(uv[k, 1]) + R.FD * mpf(duv[k, 1]))
                        - R.alpha_p(R.MP, C, mpf(z5[1]), mpf(z5[2]), mpf(uv[k, 0]) - R.FD * mpf(duv[k, 0]), mpf(uv[k, 1]) - R.FD * mpf(duv[k, 1]))) / (2 * R.FD)
                for r in range(3):
                    for c in (1, 2) if self.row_scale(k, r) != 0 else ():
                        self.JH[k, r, c] = float(abs(f_H[r] * gH * dap[c - 1]) / self.row_scale(k, r))
                    if self.dT_scale[k][r] != 0:
                        self.dTH[k, r] = float(abs(f_H[r] * gH * ap_t) / self.dT_scale[k][r])

    def row_scale(self, k, r):
        return max(abs(x) for x in self.J[k][r])

    def f_err(self, f):
        return np.array([R.fp64_noise(self.f[k], f[k]) for k in range(len(f))])

    def J_err(self, J):
        return np.array([[R.fp64_noise(self.J[k][r], J[k, r], [self.row_scale(k, r)] * 3) for r in range(3)] for k in range(len(J))])

    def dT_err(self, dT):
        return np.array([R.fp64_noise(self.dT[k], dT[k], self.dT_scale[k]) for k in range(len(dT))])

    def H_term(self):
        """the derived allowance of the saturating H_β per Jacobian entry and per dT component"""
        return self.JH, self.dTH


@functools.lru_cache(maxsize=None)
def ref(name, metric, switches=()):
    return Ref(name, metric, switches)


# ---- (a) the right-hand side ----
@pytest.mark.parametrize("metric", [False, True], ids=["cartesian", "metric"])
@pytest.mark.parametrize("name", REGIMES)
def test_rhs3_against_the_reference(name, metric):
    r = ref(name, metric)
    for fast in (True, False):
        f = S.rhs3(r.phys, r.z3, r.uv, r.pc, fast=fast)
        check(f"rhs3 {name} {'metric' if metric else 'cartesian'}", r.f_noise, r.f_err(f))


# ---- (b) the Jacobians ----
@pytest.mark.parametrize("metric", [False, True], ids=["cartesian", "metric"])
@pytest.mark.parametrize("name", ["plain", "young"])
def test_structured_jacobian_against_the_reference(name, metric):
    r = ref(name, metric)
    JH, dTH = r.H_term()
    tag = f"{name} {'metric' if metric else 'cartesian'}"
    for tv in (False, True):
        J, dT, y = S.jac_plain(r.phys, r.z3, r.uv, r.pc, r.duv if tv else None)
        assert (y <= 10.0 / r.phys.r_g).all()                   # the code, too, takes these states as plain
        check(f"J {tag}", r.J_noise, r.J_err(J), JH)
        if tv:
            check(f"dT {tag}", r.dT_noise, r.dT_err(dT), dTH)
        else:
            assert (dT == 0.0).all()
    # the structured and the forward-mode Jacobian against each other, at the same tolerance
    Jv, dTv = S.jvp(r.phys, r.z3, r.uv, r.pc, r.duv, fast=True)
    scale = np.abs(np.array(r.J, dtype=np.float64)).max(axis=2, keepdims=True)
    assert (np.abs(J - Jv) / scale <= MARGIN * r.J_noise.max(axis=0) + JH).all()
    assert (np.abs(dT - dTv) <= (MARGIN * r.dT_noise.max(axis=0) + dTH) * np.array(r.dT_scale, dtype=np.float64)).all()


@pytest.mark.parametrize("metric", [False, True], ids=["cartesian", "metric"])
@pytest.mark.parametrize("name", REGIMES)
def test_forward_mode_jacobian_against_the_reference(name, metric):
    r = ref(name, metric)
    JH, dTH = r.H_term()
    tag = f"{name} {'metric' if metric else 'cartesian'}"
    for fast in (True, False):
        J, dT = S.jvp(r.phys, r.z3, r.uv, r.pc, r.duv, fast=fast)
        check(f"J {tag}", r.J_noise, r.J_err(J), JH)
        check(f"dT {tag}", r.dT_noise, r.dT_err(dT), dTH)


@pytest.mark.parametrize("term", ["input", "dissipation", "peak_shift", "direction"])
def test_general_path_one_term_at_a_time(term):
    """rhs3<false> and rhs3_jvp<false> with exactly one source term switched on: each term shown alone"""
    r = ref("aligned", True, (term,))
    JH, dTH = r.H_term()
    f = S.rhs3(r.phys, r.z3, r.uv, r.pc, fast=False)
    J, dT = S.jvp(r.phys, r.z3, r.uv, r.pc, r.duv, fast=False)
    check(f"rhs3 only {term}", r.f_noise, r.f_err(f))
    check(f"J only {term}", r.J_noise, r.J_err(J), JH)
    check(f"dT only {term}", r.dT_noise, r.dT_err(dT), dTH)
    assert (np.abs(f) > 0).any() and (np.abs(J) > 0).any()          # the term is at work


# ---- (c) one Rosenbrock23 attempt ----
TW0, DTW = 1000.0, 600.0


def attempt_cases(variant, n=100, seed=20261022):
    """states (three quarters plain, one quarter floored: the forward-mode lanes of the specialised kernels), x, y != 0, steps of
    0.1 ... 30 s, and the winds: static, the parabola window, the knot window with its knot inside (t, t + h)"""
    fast, static, metric = variant
    rng = np.random.default_rng([seed, S.ROS_VARIANTS[variant]])
    r_g = structs()[0].r_g
    floored = rng.random(n) < 0.25
    # seas whose growth over 30 s stays of order one (a young sea under a gale, d ln e/dt of 10 /s, is no state for a 30 s attempt):
    # plain |c̄| from 1 m/s, floored ones under a wind of α = U / 2 c_gp up to 2
    c = np.where(floored, rng.uniform(0.01, 0.08, n), rng.uniform(1.0, 12.0, n))
    U = np.where(floored, rng.uniform(0.02, 4.0 * c / r_g), rng.uniform(1.0, 25.0, n))
    th = rng.uniform(-np.pi, np.pi, n)
    dth = np.where(rng.random(n) < 0.75, rng.uniform(-0.6, 0.6, n), rng.uniform(-np.pi, np.pi, n))
    L = np.where(floored, rng.uniform(-20.0, -8.0, n), rng.uniform(-18.0, 3.0, n))
    z5 = np.stack([L, c * np.cos(th), c * np.sin(th), rng.uniform(0.05, 0.95, n) * rng.choice([-1.0, 1.0], n),
                   rng.uniform(0.05, 0.95, n) * rng.choice([-1.0, 1.0], n)], axis=1)
    h = np.exp(rng.uniform(np.log(0.1), np.log(30.0), n))
    t = TW0 + rng.uniform(0.0, DTW - 31.0, n)
    ipx, ipy = rng.uniform(2e-4, 2e-3, n) * rng.choice([-1.0, 1.0], n), rng.uniform(2e-4, 2e-3, n)
    pc = rng.uniform(2e-7, 2e-6, n) * rng.choice([-1.0, 1.0], n) if metric else np.zeros(n)
    form = np.zeros(n, dtype=int) if static else rng.choice([0, 1, 1, 2, 2], n)          # 0 static, 1 parabola, 2 knot
    wind, win = np.zeros((n, 6)), np.zeros((n, 3))
    ut, vt = U * np.cos(th + dth), U * np.sin(th + dth)                                    # the wind at t
    for k in range(n):
        if form[k] == 0:
            wind[k, :2] = ut[k], vt[k]
            continue
        s = (t[k] - TW0) / DTW
        d, b = rng.uniform(-3.0, 3.0, 2), rng.uniform(-4.0, 4.0, 2)
        if form[k] == 1:
            win[k] = TW0, DTW, 0.0
            lvl0 = np.array([ut[k], vt[k]]) - s * (d + (s - 1.0) * b)
        else:
            sk = (t[k] + rng.uniform(0.1, 0.9) * h[k] - TW0) / DTW
            win[k] = TW0, DTW, sk
            lvl0 = np.array([ut[k], vt[k]]) - s * d                                        # t lies before the knot
        wind[k] = lvl0[0], lvl0[1], d[0], d[1], b[0], b[1]
    return dict(z5=z5, wind=wind, win=win, t=t, h=h, ipx=ipx, ipy=ipy, pc=pc, floored=floored, form=form)


@functools.lru_cache(maxsize=None)
def attempt_refs(variant, off=None):
    """the 60-digit attempt of every case, and the same attempt in fp64 (the 60-digit Jacobian rounded, numpy's LU): the yardstick.
    `off`: a source term switched off — not the specialised physics any more: every Jacobian is the forward-mode one"""
    cs = attempt_cases(variant)
    o = structs()[1]
    phys = phys_with(**{off: 0}) if off else structs()[0]
    out = []
    for k in range(len(cs["h"])):
        a = (cs["wind"][k], cs["win"][k], cs["pc"][k], cs["ipx"][k], cs["ipy"][k])
        node = R.Node(R.MP, phys, *a)
        parts = {}
        node.f([mpf(x) for x in cs["z5"][k]], mpf(cs["t"][k]), parts)
        assert_inside("floored" if cs["floored"][k] else "plain", parts)
        if cs["form"][k] == 2:
            assert cs["t"][k] < TW0 + cs["win"][k, 2] * DTW < cs["t"][k] + cs["h"][k]
        ref = R.ros23_attempt(node, cs["z5"][k], cs["t"][k], cs["h"][k], o.abstol, o.reltol)
        J, dT = ref["J"], ref["dT"]
        Jf = np.array([[float(J[r, c]) for c in range(5)] for r in range(5)])
        fp = R.ros23_attempt(R.Node(R.FP, phys, *a), cs["z5"][k], cs["t"][k], cs["h"][k], o.abstol, o.reltol, Jf, [float(x) for x in dT])
        Jc, _ = R.jac_cs(phys, cs["z5"][k], cs["wind"][k], cs["win"][k], cs["t"][k], cs["pc"][k], cs["ipx"][k], cs["ipy"][k])
        norm = lambda M: max(max(sum(abs(M[r, c]) for c in range(5)) for r in range(3)), abs(cs["ipx"][k]), abs(cs["ipy"][k]))
        ref["eig"], fp["eig"] = norm(J), norm(Jc)
        ref["hJ"] = float(cs["h"][k] * max(sum(abs(J[r, c]) for c in range(5)) for r in range(5)))
        out.append((ref, fp))
    return cs, out, phys


@pytest.mark.parametrize("variant,off", [(v, None) for v in S.ROS_VARIANTS] + [((False, False, False), "peak_shift")],
                         ids=["fast-static", "fast-tvar", "fast-tvar-metric", "general-tvar", "general-tvar-no-peak-shift"])
def test_ros23_try_against_the_reference_attempt(variant, off):
    cs, refs, p = attempt_refs(variant, off)
    o = structs()[1]
    un, f2, ee2, eig = S.ros23(p, o, variant, cs["z5"], cs["wind"], cs["win"], cs["t"], cs["h"], cs["ipx"], cs["ipy"], cs["pc"])
    hJ = np.array([r["hJ"] for r, _ in refs])
    print(f"h ||J||_inf from {hJ.min():.1e} to {hJ.max():.1e}, {int((hJ > 1).sum())} of {len(hJ)} above 1; forms", np.bincount(cs["form"], minlength=3))
    assert hJ.max() > 10 and (hJ > 1).mean() > 0.1 and cs["floored"].sum() >= 10
    assert variant[1] or (np.bincount(cs["form"], minlength=3) >= 10).all()
    tag = "ros23 " + ("fast" if variant[0] else "general") + ("/static" if variant[1] else "/tvar") + ("/metric" if variant[2] else "") + (f"/no {off}" if off else "")
    n = len(refs)
    check(tag + " un", [R.fp64_noise(r["un"], f["un"], r["scale"]) for r, f in refs], [R.fp64_noise(refs[k][0]["un"], un[k], refs[k][0]["scale"]) for k in range(n)])
    check(tag + " f2", [R.fp64_noise(r["f2"][:3], f["f2"][:3]) for r, f in refs], [R.fp64_noise(refs[k][0]["f2"][:3], f2[k]) for k in range(n)])
    # EEst²: relative, in units of the cancellation of k1 - 2 k2 + k3 (Σ|terms| / |sum|, from the reference)
    cond = np.array([float(r["cond"]) for r, _ in refs])
    check(tag + " EEst2/cond", [R.fp64_noise([r["EE2"]], [f["EE2"]]) / cond[k] for k, (r, f) in enumerate(refs)],
          [R.fp64_noise([refs[k][0]["EE2"]], [ee2[k]]) / cond[k] for k in range(n)])
    check(tag + " eig", [R.fp64_noise([r["eig"]], [f["eig"]]) for r, f in refs], [R.fp64_noise([refs[k][0]["eig"]], [eig[k]]) for k in range(n)])


# ---- (d) the order of the attempt ----
@functools.lru_cache(maxsize=None)
def box_structs():
    """the physics of the benchmark box (C_φ = 0.04: the direction term is the stiff one), solver 2"""
    from picles_amd import fetch_relations as FR
    cfg = configs.bench06_box(n=8, U10=8.0, V10=-11.0)
    sets = cfg.model["ODEsets"]
    sets.solver = 2
    g, p, o, _ = build_structs(cfg.model["grid"], cfg.model["ODEsys"], sets, None, FR.MinimalState(2, 2, sets.timestep), True)
    return p, o, 1.0 / g.dx, 1.0 / g.dy


@pytest.mark.parametrize("h,hJ_about", [(1.0, 0.03), (0.5, 0.015)])
def test_rosenbrock23_local_error_and_estimate_fall_by_eight(h, hJ_about):
    """a method of order 2 with a local error O(h³): from h to h/2 the local error of un — against the exact solution, RK4 in mpmath
    with 400 substeps — and sqrt(EEst²) fall by 8, in the small-h||J|| range (at h||J|| >= 0.5 the factors are 4 ... 6).  The band
    (7, 9) is asserted on the reference attempt first, then on the code"""
    p, o, ipx, ipy = box_structs()
    ref_f, code_f, hJ = S.order_ratios(p, o, [0.5, 6.0, -2.5, 0.0, 0.0], (8.0, -11.0), h, ipx, ipy)
    print(f"h = {h}: h ||J||_inf = {hJ:.4f}; local error and estimate fall by {ref_f[0]:.3f}, {ref_f[1]:.3f} (reference), "
          f"{code_f[0]:.3f}, {code_f[1]:.3f} (code)")
    assert 0.8 * hJ_about < hJ < 1.25 * hJ_about
    assert all(7.0 < x < 9.0 for x in ref_f), ref_f
    assert all(7.0 < x < 9.0 for x in code_f), code_f


# ---- (e) the initial step ----
@pytest.mark.parametrize("static", [True, False], ids=["static", "tvar"])
def test_init_dt_against_the_textbook_formula(static):
    """init_dt<true, STATIC, false> on freshly remeshed particles (x = y = 0: the scale abstol) and on particles under way, against
    ode_determine_initdt with true log10 and sqrt.  The code's second-derivative term passes through pm_log_coarse: LOG_COARSE in
    the exponent on top of the yardstick"""
    p, o = structs()[0], ode_with(dtmin=1e-12)          # the floor is held in test_init_dt_early_exits
    n = 200
    rng = np.random.default_rng([20261023, int(static)])
    z3, uv, _, _ = regime_states("plain")
    z5 = np.concatenate([z3[:n], np.where(rng.random((n, 1)) < 0.5, 0.0, rng.uniform(-0.9, 0.9, (n, 2)))], axis=1)
    ipx, ipy = rng.uniform(2e-4, 2e-3, n) * rng.choice([-1.0, 1.0], n), rng.uniform(2e-4, 2e-3, n)
    wind, win, t = np.zeros((n, 6)), np.zeros((n, 3)), np.zeros(n)
    wind[:, :2] = uv[:n]
    if not static:          # parabola windows; the particle starts anywhere in the first half
        wind[:, 2:4], wind[:, 4:6] = rng.uniform(-3.0, 3.0, (n, 2)), rng.uniform(-4.0, 4.0, (n, 2))
        win[:] = TW0, DTW, 0.0
        t = TW0 + rng.uniform(0.0, 0.5 * DTW, n)
    dt = S.init_dt(p, o, static, z5, wind, win, t, ipx, ipy)
    noise, err, branches = [], [], set()
    for k in range(n):
        a = (wind[k], win[k], 0.0, ipx[k], ipy[k])
        ref, br, parts = R.init_dt_ref(R.Node(R.MP, p, *a), z5[k], t[k], o.abstol, o.reltol, o.dtmin)
        fp, brf, _ = R.init_dt_ref(R.Node(R.FP, p, *a), z5[k], t[k], o.abstol, o.reltol, o.dtmin)
        assert br == brf and "small" not in br and "flat" not in br and "dtmin" not in br          # strictly inside the main branch
        assert not 0.99 < 100 * parts["dt0"] / parts["dt1"] < 1.01 and parts["d0"] > 1.01e-5 and parts["d1"] > 1.01e-5 and parts["m"] > 1.01e-15
        branches.add(br)
        noise.append(R.fp64_noise([ref], [fp]))
        err.append(R.fp64_noise([ref], [dt[k]]))
    assert branches == {"plain/dt0", "plain/dt1"}, branches          # both 100 dt0 and dt1 are met as the smaller
    assert (z5[:, 3] == 0).sum() > 50 and (z5[:, 3] != 0).sum() > 50          # both forms of the scale
    check(f"init_dt {'static' if static else 'tvar'}", noise, err, extra=math.expm1(LOG_COARSE))


def test_init_dt_early_exits():
    p, o = structs()
    tiny = ode_with(dtmin=1e-12)
    z, uv, ip = np.array([[0.5, 6.0, -2.5, 0.0, 0.0]]), np.array([[8.0, -11.0]]), (1e-3, -5e-4)
    f0 = np.concatenate([S.rhs3(p, z[:, :3], uv), z[:, 1:3] * ip], axis=1)
    node = R.Node(R.MP, p, [8.0, -11.0, 0, 0, 0, 0], (0.0, 0.0, 0.0), 0.0, *ip)

    def both(ode, zz, ff, uvv=uv, nd=node, ipp=ip):
        ref, br, _ = R.init_dt_ref(nd, zz[0], 0.0, ode.abstol, ode.reltol, ode.dtmin, ff[0])
        return float(S.init_dt_f0(p, ode, zz, uvv, ff, *ipp)[0]), float(ref), br

    # the ordinary case through this entry point agrees with the one that evaluates f0 itself
    got, ref, br = both(o, z, f0)
    assert got == S.init_dt(p, o, True, z, [8.0, -11.0, 0, 0, 0, 0], (0.0, 0.0, 0.0), 0.0, *ip)[0] and abs(got / ref - 1) < 1e-9
    # S0 below 1e-10 (d0 < 1e-5): a state of 1e-10 in every component; S1 below 1e-10: a vanishing tendency.  dt0 = 1e-6
    for zz, ff in ((np.array([[1e-10, 1e-10, -1e-10, 0.0, 0.0]]), f0), (z, f0 * 1e-12)):
        got, ref, br = both(tiny, zz, ff)
        assert br.startswith("small") and got <= 100 * 1e-6 * (1 + 1e-12)
        assert abs(got / ref - 1) <= 1e-9, (got, ref, br)
    # the flat second-derivative estimate: no wind, no energy to speak of, no propagation, f0 = 0 — max(d1, d2) <= 1e-15,
    # dt1 = max(1e-6, 1e-3 dt0)
    calm = R.Node(R.MP, p, [0.0] * 6, (0.0, 0.0, 0.0), 0.0, 0.0, 0.0)
    zz = np.array([[-200.0, 6.0, -2.5, 0.0, 0.0]])
    got, ref, br = both(tiny, zz, np.zeros((1, 5)), np.zeros((1, 2)), calm, (0.0, 0.0))
    assert br == "small/flat/dt1" and got == ref == 1e-6
    # a NaN tendency: the code answers 1e-6 (and the dtmin floor above it)
    bad = f0.copy()
    bad[0, 1] = np.nan
    assert S.init_dt_f0(p, tiny, z, uv, bad, *ip)[0] == 1e-6
    assert S.init_dt_f0(p, o, z, uv, bad, *ip)[0] == o.dtmin
    # the dtmin floor
    floor = ode_with(dtmin=50.0)
    got, ref, br = both(floor, z, f0)
    assert br.endswith("/dtmin") and got == ref == 50.0
