"""The explicit half of the default solver against an independent 60-digit reference (no GPU).

The HOST build of physics.h's integrate_dp5 (tests/native/explicit_host.cpp, the oracle's flags) — the seven-stage DP5 / Tsit5 attempt
with its x,y sums carried on the stage c̄, the one-reciprocal EEst², the log-space PI controller, the accept / reject rule, the Tsit5
eigenvalue estimate and the AutoSwitch counters — against tests/_explicit_mp.py: the textbook embedded attempt with full Butcher sums in
mpmath at 60 digits, OrdinaryDiffEq's PI controller and the composite's stiffness test, from rationals.

ONE ATTEMPT is observed without touching the integrator: with maxiters = 1 and dtn = h > 0 exactly one attempt runs and the loop stops
at the iteration test in front of a second one; z is u_new on accept, lq = max(½ ln EEst², ln 1e-4), dtn / h the controller's factor,
acc / rej the branch.  With maxiters = 2 the AutoSwitch test in front of the second attempt shows in asw.

TOLERANCES follow tests/test_stiff_reference.py.  None is chosen: the bound is 16 x the largest distance of the reference's OWN literal
formulas, evaluated in fp64, from their 60-digit values over the same seeded sample, computed in the run from the reference alone;
RECORDED keeps (noise, the code's error) as the development machine measured them, and the run's noise may not leave [1/4, 4] x the
recorded one.  One derived term: the controller reads ln EEst² through pm_log_coarse (2e-9 absolute, tests/test_pmath.py), which
enters lq with the factor ½ and a controller factor with ½ β1, relative.
"""
import functools
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import _explicit_host as H
import _explicit_mp as X
import _stiff_host as S
from test_stiff_reference import REGIMES, assert_inside, box_structs, ode_with, regime_states, structs

MARGIN = 16.0
LOG_COARSE = 2e-9
# the correctly rounded ln 1e-4 — of the DOUBLE 1e-4, the value the controller's qold holds (qoldinit = 1//10^4 converted to Float64).  The
# distinction decides the last bit: ln(1/10000) = -9.21034037197618273607… lies within 2e-17 of the midpoint of two doubles and rounds
# to …184, the logarithm of the double 1e-4 = 1.0000000000000000479e-4, -9.21034037197618268815…, rounds to …182
LN_FLOOR = float(mp.log(mpf(1e-4)))
TW0, DTW = 1000.0, 600.0
N_PER_REGIME = 6
# the order test's step and what the REFERENCE attempt gives there at 60 digits, recorded: the factors by which the local error and EEst
# fall from h to h/2.  The band is ± 2 % around them.  (DP5's 47 is not yet 64: its principal error term is small by design, and the term
# of the next order still shows at this step; a step short enough to hide it puts the local error at the rounding of the state)
ORDER_H = 2.0
ORDER_REF = {"dp5": (47.057, 30.251), "tsit5": (68.293, 31.427)}
ORDER_BAND = {k: (tuple(0.98 * x for x in v), tuple(1.02 * x for x in v)) for k, v in ORDER_REF.items()}
BANDS = ("clamped at qmax", "accepted", "rejected", "clamped at qmin")
SETS = [("static", False), ("parabola", False), ("knot", False), ("parabola", True), ("knot", True)]          # (window, metric)
# the instantiations (FAST, STATIC, METRIC) that run each set
VARIANTS_OF = {("static", False): [(True, True, False), (False, False, False)], ("parabola", False): [(True, False, False), (False, False, False)],
               ("knot", False): [(True, False, False), (False, False, False)], ("parabola", True): [(True, False, True)],
               ("knot", True): [(True, False, True)]}

# (largest fp64 noise of the literal formulas, largest error of the code): measured on the development machine (glibc 2.39, x86-64).
# u_new in units of scale_i; ln EEst and lq absolute; factors relative.  The code's 3.4e-10 on ln EEst and 5e-11 on the factors are
# pm_log_coarse's (inside the derived ½ · 2e-9 and ½ β1 · 2e-9).  The detector's rows hold (noise of the ratio, the δ of the bracket).
RECORDED = {
    "attempt dp5 static un": (3.2e-13, 5.2e-13),
    "attempt dp5 static ln EEst": (1.1e-11, 3.4e-10),
    "attempt dp5 static factor": (1.8e-12, 5.7e-11),
    "attempt dp5 parabola un": (6.9e-13, 4.2e-13),
    "attempt dp5 parabola ln EEst": (1.3e-11, 3.4e-10),
    "attempt dp5 parabola factor": (2.1e-12, 5.7e-11),
    "attempt dp5 knot un": (3.2e-13, 4.2e-13),
    "attempt dp5 knot ln EEst": (7.5e-12, 3.4e-10),
    "attempt dp5 knot factor": (1.3e-12, 5.7e-11),
    "attempt dp5 parabola metric un": (2.4e-13, 4.4e-13),
    "attempt dp5 parabola metric ln EEst": (1.1e-11, 3.4e-10),
    "attempt dp5 parabola metric factor": (1.9e-12, 5.7e-11),
    "attempt dp5 knot metric un": (4.2e-13, 3.9e-13),
    "attempt dp5 knot metric ln EEst": (3.6e-11, 3.4e-10),
    "attempt dp5 knot metric factor": (6.2e-12, 5.7e-11),
    "attempt tsit5 static un": (2.6e-12, 1.7e-12),
    "attempt tsit5 static ln EEst": (4.9e-11, 3.5e-10),
    "attempt tsit5 static factor": (1.0e-11, 4.9e-11),
    "attempt tsit5 parabola un": (1.7e-10, 9.2e-13),
    "attempt tsit5 parabola ln EEst": (1.2e-08, 3.5e-10),
    "attempt tsit5 parabola factor": (1.7e-09, 4.9e-11),
    "attempt tsit5 knot un": (9.7e-13, 3.3e-12),
    "attempt tsit5 knot ln EEst": (4.8e-11, 3.5e-10),
    "attempt tsit5 knot factor": (7.1e-12, 4.9e-11),
    "attempt tsit5 parabola metric un": (2.6e-12, 7.3e-13),
    "attempt tsit5 parabola metric ln EEst": (5.6e-11, 3.5e-10),
    "attempt tsit5 parabola metric factor": (7.8e-12, 4.9e-11),
    "attempt tsit5 knot metric un": (1.8e-12, 3.0e-12),
    "attempt tsit5 knot metric ln EEst": (1.1e-10, 3.5e-10),
    "attempt tsit5 knot metric factor": (1.5e-11, 4.9e-11),
    "controller dp5 factor": (1.8e-12, 5.7e-11),
    "controller dp5 lq": (1.1e-11, 3.4e-10),
    "controller tsit5 factor": (1.0e-11, 4.9e-11),
    "controller tsit5 lq": (4.9e-11, 3.5e-10),
    "detector static": (2.2e-11, 5.0e-10),
    "detector parabola": (3.9e-11, 7.6e-10),
    "detector parabola metric": (3.3e-12, 1.9e-10),
    "detector knot": (4.3e-11, 8.2e-10),
}


def check(key, noise, err, extra=0.0):
    """print both figures, hold the run's yardstick against the recorded one, and the code's error against MARGIN x noise (+ extra)"""
    noise, err = np.atleast_2d(np.asarray(noise, dtype=np.float64).T).T, np.atleast_2d(np.asarray(err, dtype=np.float64).T).T
    per = noise.max(axis=0)
    noise_max, worst = float(per.max()), float(np.max(err))
    ratio = float(np.max((err - extra) / np.where(per > 0, per, np.inf))) if per.any() else 0.0
    print(f"{key}: fp64 noise of the literal formulas {noise_max:.2e}, the code's error {worst:.2e}, at most {max(ratio, 0.0):.2f} x its own yardstick")
    assert np.isfinite(per).all() and np.isfinite(err).all(), key
    if key in RECORDED:
        rec = RECORDED[key][0]
        assert rec / 4 <= noise_max <= rec * 4, (key, "the yardstick moved", noise_max, rec)
    assert (err <= MARGIN * per + extra).all(), (key, worst, noise_max)


TIGHT, LOOSE = (1e-8, 1e-8), (1e-2, 1e-2)
# With the settings' tolerances (reltol 1e-3) EEst saturates near 1/reltol, below the (γ/qmin)^(1/β1) = 6.9e3 (DP5), 4.6e4 (Tsit5) at which
# the rejected factor meets qmin: the fourth band is reached under abstol = reltol = 1e-8, which are inputs like any other.  At the other
# end the accepted factor meets qmax at EEst = (γ/qmax · qold^β2)^(1/β1) <= 3e-8 (Tsit5): under the settings' tolerances an error of
# 1e-10 scale is the rounding of the state itself and EEst measures noise; under abstol = reltol = 1e-2 it is four decades above it.


def ode(tol=None):
    return ode_with(dtmin=1e-12, force_dtmin=0) if tol is None else ode_with(dtmin=1e-12, force_dtmin=0, abstol=tol[0], reltol=tol[1])


# ---- the cases: a state, a window built around the step, a carried lq, and a step that puts the reference's EEst in a band ----
class Case:
    def __init__(self, regime, z5, uv, pc, ip, window, rng, lq):
        self.regime, self.z5, self.uv, self.pc, self.ipx, self.ipy, self.window, self.lq = regime, z5, uv, pc, ip[0], ip[1], window, lq
        U = float(np.hypot(*uv))
        s = min(1.0, 0.1 * U)          # under the speed floor a breeze is a gale: the window's changes scale with the wind
        self.d, self.b = rng.uniform(-3.0, 3.0, 2) * s, rng.uniform(-4.0, 4.0, 2) * s
        self.t = TW0 + rng.uniform(0.0, 100.0)
        self.frac = rng.uniform(0.15, 0.85)          # the knot lies at t + frac h
        self.h, self.tol = None, None

    def tols(self):
        o = ode(self.tol)
        return o.abstol, o.reltol

    def wind_win(self, h):
        """(wind [6], win [3]) whose wind at t is the regime's (u, v)"""
        u = np.asarray(self.uv, dtype=np.float64)
        if self.window == "static":
            return [u[0], u[1], 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        if self.window == "parabola":
            s = (self.t - TW0) / DTW
            l0 = u - s * (self.d + (s - 1.0) * self.b)
            return [l0[0], l0[1], *self.d, *self.b], [TW0, DTW, 0.0]
        L = max(DTW, 4.0 * h)          # the knot form: a window of at least four steps that begins L/10 before t
        tw0 = self.t - 0.1 * L
        s, sk = (self.t - tw0) / L, (self.t + self.frac * h - tw0) / L
        l0 = u - s * self.d            # t lies before the knot
        return [l0[0], l0[1], *self.d, *self.b], [tw0, L, sk]

    def node(self, A, h):
        wind, win = self.wind_win(h)
        return X.Node(A, structs()[0], wind, win, self.pc, self.ipx, self.ipy)


def eest_fp(case, tab, h):
    try:
        e = float(X.explicit_attempt(case.node(X.FP, h), tab, case.z5, case.t, h, *case.tols())["EEst"])
    except (OverflowError, ZeroDivisionError, ValueError):
        return math.inf
    return e if e == e else math.inf


def find_step(case, tab, lo, hi, target):
    """a step whose fp64 EEst lies in [lo, hi], approached from below (from 1e-9 s: the first hit lies where the attempt still
    resolves the solution): EEst ∝ h⁵ towards the target, bisection in ln h once the band is bracketed"""
    h, below, above = 1e-9, None, None
    for _ in range(200):
        e = eest_fp(case, tab, h)
        if lo <= e <= hi:
            return h
        if e < lo:
            below = h
        else:
            above = h
        if below is not None and above is not None:
            h = math.sqrt(below * above)
        elif math.isfinite(e) and e > 0:
            h *= min(max((target / e) ** 0.2, 0.2), 5.0)
        else:
            h *= 0.5 if e > 0 else 2.0
    raise AssertionError(("no step puts EEst in the band", case.regime, case.window, lo, hi))


@functools.lru_cache(maxsize=None)
def attempt_set(solver, window, metric):
    """the cases of one (tableau, window, metric) and, per case, the 60-digit attempt with the controller's answer and the same in
    fp64: computed once, shared by the tests, never changed"""
    tabs = {A.name: X.tableau(A, solver) for A in (X.MP, X.FP)}
    rng = np.random.default_rng([20261024, H.SOLVERS[solver], SETS.index((window, metric))])
    cases = []
    for name in REGIMES:
        z3, uv, _, pc = regime_states(name)
        taken = 0
        for k in range(len(z3)):
            # the regime's states in their seeded order, leaving out the seas that do not move within a day: where a step of 1e5 s
            # still sits in a band the tendencies cancel to rounding, h · (the rounding of k_i) is the whole error estimate and EEst
            # measures noise at 60 digits' distance from its fp64 value
            if taken == N_PER_REGIME:
                break
            four = []
            for band in range(4):
                xy = rng.uniform(0.05, 0.95, 2) * rng.choice([-1.0, 1.0], 2)
                ip = rng.uniform(2e-4, 2e-3, 2) * [rng.choice([-1.0, 1.0]), 1.0]
                # the carried ln qold: near 1 where the accepted factor is to clamp at qmax (its threshold on EEst grows with qold), else
                # the initial value and two others
                lq = float(np.log(rng.choice([0.9, 0.3]))) if band == 0 else [LN_FLOOR, float(np.log(3e-3)), float(np.log(0.05))][rng.integers(3)]
                c = Case(name, [*z3[k], *xy], uv[k], pc[k] if metric else 0.0, ip, window, rng, lq)
                th = {n: float(v) for n, v in X.clamp_thresholds(solver, mp.exp(mpf(lq))).items()}
                # rejected attempts up to EEst = 30 under the settings' tolerances, beyond under the tight ones (an error of 30 reltol is
                # still a step that resolves the solution; one of 1e3 reltol is not)
                tight = band == 3 or (band == 2 and taken % 2 == 1)
                lo, hi = [(th["qmax"] * 1e-3, th["qmax"] * 0.05), (3e-4, 0.7), (30.0, 0.3 * th["qmin"]) if tight else (1.5, 30.0),
                          (5.0 * th["qmin"], 1e12)][band]
                c.band, c.th, c.tol = band, th, TIGHT if tight else LOOSE if band == 0 else None
                c.h = find_step(c, tabs["fp64"], lo, hi, math.sqrt(lo * hi) if band < 3 else 50.0 * th["qmin"])
                four.append(c)
            if max(c.h for c in four) <= 1e5:
                cases += four
                taken += 1
        assert taken == N_PER_REGIME, name
    out = []
    for c in cases:
        parts = {}
        node = c.node(X.MP, c.h)
        node.f([mpf(float(x)) for x in c.z5], mpf(c.t), parts)
        assert_inside(c.regime, parts)
        if window == "knot":
            w = c.wind_win(c.h)[1]
            assert c.t < w[0] + w[2] * w[1] < c.t + c.h
        r = {}
        for A in (X.MP, X.FP):
            a = X.explicit_attempt(c.node(A, c.h), tabs[A.name], c.z5, c.t, c.h, *c.tols())
            q = mp.exp(mpf(c.lq)) if A is X.MP else math.exp(c.lq)
            a["lnE"] = X._log(A, a["EEst"])
            a["accept"] = a["EEst"] <= 1
            a["factor"], a["qold"] = X.pi_accept(A, solver, a["EEst"], q) if a["accept"] else (X.pi_reject(A, solver, a["EEst"]), q)
            r[A.name] = a
        out.append(r)
    return cases, out


def ln_eest_bound(cases, refs, band):
    """the bound on ln EEst in a band: MARGIN x the fp64 noise of the reference there, plus pm_log_coarse's ½ · 2e-9"""
    noise = [abs(float(r["fp64"]["lnE"] - r["mp"]["lnE"])) for c, r in zip(cases, refs) if c.band == band]
    return MARGIN * max(noise) + 0.5 * LOG_COARSE


def run_attempts(variant, solver, cases):
    """one attempt per case (grouped by their tolerances: one host call each), merged in the order of the cases"""
    p, out = structs()[0], None
    for tol in sorted({c.tol for c in cases}, key=str):
        ks = [k for k, c in enumerate(cases) if c.tol == tol]
        cs = [cases[k] for k in ks]
        ww = [c.wind_win(c.h) for c in cs]
        got = H.attempt(p, ode(tol), variant, solver, [c.z5 for c in cs], [w[0] for w in ww], [w[1] for w in ww], [c.t for c in cs],
                        [c.h for c in cs], [c.lq for c in cs], [c.ipx for c in cs], [c.ipy for c in cs], [c.pc for c in cs])
        if out is None:
            out = {name: np.zeros((len(cases),) + v.shape[1:], dtype=v.dtype) for name, v in got.items()}
        for name, v in got.items():
            out[name][ks] = v
    return out


def rel(a, ref):
    return abs(float((mpf(float(a)) - ref) / ref))


# ---- (a) the attempt ----
@pytest.mark.parametrize("window,metric", SETS, ids=[w + ("-metric" if m else "") for w, m in SETS])
@pytest.mark.parametrize("solver", ["dp5", "tsit5"])
def test_attempt_against_the_reference(solver, window, metric):
    cases, refs = attempt_set(solver, window, metric)
    beta1 = float(X.BETA[solver][0])
    tag = f"attempt {solver} {window}" + (" metric" if metric else "")
    n = len(cases)
    band = np.array([c.band for c in cases])
    assert (np.bincount(band, minlength=4) == n // 4).all()          # no case is left out: every state in every band
    # the reference's EEst keeps its distance from every branch and clamp: more than the bound on ln EEst of its band
    for b in range(4):
        bound = ln_eest_bound(cases, refs, b)
        for c, r in zip(cases, refs):
            if c.band != b:
                continue
            e = r["mp"]["EEst"]
            dist = min(abs(float(mp.log(e / mpf(t)))) for t in c.th.values())
            assert dist > bound, (tag, BANDS[b], float(e), c.th, bound)
            inside = [e < c.th["qmax"] and e < c.th["floor"], c.th["floor"] < e < 1 and e > c.th["qmax"], 1 < e < c.th["qmin"], e > c.th["qmin"]][b]
            assert inside and r["fp64"]["accept"] == r["mp"]["accept"], (tag, BANDS[b], float(e), c.th)
        print(f"{tag}, {BANDS[b]}: EEst from {min(float(r['mp']['EEst']) for c, r in zip(cases, refs) if c.band == b):.2e} to "
              f"{max(float(r['mp']['EEst']) for c, r in zip(cases, refs) if c.band == b):.2e}, bound on ln EEst {bound:.2e}")
    acc = band < 2
    un_noise = [X.fp64_noise(r["mp"]["un"], r["fp64"]["un"], r["mp"]["scale"]) for r in refs]
    lnE_noise = [abs(float(r["fp64"]["lnE"] - r["mp"]["lnE"])) for r in refs]
    f_noise = [rel(r["fp64"]["factor"], r["mp"]["factor"]) for r in refs]
    for variant in VARIANTS_OF[(window, metric)]:
        got = run_attempts(variant, solver, cases)
        z0 = np.array([c.z5 for c in cases], dtype=np.float64)
        h, lq0 = np.array([c.h for c in cases]), np.array([c.lq for c in cases])
        # the branch
        assert (got["acc"] == acc).all() and (got["rej"] == ~acc).all(), (tag, variant)
        assert (got["rhs"] == 7).all() and (got["status"] == H.ST_MAXITERS).all()
        # a rejected attempt leaves the state and the controller's memory alone
        assert np.array_equal(got["z"][~acc], z0[~acc]) and np.array_equal(got["lq"][~acc], lq0[~acc])
        # the clamps, to the bit
        assert (got["lq"][band == 0] == LN_FLOOR).all() and (got["dtn"][band == 0] == h[band == 0] * 10.0).all()
        assert (got["dtn"][band == 3] == h[band == 3] * 0.2).all()
        # u_new per component in units of scale_i
        ks = np.flatnonzero(acc)
        check(tag + " un", [un_noise[k] for k in ks], [X.fp64_noise(refs[k]["mp"]["un"], got["z"][k], refs[k]["mp"]["scale"]) for k in ks])
        # ln EEst where EEst > 1e-4, through the new lq
        ks = np.flatnonzero(band == 1)
        check(tag + " ln EEst", [lnE_noise[k] for k in ks], [abs(float(mpf(float(got["lq"][k])) - refs[k]["mp"]["lnE"])) for k in ks],
              extra=0.5 * LOG_COARSE)
        # the unclamped factors, accepted and rejected
        ks = np.flatnonzero((band == 1) | (band == 2))
        check(tag + " factor", [f_noise[k] for k in ks], [rel(got["dtn"][k] / h[k], refs[k]["mp"]["factor"]) for k in ks],
              extra=0.5 * beta1 * LOG_COARSE)
        for k in ks:
            assert 0.2 < got["dtn"][k] / h[k] < 10.0


# ---- (b) the controller ----
CARRIED = [LN_FLOOR, math.log(1e-3), math.log(0.02), math.log(0.3), 0.0]          # ln qold: the initial value … 1


@pytest.mark.parametrize("solver", ["dp5", "tsit5"])
def test_controller_factors_and_memory(solver):
    """both β pairs, accepted and rejected attempts, five carried ln qold: the factor dtn / h against clamp(γ qold^β2 / EEst^β1) and
    max(qmin, γ / EEst^β1) at 60 digits, the new lq against ln EEst.  A rejected factor and every new lq do not depend on the carried
    value, to the bit"""
    cases, refs = attempt_set(solver, "static", False)
    ks = [k for k, c in enumerate(cases) if c.band in (1, 2)]
    cs, rs = [cases[k] for k in ks], [refs[k] for k in ks]
    acc = np.array([c.band == 1 for c in cs])
    beta1 = float(X.BETA[solver][0])
    h = np.array([c.h for c in cs])
    first = None
    for lq in CARRIED:
        ref_f, fp_f = [], []
        for c, r in zip(cs, rs):
            th = X.clamp_thresholds(solver, mp.exp(mpf(lq)))
            if c.band == 1:          # the accepted factor stays unclamped under this qold as well
                assert abs(float(mp.log(r["mp"]["EEst"] / th["qmax"]))) > ln_eest_bound(cases, refs, 1) and r["mp"]["EEst"] > th["qmax"]
                ref_f.append(X.pi_accept(X.MP, solver, r["mp"]["EEst"], mp.exp(mpf(lq)))[0])
                fp_f.append(X.pi_accept(X.FP, solver, r["fp64"]["EEst"], math.exp(lq))[0])
            else:
                ref_f.append(X.pi_reject(X.MP, solver, r["mp"]["EEst"]))
                fp_f.append(X.pi_reject(X.FP, solver, r["fp64"]["EEst"]))
        saved = [c.lq for c in cs]
        for c in cs:
            c.lq = lq
        try:
            got = run_attempts((True, True, False), solver, cs)
        finally:
            for c, s in zip(cs, saved):
                c.lq = s
        assert (got["acc"] == acc).all() and (got["rej"] == ~acc).all()
        f = got["dtn"] / h
        assert ((f > 0.2) & (f < 10.0)).all()
        check(f"controller {solver} factor", [rel(a, b) for a, b in zip(fp_f, ref_f)], [rel(a, b) for a, b in zip(f, ref_f)],
              extra=0.5 * beta1 * LOG_COARSE)
        check(f"controller {solver} lq", [abs(float(r["fp64"]["lnE"] - r["mp"]["lnE"])) for r in np.array(rs)[acc]],
              [abs(float(mpf(float(x)) - r["mp"]["lnE"])) for x, r in zip(got["lq"][acc], np.array(rs)[acc])], extra=0.5 * LOG_COARSE)
        assert (got["lq"][~acc] == lq).all()
        if first is None:
            first = got
        else:
            assert np.array_equal(got["lq"][acc], first["lq"][acc]) and np.array_equal(got["dtn"][~acc], first["dtn"][~acc])
            assert not np.array_equal(got["dtn"][acc], first["dtn"][acc])          # the memory is at work


# ---- (c) the constants ----
def _entry(tab, field):
    i, j = int(field[1]), int(field[2:]) if len(field) > 2 else None
    return tab["A"][i - 1][j - 1] if field[0] == "a" else tab[field[0]][i - 1]


def test_compiled_tables_are_the_rationals_and_the_published_doubles():
    """all 2 x 32 entries dp_load produces: DP5's equal the correctly rounded rationals (Python rounds int / int correctly), Tsit5's
    equal tests/test_tableaux.TSIT5 entry by entry"""
    for solver in ("dp5", "tsit5"):
        got, exact = H.table(solver), X.tableau_exact(solver)
        assert list(got) == list(H.TABLE_FIELDS) and len(got) == 32
        for field, v in got.items():
            x = _entry(exact, field)
            want = x.numerator / x.denominator if solver == "dp5" else x
            assert v == want, (solver, field, v, want)


def test_controller_and_autoswitch_macros_are_the_rationals():
    c = H.constants()
    want = dict(PI_BETA1=X.BETA["dp5"][0], PI_BETA2=X.BETA["dp5"][1], PI_BETA1_TSIT=X.BETA["tsit5"][0], PI_BETA2_TSIT=X.BETA["tsit5"][1],
                PI_GAMMA=X.GAMMA, PI_QMIN=X.QMIN, PI_QMAX=X.QMAX, PI_QOLDINIT=X.QOLD_INIT, ASW_STABILITY=X.STABILITY)
    for name, x in want.items():
        assert c[name] == x.numerator / x.denominator, (name, c[name], x)
    assert c["PI_LNQOLDINIT"] == LN_FLOOR == math.log(c["PI_QOLDINIT"])
    assert c["ASW_FRESH"] == -2 ** 31


# ---- (d) the detector ----
AUTO_SETS = [((True, True, False), "static", False), ((True, False, False), "parabola", False), ((True, False, True), "parabola", True),
             ((False, False, False), "knot", False)]


def enc(count, stiff):
    """asw as the integrator carries it: counter << 1 | Rosenbrock23 active"""
    return (count << 1) | int(stiff)


@functools.lru_cache(maxsize=None)
def detector_cases(window, metric):
    """the accepted attempts of the Tsit5 set whose estimate can be bracketed: the carried ln qold that puts
    eigen_est · dt_next / (0.9 · 3.5068) at 1 asks for an accepted factor inside (0.25, 8), clear of both clamps.  Returns the cases,
    their references, the fp64 noise of that ratio per case and a function lq(k, ratio)"""
    cases, refs = attempt_set("tsit5", window, metric)
    b1, b2 = (X.num(X.MP, x) for x in X.BETA["tsit5"])
    keep, noise = [], []

    def lq_for(k, ratio):
        r = refs[k]["mp"]
        fstar = mpf(ratio) / X.stiff_ratio(X.MP, r["eig"], mpf(cases[k].h))
        return fstar, (mp.log(fstar / X.num(X.MP, X.GAMMA)) + b1 * r["lnE"]) / b2

    for k, c in enumerate(cases):
        if c.band != 1:
            continue
        fstar, lq = lq_for(k, 1)
        if not 0.25 < fstar < 8:
            continue
        fp = refs[k]["fp64"]
        f_fp = X.pi_accept(X.FP, "tsit5", fp["EEst"], math.exp(float(lq)))[0]
        keep.append(k)
        noise.append(abs(float(X.stiff_ratio(X.FP, fp["eig"], c.h * f_fp)) - 1.0))
    return cases, refs, keep, np.array(noise), lq_for


@pytest.mark.parametrize("variant,window,metric", AUTO_SETS, ids=["fast-static", "fast-parabola", "fast-parabola-metric", "general-knot"])
def test_stiffness_estimate_by_bracketing(variant, window, metric):
    """per state the carried lq that puts the reference's eigen_est · dt_next / (0.9 · 3.5068) at 1 + δ, then at 1 − δ: the AutoSwitch
    test in front of the second attempt counts a positive, then a negative.  δ = 16 x the fp64 noise of the reference's own ratio on
    this sample (the cancellation in k7 − k6 is why it is measured) + ½ β1 · 2e-9 for the controller's coarse logarithm"""
    cases, refs, keep, noise, lq_for = detector_cases(window, metric)
    tag = f"detector {window}" + (" metric" if metric else "")
    delta = MARGIN * float(noise.max()) + 0.5 * float(X.BETA["tsit5"][0]) * LOG_COARSE
    print(f"{tag}: {len(keep)} states bracketed, fp64 noise of the ratio {noise.max():.2e}, δ = {delta:.2e}")
    assert len(keep) >= 6 and delta < 1e-3
    if tag in RECORDED:
        assert RECORDED[tag][0] / 4 <= noise.max() <= RECORDED[tag][0] * 4, (tag, "the yardstick moved", noise.max())
    cs = [cases[k] for k in keep]
    saved = [c.lq for c in cs]
    try:
        for ratio, want in ((1 + delta, enc(1, False)), (1 - delta, enc(-1, False))):
            for c, k in zip(cs, keep):
                c.lq = float(lq_for(k, ratio)[1])
            p = structs()[0]
            ww = [c.wind_win(c.h) for c in cs]
            got = H.integrate(p, ode(), variant, "auto", [c.z5 for c in cs], [w[0] for w in ww], [w[1] for w in ww], [c.t for c in cs],
                              [100.0 * c.h for c in cs], [c.lq for c in cs], [c.h for c in cs], [c.ipx for c in cs], [c.ipy for c in cs],
                              [c.pc for c in cs], asw=enc(0, False), maxiters=2)
            assert (got["acc"] >= 1).all() and (got["acc"] + got["rej"] == 2).all()
            assert (got["asw"] == want).all(), (tag, ratio, got["asw"])
    finally:
        for c, s in zip(cs, saved):
            c.lq = s


def _auto(z, uv, t0, DT, lq, dtn, ip, asw, maxiters, o=None):
    """AutoTsit5 of the fast / static flavour on one state"""
    r = H.integrate(structs()[0], ode() if o is None else o, (True, True, False), "auto", z, [uv[0], uv[1], 0, 0, 0, 0], [0.0, 0.0, 0.0],
                    t0, DT, lq, dtn, ip[0], ip[1], 0.0, asw=asw, maxiters=maxiters)
    return {k: v[0] for k, v in r.items()}


def _same(a, b, keys=("z", "lq", "dtn", "asw")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def test_autoswitch_counters_and_the_step_they_hand_over():
    """the counter rules, stepped in through asw.  Non-stiff with counts 9, 10, 11 and a positive test: the switch to Rosenbrock23
    happens only beyond 10, with dt doubled; stiff with counts -2, -3, -4 and a negative test: the return only beyond 3, with dt halved.
    The step is observed by composition: two attempts in one call equal the first attempt followed by a call that enters with the
    reference's (count, stiff) and the reference's dt — and differ from the call that enters with the dt unchanged"""
    cases, refs, keep, noise, lq_for = detector_cases("static", False)
    k = keep[0]
    c = cases[k]
    ip, DT = (c.ipx, c.ipy), 1000.0 * c.h
    delta = MARGIN * float(noise.max()) + 0.5 * float(X.BETA["tsit5"][0]) * LOG_COARSE
    lq_pos = float(lq_for(k, 1 + delta)[1])
    for count in (9, 10, 11):
        a = _auto(c.z5, c.uv, c.t, DT, lq_pos, c.h, ip, enc(count, False), 1)
        b = _auto(c.z5, c.uv, c.t, DT, lq_pos, c.h, ip, enc(count, False), 2)
        n, stiff, dt = X.asw_step(count, False, True, float(a["dtn"]))
        assert stiff == (count >= 10) and a["asw"] == enc(count, False) and a["acc"] == 1
        assert b["asw"] == enc(n, stiff), (count, b["asw"])
        d = _auto(a["z"], c.uv, c.t + c.h, DT - c.h, a["lq"], dt, ip, enc(n, stiff), 1)
        assert _same(b, d) and b["acc"] + b["rej"] == 2 and b["rhs"] == a["rhs"] + d["rhs"] - 1, count
        if stiff:
            assert dt == 2.0 * a["dtn"]
            assert not _same(b, _auto(a["z"], c.uv, c.t + c.h, DT - c.h, a["lq"], float(a["dtn"]), ip, enc(n, stiff), 1), ("z", "dtn"))
    # Rosenbrock23 active: a step so short that ‖J‖ · 10 h stays below 0.9 · 3.5068 whatever the controller answers
    wind = [c.uv[0], c.uv[1], 0, 0, 0, 0]
    eig = S.ros23(structs()[0], ode(), (True, True, False), c.z5, wind, (0.0, 0.0, 0.0), c.t, 1e-3, *ip)[3][0]
    h = 0.2 / eig
    for count in (-2, -3, -4):
        a = _auto(c.z5, c.uv, c.t, 1000.0 * h, LN_FLOOR, h, ip, enc(count, True), 1)
        b = _auto(c.z5, c.uv, c.t, 1000.0 * h, LN_FLOOR, h, ip, enc(count, True), 2)
        n, stiff, dt = X.asw_step(count, True, False, float(a["dtn"]))
        assert stiff == (count > -3) and a["asw"] == enc(count, True) and a["acc"] == 1
        assert float(X.stiff_ratio(X.FP, eig, float(a["dtn"]))) < 0.5          # a clear negative
        assert b["asw"] == enc(n, stiff), (count, b["asw"])
        d = _auto(a["z"], c.uv, c.t + h, 1000.0 * h - h, a["lq"], dt, ip, enc(n, stiff), 1)
        assert _same(b, d) and b["acc"] + b["rej"] == 2, count
        if not stiff:
            assert dt == 0.5 * a["dtn"]
            assert not _same(b, _auto(a["z"], c.uv, c.t + h, 1000.0 * h - h, a["lq"], float(a["dtn"]), ip, enc(n, stiff), 1), ("z", "dtn"))


def test_a_fresh_switch_state_skips_one_test():
    """ASW_FRESH enters as (count 0, Tsit5) and skips the test in front of its first attempt — the one for which no estimate exists:
    one attempt leaves asw = 0, two attempts leave exactly ONE test counted (±1), and every output equals the entry with asw = 0"""
    cases, refs, keep, noise, lq_for = detector_cases("static", False)
    fresh = H.constants()["ASW_FRESH"]
    for k in keep[:4]:
        c = cases[k]
        delta = MARGIN * float(noise.max()) + 0.5 * float(X.BETA["tsit5"][0]) * LOG_COARSE
        for ratio, want in ((1 + delta, enc(1, False)), (1 - delta, enc(-1, False))):
            lq = float(lq_for(k, ratio)[1])
            for n, asw in ((1, 0), (2, want)):
                f = _auto(c.z5, c.uv, c.t, 100.0 * c.h, lq, c.h, (c.ipx, c.ipy), fresh, n)
                z = _auto(c.z5, c.uv, c.t, 100.0 * c.h, lq, c.h, (c.ipx, c.ipy), 0, n)
                assert f["asw"] == asw and _same(f, z, ("z", "lq", "dtn", "asw", "rhs", "acc", "rej", "status"))


# ---- (e) the loop is the composition of attempts ----
def drive(variant, solver, z, wind, win, DT, lq, dtn, ip, pc):
    """step!(integrator, DT) from Python: maxiters = 1 calls over what remains of DT, with the integrator's own rule for the last
    step (h = rem where dt is not below rem; an accepted last step ends at DT itself)"""
    p, o = structs()[0], ode()
    tr, tot, calls, cut, status = 0.0, dict(acc=0, rej=0, rhs=0), 0, False, 0
    while tr < DT:
        rem = DT - tr
        last = not dtn < rem
        h = rem if last else dtn
        r = H.integrate(p, o, variant, solver, z, wind, win, tr, rem, lq, dtn, ip[0], ip[1], pc, maxiters=1)
        calls += 1
        assert r["acc"][0] + r["rej"][0] == 1
        for key in tot:
            tot[key] += int(r[key][0])
        status |= int(r["status"][0]) & ~H.ST_MAXITERS          # the flags are sticky (a NaN estimate counts as a rejection and is flagged)
        if r["acc"][0]:
            cut |= last and dtn > rem
            tr = DT if last else tr + h
        z, lq, dtn = r["z"][0], float(r["lq"][0]), float(r["dtn"][0])
        assert calls < 1000
    tot["rhs"] -= calls - 1          # every call after the first evaluates again the stage the loop carries over (first same as last)
    return dict(z=z, lq=lq, dtn=dtn, status=status, **tot), cut


LOOP_SETS = [((True, True, False), [0.0, 0.0, 0.0], 0.0), ((True, False, False), [0.0, 600.0, 0.0], 0.0), ((False, False, False), [0.0, 600.0, 0.37], 0.0),
             ((True, False, True), [0.0, 600.0, 0.0], 3e-7)]


@pytest.mark.parametrize("variant,win,pc", LOOP_SETS, ids=["fast-static", "fast-parabola", "general-knot", "fast-parabola-metric"])
@pytest.mark.parametrize("solver", ["dp5", "tsit5"])
def test_the_loop_is_the_composition_of_attempts(solver, variant, win, pc):
    """one call over DT = 600 s equals, bit for bit, the attempts driven one by one from Python (t_start = 0: the wind time of the
    first-same-as-last stage, t + h, is the next attempt's t to the bit).  The first dt, 300 s, is rejected at least once; the last
    step is cut by what remains"""
    z3, uv, _, _ = regime_states("plain")
    rng = np.random.default_rng([20261025, H.SOLVERS[solver], H.VARIANTS[variant]])
    rejected = cuts = 0
    for k in range(6):
        z = [*z3[k], *rng.uniform(-0.9, 0.9, 2)]
        tv = 0.0 if variant[1] else 1.0
        wind = [uv[k, 0], uv[k, 1], *(rng.uniform(-3.0, 3.0, 2) * tv), *(rng.uniform(-4.0, 4.0, 2) * tv)]
        ip = (1.1e-3, -0.7e-3)
        whole = H.integrate(structs()[0], ode(), variant, solver, z, wind, win, 0.0, 600.0, math.log(3e-3), 300.0, ip[0], ip[1], pc, maxiters=100000)
        mine, cut = drive(variant, solver, z, wind, win, 600.0, math.log(3e-3), 300.0, ip, pc)
        assert whole["status"][0] == mine["status"] and not whole["status"][0] & H.ST_MAXITERS
        assert np.array_equal(whole["z"][0], mine["z"]) and whole["lq"][0] == mine["lq"] and whole["dtn"][0] == mine["dtn"]
        assert (int(whole["acc"][0]), int(whole["rej"][0]), int(whole["rhs"][0])) == (mine["acc"], mine["rej"], mine["rhs"])
        rejected += mine["rej"]
        cuts += cut
    assert rejected >= 1 and cuts >= 1


# ---- (f) the bridge to the oracle ----
@functools.lru_cache(maxsize=None)
def oracle_model(solver, U, V):
    import _oracle as O
    from picles_amd import configs, fetch_relations as FR
    from picles_amd.models import build_structs
    cfg = configs.bench06_box(n=8, U10=U, V10=V)
    sets = cfg.model["ODEsets"]
    sets.solver = solver
    g, p, o, m = build_structs(cfg.model["grid"], cfg.model["ODEsys"], sets, None, FR.MinimalState(2, 2, sets.timestep), True)
    M = O.OracleModel(g, p, o, m, kind="pmath", order=1, mask=cfg.model["grid"].data.mask)
    M.set_winds(np.full((8, 8), float(U)), np.full((8, 8), float(V)), 0.0)
    return M, p, o, (1.0 / g.dx, 1.0 / g.dy)


@pytest.mark.parametrize("solver", ["dp5", "tsit5", "auto"])
def test_host_build_equals_the_oracle_bitwise(solver):
    """the same states and inputs through OracleModel(kind="pmath", order=1).integrate / integrate_auto: z, ln qold, dt, asw and the
    counters, bit for bit — what ties this pin, through the GPU parity suites, to the device"""
    import _oracle as O
    n = 0
    for U, V in ((10.0, 10.0), (10.0, 3.0), (8.0, -11.0)):
        M, p, o, ip = oracle_model(H.SOLVERS[solver], U, V)
        seed = O.windsea(U, V, 1800.0, "pmath")
        for z in ([*seed, 0.0, 0.0], [0.5, 6.0, -2.5, 0.3, -0.2], [-6.0, 0.9, 0.7, 0.0, 0.0]):
            lq, dtn, asw = LN_FLOOR, -1.0, -2 ** 31
            zz = np.array(z, dtype=np.float64)
            for step in range(3):          # three model steps: the controller's memory and the switch state are carried
                if solver == "auto":
                    zo, so = M.integrate_auto(0, zz, 600.0 * step, 600.0, qold=lq, dtn=dtn, asw=asw)
                else:
                    zo, so = M.integrate(0, zz, 600.0 * step, 600.0, qold=lq, dtn=dtn)
                got = H.integrate(p, o, (True, True, False), solver, zz, [U, V, 0, 0, 0, 0], [0.0, 0.0, 0.0], 600.0 * step, 600.0, lq, dtn,
                                  ip[0], ip[1], 0.0, asw=asw)
                assert np.array_equal(got["z"][0], zo), (solver, U, V, z, step)
                assert got["lq"][0] == so["qold"] and got["dtn"][0] == so["dt"]
                assert (int(got["rhs"][0]), int(got["acc"][0]), int(got["rej"][0]), int(got["status"][0])) == (so["rhs"], so["acc"], so["rej"], so["status"])
                if solver == "auto":
                    assert got["asw"][0] == so["asw"]
                    asw = so["asw"]
                zz, lq, dtn = zo, so["qold"], so["dt"]
                n += so["acc"]
    assert n > 20


# ---- (g) the order of the attempt ----
@pytest.mark.parametrize("solver", ["dp5", "tsit5"])
def test_local_error_falls_by_2_to_the_6_and_the_estimate_by_2_to_the_5(solver):
    """a pair of orders 5(4): from h to h/2 the local error of u_new — against the exact solution, RK4 in mpmath with 400 substeps —
    falls by about 2⁶ and EEst by about 2⁵.  Asserted on the reference attempt at 60 digits first, then on the code"""
    p, o, ipx, ipy = box_structs()
    o = ode(TIGHT)          # EEst stays above 1e-4, where lq shows it, down to steps at which the error terms beyond the leading one are small
    z5, uv, h = [0.5, 6.0, -2.5, 0.0, 0.0], (8.0, -11.0), ORDER_H
    wind, win = [uv[0], uv[1], 0.0, 0.0, 0.0, 0.0], (0.0, 0.0, 0.0)
    node = X.Node(X.MP, p, wind, win, 0.0, ipx, ipy)
    tab = X.tableau(X.MP, solver)
    err_ref, est_ref, err_code, est_code = [], [], [], []
    for hh in (h, 0.5 * h):
        exact = X.rk4_exact(node, z5, 0.0, hh, 400)
        a = X.explicit_attempt(node, tab, z5, 0.0, hh, o.abstol, o.reltol)
        assert a["EEst"] < 1
        got = H.attempt(p, o, (True, True, False), solver, z5, wind, win, 0.0, hh, LN_FLOOR, ipx, ipy)
        assert got["acc"][0] == 1
        sc = a["scale"]
        err_ref.append(float(max(abs(x - e) / s for x, e, s in zip(a["un"], exact, sc))))
        err_code.append(float(max(abs(mpf(float(x)) - e) / s for x, e, s in zip(got["z"][0], exact, sc))))
        est_ref.append(float(a["EEst"]))
        est_code.append(math.exp(got["lq"][0]))
        assert a["EEst"] > 1e-4
    ref_f, code_f = (err_ref[0] / err_ref[1], est_ref[0] / est_ref[1]), (err_code[0] / err_code[1], est_code[0] / est_code[1])
    print(f"order {solver}: h = {h}: local error and estimate fall by {ref_f[0]:.3f}, {ref_f[1]:.3f} (reference), {code_f[0]:.3f}, {code_f[1]:.3f} (code); "
          f"EEst {est_ref[0]:.3e}, local error {err_ref[0]:.3e} scale")
    lo, hi = ORDER_BAND[solver]
    for f in (ref_f, code_f):
        assert lo[0] < f[0] < hi[0] and lo[1] < f[1] < hi[1], (solver, f)
