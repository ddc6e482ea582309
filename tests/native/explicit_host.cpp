// explicit_host.cpp — a HOST build of the explicit half of the default solver (picles_amd/csrc/physics.h: integrate_dp5 with its
// seven-stage DP5 / Tsit5 attempt, the log-space PI controller, the accept / reject rule, the Tsit5 stiffness estimate and the
// AutoSwitch counters) behind plain C functions over arrays of n states: what tests/test_explicit_reference.py holds against the
// independent 60-digit restatement of the textbook formulas (tests/_explicit_mp.py).  Compiled by the tests with the oracle's flags
// (-ffp-contract=off); the derived constants are those of picles_create (host_params.h).
// Layouts, all row-major: z5 [n][5] (ln e, c̄x, c̄y, x, y), wind [n][6] (u0, v0, du, dv, bu, bv of struct Wind), win [n][3] (tw0, dtw,
// wind_sk; dtw <= 0: the static window), stats [n][4] (rhs, acc, rej, status).
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>

#include "host_params.h"

#define API extern "C" __attribute__((visibility("default")))

template <bool FAST, bool STATIC, bool METRIC>
static void run_one(int solver, const KParams &P, const Wind &w, Vec5 &z, double &lq, double &dtn, double t0, double DT, PStats &st,
                    double m11, double m22, double pc, int *asw)
{
    switch (solver) {
    case 0: integrate_dp5<FAST, STATIC, METRIC, false, false>(P, w, z, lq, dtn, t0, DT, st, m11, m22, pc, nullptr); break;
    case 1: integrate_dp5<FAST, STATIC, METRIC, true, false>(P, w, z, lq, dtn, t0, DT, st, m11, m22, pc, nullptr); break;
    default: integrate_dp5<FAST, STATIC, METRIC, true, true>(P, w, z, lq, dtn, t0, DT, st, m11, m22, pc, asw); break;
    }
}

// variant: 0 <true, true, false>, 1 <true, false, false>, 2 <true, false, true>, 3 <false, false, false> (FAST, STATIC, METRIC);
// solver: 0 DP5, 1 Tsit5, 2 AUTO.  The projection (ipx, ipy) is 1/Δx, 1/Δy of KParams for the Cartesian variants and m11, m22 for the
// metric one, which alone reads pc.  z5, lq, dtn and asw are updated in place; maxiters and the tolerances come from *o.
API int32_t explicit_integrate(const picles_phys *p, const picles_ode *o, int32_t variant, int32_t solver, int64_t n, double *z5,
                               const double *wind, const double *win, const double *t_start, const double *DT, double *lq, double *dtn,
                               const double *ipx, const double *ipy, const double *pc, int32_t *asw, int64_t *stats)
{
    if (variant < 0 || variant > 3 || solver < 0 || solver > 2) return -1;
    KParams P;
    host_params(p, nullptr, P);
    host_params_ode(o, P);
    for (int64_t k = 0; k < n; k++) {
        host_params_window(win[3 * k], win[3 * k + 1], win[3 * k + 2], P);
        P.inv_dx = ipx[k]; P.inv_dy = ipy[k];
        Wind w;
        const double *a = wind + 6 * k;
        w.u0 = a[0]; w.v0 = a[1]; w.du = a[2]; w.dv = a[3]; w.bu = a[4]; w.bv = a[5]; w.xi = 0;
        double *zz = z5 + 5 * k;
        Vec5 z = {zz[0], zz[1], zz[2], zz[3], zz[4]};
        PStats st = {0, 0, 0, 0};
        int sw = asw[k];
        switch (variant) {
        case 0: run_one<true, true, false>(solver, P, w, z, lq[k], dtn[k], t_start[k], DT[k], st, 0.0, 0.0, 0.0, &sw); break;
        case 1: run_one<true, false, false>(solver, P, w, z, lq[k], dtn[k], t_start[k], DT[k], st, 0.0, 0.0, 0.0, &sw); break;
        case 2: run_one<true, false, true>(solver, P, w, z, lq[k], dtn[k], t_start[k], DT[k], st, ipx[k], ipy[k], pc[k], &sw); break;
        default: run_one<false, false, false>(solver, P, w, z, lq[k], dtn[k], t_start[k], DT[k], st, 0.0, 0.0, 0.0, &sw); break;
        }
        asw[k] = sw;
        zz[0] = z.lne; zz[1] = z.cx; zz[2] = z.cy; zz[3] = z.x; zz[4] = z.y;
        stats[4 * k] = st.rhs; stats[4 * k + 1] = st.acc; stats[4 * k + 2] = st.rej; stats[4 * k + 3] = st.status;
    }
    return 0;
}

// the DPTAB_N = 32 entries dp_load produces, in the order of struct DPTab (a21 … a76, c2 … c5, e1 … e7); solver 0 DP5, 1 Tsit5
API int32_t explicit_table(int32_t solver, double *out)
{
    static_assert(sizeof(DPTab) == DPTAB_N * sizeof(double), "DPTab is DPTAB_N doubles");
    DPTab T;
    dp_load(T, solver);
    const double *t = &T.a21;
    for (int k = 0; k < DPTAB_N; k++) out[k] = t[k];
    return DPTAB_N;
}

// the PI and AutoSwitch macros: β1, β2 (DP5), β1, β2 (Tsit5), γ, qmin, qmax, qold's initial value and its logarithm, the stability
// size; *fresh receives ASW_FRESH
API int32_t explicit_constants(double *out, int32_t *fresh)
{
    const double c[10] = {PI_BETA1, PI_BETA2, PI_BETA1_TSIT, PI_BETA2_TSIT, PI_GAMMA, PI_QMIN, PI_QMAX, PI_QOLDINIT, PI_LNQOLDINIT, ASW_STABILITY};
    for (int k = 0; k < 10; k++) out[k] = c[k];
    *fresh = ASW_FRESH;
    return 10;
}
