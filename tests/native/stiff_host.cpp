// stiff_host.cpp — a HOST build of the stiff half of the default solver (picles_amd/csrc/physics.h: rhs3, rhs3_jac_plain, rhs3_jvp,
// ros23_try, init_dt) behind plain C functions over arrays of n states: what tests/test_stiff_reference.py holds against the
// independent 60-digit restatement of the reference's formulas (tests/_stiff_mp.py).  Compiled by the tests with the oracle's flags
// (-ffp-contract=off); the derived constants are those of picles_create (host_params.h).
// Layouts, all row-major doubles: z3 [n][3] (ln e, c̄x, c̄y), z5 [n][5] (+ x, y), uv [n][2], duv [n][2] (the wind's slope per second),
// wind [n][6] (u0, v0, du, dv, bu, bv of struct Wind), win [n][3] (tw0, dtw, wind_sk; dtw <= 0: the static window).
// TEST INFRASTRUCTURE ONLY.
#include <cstdint>

#include "host_params.h"

#define API extern "C" __attribute__((visibility("default")))

static void wind_of(const KParams &P, double u, double v, WindD &W)
{
    W.sh = PM_EXP_SHIFTER();
    wind_derive(P, u, v, W);
}

API void stiff_rhs3(const picles_phys *p, int32_t fast, int32_t metric, int64_t n, const double *z3, const double *uv, const double *pc,
                    double *f)
{
    KParams P;
    host_params(p, nullptr, P);
    for (int64_t k = 0; k < n; k++) {
        WindD W;
        wind_of(P, uv[2 * k], uv[2 * k + 1], W);
        Vec3 d;
        const double L = z3[3 * k], cx = z3[3 * k + 1], cy = z3[3 * k + 2];
        if (fast) { if (metric) rhs3<true, true>(P, L, cx, cy, W, d, pc[k]); else rhs3<true, false>(P, L, cx, cy, W, d, 0.0); }
        else      { if (metric) rhs3<false, true>(P, L, cx, cy, W, d, pc[k]); else rhs3<false, false>(P, L, cx, cy, W, d, 0.0); }
        f[3 * k] = d.lne; f[3 * k + 1] = d.cx; f[3 * k + 2] = d.cy;
    }
}

// J [n][9] row-major (J[3 r + c] = ∂f_r/∂u_c), dT [n][3] (zeros when tv == 0), y [n] = 1/|c̄|
API void stiff_jac_plain(const picles_phys *p, int32_t metric, int32_t tv, int64_t n, const double *z3, const double *uv, const double *pc,
                         const double *duv, double *J, double *dT, double *y)
{
    KParams P;
    host_params(p, nullptr, P);
    for (int64_t k = 0; k < n; k++) {
        WindD W;
        wind_of(P, uv[2 * k], uv[2 * k + 1], W);
        double Jm[9];
        Vec3 d = {0.0, 0.0, 0.0};
        const double L = z3[3 * k], cx = z3[3 * k + 1], cy = z3[3 * k + 2], du = duv[2 * k], dv = duv[2 * k + 1];
        if (metric) y[k] = tv ? rhs3_jac_plain<true, true>(P, L, cx, cy, W, pc[k], du, dv, Jm, d)
                              : rhs3_jac_plain<true, false>(P, L, cx, cy, W, pc[k], du, dv, Jm, d);
        else        y[k] = tv ? rhs3_jac_plain<false, true>(P, L, cx, cy, W, 0.0, du, dv, Jm, d)
                              : rhs3_jac_plain<false, false>(P, L, cx, cy, W, 0.0, du, dv, Jm, d);
        for (int q = 0; q < 9; q++) J[9 * k + q] = Jm[q];
        dT[3 * k] = d.lne; dT[3 * k + 1] = d.cx; dT[3 * k + 2] = d.cy;
    }
}

template <bool FAST, bool METRIC>
static void jvp_one(const KParams &P, const double *z, const WindD &W, double pc, double du, double dv, double *J, double *dT)
{
    Seed5 seeds[4];
    Vec3 dfs[4];
    seeds[0] = {1.0, 0.0, 0.0, 0.0, 0.0};
    seeds[1] = {0.0, 1.0, 0.0, 0.0, 0.0};
    seeds[2] = {0.0, 0.0, 1.0, 0.0, 0.0};
    seeds[3] = {0.0, 0.0, 0.0, du, dv};
    rhs3_jvp<FAST, METRIC, 4>(P, z[0], z[1], z[2], W, pc, seeds, dfs);
    for (int c = 0; c < 3; c++) { J[c] = dfs[c].lne; J[3 + c] = dfs[c].cx; J[6 + c] = dfs[c].cy; }
    dT[0] = dfs[3].lne; dT[1] = dfs[3].cx; dT[2] = dfs[3].cy;
}

API void stiff_jvp(const picles_phys *p, int32_t fast, int32_t metric, int64_t n, const double *z3, const double *uv, const double *pc,
                   const double *duv, double *J, double *dT)
{
    KParams P;
    host_params(p, nullptr, P);
    for (int64_t k = 0; k < n; k++) {
        WindD W;
        wind_of(P, uv[2 * k], uv[2 * k + 1], W);
        const double *z = z3 + 3 * k, du = duv[2 * k], dv = duv[2 * k + 1];
        if (fast) { if (metric) jvp_one<true, true>(P, z, W, pc[k], du, dv, J + 9 * k, dT + 3 * k); else jvp_one<true, false>(P, z, W, 0.0, du, dv, J + 9 * k, dT + 3 * k); }
        else      { if (metric) jvp_one<false, true>(P, z, W, pc[k], du, dv, J + 9 * k, dT + 3 * k); else jvp_one<false, false>(P, z, W, 0.0, du, dv, J + 9 * k, dT + 3 * k); }
    }
}

static Wind wind_in(const double *w)
{
    Wind o;
    o.u0 = w[0]; o.v0 = w[1]; o.du = w[2]; o.dv = w[3]; o.bu = w[4]; o.bv = w[5]; o.xi = 0;
    return o;
}

// the integrator's own preamble (integrate_dp5): the wind at t and f0 = f(z, t)
template <bool FAST, bool STATIC, bool METRIC>
static void start_of(const KParams &P, const Wind &w, const double *z, double pc, double t, WindD &W, Vec3 &f0)
{
    W.sh = PM_EXP_SHIFTER();
    if (STATIC) wind_derive(P, w.u0, w.v0, W);
    else wind_stage<false, (!FAST && !STATIC)>(P, w, t, W);
    rhs3<FAST, METRIC>(P, z[0], z[1], z[2], W, f0, pc);
}

template <bool FAST, bool STATIC, bool METRIC>
static void ros_one(const KParams &P, const Wind &w, const double *z, double t, double h, double ipx, double ipy, double pc, double *un,
                    double *f2, double *ee2, double *eig)
{
    WindD W;
    Vec3 f0, F2;
    start_of<FAST, STATIC, METRIC>(P, w, z, pc, t, W, f0);
    const Vec5 z5 = {z[0], z[1], z[2], z[3], z[4]};
    Vec5 U;
    PStats st = {0, 0, 0, 0};
    *ee2 = ros23_try<FAST, STATIC, METRIC>(P, w, W, z5, f0, t, h, ipx, ipy, pc, U, F2, *eig, st);
    un[0] = U.lne; un[1] = U.cx; un[2] = U.cy; un[3] = U.x; un[4] = U.y;
    f2[0] = F2.lne; f2[1] = F2.cx; f2[2] = F2.cy;
}

// variant: 0 <true, true, false>, 1 <true, false, false>, 2 <true, false, true>, 3 <false, false, false>.  pc is read by variant 2 only.
API int32_t stiff_ros23(const picles_phys *p, const picles_ode *o, int32_t variant, int64_t n, const double *z5, const double *wind,
                        const double *win, const double *t, const double *h, const double *ipx, const double *ipy, const double *pc,
                        double *un, double *f2, double *ee2, double *eig)
{
    if (variant < 0 || variant > 3) return -1;
    KParams P;
    host_params(p, nullptr, P);
    host_params_ode(o, P);
    for (int64_t k = 0; k < n; k++) {
        host_params_window(win[3 * k], win[3 * k + 1], win[3 * k + 2], P);
        const Wind w = wind_in(wind + 6 * k);
        const double *z = z5 + 5 * k;
        switch (variant) {
        case 0: ros_one<true, true, false>(P, w, z, t[k], h[k], ipx[k], ipy[k], 0.0, un + 5 * k, f2 + 3 * k, ee2 + k, eig + k); break;
        case 1: ros_one<true, false, false>(P, w, z, t[k], h[k], ipx[k], ipy[k], 0.0, un + 5 * k, f2 + 3 * k, ee2 + k, eig + k); break;
        case 2: ros_one<true, false, true>(P, w, z, t[k], h[k], ipx[k], ipy[k], pc[k], un + 5 * k, f2 + 3 * k, ee2 + k, eig + k); break;
        default: ros_one<false, false, false>(P, w, z, t[k], h[k], ipx[k], ipy[k], 0.0, un + 5 * k, f2 + 3 * k, ee2 + k, eig + k); break;
        }
    }
    return 0;
}

template <bool STATIC>
static double initdt_one(const KParams &P, const Wind &w, const double *z, double t, double ipx, double ipy)
{
    WindD W;
    Vec3 f0;
    start_of<true, STATIC, false>(P, w, z, 0.0, t, W, f0);
    const Vec5 z5 = {z[0], z[1], z[2], z[3], z[4]};
    PStats st = {0, 0, 0, 0};
    return init_dt<true, STATIC, false>(P, w, W, z5, f0, z[1] * ipx, z[2] * ipy, ipx, ipy, 0.0, t, st);
}

// is_static: 1 init_dt<true, true, false>, 0 init_dt<true, false, false>
API void stiff_init_dt(const picles_phys *p, const picles_ode *o, int32_t is_static, int64_t n, const double *z5, const double *wind,
                       const double *win, const double *t, const double *ipx, const double *ipy, double *dt)
{
    KParams P;
    host_params(p, nullptr, P);
    host_params_ode(o, P);
    for (int64_t k = 0; k < n; k++) {
        host_params_window(win[3 * k], win[3 * k + 1], win[3 * k + 2], P);
        const Wind w = wind_in(wind + 6 * k);
        dt[k] = is_static ? initdt_one<true>(P, w, z5 + 5 * k, t[k], ipx[k], ipy[k]) : initdt_one<false>(P, w, z5 + 5 * k, t[k], ipx[k], ipy[k]);
    }
}

// init_dt<true, true, false> with f0 GIVEN (the early exits: a vanishing or a NaN tendency cannot be had from the RHS itself)
API void stiff_init_dt_f0(const picles_phys *p, const picles_ode *o, int64_t n, const double *z5, const double *uv, const double *f0,
                          const double *ipx, const double *ipy, double *dt)
{
    KParams P;
    host_params(p, nullptr, P);
    host_params_ode(o, P);
    for (int64_t k = 0; k < n; k++) {
        WindD W;
        wind_of(P, uv[2 * k], uv[2 * k + 1], W);
        Wind w = {uv[2 * k], uv[2 * k + 1], 0.0, 0.0, 0.0, 0.0, 0};
        const double *z = z5 + 5 * k;
        const Vec5 u0 = {z[0], z[1], z[2], z[3], z[4]};
        const Vec3 k1 = {f0[5 * k], f0[5 * k + 1], f0[5 * k + 2]};
        PStats st = {0, 0, 0, 0};
        dt[k] = init_dt<true, true, false>(P, w, W, u0, k1, f0[5 * k + 3], f0[5 * k + 4], ipx[k], ipy[k], 0.0, 0.0, st);
    }
}
