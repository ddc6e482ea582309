// Device-vs-host bit comparison of the Rosenbrock23 attempt (physics.h ros23_try, four instantiations) and of the initial step (init_dt,
// two): built and run by tests/test_gpu_stiff.py.  The same eval function is compiled for both sides.  What the whole-step parity tests
// cannot aim at is the WAVE-uniform branches — PM_WAVE_ALL around the forward-mode Jacobian, the `mine` selection, 1/det, pm_exp_sat and
// W.ymaxw: the host decides them per state, the device per wave of 64 — so the states are ordered by wave (category = wave index mod 8):
//   0 all plain   1 all non-plain (|c̄| under the speed floor)   2 / 3 exactly one non-plain lane, lane 0 / lane 63
//   4 plain, every fifth lane with |det W| beyond 1e290   5 plain, lane 17 with e² under pm_exp_sat's floor
//   6 plain, one lane under a wind that is not plain (none at all at lane 0, or 150 m/s at lane 63)   7 plain and non-plain at random
// and a last wave of 37 live lanes, its last lane non-plain.  `--host-only` stops after laying the states out and checking the layout.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "physics.h"

struct In { double z[5], w[6], t, h, ipx, ipy, pc; };
struct Out { double un[5], f2[3], ee2, eig; };

// VAR 0..3: ros23_try <true,true,false> <true,false,false> <true,false,true> <false,false,false>; 4, 5: init_dt <true,true,false> <true,false,false>
template <int VAR>
PM_HD void eval(const KParams &P, const In &a, Out &o)
{
    constexpr bool FAST = VAR != 3, STATIC = VAR == 0 || VAR == 4, METRIC = VAR == 2, POLY = !FAST && !STATIC;
    Wind w;
    w.u0 = a.w[0]; w.v0 = a.w[1]; w.du = a.w[2]; w.dv = a.w[3]; w.bu = a.w[4]; w.bv = a.w[5]; w.xi = 0;
    const Vec5 z = {a.z[0], a.z[1], a.z[2], a.z[3], a.z[4]};
    const double pc = METRIC ? a.pc : 0.0;
    WindD W;
    W.sh = PM_EXP_SHIFTER();
    if (STATIC) wind_derive(P, w.u0, w.v0, W);
    else wind_stage<false, POLY>(P, w, a.t, W);
    Vec3 f0;
    rhs3<FAST, METRIC>(P, z.lne, z.cx, z.cy, W, f0, pc);
    PStats st = {0, 0, 0, 0};
    if (VAR < 4) {
        Vec5 un;
        Vec3 f2;
        double eig;
        o.ee2 = ros23_try<FAST, STATIC, METRIC>(P, w, W, z, f0, a.t, a.h, a.ipx, a.ipy, pc, un, f2, eig, st);
        o.un[0] = un.lne; o.un[1] = un.cx; o.un[2] = un.cy; o.un[3] = un.x; o.un[4] = un.y;
        o.f2[0] = f2.lne; o.f2[1] = f2.cx; o.f2[2] = f2.cy;
        o.eig = eig;
    } else {
        o.ee2 = init_dt<FAST, STATIC, METRIC>(P, w, W, z, f0, z.cx * a.ipx, z.cy * a.ipy, a.ipx, a.ipy, pc, a.t, st);
        o.eig = (double)st.rhs;
    }
}

// KParams is the FIRST argument: the rare paths read it afresh from the kernarg segment (physics.h ros_params)
template <int VAR>
__global__ void k_eval(KParams P, int64_t n, const In *in, Out *out)
{
    pm_device_init();
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) eval<VAR>(P, in[i], out[i]);
}

static void host_eval(int var, const KParams &P, const In &a, Out &o)
{
    switch (var) {
    case 0: eval<0>(P, a, o); break;
    case 1: eval<1>(P, a, o); break;
    case 2: eval<2>(P, a, o); break;
    case 3: eval<3>(P, a, o); break;
    case 4: eval<4>(P, a, o); break;
    default: eval<5>(P, a, o); break;
    }
}

// det (I - h d J) of the attempt's W, as ros23_try forms it (the layout check of category 4)
PM_HD double det_of(const KParams &P, const In &a)
{
    WindD W;
    W.sh = PM_EXP_SHIFTER();
    wind_derive(P, a.w[0], a.w[1], W);
    double J[9];
    Vec3 dT;
    rhs3_jac_plain<false, false>(P, a.z[0], a.z[1], a.z[2], W, 0.0, 0.0, 0.0, J, dT);
    const double g = a.h * ROS_D;
    double M[9];
    for (int k = 0; k < 9; k++) M[k] = ((k % 4 == 0) ? 1.0 : 0.0) - g * J[k];
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

static bool state_plain(const KParams &P, const In &a)
{
    const double U2 = a.w[0] * a.w[0] + a.w[1] * a.w[1], c2 = a.z[1] * a.z[1] + a.z[2] * a.z[2];
    return wind_is_plain(P, U2, (0.25 * U2) * P.rg2) && 1.0 / std::sqrt(c2) <= P.ymax * (1.0 - 1e-9);
}

static void window(KParams &P, int form)      // 0 static, 1 parabola, 2 one knot at mid-window (WindWindow::publish)
{
    const bool knot = form == 2;
    P.wind_static = form == 0;
    P.tw0 = 1000.0;
    P.inv_dtw = form == 0 ? 0.0 : 1.0 / 600.0;
    P.wind_sk = knot ? 0.5 : 0.0;
    P.wind_isk = knot ? 1.0 / P.wind_sk : 0.0;
    P.wind_i1sk = knot ? 1.0 / (1.0 - P.wind_sk) : 0.0;
    P.wind_nk = knot ? 1 : 0;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char **argv)
{
    const bool host_only = argc > 1 && !strcmp(argv[1], "--host-only");
    KParams P;
    memset(&P, 0, sizeof(P));
    P.r_g = 0.85; P.inv_rg = 1.0 / P.r_g; P.C_alpha = -1.41; P.C_phi = 0.04; P.C_e = 2.16e-4;
    P.p = 0.75; P.n = 2.0; P.neg2p = -1.5; P.inv_eT = 1.0 / 0.6;
    P.propagation = P.input = P.dissipation = P.peak_shift = P.direction = P.n_is_2 = P.p_is_075 = P.fast_phys = 1;
    {
        const double k1 = 0.25 * PK_G0, k2 = k1 * k1, K = k2 * k2;
        const double i2 = P.inv_eT * P.inv_eT;
        P.inv_eT4 = i2 * i2; P.half_inv_rg = 0.5 * P.inv_rg; P.two_inv_rg2 = 2.0 * (P.inv_rg * P.inv_rg);
        P.KeT4 = K * P.inv_eT4; P.KrCa = (K * P.r_g) * P.C_alpha; P.Cdir = P.C_phi * P.two_inv_rg2;
        P.rg2 = P.r_g * P.r_g;
        const double rg4 = P.rg2 * P.rg2, rg8 = rg4 * rg4;
        P.Cw = (0.5 * PK_G0) * P.r_g; P.Chrh = -0.25 * P.r_g; P.ymax = 10.0 / P.r_g; P.sgmax = 1e8 / P.rg2;
        P.KeT4y = P.KeT4 * rg8; P.KrCay = P.KrCa * rg8; P.Cs = (0.5 * P.C_phi) * P.rg2; P.Cdir2 = 2.0 * P.C_phi;
        P.g4rg2 = k1 * P.rg2; P.qU2r_max = 249999.0 / (P.ymax * P.ymax);
    }
    P.abstol = 1e-4; P.reltol = 1e-3; P.inv_abstol = 1.0 / P.abstol; P.dt0 = 1e-3; P.dtmin = 1e-4; P.maxiters = 10000; P.force_dtmin = 1;
    P.solver = 2;

    const int64_t WAVES = 256, N = 64 * WAVES + 37;
    std::mt19937_64 g(20261021);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    std::vector<In> in(N);
    int64_t n_huge = 0;
    for (int64_t i = 0; i < N; i++) {
        In &a = in[i];
        const int64_t wv = i / 64, lane = i % 64;
        const int cat = wv < WAVES ? (int)(wv % 8) : 8;
        bool floored = false, calm = false, gale = false, huge = false, faint = false;
        switch (cat) {
        case 1: floored = true; break;
        case 2: floored = lane == 0; break;
        case 3: floored = lane == 63; break;
        case 4: huge = lane % 5 == 2; break;
        case 5: faint = lane == 17; break;
        case 6: calm = (wv % 16 == 6) && lane == 0; gale = (wv % 16 == 14) && lane == 63; break;
        case 7: floored = (g() & 1) != 0; break;
        case 8: floored = lane == 36; break;
        default: break;
        }
        // seas whose growth over the attempt stays of order one: |c̄| from 1 m/s, or under the speed floor with a wind of α <= 2
        const double c = floored ? 0.01 + 0.07 * u01(g) : (huge ? 3.0 + u01(g) : 1.0 + 11.0 * u01(g)), th = 6.283185307179586 * u01(g);
        double U = floored ? 0.02 + (4.0 * c / P.r_g - 0.02) * u01(g) : 1.0 + 24.0 * u01(g);
        const double tw = th + 2.0 * (u01(g) - 0.5) * ((g() & 3) ? 0.6 : 3.0);
        if (calm) U = 0.0;
        if (gale) U = 150.0;
        a.z[0] = floored ? -20.0 + 12.0 * u01(g) : -18.0 + 21.0 * u01(g);
        if (!floored) a.z[0] = std::fmin(a.z[0], -5.75 + 4.0 * std::log(c));      // steepness e k_p² <= 1e-2: a sea that exists
        if (faint) a.z[0] = -400.0;
        a.z[1] = c * std::cos(th); a.z[2] = c * std::sin(th);
        a.z[3] = (0.05 + 0.9 * u01(g)) * ((g() & 1) ? 1.0 : -1.0); a.z[4] = (0.05 + 0.9 * u01(g)) * ((g() & 1) ? 1.0 : -1.0);
        a.h = std::exp(std::log(0.1) + std::log(300.0) * u01(g));
        a.t = 1300.0 - (0.1 + 0.8 * u01(g)) * a.h;         // the knot of the knot window (t = 1300) lies inside (t, t + h)
        a.ipx = (2e-4 + 1.8e-3 * u01(g)) * ((g() & 1) ? 1.0 : -1.0); a.ipy = 2e-4 + 1.8e-3 * u01(g);
        a.pc = (2e-7 + 1.8e-6 * u01(g)) * ((g() & 1) ? 1.0 : -1.0);
        // the window's wind: level 0 such that the parabola passes near (U, tw) at mid-window; slopes of a few m/s over the window
        const bool still = calm || gale;
        a.w[2] = still ? 0.0 : 6.0 * (u01(g) - 0.5); a.w[3] = still ? 0.0 : 6.0 * (u01(g) - 0.5);
        a.w[4] = still ? 0.0 : 4.0 * (u01(g) - 0.5); a.w[5] = still ? 0.0 : 4.0 * (u01(g) - 0.5);
        a.w[0] = U * std::cos(tw); a.w[1] = U * std::sin(tw);
        if (floored)      // under the speed floor a breeze is a gale (α = U / 2 c_gp): the window's changes scale with the wind
            for (int k = 2; k < 6; k++) a.w[k] *= 0.1 * U;
        if (huge) {
            // ln e such that |det W| lands near 1e297: det grows like e^(6 ln e) (three rows ∝ e²)
            a.h = 1.0; a.t = 1299.5;
            double lo = 20.0, hi = 130.0;
            for (int it = 0; it < 60; it++) {
                a.z[0] = 0.5 * (lo + hi);
                const double d = std::fabs(det_of(P, a));
                if (d == d && d < 1e297) lo = a.z[0]; else hi = a.z[0];
            }
            a.z[0] = lo;
            n_huge++;
        }
    }
    // the layout is what the head of this file says (host side): counted on the static window's wind
    {
        int64_t all_plain = 0, none_plain = 0, one0 = 0, one63 = 0, det_mixed = 0, sat = 0, windy = 0;
        window(P, 0);
        for (int64_t wv = 0; wv < WAVES; wv++) {
            int np = 0, big = 0, ord = 0, faint = 0, wnp = 0;
            for (int l = 0; l < 64; l++) {
                const In &a = in[64 * wv + l];
                np += !state_plain(P, a);
                const double d = std::fabs(det_of(P, a)), U2 = a.w[0] * a.w[0] + a.w[1] * a.w[1];
                big += d > 1e290 && d < 1e306; ord += d >= 1e-290 && d <= 1e290;
                faint += a.z[0] < -350.0;
                wnp += !wind_is_plain(P, U2, (0.25 * U2) * P.rg2);
            }
            all_plain += np == 0; none_plain += np == 64;
            one0 += np == 1 && !state_plain(P, in[64 * wv]); one63 += np == 1 && !state_plain(P, in[64 * wv + 63]);
            det_mixed += big >= 8 && ord >= 32 && big + ord == 64;
            sat += faint == 1; windy += wnp == 1;
        }
        printf("layout: %lld waves all plain, %lld all non-plain, %lld / %lld with one non-plain lane at 0 / 63, %lld mixing |det| > 1e290 with "
               "ordinary ones, %lld with one lane under the floor of e², %lld with one wind that is not plain; last wave %lld lanes\n",
               (long long)all_plain, (long long)none_plain, (long long)one0, (long long)one63, (long long)det_mixed, (long long)sat,
               (long long)windy, (long long)(N - 64 * WAVES));
        if (all_plain < 32 || none_plain < 32 || one0 < 32 || one63 < 32 || det_mixed < 32 || sat < 32 || windy < 32 || state_plain(P, in[N - 1])) {
            fprintf(stderr, "the states are not laid out as intended\n");
            return 3;
        }
        // no NaN in what the host computes (a NaN's bits are not comparable across the two sides)
        for (int var = 0; var < 6; var++)
            for (int form = (var == 0 || var == 4) ? 0 : 1; form <= ((var == 0 || var == 4) ? 0 : 2); form++) {
                window(P, form);
                int64_t nans = 0;
                for (int64_t i = 0; i < N; i++) {
                    Out h;
                    memset(&h, 0, sizeof(h));
                    host_eval(var, P, in[i], h);
                    const double *x = (const double *)&h;
                    for (int k = 0; k < 10; k++)
                        if (!(x[k] == x[k]) && nans++ < 4)
                            fprintf(stderr, "state %lld (wave %lld lane %lld) value %d is a NaN: ln e %g |c| %g wind %g %g h %g\n", (long long)i,
                                    (long long)(i / 64), (long long)(i % 64), k, in[i].z[0], std::hypot(in[i].z[1], in[i].z[2]), in[i].w[0], in[i].w[1], in[i].h);
                }
                if (nans) { fprintf(stderr, "variant %d window %d: %lld NaN values on the host\n", var, form, (long long)nans); return 3; }
            }
    }
    if (host_only) return 0;

    In *din; Out *dout;
    CK(hipMalloc(&din, N * sizeof(In))); CK(hipMalloc(&dout, N * sizeof(Out)));
    CK(hipMemcpy(din, in.data(), N * sizeof(In), hipMemcpyHostToDevice));
    std::vector<Out> out(N);
    static const char *names[6] = {"ros23_try<fast,static>", "ros23_try<fast,tvar>", "ros23_try<fast,tvar,metric>", "ros23_try<general,tvar>",
                                   "init_dt<fast,static>", "init_dt<fast,tvar>"};
    int bad_total = 0;
    for (int var = 0; var < 6; var++) {
        const bool stat = var == 0 || var == 4;
        int64_t bad = 0, runs = 0;
        for (int form = stat ? 0 : 1; form <= (stat ? 0 : 2); form++) {      // time-varying flavours: the parabola window, then the knot window
            window(P, form);
            CK(hipMemset(dout, 0, N * sizeof(Out)));
            dim3 grid((unsigned)((N + 255) / 256)), block(256);
            switch (var) {
            case 0: hipLaunchKernelGGL((k_eval<0>), grid, block, 0, 0, P, N, din, dout); break;
            case 1: hipLaunchKernelGGL((k_eval<1>), grid, block, 0, 0, P, N, din, dout); break;
            case 2: hipLaunchKernelGGL((k_eval<2>), grid, block, 0, 0, P, N, din, dout); break;
            case 3: hipLaunchKernelGGL((k_eval<3>), grid, block, 0, 0, P, N, din, dout); break;
            case 4: hipLaunchKernelGGL((k_eval<4>), grid, block, 0, 0, P, N, din, dout); break;
            default: hipLaunchKernelGGL((k_eval<5>), grid, block, 0, 0, P, N, din, dout); break;
            }
            CK(hipGetLastError());
            CK(hipMemcpy(out.data(), dout, N * sizeof(Out), hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < N; i++) {
                Out h;
                memset(&h, 0, sizeof(h));
                host_eval(var, P, in[i], h);
                if (memcmp(&h, &out[i], sizeof(Out)) != 0) {
                    if (bad < 3) {
                        const double *x = (const double *)&h, *y = (const double *)&out[i];
                        for (int k = 0; k < 10; k++)
                            if (memcmp(&x[k], &y[k], 8))
                                fprintf(stderr, "%s window %d state %lld (wave %lld lane %lld) value %d: host %a device %a\n", names[var], form,
                                        (long long)i, (long long)(i / 64), (long long)(i % 64), k, x[k], y[k]);
                    }
                    bad++;
                }
            }
            runs++;
        }
        printf("%s %lld states x %lld windows, %lld mismatches\n", names[var], (long long)N, (long long)runs, (long long)bad);
        bad_total += bad != 0;
    }
    (void)hipFree(din); (void)hipFree(dout);
    return bad_total ? 1 : 0;
}
