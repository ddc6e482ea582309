// Device-vs-host bit comparison of whole integrations over one DT by integrate_dp5 (physics.h): built and run by
// tests/test_gpu_explicit.py.  The same eval function is compiled for both sides; tests/test_explicit_reference.py holds the host
// build against the 60-digit reference and against the oracle.  What the whole-step parity tests cannot aim at is how the device
// decides per WAVE what the host decides per state — lane-divergent loop exits, the divergent Rosenbrock23 / Tsit5 branches of the
// auto-switching flavour — and the two forms of table access (TABS = true: scalar loads; false: LDS behind dp_device_init).  So the
// states are ordered by wave (category = wave index mod 8):
//   0 one state in every lane: all lanes take the same attempts      1 the same, but one lane alone enters with dtn = DT and rejects
//   2 dtn spread over three decades across the lanes: very different attempt counts
//   3 / 4 only lane 0 / only lane 63 enters with Rosenbrock23 active, the rest with Tsit5
//   5 every second lane enters with its counter at 10 on a sea where the next test is positive: the counter crosses inside the integration
//   6 states, dtn (init_dt among them), controller memory and switch state at random      7 as 0, the first step from init_dt
// and a last wave of 37 live lanes.  maxiters is modest (no lane can run long; a lane that meets it carries the flag on both sides).
// `--host-only` stops after laying the states out and checking the layout.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "physics.h"

struct In { double z[5], w[6], lq, dtn, m11, m22, pc; int asw, pad; };
struct Out { double z[5], lq, dtn; int asw, status; unsigned int rhs, acc, rej, pad; };

static constexpr double T_START = 1000.0, DT_STEP = 600.0;
static constexpr int N_VAR = 7;
// VAR: 0 DP5 fast/static, scalar-load tables   1 the same through LDS   2 Tsit5 fast/time-varying   3 AUTO fast/static, scalar loads
//      4 the same through LDS   5 the general flavour of k_bforce <false, false, ·, TSIT, AUTO, false>   6 Tsit5 fast/time-varying/metric
template <int VAR>
struct Flavour {
    static constexpr bool FAST = VAR != 5, STATIC = VAR == 0 || VAR == 1 || VAR == 3 || VAR == 4, METRIC = VAR == 6;
    static constexpr bool TSIT = VAR >= 2, AUTO = VAR == 3 || VAR == 4 || VAR == 5, TABS = VAR == 0 || VAR == 2 || VAR == 3 || VAR == 6;
};
static const char *const names[N_VAR] = {"DP5<fast,static,scalar tables>", "DP5<fast,static,LDS tables>", "Tsit5<fast,tvar> parabola",
                                         "AUTO<fast,static,scalar tables>", "AUTO<fast,static,LDS tables>", "AUTO<general,tvar,LDS tables> knot",
                                         "Tsit5<fast,tvar,metric> parabola"};
static const int window_of[N_VAR] = {0, 0, 1, 0, 0, 2, 1};

template <int VAR>
PM_HD void eval(const KParams &P, const In &a, Out &o)
{
    typedef Flavour<VAR> F;
    Wind w;
    w.u0 = a.w[0]; w.v0 = a.w[1]; w.du = a.w[2]; w.dv = a.w[3]; w.bu = a.w[4]; w.bv = a.w[5]; w.xi = 0;
    Vec5 z = {a.z[0], a.z[1], a.z[2], a.z[3], a.z[4]};
    double lq = a.lq, dtn = a.dtn;
    int asw = a.asw;
    PStats st = {0, 0, 0, 0};
    integrate_dp5<F::FAST, F::STATIC, F::METRIC, F::TSIT, F::AUTO, F::TABS>(P, w, z, lq, dtn, T_START, DT_STEP, st, a.m11, a.m22, a.pc, &asw);
    o.z[0] = z.lne; o.z[1] = z.cx; o.z[2] = z.cy; o.z[3] = z.x; o.z[4] = z.y;
    o.lq = lq; o.dtn = dtn; o.asw = F::AUTO ? asw : 0; o.status = st.status;
    o.rhs = st.rhs; o.acc = st.acc; o.rej = st.rej; o.pad = 0;
}

// KParams is the FIRST argument: the rare paths read it afresh from the kernarg segment (physics.h ros_params); 256 threads per
// workgroup (pm_device_init), every one of them through both table initialisations before the bounds test
template <int VAR>
__global__ void __launch_bounds__(256) k_eval(KParams P, int64_t n, const In *in, Out *out)
{
    dp_device_init(Flavour<VAR>::TSIT ? 1 : 0);
    pm_device_init();
    int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
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
    case 5: eval<5>(P, a, o); break;
    default: eval<6>(P, a, o); break;
    }
}

static void window(KParams &P, int form)      // 0 static, 1 parabola, 2 one knot at mid-window (WindWindow::publish)
{
    const bool knot = form == 2;
    P.wind_static = form == 0;
    P.tw0 = T_START;
    P.inv_dtw = form == 0 ? 0.0 : 1.0 / DT_STEP;
    P.wind_sk = knot ? 0.5 : 0.0;
    P.wind_isk = knot ? 1.0 / P.wind_sk : 0.0;
    P.wind_i1sk = knot ? 1.0 / (1.0 - P.wind_sk) : 0.0;
    P.wind_nk = knot ? 1 : 0;
}

static int enc(int count, int stiff) { return (int)((unsigned int)count << 1) | stiff; }

static bool same(const Out &h, const Out &d)
{
    return !memcmp(h.z, d.z, sizeof h.z) && !memcmp(&h.lq, &d.lq, 8) && !memcmp(&h.dtn, &d.dtn, 8) && h.asw == d.asw && h.status == d.status &&
           h.rhs == d.rhs && h.acc == d.acc && h.rej == d.rej;
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
    P.abstol = 1e-4; P.reltol = 1e-3; P.inv_abstol = 1.0 / P.abstol; P.dt0 = 1e-3; P.dtmin = 1e-4; P.force_dtmin = 1;
    P.maxiters = 80;      // modest: no lane can run long
    P.solver = 2;
    P.inv_dx = 1.0 / 2000.0; P.inv_dy = 1.0 / 2500.0;

    const int64_t WAVES = 64, N = 64 * WAVES + 37;
    std::mt19937_64 g(20261024);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    std::vector<In> in(N);
    const double ln_floor = PI_LNQOLDINIT;
    // a state: a sea that exists (steepness e k_p² <= 1e-2) under a wind of 1 … 25 m/s within ±0.6 rad of it (three in four) or anywhere
    auto state = [&](In &a) {
        const double c = 1.0 + 11.0 * u01(g), th = 6.283185307179586 * u01(g);
        const double U = 1.0 + 24.0 * u01(g);
        const double tw = th + 2.0 * (u01(g) - 0.5) * ((g() & 3) ? 0.6 : 3.0);
        a.z[0] = -18.0 + 21.0 * u01(g);
        a.z[0] = std::fmin(a.z[0], -5.75 + 4.0 * std::log(c));
        a.z[1] = c * std::cos(th); a.z[2] = c * std::sin(th);
        a.z[3] = (0.05 + 0.9 * u01(g)) * ((g() & 1) ? 1.0 : -1.0); a.z[4] = (0.05 + 0.9 * u01(g)) * ((g() & 1) ? 1.0 : -1.0);
        a.w[0] = U * std::cos(tw); a.w[1] = U * std::sin(tw);
        a.w[2] = 6.0 * (u01(g) - 0.5); a.w[3] = 6.0 * (u01(g) - 0.5); a.w[4] = 4.0 * (u01(g) - 0.5); a.w[5] = 4.0 * (u01(g) - 0.5);
        a.m11 = (2e-4 + 1.8e-3 * u01(g)) * ((g() & 1) ? 1.0 : -1.0); a.m22 = 2e-4 + 1.8e-3 * u01(g);
        a.pc = (2e-7 + 1.8e-6 * u01(g)) * ((g() & 1) ? 1.0 : -1.0);
        a.lq = ln_floor; a.dtn = 5.0; a.asw = 0; a.pad = 0;
    };
    for (int64_t wv = 0; wv <= WAVES; wv++) {
        const int cat = wv < WAVES ? (int)(wv % 8) : 8;
        const int lanes = wv < WAVES ? 64 : 37;
        In base;
        state(base);
        const int lone = (int)(g() % 64);
        window(P, 0);
        if (cat == 1)      // a state that DP5 integrates from dtn = 5 s without a rejection, and from dtn = DT with one
            for (int tries = 0; tries < 400; tries++) {
                In big = base;
                big.dtn = DT_STEP;
                Out calm, rough;
                host_eval(0, P, base, calm);
                host_eval(0, P, big, rough);
                if (calm.rej == 0 && rough.rej > 0) break;
                state(base);
            }
        for (int l = 0; l < lanes; l++) {
            In &a = in[64 * wv + l];
            switch (cat) {
            case 0: a = base; break;
            case 1: a = base; if (l == lone) a.dtn = DT_STEP; break;
            case 2: state(a); a.dtn = 0.6 * std::pow(10.0, 3.0 * l / 63.0); break;
            case 3: state(a); a.asw = enc(0, l == 0); break;
            case 4: state(a); a.asw = enc(0, l == 63); break;
            case 5:      // odd lanes: a sea on which the first AutoSwitch test, counter at 10 and a step of two minutes, hands over to Rosenbrock23
                for (int tries = 0; tries < 400; tries++) {
                    state(a);
                    a.asw = enc((l & 1) ? 10 : 0, 0); a.dtn = 120.0;
                    Out o;
                    host_eval(3, P, a, o);
                    if (!(l & 1) || (o.asw & 1)) break;
                }
                break;
            case 7: a = base; a.dtn = -1.0; a.asw = ASW_FRESH; break;
            default:
                state(a);
                a.dtn = (g() & 3) ? std::exp(std::log(0.05) + std::log(1e4) * u01(g)) : -1.0;
                a.lq = ln_floor + (0.0 - ln_floor) * u01(g);
                { const int pick = (int)(g() % 5); a.asw = pick == 0 ? ASW_FRESH : pick == 1 ? 0 : pick == 2 ? enc(5, 0) : pick == 3 ? enc(-2, 1) : enc(9, 0); }
                break;
            }
        }
    }
    // the layout is what the head of this file says (host side), and the host computes no NaN (whose bits are not comparable)
    std::vector<std::vector<Out>> host(N_VAR, std::vector<Out>(N));
    for (int var = 0; var < N_VAR; var++) {
        window(P, window_of[var]);
        int64_t nans = 0;
        for (int64_t i = 0; i < N; i++) {
            memset(&host[var][i], 0, sizeof(Out));
            host_eval(var, P, in[i], host[var][i]);
            const Out &h = host[var][i];
            for (int k = 0; k < 7; k++) nans += !((&h.z[0])[k] == (&h.z[0])[k]);
        }
        if (nans) { fprintf(stderr, "%s: %lld NaN values on the host\n", names[var], (long long)nans); return 3; }
    }
    {
        int64_t uniform = 0, lone_rej = 0, spread = 0, ros0 = 0, ros63 = 0, crossing = 0, maxit = 0;
        for (int64_t wv = 0; wv < WAVES; wv++) {
            const Out *t5 = &host[2][64 * wv], *d5 = &host[0][64 * wv], *au = &host[3][64 * wv];
            const In *a = &in[64 * wv];
            bool uni = true;
            int rejecting = 0, amin = 1 << 30, amax = 0, stiff_in = 0, crossed = 0;
            for (int l = 0; l < 64; l++) {
                uni = uni && same(d5[l], d5[0]) && same(t5[l], t5[0]) && same(au[l], au[0]);
                rejecting += d5[l].rej > 0;
                const int att = (int)(t5[l].acc + t5[l].rej);
                amin = att < amin ? att : amin; amax = att > amax ? att : amax;
                stiff_in += (a[l].asw != ASW_FRESH) && (a[l].asw & 1);
                crossed += !(a[l].asw & 1) && (au[l].asw & 1) && (a[l].asw >> 1) == 10;
                maxit += (au[l].status & 2) != 0;
            }
            switch (wv % 8) {
            case 0: case 7: uniform += uni; break;
            case 1: lone_rej += rejecting == 1; break;
            case 2: spread += amax >= amin + 3; break;
            case 3: ros0 += stiff_in == 1 && (a[0].asw & 1); break;
            case 4: ros63 += stiff_in == 1 && (a[63].asw & 1); break;
            case 5: crossing += crossed >= 4 && crossed < 64; break;
            default: break;
            }
        }
        printf("layout: %lld waves with one state in every lane, %lld where one lane alone rejects, %lld with attempt counts spread by 3 or more, "
               "%lld / %lld with Rosenbrock23 active in lane 0 / 63 alone, %lld where some lanes' counters cross 10 inside the integration; "
               "%lld lanes meet maxiters; last wave %lld lanes\n", (long long)uniform, (long long)lone_rej, (long long)spread, (long long)ros0,
               (long long)ros63, (long long)crossing, (long long)maxit, (long long)(N - 64 * WAVES));
        if (uniform < 16 || lone_rej < 6 || spread < 8 || ros0 < 8 || ros63 < 8 || crossing < 4) {
            fprintf(stderr, "the states are not laid out as intended\n");
            return 3;
        }
    }
    if (host_only) return 0;

    In *din; Out *dout;
    CK(hipMalloc(&din, N * sizeof(In))); CK(hipMalloc(&dout, N * sizeof(Out)));
    CK(hipMemcpy(din, in.data(), N * sizeof(In), hipMemcpyHostToDevice));
    std::vector<Out> out(N);
    int bad_total = 0;
    for (int var = 0; var < N_VAR; var++) {
        window(P, window_of[var]);
        CK(hipMemset(dout, 0, N * sizeof(Out)));
        dim3 grid((unsigned)((N + 255) / 256)), block(256);
        switch (var) {
        case 0: hipLaunchKernelGGL((k_eval<0>), grid, block, 0, 0, P, N, din, dout); break;
        case 1: hipLaunchKernelGGL((k_eval<1>), grid, block, 0, 0, P, N, din, dout); break;
        case 2: hipLaunchKernelGGL((k_eval<2>), grid, block, 0, 0, P, N, din, dout); break;
        case 3: hipLaunchKernelGGL((k_eval<3>), grid, block, 0, 0, P, N, din, dout); break;
        case 4: hipLaunchKernelGGL((k_eval<4>), grid, block, 0, 0, P, N, din, dout); break;
        case 5: hipLaunchKernelGGL((k_eval<5>), grid, block, 0, 0, P, N, din, dout); break;
        default: hipLaunchKernelGGL((k_eval<6>), grid, block, 0, 0, P, N, din, dout); break;
        }
        CK(hipGetLastError());
        CK(hipMemcpy(out.data(), dout, N * sizeof(Out), hipMemcpyDeviceToHost));
        int64_t bad = 0;
        for (int64_t i = 0; i < N; i++) {
            const Out &h = host[var][i], &d = out[i];
            if (!same(h, d)) {
                if (bad < 3)
                    fprintf(stderr, "%s state %lld (wave %lld lane %lld): host z %a %a %a %a %a lq %a dtn %a asw %d status %d rhs %u acc %u rej %u\n"
                            "    device z %a %a %a %a %a lq %a dtn %a asw %d status %d rhs %u acc %u rej %u\n", names[var], (long long)i,
                            (long long)(i / 64), (long long)(i % 64), h.z[0], h.z[1], h.z[2], h.z[3], h.z[4], h.lq, h.dtn, h.asw, h.status, h.rhs, h.acc, h.rej,
                            d.z[0], d.z[1], d.z[2], d.z[3], d.z[4], d.lq, d.dtn, d.asw, d.status, d.rhs, d.acc, d.rej);
                bad++;
            }
        }
        printf("%s %lld states, %lld mismatches\n", names[var], (long long)N, (long long)bad);
        bad_total += bad != 0;
    }
    (void)hipFree(din); (void)hipFree(dout);
    return bad_total ? 1 : 0;
}
