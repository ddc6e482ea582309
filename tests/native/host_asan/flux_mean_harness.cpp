// flux_mean_harness.cpp — the host side of the flux means (picles_flux_mean_*) under AddressSanitizer, on top of fake_hip.cpp like
// flux_harness.cpp: seeded programs of init / shape / update / push / export / get / set / reset / free around steps, for whole-grid,
// slab and lattice contexts, with every buffer handed to picles_flux_mean_get / _set, picles_flux_pop and picles_flux_mean_export
// allocated with exactly the size the shape calls report.  Every refusal of the header is provoked (no flux set, no mean set, a
// second init, every / first < 1, push and export without a sample, a full ring, the wind rule, a NULL plane block), the mean set
// is freed with samples held, dropped with its flux set, and every context is destroyed with whatever mean pushes are still pending.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_flux_mean.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../../include/picles_hip.h"

extern "C" int hipMalloc(void **p, size_t bytes);      /* fake_hip.cpp's (hipError_t is an int-sized enum, 0 = success) */
extern "C" int hipFree(void *p);
extern "C" int hipStreamCreateWithFlags(void **s, unsigned flags);
extern "C" int hipStreamDestroy(void *s);

namespace {
struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t s) : g(s) {}
    int in(int lo, int hi) { return lo + (int)(g() % (uint64_t)(hi - lo + 1)); }
    bool coin() { return g() & 1; }
};
long g_calls = 0, g_refused = 0;
void die(const char *what) { fprintf(stderr, "flux mean harness: %s\n", what); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "flux mean harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, int want, const char *what, const char *text = nullptr)
{
    g_calls++; g_refused++;
    if (rc != want) { fprintf(stderr, "flux mean harness: %s: rc=%d, expected %d (%s)\n", what, rc, want, picles_last_error(c)); exit(3); }
    if (!picles_last_error(c)[0]) { fprintf(stderr, "flux mean harness: %s refused without a text\n", what); exit(3); }
    if (text && !strstr(picles_last_error(c), text)) { fprintf(stderr, "flux mean harness: %s: the text lacks '%s': %s\n", what, text, picles_last_error(c)); exit(3); }
}

struct Shape { size_t field_bytes = 0, acc_bytes = 0; int np = 0; };

int64_t samples(picles_ctx *c)
{
    int64_t n = -1;
    ok(c, picles_flux_mean_get(c, nullptr, &n, nullptr, nullptr), "flux_mean_get (scalars alone)");
    return n;
}

/* get into an exact-size block, then hand the same block back */
void get_set_exact(picles_ctx *c, Rng &R, const Shape &S)
{
    double *a = (double *)malloc(S.acc_bytes);
    int64_t n = -1;
    double t0 = -1.0, t1 = -1.0;
    ok(c, picles_flux_mean_get(c, a, &n, R.coin() ? &t0 : nullptr, R.coin() ? &t1 : nullptr), "flux_mean_get");
    if (n != samples(c)) die("n_samples of get");
    if (R.coin()) {
        refused(c, picles_flux_mean_set(c, nullptr, n, t0, t1), -2, "set without planes", "planes must be given");
        refused(c, picles_flux_mean_set(c, a, -1, t0, t1), -2, "set with n_samples < 0", "n_samples");
        ok(c, picles_flux_mean_set(c, a, n, t0, t1), "flux_mean_set");
        if (samples(c) != n) die("n_samples after set");
    }
    free(a);
}

void pop_exact(picles_ctx *c, Rng &R, const Shape &S)
{
    void *f = malloc(S.field_bytes ? S.field_bytes : 1);
    double *pp = (double *)malloc((size_t)S.np * PICLES_FLUX_NPARTIAL * 8), t = -1.0;
    ok(c, picles_flux_pop(c, f, R.coin() ? pp : nullptr, R.coin() ? &t : nullptr), "flux_pop");
    free(f); free(pp);
}

void export_exact(picles_ctx *c, Rng &R, const Shape &S, int reset)
{
    void *fd = nullptr, *pd = nullptr, *caller = nullptr;
    if (R.coin() && hipStreamCreateWithFlags(&caller, 0) != 0) die("hipStreamCreate");
    if (hipMalloc(&fd, S.field_bytes ? S.field_bytes : 1) != 0 || hipMalloc(&pd, (size_t)S.np * PICLES_FLUX_NPARTIAL * 8) != 0) die("hipMalloc");
    refused(c, picles_flux_mean_export(c, nullptr, (double *)pd, caller, reset), -2, "export without a field buffer", "no device buffer");
    if (samples(c) == 0) refused(c, picles_flux_mean_export(c, fd, (double *)pd, caller, reset), -2, "export without a sample", "holds no sample");
    else {
        ok(c, picles_flux_mean_export(c, fd, R.coin() ? (double *)pd : nullptr, caller, reset), "flux_mean_export");
        if (reset && samples(c) != 0) die("samples after an export with reset");
    }
    hipFree(fd); hipFree(pd);
    if (caller) hipStreamDestroy(caller);
}

void program(uint64_t seed)
{
    Rng R(0xD1B54A32D192ED03ull * (seed + 1));
    const int Nx = R.in(4, 600), Ny = R.in(4, 40);
    picles_grid g; picles_phys p; picles_ode o; picles_model m;
    memset(&g, 0, sizeof g); memset(&p, 0, sizeof p); memset(&o, 0, sizeof o); memset(&m, 0, sizeof m);
    g.Nx = Nx; g.Ny = Ny; g.dx = 2000.0; g.dy = 1500.0; g.periodic_x = 1; g.periodic_y = R.coin();
    const bool slab = R.coin();
    g.j_begin = slab ? R.in(0, Ny - 3) : 0;
    g.j_end = slab ? R.in(g.j_begin + 2, Ny) : Ny;
    p.r_g = 0.85; p.C_alpha = -1.41; p.C_phi = 0.04; p.C_e = 2.2117647058823533e-4; p.g = 9.81; p.gamma = 0.88; p.q = -0.25;
    p.c_beta = 0.04; p.c_D = 2e-3; p.c_e = 1.3e-6; p.c_alpha = 11.8;
    p.propagation = p.input = p.dissipation = p.peak_shift = p.direction = 1;
    o.abstol = 1e-4; o.reltol = 1e-3; o.dt0 = 1e-3; o.dtmin = 1e-4; o.force_dtmin = 1; o.solver = 0; o.maxiters = 10000;
    o.log_energy_minimum = -13.0; o.log_energy_maximum = 3.3; o.wind_min_squared = 4.0; o.timestep = 600.0;
    m.periodic_boundary = 1; m.minimal_state[0] = 1.25e-6; m.minimal_state[1] = 1.28e-9;
    picles_ctx *c = nullptr;
    g_calls++;
    if (picles_create(&g, &p, &o, &m, 0, 1, &c) != 0) { g_refused++; return; }
    const int ny = g.j_end - g.j_begin;
    const size_t N = (size_t)Nx * ny;
    const bool whole = !slab || (g.j_begin == 0 && g.j_end == Ny);
    const bool lattice = R.in(0, 2) == 0;
    std::vector<double> u(N, 9.0), v(N, 4.0), u1(N, 7.0), v1(N, 5.0);
    if (lattice) {
        const double lu[2 * 2 * 3] = {9, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7, 7}, lv[2 * 2 * 3] = {4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6};
        ok(c, picles_set_wind_grid(c, 2, 2, 3, 0.0, 2000.0 * Nx, 0.0, 1500.0 * Ny, 0.0, 1800.0, lu, lv, 0.0, 0.0), "set_wind_grid");
    } else {
        ok(c, picles_set_winds(c, u.data(), v.data(), 0.0, nullptr, nullptr, 0.0), "set_winds");
    }
    ok(c, picles_seed(c, 0.0), "seed");

    /* before the flux set, and before the mean set */
    refused(c, picles_flux_mean_init(c, 1, 1), -2, "mean init without a flux set", "picles_flux_init first");
    refused(c, picles_flux_mean_update(c, nullptr), -2, "update before init", "picles_flux_mean_init first");
    refused(c, picles_flux_mean_push(c, 1), -2, "push before init", "picles_flux_mean_init first");
    refused(c, picles_flux_mean_export(c, &g, nullptr, nullptr, 0), -2, "export before init", "picles_flux_mean_init first");
    refused(c, picles_flux_mean_get(c, nullptr, nullptr, nullptr, nullptr), -2, "get before init", "picles_flux_mean_init first");
    refused(c, picles_flux_mean_set(c, nullptr, 0, 0.0, 0.0), -2, "set before init", "picles_flux_mean_init first");
    refused(c, picles_flux_mean_reset(c), -2, "reset before init", "picles_flux_mean_init first");
    ok(c, picles_flux_mean_free(c), "free without a set");
    if (picles_flux_mean_shape(c, nullptr, nullptr, nullptr) == 0) die("shape before init");

    for (int round = 0; round < 2; round++) {          /* the second round: another flux set, another mean set */
        int cx = R.in(1, 16), cy = R.in(1, 16);
        if (R.in(0, 2) == 0) cx = 1 << R.in(0, 4);      /* the grouped instances as often as the generic one */
        if (g.j_begin % cy != 0) cy = 1;
        const int mask = R.in(1, PICLES_FLUX_ALL), slots = R.in(1, 3);
        ok(c, picles_flux_init(c, cx, cy, mask, 10055.25, 1025.0, slots), "flux_init");
        refused(c, picles_flux_mean_init(c, 0, 1), -2, "every = 0", "every and first");
        refused(c, picles_flux_mean_init(c, 1, 0), -2, "first = 0", "every and first");
        refused(c, picles_flux_mean_init(c, -2, -1), -2, "negative cadence", "every and first");
        if (picles_flux_mean_shape(c, nullptr, nullptr, nullptr) == 0) die("a refused init left a set");
        const int every = R.in(1, 3), first = R.in(1, 3);
        ok(c, picles_flux_mean_init(c, every, first), "flux_mean_init");
        refused(c, picles_flux_mean_init(c, every, first), -2, "init twice", "a mean set exists");
        Shape S;
        int32_t nxc, nyc, nf, ev = 0, npl = 0;
        ok(c, picles_flux_shape(c, &nxc, &nyc, &nf, &S.np, &S.field_bytes), "flux_shape");
        ok(c, picles_flux_mean_shape(c, &ev, &npl, &S.acc_bytes), "flux_mean_shape");
        ok(c, picles_flux_mean_shape(c, nullptr, nullptr, nullptr), "flux_mean_shape (no outputs)");
        if (ev != every || npl != PICLES_FLUX_NPARTIAL || S.acc_bytes != (size_t)88 * nxc * nyc) die("mean shape");
        refused(c, picles_flux_mean_push(c, 0), -2, "push without a sample", "holds no sample");
        export_exact(c, R, S, 0);
        const int nops = R.in(4, 24);
        for (int k = 0; k < nops; k++) {
            switch (R.in(0, 7)) {
            case 0:
                if (whole) {
                    if (R.coin()) ok(c, picles_run_steps(c, 600.0, R.in(1, 4)), "run_steps");
                    else ok(c, picles_time_step(c, 600.0, PICLES_STEP_ZERO_FIRST), "time_step");
                }
                break;
            case 1: {      /* a manual update, on the context stream or on a caller's */
                void *s = nullptr;
                if (R.coin() && hipStreamCreateWithFlags(&s, 0) != 0) die("hipStreamCreate");
                const int64_t n = samples(c);
                ok(c, picles_flux_mean_update(c, s), "flux_mean_update");
                if (samples(c) != n + 1) die("an update counts one sample");
                if (s) { ok(c, picles_sync(c), "sync"); hipStreamDestroy(s); }
            } break;
            case 2:
                if (samples(c) == 0) refused(c, picles_flux_mean_push(c, 1), -2, "push without a sample", "holds no sample");
                else if (picles_flux_pending(c) == slots) refused(c, picles_flux_mean_push(c, 1), -3, "push into a full ring", "ring full");
                else {
                    const int reset = R.coin();
                    const int64_t n = samples(c);
                    ok(c, picles_flux_mean_push(c, reset), "flux_mean_push");
                    if (samples(c) != (reset ? 0 : n)) die("samples after a push");
                }
                break;
            case 3: if (picles_flux_pending(c) > 0) pop_exact(c, R, S); break;
            case 4: export_exact(c, R, S, R.coin()); break;
            case 5: get_set_exact(c, R, S); break;
            case 6:
                if (R.coin()) { ok(c, picles_flux_mean_reset(c), "flux_mean_reset"); if (samples(c) != 0) die("samples after reset"); }
                else if (!lattice) {      /* the wind rule: the clock inside a host-set window */
                    const double t = picles_clock(c);
                    const int64_t n = samples(c);
                    ok(c, picles_set_winds(c, u.data(), v.data(), t, u1.data(), v1.data(), t + 600.0), "set_winds (two levels)");
                    ok(c, picles_tick(c, 100.0), "tick");
                    refused(c, picles_flux_mean_update(c, nullptr), -2, "update inside a host window", "step to a level");
                    if (samples(c) != n) die("a refused update counted");
                    ok(c, picles_tick(c, 500.0), "tick");                  /* the window's end: (u1, v1) */
                    ok(c, picles_flux_mean_update(c, nullptr), "update at the window's end");
                    ok(c, picles_set_winds(c, u.data(), v.data(), t + 600.0, nullptr, nullptr, 0.0), "set_winds (static)");
                } else {
                    /* (a lattice step does not follow a pending one across a moved clock: the pending step is completed first) */
                    std::vector<double> st(3 * N);
                    ok(c, picles_get_state(c, st.data()), "get_state");
                    ok(c, picles_tick(c, 100.0), "tick");                  /* between the lattice's levels: sampled into the spare pair */
                    ok(c, picles_flux_mean_update(c, nullptr), "update between lattice levels");
                    ok(c, picles_tick(c, 500.0), "tick");
                }
                break;
            default: {      /* free with samples held, and a set again */
                ok(c, picles_flux_mean_update(c, nullptr), "flux_mean_update");
                ok(c, picles_flux_mean_free(c), "flux_mean_free");
                if (picles_flux_mean_shape(c, nullptr, nullptr, nullptr) == 0) die("free left a set");
                ok(c, picles_flux_mean_init(c, every, first), "flux_mean_init again");
                if (samples(c) != 0) die("a new set holds samples");
            } break;
            }
        }
        if (round == 0) {
            if (R.coin()) break;                       /* destroy with the sets and whatever mean pushes are pending */
            if (R.coin()) ok(c, picles_flux_mean_update(c, nullptr), "flux_mean_update");
            ok(c, picles_flux_free(c), "flux_free");   /* drops the mean set with the flux set */
            if (picles_flux_mean_shape(c, nullptr, nullptr, nullptr) == 0) die("flux_free left a mean set");
            refused(c, picles_flux_mean_update(c, nullptr), -2, "update after flux_free", "picles_flux_mean_init first");
        } else if (picles_flux_pending(c) < slots && whole) {
            ok(c, picles_flux_mean_update(c, nullptr), "flux_mean_update");
            ok(c, picles_flux_mean_push(c, 0), "a mean push left pending for destroy");
        }
    }
    ok(c, picles_destroy(c), "destroy");
}
}   // namespace

int main(int argc, char **argv)
{
    const uint64_t first = argc > 1 ? strtoull(argv[1], nullptr, 10) : 0, count = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    if (picles_abi_version() != PICLES_ABI_VERSION || PICLES_ABI_VERSION < 20) { fprintf(stderr, "ABI version\n"); return 2; }
    for (uint64_t s = first; s < first + count; s++) program(s);
    printf("flux mean harness: %llu programs, %ld ABI calls, %ld refused as documented, no sanitizer report\n", (unsigned long long)count, g_calls, g_refused);
    return 0;
}
