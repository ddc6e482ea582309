// flux_harness.cpp — the host side of the coupling-flux set (picles_flux_*) under AddressSanitizer, on top of fake_hip.cpp like
// diag_harness.cpp: seeded programs of init / shape / push / pop / export / free around steps, for whole-grid and slab contexts, with
// every buffer handed to picles_flux_pop and picles_flux_export allocated with exactly the size picles_flux_shape reports — a copy
// that assumes any other size (whole grid instead of slab, another plane count, the padded slot instead of the field block, seven
// doubles per partial instead of eleven) is an ASan report.  Every refusal of the header is provoked, the wind rule among them (a
// host-set window with the clock moved inside it; a lattice context, which samples into its spare pair instead; a wind-stream
// context at a level, between two held levels, past the newest level and before the first), and every context
// is destroyed with whatever snapshots are still pending.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_flux.py).
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
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "flux harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, int want, const char *what, const char *text = nullptr)
{
    g_calls++; g_refused++;
    if (rc != want) { fprintf(stderr, "flux harness: %s: rc=%d, expected %d (%s)\n", what, rc, want, picles_last_error(c)); exit(3); }
    if (!picles_last_error(c)[0]) { fprintf(stderr, "flux harness: %s refused without a text\n", what); exit(3); }
    if (text && !strstr(picles_last_error(c), text)) { fprintf(stderr, "flux harness: %s: the text lacks '%s': %s\n", what, text, picles_last_error(c)); exit(3); }
}

void pop_exact(picles_ctx *c, Rng &R, size_t bytes, int np)
{
    void *f = malloc(bytes ? bytes : 1);
    double *pp = (double *)malloc((size_t)np * PICLES_FLUX_NPARTIAL * 8), t = -1.0;
    ok(c, picles_flux_pop(c, f, R.coin() ? pp : nullptr, R.coin() ? &t : nullptr), "flux_pop");
    free(f); free(pp);
}

void export_exact(picles_ctx *c, Rng &R, size_t bytes, int np)
{
    void *fd = nullptr, *pd = nullptr, *caller = nullptr;      /* the caller's stream, or none */
    if (R.coin() && hipStreamCreateWithFlags(&caller, 0) != 0) { fprintf(stderr, "hipStreamCreate\n"); exit(3); }
    if (hipMalloc(&fd, bytes ? bytes : 1) != 0 || hipMalloc(&pd, (size_t)np * PICLES_FLUX_NPARTIAL * 8) != 0) { fprintf(stderr, "hipMalloc\n"); exit(3); }
    refused(c, picles_flux_export(c, nullptr, (double *)pd, caller), -2, "export without a field buffer", "no device buffer");
    ok(c, picles_flux_export(c, fd, R.coin() ? (double *)pd : nullptr, caller), "flux_export");
    hipFree(fd); hipFree(pd);
    if (caller) hipStreamDestroy(caller);
}

void program(uint64_t seed)
{
    Rng R(0x9E3779B97F4A7C15ull * (seed + 1));
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
    const bool lattice = R.in(0, 3) == 0;
    const bool stream = !slab && !lattice && R.in(0, 2) == 0;      /* a wind stream: levels 0 and 1 of a ring of three held, the clock stays at 0 */
    std::vector<double> u(N, 9.0), v(N, 4.0), u1(N, 7.0), v1(N, 5.0);
    if (lattice) {
        const double lu[2 * 2 * 3] = {9, 9, 9, 9, 8, 8, 8, 8, 7, 7, 7, 7}, lv[2 * 2 * 3] = {4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6};
        ok(c, picles_set_wind_grid(c, 2, 2, 3, 0.0, 2000.0 * Nx, 0.0, 1500.0 * Ny, 0.0, 1800.0, lu, lv, 0.0, 0.0), "set_wind_grid");
    } else if (stream) {
        const double l0[4] = {9, 9, 9, 9}, l1[4] = {7, 7, 7, 7};
        ok(c, picles_wind_stream_init(c, 2, 2, 0.0, 2000.0 * Nx, 0.0, 1500.0 * Ny, 0.0, 1800.0, 0.0, 0.0, 3), "wind_stream_init");
        ok(c, picles_wind_stream_push(c, 0, l0, l1, PICLES_WIND_F64, PICLES_WIND_HOST, nullptr), "wind_stream_push 0");
        ok(c, picles_wind_stream_push(c, 1, l1, l0, PICLES_WIND_F64, PICLES_WIND_HOST, nullptr), "wind_stream_push 1");
    } else {
        ok(c, picles_set_winds(c, u.data(), v.data(), 0.0, nullptr, nullptr, 0.0), "set_winds");
    }
    ok(c, picles_seed(c, 0.0), "seed");

    size_t bytes = 0;
    refused(c, picles_flux_push(c), -2, "push before init", "picles_flux_init first");
    refused(c, picles_flux_export(c, &bytes, nullptr, nullptr), -2, "export before init", "picles_flux_init first");
    refused(c, picles_flux_free(c), -2, "free before init", "picles_flux_init first");
    if (picles_flux_shape(c, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 || picles_flux_pending(c) != 0) { fprintf(stderr, "shape / pending before init\n"); exit(3); }
    refused(c, picles_flux_init(c, 0, 2, PICLES_FLUX_PHI_IN, 1.0, 1.0, 2), -2, "cx = 0", "1 ... 16");
    refused(c, picles_flux_init(c, 17, 2, PICLES_FLUX_PHI_IN, 1.0, 1.0, 2), -2, "cx = 17", "1 ... 16");
    refused(c, picles_flux_init(c, 2, 0, PICLES_FLUX_PHI_IN, 1.0, 1.0, 2), -2, "cy = 0", "1 ... 16");
    refused(c, picles_flux_init(c, 2, 2, 0, 1.0, 1.0, 2), -2, "empty mask", "field mask");
    refused(c, picles_flux_init(c, 2, 2, 512, 1.0, 1.0, 2), -2, "unknown mask", "field mask");
    refused(c, picles_flux_init(c, 2, 2, -1, 1.0, 1.0, 2), -2, "negative mask", "field mask");
    refused(c, picles_flux_init(c, 2, 2, PICLES_FLUX_ALL, 0.0, 1.0, 2), -2, "scale_phi = 0", "finite and positive");
    refused(c, picles_flux_init(c, 2, 2, PICLES_FLUX_ALL, 1.0, -2.0, 2), -2, "scale_tau < 0", "finite and positive");
    refused(c, picles_flux_init(c, 2, 2, PICLES_FLUX_ALL, INFINITY, 1.0, 2), -2, "scale_phi = inf", "finite and positive");
    refused(c, picles_flux_init(c, 2, 2, PICLES_FLUX_ALL, 1.0, NAN, 2), -2, "scale_tau = NaN", "finite and positive");
    refused(c, picles_flux_init(c, 2, 2, PICLES_FLUX_PHI_IN, 1.0, 1.0, 0), -2, "no slots", "n_slots");
    if (picles_flux_pending(c) != 0) { fprintf(stderr, "a refused init left a ring\n"); exit(3); }

    for (int round = 0; round < 2; round++) {          /* the second round: after picles_flux_free, another set */
        int cx = R.in(1, 16), cy = R.in(1, 16);
        const int mask = R.in(1, PICLES_FLUX_ALL), slots = R.in(1, 3);
        if (g.j_begin % cy != 0) {
            refused(c, picles_flux_init(c, cx, cy, mask, 10055.25, 1025.0, slots), -2, "j_begin not a multiple of cy", "multiple of cy");
            cy = 1;
        }
        ok(c, picles_flux_init(c, cx, cy, mask, 10055.25, 1025.0, slots), "flux_init");
        refused(c, picles_flux_init(c, cx, cy, mask, 10055.25, 1025.0, slots), -2, "init twice", "already initialised");
        int32_t nxc, nyc, nf, np;
        ok(c, picles_flux_shape(c, &nxc, &nyc, &nf, &np, &bytes), "flux_shape");
        if (nxc != (Nx + cx - 1) / cx || nyc != (ny + cy - 1) / cy || nf != __builtin_popcount(mask) || np != nyc * ((nxc + 255) / 256) ||
            bytes != (size_t)4 * nxc * nyc * nf) { fprintf(stderr, "flux shape\n"); exit(3); }
        refused(c, picles_flux_pop(c, &bytes, nullptr, nullptr), -3, "pop when empty", "no flux snapshot");
        const int nops = R.in(4, 20);
        for (int k = 0; k < nops; k++) {
            switch (R.in(0, 5)) {
            case 0: if (whole && !stream) ok(c, picles_run_steps(c, 600.0, R.in(1, 3)), "run_steps"); break;
            case 1:
                if (picles_flux_pending(c) == slots) refused(c, picles_flux_push(c), -3, "push into a full ring", "ring full");
                else ok(c, picles_flux_push(c), "flux_push");
                break;
            case 2: if (picles_flux_pending(c) > 0) pop_exact(c, R, bytes, np); break;
            case 3: export_exact(c, R, bytes, np); break;
            case 4: {      /* the wind rule: the clock moved to a time at which the window holds no level */
                const double t = picles_clock(c);
                const int pending = picles_flux_pending(c);
                if (stream) {      /* at a level, between two held levels, past the newest, before the first */
                    if (pending < slots) ok(c, picles_flux_push(c), "push at a stream level");
                    ok(c, picles_tick(c, 100.0), "tick");
                    export_exact(c, R, bytes, np);
                    ok(c, picles_tick(c, 3600.0), "tick");
                    refused(c, picles_flux_push(c), pending + (pending < slots ? 1 : 0) == slots ? -3 : -2, "push past the newest level",
                            pending + (pending < slots ? 1 : 0) == slots ? "ring full" : "picles_wind_stream_push");
                    void *fd = nullptr;
                    if (hipMalloc(&fd, bytes ? bytes : 1) != 0) { fprintf(stderr, "hipMalloc\n"); exit(3); }
                    refused(c, picles_flux_export(c, fd, nullptr, nullptr), -2, "export past the newest level", "not held");
                    ok(c, picles_tick(c, -3750.0), "tick");
                    refused(c, picles_flux_export(c, fd, nullptr, nullptr), -2, "export before the first level", "before the first time level");
                    hipFree(fd);
                    ok(c, picles_tick(c, 50.0), "tick");
                } else if (!lattice) {
                    ok(c, picles_set_winds(c, u.data(), v.data(), t, u1.data(), v1.data(), t + 600.0), "set_winds (two levels)");
                    ok(c, picles_tick(c, 100.0), "tick");
                    refused(c, picles_flux_push(c), pending == slots ? -3 : -2, "push inside a host window", pending == slots ? "ring full" : "step to a level");
                    void *fd = nullptr;
                    if (hipMalloc(&fd, bytes ? bytes : 1) != 0) { fprintf(stderr, "hipMalloc\n"); exit(3); }
                    refused(c, picles_flux_export(c, fd, nullptr, nullptr), -2, "export inside a host window", "set the window");
                    hipFree(fd);
                    ok(c, picles_tick(c, 500.0), "tick");                  /* the window's end: (u1, v1) */
                    if (pending < slots) ok(c, picles_flux_push(c), "push at the window's end");
                    ok(c, picles_set_winds(c, u.data(), v.data(), t + 600.0, nullptr, nullptr, 0.0), "set_winds (static)");
                } else {
                    ok(c, picles_tick(c, 100.0), "tick");                  /* between the lattice's levels: sampled into the spare pair */
                    if (pending < slots) ok(c, picles_flux_push(c), "push between lattice levels");
                    export_exact(c, R, bytes, np);
                    ok(c, picles_tick(c, 500.0), "tick");
                }
                if (picles_flux_pending(c) != pending + (pending < slots ? 1 : 0)) { fprintf(stderr, "pending after the wind rule\n"); exit(3); }
            } break;
            default: { size_t b; ok(c, picles_checkpoint_size(c, &b), "checkpoint_size"); } break;
            }
        }
        if (round == 0) {
            if (R.coin()) { ok(c, picles_flux_free(c), "flux_free");      /* with whatever is still pending */
                            if (picles_flux_pending(c) != 0 || picles_flux_shape(c, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) { fprintf(stderr, "free left a set\n"); exit(3); } }
            else break;
        }
    }
    ok(c, picles_destroy(c), "destroy");      /* with whatever is still pending */
}
}   // namespace

int main(int argc, char **argv)
{
    const uint64_t first = argc > 1 ? strtoull(argv[1], nullptr, 10) : 0, count = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    if (picles_abi_version() != PICLES_ABI_VERSION || PICLES_ABI_VERSION < 19) { fprintf(stderr, "ABI version\n"); return 2; }
    for (uint64_t s = first; s < first + count; s++) program(s);
    printf("flux harness: %llu programs, %ld ABI calls, %ld refused as documented, no sanitizer report\n", (unsigned long long)count, g_calls, g_refused);
    return 0;
}
