// diag_harness.cpp — the host side of the coarse-diagnostics ring (picles_diag_*) under AddressSanitizer, on top of fake_hip.cpp
// like harness.cpp: seeded programs of init / shape / push / pop around steps, for whole-grid and slab contexts, with every buffer
// handed to picles_diag_pop allocated with exactly the size picles_diag_shape reports — a copy that assumes any other size (whole
// grid instead of slab, another field count, the padded slot instead of the field block) is an ASan report.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_diag.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../../include/picles_hip.h"

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
    if (rc != 0) { fprintf(stderr, "diag harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what)
{
    g_calls++; g_refused++;
    if (rc == 0) { fprintf(stderr, "diag harness: %s was not refused\n", what); exit(3); }
    if (!picles_last_error(c)[0]) { fprintf(stderr, "diag harness: %s refused without a text\n", what); exit(3); }
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
    double *u = (double *)malloc(N * 8), *v = (double *)malloc(N * 8);
    for (size_t k = 0; k < N; k++) { u[k] = 9.0; v[k] = 4.0; }
    ok(c, picles_set_winds(c, u, v, 0.0, nullptr, nullptr, 0.0), "set_winds");
    ok(c, picles_seed(c, 0.0), "seed");
    free(u); free(v);

    refused(c, picles_diag_push(c), "push before init");
    if (picles_diag_shape(c, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) { fprintf(stderr, "shape before init\n"); exit(3); }
    refused(c, picles_diag_init(c, 0, 2, PICLES_DIAG_HS, 2), "cx = 0");
    refused(c, picles_diag_init(c, 17, 2, PICLES_DIAG_HS, 2), "cx = 17");
    refused(c, picles_diag_init(c, 2, 2, 0, 2), "empty mask");
    refused(c, picles_diag_init(c, 2, 2, 128, 2), "unknown mask");
    refused(c, picles_diag_init(c, 2, 2, PICLES_DIAG_HS, 0), "no slots");
    int cx = R.in(1, 16), cy = R.in(1, 16);
    const int mask = R.in(1, PICLES_DIAG_ALL), slots = R.in(1, 3);
    if (g.j_begin % cy != 0) {
        refused(c, picles_diag_init(c, cx, cy, mask, slots), "j_begin not a multiple of cy");
        cy = 1;
    }
    ok(c, picles_diag_init(c, cx, cy, mask, slots), "diag_init");
    refused(c, picles_diag_init(c, cx, cy, mask, slots), "init twice");
    int32_t nxc, nyc, nf, np; size_t bytes;
    ok(c, picles_diag_shape(c, &nxc, &nyc, &nf, &np, &bytes), "diag_shape");
    if (nxc != (Nx + cx - 1) / cx || nyc != (ny + cy - 1) / cy || nf != __builtin_popcount(mask) || np != nyc * ((nxc + 255) / 256) ||
        bytes != (size_t)4 * nxc * nyc * nf) { fprintf(stderr, "diag shape\n"); exit(3); }
    refused(c, picles_diag_pop(c, &bytes, nullptr, nullptr), "pop when empty");
    const bool whole = !slab || (g.j_begin == 0 && g.j_end == Ny);
    const int nops = R.in(4, 20);
    for (int k = 0; k < nops; k++) {
        switch (R.in(0, 3)) {
        case 0: if (whole) ok(c, picles_run_steps(c, 600.0, R.in(1, 3)), "run_steps"); break;
        case 1:
            if (picles_diag_pending(c) == slots) refused(c, picles_diag_push(c), "push into a full ring");
            else ok(c, picles_diag_push(c), "diag_push");
            break;
        case 2: if (picles_diag_pending(c) > 0) {
            void *f = malloc(bytes ? bytes : 1);
            double *pp = (double *)malloc((size_t)np * 7 * 8), t = -1.0;
            ok(c, picles_diag_pop(c, f, R.coin() ? pp : nullptr, R.coin() ? &t : nullptr), "diag_pop");
            free(f); free(pp);
        } break;
        default: { size_t b; ok(c, picles_checkpoint_size(c, &b), "checkpoint_size"); } break;
        }
    }
    ok(c, picles_destroy(c), "destroy");      /* with whatever is still pending */
}
}   // namespace

int main(int argc, char **argv)
{
    const uint64_t first = argc > 1 ? strtoull(argv[1], nullptr, 10) : 0, count = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    if (picles_abi_version() != PICLES_ABI_VERSION) { fprintf(stderr, "ABI version\n"); return 2; }
    for (uint64_t s = first; s < first + count; s++) program(s);
    printf("diag harness: %llu programs, %ld ABI calls, %ld refused as documented, no sanitizer report\n", (unsigned long long)count, g_calls, g_refused);
    return 0;
}
