// probe_harness.cpp — the host side of the station-probe ring (picles_probe_*) under AddressSanitizer, on top of fake_hip.cpp like
// diag_harness.cpp: seeded programs of init / sample / steps / pop / free for whole-grid and slab contexts.  Every buffer handed to
// picles_probe_pop has exactly the size of the samples it may hand out (min(max_samples, pending) x 3 n doubles, as many times and
// steps): a copy that assumes the ring's capacity, the whole grid or another node count is an ASan report.  The ring wraps many
// times per program; a full ring must refuse with PICLES_PROBE_E_FULL and an unchanged clock, and the same call must succeed after
// a pop.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_probe.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../../include/picles_hip.h"

namespace {
struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t s) : g(s) {}
    int in(int lo, int hi) { return lo + (int)(g() % (uint64_t)(hi - lo + 1)); }
    bool coin() { return g() & 1; }
};
long g_calls = 0, g_refused = 0, g_full = 0, g_popped = 0, g_wraps = 0;
void die(const char *what) { fprintf(stderr, "probe harness: %s\n", what); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "probe harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what, int code)
{
    g_calls++; g_refused++;
    if (rc == 0) { fprintf(stderr, "probe harness: %s was not refused\n", what); exit(3); }
    if (rc != code) { fprintf(stderr, "probe harness: %s refused with %d, not %d\n", what, rc, code); exit(3); }
    if (!picles_last_error(c)[0]) { fprintf(stderr, "probe harness: %s refused without a text\n", what); exit(3); }
}

/* n model steps through an entry point that fits the context */
int step(picles_ctx *c, bool whole, Rng &R, int n)
{
    if (whole) return (n == 1 && R.coin()) ? picles_time_step(c, 600.0, R.coin() ? PICLES_STEP_ZERO_FIRST : 0) : picles_run_steps(c, 600.0, n);
    for (int k = 0; k < n; k++) {      /* a slab: the split-phase calls (they count the step and do not sample) */
        int rc = picles_begin_step(c, 600.0, PICLES_STEP_ZERO_FIRST);
        if (!rc) rc = picles_advance_rows(c, PICLES_ROWS_ALL, nullptr);
        if (!rc) rc = picles_scatter_remesh(c, nullptr);
        if (rc) return rc;
    }
    return 0;
}

void pop_some(picles_ctx *c, Rng &R, int n, long long &last_step)
{
    const int pending = picles_probe_pending(c);
    const int m = R.in(1, pending + 2);                                   /* may ask for more than there is */
    const int want = m < pending ? m : pending;
    double *v = (double *)malloc((size_t)want * 3 * n * 8), *t = (double *)malloc((size_t)want * 8);
    int64_t *s = (int64_t *)malloc((size_t)want * 8);
    int32_t got = -1;
    const bool wt = R.coin();
    ok(c, picles_probe_pop(c, m, v, wt ? t : nullptr, s, &got), "probe_pop");
    if (got != want || picles_probe_pending(c) != pending - got) die("pop count");
    for (int k = 0; k < got; k++) {
        if (s[k] < last_step) die("samples out of order");
        last_step = s[k];
    }
    g_popped += got;
    free(v); free(t); free(s);
}

void program(uint64_t seed)
{
    Rng R(0xD1B54A32D192ED03ull * (seed + 1));
    const int Nx = R.in(4, 300), Ny = R.in(4, 40);
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
    const bool whole = (g.j_begin == 0 && g.j_end == Ny);
    const size_t N = (size_t)Nx * ny;
    double *u = (double *)malloc(N * 8), *v = (double *)malloc(N * 8);
    for (size_t k = 0; k < N; k++) { u[k] = 9.0; v[k] = 4.0; }
    ok(c, picles_set_winds(c, u, v, 0.0, nullptr, nullptr, 0.0), "set_winds");
    ok(c, picles_seed(c, 0.0), "seed");
    free(u); free(v);

    /* without a set */
    int32_t dummy = 0; double dv[3];
    refused(c, picles_probe_sample(c, nullptr), "sample without a set", -2);
    refused(c, picles_probe_pop(c, 1, dv, nullptr, nullptr, &dummy), "pop without a set", -2);
    if (picles_probe_shape(c, nullptr, nullptr, nullptr) == 0 || picles_probe_pending(c) != 0) die("shape / pending without a set");
    ok(c, picles_probe_free(c), "free without a set");

    const int n = R.in(1, 700);
    std::vector<int32_t> ij((size_t)2 * n);          /* exactly 2 n entries */
    for (int k = 0; k < n; k++) { ij[k] = R.in(0, Nx - 1); ij[(size_t)n + k] = R.in(g.j_begin, g.j_end - 1); }
    if (n > 1) { ij[1] = ij[0]; ij[(size_t)n + 1] = ij[n]; }      /* a duplicate */
    const int every = R.in(1, 3), first = R.in(1, 3), cap = R.in(1, 5);
    refused(c, picles_probe_init(c, 0, ij.data(), every, first, cap), "n = 0", -2);
    refused(c, picles_probe_init(c, n, ij.data(), 0, first, cap), "every = 0", -2);
    refused(c, picles_probe_init(c, n, ij.data(), every, 0, cap), "first = 0", -2);
    refused(c, picles_probe_init(c, n, ij.data(), every, first, 0), "capacity = 0", -2);
    {
        std::vector<int32_t> bad(ij);
        const int k = R.in(0, n - 1);
        switch (R.in(0, 3)) {
        case 0: bad[k] = -1; break;
        case 1: bad[k] = Nx; break;
        case 2: bad[(size_t)n + k] = g.j_begin - 1; break;
        default: bad[(size_t)n + k] = g.j_end; break;
        }
        refused(c, picles_probe_init(c, n, bad.data(), every, first, cap), "node outside the context's rows", -2);
        if (picles_probe_shape(c, nullptr, nullptr, nullptr) == 0) die("a refused init left a set behind");
    }
    ok(c, picles_probe_init(c, n, ij.data(), every, first, cap), "probe_init");
    refused(c, picles_probe_init(c, n, ij.data(), every, first, cap), "init twice", -2);
    int32_t sn, se, sc;
    ok(c, picles_probe_shape(c, &sn, &se, &sc), "probe_shape");
    if (sn != n || se != every || sc != cap) die("shape");
    refused(c, picles_probe_pop(c, 1, dv, nullptr, nullptr, &dummy), "pop when empty", -3);
    refused(c, picles_probe_pop(c, 0, dv, nullptr, nullptr, &dummy), "max_samples = 0", -2);

    long long steps = 0, last = 0, taken = 0;
    const int nops = R.in(10, 40);
    for (int k = 0; k < nops; k++) {
        const int pending = picles_probe_pending(c);
        switch (R.in(0, 3)) {
        case 0: case 1: {
            const int ns = R.in(1, 4);
            int due = 0;
            for (long long s = steps + 1; s <= steps + ns; s++) if (s >= first && (s - first) % every == 0) due++;
            const double clock = picles_clock(c);
            if (whole && due && pending + due > cap) {
                if (due > cap) break;                /* more samples than the ring holds: no pop makes room for this call */
                refused(c, step(c, true, R, ns), "steps that would overrun the ring", PICLES_PROBE_E_FULL);
                g_full++;
                if (picles_clock(c) != clock || picles_probe_pending(c) != pending) die("a refused step changed the context");
                while (picles_probe_pending(c) + due > cap) pop_some(c, R, n, last);
                const int before = picles_probe_pending(c);
                ok(c, picles_run_steps(c, 600.0, ns), "the same steps after a pop");
                if (picles_probe_pending(c) != before + due) die("samples after the repeated call");
            } else {
                ok(c, step(c, whole, R, ns), "steps");
                if (whole && picles_probe_pending(c) != pending + due) die("automatic samples");
                if (!whole && picles_probe_pending(c) != pending) die("the split-phase calls sampled by themselves");
            }
            steps += ns;
            if (whole) taken += due;
        } break;
        case 2:
            if (pending == cap) {
                refused(c, picles_probe_sample(c, nullptr), "sample into a full ring", PICLES_PROBE_E_FULL);
                g_full++;
                pop_some(c, R, n, last);
            }
            ok(c, picles_probe_sample(c, nullptr), "probe_sample");
            taken++;
            break;
        default:
            if (pending > 0) pop_some(c, R, n, last);
            break;
        }
    }
    if (taken > cap) g_wraps++;
    if (picles_probe_pending(c) > 0 && whole) {
        size_t bytes = 0;
        ok(c, picles_checkpoint_size(c, &bytes), "checkpoint_size");
        std::vector<unsigned char> blob(bytes);
        refused(c, picles_checkpoint_load(c, blob.data(), bytes), "checkpoint_load with samples pending", PICLES_CKPT_E_BUSY);
    }
    if (R.coin()) {
        ok(c, picles_probe_free(c), "free with samples pending");
        if (picles_probe_pending(c) != 0) die("pending after free");
        if (R.coin()) {
            const int32_t one[2] = {ij[0], ij[n]};
            ok(c, picles_probe_init(c, 1, one, 1, 1, 2), "a new set after free");
            ok(c, picles_probe_sample(c, nullptr), "sample of the new set");
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
    if (count >= 100 && (g_full == 0 || g_popped == 0 || g_wraps == 0)) {
        fprintf(stderr, "probe harness: no full ring met (%ld), nothing popped (%ld) or no ring wrapped (%ld)\n", g_full, g_popped, g_wraps);
        return 3;
    }
    printf("probe harness: %llu programs, %ld ABI calls, %ld refused as documented (%ld full rings), %ld samples popped, %ld rings wrapped, "
           "no sanitizer report\n", (unsigned long long)count, g_calls, g_refused, g_full, g_popped, g_wraps);
    return 0;
}
