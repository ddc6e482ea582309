// probe_harness.cpp — the host side of the station-probe ring (picles_probe_*) under AddressSanitizer, on top of fake_hip.cpp like
// diag_harness.cpp: seeded programs of init / sample / steps / pop / free for whole-grid and slab contexts.  Every buffer handed to
// picles_probe_pop has exactly the size of the samples it may hand out (min(max_samples, pending) x 3 n doubles, as many times and
// steps): a copy that assumes the ring's capacity, the whole grid or another node count is an ASan report.  The ring wraps many
// times per program; a full ring must refuse with PICLES_PROBE_E_FULL and an unchanged clock, and the same call must succeed after
// a pop.
// A second kind of program (all_at_once) puts a snapshot ring, a diagnostics ring, a probe set and a checkpoint in flight on ONE
// context — they share its store stream and the ring code —, each ring set up through every allocation failure its init can meet
// (fake_hip_fail_alloc: the failed init leaves nothing behind and the next one works), driven through wrap-around and its full-ring
// refusal, freed and destroyed with entries pending.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_probe.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../../include/picles_hip.h"

extern "C" long fake_hip_fail_alloc(long k);      /* fake_hip.cpp */
extern "C" long fake_hip_live(void);

namespace {
struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t s) : g(s) {}
    int in(int lo, int hi) { return lo + (int)(g() % (uint64_t)(hi - lo + 1)); }
    bool coin() { return g() & 1; }
};
long g_calls = 0, g_refused = 0, g_full = 0, g_popped = 0, g_wraps = 0;
long g_all_full[3] = {0, 0, 0}, g_all_wraps[3] = {0, 0, 0}, g_failed_inits = 0, g_checkpoints = 0;      /* all_at_once: store, diag, probe */
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

/* a seeded context over the whole grid or a slab of it; nullptr: picles_create refused the shape */
picles_ctx *make_context(Rng &R, picles_grid &g)
{
    const int Nx = R.in(4, 300), Ny = R.in(4, 40);
    picles_phys p; picles_ode o; picles_model m;
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
    if (picles_create(&g, &p, &o, &m, 0, 1, &c) != 0) { g_refused++; return nullptr; }
    const size_t N = (size_t)Nx * (g.j_end - g.j_begin);
    double *u = (double *)malloc(N * 8), *v = (double *)malloc(N * 8);
    for (size_t k = 0; k < N; k++) { u[k] = 9.0; v[k] = 4.0; }
    ok(c, picles_set_winds(c, u, v, 0.0, nullptr, nullptr, 0.0), "set_winds");
    ok(c, picles_seed(c, 0.0), "seed");
    free(u); free(v);
    return c;
}

void program(uint64_t seed)
{
    Rng R(0xD1B54A32D192ED03ull * (seed + 1));
    picles_grid g;
    picles_ctx *c = make_context(R, g);
    if (!c) return;
    const int Nx = g.Nx, Ny = g.Ny;
    const bool whole = (g.j_begin == 0 && g.j_end == Ny);

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

/* an init that meets an allocation failure at every place it can: each failed attempt hands back what it had taken and leaves the
 * context without the ring (`exists` says so), and the attempt that meets none succeeds */
template <class Init, class Exists>
void init_through_failures(picles_ctx *c, Init init, Exists exists, const char *what)
{
    for (long k = 1;; k++) {
        const long live = fake_hip_live();
        fake_hip_fail_alloc(k);
        const int rc = init();
        g_calls++;
        if (fake_hip_fail_alloc(0) > 0) {      /* the init made fewer than k allocations: nothing failed */
            if (rc != 0) { fprintf(stderr, "probe harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
            return;
        }
        g_failed_inits++;
        if (rc == 0) { fprintf(stderr, "probe harness: %s succeeded although allocation %ld failed\n", what, k); exit(3); }
        if (exists()) { fprintf(stderr, "probe harness: the failed %s (allocation %ld) left a ring behind\n", what, k); exit(3); }
        if (fake_hip_live() != live) {
            fprintf(stderr, "probe harness: the failed %s (allocation %ld) kept %ld allocations or events\n", what, k, fake_hip_live() - live);
            exit(3);
        }
        if (k > 64) die("an init that never gets through");
    }
}

/* every output path on one context: a snapshot ring, a diagnostics ring, a probe set and a checkpoint in flight at once */
void all_at_once(uint64_t seed)
{
    Rng R(0xA0761D6478BD642Full * (seed + 1));
    picles_grid g;
    picles_ctx *c = make_context(R, g);
    if (!c) return;
    const int Nx = g.Nx, ny = g.j_end - g.j_begin;
    const bool whole = (g.j_begin == 0 && g.j_end == g.Ny);
    const size_t N = (size_t)Nx * ny;
    const int cap[3] = {R.in(1, 3), R.in(1, 3), R.in(1, 4)};
    const int cx = R.in(1, 4), cy = (g.j_begin % 2 == 0) ? R.in(1, 2) : 1, mask = R.in(1, PICLES_DIAG_ALL), n = R.in(1, 40);
    std::vector<int32_t> ij((size_t)2 * n);
    for (int k = 0; k < n; k++) { ij[k] = R.in(0, Nx - 1); ij[(size_t)n + k] = R.in(g.j_begin, g.j_end - 1); }
    init_through_failures(c, [&] { return picles_store_init(c, cap[0]); }, [&] { return picles_store_push(c) == 0; }, "store_init");
    init_through_failures(c, [&] { return picles_diag_init(c, cx, cy, mask, cap[1]); },
                          [&] { return picles_diag_shape(c, nullptr, nullptr, nullptr, nullptr, nullptr) == 0; }, "diag_init");
    init_through_failures(c, [&] { return picles_probe_init(c, n, ij.data(), 1, 1, cap[2]); },
                          [&] { return picles_probe_shape(c, nullptr, nullptr, nullptr) == 0; }, "probe_init");
    refused(c, picles_store_init(c, cap[0]), "store_init twice", -2);
    refused(c, picles_diag_init(c, cx, cy, mask, cap[1]), "diag_init twice", -2);
    refused(c, picles_probe_init(c, n, ij.data(), 1, 1, cap[2]), "probe_init twice", -2);
    int32_t nxc, nyc, nf, np; size_t fbytes, ckbytes;
    ok(c, picles_diag_shape(c, &nxc, &nyc, &nf, &np, &fbytes), "diag_shape");
    ok(c, picles_checkpoint_size(c, &ckbytes), "checkpoint_size");

    /* pops into buffers of exactly the size the entry has */
    auto pop_store = [&] {
        double *s = (double *)malloc(3 * N * 8), t;
        ok(c, picles_store_pop(c, s, &t), "store_pop");
        free(s);
    };
    auto pop_diag = [&] {
        void *f = malloc(fbytes ? fbytes : 1);
        double *pp = (double *)malloc((size_t)np * 7 * 8), t;
        ok(c, picles_diag_pop(c, f, pp, &t), "diag_pop");
        free(f); free(pp);
    };
    long long last = 0;
    long pushed[3] = {0, 0, 0};
    bool inflight = false;
    const int nops = R.in(20, 60);
    for (int k = 0; k < nops; k++) {
        switch (R.in(0, 7)) {
        case 0: case 1: {      /* one model step; a whole grid samples by itself, a slab's caller does */
            if (picles_probe_pending(c) == cap[2]) {
                const double clock = picles_clock(c);
                if (whole) {
                    refused(c, picles_time_step(c, 600.0, PICLES_STEP_ZERO_FIRST), "a step into a full probe ring", PICLES_PROBE_E_FULL);
                    if (picles_clock(c) != clock) die("a refused step moved the clock");
                } else refused(c, picles_probe_sample(c, nullptr), "a sample into a full probe ring", PICLES_PROBE_E_FULL);
                g_all_full[2]++;
                pop_some(c, R, n, last);
            }
            if (whole) ok(c, picles_time_step(c, 600.0, PICLES_STEP_ZERO_FIRST), "time_step");
            else { ok(c, step(c, false, R, 1), "slab step"); ok(c, picles_probe_sample(c, nullptr), "probe_sample"); }
            pushed[2]++;
        } break;
        case 2:
            if (picles_store_pending(c) == cap[0]) {
                refused(c, picles_store_push(c), "push into a full snapshot ring", -3);
                g_all_full[0]++;
                pop_store();
            }
            ok(c, picles_store_push(c), "store_push");      /* after the refusal and a pop: the same call again */
            pushed[0]++;
            break;
        case 3:
            if (picles_diag_pending(c) == cap[1]) {
                refused(c, picles_diag_push(c), "push into a full diagnostics ring", -3);
                g_all_full[1]++;
                pop_diag();
            }
            ok(c, picles_diag_push(c), "diag_push");
            pushed[1]++;
            break;
        case 4: if (picles_store_pending(c) > 0) pop_store(); break;
        case 5: if (picles_diag_pending(c) > 0) pop_diag(); break;
        case 6: if (picles_probe_pending(c) > 0) pop_some(c, R, n, last); break;
        default:
            if (!inflight) { ok(c, picles_checkpoint_begin(c), "checkpoint_begin"); inflight = true; break; }
            refused(c, picles_checkpoint_begin(c), "a second checkpoint", PICLES_CKPT_E_BUSY);
            if (R.coin()) {
                unsigned char *blob = (unsigned char *)malloc(ckbytes);      /* exactly the blob */
                if (ckbytes > 1) refused(c, picles_checkpoint_end(c, blob, ckbytes - 1), "checkpoint_end into a short buffer", PICLES_CKPT_E_SHORT);
                ok(c, picles_checkpoint_end(c, blob, ckbytes), "checkpoint_end");
                inflight = false;
                g_checkpoints++;
                if (picles_store_pending(c) + picles_diag_pending(c) + picles_probe_pending(c) > 0)
                    refused(c, picles_checkpoint_load(c, blob, ckbytes), "checkpoint_load with entries pending", PICLES_CKPT_E_BUSY);
                free(blob);
            }
            break;
        }
    }
    for (int r = 0; r < 3; r++) if (pushed[r] > 2 * cap[r]) g_all_wraps[r]++;
    if (R.coin()) {
        ok(c, picles_probe_free(c), "free with samples pending");
        if (R.coin()) {
            init_through_failures(c, [&] { return picles_probe_init(c, n, ij.data(), 2, 1, cap[2]); },
                                  [&] { return picles_probe_shape(c, nullptr, nullptr, nullptr) == 0; }, "probe_init after free");
            ok(c, picles_probe_sample(c, nullptr), "sample of the new set");
        }
    }
    ok(c, picles_destroy(c), "destroy");      /* with entries pending in every ring and, maybe, a checkpoint in flight */
}
}   // namespace

int main(int argc, char **argv)
{
    const uint64_t first = argc > 1 ? strtoull(argv[1], nullptr, 10) : 0, count = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    if (picles_abi_version() != PICLES_ABI_VERSION) { fprintf(stderr, "ABI version\n"); return 2; }
    for (uint64_t s = first; s < first + count; s++) { program(s); all_at_once(s); }
    if (count >= 100 && (g_full == 0 || g_popped == 0 || g_wraps == 0)) {
        fprintf(stderr, "probe harness: no full ring met (%ld), nothing popped (%ld) or no ring wrapped (%ld)\n", g_full, g_popped, g_wraps);
        return 3;
    }
    for (int r = 0; r < 3; r++)
        if (count >= 100 && (g_all_full[r] == 0 || g_all_wraps[r] == 0 || g_failed_inits == 0 || g_checkpoints == 0)) {
            fprintf(stderr, "probe harness: all at once: ring %d met no full ring (%ld) or never wrapped twice (%ld), no init failed (%ld) or no "
                    "checkpoint completed (%ld)\n", r, g_all_full[r], g_all_wraps[r], g_failed_inits, g_checkpoints);
            return 3;
        }
    printf("probe harness: %llu programs, %ld ABI calls, %ld refused as documented (%ld full rings), %ld samples popped, %ld rings wrapped; "
           "all at once: full rings %ld / %ld / %ld, rings wrapped twice %ld / %ld / %ld (snapshots / diagnostics / probes), %ld failed inits "
           "undone, %ld checkpoints; no sanitizer report\n", (unsigned long long)count, g_calls, g_refused, g_full, g_popped, g_wraps,
           g_all_full[0], g_all_full[1], g_all_full[2], g_all_wraps[0], g_all_wraps[1], g_all_wraps[2], g_failed_inits, g_checkpoints);
    return 0;
}
