// track_harness.cpp — the host side of the track samples (picles_track_*) under AddressSanitizer + UBSan, on top of fake_hip.cpp like
// probe_harness.cpp: seeded programs of init / sample / steps / fetch / free on whole-grid contexts.  The arrays handed to
// picles_track_init have exactly m, 8 m and 4 m entries and the buffer handed to picles_track_fetch_end exactly 8 n doubles: a copy
// that assumes the whole table, the staging capacity or another event count is an ASan report.  Every refusal of the contract is
// met with its code and a text and leaves the context without a set (or with the set it had); every creation inside
// picles_track_init is failed in turn (fake_hip_fail_alloc: the failed init leaves nothing behind and the same call then succeeds);
// the fetch staging grows at least twice per program, also through failed allocations; contexts are destroyed with a set and with
// an open fetch.  The refusal on the native ring runs on a ring of one through the loopback communicator (PICLES_CCL_LIB), as harness.cpp
// reaches the ring.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_track.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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
    double u() { return (double)(g() >> 11) / 9007199254740992.0; }
    bool coin() { return g() & 1; }
};
long g_calls = 0, g_refused = 0, g_failed_inits = 0, g_fetches = 0, g_grown = 0, g_failed_grow = 0, g_open_destroyed = 0, g_long_steps = 0, g_ring = 0;
const double DT = 600.0;
void die(const char *what) { fprintf(stderr, "track harness: %s\n", what); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "track harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what, int code)
{
    g_calls++; g_refused++;
    if (rc == 0) { fprintf(stderr, "track harness: %s was not refused\n", what); exit(3); }
    if (rc != code) { fprintf(stderr, "track harness: %s refused with %d, not %d\n", what, rc, code); exit(3); }
    if (!picles_last_error(c)[0]) { fprintf(stderr, "track harness: %s refused without a text\n", what); exit(3); }
}
bool has_set(picles_ctx *c)
{
    int32_t m = 0;
    const int rc = picles_track_info(c, &m, nullptr, nullptr);
    if ((rc == 0) != (m >= 1) || (rc != 0 && m != -1)) die("track_info: return value and m disagree");
    return rc == 0;
}

/* a context over the whole grid, or over a slab of it; seeded or not */
picles_ctx *make_context(Rng &R, picles_grid &g, bool slab, bool seed)
{
    const int Nx = R.in(4, 200), Ny = R.in(6, 30);
    picles_phys p; picles_ode o; picles_model m;
    memset(&g, 0, sizeof g); memset(&p, 0, sizeof p); memset(&o, 0, sizeof o); memset(&m, 0, sizeof m);
    g.Nx = Nx; g.Ny = Ny; g.dx = 2000.0; g.dy = 1500.0; g.periodic_x = 1; g.periodic_y = 1;
    g.j_begin = slab ? 1 : 0;
    g.j_end = slab ? Ny - 1 : Ny;
    p.r_g = 0.85; p.C_alpha = -1.41; p.C_phi = 0.04; p.C_e = 2.2117647058823533e-4; p.g = 9.81; p.gamma = 0.88; p.q = -0.25;
    p.c_beta = 0.04; p.c_D = 2e-3; p.c_e = 1.3e-6; p.c_alpha = 11.8;
    p.propagation = p.input = p.dissipation = p.peak_shift = p.direction = 1;
    o.abstol = 1e-4; o.reltol = 1e-3; o.dt0 = 1e-3; o.dtmin = 1e-4; o.force_dtmin = 1; o.solver = 0; o.maxiters = 10000;
    o.log_energy_minimum = -13.0; o.log_energy_maximum = 3.3; o.wind_min_squared = 4.0; o.timestep = DT;
    m.periodic_boundary = 1; m.minimal_state[0] = 1.25e-6; m.minimal_state[1] = 1.28e-9;
    picles_ctx *c = nullptr;
    g_calls++;
    if (picles_create(&g, &p, &o, &m, 0, 1, &c) != 0) return nullptr;
    if (seed) {
        const size_t N = (size_t)Nx * (g.j_end - g.j_begin);
        std::vector<double> u(N, 9.0), v(N, 4.0);
        ok(c, picles_set_winds(c, u.data(), v.data(), 0.0, nullptr, nullptr, 0.0), "set_winds");
        ok(c, picles_seed(c, 0.0), "seed");
    }
    return c;
}

struct Events {
    int m;
    std::vector<double> t, w;          /* exactly m and 4 m */
    std::vector<int32_t> ij;           /* exactly 8 m */
};
Events make_events(Rng &R, const picles_grid &g, int m)
{
    Events e{m, std::vector<double>((size_t)m), std::vector<double>((size_t)4 * m), std::vector<int32_t>((size_t)8 * m)};
    for (int k = 0; k < m; k++) e.t[k] = -2.0 * DT + R.u() * 24.0 * DT;
    std::sort(e.t.begin(), e.t.end());
    if (m > 2) e.t[1] = e.t[0];      /* equal times */
    for (int c = 0; c < 4; c++)
        for (int k = 0; k < m; k++) {
            e.ij[(size_t)c * m + k] = R.in(0, g.Nx - 1);
            e.ij[(size_t)(4 + c) * m + k] = R.in(0, g.Ny - 1);
            e.w[(size_t)c * m + k] = R.coin() ? R.u() : 0.0;
        }
    return e;
}
int init(picles_ctx *c, const Events &e, double H) { return picles_track_init(c, e.m, e.t.data(), e.ij.data(), e.w.data(), H); }

/* every creation inside the init failed in turn: each failed attempt hands back what it had taken and leaves no set; the attempt
 * that meets no failure succeeds */
void init_through_failures(picles_ctx *c, const Events &e, double H)
{
    for (long k = 1;; k++) {
        const long live = fake_hip_live();
        fake_hip_fail_alloc(k);
        const int rc = init(c, e, H);
        g_calls++;
        if (fake_hip_fail_alloc(0) > 0) {      /* the init made fewer than k creations: nothing failed */
            if (rc != 0) { fprintf(stderr, "track harness: track_init failed rc=%d: %s\n", rc, picles_last_error(c)); exit(3); }
            return;
        }
        g_failed_inits++;
        if (rc == 0) die("track_init succeeded although a creation failed");
        if (!picles_last_error(c)[0]) die("a failed creation without a text");
        if (has_set(c)) die("the failed track_init left a set behind");
        if (fake_hip_live() != live) die("the failed track_init kept allocations or events");
        if (k > 32) die("an init that never gets through");
    }
}

/* one fetch of [k0, k0 + n) into a buffer of exactly 8 n doubles */
void fetch(picles_ctx *c, Rng &R, int k0, int n, size_t &cap, long long &samples)
{
    const bool grows = (size_t)8 * n > cap;
    if (grows && R.coin()) {      /* the growth meets a failed allocation (the device block, or its pinned twin): no fetch is open afterwards */
        fake_hip_fail_alloc(R.in(1, 2));
        const int rc = picles_track_fetch_begin(c, k0, n);
        g_calls++;
        if (fake_hip_fail_alloc(0) > 0 || rc == 0) die("a fetch whose staging could not grow went through");
        g_failed_grow++;
        double d;
        refused(c, picles_track_fetch_end(c, &d), "fetch_end after a failed fetch_begin", -2);
        cap = 0;
    }
    ok(c, picles_track_fetch_begin(c, k0, n), "fetch_begin");
    if (grows) { g_grown++; cap = (size_t)8 * n; }
    refused(c, picles_track_fetch_begin(c, k0, n), "a second fetch_begin", -2);
    if (R.coin()) { ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "a step beside the copy"); samples++; }
    refused(c, picles_track_fetch_end(c, nullptr), "fetch_end without a buffer", -2);
    double *out = (double *)malloc((size_t)8 * n * sizeof(double));
    ok(c, picles_track_fetch_end(c, out), "fetch_end");
    for (size_t k = 0; k < (size_t)8 * n; k++) if (out[k] == out[k]) die("an entry that is not NaN (no kernel runs here)");
    free(out);
    refused(c, picles_track_fetch_end(c, out), "fetch_end twice", -2);
    g_fetches++;
}

void program(uint64_t seed)
{
    Rng R(0x9E3779B97F4A7C15ull * (seed + 1));
    picles_grid g;
    picles_ctx *c = make_context(R, g, false, true);
    if (!c) die("picles_create");
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double d8[8];

    /* without a set */
    refused(c, picles_track_sample(c, nullptr), "sample without a set", -2);
    refused(c, picles_track_fetch_begin(c, 0, 1), "fetch_begin without a set", -2);
    refused(c, picles_track_fetch_end(c, d8), "fetch_end without a set", -2);
    if (has_set(c)) die("a set before init");
    ok(c, picles_track_free(c), "free without a set");
    ok(c, picles_time_step(c, 5.0 * DT, PICLES_STEP_ZERO_FIRST), "a long step without a set");

    const int m = R.in(1, 900);
    const Events e = make_events(R, g, m);
    const double H = DT * (R.coin() ? 1.0 : 1.5);
    /* the refusals of init: each leaves no set, and the context steps */
    refused(c, init(c, Events{0, {}, {}, {}}, H), "m = 0", -2);
    refused(c, picles_track_init(c, 1 << 28, e.t.data(), e.ij.data(), e.w.data(), H), "8 m beyond INT32_MAX", -2);      /* refused before an array is read */
    refused(c, picles_track_init(c, m, nullptr, e.ij.data(), e.w.data(), H), "no times", -2);
    for (double h : {0.0, -DT, inf, nan}) refused(c, init(c, e, h), "a horizon that is not finite and positive", -2);
    {
        Events b = e;
        const int k = R.in(0, m - 1);
        b.t[k] = R.coin() ? nan : inf;
        refused(c, init(c, b, H), "a time that is not finite", -2);
        if (m > 1) { b = e; b.t[m - 1] = b.t[0] - 1.0; refused(c, init(c, b, H), "times out of order", -2); }
        for (int v = 0; v < 4; v++) {
            b = e;
            const int q = R.in(0, 3);
            b.ij[(size_t)((v < 2 ? 0 : 4) + q) * m + k] = (v & 1) ? (v < 2 ? g.Nx : g.Ny) : -1;
            refused(c, init(c, b, H), "a node off the grid", -2);
        }
        for (double w : {-1e-300, nan, inf}) { b = e; b.w[(size_t)R.in(0, 3) * m + k] = w; refused(c, init(c, b, H), "a weight that is negative or not finite", -2); }
        if (has_set(c)) die("a refused init left a set behind");
        ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "a step after the refusals");
    }
    init_through_failures(c, e, H);
    refused(c, init(c, e, H), "init twice", -2);
    int32_t im; double ih; int64_t is;
    ok(c, picles_track_info(c, &im, &ih, &is), "track_info");
    if (im != m || ih != H || is != 0) die("info after init");
    unsigned char id[PICLES_SLAB_ID_BYTES] = {0};
    refused(c, picles_slab_comm_init(c, id, 0, 1), "the native ring on a context with a set", -5);

    long long samples = 0;
    size_t cap = 0;
    for (int n : {1, std::min(m, 1 + m / 3), m}) fetch(c, R, 0, n, cap, samples);      /* the staging is made, then grows twice (m >= 3) */
    const int nops = R.in(12, 30);
    for (int k = 0; k < nops; k++) {
        switch (R.in(0, 4)) {
        case 0: {
            const int n = R.in(1, 4);
            const double clock = picles_clock(c);
            if (R.coin()) {
                refused(c, n == 1 ? picles_time_step(c, 2.0 * DT, PICLES_STEP_ZERO_FIRST) : picles_run_steps(c, 2.0 * DT, n), "a step beyond the horizon", -2);
                g_long_steps++;
                if (picles_clock(c) != clock) die("a refused step moved the clock");
            }
            ok(c, n == 1 ? picles_time_step(c, H, PICLES_STEP_ZERO_FIRST) : picles_run_steps(c, DT, n), "steps");
            samples += n;
        } break;
        case 1:
            ok(c, picles_track_sample(c, nullptr), "track_sample");
            samples++;
            break;
        case 2: {
            const int n = R.in(1, m), k0 = R.in(0, m - n);
            fetch(c, R, k0, n, cap, samples);
        } break;
        case 3:
            refused(c, picles_track_fetch_end(c, d8), "fetch_end without fetch_begin", -2);
            refused(c, picles_track_fetch_begin(c, -1, 1), "k0 < 0", -2);
            refused(c, picles_track_fetch_begin(c, 0, 0), "n < 1", -2);
            refused(c, picles_track_fetch_begin(c, R.in(0, m), m + 1), "a range beyond m", -2);
            refused(c, picles_track_fetch_begin(c, m, 1), "k0 = m", -2);
            break;
        default: {      /* a checkpoint round trip leaves the set alone */
            size_t bytes = 0;
            ok(c, picles_checkpoint_size(c, &bytes), "checkpoint_size");
            std::vector<unsigned char> blob(bytes);
            ok(c, picles_checkpoint_begin(c), "checkpoint_begin");
            ok(c, picles_checkpoint_end(c, blob.data(), bytes), "checkpoint_end");
            ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "a step behind the checkpoint");
            samples++;
            ok(c, picles_checkpoint_load(c, blob.data(), bytes), "checkpoint_load with a set");
            ok(c, picles_seed(c, picles_clock(c)), "seed with a set");
        }
        }
        ok(c, picles_track_info(c, &im, nullptr, &is), "track_info");
        if (im != m || is != samples) die("samples taken");
    }
    if (R.coin()) {
        ok(c, picles_track_free(c), "track_free");
        if (has_set(c)) die("a set after free");
        refused(c, picles_track_sample(c, nullptr), "sample after free", -2);
        ok(c, picles_time_step(c, 3.0 * DT, PICLES_STEP_ZERO_FIRST), "a long step after free");
        if (R.coin()) {
            const Events e2 = make_events(R, g, R.in(1, 50));
            init_through_failures(c, e2, 3.0 * DT);
            ok(c, picles_track_sample(c, nullptr), "sample of the new set");
            ok(c, picles_time_step(c, 3.0 * DT, PICLES_STEP_ZERO_FIRST), "a step under the new horizon");
        }
    }
    if (has_set(c) && R.coin()) {
        ok(c, picles_track_info(c, &im, nullptr, nullptr), "track_info");
        ok(c, picles_track_fetch_begin(c, 0, im), "fetch_begin before destroy");
        g_open_destroyed++;
    }
    ok(c, picles_destroy(c), "destroy");      /* with a set, maybe with an open fetch */

    /* slab mode, either way round, on a context that has not been seeded (the mode cannot change afterwards) */
    c = make_context(R, g, false, false);
    if (!c) die("picles_create");
    const Events s = make_events(R, g, R.in(1, 20));
    ok(c, init(c, s, DT), "init before the seed");
    refused(c, picles_set_slab_mode(c, 1), "slab mode on a context with a set", -5);
    ok(c, picles_track_free(c), "track_free");
    ok(c, picles_set_slab_mode(c, 1), "slab mode");
    refused(c, init(c, s, DT), "init in slab mode", -5);
    if (has_set(c)) die("a set in slab mode");
    ok(c, picles_set_slab_mode(c, 0), "slab mode off");
    ok(c, init(c, s, DT), "init out of slab mode");
    ok(c, picles_destroy(c), "destroy");
    /* a slab */
    c = make_context(R, g, true, true);
    if (!c) die("picles_create of a slab");
    refused(c, init(c, make_events(R, g, 3), DT), "init on a slab", -5);
    ok(c, picles_destroy(c), "destroy");
    /* the native ring: a whole-grid context on a ring of one, through the loopback communicator (PICLES_CCL_LIB) */
    c = make_context(R, g, false, true);
    if (!c) die("picles_create");
    const Events q = make_events(R, g, R.in(1, 20));
    char uid[PICLES_SLAB_ID_BYTES];
    ok(c, picles_slab_unique_id(uid), "slab_unique_id");
    ok(c, picles_slab_comm_init(c, uid, 0, 1), "slab_comm_init");
    refused(c, init(c, q, DT), "init on the native ring", -5);
    if (has_set(c)) die("a set on the native ring");
    ok(c, picles_slab_run_steps(c, DT, R.in(1, 3), PICLES_STEP_ZERO_FIRST), "ring steps after the refusal");
    ok(c, picles_slab_comm_destroy(c), "slab_comm_destroy");
    ok(c, init(c, q, DT), "init after the ring has gone");
    ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "a step with the set");
    {
        int64_t n = -1;
        ok(c, picles_track_info(c, nullptr, nullptr, &n), "track_info");
        if (n != 1) die("samples after the ring");
    }
    g_ring++;
    ok(c, picles_destroy(c), "destroy");
}
}   // namespace

int main(int argc, char **argv)
{
    const uint64_t first = argc > 1 ? strtoull(argv[1], nullptr, 10) : 0, count = argc > 2 ? strtoull(argv[2], nullptr, 10) : 120;
    if (picles_abi_version() != PICLES_ABI_VERSION) { fprintf(stderr, "ABI version\n"); return 2; }
    for (uint64_t s = first; s < first + count; s++) program(s);
    if (count >= 50 && (g_failed_inits < 6 * (long)count || g_grown < 2 * (long)count || g_failed_grow == 0 || g_open_destroyed == 0 || g_long_steps == 0 || g_ring != (long)count)) {
        fprintf(stderr, "track harness: too few failed inits (%ld), staging growths (%ld), failed growths (%ld), contexts destroyed with an open "
                "fetch (%ld) or refused long steps (%ld)\n", g_failed_inits, g_grown, g_failed_grow, g_open_destroyed, g_long_steps);
        return 3;
    }
    printf("track harness: %llu programs, %ld ABI calls, %ld refused as documented, %ld inits failed by a creation and undone, %ld fetches, "
           "staging grown %ld times (%ld growths failed first), %ld contexts destroyed with an open fetch, %ld inits refused on the native ring; "
           "no sanitizer report\n",
           (unsigned long long)count, g_calls, g_refused, g_failed_inits, g_fetches, g_grown, g_failed_grow, g_open_destroyed, g_ring);
    return 0;
}
