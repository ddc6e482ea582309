// stat_harness.cpp — the host side of the run statistics (picles_stat_*) under AddressSanitizer, on top of fake_hip.cpp like
// probe_harness.cpp: seeded programs of init / steps / update / get / set / reset / free for whole-grid and slab contexts.  Every
// buffer handed to picles_stat_get and picles_stat_set has exactly the size of the plane block of the call's mask: a copy that
// assumes the whole set's block, another threshold count or another node count is an ASan report.  The fake runtime copies for
// real, so a plane block written with picles_stat_set must come back from picles_stat_get byte for byte, whole and by group — which
// pins the offsets of the pieces —, and picles_stat_reset must leave zeros.  The kernels are launch stubs here: the planes change
// through set and reset alone, the host-side scalars through every update.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_stat.py).
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
long g_calls = 0, g_refused = 0, g_gets = 0, g_sets = 0, g_updates = 0, g_slabs = 0;
void die(const char *what) { fprintf(stderr, "stat harness: %s\n", what); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "stat harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what, int code = -2)
{
    g_calls++; g_refused++;
    if (rc == 0) { fprintf(stderr, "stat harness: %s was not refused\n", what); exit(3); }
    if (rc != code) { fprintf(stderr, "stat harness: %s refused with %d, not %d\n", what, rc, code); exit(3); }
    if (!picles_last_error(c)[0]) { fprintf(stderr, "stat harness: %s refused without a text\n", what); exit(3); }
}

/* bytes of the plane block of `mask` (the header's formula) */
size_t block_bytes(size_t N, int mask, int nthr)
{
    return N * (8 * (size_t)(((mask & PICLES_STAT_PEAK) ? 4 : 0) + ((mask & PICLES_STAT_MEAN) ? 4 : 0)) +
                4 * (size_t)(1 + ((mask & PICLES_STAT_EXCEED) ? nthr : 0)));
}

/* the byte every plane of the whole set is filled with: plane p of the set's block (in its order), salted */
struct Plane { int group; size_t bytes; unsigned char fill; };
std::vector<Plane> planes_of(size_t N, int mask, int nthr, unsigned char salt)
{
    std::vector<Plane> v;
    unsigned char p = 0;
    if (mask & PICLES_STAT_PEAK) for (int k = 0; k < 4; k++) v.push_back({PICLES_STAT_PEAK, N * 8, (unsigned char)(salt + ++p)});
    if (mask & PICLES_STAT_MEAN) for (int k = 0; k < 4; k++) v.push_back({PICLES_STAT_MEAN, N * 8, (unsigned char)(salt + ++p)});
    v.push_back({0, N * 4, (unsigned char)(salt + ++p)});
    if (mask & PICLES_STAT_EXCEED) for (int k = 0; k < nthr; k++) v.push_back({PICLES_STAT_EXCEED, N * 4, (unsigned char)(salt + ++p)});
    return v;
}

/* the block of sub-mask `sub` of a set whose planes hold their fill bytes */
std::vector<unsigned char> expected_block(const std::vector<Plane> &all, int sub)
{
    std::vector<unsigned char> b;
    for (const Plane &p : all)
        if (p.group == 0 || (p.group & sub)) b.insert(b.end(), p.bytes, p.fill);
    return b;
}

/* n model steps through an entry point that fits the context; a slab updates by itself behind its split-phase steps */
int step(picles_ctx *c, bool whole, Rng &R, int n, int every, int first, long long &s, long long &updates)
{
    if (whole) {
        int rc = (n == 1 && R.coin()) ? picles_time_step(c, 600.0, R.coin() ? PICLES_STEP_ZERO_FIRST : 0) : picles_run_steps(c, 600.0, n);
        if (rc) return rc;
        for (int k = 0; k < n; k++) { s++; if (every && s >= first && (s - first) % every == 0) updates++; }
        return 0;
    }
    for (int k = 0; k < n; k++) {
        int rc = picles_begin_step(c, 600.0, PICLES_STEP_ZERO_FIRST);
        if (!rc) rc = picles_advance_rows(c, PICLES_ROWS_ALL, nullptr);
        if (!rc) rc = picles_scatter_remesh(c, nullptr);
        if (rc) return rc;
        s++;
    }
    return 0;
}

void check_scalars(picles_ctx *c, int mask, size_t N, int nthr, long long want_samples)
{
    /* exactly the n_wet plane, and the scalars */
    unsigned char *b = (unsigned char *)malloc(block_bytes(N, 0, nthr));
    int64_t n = -1; double t0 = -1.0, t1 = -1.0;
    ok(c, picles_stat_get(c, 0, b, &n, &t0, &t1), "stat_get (n_wet alone)");
    g_gets++;
    if (n != want_samples) { fprintf(stderr, "stat harness: n_samples %lld, expected %lld\n", (long long)n, want_samples); exit(3); }
    if (want_samples == 0 && (t0 != 0.0 || t1 != 0.0)) die("clocks of an empty set");
    if (want_samples > 0 && !(t0 <= t1 && t1 <= picles_clock(c))) die("clocks of the samples");
    free(b);
    (void)mask;
}

void program(uint64_t seed)
{
    Rng R(0x9E3779B97F4A7C15ull * (seed + 1));
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
    if (!whole) g_slabs++;
    const size_t N = (size_t)Nx * ny;
    double *u = (double *)malloc(N * 8), *v = (double *)malloc(N * 8);
    for (size_t k = 0; k < N; k++) { u[k] = 9.0; v[k] = 4.0; }
    ok(c, picles_set_winds(c, u, v, 0.0, nullptr, nullptr, 0.0), "set_winds");
    ok(c, picles_seed(c, 0.0), "seed");
    free(u); free(v);

    /* without a set */
    unsigned char one[8];
    refused(c, picles_stat_update(c, nullptr), "update without a set");
    refused(c, picles_stat_get(c, 0, one, nullptr, nullptr, nullptr), "get without a set");
    refused(c, picles_stat_set(c, 0, one, 0, 0.0, 0.0), "set without a set");
    refused(c, picles_stat_reset(c), "reset without a set");
    if (picles_stat_shape(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) die("shape without a set");
    ok(c, picles_stat_free(c), "free without a set");

    /* the refusals of init: exactly n thresholds are readable */
    const int mask = R.in(1, 7), nthr = (mask & PICLES_STAT_EXCEED) ? R.in(1, 4) : 0;
    const int every = R.in(1, 3), first = R.in(1, 3);
    double *thr = (double *)malloc((size_t)(nthr ? nthr : 1) * 8);
    for (int k = 0; k < nthr; k++) thr[k] = 0.5 * (k + 1);
    refused(c, picles_stat_init(c, 0, 0, nullptr, every, first), "empty mask");
    refused(c, picles_stat_init(c, 8 | mask, nthr, thr, every, first), "unknown mask bit");
    refused(c, picles_stat_init(c, mask, nthr, thr, 0, first), "every = 0");
    refused(c, picles_stat_init(c, mask, nthr, thr, every, 0), "first = 0");
    if (mask & PICLES_STAT_EXCEED) {
        refused(c, picles_stat_init(c, mask, 0, thr, every, first), "EXCEED without thresholds");
        refused(c, picles_stat_init(c, mask, nthr, nullptr, every, first), "EXCEED with a NULL list");
        double five[5] = {1, 2, 3, 4, 5};
        refused(c, picles_stat_init(c, mask, 5, five, every, first), "five thresholds");
        double *bad = (double *)malloc((size_t)nthr * 8);
        memcpy(bad, thr, (size_t)nthr * 8);
        const int k = R.in(0, nthr - 1);
        switch (R.in(0, 3)) {
        case 0: bad[k] = 0.0; break;
        case 1: bad[k] = -1.0; break;
        case 2: bad[k] = __builtin_inf(); break;
        default: bad[k] = (k > 0) ? bad[k - 1] : __builtin_nan(""); break;
        }
        refused(c, picles_stat_init(c, mask, nthr, bad, every, first), "thresholds that break the rule");
        free(bad);
    } else {
        double t1[1] = {1.0};
        refused(c, picles_stat_init(c, mask, 1, t1, every, first), "thresholds without EXCEED");
    }
    if (picles_stat_shape(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0) die("a refused init left a set behind");
    ok(c, picles_stat_init(c, mask, nthr, thr, every, first), "stat_init");
    refused(c, picles_stat_init(c, mask, nthr, thr, every, first), "init twice");
    {
        int32_t sm, sn, se, sp; size_t sb; double st[4];
        ok(c, picles_stat_shape(c, &sm, &sn, st, &se, &sp, &sb), "stat_shape");
        if (sm != mask || sn != nthr || se != every || sb != block_bytes(N, mask, nthr)) die("shape");
        if (sp != ((mask & 1) ? 4 : 0) + ((mask & 2) ? 4 : 0) + 1 + nthr) die("plane count");
        for (int k = 0; k < nthr; k++) if (st[k] != thr[k]) die("thresholds of shape");
    }
    free(thr);
    refused(c, picles_stat_get(c, mask, nullptr, nullptr, nullptr, nullptr), "get into NULL");
    refused(c, picles_stat_set(c, mask, nullptr, 0, 0.0, 0.0), "set from NULL");
    if (mask != 7) {
        refused(c, picles_stat_get(c, 7, one, nullptr, nullptr, nullptr), "get of a group the set lacks");
        refused(c, picles_stat_set(c, 7 & ~mask, one, 0, 0.0, 0.0), "set of a group the set lacks");
    }
    refused(c, picles_stat_set(c, 0, one, -1, 0.0, 0.0), "negative n_samples");
    check_scalars(c, mask, N, nthr, 0);

    long long s = 0, samples = 0;
    unsigned char salt = 0;
    bool filled = false;
    const int nops = R.in(8, 30);
    for (int k = 0; k < nops; k++) {
        switch (R.in(0, 5)) {
        case 0: case 1: {
            long long upd = 0;
            ok(c, step(c, whole, R, R.in(1, 4), every, first, s, upd), "steps");
            samples += upd;                       /* the split-phase calls of a slab count and do not update */
            g_updates += upd;
        } break;
        case 2:
            ok(c, picles_stat_update(c, nullptr), "stat_update");
            samples++; g_updates++;
            break;
        case 3: {                                 /* upload the whole set's block, or one group's, from an exact-size buffer */
            const int sub = R.coin() ? mask : (mask & R.in(0, 7));
            if (sub == mask || !filled) {
                salt = (unsigned char)R.in(1, 200);
                const std::vector<Plane> all = planes_of(N, mask, nthr, salt);
                std::vector<unsigned char> blk = expected_block(all, mask);
                if (blk.size() != block_bytes(N, mask, nthr)) die("block size");
                unsigned char *b = (unsigned char *)malloc(blk.size());
                memcpy(b, blk.data(), blk.size());
                samples = R.in(0, 1000);
                ok(c, picles_stat_set(c, mask, b, samples, 0.0, picles_clock(c)), "stat_set (whole set)");
                free(b);
                filled = true;
            } else {                              /* a group alone: the same fill bytes again, from a buffer of that group's size */
                std::vector<unsigned char> blk = expected_block(planes_of(N, mask, nthr, salt), sub);
                unsigned char *b = (unsigned char *)malloc(blk.size());
                memcpy(b, blk.data(), blk.size());
                ok(c, picles_stat_set(c, sub, b, samples, 0.0, picles_clock(c)), "stat_set (groups)");
                free(b);
            }
            g_sets++;
        } break;
        case 4: {                                 /* read a random selection back into an exact-size buffer */
            const int sub = mask & R.in(0, 7);
            const size_t bytes = block_bytes(N, sub, nthr);
            unsigned char *b = (unsigned char *)malloc(bytes);
            int64_t n = -1;
            ok(c, picles_stat_get(c, sub, b, &n, nullptr, nullptr), "stat_get");
            g_gets++;
            if (n != samples) die("n_samples of get");
            if (filled) {
                std::vector<unsigned char> want = expected_block(planes_of(N, mask, nthr, salt), sub);
                if (want.size() != bytes || memcmp(want.data(), b, bytes) != 0) die("get does not return what set uploaded");
            } else {
                for (size_t q = 0; q < bytes; q++) if (b[q]) die("planes not zero before any upload");
            }
            free(b);
        } break;
        default:
            ok(c, picles_stat_reset(c), "stat_reset");
            samples = 0; filled = false;
            check_scalars(c, mask, N, nthr, 0);
            break;
        }
    }
    check_scalars(c, mask, N, nthr, samples);
    if (R.coin()) {
        ok(c, picles_stat_update(c, nullptr), "update before free");
        ok(c, picles_stat_free(c), "free with updates issued");
        refused(c, picles_stat_update(c, nullptr), "update after free");
        if (R.coin()) {
            ok(c, picles_stat_init(c, PICLES_STAT_MEAN, 0, nullptr, 1, 1), "a new set after free");
            long long upd = 0, s2 = 0;
            ok(c, step(c, whole, R, 2, 1, 1, s2, upd), "steps of the new set");
            check_scalars(c, PICLES_STAT_MEAN, N, 0, whole ? 2 : 0);
        }
    } else {
        ok(c, picles_stat_update(c, nullptr), "update before destroy");
    }
    ok(c, picles_destroy(c), "destroy");      /* with updates issued */
}
}   // namespace

int main(int argc, char **argv)
{
    const uint64_t first = argc > 1 ? strtoull(argv[1], nullptr, 10) : 0, count = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    if (picles_abi_version() != PICLES_ABI_VERSION) { fprintf(stderr, "ABI version\n"); return 2; }
    for (uint64_t s = first; s < first + count; s++) program(s);
    if (count >= 100 && (g_gets == 0 || g_sets == 0 || g_updates == 0 || g_slabs == 0)) {
        fprintf(stderr, "stat harness: nothing read (%ld), uploaded (%ld) or updated (%ld), or no slab met (%ld)\n", g_gets, g_sets, g_updates, g_slabs);
        return 3;
    }
    printf("stat harness: %llu programs, %ld ABI calls, %ld refused as documented, %ld gets, %ld sets, %ld updates, %ld slab contexts, "
           "no sanitizer report\n", (unsigned long long)count, g_calls, g_refused, g_gets, g_sets, g_updates, g_slabs);
    return 0;
}
