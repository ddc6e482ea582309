// nest_restart_harness.cpp — the host side of picles_nest_set_levels (a nested pair resumed from a checkpoint) under AddressSanitizer,
// on top of fake_hip.cpp like nest_harness.cpp.  One fixed program, no random numbers: a 12x9 parent and a 10x7 child, whole grids, an
// open rim on both; parent step 600 s, child step 200 s.
//   * a pair run 1, 2 and 3 child steps past a parent level, its two blobs and its pair taken into heap blocks of exactly the size the
//     contract names, loaded into new contexts, the set and the nest made again and the pair put back — one-way and with feedback —
//     and the resumed pair run on: the refused sample, the rest of the window, the third sample (rotates) and the fourth (claims the
//     slot a put-back level lay in);
//   * every refusal of the call, the texts compared, and behind each both contexts step on and nothing was left behind;
//   * the destroy orders after a resume: child first, parent first, picles_nest_free and picles_bforce_free in between.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_nest_restart.py).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/picles_hip.h"

extern "C" long fake_hip_live(void);      /* fake_hip.cpp */

namespace {
long g_calls = 0, g_refused = 0, g_resumed = 0, g_destroyed = 0;
const double DT = 600.0, DTC = 200.0;
const int PNX = 12, PNY = 9, CNX = 10, CNY = 7;

void die(const std::string &what) { fprintf(stderr, "nest restart harness: %s\n", what.c_str()); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "nest restart harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what, int code, const std::string &text)
{
    g_calls++; g_refused++;
    if (rc == 0) die(std::string(what) + " was not refused");
    if (rc != code) die(std::string(what) + " refused with " + std::to_string(rc) + ", not " + std::to_string(code));
    const std::string got = picles_last_error(c);
    if (got.find("picles_nest_set_levels") != 0 || got.find(text) == std::string::npos) die(std::string(what) + ": the text is \"" + got + "\", expected \"" + text + "\"");
}

picles_ctx *make_context(int Nx, int Ny)
{
    picles_grid g; picles_phys p; picles_ode o; picles_model m;
    memset(&g, 0, sizeof g); memset(&p, 0, sizeof p); memset(&o, 0, sizeof o); memset(&m, 0, sizeof m);
    g.Nx = Nx; g.Ny = Ny; g.dx = 2000.0; g.dy = 1500.0; g.mask = nullptr; g.j_begin = 0; g.j_end = Ny;
    p.r_g = 0.85; p.C_alpha = -1.41; p.C_phi = 0.04; p.C_e = 2.2117647058823533e-4; p.g = 9.81; p.gamma = 0.88; p.q = -0.25;
    p.c_beta = 0.04; p.c_D = 2e-3; p.c_e = 1.3e-6; p.c_alpha = 11.8;
    p.propagation = p.input = p.dissipation = p.peak_shift = p.direction = 1;
    o.abstol = 1e-4; o.reltol = 1e-3; o.dt0 = 1e-3; o.dtmin = 1e-4; o.force_dtmin = 1; o.solver = 0; o.maxiters = 10000;
    o.log_energy_minimum = -13.0; o.log_energy_maximum = 3.3; o.wind_min_squared = 4.0; o.timestep = 600.0;
    m.periodic_boundary = 0; m.minimal_state[0] = 1.25e-6; m.minimal_state[1] = 1.28e-9;
    picles_ctx *c = nullptr;
    g_calls++;
    if (picles_create(&g, &p, &o, &m, 0, 1, &c) != 0) die(std::string("picles_create: ") + picles_last_error(nullptr));
    const size_t N = (size_t)Nx * Ny;
    std::vector<double> u(N, 9.0), v(N, 4.0);
    ok(c, picles_set_winds(c, u.data(), v.data(), 0.0, nullptr, nullptr, 0.0), "set_winds");
    ok(c, picles_seed(c, 0.0), "seed");
    return c;
}
void destroy(picles_ctx *c, const char *what) { ok(nullptr, picles_destroy(c), what); g_destroyed++; }

/* ---- the geometry of nest_harness.cpp: exact-size heap blocks ---- */
struct Geometry {
    int n = 0, n_corner = 20, n_fb = 6, n_src = 12, m = 3;
    std::vector<int32_t> rim, corner_ij, index, fb_ij, src_ij, fb_index;
    std::vector<double> weight, fb_weight;
    Geometry()
    {
        std::vector<int32_t> i, j;
        for (int y = 0; y < CNY; y++)
            for (int x = 0; x < CNX; x++)
                if (x == 0 || y == 0 || x == CNX - 1 || y == CNY - 1) { i.push_back(x); j.push_back(y); }
        n = (int)i.size();
        rim.reserve((size_t)2 * n);
        rim.insert(rim.end(), i.begin(), i.end());
        rim.insert(rim.end(), j.begin(), j.end());
        corner_ij.resize((size_t)2 * n_corner);
        for (int k = 0; k < n_corner; k++) { corner_ij[k] = 1 + k % 10; corner_ij[n_corner + k] = 1 + k / 10; }
        index.resize((size_t)4 * n);
        weight.resize((size_t)4 * n);
        for (int c = 0; c < 4; c++)
            for (int k = 0; k < n; k++) { index[(size_t)c * n + k] = (k + 3 * c) % n_corner; weight[(size_t)c * n + k] = (k % 7 == 3 && c == 1) ? 0.0 : 0.25; }
        fb_ij.resize((size_t)2 * n_fb);
        for (int k = 0; k < n_fb; k++) { fb_ij[k] = 4 + k % 3; fb_ij[n_fb + k] = 3 + k / 3; }
        src_ij.resize((size_t)2 * n_src);
        for (int k = 0; k < n_src; k++) { src_ij[k] = 1 + k % 4; src_ij[n_src + k] = 1 + k / 4; }
        fb_index.resize((size_t)m * n_fb);
        fb_weight.resize((size_t)m * n_fb);
        for (int c = 0; c < m; c++)
            for (int k = 0; k < n_fb; k++) { fb_index[(size_t)c * n_fb + k] = (2 * k + c) % n_src; fb_weight[(size_t)c * n_fb + k] = (c == 2 && k % 2) ? 0.0 : 0.5; }
    }
};
const Geometry &G() { static const Geometry g; return g; }

void set_and_nest(picles_ctx *c, picles_ctx *p)
{
    ok(c, picles_bforce_init(c, G().n, G().rim.data()), "bforce_init");
    ok(c, picles_nest_init(c, p, G().n_corner, G().corner_ij.data(), G().index.data(), G().weight.data()), "nest_init");
}
int feedback_init(picles_ctx *c)
{
    return picles_nest_feedback_init(c, G().n_fb, G().fb_ij.data(), G().n_src, G().src_ij.data(), G().m, G().fb_index.data(), G().fb_weight.data());
}

/* what a pair checkpoint holds: two blobs and the pair, each in a heap block of exactly its size */
struct Saved {
    std::vector<unsigned char> child, parent;
    double t0 = 0, t1 = 0;
    std::vector<double> v0, v1;
    long child_steps = 0;          /* child steps past the parent level t0 */
};
void blob_of(picles_ctx *c, std::vector<unsigned char> &b)
{
    size_t bytes = 0;
    ok(c, picles_checkpoint_size(c, &bytes), "checkpoint_size");
    b.assign(bytes, 0);
    std::vector<unsigned char>(b).swap(b);      /* capacity == size */
    ok(c, picles_checkpoint_begin(c), "checkpoint_begin");
    ok(c, picles_checkpoint_end(c, b.data(), bytes), "checkpoint_end");
}
void info_is(picles_ctx *c, int levels, double t0, double t1, long samples, const char *what)
{
    int32_t n = 0, lv = -1, nc = 0; double a = -1, b = -1; int64_t s = -1;
    ok(c, picles_bforce_info(c, &n, &lv, &a, &b), "bforce_info");
    ok(c, picles_nest_info(c, &nc, &s), "nest_info");
    if (n != G().n || lv != levels || a != t0 || b != t1 || s != samples || nc != G().n_corner) die(std::string(what) + ": the set or the nest is not what it should be");
}

/* a pair run `past` child steps past the parent level t = 600 (3: onto the next one), with the parent one step ahead as NestForcing keeps it */
Saved run_and_save(int past, bool feedback)
{
    picles_ctx *p = make_context(PNX, PNY), *c = make_context(CNX, CNY);
    set_and_nest(c, p);
    ok(c, picles_nest_sample(c), "nest_sample (level 0)");
    if (feedback) { ok(c, feedback_init(c), "nest_feedback_init"); ok(c, picles_nest_feedback(c), "nest_feedback (seed)"); ok(c, picles_nest_feedback(c), "nest_feedback"); }
    ok(p, picles_run_steps(p, DT, 1), "run_steps (parent)");
    ok(c, picles_nest_sample(c), "nest_sample (level 1)");
    ok(c, picles_run_steps(c, DTC, 3), "run_steps (child: the first window)");
    if (feedback) ok(c, picles_nest_feedback(c), "nest_feedback");
    ok(p, picles_run_steps(p, DT, 1), "run_steps (parent)");
    ok(c, picles_nest_sample(c), "nest_sample (rotates)");
    ok(c, picles_run_steps(c, DTC, past), "run_steps (child: into the second window)");
    Saved S;
    S.child_steps = past;
    blob_of(c, S.child);
    blob_of(p, S.parent);
    int32_t n = 0, lv = 0;
    ok(c, picles_bforce_info(c, &n, &lv, &S.t0, &S.t1), "bforce_info");
    if (lv != 2 || S.t0 != DT || S.t1 != 2 * DT || picles_clock(p) != S.t1) die("the pair a checkpoint finds");
    S.v0.assign((size_t)3 * n, 0.0); S.v1.assign((size_t)3 * n, 0.0);
    std::vector<double>(S.v0).swap(S.v0); std::vector<double>(S.v1).swap(S.v1);
    ok(c, picles_bforce_get_levels(c, S.v0.data(), S.v1.data()), "bforce_get_levels");
    S.v0[1] = S.v0[(size_t)n + 1] = S.v0[(size_t)2 * n + 1] = __builtin_nan("0x5a5a");      /* a NaN level row, with a payload */
    if (past % 2) { destroy(c, "destroy (child first)"); destroy(p, "destroy (parent)"); }
    else { destroy(p, "destroy (parent first)"); destroy(c, "destroy (child)"); }
    return S;
}

struct Resumed { picles_ctx *p, *c; };
Resumed resume(const Saved &S, bool feedback)
{
    Resumed R{make_context(PNX, PNY), make_context(CNX, CNY)};
    ok(R.c, picles_checkpoint_load(R.c, S.child.data(), S.child.size()), "checkpoint_load (child)");
    ok(R.p, picles_checkpoint_load(R.p, S.parent.data(), S.parent.size()), "checkpoint_load (parent)");
    if (picles_clock(R.p) != S.t1 || picles_clock(R.c) != S.t0 + S.child_steps * DTC) die("the clocks the blobs bring");
    set_and_nest(R.c, R.p);
    info_is(R.c, 0, 0.0, 0.0, 0, "a fresh nest");
    ok(R.c, picles_nest_set_levels(R.c, S.t0, S.v0.data(), S.t1, S.v1.data()), "nest_set_levels");
    info_is(R.c, 2, S.t0, S.t1, 2, "behind nest_set_levels");
    std::vector<double> a(S.v0.size()), b(S.v1.size());
    ok(R.c, picles_bforce_get_levels(R.c, a.data(), b.data()), "bforce_get_levels");
    if (memcmp(a.data(), S.v0.data(), a.size() * sizeof(double)) || memcmp(b.data(), S.v1.data(), b.size() * sizeof(double))) die("the pair did not come back verbatim");
    if (feedback) ok(R.c, feedback_init(R.c), "nest_feedback_init (no seed feedback)");
    g_resumed++;
    return R;
}
/* the resumed pair runs on as the uninterrupted one would: the rest of the window, the feedback on the common clock in front of the
 * parent's step, the third sample, a window, the fourth sample */
void run_on(Resumed &R, const Saved &S, bool feedback)
{
    g_calls++; g_refused++;
    if (picles_nest_sample(R.c) != -2 || !strstr(picles_last_error(R.c), "has not moved past")) die("a sample before the parent has stepped");
    if (S.child_steps < 3) ok(R.c, picles_run_steps(R.c, DTC, 3 - (int)S.child_steps), "run_steps (child: the rest of the window)");
    for (int k = 0; k < 2; k++) {
        if (feedback) ok(R.c, picles_nest_feedback(R.c), "nest_feedback (in front of the parent's step)");
        ok(R.p, picles_run_steps(R.p, DT, 1), "run_steps (parent)");
        ok(R.c, picles_nest_sample(R.c), k ? "nest_sample (the fourth)" : "nest_sample (the third: rotates)");
        info_is(R.c, 2, S.t1 + k * DT, S.t1 + (k + 1) * DT, 3 + k, "behind a sample of the resumed nest");
        ok(R.c, picles_run_steps(R.c, DTC, 3), "run_steps (child: a window)");
    }
    std::vector<double> s((size_t)3 * CNX * CNY);
    ok(R.c, picles_get_state(R.c, s.data()), "get_state (child)");
}

void resumes()
{
    int variant = 0;
    for (int fb = 0; fb < 2; fb++)
        for (int past = 1; past <= 3; past++, variant++) {
            const Saved S = run_and_save(past, fb);
            Resumed R = resume(S, fb);
            run_on(R, S, fb);
            switch (variant % 6) {
            case 0: destroy(R.c, "destroy (child first)"); destroy(R.p, "destroy (parent)"); break;
            case 1: destroy(R.p, "destroy (parent first)"); ok(R.c, picles_run_steps(R.c, DTC, 1), "run_steps (child, its parent gone)"); destroy(R.c, "destroy (child)"); break;
            case 2: ok(R.c, picles_nest_free(R.c), "nest_free"); ok(R.c, picles_run_steps(R.c, DTC, 1), "run_steps (child, under the kept pair)");
                    destroy(R.c, "destroy (child)"); destroy(R.p, "destroy (parent)"); break;
            case 3: ok(R.c, picles_bforce_free(R.c), "bforce_free (the feedback and the nest go with it)"); destroy(R.p, "destroy (parent first)"); destroy(R.c, "destroy (child)"); break;
            case 4: ok(R.c, picles_nest_feedback_free(R.c), "nest_feedback_free"); destroy(R.c, "destroy (child first)"); destroy(R.p, "destroy (parent)"); break;
            default: destroy(R.p, "destroy (parent first, feedback alive)"); destroy(R.c, "destroy (child)"); break;
            }
        }
    /* destroyed right behind the call, nothing run: either order */
    for (int order = 0; order < 2; order++) {
        const Saved S = run_and_save(2, order);
        Resumed R = resume(S, order);
        destroy(order ? R.p : R.c, "destroy (behind the resume)");
        destroy(order ? R.c : R.p, "destroy (the other)");
    }
}

void refusals()
{
    const Saved S = run_and_save(2, false);
    picles_ctx *p = make_context(PNX, PNY), *c = make_context(CNX, CNY);
    ok(c, picles_checkpoint_load(c, S.child.data(), S.child.size()), "checkpoint_load (child)");
    ok(p, picles_checkpoint_load(p, S.parent.data(), S.parent.size()), "checkpoint_load (parent)");
    const int n = G().n;
    const double *v0 = S.v0.data(), *v1 = S.v1.data();
    std::vector<double> level((size_t)3 * n, 0.5);
    long live = 0;
    double t1 = S.t1;
    /* a step of both; the child under a level of its own, since a refusal left its nest without levels.  Then a fresh nest again */
    auto behind = [&](const char *what, bool nested = true) {
        if (fake_hip_live() != live) die(std::string(what) + " left something behind");
        ok(p, picles_run_steps(p, DT, 1), "run_steps (parent)");
        t1 += DT;
        ok(c, picles_bforce_free(c), "bforce_free");
        ok(c, picles_bforce_init(c, n, G().rim.data()), "bforce_init");
        ok(c, picles_bforce_set_levels(c, 0.0, level.data(), 0.0, nullptr), "bforce_set_levels");
        ok(c, picles_run_steps(c, DTC, 1), "run_steps (child)");
        if (nested) ok(c, picles_nest_init(c, p, G().n_corner, G().corner_ij.data(), G().index.data(), G().weight.data()), "nest_init");
        live = fake_hip_live();
    };
    if (picles_nest_set_levels(nullptr, S.t0, v0, S.t1, v1) != -1) die("a NULL context");
    ok(c, picles_bforce_init(c, n, G().rim.data()), "bforce_init");
    live = fake_hip_live();
    refused(c, picles_nest_set_levels(c, t1 - DT, v0, t1, v1), "a child without a nest", -2, "picles_nest_init first"); behind("a child without a nest");
    refused(c, picles_nest_set_levels(c, t1 - DT, nullptr, t1, v1), "no level 0", -2, "both levels must be given"); behind("no level 0");
    refused(c, picles_nest_set_levels(c, t1 - DT, v0, t1, nullptr), "no level 1", -2, "both levels must be given"); behind("no level 1");
    const double bad[3] = {__builtin_nan(""), __builtin_inf(), -__builtin_inf()};
    for (double b : bad) {
        refused(c, picles_nest_set_levels(c, b, v0, t1, v1), "t0 not finite", -2, "the level times must be finite"); behind("t0 not finite");
        refused(c, picles_nest_set_levels(c, t1 - DT, v0, b, v1), "t1 not finite", -2, "the level times must be finite"); behind("t1 not finite");
    }
    refused(c, picles_nest_set_levels(c, t1, v0, t1, v1), "t1 == t0", -2, "the pair needs t1 > t0"); behind("t1 == t0");
    refused(c, picles_nest_set_levels(c, t1 + DT, v0, t1, v1), "t1 < t0", -2, "the pair needs t1 > t0"); behind("t1 < t0");
    refused(c, picles_nest_set_levels(c, t1 - DT, v0, t1 + DT, v1), "the parent's clock behind t1", -2, "is not t1"); behind("the parent's clock behind t1");
    refused(c, picles_nest_set_levels(c, t1 - 2 * DT, v0, t1 - DT, v1), "the parent's clock past t1", -2, "is not t1"); behind("the parent's clock past t1");
    refused(c, picles_nest_set_levels(c, t1 - DT, v0, std::nextafter(t1, 0.0), v1), "the parent's clock one ulp off t1", -2, "is not t1"); behind("one ulp off");
    ok(c, picles_nest_sample(c), "nest_sample");
    refused(c, picles_nest_set_levels(c, t1 - DT, v0, t1, v1), "a nest that has sampled", -2, "has taken 1 sample(s)");
    ok(c, picles_run_steps(c, DTC, 1), "run_steps (child, under the sampled level)");
    live = fake_hip_live();
    behind("a nest that has sampled");
    ok(c, picles_nest_set_levels(c, t1 - DT, v0, t1, v1), "nest_set_levels behind the refusals");
    refused(c, picles_nest_set_levels(c, t1 - DT, v0, t1, v1), "a second call", -2, "has taken 2 sample(s)");
    g_calls++; g_refused++;
    if (picles_bforce_set_levels(c, 0.0, level.data(), 0.0, nullptr) != -2 || !strstr(picles_last_error(c), "picles_nest_free first")) die("bforce_set_levels with a nest is refused as before");
    {   /* caller-provided streams: the child has run on one since its nest was made */
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, 0) != hipSuccess) die("stream");
        picles_ctx *x = make_context(CNX, CNY);
        set_and_nest(x, p);
        ok(x, picles_stat_init(x, PICLES_STAT_MEAN, 0, nullptr, 1, 1), "stat_init");
        ok(x, picles_stat_update(x, s), "stat_update on a caller's stream");
        refused(x, picles_nest_set_levels(x, t1 - DT, v0, t1, v1), "a child that ran on a caller's stream", -2, "caller-provided streams");
        destroy(x, "destroy");
        if (hipStreamDestroy(s) != hipSuccess) die("stream");
    }
    {   /* a nest whose parent was destroyed */
        picles_ctx *q = make_context(PNX, PNY), *x = make_context(CNX, CNY);
        set_and_nest(x, q);
        destroy(q, "destroy (parent)");
        refused(x, picles_nest_set_levels(x, -DT, v0, 0.0, v1), "a nest whose parent was destroyed", -2, "the parent context was destroyed");
        ok(x, picles_nest_free(x), "nest_free");
        ok(x, picles_bforce_set_levels(x, 0.0, level.data(), 0.0, nullptr), "bforce_set_levels");
        ok(x, picles_run_steps(x, DTC, 1), "run_steps (child, its parent gone)");
        destroy(x, "destroy (child)");
    }
    destroy(c, "destroy (child)");
    destroy(p, "destroy (parent)");
}
}   // namespace

int main()
{
    if (picles_abi_version() != PICLES_ABI_VERSION || PICLES_ABI_VERSION < 16) { fprintf(stderr, "ABI version\n"); return 2; }
    const long live = fake_hip_live();
    resumes();
    refusals();
    if (fake_hip_live() != live) die("blocks or events alive at the end");
    if (g_resumed < 8) die("too few pairs resumed");
    printf("nest restart harness: %ld ABI calls, %ld refused as documented, %ld pairs resumed, %ld contexts destroyed, no sanitizer report\n",
           g_calls, g_refused, g_resumed, g_destroyed);
    return 0;
}
