// prolong_harness.cpp — the host side of picles_nest_prolong (a child started from its parent) under AddressSanitizer, on top of
// fake_hip.cpp like nest_harness.cpp.  One fixed program, no random numbers: a 12x9 periodic parent and a 10x7 open child, whole grids.
//   * the call through success, with every table on the heap at exactly the size the contract names, with the parent's step
//     pending and with none, and a second and third call on the same pair (the device copy of the tables is reused);
//   * every refusal a single fake device can reach — the texts of the table checks compared to the byte — and behind each both
//     contexts step on and nothing was left behind (fake_hip_live);
//   * every creation the call makes failed in turn: the call fails, nothing is left behind, the clocks stand where they stood, both
//     contexts step, and the same call then succeeds;
//   * picles_destroy of either context first afterwards, and of a child that was never started.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_prolong.py).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/picles_hip.h"

extern "C" long fake_hip_fail_alloc(long k);      /* fake_hip.cpp */
extern "C" long fake_hip_live(void);

namespace {
long g_calls = 0, g_refused = 0, g_started = 0, g_failed = 0, g_destroyed = 0;
const double DT = 600.0, DTC = 200.0;
const int PNX = 12, PNY = 9, CNX = 10, CNY = 7;

void die(const std::string &what) { fprintf(stderr, "prolong harness: %s\n", what.c_str()); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "prolong harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what, int code, const std::string &text, bool exact = false)
{
    g_calls++; g_refused++;
    if (rc == 0) die(std::string(what) + " was not refused");
    if (rc != code) die(std::string(what) + " refused with " + std::to_string(rc) + ", not " + std::to_string(code));
    const std::string got = picles_last_error(c);
    if (exact ? got != text : got.find(text) == std::string::npos) die(std::string(what) + ": the text is \"" + got + "\", expected \"" + text + "\"");
}

picles_ctx *make_context(int Nx, int Ny, int periodic, int j_begin = 0, int j_end = -1, bool seed = true)
{
    picles_grid g; picles_phys p; picles_ode o; picles_model m;
    memset(&g, 0, sizeof g); memset(&p, 0, sizeof p); memset(&o, 0, sizeof o); memset(&m, 0, sizeof m);
    g.Nx = Nx; g.Ny = Ny; g.dx = 2000.0; g.dy = 1500.0; g.periodic_x = periodic; g.periodic_y = periodic; g.mask = nullptr;
    g.j_begin = j_begin; g.j_end = j_end < 0 ? Ny : j_end;
    p.r_g = 0.85; p.C_alpha = -1.41; p.C_phi = 0.04; p.C_e = 2.2117647058823533e-4; p.g = 9.81; p.gamma = 0.88; p.q = -0.25;
    p.c_beta = 0.04; p.c_D = 2e-3; p.c_e = 1.3e-6; p.c_alpha = 11.8;
    p.propagation = p.input = p.dissipation = p.peak_shift = p.direction = 1;
    o.abstol = 1e-4; o.reltol = 1e-3; o.dt0 = 1e-3; o.dtmin = 1e-4; o.force_dtmin = 1; o.solver = 0; o.maxiters = 10000;
    o.log_energy_minimum = -13.0; o.log_energy_maximum = 3.3; o.wind_min_squared = 4.0; o.timestep = 600.0;
    m.periodic_boundary = periodic; m.minimal_state[0] = 1.25e-6; m.minimal_state[1] = 1.28e-9;
    picles_ctx *c = nullptr;
    g_calls++;
    if (picles_create(&g, &p, &o, &m, 0, 1, &c) != 0) die(std::string("picles_create: ") + picles_last_error(nullptr));
    const size_t N = (size_t)Nx * (g.j_end - g.j_begin);
    std::vector<double> u(N, 9.0), v(N, 4.0);
    ok(c, picles_set_winds(c, u.data(), v.data(), 0.0, nullptr, nullptr, 0.0), "set_winds");
    if (seed) ok(c, picles_seed(c, 0.0), "seed");
    return c;
}

/* the six tables, exact-size heap blocks: the child's columns run through the parent's wrap cell (11, 0) */
struct Tables {
    std::vector<int32_t> ix0, ix1, iy0, iy1;
    std::vector<double> wx, wy;
    Tables() : ix0(CNX), ix1(CNX), iy0(CNY), iy1(CNY), wx(CNX), wy(CNY)
    {
        for (int i = 0; i < CNX; i++) { ix0[i] = (5 + i) % PNX; ix1[i] = (6 + i) % PNX; wx[i] = i == 0 ? 0.0 : i == CNX - 1 ? 1.0 : 0.125 * (i % 8); }
        for (int j = 0; j < CNY; j++) { iy0[j] = 1 + j; iy1[j] = (2 + j) % PNY; wy[j] = 0.25 + 0.0625 * j; }
    }
};
int prolong(picles_ctx *c, picles_ctx *p, const Tables &T, double dt = DTC)
{
    return picles_nest_prolong(c, p, T.ix0.data(), T.ix1.data(), T.wx.data(), T.iy0.data(), T.iy1.data(), T.wy.data(), dt);
}
/* both contexts still work: each takes a step of its own and hands its State out */
void step_both(picles_ctx *p, picles_ctx *c)
{
    ok(p, picles_run_steps(p, DT, 1), "run_steps (parent)");
    ok(c, picles_run_steps(c, DTC, 1), "run_steps (child)");
    std::vector<double> s((size_t)3 * CNX * CNY);
    ok(c, picles_get_state(c, s.data()), "get_state (child)");
}
void started(picles_ctx *p, picles_ctx *c, const char *what)
{
    g_started++;
    if (picles_clock(c) != picles_clock(p)) die(std::string(what) + ": the child's clock is not the parent's");
    picles_counters k;
    ok(c, picles_get_counters(c, &k), "get_counters");
}

void success_and_again()
{
    picles_ctx *p = make_context(PNX, PNY, 1), *c = make_context(CNX, CNY, 0, 0, -1, false);      /* the child was never seeded */
    const Tables T;
    ok(p, picles_run_steps(p, DT, 3), "run_steps (parent: the spin-up, a step left pending)");
    ok(c, prolong(c, p, T), "nest_prolong (parent's step pending)");
    started(p, c, "first call");
    step_both(p, c); step_both(p, c);
    ok(p, picles_run_steps(p, DT, 1), "run_steps (parent)");
    ok(p, picles_sync(p), "sync (parent)");
    ok(c, prolong(c, p, T, DT), "nest_prolong (second call, nothing pending, another step length)");
    started(p, c, "second call");
    ok(c, prolong(c, p, T), "nest_prolong (third call, at once)");
    started(p, c, "third call");
    step_both(p, c);
    ok(nullptr, picles_destroy(c), "destroy (the child first)"); g_destroyed++;
    ok(p, picles_run_steps(p, DT, 1), "run_steps (parent, its child gone)");
    ok(nullptr, picles_destroy(p), "destroy (parent)"); g_destroyed++;
}

void refusals()
{
    picles_ctx *p = make_context(PNX, PNY, 1), *c = make_context(CNX, CNY, 0);
    const Tables T;
    const std::string W = "picles_nest_prolong: ";
    ok(p, picles_run_steps(p, DT, 2), "run_steps (parent)");
    const long live = fake_hip_live();
    const double clock = picles_clock(c);
    long stepped = 0;
    auto behind = [&](const char *what) {
        if (fake_hip_live() != live) die(std::string(what) + " left something behind");
        if (picles_clock(c) != clock + stepped * DTC) die(std::string(what) + " moved the child's clock");
        step_both(p, c);
        stepped++;
    };
    if (picles_nest_prolong(nullptr, p, T.ix0.data(), T.ix1.data(), T.wx.data(), T.iy0.data(), T.iy1.data(), T.wy.data(), DTC) != -1) die("a NULL context");
    behind("a NULL context");
    refused(c, prolong(c, nullptr, T), "no parent", -2, W + "no parent context given", true); behind("no parent");
    refused(c, prolong(c, c, T), "child == parent", -2, "child and parent are the same context"); behind("child == parent");
    refused(c, prolong(c, p, T, 0.0), "dt = 0", -2, W + "dt must be positive"); behind("dt = 0");
    refused(c, prolong(c, p, T, -__builtin_nan("")), "dt = NaN", -2, W + "dt must be positive"); behind("dt = NaN");
    refused(c, picles_nest_prolong(c, p, T.ix0.data(), T.ix1.data(), nullptr, T.iy0.data(), T.iy1.data(), T.wy.data(), DTC), "no wx", -2,
            W + "the six tables ix0, ix1, wx, iy0, iy1, wy must be given", true);
    behind("no wx");
    refused(c, picles_nest_prolong(c, p, T.ix0.data(), T.ix1.data(), T.wx.data(), T.iy0.data(), nullptr, T.wy.data(), DTC), "no iy1", -2,
            W + "the six tables ix0, ix1, wx, iy0, iy1, wy must be given", true);
    behind("no iy1");
    { Tables B; B.ix0[3] = PNX;
      refused(c, prolong(c, p, B), "a column off the parent", -2, W + "index 12 of the child's column 3 lies outside the parent's grid [0, 12)", true); behind("ix0"); }
    { Tables B; B.ix1[CNX - 1] = -1;
      refused(c, prolong(c, p, B), "a column off the parent", -2, W + "index -1 of the child's column 9 lies outside the parent's grid [0, 12)", true); behind("ix1"); }
    { Tables B; B.iy0[0] = PNY;
      refused(c, prolong(c, p, B), "a row off the parent", -2, W + "index 9 of the child's row 0 lies outside the parent's grid [0, 9)", true); behind("iy0"); }
    { Tables B; B.iy1[CNY - 1] = -7;
      refused(c, prolong(c, p, B), "a row off the parent", -2, W + "index -7 of the child's row 6 lies outside the parent's grid [0, 9)", true); behind("iy1"); }
    const double bad[4] = {__builtin_nan(""), __builtin_inf(), -0.25, 1.0 + 1e-12};
    for (double b : bad) {
        { Tables B; B.wx[CNX - 1] = b;
          refused(c, prolong(c, p, B), "a column weight outside [0, 1]", -2, W + "the weight of the child's column 9 is not finite or lies outside [0, 1]", true); behind("wx"); }
        { Tables B; B.wy[2] = b;
          refused(c, prolong(c, p, B), "a row weight outside [0, 1]", -2, W + "the weight of the child's row 2 is not finite or lies outside [0, 1]", true); behind("wy"); }
    }
    {   /* a slab as either end; a parent that was never seeded */
        picles_ctx *s = make_context(CNX, CNY, 0, 2, 6);
        refused(s, prolong(s, p, T), "a slab as a child", -5, W + "slabs, slab mode and the native ring do not nest: both contexts must be whole-grid contexts", true);
        refused(c, prolong(c, s, T), "a slab as a parent", -5, "slabs, slab mode and the native ring do not nest");
        ok(nullptr, picles_destroy(s), "destroy (slab)"); g_destroyed++;
        picles_ctx *q = make_context(PNX, PNY, 1, 0, -1, false);
        refused(c, prolong(c, q, T), "a parent never seeded", -2, W + "the parent was never seeded");
        ok(nullptr, picles_destroy(q), "destroy (unseeded)"); g_destroyed++;
        behind("a slab, a parent never seeded");
    }
    {   /* caller-provided streams */
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, 0) != hipSuccess) die("stream");
        picles_ctx *x = make_context(CNX, CNY, 0);
        ok(x, picles_stat_init(x, PICLES_STAT_MEAN, 0, nullptr, 1, 1), "stat_init");
        ok(x, picles_stat_update(x, s), "stat_update on a caller's stream");
        refused(x, prolong(x, p, T), "a child that ran on a caller's stream", -5, "picles_nest_prolong: a context that has run on caller-provided streams");
        ok(nullptr, picles_destroy(x), "destroy"); g_destroyed++;
        if (hipStreamDestroy(s) != hipSuccess) die("stream");
        behind("a caller's stream");
    }
    ok(c, prolong(c, p, T), "nest_prolong behind the refusals");
    started(p, c, "behind the refusals");
    step_both(p, c);
    ok(nullptr, picles_destroy(p), "destroy (the parent first)"); g_destroyed++;
    ok(c, picles_run_steps(c, DTC, 2), "run_steps (child, its parent gone)");
    ok(nullptr, picles_destroy(c), "destroy (child)"); g_destroyed++;
}

void failed_creations()
{
    picles_ctx *p = make_context(PNX, PNY, 1), *c = make_context(CNX, CNY, 0);
    const Tables T;
    ok(p, picles_run_steps(p, DT, 2), "run_steps (parent)");
    for (int round = 0; round < 2; round++) {      /* the first call creates the device copy of the tables; the second reuses it */
        int k = 1;
        for (;; k++) {
            const long live = fake_hip_live();
            const double clock = picles_clock(c);
            fake_hip_fail_alloc(k);
            const int rc = prolong(c, p, T);
            if (fake_hip_fail_alloc(0) > 0) { ok(c, rc, "nest_prolong behind failed creations"); break; }
            g_calls++; g_failed++;
            if (rc == 0) die("nest_prolong succeeded with a failed creation");
            if (!picles_last_error(c)[0]) die("nest_prolong failed without a text");
            if (fake_hip_live() != live) die("nest_prolong left something behind when creation " + std::to_string(k) + " failed");
            if (picles_clock(c) != clock) die("a failed nest_prolong moved the child's clock");
            step_both(p, c);
        }
        if (round == 0 && k - 1 < 1) die("nest_prolong made no creation");
        started(p, c, "behind failed creations");
        step_both(p, c);
    }
    ok(nullptr, picles_destroy(c), "destroy (child)"); g_destroyed++;
    ok(nullptr, picles_destroy(p), "destroy (parent)"); g_destroyed++;
}
}   // namespace

int main()
{
    if (picles_abi_version() != PICLES_ABI_VERSION || PICLES_ABI_VERSION < 15) { fprintf(stderr, "ABI version\n"); return 2; }
    const long live = fake_hip_live();
    success_and_again();
    refusals();
    failed_creations();
    if (fake_hip_live() != live) die("blocks or events alive at the end");
    if (g_started < 6) die("too few children started");
    printf("prolong harness: %ld ABI calls, %ld refused as documented, %ld children started, %ld calls failed by a creation, %ld contexts destroyed, "
           "no sanitizer report\n", g_calls, g_refused, g_started, g_failed, g_destroyed);
    return 0;
}
