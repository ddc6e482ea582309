// nest_harness.cpp — the host side of the boundary forcing and of both directions of a nest (picles_bforce_*, picles_nest_*,
// picles_nest_feedback_*) under AddressSanitizer, on top of fake_hip.cpp like stat_harness.cpp.  One fixed program, no random
// numbers: a 12x9 parent and a 10x7 child, whole grids, an open rim on both.
//   * every entry point, every caller buffer on the heap at exactly the size the contract names;
//   * every refusal those entry points have that a single fake device can reach, the texts of the geometry checks compared to the
//     byte, and behind each refusal a cycle() — both contexts step, sample, feed back and hand their levels out;
//   * the lifetimes in every order the code distinguishes (free and destroy from either end, one-way and two-way, a new nest and a
//     new feedback behind each), and the calls that must fail with a text once the parent is gone;
//   * enough cycles for every level slot of both directions to be written more than twice, with a step pending and with none;
//   * (not with "trace") for picles_bforce_init_band, picles_nest_init and picles_nest_feedback_init every creation the call makes
//     failed in turn: the call fails, nothing is left behind (fake_hip_live), both contexts go on, and the same call then succeeds.
// "nest_harness trace" runs all but the last part: with PICLES_FAKE_HIP_TRACE set, that run's trace is what
// tests/golden/nest_host_trace_parent.txt holds, taken from the host code before the two directions were put on one link —
// trace_diff.py says whether a later build still enqueues, waits, records and synchronises alike.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_nest.py).
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

extern "C" long fake_hip_fail_alloc(long k);      /* fake_hip.cpp */
extern "C" long fake_hip_live(void);

namespace {
long g_calls = 0, g_refused = 0, g_samples = 0, g_feedbacks = 0, g_pending[2] = {0, 0}, g_failed_inits = 0, g_cycles = 0;
const double DT = 600.0;

void die(const std::string &what) { fprintf(stderr, "nest harness: %s\n", what.c_str()); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "nest harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
/* text: a piece the error text must hold; exact: the text must be it to the byte */
void refused(picles_ctx *c, int rc, const char *what, int code, const std::string &text = "", bool exact = false)
{
    g_calls++; g_refused++;
    if (rc == 0) die(std::string(what) + " was not refused");
    if (rc != code) die(std::string(what) + " refused with " + std::to_string(rc) + ", not " + std::to_string(code));
    const std::string got = picles_last_error(c);
    if (got.empty()) die(std::string(what) + " refused without a text");
    if (exact ? got != text : got.find(text) == std::string::npos) die(std::string(what) + ": the text is \"" + got + "\", expected \"" + text + "\"");
}

picles_ctx *make_context(int Nx, int Ny, int periodic_boundary, int j_begin = 0, int j_end = -1, const int8_t *mask = nullptr, int periodic = 0)
{
    picles_grid g; picles_phys p; picles_ode o; picles_model m;
    memset(&g, 0, sizeof g); memset(&p, 0, sizeof p); memset(&o, 0, sizeof o); memset(&m, 0, sizeof m);
    g.Nx = Nx; g.Ny = Ny; g.dx = 2000.0; g.dy = 1500.0; g.periodic_x = periodic ? 1 : 0; g.periodic_y = periodic; g.mask = mask;
    g.j_begin = j_begin; g.j_end = j_end < 0 ? Ny : j_end;
    p.r_g = 0.85; p.C_alpha = -1.41; p.C_phi = 0.04; p.C_e = 2.2117647058823533e-4; p.g = 9.81; p.gamma = 0.88; p.q = -0.25;
    p.c_beta = 0.04; p.c_D = 2e-3; p.c_e = 1.3e-6; p.c_alpha = 11.8;
    p.propagation = p.input = p.dissipation = p.peak_shift = p.direction = 1;
    o.abstol = 1e-4; o.reltol = 1e-3; o.dt0 = 1e-3; o.dtmin = 1e-4; o.force_dtmin = 1; o.solver = 0; o.maxiters = 10000;
    o.log_energy_minimum = -13.0; o.log_energy_maximum = 3.3; o.wind_min_squared = 4.0; o.timestep = 600.0;
    m.periodic_boundary = periodic_boundary; m.minimal_state[0] = 1.25e-6; m.minimal_state[1] = 1.28e-9;
    picles_ctx *c = nullptr;
    g_calls++;
    if (picles_create(&g, &p, &o, &m, 0, 1, &c) != 0) die(std::string("picles_create: ") + picles_last_error(nullptr));
    const size_t N = (size_t)Nx * (g.j_end - g.j_begin);
    std::vector<double> u(N, 9.0), v(N, 4.0);
    ok(c, picles_set_winds(c, u.data(), v.data(), 0.0, nullptr, nullptr, 0.0), "set_winds");
    ok(c, picles_seed(c, 0.0), "seed");
    return c;
}

/* ---- the geometry: exact-size heap blocks ---- */
struct Geometry {
    int n = 0;                                /* the child's set: its open rim */
    std::vector<int32_t> rim;
    int n_corner = 20;                        /* the nest: 20 parent nodes, four corners a child node */
    std::vector<int32_t> corner_ij, index;
    std::vector<double> weight;
    int n_fb = 6, n_src = 12, m = 3;          /* the feedback: 6 parent ocean nodes from 12 child nodes, three entries each */
    std::vector<int32_t> fb_ij, src_ij, fb_index;
    std::vector<double> fb_weight;
};
std::vector<int32_t> rim_of(int Nx, int Ny)
{
    std::vector<int32_t> i, j;
    for (int y = 0; y < Ny; y++)
        for (int x = 0; x < Nx; x++)
            if (x == 0 || y == 0 || x == Nx - 1 || y == Ny - 1) { i.push_back(x); j.push_back(y); }
    std::vector<int32_t> ij(i);
    ij.insert(ij.end(), j.begin(), j.end());
    return std::vector<int32_t>(ij.begin(), ij.end());      /* (a copy: capacity == size) */
}
Geometry geometry(int cNx, int cNy)
{
    Geometry G;
    G.rim = rim_of(cNx, cNy);
    G.n = (int)G.rim.size() / 2;
    G.corner_ij.resize((size_t)2 * G.n_corner);
    for (int k = 0; k < G.n_corner; k++) { G.corner_ij[k] = 1 + k % 10; G.corner_ij[G.n_corner + k] = 1 + k / 10; }
    G.index.resize((size_t)4 * G.n);
    G.weight.resize((size_t)4 * G.n);
    for (int c = 0; c < 4; c++)
        for (int k = 0; k < G.n; k++) {
            G.index[(size_t)c * G.n + k] = (k + 3 * c) % G.n_corner;
            G.weight[(size_t)c * G.n + k] = (k % 7 == 3 && c == 1) ? 0.0 : (k % 11 == 5 && c == 2) ? -0.125 : 0.25;
        }
    G.fb_ij.resize((size_t)2 * G.n_fb);
    for (int k = 0; k < G.n_fb; k++) { G.fb_ij[k] = 4 + k % 3; G.fb_ij[G.n_fb + k] = 3 + k / 3; }
    G.src_ij.resize((size_t)2 * G.n_src);
    for (int k = 0; k < G.n_src; k++) { G.src_ij[k] = 1 + k % 4; G.src_ij[G.n_src + k] = 1 + k / 4; }
    G.fb_index.resize((size_t)G.m * G.n_fb);
    G.fb_weight.resize((size_t)G.m * G.n_fb);
    for (int c = 0; c < G.m; c++)
        for (int k = 0; k < G.n_fb; k++) {
            G.fb_index[(size_t)c * G.n_fb + k] = (2 * k + c) % G.n_src;
            G.fb_weight[(size_t)c * G.n_fb + k] = (c == 2 && k % 2) ? 0.0 : 0.5;
        }
    return G;
}

/* ---- a parent and a child, and what the harness knows of the links between them ---- */
struct Pair {
    picles_ctx *p = nullptr, *c = nullptr;
    bool attached = false;                    /* the child holds a nest whose parent lives */
    bool feeding = false;                     /* the child holds a feedback whose parent lives */
    Geometry G;
};
const int PNX = 12, PNY = 9, CNX = 10, CNY = 7;

void get_levels(picles_ctx *c)
{
    int32_t n = 0, levels = 0;
    if (picles_bforce_info(c, &n, &levels, nullptr, nullptr) != 0 || levels == 0) return;
    std::vector<double> v0((size_t)3 * n), v1(levels == 2 ? (size_t)3 * n : 0);
    ok(c, picles_bforce_get_levels(c, v0.data(), levels == 2 ? v1.data() : nullptr), "bforce_get_levels");
}
bool can_step(picles_ctx *c)
{
    int32_t levels = 0; double t0 = 0, t1 = 0;
    if (picles_bforce_info(c, nullptr, &levels, &t0, &t1) != 0) return true;      /* no set */
    if (levels == 0) return false;
    return levels == 1 || (picles_clock(c) >= t0 && picles_clock(c) <= t1);
}
/* both contexts still work: the parent steps, the child is sampled and steps, feeds back, and the levels of both come out.
 * flush: complete the pending steps first, so the sample and the feedback read State and not a pending step's records */
void cycle(Pair &P, bool flush = false)
{
    g_cycles++;
    if (P.p && can_step(P.p)) ok(P.p, picles_run_steps(P.p, DT, 1), "run_steps (parent)");
    if (P.p && flush) ok(P.p, picles_sync(P.p), "sync (parent)");
    if (P.c) {
        if (P.attached) { ok(P.c, picles_nest_sample(P.c), "nest_sample"); g_samples++; g_pending[flush ? 0 : 1]++; }
        else {
            int32_t n = 0, levels = 0;
            if (picles_bforce_info(P.c, &n, &levels, nullptr, nullptr) == 0 && levels == 0) {      /* a set of its own, empty: one constant level */
                std::vector<double> v((size_t)3 * n, 0.5);
                ok(P.c, picles_bforce_set_levels(P.c, 0.0, v.data(), 0.0, nullptr), "bforce_set_levels (one level)");
            }
        }
        if (can_step(P.c)) ok(P.c, picles_run_steps(P.c, DT, 1), "run_steps (child)");
        if (flush) ok(P.c, picles_sync(P.c), "sync (child)");
        if (P.feeding) { ok(P.c, picles_nest_feedback(P.c), "nest_feedback"); g_feedbacks++; }
        get_levels(P.c);
    }
    if (P.p) get_levels(P.p);
}

void bforce_rim(Pair &P) { ok(P.c, picles_bforce_init(P.c, P.G.n, P.G.rim.data()), "bforce_init"); }
void nest(Pair &P)
{
    ok(P.c, picles_nest_init(P.c, P.p, P.G.n_corner, P.G.corner_ij.data(), P.G.index.data(), P.G.weight.data()), "nest_init");
    P.attached = true;
    int32_t nc = 0; int64_t s = -1;
    ok(P.c, picles_nest_info(P.c, &nc, &s), "nest_info");
    if (nc != P.G.n_corner || s != 0) die("nest_info after init");
}
int feedback_init(Pair &P) { return picles_nest_feedback_init(P.c, P.G.n_fb, P.G.fb_ij.data(), P.G.n_src, P.G.src_ij.data(), P.G.m, P.G.fb_index.data(), P.G.fb_weight.data()); }
/* the clocks agree behind every cycle: the first feedback right away, so the parent has its level and steps */
void feed(Pair &P)
{
    ok(P.c, feedback_init(P), "nest_feedback_init");
    P.feeding = true;
    int32_t a = 0, b = 0, m = 0; int64_t t = -1;
    ok(P.c, picles_nest_feedback_info(P.c, &a, &b, &m, &t), "nest_feedback_info");
    if (a != P.G.n_fb || b != P.G.n_src || m != P.G.m || t != 0) die("nest_feedback_info after init");
    ok(P.c, picles_nest_feedback(P.c), "nest_feedback (first)");
    g_feedbacks++;
}
Pair make_pair(bool with_set = true, bool with_nest = true, bool with_feedback = false)
{
    Pair P;
    P.p = make_context(PNX, PNY, 0);
    P.c = make_context(CNX, CNY, 0);
    P.G = geometry(CNX, CNY);
    if (with_set) bforce_rim(P);
    if (with_set && with_nest) { nest(P); cycle(P); }
    if (with_set && with_nest && with_feedback) feed(P);
    return P;
}
/* a new parent for a child whose parent went: at the child's clock */
void new_parent(Pair &P)
{
    P.p = make_context(PNX, PNY, 0);
    const int n = (int)std::llround(picles_clock(P.c) / DT);
    if (n) ok(P.p, picles_run_steps(P.p, DT, n), "run_steps (the new parent catches up)");
}
void destroy_parent(Pair &P) { ok(nullptr, picles_destroy(P.p), "destroy (parent)"); P.p = nullptr; P.attached = P.feeding = false; }
void destroy_child(Pair &P) { ok(nullptr, picles_destroy(P.c), "destroy (child)"); P.c = nullptr; P.attached = P.feeding = false; }
void destroy(Pair &P) { if (P.c) destroy_child(P); if (P.p) destroy_parent(P); }

/* ---- the refusals ---- */
void refusals_of_the_set()
{
    Pair P = make_pair(false);
    picles_ctx *c = P.c;
    const Geometry &G = P.G;
    const int n = G.n;
    std::vector<double> lv((size_t)3 * n, 0.25);
    /* without a set */
    refused(c, picles_bforce_set_levels(c, 0.0, lv.data(), 0.0, nullptr), "set_levels without a set", -2, "picles_bforce_init first", true);
    refused(c, picles_bforce_get_levels(c, lv.data(), nullptr), "get_levels without a set", -2, "picles_bforce_init first", true);
    if (picles_bforce_info(c, nullptr, nullptr, nullptr, nullptr) != -1) die("bforce_info without a set");
    ok(c, picles_bforce_free(c), "bforce_free without a set");
    if (picles_bforce_init(nullptr, n, G.rim.data()) != -1 || picles_bforce_init_band(nullptr, n, G.rim.data(), nullptr) != -1) die("a NULL context");
    cycle(P);
    /* init, both flavours */
    refused(c, picles_bforce_init(c, 0, G.rim.data()), "n = 0", -2, "picles_bforce_init: n must be >= 1 and the node list given", true);
    refused(c, picles_bforce_init_band(c, n, nullptr, nullptr), "no node list", -2, "picles_bforce_init_band: n must be >= 1 and the node list given", true);
    {
        std::vector<int32_t> ij(G.rim);
        ij[3] = CNX;
        refused(c, picles_bforce_init(c, n, ij.data()), "a node off the grid", -2, "picles_bforce_init: node 3 = (10, 0) lies outside [0, Nx) x [0, Ny)", true);
        ij = G.rim; ij[5] = 4; ij[n + 5] = 3;
        refused(c, picles_bforce_init(c, n, ij.data()), "an ocean node in a rim set", -2, "is no grid-boundary node (mask class 1, 3 is needed)");
        ij = G.rim; ij[7] = ij[6]; ij[n + 7] = ij[n + 6];
        refused(c, picles_bforce_init_band(c, n, ij.data(), nullptr), "a node given twice", -2, "picles_bforce_init_band: node 7 = (6, 0) is given twice", true);
        cycle(P);
        const double bad[4] = {__builtin_nan(""), 0.0, 1.5, -0.5};
        for (double b : bad) {
            std::vector<double> w((size_t)n, 0.5);
            w[(size_t)n - 1] = b;
            refused(c, picles_bforce_init_band(c, n, G.rim.data(), w.data()), "a weight outside (0, 1]", -2, ": a weight must be finite and in (0, 1]");
        }
    }
    {   /* land in a band; a periodic model; a slab */
        std::vector<int8_t> mask((size_t)CNX * CNY, 1);
        for (int y = 0; y < CNY; y++) for (int x = 0; x < CNX; x++) if (x == 0 || y == 0 || x == CNX - 1 || y == CNY - 1) mask[(size_t)y * CNX + x] = 3;
        mask[(size_t)3 * CNX + 4] = 0;
        picles_ctx *l = make_context(CNX, CNY, 0, 0, -1, mask.data());
        std::vector<int32_t> ij(G.rim);
        ij[5] = 4; ij[n + 5] = 3;
        refused(l, picles_bforce_init_band(l, n, ij.data(), nullptr), "land in a band", -2, "is neither a grid-boundary node nor an ocean node (mask class 0, 3 or 1 is needed)");
        ok(l, picles_run_steps(l, DT, 1), "run_steps behind a refusal");
        ok(l, picles_destroy(l), "destroy");
        picles_ctx *q = make_context(CNX, CNY, 1, 0, -1, nullptr, 1);
        refused(q, picles_bforce_init(q, n, G.rim.data()), "a periodic model", -5, "there is no open rim to force");
        ok(q, picles_destroy(q), "destroy");
        picles_ctx *s = make_context(CNX, CNY, 0, 2, 6);
        refused(s, picles_bforce_init(s, n, G.rim.data()), "a slab", -5, "slabs and the native ring do not carry a boundary forcing");
        refused(s, picles_nest_init(s, P.p, G.n_corner, G.corner_ij.data(), G.index.data(), G.weight.data()), "a slab as a child", -5,
                "picles_nest_init: slabs, slab mode and the native ring do not nest: both contexts must be whole-grid contexts", true);
        ok(s, picles_destroy(s), "destroy");
    }
    /* a band set with a blend plane, all of its entry points */
    {
        std::vector<double> w((size_t)n, 1.0);
        w[2] = 0.5;
        ok(c, picles_bforce_init_band(c, n, G.rim.data(), w.data()), "bforce_init_band");
    }
    refused(c, picles_bforce_init(c, n, G.rim.data()), "a second set", -2, "picles_bforce_init: a boundary forcing set exists (picles_bforce_free first)", true);
    refused(c, picles_run_steps(c, DT, 1), "a step without levels", -2, "the boundary forcing set has no levels yet");
    refused(c, picles_bforce_get_levels(c, lv.data(), nullptr), "get_levels of a level not held", -2, "the set holds 0 level(s)");
    refused(c, picles_bforce_set_levels(c, 0.0, nullptr, 0.0, nullptr), "no level 0", -2, "picles_bforce_set_levels: level 0 must be given", true);
    refused(c, picles_bforce_set_levels(c, 1.0, lv.data(), 1.0, lv.data()), "t1 == t0", -2, "picles_bforce_set_levels: two levels need t1 > t0", true);
    refused(c, picles_bforce_set_levels(c, -__builtin_inf(), lv.data(), 1.0, lv.data()), "t0 = -inf", -2, "picles_bforce_set_levels: the level times must be finite", true);
    cycle(P);                                 /* (uploads one level) */
    refused(c, picles_bforce_get_levels(c, lv.data(), lv.data()), "get_levels of level 1 of one", -2, "the set holds 1 level(s)");
    {
        std::vector<double> v1((size_t)3 * n, 0.75);
        const double t = picles_clock(c);
        ok(c, picles_bforce_set_levels(c, t, lv.data(), t + 2 * DT, v1.data()), "bforce_set_levels (two levels)");
        int32_t nn = 0, levels = 0; double t0 = -1, t1 = -1;
        ok(c, picles_bforce_info(c, &nn, &levels, &t0, &t1), "bforce_info");
        if (nn != n || levels != 2 || t0 != t || t1 != t + 2 * DT) die("bforce_info");
        std::vector<double> b0((size_t)3 * n), b1((size_t)3 * n);
        ok(c, picles_bforce_get_levels(c, b0.data(), b1.data()), "bforce_get_levels (two levels)");
        if (memcmp(b0.data(), lv.data(), b0.size() * 8) || memcmp(b1.data(), v1.data(), b1.size() * 8)) die("get_levels does not return what set_levels uploaded");
        ok(c, picles_bforce_get_levels(c, nullptr, b1.data()), "bforce_get_levels (level 1 alone)");
        cycle(P); cycle(P); cycle(P);         /* the window's last start time */
        refused(c, picles_run_steps(c, DT, 1), "a step outside the window", -2, "outside the window");
        refused(c, picles_time_step(c, DT, 0), "a step outside the window", -2, "outside the window");
        ok(c, picles_bforce_set_levels(c, 0.0, lv.data(), 0.0, nullptr), "bforce_set_levels (one level again)");
    }
    cycle(P);
    ok(c, picles_bforce_free(c), "bforce_free (a band)");
    cycle(P);
    destroy(P);
}

void refusals_of_the_nest()
{
    Pair P = make_pair(false);
    picles_ctx *c = P.c, *p = P.p;
    const Geometry &G = P.G;
    const int n = G.n;
    auto init = [&](const std::vector<int32_t> &cij, const std::vector<int32_t> &ix, const std::vector<double> &w, int nc) {
        return picles_nest_init(c, p, nc, cij.data(), ix.data(), w.data());
    };
    /* without a nest */
    refused(c, picles_nest_sample(c), "sample without a nest", -2, "picles_nest_sample: picles_nest_init first", true);
    if (picles_nest_info(c, nullptr, nullptr) != -1 || picles_nest_feedback_info(c, nullptr, nullptr, nullptr, nullptr) != -1) die("info without a nest");
    ok(c, picles_nest_free(c), "nest_free without a nest");
    ok(c, picles_nest_feedback_free(c), "nest_feedback_free without a feedback");
    refused(c, picles_nest_feedback(c), "feedback without one", -2, "picles_nest_feedback: picles_nest_feedback_init first", true);
    refused(c, feedback_init(P), "feedback_init without a nest", -2, "picles_nest_feedback_init: the child holds no nest");
    if (picles_nest_init(nullptr, p, G.n_corner, G.corner_ij.data(), G.index.data(), G.weight.data()) != -1 || picles_nest_sample(nullptr) != -1 ||
        picles_nest_free(nullptr) != -1 || picles_nest_feedback(nullptr) != -1 || picles_nest_feedback_free(nullptr) != -1) die("a NULL context");
    refused(c, init(G.corner_ij, G.index, G.weight, G.n_corner), "a child without a set", -2, "picles_nest_init: the child has no boundary forcing set");
    cycle(P);
    bforce_rim(P);
    refused(c, picles_nest_init(c, nullptr, G.n_corner, G.corner_ij.data(), G.index.data(), G.weight.data()), "no parent", -2, "picles_nest_init: no parent context given", true);
    refused(c, picles_nest_init(c, c, G.n_corner, G.corner_ij.data(), G.index.data(), G.weight.data()), "child == parent", -2, "child and parent are the same context");
    refused(c, init(G.corner_ij, G.index, G.weight, 0), "n_corner = 0", -2, "picles_nest_init: n_corner must be >= 1 and corner_ij, index and weight given", true);
    refused(c, picles_nest_init(c, p, G.n_corner, G.corner_ij.data(), nullptr, G.weight.data()), "no index", -2,
            "picles_nest_init: n_corner must be >= 1 and corner_ij, index and weight given", true);
    {
        std::vector<int32_t> cij(G.corner_ij), ix(G.index);
        std::vector<double> w(G.weight);
        cij[G.n_corner + 4] = PNY;
        refused(c, init(cij, G.index, G.weight, G.n_corner), "a corner off the parent's grid", -2,
                "picles_nest_init: corner 4 = (5, 9) lies outside the parent's grid [0, 12) x [0, 9)", true);
        cij = G.corner_ij; cij[0] = -1;
        refused(c, init(cij, G.index, G.weight, G.n_corner), "a corner off the parent's grid", -2,
                "picles_nest_init: corner 0 = (-1, 1) lies outside the parent's grid [0, 12) x [0, 9)", true);
        ix[(size_t)2 * n + 7] = G.n_corner;
        refused(c, init(G.corner_ij, ix, G.weight, G.n_corner), "an index off the list", -2,
                "picles_nest_init: index 20 of node 7, corner 2, lies outside [0, n_corner = 20)", true);
        ix = G.index; ix[(size_t)4 * n - 1] = -3;
        refused(c, init(G.corner_ij, ix, G.weight, G.n_corner), "an index off the list", -2,
                "picles_nest_init: index -3 of node " + std::to_string(n - 1) + ", corner 3, lies outside [0, n_corner = 20)", true);
        w[(size_t)n + 2] = __builtin_inf();
        refused(c, init(G.corner_ij, G.index, w, G.n_corner), "a weight that is not finite", -2, "picles_nest_init: the weight of node 2, corner 1, is not finite", true);
    }
    if (picles_nest_info(c, nullptr, nullptr) != -1) die("a refused nest_init left a nest behind");
    cycle(P);
    nest(P);
    refused(c, init(G.corner_ij, G.index, G.weight, G.n_corner), "a second nest", -2, "picles_nest_init: this context holds a nest (picles_nest_free first)", true);
    std::vector<double> lv((size_t)3 * n, 0.25);
    refused(c, picles_bforce_set_levels(c, 0.0, lv.data(), 0.0, nullptr), "set_levels under a nest", -2, "this set's levels come from a parent context (a nest)");
    refused(c, picles_run_steps(c, DT, 1), "a step before the first sample", -2, "the boundary forcing set has no levels yet");
    ok(c, picles_nest_sample(c), "nest_sample (first)"); g_samples++;
    refused(c, picles_nest_sample(c), "a sample without a parent step", -2, "has not moved past the latest level");
    cycle(P); cycle(P);

    /* feedback_init */
    auto fbinit = [&](int n_fb, const std::vector<int32_t> &fij, int n_src, const std::vector<int32_t> &sij, int m, const std::vector<int32_t> &ix, const std::vector<double> &w) {
        return picles_nest_feedback_init(c, n_fb, fij.data(), n_src, sij.data(), m, ix.data(), w.data());
    };
    const std::string F = "picles_nest_feedback_init: ";
    refused(c, fbinit(0, G.fb_ij, G.n_src, G.src_ij, G.m, G.fb_index, G.fb_weight), "n_fb = 0", -2, F + "n_fb must be >= 1 and fb_ij given", true);
    refused(c, fbinit(G.n_fb, G.fb_ij, 0, G.src_ij, G.m, G.fb_index, G.fb_weight), "n_src = 0", -2, F + "n_src and m must be >= 1 and src_ij, index and weight given", true);
    refused(c, fbinit(G.n_fb, G.fb_ij, G.n_src, G.src_ij, 0, G.fb_index, G.fb_weight), "m = 0", -2, F + "n_src and m must be >= 1 and src_ij, index and weight given", true);
    {
        std::vector<int32_t> sij(G.src_ij), ix(G.fb_index), fij(G.fb_ij);
        std::vector<double> w(G.fb_weight);
        sij[3] = CNX + 2;
        refused(c, fbinit(G.n_fb, G.fb_ij, G.n_src, sij, G.m, G.fb_index, G.fb_weight), "a source node off the child's grid", -2,
                F + "source node 3 = (12, 1) lies outside the child's grid [0, 10) x [0, 7)", true);
        ix[(size_t)G.n_fb + 1] = G.n_src;
        refused(c, fbinit(G.n_fb, G.fb_ij, G.n_src, G.src_ij, G.m, ix, G.fb_weight), "an index off the source list", -2,
                F + "index 12 of node 1, entry 1, lies outside [0, n_src = 12)", true);
        w[(size_t)2 * G.n_fb] = -0.5;
        refused(c, fbinit(G.n_fb, G.fb_ij, G.n_src, G.src_ij, G.m, G.fb_index, w), "a negative weight", -2,
                F + "the weight of node 0, entry 2, is not finite or is negative", true);
        w = G.fb_weight; w[4] = __builtin_nan("");
        refused(c, fbinit(G.n_fb, G.fb_ij, G.n_src, G.src_ij, G.m, G.fb_index, w), "a NaN weight", -2,
                F + "the weight of node 4, entry 0, is not finite or is negative", true);
        w = G.fb_weight;
        for (int e = 0; e < G.m; e++) w[(size_t)e * G.n_fb + 5] = 0.0;
        refused(c, fbinit(G.n_fb, G.fb_ij, G.n_src, G.src_ij, G.m, G.fb_index, w), "a node without a source", -2, F + "every weight of node 5 is zero: it has no source", true);
        cycle(P);
        /* what the parent's set refuses: both contexts as they were */
        const long live = fake_hip_live();
        fij[2] = 0;
        refused(c, fbinit(G.n_fb, fij, G.n_src, G.src_ij, G.m, G.fb_index, G.fb_weight), "a rim node of the parent", -2,
                "picles_nest_feedback_init: the parent's set: node 2 = (0, 3) is no ocean node of the parent (mask class 3, 1 is needed)");
        fij = G.fb_ij; fij[1] = fij[0]; fij[G.n_fb + 1] = fij[G.n_fb];
        refused(c, fbinit(G.n_fb, fij, G.n_src, G.src_ij, G.m, G.fb_index, G.fb_weight), "a feedback node given twice", -2, "picles_nest_feedback_init: the parent's set: node 1 = (4, 3) is given twice", true);
        if (fake_hip_live() != live) die("a refused feedback_init left blocks behind");
        if (picles_bforce_info(p, nullptr, nullptr, nullptr, nullptr) != -1 || picles_nest_feedback_info(c, nullptr, nullptr, nullptr, nullptr) != -1) die("a refused feedback_init left a set behind");
        cycle(P);
    }
    {   /* a parent with a set of its own; a parent another child feeds */
        std::vector<int32_t> prim = rim_of(PNX, PNY);
        ok(p, picles_bforce_init(p, (int)prim.size() / 2, prim.data()), "bforce_init (parent)");
        refused(c, feedback_init(P), "a parent with its own set", -5, "the parent holds a boundary forcing set of its own");
        ok(p, picles_bforce_free(p), "bforce_free (parent)");
        Pair Q;
        Q.p = p; Q.G = geometry(CNX, CNY);
        Q.c = make_context(CNX, CNY, 0);
        const int k = (int)std::llround(picles_clock(p) / DT);
        bforce_rim(Q);
        {   /* (the second child catches up under a level of its own, then nests) */
            std::vector<double> v((size_t)3 * n, 0.5);
            ok(Q.c, picles_bforce_set_levels(Q.c, 0.0, v.data(), 0.0, nullptr), "bforce_set_levels");
            ok(Q.c, picles_run_steps(Q.c, DT, k), "run_steps (second child)");
        }
        nest(Q);
        ok(Q.c, picles_nest_sample(Q.c), "nest_sample (second child)");
        feed(Q);
        refused(c, feedback_init(P), "a parent fed by another child", -5, "picles_nest_feedback_init: the parent is fed by another child: one child per parent feeds back", true);
        std::vector<double> pl((size_t)3 * G.n_fb, 0.25);
        refused(p, picles_bforce_set_levels(p, 0.0, pl.data(), 0.0, nullptr), "set_levels on a fed parent", -2, "this set's level comes from a child context (nest feedback)");
        refused(Q.c, feedback_init(Q), "a second feedback", -2, "picles_nest_feedback_init: this context feeds back already (picles_nest_feedback_free first)", true);
        /* one parent, two children, one of them feeding: all three go on */
        ok(p, picles_run_steps(p, DT, 1), "run_steps (parent of two)");
        ok(c, picles_nest_sample(c), "nest_sample"); ok(Q.c, picles_nest_sample(Q.c), "nest_sample"); g_samples += 2;
        ok(c, picles_run_steps(c, DT, 1), "run_steps"); ok(Q.c, picles_run_steps(Q.c, DT, 1), "run_steps");
        ok(Q.c, picles_nest_feedback(Q.c), "nest_feedback"); g_feedbacks++;
        /* the clocks */
        ok(Q.c, picles_run_steps(Q.c, DT, 1), "run_steps (the child runs ahead)");
        refused(Q.c, picles_nest_feedback(Q.c), "clocks that differ", -2, "differ: a feedback is taken where both models stand at the same time");
        ok(Q.c, picles_destroy(Q.c), "destroy (the feeding child, first)");
        if (picles_bforce_info(p, nullptr, nullptr, nullptr, nullptr) != -1) die("the feeding child went and the parent kept its set");
        cycle(P);
    }
    {   /* caller-provided streams: a context that used one is out, at init and behind it */
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, 0) != hipSuccess) die("stream");
        picles_ctx *x = make_context(CNX, CNY, 0);
        ok(x, picles_stat_init(x, PICLES_STAT_MEAN, 0, nullptr, 1, 1), "stat_init");
        ok(x, picles_stat_update(x, s), "stat_update on a caller's stream");
        ok(x, picles_bforce_init(x, n, G.rim.data()), "bforce_init");
        refused(x, picles_nest_init(x, p, G.n_corner, G.corner_ij.data(), G.index.data(), G.weight.data()), "a child that ran on a caller's stream", -5,
                "picles_nest_init: a context that has run on caller-provided streams cannot be ordered by the nest's events");
        ok(x, picles_destroy(x), "destroy");
        feed(P);
        cycle(P);
        ok(p, picles_stat_init(p, PICLES_STAT_MEAN, 0, nullptr, 1, 1), "stat_init (parent)");
        ok(p, picles_stat_update(p, s), "stat_update on a caller's stream (parent)");
        refused(c, picles_nest_sample(c), "a sample with a caller's stream in play", -5, "picles_nest_sample: a context that has run on caller-provided streams");
        refused(c, picles_nest_feedback(c), "a feedback with a caller's stream in play", -5, "picles_nest_feedback: a context that has run on caller-provided streams");
        ok(c, picles_nest_feedback_free(c), "nest_feedback_free"); P.feeding = false;
        refused(c, feedback_init(P), "feedback_init with a caller's stream in play", -5, "picles_nest_feedback_init: a context that has run on caller-provided streams");
        ok(c, picles_nest_free(c), "nest_free"); P.attached = false;
        refused(c, init(G.corner_ij, G.index, G.weight, G.n_corner), "a parent that ran on a caller's stream", -5, "picles_nest_init: a context that has run on caller-provided streams");
        get_levels(c);
        ok(p, picles_run_steps(p, DT, 1), "run_steps (parent)");
        destroy(P);
        if (hipStreamDestroy(s) != hipSuccess) die("stream");
    }
}

/* ---- the lifetimes ---- */
void gone_parent_texts(Pair &P, bool two_way)
{
    refused(P.c, picles_nest_sample(P.c), "a sample after the parent went", -2, "picles_nest_sample: the parent context was destroyed (the set keeps its last levels)");
    if (two_way) {
        refused(P.c, picles_nest_feedback(P.c), "a feedback after the parent went", -2,
                "picles_nest_feedback: the parent context was destroyed (its set went with it): picles_nest_feedback_free", true);
        ok(P.c, picles_nest_feedback_free(P.c), "nest_feedback_free (detached)");
    }
    refused(P.c, feedback_init(P), "feedback_init after the parent went", -2, "picles_nest_feedback_init: the parent context was destroyed", true);
    get_levels(P.c);                          /* the child keeps its last levels */
    cycle(P);
}
void lifetimes()
{
    {   /* nest_free before bforce_free; a new nest on the same set */
        Pair P = make_pair();
        cycle(P); cycle(P);
        ok(P.c, picles_nest_free(P.c), "nest_free"); P.attached = false;
        get_levels(P.c);                      /* the pair moved home */
        std::vector<double> v((size_t)3 * P.G.n, 0.5);
        ok(P.c, picles_bforce_set_levels(P.c, 0.0, v.data(), 0.0, nullptr), "bforce_set_levels behind nest_free");
        cycle(P);
        nest(P); cycle(P); cycle(P, true);
        ok(P.c, picles_nest_free(P.c), "nest_free");  P.attached = false;
        ok(P.c, picles_bforce_free(P.c), "bforce_free behind nest_free");
        cycle(P);
        bforce_rim(P); nest(P); cycle(P); cycle(P);
        /* bforce_free with the nest alive: the nest goes with the set */
        ok(P.c, picles_bforce_free(P.c), "bforce_free with a nest"); P.attached = false;
        if (picles_nest_info(P.c, nullptr, nullptr) != -1) die("the set went and the nest stayed");
        cycle(P);
        bforce_rim(P); nest(P); cycle(P);
        destroy(P);                           /* the child first, nested */
    }
    {   /* bforce_free on a fed parent: the feedback goes, the nest stays */
        Pair P = make_pair(true, true, true);
        cycle(P); cycle(P);
        ok(P.p, picles_bforce_free(P.p), "bforce_free on a fed parent"); P.feeding = false;
        if (picles_nest_feedback_info(P.c, nullptr, nullptr, nullptr, nullptr) != -1) die("the parent's set went and the feedback stayed");
        cycle(P);
        feed(P); cycle(P); cycle(P, true);
        /* nest_feedback_free, then nest_free */
        ok(P.c, picles_nest_feedback_free(P.c), "nest_feedback_free"); P.feeding = false;
        if (picles_bforce_info(P.p, nullptr, nullptr, nullptr, nullptr) != -1) die("the feedback went and the parent's set stayed");
        cycle(P);
        ok(P.c, picles_nest_free(P.c), "nest_free behind nest_feedback_free"); P.attached = false;
        cycle(P);
        /* nest_free with a live feedback */
        nest(P); cycle(P); feed(P); cycle(P);
        ok(P.c, picles_nest_free(P.c), "nest_free with a feedback"); P.attached = P.feeding = false;
        if (picles_nest_feedback_info(P.c, nullptr, nullptr, nullptr, nullptr) != -1 || picles_bforce_info(P.p, nullptr, nullptr, nullptr, nullptr) != -1)
            die("the nest went and the feedback stayed");
        cycle(P);
        /* bforce_free on the child with both alive */
        nest(P); cycle(P); feed(P); cycle(P);
        ok(P.c, picles_bforce_free(P.c), "bforce_free on a feeding child"); P.attached = P.feeding = false;
        cycle(P);
        bforce_rim(P); nest(P); cycle(P); feed(P); cycle(P);
        destroy_child(P);                     /* the child first, feeding */
        if (picles_bforce_info(P.p, nullptr, nullptr, nullptr, nullptr) != -1) die("the feeding child went and the parent kept its set");
        cycle(P);
        P.c = make_context(CNX, CNY, 0);      /* a new child for the old parent, at its clock */
        bforce_rim(P);
        {
            std::vector<double> v((size_t)3 * P.G.n, 0.5);
            ok(P.c, picles_bforce_set_levels(P.c, 0.0, v.data(), 0.0, nullptr), "bforce_set_levels");
            ok(P.c, picles_run_steps(P.c, DT, (int)std::llround(picles_clock(P.p) / DT)), "run_steps (the new child catches up)");
        }
        nest(P); cycle(P); feed(P); cycle(P);
        destroy_parent(P); destroy(P);        /* the parent first, then the child with its detached links */
    }
    {   /* the parent first, one-way */
        Pair P = make_pair();
        cycle(P); cycle(P);
        destroy_parent(P);
        gone_parent_texts(P, false);
        ok(P.c, picles_nest_free(P.c), "nest_free (detached)");
        new_parent(P);
        nest(P); cycle(P); cycle(P);
        destroy_parent(P);
        ok(P.c, picles_bforce_free(P.c), "bforce_free with a detached nest");
        cycle(P);
        destroy(P);
    }
    {   /* the parent first, two-way */
        Pair P = make_pair(true, true, true);
        cycle(P); cycle(P);
        destroy_parent(P);
        gone_parent_texts(P, true);
        ok(P.c, picles_nest_free(P.c), "nest_free (detached)");
        new_parent(P);
        nest(P); cycle(P); feed(P); cycle(P); cycle(P);
        destroy_parent(P);
        ok(P.c, picles_nest_free(P.c), "nest_free with a detached feedback");
        new_parent(P);
        nest(P); cycle(P); feed(P); cycle(P);
        destroy(P);
    }
}

/* ---- the slots: three of the nest, two of the feedback, each written more than twice ---- */
void rotation()
{
    Pair P = make_pair(true, true, true);
    for (int k = 0; k < 8; k++) cycle(P, k % 3 == 1);
    int64_t s = 0, t = 0;
    ok(P.c, picles_nest_info(P.c, nullptr, &s), "nest_info");
    ok(P.c, picles_nest_feedback_info(P.c, nullptr, nullptr, nullptr, &t), "nest_feedback_info");
    if (s < 7 || t < 5) die("too few samples or feedbacks for every slot to be written twice");
    int32_t levels = 0; double t0 = 0, t1 = 0;
    ok(P.c, picles_bforce_info(P.c, nullptr, &levels, &t0, &t1), "bforce_info");
    if (levels != 2 || t1 != picles_clock(P.p) || t0 != t1 - DT) die("the child's window after the rotation");
    ok(P.p, picles_bforce_info(P.p, nullptr, &levels, &t0, &t1), "bforce_info (parent)");
    if (levels != 1 || t0 != picles_clock(P.c) || t1 != t0) die("the parent's level after the rotation");
    /* several steps a call, and the single-step entry point */
    ok(P.p, picles_run_steps(P.p, DT, 2), "run_steps (parent, two)");
    ok(P.c, picles_nest_sample(P.c), "nest_sample"); g_samples++;
    refused(P.c, picles_run_steps(P.c, DT, 4), "four child steps in a window of two", -2, "outside the window");
    ok(P.c, picles_time_step(P.c, DT, PICLES_STEP_ZERO_FIRST), "time_step (child)");
    ok(P.c, picles_time_step(P.c, DT, 0), "time_step (child)");
    ok(P.c, picles_nest_feedback(P.c), "nest_feedback"); g_feedbacks++;
    cycle(P);
    destroy(P);
}

/* ---- every creation a call makes fails in turn ---- */
template <class Call> void sweep(Pair &P, const char *what, Call call, int at_least)
{
    int k = 1;
    for (;; k++) {
        const long live = fake_hip_live();
        fake_hip_fail_alloc(k);
        const int rc = call();
        if (fake_hip_fail_alloc(0) > 0) {      /* the failure never came: the call made k - 1 creations, and has succeeded */
            ok(P.c, rc, what);
            break;
        }
        g_calls++; g_failed_inits++;
        if (rc == 0) die(std::string(what) + " succeeded with a failed creation");
        if (!picles_last_error(P.c)[0]) die(std::string(what) + " failed without a text");
        if (fake_hip_live() != live) die(std::string(what) + " left something behind when creation " + std::to_string(k) + " failed");
        cycle(P);
    }
    if (k - 1 < at_least) die(std::string(what) + " made fewer creations than it must");
}
void failed_creations()
{
    Pair P = make_pair(false);
    std::vector<double> w((size_t)P.G.n, 1.0);
    w[1] = 0.25;
    sweep(P, "bforce_init_band", [&] { return picles_bforce_init_band(P.c, P.G.n, P.G.rim.data(), w.data()); }, 3);
    cycle(P);
    sweep(P, "nest_init", [&] { return picles_nest_init(P.c, P.p, P.G.n_corner, P.G.corner_ij.data(), P.G.index.data(), P.G.weight.data()); }, 9);
    P.attached = true;
    cycle(P);
    sweep(P, "nest_feedback_init", [&] { return feedback_init(P); }, 9);
    P.feeding = true;
    ok(P.c, picles_nest_feedback(P.c), "nest_feedback (first)");
    cycle(P); cycle(P);
    destroy(P);
}
}   // namespace

int main(int argc, char **argv)
{
    const bool trace_only = argc > 1 && !strcmp(argv[1], "trace");
    if (picles_abi_version() != PICLES_ABI_VERSION) { fprintf(stderr, "ABI version\n"); return 2; }
    const long live = fake_hip_live();
    rotation();
    refusals_of_the_set();
    refusals_of_the_nest();
    lifetimes();
    if (!trace_only) failed_creations();
    if (fake_hip_live() != live) die("blocks or events alive at the end");
    if (g_samples < 5 || g_feedbacks < 4 || !g_pending[0] || !g_pending[1]) die("too few samples or feedbacks, or none with (without) a step pending");
    printf("nest harness: %ld ABI calls, %ld refused as documented, %ld cycles, %ld samples (%ld behind a flush), %ld feedbacks, %ld inits failed by a "
           "creation, no sanitizer report\n", g_calls, g_refused, g_cycles, g_samples, g_pending[0], g_feedbacks, g_failed_inits);
    return 0;
}
