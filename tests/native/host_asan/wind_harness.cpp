// wind_harness.cpp — the host side of the wind window (picles_set_winds*, picles_set_wind_grid*, and what picles_seed, the step entry
// points and the checkpoint do to it) under AddressSanitizer, on top of fake_hip.cpp like nest_harness.cpp.  One fixed program, no
// random numbers.  It sees what the kernels would see through the fake's launch hook:
//   * every host level is a plane filled with a constant of its own, and at a k_wind_sample launch the hook writes each sampled time
//     into element 0 of the planes it goes to: the fake's copies really copy, so element 0 of a plane says which level it holds;
//   * at every launch that takes KParams (k_seed, k_advance, k_step*, k_scatter, k_remesh) it appends a "window" line to the trace: the
//     nine wind fields, floats as hex, and for each of u0, u1, um, uP that the form makes live the tag in element 0 ("-": null or not
//     live); at a k_wind_poly launch the form it was handed and the tags of the levels it reads.  No pointer values, no ordinals;
//   * at every launch no plane that reaches it is null, and a u plane and its v plane hold the same level.
// The walk: one context through every form and every transition between neighbouring forms — from host levels (static, two levels,
// parabola, knot, polylines of 2 and PICLES_MAX_KNOTS knots, the refusal at one more, static), from a lattice in linear mode with 0, 1, 2
// and too many knots in the step (un-fused, fused, a window that does not follow the pending step's, smooth3, a re-seed, a checkpoint
// taken and loaded) and back — and the same walk on a two-slab pair through the split phases.
// "wind_harness trace" runs the walk alone: with PICLES_FAKE_HIP_TRACE set, that run's trace is what
// tests/golden/wind_host_trace_parent.txt holds, taken from the host code before the window had one owner.  Without "trace" every
// creation inside the lazily made plane pairs is also failed in turn: the call fails, the same call then succeeds, and the steps behind
// it launch with whole pairs.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_wind.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../picles_amd/csrc/kernels.h"      /* KParams, GridP, Arrays */

extern "C" long fake_hip_fail_alloc(long k);      /* fake_hip.cpp */
extern "C" long fake_hip_live(void);
extern "C" void fake_hip_launch_hook(void (*f)(const char *kernel, void **args));
extern "C" void fake_hip_trace_line(const char *text);

namespace {
long g_calls = 0, g_refused = 0, g_launches = 0, g_samples = 0, g_failed = 0, g_fused = 0, g_plain = 0;
const double DT = 600.0, LAT_DT = 900.0;

void die(const std::string &what) { fprintf(stderr, "wind harness: %s\n", what.c_str()); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "wind harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what, int code, const char *text)
{
    g_calls++; g_refused++;
    if (rc != code) die(std::string(what) + " gave " + std::to_string(rc) + ", not " + std::to_string(code));
    if (!strstr(picles_last_error(c), text)) die(std::string(what) + ": the text is \"" + picles_last_error(c) + "\"");
}

/* ---- the launch hook ---- */
/* the argument structs of k_wind_sample and k_wind_poly as picles_hip.hip declares them (they live in no header) */
struct SampleOut { double t[2]; double *u[2], *v[2]; };
struct PolyForm { int nk; double sk[PICLES_MAX_KNOTS]; double ilen[PICLES_MAX_KNOTS + 1]; };

bool has(const char *name, const char *piece) { return strstr(name, piece) != nullptr; }
std::string tag(const double *u, const double *v, const char *what)
{
    if (!u || !v) die(std::string("a null ") + what + " plane reaches a launch");
    if (u[0] != v[0]) die(std::string("the u and v planes of ") + what + " hold different levels");
    char b[40];
    snprintf(b, sizeof b, "%a", u[0]);
    return b;
}
void hook(const char *name, void **args)
{
    g_launches++;
    char line[1024];
    if (has(name, "k_wind_sample")) {
        const int nt = has(name, "ILi2E") ? 2 : 1;
        const SampleOut &O = *(const SampleOut *)args[2];
        for (int k = 0; k < nt; k++) {
            if (!O.u[k] || !O.v[k]) die("k_wind_sample is handed a null plane");
            O.u[k][0] = O.v[k][0] = O.t[k];
            g_samples++;
        }
        return;
    }
    if (has(name, "k_wind_poly")) {
        const PolyForm &F = *(const PolyForm *)args[0];
        const double *u0 = *(const double **)args[1], *v0 = *(const double **)args[2], *u1 = *(const double **)args[3], *v1 = *(const double **)args[4];
        const double *lv = *(const double **)args[5], *xb = *(const double **)args[6];
        const long long n = *(const long long *)args[7];
        if (!lv || !xb) die("k_wind_poly is handed a null buffer");
        int at = snprintf(line, sizeof line, "window k_wind_poly nk=%d u0=%s u1=%s sk", F.nk, tag(u0, v0, "level 0").c_str(), tag(u1, v1, "level 1").c_str());
        for (int k = 0; k < PICLES_MAX_KNOTS; k++) at += snprintf(line + at, sizeof line - at, " %a", F.sk[k]);
        at += snprintf(line + at, sizeof line - at, " ilen");
        for (int k = 0; k <= PICLES_MAX_KNOTS; k++) at += snprintf(line + at, sizeof line - at, " %a", F.ilen[k]);
        at += snprintf(line + at, sizeof line - at, " lv");
        for (int k = 0; k < F.nk; k++) at += snprintf(line + at, sizeof line - at, " %s", tag(lv + (size_t)(2 * k) * n, lv + (size_t)(2 * k + 1) * n, "a knot").c_str());
        fake_hip_trace_line(line);
        return;
    }
    const char *fam = has(name, "k_seed") ? "k_seed" : has(name, "k_advance") ? "k_advance" : has(name, "k_step") ? "k_step" :
                      has(name, "k_scatter") ? "k_scatter" : has(name, "k_remesh") ? "k_remesh" : nullptr;
    if (!fam) return;
    const KParams &P = *(const KParams *)args[0];
    const Arrays &A = *(const Arrays *)args[2];
    const bool tv = !P.wind_static;
    if ((A.um == nullptr) != (A.vm == nullptr)) die("half a middle pair reaches a launch");
    if ((A.uP == nullptr) != (A.vP == nullptr)) die("half a previous-level pair reaches a launch");
    if (tv && P.wind_nk > 1 && !P.wind_xb) die("a polyline window without its coefficient planes reaches a launch");
    const bool prev = tv && !strcmp(fam, "k_step");      /* the fused step's remesh evaluates the previous window at its start */
    snprintf(line, sizeof line, "window %s static=%d tw0=%a inv_dtw=%a sk=%a isk=%a i1sk=%a nk=%d xb=%s xn=%lld u0=%s u1=%s um=%s uP=%s", fam,
             P.wind_static, P.tw0, P.inv_dtw, P.wind_sk, P.wind_isk, P.wind_i1sk, P.wind_nk, P.wind_xb ? "set" : "-", P.wind_xn,
             tag(A.u0, A.v0, "level 0").c_str(), tv ? tag(A.u1, A.v1, "level 1").c_str() : "-",
             tv && A.um ? tag(A.um, A.vm, "the middle level").c_str() : "-", prev ? tag(A.uP, A.vP, "the previous level 0").c_str() : "-");
    fake_hip_trace_line(line);
}

/* ---- a model: the whole grid, or two slabs of it driven through the split phases ---- */
const int NX = 16, NY = 16;
picles_ctx *make_context(int j_begin, int j_end)
{
    picles_grid g; picles_phys p; picles_ode o; picles_model m;
    memset(&g, 0, sizeof g); memset(&p, 0, sizeof p); memset(&o, 0, sizeof o); memset(&m, 0, sizeof m);
    g.Nx = NX; g.Ny = NY; g.dx = 2000.0; g.dy = 1500.0; g.periodic_x = 1; g.periodic_y = 1; g.j_begin = j_begin; g.j_end = j_end;
    p.r_g = 0.85; p.C_alpha = -1.41; p.C_phi = 0.04; p.C_e = 2.2117647058823533e-4; p.g = 9.81; p.gamma = 0.88; p.q = -0.25;
    p.c_beta = 0.04; p.c_D = 2e-3; p.c_e = 1.3e-6; p.c_alpha = 11.8;
    p.propagation = p.input = p.dissipation = p.peak_shift = p.direction = 1;
    o.abstol = 1e-4; o.reltol = 1e-3; o.dt0 = 1e-3; o.dtmin = 1e-4; o.force_dtmin = 1; o.solver = 0; o.maxiters = 10000;
    o.log_energy_minimum = -13.0; o.log_energy_maximum = 3.3; o.wind_min_squared = 4.0; o.timestep = DT;
    m.periodic_boundary = 1; m.minimal_state[0] = 1.25e-6; m.minimal_state[1] = 1.28e-9;
    picles_ctx *c = nullptr;
    g_calls++;
    if (picles_create(&g, &p, &o, &m, 0, 1, &c) != 0) die(std::string("picles_create: ") + picles_last_error(nullptr));
    return c;
}

struct Model {
    std::vector<picles_ctx *> c;              /* one context, or the two slabs */
    hipStream_t sE = nullptr, sM = nullptr;   /* the slabs' caller streams */
    size_t n = 0;                             /* nodes per context */
    bool slabs() const { return c.size() > 1; }
};
Model make_model(bool slabs)
{
    Model M;
    if (slabs) {
        M.c = {make_context(0, NY / 2), make_context(NY / 2, NY)};
        if (hipStreamCreateWithFlags(&M.sE, 0) != hipSuccess || hipStreamCreateWithFlags(&M.sM, 0) != hipSuccess) die("stream");
        M.n = (size_t)NX * NY / 2;
    } else {
        M.c = {make_context(0, NY)};
        M.n = (size_t)NX * NY;
    }
    return M;
}
void destroy(Model &M)
{
    for (picles_ctx *c : M.c) ok(nullptr, picles_destroy(c), "destroy");
    if (M.sE && (hipStreamDestroy(M.sE) != hipSuccess || hipStreamDestroy(M.sM) != hipSuccess)) die("stream");
    M.c.clear();
}

/* host levels: exact-size heap planes, each filled with a constant no other level has */
double g_next_tag = 1000.0;
struct Levels {
    std::vector<std::vector<double>> u, v;
    std::vector<const double *> pu, pv;
    Levels(size_t n, int count)
    {
        for (int k = 0; k < count; k++) { u.emplace_back(n, g_next_tag); v.emplace_back(n, g_next_tag); g_next_tag += 1.0; }
        for (int k = 0; k < count; k++) { pu.push_back(u[k].data()); pv.push_back(v[k].data()); }
    }
};

/* one model step of every context.  The whole grid: picles_time_step.  A slab: the split phases on the caller's streams, fused where
 * picles_begin_fused_step takes the step.  Returns what the step entry point refused with (0: the step was taken) */
int step_one(Model &M, picles_ctx *c, double dt, bool run_style)
{
    const int flags = run_style ? PICLES_STEP_ZERO_FIRST : 0;
    if (!M.slabs()) return picles_time_step(c, dt, flags);
    int rc = run_style ? picles_begin_fused_step(c, dt) : 1;
    if (rc < 0) return rc;
    if (rc == 0) {
        g_fused++;
        ok(c, picles_step_rows(c, PICLES_ROWS_EDGE, M.sE), "step_rows (edge)");
        ok(c, picles_step_rows(c, PICLES_ROWS_INTERIOR, M.sM), "step_rows (interior)");
        ok(c, picles_end_fused_step(c), "end_fused_step");
        return 0;
    }
    if ((rc = picles_begin_step(c, dt, flags))) return rc;
    g_plain++;
    ok(c, picles_advance_rows(c, PICLES_ROWS_EDGE, M.sE), "advance_rows (edge)");
    ok(c, picles_advance_rows(c, PICLES_ROWS_INTERIOR, M.sM), "advance_rows (interior)");
    ok(c, picles_scatter_remesh(c, M.sM), "scatter_remesh");
    return 0;
}
void step(Model &M, double dt, bool run_style, int count = 1)
{
    for (int k = 0; k < count; k++)
        for (picles_ctx *c : M.c) { g_calls++; ok(c, step_one(M, c, dt, run_style), "a model step"); }
}
void step_refused(Model &M, double dt, bool run_style, int code, const char *text)
{
    for (picles_ctx *c : M.c) refused(c, step_one(M, c, dt, run_style), "a model step", code, text);
}
void mid(Model &M, bool expected)
{
    std::vector<double> um(M.n), vm(M.n);
    for (picles_ctx *c : M.c) {
        g_calls++;
        const int rc = picles_get_winds_mid(c, um.data(), vm.data());
        if (rc != (expected ? 0 : 1)) die("get_winds_mid: " + std::to_string(rc));
    }
}

/* the windows the caller uploads, each over the next model step */
void host_static(Model &M)
{
    Levels L(M.n, 1);
    for (picles_ctx *c : M.c) ok(c, picles_set_winds(c, L.pu[0], L.pv[0], picles_clock(c), nullptr, nullptr, 0.0), "set_winds (static)");
    mid(M, false);
}
void host_two(Model &M)
{
    Levels L(M.n, 2);
    for (picles_ctx *c : M.c) { const double t = picles_clock(c); ok(c, picles_set_winds(c, L.pu[0], L.pv[0], t, L.pu[1], L.pv[1], t + DT), "set_winds (two levels)"); }
    mid(M, false);
}
void host_parabola(Model &M)
{
    Levels L(M.n, 3);
    for (picles_ctx *c : M.c) { const double t = picles_clock(c); ok(c, picles_set_winds3(c, L.pu[0], L.pv[0], t, L.pu[1], L.pv[1], L.pu[2], L.pv[2], t + DT), "set_winds3"); }
    mid(M, true);
}
void host_knot(Model &M)
{
    Levels L(M.n, 3);
    for (picles_ctx *c : M.c) {
        const double t = picles_clock(c);
        refused(c, picles_set_winds_knot(c, L.pu[0], L.pv[0], t, L.pu[1], L.pv[1], t + DT, L.pu[2], L.pv[2], t + DT), "a knot at the window's end", -2, "strictly inside");
        ok(c, picles_set_winds_knot(c, L.pu[0], L.pv[0], t, L.pu[1], L.pv[1], t + 0.375 * DT, L.pu[2], L.pv[2], t + DT), "set_winds_knot");
    }
    mid(M, true);
}
int host_polyline_rc(Model &M, picles_ctx *c, int knots, const Levels &L)
{
    (void)M;
    std::vector<double> times((size_t)knots + 2);
    const double t = picles_clock(c);
    for (int k = 0; k < knots + 2; k++) times[k] = t + DT * (double)(k * k) / (double)((knots + 1) * (knots + 1));      /* (uneven segments) */
    return picles_set_winds_polyline(c, knots + 2, L.pu.data(), L.pv.data(), times.data());
}
void host_polyline(Model &M, int knots)
{
    Levels L(M.n, knots + 2);
    for (picles_ctx *c : M.c) ok(c, host_polyline_rc(M, c, knots, L), "set_winds_polyline");
    mid(M, knots >= 1);
}

/* a lattice of 3 x 3 x 40 knots, 900 s apart in time: steps of 600 s hold no knot or one, a step of 2000 s two or three, one of 9000 s
 * more than a window carries */
void lattice(Model &M)
{
    const int nx = 3, ny = 3, nt = 40;
    std::vector<double> u((size_t)nx * ny * nt), v(u.size());
    for (size_t k = 0; k < u.size(); k++) { u[k] = 5.0 + 0.01 * (double)k; v[k] = -3.0 + 0.02 * (double)k; }
    for (picles_ctx *c : M.c) {
        refused(c, picles_set_wind_grid(c, nx, ny, 1, 0.0, 20000.0, 0.0, 15000.0, 0.0, LAT_DT, u.data(), v.data(), 0.0, 0.0), "a lattice of one time knot", -2, ">= 2 knots");
        ok(c, picles_set_wind_grid(c, nx, ny, nt, 0.0, 20000.0, 0.0, 15000.0, 0.0, LAT_DT, u.data(), v.data(), 0.0, 0.0), "set_wind_grid");
    }
    mid(M, false);
}
void lattice_mode(Model &M, int mode)
{
    for (picles_ctx *c : M.c) ok(c, picles_set_wind_grid_mode(c, mode), "set_wind_grid_mode");
}

void checkpoint_round(Model &M)
{
    for (picles_ctx *c : M.c) {
        size_t bytes = 0;
        ok(c, picles_checkpoint_size(c, &bytes), "checkpoint_size");
        std::vector<unsigned char> blob(bytes);
        ok(c, picles_checkpoint_begin(c), "checkpoint_begin");
        ok(c, picles_checkpoint_end(c, blob.data(), blob.size()), "checkpoint_end");
        ok(c, picles_checkpoint_load(c, blob.data(), blob.size()), "checkpoint_load");
    }
}

void walk(bool slabs)
{
    Model M = make_model(slabs);
    /* from host levels */
    host_static(M);
    for (picles_ctx *c : M.c) ok(c, picles_seed(c, 0.0), "seed");
    step(M, DT, false); step(M, DT, true, 3); step(M, DT, false);
    host_two(M);            step(M, DT, false); host_two(M); step(M, DT, true);
    host_parabola(M);       step(M, DT, false); host_parabola(M); step(M, DT, true);
    host_knot(M);           step(M, DT, false); host_knot(M); step(M, DT, true);
    host_polyline(M, 2);    step(M, DT, false); host_polyline(M, 2); step(M, DT, true);
    host_polyline(M, PICLES_MAX_KNOTS); step(M, DT, false);
    host_polyline(M, 3);    step(M, DT, true);                      /* (a shorter polyline in buffers that have room for a longer one) */
    {
        Levels L(M.n, PICLES_MAX_KNOTS + 3);
        for (picles_ctx *c : M.c) refused(c, host_polyline_rc(M, c, PICLES_MAX_KNOTS + 1, L), "a polyline of one knot too many", -2, "at most");
        mid(M, true);                                              /* the window on the device is the one before */
        step(M, DT, false);
    }
    host_static(M);         step(M, DT, true, 3);
    /* and back down, each form from its other neighbour */
    host_polyline(M, 2); step(M, DT, false); host_knot(M); step(M, DT, false); host_parabola(M); step(M, DT, false); host_two(M); step(M, DT, false);
    host_static(M); step(M, DT, true, 2);

    /* from a lattice, linear in time: un-fused steps with no knot, one, two and too many inside */
    lattice(M);
    step(M, DT, false, 3);                                         /* (600 s steps against 900 s knots: no knot, one, none, ...) */
    step(M, 2000.0, false); step(M, DT, false); step(M, 2700.0, false);
    step_refused(M, 9000.0, false, -7, "time knots of the wind lattice");
    /* fused: the first step takes the stand-alone advance, the later ones rotate the planes */
    step(M, DT, true, 6);
    step(M, 2000.0, true);                                         /* a polyline ahead: the plain phases, which flush first */
    step(M, DT, true, 4);
    step_refused(M, 9000.0, true, -7, "time knots of the wind lattice");
    step(M, DT, true, 3);
    /* a window that does not follow the pending step's: the clock moved under it */
    for (picles_ctx *c : M.c) ok(c, picles_tick(c, 300.0), "tick");
    if (!slabs) step_refused(M, DT, true, -6, "fusable step refused");      /* (picles_time_step has no plain detour here: as before) */
    for (picles_ctx *c : M.c) {
        g_calls++;
        if (picles_begin_fused_step(c, DT) != 1) die("a fused step was begun on a window that does not follow the pending one");
        ok(c, picles_begin_step(c, DT, PICLES_STEP_ZERO_FIRST), "begin_step");
        ok(c, picles_advance_rows(c, slabs ? PICLES_ROWS_EDGE : PICLES_ROWS_ALL, slabs ? M.sE : nullptr), "advance_rows");
        if (slabs) ok(c, picles_advance_rows(c, PICLES_ROWS_INTERIOR, M.sM), "advance_rows (interior)");
        ok(c, picles_scatter_remesh(c, slabs ? M.sM : nullptr), "scatter_remesh");
    }
    step(M, DT, true, 3);
    /* smooth3: three levels as a parabola, whatever the knots */
    lattice_mode(M, PICLES_LATTICE_SMOOTH3);
    step(M, DT, true, 3); step(M, 2000.0, true); step(M, DT, false); mid(M, true);
    lattice_mode(M, PICLES_LATTICE_LINEAR);
    step(M, DT, true, 2);
    /* a re-seed, with a step pending */
    for (picles_ctx *c : M.c) ok(c, picles_seed(c, 0.0), "seed (lattice)");
    step(M, DT, true, 3);
    checkpoint_round(M);
    step(M, DT, true, 3); step(M, 2000.0, false);
    /* back to host levels */
    host_static(M); step(M, DT, true, 2);
    host_knot(M); step(M, DT, false);
    lattice(M); step(M, DT, true, 2);                              /* a second lattice upload replaces the first */
    host_two(M); step(M, DT, false);
    for (picles_ctx *c : M.c) ok(c, picles_sync(c), "sync");
    destroy(M);
}

/* ---- every creation inside a lazily made pair fails in turn ---- */
/* before(M): a fresh model brought to where the next call() makes the pair; call(M, c): that call on one context */
template <class Before, class Call> void fail_each(const char *what, bool slabs, Before before, Call call, int creations)
{
    int k = 1;
    for (;; k++) {
        const long live0 = fake_hip_live();
        Model M = make_model(slabs);
        before(M);
        bool came = true;
        for (picles_ctx *c : M.c) {
            fake_hip_fail_alloc(k);
            const int rc = call(M, c);
            came = fake_hip_fail_alloc(0) <= 0;
            if (!came) { ok(c, rc, what); continue; }
            g_calls++; g_failed++;
            if (rc == 0) die(std::string(what) + " succeeded with a failed creation");
            if (!picles_last_error(c)[0]) die(std::string(what) + " failed without a text");
            ok(c, call(M, c), what);                              /* the same call again */
        }
        step(M, DT, true, 3); step(M, DT, false);                   /* launches behind it: the hook sees whole pairs only */
        for (picles_ctx *c : M.c) ok(c, picles_sync(c), "sync");
        destroy(M);
        if (fake_hip_live() != live0) die(std::string(what) + " left something behind");
        if (!came) break;
    }
    if (k - 1 != creations) die(std::string(what) + " made " + std::to_string(k - 1) + " creations, not " + std::to_string(creations));
}
void failed_creations(bool slabs)
{
    auto seeded = [](Model &M) { host_static(M); for (picles_ctx *c : M.c) ok(c, picles_seed(c, 0.0), "seed"); };
    auto on_lattice = [&](Model &M) { seeded(M); lattice(M); };
    /* the middle level: from the host, and from a lattice step with a knot inside ([600, 1200] holds the knot at 900) */
    fail_each("set_winds3 (the middle pair)", slabs, seeded, [](Model &M, picles_ctx *c) {
        Levels L(M.n, 3);
        return picles_set_winds3(c, L.pu[0], L.pv[0], picles_clock(c), L.pu[1], L.pv[1], L.pu[2], L.pv[2], picles_clock(c) + DT);
    }, 2);
    fail_each("a lattice step with a knot (the middle pair)", slabs, [&](Model &M) { on_lattice(M); step(M, DT, false); },
              [](Model &M, picles_ctx *c) { return step_one(M, c, DT, false); }, 2);
    /* the previous level 0: the second fused step under a lattice */
    fail_each("the second fused lattice step (the previous-level pair)", slabs, [&](Model &M) { on_lattice(M); step(M, DT, true); },
              [](Model &M, picles_ctx *c) { return step_one(M, c, 300.0, true); }, 2);
    /* the polyline buffers: from the host, from a lattice step with two knots, and grown for a longer polyline */
    fail_each("set_winds_polyline (the polyline pair, behind the middle pair)", slabs, seeded, [](Model &M, picles_ctx *c) {
        Levels L(M.n, 4);
        return host_polyline_rc(M, c, 2, L);
    }, 4);
    fail_each("a lattice step with two knots (the polyline pair)", slabs, on_lattice,
              [](Model &M, picles_ctx *c) { return step_one(M, c, 2000.0, false); }, 2);
    fail_each("a longer polyline (the polyline pair, grown)", slabs, [&](Model &M) { seeded(M); host_polyline(M, 2); step(M, DT, false); },
              [](Model &M, picles_ctx *c) {
        Levels L(M.n, 6);
        return host_polyline_rc(M, c, 4, L);
    }, 2);
}
}   // namespace

int main(int argc, char **argv)
{
    const bool trace_only = argc > 1 && !strcmp(argv[1], "trace");
    if (picles_abi_version() != PICLES_ABI_VERSION) { fprintf(stderr, "ABI version\n"); return 2; }
    fake_hip_launch_hook(hook);
    const long live = fake_hip_live();
    walk(false);
    walk(true);
    if (!trace_only) { failed_creations(false); failed_creations(true); }
    if (fake_hip_live() != live) die("blocks or events alive at the end");
    if (!g_fused || !g_plain || !g_samples) die("the slabs took no fused step, no plain step, or nothing was sampled");
    printf("wind harness: %ld ABI calls, %ld refused as documented, %ld launches seen, %ld lattice levels sampled, %ld creations failed, "
           "no sanitizer report\n", g_calls, g_refused, g_launches, g_samples, g_failed);
    return 0;
}
