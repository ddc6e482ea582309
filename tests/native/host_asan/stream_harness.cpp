// stream_harness.cpp — the host side of the wind stream (picles_wind_stream_*, and what picles_seed, the step entry points and the
// checkpoint do under one) and of picles_diag_export under AddressSanitizer, on top of fake_hip.cpp like wind_harness.cpp.  One
// fixed program, no random numbers.  Every level k is pushed as planes filled with ITS TIME t0 + k dt, and the launch hook plays
// k_wind_sample_ring on element 0: L_s0 + (L_s1 - L_s0) f of the slots it is handed IS the time the library meant to sample, so at
// every launch that takes KParams the hook holds the window's planes against the window's own times — a wrong slot, a stale level or
// a wrong weight shows as a plane that holds another time.  k_wind_ingest is played whole (the widening).
// The walk: refusals before init; init; seed with and without its levels; steps refused for a missing level (the text names it);
// TWO / KNOT windows, fused chunks, pushes around the ring from the host and from "device" memory (f64, f32, with a caller stream and
// without), out of order, onto a needed slot; a step with more knots than the ring carries; smooth3; a checkpoint taken and loaded,
// here and into a context of another ring size; reset; slab mode against a stream, both ways; a polyline window in a ring of five;
// picles_diag_export with and without partials; the stream replaced by a lattice.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan_stream.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../picles_amd/csrc/kernels.h"      /* KParams, GridP, Arrays */

extern "C" void fake_hip_launch_hook(void (*f)(const char *kernel, void **args));

namespace {
long g_calls = 0, g_refused = 0, g_samples = 0, g_windows = 0, g_ingests = 0;
const double T0 = -600.0, LAT_DT = 900.0, DT = 600.0;
const int LNX = 5, LNY = 4;

void die(const std::string &what) { fprintf(stderr, "stream harness: %s\n", what.c_str()); exit(3); }
void ok(picles_ctx *c, int rc, const char *what)
{
    g_calls++;
    if (rc != 0) { fprintf(stderr, "stream harness: %s failed rc=%d: %s\n", what, rc, picles_last_error(c)); exit(3); }
}
void refused(picles_ctx *c, int rc, const char *what, int code, const char *text)
{
    g_calls++; g_refused++;
    if (rc != code) die(std::string(what) + " gave " + std::to_string(rc) + ", not " + std::to_string(code) + ": " + picles_last_error(c));
    if (!strstr(picles_last_error(c), text)) die(std::string(what) + ": the text is \"" + picles_last_error(c) + "\"");
}

/* the argument structs of the two kernels as picles_hip.hip declares them (they live in no header) */
struct WindGridArg { int nx, ny, nt; double x0, inv_dx, y0, inv_dy, t0, inv_dt; double mesh_x0, mesh_y0, mesh_dx, mesh_dy; const double *u, *v; };
struct RingOut { int s0[2], s1[2]; double f[2]; double *u[2], *v[2]; };

bool has(const char *name, const char *piece) { return strstr(name, piece) != nullptr; }
bool near(double a, double b) { return std::fabs(a - b) <= 1e-6; }
void hook(const char *name, void **args)
{
    if (has(name, "k_wind_sample_ring")) {
        const int nt = has(name, "ILi2E") ? 2 : 1;
        const WindGridArg &W = *(const WindGridArg *)args[1];
        const RingOut &O = *(const RingOut *)args[2];
        const size_t st = (size_t)W.nx * W.ny;
        for (int q = 0; q < nt; q++) {
            if (!O.u[q] || !O.v[q]) die("k_wind_sample_ring is handed a null plane");
            if (O.s0[q] < 0 || O.s0[q] >= W.nt || O.s1[q] < 0 || O.s1[q] >= W.nt) die("a slot outside the ring reaches k_wind_sample_ring");
            if (!(O.f[q] >= 0.0 && O.f[q] < 1.0) || (O.f[q] == 0.0 && O.s1[q] != O.s0[q])) die("a bad weight reaches k_wind_sample_ring");
            for (int cpt = 0; cpt < 2; cpt++) {
                const double *F = cpt ? W.v : W.u;
                const double a = F[O.s0[q] * st + st - 1], b = F[O.s1[q] * st + st - 1];      /* (the last element: the whole plane was filled) */
                (cpt ? O.v[q] : O.u[q])[0] = O.f[q] != 0.0 ? a + (b - a) * O.f[q] : a;
            }
            g_samples++;
        }
        return;
    }
    if (has(name, "k_wind_sample")) die("the lattice sampler is launched under a wind stream");
    if (has(name, "k_wind_ingest")) {
        const float *u = *(const float **)args[0], *v = *(const float **)args[1];
        double *du = *(double **)args[2], *dv = *(double **)args[3];
        const long long n = *(const long long *)args[4];
        for (long long k = 0; k < n; k++) { du[k] = (double)u[k]; dv[k] = (double)v[k]; }
        g_ingests++;
        return;
    }
    const bool seed = has(name, "k_seed");
    if (!(seed || has(name, "k_advance") || has(name, "k_step"))) return;
    const KParams &P = *(const KParams *)args[0];
    const Arrays &A = *(const Arrays *)args[2];
    if (P.wind_static) die("a static window reaches a launch under a wind stream");
    /* level 0 holds the window's start; a seed's window holds the same level twice; else level 1 holds its end, the middle level of
     * a KNOT window its knot and of a PARABOLA its middle */
    const double t0 = P.tw0, t1 = P.tw0 + 1.0 / P.inv_dtw;
    if (seed) {
        if (A.u0[0] != A.u1[0] || A.v0[0] != A.v1[0]) die("the seed's window does not hold one level twice");
        g_windows++;
        return;
    }
    if (!near(A.u0[0], t0) || !near(A.v0[0], t0)) die("level 0 holds t = " + std::to_string(A.u0[0]) + ", the window starts at " + std::to_string(t0));
    if (!near(A.u1[0], t1) || !near(A.v1[0], t1)) die("level 1 holds t = " + std::to_string(A.u1[0]) + ", the window ends at " + std::to_string(t1));
    if (A.um && P.wind_nk <= 1) {
        const double tm = P.wind_nk == 1 ? t0 + P.wind_sk / P.inv_dtw : 0.5 * (t0 + t1);
        if (!near(A.um[0], tm) || !near(A.vm[0], tm)) die("the middle level holds t = " + std::to_string(A.um[0]) + ", not " + std::to_string(tm));
    }
    g_windows++;
}

picles_ctx *make_context()
{
    picles_grid g; picles_phys p; picles_ode o; picles_model m;
    memset(&g, 0, sizeof g); memset(&p, 0, sizeof p); memset(&o, 0, sizeof o); memset(&m, 0, sizeof m);
    g.Nx = 16; g.Ny = 16; g.dx = 2000.0; g.dy = 1500.0; g.periodic_x = 1; g.periodic_y = 1; g.j_begin = 0; g.j_end = 16;
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

int init(picles_ctx *c, int slots) { return picles_wind_stream_init(c, LNX, LNY, 0.0, 8000.0, 0.0, 8000.0, T0, LAT_DT, 0.0, 0.0, slots); }

/* level k, exact-size planes filled with its time; where: 0 host f64, 1 host f32, 2 "device" f64, 3 "device" f32 */
int push(picles_ctx *c, long long k, int how, hipStream_t s = nullptr)
{
    const size_t n = (size_t)LNX * LNY;
    const double t = T0 + (double)k * LAT_DT;
    std::vector<double> d(n, t);
    std::vector<float> f(n, (float)t);
    const bool f32 = how & 1;
    const void *src = f32 ? (const void *)f.data() : (const void *)d.data();
    const size_t bytes = n * (f32 ? 4 : 8);
    if (how < 2) return picles_wind_stream_push(c, k, src, src, f32 ? PICLES_WIND_F32 : PICLES_WIND_F64, PICLES_WIND_HOST, nullptr);
    void *du = nullptr, *dv = nullptr;
    if (hipMalloc(&du, bytes) != hipSuccess || hipMalloc(&dv, bytes) != hipSuccess) die("hipMalloc");
    hipMemcpy(du, src, bytes, hipMemcpyHostToDevice);
    hipMemcpy(dv, src, bytes, hipMemcpyHostToDevice);
    const int rc = picles_wind_stream_push(c, k, du, dv, f32 ? PICLES_WIND_F32 : PICLES_WIND_F64, PICLES_WIND_DEVICE, s);
    hipFree(du); hipFree(dv);
    return rc;
}

void info_is(picles_ctx *c, int slots, long long oldest, long long newest, long long pushes)
{
    int32_t s = -1;
    int64_t o = -9, n = -9, p = -9;
    ok(c, picles_wind_stream_info(c, &s, &o, &n, &p), "picles_wind_stream_info");
    if (s != slots || o != oldest || n != newest || p != pushes)
        die("info gives " + std::to_string(s) + " slots, levels " + std::to_string(o) + " .. " + std::to_string(n) + ", " + std::to_string(p) + " pushes; expected " +
            std::to_string(slots) + ", " + std::to_string(oldest) + " .. " + std::to_string(newest) + ", " + std::to_string(pushes));
    ok(c, picles_wind_stream_info(c, nullptr, nullptr, nullptr, nullptr), "picles_wind_stream_info (no outputs)");
}
}      // namespace

int main()
{
    if (picles_abi_version() != PICLES_ABI_VERSION || PICLES_ABI_VERSION < 17) { fprintf(stderr, "ABI version\n"); return 2; }
    fake_hip_launch_hook(hook);
    hipStream_t caller = nullptr;
    if (hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) != hipSuccess) die("hipStreamCreateWithFlags");

    /* the time rule */
    {
        int64_t k = -1; double f = -1.0;
        g_calls++;
        if (picles_wind_stream_coord(T0, LAT_DT, T0 + 2.5 * LAT_DT, &k, &f) != 0 || k != 2 || f != 0.5) die("coord of 2.5 intervals");
        if (picles_wind_stream_coord(T0, LAT_DT, T0 + 3.0 * LAT_DT * (1.0 + 1e-12), &k, &f) != 0 || k != 3 || f != 0.0) die("coord beside a level");
        if (picles_wind_stream_coord(T0, LAT_DT, T0 - 1.0, &k, &f) != -2 || picles_wind_stream_coord(T0, 0.0, T0, &k, &f) != -2) die("coord refusals");
        if (picles_wind_stream_coord(T0, LAT_DT, T0, nullptr, nullptr) != 0) die("coord without outputs");
    }

    picles_ctx *c = make_context();
    /* before init */
    refused(c, push(c, 0, 0), "push before init", -2, "picles_wind_stream_init first");
    refused(c, picles_wind_stream_reset(c), "reset before init", -2, "picles_wind_stream_init first");
    g_calls++;
    if (picles_wind_stream_info(c, nullptr, nullptr, nullptr, nullptr) != -1) die("info before init");
    refused(c, init(c, 1), "init with one slot", -2, "n_slots must be");
    refused(c, picles_wind_stream_init(c, 1, LNY, 0.0, 8000.0, 0.0, 8000.0, T0, LAT_DT, 0.0, 0.0, 3), "init with one x knot", -2, "positive spacing");
    refused(c, picles_wind_stream_init(c, LNX, LNY, 0.0, 8000.0, 0.0, 8000.0, T0, 0.0, 0.0, 0.0, 3), "init with dt = 0", -2, "positive spacing");
    ok(c, init(c, 3), "picles_wind_stream_init");
    info_is(c, 3, -1, -1, 0);

    /* picles_seed reads the winds at time 0.0, two thirds into the stream's first interval: levels 0 and 1 */
    refused(c, picles_seed(c, 0.0), "seed without a level", -2, "level k = 0");
    ok(c, push(c, 0, 0), "push 0 (host f64)");
    refused(c, picles_seed(c, 0.0), "seed without level 1", -2, "level k = 1 (t = 300)");
    refused(c, picles_wind_stream_push(c, 1, nullptr, nullptr, 0, 0, nullptr), "push without planes", -2, "both planes");
    {
        double x = 0.0;
        refused(c, picles_wind_stream_push(c, 1, &x, &x, 5, 0, nullptr), "push of an unknown dtype", -2, "dtype must be");
        refused(c, picles_wind_stream_push(c, 1, &x, &x, 0, 2, nullptr), "push to an unknown place", -2, "dtype must be");
    }
    ok(c, push(c, 1, 2, caller), "push 1 (device f64, caller stream)");
    info_is(c, 3, 0, 1, 2);
    ok(c, picles_seed(c, 0.0), "picles_seed");

    /* steps: refused for a missing level with a text that names it, by every entry point; then the windows */
    refused(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "time_step without level 2", -2, "reads level k = 2 (t = 1200)");
    refused(c, picles_run_steps(c, DT, 2), "run_steps without level 2", -2, "picles_run_steps: step 1 of this call");
    refused(c, picles_begin_fused_step(c, DT), "begin_fused_step without level 2", -2, "reads level k = 2");
    refused(c, picles_begin_step(c, DT, 0), "begin_step without level 2", -2, "reads level k = 2");
    refused(c, picles_advance(c, DT, 0), "advance without level 2", -2, "reads level k = 2");
    ok(c, push(c, 2, 3, caller), "push 2 (device f32, caller stream)");
    refused(c, picles_run_steps(c, DT, 3), "run_steps without level 3", -2, "picles_run_steps: step 3 of this call");
    refused(c, push(c, 2, 0), "push 2 again", -2, "out of order");
    refused(c, push(c, 4, 0), "push 4 before 3", -2, "the next one is k = 3");
    refused(c, push(c, -1, 0), "push -1", -2, "out of order");
    refused(c, push(c, 3, 0), "push 3 onto the slot of level 0", -2, "still needs");
    info_is(c, 3, 0, 2, 3);
    ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "step [0, 600]: KNOT at 300");
    ok(c, push(c, 3, 1), "push 3 (host f32)");
    info_is(c, 3, 1, 3, 4);
    ok(c, picles_run_steps(c, DT, 2), "steps [600, 1200], [1200, 1800]: TWO, fused");
    refused(c, picles_run_steps(c, DT, 2), "run_steps past level 3", -2, "reads level k = 4 (t = 3000)");
    ok(c, push(c, 4, 2, nullptr), "push 4 (device f64, no caller stream)");
    ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "step [1800, 2400]: KNOT at 2100, behind the pending step");
    refused(c, picles_time_step(c, 4000.0, PICLES_STEP_ZERO_FIRST), "a step with four knots in a ring of three", -2, "n_slots >= nk + 2");
    refused(c, picles_set_slab_mode(c, 1), "slab mode after the seed", -2, "before picles_seed");
    ok(c, picles_sync(c), "picles_sync");

    /* smooth3: three samples a window */
    ok(c, picles_set_wind_grid_mode(c, PICLES_LATTICE_SMOOTH3), "smooth3");
    ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "step [2400, 3000]: PARABOLA");
    ok(c, push(c, 5, 0), "push 5");
    ok(c, picles_run_steps(c, DT, 1), "step [3000, 3600]: PARABOLA");
    ok(c, picles_set_wind_grid_mode(c, PICLES_LATTICE_LINEAR), "linear");

    /* checkpoint: the blob holds no levels; the ring keeps its own; another ring size is another configuration */
    size_t bytes = 0;
    ok(c, picles_checkpoint_size(c, &bytes), "picles_checkpoint_size");
    std::vector<unsigned char> blob(bytes);
    ok(c, picles_checkpoint_begin(c), "picles_checkpoint_begin");
    ok(c, picles_checkpoint_end(c, blob.data(), bytes), "picles_checkpoint_end");
    ok(c, push(c, 6, 0), "push 6");
    ok(c, picles_run_steps(c, DT, 2), "steps [3600, 4200], [4200, 4800]");
    ok(c, picles_checkpoint_load(c, blob.data(), bytes), "picles_checkpoint_load (same context)");
    if (picles_clock(c) != 6 * DT) die("the restored clock");
    info_is(c, 3, 4, 6, 7);
    ok(c, picles_run_steps(c, DT, 2), "steps [3600, 4200], [4200, 4800] again: the levels in the ring stayed valid");
    {
        picles_ctx *d = make_context();
        ok(d, init(d, 4), "init (four slots)");
        refused(d, picles_checkpoint_load(d, blob.data(), bytes), "load into a ring of another size", PICLES_CKPT_E_CONFIG, "another configuration");
        ok(d, init(d, 3), "init (three slots)");
        ok(d, picles_checkpoint_load(d, blob.data(), bytes), "picles_checkpoint_load (fresh context)");
        refused(d, picles_run_steps(d, DT, 1), "a fresh context steps without levels", -2, "reads level k = 4");
        for (long long k = 4; k <= 6; k++) ok(d, push(d, k, 0), "push (the first push may be any k)");
        info_is(d, 3, 4, 6, 3);
        ok(d, picles_run_steps(d, DT, 2), "steps [3600, 4200], [4200, 4800] in the fresh context");
        refused(d, picles_run_steps(d, DT, 1), "the next one", -2, "reads level k = 7");
        ok(d, picles_destroy(d), "picles_destroy");
        /* slab mode against a stream, both ways; a lattice replaces a stream */
        d = make_context();
        ok(d, init(d, 3), "init");
        refused(d, picles_set_slab_mode(d, 1), "slab mode with a stream", -5, "holds a wind stream");
        std::vector<double> lat((size_t)LNX * LNY * 2, 1.0);
        ok(d, picles_set_wind_grid(d, LNX, LNY, 2, 0.0, 8000.0, 0.0, 8000.0, 0.0, LAT_DT, lat.data(), lat.data(), 0.0, 0.0), "a lattice replaces the stream");
        g_calls++;
        if (picles_wind_stream_info(d, nullptr, nullptr, nullptr, nullptr) != -1) die("info after the stream was replaced");
        refused(d, push(d, 0, 0), "push after the stream was replaced", -2, "picles_wind_stream_init first");
        ok(d, picles_set_slab_mode(d, 1), "slab mode without one");
        refused(d, init(d, 3), "init in slab mode", -5, "whole-grid context");
        ok(d, picles_destroy(d), "picles_destroy");
    }

    /* reset: the ring is empty, the window invalid; any level may come first */
    ok(c, picles_wind_stream_reset(c), "picles_wind_stream_reset");
    info_is(c, 3, -1, -1, 7);
    refused(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "a step after the reset", -2, "reads level k = 6");
    ok(c, push(c, 6, 0), "push 6");
    ok(c, push(c, 7, 3, caller), "push 7");
    ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "step [4800, 5400]");

    /* a ring of five carries a step with three knots inside: a polyline window through the plain phases */
    ok(c, init(c, 5), "init (five slots) replaces the ring");
    info_is(c, 5, -1, -1, 0);
    for (long long k = 6; k <= 10; k++) ok(c, push(c, k, (int)(k & 3), caller), "push");
    refused(c, push(c, 11, 0), "push onto the clock's level", -2, "still needs");
    ok(c, picles_time_step(c, 3000.0, PICLES_STEP_ZERO_FIRST), "step [5400, 8400]: knots at 5700, 6600, 7500");
    ok(c, push(c, 11, 0), "push 11");
    ok(c, picles_time_step(c, DT, PICLES_STEP_ZERO_FIRST), "step [8400, 9000]");

    /* the diagnostics into the caller's device buffers */
    refused(c, picles_diag_export(c, &bytes, nullptr, nullptr), "export before init", -2, "picles_diag_init first");
    ok(c, picles_diag_init(c, 4, 4, PICLES_DIAG_ALL, 1), "picles_diag_init");
    {
        int32_t nxc, nyc, nf, np;
        size_t fb;
        ok(c, picles_diag_shape(c, &nxc, &nyc, &nf, &np, &fb), "picles_diag_shape");
        void *fd = nullptr, *pd = nullptr;
        if (hipMalloc(&fd, fb) != hipSuccess || hipMalloc(&pd, (size_t)np * 7 * 8) != hipSuccess) die("hipMalloc");
        refused(c, picles_diag_export(c, nullptr, (double *)pd, caller), "export without a field buffer", -2, "no device buffer");
        ok(c, picles_diag_export(c, fd, (double *)pd, caller), "picles_diag_export");
        ok(c, picles_diag_export(c, fd, nullptr, nullptr), "picles_diag_export (no partials, no stream)");
        ok(c, picles_diag_export(c, fd, nullptr, caller), "picles_diag_export (no partials)");
        g_calls++;
        if (picles_diag_pending(c) != 0) die("an export took a ring slot");
        ok(c, picles_diag_push(c), "picles_diag_push");
        std::vector<unsigned char> f(fb);
        std::vector<double> p((size_t)np * 7);
        ok(c, picles_diag_pop(c, f.data(), p.data(), nullptr), "picles_diag_pop");
        hipFree(fd); hipFree(pd);
    }
    ok(c, picles_destroy(c), "picles_destroy");
    hipStreamDestroy(caller);
    if (g_samples < 20 || g_windows < 10 || g_ingests < 3) die("the walk did not reach the launches it was written for");
    printf("stream harness: %ld calls, %ld refused, %ld ring samples, %ld windows checked, %ld ingests: no sanitizer report\n",
           g_calls, g_refused, g_samples, g_windows, g_ingests);
    return 0;
}
