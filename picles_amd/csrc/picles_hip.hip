/*
 * picles_hip.hip — the C ABI of include/picles_hip.h (host side) and the HIP kernels (gfx950 / CDNA4) that are not
 * flavoured: k_seed, k_scatter, k_remesh, k_push_tiles, the cell list, k_wind_sample.  The flavoured kernel families live in
 * their own translation units so that they compile in parallel — k_step_explicit.hip, k_step_auto.hip (template in
 * k_step.inc), k_advance.hip, k_bforce.hip — and kernels.h holds the device code all of them share.
 *
 * One context = one GPU = one y-slab of the 2D Cartesian mesh.  Particles are born at and
 * return to their node every model step (mapping_2D.jl:279-356), so particle k IS node k:
 * the particle SoA, the State planes and the cell list share one index (identity cell list).
 *
 * HBM layout (all fp64 unless noted; i fastest, local rows jl = j - j_begin):
 *   state[3][n]      e, m_x, m_y planes              (reference State[Nx,Ny,3], col-major)
 *   movie[3][n]      MovieState snapshot
 *   z[5][n]          lne, c̄x, c̄y, x, y planes        (ParticleInstance2D.ODEIntegrator.u)
 *   qold[n], dtn[n]  PI-controller memory ln(qold), next dt (<0 => auto_dt_reset!); asw[n] i32 AutoSwitch state (solver 2)
 *   on[n] u8, pflags[n] u8 (bit0 stepped, bit1 group-2 (mask 3), bit2 boundary), status[n] i32
 *   wind u0,v0,u1,v1 [n] (+ uP,vP: level 0 of the previous window, for fused steps under device-sampled winds)
 *   rec[(ny_loc+2R)][6][Nx]   per-row scatter records e, m_x, m_y, wx_hi, wy_hi, code(list, floor x, floor y)
 *                    (+R ghost rows per side = the halo blocks exchanged between slabs; a row
 *                    block is contiguous, so halo send/recv need no pack/unpack)
 *
 * Kernels and the roofline that bounds each (DESIGN.md has the numbers):
 *   k_step           ONE launch per model step for run!-style steps: pull-scatter + remesh of the previous step,
 *                    whole adaptive advance of this one, new record.  Flavours (compile time): solver (DP5 / Tsit5 /
 *                    auto-switching), dead band, static vs time-varying winds, per-node metric.  fp64-VALU bound.
 *   k_advance        per-particle step alone: guards + adaptive RK of the 5-vector in
 *                    registers + charge/record write.  fp64-VALU bound (~10^4..10^5 flop per
 *                    particle-step against 136 B).  No MFMA: not a contraction.
 *   k_scatter        deterministic PULL scatter (each node sums its <= (2R+1)^2 candidate
 *                    sources in the reference's sequential order => bitwise reproducible),
 *                    fused with State zero-fill, MovieState snapshot and remesh. HBM bound.
 *   k_push_tiles     PUSH scatter: LDS-staged grid tile + apron, ds_add_f64 inside the tile,
 *                    one global fp64 atomic per touched tile node. HBM/atomic bound.
 *   k_remesh         stand-alone NodeToParticle! (split API).
 *   k_bforce         (k_bforce.hip) open-boundary forcing: behind the launch that writes a step's records, one lane per forced rim
 *                    node bears a particle from the prescribed sea state, advances it and leaves its record.  Latency bound.
 *   k_ckpt           checkpoint payload: packs / verifies / unpacks the planes of a restart blob in one pass. HBM bound.
 *   k_flux           (k_flux.h) coupling fluxes: wind input, dissipation, stress and Stokes drift planes + one partial per tile
 *   k_flux_mean_update, k_flux_mean_final   (k_flux_mean.h) flux means: the cell sums of k_flux added to fp64 accumulators behind every
 *                    step, from the scatter records where a fused step is pending; the interval mean in k_flux's planes and partials
 *   k_diag           (k_diag.h) coarse wave diagnostics: float32 Hs / Tp / cg planes + one partial of sums and maxima per tile of
 *                    256 coarse cells, one pass over State. HBM bound.
 */
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/picles_hip.h"
#include "physics.h"

#define PX_EXPORT extern "C" __attribute__((visibility("default")))

#include "kernels.h"
#include "k_diag.h"
#include "k_flux.h"
#include "k_probe.h"
#include "k_stat.h"
#include "k_flux_mean.h"
#include "k_nest.h"
#include "k_track.h"

/* ------------------------------------------------------------------------------------------
 * k_seed — init_particles! / SeedParticle / InitParticleValues / init_z0_to_State!
 * (run.jl:199-247, core_2D.jl:247-288,434-488, initialize.jl:14-17)
 * ---------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(256) k_seed(KParams P, GridP G, Arrays A, const signed char *mask, double seed_T)
{
    pm_device_init();
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n) return;
    int i = (int)(t % G.Nx), jl = (int)(t / G.Nx);
    Vec5 z = {0.0, 0.0, 0.0, 0.0, 0.0};
    int on = 0;
    double e = 0.0, mx = 0.0, my = 0.0;
    if (mask[t] != 0) {
        Wind w = load_wind<true>(P, A, t);
        double u, v;
        wind_at<true>(P, w, 0.0, u, v);   /* winds at t = 0.0 (run.jl:213-215) */
        if (P.init_type == 0) {
            if (__builtin_sqrt(u * u + v * v) > __builtin_sqrt(2.0)) {
                seed_windsea(u, v, seed_T, z.lne, z.cx, z.cy);
                on = 1;
            } else {   /* MinimalParticle: unit-speed wind in the wind's direction (rand_sign -> +1) */
                double uu = (u == 0.0) ? 1.0 : u, vv = (v == 0.0) ? 1.0 : v;
                double am = __builtin_sqrt(uu * uu + vv * vv);
                seed_windsea(1.0 * uu / am, 1.0 * vv / am, seed_T, z.lne, z.cx, z.cy);
                on = 0;
            }
        } else {
            z.lne = P.def_lne; z.cx = P.def_cx; z.cy = P.def_cy;
            on = 1;
        }
        if (on) particle_to_charge(z.lne, z.cx, z.cy, e, mx, my);
    }
    A.z[t] = z.lne; A.z[t + A.n] = z.cx; A.z[t + 2 * A.n] = z.cy; A.z[t + 3 * A.n] = 0.0; A.z[t + 4 * A.n] = 0.0;
    A.on[t] = (unsigned char)on;
    A.qold[t] = PI_LNQOLDINIT;
    A.asw[t] = ASW_FRESH;
    A.dtn[t] = P.dt0;
    A.status[t] = 0;
    A.state[t] = e; A.state[t + A.n] = mx; A.state[t + 2 * A.n] = my;
    double *rr = rec_row(A, G, jl + G.R);
    rr[5 * G.Nx + i] = 0.0;
}

template <bool REMESH>
__global__ void __launch_bounds__(256) k_scatter(KParams P, GridP G, Arrays A, int accum, int movie,
                                                   double clock, double DT)
{
    if (REMESH) pm_device_init();
    long long t = (long long)xcd_block() * PICLES_BLOCK + threadIdx.x;
    unsigned int reseeds = 0;
    const bool active = t < A.n;
    if (active) {
        int i = (int)(t % G.Nx), jl = (int)(t / G.Nx);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (accum) { s0 = A.state[t]; s1 = A.state[t + A.n]; s2 = A.state[t + 2 * A.n]; }
        pull_any(G, A, i, jl, pull_reach_local(G, A, i, jl, pull_reach(G, A, jl)), s0, s1, s2);
        if (movie) {
            A.movie[t] = s0; A.movie[t + A.n] = s1; A.movie[t + 2 * A.n] = s2;
            A.state[t] = 0.0; A.state[t + A.n] = 0.0; A.state[t + 2 * A.n] = 0.0;
        } else {
            A.state[t] = s0; A.state[t + A.n] = s1; A.state[t + 2 * A.n] = s2;
        }
        if (REMESH) {
            unsigned char pf = A.pflags[t];
            if (pf & PF_STEPPED) remesh_particle(P, A, t, pf, s0, s1, s2, clock, DT, reseeds);
        }
    }
    if (REMESH) {
        unsigned long long s = wave_sum_u64(reseeds);
        if ((threadIdx.x & 63) == 0 && s)
            atomicAdd(&A.cnt[(blockIdx.x * 4u + (threadIdx.x >> 6)) & (NSLOTS - 1)].reseeds, s);
    }
}

/* stand-alone time_step!_remesh (TimeSteppers.jl:182-193) */
__global__ void __launch_bounds__(256) k_remesh(KParams P, GridP G, Arrays A, double clock, double DT)
{
    pm_device_init();
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned int reseeds = 0;
    if (t < A.n) {
        unsigned char pf = A.pflags[t];
        if (pf & PF_STEPPED)
            remesh_particle(P, A, t, pf, A.state[t], A.state[t + A.n], A.state[t + 2 * A.n], clock, DT, reseeds);
    }
    unsigned long long s = wave_sum_u64(reseeds);
    if ((threadIdx.x & 63) == 0 && s)
        atomicAdd(&A.cnt[(blockIdx.x * 4u + (threadIdx.x >> 6)) & (NSLOTS - 1)].reseeds, s);
}

/* ------------------------------------------------------------------------------------------
 * k_push_tiles — PUSH scatter with an LDS-staged grid tile.
 * One workgroup owns a TX×TY tile of birth nodes; its LDS holds the tile plus an apron of AP
 * nodes on every side (3 planes).  Every on-particle of the tile adds its 4 weighted corners
 * with ds_add_f64 (LDS atomics resolve same-node collisions inside the workgroup); corners
 * beyond the apron go straight to global fp64 atomics.  The LDS tile is then flushed with ONE
 * global atomic per touched node (drop / wrap by the grid's periodicity).
 * Sum order is not fixed => last-bit run-to-run differences; PICLES_STEP_ATOMIC selects it.
 * IDENTITY=true : particles = the tile's own nodes, read from the scatter records.
 * IDENTITY=false: particles = a cell-list segment of an arbitrary particle list
 *                 (picles_scatter_particles), sorted by the tile of the birth node.
 * ---------------------------------------------------------------------------------------- */
#define PT_TX 64
#define PT_TY 4
#define PT_AP 2
#define PT_LX (PT_TX + 2 * PT_AP)
#define PT_LY (PT_TY + 2 * PT_AP)

__device__ __forceinline__ void global_add3(const GridP &G, const Arrays &A, int ig, int jg, double a0, double a1, double a2)
{
    /* ig, jg: unwrapped global node indices */
    if (ig < 0 || ig >= G.Nx) { if (!G.periodic_x) return; ig %= G.Nx; if (ig < 0) ig += G.Nx; }
    if (jg < 0 || jg >= G.Ny) { if (!G.periodic_y) return; jg %= G.Ny; if (jg < 0) jg += G.Ny; }
    int jl = jg - G.j_begin;
    if (jl < 0 || jl >= G.ny_loc) return;   /* other slab: single-slab use only */
    long long t = (long long)jl * G.Nx + ig;
    unsafeAtomicAdd(&A.state[t], a0);
    unsafeAtomicAdd(&A.state[t + A.n], a1);
    unsafeAtomicAdd(&A.state[t + 2 * A.n], a2);
}

/* Wave-level pre-reduction of same-destination contributions (the "wavefront-reduced atomics" of the scatter design).
 * Every lane offers one contribution (value triple q, destination key; key < 0: nothing).  Lanes that are neighbours in
 * the wave and target the same node form a run; the run is summed with a segmented shuffle scan and its first lane
 * alone issues the LDS / global atomic.  With one particle per cell and lanes laid along x this turns the upper-x corner
 * of lane k and the lower-x corner of lane k+1 into ONE atomic (after rotating the upper corners by one lane); with a
 * cell-sorted particle list it also folds all particles of one cell.  Runs are short (2 in the identity layout), so the
 * scan stops as soon as no lane has a partner left: usually after one step. */
__device__ __forceinline__ bool wave_fold_runs(int key, double &q0, double &q1, double &q2)
{
    const int lane = threadIdx.x & 63;
    const int kl = __shfl_up(key, 1, 64);
    const bool head = (lane == 0) || (kl != key) || (key < 0);
    if (__ballot(!head) == 0) return key >= 0;             /* no two neighbouring lanes share a node */
    /* run id = number of run heads at or below this lane; two lanes belong to the same run iff the ids agree */
    const unsigned long long hb = __ballot(head);
    const int rid = __popcll(hb & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull)));
    for (int o = 1; o < 64; o <<= 1) {
        const double a0 = __shfl_down(q0, o, 64), a1 = __shfl_down(q1, o, 64), a2 = __shfl_down(q2, o, 64);
        const int r2 = __shfl_down(rid, o, 64);
        const bool take = (lane + o < 64) && (r2 == rid);
        if (take) { q0 += a0; q1 += a1; q2 += a2; }
        if (__ballot(take) == 0) break;                      /* every run is folded */
    }
    return head && key >= 0;
}

template <bool IDENTITY>
__global__ void __launch_bounds__(256) k_push_tiles(GridP G, Arrays A, int ntx,
                                                      const int *seg_start, const int *perm,
                                                      const int *pij, const double *pxy, const double *pch, long long np)
{
    __shared__ double tile[3][PT_LY][PT_LX];
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int i0 = tx * PT_TX, j0 = ty * PT_TY + G.j_begin;   /* global origin of the tile */
    for (int k = threadIdx.x; k < 3 * PT_LY * PT_LX; k += blockDim.x) (&tile[0][0][0])[k] = 0.0;
    __syncthreads();

    int count, base = 0;
    if (IDENTITY) count = PT_TX * PT_TY;
    else { base = seg_start[blockIdx.x]; count = seg_start[blockIdx.x + 1] - base; }
    const int rounds = (count + (int)blockDim.x - 1) / (int)blockDim.x;
    for (int rd = 0; rd < rounds; rd++) {                 /* whole waves stay together: the fold below shuffles across lanes */
        const int k = rd * (int)blockDim.x + (int)threadIdx.x;
        bool have = k < count;
        int ib = 0, jb = 0, bx = 0, by = 0;                /* birth node (global), cell offset */
        double e = 0.0, mx = 0.0, my = 0.0, wxh = 0.0, wyh = 0.0;
        if (have) {
            if (IDENTITY) {
                ib = i0 + (k % PT_TX);
                jb = j0 + (k / PT_TX);
                const int jl = jb - G.j_begin;
                have = ib < G.Nx && jl < G.ny_loc;
                if (have) {
                    const double *rr = rec_row(A, G, jl + G.R);
                    const double code = rr[5 * G.Nx + ib];
                    have = code != 0.0;
                    if (have) {
                        int cg;
                        rec_decode(code, cg, bx, by);
                        e = rr[ib]; mx = rr[G.Nx + ib]; my = rr[2 * G.Nx + ib]; wxh = rr[3 * G.Nx + ib]; wyh = rr[4 * G.Nx + ib];
                    }
                }
            } else {
                const long long pidx = perm[base + k];
                ib = pij[pidx]; jb = pij[np + pidx];
                const double x = pxy[pidx], y = pxy[np + pidx];
                e = pch[pidx]; mx = pch[np + pidx]; my = pch[2 * np + pidx];
                have = pm_isfinite(x) && pm_isfinite(y);
                if (have) { index_weight(x, bx, wxh); index_weight(y, by, wyh); }
            }
        }
        /* the four corners in two passes of (lower-x, upper-x) per y row.  The upper-x contributions are rotated by one
         * lane (lane k offers the upper corner of lane k-1) so that, in the identity layout, it sits next to the lower
         * corner of the particle one cell to the right — the same node. */
#pragma unroll
        for (int ay = 0; ay < 2; ay++) {
            const double wy = ay ? wyh : 1.0 - wyh;
            const int jg = jb + by + ay;
            int klo = -1;
            double l0 = 0.0, l1 = 0.0, l2 = 0.0;
#pragma unroll
            for (int ax = 0; ax < 2; ax++) {
                const double w = (ax ? wxh : 1.0 - wxh) * wy;
                double q0 = w * e, q1 = w * mx, q2 = w * my;
                int ig = ib + bx + ax, jgc = jg;
                int li = ig - i0 + PT_AP, lj = jgc - j0 + PT_AP;
                const bool inside = have && li >= 0 && li < PT_LX && lj >= 0 && lj < PT_LY;
                if (have && !inside) global_add3(G, A, ig, jgc, q0, q1, q2);      /* beyond the apron: rare, straight to HBM */
                int key = inside ? lj * PT_LX + li : -1;
                if (ax == 1) {                                /* rotate the upper-x corner to the right-hand neighbour lane */
                    const int lane = threadIdx.x & 63;
                    const int kk = __shfl_up(key, 1, 64);
                    const double r0 = __shfl_up(q0, 1, 64), r1 = __shfl_up(q1, 1, 64), r2 = __shfl_up(q2, 1, 64);
                    const int k63 = __shfl(key, 63, 64);       /* lane 63's own upper corner wraps to lane 0 */
                    const double s0 = __shfl(q0, 63, 64), s1 = __shfl(q1, 63, 64), s2 = __shfl(q2, 63, 64);
                    key = lane ? kk : k63; q0 = lane ? r0 : s0; q1 = lane ? r1 : s1; q2 = lane ? r2 : s2;
                    /* pair it with this lane's own lower corner of the same y row: two offers per lane, folded one after
                     * the other — first the rotated upper corner joins the lower one if they agree */
                }
                if (ax == 0) { klo = key; l0 = q0; l1 = q1; l2 = q2; }
                else {
                    if (key >= 0 && key == klo) { l0 += q0; l1 += q1; l2 += q2; key = -1; }    /* same node: one offer */
                    /* lower corners (now carrying the neighbour's upper one) */
                    double f0 = l0, f1 = l1, f2 = l2;
                    if (wave_fold_runs(klo, f0, f1, f2)) {
                        const int lj2 = klo / PT_LX, li2 = klo % PT_LX;
                        atomicAdd(&tile[0][lj2][li2], f0); atomicAdd(&tile[1][lj2][li2], f1); atomicAdd(&tile[2][lj2][li2], f2);
                    }
                    /* upper corners that found no partner (different cell offset next door, tile edge) */
                    if (__ballot(key >= 0)) {
                        if (wave_fold_runs(key, q0, q1, q2)) {
                            const int lj2 = key / PT_LX, li2 = key % PT_LX;
                            atomicAdd(&tile[0][lj2][li2], q0); atomicAdd(&tile[1][lj2][li2], q1); atomicAdd(&tile[2][lj2][li2], q2);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < PT_LY * PT_LX; k += blockDim.x) {
        int li = k % PT_LX, lj = k / PT_LX;
        double a0 = tile[0][lj][li], a1 = tile[1][lj][li], a2 = tile[2][lj][li];
        if (a0 == 0.0 && a1 == 0.0 && a2 == 0.0) continue;
        global_add3(G, A, i0 + li - PT_AP, j0 + lj - PT_AP, a0, a1, a2);
    }
}

/* cell list for an arbitrary particle list: histogram of birth tiles, then (after an exclusive
 * scan) a stable-enough fill of the permutation */
__global__ void k_tile_count(GridP G, int ntx, const int *pij, long long np, int *count, int *tile_of)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= np) return;
    int ib = pij[k], jb = pij[np + k] - G.j_begin;
    int tile = -1;
    if (ib >= 0 && ib < G.Nx && jb >= 0 && jb < G.ny_loc) {
        tile = (jb / PT_TY) * ntx + ib / PT_TX;
        atomicAdd(&count[tile], 1);
    }
    tile_of[k] = tile;
}
__global__ void k_tile_fill(long long np, const int *tile_of, const int *seg_start, int *cursor, int *perm)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= np) return;
    int tile = tile_of[k];
    if (tile < 0) return;
    int pos = atomicAdd(&cursor[tile], 1);
    perm[seg_start[tile] + pos] = (int)k;
}

/* ------------------------------------------------------------------------------------------
 * k_wind_sample — wind_interpolator (Utils/WindEmulator.jl:18-43): tri-linear interpolation of a
 * regular (x,y,t) lattice to the mesh nodes at time t, periodic continuation outside the lattice
 * (Interpolations.jl extrapolation_bc = Periodic(): period = last - first knot).
 * ---------------------------------------------------------------------------------------- */
struct WindGrid {
    int nx, ny, nt;
    double x0, inv_dx, y0, inv_dy, t0, inv_dt;
    double mesh_x0, mesh_y0, mesh_dx, mesh_dy;
    const double *u, *v;
};

__device__ __forceinline__ void lattice_coord(double c, int n, int &i0, double &f)
{
    /* c in lattice units; inside [0, n-1] as is, outside continued periodically */
    double per = (double)(n - 1);
    double w = (c < 0.0 || c > per) ? c - __builtin_floor(c / per) * per : c;
    double fl = __builtin_floor(w);
    i0 = (int)fl;
    if (i0 > n - 2) i0 = n - 2;   /* w == per after rounding */
    if (i0 < 0) i0 = 0;
    f = w - (double)i0;
}

/* NT time levels per launch (the spatial cell and its weights are shared): level q at time tq[q] goes to (uo[q], vo[q]) */
struct WindSampleOut { double t[2]; double *u[2], *v[2]; };
template <int NT>
__global__ void __launch_bounds__(256) k_wind_sample(GridP G, WindGrid Wg, WindSampleOut O, long long n)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int i = (int)(k % G.Nx), j = (int)(k / G.Nx) + G.j_begin;
    double x = Wg.mesh_x0 + (double)i * Wg.mesh_dx, y = Wg.mesh_y0 + (double)j * Wg.mesh_dy;
    int ix, iy;
    double fx, fy;
    lattice_coord((x - Wg.x0) * Wg.inv_dx, Wg.nx, ix, fx);
    lattice_coord((y - Wg.y0) * Wg.inv_dy, Wg.ny, iy, fy);
    size_t sx = 1, sy = (size_t)Wg.nx, st = (size_t)Wg.nx * Wg.ny;
    const double *F[2] = {Wg.u, Wg.v};
#pragma unroll
    for (int q = 0; q < NT; q++) {
        int it;
        double ft;
        lattice_coord((O.t[q] - Wg.t0) * Wg.inv_dt, Wg.nt, it, ft);
        size_t b = ix * sx + iy * sy + it * st;
        double out[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const double *f = F[c];
            double c00 = f[b] + (f[b + sx] - f[b]) * fx;
            double c10 = f[b + sy] + (f[b + sy + sx] - f[b + sy]) * fx;
            double c01 = f[b + st] + (f[b + st + sx] - f[b + st]) * fx;
            double c11 = f[b + st + sy] + (f[b + st + sy + sx] - f[b + st + sy]) * fx;
            double c0 = c00 + (c10 - c00) * fy;
            double c1 = c01 + (c11 - c01) * fy;
            out[c] = c0 + (c1 - c0) * ft;
        }
        O.u[q][k] = out[0];
        O.v[q][k] = out[1];
    }
}

/* k_wind_sample_ring — the same sample from a wind stream (picles_wind_stream_*): the lattice's time levels live in a ring of slots,
 * Wg.u / Wg.v are the ring's bases and a slot is one (x, y) plane.  The host has worked out, per level q, the slots of the two time
 * levels and the weight f (include/picles_hip.h, "the time rule"): uniform over the launch.  f == 0 reads slot s0 alone; otherwise the
 * operations are k_wind_sample's, in its order */
struct WindRingOut { int s0[2], s1[2]; double f[2]; double *u[2], *v[2]; };
template <int NT>
__global__ void __launch_bounds__(256) k_wind_sample_ring(GridP G, WindGrid Wg, WindRingOut O, long long n)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    int i = (int)(k % G.Nx), j = (int)(k / G.Nx) + G.j_begin;
    double x = Wg.mesh_x0 + (double)i * Wg.mesh_dx, y = Wg.mesh_y0 + (double)j * Wg.mesh_dy;
    int ix, iy;
    double fx, fy;
    lattice_coord((x - Wg.x0) * Wg.inv_dx, Wg.nx, ix, fx);
    lattice_coord((y - Wg.y0) * Wg.inv_dy, Wg.ny, iy, fy);
    size_t sx = 1, sy = (size_t)Wg.nx, st = (size_t)Wg.nx * Wg.ny;
    const double *F[2] = {Wg.u, Wg.v};
#pragma unroll
    for (int q = 0; q < NT; q++) {
        const double ft = O.f[q];
        size_t b0 = ix * sx + iy * sy + (size_t)O.s0[q] * st, b1 = ix * sx + iy * sy + (size_t)O.s1[q] * st;
        double out[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const double *f = F[c];
            double c00 = f[b0] + (f[b0 + sx] - f[b0]) * fx;
            double c10 = f[b0 + sy] + (f[b0 + sy + sx] - f[b0 + sy]) * fx;
            double c0 = c00 + (c10 - c00) * fy;
            if (ft != 0.0) {
                double c01 = f[b1] + (f[b1 + sx] - f[b1]) * fx;
                double c11 = f[b1 + sy] + (f[b1 + sy + sx] - f[b1 + sy]) * fx;
                double c1 = c01 + (c11 - c01) * fy;
                c0 = c0 + (c1 - c0) * ft;
            }
            out[c] = c0;
        }
        O.u[q][k] = out[0];
        O.v[q][k] = out[1];
    }
}

/* k_wind_ingest — a float32 level of a wind stream into its slot: both planes, widened (exact) */
__global__ void __launch_bounds__(256) k_wind_ingest(const float *__restrict__ u, const float *__restrict__ v,
                                                     double *__restrict__ du, double *__restrict__ dv, long long n)
{
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    du[k] = (double)u[k];
    dv[k] = (double)v[k];
}

/* ------------------------------------------------------------------------------------------
 * k_wind_poly — coefficients of a polyline window (KParams::wind_nk >= 2; physics.h, wind_eval): from the node's levels
 * L_0 (u0 plane), L_1 .. L_nk (lv planes, one pair per knot), L_nk+1 (u1 plane) the segment slopes per unit s,
 * sl_j = (L_j+1 - L_j) ilen_j, and their jumps at the knots:  du = sl_0,  b_k = sl_k - sl_k-1.  xb: [0, PICLES_MAX_KNOTS) the
 * knots' s, then planes du, dv, b_1u, b_1v, b_2u, ...
 * ---------------------------------------------------------------------------------------- */
struct WindPolyForm { int nk; double sk[PICLES_MAX_KNOTS]; double ilen[PICLES_MAX_KNOTS + 1]; };
__global__ void __launch_bounds__(256) k_wind_poly(WindPolyForm F, const double *u0, const double *v0, const double *u1, const double *v1,
                                                   const double *lv, double *xb, long long n)
{
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < PICLES_MAX_KNOTS) xb[t] = (t < F.nk) ? F.sk[t] : 2.0;    /* (beyond the window: never reached) */
    if (t >= n) return;
    double *pl = xb + PICLES_MAX_KNOTS;
    for (int c = 0; c < 2; c++) {
        double prev = c ? v0[t] : u0[t], slp = 0.0;
        for (int j = 0; j <= F.nk; j++) {
            const double next = (j < F.nk) ? lv[(size_t)(2 * j + c) * n + t] : (c ? v1[t] : u1[t]);
            const double sl = (next - prev) * F.ilen[j];
            pl[(size_t)(2 * j + c) * n + t] = j ? sl - slp : sl;
            slp = sl;
            prev = next;
        }
    }
}

/* ------------------------------------------------------------------------------------------
 * host side
 * ---------------------------------------------------------------------------------------- */
static thread_local std::string g_create_error;

/* configuration fingerprint of a checkpoint (picles_checkpoint_*): a 64-bit word hash, FNV-style multiply + fold */
static const uint64_t FP_SEED = 0xcbf29ce484222325ull;
static uint64_t fp_bytes(uint64_t h, const void *p, size_t bytes)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t k = 0;
    for (; k + 8 <= bytes; k += 8) {
        uint64_t w;
        memcpy(&w, b + k, 8);
        h = (h ^ w) * 0x100000001b3ull;
        h ^= h >> 29;
    }
    uint64_t w = (uint64_t)(bytes - k) << 56;
    if (k < bytes) { uint64_t t = 0; memcpy(&t, b + k, bytes - k); w ^= t; }
    h = (h ^ w) * 0x100000001b3ull;
    return h ^ (h >> 29);
}
template <class T> static uint64_t fp_val(uint64_t h, T v) { return fp_bytes(h, &v, sizeof v); }

/* The device-to-host ring behind snapshots (picles_store_*), coarse diagnostics (picles_diag_*) and station probes (picles_probe_*):
 * `cap` slots in ONE device block and ONE pinned host block, two events per slot.  A producer writes the slot
 * next_slot() hands out on its own stream and ships it: the copy to the host rides the context's store stream behind the slot's
 * `ready` event and is followed by its `done` event; a reader waits for the oldest slot's `done` alone.
 * stride: the slot size rounded up to 16 bytes, the widest alignment a slot's contents ask for (the diagnostics slot keeps its fp64
 * partials at a 16-byte-aligned offset behind the float32 planes; snapshots and probe samples are fp64 planes): both blocks start
 * on a far coarser boundary, so every slot, and the partials inside it, stay aligned as in a block of their own. */
struct OutRing {
    struct Slot { const unsigned char *host; double time; long long step; };
    unsigned char *dev = nullptr, *host = nullptr;
    size_t stride = 0;
    std::vector<hipEvent_t> ready, done;
    std::vector<double> time;                      /* c->clock when the slot was shipped */
    std::vector<long long> step;                   /* the producer's step count at that moment */
    int head = 0, count = 0, cap = 0;              /* cap == 0: no ring */

    int init(picles_ctx *c, int n_slots, size_t slot_bytes);      /* completes, or leaves nothing behind */
    void release();                                               /* idempotent; the caller has drained the streams that use the slots */
    unsigned char *next_slot() const { return count == cap ? nullptr : dev + (size_t)((head + count) % cap) * stride; }   /* nullptr: full */
    int ship(picles_ctx *c, unsigned char *slot, hipStream_t producer, size_t bytes, long long step_tag);
    int front(picles_ctx *c, Slot &out);                          /* waits for the oldest slot's copy alone */
    void drop() { head = (head + 1) % cap; count--; }
};

/* a sampling schedule counted in completed model steps: step s is due when s = first + k every */
struct Cadence {
    int every = 1, first = 1;
    long long steps = 0;                           /* model steps completed since the schedule was set */
    bool due(long long s) const { return s >= first && (s - first) % every == 0; }
    long long due_within(long long n_steps) const  /* samples the next n_steps model steps will take */
    {
        const long long a = steps + 1, b = steps + n_steps, f = first, e = every;
        if (b < f || n_steps <= 0) return 0;
        /* multiples f + k e inside [max(a, f), b] */
        const long long lo = a > f ? a : f;
        const long long k0 = (lo - f + e - 1) / e, k1 = (b - f) / e;
        return k1 >= k0 ? k1 - k0 + 1 : 0;
    }
};

/* The wind over one model step as the kernels see it: where its levels come from, its shape and [t0, t1], which time the
 * (u1, v1) planes hold, and the plane pairs that exist only once a form has needed them.  publish() is the only writer of the wind
 * fields of KParams and of A.um / A.vm; every pair is made whole or not at all (make_pair); the (u0, v0) / (u1, v1) / (uP, vP) planes
 * change places in reuse_swap() and rotate() alone. */
struct WindWindow {
    enum Form { STATIC, TWO, PARABOLA, KNOT, POLYLINE };
    /* three levels: the parabola through (t0, (t0 + t1)/2, t1), or two straight segments meeting at the knot tk[0]; a polyline has
     * nk >= 2 knots at tk[0 .. nk) */
    struct Shape { Form form = STATIC; int nk = 0; double tk[PICLES_MAX_KNOTS] = {}; };
    /* the source: levels the caller uploads (picles_set_winds*), or a lattice that k_wind_sample takes them from */
    bool lattice = false;
    int mode = PICLES_LATTICE_LINEAR;
    WindGrid wg{};
    double *d_wgu = nullptr, *d_wgv = nullptr;
    double lat_t0 = 0.0, lat_dt = 0.0;             /* the lattice's first time knot and spacing as the caller gave them (knot times are computed from these) */
    /* a wind stream (picles_wind_stream_*): a lattice (`lattice` is set too: the step paths are the lattice's) whose
     * time levels arrive one at a time.  d_wgu / d_wgv are then rings of ring_slots (x, y) planes, level k in slot k % ring_slots;
     * the levels [ring_oldest(), ring_newest] are held (ring_newest < 0: none).  Everything that reads or writes a slot is enqueued
     * on the context stream: stream order is all the ordering the ring needs */
    bool ring = false;
    int ring_slots = 0;
    long long ring_first = -1, ring_newest = -1, ring_pushes = 0;
    hipEvent_t ring_in = nullptr, ring_out = nullptr;      /* a device push: caller stream -> context stream -> caller stream */
    /* the window on the device */
    Shape shape;
    double t0 = 0.0, t1 = 0.0;
    bool held = false;                             /* (u1, v1) hold the lattice at time held_t */
    double held_t = 0.0;
    /* made on first use: the middle level (PARABOLA, KNOT); the polyline's levels at the knots (2 planes per knot) and coefficient
     * planes (k_wind_poly), with room for poly_cap knots; level 0 of the previous window is A.uP / A.vP */
    double *um_buf = nullptr, *vm_buf = nullptr;
    double *lv_buf = nullptr, *xb_buf = nullptr;
    int poly_cap = 0;
    double *sp_u = nullptr, *sp_v = nullptr;       /* a spare pair: the lattice's level at a time that is none of the window's (sample_spare) */

    bool static_() const { return shape.form == STATIC; }
    bool polyline() const { return shape.form == POLYLINE; }
    bool from_lattice() const { return lattice; }
    bool streamed() const { return ring; }
    long long ring_oldest() const { return ring_newest < 0 ? -1 : std::max(ring_first, ring_newest - ring_slots + 1); }
    bool ring_holds(long long k) const { return ring_newest >= 0 && k >= ring_oldest() && k <= ring_newest; }
    int ring_levels(picles_ctx *c, double t, double dt, long long n_steps, const char *who) const;      /* are the levels of the next steps' windows held? */
    int ring_seed_levels(picles_ctx *c, double t) const;
    void ring_off() { ring = false; ring_slots = 0; ring_first = ring_newest = -1; }
    bool lattice_polyline_ahead(double t, double dt) const;      /* will the lattice's window over [t, t + dt] be a polyline? */
    /* does the window start where the pending step started, with (u1, v1) holding the lattice at the clock: can prepare() follow it? */
    bool contiguous_with(double pend_t, double clock) const { return held && held_t == clock && t0 == pend_t && !static_(); }
    bool middle(const Arrays &A, const double *&u, const double *&v) const { u = A.um; v = A.vm; return u != nullptr; }
    /* the level planes the window holds at time t, as they stand — nothing is interpolated (picles_flux_*): a static
     * window's only level; level 0 at the window's start; (u1, v1) at its end (whatever lies between: a knot or polyline window keeps
     * its end level there too) — for a lattice at the time they hold it, and only while they are known to (invalidate()) */
    bool level_at(const Arrays &A, double t, const double *&u, const double *&v) const
    {
        const bool ok = !lattice || held;
        if (ok && (static_() || t == t0)) { u = A.u0; v = A.v0; return true; }
        if (ok && t == (lattice ? held_t : t1)) { u = A.u1; v = A.v1; return true; }
        return false;
    }

    int make_pair(picles_ctx *c, double *&a, size_t a_bytes, double *&b, size_t b_bytes);
    int need(picles_ctx *c, const Shape &sh, bool prev = false);      /* the pairs a window of this shape reads (prev: and the fused remesh) */
    int set(picles_ctx *c, const Shape &sh, double t0_, double t1_, hipStream_t s) { shape = sh; t0 = t0_; t1 = t1_; return publish(c, s); }
    int publish(picles_ctx *c, hipStream_t s);
    int drop_middle(picles_ctx *c);
    /* the three plane movements */
    void reuse_swap(Arrays &A) { std::swap(A.u0, A.u1); std::swap(A.v0, A.v1); }      /* what (u1, v1) held becomes level 0 */
    void rotate(Arrays &A) { std::swap(A.uP, A.u0); std::swap(A.vP, A.v0); reuse_swap(A); }      /* uP <- u0 <- u1 <- the spare pair */
    void invalidate() { held = false; }            /* whatever (u1, v1) hold, the next lattice window samples both of its ends */
    /* the lattice as a source */
    int plan(picles_ctx *c, double t, double dt, Shape &sh) const;
    int sample(picles_ctx *c, const Shape &sh, double t, double dt, bool with0, hipStream_t s);
    int prepare(picles_ctx *c, double t, double dt, bool follow, hipStream_t s);
    /* the lattice's level at time t, sampled on stream s into the spare pair (made on first use): for a reader whose clock is at
     * none of the window's levels (level_at).  A wind stream that does not hold the level(s) bracketing t refuses, before anything is launched */
    int sample_spare(picles_ctx *c, double t, const char *who, hipStream_t s, const double *&u, const double *&v);
    void release(Arrays &A);                       /* idempotent; the caller has drained the streams that read the planes */
};

struct picles_ctx {
    picles_grid g;
    picles_phys ph;
    picles_ode od;
    picles_model md;
    KParams P;
    GridP G;
    Arrays A;
    int device;
    hipStream_t stream;
    hipEvent_t ev_edge;
    hipEvent_t ev_ctx = nullptr;        /* "everything enqueued on the context stream so far": caller streams wait for it */
    bool edge_pending = false;
    struct SlabRing *ring = nullptr;    /* native RCCL slab ring (picles_slab_*) */
    /* record buffer pair: rec_buf[cur] belongs to the step in flight / last completed advance */
    double *rec_buf[2] = {nullptr, nullptr};
    /* reach counters, rotating with the steps: the previous step's is read by the pull, the current one is written, the one two
     * steps ahead is cleared (five, not three: with the read one a step behind and the cleared one two ahead, three counters would
     * have a launch clear the one it reads, and four would have the NEXT step's launch clear it; with five no launch clears what a
     * launch of a neighbouring step reads or writes) */
    int *mr_buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int mr_w = 0;                                      /* index of the counter the step in flight writes.  Whoever rotates it counts cmap_hot down, and whoever
                                                        * launches k_step or k_advance clears the class map's rows ahead while it is positive (cmap_hot below) */
    int cur = 0;
    /* k_step_waverow (k_step.inc) for the fused launches whose geometry qualifies; PICLES_WAVEROW, read once at create:
     * 0 never; 1 (default) where it qualifies AND the flavour is the one whose speed has been measured against k_step on the hardware
     * (DP5 under static winds, the BASELINE launch: waverow_measured); 2 ("require") every flavour, and a fused step with a launch
     * that does not qualify is refused */
    int waverow_mode = 1;
    /* the tile class map (kernels.h: Arrays::rmap, class_map): PICLES_PULL_CLASS=0, read once at create, turns its reader and its writer
     * off.  cmap_hot: steps for which a buffer of the map may still hold an entry of a k_step_waverow launch (set to 4 by such a launch,
     * counted down by every step): while it is positive, the launches of k_step and k_advance — which keep their instruction streams and
     * clear nothing of this map themselves — have their rows' entries of the clear-ahead buffer zeroed from the host (class_map_clear_rows) */
    bool pull_class = true;
    int cmap_hot = 0;
    bool pending = false;                              /* fused stepping: the last advance's records still await their scatter + remesh */
    double pend_t = 0.0, pend_dt = 0.0;
    signed char *d_mask = nullptr;
    std::vector<signed char> h_mask;
    long long first_land = -1;          /* the first node of class 0 or 2 in h_mask (-1: an all-ocean box; picles_nest_relocate moves no other) */
    double clock = 0.0;
    /* pending step (begin_step .. scatter_remesh) */
    double step_dt = 0.0;
    int step_flags = 0;
    bool state_zero = false;      /* State known to be all zero (skip the accumulate read) */
    bool seeded = false;
    /* timing */
    bool timing = false;
    int timing_mode = 0;          /* 1: events around every launch; 2: one pair around each picles_run_steps call (its launches are
                                     back to back on one stream: region / launches = the mean launch, with no event between them) */
    bool in_region = false;       /* inside a mode-2 region: the per-launch events are skipped */
    int region_launches = 0;
    struct Ev { hipEvent_t a, b; int kind; };
    std::vector<Ev> ev_used, ev_free;
    picles_timing tim{};
    std::vector<float> tim_samples[3];   /* per-launch durations by kind (advance / scatter / remesh) */
    std::string err;
    /* the stream every device-to-host copy of the output paths rides on (store_stream_get: made on first use), and the three rings
     * (OutRing above): snapshots of State (run! stores), coarse diagnostics — a slot is the float32 planes followed by the tile
     * partials —, station probes — a slot is one sample, 3 planes of probe_n doubles */
    hipStream_t store_stream = nullptr;
    OutRing store, diag_ring, probe;
    DiagP diag{};
    int diag_nfields = 0, diag_npart = 0;
    size_t diag_field_bytes = 0, diag_part_off = 0, diag_slot_bytes = 0;
    double *diag_scratch = nullptr;                /* picles_diag_export without a partials buffer: where the kernel's partials go */
    /* coupling fluxes (picles_flux_*; k_flux.h): a ring like the diagnostics' — a slot is the float32 planes followed by the tile partials */
    OutRing flux_ring;
    FluxP flux{};
    int flux_nfields = 0, flux_npart = 0;
    size_t flux_field_bytes = 0, flux_part_off = 0, flux_slot_bytes = 0;
    double *flux_scratch = nullptr;                /* picles_flux_export without a partials buffer */
    /* flux means (picles_flux_mean_*; k_flux_mean.h): eleven fp64 accumulator planes of the flux set's coarse cells in one device
     * block, the host-side scalars, and the event behind the latest operation on the planes, as the statistics set keeps them */
    bool fm_on = false;
    Cadence fm_cad;                                /* steps: model steps completed since picles_flux_mean_init */
    long long fm_samples = 0;
    double fm_t_first = 0.0, fm_t_last = 0.0;
    double *fm_acc = nullptr;
    size_t fm_bytes = 0;
    hipEvent_t fm_ev = nullptr;
    hipStream_t fm_stream = nullptr;               /* the stream fm_ev was recorded on */
    bool fm_ev_live = false;
    int probe_n = 0;
    int *probe_nodes = nullptr;                    /* device: i plane, then the LOCAL row plane */
    Cadence probe_cad;                             /* steps: model steps completed since picles_probe_init */
    struct Track *trk = nullptr;                   /* track samples (picles_track_*; struct Track behind the station probes): nullptr without a set */
    /* run statistics (picles_stat_*): one device block of accumulator planes — the fp64 planes of the selected groups first (PEAK,
     * then MEAN), then the uint32 planes (n_wet, then n_exc[k]) —, the host-side scalars, and the event behind the latest
     * operation on the planes (update, reset, upload): operations on another stream wait for it, and so does picles_stat_get */
    bool stat_on = false;
    StatP stat{};
    Cadence stat_cad;                              /* steps: model steps completed since picles_stat_init */
    long long stat_samples = 0;
    double stat_t_first = 0.0, stat_t_last = 0.0;
    unsigned char *stat_dev = nullptr;
    size_t stat_bytes = 0;
    hipEvent_t stat_ev = nullptr;
    hipStream_t stat_stream = nullptr;             /* the stream stat_ev was recorded on */
    bool stat_ev_live = false;
    /* open-boundary forcing (picles_bforce_*): the forced nodes' local indices, and one device block of 6 planes of bf_n doubles —
     * level 0 (e, m_x, m_y), then level 1.  bf_levels: 0 none set yet, 1 constant, 2 a pair over [bf_t0, bf_t1] */
    int bf_n = 0;
    int *bf_nodes = nullptr;
    double *bf_lv = nullptr;
    int bf_levels = 0;
    double bf_t0 = 0.0, bf_t1 = 0.0;
    /* the planes bforce_launch hands k_bforce as level 0 and level 1: bf_lv and bf_lv + 3 bf_n for a set without a nest; with a nest
     * (picles_nest_*, struct Nest below the context) two of its three slots, rotated by pointer at every sample */
    double *bf_v0 = nullptr, *bf_v1 = nullptr;
    /* a band set (picles_bforce_init_band): the set's ocean nodes (mask class 1, local indices), whose PF_STEPPED is cleared in
     * A.pflags while the set lives (context_pflags), and the blend weights of a set that has one below 1 (nullptr: none) */
    std::vector<int> bf_ocean;
    double *bf_w = nullptr;
    /* nesting (picles_nest_*, picles_nest_feedback_*; struct Nest and struct Feedback below the forcing): a child owns `nest` (its
     * levels come from a parent) and, where it feeds its State back, `fb`; a parent names its children, and the one that feeds it */
    struct Nest *nest = nullptr;
    struct Feedback *fb = nullptr;
    std::vector<picles_ctx *> nest_children;
    picles_ctx *fb_child = nullptr;
    double *prolong_tab = nullptr; /* picles_nest_prolong: wx, wy, then ix0, ix1, iy0, iy1 of the latest call (a launch may still read them) */
    size_t prolong_cap = 0;        /* its size in bytes */
    WindWindow wind;              /* the wind window: host-set levels or the device-sampled lattice */
    bool ord_valid = false;        /* the previous fused step filed a dispatch order (kernels.h: Arrays::ord) with ... */
    int ord_nblk = 0;              /* ... this many workgroups: the whole grid, or the interior rows of a slab */
    bool ext_streams = false;      /* a caller-provided stream has been used: order across streams with device syncs */
    bool ring_orders = false;      /* inside picles_slab_run_steps: the ring orders its streams against the context stream with events */
    /* exact restart (picles_checkpoint_*): the device snapshot of the payload + its sum words, its pinned host copy */
    unsigned char *ck_dev = nullptr, *ck_host = nullptr;
    size_t ck_cap = 0;
    hipEvent_t ck_ready = nullptr, ck_done = nullptr;
    bool ck_inflight = false;
    unsigned char ck_hdr[256];                     /* header of the checkpoint in flight (CkptHeader), written by begin */
    int halo0 = 0;                                 /* halo_rows the context was created with (fingerprinted; the current ones are state) */
    uint64_t fp_metric = 0, fp_lattice = 0;        /* hashes of the metric planes / the wind lattice as the caller handed them over */
    /* generic scatter scratch */
    int *d_count = nullptr, *d_start = nullptr, *d_cursor = nullptr;
    void *d_scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
};

#define HIPCHK(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
            (void)hipGetLastError();   /* reported here: not left for the next launch check */ \
            return -10;                                                                        \
        }                                                                                      \
    } while (0)

/* an init that fails half-way leaves nothing behind: `undo` runs when the scope is left, unless the init got through and kept it */
template <class F> struct Undo {
    F undo;
    bool armed = true;
    ~Undo() { if (armed) undo(); }
};
template <class F> Undo(F) -> Undo<F>;

/* hipStreamQuery without side effects on the sticky last-error state (hipErrorNotReady is not a failure) */
static bool stream_idle(hipStream_t s)
{
    hipError_t e = hipStreamQuery(s);
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess;
}

static int fail(picles_ctx *c, int code, const std::string &m)
{
    c->err = m;
    return code;
}

static void timing_begin(picles_ctx *c, hipStream_t s, int kind)
{
    if (!c->timing) return;
    if (c->in_region) { if (kind == 0) c->region_launches++; return; }
    picles_ctx::Ev e;
    if (!c->ev_free.empty()) { e = c->ev_free.back(); c->ev_free.pop_back(); }
    else { hipEventCreate(&e.a); hipEventCreate(&e.b); }
    e.kind = kind;
    hipEventRecord(e.a, s);
    c->ev_used.push_back(e);
}
static void timing_end(picles_ctx *c, hipStream_t s)
{
    if (!c->timing || c->in_region) return;
    hipEventRecord(c->ev_used.back().b, s);
}
static void timing_collect(picles_ctx *c)
{
    for (auto &e : c->ev_used) {
        hipEventSynchronize(e.b);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e.a, e.b);
        if (e.kind >= 0 && e.kind < 3 && c->tim_samples[e.kind].size() < (1u << 20)) c->tim_samples[e.kind].push_back(ms);
        switch (e.kind) {
        case 3: c->tim.advance_ms += ms; break;      /* a mode-2 region: its launches were counted when they were enqueued */
        case 0: c->tim.advance_ms += ms; c->tim.advance_launches++; break;
        case 1: c->tim.scatter_ms += ms; c->tim.scatter_launches++; break;
        case 2: c->tim.remesh_ms += ms; c->tim.remesh_launches++; break;
        default: c->tim.other_ms += ms;
        }
        c->ev_free.push_back(e);
    }
    c->ev_used.clear();
}

static size_t rec_bytes(const picles_ctx *c) { return (size_t)(c->G.ny_loc + 2 * c->G.R) * 6 * c->G.Nx * sizeof(double); }

/* Arrays as a kernel sees them: which record buffer is read (scatter) / written (advance) */
static Arrays arrays_for(picles_ctx *c, int read_buf, int write_buf)
{
    Arrays A = c->A;
    A.rec = c->rec_buf[read_buf];
    A.rec_out = c->rec_buf[write_buf];
    /* reach counters rotate with the steps, independently of the record pair: a launch that scatters the records it has just
     * written (read_buf == write_buf: k_scatter after k_advance) reads the counter of the step in flight */
    A.mr_idx = (read_buf == write_buf ? c->mr_w : (c->mr_w + 4) % 5) | (c->mr_w << 4) | (((c->mr_w + 2) % 5) << 8) | (c->pull_class ? MR_CLASS_ON : 0);
    return A;
}

/* The invariant of the class map: a non-zero entry of the buffer a pull reads means that all 64 records of that tile, in the record
 * buffer it reads, carry that code.  Every entry point that writes a record buffer by other means than the step kernels — seed,
 * checkpoint load, the re-packing of picles_set_halo_rows, the particle setter — zeroes all five buffers (DESIGN.md §10 lists them). */
static int class_map_zero(picles_ctx *c)
{
    c->cmap_hot = 0;
    HIPCHK(c, hipMemsetAsync(c->A.rmap + (size_t)5 * c->A.ntile, 0, (size_t)5 * c->A.ntile * sizeof(int), c->stream));
    return 0;
}
/* the clear-ahead of a k_step or k_advance launch over rows [r0, r0 + n0) and [r1, r1 + n1): every tile the rows touch (a tile shared with a
 * neighbouring row belongs to a buffer that the whole step clears: nobody reads or writes it during this step) */
static int class_map_clear_rows(picles_ctx *c, hipStream_t s, int r0, int n0, int r1, int n1)
{
    int *const cm = c->A.rmap + (size_t)(5 + (c->mr_w + 2) % 5) * c->A.ntile;
    const int rr[2] = {r0, r1}, nn[2] = {n0, n1};
    for (int k = 0; k < 2; k++) {
        if (nn[k] <= 0) continue;
        const long long a = ((long long)rr[k] * c->G.Nx) >> 6, b = ((long long)(rr[k] + nn[k]) * c->G.Nx + 63) >> 6;
        const long long hi = b < (long long)c->A.ntile ? b : (long long)c->A.ntile;
        if (hi > a) HIPCHK(c, hipMemsetAsync(cm + a, 0, (size_t)(hi - a) * sizeof(int), s));
    }
    return 0;
}

static int launch_scatter(picles_ctx *c, hipStream_t s, bool remesh);

/* station probes (defined behind the diagnostics ring) */
static int probe_room(picles_ctx *c, long long n_steps, const char *who);
static int probe_take(picles_ctx *c, hipStream_t s);
static void probe_release(picles_ctx *c);
/* track samples (defined behind the station probes) */
static int track_step_ok(picles_ctx *c, double dt, const char *who);
static int track_take(picles_ctx *c, hipStream_t s);
static void track_release(picles_ctx *c);
/* run statistics (defined behind the station probes) */
static int stat_update(picles_ctx *c, hipStream_t s);
static void stat_release(picles_ctx *c);
/* flux means (defined behind the run statistics) */
static int flux_mean_update(picles_ctx *c, hipStream_t s, const char *who);
static void flux_mean_release(picles_ctx *c);
/* open-boundary forcing (defined behind the run statistics) */
static void bforce_release(picles_ctx *c);

/* the particle flags of a context without a forcing set, from the node classes and the model alone:
 * ocean_points (WaveGrowthModels2D.jl:256-270) and check_boundary_point (core_2D.jl:360-366) */
static std::vector<unsigned char> home_pflags(const std::vector<signed char> &mask, bool periodic_boundary)
{
    std::vector<unsigned char> pf(mask.size(), 0);
    for (size_t k = 0; k < mask.size(); k++) {
        const signed char mk = mask[k];
        unsigned char f = 0;
        if (mk == 1) f |= PF_STEPPED;
        if (mk == 3 && periodic_boundary) f |= PF_STEPPED | PF_GROUP2;
        const bool bnd = periodic_boundary ? (mk == 2) : (mk >= 2);
        if (bnd) f |= PF_BOUNDARY;
        pf[k] = f;
    }
    return pf;
}

/* A.pflags as this context must hold it: the home flags with the live band set, if any, applied — its ocean nodes are not stepped.
 * Formed from the host's own truth, never from the device plane; on the context stream, complete on return */
static int context_pflags(picles_ctx *c)
{
    std::vector<unsigned char> pf = home_pflags(c->h_mask, c->md.periodic_boundary != 0);
    for (int t : c->bf_ocean) pf[(size_t)t] &= (unsigned char)~PF_STEPPED;
    HIPCHK(c, hipMemcpyAsync(c->A.pflags, pf.data(), pf.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      /* pf dies here */
    return 0;
}
/* nesting, both directions (defined behind the open-boundary forcing) */
static int nest_levels_wait(picles_ctx *c, hipStream_t s);
static int nest_levels_read(picles_ctx *c, hipStream_t s, const double *read);
static int nest_leave_set(picles_ctx *c);
static void nest_leave_context(picles_ctx *c);

/* a model step has completed: the clock and the step counts the sampling schedules are counted in */
static void step_completed(picles_ctx *c)
{
    c->clock += c->step_dt;
    c->probe_cad.steps++;
    c->stat_cad.steps++;
    c->fm_cad.steps++;
}

/* scatter + remesh of the last fused step, if still outstanding */
static int flush(picles_ctx *c)
{
    if (!c->pending) return 0;
    HIPCHK(c, hipDeviceSynchronize());   /* the fused launches may have run on caller-provided streams */
    c->pending = false;                  /* only now: a failed synchronisation leaves the step pending */
    double clock_save = c->clock, dt_save = c->step_dt;
    int flags_save = c->step_flags;
    c->clock = c->pend_t;           /* remesh samples the wind at the start-of-step clock */
    c->step_dt = c->pend_dt;
    c->step_flags = PICLES_STEP_ZERO_FIRST;
    int rc = launch_scatter(c, c->stream, true);
    c->clock = clock_save; c->step_dt = dt_save; c->step_flags = flags_save;
    return rc;
}

PX_EXPORT int32_t picles_abi_version(void) { return PICLES_ABI_VERSION; }

PX_EXPORT const char *picles_last_error(const picles_ctx *ctx)
{
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

PX_EXPORT int32_t picles_destroy(picles_ctx *c);
PX_EXPORT int32_t picles_slab_comm_destroy(picles_ctx *c);

PX_EXPORT int32_t picles_create(const picles_grid *g, const picles_phys *p, const picles_ode *o,
                                const picles_model *m, int32_t device_id, int32_t halo_rows, picles_ctx **out)
{
    if (!g || !p || !o || !m || !out) { g_create_error = "null argument"; return -1; }
    *out = nullptr;
    if (g->Nx < 2 || g->Ny < 2) { g_create_error = "grid must be at least 2x2"; return -2; }
    if (g->j_begin < 0 || g->j_end > g->Ny || g->j_end <= g->j_begin) { g_create_error = "bad slab rows [j_begin,j_end)"; return -2; }
    if (o->solver < 0 || o->solver > 2) { g_create_error = "solver must be 0 (DP5), 1 (Tsit5) or 2 (AutoTsit5(Rosenbrock23()))"; return -3; }
    if (halo_rows < 1) halo_rows = 1;
    if (halo_rows > 1024) { g_create_error = "halo_rows must be <= 1024"; return -2; }
    if (!(o->abstol > 0.0) || !(o->reltol >= 0.0) || !(o->maxiters > 0) || !(o->dtmin >= 0.0)) {
        g_create_error = "ODE settings: abstol > 0, reltol >= 0, maxiters > 0, dtmin >= 0 required";
        return -3;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = "no HIP device available (this library has no CPU path)";
        return -4;
    }
    if (device_id < 0 || device_id >= ndev) { g_create_error = "device_id out of range"; return -4; }
    if ((e = hipSetDevice(device_id)) != hipSuccess) { g_create_error = hipGetErrorString(e); return -4; }

    picles_ctx *c = new picles_ctx();
    if (const char *wr = getenv("PICLES_WAVEROW")) c->waverow_mode = !strcmp(wr, "0") ? 0 : (!strcmp(wr, "require") ? 2 : 1);
    if (const char *pc = getenv("PICLES_PULL_CLASS")) c->pull_class = strcmp(pc, "0") != 0;
    memset(&c->A, 0, sizeof(c->A));
    c->stream = nullptr;
    c->ev_edge = nullptr;
    c->g = *g; c->ph = *p; c->od = *o; c->md = *m;
    c->device = device_id;
    /* derived constants: magic_fractions :87-92, e_T_func :271 (same primitives as the kernels) */
    KParams &P = c->P;
    P.r_g = p->r_g; P.inv_rg = 1.0 / p->r_g; P.C_alpha = p->C_alpha; P.C_phi = p->C_phi; P.C_e = p->C_e;
    double q = p->q;
    P.p = (-1.0 - 10.0 * q) / 2.0;
    P.n = 2.0 * q / (P.p + 4.0 * q);
    P.neg2p = -2.0 * P.p;
    double e_T = std::sqrt(p->c_e * pm_pow(p->c_alpha, -P.p / q) / pm_pow(p->gamma * p->c_beta * p->c_D, 1.0 / P.n));
    P.inv_eT = 1.0 / e_T;
    P.inv_eT4 = (P.inv_eT * P.inv_eT) * (P.inv_eT * P.inv_eT);
    P.half_inv_rg = 0.5 * P.inv_rg;
    P.two_inv_rg2 = 2.0 * (P.inv_rg * P.inv_rg);
    {
        const double k1 = 0.25 * PK_G0, k2 = k1 * k1, K = k2 * k2;      /* k_p⁴ = K (1/c_gp)⁸ */
        P.KeT4 = K * P.inv_eT4;
        P.KrCa = (K * P.r_g) * P.C_alpha;
        P.Cdir = P.C_phi * P.two_inv_rg2;
        /* the y = 1/|c̄| form of the RHS (physics.h rhs3): the powers of r_g in the constants */
        P.rg2 = P.r_g * P.r_g;
        const double rg4 = P.rg2 * P.rg2, rg8 = rg4 * rg4;
        P.Cw = (0.5 * PK_G0) * P.r_g;
        P.Chrh = -0.25 * P.r_g;
        P.ymax = 10.0 / P.r_g;
        P.sgmax = 1e8 / P.rg2;
        P.KeT4y = P.KeT4 * rg8;
        P.KrCay = P.KrCa * rg8;
        P.Cs = (0.5 * P.C_phi) * P.rg2;
        P.Cdir2 = 2.0 * P.C_phi;
        P.g4rg2 = k1 * P.rg2;
        P.qU2r_max = 249999.0 / (P.ymax * P.ymax);
    }
    P.inv_dx = 1.0 / g->dx; P.inv_dy = 1.0 / g->dy;
    P.deadband2 = p->dir_deadband * p->dir_deadband;
    P.propagation = p->propagation; P.input = p->input; P.dissipation = p->dissipation;
    P.peak_shift = p->peak_shift; P.direction = p->direction; P.n_is_2 = (P.n == 2.0);
    P.p_is_075 = (P.p == 0.75);
    P.fast_phys = P.propagation && P.input && P.dissipation && P.peak_shift && P.direction && P.n_is_2 && P.p_is_075 && P.deadband2 == 0.0;
    P.abstol = o->abstol; P.reltol = o->reltol; P.dt0 = o->dt0; P.dtmin = o->dtmin;
    P.inv_abstol = 1.0 / o->abstol;
    P.maxiters = o->maxiters; P.force_dtmin = o->force_dtmin;
    P.solver = o->solver;
    P.lne_max = o->log_energy_maximum; P.wind_min_sq = o->wind_min_squared;
    P.init_type = m->init_type;
    P.def_lne = m->default_particle[0]; P.def_cx = m->default_particle[1]; P.def_cy = m->default_particle[2];
    P.min_e = m->minimal_state[0]; P.min_m2 = m->minimal_state[1];
    (void)c->wind.publish(c, nullptr);      /* a static window at t = 0 (nothing is launched for one) */

    GridP &G = c->G;
    G.Nx = g->Nx; G.Ny = g->Ny; G.periodic_x = (g->periodic_x != 0); G.periodic_y = (g->periodic_y == 1);
    G.tripolar = (g->periodic_y == 2);
    if (g->periodic_y < 0 || g->periodic_y > 2 || (G.tripolar && !G.periodic_x)) {
        g_create_error = "periodic_y must be 0, 1 or 2 (tripolar north, which needs a periodic x axis)";
        delete c;
        return -2;
    }
    G.j_begin = g->j_begin; G.ny_loc = g->j_end - g->j_begin;
    G.single_slab = (g->j_begin == 0 && g->j_end == g->Ny);
    G.R = halo_rows;
    c->halo0 = halo_rows;
    G.Rp = G.single_slab ? 0 : halo_rows;
    G.ngroups = 1;

    /* total mask (mask_utils.jl:38-55) for the local rows */
    long long n = (long long)G.Nx * G.ny_loc;
    c->h_mask.resize(n);
    for (int jl = 0; jl < G.ny_loc; jl++)
        for (int i = 0; i < G.Nx; i++) {
            int j = jl + G.j_begin;
            signed char mk;
            if (g->mask) mk = g->mask[(long long)j * G.Nx + i];
            else {
                bool ring = (!g->periodic_x && (i == 0 || i == G.Nx - 1)) || (!g->periodic_y && (j == 0 || j == G.Ny - 1));
                mk = ring ? 3 : 1;
            }
            c->h_mask[(long long)jl * G.Nx + i] = mk;
            if ((mk == 0 || mk == 2) && c->first_land < 0) c->first_land = (long long)jl * G.Nx + i;
        }
    /* ocean_points (WaveGrowthModels2D.jl:256-270) and check_boundary_point (core_2D.jl:360-366) */
    bool any3 = false;
    if (g->mask) { for (long long k = 0; k < (long long)G.Nx * G.Ny; k++) if (g->mask[k] == 3) { any3 = true; break; } }
    else any3 = (!g->periodic_x || !g->periodic_y);
    const std::vector<unsigned char> pf = home_pflags(c->h_mask, m->periodic_boundary != 0);
    if (any3 && m->periodic_boundary) G.ngroups = 2;
    if ((long long)(G.ny_loc + 2 * G.R) * 6 * G.Nx >= (1LL << 31)) {
        g_create_error = "slab too large for 32-bit record offsets ((ny_loc + 2 halo_rows) * 6 * Nx must be < 2^31): use more slabs";
        delete c;
        return -2;
    }
    /* a whole-grid context follows any reach (a reach that wraps around a periodic axis takes the general
     * pull); a slab covers halo_rows of reach, and its periodic y axis must be longer than 2*halo_rows */
    if (!G.single_slab && ((G.periodic_y && G.Ny <= 2 * G.R) || G.ny_loc < G.R)) {
        g_create_error = "slab: periodic y axis not longer than 2*halo_rows, or fewer own rows than halo_rows";
        delete c;
        return -2;
    }

#define CK(call) do { hipError_t e2 = (call); if (e2 != hipSuccess) { g_create_error = std::string(#call) + ": " + hipGetErrorString(e2); picles_destroy(c); return -10; } } while (0)
    CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    CK(hipEventCreateWithFlags(&c->ev_edge, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&c->ev_ctx, hipEventDisableTiming));
    Arrays &A = c->A;
    memset(&A, 0, sizeof(A));
    A.n = n;
    CK(hipMalloc(&A.state, 3 * n * 8)); CK(hipMalloc(&A.movie, 3 * n * 8));
    CK(hipMalloc(&A.z, 5 * n * 8));
    CK(hipMalloc(&A.qold, n * 8)); CK(hipMalloc(&A.dtn, n * 8)); CK(hipMalloc(&A.asw, n * 4)); CK(hipMemset(A.asw, 0, n * 4));
    CK(hipMalloc(&A.on, n)); CK(hipMalloc(&A.pflags, n)); CK(hipMalloc(&A.status, n * 4));
    CK(hipMalloc(&A.u0, n * 8)); CK(hipMalloc(&A.v0, n * 8)); CK(hipMalloc(&A.u1, n * 8)); CK(hipMalloc(&A.v1, n * 8));
    CK(hipMalloc(&A.cnt, NSLOTS * sizeof(DevCounters) + 16 * sizeof(int)));     /* + the reach counters (kernels.h: reach_counters) */
    for (int k = 0; k < 5; k++) c->mr_buf[k] = (int *)(A.cnt + NSLOTS) + k;     /* five rotating reach counters; [5] = the running maximum */
    CK(hipMemset(c->mr_buf[0], 0, 16 * sizeof(int)));
    for (int k = 0; k < 2; k++) {
        CK(hipMalloc(&c->rec_buf[k], rec_bytes(c)));
        CK(hipMemset(c->rec_buf[k], 0, rec_bytes(c)));
    }
    A.nblk = (int)((n + 255) / 256);
    A.ord_on = 0;
    A.ord = nullptr;
    CK(hipMalloc(&A.ord, (size_t)5 * (2 + A.nblk) * sizeof(int)));      /* (a slab orders the launch over its interior rows: fewer workgroups) */
    CK(hipMemset(A.ord, 0, (size_t)5 * (2 + A.nblk) * sizeof(int)));
    A.ntile = (int)((n + 63) / 64);
    CK(hipMalloc(&A.rmap, (size_t)10 * A.ntile * sizeof(int)));     /* local reach map, five rotating buffers, and the tile class map behind it, five more (kernels.h: Arrays::rmap) */
    CK(hipMemset(A.rmap, 0, (size_t)10 * A.ntile * sizeof(int)));
    CK(hipMalloc(&c->d_mask, n));
    CK(hipMemset(A.state, 0, 3 * n * 8)); CK(hipMemset(A.movie, 0, 3 * n * 8)); CK(hipMemset(A.z, 0, 5 * n * 8));
    CK(hipMemset(A.qold, 0, n * 8)); CK(hipMemset(A.dtn, 0, n * 8)); CK(hipMemset(A.on, 0, n)); CK(hipMemset(A.status, 0, n * 4));
    CK(hipMemset(A.u0, 0, n * 8)); CK(hipMemset(A.v0, 0, n * 8)); CK(hipMemset(A.u1, 0, n * 8)); CK(hipMemset(A.v1, 0, n * 8));
    CK(hipMemset(A.cnt, 0, NSLOTS * sizeof(DevCounters)));
    CK(hipMemcpy(A.pflags, pf.data(), n, hipMemcpyHostToDevice));
    CK(hipMemcpy(c->d_mask, c->h_mask.data(), n, hipMemcpyHostToDevice));
#undef CK
    c->state_zero = true;
    *out = c;
    return 0;
}

PX_EXPORT int32_t picles_destroy(picles_ctx *c)
{
    if (!c) return 0;
    hipSetDevice(c->device);
    if (c->ring) picles_slab_comm_destroy(c);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->store_stream) hipStreamSynchronize(c->store_stream);     /* a checkpoint's copy-out may still be on PCIe */
    nest_leave_context(c);      /* nests and feedback, as a parent and as a child */
    Arrays &A = c->A;
    hipFree(A.state); hipFree(A.movie); hipFree(A.z); hipFree(A.qold); hipFree(A.dtn); hipFree(A.asw); hipFree(A.on);
    hipFree(A.pflags); hipFree(A.status); hipFree(A.u0); hipFree(A.v0); hipFree(A.u1); hipFree(A.v1);
    c->wind.release(A);
    hipFree(A.cnt); hipFree(A.rmap); hipFree(c->d_mask);
    if (A.ord) hipFree(A.ord);
    if (A.m11) { hipFree(A.m11); hipFree(A.m22); hipFree(A.pc); }
    for (int k = 0; k < 2; k++) hipFree(c->rec_buf[k]);

    c->store.release();
    c->diag_ring.release();
    if (c->diag_scratch) hipFree(c->diag_scratch);
    if (c->fm_on) hipDeviceSynchronize();       /* updates issued on caller streams read and write the planes about to go */
    flux_mean_release(c);
    c->flux_ring.release();
    if (c->flux_scratch) hipFree(c->flux_scratch);
    probe_release(c);
    if (c->trk) hipDeviceSynchronize();         /* samples issued on caller streams write the table about to go */
    track_release(c);
    if (c->stat_on) hipDeviceSynchronize();     /* updates issued on caller streams read and write the planes about to go */
    stat_release(c);
    bforce_release(c);
    if (c->prolong_tab) hipFree(c->prolong_tab);
    if (c->ck_dev) hipFree(c->ck_dev);
    if (c->ck_host) hipHostFree(c->ck_host);
    if (c->ck_ready) hipEventDestroy(c->ck_ready);
    if (c->ck_done) hipEventDestroy(c->ck_done);
    if (c->store_stream) hipStreamDestroy(c->store_stream);
    if (c->d_count) hipFree(c->d_count);
    if (c->d_start) hipFree(c->d_start);
    if (c->d_cursor) hipFree(c->d_cursor);
    if (c->d_scan_tmp) hipFree(c->d_scan_tmp);
    for (auto &e : c->ev_used) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    for (auto &e : c->ev_free) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    if (c->ev_edge) hipEventDestroy(c->ev_edge);
    if (c->ev_ctx) hipEventDestroy(c->ev_ctx);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

PX_EXPORT int32_t picles_sync(picles_ctx *c)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    HIPCHK(c, hipDeviceSynchronize());
    return 0;
}

PX_EXPORT double picles_clock(const picles_ctx *c) { return c ? c->clock : 0.0; }

static inline unsigned nblocks(long long n, int b) { return (unsigned)((n + b - 1) / b); }

/* ---- the wind window (struct WindWindow, above the context) ---- */
/* a pair of device blocks, both or neither: a failed second allocation frees the first and leaves a and b as they were */
int WindWindow::make_pair(picles_ctx *c, double *&a, size_t a_bytes, double *&b, size_t b_bytes)
{
    double *pa = nullptr, *pb = nullptr;
    Undo undo{[&] { hipFree(pa); }};
    HIPCHK(c, hipMalloc(&pa, a_bytes));
    HIPCHK(c, hipMalloc(&pb, b_bytes));
    undo.armed = false;
    a = pa; b = pb;
    return 0;
}
int WindWindow::need(picles_ctx *c, const Shape &sh, bool prev)
{
    const size_t n = (size_t)c->A.n, plane = n * 8;
    int rc = 0;
    if (prev && !c->A.uP) rc = make_pair(c, c->A.uP, plane, c->A.vP, plane);
    if (!rc && (sh.form == PARABOLA || sh.form == KNOT) && !um_buf) rc = make_pair(c, um_buf, plane, vm_buf, plane);
    if (rc || sh.form != POLYLINE || sh.nk <= poly_cap) return rc;
    /* a longer polyline than the buffers hold.  The smaller pair goes first (both would not fit side by side on a large grid); a polyline
     * on the device falls back to the straight line between its ends, which reads neither buffer */
    if (polyline() && (rc = drop_middle(c))) return rc;
    if (lv_buf) { hipFree(lv_buf); hipFree(xb_buf); }
    lv_buf = xb_buf = nullptr;
    poly_cap = 0;
    rc = make_pair(c, lv_buf, (size_t)2 * sh.nk * plane, xb_buf, ((size_t)PICLES_MAX_KNOTS + (size_t)2 * (sh.nk + 1) * n) * 8);
    if (rc == 0) poly_cap = sh.nk;
    return rc;
}

/* Hand the window to the kernels.  A polyline has the levels at its knots in lv_buf, levels 0 and nk + 1 in the (u0, v0) / (u1, v1)
 * planes, and its coefficient planes laid down on `s`; (um, vm) = the first knot's level and the one-knot scalars describe the first
 * knot: whatever evaluates the window at its START without knowing about polylines — the fused step's remesh reads level 0 from its
 * plane — still gets level 0.  wind_xb / wind_xn keep what the last polyline left there: nothing reads them while wind_nk < 2. */
int WindWindow::publish(picles_ctx *c, hipStream_t s)
{
    KParams &P = c->P;
    Arrays &A = c->A;
    const Form f = shape.form;
    const bool knot = f == KNOT || f == POLYLINE, three = f == PARABOLA || f == KNOT;
    const int nk = shape.nk;
    const double *tk = shape.tk;
    P.wind_static = static_() ? 1 : 0;
    P.tw0 = t0;
    P.inv_dtw = static_() ? 0.0 : 1.0 / (t1 - t0);
    P.wind_sk = knot ? (tk[0] - t0) * P.inv_dtw : 0.0;
    P.wind_isk = knot ? 1.0 / P.wind_sk : 0.0;
    P.wind_i1sk = knot ? 1.0 / (1.0 - P.wind_sk) : 0.0;
    P.wind_nk = knot ? 1 : 0;
    A.um = three ? um_buf : nullptr;           /* no middle level: linear in t (bit for bit the two-level arithmetic) */
    A.vm = three ? vm_buf : nullptr;
    if (!polyline()) return 0;
    WindPolyForm F;
    F.nk = nk;
    double sprev = 0.0;
    for (int k = 0; k < PICLES_MAX_KNOTS; k++) F.sk[k] = 2.0;
    for (int k = 0; k <= nk; k++) {
        const double sn = (k < nk) ? (tk[k] - t0) * P.inv_dtw : 1.0;
        if (k < nk) F.sk[k] = sn;
        F.ilen[k] = 1.0 / (sn - sprev);
        sprev = sn;
    }
    for (int k = nk + 1; k <= PICLES_MAX_KNOTS; k++) F.ilen[k] = 0.0;
    hipLaunchKernelGGL(k_wind_poly, dim3(nblocks(A.n, 256)), dim3(256), 0, s, F, A.u0, A.v0, A.u1, A.v1, lv_buf, xb_buf, A.n);
    HIPCHK(c, hipGetLastError());
    A.um = lv_buf; A.vm = lv_buf + A.n;
    P.wind_nk = nk;
    P.wind_xb = xb_buf;
    P.wind_xn = A.n;
    return 0;
}
/* back to no middle level, no knot: what is left is static, or the straight line between the window's ends */
int WindWindow::drop_middle(picles_ctx *c)
{
    shape.form = static_() ? STATIC : TWO;
    shape.nk = 0;
    return publish(c, nullptr);
}
void WindWindow::release(Arrays &A)
{
    for (double **p : {&A.uP, &A.vP, &um_buf, &vm_buf, &lv_buf, &xb_buf, &d_wgu, &d_wgv, &sp_u, &sp_v}) { hipFree(*p); *p = nullptr; }
    poly_cap = 0;
    for (hipEvent_t *e : {&ring_in, &ring_out}) { if (*e) hipEventDestroy(*e); *e = nullptr; }
    ring_off();
}

static int set_wind_levels(picles_ctx *c, const double *u0, const double *v0, double t0,
                           const double *um, const double *vm, bool knot, double tk,
                           const double *u1, const double *v1, double t1)
{
    if (!c || !u0 || !v0) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    HIPCHK(c, hipDeviceSynchronize());   /* the previous step may still read the wind planes */
    const bool two = u1 && v1 && t1 != t0;
    const bool three = two && um && vm;
    WindWindow &W = c->wind;
    WindWindow::Shape sh;
    sh.form = !two ? WindWindow::STATIC : !three ? WindWindow::TWO : knot ? WindWindow::KNOT : WindWindow::PARABOLA;
    sh.nk = sh.form == WindWindow::KNOT ? 1 : 0;
    sh.tk[0] = tk;
    { int rc = W.need(c, sh); if (rc) return rc; }      /* (first: a call that fails here has changed nothing) */
    W.lattice = false;
    W.ring_off();
    Arrays &A = c->A;
    size_t b = (size_t)A.n * 8;
    HIPCHK(c, hipMemcpyAsync(A.u0, u0, b, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(A.v0, v0, b, hipMemcpyHostToDevice, c->stream));
    if (two) {
        HIPCHK(c, hipMemcpyAsync(A.u1, u1, b, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(A.v1, v1, b, hipMemcpyHostToDevice, c->stream));
    }
    if (three) {
        HIPCHK(c, hipMemcpyAsync(W.um_buf, um, b, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(W.vm_buf, vm, b, hipMemcpyHostToDevice, c->stream));
    }
    (void)W.set(c, sh, t0, t1, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));   /* caller may reuse its host buffers */
    return 0;
}

PX_EXPORT int32_t picles_set_winds3(picles_ctx *c, const double *u0, const double *v0, double t0,
                                    const double *um, const double *vm,
                                    const double *u1, const double *v1, double t1)
{
    return set_wind_levels(c, u0, v0, t0, um, vm, false, 0.0, u1, v1, t1);
}

PX_EXPORT int32_t picles_set_winds(picles_ctx *c, const double *u0, const double *v0, double t0,
                                   const double *u1, const double *v1, double t1)
{
    return set_wind_levels(c, u0, v0, t0, nullptr, nullptr, false, 0.0, u1, v1, t1);
}

PX_EXPORT int32_t picles_set_winds_knot(picles_ctx *c, const double *u0, const double *v0, double t0,
                                        const double *uk, const double *vk, double tk,
                                        const double *u1, const double *v1, double t1)
{
    if (!c) return -1;
    if (!uk || !vk || !u1 || !v1) return fail(c, -2, "picles_set_winds_knot needs all three levels");
    if (!(t0 < tk && tk < t1)) return fail(c, -2, "picles_set_winds_knot: the knot must lie strictly inside the window, t0 < tk < t1");
    return set_wind_levels(c, u0, v0, t0, uk, vk, true, tk, u1, v1, t1);
}

/* nlev >= 2 node-sampled levels at strictly increasing times: the piecewise-linear wind through them (a gridded wind sampled by the
 * host at every time knot inside the step and at its ends).  2 levels = picles_set_winds, 3 = picles_set_winds_knot; more: the
 * polyline window (at most PICLES_MAX_KNOTS levels between the ends). */
PX_EXPORT int32_t picles_set_winds_polyline(picles_ctx *c, int32_t nlev, const double *const *u, const double *const *v, const double *times)
{
    if (!c) return -1;
    if (nlev < 2 || !u || !v || !times) return fail(c, -2, "picles_set_winds_polyline needs at least two levels");
    for (int k = 0; k < nlev; k++) if (!u[k] || !v[k]) return fail(c, -2, "picles_set_winds_polyline: a level is missing");
    for (int k = 1; k < nlev; k++) if (!(times[k - 1] < times[k])) return fail(c, -2, "picles_set_winds_polyline: the level times must increase strictly");
    if (nlev == 2) return set_wind_levels(c, u[0], v[0], times[0], nullptr, nullptr, false, 0.0, u[1], v[1], times[1]);
    if (nlev == 3) return set_wind_levels(c, u[0], v[0], times[0], u[1], v[1], true, times[1], u[2], v[2], times[2]);
    const int nk = nlev - 2;
    if (nk > PICLES_MAX_KNOTS) {
        char buf[160];
        snprintf(buf, sizeof buf, "picles_set_winds_polyline: %d levels inside the window, at most %d are carried", nk, PICLES_MAX_KNOTS);
        return fail(c, -2, buf);
    }
    /* levels 0, 1 and the last through the three-level path (the one-knot form of the first knot), then the further knots */
    int rc = set_wind_levels(c, u[0], v[0], times[0], u[1], v[1], true, times[1], u[nlev - 1], v[nlev - 1], times[nlev - 1]);
    if (rc) return rc;
    WindWindow &W = c->wind;
    WindWindow::Shape sh;
    sh.form = WindWindow::POLYLINE;
    sh.nk = nk;
    for (int k = 0; k < nk; k++) sh.tk[k] = times[k + 1];
    if ((rc = W.need(c, sh))) return rc;
    const size_t b = (size_t)c->A.n * 8;
    for (int k = 0; k < nk; k++) {
        HIPCHK(c, hipMemcpyAsync(W.lv_buf + (size_t)(2 * k) * c->A.n, u[k + 1], b, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(W.lv_buf + (size_t)(2 * k + 1) * c->A.n, v[k + 1], b, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = W.set(c, sh, times[0], times[nlev - 1], c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   /* caller may reuse its host buffers */
    return 0;
}


/* per-node ProjetionKernel diagonal + PropagationCorrection coefficient */
PX_EXPORT int32_t picles_set_metric(picles_ctx *c, const double *m11, const double *m22, const double *pc)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    HIPCHK(c, hipDeviceSynchronize());
    Arrays &A = c->A;
    if (A.m11) { hipFree(A.m11); hipFree(A.m22); hipFree(A.pc); A.m11 = A.m22 = A.pc = nullptr; }
    c->fp_metric = 0;
    if (!m11 || !m22 || !pc) return 0;   /* back to the Cartesian constants */
    size_t b = (size_t)A.n * 8;
    c->fp_metric = fp_bytes(fp_bytes(fp_bytes(FP_SEED, m11, b), m22, b), pc, b);
    HIPCHK(c, hipMalloc(&A.m11, b)); HIPCHK(c, hipMalloc(&A.m22, b)); HIPCHK(c, hipMalloc(&A.pc, b));
    HIPCHK(c, hipMemcpy(A.m11, m11, b, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(A.m22, m22, b, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(A.pc, pc, b, hipMemcpyHostToDevice));
    return 0;
}

PX_EXPORT int32_t picles_set_wind_grid(picles_ctx *c, int32_t nx, int32_t ny, int32_t nt,
                                       double x0, double dx, double y0, double dy, double t0, double dt,
                                       const double *u, const double *v, double mesh_x0, double mesh_y0)
{
    if (!c || !u || !v) return -1;
    if (nx < 2 || ny < 2 || nt < 2 || !(dx > 0) || !(dy > 0) || !(dt > 0)) return fail(c, -2, "wind lattice needs >= 2 knots per axis and positive spacing");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    HIPCHK(c, hipDeviceSynchronize());
    WindWindow &W = c->wind;
    if (W.d_wgu) { hipFree(W.d_wgu); hipFree(W.d_wgv); W.d_wgu = W.d_wgv = nullptr; }
    W.lattice = false;                   /* (until the new one is up: a failed upload leaves the window on the device, not a freed lattice) */
    W.ring_off();
    size_t nb = (size_t)nx * ny * nt * 8;
    { int rc = W.make_pair(c, W.d_wgu, nb, W.d_wgv, nb); if (rc) return rc; }
    HIPCHK(c, hipMemcpy(W.d_wgu, u, nb, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(W.d_wgv, v, nb, hipMemcpyHostToDevice));
    c->fp_lattice = fp_bytes(fp_bytes(FP_SEED, u, nb), v, nb);
    WindGrid &w = W.wg;
    w.nx = nx; w.ny = ny; w.nt = nt;
    w.x0 = x0; w.inv_dx = 1.0 / dx; w.y0 = y0; w.inv_dy = 1.0 / dy; w.t0 = t0; w.inv_dt = 1.0 / dt;
    w.mesh_x0 = mesh_x0; w.mesh_y0 = mesh_y0; w.mesh_dx = c->g.dx; w.mesh_dy = c->g.dy;
    w.u = W.d_wgu; w.v = W.d_wgv;
    W.lat_t0 = t0; W.lat_dt = dt;
    (void)W.drop_middle(c);
    W.lattice = true;
    W.mode = PICLES_LATTICE_LINEAR;
    W.invalidate();
    return 0;
}

PX_EXPORT int32_t picles_set_wind_grid_mode(picles_ctx *c, int32_t mode)
{
    if (!c) return -1;
    if (mode != PICLES_LATTICE_LINEAR && mode != PICLES_LATTICE_SMOOTH3) return fail(c, -2, "unknown wind lattice mode");
    if (!c->wind.from_lattice()) return fail(c, -2, "picles_set_wind_grid first");
    { int rc = flush(c); if (rc) return rc; }
    c->wind.mode = mode;
    c->wind.invalidate();
    return 0;
}

/* time knots of the lattice strictly inside (t, t + dt): 0, 1 or 2 (= two or more); *tk = the first one.  Knots sit at whole
 * multiples of lat_dt from lat_t0 (the periodic continuation's period is a whole number of intervals); one closer to an end of the
 * window than 1e-9 intervals is that end (600-second steps against 900-second knots must not see a "knot" 1e-13 s before t + dt). */
PX_EXPORT int32_t picles_lattice_knots(double lat_t0, double lat_dt, double t, double dt, double *tk)
{
    const double eps = 1e-9;
    const double c0 = (t - lat_t0) / lat_dt, c1 = (t + dt - lat_t0) / lat_dt;
    const double k0 = __builtin_floor(c0 + eps) + 1.0;
    if (!(k0 < c1 - eps)) return 0;
    if (tk) *tk = lat_t0 + k0 * lat_dt;
    return (k0 + 1.0 < c1 - eps) ? 2 : 1;
}

/* all of them: the number of time knots strictly inside (t, t + dt) (same rule), the first `cap` of their times in tks */
PX_EXPORT int32_t picles_lattice_knot_times(double lat_t0, double lat_dt, double t, double dt, double *tks, int32_t cap)
{
    const double eps = 1e-9;
    const double c0 = (t - lat_t0) / lat_dt, c1 = (t + dt - lat_t0) / lat_dt;
    int n = 0;
    for (double k = __builtin_floor(c0 + eps) + 1.0; k < c1 - eps; k += 1.0) {
        if (tks && n < cap) tks[n] = lat_t0 + k * lat_dt;
        if (++n == 0x7fffffff) break;
    }
    return n;
}

bool WindWindow::lattice_polyline_ahead(double t, double dt) const
{
    return lattice && mode != PICLES_LATTICE_SMOOTH3 && picles_lattice_knot_times(lat_t0, lat_dt, t, dt, nullptr, 0) >= 2;
}
/* the shape of the step window [t, t + dt] over the lattice: smooth3, the parabola; linear, by the time knots strictly inside */
int WindWindow::plan(picles_ctx *c, double t, double dt, Shape &sh) const
{
    sh = Shape{};
    sh.form = PARABOLA;
    if (mode == PICLES_LATTICE_SMOOTH3) return 0;
    sh.nk = picles_lattice_knot_times(lat_t0, lat_dt, t, dt, sh.tk, PICLES_MAX_KNOTS);
    if (sh.nk > PICLES_MAX_KNOTS) {
        char buf[360];
        snprintf(buf, sizeof buf, "the model step [%.17g, %.17g] contains %d time knots of the wind lattice (spacing %.17g s); a window carries at most %d: "
                 "take shorter model steps, or picles_set_wind_grid_mode(PICLES_LATTICE_SMOOTH3) if the lattice tabulates a smooth closure",
                 t, t + dt, sh.nk, lat_dt, PICLES_MAX_KNOTS);
        return fail(c, -7, buf);
    }
    sh.form = sh.nk == 0 ? TWO : sh.nk == 1 ? KNOT : POLYLINE;
    return 0;
}

/* sample the levels of the window [t, t + dt] that are not on the device yet — level 0 into (u0, v0) when `with0`; then the middle
 * level (the knot, or t + dt/2) into (um, vm), or the levels at a polyline's knots into lv_buf, and level 1 at t + dt into (u1, v1),
 * two levels a launch — and publish the window.  The pairs the shape reads exist (need) */
int WindWindow::sample(picles_ctx *c, const Shape &sh, double t, double dt, bool with0, hipStream_t s)
{
    Arrays &A = c->A;
    dim3 grid(nblocks(A.n, 256)), block(256);
    const size_t n = (size_t)A.n;
    struct { double t; double *u, *v; } L[PICLES_MAX_KNOTS + 1];
    int m = 0;
    if (sh.form == PARABOLA || sh.form == KNOT) L[m++] = {sh.form == KNOT ? sh.tk[0] : t + 0.5 * dt, um_buf, vm_buf};
    for (int k = 0; sh.form == POLYLINE && k < sh.nk; k++) L[m++] = {sh.tk[k], lv_buf + (size_t)(2 * k) * n, lv_buf + (size_t)(2 * k + 1) * n};
    L[m++] = {t + dt, A.u1, A.v1};
    if (ring) {
        /* the same launches from the ring: (slots, f) per level by the time rule.  The entry points have checked that the levels are held */
        auto put = [&](WindRingOut &O, int q, double tq, double *u, double *v) {
            int64_t k = 0;
            double f = 0.0;
            (void)picles_wind_stream_coord(lat_t0, lat_dt, tq, &k, &f);
            O.s0[q] = (int)(k % ring_slots);
            O.s1[q] = f != 0.0 ? (int)((k + 1) % ring_slots) : O.s0[q];
            O.f[q] = f;
            O.u[q] = u; O.v[q] = v;
        };
        if (with0) {
            WindRingOut O{};
            put(O, 0, t, A.u0, A.v0);
            hipLaunchKernelGGL(k_wind_sample_ring<1>, grid, block, 0, s, c->G, wg, O, A.n);
        }
        for (int k = 0; k < m; k += 2) {
            WindRingOut O{};
            put(O, 0, L[k].t, L[k].u, L[k].v);
            if (k + 1 < m) {
                put(O, 1, L[k + 1].t, L[k + 1].u, L[k + 1].v);
                hipLaunchKernelGGL(k_wind_sample_ring<2>, grid, block, 0, s, c->G, wg, O, A.n);
            } else
                hipLaunchKernelGGL(k_wind_sample_ring<1>, grid, block, 0, s, c->G, wg, O, A.n);
        }
        HIPCHK(c, hipGetLastError());
        held_t = t + dt;
        held = true;
        return set(c, sh, t, t + dt, s);
    }
    if (with0) {
        WindSampleOut O = {{t, 0.0}, {A.u0, nullptr}, {A.v0, nullptr}};
        hipLaunchKernelGGL(k_wind_sample<1>, grid, block, 0, s, c->G, wg, O, A.n);
    }
    for (int k = 0; k < m; k += 2) {
        if (k + 1 < m) {
            WindSampleOut O = {{L[k].t, L[k + 1].t}, {L[k].u, L[k + 1].u}, {L[k].v, L[k + 1].v}};
            hipLaunchKernelGGL(k_wind_sample<2>, grid, block, 0, s, c->G, wg, O, A.n);
        } else {
            WindSampleOut O = {{L[k].t, 0.0}, {L[k].u, nullptr}, {L[k].v, nullptr}};
            hipLaunchKernelGGL(k_wind_sample<1>, grid, block, 0, s, c->G, wg, O, A.n);
        }
    }
    HIPCHK(c, hipGetLastError());
    held_t = t + dt;
    held = true;
    return set(c, sh, t, t + dt, s);
}

/* the window of the step [t, t + dt].  follow: behind a pending step whose window it is contiguous with — the planes rotate and only
 * the new level 1 is sampled; else the level the previous step left in (u1, v1), if it is this step's start, is reused as level 0 */
int WindWindow::prepare(picles_ctx *c, double t, double dt, bool follow, hipStream_t s)
{
    Shape sh;
    { int rc = plan(c, t, dt, sh); if (rc) return rc; }
    { int rc = need(c, sh, follow); if (rc) return rc; }      /* (before a plane moves: a call that fails here can be made again) */
    const bool reuse = !follow && held && held_t == t;
    if (follow) rotate(c->A);
    else if (reuse) reuse_swap(c->A);
    return sample(c, sh, t, dt, !follow && !reuse, s);
}

int WindWindow::sample_spare(picles_ctx *c, double t, const char *who, hipStream_t s, const double *&u, const double *&v)
{
    const size_t plane = (size_t)c->A.n * 8;
    dim3 grid(nblocks(c->A.n, 256)), block(256);
    if (ring) {
        int64_t k = 0;
        double f = 0.0;
        char b[400];
        if (picles_wind_stream_coord(lat_t0, lat_dt, t, &k, &f)) {
            snprintf(b, sizeof b, "%s: the clock %.17g lies before the first time level of the wind stream (t0 = %.17g)", who, t, lat_t0);
            return fail(c, -2, b);
        }
        for (long long q = k; q <= k + (f != 0.0 ? 1 : 0); q++)
            if (!ring_holds(q)) {
                snprintf(b, sizeof b, "%s: the wind at the clock %.17g needs level k = %lld (t = %.17g) of the wind stream, which is not held "
                                      "(levels held: %lld .. %lld): picles_wind_stream_push it first, or step to a level the window holds",
                         who, t, q, lat_t0 + (double)q * lat_dt, ring_oldest(), ring_newest);
                return fail(c, -2, b);
            }
        if (!sp_u) { int rc = make_pair(c, sp_u, plane, sp_v, plane); if (rc) return rc; }
        WindRingOut O{};
        O.s0[0] = (int)(k % ring_slots);
        O.s1[0] = f != 0.0 ? (int)((k + 1) % ring_slots) : O.s0[0];
        O.f[0] = f;
        O.u[0] = sp_u; O.v[0] = sp_v;
        hipLaunchKernelGGL(k_wind_sample_ring<1>, grid, block, 0, s, c->G, wg, O, c->A.n);
    } else {
        if (!sp_u) { int rc = make_pair(c, sp_u, plane, sp_v, plane); if (rc) return rc; }
        WindSampleOut O = {{t, 0.0}, {sp_u, nullptr}, {sp_v, nullptr}};
        hipLaunchKernelGGL(k_wind_sample<1>, grid, block, 0, s, c->G, wg, O, c->A.n);
    }
    HIPCHK(c, hipGetLastError());
    u = sp_u; v = sp_v;
    return 0;
}

/* ---- the wind stream (the contract: include/picles_hip.h, "streamed winds") ---- */
/* the time rule: host arithmetic only */
PX_EXPORT int32_t picles_wind_stream_coord(double t0, double dt, double t, int64_t *k, double *f)
{
    if (!(dt > 0.0)) return -2;
    const double inv_dt = 1.0 / dt;
    double cc = (t - t0) * inv_dt;               /* as k_wind_sample forms it */
    const double r = __builtin_rint(cc);
    if (__builtin_fabs(cc - r) <= 1e-9) cc = r;
    if (!(cc >= 0.0) || !(cc < 9.0e15)) return -2;
    const double fl = __builtin_floor(cc);
    if (k) *k = (int64_t)fl;
    if (f) *f = cc - fl;
    return 0;
}

/* every level the windows of the next n_steps steps of length dt from time t read — [floor(c(t)), ceil(c(t + dt))] of each — must be
 * held, and one window's levels must fit the ring together.  Asked before anything is enqueued (the style of bforce_window) */
int WindWindow::ring_levels(picles_ctx *c, double t, double dt, long long n_steps, const char *who) const
{
    if (!ring || n_steps <= 0 || !(dt > 0.0)) return 0;
    char b[512];
    for (long long s = 0; s < n_steps; s++, t += dt) {
        int64_t k0 = 0, k1 = 0;
        double f0 = 0.0, f1 = 0.0;
        if (picles_wind_stream_coord(lat_t0, lat_dt, t, &k0, &f0) || picles_wind_stream_coord(lat_t0, lat_dt, t + dt, &k1, &f1)) {
            snprintf(b, sizeof b, "%s: step %lld of this call, [%.17g, %.17g], starts before the first time level of the wind stream (t0 = %.17g): "
                                  "a stream has no periodic continuation in t", who, s + 1, t, t + dt, lat_t0);
            return fail(c, -2, b);
        }
        if (f1 != 0.0) k1++;
        if (k1 - k0 + 1 > ring_slots) {
            snprintf(b, sizeof b, "%s: step %lld of this call, [%.17g, %.17g], has %lld time knots of the wind stream (interval %.17g s) inside and reads "
                                  "%lld levels, the ring holds %d: a step with nk interior knots needs n_slots >= nk + 2 "
                                  "(picles_wind_stream_init with more slots, or shorter steps)",
                     who, s + 1, t, t + dt, (long long)(k1 - k0 - 1), lat_dt, (long long)(k1 - k0 + 1), ring_slots);
            return fail(c, -2, b);
        }
        for (long long k = k0; k <= k1; k++)
            if (!ring_holds(k)) {
                snprintf(b, sizeof b, "%s: step %lld of this call, [%.17g, %.17g], reads level k = %lld (t = %.17g) of the wind stream, which is not held "
                                      "(levels held: %lld .. %lld): picles_wind_stream_push it first, or take fewer steps per call",
                         who, s + 1, t, t + dt, k, lat_t0 + (double)k * lat_dt, ring_oldest(), ring_newest);
                return fail(c, -2, b);
            }
    }
    return 0;
}
/* picles_seed reads level 0 of its window alone: the level(s) bracketing time t */
int WindWindow::ring_seed_levels(picles_ctx *c, double t) const
{
    if (!ring) return 0;
    int64_t k = 0;
    double f = 0.0;
    char b[384];
    if (picles_wind_stream_coord(lat_t0, lat_dt, t, &k, &f)) {
        snprintf(b, sizeof b, "picles_seed: the seed reads the wind at t = %.17g, before the first time level of the wind stream (t0 = %.17g)", t, lat_t0);
        return fail(c, -2, b);
    }
    for (long long q = k; q <= k + (f != 0.0 ? 1 : 0); q++)
        if (!ring_holds(q)) {
            snprintf(b, sizeof b, "picles_seed: the seed reads the wind at t = %.17g: level k = %lld (t = %.17g) of the wind stream is not held "
                                  "(levels held: %lld .. %lld): picles_wind_stream_push it first",
                     t, q, lat_t0 + (double)q * lat_dt, ring_oldest(), ring_newest);
            return fail(c, -2, b);
        }
    return 0;
}

PX_EXPORT int32_t picles_wind_stream_init(picles_ctx *c, int32_t nx, int32_t ny, double x0, double dx, double y0, double dy,
                                          double t0, double dt, double mesh_x0, double mesh_y0, int32_t n_slots)
{
    if (!c) return -1;
    if (nx < 2 || ny < 2 || !(dx > 0) || !(dy > 0) || !(dt > 0)) return fail(c, -2, "picles_wind_stream_init: the lattice needs >= 2 knots per space axis and positive spacing");
    if (n_slots < 2 || n_slots > 4096) return fail(c, -2, "picles_wind_stream_init: n_slots must be 2 ... 4096 (two levels bracket a time)");
    if (!c->G.single_slab || c->ring || !(c->G.j_begin == 0 && c->G.ny_loc == c->G.Ny))
        return fail(c, -5, "picles_wind_stream_init: slabs, slab mode and the native ring do not carry a wind stream: a whole-grid context is needed");
    if (c->nest || !c->nest_children.empty())
        return fail(c, -5, "picles_wind_stream_init: the context is part of a nest: streamed nests are not carried (picles_nest_free first)");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    HIPCHK(c, hipDeviceSynchronize());
    WindWindow &W = c->wind;
    if (!W.ring_in) {
        HIPCHK(c, hipEventCreateWithFlags(&W.ring_in, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&W.ring_out, hipEventDisableTiming));
    }
    if (W.d_wgu) { hipFree(W.d_wgu); hipFree(W.d_wgv); W.d_wgu = W.d_wgv = nullptr; }
    W.lattice = false;                   /* (until the ring is up, as picles_set_wind_grid) */
    W.ring_off();
    const size_t nb = (size_t)nx * ny * n_slots * 8;
    { int rc = W.make_pair(c, W.d_wgu, nb, W.d_wgv, nb); if (rc) return rc; }
    HIPCHK(c, hipMemsetAsync(W.d_wgu, 0, nb, c->stream));
    HIPCHK(c, hipMemsetAsync(W.d_wgv, 0, nb, c->stream));
    c->fp_lattice = 0;
    WindGrid &w = W.wg;
    w.nx = nx; w.ny = ny; w.nt = n_slots;
    w.x0 = x0; w.inv_dx = 1.0 / dx; w.y0 = y0; w.inv_dy = 1.0 / dy; w.t0 = t0; w.inv_dt = 1.0 / dt;
    w.mesh_x0 = mesh_x0; w.mesh_y0 = mesh_y0; w.mesh_dx = c->g.dx; w.mesh_dy = c->g.dy;
    w.u = W.d_wgu; w.v = W.d_wgv;
    W.lat_t0 = t0; W.lat_dt = dt;
    (void)W.drop_middle(c);
    W.lattice = true;
    W.ring = true;
    W.ring_slots = n_slots;
    W.ring_pushes = 0;
    W.mode = PICLES_LATTICE_LINEAR;
    W.invalidate();
    return 0;
}

PX_EXPORT int32_t picles_wind_stream_push(picles_ctx *c, int64_t k, const void *u, const void *v, int32_t dtype, int32_t where, void *caller_stream)
{
    if (!c) return -1;
    WindWindow &W = c->wind;
    if (!W.streamed()) return fail(c, -2, "picles_wind_stream_push: picles_wind_stream_init first");
    if (!u || !v) return fail(c, -2, "picles_wind_stream_push: both planes are needed");
    if ((dtype != PICLES_WIND_F64 && dtype != PICLES_WIND_F32) || (where != PICLES_WIND_HOST && where != PICLES_WIND_DEVICE))
        return fail(c, -2, "picles_wind_stream_push: dtype must be PICLES_WIND_F64 or _F32, where PICLES_WIND_HOST or _DEVICE");
    char b[384];
    if (k < 0 || (W.ring_newest >= 0 && k != W.ring_newest + 1)) {
        snprintf(b, sizeof b, "picles_wind_stream_push: level k = %lld is out of order: the levels arrive one at a time, the next one is k = %lld "
                              "(a level already held is not pushed again; picles_wind_stream_reset starts over)",
                 (long long)k, W.ring_newest >= 0 ? W.ring_newest + 1 : 0LL);
        return fail(c, -2, b);
    }
    int64_t kc = 0;
    double fc = 0.0;
    if (picles_wind_stream_coord(W.lat_t0, W.lat_dt, c->clock, &kc, &fc) == 0 && W.ring_holds(k - W.ring_slots) && k - W.ring_slots >= kc) {
        snprintf(b, sizeof b, "picles_wind_stream_push: level k = %lld goes to the slot of level %lld, which the interval of the clock (t = %.17g, "
                              "levels %lld and up) still needs: step the model first, or picles_wind_stream_init with more than %d slots",
                 (long long)k, (long long)(k - W.ring_slots), c->clock, (long long)kc, W.ring_slots);
        return fail(c, -2, b);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)W.wg.nx * W.wg.ny;
    double *du = W.d_wgu + (size_t)(k % W.ring_slots) * n, *dv = W.d_wgv + (size_t)(k % W.ring_slots) * n;
    hipStream_t cs = (hipStream_t)caller_stream;
    if (where == PICLES_WIND_DEVICE) {
        if (cs) {      /* what the caller enqueued so far produces the planes */
            HIPCHK(c, hipEventRecord(W.ring_in, cs));
            HIPCHK(c, hipStreamWaitEvent(c->stream, W.ring_in, 0));
        }
        if (dtype == PICLES_WIND_F64) {
            HIPCHK(c, hipMemcpyAsync(du, u, n * 8, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(dv, v, n * 8, hipMemcpyDeviceToDevice, c->stream));
        } else {
            hipLaunchKernelGGL(k_wind_ingest, dim3(nblocks((long long)n, 256)), dim3(256), 0, c->stream, (const float *)u, (const float *)v, du, dv, (long long)n);
            HIPCHK(c, hipGetLastError());
        }
        if (cs) {      /* the caller may overwrite its planes in stream order */
            HIPCHK(c, hipEventRecord(W.ring_out, c->stream));
            HIPCHK(c, hipStreamWaitEvent(cs, W.ring_out, 0));
        }
    } else {
        std::vector<double> wide;
        const double *hu = (const double *)u, *hv = (const double *)v;
        if (dtype == PICLES_WIND_F32) {
            wide.resize(2 * n);
            for (size_t q = 0; q < n; q++) { wide[q] = (double)((const float *)u)[q]; wide[n + q] = (double)((const float *)v)[q]; }
            hu = wide.data(); hv = wide.data() + n;
        }
        HIPCHK(c, hipMemcpyAsync(du, hu, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dv, hv, n * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));      /* complete on return: the caller may reuse its host buffers */
    }
    if (W.ring_newest < 0) W.ring_first = k;
    W.ring_newest = k;
    W.ring_pushes++;
    return 0;
}

PX_EXPORT int32_t picles_wind_stream_info(const picles_ctx *c, int32_t *n_slots, int64_t *oldest, int64_t *newest, int64_t *pushes)
{
    if (!c || !c->wind.streamed()) return -1;
    const WindWindow &W = c->wind;
    if (n_slots) *n_slots = W.ring_slots;
    if (oldest) *oldest = W.ring_oldest();
    if (newest) *newest = W.ring_newest;
    if (pushes) *pushes = W.ring_pushes;
    return 0;
}

PX_EXPORT int32_t picles_wind_stream_reset(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->wind.streamed()) return fail(c, -2, "picles_wind_stream_reset: picles_wind_stream_init first");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }      /* (a pending fused step is completed under its own window, as picles_set_wind_grid_mode does) */
    c->wind.ring_first = c->wind.ring_newest = -1;
    c->wind.invalidate();
    return 0;
}

PX_EXPORT int32_t picles_get_winds(picles_ctx *c, double *u0, double *v0, double *u1, double *v1)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    size_t b = (size_t)c->A.n * 8;
    if (u0) HIPCHK(c, hipMemcpy(u0, c->A.u0, b, hipMemcpyDeviceToHost));
    if (v0) HIPCHK(c, hipMemcpy(v0, c->A.v0, b, hipMemcpyDeviceToHost));
    if (u1) HIPCHK(c, hipMemcpy(u1, c->A.u1, b, hipMemcpyDeviceToHost));
    if (v1) HIPCHK(c, hipMemcpy(v1, c->A.v1, b, hipMemcpyDeviceToHost));
    return 0;
}

PX_EXPORT int32_t picles_get_winds_mid(picles_ctx *c, double *um, double *vm)
{
    if (!c) return -1;
    const double *mu, *mv;
    if (!c->wind.middle(c->A, mu, mv)) return 1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    size_t b = (size_t)c->A.n * 8;
    if (um) HIPCHK(c, hipMemcpy(um, mu, b, hipMemcpyDeviceToHost));
    if (vm) HIPCHK(c, hipMemcpy(vm, mv, b, hipMemcpyDeviceToHost));
    return 0;
}

/* picles_seed at clock t0; a lattice is sampled as the two-level window [wind_t, wind_t + wind_dt] (picles_seed: at 0.0 with the seed
 * time scale; picles_nest_prolong: at t0 with the step to come) */
static int seed_at(picles_ctx *c, double t0, double wind_t, double wind_dt)
{
    HIPCHK(c, hipSetDevice(c->device));
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());   /* earlier steps may still run on caller / ring streams */
    { int rc = c->wind.ring_seed_levels(c, wind_t); if (rc) return rc; }      /* (a wind stream: refused before anything has changed) */
    c->clock = t0;
    if (c->wind.streamed()) {
        /* a wind stream may not hold the window's end yet, and only level 0 is read: the level at wind_t in both planes of the seed's
         * two-level window (the same level 0, to the bit), which the first step replaces by its own */
        WindWindow &W = c->wind;
        int64_t k = 0;
        double f = 0.0;
        (void)picles_wind_stream_coord(W.lat_t0, W.lat_dt, wind_t, &k, &f);
        WindRingOut O{};
        for (int q = 0; q < 2; q++) {
            O.s0[q] = (int)(k % W.ring_slots);
            O.s1[q] = f != 0.0 ? (int)((k + 1) % W.ring_slots) : O.s0[q];
            O.f[q] = f;
        }
        O.u[0] = c->A.u0; O.v[0] = c->A.v0; O.u[1] = c->A.u1; O.v[1] = c->A.v1;
        hipLaunchKernelGGL(k_wind_sample_ring<2>, dim3(nblocks(c->A.n, 256)), dim3(256), 0, c->stream, c->G, W.wg, O, c->A.n);
        HIPCHK(c, hipGetLastError());
        WindWindow::Shape two;
        two.form = WindWindow::TWO;
        int rc = W.set(c, two, wind_t, wind_t + wind_dt, c->stream);
        if (rc) return rc;
        W.invalidate();
    } else if (c->wind.from_lattice()) {   /* winds at t = 0.0 seed the particles (run.jl:213-215) */
        /* only level 0 is read (k_seed evaluates the window at its start); the window's end is sampled at the seed time scale, whatever
         * lies between: a plain two-level window, replaced by the first step's own */
        c->wind.invalidate();
        WindWindow::Shape two;
        two.form = WindWindow::TWO;
        int rc = c->wind.sample(c, two, wind_t, wind_dt, true, c->stream);
        if (rc) return rc;
    }
    c->pending = false;
    c->ord_valid = false;
    c->cur = 0;
    c->mr_w = 0;
    for (int k = 0; k < 2; k++) {
        HIPCHK(c, hipMemsetAsync(c->rec_buf[k], 0, rec_bytes(c), c->stream));
        HIPCHK(c, hipMemsetAsync(c->mr_buf[k], 0, sizeof(int), c->stream));
        if (k == 0) for (int q = 2; q < 5; q++) HIPCHK(c, hipMemsetAsync(c->mr_buf[q], 0, sizeof(int), c->stream));
    }
    HIPCHK(c, hipMemsetAsync(c->A.cnt, 0, NSLOTS * sizeof(DevCounters), c->stream));
    HIPCHK(c, hipMemsetAsync(c->mr_buf[0] + 5, 0, 11 * sizeof(int), c->stream));      /* running maximum + the "calm waves" words (kernels.h: order_wanted) */
    HIPCHK(c, hipMemsetAsync(c->A.rmap, 0, (size_t)5 * c->A.ntile * sizeof(int), c->stream));
    { int rc = class_map_zero(c); if (rc) return rc; }
    /* k_seed reads the window at time 0.0 (run.jl:213-215).  A child started from its parent is seeded under the wind at wind_t: its
     * copy of the parameters carries the window's start moved back by wind_t (picles_seed: by 0.0, the same bits) */
    KParams seedP = c->P;
    seedP.tw0 = c->P.tw0 - wind_t;
    hipLaunchKernelGGL(k_seed, dim3(nblocks(c->A.n, 256)), dim3(256), 0, c->stream, seedP, c->G, arrays_for(c, 0, 0), c->d_mask, c->od.timestep);
    HIPCHK(c, hipGetLastError());
    c->state_zero = false;
    c->seeded = true;
    return 0;
}

PX_EXPORT int32_t picles_seed(picles_ctx *c, double t0)
{
    if (!c) return -1;
    return seed_at(c, t0, 0.0, c->od.timestep);
}

PX_EXPORT int32_t picles_zero_state(picles_ctx *c)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    /* launches on caller / ring streams (the un-fused slab phases: k_scatter on stream M) may still be writing State */
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemsetAsync(c->A.state, 0, 3 * c->A.n * 8, c->stream));
    c->state_zero = true;
    return 0;
}

PX_EXPORT int32_t picles_tick(picles_ctx *c, double dt)
{
    if (!c) return -1;
    c->clock += dt;
    return 0;
}

/* a model step begins: its length and flags, and the buffers that rotate with the steps */
static void step_begun(picles_ctx *c, double dt, int flags)
{
    c->step_dt = dt;
    c->step_flags = flags;
    c->edge_pending = false;
    c->cur ^= 1;            /* this step's records go to (and are scattered from) rec_buf[cur] */
    c->mr_w = (c->mr_w + 1) % 5;
    if (c->cmap_hot > 0) c->cmap_hot--;
}

static int begin_step(picles_ctx *c, double dt, int32_t flags)
{
    if (!(dt > 0.0)) return fail(c, -2, "dt must be positive");
    { int rc = c->wind.ring_levels(c, c->clock, dt, 1, "picles_begin_step"); if (rc) return rc; }      /* (before the flush: a refused call has changed nothing) */
    { int rc = flush(c); if (rc) return rc; }
    if (c->wind.from_lattice()) {  /* (first: a window the lattice cannot carry is refused before the step has changed anything) */
        HIPCHK(c, hipSetDevice(c->device));
        if (c->ext_streams && !c->ring_orders) HIPCHK(c, hipDeviceSynchronize());   /* previous step (any stream) done with the wind planes */
        int rc = c->wind.prepare(c, c->clock, dt, false, c->stream);
        if (rc) return rc;
        /* caller-stream launches wait for the sampler through ev_ctx (step_prologue) */
    }
    step_begun(c, dt, flags);
    return 0;
}

/* the split phases are the slab drivers' interface: they bring the edge rows' records to the neighbours before a kernel behind the
 * launch could add the forced nodes' (include/picles_hip.h, "open-boundary forcing") */
static const char *const BFORCE_NO_SLABS = ": the context has a boundary forcing set, which the split phases and slabs do not carry "
                                           "(picles_time_step / picles_run_steps / picles_advance do; or picles_bforce_free first)";
PX_EXPORT int32_t picles_begin_step(picles_ctx *c, double dt, int32_t flags)
{
    if (!c) return -1;
    if (c->bf_n) return fail(c, -5, std::string("picles_begin_step") + BFORCE_NO_SLABS);
    return begin_step(c, dt, flags);
}

/* the specialised variant of the step kernels: every physics switch on, n = 2, p = 3/4, no dead band (all reference scripts).
 * picles_create works it out once; nothing changes the switches afterwards */
static bool physics_fast(const KParams &P) { return P.fast_phys != 0; }

/* the row ranges of a selector; false: no such selector */
static bool rows_of(const GridP &G, int which, int &r0, int &n0, int &r1, int &n1)
{
    int R = G.R;
    r0 = n0 = r1 = n1 = 0;
    bool small = G.ny_loc <= 2 * R;
    if (which == PICLES_ROWS_ALL) { n0 = G.ny_loc; }
    else if (which == PICLES_ROWS_EDGE) {
        if (small) n0 = G.ny_loc;
        else { n0 = R; r1 = G.ny_loc - R; n1 = R; }
    } else if (which == PICLES_ROWS_INTERIOR) {
        if (!small) { r0 = R; n0 = G.ny_loc - 2 * R; }
    } else return false;
    return true;
}
static int select_rows(picles_ctx *c, int which, int &r0, int &n0, int &r1, int &n1)
{
    return rows_of(c->G, which, r0, n0, r1, n1) ? 0 : fail(c, -2, "bad row selector");
}

/* Launches of one step may come on caller-provided streams.  Whatever the library enqueued on its own stream before (the
 * scatter + remesh of a flushed step, a wind-lattice sample, the seed) must be complete before a caller-stream kernel reads
 * it: the caller stream waits for an event recorded on the context stream.  (The step's reach counter needs no clearing
 * here: five counters rotate and the launches of the step before last cleared this one, kernels.h: reach_counters.) */
static int step_prologue(picles_ctx *c, hipStream_t s)
{
    if (s != c->stream && !stream_idle(c->stream)) {     /* an idle context stream has nothing to wait for */
        HIPCHK(c, hipEventRecord(c->ev_ctx, c->stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->ev_ctx, 0));
    }
    return 0;
}

/* ---- open-boundary forcing: the checks the step entry points make, and the launch (the contract: include/picles_hip.h; the
 * kernel: k_bforce.hip; the set's own entry points: behind the run statistics) ---- */
/* do the start times of the next n_steps steps of length dt lie inside the level pair's window?  Asked before anything is enqueued;
 * a time closer to an end of the window than 1e-9 of its length is that end (the rule of picles_lattice_knots) */
static int bforce_window(picles_ctx *c, double dt, long long n_steps, const char *who)
{
    if (!c->bf_n || n_steps <= 0) return 0;
    if (!c->bf_levels) return fail(c, -2, std::string(who) + ": the boundary forcing set has no levels yet: picles_bforce_set_levels first");
    if (c->bf_levels == 1) return 0;
    const double slack = 1e-9 * (c->bf_t1 - c->bf_t0);
    double t = c->clock;
    for (long long k = 0; k < n_steps; k++, t += dt)
        if (!(t >= c->bf_t0 - slack && t <= c->bf_t1 + slack)) {
            char b[384];
            snprintf(b, sizeof b, "%s: step %lld of this call starts at t = %.17g, outside the window [%.17g, %.17g] of the boundary forcing levels: "
                                  "call picles_bforce_set_levels with the pair that brackets that time first, or take fewer steps per call",
                     who, k + 1, t, c->bf_t0, c->bf_t1);
            return fail(c, -2, b);
        }
    return 0;
}

/* the forced nodes' particles of the step in flight, behind the launch that wrote its records for the whole grid, on its stream:
 * the same record buffer, the same generation of the reach counters and maps (A: the Arrays that launch was given) */
/* from_rec: that launch scatters a pending fused step (A.rec holds its records, A.mr_idx its reach): State at the step's start, which
 * a weighted set blends into, exists as those records only — probe_launch's choice */
static int bforce_launch(picles_ctx *c, hipStream_t s, const Arrays &A, bool from_rec)
{
    BForceP B;
    B.n = c->bf_n;
    B.nodes = c->bf_nodes;
    B.w = c->bf_w;
    B.from_rec = from_rec ? 1 : 0;
    { int rc = nest_levels_wait(c, s); if (rc) return rc; }      /* levels another context's stream wrote: read after write */
    B.v0 = c->bf_v0;
    B.v1 = c->bf_levels == 2 ? c->bf_v1 : nullptr;
    B.s = c->bf_levels == 2 ? (c->clock - c->bf_t0) / (c->bf_t1 - c->bf_t0) : 0.0;
    StepLaunch L = {dim3(1), dim3(256), s, &c->P, &c->G, &A, 0.0, 0.0, c->clock, c->step_dt, 0, 0, 0, 0};
    launch_k_bforce(L, B, c->P.solver, c->A.pc != nullptr);      /* k_bforce.hip */
    HIPCHK(c, hipGetLastError());
    return nest_levels_read(c, s, B.v0);      /* the slot this launch read: write after read */
}
/* a launch over some of the rows is a slab's: refused with a set (nothing has been launched) */
static int bforce_rows(picles_ctx *c, int which, const char *who)
{
    if (c->bf_n && (which != PICLES_ROWS_ALL || !c->G.single_slab)) return fail(c, -5, std::string(who) + BFORCE_NO_SLABS);
    if (c->bf_n && !c->bf_levels) return fail(c, -2, std::string(who) + ": the boundary forcing set has no levels yet: picles_bforce_set_levels first");
    return 0;
}

PX_EXPORT int32_t picles_advance_rows(picles_ctx *c, int32_t which, void *stream)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (stream) c->ext_streams = true;
    int r0, n0, r1, n1;
    int rc = select_rows(c, which, r0, n0, r1, n1);
    if (rc) return rc;
    long long nt = (long long)(n0 + n1) * c->G.Nx;
    if (nt == 0) return 0;
    if ((rc = bforce_rows(c, which, "picles_advance_rows"))) return rc;
    if ((rc = step_prologue(c, s))) return rc;
    c->ord_valid = false;        /* the stand-alone advance files no dispatch order */
    if (c->cmap_hot > 0 && (rc = class_map_clear_rows(c, s, r0, n0, r1, n1))) return rc;
    Arrays A = arrays_for(c, c->cur, c->cur);
    timing_begin(c, s, 0);
    {
        const KParams &P = c->P;
        bool fast = physics_fast(P);
        if (c->wind.polyline()) fast = false;     /* a polyline window: the general flavours carry it (same bits: the oracle's one arithmetic) */
        StepLaunch L = {dim3(nblocks(nt, 256)), dim3(256), s, &c->P, &c->G, &A, 0.0, 0.0, c->clock, c->step_dt, r0, n0, r1, n1};
        launch_k_advance(L, fast, P.solver, c->wind.static_(), c->A.pc != nullptr);      /* k_advance.hip */
    }
    timing_end(c, s);
    HIPCHK(c, hipGetLastError());
    if (c->bf_n && (rc = bforce_launch(c, s, A, false))) return rc;
    if (which == PICLES_ROWS_EDGE && s != c->stream) {
        HIPCHK(c, hipEventRecord(c->ev_edge, s));
        c->edge_pending = true;
    }
    return 0;
}

/* can this step ride on fused k_step launches? (run!-style: State zeroed first, static winds) */
static bool step_fusable(const picles_ctx *c, int flags, double dt)
{
    if (flags != PICLES_STEP_ZERO_FIRST) return false;
    const KParams &P = c->P;
    /* a polyline window (two or more lattice knots inside the step; host levels set by picles_set_winds_polyline) takes the plain
     * phases: only the general flavours of the stand-alone advance evaluate one */
    const WindWindow &W = c->wind;
    if (W.from_lattice() ? W.lattice_polyline_ahead(c->clock, dt) : W.polyline()) return false;
    const bool fast = physics_fast(P);
    /* the time-varying-wind and per-node-metric flavours of the fused kernel exist for the specialised physics */
    if (W.from_lattice()) return fast;
    if (c->A.pc) return fast && W.static_();
    if (P.solver == 2) return fast && W.static_();   /* the auto-switching flavour exists for the specialised physics */
    return W.static_();
}

/* does the fused launch of these rows take k_step_waverow? */
static bool step_rows_waverow(const picles_ctx *c, int which)
{
    int r0, n0, r1, n1;
    if (!rows_of(c->G, which, r0, n0, r1, n1)) return false;
    if (n0 + n1 == 0) return true;             /* (nothing is launched) */
    return waverow_flavour(physics_fast(c->P), c->A.pc != nullptr) && waverow_geometry(c->G.Nx, n0, n1);
}

/* the flavours the default mode hands to k_step_waverow: those timed against k_step, same session, and found faster.
 * The Tsit5, time-varying-wind and default-solver flavours give the same bits (tests/test_gpu_waverow.py) but have not been timed:
 * they stay on k_step unless PICLES_WAVEROW=require asks for them */
static bool waverow_measured(const picles_ctx *c) { return c->P.solver == 0 && c->wind.static_(); }

/* fused phase launcher: scatter+remesh of the pending step and advance of the current one for the
 * selected rows (records of the pending step: rec_buf[1-cur], of this step: rec_buf[cur]) */
static int launch_step_rows(picles_ctx *c, int which, hipStream_t s)
{
    int r0, n0, r1, n1;
    int rc = select_rows(c, which, r0, n0, r1, n1);
    if (rc) return rc;
    long long nt = (long long)(n0 + n1) * c->G.Nx;
    if (nt == 0) return 0;
    if ((rc = bforce_rows(c, which, "picles_step_rows"))) return rc;
    if ((rc = step_prologue(c, s))) return rc;
    const KParams &P = c->P;
    Arrays A = arrays_for(c, c->cur ^ 1, c->cur);
    /* specialised variant: every physics switch on and n = 2 (all reference scripts) */
    bool fast = physics_fast(P);
    /* cost-ordered dispatch (kernels.h): the launch that covers (nearly) everything — the whole grid of a plain context, the interior
     * rows of a slab — files an order over ITS workgroups and follows the one its predecessor of the same shape filed.  The edge
     * launch of a slab (a handful of workgroups, on the other stream) neither reads nor files one and leaves the chain alone; a
     * stand-alone advance, a re-seed or a change of the launch shape (halo resize) breaks it (its counters are cleared on the way). */
    const bool orders = c->A.ord && (c->G.single_slab ? which == PICLES_ROWS_ALL : which == PICLES_ROWS_INTERIOR);
    if (orders) {
        A.nblk = (int)nblocks(nt, 256);
        const bool follows = c->ord_valid && c->ord_nblk == A.nblk;
        if (!follows) HIPCHK(c, hipMemsetAsync(c->A.ord, 0, (size_t)5 * (2 + c->A.nblk) * sizeof(int), s));
        A.ord_on = follows ? 1 : 0;
        c->ord_valid = true;
        c->ord_nblk = A.nblk;
    } else {
        A.ord = nullptr;            /* (this launch neither reads nor files an order) */
        if (c->G.single_slab || which != PICLES_ROWS_EDGE) c->ord_valid = false;
    }
    /* (the four-wave static flavours of k_step_waverow fetch u0, v0 and ln q_old sixteen bytes at a time: kernels.h, stage_aligned;
     * planes that are not so aligned take k_step, same bits) */
    const bool staged = c->wind.static_() && !(fast && P.solver == 2);
    const bool waverow = (c->waverow_mode == 2 || (c->waverow_mode == 1 && waverow_measured(c))) && step_rows_waverow(c, which) &&
                         (!staged || stage_aligned(A));
    if (waverow && c->pull_class) c->cmap_hot = 4;       /* its entries live in buffer mr_w until the step after next but one clears them */
    else if (!waverow && c->cmap_hot > 0 && (rc = class_map_clear_rows(c, s, r0, n0, r1, n1))) return rc;
    timing_begin(c, s, 0);
    {
        StepLaunch L = {dim3(nblocks(nt, 256)), dim3(256), s, &c->P, &c->G, &A, c->pend_t, c->pend_dt, c->clock, c->step_dt, r0, n0, r1, n1, waverow};
        if (fast && P.solver == 2) launch_k_step_auto(L, c->wind.static_(), c->A.pc != nullptr);          /* k_step_auto.hip */
        else launch_k_step_explicit(L, fast, P.solver, c->wind.static_(), c->A.pc != nullptr);             /* k_step_explicit.hip */
    }
    timing_end(c, s);
    HIPCHK(c, hipGetLastError());
    if (c->bf_n && (rc = bforce_launch(c, s, A, true))) return rc;
    return 0;
}

/* Slab form of the fused step.  Per model step:
 *   picles_begin_fused_step(dt)            (returns 1 if the step cannot be fused: use the plain phases)
 *   picles_step_rows(EDGE, stream_E)  ->  exchange halo blocks  ||  picles_step_rows(INTERIOR, stream_M)
 *   picles_end_fused_step()                (ticks the clock; scatter+remesh of this step stay pending) */
PX_EXPORT int32_t picles_begin_fused_step(picles_ctx *c, double dt)
{
    if (!c) return -1;
    if (!(dt > 0.0)) return fail(c, -2, "dt must be positive");
    { int rc = bforce_window(c, dt, 1, "picles_begin_fused_step"); if (rc) return rc; }
    { int rc = c->wind.ring_levels(c, c->clock, dt, 1, "picles_begin_fused_step"); if (rc) return rc; }
    if (!step_fusable(c, PICLES_STEP_ZERO_FIRST, dt)) return 1;
    /* PICLES_WAVEROW=require: every launch of the step — the whole grid, or a slab's edge and interior rows — must take k_step_waverow;
     * refused here, before the step has changed anything */
    if (c->waverow_mode == 2 && !(c->G.single_slab ? step_rows_waverow(c, PICLES_ROWS_ALL)
                                                   : step_rows_waverow(c, PICLES_ROWS_EDGE) && step_rows_waverow(c, PICLES_ROWS_INTERIOR)))
        return fail(c, -5, "PICLES_WAVEROW=require: a fused launch of this step does not qualify for k_step_waverow (one row range, "
                           "Nx a multiple of 64, rows a multiple of 4, specialised physics without the per-node metric)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->wind.from_lattice()) {
        /* device-sampled winds.  With a step pending, its remesh (done by this step's launches) needs the wind at ITS clock: level 0
         * of its window, which prepare() keeps in (uP, vP) */
        if (c->pending && !c->wind.contiguous_with(c->pend_t, c->clock))
            return 1;   /* the windows are not contiguous: take the plain phases (they flush first) */
        /* earlier launches on other streams read the planes (the native slab ring orders its own streams with events) */
        if (c->ext_streams && !c->ring_orders) HIPCHK(c, hipDeviceSynchronize());
        int rc = c->wind.prepare(c, c->clock, dt, c->pending, c->stream);
        if (rc) return rc;
        if (c->ext_streams && !c->ring_orders) HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    step_begun(c, dt, PICLES_STEP_ZERO_FIRST);
    return 0;
}

PX_EXPORT int32_t picles_step_rows(picles_ctx *c, int32_t which, void *stream)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (stream) c->ext_streams = true;
    if (!c->pending) return picles_advance_rows(c, which, stream);   /* first step: nothing to scatter yet */
    return launch_step_rows(c, which, s);
}

PX_EXPORT int32_t picles_end_fused_step(picles_ctx *c)
{
    if (!c) return -1;
    c->pending = true;
    c->pend_t = c->clock;
    c->pend_dt = c->step_dt;
    c->state_zero = false;
    c->edge_pending = false;
    step_completed(c);
    return 0;
}

static int launch_scatter(picles_ctx *c, hipStream_t s, bool remesh)
{
    Arrays A = arrays_for(c, c->cur, c->cur);
    int flags = c->step_flags;
    bool movie = (flags & PICLES_STEP_MOVIE) != 0;
    bool zero_first = (flags & PICLES_STEP_ZERO_FIRST) != 0;
    int accum = (zero_first || c->state_zero) ? 0 : 1;
    if (flags & PICLES_STEP_ATOMIC) {
        if (!c->G.single_slab) return fail(c, -5, "PICLES_STEP_ATOMIC is single-slab only");
        if (c->G.tripolar) return fail(c, -5, "PICLES_STEP_ATOMIC does not implement the tripolar fold: use the deterministic pull");
        if (!accum) HIPCHK(c, hipMemsetAsync(c->A.state, 0, 3 * c->A.n * 8, s));
        int ntx = (c->G.Nx + PT_TX - 1) / PT_TX, nty = (c->G.ny_loc + PT_TY - 1) / PT_TY;
        timing_begin(c, s, 1);
        hipLaunchKernelGGL(k_push_tiles<true>, dim3(ntx * nty), dim3(256), 0, s, c->G, A, ntx,
                           (const int *)nullptr, (const int *)nullptr, (const int *)nullptr,
                           (const double *)nullptr, (const double *)nullptr, 0LL);
        timing_end(c, s);
        HIPCHK(c, hipGetLastError());
        if (movie) HIPCHK(c, hipMemcpyAsync(c->A.movie, c->A.state, 3 * c->A.n * 8, hipMemcpyDeviceToDevice, s));
        if (remesh) {
            timing_begin(c, s, 2);
            hipLaunchKernelGGL(k_remesh, dim3(nblocks(c->A.n, 256)), dim3(256), 0, s, c->P, c->G, A, c->clock, c->step_dt);
            timing_end(c, s);
            HIPCHK(c, hipGetLastError());
        }
        if (movie && remesh) HIPCHK(c, hipMemsetAsync(c->A.state, 0, 3 * c->A.n * 8, s));
        c->state_zero = movie && remesh;
        return 0;
    }
    timing_begin(c, s, 1);
    if (remesh)
        hipLaunchKernelGGL(k_scatter<true>, dim3(nblocks(c->A.n, 256)), dim3(256), 0, s, c->P, c->G, A, accum, movie ? 1 : 0, c->clock, c->step_dt);
    else
        hipLaunchKernelGGL(k_scatter<false>, dim3(nblocks(c->A.n, 256)), dim3(256), 0, s, c->P, c->G, A, accum, 0, c->clock, c->step_dt);
    timing_end(c, s);
    HIPCHK(c, hipGetLastError());
    c->state_zero = movie && remesh;
    return 0;
}

PX_EXPORT int32_t picles_scatter_remesh(picles_ctx *c, void *stream)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->edge_pending) { HIPCHK(c, hipStreamWaitEvent(s, c->ev_edge, 0)); c->edge_pending = false; }
    int rc = step_prologue(c, s);      /* ordered behind whatever the library enqueued on its own stream */
    if (rc || (rc = launch_scatter(c, s, true))) return rc;
    step_completed(c);
    return 0;
}

static int time_step_phases(picles_ctx *c, double dt, int32_t flags)
{
    if (step_fusable(c, flags, dt)) {
        /* run!-style consecutive steps: one launch per step (k_step), the scatter + remesh of the
         * previous step ride along; the last one is flushed when somebody looks */
        int rc0 = picles_begin_fused_step(c, dt);
        if (rc0) return rc0 < 0 ? rc0 : fail(c, -6, "internal: fusable step refused");
        if ((rc0 = picles_step_rows(c, PICLES_ROWS_ALL, nullptr))) return rc0;
        return picles_end_fused_step(c);
    }
    int rc = begin_step(c, dt, flags);
    if (rc) return rc;
    rc = picles_advance_rows(c, PICLES_ROWS_ALL, nullptr);
    if (rc) return rc;
    return picles_scatter_remesh(c, nullptr);
}

PX_EXPORT int32_t picles_time_step(picles_ctx *c, double dt, int32_t flags)
{
    if (!c) return -1;
    if (!c->G.single_slab) return fail(c, -5, "picles_time_step needs the whole grid; slabs use begin_step/advance_rows/scatter_remesh");
    if (!(dt > 0.0)) return fail(c, -2, "dt must be positive");
    { int rc = probe_room(c, 1, "picles_time_step"); if (rc) return rc; }      /* refused before anything has changed */
    { int rc = bforce_window(c, dt, 1, "picles_time_step"); if (rc) return rc; }
    { int rc = c->wind.ring_levels(c, c->clock, dt, 1, "picles_time_step"); if (rc) return rc; }
    { int rc = track_step_ok(c, dt, "picles_time_step"); if (rc) return rc; }
    int rc = time_step_phases(c, dt, flags);
    if (rc) return rc;
    /* the sample of this step: directly behind its launch on the context stream.  The next step's launch reads the record buffer
     * the probe reads and writes the other one: stream order is all the ordering there is */
    if (c->probe_n && c->probe_cad.due(c->probe_cad.steps)) { if ((rc = probe_take(c, c->stream))) return rc; }
    /* the track sample of this step, at the clock after the tick: the same place, the same ordering */
    if (c->trk && (rc = track_take(c, c->stream))) return rc;
    /* the statistics update of this step: the same place, the same ordering */
    if (c->stat_on && c->stat_cad.due(c->stat_cad.steps)) { if ((rc = stat_update(c, c->stream))) return rc; }
    /* the flux-mean update of this step: the same place, the same ordering */
    if (c->fm_on && c->fm_cad.due(c->fm_cad.steps)) return flux_mean_update(c, c->stream, "picles_time_step");
    return 0;
}

PX_EXPORT int32_t picles_run_steps(picles_ctx *c, double dt, int32_t n_steps)
{
    if (!c || n_steps < 0) return -1;
    if (c->G.single_slab && dt > 0.0) { int rc = probe_room(c, n_steps, "picles_run_steps"); if (rc) return rc; }   /* up front, not half-way */
    if (c->G.single_slab && dt > 0.0) { int rc = bforce_window(c, dt, n_steps, "picles_run_steps"); if (rc) return rc; }   /* every start time, before anything is enqueued */
    if (n_steps > 0) { int rc = track_step_ok(c, dt, "picles_run_steps"); if (rc) return rc; }
    { int rc = c->wind.ring_levels(c, c->clock, dt, n_steps, "picles_run_steps"); if (rc) return rc; }      /* a wind stream: every level, before anything is enqueued */
    const bool region = c->timing && c->timing_mode == 2 && n_steps > 0;
    if (region) {      /* one event pair around the whole call, on the stream the launches go to */
        HIPCHK(c, hipSetDevice(c->device));
        timing_begin(c, c->stream, 3);
        c->in_region = true;
        c->region_launches = 0;
    }
    int rc = 0;
    for (int k = 0; k < n_steps && rc == 0; k++) rc = picles_time_step(c, dt, PICLES_STEP_ZERO_FIRST);
    if (region) {
        c->in_region = false;
        timing_end(c, c->stream);
        c->tim.advance_launches += (uint64_t)c->region_launches;
    }
    return rc;
}

PX_EXPORT int32_t picles_advance(picles_ctx *c, double dt, int32_t flags)
{
    if (!c) return -1;
    if (!c->G.single_slab) return fail(c, -5, "picles_advance needs the whole grid");
    int rc = (dt > 0.0) ? bforce_window(c, dt, 1, "picles_advance") : 0;
    if (rc || (rc = begin_step(c, dt, flags & ~(PICLES_STEP_MOVIE)))) return rc;
    rc = picles_advance_rows(c, PICLES_ROWS_ALL, nullptr);
    if (rc) return rc;
    return launch_scatter(c, c->stream, false);
}

PX_EXPORT int32_t picles_remesh(picles_ctx *c, double dt)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    timing_begin(c, c->stream, 2);
    hipLaunchKernelGGL(k_remesh, dim3(nblocks(c->A.n, 256)), dim3(256), 0, c->stream, c->P, c->G, arrays_for(c, c->cur, c->cur), c->clock, dt);
    timing_end(c, c->stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

/* ---- data access ---- */
static int d2h(picles_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    HIPCHK(c, hipDeviceSynchronize());   /* kernels may have run on caller-provided streams */
    /* a BLOCKING copy into the caller's (pageable) buffer: when this returns the runtime has written the last byte of it and
     * holds no staging reference to it any more — the caller may free the buffer at once (ctypes / ccall hosts do) */
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}
static int h2d(picles_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

PX_EXPORT int32_t picles_get_state(picles_ctx *c, double *s) { return (c && s) ? d2h(c, s, c->A.state, 3 * c->A.n * 8) : -1; }
PX_EXPORT int32_t picles_get_movie_state(picles_ctx *c, double *s) { return (c && s) ? d2h(c, s, c->A.movie, 3 * c->A.n * 8) : -1; }
PX_EXPORT int32_t picles_set_state(picles_ctx *c, const double *s)
{
    if (!c || !s) return -1;
    c->state_zero = false;
    return h2d(c, c->A.state, s, 3 * c->A.n * 8);
}

PX_EXPORT int32_t picles_get_particles(picles_ctx *c, double *z, uint8_t *on, uint8_t *boundary, int32_t *status)
{
    if (!c) return -1;
    int rc = 0;
    if (z && (rc = d2h(c, z, c->A.z, 5 * c->A.n * 8))) return rc;
    if (on && (rc = d2h(c, on, c->A.on, c->A.n))) return rc;
    if (status && (rc = d2h(c, status, c->A.status, c->A.n * 4))) return rc;
    if (boundary) {
        std::vector<unsigned char> pf(c->A.n);
        if ((rc = d2h(c, pf.data(), c->A.pflags, c->A.n))) return rc;
        for (long long k = 0; k < c->A.n; k++) boundary[k] = (pf[k] & PF_BOUNDARY) ? 1 : 0;
    }
    return 0;
}

PX_EXPORT int32_t picles_set_particles(picles_ctx *c, const double *z, const uint8_t *on)
{
    if (!c) return -1;
    int rc = 0;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = class_map_zero(c))) return rc;
    if (z && (rc = h2d(c, c->A.z, z, 5 * c->A.n * 8))) return rc;
    if (on && (rc = h2d(c, c->A.on, on, c->A.n))) return rc;
    std::vector<double> neg(c->A.n, -1.0);   /* auto_dt_reset! on the next advance */
    return h2d(c, c->A.dtn, neg.data(), c->A.n * 8);
}

PX_EXPORT int32_t picles_get_counters(picles_ctx *c, picles_counters *out)
{
    if (!c || !out) return -1;
    std::vector<DevCounters> d(NSLOTS);
    int rc = d2h(c, d.data(), c->A.cnt, NSLOTS * sizeof(DevCounters));
    if (rc) return rc;
    int mr = 0, mrt = 0;
    if ((rc = d2h(c, &mr, c->mr_buf[c->mr_w], sizeof(int)))) return rc;
    if ((rc = d2h(c, &mrt, c->mr_buf[0] + 5, sizeof(int)))) return rc;
    memset(out, 0, sizeof(*out));
    for (const DevCounters &k : d) {
        out->rhs_evals += k.rhs; out->steps_accepted += k.acc; out->steps_rejected += k.rej;
        out->reseeds += k.reseeds; out->clamps += k.clamps; out->maxiters_hits += k.maxit;
        out->particles_advanced += k.adv; out->halo_overflow += k.overflow;
        out->dropped_nonfinite += k.nonfinite;
        out->wave_attempt_slots += k.wslots;
    }
#ifdef PICLES_PHASE_CLOCK
    {
        unsigned long long p0 = 0, p1 = 0, p2 = 0, nw = 0;
        for (const DevCounters &k : d) { p0 += k.pad_[0]; p1 += k.pad_[1]; p2 += k.pad_[2]; nw += k.pad_[3]; }
        if (nw) fprintf(stderr, "PHASE_CLOCK waves %llu: prologue+pull %.0f, RK+guards %.0f, record+stats %.0f cycles per wave (lane 0's view)\n",
                        nw, (double)p0 / nw, (double)p1 / nw, (double)p2 / nw);
    }
#endif
    out->max_reach = mr;
    out->max_reach_seen = mrt;
    return 0;
}

PX_EXPORT int32_t picles_get_pull_class_counts(picles_ctx *c, int64_t *out)
{
    if (!c || !out) return -1;
    std::vector<DevCounters> d(NSLOTS);
    HIPCHK(c, hipSetDevice(c->device));
    /* no flush: a pending fused step stays pending (asking after every step must not take the run off the fused launches it counts) */
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(d.data(), c->A.cnt, NSLOTS * sizeof(DevCounters), hipMemcpyDeviceToHost));
    out[0] = out[1] = 0;
    for (const DevCounters &k : d) { out[0] += (int64_t)k.cls; out[1] += (int64_t)k.cls_empty; }
    return 0;
}

PX_EXPORT int32_t picles_get_dispatch_order(picles_ctx *c, int32_t *out, int32_t cap)
{
    if (!c) return -1;
    if (cap < 0 || (cap > 0 && !out)) return fail(c, -2, "picles_get_dispatch_order: bad buffer");
    if (!c->A.ord || !c->ord_valid) return 0;
    const int n = c->ord_nblk;
    std::vector<int> h((size_t)2 + n);
    /* the buffer the latest step wrote: the counters rotate at the end of a step */
    int rc = d2h(c, h.data(), c->A.ord + (size_t)((c->mr_w + 4) % 5) * (size_t)(2 + n), h.size() * sizeof(int));
    if (rc) return rc;
    if (h[0] + h[1] != n) return 0;
    const int m = cap < 2 + n ? cap : 2 + n;
    for (int k = 0; k < m; k++) out[k] = h[k];
    return n;
}

PX_EXPORT int32_t picles_reset_counters(picles_ctx *c)
{
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    /* no flush: a pending fused step stays pending (its scatter + remesh ride on the next step's launch as usual; the
     * re-seeds of that remesh are then counted in the new window — as the last step of the window leaves its own behind) */
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemsetAsync(c->A.cnt, 0, NSLOTS * sizeof(DevCounters), c->stream));
    HIPCHK(c, hipMemsetAsync(c->mr_buf[0] + 5, 0, sizeof(int), c->stream));
    return 0;
}

PX_EXPORT int32_t picles_enable_timing(picles_ctx *c, int32_t on)
{
    if (!c) return -1;
    timing_collect(c);          /* (does not flush a pending fused step: see picles_reset_counters) */
    c->timing = on != 0;
    c->timing_mode = (on == 2) ? 2 : (on ? 1 : 0);
    if (on) { memset(&c->tim, 0, sizeof(c->tim)); for (auto &v : c->tim_samples) v.clear(); }
    return 0;
}

PX_EXPORT int32_t picles_get_timing(picles_ctx *c, picles_timing *t)
{
    if (!c || !t) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    timing_collect(c);
    *t = c->tim;
    return 0;
}

PX_EXPORT int32_t picles_get_timing_samples(picles_ctx *c, int32_t kind, double *out_ms, int32_t cap)
{
    if (!c || kind < 0 || kind > 2 || cap < 0 || (cap > 0 && !out_ms)) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    timing_collect(c);
    const std::vector<float> &v = c->tim_samples[kind];
    int n = (int)std::min<size_t>(v.size(), (size_t)cap);
    for (int k = 0; k < n; k++) out_ms[k] = v[k];
    return (int32_t)v.size();
}

/* ---- the output ring (OutRing, in front of the context) ---- */
static int store_stream_get(picles_ctx *c)      /* the store stream, made by whoever needs it first */
{
    if (!c->store_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->store_stream, hipStreamNonBlocking));
    return 0;
}

/* the hand-off every output path ends with: `bytes` at dev are complete in the order of stream `producer`; copy them to the pinned
 * block at host on the store stream, beside whatever the producer runs next.  `done` tells a reader that the copy has landed */
static int ship_d2h(picles_ctx *c, hipStream_t producer, hipEvent_t ready, hipEvent_t done, void *host, const void *dev, size_t bytes)
{
    HIPCHK(c, hipEventRecord(ready, producer));
    HIPCHK(c, hipStreamWaitEvent(c->store_stream, ready, 0));
    HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->store_stream));
    HIPCHK(c, hipEventRecord(done, c->store_stream));
    return 0;
}

void OutRing::release()
{
    if (dev) hipFree(dev);
    if (host) hipHostFree(host);
    for (auto *v : {&ready, &done})
        for (hipEvent_t e : *v) if (e) hipEventDestroy(e);
    *this = OutRing{};
}

int OutRing::init(picles_ctx *c, int n_slots, size_t slot_bytes)
{
    Undo undo{[this] { release(); }};
    { int rc = store_stream_get(c); if (rc) return rc; }
    stride = (slot_bytes + 15) & ~(size_t)15;
    HIPCHK(c, hipMalloc(&dev, (size_t)n_slots * stride));
    HIPCHK(c, hipHostMalloc(&host, (size_t)n_slots * stride, hipHostMallocDefault));
    ready.assign(n_slots, nullptr);
    done.assign(n_slots, nullptr);
    for (int k = 0; k < n_slots; k++) {
        HIPCHK(c, hipEventCreateWithFlags(&ready[k], hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    }
    time.assign(n_slots, 0.0);
    step.assign(n_slots, 0);
    cap = n_slots;
    undo.armed = false;
    return 0;
}

int OutRing::ship(picles_ctx *c, unsigned char *slot, hipStream_t producer, size_t bytes, long long step_tag)
{
    const int k = (int)((size_t)(slot - dev) / stride);
    { int rc = ship_d2h(c, producer, ready[k], done[k], host + (slot - dev), slot, bytes); if (rc) return rc; }
    time[k] = c->clock;
    step[k] = step_tag;
    count++;
    return 0;
}

int OutRing::front(picles_ctx *c, Slot &out)
{
    HIPCHK(c, hipEventSynchronize(done[head]));      /* this slot's copy alone: later work stays enqueued */
    out = Slot{host + (size_t)head * stride, time[head], step[head]};
    return 0;
}

/* ---- snapshot ring ---- */
PX_EXPORT int32_t picles_store_init(picles_ctx *c, int32_t n_slots)
{
    if (!c || n_slots < 1) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (c->store.cap) return fail(c, -2, "store already initialised");
    return c->store.init(c, n_slots, 3 * (size_t)c->A.n * 8);
}

PX_EXPORT int32_t picles_store_pending(const picles_ctx *c) { return c ? c->store.count : -1; }

PX_EXPORT int32_t picles_store_push(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->store.cap) return fail(c, -2, "picles_store_init first");
    unsigned char *d = c->store.next_slot();
    if (!d) return fail(c, -3, "snapshot ring full: pop first");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());   /* an un-fused slab step leaves its scatter on the ring's stream M */
    const size_t b = 3 * (size_t)c->A.n * 8;
    /* stream-ordered behind the step that produced State; the D2H leg runs beside the next steps */
    HIPCHK(c, hipMemcpyAsync(d, c->A.state, b, hipMemcpyDeviceToDevice, c->stream));
    return c->store.ship(c, d, c->stream, b, 0);
}

PX_EXPORT int32_t picles_store_pop(picles_ctx *c, double *state, double *time)
{
    if (!c || !state) return -1;
    if (!c->store.count) return fail(c, -3, "no snapshot pending");
    HIPCHK(c, hipSetDevice(c->device));
    OutRing::Slot s;
    { int rc = c->store.front(c, s); if (rc) return rc; }
    memcpy(state, s.host, 3 * (size_t)c->A.n * 8);
    if (time) *time = s.time;
    c->store.drop();
    return 0;
}

/* ---- coarse diagnostics ring (the definition: include/picles_hip.h; the kernel: k_diag.h) ---- */
PX_EXPORT int32_t picles_diag_init(picles_ctx *c, int32_t cx, int32_t cy, int32_t field_mask, int32_t n_slots)
{
    if (!c) return -1;
    if (cx < 1 || cx > 16 || cy < 1 || cy > 16) return fail(c, -2, "picles_diag_init: coarsening factors must be 1 ... 16");
    if (field_mask <= 0 || (field_mask & ~PICLES_DIAG_ALL)) return fail(c, -2, "picles_diag_init: empty or unknown field mask");
    if (n_slots < 1) return fail(c, -2, "picles_diag_init: n_slots must be >= 1");
    if (c->diag_ring.cap) return fail(c, -2, "picles_diag_init: diagnostics already initialised");
    if (c->G.j_begin % cy != 0) return fail(c, -2, "picles_diag_init: the slab's j_begin must be a multiple of cy (coarse cells are global)");
    HIPCHK(c, hipSetDevice(c->device));
    DiagP D{};
    D.Nx = c->G.Nx; D.ny_loc = c->G.ny_loc; D.cx = cx; D.cy = cy;
    D.Nxc = (c->G.Nx + cx - 1) / cx; D.nyc_loc = (c->G.ny_loc + cy - 1) / cy;
    D.tiles_per_row = (D.Nxc + DIAG_TILE - 1) / DIAG_TILE;
    D.mask = (unsigned)field_mask; D.g = c->ph.g; D.r_g = c->ph.r_g; D.plane = c->A.n;
    const int nf = __builtin_popcount((unsigned)field_mask), np = D.nyc_loc * D.tiles_per_row;
    const size_t fb = (size_t)4 * D.Nxc * D.nyc_loc * nf, po = (fb + 15) & ~(size_t)15, sb = po + (size_t)np * 7 * 8;
    { int rc = c->diag_ring.init(c, n_slots, sb); if (rc) return rc; }
    c->diag = D; c->diag_nfields = nf; c->diag_npart = np;
    c->diag_field_bytes = fb; c->diag_part_off = po; c->diag_slot_bytes = sb;
    return 0;
}

PX_EXPORT int32_t picles_diag_shape(const picles_ctx *c, int32_t *nxc, int32_t *nyc_loc, int32_t *n_fields, int32_t *n_partials, size_t *bytes)
{
    if (!c || !c->diag_ring.cap) return -1;
    if (nxc) *nxc = c->diag.Nxc;
    if (nyc_loc) *nyc_loc = c->diag.nyc_loc;
    if (n_fields) *n_fields = c->diag_nfields;
    if (n_partials) *n_partials = c->diag_npart;
    if (bytes) *bytes = c->diag_field_bytes;
    return 0;
}

PX_EXPORT int32_t picles_diag_pending(const picles_ctx *c) { return c ? c->diag_ring.count : -1; }

template <int CX, bool VEC>
static void diag_launch(picles_ctx *c, float *fields, double *partials)
{
    hipLaunchKernelGGL((k_diag<CX, VEC>), dim3((unsigned)c->diag_npart), dim3(DIAG_TILE), 0, c->stream, c->diag, (const double *)c->A.state,
                       fields, partials);
}

/* State at the step boundary, then the kernel on the context stream into (fields, partials): a ring slot (push) or the caller's
 * device buffers (export) */
static int diag_run(picles_ctx *c, float *fields, double *partials)
{
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());   /* an un-fused slab step leaves its scatter on the ring's stream M */
    const bool vec = (c->diag.Nx & 1) == 0;                  /* every cell's row segment then starts on a 16-byte boundary */
    timing_begin(c, c->stream, 4);
    switch (c->diag.cx) {
    case 1: diag_launch<1, false>(c, fields, partials); break;
    case 2: if (vec) diag_launch<2, true>(c, fields, partials); else diag_launch<2, false>(c, fields, partials); break;
    case 4: if (vec) diag_launch<4, true>(c, fields, partials); else diag_launch<4, false>(c, fields, partials); break;
    default: diag_launch<0, false>(c, fields, partials);
    }
    timing_end(c, c->stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

PX_EXPORT int32_t picles_diag_push(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->diag_ring.cap) return fail(c, -2, "picles_diag_init first");
    unsigned char *d = c->diag_ring.next_slot();
    if (!d) return fail(c, -3, "diagnostics ring full: pop first");
    { int rc = diag_run(c, (float *)d, (double *)(d + c->diag_part_off)); if (rc) return rc; }
    /* stream-ordered behind the step that produced State; the D2H leg runs beside the next steps */
    return c->diag_ring.ship(c, d, c->stream, c->diag_slot_bytes, 0);
}

/* the same kernel into the caller's device buffers: no slot, no copy to the host; the caller's stream waits for the kernel */
PX_EXPORT int32_t picles_diag_export(picles_ctx *c, void *fields_dev, double *partials_dev, void *caller_stream)
{
    if (!c) return -1;
    if (!c->diag_ring.cap) return fail(c, -2, "picles_diag_init first");
    if (!fields_dev) return fail(c, -2, "picles_diag_export: no device buffer for the fields");
    HIPCHK(c, hipSetDevice(c->device));
    if (!partials_dev) {      /* the kernel writes its partials somewhere: a block of the context's own, made on first use */
        if (!c->diag_scratch) HIPCHK(c, hipMalloc(&c->diag_scratch, (size_t)c->diag_npart * 7 * 8));
        partials_dev = c->diag_scratch;
    }
    if (caller_stream) {      /* whatever the caller still has reading or writing its buffers comes first */
        HIPCHK(c, hipEventRecord(c->ev_ctx, (hipStream_t)caller_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ctx, 0));
    }
    { int rc = diag_run(c, (float *)fields_dev, partials_dev); if (rc) return rc; }
    if (caller_stream) {
        HIPCHK(c, hipEventRecord(c->ev_ctx, c->stream));
        HIPCHK(c, hipStreamWaitEvent((hipStream_t)caller_stream, c->ev_ctx, 0));
    }
    return 0;
}

PX_EXPORT int32_t picles_diag_pop(picles_ctx *c, void *fields, double *partials, double *time)
{
    if (!c || !fields) return -1;
    if (!c->diag_ring.count) return fail(c, -3, "no diagnostics snapshot pending");
    HIPCHK(c, hipSetDevice(c->device));
    OutRing::Slot s;
    { int rc = c->diag_ring.front(c, s); if (rc) return rc; }
    memcpy(fields, s.host, c->diag_field_bytes);
    if (partials) memcpy(partials, s.host + c->diag_part_off, (size_t)c->diag_npart * 7 * 8);
    if (time) *time = s.time;
    c->diag_ring.drop();
    return 0;
}

/* ---- coupling fluxes (the definition: include/picles_hip.h, "coupling fluxes"; the node and the kernel: k_flux.h) ---- */
PX_EXPORT int32_t picles_flux_init(picles_ctx *c, int32_t cx, int32_t cy, int32_t field_mask, double scale_phi, double scale_tau, int32_t n_slots)
{
    if (!c) return -1;
    if (cx < 1 || cx > 16 || cy < 1 || cy > 16) return fail(c, -2, "picles_flux_init: coarsening factors must be 1 ... 16");
    if (field_mask <= 0 || (field_mask & ~PICLES_FLUX_ALL)) return fail(c, -2, "picles_flux_init: empty or unknown field mask");
    if (!(std::isfinite(scale_phi) && scale_phi > 0.0 && std::isfinite(scale_tau) && scale_tau > 0.0))
        return fail(c, -2, "picles_flux_init: scale_phi and scale_tau must be finite and positive");
    if (n_slots < 1) return fail(c, -2, "picles_flux_init: n_slots must be >= 1");
    if (c->flux_ring.cap) return fail(c, -2, "picles_flux_init: the flux set is already initialised (picles_flux_free first)");
    if (c->G.j_begin % cy != 0) return fail(c, -2, "picles_flux_init: the slab's j_begin must be a multiple of cy (coarse cells are global)");
    HIPCHK(c, hipSetDevice(c->device));
    FluxP F{};
    F.Nx = c->G.Nx; F.ny_loc = c->G.ny_loc; F.cx = cx; F.cy = cy;
    F.Nxc = (c->G.Nx + cx - 1) / cx; F.nyc_loc = (c->G.ny_loc + cy - 1) / cy;
    F.tiles_per_row = (F.Nxc + DIAG_TILE - 1) / DIAG_TILE;
    F.mask = (unsigned)field_mask; F.scale_phi = scale_phi; F.scale_tau = scale_tau; F.plane = c->A.n;
    const int nf = __builtin_popcount((unsigned)field_mask), np = F.nyc_loc * F.tiles_per_row;
    const size_t fb = (size_t)4 * F.Nxc * F.nyc_loc * nf, po = (fb + 15) & ~(size_t)15, sb = po + (size_t)np * FLUX_NP * 8;
    { int rc = c->flux_ring.init(c, n_slots, sb); if (rc) return rc; }
    c->flux = F; c->flux_nfields = nf; c->flux_npart = np;
    c->flux_field_bytes = fb; c->flux_part_off = po; c->flux_slot_bytes = sb;
    return 0;
}

PX_EXPORT int32_t picles_flux_shape(const picles_ctx *c, int32_t *nxc, int32_t *nyc_loc, int32_t *n_fields, int32_t *n_partials, size_t *bytes)
{
    if (!c || !c->flux_ring.cap) return -1;
    if (nxc) *nxc = c->flux.Nxc;
    if (nyc_loc) *nyc_loc = c->flux.nyc_loc;
    if (n_fields) *n_fields = c->flux_nfields;
    if (n_partials) *n_partials = c->flux_npart;
    if (bytes) *bytes = c->flux_field_bytes;
    return 0;
}

PX_EXPORT int32_t picles_flux_pending(const picles_ctx *c) { return c ? c->flux_ring.count : -1; }

/* the wind rule: the level planes the window holds at the clock; a lattice or streamed context whose window holds none samples the
 * level at the clock (k_wind_sample<1>, the sampler of its windows: a function of the time alone); a host-set window refuses with a
 * text that names the remedy — before anything is launched (the flush of a pending step included: it changes neither the window nor
 * the clock) */
static int flux_wind(picles_ctx *c, const char *who, const double *&u, const double *&v, hipStream_t s = nullptr)
{
    if (!s) s = c->stream;
    if (c->wind.level_at(c->A, c->clock, u, v)) return 0;
    if (c->wind.from_lattice()) {      /* the device has the source: the level at the clock itself, into the spare pair */
        HIPCHK(c, hipSetDevice(c->device));
        return c->wind.sample_spare(c, c->clock, who, s, u, v);
    }
    char buf[400];
    snprintf(buf, sizeof buf, "%s: the wind window [%.17g, %.17g] holds no level at the clock %.17g, and nothing is interpolated: step to a "
             "level (the end of a model step is one), or set the window (picles_set_winds*) so that it starts or ends at the clock",
             who, c->wind.t0, c->wind.t1, c->clock);
    return fail(c, -2, buf);
}

template <int CX, bool VEC>
static void flux_launch(picles_ctx *c, const double *u, const double *v, float *fields, double *partials)
{
    hipLaunchKernelGGL((k_flux<CX, VEC>), dim3((unsigned)c->flux_npart), dim3(DIAG_TILE), 0, c->stream, c->P, c->flux, (const double *)c->A.state,
                       u, v, fields, partials);
}

/* State at the step boundary, then the kernel on the context stream into (fields, partials): a ring slot (push) or the caller's
 * device buffers (export).  (u, v): the planes flux_wind found */
static int flux_run(picles_ctx *c, const double *u, const double *v, float *fields, double *partials)
{
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());   /* an un-fused slab step leaves its scatter on the ring's stream M */
    /* 16-byte loads: every cell's row segment starts on a 16-byte boundary of each of the five planes */
    const bool vec = (c->flux.Nx & 1) == 0 && (c->A.n & 1) == 0 && (((uintptr_t)c->A.state | (uintptr_t)u | (uintptr_t)v) & 15u) == 0;
    timing_begin(c, c->stream, 4);      /* other_ms of picles_get_timing: the slot k_diag and the checkpoint kernel share (a kernel trace tells them apart) */
    switch (c->flux.cx) {
    case 1: flux_launch<1, false>(c, u, v, fields, partials); break;
    case 2: if (vec) flux_launch<2, true>(c, u, v, fields, partials); else flux_launch<2, false>(c, u, v, fields, partials); break;
    case 4: if (vec) flux_launch<4, true>(c, u, v, fields, partials); else flux_launch<4, false>(c, u, v, fields, partials); break;
    default: flux_launch<0, false>(c, u, v, fields, partials);
    }
    timing_end(c, c->stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}

PX_EXPORT int32_t picles_flux_push(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->flux_ring.cap) return fail(c, -2, "picles_flux_init first");
    unsigned char *d = c->flux_ring.next_slot();
    if (!d) return fail(c, -3, "flux ring full: pop first");
    const double *u, *v;
    { int rc = flux_wind(c, "picles_flux_push", u, v); if (rc) return rc; }
    { int rc = flux_run(c, u, v, (float *)d, (double *)(d + c->flux_part_off)); if (rc) return rc; }
    /* stream-ordered behind the step that produced State; the D2H leg runs beside the next steps */
    return c->flux_ring.ship(c, d, c->stream, c->flux_slot_bytes, 0);
}

/* the same kernel into the caller's device buffers: no slot, no copy to the host; the caller's stream waits for the kernel */
PX_EXPORT int32_t picles_flux_export(picles_ctx *c, void *fields_dev, double *partials_dev, void *caller_stream)
{
    if (!c) return -1;
    if (!c->flux_ring.cap) return fail(c, -2, "picles_flux_init first");
    if (!fields_dev) return fail(c, -2, "picles_flux_export: no device buffer for the fields");
    const double *u, *v;
    { int rc = flux_wind(c, "picles_flux_export", u, v); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    if (!partials_dev) {      /* the kernel writes its partials somewhere: a block of the context's own, made on first use */
        if (!c->flux_scratch) HIPCHK(c, hipMalloc(&c->flux_scratch, (size_t)c->flux_npart * FLUX_NP * 8));
        partials_dev = c->flux_scratch;
    }
    if (caller_stream) {      /* whatever the caller still has reading or writing its buffers comes first */
        HIPCHK(c, hipEventRecord(c->ev_ctx, (hipStream_t)caller_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ctx, 0));
    }
    { int rc = flux_run(c, u, v, (float *)fields_dev, partials_dev); if (rc) return rc; }
    if (caller_stream) {
        HIPCHK(c, hipEventRecord(c->ev_ctx, c->stream));
        HIPCHK(c, hipStreamWaitEvent((hipStream_t)caller_stream, c->ev_ctx, 0));
    }
    return 0;
}

PX_EXPORT int32_t picles_flux_pop(picles_ctx *c, void *fields, double *partials, double *time)
{
    if (!c || !fields) return -1;
    if (!c->flux_ring.count) return fail(c, -3, "no flux snapshot pending");
    HIPCHK(c, hipSetDevice(c->device));
    OutRing::Slot s;
    { int rc = c->flux_ring.front(c, s); if (rc) return rc; }
    memcpy(fields, s.host, c->flux_field_bytes);
    if (partials) memcpy(partials, s.host + c->flux_part_off, (size_t)c->flux_npart * FLUX_NP * 8);
    if (time) *time = s.time;
    c->flux_ring.drop();
    return 0;
}

/* the set goes, with whatever is still pending: the kernel and the copies that use the slots are waited for first */
PX_EXPORT int32_t picles_flux_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->flux_ring.cap) return fail(c, -2, "picles_flux_init first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->store_stream) HIPCHK(c, hipStreamSynchronize(c->store_stream));
    if (c->fm_on) {      /* the mean set takes its cells from this one: it goes with it */
        HIPCHK(c, hipDeviceSynchronize());
        flux_mean_release(c);
    }
    c->flux_ring.release();
    if (c->flux_scratch) { hipFree(c->flux_scratch); c->flux_scratch = nullptr; }
    c->flux = FluxP{};
    c->flux_nfields = c->flux_npart = 0;
    c->flux_field_bytes = c->flux_part_off = c->flux_slot_bytes = 0;
    return 0;
}

/* ---- station probes (the contract: include/picles_hip.h; the kernel: k_probe.h) ---- */
/* would the samples of the next n_steps steps overrun the ring?  Asked by the step entry points before they change anything */
static int probe_room(picles_ctx *c, long long n_steps, const char *who)
{
    if (!c->probe_n) return 0;
    const long long due = c->probe_cad.due_within(n_steps);
    if (due && c->probe.count + due > c->probe.cap)
        return fail(c, PICLES_PROBE_E_FULL, std::string(who) + ": probe ring full (" + std::to_string(c->probe.count) + " samples pending, " +
                                            std::to_string(due) + " due, capacity " + std::to_string(c->probe.cap) + "): picles_probe_pop first");
    return 0;
}

/* State of context c at n nodes (device list: the i plane, then the local-row plane) into 3 planes of n doubles at `out`, on stream
 * s — which the caller has ordered behind everything the values depend on.  With a fused step pending they come from its records,
 * with the arrays and reach indices flush() would hand k_scatter at this point; otherwise from State.  Neither the pending step
 * nor any plane of the model is touched; the host does not wait.  Errors are reported on `err`: c, or the context whose call this is */
static int probe_launch(picles_ctx *err, picles_ctx *c, hipStream_t s, int n, const int *nodes, double *out)
{
    const dim3 grid(nblocks(n, PROBE_BLOCK)), block(PROBE_BLOCK);
    if (c->pending)
        hipLaunchKernelGGL(k_probe<true>, grid, block, 0, s, c->G, arrays_for(c, c->cur, c->cur), n, nodes, out);
    else
        hipLaunchKernelGGL(k_probe<false>, grid, block, 0, s, c->G, c->A, n, nodes, out);
    HIPCHK(err, hipGetLastError());
    return 0;
}

/* one sample into the next ring slot */
static int probe_take(picles_ctx *c, hipStream_t s)
{
    unsigned char *slot = c->probe.next_slot();
    if (!slot) return fail(c, PICLES_PROBE_E_FULL, "probe ring full: picles_probe_pop first");
    { int rc = probe_launch(c, c, s, c->probe_n, c->probe_nodes, (double *)slot); if (rc) return rc; }
    return c->probe.ship(c, slot, s, (size_t)3 * c->probe_n * sizeof(double), c->probe_cad.steps);
}

static void probe_release(picles_ctx *c)
{
    if (c->probe_nodes) hipFree(c->probe_nodes);
    c->probe_nodes = nullptr;
    c->probe.release();
    c->probe_n = 0;
    c->probe_cad = Cadence{};
}

PX_EXPORT int32_t picles_probe_init(picles_ctx *c, int32_t n, const int32_t *ij, int32_t every, int32_t first, int32_t capacity)
{
    if (!c) return -1;
    if (c->probe_n) return fail(c, -2, "picles_probe_init: a probe set exists (picles_probe_free first)");
    if (n < 1 || !ij) return fail(c, -2, "picles_probe_init: n must be >= 1 and the node list given");
    if (every < 1 || first < 1 || capacity < 1) return fail(c, -2, "picles_probe_init: every, first and capacity must be >= 1");
    const GridP &G = c->G;
    std::vector<int> loc((size_t)2 * n);
    for (int k = 0; k < n; k++) {
        const int i = ij[k], j = ij[(size_t)n + k];
        if (i < 0 || i >= G.Nx || j < G.j_begin || j >= G.j_begin + G.ny_loc)
            return fail(c, -2, "picles_probe_init: node " + std::to_string(k) + " = (" + std::to_string(i) + ", " + std::to_string(j) +
                                   ") lies outside [0, Nx) x [j_begin, j_end)");
        loc[k] = i;
        loc[(size_t)n + k] = j - G.j_begin;
    }
    HIPCHK(c, hipSetDevice(c->device));
    Undo undo{[c] { probe_release(c); }};
    { int rc = c->probe.init(c, capacity, (size_t)3 * n * sizeof(double)); if (rc) return rc; }
    HIPCHK(c, hipMalloc(&c->probe_nodes, (size_t)2 * n * sizeof(int)));
    HIPCHK(c, hipMemcpy(c->probe_nodes, loc.data(), (size_t)2 * n * sizeof(int), hipMemcpyHostToDevice));     /* blocking: loc dies here */
    c->probe_cad = Cadence{every, first, 0};
    c->probe_n = n;
    undo.armed = false;
    return 0;
}

PX_EXPORT int32_t picles_probe_shape(const picles_ctx *c, int32_t *n, int32_t *every, int32_t *capacity)
{
    if (!c || !c->probe_n) return -1;
    if (n) *n = c->probe_n;
    if (every) *every = c->probe_cad.every;
    if (capacity) *capacity = c->probe.cap;
    return 0;
}

PX_EXPORT int32_t picles_probe_pending(const picles_ctx *c) { return c ? c->probe.count : -1; }

PX_EXPORT int32_t picles_probe_sample(picles_ctx *c, void *stream)
{
    if (!c) return -1;
    if (!c->probe_n) return fail(c, -2, "picles_probe_init first");
    if (!c->probe.next_slot()) return fail(c, PICLES_PROBE_E_FULL, "picles_probe_sample: probe ring full: picles_probe_pop first");
    HIPCHK(c, hipSetDevice(c->device));
    return probe_take(c, stream ? (hipStream_t)stream : c->stream);
}

PX_EXPORT int32_t picles_probe_pop(picles_ctx *c, int32_t max_samples, double *values, double *times, int64_t *steps, int32_t *n_out)
{
    if (!c) return -1;
    if (n_out) *n_out = 0;
    if (!c->probe_n) return fail(c, -2, "picles_probe_init first");
    if (max_samples < 1 || !values || !n_out) return fail(c, -2, "picles_probe_pop: max_samples must be >= 1, values and n_out given");
    if (!c->probe.count) return fail(c, -3, "no probe sample pending");
    HIPCHK(c, hipSetDevice(c->device));
    const int m = max_samples < c->probe.count ? max_samples : c->probe.count;
    const size_t sample = (size_t)3 * c->probe_n;
    for (int k = 0; k < m; k++) {
        OutRing::Slot s;
        { int rc = c->probe.front(c, s); if (rc) return rc; }      /* this sample's copy alone: later steps stay enqueued */
        memcpy(values + (size_t)k * sample, s.host, sample * sizeof(double));
        if (times) times[k] = s.time;
        if (steps) steps[k] = (int64_t)s.step;
        c->probe.drop();
        *n_out = k + 1;
    }
    return 0;
}

PX_EXPORT int32_t picles_probe_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->probe_n) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());       /* probe launches and copies in flight read and write the buffers about to go */
    probe_release(c);
    return 0;
}

/* ---- track samples (the contract: include/picles_hip.h; the kernel: k_track.h) ---- */
struct Track {
    int m = 0;
    double H = 0.0;                                /* the horizon: the longest step taken while the set lives */
    long long samples = 0;                         /* samples taken, those that visited no event included */
    std::vector<double> t;                         /* host copy of the event times: the range of a sample is found here */
    double *d_t = nullptr, *d_w = nullptr, *table = nullptr;      /* device: m times, 4 m weights, the 8 planes of m */
    int *d_ij = nullptr;                           /* device: 8 planes of m, i of the four corners, then their row */
    /* the fetch: a device block the range is gathered into on the context stream, its pinned twin, the ring's two events */
    double *stage_dev = nullptr, *stage_host = nullptr;
    size_t stage_cap = 0;                          /* doubles either block holds */
    hipEvent_t ready = nullptr, done = nullptr;
    bool open = false;
    int fetch_n = 0;
};

/* is a step of dt allowed under the set's horizon?  Asked by the step entry points before they change anything */
static int track_step_ok(picles_ctx *c, double dt, const char *who)
{
    if (!c->trk || !(dt > c->trk->H)) return 0;
    return fail(c, -2, std::string(who) + ": a step of " + std::to_string(dt) + " s is longer than the horizon of the track set (" +
                           std::to_string(c->trk->H) + " s): events between two samples would be missed");
}

/* one sample at the clock as it stands, on stream s: the events with T - H < t_k < T + H, a contiguous range of the sorted times.
 * probe_launch's choice between the records of a pending fused step and State; nothing of the model is touched, the host does not wait */
static int track_take(picles_ctx *c, hipStream_t s)
{
    Track *K = c->trk;
    const double T = c->clock, lo = T - K->H, hi = T + K->H;
    const int k0 = (int)(std::upper_bound(K->t.begin(), K->t.end(), lo) - K->t.begin());      /* the first t_k > T - H */
    const int k1 = (int)(std::lower_bound(K->t.begin(), K->t.end(), hi) - K->t.begin());      /* the first t_k >= T + H */
    K->samples++;
    if (k1 <= k0) return 0;
    const dim3 grid(nblocks(4LL * (k1 - k0), TRACK_BLOCK)), block(TRACK_BLOCK);
    if (c->pending)
        hipLaunchKernelGGL(k_track<true>, grid, block, 0, s, c->G, arrays_for(c, c->cur, c->cur), k0, k1, K->m, T, (const double *)K->d_t,
                           (const int *)K->d_ij, (const double *)K->d_w, K->table);
    else
        hipLaunchKernelGGL(k_track<false>, grid, block, 0, s, c->G, c->A, k0, k1, K->m, T, (const double *)K->d_t, (const int *)K->d_ij,
                           (const double *)K->d_w, K->table);
    HIPCHK(c, hipGetLastError());
    return 0;
}

static void track_release(picles_ctx *c)
{
    Track *K = c->trk;
    if (!K) return;
    if (K->d_t) hipFree(K->d_t);
    if (K->d_w) hipFree(K->d_w);
    if (K->d_ij) hipFree(K->d_ij);
    if (K->table) hipFree(K->table);
    if (K->stage_dev) hipFree(K->stage_dev);
    if (K->stage_host) hipHostFree(K->stage_host);
    if (K->ready) hipEventDestroy(K->ready);
    if (K->done) hipEventDestroy(K->done);
    delete K;
    c->trk = nullptr;
}

PX_EXPORT int32_t picles_track_init(picles_ctx *c, int32_t m, const double *t, const int32_t *ij, const double *w, double horizon)
{
    if (!c) return -1;
    if (c->trk) return fail(c, -2, "picles_track_init: a track set exists (picles_track_free first)");
    const GridP &G = c->G;
    if (!G.single_slab || c->ring || G.j_begin > 0 || G.ny_loc < G.Ny)
        return fail(c, -5, "picles_track_init: track samples need a whole-grid context (no slab, no slab mode, no native ring): the corners of an event may lie on two slabs");
    if (m < 1 || !t || !ij || !w) return fail(c, -2, "picles_track_init: m must be >= 1 and times, corners and weights given");
    if ((long long)m * 8 > (long long)INT32_MAX) return fail(c, -2, "picles_track_init: 8 m must not exceed INT32_MAX");
    if (!std::isfinite(horizon) || !(horizon > 0.0)) return fail(c, -2, "picles_track_init: the horizon must be finite and positive");
    for (int k = 0; k < m; k++)
        if (!std::isfinite(t[k]) || (k > 0 && t[k] < t[k - 1]))
            return fail(c, -2, "picles_track_init: event " + std::to_string(k) + ": times must be finite and nondecreasing");
    for (int q = 0; q < 4; q++)
        for (int k = 0; k < m; k++) {
            const int i = ij[(size_t)q * m + k], j = ij[(size_t)(4 + q) * m + k];
            if (i < 0 || i >= G.Nx || j < 0 || j >= G.Ny)
                return fail(c, -2, "picles_track_init: event " + std::to_string(k) + ", corner " + std::to_string(q) + " = (" + std::to_string(i) +
                                       ", " + std::to_string(j) + ") lies outside the grid");
            const double wk = w[(size_t)q * m + k];
            if (!std::isfinite(wk) || wk < 0.0)
                return fail(c, -2, "picles_track_init: event " + std::to_string(k) + ", corner " + std::to_string(q) + ": weights must be finite and >= 0");
        }
    HIPCHK(c, hipSetDevice(c->device));
    Track *K = new Track();
    c->trk = K;
    Undo undo{[c] { track_release(c); }};
    { int rc = store_stream_get(c); if (rc) return rc; }
    const size_t M = (size_t)m;
    HIPCHK(c, hipMalloc(&K->d_t, M * sizeof(double)));
    HIPCHK(c, hipMalloc(&K->d_ij, 8 * M * sizeof(int)));
    HIPCHK(c, hipMalloc(&K->d_w, 4 * M * sizeof(double)));
    HIPCHK(c, hipMalloc(&K->table, 8 * M * sizeof(double)));
    HIPCHK(c, hipEventCreateWithFlags(&K->ready, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&K->done, hipEventDisableTiming));
    /* blocking uploads: the caller's arrays are free on return (whole-grid context: a global row is the local row) */
    HIPCHK(c, hipMemcpy(K->d_t, t, M * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(K->d_ij, ij, 8 * M * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(K->d_w, w, 4 * M * sizeof(double), hipMemcpyHostToDevice));
    /* every entry NaN: a double of all-one bits is one.  Complete on return, whatever stream the first sample rides */
    HIPCHK(c, hipMemsetAsync(K->table, 0xFF, 8 * M * sizeof(double), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    K->t.assign(t, t + m);
    K->m = m;
    K->H = horizon;
    undo.armed = false;
    return 0;
}

PX_EXPORT int32_t picles_track_info(const picles_ctx *c, int32_t *m, double *horizon, int64_t *samples_taken)
{
    if (!c || !c->trk) { if (m) *m = -1; return -1; }
    if (m) *m = c->trk->m;
    if (horizon) *horizon = c->trk->H;
    if (samples_taken) *samples_taken = (int64_t)c->trk->samples;
    return 0;
}

PX_EXPORT int32_t picles_track_sample(picles_ctx *c, void *stream)
{
    if (!c) return -1;
    if (!c->trk) return fail(c, -2, "picles_track_init first");
    HIPCHK(c, hipSetDevice(c->device));
    return track_take(c, stream ? (hipStream_t)stream : c->stream);
}

PX_EXPORT int32_t picles_track_fetch_begin(picles_ctx *c, int32_t k0, int32_t n)
{
    if (!c) return -1;
    Track *K = c->trk;
    if (!K) return fail(c, -2, "picles_track_init first");
    if (K->open) return fail(c, -2, "picles_track_fetch_begin: a fetch is open (picles_track_fetch_end first)");
    if (k0 < 0 || n < 1 || (long long)k0 + n > (long long)K->m)
        return fail(c, -2, "picles_track_fetch_begin: events [" + std::to_string(k0) + ", " + std::to_string((long long)k0 + n) + ") lie outside [0, " +
                               std::to_string(K->m) + ")");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t need = (size_t)8 * n;
    if (need > K->stage_cap) {      /* grown lazily; no copy is in flight: the last fetch was ended */
        if (K->stage_dev) hipFree(K->stage_dev);
        if (K->stage_host) hipHostFree(K->stage_host);
        K->stage_dev = K->stage_host = nullptr;
        K->stage_cap = 0;
        HIPCHK(c, hipMalloc(&K->stage_dev, need * sizeof(double)));
        HIPCHK(c, hipHostMalloc(&K->stage_host, need * sizeof(double), hipHostMallocDefault));
        K->stage_cap = need;
    }
    /* the range as it is at this point of the context stream, gathered into the staging block behind the samples enqueued so far;
     * the leg to the host rides the store stream beside whatever is enqueued next (samples that rewrite the table included) */
    for (int p = 0; p < 8; p++)
        HIPCHK(c, hipMemcpyAsync(K->stage_dev + (size_t)p * n, K->table + (size_t)p * K->m + k0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    { int rc = ship_d2h(c, c->stream, K->ready, K->done, K->stage_host, K->stage_dev, need * sizeof(double)); if (rc) return rc; }
    K->fetch_n = n;
    K->open = true;
    return 0;
}

PX_EXPORT int32_t picles_track_fetch_end(picles_ctx *c, double *out)
{
    if (!c) return -1;
    Track *K = c->trk;
    if (!K) return fail(c, -2, "picles_track_init first");
    if (!K->open) return fail(c, -2, "picles_track_fetch_end: no fetch is open (picles_track_fetch_begin first)");
    if (!out) return fail(c, -2, "picles_track_fetch_end: out must be given");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(K->done));      /* this copy alone: later steps stay enqueued */
    memcpy(out, K->stage_host, (size_t)8 * K->fetch_n * sizeof(double));
    K->open = false;
    return 0;
}

PX_EXPORT int32_t picles_track_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->trk) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());       /* samples and copies in flight read and write the buffers about to go */
    track_release(c);
    return 0;
}

/* ---- run statistics (the contract: include/picles_hip.h; the kernel: k_stat.h) ---- */
static inline int stat_nf64(const StatP &S) { return ((S.mask & PICLES_STAT_PEAK) ? 4 : 0) + ((S.mask & PICLES_STAT_MEAN) ? 4 : 0); }
static inline int stat_nu32(const StatP &S) { return 1 + ((S.mask & PICLES_STAT_EXCEED) ? S.nthr : 0); }

/* the planes of the groups in `mask` (a subset of the set's; n_wet always), in the order of the device block: offset and bytes of
 * each contiguous piece */
static int stat_pieces(const picles_ctx *c, unsigned mask, size_t off[4], size_t len[4])
{
    const size_t N = (size_t)c->A.n;
    const bool peak = c->stat.mask & PICLES_STAT_PEAK;
    const size_t u32_0 = (size_t)stat_nf64(c->stat) * N * 8;
    int n = 0;
    if (mask & PICLES_STAT_PEAK) { off[n] = 0; len[n++] = 4 * N * 8; }
    if (mask & PICLES_STAT_MEAN) { off[n] = peak ? 4 * N * 8 : 0; len[n++] = 4 * N * 8; }
    off[n] = u32_0; len[n++] = N * 4;
    if (mask & PICLES_STAT_EXCEED) { off[n] = u32_0 + N * 4; len[n++] = (size_t)c->stat.nthr * N * 4; }
    return n;
}

/* an operation on the planes, on stream s: behind the latest one wherever that ran */
static int stat_order(picles_ctx *c, hipStream_t s)
{
    if (c->stat_ev_live && c->stat_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->stat_ev, 0));
    return 0;
}
static int stat_mark(picles_ctx *c, hipStream_t s)
{
    HIPCHK(c, hipEventRecord(c->stat_ev, s));
    c->stat_stream = s;
    c->stat_ev_live = true;
    return 0;
}

/* one update, on stream s — the stream behind which everything the sample depends on has been ordered.  With a fused step pending
 * the samples come from its records, with the arrays and reach indices flush() would hand k_scatter at this moment (probe_take) */
static int stat_update(picles_ctx *c, hipStream_t s)
{
    { int rc = stat_order(c, s); if (rc) return rc; }
    const size_t N = (size_t)c->A.n;
    double *f64 = (double *)c->stat_dev;
    double *peak = (c->stat.mask & PICLES_STAT_PEAK) ? f64 : nullptr;
    double *mean = (c->stat.mask & PICLES_STAT_MEAN) ? f64 + (peak ? 4 * N : 0) : nullptr;
    unsigned int *n_wet = (unsigned int *)(c->stat_dev + (size_t)stat_nf64(c->stat) * N * 8);
    unsigned int *n_exc = (c->stat.mask & PICLES_STAT_EXCEED) ? n_wet + N : nullptr;
    const dim3 grid(nblocks(c->A.n, PICLES_BLOCK)), block(PICLES_BLOCK);
    if (c->pending)
        hipLaunchKernelGGL(k_stat<true>, grid, block, 0, s, c->G, arrays_for(c, c->cur, c->cur), c->stat, c->clock, n_wet, peak, mean, n_exc);
    else
        hipLaunchKernelGGL(k_stat<false>, grid, block, 0, s, c->G, c->A, c->stat, c->clock, n_wet, peak, mean, n_exc);
    HIPCHK(c, hipGetLastError());
    { int rc = stat_mark(c, s); if (rc) return rc; }
    if (c->stat_samples == 0) c->stat_t_first = c->clock;
    c->stat_t_last = c->clock;
    c->stat_samples++;
    return 0;
}

static void stat_release(picles_ctx *c)
{
    if (c->stat_dev) hipFree(c->stat_dev);
    if (c->stat_ev) hipEventDestroy(c->stat_ev);
    c->stat_dev = nullptr; c->stat_ev = nullptr; c->stat_stream = nullptr; c->stat_ev_live = false;
    c->stat_on = false; c->stat = StatP{}; c->stat_bytes = 0;
    c->stat_cad = Cadence{};
    c->stat_samples = 0; c->stat_t_first = 0.0; c->stat_t_last = 0.0;
}

PX_EXPORT int32_t picles_stat_init(picles_ctx *c, int32_t group_mask, int32_t n_thresholds, const double *thresholds, int32_t every,
                                   int32_t first)
{
    if (!c) return -1;
    if (c->stat_on) return fail(c, -2, "picles_stat_init: a statistics set exists (picles_stat_free first)");
    if (group_mask <= 0 || (group_mask & ~PICLES_STAT_ALL)) return fail(c, -2, "picles_stat_init: empty or unknown group mask");
    if (every < 1 || first < 1) return fail(c, -2, "picles_stat_init: every and first must be >= 1");
    if (group_mask & PICLES_STAT_EXCEED) {
        if (n_thresholds < 1 || n_thresholds > STAT_MAX_THR || !thresholds)
            return fail(c, -2, "picles_stat_init: PICLES_STAT_EXCEED takes 1 ... 4 thresholds");
        for (int k = 0; k < n_thresholds; k++)
            if (!std::isfinite(thresholds[k]) || !(thresholds[k] > 0.0) || (k > 0 && !(thresholds[k] > thresholds[k - 1])))
                return fail(c, -2, "picles_stat_init: thresholds must be finite, positive and strictly ascending");
    } else if (n_thresholds != 0) {
        return fail(c, -2, "picles_stat_init: thresholds given without PICLES_STAT_EXCEED");
    }
    HIPCHK(c, hipSetDevice(c->device));
    StatP S{};
    S.mask = (unsigned)group_mask;
    S.nthr = n_thresholds;
    for (int k = 0; k < n_thresholds; k++) S.thr[k] = thresholds[k];
    const size_t bytes = (size_t)c->A.n * ((size_t)stat_nf64(S) * 8 + (size_t)stat_nu32(S) * 4);
    Undo undo{[c] { stat_release(c); }};
    { int rc = store_stream_get(c); if (rc) return rc; }
    HIPCHK(c, hipMalloc(&c->stat_dev, bytes));
    HIPCHK(c, hipEventCreateWithFlags(&c->stat_ev, hipEventDisableTiming));
    HIPCHK(c, hipMemsetAsync(c->stat_dev, 0, bytes, c->stream));
    c->stat = S; c->stat_bytes = bytes;
    { int rc = stat_mark(c, c->stream); if (rc) return rc; }
    c->stat_cad = Cadence{every, first, 0};
    c->stat_samples = 0; c->stat_t_first = 0.0; c->stat_t_last = 0.0;
    c->stat_on = true;
    undo.armed = false;
    return 0;
}

PX_EXPORT int32_t picles_stat_shape(const picles_ctx *c, int32_t *group_mask, int32_t *n_thresholds, double *thresholds, int32_t *every,
                                    int32_t *n_planes, size_t *bytes)
{
    if (!c || !c->stat_on) return -1;
    if (group_mask) *group_mask = (int32_t)c->stat.mask;
    if (n_thresholds) *n_thresholds = c->stat.nthr;
    if (thresholds) for (int k = 0; k < c->stat.nthr; k++) thresholds[k] = c->stat.thr[k];
    if (every) *every = c->stat_cad.every;
    if (n_planes) *n_planes = stat_nf64(c->stat) + stat_nu32(c->stat);
    if (bytes) *bytes = c->stat_bytes;
    return 0;
}

PX_EXPORT int32_t picles_stat_update(picles_ctx *c, void *stream)
{
    if (!c) return -1;
    if (!c->stat_on) return fail(c, -2, "picles_stat_init first");
    HIPCHK(c, hipSetDevice(c->device));
    if (stream) c->ext_streams = true;
    return stat_update(c, stream ? (hipStream_t)stream : c->stream);
}

static int stat_mask_ok(picles_ctx *c, int32_t group_mask, const char *who)
{
    if (group_mask < 0 || (group_mask & ~(int32_t)c->stat.mask))
        return fail(c, -2, std::string(who) + ": group mask is no subset of the set's");
    return 0;
}

PX_EXPORT int32_t picles_stat_get(picles_ctx *c, int32_t group_mask, void *planes, int64_t *n_samples, double *t_first, double *t_last)
{
    if (!c) return -1;
    if (!c->stat_on) return fail(c, -2, "picles_stat_init first");
    if (!planes) return fail(c, -2, "picles_stat_get: planes must be given");
    { int rc = stat_mask_ok(c, group_mask, "picles_stat_get"); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    /* the latest operation on the planes alone: the copy rides the store stream behind its event; a pending step stays pending */
    HIPCHK(c, hipStreamWaitEvent(c->store_stream, c->stat_ev, 0));
    size_t off[4], len[4], at = 0;
    const int n = stat_pieces(c, (unsigned)group_mask, off, len);
    for (int k = 0; k < n; k++) {
        HIPCHK(c, hipMemcpyAsync((unsigned char *)planes + at, c->stat_dev + off[k], len[k], hipMemcpyDeviceToHost, c->store_stream));
        at += len[k];
    }
    HIPCHK(c, hipStreamSynchronize(c->store_stream));      /* the caller's (pageable) buffer is complete and released */
    if (n_samples) *n_samples = (int64_t)c->stat_samples;
    if (t_first) *t_first = c->stat_t_first;
    if (t_last) *t_last = c->stat_t_last;
    return 0;
}

PX_EXPORT int32_t picles_stat_set(picles_ctx *c, int32_t group_mask, const void *planes, int64_t n_samples, double t_first, double t_last)
{
    if (!c) return -1;
    if (!c->stat_on) return fail(c, -2, "picles_stat_init first");
    if (!planes) return fail(c, -2, "picles_stat_set: planes must be given");
    if (n_samples < 0) return fail(c, -2, "picles_stat_set: n_samples must be >= 0");
    { int rc = stat_mask_ok(c, group_mask, "picles_stat_set"); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = stat_order(c, c->stream); if (rc) return rc; }
    size_t off[4], len[4], at = 0;
    const int n = stat_pieces(c, (unsigned)group_mask, off, len);
    for (int k = 0; k < n; k++) {
        HIPCHK(c, hipMemcpyAsync(c->stat_dev + off[k], (const unsigned char *)planes + at, len[k], hipMemcpyHostToDevice, c->stream));
        at += len[k];
    }
    { int rc = stat_mark(c, c->stream); if (rc) return rc; }
    HIPCHK(c, hipEventSynchronize(c->stat_ev));            /* the caller's buffer has been read to its last byte */
    c->stat_samples = (long long)n_samples; c->stat_t_first = t_first; c->stat_t_last = t_last;
    return 0;
}

PX_EXPORT int32_t picles_stat_reset(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->stat_on) return fail(c, -2, "picles_stat_init first");
    HIPCHK(c, hipSetDevice(c->device));
    /* in stream order behind the updates already issued, wherever they ran; no host synchronisation */
    hipStream_t s = c->stream;
    { int rc = stat_order(c, s); if (rc) return rc; }
    HIPCHK(c, hipMemsetAsync(c->stat_dev, 0, c->stat_bytes, s));
    { int rc = stat_mark(c, s); if (rc) return rc; }
    c->stat_samples = 0; c->stat_t_first = 0.0; c->stat_t_last = 0.0;
    return 0;
}

PX_EXPORT int32_t picles_stat_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->stat_on) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());       /* updates in flight read and write the planes about to go */
    stat_release(c);
    return 0;
}

/* ---- flux means (the contract: include/picles_hip.h, "flux means"; the kernels: k_flux_mean.h) ---- */
/* an operation on the accumulators, on stream s: behind the latest one wherever that ran */
static int flux_mean_order(picles_ctx *c, hipStream_t s)
{
    if (c->fm_ev_live && c->fm_stream != s) HIPCHK(c, hipStreamWaitEvent(s, c->fm_ev, 0));
    return 0;
}
static int flux_mean_mark(picles_ctx *c, hipStream_t s)
{
    HIPCHK(c, hipEventRecord(c->fm_ev, s));
    c->fm_stream = s;
    c->fm_ev_live = true;
    return 0;
}

template <bool FROM_REC>
static void flux_mean_launch(picles_ctx *c, hipStream_t s, const Arrays &A, const double *u, const double *v)
{
    const FluxP &F = c->flux;
    const dim3 block(PICLES_BLOCK);
    const dim3 grid((unsigned)(nblocks(F.Nx, PICLES_BLOCK) * (long long)F.nyc_loc));
#define FM_CASE(CX) case CX: hipLaunchKernelGGL((k_flux_mean_update<FROM_REC, CX>), grid, block, 0, s, c->P, c->G, A, F, u, v, c->fm_acc); break
    switch (F.cx) {
    FM_CASE(1); FM_CASE(2); FM_CASE(4); FM_CASE(8); FM_CASE(16);
    default:
        hipLaunchKernelGGL((k_flux_mean_update<FROM_REC, 0>), dim3((unsigned)c->flux_npart), dim3(DIAG_TILE), 0, s, c->P, c->G, A, F, u, v, c->fm_acc);
    }
#undef FM_CASE
}

/* one update, on stream s — the stream behind which everything the sample depends on has been ordered (stat_update's rule).  The wind
 * rule first: it refuses before anything is launched; a lattice's level at the clock is sampled on s, behind the set's latest operation */
static int flux_mean_update(picles_ctx *c, hipStream_t s, const char *who)
{
    { int rc = flux_mean_order(c, s); if (rc) return rc; }
    const double *u, *v;
    { int rc = flux_wind(c, who, u, v, s); if (rc) return rc; }
    if (c->pending) flux_mean_launch<true>(c, s, arrays_for(c, c->cur, c->cur), u, v);
    else flux_mean_launch<false>(c, s, c->A, u, v);
    HIPCHK(c, hipGetLastError());
    { int rc = flux_mean_mark(c, s); if (rc) return rc; }
    /* a wind lattice samples the next windows on the context stream into planes this update may still be reading on another one */
    if (s != c->stream && c->wind.from_lattice()) HIPCHK(c, hipStreamWaitEvent(c->stream, c->fm_ev, 0));
    if (c->fm_samples == 0) c->fm_t_first = c->clock;
    c->fm_t_last = c->clock;
    c->fm_samples++;
    return 0;
}

static void flux_mean_release(picles_ctx *c)
{
    if (c->fm_acc) hipFree(c->fm_acc);
    if (c->fm_ev) hipEventDestroy(c->fm_ev);
    c->fm_acc = nullptr; c->fm_ev = nullptr; c->fm_stream = nullptr; c->fm_ev_live = false;
    c->fm_on = false; c->fm_bytes = 0;
    c->fm_cad = Cadence{};
    c->fm_samples = 0; c->fm_t_first = 0.0; c->fm_t_last = 0.0;
}

PX_EXPORT int32_t picles_flux_mean_init(picles_ctx *c, int32_t every, int32_t first)
{
    if (!c) return -1;
    if (!c->flux_ring.cap) return fail(c, -2, "picles_flux_mean_init: the mean set takes its cells, mask and scales from a flux set (picles_flux_init first)");
    if (c->fm_on) return fail(c, -2, "picles_flux_mean_init: a mean set exists (picles_flux_mean_free first)");
    if (every < 1 || first < 1) return fail(c, -2, "picles_flux_mean_init: every and first must be >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->flux.Nxc * c->flux.nyc_loc * FLUX_NP * 8;
    Undo undo{[c] { flux_mean_release(c); }};
    { int rc = store_stream_get(c); if (rc) return rc; }
    HIPCHK(c, hipMalloc(&c->fm_acc, bytes));
    HIPCHK(c, hipEventCreateWithFlags(&c->fm_ev, hipEventDisableTiming));
    HIPCHK(c, hipMemsetAsync(c->fm_acc, 0, bytes, c->stream));
    c->fm_bytes = bytes;
    { int rc = flux_mean_mark(c, c->stream); if (rc) return rc; }
    c->fm_cad = Cadence{every, first, 0};
    c->fm_samples = 0; c->fm_t_first = 0.0; c->fm_t_last = 0.0;
    c->fm_on = true;
    undo.armed = false;
    return 0;
}

PX_EXPORT int32_t picles_flux_mean_shape(const picles_ctx *c, int32_t *every, int32_t *n_planes, size_t *bytes)
{
    if (!c || !c->fm_on) return -1;
    if (every) *every = c->fm_cad.every;
    if (n_planes) *n_planes = FLUX_NP;
    if (bytes) *bytes = c->fm_bytes;
    return 0;
}

PX_EXPORT int32_t picles_flux_mean_update(picles_ctx *c, void *stream)
{
    if (!c) return -1;
    if (!c->fm_on) return fail(c, -2, "picles_flux_mean_init first");
    HIPCHK(c, hipSetDevice(c->device));
    if (stream) c->ext_streams = true;
    return flux_mean_update(c, stream ? (hipStream_t)stream : c->stream, "picles_flux_mean_update");
}

/* the accumulators and the three scalars to zero, on stream s behind the latest operation */
static int flux_mean_zero(picles_ctx *c, hipStream_t s)
{
    { int rc = flux_mean_order(c, s); if (rc) return rc; }
    HIPCHK(c, hipMemsetAsync(c->fm_acc, 0, c->fm_bytes, s));
    { int rc = flux_mean_mark(c, s); if (rc) return rc; }
    c->fm_samples = 0; c->fm_t_first = 0.0; c->fm_t_last = 0.0;
    return 0;
}

/* the finalising kernel on the context stream into (fields, partials), behind the updates wherever they ran.  Nothing is flushed */
static int flux_mean_final(picles_ctx *c, float *fields, double *partials)
{
    { int rc = flux_mean_order(c, c->stream); if (rc) return rc; }
    hipLaunchKernelGGL(k_flux_mean_final, dim3((unsigned)c->flux_npart), dim3(DIAG_TILE), 0, c->stream, c->flux, (double)c->fm_samples,
                       (const double *)c->fm_acc, fields, partials);
    HIPCHK(c, hipGetLastError());
    return flux_mean_mark(c, c->stream);
}

PX_EXPORT int32_t picles_flux_mean_push(picles_ctx *c, int32_t reset)
{
    if (!c) return -1;
    if (!c->fm_on) return fail(c, -2, "picles_flux_mean_init first");
    if (c->fm_samples == 0) return fail(c, -2, "picles_flux_mean_push: the mean set holds no sample: there is no mean to form");
    unsigned char *d = c->flux_ring.next_slot();
    if (!d) return fail(c, -3, "flux ring full: pop first");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flux_mean_final(c, (float *)d, (double *)(d + c->flux_part_off)); if (rc) return rc; }
    { int rc = c->flux_ring.ship(c, d, c->stream, c->flux_slot_bytes, 0); if (rc) return rc; }
    return reset ? flux_mean_zero(c, c->stream) : 0;
}

PX_EXPORT int32_t picles_flux_mean_export(picles_ctx *c, void *fields_dev, double *partials_dev, void *caller_stream, int32_t reset)
{
    if (!c) return -1;
    if (!c->fm_on) return fail(c, -2, "picles_flux_mean_init first");
    if (!fields_dev) return fail(c, -2, "picles_flux_mean_export: no device buffer for the fields");
    if (c->fm_samples == 0) return fail(c, -2, "picles_flux_mean_export: the mean set holds no sample: there is no mean to form");
    HIPCHK(c, hipSetDevice(c->device));
    if (!partials_dev) {
        if (!c->flux_scratch) HIPCHK(c, hipMalloc(&c->flux_scratch, (size_t)c->flux_npart * FLUX_NP * 8));
        partials_dev = c->flux_scratch;
    }
    if (caller_stream) {      /* whatever the caller still has reading or writing its buffers comes first */
        HIPCHK(c, hipEventRecord(c->ev_ctx, (hipStream_t)caller_stream));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_ctx, 0));
    }
    { int rc = flux_mean_final(c, (float *)fields_dev, partials_dev); if (rc) return rc; }
    if (caller_stream) {
        HIPCHK(c, hipEventRecord(c->ev_ctx, c->stream));
        HIPCHK(c, hipStreamWaitEvent((hipStream_t)caller_stream, c->ev_ctx, 0));
    }
    return reset ? flux_mean_zero(c, c->stream) : 0;
}

PX_EXPORT int32_t picles_flux_mean_get(picles_ctx *c, double *planes, int64_t *n_samples, double *t_first, double *t_last)
{
    if (!c) return -1;
    if (!c->fm_on) return fail(c, -2, "picles_flux_mean_init first");
    if (planes) {
        HIPCHK(c, hipSetDevice(c->device));
        /* the latest operation on the planes alone: the copy rides the store stream behind its event; a pending step stays pending */
        HIPCHK(c, hipStreamWaitEvent(c->store_stream, c->fm_ev, 0));
        HIPCHK(c, hipMemcpyAsync(planes, c->fm_acc, c->fm_bytes, hipMemcpyDeviceToHost, c->store_stream));
        HIPCHK(c, hipStreamSynchronize(c->store_stream));      /* the caller's (pageable) buffer is complete and released */
    }
    if (n_samples) *n_samples = (int64_t)c->fm_samples;
    if (t_first) *t_first = c->fm_t_first;
    if (t_last) *t_last = c->fm_t_last;
    return 0;
}

PX_EXPORT int32_t picles_flux_mean_set(picles_ctx *c, const double *planes, int64_t n_samples, double t_first, double t_last)
{
    if (!c) return -1;
    if (!c->fm_on) return fail(c, -2, "picles_flux_mean_init first");
    if (!planes) return fail(c, -2, "picles_flux_mean_set: planes must be given");
    if (n_samples < 0) return fail(c, -2, "picles_flux_mean_set: n_samples must be >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flux_mean_order(c, c->stream); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(c->fm_acc, planes, c->fm_bytes, hipMemcpyHostToDevice, c->stream));
    { int rc = flux_mean_mark(c, c->stream); if (rc) return rc; }
    HIPCHK(c, hipEventSynchronize(c->fm_ev));              /* the caller's buffer has been read to its last byte */
    c->fm_samples = (long long)n_samples; c->fm_t_first = t_first; c->fm_t_last = t_last;
    return 0;
}

PX_EXPORT int32_t picles_flux_mean_reset(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->fm_on) return fail(c, -2, "picles_flux_mean_init first");
    HIPCHK(c, hipSetDevice(c->device));
    return flux_mean_zero(c, c->stream);      /* in stream order behind the updates already issued; no host synchronisation; s goes on */
}

PX_EXPORT int32_t picles_flux_mean_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->fm_on) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());       /* updates in flight read and write the planes about to go */
    flux_mean_release(c);
    return 0;
}

/* ---- open-boundary forcing (the contract: include/picles_hip.h; the kernel: k_bforce.hip; the launch: bforce_launch above) ---- */
/* the forced nodes' records, emptied in both buffers of the pair when the set goes: no step kernel writes the record of a node it
 * does not step, so a record left behind would be scattered again by every later step.  Their particle slots go back to what a rim
 * node's is without a set (off, no status): picles_get_particles and later checkpoints show no particle that no longer exists */
__global__ void __launch_bounds__(256) k_bforce_clear(GridP G, double *rec_a, double *rec_b, unsigned char *on, int *status, int n, const int *nodes)
{
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k >= n) return;
    const int t = nodes[k], i = t % G.Nx, jl = t / G.Nx;
    const size_t at = (size_t)(jl + G.R) * 6 * G.Nx + (size_t)5 * G.Nx + i;
    rec_a[at] = 0.0;
    rec_b[at] = 0.0;
    on[t] = 0;
    status[t] = 0;
}

static void bforce_release(picles_ctx *c)
{
    if (c->bf_nodes) hipFree(c->bf_nodes);
    if (c->bf_lv) hipFree(c->bf_lv);
    if (c->bf_w) hipFree(c->bf_w);
    c->bf_nodes = nullptr;
    c->bf_lv = nullptr;
    c->bf_w = nullptr;
    c->bf_ocean.clear();
    c->bf_v0 = c->bf_v1 = nullptr;
    c->bf_n = 0;
    c->bf_levels = 0;
    c->bf_t0 = c->bf_t1 = 0.0;
}

/* band: picles_bforce_init_band — ocean nodes (mask class 1) are taken too, and an optional weight per node */
__global__ void __launch_bounds__(256) k_bforce_unstep(unsigned char *pflags, int n, const int *nodes)
{
    const int k = (int)(blockIdx.x * 256u + threadIdx.x);
    if (k < n) pflags[nodes[k]] &= (unsigned char)~PF_STEPPED;      /* each node once in the list: a byte has one writer */
}

/* mode: the rim set of picles_bforce_init, the band set of picles_bforce_init_band, or BF_FEEDBACK — the set picles_nest_feedback_init
 * makes on a parent: ocean nodes (mask class 1) only, unweighted, and allowed on a periodic_boundary model (no rim there, but an interior) */
enum { BF_RIM = 0, BF_BAND = 1, BF_FEEDBACK = 2 };

static int bforce_init_any(picles_ctx *c, int32_t n, const int32_t *ij, const double *weight, int mode)
{
    const bool band = mode == BF_BAND;
    const std::string who = mode == BF_FEEDBACK ? "picles_nest_feedback_init: the parent's set" : band ? "picles_bforce_init_band" : "picles_bforce_init";
    if (c->bf_n) return fail(c, -2, who + ": a boundary forcing set exists (picles_bforce_free first)");
    if (!launch_k_bforce) return fail(c, -5, who + ": this build of the library was linked without k_bforce");
    if (n < 1 || !ij) return fail(c, -2, who + ": n must be >= 1 and the node list given");
    const GridP &G = c->G;
    if (!G.single_slab || c->ring)
        return fail(c, -5, who + ": slabs and the native ring do not carry a boundary forcing (a whole-grid context, not in slab mode, is needed)");
    if (G.tripolar) return fail(c, -5, who + ": not supported on a tripolar grid");
    if (c->md.periodic_boundary && mode != BF_FEEDBACK)
        return fail(c, -5, who + ": a model with periodic_boundary steps its grid-boundary nodes itself: there is no open rim to force");
    std::vector<int> loc((size_t)n), ocean;
    std::vector<unsigned char> seen((size_t)c->A.n, 0);
    bool blend = false;
    for (int k = 0; k < n; k++) {
        const int i = ij[k], j = ij[(size_t)n + k];
        const std::string node = who + ": node " + std::to_string(k) + " = (" + std::to_string(i) + ", " + std::to_string(j) + ")";
        if (i < 0 || i >= G.Nx || j < 0 || j >= G.Ny) return fail(c, -2, node + " lies outside [0, Nx) x [0, Ny)");
        const long long t = (long long)j * G.Nx + i;
        const int mk = (int)c->h_mask[t];
        if (mode == BF_FEEDBACK && mk != 1)
            return fail(c, -2, node + " is no ocean node of the parent (mask class " + std::to_string(mk) + ", 1 is needed): feedback goes to nodes the parent steps");
        if (mode == BF_RIM && mk != 3)
            return fail(c, -2, node + " is no grid-boundary node (mask class " + std::to_string(mk) + ", 3 is needed): only the open rim can be forced");
        if (band && mk != 3 && mk != 1)
            return fail(c, -2, node + " is neither a grid-boundary node nor an ocean node (mask class " + std::to_string(mk) +
                               ", 3 or 1 is needed): land and coast carry no particle");
        if (seen[t]) return fail(c, -2, node + " is given twice");
        if (weight) {
            const double w = weight[k];
            if (!(std::isfinite(w) && w > 0.0 && w <= 1.0)) {
                char b[64];
                snprintf(b, sizeof b, "%.17g", w);
                return fail(c, -2, node + " has the weight " + b + ": a weight must be finite and in (0, 1]");
            }
            if (w != 1.0) blend = true;
        }
        seen[t] = 1;
        loc[k] = (int)t;
        if (mk == 1) ocean.push_back((int)t);
    }
    HIPCHK(c, hipSetDevice(c->device));
    Undo undo{[c] { bforce_release(c); }};
    HIPCHK(c, hipMalloc(&c->bf_nodes, (size_t)n * sizeof(int)));
    HIPCHK(c, hipMalloc(&c->bf_lv, (size_t)6 * n * sizeof(double)));
    HIPCHK(c, hipMemcpy(c->bf_nodes, loc.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));     /* blocking: loc dies here */
    if (blend) {      /* (a set whose weights are all 1.0 is an unweighted set: the flavours without BLEND, no plane) */
        HIPCHK(c, hipMalloc(&c->bf_w, (size_t)n * sizeof(double)));
        HIPCHK(c, hipMemcpy(c->bf_w, weight, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!ocean.empty()) {
        /* the set's ocean nodes leave the step kernels' hands: in stream order behind whatever is enqueued (a launch in flight on
         * a caller's stream is waited for), a pending fused step stays pending — the records it left at these nodes are legitimate
         * and the next step pulls them */
        if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());
        hipLaunchKernelGGL(k_bforce_unstep, dim3(nblocks(n, 256)), dim3(256), 0, c->stream, c->A.pflags, n, (const int *)c->bf_nodes);
        HIPCHK(c, hipGetLastError());
    }
    c->bf_ocean.swap(ocean);
    c->bf_n = n;
    c->bf_levels = 0;
    c->bf_v0 = c->bf_lv;
    c->bf_v1 = c->bf_lv + (size_t)3 * n;
    undo.armed = false;
    return 0;
}

PX_EXPORT int32_t picles_bforce_init(picles_ctx *c, int32_t n, const int32_t *ij)
{
    if (!c) return -1;
    return bforce_init_any(c, n, ij, nullptr, BF_RIM);
}

PX_EXPORT int32_t picles_bforce_init_band(picles_ctx *c, int32_t n, const int32_t *ij, const double *weight)
{
    if (!c) return -1;
    return bforce_init_any(c, n, ij, weight, BF_BAND);
}

PX_EXPORT int32_t picles_bforce_set_levels(picles_ctx *c, double t0, const double *v0, double t1, const double *v1)
{
    if (!c) return -1;
    if (!c->bf_n) return fail(c, -2, "picles_bforce_init first");
    if (c->nest) return fail(c, -2, "picles_bforce_set_levels: this set's levels come from a parent context (a nest): picles_nest_free first");
    if (c->fb_child) return fail(c, -2, "picles_bforce_set_levels: this set's level comes from a child context (nest feedback): picles_nest_feedback_free "
                                        "on the child, or picles_bforce_free here, first");
    if (!v0) return fail(c, -2, "picles_bforce_set_levels: level 0 must be given");
    if (v1 && !(t1 > t0)) return fail(c, -2, "picles_bforce_set_levels: two levels need t1 > t0");
    if (v1 && !(std::isfinite(t0) && std::isfinite(t1))) return fail(c, -2, "picles_bforce_set_levels: the level times must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    /* in stream order behind the launches that read the levels in place; a pending fused step stays pending */
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());
    const size_t b = (size_t)3 * c->bf_n * sizeof(double);
    HIPCHK(c, hipMemcpyAsync(c->bf_lv, v0, b, hipMemcpyHostToDevice, c->stream));
    if (v1) HIPCHK(c, hipMemcpyAsync((char *)c->bf_lv + b, v1, b, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      /* the caller's buffers are free when this returns */
    c->bf_levels = v1 ? 2 : 1;
    c->bf_t0 = t0;
    c->bf_t1 = v1 ? t1 : t0;
    return 0;
}

PX_EXPORT int32_t picles_bforce_info(const picles_ctx *c, int32_t *n, int32_t *levels, double *t0, double *t1)
{
    if (!c || !c->bf_n) return -1;
    if (n) *n = c->bf_n;
    if (levels) *levels = c->bf_levels;
    if (t0) *t0 = c->bf_t0;
    if (t1) *t1 = c->bf_t1;
    return 0;
}

PX_EXPORT int32_t picles_bforce_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->bf_n) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = nest_leave_set(c); if (rc) return rc; }      /* a nest and a feedback go with the set they fill */
    { int rc = flush(c); if (rc) return rc; }      /* a pending step's forced records are scattered before they are emptied */
    HIPCHK(c, hipDeviceSynchronize());       /* launches in flight read the list and the levels about to go */
    hipLaunchKernelGGL(k_bforce_clear, dim3(nblocks(c->bf_n, 256)), dim3(256), 0, c->stream, c->G, c->rec_buf[0], c->rec_buf[1], c->A.on, c->A.status,
                       c->bf_n, (const int *)c->bf_nodes);
    HIPCHK(c, hipGetLastError());
    { int rc = class_map_zero(c); if (rc) return rc; }      /* records written by other means than the step kernels */
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool band = !c->bf_ocean.empty();
    bforce_release(c);
    /* the band's ocean nodes go back to the step kernels: the home flags, from h_mask and the model; the remesh of the next step
     * finds them without a particle and seeds them like any other node */
    if (band) return context_pflags(c);
    return 0;
}

PX_EXPORT int32_t picles_bforce_get_levels(picles_ctx *c, double *v0, double *v1)
{
    if (!c) return -1;
    if (!c->bf_n) return fail(c, -2, "picles_bforce_init first");
    if ((v0 && c->bf_levels < 1) || (v1 && c->bf_levels < 2))
        return fail(c, -2, "picles_bforce_get_levels: the set holds " + std::to_string(c->bf_levels) + " level(s): pass NULL for a plane block it does not hold");
    HIPCHK(c, hipSetDevice(c->device));
    /* behind whatever wrote the levels: another context's stencil (its event), an upload on the context stream.  No flush: a pending step stays pending */
    { int rc = nest_levels_wait(c, c->stream); if (rc) return rc; }
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t b = (size_t)3 * c->bf_n * sizeof(double);
    if (v0) HIPCHK(c, hipMemcpy(v0, c->bf_v0, b, hipMemcpyDeviceToHost));      /* blocking: the caller's buffers are complete on return */
    if (v1) HIPCHK(c, hipMemcpy(v1, c->bf_v1, b, hipMemcpyDeviceToHost));
    return 0;
}

/* ---- nesting: one link behind both directions (the contract: include/picles_hip.h "one-way nesting" and "two-way nesting"; the
 * stencil kernels: k_nest.h) ----
 * A link carries the State of a SOURCE context onto the nodes of a TARGET context's forcing set, all on the device: the State at the
 * distinct source nodes (k_probe, into the stencil's staging block), then per target node the weighted mean of its entries
 * (k_nest_mix / k_nest_restrict) straight into one of the set's level slots.  Both kernels run on the SOURCE's stream; the target's
 * k_bforce reads the slots on the TARGET's.
 *   one-way (struct Nest)      source = parent, target = child.  Three slots: 0 and 1 are the set's own block (bf_lv, bf_lv + 3 n),
 *                              2 is the nest's; the pair the child reads is (slot[i0], slot[i1]), rotated by pointer, and a sample
 *                              writes the slot outside the pair
 *   two-way (struct Feedback)  source = child, target = parent.  The set's own two slots, used alternately; the parent reads one
 *                              level, its bf_v0 switched by pointer
 * ORDERING: two rules, kept by one SlotSync per link.
 *   read after write   `written` is recorded on the source's stream behind the stencil kernel (published); the target's next launch
 *                      that reads the levels, and picles_bforce_get_levels, wait for it (wait_written).  k_bforce sits behind the
 *                      target's step kernel on its stream, so that kernel still overlaps the source's work
 *   write after read   read[k] is recorded on the target's stream behind a launch that read slot k (mark_read); the source's stream
 *                      waits for it before the stencil that overwrites slot k (claim)
 *   one-way marks a slot once, when it leaves the pair — in picles_nest_sample, behind the last enqueued launch that read it, and at
 *   init for slots 0 and 1, which launches enqueued under uploaded levels may still read: no runtime call in a child step, and the
 *   wait lies a whole chunk of the child back, so the parent's step kernels, in front of the sampling on its stream, never wait for
 *   the child's current chunk.  Two-way marks behind every k_bforce of the parent (nest_levels_read); with two slots the launch
 *   waited for belongs to the parent step before last: never current work */
struct SlotSync {
    hipEvent_t written = nullptr, read[3] = {nullptr, nullptr, nullptr};
    bool unseen = false, live[3] = {false, false, false};
    int create(picles_ctx *c, int n_slots)
    {
        HIPCHK(c, hipEventCreateWithFlags(&written, hipEventDisableTiming));
        for (int k = 0; k < n_slots; k++) HIPCHK(c, hipEventCreateWithFlags(&read[k], hipEventDisableTiming));
        return 0;
    }
    void destroy() { for (hipEvent_t e : {written, read[0], read[1], read[2]}) if (e) hipEventDestroy(e); }
    void forget() { unseen = live[0] = live[1] = live[2] = false; }
    /* the target's stream s is about to read the levels.  own: s is its context stream, which every later launch of it follows */
    int wait_written(picles_ctx *c, hipStream_t s, bool own)
    {
        if (unseen) { HIPCHK(c, hipStreamWaitEvent(s, written, 0)); unseen = !own; }
        return 0;
    }
    int mark_read(picles_ctx *c, int k, hipStream_t s) { HIPCHK(c, hipEventRecord(read[k], s)); live[k] = true; return 0; }
    int claim(picles_ctx *c, int k, hipStream_t s)
    {
        if (live[k]) { HIPCHK(c, hipStreamWaitEvent(s, read[k], 0)); live[k] = false; }
        return 0;
    }
    int published(picles_ctx *c, hipStream_t s) { HIPCHK(c, hipEventRecord(written, s)); unseen = true; return 0; }
};

/* the words and the rules in which the stencils of the two directions differ */
struct StencilRules {
    const char *who, *source, *entry, *grid, *count;
    bool padded;      /* weights are >= 0, 0.0 marks padding, a node needs an entry that is none: k_nest_restrict; else four entries, k_nest_mix */
};
static const StencilRules NEST_RULES = {"picles_nest_init", "corner", "corner", "the parent's grid", "n_corner", false};
static const StencilRules FEEDBACK_RULES = {"picles_nest_feedback_init", "source node", "entry", "the child's grid", "n_src", true};

/* G: the source's grid (a whole grid: its local rows are the global ones) */
static int stencil_check(picles_ctx *c, const StencilRules &R, const GridP &G, int n_out, int n_src, int m, const int32_t *src_ij, const int32_t *index,
                         const double *weight)
{
    const std::string who = std::string(R.who) + ": ";
    for (int k = 0; k < n_src; k++) {
        const int i = src_ij[k], j = src_ij[(size_t)n_src + k];
        if (i < 0 || i >= G.Nx || j < 0 || j >= G.Ny)
            return fail(c, -2, who + R.source + " " + std::to_string(k) + " = (" + std::to_string(i) + ", " + std::to_string(j) + ") lies outside " + R.grid +
                               " [0, " + std::to_string(G.Nx) + ") x [0, " + std::to_string(G.Ny) + ")");
    }
    std::vector<unsigned char> any((size_t)n_out, 0);
    for (size_t k = 0; k < (size_t)m * n_out; k++) {
        auto at = [&] { return "node " + std::to_string(k % n_out) + ", " + R.entry + " " + std::to_string(k / n_out); };
        if (index[k] < 0 || index[k] >= n_src)
            return fail(c, -2, who + "index " + std::to_string(index[k]) + " of " + at() + ", lies outside [0, " + R.count + " = " + std::to_string(n_src) + ")");
        if (!std::isfinite(weight[k]) || (R.padded && weight[k] < 0.0))
            return fail(c, -2, who + "the weight of " + at() + (R.padded ? ", is not finite or is negative" : ", is not finite"));
        if (weight[k] > 0.0) any[k % n_out] = 1;
    }
    for (int k = 0; R.padded && k < n_out; k++)
        if (!any[(size_t)k]) return fail(c, -2, who + "every weight of node " + std::to_string(k) + " is zero: it has no source");
    return 0;
}

struct NestStencil {
    int n_out = 0, n_src = 0, m = 0;
    bool padded = false;
    int *src_nodes = nullptr;                 /* device: the i plane, then the row plane, of the source nodes */
    double *src = nullptr;                    /* device: 3 planes of n_src doubles, the staging block k_probe fills */
    int *index = nullptr;                     /* device: m planes of n_out */
    double *weight = nullptr;                 /* device: m planes of n_out */
    /* checked arrays (stencil_check) onto the device; blocking copies: the caller's arrays are free on return */
    int upload(picles_ctx *c, const StencilRules &R, int n_out_, int n_src_, int m_, const int32_t *src_ij, const int32_t *ix, const double *w)
    {
        n_out = n_out_; n_src = n_src_; m = m_; padded = R.padded;
        const size_t e = (size_t)m * n_out;
        HIPCHK(c, hipMalloc(&src_nodes, (size_t)2 * n_src * sizeof(int)));
        HIPCHK(c, hipMalloc(&src, (size_t)3 * n_src * sizeof(double)));
        HIPCHK(c, hipMalloc(&index, e * sizeof(int)));
        HIPCHK(c, hipMalloc(&weight, e * sizeof(double)));
        HIPCHK(c, hipMemcpy(src_nodes, src_ij, (size_t)2 * n_src * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(index, ix, e * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(weight, w, e * sizeof(double), hipMemcpyHostToDevice));
        return 0;
    }
    void release() { for (void *q : {(void *)src_nodes, (void *)src, (void *)index, (void *)weight}) if (q) hipFree(q); }
    /* one level into `out` (3 planes of n_out) on stream s: the State of `from` as that stream finds it — probe_launch's choice: from
     * the records of a pending fused step, which stays pending, or from State.  Errors are reported on c, the child */
    int run(picles_ctx *c, picles_ctx *from, hipStream_t s, double *out) const
    {
        { int rc = probe_launch(c, from, s, n_src, src_nodes, src); if (rc) return rc; }
        const dim3 grid(nblocks(n_out, NEST_BLOCK)), block(NEST_BLOCK);
        if (padded)
            hipLaunchKernelGGL(k_nest_restrict, grid, block, 0, s, n_out, n_src, m, (const int *)index, (const double *)weight, (const double *)src, out);
        else
            hipLaunchKernelGGL(k_nest_mix, grid, block, 0, s, n_out, n_src, (const int *)index, (const double *)weight, (const double *)src, out);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
};

struct Nest {
    picles_ctx *parent = nullptr;             /* nullptr: detached — the parent was destroyed; the levels stay */
    NestStencil st;                           /* the parent's corner nodes onto the child's forced nodes, four corners each */
    SlotSync sync;
    double *extra = nullptr;                  /* device: slot 2 */
    double *slot[3] = {nullptr, nullptr, nullptr};
    int i0 = 0, i1 = 1;
    long long samples = 0;
};
struct Feedback {
    picles_ctx *parent = nullptr;             /* nullptr: detached — the parent was destroyed, and the slots with its set */
    NestStencil st;                           /* the child's source nodes onto the parent's feedback nodes, m entries each */
    SlotSync sync;
    double *slot[2] = {nullptr, nullptr};     /* the parent's bf_lv and bf_lv + 3 n_fb */
    int cur = 1;                              /* the slot the parent reads (the first feedback writes slot 0) */
    long long taken = 0;
};

/* stream s of context c is about to read c's levels: behind the latest stencil of whoever writes them */
static int nest_levels_wait(picles_ctx *c, hipStream_t s)
{
    if (c->nest) { int rc = c->nest->sync.wait_written(c, s, s == c->stream); if (rc) return rc; }
    if (c->fb_child) return c->fb_child->fb->sync.wait_written(c, s, s == c->stream);
    return 0;
}

/* a launch on stream s of context c has been enqueued that reads the level at `read`: a fed parent marks the slot */
static int nest_levels_read(picles_ctx *c, hipStream_t s, const double *read)
{
    if (!c->fb_child) return 0;
    Feedback *F = c->fb_child->fb;
    for (int k = 0; k < 2; k++)
        if (read == F->slot[k]) { int rc = F->sync.mark_read(c, k, s); if (rc) return rc; }
    return 0;
}

/* drop the nest of c.  keep_levels: the pair the set holds moves home to (bf_lv, bf_lv + 3 n), where a set without a nest keeps it */
static int nest_release(picles_ctx *c, bool keep_levels)
{
    Nest *N = c->nest;
    if (!N) return 0;
    HIPCHK(c, hipDeviceSynchronize());       /* a mix in flight writes the slots, launches in flight read them */
    const size_t n3 = (size_t)3 * c->bf_n;
    if (keep_levels && c->bf_levels > 0 && (N->i0 != 0 || (c->bf_levels == 2 && N->i1 != 1))) {
        std::vector<double> h(2 * n3);
        HIPCHK(c, hipMemcpy(h.data(), N->slot[N->i0], n3 * sizeof(double), hipMemcpyDeviceToHost));
        if (c->bf_levels == 2) HIPCHK(c, hipMemcpy(h.data() + n3, N->slot[N->i1], n3 * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(c->bf_lv, h.data(), (c->bf_levels == 2 ? 2 : 1) * n3 * sizeof(double), hipMemcpyHostToDevice));
    }
    if (N->parent) {
        auto &v = N->parent->nest_children;
        v.erase(std::remove(v.begin(), v.end(), c), v.end());
    }
    N->st.release();
    if (N->extra) hipFree(N->extra);
    N->sync.destroy();
    delete N;
    c->nest = nullptr;
    c->bf_v0 = c->bf_lv;
    c->bf_v1 = c->bf_lv ? c->bf_lv + n3 : nullptr;
    return 0;
}

/* free the child's feedback blocks and cut both links; the parent's set is the caller's business (nothing of it is touched).
 * The caller has drained the device where work may be in flight */
static void fb_drop(picles_ctx *c)
{
    Feedback *F = c->fb;
    if (!F) return;
    if (F->parent) F->parent->fb_child = nullptr;
    F->st.release();
    F->sync.destroy();
    delete F;
    c->fb = nullptr;
}

/* drop the feedback of child c and, where the parent lives, the set it made there (its nodes go back to the parent's step kernels:
 * picles_bforce_free restores the flags through context_pflags) */
static int fb_release(picles_ctx *c)
{
    if (!c->fb) return 0;
    picles_ctx *p = c->fb->parent;
    HIPCHK(c, hipDeviceSynchronize());       /* a restrict in flight writes the parent's slots, the parent's launches read them */
    fb_drop(c);
    if (p) {
        int rc = picles_bforce_free(p);
        if (rc) return fail(c, rc, "picles_nest_feedback_free: the parent's set: " + p->err);
    }
    return 0;
}

/* picles_bforce_free(c): a nest and a feedback go with the set they fill */
static int nest_leave_set(picles_ctx *c)
{
    if (c->fb) { int rc = fb_release(c); if (rc) return rc; }                  /* a child's feedback goes before its nest */
    if (c->nest) { int rc = nest_release(c, false); if (rc) return rc; }      /* the nest goes with the set it feeds */
    if (c->fb_child) {      /* a fed parent: the feedback goes with the set; the child keeps its one-way nest */
        HIPCHK(c, hipDeviceSynchronize());       /* a restrict in flight on the child's stream writes the level block */
        fb_drop(c->fb_child);
    }
    return 0;
}

/* picles_destroy(c), its streams drained.  As a parent: the children keep their last levels and lose their parent (no mix is in
 * flight); a child that feeds c keeps its Feedback, without a parent and without slots (picles_nest_feedback then fails with a
 * text) and its one-way nest — its stream is drained first: a restrict in flight writes c's level block.  As a child: the feedback
 * goes, and with it the set it made on the parent; then the nest, which leaves the parent's list before its blocks go */
static void nest_leave_context(picles_ctx *c)
{
    for (picles_ctx *k : c->nest_children)
        if (k->nest) k->nest->parent = nullptr;
    c->nest_children.clear();
    if (c->fb) fb_release(c);
    if (c->fb_child) {
        hipDeviceSynchronize();
        Feedback *F = c->fb_child->fb;
        F->parent = nullptr;
        F->slot[0] = F->slot[1] = nullptr;
        F->sync.forget();
        c->fb_child = nullptr;
    }
    if (c->nest) nest_release(c, false);
}

static const char *const NEST_NO_EXT_STREAMS = ": a context that has run on caller-provided streams cannot be ordered by the nest's events: "
                                               "nest contexts that step on their own stream (stream = NULL everywhere)";

PX_EXPORT int32_t picles_nest_init(picles_ctx *c, picles_ctx *p, int32_t n_corner, const int32_t *corner_ij, const int32_t *index, const double *weight)
{
    if (!c) return -1;
    if (!p) return fail(c, -2, "picles_nest_init: no parent context given");
    if (c == p) return fail(c, -2, "picles_nest_init: child and parent are the same context: a nest needs two (create the parent model separately)");
    if (c->nest) return fail(c, -2, "picles_nest_init: this context holds a nest (picles_nest_free first)");
    if (c->device != p->device)
        return fail(c, -5, "picles_nest_init: child on device " + std::to_string(c->device) + ", parent on device " + std::to_string(p->device) +
                           ": create both contexts on one device");
    if (!c->G.single_slab || c->ring || !p->G.single_slab || p->ring)
        return fail(c, -5, "picles_nest_init: slabs, slab mode and the native ring do not nest: both contexts must be whole-grid contexts");
    if (c->wind.streamed() || p->wind.streamed())
        return fail(c, -5, "picles_nest_init: the child or the parent holds a wind stream (picles_wind_stream_*): streamed nests are not carried");
    if (!c->bf_n) return fail(c, -2, "picles_nest_init: the child has no boundary forcing set: picles_bforce_init with the nodes to force first");
    if (c->ext_streams || p->ext_streams) return fail(c, -5, std::string("picles_nest_init") + NEST_NO_EXT_STREAMS);
    if (n_corner < 1 || !corner_ij || !index || !weight)
        return fail(c, -2, "picles_nest_init: n_corner must be >= 1 and corner_ij, index and weight given");
    const int n = c->bf_n;
    { int rc = stencil_check(c, NEST_RULES, p->G, n, n_corner, 4, corner_ij, index, weight); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    Nest *N = new Nest;
    c->nest = N;                              /* (no parent yet: a failure below releases without touching p) */
    Undo undo{[c] { nest_release(c, true); }};
    { int rc = N->st.upload(c, NEST_RULES, n, n_corner, 4, corner_ij, index, weight); if (rc) return rc; }
    HIPCHK(c, hipMalloc(&N->extra, (size_t)3 * n * sizeof(double)));
    { int rc = N->sync.create(c, 3); if (rc) return rc; }
    /* launches of the child enqueued under uploaded levels may still read slots 0 and 1 */
    for (int k = 0; k < 2; k++) { int rc = N->sync.mark_read(c, k, c->stream); if (rc) return rc; }
    N->slot[0] = c->bf_lv;
    N->slot[1] = c->bf_lv + (size_t)3 * n;
    N->slot[2] = N->extra;
    N->parent = p;
    p->nest_children.push_back(c);
    c->bf_levels = 0;                         /* the levels come from the parent from here on: none taken yet */
    c->bf_t0 = c->bf_t1 = 0.0;
    c->bf_v0 = N->slot[0];
    c->bf_v1 = N->slot[1];
    undo.armed = false;
    return 0;
}

PX_EXPORT int32_t picles_nest_sample(picles_ctx *c)
{
    if (!c) return -1;
    Nest *N = c->nest;
    if (!N) return fail(c, -2, "picles_nest_sample: picles_nest_init first");
    picles_ctx *p = N->parent;
    if (!p) return fail(c, -2, "picles_nest_sample: the parent context was destroyed (the set keeps its last levels): picles_nest_free, then "
                               "picles_nest_init with a living parent");
    if (c->ext_streams || p->ext_streams) return fail(c, -5, std::string("picles_nest_sample") + NEST_NO_EXT_STREAMS);
    if (N->samples > 0 && !(p->clock > c->bf_t1)) {
        char b[256];
        snprintf(b, sizeof b, "picles_nest_sample: the parent's clock (%.17g) has not moved past the latest level (%.17g): step the parent first", p->clock, c->bf_t1);
        return fail(c, -2, b);
    }
    HIPCHK(c, hipSetDevice(c->device));
    /* the slot to write: level 0 at first, level 1 next, then the slot outside the pair — after the level that leaves the pair has
     * had its last reader marked on the child's stream */
    int w;
    if (c->bf_levels == 0) w = N->i0;
    else if (c->bf_levels == 1) w = N->i1;
    else {
        { int rc = N->sync.mark_read(c, N->i0, c->stream); if (rc) return rc; }
        w = 3 - N->i0 - N->i1;
    }
    hipStream_t s = p->stream;
    { int rc = N->sync.claim(c, w, s); if (rc) return rc; }
    { int rc = N->st.run(c, p, s, N->slot[w]); if (rc) return rc; }
    { int rc = N->sync.published(c, s); if (rc) return rc; }
    if (c->bf_levels == 0) {
        c->bf_levels = 1;
        c->bf_t0 = c->bf_t1 = p->clock;
    } else {
        if (c->bf_levels == 2) { N->i0 = N->i1; c->bf_t0 = c->bf_t1; }
        N->i1 = w;
        c->bf_levels = 2;
        c->bf_t1 = p->clock;
    }
    c->bf_v0 = N->slot[N->i0];
    c->bf_v1 = N->slot[N->i1];
    N->samples++;
    return 0;
}

/* a nest resumed: the pair a checkpointed child held goes back into the slots (i0, i1) name, as if two samples had been taken.  The
 * copies ride on the CHILD's stream, behind the launches nest_init marked as readers of slots 0 and 1 (read[0], read[1] were recorded
 * on that stream), and the call waits for them: both marks are spent as the claims of two real samples spend them, and nothing was
 * published — no event the child's next launch could wait for in vain.  The third sample marks slot i0 and writes slot 2, unclaimed */
PX_EXPORT int32_t picles_nest_set_levels(picles_ctx *c, double t0, const double *v0, double t1, const double *v1)
{
    if (!c) return -1;
    Nest *N = c->nest;
    if (!N) return fail(c, -2, "picles_nest_set_levels: picles_nest_init first (a set without a nest takes picles_bforce_set_levels)");
    picles_ctx *p = N->parent;
    if (!p) return fail(c, -2, "picles_nest_set_levels: the parent context was destroyed: picles_nest_free, then picles_nest_init with a living parent");
    if (c->ext_streams || p->ext_streams) return fail(c, -2, std::string("picles_nest_set_levels") + NEST_NO_EXT_STREAMS);
    if (N->samples > 0)
        return fail(c, -2, "picles_nest_set_levels: this nest has taken " + std::to_string(N->samples) + " sample(s): a pair is put back into a fresh nest "
                           "(picles_nest_free, picles_nest_init), in front of the first picles_nest_sample");
    if (!v0 || !v1) return fail(c, -2, "picles_nest_set_levels: both levels must be given (a resumed nest holds a pair)");
    if (!(std::isfinite(t0) && std::isfinite(t1))) return fail(c, -2, "picles_nest_set_levels: the level times must be finite");
    if (!(t1 > t0)) return fail(c, -2, "picles_nest_set_levels: the pair needs t1 > t0");
    if (!(p->clock == t1)) {
        char b[256];
        snprintf(b, sizeof b, "picles_nest_set_levels: the parent's clock (%.17g) is not t1 (%.17g): level 1 is the parent's State at its clock "
                              "(load the parent's checkpoint first)", p->clock, t1);
        return fail(c, -2, b);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t b = (size_t)3 * c->bf_n * sizeof(double);
    HIPCHK(c, hipMemcpyAsync(N->slot[N->i0], v0, b, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(N->slot[N->i1], v1, b, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      /* the caller's buffers are free when this returns */
    N->sync.live[N->i0] = N->sync.live[N->i1] = false;      /* their readers lie behind the copies, which are complete */
    c->bf_levels = 2;
    c->bf_t0 = t0;
    c->bf_t1 = t1;
    c->bf_v0 = N->slot[N->i0];
    c->bf_v1 = N->slot[N->i1];
    N->samples = 2;
    return 0;
}

PX_EXPORT int32_t picles_nest_info(const picles_ctx *c, int32_t *n_corner, int64_t *samples)
{
    if (!c || !c->nest) return -1;
    if (n_corner) *n_corner = c->nest->st.n_src;
    if (samples) *samples = c->nest->samples;
    return 0;
}

PX_EXPORT int32_t picles_nest_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->nest) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->fb) { int rc = fb_release(c); if (rc) return rc; }      /* the feedback lives on the nest */
    return nest_release(c, true);
}

/* one axis of picles_nest_prolong's tables, held as stencil_check holds a stencil: indices inside [0, n_par), weights finite and in [0, 1] */
static int prolong_axis_check(picles_ctx *c, const char *axis, int n_child, int n_par, const int32_t *i0, const int32_t *i1, const double *w,
                              const char *call = "picles_nest_prolong")
{
    const std::string who = std::string(call) + ": ";
    for (int k = 0; k < n_child; k++) {
        for (int v : {i0[k], i1[k]})
            if (v < 0 || v >= n_par)
                return fail(c, -2, who + "index " + std::to_string(v) + " of the child's " + axis + " " + std::to_string(k) + " lies outside the parent's grid [0, " +
                                   std::to_string(n_par) + ")");
        if (!std::isfinite(w[k]) || w[k] < 0.0 || w[k] > 1.0)
            return fail(c, -2, who + "the weight of the child's " + axis + " " + std::to_string(k) + " is not finite or lies outside [0, 1]");
    }
    return 0;
}

/* the six tables of picles_nest_prolong / picles_nest_relocate on the device, one block the child keeps: wx, wy, then ix0, ix1, iy0, iy1 */
static int prolong_tab_upload(picles_ctx *c, const int32_t *ix0, const int32_t *ix1, const double *wx, const int32_t *iy0, const int32_t *iy1,
                              const double *wy)
{
    const int ncx = c->G.Nx, ncy = c->G.Ny;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nd = (size_t)ncx + ncy, bytes = nd * sizeof(double) + 2 * nd * sizeof(int);
    if (c->prolong_tab) HIPCHK(c, hipStreamSynchronize(c->stream));      /* the launch of an earlier call may still read them */
    if (c->prolong_cap < bytes) {
        double *q = nullptr;
        HIPCHK(c, hipMalloc(&q, bytes));
        if (c->prolong_tab) hipFree(c->prolong_tab);
        c->prolong_tab = q;
        c->prolong_cap = bytes;
    }
    std::vector<unsigned char> h(bytes);
    {
        double *hd = (double *)h.data();
        int *hi = (int *)(hd + nd);
        std::copy(wx, wx + ncx, hd);
        std::copy(wy, wy + ncy, hd + ncx);
        std::copy(ix0, ix0 + ncx, hi);
        std::copy(ix1, ix1 + ncx, hi + ncx);
        std::copy(iy0, iy0 + ncy, hi + 2 * ncx);
        std::copy(iy1, iy1 + ncy, hi + 2 * ncx + ncy);
    }
    HIPCHK(c, hipMemcpy(c->prolong_tab, h.data(), bytes, hipMemcpyHostToDevice));       /* blocking: the caller's tables are free on return */
    return 0;
}

PX_EXPORT int32_t picles_nest_prolong(picles_ctx *c, picles_ctx *p, const int32_t *ix0, const int32_t *ix1, const double *wx,
                                      const int32_t *iy0, const int32_t *iy1, const double *wy, double dt)
{
    if (!c) return -1;
    if (!p) return fail(c, -2, "picles_nest_prolong: no parent context given");
    if (c == p) return fail(c, -2, "picles_nest_prolong: child and parent are the same context: a child is started from another model");
    if (c->device != p->device)
        return fail(c, -5, "picles_nest_prolong: child on device " + std::to_string(c->device) + ", parent on device " + std::to_string(p->device) +
                           ": create both contexts on one device");
    if (!c->G.single_slab || c->ring || !p->G.single_slab || p->ring)
        return fail(c, -5, "picles_nest_prolong: slabs, slab mode and the native ring do not nest: both contexts must be whole-grid contexts");
    if (c->ext_streams || p->ext_streams) return fail(c, -5, std::string("picles_nest_prolong") + NEST_NO_EXT_STREAMS);
    if (!p->seeded) return fail(c, -2, "picles_nest_prolong: the parent was never seeded: it holds no sea state to start a child from");
    if (!(dt > 0.0)) return fail(c, -2, "picles_nest_prolong: dt must be positive (the child's step: the remesh and a lattice's first window use it)");
    if (!ix0 || !ix1 || !wx || !iy0 || !iy1 || !wy) return fail(c, -2, "picles_nest_prolong: the six tables ix0, ix1, wx, iy0, iy1, wy must be given");
    const int ncx = c->G.Nx, ncy = c->G.Ny;
    { int rc = prolong_axis_check(c, "column", ncx, p->G.Nx, ix0, ix1, wx); if (rc) return rc; }
    { int rc = prolong_axis_check(c, "row", ncy, p->G.Ny, iy0, iy1, wy); if (rc) return rc; }
    { int rc = prolong_tab_upload(c, ix0, ix1, wx, iy0, iy1, wy); if (rc) return rc; }
    const size_t nd = (size_t)ncx + ncy;
    {   /* the parent's State at its clock, whole: its pending step completed on its own stream */
        const std::string keep = p->err;
        int rc = flush(p);
        if (rc) { const std::string why = p->err; p->err = keep; return fail(c, rc, "picles_nest_prolong: the parent's pending step: " + why); }
    }
    /* from here on the child changes: what picles_seed resets, at the parent's clock and under the wind there */
    { int rc = seed_at(c, p->clock, p->clock, dt); if (rc) return rc; }
    HIPCHK(c, hipEventRecord(p->ev_ctx, p->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, p->ev_ctx, 0));
    const double *dwx = c->prolong_tab, *dwy = dwx + ncx;
    const int *dix0 = (const int *)(c->prolong_tab + nd), *dix1 = dix0 + ncx, *diy0 = dix1 + ncx, *diy1 = diy0 + ncy;
    hipLaunchKernelGGL(k_nest_prolong, dim3(nblocks(c->A.n, NEST_BLOCK)), dim3(NEST_BLOCK), 0, c->stream, ncx, ncy, p->G.Nx, p->A.n, dix0, dix1, dwx, diy0, diy1,
                       dwy, (const double *)p->A.state, c->A.state);
    HIPCHK(c, hipGetLastError());
    /* the parent's next step overwrites the State this kernel reads: its stream goes on behind it */
    HIPCHK(c, hipEventRecord(c->ev_ctx, c->stream));
    HIPCHK(c, hipStreamWaitEvent(p->stream, c->ev_ctx, 0));
    c->state_zero = false;
    return picles_remesh(c, dt);
}

/* a child moved across its parent (include/picles_hip.h) */
PX_EXPORT int32_t picles_nest_relocate(picles_ctx *c, picles_ctx *p, int32_t si, int32_t sj, int32_t keep_margin, const int32_t *ix0,
                                       const int32_t *ix1, const double *wx, const int32_t *iy0, const int32_t *iy1, const double *wy, double dt,
                                       double mesh_x0, double mesh_y0)
{
    if (!c) return -1;
    const char *const who = "picles_nest_relocate";
    const std::string W = std::string(who) + ": ";
    if (!p) return fail(c, -2, W + "no parent context given");
    if (c == p) return fail(c, -2, W + "child and parent are the same context: a child is moved across another model");
    if (c->device != p->device)
        return fail(c, -5, W + "child on device " + std::to_string(c->device) + ", parent on device " + std::to_string(p->device) +
                           ": create both contexts on one device");
    if (!c->G.single_slab || c->ring || !p->G.single_slab || p->ring)
        return fail(c, -5, W + "slabs, slab mode and the native ring do not nest: both contexts must be whole-grid contexts");
    if (c->ext_streams || p->ext_streams) return fail(c, -5, std::string(who) + NEST_NO_EXT_STREAMS);
    if (!p->seeded) return fail(c, -2, W + "the parent was never seeded: it holds no sea state to expose a child to");
    if (!c->seeded) return fail(c, -2, W + "the child was never seeded: it holds no sea state to keep (picles_nest_prolong starts a child)");
    if (!(dt > 0.0)) return fail(c, -2, W + "dt must be positive (the child's step: the remesh and a lattice's first window use it)");
    if (keep_margin < 0) return fail(c, -2, W + "keep_margin must be >= 0 (the nodes dropped along the old box's rim)");
    if (c->clock != p->clock) {
        char buf[200];
        snprintf(buf, sizeof buf, "picles_nest_relocate: the child's clock (%.17g) and the parent's (%.17g) differ: a box moves between two legs, on a common clock",
                 c->clock, p->clock);
        return fail(c, -2, buf);
    }
    if (c->nest || c->bf_n || c->fb || c->stat_on)
        return fail(c, -5, W + "the child still holds a " + (c->fb ? "feedback" : c->nest ? "nest" : c->bf_n ? "forcing set" : "statistics set") +
                           ": its nodes would keep their indices and lose their places (end the leg first: picles_nest_free, picles_bforce_free, "
                           "picles_stat_free)");
    if (c->fm_on && c->fm_samples > 0)
        return fail(c, -2, W + "the child's flux-mean set holds " + std::to_string(c->fm_samples) + " samples, whose cells would mean another place "
                           "after the move: picles_flux_mean_push or picles_flux_mean_reset first");
    if (c->G.periodic_x || c->G.periodic_y || c->G.tripolar) return fail(c, -5, W + "the child has a periodic axis: only an open box moves");
    if (c->A.m11) return fail(c, -5, W + "the child has a metric set (picles_set_metric): its planes belong to the old position");
    if (c->wind.streamed()) return fail(c, -5, W + "the child runs under a wind stream: its ring holds levels sampled for the old position's lattice window");
    if (c->first_land >= 0)
        return fail(c, -5, W + "the child's mask has land nodes (node " + std::to_string(c->first_land) + " is of class " +
                           std::to_string((int)c->h_mask[(size_t)c->first_land]) + "): the mask is index space and would travel with the box");
    if (!ix0 || !ix1 || !wx || !iy0 || !iy1 || !wy) return fail(c, -2, W + "the six tables ix0, ix1, wx, iy0, iy1, wy must be given");
    const int ncx = c->G.Nx, ncy = c->G.Ny;
    { int rc = prolong_axis_check(c, "column", ncx, p->G.Nx, ix0, ix1, wx, who); if (rc) return rc; }
    { int rc = prolong_axis_check(c, "row", ncy, p->G.Ny, iy0, iy1, wy, who); if (rc) return rc; }
    { int rc = prolong_tab_upload(c, ix0, ix1, wx, iy0, iy1, wy); if (rc) return rc; }
    const size_t nd = (size_t)ncx + ncy;
    {   /* both States at the common clock, whole: the pending steps completed, each on its own stream */
        const std::string keep = p->err;
        int rc = flush(p);
        if (rc) { const std::string why = p->err; p->err = keep; return fail(c, rc, W + "the parent's pending step: " + why); }
        if ((rc = flush(c))) return rc;
    }
    HIPCHK(c, hipEventRecord(p->ev_ctx, p->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, p->ev_ctx, 0));
    const double *dwx = c->prolong_tab, *dwy = dwx + ncx;
    const int *dix0 = (const int *)(c->prolong_tab + nd), *dix1 = dix0 + ncx, *diy0 = dix1 + ncx, *diy1 = diy0 + ncy;
    /* into MovieState: an in-place shift races with itself, and the seed below writes State */
    hipLaunchKernelGGL(k_nest_relocate, dim3(nblocks(c->A.n, NEST_BLOCK)), dim3(NEST_BLOCK), 0, c->stream, ncx, ncy, (int)si, (int)sj, (int)keep_margin,
                       p->G.Nx, p->A.n, dix0, dix1, dwx, diy0, diy1, dwy, (const double *)p->A.state, (const double *)c->A.state, c->A.movie);
    HIPCHK(c, hipGetLastError());
    /* the parent's next step overwrites the State this kernel reads: its stream goes on behind it */
    HIPCHK(c, hipEventRecord(c->ev_ctx, c->stream));
    HIPCHK(c, hipStreamWaitEvent(p->stream, c->ev_ctx, 0));
    if (c->wind.from_lattice()) {      /* the lattice stays where it is in the common frame: the mesh moves under it */
        c->wind.wg.mesh_x0 = mesh_x0;
        c->wind.wg.mesh_y0 = mesh_y0;
        c->wind.invalidate();
    }
    /* what picles_seed resets, at the common clock and under the wind at the new nodes; then the relocated State and its particles */
    { int rc = seed_at(c, c->clock, c->clock, dt); if (rc) return rc; }
    /* no step of the box at its new place has been taken: a restart blob reads as that of a context seeded there (nothing reads
     * either before the next step sets them) */
    c->step_dt = 0.0;
    c->step_flags = 0;
    HIPCHK(c, hipMemcpyAsync(c->A.state, c->A.movie, 3 * (size_t)c->A.n * 8, hipMemcpyDeviceToDevice, c->stream));
    c->state_zero = false;
    return picles_remesh(c, dt);
}

PX_EXPORT int32_t picles_nest_feedback_init(picles_ctx *c, int32_t n_fb, const int32_t *fb_ij, int32_t n_src, const int32_t *src_ij, int32_t m,
                                            const int32_t *index, const double *weight)
{
    if (!c) return -1;
    if (c->fb) return fail(c, -2, "picles_nest_feedback_init: this context feeds back already (picles_nest_feedback_free first)");
    Nest *N = c->nest;
    if (!N) return fail(c, -2, "picles_nest_feedback_init: the child holds no nest: picles_nest_init first (feedback goes to the parent of a nest)");
    picles_ctx *p = N->parent;
    if (!p) return fail(c, -2, "picles_nest_feedback_init: the parent context was destroyed");
    if (p->bf_n)
        return fail(c, -5, p->fb_child ? "picles_nest_feedback_init: the parent is fed by another child: one child per parent feeds back"
                                       : "picles_nest_feedback_init: the parent holds a boundary forcing set of its own; a context carries one set, and feedback "
                                         "is one: not supported together (picles_bforce_free on the parent first)");
    if (c->ext_streams || p->ext_streams) return fail(c, -5, std::string("picles_nest_feedback_init") + NEST_NO_EXT_STREAMS);
    if (n_fb < 1 || !fb_ij) return fail(c, -2, "picles_nest_feedback_init: n_fb must be >= 1 and fb_ij given");
    if (n_src < 1 || m < 1 || !src_ij || !index || !weight)
        return fail(c, -2, "picles_nest_feedback_init: n_src and m must be >= 1 and src_ij, index and weight given");
    { int rc = stencil_check(c, FEEDBACK_RULES, c->G, n_fb, n_src, m, src_ij, index, weight); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->device));
    Feedback *F = new Feedback;
    c->fb = F;                                /* (no parent yet: a failure below drops without touching p) */
    Undo undo{[c] { fb_drop(c); }};
    { int rc = F->st.upload(c, FEEDBACK_RULES, n_fb, n_src, m, src_ij, index, weight); if (rc) return rc; }
    { int rc = F->sync.create(c, 2); if (rc) return rc; }
    /* the parent's set, last: what it refuses (a node off the grid, given twice or not of class 1; a tripolar grid) leaves both contexts as they were */
    {
        const std::string keep = p->err;
        int rc = bforce_init_any(p, n_fb, fb_ij, nullptr, BF_FEEDBACK);
        if (rc) {
            const std::string why = p->err;
            p->err = keep;
            return fail(c, rc, why);
        }
    }
    F->slot[0] = p->bf_lv;
    F->slot[1] = p->bf_lv + (size_t)3 * n_fb;
    F->parent = p;
    p->fb_child = c;
    undo.armed = false;
    return 0;
}

PX_EXPORT int32_t picles_nest_feedback(picles_ctx *c)
{
    if (!c) return -1;
    Feedback *F = c->fb;
    if (!F) return fail(c, -2, "picles_nest_feedback: picles_nest_feedback_init first");
    picles_ctx *p = F->parent;
    if (!p) return fail(c, -2, "picles_nest_feedback: the parent context was destroyed (its set went with it): picles_nest_feedback_free");
    if (c->ext_streams || p->ext_streams) return fail(c, -5, std::string("picles_nest_feedback") + NEST_NO_EXT_STREAMS);
    /* the slack rule of the window check: within 1e-9 of the child's step length; before any step the clocks must be equal */
    if (!(std::fabs(c->clock - p->clock) <= 1e-9 * c->step_dt)) {
        char b[256];
        snprintf(b, sizeof b, "picles_nest_feedback: the child's clock (%.17g) and the parent's (%.17g) differ: a feedback is taken where both "
                              "models stand at the same time", c->clock, p->clock);
        return fail(c, -2, b);
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int w = 1 - F->cur;
    hipStream_t s = c->stream;
    { int rc = F->sync.claim(c, w, s); if (rc) return rc; }
    { int rc = F->st.run(c, c, s, F->slot[w]); if (rc) return rc; }
    { int rc = F->sync.published(c, s); if (rc) return rc; }
    F->cur = w;
    F->taken++;
    p->bf_v0 = F->slot[w];
    p->bf_levels = 1;                         /* one level, constant: the parent's next step bears its feedback particles from it as it is */
    p->bf_t0 = p->bf_t1 = c->clock;
    return 0;
}

PX_EXPORT int32_t picles_nest_feedback_info(const picles_ctx *c, int32_t *n_fb, int32_t *n_src, int32_t *m, int64_t *taken)
{
    if (!c || !c->fb) return -1;
    if (n_fb) *n_fb = c->fb->st.n_out;
    if (n_src) *n_src = c->fb->st.n_src;
    if (m) *m = c->fb->st.m;
    if (taken) *taken = c->fb->taken;
    return 0;
}

PX_EXPORT int32_t picles_nest_feedback_free(picles_ctx *c)
{
    if (!c) return -1;
    if (!c->fb) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    return fb_release(c);
}

/* ---- halo blocks ---- */
PX_EXPORT int32_t picles_halo_rows(const picles_ctx *c) { return c ? c->G.R : -1; }

PX_EXPORT int32_t picles_set_halo_rows(picles_ctx *c, int32_t r)
{
    if (!c || r < 1 || r > 1024) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->G.single_slab && ((c->G.periodic_y && c->G.Ny <= 2 * r) || c->G.ny_loc < r))
        return fail(c, -2, "slab: periodic y axis not longer than 2*halo_rows, or fewer own rows than halo_rows");
    { int rc = flush(c); if (rc) return rc; }
    /* the whole device, not only the context stream: after picles_slab_run_steps the scatter of the last (un-fused) step is
     * still queued on the ring's streams, and the records it reads are about to be re-packed and freed */
    HIPCHK(c, hipDeviceSynchronize());
    /* keep the records of the own rows: re-pack into the new ghost-row geometry */
    int oldR = c->G.R;
    size_t row_b = (size_t)6 * c->G.Nx * 8;
    c->G.R = r;
    c->G.Rp = c->G.single_slab ? 0 : r;
    for (int k = 0; k < 2; k++) {
        double *old = c->rec_buf[k];
        c->rec_buf[k] = nullptr;
        HIPCHK(c, hipMalloc(&c->rec_buf[k], rec_bytes(c)));
        HIPCHK(c, hipMemsetAsync(c->rec_buf[k], 0, rec_bytes(c), c->stream));
        HIPCHK(c, hipMemcpyAsync((char *)c->rec_buf[k] + (size_t)r * row_b, (char *)old + (size_t)oldR * row_b,
                                 (size_t)c->G.ny_loc * row_b, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(old));
    }
    return class_map_zero(c);
}

PX_EXPORT int32_t picles_set_slab_mode(picles_ctx *c, int32_t on)
{
    if (!c) return -1;
    GridP &G = c->G;
    if (!(G.j_begin == 0 && G.ny_loc == G.Ny)) return on ? 0 : fail(c, -2, "a partial slab cannot resolve the y wrap locally");
    if (c->pending || c->seeded) return fail(c, -2, "picles_set_slab_mode: call before picles_seed");
    if (on && c->bf_n) return fail(c, -5, std::string("picles_set_slab_mode") + BFORCE_NO_SLABS);
    if (on && c->trk) return fail(c, -5, "picles_set_slab_mode: the context holds a track set (picles_track_free first): the corners of an event may lie on two slabs");
    if (on && !c->nest_children.empty()) return fail(c, -5, "picles_set_slab_mode: the context is the parent of a nest (picles_nest_free on its children first)");
    if (on && c->wind.streamed()) return fail(c, -5, "picles_set_slab_mode: the context holds a wind stream (picles_wind_stream_*), which slabs do not carry: picles_set_winds or picles_set_wind_grid first");
    if (on) {
        if ((G.periodic_y && G.Ny <= 2 * G.R) || G.ny_loc < G.R)
            return fail(c, -2, "slab: periodic y axis not longer than 2*halo_rows, or fewer own rows than halo_rows");
        if (G.tripolar) return fail(c, -5, "slab mode on a whole tripolar grid is not supported");
        G.single_slab = 0;
        G.Rp = G.R;
    } else {
        G.single_slab = 1;
        G.Rp = 0;
    }
    return 0;
}

static int halo_ptr(picles_ctx *c, int side, bool send, void **ptr, size_t *bytes)
{
    if (!c || !ptr || !bytes || side < 0 || side > 1) return -1;
    const GridP &G = c->G;
    if (G.ny_loc < G.R) return fail(c, -2, "slab has fewer rows than halo_rows");
    size_t row_b = (size_t)6 * G.Nx * 8;
    int row;
    if (send) row = (side == 0) ? G.R : G.ny_loc;          /* own first R rows / own last R rows */
    else row = (side == 0) ? 0 : G.ny_loc + G.R;            /* ghost rows below / above */
    *ptr = (char *)c->rec_buf[c->cur] + (size_t)row * row_b;   /* the step in flight (after picles_begin_step) */
    *bytes = (size_t)G.R * row_b;
    return 0;
}
PX_EXPORT int32_t picles_halo_send_dev(picles_ctx *c, int32_t side, void **ptr, size_t *bytes) { return halo_ptr(c, side, true, ptr, bytes); }
PX_EXPORT int32_t picles_halo_recv_dev(picles_ctx *c, int32_t side, void **ptr, size_t *bytes) { return halo_ptr(c, side, false, ptr, bytes); }

/* ------------------------------------------------------------------------------------------
 * Native slab ring: the multi-GPU model step with no interpreter in the loop.
 * RCCL is bound at run time (dlopen of librccl.so.1 — the copy already in the process if the host has
 * loaded one, e.g. PyTorch's): the library has no link-time dependency on it and single-GPU hosts never
 * touch it.  One communicator per context = per GPU = per process; rank r owns slab r of a y-ring.
 * Per model step:
 *     edge rows   k_step on stream E  ->  ncclGroup{Send hi->next, Send lo->prev, Recv lo<-prev, Recv hi<-next} on E
 *     interior    k_step on stream M      (overlaps the exchange)
 *     M waits for E (the halo has landed before the next step's launches pull from it)
 * The halo blocks are contiguous row ranges of the record buffer: sent and received in place.
 * The reference has no counterpart (TimeSteppers.jl:144-178 is a shared-memory @threads loop).
 * ---------------------------------------------------------------------------------------- */
#include <dlfcn.h>
#include <rccl/rccl.h>

struct RcclApi {
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    void *handle = nullptr;
};

/* RCCL by default (the copy torch.distributed has loaded, if any).  PICLES_CCL_LIB names another library that exports the same
 * eight entry points — an MPI-backed shim, or the thread loopback the tests use to run the ring with several ranks on one GPU. */
static RcclApi *rccl_api(std::string &err)
{
    static RcclApi api;
    static bool tried = false;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (api.handle) return &api;
    if (tried) { err = "the communication library could not be loaded"; return nullptr; }
    tried = true;
    void *h = nullptr;
    const char *over = getenv("PICLES_CCL_LIB");
    if (over && *over) {
        h = dlopen(over, RTLD_NOW | RTLD_LOCAL);
        if (!h) { err = std::string("dlopen(PICLES_CCL_LIB=") + over + "): " + dlerror(); return nullptr; }
    } else {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;    /* the copy already loaded, if any */
        if (!h) for (const char *n : names) if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) { err = std::string("dlopen(librccl.so.1): ") + dlerror(); return nullptr; }
    }
#define RSYM(f) do { api.f = (decltype(api.f))dlsym(h, "nccl" #f); if (!api.f) { err = "the communication library lacks nccl" #f; return nullptr; } } while (0)
    RSYM(GetUniqueId); RSYM(CommInitRank); RSYM(CommDestroy); RSYM(GroupStart); RSYM(GroupEnd); RSYM(Send); RSYM(Recv);
    RSYM(GetErrorString);
#undef RSYM
    api.handle = h;
    return &api;
}

struct SlabRing {
    RcclApi *api = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, prev = -1, next = -1;      /* -1: no neighbour on that side (open y axis) */
    hipStream_t sE = nullptr, sM = nullptr;
    hipEvent_t evE = nullptr, evM = nullptr, evEd = nullptr;      /* evEd: this step's edge launch alone (without the exchange behind it) */
    unsigned long long steps = 0, exchanged_bytes = 0;
    /* station probes of fused steps run on a side stream P that waits for the step's interior launch (evPm, stream M) and for its
     * exchange (evPx, stream E): neither M nor E waits for the other on the probe's account.  evP[b]: the latest probe that reads
     * record buffer b; the launches that overwrite the buffer two steps later wait for it (it completed long before) */
    hipStream_t sP = nullptr;
    hipEvent_t evPx = nullptr, evPm = nullptr, evP[2] = {nullptr, nullptr};
    bool evP_live[2] = {false, false};
    /* phase timing (picles_slab_get_phases): five events per step while per-launch timing is on */
    struct PhaseEv { hipEvent_t e0, e1, x1, m0, m1; };
    std::vector<PhaseEv> ph_used, ph_free;
};

#define NCCLCHK(c, R, call)                                                                     \
    do {                                                                                        \
        ncclResult_t r_ = (call);                                                               \
        if (r_ != ncclSuccess) {                                                                \
            (c)->err = std::string(#call) + ": " + (R)->api->GetErrorString(r_);                \
            return -11;                                                                         \
        }                                                                                       \
    } while (0)

PX_EXPORT int32_t picles_slab_unique_id(void *id128)
{
    if (!id128) return -1;
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) { g_create_error = err; return -11; }
    ncclUniqueId id;
    ncclResult_t r = api->GetUniqueId(&id);
    if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + api->GetErrorString(r); return -11; }
    static_assert(sizeof(id) == PICLES_SLAB_ID_BYTES, "ncclUniqueId size");
    memcpy(id128, &id, sizeof(id));
    return 0;
}

PX_EXPORT int32_t picles_slab_comm_destroy(picles_ctx *c)
{
    if (!c) return -1;
    SlabRing *R = c->ring;
    if (!R) return 0;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    if (R->comm) R->api->CommDestroy(R->comm);
    if (R->evE) hipEventDestroy(R->evE);
    if (R->evM) hipEventDestroy(R->evM);
    if (R->evEd) hipEventDestroy(R->evEd);
    for (hipEvent_t e : {R->evPx, R->evPm, R->evP[0], R->evP[1]}) if (e) hipEventDestroy(e);
    if (R->sP) hipStreamDestroy(R->sP);
    for (auto *v : {&R->ph_used, &R->ph_free})
        for (auto &e : *v) { hipEventDestroy(e.e0); hipEventDestroy(e.e1); hipEventDestroy(e.x1); hipEventDestroy(e.m0); hipEventDestroy(e.m1); }
    if (R->sE) hipStreamDestroy(R->sE);
    if (R->sM) hipStreamDestroy(R->sM);
    delete R;
    c->ring = nullptr;
    return 0;
}

PX_EXPORT int32_t picles_slab_comm_init(picles_ctx *c, const void *id128, int32_t rank, int32_t world)
{
    if (!c || !id128) return -1;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, -2, "slab ring: need 0 <= rank < world");
    if (c->ring) return fail(c, -2, "slab ring already initialised");
    if (c->bf_n) return fail(c, -5, std::string("picles_slab_comm_init") + BFORCE_NO_SLABS);
    if (c->trk) return fail(c, -5, "picles_slab_comm_init: the context holds a track set (picles_track_free first): the corners of an event may lie on two slabs");
    if (!c->nest_children.empty()) return fail(c, -5, "picles_slab_comm_init: the context is the parent of a nest (picles_nest_free on its children first)");
    if (c->G.single_slab && world > 1) return fail(c, -2, "slab ring of several ranks needs slab contexts (j_begin, j_end)");
    if (c->G.tripolar) return fail(c, -5, "slab ring: the tripolar fold is not wired into the native ring (use picles_amd.parallel)");
    HIPCHK(c, hipSetDevice(c->device));
    std::string err;
    RcclApi *api = rccl_api(err);
    if (!api) return fail(c, -11, err);
    SlabRing *R = new SlabRing();
    R->api = api; R->rank = rank; R->world = world;
    const bool per = c->G.periodic_y;
    R->prev = (rank > 0) ? rank - 1 : (per ? world - 1 : -1);
    R->next = (rank < world - 1) ? rank + 1 : (per ? 0 : -1);
    if (c->G.single_slab) R->prev = R->next = -1;       /* a whole-grid context wraps locally: nothing to exchange */
    c->ring = R;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclResult_t r = api->CommInitRank(&R->comm, world, id, rank);
    if (r != ncclSuccess) {
        c->err = std::string("ncclCommInitRank: ") + api->GetErrorString(r);
        R->comm = nullptr;
        picles_slab_comm_destroy(c);
        return -11;
    }
    /* (stream priorities were tried for the edge chain and measured slower on MI355X: 0.65 vs 0.46 ms per step at 1448²) */
    HIPCHK(c, hipStreamCreateWithFlags(&R->sE, hipStreamNonBlocking));
    HIPCHK(c, hipStreamCreateWithFlags(&R->sM, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&R->evE, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&R->evM, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&R->evEd, hipEventDisableTiming));
    return 0;
}

/* the halo exchange of the step in flight, in place, on stream s */
static int ring_exchange(picles_ctx *c, SlabRing *R, hipStream_t s)
{
    if (R->prev < 0 && R->next < 0) return 0;
    void *s_lo, *s_hi, *r_lo, *r_hi;
    size_t b = 0;
    int rc;
    if ((rc = halo_ptr(c, 0, true, &s_lo, &b)) || (rc = halo_ptr(c, 1, true, &s_hi, &b)) ||
        (rc = halo_ptr(c, 0, false, &r_lo, &b)) || (rc = halo_ptr(c, 1, false, &r_hi, &b))) return rc;
    const size_t n = b / 8;
    /* order matters when prev == next (two ranks on a periodic axis, or the ring of one): sends [hi -> next, lo -> prev]
     * pair with the peer's recvs [lo <- prev, hi <- next] */
    NCCLCHK(c, R, R->api->GroupStart());
    if (R->next >= 0) NCCLCHK(c, R, R->api->Send(s_hi, n, ncclDouble, R->next, R->comm, s));
    if (R->prev >= 0) NCCLCHK(c, R, R->api->Send(s_lo, n, ncclDouble, R->prev, R->comm, s));
    if (R->prev >= 0) NCCLCHK(c, R, R->api->Recv(r_lo, n, ncclDouble, R->prev, R->comm, s));
    if (R->next >= 0) NCCLCHK(c, R, R->api->Recv(r_hi, n, ncclDouble, R->next, R->comm, s));
    NCCLCHK(c, R, R->api->GroupEnd());
    R->exchanged_bytes += (size_t)((R->next >= 0) + (R->prev >= 0)) * b;
    return 0;
}

PX_EXPORT int32_t picles_slab_exchange(picles_ctx *c)
{
    if (!c) return -1;
    SlabRing *R = c->ring;
    if (!R) return fail(c, -2, "picles_slab_comm_init first");
    if (c->bf_n) return fail(c, -5, std::string("picles_slab_exchange") + BFORCE_NO_SLABS);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    int rc = ring_exchange(c, R, R->sE);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(R->sE));
    return 0;
}

PX_EXPORT int32_t picles_slab_run_steps(picles_ctx *c, double dt, int32_t n_steps, int32_t flags)
{
    if (!c || n_steps < 0) return -1;
    SlabRing *R = c->ring;
    if (!R) return fail(c, -2, "picles_slab_comm_init first");
    if (c->bf_n) return fail(c, -5, std::string("picles_slab_run_steps") + BFORCE_NO_SLABS);
    if (!(dt > 0.0)) return fail(c, -2, "dt must be positive");
    if (flags & PICLES_STEP_ATOMIC) return fail(c, -5, "PICLES_STEP_ATOMIC is single-slab only");
    { int rc = probe_room(c, n_steps, "picles_slab_run_steps"); if (rc) return rc; }      /* up front: nothing has changed yet */
    HIPCHK(c, hipSetDevice(c->device));
    if ((c->probe_n || c->stat_on || c->fm_on) && !R->sP) {
        HIPCHK(c, hipStreamCreateWithFlags(&R->sP, hipStreamNonBlocking));
        for (hipEvent_t *e : {&R->evPx, &R->evPm, &R->evP[0], &R->evP[1]}) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    c->ext_streams = true;
    c->ring_orders = true;
    /* timing mode 2: ONE event pair around the whole call, on the stream of the interior launches (every step's edge launch and
     * exchange are ordered into it by events: the pair spans the steps); its launches are counted, not bracketed, and the phase
     * events stay away — per-launch pairs and the five phase events of mode 1 cost a slab of 2 M particles 9 % of its step
     * (0.306 -> 0.333 ms, DESIGN.md lab notes of round 4): the diagnosis runs in a pass of its own, outside the timed steps */
    const bool region = c->timing && c->timing_mode == 2 && n_steps > 0;
    if (region) {
        timing_begin(c, R->sM, 3);
        c->in_region = true;
        c->region_launches = 0;
    }
    struct Off {
        picles_ctx *c; SlabRing *R; bool region;
        ~Off() {
            c->ring_orders = false;
            if (region) {      /* also on an error path: the pair is closed and the context leaves the region */
                c->in_region = false;
                timing_end(c, R->sM);
                c->tim.advance_launches += (uint64_t)c->region_launches;
            }
        }
    } off{c, R, region};
    for (int k = 0; k < n_steps; k++) {
        /* the context stream (wind-lattice sampler of this step) must come after the previous step's launches on E and
         * M, and this step's launches after it (step_prologue: ev_ctx); a flush synchronises the device by itself */
        HIPCHK(c, hipEventRecord(R->evM, R->sM));
        if (c->wind.from_lattice()) {
            HIPCHK(c, hipEventRecord(R->evE, R->sE));
            HIPCHK(c, hipStreamWaitEvent(c->stream, R->evM, 0));
            HIPCHK(c, hipStreamWaitEvent(c->stream, R->evE, 0));
        }
        int fused = (flags == PICLES_STEP_ZERO_FIRST) ? picles_begin_fused_step(c, dt) : 1;
        if (fused < 0) return fused;
        if (fused == 1) { int rc = picles_begin_step(c, dt, flags); if (rc) return rc; }
        if (R->evP_live[c->cur]) {
            /* this step's launches overwrite the record buffer that the probe of two steps ago reads */
            HIPCHK(c, hipStreamWaitEvent(R->sE, R->evP[c->cur], 0));
            HIPCHK(c, hipStreamWaitEvent(R->sM, R->evP[c->cur], 0));
            R->evP_live[c->cur] = false;
        }
        /* the previous step's interior launch (stream M) wrote / read what the edge launch touches */
        HIPCHK(c, hipStreamWaitEvent(R->sE, R->evM, 0));
        const bool phases = c->timing && c->timing_mode == 1 && R->ph_used.size() < (1u << 16);
        SlabRing::PhaseEv pe{};
        if (phases) {
            if (!R->ph_free.empty()) { pe = R->ph_free.back(); R->ph_free.pop_back(); }
            else { hipEventCreate(&pe.e0); hipEventCreate(&pe.e1); hipEventCreate(&pe.x1); hipEventCreate(&pe.m0); hipEventCreate(&pe.m1); }
            HIPCHK(c, hipEventRecord(pe.e0, R->sE));
        }
        int rc = (fused == 0) ? picles_step_rows(c, PICLES_ROWS_EDGE, R->sE) : picles_advance_rows(c, PICLES_ROWS_EDGE, R->sE);
        if (rc) return rc;
        if (fused == 0) HIPCHK(c, hipEventRecord(R->evEd, R->sE));
        if (phases) HIPCHK(c, hipEventRecord(pe.e1, R->sE));
        if ((rc = ring_exchange(c, R, R->sE))) return rc;
        if (phases) { HIPCHK(c, hipEventRecord(pe.x1, R->sE)); HIPCHK(c, hipEventRecord(pe.m0, R->sM)); }
        rc = (fused == 0) ? picles_step_rows(c, PICLES_ROWS_INTERIOR, R->sM) : picles_advance_rows(c, PICLES_ROWS_INTERIOR, R->sM);
        if (rc) return rc;
        if (phases) { HIPCHK(c, hipEventRecord(pe.m1, R->sM)); R->ph_used.push_back(pe); }
        const bool probe = c->probe_n && c->probe_cad.due(c->probe_cad.steps + 1);
        const bool stat = c->stat_on && c->stat_cad.due(c->stat_cad.steps + 1);      /* the statistics update: ordered exactly as a probe */
        const bool fmean = c->fm_on && c->fm_cad.due(c->fm_cad.steps + 1);        /* the flux-mean update: likewise */
        const bool sample = probe || stat || fmean;
        if (sample && fused == 0) {      /* what the probe of a fused step waits for: the interior launch and the delivered halo */
            HIPCHK(c, hipEventRecord(R->evPm, R->sM));
            HIPCHK(c, hipEventRecord(R->evPx, R->sE));
        }
        if (fused == 0) {
            /* fused steps: what runs next on M is the next step's interior launch.  Its pull reads own rows only — the records the
             * edge launch of THIS step wrote among them — never the ghost rows: it waits for the edge kernel, not for the exchange
             * behind it.  The communication is off the interior's critical path altogether; only the next edge launch (same
             * stream as the exchange) consumes the received rows. */
            HIPCHK(c, hipStreamWaitEvent(R->sM, R->evEd, 0));
        } else {
            HIPCHK(c, hipEventRecord(R->evE, R->sE));
            HIPCHK(c, hipStreamWaitEvent(R->sM, R->evE, 0));      /* the scatter on M reads the edge rows and the received halo */
        }
        c->edge_pending = false;
        rc = (fused == 0) ? picles_end_fused_step(c) : picles_scatter_remesh(c, R->sM);
        if (rc) return rc;
        if (sample && fused == 0) {
            /* records: edge-row nodes are fed by the neighbour's records, so the probe needs the exchange as well as both launches
             * — on the side stream, so that stream M never waits for the exchange */
            HIPCHK(c, hipStreamWaitEvent(R->sP, R->evPm, 0));
            HIPCHK(c, hipStreamWaitEvent(R->sP, R->evPx, 0));
            if (probe && (rc = probe_take(c, R->sP))) return rc;
            if (stat && (rc = stat_update(c, R->sP))) return rc;
            if (fmean && (rc = flux_mean_update(c, R->sP, "picles_slab_run_steps"))) return rc;
            HIPCHK(c, hipEventRecord(R->evP[c->cur], R->sP));
            R->evP_live[c->cur] = true;
        } else if (sample) {
            if (probe && (rc = probe_take(c, R->sM))) return rc;      /* State is in memory: gathered on the stream that ran the scatter */
            if (stat && (rc = stat_update(c, R->sM))) return rc;
            if (fmean && (rc = flux_mean_update(c, R->sM, "picles_slab_run_steps"))) return rc;
        }
        R->steps++;
    }
    return 0;
}

PX_EXPORT int32_t picles_slab_get_phases(picles_ctx *c, picles_slab_phases *out)
{
    if (!c || !out) return -1;
    SlabRing *R = c->ring;
    if (!R) return fail(c, -2, "picles_slab_comm_init first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    picles_slab_phases P{};
    for (auto &e : R->ph_used) {
        float ed = 0.f, ex = 0.f, in = 0.f, sl = 0.f, se = 0.f, sm = 0.f;
        hipEventElapsedTime(&ed, e.e0, e.e1);
        hipEventElapsedTime(&ex, e.e1, e.x1);
        hipEventElapsedTime(&in, e.m0, e.m1);
        hipEventElapsedTime(&sl, e.x1, e.m1);      /* > 0: the interior launch ended after the exchange had completed */
        hipEventElapsedTime(&se, e.e0, e.x1);
        hipEventElapsedTime(&sm, e.e0, e.m1);
        P.steps++;
        if (sl >= 0.f) P.exchange_hidden++;
        P.edge_ms += ed; P.exchange_ms += ex; P.interior_ms += in; P.slack_ms += sl;
        P.span_ms += (se > sm) ? se : sm;
        R->ph_free.push_back(e);
    }
    R->ph_used.clear();
    *out = P;
    return 0;
}

PX_EXPORT int32_t picles_slab_streams(picles_ctx *c, void **edge, void **interior)
{
    if (!c || !c->ring) return -1;
    if (edge) *edge = c->ring->sE;
    if (interior) *interior = c->ring->sM;
    return 0;
}

/* ---- generic push_to_grid! of a particle list ---- */
PX_EXPORT int32_t picles_scatter_particles(picles_ctx *c, int64_t np, const int32_t *ij, const double *xy, const double *charge)
{
    if (!c || np < 0 || (np > 0 && (!ij || !xy || !charge))) return -1;
    if (!c->G.single_slab) return fail(c, -5, "picles_scatter_particles is single-slab only");
    if (c->G.tripolar) return fail(c, -5, "picles_scatter_particles does not implement the tripolar fold");
    if (np == 0) return 0;
    if (np > 0x7fffffffLL) return fail(c, -2, "too many particles for one call");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }
    hipStream_t s = c->stream;
    int ntx = (c->G.Nx + PT_TX - 1) / PT_TX, nty = (c->G.ny_loc + PT_TY - 1) / PT_TY;
    int ntiles = ntx * nty;
    int *d_ij = nullptr, *d_tile = nullptr, *d_perm = nullptr;
    double *d_xy = nullptr, *d_ch = nullptr;
    struct Tmp {   /* released on every exit path */
        int *&a, *&b, *&c2; double *&d, *&e;
        ~Tmp() { hipFree(a); hipFree(b); hipFree(c2); hipFree(d); hipFree(e); }
    } tmp{d_ij, d_tile, d_perm, d_xy, d_ch};
    HIPCHK(c, hipMalloc(&d_ij, 2 * np * 4)); HIPCHK(c, hipMalloc(&d_tile, np * 4)); HIPCHK(c, hipMalloc(&d_perm, np * 4));
    HIPCHK(c, hipMalloc(&d_xy, 2 * np * 8)); HIPCHK(c, hipMalloc(&d_ch, 3 * np * 8));
    if (!c->d_count) {
        HIPCHK(c, hipMalloc(&c->d_count, (ntiles + 1) * 4));
        HIPCHK(c, hipMalloc(&c->d_start, (ntiles + 1) * 4));
        HIPCHK(c, hipMalloc(&c->d_cursor, (ntiles + 1) * 4));
        hipcub::DeviceScan::ExclusiveSum(nullptr, c->scan_tmp_bytes, c->d_count, c->d_start, ntiles + 1, s);
        HIPCHK(c, hipMalloc(&c->d_scan_tmp, c->scan_tmp_bytes));
    }
    HIPCHK(c, hipMemcpyAsync(d_ij, ij, 2 * np * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_xy, xy, 2 * np * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_ch, charge, 3 * np * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(c->d_count, 0, (ntiles + 1) * 4, s));
    HIPCHK(c, hipMemsetAsync(c->d_cursor, 0, (ntiles + 1) * 4, s));
    hipLaunchKernelGGL(k_tile_count, dim3(nblocks(np, 256)), dim3(256), 0, s, c->G, ntx, d_ij, (long long)np, c->d_count, d_tile);
    HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(c->d_scan_tmp, c->scan_tmp_bytes, c->d_count, c->d_start, ntiles + 1, s));
    hipLaunchKernelGGL(k_tile_fill, dim3(nblocks(np, 256)), dim3(256), 0, s, (long long)np, d_tile, c->d_start, c->d_cursor, d_perm);
    timing_begin(c, s, 1);
    hipLaunchKernelGGL(k_push_tiles<false>, dim3(ntiles), dim3(256), 0, s, c->G, arrays_for(c, c->cur, c->cur), ntx, c->d_start, d_perm, d_ij, d_xy, d_ch, (long long)np);
    timing_end(c, s);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(s));
    c->state_zero = false;
    return 0;
}

/* ------------------------------------------------------------------------------------------
 * Exact restart: the checkpoint blob (picles_checkpoint_*).
 * blob = CkptHeader (256 bytes) + payload.  The payload is the context's planes, one segment each in a fixed order, every segment
 * starting at a multiple of 256 bytes and zero-padded up to the next:
 *   0 State (3 planes f64)   1 z (5 planes f64)   2 qold f64   3 dtn f64   4 asw i32   5 status i32   6 on u8   7 pflags u8
 *   8 the statistics slots + the 16 reach-counter words behind them (kernels.h: DevCounters, reach_counters)
 *   9 the five rotating local-reach maps (Arrays::rmap)
 * k_ckpt moves it between the planes and one contiguous device snapshot in a single pass over HBM (16-byte loads and stores,
 * one segment per grid row) and sums it on the way.  The sum: Σ over the payload's 16-byte chunks g of
 * mix(lo ^ 2g K) + mix(hi ^ (2g+1) K) mod 2^64 — independent of the order the chunks are visited in (the same bits for any dispatch),
 * bound to positions, and a changed word changes exactly one term (mix is a bijection), so any changed byte changes the sum.
 *   MODE 0: pack the planes into the snapshot, add its sum to sums[0]
 *   MODE 1: add the sum of the snapshot (a blob being loaded) to sums[0]
 *   MODE 2: unpack the snapshot into the planes — only where sums[0] == sums[1] (the verified sum and the header's)
 * ---------------------------------------------------------------------------------------- */
#define CKPT_NSEG 10
#define CKPT_MAGIC 0x31544b4353454c43ull      /* "CLESCKT1" little-endian */
#define CKPT_FORMAT 1
struct CkptSegs {
    unsigned char *ptr[CKPT_NSEG];            /* the context's plane */
    unsigned long long off[CKPT_NSEG];        /* its offset in the payload */
    unsigned long long len[CKPT_NSEG];        /* its length [bytes] */
    unsigned long long span[CKPT_NSEG];       /* its length padded to 256 bytes: off[k + 1] - off[k] */
};
struct CkptHeader {                           /* little-endian, 256 bytes; the offsets of the fields are part of the format */
    uint64_t magic;                           /*   0  CKPT_MAGIC                                                      */
    uint32_t format, abi;                     /*   8  CKPT_FORMAT, PICLES_ABI_VERSION                                 */
    uint64_t header_bytes, payload_bytes;     /*  16  sizeof(CkptHeader), the payload that follows                    */
    uint64_t fingerprint, checksum;           /*  32  configuration hash, payload sum (k_ckpt)                        */
    double   clock;                           /*  48  model time of the step boundary                                  */
    int32_t  halo_rows, mr_w;                 /*  56  ghost rows; index of the reach counter of the latest step        */
    int32_t  cur, nseg;                       /*  64  record buffer of the latest step; CKPT_NSEG                      */
    int64_t  n;                               /*  72  nodes = particles of the context's rows                          */
    uint64_t seg_off[CKPT_NSEG];              /*  80  segment offsets in the payload                                   */
    uint64_t seg_len[CKPT_NSEG];              /* 160  segment lengths                                                  */
    double   step_dt;                         /* 240  Δt of the latest step                                            */
    int32_t  state_zero, pad_;                /* 248  State known to be all zero                                       */
};
static_assert(sizeof(CkptHeader) == 256, "checkpoint header layout");

__device__ __forceinline__ unsigned long long ck_mix(unsigned long long x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

template <int MODE>
__global__ void __launch_bounds__(256) k_ckpt(CkptSegs S, unsigned char *snap, unsigned long long *sums)
{
    if (MODE == 2 && sums[0] != sums[1]) return;        /* not verified: nothing of the context is touched */
    const int s = blockIdx.y;
    unsigned char *seg = S.ptr[s];
    const unsigned long long len = S.len[s], nch = S.span[s] >> 4, nfull = len >> 4, g0 = S.off[s] >> 4;
    uint4 *sn = (uint4 *)(snap + S.off[s]);
    unsigned long long acc = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < nch; q += stride) {
        uint4 v;
        if (MODE == 0) {
            if (q < nfull) v = ((const uint4 *)seg)[q];
            else {                                        /* the segment's partial last chunk, and the zero padding behind it */
                unsigned int w[4] = {0u, 0u, 0u, 0u};
                for (int k = 0; k < 16; k++) {
                    const unsigned long long o = q * 16 + k;
                    if (o < len) w[k >> 2] |= (unsigned int)seg[o] << (8 * (k & 3));
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            sn[q] = v;
        } else {
            v = sn[q];
            if (MODE == 2) {
                if (q < nfull) ((uint4 *)seg)[q] = v;
                else {
                    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
                    for (int k = 0; k < 16; k++) {
                        const unsigned long long o = q * 16 + k;
                        if (o < len) seg[o] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
                    }
                }
            }
        }
        if (MODE != 2) {
            const unsigned long long g = g0 + q, K = 0x9e3779b97f4a7c15ull;
            const unsigned long long lo = ((unsigned long long)v.y << 32) | v.x, hi = ((unsigned long long)v.w << 32) | v.z;
            acc += ck_mix(lo ^ (2 * g) * K) + ck_mix(hi ^ (2 * g + 1) * K);
        }
    }
    if (MODE != 2) {
        acc = wave_sum_u64(acc);                          /* kernels.h: every lane of the wave is here */
        if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sums, acc);
    }
}

static unsigned long long ckpt_layout(picles_ctx *c, CkptSegs &S)
{
    Arrays &A = c->A;
    const unsigned long long n = (unsigned long long)A.n;
    struct { void *p; unsigned long long len; } seg[CKPT_NSEG] = {
        {A.state, 24 * n}, {A.z, 40 * n}, {A.qold, 8 * n}, {A.dtn, 8 * n}, {A.asw, 4 * n}, {A.status, 4 * n}, {A.on, n}, {A.pflags, n},
        {A.cnt, NSLOTS * sizeof(DevCounters) + 16 * sizeof(int)}, {A.rmap, (unsigned long long)5 * A.ntile * sizeof(int)}};
    unsigned long long off = 0;
    for (int k = 0; k < CKPT_NSEG; k++) {
        S.ptr[k] = (unsigned char *)seg[k].p;
        S.off[k] = off;
        S.len[k] = seg[k].len;
        S.span[k] = (seg[k].len + 255) & ~255ull;
        off += S.span[k];
    }
    return off;
}

/* what the blob is checked against: the configuration the restoring program builds from its script */
static uint64_t ckpt_fingerprint(const picles_ctx *c)
{
    uint64_t h = FP_SEED;
    const picles_grid &g = c->g;
    h = fp_val(h, g.Nx); h = fp_val(h, g.Ny); h = fp_val(h, g.dx); h = fp_val(h, g.dy);
    h = fp_val(h, g.periodic_x); h = fp_val(h, g.periodic_y); h = fp_val(h, g.j_begin); h = fp_val(h, g.j_end);
    const picles_phys &p = c->ph;
    for (double v : {p.r_g, p.C_alpha, p.C_phi, p.C_e, p.g, p.gamma, p.q, p.c_beta, p.c_D, p.c_e, p.c_alpha, p.dir_deadband}) h = fp_val(h, v);
    for (int32_t v : {p.propagation, p.input, p.dissipation, p.peak_shift, p.direction}) h = fp_val(h, v);
    const picles_ode &o = c->od;
    for (double v : {o.abstol, o.reltol, o.dt0, o.dtmin, o.log_energy_minimum, o.log_energy_maximum, o.wind_min_squared, o.timestep}) h = fp_val(h, v);
    h = fp_val(h, o.force_dtmin); h = fp_val(h, o.solver); h = fp_val(h, o.maxiters);
    const picles_model &m = c->md;
    h = fp_val(h, m.periodic_boundary); h = fp_val(h, m.init_type);
    for (int k = 0; k < 3; k++) h = fp_val(h, m.default_particle[k]);
    for (int k = 0; k < 2; k++) h = fp_val(h, m.minimal_state[k]);
    h = fp_bytes(h, c->h_mask.data(), c->h_mask.size());
    h = fp_val(h, c->G.single_slab); h = fp_val(h, c->halo0);
    h = fp_val(h, (int32_t)(c->A.m11 != nullptr)); h = fp_val(h, c->fp_metric);
    if (c->wind.streamed()) {      /* a wind stream: its geometry, time axis, mode and ring size — not its contents */
        const WindGrid &w = c->wind.wg;
        h = fp_bytes(h, "stream", 6);
        h = fp_val(h, c->wind.mode); h = fp_val(h, w.nx); h = fp_val(h, w.ny); h = fp_val(h, c->wind.ring_slots);
        for (double v : {w.x0, w.inv_dx, w.y0, w.inv_dy, c->wind.lat_t0, c->wind.lat_dt, w.mesh_x0, w.mesh_y0}) h = fp_val(h, v);
        return h;
    }
    h = fp_val(h, (int32_t)c->wind.from_lattice());
    if (c->wind.from_lattice()) {
        const WindGrid &w = c->wind.wg;
        h = fp_val(h, c->wind.mode); h = fp_val(h, w.nx); h = fp_val(h, w.ny); h = fp_val(h, w.nt);
        for (double v : {w.x0, w.inv_dx, w.y0, w.inv_dy, c->wind.lat_t0, c->wind.lat_dt, w.mesh_x0, w.mesh_y0}) h = fp_val(h, v);
        h = fp_val(h, c->fp_lattice);
    }
    return h;
}

/* the device snapshot (payload + two sum words) and its pinned host copy, allocated on first use; the copy-out rides on the store stream */
static int ckpt_buffers(picles_ctx *c, unsigned long long payload)
{
    const size_t need = (size_t)payload + 16;
    { int rc = store_stream_get(c); if (rc) return rc; }
    if (!c->ck_ready) {
        HIPCHK(c, hipEventCreateWithFlags(&c->ck_ready, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ck_done, hipEventDisableTiming));
    }
    if (c->ck_cap >= need) return 0;
    if (c->ck_dev) { HIPCHK(c, hipFree(c->ck_dev)); c->ck_dev = nullptr; }
    if (c->ck_host) { HIPCHK(c, hipHostFree(c->ck_host)); c->ck_host = nullptr; }
    c->ck_cap = 0;
    HIPCHK(c, hipMalloc(&c->ck_dev, need));
    HIPCHK(c, hipHostMalloc(&c->ck_host, need, hipHostMallocDefault));
    c->ck_cap = need;
    return 0;
}

static void ckpt_launch(picles_ctx *c, int mode, const CkptSegs &S, unsigned long long payload)
{
    unsigned long long maxch = 0;
    for (int k = 0; k < CKPT_NSEG; k++) maxch = std::max(maxch, S.span[k] >> 4);
    const unsigned gx = (unsigned)std::min<unsigned long long>((maxch + 255) / 256, 2048);
    dim3 grid(gx ? gx : 1, CKPT_NSEG), block(256);
    unsigned long long *sums = (unsigned long long *)(c->ck_dev + payload);
    if (mode == 0) hipLaunchKernelGGL(k_ckpt<0>, grid, block, 0, c->stream, S, c->ck_dev, sums);
    else if (mode == 1) hipLaunchKernelGGL(k_ckpt<1>, grid, block, 0, c->stream, S, c->ck_dev, sums);
    else hipLaunchKernelGGL(k_ckpt<2>, grid, block, 0, c->stream, S, c->ck_dev, sums);
}

PX_EXPORT int32_t picles_checkpoint_size(picles_ctx *c, size_t *bytes)
{
    if (!c || !bytes) return -1;
    CkptSegs S;
    *bytes = sizeof(CkptHeader) + (size_t)ckpt_layout(c, S);
    return 0;
}

PX_EXPORT int32_t picles_checkpoint_begin(picles_ctx *c)
{
    if (!c) return -1;
    if (c->ck_inflight) return fail(c, PICLES_CKPT_E_BUSY, "picles_checkpoint_begin: a checkpoint is in flight (picles_checkpoint_end first)");
    if (!c->seeded) return fail(c, -2, "picles_checkpoint_begin: nothing to save (picles_seed or picles_checkpoint_load first)");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = flush(c); if (rc) return rc; }          /* State at the step boundary: no step is left pending */
    if (c->ext_streams) HIPCHK(c, hipDeviceSynchronize());   /* an un-fused slab step leaves its scatter on the ring's stream M */
    CkptSegs S;
    const unsigned long long payload = ckpt_layout(c, S);
    { int rc = ckpt_buffers(c, payload); if (rc) return rc; }
    unsigned long long *sums = (unsigned long long *)(c->ck_dev + payload);
    HIPCHK(c, hipMemsetAsync(sums, 0, 16, c->stream));
    timing_begin(c, c->stream, 4);
    ckpt_launch(c, 0, S, payload);
    timing_end(c, c->stream);
    HIPCHK(c, hipGetLastError());
    /* stream-ordered behind the pack; the D2H leg runs beside whatever the caller enqueues next (as picles_store_push) */
    { int rc = ship_d2h(c, c->stream, c->ck_ready, c->ck_done, c->ck_host, c->ck_dev, (size_t)payload + 8); if (rc) return rc; }
    CkptHeader h;
    memset(&h, 0, sizeof h);
    h.magic = CKPT_MAGIC; h.format = CKPT_FORMAT; h.abi = PICLES_ABI_VERSION;
    h.header_bytes = sizeof(CkptHeader); h.payload_bytes = payload;
    h.fingerprint = ckpt_fingerprint(c);
    h.clock = c->clock;
    h.halo_rows = c->G.R; h.mr_w = c->mr_w; h.cur = c->cur; h.nseg = CKPT_NSEG;
    h.n = c->A.n;
    for (int k = 0; k < CKPT_NSEG; k++) { h.seg_off[k] = S.off[k]; h.seg_len[k] = S.len[k]; }
    h.step_dt = c->step_dt;
    h.state_zero = c->state_zero ? 1 : 0;
    memcpy(c->ck_hdr, &h, sizeof h);
    c->ck_inflight = true;
    return 0;
}

PX_EXPORT int32_t picles_checkpoint_end(picles_ctx *c, void *buf, size_t bytes)
{
    if (!c) return -1;
    if (!c->ck_inflight) return fail(c, -2, "picles_checkpoint_end: no checkpoint in flight (picles_checkpoint_begin first)");
    CkptHeader h;
    memcpy(&h, c->ck_hdr, sizeof h);
    const size_t total = sizeof h + (size_t)h.payload_bytes;
    if (!buf || bytes < total) {
        char m[160];
        snprintf(m, sizeof m, "picles_checkpoint_end: the blob needs %zu bytes, the buffer has %zu", total, buf ? bytes : (size_t)0);
        return fail(c, PICLES_CKPT_E_SHORT, m);         /* (still in flight: call again with a large enough buffer) */
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ck_done));
    memcpy(&h.checksum, c->ck_host + h.payload_bytes, 8);
    memcpy(buf, &h, sizeof h);
    memcpy((unsigned char *)buf + sizeof h, c->ck_host, (size_t)h.payload_bytes);
    c->ck_inflight = false;
    return 0;
}

PX_EXPORT int32_t picles_checkpoint_load(picles_ctx *c, const void *buf, size_t bytes)
{
    if (!c || !buf) return -1;
    if (c->probe.count > 0)
        return fail(c, PICLES_CKPT_E_BUSY, "picles_checkpoint_load: probe samples of this context are pending (picles_probe_pop first)");
    if (c->ck_inflight || c->store.count > 0 || c->diag_ring.count > 0 || c->flux_ring.count > 0)
        return fail(c, PICLES_CKPT_E_BUSY, "picles_checkpoint_load: a checkpoint or store snapshot of this context is in flight (end / pop it first)");
    CkptHeader h;
    if (bytes < sizeof h) return fail(c, PICLES_CKPT_E_SHORT, "picles_checkpoint_load: buffer shorter than a checkpoint header");
    memcpy(&h, buf, sizeof h);
    if (h.magic != CKPT_MAGIC) return fail(c, PICLES_CKPT_E_MAGIC, "picles_checkpoint_load: not a checkpoint blob (bad magic)");
    if (h.format != CKPT_FORMAT || h.abi != PICLES_ABI_VERSION || h.header_bytes != sizeof h) {
        char m[200];
        snprintf(m, sizeof m, "picles_checkpoint_load: blob format %u / ABI %u, this library reads format %d / ABI %d", h.format, h.abi,
                 CKPT_FORMAT, PICLES_ABI_VERSION);
        return fail(c, PICLES_CKPT_E_VERSION, m);
    }
    if (bytes - sizeof h < h.payload_bytes) {
        char m[200];
        snprintf(m, sizeof m, "picles_checkpoint_load: truncated blob (%zu payload bytes of %llu)", bytes - sizeof h, (unsigned long long)h.payload_bytes);
        return fail(c, PICLES_CKPT_E_SHORT, m);
    }
    CkptSegs S;
    const unsigned long long payload = ckpt_layout(c, S);
    bool same = h.fingerprint == ckpt_fingerprint(c) && h.payload_bytes == payload && h.n == c->A.n && h.nseg == CKPT_NSEG;
    for (int k = 0; same && k < CKPT_NSEG; k++) same = h.seg_off[k] == S.off[k] && h.seg_len[k] == S.len[k];
    if (!same) return fail(c, PICLES_CKPT_E_CONFIG, "picles_checkpoint_load: the blob was written by a model of another configuration "
                                                    "(grid, mask, physics, ODE settings, metric, wind lattice or wind stream, slab rows or slab mode differ)");
    const GridP &G = c->G;
    const int R = h.halo_rows;
    if (R < 1 || R > 1024 || (!G.single_slab && ((G.periodic_y && G.Ny <= 2 * R) || G.ny_loc < R)) || h.mr_w < 0 || h.mr_w > 4 || (h.cur & ~1))
        return fail(c, PICLES_CKPT_E_CONFIG, "picles_checkpoint_load: the blob's halo rows / counter indices do not fit this context");
    HIPCHK(c, hipSetDevice(c->device));
    { int rc = ckpt_buffers(c, payload); if (rc) return rc; }
    /* verify on the device before anything of the context is touched: the snapshot buffer is scratch */
    unsigned long long *sums = (unsigned long long *)(c->ck_dev + payload);
    const unsigned long long want[2] = {0ull, (unsigned long long)h.checksum};
    HIPCHK(c, hipMemcpyAsync(c->ck_dev, (const unsigned char *)buf + sizeof h, (size_t)payload, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(sums, want, 16, hipMemcpyHostToDevice, c->stream));
    ckpt_launch(c, 1, S, payload);
    HIPCHK(c, hipGetLastError());
    unsigned long long got = 0;
    HIPCHK(c, hipMemcpyAsync(&got, sums, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (got != h.checksum) return fail(c, PICLES_CKPT_E_CHECKSUM, "picles_checkpoint_load: payload checksum mismatch (the blob is damaged)");
    /* commit: a step still pending is superseded (everything it would write is replaced) */
    HIPCHK(c, hipDeviceSynchronize());
    c->pending = false;
    if (R != G.R) { int rc = picles_set_halo_rows(c, R); if (rc) return rc; }
    ckpt_launch(c, 2, S, payload);
    HIPCHK(c, hipGetLastError());
    { int rc = class_map_zero(c); if (rc) return rc; }      /* the map is not part of a checkpoint: it changes speed, never results */
    /* the flags plane of the blob is the writer's; this context keeps its own: a band set that lives here leaves its ocean nodes
     * unstepped, one that lived there does not reach here */
    { int rc = context_pflags(c); if (rc) return rc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->clock = h.clock;
    c->step_dt = h.step_dt;
    c->pend_t = h.clock; c->pend_dt = h.step_dt;
    c->mr_w = h.mr_w;
    c->cur = h.cur;
    c->state_zero = h.state_zero != 0;
    c->seeded = true;
    c->edge_pending = false;
    c->ord_valid = false;     /* the dispatch order is scheduling only: the first fused step after a load runs in natural order */
    c->wind.invalidate();     /* a lattice window is sampled afresh (the same bits: the sampler is a function of the time alone) */
    return 0;
}
