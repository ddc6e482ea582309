/* k_bforce.hip — open-boundary forcing: the particles of the forced nodes (picles_bforce_*, include/picles_hip.h) */
/* The step kernels do not step a node without PF_STEPPED: the grid-boundary nodes of a model without periodic_boundary (mask class 3),
 * and the ocean nodes of a band set (picles_bforce_init_band clears the flag of its class-1 nodes while the set lives), and no
 * kernel reads or writes their particle slots or their records.  k_bforce runs behind whichever launch writes the records of
 * a step for the whole grid (k_step, k_step_waverow, k_advance), on the same stream, and does for every forced node what those do for
 * a stepped one: a particle is born from the prescribed (e, m_x, m_y) at the step's start time, advanced over the step by the model's
 * own solver under the node's wind, and leaves its scatter record in the buffer the step writes.
 *
 * What it shares with the step kernels, and how it keeps their bookkeeping (kernels.h):
 *   reach      flush_stats raises the reach map entry of the node's tile and the rotating reach counter of the generation being
 *              written: a swell particle may travel farther than anything the step kernel saw in that tile
 *   class map  the entry of every tile it writes a record into is zeroed in the generation being written (a k_step_waverow launch
 *              in front of it may just have filed "all 64 records carry code c" for that tile)
 *   clears     rmap_clear_ahead and the cost-ordered dispatch are the step kernels' business: not touched (every wave that reaches
 *              flush_stats has advanced a particle, so none of them files the "calm wave" word order_wanted reads)
 *   sum order  a record carries list code 1 (ocean), GridP::ngroups stays 1, and the pull visits the forced particles in the plain
 *              column-major order of all records — there is no second list
 *   statistics the counters of the context count these particles like any others
 * General-physics flavours only (FAST = false, STATIC = false: the same bits as the specialised ones, every wind window carried,
 * polylines included), by solver and by metric.  One lane per forced node: a rim is a few thousand, a three-deep band on a 4096²
 * box about 49,000 — 192 workgroups, still less than one per compute unit, so the launch stays latency-bound at about one RK
 * integration, and occupancy beyond the two workgroups per compute unit the bounds ask for would buy nothing: the bounds stay.
 * Behind the RK loop the arguments are read again (k_advance.hip has the reasons); the lane's node index comes from the list
 * again, so nothing waits in LDS.
 *
 * BLEND (a set with a weight below 1): the prescribed value p is mixed into the model's own State m of the node at
 * the step's start, v = m + w (p - m) per component, three IEEE operations, and the birth test is made on v.  m is k_probe's value
 * (k_probe.h): the pull over the records of the pending fused step where the launch in front scatters one (B.from_rec: A.rec and
 * the reach indices are that launch's own), State in memory otherwise.  A lane with w == 1.0 pulls nothing: v is p to the bit.
 * The flavours without BLEND are instantiated apart and do not know about any of this. */
#include "kernels.h"

/* the kernel arguments as the kernarg segment lays them out (kargs_reload, kernels.h) */
struct BForceArgs {
    KParams P;
    GridP G;
    Arrays A;
    BForceP B;
    double t_start, DT;
};
static_assert(__builtin_offsetof(BForceArgs, G) == sizeof(KParams) && __builtin_offsetof(BForceArgs, A) % 8 == 0 &&
              __builtin_offsetof(BForceArgs, B) == __builtin_offsetof(BForceArgs, A) + sizeof(Arrays) &&
              __builtin_offsetof(BForceArgs, t_start) == __builtin_offsetof(BForceArgs, B) + sizeof(BForceP),
              "BForceArgs must mirror the kernarg layout of k_bforce");

template <bool METRIC, bool TSIT, bool AUTO, bool BLEND>
__global__ void __launch_bounds__(256, 2) k_bforce(KParams P, GridP G, Arrays A, BForceP B, double t_start, double DT)
{
    dp_device_init(TSIT ? 1 : 0);
    pm_device_init();
    const int k = (int)(blockIdx.x * PICLES_BLOCK + threadIdx.x);
    const bool active = k < B.n;
    StepStats S = {{0u, 0u, 0u, 0}, 0u, 0u, 0u, 0u, 0u, 0u, 0};
    int rtile = -1;
    Vec5 z = {0.0, 0.0, 0.0, 0.0, 0.0};
    int on = 0, status = 0, asw = ASW_FRESH;
    double qold = PI_LNQOLDINIT, dtn = -1.0;      /* the controller memory of a freshly seeded particle, every step */
    if (active) {
        const long long t = B.nodes[k];      /* local node index i + Nx jl, checked by picles_bforce_init */
        /* the prescribed value at t_start: level 0, or the line through the two levels — three IEEE operations per component */
        double e = B.v0[k], mx = B.v0[(size_t)B.n + k], my = B.v0[2 * (size_t)B.n + k];
        if (B.v1) {
            const double e1 = B.v1[k], mx1 = B.v1[(size_t)B.n + k], my1 = B.v1[2 * (size_t)B.n + k];
            e = e + B.s * (e1 - e);
            mx = mx + B.s * (mx1 - mx);
            my = my + B.s * (my1 - my);
        }
        if constexpr (BLEND) {
            const double wk = B.w[k];
            if (wk != 1.0) {
                double m0 = 0.0, m1 = 0.0, m2 = 0.0;
                if (B.from_rec) {
                    const int i = (int)(t % G.Nx), jl = (int)(t / G.Nx);
                    pull_any(G, A, i, jl, pull_reach_local(G, A, i, jl, pull_reach(G, A, jl)), m0, m1, m2);
                } else {
                    m0 = A.state[t]; m1 = A.state[t + A.n]; m2 = A.state[t + 2 * A.n];
                }
                e = m0 + wk * (e - m0);
                mx = m1 + wk * (mx - m1);
                my = m2 + wk * (my - m2);
            }
        }
        /* NodeToParticle! branch A on the prescribed value; anything else: no particle at this node this step */
        if (pm_isfinite(e) && pm_isfinite(mx) && pm_isfinite(my) && e >= P.min_e && mx * mx + my * my >= P.min_m2) {
            charge_to_particle(e, mx, my, z);
            on = 1;
            const Wind w = load_wind<true>(P, A, t);
            if (METRIC) status = advance_core<false, false, true, TSIT, AUTO, false>(P, w, z, on, qold, dtn, t_start, DT, S, A.m11[t], A.m22[t], A.pc[t], &asw);
            else status = advance_core<false, false, false, TSIT, AUTO, false>(P, w, z, on, qold, dtn, t_start, DT, S, 0.0, 0.0, 0.0, &asw);
        }
    }
    /* behind the RK loop the arguments are read again from the kernarg segment instead of living through it in scalar registers
     * (kargs_reload, kernels.h: taken where all lanes meet again), and a lane finds its node in the list again: nothing waits in LDS */
    const BForceArgs *K = (const BForceArgs *)kargs_reload();
    const KParams Pb = K->P;
    const GridP Gb = K->G;
    const Arrays Ab = K->A;
    __asm__ volatile("" ::: "memory");
    if ((int)(blockIdx.x * PICLES_BLOCK + threadIdx.x) < K->B.n) {
        const long long tb = K->B.nodes[blockIdx.x * PICLES_BLOCK + threadIdx.x];
        if (on) status = advance_guards<true>(Pb, [&]() { return load_wind<true>(Pb, Ab, tb); }, z, dtn, K->t_start, K->DT, status, S);
        Ab.asw[tb] = asw;
        Ab.z[tb] = z.lne; Ab.z[tb + Ab.n] = z.cx; Ab.z[tb + 2 * Ab.n] = z.cy; Ab.z[tb + 3 * Ab.n] = z.x; Ab.z[tb + 4 * Ab.n] = z.y;
        Ab.on[tb] = (unsigned char)on;
        Ab.qold[tb] = qold;
        Ab.dtn[tb] = dtn;
        Ab.status[tb] = status;
        /* the record — the empty one (code 0) where no particle was born: what the step kernels leave at a node they do not step
         * is not relied upon (the record buffers are a rotating pair) */
        write_record(Gb, Ab, (int)(tb % Gb.Nx), (int)(tb / Gb.Nx), 0, on, z, S);
        rtile = (int)(tb >> 6);
        class_map(Ab, (Ab.mr_idx >> 4) & 15)[tb >> 6] = 0;
    }
    /* a wave that bore nobody (the empty tail of the last workgroup, or refused values throughout) has nothing to count and no reach
     * to raise, and it stays out of flush_stats altogether: there it would pass for a wave of the step kernel with nothing to do
     * and switch the cost-ordered dispatch of the next step on, which is the step kernels' business */
    if (__ballot(on != 0)) flush_stats(Ab, S, rtile);
}

#define LAUNCH_BF(M, W) do { if (solver == 2) hipLaunchKernelGGL((k_bforce<M, true, true, W>), grid, dim3(PICLES_BLOCK), 0, L.stream, *L.P, *L.G, *L.A, B, L.t_start, L.DT); \
                             else if (solver) hipLaunchKernelGGL((k_bforce<M, true, false, W>), grid, dim3(PICLES_BLOCK), 0, L.stream, *L.P, *L.G, *L.A, B, L.t_start, L.DT); \
                             else hipLaunchKernelGGL((k_bforce<M, false, false, W>), grid, dim3(PICLES_BLOCK), 0, L.stream, *L.P, *L.G, *L.A, B, L.t_start, L.DT); } while (0)
/* B.w != nullptr: the set has a weight below 1 (picles_bforce_init_band keeps no weight plane otherwise) */
void launch_k_bforce(const StepLaunch &L, const BForceP &B, int solver, bool metric)
{
    const dim3 grid((unsigned)((B.n + PICLES_BLOCK - 1) / PICLES_BLOCK));
    if (B.w) { if (metric) LAUNCH_BF(true, true); else LAUNCH_BF(false, true); }
    else { if (metric) LAUNCH_BF(true, false); else LAUNCH_BF(false, false); }
}
