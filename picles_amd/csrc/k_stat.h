/*
 * k_stat.h — run statistics (picles_stat_*, include/picles_hip.h "run statistics"): the State value of EVERY node, folded into
 * per-node accumulators that stay in device memory, without completing a pending fused step.  Included by picles_hip.hip behind
 * kernels.h (not a translation unit of its own).
 *
 * One lane per node with k_scatter's node-to-lane mapping (xcd_block: 256 consecutive nodes per workgroup, the workgroups of an
 * XCD a contiguous band), 256-lane workgroups, no LDS, no atomics: a node belongs to one lane, and the updates of one set are
 * ordered behind each other by the host (stat_update).
 *   FROM_REC = true:  a fused step is pending — State of that step exists only as its scatter records.  The lane evaluates for its
 *                     node exactly what k_scatter evaluates: pull_any over the records, from +0.0, with the reach of pull_reach /
 *                     pull_reach_local (tripolar fold, aliased small grids, ghost rows and G.Rp included: the functions are used
 *                     as they stand).  The lanes of a wave are neighbours along a row as in k_scatter, so the wave-uniform reach
 *                     of pull_reach_local is the one k_scatter would use.
 *   FROM_REC = false: State is in memory: a plain coalesced read.
 * Every plane is indexed by the node index t: a wave's access to a plane is 64 consecutive words.  A plane is written only where
 * it changes: nothing for a sample that is not wet, the four PEAK planes only on a new maximum, an n_exc plane only where the
 * threshold is met.  The group mask and the thresholds are kernel arguments (wave-uniform: the group branches are scalar).
 * Per wet node and update with every group: 8 B + 32 B + 4 B (+ 4 B per threshold) read, 32 B + 4 B written (+ 32 B on a new
 * maximum, + 4 B per threshold met), next to the pull's record reads (DESIGN.md §14 has the measured time).
 */
#ifndef PICLES_K_STAT_H
#define PICLES_K_STAT_H

#define STAT_MAX_THR 4

struct StatP {
    unsigned mask;               /* PICLES_STAT_* bits */
    int nthr;                    /* thresholds in use (0 without PICLES_STAT_EXCEED) */
    double thr[STAT_MAX_THR];    /* Hs thresholds, ascending */
};

template <bool FROM_REC>
__global__ void __launch_bounds__(PICLES_BLOCK) k_stat(GridP G, Arrays A, StatP S, double clock, unsigned int *__restrict__ n_wet,
                                                       double *__restrict__ peak, double *__restrict__ mean,
                                                       unsigned int *__restrict__ n_exc)
{
    const long long t = (long long)xcd_block() * PICLES_BLOCK + threadIdx.x;
    if (t < A.n) {
        double e = 0.0, mx = 0.0, my = 0.0;
        if (FROM_REC) {
            const int i = (int)(t % G.Nx), jl = (int)(t / G.Nx);
            pull_any(G, A, i, jl, pull_reach_local(G, A, i, jl, pull_reach(G, A, jl)), e, mx, my);
        } else {
            e = A.state[t]; mx = A.state[t + A.n]; my = A.state[t + 2 * A.n];
        }
        const double m2 = mx * mx + my * my;
        const bool wet = __builtin_isfinite(e) && __builtin_isfinite(mx) && __builtin_isfinite(my) && e > 0.0 && m2 > 0.0;
        if (wet) {
            const unsigned int nw = n_wet[t];
            n_wet[t] = nw + 1u;
            if (S.mask & PICLES_STAT_PEAK) {
                if (nw == 0u || e > peak[t]) {
                    peak[t] = e; peak[t + A.n] = mx; peak[t + 2 * A.n] = my; peak[t + 3 * A.n] = clock;
                }
            }
            if (S.mask & (PICLES_STAT_MEAN | PICLES_STAT_EXCEED)) {
                const double hs = 4.0 * __builtin_sqrt(e);
                if (S.mask & PICLES_STAT_MEAN) {
                    const double a = mean[t], b = mean[t + A.n], c = mean[t + 2 * A.n], d = mean[t + 3 * A.n];
                    mean[t] = a + e; mean[t + A.n] = b + mx; mean[t + 2 * A.n] = c + my; mean[t + 3 * A.n] = d + hs;
                }
                if (S.mask & PICLES_STAT_EXCEED) {
#pragma unroll
                    for (int k = 0; k < STAT_MAX_THR; k++)
                        if (k < S.nthr && hs >= S.thr[k]) { unsigned int *p = n_exc + (size_t)k * (size_t)A.n + t; *p = *p + 1u; }
                }
            }
        }
    }
}

#endif /* PICLES_K_STAT_H */
