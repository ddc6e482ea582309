/*
 * k_probe.h — station probes (picles_probe_*, include/picles_hip.h "station probes"): the State value of a list of nodes, taken
 * without completing a pending fused step.  Included by picles_hip.hip behind kernels.h (not a translation unit of its own).
 *
 * One lane per probed node, 256-lane workgroups, no LDS, no atomics.  The node list is two int planes (i, then the LOCAL row jl),
 * read coalesced; the sample is three planes of n doubles [k][node], written coalesced into the ring slot.
 *   FROM_REC = true:  a fused step is pending — State of that step exists only as its scatter records.  The lane evaluates for its
 *                     node exactly what k_scatter evaluates for every node: pull_any over the records, from +0.0, with the reach of
 *                     pull_reach / pull_reach_local (tripolar fold, aliased small grids, ghost rows and G.Rp included: the functions
 *                     are used as they stand).  pull_reach_local makes the reach uniform over the ACTIVE lanes of the wave; here the
 *                     lanes of a wave sit anywhere on the grid, so a lane may pull with a neighbour's larger reach — the same bits
 *                     (kernels.h: any reach >= the true one), never beyond halo_rows on a slab (pull_reach caps at G.Rp).
 *   FROM_REC = false: State is in memory: a plain gather.
 * The gathers are 24 B per node from wherever the nodes are; with a few thousand nodes the kernel is a handful of workgroups whose
 * cost is the launch (DESIGN.md §13 has the resources and the measured time).
 */
#ifndef PICLES_K_PROBE_H
#define PICLES_K_PROBE_H

#define PROBE_BLOCK 256

template <bool FROM_REC>
__global__ void __launch_bounds__(PROBE_BLOCK) k_probe(GridP G, Arrays A, int n, const int *__restrict__ nodes, double *__restrict__ out)
{
    const int p = (int)(blockIdx.x * PROBE_BLOCK + threadIdx.x);
    if (p < n) {
        const int i = nodes[p], jl = nodes[n + p];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (FROM_REC) {
            pull_any(G, A, i, jl, pull_reach_local(G, A, i, jl, pull_reach(G, A, jl)), s0, s1, s2);
        } else {
            const long long t = (long long)jl * G.Nx + i;
            s0 = A.state[t]; s1 = A.state[t + A.n]; s2 = A.state[t + 2 * A.n];
        }
        out[p] = s0; out[(size_t)n + p] = s1; out[2 * (size_t)n + p] = s2;
    }
}

#endif /* PICLES_K_PROBE_H */
