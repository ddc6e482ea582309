/*
 * k_flux_mean.h — flux means (picles_flux_mean_*, include/picles_hip.h "flux means"): the coupling fluxes of k_flux.h
 * accumulated per coarse cell behind every model step, without completing a pending fused step, and finalised into interval means.
 * Included by picles_hip.hip behind kernels.h, k_diag.h and k_flux.h (not a translation unit of its own).
 *
 * THE ACCUMULATORS.  Eleven fp64 planes of Nxc x nyc_loc, column-major [I + Nxc J]: the nine sums in PICLES_FLUX_* bit order, then
 * n_active and n_bad.  One update adds to every cell the eleven cell sums S_q of k_flux — flux_node per node, the nodes visited
 * j outer, i inner, from +0.0, the values of the ACTIVE nodes (status 1) added, statuses 1 and 2 counted — by ONE fp64 addition per
 * plane and cell: acc_q = acc_q + S_q.  A cell belongs to one lane, and the operations on one set are ordered behind each other by
 * the host (flux_mean_order / flux_mean_mark): no LDS, no atomics.
 *
 * k_flux_mean_update<FROM_REC, CX>
 *   FROM_REC = true:  a fused step is pending — State of that step exists only as its scatter records.  A lane evaluates for its node
 *                     what k_scatter evaluates: pull_any from +0.0 with the reach of pull_reach / pull_reach_local, as k_stat<true>
 *                     and k_probe<true> do (any arrangement of the lanes gives the same bits: k_probe.h has the argument).
 *   FROM_REC = false: State is in memory: plain loads.
 *   CX in {1, 2, 4, 8, 16}: k_scatter's decomposition along x.  A workgroup covers 256 consecutive nodes of a row — 256 / CX whole
 *                     cells; a power-of-two group never straddles a wave — and loops over the rows of its coarse row.  Every lane
 *                     pulls its own node (coalesced record reads, the reach wave-uniform among the lanes inside `if (active)`) and
 *                     runs flux_node for it; the leading lane of each group of CX lanes collects the group's nine values and status
 *                     by shuffles in ascending i and keeps the running cell sums across the rows in registers: the sequential
 *                     order of the definition.  A lane beyond Nx holds status 0: a ragged last cell falls out of the i < Nx tests.
 *   CX = 0:           any factor: one lane per coarse cell visiting its nodes in turn, the shape of k_flux<0, false>.
 * flux_exp_core reads its table from constant memory: the kernel needs no pm_device_init.
 *
 * k_flux_mean_final: k_flux's epilogue on the accumulators.  One lane per coarse cell, one workgroup per tile of 256 coarse columns of
 * one coarse row, in global indices.  Plane q of the mask = (float)((acc_q / (n_cover * n)) * scale_q): the product in fp64 (exact),
 * one division, the scale as the last fp64 operation, rounded to float32 (nearest even).  The tile's partial: the eleven accumulator
 * planes, each through k_diag's tree (diag_wave_sum, then the four waves in ascending order), unscaled and undivided.
 */
#ifndef PICLES_K_FLUX_MEAN_H
#define PICLES_K_FLUX_MEAN_H

template <bool FROM_REC>
__device__ __forceinline__ void flux_mean_node(const KParams &P, const GridP &G, const Arrays &A, int i, int jl, const double *__restrict__ wu,
                                               const double *__restrict__ wv, FluxNode &f)
{
    const long long t = (long long)jl * G.Nx + i;
    double e = 0.0, mx = 0.0, my = 0.0;
    if (FROM_REC) {
        pull_any(G, A, i, jl, pull_reach_local(G, A, i, jl, pull_reach(G, A, jl)), e, mx, my);
    } else {
        e = A.state[t]; mx = A.state[t + A.n]; my = A.state[t + 2 * A.n];
    }
    flux_node(P, e, mx, my, wu[t], wv[t], f);
}

template <bool FROM_REC, int CX>
__global__ void __launch_bounds__(PICLES_BLOCK) k_flux_mean_update(KParams P, GridP G, Arrays A, FluxP F, const double *__restrict__ wu,
                                                                   const double *__restrict__ wv, double *__restrict__ acc)
{
    double s[FLUX_NV], na = 0.0, nb = 0.0;
#pragma unroll
    for (int k = 0; k < FLUX_NV; k++) s[k] = 0.0;
    const size_t cells = (size_t)F.Nxc * F.nyc_loc;
    if (CX > 0) {
        /* blocks_x workgroups per coarse row, 256 consecutive nodes each */
        const unsigned int blocks_x = ((unsigned int)F.Nx + PICLES_BLOCK - 1u) / PICLES_BLOCK;
        const int Jl = (int)(blockIdx.x / blocks_x);
        const int i = (int)(blockIdx.x % blocks_x) * PICLES_BLOCK + (int)threadIdx.x;
        const bool active = i < F.Nx && Jl < F.nyc_loc;
        const int j0 = Jl * F.cy, j1 = min(j0 + F.cy, F.ny_loc);
        const int lane = (int)(threadIdx.x & 63u);
        for (int j = j0; j < j1; j++) {
            FluxNode f;
#pragma unroll
            for (int k = 0; k < FLUX_NV; k++) f.v[k] = 0.0;
            f.status = 0;
            if (active) flux_mean_node<FROM_REC>(P, G, A, i, j, wu, wv, f);
            /* the group's nodes in ascending i, into the registers of its leading lane (every lane shuffles; the leaders keep) */
#pragma unroll
            for (int m = 0; m < CX; m++) {
                const int src = CX > 1 ? lane + m : lane;
                const int st = CX > 1 ? __shfl(f.status, src) : f.status;
                double v[FLUX_NV];
#pragma unroll
                for (int k = 0; k < FLUX_NV; k++) v[k] = CX > 1 ? __shfl(f.v[k], src) : f.v[k];
                if (st == 1) {
#pragma unroll
                    for (int k = 0; k < FLUX_NV; k++) s[k] = s[k] + v[k];
                    na = na + 1.0;
                } else if (st == 2) {
                    nb = nb + 1.0;
                }
            }
        }
        if (active && (threadIdx.x & (unsigned)(CX - 1)) == 0u) {
            double *p = acc + (size_t)(i / CX) + (size_t)F.Nxc * Jl;
#pragma unroll
            for (int k = 0; k < FLUX_NV; k++) { const double a = p[k * cells]; p[k * cells] = a + s[k]; }
            const double a = p[FLUX_NV * cells], b = p[(FLUX_NV + 1) * cells];
            p[FLUX_NV * cells] = a + na;
            p[(FLUX_NV + 1) * cells] = b + nb;
        }
    } else {
        /* any factor: one lane per coarse cell, k_flux's tiles */
        const int T = (int)(blockIdx.x % (unsigned)F.tiles_per_row), Jl = (int)(blockIdx.x / (unsigned)F.tiles_per_row);
        const int I = T * DIAG_TILE + (int)threadIdx.x;
        if (I < F.Nxc && Jl < F.nyc_loc) {
            const int i0 = I * F.cx, i1 = min(i0 + F.cx, F.Nx);
            const int j0 = Jl * F.cy, j1 = min(j0 + F.cy, F.ny_loc);
            for (int j = j0; j < j1; j++)
                for (int i = i0; i < i1; i++) {
                    FluxNode f;
                    flux_mean_node<FROM_REC>(P, G, A, i, j, wu, wv, f);
                    if (f.status == 1) {
#pragma unroll
                        for (int k = 0; k < FLUX_NV; k++) s[k] = s[k] + f.v[k];
                        na = na + 1.0;
                    } else if (f.status == 2) {
                        nb = nb + 1.0;
                    }
                }
            double *p = acc + (size_t)I + (size_t)F.Nxc * Jl;
#pragma unroll
            for (int k = 0; k < FLUX_NV; k++) { const double a = p[k * cells]; p[k * cells] = a + s[k]; }
            const double a = p[FLUX_NV * cells], b = p[(FLUX_NV + 1) * cells];
            p[FLUX_NV * cells] = a + na;
            p[(FLUX_NV + 1) * cells] = b + nb;
        }
    }
}

/* n: the samples the accumulators hold (>= 1), as a double */
__global__ void __launch_bounds__(DIAG_TILE) k_flux_mean_final(FluxP F, double n, const double *__restrict__ acc, float *__restrict__ fields,
                                                               double *__restrict__ partials)
{
    const int T = (int)(blockIdx.x % (unsigned)F.tiles_per_row), Jl = (int)(blockIdx.x / (unsigned)F.tiles_per_row);
    const int I = T * DIAG_TILE + (int)threadIdx.x;
    double a[FLUX_NP];
#pragma unroll
    for (int k = 0; k < FLUX_NP; k++) a[k] = 0.0;
    if (I < F.Nxc && Jl < F.nyc_loc) {
        const size_t cells = (size_t)F.Nxc * F.nyc_loc;
        const double *p = acc + (size_t)I + (size_t)F.Nxc * Jl;
#pragma unroll
        for (int k = 0; k < FLUX_NP; k++) a[k] = p[k * cells];
        const int i0 = I * F.cx, i1 = min(i0 + F.cx, F.Nx);
        const int j0 = Jl * F.cy, j1 = min(j0 + F.cy, F.ny_loc);
        const double den = (double)((i1 - i0) * (j1 - j0)) * n;
        float *out = fields + (size_t)I + (size_t)F.Nxc * Jl;
#pragma unroll
        for (int k = 0; k < FLUX_NV; k++) {
            if (F.mask & (1u << k)) {
                const double scale = k < 3 ? F.scale_phi : k < 7 ? F.scale_tau : 1.0;
                *out = (float)((a[k] / den) * scale);
                out += cells;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < FLUX_NP; k++) a[k] = diag_wave_sum(a[k]);
    __shared__ double red[DIAG_TILE / 64][FLUX_NP];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < FLUX_NP; k++) red[w][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x < FLUX_NP && Jl < F.nyc_loc) {
        const int q = threadIdx.x;
        double r = red[0][q];
#pragma unroll
        for (int k = 1; k < DIAG_TILE / 64; k++) r = r + red[k][q];
        partials[(size_t)blockIdx.x * FLUX_NP + q] = r;
    }
}

#endif /* PICLES_K_FLUX_MEAN_H */
