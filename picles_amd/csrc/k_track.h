/*
 * k_track.h — track samples (picles_track_*, include/picles_hip.h "track samples"): the sea state at events (t_k, x_k, y_k) along a
 * moving platform, taken without completing a pending fused step.  Included by picles_hip.hip behind k_nest.h (not a translation
 * unit of its own).
 *
 * A launch covers the events [k0, k1) whose time lies next to the clock T (the host found the range by binary search in its copy of
 * the sorted times).  FOUR LANES PER EVENT, one per corner: 64 events per 256-lane workgroup, no LDS, no atomics.
 *   1. each lane takes the value of its corner node — FROM_REC = true: the pull k_scatter would run for that node over the records of
 *      the pending fused step (k_probe.h has the argument for pull_reach_local among scattered lanes; the four lanes of a quad are
 *      active or idle together, so the ballot ladder sees whole quads); FROM_REC = false: a gather from State —, tests it for WET
 *      and forms its three products w*e, w*m_x, w*m_y;
 *   2. the quad exchanges the twelve values (weight and three products of each corner, zeros where the corner is not wet) with
 *      quad-local lane shuffles (__shfl of width 4: lanes outside the quad are never read);
 *   3. every lane sums them serially in corner order — the station definition of k_nest.h, operation for operation: a corner that is
 *      not wet is SKIPPED (a select keeps the running sum, it does not add a zero), every product and every sum rounds once
 *      (-ffp-contract=off), so NumPy reproduces the bits;
 *   4. quad lane 0 applies the before / after rule and writes the slots: 8 planes of m doubles,
 *      [e_b mx_b my_b t_b] [e_a mx_a my_a t_a].
 * Why a quad: the launch is a handful of workgroups whose time is the latency of the pulls (9 - 25 candidate records each, dependent
 * on the reach map); with the four corners in four lanes the serial chain is one pull, not four.
 * Bounds: k0 <= k < k1 <= m; the corner nodes were checked against the grid when the set was made.
 */
#ifndef PICLES_K_TRACK_H
#define PICLES_K_TRACK_H

#define TRACK_BLOCK 256

template <bool FROM_REC>
__global__ void __launch_bounds__(TRACK_BLOCK) k_track(GridP G, Arrays A, int k0, int k1, int m, double T, const double *__restrict__ tk,
                                                       const int *__restrict__ ij, const double *__restrict__ weight, double *__restrict__ table)
{
    const unsigned int g = blockIdx.x * TRACK_BLOCK + threadIdx.x;
    const int k = k0 + (int)(g >> 2), c = (int)(g & 3u);
    if (k < k1) {       /* whole quads: TRACK_BLOCK is a multiple of 4 */
        const int i = ij[(size_t)c * m + k], jl = ij[(size_t)(4 + c) * m + k];      /* the set lives on whole-grid contexts: local row = global row */
        const double w = weight[(size_t)c * m + k];
        double e = 0.0, mx = 0.0, my = 0.0;
        if (FROM_REC) {
            pull_any(G, A, i, jl, pull_reach_local(G, A, i, jl, pull_reach(G, A, jl)), e, mx, my);
        } else {
            const long long t = (long long)jl * G.Nx + i;
            e = A.state[t]; mx = A.state[t + A.n]; my = A.state[t + 2 * A.n];
        }
        const bool wet = pm_isfinite(e) && pm_isfinite(mx) && pm_isfinite(my) && e > 0.0 && mx * mx + my * my > 0.0;
        const double pe = w * e, px = w * mx, py = w * my;
        double W = 0.0, SE = 0.0, SX = 0.0, SY = 0.0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int wq = __shfl((int)wet, q, 4);
            const double ww = __shfl(w, q, 4), qe = __shfl(pe, q, 4), qx = __shfl(px, q, 4), qy = __shfl(py, q, 4);
            if (wq) {
                W = W + ww;
                SE = SE + qe;
                SX = SX + qx;
                SY = SY + qy;
            }
        }
        if (c == 0) {
            const double E = SE / W, MX = SX / W, MY = SY / W;
            const double M2 = MX * MX + MY * MY;
            const bool valid = W > 0.0 && M2 > 0.0;
            const double nan = __builtin_nan("");
            const double oe = valid ? E : nan, ox = valid ? MX : nan, oy = valid ? MY : nan;
            const double t = tk[k];
            const size_t M = (size_t)m;
            if (t >= T) {       /* before: the latest sample at a clock <= t_k */
                table[k] = oe; table[M + k] = ox; table[2 * M + k] = oy; table[3 * M + k] = T;
            }
            if (t <= T && table[7 * M + k] != table[7 * M + k]) {       /* after: the earliest sample at a clock >= t_k (t_a still NaN) */
                table[4 * M + k] = oe; table[5 * M + k] = ox; table[6 * M + k] = oy; table[7 * M + k] = T;
            }
        }
    }
}

#endif /* PICLES_K_TRACK_H */
