/*
 * k_nest.h — one-way nesting (picles_nest_*, include/picles_hip.h "one-way nesting"): the mix stage of a nest sample; and, at the
 * end of the file, the restrict stage of two-way nesting (k_nest_restrict, picles_nest_feedback_*).  Included by picles_hip.hip
 * behind k_probe.h (not a translation unit of its own).
 *
 * The corner stage in front of it is k_probe as it stands, run over the distinct PARENT corner nodes into a scratch block of three
 * planes of n_corner doubles.  k_nest_mix turns that block into one time level of the CHILD's forcing set: per forced child node the
 * weighted mean of its four corners — the station definition of picles_amd/station_output.py, operation for operation:
 *
 *     a corner is WET when e, m_x, m_y are finite, e > 0 and m_x*m_x + m_y*m_y > 0
 *     W = SE = SX = SY = +0.0;  for the corners in order, if wet:  W = W + w;  SE = SE + w*e;  SX = SX + w*m_x;  SY = SY + w*m_y
 *     E = SE / W;  MX = SX / W;  MY = SY / W;  M2 = MX*MX + MY*MY
 *     VALID when W > 0 and M2 > 0: the level is (E, MX, MY); otherwise NaN in all three (k_bforce bears nobody from a NaN level)
 *
 * Every operation rounds once (the unit is built with -ffp-contract=off: no multiply-add is fused here; the fp64 division is the
 * compiler's correctly rounded expansion), so NumPy reproduces the bits.
 * One lane per forced node, 256-lane workgroups, no LDS, no atomics.  The four indices and weights are planes of n (corner c of
 * node p at [c n + p]): read coalesced; the twelve corner values are gathers from a block of a few kilobytes that stays in L2; the
 * level is three planes of n written coalesced.  With a few thousand nodes the kernel is a handful of workgroups whose cost is the
 * launch.
 */
#ifndef PICLES_K_NEST_H
#define PICLES_K_NEST_H

#define NEST_BLOCK 256

__global__ void __launch_bounds__(NEST_BLOCK) k_nest_mix(int n, int n_corner, const int *__restrict__ index, const double *__restrict__ weight,
                                                         const double *__restrict__ corner, double *__restrict__ out)
{
    const int p = (int)(blockIdx.x * NEST_BLOCK + threadIdx.x);
    if (p < n) {
        double W = 0.0, SE = 0.0, SX = 0.0, SY = 0.0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int q = index[(size_t)c * n + p];      /* in [0, n_corner): checked by picles_nest_init */
            const double w = weight[(size_t)c * n + p];
            const double e = corner[q], mx = corner[(size_t)n_corner + q], my = corner[2 * (size_t)n_corner + q];
            if (pm_isfinite(e) && pm_isfinite(mx) && pm_isfinite(my) && e > 0.0 && mx * mx + my * my > 0.0) {
                W = W + w;
                SE = SE + w * e;
                SX = SX + w * mx;
                SY = SY + w * my;
            }
        }
        const double E = SE / W, MX = SX / W, MY = SY / W;
        const double M2 = MX * MX + MY * MY;
        const bool valid = W > 0.0 && M2 > 0.0;
        const double nan = __builtin_nan("");
        out[p] = valid ? E : nan;
        out[(size_t)n + p] = valid ? MX : nan;
        out[2 * (size_t)n + p] = valid ? MY : nan;
    }
}

/*
 * k_nest_restrict — two-way nesting (picles_nest_feedback_*, include/picles_hip.h "two-way nesting"): the restrict stage of a
 * feedback.  The source stage in front of it is k_probe as it stands, run over the distinct CHILD nodes any feedback node uses, into
 * a scratch block of three planes of n_src doubles; this kernel turns that block into the one level of the PARENT's feedback set.
 * Per feedback node the definition above, generalised from four corners to m stencil entries (entry c of node p at [c n + p], m a
 * run-time argument): the entries are visited in order, an entry whose weight is 0.0 is padding and is skipped whatever its source
 * holds, a source value that is not wet adds nothing, and every operation rounds once — the sum is serial, so NumPy reproduces the
 * bits (picles_amd/nesting.py: restrict_records).  One lane per feedback node, 256-lane workgroups, no LDS, no atomics; index and
 * weight planes read coalesced, 3 m gathers per lane from a block that stays in L2, three planes of n written coalesced.
 */
__global__ void __launch_bounds__(NEST_BLOCK) k_nest_restrict(int n, int n_src, int m, const int *__restrict__ index, const double *__restrict__ weight,
                                                              const double *__restrict__ src, double *__restrict__ out)
{
    const int p = (int)(blockIdx.x * NEST_BLOCK + threadIdx.x);
    if (p < n) {
        double W = 0.0, SE = 0.0, SX = 0.0, SY = 0.0;
        for (int c = 0; c < m; c++) {
            const double w = weight[(size_t)c * n + p];
            if (w == 0.0) continue;                      /* padding */
            const int q = index[(size_t)c * n + p];      /* in [0, n_src): checked by picles_nest_feedback_init */
            const double e = src[q], mx = src[(size_t)n_src + q], my = src[2 * (size_t)n_src + q];
            if (pm_isfinite(e) && pm_isfinite(mx) && pm_isfinite(my) && e > 0.0 && mx * mx + my * my > 0.0) {
                W = W + w;
                SE = SE + w * e;
                SX = SX + w * mx;
                SY = SY + w * my;
            }
        }
        const double E = SE / W, MX = SX / W, MY = SY / W;
        const double M2 = MX * MX + MY * MY;
        const bool valid = W > 0.0 && M2 > 0.0;
        const double nan = __builtin_nan("");
        out[p] = valid ? E : nan;
        out[(size_t)n + p] = valid ? MX : nan;
        out[2 * (size_t)n + p] = valid ? MY : nan;
    }
}

#endif /* PICLES_K_NEST_H */
