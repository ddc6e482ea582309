/*
 * k_nest.h — the stencil stage of a nest, both directions: k_nest_mix (one-way nesting, picles_nest_*: the parent's State onto the
 * child's forced nodes) and k_nest_restrict (two-way nesting, picles_nest_feedback_*: the child's State onto the parent's feedback
 * nodes).  Behind them the kernels that fill a whole child: k_nest_prolong (a child started from its parent) and k_nest_relocate (a
 * child moved across it).  Included by picles_hip.hip behind k_probe.h (not a translation unit of its own).
 *
 * The stage in front of either is k_probe as it stands, run over the distinct SOURCE nodes — the parent's corner nodes, the child's
 * source nodes — into a block of three planes of n_src doubles.  The stencil turns that block into one time level of the OTHER
 * context's forcing set: per output node p the weighted mean of its M entries (entry c of node p: index and weight at [c n + p]) —
 * the station definition of picles_amd/station_output.py, operation for operation:
 *
 *     a source is WET when e, m_x, m_y are finite, e > 0 and m_x*m_x + m_y*m_y > 0
 *     W = SE = SX = SY = +0.0;  for the entries in order, if wet:  W = W + w;  SE = SE + w*e;  SX = SX + w*m_x;  SY = SY + w*m_y
 *     E = SE / W;  MX = SX / W;  MY = SY / W;  M2 = MX*MX + MY*MY
 *     VALID when W > 0 and M2 > 0: the level is (E, MX, MY); otherwise NaN in all three (k_bforce bears nobody from a NaN level)
 *
 * Every operation rounds once (the unit is built with -ffp-contract=off: no multiply-add is fused here; the fp64 division is the
 * compiler's correctly rounded expansion) and the sum is serial, so NumPy reproduces the bits.
 * nest_stencil<M>: M = 4 is the mix, four corners, a constant trip count the compiler unrolls; M = 0 is the restrict, the entry
 * count the run-time argument m.  The kernels' pointers are __restrict__; the body is inlined into them and needs no word of it.  The
 * run-time flavour alone skips an entry whose weight is 0.0 — padding, whatever its index names — before it loads anything of it.
 * The skip changes no bit: an entry with w = 0.0 at a wet source adds W + 0 = W and w*v = +-0 to sums that started at +0.0, and
 * S + (+-0) = S for every S under round to nearest (+0 + -0 = +0); at a source that is not wet it adds nothing either way.
 * One lane per output node, 256-lane workgroups, no LDS, no atomics.  Index and weight planes are read coalesced; the 3 M source
 * values are gathers from a block of a few kilobytes that stays in L2; the level is three planes of n written coalesced.  With a few
 * thousand nodes the kernel is a handful of workgroups whose cost is the launch.
 */
#ifndef PICLES_K_NEST_H
#define PICLES_K_NEST_H

#define NEST_BLOCK 256

template <int M>
__device__ __forceinline__ void nest_stencil(int n, int n_src, int m, const int *index, const double *weight, const double *src, double *out)
{
    const int p = (int)(blockIdx.x * NEST_BLOCK + threadIdx.x);
    if (p < n) {
        double W = 0.0, SE = 0.0, SX = 0.0, SY = 0.0;
        for (int c = 0; c < (M ? M : m); c++) {
            const double w = weight[(size_t)c * n + p];
            if constexpr (M == 0) {
                if (w == 0.0) continue;                  /* padding */
            }
            const int q = index[(size_t)c * n + p];      /* in [0, n_src): checked when the stencil was uploaded */
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

__global__ void __launch_bounds__(NEST_BLOCK) k_nest_mix(int n, int n_corner, const int *__restrict__ index, const double *__restrict__ weight,
                                                         const double *__restrict__ corner, double *__restrict__ out)
{
    nest_stencil<4>(n, n_corner, 4, index, weight, corner, out);
}

__global__ void __launch_bounds__(NEST_BLOCK) k_nest_restrict(int n, int n_src, int m, const int *__restrict__ index, const double *__restrict__ weight,
                                                              const double *__restrict__ src, double *__restrict__ out)
{
    nest_stencil<0>(n, n_src, m, index, weight, src, out);
}

/*
 * k_nest_prolong (picles_nest_prolong: a child started from its parent): the parent's State, in memory, onto EVERY
 * node of the child.  One lane per child node, i fastest; the stencil is separable, so a lane loads the table row of its column
 * (ix0, ix1, wx) and of its row (iy0, iy1, wy) once and forms the four weights itself, in locate_points' order and with its
 * operations: gx = 1 - wx, gy = 1 - wy; gx*gy, wx*gy, gx*wy, wx*wy.  The twelve parent values are gathers from the parent's State
 * planes (neighbouring lanes share corners); three coalesced plane stores.  The station definition above, restated here
 * (nest_prolong_node) and not shared with nest_stencil (so that k_nest_mix and k_nest_restrict compile to what they were): the same
 * wet test, serial sums and three divisions, one rounding each.  A node that is not VALID is written as (0, 0, 0), not NaN: State is read by the remesh,
 * which makes a calm node's particle from the local wind, as it does for a node nothing was deposited on after any step.
 * np_x: the parent's Nx; n_par = its node count (the plane stride); the indices were checked on the host.
 */
/* one child node of the prolong: (i, j) from the table rows of its column and its row; n_par = the parent's plane stride.  Shared by
 * k_nest_prolong and k_nest_relocate: inlined into both, the same operations in the same order */
__device__ __forceinline__ void nest_prolong_node(int i, int j, int np_x, long long n_par, const int *ix0, const int *ix1, const double *wx,
                                                  const int *iy0, const int *iy1, const double *wy, const double *src, double &oe, double &ox,
                                                  double &oy)
{
    const int a0 = ix0[i], a1 = ix1[i], b0 = iy0[j], b1 = iy1[j];
    const double fx = wx[i], fy = wy[j];
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const double w4[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    const long long q4[4] = {(long long)b0 * np_x + a0, (long long)b0 * np_x + a1, (long long)b1 * np_x + a0, (long long)b1 * np_x + a1};
    double W = 0.0, SE = 0.0, SX = 0.0, SY = 0.0;
    for (int c = 0; c < 4; c++) {
        const double w = w4[c];
        const double e = src[q4[c]], mx = src[n_par + q4[c]], my = src[2 * n_par + q4[c]];
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
    oe = valid ? E : 0.0;
    ox = valid ? MX : 0.0;
    oy = valid ? MY : 0.0;
}

__global__ void __launch_bounds__(NEST_BLOCK) k_nest_prolong(int ncx, int ncy, int np_x, long long n_par, const int *__restrict__ ix0,
                                                             const int *__restrict__ ix1, const double *__restrict__ wx, const int *__restrict__ iy0,
                                                             const int *__restrict__ iy1, const double *__restrict__ wy,
                                                             const double *__restrict__ src, double *__restrict__ out)
{
    const long long n = (long long)ncx * ncy;
    const long long p = (long long)blockIdx.x * NEST_BLOCK + threadIdx.x;
    if (p < n) {
        const int i = (int)(p % ncx), j = (int)(p / ncx);
        double e, mx, my;
        nest_prolong_node(i, j, np_x, n_par, ix0, ix1, wx, iy0, iy1, wy, src, e, mx, my);
        out[p] = e;
        out[n + p] = mx;
        out[2 * n + p] = my;
    }
}

/*
 * k_nest_relocate (picles_nest_relocate: a child moved across its parent): the State of a child whose box has been
 * translated by (si, sj) of its own nodes, so that new node (i, j) lies where old node (i + si, j + sj) lay.  One lane per child node,
 * i fastest.  A KEPT lane — m <= i + si < ncx - m and m <= j + sj < ncy - m, m the margin that drops the old box's rim and band —
 * copies the bits of the child's old State at (i + si, j + sj): three coalesced loads, three coalesced stores, calm (0, 0, 0) nodes
 * and NaN payloads as they stand.  Any other lane is a lane of k_nest_prolong for the NEW box's tables (nest_prolong_node).  The
 * branch is per lane: a wave that lies wholly in the kept region never touches the tables or the parent.  `out` is not `old` (an
 * in-place shift races with itself); the sums i + si, j + sj are formed in 64 bits, so every shift is in bounds.
 */
__global__ void __launch_bounds__(NEST_BLOCK) k_nest_relocate(int ncx, int ncy, int si, int sj, int m, int np_x, long long n_par,
                                                              const int *__restrict__ ix0, const int *__restrict__ ix1,
                                                              const double *__restrict__ wx, const int *__restrict__ iy0,
                                                              const int *__restrict__ iy1, const double *__restrict__ wy,
                                                              const double *__restrict__ src, const double *__restrict__ old,
                                                              double *__restrict__ out)
{
    const long long n = (long long)ncx * ncy;
    const long long p = (long long)blockIdx.x * NEST_BLOCK + threadIdx.x;
    if (p < n) {
        const int i = (int)(p % ncx), j = (int)(p / ncx);
        const long long io = (long long)i + si, jo = (long long)j + sj;
        double e, mx, my;
        if (io >= m && io < (long long)ncx - m && jo >= m && jo < (long long)ncy - m) {
            const long long q = jo * ncx + io;
            e = old[q];
            mx = old[n + q];
            my = old[2 * n + q];
        } else {
            nest_prolong_node(i, j, np_x, n_par, ix0, ix1, wx, iy0, iy1, wy, src, e, mx, my);
        }
        out[p] = e;
        out[n + p] = mx;
        out[2 * n + p] = my;
    }
}

#endif /* PICLES_K_NEST_H */
