/*
 * k_flux.h — coupling fluxes (picles_flux_*, include/picles_hip.h "coupling fluxes"): what the partner models of a
 * coupled system consume — the energy and momentum the waves take out of the wind, what the breaking waves hand down to the ocean,
 * the surface Stokes drift — formed per node from State and the wind at the clock, coarsened to float32 planes and reduced to one
 * partial of eleven doubles per tile.  flux_node compiles for the host and the device like the pmath.h functions (the tests build it
 * for the host behind a plain C function and hold the kernel against it bit for bit); the kernel, a sibling of k_diag with the same
 * decomposition, is device code.  Included by picles_hip.hip (not a translation unit of its own).  It only reads State and the winds.
 *
 * THE NODE (this text is the contract).  Inputs: the node's State (e, m_x, m_y), the wind (u, v), the context's KParams P.  Every line
 * is ONE correctly rounded IEEE operation, or one call of a pmath.h function, in the order written; fma(a, b, c) is a fused
 * multiply-add, nothing else is contracted (-ffp-contract=off).  exp_core(x) is pm_exp_core's arithmetic (pmath.h); on the device its
 * table entry comes from constant memory, not from LDS (flux_exp_core below): the same bits.
 *
 *   ACTIVE:  e, m_x, m_y finite,  e >= P.min_e,  m_x m_x + m_y m_y >= P.min_m2        (NodeToParticle! branch A, as k_bforce tests it)
 *   anything else: status 0, the nine values +0.0.
 *   the particle (charge_to_particle):  q = e / (2.0 fma(m_x, m_x, m_y m_y)),  lne = pm_log(e),  cx = m_x q,  cy = m_y q
 *
 *   the RHS quantities — the arithmetic of rhs3<false> (physics.h), guarded forms, lane by lane:
 *     c2 = fma(cx, cx, cy cy)      y = pm_rsqrt(c2)      y2 = y y      dotc = fma(u, cx, v cy)
 *     U2 = fma(u, u, v v)          qU2r = (0.25 U2) P.rg2
 *     ym = fmin(y, P.ymax)         w_p = P.Cw ym                                       ω_p = g / (2 max(c_gp, 0.1))
 *     m2 = ym ym                   k_p = P.g4rg2 m2                                    k_p = g / (4 max(c_gp², 0.01))
 *     aph = (P.Chrh dotc) fmin(y2, P.sgmax),  clamped to [-699, 699]                   -α_p/2 with the floor 1e-4 on the speed
 *     yh = aph + 0.425
 *     2p = 3/2 (P.p_is_075):  w = exp_core(-|yh|)   w2 = w w   s3 = w2 w   w5 = s3 w2   w10 = w5 w5   w20 = w10 w10   t = w20 w20
 *                             hp = 1.0 + s3   t1 = 1.0 + t   t12 = t1 t1   r = pm_rcp_plain(hp t12)   H = (t12 r) (yh <= 0 ? 1.0 : s3)
 *     general p:              ya = -2.0 yh   hp = 1.0 + exp(min(P.neg2p ya, 700))   t = 20|ya| >= 40 ? 0.0 : exp_core(-20.0 |ya|)
 *                             t1 = 1.0 + t   t12 = t1 t1   r = pm_rcp_plain(hp t12)   H = t12 r
 *     Δ = fma(-((5.0 t) hp), r, 1.0)
 *     plain = y <= P.ymax and U2 >= 1e-290 and qU2r <= P.qU2r_max
 *     aH = plain ? qU2r (y2 H) : fmin(qU2r y2, 250000.0) H                             α² H_β, α <= 500; 0 for a vanishing wind
 *     Ĩ  = P.input ? P.C_e aH : +0.0
 *     m4 = m2 m2      Ek8 = exp(clamp(lne + lne, ±700)) (m4 m4)                        (needed by D̃ at n = 2 and by the peak shift)
 *     D̃  = !P.dissipation ? +0.0 : P.n_is_2 ? Ek8 P.KeT4y : pm_exp(P.n lne) pm_pow((P.g4rg2 m2) P.inv_eT, 2.0 P.n)
 *     wrS = P.peak_shift ? (w_p Δ) (Ek8 P.KrCay) : +0.0                                ω_p r_g S_cg
 *
 *   the nine values, d = c̄ / |c̄|:
 *     dx = cx y      dy = cy y      ew = e w_p
 *     phi_in = ew Ĩ      phi_dis = ew D̃      phi_shift = e wrS
 *     a = w_p phi_in     tq_in_x = a dx      tq_in_y = a dy
 *     b = w_p phi_dis    tq_dis_x = b dx     tq_dis_y = b dy
 *     s = (2.0 ew) k_p   us_x = s dx         us_y = s dy
 *   BAD: an active node one of whose nine values is not finite: status 2, the nine values +0.0.  Otherwise status 1.
 *
 * phi_in - phi_dis + phi_shift is e times the first component of rhs3 to rounding (rhs3 fuses Ĩ - D̃ and the final sum).
 */
#ifndef PICLES_K_FLUX_H
#define PICLES_K_FLUX_H

#include "physics.h"

#define FLUX_NV 9                /* values per node, in the bit order of PICLES_FLUX_* */
#define FLUX_NP 11               /* doubles per tile partial: the nine unscaled sums, n_active, n_bad */

struct FluxNode {
    double v[FLUX_NV];           /* phi_in, phi_dis, phi_shift, tq_in_x, tq_in_y, tq_dis_x, tq_dis_y, us_x, us_y */
    int status;                  /* 0 not active, 1 active, 2 bad */
};

/* pm_exp_core with the table entry from constant memory on the device: a kernel that calls it needs neither pm_device_init nor the
 * 4 KB of LDS behind it.  The index is masked: in bounds whatever x is */
PM_HD double flux_exp_core(double x)
{
    const double kd = PM_FMA(x, PM_EXP_RN, 6755399441055744.0);
    const double k = kd - 6755399441055744.0;
    double r = PM_FMA(-k, PM_EXP_LHI, x);
    r = PM_FMA(-k, PM_EXP_LLO, r);
    const int ki = (int)(uint32_t)pm_bits(kd);
    const int j = ki & (PM_EXP_N - 1);
    const int m = ki >> PM_EXP_SHIFT;
    const double q = pm_expm1_poly(r);
#if defined(__HIP_DEVICE_COMPILE__)
    const double T = PM_EXP_TAB_C[j];
#else
    const double T = PM_EXP_TAB_H[j];
#endif
    return __builtin_ldexp(PM_FMA(T, q, T), m);
}
/* exp(clamp(x, lo, hi)): the clamps of pm_exp (-746, 710), pm_exp_finite (-746, 700) and pm_exp_sat (-700, 700); a NaN passes */
PM_HD double flux_exp_clamped(double x, double lo, double hi)
{
    x = (x > hi) ? hi : x;
    x = (x < lo) ? lo : x;
    return flux_exp_core(x);
}

PM_HD void flux_node(const KParams &P, double e, double mx, double my, double u, double v, FluxNode &out)
{
#pragma unroll
    for (int k = 0; k < FLUX_NV; k++) out.v[k] = 0.0;
    out.status = 0;
    if (!(pm_isfinite(e) && pm_isfinite(mx) && pm_isfinite(my) && e >= P.min_e && mx * mx + my * my >= P.min_m2)) return;
    Vec5 z;
    charge_to_particle(e, mx, my, z);
    const double lne = z.lne, cx = z.cx, cy = z.cy;
    const double c2 = PM_FMA(cx, cx, cy * cy);
    const double y = pm_rsqrt(c2);
    const double y2 = y * y;
    const double dotc = PM_FMA(u, cx, v * cy);
    const double U2 = PM_FMA(u, u, v * v);
    const double qU2r = (0.25 * U2) * P.rg2;
    const double ym = pm_fmin(y, P.ymax);
    const double wp = P.Cw * ym;
    const double m2 = ym * ym;
    const double kp = P.g4rg2 * m2;
    double aph = (P.Chrh * dotc) * pm_fmin(y2, P.sgmax);
    aph = (aph > 699.0) ? 699.0 : aph;
    aph = (aph < -699.0) ? -699.0 : aph;
    const double yh = aph + 0.425;
    double hp, t, H, rHD, t12;
    if (P.p_is_075) {
        const double w = flux_exp_core(-pm_fabs(yh));
        const double w2 = w * w, s3 = w2 * w;
        const double w5 = s3 * w2, w10 = w5 * w5, w20 = w10 * w10;
        t = w20 * w20;
        hp = 1.0 + s3;
        const double t1 = 1.0 + t;
        t12 = t1 * t1;
        rHD = pm_rcp_plain(hp * t12);
        H = (t12 * rHD) * ((yh <= 0.0) ? 1.0 : s3);
    } else {
        const double ya = -2.0 * yh;
        hp = 1.0 + flux_exp_clamped(P.neg2p * ya, -746.0, 700.0);
        const double targ = -20.0 * pm_fabs(ya);
        t = 0.0;
        if (!(targ <= -40.0)) t = flux_exp_core(targ);
        const double t1 = 1.0 + t;
        t12 = t1 * t1;
        rHD = pm_rcp_plain(hp * t12);
        H = t12 * rHD;
    }
    const double D = PM_FMA(-((5.0 * t) * hp), rHD, 1.0);
    const bool plain = (y <= P.ymax) && wind_is_plain(P, U2, qU2r);
    const double aH = plain ? qU2r * (y2 * H) : pm_fmin(qU2r * y2, 250000.0) * H;
    const double It = P.input ? P.C_e * aH : 0.0;
    double Ek8 = 0.0;
    if ((P.dissipation && P.n_is_2) || P.peak_shift) {
        const double m4 = m2 * m2;
        Ek8 = flux_exp_clamped(lne + lne, -700.0, 700.0) * (m4 * m4);
    }
    double Dt = 0.0;
    if (P.dissipation) {
        if (P.n_is_2) {
            Dt = Ek8 * P.KeT4y;
        } else {
            const double ke = (P.g4rg2 * m2) * P.inv_eT;
            Dt = flux_exp_clamped(P.n * lne, -746.0, 710.0) * flux_exp_clamped((2.0 * P.n) * pm_log(ke), -746.0, 710.0);
        }
    }
    double wrS = 0.0;
    if (P.peak_shift) wrS = (wp * D) * (Ek8 * P.KrCay);

    const double dx = cx * y, dy = cy * y;
    const double ew = e * wp;
    double r[FLUX_NV];
    r[0] = ew * It;
    r[1] = ew * Dt;
    r[2] = e * wrS;
    const double a = wp * r[0], b = wp * r[1], s = (2.0 * ew) * kp;
    r[3] = a * dx; r[4] = a * dy;
    r[5] = b * dx; r[6] = b * dy;
    r[7] = s * dx; r[8] = s * dy;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < FLUX_NV; k++) fin = fin && pm_isfinite(r[k]);
    if (!fin) { out.status = 2; return; }
#pragma unroll
    for (int k = 0; k < FLUX_NV; k++) out.v[k] = r[k];
    out.status = 1;
}

#if defined(__HIPCC__)
/*
 * THE KERNEL.  One lane per coarse cell along x, one workgroup per tile of 256 coarse columns of one coarse row, both in GLOBAL
 * indices (k_diag's decomposition: the tiles, and with them every sum, depend neither on the launch geometry nor on the slabs).
 * Per cell, over its nodes in the order j outer, i inner, from +0.0: the nine sums take the values of the ACTIVE nodes (status 1),
 * n_active and n_bad count statuses 1 and 2.  Plane q of a cell = ((sum_q / n_cover) * scale_q) rounded to float32 (nearest even),
 * n_cover = the nodes the cell covers (cx cy, fewer in a ragged last cell), scale = scale_phi for q < 3, scale_tau for 3 <= q < 7,
 * 1.0 for the Stokes drift; only the planes of the mask are written, in ascending bit order; no NaN is ever written.
 * The tile's partial: the nine UNSCALED sums, n_active, n_bad, each through k_diag's tree (diag_wave_sum: halving inside each wave,
 * then the four waves in ascending order).  4 x 11 LDS words, no atomics.
 *
 * Reads 24 B of State and 16 B of wind per node.  A lane holds ONE node row of its cell in flight (CX doubles of each of the five
 * planes, 16-byte loads where CX and Nx are even), not two as k_diag does.  The reasoning, an EXPECTATION from the instruction
 * listing and not a measurement: a node costs some 150 fp64 instructions (a logarithm, a reciprocal square root, two exponentials,
 * a division) against k_diag's four additions, which puts the arithmetic of a node and its 40 B within a small factor of each other;
 * with that much work behind every load, the loads of the next row can hide under the arithmetic of this one across the waves of
 * the SIMD, and the registers a second row in flight would take (20 at CX = 4) are left to occupancy.  DESIGN.md §27 records what
 * has been measured and what has not.
 */
struct FluxP {
    int Nx, ny_loc;              /* own node rows */
    int cx, cy;
    int Nxc, nyc_loc, tiles_per_row;
    unsigned mask;               /* PICLES_FLUX_* bits */
    double scale_phi, scale_tau;
    long long plane;             /* nodes per State plane (A.n) */
};

__device__ __forceinline__ void flux_add(const KParams &P, double e, double mx, double my, double u, double v, double (&s)[FLUX_NV],
                                         double &na, double &nb)
{
    FluxNode f;
    flux_node(P, e, mx, my, u, v, f);
    if (f.status == 1) {
#pragma unroll
        for (int k = 0; k < FLUX_NV; k++) s[k] = s[k] + f.v[k];
        na = na + 1.0;
    } else if (f.status == 2) {
        nb = nb + 1.0;
    }
}

/* CX > 0: the coarsening factor in x at compile time (VEC: 16-byte loads, needs CX and Nx even); CX == 0: any factor, from F.cx */
template <int CX, bool VEC>
__global__ void __launch_bounds__(DIAG_TILE) k_flux(KParams P, FluxP F, const double *__restrict__ state, const double *__restrict__ wu,
                                                    const double *__restrict__ wv, float *__restrict__ fields, double *__restrict__ partials)
{
    const int cx = CX > 0 ? CX : F.cx;
    const int T = (int)(blockIdx.x % (unsigned)F.tiles_per_row), Jl = (int)(blockIdx.x / (unsigned)F.tiles_per_row);
    const int I = T * DIAG_TILE + (int)threadIdx.x;
    double s[FLUX_NV], na = 0.0, nb = 0.0;
#pragma unroll
    for (int k = 0; k < FLUX_NV; k++) s[k] = 0.0;
    const bool live = I < F.Nxc && Jl < F.nyc_loc;
    if (live) {
        const int i0 = I * cx, i1 = min(i0 + cx, F.Nx);
        const int j0 = Jl * F.cy, j1 = min(j0 + F.cy, F.ny_loc);
        const double *pe = state, *px = state + F.plane, *py = state + 2 * F.plane;
        if (CX > 0 && i0 + CX <= F.Nx) {
            for (int j = j0; j < j1; j++) {
                const long long b = (long long)j * F.Nx + i0;
                double e[CX > 0 ? CX : 1], mx[CX > 0 ? CX : 1], my[CX > 0 ? CX : 1], u[CX > 0 ? CX : 1], v[CX > 0 ? CX : 1];
                if (VEC) {
#pragma unroll
                    for (int k = 0; k < CX; k += 2) {
                        const double2 a = *reinterpret_cast<const double2 *>(pe + b + k);
                        const double2 c = *reinterpret_cast<const double2 *>(px + b + k);
                        const double2 d = *reinterpret_cast<const double2 *>(py + b + k);
                        const double2 g = *reinterpret_cast<const double2 *>(wu + b + k);
                        const double2 h = *reinterpret_cast<const double2 *>(wv + b + k);
                        e[k] = a.x; e[k + 1] = a.y; mx[k] = c.x; mx[k + 1] = c.y; my[k] = d.x; my[k + 1] = d.y;
                        u[k] = g.x; u[k + 1] = g.y; v[k] = h.x; v[k + 1] = h.y;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < CX; k++) { e[k] = pe[b + k]; mx[k] = px[b + k]; my[k] = py[b + k]; u[k] = wu[b + k]; v[k] = wv[b + k]; }
                }
#pragma unroll
                for (int k = 0; k < CX; k++) flux_add(P, e[k], mx[k], my[k], u[k], v[k], s, na, nb);
            }
        } else {
            /* any factor, and the ragged last cell of a row */
            for (int j = j0; j < j1; j++) {
                const long long b = (long long)j * F.Nx;
                for (int i = i0; i < i1; i++) flux_add(P, pe[b + i], px[b + i], py[b + i], wu[b + i], wv[b + i], s, na, nb);
            }
        }
        const double ncov = (double)((i1 - i0) * (j1 - j0));
        const size_t cells = (size_t)F.Nxc * F.nyc_loc;
        float *out = fields + (size_t)I + (size_t)F.Nxc * Jl;
#pragma unroll
        for (int k = 0; k < FLUX_NV; k++) {
            if (F.mask & (1u << k)) {
                const double scale = k < 3 ? F.scale_phi : k < 7 ? F.scale_tau : 1.0;
                *out = (float)((s[k] / ncov) * scale);
                out += cells;
            }
        }
    }
    /* the tile's partial: halving tree inside each wave, then the four waves in ascending order */
#pragma unroll
    for (int k = 0; k < FLUX_NV; k++) s[k] = diag_wave_sum(s[k]);
    na = diag_wave_sum(na); nb = diag_wave_sum(nb);
    __shared__ double red[DIAG_TILE / 64][FLUX_NP];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < FLUX_NV; k++) red[w][k] = s[k];
        red[w][FLUX_NV] = na; red[w][FLUX_NV + 1] = nb;
    }
    __syncthreads();
    if (threadIdx.x < FLUX_NP && Jl < F.nyc_loc) {
        const int q = threadIdx.x;
        double a = red[0][q];
#pragma unroll
        for (int k = 1; k < DIAG_TILE / 64; k++) a = a + red[k][q];
        partials[(size_t)blockIdx.x * FLUX_NP + q] = a;
    }
}
#endif /* __HIPCC__ */

#endif /* PICLES_K_FLUX_H */
