/*
 * k_diag.h — device-side wave diagnostics (picles_diag_*, include/picles_hip.h "coarse wave diagnostics"): one pass over State
 * that writes the coarsened float32 planes (Hs, Tp, cg, E, M) and one partial of seven doubles per tile of 256 coarse cells.
 * Included by picles_hip.hip (not a translation unit of its own).
 *
 * One lane per coarse cell along x, one workgroup per tile: 256 consecutive coarse columns I of one coarse row J, both in GLOBAL
 * indices, so that the tiles — and with them every sum — do not depend on the launch geometry or on the slab decomposition.
 * A wave's loads of one node row are contiguous (CX doubles per lane, 64 lanes side by side); with an even CX on a grid whose Nx
 * is even they are 16-byte loads.  The fields need no LDS; the tile reduction is a shuffle tree per wave and 4 x 7 LDS words.
 * Streaming kernel: 24 B per node read, 4 B per coarse cell and selected field written.  HBM bound once a lane covers several
 * nodes; at (1,1) the fp64 divisions and square roots of the planes and the 42 double shuffles of the tile reduction, paid per
 * node, bind it to VALU issue instead (DESIGN.md §12 has the measured rates).
 */
#ifndef PICLES_K_DIAG_H
#define PICLES_K_DIAG_H

#define DIAG_TILE 256            /* coarse cells per workgroup = lanes per workgroup (PICLES_DIAG_TILE of the header) */
#define DIAG_FOUR_PI 12.566370614359172      /* 4·M_PI as a double */

struct DiagP {
    int Nx, ny_loc;              /* own node rows */
    int cx, cy;
    int Nxc, nyc_loc, tiles_per_row;
    unsigned mask;               /* PICLES_DIAG_* bits */
    double g, r_g;
    long long plane;             /* nodes per State plane (A.n) */
};

/* one node of a coarse cell, in the cell's fixed order: sums take wet nodes only, maxima every node (fmax skips a NaN) */
__device__ __forceinline__ void diag_node(double e, double mx, double my, double &se, double &sx, double &sy, double &n,
                                          double &xe, double &xx, double &xy)
{
    xe = __builtin_fmax(xe, e); xx = __builtin_fmax(xx, mx); xy = __builtin_fmax(xy, my);
    const double m2 = mx * mx + my * my;
    const bool wet = __builtin_isfinite(e) && __builtin_isfinite(mx) && __builtin_isfinite(my) && e > 0.0 && m2 > 0.0;
    if (wet) { se = se + e; sx = sx + mx; sy = sy + my; n = n + 1.0; }
}

/* lane l <- v[l] + v[l + s] for s = 32, 16, 8, 4, 2, 1: lane 0 of the wave ends with the halving tree over its 64 lanes */
__device__ __forceinline__ double diag_wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
    return v;
}
__device__ __forceinline__ double diag_wave_max(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = __builtin_fmax(v, __shfl_down(v, s, 64));
    return v;
}

/* CX > 0: the coarsening factor in x at compile time (the row loads of a lane unroll; VEC: 16-byte loads, needs CX and Nx even);
 * CX == 0: any factor, read from D.cx */
template <int CX, bool VEC>
__global__ void __launch_bounds__(DIAG_TILE) k_diag(DiagP D, const double *__restrict__ state, float *__restrict__ fields,
                                                    double *__restrict__ partials)
{
    const int cx = CX > 0 ? CX : D.cx;
    const int T = (int)(blockIdx.x % (unsigned)D.tiles_per_row), Jl = (int)(blockIdx.x / (unsigned)D.tiles_per_row);
    const int I = T * DIAG_TILE + (int)threadIdx.x;
    const double NEG_INF = -__builtin_inf();
    double se = 0.0, sx = 0.0, sy = 0.0, n = 0.0, xe = NEG_INF, xx = NEG_INF, xy = NEG_INF;
    const bool live = I < D.Nxc && Jl < D.nyc_loc;
    if (live) {
        const int i0 = I * cx, i1 = min(i0 + cx, D.Nx);
        const int j0 = Jl * D.cy, j1 = min(j0 + D.cy, D.ny_loc);
        const double *pe = state, *px = state + D.plane, *py = state + 2 * D.plane;
        if (CX > 0 && i0 + CX <= D.Nx) {
            /* a whole cell: CX doubles of each plane per row, all loaded before the first is used */
#pragma unroll 2
            for (int j = j0; j < j1; j++) {
                const long long b = (long long)j * D.Nx + i0;
                double e[CX > 0 ? CX : 1], mx[CX > 0 ? CX : 1], my[CX > 0 ? CX : 1];
                if (VEC) {
#pragma unroll
                    for (int k = 0; k < CX; k += 2) {
                        const double2 a = *reinterpret_cast<const double2 *>(pe + b + k);
                        const double2 c = *reinterpret_cast<const double2 *>(px + b + k);
                        const double2 d = *reinterpret_cast<const double2 *>(py + b + k);
                        e[k] = a.x; e[k + 1] = a.y; mx[k] = c.x; mx[k + 1] = c.y; my[k] = d.x; my[k + 1] = d.y;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < CX; k++) { e[k] = pe[b + k]; mx[k] = px[b + k]; my[k] = py[b + k]; }
                }
#pragma unroll
                for (int k = 0; k < CX; k++) diag_node(e[k], mx[k], my[k], se, sx, sy, n, xe, xx, xy);
            }
        } else {
            /* any factor, and the ragged last cell of a row */
            for (int j = j0; j < j1; j++) {
                const long long b = (long long)j * D.Nx;
                for (int i = i0; i < i1; i++) diag_node(pe[b + i], px[b + i], py[b + i], se, sx, sy, n, xe, xx, xy);
            }
        }
        /* the cell's planes: every operation one correctly rounded IEEE operation, in the order of the header; only the selected
         * planes are computed (the mask is uniform).  x / 1.0 is x: a cell with one wet node skips the three divisions, and one
         * with none is not valid whatever its averages are */
        double E = se, MX = sx, MY = sy;
        if (n > 1.0) { E = se / n; MX = sx / n; MY = sy / n; }
        const double M2 = MX * MX + MY * MY;
        const bool valid = n > 0.0 && M2 > 0.0;
        const float qnan = __builtin_nanf("");
        const size_t cells = (size_t)D.Nxc * D.nyc_loc;
        float *out = fields + (size_t)I + (size_t)D.Nxc * Jl;
        if (D.mask & PICLES_DIAG_HS) { *out = valid ? (float)(4.0 * __builtin_sqrt(E)) : qnan; out += cells; }
        if (D.mask & PICLES_DIAG_TP) {
            const double cbar = E / (2.0 * __builtin_sqrt(M2));
            *out = valid ? (float)((DIAG_FOUR_PI * __builtin_fmax(cbar / D.r_g, 0.1)) / D.g) : qnan; out += cells;
        }
        if (D.mask & (PICLES_DIAG_CG_X | PICLES_DIAG_CG_Y)) {
            const double two_m2 = 2.0 * M2;
            if (D.mask & PICLES_DIAG_CG_X) { *out = valid ? (float)((MX * E) / two_m2) : qnan; out += cells; }
            if (D.mask & PICLES_DIAG_CG_Y) { *out = valid ? (float)((MY * E) / two_m2) : qnan; out += cells; }
        }
        if (D.mask & PICLES_DIAG_E) { *out = valid ? (float)E : qnan; out += cells; }
        if (D.mask & PICLES_DIAG_MX) { *out = valid ? (float)MX : qnan; out += cells; }
        if (D.mask & PICLES_DIAG_MY) { *out = valid ? (float)MY : qnan; out += cells; }
    }
    /* the tile's partial: halving tree inside each wave, then the four waves in ascending order */
    se = diag_wave_sum(se); sx = diag_wave_sum(sx); sy = diag_wave_sum(sy); n = diag_wave_sum(n);
    xe = diag_wave_max(xe); xx = diag_wave_max(xx); xy = diag_wave_max(xy);
    __shared__ double red[DIAG_TILE / 64][8];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w][0] = se; red[w][1] = sx; red[w][2] = sy; red[w][3] = n; red[w][4] = xe; red[w][5] = xx; red[w][6] = xy;
    }
    __syncthreads();
    if (threadIdx.x < 7 && Jl < D.nyc_loc) {
        const int q = threadIdx.x;
        double a = red[0][q];
#pragma unroll
        for (int k = 1; k < DIAG_TILE / 64; k++) a = q < 4 ? a + red[k][q] : __builtin_fmax(a, red[k][q]);
        if (q >= 4) a = a + 0.0;          /* a zero maximum is +0.0 whichever zero fmax kept */
        partials[(size_t)blockIdx.x * 7 + q] = a;
    }
}

#endif /* PICLES_K_DIAG_H */
