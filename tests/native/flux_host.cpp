// flux_host.cpp — a HOST build of flux_node (picles_amd/csrc/k_flux.h) behind a plain C function: the reference the GPU tests hold
// k_flux against bit for bit, and what tests/test_flux_host.py holds against the literal restatement of the reference's formulas.
// Compiled by the tests with the oracle's flags (-ffp-contract=off).  The derived constants are those of picles_create
// (picles_hip.hip), restated here: a context whose constants differed would fail the bitwise GPU comparison.
// TEST INFRASTRUCTURE ONLY.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/picles_hip.h"
#include "../../picles_amd/csrc/k_flux.h"

static void host_params(const picles_phys *p, const double *minimal_state, KParams &P)
{
    memset(&P, 0, sizeof P);
    P.r_g = p->r_g; P.inv_rg = 1.0 / p->r_g; P.C_alpha = p->C_alpha; P.C_phi = p->C_phi; P.C_e = p->C_e;
    const double q = p->q;
    P.p = (-1.0 - 10.0 * q) / 2.0;
    P.n = 2.0 * q / (P.p + 4.0 * q);
    P.neg2p = -2.0 * P.p;
    const double e_T = std::sqrt(p->c_e * pm_pow(p->c_alpha, -P.p / q) / pm_pow(p->gamma * p->c_beta * p->c_D, 1.0 / P.n));
    P.inv_eT = 1.0 / e_T;
    P.inv_eT4 = (P.inv_eT * P.inv_eT) * (P.inv_eT * P.inv_eT);
    const double k1 = 0.25 * PK_G0, k2 = k1 * k1, K = k2 * k2;
    P.KeT4 = K * P.inv_eT4;
    P.KrCa = (K * P.r_g) * P.C_alpha;
    P.rg2 = P.r_g * P.r_g;
    const double rg4 = P.rg2 * P.rg2, rg8 = rg4 * rg4;
    P.Cw = (0.5 * PK_G0) * P.r_g;
    P.Chrh = -0.25 * P.r_g;
    P.ymax = 10.0 / P.r_g;
    P.sgmax = 1e8 / P.rg2;
    P.KeT4y = P.KeT4 * rg8;
    P.KrCay = P.KrCa * rg8;
    P.g4rg2 = k1 * P.rg2;
    P.qU2r_max = 249999.0 / (P.ymax * P.ymax);
    P.propagation = p->propagation; P.input = p->input; P.dissipation = p->dissipation;
    P.peak_shift = p->peak_shift; P.direction = p->direction; P.n_is_2 = (P.n == 2.0);
    P.p_is_075 = (P.p == 0.75);
    P.min_e = minimal_state[0]; P.min_m2 = minimal_state[1];
}

extern "C" {
// n nodes: out[9 k .. 9 k + 9) the nine values of node k, status[k] 0 / 1 / 2 (not active / active / bad)
__attribute__((visibility("default"))) void flux_host_nodes(const picles_phys *p, const double *minimal_state, int64_t n, const double *e,
                                                            const double *mx, const double *my, const double *u, const double *v,
                                                            double *out, int32_t *status)
{
    KParams P;
    host_params(p, minimal_state, P);
    for (int64_t k = 0; k < n; k++) {
        FluxNode f;
        flux_node(P, e[k], mx[k], my[k], u[k], v[k], f);
        for (int q = 0; q < FLUX_NV; q++) out[FLUX_NV * k + q] = f.v[q];
        status[k] = f.status;
    }
}
}
