// host_params.h — KParams on the host, for the host builds of the kernels' inline code (flux_host.cpp, stiff_host.cpp): every derived
// constant exactly as picles_create and WindWindow::publish (picles_amd/csrc/picles_hip.hip) derive it, restated here — a context
// whose constants differed would fail the bitwise GPU comparisons.
// TEST INFRASTRUCTURE ONLY: nothing under picles_amd/ includes this file.
#ifndef PICLES_TESTS_HOST_PARAMS_H
#define PICLES_TESTS_HOST_PARAMS_H
#include <cmath>
#include <cstring>

#include "../../include/picles_hip.h"
#include "../../picles_amd/csrc/physics.h"

// the physics (picles_create); minimal_state may be null (min_e = min_m2 = 0)
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
    P.half_inv_rg = 0.5 * P.inv_rg;
    P.two_inv_rg2 = 2.0 * (P.inv_rg * P.inv_rg);
    const double k1 = 0.25 * PK_G0, k2 = k1 * k1, K = k2 * k2;
    P.KeT4 = K * P.inv_eT4;
    P.KrCa = (K * P.r_g) * P.C_alpha;
    P.Cdir = P.C_phi * P.two_inv_rg2;
    P.rg2 = P.r_g * P.r_g;
    const double rg4 = P.rg2 * P.rg2, rg8 = rg4 * rg4;
    P.Cw = (0.5 * PK_G0) * P.r_g;
    P.Chrh = -0.25 * P.r_g;
    P.ymax = 10.0 / P.r_g;
    P.sgmax = 1e8 / P.rg2;
    P.KeT4y = P.KeT4 * rg8;
    P.KrCay = P.KrCa * rg8;
    P.Cs = (0.5 * P.C_phi) * P.rg2;
    P.Cdir2 = 2.0 * P.C_phi;
    P.g4rg2 = k1 * P.rg2;
    P.qU2r_max = 249999.0 / (P.ymax * P.ymax);
    P.deadband2 = p->dir_deadband * p->dir_deadband;
    P.propagation = p->propagation; P.input = p->input; P.dissipation = p->dissipation;
    P.peak_shift = p->peak_shift; P.direction = p->direction; P.n_is_2 = (P.n == 2.0);
    P.p_is_075 = (P.p == 0.75);
    P.fast_phys = P.propagation && P.input && P.dissipation && P.peak_shift && P.direction && P.n_is_2 && P.p_is_075 && P.deadband2 == 0.0;
    if (minimal_state) { P.min_e = minimal_state[0]; P.min_m2 = minimal_state[1]; }
    P.wind_static = 1;      // a static window at t = 0, as picles_create leaves it
}

// the ODE settings (picles_create)
static void host_params_ode(const picles_ode *o, KParams &P)
{
    P.abstol = o->abstol; P.reltol = o->reltol; P.dt0 = o->dt0; P.dtmin = o->dtmin;
    P.inv_abstol = 1.0 / o->abstol;
    P.maxiters = o->maxiters; P.force_dtmin = o->force_dtmin;
    P.solver = o->solver;
    P.lne_max = o->log_energy_maximum; P.wind_min_sq = o->wind_min_squared;
}

// the wind window (WindWindow::publish): dtw <= 0 is the static window; sk in (0, 1) the knot form, 0 the parabola
static void host_params_window(double tw0, double dtw, double sk, KParams &P)
{
    const bool stat = !(dtw > 0.0), knot = !stat && sk > 0.0;
    P.wind_static = stat ? 1 : 0;
    P.tw0 = tw0;
    P.inv_dtw = stat ? 0.0 : 1.0 / dtw;
    P.wind_sk = knot ? sk : 0.0;
    P.wind_isk = knot ? 1.0 / P.wind_sk : 0.0;
    P.wind_i1sk = knot ? 1.0 / (1.0 - P.wind_sk) : 0.0;
    P.wind_nk = knot ? 1 : 0;
}
#endif
