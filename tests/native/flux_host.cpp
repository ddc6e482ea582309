// flux_host.cpp — a HOST build of flux_node (picles_amd/csrc/k_flux.h) behind a plain C function: the reference the GPU tests hold
// k_flux against bit for bit, and what tests/test_flux_host.py holds against the literal restatement of the reference's formulas.
// Compiled by the tests with the oracle's flags (-ffp-contract=off).  The derived constants are those of picles_create
// (picles_hip.hip), restated in host_params.h: a context whose constants differed would fail the bitwise GPU comparison.
// TEST INFRASTRUCTURE ONLY.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_params.h"
#include "../../picles_amd/csrc/k_flux.h"

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
