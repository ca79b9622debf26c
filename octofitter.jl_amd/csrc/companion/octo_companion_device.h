// octo_companion_device.h — what the companion libraries that evaluate orbits (csrc/predict, csrc/pointwise) share on top of the main
// library's device routines (octo_kernels.h): the orbit constructor of one (walker, planet), the three primitives of a planet at an epoch,
// the wave sum, and dev_consts. The rule "a companion's arithmetic is astrom_row's / rv_row's on the cold solve" is stated here, once.
// The PSIS library does not include this file: it uses nothing of the main library.
#pragma once

#include "octo_kernels.h"

namespace {
using namespace octo;

constexpr int NEED_AST = 1, NEED_RV = 2;

// octo_api.hip: dev_consts (octo_consts -> DevConsts, five assignments and one quotient). Restated because it is a host function of the main
// library's C ABI translation unit, not reachable by inclusion; tests/test_predict.py pins it to the oracle through every offset and velocity.
inline DevConsts dev_consts(const octo_consts& c) {
    DevConsts d;
    d.k_yr = c.kepler_year_to_julian_day; d.yd = c.year2day_julian; d.au2m = c.au2m; d.sec2yr = c.sec2year_julian;
    d.mas_per_au_per_plx = c.rad2as / c.pc2au;      // cart2angle = plx · rad2as/pc2au   (parameterizations.jl:215-216)
    d.mjup2msol = c.mjup2msol;
    return d;
}

// The three primitives of one planet at epoch t, the arithmetic of astrom_row / rv_row (octo_kernels.h) on the cold solve:
//   raoff = cB·cosE + cG·β·sinE − cB·e, decoff likewise; V = cos(ν + ω) + e·cos ω, radvel = K·V.
__device__ __forceinline__ void planet_prims(const PC& pc, double t, int need, double& ra, double& de, double& V) {
    const KSol s = kepler_solve<2, false>(t, pc);
    ra = 0.0; de = 0.0; V = 0.0;
    if (need & NEED_AST) {
        ra = fma(pc.cB, s.cE, fma(pc.cGb, s.sE, -pc.cBe));
        de = fma(pc.cA, s.cE, fma(pc.cFb, s.sE, -pc.cAe));
    }
    if (need & NEED_RV) {
        const double cnu = (s.cE - pc.e) * s.invD;
        const double snu = pc.beta * s.sE * s.invD;
        V = fma(cnu + pc.e, pc.cw, -(snu * pc.sw));
    }
}

// the orbit constructor of (walker wl, planet p): constants into v[NWC], validity returned — setup_planet_vals<true>, what k_setup runs.
// Args: a library's kernel argument struct; read are .elems, .ld, .c, .orbit_kind and .has_mass.
template <class Args>
__device__ __forceinline__ bool walker_setup(const Args& a, int p, int64_t wl, double (&v)[NWC]) {
    const double* el = a.elems + (int64_t)p * OCTO_N_EL * a.ld + wl;
    double elv[OCTO_N_EL];
#pragma unroll
    for (int k = 0; k < OCTO_N_EL; ++k) elv[k] = el[(int64_t)k * a.ld];
    const SetupOut so = setup_planet_vals<true>(elv, a.c, a.orbit_kind[p], a.has_mass[p]);
#pragma unroll
    for (int k = 0; k < NWC; ++k) v[k] = so.v[k];
    return so.ok;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, WAVE);      // x_i + x_{i^m} on both partners: every lane ends with the same bits
    return x;
}

}  // namespace
