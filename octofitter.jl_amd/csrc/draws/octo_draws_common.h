// octo_draws_common.h — what the translation units of liboctofitter_hip_draws.so share: the handle, the counter generator, the prior
// helpers on top of octo_model.h's device routines, the tempered target of the two samplers, and the argument checks their functions repeat.
// Seven units include it: octo_draws.hip (the draws and the two drivers that consume a batch of them), octo_draws_hmc.hip (the tempered HMC
// explorer), octo_draws_nuts.hip (the no-U-turn sampler), octo_draws_lbfgs.hip (the multi-start L-BFGS), octo_draws_pathfinder.hip (Pathfinder
// on its paths), octo_draws_adapt.hip (the warm-up statistics of the explorer) and octo_draws_diag.hip (the convergence diagnostics of stored draws). Everything but the handle lives in an unnamed namespace,
// one copy per unit. How the handle's work allocations are cut into their parts is octo_draws_layout.h.
// It stays under csrc/draws/: csrc/companion/ holds only what EVERY companion library shares.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "octo_companion_host.h"
#include "octo_draws_layout.h"
#include "octo_model.h"
#include "octofitter_hip_draws.h"

namespace {
using namespace octo;

constexpr uint64_t PHILOX_M0 = 0xD2E7470EE14C6C93ull, PHILOX_M1 = 0xCA5A826395121157ull;
constexpr uint64_t PHILOX_W0 = 0x9E3779B97F4A7C15ull, PHILOX_W1 = 0xBB67AE8584CAA73Bull;
constexpr uint64_t KEY1 = 0x6f63746f64726177ull;      // "octodraw"
constexpr int TPB = 256;
constexpr int IC_N = 4;                               // inverse-CDF constants per prior
constexpr int64_t MAX_CHAINS = (int64_t)1 << 30;      // one launch: 2²² blocks
constexpr double HEALED = -1.7976931348623157e308;    // the sentinel of a healed prior (k_model_fwd)

// Philox4x64-10 (Salmon et al. 2011), the variant NumPy ships: ten rounds, the key bumped after each.
__device__ __forceinline__ void philox4x64(uint64_t k0, uint64_t k1, uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t hi0 = __umul64hi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint64_t hi1 = __umul64hi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// (2·(x >> 12) + 1)·2⁻⁵³: an odd multiple of 2⁻⁵³ below 1 — exact, never 0 or 1
__device__ __forceinline__ double u01(uint64_t x) { return (double)(2 * (x >> 12) + 1) * 0x1p-53; }

// Quantile of the prior at u, strictly inside the support the bijector assumes (prior_bounds). ic: constants made at octo_draws_create —
//   Uniform {a, b − a} · LogUniform {log a, log b − log a} · truncated Normal {P0, ΔP, mirrored} with α = (lo − μ)/σ, β = (hi − μ)/σ:
//   α < 0: z = Φ⁻¹(Φ(α) + u(Φ(β) − Φ(α))) · α >= 0 (a tail): z = −Φ⁻¹(Φ(−α) − u(Φ(−α) − Φ(−β))), so that the tail keeps its digits.
// The coordinate d is the same for every lane, so the branch on the kind is wave-uniform.
__device__ __forceinline__ double prior_quantile(const octo_prior& pr, const PriorBounds& B, const double* __restrict__ ic, double u) {
    double x;
    switch (pr.kind) {
    case OCTO_PRIOR_UNIFORM: x = ic[0] + ic[1] * u; break;
    case OCTO_PRIOR_LOGUNIFORM: x = exp(ic[0] + u * ic[1]); break;
    case OCTO_PRIOR_NORMAL: x = pr.p0 + pr.p1 * normcdfinv(u); break;
    case OCTO_PRIOR_TRUNCNORMAL: {
        const bool mirrored = ic[2] != 0.0;
        double p = mirrored ? ic[0] - u * ic[1] : ic[0] + u * ic[1];
        p = fmin(fmax(p, 2.2250738585072014e-308), 1.0 - 0x1p-53);      // a probability that rounded onto 0 or 1 has no finite quantile
        const double z = normcdfinv(p);
        x = pr.p0 + pr.p1 * (mirrored ? -z : z);
        break;
    }
    default: x = acos(1.0 - 2.0 * u); break;                              // Sine: distributions.jl:39
    }
    if (B.fa && !(x > B.a)) x = nextafter(B.a, INFINITY);
    if (B.fb && !(x < B.b)) x = nextafter(B.b, -INFINITY);
    return x;
}

// Bijectors.link (TruncatedBijector), the inverse of prior_link_lanes; host/priors.py: Prior.link is its executable statement
__device__ __forceinline__ double prior_link_forward(const PriorBounds& B, double x) {
    if (B.both) {
        double u = (x - B.a) / (B.b - B.a);
        u = fmin(fmax(u, 2.2250738585072014e-308), 1.0 - 0x1p-53);        // x is inside (a, b); the quotient may still round onto 1
        return log(u) - log1p(-u);
    }
    if (B.fa) return log(x - B.a);
    if (B.fb) return log(B.b - x);
    return x;
}

// ---- the tempered target of the HMC step and of NUTS (include/octofitter_hip_draws.h, "Target" and "Decision")
// E = ℓprior_t + β(ℓπ − ℓprior_t); β = 0 never consults ℓπ
__device__ __forceinline__ double tempered_energy(double beta, double lp, double lpt) { return beta == 0.0 ? lpt : lpt + beta * (lp - lpt); }

__device__ __forceinline__ bool dead_state(double beta, double E, double lp, double lpt) {
    return !isfinite(E) || lpt == HEALED || (beta > 0.0 && !isfinite(lp));
}

// ∇E at offset o from ∇ℓπ (glp, read only where β != 0: null without a model) and ∇ℓprior_t there (gp); β = 1 takes ∇ℓπ bit for bit
__device__ __forceinline__ double tempered_gradient(double beta, const double* glp, int64_t o, double gp) {
    return beta == 1.0 ? glp[o] : (beta == 0.0 ? gp : beta * glp[o] + (1.0 - beta) * gp);
}

// ℓprior_t of chain wl at the point `at` [D][ld]: every transcendental (link, density), summed in declaration order — the routine and the
// order of k_draw's logprior_t. It leaves ∇ℓprior_t in gpr (live lanes: w = wl) because whether the prior was healed (and its derivative is 0
// in EVERY coordinate, as k_model_fwd has it) is known only after the last coordinate. prior_link_lanes and prior_density_lanes vote across
// the wave: every lane of a wave calls this, a lane beyond the batch with the last chain's column.
__device__ __forceinline__ double prior_loop(const octo_prior* priors, const double* pc, int32_t D, const double* __restrict__ at, int64_t ld, int64_t w,
                                             int64_t wl, bool live, double* gpr, bool& healed) {
    double lpt = 0.0;
    healed = false;
    for (int d = 0; d < D; ++d) {
        const octo_prior pr = priors[d];
        double xv, xd, pv, pd;
        prior_link_lanes(pr, at[(int64_t)d * ld + wl], xv, xd);
        prior_density_lanes(pr, xv, xd, pv, pd, pc + PRIOR_NC * d);
        healed = healed || !isfinite(pv);
        lpt += pv;
        if (live) gpr[(int64_t)d * ld + w] = pd;
    }
    return healed ? HEALED : lpt;
}

}  // namespace

struct octo_draws : CompanionBase {
    octo_ctx* ctx = nullptr;
    octo_model* model = nullptr;
    int D = 0;
    bool ctx_on_stream = false;      // the context was handed a stream (octo_model_logpost_device) and may still name it as its last stream
    octo_prior* d_priors = nullptr;
    double *d_pc = nullptr, *d_ic = nullptr;
    // the drivers (octo_draws.hip), one allocation per group: the chunk buffers and candidate lists (fixed size), the per-draw arrays of a
    // call and the outputs before they go to the host (both grown on demand)
    double* d_chunk = nullptr; int64_t cap_chunk = 0;
    double* d_arr = nullptr; int64_t cap_arr = 0;
    double* d_out = nullptr; int64_t cap_out = 0;
    // the explorer (octo_draws_hmc.hip), grown on demand: its work arrays in one allocation, and the device side of the host-buffer call
    double* d_hmc = nullptr; int64_t cap_hmc = 0;
    double* d_hst = nullptr; int64_t cap_hst = 0;
    // the L-BFGS (octo_draws_lbfgs.hip), grown on demand: the chains' state in one allocation with the shape it was opened for (lbf_m = 0:
    // nothing to resume), and the coefficients of the direction call
    double* d_lbf = nullptr; int64_t cap_lbf = 0;
    int64_t lbf_W = 0, lbf_ld = 0; int32_t lbf_m = 0;
    double* d_lbd = nullptr; int64_t cap_lbd = 0;
    // Pathfinder (octo_draws_pathfinder.hip), grown on demand: the chains' fits in one allocation with the shape it was opened for (pf_W = 0:
    // nothing to resume or to draw from), and the transient work of a call (the ELBO batch; √α of the fit call)
    double* d_pf = nullptr; int64_t cap_pf = 0;
    int64_t pf_W = 0, pf_ld = 0;
    double* d_pfb = nullptr; int64_t cap_pfb = 0;
    // warm-up (octo_draws_adapt.hip), grown on demand: the block partials of the grouped moments
    double* d_mom = nullptr; int64_t cap_mom = 0;
    // NUTS (octo_draws_nuts.hip), grown on demand: the chains' trees in one allocation with the transition it was opened for (nuts_depth = 0:
    // nothing to resume)
    double* d_nuts = nullptr; int64_t cap_nuts = 0;
    int64_t nuts_W = 0, nuts_ld = 0; int32_t nuts_depth = 0;
    uint64_t nuts_seed = 0, nuts_step = 0, nuts_chain0 = 0;
    // the convergence diagnostics (octo_draws_diag.hip), grown on demand: sorted keys, rank-normalised draws, the chains' moments, ρ
    double* d_diag = nullptr; int64_t cap_diag = 0;
};

namespace {

inline int main_call(octo_draws* h, int rc, const char* what) {
    h->ctx_on_stream = true;
    if (rc == OCTO_OK) return rc;
    const char* m = octo_last_error(h->ctx);
    return fail(h, rc, std::string(what) + ": " + (m ? m : ""));
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + TPB - 1) / TPB)); }

// the allocation (p, cap) grown to hold layout(args…), and its parts
template <class S, class F, class... A>
int grow_to(octo_draws* h, double*& p, int64_t& cap, S& parts, F layout, A... args) {
    const int rc = grow(h, p, cap, carve_size(layout, args...));
    parts = carve_at(p, layout, args...);
    return rc;
}

// The argument checks the functions share: who = the function's name, the rest of the message is the same in each.
inline int check_model(octo_draws* h, const char* who) {
    return h->model && h->ctx ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no model (created without one, or detached)");
}
inline int check_m(octo_draws* h, const char* who, int32_t m) {
    return m >= 1 && m <= OCTO_DRAWS_LBFGS_MAX_M ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": m must be 1 ... OCTO_DRAWS_LBFGS_MAX_M");
}
inline int check_chains(octo_draws* h, const char* who, int64_t W, int64_t ld, int64_t limit, const char* limit_text) {      // "2^30": limit as the message spells it
    return W >= 0 && ld >= W && W <= limit ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= W <= ld, W <= " + limit_text);
}
inline int check_tolerances(octo_draws* h, const char* who, double gtol, double ftol) {
    if (!(std::isfinite(gtol) && gtol >= 0.0)) return fail(h, OCTO_EINVAL, std::string(who) + ": gtol must be finite and >= 0");
    return std::isfinite(ftol) && ftol >= 0.0 ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": ftol must be finite and >= 0");
}

}  // namespace
