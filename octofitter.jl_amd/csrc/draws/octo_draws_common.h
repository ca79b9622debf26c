// octo_draws_common.h — what the translation units of liboctofitter_hip_draws.so share: the handle, the counter generator, the prior
// helpers on top of octo_model.h's device routines, the argument checks their functions repeat, and what the lockstep algorithms have in
// common. On the device: the metric (inv_mass_at, momentum_of: the only readers of inv_mass), the head of the two samplers' kernel arguments
// (SamplerHead), the per-lane preamble (Chain, chain_of) and the tempered target at a point (Target, target_at over prior_loop, tempered_energy,
// dead_state). On the host: check_sampler_call, sampler_head, logpost_at (every octo_model_logpost_device call of the four units) and
// run_rounds (the round driver of the L-BFGS and of NUTS).
// The fourteenth part, the dense metric (octo_draws_dense.hip: pooled covariance, its Cholesky factor, the products with it), adds metric_lower and
// metric_lower_t to the metric and metric_gradient behind the target: the HMC step and NUTS reach a factor through these alone.
// Eleven units include it (the eleventh: octo_draws_program.hip, the expression programs of derived variables, which logpost_at chooses over the model;
// the tenth: octo_draws_vref.hip, the reference table of a variational tempering leg and the exchange of two legs' target
// replicas, which take prior_loop and the handle's active table): octo_draws.hip (the draws and the two drivers that consume a batch of them), octo_draws_hmc.hip (the tempered HMC
// explorer), octo_draws_nuts.hip (the no-U-turn sampler), octo_draws_slice.hip (the slice sampler, which takes the samplers' head, preamble, target
// and round driver without a gradient), octo_draws_lbfgs.hip (the multi-start L-BFGS), octo_draws_pathfinder.hip (Pathfinder
// on its paths), octo_draws_adapt.hip (the warm-up statistics of the explorer), octo_draws_diag.hip (the convergence diagnostics of stored draws) and
// octo_draws_pt.hip (the tempering statistics between the scans, which take wave_sum and waves_total). Everything but the handle lives in an unnamed namespace,
// one copy per unit. How the handle's work allocations are cut into their parts is octo_draws_layout.h.
// The thirteenth part of the library, nested sampling (octo_draws_nested.hip), takes DrawArgs, cube_link and draw_block (what k_draw does after its Philox
// call) beside the samplers' head, preamble, target and round driver.
// The fifteenth part, differential evolution (octo_draws_de.hip), takes the samplers' head, preamble, target, dead test and round driver as the slice
// sampler does, one generation a run_rounds call of one round.
// The sixteenth part, the OFTI rejection sampler (octo_draws_ofti.hip), takes the generator, the handle and grow_to, and from octo_draws.hip the draw
// launches and the rejection's second pass (draws_launch_draw, draws_max_pass, draws_accept_pass below).
// The seventeenth part, along-scan absolute astrometry (octo_draws_scan.hip), takes the handle, grow_to and the argument checks; the expression program
// calls its draws_scan_accumulate (below) between octo_eval_device and k_prog_bwd while a table is bound.
// The eighteenth part, the catalogue proper-motion anomaly (octo_draws_pma.hip), takes the same and hands the program draws_pma_accumulate; its table
// algebra is octo_draws_pma_host.h.
// The nineteenth part, the Gaussian-process RV term (octo_draws_gp.hip), takes the same and hands the program draws_gp_accumulate.
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
#include "octo_draws_pma_host.h"
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

// ---- a draw from its uniforms: what k_draw does after its Philox call, and the hypercube transform of nested sampling (octo_draws_nested.hip)
struct DrawArgs {
    const octo_prior* priors;      // [D]
    const double* pc;              // [D][PRIOR_NC] constants of prior_density_lanes
    const double* ic;              // [D][IC_N] constants of prior_quantile
    const uint64_t* idx;           // [n] draw indices, or null: first + t
    uint64_t seed, first;
    int64_t n, ld;
    int32_t D, d0;                 // this launch: coordinates d0 … d0 + 3 (d0 a multiple of 4)
    double* theta; double* theta_t; double* lpt;
};

// θ = the quantile of u (one ulp inside a bound it rounds onto) and θ_t = its link: the one routine that takes a cube coordinate to θ_t
__device__ __forceinline__ double cube_link(const octo_prior& pr, const PriorBounds& B, const double* __restrict__ ic, double u, double& x) {
    x = prior_quantile(pr, B, ic, u);
    return prior_link_forward(B, x);
}

// Coordinates [d0, d0 + 4) ∩ [0, D) of draw t from their uniforms u: quantile -> link -> density, logprior_t carried through a.lpt from launch to
// launch in declaration order with the healing sentinel. Every lane of a wave calls it (prior_density_lanes votes), a lane beyond the batch as
// tl = the last draw. bad: the draw's outputs are NaN (a cube point outside (0, 1); its u are then read as ½) — k_draw passes false.
__device__ __forceinline__ void draw_block(const DrawArgs& a, int64_t t, int64_t tl, bool live, const double (&u)[4], bool bad) {
    const bool want_t = a.theta_t != nullptr || a.lpt != nullptr;
    double lp = 0.0;
    bool healed = false;
    if (a.lpt && a.d0 > 0) { lp = a.lpt[tl]; healed = lp == HEALED; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = a.d0 + q;
        if (d >= a.D) break;
        const octo_prior pr = a.priors[d];
        const PriorBounds B = prior_bounds(pr);
        const double x = prior_quantile(pr, B, a.ic + IC_N * d, u[q]);
        if (a.theta && live) a.theta[(int64_t)d * a.ld + t] = bad ? NAN : x;
        if (!want_t) continue;
        const double y = prior_link_forward(B, x);
        if (a.theta_t && live) a.theta_t[(int64_t)d * a.ld + t] = bad ? NAN : y;
        if (a.lpt) {
            // what the model callback does with this θ_t: x' = invlink(y), logpdf_with_trans at x', the healing rule (k_model_fwd)
            double xv, xd, pv, pd;
            prior_link_lanes(pr, y, xv, xd);
            prior_density_lanes(pr, xv, xd, pv, pd, a.pc + PRIOR_NC * d);
            healed = healed || !isfinite(pv);
            lp += pv;
        }
    }
    if (a.lpt && live) a.lpt[t] = bad ? NAN : (healed ? HEALED : lp);
}

// ---- the cross-chain sums of the warm-up statistics, the diagnostics and the tempering statistics (octo_draws_adapt.hip, _diag.hip, _pt.hip)
// the sum over the 64 lanes, the same bits in every lane (IEEE addition commutes, so both sides of every exchange add the same pair)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the four waves' sums of a block of TPB lanes in wave order from 0
__device__ __forceinline__ double waves_total(const double (&s)[TPB / 64]) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < TPB / 64; ++q) t += s[q];
    return t;
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

// ---- the metric: every use of inv_mass in the library goes through these two
// m⁻¹ of coordinate d of the diagonal metric inv_mass [D], null = the identity
__device__ __forceinline__ double inv_mass_at(const double* inv_mass, int d) { return inv_mass ? inv_mass[d] : 1.0; }
// the momentum p = z/√m⁻¹ of a standard normal z (a null metric takes z bit for bit)
__device__ __forceinline__ double momentum_of(const double* inv_mass, int d, double z) { return inv_mass ? z / sqrt(inv_mass[d]) : z; }
// The dense metric M⁻¹ = L·Lᵀ (octo_draws_use_metric): L lower-triangular, packed by rows (row i at i(i+1)/2), one factor for all chains — its
// index is wave-uniform, so it comes through the scalar cache. x is one lane's column of a [D][ld] array at offset w; D <= OCTO_DRAWS_DENSE_MAX_D
// is a run-time value and nothing of the column is kept in a private array: it is read again through the caches. put(i, v) receives the
// products; every sum runs over the coordinate index in ascending order by fma, so a product has the same bits wherever it is formed.
// (L·x)_i for i = D − 1 … 0: put may overwrite x_i (no later i reads it), which forms the product in place
template <class Put>
__device__ __forceinline__ void metric_lower(const double* __restrict__ L, int32_t D, const double* x, int64_t ld, int64_t w, Put put) {
    for (int i = D - 1; i >= 0; --i) {
        const double* __restrict__ row = L + (i * (i + 1) >> 1);
        double s = 0.0;
        for (int j = 0; j <= i; ++j) s = fma(row[j], x[(int64_t)j * ld + w], s);
        put(i, s);
    }
}
// (Lᵀ·x)_j for j = 0 … D − 1: put may overwrite x_j likewise
template <class Put>
__device__ __forceinline__ void metric_lower_t(const double* __restrict__ L, int32_t D, const double* x, int64_t ld, int64_t w, Put put) {
    for (int j = 0; j < D; ++j) {
        double s = 0.0;
        for (int i = j; i < D; ++i) s = fma(L[(i * (i + 1) >> 1) + j], x[(int64_t)i * ld + w], s);
        put(j, s);
    }
}

// ---- the head of the two samplers' kernel arguments (HmcArgs, NutsArgs derive from it), filled by sampler_head
struct SamplerHead {
    const octo_prior* priors;      // [D]
    const double* pc;              // [D][PRIOR_NC]
    const double* beta;            // [W] or null = 1 (ignored without a model: 0)
    const double* eps_w;           // [W] or null = eps
    const double* inv_mass;        // [D] or null = 1
    double eps;
    uint64_t seed, step, chain0;
    int64_t W, ld;
    int32_t D, has_model;
    double* theta_t;               // [D][ld] the caller's states
};

// The chain of a lane: w its index, live = it is inside the batch, wl = the column it reads (a lane beyond the batch: the last chain's), its
// β and ε. No kernel leaves a lane out ahead of target_at: prior_loop votes across the wave, so EVERY lane of the wave goes on to it.
struct Chain {
    int64_t w, wl;
    bool live;
    double beta, eps;
};
__device__ __forceinline__ Chain chain_of(const SamplerHead& a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool live = w < a.W;
    const int64_t wl = live ? w : a.W - 1;
    return {w, wl, live, a.has_model ? (a.beta ? a.beta[wl] : 1.0) : 0.0, a.eps_w ? a.eps_w[wl] : a.eps};
}

// The target of chain c at the point `at` [D][ld]: ℓprior_t and whether the prior was healed (prior_loop; gpr [D][ld] receives ∇ℓprior_t), ℓπ from
// lp [W] and ∇E at offset o from glp [D][ld] (∇ℓπ; both null without a model) and gpr, with ∇ℓprior_t = 0 in every coordinate of a healed
// prior. ℓπ is 0 without a model (E and ∇E consult it only where β != 0, the outputs report it for every chain). lp(column) reads it where
// the kernel asks: k_nuts_open and k_nuts_leaf do so once the lanes beyond the batch have left (read ahead of that exit, each takes 4 more VGPRs).
struct Target {
    double lpt, beta;
    bool healed;
    int32_t has_model;
    const double *lpi, *glp, *gpr;
    __device__ __forceinline__ double lp(int64_t w) const { return has_model ? lpi[w] : 0.0; }
    __device__ __forceinline__ double grad(int64_t o) const { return tempered_gradient(beta, glp, o, healed ? 0.0 : gpr[o]); }
};
__device__ __forceinline__ Target target_at(const SamplerHead& a, const Chain& c, const double* __restrict__ at, const double* lp, const double* glp, double* gpr) {
    Target t;
    t.lpt = prior_loop(a.priors, a.pc, a.D, at, a.ld, c.w, c.wl, c.live, gpr, t.healed);
    t.beta = c.beta; t.has_model = a.has_model; t.lpi = lp; t.glp = glp; t.gpr = gpr;
    return t;
}

// ∇E of chain column w in the coordinates the momenta live in, for d = 0 … D − 1 in that order: body(d, o, g), o = d·ld + w. The diagonal metric
// keeps p itself and g = ∇E_d. DENSE (the whitened momenta r = Lᵀp of a factor L): the mixed gradient tg.grad — ∇ℓπ and ∇ℓprior_t by β — goes to
// the column gpr, whose ∇ℓprior_t is spent by then, and g = (Lᵀ∇E)_d is formed on it in place.
template <bool DENSE, class Body>
__device__ __forceinline__ void metric_gradient(const Target& tg, const double* chol, double* gpr, int32_t D, int64_t ld, int64_t w, Body body) {
    if (DENSE) {
        for (int d = 0; d < D; ++d) { const int64_t o = (int64_t)d * ld + w; gpr[o] = tg.grad(o); }
        metric_lower_t(chol, D, gpr, ld, w, [&](int d, double g) { const int64_t o = (int64_t)d * ld + w; gpr[o] = g; body(d, o, g); });
    } else
        for (int d = 0; d < D; ++d) { const int64_t o = (int64_t)d * ld + w; body(d, o, tg.grad(o)); }
}

}  // namespace

struct octo_draws : CompanionBase {
    octo_ctx* ctx = nullptr;
    octo_model* model = nullptr;
    int D = 0;
    bool ctx_on_stream = false;      // the context was handed a stream (octo_model_logpost_device) and may still name it as its last stream
    // the ACTIVE prior table, what every function reads: the handle's own (own_*, made by octo_draws_create and freed by octo_draws_destroy) or
    // a caller's reference table (octo_draws_use_reference, octo_draws_vref.hip)
    octo_prior* d_priors = nullptr;
    double *d_pc = nullptr, *d_ic = nullptr;
    octo_prior* own_priors = nullptr;
    double *own_pc = nullptr, *own_ic = nullptr;
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
    // warm-up (octo_draws_adapt.hip) and the tempering statistics (octo_draws_pt.hip), grown on demand: the block partials of a call's sums
    double* d_mom = nullptr; int64_t cap_mom = 0;
    // NUTS (octo_draws_nuts.hip), grown on demand: the chains' trees in one allocation with the transition it was opened for (nuts_depth = 0:
    // nothing to resume)
    double* d_nuts = nullptr; int64_t cap_nuts = 0;
    int64_t nuts_W = 0, nuts_ld = 0; int32_t nuts_depth = 0;
    uint64_t nuts_seed = 0, nuts_step = 0, nuts_chain0 = 0;
    // the convergence diagnostics (octo_draws_diag.hip), grown on demand: sorted keys, rank-normalised draws, the chains' moments, ρ
    double* d_diag = nullptr; int64_t cap_diag = 0;
    // the slice sampler (octo_draws_slice.hip), grown on demand: the chains' state machines in one allocation with the transition it was opened
    // for (slice_passes = 0: nothing to resume)
    double* d_slice = nullptr; int64_t cap_slice = 0;
    int64_t slice_W = 0, slice_ld = 0; int32_t slice_passes = 0, slice_p = 0, slice_shrink = 0;
    uint64_t slice_seed = 0, slice_step = 0, slice_chain0 = 0;
    // the expression program (octo_draws_program.hip) of a handle without a model: the dataset it evaluates, its tables on the device in one
    // allocation (prog_ops null: no program), its shape, and its work arrays, grown on demand
    const octo_dataset* prog_ds = nullptr;
    void* d_prog_tab = nullptr;
    const octo_draws_op* prog_ops = nullptr; const octo_draws_bind* prog_binds = nullptr; const int32_t* prog_terms = nullptr;
    int32_t prog_n_ops = 0, prog_n_in = 0, prog_n_el = 0, prog_n_terms = 0, prog_planets = 0;
    double prog_k_yr = 0.0;
    double* d_prog = nullptr; int64_t cap_prog = 0;
    // nested sampling (octo_draws_nested.hip), grown on demand: the order of a cull, and the state machines of a move in one allocation with the
    // transition it was opened for (nest_passes = 0: nothing to resume)
    double* d_ncull = nullptr; int64_t cap_ncull = 0;
    double* d_nest = nullptr; int64_t cap_nest = 0;
    int64_t nest_B = 0, nest_ld = 0, nest_ldK = 0; int32_t nest_K = 0, nest_passes = 0, nest_steps = 0, nest_shrink = 0;
    uint64_t nest_seed = 0, nest_iter = 0;
    // the dense metric (octo_draws_dense.hip): the CALLER's packed factor L [D(D+1)/2] that the HMC step and NUTS read while it is set
    // (octo_draws_use_metric; null: the per-call diagonal metric), and the one the open NUTS transition was started with
    const double* d_metric = nullptr;
    const double* nuts_metric = nullptr;
    // differential evolution (octo_draws_de.hip), grown on demand: the population, its trial points and their copies in one allocation with the
    // search it was opened for (de_open = false: nothing to resume), the generation its trial points are built for and which copies are current
    double* d_de = nullptr; int64_t cap_de = 0;
    int64_t de_W = 0, de_ld = 0; int32_t de_radius = 0, de_flip = 0;
    uint64_t de_seed = 0, de_gen = 0;
    bool de_open = false, de_bounds = false;
    // the OFTI rejection sampler (octo_draws_ofti.hip) while octo_draws_ofti_set holds (ofti null: not set): the main library's handle on the table,
    // the table's rows for k_oftis_post with the scalars octo_ofti_create forms beside them, how the third coordinate is read, and the driver's work
    // group, grown on demand
    octo_ofti* ofti = nullptr;
    double* d_oftis_rows = nullptr; int64_t cap_oftis_rows = 0;
    int32_t oftis_n_rows = 0, oftis_tp_mode = 0;
    double oftis_t_ref = 0.0, oftis_k_yr = 0.0, oftis_lambda = 0.0, oftis_data_quad = 0.0, oftis_log_det_data_cov = 0.0, oftis_log_det_prior_inv = 0.0,
           oftis_n_log2pi = 0.0;
    double* d_oftis = nullptr; int64_t cap_oftis = 0;
    // along-scan absolute astrometry (octo_draws_scan.hip) while octo_draws_scan_set holds (scan_n = 0: not set): the table's rows on the device, its
    // shape, the planets' descriptors and the constants of the orbit constructor, the work array (grown on demand), the device side of the host-buffer
    // twin, and the binding to the expression program (scan_bound = 0: none; otherwise 1 + mode): the program's bindings with the bound nodes appended
    double* d_scan_rows = nullptr; int64_t cap_scan_rows = 0;
    int32_t scan_n = 0, scan_K = 0, scan_P = 0;
    int32_t scan_kind[OCTO_MAX_PLANETS] = {}, scan_mass[OCTO_MAX_PLANETS] = {};
    octo_consts scan_consts = {};
    double* d_scan = nullptr; int64_t cap_scan = 0;
    double* d_scan_hst = nullptr; int64_t cap_scan_hst = 0;
    int32_t scan_bound = 0, scan_n_bind = 0;
    double* d_scan_binds = nullptr; int64_t cap_scan_binds = 0;
    // the catalogue proper-motion anomaly (octo_draws_pma.hip) while octo_draws_pma_set holds (pma_n = 0: not set): the rows {t, u, v, 0, L[0 … 7]} on the
    // device, the shape, the host-made matrices of both modes, the planets' descriptors and constants, the work array, the device side of the host-buffer
    // twin, and the binding to the expression program as for the scan table (pma_bound = 0: none; otherwise 1 + mode). One bound table a handle.
    double* d_pma_rows = nullptr; int64_t cap_pma_rows = 0;
    int32_t pma_n = 0, pma_Q = 0, pma_K = 0, pma_P = 0;
    PmaTable pma_tab = {};
    int32_t pma_kind[OCTO_MAX_PLANETS] = {}, pma_mass[OCTO_MAX_PLANETS] = {};
    octo_consts pma_consts = {};
    double* d_pma = nullptr; int64_t cap_pma = 0;
    double* d_pma_hst = nullptr; int64_t cap_pma_hst = 0;
    int32_t pma_bound = 0, pma_n_bind = 0;
    double* d_pma_binds = nullptr; int64_t cap_pma_binds = 0;
    // the Gaussian-process RV term (octo_draws_gp.hip) while octo_draws_gp_set holds (gp_n = 0: not set): the rows {t, rv, σ², c[0 … 3], 0} on the device,
    // the shape (J terms of R slots and H hyperparameters; RP = the instantiation's slots), the terms' kinds and every slot's role, the planets'
    // descriptors and constants, the work array, the device side of the host-buffer twin, and the binding to the expression program as for the scan table.
    double* d_gp_rows = nullptr; int64_t cap_gp_rows = 0;
    int32_t gp_n = 0, gp_K = 0, gp_P = 0, gp_J = 0, gp_R = 0, gp_RP = 0, gp_H = 0;
    int32_t gp_dense = 0;      // the terms are dense kinds (octo_draws_gpd.hip: a workgroup a walker); R = RP = 0 and gp_slot is not read
    int32_t gp_term[OCTO_DRAWS_GP_MAX_TERMS] = {}, gp_slot[OCTO_DRAWS_GP_MAX_SLOTS] = {};
    int32_t gp_kind[OCTO_MAX_PLANETS] = {}, gp_mass[OCTO_MAX_PLANETS] = {};
    octo_consts gp_consts = {};
    double* d_gp = nullptr; int64_t cap_gp = 0;
    double* d_gp_hst = nullptr; int64_t cap_gp_hst = 0;
    int32_t gp_bound = 0, gp_n_bind = 0;
    double* d_gp_binds = nullptr; int64_t cap_gp_binds = 0;
};

// What octo_draws_ofti.hip takes from octo_draws.hip (defined there, not exported): k_draw's launches into θ alone, and the two halves of pass 2 of the
// rejection on ℓ [N] with its block maxima, the code octo_draws_rejection itself runs — draws_max_pass: k_max, the maximum on the host, the refusal when
// every ℓ is −Inf; draws_accept_pass: k_count, k_scan, k_scatter and the full count.
#define OCTO_DRAWS_INTERNAL __attribute__((visibility("hidden")))
OCTO_DRAWS_INTERNAL int draws_launch_draw(octo_draws* h, hipStream_t st, uint64_t seed, uint64_t first, const uint64_t* d_idx, int64_t n, int64_t ld, double* d_theta);
OCTO_DRAWS_INTERNAL int draws_max_pass(octo_draws* h, hipStream_t st, const double* pmax, int64_t N, double* d_max, double* mx_out);
OCTO_DRAWS_INTERNAL int draws_accept_pass(octo_draws* h, hipStream_t st, const double* ll, const double* lp, int64_t N, const double* d_max, uint64_t seed,
                                          uint64_t first, int64_t* cnt, int64_t room, uint64_t* o_ix, double* o_ll, double* o_lp, int64_t* total_out);

// What octo_draws_program.hip takes from octo_draws_scan.hip (defined there, not exported): ℓ_scan of the bound table added into ll [W] and its element
// adjoints into g_in (null: no gradient), the bound rows' adjoints stored behind the program's n_in rows; inputs and g_in are [rows][ldw].
OCTO_DRAWS_INTERNAL int draws_scan_accumulate(octo_draws* h, hipStream_t st, const double* inputs, double* g_in, double* ll, int64_t ldw, int64_t W, int32_t n_in);
// … and from octo_draws_pma.hip, the same for the bound catalogue table: ℓ_pma into ll, the element adjoints into g_in, ∂ℓ/∂γ stored behind the n_in rows
OCTO_DRAWS_INTERNAL int draws_pma_accumulate(octo_draws* h, hipStream_t st, const double* inputs, double* g_in, double* ll, int64_t ldw, int64_t W, int32_t n_in);
// … and from octo_draws_gp.hip for the bound Gaussian-process table: ℓ_gp into ll, the element adjoints into g_in, ∂ℓ/∂(hyper, β, s) stored behind the n_in rows
OCTO_DRAWS_INTERNAL int draws_gp_accumulate(octo_draws* h, hipStream_t st, const double* inputs, double* g_in, double* ll, int64_t ldw, int64_t W, int32_t n_in);

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
// ℓπ of the handle: its model's, or its expression program's
inline bool has_target(const octo_draws* h) { return h->ctx && (h->model || h->prog_ops); }
inline int check_model(octo_draws* h, const char* who) {
    return has_target(h) ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no model (created without one, or detached)");
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
// the checks of the two samplers, in their order: the chains, ε, and no ℓπ outputs from a handle without a model
inline int check_sampler_call(octo_draws* h, const char* who, int64_t W, int64_t ld, const double* d_eps, double eps, bool has_model, const double* d_logpost,
                              const double* d_loglike) {
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    if (!d_eps && !(eps > 0.0 && std::isfinite(eps))) return fail(h, OCTO_EINVAL, std::string(who) + ": eps must be finite and > 0 when d_eps is NULL");
    return has_model || !(d_logpost || d_loglike) ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no model (created without one, or detached): d_logpost and d_loglike must be NULL");
}

inline SamplerHead sampler_head(const octo_draws* h, bool has_model, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t,
                                const double* d_beta, const double* d_eps, double eps, const double* d_inv_mass) {
    return {h->d_priors, h->d_pc, d_beta, d_eps, d_inv_mass, eps, seed, step, chain0, W, ld, h->D, has_model ? 1 : 0, d_theta_t};
}

// ℓπ [W] and ∇ℓπ [D][ld] (or null) at the points `at` [D][ld] on the stream st; nothing to do on a handle without a model. The one place that
// chooses between the model and the expression program.
inline int logpost_at(octo_draws* h, hipStream_t st, bool has_model, const double* at, int64_t ld, int64_t W, double* lp, double* glp) {
    if (has_model && h->prog_ops) return octo_draws_program_logpost_device(h, at, ld, W, lp, glp, (void*)st);
    return has_model ? main_call(h, octo_model_logpost_device(h->ctx, h->model, at, ld, W, lp, glp, (void*)st), "octo_model_logpost_device") : OCTO_OK;
}

// The round driver of the L-BFGS and of NUTS. Args holds W, ld, write_out and its state s with the trial points s.trial; lp and glp are where
// ℓπ and ∇ℓπ go (a.s.lp and a.s.glp may be nulled for the kernels). Not resumed: ℓπ at θ_t and `open`, which writes the outputs when no
// round follows; n_rounds times ℓπ at the trial points and `round`, the last writing the outputs; resumed with no round: `report`.
template <class Args>
int run_rounds(octo_draws* h, hipStream_t st, Args& a, bool has_model, const double* d_theta_t, double* lp, double* glp, int32_t n_rounds, bool resume,
               void (*open)(Args), void (*round)(Args), void (*report)(Args)) {
    const dim3 grid = grid_of(a.W), block(TPB);
    if (!resume) {
        if (int rc = logpost_at(h, st, has_model, d_theta_t, a.ld, a.W, lp, glp)) return rc;
        a.write_out = n_rounds == 0;
        hipLaunchKernelGGL(open, grid, block, 0, st, a);
    }
    for (int r = 1; r <= n_rounds; ++r) {
        if (int rc = logpost_at(h, st, has_model, a.s.trial, a.ld, a.W, lp, glp)) return rc;
        a.write_out = r == n_rounds;
        hipLaunchKernelGGL(round, grid, block, 0, st, a);
    }
    if (resume && n_rounds == 0) {
        a.write_out = 1;
        hipLaunchKernelGGL(report, grid, block, 0, st, a);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // namespace
