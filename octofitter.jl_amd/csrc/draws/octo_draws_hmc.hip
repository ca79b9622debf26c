// octo_draws_hmc.hip — the tempered HMC explorer of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the algorithm):
// momentum draws, the tempered leapfrog and the Metropolis decision of every chain on the device, around octo_model_logpost_device.
// Lane = chain, SoA with the chain index fastest (every load and store coalesced); β, ε and the decision are per lane, the coordinate
// index is wave-uniform, so the prior's kind never diverges inside a wave.
//
//   k_hmc_momentum  one launch = one Philox block of four coordinates (as k_draw, and for its reason: normcdfinv stays out of every loop).
//   k_hmc_leap<OPEN>   the start point: prior value and derivative, E₀, K₀, the half kick and the drift.
//   k_hmc_leap<STEP>   a point inside the trajectory: prior value and derivative at it, the whole kick and the drift.
//   k_hmc_leap<LAST>   the end point: the half kick, H₁, the decision, the selection and every output.
// A step is ⌈D/4⌉ + 1 + n_leapfrog launches besides the n_leapfrog + 1 log-posterior calls; the host reads nothing.
#include "octo_draws_common.h"

namespace {

enum { HMC_OPEN = 0, HMC_STEP = 1, HMC_LAST = 2 };

struct MomentumArgs {
    const double* inv_mass;        // [D] or null = 1
    uint64_t seed, step, chain0;
    int64_t n, ld;
    int32_t D, d0;                 // this launch: coordinates d0 … d0 + 3 (d0 a multiple of 4)
    double* p;                     // [D][ld]
};

__global__ __launch_bounds__(TPB) void k_hmc_momentum(MomentumArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= a.n) return;
    uint64_t r[4];
    philox4x64(a.seed, KEY1, a.chain0 + (uint64_t)t, (uint64_t)(a.d0 >> 2), OCTO_DRAWS_PURPOSE_MOMENTUM, a.step, r);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = a.d0 + q;
        if (d >= a.D) break;
        const double z = normcdfinv(u01(r[q]));
        a.p[(int64_t)d * a.ld + t] = a.inv_mass ? z / sqrt(a.inv_mass[d]) : z;
    }
}

struct HmcArgs {
    const octo_prior* priors;      // [D]
    const double* pc;              // [D][PRIOR_NC]
    const double* beta;            // [W] or null = 1 (ignored without a model: 0)
    const double* eps_w;           // [W] or null = eps
    const double* inv_mass;        // [D] or null = 1
    double eps;
    uint64_t seed, step, chain0;
    int64_t W, ld;
    int32_t D, has_model;
    double* theta_t;               // [D][ld] the caller's states: read by OPEN, written by LAST where a chain accepts
    double* q;                     // [D][ld] the moving point
    double* p;                     // [D][ld] its momentum
    const double* glp;             // [D][ld] ∇ℓπ at the point of this launch (null without a model)
    double* gpr;                   // [D][ld] ∇ℓprior_t at it, between the two loops of a launch
    const double* lp;              // [W] ℓπ at it (null without a model)
    double *lp0, *lpt0, *K0;       // [W] of the start point, from OPEN to LAST
    double *theta_prop, *o_lp, *o_ll, *o_dH;
    int32_t* o_acc;
};

// Two loops over the coordinates. The first is prior_loop (octo_draws_common.h, shared with the no-U-turn sampler): every transcendental, and
// ∇ℓprior_t left in a.gpr. The second is arithmetic alone.
template <int PHASE>
__global__ __launch_bounds__(TPB) void k_hmc_leap(HmcArgs a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const bool live = w < a.W;                          // no early exit: prior_density_lanes votes across the wave
    const int64_t wl = live ? w : a.W - 1;
    const double beta = a.has_model ? (a.beta ? a.beta[wl] : 1.0) : 0.0;
    const double eps = a.eps_w ? a.eps_w[wl] : a.eps;
    const double* __restrict__ at = PHASE == HMC_OPEN ? a.theta_t : a.q;
    bool healed;
    const double lpt = prior_loop(a.priors, a.pc, a.D, at, a.ld, w, wl, live, a.gpr, healed);
    const double lp = a.has_model ? a.lp[wl] : 0.0;      // E and ∇E consult it only where β != 0; the outputs report it for every chain
    const double kick = PHASE == HMC_STEP ? eps : 0.5 * eps;
    double K = 0.0;
    for (int d = 0; d < a.D; ++d) {
        const int64_t o = (int64_t)d * a.ld + wl;
        const double im = a.inv_mass ? a.inv_mass[d] : 1.0;
        const double gp = healed ? 0.0 : a.gpr[o];
        const double g = tempered_gradient(beta, a.glp, o, gp);
        double pd = a.p[o];
        if (PHASE == HMC_OPEN) K += im * pd * pd;
        pd += kick * g;
        if (PHASE == HMC_LAST) K += im * pd * pd;
        else if (live) {
            a.p[o] = pd;
            a.q[o] = at[o] + eps * (im * pd);
        }
    }
    K *= 0.5;
    if (PHASE == HMC_OPEN && live) { a.lp0[w] = lp; a.lpt0[w] = lpt; a.K0[w] = K; }
    if (PHASE != HMC_LAST) return;
    const double lp0 = a.lp0[wl], lpt0 = a.lpt0[wl];
    const double E0 = tempered_energy(beta, lp0, lpt0), E1 = tempered_energy(beta, lp, lpt);
    const bool dead0 = dead_state(beta, E0, lp0, lpt0), dead1 = dead_state(beta, E1, lp, lpt);
    const double dH = (-E0 + a.K0[wl]) - (-E1 + K);
    uint64_t r[4];
    philox4x64(a.seed, KEY1, a.chain0 + (uint64_t)wl, 0, OCTO_DRAWS_PURPOSE_ACCEPT, a.step, r);
    const bool acc = !dead1 && (dead0 || log(u01(r[0])) < dH);
    if (!live) return;
    if (acc || a.theta_prop)
        for (int d = 0; d < a.D; ++d) {
            const int64_t o = (int64_t)d * a.ld + w;
            const double y = a.q[o];
            if (a.theta_prop) a.theta_prop[o] = y;
            if (acc) a.theta_t[o] = y;
        }
    if (a.o_lp) a.o_lp[w] = acc ? lp : lp0;
    if (a.o_ll) {
        const double ll = acc ? lp - lpt : lp0 - lpt0;
        a.o_ll[w] = isfinite(ll) ? ll : -INFINITY;
    }
    if (a.o_dH) a.o_dH[w] = dH;
    a.o_acc[w] = acc ? 1 : 0;
}

void launch_momentum(hipStream_t st, uint64_t seed, uint64_t step, uint64_t chain0, int64_t n, int64_t ld, int32_t D, const double* d_inv_mass, double* d_p) {
    MomentumArgs m;
    m.inv_mass = d_inv_mass; m.seed = seed; m.step = step; m.chain0 = chain0; m.n = n; m.ld = ld; m.D = D; m.p = d_p;
    for (m.d0 = 0; m.d0 < D; m.d0 += 4) hipLaunchKernelGGL(k_hmc_momentum, grid_of(n), dim3(TPB), 0, st, m);
}

}  // namespace

extern "C" {

int32_t octo_draws_momentum_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t n, int64_t ld, const double* d_inv_mass,
                                   double* d_p, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (n < 0 || ld < n || n > MAX_CHAINS) return fail(h, OCTO_EINVAL, "octo_draws_momentum_device: need 0 <= n <= ld, n <= 2^30");
    if (n == 0) return OCTO_OK;
    if (!d_p) return fail(h, OCTO_EINVAL, "octo_draws_momentum_device: null output");
    OCHK(h, hipSetDevice(h->device));
    launch_momentum(stream_of(h, hip_stream), seed, step, chain0, n, ld, h->D, d_inv_mass, d_p);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_hmc_step_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t,
                                   const double* d_beta, const double* d_eps, double eps, int32_t n_leapfrog, const double* d_inv_mass,
                                   double* d_theta_prop, double* d_logpost, double* d_loglike, double* d_dH, int32_t* d_accepted, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (n_leapfrog < 1) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step_device: n_leapfrog >= 1");
    if (int rc = check_chains(h, "octo_draws_hmc_step_device", W, ld, MAX_CHAINS, "2^30")) return rc;
    if (!d_eps && !(eps > 0.0 && std::isfinite(eps))) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step_device: eps must be finite and > 0 when d_eps is NULL");
    const bool has_model = h->model && h->ctx;
    if (!has_model && (d_logpost || d_loglike))
        return fail(h, OCTO_EINVAL, "octo_draws_hmc_step_device: the handle has no model (created without one, or detached): d_logpost and d_loglike must be NULL");
    if (W == 0) return OCTO_OK;
    if (!d_theta_t || !d_accepted) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step_device: d_theta_t and d_accepted are required");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    HmcWork w;
    if (int rc = grow_to(h, h->d_hmc, h->cap_hmc, w, hmc_work, (int64_t)h->D, ld)) return rc;
    HmcArgs a;
    std::memset(&a, 0, sizeof(a));
    a.priors = h->d_priors; a.pc = h->d_pc; a.beta = d_beta; a.eps_w = d_eps; a.inv_mass = d_inv_mass; a.eps = eps;
    a.seed = seed; a.step = step; a.chain0 = chain0; a.W = W; a.ld = ld; a.D = h->D; a.has_model = has_model ? 1 : 0;
    a.theta_t = d_theta_t;
    a.q = w.q; a.p = w.p; a.gpr = w.gpr; a.lp0 = w.lp0; a.lpt0 = w.lpt0; a.K0 = w.K0;
    if (has_model) { a.glp = w.glp; a.lp = w.lp; }
    a.theta_prop = d_theta_prop; a.o_lp = d_logpost; a.o_ll = d_loglike; a.o_dH = d_dH; a.o_acc = d_accepted;
    const dim3 grid = grid_of(W), block(TPB);
    launch_momentum(st, seed, step, chain0, W, ld, h->D, d_inv_mass, a.p);
    OCHK(h, hipGetLastError());
    if (has_model) { int rc = main_call(h, octo_model_logpost_device(h->ctx, h->model, d_theta_t, ld, W, w.lp, w.glp, (void*)st), "octo_model_logpost_device"); if (rc) return rc; }
    hipLaunchKernelGGL(k_hmc_leap<HMC_OPEN>, grid, block, 0, st, a);
    for (int s = 1; s <= n_leapfrog; ++s) {
        if (has_model) { int rc = main_call(h, octo_model_logpost_device(h->ctx, h->model, a.q, ld, W, w.lp, w.glp, (void*)st), "octo_model_logpost_device"); if (rc) return rc; }
        if (s < n_leapfrog) hipLaunchKernelGGL(k_hmc_leap<HMC_STEP>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_hmc_leap<HMC_LAST>, grid, block, 0, st, a);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_hmc_step(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld, double* theta_t, const double* beta,
                            const double* eps_w, double eps, int32_t n_leapfrog, const double* inv_mass, double* theta_prop, double* logpost,
                            double* loglike, double* dH, int32_t* accepted) {
    if (!h) return OCTO_EINVAL;
    if (n_leapfrog < 1) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step: n_leapfrog >= 1");
    if (W < 0 || ld < W) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step: need 0 <= W <= ld");
    if (W == 0) return OCTO_OK;
    if (!theta_t || !accepted) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step: theta_t and accepted are required");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    const int64_t D = h->D, plane = D * ld;
    HmcStaging d;
    if (int rc = grow_to(h, h->d_hst, h->cap_hst, d, hmc_staging, D, ld)) return rc;
    OCHK(h, hipMemcpyAsync(d.theta_t, theta_t, sizeof(double) * plane, hipMemcpyHostToDevice, st));
    if (beta) OCHK(h, hipMemcpyAsync(d.beta, beta, sizeof(double) * W, hipMemcpyHostToDevice, st));
    if (eps_w) OCHK(h, hipMemcpyAsync(d.eps, eps_w, sizeof(double) * W, hipMemcpyHostToDevice, st));
    if (inv_mass) OCHK(h, hipMemcpyAsync(d.inv_mass, inv_mass, sizeof(double) * D, hipMemcpyHostToDevice, st));
    {
        int rc = octo_draws_hmc_step_device(h, seed, step, chain0, W, ld, d.theta_t, beta ? d.beta : nullptr, eps_w ? d.eps : nullptr, eps, n_leapfrog,
                                            inv_mass ? d.inv_mass : nullptr, theta_prop ? d.theta_prop : nullptr, logpost ? d.lp : nullptr, loglike ? d.ll : nullptr,
                                            dH ? d.dH : nullptr, d.accepted, OCTO_STREAM_CTX);
        if (rc) return rc;
    }
    OCHK(h, hipMemcpyAsync(theta_t, d.theta_t, sizeof(double) * plane, hipMemcpyDeviceToHost, st));
    if (theta_prop) OCHK(h, hipMemcpyAsync(theta_prop, d.theta_prop, sizeof(double) * plane, hipMemcpyDeviceToHost, st));
    if (logpost) OCHK(h, hipMemcpyAsync(logpost, d.lp, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    if (loglike) OCHK(h, hipMemcpyAsync(loglike, d.ll, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    if (dH) OCHK(h, hipMemcpyAsync(dH, d.dH, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpyAsync(accepted, d.accepted, sizeof(int32_t) * W, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

}  // extern "C"
