// octo_draws_hmc.hip — the tempered HMC explorer of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the algorithm):
// momentum draws, the tempered leapfrog and the Metropolis decision of every chain on the device, around octo_model_logpost_device.
// Lane = chain, SoA with the chain index fastest (every load and store coalesced); β, ε and the decision are per lane, the coordinate
// index is wave-uniform, so the prior's kind never diverges inside a wave.
//
//   k_hmc_momentum  one launch = one Philox block of four coordinates (as k_draw, and for its reason: normcdfinv stays out of every loop).
//   k_hmc_leap<OPEN>   the start point: prior value and derivative, E₀, K₀, the half kick and the drift.
//   k_hmc_leap<STEP>   a point inside the trajectory: prior value and derivative at it, the whole kick and the drift.
//   k_hmc_leap<LAST>   the end point: the half kick, H₁, the decision, the selection and every output.
//   k_dense_hmc_leap<·>  the same three bodies with the handle's dense metric (octo_draws_use_metric): whitened momenta, two triangular products.
// A step is ⌈D/4⌉ + 1 + n_leapfrog launches besides the n_leapfrog + 1 log-posterior calls; the host reads nothing.
// From octo_draws_common.h: the head of HmcArgs and its filling, the lane's chain (chain_of), the target at a point (target_at), the metric
// (inv_mass_at, momentum_of), the shared argument checks (check_sampler_call) and the log-posterior call (logpost_at).
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
        a.p[(int64_t)d * a.ld + t] = momentum_of(a.inv_mass, d, normcdfinv(u01(r[q])));
    }
}

// theta_t is read by OPEN and written by LAST where a chain accepts. Of s: q the moving point and p its momentum; glp and lp, ∇ℓπ and ℓπ at the
// point of this launch (null without a model); gpr, ∇ℓprior_t at it, between the two loops of a launch; lp0, lpt0, K0 of the start point, from
// OPEN to LAST.
struct HmcArgs : SamplerHead {
    HmcWork s;
    double *theta_prop, *o_lp, *o_ll, *o_dH;
    int32_t* o_acc;
    const double* chol;            // the handle's dense factor L, packed; read by k_dense_hmc_leap alone
};

// Two loops over the coordinates. The first is target_at's prior_loop() (octo_draws_common.h, shared with the no-U-turn sampler): every
// transcendental, and ∇ℓprior_t left in a.s.gpr. The second is arithmetic alone. DENSE: the handle's factor L is set and p holds the whitened
// momenta r = Lᵀp ~ N(0, I) (a.inv_mass is null: K = ½Σr²); the kick takes Lᵀ∇E (metric_gradient) and the drift L·r, after the loop that made r½.
template <int PHASE, bool DENSE>
__device__ __forceinline__ void hmc_leap(const HmcArgs& a) {
    const Chain ch = chain_of(a);
    const int64_t w = ch.w, wl = ch.wl;
    const bool live = ch.live;
    const double beta = ch.beta, eps = ch.eps;
    const double* __restrict__ at = PHASE == HMC_OPEN ? a.theta_t : a.s.q;
    const Target tg = target_at(a, ch, at, a.s.lp, a.s.glp, a.s.gpr);
    if (DENSE && !live) return;      // the products write the lane's own column
    const double lp = tg.lp(wl), lpt = tg.lpt;
    const double kick = PHASE == HMC_STEP ? eps : 0.5 * eps;
    double K = 0.0;
    metric_gradient<DENSE>(tg, a.chol, a.s.gpr, a.D, a.ld, wl, [&](int d, int64_t o, double g) {
        const double im = inv_mass_at(a.inv_mass, d);
        double pd = a.s.p[o];
        if (PHASE == HMC_OPEN) K += im * pd * pd;
        pd += kick * g;
        if (PHASE == HMC_LAST) K += im * pd * pd;
        else if (live) {
            a.s.p[o] = pd;
            if (!DENSE) a.s.q[o] = at[o] + eps * (im * pd);
        }
    });
    if (DENSE && PHASE != HMC_LAST)
        metric_lower(a.chol, a.D, a.s.p, a.ld, w, [&](int d, double v) { const int64_t o = (int64_t)d * a.ld + w; a.s.q[o] = at[o] + eps * v; });
    K *= 0.5;
    if (PHASE == HMC_OPEN && live) { a.s.lp0[w] = lp; a.s.lpt0[w] = lpt; a.s.K0[w] = K; }
    if (PHASE != HMC_LAST) return;
    const double lp0 = a.s.lp0[wl], lpt0 = a.s.lpt0[wl];
    const double E0 = tempered_energy(beta, lp0, lpt0), E1 = tempered_energy(beta, lp, lpt);
    const bool dead0 = dead_state(beta, E0, lp0, lpt0), dead1 = dead_state(beta, E1, lp, lpt);
    const double dH = (-E0 + a.s.K0[wl]) - (-E1 + K);
    uint64_t r[4];
    philox4x64(a.seed, KEY1, a.chain0 + (uint64_t)wl, 0, OCTO_DRAWS_PURPOSE_ACCEPT, a.step, r);
    const bool acc = !dead1 && (dead0 || log(u01(r[0])) < dH);
    if (!live) return;
    if (acc || a.theta_prop)
        for (int d = 0; d < a.D; ++d) {
            const int64_t o = (int64_t)d * a.ld + w;
            const double y = a.s.q[o];
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

template <int PHASE>
__global__ __launch_bounds__(TPB) void k_hmc_leap(HmcArgs a) { hmc_leap<PHASE, false>(a); }
template <int PHASE>
__global__ __launch_bounds__(TPB) void k_dense_hmc_leap(HmcArgs a) { hmc_leap<PHASE, true>(a); }

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
    const bool has_model = has_target(h);
    if (int rc = check_sampler_call(h, "octo_draws_hmc_step_device", W, ld, d_eps, eps, has_model, d_logpost, d_loglike)) return rc;
    if (W == 0) return OCTO_OK;
    if (!d_theta_t || !d_accepted) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step_device: d_theta_t and d_accepted are required");
    const bool dense = h->d_metric != nullptr;
    if (dense && d_inv_mass) return fail(h, OCTO_EINVAL, "octo_draws_hmc_step_device: d_inv_mass must be NULL while a dense metric is set (octo_draws_use_metric)");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    HmcArgs a{sampler_head(h, has_model, seed, step, chain0, W, ld, d_theta_t, d_beta, d_eps, eps, d_inv_mass)};
    if (int rc = grow_to(h, h->d_hmc, h->cap_hmc, a.s, hmc_work, (int64_t)h->D, ld)) return rc;
    double *lp = a.s.lp, *glp = a.s.glp;
    if (!has_model) { a.s.lp = nullptr; a.s.glp = nullptr; }
    a.theta_prop = d_theta_prop; a.o_lp = d_logpost; a.o_ll = d_loglike; a.o_dH = d_dH; a.o_acc = d_accepted; a.chol = h->d_metric;
    const dim3 grid = grid_of(W), block(TPB);
    launch_momentum(st, seed, step, chain0, W, ld, h->D, d_inv_mass, a.s.p);
    OCHK(h, hipGetLastError());
    if (int rc = logpost_at(h, st, has_model, d_theta_t, ld, W, lp, glp)) return rc;
    hipLaunchKernelGGL(dense ? k_dense_hmc_leap<HMC_OPEN> : k_hmc_leap<HMC_OPEN>, grid, block, 0, st, a);
    for (int s = 1; s <= n_leapfrog; ++s) {
        if (int rc = logpost_at(h, st, has_model, a.s.q, ld, W, lp, glp)) return rc;
        if (s < n_leapfrog) hipLaunchKernelGGL(dense ? k_dense_hmc_leap<HMC_STEP> : k_hmc_leap<HMC_STEP>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(dense ? k_dense_hmc_leap<HMC_LAST> : k_hmc_leap<HMC_LAST>, grid, block, 0, st, a);
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
