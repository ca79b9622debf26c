// octo_draws_nuts.hip — the no-U-turn sampler of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the transition): W chains
// build their trees in lockstep, a round being one octo_model_logpost_device call at the trial points of all chains and one k_nuts_leaf
// launch — one leapfrog per chain per round. Lane = chain, SoA with the chain index fastest (every load and store coalesced); the coordinate
// index is a wave-uniform loop variable; the direction, the leaf number, the checkpoint slot and every decision are per lane. Nothing of a
// chain lives in a private array: the endpoints, the proposals, the checkpoint stacks and every scalar of the tree sit in the handle's work
// array (nuts_work of octo_draws_layout.h), and a lane reaches its endpoint and its checkpoint slot through addresses it computes.
//
//   k_nuts_open    the start point: prior value and derivative, E₀, K₀, H₀, the dead test, the tree of one point, the first trial point.
//   k_nuts_leaf    a leaf: prior value and derivative at the trial point, the closing half kick, Δ, the subtree's weight, proposal and ρ_s,
//                  the checkpoint store or the turn tests, the merge and the tree's test where the subtree completes, the write-back where
//                  the chain ends, and the opening half kick and drift of the next leaf.
//   k_nuts_report  the outputs alone: a resumed call of no rounds.
//   k_dense_nuts_open, k_dense_nuts_leaf   the same two bodies with the handle's dense metric (octo_draws_use_metric): whitened momenta and
//                  gradients in every array of the tree, Lᵀ∇E after the gradient arrives and L·r½ before the drift.
// The last launch of a call writes the outputs. The momenta are octo_draws_momentum_device's (purpose 2), the HMC step's.
// From octo_draws_common.h, as the HMC step: the head of NutsArgs, chain_of, target_at, inv_mass_at, check_sampler_call; and run_rounds, the
// round driver it shares with the L-BFGS (opening, rounds, report; the last launch writes the outputs).
#include "octo_draws_common.h"

namespace {

enum { NUTS_BUILDING = 0, NUTS_MAX_DEPTH = 1, NUTS_TURN_SUBTREE = 2, NUTS_TURN_TREE = 3, NUTS_DIVERGED = 4, NUTS_DEAD = 5 };
constexpr double NUTS_DELTA_MAX = 1000.0;

// theta_t is read by k_nuts_open and written where a chain ends on a leaf of its tree
struct NutsArgs : SamplerHead {
    int32_t max_depth, write_out;
    NutsWork s;
    double *o_lp, *o_ll, *o_la;
    int32_t *o_acc, *o_depth, *o_nleaf, *o_div, *o_nact;
    const double* chol;            // the handle's dense factor L, packed; read by k_dense_nuts_open and k_dense_nuts_leaf alone
};

__device__ __forceinline__ double log_add_exp(double x, double y) {
    const double m = fmax(x, y);
    return m == -INFINITY ? m : m + log1p(exp(-fabs(x - y)));
}

// log u, u the uniform of word 0 of the counter (c, word1, purpose, step)
__device__ __forceinline__ double nuts_uniform(const NutsArgs& a, int64_t w, uint64_t word1, uint64_t purpose) {
    uint64_t r[4];
    philox4x64(a.seed, KEY1, a.chain0 + (uint64_t)w, word1, purpose, a.step, r);
    return u01(r[0]);
}

// the opening half kick and the drift of the next leaf, from the endpoint on the side v: p½ and q′ into pt and trial. DENSE: the endpoints hold
// whitened momenta and gradients, so the kick is the same line, and the drift takes L·r½ once pt holds all of r½
template <bool DENSE>
__device__ __forceinline__ void next_leaf(const NutsArgs& a, int64_t w, int32_t v, double eps) {
    const double *qe = v > 0 ? a.s.qR : a.s.qL, *pe = v > 0 ? a.s.pR : a.s.pL, *ge = v > 0 ? a.s.gR : a.s.gL;
    const double hk = (double)v * (0.5 * eps), dr = (double)v * eps;
    for (int d = 0; d < a.D; ++d) {
        const int64_t o = (int64_t)d * a.ld + w;
        const double ph = pe[o] + hk * ge[o];
        a.s.pt[o] = ph;
        if (!DENSE) a.s.trial[o] = qe[o] + dr * (inv_mass_at(a.inv_mass, d) * ph);
    }
    if (DENSE) metric_lower(a.chol, a.D, a.s.pt, a.ld, w, [&](int d, double u) { const int64_t o = (int64_t)d * a.ld + w; a.s.trial[o] = qe[o] + dr * u; });
}

// a chain that has ended: θ_t takes the proposal if it moved, and the trial point is θ_t from now on
__device__ __forceinline__ void finish(const NutsArgs& a, int64_t w, bool moved, double prop_lp, double prop_lpt) {
    for (int d = 0; d < a.D; ++d) {
        const int64_t o = (int64_t)d * a.ld + w;
        const double y = moved ? a.s.prop[o] : a.theta_t[o];
        if (moved) a.theta_t[o] = y;
        a.s.trial[o] = y;
    }
    if (moved) { a.s.out_lp[w] = prop_lp; a.s.out_lpt[w] = prop_lpt; }
}

__device__ __forceinline__ void report(const NutsArgs& a, int64_t w) {
    const int32_t status = a.s.status[w], nleaf = a.s.nleaf[w];
    if (a.o_lp) a.o_lp[w] = a.s.out_lp[w];
    if (a.o_ll) {
        const double ll = a.s.out_lp[w] - a.s.out_lpt[w];
        a.o_ll[w] = isfinite(ll) ? ll : -INFINITY;
    }
    if (a.o_la) a.o_la[w] = log(a.s.sum_acc[w] / (double)nleaf);
    a.o_acc[w] = status != NUTS_BUILDING && a.s.sel[w] != 0 ? 1 : 0;
    if (a.o_depth) a.o_depth[w] = a.s.depth[w];
    if (a.o_nleaf) a.o_nleaf[w] = nleaf;
    if (a.o_div) a.o_div[w] = status == NUTS_DIVERGED ? 1 : 0;
    if (a.o_nact && status == NUTS_BUILDING) atomicAdd(a.o_nact, 1);      // an integer count: order-free
}

// DENSE in the two bodies below: the handle's factor L is set, and every momentum of the tree — the endpoints, ρ, ρ_s, the checkpoints — is the
// whitened r = Lᵀp ~ N(0, I), every stored gradient Lᵀ∇E (metric_gradient). a.inv_mass is null, so K and the turn tests are the identity metric's.
template <bool DENSE>
__device__ __forceinline__ void nuts_open(const NutsArgs& a) {
    const Chain ch = chain_of(a);
    const Target tg = target_at(a, ch, a.theta_t, a.s.lp, a.s.glp, a.s.gpr);      // every lane: its prior_loop() votes across the wave
    if (!ch.live) return;
    const int64_t w = ch.w;
    const double beta = ch.beta, lp = tg.lp(w), lpt = tg.lpt;
    double K = 0.0;
    metric_gradient<DENSE>(tg, a.chol, a.s.gpr, a.D, a.ld, w, [&](int d, int64_t o, double g) {
        const double im = inv_mass_at(a.inv_mass, d);
        const double p = a.s.pL[o], q = a.theta_t[o];      // the momenta were drawn into pL
        K += im * p * p;
        a.s.qL[o] = q; a.s.qR[o] = q; a.s.pR[o] = p; a.s.gL[o] = g; a.s.gR[o] = g;
        a.s.prop[o] = q; a.s.rho[o] = p;
    });
    K *= 0.5;
    const double E0 = tempered_energy(beta, lp, lpt);
    const bool dead = dead_state(beta, E0, lp, lpt);
    a.s.H0[w] = -E0 + K; a.s.logw[w] = 0.0; a.s.logw_s[w] = 0.0; a.s.sum_acc[w] = 0.0;
    a.s.prop_lp[w] = lp; a.s.prop_lpt[w] = lpt; a.s.sprop_lp[w] = lp; a.s.sprop_lpt[w] = lpt; a.s.out_lp[w] = lp; a.s.out_lpt[w] = lpt;
    a.s.status[w] = dead ? NUTS_DEAD : NUTS_BUILDING;
    a.s.depth[w] = 0; a.s.n[w] = 0; a.s.nleaf[w] = 0; a.s.sel[w] = 0; a.s.ssel[w] = 0;
    const int32_t v = nuts_uniform(a, w, 0, OCTO_DRAWS_PURPOSE_NUTS_DIRECTION) < 0.5 ? 1 : -1;
    a.s.v[w] = v;
    if (dead) finish(a, w, false, lp, lpt);
    else next_leaf<DENSE>(a, w, v, ch.eps);
    if (a.write_out) report(a, w);
}

template <bool DENSE>
__device__ __forceinline__ void nuts_leaf(const NutsArgs& a) {
    const Chain ch = chain_of(a);
    const Target tg = target_at(a, ch, a.s.trial, a.s.lp, a.s.glp, a.s.gpr);      // every lane: its prior_loop() votes across the wave; a frozen chain: at its θ_t, ignored
    if (!ch.live) return;
    const int64_t w = ch.w;
    if (a.s.status[w] == NUTS_BUILDING) {
        const int64_t plane = (int64_t)a.D * a.ld;
        const double beta = ch.beta, eps = ch.eps, lp = tg.lp(w), lpt = tg.lpt;
        const int32_t v = a.s.v[w], n = a.s.n[w], nleaf = a.s.nleaf[w] + 1;
        int32_t j = a.s.depth[w];
        const bool first = n == 0, even = !(n & 1);
        const int32_t imax = __popc(n >> 1);
        // 2. the closing half kick; the leaf becomes the endpoint on its side, enters ρ_s and, at an even n, opens the checkpoint imax
        double *qe = v > 0 ? a.s.qR : a.s.qL, *pe = v > 0 ? a.s.pR : a.s.pL, *ge = v > 0 ? a.s.gR : a.s.gL;
        double *ckp = a.s.ck_p + imax * plane, *ckr = a.s.ck_r + imax * plane;
        const double hk = (double)v * (0.5 * eps);
        double K = 0.0;
        metric_gradient<DENSE>(tg, a.chol, a.s.gpr, a.D, a.ld, w, [&](int d, int64_t o, double g) {
            const double im = inv_mass_at(a.inv_mass, d);
            const double p = a.s.pt[o] + hk * g;
            K += im * p * p;
            const double rs = first ? p : a.s.rho_s[o] + p;
            qe[o] = a.s.trial[o]; pe[o] = p; ge[o] = g; a.s.rho_s[o] = rs;
            if (even) { ckp[o] = p; ckr[o] = rs; }
        });
        K *= 0.5;
        const double E1 = tempered_energy(beta, lp, lpt);
        const double delta = (-E1 + K) - a.s.H0[w];
        const bool div = dead_state(beta, E1, lp, lpt) || !(delta <= NUTS_DELTA_MAX);
        a.s.nleaf[w] = nleaf;
        a.s.sum_acc[w] += div ? 0.0 : fmin(1.0, exp(-delta));
        // 3. the subtree's weight and proposal
        const double lw = div ? -INFINITY : -delta;
        const double lws = first ? lw : log_add_exp(a.s.logw_s[w], lw);
        a.s.logw_s[w] = lws;
        const bool take = !div && (first || log(nuts_uniform(a, w, (uint64_t)nleaf, OCTO_DRAWS_PURPOSE_NUTS_LEAF)) < lw - lws);
        if (take) {
            for (int d = 0; d < a.D; ++d) a.s.sprop[(int64_t)d * a.ld + w] = a.s.trial[(int64_t)d * a.ld + w];
            a.s.sprop_lp[w] = lp; a.s.sprop_lpt[w] = lpt; a.s.ssel[w] = nleaf;
        }
        // 4. an odd n closes the aligned sub-subtrees of checkpoints imax … imin: the turn test of each, the smallest first
        int32_t status = div ? NUTS_DIVERGED : NUTS_BUILDING;
        if (!div && !even) {
            const int32_t imin = imax - (__ffs(~n) - 1) + 1;      // __ffs(~n) − 1: the trailing one-bits of n
            for (int i = imax; i >= imin && status == NUTS_BUILDING; --i) {
                const double *cp = a.s.ck_p + i * plane, *cr = a.s.ck_r + i * plane;
                double ta = 0.0, tb = 0.0;
                for (int d = 0; d < a.D; ++d) {
                    const int64_t o = (int64_t)d * a.ld + w;
                    const double c = cp[o];
                    const double mr = inv_mass_at(a.inv_mass, d) * (a.s.rho_s[o] - cr[o] + c);
                    ta += c * mr; tb += pe[o] * mr;
                }
                if (ta <= 0.0 || tb <= 0.0) status = NUTS_TURN_SUBTREE;
            }
        }
        // 5. the merge of a completed subtree and the tree's test
        if (status == NUTS_BUILDING && n + 1 == (1 << j)) {
            const double logw = a.s.logw[w];
            if (log(nuts_uniform(a, w, (uint64_t)j, OCTO_DRAWS_PURPOSE_NUTS_MERGE)) < lws - logw) {
                for (int d = 0; d < a.D; ++d) a.s.prop[(int64_t)d * a.ld + w] = a.s.sprop[(int64_t)d * a.ld + w];
                a.s.prop_lp[w] = a.s.sprop_lp[w]; a.s.prop_lpt[w] = a.s.sprop_lpt[w]; a.s.sel[w] = a.s.ssel[w];
            }
            a.s.logw[w] = log_add_exp(logw, lws);
            double ta = 0.0, tb = 0.0;
            for (int d = 0; d < a.D; ++d) {
                const int64_t o = (int64_t)d * a.ld + w;
                const double r = a.s.rho[o] + a.s.rho_s[o];
                a.s.rho[o] = r;
                const double mr = inv_mass_at(a.inv_mass, d) * r;
                ta += a.s.pL[o] * mr; tb += a.s.pR[o] * mr;
            }
            j += 1;
            a.s.depth[w] = j;
            if (ta <= 0.0 || tb <= 0.0) status = NUTS_TURN_TREE;
            else if (j == a.max_depth) status = NUTS_MAX_DEPTH;
            else {
                a.s.v[w] = nuts_uniform(a, w, (uint64_t)j, OCTO_DRAWS_PURPOSE_NUTS_DIRECTION) < 0.5 ? 1 : -1;
                a.s.n[w] = 0;
            }
        } else if (status == NUTS_BUILDING) a.s.n[w] = n + 1;
        // 6. the write-back of a chain that ends here; 7. otherwise the opening half kick and the drift of its next leaf
        if (status != NUTS_BUILDING) {
            a.s.status[w] = status;
            finish(a, w, a.s.sel[w] != 0, a.s.prop_lp[w], a.s.prop_lpt[w]);
        } else next_leaf<DENSE>(a, w, a.s.v[w], eps);
    }
    if (a.write_out) report(a, w);
}

__global__ __launch_bounds__(TPB) void k_nuts_open(NutsArgs a) { nuts_open<false>(a); }
__global__ __launch_bounds__(TPB) void k_nuts_leaf(NutsArgs a) { nuts_leaf<false>(a); }
__global__ __launch_bounds__(TPB) void k_dense_nuts_open(NutsArgs a) { nuts_open<true>(a); }
__global__ __launch_bounds__(TPB) void k_dense_nuts_leaf(NutsArgs a) { nuts_leaf<true>(a); }

__global__ __launch_bounds__(TPB) void k_nuts_report(NutsArgs a) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w < a.W) report(a, w);
}

}  // namespace

extern "C" {

int32_t octo_draws_nuts_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t, const double* d_beta,
                               const double* d_eps, double eps, const double* d_inv_mass, int32_t max_depth, int32_t n_rounds, int32_t resume, double* d_logpost,
                               double* d_loglike, double* d_log_accept, int32_t* d_accepted, int32_t* d_depth, int32_t* d_n_leapfrog, int32_t* d_diverged,
                               int32_t* d_n_active, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (max_depth < 1 || max_depth > OCTO_DRAWS_NUTS_MAX_DEPTH) return fail(h, OCTO_EINVAL, "octo_draws_nuts_device: max_depth must be 1 ... OCTO_DRAWS_NUTS_MAX_DEPTH");
    if (n_rounds < 0) return fail(h, OCTO_EINVAL, "octo_draws_nuts_device: n_rounds >= 0");
    const bool has_model = has_target(h);
    if (int rc = check_sampler_call(h, "octo_draws_nuts_device", W, ld, d_eps, eps, has_model, d_logpost, d_loglike)) return rc;
    const bool dense = h->d_metric != nullptr;
    if (dense && d_inv_mass) return fail(h, OCTO_EINVAL, "octo_draws_nuts_device: d_inv_mass must be NULL while a dense metric is set (octo_draws_use_metric)");
    if (resume && h->nuts_depth != 0 && h->nuts_metric != h->d_metric)
        return fail(h, OCTO_EINVAL, "octo_draws_nuts_device: resume needs the dense metric (octo_draws_use_metric) of the call it resumes");
    if (resume && (h->nuts_depth != max_depth || h->nuts_W != W || h->nuts_ld != ld || h->nuts_seed != seed || h->nuts_step != step || h->nuts_chain0 != chain0))
        return fail(h, OCTO_EINVAL, "octo_draws_nuts_device: resume needs a previous call with the same W, ld, max_depth, seed, step and chain0");
    if (W == 0) {
        if (!resume) h->nuts_depth = 0;
        return OCTO_OK;
    }
    if (!d_theta_t || !d_accepted) return fail(h, OCTO_EINVAL, "octo_draws_nuts_device: d_theta_t and d_accepted are required");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    if (!resume) {
        h->nuts_depth = 0;      // a call that fails below leaves nothing to resume
        int rc = grow(h, h->d_nuts, h->cap_nuts, carve_size(nuts_work, (int64_t)h->D, ld, (int64_t)max_depth)); if (rc) return rc;
    }
    NutsArgs a{sampler_head(h, has_model, seed, step, chain0, W, ld, d_theta_t, d_beta, d_eps, eps, d_inv_mass)};
    a.max_depth = max_depth;
    a.s = carve_at(h->d_nuts, nuts_work, (int64_t)h->D, ld, (int64_t)max_depth);
    double *lp = a.s.lp, *glp = a.s.glp;
    if (!has_model) { a.s.lp = nullptr; a.s.glp = nullptr; }
    a.o_lp = d_logpost; a.o_ll = d_loglike; a.o_la = d_log_accept; a.o_acc = d_accepted; a.o_depth = d_depth; a.o_nleaf = d_n_leapfrog; a.o_div = d_diverged;
    a.o_nact = d_n_active; a.chol = h->d_metric;
    if (d_n_active) OCHK(h, hipMemsetAsync(d_n_active, 0, sizeof(int32_t), st));      // the last launch of the call counts into it
    if (!resume)
        if (int rc = octo_draws_momentum_device(h, seed, step, chain0, W, ld, d_inv_mass, a.s.pL, hip_stream)) return rc;
    if (int rc = run_rounds(h, st, a, has_model, d_theta_t, lp, glp, n_rounds, resume != 0, dense ? k_dense_nuts_open : k_nuts_open, dense ? k_dense_nuts_leaf : k_nuts_leaf,
                            k_nuts_report)) return rc;
    h->nuts_metric = h->d_metric;
    h->nuts_W = W; h->nuts_ld = ld; h->nuts_depth = max_depth; h->nuts_seed = seed; h->nuts_step = step; h->nuts_chain0 = chain0;
    return OCTO_OK;
}

}  // extern "C"
