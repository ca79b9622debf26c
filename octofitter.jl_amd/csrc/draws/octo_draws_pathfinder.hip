// octo_draws_pathfinder.hip — Pathfinder on the L-BFGS paths of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states the
// function): a normal approximation at every accepted iterate of every chain, an ELBO estimate of it from a few draws, the best one kept,
// and draws from the kept one. The L-BFGS is octo_draws_lbfgs_device itself, called one round at a time with `resume`; this unit only READS
// the state that call leaves in the handle (x is the caller's θ_t; g, α, the ring and the counters sit in h->d_lbf, found through the
// optimiser's own layout function, lbfgs_state of octo_draws_layout.h; the Pathfinder state of h->d_pf is pf_state there).
//
//   k_pf_open     the chains' Pathfinder state at the start: no fit, ELBO −Inf.
//   k_pf_fit      the fit: ONE WAVE PER CHAIN, lane i = row i of H̃, H̃ in LDS (D·(D|1) doubles: 33 KB at D = 64). A lane runs its row's
//                 sums in index order; the few scalars (s̃ᵀỹ, ỹᵀw, logdet) are summed in index order from LDS by every lane alike, so no
//                 cross-lane reduction exists and the result of a chain depends on nothing but the chain.
//   k_pf_normals  one launch = one Philox block of four coordinates (as k_draw and k_hmc_momentum, and for their reason).
//   k_pf_map      z -> φ = μ + √α ⊙ (L̃z) and log q, lane = chain, a thread per (draw, chain); in place, rows from the last to the first.
//   k_pf_elbo     the ELBO of the candidate, the strict comparison with the kept one, the promotion (a flag flip) and the outputs.
//   k_pf_mask     ℓπ = −Inf at the draws of a chain without a fit (octo_draws_pathfinder_draw_device).
// Nothing of a chain lives in a private array. A round is 3 + ⌈D/4⌉ launches and one log-posterior call (logpost_at of octo_draws_common.h,
// without a gradient) besides the L-BFGS round.
#include "octo_draws_common.h"

namespace {

constexpr int PF_WAVE = 64;
constexpr double PF_LOG_2PI = 1.8378770664093453;

struct OpenArgs {
    PfState s;
    int64_t W;
};

__global__ __launch_bounds__(TPB) void k_pf_open(OpenArgs a) {
    const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (c >= a.W) return;
    a.s.elbo[c] = -INFINITY;
    a.s.slot[c] = 0; a.s.elbo_iter[c] = -1; a.s.n_fits[c] = 0; a.s.prev_iters[c] = 0; a.s.fresh[c] = 0;
}

struct FitArgs {
    const int32_t *cnt, *head;          // [W]
    const double *S, *Y;                // [m][D][ld]
    const double *x, *g, *alpha;        // [D][ld]
    const int32_t* iters;               // [W] or null: every chain is fitted. Otherwise only a chain whose iters moved past prev_iters
    int32_t* prev_iters;                // [W] with iters
    const int32_t* slot;                // [W] or null: the fit goes to slot 0. Otherwise to the slot that is not slot[c]
    double *mu, *sqa, *chol, *logdet;   // slot 0 of each; a slot is D·ld, D·ld, P·ld, ld doubles
    int32_t* ok;                        // [W] 1: a new fit
    int64_t ld;
    int32_t D, m;
};

__global__ __launch_bounds__(PF_WAVE) void k_pf_fit(FitArgs a) {
    extern __shared__ double pf_lds[];      // H̃ [D][st], then three vectors of PF_WAVE
    __shared__ int bad;
    const int64_t c = blockIdx.x;
    const int i = threadIdx.x, D = a.D, st = D | 1;      // an odd row length: the lanes' rows start on different banks
    double* H = pf_lds;
    double* vs = H + D * st;
    double* vy = vs + PF_WAVE;
    double* vw = vy + PF_WAVE;
    if (a.iters) {                          // the same for the whole block: no barrier is skipped by a part of it
        const int32_t it = a.iters[c], prev = a.prev_iters[c];
        __syncthreads();
        if (i == 0) a.prev_iters[c] = it;
        if (it == prev) {
            if (i == 0) a.ok[c] = 0;
            return;
        }
    }
    const int cand = a.slot ? 1 - a.slot[c] : 0;
    const bool on = i < D;
    const int64_t plane = (int64_t)D * a.ld, o = (int64_t)i * a.ld + c;
    const double al = on ? a.alpha[o] : 1.0, sa = sqrt(al);
    if (i == 0) bad = 0;
    __syncthreads();
    if (!(isfinite(al) && al > 0.0)) bad = 1;
    double* Hi = H + i * st;
    if (on)
        for (int j = 0; j < D; ++j) Hi[j] = i == j ? 1.0 : 0.0;
    const int32_t cnt = min(max(a.cnt[c], 0), a.m);
    const int32_t head = ((a.head[c] % a.m) + a.m) % a.m;
    for (int k = 0; k < cnt; ++k) {         // the inverse-BFGS updates, oldest pair first
        int32_t slot = head - cnt + k;
        slot += slot < 0 ? a.m : 0;
        if (on) {
            vs[i] = a.S[slot * plane + o] / sa;
            vy[i] = a.Y[slot * plane + o] * sa;
        }
        __syncthreads();
        double w = 0.0;
        if (on) {
            for (int j = 0; j < D; ++j) w += Hi[j] * vy[j];
            vw[i] = w;
        }
        __syncthreads();
        double sy = 0.0, yw = 0.0;
        for (int d = 0; d < D; ++d) {
            sy += vs[d] * vy[d];
            yw += vy[d] * vw[d];
        }
        const double rho = 1.0 / sy, cc = rho * (1.0 + rho * yw);
        if (on) {
            const double si = vs[i];
            for (int j = 0; j < D; ++j) Hi[j] = Hi[j] - rho * (si * vw[j] + w * vs[j]) + cc * (si * vs[j]);
        }
        __syncthreads();                    // vs, vy and vw are free again
    }
    if (on) vy[i] = sa * a.g[o];
    __syncthreads();
    if (on) {                               // μ = x − √α ⊙ (H̃(√α ⊙ g)), while H̃ is still whole
        double u = 0.0;
        for (int j = 0; j < D; ++j) u += Hi[j] * vy[j];
        a.mu[cand * plane + o] = a.x[o] - sa * u;
        a.sqa[cand * plane + o] = sa;
    }
    for (int j = 0; j < D; ++j) {           // Cholesky in the lower triangle, column by column: lane j the pivot, the lanes below it their entry
        if (i == j) {
            double p = Hi[j];
            for (int k = 0; k < j; ++k) p -= Hi[k] * Hi[k];
            if (!(isfinite(p) && p > 0.0)) bad = 1;
            Hi[j] = sqrt(p);
        }
        __syncthreads();
        if (on && i > j) {
            const double* Hj = H + j * st;
            double v = Hi[j];
            for (int k = 0; k < j; ++k) v -= Hi[k] * Hj[k];
            Hi[j] = v / Hj[j];
        }
    }
    if (on) {
        vs[i] = log(al);
        vw[i] = log(Hi[i]);
        double* row = a.chol + cand * ((int64_t)D * (D + 1) / 2) * a.ld + ((int64_t)i * (i + 1) / 2) * a.ld + c;
        for (int j = 0; j <= i; ++j) row[(int64_t)j * a.ld] = Hi[j];
    }
    __syncthreads();
    if (i == 0) {
        double la = 0.0, ll = 0.0;
        for (int d = 0; d < D; ++d) la += vs[d];
        for (int d = 0; d < D; ++d) ll += vw[d];
        a.logdet[(int64_t)cand * a.ld + c] = la + 2.0 * ll;
        a.ok[c] = bad ? 0 : 1;
    }
}

struct NormalArgs {
    uint64_t seed, chain0;
    const int32_t* iters;          // [W]: ELBO draws, purpose 4, t = iters[c]·32 + j. Null: final draws, purpose 5, t = j
    int64_t W, n;                  // chains, draws of each
    int64_t sj, sd;                // z of (draw j, coordinate d, chain c) at z[j·sj + d·sd + c]
    int32_t D, d0;                 // this launch: coordinates d0 … d0 + 3 (d0 a multiple of 4)
    double* z;
};

__global__ __launch_bounds__(TPB) void k_pf_normals(NormalArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= a.n * a.W) return;
    const int64_t j = t / a.W, c = t - j * a.W;
    const uint64_t step = a.iters ? (uint64_t)a.iters[c] * OCTO_DRAWS_PF_MAX_ELBO_DRAWS + (uint64_t)j : (uint64_t)j;
    uint64_t r[4];
    philox4x64(a.seed, KEY1, a.chain0 + (uint64_t)c, (uint64_t)(a.d0 >> 2), a.iters ? OCTO_DRAWS_PURPOSE_ELBO : OCTO_DRAWS_PURPOSE_PATHFINDER, step, r);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = a.d0 + q;
        if (d >= a.D) break;
        a.z[j * a.sj + (int64_t)d * a.sd + c] = normcdfinv(u01(r[q]));
    }
}

struct MapArgs {
    const double *mu, *sqa, *chol, *logdet;      // slot 0 of each, as in FitArgs
    const int32_t* slot;           // [W] or null: slot 0. Otherwise slot[c] ^ flip (flip = 1: the candidate)
    const int32_t* use;            // [W] or null: every chain. Otherwise a chain with use[c] < use_min sends x, and log q = NaN
    const double* x;               // [D][ld], with use
    const double* z;               // z and φ of (draw j, coordinate d, chain c) at [j·sj + d·sd + c]; they may be the same array
    double* phi;
    double* logq;                  // [n·W], draw j of chain c at j·W + c, or null
    int64_t W, n, ld, sj, sd;
    int32_t D, flip, use_min;
};

__global__ __launch_bounds__(TPB) void k_pf_map(MapArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= a.n * a.W) return;
    const int64_t j = t / a.W, c = t - j * a.W;
    const double* z = a.z + j * a.sj + c;      // not __restrict__: z and φ may be one array
    double* phi = a.phi + j * a.sj + c;
    if (a.use && a.use[c] < a.use_min) {
        for (int d = 0; d < a.D; ++d) phi[(int64_t)d * a.sd] = a.x[(int64_t)d * a.ld + c];
        if (a.logq) a.logq[t] = NAN;
        return;
    }
    const int s = a.slot ? a.slot[c] ^ a.flip : 0;
    const int64_t plane = (int64_t)a.D * a.ld;
    const double* __restrict__ mu = a.mu + s * plane + c;
    const double* __restrict__ sqa = a.sqa + s * plane + c;
    const double* __restrict__ L = a.chol + s * ((int64_t)a.D * (a.D + 1) / 2) * a.ld + c;
    double zz = 0.0;
    for (int d = 0; d < a.D; ++d) {
        const double zd = z[(int64_t)d * a.sd];
        zz += zd * zd;
    }
    for (int i = a.D - 1; i >= 0; --i) {     // row i reads z_0 … z_i alone: from the last row to the first, φ may take z's place
        const double* __restrict__ row = L + ((int64_t)i * (i + 1) / 2) * a.ld;
        double acc = 0.0;
        for (int k = 0; k <= i; ++k) acc += row[(int64_t)k * a.ld] * z[(int64_t)k * a.sd];
        phi[(int64_t)i * a.sd] = mu[(int64_t)i * a.ld] + sqa[(int64_t)i * a.ld] * acc;
    }
    if (a.logq) a.logq[t] = -0.5 * (a.D * PF_LOG_2PI + a.logdet[(int64_t)s * a.ld + c] + zz);
}

struct ElboArgs {
    PfState s;
    const int32_t* iters;          // [W] of the L-BFGS state
    const double *lp, *logq;       // [K·W], draw k of chain c at k·W + c
    int64_t W;
    int32_t K, update;             // update = 0: the outputs alone
    double* o_elbo;
    int32_t *o_iter, *o_nfits;
};

__global__ __launch_bounds__(TPB) void k_pf_elbo(ElboArgs a) {
    const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (c >= a.W) return;
    if (a.update && a.s.fresh[c]) {
        double sum = 0.0;
        bool fin = true;
        for (int k = 0; k < a.K; ++k) {
            const double lp = a.lp[(int64_t)k * a.W + c];
            fin = fin && isfinite(lp);
            sum += lp - a.logq[(int64_t)k * a.W + c];
        }
        const double elbo = fin ? sum / a.K : -INFINITY;
        a.s.n_fits[c] += 1;
        if (elbo > a.s.elbo[c]) {           // strict: the earliest fit wins a tie, −Inf and NaN never win
            a.s.elbo[c] = elbo;
            a.s.elbo_iter[c] = a.iters[c];
            a.s.slot[c] ^= 1;               // the candidate is the kept fit now
        }
    }
    a.o_elbo[c] = a.s.elbo[c]; a.o_iter[c] = a.s.elbo_iter[c]; a.o_nfits[c] = a.s.n_fits[c];
}

struct MaskArgs {
    const int32_t* elbo_iter;      // [W]
    double* lp;                    // [n·W]
    int64_t W, n;
};

__global__ __launch_bounds__(TPB) void k_pf_mask(MaskArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= a.n * a.W) return;
    if (a.elbo_iter[t % a.W] < 0) a.lp[t] = -INFINITY;
}

inline size_t fit_lds_bytes(int D) { return sizeof(double) * ((size_t)D * (D | 1) + 3 * PF_WAVE); }

void launch_normals(hipStream_t st, NormalArgs n) {
    for (n.d0 = 0; n.d0 < n.D; n.d0 += 4) hipLaunchKernelGGL(k_pf_normals, grid_of(n.n * n.W), dim3(TPB), 0, st, n);
}

}  // namespace

extern "C" {

int32_t octo_draws_pathfinder_fit_device(octo_draws* h, int64_t W, int64_t ld, int32_t m, const int32_t* d_cnt, const int32_t* d_head, const double* d_S,
                                         const double* d_Y, const double* d_x, const double* d_g, const double* d_alpha, double* d_mu, double* d_chol,
                                         double* d_logdet, int32_t* d_ok, int32_t n, const double* d_z, double* d_phi, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (h->D > OCTO_DRAWS_PF_MAX_D) return fail(h, OCTO_ENOTSUP, "octo_draws_pathfinder_fit_device: D > OCTO_DRAWS_PF_MAX_D");
    if (int rc = check_m(h, "octo_draws_pathfinder_fit_device", m)) return rc;
    if (int rc = check_chains(h, "octo_draws_pathfinder_fit_device", W, ld, MAX_CHAINS, "2^30")) return rc;
    if (n < 0 || (int64_t)n * W > MAX_CHAINS) return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_fit_device: need n >= 0, n*W <= 2^30");
    if (W == 0) return OCTO_OK;
    if (!d_cnt || !d_head || !d_S || !d_Y || !d_x || !d_g || !d_alpha || !d_mu || !d_chol || !d_logdet || !d_ok || (n > 0 && (!d_z || !d_phi)))
        return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_fit_device: only d_z and d_phi may be NULL, with n = 0");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t D = h->D, plane = D * ld;
    { int rc = grow(h, h->d_pfb, h->cap_pfb, plane); if (rc) return rc; }      // √α
    FitArgs f;
    std::memset(&f, 0, sizeof(f));
    f.cnt = d_cnt; f.head = d_head; f.S = d_S; f.Y = d_Y; f.x = d_x; f.g = d_g; f.alpha = d_alpha;
    f.mu = d_mu; f.sqa = h->d_pfb; f.chol = d_chol; f.logdet = d_logdet; f.ok = d_ok; f.ld = ld; f.D = h->D; f.m = m;
    hipLaunchKernelGGL(k_pf_fit, dim3((unsigned)W), dim3(PF_WAVE), fit_lds_bytes(h->D), st, f);
    if (n > 0) {
        MapArgs p;
        std::memset(&p, 0, sizeof(p));
        p.mu = d_mu; p.sqa = h->d_pfb; p.chol = d_chol; p.logdet = d_logdet; p.z = d_z; p.phi = d_phi;
        p.W = W; p.n = n; p.ld = ld; p.sj = plane; p.sd = ld; p.D = h->D;
        hipLaunchKernelGGL(k_pf_map, grid_of((int64_t)n * W), dim3(TPB), 0, st, p);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_pathfinder_device(octo_draws* h, uint64_t seed, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t, const double* d_inv_mass,
                                     int32_t m, int32_t n_rounds, double gtol, double ftol, int32_t n_elbo, int32_t resume, double* d_logpost,
                                     double* d_gnorm, int32_t* d_status, int32_t* d_iters, int32_t* d_evals, double* d_inv_hess_diag, double* d_elbo,
                                     int32_t* d_elbo_iter, int32_t* d_n_fits, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (int rc = check_model(h, "octo_draws_pathfinder_device")) return rc;
    if (h->D > OCTO_DRAWS_PF_MAX_D) return fail(h, OCTO_ENOTSUP, "octo_draws_pathfinder_device: D > OCTO_DRAWS_PF_MAX_D");
    if (int rc = check_m(h, "octo_draws_pathfinder_device", m)) return rc;
    if (n_rounds < 0) return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_device: n_rounds >= 0");
    if (n_elbo < 1 || n_elbo > OCTO_DRAWS_PF_MAX_ELBO_DRAWS) return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_device: n_elbo must be 1 ... OCTO_DRAWS_PF_MAX_ELBO_DRAWS");
    if (int rc = check_chains(h, "octo_draws_pathfinder_device", W, ld, MAX_CHAINS / OCTO_DRAWS_PF_MAX_ELBO_DRAWS, "2^25")) return rc;
    if (int rc = check_tolerances(h, "octo_draws_pathfinder_device", gtol, ftol)) return rc;
    if (resume && (h->pf_W == 0 || h->pf_W != W || h->pf_ld != ld || h->lbf_W != W || h->lbf_ld != ld || h->lbf_m != m))
        return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_device: resume needs a previous call with the same W, ld and m");
    if (W == 0) return OCTO_OK;
    if (!d_theta_t || !d_logpost || !d_gnorm || !d_status || !d_iters || !d_evals || !d_elbo || !d_elbo_iter || !d_n_fits)
        return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_device: only d_inv_mass and d_inv_hess_diag may be NULL");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t D = h->D, KW = (int64_t)n_elbo * W;
    if (!resume) {
        h->pf_W = 0;      // a call that fails below leaves nothing to resume or to draw from
        int rc = grow(h, h->d_pf, h->cap_pf, carve_size(pf_state, D, ld)); if (rc) return rc;
    }
    PfBatch b;
    if (int rc = grow_to(h, h->d_pfb, h->cap_pfb, b, pf_batch, D, KW)) return rc;
    const PfState s = carve_at(h->d_pf, pf_state, D, ld);
    // the opening evaluation (or, resumed, the outputs as they stand); every round below is the existing call with one round and resume
    {
        int rc = octo_draws_lbfgs_device(h, W, ld, d_theta_t, d_inv_mass, m, 0, gtol, ftol, resume, d_logpost, d_gnorm, d_status, d_iters, d_evals,
                                         d_inv_hess_diag, hip_stream);
        if (rc) return rc;
    }
    if (!resume) {
        OpenArgs o; o.s = s; o.W = W;
        hipLaunchKernelGGL(k_pf_open, grid_of(W), dim3(TPB), 0, st, o);
    }
    const LbfgsState v = carve_at(h->d_lbf, lbfgs_state, D, ld, (int64_t)m);      // as the call above left it
    FitArgs f;
    std::memset(&f, 0, sizeof(f));
    f.cnt = v.cnt; f.head = v.head; f.S = v.S; f.Y = v.Y; f.x = d_theta_t; f.g = v.g; f.alpha = v.alpha; f.iters = v.iters; f.prev_iters = s.prev_iters;
    f.slot = s.slot; f.mu = s.mu; f.sqa = s.sqa; f.chol = s.chol; f.logdet = s.logdet; f.ok = s.fresh; f.ld = ld; f.D = h->D; f.m = m;
    NormalArgs z;
    std::memset(&z, 0, sizeof(z));
    z.seed = seed; z.chain0 = chain0; z.iters = v.iters; z.W = W; z.n = n_elbo; z.sj = W; z.sd = KW; z.D = h->D; z.z = b.phi;
    MapArgs p;
    std::memset(&p, 0, sizeof(p));
    p.mu = s.mu; p.sqa = s.sqa; p.chol = s.chol; p.logdet = s.logdet; p.slot = s.slot; p.flip = 1; p.use = s.fresh; p.use_min = 1; p.x = d_theta_t;
    p.z = b.phi; p.phi = b.phi; p.logq = b.logq; p.W = W; p.n = n_elbo; p.ld = ld; p.sj = W; p.sd = KW; p.D = h->D;
    ElboArgs e;
    std::memset(&e, 0, sizeof(e));
    e.s = s; e.iters = v.iters; e.lp = b.lp; e.logq = b.logq; e.W = W; e.K = n_elbo; e.update = 1; e.o_elbo = d_elbo; e.o_iter = d_elbo_iter; e.o_nfits = d_n_fits;
    for (int r = 1; r <= n_rounds; ++r) {
        int rc = octo_draws_lbfgs_device(h, W, ld, d_theta_t, d_inv_mass, m, 1, gtol, ftol, 1, d_logpost, d_gnorm, d_status, d_iters, d_evals,
                                         d_inv_hess_diag, hip_stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_pf_fit, dim3((unsigned)W), dim3(PF_WAVE), fit_lds_bytes(h->D), st, f);
        launch_normals(st, z);
        hipLaunchKernelGGL(k_pf_map, grid_of(KW), dim3(TPB), 0, st, p);
        OCHK(h, hipGetLastError());
        rc = logpost_at(h, st, true, b.phi, KW, KW, b.lp, nullptr); if (rc) return rc;
        hipLaunchKernelGGL(k_pf_elbo, grid_of(W), dim3(TPB), 0, st, e);
    }
    if (n_rounds == 0) {
        e.update = 0;
        hipLaunchKernelGGL(k_pf_elbo, grid_of(W), dim3(TPB), 0, st, e);
    }
    OCHK(h, hipGetLastError());
    h->pf_W = W; h->pf_ld = ld;
    return OCTO_OK;
}

int32_t octo_draws_pathfinder_draw_device(octo_draws* h, uint64_t seed, uint64_t chain0, int64_t W, int64_t ld, const double* d_theta_t, int32_t n_draws,
                                          int64_t ld_out, double* d_phi, double* d_logq, double* d_logpost, void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    if (int rc = check_model(h, "octo_draws_pathfinder_draw_device")) return rc;
    if (h->D > OCTO_DRAWS_PF_MAX_D) return fail(h, OCTO_ENOTSUP, "octo_draws_pathfinder_draw_device: D > OCTO_DRAWS_PF_MAX_D");
    if (n_draws < 1) return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_draw_device: n_draws >= 1");
    if (W < 0 || ld < W || (int64_t)n_draws * W > MAX_CHAINS) return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_draw_device: need 0 <= W <= ld, n_draws*W <= 2^30");
    if (ld_out < (int64_t)n_draws * W) return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_draw_device: need ld_out >= n_draws*W");
    if (h->pf_W == 0 || h->pf_W != W || h->pf_ld != ld)
        return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_draw_device: needs a previous octo_draws_pathfinder_device call with the same W and ld");
    if (W == 0) return OCTO_OK;
    if (!d_theta_t || !d_phi || !d_logq || !d_logpost) return fail(h, OCTO_EINVAL, "octo_draws_pathfinder_draw_device: no array may be NULL");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t NW = (int64_t)n_draws * W;
    const PfState s = carve_at(h->d_pf, pf_state, (int64_t)h->D, ld);
    NormalArgs z;
    std::memset(&z, 0, sizeof(z));
    z.seed = seed; z.chain0 = chain0; z.W = W; z.n = n_draws; z.sj = W; z.sd = ld_out; z.D = h->D; z.z = d_phi;
    launch_normals(st, z);
    MapArgs p;
    std::memset(&p, 0, sizeof(p));
    p.mu = s.mu; p.sqa = s.sqa; p.chol = s.chol; p.logdet = s.logdet; p.slot = s.slot; p.flip = 0; p.use = s.elbo_iter; p.use_min = 0; p.x = d_theta_t;
    p.z = d_phi; p.phi = d_phi; p.logq = d_logq; p.W = W; p.n = n_draws; p.ld = ld; p.sj = W; p.sd = ld_out; p.D = h->D;
    hipLaunchKernelGGL(k_pf_map, grid_of(NW), dim3(TPB), 0, st, p);
    OCHK(h, hipGetLastError());
    if (int rc = logpost_at(h, st, true, d_phi, ld_out, NW, d_logpost, nullptr)) return rc;
    MaskArgs k;
    k.elbo_iter = s.elbo_iter; k.lp = d_logpost; k.W = W; k.n = n_draws;
    hipLaunchKernelGGL(k_pf_mask, grid_of(NW), dim3(TPB), 0, st, k);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // extern "C"
