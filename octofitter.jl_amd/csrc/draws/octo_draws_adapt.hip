// octo_draws_adapt.hip — the warm-up statistics of the explorer in liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states them):
// grouped cross-chain moments, the diagonal metric they give, dual averaging of the step size on the mean acceptance probability, and
// per-chain running moments. Lane = chain, SoA with the chain index fastest. No floating-point atomic: every sum has a fixed order.
//
//   k_adapt_partials<ACCEPT>  one block = 256 chains. Per row and group present in a wave (a wave-uniform ballot): the masked sum by a
//                             butterfly over the wave, the four waves added in wave order through LDS, the block's mean, then the masked
//                             Σ(x − mean)² the same way — two passes over a value the lane holds in a register. Stores (n, Σx, M2) per
//                             (block, group, row). ACCEPT = true: the one row is min(1, exp(dH)) made on the fly, and no M2.
//   k_adapt_merge             one block per group, one thread per row: the blocks' triples in block order, then the held state (accumulate).
//   k_adapt_metric            K threads · k_adapt_init, k_adapt_da  G threads · k_adapt_eps, k_adapt_chain  element-wise.
// The moments are 2 launches, an update of the step size 3 (2 without d_eps_w), the others 1.
#include "octo_draws_common.h"

namespace {

constexpr int WAVES = TPB / 64;
constexpr int MAXG = OCTO_DRAWS_MAX_GROUPS;
constexpr int64_t MAX_ADAPT_CHAINS = (int64_t)1 << 24;

struct PartialArgs {
    const double* x;               // [K][ld]; ACCEPT: dH [W]
    const int32_t* accepted;       // ACCEPT: [W]
    const int32_t* group;          // [W] or null = 0
    int64_t W, ld;
    int32_t K, G;
    MomentsPartials p;
};

// the four waves' entries of group g in wave order; a wave without a member of g wrote none
__device__ __forceinline__ double block_total(const double (&s)[WAVES][MAXG], const double (&n)[WAVES][MAXG], int g) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < WAVES; ++q) t += n[q][g] > 0.0 ? s[q][g] : 0.0;
    return t;
}

template <bool ACCEPT>
__global__ __launch_bounds__(TPB) void k_adapt_partials(PartialArgs a) {
    __shared__ double s_n[WAVES][MAXG], s_sum[WAVES][MAXG], s_m2[WAVES][MAXG];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t w = (int64_t)blockIdx.x * TPB + tid;
    const bool live = w < a.W;                          // no early exit: ballots, shuffles and barriers below
    int gid = live ? (a.group ? a.group[w] : 0) : -1;
    bool valid = live && gid >= 0 && gid < a.G;
    if (!ACCEPT && valid) {                             // every row is read, none waits for the one before it
        bool fin = true;
        for (int k = 0; k < a.K; ++k) fin = fin & isfinite(a.x[(int64_t)k * a.ld + w]);
        valid = fin;
    }
    gid = valid ? gid : -1;
    s_n[wave][lane] = 0.0;
    __syncthreads();
    for (int g = 0; g < a.G; ++g) {
        const unsigned long long m = __ballot(gid == g);
        if (m && lane == 0) s_n[wave][g] = (double)__popcll(m);
    }
    __syncthreads();
    const int gl = valid ? gid : 0;
    double nb = 0.0, ng = 0.0;                          // chains of the block in this lane's group · in group tid (tid < G)
#pragma unroll
    for (int q = 0; q < WAVES; ++q) { nb += s_n[q][gl]; ng += tid < a.G ? s_n[q][tid] : 0.0; }
    const int64_t og = (int64_t)blockIdx.x * a.G + tid;
    if (tid < a.G) a.p.cnt[og] = ng;
    double vn = 0.0;                                    // the next row's value, loaded a row ahead of the barriers
    if (valid) {
        if (ACCEPT) {
            const double dH = a.x[w];
            vn = dH != dH ? (a.accepted[w] ? 1.0 : 0.0) : fmin(1.0, exp(dH));
        } else vn = a.x[w];
    }
    for (int k = 0; k < a.K; ++k) {
        const double v = vn;
        if (!ACCEPT && valid && k + 1 < a.K) vn = a.x[(int64_t)(k + 1) * a.ld + w];
        for (int g = 0; g < a.G; ++g) {
            if (!__ballot(gid == g)) continue;          // wave-uniform
            const double t = wave_sum(gid == g ? v : 0.0);
            if (lane == 0) s_sum[wave][g] = t;
        }
        __syncthreads();
        if (tid < a.G && ng > 0.0) a.p.sum[og * a.K + k] = block_total(s_sum, s_n, tid);
        if (ACCEPT) continue;                           // one row: no barrier follows
        const double dev = valid ? v - block_total(s_sum, s_n, gl) / nb : 0.0;
        for (int g = 0; g < a.G; ++g) {
            if (!__ballot(gid == g)) continue;
            const double t = wave_sum(gid == g ? dev * dev : 0.0);
            if (lane == 0) s_m2[wave][g] = t;
        }
        __syncthreads();
        if (tid < a.G && ng > 0.0) a.p.m2[og * a.K + k] = block_total(s_m2, s_n, tid);
    }
}

struct MergeArgs {
    MomentsPartials p;
    int64_t nblk;
    int32_t G, K, accumulate;
    double *count, *mean, *m2;     // [G], [G][K], [G][K]
};

__global__ __launch_bounds__(TPB) void k_adapt_merge(MergeArgs a) {
    const int g = blockIdx.x, k = threadIdx.x;
    const bool live = k < a.K;
    double n = 0.0, s = 0.0, m2 = 0.0;
    if (live)
        for (int64_t b = 0; b < a.nblk; ++b) {
            const double nb = a.p.cnt[b * a.G + g];
            if (nb == 0.0) continue;
            const int64_t o = (b * a.G + g) * a.K + k;
            const double sb = a.p.sum[o], mb = a.p.m2[o];
            if (n == 0.0) { n = nb; s = sb; m2 = mb; continue; }
            const double d = sb / nb - s / n, nn = n + nb;
            m2 = m2 + mb + d * d * n * nb / nn;
            s += sb;
            n = nn;
        }
    double mean = n > 0.0 ? s / n : 0.0;
    const int64_t o = (int64_t)g * a.K + k;
    const double na = live && a.accumulate ? a.count[g] : 0.0;      // every row reads the held count before row 0 replaces it
    __syncthreads();
    if (!live) return;
    if (a.accumulate) {
        if (n == 0.0) return;
        if (na > 0.0) {
            const double ma = a.mean[o], nn = na + n, d = mean - ma;
            mean = ma + d * n / nn;
            m2 = a.m2[o] + m2 + d * d * na * n / nn;
            n = nn;
        }
    }
    if (k == 0) a.count[g] = n;
    a.mean[o] = mean;
    a.m2[o] = m2;
}

__global__ __launch_bounds__(TPB) void k_adapt_metric(int32_t K, const double* count, const double* m2, int32_t regularize, double* inv_mass) {
    const int d = threadIdx.x;
    if (d >= K) return;
    const double n = count[0];
    if (!(n >= 2.0)) return;
    const double var = m2[d] / (n - 1.0);
    const double v = regularize ? (n / (n + 5.0)) * var + 1e-3 * 5.0 / (n + 5.0) : var;
    if (isfinite(v) && v > 0.0) inv_mass[d] = v;
}

__global__ __launch_bounds__(TPB) void k_adapt_init(int32_t G, const double* eps0_g, double eps0, double* state) {
    const int g = threadIdx.x;
    if (g >= G) return;
    const double e = eps0_g ? eps0_g[g] : eps0, x = log(e);
    state[4 * g] = x; state[4 * g + 1] = x; state[4 * g + 2] = 0.0; state[4 * g + 3] = log(10.0 * e);
}

struct DaArgs {
    MomentsPartials p;             // of k_adapt_partials<true>: one row
    int64_t nblk;
    int32_t G;
    double eta, delta, sk, wk;     // 1/(k + t0), δ, √k/γ, k^(−κ): the host's doubles
    double *state, *accept_stat;
};

__global__ __launch_bounds__(TPB) void k_adapt_da(DaArgs a) {
    const int g = threadIdx.x;
    if (g >= a.G) return;
    double n = 0.0, s = 0.0;
    for (int64_t b = 0; b < a.nblk; ++b) {
        const double nb = a.p.cnt[b * a.G + g];
        if (nb == 0.0) continue;
        n += nb;
        s += a.p.sum[b * a.G + g];
    }
    if (n == 0.0) {
        if (a.accept_stat) a.accept_stat[g] = NAN;
        return;
    }
    const double ag = s / n;
    if (a.accept_stat) a.accept_stat[g] = ag;
    double* st = a.state + 4 * g;
    const double Hbar = (1.0 - a.eta) * st[2] + a.eta * (a.delta - ag);
    const double x = st[3] - a.sk * Hbar;
    st[0] = x;
    st[1] = a.wk * x + (1.0 - a.wk) * st[1];
    st[2] = Hbar;
}

__global__ __launch_bounds__(TPB) void k_adapt_eps(int64_t W, const int32_t* group, int32_t G, const double* state, int32_t use_average, double* eps_w) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w >= W) return;
    const int g = group ? group[w] : 0;
    if (g < 0 || g >= G) return;
    eps_w[w] = exp(state[4 * g + (use_average ? 1 : 0)]);
}

// blockIdx.y = the row
__global__ __launch_bounds__(TPB) void k_adapt_chain(int64_t W, int64_t ld, int64_t k, const double* x, double* cmean, double* cm2) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w >= W) return;
    const int64_t o = (int64_t)blockIdx.y * ld + w;
    const double v = x[o];
    if (k == 1) { cmean[o] = v; cm2[o] = 0.0; return; }
    const double d = v - cmean[o], mean = cmean[o] + d / (double)k;
    cmean[o] = mean;
    cm2[o] += d * (v - mean);
}

inline int check_count(octo_draws* h, const char* who, const char* name, int32_t v) {
    return v >= 1 && v <= OCTO_DRAWS_MAX_GROUPS ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": " + name + " must be 1 ... OCTO_DRAWS_MAX_GROUPS");
}

}  // namespace

extern "C" {

int32_t octo_draws_moments_device(octo_draws* h, int64_t W, int64_t ld, int32_t K, const double* d_x, const int32_t* d_group, int32_t G,
                                  int32_t accumulate, double* d_count, double* d_mean, double* d_m2, void* hip_stream) {
    const char* who = "octo_draws_moments_device";
    if (!h) return OCTO_EINVAL;
    if ((!d_x && W != 0) || !d_count || !d_mean || !d_m2) return fail(h, OCTO_EINVAL, std::string(who) + ": d_x, d_count, d_mean and d_m2 are required");
    if (int rc = check_count(h, who, "K", K)) return rc;
    if (int rc = check_count(h, who, "G", G)) return rc;
    if (!d_group && G != 1 && W != 0) return fail(h, OCTO_EINVAL, std::string(who) + ": G must be 1 when d_group is NULL");
    if (int rc = check_chains(h, who, W, ld, MAX_ADAPT_CHAINS, "2^24")) return rc;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t nblk = (W + TPB - 1) / TPB;
    PartialArgs a;
    a.x = d_x; a.accepted = nullptr; a.group = d_group; a.W = W; a.ld = ld; a.K = K; a.G = G;
    if (int rc = grow_to(h, h->d_mom, h->cap_mom, a.p, moments_partials, nblk, (int64_t)G, (int64_t)K)) return rc;
    if (nblk) hipLaunchKernelGGL(k_adapt_partials<false>, dim3((unsigned)nblk), dim3(TPB), 0, st, a);
    MergeArgs m;
    m.p = a.p; m.nblk = nblk; m.G = G; m.K = K; m.accumulate = accumulate ? 1 : 0; m.count = d_count; m.mean = d_mean; m.m2 = d_m2;
    hipLaunchKernelGGL(k_adapt_merge, dim3((unsigned)G), dim3(TPB), 0, st, m);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_metric_device(octo_draws* h, int32_t K, const double* d_count_g, const double* d_mean_g, const double* d_m2_g,
                                 int32_t regularize, double* d_inv_mass, void* hip_stream) {
    const char* who = "octo_draws_metric_device";
    if (!h) return OCTO_EINVAL;
    if (!d_count_g || !d_mean_g || !d_m2_g || !d_inv_mass) return fail(h, OCTO_EINVAL, std::string(who) + ": every array is required");
    if (int rc = check_count(h, who, "K", K)) return rc;
    OCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_adapt_metric, dim3(1), dim3(TPB), 0, stream_of(h, hip_stream), K, d_count_g, d_m2_g, regularize ? 1 : 0, d_inv_mass);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_hmc_adapt_init_device(octo_draws* h, int32_t G, const double* d_eps0, double eps0, double* d_state, void* hip_stream) {
    const char* who = "octo_draws_hmc_adapt_init_device";
    if (!h) return OCTO_EINVAL;
    if (!d_state) return fail(h, OCTO_EINVAL, std::string(who) + ": d_state is required");
    if (int rc = check_count(h, who, "G", G)) return rc;
    if (!d_eps0 && !(eps0 > 0.0 && std::isfinite(eps0))) return fail(h, OCTO_EINVAL, std::string(who) + ": eps0 must be finite and > 0 when d_eps0 is NULL");
    OCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_adapt_init, dim3(1), dim3(TPB), 0, stream_of(h, hip_stream), G, d_eps0, eps0, d_state);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_hmc_adapt_device(octo_draws* h, int64_t W, const int32_t* d_group, int32_t G, const double* d_dH, const int32_t* d_accepted,
                                    int64_t k, double delta, double gamma, double t0, double kappa, double* d_state, double* d_accept_stat,
                                    int32_t use_average, double* d_eps_w, void* hip_stream) {
    const char* who = "octo_draws_hmc_adapt_device";
    if (!h) return OCTO_EINVAL;
    if (!d_dH || !d_accepted || !d_state) return fail(h, OCTO_EINVAL, std::string(who) + ": d_dH, d_accepted and d_state are required");
    if (int rc = check_count(h, who, "G", G)) return rc;
    if (!d_group && G != 1 && W != 0) return fail(h, OCTO_EINVAL, std::string(who) + ": G must be 1 when d_group is NULL");
    if (int rc = check_chains(h, who, W, W, MAX_ADAPT_CHAINS, "2^24")) return rc;
    if (k < 1) return fail(h, OCTO_EINVAL, std::string(who) + ": k >= 1");
    if (!(std::isfinite(delta) && delta > 0.0 && delta < 1.0 && std::isfinite(gamma) && gamma > 0.0 && std::isfinite(t0) && t0 >= 0.0 &&
          std::isfinite(kappa) && kappa > 0.0))
        return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 < delta < 1, gamma > 0, t0 >= 0, kappa > 0, all finite");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t nblk = (W + TPB - 1) / TPB;
    PartialArgs a;
    a.x = d_dH; a.accepted = d_accepted; a.group = d_group; a.W = W; a.ld = W; a.K = 1; a.G = G;
    if (int rc = grow_to(h, h->d_mom, h->cap_mom, a.p, moments_partials, nblk, (int64_t)G, (int64_t)1)) return rc;
    if (nblk) hipLaunchKernelGGL(k_adapt_partials<true>, dim3((unsigned)nblk), dim3(TPB), 0, st, a);
    DaArgs d;
    d.p = a.p; d.nblk = nblk; d.G = G; d.eta = 1.0 / ((double)k + t0); d.delta = delta; d.sk = std::sqrt((double)k) / gamma;
    d.wk = std::pow((double)k, -kappa); d.state = d_state; d.accept_stat = d_accept_stat;
    hipLaunchKernelGGL(k_adapt_da, dim3(1), dim3(TPB), 0, st, d);
    if (d_eps_w && W) hipLaunchKernelGGL(k_adapt_eps, grid_of(W), dim3(TPB), 0, st, W, d_group, G, (const double*)d_state, use_average ? 1 : 0, d_eps_w);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_chain_moments_device(octo_draws* h, int64_t W, int64_t ld, int32_t K, int64_t k, const double* d_x, double* d_cmean,
                                        double* d_cm2, void* hip_stream) {
    const char* who = "octo_draws_chain_moments_device";
    if (!h) return OCTO_EINVAL;
    if (!d_x || !d_cmean || !d_cm2) return fail(h, OCTO_EINVAL, std::string(who) + ": d_x, d_cmean and d_cm2 are required");
    if (int rc = check_count(h, who, "K", K)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_ADAPT_CHAINS, "2^24")) return rc;
    if (k < 1) return fail(h, OCTO_EINVAL, std::string(who) + ": k >= 1");
    if (W == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_adapt_chain, dim3((unsigned)((W + TPB - 1) / TPB), (unsigned)K), dim3(TPB), 0, stream_of(h, hip_stream), W, ld, k, d_x, d_cmean, d_cm2);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // extern "C"
