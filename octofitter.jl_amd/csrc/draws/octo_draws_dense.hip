// octo_draws_dense.hip — the dense metric of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, the fourteenth part, states it): the
// pooled covariance of the chains, its Cholesky factor L (M⁻¹ = L·Lᵀ), the products L·x and Lᵀ·x behind an entry point, and the handle state that
// sends the HMC step and NUTS down their dense kernels. No floating-point atomic: every sum has a fixed order, every call the same bits.
//
//   k_dense_cov_partials  one block = 256 chains: the chains with every row finite, per row their sum (a butterfly over the wave, the four waves in
//                         wave order through LDS) and the block's mean, then per pair i >= j the Σ of the products of the deviations from it the same
//                         way, a row of pairs between two barriers. The rows are read again through the caches: nothing of a chain in a private array.
//   k_dense_cov_merge     one block: a thread per pair merges the blocks' triples in block order by Chan's formula, then into the held state
//                         (accumulate); the means and the count follow behind a barrier, once every pair has read what was held.
//   k_dense_factor        one wave, lane = row: Σ from the co-moments into LDS, the left-looking Cholesky on it in place, the copy out if every pivot held.
//   k_dense_apply         lane = column: metric_lower or metric_lower_t of octo_draws_common.h, the routines the samplers' dense kernels call.
#include "octo_draws_common.h"

namespace {

constexpr int WAVES = TPB / 64;
constexpr int MAXK = OCTO_DRAWS_DENSE_MAX_D;
constexpr int64_t MAX_COV_CHAINS = (int64_t)1 << 24;

struct CovArgs {
    const double* x;               // [K][ld]
    int64_t W, ld;
    int32_t K;
    CovPartials p;
};

// the four waves' entries of column k in wave order
__device__ __forceinline__ double column_total(const double (&s)[WAVES][MAXK], int k) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < WAVES; ++q) t += s[q][k];
    return t;
}

__global__ __launch_bounds__(TPB) void k_dense_cov_partials(CovArgs a) {
    __shared__ double s_w[WAVES][MAXK], s_mean[MAXK], s_n[WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t w = (int64_t)blockIdx.x * TPB + tid;
    bool valid = w < a.W;                               // no early exit of a lane: ballots, shuffles and barriers below
    if (valid) {
        bool fin = true;
        for (int k = 0; k < a.K; ++k) fin = fin & isfinite(a.x[(int64_t)k * a.ld + w]);
        valid = fin;
    }
    const unsigned long long m = __ballot(valid);
    if (lane == 0) s_n[wave] = (double)__popcll(m);
    __syncthreads();
    const double nb = waves_total(s_n);
    if (tid == 0) a.p.cnt[blockIdx.x] = nb;
    if (nb == 0.0) return;                              // the whole block
    for (int k = 0; k < a.K; ++k) {
        const double t = wave_sum(valid ? a.x[(int64_t)k * a.ld + w] : 0.0);
        if (lane == 0) s_w[wave][k] = t;
    }
    __syncthreads();
    if (tid < a.K) {
        const double s = column_total(s_w, tid);
        a.p.sum[(int64_t)blockIdx.x * a.K + tid] = s;
        s_mean[tid] = s / nb;
    }
    __syncthreads();
    const int64_t P = (int64_t)a.K * (a.K + 1) / 2;
    for (int i = 0; i < a.K; ++i) {
        const double di = valid ? a.x[(int64_t)i * a.ld + w] - s_mean[i] : 0.0;
        for (int j = 0; j <= i; ++j) {
            const double dj = valid ? a.x[(int64_t)j * a.ld + w] - s_mean[j] : 0.0;
            const double t = wave_sum(di * dj);
            if (lane == 0) s_w[wave][j] = t;
        }
        __syncthreads();
        if (tid <= i) a.p.m2[(int64_t)blockIdx.x * P + (i * (i + 1) >> 1) + tid] = column_total(s_w, tid);
        __syncthreads();
    }
}

struct CovMergeArgs {
    CovPartials p;
    int64_t nblk;
    int32_t K, accumulate;
    double *count, *mean, *m2;     // [1], [K], [K(K+1)/2]
};

__global__ __launch_bounds__(TPB) void k_dense_cov_merge(CovMergeArgs a) {
    const int tid = threadIdx.x;
    const int P = a.K * (a.K + 1) / 2;
    const double na = a.accumulate ? a.count[0] : 0.0;      // every thread reads the held count before thread 0 replaces it
    double nt = 0.0;                                        // this call's chains
    for (int p = tid; p < P; p += TPB) {
        int i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);   // the row of pair p, put right where the root rounded
        while ((i * (i + 1) >> 1) > p) --i;
        while (((i + 1) * (i + 2) >> 1) <= p) ++i;
        const int j = p - (i * (i + 1) >> 1);
        double n = 0.0, si = 0.0, sj = 0.0, m2 = 0.0;
        for (int64_t b = 0; b < a.nblk; ++b) {
            const double nb = a.p.cnt[b];
            if (nb == 0.0) continue;
            const double bi = a.p.sum[b * a.K + i], bj = a.p.sum[b * a.K + j], mb = a.p.m2[b * P + p];
            if (n == 0.0) { n = nb; si = bi; sj = bj; m2 = mb; continue; }
            const double di = bi / nb - si / n, dj = bj / nb - sj / n, nn = n + nb;
            m2 = m2 + mb + di * dj * n * nb / nn;
            si += bi; sj += bj;
            n = nn;
        }
        if (a.accumulate) {
            if (n == 0.0) continue;
            if (na > 0.0) {
                const double di = si / n - a.mean[i], dj = sj / n - a.mean[j];
                m2 = a.m2[p] + m2 + di * dj * na * n / (na + n);
            }
        }
        a.m2[p] = m2;
    }
    __syncthreads();                                        // every pair has read the held means
    if (tid >= a.K) return;
    double s = 0.0;
    for (int64_t b = 0; b < a.nblk; ++b) {
        const double nb = a.p.cnt[b];
        if (nb == 0.0) continue;
        s += a.p.sum[b * a.K + tid];
        nt += nb;
    }
    double mean = nt > 0.0 ? s / nt : 0.0, n = nt;
    if (a.accumulate) {
        if (nt == 0.0) return;
        if (na > 0.0) {
            const double ma = a.mean[tid], nn = na + nt;
            mean = ma + (mean - ma) * nt / nn;
            n = nn;
        }
    }
    a.mean[tid] = mean;
    if (tid == 0) a.count[0] = n;
}

// info = 0: chol written. info = j + 1: pivot j was not finite and > 0 (n < 2: j = 0), chol untouched
__global__ __launch_bounds__(64) void k_dense_factor(int32_t K, const double* count, const double* m2, int32_t regularize, double* chol, int32_t* info) {
    __shared__ double A[MAXK * (MAXK + 1) / 2];
    const int i = threadIdx.x;                              // the lane's row
    const double n = count[0];
    if (!(n >= 2.0)) {
        if (i == 0) info[0] = 1;
        return;
    }
    const int ri = i * (i + 1) >> 1;
    if (i < K)
        for (int j = 0; j <= i; ++j) {
            double v = m2[ri + j] / (n - 1.0);
            if (regularize) v = i == j ? (n / (n + 5.0)) * v + 1e-3 * 5.0 / (n + 5.0) : (n / (n + 5.0)) * v;
            A[ri + j] = v;
        }
    __syncthreads();
    for (int j = 0; j < K; ++j) {
        const int rj = j * (j + 1) >> 1;
        double s = 0.0;
        if (i >= j && i < K) {
            s = A[ri + j];
            for (int k = 0; k < j; ++k) s -= A[ri + k] * A[rj + k];
        }
        const double d = __shfl(s, j);
        if (!(isfinite(d) && d > 0.0)) {                    // the whole wave
            if (i == 0) info[0] = j + 1;
            return;
        }
        const double l = sqrt(d);
        if (i >= j && i < K) A[ri + j] = i == j ? l : s / l;
        __syncthreads();
    }
    if (i < K)
        for (int j = 0; j <= i; ++j) chol[ri + j] = A[ri + j];
    if (i == 0) info[0] = 0;
}

__global__ __launch_bounds__(TPB) void k_dense_apply(int64_t n, int64_t ld, int32_t D, const double* chol, int32_t transpose, const double* x, double* out) {
    const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (w >= n) return;
    const auto put = [&](int d, double v) { out[(int64_t)d * ld + w] = v; };
    if (transpose) metric_lower_t(chol, D, x, ld, w, put);
    else metric_lower(chol, D, x, ld, w, put);
}

inline int check_k(octo_draws* h, const char* who, int32_t K) {
    return K >= 1 && K <= OCTO_DRAWS_DENSE_MAX_D ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": K must be 1 ... OCTO_DRAWS_DENSE_MAX_D");
}

}  // namespace

extern "C" {

int32_t octo_draws_cov_device(octo_draws* h, int64_t W, int64_t ld, int32_t K, const double* d_x, int32_t accumulate, double* d_count, double* d_mean,
                              double* d_m2, void* hip_stream) {
    const char* who = "octo_draws_cov_device";
    if (!h) return OCTO_EINVAL;
    if ((!d_x && W != 0) || !d_count || !d_mean || !d_m2) return fail(h, OCTO_EINVAL, std::string(who) + ": d_x, d_count, d_mean and d_m2 are required");
    if (int rc = check_k(h, who, K)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_COV_CHAINS, "2^24")) return rc;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t nblk = (W + TPB - 1) / TPB;
    CovArgs a;
    a.x = d_x; a.W = W; a.ld = ld; a.K = K;
    if (int rc = grow_to(h, h->d_mom, h->cap_mom, a.p, cov_partials, nblk, (int64_t)K)) return rc;
    if (nblk) hipLaunchKernelGGL(k_dense_cov_partials, dim3((unsigned)nblk), dim3(TPB), 0, st, a);
    CovMergeArgs m;
    m.p = a.p; m.nblk = nblk; m.K = K; m.accumulate = accumulate ? 1 : 0; m.count = d_count; m.mean = d_mean; m.m2 = d_m2;
    hipLaunchKernelGGL(k_dense_cov_merge, dim3(1), dim3(TPB), 0, st, m);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_metric_dense_device(octo_draws* h, int32_t K, const double* d_count, const double* d_m2, int32_t regularize, double* d_chol,
                                       int32_t* d_info, void* hip_stream) {
    const char* who = "octo_draws_metric_dense_device";
    if (!h) return OCTO_EINVAL;
    if (!d_count || !d_m2 || !d_chol || !d_info) return fail(h, OCTO_EINVAL, std::string(who) + ": every array is required");
    if (int rc = check_k(h, who, K)) return rc;
    OCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_dense_factor, dim3(1), dim3(64), 0, stream_of(h, hip_stream), K, d_count, d_m2, regularize ? 1 : 0, d_chol, d_info);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_metric_apply_device(octo_draws* h, int64_t n, int64_t ld, const double* d_chol, int32_t transpose, const double* d_x, double* d_out,
                                       void* hip_stream) {
    const char* who = "octo_draws_metric_apply_device";
    if (!h) return OCTO_EINVAL;
    if (h->D > OCTO_DRAWS_DENSE_MAX_D) return fail(h, OCTO_EINVAL, std::string(who) + ": D > OCTO_DRAWS_DENSE_MAX_D");
    if (int rc = check_chains(h, who, n, ld, MAX_CHAINS, "2^30")) return rc;
    if (n == 0) return OCTO_OK;
    if (!d_chol || !d_x || !d_out) return fail(h, OCTO_EINVAL, std::string(who) + ": d_chol, d_x and d_out are required");
    OCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_dense_apply, grid_of(n), dim3(TPB), 0, stream_of(h, hip_stream), n, ld, (int32_t)h->D, d_chol, transpose ? 1 : 0, d_x, d_out);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_use_metric(octo_draws* h, const double* d_chol) {
    if (!h) return OCTO_EINVAL;
    if (d_chol && h->D > OCTO_DRAWS_DENSE_MAX_D) return fail(h, OCTO_EINVAL, "octo_draws_use_metric: D > OCTO_DRAWS_DENSE_MAX_D");
    h->d_metric = d_chol;
    return OCTO_OK;
}

}  // extern "C"
