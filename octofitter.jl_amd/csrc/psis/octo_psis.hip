// octo_psis.hip — liboctofitter_hip_psis.so: PSIS-LOO of a pointwise log-likelihood matrix on the device (include/octofitter_hip_psis.h,
// which states the algorithm). It includes nothing of the main library's sources and links nothing of it.
//
//   k_psis   one block of 256 threads per row (datum). Every pass walks the row coalesced, lane = sample index mod 256, and re-reads it
//            from L2 (a row of 1e4 samples is 80 KB):
//              (a) n, min and max of the finite entries;
//              (b) the (M+1)-th largest x by an exact radix select on u = bits(ll − min ll) — x = −(ll − min ll) <= 0, so the bits of −x
//                  order as unsigned integers and the k-th largest x is the k-th smallest u — 8-bit digits, one LDS histogram per digit
//                  filled with INTEGER LDS atomics (counts do not depend on the order of arrival) and scanned by the block; as soon as
//                  the entries that share the digits chosen so far fit the sort buffer they are gathered into it, and the remaining
//                  digits are read from LDS: three walks over a row of 1e4 samples instead of eight, two over one of <= 4096;
//              (c) the tail {u < u_c} into LDS as (~u, sample index); the slot comes from an integer LDS counter: the order of arrival is
//                  free because (d) is a total order;
//              (d) bitonic sort of the tail in LDS, ascending by (~u, index) = ascending by (x, index), padded to a power of two;
//              (e) the Zhang–Stephens fit: grid points dealt to the waves, tail entries to the lanes; the m² softmax on the first m
//                  threads; the smoothed tail back into the sort buffer;
//              (f) two closing passes (the log-sum-exp of the weights; then elpd, ess and the weights themselves): non-tail entries from
//                  memory, tail entries from LDS.
//            Every floating-point sum is a lane's strided partial, a wave butterfly, then the four waves in wave order: a result depends
//            on the row's values alone, not on R, the row's position, ld or the entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "octo_companion_host.h"
#include "octofitter_hip_psis.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVE = 64;
constexpr int NWV = TPB / WAVE;
constexpr int MAX_TAIL = 4096;            // the sort buffer: 4096 × (8 + 4) bytes = 48 KB of LDS, three blocks per CU
constexpr int MAX_GRID = 30 + 64;         // m = 30 + ⌊√tail_len⌋
constexpr int NSTAT = OCTO_PSIS_N_STATS;
constexpr double LOG_DBL_MIN = -708.3964185322641;      // log(DBL_MIN)
constexpr double EPS = 2.220446049250313e-16;           // 2⁻⁵²

// M(n) = ceil(min(n/5, 3·√n)). ceil(n/5) is integer arithmetic; ceil(3·√n) is the smallest t with t² >= 9n, to which the rounded
// double expression is corrected (for the n served the two agree: 3·√n is an integer or at least 1/(2t) away from one).
__host__ __device__ inline int64_t tail_len(int64_t n) {
    if (n <= 0) return 0;
    int64_t t = (int64_t)ceil(3.0 * sqrt((double)n));
    while (t * t < 9 * n) ++t;
    while (t > 0 && (t - 1) * (t - 1) >= 9 * n) --t;
    const int64_t f = (n + 4) / 5;
    return f < t ? f : t;
}

__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ double bits_d(unsigned long long u) { return __longlong_as_double((long long)u); }

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, WAVE);      // both partners add the same pair: every lane ends with the same bits
    return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m, WAVE));
    return x;
}

struct Shared {
    unsigned long long key[MAX_TAIL];      // ~u of the tail; after the sort y_i, then the smoothed x_i (as doubles)
    int idx[MAX_TAIL];
    unsigned int hist[TPB];
    double red[NWV];
    double grid_b[MAX_GRID], grid_l[MAX_GRID], grid_w[MAX_GRID];
    unsigned int wsum[NWV];
    unsigned int sel_digit, sel_k, sel_count;
    int count;
};

// The block's sum in wave order, the same bits in every thread. Two barriers: `red` is free again on return.
__device__ __forceinline__ double block_sum(double x, double* red) {
    x = wave_sum(x);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = x;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < NWV; ++k) s += red[k];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double block_max(double x, double* red) {
    x = wave_max(x);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = x;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int k = 1; k < NWV; ++k) s = fmax(s, red[k]);
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(TPB) void k_psis(const double* __restrict__ ll, int64_t ld, int64_t S, int64_t R, double* __restrict__ out,
                                              double* __restrict__ lw, int64_t ld_w) {
    __shared__ Shared sh;
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
    const double* row = ll + r * ld;
    double* lwrow = lw ? lw + r * ld_w : nullptr;
    const int n_s = (int)S;      // S <= octo_psis_max_samples() < 2^31

    // (a) the finite entries: count, minimum, maximum
    double cnt = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int s = tid; s < n_s; s += TPB) {
        const double v = row[s];
        if (isfinite(v)) { cnt += 1.0; mn = fmin(mn, v); mx = fmax(mx, v); }
    }
    const int n = (int)block_sum(cnt, sh.red);      // whole numbers below 2^53: exact in any order
    const double llmin = -block_max(-mn, sh.red), llmax = block_max(mx, sh.red);
    if (n == 0) {      // block-uniform
        if (tid == 0) {
            out[OCTO_PSIS_N * R + r] = 0.0;
            for (int k = 1; k < NSTAT; ++k) out[k * R + r] = NAN;
        }
        if (lwrow) for (int s = tid; s < n_s; s += TPB) lwrow[s] = -INFINITY;
        return;
    }

    // (b) the cut-off: u_c = min(the (M+1)-th smallest u, bits(−log DBL_MIN)); no tail when n <= M (u_c = 0: no u lies below it)
    const int M = (int)tail_len(n);
    unsigned long long uc = 0;
    if (n > M) {
        unsigned long long prefix = 0;
        unsigned int k = (unsigned int)M + 1u;
        int ncand = -1;      // >= 0: the candidates (every entry that shares the digits chosen so far, and possibly more) are sh.key[0 .. ncand)
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            // Once the candidates fit the sort buffer (free until (c)) they are gathered there — in any order: the counts below do not
            // depend on it — and the remaining digits are read from LDS, not from the row.
            if (ncand < 0 && (pass == 0 ? n <= MAX_TAIL : sh.sel_count <= (unsigned int)MAX_TAIL)) {
                if (tid == 0) sh.count = 0;
                __syncthreads();
                for (int s = tid; s < n_s; s += TPB) {
                    const double v = row[s];
                    if (isfinite(v)) {
                        const unsigned long long u = dbits(v - llmin);
                        if (pass == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))) {
                            const int pos = atomicAdd(&sh.count, 1);
                            if (pos < MAX_TAIL) sh.key[pos] = u;
                        }
                    }
                }
                __syncthreads();
                ncand = sh.count < MAX_TAIL ? sh.count : MAX_TAIL;
            }
            sh.hist[tid] = 0u;
            __syncthreads();
            if (ncand < 0) {
                for (int s = tid; s < n_s; s += TPB) {
                    const double v = row[s];
                    if (isfinite(v)) {
                        const unsigned long long u = dbits(v - llmin);
                        if (pass == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh.hist[(unsigned int)(u >> shift) & 255u], 1u);
                    }
                }
            } else {
                for (int i = tid; i < ncand; i += TPB) {
                    const unsigned long long u = sh.key[i];
                    if (pass == 0 || (u >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh.hist[(unsigned int)(u >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            // inclusive scan of the 256 counts in thread order; the digit whose range holds k
            unsigned int x = sh.hist[tid];
            const unsigned int c = x;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const unsigned int y = __shfl_up(x, d, WAVE);
                if (lane >= d) x += y;
            }
            if (lane == WAVE - 1) sh.wsum[wv] = x;
            __syncthreads();
            unsigned int off = 0;
            for (int q = 0; q < wv; ++q) off += sh.wsum[q];
            const unsigned int incl = x + off, excl = incl - c;
            if (excl < k && k <= incl) { sh.sel_digit = (unsigned int)tid; sh.sel_k = k - excl; sh.sel_count = c; }
            __syncthreads();
            prefix |= (unsigned long long)sh.sel_digit << shift;
            k = sh.sel_k;
        }
        const unsigned long long clamp = dbits(-LOG_DBL_MIN);
        uc = prefix < clamp ? prefix : clamp;
    }
    const double xc = -bits_d(uc);

    // (c) the tail into LDS: at most M <= MAX_TAIL entries lie strictly below the (M+1)-th smallest u
    if (tid == 0) sh.count = 0;
    __syncthreads();
    if (uc != 0)
        for (int s = tid; s < n_s; s += TPB) {
            const double v = row[s];
            if (isfinite(v)) {
                const unsigned long long u = dbits(v - llmin);
                if (u < uc) {
                    const int pos = atomicAdd(&sh.count, 1);
                    if (pos < MAX_TAIL) { sh.key[pos] = ~u; sh.idx[pos] = s; }
                }
            }
        }
    __syncthreads();
    const int tl = sh.count < MAX_TAIL ? sh.count : MAX_TAIL;

    double khat = INFINITY;
    bool smoothed = false;
    double tail_max = -INFINITY;
    if (tl > 4) {      // block-uniform
        // (d) bitonic sort, ascending by (~u, index)
        int P = 8;
        while (P < tl) P <<= 1;
        for (int i = tl + tid; i < P; i += TPB) { sh.key[i] = ~0ull; sh.idx[i] = 0x7fffffff; }
        __syncthreads();
        for (int k2 = 2; k2 <= P; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P / 2; t += TPB) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const unsigned long long ka = sh.key[i], kb = sh.key[l];
                    const int ia = sh.idx[i], ib = sh.idx[l];
                    const bool gt = ka > kb || (ka == kb && ia > ib);
                    if (gt == ((i & k2) == 0)) { sh.key[i] = kb; sh.key[l] = ka; sh.idx[i] = ib; sh.idx[l] = ia; }
                }
                __syncthreads();
            }
        // y_i = exp(x_i) − exp(x_c), in place
        const double exc = exp(xc);
        for (int i = tid; i < tl; i += TPB) {
            const double x = -bits_d(~sh.key[i]);
            sh.key[i] = dbits(exp(x) - exc);
        }
        __syncthreads();

        // (e) the fit
        int rt = (int)sqrt((double)tl);
        while (rt * rt > tl) --rt;
        while ((rt + 1) * (rt + 1) <= tl) ++rt;
        const int m = 30 + rt;
        const double dtl = (double)tl;
        const double yq = bits_d(sh.key[(tl + 2) / 4 - 1]), yt = bits_d(sh.key[tl - 1]);
        for (int j = wv; j < m; j += NWV) {
            const double bj = (1.0 - sqrt((double)m / ((double)(j + 1) - 0.5))) / (3.0 * yq) + 1.0 / yt;
            double acc = 0.0;
            for (int i = lane; i < tl; i += WAVE) acc += log1p(-bj * bits_d(sh.key[i]));
            const double kj = wave_sum(acc) / dtl;
            if (lane == 0) { sh.grid_b[j] = bj; sh.grid_l[j] = dtl * (log(-bj / kj) - kj - 1.0); }
        }
        __syncthreads();
        if (tid < m) {
            const double lt = sh.grid_l[tid];
            double s = 0.0;
            for (int l = 0; l < m; ++l) s += exp(sh.grid_l[l] - lt);
            const double w = 1.0 / s;
            sh.grid_w[tid] = w < 10.0 * EPS ? 0.0 : w;
        }
        __syncthreads();
        double sw = 0.0;
        for (int l = 0; l < m; ++l) sw += sh.grid_w[l];
        double b = 0.0;
        for (int l = 0; l < m; ++l) b += (sh.grid_w[l] / sw) * sh.grid_b[l];
        double acc = 0.0;
        for (int i = tid; i < tl; i += TPB) acc += log1p(-b * bits_d(sh.key[i]));
        const double kk = block_sum(acc, sh.red) / dtl;
        const double sigma = -kk / b;
        khat = (dtl * kk + 5.0) / (dtl + 10.0);
        if (isfinite(khat)) {
            smoothed = true;
            double tm = -INFINITY;
            for (int i = tid; i < tl; i += TPB) {
                const double p = ((double)i + 0.5) / dtl;
                const double l1 = log1p(-p);
                const double q = khat == 0.0 ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
                const double xs = fmin(log(q + exc), 0.0);
                sh.key[i] = dbits(xs);
                tm = fmax(tm, xs);
            }
            tail_max = block_max(tm, sh.red);      // its barriers also publish the smoothed tail
        }
    }

    // (f) closing pass 1: Σ exp(x − shift), Σ exp(ll − max ll), max(ll + x)
    const double shift = smoothed ? fmax(tail_max, xc) : 0.0;
    double a1 = 0.0, lp = 0.0, tmx = -INFINITY;
    for (int s = tid; s < n_s; s += TPB) {
        const double v = row[s];
        if (isfinite(v)) {
            const double d = v - llmin;
            lp += exp(v - llmax);
            if (!(smoothed && dbits(d) < uc)) {
                const double x = -d;
                a1 += exp(x - shift);
                tmx = fmax(tmx, v + x);
            }
        }
    }
    if (smoothed)
        for (int i = tid; i < tl; i += TPB) {
            const double x = bits_d(sh.key[i]), v = row[sh.idx[i]];
            a1 += exp(x - shift);
            tmx = fmax(tmx, v + x);
        }
    const double lse = shift + log(block_sum(a1, sh.red));
    const double lppd = llmax + log(block_sum(lp, sh.red)) - log((double)n);
    const double shift2 = block_max(tmx, sh.red) - lse;
    // closing pass 2: the weights, Σ exp(ll + lw − shift2), Σ exp(2·lw)
    double e1 = 0.0, e2 = 0.0;
    for (int s = tid; s < n_s; s += TPB) {
        const double v = row[s];
        if (isfinite(v)) {
            const double d = v - llmin;
            if (!(smoothed && dbits(d) < uc)) {
                const double w = -d - lse;
                e1 += exp((v + w) - shift2);
                e2 += exp(2.0 * w);
                if (lwrow) lwrow[s] = w;
            }
        } else if (lwrow) {
            lwrow[s] = -INFINITY;
        }
    }
    if (smoothed)
        for (int i = tid; i < tl; i += TPB) {
            const int s = sh.idx[i];
            const double w = bits_d(sh.key[i]) - lse, v = row[s];
            e1 += exp((v + w) - shift2);
            e2 += exp(2.0 * w);
            if (lwrow) lwrow[s] = w;
        }
    const double elpd = shift2 + log(block_sum(e1, sh.red));
    const double ess = 1.0 / block_sum(e2, sh.red);
    if (tid == 0) {
        out[OCTO_PSIS_N * R + r] = (double)n;
        out[OCTO_PSIS_TAIL_LEN * R + r] = (double)tl;
        out[OCTO_PSIS_PARETO_K * R + r] = khat;
        out[OCTO_PSIS_ELPD_LOO * R + r] = elpd;
        out[OCTO_PSIS_LPPD * R + r] = lppd;
        out[OCTO_PSIS_ESS * R + r] = ess;
    }
}

}  // namespace

struct octo_psis : CompanionStaged {
    // host-buffer call: matrix chunk, weights chunk, result chunk (grown on demand)
    double* d_mat = nullptr; int64_t cap_mat = 0;
    double* d_lw = nullptr; int64_t cap_lw = 0;
    double* d_out = nullptr; int64_t cap_out = 0;
    int64_t mat_bytes = (int64_t)64 << 20;
};

namespace {

int check_args(octo_psis* h, const char* who, const void* ll, int64_t ld, int64_t R, int64_t S, const void* out, const void* lw, int64_t ld_w) {
    if (R < 0 || S < 1 || ld < S) return fail(h, OCTO_EINVAL, std::string(who) + ": need R >= 0 and 1 <= S <= ld");
    if (lw && ld_w < S) return fail(h, OCTO_EINVAL, std::string(who) + ": need S <= ld_w");
    if (R > 0 && (!ll || !out)) return fail(h, OCTO_EINVAL, std::string(who) + ": null matrix or output");
    if (R > 0x7fffffff) return fail(h, OCTO_EINVAL, std::string(who) + ": more than 2^31 - 1 rows");
    if (S > octo_psis_max_samples())
        return fail(h, OCTO_ENOTSUP, std::string(who) + ": S = " + std::to_string(S) + " is above octo_psis_max_samples() = " + std::to_string(octo_psis_max_samples()));
    return OCTO_OK;
}

// nr rows of S doubles between a host array (leading dimension ld_h) and a packed device array, through the pinned staging buffer: whole
// rows per pass where a row fits it, pieces of a row where it does not
int staged_rows(octo_psis* h, double* host, int64_t ld_h, double* dev, int64_t nr, int64_t S, bool to_device) {
    const auto kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    const int64_t piece = std::min(S, h->cap_stage), rps = std::max<int64_t>(h->cap_stage / S, 1);
    for (int64_t r0 = 0; r0 < nr; r0 += rps) {
        const int64_t k = std::min(rps, nr - r0);
        for (int64_t at = 0; at < S; at += piece) {      // one pass unless a row is larger than the staging buffer (then k = 1)
            const int64_t w = std::min(piece, S - at);
            if (to_device)
                for (int64_t r = 0; r < k; ++r) std::memcpy(h->h_stage + r * w, host + (r0 + r) * ld_h + at, sizeof(double) * (size_t)w);
            if (w == S) OCHK(h, hipMemcpyAsync(to_device ? dev + r0 * S : h->h_stage, to_device ? h->h_stage : dev + r0 * S, sizeof(double) * (size_t)(k * S), kind, h->stream));
            else OCHK(h, hipMemcpyAsync(to_device ? dev + r0 * S + at : h->h_stage, to_device ? h->h_stage : dev + r0 * S + at, sizeof(double) * (size_t)w, kind, h->stream));
            OCHK(h, hipStreamSynchronize(h->stream));
            if (!to_device)
                for (int64_t r = 0; r < k; ++r) std::memcpy(host + (r0 + r) * ld_h + at, h->h_stage + r * w, sizeof(double) * (size_t)w);
        }
    }
    return OCTO_OK;
}

}  // namespace

extern "C" {

int64_t octo_psis_tail_len(int64_t n) { return tail_len(n); }

int64_t octo_psis_max_samples(void) {
    static const int64_t s_max = [] {
        int64_t s = ((int64_t)MAX_TAIL * MAX_TAIL) / 9 + 8;      // 3·√S <= 4096 up to S = 4096²/9
        while (tail_len(s) > MAX_TAIL) --s;
        return s;
    }();
    return s_max;
}

int32_t octo_psis_create(int32_t device_id, octo_psis** out) {
    const std::string fn = "octo_psis_create: ";
    if (!out) return fail(nullptr, OCTO_EINVAL, fn + "null out pointer");
    *out = nullptr;
    octo_psis* h;
    { int rc = open_device(device_id, fn, h); if (rc) return rc; }
    h->mat_bytes = env_bytes("OCTO_PSIS_MATRIX_BYTES", h->mat_bytes);
    h->stage_bytes = env_bytes("OCTO_PSIS_STAGE_BYTES", h->stage_bytes);
    *out = h;
    return OCTO_OK;
}

int32_t octo_psis_destroy(octo_psis* h) {
    if (!h) return OCTO_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    (void)hipFree(h->d_mat); (void)hipFree(h->d_lw); (void)hipFree(h->d_out);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    delete h;
    return OCTO_OK;
}

const char* octo_psis_last_error(const octo_psis* h) { return last_error(h); }

int32_t octo_psis_sync(octo_psis* h) { return sync_handle(h); }

int32_t octo_psis_loo_device(octo_psis* h, const double* d_ll, int64_t ld, int64_t R, int64_t S, double* d_out, double* d_lw, int64_t ld_w,
                             void* hip_stream) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_args(h, "octo_psis_loo_device", d_ll, ld, R, S, d_out, d_lw, ld_w); if (rc) return rc; }
    if (R == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    hipLaunchKernelGGL(k_psis, dim3((unsigned)R), dim3(TPB), 0, st, d_ll, ld, S, R, d_out, d_lw, ld_w);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_psis_loo(octo_psis* h, const double* ll, int64_t ld, int64_t R, int64_t S, double* out, double* lw, int64_t ld_w) {
    if (!h) return OCTO_EINVAL;
    { int rc = check_args(h, "octo_psis_loo", ll, ld, R, S, out, lw, ld_w); if (rc) return rc; }
    if (R == 0) return OCTO_OK;
    const int64_t cap_rows = h->mat_bytes / (int64_t)(sizeof(double) * (size_t)S);
    if (cap_rows < 1)
        return fail(h, OCTO_ENOMEM, "octo_psis_loo: one row of S = " + std::to_string(S) + " samples (" + std::to_string(S * 8) + " bytes) is larger than the device buffer of " +
                                        std::to_string(h->mat_bytes) + " bytes (OCTO_PSIS_MATRIX_BYTES)");
    OCHK(h, hipSetDevice(h->device));
    const int64_t Rc = std::min(cap_rows, R);      // rows per chunk
    { int rc = grow(h, h->d_mat, h->cap_mat, Rc * S); if (rc) return rc; }
    if (lw) { int rc = grow(h, h->d_lw, h->cap_lw, Rc * S); if (rc) return rc; }
    { int rc = grow(h, h->d_out, h->cap_out, Rc * NSTAT); if (rc) return rc; }
    { int rc = ensure_stage(h, std::max<int64_t>(h->stage_bytes / (int64_t)sizeof(double), NSTAT)); if (rc) return rc; }
    for (int64_t r0 = 0; r0 < R; r0 += Rc) {
        const int64_t nr = std::min(Rc, R - r0);
        { int rc = staged_rows(h, const_cast<double*>(ll) + r0 * ld, ld, h->d_mat, nr, S, true); if (rc) return rc; }
        { int rc = octo_psis_loo_device(h, h->d_mat, S, nr, S, h->d_out, lw ? h->d_lw : nullptr, S, OCTO_STREAM_CTX); if (rc) return rc; }
        { int rc = staged_rows(h, out + r0, R, h->d_out, NSTAT, nr, false); if (rc) return rc; }      // [NSTAT][nr] into [NSTAT][R] at column r0
        if (lw) { int rc = staged_rows(h, lw + r0 * ld_w, ld_w, h->d_lw, nr, S, false); if (rc) return rc; }
    }
    return OCTO_OK;
}

}  // extern "C"
