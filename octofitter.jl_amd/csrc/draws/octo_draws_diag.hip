// octo_draws_diag.hip — the convergence diagnostics of stored draws in liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states them):
// rank-normalised split-R̂, bulk and tail ESS, the basic pair and three quantiles of every row of a cube [n][K][W]. Lane = split chain wherever
// a chain is walked, lane = draw in the sort and the rank step. No floating-point atomic: every sum has a fixed order.
//
//   k_diag_keys          the used draws of a row (fold: their |x − median|) into its P keys, +Inf behind the S; flags a non-finite draw.
//   k_diag_sort_local    one block = 2048 keys in LDS: every stage up to 2048 of the bitonic network, or the strides below 2048 of a later stage.
//   k_diag_sort_global   one compare-exchange per thread at a stride of 2048 or more.
//   k_diag_quant         K threads: the three type-7 quantiles and the row's validity.
//   k_diag_rank          one thread per used draw: lower and upper bound in the sorted keys, the average rank, z.
//   k_diag_moments       one thread per split chain and (row, quantity): its mean and variance over time, in index order.
//   k_diag_acov          one thread per split chain, grid = (chain tiles × lag blocks) × (row, quantity): 16 lags at once over a sliding window
//                        of 16 centred values in registers (both loops unrolled: no private array is indexed at run time), then the block's
//                        sums per lag: a butterfly over the wave, the four waves in wave order.
//   k_diag_finish        one block per row, one wave per quantity: the cross-chain means in the documented order, ρ_t of every lag, then one
//                        lane runs Geyer's truncation on them (in LDS up to 1024 lags, in the work array beyond).
// A diagnosis is 8 launches, two sorts (a local launch, then for each stage above 2048 its global passes and a local launch) and one 4·K-byte memset.
#include "octo_draws_common.h"

namespace {

constexpr int WAVES = TPB / 64;
constexpr int SORT_BLK = 2048;                 // keys a block sorts in LDS
constexpr int LAGS = 16;                       // lags of one launch block = the window
constexpr int LDS_T = 1024;                    // lags a wave of k_diag_finish holds in LDS
constexpr int NQ = 5, NQ_ACOV = 4;             // z, x, 1[x <= q05], 1[x <= q95], z_folded; the first four at every lag
constexpr int64_t MAX_USED = (int64_t)1 << 24;

struct Shape {
    int64_t n, W, ld, ls;
    int64_t N, M, S, P, T, nblk;
    int32_t K;
};

inline Shape shape_of(int64_t n, int64_t W, int64_t ld, int64_t ls, int32_t K) {
    Shape s;
    s.n = n; s.W = W; s.ld = ld; s.ls = ls; s.K = K;
    s.N = n / 2; s.M = 2 * W; s.S = s.M * s.N;
    s.P = SORT_BLK;
    while (s.P < s.S) s.P <<= 1;
    s.T = (s.N + LAGS - 1) / LAGS * LAGS;
    s.nblk = (s.M + TPB - 1) / TPB;
    return s;
}

inline bool shape_ok(int64_t n, int64_t W, int32_t K) { return n >= 8 && W >= 1 && K >= 1 && K <= OCTO_DRAWS_MAX_GROUPS; }
inline bool shape_supported(int64_t n, int64_t W) { return W <= MAX_USED && n / 2 <= MAX_USED && 2 * (n / 2) * W <= MAX_USED; }

// element (i, m) of row k: draw i of split chain m = h·W + w is sample h·(n − N) + i of chain w
__device__ __forceinline__ int64_t x_offset(const Shape& s, int k, int64_t m, int64_t i) {
    const int64_t h = m >= s.W ? 1 : 0;
    return (h * (s.n - s.N) + i) * s.ls + (int64_t)k * s.ld + (m - h * s.W);
}

struct KeyArgs {
    const double* x;
    Shape s;
    DiagWork w;
    int32_t fold;
};

// blockIdx.y = the row; key j = i·M + m
__global__ __launch_bounds__(TPB) void k_diag_keys(KeyArgs a) {
    const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int k = blockIdx.y;
    if (j >= a.s.P) return;
    double v = INFINITY;
    if (j < a.s.S) {
        const int64_t i = j / a.s.M, m = j - i * a.s.M;
        v = a.x[x_offset(a.s, k, m, i)];
        if (a.fold) v = fabs(v - a.w.q[a.s.K + k]);
        else if (!isfinite(v)) a.w.bad[k] = 1;      // every writer stores the same value
    }
    (a.fold ? a.w.fkeys : a.w.keys)[(int64_t)k * a.s.P + j] = v;
}

// pair p of a stride j (a power of two): the lower index has bit j clear
__device__ __forceinline__ int64_t pair_low(int64_t p, int64_t j) { return ((p & ~(j - 1)) << 1) | (p & (j - 1)); }

// stage = 0: every stage 2 … SORT_BLK of the network on the block's keys. Otherwise the strides SORT_BLK/2 … 1 of that stage (> SORT_BLK).
// Element g of the row sorts ascending in stage kk iff g & kk is 0.
__global__ __launch_bounds__(TPB) void k_diag_sort_local(double* keys, int64_t P, int64_t stage) {
    __shared__ double s[SORT_BLK];
    const int tid = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * SORT_BLK;
    double* row = keys + (int64_t)blockIdx.y * P + first;
#pragma unroll
    for (int e = 0; e < SORT_BLK / TPB; ++e) s[tid + e * TPB] = row[tid + e * TPB];
    __syncthreads();
    for (int64_t kk = stage ? stage : 2; kk <= (stage ? stage : SORT_BLK); kk <<= 1) {
        for (int j = (int)(kk < SORT_BLK ? kk >> 1 : SORT_BLK >> 1); j >= 1; j >>= 1) {
#pragma unroll
            for (int e = 0; e < SORT_BLK / 2 / TPB; ++e) {
                const int lo = (int)pair_low(tid + e * TPB, j), hi = lo | j;
                const bool up = ((first + lo) & kk) == 0;
                const double u = s[lo], v = s[hi];
                if ((u > v) == up) { s[lo] = v; s[hi] = u; }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int e = 0; e < SORT_BLK / TPB; ++e) row[tid + e * TPB] = s[tid + e * TPB];
}

__global__ __launch_bounds__(TPB) void k_diag_sort_global(double* keys, int64_t P, int64_t kk, int64_t j) {
    const int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (p >= P / 2) return;
    double* row = keys + (int64_t)blockIdx.y * P;
    const int64_t lo = pair_low(p, j), hi = lo | j;
    const bool up = (lo & kk) == 0;
    const double u = row[lo], v = row[hi];
    if ((u > v) == up) { row[lo] = v; row[hi] = u; }
}

// q_p = s[lo] + (h − lo)·(s[lo+1] − s[lo]), every operation rounded by itself
__device__ __forceinline__ double quantile7(const double* s, int64_t S, double p) {
    const double h = (double)(S - 1) * p, fl = floor(h);
    const int64_t lo = (int64_t)fl, up = lo + 1 < S ? lo + 1 : S - 1;
    return __dadd_rn(s[lo], __dmul_rn(h - fl, __dadd_rn(s[up], -s[lo])));
}

__global__ __launch_bounds__(TPB) void k_diag_quant(Shape s, DiagWork w) {
    const int k = threadIdx.x;
    if (k >= s.K) return;
    const double* key = w.keys + (int64_t)k * s.P;
    w.ok[k] = !w.bad[k] && key[0] < key[s.S - 1] ? 1 : 0;
    w.q[k] = quantile7(key, s.S, 0.05);
    w.q[s.K + k] = quantile7(key, s.S, 0.5);
    w.q[2 * s.K + k] = quantile7(key, s.S, 0.95);
}

struct RankArgs {
    const double* x;
    Shape s;
    DiagWork w;
    int32_t fold, user;      // user: the outputs are on the strides of x; otherwise [K][N][M]
    double *rank, *z;
};

__global__ __launch_bounds__(TPB) void k_diag_rank(RankArgs a) {
    const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int k = blockIdx.y;
    const int64_t S = a.s.S;
    if (j >= S) return;
    const int64_t i = j / a.s.M, m = j - i * a.s.M, ox = x_offset(a.s, k, m, i);
    double v = a.x[ox];
    if (a.fold) v = fabs(v - a.w.q[a.s.K + k]);
    const double* key = (a.fold ? a.w.fkeys : a.w.keys) + (int64_t)k * a.s.P;
    int64_t lo = 0, hi = S;                 // #{s < v}
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key[mid] < v) lo = mid + 1; else hi = mid;
    }
    int64_t b = 1;                          // #{s <= v}: ties are short, so gallop from lo before bisecting
    while (lo + b < S && key[lo + b] <= v) b <<= 1;
    int64_t ub = lo + (b >> 1);
    hi = lo + b < S ? lo + b : S;
    while (ub < hi) {
        const int64_t mid = (ub + hi) >> 1;
        if (key[mid] <= v) ub = mid + 1; else hi = mid;
    }
    const double r = a.w.ok[k] ? (double)lo + 0.5 * (double)(ub - lo + 1) : NAN;
    const int64_t o = a.user ? ox : (int64_t)k * S + j;
    if (a.rank) a.rank[o] = r;
    if (a.z) a.z[o] = normcdfinv((r - 0.375) / ((double)S + 0.25));
}

struct ChainArgs {
    const double* x;
    Shape s;
    DiagWork w;
};

// draw i of one split chain of one quantity: p[i·stride], or whether it is <= thr
struct Src {
    const double* p;
    int64_t stride;
    double thr;
    int ind;
};

__device__ __forceinline__ Src source(const ChainArgs& a, int q, int k, int64_t m) {
    Src s;
    s.thr = 0.0; s.ind = 0;
    if (q == 0 || q == 4) {
        s.p = (q == 0 ? a.w.z : a.w.zf) + (int64_t)k * a.s.S + m;
        s.stride = a.s.M;
    } else {
        s.p = a.x + x_offset(a.s, k, m, 0);
        s.stride = a.s.ls;
        if (q >= 2) { s.ind = 1; s.thr = a.w.q[(q == 2 ? 0 : 2 * a.s.K) + k]; }
    }
    return s;
}

__device__ __forceinline__ double at(const Src& s, int64_t i) {
    const double v = s.p[i * s.stride];
    return s.ind ? (v <= s.thr ? 1.0 : 0.0) : v;
}

// blockIdx.y = row·5 + quantity
__global__ __launch_bounds__(TPB) void k_diag_moments(ChainArgs a) {
    const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (m >= a.s.M) return;
    const int k = blockIdx.y / NQ, q = blockIdx.y % NQ;
    const Src s = source(a, q, k, m);
    const int64_t N = a.s.N;
    double sum = 0.0;
    for (int64_t i = 0; i < N; ++i) sum += at(s, i);
    const double mu = sum / (double)N;
    double ss = 0.0;
    for (int64_t i = 0; i < N; ++i) {
        const double d = at(s, i) - mu;
        ss += d * d;
    }
    const int64_t o = (int64_t)blockIdx.y * a.s.M + m;
    a.w.mu[o] = mu;
    a.w.var[o] = ss / (double)N * (double)N / (double)(N - 1);
}

// blockIdx.x = lag block·nblk + chain tile · blockIdx.y = row·4 + quantity
__global__ __launch_bounds__(TPB) void k_diag_acov(ChainArgs a) {
    __shared__ double s_red[WAVES][LAGS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t tile = blockIdx.x % a.s.nblk, t0 = (int64_t)(blockIdx.x / a.s.nblk) * LAGS;
    const int k = blockIdx.y / NQ_ACOV, q = blockIdx.y % NQ_ACOV;
    const int64_t m = tile * TPB + tid, N = a.s.N;
    const bool live = m < a.s.M;                                  // no early exit: shuffles and a barrier below
    const int64_t mc = live ? m : a.s.M - 1;
    const Src s = source(a, q, k, mc);
    const double mu = a.w.mu[((int64_t)k * NQ + q) * a.s.M + mc];
    auto centred = [&](int64_t i) { return i < N ? at(s, i) - mu : 0.0; };
    double w[LAGS], acc[LAGS];
#pragma unroll
    for (int j = 0; j < LAGS; ++j) { w[j] = centred(t0 + j); acc[j] = 0.0; }
    // at draw i = i0 + u the window slot (u + j) mod 16 holds the centred draw i + t0 + j; a slot beyond the chain holds 0
    for (int64_t i0 = 0; i0 < N - t0; i0 += LAGS) {
#pragma unroll
        for (int u = 0; u < LAGS; ++u) {
            const double c = centred(i0 + u);
#pragma unroll
            for (int j = 0; j < LAGS; ++j) acc[j] += c * w[(u + j) & (LAGS - 1)];
            w[u] = centred(i0 + u + t0 + LAGS);
        }
    }
#pragma unroll
    for (int j = 0; j < LAGS; ++j) {
        const double t = wave_sum(live ? acc[j] / (double)N : 0.0);
        if (lane == 0) s_red[wave][j] = t;
    }
    __syncthreads();
    if (tid < LAGS) {
        double t = 0.0;
#pragma unroll
        for (int v = 0; v < WAVES; ++v) t += s_red[v][tid];
        a.w.part[(((int64_t)k * NQ_ACOV + q) * a.s.T + t0 + tid) * a.s.nblk + tile] = t;
    }
}

// Σ over the M split chains of v_m (sq: of (v_m − c)²) in the documented order, by one wave: per block of 256 chains a butterfly over each
// of its four waves' lanes, those four in wave order, then the blocks in block order. The same bits in every lane.
__device__ __forceinline__ double chain_sum(const double* v, int64_t M, int64_t nblk, int lane, bool sq, double c) {
    double total = 0.0;
    for (int64_t b = 0; b < nblk; ++b) {
        double t = 0.0;
#pragma unroll
        for (int u = 0; u < WAVES; ++u) {
            const int64_t m = b * TPB + u * 64 + lane;
            double x = 0.0;
            if (m < M) {
                x = v[m];
                if (sq) x = (x - c) * (x - c);
            }
            t += wave_sum(x);
        }
        total += t;
    }
    return total;
}

// W̄ and var⁺ of quantity q of row k
__device__ __forceinline__ void lag0(const ChainArgs& a, int k, int q, int lane, double& wbar, double& varplus) {
    const int64_t M = a.s.M, N = a.s.N, o = ((int64_t)k * NQ + q) * M;
    const double mubar = chain_sum(a.w.mu + o, M, a.s.nblk, lane, false, 0.0) / (double)M;
    const double between = chain_sum(a.w.mu + o, M, a.s.nblk, lane, true, mubar) / (double)(M - 1);
    wbar = chain_sum(a.w.var + o, M, a.s.nblk, lane, false, 0.0) / (double)M;
    varplus = wbar * (double)(N - 1) / (double)N + between;
}

// Geyer's truncation as Stan writes it, on r[0 … T): ρ_t on entry, ρ̂_t afterwards. Returns S/τ.
__device__ double geyer_ess(double* r, int64_t N, int64_t S, double tau_min) {
    double even = 1.0, odd = r[1];
    r[0] = 1.0;
    int64_t t = 1;
    while (t < N - 4 && even + odd > 0.0) {
        even = r[t + 1];
        odd = r[t + 2];
        if (!(even + odd >= 0.0)) { r[t + 1] = 0.0; r[t + 2] = 0.0; }
        t += 2;
    }
    const int64_t max_t = t;
    r[max_t + 1] = even > 0.0 ? even : 0.0;
    for (t = 1; t <= max_t - 3; t += 2) {
        const double before = r[t - 1] + r[t];
        if (r[t + 1] + r[t + 2] > before) { r[t + 1] = before / 2.0; r[t + 2] = r[t + 1]; }
    }
    double sum = 0.0;
    for (t = 0; t < max_t; ++t) sum += r[t];
    const double tau = fmax(-1.0 + 2.0 * sum + r[max_t + 1], tau_min);
    return (double)S / tau;
}

struct FinishArgs {
    ChainArgs c;
    double tau_min;      // 1/log10(S)
    double* out;         // [OCTO_DRAWS_DIAG_N_STATS][K]
};

// blockIdx.x = the row; wave q = quantity q, and wave 0 the folded lag 0 besides
__global__ __launch_bounds__(TPB) void k_diag_finish(FinishArgs a) {
    __shared__ double s_rho[NQ_ACOV][LDS_T];
    __shared__ double s_rhat[NQ], s_ess[NQ_ACOV];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, k = blockIdx.x;
    const Shape& s = a.c.s;
    double wbar, varplus;
    lag0(a.c, k, wave, lane, wbar, varplus);
    if (lane == 0) s_rhat[wave] = sqrt(varplus / wbar);
    if (wave == 0) {
        double wf, vf;
        lag0(a.c, k, 4, lane, wf, vf);
        if (lane == 0) s_rhat[4] = sqrt(vf / wf);
    }
    double* r = s.T <= LDS_T ? s_rho[wave] : a.c.w.rho + ((int64_t)k * NQ_ACOV + wave) * s.T;
    const double* part = a.c.w.part + ((int64_t)k * NQ_ACOV + wave) * s.T * s.nblk;
    for (int64_t t = lane; t < s.T; t += 64) {
        double sum = 0.0;
        for (int64_t b = 0; b < s.nblk; ++b) sum += part[t * s.nblk + b];
        r[t] = 1.0 - (wbar - sum / (double)s.M) / varplus;
    }
    __syncthreads();
    if (lane == 0) s_ess[wave] = isfinite(varplus) && varplus > 0.0 ? geyer_ess(r, s.N, s.S, a.tau_min) : NAN;
    __syncthreads();
    if (tid != 0) return;
    const int K = s.K;
    const bool ok = a.c.w.ok[k] != 0;
    auto put = [&](int stat, double v) { a.out[(int64_t)stat * K + k] = ok ? v : NAN; };
    const double rz = s_rhat[0], rf = s_rhat[4], e05 = s_ess[2], e95 = s_ess[3];
    put(OCTO_DRAWS_DIAG_RHAT, rz != rz || rf != rf ? NAN : fmax(rz, rf));
    put(OCTO_DRAWS_DIAG_ESS_BULK, s_ess[0]);
    put(OCTO_DRAWS_DIAG_ESS_TAIL, e05 != e05 || e95 != e95 ? NAN : fmin(e05, e95));
    put(OCTO_DRAWS_DIAG_RHAT_BASIC, s_rhat[1]);
    put(OCTO_DRAWS_DIAG_ESS_BASIC, s_ess[1]);
    put(OCTO_DRAWS_DIAG_Q05, a.c.w.q[k]);
    put(OCTO_DRAWS_DIAG_Q50, a.c.w.q[K + k]);
    put(OCTO_DRAWS_DIAG_Q95, a.c.w.q[2 * K + k]);
}

// ---- host side
int check_shape(octo_draws* h, const char* who, int64_t n, int64_t W, int64_t ld, int64_t ls, int32_t K) {
    if (K < 1 || K > OCTO_DRAWS_MAX_GROUPS) return fail(h, OCTO_EINVAL, std::string(who) + ": K must be 1 ... OCTO_DRAWS_MAX_GROUPS");
    if (n < 8 || W < 1 || ld < W || ls / K < ld) return fail(h, OCTO_EINVAL, std::string(who) + ": need n >= 8, 1 <= W <= ld, ls >= K*ld");
    if (!shape_supported(n, W)) return fail(h, OCTO_ENOTSUP, std::string(who) + ": more than 2^24 used draws per row");
    return OCTO_OK;
}

inline int64_t work_doubles(const Shape& s) { return carve_size(diag_work, (int64_t)s.K, s.P, s.S, s.M, s.T, s.nblk); }

int grow_work(octo_draws* h, const Shape& s, DiagWork& w) { return grow_to(h, h->d_diag, h->cap_diag, w, diag_work, (int64_t)s.K, s.P, s.S, s.M, s.T, s.nblk); }

// the bitonic network on the K rows of P keys
void sort_rows(hipStream_t st, double* keys, const Shape& s) {
    const dim3 blocks((unsigned)(s.P / SORT_BLK), (unsigned)s.K), pairs((unsigned)((s.P / 2 + TPB - 1) / TPB), (unsigned)s.K);
    hipLaunchKernelGGL(k_diag_sort_local, blocks, dim3(TPB), 0, st, keys, s.P, (int64_t)0);
    for (int64_t kk = 2 * SORT_BLK; kk <= s.P; kk <<= 1) {
        for (int64_t j = kk >> 1; j >= SORT_BLK; j >>= 1) hipLaunchKernelGGL(k_diag_sort_global, pairs, dim3(TPB), 0, st, keys, s.P, kk, j);
        hipLaunchKernelGGL(k_diag_sort_local, blocks, dim3(TPB), 0, st, keys, s.P, kk);
    }
}

// the keys of every row sorted, its quantiles and validity; fold: the folded keys sorted too
int sorted_keys(octo_draws* h, hipStream_t st, const double* d_x, const Shape& s, const DiagWork& w, bool fold) {
    OCHK(h, hipMemsetAsync(w.bad, 0, sizeof(int32_t) * (size_t)s.K, st));
    KeyArgs ka;
    ka.x = d_x; ka.s = s; ka.w = w; ka.fold = 0;
    const dim3 grid((unsigned)(s.P / TPB), (unsigned)s.K);
    hipLaunchKernelGGL(k_diag_keys, grid, dim3(TPB), 0, st, ka);
    sort_rows(st, w.keys, s);
    hipLaunchKernelGGL(k_diag_quant, dim3(1), dim3(TPB), 0, st, s, w);
    if (fold) {
        ka.fold = 1;
        hipLaunchKernelGGL(k_diag_keys, grid, dim3(TPB), 0, st, ka);
        sort_rows(st, w.fkeys, s);
    }
    return OCTO_OK;
}

void launch_rank(hipStream_t st, const double* d_x, const Shape& s, const DiagWork& w, bool fold, bool user, double* rank, double* z) {
    RankArgs ra;
    ra.x = d_x; ra.s = s; ra.w = w; ra.fold = fold ? 1 : 0; ra.user = user ? 1 : 0; ra.rank = rank; ra.z = z;
    hipLaunchKernelGGL(k_diag_rank, dim3((unsigned)((s.S + TPB - 1) / TPB), (unsigned)s.K), dim3(TPB), 0, st, ra);
}

}  // namespace

extern "C" {

int64_t octo_draws_diagnose_work_doubles(int64_t n, int64_t W, int32_t K) {
    if (!shape_ok(n, W, K) || !shape_supported(n, W)) return 0;
    return work_doubles(shape_of(n, W, W, (int64_t)K * W, K));
}

int32_t octo_draws_rank_device(octo_draws* h, int64_t n, int64_t W, int64_t ld, int64_t ls, int32_t K, const double* d_x, int32_t fold,
                               double* d_rank, double* d_z, void* hip_stream) {
    const char* who = "octo_draws_rank_device";
    if (!h) return OCTO_EINVAL;
    if (!d_x) return fail(h, OCTO_EINVAL, std::string(who) + ": d_x is required");
    if (int rc = check_shape(h, who, n, W, ld, ls, K)) return rc;
    if (!d_rank && !d_z) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const Shape s = shape_of(n, W, ld, ls, K);
    DiagWork w;
    if (int rc = grow_work(h, s, w)) return rc;
    if (int rc = sorted_keys(h, st, d_x, s, w, fold != 0)) return rc;
    launch_rank(st, d_x, s, w, fold != 0, true, d_rank, d_z);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_diagnose_device(octo_draws* h, int64_t n, int64_t W, int64_t ld, int64_t ls, int32_t K, const double* d_x, double* d_out,
                                   void* hip_stream) {
    const char* who = "octo_draws_diagnose_device";
    if (!h) return OCTO_EINVAL;
    if (!d_x || !d_out) return fail(h, OCTO_EINVAL, std::string(who) + ": d_x and d_out are required");
    if (int rc = check_shape(h, who, n, W, ld, ls, K)) return rc;
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const Shape s = shape_of(n, W, ld, ls, K);
    FinishArgs f;
    ChainArgs& c = f.c;
    c.x = d_x; c.s = s;
    if (int rc = grow_work(h, s, c.w)) return rc;
    if (int rc = sorted_keys(h, st, d_x, s, c.w, true)) return rc;
    launch_rank(st, d_x, s, c.w, false, false, nullptr, c.w.z);
    launch_rank(st, d_x, s, c.w, true, false, nullptr, c.w.zf);
    hipLaunchKernelGGL(k_diag_moments, dim3((unsigned)s.nblk, (unsigned)(s.K * NQ)), dim3(TPB), 0, st, c);
    hipLaunchKernelGGL(k_diag_acov, dim3((unsigned)(s.nblk * (s.T / LAGS)), (unsigned)(s.K * NQ_ACOV)), dim3(TPB), 0, st, c);
    f.tau_min = 1.0 / std::log10((double)s.S);
    f.out = d_out;
    hipLaunchKernelGGL(k_diag_finish, dim3((unsigned)s.K), dim3(TPB), 0, st, f);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // extern "C"
