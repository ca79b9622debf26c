// octo_draws_gpd.hip — liboctofitter_hip_draws.so, the twentieth part: the Gaussian-process RV table under DENSE kernels (include/octofitter_hip_draws.h,
// "The twentieth"): squared-exponential, Matérn 3/2 and 5/2, periodic and quasi-periodic terms, log N(r; 0, K) by a dense Cholesky factor and the exact
// gradient through K⁻¹. octo_draws_gp.hip owns the table, the C ABI and the row-parallel passes; gp_launch there runs k_gp_rows (r into the work array), then
// draws_gpd_launch here, then k_gp_adj and k_gp_finish on α where r was.
//
// ONE WORKGROUP OF 256 THREADS A WALKER, grid = W: the celerite recursion is sequential in the rows (lane = walker), a dense factorisation is O(n³) and
// parallel inside a walker. The packed lower triangle (row-major: (i, j) at i(i + 1)/2 + j) lives in the workgroup's LDS for n <= OCTO_DRAWS_GP_DENSE_LDS_ROWS
// and in the work array beyond (TriLds / TriGlobal: one body, two accessors). Consecutive rows of one column are triangular numbers apart, which visit every
// bank residue: a column access by 32 consecutive lanes is at most 2-way conflicted, a row access is contiguous.
//
//   k_gpd_factor   K from the epochs and this walker's hyperparameters; right-looking Cholesky in place — per column: scale it, barrier, rank-1 update of
//                  the trailing triangle (eight half-waves take rows, their lanes the columns), barrier — with y = L⁻¹r carried as the factorisation's row n;
//                  ℓ = −½yᵀy − Σ log L_jj − (n/2)·log 2π and the validity, every thread adding the same terms in column order; α = L⁻ᵀy by columns from the
//                  last (one barrier a column), written over r, and μ.
//   k_gpd_grad     the same body (LDS does not outlive a launch, so the gradient call factors in its own launch: its ℓ and α are the forward call's bits),
//                  then L⁻¹ in place column by column from the last (dtrti2) and K⁻¹ = L⁻ᵀL⁻¹ row by row from the first (dlauu2), every dot product one
//                  thread's in index order; then G_ij = α_iα_j − K⁻¹_ij against the closed-form ∂k/∂h at τ_ij, each thread a fixed set of pairs, the
//                  partials added in a wave (wave_sum's fixed butterfly) and across the four waves in wave order.
// No atomics; nothing runs for the padding columns up to ldw.
#include "octo_draws_gp_shared.h"

namespace {

constexpr int GPD_T = 256, GPD_GROUPS = GPD_T / 32, GPD_LDS_ROWS = OCTO_DRAWS_GP_DENSE_LDS_ROWS, GPD_MAX_N = OCTO_DRAWS_GP_DENSE_MAX_N;
constexpr int GPD_NV = 4;                    // the vectors of n in LDS: epochs, r → y → the back substitution's running vector, α, 1/L_jj
constexpr int GPD_NSUM = 4 * GP_J + 2;       // a thread's partial sums: four a term, tr K⁻¹, Σα²
constexpr int GPD_RED = 128;                 // the four waves' sums, the walker's hyperparameters
static_assert(GPD_NSUM * (GPD_T / WAVE) + 4 * GP_J <= GPD_RED, "the waves' sums and the hyperparameters fit their part of LDS");
constexpr size_t GPD_LDS_LIMIT = 163840;     // what one workgroup of a gfx950 may hold

constexpr size_t gpd_lds_bytes(int64_t n, bool lds) { return sizeof(double) * (size_t)((lds ? n * (n + 1) / 2 : 0) + GPD_NV * n + GPD_RED); }
static_assert(gpd_lds_bytes(GPD_LDS_ROWS, true) <= GPD_LDS_LIMIT, "OCTO_DRAWS_GP_DENSE_LDS_ROWS rows fit one workgroup's LDS");
static_assert(gpd_lds_bytes(GPD_MAX_N, false) <= GPD_LDS_LIMIT, "the vectors of the longest table fit");
static_assert((int64_t)GPD_MAX_N * (GPD_MAX_N + 1) / 2 < ((int64_t)1 << 31), "an index into one walker's triangle is an int");

// the packed lower triangle: NQ = the rows (or columns) one thread may own in the inverse's passes, ⌈most rows/256⌉
struct TriLds {
    static constexpr int NQ = (GPD_LDS_ROWS + GPD_T - 1) / GPD_T;
    static constexpr bool LDS = true;
    double* p;
    __device__ __forceinline__ double& operator()(int i, int j) const { return p[i * (i + 1) / 2 + j]; }
};
struct TriGlobal {
    static constexpr int NQ = (GPD_MAX_N + GPD_T - 1) / GPD_T;
    static constexpr bool LDS = false;
    double* p;
    __device__ __forceinline__ double& operator()(int i, int j) const { return p[i * (i + 1) / 2 + j]; }
};

// k(τ) of one term and, with DERIV, ∂k/∂(its parameters in hyper-row order); h = (a, ·, ·, ·)
template <bool DERIV>
__device__ __forceinline__ double gpd_term(int kind, const double* h, double tau, double (&dk)[4]) {
    const double a = h[0], a2 = a * a;
    if (kind == OCTO_DRAWS_GP_SE) {
        const double q = tau / h[1], E = exp(-0.5 * (q * q)), k = a2 * E;
        if (DERIV) { dk[0] = 2.0 * a * E; dk[1] = k * (q * q) / h[1]; }
        return k;
    }
    if (kind == OCTO_DRAWS_GP_MATERN32) {
        const double u = 1.7320508075688772 * tau / h[1], e = exp(-u);
        if (DERIV) { dk[0] = 2.0 * a * ((1.0 + u) * e); dk[1] = a2 * (u * u) * e / h[1]; }
        return a2 * ((1.0 + u) * e);
    }
    if (kind == OCTO_DRAWS_GP_MATERN52) {
        const double u = 2.23606797749979 * tau / h[1], e = exp(-u), p = fma(u, fma(u, 1.0 / 3.0, 1.0), 1.0);
        if (DERIV) { dk[0] = 2.0 * a * (p * e); dk[1] = a2 * (u * u) * (1.0 + u) * e / (3.0 * h[1]); }
        return a2 * (p * e);
    }
    const bool qp = kind == OCTO_DRAWS_GP_QUASIPERIODIC;
    const double P = qp ? h[2] : h[1], r = qp ? h[3] : h[2];
    double sn, cs;
    sincospi(tau / P, &sn, &cs);
    const double z = sn / r, q = qp ? tau / h[1] : 0.0;
    const double E = exp(-0.5 * fma(q, q, z * z)), k = a2 * E;
    if (DERIV) {
        const double dP = k * (sn * cs) * (M_PI * tau) / ((P * P) * (r * r)), dr = k * (z * z) / r;
        dk[0] = 2.0 * a * E;
        if (qp) { dk[1] = k * (q * q) / h[1]; dk[2] = dP; dk[3] = dr; }
        else { dk[1] = dP; dk[2] = dr; }
    }
    return k;
}

struct GpdVecs { double *ts, *yv, *al, *dinv, *red, *hp; };      // hp [GP_J][4]: this walker's hyperparameters, read from LDS where they are used

// this walker's hyperparameters to hp [term][parameter] in LDS (every thread stores the same values); returns their validity: finite, a² finite, every
// length, period and width > 0
__device__ __forceinline__ bool gpd_hyper(const GpArgs& a, int64_t w, double* hp) {
    bool ok = true;
    int o = 0;
#pragma unroll
    for (int t = 0; t < GP_J; ++t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) hp[4 * t + k] = 1.0;
        if (t < a.J) {      // the terms' kinds are uniform
            const int nh = a.term[t] == OCTO_DRAWS_GP_QUASIPERIODIC ? 4 : (a.term[t] == OCTO_DRAWS_GP_PERIODIC ? 3 : 2);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nh) {
                    const double x = a.hyper[(int64_t)(o + k) * a.ld + w];
                    hp[4 * t + k] = x;
                    ok = ok && isfinite(x) && (k == 0 ? isfinite(x * x) : x > 0.0);
                }
            o += nh;
        }
    }
    return ok;
}

// K, its factor, y, ℓ, the validity and α (kept in v.al, written over r with want_alpha); returns the validity. Every thread of the workgroup calls it.
template <class Tri>
__device__ __forceinline__ bool gpd_factor_body(const GpArgs& a, int64_t w, const Tri A, const GpdVecs v, bool ok, double s2,
                                                bool want_alpha) {
    const int tid = threadIdx.x, grp = tid >> 5, l = tid & 31, n = a.n;
    for (int i = tid; i < n; i += GPD_T) {
        v.ts[i] = a.rows[(int64_t)i * GROWW];
        v.yv[i] = a.k.res[(int64_t)i * a.ldw + w];
    }
    __syncthreads();
    double ll = 0.0;
    if (ok) {      // uniform: every thread holds the same validity
        for (int i = grp; i < n; i += GPD_GROUPS) {
            const double ti = v.ts[i];
            for (int k = l; k <= i; k += 32) {
                const double tau = fabs(ti - v.ts[k]);
                double x = 0.0, dk[4];
#pragma unroll 1
                for (int t = 0; t < a.J; ++t) x += gpd_term<false>(a.term[t], v.hp + 4 * t, tau, dk);      // in term order
                A(i, k) = i == k ? (a.rows[(int64_t)i * GROWW + 2] + s2) + x : x;
            }
        }
        __syncthreads();
        double yy = 0.0, logdet = 0.0;
        for (int j = 0; j < n; ++j) {
            const double d = A(j, j);
            if (!(d > 0.0 && isfinite(d))) { ok = false; break; }      // uniform: the pivot every thread read behind the barrier
            const double Ljj = sqrt(d), inv = 1.0 / Ljj, yj = v.yv[j] * inv;
            yy = fma(yj, yj, yy);
            logdet += log(Ljj);
            for (int i = j + 1 + tid; i < n; i += GPD_T) A(i, j) *= inv;
            __syncthreads();      // the column is scaled, and nobody reads the pivot or r_j any more
            if (tid == 0) { A(j, j) = Ljj; v.yv[j] = yj; v.dinv[j] = inv; }
            for (int i = j + 1 + tid; i < n; i += GPD_T) v.yv[i] = fma(-A(i, j), yj, v.yv[i]);      // row n of the factorisation: r
            for (int i = j + 1 + grp; i < n; i += GPD_GROUPS) {
                const double Lij = A(i, j);
                for (int k = j + 1 + l; k <= i; k += 32) A(i, k) = fma(-Lij, A(k, j), A(i, k));
            }
            __syncthreads();
        }
        ll = fma(-0.5, yy, -logdet) - 0.5 * (double)n * LOG2PI;
        ok = ok && isfinite(ll);
    }
    if (ok && want_alpha) {
        for (int j = n - 1; j >= 0; --j) {      // α = L⁻ᵀy by columns from the last: y_i −= L_ji·α_j for i < j
            const double aj = v.yv[j] * v.dinv[j];
            for (int i = tid; i < j; i += GPD_T) v.yv[i] = fma(-A(j, i), aj, v.yv[i]);
            if (tid == 0) v.al[j] = aj;
            __syncthreads();
        }
    }
    if (tid == 0) {
        a.k.ok[w] = ok ? 1.0 : 0.0;
        if (a.ll) a.ll[w] = (a.accumulate ? a.ll[w] : 0.0) + (ok ? ll : -INFINITY);
    }
    if (want_alpha)
        for (int i = tid; i < n; i += GPD_T) {
            double* r = a.k.res + (int64_t)i * a.ldw + w;
            const double res = *r, alpha = ok ? v.al[i] : 0.0;
            *r = alpha;
            if (a.mu) a.mu[(int64_t)i * a.ld_out + w] = fma(-(a.rows[(int64_t)i * GROWW + 2] + s2), alpha, res);
        }
    return ok;
}

// what every thread needs before the body: the vectors' places, the walker's validity apart from the factorisation
template <class Tri>
__device__ __forceinline__ bool gpd_open(const GpArgs& a, int64_t w, double* lds, Tri& A, GpdVecs& v, double& s, double& s2) {
    const int64_t ntri = (int64_t)a.n * (a.n + 1) / 2;
    double* vec = lds;
    if constexpr (Tri::LDS) { A.p = lds; vec = lds + ntri; }
    else A.p = a.tri + w * ntri;
    v.ts = vec; v.yv = vec + a.n; v.al = vec + 2 * a.n; v.dinv = vec + 3 * a.n; v.red = vec + 4 * a.n; v.hp = v.red + GPD_NSUM * (GPD_T / WAVE);
    s = a.jitter ? a.jitter[w] : 0.0;
    s2 = s * s;
    bool ok = gpd_hyper(a, w, v.hp) && isfinite(s) && s >= 0.0;
    if (a.beta)
        for (int k = 0; k < a.K; ++k) ok = ok && isfinite(a.beta[(int64_t)k * a.ld + w]);
#pragma unroll 1
    for (int p = 0; p < a.P; ++p) {
        double elv[OCTO_N_EL];
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) elv[k] = a.elems[((int64_t)p * OCTO_N_EL + k) * a.ld + w];
        const SetupScalars q = setup_scalars<true>(elv, a.c, a.orbit_kind[p], a.has_mass[p]);
        ok = ok && setup_valid<true>(elv, a.orbit_kind[p], a.has_mass[p], q.sma);
    }
    return ok;
}

template <class Tri>
__global__ __launch_bounds__(GPD_T) void k_gpd_factor(GpArgs a, int want_alpha) {
    extern __shared__ __attribute__((aligned(16))) double gpd_lds[];
    const int64_t w = blockIdx.x;      // w < W
    Tri A; GpdVecs v; double s, s2;
    const bool ok = gpd_open(a, w, gpd_lds, A, v, s, s2);
    (void)gpd_factor_body(a, w, A, v, ok, s2, want_alpha != 0);
}

template <class Tri>
__global__ __launch_bounds__(GPD_T) void k_gpd_grad(GpArgs a) {
    extern __shared__ __attribute__((aligned(16))) double gpd_lds[];
    const int64_t w = blockIdx.x;      // w < W
    const int tid = threadIdx.x, grp = tid >> 5, l = tid & 31, n = a.n;
    Tri A; GpdVecs v; double s, s2;
    bool ok = gpd_open(a, w, gpd_lds, A, v, s, s2);
    ok = gpd_factor_body(a, w, A, v, ok, s2, true);
    if (ok) {      // uniform
        __syncthreads();
        double acc[Tri::NQ];
        for (int j = n - 1; j >= 0; --j) {      // M = L⁻¹ in place, column j below its diagonal: −(1/L_jj)·Σ_{k = j+1 … i} M_ik·L_kj
            const double dj = v.dinv[j];
#pragma unroll
            for (int q = 0; q < Tri::NQ; ++q) {
                const int i = j + 1 + tid + q * GPD_T;
                double x = 0.0;
                if (i < n)
                    for (int k = j + 1; k <= i; ++k) x = fma(A(i, k), A(k, j), x);
                acc[q] = x;
            }
            __syncthreads();      // the column is read …
#pragma unroll
            for (int q = 0; q < Tri::NQ; ++q) {
                const int i = j + 1 + tid + q * GPD_T;
                if (i < n) A(i, j) = -dj * acc[q];
            }
            if (tid == 0) A(j, j) = dj;
            __syncthreads();      // … and written
        }
        for (int i = 0; i < n; ++i) {      // K⁻¹ = MᵀM in place, row i: Σ_{k >= i} M_ki·M_kj; the rows behind i are still M
#pragma unroll
            for (int q = 0; q < Tri::NQ; ++q) {
                const int j = tid + q * GPD_T;
                double x = 0.0;
                if (j <= i)
                    for (int k = i; k < n; ++k) x = fma(A(k, i), A(k, j), x);
                acc[q] = x;
            }
            __syncthreads();      // row i is read (its own k = i products) before it is written; the next row reads none of it
#pragma unroll
            for (int q = 0; q < Tri::NQ; ++q) {
                const int j = tid + q * GPD_T;
                if (j <= i) A(i, j) = acc[q];
            }
        }
        __syncthreads();
        // ½·Σ_ij G_ij·∂K_ij/∂h, term by term: the diagonal once, a pair below it for both of its places. A thread's pairs are fixed by its index; its
        // partials go through a fixed butterfly in its wave, and the four waves' sums wait in LDS to be added in wave order.
#pragma unroll 1
        for (int t = 0; t < a.J; ++t) {
            const int kind = a.term[t];
            double sum[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = grp; i < n; i += GPD_GROUPS) {
                const double ti = v.ts[i], ai = v.al[i];
                for (int k = l; k <= i; k += 32) {
                    const double tau = fabs(ti - v.ts[k]), G = (i == k ? 0.5 : 1.0) * fma(ai, v.al[k], -A(i, k));
                    double dk[4] = {0.0, 0.0, 0.0, 0.0};
                    (void)gpd_term<true>(kind, v.hp + 4 * t, tau, dk);
#pragma unroll
                    for (int p = 0; p < 4; ++p) sum[p] = fma(G, dk[p], sum[p]);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const double x = wave_sum(sum[p]);
                if ((tid & (WAVE - 1)) == 0) v.red[(tid / WAVE) * GPD_NSUM + 4 * t + p] = x;
            }
        }
        double tr = 0.0, aa = 0.0;
        for (int i = tid; i < n; i += GPD_T) {
            tr += A(i, i);
            aa = fma(v.al[i], v.al[i], aa);
        }
        tr = wave_sum(tr);
        aa = wave_sum(aa);
        if ((tid & (WAVE - 1)) == 0) { v.red[(tid / WAVE) * GPD_NSUM + 4 * GP_J] = tr; v.red[(tid / WAVE) * GPD_NSUM + 4 * GP_J + 1] = aa; }
    }
    __syncthreads();
    if (tid != 0) return;
    const auto total = [&](int k) {      // the four waves in wave order
        double x = 0.0;
#pragma unroll
        for (int q = 0; q < GPD_T / WAVE; ++q) x += v.red[q * GPD_NSUM + k];
        return x;
    };
    if (a.g_jitter) a.g_jitter[w] = ok ? s * (total(4 * GP_J + 1) - total(4 * GP_J)) : 0.0;
    if (!a.g_hyper) return;
    int o = 0;
#pragma unroll 1
    for (int t = 0; t < a.J; ++t) {
        const int nh = a.term[t] == OCTO_DRAWS_GP_QUASIPERIODIC ? 4 : (a.term[t] == OCTO_DRAWS_GP_PERIODIC ? 3 : 2);
        for (int p = 0; p < nh; ++p) a.g_hyper[(int64_t)(o + p) * a.ld + w] = ok ? total(4 * t + p) : 0.0;
        o += nh;
    }
}

template <class Tri>
int gpd_raise_lds(octo_draws* h, size_t bytes) {
    for (const void* f : {(const void*)k_gpd_factor<Tri>, (const void*)k_gpd_grad<Tri>})
        if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, OCTO_ENOTSUP, "octo_draws_gp_set: a dense table of this many rows needs more LDS per block than this device gives");
        }
    return OCTO_OK;
}

}  // namespace

int draws_gpd_prepare(octo_draws* h, int64_t n) {
    const bool lds = n <= GPD_LDS_ROWS;
    const size_t bytes = gpd_lds_bytes(n, lds);
    int limit = 0;
    OCHK(h, hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
    if ((size_t)limit < bytes)
        return fail(h, OCTO_ENOTSUP, "octo_draws_gp_set: a dense table of " + std::to_string(n) + " rows needs " + std::to_string(bytes) +
                                         " bytes of LDS per block, this device gives " + std::to_string(limit));
    return lds ? gpd_raise_lds<TriLds>(h, gpd_lds_bytes(GPD_LDS_ROWS, true)) : gpd_raise_lds<TriGlobal>(h, gpd_lds_bytes(GPD_MAX_N, false));
}

int draws_gpd_launch(octo_draws* h, hipStream_t st, const void* gp_args, bool want_ll, bool want_alpha) {
    const GpArgs& a = *static_cast<const GpArgs*>(gp_args);
    if (!want_ll && !want_alpha) return OCTO_OK;
    const bool lds = a.n <= GPD_LDS_ROWS, grad = a.g_hyper || a.g_jitter;
    const size_t bytes = gpd_lds_bytes(a.n, lds);
    const dim3 grid((unsigned)a.W), block(GPD_T);
    if (lds) {
        if (grad) hipLaunchKernelGGL(k_gpd_grad<TriLds>, grid, block, bytes, st, a);
        else hipLaunchKernelGGL(k_gpd_factor<TriLds>, grid, block, bytes, st, a, want_alpha ? 1 : 0);
    } else {
        if (grad) hipLaunchKernelGGL(k_gpd_grad<TriGlobal>, grid, block, bytes, st, a);
        else hipLaunchKernelGGL(k_gpd_factor<TriGlobal>, grid, block, bytes, st, a, want_alpha ? 1 : 0);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}
