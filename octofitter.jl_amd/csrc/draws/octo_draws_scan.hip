// octo_draws_scan.hip — liboctofitter_hip_draws.so, the seventeenth part: along-scan absolute astrometry (include/octofitter_hip_draws.h, "The
// seventeenth"): the Hipparcos intermediate astrometric data and Gaia's epoch astrometry as one table of along-scan residuals against the star's reflex
// motion plus a linear model in the caller's design columns. Of the main library's sources it INCLUDES the device routines the likelihood kernels run
// (octo_companion_device.h: walker_setup = setup_planet_vals<true>, load_pc, the cold kepler_solve<2, false>; octo_kernels.h: setup_scalars, setup_valid,
// planet_finish), so the orbit constructor, the solve and the chain rule through the constructor are the code the main library runs.
//
//   k_scan_rows<GRAD, MODE>   grid = (walker tiles of 64, tasks of OCTO_DRAWS_SCAN_ROWS rows), one wave a block, lane = walker; the rows are wave-uniform
//                      (scalar loads). r_i is known only once every planet's reflex at row i is in, and the adjoint sums of a planet are against
//                      g_i = w_i r_i, so a task runs planet-outer TWICE over its rows with ONE Kepler solve per (walker, row, planet): sweep A solves,
//                      adds f_p·(u·ra + v·de) into η [row][64] in LDS and keeps (sin E, cos E) [planet][row][2][64] and nine constants of the planet
//                      [planet][9][64] there; the residual sweep forms ℓ, the β and jitter sums and leaves g_i in η's place; sweep B forms a planet's
//                      ten sums in registers from LDS (1/(1 − e cos E) is the solve's own expression on the kept cos E). LDS: 4 KB + 12.5 KB a planet.
//                      MODE 0 sampled · 1 the marginal mode's first pass (A, b) · 2 its second pass (β̂ from the work array, Σw²cᵀA⁻¹c) · 3 η alone.
//   k_scan_solve       marginal mode: A, b summed over the tasks in task order, Cholesky per lane, β̂, A⁻¹, log det A.
//   k_scan_finish      the tasks' sums in task order, validity, and planet_finish per planet: the sums to ∂ℓ/∂(a, e, i, ω, Ω, tp, M, plx, mass).
// Nothing is stored per (walker, row) in HBM, there is no atomic, and the row partition does not depend on W: a walker's bits depend on its column alone.
#include "octo_draws_common.h"

namespace scan_dev {      // the companions' device routines under a name of their own: that header and octo_draws_common.h both define a wave_sum
#include "octo_companion_device.h"
}

namespace {
using scan_dev::dev_consts;
using scan_dev::walker_setup;

constexpr int SCAN_R = OCTO_DRAWS_SCAN_ROWS, SCAN_K = OCTO_DRAWS_SCAN_MAX_K;
constexpr int ROWW = 12;                       // a row record: {t, u, v, y, σ², c[6] (0 behind K), 0}
constexpr int N_TRI = SCAN_K * (SCAN_K + 1) / 2;      // 21
constexpr int N_MARG = SCAN_K + N_TRI + 1;     // ScanWork::marg: β̂, A⁻¹, log det A
enum { S_LL = 0, S_JIT, S_MARG, S_BETA, S_PL = S_BETA + SCAN_K, PL_N = 10 };      // a task's sums; first pass of the marginal mode: A at 0, b at N_TRI
enum { C_F = 0, C_E, C_TP, C_CB, C_CGB, C_CA, C_CFB, C_CBE, C_CAE, N_CST };       // a planet's constants in LDS
using FinL = Layout<2, true, false, KM_RADEC>;      // the main library's sums of a planet with a mass term and no RV: U1 … U6, GE, GM, GT, GC
static_assert(FinL::PL_N == PL_N, "ten sums a planet");
static_assert(N_MARG == 28, "octo_draws_layout.h: ScanWork::marg");

struct ScanArgs {
    const double* rows;            // [n][ROWW]
    int32_t n, K, P, accumulate;
    int32_t orbit_kind[MAXP], has_mass[MAXP];
    DevConsts c;
    const double* elems; int64_t ld, W, ldw;
    const double* beta; int64_t ldb;      // [K][ldb] or null
    const double* jitter;                 // [W] or null
    ScanWork k;
    int32_t n_tasks, n_sums, marginal, grad;
    double *ll, *g_elems, *g_beta, *g_jitter, *beta_hat;
    double* eta; int64_t ld_eta;          // MODE 3
};

__device__ __forceinline__ bool scan_contributes(const ScanArgs& a, int p) {      // wave-uniform
    const int kind = a.orbit_kind[p];
    return (kind == OCTO_ORBIT_VISUAL_KEP || kind == OCTO_ORBIT_THIELE_INNES) && a.has_mass[p] != 0;
}

template <bool GRAD, int MODE>
__global__ __launch_bounds__(WAVE) void k_scan_rows(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) double L[];
    const int lane = threadIdx.x, task = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;      // w < ldw: the work array has a column for every lane
    const int64_t wl = w < a.W ? w : a.W - 1;
    const int r0 = task * SCAN_R, nr = min(SCAN_R, a.n - r0), P = a.P;
    const double* __restrict__ rows = a.rows + (int64_t)r0 * ROWW;
    double* eta = L + lane;                                              // [SCAN_R][64]
    double* sol = L + SCAN_R * WAVE + lane;                              // [P][SCAN_R][2][64]
    double* cst = L + (SCAN_R + P * SCAN_R * 2) * WAVE + lane;           // [P][N_CST][64]
    const double s = a.jitter ? a.jitter[wl] : 0.0, s2 = s * s;

    // ---- the linear part
    {
        double bk[SCAN_K];
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) {
            if constexpr (MODE == 2) bk[k] = a.k.marg[(int64_t)k * a.ldw + w];
            else bk[k] = (MODE == 1 || !a.beta || k >= a.K) ? 0.0 : a.beta[(int64_t)k * a.ldb + wl];
        }
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * ROWW;
            double e = 0.0;
#pragma unroll
            for (int k = 0; k < SCAN_K; ++k) e = fma(rw[5 + k], bk[k], e);
            eta[r * WAVE] = e;
        }
    }
    // ---- sweep A: one solve per (row, planet)
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        if (!scan_contributes(a, p)) continue;
        double v[NWC];
        (void)walker_setup(a, p, wl, v);
        PC pc;
        load_pc(pc, v, 1, 0, 0);
        const double f = -v[WC_MU];
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * ROWW;
            const KSol ks = kepler_solve<2, false>(rw[0], pc);
            const double ra = fma(pc.cB, ks.cE, fma(pc.cGb, ks.sE, -pc.cBe));
            const double de = fma(pc.cA, ks.cE, fma(pc.cFb, ks.sE, -pc.cAe));
            eta[r * WAVE] = fma(f, fma(rw[1], ra, rw[2] * de), eta[r * WAVE]);
            if constexpr (GRAD) {
                sol[((p * SCAN_R + r) * 2 + 0) * WAVE] = ks.sE;
                sol[((p * SCAN_R + r) * 2 + 1) * WAVE] = ks.cE;
            }
        }
        if constexpr (GRAD) {
            double* o = cst + p * N_CST * WAVE;
            o[C_F * WAVE] = f; o[C_E * WAVE] = pc.e; o[C_TP * WAVE] = pc.tp; o[C_CB * WAVE] = pc.cB; o[C_CGB * WAVE] = pc.cGb;
            o[C_CA * WAVE] = pc.cA; o[C_CFB * WAVE] = pc.cFb; o[C_CBE * WAVE] = pc.cBe; o[C_CAE * WAVE] = pc.cAe;
        }
    }
    if constexpr (MODE == 3) {
        if (w < a.W)
            for (int r = 0; r < nr; ++r) a.eta[(int64_t)(r0 + r) * a.ld_eta + w] = eta[r * WAVE];
        return;
    }
    double* part = a.k.part + (int64_t)task * a.n_sums * a.ldw + w;
    // ---- the residual sweep
    if constexpr (MODE == 1) {
        double A[N_TRI], b[SCAN_K];
#pragma unroll
        for (int k = 0; k < N_TRI; ++k) A[k] = 0.0;
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) b[k] = 0.0;
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * ROWW;
            const double wgt = 1.0 / (rw[4] + s2), rho = rw[3] - eta[r * WAVE];
#pragma unroll
            for (int i = 0; i < SCAN_K; ++i) {
                const double wc = wgt * rw[5 + i];
                b[i] = fma(wc, rho, b[i]);
#pragma unroll
                for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = fma(wc, rw[5 + j], A[i * (i + 1) / 2 + j]);
            }
        }
#pragma unroll
        for (int k = 0; k < N_TRI; ++k) part[(int64_t)k * a.ldw] = A[k];
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) part[(int64_t)(N_TRI + k) * a.ldw] = b[k];
        return;
    } else {
        double ll = 0.0, sj = 0.0, sm = 0.0, sb[SCAN_K];
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) sb[k] = 0.0;
        double Ai[(GRAD && MODE == 2) ? N_TRI : 1];
        if constexpr (GRAD && MODE == 2) {
#pragma unroll
            for (int k = 0; k < N_TRI; ++k) Ai[k] = a.k.marg[(int64_t)(SCAN_K + k) * a.ldw + w];
        }
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * ROWW;
            const double var = rw[4] + s2, wgt = 1.0 / var, res = rw[3] - eta[r * WAVE], hh = wgt * res;
            ll += fma(-0.5 * hh, res, -0.5 * log(var)) - 0.5 * LOG2PI;
            if constexpr (GRAD) {
                sj += fma(hh, hh, -wgt);
#pragma unroll
                for (int k = 0; k < SCAN_K; ++k) sb[k] = fma(hh, rw[5 + k], sb[k]);
                eta[r * WAVE] = hh;
                if constexpr (MODE == 2) {
                    double q = 0.0;      // cᵀA⁻¹c
#pragma unroll
                    for (int i = 0; i < SCAN_K; ++i) {
                        double ti = 0.0;
#pragma unroll
                        for (int j = 0; j < SCAN_K; ++j) ti = fma(Ai[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i], rw[5 + j], ti);
                        q = fma(ti, rw[5 + i], q);
                    }
                    sm = fma(wgt * wgt, q, sm);
                }
            }
        }
        part[(int64_t)S_LL * a.ldw] = ll;
        if constexpr (GRAD) {
            part[(int64_t)S_JIT * a.ldw] = sj;
            part[(int64_t)S_MARG * a.ldw] = sm;
#pragma unroll
            for (int k = 0; k < SCAN_K; ++k) part[(int64_t)(S_BETA + k) * a.ldw] = sb[k];
        }
    }
    // ---- sweep B: a planet's ten sums against g_i = w_i r_i, the running sums of the main library's astrom_row with r̄a = g·u, d̄ec = g·v
    if constexpr (GRAD) {
#pragma unroll 1
        for (int p = 0; p < P; ++p) {
            double g[PL_N];
#pragma unroll
            for (int k = 0; k < PL_N; ++k) g[k] = 0.0;
            if (scan_contributes(a, p)) {
                const double* o = cst + p * N_CST * WAVE;
                const double f = o[C_F * WAVE], e = o[C_E * WAVE], tp = o[C_TP * WAVE], cB = o[C_CB * WAVE], cGb = o[C_CGB * WAVE], cA = o[C_CA * WAVE],
                             cFb = o[C_CFB * WAVE], cBe = o[C_CBE * WAVE], cAe = o[C_CAE * WAVE];
                for (int r = 0; r < nr; ++r) {
                    const double* __restrict__ rw = rows + r * ROWW;
                    const double hh = eta[r * WAVE];
                    const double sE = sol[((p * SCAN_R + r) * 2 + 0) * WAVE], cE = sol[((p * SCAN_R + r) * 2 + 1) * WAVE];
                    const double invD = rcp_nr<2>(fma(-e, cE, 1.0));
                    const double rab = hh * rw[1], deb = hh * rw[2];
                    const double ra_f = f * rab, de_f = f * deb;
                    g[FinL::U1] = fma(cE, ra_f, g[FinL::U1]);
                    g[FinL::U2] = fma(sE, ra_f, g[FinL::U2]);
                    g[FinL::U3] = fma(cE, de_f, g[FinL::U3]);
                    g[FinL::U4] = fma(sE, de_f, g[FinL::U4]);
                    g[FinL::U5] += ra_f;
                    g[FinL::U6] += de_f;
                    const double rap = fma(cB, cE, fma(cGb, sE, -cBe)), dep = fma(cA, cE, fma(cFb, sE, -cAe));
                    g[FinL::GC] -= fma(rab, rap, deb * dep);      // ∂ℓ/∂(m/M): f = −m/M
                    const double dra = fma(cGb, cE, -(cB * sE)), dde = fma(cFb, cE, -(cA * sE));
                    const double Mb = fma(ra_f, dra, de_f * dde) * invD;
                    g[FinL::GE] = fma(Mb, sE, g[FinL::GE]);
                    g[FinL::GM] += Mb;
                    g[FinL::GT] = fma(Mb, rw[0] - tp, g[FinL::GT]);
                }
            }
#pragma unroll
            for (int k = 0; k < PL_N; ++k) part[(int64_t)(S_PL + p * PL_N + k) * a.ldw] = g[k];
        }
    }
}

// A = L·Lᵀ per lane for the K leading coordinates (the others: the identity), β̂ = A⁻¹b, A⁻¹ = L⁻ᵀL⁻¹, log det A
__global__ __launch_bounds__(WAVE) void k_scan_solve(ScanArgs a) {
    const int64_t w = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    double A[N_TRI], b[SCAN_K];
#pragma unroll
    for (int k = 0; k < N_TRI; ++k) A[k] = 0.0;
#pragma unroll
    for (int k = 0; k < SCAN_K; ++k) b[k] = 0.0;
    for (int t = 0; t < a.n_tasks; ++t) {
        const double* part = a.k.part + (int64_t)t * a.n_sums * a.ldw + w;
#pragma unroll
        for (int k = 0; k < N_TRI; ++k) A[k] += part[(int64_t)k * a.ldw];
#pragma unroll
        for (int k = 0; k < SCAN_K; ++k) b[k] += part[(int64_t)(N_TRI + k) * a.ldw];
    }
#pragma unroll
    for (int i = 0; i < SCAN_K; ++i)
        if (i >= a.K) A[i * (i + 1) / 2 + i] = 1.0;
    double logdet = 0.0;
#pragma unroll
    for (int j = 0; j < SCAN_K; ++j) {
        double d = A[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = fma(-A[j * (j + 1) / 2 + k], A[j * (j + 1) / 2 + k], d);
        const double ljj = sqrt(d), inv = 1.0 / ljj;      // d <= 0 or NaN: NaN from here on, the walker is invalid
        A[j * (j + 1) / 2 + j] = ljj;
        logdet += log(d);
#pragma unroll
        for (int i = j + 1; i < SCAN_K; ++i) {
            double x = A[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) x = fma(-A[i * (i + 1) / 2 + k], A[j * (j + 1) / 2 + k], x);
            A[i * (i + 1) / 2 + j] = x * inv;
        }
    }
    // L⁻¹, lower, column by column
    double Li[N_TRI];
#pragma unroll
    for (int j = 0; j < SCAN_K; ++j) {
        Li[j * (j + 1) / 2 + j] = 1.0 / A[j * (j + 1) / 2 + j];
#pragma unroll
        for (int i = j + 1; i < SCAN_K; ++i) {
            double x = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) x = fma(-A[i * (i + 1) / 2 + k], Li[k * (k + 1) / 2 + j], x);
            Li[i * (i + 1) / 2 + j] = x / A[i * (i + 1) / 2 + i];
        }
    }
    // z = L⁻¹b, β̂ = L⁻ᵀz
    double z[SCAN_K];
#pragma unroll
    for (int i = 0; i < SCAN_K; ++i) {
        double x = 0.0;
#pragma unroll
        for (int k = 0; k <= i; ++k) x = fma(Li[i * (i + 1) / 2 + k], b[k], x);
        z[i] = x;
    }
#pragma unroll
    for (int j = 0; j < SCAN_K; ++j) {
        double x = 0.0;
#pragma unroll
        for (int i = j; i < SCAN_K; ++i) x = fma(Li[i * (i + 1) / 2 + j], z[i], x);
        a.k.marg[(int64_t)j * a.ldw + w] = x;
    }
    // A⁻¹ (i >= j) = Σ_{k >= i} L⁻¹[k][i]·L⁻¹[k][j]
#pragma unroll
    for (int i = 0; i < SCAN_K; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double x = 0.0;
#pragma unroll
            for (int k = i; k < SCAN_K; ++k) x = fma(Li[k * (k + 1) / 2 + i], Li[k * (k + 1) / 2 + j], x);
            a.k.marg[(int64_t)(SCAN_K + i * (i + 1) / 2 + j) * a.ldw + w] = x;
        }
    a.k.marg[(int64_t)(SCAN_K + N_TRI) * a.ldw + w] = logdet;
}

__global__ __launch_bounds__(WAVE) void k_scan_finish(ScanArgs a) {
    const int64_t w = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (w >= a.W) return;
    const int P = a.P, K = a.K;
    const double s = a.jitter ? a.jitter[w] : 0.0;
    bool ok = isfinite(s) && s >= 0.0;
    if (!a.marginal && a.beta)
        for (int k = 0; k < K; ++k) ok = ok && isfinite(a.beta[(int64_t)k * a.ldb + w]);
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        double elv[OCTO_N_EL];
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) elv[k] = a.elems[((int64_t)p * OCTO_N_EL + k) * a.ld + w];
        const SetupScalars q = setup_scalars<true>(elv, a.c, a.orbit_kind[p], a.has_mass[p]);
        ok = ok && setup_valid<true>(elv, a.orbit_kind[p], a.has_mass[p], q.sma);
    }
    double ll = 0.0, sj = 0.0, sm = 0.0;
    for (int t = 0; t < a.n_tasks; ++t) {
        const double* part = a.k.part + (int64_t)t * a.n_sums * a.ldw + w;
        ll += part[(int64_t)S_LL * a.ldw];
        if (a.grad) { sj += part[(int64_t)S_JIT * a.ldw]; sm += part[(int64_t)S_MARG * a.ldw]; }
    }
    if (a.marginal) ll = ll + 0.5 * (double)K * LOG2PI - 0.5 * a.k.marg[(int64_t)(SCAN_K + N_TRI) * a.ldw + w];
    ok = ok && isfinite(ll);
    a.ll[w] = (a.accumulate ? a.ll[w] : 0.0) + (ok ? ll : -INFINITY);
    if (a.marginal && a.beta_hat)
        for (int k = 0; k < K; ++k) a.beta_hat[(int64_t)k * a.ld + w] = a.k.marg[(int64_t)k * a.ldw + w];
    if (!a.grad) return;
    if (a.g_jitter) a.g_jitter[w] = ok ? s * (sj + sm) : 0.0;
    if (a.g_beta && !a.marginal)
        for (int k = 0; k < K; ++k) {
            double x = 0.0;
            for (int t = 0; t < a.n_tasks; ++t) x += a.k.part[((int64_t)t * a.n_sums + S_BETA + k) * a.ldw + w];
            a.g_beta[(int64_t)k * a.ld + w] = ok ? x : 0.0;
        }
    if (!a.g_elems) return;
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        double out[OCTO_N_EL];
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) out[k] = 0.0;
        if (ok && scan_contributes(a, p)) {
            double g[PL_N];
#pragma unroll
            for (int k = 0; k < PL_N; ++k) g[k] = 0.0;
            for (int t = 0; t < a.n_tasks; ++t) {
                const double* part = a.k.part + ((int64_t)t * a.n_sums + S_PL + p * PL_N) * a.ldw + w;
#pragma unroll
                for (int k = 0; k < PL_N; ++k) g[k] += part[(int64_t)k * a.ldw];
            }
            double elv[OCTO_N_EL];
#pragma unroll
            for (int k = 0; k < OCTO_N_EL; ++k) elv[k] = a.elems[((int64_t)p * OCTO_N_EL + k) * a.ld + w];
            const SetupOut so = setup_planet_vals<true>(elv, a.c, a.orbit_kind[p], a.has_mass[p]);
            FinPC fp;
            fp.sma = so.v[WC_A]; fp.P_d = rcp_nr<2>(so.v[WC_INVP]); fp.beta = so.v[WC_BETA];
            fp.si = so.v[WC_SINI]; fp.ci = so.v[WC_COSI]; fp.sO = so.v[WC_SINO]; fp.cO = so.v[WC_COSO]; fp.sw = so.v[WC_SINW]; fp.cw = so.v[WC_COSW];
            planet_finish<2, true, false, KM_RADEC>(so.el, out, 1, nullptr, 0, a.c, a.orbit_kind[p], a.has_mass[p], p, g, nullptr, fp, true);
        }
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) {
            double* o = a.g_elems + ((int64_t)p * OCTO_N_EL + k) * a.ld + w;
            *o = (a.accumulate ? *o : 0.0) + out[k];
        }
    }
}

inline size_t scan_lds(int P, bool grad) { return sizeof(double) * WAVE * (size_t)(SCAN_R + (grad ? P * (SCAN_R * 2 + N_CST) : 0)); }

inline int check_scan_table(octo_draws* h, const char* who) {
    return h->scan_n > 0 ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no scan table (octo_draws_scan_set)");
}
inline int check_scan_mode(octo_draws* h, const char* who, int32_t mode) {
    if (mode != OCTO_DRAWS_SCAN_SAMPLED && mode != OCTO_DRAWS_SCAN_MARGINAL) return fail(h, OCTO_EINVAL, std::string(who) + ": mode must be OCTO_DRAWS_SCAN_SAMPLED or OCTO_DRAWS_SCAN_MARGINAL");
    return mode == OCTO_DRAWS_SCAN_MARGINAL && h->scan_K == 0 ? fail(h, OCTO_EINVAL, std::string(who) + ": the marginal mode needs K >= 1 design columns") : OCTO_OK;
}

void scan_drop_binding(octo_draws* h) {
    if (!h->scan_bound) return;
    h->scan_bound = 0; h->scan_n_bind = 0;
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->pf_W = 0; h->de_open = false; h->nest_passes = 0;      // a transition is never resumed on another target
}

ScanArgs scan_args(const octo_draws* h, const double* d_elems, int64_t ld, int64_t W, int64_t ldw) {
    ScanArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = h->d_scan_rows; a.n = h->scan_n; a.K = h->scan_K; a.P = h->scan_P;
    for (int p = 0; p < h->scan_P; ++p) { a.orbit_kind[p] = h->scan_kind[p]; a.has_mass[p] = h->scan_mass[p]; }
    a.c = dev_consts(h->scan_consts);
    a.elems = d_elems; a.ld = ld; a.W = W; a.ldw = ldw;
    a.n_tasks = (h->scan_n + SCAN_R - 1) / SCAN_R;
    return a;
}

// the launches of one evaluation on st; ldb: the leading dimension of d_beta, d_g_beta and d_beta_hat's rows is ld
int scan_launch(octo_draws* h, hipStream_t st, int32_t mode, const double* d_elems, int64_t ld, int64_t W, const double* d_beta, const double* d_jitter, double* d_ll,
                double* d_g_elems, double* d_g_beta, double* d_g_jitter, double* d_beta_hat, int32_t accumulate) {
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    ScanArgs a = scan_args(h, d_elems, ld, W, ldw);
    const bool marginal = mode == OCTO_DRAWS_SCAN_MARGINAL, grad = d_g_elems || d_g_jitter || (!marginal && d_g_beta);
    a.n_sums = std::max(S_PL + PL_N * a.P, marginal ? N_TRI + SCAN_K : 0);
    if (int rc = grow_to(h, h->d_scan, h->cap_scan, a.k, scan_work, (int64_t)a.n_tasks, (int64_t)a.n_sums, ldw)) return rc;
    a.beta = marginal ? nullptr : d_beta; a.ldb = ld; a.jitter = d_jitter; a.accumulate = accumulate; a.marginal = marginal; a.grad = grad;
    a.ll = d_ll; a.g_elems = d_g_elems; a.g_beta = d_g_beta; a.g_jitter = d_g_jitter; a.beta_hat = d_beta_hat;
    const dim3 grid((unsigned)(ldw / WAVE), (unsigned)a.n_tasks), tiles((unsigned)(ldw / WAVE)), block(WAVE);
    const size_t lds_f = scan_lds(a.P, false), lds_g = scan_lds(a.P, true);
    if (marginal) {
        hipLaunchKernelGGL((k_scan_rows<false, 1>), grid, block, lds_f, st, a);
        hipLaunchKernelGGL(k_scan_solve, tiles, block, 0, st, a);
        if (grad) hipLaunchKernelGGL((k_scan_rows<true, 2>), grid, block, lds_g, st, a);
        else hipLaunchKernelGGL((k_scan_rows<false, 2>), grid, block, lds_f, st, a);
    } else {
        if (grad) hipLaunchKernelGGL((k_scan_rows<true, 0>), grid, block, lds_g, st, a);
        else hipLaunchKernelGGL((k_scan_rows<false, 0>), grid, block, lds_f, st, a);
    }
    hipLaunchKernelGGL(k_scan_finish, tiles, block, 0, st, a);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

// CᵀΣ⁻¹C is positive definite: the Cholesky factor of its correlation form (unit diagonal) has every pivot above 1e-10
bool scan_full_rank(const double* c, const double* sigma, int K, int64_t n) {
    double A[SCAN_K][SCAN_K] = {};
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) {
            double x = 0.0;
            for (int64_t r = 0; r < n; ++r) x += c[(int64_t)i * n + r] * c[(int64_t)j * n + r] / (sigma[r] * sigma[r]);
            A[i][j] = x;
        }
    double d[SCAN_K];
    for (int i = 0; i < K; ++i) {
        if (!(A[i][i] > 0.0)) return false;
        d[i] = std::sqrt(A[i][i]);
    }
    for (int i = 0; i < K; ++i)
        for (int j = 0; j <= i; ++j) A[i][j] /= d[i] * d[j];
    for (int j = 0; j < K; ++j) {
        double x = A[j][j];
        for (int k = 0; k < j; ++k) x -= A[j][k] * A[j][k];
        if (!(x > 1e-10)) return false;
        A[j][j] = std::sqrt(x);
        for (int i = j + 1; i < K; ++i) {
            double y = A[i][j];
            for (int k = 0; k < j; ++k) y -= A[i][k] * A[j][k];
            A[i][j] = y / A[j][j];
        }
    }
    return true;
}

}  // namespace

int draws_scan_accumulate(octo_draws* h, hipStream_t st, const double* inputs, double* g_in, double* ll, int64_t ldw, int64_t W, int32_t n_in) {
    const int32_t mode = h->scan_bound - 1, K = mode == OCTO_DRAWS_SCAN_MARGINAL ? 0 : h->scan_K;
    const double* x = inputs + (int64_t)n_in * ldw;
    double* gx = g_in ? g_in + (int64_t)n_in * ldw : nullptr;
    return scan_launch(h, st, mode, inputs, ldw, W, K ? x : nullptr, x + (int64_t)K * ldw, ll, g_in, K ? gx : nullptr, gx ? gx + (int64_t)K * ldw : nullptr, nullptr, 1);
}

extern "C" {

int32_t octo_draws_scan_clear(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    scan_drop_binding(h);
    h->scan_n = 0; h->scan_K = 0; h->scan_P = 0;
    return OCTO_OK;
}

int32_t octo_draws_scan_set(octo_draws* h, const octo_planet_desc* planets, int32_t n_planets, const octo_consts* consts, const double* t, const double* u,
                            const double* v, const double* y, const double* sigma, const double* c, int32_t K, int64_t n) {
    const std::string who = "octo_draws_scan_set: ";
    if (!h) return OCTO_EINVAL;
    if (n < 1 || n > 65536) return fail(h, OCTO_EINVAL, who + "need 1 <= n <= 65536 rows");
    if (K < 0 || K > SCAN_K) return fail(h, OCTO_EINVAL, who + "need 0 <= K <= OCTO_DRAWS_SCAN_MAX_K design columns");
    if (n_planets < 1 || n_planets > OCTO_MAX_PLANETS) return fail(h, OCTO_EINVAL, who + "need 1 <= n_planets <= OCTO_MAX_PLANETS");
    if (!planets || !t || !u || !v || !y || !sigma || (K > 0 && !c)) return fail(h, OCTO_EINVAL, who + "null argument");
    for (int p = 0; p < n_planets; ++p) {
        const int kind = planets[p].orbit_kind;
        if (kind != OCTO_ORBIT_VISUAL_KEP && kind != OCTO_ORBIT_RADVEL && kind != OCTO_ORBIT_THIELE_INNES && kind != OCTO_ORBIT_KEP)
            return fail(h, OCTO_EINVAL, who + "planet " + std::to_string(p) + ": unknown orbit kind " + std::to_string(kind));
    }
    std::vector<double> rows((size_t)n * ROWW, 0.0);
    for (int64_t r = 0; r < n; ++r) {
        bool fin = std::isfinite(t[r]) && std::isfinite(u[r]) && std::isfinite(v[r]) && std::isfinite(y[r]) && std::isfinite(sigma[r]);
        for (int k = 0; k < K; ++k) fin = fin && std::isfinite(c[(int64_t)k * n + r]);
        if (!fin) return fail(h, OCTO_EINVAL, who + "row " + std::to_string(r) + ": a non-finite entry");
        if (!(sigma[r] > 0.0)) return fail(h, OCTO_EINVAL, who + "row " + std::to_string(r) + ": sigma must be > 0");
        double* o = rows.data() + r * ROWW;
        o[0] = t[r]; o[1] = u[r]; o[2] = v[r]; o[3] = y[r]; o[4] = sigma[r] * sigma[r];
        for (int k = 0; k < K; ++k) o[5 + k] = c[(int64_t)k * n + r];
    }
    if (K > 0 && !scan_full_rank(c, sigma, K, n)) return fail(h, OCTO_EINVAL, who + "the design columns are rank deficient: C'Sigma^-1 C is not positive definite");
    octo_consts cst;
    if (consts) cst = *consts;
    else if (octo_consts_default(&cst) != OCTO_OK) return fail(h, OCTO_EINVAL, who + "octo_consts_default failed");
    OCHK(h, hipSetDevice(h->device));
    const size_t lds = scan_lds(n_planets, true);
    if (lds > 48 * 1024) {      // beyond the default limit: raised for the two kernels that keep the solutions
        for (const void* fn : {(const void*)k_scan_rows<true, 0>, (const void*)k_scan_rows<true, 2>})
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, OCTO_ENOTSUP, who + "the table's planets need more LDS per block than this device gives");
            }
    }
    octo_draws_scan_clear(h);
    if (int rc = grow(h, h->d_scan_rows, h->cap_scan_rows, (int64_t)rows.size())) return rc;
    OCHK(h, hipStreamSynchronize(h->stream));
    OCHK(h, hipMemcpy(h->d_scan_rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    h->scan_n = (int32_t)n; h->scan_K = K; h->scan_P = n_planets; h->scan_consts = cst;
    for (int p = 0; p < n_planets; ++p) { h->scan_kind[p] = planets[p].orbit_kind; h->scan_mass[p] = planets[p].has_mass ? 1 : 0; }
    return OCTO_OK;
}

int32_t octo_draws_scan_eval_device(octo_draws* h, int32_t mode, const double* d_elems, int64_t ld, int64_t W, const double* d_beta, const double* d_jitter,
                                    double* d_ll, double* d_g_elems, double* d_g_beta, double* d_g_jitter, double* d_beta_hat, int32_t accumulate,
                                    void* hip_stream) {
    const char* who = "octo_draws_scan_eval_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_scan_table(h, who)) return rc;
    if (int rc = check_scan_mode(h, who, mode)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    if (W == 0) return OCTO_OK;
    if (!d_elems || !d_ll) return fail(h, OCTO_EINVAL, std::string(who) + ": d_elems or d_ll is NULL");
    if (mode == OCTO_DRAWS_SCAN_SAMPLED && h->scan_K > 0 && !d_beta) return fail(h, OCTO_EINVAL, std::string(who) + ": d_beta is NULL (sampled mode with K > 0)");
    OCHK(h, hipSetDevice(h->device));
    return scan_launch(h, stream_of(h, hip_stream), mode, d_elems, ld, W, d_beta, d_jitter, d_ll, d_g_elems, d_g_beta, d_g_jitter, d_beta_hat, accumulate ? 1 : 0);
}

int32_t octo_draws_scan_eval(octo_draws* h, int32_t mode, const double* elems, int64_t ld, int64_t W, const double* beta, const double* jitter, double* ll,
                             double* g_elems, double* g_beta, double* g_jitter, double* beta_hat) {
    const char* who = "octo_draws_scan_eval";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_scan_table(h, who)) return rc;
    if (int rc = check_scan_mode(h, who, mode)) return rc;
    if (W < 0 || ld < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= W <= ld");
    if (W == 0) return OCTO_OK;
    if (!elems || !ll) return fail(h, OCTO_EINVAL, std::string(who) + ": elems or ll is NULL");
    const int64_t P = h->scan_P, K = h->scan_K, n_el = P * OCTO_N_EL;
    const bool sampled = mode == OCTO_DRAWS_SCAN_SAMPLED;
    if (sampled && K > 0 && !beta) return fail(h, OCTO_EINVAL, std::string(who) + ": beta is NULL (sampled mode with K > 0)");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    ScanStaging d;
    if (int rc = grow_to(h, h->d_scan_hst, h->cap_scan_hst, d, scan_staging, P, K, ld)) return rc;
    OCHK(h, hipMemcpyAsync(d.elems, elems, sizeof(double) * n_el * ld, hipMemcpyHostToDevice, st));
    if (sampled && K > 0) OCHK(h, hipMemcpyAsync(d.beta, beta, sizeof(double) * K * ld, hipMemcpyHostToDevice, st));
    if (jitter) OCHK(h, hipMemcpyAsync(d.jitter, jitter, sizeof(double) * W, hipMemcpyHostToDevice, st));
    const bool want_gb = sampled && g_beta && K > 0, want_bh = !sampled && beta_hat;
    if (int rc = octo_draws_scan_eval_device(h, mode, d.elems, ld, W, sampled && K > 0 ? d.beta : nullptr, jitter ? d.jitter : nullptr, d.ll, g_elems ? d.g_elems : nullptr,
                                             want_gb ? d.g_beta : nullptr, g_jitter ? d.g_jitter : nullptr, want_bh ? d.beta_hat : nullptr, 0, OCTO_STREAM_CTX)) return rc;
    OCHK(h, hipMemcpyAsync(ll, d.ll, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    if (g_elems) OCHK(h, hipMemcpyAsync(g_elems, d.g_elems, sizeof(double) * n_el * ld, hipMemcpyDeviceToHost, st));
    if (want_gb) OCHK(h, hipMemcpyAsync(g_beta, d.g_beta, sizeof(double) * K * ld, hipMemcpyDeviceToHost, st));
    if (g_jitter) OCHK(h, hipMemcpyAsync(g_jitter, d.g_jitter, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    if (want_bh) OCHK(h, hipMemcpyAsync(beta_hat, d.beta_hat, sizeof(double) * K * ld, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

int32_t octo_draws_scan_values_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_beta, double* d_eta, int64_t ld_out,
                                      void* hip_stream) {
    const char* who = "octo_draws_scan_values_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_scan_table(h, who)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    if (ld_out < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need ld_out >= W");
    if (W == 0) return OCTO_OK;
    if (!d_elems || !d_eta) return fail(h, OCTO_EINVAL, std::string(who) + ": d_elems or d_eta is NULL");
    OCHK(h, hipSetDevice(h->device));
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    ScanArgs a = scan_args(h, d_elems, ld, W, ldw);
    a.beta = d_beta; a.ldb = ld; a.eta = d_eta; a.ld_eta = ld_out;
    hipLaunchKernelGGL((k_scan_rows<false, 3>), dim3((unsigned)(ldw / WAVE), (unsigned)a.n_tasks), dim3(WAVE), scan_lds(a.P, false), stream_of(h, hip_stream), a);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_scan_unbind(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    scan_drop_binding(h);
    return OCTO_OK;
}

int32_t octo_draws_scan_bind(octo_draws* h, int32_t mode, const octo_draws_bind* binds, int32_t n_binds) {
    const char* who = "octo_draws_scan_bind";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_scan_table(h, who)) return rc;
    if (int rc = check_scan_mode(h, who, mode)) return rc;
    if (!h->prog_ops || !h->ctx) return fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no program (octo_draws_program_set)");
    if (h->pma_bound) return fail(h, OCTO_ENOTSUP, std::string(who) + ": a catalogue table is bound (octo_draws_pma_bind): one bound table a handle");
    if (h->gp_bound) return fail(h, OCTO_ENOTSUP, std::string(who) + ": a Gaussian-process RV table is bound (octo_draws_gp_bind): one bound table a handle");
    if (h->prog_planets != h->scan_P)
        return fail(h, OCTO_EINVAL, std::string(who) + ": the program has " + std::to_string(h->prog_planets) + " planets, the table " + std::to_string(h->scan_P));
    const int32_t want = mode == OCTO_DRAWS_SCAN_MARGINAL ? 1 : h->scan_K + 1;
    if (n_binds != want || !binds) return fail(h, OCTO_EINVAL, std::string(who) + ": need " + std::to_string(want) + " bindings (sampled: K + 1, marginal: 1)");
    const int N = h->D + h->prog_n_ops;
    for (int k = 0; k < n_binds; ++k) {
        if (binds[k].kind != OCTO_DRAWS_BIND_NODE) return fail(h, OCTO_EINVAL, std::string(who) + ": binding " + std::to_string(k) + " must be an OCTO_DRAWS_BIND_NODE");
        if (binds[k].node < 0 || binds[k].node >= N) return fail(h, OCTO_EINVAL, std::string(who) + ": binding " + std::to_string(k) + ": node out of range");
    }
    OCHK(h, hipSetDevice(h->device));
    scan_drop_binding(h);
    // the program's bindings and the bound nodes behind them, 16 bytes each: two doubles' room
    const int64_t n_all = (int64_t)h->prog_n_in + n_binds;
    if (int rc = grow(h, h->d_scan_binds, h->cap_scan_binds, 2 * n_all)) return rc;
    OCHK(h, hipStreamSynchronize(h->stream));
    octo_draws_bind* d = (octo_draws_bind*)h->d_scan_binds;
    OCHK(h, hipMemcpy(d, h->prog_binds, sizeof(octo_draws_bind) * (size_t)h->prog_n_in, hipMemcpyDeviceToDevice));
    OCHK(h, hipMemcpy(d + h->prog_n_in, binds, sizeof(octo_draws_bind) * (size_t)n_binds, hipMemcpyHostToDevice));
    h->scan_bound = 1 + mode; h->scan_n_bind = n_binds;
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->pf_W = 0; h->de_open = false; h->nest_passes = 0;
    return OCTO_OK;
}

}  // extern "C"
