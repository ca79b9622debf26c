// octo_draws_pma.hip — liboctofitter_hip_draws.so, the eighteenth part: the catalogue proper-motion anomaly from refitted scans (include/octofitter_hip_draws.h,
// "The eighteenth"): the star's reflex at every scan of a table, Q fixed linear maps of the reflex rows (each mission's refitted linear model, folded into
// the projector L by the host) and a Q × Q Gaussian against the catalogue values under their covariance. Of the main library's sources it INCLUDES the device
// routines the likelihood kernels run, as octo_draws_scan.hip does: the orbit constructor, the cold Kepler solve and the chain rule through the constructor
// are the code the main library runs. The matrices (Σ⁻¹, P_m, N⁻¹HᵀΣ⁻¹) and the constants are made once on the host (octo_draws_pma_host.h).
//
//   k_pma_rows     grid = (walker tiles of 64, tasks of OCTO_DRAWS_SCAN_ROWS rows), one wave a block, lane = walker; the rows and L are wave-uniform (scalar
//                  loads). Planet-outer: construct, solve the task's rows, add f_p·(u·ra + v·dec) into ρ [row][64] in LDS (4 KB); then Q fma chains
//                  z_q += L[q][i]·ρ_i in row order. Q partials a task.
//   k_pma_close    per walker: the tasks in task order, m = z + H·γ, r = d − m, λ = M·r, ℓ = −½·rᵀλ + c, ∂ℓ/∂γ = Hᵀλ or γ̂ = G·r, validity; λ and the
//                  validity stay in the work array. With a values output it stores m and nothing else.
//   k_pma_adj      the grid of k_pma_rows. The adjoint of ρ_i is g_i = Σ_q L[q][i]·λ_q, known from λ alone, so ONE planet-outer sweep: solve again, the ten
//                  sums of the planet against g_i in registers. No LDS. A call with a gradient makes two solves per (row, planet), a forward call one.
//   k_pma_finish   the tasks' sums in task order and planet_finish per planet: the sums to ∂ℓ/∂(a, e, i, ω, Ω, tp, M, plx, mass).
// Nothing is stored per (walker, row) in HBM, there is no atomic, and the row partition does not depend on W: a walker's bits depend on its column alone.
#include "octo_draws_common.h"

namespace pma_dev {      // the companions' device routines under a name of their own: that header and octo_draws_common.h both define a wave_sum
#include "octo_companion_device.h"
}

namespace {
using pma_dev::dev_consts;
using pma_dev::walker_setup;

constexpr int PMA_R = OCTO_DRAWS_SCAN_ROWS;
constexpr int PROWW = 4 + PMA_Q;               // a row record: {t, u, v, 0, L[0 … 7][i] (0 behind Q)}
constexpr int PL_N = 10;
using FinL = Layout<2, true, false, KM_RADEC>;      // the main library's sums of a planet with a mass term and no RV: U1 … U6, GE, GM, GT, GC
static_assert(FinL::PL_N == PL_N, "ten sums a planet");
static_assert(PMA_Q == OCTO_DRAWS_PMA_MAX_Q && PMA_K == OCTO_DRAWS_PMA_MAX_K, "octo_draws_pma_host.h and the public header");

struct PmaArgs {
    const double* rows;            // [n][PROWW]
    int32_t n, Q, K, P, accumulate, marginal, n_tasks, n_sums;
    int32_t orbit_kind[MAXP], has_mass[MAXP];
    DevConsts c;
    const double* elems; int64_t ld, W, ldw;
    const double* gamma;           // [K][ld] or null
    PmaWork k;
    double *ll, *g_elems, *g_gamma, *gamma_hat;
    double* m_out; int64_t ld_out;      // k_pma_close: the values output
};

struct PmaMats {      // what k_pma_close applies: the mode's M, and H, G, d, c
    double M[PMA_Q * PMA_Q], H[PMA_Q * PMA_K], G[PMA_K * PMA_Q], d[PMA_Q], cst;
};

__device__ __forceinline__ bool pma_contributes(const PmaArgs& a, int p) {      // wave-uniform: the scan part's reflex rule
    const int kind = a.orbit_kind[p];
    return (kind == OCTO_ORBIT_VISUAL_KEP || kind == OCTO_ORBIT_THIELE_INNES) && a.has_mass[p] != 0;
}

__global__ __launch_bounds__(WAVE) void k_pma_rows(PmaArgs a) {
    __shared__ __attribute__((aligned(16))) double rho_s[PMA_R * WAVE];
    const int lane = threadIdx.x, task = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;      // w < ldw: the work array has a column for every lane
    const int64_t wl = w < a.W ? w : a.W - 1;
    const int r0 = task * PMA_R, nr = min(PMA_R, a.n - r0), P = a.P;
    const double* __restrict__ rows = a.rows + (int64_t)r0 * PROWW;
    double* rho = rho_s + lane;
    for (int r = 0; r < nr; ++r) rho[r * WAVE] = 0.0;
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        if (!pma_contributes(a, p)) continue;
        double v[NWC];
        (void)walker_setup(a, p, wl, v);
        PC pc;
        load_pc(pc, v, 1, 0, 0);
        const double f = -v[WC_MU];
        for (int r = 0; r < nr; ++r) {
            const double* __restrict__ rw = rows + r * PROWW;
            const KSol ks = kepler_solve<2, false>(rw[0], pc);
            const double ra = fma(pc.cB, ks.cE, fma(pc.cGb, ks.sE, -pc.cBe));
            const double de = fma(pc.cA, ks.cE, fma(pc.cFb, ks.sE, -pc.cAe));
            rho[r * WAVE] = fma(f, fma(rw[1], ra, rw[2] * de), rho[r * WAVE]);
        }
    }
    double z[PMA_Q];
#pragma unroll
    for (int q = 0; q < PMA_Q; ++q) z[q] = 0.0;
    for (int r = 0; r < nr; ++r) {
        const double* __restrict__ rw = rows + r * PROWW;
        const double x = rho[r * WAVE];
#pragma unroll
        for (int q = 0; q < PMA_Q; ++q) z[q] = fma(rw[4 + q], x, z[q]);
    }
    double* part = a.k.part + (int64_t)task * a.n_sums * a.ldw + w;      // n_sums >= PMA_Q
#pragma unroll
    for (int q = 0; q < PMA_Q; ++q) part[(int64_t)q * a.ldw] = z[q];
}

__global__ __launch_bounds__(WAVE) void k_pma_close(PmaArgs a, PmaMats t) {
    const int64_t w = (int64_t)blockIdx.x * WAVE + threadIdx.x;      // w < ldw
    if (w >= a.W) {      // a lane behind the batch: k_pma_adj reads its column of λ
        if (!a.m_out) {
#pragma unroll
            for (int q = 0; q < PMA_Q; ++q) a.k.lam[(int64_t)q * a.ldw + w] = 0.0;
            a.k.ok[w] = 0.0;
        }
        return;
    }
    const int Q = a.Q, K = a.K;
    double m[PMA_Q], gam[PMA_K];
#pragma unroll
    for (int q = 0; q < PMA_Q; ++q) m[q] = 0.0;
    for (int tk = 0; tk < a.n_tasks; ++tk) {
        const double* part = a.k.part + (int64_t)tk * a.n_sums * a.ldw + w;
#pragma unroll
        for (int q = 0; q < PMA_Q; ++q) m[q] += part[(int64_t)q * a.ldw];      // the rows behind Q hold the sums of an all-zero L: 0, or NaN with an invalid walker
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < PMA_K; ++k) {
        gam[k] = (a.gamma && k < K) ? a.gamma[(int64_t)k * a.ld + w] : 0.0;
        ok = ok && isfinite(gam[k]);
    }
    if (!a.marginal || a.m_out) {
#pragma unroll
        for (int q = 0; q < PMA_Q; ++q)
#pragma unroll
            for (int k = 0; k < PMA_K; ++k) m[q] = fma(t.H[q * PMA_K + k], gam[k], m[q]);
    }
    if (a.m_out) {
#pragma unroll
        for (int q = 0; q < PMA_Q; ++q)
            if (q < Q) a.m_out[(int64_t)q * a.ld_out + w] = m[q];
        return;
    }
#pragma unroll 1
    for (int p = 0; p < a.P; ++p) {
        double elv[OCTO_N_EL];
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) elv[k] = a.elems[((int64_t)p * OCTO_N_EL + k) * a.ld + w];
        const SetupScalars s = setup_scalars<true>(elv, a.c, a.orbit_kind[p], a.has_mass[p]);
        ok = ok && setup_valid<true>(elv, a.orbit_kind[p], a.has_mass[p], s.sma);
    }
    double r[PMA_Q], lam[PMA_Q];
#pragma unroll
    for (int q = 0; q < PMA_Q; ++q) r[q] = q < Q ? t.d[q] - m[q] : 0.0;
    double quad = 0.0;
#pragma unroll
    for (int q = 0; q < PMA_Q; ++q) {
        double x = 0.0;
#pragma unroll
        for (int j = 0; j < PMA_Q; ++j) x = fma(t.M[q * PMA_Q + j], r[j], x);
        lam[q] = x;
        quad = fma(r[q], x, quad);
    }
    const double ll = fma(-0.5, quad, t.cst);
    ok = ok && isfinite(ll);
    a.ll[w] = (a.accumulate ? a.ll[w] : 0.0) + (ok ? ll : -INFINITY);
#pragma unroll
    for (int q = 0; q < PMA_Q; ++q) a.k.lam[(int64_t)q * a.ldw + w] = ok ? lam[q] : 0.0;
    a.k.ok[w] = ok ? 1.0 : 0.0;
    if (a.marginal) {
        if (a.gamma_hat) {
#pragma unroll
            for (int k = 0; k < PMA_K; ++k) {
                double x = 0.0;
#pragma unroll
                for (int q = 0; q < PMA_Q; ++q) x = fma(t.G[k * PMA_Q + q], r[q], x);
                if (k < K) a.gamma_hat[(int64_t)k * a.ld + w] = x;
            }
        }
    } else if (a.g_gamma) {
#pragma unroll
        for (int k = 0; k < PMA_K; ++k) {
            double x = 0.0;
#pragma unroll
            for (int q = 0; q < PMA_Q; ++q) x = fma(t.H[q * PMA_K + k], lam[q], x);
            if (k < K) a.g_gamma[(int64_t)k * a.ld + w] = ok ? x : 0.0;
        }
    }
}

// a planet's ten sums against g_i: the running sums of the main library's astrom_row with r̄a = g·u, d̄ec = g·v, as sweep B of k_scan_rows forms them
__global__ __launch_bounds__(WAVE) void k_pma_adj(PmaArgs a) {
    const int lane = threadIdx.x, task = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * WAVE + lane;
    const int64_t wl = w < a.W ? w : a.W - 1;
    const int r0 = task * PMA_R, nr = min(PMA_R, a.n - r0), P = a.P;
    const double* __restrict__ rows = a.rows + (int64_t)r0 * PROWW;
    double lam[PMA_Q];
#pragma unroll
    for (int q = 0; q < PMA_Q; ++q) lam[q] = a.k.lam[(int64_t)q * a.ldw + w];
    double* part = a.k.part + (int64_t)task * a.n_sums * a.ldw + w;
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
        double g[PL_N];
#pragma unroll
        for (int k = 0; k < PL_N; ++k) g[k] = 0.0;
        if (pma_contributes(a, p)) {
            double v[NWC];
            (void)walker_setup(a, p, wl, v);
            PC pc;
            load_pc(pc, v, 1, 0, 0);
            const double f = -v[WC_MU];
            for (int r = 0; r < nr; ++r) {
                const double* __restrict__ rw = rows + r * PROWW;
                double hh = 0.0;
#pragma unroll
                for (int q = 0; q < PMA_Q; ++q) hh = fma(rw[4 + q], lam[q], hh);
                const KSol ks = kepler_solve<2, false>(rw[0], pc);
                const double sE = ks.sE, cE = ks.cE;
                const double rab = hh * rw[1], deb = hh * rw[2];
                const double ra_f = f * rab, de_f = f * deb;
                g[FinL::U1] = fma(cE, ra_f, g[FinL::U1]);
                g[FinL::U2] = fma(sE, ra_f, g[FinL::U2]);
                g[FinL::U3] = fma(cE, de_f, g[FinL::U3]);
                g[FinL::U4] = fma(sE, de_f, g[FinL::U4]);
                g[FinL::U5] += ra_f;
                g[FinL::U6] += de_f;
                const double rap = fma(pc.cB, cE, fma(pc.cGb, sE, -pc.cBe)), dep = fma(pc.cA, cE, fma(pc.cFb, sE, -pc.cAe));
                g[FinL::GC] -= fma(rab, rap, deb * dep);      // ∂ℓ/∂(m/M): f = −m/M
                const double dra = fma(pc.cGb, cE, -(pc.cB * sE)), dde = fma(pc.cFb, cE, -(pc.cA * sE));
                const double Mb = fma(ra_f, dra, de_f * dde) * ks.invD;
                g[FinL::GE] = fma(Mb, sE, g[FinL::GE]);
                g[FinL::GM] += Mb;
                g[FinL::GT] = fma(Mb, rw[0] - pc.tp, g[FinL::GT]);
            }
        }
#pragma unroll
        for (int k = 0; k < PL_N; ++k) part[(int64_t)(p * PL_N + k) * a.ldw] = g[k];
    }
}

__global__ __launch_bounds__(WAVE) void k_pma_finish(PmaArgs a) {
    const int64_t w = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (w >= a.W) return;
    const bool ok = a.k.ok[w] != 0.0;
#pragma unroll 1
    for (int p = 0; p < a.P; ++p) {
        double out[OCTO_N_EL];
#pragma unroll
        for (int k = 0; k < OCTO_N_EL; ++k) out[k] = 0.0;
        if (ok && pma_contributes(a, p)) {
            double g[PL_N];
#pragma unroll
            for (int k = 0; k < PL_N; ++k) g[k] = 0.0;
            for (int t = 0; t < a.n_tasks; ++t) {
                const double* part = a.k.part + ((int64_t)t * a.n_sums + p * PL_N) * a.ldw + w;
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

inline int check_pma_table(octo_draws* h, const char* who) {
    return h->pma_n > 0 ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no catalogue table (octo_draws_pma_set)");
}
inline int check_pma_mode(octo_draws* h, const char* who, int32_t mode) {
    if (mode != OCTO_DRAWS_PMA_SAMPLED && mode != OCTO_DRAWS_PMA_MARGINAL) return fail(h, OCTO_EINVAL, std::string(who) + ": mode must be OCTO_DRAWS_PMA_SAMPLED or OCTO_DRAWS_PMA_MARGINAL");
    if (mode == OCTO_DRAWS_PMA_MARGINAL && h->pma_K == 0) return fail(h, OCTO_EINVAL, std::string(who) + ": the marginal mode needs K >= 1 linear parameters");
    return mode == OCTO_DRAWS_PMA_MARGINAL && !h->pma_tab.marg_ok ? fail(h, OCTO_EINVAL, std::string(who) + ": the marginal mode needs H'Sigma^-1 H positive definite: H is rank deficient") : OCTO_OK;
}

void pma_drop_binding(octo_draws* h) {
    if (!h->pma_bound) return;
    h->pma_bound = 0; h->pma_n_bind = 0;
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->pf_W = 0; h->de_open = false; h->nest_passes = 0;      // a transition is never resumed on another target
}

PmaArgs pma_args(const octo_draws* h, const double* d_elems, int64_t ld, int64_t W, int64_t ldw) {
    PmaArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = h->d_pma_rows; a.n = h->pma_n; a.Q = h->pma_Q; a.K = h->pma_K; a.P = h->pma_P;
    for (int p = 0; p < h->pma_P; ++p) { a.orbit_kind[p] = h->pma_kind[p]; a.has_mass[p] = h->pma_mass[p]; }
    a.c = dev_consts(h->pma_consts);
    a.elems = d_elems; a.ld = ld; a.W = W; a.ldw = ldw;
    a.n_tasks = (h->pma_n + PMA_R - 1) / PMA_R;
    a.n_sums = std::max(PMA_Q, PL_N * a.P);
    return a;
}

PmaMats pma_mats(const octo_draws* h, int32_t mode) {
    PmaMats t;
    const PmaTable& s = h->pma_tab;
    std::memcpy(t.M, s.M[mode], sizeof(t.M)); std::memcpy(t.H, s.H, sizeof(t.H)); std::memcpy(t.G, s.G, sizeof(t.G)); std::memcpy(t.d, s.d, sizeof(t.d));
    t.cst = s.cst[mode];
    return t;
}

// the launches of one evaluation on st; the rows of d_gamma, d_g_gamma and d_gamma_hat are ld apart
int pma_launch(octo_draws* h, hipStream_t st, int32_t mode, const double* d_elems, int64_t ld, int64_t W, const double* d_gamma, double* d_ll, double* d_g_elems,
               double* d_g_gamma, double* d_gamma_hat, int32_t accumulate) {
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    PmaArgs a = pma_args(h, d_elems, ld, W, ldw);
    if (int rc = grow_to(h, h->d_pma, h->cap_pma, a.k, pma_work, (int64_t)a.n_tasks, (int64_t)a.n_sums, ldw)) return rc;
    const bool marginal = mode == OCTO_DRAWS_PMA_MARGINAL;
    a.gamma = marginal ? nullptr : d_gamma; a.accumulate = accumulate; a.marginal = marginal;
    a.ll = d_ll; a.g_elems = d_g_elems; a.g_gamma = marginal ? nullptr : d_g_gamma; a.gamma_hat = marginal ? d_gamma_hat : nullptr;
    const dim3 grid((unsigned)(ldw / WAVE), (unsigned)a.n_tasks), tiles((unsigned)(ldw / WAVE)), block(WAVE);
    hipLaunchKernelGGL(k_pma_rows, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_pma_close, tiles, block, 0, st, a, pma_mats(h, mode));
    if (d_g_elems) {
        hipLaunchKernelGGL(k_pma_adj, grid, block, 0, st, a);
        hipLaunchKernelGGL(k_pma_finish, tiles, block, 0, st, a);
    }
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

}  // namespace

int draws_pma_accumulate(octo_draws* h, hipStream_t st, const double* inputs, double* g_in, double* ll, int64_t ldw, int64_t W, int32_t n_in) {
    const int32_t mode = h->pma_bound - 1, K = mode == OCTO_DRAWS_PMA_MARGINAL ? 0 : h->pma_K;
    const double* x = inputs + (int64_t)n_in * ldw;
    double* gx = g_in ? g_in + (int64_t)n_in * ldw : nullptr;
    return pma_launch(h, st, mode, inputs, ldw, W, K ? x : nullptr, ll, g_in, K ? gx : nullptr, nullptr, 1);
}

extern "C" {

int32_t octo_draws_pma_clear(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    pma_drop_binding(h);
    h->pma_n = 0; h->pma_Q = 0; h->pma_K = 0; h->pma_P = 0;
    return OCTO_OK;
}

int32_t octo_draws_pma_set(octo_draws* h, const octo_planet_desc* planets, int32_t n_planets, const octo_consts* consts, const double* t, const double* u,
                           const double* v, const double* L, int32_t Q, const double* d, const double* cov, const double* H, int32_t K, int64_t n) {
    const std::string who = "octo_draws_pma_set: ";
    if (!h) return OCTO_EINVAL;
    if (n < 1 || n > 65536) return fail(h, OCTO_EINVAL, who + "need 1 <= n <= 65536 rows");
    if (Q < 1 || Q > PMA_Q) return fail(h, OCTO_EINVAL, who + "need 1 <= Q <= OCTO_DRAWS_PMA_MAX_Q catalogue values");
    if (K < 0 || K > PMA_K) return fail(h, OCTO_EINVAL, who + "need 0 <= K <= OCTO_DRAWS_PMA_MAX_K linear parameters");
    if (n_planets < 1 || n_planets > OCTO_MAX_PLANETS) return fail(h, OCTO_EINVAL, who + "need 1 <= n_planets <= OCTO_MAX_PLANETS");
    if (!planets || !t || !u || !v || !L || !d || !cov || (K > 0 && !H)) return fail(h, OCTO_EINVAL, who + "null argument");
    for (int p = 0; p < n_planets; ++p) {
        const int kind = planets[p].orbit_kind;
        if (kind != OCTO_ORBIT_VISUAL_KEP && kind != OCTO_ORBIT_RADVEL && kind != OCTO_ORBIT_THIELE_INNES && kind != OCTO_ORBIT_KEP)
            return fail(h, OCTO_EINVAL, who + "planet " + std::to_string(p) + ": unknown orbit kind " + std::to_string(kind));
    }
    std::vector<double> rows((size_t)n * PROWW, 0.0);
    for (int64_t r = 0; r < n; ++r) {
        bool fin = std::isfinite(t[r]) && std::isfinite(u[r]) && std::isfinite(v[r]);
        for (int q = 0; q < Q; ++q) fin = fin && std::isfinite(L[(int64_t)q * n + r]);
        if (!fin) return fail(h, OCTO_EINVAL, who + "row " + std::to_string(r) + ": a non-finite entry");
        double* o = rows.data() + r * PROWW;
        o[0] = t[r]; o[1] = u[r]; o[2] = v[r];
        for (int q = 0; q < Q; ++q) o[4 + q] = L[(int64_t)q * n + r];
    }
    bool fin = true;
    for (int q = 0; q < Q; ++q) {
        fin = fin && std::isfinite(d[q]);
        for (int j = 0; j < Q; ++j) fin = fin && std::isfinite(cov[q * Q + j]);
        for (int k = 0; k < K; ++k) fin = fin && std::isfinite(H[q * K + k]);
    }
    if (!fin) return fail(h, OCTO_EINVAL, who + "a non-finite entry of d, cov or H");
    PmaTable tab;
    if (const int bad = pma_table_build(cov, H, d, Q, K, &tab))
        return fail(h, OCTO_EINVAL, who + (bad == 1 ? "the covariance is not symmetric" : "the covariance is not positive definite"));
    octo_consts cst;
    if (consts) cst = *consts;
    else if (octo_consts_default(&cst) != OCTO_OK) return fail(h, OCTO_EINVAL, who + "octo_consts_default failed");
    OCHK(h, hipSetDevice(h->device));
    octo_draws_pma_clear(h);
    if (int rc = grow(h, h->d_pma_rows, h->cap_pma_rows, (int64_t)rows.size())) return rc;
    OCHK(h, hipStreamSynchronize(h->stream));
    OCHK(h, hipMemcpy(h->d_pma_rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    h->pma_n = (int32_t)n; h->pma_Q = Q; h->pma_K = K; h->pma_P = n_planets; h->pma_consts = cst; h->pma_tab = tab;
    for (int p = 0; p < n_planets; ++p) { h->pma_kind[p] = planets[p].orbit_kind; h->pma_mass[p] = planets[p].has_mass ? 1 : 0; }
    return OCTO_OK;
}

int32_t octo_draws_pma_eval_device(octo_draws* h, int32_t mode, const double* d_elems, int64_t ld, int64_t W, const double* d_gamma, double* d_ll,
                                   double* d_g_elems, double* d_g_gamma, double* d_gamma_hat, int32_t accumulate, void* hip_stream) {
    const char* who = "octo_draws_pma_eval_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_pma_table(h, who)) return rc;
    if (int rc = check_pma_mode(h, who, mode)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    if (W == 0) return OCTO_OK;
    if (!d_elems || !d_ll) return fail(h, OCTO_EINVAL, std::string(who) + ": d_elems or d_ll is NULL");
    if (mode == OCTO_DRAWS_PMA_SAMPLED && h->pma_K > 0 && !d_gamma) return fail(h, OCTO_EINVAL, std::string(who) + ": d_gamma is NULL (sampled mode with K > 0)");
    OCHK(h, hipSetDevice(h->device));
    return pma_launch(h, stream_of(h, hip_stream), mode, d_elems, ld, W, h->pma_K ? d_gamma : nullptr, d_ll, d_g_elems, h->pma_K ? d_g_gamma : nullptr,
                      d_gamma_hat, accumulate ? 1 : 0);
}

int32_t octo_draws_pma_eval(octo_draws* h, int32_t mode, const double* elems, int64_t ld, int64_t W, const double* gamma, double* ll, double* g_elems,
                            double* g_gamma, double* gamma_hat) {
    const char* who = "octo_draws_pma_eval";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_pma_table(h, who)) return rc;
    if (int rc = check_pma_mode(h, who, mode)) return rc;
    if (W < 0 || ld < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= W <= ld");
    if (W == 0) return OCTO_OK;
    if (!elems || !ll) return fail(h, OCTO_EINVAL, std::string(who) + ": elems or ll is NULL");
    const int64_t P = h->pma_P, K = h->pma_K, n_el = P * OCTO_N_EL;
    const bool sampled = mode == OCTO_DRAWS_PMA_SAMPLED;
    if (sampled && K > 0 && !gamma) return fail(h, OCTO_EINVAL, std::string(who) + ": gamma is NULL (sampled mode with K > 0)");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    PmaStaging d;
    if (int rc = grow_to(h, h->d_pma_hst, h->cap_pma_hst, d, pma_staging, P, K, ld)) return rc;
    OCHK(h, hipMemcpyAsync(d.elems, elems, sizeof(double) * n_el * ld, hipMemcpyHostToDevice, st));
    if (sampled && K > 0) OCHK(h, hipMemcpyAsync(d.gamma, gamma, sizeof(double) * K * ld, hipMemcpyHostToDevice, st));
    const bool want_gg = sampled && g_gamma && K > 0, want_gh = !sampled && gamma_hat;
    if (int rc = octo_draws_pma_eval_device(h, mode, d.elems, ld, W, sampled && K > 0 ? d.gamma : nullptr, d.ll, g_elems ? d.g_elems : nullptr,
                                            want_gg ? d.g_gamma : nullptr, want_gh ? d.gamma_hat : nullptr, 0, OCTO_STREAM_CTX)) return rc;
    OCHK(h, hipMemcpyAsync(ll, d.ll, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    if (g_elems) OCHK(h, hipMemcpyAsync(g_elems, d.g_elems, sizeof(double) * n_el * ld, hipMemcpyDeviceToHost, st));
    if (want_gg) OCHK(h, hipMemcpyAsync(g_gamma, d.g_gamma, sizeof(double) * K * ld, hipMemcpyDeviceToHost, st));
    if (want_gh) OCHK(h, hipMemcpyAsync(gamma_hat, d.gamma_hat, sizeof(double) * K * ld, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

int32_t octo_draws_pma_values_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_gamma, double* d_m, int64_t ld_out,
                                     void* hip_stream) {
    const char* who = "octo_draws_pma_values_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_pma_table(h, who)) return rc;
    if (int rc = check_chains(h, who, W, ld, MAX_CHAINS, "2^30")) return rc;
    if (ld_out < W) return fail(h, OCTO_EINVAL, std::string(who) + ": need ld_out >= W");
    if (W == 0) return OCTO_OK;
    if (!d_elems || !d_m) return fail(h, OCTO_EINVAL, std::string(who) + ": d_elems or d_m is NULL");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = stream_of(h, hip_stream);
    const int64_t ldw = (W + WAVE - 1) / WAVE * WAVE;
    PmaArgs a = pma_args(h, d_elems, ld, W, ldw);
    if (int rc = grow_to(h, h->d_pma, h->cap_pma, a.k, pma_work, (int64_t)a.n_tasks, (int64_t)a.n_sums, ldw)) return rc;
    a.gamma = h->pma_K ? d_gamma : nullptr; a.m_out = d_m; a.ld_out = ld_out;
    hipLaunchKernelGGL(k_pma_rows, dim3((unsigned)(ldw / WAVE), (unsigned)a.n_tasks), dim3(WAVE), 0, st, a);
    hipLaunchKernelGGL(k_pma_close, dim3((unsigned)(ldw / WAVE)), dim3(WAVE), 0, st, a, pma_mats(h, OCTO_DRAWS_PMA_SAMPLED));
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_pma_unbind(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    pma_drop_binding(h);
    return OCTO_OK;
}

int32_t octo_draws_pma_bind(octo_draws* h, int32_t mode, const octo_draws_bind* binds, int32_t n_binds) {
    const char* who = "octo_draws_pma_bind";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_pma_table(h, who)) return rc;
    if (int rc = check_pma_mode(h, who, mode)) return rc;
    if (!h->prog_ops || !h->ctx) return fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no program (octo_draws_program_set)");
    if (h->scan_bound) return fail(h, OCTO_ENOTSUP, std::string(who) + ": a scan table is bound (octo_draws_scan_bind): one bound table a handle");
    if (h->gp_bound) return fail(h, OCTO_ENOTSUP, std::string(who) + ": a Gaussian-process RV table is bound (octo_draws_gp_bind): one bound table a handle");
    if (h->prog_planets != h->pma_P)
        return fail(h, OCTO_EINVAL, std::string(who) + ": the program has " + std::to_string(h->prog_planets) + " planets, the table " + std::to_string(h->pma_P));
    const int32_t want = mode == OCTO_DRAWS_PMA_MARGINAL ? 0 : h->pma_K;
    if (n_binds != want || (want > 0 && !binds)) return fail(h, OCTO_EINVAL, std::string(who) + ": need " + std::to_string(want) + " bindings (sampled: K, marginal: 0)");
    const int N = h->D + h->prog_n_ops;
    for (int k = 0; k < n_binds; ++k) {
        if (binds[k].kind != OCTO_DRAWS_BIND_NODE) return fail(h, OCTO_EINVAL, std::string(who) + ": binding " + std::to_string(k) + " must be an OCTO_DRAWS_BIND_NODE");
        if (binds[k].node < 0 || binds[k].node >= N) return fail(h, OCTO_EINVAL, std::string(who) + ": binding " + std::to_string(k) + ": node out of range");
    }
    OCHK(h, hipSetDevice(h->device));
    pma_drop_binding(h);
    // the program's bindings and the bound nodes behind them, 16 bytes each: two doubles' room
    const int64_t n_all = (int64_t)h->prog_n_in + n_binds;
    if (int rc = grow(h, h->d_pma_binds, h->cap_pma_binds, 2 * n_all)) return rc;
    OCHK(h, hipStreamSynchronize(h->stream));
    octo_draws_bind* d = (octo_draws_bind*)h->d_pma_binds;
    OCHK(h, hipMemcpy(d, h->prog_binds, sizeof(octo_draws_bind) * (size_t)h->prog_n_in, hipMemcpyDeviceToDevice));
    if (n_binds > 0) OCHK(h, hipMemcpy(d + h->prog_n_in, binds, sizeof(octo_draws_bind) * (size_t)n_binds, hipMemcpyHostToDevice));
    h->pma_bound = 1 + mode; h->pma_n_bind = n_binds;
    h->nuts_depth = 0; h->slice_passes = 0; h->lbf_m = 0; h->pf_W = 0; h->de_open = false; h->nest_passes = 0;
    return OCTO_OK;
}

}  // extern "C"
