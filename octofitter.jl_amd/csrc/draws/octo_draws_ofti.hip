// octo_draws_ofti.hip — the OFTI rejection sampler, the sixteenth part of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h states it): prior
// draws of (e, a, tp | τ, M, plx) scored by the main library's OFTI marginal likelihood (octo_ofti_eval_device: a client of the public ABI, as the
// model path is), the rejection step of octo_draws_rejection, and for every survivor a draw of the Thiele-Innes constants with its Campbell elements.
//
//   k_oftis_nl     θ -> nl: four rows copied, the third tp itself or fma(τ, P_d, t_ref). 80 bytes a draw.
//   k_oftis_ll     ℓ in place (not finite -> −Inf) and the block maxima: the input of pass 2 (k_max … k_scatter of octo_draws.hip, unchanged).
//   k_oftis_post   lane = draw: the 13 sums over the table's rows in row order — the rows through wave-uniform (scalar) loads as k_ofti_main reads
//                  them, the COLD Kepler solve kepler_solve<-1, false> of octo_device.h (Markley's starter, the fifth-order correction, the half-angle
//                  polynomial sin/cos: no table in LDS, so a lane with e >= 1 or NaN elements indexes nothing) — then S, its Cholesky factor, μ and ℓ as
//                  k_ofti_finish forms them, four normals of purpose 13, x = μ + L⁻ᵀz, and the elements of x. It runs on the ACCEPTED draws only
//                  (hundreds to thousands of a million), so its rate is not the driver's: pass 1 is k_ofti_main's.
// Nothing of a draw is stored for all N but ℓ (8 bytes): θ and nl live a chunk at a time and are regenerated from the counter for the survivors.
#include "octo_draws_common.h"

namespace {

constexpr int64_t CHUNK = 1 << 18;      // draws per octo_ofti_eval_device call: octo_draws_rejection's, a multiple of TPB
static_assert(CHUNK % TPB == 0, "chunk boundaries are block boundaries of the rejection pass");

// P_d of k_ofti_main (octo_kernels.h, parameterizations.jl:322)
__device__ __forceinline__ double period_days(double k_yr, double sma, double Mt) { return k_yr * sqrt(sma * sma * sma / Mt); }

__global__ __launch_bounds__(TPB) void k_oftis_nl(const double* __restrict__ theta, double* __restrict__ nl, int64_t n, int64_t ld, int32_t tp_mode, double t_ref,
                                                  double k_yr) {
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (k >= n) return;
    const double e = theta[k], sma = theta[ld + k], third = theta[2 * ld + k], Mt = theta[3 * ld + k], plx = theta[4 * ld + k];
    nl[k] = e; nl[ld + k] = sma; nl[3 * ld + k] = Mt; nl[4 * ld + k] = plx;
    nl[2 * ld + k] = tp_mode ? fma(third, period_days(k_yr, sma, Mt), t_ref) : third;
}

// ll[k] <- −Inf where it is not finite; pmax[block] = the block's maximum
__global__ __launch_bounds__(TPB) void k_oftis_ll(double* __restrict__ ll, int64_t n, double* __restrict__ pmax) {
    __shared__ double s[TPB / WAVE];
    const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double v = -INFINITY;
    if (k < n) {
        v = ll[k];
        v = isfinite(v) ? v : -INFINITY;
        ll[k] = v;
    }
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = s[0];
#pragma unroll
        for (int w = 1; w < TPB / WAVE; ++w) v = fmax(v, s[w]);
        pmax[blockIdx.x] = v;
    }
}

struct PostArgs {
    const double* rows;       // [n_rows][8] {t, w_rr, w_dd, w_rd, p, q, 0, 0}: OftiArgs::rows
    const uint64_t* idx;      // [n]
    const double* nl;         // [5][ld]
    double* out;              // [OCTO_DRAWS_OFTI_N_OUT][ld]
    int64_t n, ld;
    uint64_t seed;
    int32_t n_rows, pad;
    double k_yr, lambda, data_quad, log_det_data_cov, log_det_prior_inv, n_log2pi;
};

__global__ __launch_bounds__(TPB) void k_oftis_post(PostArgs a) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= a.n) return;      // nothing below votes or exchanges across the wave
    const double e = a.nl[t], sma = a.nl[a.ld + t], tp = a.nl[2 * a.ld + t], Mt = a.nl[3 * a.ld + t], plx = a.nl[4 * a.ld + t];
    const double P_d = period_days(a.k_yr, sma, Mt);
    PC pc = {};
    pc.invP = 1.0 / P_d; pc.tp = tp; pc.e = e; pc.beta = sqrt(1.0 - e * e);
    set_starter<false>(pc, (float)e, (float)(1.0 - e), (float)(MK_K1N / (1.0 + e)));
    double v[OFTI_NACC];
#pragma unroll
    for (int k = 0; k < OFTI_NACC; ++k) v[k] = 0.0;
    const crow_t rows = constant_rows(a.rows);
    for (int j = 0; j < a.n_rows; ++j) {
        const crow_t rw = rows + (int64_t)j * ROW_STRIDE;
        const double tj = rw[0], wrr = rw[1], wdd = rw[2], wrd = rw[3], pp = rw[4], qq = rw[5];
        const KSol s = kepler_solve<-1, false>(tj, pc);
        const double x = s.cE - pc.e, y = s.sE * pc.beta;
        const double xx = x * x, xy = x * y, yy = y * y;
        v[0] = fma(wrr, xx, v[0]); v[1] = fma(wrr, xy, v[1]); v[2] = fma(wrr, yy, v[2]);
        v[3] = fma(wdd, xx, v[3]); v[4] = fma(wdd, xy, v[4]); v[5] = fma(wdd, yy, v[5]);
        v[6] = fma(wrd, xx, v[6]); v[7] = fma(wrd, xy, v[7]); v[8] = fma(wrd, yy, v[8]);
        v[9] = fma(x, qq, v[9]); v[10] = fma(y, qq, v[10]);
        v[11] = fma(x, pp, v[11]); v[12] = fma(y, pp, v[12]);
    }
    // ---- S, L, μ, ℓ: k_ofti_finish (octo_kernels.h), operation for operation
    const bool ok = isfinite(e) && isfinite(sma) && isfinite(tp) && isfinite(Mt) && isfinite(plx) && e >= 0.0 && e < 1.0 && sma > 0.0 && Mt > 0.0;
    const double lam = a.lambda;
    double S[4][4];
    S[0][0] = v[3] + lam; S[0][1] = v[6]; S[0][2] = v[4]; S[0][3] = v[7];
    S[1][1] = v[0] + lam; S[1][2] = v[7]; S[1][3] = v[1];
    S[2][2] = v[5] + lam; S[2][3] = v[8];
    S[3][3] = v[2] + lam;
    const double b[4] = {v[9], v[11], v[10], v[12]};
    double L[4][4];
    bool pd = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double sum = S[j][i];
#pragma unroll
            for (int k = 0; k < j; ++k) sum -= L[i][k] * L[j][k];
            if (i == j) { pd = pd && (sum > 0.0); L[i][i] = sqrt(sum); }
            else L[i][j] = sum / L[j][j];
        }
    }
    double z[4], mu[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sum = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum -= L[i][k] * z[k];
        z[i] = sum / L[i][i];
    }
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        double sum = z[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) sum -= L[k][i] * mu[k];
        mu[i] = sum / L[i][i];
    }
    const double post_quad = z[0] * z[0] + z[1] * z[1] + z[2] * z[2] + z[3] * z[3];
    const double log_det_post_inv = 2.0 * (log(L[0][0]) + log(L[1][1]) + log(L[2][2]) + log(L[3][3]));
    const double lm = -0.5 * (a.data_quad - post_quad + log_det_post_inv - a.log_det_prior_inv + a.log_det_data_cov) - a.n_log2pi;
    const bool fin = ok && pd && isfinite(lm);
    // ---- the draw: x = μ + L⁻ᵀ·z, z the four normals of purpose 13
    uint64_t r[4];
    philox4x64(a.seed, KEY1, a.idx[t], 0, OCTO_DRAWS_PURPOSE_OFTI, 0, r);
    double g[4], x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = normcdfinv(u01(r[k]));
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        double sum = g[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) sum -= L[k][i] * x[k];
        x[i] = sum / L[i][i];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] += mu[k];
    // ---- the elements of the draw
    const double A = x[0], B = x[1], F = x[2], G = x[3];
    const double apg = A + G, bmf = B - F, amg = A - G, bpf = B + F;
    const double sp = sqrt(0.5 * fma(apg, apg, bmf * bmf)), sm = sqrt(0.5 * fma(amg, amg, bpf * bpf));      // √(u+v), √(u−v)
    const double alpha = (sp + sm) * 0.70710678118654752440;
    const double cosi = (sp - sm) / (sp + sm);
    const double inc = acos(cosi);
    const double wpo = atan2(bmf, apg), wmo = atan2(-bpf, amg);
    double om = 0.5 * (wpo + wmo), Om = 0.5 * (wpo - wmo);
    if (Om < 0.0) { Om += PI; om += PI; }
    else if (Om >= PI) { Om -= PI; om -= PI; }
    if (om < 0.0) om += TWO_PI;
    else if (om >= TWO_PI) om -= TWO_PI;
    const double a_ti = alpha / plx;
    const double ratio = a_ti / sma;
    const double M_dyn = Mt * (ratio * ratio * ratio);
    const double o[OCTO_DRAWS_OFTI_N_OUT] = {A, B, F, G, mu[0], mu[1], mu[2], mu[3], alpha, a_ti, inc, om, Om, P_d, M_dyn, 0.0};
#pragma unroll
    for (int k = 0; k < OCTO_DRAWS_OFTI_N_OUT - 1; ++k) a.out[(int64_t)k * a.ld + t] = fin ? o[k] : NAN;
    a.out[(int64_t)(OCTO_DRAWS_OFTI_N_OUT - 1) * a.ld + t] = fin ? lm : -INFINITY;
}

int check_set(octo_draws* h, const char* who) {
    return h->ofti ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": no table is set (octo_draws_ofti_set)");
}

int check_batch(octo_draws* h, const char* who, int64_t n, int64_t ld, bool arrays) {
    if (n < 0 || ld < n) return fail(h, OCTO_EINVAL, std::string(who) + ": need 0 <= n <= ld");
    return n == 0 || arrays ? OCTO_OK : fail(h, OCTO_EINVAL, std::string(who) + ": null array");
}

void launch_nl(const octo_draws* h, hipStream_t st, int64_t n, int64_t ld, const double* d_theta, double* d_nl) {
    hipLaunchKernelGGL(k_oftis_nl, grid_of(n), dim3(TPB), 0, st, d_theta, d_nl, n, ld, h->oftis_tp_mode, h->oftis_t_ref, h->oftis_k_yr);
}

void launch_post(const octo_draws* h, hipStream_t st, uint64_t seed, int64_t n, int64_t ld, const uint64_t* d_index, const double* d_nl, double* d_out) {
    PostArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = h->d_oftis_rows; a.idx = d_index; a.nl = d_nl; a.out = d_out; a.n = n; a.ld = ld; a.seed = seed; a.n_rows = h->oftis_n_rows;
    a.k_yr = h->oftis_k_yr; a.lambda = h->oftis_lambda; a.data_quad = h->oftis_data_quad; a.log_det_data_cov = h->oftis_log_det_data_cov;
    a.log_det_prior_inv = h->oftis_log_det_prior_inv; a.n_log2pi = h->oftis_n_log2pi;
    hipLaunchKernelGGL(k_oftis_post, grid_of(n), dim3(TPB), 0, st, a);
}

}  // namespace

extern "C" {

int32_t octo_draws_ofti_clear(octo_draws* h) {
    if (!h) return OCTO_EINVAL;
    if (!h->ofti) return OCTO_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)octo_ofti_destroy(h->ofti);
    h->ofti = nullptr;
    h->oftis_n_rows = 0;
    return OCTO_OK;
}

int32_t octo_draws_ofti_set(octo_draws* h, const double* epochs, const double* ra, const double* dec, const double* sigma_ra, const double* sigma_dec,
                            const double* cor, int64_t n_epochs, double sigma_abfg, int32_t tp_mode, double t_ref, const octo_consts* consts) {
    const char* who = "octo_draws_ofti_set";
    if (!h) return OCTO_EINVAL;
    if (h->D != 5) return fail(h, OCTO_EINVAL, std::string(who) + ": the handle must have D = 5 priors: e, a, tp or tau, M, plx");
    if (!h->ctx) return fail(h, OCTO_EINVAL, std::string(who) + ": the handle has no context (detached)");
    if (tp_mode != 0 && tp_mode != 1) return fail(h, OCTO_EINVAL, std::string(who) + ": tp_mode must be 0 (tp) or 1 (tau)");
    if (tp_mode == 1 && !std::isfinite(t_ref)) return fail(h, OCTO_EINVAL, std::string(who) + ": t_ref must be finite with tp_mode 1");
    (void)octo_draws_ofti_clear(h);
    octo_ofti* o = nullptr;
    if (int rc = octo_ofti_create(h->ctx, epochs, ra, dec, sigma_ra, sigma_dec, cor, n_epochs, sigma_abfg, &o)) {
        const char* m = octo_last_error(h->ctx);
        return fail(h, rc, m ? m : "octo_ofti_create failed");
    }
    auto bail = [&](int rc) { (void)octo_ofti_destroy(o); return rc; };
    octo_consts c;
    if (consts) c = *consts;
    else if (octo_consts_default(&c) != OCTO_OK) return bail(fail(h, OCTO_EINVAL, std::string(who) + ": octo_consts_default failed"));
    // the rows and the scalars beside them, as octo_ofti_create forms them (octo_api.hip; parameterizations.jl:359-366, 387-400)
    std::vector<double> rows((size_t)n_epochs * ROW_STRIDE, 0.0);
    double data_quad = 0.0, log_det_data_cov = 0.0;
    for (int64_t j = 0; j < n_epochs; ++j) {
        const double sr = sigma_ra[j], sd = sigma_dec[j], rho = cor ? cor[j] : 0.0;
        const double det = sr * sr * sd * sd * (1.0 - rho * rho);
        const double wrr = sd * sd / det, wdd = sr * sr / det, wrd = -rho * sr * sd / det;
        double* r = &rows[(size_t)j * ROW_STRIDE];
        r[0] = epochs[j]; r[1] = wrr; r[2] = wdd; r[3] = wrd;
        r[4] = wrr * ra[j] + wrd * dec[j]; r[5] = wdd * dec[j] + wrd * ra[j];
        data_quad += ra[j] * r[4] + dec[j] * r[5];
        log_det_data_cov += std::log(det);
    }
    if (hipSetDevice(h->device) != hipSuccess) return bail(fail(h, OCTO_EHIP, std::string(who) + ": hipSetDevice failed"));
    OftiRows parts;
    if (int rc = grow_to(h, h->d_oftis_rows, h->cap_oftis_rows, parts, ofti_rows, std::max<int64_t>(n_epochs, 1))) return bail(rc);
    if (n_epochs > 0 && hipMemcpy(parts.rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice) != hipSuccess)
        return bail(fail(h, OCTO_EHIP, std::string(who) + ": upload failed"));
    h->ofti = o;
    h->oftis_n_rows = (int32_t)n_epochs; h->oftis_tp_mode = tp_mode; h->oftis_t_ref = t_ref; h->oftis_k_yr = c.kepler_year_to_julian_day;
    h->oftis_lambda = 1.0 / (sigma_abfg * sigma_abfg); h->oftis_data_quad = data_quad; h->oftis_log_det_data_cov = log_det_data_cov;
    h->oftis_log_det_prior_inv = 4.0 * std::log(h->oftis_lambda); h->oftis_n_log2pi = (double)n_epochs * std::log(TWO_PI);
    return OCTO_OK;
}

int32_t octo_draws_ofti_nl_device(octo_draws* h, int64_t n, int64_t ld, const double* d_theta, double* d_nl, void* hip_stream) {
    const char* who = "octo_draws_ofti_nl_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_set(h, who)) return rc;
    if (int rc = check_batch(h, who, n, ld, d_theta && d_nl)) return rc;
    if (n == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    launch_nl(h, stream_of(h, hip_stream), n, ld, d_theta, d_nl);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_ofti_posterior_device(octo_draws* h, uint64_t seed, int64_t n, int64_t ld, const uint64_t* d_index, const double* d_nl, double* d_out,
                                         void* hip_stream) {
    const char* who = "octo_draws_ofti_posterior_device";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_set(h, who)) return rc;
    if (int rc = check_batch(h, who, n, ld, d_index && d_nl && d_out)) return rc;
    if (n == 0) return OCTO_OK;
    OCHK(h, hipSetDevice(h->device));
    launch_post(h, stream_of(h, hip_stream), seed, n, ld, d_index, d_nl, d_out);
    OCHK(h, hipGetLastError());
    return OCTO_OK;
}

int32_t octo_draws_ofti_rejection(octo_draws* h, uint64_t seed, uint64_t first, int64_t N, int64_t cap, double* theta_out, double* nl_out, double* post_out,
                                  uint64_t* index_out, int64_t* n_accepted, double* max_logml) {
    const char* who = "octo_draws_ofti_rejection";
    if (!h) return OCTO_EINVAL;
    if (int rc = check_set(h, who)) return rc;
    if (N < 1) return fail(h, OCTO_EINVAL, std::string(who) + ": N >= 1");
    if (first + (uint64_t)N < first) return fail(h, OCTO_EINVAL, std::string(who) + ": first + N overflows the draw index");
    if (cap < 0 || !n_accepted) return fail(h, OCTO_EINVAL, std::string(who) + ": cap >= 0 and n_accepted are required");
    if (cap > 0 && (!theta_out || !nl_out || !post_out || !index_out)) return fail(h, OCTO_EINVAL, std::string(who) + ": null output with cap > 0");
    OCHK(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    const int64_t nblk = (N + TPB - 1) / TPB, room = std::min(cap, N);
    OftiWork k;
    if (int rc = grow_to(h, h->d_oftis, h->cap_oftis, k, ofti_work, CHUNK, N, nblk, std::max<int64_t>(room, 1))) return rc;
    // pass 1: ℓ of every draw, chunk by chunk (chunk boundaries are block boundaries), and the block maxima
    for (int64_t done = 0; done < N; done += CHUNK) {
        const int64_t n = std::min(CHUNK, N - done);
        if (int rc = draws_launch_draw(h, st, seed, first + (uint64_t)done, nullptr, n, CHUNK, k.theta)) return rc;
        launch_nl(h, st, n, CHUNK, k.theta, k.nl);
        OCHK(h, hipGetLastError());
        if (int rc = main_call(h, octo_ofti_eval_device(h->ctx, h->ofti, k.nl, CHUNK, n, nullptr, k.ll + done, (void*)st), "octo_ofti_eval_device")) return rc;
        hipLaunchKernelGGL(k_oftis_ll, grid_of(n), dim3(TPB), 0, st, k.ll + done, n, k.pmax + done / TPB);
        OCHK(h, hipGetLastError());
    }
    // pass 2: octo_draws_rejection's — ℓ stands for both of its columns
    double mx = 0.0;
    int64_t total = 0;
    *n_accepted = 0;
    const int rc2 = draws_max_pass(h, st, k.pmax, N, k.max, &mx);
    if (max_logml) *max_logml = mx;
    if (rc2) return rc2;
    if (int rc = draws_accept_pass(h, st, k.ll, k.ll, N, k.max, seed, first, k.cnt, room, k.ix, k.oll, k.olp, &total)) return rc;
    *n_accepted = total;
    const int64_t ns = std::min(total, room);
    if (ns == 0) return OCTO_OK;
    // the survivors: θ from the counter, nl, the posterior draw
    if (int rc = draws_launch_draw(h, st, seed, 0, k.ix, ns, ns, k.otheta)) return rc;
    launch_nl(h, st, ns, ns, k.otheta, k.onl);
    launch_post(h, st, seed, ns, ns, k.ix, k.onl, k.post);
    OCHK(h, hipGetLastError());
    OCHK(h, hipMemcpyAsync(index_out, k.ix, sizeof(uint64_t) * ns, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpy2DAsync(theta_out, sizeof(double) * cap, k.otheta, sizeof(double) * ns, sizeof(double) * ns, 5, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpy2DAsync(nl_out, sizeof(double) * cap, k.onl, sizeof(double) * ns, sizeof(double) * ns, 5, hipMemcpyDeviceToHost, st));
    OCHK(h, hipMemcpy2DAsync(post_out, sizeof(double) * cap, k.post, sizeof(double) * ns, sizeof(double) * ns, OCTO_DRAWS_OFTI_N_OUT, hipMemcpyDeviceToHost, st));
    OCHK(h, hipStreamSynchronize(st));
    return OCTO_OK;
}

}  // extern "C"
