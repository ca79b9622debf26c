/*
 * octofitter_hip_psis.h — companion C ABI: Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO; Vehtari, Gelman & Gabry
 * 2017; Vehtari et al. 2024) of a pointwise log-likelihood matrix on the device: per datum the fitted Pareto shape k̂ (the
 * diagnostic: k̂ > 0.7 = do not trust this row), the smoothed elpd_loo, the lppd, the effective sample size and, optionally, the
 * smoothed normalised log-weights.
 *
 * The input is the matrix of include/octofitter_hip_pointwise.h exactly as octo_pointwise_eval_device writes it: ll[r·ld + s],
 * row = datum, sample index fastest. Only 6·R numbers have to leave the device, not R·S·8 bytes.
 *
 * A companion of include/octofitter_hip.h in a shared object of its own (liboctofitter_hip_psis.so): it adds nothing to the
 * main header or library, links nothing of it, and needs no octo_ctx. Same conventions: `extern "C"`, the int32 status codes of
 * the main header, no C++ exception across the boundary.
 *
 * THE ALGORITHM, per row, over the entries with a FINITE ll (n of them); it follows ArviZ's _psislw / _gpdfit with the edge
 * cases made explicit:
 *   1. x_s = −ll_s − max(−ll); M = ceil(min(n/5, 3·√n)) (octo_psis_tail_len). n = 0: every statistic NaN, N = 0, weights −Inf.
 *      n <= M: no smoothing, k̂ = +Inf, tail_len = 0.
 *   2. cut-off x_c = max(the (M+1)-th largest x, log(DBL_MIN)); the tail is {s : x_s > x_c}, STRICT — ties at the cut-off stay
 *      out, so tail_len can be below M. tail_len <= 4: k̂ = +Inf, no smoothing.
 *   3. the tail sorted ascending by (x, sample index); y_i = exp(x_i) − exp(x_c).
 *   4. Zhang–Stephens fit with the PSIS prior, tl = tail_len, m = 30 + ⌊√tl⌋, j = 1 … m (1-based indices):
 *        b_j = (1 − √(m/(j − ½)))/(3·y_[⌊tl/4 + ½⌋]) + 1/y_[tl],  k_j = mean_i log1p(−b_j y_i),  L_j = tl·(log(−b_j/k_j) − k_j − 1),
 *        w_j = 1/Σ_l exp(L_l − L_j), w_j < 10·2⁻⁵² dropped, renormalised; b = Σ w_j b_j, k = mean_i log1p(−b y_i), σ = −k/b,
 *        k̂ = (tl·k + 5)/(tl + 10).
 *   5. k̂ finite: p_i = (i − ½)/tl, q_i = σ·expm1(−k̂·log1p(−p_i))/k̂ (−σ·log1p(−p_i) at k̂ = 0); the i-th sorted tail entry
 *      gets x = min(log(q_i + exp(x_c)), 0).
 *   6. lw = x − logsumexp(x); elpd_loo = logsumexp(ll + lw); lppd = logsumexp(ll) − log n; ess = 1/Σ exp(2·lw).
 *
 * Every sum is taken in a fixed order (a lane's strided partial, wave butterflies, the block's waves in wave order): no
 * floating-point atomics, results bit-identical from run to run, independent of R, of the row's position in the matrix, of the
 * leading dimensions and of the entry point.
 *
 * Not thread-safe: one host thread at a time per handle (the host-buffer call's device buffers belong to the handle).
 */
#ifndef OCTOFITTER_HIP_PSIS_H
#define OCTOFITTER_HIP_PSIS_H

#include "octofitter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of the result: out[k][r] */
#define OCTO_PSIS_N        0   /* entries with a finite ll                                                      */
#define OCTO_PSIS_TAIL_LEN 1   /* entries strictly above the cut-off (0: n <= M)                                */
#define OCTO_PSIS_PARETO_K 2   /* k̂ (+Inf: no fit was made)                                                     */
#define OCTO_PSIS_ELPD_LOO 3   /* logsumexp(ll + lw)                                                            */
#define OCTO_PSIS_LPPD     4   /* log mean exp(ll)                                                              */
#define OCTO_PSIS_ESS      5   /* 1/Σ exp(2·lw)                                                                 */
#define OCTO_PSIS_N_STATS  6

typedef struct octo_psis octo_psis;

/* OCTO_EINVAL: NULL out, device_id out of range. OCTO_ENODEV: no device. The handle owns a stream and its buffers.
 * Environment, read here: OCTO_PSIS_MATRIX_BYTES (device buffer of a chunk of rows of the host-buffer call, default 64 MiB),
 * OCTO_PSIS_STAGE_BYTES (its pinned staging buffer, default 16 MiB). */
int32_t octo_psis_create(int32_t device_id, octo_psis** out);
int32_t octo_psis_destroy(octo_psis* h);
/* Text of the last failure of a call on `h`; with h = NULL, of the last octo_psis_create on this thread. */
const char* octo_psis_last_error(const octo_psis* h);
/* Waits for the handle's own stream (OCTO_STREAM_CTX below). */
int32_t octo_psis_sync(octo_psis* h);

/* M(n) = ceil(min(n/5, 3·√n)) in double arithmetic; 0 for n <= 0. Host only, no handle. */
int64_t octo_psis_tail_len(int64_t n);
/* The largest S served: the largest S with M(S) <= 4096, the tail the kernel's sort buffer holds. */
int64_t octo_psis_max_samples(void);

/* DEVICE buffers, asynchronous on hip_stream (a hipStream_t as in the main header; OCTO_STREAM_CTX selects the HANDLE's own
 * stream, which octo_psis_sync waits for).
 *   d_ll  [R][ld]   the pointwise matrix; no value is read past S in a row
 *   d_out [OCTO_PSIS_N_STATS][R]
 *   d_lw  [R][ld_w] or NULL   the smoothed, normalised log-weights; −Inf for an entry whose ll is not finite
 * OCTO_EINVAL: NULL handle or d_ll / d_out (with R > 0), R < 0, S < 1, ld < S, ld_w < S with d_lw given.
 * OCTO_ENOTSUP: S > octo_psis_max_samples(). */
int32_t octo_psis_loo_device(octo_psis* h, const double* d_ll, int64_t ld, int64_t R, int64_t S,
                             double* d_out, double* d_lw, int64_t ld_w, void* hip_stream);
/* The same on HOST buffers, blocking. The matrix goes to the device in chunks of ROWS (a row needs all its samples) through
 * the pinned staging buffer, so a matrix larger than the handle's device buffer is not an error; a single ROW larger than it
 * is OCTO_ENOMEM with a message. */
int32_t octo_psis_loo(octo_psis* h, const double* ll, int64_t ld, int64_t R, int64_t S,
                      double* out, double* lw, int64_t ld_w);

#ifdef __cplusplus
}
#endif
#endif /* OCTOFITTER_HIP_PSIS_H */
