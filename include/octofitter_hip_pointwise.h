/*
 * octofitter_hip_pointwise.h — companion C ABI: the POINTWISE log-likelihood of a batch of parameter sets on the device —
 * ll[datum][posterior sample], one row per table row — as a matrix, or reduced over the samples to the per-datum sums that
 * WAIC and importance-sampling LOO are made from.
 *
 * In the reference this is `pointwise_like` (src/cross-validation.jl:17-46: one system per epoch, threaded over the samples):
 * the matrix that WAIC, IS-LOO and PSIS-LOO consume. PSIS smoothing of it on the device: include/octofitter_hip_psis.h.
 *
 * A companion of include/octofitter_hip.h in a shared object of its own (liboctofitter_hip_pointwise.so): it adds nothing to
 * the main header or library, and needs no octo_ctx. Same conventions: `extern "C"`, the int32 status codes of the main
 * header, SoA arrays with the walker index fastest, no C++ exception across the boundary. The orbit constants and the Kepler
 * solve come from the device routines of the likelihood kernels (setup_planet_vals, the cold kepler_solve), included, not
 * restated; the per-row density is written in this library, by the rules of the likelihood's row bodies.
 *
 * A value is a function of (θ of the walker, its table's nuisances, the row) alone — no warm start, no dependence on the
 * neighbouring rows, on the other walkers of a wave or on the launch shape: it is BIT-IDENTICAL whatever batch size, walker
 * index or entry point (matrix, host-buffer matrix) evaluates it, and the summary reduces exactly those values.
 *
 * Not thread-safe: one host thread at a time per handle; calls on one handle that use different streams must be ordered by
 * the caller (the summary's partial buffer and the host-buffer calls' device buffers belong to the handle).
 */
#ifndef OCTOFITTER_HIP_POINTWISE_H
#define OCTOFITTER_HIP_POINTWISE_H

#include "octofitter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OCTO_POINTWISE_MAX_TABLES 1024

/* rows of the summary: out[k][r] */
#define OCTO_POINTWISE_N           0   /* walkers with a finite value                                         */
#define OCTO_POINTWISE_LPPD        1   /* log mean exp(ll): the log pointwise predictive density              */
#define OCTO_POINTWISE_MEAN        2   /* mean of ll                                                          */
#define OCTO_POINTWISE_VAR         3   /* sample variance of ll (n − 1): the WAIC penalty p_waic              */
#define OCTO_POINTWISE_ELPD_IS_LOO 4   /* −log mean exp(−ll): importance-sampling leave-one-out               */
#define OCTO_POINTWISE_MIN         5
#define OCTO_POINTWISE_MAX         6
#define OCTO_POINTWISE_N_STATS     7

typedef struct octo_pointwise octo_pointwise;

/* consts: NULL = octo_consts_default. obs / n_obs, planets / n_planets: as given to octo_dataset_create (the columns are
 * copied; the caller keeps ownership), 0 … OCTO_POINTWISE_MAX_TABLES tables, 1 … OCTO_MAX_PLANETS planets.
 * Kinds served: OCTO_ASTROM_RADEC, OCTO_ASTROM_SEPPA (with or without cor), OCTO_RV_ABS and OCTO_RV_REL (with or without the
 * trend basis column in `extra`), on every orbit kind the main library accepts for those tables.
 * OCTO_ENOTSUP (before any device is touched, the message names the table): OCTO_RV_ABS_MARG, OCTO_HGCA, OCTO_ONEIL_RADEC,
 * OCTO_ONEIL_SEPPA — the value of such a table is not a sum over its rows — and an RV table next to a ThieleInnesOrbit planet.
 * OCTO_EINVAL (likewise before any device is touched): the input rules of octo_dataset_create — an uncertainty that is not finite
 * and > 0, a non-finite epoch, measurement or basis value, a correlation outside the reference's bound, a planet index outside
 * the system, astrometry on a planet without parallax, absolute RV in a system with a planet without a mass, a missing column,
 * `extra` of the wrong length — NULL obs (with n_obs > 0) / planets / out, counts out of range, an unknown kind or orbit kind,
 * more than 2^31 − 1 rows in all. The handle owns a stream and its buffers. */
int32_t octo_pointwise_create(int32_t device_id, const octo_consts* consts,
                              const octo_obs_desc* obs, int32_t n_obs,
                              const octo_planet_desc* planets, int32_t n_planets,
                              octo_pointwise** out);
int32_t octo_pointwise_destroy(octo_pointwise* h);
/* Text of the last failure of a call on `h`; with h = NULL, of the last octo_pointwise_create on this thread. */
const char* octo_pointwise_last_error(const octo_pointwise* h);
/* Waits for the handle's own stream (OCTO_STREAM_CTX below). */
int32_t octo_pointwise_sync(octo_pointwise* h);

/* R = Σ n_epochs over the tables: the rows of the matrix, in table order, then row order. −1 for a NULL handle. */
int64_t octo_pointwise_n_rows(const octo_pointwise* h);
/* out[R]: the table index of each row. */
int32_t octo_pointwise_row_table(const octo_pointwise* h, int32_t* out);

/* The matrix, DEVICE buffers, asynchronous on hip_stream (a hipStream_t as in the main header; OCTO_STREAM_CTX selects the
 * HANDLE's own stream, which octo_pointwise_sync waits for).
 *   d_elems [n_planets*OCTO_N_EL][ld]   the main ABI's element rows
 *   d_nuis  [n_obs*OCTO_N_NUIS][ld] or NULL   the main ABI's nuisance rows; NULL = the defaults (jitter 0, platescale 1,
 *           northangle 0, offset 0, trend 0). The trend coefficient of a table without a basis column is not read.
 *   d_out   [R][ld_out]   d_out[r·ld_out + w] = the log-density of row r ALONE under walker w, constant terms included:
 *           what a one-row dataset of that table scores.
 * A walker the likelihood scores −Inf (setup_valid of ANY of its planets fails: a non-finite element, e ∉ [0, 1), a <= 0,
 * M <= 0, plx <= 0) gives −Inf in all its rows. A NaN nuisance gives NaN in the rows of its table. Neither is ever a status.
 * OCTO_EINVAL: W < 0, ld < W, ld_out < W, NULL d_elems or d_out with W > 0 and R > 0. */
int32_t octo_pointwise_eval_device(octo_pointwise* h, const double* d_elems, int64_t ld, int64_t W,
                                   const double* d_nuis, double* d_out, int64_t ld_out, void* hip_stream);
/* The same on HOST buffers, blocking. The matrix goes back in chunks of walkers through a pinned staging buffer of bounded
 * size, so a matrix larger than the handle's device buffer is not an error. Environment at octo_pointwise_create:
 * OCTO_POINTWISE_MATRIX_BYTES (device buffer of a chunk, default 64 MiB), OCTO_POINTWISE_STAGE_BYTES (pinned buffer, 16 MiB). */
int32_t octo_pointwise_eval(octo_pointwise* h, const double* elems, int64_t ld, int64_t W,
                            const double* nuis, double* out, int64_t ld_out);

/* The reduction over the walkers with a FINITE value, the matrix never stored.
 *   out [OCTO_POINTWISE_N_STATS][R]: n · lppd · mean · sample variance (n − 1) · elpd_is_loo · minimum · maximum
 * n = 1: the variance is NaN (0/0). n = 0: rows 1 … 6 are NaN.
 * The order of combination is fixed — per block of walkers (n, max, Σ exp(ll − max), min, Σ exp(min − ll), mean, M2) by wave
 * butterflies and then the block's waves in wave order, one partial per block; a second kernel merges the partials in block
 * order (log-sum-exp pairs rescaled to the common extreme, Chan's merge for mean / M2); no floating-point atomics — so results
 * are bit-identical from run to run. The values reduced are those of the matrix, from the same inlined routine.
 * OCTO_EINVAL: W < 1, ld < W, NULL d_elems or d_out. */
int32_t octo_pointwise_summary_device(octo_pointwise* h, const double* d_elems, int64_t ld, int64_t W,
                                      const double* d_nuis, double* d_out, void* hip_stream);
int32_t octo_pointwise_summary(octo_pointwise* h, const double* elems, int64_t ld, int64_t W,
                               const double* nuis, double* out);

#ifdef __cplusplus
}
#endif
#endif /* OCTOFITTER_HIP_POINTWISE_H */
