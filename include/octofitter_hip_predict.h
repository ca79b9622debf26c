/*
 * octofitter_hip_predict.h — companion C ABI: the MODEL VALUES of a batch of parameter sets on the device — the sky offset
 * and the radial velocity of each companion at each epoch of a grid — as a cube, or reduced over the draws to a band.
 *
 * In the reference these are `simulate!` (relative-astrometry.jl:104-142, rv-absolute.jl:135-158,
 * rv-absolute-margin.jl:106-126, rv-relative.jl:121-164): what residuals, posterior-predictive checks,
 * generate_from_params (relative-astrometry.jl:256-319) and every orbit / RV curve of a results plot are made from.
 *
 * A companion of include/octofitter_hip.h in a shared object of its own (liboctofitter_hip_predict.so): it adds nothing to
 * the main header or library, and needs no octo_ctx. Same conventions: `extern "C"`, the int32 status codes of the main
 * header, SoA arrays with the walker index fastest, no C++ exception across the boundary. The orbit constants come from the
 * device routines of the likelihood kernels (setup_planet_vals, the cold kepler_solve), included, not restated.
 *
 * A value is a function of (θ of the walker, epoch, channel) alone — no warm start, no dependence on the other walkers of a
 * wave, on the row partition or on the neighbouring epochs: it is BIT-IDENTICAL whatever batch size, walker index, grid
 * position, grid order or entry point (cube, host-buffer cube, summary) evaluates it.
 *
 * Not thread-safe: one host thread at a time per handle; calls on one handle that use different streams must be ordered by
 * the caller (the summary's partial buffer and the host-buffer calls' device buffers belong to the handle).
 */
#ifndef OCTOFITTER_HIP_PREDICT_H
#define OCTOFITTER_HIP_PREDICT_H

#include "octofitter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OCTO_PREDICT_MAX_CHANNELS 32

/* ---- quantities; a channel is (quantity, planet) -------------------------------------------------------------------- */
#define OCTO_PREDICT_RAOFF      0   /* raoff(sol) of the planet                                   [mas]            */
#define OCTO_PREDICT_DECOFF     1   /* decoff(sol)                                                [mas]            */
#define OCTO_PREDICT_SEP        2   /* hypot(raoff, decoff)                                       [mas]            */
#define OCTO_PREDICT_PA         3   /* atan(raoff, decoff), east of north                         [rad], (−π, π]   */
#define OCTO_PREDICT_RADVEL     4   /* radvel(sol) of the planet                                  [m/s]            */
#define OCTO_PREDICT_ASTROM_RA  5   /* model of a relative-astrometry table of the planet: its offset minus the reflex       */
#define OCTO_PREDICT_ASTROM_DEC 6   /*   offsets −m_k/M_k·raoff_k of every strictly inner planet with a mass  [mas]           */
#define OCTO_PREDICT_ASTROM_SEP 7   /* the same model as ρ                                        [mas]            */
#define OCTO_PREDICT_ASTROM_PA  8   /*   … and as position angle                                  [rad], (−π, π]   */
#define OCTO_PREDICT_RV_STAR    9   /* Σ_p −m_p/M_p·radvel_p over ALL planets (rv-absolute.jl:146-155); planet = −1  [m/s] */
#define OCTO_PREDICT_RV_REL    10   /* radvel_p + the reflex terms of strictly inner planets with a mass (rv-relative.jl:143-156) [m/s] */
#define OCTO_PREDICT_N_QUANTITIES 11

typedef struct octo_predict_channel {
    int32_t quantity;      /* OCTO_PREDICT_*                                  */
    int32_t planet;        /* 0-based; −1 (required) for OCTO_PREDICT_RV_STAR */
} octo_predict_channel;

typedef struct octo_predict octo_predict;

/* consts: NULL = octo_consts_default. planets / n_planets: 1 … OCTO_MAX_PLANETS, as given to octo_dataset_create.
 * epochs[T]: MJD, finite, any order, repeats allowed (copied). basis[T] or NULL: the column an RV channel's add1 multiplies
 * (the trend basis of OCTO_NU_RV_TREND, e.g. epoch − 57000). channels / n_channels: 1 … OCTO_PREDICT_MAX_CHANNELS.
 * The platescale and northangle nuisances act on the DATA in the reference: they are no part of a model value.
 * OCTO_EINVAL (before any device is touched): NULL planets / epochs / channels / out, T < 1, a count outside its range, a
 * non-finite epoch or basis value, an unknown orbit kind or quantity, a planet index outside the system, and the boundary
 * of the main header — an astrometric quantity (RAOFF … PA) for an OCTO_ORBIT_RADVEL / OCTO_ORBIT_KEP planet (no parallax),
 * an ASTROM_* quantity in a system that holds such a planet, RADVEL for an OCTO_ORBIT_THIELE_INNES planet, RV_STAR / RV_REL
 * in a system that holds one. The handle owns a stream and its buffers. */
int32_t octo_predict_create(int32_t device_id, const octo_consts* consts,
                            const octo_planet_desc* planets, int32_t n_planets,
                            const double* epochs, int64_t T, const double* basis,
                            const octo_predict_channel* channels, int32_t n_channels,
                            octo_predict** out);
int32_t octo_predict_destroy(octo_predict* h);
/* Text of the last failure of a call on `h`; with h = NULL, of the last octo_predict_create on this thread. */
const char* octo_predict_last_error(const octo_predict* h);
/* Waits for the handle's own stream (OCTO_STREAM_CTX below). */
int32_t octo_predict_sync(octo_predict* h);

/* The cube, DEVICE buffers, asynchronous on hip_stream (a hipStream_t as in the main header; OCTO_STREAM_CTX selects the
 * HANDLE's own stream, which octo_predict_sync waits for).
 *   d_elems [n_planets*OCTO_N_EL][ld]   the main ABI's element rows
 *   d_add0, d_add1 [n_channels][ld] or NULL   affine nuisance term of the RV channels (RADVEL, RV_STAR, RV_REL):
 *           value + add0[c][w] + add1[c][w]·basis[j] — the offset and the OCTO_NU_RV_TREND coefficient, which make the channel
 *           rv_model of the tables' simulate!. Rows of other channels are not read; add1 is ignored without a basis column.
 *   d_out   [n_channels*T][ld_out]   d_out[(c·T + j)·ld_out + w]
 * A walker the likelihood would score −Inf (a non-finite element, e ∉ [0, 1), a <= 0, M <= 0, plx <= 0: setup_valid of ANY of
 * its planets) gives NaN in all its outputs — the convention of octo_kepler_solve, never an error status.
 * OCTO_EINVAL: W < 0, ld < W, ld_out < W, NULL d_elems or d_out with W > 0. */
int32_t octo_predict_eval_device(octo_predict* h, const double* d_elems, int64_t ld, int64_t W,
                                 const double* d_add0, const double* d_add1,
                                 double* d_out, int64_t ld_out, void* hip_stream);
/* The same on HOST buffers, blocking. The cube goes back in chunks of walkers through a pinned staging buffer of bounded
 * size, so a cube larger than the handle's device buffer is not an error. */
int32_t octo_predict_eval(octo_predict* h, const double* elems, int64_t ld, int64_t W,
                          const double* add0, const double* add1, double* out, int64_t ld_out);

/* The band: for every (channel, epoch) the statistics over the VALID walkers, the cube never stored.
 *   out [5][n_channels][T]: n_valid · mean · standard deviation (n − 1) · minimum · maximum
 * n_valid = 1: the standard deviation is NaN (0/0, as a sample variance of one value); n_valid = 0: all four are NaN.
 * The order of combination is fixed — per block of 256 walkers an exact (count, mean, M2, min, max), then a Chan merge of the
 * blocks in index order in a second kernel; no floating-point atomics — so results are bit-identical from run to run. The
 * values reduced are those of the cube, from the same inlined routine. OCTO_EINVAL: W < 1, ld < W, NULL d_elems or d_out. */
int32_t octo_predict_summary_device(octo_predict* h, const double* d_elems, int64_t ld, int64_t W,
                                    const double* d_add0, const double* d_add1, double* d_out, void* hip_stream);
int32_t octo_predict_summary(octo_predict* h, const double* elems, int64_t ld, int64_t W,
                             const double* add0, const double* add1, double* out);

/* Measurement hook (tools/predict_bench.py): the cube kernel's store-width variant. 1: one walker per lane, 8-byte stores;
 * 2: two adjacent walkers per lane, one 16-byte store per lane, wherever that variant is compiled (one and two planets) and
 * the output allows it (ld_out even, d_out 16-byte aligned), else 1; 0 (default): 2 for one planet, 1 otherwise.
 * The values do not depend on it, bit for bit. OCTO_EINVAL outside 0 … 2. */
int32_t octo_predict_set_variant(octo_predict* h, int32_t variant);

#ifdef __cplusplus
}
#endif
#endif /* OCTOFITTER_HIP_PREDICT_H */
