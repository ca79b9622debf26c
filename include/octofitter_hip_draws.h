/*
 * octofitter_hip_draws.h — companion C ABI: IID prior draws made ON the device, and the two reference drivers that
 * consume a whole batch of them.
 *
 *   octo_draws_best       <- guess_starting_position, src/initialization.jl:14-66: score N prior draws, keep the best.
 *   octo_draws_rejection  <- octofit_rejection, src/sampling.jl:168-268: accept draw i with probability exp(ll_i − max ll).
 *
 * A companion of include/octofitter_hip.h, in a shared object of its own (liboctofitter_hip_draws.so, which links
 * liboctofitter_hip.so): it is a CLIENT of the public ABI — every log-posterior comes from octo_model_logpost_device — and
 * adds nothing to the main header or library. Same conventions: `extern "C"`, int32 status codes of the main header
 * (OCTO_OK …), SoA arrays with the draw index fastest, no C++ exception across the boundary.
 *
 * The generator is counter based and stateless (Philox4x64-10): draw i of a seed is a pure function of (seed, i, d), so it
 * is the same number whatever call, batch, chunk or grid produces it. Nothing of a draw is ever stored for all N: what a
 * driver returns is regenerated from the counter.
 *   key     = (seed, 0x6f63746f64726177)
 *   counter = (i, j, purpose, 0)   i: draw index · j = d / 4: block of four coordinates, coordinate d takes word d % 4
 *   purpose 0: the prior draws · purpose 1, block 0, word 0: the rejection uniform of draw i
 *   uniform = (2·(x >> 12) + 1)·2⁻⁵³ of a 64-bit word x: exact in a double and strictly inside (0, 1)
 * Each coordinate is the prior's inverse CDF of its uniform (a result that rounds onto a bound of the support is moved one
 * ulp inside), then Bijectors' link of it; the densities and Jacobians are the device routines of the model callback.
 *
 * Not thread-safe: a handle uses its context (scratch, stream ordering), so the rule of the main header holds — one host
 * thread at a time per context, the handle's calls included.
 */
#ifndef OCTOFITTER_HIP_DRAWS_H
#define OCTOFITTER_HIP_DRAWS_H

#include "octofitter_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OCTO_DRAWS_MAX_KEEP 64
#define OCTO_DRAWS_PURPOSE_PRIOR   0
#define OCTO_DRAWS_PURPOSE_UNIFORM 1

typedef struct octo_draws octo_draws;

/* priors / D: the array given to octo_model_create (copied). `model` may be NULL: a handle that only samples.
 * `device_id`: the device of `ctx` (octo_ctx_create's argument). The handle owns a stream and its buffers; it keeps
 * `ctx` and `model`, which must outlive it. OCTO_EINVAL: NULL ctx, priors or out; D outside 1…64; an unknown prior kind. */
int32_t octo_draws_create(octo_ctx* ctx, octo_model* model, const octo_prior* priors,
                          int32_t D, int32_t device_id, octo_draws** out);
/* Destroying a handle whose stream the context has seen makes one small host-buffer call on the context (it moves the context back to its own
 * stream: the context orders a change of stream through the stream of its previous call, which must still exist). So destroy the handle BEFORE
 * its model and context — or, if they are already gone, call octo_draws_detach first: the handle then forgets them (sampling still works). */
int32_t octo_draws_destroy(octo_draws* h);
int32_t octo_draws_detach(octo_draws* h);

/* Text of the last failure of a call on `h`; with h = NULL, of the last octo_draws_create on this thread. */
const char* octo_draws_last_error(const octo_draws* h);

/* Draws first … first+n-1 of stream `seed` into DEVICE buffers, asynchronous on hip_stream (a hipStream_t as in the main
 * header; OCTO_STREAM_CTX selects the HANDLE's own stream, which octo_draws_sync waits for). Every output may be NULL.
 *   d_theta      [D][ld]  natural domain
 *   d_theta_t    [D][ld]  linked (unconstrained)
 *   d_logprior_t [n]      Σ_d logpdf_with_trans, the prior term of the model callback at this θ_t
 * OCTO_EINVAL: n < 0, ld < n, first + n overflowing. */
int32_t octo_draws_sample_device(octo_draws* h, uint64_t seed, uint64_t first, int64_t n, int64_t ld,
                                 double* d_theta, double* d_theta_t, double* d_logprior_t, void* hip_stream);
int32_t octo_draws_sync(octo_draws* h);

/* guess_starting_position: the `keep` (1…OCTO_DRAWS_MAX_KEEP, <= N) highest log-posteriors among draws first…first+N-1, best
 * first, ties to the lower draw index. Non-finite log-posteriors never win: if fewer than `keep` draws are finite the
 * remaining places hold logpost = -Inf and the lowest draw indices not already listed (with none finite: the first `keep`
 * draws — the reference returns a prior draw and -Inf). HOST outputs, blocking. */
int32_t octo_draws_best(octo_draws* h, uint64_t seed, uint64_t first, int64_t N, int32_t keep,
                        double* theta_out /*[D][keep]*/, double* logpost_out /*[keep]*/, uint64_t* index_out /*[keep]*/);

/* octofit_rejection: ll_i = logpost_i − logprior_t_i (the likelihood and the UnitLengthPrior terms; non-finite -> -Inf),
 * draw i accepted iff ll_i != -Inf and u_i < exp(ll_i − max ll). Accepted draws in draw-index order, HOST outputs, blocking.
 * At most `cap` are stored (cap = 0: count only; the arrays may then be NULL); *n_accepted is the full count.
 * OCTO_EINVAL with the reference's message when every ll is -Inf. */
int32_t octo_draws_rejection(octo_draws* h, uint64_t seed, uint64_t first, int64_t N, int64_t cap,
                             double* theta_out /*[D][cap]*/, double* loglike_out /*[cap]*/, double* logpost_out /*[cap]*/,
                             uint64_t* index_out /*[cap]*/, int64_t* n_accepted, double* max_loglike);

#ifdef __cplusplus
}
#endif
#endif /* OCTOFITTER_HIP_DRAWS_H */
