/*
 * octofitter_hip_draws.h — companion C ABI: IID prior draws made ON the device, and the two reference drivers that
 * consume a whole batch of them, and a tempered HMC explorer for batches of chains (below).
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
 * The third driver is an explorer: one tempered HMC step of every chain of a batch (octo_draws_hmc_step_device), the piece between the
 * batched log-posterior with its gradient and the swap step of parallel tempering (octo_pt_step_device). Its two streams add
 *   purpose 2: the momentum of chain c at `step`, counter (c, d / 4, 2, step), coordinate d takes word d % 4
 *   purpose 3: the acceptance uniform of chain c at `step`, counter (c, 0, 3, step), word 0
 * Purposes 0 and 1 keep counter word 3 = 0. The step is stated in full at its declaration, so that a restatement elsewhere (tests/hmc_reference.py)
 * and the device compute the same function.
 *
 * The fourth is an optimiser: a batched L-BFGS that takes W chains from starting points (octo_draws_best's, say) to local optima of ℓπ
 * (octo_draws_lbfgs_device), also stated in full at its declaration (tests/lbfgs_reference.py restates it). It draws no random number.
 *
 * The fifth is Pathfinder on those paths (octo_draws_pathfinder_device): a normal approximation at every accepted iterate, an ELBO estimate
 * of each from a few draws, the best one kept, and draws from it (tests/pathfinder_reference.py restates it). Its two streams add
 *   purpose 4: ELBO draw k of chain c at its iterate number it, counter (c, d / 4, 4, it·32 + k), coordinate d takes word d % 4
 *   purpose 5: final draw j of chain c, counter (c, d / 4, 5, j)
 *
 * The sixth is the explorer's warm-up: grouped cross-chain moments, the diagonal metric they give, dual averaging of the step size and
 * per-chain running moments (octo_draws_moments_device … octo_draws_chain_moments_device; tests/adapt_reference.py restates them). No random number.
 *
 * The seventh is the no-U-turn sampler (octo_draws_nuts_device): one NUTS transition of every chain of a batch, the trees built in lockstep,
 * stated in full at its declaration (tests/nuts_reference.py restates it). Its momenta are purpose 2's, the HMC step's; its three streams add
 *   purpose 6: the direction of doubling j of chain c at `step`, counter (c, j, 6, step), word 0
 *   purpose 7: the proposal uniform of the chain's leaf number k = 1, 2, … of the transition, counter (c, k, 7, step), word 0
 *   purpose 8: the merge uniform of doubling j, counter (c, j, 8, step), word 0
 * Counter word 1, which holds d / 4 for the other purposes, holds j or the leaf number here.
 *
 * The eighth reads what the samplers stored: the convergence diagnostics of a cube of draws (octo_draws_diagnose_device: rank-normalised split-R̂,
 * bulk and tail ESS, three quantiles per row) and the rank step by itself (octo_draws_rank_device), stated in full at their declaration
 * (tests/diag_reference.py restates them). No random number.
 *
 * The ninth is a second explorer, a slice sampler (octo_draws_slice_device): coordinate-wise, gradient-free, with no step size and no metric,
 * the W chains walking through their coordinates in lockstep rounds of one forward log-posterior call, stated in full at its declaration
 * (tests/slice_reference.py restates it). Its stream adds
 *   purpose 9: uniform number i of update j of chain c at `step`, counter (c, j·128 + i, 9, step), word 0 (the interval's position: word 1 of i = 0)
 *
 * The tenth is what a parallel-tempering driver does between its scans (octo_draws_pt_stats_device, octo_draws_pt_schedule_device): the swap
 * acceptance probabilities, the stepping-stone sums of the log evidence and the tempered restarts of every scan, and once a round the communication
 * barrier and the ladder that equalises the rejection rates along it, stated in full at their declaration (tests/pt_reference.py restates them).
 * No model, no random number.
 *
 * The eleventh is the variational reference of a second tempering leg (octo_draws_reference_set_device … octo_draws_reference_exchange_device): a
 * mean-field normal on θ_t fitted to the target's own draws, kept as a prior table in caller-owned device memory, put under the handle's
 * functions in place of its own table, and the exchange of the two legs' target replicas, stated in full at their declaration
 * (tests/vref_reference.py restates them). No model, no random number.
 *
 * The twelfth is derived variables (octo_draws_program_set … octo_draws_program_values_device): the straight-line arithmetic a variable block puts
 * between θ and the kernel inputs, as an expression program that the device interprets forward and reverse in place of octo_model_logpost_device, under
 * every function of the handle that needs ℓπ, stated in full at its declaration (tests/program_reference.py restates it). No random number.
 *
 * The thirteenth is nested sampling (octo_draws_cube_device … octo_draws_nested_move_device): the unit cube behind the prior draws and the hypercube
 * transform out of it, the ordered cull of a live set with its evidence bookkeeping, and a constrained-prior slice move in the cube in lockstep rounds,
 * stated in full at their declaration (tests/nested_reference.py restates them). Its two streams add
 *   purpose 10: the survivor that seeds dead rank r of iteration `iter`, counter (r, 0, 10, iter), word 0
 *   purpose 11: uniform number i of update j of live slot c at `iter`, counter (c, j·128 + i, 11, iter), word 0 (words 1 and 2 of i = 0: the interval's
 *               position and the split of the steps)
 *
 * The fourteenth is the dense metric of the HMC step and NUTS (octo_draws_cov_device … octo_draws_use_metric), stated at its declaration. No random number.
 *
 * The fifteenth is differential evolution (octo_draws_de_device): the gradient-free global search between the prior search and the local optimisers,
 * a population climbing ℓπ in generations of one forward log-posterior call, stated in full at its declaration (tests/de_reference.py restates it).
 * Its stream adds
 *   purpose 12: block k of individual i at generation gen, counter (i, k, 12, gen) — k = 0: the three parent picks and j_rand (words 0 … 3) · k = 1: the
 *               two adaptation tests and the two new values · k = 2 + d/4, word d % 4: the crossover uniform of coordinate d · k = 18 + d/4, word
 *               d % 4: the bound-repair uniform of coordinate d (D <= 64: the blocks of the two do not meet)
 *
 * The sixteenth is the OFTI rejection sampler (octo_draws_ofti_set … octo_draws_ofti_rejection): prior draws scored by the marginal likelihood of
 * ofti_linear_solve, the rejection step, and for every survivor a draw of the Thiele-Innes constants from their conditional normal with its Campbell
 * elements, stated in full at their declaration (tests/ofti_draws_reference.py restates them). Its stream adds
 *   purpose 13: the four standard normals of draw i's Thiele-Innes constants, counter (i, 0, 13, 0), words 0 … 3
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
#define OCTO_DRAWS_PURPOSE_MOMENTUM 2
#define OCTO_DRAWS_PURPOSE_ACCEPT   3
#define OCTO_DRAWS_PURPOSE_ELBO       4
#define OCTO_DRAWS_PURPOSE_PATHFINDER 5
#define OCTO_DRAWS_PURPOSE_NUTS_DIRECTION 6
#define OCTO_DRAWS_PURPOSE_NUTS_LEAF      7
#define OCTO_DRAWS_PURPOSE_NUTS_MERGE     8
#define OCTO_DRAWS_PURPOSE_SLICE 9

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

/* ---- The tempered HMC explorer. Chain c = chain0 + w (w < W) at `step`; D, the priors and (if any) the model are the handle's.
 *
 * Momentum   z_d = normcdfinv(uniform of word d % 4 of Philox(key, counter (c, d / 4, 2, step))), p_d = z_d / sqrt(inv_mass_d).
 * Target     E(θ_t) = ℓprior_t + β·(ℓπ − ℓprior_t) and ∇E = β·∇ℓπ + (1 − β)·∇ℓprior_t, with
 *              ℓπ, ∇ℓπ     octo_model_logpost_device;
 *              ℓprior_t    Σ_d logpdf_with_trans in declaration order — octo_draws_sample_device's d_logprior_t, the same routine, the
 *                          same order, the same sentinel −DBL_MAX when a term is non-finite (the healed prior of the model callback);
 *              ∇ℓprior_t   the derivative of the same routine; 0 in every coordinate when the prior was healed.
 *            β = 1 takes ∇E = ∇ℓπ bit for bit. β = 0 takes E = ℓprior_t and ∇E = ∇ℓprior_t and never consults ℓπ (a −Inf likelihood is
 *            no NaN there).
 * Trajectory n_leapfrog >= 1 leapfrog steps of size ε_w with the diagonal inverse mass: p += (ε/2)∇E, then n_leapfrog times
 *            { θ_t += ε·inv_mass·p;  p += ε∇E (the last time: (ε/2)∇E) }. K = ½ Σ_d inv_mass_d p_d², summed in index order. The start point
 *            is always evaluated (n_leapfrog + 1 log-posterior calls a step); nothing is kept from the previous step.
 * Decision   H = −E + K. A state is dead if E is not finite, if ℓprior_t is the sentinel, or if β > 0 and ℓπ is not finite.
 *            Accepted iff the end state is alive and (the start is dead or log u < H₀ − H₁), u the uniform of word 0 of counter
 *            (c, 0, 3, step). NaN runs through the trajectory and ends as a rejection; there is no other special case. A rejected chain
 *            keeps its θ_t bit for bit.
 * ℓ = ℓπ − ℓprior_t (not finite -> −Inf, as octo_draws_rejection defines it) is what octo_pt_step_device gathers.
 *
 * octo_draws_momentum_device: the momenta alone, d_p [D][ld], of chains chain0 … chain0 + n − 1; d_inv_mass [D] or NULL = 1.
 * OCTO_EINVAL: NULL handle, n < 0, ld < n, n > 2^30. */
int32_t octo_draws_momentum_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t n, int64_t ld,
                                   const double* d_inv_mass, double* d_p, void* hip_stream);

/* One step of W chains on DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no allocation once the handle's work
 * arrays hold (4·D + 4)·ld doubles (they grow behind the handle's own stream), no graph capture. The decision is made on the device.
 *   d_theta_t    [D][ld]  in/out: the states; an accepted chain receives its proposal, a rejected one is not written
 *   d_beta       [W]      or NULL: β = 1
 *   d_eps        [W]      or NULL: the scalar eps for every chain
 *   d_inv_mass   [D]      or NULL: 1
 *   d_theta_prop [D][ld]  or NULL: the end point of the trajectory, whatever the decision
 *   d_logpost    [W]      or NULL: ℓπ of the returned state
 *   d_loglike    [W]      or NULL: ℓ of the returned state
 *   d_dH         [W]      or NULL: H₀ − H₁
 *   d_accepted   [W]      int32 0 / 1
 * A handle without a model (created with model = NULL, or detached) explores the prior: β = 0 for every chain, d_beta is ignored,
 * d_logpost and d_loglike must be NULL.
 * OCTO_EINVAL: NULL handle; n_leapfrog < 1; W < 0, ld < W, W > 2^30; eps not finite or <= 0 with d_eps NULL; d_logpost or d_loglike on a
 * handle without a model; NULL d_theta_t or d_accepted with W > 0. */
int32_t octo_draws_hmc_step_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld,
                                   double* d_theta_t, const double* d_beta, const double* d_eps, double eps, int32_t n_leapfrog,
                                   const double* d_inv_mass, double* d_theta_prop, double* d_logpost, double* d_loglike,
                                   double* d_dH, int32_t* d_accepted, void* hip_stream);

/* The same step on HOST arrays of the same shapes, blocking, staged through the handle on its own stream: the same bits. */
int32_t octo_draws_hmc_step(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld,
                            double* theta_t, const double* beta, const double* eps_w, double eps, int32_t n_leapfrog,
                            const double* inv_mass, double* theta_prop, double* logpost, double* loglike,
                            double* dH, int32_t* accepted);

/* ---- Multi-start L-BFGS: W chains minimise f = −ℓπ over θ_t independently and in lockstep (stage 2 of the reference's initialisation,
 * src/initialization.jl:188-289: optimise from the best prior draws). D, the priors and the model are the handle's; ℓπ and ∇ℓπ come from
 * octo_model_logpost_device. Deterministic: no random number. The function is stated in full so that a restatement elsewhere
 * (tests/lbfgs_reference.py) and the device compute the same thing.
 *
 * Scaling    v = d_inv_mass [D], a variance per coordinate with the meaning it has in the HMC step (NULL: v = 1). It defines the metric
 *            ⟨a,b⟩_v = Σ_d v_d a_d b_d and ⟨a,b⟩_{1/v} = Σ_d a_d b_d / v_d. Every sum over d runs in index order.
 * Open       f, g at x = θ_t. The chain is DEAD if f or any g_d is not finite (its θ_t is never written). Otherwise d = −v⊙g, gd = gᵀd,
 *            t = min(1, 1/√⟨g,g⟩_v), trial = x + t·d; the ring is empty, the diagonal α = v, iters = 0, evals = 1.
 * Round      one log-posterior call at the trial points of all W chains (evals += 1 of every ACTIVE chain), then per chain:
 *   accept   iff f_t and every g_t,d are finite and f_t <= f + c1·t·gd, c1 = 1e-4. Then
 *            1. s = trial − x, y = g_t − g; x, f, g take the trial values; iters += 1; the backtrack count returns to 0.
 *            2. the pair (s, y, sᵀy) goes into a ring of m slots (over the oldest when full) iff sᵀy > 1e-10·√(⟨s,s⟩_{1/v}·⟨y,y⟩_v);
 *            3. with a stored pair the Pathfinder diagonal: a = ⟨y,y⟩_α, b = sᵀy, c = ⟨s,s⟩_{1/α} (all with the α before the update),
 *               α_d <- 1 / (a/(b·α_d) + y_d²/b − a·s_d²/(b·c·α_d²)) — the diagonal of the BFGS update of (a/b)·diag(1/α);
 *            4. max_d |g_d|·√v_d <= gtol: status GTOL. Otherwise ftol > 0 and |f_old − f| <= ftol·max(1, |f|): status FTOL.
 *            5. otherwise the new direction by the two-loop recursion over the stored pairs, newest first:
 *                 q = g; for each pair: c_k = sᵀq / sᵀy, q −= c_k·y;  r = γ·v⊙q, γ = sᵀy/⟨y,y⟩_v of the newest pair (1 with none);
 *                 for each pair, oldest first: r += (c_k − yᵀr / sᵀy)·s;  d = −r.
 *               gd = gᵀd; if gd is not < 0 the ring is emptied and d = −v⊙g. t = 1, trial = x + t·d.
 *   reject   t <- t/2, one more backtrack; more than 30 in a row: status LINESEARCH, the chain stays at x. Otherwise trial = x + t·d.
 * A chain whose status is not ACTIVE is frozen: its trial point is x, the result there is ignored, and its θ_t and every output keep their
 * bits for the rest of the call and across `resume`. */
#define OCTO_DRAWS_LBFGS_MAX_M 8
#define OCTO_DRAWS_LBFGS_ACTIVE     0
#define OCTO_DRAWS_LBFGS_GTOL       1
#define OCTO_DRAWS_LBFGS_FTOL       2
#define OCTO_DRAWS_LBFGS_LINESEARCH 3
#define OCTO_DRAWS_LBFGS_DEAD       4

/* The two-loop recursion alone (step 5 without the descent test), a pure function of its inputs, for callers who keep their own history;
 * the optimiser's kernel calls the same device routine. Asynchronous on hip_stream; the handle needs no model.
 *   d_cnt  [W] int32   stored pairs of the chain, 0 … m (clamped)
 *   d_head [W] int32   the slot the NEXT pair would take: the newest pair is in slot (head − 1) mod m, the one before it in (head − 2) mod m …
 *   d_S, d_Y [m][D][ld]  slot-major; sᵀy of a slot is summed from them in index order
 *   d_g [D][ld], d_inv_mass [D] or NULL = 1, d_dir [D][ld] out
 * OCTO_EINVAL: NULL handle; m outside 1 … OCTO_DRAWS_LBFGS_MAX_M; W < 0, ld < W, W > 2^30; a NULL array other than d_inv_mass with W > 0. */
int32_t octo_draws_lbfgs_direction_device(octo_draws* h, int64_t W, int64_t ld, int32_t m, const int32_t* d_cnt, const int32_t* d_head,
                                          const double* d_S, const double* d_Y, const double* d_g, const double* d_inv_mass,
                                          double* d_dir, void* hip_stream);

/* The optimiser on DEVICE buffers, asynchronous on hip_stream: no host synchronisation, and no allocation once the handle's work arrays
 * hold ((5 + 2m)·D + 2m + 11)·ld doubles (they grow behind the handle's own stream). resume = 0 opens and makes n_rounds rounds:
 * n_rounds + 1 log-posterior calls. resume = 1 continues the state the handle holds with n_rounds more rounds: the same W, ld and m as the
 * call before it, and d_theta_t as that call left it. Two calls of a and b rounds give the bits of one call of a + b.
 *   d_theta_t       [D][ld]  in/out: x of every chain; a DEAD chain's column is never written
 *   d_inv_mass      [D]      or NULL: v = 1
 *   d_logpost       [W]      ℓπ at the returned θ_t (of a DEAD chain: what the callback gave)
 *   d_gnorm         [W]      max_d |g_d|·√v_d there (of a DEAD chain: NaN)
 *   d_status        [W]      int32 OCTO_DRAWS_LBFGS_*
 *   d_iters, d_evals [W]     int32: accepted steps, log-posterior evaluations while the chain was ACTIVE (the opening one included)
 *   d_inv_hess_diag [D][ld]  or NULL: α
 * OCTO_EINVAL: NULL handle; a handle without a model (created with model = NULL, or detached); m outside 1 … OCTO_DRAWS_LBFGS_MAX_M;
 * n_rounds < 0; W < 0, ld < W, W > 2^30; gtol or ftol not finite or < 0; resume without a previous call or with another W, ld or m; a NULL
 * array other than d_inv_mass and d_inv_hess_diag with W > 0. */
int32_t octo_draws_lbfgs_device(octo_draws* h, int64_t W, int64_t ld, double* d_theta_t, const double* d_inv_mass, int32_t m,
                                int32_t n_rounds, double gtol, double ftol, int32_t resume, double* d_logpost, double* d_gnorm,
                                int32_t* d_status, int32_t* d_iters, int32_t* d_evals, double* d_inv_hess_diag, void* hip_stream);

/* The same optimisation (resume = 0) on HOST arrays of the same shapes, blocking, staged through the handle on its own stream: the same bits. */
int32_t octo_draws_lbfgs(octo_draws* h, int64_t W, int64_t ld, double* theta_t, const double* inv_mass, int32_t m, int32_t n_rounds,
                         double gtol, double ftol, double* logpost, double* gnorm, int32_t* status, int32_t* iters, int32_t* evals,
                         double* inv_hess_diag);

/* ---- Pathfinder (Zhang, Carpenter, Gelman & Vehtari 2022) on the L-BFGS paths: stage 3 of the reference's initialisation. At every accepted
 * iterate of a chain the L-BFGS state defines a normal approximation N(μ, Σ) of the posterior in θ_t; an ELBO estimate from a few draws scores
 * it; the chain keeps the best; octo_draws_pathfinder_draw_device draws from the kept one. The function is stated in full so that a
 * restatement elsewhere (tests/pathfinder_reference.py) and the device compute the same thing. D <= OCTO_DRAWS_PF_MAX_D.
 *
 * Write g = ∇f = −∇ℓπ at x, α the Pathfinder diagonal, and the chain's cnt stored pairs oldest first: pair k = 0 … cnt − 1 sits in slot
 * (head − cnt + k) mod m. Every sum over a coordinate or a pair runs in index order.
 * Fit        in the scaled space s̃ = s/√α, ỹ = y·√α, from H̃ = I; for each pair, oldest first:
 *              w = H̃ỹ, ρ = 1/(s̃ᵀỹ), H̃_ij <- H̃_ij − ρ·(s̃_i·w_j + w_i·s̃_j) + ρ·(1 + ρ·ỹᵀw)·(s̃_i·s̃_j)      (the inverse-BFGS update).
 *            Σ = diag(√α)·H̃·diag(√α) is the L-BFGS inverse Hessian with H₀ = diag(α): the matrix of the paper's compact form
 *            diag(α) + [αY, S]·γ·[αY, S]ᵀ, dense because D <= 64 (2·cnt can exceed D, and a Cholesky factor is unique).
 *            μ = x − √α ⊙ (H̃(√α ⊙ g)). L̃ is the lower Cholesky factor of H̃, row by row from the left: the pivot of column j is
 *            H̃_jj − Σ_{k<j} L̃_jk², the entry below it (H̃_ij − Σ_{k<j} L̃_ik·L̃_jk)/L̃_jj. logdet Σ = Σ_d log α_d + 2·Σ_d log L̃_dd.
 *            The fit fails (ok = 0) if an α_d or a pivot is not finite and > 0; a failed fit is no candidate. With cnt = 0, Σ = diag(α).
 * Draw       φ = μ + √α ⊙ (L̃z), log q(φ) = −½(D·log 2π + logdet Σ + zᵀz). z_d = normcdfinv(uniform of word d % 4 of Philox(key, counter
 *            (chain0 + c, d / 4, purpose, t))): purpose 4 and t = iters_c·32 + k for ELBO draw k of the chain's iterate number iters_c,
 *            purpose 5 and t = j for final draw j. The counter depends on the chain and its own iterate count, never on the round or the batch.
 * ELBO       (1/K)·Σ_k (ℓπ(φ_k) − log q(φ_k)), K = n_elbo; a draw with a non-finite ℓπ makes it −Inf.
 * Selection  a chain keeps the fit with the greatest ELBO over its accepted iterates (those that ended an L-BFGS round with iters advanced;
 *            one that reaches GTOL or FTOL included; the opening point is not fitted). The comparison is strict: the earliest fit wins a
 *            tie, −Inf never wins. The fit uses x, g, α and the ring as they stand after the round. DEAD chains and chains that never
 *            accept have no fit. n_fits counts the candidates (fits with ok = 1). */
#define OCTO_DRAWS_PF_MAX_D 64
#define OCTO_DRAWS_PF_MAX_ELBO_DRAWS 32

/* The fit alone, a pure function of a caller's history (the twin of octo_draws_lbfgs_direction_device: the same d_cnt, d_head, d_S, d_Y; the
 * Pathfinder kernel is the same kernel). Asynchronous on hip_stream; the handle needs no model.
 *   d_x, d_g, d_alpha [D][ld]   in
 *   d_mu     [D][ld]            μ
 *   d_chol   [D(D+1)/2][ld]     L̃ packed row-major: L̃_ij (j <= i) in row i(i+1)/2 + j
 *   d_logdet [W], d_ok [W] int32
 *   n, d_z [n][D][ld] -> d_phi [n][D][ld]   the draw map applied to the caller's z (n = 0: both may be NULL); of a chain with ok = 0: undefined
 * OCTO_ENOTSUP: D > OCTO_DRAWS_PF_MAX_D. OCTO_EINVAL: NULL handle; m outside 1 … OCTO_DRAWS_LBFGS_MAX_M; W < 0, ld < W, W > 2^30; n < 0,
 * n·W > 2^30; a NULL array with W > 0 (d_z, d_phi: with n > 0). */
int32_t octo_draws_pathfinder_fit_device(octo_draws* h, int64_t W, int64_t ld, int32_t m, const int32_t* d_cnt, const int32_t* d_head,
                                         const double* d_S, const double* d_Y, const double* d_x, const double* d_g, const double* d_alpha,
                                         double* d_mu, double* d_chol, double* d_logdet, int32_t* d_ok, int32_t n, const double* d_z,
                                         double* d_phi, void* hip_stream);

/* octo_draws_lbfgs_device with Pathfinder along the path: the arguments, the outputs and `resume` of that call (which it makes, one round at
 * a time: d_theta_t and the L-BFGS outputs have the bits that call gives), and per round the fit of every chain whose iters advanced, n_elbo
 * draws of each into a dense batch [D][n_elbo·W] (draw k of chain c in column k·W + c; a chain without a new fit sends its x and the
 * result is ignored), ONE log-posterior call on the batch, the ELBO and the selection. n_rounds·2 + 1 log-posterior calls when resume = 0.
 * Asynchronous on hip_stream, no host synchronisation, and no allocation once the work arrays hold (D² + 5D + 8)·ld doubles of fits (two per
 * chain, the kept one and the candidate: promotion is a flag flip) and (D + 2)·n_elbo·W of the batch, besides those of the L-BFGS.
 * resume = 1 continues the previous octo_draws_pathfinder_device call of the handle (no octo_draws_lbfgs_device call of the handle's in
 * between, other than a resumed one); n_elbo may differ. A chain's outputs do not depend on W, ld or its position: only on chain0 + c.
 *   d_elbo      [W]        the ELBO of the kept fit, −Inf without one
 *   d_elbo_iter [W] int32  the iters of the kept fit, −1 without one
 *   d_n_fits    [W] int32
 * OCTO_ENOTSUP: D > OCTO_DRAWS_PF_MAX_D. OCTO_EINVAL: as octo_draws_lbfgs_device, W > 2^25, n_elbo outside 1 … OCTO_DRAWS_PF_MAX_ELBO_DRAWS,
 * resume without a previous call of THIS function with the same W, ld and m, a NULL d_elbo, d_elbo_iter or d_n_fits with W > 0. */
int32_t octo_draws_pathfinder_device(octo_draws* h, uint64_t seed, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t,
                                     const double* d_inv_mass, int32_t m, int32_t n_rounds, double gtol, double ftol, int32_t n_elbo,
                                     int32_t resume, double* d_logpost, double* d_gnorm, int32_t* d_status, int32_t* d_iters,
                                     int32_t* d_evals, double* d_inv_hess_diag, double* d_elbo, int32_t* d_elbo_iter, int32_t* d_n_fits,
                                     void* hip_stream);

/* n_draws draws from the kept fit of every chain of the previous octo_draws_pathfinder_device call (the same W, ld, d_theta_t, chain0),
 * and ONE log-posterior call on them. Asynchronous on hip_stream.
 *   d_phi     [D][ld_out]  ld_out >= n_draws·W; draw j of chain c in column j·W + c
 *   d_logq    [n_draws·W]  log q(φ)
 *   d_logpost [n_draws·W]  ℓπ(φ)
 * Of a chain without a fit: φ = its x, log q = NaN, ℓπ = −Inf.
 * OCTO_ENOTSUP: D > OCTO_DRAWS_PF_MAX_D. OCTO_EINVAL: NULL handle; a handle without a model; n_draws < 1; W < 0, ld < W, n_draws·W > 2^30;
 * ld_out < n_draws·W; no previous octo_draws_pathfinder_device call, or one with another W or ld; a NULL array with W > 0. */
int32_t octo_draws_pathfinder_draw_device(octo_draws* h, uint64_t seed, uint64_t chain0, int64_t W, int64_t ld, const double* d_theta_t,
                                          int32_t n_draws, int64_t ld_out, double* d_phi, double* d_logq, double* d_logpost, void* hip_stream);

/* ---- Warm-up of the explorer: what turns octo_draws_hmc_step_device into a sampler — the cross-chain statistics that give it d_inv_mass (the
 * pooled variance of the chains) and d_eps (dual averaging on the mean acceptance probability), and the per-chain moments R̂ is made of. Five
 * calls on DEVICE arrays, asynchronous on hip_stream, no host synchronisation, no allocation once the handle's work array holds
 * ⌈W/256⌉·G·(2K + 1) doubles, no random number (no new Philox purpose), no model needed. Every sum runs in a fixed order — no floating-point
 * atomic anywhere — so a call's outputs are the same bits from run to run, and they depend neither on ld, nor on what lies beyond column W, nor
 * on the values of excluded chains. tests/adapt_reference.py restates the five. K, the rows of an array [K][ld], is an argument of its own
 * (1 … 64), not the handle's D: the same call serves a [1][ld] array.
 *
 * Grouped moments. Chain w belongs to group d_group[w] (int32); d_group NULL: every chain in group 0, and G must be 1. A chain is EXCLUDED
 * from every row if its id is outside 0 … G − 1 or if any of its K values is not finite. Over the remaining chains of group g:
 *   d_count [G]     their number n, a double holding an exact integer
 *   d_mean  [G][K]  (Σ x)/n
 *   d_m2    [G][K]  Σ (x − mean)²
 * Order: a block of 256 consecutive chains sums each row of a group by a butterfly over the 64 lanes of a wave and then over its four waves
 * in wave order, takes the block's mean, and sums (x − that mean)² the same way; the blocks' triples (n, Σx, M2) are merged in block order,
 * δ = Σx_b/n_b − Σx_a/n_a, M2 = M2_a + M2_b + δ²·n_a·n_b/(n_a + n_b); mean = Σx/n at the end.
 * accumulate = 0 overwrites the three arrays; an empty group gives count 0, mean 0, M2 0. accumulate = 1 Chan-merges this call's block b into
 * what they hold (a): n = n_a + n_b, δ = mean_b − mean_a, mean = mean_a + δ·n_b/n, M2 = M2_a + M2_b + δ²·n_a·n_b/n; a group empty in this call
 * is left untouched, and a group whose held count is 0 takes this call's values.
 * OCTO_EINVAL: NULL handle or array (d_group excepted, and d_x with W = 0); K or G outside 1 … OCTO_DRAWS_MAX_GROUPS; NULL d_group with G != 1 and W > 0; W < 0,
 * ld < W, W > 2^24. */
#define OCTO_DRAWS_MAX_GROUPS 64
int32_t octo_draws_moments_device(octo_draws* h, int64_t W, int64_t ld, int32_t K, const double* d_x, const int32_t* d_group, int32_t G,
                                  int32_t accumulate, double* d_count, double* d_mean, double* d_m2, void* hip_stream);

/* One group's moments (d_count_g [1], d_mean_g [K] — not consulted, kept for symmetry —, d_m2_g [K]: rows of the arrays above) as a metric:
 * var_d = M2_d/(n − 1); regularize = 0: v_d = var_d; regularize = 1, Stan's shrinkage: v_d = (n/(n + 5))·var_d + 1e-3·5/(n + 5).
 * d_inv_mass[d] is written only where n >= 2 and v_d is finite and > 0; elsewhere it keeps its value.
 * OCTO_EINVAL: NULL handle or array; K outside 1 … OCTO_DRAWS_MAX_GROUPS. */
int32_t octo_draws_metric_device(octo_draws* h, int32_t K, const double* d_count_g, const double* d_mean_g, const double* d_m2_g,
                                 int32_t regularize, double* d_inv_mass, void* hip_stream);

/* Dual averaging of the step size (Hoffman & Gelman 2014, as Stan's stepsize_adaptation). d_state [G][4] = (x, x̄, H̄, μ) of group g, x = log ε.
 * init: x = x̄ = log ε0_g, H̄ = 0, μ = log(10·ε0_g); ε0_g = d_eps0[g], or the scalar eps0 with d_eps0 NULL.
 * OCTO_EINVAL: NULL handle or d_state; G outside 1 … OCTO_DRAWS_MAX_GROUPS; eps0 not finite or <= 0 with d_eps0 NULL. */
int32_t octo_draws_hmc_adapt_init_device(octo_draws* h, int32_t G, const double* d_eps0, double eps0, double* d_state, void* hip_stream);

/* Update number k >= 1 from the outputs d_dH, d_accepted of one octo_draws_hmc_step_device over W chains.
 *   per chain   a_c = min(1, exp(dH_c)) where dH_c is not NaN; otherwise a_c = accepted_c ? 1 : 0 (defined whatever a dead state left in d_dH)
 *   per group   a_g = the mean of a_c: the grouped reduction of octo_draws_moments_device on one row, the same exclusion by id (d_group NULL:
 *               G must be 1). d_accept_stat [G] (may be NULL) receives it, NaN for an empty group.
 *   update      η = 1/(k + t0); H̄ <- (1 − η)·H̄ + η·(δ − a_g); x <- μ − (√k/γ)·H̄; w = k^(−κ); x̄ <- w·x + (1 − w)·x̄.
 *               An empty group keeps its state bit for bit.
 *   d_eps_w [W] (may be NULL) receives exp(x_g) of the chain's group — with use_average = 1, exp(x̄_g) —, what d_eps of the step takes.
 *               Excluded chains are not written.
 * Stan's values: delta = 0.8, gamma = 0.05, t0 = 10, kappa = 0.75.
 * OCTO_EINVAL: NULL handle, d_dH, d_accepted or d_state; G out of range; NULL d_group with G != 1 and W > 0; W < 0, W > 2^24; k < 1; delta, gamma, t0,
 * kappa not finite or outside 0 < delta < 1, gamma > 0, t0 >= 0, kappa > 0. */
int32_t octo_draws_hmc_adapt_device(octo_draws* h, int64_t W, const int32_t* d_group, int32_t G, const double* d_dH, const int32_t* d_accepted,
                                    int64_t k, double delta, double gamma, double t0, double kappa, double* d_state, double* d_accept_stat,
                                    int32_t use_average, double* d_eps_w, void* hip_stream);

/* Per-chain running moments over time, lane = chain: d_cmean, d_cm2 [K][ld] of d_x [K][ld], k >= 1 the number of this sample.
 * k = 1: mean = x, M2 = 0, whatever the arrays held. Otherwise Welford: δ = x − mean, mean += δ/k, M2 += δ·(x − mean). Non-finite values
 * propagate. OCTO_EINVAL: NULL handle or array; K out of range; W < 0, ld < W, W > 2^24; k < 1.
 *
 * R̂ (Gelman & Rubin) of n samples per chain follows from these with no further function. Per coordinate d:
 *   B/n  = M2/(count − 1) of octo_draws_moments_device(d_cmean): the variance of the chain means;
 *   Wv   = the mean of octo_draws_moments_device(d_cm2), divided by n − 1: the mean within-chain variance;
 *   R̂_d = √(((n − 1)/n·Wv + B/n)/Wv). */
int32_t octo_draws_chain_moments_device(octo_draws* h, int64_t W, int64_t ld, int32_t K, int64_t k, const double* d_x, double* d_cmean,
                                        double* d_cm2, void* hip_stream);

/* ---- The no-U-turn sampler (Hoffman & Gelman 2014; the reference samples with AdvancedHMC's NUTS: multinomial sampling, the generalised
 * no-U-turn criterion, tree depth <= 10, Δ_max = 1000). One transition of W chains, built in lockstep: a ROUND is one log-posterior call at the
 * trial points of all W chains and one leapfrog of every chain still building. Chain c = chain0 + w at `step`. E, ∇E, dead states, ℓprior_t, β
 * and the handle without a model are exactly those of the HMC step above (a term of ℓprior_t is non-finite also where the linked x rounds onto a
 * bound of the prior's support, log|J| = log 0: such a point is dead); ⟨a,b⟩ = Σ_d inv_mass_d·a_d·b_d; every sum over d runs in index order.
 *
 * Open       p₀: the momenta octo_draws_hmc_step_device draws for (seed, step, c). The start is evaluated: H₀ = −E₀ + K₀, K as in the HMC step.
 *            A dead start ends the transition at once: θ_t is not written, n_leapfrog = 0, accepted = 0. Otherwise the tree is the start
 *            point: both endpoints (θ_t, p₀, ∇E₀), the proposal θ_t, ρ = p₀, log w = 0, depth j = 0.
 * Doubling j adds a subtree of 2^j leaves in the direction v = +1 if u < ½, else −1, u of counter (c, j, 6, step), built from the endpoint on
 *            that side, which every new leaf replaces. A leaf is one leapfrog: p½ = p + v(ε/2)∇E, q′ = q + vε·inv_mass⊙p½, the evaluation at
 *            q′, p′ = p½ + v(ε/2)∇E′. Δ = (−E′ + K′) − H₀. The leaf DIVERGES if q′ is dead or not (Δ <= 1000) — NaN diverges. Its weight is
 *            log w_leaf = −Δ (−Inf when it diverges); it adds min(1, exp(−Δ)) (0 when it diverges) to the acceptance statistic.
 * Subtree    leaf n = 0 … 2^j − 1: log w_s <- logaddexp(log w_s, log w_leaf) (n = 0: log w_leaf). The subtree's proposal becomes the leaf iff
 *            n = 0 or log u < log w_leaf − log w_s (the new one), u of counter (c, k, 7, step), k = 1, 2, … the chain's leaf number in this
 *            transition. ρ_s is the running sum of the subtree's p′ in build order.
 *            Checkpoints, i_max = popcount(n >> 1), t = the trailing one-bits of n, i_min = i_max − t + 1: an even n stores (p′, ρ_s) in slot
 *            i_max; an odd n tests, for i = i_max down to i_min, ρ = ρ_s − ρ_ckpt[i] + p_ckpt[i]: the subtree TURNS iff ⟨p_ckpt[i], ρ⟩ <= 0 or
 *            ⟨p′, ρ⟩ <= 0, and the first turn stops the tests. That tests every aligned sub-subtree that ends at leaf n (the test is symmetric in
 *            the direction) with max_depth slots. A turning or diverging subtree ends the transition with the tree's proposal unchanged.
 * Merge      of a completed subtree: the tree's proposal becomes the subtree's iff log u < log w_s − log w (biased progressive sampling), u of
 *            counter (c, j, 8, step); log w <- logaddexp(log w, log w_s); ρ <- ρ + ρ_s; j <- j + 1. The transition ends if ⟨p_left, ρ⟩ <= 0
 *            or ⟨p_right, ρ⟩ <= 0, or if j = max_depth. No further junction test is made.
 * End        θ_t takes the proposal — it is written only if the proposal is not the start point —, and ℓπ and ℓ of it are returned. depth is j,
 *            the doublings merged; n_leapfrog counts every leaf made, the one that diverged or turned included. A chain that has ended is
 *            FROZEN, as in the L-BFGS: its trial point is its θ_t, the result there is ignored, and θ_t and every output keep their bits for the
 *            rest of the call and across `resume`.
 *
 * On DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no allocation once the handle's work array holds
 * ((14 + 2·max_depth)·D + 18)·ld doubles (it grows behind the handle's own stream), no graph capture, no floating-point atomic. resume = 0 opens and
 * makes n_rounds rounds: n_rounds + 1 log-posterior calls. resume = 1 continues the state the handle holds with n_rounds more rounds: the same W, ld,
 * max_depth, seed, step and chain0 as the call before it, and the other inputs and d_theta_t as that call had and left them. Two calls of a and b
 * rounds give the bits of one call of a + b; 2^max_depth − 1 rounds always finish every chain. A chain's outputs depend only on chain0 + c, never
 * on W, ld, its position or how the rounds were cut.
 *   d_theta_t, d_beta, d_eps, eps, d_inv_mass   as octo_draws_hmc_step_device
 *   d_logpost, d_loglike [W]   or NULL: ℓπ and ℓ of θ_t as the call leaves it (of a chain still building: of its start)
 *   d_log_accept [W]           or NULL: the log of the mean acceptance statistic over the leaves made; NaN with n_leapfrog = 0. min(1, exp(·)) of
 *                              it is what octo_draws_hmc_adapt_device makes of its d_dH argument: the warm-up calls take it where dH went.
 *   d_accepted   [W]           int32: 1 iff θ_t was written
 *   d_depth, d_n_leapfrog, d_diverged [W]   int32 or NULL (of a chain still building: so far)
 *   d_n_active   [1]           int32 or NULL: the chains still building after the call
 * OCTO_EINVAL: as octo_draws_hmc_step_device (without n_leapfrog); max_depth outside 1 … OCTO_DRAWS_NUTS_MAX_DEPTH; n_rounds < 0; resume without
 * a previous call of the same W, ld, max_depth, seed, step and chain0. */
#define OCTO_DRAWS_NUTS_MAX_DEPTH 10
int32_t octo_draws_nuts_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t,
                               const double* d_beta, const double* d_eps, double eps, const double* d_inv_mass, int32_t max_depth,
                               int32_t n_rounds, int32_t resume, double* d_logpost, double* d_loglike, double* d_log_accept,
                               int32_t* d_accepted, int32_t* d_depth, int32_t* d_n_leapfrog, int32_t* d_diverged, int32_t* d_n_active,
                               void* hip_stream);

/* ---- The slice sampler (Neal 2003, "Slice sampling", Ann. Statist. 31: the doubling procedure of Fig. 4, the shrinkage of Fig. 5, the acceptance
 * test of Fig. 6; the explorer the reference's octofit_pigeons runs, Pigeons' SliceSampler). One transition of W chains: n_passes sweeps over the
 * D coordinates of θ_t in index order, update number j = pass·D + d changing coordinate d alone. Chain c = chain0 + w at `step`. The target is E
 * of the HMC step above, with its ℓprior_t (the same routine, order and sentinel), its β = 1 and β = 0, its dead states and its handle without a
 * model; a dead trial point has E = −Inf. No gradient is evaluated anywhere. A ROUND is one forward octo_model_logpost_device call at the trial
 * points of all W chains — a chain's trial point is its θ_t but for the coordinate it is updating — and one step of every chain's state machine.
 * Chains advance through their coordinates independently: none waits for another.
 *
 * Width      w_d = d_width[d], or the scalar w with d_width NULL. p = the number of doublings, max_shrink = the shrink proposals of an update.
 * Uniforms   u_i = the uniform of word 0 of counter (c, j·128 + i, 9, step); u′ = that of word 1 of the counter of i = 0.
 * Open       E₀ at θ_t. A dead start ends the chain at once: θ_t is not written, the status is DEAD, every count is 0.
 * Level      x = coordinate d of θ_t. z = E₀ + log u_0; L = x − w_d·u′; R = L + w_d. E_L is evaluated, then E_R.
 * Doubling   for k = 1 … p: stop if neither z < E_L nor z < E_R; otherwise, if u_k < ½, L <- L − (R − L) and E_L is evaluated, else
 *            R <- R + (R − L) and E_R is evaluated.
 * Shrink     from L̄ = L, R̄ = R, for s = 0 … max_shrink − 1: x′ = L̄ + u_{64+s}·(R̄ − L̄); E′ is evaluated. x′ is a candidate iff z < E′, and a
 *            candidate is accepted iff it passes the test below. On acceptance coordinate d of θ_t is written with x′, and E₀, ℓπ and ℓprior_t of
 *            the chain become those evaluated at x′: nothing is evaluated twice. Otherwise x′ < x sets L̄ <- x′, else R̄ <- x′. After max_shrink
 *            proposals the coordinate keeps its value and n_stuck counts it.
 * Test       L̂ = L, R̂ = R, E_L̂ = E_L, E_R̂ = E_R, the flag off. While R̂ − L̂ > 1.1·w_d: M = (L̂ + R̂)/2; the flag goes on if (x < M) != (x′ < M);
 *            x′ < M sets R̂ <- M, else L̂ <- M; the new endpoint is evaluated, in every iteration; the candidate is rejected iff the flag is on and
 *            z >= E_L̂ and z >= E_R̂. It passes when the loop ends. With p = 0 the loop never runs.
 * End        after n_passes·D updates the status is DONE. A chain that is DONE or DEAD is FROZEN, as in NUTS: its trial point is its θ_t, the
 *            result there is ignored, and θ_t and every output keep their bits for the rest of the call and across `resume`.
 * An update takes 2 + (doublings made) + (shrink proposals) + (test midpoints) rounds: at most 2 + p + max_shrink·(1 + p).
 *
 * On DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no allocation once the handle's work array holds (2·D + 28)·ld doubles
 * (it grows behind the handle's own stream), no graph capture, no floating-point atomic. resume = 0 opens and makes n_rounds rounds: n_rounds + 1
 * log-posterior calls. resume = 1 continues the state the handle holds with n_rounds more rounds: the same W, ld, p, n_passes, max_shrink, seed,
 * step and chain0 as the call before it, and the other inputs and d_theta_t as that call had and left them. Two calls of a and b rounds give the
 * bits of one call of a + b. A chain's outputs depend only on chain0 + c, never on W, ld, its position or how the rounds were cut.
 *   d_theta_t    [D][ld]  in/out: a coordinate is written where its update accepts a proposal
 *   d_beta       [W]      or NULL: β = 1 (as octo_draws_hmc_step_device)
 *   d_width      [D]      or NULL: the scalar w for every coordinate
 *   d_logpost, d_loglike [W]   or NULL: ℓπ and ℓ of θ_t as the call leaves it
 *   d_n_eval, d_n_expand, d_n_shrink, d_n_stuck [W]   int32 or NULL: the rounds the chain took part in (its evaluations, the opening one not
 *                         counted), the doublings made, the shrink proposals made, the updates that ran out of proposals — so far
 *   d_status     [W]      int32 or NULL: OCTO_DRAWS_SLICE_*
 *   d_n_active   [1]      int32 or NULL: the chains still ACTIVE after the call
 * OCTO_EINVAL: NULL handle; w not finite or <= 0 with d_width NULL; p outside 0 … OCTO_DRAWS_SLICE_MAX_DOUBLINGS; max_shrink outside
 * 1 … OCTO_DRAWS_SLICE_MAX_SHRINK; n_passes outside 1 … OCTO_DRAWS_SLICE_MAX_PASSES; n_rounds < 0; W < 0, ld < W, W > 2^30; d_logpost or d_loglike
 * on a handle without a model; NULL d_theta_t with W > 0; resume without a previous call of the same W, ld, p, n_passes, max_shrink, seed, step
 * and chain0. */
#define OCTO_DRAWS_SLICE_MAX_DOUBLINGS 8
#define OCTO_DRAWS_SLICE_MAX_SHRINK 64
#define OCTO_DRAWS_SLICE_MAX_PASSES 1024
#define OCTO_DRAWS_SLICE_ACTIVE 0
#define OCTO_DRAWS_SLICE_DONE   1
#define OCTO_DRAWS_SLICE_DEAD   2
int32_t octo_draws_slice_device(octo_draws* h, uint64_t seed, uint64_t step, uint64_t chain0, int64_t W, int64_t ld, double* d_theta_t,
                                const double* d_beta, const double* d_width, double w, int32_t p, int32_t n_passes, int32_t max_shrink,
                                int32_t n_rounds, int32_t resume, double* d_logpost, double* d_loglike, int32_t* d_n_eval, int32_t* d_n_expand,
                                int32_t* d_n_shrink, int32_t* d_n_stuck, int32_t* d_status, int32_t* d_n_active, void* hip_stream);

/* ---- Convergence diagnostics of stored draws (Vehtari, Gelman, Simpson, Carpenter & Bürkner 2021; the table the reference's user reads after
 * octofit: ess_bulk, ess_tail and the rank-normalised split-R̂). The function is stated in full so that a restatement elsewhere
 * (tests/diag_reference.py) and the device compute the same thing. On DEVICE arrays, asynchronous on hip_stream, no host synchronisation, no
 * random number, no model needed; no allocation once the handle's work array holds octo_draws_diagnose_work_doubles(n, W, K) doubles.
 *
 * Input      d_x: n samples of K rows of W chains, element (i, k, w) at d_x[i·ls + k·ld + w], ld >= W, ls >= K·ld. The recorded θ_t of the samplers
 *            is this with ls = D·ld, their recorded ℓπ with K = 1 and ls = ld. K is an argument of its own (1 … OCTO_DRAWS_MAX_GROUPS), not the handle's D.
 * Split      N = ⌊n/2⌋. Split chain m = h·W + w (h = 0, 1) holds samples h·(n − N) … h·(n − N) + N − 1 of chain w: draw i of m is sample h·(n − N) + i.
 *            With n odd the middle sample, number N, belongs to no split chain: it is UNUSED throughout (never read for a statistic, never written
 *            by the rank step). With n even this is the split of posterior and ArviZ. M = 2W split chains, S = M·N used draws per row.
 * Validity   A row with a used draw that is not finite, and a row whose used draws are all equal, has NaN in every statistic (the quantiles
 *            included) and NaN in every rank and z of the rank step. The other rows are not affected.
 * Quantiles  s = the S used draws of the row sorted ascending. Type 7: q_p = s[lo] + (h − lo)·(s[lo+1] − s[lo]), h = (S − 1)·p, lo = ⌊h⌋, every
 *            operation rounded by itself (no fused multiply-add), for p = 0.05, 0.5 and 0.95. The median is q_0.5 by this formula.
 * Ranks      r(x) = #{s < x} + (#{s = x} + 1)/2: the average rank, 1-based, exact in a double. The comparison is that of doubles: −0 = +0.
 *            z(x) = normcdfinv((r − 3/8)/(S + 1/4)). Folded: the same applied to y = |x − median| among the S values of y.
 * Sums over the split chains — Σ_m below — run in the order octo_draws_moments_device documents: within a block of 256 consecutive split
 *            chains a butterfly over the 64 lanes of each wave (a lane beyond M holds 0), the four waves added in wave order from 0; the blocks
 *            then added in block order from 0. No floating-point atomic anywhere.
 * ESS(v)     of M split chains of N draws v_{m,i} (Stan's compute_effective_sample_size):
 *              μ_m = (Σ_i v_{m,i})/N, summed in index order;
 *              acov_m(t) = (Σ_{i=0}^{N−1−t} (v_{m,i} − μ_m)·(v_{m,i+t} − μ_m))/N, summed in index order (a product may be fused into the sum);
 *              var_m = acov_m(0)·N/(N − 1);   W̄ = (Σ_m var_m)/M;   μ̄ = (Σ_m μ_m)/M;
 *              var⁺ = W̄·(N − 1)/N + (Σ_m (μ_m − μ̄)²)/(M − 1);   Ā(t) = (Σ_m acov_m(t))/M;   ρ_0 = 1, ρ_t = 1 − (W̄ − Ā(t))/var⁺.
 *            Geyer's truncation exactly as Stan writes it: even = 1, odd = ρ_1, t = 1; while t < N − 4 and even + odd > 0: even = ρ_{t+1},
 *            odd = ρ_{t+2}, both are STORED as ρ̂_{t+1}, ρ̂_{t+2} iff even + odd >= 0, t += 2. max_t = t. If even > 0: ρ̂_{max_t+1} = even.
 *            ρ̂_0 = 1, ρ̂_1 = ρ_1, and a ρ̂ that was not stored is 0. Monotone pass, for t = 1, 3, … <= max_t − 3: if ρ̂_{t+1} + ρ̂_{t+2} >
 *            ρ̂_{t−1} + ρ̂_t, both take (ρ̂_{t−1} + ρ̂_t)/2. τ = −1 + 2·Σ_{t<max_t} ρ̂_t + ρ̂_{max_t+1}, summed in index order;
 *            τ <- max(τ, 1/log10(S)); ESS = S/τ. A var⁺ that is not finite or not > 0 gives NaN.
 * split-R̂(v) = √(var⁺/W̄), from the same lag-0 quantities.
 * Outputs    d_out [OCTO_DRAWS_DIAG_N_STATS][K], statistic-major:
 *              RHAT        max(split-R̂(z), split-R̂(z_folded)), NaN if either is
 *              ESS_BULK    ESS(z)
 *              ESS_TAIL    min(ESS(1[x <= q_0.05]), ESS(1[x <= q_0.95])), NaN if either is
 *              RHAT_BASIC  split-R̂(x)            ESS_BASIC   ESS(x)
 *              Q05, Q50, Q95   the three quantiles
 * The outputs are the same bits from run to run, and they depend neither on ld, nor on ls, nor on what lies beyond column W or in the unused
 * sample.
 * Work       octo_draws_diagnose_work_doubles(n, W, K) = 2K(P + S) + 10KM + 4K·T·(nblk + 1) + 5K doubles, P = max(2048, the least power of two >= S),
 *            T = 16·⌈N/16⌉, nblk = ⌈M/256⌉: the sorted keys of x and of y, z and z_folded, the chains' means and variances, the block sums of
 *            acov_m(t) and ρ, the quantiles and two flags per row. Host only, no handle; 0 for arguments the two calls refuse.
 * OCTO_EINVAL: NULL handle or array; K outside 1 … OCTO_DRAWS_MAX_GROUPS; n < 8; W < 1; ld < W; ls < K·ld. OCTO_ENOTSUP: S = 2·N·W > 2^24. */
#define OCTO_DRAWS_DIAG_RHAT 0
#define OCTO_DRAWS_DIAG_ESS_BULK 1
#define OCTO_DRAWS_DIAG_ESS_TAIL 2
#define OCTO_DRAWS_DIAG_RHAT_BASIC 3
#define OCTO_DRAWS_DIAG_ESS_BASIC 4
#define OCTO_DRAWS_DIAG_Q05 5
#define OCTO_DRAWS_DIAG_Q50 6
#define OCTO_DRAWS_DIAG_Q95 7
#define OCTO_DRAWS_DIAG_N_STATS 8
int32_t octo_draws_diagnose_device(octo_draws* h, int64_t n, int64_t W, int64_t ld, int64_t ls, int32_t K, const double* d_x, double* d_out,
                                   void* hip_stream);
int64_t octo_draws_diagnose_work_doubles(int64_t n, int64_t W, int32_t K);

/* The rank step alone (the twin that octo_draws_lbfgs_direction_device is to the optimiser: the diagnosis launches the same kernels): r and/or z of
 * every used draw, written on the strides of d_x — element (i, k, w) of d_rank and d_z at [i·ls + k·ld + w]. Either output may be NULL; an unused
 * middle sample is not written. fold = 1 ranks y = |x − median|. The work array and the status codes are those of octo_draws_diagnose_device. */
int32_t octo_draws_rank_device(octo_draws* h, int64_t n, int64_t W, int64_t ld, int64_t ls, int32_t K, const double* d_x, int32_t fold,
                               double* d_rank, double* d_z, void* hip_stream);

/* ---- Parallel tempering between the scans (non-reversible parallel tempering: Syed, Bouchard-Côté, Deligiannidis & Doucet 2021, the scheme of
 * Pigeons, which the reference's octofit_pigeons runs; the stepping-stone estimator of Xie, Lewis, Fan, Kuo & Chen 2011). The layout is that of
 * octo_pt_swap_device: d_ll [T][Cn] by replica (walker r·Cn + c), d_slot2rep [Cn][T] int32, d_beta [T] with slot 0 the target; T = 2 … OCTO_DRAWS_MAX_GROUPS,
 * Cn = 1 … 2^24. On DEVICE arrays, asynchronous on hip_stream, no model, no random number, no floating-point atomic, no allocation once the
 * handle's work array holds 7·(T − 1)·⌈Cn/256⌉ doubles (the array of octo_draws_moments_device's block partials).
 *
 * octo_draws_pt_stats_device: one call per scan, on the ℓ and the slot2rep the swap step is about to see. For chain c and pair t (slots t, t + 1):
 * li = ℓ of the replica at slot t, lj = ℓ of the replica at slot t + 1, db = β_t − β_{t+1}. A replica index outside 0 … T − 1 reads ℓ = NaN.
 * The caller-owned state d_acc [T − 1][8] of doubles holds (n, A, n_f, m_f, s_f, n_b, m_b, s_b) per pair; before its first call every m is −Inf
 * and the rest 0.
 *   α          the swap's acceptance PROBABILITY: both li and lj finite: min(1, exp(db·(lj − li))); otherwise 1 where the swap kernel accepts for every
 *              uniform (lj finite, li not, β_t > β_{t+1}); otherwise 0. n += 1 and A += α for EVERY pair at every scan, whatever the parity the
 *              swap step tries: the Rao-Blackwellised rate. The accepted-swap counts of octo_pt_swap_device are another statistic and stay.
 *   Forward    stepping-stone term (the draws of slot t + 1 estimating Z_t/Z_{t+1}): v = db·lj, counted in n_f. lj = −Inf — a dead prior draw at the
 *              cold end — adds exp(−Inf) = 0 to the sum and 1 to n_f, decided before the multiply so that db = 0 gives no NaN; lj NaN or +Inf is skipped.
 *   Backward   term (the draws of slot t estimating Z_{t+1}/Z_t): v = −db·li, counted in n_b; skipped unless li is finite.
 *   (m, s)     a streaming log-sum-exp: m the maximum so far, s = Σ exp(v − m). A call forms its own (m_call, s_call) first and merges them into
 *              the held pair: m' = max(m, m_call), s' = s·exp(m − m') + s_call·exp(m_call − m'). A side without a term (m = −Inf) leaves the other's (m, s) untouched;
 *              the counts add.
 * Order of the sums: that of octo_draws_moments_device — a butterfly over the 64 lanes of a wave (a lane beyond Cn holds 0), the four waves of a
 * block of 256 consecutive chains in wave order from 0, the blocks in block order from 0. A block's log-sum-exp takes the block maximum first
 * (exact) and sums exp(v − max) in that order; the blocks merge in block order by the rule above, from an empty pair, and the call's pair then
 * merges into the held one. A is the call's sum added to the held A. The outputs are the same bits from run to run, and they do not depend on
 * what the excluded terms held.
 *   Restarts   d_leg [Cn][T] (int32, 0/1, by replica) and d_restarts [Cn] (int32), both NULL or both given, zero before the first call: for each
 *              chain the replica at slot T − 1 gets leg = 1; the replica at slot 0 with leg = 1 adds one to d_restarts[c] and gets leg = 0. A
 *              tempered restart is a journey from the reference (β_{T−1}) to the target (β_0).
 * OCTO_EINVAL: NULL handle, d_ll, d_slot2rep, d_beta or d_acc; one of d_leg, d_restarts without the other; T or Cn out of range. The values of
 * d_beta are not read on the host here (the call stays asynchronous): α is defined for any β, and octo_draws_pt_schedule_device refuses a ladder
 * that is not non-increasing. */
int32_t octo_draws_pt_stats_device(octo_draws* h, int32_t T, int64_t Cn, const double* d_ll, const int32_t* d_slot2rep, const double* d_beta,
                                   double* d_acc, int32_t* d_leg, int32_t* d_restarts, void* hip_stream);

/* octo_draws_pt_schedule_device: one call per round, from d_acc. For t = 0 … T − 2:
 *   r_t        = 1 − A/n clipped to [0, 1]: the rejection rate of pair t. With n = 0 it is NaN, and the ladder is left unchanged.
 *   Λ          Λ_0 = 0, Λ_{t+1} = Λ_t + r_t, summed in t order; Λ = Λ_{T−1}, the communication barrier between the target and the reference.
 *   β*         β*_0 = β_0 and β*_{T−1} = β_{T−1} bit for bit. For k = 1 … T − 2: g = k·Λ/(T − 1), t the first index with Λ_{t+1} >= g, and
 *              β*_k = β_t + (β_{t+1} − β_t)·(g − Λ_t)/(Λ_{t+1} − Λ_t), every operation rounded by itself; the denominator is positive by
 *              construction. If Λ is 0 or not finite the ladder is copied through. LINEAR interpolation of Λ(β) between the nodes is a
 *              deliberate choice: Pigeons interpolates Λ monotonically with a smoother curve; a linear one needs no derivative estimate, keeps β*
 *              inside [β_{t+1}, β_t] and has the same fixed point, equal rejection rates.
 *   d_beta_out [T], may be d_beta itself · d_rej [T − 1] = r_t · d_summary [4] = (Λ, fwd, rev, ½(fwd + rev)) with the two stepping-stone estimates of
 *              log Z: fwd = Σ_t (m_f + log(s_f/n_f)), rev = −Σ_t (m_b + log(s_b/n_b)), both summed in t order. A pair with nothing to say makes
 *              its sum NaN, not silently smaller.
 *   adapt = 0  statistics only: β is copied through. reset = 1 puts d_acc back to its state before the first call (every m = −Inf, the rest 0)
 *              once it has been read, so that a driver starts the next round without a host call.
 * The kernel is one wave. The call copies d_beta [T] to the host to check it and waits for hip_stream to do so: one synchronisation, once a round.
 * OCTO_EINVAL: NULL handle or array; T out of range; a d_beta that is not non-increasing from slot 0 (a NaN included). */
int32_t octo_draws_pt_schedule_device(octo_draws* h, int32_t T, double* d_acc, const double* d_beta, int32_t adapt, int32_t reset, double* d_beta_out,
                                      double* d_rej, double* d_summary, void* hip_stream);

/* ---- The variational reference of a tempering leg (Pigeons' GaussianReference, a mean-field normal in the unconstrained space, fitted by moment
 * matching to the target's draws of the previous round; Surjanovic, Syed, Bouchard-Côté & Campbell 2022 anneal a second leg from it and join the
 * two legs at the target. Recalled, not checked against Pigeons' source). A normal N(μ_d, σ_d) on θ_t is a prior of kind OCTO_PRIOR_NORMAL, whose
 * link is the identity: with it as the handle's prior table ℓprior_t is log q(θ_t), the tempered target is (1 − β)·log q + β·ℓπ,
 * octo_draws_sample_device draws μ + σ·Φ⁻¹(u), and the explorers' d_loglike is ℓπ − log q: the swap potential of a leg that anneals from q, what
 * octo_pt_swap_device and octo_draws_pt_stats_device take. The handle's D is the number of coordinates throughout.
 *
 * The reference table d_ref: octo_draws_reference_doubles(D) = 15·D doubles of CALLER-owned device memory (0 for D < 1) — octo_prior [D] (40 bytes
 * each), the density constants [D][4], the quantile constants [D][4], μ [D], σ [D], in this order. Host only, no handle.
 *
 * octo_draws_reference_set_device writes it from d_mean [D], d_sd [D]; octo_draws_reference_fit_device from ONE group's rows of
 * octo_draws_moments_device (d_count_g [1], d_mean_g [D], d_m2_g [D]): μ_d = mean_d, σ_d = inflate·√(M2_d/(n − 1)), each operation rounded by itself.
 * One wave, lane = coordinate. Coordinate d is BAD if μ_d or σ_d is not finite, σ_d <= 0, or (fit) n < 2. For every good coordinate:
 *   octo_prior   kind = OCTO_PRIOR_NORMAL, pad = 0, p0 = μ, p1 = σ, lo = −Inf, hi = +Inf
 *   constants    {NaN, 0 (= 1/(b − a) with both ends open), −log σ, 1/σ}: the entries octo_draws_create forms for a Normal; the quantile constants 0
 *   μ, σ         as used
 * A bad coordinate keeps every byte it had, so THE FIRST CALL ON A FRESH BUFFER MUST BE CLEAN: a table with a coordinate that was never written is
 * no prior table. d_bad [1] (int32) receives the number of bad coordinates — written, not accumulated. No host synchronisation, no allocation:
 * a driver re-fits between rounds and reads d_bad when it next waits anyway.
 * OCTO_EINVAL: NULL handle or array; (fit) inflate not finite or <= 0. */
int64_t octo_draws_reference_doubles(int32_t D);
int32_t octo_draws_reference_set_device(octo_draws* h, const double* d_mean, const double* d_sd, double* d_ref, int32_t* d_bad, void* hip_stream);
int32_t octo_draws_reference_fit_device(octo_draws* h, const double* d_count_g, const double* d_mean_g, const double* d_m2_g, double inflate, double* d_ref,
                                        int32_t* d_bad, void* hip_stream);

/* From the next call on, every function of the handle that reads the prior table — octo_draws_sample_device, octo_draws_best, octo_draws_rejection,
 * the HMC step, NUTS, the slice sampler, the L-BFGS and Pathfinder — reads d_ref instead; NULL restores the handle's own table. Host only: two
 * pointers change hands, nothing is copied, so the table may be re-fitted in place while it is active (work already enqueued reads whatever the
 * table holds when it runs: order the re-fit on the same stream) and must outlive its use; its lifetime is the caller's. The call forgets the
 * resume records of NUTS, the slice sampler and the L-BFGS: a transition is never resumed on another target. OCTO_EINVAL: NULL handle. */
int32_t octo_draws_use_reference(octo_draws* h, const double* d_ref);

/* The exchange of two legs at the target. Leg A (T_a slots) and leg B (T_b slots) hold Cn chains each in the layout of octo_pt_swap_device:
 * d_slot2rep [Cn][T] int32, d_theta [D][ld] with replica r of chain c in column r·Cn + c, d_lp (ℓπ) and d_ll (the swap potential) by replica.
 * d_ref_a, d_ref_b: the legs' reference tables, NULL = the handle's own prior (octo_draws_create's table, whether or not a reference is active). Lane = chain c;
 * with column a = slot2rep_a[c][0]·Cn + c of leg A and b likewise of leg B:
 *   θ_t    the D values of column a of d_theta_a and of column b of d_theta_b trade places, bit for bit; so do d_lp_a[a] and d_lp_b[b]
 *   ℓ      each side's potential under ITS OWN reference at its NEW point: d_ll_a[a] = ℓπ_b − ℓprior_t,A(θ_b), d_ll_b[b] = ℓπ_a − ℓprior_t,B(θ_a),
 *          ℓprior_t by the routine and in the order of the explorers; −Inf where the difference is not finite or the prior was healed.
 * No other element of the six arrays is written. A chain with a slot-0 replica index outside 0 … T − 1 in either leg exchanges nothing.
 * Why this is a valid move: both target replicas are at β = 1, where the tempered density of EITHER leg is π whatever its reference, and the two
 * legs are independent; exchanging two independent states with the same marginal leaves the joint law unchanged, so the exchange is always
 * accepted. It is how a tempered restart of one leg reaches the other.
 * OCTO_EINVAL: NULL handle or array (the references excepted); T_a or T_b < 2; Cn < 1 or > 2^30; ld_a < T_a·Cn or ld_b < T_b·Cn; d_theta_a == d_theta_b. */
int32_t octo_draws_reference_exchange_device(octo_draws* h, int64_t Cn, int32_t T_a, const int32_t* d_slot2rep_a, int64_t ld_a, double* d_theta_a,
                                             double* d_lp_a, double* d_ll_a, const double* d_ref_a, int32_t T_b, const int32_t* d_slot2rep_b, int64_t ld_b,
                                             double* d_theta_b, double* d_lp_b, double* d_ll_b, const double* d_ref_b, void* hip_stream);

/* ---- Derived variables: expression programs (the twelfth part). The reference's `@variables` block produces, next to the priors, a short
 * straight-line list of arithmetic on θ evaluated in declaration order: a = cbrt(M·P²), e = h² + k², tp = τ·P·365.25 + t_ref. Such a list is
 * DATA. A handle created with a context and WITHOUT a model takes one (octo_draws_program_set), and from then on every function of the handle
 * that needs ℓπ — octo_draws_best, octo_draws_rejection, the HMC step, NUTS, the slice sampler, the L-BFGS, Pathfinder — evaluates
 * octo_draws_program_logpost_device where a handle with a model evaluates octo_model_logpost_device. No generated code: an interpreter, forward
 * and reverse, on the device (tests/program_reference.py restates it).
 *
 * Nodes. Node d < D is the natural parameter x_d = invlink_d(θ_t[d]) of the handle's prior d; node D + j is the result of op j. An operand
 * index must be lower than the node's own index (declaration order is topological order); a node may have any number of consumers.
 * Ops (IEEE / ocml routines, not the fast-math variants of the one-θ path): */
#define OCTO_DRAWS_OP_CONST 0    /* value                                   */
#define OCTO_DRAWS_OP_ADD   1    /* a + b                                   */
#define OCTO_DRAWS_OP_SUB   2    /* a − b                                   */
#define OCTO_DRAWS_OP_MUL   3    /* a·b                                     */
#define OCTO_DRAWS_OP_DIV   4    /* a/b                                     */
#define OCTO_DRAWS_OP_NEG   5    /* −a                                      */
#define OCTO_DRAWS_OP_SQRT  6
#define OCTO_DRAWS_OP_CBRT  7
#define OCTO_DRAWS_OP_EXP   8
#define OCTO_DRAWS_OP_LOG   9
#define OCTO_DRAWS_OP_SIN   10
#define OCTO_DRAWS_OP_COS   11
#define OCTO_DRAWS_OP_ATAN2 12   /* atan2 with a = y, b = x: the reference's atan(y, x)  */
#define OCTO_DRAWS_OP_POWC  13   /* pow of a and value                      */
#define OCTO_DRAWS_OP_MULC  14   /* a·value                                 */
#define OCTO_DRAWS_OP_ADDC  15   /* a + value                               */
#define OCTO_DRAWS_N_OPS    16
#define OCTO_DRAWS_PROGRAM_MAX_OPS 192   /* with D <= 64: D + n_ops <= 256 nodes, 128 KB of the 160 KB of LDS at 512 B a node */
typedef struct octo_draws_op   { int32_t op, a, b, pad; double value; } octo_draws_op;    /* 24 bytes; operands an op does not read: 0 */
/* Bindings: one per kernel input in the order octo_eval_device reads them, n_planets·OCTO_N_EL elements, then n_obs·OCTO_N_NUIS nuisances.
 *   OCTO_DRAWS_BIND_NODE   the input is the value of `node`
 *   OCTO_DRAWS_BIND_TPERI  only on the OCTO_EL_TP slot of a Campbell planet whose A, E, I, W, O and M slots are NODE bindings: the input is
 *                          θ_at_epoch_to_tperi with node = the angle, value = theta_epoch and M, e, a, i, ω, Ω the planet's six bound nodes,
 *                          in closed form with its gradient into all seven, with the constants of octo_consts_default. Flag
 *                          OCTO_DRAWS_BIND_FLAG_TI in the upper half of `kind` says the planet is a Thiele-Innes planet — the dataset is
 *                          opaque to this library, the caller knows — and is answered with OCTO_ENOTSUP. */
#define OCTO_DRAWS_BIND_NODE  0
#define OCTO_DRAWS_BIND_TPERI 1
#define OCTO_DRAWS_BIND_FLAG_TI 65536
typedef struct octo_draws_bind { int32_t kind, node; double value; } octo_draws_bind;  /* 16 bytes */
/* Terms: terms[n_terms] are node indices whose values are added to ℓπ on the likelihood side of the split, as k_model_fwd treats the
 * UnitLengthPrior of a UniformCircular pair (written in primitives here): they survive a healed prior and are tempered with ℓ.
 *
 * octo_draws_program_set copies ops, binds and terms to the device and validates on the host; ds (a dataset of n_planets planets and n_obs tables
 * made with the handle's context) must outlive the program. It replaces a program already set and forgets the resume records of NUTS, the slice
 * sampler and the L-BFGS. octo_draws_program_clear removes the program: the handle is a sampling-only handle again.
 *   OCTO_EINVAL   NULL handle, ds or a NULL array with a non-zero count; a handle WITH a model, or without a context; n_planets < 1, n_obs < 0;
 *                 n_binds != n_planets·OCTO_N_EL + n_obs·OCTO_N_NUIS; an unknown op ("op j: …"); an operand that is not an earlier node
 *                 (forward reference); a binding of unknown kind or with a node out of range ("binding k: …"); a TPERI binding on a slot that
 *                 is not OCTO_EL_TP, or whose planet has another of its seven as a non-NODE binding; a term index out of range ("term i: …")
 *   OCTO_ENOTSUP  n_ops > OCTO_DRAWS_PROGRAM_MAX_OPS; a TPERI binding flagged Thiele-Innes; more LDS than the device has
 *
 * octo_draws_program_logpost_device: the signature and the contract of octo_model_logpost_device — d_theta_t [D][ld], W columns, d_lp [W],
 * d_grad [D][ld] or NULL, asynchronous on hip_stream, elements beyond W in a row never written. Three steps on the stream, lane = walker, one
 * wave a block, no host synchronisation and no allocation once the handle's work array (prog_work of csrc/draws/octo_draws_layout.h,
 * (N + 2·D + 2·n_in + 7·P + 3)·ldw doubles at N = D + n_ops nodes, n_in inputs, P planets and ldw = W rounded up to 64) is large enough:
 *   k_prog_fwd   x_d, dx_d/dθ_t and logpdf_with_trans of each prior in declaration order (the routines of the model callback, ALWAYS on the table
 *                given to octo_draws_create, whatever octo_draws_use_reference has put in place); the ops in order, node values in LDS
 *                [node][64] (with a gradient: streamed to the work array as well); the inputs; Σ terms in the order given
 *   octo_eval_device   ℓ and ∂ℓ/∂inputs
 *   k_prog_bwd   adjoints in LDS, zero but for the inputs' ∂ℓ/∂input (a TPERI input: times its closed-form gradient, into its seven nodes) and 1
 *                for every term, in that order; the ops in reverse order, operand values read back from the work array; then
 *                ∂/∂θ_t[d] = adjoint_d·dx_d/dθ_t + ∂prior_d/∂θ_t. No atomics: a lane owns its column, the order of accumulation is the program's.
 * Semantics, those of octo_model_logpost_device: prior part = Σ logpdf_with_trans, −1.7976931348623157e308 with zero prior gradient in every
 * coordinate if any term of it is not finite (the healing rule); −Inf if any θ_t entry is not finite; pp = prior part + Σ terms;
 * lp = isfinite(pp) ? pp + ℓ : pp; NaN becomes −Inf; the gradient row of a walker is 0 wherever its lp is not finite. A domain error inside the
 * program (log of a negative, e = h² + k² >= 1) is a NaN node: it reaches the likelihood as an invalid input, or pp as a NaN term, and costs
 * THAT walker −Inf with zero gradient — never a status, never another walker: a lane's result depends on its own column alone, bit for bit.
 * OCTO_EINVAL: NULL handle, no program, NULL d_theta_t or d_lp with W > 0, W < 0, ld < W, W > 2^30. W = 0 does nothing.
 *
 * octo_draws_program_values_device: d_out[k·ld_out + w] = the value of node nodes[k] (a HOST array of n indices, each 0 … N − 1; n <= 256) of
 * walker w: the derived columns of a chain, and the forward sweep on its own. Elements beyond W in a row are not written.
 * OCTO_EINVAL as above, and: n < 0 or > 256, a node out of range, ld_out < W. */
int32_t octo_draws_program_set(octo_draws* h, const octo_dataset* ds, int32_t n_planets, int32_t n_obs, const octo_draws_op* ops, int32_t n_ops,
                               const octo_draws_bind* binds, int32_t n_binds, const int32_t* terms, int32_t n_terms);
int32_t octo_draws_program_clear(octo_draws* h);
int32_t octo_draws_program_logpost_device(octo_draws* h, const double* d_theta_t, int64_t ld, int64_t W, double* d_lp, double* d_grad, void* hip_stream);
int32_t octo_draws_program_values_device(octo_draws* h, const double* d_theta_t, int64_t ld, int64_t W, const int32_t* nodes, int32_t n, double* d_out,
                                         int64_t ld_out, void* hip_stream);

/* ---- Nested sampling (the thirteenth part; Skilling 2006, "Nested sampling for general Bayesian computation"; the reference's fourth sampler is
 * dynesty behind a hypercube prior transform, ext/OctofitterDynestyHypercubeTransformExt.jl): K live points in the unit cube (0, 1)^D, the B lowest
 * likelihoods removed per iteration with their share of the prior volume, and B new points drawn from the prior restricted to ℓ > ℓ* by a
 * coordinate-wise slice move in the cube (Neal 2003, Fig. 3 and Fig. 5). The likelihood at a point is the rejection driver's: ℓ = ℓπ − ℓprior_t,
 * non-finite -> −Inf. All on DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no graph capture, no floating-point atomic.
 *
 * THE CUBE. octo_draws_cube_device writes u[d][t] (d_u [D][ld], t < n) = the uniform of word d % 4 of counter (first + t, d / 4, 0, 0): the numbers
 * octo_draws_sample_device feeds to the quantile. octo_draws_from_cube_device is the hypercube transform, every output optional: per coordinate, with
 * the routines of octo_draws_sample_device in its order, θ = the prior's quantile of u (moved one ulp inside where it rounds onto a bound),
 * θ_t = link(θ), and ℓprior_t accumulated in declaration order with the healing sentinel. from_cube(cube(seed, first, n)) is byte for byte
 * octo_draws_sample_device(seed, first, n) in all three outputs. A draw with ANY coordinate not inside (0, 1) — 0, 1, beyond, NaN — has every output
 * NaN (θ and θ_t in all D coordinates, ℓprior_t). The prior table is the handle's active one (octo_draws_use_reference applies).
 * OCTO_EINVAL: NULL handle; n < 0, ld < n, n > 2^30; first + n overflowing; NULL d_u with something to do.
 *
 * THE CULL. octo_draws_nested_cull_device, one iteration's bookkeeping on K live points, 2 <= K <= OCTO_DRAWS_NESTED_MAX_LIVE.
 *   Order     the live points ascending by (key, slot index), key = ℓ, or −Inf where ℓ is NaN or −Inf: a total order. Ranks r = 0 … B − 1 are the dead.
 *   Volume    t_r = 1/(K − r). With logX the state's log volume on entry: logX_r = logX_{r−1} − t_r (logX_{−1} = logX), one subtraction per rank in
 *             rank order; logwt_r = (key_r + logX_{r−1}) + log(−expm1(−t_r)).
 *   Evidence  logZ <- logaddexp(logZ, logwt_r) for r = 0 … B − 1 in that order; logaddexp(a, b) = max(a, b) + log1p(exp(−|a − b|)), −Inf when both are.
 *   State     d_state, 8 doubles in/out: [0] logZ · [1] logX = logX_{B−1} · [2] the floor ℓ* = key of rank B − 1 · [3] ℓmax = key of rank K − 1 (the
 *             largest live ℓ, before and after the replacement) · [4] the remaining-evidence bound logaddexp(logZ, ℓmax + logX) − logZ, +Inf while
 *             logZ = −Inf · [5] the number of dead so far · [6], [7] reserved, written 0. The initial state is (−Inf, 0, −Inf, −Inf, +Inf, 0, 0, 0).
 *   Records   at columns dead_first + r of caller arrays of leading dimension ld_dead (each may be NULL): d_dead_u [D][ld_dead] the u column of rank
 *             r, d_dead_loglike its key, d_dead_logvol logX_r, d_dead_logwt logwt_r. d_slot[r] = the live slot that held rank r.
 *   replace = 1 (1 <= B <= K − 1): slot d_slot[r] receives the u column and the ℓ (its bits, not its key) of the survivor of rank
 *             B + min(K − B − 1, ⌊v_r·(K − B)⌋), v_r = the uniform of word 0 of counter (r, 0, 10, iter). d_width[d] (or NULL) = max − min of
 *             coordinate d over all K live points as they stood on entry (fmax / fmin: exact, order-free).
 *   replace = 0 requires B = K: the final flush by the same rule; no seeds, d_width is not written, d_slot holds the whole order.
 * Nothing is written beyond column K of the live arrays or outside the B dead records. Non-finite inputs never trap. No allocation once the handle's
 * order array holds K doubles.
 * OCTO_EINVAL: NULL handle; K out of range; ldK < K; NULL d_u_live, d_loglike_live or d_state; replace not 0 or 1; B out of range for `replace`;
 * dead_first < 0 or dead_first + B > ld_dead; NULL d_slot.
 *
 * THE MOVE. octo_draws_nested_move_device, one constrained-prior transition of the B live slots named by d_slot (distinct), in place in d_u_live and
 * d_loglike_live, in lockstep ROUNDS as octo_draws_slice_device: a round is one forward log-posterior call at the trial points of all B chains and one
 * step of every chain's state machine. Chain = slot c = d_slot[w] at iteration `iter`. The floor ℓ* is read from d_state[2] on the device.
 *   Inside     inside(y) for coordinate d: 0 < y < 1 and ℓ(u with coordinate d replaced by y) > ℓ*. A y not in (0, 1) is outside without an
 *              evaluation and takes no round.
 *   Updates    n_passes sweeps over the D coordinates; update j = pass·D + d changes coordinate d alone. x = the coordinate, w_d = d_width[d] or w.
 *   Uniforms   v_i = word 0 of counter (c, j·128 + i, 11, iter); v′, v″ = words 1 and 2 of the counter of i = 0.
 *   Interval   L = x − w_d·v′, R = L + w_d.
 *   Stepping   m = max_steps: J = min(m − 1, ⌊m·v″⌋), Kr = m − 1 − J. While J > 0 and inside(L): L <- L − w_d, J <- J − 1 (n_step counts it). Then
 *              while Kr > 0 and inside(R): R <- R + w_d, Kr <- Kr − 1. With m = 1 there is no stepping out.
 *   Clip       L <- max(L, 0), R <- min(R, 1).
 *   Shrink     for s = 0 … max_shrink − 1: x′ = L + v_{64+s}·(R − L) (n_shrink counts it). If inside(x′) the coordinate becomes x′ and the slot's ℓ
 *              the ℓ evaluated there; the trial point keeps its transformed value: nothing is evaluated twice. Otherwise x′ < x sets L <- x′, else
 *              R <- x′ (an x′ that rounded onto 0 or 1 among them, without a round).
 *   Stuck      after max_shrink proposals the coordinate keeps its value and n_stuck counts it.
 *   End        after n_passes·D updates the status is DONE; a DONE chain is FROZEN: its outputs and its slot keep their bits for the rest of the
 *              call and across `resume`.
 * A trial coordinate reaches θ_t by the hypercube transform's routine; the opening gathers the B columns and transforms all D coordinates of them by
 * octo_draws_from_cube_device's launches. resume = 0 opens and makes n_rounds rounds; resume = 1 continues with n_rounds more: the same K, ldK, B, ld,
 * max_steps, n_passes, max_shrink, seed and iter, and the other arguments as that call had and left them. Two calls of a and b rounds give the bits
 * of one call of a + b. A chain's result depends only on its slot, iter and seed — never on B, ld, its position in d_slot or how the rounds were
 * cut. No allocation once the handle's work array holds (3·D + 15)·ld doubles.
 *   d_theta_t  [D][ld]  or NULL: θ_t of the B points as they stand
 *   d_n_eval, d_n_step, d_n_shrink, d_n_stuck [B]  int32 or NULL: the rounds the chain took part in, the steps out, the proposals, the stuck updates
 *   d_status   [B]      int32 or NULL: OCTO_DRAWS_NESTED_ACTIVE / _DONE
 *   d_n_active [1]      int32 or NULL: the chains still ACTIVE after the call
 * OCTO_EINVAL, each with a message: NULL handle; a handle with neither a model nor a program ("nested sampling needs a likelihood"); K out of range,
 * ldK < K, NULL d_u_live, d_loglike_live or d_state; B outside 0 … K − 1 or ld < B; w not in (0, 1] with d_width NULL; max_steps outside
 * 1 … OCTO_DRAWS_NESTED_MAX_STEPS; max_shrink outside 1 … OCTO_DRAWS_NESTED_MAX_SHRINK; n_passes outside 1 … OCTO_DRAWS_NESTED_MAX_PASSES;
 * n_rounds < 0; a resume that does not match the call before it; NULL d_slot with B > 0. */
#define OCTO_DRAWS_PURPOSE_NESTED_SEED 10
#define OCTO_DRAWS_PURPOSE_NESTED_MOVE 11
#define OCTO_DRAWS_NESTED_MAX_LIVE 4096
#define OCTO_DRAWS_NESTED_MAX_STEPS 64
#define OCTO_DRAWS_NESTED_MAX_SHRINK 64
#define OCTO_DRAWS_NESTED_MAX_PASSES 1024
#define OCTO_DRAWS_NESTED_ACTIVE 0
#define OCTO_DRAWS_NESTED_DONE   1
int32_t octo_draws_cube_device(octo_draws* h, uint64_t seed, uint64_t first, int64_t n, int64_t ld, double* d_u, void* hip_stream);
int32_t octo_draws_from_cube_device(octo_draws* h, int64_t n, int64_t ld, const double* d_u, double* d_theta, double* d_theta_t, double* d_logprior_t,
                                    void* hip_stream);
int32_t octo_draws_nested_cull_device(octo_draws* h, uint64_t seed, uint64_t iter, int32_t K, int64_t ldK, double* d_u_live, double* d_loglike_live,
                                      double* d_state, int32_t B, int32_t replace, int64_t dead_first, int64_t ld_dead, double* d_dead_u,
                                      double* d_dead_loglike, double* d_dead_logvol, double* d_dead_logwt, int32_t* d_slot, double* d_width,
                                      void* hip_stream);
int32_t octo_draws_nested_move_device(octo_draws* h, uint64_t seed, uint64_t iter, int32_t K, int64_t ldK, double* d_u_live, double* d_loglike_live,
                                      const double* d_state, int64_t B, int64_t ld, const int32_t* d_slot, const double* d_width, double w,
                                      int32_t max_steps, int32_t n_passes, int32_t max_shrink, int32_t n_rounds, int32_t resume, double* d_theta_t,
                                      int32_t* d_n_eval, int32_t* d_n_step, int32_t* d_n_shrink, int32_t* d_n_stuck, int32_t* d_status,
                                      int32_t* d_n_active, void* hip_stream);

/* ---- The dense metric (the fourteenth part; the reference's octofit runs NUTS with a dense Euclidean metric, AdvancedHMC's DenseEuclideanMetric, and
 * Stan's dense_e adapts it by the rule below): M⁻¹ = Σ = L·Lᵀ, L the lower Cholesky factor of a pooled covariance estimate of θ_t, PACKED by rows
 * (row i at i(i+1)/2, D(D+1)/2 doubles). All on DEVICE buffers, asynchronous on hip_stream; no floating-point atomic, the same bits on every run.
 *
 * THE WHITENED TRANSITION. While a factor is set (octo_draws_use_metric) octo_draws_hmc_step_device, octo_draws_hmc_step and octo_draws_nuts_device
 * simulate H = −E(θ_t) + ½pᵀΣp with p ~ N(0, Σ⁻¹), carried as the whitened momentum r = Lᵀp:
 *   r ~ N(0, I): the draw is octo_draws_momentum_device with a NULL metric, bit for bit · K = ½Σ r_d²
 *   kick   r += c·(Lᵀ∇E), ∇E the tempered gradient (∇ℓπ and ∇ℓprior_t mixed by β BEFORE the product) · drift  θ_t += ε·(L·r)
 *   every turn test ρᵀΣp is the plain product ρ_r·r with ρ_r = Σ r over the subtree: NUTS's checkpoints, ρ and ρ_s hold whitened momenta, its endpoint
 *   gradients hold Lᵀ∇E, and its tree logic, its counters and every output are those of the diagonal call. No work array grows.
 * A leapfrog is two triangular products per chain, each summed over the coordinate index in ascending order by fma. With L = diag(√inv_mass) the
 * transition is the diagonal one up to rounding. d_inv_mass must be NULL in those three calls while a factor is set (OCTO_EINVAL otherwise), and a
 * NUTS `resume` needs the factor pointer of the call it resumes (OCTO_EINVAL otherwise). The factor is CALLER-owned and read by every such call: it
 * must stay allocated and unchanged while a transition is open. octo_draws_momentum_device is unchanged; the L-BFGS, Pathfinder, the slice sampler,
 * nested sampling and the tempering statistics do not read the factor.
 *
 * octo_draws_cov_device: the pooled co-moments of the W chains in d_x [K][ld], one group, 1 <= K <= OCTO_DRAWS_DENSE_MAX_D. A chain with any
 * non-finite value is left out (octo_draws_moments_device's rule). d_count [1] = n, d_mean [K], d_m2 [K(K+1)/2] packed as L is:
 * Σ_w (x_i − mean_i)(x_j − mean_j). Block partials of 256 chains, two-pass about the block's mean, merged in block order by Chan's formula (cross term
 * d_i·d_j·n·n_b/(n + n_b)); with `accumulate` the result is then merged into what the three arrays hold (a held count of 0: replaced; a call without a
 * valid chain: untouched). The partials are cov_partials of csrc/draws/octo_draws_layout.h, nblk·(1 + K + K(K+1)/2) doubles of the handle's
 * moments allocation. OCTO_EINVAL: NULL handle; NULL d_count, d_mean or d_m2, NULL d_x with W > 0; K out of range; W < 0, ld < W, W > 2^24.
 *
 * octo_draws_metric_dense_device: Σ = M2/(n − 1); with `regularize` (n/(n + 5))·Σ + 1e-3·(5/(n + 5))·I, octo_draws_metric_device's constants. One
 * wave factors it in LDS (left-looking, lane = row). d_info [1] = 0: d_chol was written. d_info = j + 1: pivot j was not finite and > 0 (n < 2: 1), and
 * d_chol is UNTOUCHED. OCTO_EINVAL: NULL handle, a NULL array, K out of range.
 *
 * octo_draws_metric_apply_device: d_out [D][ld] = L·x (transpose = 0) or Lᵀ·x (transpose = 1) for the n columns of d_x [D][ld], D the handle's;
 * d_out may be d_x. The routines of the samplers' dense kernels behind an entry point: θ_t = μ + L·z from whitened draws, z = Lᵀ… of a gradient.
 * OCTO_EINVAL: NULL handle; D > OCTO_DRAWS_DENSE_MAX_D; n < 0, ld < n, n > 2^30; a NULL array with n > 0.
 *
 * octo_draws_use_metric: handle state, as octo_draws_use_reference. d_chol: the factor, D(D+1)/2 doubles, or NULL = back to the per-call diagonal
 * metric. OCTO_EINVAL: NULL handle; D > OCTO_DRAWS_DENSE_MAX_D with a non-NULL factor. */
#define OCTO_DRAWS_DENSE_MAX_D 64
int32_t octo_draws_cov_device(octo_draws* h, int64_t W, int64_t ld, int32_t K, const double* d_x, int32_t accumulate, double* d_count, double* d_mean,
                              double* d_m2, void* hip_stream);
int32_t octo_draws_metric_dense_device(octo_draws* h, int32_t K, const double* d_count, const double* d_m2, int32_t regularize, double* d_chol,
                                       int32_t* d_info, void* hip_stream);
int32_t octo_draws_metric_apply_device(octo_draws* h, int64_t n, int64_t ld, const double* d_chol, int32_t transpose, const double* d_x, double* d_out,
                                       void* hip_stream);
int32_t octo_draws_use_metric(octo_draws* h, const double* d_chol);

/* ---- Differential evolution (the fifteenth part; Storn & Price 1997, DE/rand/1/bin; the self-adaptation of Brest et al. 2006, "jDE"; the stage of the
 * reference's initialisation between its prior search and Pathfinder, src/initialization.jl:188-289, which calls BlackBoxOptim's
 * adaptive_de_rand_1_bin_radiuslimited — recalled, not read: that optimiser is steady-state on a host generator and its source is not in this tree.
 * This is the same family made GENERATIONAL, so that the W trial points of a generation share one forward octo_model_logpost_device call). The
 * function is stated in full so that a restatement elsewhere (tests/de_reference.py) and the device compute the same function.
 *
 * State      the population X = d_theta_t [D][ld] in θ_t, W individuals. f_i = ℓπ(X_i) — on a handle without a model ℓprior_t(X_i), with the
 *            HMC step's ℓprior_t (the same routine, order and sentinel); a set expression program and a reference table in use apply as they do
 *            to the slice sampler. A dead or non-finite point (the HMC step's dead states at β = 1, β = 0 without a model) has f = −Inf.
 *            Per individual (F_i, CR_i): d_fcr, or F = OCTO_DRAWS_DE_F0 and CR = OCTO_DRAWS_DE_CR0 at the opening with d_fcr NULL.
 * Uniforms   U(k, word) = the uniform of that word of counter (i, k, 12, gen), i the individual's index, gen = gen0 + g for generation g of the
 *            call. Every ⌊U·n⌋ below is at most n − 1.
 * A generation, for every individual i from the population and f as the generation before left them (the update is synchronous):
 * Parameters F′ = U(1,0) < OCTO_DRAWS_DE_TAU_F ? OCTO_DRAWS_DE_F_LOW + OCTO_DRAWS_DE_F_SPAN·U(1,1) : F_i · CR′ = U(1,2) < OCTO_DRAWS_DE_TAU_CR ? U(1,3) : CR_i
 * Neighbours n = W − 1 with radius = 0 (the whole population), otherwise n = min(max(2·radius, 3), W − 1). With h = ⌊n/2⌋, member
 *            m_k = (i − h + k + (k >= h ? 1 : 0)) mod W for k = 0 … n − 1: distinct, none of them i.
 * Parents    a = ⌊U(0,0)·n⌋ · b = ⌊U(0,1)·(n − 1)⌋, b += (b >= a) · c = ⌊U(0,2)·(n − 2)⌋, c += (c >= min(a, b)), then c += (c >= max(a, b)) ·
 *            r1 = m_a, r2 = m_b, r3 = m_c.
 * Trial      j_rand = ⌊U(0,3)·D⌋. Coordinate d CROSSES iff d = j_rand or U(2 + d/4, d % 4) < CR′: v_d = X[d][r3] + F′·(X[d][r1] − X[d][r2]), the
 *            difference, the product and the sum each rounded by itself (no fused multiply-add). The others keep v_d = X[d][i].
 * Bounds     with d_lo and d_hi: a crossing v_d < lo_d becomes lo_d + U(18 + d/4, d % 4)·(X[d][i] − lo_d), a crossing v_d > hi_d becomes
 *            hi_d − U(18 + d/4, d % 4)·(hi_d − X[d][i]), each operation rounded by itself. A NaN stays NaN. The population is not clipped.
 * Selection  f′ at v. The trial replaces the individual iff f′ > −Inf and f′ >= f_i: X_i, f_i, ℓ and ℓprior_t become the trial's (nothing is
 *            evaluated twice), (F_i, CR_i) <- (F′, CR′), and n_accept_i counts it.
 *
 * On DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no allocation once the handle's work array holds (5·D + 12)·ld doubles
 * (octo_draws_de_work_doubles; it grows behind the handle's own stream), no graph capture, no floating-point atomic. A generation is the forward
 * call and ONE launch: a lane decides its own selection and builds its next trial point from parents read as the selection leaves them, deciding
 * each parent's selection again from that parent's f and f′; the population and the trial points are kept twice, one copy read and one written.
 * resume = 0 opens — f of the population — and makes n_gen generations: n_gen + 1 log-posterior calls. resume = 1 continues the state the handle
 * holds (d_theta_t and d_fcr are then written only): the same seed, W, ld, radius and bounds, and gen0 = the gen0 + n_gen of the call before it.
 * Two calls of a and b generations give the bits of one call of a + b.
 *   d_theta_t    [D][ld]  in/out: the population; columns W … ld − 1 are not touched
 *   d_lo, d_hi   [D]      both or neither
 *   d_fcr        [2][ld]  or NULL: F, then CR; read at the opening, written by every call
 *   d_logpost, d_loglike [W]   or NULL: f and ℓ = f − ℓprior_t (−Inf where that is not finite) of the population as the call leaves it
 *   d_n_accept   [W]      int32 or NULL: acceptances since the opening
 *   d_best       [1]      int32 or NULL: the index of the highest finite f, ties to the lower index; −1 with none finite
 *   d_best_logpost [1]    or NULL: the f of that individual (−Inf with none)
 *   d_n_improved [1]      int32 or NULL: the acceptances of the last generation made (0 at the opening)
 * OCTO_EINVAL: NULL handle; W < 4, ld < W, W > 2^30; radius < 0; n_gen < 0; one of d_lo, d_hi without the other; NULL d_theta_t; d_logpost or
 * d_loglike on a handle without a model; resume without such a previous call. */
#define OCTO_DRAWS_PURPOSE_DE 12
#define OCTO_DRAWS_DE_TAU_F 0.1
#define OCTO_DRAWS_DE_F_LOW 0.1
#define OCTO_DRAWS_DE_F_SPAN 0.9
#define OCTO_DRAWS_DE_TAU_CR 0.1
#define OCTO_DRAWS_DE_F0 0.5
#define OCTO_DRAWS_DE_CR0 0.9
int32_t octo_draws_de_device(octo_draws* h, uint64_t seed, uint64_t gen0, int64_t W, int64_t ld, double* d_theta_t, const double* d_lo,
                             const double* d_hi, int32_t radius, int32_t n_gen, int32_t resume, double* d_fcr, double* d_logpost, double* d_loglike,
                             int32_t* d_n_accept, int32_t* d_best, double* d_best_logpost, int32_t* d_n_improved, void* hip_stream);
/* Host only: the doubles of that work array at D coordinates and leading dimension ld, (5·D + 12)·ld; 0 with D < 1 or ld < 0. */
int64_t octo_draws_de_work_doubles(int32_t D, int64_t ld);

/* ---- The sixteenth: the OFTI rejection sampler (examples/ofti_rejection_sampling.jl:78-108 of the reference): prior draws of (e, a, tp, M, plx), each
 * scored by the marginal likelihood of ofti_linear_solve (octo_ofti_eval_device of the main library), accepted with probability exp(ℓ − max ℓ), and every
 * survivor turned into an orbit: a draw of the Thiele-Innes constants from their conditional normal and the Campbell elements of that draw. The functions
 * are stated in full so that a restatement elsewhere (tests/ofti_draws_reference.py) and the device compute the same function.
 *
 * octo_draws_ofti_set: the handle must have D = 5 priors in the order (e, a, tp or τ, M, plx) and a context; it needs no model. The call creates an
 * octo_ofti of its own on the handle's context (octo_ofti_create: its input checks, its status and its message are passed through) and uploads the rows
 * of the table for k_oftis_post with the weights octo_ofti_create forms: det = σ_ra²σ_dec²(1 − ρ²), w_rr = σ_dec²/det, w_dd = σ_ra²/det,
 * w_rd = −ρσ_raσ_dec/det, p = w_rr·ra + w_rd·dec, q = w_dd·dec + w_rd·ra; λ = 1/σ_ABFG².
 *   tp_mode 0   the third coordinate is tp [MJD]
 *   tp_mode 1   the third coordinate is τ, tp = fma(τ, P_d, t_ref) with P_d = k_yr·sqrt(a·a·a/M), k_yr = consts->kepler_year_to_julian_day
 * consts (NULL: octo_consts_default) must be what the CONTEXT holds (octo_consts_set): the context's kernels form the period from theirs. The main
 * header has no call that reads a context's constants back, so this cannot be checked here: with other constants the draws are SCORED at one period
 * and their tp (tp_mode 1), P_d and M_dyn are formed at another, silently.
 * A second call replaces the first (one that fails past its argument checks leaves nothing set). octo_draws_ofti_clear undoes the call (no-op when nothing is set); octo_draws_destroy and octo_draws_detach release
 * the OFTI state first.
 * OCTO_EINVAL: NULL handle; D != 5; a handle without a context (detached); tp_mode outside 0, 1; t_ref not finite with tp_mode 1; and what
 * octo_ofti_create refuses. */
#define OCTO_DRAWS_PURPOSE_OFTI 13
#define OCTO_DRAWS_OFTI_N_OUT 16
int32_t octo_draws_ofti_set(octo_draws* h, const double* epochs, const double* ra, const double* dec, const double* sigma_ra, const double* sigma_dec,
                            const double* cor /*NULL = 0*/, int64_t n_epochs, double sigma_abfg, int32_t tp_mode, double t_ref,
                            const octo_consts* consts /*NULL = octo_consts_default*/);
int32_t octo_draws_ofti_clear(octo_draws* h);

/* θ (natural domain, d_theta [5][ld]: octo_draws_sample_device's) to the nl of octo_ofti_eval_device, d_nl [5][ld]: rows 0, 1, 3, 4 are copied, row 2 is tp
 * by the handle's tp_mode. Asynchronous on hip_stream. OCTO_EINVAL: NULL handle; nothing set; n < 0, ld < n; a NULL array with n > 0. */
int32_t octo_draws_ofti_nl_device(octo_draws* h, int64_t n, int64_t ld, const double* d_theta, double* d_nl, void* hip_stream);

/* The posterior draw of n parameter sets, lane = draw (k_oftis_post), asynchronous on hip_stream. Per draw with index i = d_index[k] and nl = column k:
 *   sums     the 13 sums of the normal equations over the rows of the table IN ROW ORDER by fma, from x = cos E − e, y = √(1 − e²)·sin E of the cold
 *            Kepler solve (Markley's starter and fifth-order correction with the half-angle polynomial sin/cos: octo_device.h, kepler_solve<-1, false>):
 *            Σw·xx, Σw·xy, Σw·yy for w = w_rr, w_dd, w_rd; Σx·q, Σy·q, Σx·p, Σy·p.
 *   solve    S = DᵀWD + λI in the order (A, B, F, G), its Cholesky factor L (S = L·Lᵀ), μ = S⁻¹b and ℓ, operation for operation as octo_ofti_eval_device's
 *            finishing kernel forms them; ℓ = −Inf by its rule: an element not finite, e outside [0, 1), a <= 0, M <= 0, S not positive definite, ℓ not finite.
 *   normals  z_k = normcdfinv(uniform of word k of Philox(key, counter (i, 0, 13, 0))), k = 0 … 3: octo_draws_momentum_device's routines.
 *   draw     x = μ + L⁻ᵀz by back substitution from k = 3: a function of (seed, i, nl) alone.
 *   elements with u+v = ((A + G)² + (B − F)²)/2 and u−v = ((A − G)² + (B + F)²)/2 — u = (A² + B² + F² + G²)/2, v = AG − BF, without their cancellation —
 *            s₊ = √(u+v), s₋ = √(u−v): α = (s₊ + s₋)/√2 [mas] · cos i = (s₊ − s₋)/(s₊ + s₋) · ω + Ω = atan2(B − F, A + G) · ω − Ω = atan2(−B − F, A − G) ·
 *            ω and Ω their half sum and half difference, folded by (ω, Ω) -> (ω ± π, Ω ± π) to Ω ∈ [0, π) and then ω by 2π to [0, 2π) · a_ti = α/plx [AU] ·
 *            P_d = k_yr·sqrt(a·a·a/M) [d] · M_dyn = M·a_ti³/a³, the total mass at which an orbit of semi-major axis a_ti has the period the solve used.
 *            The convention is the main library's: dec = A·X + F·Y, ra = B·X + G·Y, and its Campbell planet at (a_ti, e, i, ω, Ω, tp, M_dyn, plx) is its
 *            Thiele-Innes planet at the draw.
 *   d_out    [OCTO_DRAWS_OFTI_N_OUT][ld]: rows 0-3 the draw (A, B, F, G) · 4-7 μ · 8 α · 9 a_ti · 10 i · 11 ω · 12 Ω · 13 P_d · 14 M_dyn · 15 ℓ.
 *            A draw with ℓ = −Inf has NaN in rows 0-14. No lane reads another lane's data: an invalid draw leaves its neighbours their bits.
 * OCTO_EINVAL: NULL handle; nothing set; n < 0, ld < n; a NULL array with n > 0. */
int32_t octo_draws_ofti_posterior_device(octo_draws* h, uint64_t seed, int64_t n, int64_t ld, const uint64_t* d_index /*[n]*/, const double* d_nl /*[5][ld]*/,
                                         double* d_out /*[OCTO_DRAWS_OFTI_N_OUT][ld]*/, void* hip_stream);

/* The twin of octo_draws_rejection on the OFTI likelihood: HOST outputs, blocking, on the handle's stream. Pass 1, in chunks of 2^18 draws: the prior
 * draws (purpose 0), their nl, octo_ofti_eval_device without the means, ℓ (not finite -> −Inf) kept for all N at 8 bytes a draw. Pass 2 is
 * octo_draws_rejection's, the same kernels: draw i accepted iff ℓ_i != −Inf and its purpose-1 uniform is below exp(ℓ_i − max ℓ); accepted draws in
 * draw-index order. θ of the stored draws is regenerated from the counter, then their nl and their posterior draw as above.
 * Row 15 of post_out is octo_draws_ofti_posterior_device's OWN ℓ, not the ℓ that decided acceptance: the two kernels solve Kepler's equation with
 * different sin/cos routines and sum the rows in different orders, so they agree to rounding (1e-9·max(1, |ℓ|) is the tested bar) and not bit for bit;
 * *max_logml is pass 1's. In principle a draw that pass 1 accepts at the very edge of validity (S barely positive definite) can come back invalid
 * from the posterior kernel, with NaN in rows 0-14 and ℓ = −Inf: a caller should drop such a column.
 * At most `cap` are stored (cap = 0: count only; the arrays may then be NULL); *n_accepted is the full count, *max_logml (or NULL) the maximum.
 *   theta_out [5][cap] · nl_out [5][cap] · post_out [OCTO_DRAWS_OFTI_N_OUT][cap] · index_out [cap]
 * OCTO_EINVAL: NULL handle; nothing set; N < 1, first + N overflowing; cap < 0, NULL n_accepted, a NULL array with cap > 0; with the reference's message
 * when every ℓ is −Inf. OCTO_ENOMEM: the work group (10·2^18 + N + 2⌈N/256⌉ + 2 + 29·min(cap, N) doubles) could not be allocated; the handle stays usable. */
int32_t octo_draws_ofti_rejection(octo_draws* h, uint64_t seed, uint64_t first, int64_t N, int64_t cap, double* theta_out /*[5][cap]*/,
                                  double* nl_out /*[5][cap]*/, double* post_out /*[16][cap]*/, uint64_t* index_out /*[cap]*/, int64_t* n_accepted,
                                  double* max_logml);

/* ---- The seventeenth: along-scan absolute astrometry — the Hipparcos intermediate astrometric data and Gaia's per-transit epoch astrometry: one
 * along-scan coordinate per transit, a scan direction and design columns the caller builds (parallax factors, reference epochs: the library knows
 * nothing of them). The functions are stated in full so that a restatement elsewhere (tests/scan_reference.py) and the device compute the same function.
 *
 * Table      n rows, 1 <= n <= 65536. Row i: epoch t_i [MJD], scan direction (u_i, v_i) along α* and δ, measurement y_i [mas], σ_i > 0 [mas] and
 *            K design coefficients c_i[0 … K − 1], 0 <= K <= OCTO_DRAWS_SCAN_MAX_K; c is [K][n].
 * Walker     the main ABI's element rows elems[(p·9 + k)·ld + w], the linear parameters β[k·ld + w], the jitter s[w] (NULL: 0), the planets'
 *            descriptors (1 <= n_planets <= OCTO_MAX_PLANETS) and the constants (NULL: octo_consts_default, what the program route uses).
 * Model      R_p(t) = f_p·(raoff_p(t), decoff_p(t)) [mas], f_p = −mass_p·mjup2msol/M_p (0 with has_mass = 0): the reflex rule of the HGCA term,
 *            q_star = −m_p/M_tot·q_planet. raoff and decoff are the orbit constructor and the projection of the main library on the COLD Kepler solve
 *            (the companion libraries' rule). OCTO_ORBIT_VISUAL_KEP and OCTO_ORBIT_THIELE_INNES planets contribute, the others contribute 0.
 *              η_i = Σ_k c_i[k]·β_k + Σ_p (u_i·R_p,α(t_i) + v_i·R_p,δ(t_i))      r_i = y_i − η_i      w_i = 1/(σ_i² + s²)
 *              ℓ   = Σ_i (−½·w_i·r_i² + ½·log w_i − ½·log 2π)
 * Gradient   reverse mode: ∂ℓ/∂elems [P·9][ld] through the constructor (the adjoint rules of the main library's finish), ∂ℓ/∂β_k = Σ_i w_i r_i c_i[k],
 *            ∂ℓ/∂s = s·Σ_i (w_i² r_i² − w_i).
 * Invalid    a non-finite input, an element outside the main library's domain, s < 0, a non-finite β (or ℓ): ℓ = −Inf and a zero gradient for that
 *            walker; never a status, never another walker's bits.
 * Marginal   OCTO_DRAWS_SCAN_MARGINAL: β integrated out under a flat prior. A = Σ_i w_i c_i c_iᵀ, b = Σ_i w_i c_i (y_i − reflex_i), β̂ = A⁻¹b by Cholesky
 *            per walker, ℓ_marg = ℓ(β̂) + (K/2)·log 2π − ½·log det A; ∂ℓ_marg/∂elems = the sampled adjoints at β̂;
 *            ∂ℓ_marg/∂s = s·Σ(w_i² r̂_i² − w_i) + s·Σ w_i² c_iᵀA⁻¹c_i. d_beta and d_g_beta are not used; d_beta_hat [K][ld] (or NULL) receives β̂.
 *            Two Kepler solves per (row, planet): one pass for A and b, one at β̂.
 * Order      the rows are cut into tasks of OCTO_DRAWS_SCAN_ROWS rows, whatever W is; a task adds its rows in row order by fma, the tasks are added in
 *            task order. No atomics: a walker's ℓ and gradient depend on its own column alone, bit for bit, in any batch and with any ld.
 *
 * octo_draws_scan_set copies the table to the device; it needs neither a model nor a context. A second call replaces the first;
 * octo_draws_scan_clear removes it (no-op when nothing is set). Both drop a binding. With K > 0 the table must have full column rank: CᵀΣ⁻¹C must be
 * positive definite (w_i > 0 for every s, so that is a property of the table alone), also where only the sampled mode will be used.
 * OCTO_EINVAL: NULL handle; a NULL array (c may be NULL with K = 0); n or K or n_planets out of range; σ <= 0; a non-finite entry; an unknown
 * orbit kind; CᵀΣ⁻¹C not positive definite. */
#define OCTO_DRAWS_SCAN_MAX_K 6
#define OCTO_DRAWS_SCAN_ROWS 8
#define OCTO_DRAWS_SCAN_SAMPLED 0
#define OCTO_DRAWS_SCAN_MARGINAL 1
int32_t octo_draws_scan_set(octo_draws* h, const octo_planet_desc* planets, int32_t n_planets, const octo_consts* consts /*NULL = octo_consts_default*/,
                            const double* t, const double* u, const double* v, const double* y, const double* sigma, const double* c /*[K][n]*/, int32_t K,
                            int64_t n);
int32_t octo_draws_scan_clear(octo_draws* h);

/* ℓ [W] and the gradients of W walkers on DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no allocation once the handle's work
 * array holds (⌈n/OCTO_DRAWS_SCAN_ROWS⌉·n_sums + 28)·ldw doubles, ldw = W rounded up to whole waves, n_sums = 9 + 10·n_planets (marginal: at least 27).
 * Every gradient output may be NULL; with all of them NULL no adjoint is formed. accumulate = 1 ADDS ℓ into d_ll and the element adjoints into
 * d_g_elems (an invalid walker adds −Inf and 0); d_g_beta [K][ld], d_g_jitter [W] and d_beta_hat [K][ld] are always stored. accumulate = 0 stores
 * 0 + the value, so that accumulating into zeroed outputs gives the same bits.
 * OCTO_EINVAL: NULL handle; no table; mode outside 0, 1; marginal mode with K = 0; W < 0, ld < W; NULL d_elems or d_ll, or NULL d_beta in sampled mode
 * with K > 0, with W > 0. */
int32_t octo_draws_scan_eval_device(octo_draws* h, int32_t mode, const double* d_elems, int64_t ld, int64_t W, const double* d_beta, const double* d_jitter,
                                    double* d_ll, double* d_g_elems, double* d_g_beta, double* d_g_jitter, double* d_beta_hat, int32_t accumulate,
                                    void* hip_stream);
/* The twin on HOST buffers, blocking, through the handle's staging on its own stream; accumulate = 0. */
int32_t octo_draws_scan_eval(octo_draws* h, int32_t mode, const double* elems, int64_t ld, int64_t W, const double* beta, const double* jitter, double* ll,
                             double* g_elems, double* g_beta, double* g_jitter, double* beta_hat);

/* The model values η [n][ld_out] of W walkers (d_beta NULL: the reflex part alone), asynchronous on hip_stream: for posterior-predictive residuals.
 * An invalid walker's column is not defined. OCTO_EINVAL: NULL handle; no table; W < 0, ld < W, ld_out < W; NULL d_elems or d_eta with W > 0. */
int32_t octo_draws_scan_values_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_beta, double* d_eta /*[n][ld_out]*/,
                                      int64_t ld_out, void* hip_stream);

/* The table as a term of the handle's expression program: from the next call on octo_draws_program_logpost_device — and through it every function of
 * the handle that needs ℓπ — adds ℓ_scan to the likelihood that octo_eval_device returns (it is tempered with it and survives a healed prior) and its
 * adjoints to the inputs' gradient. binds names the nodes the table reads, OCTO_DRAWS_BIND_NODE only (a constant is a CONST node): in sampled mode
 * n_binds = K + 1, the β nodes in column order and then the jitter node; in marginal mode n_binds = 1, the jitter node. The planets' elements are the
 * program's own element rows. The bound nodes become input rows behind the program's own, so with nothing bound no launch and no work array differs.
 * octo_draws_program_set, octo_draws_program_clear, octo_draws_scan_set and octo_draws_scan_clear drop the binding; octo_draws_scan_unbind is a no-op
 * when nothing is bound. A transition that was open is never resumed across a change of the binding.
 * OCTO_EINVAL: NULL handle; no table; no program, or one whose n_planets is not the table's; mode outside 0, 1; marginal mode with K = 0; n_binds not as
 * above; a binding that is not a NODE or whose node is out of range. */
int32_t octo_draws_scan_bind(octo_draws* h, int32_t mode, const octo_draws_bind* binds, int32_t n_binds);
int32_t octo_draws_scan_unbind(octo_draws* h);

/* ---- The eighteenth: the catalogue proper-motion anomaly ("pma") from refitted scans — the reference's HGCAObs: the star is simulated at every Hipparcos
 * and Gaia scan, each mission's linear model is refitted, and the fitted proper motions are compared with the catalogue under its covariance. The scan
 * geometry and the weights do not depend on the walker, so each refit is a FIXED linear map of the reflex rows, which the host folds into the projector L:
 * the library knows nothing of missions, reference epochs or parallax factors. The functions are stated in full so that a restatement elsewhere
 * (tests/pma_reference.py) and the device compute the same function. The table is held beside the scan table of the seventeenth part, independent of it.
 *
 * Table      n rows, 1 <= n <= 65536. Row i: epoch t_i [MJD] and scan direction (u_i, v_i) along α* and δ. A projector L [Q][n], 1 <= Q <=
 *            OCTO_DRAWS_PMA_MAX_Q; catalogue values d [Q]; a symmetric positive-definite covariance Σ [Q][Q]; a constant design H [Q][K] for K linear
 *            walker parameters γ, 0 <= K <= OCTO_DRAWS_PMA_MAX_K (H may be NULL with K = 0); the planets' descriptors and the constants, as for
 *            octo_draws_scan_set. Everything is in the units of L's rows: mas/yr for the HGCA.
 * Model      ρ_i = Σ_p f_p·(u_i·raoff_p(t_i) + v_i·decoff_p(t_i)), f_p = −mass_p·mjup2msol/M_p: the scan part's reflex rule, word for word —
 *            OCTO_ORBIT_VISUAL_KEP and OCTO_ORBIT_THIELE_INNES planets with a mass contribute, the others contribute 0; the companions' COLD Kepler solve
 *            and the main library's constructor and projection.   z_q = Σ_i L[q][i]·ρ_i      m = z + H·γ      r = d − m
 * Sampled    OCTO_DRAWS_PMA_SAMPLED: ℓ = −½·rᵀΣ⁻¹r − ½·log det(2πΣ). Reverse mode: λ = Σ⁻¹r, ∂ℓ/∂γ = Hᵀλ, the adjoint of ρ_i is g_i = Σ_q L[q][i]·λ_q,
 *            and from g_i each planet's ten sums go through the main library's finish to ∂ℓ/∂elems [P·9][ld].
 * Marginal   OCTO_DRAWS_PMA_MARGINAL: γ integrated out under a flat prior; needs K > 0 and N = HᵀΣ⁻¹H positive definite. P_m = Σ⁻¹ − Σ⁻¹H·N⁻¹·HᵀΣ⁻¹,
 *            r = d − z, ℓ_marg = −½·rᵀP_m r − ½·log det(2πΣ) + (K/2)·log 2π − ½·log det N, λ = P_m r; γ̂ = N⁻¹HᵀΣ⁻¹r [K][ld] is an output.
 * Matrices   Σ⁻¹, P_m, N⁻¹HᵀΣ⁻¹ and both constants are made once, on the host, in octo_draws_pma_set by Cholesky factors (csrc/draws/
 *            octo_draws_pma_host.h; a pivot must exceed 1e-12 of its diagonal entry); the device only applies Q × Q and K × Q matrices. There is no jitter:
 *            a fit with inflated errors passes an inflated Σ.
 * Invalid    a non-finite input, an element outside the main library's domain, a non-finite γ (or ℓ): ℓ = −Inf and a zero gradient for that walker;
 *            never a status, never another walker's bits. γ̂ of an invalid walker is not defined.
 * Order      the rows are cut into tasks of OCTO_DRAWS_SCAN_ROWS rows, whatever W is; a task adds its planets into ρ_i in planet order and its rows
 *            into z_q in row order by fma, the tasks are added in task order, the q and k sums run in index order. No atomics: a walker's outputs depend on
 *            its own column alone, bit for bit, in any batch and with any ld.
 *
 * octo_draws_pma_set copies the table to the device; it needs neither a model nor a context. A second call replaces the first; octo_draws_pma_clear
 * removes it (no-op when nothing is set). Both drop a binding. A rank-deficient H is not refused here: that is the marginal mode's condition, answered at
 * eval and bind.
 * OCTO_EINVAL: NULL handle; a NULL array (H may be NULL with K = 0); n, Q, K or n_planets out of range; a non-finite entry; an unknown orbit kind; Σ not
 * symmetric (beyond 1e-12·√(Σ_ii Σ_jj)) or not positive definite. */
#define OCTO_DRAWS_PMA_MAX_Q 8
#define OCTO_DRAWS_PMA_MAX_K 4
#define OCTO_DRAWS_PMA_SAMPLED 0
#define OCTO_DRAWS_PMA_MARGINAL 1
int32_t octo_draws_pma_set(octo_draws* h, const octo_planet_desc* planets, int32_t n_planets, const octo_consts* consts /*NULL = octo_consts_default*/,
                           const double* t, const double* u, const double* v, const double* L /*[Q][n]*/, int32_t Q, const double* d /*[Q]*/,
                           const double* cov /*[Q][Q]*/, const double* H /*[Q][K]*/, int32_t K, int64_t n);
int32_t octo_draws_pma_clear(octo_draws* h);

/* ℓ [W] and the gradients of W walkers on DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no allocation once the handle's work
 * array holds (⌈n/OCTO_DRAWS_SCAN_ROWS⌉·n_sums + 9)·ldw doubles, ldw = W rounded up to whole waves, n_sums = max(8, 10·n_planets). d_gamma, d_g_gamma and
 * d_gamma_hat are [K][ld]. Every gradient output may be NULL; with d_g_elems NULL only the two forward kernels run (∂ℓ/∂γ and γ̂ come from them).
 * accumulate = 1 ADDS ℓ into d_ll and the element adjoints into d_g_elems (an invalid walker adds −Inf and 0); d_g_gamma and d_gamma_hat are always
 * stored. accumulate = 0 stores 0 + the value, so that accumulating into zeroed outputs gives the same bits.
 * OCTO_EINVAL: NULL handle; no table; mode outside 0, 1; marginal mode with K = 0 or with HᵀΣ⁻¹H not positive definite; W < 0, ld < W; NULL d_elems or
 * d_ll, or NULL d_gamma in sampled mode with K > 0, with W > 0. */
int32_t octo_draws_pma_eval_device(octo_draws* h, int32_t mode, const double* d_elems, int64_t ld, int64_t W, const double* d_gamma, double* d_ll,
                                   double* d_g_elems, double* d_g_gamma, double* d_gamma_hat, int32_t accumulate, void* hip_stream);
/* The twin on HOST buffers, blocking, through the handle's staging ((2·P·9 + 3·K + 1)·ld doubles) on its own stream; accumulate = 0. */
int32_t octo_draws_pma_eval(octo_draws* h, int32_t mode, const double* elems, int64_t ld, int64_t W, const double* gamma, double* ll, double* g_elems,
                            double* g_gamma, double* gamma_hat);

/* The model's catalogue values m = z + H·γ [Q][ld_out] of W walkers (d_gamma NULL: z alone), asynchronous on hip_stream: for posterior-predictive checks
 * against the catalogue. An invalid walker's column is not defined. OCTO_EINVAL: NULL handle; no table; W < 0, ld < W, ld_out < W; NULL d_elems or d_m
 * with W > 0. */
int32_t octo_draws_pma_values_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_gamma, double* d_m /*[Q][ld_out]*/,
                                     int64_t ld_out, void* hip_stream);

/* The table as a term of the handle's expression program, exactly as octo_draws_scan_bind: ℓ_pma is added to the likelihood that octo_eval_device returns
 * (it is tempered with it and survives a healed prior) and its adjoints to the inputs' gradient. binds names the γ nodes in column order,
 * OCTO_DRAWS_BIND_NODE only: n_binds = K in sampled mode, 0 in marginal mode (binds may then be NULL). The bound nodes become input rows behind the
 * program's own, so with nothing bound no launch and no work array differs. octo_draws_program_set, octo_draws_program_clear, octo_draws_pma_set and
 * octo_draws_pma_clear drop the binding; octo_draws_pma_unbind is a no-op when nothing is bound. A transition that was open is never resumed across a
 * change of the binding. ONE bound table a handle: with a scan table bound octo_draws_pma_bind answers OCTO_ENOTSUP, and so does octo_draws_scan_bind
 * with a catalogue table bound.
 * OCTO_EINVAL: NULL handle; no table; no program, or one whose n_planets is not the table's; mode outside 0, 1; marginal mode with K = 0 or a rank-
 * deficient H; n_binds not as above; a binding that is not a NODE or whose node is out of range. */
int32_t octo_draws_pma_bind(octo_draws* h, int32_t mode, const octo_draws_bind* binds, int32_t n_binds);
int32_t octo_draws_pma_unbind(octo_draws* h);

/* ---- The nineteenth: a radial-velocity table of the star under a Gaussian process with celerite kernels — the reference's StarAbsoluteRVObs with a
 * gaussian_process that returns a Celerite kernel: log N(r; 0, K) of the residuals by the semiseparable recursion, O(n·R²) a walker, and its exact
 * gradient in reverse mode. The functions are stated in full so that a restatement elsewhere (tests/gp_reference.py: the DENSE normal in mpmath, and the
 * recursion in NumPy) and the device compute the same function. The table is held beside the scan and catalogue tables, independent of them.
 *
 * Table      n rows, 1 <= n <= 65536. Row i: epoch t_i [MJD], non-decreasing; rv_i [m/s]; σ_i > 0 [m/s]; K design coefficients c_i[0 … K − 1],
 *            0 <= K <= OCTO_DRAWS_GP_MAX_K (the offset's column of ones, the trend basis); c is [K][n]. The planets' descriptors and the constants as
 *            for octo_draws_scan_set. A term list of 1 <= J <= OCTO_DRAWS_GP_MAX_TERMS kinds.
 * Terms      a term occupies slots, R = Σ slots <= OCTO_DRAWS_GP_MAX_SLOTS, and reads hyperparameters hyper[h·ld + w], H = Σ (2 | 4 | 3) rows in term
 *            order. With x = d·(t_i − t_1) (the origin is row 1: any origin is exact for a stationary kernel, this one keeps the phases small):
 *              OCTO_DRAWS_GP_REAL     1 slot   (a, c)         k(τ) = a·e^{−cτ}                          Ũ = a, Ṽ = 1, rate c
 *              OCTO_DRAWS_GP_COMPLEX  2 slots  (a, b, c, d)   k(τ) = e^{−cτ}(a·cos dτ + b·sin dτ)       Ũ = (a cos x + b sin x, a sin x − b cos x),
 *                                                                                                       Ṽ = (cos x, sin x), rate c on both
 *              OCTO_DRAWS_GP_SHO      2 slots  (S0, Q, ω0)    decided PER WALKER: Q > ½ is a COMPLEX with f = √(4Q² − 1), a = S0·ω0·Q, b = a/f,
 *                                                             c = ω0/(2Q), d = c·f; Q < ½ is two REAL slots with f = √(1 − 4Q²),
 *                                                             a± = ½·S0·ω0·Q·(1 ± 1/f), c± = ω0/(2Q)·(1 ∓ f); at Q = ½ the coefficients are not
 *                                                             finite and the walker is invalid. Lanes of one wave may sit on both sides of ½.
 * Model      η_i = Σ_k c_i[k]·β_k + Σ_p f_p·K_p·V_p(t_i), f_p = −mass_p·mjup2msol/M_p (0 with has_mass = 0), K_p the semi-amplitude and V_p =
 *            cos(ν + ω) + e·cos ω: the main library's absolute-RV rule, rv_row's arithmetic on the COLD Kepler solve (the companion libraries' rule).
 *            OCTO_ORBIT_VISUAL_KEP, OCTO_ORBIT_RADVEL and OCTO_ORBIT_KEP planets with a mass contribute. r_i = rv_i − η_i, A_i = σ_i² + s² + Σ_j a_j
 *            (a complex pair adds its a once, an SHO below ½ adds a₊ + a₋).
 * Recursion  φ_i = e^{−c·(t_i − t_{i−1})} per slot, S_1 = 0, f_1 = 0, and in row order
 *              S_i = φ_iφ_iᵀ ∘ (S_{i−1} + D_{i−1}W_{i−1}W_{i−1}ᵀ)      f_i = φ_i ∘ (f_{i−1} + W_{i−1}z_{i−1})
 *              D_i = A_i − Ũ_iᵀS_iŨ_i      W_i = (Ṽ_i − S_iŨ_i)/D_i      z_i = r_i − Ũ_i·f_i
 *              ℓ   = Σ_i (−½·z_i²/D_i − ½·log D_i − ½·log 2π)   = log N(r; 0, K), K_ij = [i = j](σ_i² + s²) + Σ_j k_j(|t_i − t_j|)
 * Gradient   the exact derivative of ℓ in reverse mode: α = K⁻¹r is the adjoint of −r, so ∂ℓ/∂η_i = α_i; ∂ℓ/∂elems [P·9][ld] from α through each
 *            planet's sums and the main library's finish; ∂ℓ/∂β_k = Σ_i α_i c_i[k]; ∂ℓ/∂s; ∂ℓ/∂hyper [H][ld] in the terms' OWN parameters (S0, Q, ω0
 *            of an SHO). The reverse walk never divides by φ (a seasonal gap has φ down to exactly 0): the state a row hands to the next,
 *            (S + D·W·Wᵀ, f + W·z), is kept every OCTO_DRAWS_GP_SEGMENT rows by the forward pass, and the reverse pass recomputes a segment's states
 *            forward from its checkpoint before it walks the segment backward.
 * Invalid    a non-finite input, an element outside the main library's domain, s < 0, a rate c <= 0, a non-finite coefficient, a D_i that is not
 *            > 0 and finite (the kernel is not positive definite there), a non-finite ℓ: ℓ = −Inf and a zero gradient for that walker; never a
 *            status, never another walker's bits.
 * Order      the row-parallel passes (η, and the planets' and β's sums against α) cut the rows into tasks of OCTO_DRAWS_SCAN_ROWS and add in row
 *            order, then task order; the recursion is in row order by construction. No atomics: a walker's outputs depend on its own column alone,
 *            bit for bit, in any batch and with any ld. There is no marginal mode: the reference's marginalised RV has no Gaussian process.
 *
 * octo_draws_gp_set copies the table to the device; it needs neither a model nor a context. A second call replaces the first; octo_draws_gp_clear
 * removes it (no-op when nothing is set). Both drop a binding.
 * OCTO_EINVAL: NULL handle; a NULL array (c may be NULL with K = 0); n, K, n_planets or n_terms out of range; σ <= 0; a non-finite entry; epochs that
 * decrease; an unknown orbit kind or term kind. OCTO_ENOTSUP: an OCTO_ORBIT_THIELE_INNES planet with a mass (as the main library answers an RV table
 * on such a planet). */
#define OCTO_DRAWS_GP_MAX_K 4
#define OCTO_DRAWS_GP_MAX_TERMS 4
#define OCTO_DRAWS_GP_MAX_SLOTS 8
#define OCTO_DRAWS_GP_SEGMENT 16
#define OCTO_DRAWS_GP_REAL 0
#define OCTO_DRAWS_GP_COMPLEX 1
#define OCTO_DRAWS_GP_SHO 2
int32_t octo_draws_gp_set(octo_draws* h, const octo_planet_desc* planets, int32_t n_planets, const octo_consts* consts /*NULL = octo_consts_default*/,
                          const double* t, const double* rv, const double* sigma, const double* c /*[K][n]*/, int32_t K, int64_t n,
                          const int32_t* term_kinds, int32_t n_terms);
int32_t octo_draws_gp_clear(octo_draws* h);

/* The doubles of the handle's work array that one evaluation of W walkers needs (−1: an argument out of range):
 *   ldw·(n + 1 + [grad]·((⌈n/OCTO_DRAWS_GP_SEGMENT⌉ + OCTO_DRAWS_GP_SEGMENT)·(R'(R' + 1)/2 + R') + ⌈n/OCTO_DRAWS_SCAN_ROWS⌉·(4 + 6·n_planets)))
 * ldw = W rounded up to whole waves, R' = n_slots rounded up to 2, 4 or 8 (the kernels' instantiations; a padding slot changes no bit). The residuals
 * (then α) and the validity; with a gradient the checkpoints, one segment's states, and the row tasks' sums. */
int64_t octo_draws_gp_work_doubles(int64_t n, int32_t n_slots, int32_t n_planets, int64_t W, int32_t grad);

/* ℓ [W] and the gradients of W walkers on DEVICE buffers, asynchronous on hip_stream: no host synchronisation, no allocation once the handle's work
 * array holds octo_draws_gp_work_doubles. d_hyper and d_g_hyper are [H][ld], d_beta and d_g_beta [K][ld], d_jitter (NULL: 0) and d_g_jitter [W]. Every
 * gradient output may be NULL; with all of them NULL no reverse pass runs and nothing is stored for one, and ℓ has the gradient call's bits.
 * accumulate = 1 ADDS ℓ into d_ll and the element adjoints into d_g_elems (an invalid walker adds −Inf and 0); the other gradients are always stored.
 * accumulate = 0 stores 0 + the value, so that accumulating into zeroed outputs gives the same bits.
 * OCTO_EINVAL: NULL handle; no table; W < 0, ld < W; NULL d_elems, d_hyper or d_ll, or NULL d_beta with K > 0, with W > 0. */
int32_t octo_draws_gp_eval_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_hyper, const double* d_beta,
                                  const double* d_jitter, double* d_ll, double* d_g_elems, double* d_g_hyper, double* d_g_beta, double* d_g_jitter,
                                  int32_t accumulate, void* hip_stream);
/* The twin on HOST buffers, blocking, through the handle's staging ((2·P·9 + 2·H + 2·K + 3)·ld doubles) on its own stream; accumulate = 0. */
int32_t octo_draws_gp_eval(octo_draws* h, const double* elems, int64_t ld, int64_t W, const double* hyper, const double* beta, const double* jitter,
                           double* ll, double* g_elems, double* g_hyper, double* g_beta, double* g_jitter);

/* The model values η [n][ld_out] of W walkers (d_beta NULL: the planets alone) and, with d_mu, the process's conditional mean at the table's epochs,
 * μ_i = r_i − (σ_i² + s²)·α_i [n][ld_out] (residual plots subtract it); d_eta or d_mu may be NULL, d_hyper and d_jitter are read for d_mu alone.
 * Asynchronous on hip_stream. An invalid walker's column is not defined. OCTO_EINVAL: NULL handle; no table; W < 0, ld < W, ld_out < W; NULL d_elems,
 * both outputs NULL, or d_mu without d_hyper, with W > 0. */
int32_t octo_draws_gp_values_device(octo_draws* h, const double* d_elems, int64_t ld, int64_t W, const double* d_hyper, const double* d_beta,
                                    const double* d_jitter, double* d_eta /*[n][ld_out]*/, double* d_mu /*[n][ld_out]*/, int64_t ld_out, void* hip_stream);

/* The table as a term of the handle's expression program, exactly as octo_draws_scan_bind: ℓ_gp is added to the likelihood that octo_eval_device
 * returns (it is tempered with it and survives a healed prior) and its adjoints to the inputs' gradient. binds names the nodes the table reads,
 * OCTO_DRAWS_BIND_NODE only: n_binds = H + K + 1, the hyperparameter nodes in term order, the β nodes in column order, then the jitter node. The bound
 * nodes become input rows behind the program's own, so with nothing bound no launch and no work array differs. octo_draws_program_set,
 * octo_draws_program_clear, octo_draws_gp_set and octo_draws_gp_clear drop the binding; octo_draws_gp_unbind is a no-op when nothing is bound. A
 * transition that was open is never resumed across a change of the binding. ONE bound table a handle: with a scan or catalogue table bound
 * octo_draws_gp_bind answers OCTO_ENOTSUP, and so do octo_draws_scan_bind and octo_draws_pma_bind with this table bound.
 * OCTO_EINVAL: NULL handle; no table; no program, or one whose n_planets is not the table's; n_binds not as above; a binding that is not a NODE or
 * whose node is out of range. */
int32_t octo_draws_gp_bind(octo_draws* h, const octo_draws_bind* binds, int32_t n_binds);
int32_t octo_draws_gp_unbind(octo_draws* h);

/* ---- The twentieth: the same table under DENSE kernels — the reference's StarAbsoluteRVObs with a gaussian_process that returns an AbstractGPs /
 * KernelFunctions kernel, the quasi-periodic one of its RV tutorial first. No semiseparable form exists, so ℓ = log N(r; 0, K) comes from a dense
 * Cholesky factor, O(n³) a walker, one workgroup a walker (csrc/draws/octo_draws_gpd.hip). No new entry point but the work formula: octo_draws_gp_set,
 * _clear, _eval_device, _eval, _values_device, _bind and _unbind take a dense term list as they take a celerite one. The table, the model η, r, β, the
 * planets' rule, accumulate and the binding (n_binds = H + K + 1, the hyperparameter nodes in term order) are the nineteenth part's, word for word.
 *
 * Terms      kinds from 16 up; a list holds 1 <= J <= OCTO_DRAWS_GP_MAX_TERMS of them (H <= 16) and is EITHER celerite (kinds 0 … 2) OR dense: a mixed
 *            list is OCTO_EINVAL, and so is every other kind (3 … 15, 21 …). A celerite list takes the nineteenth part's kernels and keeps its bits.
 *            With τ = |t_i − t_j| and the hyper rows in the order given:
 *              OCTO_DRAWS_GP_SE             (a, ℓ)         k(τ) = a²·exp(−τ²/(2ℓ²))
 *              OCTO_DRAWS_GP_MATERN32       (a, ℓ)         k(τ) = a²·(1 + u)·e^{−u},           u = √3·τ/ℓ
 *              OCTO_DRAWS_GP_MATERN52       (a, ℓ)         k(τ) = a²·(1 + u + u²/3)·e^{−u},    u = √5·τ/ℓ
 *              OCTO_DRAWS_GP_PERIODIC       (a, P, r)      k(τ) = a²·exp(−sin²(πτ/P)/(2r²))
 *              OCTO_DRAWS_GP_QUASIPERIODIC  (a, ℓ, P, r)   k(τ) = a²·exp(−τ²/(2ℓ²) − sin²(πτ/P)/(2r²))
 *            These are KernelFunctions.jl's SqExponentialKernel, Matern32Kernel, Matern52Kernel and PeriodicKernel(r = [r]) under ScaleTransform(1/ℓ)
 *            and ScaleTransform(1/P), scaled by a²; the quasi-periodic one is the tutorial's η₁²·SqExponential(τ/η₂)·Periodic(τ/η₃; r = η₄). The formulas
 *            are recalled, not pinned against the running reference.
 * Function   K_ij = [i = j]·(σ_i² + s²) + Σ_terms k(|t_i − t_j|), K = L·Lᵀ, y = L⁻¹r, ℓ = −½·yᵀy − Σ_j log L_jj − (n/2)·log 2π, α = L⁻ᵀy = K⁻¹r.
 * Gradient   ∂ℓ/∂η_i = α_i, through the nineteenth part's passes to elements and β. ∂ℓ/∂h = ½·Σ_ij (α_iα_j − K⁻¹_ij)·∂K_ij/∂h with the closed forms
 *              ∂k/∂a = 2k/a (written 2a·…, so a = 0 is no division)    ∂k/∂ℓ = k·τ²/ℓ³ (SE, QP) · a²·u²·e^{−u}/ℓ (M32) · a²·u²(1 + u)·e^{−u}/(3ℓ) (M52)
 *              ∂k/∂P = k·sin(πτ/P)·cos(πτ/P)·πτ/(P²r²)                  ∂k/∂r = k·sin²(πτ/P)/r³
 *            and ∂ℓ/∂s = s·(Σ α_i² − tr K⁻¹). K⁻¹ is formed in place of L (the inverse of L, then its product with its transpose); no finite difference.
 * Invalid    what the nineteenth part calls invalid in elements, β and s; a non-finite hyperparameter; ℓ, P or r <= 0; a non-finite a²; a pivot K_jj −
 *            Σ L_jm² that is not > 0 and finite: ℓ = −Inf and a zero gradient for that walker; never a status, never another walker's bits.
 * Order      right-looking: column j is scaled, then the trailing triangle takes its rank-1 update, so every element receives its updates in column
 *            order whatever thread makes them; y is the factorisation's row n. Every dot product of the inverse is one thread's, in index order; the
 *            contraction gives each thread a fixed set of pairs and adds the threads' partials by a fixed tree (in a wave, then the four waves in wave
 *            order). No atomics: a walker's bits depend on its own column alone, in any batch, with any ld, at any block index.
 * Sizes      a table of n <= OCTO_DRAWS_GP_DENSE_LDS_ROWS rows keeps the packed lower triangle, n(n + 1)/2 doubles, and four vectors of n in the
 *            workgroup's LDS (8·(n(n + 1)/2 + 4n + 128) bytes: 155 392 at 192 rows, of the 163 840 a workgroup of this device may hold; octo_draws_gp_set
 *            answers OCTO_ENOTSUP on a device that gives less). A longer one, up to OCTO_DRAWS_GP_DENSE_MAX_N rows, runs the same kernel bodies on
 *            triangles in the work array: a functional fallback, O(n³) traffic through L2 / HBM, unblocked. More rows: OCTO_EINVAL. */
#define OCTO_DRAWS_GP_SE 16
#define OCTO_DRAWS_GP_MATERN32 17
#define OCTO_DRAWS_GP_MATERN52 18
#define OCTO_DRAWS_GP_PERIODIC 19
#define OCTO_DRAWS_GP_QUASIPERIODIC 20
#define OCTO_DRAWS_GP_DENSE_LDS_ROWS 192
#define OCTO_DRAWS_GP_DENSE_MAX_N 2048
/* The doubles of the handle's work array that one evaluation of W walkers of a dense table needs (−1: an argument out of range; n > DENSE_MAX_N too):
 *   ldw·(n + 1 + [grad]·⌈n/OCTO_DRAWS_SCAN_ROWS⌉·(4 + 6·n_planets)) + [n > OCTO_DRAWS_GP_DENSE_LDS_ROWS]·W·n(n + 1)/2
 * ldw = W rounded up to whole waves. The residuals (then α) and the validity; with a gradient the row tasks' sums; the triangles of a long table. */
int64_t octo_draws_gp_dense_work_doubles(int64_t n, int32_t n_planets, int64_t W, int32_t grad);

#ifdef __cplusplus
}
#endif
#endif /* OCTOFITTER_HIP_DRAWS_H */
