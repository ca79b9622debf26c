"""
ctypes binding of the companion C ABI in include/octofitter_hip_draws.h (lib/liboctofitter_hip_draws.so) and its host face.

    draws = PriorDraws(model)                       # model: LogDensityModel
    θ, θ_t, logprior_t = draws.sample(seed, first, n)       # torch tensors on the model's device: [D, n], [D, n], [n]
    θ, logpost, index = draws.best(seed, N, keep=8)         # NumPy: [D, keep], [keep], [keep]
    chain = draws.rejection(seed, N)                        # dict: samples [D, n_accepted], loglike, logpost, index, …
    p = draws.momentum(seed, step, n)                       # torch [D, n]: the momenta of chains 0 … n − 1 at `step`
    lp, ll, dH, acc = draws.hmc_step(θ_t, beta, eps=0.1, n_leapfrog=4, seed=seed, step=step)      # one tempered HMC step, θ_t updated in place
    r = draws.lbfgs(θ_t, inv_mass=v, n_rounds=50)           # 50 rounds of L-BFGS on every column, θ_t updated in place: dict of device tensors
    r = draws.pathfinder(θ_t, inv_mass=v, n_rounds=50, seed=seed)      # the same rounds with Pathfinder's fits along the path: also elbo, elbo_iter, n_fits
    φ, logq, logpost = draws.pathfinder_draw(θ_t, 256, seed=seed)      # [D, 256·W], [256·W], [256·W]: draws from every chain's kept fit
    lp, ll, log_accept, acc, depth, n_leapfrog, diverged = draws.nuts_step(θ_t, eps=0.1, max_depth=10, seed=seed, step=step)      # one NUTS transition
    r = draws.slice_step(θ_t, beta, w=10.0, p=3, n_passes=3, seed=seed, step=step)      # one slice-sampling transition (no gradient, no ε, no metric): dict
    u = draws.cube(seed, first, n); θ, θ_t, lpt = draws.from_cube(u)      # the unit cube behind `sample` and the hypercube transform out of it: the same bytes
    r = draws.nested_step(u_live, ll_live, state, B, seed=seed, iter=it)  # one iteration of nested sampling: cull the B lowest, move their slots (dict)
    count, mean, m2 = draws.moments(θ_t)                    # warm-up: pooled moments of the chains, [1], [1, D], [1, D] (or per group)
    draws.metric(count[0:1], mean[0], m2[0], inv_mass)      # … the diagonal metric they give, written into inv_mass [D]
    state = draws.adapt_init(1, 0.1)                        # … dual averaging of ε: the state [G, 4]
    a, eps_w = draws.adapt_step(state, dH, acc, k)          # … update k from a step's dH and accepted: mean acceptance [G], ε per chain [W]
    draws.chain_moments(θ_t, k, cmean, cm2)                 # per-chain running mean and M2 over time (R̂: include/octofitter_hip_draws.h)
    d = draws.diagnose(rec)                                 # stored draws [n, K, W]: dict of [K] tensors, rhat (rank-normalised split-R̂), ess_bulk, ess_tail, …
    r, z = draws.ranks(rec)                                 # … the rank step alone: average ranks and normal scores, of rec's shape
    state = draws.pt_state(T, Cn)                           # parallel tempering between the scans: the zeroed state (acc, leg, restarts)
    draws.pt_stats(ll, slot2rep, beta, state)               # … a scan's swap probabilities, stepping-stone sums and tempered restarts, accumulated
    lp, g = draws.program_logpost(θ_t)                      # a model with Derived variables: ℓπ and ∇ℓπ through its expression program
    v = draws.program_values(θ_t, nodes)                    # … the values of chosen nodes [n, W]: the derived columns of a chain
    r = draws.pt_schedule(state, beta)                      # … a round's rejection rates, barrier Λ, log evidence and the re-placed ladder: dict
    ref = draws.reference_table()                           # a variational tempering leg: the reference table, an empty device buffer
    bad = draws.reference_fit(ref, count[0:1], mean[0], m2[0])      # … a mean-field normal on θ_t from one group's moments (reference_set: from μ, σ)
    with draws.reference(ref): ...                          # … every call inside reads the table in place of the handle's priors
    draws.reference_exchange(s2r_a, θ_a, lp_a, ll_a, None, s2r_b, θ_b, lp_b, ll_b, ref)      # … the two legs' target replicas trade places
    count, mean, m2 = draws.cov(θ_t)                        # the dense metric: pooled co-moments of the chains, [1], [D], [D(D+1)/2] packed by rows
    chol, info = draws.metric_dense(count, m2, chol)        # … their regularised Cholesky factor L (M⁻¹ = L·Lᵀ), written only where it exists (info = 0)
    y = draws.metric_apply(chol, x, transpose=False)        # … L·x or Lᵀ·x of the columns of x [D, n]
    with draws.use_metric(chol): ...                        # … hmc_step and nuts inside run under L·Lᵀ and take no inv_mass (pack_lower, unpack_lower)
    r = draws.de_step(θ_t, lo, hi, radius=8, n_gen=200, seed=seed)      # differential evolution: 200 generations of the population θ_t, updated in place (dict)
    pd = PriorDraws(priors=[e, a, τ, M, plx]); pd.ofti_set(epochs, ra, dec, σ_ra, σ_dec, cor, σ_ABFG, tp_mode=1, t_ref=50000.0)
    r = pd.ofti_rejection(seed, 1_000_000)                  # OFTI: prior draws -> accepted orbits, dict(theta, nl, post [16, n], index, n_accepted, max_logml)

Draw i of a seed is a pure function of (seed, i): Philox4x64-10 with key (seed, "octodraw") and counter (i, d // 4, purpose, 0)
— the same number whatever call, batch or chunk produces it. Like capi.py this is plumbing that FAILS LOUDLY when the library
has not been built: the draws have no NumPy fallback here (host/callers.py keeps the host-side twins of both drivers).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import numpy as np

from . import capi, companion

DRAWS_LIB_PATH = capi.PKG_DIR / "lib" / "liboctofitter_hip_draws.so"
MAX_KEEP = 64                      # OCTO_DRAWS_MAX_KEEP
PHILOX_KEY1 = 0x6F63746F64726177   # second key word; the first is the seed
PURPOSE_PRIOR, PURPOSE_UNIFORM, PURPOSE_MOMENTUM, PURPOSE_ACCEPT, PURPOSE_ELBO, PURPOSE_PATHFINDER = 0, 1, 2, 3, 4, 5
PURPOSE_NUTS_DIRECTION, PURPOSE_NUTS_LEAF, PURPOSE_NUTS_MERGE = 6, 7, 8
NUTS_MAX_DEPTH = 10                # OCTO_DRAWS_NUTS_MAX_DEPTH
PURPOSE_SLICE = 9
SLICE_MAX_DOUBLINGS, SLICE_MAX_SHRINK, SLICE_MAX_PASSES = 8, 64, 1024      # OCTO_DRAWS_SLICE_MAX_*
SLICE_ACTIVE, SLICE_DONE, SLICE_DEAD = 0, 1, 2                            # OCTO_DRAWS_SLICE_*
SLICE_OUTPUTS = ("logpost", "loglike", "n_eval", "n_expand", "n_shrink", "n_stuck", "status", "n_active")      # the outputs of octo_draws_slice_device, in order
PURPOSE_NESTED_SEED, PURPOSE_NESTED_MOVE = 10, 11
NESTED_MAX_LIVE, NESTED_MAX_STEPS, NESTED_MAX_SHRINK, NESTED_MAX_PASSES = 4096, 64, 64, 1024      # OCTO_DRAWS_NESTED_MAX_*
NESTED_ACTIVE, NESTED_DONE = 0, 1                                                                  # OCTO_DRAWS_NESTED_*
NESTED_STATE = ("logz", "logvol", "floor", "loglike_max", "remaining", "n_dead")                   # the entries of d_state [8], in order (two reserved)
NESTED_MOVE_OUTPUTS = ("theta_t", "n_eval", "n_step", "n_shrink", "n_stuck", "status", "n_active")      # the outputs of octo_draws_nested_move_device, in order
LBFGS_MAX_M = 8                    # OCTO_DRAWS_LBFGS_MAX_M
LBFGS_ACTIVE, LBFGS_GTOL, LBFGS_FTOL, LBFGS_LINESEARCH, LBFGS_DEAD = 0, 1, 2, 3, 4      # OCTO_DRAWS_LBFGS_*
PF_MAX_D = 64                      # OCTO_DRAWS_PF_MAX_D
PF_MAX_ELBO_DRAWS = 32             # OCTO_DRAWS_PF_MAX_ELBO_DRAWS
MAX_GROUPS = 64                    # OCTO_DRAWS_MAX_GROUPS
DENSE_MAX_D = 64                   # OCTO_DRAWS_DENSE_MAX_D
PURPOSE_DE = 12
DE_TAU_F, DE_F_LOW, DE_F_SPAN, DE_TAU_CR, DE_F0, DE_CR0 = 0.1, 0.1, 0.9, 0.1, 0.5, 0.9      # OCTO_DRAWS_DE_*
DE_OUTPUTS = ("fcr", "logpost", "loglike", "n_accept", "best", "best_logpost", "n_improved")      # the outputs of octo_draws_de_device, in order
PURPOSE_OFTI = 13
OFTI_N_OUT = 16                    # OCTO_DRAWS_OFTI_N_OUT
SCAN_MAX_K = 6                     # OCTO_DRAWS_SCAN_MAX_K
SCAN_ROWS = 8                      # OCTO_DRAWS_SCAN_ROWS: the rows of a task
SCAN_SAMPLED, SCAN_MARGINAL = 0, 1
SCAN_MODES = {"sampled": SCAN_SAMPLED, "marginal": SCAN_MARGINAL}
PMA_MAX_Q = 8                      # OCTO_DRAWS_PMA_MAX_Q: catalogue values of a table
PMA_MAX_K = 4                      # OCTO_DRAWS_PMA_MAX_K: its linear parameters γ
PMA_SAMPLED, PMA_MARGINAL = 0, 1
PMA_MODES = {"sampled": PMA_SAMPLED, "marginal": PMA_MARGINAL}
GP_MAX_K = 4                       # OCTO_DRAWS_GP_MAX_K: design columns of a Gaussian-process RV table
GP_MAX_TERMS = 4                   # OCTO_DRAWS_GP_MAX_TERMS: celerite terms of its kernel
GP_MAX_SLOTS = 8                   # OCTO_DRAWS_GP_MAX_SLOTS: their slots (REAL 1, COMPLEX 2, SHO 2)
GP_SEGMENT = 16                    # OCTO_DRAWS_GP_SEGMENT: rows between two checkpoints of the recursion
GP_REAL, GP_COMPLEX, GP_SHO = 0, 1, 2
GP_N_HYPER = {GP_REAL: 2, GP_COMPLEX: 4, GP_SHO: 3}
GP_N_SLOTS = {GP_REAL: 1, GP_COMPLEX: 2, GP_SHO: 2}
# the dense kinds (include/octofitter_hip_draws.h, "The twentieth"): a term list is celerite kinds alone or dense kinds alone
GP_SE, GP_MATERN32, GP_MATERN52, GP_PERIODIC, GP_QUASIPERIODIC = 16, 17, 18, 19, 20
GP_DENSE_N_HYPER = {GP_SE: 2, GP_MATERN32: 2, GP_MATERN52: 2, GP_PERIODIC: 3, GP_QUASIPERIODIC: 4}      # (a, ℓ) · (a, ℓ) · (a, ℓ) · (a, P, r) · (a, ℓ, P, r)
GP_DENSE_LDS_ROWS = 192            # OCTO_DRAWS_GP_DENSE_LDS_ROWS: the longest dense table whose triangle a workgroup keeps in LDS
GP_DENSE_MAX_N = 2048              # OCTO_DRAWS_GP_DENSE_MAX_N
OFTI_OUTPUTS = ("A", "B", "F", "G", "A_mean", "B_mean", "F_mean", "G_mean", "alpha", "a_ti", "i", "ω", "Ω", "P_d", "M_dyn", "logml")      # the rows of d_out, in order
DIAG_RHAT, DIAG_ESS_BULK, DIAG_ESS_TAIL, DIAG_RHAT_BASIC, DIAG_ESS_BASIC, DIAG_Q05, DIAG_Q50, DIAG_Q95, DIAG_N_STATS = range(9)      # OCTO_DRAWS_DIAG_*
PT_ACC_COLUMNS = ("n", "A", "n_f", "m_f", "s_f", "n_b", "m_b", "s_b")      # the columns of d_acc [T − 1][8]
PT_SUMMARY = ("barrier", "log_evidence_fwd", "log_evidence_rev", "log_evidence")      # the entries of d_summary, in order
DIAG_NAMES = ("rhat", "ess_bulk", "ess_tail", "rhat_basic", "ess_basic", "q05", "q50", "q95")      # the rows of d_out, in order

c_uint64_p = C.POINTER(C.c_uint64)

_SIGS = {
    "octo_draws_create": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(capi.OctoPrior), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "octo_draws_destroy": (C.c_int32, [C.c_void_p]),
    "octo_draws_detach": (C.c_int32, [C.c_void_p]),
    "octo_draws_last_error": (C.c_char_p, [C.c_void_p]),
    "octo_draws_sample_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_sync": (C.c_int32, [C.c_void_p]),
    "octo_draws_best": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, capi.c_double_p, capi.c_double_p, c_uint64_p]),
    "octo_draws_rejection": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, capi.c_double_p,
                                         c_uint64_p, C.POINTER(C.c_int64), capi.c_double_p]),
    "octo_draws_momentum_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_hmc_step_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_hmc_step": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p,
                                        capi.c_double_p, C.c_double, C.c_int32, capi.c_double_p, capi.c_double_p, capi.c_double_p, capi.c_double_p,
                                        capi.c_double_p, C.POINTER(C.c_int32)]),
    "octo_draws_lbfgs_direction_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_lbfgs_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_lbfgs": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                     capi.c_double_p, capi.c_double_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), capi.c_double_p]),
    "octo_draws_pathfinder_fit_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32] + [C.c_void_p] * 11 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_pathfinder_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double,
                                                 C.c_double, C.c_int32, C.c_int32] + [C.c_void_p] * 10),
    "octo_draws_pathfinder_draw_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_moments_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "octo_draws_metric_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "octo_draws_hmc_adapt_init_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "octo_draws_hmc_adapt_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_double,
                                                C.c_double, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "octo_draws_chain_moments_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_nuts_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                           C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 9),
    "octo_draws_slice_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                            C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 9),
    "octo_draws_diagnose_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_diagnose_work_doubles": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "octo_draws_rank_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "octo_draws_pt_stats_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 7),
    "octo_draws_pt_schedule_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    "octo_draws_reference_doubles": (C.c_int64, [C.c_int32]),
    "octo_draws_reference_set_device": (C.c_int32, [C.c_void_p] * 6),
    "octo_draws_reference_fit_device": (C.c_int32, [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 3),
    "octo_draws_use_reference": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "octo_draws_reference_exchange_device": (C.c_int32, [C.c_void_p, C.c_int64] + [C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
                                             + [C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_void_p]),
    "octo_draws_program_set": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "octo_draws_program_clear": (C.c_int32, [C.c_void_p]),
    "octo_draws_program_logpost_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_program_values_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "octo_draws_cube_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "octo_draws_from_cube_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 5),
    "octo_draws_nested_cull_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                  C.c_int64, C.c_int64] + [C.c_void_p] * 7),
    "octo_draws_nested_move_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 8),
    "octo_draws_cov_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_metric_dense_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_metric_apply_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_use_metric": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "octo_draws_de_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
                             + [C.c_void_p] * 8),
    "octo_draws_de_work_doubles": (C.c_int64, [C.c_int32, C.c_int64]),
    "octo_draws_ofti_set": (C.c_int32, [C.c_void_p] + [capi.c_double_p] * 6 + [C.c_int64, C.c_double, C.c_int32, C.c_double, C.c_void_p]),
    "octo_draws_ofti_clear": (C.c_int32, [C.c_void_p]),
    "octo_draws_ofti_nl_device": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_ofti_posterior_device": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "octo_draws_ofti_rejection": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, capi.c_double_p, capi.c_double_p, capi.c_double_p,
                                              c_uint64_p, C.POINTER(C.c_int64), capi.c_double_p]),
    "octo_draws_scan_set": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + [capi.c_double_p] * 6 + [C.c_int32, C.c_int64]),
    "octo_draws_scan_clear": (C.c_int32, [C.c_void_p]),
    "octo_draws_scan_eval_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p]),
    "octo_draws_scan_eval": (C.c_int32, [C.c_void_p, C.c_int32, capi.c_double_p, C.c_int64, C.c_int64] + [capi.c_double_p] * 7),
    "octo_draws_scan_values_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "octo_draws_scan_bind": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "octo_draws_scan_unbind": (C.c_int32, [C.c_void_p]),
    "octo_draws_pma_set": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + [capi.c_double_p] * 4 + [C.c_int32] + [capi.c_double_p] * 3 + [C.c_int32, C.c_int64]),
    "octo_draws_pma_clear": (C.c_int32, [C.c_void_p]),
    "octo_draws_pma_eval_device": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]),
    "octo_draws_pma_eval": (C.c_int32, [C.c_void_p, C.c_int32, capi.c_double_p, C.c_int64, C.c_int64] + [capi.c_double_p] * 5),
    "octo_draws_pma_values_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "octo_draws_pma_bind": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "octo_draws_pma_unbind": (C.c_int32, [C.c_void_p]),
    "octo_draws_gp_set": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p] + [capi.c_double_p] * 4 + [C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.c_int32]),
    "octo_draws_gp_clear": (C.c_int32, [C.c_void_p]),
    "octo_draws_gp_work_doubles": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "octo_draws_gp_dense_work_doubles": (C.c_int64, [C.c_int64, C.c_int32, C.c_int64, C.c_int32]),
    "octo_draws_gp_eval_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 8 + [C.c_int32, C.c_void_p]),
    "octo_draws_gp_eval": (C.c_int32, [C.c_void_p, capi.c_double_p, C.c_int64, C.c_int64] + [capi.c_double_p] * 8),
    "octo_draws_gp_values_device": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]),
    "octo_draws_gp_bind": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32]),
    "octo_draws_gp_unbind": (C.c_int32, [C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)

def load_library(path=None):
    """Load liboctofitter_hip_draws.so (after the main library it links against). Raises if it has not been built."""
    return companion.load_library(path, DRAWS_LIB_PATH, "OCTOFITTER_HIP_DRAWS_LIB", _SIGS, needs_main=True,
                                  no_fallback="Prior draws on the device have no CPU fallback.")


def _u64ptr(a):
    return a.ctypes.data_as(c_uint64_p)


# ---- the argument rules of the device calls. They only inspect their arguments; `dev` is the handle's torch.device.
def ptr(x):
    """The address of a tensor; None (a NULL pointer) for None: an input left at its default, an output switched off."""
    return None if x is None else x.data_ptr()


def chain_matrix(x, rows, dev, what, name="theta_t"):
    """(K, W, ld) of a float64 [K, W] tensor on `dev` with contiguous rows. rows: the K it must have (the handle's D), None: any.
    ld is the distance of two rows; a single row or empty rows have none, and ld = W."""
    import torch
    if x.dtype != torch.float64 or x.ndim != 2 or (rows is not None and x.shape[0] != rows) or x.device != dev or (x.shape[1] and x.stride(1) != 1):
        shape = "[K, W]" if rows is None else f"[D = {rows}, W]"
        raise ValueError(f"{what}: {name} must be a float64 {shape} tensor on {dev} with contiguous rows")
    K, W = int(x.shape[0]), int(x.shape[1])
    return K, W, (int(x.stride(0)) if K > 1 and W else W)


def single_row_ld(ld, D, *stacks):
    """The leading dimension of slot-major stacks [n, D, W] beside a matrix [D, W] of leading dimension ld. With D == 1 the matrix has no
    second row to say it: only the slots' distance does, that of the first (stack, n) with more than one slot."""
    if D == 1:
        for x, n in stacks:
            if n > 1:
                return int(x.stride(0))
    return ld


def slot_stack(x, n, D, W, ld, dev, what, name, slots="m"):
    """Refuses x unless it is a float64 [n, D, W] tensor on `dev`, slot-major: rows contiguous and ld apart, slots D·ld apart."""
    import torch
    ok = x.dtype == torch.float64 and x.device == dev and tuple(x.shape) == (n, D, W)
    if ok and W:
        ok = x.stride(2) == 1 and (D == 1 or x.stride(1) == ld) and (n == 1 or x.stride(0) == D * ld)
    if not ok:
        raise ValueError(f"{what}: {name} must be a float64 [{slots}, D = {D}, W = {W}] tensor on {dev} with g's leading dimension")


def history(cnt, head, S, Y, g, D, dev, what):
    """(W, ld, m, cnt, head) of a caller's L-BFGS history: g [D, W], S and Y [m, D, W] slot-major with g's leading dimension."""
    import torch
    _, W, ld = chain_matrix(g, D, dev, what, "g")
    m = int(S.shape[0]) if S.ndim == 3 else 0
    ld = single_row_ld(ld, D, (S, m))
    slot_stack(S, m, D, W, ld, dev, what, "S")
    slot_stack(Y, m, D, W, ld, dev, what, "Y")
    cnt, head = (torch.as_tensor(t, dtype=torch.int32, device=dev).contiguous() for t in (cnt, head))
    if cnt.shape != (W,) or head.shape != (W,):
        raise ValueError(f"{what}: cnt and head take {W} values each")
    return W, ld, m, cnt, head


def draw_cube(x, dev, what):
    """(x as [n, K, W], n, K, W, ld, ls) of stored draws: a float64 [n, K, W] or [n, W] tensor on `dev` whose samples are chain matrices
    (chain_matrix) a fixed distance ls apart."""
    if x.ndim == 2:
        x = x[:, None, :]
    if x.ndim != 3 or x.shape[0] < 1:
        raise ValueError(f"{what}: x must be a float64 [n, K, W] or [n, W] tensor on {dev}")
    K, W, ld = chain_matrix(x[0], None, dev, what, "x")
    return x, int(x.shape[0]), K, W, ld, int(x.stride(0))


def device_vector(x, n, dev, what):
    """None, or a float64 tensor of n elements on `dev` (a scalar is broadcast, host values are uploaded)."""
    import torch
    if x is None:
        return None
    t = torch.as_tensor(x, dtype=torch.float64, device=dev)
    t = t.expand(n).contiguous() if t.ndim == 0 else t.contiguous()
    if t.shape != (n,):
        raise ValueError(f"{what}: expected {n} values, got a tensor of shape {tuple(t.shape)}")
    return t


def group_ids(group, W, dev, what):
    """None, or the int32 [W] group ids on `dev`."""
    import torch
    if group is None:
        return None
    g = torch.as_tensor(group, device=dev).to(torch.int32).contiguous()
    if g.shape != (W,):
        raise ValueError(f"{what}: group takes {W} ids")
    return g


def pack_lower(L):
    """The packed factor [K(K+1)/2] (row i at i(i+1)/2, what octo_draws_use_metric reads) of the lower triangle of L [K, K]; what stands above
    the diagonal is dropped."""
    import torch
    K = int(L.shape[0])
    i, j = torch.tril_indices(K, K, device=L.device)
    return L[i, j].contiguous()


def unpack_lower(packed, K):
    """The lower-triangular [K, K] matrix of a packed factor [K(K+1)/2], zeros above the diagonal."""
    import torch
    L = torch.zeros((K, K), dtype=packed.dtype, device=packed.device)
    i, j = torch.tril_indices(K, K, device=packed.device)
    L[i, j] = packed
    return L


def is_adapt_state(state, G, dev):
    """Whether `state` is a dual-averaging state: a contiguous float64 [G, 4] tensor on `dev`."""
    import torch
    return state.dtype == torch.float64 and state.device == dev and state.shape == (G, 4) and state.is_contiguous()


class _MetricScope:
    """What PriorDraws.use_metric returns: leaving it as a context manager returns the handle to the diagonal metric."""
    def __init__(self, pd):
        self._pd = pd

    def __enter__(self):
        return self._pd

    def __exit__(self, *exc):
        self._pd.use_metric(None)
        return False


class PriorDraws(companion.Handle):
    """The handle of octo_draws_create. PriorDraws(model): for one LogDensityModel — its priors, its device model, its context; a model
    with Derived variables has an expression program instead of a device model, and the handle is given that (octo_draws_program_set).
    PriorDraws(model, program=(prog, binds)[, priors=[…]]): the model's context and dataset — and its priors unless others are given —
    under a program of the caller's (host/derived.py: Program; binds [(kind, node, value)] one per kernel input) in place of its device model.
    PriorDraws(priors=[…], device=0): a list of host/priors.py priors and a context of its own — sampling only (no best / rejection)."""

    PREFIX = "octo_draws"

    def __init__(self, model=None, priors=None, device=0, program=None):
        if model is None and priors is None or (model is not None and priors is not None and program is None):
            raise ValueError("PriorDraws takes a LogDensityModel or a list of priors (both only with a program)")
        if program is not None and model is None:
            raise ValueError("PriorDraws: a program needs a model, whose context and dataset it is evaluated on")
        self.model = model
        self._own_ctx = None
        self.program = None
        self._target = model is not None      # the handle has an ℓπ: a device model or a program
        self._open(load_library(), model.ln_like.device_index if model is not None else device)
        if model is not None and program is None and getattr(model, "program", None) is not None:
            program = (model.program, model._binds)
        if priors is None:
            self.D = int(model.D)
            self._c_priors = model._c_priors
        else:
            self.D = len(priors)
            self._c_priors = (capi.OctoPrior * max(self.D, 1))()
            for k, p in enumerate(priors):
                self._c_priors[k].kind = p.kind
                self._c_priors[k].p0, self._c_priors[k].p1, self._c_priors[k].lo, self._c_priors[k].hi = p.c_params()
        if model is not None:
            ctx, m = model.ln_like._ctx, (None if program is not None else model._m)
        else:
            main = capi.load_library()
            ctx, m = C.c_void_p(), None
            st = main.octo_ctx_create(C.byref(ctx), self.device_index)
            if st != capi.OCTO_OK:
                raise capi.OctoError(st, "octo_ctx_create")
            self._own_ctx = ctx
        self._created(self.lib.octo_draws_create(ctx, m, self._c_priors, self.D, self.device_index, C.byref(self._h)))
        self.scan_shape = None      # (n, K, P) of the scan table while one is set
        self.pma_shape = None       # (n, Q, K, P) of the catalogue table while one is set
        self.gp_shape = None        # (n, K, P, H, R) of the Gaussian-process RV table while one is set; R = 0 under dense kernels
        self.gp_dense = False       # its terms are dense kinds
        if program is not None:
            self.program_set(*program)
            scan = getattr(model, "_scan", None)
            if scan is not None and program[0] is getattr(model, "program", None):      # the model's along-scan observation: a term of its program
                obs, nodes = scan
                t = obs.table
                self.scan_set([(d["orbit_kind"], d["has_mass"]) for d in model.ln_like.planet_desc], t["epoch"], t["u"], t["v"], t["y"], t["sigma"],
                              obs.columns if obs.columns.shape[0] else None)
                self.scan_bind(nodes, obs.mode)
            pma = getattr(model, "_pma", None)
            if pma is not None and program[0] is getattr(model, "program", None):      # the model's catalogue fit: a term of its program
                obs, nodes = pma
                self.pma_set([(d["orbit_kind"], d["has_mass"]) for d in model.ln_like.planet_desc], obs.t, obs.u, obs.v, obs.L, obs.d, obs.cov, obs.H)
                self.pma_bind(nodes, obs.mode)
            gp = getattr(model, "_gp", None)
            if gp is not None and program[0] is getattr(model, "program", None):      # the model's Gaussian-process RV observation: a term of its program
                obs, nodes = gp
                self.gp_set([(d["orbit_kind"], d["has_mass"]) for d in model.ln_like.planet_desc], obs.table["epoch"], obs.table["rv"], obs.table["σ_rv"],
                            obs.gp_columns if obs.gp_columns.shape[0] else None, obs.gp_terms)
                self.gp_bind(nodes)

    # ---- derived variables (include/octofitter_hip_draws.h, "Derived variables"): a handle made from a model, without its device model
    def program_set(self, prog, binds):
        """octo_draws_program_set: from the next call on every function of the handle that needs ℓπ evaluates the program `prog`
        (host/derived.py: Program) with the bindings binds [(kind, node, value)] on the model's dataset."""
        fn = self.model.ln_like
        arrays = prog.c_arrays(binds)
        ops, n_ops, bs, n_binds, ts, n_terms = arrays
        self._check(self.lib.octo_draws_program_set(self._h, fn._ds, fn.n_planets, fn.n_obs, C.cast(ops, C.c_void_p), n_ops, C.cast(bs, C.c_void_p), n_binds,
                                                    C.cast(ts, C.c_void_p), n_terms))
        self.program, self._target = prog, True

    def program_clear(self):
        """octo_draws_program_clear: the handle is a sampling-only handle again."""
        self._check(self.lib.octo_draws_program_clear(self._h))
        self.program, self._target = None, False

    def program_logpost(self, theta_t, grad=True, out=None, stream=None):
        """(ℓπ [W], ∇ℓπ [D, W] of theta_t's leading dimension, or None) of the W columns of theta_t (torch float64 [D, W] on the handle's
        device, rows contiguous) through the program. out=(lp, grad): written in place. Asynchronous on `stream`."""
        _, W, ld = chain_matrix(theta_t, self.D, self.device, "program_logpost")
        lp, g = out if out is not None else (self._out(W), self._out(W, self.D, ld) if grad else None)
        self._check(self.lib.octo_draws_program_logpost_device(self._h, theta_t.data_ptr(), ld, W, lp.data_ptr(), ptr(g), self._stream(stream, self.device)))
        self._keep = (theta_t, lp, g)
        return lp, g

    def program_values(self, theta_t, nodes, stream=None):
        """The values [n, W] of the nodes `nodes` (indices: d < D a natural parameter, D + j the result of op j) at the W columns of theta_t."""
        _, W, ld = chain_matrix(theta_t, self.D, self.device, "program_values")
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        out = self._out(W, max(int(nodes.size), 1))[:nodes.size]
        self._check(self.lib.octo_draws_program_values_device(self._h, theta_t.data_ptr(), ld, W, nodes.ctypes.data_as(C.c_void_p), int(nodes.size), out.data_ptr(),
                                                              max(W, 1), self._stream(stream, self.device)))
        self._keep = (theta_t, out)
        return out

    def derived_columns(self, theta_t):
        """{name: [W] tensor} of the model's Derived variables at the columns of theta_t; {} for a model without any."""
        names = getattr(self.model, "derived_names", None) if self.model is not None and self.program is not None else None
        if not names:
            return {}
        return dict(zip(names, self.program_values(theta_t, self.model.derived_nodes)))

    @functools.cached_property
    def device(self):
        """The torch.device every tensor of a device call lives on."""
        import torch
        return torch.device("cuda", self.device_index)

    def _out(self, n, rows=None, ld=None, dtype=None):
        """An uninitialised output on the handle's device: [n] of `dtype` (default float64), or float64 [rows, n] whose rows are ld apart
        (default: contiguous)."""
        import torch
        if rows is None:
            return torch.empty(n, dtype=dtype or torch.float64, device=self.device)
        if ld is None:
            return torch.empty((rows, n), dtype=torch.float64, device=self.device)
        return torch.empty_strided((rows, n), (ld, 1), dtype=torch.float64, device=self.device)

    def sample(self, seed, first, n, theta=True, theta_t=True, logprior_t=True, stream=None):
        """Draws first … first + n − 1 of stream `seed` as torch float64 tensors on the model's device: (θ [D, n] natural domain,
        θ_t [D, n] linked, logprior_t [n]); None for an output switched off. Asynchronous on `stream` (default: torch's current stream)."""
        n = int(n)
        th = self._out(n, self.D) if theta else None
        tt = self._out(n, self.D) if theta_t else None
        lp = self._out(n) if logprior_t else None
        self._check(self.lib.octo_draws_sample_device(self._h, int(seed), int(first), n, n, ptr(th), ptr(tt), ptr(lp), self._stream(stream, self.device)))
        return th, tt, lp

    def best(self, seed, N, keep=1, first=0):
        """The `keep` highest log-posteriors among draws first … first + N − 1, best first (ties: lower draw index):
        (θ [D, keep] natural domain, logpost [keep], index [keep] uint64)."""
        keep = int(keep)
        th = np.empty((self.D, max(keep, 1)))
        lp = np.empty(max(keep, 1))
        ix = np.empty(max(keep, 1), dtype=np.uint64)
        self._check(self.lib.octo_draws_best(self._h, int(seed), int(first), int(N), keep, capi._dptr(th), capi._dptr(lp), _u64ptr(ix)))
        return th, lp, ix

    def rejection(self, seed, N, cap=None, first=0):
        """Rejection sampling with the prior as proposal over draws first … first + N − 1: the accepted draws in draw-index order,
        at most `cap` of them stored (default: all). dict(samples [D, n_stored], loglike, logpost, index, n_accepted, max_loglike)."""
        N = int(N)
        n_acc, mx = C.c_int64(0), C.c_double(0.0)
        room = min(N, max(65536, N // 16)) if cap is None else int(cap)
        while True:
            th = np.empty((self.D, max(room, 1)))      # the [D][cap] layout of the C call; only the accepted columns are ever touched
            ll, lp, ix = np.empty(max(room, 1)), np.empty(max(room, 1)), np.empty(max(room, 1), dtype=np.uint64)
            self._check(self.lib.octo_draws_rejection(self._h, int(seed), int(first), N, room, capi._dptr(th), capi._dptr(ll), capi._dptr(lp), _u64ptr(ix),
                                                      C.byref(n_acc), C.byref(mx)))
            if cap is not None or n_acc.value <= room:
                break
            room = int(n_acc.value)                    # more accepted than the first guess held: once more with room for all
        cap = room
        ns = min(int(n_acc.value), cap)
        return dict(samples=np.ascontiguousarray(th[:, :ns]), loglike=ll[:ns].copy(), logpost=lp[:ns].copy(), index=ix[:ns].copy(),
                    n_accepted=int(n_acc.value), max_loglike=float(mx.value))

    # ---- the OFTI rejection sampler (include/octofitter_hip_draws.h, "The sixteenth"): a handle of five priors (e, a, tp or τ, M, plx)
    def ofti_set(self, epochs, ra, dec, σ_ra, σ_dec, cor, σ_ABFG, tp_mode=0, t_ref=0.0, consts=None):
        """octo_draws_ofti_set: the RA/Dec table (host arrays; cor None = 0) and σ_ABFG of the OFTI likelihood. tp_mode 1: the third prior is τ and
        tp = t_ref + τ·P_d. consts: a capi.OctoConsts, what the context holds (None: the defaults)."""
        cols = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in (epochs, ra, dec, σ_ra, σ_dec)]
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError("ofti_set: the columns must have one length")
        cc = None if cor is None else np.ascontiguousarray(cor, dtype=np.float64).reshape(-1)
        if cc is not None and cc.size != n:
            raise ValueError("ofti_set: cor must have the columns' length")
        self._check(self.lib.octo_draws_ofti_set(self._h, *[capi._dptr(c) for c in cols], capi._dptr(cc), n, float(σ_ABFG), int(tp_mode), float(t_ref),
                                                 None if consts is None else C.cast(C.pointer(consts), C.c_void_p)))

    def ofti_clear(self):
        """octo_draws_ofti_clear"""
        self._check(self.lib.octo_draws_ofti_clear(self._h))

    def ofti_nl(self, theta, stream=None):
        """nl [5, n] (e, a, tp, M, plx: what octo_ofti_eval_device reads) of θ [5, n] in the natural domain (`sample`'s). Asynchronous on `stream`."""
        _, n, ld = chain_matrix(theta, 5, self.device, "ofti_nl", "theta")
        nl = self._out(n, 5, ld)
        self._check(self.lib.octo_draws_ofti_nl_device(self._h, n, ld, theta.data_ptr(), nl.data_ptr(), self._stream(stream, self.device)))
        self._keep = (theta, nl)
        return nl

    def ofti_posterior(self, seed, index, nl, stream=None):
        """The posterior rows [OFTI_N_OUT, n] (OFTI_OUTPUTS) of the parameter sets nl [5, n] with the draw indices `index` (uint64 values, n of them):
        the Thiele-Innes draw, its mean, its Campbell elements, ℓ. Asynchronous on `stream`."""
        import torch
        _, n, ld = chain_matrix(nl, 5, self.device, "ofti_posterior", "nl")
        ix = torch.as_tensor(np.ascontiguousarray(index, dtype=np.uint64).view(np.int64), device=self.device).contiguous()
        if ix.shape != (n,):
            raise ValueError(f"ofti_posterior: index takes {n} values")
        out = self._out(n, OFTI_N_OUT, ld)
        self._check(self.lib.octo_draws_ofti_posterior_device(self._h, int(seed), n, ld, ix.data_ptr(), nl.data_ptr(), out.data_ptr(), self._stream(stream, self.device)))
        self._keep = (ix, nl, out)
        return out

    def ofti_rejection(self, seed, N, cap=None, first=0):
        """Rejection sampling on the OFTI likelihood over draws first … first + N − 1: the accepted draws in draw-index order, at most `cap` of them
        stored (default: all). dict(theta [5, n_stored], nl [5, n_stored], post [OFTI_N_OUT, n_stored], index, n_accepted, max_logml)."""
        N = int(N)
        n_acc, mx = C.c_int64(0), C.c_double(0.0)
        room = min(N, max(65536, N // 16)) if cap is None else int(cap)
        while True:
            w = max(room, 1)
            th, nl, post, ix = np.empty((5, w)), np.empty((5, w)), np.empty((OFTI_N_OUT, w)), np.empty(w, dtype=np.uint64)
            self._check(self.lib.octo_draws_ofti_rejection(self._h, int(seed), int(first), N, room, capi._dptr(th), capi._dptr(nl), capi._dptr(post), _u64ptr(ix),
                                                           C.byref(n_acc), C.byref(mx)))
            if cap is not None or n_acc.value <= room:
                break
            room = int(n_acc.value)                    # more accepted than the first guess held: once more with room for all
        ns = min(int(n_acc.value), room)
        return dict(theta=np.ascontiguousarray(th[:, :ns]), nl=np.ascontiguousarray(nl[:, :ns]), post=np.ascontiguousarray(post[:, :ns]), index=ix[:ns].copy(),
                    n_accepted=int(n_acc.value), max_logml=float(mx.value))

    # ---- along-scan absolute astrometry (include/octofitter_hip_draws.h, "The seventeenth"): any handle; the binding needs a program
    def scan_set(self, planets, t, u, v, y, sigma, columns=None, consts=None):
        """octo_draws_scan_set: the scan table (host arrays of one length n; columns [K, n] or None) for the planets [(orbit_kind, has_mass)].
        consts: a capi.OctoConsts (None: the defaults)."""
        cols = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in (t, u, v, y, sigma)]
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError("scan_set: the columns must have one length")
        cm = np.zeros((0, n)) if columns is None else np.ascontiguousarray(columns, dtype=np.float64).reshape(-1, n)
        K = int(cm.shape[0])
        desc = (capi.OctoPlanetDesc * max(len(planets), 1))(*[capi.OctoPlanetDesc(int(k), int(bool(m))) for k, m in planets])
        self._check(self.lib.octo_draws_scan_set(self._h, C.cast(desc, C.c_void_p), len(planets), None if consts is None else C.cast(C.pointer(consts), C.c_void_p),
                                                 *[capi._dptr(c) for c in cols], capi._dptr(cm if K else None), K, n))
        self.scan_shape = (n, K, len(planets))

    def scan_clear(self):
        """octo_draws_scan_clear"""
        self._check(self.lib.octo_draws_scan_clear(self._h))
        self.scan_shape = None

    def scan_eval(self, elems, beta=None, jitter=None, mode="sampled", grad=True, accumulate=False, out=None, stream=None):
        """ℓ and its gradients of the W columns of elems (torch float64 [P·9, W] on the handle's device, rows contiguous; beta [K, W] with the same
        row distance, jitter [W] or None = 0): dict(ll [W], g_elems [P·9, W], g_beta [K, W] (sampled), g_jitter [W], beta_hat [K, W] (marginal));
        the gradients None with grad=False. accumulate: ll and g_elems are ADDED into out["ll"] and out["g_elems"]. Asynchronous on `stream`."""
        n, K, P = self.scan_shape
        _, W, ld = chain_matrix(elems, P * capi.N_EL, self.device, "scan_eval", "elems")
        m = SCAN_MODES[mode]
        if beta is not None and K:
            _, Wb, ldb = chain_matrix(beta, K, self.device, "scan_eval", "beta")
            if Wb != W or (K > 1 and W and ldb != ld):
                raise ValueError("scan_eval: beta must have elems' width and row distance")
        out = dict(out or {})
        if "ll" not in out:
            if accumulate:
                raise ValueError("scan_eval: accumulate needs out['ll']")
            out["ll"] = self._out(W)
        if grad:
            out.setdefault("g_elems", self._out(W, P * capi.N_EL, ld))
            out.setdefault("g_jitter", self._out(W))
            if m == SCAN_SAMPLED and K:
                out.setdefault("g_beta", self._out(W, K, ld))
        if m == SCAN_MARGINAL:
            out.setdefault("beta_hat", self._out(W, K, ld))
        self._check(self.lib.octo_draws_scan_eval_device(self._h, m, elems.data_ptr(), ld, W, ptr(beta) if K else None, ptr(jitter), out["ll"].data_ptr(),
                                                         ptr(out.get("g_elems")), ptr(out.get("g_beta")), ptr(out.get("g_jitter")), ptr(out.get("beta_hat")),
                                                         int(bool(accumulate)), self._stream(stream, self.device)))
        self._keep = (elems, beta, jitter, out)
        return out

    def scan_eval_host(self, elems, beta=None, jitter=None, mode="sampled", grad=True):
        """octo_draws_scan_eval: the same on NumPy arrays (elems [P·9, W], beta [K, W], jitter [W]), blocking."""
        n, K, P = self.scan_shape
        m = SCAN_MODES[mode]
        elems = np.ascontiguousarray(elems, dtype=np.float64).reshape(P * capi.N_EL, -1)
        W = elems.shape[1]
        beta = None if beta is None or not K else np.ascontiguousarray(beta, dtype=np.float64).reshape(K, W)
        jitter = None if jitter is None else np.ascontiguousarray(jitter, dtype=np.float64).reshape(W)
        out = dict(ll=np.empty(W))
        if grad:
            out.update(g_elems=np.empty((P * capi.N_EL, W)), g_jitter=np.empty(W))
            if m == SCAN_SAMPLED and K:
                out["g_beta"] = np.empty((K, W))
        if m == SCAN_MARGINAL:
            out["beta_hat"] = np.empty((K, W))
        self._check(self.lib.octo_draws_scan_eval(self._h, m, capi._dptr(elems), W, W, capi._dptr(beta), capi._dptr(jitter), capi._dptr(out["ll"]),
                                                  capi._dptr(out.get("g_elems")), capi._dptr(out.get("g_beta")), capi._dptr(out.get("g_jitter")),
                                                  capi._dptr(out.get("beta_hat"))))
        return out

    def scan_values(self, elems, beta=None, stream=None):
        """The model values η [n, W] at the W columns of elems (beta None: the reflex part alone). Asynchronous on `stream`."""
        n, K, P = self.scan_shape
        _, W, ld = chain_matrix(elems, P * capi.N_EL, self.device, "scan_values", "elems")
        if beta is not None and K:
            _, Wb, ldb = chain_matrix(beta, K, self.device, "scan_values", "beta")
            if Wb != W or (K > 1 and W and ldb != ld):
                raise ValueError("scan_values: beta must have elems' width and row distance")
        eta = self._out(W, n)
        self._check(self.lib.octo_draws_scan_values_device(self._h, elems.data_ptr(), ld, W, ptr(beta) if K else None, eta.data_ptr(), max(W, 1),
                                                           self._stream(stream, self.device)))
        self._keep = (elems, beta, eta)
        return eta

    def scan_bind(self, nodes, mode="sampled"):
        """octo_draws_scan_bind: the table becomes a term of the handle's program. nodes: the program's node indices of the β parameters in
        column order and then of the jitter (sampled), or of the jitter alone (marginal)."""
        from . import derived
        bs = (derived.OctoDrawsBind * max(len(nodes), 1))(*[derived.OctoDrawsBind(derived.BIND_NODE, int(k), 0.0) for k in nodes])
        self._check(self.lib.octo_draws_scan_bind(self._h, SCAN_MODES[mode], C.cast(bs, C.c_void_p), len(nodes)))

    def scan_unbind(self):
        """octo_draws_scan_unbind"""
        self._check(self.lib.octo_draws_scan_unbind(self._h))

    # ---- the catalogue proper-motion anomaly (include/octofitter_hip_draws.h, "The eighteenth"): any handle; the binding needs a program
    def pma_set(self, planets, t, u, v, L, d, cov, H=None, consts=None):
        """octo_draws_pma_set: the table (host arrays: t, u, v of one length n; the projector L [Q, n]; the catalogue values d [Q]; their covariance
        cov [Q, Q]; the constant design H [Q, K] or None) for the planets [(orbit_kind, has_mass)]. consts: a capi.OctoConsts (None: the defaults)."""
        cols = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in (t, u, v)]
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError("pma_set: t, u and v must have one length")
        Lm = np.ascontiguousarray(L, dtype=np.float64).reshape(-1, n)
        Q = int(Lm.shape[0])
        dv = np.ascontiguousarray(d, dtype=np.float64).reshape(-1)
        cm = np.ascontiguousarray(cov, dtype=np.float64)
        Hm = np.zeros((Q, 0)) if H is None else np.ascontiguousarray(H, dtype=np.float64).reshape(Q, -1)
        K = int(Hm.shape[1])
        if dv.size != Q or cm.shape != (Q, Q):
            raise ValueError("pma_set: L [Q, n], d [Q] and cov [Q, Q] must agree on Q")
        desc = (capi.OctoPlanetDesc * max(len(planets), 1))(*[capi.OctoPlanetDesc(int(k), int(bool(m))) for k, m in planets])
        self._check(self.lib.octo_draws_pma_set(self._h, C.cast(desc, C.c_void_p), len(planets), None if consts is None else C.cast(C.pointer(consts), C.c_void_p),
                                                *[capi._dptr(c) for c in cols], capi._dptr(Lm), Q, capi._dptr(dv), capi._dptr(cm), capi._dptr(Hm if K else None), K, n))
        self.pma_shape = (n, Q, K, len(planets))

    def pma_clear(self):
        """octo_draws_pma_clear"""
        self._check(self.lib.octo_draws_pma_clear(self._h))
        self.pma_shape = None

    def pma_eval(self, elems, gamma=None, mode="sampled", grad=True, accumulate=False, out=None, stream=None):
        """ℓ and its gradients of the W columns of elems (torch float64 [P·9, W] on the handle's device, rows contiguous; gamma [K, W] with the same
        row distance): dict(ll [W], g_elems [P·9, W], g_gamma [K, W] (sampled), gamma_hat [K, W] (marginal)); with grad=False no g_elems and only the
        two forward kernels run. accumulate: ll and g_elems are ADDED into out["ll"] and out["g_elems"]. Asynchronous on `stream`."""
        n, Q, K, P = self.pma_shape
        _, W, ld = chain_matrix(elems, P * capi.N_EL, self.device, "pma_eval", "elems")
        m = PMA_MODES[mode]
        if gamma is not None and K:
            _, Wg, ldg = chain_matrix(gamma, K, self.device, "pma_eval", "gamma")
            if Wg != W or (K > 1 and W and ldg != ld):
                raise ValueError("pma_eval: gamma must have elems' width and row distance")
        out = dict(out or {})
        if "ll" not in out:
            if accumulate:
                raise ValueError("pma_eval: accumulate needs out['ll']")
            out["ll"] = self._out(W)
        if grad:
            out.setdefault("g_elems", self._out(W, P * capi.N_EL, ld))
        if m == PMA_SAMPLED and K:
            out.setdefault("g_gamma", self._out(W, K, ld))
        if m == PMA_MARGINAL:
            out.setdefault("gamma_hat", self._out(W, K, ld))
        self._check(self.lib.octo_draws_pma_eval_device(self._h, m, elems.data_ptr(), ld, W, ptr(gamma) if K else None, out["ll"].data_ptr(), ptr(out.get("g_elems")),
                                                        ptr(out.get("g_gamma")), ptr(out.get("gamma_hat")), int(bool(accumulate)), self._stream(stream, self.device)))
        self._keep = (elems, gamma, out)
        return out

    def pma_eval_host(self, elems, gamma=None, mode="sampled", grad=True):
        """octo_draws_pma_eval: the same on NumPy arrays (elems [P·9, W], gamma [K, W]), blocking."""
        n, Q, K, P = self.pma_shape
        m = PMA_MODES[mode]
        elems = np.ascontiguousarray(elems, dtype=np.float64).reshape(P * capi.N_EL, -1)
        W = elems.shape[1]
        gamma = None if gamma is None or not K else np.ascontiguousarray(gamma, dtype=np.float64).reshape(K, W)
        out = dict(ll=np.empty(W))
        if grad:
            out["g_elems"] = np.empty((P * capi.N_EL, W))
        if m == PMA_SAMPLED and K:
            out["g_gamma"] = np.empty((K, W))
        if m == PMA_MARGINAL:
            out["gamma_hat"] = np.empty((K, W))
        self._check(self.lib.octo_draws_pma_eval(self._h, m, capi._dptr(elems), W, W, capi._dptr(gamma), capi._dptr(out["ll"]), capi._dptr(out.get("g_elems")),
                                                 capi._dptr(out.get("g_gamma")), capi._dptr(out.get("gamma_hat"))))
        return out

    def pma_values(self, elems, gamma=None, stream=None):
        """The model's catalogue values m = z + H·γ [Q, W] at the W columns of elems (gamma None: z alone). Asynchronous on `stream`."""
        n, Q, K, P = self.pma_shape
        _, W, ld = chain_matrix(elems, P * capi.N_EL, self.device, "pma_values", "elems")
        if gamma is not None and K:
            _, Wg, ldg = chain_matrix(gamma, K, self.device, "pma_values", "gamma")
            if Wg != W or (K > 1 and W and ldg != ld):
                raise ValueError("pma_values: gamma must have elems' width and row distance")
        m = self._out(W, Q)
        self._check(self.lib.octo_draws_pma_values_device(self._h, elems.data_ptr(), ld, W, ptr(gamma) if K else None, m.data_ptr(), max(W, 1),
                                                          self._stream(stream, self.device)))
        self._keep = (elems, gamma, m)
        return m

    def pma_bind(self, nodes, mode="sampled"):
        """octo_draws_pma_bind: the table becomes a term of the handle's program. nodes: the program's node indices of the γ parameters in column
        order (sampled), or none (marginal)."""
        from . import derived
        bs = (derived.OctoDrawsBind * max(len(nodes), 1))(*[derived.OctoDrawsBind(derived.BIND_NODE, int(k), 0.0) for k in nodes])
        self._check(self.lib.octo_draws_pma_bind(self._h, PMA_MODES[mode], C.cast(bs, C.c_void_p), len(nodes)))

    def pma_unbind(self):
        """octo_draws_pma_unbind"""
        self._check(self.lib.octo_draws_pma_unbind(self._h))

    # ---- the Gaussian-process RV term (include/octofitter_hip_draws.h, "The nineteenth"): any handle; the binding needs a program
    def gp_set(self, planets, t, rv, sigma, columns=None, terms=(GP_SHO,), consts=None):
        """octo_draws_gp_set: the RV table (host arrays of one length n, t non-decreasing; columns [K, n] or None) for the planets
        [(orbit_kind, has_mass)] under a celerite kernel of the term kinds `terms` (GP_REAL, GP_COMPLEX, GP_SHO) or a dense one (GP_SE, GP_MATERN32,
        GP_MATERN52, GP_PERIODIC, GP_QUASIPERIODIC; n <= GP_DENSE_MAX_N), never both. consts: a capi.OctoConsts."""
        cols = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in (t, rv, sigma)]
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError("gp_set: the columns must have one length")
        cm = np.zeros((0, n)) if columns is None else np.ascontiguousarray(columns, dtype=np.float64).reshape(-1, n)
        K = int(cm.shape[0])
        terms = [int(k) for k in terms]
        kinds = (C.c_int32 * max(len(terms), 1))(*terms)
        desc = (capi.OctoPlanetDesc * max(len(planets), 1))(*[capi.OctoPlanetDesc(int(k), int(bool(m))) for k, m in planets])
        self._check(self.lib.octo_draws_gp_set(self._h, C.cast(desc, C.c_void_p), len(planets), None if consts is None else C.cast(C.pointer(consts), C.c_void_p),
                                               *[capi._dptr(c) for c in cols], capi._dptr(cm if K else None), K, n, kinds, len(terms)))
        self.gp_dense = bool(terms) and all(k in GP_DENSE_N_HYPER for k in terms)      # the library refused a mixed list
        self.gp_shape = (n, K, len(planets), sum(GP_DENSE_N_HYPER[k] if self.gp_dense else GP_N_HYPER[k] for k in terms),
                         0 if self.gp_dense else sum(GP_N_SLOTS[k] for k in terms))

    def gp_clear(self):
        """octo_draws_gp_clear"""
        self._check(self.lib.octo_draws_gp_clear(self._h))
        self.gp_shape, self.gp_dense = None, False

    def gp_work_doubles(self, W, grad=True):
        """octo_draws_gp_work_doubles of the table that is set"""
        n, K, P, H, R = self.gp_shape
        if self.gp_dense:
            return int(self.lib.octo_draws_gp_dense_work_doubles(n, P, int(W), int(bool(grad))))
        return int(self.lib.octo_draws_gp_work_doubles(n, R, P, int(W), int(bool(grad))))

    def _gp_inputs(self, what, elems, hyper, beta):
        n, K, P, H, R = self.gp_shape
        _, W, ld = chain_matrix(elems, P * capi.N_EL, self.device, what, "elems")
        for name, x, rows in (("hyper", hyper, H), ("beta", beta, K)):
            if x is not None and rows:
                _, Wx, ldx = chain_matrix(x, rows, self.device, what, name)
                if Wx != W or (rows > 1 and W and ldx != ld):
                    raise ValueError(f"{what}: {name} must have elems' width and row distance")
        return W, ld

    def gp_eval(self, elems, hyper, beta=None, jitter=None, grad=True, accumulate=False, out=None, stream=None):
        """ℓ and its gradients of the W columns of elems (torch float64 [P·9, W] on the handle's device, rows contiguous; hyper [H, W] and beta [K, W]
        with the same row distance, jitter [W] or None = 0): dict(ll [W], g_elems [P·9, W], g_hyper [H, W], g_beta [K, W], g_jitter [W]); the
        gradients absent with grad=False. accumulate: ll and g_elems are ADDED into out["ll"] and out["g_elems"]. Asynchronous on `stream`."""
        n, K, P, H, R = self.gp_shape
        W, ld = self._gp_inputs("gp_eval", elems, hyper, beta)
        out = dict(out or {})
        if "ll" not in out:
            if accumulate:
                raise ValueError("gp_eval: accumulate needs out['ll']")
            out["ll"] = self._out(W)
        if grad:
            out.setdefault("g_elems", self._out(W, P * capi.N_EL, ld))
            out.setdefault("g_hyper", self._out(W, H, ld))
            out.setdefault("g_jitter", self._out(W))
            if K:
                out.setdefault("g_beta", self._out(W, K, ld))
        self._check(self.lib.octo_draws_gp_eval_device(self._h, elems.data_ptr(), ld, W, hyper.data_ptr(), ptr(beta) if K else None, ptr(jitter), out["ll"].data_ptr(),
                                                       ptr(out.get("g_elems")), ptr(out.get("g_hyper")), ptr(out.get("g_beta")), ptr(out.get("g_jitter")),
                                                       int(bool(accumulate)), self._stream(stream, self.device)))
        self._keep = (elems, hyper, beta, jitter, out)
        return out

    def gp_eval_host(self, elems, hyper, beta=None, jitter=None, grad=True):
        """octo_draws_gp_eval: the same on NumPy arrays (elems [P·9, W], hyper [H, W], beta [K, W], jitter [W]), blocking."""
        n, K, P, H, R = self.gp_shape
        elems = np.ascontiguousarray(elems, dtype=np.float64).reshape(P * capi.N_EL, -1)
        W = elems.shape[1]
        hyper = np.ascontiguousarray(hyper, dtype=np.float64).reshape(H, W)
        beta = None if beta is None or not K else np.ascontiguousarray(beta, dtype=np.float64).reshape(K, W)
        jitter = None if jitter is None else np.ascontiguousarray(jitter, dtype=np.float64).reshape(W)
        out = dict(ll=np.empty(W))
        if grad:
            out.update(g_elems=np.empty((P * capi.N_EL, W)), g_hyper=np.empty((H, W)), g_jitter=np.empty(W))
            if K:
                out["g_beta"] = np.empty((K, W))
        self._check(self.lib.octo_draws_gp_eval(self._h, capi._dptr(elems), W, W, capi._dptr(hyper), capi._dptr(beta), capi._dptr(jitter), capi._dptr(out["ll"]),
                                                capi._dptr(out.get("g_elems")), capi._dptr(out.get("g_hyper")), capi._dptr(out.get("g_beta")),
                                                capi._dptr(out.get("g_jitter"))))
        return out

    def gp_values(self, elems, hyper=None, beta=None, jitter=None, mean=False, stream=None):
        """The model values η [n, W] at the W columns of elems (beta None: the planets alone); with mean=True (η, μ), μ [n, W] the process's conditional
        mean at the table's epochs under hyper and jitter. Asynchronous on `stream`."""
        n, K, P, H, R = self.gp_shape
        W, ld = self._gp_inputs("gp_values", elems, hyper, beta)
        if mean and hyper is None:
            raise ValueError("gp_values: the conditional mean needs hyper")
        eta = self._out(W, n)
        mu = self._out(W, n) if mean else None
        self._check(self.lib.octo_draws_gp_values_device(self._h, elems.data_ptr(), ld, W, ptr(hyper), ptr(beta) if K else None, ptr(jitter), eta.data_ptr(), ptr(mu),
                                                         max(W, 1), self._stream(stream, self.device)))
        self._keep = (elems, hyper, beta, jitter, eta, mu)
        return (eta, mu) if mean else eta

    def gp_bind(self, nodes):
        """octo_draws_gp_bind: the table becomes a term of the handle's program. nodes: the program's node indices of the hyperparameters in term
        order, of the β parameters in column order, and then of the jitter."""
        from . import derived
        bs = (derived.OctoDrawsBind * max(len(nodes), 1))(*[derived.OctoDrawsBind(derived.BIND_NODE, int(k), 0.0) for k in nodes])
        self._check(self.lib.octo_draws_gp_bind(self._h, C.cast(bs, C.c_void_p), len(nodes)))

    def gp_unbind(self):
        """octo_draws_gp_unbind"""
        self._check(self.lib.octo_draws_gp_unbind(self._h))

    def momentum(self, seed, step, n, inv_mass=None, chain0=0, stream=None):
        """The momenta p [D, n] of chains chain0 … chain0 + n − 1 at `step`: standard normals of the counter generator over √inv_mass."""
        n = int(n)
        im = device_vector(inv_mass, self.D, self.device, "inv_mass")
        p = self._out(n, self.D)
        self._check(self.lib.octo_draws_momentum_device(self._h, int(seed), int(step), int(chain0), n, n, ptr(im), p.data_ptr(), self._stream(stream, self.device)))
        self._keep = (im,)
        return p

    def hmc_step(self, theta_t, beta=None, eps=None, n_leapfrog=4, inv_mass=None, seed=0, step=0, chain0=0, want_proposal=False, stream=None):
        """One tempered HMC step of the W chains in theta_t (torch float64 [D, W] on the handle's device, rows contiguous; updated in
        place where a chain accepts). beta: [W] or None (β = 1); eps: a number or [W]; inv_mass: [D] or None (1). A handle made from priors
        alone explores the prior (β = 0) and returns None for logpost and loglike.
        Returns (logpost [W], loglike [W], dH [W], accepted int32 [W][, proposal [D, W]]). Asynchronous on `stream`."""
        import torch
        dev = self.device
        _, W, ld = chain_matrix(theta_t, self.D, dev, "hmc_step")
        if eps is None:
            raise ValueError("hmc_step: eps is required (a number, or one value per chain)")
        per_chain = torch.is_tensor(eps) or np.ndim(eps) > 0
        eps_w = device_vector(eps, W, dev, "eps") if per_chain else None
        be = device_vector(beta, W, dev, "beta")
        im = device_vector(inv_mass, self.D, dev, "inv_mass")
        lp, ll = (self._out(W), self._out(W)) if self._target else (None, None)
        dH = self._out(W)
        acc = self._out(W, dtype=torch.int32)
        prop = self._out(W, self.D, ld) if want_proposal else None
        self._check(self.lib.octo_draws_hmc_step_device(self._h, int(seed), int(step), int(chain0), W, ld, theta_t.data_ptr(), ptr(be), ptr(eps_w),
                                                        0.0 if per_chain else float(eps), int(n_leapfrog), ptr(im), ptr(prop), ptr(lp), ptr(ll),
                                                        dH.data_ptr(), acc.data_ptr(), self._stream(stream, dev)))
        self._keep = (theta_t, be, eps_w, im)
        return (lp, ll, dH, acc, prop) if want_proposal else (lp, ll, dH, acc)

    def nuts(self, theta_t, beta=None, eps=None, inv_mass=None, max_depth=10, n_rounds=0, resume=False, seed=0, step=0, chain0=0, out=None, stream=None):
        """octo_draws_nuts_device, the raw call: opens (resume=False) or continues (resume=True: the same arguments, and out= the dict the
        opening call returned) one NUTS transition of the W chains in theta_t and makes n_rounds rounds of it, a leapfrog per chain still
        building. beta, eps, inv_mass as in hmc_step.
        Returns dict(logpost, loglike (None on a handle made from priors alone), log_accept [W], accepted, depth, n_leapfrog, diverged int32 [W],
        n_active int32 [1]: the chains still building), device tensors. Asynchronous on `stream`."""
        import torch
        dev = self.device
        _, W, ld = chain_matrix(theta_t, self.D, dev, "nuts")
        if eps is None:
            raise ValueError("nuts: eps is required (a number, or one value per chain)")
        per_chain = torch.is_tensor(eps) or np.ndim(eps) > 0
        eps_w = device_vector(eps, W, dev, "eps") if per_chain else None
        be = device_vector(beta, W, dev, "beta")
        im = device_vector(inv_mass, self.D, dev, "inv_mass")
        if out is None:
            i32 = lambda n: self._out(n, dtype=torch.int32)      # noqa: E731
            lp, ll = (self._out(W), self._out(W)) if self._target else (None, None)
            out = dict(logpost=lp, loglike=ll, log_accept=self._out(W), accepted=i32(W), depth=i32(W), n_leapfrog=i32(W), diverged=i32(W), n_active=i32(1))
        self._check(self.lib.octo_draws_nuts_device(self._h, int(seed), int(step), int(chain0), W, ld, theta_t.data_ptr(), ptr(be), ptr(eps_w),
                                                    0.0 if per_chain else float(eps), ptr(im), int(max_depth), int(n_rounds), 1 if resume else 0,
                                                    *(ptr(out[k]) for k in ("logpost", "loglike", "log_accept", "accepted", "depth", "n_leapfrog", "diverged", "n_active")),
                                                    self._stream(stream, dev)))
        self._keep = (theta_t, be, eps_w, im, out)
        return out

    def nuts_step(self, theta_t, beta=None, eps=None, inv_mass=None, max_depth=10, seed=0, step=0, chain0=0, check_from=3, stream=None):
        """One whole NUTS transition of the W chains in theta_t (torch float64 [D, W] on the handle's device, rows contiguous; a chain's
        column is written where its proposal is not its start). After 2^j − 1 rounds every unfinished chain stands at a doubling boundary: at
        those counts with j >= check_from the number of chains still building is read (a 4-byte copy, the only synchronisation) and the
        transition stops at 0. check_from=None: all 2^max_depth − 1 rounds, no synchronisation — the same bits.
        Returns (logpost [W], loglike [W], log_accept [W], accepted int32 [W], depth, n_leapfrog, diverged int32 [W]): hmc_step's tuple with the
        log of the mean acceptance statistic where dH is (adapt_step takes it as dH), and the tree's three counts."""
        md = int(max_depth)
        args = dict(beta=beta, eps=eps, inv_mass=inv_mass, max_depth=md, seed=seed, step=step, chain0=chain0, stream=stream)
        j = md if check_from is None else min(max(int(check_from), 0), md)
        out = self.nuts(theta_t, n_rounds=(1 << j) - 1, **args)
        while j < md and int(out["n_active"].item()) > 0:
            out = self.nuts(theta_t, n_rounds=1 << j, resume=True, out=out, **args)
            j += 1
        return tuple(out[k] for k in ("logpost", "loglike", "log_accept", "accepted", "depth", "n_leapfrog", "diverged"))

    def slice(self, theta_t, beta=None, w=10.0, p=3, n_passes=3, max_shrink=SLICE_MAX_SHRINK, n_rounds=0, resume=False, seed=0, step=0, chain0=0, out=None,
              stream=None):
        """octo_draws_slice_device, the raw call: opens (resume=False) or continues (resume=True: the same arguments, and out= the dict the
        opening call returned) one slice-sampling transition of the W chains in theta_t — n_passes sweeps over the coordinates — and makes
        n_rounds rounds of it, one forward evaluation per chain still active. w: the width, a number or one per coordinate [D]; p: the
        doublings; beta as in hmc_step.
        Returns dict(logpost, loglike (None on a handle made from priors alone), n_eval, n_expand, n_shrink, n_stuck, status int32 [W],
        n_active int32 [1]: the chains still active), device tensors. Asynchronous on `stream`."""
        import torch
        dev = self.device
        _, W, ld = chain_matrix(theta_t, self.D, dev, "slice")
        per_coordinate = torch.is_tensor(w) or np.ndim(w) > 0
        width = device_vector(w, self.D, dev, "w") if per_coordinate else None
        be = device_vector(beta, W, dev, "beta")
        if out is None:
            i32 = lambda n: self._out(n, dtype=torch.int32)      # noqa: E731
            lp, ll = (self._out(W), self._out(W)) if self._target else (None, None)
            out = dict(logpost=lp, loglike=ll, n_eval=i32(W), n_expand=i32(W), n_shrink=i32(W), n_stuck=i32(W), status=i32(W), n_active=i32(1))
        self._check(self.lib.octo_draws_slice_device(self._h, int(seed), int(step), int(chain0), W, ld, theta_t.data_ptr(), ptr(be), ptr(width),
                                                     0.0 if per_coordinate else float(w), int(p), int(n_passes), int(max_shrink), int(n_rounds), 1 if resume else 0,
                                                     *(ptr(out[k]) for k in SLICE_OUTPUTS), self._stream(stream, dev)))
        self._keep = (theta_t, be, width, out)
        return out

    def slice_step(self, theta_t, beta=None, w=10.0, p=3, n_passes=3, max_shrink=SLICE_MAX_SHRINK, seed=0, step=0, chain0=0, rounds_per_call=None, stream=None):
        """One whole slice-sampling transition of the W chains in theta_t (torch float64 [D, W] on the handle's device, rows contiguous; a
        coordinate is written where its update accepts). The rounds run in segments of rounds_per_call (default: 4·n_passes·D, about half of
        what a transition takes at the default p); after each the number of chains still active is read (a 4-byte copy, the only
        synchronisation) and the transition stops at 0, at the latest after the n_passes·D·(2 + p + max_shrink·(1 + p)) rounds that finish
        every chain. The same bits however the rounds are cut. Returns slice()'s dict."""
        updates = int(n_passes) * self.D
        per_call = 4 * updates if rounds_per_call is None else int(rounds_per_call)
        if per_call < 1:
            raise ValueError("slice_step: rounds_per_call >= 1")
        args = dict(beta=beta, w=w, p=p, n_passes=n_passes, max_shrink=max_shrink, seed=seed, step=step, chain0=chain0, stream=stream)
        done, out = 0, None
        most = updates * (2 + int(p) + int(max_shrink) * (1 + int(p)))
        while out is None or (done < most and int(out["n_active"].item()) > 0):
            n = min(per_call, most - done)
            out = self.slice(theta_t, n_rounds=n, resume=out is not None, out=out, **args)
            done += n
        return out

    # ---- differential evolution (include/octofitter_hip_draws.h, "Differential evolution")
    def de(self, theta_t, lo=None, hi=None, radius=8, n_gen=0, gen0=0, seed=0, resume=False, fcr=None, out=None, stream=None):
        """octo_draws_de_device, the raw call: opens (resume=False) or continues (resume=True: the same seed, radius and bounds, gen0 = the
        generations made so far, and out= the dict the opening call returned) a differential-evolution search on the population theta_t
        (torch float64 [D, W >= 4] on the handle's device, rows contiguous, updated in place) and makes n_gen generations of it, one forward
        evaluation per individual each. lo, hi: the bounds in θ_t [D], both or neither; radius: the ring neighbourhood the parents come from,
        0 = the whole population; fcr: a float64 [2, W] tensor with theta_t's leading dimension holding (F, CR) per individual, read at the
        opening and written by every call (default: one is made, opened at F = 0.5, CR = 0.9; False: none, the pairs stay in the handle).
        Returns dict(fcr, logpost, loglike (None on a handle made from priors alone), n_accept int32 [W], best int32 [1], best_logpost [1],
        n_improved int32 [1]), device tensors. Asynchronous on `stream`."""
        import torch
        dev = self.device
        _, W, ld = chain_matrix(theta_t, self.D, dev, "de")
        if (lo is None) != (hi is None):
            raise ValueError("de: lo and hi, both or neither")
        lo_t, hi_t = device_vector(lo, self.D, dev, "lo"), device_vector(hi, self.D, dev, "hi")
        if out is None:
            i32 = lambda n: self._out(n, dtype=torch.int32)      # noqa: E731
            lp, ll = (self._out(W), self._out(W)) if self._target else (None, None)
            pair = fcr
            if fcr is None:      # the library's opening values, in a pair the caller can read
                pair = self._out(W, 2, ld)
                pair[0].fill_(DE_F0)
                pair[1].fill_(DE_CR0)
            elif fcr is False:
                pair = None
            out = dict(fcr=pair, logpost=lp, loglike=ll, n_accept=i32(W), best=i32(1), best_logpost=self._out(1), n_improved=i32(1))
        if out["fcr"] is not None and chain_matrix(out["fcr"], 2, dev, "de", "fcr")[1:] != (W, ld):
            raise ValueError("de: fcr must be a float64 [2, W] tensor with theta_t's leading dimension")
        self._check(self.lib.octo_draws_de_device(self._h, int(seed), int(gen0), W, ld, theta_t.data_ptr(), ptr(lo_t), ptr(hi_t), int(radius), int(n_gen),
                                                  1 if resume else 0, *(ptr(out[k]) for k in DE_OUTPUTS), self._stream(stream, dev)))
        self._keep = (theta_t, lo_t, hi_t, out)
        return out

    def de_step(self, theta_t, lo=None, hi=None, radius=8, n_gen=100, gen0=0, seed=0, fcr=None, gens_per_call=None, stream=None):
        """n_gen generations of differential evolution on the population theta_t from its opening, in calls of gens_per_call generations
        (default: all in one). No value is read between the calls; the same bits however the generations are cut. Returns de()'s dict."""
        n_gen = int(n_gen)
        per_call = max(n_gen, 1) if gens_per_call is None else int(gens_per_call)
        if per_call < 1:
            raise ValueError("de_step: gens_per_call >= 1")
        args = dict(lo=lo, hi=hi, radius=radius, seed=seed, stream=stream)
        out = self.de(theta_t, n_gen=0, gen0=gen0, fcr=fcr, **args)
        done = 0
        while done < n_gen:
            n = min(per_call, n_gen - done)
            out = self.de(theta_t, n_gen=n, gen0=int(gen0) + done, resume=True, out=out, **args)
            done += n
        return out

    # ---- nested sampling (include/octofitter_hip_draws.h, "Nested sampling")
    def cube(self, seed, first, n, out=None, stream=None):
        """octo_draws_cube_device: the uniforms u [D, n] of draws first … first + n − 1, what `sample` feeds to the quantile. out: a float64
        [D, n] tensor with contiguous rows, written in place. Asynchronous on `stream`."""
        n = int(n)
        u = self._out(n, self.D) if out is None else out
        _, n_u, ld = chain_matrix(u, self.D, self.device, "cube", "out")
        if n_u != n:
            raise ValueError(f"cube: out must hold {n} columns")
        self._check(self.lib.octo_draws_cube_device(self._h, int(seed), int(first), n, ld, u.data_ptr(), self._stream(stream, self.device)))
        self._keep = (u,)
        return u

    def from_cube(self, u, theta=True, theta_t=True, logprior_t=True, out=None, stream=None):
        """octo_draws_from_cube_device, the hypercube transform of the columns of u [D, n]: (θ [D, n], θ_t [D, n], logprior_t [n]) as `sample`
        returns them, of u's leading dimension; None for an output switched off. A column with a coordinate outside (0, 1) gives NaN.
        out=(θ, θ_t, logprior_t): written in place (None: switched off); the matrices have u's shape and leading dimension."""
        _, n, ld = chain_matrix(u, self.D, self.device, "from_cube", "u")
        if out is not None:
            th, tt, lp = out
            for t, name in ((th, "theta"), (tt, "theta_t")):
                if t is not None and chain_matrix(t, self.D, self.device, "from_cube", name) != (self.D, n, ld):
                    raise ValueError(f"from_cube: {name} must have u's shape and leading dimension")
        else:
            th = self._out(n, self.D, ld) if theta else None
            tt = self._out(n, self.D, ld) if theta_t else None
            lp = self._out(n) if logprior_t else None
        self._check(self.lib.octo_draws_from_cube_device(self._h, n, ld, u.data_ptr(), ptr(th), ptr(tt), ptr(lp), self._stream(stream, self.device)))
        self._keep = (u,)
        return th, tt, lp

    def nested_state(self):
        """The initial state of a nested-sampling run, float64 [8] on the device: NESTED_STATE names its entries."""
        import torch
        inf = float("inf")
        return torch.tensor([-inf, 0.0, -inf, -inf, inf, 0.0, 0.0, 0.0], dtype=torch.float64, device=self.device)

    def _live(self, u_live, loglike_live, state, what):
        import torch
        _, K, ldK = chain_matrix(u_live, self.D, self.device, what, "u_live")
        for t, n, name in ((loglike_live, K, "loglike_live"), (state, 8, "state")):
            if t.dtype != torch.float64 or t.device != self.device or t.shape != (n,) or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be a contiguous float64 [{n}] tensor on {self.device}")
        return K, ldK

    def nested_cull(self, u_live, loglike_live, state, B, replace=True, seed=0, iter=0, dead=None, dead_first=0, slot=None, width=None, stream=None):
        """octo_draws_nested_cull_device: removes the B lowest of the K live points u_live [D, K], loglike_live [K] (both in place), updates
        state [8] in place, and with replace copies a survivor into every dead slot. dead: None, or dict(u [D, n], loglike, logvol, logwt [n]) of
        caller arrays that receive the records at columns dead_first … dead_first + B − 1. Returns (slot int32 [B], width [D] or None without
        replace). Asynchronous on `stream`."""
        import torch
        K, ldK = self._live(u_live, loglike_live, state, "nested_cull")
        B = int(B)
        slot = self._out(max(B, 1), dtype=torch.int32) if slot is None else slot
        if replace and width is None:
            width = self._out(self.D)
        ld_dead, dp = int(dead_first) + B, [None] * 4
        if dead is not None:
            _, _, ld_dead = chain_matrix(dead["u"], self.D, self.device, "nested_cull", "dead['u']")
            if any(int(dead[k].numel()) < int(dead_first) + B for k in ("loglike", "logvol", "logwt")):
                raise ValueError("nested_cull: the dead arrays hold fewer than dead_first + B records")
            dp = [ptr(dead[k]) for k in ("u", "loglike", "logvol", "logwt")]
        self._check(self.lib.octo_draws_nested_cull_device(self._h, int(seed), int(iter), K, ldK, u_live.data_ptr(), loglike_live.data_ptr(), state.data_ptr(), B,
                                                           1 if replace else 0, int(dead_first), ld_dead, *dp, slot.data_ptr(), ptr(width) if replace else None,
                                                           self._stream(stream, self.device)))
        self._keep = (u_live, loglike_live, state, dead, slot, width)
        return slot[:B], (width if replace else None)

    def nested_move(self, u_live, loglike_live, state, slot, w=1.0, max_steps=8, n_passes=3, max_shrink=NESTED_MAX_SHRINK, n_rounds=0, resume=False, seed=0, iter=0,
                    want_theta_t=False, out=None, stream=None):
        """octo_draws_nested_move_device, the raw call: opens (resume=False) or continues (resume=True: the same arguments, and out= the dict
        the opening call returned) one constrained-prior transition of the live slots `slot` (int32 [B]) under the floor state[2], in place in
        u_live and loglike_live, and makes n_rounds rounds of it. w: the width in the cube, a number or one per coordinate [D].
        Returns dict(theta_t [D, B] or None, n_eval, n_step, n_shrink, n_stuck, status int32 [B], n_active int32 [1]). Asynchronous on `stream`."""
        import torch
        dev = self.device
        K, ldK = self._live(u_live, loglike_live, state, "nested_move")
        if slot.dtype != torch.int32 or slot.device != dev or slot.ndim != 1 or not slot.is_contiguous():
            raise ValueError(f"nested_move: slot must be a contiguous int32 [B] tensor on {dev}")
        B = int(slot.numel())
        per_coordinate = torch.is_tensor(w) or np.ndim(w) > 0
        width = device_vector(w, self.D, dev, "w") if per_coordinate else None
        if out is None:
            i32 = lambda n: self._out(n, dtype=torch.int32)      # noqa: E731
            out = dict(theta_t=self._out(B, self.D) if want_theta_t else None, n_eval=i32(B), n_step=i32(B), n_shrink=i32(B), n_stuck=i32(B), status=i32(B),
                       n_active=i32(1))
        ld = B if out["theta_t"] is None else chain_matrix(out["theta_t"], self.D, dev, "nested_move", "out['theta_t']")[2]
        self._check(self.lib.octo_draws_nested_move_device(self._h, int(seed), int(iter), K, ldK, u_live.data_ptr(), loglike_live.data_ptr(), state.data_ptr(), B, ld,
                                                           slot.data_ptr(), ptr(width), 0.0 if per_coordinate else float(w), int(max_steps), int(n_passes),
                                                           int(max_shrink), int(n_rounds), 1 if resume else 0, *(ptr(out[k]) for k in NESTED_MOVE_OUTPUTS),
                                                           self._stream(stream, dev)))
        self._keep = (u_live, loglike_live, state, slot, width, out)
        return out

    def nested_step(self, u_live, loglike_live, state, B, w=None, max_steps=8, n_passes=3, max_shrink=NESTED_MAX_SHRINK, seed=0, iter=0, dead=None, dead_first=0,
                    rounds_per_call=None, want_theta_t=False, stream=None):
        """One iteration of nested sampling: one cull of the B lowest live points (nested_cull with replace), then the move of their slots in
        segments of rounds_per_call rounds (default 2·n_passes·D) until no chain is active — after each segment the number of active chains is
        read (a 4-byte copy, the only synchronisation). w: None = the cull's per-coordinate widths. The same bits however the rounds are cut.
        Returns nested_move's dict, with slot and width."""
        slot, width = self.nested_cull(u_live, loglike_live, state, B, replace=True, seed=seed, iter=iter, dead=dead, dead_first=dead_first, stream=stream)
        updates = int(n_passes) * self.D
        per_call = 2 * updates if rounds_per_call is None else int(rounds_per_call)
        if per_call < 1:
            raise ValueError("nested_step: rounds_per_call >= 1")
        args = dict(w=width if w is None else w, max_steps=max_steps, n_passes=n_passes, max_shrink=max_shrink, seed=seed, iter=iter, stream=stream)
        done, out = 0, None
        most = updates * (int(max_steps) - 1 + int(max_shrink))      # what finishes every chain
        while out is None or (done < most and int(out["n_active"].item()) > 0):
            n = min(per_call, most - done)
            out = self.nested_move(u_live, loglike_live, state, slot, n_rounds=n, resume=out is not None, want_theta_t=want_theta_t, out=out, **args)
            done += n
        return dict(out, slot=slot, width=width)

    def lbfgs_direction(self, cnt, head, S, Y, g, inv_mass=None, stream=None):
        """The two-loop recursion of every chain on its own history: d [D, W] = −H·g with H₀ = γ·diag(inv_mass). cnt, head: int32 [W] (stored
        pairs; the slot the next pair would take); S, Y: float64 [m, D, W], slot-major, rows contiguous and of g's leading dimension; g: [D, W]. Asynchronous."""
        W, ld, m, cnt, head = history(cnt, head, S, Y, g, self.D, self.device, "lbfgs_direction")
        im = device_vector(inv_mass, self.D, self.device, "inv_mass")
        out = self._out(W, self.D, ld)
        self._check(self.lib.octo_draws_lbfgs_direction_device(self._h, W, ld, m, cnt.data_ptr(), head.data_ptr(), S.data_ptr(), Y.data_ptr(), g.data_ptr(),
                                                               ptr(im), out.data_ptr(), self._stream(stream, self.device)))
        self._keep = (cnt, head, S, Y, g, im)
        return out

    def _optimizer_outputs(self, what, theta_t, inv_mass, want_inv_hess_diag):
        """What lbfgs and pathfinder share: (W, ld) of theta_t, inv_mass on the device, and the dict they return, its tensors allocated."""
        import torch
        _, W, ld = chain_matrix(theta_t, self.D, self.device, what)
        im = device_vector(inv_mass, self.D, self.device, "inv_mass")
        r = dict(logpost=self._out(W), gnorm=self._out(W), status=self._out(W, dtype=torch.int32), iters=self._out(W, dtype=torch.int32),
                 evals=self._out(W, dtype=torch.int32), inv_hess_diag=self._out(W, self.D, ld) if want_inv_hess_diag else None)
        return W, ld, im, r

    def lbfgs(self, theta_t, inv_mass=None, m=6, n_rounds=50, gtol=1e-6, ftol=0.0, resume=False, want_inv_hess_diag=False, stream=None):
        """n_rounds rounds of the batched L-BFGS (include/octofitter_hip_draws.h states it) on the W chains in theta_t (torch float64 [D, W] on
        the handle's device, rows contiguous; updated in place where a chain accepts). inv_mass: the scaling v, [D] or None (1). resume=True
        goes on from the state the handle holds: the same theta_t, W and m as the call before.
        Returns dict(logpost [W], gnorm [W], status int32 [W] (LBFGS_*), iters, evals int32 [W], inv_hess_diag [D, W] or None), device tensors.
        Asynchronous on `stream`."""
        W, ld, im, r = self._optimizer_outputs("lbfgs", theta_t, inv_mass, want_inv_hess_diag)
        self._check(self.lib.octo_draws_lbfgs_device(self._h, W, ld, theta_t.data_ptr(), ptr(im), int(m), int(n_rounds), float(gtol), float(ftol),
                                                     1 if resume else 0, *(ptr(t) for t in r.values()), self._stream(stream, self.device)))
        self._keep = (theta_t, im)
        return r

    def pathfinder_fit(self, cnt, head, S, Y, x, g, alpha, z=None, stream=None):
        """Pathfinder's normal fit of every chain on its own history (include/octofitter_hip_draws.h states it): cnt, head, S, Y as in
        lbfgs_direction; x, g (= −∇ℓπ), alpha: float64 [D, W] of one leading dimension; z: None or [n, D, W] standard normals of the same
        leading dimension. Returns dict(mu [D, W], chol [D(D+1)/2, W] (L̃ packed row-major), logdet [W], ok int32 [W], phi [n, D, W] or None):
        Σ = diag(√α)·L̃L̃ᵀ·diag(√α), φ = μ + √α ⊙ (L̃z). Asynchronous."""
        import torch
        dev = self.device
        W, ld, m, cnt, head = history(cnt, head, S, Y, g, self.D, dev, "pathfinder_fit")
        like_g = chain_matrix(g, self.D, dev, "pathfinder_fit", "g")      # before the single-row rule: x and alpha are matrices, as g is
        for t, name in ((x, "x"), (alpha, "alpha")):
            if chain_matrix(t, self.D, dev, "pathfinder_fit", name) != like_g:
                raise ValueError(f"pathfinder_fit: {name} must have g's shape and leading dimension")
        n = 0 if z is None else int(z.shape[0])
        ld = single_row_ld(ld, self.D, (S, m), (z, n))
        if z is not None:
            slot_stack(z, n, self.D, W, ld, dev, "pathfinder_fit", "z", slots="n")
        mu = self._out(W, self.D, ld)
        chol = self._out(W, self.D * (self.D + 1) // 2, ld)
        logdet = self._out(W)
        ok = self._out(W, dtype=torch.int32)
        phi = torch.empty_strided((n, self.D, W), (self.D * ld, ld, 1), dtype=torch.float64, device=dev) if n else None
        self._check(self.lib.octo_draws_pathfinder_fit_device(self._h, W, ld, m, cnt.data_ptr(), head.data_ptr(), S.data_ptr(), Y.data_ptr(), x.data_ptr(),
                                                              g.data_ptr(), alpha.data_ptr(), mu.data_ptr(), chol.data_ptr(), logdet.data_ptr(), ok.data_ptr(), n,
                                                              ptr(z), ptr(phi), self._stream(stream, dev)))
        self._keep = (cnt, head, S, Y, x, g, alpha, z)
        return dict(mu=mu, chol=chol, logdet=logdet, ok=ok, phi=phi)

    def pathfinder(self, theta_t, inv_mass=None, m=6, n_rounds=50, gtol=1e-6, ftol=0.0, resume=False, want_inv_hess_diag=False, seed=0, chain0=0, n_elbo=5,
                   stream=None):
        """lbfgs (the same arguments, the same bits in theta_t and in its outputs) with Pathfinder along the path: after every round the
        normal fit of each chain that accepted, its ELBO from n_elbo draws of the counter stream (seed, chain0 + c), and the best fit kept
        on the handle for pathfinder_draw. resume=True goes on from the previous pathfinder call.
        Returns lbfgs's dict plus elbo [W] (−Inf without a fit), elbo_iter int32 [W] (the iters of the kept fit, −1 without one), n_fits int32 [W].
        Asynchronous on `stream`."""
        import torch
        W, ld, im, r = self._optimizer_outputs("pathfinder", theta_t, inv_mass, want_inv_hess_diag)
        r.update(elbo=self._out(W), elbo_iter=self._out(W, dtype=torch.int32), n_fits=self._out(W, dtype=torch.int32))
        self._check(self.lib.octo_draws_pathfinder_device(self._h, int(seed), int(chain0), W, ld, theta_t.data_ptr(), ptr(im), int(m), int(n_rounds), float(gtol),
                                                          float(ftol), int(n_elbo), 1 if resume else 0, *(ptr(t) for t in r.values()),
                                                          self._stream(stream, self.device)))
        self._keep = (theta_t, im)
        return r

    def pathfinder_draw(self, theta_t, n_draws, seed=0, chain0=0, stream=None):
        """n_draws draws from the kept fit of every chain of the previous pathfinder call (theta_t as that call left it, the same chain0):
        (φ [D, n_draws·W] in θ_t, draw j of chain c in column j·W + c; log q [n_draws·W]; ℓπ [n_draws·W]). A chain without a fit gives its
        x, log q = NaN and ℓπ = −Inf. Asynchronous on `stream`."""
        _, W, ld = chain_matrix(theta_t, self.D, self.device, "pathfinder_draw")
        n = int(n_draws)
        cols = max(n, 0) * W
        phi, logq, lp = self._out(cols, self.D), self._out(cols), self._out(cols)
        self._check(self.lib.octo_draws_pathfinder_draw_device(self._h, int(seed), int(chain0), W, ld, theta_t.data_ptr(), n, cols, phi.data_ptr(), logq.data_ptr(),
                                                               lp.data_ptr(), self._stream(stream, self.device)))
        self._keep = (theta_t,)
        return phi, logq, lp

    # ---- warm-up (include/octofitter_hip_draws.h, "Warm-up of the explorer"): K = the rows of x, not the handle's D
    def moments(self, x, group=None, G=1, out=None, accumulate=False, stream=None):
        """Cross-chain moments of x [K, W] per group (group: int32 [W] ids, None = one group; ids outside 0 … G − 1 and chains with a
        non-finite value are excluded): (count [G], mean [G, K], m2 [G, K] = Σ(x − mean)²), device tensors. out=(count, mean, m2): write into these;
        with accumulate=True Chan-merge this call's block into what they hold. Asynchronous on `stream`."""
        K, W, ld = chain_matrix(x, None, self.device, "moments", "x")
        g = group_ids(group, W, self.device, "moments")
        G = int(G)
        if accumulate and out is None:
            raise ValueError("moments: accumulate=True needs out=(count, mean, m2)")
        if out is None:
            cnt, mean, m2 = self._out(G), self._out(K, G), self._out(K, G)
        else:
            cnt, mean, m2 = out
            if cnt.shape != (G,) or mean.shape != (G, K) or m2.shape != (G, K) or not (cnt.is_contiguous() and mean.is_contiguous() and m2.is_contiguous()):
                raise ValueError(f"moments: out must be contiguous (count [{G}], mean [{G}, {K}], m2 [{G}, {K}])")
        self._check(self.lib.octo_draws_moments_device(self._h, W, ld, K, x.data_ptr(), ptr(g), G, 1 if accumulate else 0,
                                                       cnt.data_ptr(), mean.data_ptr(), m2.data_ptr(), self._stream(stream, self.device)))
        self._keep = (x, g)
        return cnt, mean, m2

    def metric(self, count, mean, m2, inv_mass, regularize=True, stream=None):
        """inv_mass [K] (updated in place, returned) from ONE group's moments: count [1], mean [K], m2 [K] (rows of moments' outputs).
        M2/(n − 1), with regularize Stan's shrinkage towards 1e-3; entries with n < 2 or a variance not finite and > 0 keep their value."""
        import torch
        K = int(m2.numel())
        for t, n in ((count, 1), (mean, K), (m2, K), (inv_mass, K)):
            if t.dtype != torch.float64 or t.device != self.device or t.numel() != n or not t.is_contiguous():
                raise ValueError("metric: count [1], mean [K], m2 [K] and inv_mass [K] must be contiguous float64 tensors on the handle's device")
        self._check(self.lib.octo_draws_metric_device(self._h, K, count.data_ptr(), mean.data_ptr(), m2.data_ptr(), 1 if regularize else 0, inv_mass.data_ptr(),
                                                      self._stream(stream, self.device)))
        self._keep = (count, mean, m2, inv_mass)
        return inv_mass

    # ---- the dense metric (include/octofitter_hip_draws.h, "The dense metric"): packed lower triangles, row i at i(i+1)/2 (pack_lower, unpack_lower)
    def cov(self, x, out=None, accumulate=False, stream=None):
        """Pooled co-moments of the chains in x [K, W], K <= DENSE_MAX_D (chains with a non-finite value are excluded): (count [1], mean [K],
        m2 [K(K+1)/2] packed = Σ(x_i − mean_i)(x_j − mean_j)), device tensors. out=(count, mean, m2): write into these; with accumulate=True
        Chan-merge this call's block into what they hold. Asynchronous on `stream`."""
        K, W, ld = chain_matrix(x, None, self.device, "cov", "x")
        P = K * (K + 1) // 2
        if accumulate and out is None:
            raise ValueError("cov: accumulate=True needs out=(count, mean, m2)")
        if out is None:
            cnt, mean, m2 = self._out(1), self._out(K), self._out(P)
        else:
            cnt, mean, m2 = out
            if cnt.shape != (1,) or mean.shape != (K,) or m2.shape != (P,) or not (cnt.is_contiguous() and mean.is_contiguous() and m2.is_contiguous()):
                raise ValueError(f"cov: out must be contiguous (count [1], mean [{K}], m2 [{P}])")
        self._check(self.lib.octo_draws_cov_device(self._h, W, ld, K, x.data_ptr(), 1 if accumulate else 0, cnt.data_ptr(), mean.data_ptr(), m2.data_ptr(),
                                                   self._stream(stream, self.device)))
        self._keep = (x,)
        return cnt, mean, m2

    def metric_dense(self, count, m2, chol, regularize=True, info=None, stream=None):
        """The packed Cholesky factor L of the covariance of cov's (count [1], m2 [K(K+1)/2]) into chol [K(K+1)/2] (written only where the
        factorisation holds): M2/(n − 1), with regularize Stan's shrinkage towards 1e-3·I. Returns (chol, info int32 [1]): info = 0, or j + 1 where
        pivot j was not finite and > 0 (n < 2: 1) and chol is untouched. Nothing is read back."""
        import torch
        P = int(m2.numel())
        K = int((np.sqrt(8 * P + 1) - 1) / 2 + 0.5)
        for t, n in ((count, 1), (m2, K * (K + 1) // 2), (chol, P)):
            if t.dtype != torch.float64 or t.device != self.device or t.numel() != n or not t.is_contiguous():
                raise ValueError("metric_dense: count [1], m2 [K(K+1)/2] and chol [K(K+1)/2] must be contiguous float64 tensors on the handle's device")
        if info is None:
            info = self._out(1, dtype=torch.int32)
        self._check(self.lib.octo_draws_metric_dense_device(self._h, K, count.data_ptr(), m2.data_ptr(), 1 if regularize else 0, chol.data_ptr(),
                                                            info.data_ptr(), self._stream(stream, self.device)))
        self._keep = (count, m2, chol, info)
        return chol, info

    def metric_apply(self, chol, x, transpose=False, out=None, stream=None):
        """L·x (transpose=False) or Lᵀ·x of the columns of x [D, n] with the packed factor chol [D(D+1)/2]; out: a tensor of x's layout, x itself
        for the product in place, None for a new one. Returns out."""
        import torch
        dev = self.device
        D = self.D
        _, n, ld = chain_matrix(x, D, dev, "metric_apply", "x")
        if chol.dtype != torch.float64 or chol.device != dev or chol.numel() != D * (D + 1) // 2 or not chol.is_contiguous():
            raise ValueError("metric_apply: chol must be a contiguous float64 [D(D+1)/2] tensor on the handle's device")
        if out is None:
            out = self._out(n, D, ld)
        elif chain_matrix(out, D, dev, "metric_apply", "out") != (D, n, ld):
            raise ValueError("metric_apply: out must have x's shape and leading dimension")
        self._check(self.lib.octo_draws_metric_apply_device(self._h, n, ld, chol.data_ptr(), 1 if transpose else 0, x.data_ptr(), out.data_ptr(),
                                                            self._stream(stream, dev)))
        self._keep = (chol, x, out)
        return out

    def use_metric(self, chol):
        """octo_draws_use_metric: from the next call on hmc_step and nuts take the dense metric L·Lᵀ of the packed factor chol [D(D+1)/2] (and refuse
        an inv_mass); None returns to the per-call diagonal metric. The handle keeps the tensor alive while it is set. Also a context manager:
        `with pd.use_metric(chol): …` sets None on leaving."""
        import torch
        if chol is not None and (chol.dtype != torch.float64 or chol.device != self.device or chol.numel() != self.D * (self.D + 1) // 2 or not chol.is_contiguous()):
            raise ValueError("use_metric: chol must be a contiguous float64 [D(D+1)/2] tensor on the handle's device, or None")
        self._check(self.lib.octo_draws_use_metric(self._h, ptr(chol)))
        self._active_metric = chol
        return _MetricScope(self)

    def adapt_init(self, G, eps0, state=None, stream=None):
        """The dual-averaging state [G, 4] = (log ε, log ε̄, H̄, μ) started at eps0 (a number, or one value per group); state: written in place."""
        import torch
        G = int(G)
        per_group = torch.is_tensor(eps0) or np.ndim(eps0) > 0
        e = device_vector(eps0, G, self.device, "eps0") if per_group else None
        if state is None:
            state = self._out(4, G)
        elif not is_adapt_state(state, G, self.device):
            raise ValueError(f"adapt_init: state must be a contiguous float64 [{G}, 4] tensor on {self.device}")
        self._check(self.lib.octo_draws_hmc_adapt_init_device(self._h, G, ptr(e), 0.0 if per_group else float(eps0), state.data_ptr(),
                                                              self._stream(stream, self.device)))
        self._keep = (e, state)
        return state

    def adapt_step(self, state, dH, accepted, k, group=None, delta=0.8, gamma=0.05, t0=10.0, kappa=0.75, use_average=False, eps_w=None, want_eps=True,
                   stream=None):
        """Dual-averaging update number k >= 1 of `state` [G, 4] (in place) from a step's dH [W] and accepted int32 [W]; group: int32 [W] ids or
        None (G = 1). Returns (accept_stat [G], the mean of min(1, exp(dH)) per group, NaN for an empty one; eps_w [W], ε — with use_average
        ε̄ — of every chain's group, what hmc_step takes as eps; None with want_eps=False). eps_w: written in place where a chain has a group."""
        import torch
        dev = self.device
        W, G = int(dH.numel()), int(state.shape[0])
        if dH.dtype != torch.float64 or accepted.dtype != torch.int32 or accepted.numel() != W or not (dH.is_contiguous() and accepted.is_contiguous()) \
                or not is_adapt_state(state, G, dev) or dH.device != dev or accepted.device != dev:
            raise ValueError(f"adapt_step: dH float64 [W], accepted int32 [W] and state float64 [G, 4], contiguous on {dev}")
        g = group_ids(group, W, dev, "adapt_step")
        a = self._out(G)
        if eps_w is None and want_eps:
            eps_w = self._out(W)
        self._check(self.lib.octo_draws_hmc_adapt_device(self._h, W, ptr(g), G, dH.data_ptr(), accepted.data_ptr(), int(k), float(delta), float(gamma), float(t0),
                                                         float(kappa), state.data_ptr(), a.data_ptr(), 1 if use_average else 0, ptr(eps_w), self._stream(stream, dev)))
        self._keep = (state, dH, accepted, g, eps_w)
        return a, eps_w

    def chain_moments(self, x, k, cmean, cm2, stream=None):
        """Sample number k >= 1 of every chain's running moments over time: cmean, cm2 [K, W] of x's shape and leading dimension, in place
        (k = 1 starts them). R̂ follows from two moments calls on them (include/octofitter_hip_draws.h)."""
        K, W, ld = chain_matrix(x, None, self.device, "chain_moments", "x")
        for t, name in ((cmean, "cmean"), (cm2, "cm2")):
            if chain_matrix(t, None, self.device, "chain_moments", name) != (K, W, ld):
                raise ValueError(f"chain_moments: {name} must have x's shape and leading dimension")
        self._check(self.lib.octo_draws_chain_moments_device(self._h, W, ld, K, int(k), x.data_ptr(), cmean.data_ptr(), cm2.data_ptr(), self._stream(stream, self.device)))
        self._keep = (x, cmean, cm2)
        return cmean, cm2

    # ---- convergence diagnostics of stored draws (include/octofitter_hip_draws.h, "Convergence diagnostics"): K = the rows of x, no model needed
    def diagnose(self, x, out=None, stream=None):
        """Rank-normalised split-R̂, bulk and tail ESS, the basic pair and three quantiles of every row of the stored draws x [n, K, W] (or
        [n, W]: one row), n >= 8; its strides give ld and ls. out: a contiguous float64 [DIAG_N_STATS, K] tensor to write into.
        Returns a dict of [K] device tensors by DIAG_NAMES (rows of one tensor). Asynchronous on `stream`."""
        import torch
        x, n, K, W, ld, ls = draw_cube(x, self.device, "diagnose")
        if out is None:
            out = self._out(K, DIAG_N_STATS)
        elif out.dtype != torch.float64 or out.device != self.device or out.shape != (DIAG_N_STATS, K) or not out.is_contiguous():
            raise ValueError(f"diagnose: out must be a contiguous float64 [{DIAG_N_STATS}, {K}] tensor on {self.device}")
        self._check(self.lib.octo_draws_diagnose_device(self._h, n, W, ld, ls, K, x.data_ptr(), out.data_ptr(), self._stream(stream, self.device)))
        self._keep = (x, out)
        return dict(zip(DIAG_NAMES, out))

    def ranks(self, x, fold=False, z=True, stream=None):
        """The rank step of diagnose alone: (r, z) of x's shape and strides — the average rank of every used draw among its row's (fold: of
        |x − median|) and its normal score; z=False: (r, None). NaN in an unused middle sample and in an invalid row. Asynchronous on `stream`."""
        import torch
        cube, n, K, W, ld, ls = draw_cube(x, self.device, "ranks")
        r, zs = (torch.empty_strided(x.shape, x.stride(), dtype=torch.float64, device=self.device).fill_(float("nan")) if want else None for want in (True, z))
        self._check(self.lib.octo_draws_rank_device(self._h, n, W, ld, ls, K, cube.data_ptr(), 1 if fold else 0, r.data_ptr(), ptr(zs),
                                                    self._stream(stream, self.device)))
        self._keep = (cube,)
        return r, zs

    # ---- parallel tempering between the scans (include/octofitter_hip_draws.h, "Parallel tempering between the scans"): no model needed
    def pt_state(self, T, Cn):
        """The state of pt_stats before its first call, for T temperatures and Cn chains: dict(acc float64 [T − 1, 8] (every m = −Inf, the rest
        0), leg int32 [Cn, T], restarts int32 [Cn]), device tensors."""
        import torch
        T, Cn = int(T), int(Cn)
        if not (2 <= T <= MAX_GROUPS and Cn >= 1):
            raise ValueError(f"pt_state: T is 2 … {MAX_GROUPS}, Cn >= 1")
        acc = torch.zeros((T - 1, 8), dtype=torch.float64, device=self.device)
        acc[:, 3] = acc[:, 6] = -float("inf")
        return dict(acc=acc, leg=torch.zeros((Cn, T), dtype=torch.int32, device=self.device), restarts=torch.zeros(Cn, dtype=torch.int32, device=self.device))

    def _pt_acc(self, state, T, what):
        import torch
        acc = state["acc"]
        if acc.dtype != torch.float64 or acc.device != self.device or acc.shape != (T - 1, 8) or not acc.is_contiguous():
            raise ValueError(f"{what}: state['acc'] must be a contiguous float64 [{T - 1}, 8] tensor on {self.device} (pt_state makes it)")
        return acc

    def pt_stats(self, ll, slot2rep, beta, state, stream=None):
        """One scan's statistics, accumulated into `state` (pt_state's dict, in place; returned): per pair of neighbouring slots the swap
        acceptance probabilities and the two stepping-stone sums over every chain, and — unless state["leg"] is None — the tempered restarts.
        ll: float64 [T·Cn] or [T, Cn] by replica; slot2rep: int32 [Cn, T]; beta: float64 [T] — TemperedSwap's three, as the swap step is about
        to see them. Asynchronous on `stream`."""
        import torch
        dev = self.device
        Cn, T = (int(n) for n in slot2rep.shape)
        ok = ll.dtype == torch.float64 and ll.numel() == T * Cn and ll.is_contiguous() and slot2rep.dtype == torch.int32 and slot2rep.is_contiguous() \
            and beta.dtype == torch.float64 and beta.shape == (T,) and beta.is_contiguous() and ll.device == dev and slot2rep.device == dev and beta.device == dev
        if not ok:
            raise ValueError(f"pt_stats: ll float64 [T·Cn], slot2rep int32 [Cn, T] and beta float64 [T], contiguous on {dev}")
        acc = self._pt_acc(state, T, "pt_stats")
        leg, rst = state.get("leg"), state.get("restarts")
        if (leg is None) != (rst is None) or (leg is not None and not (leg.dtype == rst.dtype == torch.int32 and leg.shape == (Cn, T) and rst.shape == (Cn,)
                                                                        and leg.is_contiguous() and rst.is_contiguous() and leg.device == dev and rst.device == dev)):
            raise ValueError(f"pt_stats: state['leg'] int32 [Cn, T] and state['restarts'] int32 [Cn], contiguous on {dev}, or both None")
        self._check(self.lib.octo_draws_pt_stats_device(self._h, T, Cn, ll.data_ptr(), slot2rep.data_ptr(), beta.data_ptr(), acc.data_ptr(), ptr(leg), ptr(rst),
                                                        self._stream(stream, dev)))
        self._keep = (ll, slot2rep, beta, state)
        return state

    def pt_schedule(self, state, beta, adapt=True, reset=True, beta_out=None, stream=None):
        """A round's summary of `state` and the ladder that equalises the rejection rates along the barrier. beta: float64 [T]; beta_out: where
        the ladder goes (default: a new tensor; beta itself may be given). adapt=False: statistics only, β copied through; reset: state["acc"]
        is put back to zero once read (leg and restarts go on). Returns dict(beta [T], rejection [T − 1], summary [4], and its entries barrier,
        log_evidence_fwd, log_evidence_rev, log_evidence as 0-d views), device tensors. Waits for `stream` once: β is checked on the host."""
        import torch
        dev = self.device
        T = int(beta.numel())
        if beta.dtype != torch.float64 or beta.device != dev or beta.ndim != 1 or not beta.is_contiguous():
            raise ValueError(f"pt_schedule: beta must be a contiguous float64 [T] tensor on {dev}")
        acc = self._pt_acc(state, T, "pt_schedule")
        if beta_out is None:
            beta_out = self._out(T)
        elif beta_out.dtype != torch.float64 or beta_out.device != dev or beta_out.shape != (T,) or not beta_out.is_contiguous():
            raise ValueError(f"pt_schedule: beta_out must be a contiguous float64 [{T}] tensor on {dev}")
        rej, summary = self._out(max(T - 1, 0)), self._out(len(PT_SUMMARY))
        self._check(self.lib.octo_draws_pt_schedule_device(self._h, T, acc.data_ptr(), beta.data_ptr(), 1 if adapt else 0, 1 if reset else 0, beta_out.data_ptr(),
                                                           rej.data_ptr(), summary.data_ptr(), self._stream(stream, dev)))
        self._keep = (state, beta, beta_out)
        return dict(beta=beta_out, rejection=rej, summary=summary, **dict(zip(PT_SUMMARY, summary)))

    # ---- the variational reference of a tempering leg (include/octofitter_hip_draws.h, "The variational reference of a tempering leg"): no model needed
    def reference_table(self):
        """An empty reference table for this handle's D on its device: float64 [octo_draws_reference_doubles(D)]. Its first reference_set or
        reference_fit must be clean (bad = 0): a coordinate never written is no prior."""
        import torch
        return torch.zeros(int(self.lib.octo_draws_reference_doubles(self.D)), dtype=torch.float64, device=self.device)

    def _reference(self, ref, what, none_ok=False):
        import torch
        if ref is None and none_ok:
            return None
        if ref is None or ref.dtype != torch.float64 or ref.device != self.device or ref.ndim != 1 or not ref.is_contiguous() \
                or ref.numel() != int(self.lib.octo_draws_reference_doubles(self.D)):
            raise ValueError(f"{what}: ref must be the contiguous float64 tensor reference_table() makes, on {self.device}")
        return ref

    def reference_set(self, ref, mean, sd, bad=None, stream=None):
        """The table of N(mean_d, sd_d) on θ_t written into `ref` (in place): mean, sd float64 [D]. A coordinate with a non-finite mean or sd, or
        sd <= 0, keeps what it had. Returns the device tensor bad int32 [1], their number (bad=: written into it). Asynchronous on `stream`."""
        import torch
        self._reference(ref, "reference_set")
        mu, sg = (device_vector(t, self.D, self.device, "reference_set") for t in (mean, sd))
        bad = self._out(1, dtype=torch.int32) if bad is None else bad
        self._check(self.lib.octo_draws_reference_set_device(self._h, mu.data_ptr(), sg.data_ptr(), ref.data_ptr(), bad.data_ptr(), self._stream(stream, self.device)))
        self._keep = (ref, mu, sg, bad)
        return bad

    def reference_fit(self, ref, count, mean, m2, inflate=1.0, bad=None, stream=None):
        """The table fitted to ONE group's moments (count [1], mean [D], m2 [D]: rows of moments' outputs), written into `ref` in place:
        μ = mean, σ = inflate·√(M2/(n − 1)). With n < 2 every coordinate is bad and the table keeps what it had. Returns bad int32 [1]."""
        import torch
        self._reference(ref, "reference_fit")
        for t, n in ((count, 1), (mean, self.D), (m2, self.D)):
            if t.dtype != torch.float64 or t.device != self.device or t.numel() != n or not t.is_contiguous():
                raise ValueError("reference_fit: count [1], mean [D] and m2 [D] must be contiguous float64 tensors on the handle's device")
        bad = self._out(1, dtype=torch.int32) if bad is None else bad
        self._check(self.lib.octo_draws_reference_fit_device(self._h, count.data_ptr(), mean.data_ptr(), m2.data_ptr(), float(inflate), ref.data_ptr(),
                                                             bad.data_ptr(), self._stream(stream, self.device)))
        self._keep = (ref, count, mean, m2, bad)
        return bad

    def reference_moments(self, ref):
        """(μ [D], σ [D]) of the table `ref`: views of its last two parts."""
        self._reference(ref, "reference_moments")
        return ref[-2 * self.D:-self.D], ref[-self.D:]

    def use_reference(self, ref):
        """octo_draws_use_reference: from the next call on the handle reads `ref` in place of its priors; None restores them. The handle keeps
        the tensor alive while it is active."""
        self._reference(ref, "use_reference", none_ok=True)
        self._check(self.lib.octo_draws_use_reference(self._h, ptr(ref)))
        self._active_reference = ref

    @contextlib.contextmanager
    def reference(self, ref):
        """with pd.reference(ref): every call inside reads the table `ref`; on leaving, what was active before is active again. None: the
        handle's own priors (a leg that has no reference yet takes the same code path)."""
        before = getattr(self, "_active_reference", None)
        self.use_reference(ref)
        try:
            yield self
        finally:
            self.use_reference(before)

    def reference_exchange(self, slot2rep_a, theta_a, lp_a, ll_a, ref_a, slot2rep_b, theta_b, lp_b, ll_b, ref_b, stream=None):
        """The exchange of two legs' target replicas, in place: per leg slot2rep int32 [Cn, T], theta_t float64 [D, >= T·Cn] (rows contiguous), ℓπ
        and the swap potential float64 [>= T·Cn] by replica, and its reference table (None: the handle's own prior). The two legs' Cn agree.
        Asynchronous on `stream`."""
        import torch
        dev = self.device
        legs = []
        for s2r, th, lp, ll, ref, name in ((slot2rep_a, theta_a, lp_a, ll_a, ref_a, "a"), (slot2rep_b, theta_b, lp_b, ll_b, ref_b, "b")):
            if s2r.dtype != torch.int32 or s2r.ndim != 2 or s2r.device != dev or not s2r.is_contiguous():
                raise ValueError(f"reference_exchange: slot2rep_{name} must be a contiguous int32 [Cn, T] tensor on {dev}")
            Cn, T = (int(n) for n in s2r.shape)
            _, cols, ld = chain_matrix(th, self.D, dev, "reference_exchange", f"theta_{name}")
            for t, what in ((lp, "lp"), (ll, "ll")):
                if t.dtype != torch.float64 or t.device != dev or t.ndim != 1 or not t.is_contiguous() or t.numel() < T * Cn:
                    raise ValueError(f"reference_exchange: {what}_{name} must be a contiguous float64 tensor of at least T·Cn values on {dev}")
            if cols < T * Cn:
                raise ValueError(f"reference_exchange: theta_{name} holds fewer than T·Cn columns")
            legs.append((Cn, T, s2r, ld, th, lp, ll, self._reference(ref, "reference_exchange", none_ok=True)))
        (Cn, T_a, s_a, ld_a, th_a, p_a, l_a, r_a), (Cn_b, T_b, s_b, ld_b, th_b, p_b, l_b, r_b) = legs
        if Cn != Cn_b:
            raise ValueError("reference_exchange: the two legs must hold the same number of chains")
        self._check(self.lib.octo_draws_reference_exchange_device(self._h, Cn, T_a, s_a.data_ptr(), ld_a, th_a.data_ptr(), p_a.data_ptr(), l_a.data_ptr(), ptr(r_a),
                                                                  T_b, s_b.data_ptr(), ld_b, th_b.data_ptr(), p_b.data_ptr(), l_b.data_ptr(), ptr(r_b),
                                                                  self._stream(stream, dev)))
        self._keep = tuple(x for leg in legs for x in leg[2:])

    def close(self):
        if getattr(self, "_h", None) and self.model is not None and not getattr(self.model.ln_like, "_ctx", None):
            self.lib.octo_draws_detach(self._h)      # the model was closed first: its context is gone
        super().close()
        if getattr(self, "_own_ctx", None):
            capi.load_library().octo_ctx_destroy(self._own_ctx)
            self._own_ctx = None
