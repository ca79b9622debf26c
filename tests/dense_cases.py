"""
The inputs and bars the suites of the dense metric share (tests/test_dense_reference.py on the CPU, tests/test_dense.py on the device), on top of
tests/draws_cases.py: the deterministic test factor, the seeds tests/test_dense_reference.py found on the restatement alone, and the restatement's
own sensitivity to one ulp of the starts. A plain module, not a conftest and not a test module.
"""
import functools

import numpy as np

import dense_reference as dref
import draws_cases as cases
import hmc_reference as ref

RHO = 0.6


def factor_of(inv_mass, rho=RHO):
    """L [D, D] lower with L·Lᵀ = S·C·S, S = diag(√inv_mass), C_ij = ρ^|i − j| (positive definite for every D), in closed form:
    the factor of C is ρ^(i − j)·(1 for j = 0, √(1 − ρ²) otherwise)."""
    im = np.asarray(inv_mass, dtype=np.float64)
    D = im.size
    i, j = np.indices((D, D))
    with np.errstate(over="ignore"):
        Lc = np.where(i >= j, rho ** np.maximum(i - j, 0) * np.where(j == 0, 1.0, np.sqrt(1.0 - rho * rho)), 0.0)
    return np.sqrt(im)[:, None] * Lc


def diagonal_factor(inv_mass):
    """L = diag(√inv_mass): the dense path of the diagonal metric"""
    return np.diag(np.sqrt(np.asarray(inv_mass, dtype=np.float64)))


# ---------------------------------------------------------------------------------------------------- one HMC step
STEP_W, STEP_LD = 65, 72
STEP_LEAPFROGS = (1, 4)


def step_inputs():
    """(β, ε, L) of the one-step comparison: draws_cases.step_inputs at W = 65 with the correlated factor of its inv_mass"""
    beta, eps, im = cases.step_inputs(STEP_W)
    return beta, eps, factor_of(im)


def step_prior_inputs():
    """(ε, L) of the same on the prior-only handle of STAT_PRIORS"""
    return 0.2 + 0.1 * (np.arange(STEP_W) % 5), factor_of(cases.STAT_INV_MASS)


# ---------------------------------------------------------------------------------------------------- NUTS
# The one-transition and the deep case of draws_cases (ONE_*: W = 65, ld = 72, depth 4; DEEP_*: depth 10, ε by DEEP_SCALES) under the correlated
# factor of their inv_mass. ONE_STEP_DENSE and DEEP_STEP_DENSE are the first of ONE_STEP, ONE_STEP + 1, … at which the restatement meets the
# conditions of check_one_transition_is_decided and check_deep_transition_is_decided (tests/test_dense_reference.py holds them there).
ONE_STEP_DENSE = cases.ONE_STEP
DEEP_STEP_DENSE = cases.ONE_STEP + 1


def one_transition(oracle, start, form="textbook", L=None):
    beta, eps, im = cases.one_inputs(start.shape[1])
    return dref.nuts_transition_dense(cases.MODEL_PRIORS, start, beta, eps, factor_of(im) if L is None else L, cases.ONE_DEPTH, cases.ONE_SEED, ONE_STEP_DENSE,
                                      logpost=cases.oracle_logpost(oracle, cases.oracle_model(oracle)), form=form)


def deep_transition(oracle, start, form="textbook"):
    beta, eps, im = cases.deep_inputs(start.shape[1])
    return dref.nuts_transition_dense(cases.MODEL_PRIORS, start, beta, eps, factor_of(im), cases.DEEP_DEPTH, cases.ONE_SEED, DEEP_STEP_DENSE,
                                      logpost=cases.oracle_logpost(oracle, cases.oracle_model(oracle)), form=form)


def model_start(W=cases.ONE_W):
    """the starts of the two cases: prior draws 0 … W − 1 of ONE_SEED, as the device's pd.sample(ONE_SEED, 0, W) gives them"""
    return ref.prior_sample(cases.MODEL_PRIORS, cases.ONE_SEED, np.arange(W, dtype=np.uint64))[1]


# The largest deviation (draws_cases.transition_deviation) between two runs of the textbook restatement whose starts differ by one ulp in every
# coordinate, measured by tests/test_dense_reference.py::test_sensitivity_to_one_ulp, which holds the constants to what it measures. The device is
# held to max(1e-8, 100·s), as the diagonal deep case is to DEEP_S.
ONE_S = 1.46e-12      # measured: 1.453e-12
DEEP_S = 4.51e-11     # measured: 4.505e-11
ONE_BAR = max(1e-8, 100 * ONE_S)
DEEP_BAR = max(1e-8, 100 * DEEP_S)


def dim_transition(D, form="textbook"):
    """the prior-only cases of draws_cases.dim_inputs (D = 1 and 64, depth 7) under the correlated factor: (priors, start, ε, L, result)"""
    priors = cases.dim_priors(D)
    eps, im = cases.dim_inputs(D)
    L = factor_of(im)
    start = ref.prior_sample(priors, cases.DIM_SEED, np.arange(cases.DIM_W, dtype=np.uint64))[1]
    return priors, start, eps, L, dref.nuts_transition_dense(priors, start, None, eps, L, cases.DIM_DEPTH, cases.DIM_SEED, cases.DIM_STEP, form=form)


# ---------------------------------------------------------------------------------------------------- the prior is stationary
# STAT_W exact prior draws through STAT_STEPS dense HMC steps (STAT_SETTINGS[0]) and through STAT_STEPS NUTS transitions of depth NUTS_STAT_DEPTH
# (NUTS_STAT_EPS[0]) under the correlated factor of STAT_INV_MASS: KS per coordinate under STAT_BAR. The seeds are the first two of 21, 22, … for
# which the restatement stays under the bar (tests/test_dense_reference.py), as FROZEN_SEEDS were chosen.
STAT_SEEDS_HMC = (21, 22)
STAT_SEEDS_NUTS = (21, 22)


def stationary_factor():
    return factor_of(cases.STAT_INV_MASS)


# ---------------------------------------------------------------------------------------------------- the co-moments
COV_W = (1, 63, 64, 65, 257, 1000)      # a partial wave, a wave edge, a partial block, several blocks
COV_K = (1, 2, 11, 64)


@functools.lru_cache(maxsize=None)
def cov_case(W, K):
    """(x [K][W], its exact co-moments) of draws_cases.moments_case(W, K, 1) — a NaN and an Inf chain, row 0 with mean 5e4 and deviation 0.5 —
    computed once, shared, never modified"""
    x, _ = cases.moments_case(W, K, 1)
    exact = dref.exact_cov(x)
    for a in (x, *exact):
        a.setflags(write=False)
    return x, exact


def check_cov(got, exact, what):
    """counts exact; the mean under check_moments' bar; |M2_ij − exact| <= 1e-10·√(exact_ii·exact_jj) — the error of either form is O(n·2⁻⁵³) of
    Σ|dx_i·dx_j|, which Cauchy-Schwarz bounds by that scale"""
    cnt, mean, m2 = (np.asarray(t, dtype=np.float64) for t in got)
    ecnt, emean, em2, amax = exact
    K = emean.size
    assert np.array_equal(cnt, ecnt), (what, cnt, ecnt)
    assert np.all(np.abs(mean - emean) <= ecnt[0] * cases.U * amax), (what, "mean")
    diag = em2[[i * (i + 1) // 2 + i for i in range(K)]]
    i, j = np.tril_indices(K)
    scale = np.sqrt(diag[i] * diag[j])
    err = np.abs(m2 - em2)
    assert np.all(err <= cases.M2_BAR * scale), (what, "M2", float(np.max(err / np.where(scale > 0, scale, 1.0))))
