"""
The inputs, seeds and conditions the two suites of nested sampling share (tests/test_nested_reference.py on the CPU, tests/test_nested.py on
the device), in the manner of tests/slice_cases.py. A plain module, not a conftest and not a test module. Every condition here is on the
restatement alone (tests/nested_reference.py).

A chain is DECIDED if the smallest |ℓ_trial − ℓ*| of its transition exceeds nested_reference.MARGIN = 1e-6 relative to max(1, |ℓ*|); decisions are
compared on decided chains only, and at most cases.ONE_UNDECIDED of a case's chains may be undecided.
"""
import math

import numpy as np

import draws_cases as cases
import nested_reference as nr

COUNTS = ("n_eval", "n_step", "n_shrink", "n_stuck", "status")

# ---------------------------------------------------------------------------------------------------- the cull: synthetic live sets
CULL_K = (2, 63, 64, 65, 257, 1000, 4096)      # the sort's padding: below, at and above powers of two, one block's 1024 lanes and the limit
CULL_B = ("one", "half", "all_but_one", "flush")
CULL_D = (1, 14, 64)
CULL_VARIANTS = ("ties", "neginf", "nan")
CULL_SEED = 77


def cull_batch(K, kind):
    """(B, replace) of a case"""
    return {"one": (1, True), "half": (max(K // 2, 1), True), "all_but_one": (K - 1, True), "flush": (K, False)}[kind]


def cull_dims(K):
    """the D of a case: all three at the limit and at 65, else one of them in turn"""
    return CULL_D if K in (65, 4096) else (CULL_D[CULL_K.index(K) % 3],)


def cull_live(K, D, B, variant):
    """(u_live [D][K], ℓ [K]) of a synthetic live set: ties — a block of equal ℓ straddling rank B (ranks B − 2 … B + 1 where they exist) and a second
    block of three at the top; neginf — more than B entries of −Inf where the set is large enough (a tie block of −Inf straddling rank B); nan — a
    NaN, a −Inf and a +Inf-free finite rest. The slots are shuffled, so that ranks and slots do not coincide."""
    rng = np.random.default_rng([CULL_SEED, K, D, B, CULL_VARIANTS.index(variant)])
    u = rng.uniform(0.0, 1.0, (D, K))
    ll = np.sort(rng.normal(-20.0, 5.0, K))
    if variant == "ties":
        lo, hi = max(B - 2, 0), min(B + 2, K)
        ll[lo:hi] = ll[lo]
        ll[max(K - 3, 0):] = ll[K - 1]
    elif variant == "neginf":
        ll[:min(K - 1, B + 3)] = -math.inf
    else:
        ll[0] = math.nan
        if K > 2:
            ll[1] = -math.inf
    perm = rng.permutation(K)
    return u, ll[perm]


# ---------------------------------------------------------------------------------------------------- the move on the test model
MOVE_K, MOVE_SEED, MOVE_ITER = 320, 61, 5
MOVE_B = (1, 63, 65, 257)
MOVE_STEPS, MOVE_PASSES = 4, 1


def model_loglike(oracle):
    """loglike(u) of the test model from the oracle's callback on one thread (slice_cases.model_logpost explains the thread)"""
    obs, planets, priors, esrc, nsrc = cases.oracle_model(oracle)
    logpost = lambda th: oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, np.ascontiguousarray(th), grad=False, n_threads=1)      # noqa: E731
    return nr.model_loglike(cases.MODEL_PRIORS, logpost)


def move_live(loglike):
    """the live set of the move cases: MOVE_K points of the cube of MOVE_SEED and their ℓ by the restatement (shared by the cases: computed once)"""
    u = nr.cube(MOVE_SEED, 0, MOVE_K, len(cases.MODEL_PRIORS))
    ll = loglike(u)
    u.setflags(write=False)
    ll.setflags(write=False)
    return u, ll


def undecided(r):
    return float(np.mean(r["margin"] <= nr.MARGIN))


def summary(r):
    return (f"{np.sum(r['margin'] <= nr.MARGIN)} of {r['margin'].size} chains undecided; rounds {r['rounds']}; per chain: evaluations {r['n_eval'].mean():.1f}, "
            f"steps out {r['n_step'].mean():.1f}, shrink proposals {r['n_shrink'].mean():.1f}; stuck {r['n_stuck'].sum()}")


# ---------------------------------------------------------------------------------------------------- the analytic evidence
GAUSS_D, GAUSS_SIGMA, GAUSS_SEEDS = 3, 0.05, (1, 2, 3)


def gauss_loglike(u):
    """a normalised Gaussian N(½, σ²) per coordinate on the unit cube (uniform priors on (0, 1)), summed in coordinate order"""
    acc = np.zeros(u.shape[1])
    for d in range(u.shape[0]):
        acc = acc + (-0.5 * ((u[d] - 0.5) / GAUSS_SIGMA) ** 2 - math.log(GAUSS_SIGMA * math.sqrt(2.0 * math.pi)))
    return acc


def gauss_logz(D=GAUSS_D):
    from scipy.special import ndtr
    return D * math.log(ndtr(0.5 / GAUSS_SIGMA) - ndtr(-0.5 / GAUSS_SIGMA))
