"""
The inputs, seeds and conditions the two suites of differential evolution share (tests/test_de_reference.py on the CPU, tests/test_de.py on the
device), in the manner of tests/slice_cases.py, on the models, priors and bars of tests/draws_cases.py. A plain module, not a conftest and not
a test module. Every condition here is on the restatement alone (tests/de_reference.py): the CPU suite establishes it for the seeds below, the
GPU suite asserts it again on the population the device holds, before the device is compared.

An individual is DECIDED in a generation if its selection margin |f′ − f_i| / max(1, |f_i|) exceeds de_reference.MARGIN = 1e-6; decisions are
compared on decided individuals only.
"""
import functools
import math

import numpy as np

import draws_cases as cases
import de_reference as de
import hmc_reference as ref

DEFAULT_RADIUS = 8

# ---------------------------------------------------------------------------------------------------- the test model: six generations
MODEL_W, MODEL_LD, MODEL_SEED, MODEL_GEN0, MODEL_GENS = 96, 101, 47, 5, 6      # a wave and a half, a padded leading dimension
MODEL_UNDECIDED = 2                                                            # individuals of MODEL_W, in any generation


def model_start():
    """the population as the restatement draws it (the device's differs in the last bits)"""
    return ref.prior_sample(cases.MODEL_PRIORS, MODEL_SEED, np.arange(MODEL_W, dtype=np.uint64))[1]


@functools.lru_cache(maxsize=None)
def _model_cloud():
    tt = ref.prior_sample(cases.MODEL_PRIORS, MODEL_SEED, np.arange(4096, dtype=np.uint64))[1]
    lo, hi = tt.min(axis=1), tt.max(axis=1)
    lo.setflags(write=False)
    hi.setflags(write=False)      # computed once, shared, never modified
    return lo, hi


def model_bounds(pop):
    """the per-coordinate minimum and maximum of θ_t over prior draws 0 … 4095 and the population: global_search_device's rule"""
    lo, hi = _model_cloud()
    return np.minimum(lo, np.nanmin(pop, axis=1)), np.maximum(hi, np.nanmax(pop, axis=1))


def model_logpost(oracle):
    """logpost(θ_t) -> (ℓπ, ∇ℓπ) of the test model from the oracle's callback on one thread"""
    obs, planets, priors, esrc, nsrc = cases.oracle_model(oracle)
    return lambda th: oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, np.ascontiguousarray(th), grad=True, n_threads=1)


def undecided(rec):
    return int(np.sum(rec["margin"] <= de.MARGIN))


def summary(rec):
    return (f"{undecided(rec)} of {rec['margin'].size} undecided; accepted {int(rec['accepted'].sum())}; crossing {rec['cross'].mean():.2f}, repaired "
            f"{int(rec['repaired'].sum())}; new F {int(rec['new_F'].sum())}, new CR {int(rec['new_CR'].sum())}; dead trials {int(np.sum(rec['f_trial'] == -np.inf))}")


def check_model_generation(g, rec):
    print(f"generation {g}: {summary(rec)}")
    assert undecided(rec) <= MODEL_UNDECIDED, "condition on the seed (the reference alone)"


# ---------------------------------------------------------------------------------------------------- handles without a model: the edges
# name -> (D (5: cases.STAT_PRIORS, otherwise cases.dim_priors), W, radius, bounds ("wide": the population's own range, "narrow": its 40 % and 60 % quantiles, with
# most of the population outside them, None), the individual with a NaN coordinate or None, fcr ("given": drawn pairs, "made": the binding's pair at the
# opening values, None: a NULL pointer), whether the optional outputs are asked for)
EDGE_SEED, EDGE_GEN0, EDGE_GENS = 13, 3, 3
EDGE_UNDECIDED = 0.05
EDGES = {
    "W4": (5, 4, DEFAULT_RADIUS, "wide", None, "made", True),
    "W5": (5, 5, DEFAULT_RADIUS, "wide", None, "made", True),
    "W63": (5, 63, DEFAULT_RADIUS, "wide", None, "given", True),
    "W65": (5, 65, DEFAULT_RADIUS, "wide", None, "made", True),
    "W257": (5, 257, DEFAULT_RADIUS, "wide", 130, "made", True),
    "D1": (1, 65, DEFAULT_RADIUS, "wide", None, "made", True),
    "D64": (64, 65, DEFAULT_RADIUS, "wide", None, "made", True),
    "radius0": (5, 65, 0, "wide", None, "made", True),
    "r8W16": (5, 16, 8, "wide", None, "made", True),
    "r8W17": (5, 17, 8, "wide", None, "made", True),
    "r8W18": (5, 18, 8, "wide", None, "made", True),
    "narrow": (5, 65, DEFAULT_RADIUS, "narrow", None, "made", True),
    "nobounds": (5, 65, DEFAULT_RADIUS, None, None, "made", True),
    "nofcr": (5, 65, DEFAULT_RADIUS, "wide", None, None, True),
    "nooutputs": (5, 65, DEFAULT_RADIUS, "wide", None, None, False),
}


def edge_priors(name):
    D = EDGES[name][0]
    return cases.STAT_PRIORS if D == 5 else cases.dim_priors(D)


def edge_population(name, tt):
    """(population, lo, hi) of a case from prior draws tt [D][W], the restatement's or the device's: the NaN coordinate in place, the bounds from
    the draws"""
    D, _W, _r, bounds, nan_at, _fcr, _outs = EDGES[name]
    tt = np.array(tt, dtype=np.float64)
    lo = hi = None
    if bounds == "wide":
        lo, hi = tt.min(axis=1), tt.max(axis=1)
    elif bounds == "narrow":
        lo, hi = np.quantile(tt, 0.4, axis=1), np.quantile(tt, 0.6, axis=1)
    if nan_at is not None:
        tt[D // 2, nan_at] = np.nan
    return tt, lo, hi


def edge_start(name):
    W = EDGES[name][1]
    return edge_population(name, ref.prior_sample(edge_priors(name), EDGE_SEED, np.arange(W, dtype=np.uint64))[1])


def edge_fcr(name):
    """the pairs of a case that gives them: F in [0.1, 1], CR in (0, 1), from a generator of the case's own"""
    W = EDGES[name][1]
    rng = np.random.default_rng(EDGE_SEED)
    return np.stack([rng.uniform(0.1, 1.0, W), rng.uniform(0.05, 0.95, W)])


def check_edge_generation(name, g, rec):
    print(f"{name}, generation {g}: {summary(rec)}")
    _D, W, _r, bounds, nan_at, _fcr, _outs = EDGES[name]
    assert undecided(rec) <= max(1, math.floor(EDGE_UNDECIDED * W)), "condition on the seed (the reference alone)"
    if bounds == "narrow":
        assert rec["repaired"].sum() > 0.5 * rec["cross"].sum(), name      # most crossing coordinates are repaired
    if bounds is None:
        assert rec["repaired"].sum() == 0
    if nan_at is not None and g == 0:
        assert rec["f_trial"][nan_at] > -np.inf or not rec["accepted"][nan_at]


# ---------------------------------------------------------------------------------------------------- it optimises: eight Normal priors
OPT_PRIORS = [ref.prior(ref.NORMAL, mu, sd) for mu, sd in ((0.0, 1.0), (3.0, 0.5), (-2.0, 2.0), (10.0, 0.1), (0.5, 5.0), (-7.0, 1.5), (1.2, 0.05), (50.0, 20.0))]
OPT_W, OPT_SEED, OPT_GENS = 256, 61, 100      # the restatement's gap: 2e-5 after 75 generations, 5e-7 after 100, 3e-8 after 125
OPT_MAX = float(sum(-math.log(p["p1"]) - 0.5 * math.log(2.0 * math.pi) for p in OPT_PRIORS))      # ℓprior_t at the means: the link is the identity
OPT_GAP, OPT_FACTOR = 1e-6, 10.0


def opt_start():
    return ref.prior_sample(OPT_PRIORS, OPT_SEED, np.arange(OPT_W, dtype=np.uint64))[1]


@functools.lru_cache(maxsize=None)
def opt_reference_gap():
    """the gap to the analytic maximum that the restatement reaches alone after OPT_GENS generations, computed once"""
    s = de.de_open(OPT_PRIORS, opt_start())
    s, _ = de.de_run(OPT_PRIORS, s, OPT_SEED, 0, OPT_GENS, DEFAULT_RADIUS)
    return OPT_MAX - de.best(s)[1]


# ---------------------------------------------------------------------------------------------------- the callers
SEARCH = dict(n_pop=128, N=4096, radius=DEFAULT_RADIUS, max_gen=40, gens_per_call=10, patience=1000, seed=3)
INIT_STARTS = 8
