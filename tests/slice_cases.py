"""
The inputs, seeds and conditions the two suites of the slice sampler share (tests/test_slice_reference.py on the CPU, tests/test_slice.py on
the device), in the manner of tests/draws_cases.py, whose models, priors and bars they build on. A plain module, not a conftest and not a
test module. Every condition here is on the restatement alone (tests/slice_reference.py): the CPU suite establishes it for the seeds below,
the GPU suite asserts it again on the starts the device drew, before the device runs.

A chain is DECIDED if the smallest margin of any comparison it made exceeds slice_reference.MARGIN = 1e-6; decisions are compared on decided
chains only, and at most cases.ONE_UNDECIDED of a case's chains may be undecided.
"""
import functools

import numpy as np

import draws_cases as cases
import hmc_reference as ref
import slice_reference as sl

DEFAULT_W, DEFAULT_P, DEFAULT_PASSES = 10.0, 3, 3      # Pigeons' SliceSampler defaults, as recalled
OUTPUTS = ("logpost", "loglike", "n_eval", "n_expand", "n_shrink", "n_stuck", "status")
COUNTS = ("n_eval", "n_expand", "n_shrink", "n_stuck", "status")

# ---------------------------------------------------------------------------------------------------- the test model: two transitions
ONE_W, ONE_LD, ONE_SEED, ONE_STEP = 192, 197, 43, 7      # three waves, a partial block, a padded leading dimension
WIDTH_FRACTION = 0.25


def one_betas(W=ONE_W):
    return np.array([cases.ONE_BETAS[w % 3] for w in range(W)])


def one_start():
    """the starts as the restatement draws them (the device's differ in the last bits)"""
    return ref.prior_sample(cases.MODEL_PRIORS, ONE_SEED, np.arange(ONE_W, dtype=np.uint64))[1]


@functools.lru_cache(maxsize=None)
def narrow_widths():
    """WIDTH_FRACTION of the standard deviation of prior draws 0 … 4095 in θ_t, rounded to two digits so that both suites use the same numbers"""
    tt = ref.prior_sample(cases.MODEL_PRIORS, ONE_SEED, np.arange(4096, dtype=np.uint64))[1]
    w = np.array([float(f"{WIDTH_FRACTION * v:.2g}") for v in tt.std(axis=1)])
    w.setflags(write=False)      # computed once, shared, never modified
    return w


def model_logpost(oracle):
    """logpost(θ_t) -> (ℓπ, ∇ℓπ) of the test model from the oracle's callback on one thread: a round is a small batch, and a transition makes
    hundreds of calls (cases.oracle_logpost starts a thread per CPU in each)"""
    obs, planets, priors, esrc, nsrc = cases.oracle_model(oracle)
    return lambda th: oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, np.ascontiguousarray(th), grad=True, n_threads=1)


def first_transition(oracle, start, chain0=0, beta=None):
    """at the defaults, one pass"""
    return sl.slice_transition(cases.MODEL_PRIORS, start, one_betas(start.shape[1]) if beta is None else beta, DEFAULT_W, DEFAULT_P, 1, sl.MAX_SHRINK, ONE_SEED, ONE_STEP,
                               chain0=chain0, logpost=model_logpost(oracle))


def second_transition(oracle, start):
    """narrow widths per coordinate: doubling and the acceptance test run"""
    return sl.slice_transition(cases.MODEL_PRIORS, start, one_betas(start.shape[1]), narrow_widths(), DEFAULT_P, 1, sl.MAX_SHRINK, ONE_SEED, ONE_STEP + 1,
                               logpost=model_logpost(oracle))


def summary(r):
    decided = r["margin"] > sl.MARGIN
    return (f"{np.sum(~decided)} of {decided.size} chains undecided; rounds {r['rounds']}; per chain: evaluations {r['n_eval'].mean():.1f}, doublings {r['n_expand'].mean():.1f}, "
            f"shrink proposals {r['n_shrink'].mean():.1f}; stuck {r['n_stuck'].sum()}; doubling stopped early {r['grow_early'].sum()}, ran out {r['grow_full'].sum()}; "
            f"test rejections {r['test_rejects'].sum()}; dead trial points {r['dead_trials'].sum()}; status {np.bincount(r['status'], minlength=3)}")


def undecided(r):
    return float(np.mean(r["margin"] <= sl.MARGIN))


def check_model_transitions(r1, r2):
    """the conditions on the two transitions of the test model"""
    print(f"first transition: {summary(r1)}")
    print(f"second transition: {summary(r2)}")
    assert undecided(r1) <= cases.ONE_UNDECIDED and undecided(r2) <= cases.ONE_UNDECIDED, "condition on the seed (the reference alone)"
    assert np.all(r1["status"] == sl.DONE) and np.all(r2["status"] == sl.DONE)
    assert r1["dead_trials"].sum() > 0 and r1["grow_early"].sum() > 0                 # wide intervals: ends beyond the support
    assert r2["grow_full"].sum() > 0 and r2["grow_early"].sum() > 0 and r2["n_expand"].sum() > 0 and r2["test_rejects"].sum() > 0


# ---------------------------------------------------------------------------------------------------- handles without a model: the edges
# name -> (D (5: cases.STAT_PRIORS, otherwise cases.dim_priors), W, w (a number, or "per": one width per coordinate), p, n_passes, max_shrink, the
# chain whose start has a NaN coordinate or None, what the restatement has to show; the acceptance test never rejects on these unimodal
# priors: the test model's second transition shows that)
EDGE_SEED, EDGE_STEP = 9, 4
EDGES = {
    "W1": (5, 1, DEFAULT_W, DEFAULT_P, DEFAULT_PASSES, sl.MAX_SHRINK, None, ()),
    "W63": (5, 63, 0.4, 3, 2, sl.MAX_SHRINK, None, ("grow_early", "grow_full")),
    "W65": (5, 65, "per", 3, 2, sl.MAX_SHRINK, None, ("grow_early", "grow_full")),
    "W257": (5, 257, DEFAULT_W, DEFAULT_P, 1, sl.MAX_SHRINK, 130, ("dead_trials", "dead_start")),
    "D1": (1, 65, 0.5, 3, 3, sl.MAX_SHRINK, None, ("grow_early", "grow_full")),
    "D64": (64, 65, 2.0, 2, 1, sl.MAX_SHRINK, None, ("grow_early", "grow_full")),
    "p0": (5, 65, 1.0, 0, 2, sl.MAX_SHRINK, None, ()),
    "shrink2": (5, 65, DEFAULT_W, DEFAULT_P, 2, 2, None, ("n_stuck",)),
}
PER_WIDTHS = (0.8, 0.9, 0.01, 0.7, 0.3)      # about a quarter of the priors' spreads in θ_t


def edge_priors(name):
    D = EDGES[name][0]
    return cases.STAT_PRIORS if D == 5 else cases.dim_priors(D)


def edge_width(name):
    w = EDGES[name][2]
    return np.array(PER_WIDTHS) if isinstance(w, str) else w


def edge_start(name):
    """the starts as the restatement draws them, the NaN coordinate in place"""
    D, W, nan_chain = EDGES[name][0], EDGES[name][1], EDGES[name][6]
    tt = ref.prior_sample(edge_priors(name), EDGE_SEED, np.arange(W, dtype=np.uint64))[1]
    return with_nan(tt, nan_chain, D)


def with_nan(tt, nan_chain, D):
    if nan_chain is not None:
        tt = tt.copy()
        tt[D // 2, nan_chain] = np.nan
    return tt


def edge_transition(name, start, chain0=0):
    _D, _W, _w, p, n_passes, max_shrink, _nan, _shows = EDGES[name]
    return sl.slice_transition(edge_priors(name), start, None, edge_width(name), p, n_passes, max_shrink, EDGE_SEED, EDGE_STEP, chain0=chain0)


def check_edge(name, r):
    print(f"{name}: {summary(r)}")
    assert undecided(r) <= cases.ONE_UNDECIDED, "condition on the seed (the reference alone)"
    nan_chain, shows = EDGES[name][6], EDGES[name][7]
    for what in shows:
        if what == "dead_start":
            assert r["status"][nan_chain] == sl.DEAD and r["n_eval"][nan_chain] == 0 and np.sum(r["status"] == sl.DEAD) == 1, name
        else:
            assert r[what].sum() > 0, (name, what)
    if name == "p0":
        assert r["n_expand"].sum() == 0 and r["test_rejects"].sum() == 0


# ---------------------------------------------------------------------------------------------------- stationarity
STAT_TRANSITIONS = 2      # of the default sampler with one pass each, on cases.STAT_W exact prior draws
STAT_WIDTH = 2.0


def stat_transition(tt, seed, step):
    return sl.slice_transition(cases.STAT_PRIORS, tt, None, STAT_WIDTH, DEFAULT_P, 1, sl.MAX_SHRINK, seed, step)
