"""
The NumPy restatement of the slice sampler (tests/slice_reference.py) checked on the CPU, by itself: the words of the counter generator it
consumes; the lockstep state machine against the plain chain-by-chain statement of Neal's figures; stationarity by meaning — exact draws
pushed through transitions stay exact draws (Kolmogorov-Smirnov at the project's 0.1 % bar 1.95/√n) —, with a deliberately wrong sampler
that the same check refuses; and the conditions on the seeds of the GPU suite (tests/test_slice.py): every path is reached and at most
cases.ONE_UNDECIDED of the chains are undecided. No GPU, nothing of the library.
"""
import math

import numpy as np
import pytest
from scipy.stats import norm

import draws_cases as cases
import hmc_reference as ref
import slice_cases as sc
import slice_reference as sl


# ---------------------------------------------------------------------------------------------------- 1. the generator
def test_uniforms_are_words_0_and_1_of_the_stated_counter():
    seed, step = 12345, 7
    for c, j, i in ((0, 0, 0), (3, 5, 1), (1 << 40, 41, 64), (17, 1023 * 64 + 63, 127)):
        words = ref.philox_int((seed, ref.KEY1), sl.slice_counter(c, j, i, step))
        u, u1 = sl.slice_uniforms(seed, step, np.array([c], dtype=np.uint64), np.array([j]), np.array([i]))
        assert u[0] == (2 * (words[0] >> 12) + 1) * 2.0 ** -53 and u1[0] == (2 * (words[1] >> 12) + 1) * 2.0 ** -53
    assert sl.slice_counter(1, 2, 3, 4) == (1, 2 * 128 + 3, 9, 4)


def test_counters_of_an_update_never_coincide_and_purpose_9_is_new():
    seen = {sl.slice_counter(0, j, i, 0)[1] for j in range(200) for i in list(range(0, sl.MAX_DOUBLINGS + 1)) + [64 + s for s in range(sl.MAX_SHRINK)]}
    assert len(seen) == 200 * (sl.MAX_DOUBLINGS + 1 + sl.MAX_SHRINK)
    import nuts_reference as nuts
    import pathfinder_reference as pf
    assert sl.PURPOSE_SLICE not in (ref.PURPOSE_PRIOR, ref.PURPOSE_UNIFORM, ref.PURPOSE_MOMENTUM, ref.PURPOSE_ACCEPT, pf.PURPOSE_ELBO, pf.PURPOSE_PATHFINDER,
                                    nuts.PURPOSE_NUTS_DIRECTION, nuts.PURPOSE_NUTS_LEAF, nuts.PURPOSE_NUTS_MERGE)


# ---------------------------------------------------------------------------------------------------- 2. the lockstep against the plain statement
MIX = (1.0, 0.25, 0.8)      # modes at ∓1, deviation 0.25, weight 0.8 on the left one
MIX_PRIOR = [ref.prior(ref.NORMAL, 0.0, 10.0)]      # β = 1: E = ℓπ, the prior cancels


def mix_logpost(th):
    m, s, wt = MIX
    with np.errstate(all="ignore"):
        return np.logaddexp(math.log(wt) + norm.logpdf(th[0], -m, s), math.log(1 - wt) + norm.logpdf(th[0], m, s)), np.zeros_like(th)


def mix_cdf(x):
    m, s, wt = MIX
    return wt * norm.cdf(x, -m, s) + (1 - wt) * norm.cdf(x, m, s)


def mix_draws(n, seed):
    m, s, wt = MIX
    rng = np.random.Generator(np.random.Philox(key=seed))
    left = rng.random(n) < wt
    return (np.where(left, -m, m) + s * rng.standard_normal(n))[None, :]


@pytest.mark.parametrize("what", ("priors", "per-coordinate", "mixture", "stuck"))
def test_lockstep_is_the_plain_statement(what):
    """the state machine of rounds and phases makes the transition Neal's loops make: the same bits, the same counts"""
    if what == "mixture":
        args = (MIX_PRIOR, mix_draws(400, 3), None, 0.3, 3, 3, sl.MAX_SHRINK, 5, 2)
        kw = dict(logpost=mix_logpost)
    else:
        tt = ref.prior_sample(cases.STAT_PRIORS, 4, np.arange(24, dtype=np.uint64))[1]
        tt[2, 7] = np.nan
        w, shrink = {"priors": (sc.DEFAULT_W, sl.MAX_SHRINK), "per-coordinate": (np.array(sc.PER_WIDTHS), sl.MAX_SHRINK), "stuck": (sc.DEFAULT_W, 2)}[what]
        args, kw = (cases.STAT_PRIORS, tt, None, w, 3, 2, shrink, 5, 2), dict(chain0=100)
    a, b = sl.slice_transition(*args, **kw), sl.slice_plain(*args, **kw)
    for k in ("theta_t", "logpost") + sc.COUNTS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert a["n_expand"].sum() > 0 and a["n_shrink"].sum() > 0
    if what == "stuck":
        assert a["n_stuck"].sum() > 0
    if what == "mixture":
        assert a["test_rejects"].sum() > 0      # the acceptance test's rejection is among what was compared
    if what == "priors":
        assert a["status"][7] == sl.DEAD and a["n_eval"][7] == 0 and np.isnan(a["theta_t"][2, 7])


def test_a_dead_start_ends_at_once_and_a_dead_trial_point_is_outside_the_slice():
    tt = ref.prior_sample(cases.STAT_PRIORS, 4, np.arange(16, dtype=np.uint64))[1]
    tt[0, 3] = np.inf
    r = sl.slice_transition(cases.STAT_PRIORS, tt, None, 100.0, 3, 1, sl.MAX_SHRINK, 1, 0)      # width 100: the interval's ends overflow the links
    assert r["status"][3] == sl.DEAD and r["n_eval"][3] == 0 and r["theta_t"][0, 3] == np.inf
    others = np.arange(16) != 3
    assert np.all(r["status"][others] == sl.DONE) and r["dead_trials"].sum() > 0 and np.all(np.isfinite(r["theta_t"][:, others]))


# ---------------------------------------------------------------------------------------------------- 3. stationarity
STAT_N = 32768
STAT_BAR = 1.95 / math.sqrt(STAT_N)


@pytest.mark.parametrize("w", (0.3, 10.0))
@pytest.mark.parametrize("p", (0, 3))
def test_standard_normal_is_stationary(w, p):
    priors = [ref.prior(ref.NORMAL, 0.0, 1.0)]      # β = 0: the target is the prior
    tt = ref.prior_sample(priors, 17, np.arange(STAT_N, dtype=np.uint64))[1]
    for step in range(4):
        tt = sl.slice_transition(priors, tt, None, w, p, 1, sl.MAX_SHRINK, 17, step)["theta_t"]
    stat = cases.ks_statistic(tt[0], norm.cdf)
    print(f"normal, w {w}, p {p}: D_n {stat:.3e} (bar {STAT_BAR:.3e})")
    assert stat < STAT_BAR


@pytest.mark.parametrize("w", (0.3, 10.0))
@pytest.mark.parametrize("p", (0, 3))
def test_two_mode_mixture_is_stationary(w, p):
    tt = mix_draws(STAT_N, 5)
    for step in range(4):
        tt = sl.slice_transition(MIX_PRIOR, tt, None, w, p, 1, sl.MAX_SHRINK, 11, step, logpost=mix_logpost)["theta_t"]
    stat = cases.ks_statistic(tt[0], mix_cdf)
    print(f"mixture, w {w}, p {p}: D_n {stat:.3e} (bar {STAT_BAR:.3e})")
    assert stat < STAT_BAR


def test_without_the_acceptance_test_the_mixture_is_not_stationary():
    """the check has power: doubling without Neal's acceptance test is not reversible, and twelve transitions at a small width move a visible
    share of the exact draws into the light mode — the same run with the test stays under the bar"""
    stats = {}
    for accept_test in (True, False):
        tt = mix_draws(STAT_N, 5)
        for step in range(12):
            tt = sl.slice_transition(MIX_PRIOR, tt, None, 0.3, 3, 1, sl.MAX_SHRINK, 11, step, logpost=mix_logpost, accept_test=accept_test)["theta_t"]
        stats[accept_test] = cases.ks_statistic(tt[0], mix_cdf)
    print(f"mixture, w 0.3, p 3, twelve transitions: D_n {stats[True]:.3e} with the acceptance test, {stats[False]:.3e} without (bar {STAT_BAR:.3e})")
    assert stats[True] < STAT_BAR < stats[False]


@pytest.mark.parametrize("seed", cases.STAT_SEEDS)
def test_prior_is_stationary(seed):
    """the five priors at β = 0, the setting of the GPU suite at half its chains"""
    n = cases.STAT_W // 2
    tt = ref.prior_sample(cases.STAT_PRIORS, seed, np.arange(n, dtype=np.uint64))[1]
    start = tt.copy()
    for step in range(sc.STAT_TRANSITIONS):
        tt = sc.stat_transition(tt, seed, step)["theta_t"]
    stat, bar = cases.stationarity_statistics(tt), 1.95 / math.sqrt(n)
    moved = float(np.mean(np.all(tt != start, axis=0)))
    print(f"seed {seed}: max D_n {stat:.3e} (bar {bar:.3e}); chains moved in every coordinate {moved:.3f}")
    assert stat < bar and moved > 0.99


# ---------------------------------------------------------------------------------------------------- 4. the seeds of the GPU suite
def test_model_transitions_reach_every_path_for_the_seed(oracle):
    r1 = sc.first_transition(oracle, sc.one_start())
    r2 = sc.second_transition(oracle, r1["theta_t"])
    sc.check_model_transitions(r1, r2)


@pytest.mark.parametrize("name", sc.EDGES)
def test_edges_reach_their_paths_for_the_seed(name):
    sc.check_edge(name, sc.edge_transition(name, sc.edge_start(name)))


def test_a_slice_of_the_chains_is_the_full_batch(oracle):
    """chains 20 … 40 alone, with chain0 = 20, make what they make in the full batch"""
    start = sc.one_start()[:, :64]
    full = sc.first_transition(oracle, start)
    part = sc.first_transition(oracle, start[:, 20:41], chain0=20, beta=sc.one_betas(64)[20:41])
    for k in ("theta_t", "logpost", "loglike") + sc.COUNTS:
        assert np.array_equal(full[k][..., 20:41], part[k]), k
