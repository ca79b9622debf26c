"""
Conditions on the NumPy restatement of the NUTS transition (tests/nuts_reference.py) that need no device: the counters of the three new
purposes, the stopping rule against its plainest statement by brute force, the two stationarity conditions of tests/test_hmc_reference.py
with the transition in the step's place (a deliberately wrong sampler fails the same bar), the conditions on the seeds of the one-transition
and deep-transition comparisons of tests/test_nuts.py with the sensitivity that sets the deep one's bar, and the argument checks that need
no device.

A chain is DECIDED if the smallest margin of any decision it made exceeds MARGIN = 1e-6 (the bar of the L-BFGS tests): two computations that
differ in the last bits then make the same decisions, and tests compare decisions on decided chains only.
"""
import ctypes as C

import numpy as np
import pytest

import draws_cases as cases
import hmc_reference as ref
import nuts_reference as nuts

MARGIN = nuts.MARGIN


# ---------------------------------------------------------------------------------------------------- the generator
def test_counters_of_purposes_0_to_8_never_coincide():
    """Word 2 of the counter is the purpose. Word 1 is the block of four coordinates for purposes 0 … 5, the doubling j for purposes 6 and 8
    and the leaf number for purpose 7; word 3 is 0 (purposes 0, 1), the step (2, 3, 6, 7, 8), it·32 + k (4) or the draw j (5)."""
    idx, steps = (0, 1, 5, (1 << 40) + 3, ref.M64), (0, 1, 7, ref.M64)
    seen = {}
    for i in idx:
        for blk in range(16):
            for purpose in (ref.PURPOSE_PRIOR, ref.PURPOSE_UNIFORM):
                seen.setdefault(ref.counter(purpose, i, d=4 * blk), set()).add(purpose)
            for step in steps:
                for purpose in (ref.PURPOSE_MOMENTUM, ref.PURPOSE_ACCEPT):
                    seen.setdefault(ref.counter(purpose, i, d=4 * blk, step=step), set()).add(purpose)
                for purpose in (4, 5):      # Pathfinder's two streams: (c, d / 4, purpose, t)
                    seen.setdefault((i, blk, purpose, step), set()).add(purpose)
        for step in steps:
            for j in range(nuts.MAX_DEPTH):
                for purpose in (nuts.PURPOSE_NUTS_DIRECTION, nuts.PURPOSE_NUTS_MERGE):
                    seen.setdefault(nuts.nuts_counter(purpose, i, j, step), set()).add(purpose)
            for leaf in range(1, 1 << nuts.MAX_DEPTH):
                seen.setdefault(nuts.nuts_counter(nuts.PURPOSE_NUTS_LEAF, i, leaf, step), set()).add(nuts.PURPOSE_NUTS_LEAF)
    assert all(len(v) == 1 for v in seen.values())
    assert {next(iter(v)) for v in seen.values()} == set(range(9))
    with pytest.raises(AssertionError):
        nuts.nuts_counter(ref.PURPOSE_ACCEPT, 0, 0, 0)
    # the vector helper uses exactly these counters, and the words differ from the acceptance uniform of the same chain and step
    seed, step, chains = 21, 7, np.array([0, 5, (1 << 40) + 3], dtype=np.uint64)
    for purpose, word1 in ((nuts.PURPOSE_NUTS_DIRECTION, 3), (nuts.PURPOSE_NUTS_LEAF, 1023), (nuts.PURPOSE_NUTS_MERGE, 9)):
        u = nuts.nuts_uniforms(seed, step, chains, np.full(3, word1), purpose)
        for k, c in enumerate(chains):
            word = ref.philox_int((seed, ref.KEY1), nuts.nuts_counter(purpose, c, word1, step))[0]
            assert u[k] == (2 * (word >> 12) + 1) * 2.0 ** -53
    i = np.arange(64, dtype=np.uint64)
    assert not np.any(nuts.nuts_uniforms(5, 0, i, np.zeros(64), nuts.PURPOSE_NUTS_MERGE) == ref.accept_uniforms(5, 0, 0, 64))
    assert not np.any(nuts.nuts_uniforms(5, 0, i, np.zeros(64), nuts.PURPOSE_NUTS_MERGE) == nuts.nuts_uniforms(5, 0, i, np.zeros(64), nuts.PURPOSE_NUTS_DIRECTION))


# ---------------------------------------------------------------------------------------------------- the stopping rule, by brute force
BRUTE_W = 512
BRUTE_SETTINGS = ((0.5, 5), (0.25, 3), (1.6, 4))      # (ε, max_depth): mostly turns · mostly the depth limit · turns at depth 1 and divergences


BRUTE_KEYS = ("depth", "stop", "selected", "n_leapfrog")


def differing_keys(r, b, decided):
    """the compared keys (θ_t: the same bits) under which two results disagree on a decided chain"""
    return [k for k in BRUTE_KEYS if not np.array_equal(r[k][decided], b[k][decided])] + \
        ([] if np.array_equal(r["theta_t"][:, decided], b["theta_t"][:, decided]) else ["theta_t"])


def check_against_brute_force(r, b, tt, max_depth, what):
    decided = r["margin"] > MARGIN
    assert differing_keys(r, b, decided) == [], what
    assert np.array_equal(r["accepted"], r["selected"] != 0) and np.array_equal(r["diverged"], r["stop"] == nuts.STOP_DIVERGED)
    assert np.array_equal(r["theta_t"][:, ~r["accepted"]], tt[:, ~r["accepted"]])
    assert r["rounds"] <= (1 << max_depth) - 1 and np.all(r["n_leapfrog"] <= (1 << max_depth) - 1)
    full = r["stop"] == nuts.STOP_MAX_DEPTH
    assert np.all(r["n_leapfrog"][full] == (1 << max_depth) - 1) and np.all(r["depth"][full] == max_depth)
    return decided


def test_stopping_rule_against_brute_force():
    """The last lines state the gap these settings leave: a sampler whose checkpoint stack holds four planes is the right one on all of them."""
    _, tt = ref.prior_sample(cases.STAT_PRIORS, 5, np.arange(BRUTE_W, dtype=np.uint64))
    reasons = set()
    for eps, max_depth in BRUTE_SETTINGS:
        r = nuts.nuts_transition(cases.STAT_PRIORS, tt, None, eps, cases.STAT_INV_MASS, max_depth, 5, 0)
        b = nuts.nuts_brute_force(cases.STAT_PRIORS, tt, None, eps, cases.STAT_INV_MASS, max_depth, 5, 0)
        decided = check_against_brute_force(r, b, tt, max_depth, eps)
        print(f"ε {eps}, depth <= {max_depth}: {np.sum(~decided)} of {BRUTE_W} chains undecided; stop reasons {np.bincount(r['stop'], minlength=6)[1:]}; "
              f"mean leaves {r['n_leapfrog'].mean():.2f}, rounds {r['rounds']}")
        assert decided.sum() >= 256 and decided.mean() >= 0.95
        reasons |= set(np.unique(r["stop"]))
        short = nuts.nuts_transition(cases.STAT_PRIORS, tt, None, eps, cases.STAT_INV_MASS, max_depth, 5, 0, variant="short_stack")
        assert differing_keys(short, b, decided) == [] and differing_keys(short, r, np.ones(BRUTE_W, dtype=bool)) == [], eps
    assert reasons == {nuts.STOP_MAX_DEPTH, nuts.STOP_TURN_SUBTREE, nuts.STOP_TURN_TREE, nuts.STOP_DIVERGED}


def test_stopping_rule_against_brute_force_to_depth_10():
    """cases.brute_deep_inputs(): ε from 0.004 to 0.3 over 24 chains, so that every depth from 3 to the limit occurs and with it every
    checkpoint slot 0 … 8 (slot popc(n >> 1) of leaf n, subtrees of up to 512 leaves). The sampler with the short stack, which the settings
    above cannot tell from the right one, disagrees here."""
    tt, eps = cases.brute_deep_inputs()
    args = (cases.STAT_PRIORS, tt, None, eps, cases.STAT_INV_MASS, cases.DEEP_DEPTH, cases.BRUTE_DEEP_SEED, 0)
    r, b = nuts.nuts_transition(*args), nuts.nuts_brute_force(*args)
    decided = check_against_brute_force(r, b, tt, cases.DEEP_DEPTH, "deep")
    print(f"ε {eps[0]} … {eps[-1]}, depth <= {cases.DEEP_DEPTH}: {cases.tree_summary(r)}")
    assert set(range(3, cases.DEEP_DEPTH + 1)) <= set(r["depth"][decided]), "condition on the seed"
    assert {nuts.STOP_MAX_DEPTH, nuts.STOP_TURN_SUBTREE, nuts.STOP_TURN_TREE} <= set(r["stop"][decided]), "condition on the seed"
    short = nuts.nuts_transition(*args, variant="short_stack")
    wrong = differing_keys(short, b, decided)
    caught = decided & (short["n_leapfrog"] != b["n_leapfrog"])
    print(f"short stack: disagrees under {wrong}; {caught.sum()} decided chains with another leaf count, all of depth >= {r['depth'][caught].min()}")
    assert wrong != [] and caught.any()
    assert np.all(r["depth"][caught] >= 6)      # a tree of depth <= 5 never shows it
    assert differing_keys(short, b, decided & (r["n_leapfrog"] <= 31)) == []


def test_a_dead_start_ends_at_once():
    _, tt = ref.prior_sample(cases.STAT_PRIORS, 5, np.arange(8, dtype=np.uint64))
    tt[2, 3] = np.nan
    tt[0, 5] = np.inf
    r = nuts.nuts_transition(cases.STAT_PRIORS, tt, None, 0.5, cases.STAT_INV_MASS, 3, 5, 0)
    clean = nuts.nuts_transition(cases.STAT_PRIORS, np.delete(tt, (3, 5), axis=1)[:, :3], None, 0.5, cases.STAT_INV_MASS, 3, 5, 0)
    for c in (3, 5):
        assert r["stop"][c] == nuts.STOP_DEAD and r["n_leapfrog"][c] == 0 and not r["accepted"][c] and np.isnan(r["log_accept"][c])
        assert np.array_equal(r["theta_t"][:, c], tt[:, c], equal_nan=True)
    assert np.array_equal(r["theta_t"][:, :3], clean["theta_t"])      # chains 0 … 2 are what they are without the dead ones


# ---------------------------------------------------------------------------------------------------- β = 0: the prior is stationary
NUTS_WRONG = ("uniform_leaf", 0.8)      # the wrong sampler and the ε it is run at: a subtree's proposal picked with equal weights


def run_stationarity(seed, eps, variant=None):
    _, tt = ref.prior_sample(cases.STAT_PRIORS, seed, np.arange(cases.STAT_W, dtype=np.uint64))
    leaves, used = [], []
    for step in range(cases.STAT_STEPS):
        r = nuts.nuts_transition(cases.STAT_PRIORS, tt, None, eps, cases.STAT_INV_MASS, cases.NUTS_STAT_DEPTH, seed, step, variant=variant)
        tt = r["theta_t"]
        leaves.append(r["n_leapfrog"].mean())
        used.append(r["n_leapfrog"].sum() / (cases.STAT_W * r["rounds"]))
    return cases.stationarity_statistics(tt), float(np.mean(leaves)), float(np.mean(used))


@pytest.mark.parametrize("seed", cases.STAT_SEEDS)
def test_prior_is_stationary_and_a_wrong_sampler_is_not(seed):
    for eps in cases.NUTS_STAT_EPS:
        stat, leaves, used = run_stationarity(seed, eps)
        print(f"seed {seed} (ε {eps}): correct       max D_n {stat:.3e} (bar {cases.STAT_BAR:.3e}); mean leaves {leaves:.2f}, lockstep utilisation {used:.3f}")
        assert stat < cases.STAT_BAR, (seed, eps, stat)
    variant, eps = NUTS_WRONG
    bad, leaves, _ = run_stationarity(seed, eps, variant)
    print(f"seed {seed} (ε {eps}): {variant}  max D_n {bad:.3e}; mean leaves {leaves:.2f}")
    assert bad > cases.STAT_BAR, (seed, bad)


# ---------------------------------------------------------------------------------------------------- β = 1: the posterior is stationary
POST_DEPTH = 4


@pytest.mark.parametrize("seed", cases.POST_SEEDS)
def test_posterior_is_stationary(oracle, seed):
    om = cases.oracle_model(oracle)
    a, b = (cases.rejection_batch(oracle, om, seed, first) for first in cases.POST_FIRST)
    im = cases.posterior_inv_mass(b)
    logpost = cases.oracle_logpost(oracle, om)

    def step_fn(tt, step):
        r = nuts.nuts_transition(cases.MODEL_PRIORS, tt, None, cases.POST_EPS, im, POST_DEPTH, seed, step, logpost=logpost)
        return r["theta_t"], r["accepted"]

    cases.check_posterior_stationary(a, b, step_fn, f"seed {seed} (CPU, NUTS)")


# ---------------------------------------------------------------------------------------------------- one transition: the condition on its seed
def test_one_transition_is_decided_for_the_seed(oracle):
    """at the restated prior draws; the device's differ in the last bits"""
    _, start = ref.prior_sample(cases.MODEL_PRIORS, cases.ONE_SEED, np.arange(cases.ONE_W, dtype=np.uint64))
    cases.check_one_transition_is_decided(cases.one_transition(oracle, start))


def test_deep_transition_is_decided_for_the_seed(oracle):
    """cases.deep_inputs(): max_depth = 10 with ε of the one-transition case scaled per chain, at the restated prior draws"""
    _, start = ref.prior_sample(cases.MODEL_PRIORS, cases.ONE_SEED, np.arange(cases.ONE_W, dtype=np.uint64))
    cases.check_deep_transition_is_decided(cases.deep_transition(oracle, start))


def test_deep_transition_sensitivity_to_one_ulp(oracle):
    """Measures cases.DEEP_S: the restatement from starts moved by one ulp in every coordinate, up and down, against the one from the starts
    themselves — the largest deviation of θ_t, ℓπ and log_accept over the chains whose decisions stayed the same. No decided chain may
    change a decision."""
    _, start = ref.prior_sample(cases.MODEL_PRIORS, cases.ONE_SEED, np.arange(cases.ONE_W, dtype=np.uint64))
    r = cases.deep_transition(oracle, start)
    decided = r["margin"] > MARGIN
    s = 0.0
    for moved in (np.nextafter(start, np.inf), np.nextafter(start, -np.inf)):
        r2 = cases.deep_transition(oracle, moved)
        assert differing_keys(r2, r, decided) in ([], ["theta_t"])
        dev, n_same = cases.transition_deviation(r2, r)
        assert n_same >= decided.sum()
        s = max(s, dev)
    print(f"deep transition, starts moved by one ulp: s = {s:.3e} (DEEP_S = {cases.DEEP_S:.3e}, DEEP_BAR = {cases.DEEP_BAR:.3e})")
    assert s <= cases.DEEP_S


# ---------------------------------------------------------------------------------------------------- argument checks without a device
def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made, so these go through the NULL handle, which is refused before anything else; the same
    arguments on a real handle are in tests/test_nuts.py."""
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    build_draws()
    from octofitter_jl_amd.host import draws
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    acc = (C.c_int32 * 4)()
    call = lambda depth, rounds, resume: lib.octo_draws_nuts_device(None, 0, 0, 0, 4, 4, None, None, None, 0.1, None, depth, rounds, resume,      # noqa: E731
                                                                     None, None, None, C.cast(acc, C.c_void_p), None, None, None, None, None)
    assert call(4, 1, 0) == EINVAL and call(0, 1, 0) == EINVAL and call(4, -1, 0) == EINVAL and call(4, 1, 1) == EINVAL
    assert len(draws._SIGS["octo_draws_nuts_device"][1]) == 23
