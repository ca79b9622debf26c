"""
The restatement of differential evolution (tests/de_reference.py) by itself: the parents it picks, the uniforms it reads, the repair, the
self-adaptation, the selection, and the conditions tests/test_de.py places on its seeds (tests/de_cases.py states them). CPU suite: no GPU,
nothing of the library.
"""
import numpy as np
import pytest

import de_cases as dc
import de_reference as de
import draws_cases as cases
import hmc_reference as ref

CHI2_999 = {1: 10.828, 2: 13.816, 3: 16.266, 4: 18.467, 5: 20.515, 7: 24.322, 13: 34.528, 15: 37.697}      # the 0.1 % points of chi-square


def quadratic(priors):
    """a population and its state on plain Normal priors"""
    tt = ref.prior_sample(priors, 5, np.arange(64, dtype=np.uint64))[1]
    return de.de_open(priors, tt)


@pytest.mark.parametrize("W,radius", [(4, 8), (5, 8), (16, 8), (17, 8), (18, 8), (40, 8), (40, 0), (5, 0), (9, 1), (9, 2)])
def test_parents_are_distinct_members_of_the_neighbourhood_and_never_the_individual(W, radius):
    priors = cases.dim_priors(3)
    s = de.de_open(priors, ref.prior_sample(priors, 1, np.arange(W, dtype=np.uint64))[1])
    n = de.neighbourhood_size(W, radius)
    assert n == (W - 1 if radius == 0 else min(max(2 * radius, 3), W - 1)) and 3 <= n <= W - 1
    i = np.arange(W)
    hood = de.member(i[None, :], np.arange(n)[:, None], n, W)                   # [n][W]
    for w in range(W):
        assert len(set(hood[:, w])) == n and w not in hood[:, w]
        if n < W - 1:                                                           # a ring: within radius on either side
            assert np.all(np.minimum((hood[:, w] - w) % W, (w - hood[:, w]) % W) <= n - n // 2)
    for gen in range(40):
        t = de.de_trial(s, 3, gen, radius)
        p = t["parents"]
        assert np.all((p[0] != p[1]) & (p[0] != p[2]) & (p[1] != p[2]) & (p != i[None, :]))
        assert np.all((t["picks"] >= 0) & (t["picks"] < n))
        assert all(p[k, w] in hood[:, w] for k in range(3) for w in range(W))


def test_uniforms_are_the_words_of_the_stated_counters_and_purpose_12_is_new():
    assert de.PURPOSE_DE == 12
    u = de.de_words(7, 9, np.array([3, 4]), 2)
    for col, i in enumerate((3, 4)):
        words = ref.philox_int((7, ref.KEY1), (i, 2, 12, 9))
        assert np.array_equal(u[:, col], [ref.u01(np.uint64(x)) for x in words])
    assert np.all((u > 0) & (u < 1))
    assert 2 + 63 // 4 < 18 and 18 + 63 // 4 == 33                              # D <= 64: the crossover and the repair blocks do not meet


def test_parent_and_jrand_frequencies_are_uniform():
    """chi-square at the 0.1 % level: each parent slot over the neighbourhood's members (by their offset from the individual), j_rand over D"""
    W, radius, D = 64, 4, 5
    priors = cases.dim_priors(D)
    s = de.de_open(priors, ref.prior_sample(priors, 2, np.arange(W, dtype=np.uint64))[1])
    n = de.neighbourhood_size(W, radius)
    counts, jcount, gens = np.zeros((3, n)), np.zeros(D), 200
    for gen in range(gens):
        t = de.de_trial(s, 11, gen, radius)
        off = (t["parents"] - np.arange(W)[None, :] + n // 2) % W                # 0 … n, the individual's own offset n // 2 left out
        off = off - (off > n // 2)
        for k in range(3):
            counts[k] += np.bincount(off[k], minlength=n)
        jcount += np.bincount(t["jrand"], minlength=D)
    total = gens * W
    for k in range(3):
        assert np.sum((counts[k] - total / n) ** 2 / (total / n)) < CHI2_999[n - 1], (k, counts[k])
    assert np.sum((jcount - total / D) ** 2 / (total / D)) < CHI2_999[D - 1], jcount


def test_a_repaired_coordinate_lies_between_the_bound_and_the_individuals_value():
    name = "narrow"
    tt, lo, hi = dc.edge_start(name)
    s = de.de_open(dc.edge_priors(name), tt)
    t = de.de_trial(s, dc.EDGE_SEED, dc.EDGE_GEN0, dc.DEFAULT_RADIUS, lo, hi)
    r, V, X = t["repaired"], t["trial"], s["theta_t"]
    assert r.sum() > 0.5 * t["cross"].sum() and np.all(t["cross"][r])
    L, H = np.broadcast_to(lo[:, None], V.shape), np.broadcast_to(hi[:, None], V.shape)
    free = de.de_trial(s, dc.EDGE_SEED, dc.EDGE_GEN0, dc.DEFAULT_RADIUS)["trial"]      # the same trial without bounds
    low, high = r & (free < L), r & (free > H)
    assert np.array_equal(low | high, r) and not np.any(low & high)
    assert np.all((V[low] >= np.minimum(L[low], X[low])) & (V[low] <= np.maximum(L[low], X[low])))
    assert np.all((V[high] >= np.minimum(H[high], X[high])) & (V[high] <= np.maximum(H[high], X[high])))
    assert np.array_equal(V[~r], free[~r])                                      # nothing else is touched: the population is not clipped
    inside = (X >= L) & (X <= H)
    assert np.all((V[r & inside] >= L[r & inside]) & (V[r & inside] <= H[r & inside]))      # from inside the bounds, back inside


def test_adapted_parameters_stay_in_range_and_change_at_the_stated_rate():
    s = quadratic(cases.dim_priors(4))
    W, gens = s["f"].size, 300
    nF = nCR = 0
    for gen in range(gens):
        t = de.de_trial(s, 17, gen, dc.DEFAULT_RADIUS)
        assert np.all((t["Ft"] >= 0.1) & (t["Ft"] <= 1.0)) and np.all((t["CRt"] > 0.0) & (t["CRt"] < 1.0))
        assert np.array_equal(t["Ft"][~t["new_F"]], s["F"][~t["new_F"]]) and np.array_equal(t["CRt"][~t["new_CR"]], s["CR"][~t["new_CR"]])
        nF, nCR = nF + t["new_F"].sum(), nCR + t["new_CR"].sum()
    n, sd = gens * W, np.sqrt(gens * W * 0.1 * 0.9)
    assert abs(nF - 0.1 * n) < 4 * sd and abs(nCR - 0.1 * n) < 4 * sd, (nF, nCR, n)
    assert (de.TAU_F, de.F_LOW, de.F_SPAN, de.TAU_CR, de.F0, de.CR0) == (0.1, 0.1, 0.9, 0.1, 0.5, 0.9)


def test_f_never_decreases_and_the_state_follows_the_selection():
    priors = cases.STAT_PRIORS
    tt = ref.prior_sample(priors, 8, np.arange(65, dtype=np.uint64))[1]
    tt[2, 30] = np.nan
    s = de.de_open(priors, tt)
    assert s["f"][30] == -np.inf and de.best(s)[0] == int(np.argmax(s["f"]))
    for gen in range(12):
        s1, rec = de.de_generation(priors, s, 4, gen, dc.DEFAULT_RADIUS)
        acc = rec["accepted"]
        assert np.all(s1["f"] >= s["f"]) and np.array_equal(s1["f"][~acc], s["f"][~acc])
        assert np.array_equal(s1["theta_t"][:, acc], rec["trial"][:, acc]) and np.array_equal(s1["theta_t"][:, ~acc], s["theta_t"][:, ~acc], equal_nan=True)
        assert np.array_equal(s1["F"], np.where(acc, rec["Ft"], s["F"])) and np.array_equal(s1["n_accept"], s["n_accept"] + acc)
        assert not np.any(acc & ~np.isfinite(rec["f_trial"]))                    # a dead trial never wins
        if acc[30]:
            assert np.all(np.isfinite(s1["theta_t"][:, 30]))                     # the NaN individual is replaced only by a finite trial
        s = s1
    assert np.all(np.isfinite(s["theta_t"][:, 30])) and de.best(s)[1] == s["f"].max()
    empty = de.de_open(priors, np.full((5, 4), np.nan))
    assert de.best(empty) == (-1, -np.inf)


def test_a_plus_b_generations_are_one_run():
    priors = cases.STAT_PRIORS
    tt = ref.prior_sample(priors, 8, np.arange(33, dtype=np.uint64))[1]
    lo, hi = tt.min(axis=1), tt.max(axis=1)
    one, _ = de.de_run(priors, de.de_open(priors, tt), 4, 10, 7, 3, lo, hi)
    a, _ = de.de_run(priors, de.de_open(priors, tt), 4, 10, 3, 3, lo, hi)
    b, _ = de.de_run(priors, a, 4, 13, 4, 3, lo, hi)
    assert all(np.array_equal(one[k], b[k]) for k in one)
    other, _ = de.de_run(priors, de.de_open(priors, tt), 4, 11, 7, 3, lo, hi)   # another gen0: other uniforms
    assert not np.array_equal(one["theta_t"], other["theta_t"])


def test_the_model_generations_are_decided_for_the_seed(oracle):
    logpost = dc.model_logpost(oracle)
    pop = dc.model_start()
    lo, hi = dc.model_bounds(pop)
    s = de.de_open(cases.MODEL_PRIORS, pop, logpost)
    first = de.best(s)[1]
    accepted = repaired = 0
    for g in range(dc.MODEL_GENS):
        s, rec = de.de_generation(cases.MODEL_PRIORS, s, dc.MODEL_SEED, dc.MODEL_GEN0 + g, dc.DEFAULT_RADIUS, lo, hi, logpost)
        dc.check_model_generation(g, rec)
        accepted, repaired = accepted + rec["accepted"].sum(), repaired + rec["repaired"].sum()
    assert accepted > dc.MODEL_W and repaired > 0 and de.best(s)[1] >= first


@pytest.mark.parametrize("name", dc.EDGES)
def test_edges_are_decided_for_the_seed(name):
    priors = dc.edge_priors(name)
    tt, lo, hi = dc.edge_start(name)
    s = de.de_open(priors, tt, fcr=dc.edge_fcr(name) if dc.EDGES[name][5] == "given" else None)
    for g in range(dc.EDGE_GENS):
        s, rec = de.de_generation(priors, s, dc.EDGE_SEED, dc.EDGE_GEN0 + g, dc.EDGES[name][2], lo, hi)
        dc.check_edge_generation(name, g, rec)
        if dc.EDGES[name][0] == 1:
            assert np.all(rec["jrand"] == 0) and np.all(rec["cross"])             # D = 1: every trial crosses


def test_the_restatement_reaches_the_analytic_maximum():
    gap = dc.opt_reference_gap()
    print(f"gap after {dc.OPT_GENS} generations: {gap:.3e}")
    assert 0.0 <= gap < dc.OPT_GAP
    at_means = np.array([[p["p0"]] for p in dc.OPT_PRIORS])
    assert abs(de.evaluate(dc.OPT_PRIORS, at_means, None)[0][0] - dc.OPT_MAX) < 1e-12
