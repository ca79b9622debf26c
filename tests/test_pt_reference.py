"""
The restatement of the parallel-tempering statistics (tests/pt_reference.py) pinned by meaning, on the CPU: its streaming log-sum-exp is a
log-sum-exp, its block-ordered sums are sums (a second, plainest statement agrees), its round loop with an exact explorer re-places the
ladder until every pair rejects equally often and returns the analytic log evidence — and the same loop with the forward term's sign flipped,
or with the ladder left alone, fails that check —, flat stretches of the barrier give a valid ladder, every schedule case of the GPU suite
keeps its decision margins, the tempered restarts follow a hand-made sequence of permutations, and the independent log evidence of the test
model that tests/pt_cases.py quotes is recomputed once. tests/test_pt.py holds the device to this restatement.
"""
import numpy as np
import pytest

import draws_cases as cases
import pt_cases as pc
import pt_reference as pt


def all_terms(T, Cn):
    """per pair the forward and the backward terms of the first three scans of a shape, as flat arrays, and the counts"""
    beta = pc.ladder(T, Cn)
    f, b, nf, nb = [[] for _ in range(T - 1)], [[] for _ in range(T - 1)], np.zeros(T - 1), np.zeros(T - 1)
    for ll, s2r in pc.scans(T, Cn)[:3]:
        _, v_f, c_f, v_b, c_b = pt.pair_terms(ll, s2r, beta)
        for t in range(T - 1):
            f[t].append(v_f[t][v_f[t] > -np.inf])
            b[t].append(v_b[t][v_b[t] > -np.inf])
        nf += c_f.sum(axis=1)
        nb += c_b.sum(axis=1)
    return [np.concatenate(x) for x in f], [np.concatenate(x) for x in b], nf, nb


@pytest.mark.parametrize("T,Cn", pc.SHAPES)
def test_streaming_equals_batch(T, Cn):
    """m + log s of the streamed, block-merged pairs is logaddexp.reduce over all the terms, to 1e-13"""
    acc = pc.reference(T, Cn)["accs"][2]
    f, b, nf, nb = all_terms(T, Cn)
    assert np.array_equal(acc[:, pt.NF], nf) and np.array_equal(acc[:, pt.NB], nb) and np.all(acc[:, pt.N] == 3 * Cn)
    worst = 0.0
    for t in range(T - 1):
        for v, m, s in ((f[t], pt.MF, pt.SF), (b[t], pt.MB, pt.SB)):
            if v.size == 0:
                assert acc[t, m] == -np.inf and acc[t, s] == 0.0
                continue
            want = np.logaddexp.reduce(v)
            worst = max(worst, abs(acc[t, m] + np.log(acc[t, s]) - want) / max(1.0, abs(want)))
    print(f"T = {T}, Cn = {Cn}: streaming against batch log-sum-exp, worst relative deviation {worst:.2e}")
    assert worst <= 1e-13


@pytest.mark.parametrize("T,Cn", pc.SHAPES[:5])
def test_the_plainest_statement_agrees(T, Cn):
    """a loop over chains and pairs with no blocks: counts and maxima exactly, the sums within summation rounding"""
    beta = pc.ladder(T, Cn)
    acc = pc.reference(T, Cn)["accs"][2]
    plain = pt.plain_stats([(ll, s2r, beta) for ll, s2r in pc.scans(T, Cn)[:3]])
    for col in (pt.N, pt.NF, pt.MF, pt.NB, pt.MB):
        assert np.array_equal(acc[:, col], plain[:, col]), col
    n_terms = 3 * Cn
    bar = 2.0 * n_terms * 2.0 ** -53                       # a sum of n non-negative terms in any order: relative error below n·u each way
    for col in (pt.A, pt.SF, pt.SB):
        assert np.all(np.abs(acc[:, col] - plain[:, col]) <= bar * np.maximum(np.abs(plain[:, col]), 1e-300) + 1e-300), col


# ---------------------------------------------------------------------------------------------------- exact tempered Gaussian draws
@pytest.fixture(scope="module")
def gauss_runs():
    return [pc.gauss_run(seed) for seed in pc.GAUSS_SEEDS]


def gauss_check(r):
    """what a run of the Gaussian case is held to: the list of what it misses"""
    fwd, rev, mean = (v - pc.GAUSS_LOGZ for v in r["log_evidence"])
    missed = []
    if not abs(fwd) <= pc.GAUSS_FWD_BAR:
        missed.append(("fwd", fwd))
    if not abs(rev) <= pc.GAUSS_REV_BAR:
        missed.append(("rev", rev))
    if not abs(mean) <= pc.GAUSS_MEAN_BAR:
        missed.append(("mean", mean))
    if not pc.spread(r["rejection_by_round"][-1]) <= pc.GAUSS_SPREAD_BAR:
        missed.append(("spread", pc.spread(r["rejection_by_round"][-1])))
    if not pc.GAUSS_BARRIER[0] <= r["barrier_by_round"][-1] <= pc.GAUSS_BARRIER[1]:
        missed.append(("barrier", r["barrier_by_round"][-1]))
    return missed


def test_exact_gaussian_draws_give_equal_rejection_rates_and_the_analytic_log_evidence(gauss_runs):
    err = np.array([[v - pc.GAUSS_LOGZ for v in r["log_evidence"]] for r in gauss_runs])
    first = [pc.spread(r["rejection_by_round"][0]) for r in gauss_runs]
    last = [pc.spread(r["rejection_by_round"][-1]) for r in gauss_runs]
    lam = [r["barrier_by_round"][-1] for r in gauss_runs]
    print(f"log Z = {pc.GAUSS_LOGZ:.4f}; over {len(gauss_runs)} seeds: Λ {np.mean(lam):.3f} ({min(lam):.3f} … {max(lam):.3f}); spread of r_t in round 1 "
          f"{np.mean(first):.3f}, in round {pc.GAUSS_ROUNDS} mean {np.mean(last):.4f} worst {max(last):.4f}")
    for k, name in enumerate(("fwd", "rev", "mean")):
        print(f"  last-round {name} error: mean {err[:, k].mean():+.4f}, sd {err[:, k].std(ddof=1):.4f}, worst {np.abs(err[:, k]).max():.4f}")
    for seed, r in zip(pc.GAUSS_SEEDS, gauss_runs):
        assert gauss_check(r) == [], (seed, gauss_check(r))
        assert r["n_scans"] == 2 ** (pc.GAUSS_ROUNDS + 1) - 2 and r["betas_by_round"].shape == (pc.GAUSS_ROUNDS + 1, pc.GAUSS_T)
        b = r["betas_by_round"]
        assert np.all(b[:, 0] == 1.0) and np.all(b[:, -1] == 0.0) and np.all(np.diff(b, axis=1) < 0.0)
        assert np.array_equal(b[-1], b[-2])                 # adaptation is off in the last round
        assert r["restarts"].sum() > 0
    assert min(first) > 10 * pc.GAUSS_SPREAD_BAR            # the cubic ladder is far from equal rates: the schedule has something to do
    # the measured deviations are the ones pt_cases.py quotes beside its bars
    assert abs(err[:, 0].std(ddof=1) - pc.GAUSS_FWD_SD) < 5e-4 and abs(err[:, 1].std(ddof=1) - pc.GAUSS_REV_SD) < 5e-4
    assert abs(err[:, 2].std(ddof=1) - pc.GAUSS_MEAN_SD) < 5e-4 and abs(max(last) - pc.GAUSS_WORST_SPREAD) < 5e-4


def test_the_gaussian_check_has_power(monkeypatch):
    """the ladder left at the cubic start, and db's sign flipped in the forward term: the same run fails the same check"""
    fixed = gauss_check(pc.gauss_run(0, adapt=False))
    print("schedule left at the cubic ladder:", fixed)
    assert "spread" in [name for name, _ in fixed]
    terms = pt.pair_terms

    def flipped(*args):
        alpha, v_f, n_f, v_b, n_b = terms(*args)
        return alpha, np.where(v_f > -np.inf, -v_f, v_f), n_f, v_b, n_b
    monkeypatch.setattr(pt, "pair_terms", flipped)
    wrong = gauss_check(pc.gauss_run(0))
    print("db's sign flipped in the forward term:", wrong)
    assert "fwd" in [name for name, _ in wrong] and "mean" in [name for name, _ in wrong]


# ---------------------------------------------------------------------------------------------------- the schedule
def acc_of_rates(r, n=1000.0):
    acc = pt.new_acc(len(r) + 1)
    acc[:, pt.N] = n
    acc[:, pt.A] = n * (1.0 - np.asarray(r))
    return acc


def test_flat_stretches_give_a_strictly_valid_ladder():
    """pairs with α = 1 throughout: r = 0 exactly, a flat Λ, and "the first t with Λ_{t+1} >= g" never divides by 0"""
    T, Cn = 8, 70
    beta = np.linspace(1.0, 0.0, T)
    ll = np.tile(np.linspace(-50.0, -80.0, T)[:, None], (1, Cn))      # by replica = by slot under the identity
    ll[2:5] = ll[2]                                                   # slots 2, 3, 4 hold the same ℓ: α = min(1, exp(0)) = 1 on pairs 2 and 3
    s2r = np.tile(np.arange(T), (Cn, 1))
    acc = pt.stats(ll, s2r, beta, pt.new_acc(T))
    r, lam = pt.barrier(acc)
    assert r[2] == 0.0 and r[3] == 0.0 and lam[2] == lam[3] == lam[4] and np.all(r[[0, 1, 4, 5, 6]] > 0.0)
    new = pt.schedule(acc, beta)["beta"]
    assert new[0] == 1.0 and new[-1] == 0.0 and np.all(np.isfinite(new)) and np.all(np.diff(new) < 0.0), new
    # a stretch at either end, every rate 0 (copied through), and one pair that carries the whole barrier
    for rates in ([0.0, 0.0, 0.3, 0.2, 0.0], [0.5, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.7]):
        b0 = np.linspace(1.0, 0.0, len(rates) + 1) ** 2
        new = pt.schedule(acc_of_rates(rates), b0)["beta"]
        assert new[0] == b0[0] and new[-1] == b0[-1] and np.all(np.isfinite(new)) and np.all(np.diff(new) < 0.0), (rates, new)
    b0 = np.linspace(1.0, 0.0, 6)
    assert np.array_equal(pt.schedule(acc_of_rates([0.0] * 5), b0)["beta"], b0)
    assert np.array_equal(pt.schedule(pt.new_acc(6), b0)["beta"], b0) and np.all(np.isnan(pt.schedule(pt.new_acc(6), b0)["summary"]))
    assert np.array_equal(pt.schedule(acc_of_rates([0.2, 0.1, 0.4, 0.3, 0.5]), b0, adapt=False)["beta"], b0)


def test_equal_rates_are_the_fixed_point_and_the_interpolation_is_linear():
    b0 = np.linspace(1.0, 0.0, 5)
    assert np.allclose(pt.schedule(acc_of_rates([0.25] * 4), b0)["beta"], b0, rtol=0, atol=1e-15)
    s = pt.schedule(acc_of_rates([0.6, 0.2, 0.1, 0.1]), b0)
    assert np.isclose(s["summary"][pt.LAMBDA], 1.0)
    # g = 0.25, 0.5, 0.75 all fall in or at the end of the first pair's share 0.6, the last inside the second
    assert np.allclose(s["beta"], [1.0, 1.0 - 0.25 * 0.25 / 0.6, 1.0 - 0.25 * 0.5 / 0.6, 0.75 - 0.25 * 0.15 / 0.2, 0.0])


@pytest.mark.parametrize("T,Cn", pc.SHAPES)
def test_every_gpu_schedule_case_keeps_its_decision_margins(T, Cn):
    ref = pc.reference(T, Cn)
    print(f"T = {T}, Cn = {Cn}: least |g_k − Λ_t|/Λ = {ref['margin']:.3e}")
    assert ref["margin"] > pc.MARGIN_BAR
    new = ref["schedule"]["beta"]
    assert new[0] == ref["beta"][0] and new[-1] == ref["beta"][-1] and np.all(np.diff(new) <= 0.0)
    assert T == 2 or not np.array_equal(new, ref["beta"])      # the case does re-place its ladder


# ---------------------------------------------------------------------------------------------------- tempered restarts
def test_tempered_restarts_follow_a_hand_made_sequence():
    """T = 3, one chain, slot2rep scan by scan; what each scan must leave is worked out by hand below"""
    seq = [[0, 1, 2], [0, 2, 1], [2, 0, 1], [2, 1, 0], [1, 2, 0], [1, 0, 2], [0, 1, 2]]
    leg, count = np.zeros((1, 3), dtype=np.int64), np.zeros(1, dtype=np.int64)
    seen = []
    for s2r in seq:
        pt.restarts(np.array([s2r]), leg, count)
        seen.append((int(count[0]), leg[0].tolist()))
    # scan 0: rep 2 at slot 2 -> leg[2] = 1; slot 0 holds rep 0, leg 0          -> 0, [0, 0, 1]
    # scan 1: rep 1 at slot 2 -> leg[1] = 1; slot 0 holds rep 0                  -> 0, [0, 1, 1]
    # scan 2: rep 1 at slot 2; slot 0 holds rep 2 with leg 1: restart, leg[2] = 0 -> 1, [0, 1, 0]
    # scan 3: rep 0 at slot 2 -> leg[0] = 1; slot 0 holds rep 2, leg 0           -> 1, [1, 1, 0]
    # scan 4: rep 0 at slot 2; slot 0 holds rep 1 with leg 1: restart, leg[1] = 0 -> 2, [1, 0, 0]
    # scan 5: rep 2 at slot 2 -> leg[2] = 1; slot 0 holds rep 1, leg 0           -> 2, [1, 0, 1]
    # scan 6: rep 2 at slot 2; slot 0 holds rep 0 with leg 1: restart, leg[0] = 0 -> 3, [0, 0, 1]
    assert seen == [(0, [0, 0, 1]), (0, [0, 1, 1]), (1, [0, 1, 0]), (1, [1, 1, 0]), (2, [1, 0, 0]), (2, [1, 0, 1]), (3, [0, 0, 1])]
    # chains are independent: the second walks the sequence backwards — by hand its restarts fall in scans 3 and 5
    leg, count = np.zeros((2, 3), dtype=np.int64), np.zeros(2, dtype=np.int64)
    for a, b in zip(seq, seq[::-1]):
        pt.restarts(np.array([a, b]), leg, count)
    assert count.tolist() == [3, 2]


# ---------------------------------------------------------------------------------------------------- the independent log evidence
def test_the_quoted_log_evidence_of_the_test_model_is_recomputed(oracle):
    """prior importance sampling through the CPU oracle, the first window of seed 31 (about 10 s): the constant the GPU suite holds the driver to"""
    est, ess = pc.importance_logz(oracle, cases.POST_SEEDS[0], cases.POST_FIRST[0], cases.POST_N)
    print(f"log mean exp ℓ over 2^20 prior draws of seed {cases.POST_SEEDS[0]}: {est:.4f}, ESS {ess:.0f}; quoted {pc.MODEL_LOGZ} ± {pc.MODEL_LOGZ_SE}")
    assert 8000 < ess < 11000
    assert abs(est - pc.MODEL_LOGZ) <= 4 * np.hypot(pc.MODEL_LOGZ_SE_ONE, pc.MODEL_LOGZ_SE)
