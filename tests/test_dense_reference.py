"""
Conditions on the NumPy restatement of the dense metric (tests/dense_reference.py) that need no device, and the numbers tests/dense_cases.py
records for the GPU suite (tests/test_dense.py):
  (i)   with L = diag(√inv_mass) the dense restatements are hmc_reference.hmc_step and nuts_reference.nuts_transition up to rounding;
  (ii)  the textbook form (p ~ N(0, Σ⁻¹), Σ in every place the metric occurs) and the whitened form the device runs agree likewise;
  (iii) the one-ulp sensitivities ONE_S and DEEP_S of the two NUTS cases under the correlated factor;
  (iv)  the conditions on the inputs of those cases, from the restatement alone, and the step numbers they were chosen by;
  (v)   cov against exact rational arithmetic, factor against numpy.linalg.cholesky, the two products against NumPy's;
  (vi)  the prior is stationary under the dense restatement, and the seeds the GPU suite uses.
"""
import numpy as np
import pytest

import dense_cases as dc
import dense_reference as dref
import draws_cases as cases
import hmc_reference as ref
import nuts_reference as nuts

BAR = 1e-10      # (i), (ii): relative to max(1, |value|)
NUTS_KEYS = ("depth", "stop", "selected", "n_leapfrog")


def decisions_differ(a, b, decided):
    return [k for k in NUTS_KEYS if not np.array_equal(a[k][decided], b[k][decided])]


def check_same_transition(a, b, what):
    """the decisions of b on every chain decided in b, and θ_t, ℓπ, log_accept within BAR"""
    decided = b["margin"] > nuts.MARGIN
    assert decisions_differ(a, b, decided) == [], what
    dev, n_same = cases.transition_deviation(a, b)
    print(f"{what}: {np.sum(~decided)} of {decided.size} undecided; deviation {dev:.3e} over {n_same} chains")
    assert n_same >= decided.sum() and dev <= BAR, (what, dev)


# ---------------------------------------------------------------------------------------------------- (v) the factor, the products, the co-moments
@pytest.mark.parametrize("D", (1, 2, 14, 64))
def test_the_test_factor_is_the_cholesky_factor_of_its_covariance(D):
    im = np.array([cases.STAT_INV_MASS[d % 5] for d in range(D)])
    L = dc.factor_of(im)
    i, j = np.indices((D, D))
    Sigma = np.sqrt(np.outer(im, im)) * dc.RHO ** np.abs(i - j)
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
    assert np.allclose(L @ L.T, Sigma, rtol=1e-13, atol=0)
    assert np.allclose(L, np.linalg.cholesky(Sigma), rtol=1e-12, atol=1e-300)
    assert np.array_equal(dref.unpack(dref.pack(L), D), L)
    x = np.random.default_rng(D).normal(size=(D, 7))
    for transpose, mine in ((False, dref.lower(L, x)), (True, dref.lower_t(L, x))):
        want = (L.T if transpose else L) @ x
        assert np.all(np.abs(mine - want) <= 1e-13 * dref.product_scale(L, x, transpose))
    p = dref.textbook_momentum(L, x)
    assert np.allclose(L.T @ p, x, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("K", dc.COV_K)
@pytest.mark.parametrize("W", dc.COV_W)
def test_cov_against_exact_arithmetic(W, K):
    x, exact = dc.cov_case(W, K)
    dc.check_cov(dref.cov(x), exact, f"W {W}, K {K}")
    held = None
    for a, b in cases.thirds(W):
        held = dref.cov(x[:, a:b], held=held) if held is not None else dref.cov(x[:, a:b])
    dc.check_cov(held, exact, f"W {W}, K {K}, thirds")


@pytest.mark.parametrize("K", (1, 2, 11, 64))
def test_factor_against_numpy_and_its_info_rule(K):
    rng = np.random.default_rng(K)
    n = 4 * K + 3
    x = rng.normal(size=(K, n)) * (10.0 ** (np.arange(K) % 4 - 1))[:, None]
    cnt, _, m2 = dref.cov(x)
    sentinel = np.full(K * (K + 1) // 2, -7.0)
    for regularize in (False, True):
        S = np.cov(x).reshape(K, K)
        if regularize:
            S = (n / (n + 5.0)) * S + 1e-3 * (5.0 / (n + 5.0)) * np.eye(K)
        chol, info = dref.factor(cnt, m2, sentinel, regularize)
        assert info == 0
        L = dref.unpack(chol, K)
        scale = np.sqrt(np.outer(np.diag(S), np.diag(S)))      # an entry of Σ near 0 has no digits of its own: relative to √(Σ_ii·Σ_jj)
        assert np.all(np.abs(L - np.linalg.cholesky(S)) <= 1e-10 * np.sqrt(np.diag(S))[:, None]) and np.all(np.abs(L @ L.T - S) <= 1e-12 * scale)
    if K >= 2:      # rank-deficient: n = K/2 chains (K = 2: a single chain, which the regularisation cannot mend either)
        c2, _, s2 = dref.cov(x[:, :K // 2])
        chol, info = dref.factor(c2, s2, sentinel, False)
        assert info != 0 and np.array_equal(chol, sentinel)
        assert (dref.factor(c2, s2, sentinel, True)[1] == 0) == (K // 2 >= 2)
    chol, info = dref.factor(np.array([1.0]), np.zeros_like(sentinel), sentinel, True)
    assert info == 1 and np.array_equal(chol, sentinel)


# ---------------------------------------------------------------------------------------------------- (i) the diagonal factor
def test_diagonal_factor_is_the_diagonal_step(oracle):
    logpost = cases.oracle_logpost(oracle, cases.oracle_model(oracle))
    beta, eps, im = cases.step_inputs(dc.STEP_W)
    start = ref.prior_sample(cases.MODEL_PRIORS, cases.STEP_SEED, np.arange(dc.STEP_W, dtype=np.uint64))[1]
    for n_leapfrog in dc.STEP_LEAPFROGS:
        want = ref.hmc_step(cases.MODEL_PRIORS, start, beta, eps, n_leapfrog, im, cases.STEP_SEED, cases.STEP_STEP, logpost=logpost)
        for form in ("textbook", "whitened"):
            got = dref.hmc_step_dense(cases.MODEL_PRIORS, start, beta, eps, n_leapfrog, dc.diagonal_factor(im), cases.STEP_SEED, cases.STEP_STEP, logpost=logpost, form=form)
            check_same_step(got, want, f"diagonal, {form}, L {n_leapfrog}")


def check_same_step(got, want, what):
    decided = np.abs(want["log_u"] - want["dH"]) > 1e-6
    assert np.array_equal(got["accepted"][decided], want["accepted"][decided]), what
    fin = np.isfinite(want["dH"])
    dev = float(np.max(np.abs(got["proposal"] - want["proposal"]) / np.maximum(1.0, np.abs(want["proposal"]))))
    dev = max(dev, float(np.max(np.abs(got["dH"][fin] - want["dH"][fin]) / np.maximum(1.0, np.abs(want["dH"][fin])), initial=0.0)))
    same = decided
    dev = max(dev, float(np.max(np.abs(got["logpost"][same] - want["logpost"][same]) / np.maximum(1.0, np.abs(want["logpost"][same])), initial=0.0)))
    print(f"{what}: {np.sum(~decided)} undecided flags; deviation {dev:.3e}")
    assert dev <= BAR, (what, dev)


def test_diagonal_factor_is_the_diagonal_transition(oracle):
    start = dc.model_start()
    beta, eps, im = cases.one_inputs()
    logpost = cases.oracle_logpost(oracle, cases.oracle_model(oracle))
    want = nuts.nuts_transition(cases.MODEL_PRIORS, start, beta, eps, im, cases.ONE_DEPTH, cases.ONE_SEED, cases.ONE_STEP, logpost=logpost)
    for form in ("textbook", "whitened"):
        got = dref.nuts_transition_dense(cases.MODEL_PRIORS, start, beta, eps, dc.diagonal_factor(im), cases.ONE_DEPTH, cases.ONE_SEED, cases.ONE_STEP,
                                         logpost=logpost, form=form)
        check_same_transition(got, want, f"diagonal factor, {form}")
    assert nuts._Setup.__name__ == "_Setup"      # the restatement's own setup is back in place


# ---------------------------------------------------------------------------------------------------- (ii) textbook and whitened
def test_textbook_and_whitened_steps_agree(oracle):
    logpost = cases.oracle_logpost(oracle, cases.oracle_model(oracle))
    beta, eps, L = dc.step_inputs()
    start = ref.prior_sample(cases.MODEL_PRIORS, cases.STEP_SEED, np.arange(dc.STEP_W, dtype=np.uint64))[1]
    for n_leapfrog in dc.STEP_LEAPFROGS:
        a, b = (dref.hmc_step_dense(cases.MODEL_PRIORS, start, beta, eps, n_leapfrog, L, cases.STEP_SEED, cases.STEP_STEP, logpost=logpost, form=form)
                for form in ("whitened", "textbook"))
        check_same_step(a, b, f"correlated, L {n_leapfrog}")
        undecided = np.mean(np.abs(b["log_u"] - b["dH"]) <= 1e-6)
        assert undecided <= 0.01 and 0.2 < b["accepted"].mean() < 1.0, (undecided, b["accepted"].mean())      # the condition on the seed
    e, Lp = dc.step_prior_inputs()
    tt = ref.prior_sample(cases.STAT_PRIORS, cases.STEP_SEED, np.arange(dc.STEP_W, dtype=np.uint64))[1]
    a, b = (dref.hmc_step_dense(cases.STAT_PRIORS, tt, None, e, 4, Lp, cases.STEP_SEED, cases.STEP_STEP, form=form) for form in ("whitened", "textbook"))
    check_same_step(a, b, "correlated, priors alone")


def test_textbook_and_whitened_transitions_agree(oracle):
    start = dc.model_start()
    check_same_transition(dc.one_transition(oracle, start, form="whitened"), dc.one_transition(oracle, start), "one transition")
    check_same_transition(dc.deep_transition(oracle, start, form="whitened"), dc.deep_transition(oracle, start), "deep transition")
    for D in cases.DIM_DS:
        check_same_transition(dc.dim_transition(D, form="whitened")[4], dc.dim_transition(D)[4], f"D {D}")


# ---------------------------------------------------------------------------------------------------- (iv) the conditions on the inputs
def first_step_that(check, run):
    for step in range(cases.ONE_STEP, cases.ONE_STEP + 8):
        try:
            check(run(step))
            return step
        except AssertionError:
            continue
    return None


def test_conditions_on_the_inputs_and_how_the_steps_were_chosen(oracle, monkeypatch):
    start = dc.model_start()
    cases.check_one_transition_is_decided(dc.one_transition(oracle, start))
    cases.check_deep_transition_is_decided(dc.deep_transition(oracle, start))

    def one(step):
        monkeypatch.setattr(dc, "ONE_STEP_DENSE", step)
        return dc.one_transition(oracle, start)

    def deep(step):
        monkeypatch.setattr(dc, "DEEP_STEP_DENSE", step)
        return dc.deep_transition(oracle, start)

    chosen = dc.ONE_STEP_DENSE, dc.DEEP_STEP_DENSE
    assert (first_step_that(cases.check_one_transition_is_decided, one), first_step_that(cases.check_deep_transition_is_decided, deep)) == chosen
    for D in cases.DIM_DS:
        r = dc.dim_transition(D)[4]
        decided = r["margin"] > nuts.MARGIN
        print(f"D {D}: {cases.tree_summary(r)}")
        assert np.mean(~decided) <= cases.ONE_UNDECIDED and len(set(r["depth"][decided])) >= cases.DIM_DEPTHS


# ---------------------------------------------------------------------------------------------------- (iii) the sensitivity to one ulp
@pytest.mark.parametrize("case", ("one", "deep"))
def test_sensitivity_to_one_ulp(oracle, case):
    """Measures dense_cases.ONE_S and DEEP_S as tests/test_nuts_reference.py measures DEEP_S; the recorded constant is what is measured, rounded up
    in its third digit. No decided chain may change a decision."""
    run, recorded = (dc.one_transition, dc.ONE_S) if case == "one" else (dc.deep_transition, dc.DEEP_S)
    start = dc.model_start()
    r = run(oracle, start)
    decided = r["margin"] > nuts.MARGIN
    s = 0.0
    for moved in (np.nextafter(start, np.inf), np.nextafter(start, -np.inf)):
        r2 = run(oracle, moved)
        assert decisions_differ(r2, r, decided) == []
        dev, n_same = cases.transition_deviation(r2, r)
        assert n_same >= decided.sum()
        s = max(s, dev)
    print(f"{case} transition under the correlated factor, starts moved by one ulp: s = {s:.3e} (recorded {recorded:.3e})")
    assert s <= recorded <= 1.01 * s + 1e-15


# ---------------------------------------------------------------------------------------------------- (vi) the prior is stationary
STAT_CANDIDATES = range(21, 29)


def hmc_stationarity(seed):
    eps, n_leapfrog = cases.STAT_SETTINGS[0]
    L = dc.stationary_factor()
    tt = ref.prior_sample(cases.STAT_PRIORS, seed, np.arange(cases.STAT_W, dtype=np.uint64))[1]
    acc = []
    for step in range(cases.STAT_STEPS):
        r = dref.hmc_step_dense(cases.STAT_PRIORS, tt, None, eps, n_leapfrog, L, seed, step)
        tt = r["theta_t"]
        acc.append(r["accepted"].mean())
    return cases.stationarity_statistics(tt), float(np.mean(acc))


def nuts_stationarity(seed):
    L = dc.stationary_factor()
    tt = ref.prior_sample(cases.STAT_PRIORS, seed, np.arange(cases.STAT_W, dtype=np.uint64))[1]
    leaves = []
    for step in range(cases.STAT_STEPS):
        r = dref.nuts_transition_dense(cases.STAT_PRIORS, tt, None, cases.NUTS_STAT_EPS[0], L, cases.NUTS_STAT_DEPTH, seed, step)
        tt = r["theta_t"]
        leaves.append(r["n_leapfrog"].mean())
    return cases.stationarity_statistics(tt), float(np.mean(leaves))


@pytest.mark.parametrize("sampler", ("hmc", "nuts"))
def test_prior_is_stationary_under_the_correlated_factor(sampler):
    run, chosen = (hmc_stationarity, dc.STAT_SEEDS_HMC) if sampler == "hmc" else (nuts_stationarity, dc.STAT_SEEDS_NUTS)
    passed = []
    for seed in STAT_CANDIDATES:
        stat, other = run(seed)
        print(f"{sampler}, seed {seed}: max D_n {stat:.3e} (bar {cases.STAT_BAR:.3e}); {'acceptance' if sampler == 'hmc' else 'mean leaves'} {other:.3f}")
        if stat < cases.STAT_BAR:
            passed.append(seed)
        if len(passed) == 2:
            break
    assert tuple(passed) == chosen
