"""
The NumPy restatement of the OFTI rejection sampler (tests/ofti_draws_reference.py) on the CPU: the conditions every case of
tests/ofti_draws_cases.py has to meet before tests/test_ofti_draws.py compares the device with it; its ℓ and μ against the oracle's restatement
of ofti_linear_solve at that function's own bars (tests/test_ofti.py: 1e-9 and 1e-8); the Thiele-Innes draw is the conditional normal; the
elements of a draw give the draw back.
"""
import math

import numpy as np
import pytest
from scipy.special import ndtr

import draws_cases
import ofti_draws_cases as oc
import ofti_draws_reference as oref


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: f"{c[0]}-seed{c[1]}-mode{c[2]}")
def test_the_cases_meet_their_conditions(case):
    r = oc.restated(*case)
    print(f"{case}: accepted {r['n_accepted']} of {oc.N}, undecided {r['undecided']}, max cond(S) {np.max(r['cond']):.3g}, near face-on {r['n_face_on']}")
    oc.check_conditions(r)
    assert np.all(np.diff(r["index"].astype(np.int64)) > 0) and r["index"][0] >= oc.FIRST and r["index"][-1] < oc.FIRST + oc.N
    assert r["post"].shape == (oref.N_OUT, r["n_accepted"]) and np.all(np.isfinite(r["post"]))
    assert np.all(r["post"][12] >= 0) and np.all(r["post"][12] < math.pi) and np.all(r["post"][11] >= 0) and np.all(r["post"][11] < 2 * math.pi)


@pytest.mark.parametrize("name", oc.TABLES)
def test_the_restated_marginal_likelihood_is_the_oracles(oracle, name):
    """ℓ of the accepted draws and of the first 2000 draws (wherever they fall in the prior), and μ of the accepted"""
    tab, r = oc.table(name), oc.restated(name, oc.SEEDS[0], 1)
    abfg, lm = oracle.oracle_ofti(*oc.columns(tab), r["nl"])
    assert np.all(np.abs(r["post"][15] - lm) <= 1e-9 * np.maximum(1.0, np.abs(lm)))
    assert np.all(np.abs(r["post"][4:8] - abfg) <= 1e-8 * np.linalg.norm(abfg, axis=0))
    import hmc_reference as ref
    theta, _ = ref.prior_sample(oc.PRIORS_TAU, oc.SEEDS[0], np.uint64(oc.FIRST) + np.arange(2000, dtype=np.uint64))
    nl = oref.nl_of(theta, 1, oc.T_REF, oc.k_yr())
    _, lm = oracle.oracle_ofti(*oc.columns(tab), nl)
    assert np.array_equal(r["ll"][:2000] == -np.inf, lm == -np.inf)
    assert np.all(np.abs(r["ll"][:2000] - lm) <= 1e-9 * np.maximum(1.0, np.abs(lm)))


def test_invalid_parameter_sets_are_minus_infinity():
    tab = oc.table("ofti_example")
    nl = np.array(oc.restated("ofti_example", 41, 1)["nl"][:, :5])
    nl[0, 0], nl[0, 1], nl[1, 2], nl[3, 3] = np.nan, 1.0, -2.0, 0.0
    post = oref.posterior(tab, 41, np.arange(5, dtype=np.uint64), nl, oc.k_yr())
    assert np.all(post[15, :4] == -np.inf) and np.all(np.isnan(post[:15, :4])) and np.all(np.isfinite(post[:, 4]))


def test_every_draw_is_rejected_by_the_rejecting_table():
    r = oref.rejection(oc.rejecting_table(), oc.PRIORS_NONE, 41, 0, oc.NONE_N, 1, oc.T_REF, oc.k_yr())
    assert np.all(r["ll"] == -np.inf) and r["n_accepted"] == 0 and r["max_logml"] == -np.inf


def test_the_thiele_innes_draw_is_the_conditional_normal():
    """one fixed nl, indices 0 … 65535: Lᵀ(x − μ) is N(0, I) — a Kolmogorov-Smirnov test per coordinate — the coordinates uncorrelated, and L the factor of S"""
    n = draws_cases.STAT_W
    tab = oc.table("ofti_cor_37")
    nl = np.repeat(np.array(oc.restated("ofti_cor_37", 41, 1)["nl"][:, :1]), n, axis=1)
    post = oref.posterior(tab, 43, np.arange(n, dtype=np.uint64), nl, oc.k_yr())
    s = oref.solve(tab, nl[:, :1], oc.k_yr())
    L, S = s["chol"][0], s["S"][0]
    w = L.T @ (post[:4] - post[4:8])
    for k in range(4):
        stat = draws_cases.ks_statistic(w[k], ndtr)
        print(f"coordinate {k}: D_n {stat:.3e} (bar {draws_cases.STAT_BAR:.3e})")
        assert stat < draws_cases.STAT_BAR
    # the whitened coordinates are uncorrelated: |r| of n pairs of independent normals is below 4.5/√n but for 1 in 1e5
    c = np.corrcoef(w)
    assert np.max(np.abs(c - np.eye(4))) < 4.5 / math.sqrt(n)
    assert np.allclose(L @ L.T, S, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", oc.CASES[:2] + oc.CASES[-1:], ids=lambda c: f"{c[0]}-seed{c[1]}-mode{c[2]}")
def test_the_elements_give_the_draw_back(case):
    """the textbook Thiele-Innes constants of (α, i, ω, Ω) are the draw, to 1e-12·‖x‖; and M_dyn at a_ti has the period the solve used"""
    r = oc.restated(*case)
    post, nl = r["post"], r["nl"]
    back = oref.thiele_innes(post[8], post[10], post[11], post[12])
    assert np.all(np.linalg.norm(back - post[:4], axis=0) <= 1e-12 * np.linalg.norm(post[:4], axis=0))
    assert np.allclose(oref.period_days(oc.k_yr(), post[9], post[14]), post[13], rtol=1e-13, atol=0)
    assert np.allclose(post[13], oref.period_days(oc.k_yr(), nl[1], nl[3]), rtol=0, atol=0)
