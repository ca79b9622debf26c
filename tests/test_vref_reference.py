"""
The restatement of the variational reference (tests/vref_reference.py) held to its meaning, on the CPU: log q of a table is scipy's normal
log density; the two-leg round loop on the exact tempered Gaussian of tests/pt_cases.py recovers log Z on both legs and the variational leg's
communication barrier is a small fraction of the prior leg's — and is not when the fit is skipped; the exchange permutes the two targets.
"""
import numpy as np
import pytest

import pt_cases as pc
import vref_cases as vc
import vref_reference as vr


@pytest.mark.parametrize("D", vc.TABLE_D)
def test_log_q_of_the_table_is_the_normal_log_density(D):
    import scipy.stats as ss
    mean, sd = vc.table_inputs(D)
    t = vr.table(mean, sd)
    assert not t["bad"].any() and vr.table_doubles(D) == 15 * D
    assert sum(n for _, n in vr.parts(D).values()) == vr.table_doubles(D)
    rng = np.random.default_rng(D)
    x = mean[:, None] + sd[:, None] * rng.standard_normal((D, 50)) * 3.0
    lq, healed = vr.log_q(t["priors"], x)
    want = ss.norm.logpdf(x, mean[:, None], sd[:, None]).sum(axis=0)
    assert not healed.any() and np.all(np.abs(lq - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    # the constants are the ones the density uses: −log σ and 1/σ
    assert np.array_equal(t["pc"][:, 2], -np.log(sd)) and np.array_equal(t["pc"][:, 3], 1.0 / sd) and np.all(t["pc"][:, 1] == 0.0)


def test_the_table_rule_names_the_bad_coordinates():
    mean, sd = vc.table_inputs(11)
    mean, sd = mean.copy(), sd.copy()
    mean[3], sd[5], sd[7], sd[9] = np.nan, 0.0, -1.0, np.inf
    assert np.flatnonzero(vr.table(mean, sd)["bad"]).tolist() == [3, 5, 7, 9]
    count, m, m2 = vc.moments_inputs(11)
    mu, s, n = vr.fit(count, m, m2, inflate=1.5)
    assert np.array_equal(s, 1.5 * np.sqrt(m2 / (count[0] - 1.0))) and not vr.table(mu, s, n)["bad"].any()
    assert vr.table(*vr.fit(np.array([1.0]), m, m2)).get("bad").all()


@pytest.fixture(scope="module")
def gauss_runs():
    return [vc.gauss_run(seed) for seed in vc.GAUSS_SEEDS]


def test_two_legs_on_the_exact_tempered_gaussian(gauss_runs):
    lam = np.array([[leg["barrier_by_round"][-1] for leg in run] for run in gauss_runs])                   # [seed][leg]
    err = np.array([[np.array(leg["log_evidence"]) - pc.GAUSS_LOGZ for leg in run] for run in gauss_runs])  # [seed][leg][fwd, rev, mean]
    for k, leg in enumerate(("fixed", "variational")):
        print(f"{leg:12s} Λ {lam[:, k].mean():.4f} ({lam[:, k].min():.4f} … {lam[:, k].max():.4f})")
        for j, name in enumerate(("fwd", "rev", "mean")):
            e = err[:, k, j]
            print(f"{leg:12s} {name:4s} error mean {e.mean():+.4f} sd {e.std(ddof=1):.4f} worst |·| {np.abs(e).max():.4f}")
            assert np.all(np.abs(e) < vc.GAUSS_BARS[leg][j]), (leg, name, np.abs(e).max())
    print(f"worst Λ_var/Λ_fixed {np.max(lam[:, 1] / lam[:, 0]):.4f}")
    assert np.all(lam[:, 1] < vc.GAUSS_BARRIER_VAR_BAR), lam[:, 1].max()
    assert np.all(lam[:, 1] < vc.GAUSS_BARRIER_RATIO * lam[:, 0]), np.max(lam[:, 1] / lam[:, 0])
    for run in gauss_runs:
        m, s = run[1]["mean_by_round"], run[1]["sd_by_round"]
        first = vc.GAUSS_FIRST_TUNING_ROUND - 2      # the row of the first round that ends with a fit
        assert np.isnan(m[:first]).all() and np.isfinite(m[first:]).all() and np.isfinite(s[first:]).all()
        # the fit found the posterior: N(μ/(1 + σ²), σ²/(1 + σ²)) in every coordinate
        s2 = pc.GAUSS_SIGMA ** 2
        assert np.all(np.abs(m[-1] - pc.GAUSS_MU / (1.0 + s2)) < 0.05) and np.all(np.abs(s[-1] / np.sqrt(s2 / (1.0 + s2)) - 1.0) < 0.1)


def test_the_barrier_check_has_power():
    """with the fit skipped the second leg stays on the prior, and the assertion on Λ fails at every seed tried"""
    for seed in vc.GAUSS_POWER_SEEDS:
        fixed, second = vc.gauss_run(seed, fit_reference=False)
        lam_f, lam_v = fixed["barrier_by_round"][-1], second["barrier_by_round"][-1]
        print(f"seed {seed}: fit skipped, Λ_fixed {lam_f:.4f} Λ_second {lam_v:.4f}")
        assert not lam_v < vc.GAUSS_BARRIER_RATIO * lam_f and not lam_v < vc.GAUSS_BARRIER_VAR_BAR
        assert np.isnan(second["mean_by_round"]).all()


@pytest.mark.parametrize("shape", vc.EXCHANGE_SHAPES)
def test_the_exchange_permutes_the_two_targets(shape):
    Cn, T_a, T_b = shape
    a0, b0 = vc.exchange_inputs(*shape)
    a1, b1 = vc.exchange_reference(*shape)
    c = np.arange(Cn)
    ca, cb = a0["slot2rep"][:, 0] * Cn + c, b0["slot2rep"][:, 0] * Cn + c

    def rows(legs_cols):
        return sorted(tuple(np.concatenate([g["theta"][:, k], [g["lp"][k]]]).view(np.uint64)) for g, cols in legs_cols for k in cols)
    assert rows(((a0, ca), (b0, cb))) == rows(((a1, ca), (b1, cb)))                    # the multiset of (θ, ℓπ), bit for bit
    assert np.array_equal(a1["theta"][:, ca], b0["theta"][:, cb], equal_nan=True) and np.array_equal(b1["lp"][cb], a0["lp"][ca])
    for g0, g1, cols in ((a0, a1, ca), (b0, b1, cb)):
        rest = np.setdiff1d(np.arange(g0["lp"].size), cols)
        for k in ("theta", "lp", "ll"):
            assert np.array_equal(g0[k][..., rest], g1[k][..., rest], equal_nan=True), k
    assert b1["ll"][cb[0]] == -np.inf          # leg A's target of chain 0 had ℓπ = −Inf: it is leg B's now
    assert a1["ll"][ca[Cn - 1]] == -np.inf     # leg B's target of the last chain had a NaN coordinate: leg A's reference is healed there
