"""
The reference side of the PSIS tests, checked on its own (CPU suite): the float64 restatement of the algorithm of
include/octofitter_hip_psis.h (psis_reference.psis_row) against its 40-digit twin (psis_row_mp) on every case of the generator, the
Zhang–Stephens fit against samples of scipy's generalised Pareto distribution, and the properties the device tests lean on.

Bar of the restatement: 1e-11 — relative to max(1, |ref|) for elpd_loo, lppd, ess and the log-weights (the project's pointwise bar), absolute
for k̂ — with n and tail_len exact. The observed gaps G_k (k̂, absolute) and G_e (elpd, relative) are printed: 7.4e-14 and 1.6e-14 over these
cases, both at S = 4103, (c, ν) = (1, 5), k̂ = 4.05 — the heaviest tail, where y = exp(x) − exp(x_c) cancels most. tests/test_psis.py holds
the device's k̂ and ess to 100 × the gap measured here.
"""
import numpy as np
import pytest

import psis_reference as pr


@pytest.mark.parametrize("name", list(pr.CASES))
def test_restatement_against_40_digits(name):
    LL, ref = pr.case(name)
    g = pr.gaps(pr.psis_matrix(LL), ref)
    print(f"{name}: k_ref {np.min(ref['pareto_k']):.3f} … {np.max(ref['pareto_k']):.3f}  G_k = {g['pareto_k']:.2e}  G_e = {g['elpd_loo']:.2e}  "
          f"lppd {g['lppd']:.2e}  ess {g['ess']:.2e}  lw {g['lw']:.2e}")
    assert max(g.values()) <= 1e-11, g


@pytest.mark.parametrize("k", [0.1, 0.5, 0.9])
def test_gpdfit_recovers_the_shape_of_scipy_genpareto(k):
    from scipy.stats import genpareto
    y = np.sort(genpareto.rvs(c=k, scale=2.0, size=2000, random_state=1))
    khat, sigma = pr.gpdfit(y)
    print(f"genpareto k = {k}: k̂ = {khat:.4f} (error {abs(khat - k):.4f}), σ̂ = {sigma:.4f}")
    assert abs(khat - k) <= 0.08      # the fit shrinks towards 0.5 by construction: (n·k + 5)/(n + 10)


def test_tail_len():
    assert [pr.tail_len(n) for n in (0, 1, 2, 5, 24, 25, 100, 225, 226, 120001)] == [0, 1, 1, 1, 5, 5, 20, 45, 46, 1040]
    # the largest S whose tail fits the kernel's sort buffer
    assert pr.tail_len(1864135) <= pr.MAX_TAIL < pr.tail_len(1864136)


def test_properties():
    # a row of equal values: nothing lies strictly above the cut-off
    for S in (1, 7, 300):
        r = pr.psis_row(np.full(S, -2.5))
        assert r["tail_len"] == 0 and r["pareto_k"] == np.inf and r["n"] == S
        assert abs(r["elpd_loo"] + 2.5) <= 1e-14 and abs(r["lppd"] + 2.5) <= 1e-14 and abs(r["ess"] - S) <= 1e-12 * S
    for name in pr.RESTATEMENT_CASES:
        LL, _ = pr.case(name)
        for row in LL:
            for fn in (pr.psis_row, pr.psis_row_mp):
                r = fn(row)
                assert r["tail_len"] <= pr.tail_len(int(r["n"]))
                assert abs(np.sum(np.exp(r["lw"])) - 1.0) <= 1e-13 * max(1.0, np.sqrt(row.size))
                assert np.all(r["lw"] <= 0.0)
    # ties at the cut-off stay out of the tail; excluded entries weigh nothing
    row = np.round(pr.student_rows(400, 1, 1.0, 5.0, 3)[0] * 4.0) / 4.0
    r = pr.psis_row(row)
    assert 4 < r["tail_len"] < pr.tail_len(400)
    row[::7] = np.nan
    row[3] = np.inf
    r = pr.psis_row(row)
    assert r["n"] == np.isfinite(row).sum() and np.all(r["lw"][~np.isfinite(row)] == -np.inf)
    r = pr.psis_row(np.array([np.nan, -np.inf]))
    assert r["n"] == 0 and np.isnan(r["pareto_k"]) and np.isnan(r["elpd_loo"]) and np.all(r["lw"] == -np.inf)
