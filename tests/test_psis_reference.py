"""
The reference side of the PSIS tests, checked on its own (CPU suite): the float64 restatement of the algorithm of
include/octofitter_hip_psis.h (psis_reference.psis_row) against its 40-digit twin (psis_row_mp) on every case of the generator, the
Zhang–Stephens fit against samples of scipy's generalised Pareto distribution, and the properties the device tests lean on.

Bar of the restatement: 1e-11 — relative to max(1, |ref|) for elpd_loo, lppd, ess and the log-weights (the project's pointwise bar), absolute
for k̂ — with n and tail_len exact. The observed gaps G_k (k̂, absolute) and G_e (elpd, relative) are printed: 7.4e-14 and 1.6e-14 over these
cases, both at S = 4103, (c, ν) = (1, 5), k̂ = 4.05 — the heaviest tail, where y = exp(x) − exp(x_c) cancels most. tests/test_psis.py holds
the device's k̂ and ess to 100 × the gap measured here.

The edge rows (psis_reference.EDGE_ROWS) are checked here before tests/test_psis.py may use them: each row's route through the kernel's select
(gather_pass), its tail length, its conditions, the hybrid reference of the rows above S = 120 001 against psis_row_mp, and, for the rows
whose bars are per row, that those bars cannot pass a tail that is wrong by one entry.
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


@pytest.mark.parametrize("name", ["S20011", "S120001_R2"])
def test_hybrid_reference_against_40_digits(name):
    """psis_row_hybrid (the reference of the rows above S = 120 001) against psis_row_mp: n and tail_len equal, every other field within
    2⁻⁵⁰ of it, relative to the value itself. Derived, not measured: both round to float64 once (2⁻⁵³ each), the hybrid's long-double
    terms carry 2⁻⁶³ each and its log-weights one more rounding from long double to float64."""
    assert np.finfo(np.longdouble).eps < 1e-18, "long double is no wider than float64 here: psis_row_hybrid is psis_row_mp and pins nothing"
    LL, ref = pr.case(name)
    got = pr.psis_matrix(LL, pr.psis_row_hybrid)
    assert np.array_equal(got["n"], ref["n"]) and np.array_equal(got["tail_len"], ref["tail_len"])
    for k in ("pareto_k", "elpd_loo", "lppd", "ess", "lw"):
        rel = np.max(np.abs(got[k] - ref[k]) / np.abs(ref[k]))
        print(f"{name}: {k} {rel:.2e}")
        assert rel <= 2.0 ** -50, (name, k, rel)


def test_gather_pass():
    assert pr.gather_pass(np.array([-1.0])) == "no select" and pr.gather_pass(np.array([np.nan, -np.inf])) == "no select"
    assert pr.gather_pass(np.full(7, -2.5)) == 0 and pr.gather_pass(np.arange(4096.0)) == 0
    assert pr.gather_pass(np.full(4097, -2.5)) == "never"
    # v = 0 … 4999, M = 213, the cut is u = bits(213): every v >= 2 shares its top byte (4998 > 4096), its top two bytes only [208, 216)
    assert pr.gather_pass(np.arange(5000.0)) == 2
    row = np.arange(5000.0)
    row[::2] = np.inf
    assert pr.gather_pass(row) == 0      # 2500 finite entries
    # the routes the cases of the generator take (the gap EDGE_ROWS closes): pass 0 up to S = 4096, pass 2 above
    for name, (S, R, (c, nu), seed) in pr.CASES.items():
        for row in pr.student_rows(S, R, c, nu, seed):
            assert pr.gather_pass(row) == ("no select" if S == 1 else 0 if S <= pr.MAX_TAIL else 2), name


@pytest.fixture(scope="module")
def base_bars():
    return pr.restatement_bars()


@pytest.mark.parametrize("name", list(pr.EDGE_ROWS))
def test_edge_rows_meet_their_conditions(name, base_bars):
    """edge_case asserts the row's route, tail length, spread, k̂ window and that v − min v makes no new tie; here the restatement is held to
    its own bar on the row as well, and the rows whose tail has a closed form to that."""
    LL, ref, g = pr.edge_case(name)
    bars, gap = pr.edge_bars(name, base_bars)
    print(f"{name}: S {LL.shape[1]}  n {ref['n'][0]:.0f}  gather {g}  tail_len {ref['tail_len'][0]:.0f}  k̂ {ref['pareto_k'][0]:.4f}  restatement's gaps: "
          + "  ".join(f"{k} {v:.2e}" for k, v in gap.items()))
    if name not in pr.ROUTE_ROWS:
        assert all(gap[k] <= base_bars[k] / 100.0 if k in ("pareto_k", "ess") else gap[k] <= 1e-11 for k in gap), (name, gap)
    if name.startswith("const"):
        S = LL.shape[1]
        assert ref["pareto_k"][0] == np.inf and abs(ref["elpd_loo"][0] + 2.5) <= 1e-15 and abs(ref["lppd"][0] + 2.5) <= 1e-15
        assert abs(ref["ess"][0] - S) <= 1e-15 * S and np.max(np.abs(ref["lw"] + np.log(S))) <= 1e-15 * np.log(S)
    if name == "never_tieblock":
        assert ref["tail_len"][0] < pr.tail_len(12000) and np.sort(LL[0])[pr.tail_len(12000)] == -5.0      # the cut lies inside the block
    if name.startswith("dup10"):
        assert np.count_nonzero(LL[0] == LL[0].min()) == 10      # the minimum's key ~u = ~0 is the sort's padding key, ten times


@pytest.mark.parametrize("name", pr.ROUTE_ROWS)
def test_route_rows_bars_cannot_hide_a_wrong_tail(name, base_bars):
    """The per-row bars of the ill-conditioned rows, from the reference side alone: k̂'s is at most K_BAR_CAP, the 100 × gap it comes from
    fits under the cap (so the cap cuts nothing the rule grants), every other field's stays at or below 1e-9, and a cut-off that is off by
    one entry moves k̂ by at least ten bars."""
    bars, gap = pr.edge_bars(name, base_bars)
    sens = pr.cut_sensitivity(name)
    print(f"{name}: bars " + "  ".join(f"{k} {v:.2e}" for k, v in bars.items()) + f"  k̂ moves by {sens:.2e} when the cut moves by one entry")
    assert bars["pareto_k"] <= pr.K_BAR_CAP and 100.0 * gap["pareto_k"] <= pr.K_BAR_CAP
    assert all(bars[k] <= 1e-9 for k in ("ess", "elpd_loo", "lppd", "lw")), bars
    assert sens >= 10.0 * bars["pareto_k"], (name, sens, bars["pareto_k"])


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
