"""
The restatement of the convergence diagnostics (tests/diag_reference.py) pinned by its meaning — ArviZ and posterior are not at hand, so what
the numbers must say of chains whose behaviour is known stands in for them — and the condition the GPU suite rests on: every case of
tests/diag_cases.py keeps its decision margins (the smallest |even + odd| of Geyer's tests, the smallest gap of a monotone comparison) above
1e-6, seven orders above the arithmetic's error, so the device and the restatement take the same branches. The seeds are fixed. At n = 400 and
W = 64 the AR(1) figures scatter from seed to seed (φ = 0.9: ess_basic/S between 0.039 and 0.060 over eight seeds against (1 − φ)/(1 + φ) =
0.0526; the estimator's ρ̂ tends to 1 − W̄/var⁺ > 0 at long lags of short chains); the bar is 20 % at that size. CPU suite: no GPU.
"""
import math

import numpy as np
import pytest
from scipy.stats import rankdata

import diag_cases as cases
import diag_reference as ref

N, W = 400, 64
S = N * W


def stats_of(x):
    return ref.diagnose(x)["stats"]


def test_iid_normal_draws_have_full_ess_and_rhat_one():
    s = stats_of(cases.ar1(np.random.default_rng(100), N, 3, W, 0.0))
    for name in ("ESS_BULK", "ESS_TAIL", "ESS_BASIC"):
        assert np.all(np.abs(s[getattr(ref, name)] / S - 1.0) < 0.1), (name, s[getattr(ref, name)] / S)
    assert np.all(np.abs(s[ref.RHAT] - 1.0) < 0.01) and np.all(np.abs(s[ref.RHAT_BASIC] - 1.0) < 0.01), s[[ref.RHAT, ref.RHAT_BASIC]]
    assert np.all(np.abs(s[ref.Q50]) < 0.05) and np.all(np.abs(s[ref.Q05] + 1.645) < 0.05) and np.all(np.abs(s[ref.Q95] - 1.645) < 0.05)


@pytest.mark.parametrize("row,phi", [(0, 0.5), (1, 0.9)])
def test_ar1_ess_is_near_its_closed_form(row, phi):
    s = stats_of(cases.ar1(np.random.default_rng(101), N, 2, W, (0.5, 0.9)))
    got, want = s[ref.ESS_BASIC, row] / S, (1.0 - phi) / (1.0 + phi)
    print(f"phi = {phi}: ess_basic/S = {got:.4f} against {want:.4f}")
    assert abs(got / want - 1.0) < 0.2, (got, want)


def test_antithetic_chains_have_ess_above_s_and_the_cap_holds():
    s = stats_of(cases.ar1(np.random.default_rng(102), N, 2, W, (-0.5, -0.99)))
    assert S < s[ref.ESS_BASIC, 0] <= S * math.log10(S), s[ref.ESS_BASIC]
    assert s[ref.ESS_BASIC, 1] == pytest.approx(S * math.log10(S), rel=1e-12), s[ref.ESS_BASIC]      # τ at its floor 1/log10(S)


def test_a_shifted_chain_raises_rhat():
    x = cases.ar1(np.random.default_rng(103), N, 1, 4, 0.0)
    x[:, 0, 2] += 3.0
    s = stats_of(x)
    print(f"one chain of four shifted by 3 sigma: rhat = {s[ref.RHAT, 0]:.3f}, rhat_basic = {s[ref.RHAT_BASIC, 0]:.3f}")
    assert s[ref.RHAT, 0] > 1.1 and s[ref.RHAT_BASIC, 0] > 1.1, s[:, 0]


def test_a_scale_difference_is_caught_by_the_folded_rhat_alone():
    x = cases.ar1(np.random.default_rng(104), N, 1, 4, 0.0)
    x[:, 0, 1] *= 4.0
    v = ref.used(x)[0]
    _, z = ref.normal_scores(v)
    _, zf = ref.normal_scores(np.abs(v - np.median(v)))
    bulk, folded = ref.rhat(z), ref.rhat(zf)
    print(f"one chain of four scaled by 4: bulk {bulk:.4f}, folded {folded:.4f}")
    assert bulk < 1.01 < 1.1 < folded
    assert stats_of(x)[ref.RHAT, 0] == pytest.approx(folded, rel=1e-6)      # the median of the statement is q_0.5: here the same value up to its interpolation


def test_ties_get_average_ranks():
    for name in ("ties", "signed_zero", "censored"):
        x, r = cases.draws(name), cases.reference(name)
        for k in range(x.shape[1]):
            v = ref.used(x)[k]
            want = rankdata(v, method="average", axis=None).reshape(v.shape)
            assert np.array_equal(ref.used(r["rank"])[k], want), (name, k)
    z = ref.used(cases.reference("signed_zero")["rank"])[0][ref.used(cases.draws("signed_zero"))[0] == 0.0]
    assert z.size > 1 and np.all(z == z[0])      # −0 and +0 share one rank


def tie_runs(s, longer_than):
    """[(first key, length)] of the runs of equal keys of the sorted s that are longer than `longer_than`"""
    _, first, count = np.unique(s, return_index=True, return_counts=True)
    return [(int(f), int(c)) for f, c in zip(first, count) if c > longer_than]


def test_long_chain_walks_rho_beyond_the_lags_held_in_lds():
    """what the case is for: T > 1024 puts ρ_t into the work array, and row 0's Geyer loops run past lag 1024 while row 1's stop early"""
    n, Wc, K = cases.CASES["long_chain"][2]
    T = -(-(n // 2) // ref.LAG_BLOCK) * ref.LAG_BLOCK
    assert T == 1056 and T > 1024 and (n // 2) % ref.LAG_BLOCK
    m = cases.reference("long_chain")["margins"]
    print("long_chain: max_t of " + ", ".join(ref.Margins.QUANTITIES) + f": row 0 {m.max_t[0]}, row 1 {m.max_t[1]}")
    assert len(m.max_t[0]) == 4 and all(t is not None and t > 1024 for t in m.max_t[0]), m.max_t[0]
    assert len(m.max_t[1]) == 4 and all(t is not None and t < 16 for t in m.max_t[1]), m.max_t[1]


def test_censored_has_tie_runs_longer_than_a_sort_block_at_both_ends_and_no_tail_ess():
    x, r = cases.draws("censored"), cases.reference("censored")
    v = ref.used(x)
    S = v[0].size
    assert S == 5120
    runs = [tie_runs(np.sort(v[k], axis=None), 100) for k in range(2)]
    print(f"censored: tie runs (first key, length) of row 0 {runs[0]}, of row 1 {runs[1]}")
    assert runs[0] == [(0, 2135), (2943, 2177)] and runs[1] == [(4303, 817)]
    assert all(c > ref.SORT_BLOCK for _, c in runs[0])                               # each crosses a sort block whole
    assert runs[0][0][0] == 0 and sum(runs[0][1]) == S and sum(runs[1][0]) == S      # one begins at key 0, two end at key S
    s = r["stats"]
    assert np.array_equal(s[ref.Q95], [x[:, 0].max(), x[:, 1].max()]) and np.array_equal(s[ref.Q95], [0.2, 1.0])
    assert np.all(np.isnan(s[ref.ESS_TAIL])) and not np.any(np.isnan(np.delete(s, ref.ESS_TAIL, axis=0)))
    assert all(r["margins"].max_t[k][2] is None and None not in r["margins"].max_t[k][:2] for k in range(2))      # 1[x <= q95] is constant; 1[x <= q05] is not


def test_stuck_chain_has_one_chain_of_zero_variance_in_a_valid_row():
    x, r = cases.draws("stuck_chain"), cases.reference("stuck_chain")
    assert np.all(x[:, 1, 2] == 0.7) and sum(bool(np.all(x[:, k, w] == x[0, k, w])) for k in range(2) for w in range(5)) == 1
    assert not np.any(np.isnan(r["stats"]))
    z = ref.used(r["z"])[1]
    assert np.all(z[[2, 7]] == z[2, 0]) and np.all(ref.used(r["rank"])[1][[2, 7]] == ref.used(r["rank"])[1][2, 0])      # both halves of it: N tied ranks each, one z
    print(f"stuck_chain: rhat of row 1 {r['stats'][ref.RHAT, 1]:.4f}")
    assert 1.05 < r["stats"][ref.RHAT, 1] < 1.2


def test_odd_n_drops_the_middle_sample():
    x = np.array(cases.draws("odd_n"))
    want = cases.reference("odd_n")
    x[4] = 1e9
    got = ref.diagnose(x)
    assert np.array_equal(got["stats"], want["stats"]) and np.all(np.isnan(got["rank"][4])) and not np.any(np.isnan(got["rank"][[3, 5]]))


@pytest.mark.parametrize("name", sorted(cases.INVALID_ROWS))
def test_invalid_rows_are_nan_and_the_others_are_not(name):
    r, bad = cases.reference(name), cases.INVALID_ROWS[name]
    K = r["stats"].shape[1]
    good = [k for k in range(K) if k not in bad]
    assert np.all(np.isnan(r["stats"][:, bad])) and np.all(np.isnan(r["z"][:, bad])) and np.all(np.isnan(r["rank"][:, bad]))
    assert not np.any(np.isnan(r["stats"][:, good])) and not np.any(np.isnan(r["z"][:, good]))


def test_chain_sum_is_the_documented_order_and_a_sum():
    rng = np.random.default_rng(105)
    for M in (1, 2, 63, 64, 65, 256, 257, 514, 2200):
        v = rng.standard_normal(M)
        pad = np.zeros(-(-M // 256) * 256)
        pad[:M] = v
        total = 0.0
        for block in pad.reshape(-1, 4, 64):
            t = 0.0
            for wave in block:
                a = wave.copy()
                for o in (32, 16, 8, 4, 2, 1):
                    a = np.array([a[lane] + a[lane ^ o] for lane in range(64)])
                assert np.all(a == a[0])
                t += a[0]
            total += t
        assert ref.chain_sum(v) == total and abs(total - math.fsum(v)) < 1e-12 * max(1.0, M)
    assert np.array_equal(ref.chain_sum(np.ones((3, 5, 300))), np.full((3, 5), 300.0))


def test_work_size_is_the_sum_of_its_parts():
    n, Wc, K = 35, 257, 3
    Nh, M = 17, 514
    Sc, P, T, nblk = M * Nh, 16384, 32, 3
    assert ref.work_doubles(n, Wc, K) == 2 * K * P + 2 * K * Sc + 2 * 5 * K * M + 4 * K * T * nblk + 4 * K * T + 3 * K + 2 * K


@pytest.mark.parametrize("name", list(cases.CASES))
def test_every_gpu_case_keeps_its_decision_margins(name):
    m = cases.reference(name)["margins"]
    print(f"{name}: Geyer margin {m.geyer:.3e}, monotone margin {m.monotone:.3e}")
    assert m.geyer >= cases.MARGIN_BAR and m.monotone >= cases.MARGIN_BAR, (name, m.geyer, m.monotone)


def test_the_finite_twin_is_nan_and_inf_without_its_two_entries_and_keeps_its_margins():
    a, b = cases.draws("nan_and_inf"), cases.draws("nan_and_inf_finite")
    assert a.shape == b.shape and np.all(np.isfinite(b)) and int(np.sum(a != b)) == 2 and not np.isfinite(a[3, 1, 2]) and not np.isfinite(a[9, 3, 0])
    r = cases.reference("nan_and_inf_finite")
    m = r["margins"]
    print(f"nan_and_inf_finite: Geyer margin {m.geyer:.3e}, monotone margin {m.monotone:.3e}")
    assert not np.any(np.isnan(r["stats"])) and m.geyer >= cases.MARGIN_BAR and m.monotone >= cases.MARGIN_BAR
    for k in (0, 2):      # the rows the poison did not touch are the same rows
        assert np.array_equal(r["stats"][:, k], cases.reference("nan_and_inf")["stats"][:, k])


def test_shapes_of_the_cases_are_the_listed_ones():
    listed = {(8, 1, 1), (9, 3, 2), (35, 257, 3), (400, 64, 2), (130, 1100, 1), (16, 2, 64), (2082, 3, 2), (80, 64, 2), (24, 5, 2)}
    edges = {(2 * Nh + Nh % 2, Wc, 2) for Nh in (15, 16, 17, 31, 32, 33) for Wc in (32, 33, 128, 129)}
    assert len(edges) == 24 and len(cases.EDGES) == 24 and len(cases.CASES) == 37
    assert listed | edges <= {shape for _, _, shape in cases.CASES.values()}
    assert {2 * Wc * (n // 2) for n, Wc, _ in edges} >= {2048, 4096, 8192}      # S a power of two: no padding behind the keys
    assert [(name, seed) for name, seed, _ in cases.EDGES][:2] == [("edge_N15_W32", 41), ("edge_N15_W33", 42)] and cases.CASES["edge_N16_W128"][2] == (32, 128, 2)
    for name in cases.CASES:
        cases.draws(name)


def test_recorded_gaps_are_the_ones_the_bars_are_written_from():
    """profiles/diag_throughput.txt records the long-double gaps; tests/diag_cases.py holds the same figures"""
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "profiles" / "diag_throughput.txt").read_text()
    for stat, gap in cases.LONG_DOUBLE_GAP.items():
        line = [ln.split() for ln in text.splitlines() if ln.split()[:2] == ["gap", stat]]
        assert len(line) == 1 and float(line[0][2]) == gap, (stat, line, gap)
        assert 0.0 < gap < 1e-10, (stat, gap)      # float64 arithmetic of well-conditioned sums: far below any statistical meaning
