"""
Conditions on the NumPy restatement of the warm-up statistics (tests/adapt_reference.py) that need no device, and the inputs, bars and seeds
tests/test_adapt.py then holds the device to: the grouped moments against exact rational arithmetic, the Chan merge over a three-way split,
the windowed schedule, dual averaging against a transcription of Stan's learn_stepsize, the R̂ identity against the direct formula, the
sensitivity of the warm-up loop to one ulp of its start, and the stationarity of the kernel a warm-up freezes.

The bars on the moments (the issue's): counts exact; |mean − exact| <= n·2⁻⁵³·max|x| of the group's row — (Σx)/n in any summation order
errs by at most (n − 1)·2⁻⁵³·max|x| in the sum and 2⁻⁵³·|mean| in the quotient —; |M2 − exact| <= 1e-10·exact: the two-pass and Chan forms
err by O(n·2⁻⁵³) relative, Σx² − n·mean² by about 1e-6 on the row with mean 5e4 and deviation 0.5.
"""
import math

import numpy as np
import pytest

import adapt_reference as ref
import draws_cases as cases
import hmc_reference as hmc


@pytest.mark.parametrize("G", cases.MOMENT_G)
@pytest.mark.parametrize("K", cases.MOMENT_K)
def test_moments_restatement_against_exact_arithmetic(K, G):
    for W in cases.MOMENT_W:
        x, group = cases.moments_case(W, K, G)
        exact = ref.exact_moments(x, group, G)
        if W >= 63:
            assert exact[0].sum() == W - 2 - (2 if G > 1 else 0)          # the NaN and the Inf chain, ids −1 and G
            if G > 1:
                assert exact[0][1] == 1 and exact[2][1].max() == 0.0     # the single member: M2 = 0
        if G > 1:
            assert exact[0][G - 1] == 0
        worst = cases.check_moments(ref.moments(x, group, G), exact, (W, K, G))
        # the naive form misses the M2 bar on the offset row by decades: the bar separates them
        keep, gid = ref.included(x, group, G)
        v = x[0, keep & (gid == 0)]
        if v.size >= 255:
            naive = np.sum(v * v) - v.size * np.mean(v) ** 2
            assert abs(naive - exact[2][0, 0]) > 100 * cases.M2_BAR * exact[2][0, 0]
        # accumulate: three calls on thirds of the chains against one call on all of them
        held = None
        for a, b in cases.thirds(W):
            part = ref.moments(x[:, a:b], None if group is None else group[a:b], G)
            held = part if held is None else ref.moments(x[:, a:b], None if group is None else group[a:b], G, held=held)
        cases.check_moments(held, exact, (W, K, G, "thirds"))
    print(f"K {K} G {G}: worst mean error / bar {worst[0]:.3f}, worst M2 relative error {worst[1]:.3e} (W = {cases.MOMENT_W[-1]})")


def test_merge_leaves_an_empty_block_and_takes_over_an_empty_state():
    x, group = cases.moments_case(257, 3, 3)
    full = ref.moments(x, group, 3)
    none = ref.moments(x[:, :0], group[:0], 3, held=full)
    assert all(np.array_equal(a, b) for a, b in zip(full, none))
    zero = (np.zeros(3), np.full((3, 3), 7.0), np.full((3, 3), 7.0))      # a count of 0 holds nothing, whatever mean and M2 say
    took = ref.moments(x, group, 3, held=zero)
    assert np.array_equal(took[0], full[0]) and np.array_equal(took[1][:2], full[1][:2]) and np.array_equal(took[1][2], zero[1][2])


def test_metric_restatement():
    m2 = np.array([4.0, 0.0, np.nan, np.inf, 9.0e-4])
    pre = np.full(5, -1.0)
    plain = ref.metric(10.0, m2, pre, regularize=False)
    assert np.array_equal(plain, [4.0 / 9.0, -1.0, -1.0, -1.0, 9.0e-4 / 9.0])
    reg = ref.metric(10.0, m2, pre, regularize=True)
    assert np.allclose(reg[[0, 1, 4]], [(10 / 15) * 4 / 9 + 1e-3 / 3, 1e-3 / 3, (10 / 15) * (9.0e-4 / 9.0) + 1e-3 / 3], rtol=1e-15) and np.array_equal(reg[2:4], [-1.0, -1.0])
    assert np.array_equal(ref.metric(1.0, m2, pre), pre) and np.array_equal(ref.metric(0.0, m2, pre), pre)


@pytest.mark.parametrize("n", (20, 50, 150, 1000))
def test_warmup_windows_tile_the_rounds(pkg, n):
    init, windows, term = ref.warmup_windows(n)
    assert init + sum(windows) + term == n and init >= 0 and term >= 0 and all(w > 0 for w in windows)      # no gap, no overlap
    assert all(b >= a for a, b in zip(windows, windows[1:]))
    flags = ref.round_flags(n)
    assert [f[0] for f in flags] == [False] * init + [True] * sum(windows) + [False] * term
    assert sum(f[1] for f in flags) == sum(f[2] for f in flags) == len(windows)
    if n == 1000:
        assert (init, windows, term) == (75, [25, 50, 100, 200, 500], 50)
    assert pkg.warmup_windows(n) == (init, windows, term)


def test_warmup_windows_of_the_package_are_the_restatement(pkg):
    for n in range(0, 1200):
        assert pkg.warmup_windows(n) == ref.warmup_windows(n), n
    assert ref.warmup_windows(19) == (19, [], 0)


def test_dual_averaging_is_stans_learn_stepsize():
    rng = np.random.default_rng(5)
    a_seq = np.concatenate([rng.uniform(0, 1, 40), [0.0, 1.0, 1.0, 0.0]])
    for eps0 in (0.1, 2.5e-3):
        stan = ref.learn_stepsize_stan(a_seq, eps0)
        state = ref.adapt_init(eps0)
        assert np.array_equal(state[0], [math.log(eps0), math.log(eps0), 0.0, math.log(10 * eps0)])
        for k, a in enumerate(a_seq, start=1):
            # one chain whose dH gives exactly this acceptance probability: a = 0 and 1 through the NaN branch
            dH, acc = (np.array([np.nan]), np.array([int(a)])) if a in (0.0, 1.0) else (np.array([math.log(a)]), np.array([0]))
            state, a_g = ref.adapt_step(state, dH, acc, k)
            assert abs(a_g[0] - a) <= 2 * cases.U
            eps, eps_bar = stan[k - 1]
            assert abs(math.exp(state[0, 0]) - eps) <= 1e-12 * eps and abs(math.exp(state[0, 1]) - eps_bar) <= 1e-12 * eps_bar, k


def test_dual_averaging_case_is_defined_everywhere():
    for G in (1, 8):
        dH, acc, group = cases.dual_averaging_case(G)
        a = ref.accept_prob(dH, acc)
        assert np.all((a >= 0) & (a <= 1)) and a[5] == 1.0 and a[72] == 0.0 and a[3] == 1.0 and a[4] == 0.0 and a[6] == 1.0
        state, a_g = ref.adapt_step(ref.adapt_init(0.1, G), dH, acc, 1, group)
        assert np.all(np.isfinite(state)) and (G == 1 or (np.isnan(a_g[G - 2]) and np.isfinite(np.delete(a_g, G - 2)).all()))
        if G > 1:
            assert np.array_equal(state[G - 2], ref.adapt_init(0.1, G)[G - 2])
            e = ref.eps_of(state, group, cases.DA_W)
            assert np.isnan(e[9]) and np.isnan(e[200]) and np.isfinite(np.delete(e, [9, 200])).all()


def test_rhat_identity_against_the_direct_formula():
    s = cases.rhat_case()
    cmean = cm2 = None
    for k in range(1, cases.RHAT_N + 1):
        cmean, cm2 = ref.chain_moments(s[k - 1], k, cmean, cm2)
    ok = np.arange(cases.RHAT_W) != 100
    assert np.all(np.isnan(cmean[3, 100])) and np.all(np.isnan(cm2[3, 100]))      # the chain with the NaN carries it
    assert np.allclose(cmean[:, ok], s[:, :, ok].mean(axis=0), rtol=1e-13, atol=0) and np.allclose(cm2[:, ok], s[:, :, ok].var(axis=0) * cases.RHAT_N, rtol=1e-12)
    r, direct = ref.rhat(cmean, cm2, cases.RHAT_N), ref.rhat_direct(s)
    assert np.all(np.abs(r - direct) <= 1e-10 * direct) and np.all((r > 0.9) & (r < 1.5))


# ---------------------------------------------------------------------------------------------------- the warm-up loop on the prior
def loop_start():
    return hmc.prior_sample(cases.STAT_PRIORS, cases.LOOP_SEED, np.arange(cases.LOOP_W, dtype=np.uint64))[1]


def test_warmup_loop_sensitivity_to_one_ulp():
    start = loop_start()
    run = lambda tt: ref.hmc_warmup(cases.STAT_PRIORS, tt, cases.LOOP_WARMUP, cases.LOOP_LEAPFROG, cases.LOOP_EPS, np.ones(5), cases.LOOP_SEED)      # noqa: E731
    a, b = run(start), run(np.nextafter(start, np.inf))
    s = cases.loop_deviation(b, a)
    print(f"warm-up loop, start moved by one ulp: s = {s:.3e}; ε {a['eps']:.6f}, inv_mass {a['inv_mass']}, acceptance {a['accept_stat'].mean():.3f}")
    assert np.array_equal(a["accepted"], b["accepted"])
    assert s <= cases.LOOP_S
    assert not np.array_equal(a["inv_mass"], np.ones(5)) and 0.3 < a["accept_stat"][-5:].mean() <= 1.0


# cases.FROZEN_SEEDS are the first two of these for which the restatement stays under the bar
FROZEN_CANDIDATES = (21, 22)


def test_frozen_kernel_is_stationary():
    passed = []
    for seed in FROZEN_CANDIDATES:
        wu, (stat, acc) = cases.frozen_reference(seed)
        print(f"seed {seed}: warm-up ε {wu['eps']:.5f} inv_mass {np.array2string(wu['inv_mass'], precision=4)}; fresh batch max D_n {stat:.3e} "
              f"(bar {cases.STAT_BAR:.3e}), acceptance {acc:.4f}")
        if stat < cases.STAT_BAR:
            passed.append(seed)
    assert tuple(passed[:2]) == cases.FROZEN_SEEDS
