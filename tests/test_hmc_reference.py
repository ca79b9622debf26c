"""
Conditions on the NumPy restatement of the tempered HMC step (tests/hmc_reference.py) that need no device: the generator's new purposes
against numpy.random.Philox, the momenta, and the two stationarity conditions the GPU tests of tests/test_hmc.py then hold the device to
with the same seeds — the step leaves the prior invariant at β = 0 (one-sample KS against scipy, and two deliberately broken samplers
fail the same bar), and it leaves the posterior invariant at β = 1 (two-sample KS between two independent batches of exact posterior
draws made by rejection, one of them pushed through eight steps), the log-posterior being the oracle's callback. The seeds, inputs, bars
and statistics are those of tests/draws_cases.py.
"""
import ctypes as C
import math

import numpy as np
import pytest

import draws_cases as cases
import hmc_reference as ref


# ---------------------------------------------------------------------------------------------------- generator and momenta
def test_philox_purposes_are_numpy_philox():
    """numpy.random.Philox(counter=c, key=k) hands out the block of counter c + 1 first."""
    cases = [((21, ref.KEY1), ref.counter(ref.PURPOSE_MOMENTUM, 5, d=9, step=7)), ((22, ref.KEY1), ref.counter(ref.PURPOSE_ACCEPT, (1 << 40) + 3, step=0)),
             ((0xDEADBEEFCAFEF00D, ref.KEY1), ref.counter(ref.PURPOSE_MOMENTUM, ref.M64, d=63, step=ref.M64)),
             ((3, ref.KEY1), ref.counter(ref.PURPOSE_ACCEPT, 0, step=(1 << 63) + 11))]
    for key, ctr in cases:
        assert ctr[2] in (2, 3)
        n = sum(c << (64 * k) for k, c in enumerate(ctr)) - 1      # the counter before it: NumPy increments first
        prev = tuple((n >> (64 * k)) & ref.M64 for k in range(4))
        raw = np.random.Philox(counter=np.array(prev, dtype=np.uint64), key=np.array(key, dtype=np.uint64)).random_raw(4)
        assert tuple(int(x) for x in raw) == ref.philox_int(key, ctr), (key, ctr)
        vec = ref.philox_vec(key, *[np.array([c], dtype=np.uint64) for c in ctr])
        assert tuple(int(v[0]) for v in vec) == ref.philox_int(key, ctr), (key, ctr)
    # the vector helpers use exactly these counters
    seed, step, chain0, D = 21, 7, (1 << 40) + 3, 11
    u = ref.momentum_uniforms(seed, step, chain0, 3, D)
    for w in range(3):
        for d in range(D):
            word = ref.philox_int((seed, ref.KEY1), ref.counter(ref.PURPOSE_MOMENTUM, chain0 + w, d=d, step=step))[d % 4]
            assert u[d, w] == (2 * (word >> 12) + 1) * 2.0 ** -53
        word = ref.philox_int((seed, ref.KEY1), ref.counter(ref.PURPOSE_ACCEPT, chain0 + w, step=step))[0]
        assert ref.accept_uniforms(seed, step, chain0, 3)[w] == (2 * (word >> 12) + 1) * 2.0 ** -53


def test_counters_of_the_four_purposes_never_coincide():
    """Word 2 of the counter is the purpose; purposes 0 and 1 keep word 3 = 0, so the streams that existed do not move."""
    idx, blocks, steps = (0, 1, 5, (1 << 40) + 3, ref.M64), range(16), (0, 1, 7, ref.M64)
    seen = {}
    for i in idx:
        for j in blocks:
            for purpose in (ref.PURPOSE_PRIOR, ref.PURPOSE_UNIFORM):
                seen.setdefault(ref.counter(purpose, i, d=4 * j), set()).add(purpose)
            for step in steps:
                for purpose in (ref.PURPOSE_MOMENTUM, ref.PURPOSE_ACCEPT):
                    seen.setdefault(ref.counter(purpose, i, d=4 * j, step=step), set()).add(purpose)
    assert all(len(v) == 1 for v in seen.values())
    assert all(c[3] == 0 for c, v in seen.items() if v & {ref.PURPOSE_PRIOR, ref.PURPOSE_UNIFORM})
    with pytest.raises(AssertionError):
        ref.counter(ref.PURPOSE_PRIOR, 0, step=1)
    # and the words differ: the momentum of chain 0 at step 0 is not the prior draw 0, the acceptance uniform not the rejection uniform
    i = np.arange(64, dtype=np.uint64)
    assert not np.any(ref.block_uniforms(5, i, 4, ref.PURPOSE_MOMENTUM) == ref.prior_uniforms(5, i, 4))
    assert not np.any(ref.accept_uniforms(5, 0, 0, 64) == ref.rejection_uniforms(5, i))


def test_momentum_normals_are_ndtri_of_the_uniforms():
    from scipy.special import ndtri
    import scipy.stats as ss
    seed, step, chain0, W, D = 9, 3, 17, 1 << 16, 5
    im = np.array([3.3, 3.3, 0.0025, 3.3, 1.0])
    u = ref.momentum_uniforms(seed, step, chain0, W, D)
    assert np.all((u > 0) & (u < 1))
    p = ref.momentum(seed, step, chain0, W, D, im)
    assert np.array_equal(p, ndtri(u) / np.sqrt(im)[:, None]) and np.array_equal(ref.momentum(seed, step, chain0, W, D), ndtri(u))
    for d in range(D):      # … and they are standard normals: one-sample KS at the 0.1 % bar
        z = np.sort(p[d] * math.sqrt(im[d]))
        F = ss.norm.cdf(z)
        k = np.arange(1, W + 1)
        assert max(np.max(k / W - F), np.max(F - (k - 1) / W)) < 1.95 / math.sqrt(W)


# ---------------------------------------------------------------------------------------------------- β = 0: the prior is stationary
def run_stationarity(seed, eps, n_leapfrog, **variant):
    _, tt = ref.prior_sample(cases.STAT_PRIORS, seed, np.arange(cases.STAT_W, dtype=np.uint64))
    acc = []
    for step in range(cases.STAT_STEPS):
        r = ref.hmc_step(cases.STAT_PRIORS, tt, None, eps, n_leapfrog, cases.STAT_INV_MASS, seed, step, **variant)
        tt = r["theta_t"]
        acc.append(r["accepted"].mean())
    return cases.stationarity_statistics(tt), float(np.mean(acc))


@pytest.mark.parametrize("eps,n_leapfrog", cases.STAT_SETTINGS)
def test_prior_is_stationary_and_broken_samplers_are_not(eps, n_leapfrog):
    for seed in cases.STAT_SEEDS:
        stat, acc = run_stationarity(seed, eps, n_leapfrog)
        print(f"seed {seed} (ε {eps}, L {n_leapfrog}): correct      acceptance {acc:.3f} max D_n {stat:.3e} (bar {cases.STAT_BAR:.3e})")
        assert stat < cases.STAT_BAR and acc >= 0.6, (seed, stat, acc)
        for name, variant in (("always accepts", dict(always_accept=True)), ("no mass in K ", dict(mass_in_K=False))):
            bad, acc_b = run_stationarity(seed, eps, n_leapfrog, **variant)
            print(f"seed {seed} (ε {eps}, L {n_leapfrog}): {name} acceptance {acc_b:.3f} max D_n {bad:.3e}")
            assert bad > cases.STAT_BAR, (seed, name, bad)


# ---------------------------------------------------------------------------------------------------- β = 1: the posterior is stationary
@pytest.mark.parametrize("seed", cases.POST_SEEDS)
def test_posterior_is_stationary(oracle, seed):
    om = cases.oracle_model(oracle)
    a, b = (cases.rejection_batch(oracle, om, seed, first) for first in cases.POST_FIRST)
    im = cases.posterior_inv_mass(b)
    logpost = cases.oracle_logpost(oracle, om)

    def step_fn(tt, step):
        r = ref.hmc_step(cases.MODEL_PRIORS, tt, None, cases.POST_EPS, cases.POST_LEAPFROG, im, seed, step, logpost=logpost)
        return r["theta_t"], r["accepted"]

    cases.check_posterior_stationary(a, b, step_fn, f"seed {seed} (CPU)")


# ---------------------------------------------------------------------------------------------------- one step: the condition on its seed
def test_one_step_flags_are_decided_for_the_seed(oracle):
    """The GPU test compares acceptance flags wherever |dH − log u| > 1e-6 and may leave out at most 1 % of the chains: that holds for its
    seed, from the reference alone (at the restated prior draws; the device's differ in the last bits)."""
    beta, eps, im = cases.step_inputs()
    _, start = ref.prior_sample(cases.MODEL_PRIORS, cases.STEP_SEED, np.arange(cases.STEP_W, dtype=np.uint64))
    logpost = cases.oracle_logpost(oracle, cases.oracle_model(oracle))
    for n_leapfrog in (1, 3):
        r = ref.hmc_step(cases.MODEL_PRIORS, start, beta, eps, n_leapfrog, im, cases.STEP_SEED, cases.STEP_STEP, logpost=logpost)
        close = np.abs(r["dH"] - r["log_u"]) <= 1e-6
        print(f"L {n_leapfrog}: acceptance {r['accepted'].mean():.3f}, {close.sum()} of {cases.STEP_W} chains within 1e-6 of the decision, max |E| {np.max(np.abs(r['E0'])):.3e}")
        assert close.mean() <= 0.01 and 0.2 < r["accepted"].mean() < 0.98 and np.all(np.isfinite(r["proposal"]))


# ---------------------------------------------------------------------------------------------------- argument checks without a device
def test_argument_checks_that_need_no_device(pkg):
    """Without a device no handle can be made, so these go through the NULL handle, which is refused before anything else; the same
    arguments on a real handle are in tests/test_hmc.py."""
    from __graft_entry__ import build_draws, build_hip
    build_hip()
    build_draws()
    from octofitter_jl_amd.host import draws
    lib, EINVAL = draws.load_library(), pkg.capi.OCTO_EINVAL
    acc = (C.c_int32 * 4)()
    th = np.zeros((2, 4))
    assert lib.octo_draws_momentum_device(None, 0, 0, 0, 4, 4, None, None, None) == EINVAL
    assert lib.octo_draws_hmc_step_device(None, 0, 0, 0, 4, 4, None, None, None, 0.1, 1, None, None, None, None, None, None, None) == EINVAL
    assert lib.octo_draws_hmc_step(None, 0, 0, 0, 4, 4, pkg.capi._dptr(th), None, None, 0.1, 1, None, None, None, None, None, acc) == EINVAL
    assert lib.octo_draws_hmc_step(None, 0, 0, 0, 4, 4, pkg.capi._dptr(th), None, None, 0.1, 0, None, None, None, None, None, acc) == EINVAL      # n_leapfrog = 0
    assert lib.octo_draws_hmc_step(None, 0, 0, 0, 4, 3, pkg.capi._dptr(th), None, None, 0.1, 1, None, None, None, None, None, acc) == EINVAL      # ld < W
