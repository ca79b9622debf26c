"""
Conditions on the NumPy restatement of the tempered HMC step (tests/hmc_reference.py) that need no device: the generator's new purposes
against numpy.random.Philox, the momenta, and the two stationarity conditions the GPU tests of tests/test_hmc.py then hold the device to
with the same seeds — the step leaves the prior invariant at β = 0 (one-sample KS against scipy, and two deliberately broken samplers
fail the same bar), and it leaves the posterior invariant at β = 1 (two-sample KS between two independent batches of exact posterior
draws made by rejection, one of them pushed through eight steps), the log-posterior being the oracle's callback.

The bars: 1.95/√n is the 0.1 % critical value of the one-sample Kolmogorov-Smirnov statistic (tests/test_prior_draws.py), and
1.95·√((n_A + n_B)/(n_A·n_B)) its two-sample form.
"""
import ctypes as C
import math

import numpy as np
import pytest

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
STAT_PRIORS = [ref.prior(ref.UNIFORM, -3, 7), ref.prior(ref.LOGUNIFORM, 0.1, 1000), ref.prior(ref.NORMAL, 1.2, 0.05), ref.prior(ref.SINE),
               ref.prior(ref.TRUNCNORMAL, 0, 1, lo=3)]
STAT_W = 65536
STAT_INV_MASS = (3.3, 3.3, 0.0025, 3.3, 1.0)
STAT_STEPS = 6
STAT_SEEDS = (21, 22)
STAT_SETTINGS = ((0.5, 4), (0.8, 3))      # (ε, n_leapfrog)
STAT_BAR = 1.95 / math.sqrt(STAT_W)


def ks_statistic(x, cdf):
    """One-sample Kolmogorov-Smirnov D_n."""
    F = np.sort(cdf(np.asarray(x)))
    n = F.size
    k = np.arange(1, n + 1)
    return max(np.max(k / n - F), np.max(F - (k - 1) / n))


def ks_two_sample(x, y):
    x, y = np.sort(x), np.sort(y)
    both = np.concatenate([x, y])
    return np.max(np.abs(np.searchsorted(x, both, side="right") / x.size - np.searchsorted(y, both, side="right") / y.size))


def stationarity_statistics(theta_t):
    """max over the coordinates of D_n of invlink(θ_t) against the prior's CDF"""
    return max(ks_statistic(ref.invlink(pr, theta_t[d])[0], ref.scipy_dist(pr)[0]) for d, pr in enumerate(STAT_PRIORS))


def run_stationarity(seed, eps, n_leapfrog, **variant):
    _, tt = ref.prior_sample(STAT_PRIORS, seed, np.arange(STAT_W, dtype=np.uint64))
    acc = []
    for step in range(STAT_STEPS):
        r = ref.hmc_step(STAT_PRIORS, tt, None, eps, n_leapfrog, STAT_INV_MASS, seed, step, **variant)
        tt = r["theta_t"]
        acc.append(r["accepted"].mean())
    return stationarity_statistics(tt), float(np.mean(acc))


@pytest.mark.parametrize("eps,n_leapfrog", STAT_SETTINGS)
def test_prior_is_stationary_and_broken_samplers_are_not(eps, n_leapfrog):
    for seed in STAT_SEEDS:
        stat, acc = run_stationarity(seed, eps, n_leapfrog)
        print(f"seed {seed} (ε {eps}, L {n_leapfrog}): correct      acceptance {acc:.3f} max D_n {stat:.3e} (bar {STAT_BAR:.3e})")
        assert stat < STAT_BAR and acc >= 0.6, (seed, stat, acc)
        for name, variant in (("always accepts", dict(always_accept=True)), ("no mass in K ", dict(mass_in_K=False))):
            bad, acc_b = run_stationarity(seed, eps, n_leapfrog, **variant)
            print(f"seed {seed} (ε {eps}, L {n_leapfrog}): {name} acceptance {acc_b:.3f} max D_n {bad:.3e}")
            assert bad > STAT_BAR, (seed, name, bad)


# ---------------------------------------------------------------------------------------------------- β = 1: the posterior is stationary
# The test model of tests/test_hmc.py: one planet on the parameterisation of tests/test_model.py (Visual{KepOrbit}, UniformCircular angles, tp
# from θ) with 12 RA/Dec epochs and 8 absolute-RV rows. MODEL_NAMES is the order the mirror declares the parameters in; the GPU test asserts
# that the mirror's priors and sources are these.
MODEL_NAMES = ["M", "plx", "rv_offset", "rv_jitter", "b_a", "b_e", "b_i", "b_ωx", "b_ωy", "b_Ωx", "b_Ωy", "b_θx", "b_θy", "b_mass"]
MODEL_PRIORS = [ref.prior(ref.TRUNCNORMAL, 1.2, 0.05, lo=0.1), ref.prior(ref.TRUNCNORMAL, 50.0, 0.1, lo=0.1), ref.prior(ref.NORMAL, 0.0, 20.0),
                ref.prior(ref.LOGUNIFORM, 0.1, 20.0), ref.prior(ref.LOGUNIFORM, 5.0, 20.0), ref.prior(ref.UNIFORM, 0.0, 0.6), ref.prior(ref.SINE)] + \
               [ref.prior(ref.NORMAL, 0.0, 1.0)] * 6 + [ref.prior(ref.LOGUNIFORM, 1.0, 50.0)]
SRC_CONST, SRC_THETA, SRC_CIRCULAR, SRC_TPERI, FLAG_UNITLEN = 0, 1, 2, 3, 1
MODEL_ESRC = [(SRC_THETA, 4, 0, 0, 0.0), (SRC_THETA, 5, 0, 0, 0.0), (SRC_THETA, 6, 0, 0, 0.0), (SRC_CIRCULAR, 7, 8, FLAG_UNITLEN, 2 * math.pi),
              (SRC_CIRCULAR, 9, 10, FLAG_UNITLEN, 2 * math.pi), (SRC_TPERI, 11, 12, FLAG_UNITLEN, 50000.0), (SRC_THETA, 0, 0, 0, 0.0),
              (SRC_THETA, 1, 0, 0, 0.0), (SRC_THETA, 13, 0, 0, 0.0)]
MODEL_NSRC = [(SRC_CONST, 0, 0, 0, 0.0), (SRC_CONST, 0, 0, 0, 1.0), (SRC_CONST, 0, 0, 0, 0.0), (SRC_THETA, 2, 0, 0, 0.0), (SRC_THETA, 3, 0, 0, 0.0),
              (SRC_CONST, 0, 0, 0, 0.0)]
MODEL_SIGMA_ASTROM, MODEL_SIGMA_RV = 3000.0, 600.0      # [mas], [m/s]: wide enough that rejection from the prior accepts >= 2 000 of 2²⁰ draws
POST_N = 1 << 20
POST_FIRST = (0, 1 << 20)       # batches A and B: two disjoint windows of the stream of one seed
POST_SEEDS = (31, 32)
POST_STEPS, POST_EPS, POST_LEAPFROG = 8, 0.15, 4
POST_LEAST = 2000


def model_tables():
    """(astrometry table, RV table) as the mirror's observation classes take them"""
    import synth
    rng = np.random.default_rng(17)
    t = 50000.0 + 90.0 * np.arange(12)
    ra, dec = synth.truth_radec(t)
    astrom = dict(epoch=t, ra=ra + rng.normal(0, 60.0, 12), dec=dec + rng.normal(0, 60.0, 12), σ_ra=np.full(12, MODEL_SIGMA_ASTROM), σ_dec=np.full(12, MODEL_SIGMA_ASTROM))
    rv = dict(epoch=t[:8] + 7.0, rv=rng.normal(0, 30, 8), σ_rv=np.full(8, MODEL_SIGMA_RV))
    return astrom, rv


def oracle_model(oracle):
    """What oracle_model_logpost takes for the test model, built without a device."""
    astrom, rv = model_tables()
    obs = [dict(kind=0, planet=0, epoch=astrom["epoch"], y1=astrom["ra"], y2=astrom["dec"], s1=astrom["σ_ra"], s2=astrom["σ_dec"], cor=None, extra=None),
           dict(kind=2, planet=-1, epoch=rv["epoch"], y1=rv["rv"], y2=None, s1=rv["σ_rv"], s2=None, cor=None, extra=None)]
    planets = [dict(orbit_kind=0, has_mass=True)]
    priors = oracle.make_priors([dict(kind=p["kind"], p0=p["p0"], p1=p["p1"], lo=p["lo"], hi=p["hi"]) for p in MODEL_PRIORS])
    keys = ("kind", "i0", "i1", "flags", "value")
    esrc = oracle.make_sources([dict(zip(keys, s)) for s in MODEL_ESRC])
    nsrc = oracle.make_sources([dict(zip(keys, s)) for s in MODEL_NSRC])
    return obs, planets, priors, esrc, nsrc


def oracle_logpost(oracle, om):
    """logpost(θ_t) -> (ℓπ, ∇ℓπ) of the restatement, from the oracle's callback"""
    obs, planets, priors, esrc, nsrc = om
    return lambda th: oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, th, grad=True, n_threads=0)


def rejection_batch(oracle, om, seed, first, n=POST_N):
    """octofit_rejection over prior draws first … first + n − 1 of `seed`, restated: θ_t of the accepted draws, in draw order."""
    obs, planets, priors, esrc, nsrc = om
    idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    _, tt = ref.prior_sample(MODEL_PRIORS, seed, idx)
    lp, _ = oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, tt, grad=False, n_threads=0)
    lpt, _ = ref.logprior_t(MODEL_PRIORS, tt)
    with np.errstate(all="ignore"):
        ll = lp - lpt
        ll = np.where(np.isfinite(ll), ll, -np.inf)
        acc = (ll != -np.inf) & (ref.rejection_uniforms(seed, idx) < np.exp(ll - ll.max()))
    return tt[:, acc]


def posterior_inv_mass(batch):
    """The diagonal inverse mass of the β = 1 condition: the per-coordinate variance of batch B in θ_t, rounded to two digits so that the
    CPU and the GPU test use the same numbers whatever the last bits of their batches are."""
    return np.array([float(f"{v:.2g}") for v in batch.var(axis=1)])


def check_posterior_stationary(batch_a, batch_b, step_fn, label):
    """Batch A pushed through POST_STEPS steps stays within the two-sample bar of batch B on every coordinate; mean acceptance >= 0.5."""
    n_a, n_b = batch_a.shape[1], batch_b.shape[1]
    print(f"{label}: batches of {n_a} and {n_b} accepted draws of {POST_N}")
    assert n_a >= POST_LEAST and n_b >= POST_LEAST
    bar = 1.95 * math.sqrt((n_a + n_b) / (n_a * n_b))
    before = max(ks_two_sample(batch_a[d], batch_b[d]) for d in range(batch_a.shape[0]))
    tt, accs = batch_a.copy(), []
    for step in range(POST_STEPS):
        tt, acc = step_fn(tt, step)
        accs.append(float(np.mean(acc)))
    moved = float(np.mean(np.any(tt != batch_a, axis=0)))
    stats = [ks_two_sample(tt[d], batch_b[d]) for d in range(tt.shape[0])]
    print(f"{label}: two-sample D before {before:.3e}, after {POST_STEPS} steps max {max(stats):.3e} (bar {bar:.3e}); acceptance {np.mean(accs):.3f}; moved {moved:.3f}")
    assert max(stats) < bar, stats
    assert np.mean(accs) >= 0.5, accs
    assert moved >= 0.9


@pytest.mark.parametrize("seed", POST_SEEDS)
def test_posterior_is_stationary(oracle, seed):
    om = oracle_model(oracle)
    a, b = (rejection_batch(oracle, om, seed, first) for first in POST_FIRST)
    im = posterior_inv_mass(b)
    logpost = oracle_logpost(oracle, om)

    def step_fn(tt, step):
        r = ref.hmc_step(MODEL_PRIORS, tt, None, POST_EPS, POST_LEAPFROG, im, seed, step, logpost=logpost)
        return r["theta_t"], r["accepted"]

    check_posterior_stationary(a, b, step_fn, f"seed {seed} (CPU)")


# ---------------------------------------------------------------------------------------------------- one step: the condition on its seed
STEP_W, STEP_LD, STEP_SEED, STEP_STEP = 192, 197, 41, 5      # three waves, a partial block, a padded leading dimension
STEP_BETAS = (0.0, 0.01, 0.3, 1.0)


def step_inputs(W=STEP_W):
    """(β, ε, inv_mass) of the one-step comparison of tests/test_hmc.py: β cycles through STEP_BETAS, ε differs from chain to chain."""
    beta = np.array([STEP_BETAS[w % 4] for w in range(W)])
    eps = 0.04 + 0.05 * (np.arange(W) % 5)
    im = np.array([2e-3, 4e-6, 4e2, 5.0, 3.0, 3.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 4.0])      # about the posterior's variances in θ_t
    return beta, eps, im


def test_one_step_flags_are_decided_for_the_seed(oracle):
    """The GPU test compares acceptance flags wherever |dH − log u| > 1e-6 and may leave out at most 1 % of the chains: that holds for its
    seed, from the reference alone (at the restated prior draws; the device's differ in the last bits)."""
    beta, eps, im = step_inputs()
    _, start = ref.prior_sample(MODEL_PRIORS, STEP_SEED, np.arange(STEP_W, dtype=np.uint64))
    logpost = oracle_logpost(oracle, oracle_model(oracle))
    for n_leapfrog in (1, 3):
        r = ref.hmc_step(MODEL_PRIORS, start, beta, eps, n_leapfrog, im, STEP_SEED, STEP_STEP, logpost=logpost)
        close = np.abs(r["dH"] - r["log_u"]) <= 1e-6
        print(f"L {n_leapfrog}: acceptance {r['accepted'].mean():.3f}, {close.sum()} of {STEP_W} chains within 1e-6 of the decision, max |E| {np.max(np.abs(r['E0'])):.3e}")
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
