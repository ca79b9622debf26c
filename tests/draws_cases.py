"""
The inputs, seeds, bars and statistical helpers the suites of liboctofitter_hip_draws.so share, none of which needs a device: each
tests/test_*_reference.py establishes a condition on the CPU with them, and the GPU suite of the same feature (tests/test_hmc.py,
test_lbfgs.py, test_pathfinder.py, test_adapt.py, test_nuts.py, test_prior_draws.py) then holds the device to it with the same numbers.
A plain module, not a conftest and not a test module: a value used by more than one file is stated here, once. Helpers that assert carry
their own messages (pytest does not rewrite the assertions of a plain module). The device-side helpers are in tests/draws_device.py.

The Kolmogorov-Smirnov bars: 1.95/√n is the 0.1 % critical value of the one-sample statistic, 1.95·√((n_A + n_B)/(n_A·n_B)) its two-sample
form.
"""
import functools
import math

import numpy as np

import adapt_reference as aref
import hmc_reference as ref
import lbfgs_reference as lref
import nuts_reference as nuts


# ---------------------------------------------------------------------------------------------------- Kolmogorov-Smirnov
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


# ---------------------------------------------------------------------------------------------------- β = 0: the prior is stationary
STAT_PRIORS = [ref.prior(ref.UNIFORM, -3, 7), ref.prior(ref.LOGUNIFORM, 0.1, 1000), ref.prior(ref.NORMAL, 1.2, 0.05), ref.prior(ref.SINE),
               ref.prior(ref.TRUNCNORMAL, 0, 1, lo=3)]
STAT_W = 65536
STAT_INV_MASS = (3.3, 3.3, 0.0025, 3.3, 1.0)
STAT_STEPS = 6
STAT_SEEDS = (21, 22)
STAT_SETTINGS = ((0.5, 4), (0.8, 3))      # (ε, n_leapfrog)
STAT_BAR = 1.95 / math.sqrt(STAT_W)


def stationarity_statistics(theta_t):
    """max over the coordinates of D_n of invlink(θ_t) against the prior's CDF"""
    return max(ks_statistic(ref.invlink(pr, theta_t[d])[0], ref.scipy_dist(pr)[0]) for d, pr in enumerate(STAT_PRIORS))


# ---------------------------------------------------------------------------------------------------- β = 1: the posterior is stationary
# The test model: one planet on the parameterisation of tests/test_model.py (Visual{KepOrbit}, UniformCircular angles, tp from θ) with 12
# RA/Dec epochs and 8 absolute-RV rows. MODEL_NAMES is the order the mirror declares the parameters in; draws_device.hmc_model asserts that
# the mirror's priors and sources are these.
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


def oracle_tables(astrom, rv):
    """the two tables as the oracle's callback takes them"""
    return [dict(kind=0, planet=0, epoch=astrom["epoch"], y1=astrom["ra"], y2=astrom["dec"], s1=astrom["σ_ra"], s2=astrom["σ_dec"], cor=None, extra=None),
            dict(kind=2, planet=-1, epoch=rv["epoch"], y1=rv["rv"], y2=None, s1=rv["σ_rv"], s2=None, cor=None, extra=None)]


def oracle_model(oracle):
    """What oracle_model_logpost takes for the test model, built without a device."""
    obs = oracle_tables(*model_tables())
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
    assert n_a >= POST_LEAST and n_b >= POST_LEAST, (n_a, n_b, POST_LEAST)
    bar = 1.95 * math.sqrt((n_a + n_b) / (n_a * n_b))
    before = max(ks_two_sample(batch_a[d], batch_b[d]) for d in range(batch_a.shape[0]))
    tt, accs = batch_a.copy(), []
    for step in range(POST_STEPS):
        tt, acc = step_fn(tt, step)
        accs.append(float(np.mean(acc)))
    moved = float(np.mean(np.any(tt != batch_a, axis=0)))
    stats = [ks_two_sample(tt[d], batch_b[d]) for d in range(tt.shape[0])]
    print(f"{label}: two-sample D before {before:.3e}, after {POST_STEPS} steps max {max(stats):.3e} (bar {bar:.3e}); acceptance {np.mean(accs):.3f}; moved {moved:.3f}")
    assert max(stats) < bar, (stats, bar)
    assert np.mean(accs) >= 0.5, accs
    assert moved >= 0.9, moved


# ---------------------------------------------------------------------------------------------------- one HMC step: the condition on its seed
STEP_W, STEP_LD, STEP_SEED, STEP_STEP = 192, 197, 41, 5      # three waves, a partial block, a padded leading dimension
STEP_BETAS = (0.0, 0.01, 0.3, 1.0)


def step_inputs(W=STEP_W):
    """(β, ε, inv_mass) of the one-step comparison of tests/test_hmc.py: β cycles through STEP_BETAS, ε differs from chain to chain."""
    beta = np.array([STEP_BETAS[w % 4] for w in range(W)])
    eps = 0.04 + 0.05 * (np.arange(W) % 5)
    im = np.array([2e-3, 4e-6, 4e2, 5.0, 3.0, 3.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 4.0])      # about the posterior's variances in θ_t
    return beta, eps, im


# ---------------------------------------------------------------------------------------------------- L-BFGS: the tight model and its reference case
# The test model with the noise its tables were actually drawn with as their σ (60 mas, 30 m/s): a posterior with one dominant optimum that
# the scaled L-BFGS reaches from the best prior draws. The scaling v is the variance of prior draws 0 … 4095 in θ_t, the default of the
# device drivers.
LBFGS_SEED, LBFGS_N_DRAWS, LBFGS_N_STARTS = 77, 65536, 64
LBFGS_M, LBFGS_GRAD_TOL, LBFGS_ROUNDS = 6, 1e-6, 800
LBFGS_SHORT_W, LBFGS_SHORT_LD, LBFGS_SHORT_ROUNDS = 67, 71, 4      # one full wave plus three lanes, a padded leading dimension
LBFGS_DECIDED_ROUNDS = 40                                          # how far into the full run the decisions of the decided chains are compared
LBFGS_MID_ROUNDS = 10                                              # where its Pathfinder diagonal is compared
LBFGS_MARGIN = 1e-6
LBFGS_SHORT_FTOLS = (0.0, 0.05)                                    # without the ftol test, and with one that stops about half of the chains in the short run
TIGHT_SIGMA_ASTROM, TIGHT_SIGMA_RV = 60.0, 30.0


def tight_tables():
    """model_tables() with σ the noise that was drawn"""
    astrom, rv = model_tables()
    astrom = dict(astrom, σ_ra=np.full(12, TIGHT_SIGMA_ASTROM), σ_dec=np.full(12, TIGHT_SIGMA_ASTROM))
    return astrom, dict(rv, σ_rv=np.full(8, TIGHT_SIGMA_RV))


def tight_logpost(oracle, n_threads=0):
    """logpost(θ_t) -> (ℓπ, ∇ℓπ) of the tight model from the oracle's callback (n_threads = 1 for one θ_t at a time: no thread start a call)"""
    obs = oracle_tables(*tight_tables())
    _, planets, priors, esrc, nsrc = oracle_model(oracle)
    return lambda th: oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, np.ascontiguousarray(th), grad=True, n_threads=n_threads)


def prior_theta_t(first, n):
    return ref.prior_sample(MODEL_PRIORS, LBFGS_SEED, np.uint64(first) + np.arange(n, dtype=np.uint64))[1]


def default_inv_mass(theta_t_4096):
    """the unbiased per-coordinate variance, as torch.var gives the device drivers"""
    return np.var(theta_t_4096, axis=1, ddof=1)


@functools.lru_cache(maxsize=None)
def reference_case(oracle):
    """(starts [D, 64] best first, their ℓπ, v, the restatement's result from them) — computed once, shared, never modified"""
    logpost = tight_logpost(oracle)
    tt = prior_theta_t(0, LBFGS_N_DRAWS)
    lp = np.concatenate([logpost(tt[:, k:k + 8192])[0] for k in range(0, LBFGS_N_DRAWS, 8192)])
    order = np.argsort(-np.where(np.isfinite(lp), lp, -np.inf), kind="stable")[:LBFGS_N_STARTS]
    starts, v = np.ascontiguousarray(tt[:, order]), default_inv_mass(tt[:, :4096])
    res = lref.lbfgs(logpost, starts, v, m=LBFGS_M, n_rounds=LBFGS_ROUNDS, gtol=LBFGS_GRAD_TOL)
    for a in (starts, v, *[x for x in res.values() if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return starts, lp[order], v, res


def random_history(rng, m, D, W, dtype=np.float64):
    """s random, y = A·s with A SPD of condition <= 1e3 (one A per chain); cnt cycles through 0 … m, head through 0 … m − 1"""
    S, Y = np.zeros((m, D, W), dtype=dtype), np.zeros((m, D, W), dtype=dtype)
    for w in range(W):
        Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
        A = (Q * np.logspace(0, 3 * rng.uniform(), D)) @ Q.T
        s = rng.normal(size=(m, D))
        S[:, :, w], Y[:, :, w] = s, s @ A.T
    cnt, head = np.arange(W) % (m + 1), (np.arange(W) * 3 + 1) % m
    return cnt, head, S, Y, rng.normal(size=(D, W)).astype(dtype), np.exp(rng.uniform(-3, 3, D)).astype(dtype)


# ---------------------------------------------------------------------------------------------------- Pathfinder
PF_SEED, PF_CHAIN0, PF_N_ELBO = LBFGS_SEED, 1000, 5
PF_ROUNDS = 10                    # the rounds of the GPU comparison on the tight model
PF_MARGIN = 1e-6                  # a chain is decided if its two best ELBOs differ by more than PF_MARGIN·max(1, |ELBO|)
PF_FIT_SHAPES = [(1, 1), (5, 3), (14, 6), (64, 8)]      # (D, m): the smallest, 2·cnt > D, the test model's, the top of D
PF_FIT_W, PF_FIT_LD = 23, 32


def fit_inputs(D, m, W=PF_FIT_W):
    """random_history (cnt over 0 … m, wrapped heads) with an α per chain and a point x"""
    rng = np.random.default_rng(7000 * D + m)
    cnt, head, S, Y, g, _ = random_history(rng, m, D, W)
    alpha = np.exp(rng.uniform(-3, 3, (D, W)))
    return cnt, head, S, Y, rng.normal(size=(D, W)), g, alpha


def decided_chains(r):
    return (r["elbo_iter"] >= 0) & (r["margin_elbo"] > PF_MARGIN)


# ---------------------------------------------------------------------------------------------------- warm-up: the grouped moments
# The bars on the moments: counts exact; |mean − exact| <= n·2⁻⁵³·max|x| of the group's row — (Σx)/n in any summation order errs by at most
# (n − 1)·2⁻⁵³·max|x| in the sum and 2⁻⁵³·|mean| in the quotient —; |M2 − exact| <= 1e-10·exact: the two-pass and Chan forms err by
# O(n·2⁻⁵³) relative, Σx² − n·mean² by about 1e-6 on the row with mean 5e4 and deviation 0.5.
U = 2.0 ** -53
M2_BAR = 1e-10
MOMENT_W = (1, 63, 64, 65, 255, 256, 257, 1000)      # a partial wave, a wave edge, a partial block, several blocks
MOMENT_K = (1, 11, 64)
MOMENT_G = (1, 3, 64)                                # 1: a NULL group array


def moments_case(W, K, G):
    """(x [K][W], group [W] or None). Row 0 is a `tp` in MJD: mean 5e4, deviation 0.5; the other rows have scales from 1e-2 to 1e2 and means
    of either sign. With a group array: ids −1 and G (excluded), group G − 1 empty, group 1 with a single member. One chain has a NaN and one
    an Inf coordinate (in the last row: the exclusion has to look at every row). Chains too few for a role do without it."""
    rng = np.random.default_rng(1000 * W + 10 * K + G)
    scale = 10.0 ** ((np.arange(K) % 5) - 2)
    x = rng.normal(size=(K, W)) * scale[:, None] + (np.arange(K) % 3 - 1)[:, None] * 3.0 * scale[:, None]
    x[0] = 5e4 + 0.5 * rng.normal(size=W)
    group = None
    if G > 1:
        group = rng.integers(0, G - 1, size=W).astype(np.int32)      # group G − 1 stays empty
        if W >= 63:
            group[group == 1] = 0
            group[11] = 1
            group[2], group[3] = -1, G
    if W >= 63:
        x[K - 1, 5] = np.nan
        x[K - 1, 7] = np.inf
    return x, group


def check_moments(got, exact, what):
    """the three bars on the moments"""
    cnt, mean, m2 = (np.asarray(t, dtype=np.float64) for t in got)
    ecnt, emean, em2, amax = exact
    assert np.array_equal(cnt, ecnt), (what, cnt, ecnt)
    err_mean = np.abs(mean - emean)
    assert np.all(err_mean <= ecnt[:, None] * U * amax), (what, "mean", float(np.max(err_mean - ecnt[:, None] * U * amax)))
    err_m2 = np.abs(m2 - em2)
    assert np.all(err_m2 <= M2_BAR * em2), (what, "M2", float(np.max(err_m2 / np.where(em2 > 0, em2, 1.0))))
    rel = np.max(err_m2 / np.where(em2 > 0, em2, 1.0)) if em2.size else 0.0
    return float(np.max(err_mean / np.where(amax > 0, ecnt[:, None] * U * amax, 1.0))), float(rel)


def thirds(W):
    return [(0, W // 3), (W // 3, 2 * W // 3), (2 * W // 3, W)]


# ---------------------------------------------------------------------------------------------------- warm-up: dual averaging, R̂
DA_W = 300


def dual_averaging_case(G):
    """(dH [W], accepted [W], group [W] or None): finite values of both signs, ±Inf, NaN with accepted 0 and 1, values above 700; with groups:
    ids −1 and G, and group G − 2 empty."""
    rng = np.random.default_rng(77 + G)
    dH = rng.normal(-0.3, 1.0, DA_W)
    acc = (rng.uniform(size=DA_W) < np.minimum(1.0, np.exp(dH))).astype(np.int32)
    dH[[3, 70, 140]] = np.inf
    dH[[4, 71, 141]] = -np.inf
    dH[[5, 72, 142, 143]] = np.nan
    acc[[5, 142]] = 1
    acc[[72, 143]] = 0
    dH[[6, 73, 144]] = (710.0, 1e6, 700.5)
    group = None
    if G > 1:
        group = (np.arange(DA_W) % G).astype(np.int32)
        group[group == G - 2] = 0
        group[[9, 200]] = (-1, G)
    return dH, acc, group


RHAT_W, RHAT_K, RHAT_N = 257, 11, 12


def rhat_case():
    """samples [n][K][W], row k around 5·(k + 1) so that a relative bar on the running means is meaningful; chain 100 has one NaN (sample 4, row 3)"""
    rng = np.random.default_rng(12)
    s = rng.normal(size=(RHAT_N, RHAT_K, RHAT_W)) + 0.3 * rng.normal(size=(1, RHAT_K, RHAT_W)) + 5.0 * (1 + np.arange(RHAT_K))[None, :, None]
    s[4, 3, 100] = np.nan
    return s


# ---------------------------------------------------------------------------------------------------- warm-up: the loop on the prior
LOOP_W, LOOP_WARMUP, LOOP_LEAPFROG, LOOP_SEED, LOOP_EPS = 192, 30, 3, 51, 0.1
# The largest deviation, relative to max(1, |value|), of ε, inv_mass and the final θ_t between two runs of the restatement whose starts differ
# by one ulp in every coordinate, measured by tests/test_adapt_reference.py::test_warmup_loop_sensitivity_to_one_ulp: 3.105e-8
# (thirty rounds of three leapfrog steps amplify an ulp that far on the chain that moves most). The free-running comparison of
# tests/test_adapt.py is held to max(1e-8, 100·s).
LOOP_S = 3.11e-8
LOOP_BAR = max(1e-8, 100 * LOOP_S)


def loop_deviation(a, b):
    return max(float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])) / np.maximum(1.0, np.abs(np.asarray(b[k]))))) for k in ("eps", "inv_mass", "theta_t"))


# The kernel a warm-up freezes leaves the prior invariant: (ε, inv_mass) from a warm-up on chains 0 … 4095, then a fresh batch of exact prior
# draws (draws and chains 4096 … 4096 + 65535) through six steps, one-sample KS per coordinate under STAT_BAR. FROZEN_SEEDS are the first two
# of 21, 22, 23, … for which the restatement stays under the bar (tests/test_adapt_reference.py::test_frozen_kernel_is_stationary);
# tests/test_adapt.py uses the same ones on the device.
FROZEN_WARM_W, FROZEN_W, FROZEN_STEPS = 4096, STAT_W, STAT_STEPS
FROZEN_SEEDS = (21, 22)


def frozen_run(seed, eps, inv_mass):
    """(max D_n over the coordinates, mean acceptance flag) of the fresh batch after six steps at step numbers LOOP_WARMUP …"""
    tt = ref.prior_sample(STAT_PRIORS, seed, FROZEN_WARM_W + np.arange(FROZEN_W, dtype=np.uint64))[1]
    acc = []
    for j in range(FROZEN_STEPS):
        r = ref.hmc_step(STAT_PRIORS, tt, None, eps, LOOP_LEAPFROG, inv_mass, seed, LOOP_WARMUP + j, chain0=FROZEN_WARM_W)
        tt = r["theta_t"]
        acc.append(np.mean(r["accepted"]))
    return stationarity_statistics(tt), float(np.mean(acc))


def frozen_reference(seed):
    start = ref.prior_sample(STAT_PRIORS, seed, np.arange(FROZEN_WARM_W, dtype=np.uint64))[1]
    wu = aref.hmc_warmup(STAT_PRIORS, start, LOOP_WARMUP, LOOP_LEAPFROG, LOOP_EPS, np.ones(5), seed)
    return wu, frozen_run(seed, wu["eps"], wu["inv_mass"])


# ---------------------------------------------------------------------------------------------------- NUTS
# A chain is DECIDED if the smallest margin of any decision it made exceeds nuts_reference.MARGIN = 1e-6: two computations that differ in
# the last bits then make the same decisions, and tests compare decisions on decided chains only.
NUTS_STAT_EPS = (0.5, 0.8)
NUTS_STAT_DEPTH = 5
ONE_W, ONE_LD, ONE_SEED, ONE_STEP, ONE_DEPTH = 65, 72, 41, 5, 4      # a partial second wave, a padded leading dimension
ONE_BETAS = (0.0, 0.3, 1.0)
ONE_UNDECIDED = 0.05


def one_inputs(W=ONE_W):
    """(β, ε, inv_mass) of the one-transition comparison of tests/test_nuts.py: β cycles through ONE_BETAS, ε (on the scale of step_inputs)
    differs from chain to chain."""
    beta = np.array([ONE_BETAS[w % 3] for w in range(W)])
    _, eps, im = step_inputs(W)
    return beta, eps, im


def one_transition(oracle, start):
    beta, eps, im = one_inputs(start.shape[1])
    return nuts.nuts_transition(MODEL_PRIORS, start, beta, eps, im, ONE_DEPTH, ONE_SEED, ONE_STEP, logpost=oracle_logpost(oracle, oracle_model(oracle)))


def check_one_transition_is_decided(r):
    undecided = r["margin"] <= nuts.MARGIN
    print(f"one transition: {undecided.sum()} of {undecided.size} chains undecided; stop reasons {np.bincount(r['stop'], minlength=6)[1:]}; "
          f"mean leaves {r['n_leapfrog'].mean():.2f}; moved {r['accepted'].mean():.3f}")
    assert undecided.mean() <= ONE_UNDECIDED, "condition on the seed (the reference alone)"
    assert np.all(np.isfinite(r["theta_t"])) and r["accepted"].mean() > 0.5 and len(set(r["depth"])) >= 2, \
        (bool(np.all(np.isfinite(r["theta_t"]))), r["accepted"].mean(), sorted(set(r["depth"])))


# Deep trees. The checkpoint slot of leaf n of a subtree is popc(n >> 1): a tree of depth <= 5 (n <= 15) uses the slots 0 … 3 only, the slots
# 4 … 8 need subtrees of 32 … 512 leaves. Two cases reach max_depth = 10, each with ε differing from chain to chain so that every depth below
# occurs as well.
DEEP_DEPTH = 10
# Priors only, against nuts_brute_force (tests/test_nuts_reference.py): ε spread geometrically over 0.004 … 0.3, one value per chain. The
# seed is the first of 1, 2, 3, … with a decided chain at every depth from 3 to 10 and one stopped by each of the depth limit, a turn of a
# subtree and a turn of the tree (few trees of these priors reach the limit without turning).
BRUTE_DEEP_W, BRUTE_DEEP_SEED, BRUTE_DEEP_EPS = 24, 8, (0.004, 0.3)


def brute_deep_inputs():
    """(starts, ε [W]) of the deep brute-force setting"""
    _, tt = ref.prior_sample(STAT_PRIORS, BRUTE_DEEP_SEED, np.arange(BRUTE_DEEP_W, dtype=np.uint64))
    return tt, np.geomspace(*BRUTE_DEEP_EPS, BRUTE_DEEP_W)


# The test model: the one-transition comparison with ε scaled per chain by DEEP_SCALES[w % 4] and max_depth = 10, everything else unchanged.
# The order of the four scales is a condition on the seed: in the order (1, 1/4, 1/16, 1/64) no chain of ONE_SEED stops at depth 3.
DEEP_SCALES = (1 / 16, 1 / 64, 1.0, 1 / 4)
DEEP_FULL = 5                       # at least that many chains build all 1023 leaves


def deep_inputs(W=ONE_W):
    """one_inputs() with ε multiplied per chain by DEEP_SCALES[w % 4]"""
    beta, eps, im = one_inputs(W)
    return beta, eps * np.array([DEEP_SCALES[w % 4] for w in range(W)]), im


def deep_transition(oracle, start):
    beta, eps, im = deep_inputs(start.shape[1])
    return nuts.nuts_transition(MODEL_PRIORS, start, beta, eps, im, DEEP_DEPTH, ONE_SEED, ONE_STEP, logpost=oracle_logpost(oracle, oracle_model(oracle)))


def tree_summary(r):
    decided = r["margin"] > nuts.MARGIN
    return (f"{np.sum(~decided)} of {decided.size} chains undecided; decided chains by depth 0 … {np.bincount(r['depth'][decided], minlength=DEEP_DEPTH + 1)}; "
            f"stop reasons {np.bincount(r['stop'], minlength=6)[1:]}; mean leaves {r['n_leapfrog'].mean():.1f}; rounds {r['rounds']}")


def check_deep_transition_is_decided(r):
    """the conditions on the deep case, from the restatement alone"""
    decided = r["margin"] > nuts.MARGIN
    print(f"deep transition: {tree_summary(r)}; moved {r['accepted'].mean():.3f}")
    assert np.mean(~decided) <= ONE_UNDECIDED, "condition on the seed (the reference alone)"
    assert set(range(2, DEEP_DEPTH + 1)) <= set(r["depth"][decided]), sorted(set(r["depth"][decided]))
    assert {nuts.STOP_MAX_DEPTH, nuts.STOP_TURN_SUBTREE, nuts.STOP_TURN_TREE, nuts.STOP_DIVERGED} <= set(r["stop"]), sorted(set(r["stop"]))
    assert np.sum(r["n_leapfrog"] == (1 << DEEP_DEPTH) - 1) >= DEEP_FULL, int(np.sum(r["n_leapfrog"] == (1 << DEEP_DEPTH) - 1))
    assert np.all(np.isfinite(r["theta_t"]))


# The largest deviation of θ_t, ℓπ (relative to max(1, |value|)) and log_accept (absolute) between runs of the restatement whose starts differ by
# one ulp in every coordinate, measured by tests/test_nuts_reference.py::test_deep_transition_sensitivity_to_one_ulp: 5.062e-13.
# The device is held to max(1e-8, 100·s): the factor covers its other summation order and its transcendentals over about 1000 leapfrogs.
DEEP_S = 5.07e-13
DEEP_BAR = max(1e-8, 100 * DEEP_S)


def transition_deviation(a, b):
    """the largest deviation of θ_t, ℓπ (relative to max(1, |value|)) and log_accept (absolute) between two results of the restatement, over
    the chains on which every decision of the two is the same; and how many chains those are"""
    same = np.all([a[k] == b[k] for k in ("depth", "stop", "selected", "n_leapfrog")], axis=0)
    rel = lambda x, y: float(np.max(np.abs(x - y) / np.maximum(1.0, np.abs(y)), initial=0.0))      # noqa: E731
    made = same & (a["n_leapfrog"] > 0)
    with np.errstate(invalid="ignore"):
        la = np.where(a["log_accept"][made] == b["log_accept"][made], 0.0, np.abs(a["log_accept"][made] - b["log_accept"][made]))
    return max(rel(a["theta_t"][:, same], b["theta_t"][:, same]), rel(a["logpost"][same], b["logpost"][same]), float(np.max(la, initial=0.0))), int(same.sum())


# Other dimensions, and inv_mass = None: handles without a model at D = 1 and D = 64, the priors cycling through STAT_PRIORS and the metric
# through STAT_INV_MASS, ε spread geometrically over the chains. Without a metric the 64-dimensional case is stiff (the Normal(1.2, 0.05)
# coordinates diverge from ε ≈ 0.1 on): its chains end at depth 0 or 1 by a divergence or build to the limit.
DIM_DS, DIM_W, DIM_LD, DIM_DEPTH, DIM_SEED, DIM_STEP = (1, 64), 65, 72, 7, 5, 3
DIM_EPS = (0.005, 0.6)
DIM_DEPTHS = 3                      # at least that many distinct depths among the decided chains


def dim_priors(D):
    return [STAT_PRIORS[d % len(STAT_PRIORS)] for d in range(D)]


def dim_inputs(D):
    """(ε [W], inv_mass [D])"""
    return np.geomspace(*DIM_EPS, DIM_W), np.array([STAT_INV_MASS[d % len(STAT_INV_MASS)] for d in range(D)])


# The throughput kernels under NUTS: nine waves and a lane, three blocks of 256 threads with the last partial, a padded leading dimension.
BIG_W, BIG_LD, BIG_DEPTH, BIG_DEAD = 577, 584, 3, 300
