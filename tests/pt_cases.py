"""
The inputs and bars of the parallel-tempering statistics' suites (tests/test_pt_reference.py on the CPU, tests/test_pt.py on the GPU): the
synthetic scans the two device calls are compared on, the exact tempered Gaussian the restatement is held to by meaning, the independent log
evidence of the suites' test model, and the measured scatter the bars come from. A plain module, not a conftest and not a test module.
"""
import functools
import math

import numpy as np

import pt_reference as pt

# ---------------------------------------------------------------------------------------------------- 1. the two calls on synthetic ℓ
# (T, Cn): a lone chain, a partial wave, a wave edge, a partial block, several blocks, the top of T
SHAPES = [(2, 1), (3, 63), (8, 64), (5, 65), (8, 257), (64, 1000)]
N_CALLS = 4             # three accumulating calls, the schedule with reset, one more call
MARGIN_BAR = 1e-6       # every target g_k of a schedule case stays this far, relative to Λ, from every node Λ_t


def ladder(T, Cn):
    """linspace(1, 0, T)² with two equal neighbours from T = 3 on: the two coldest slots (both the prior: db = 0 next to dead prior draws) where
    Cn is odd, two slots in the middle where it is even. T = 2 has no room for a pair of equal neighbours and a ladder to re-place."""
    beta = np.linspace(1.0, 0.0, T) ** 2
    if T >= 3:
        j = T - 2 if Cn % 2 else T // 2 - 1
        beta[j] = beta[j + 1]
    return beta


@functools.lru_cache(maxsize=None)
def scans(T, Cn, swapped=False):
    """N_CALLS scans (ℓ [T][Cn], slot2rep [Cn][T] int32) of one shape: random per-chain permutations, ℓ of magnitude 300, −Inf at the cold
    slot of a quarter of the chains, and beside clean chains one NaN and one +Inf (with fewer than three chains: scan 1 holds the NaN, scan 2
    the +Inf, at slot 0). swapped: the NaN and the +Inf trade places — both are excluded from everything, so nothing may change."""
    rng = np.random.default_rng(1000 * T + Cn)
    nan, inf = (np.inf, np.nan) if swapped else (np.nan, np.inf)
    out = []
    for k in range(N_CALLS):
        s2r = np.stack([rng.permutation(T) for _ in range(Cn)]).astype(np.int32)
        ll = -300.0 + 30.0 * rng.standard_normal((T, Cn))
        dead = np.nonzero(rng.random(Cn) < 0.25)[0]
        ll[s2r[dead, T - 1], dead] = -np.inf
        if Cn >= 3:
            a, b = rng.choice(Cn, 2, replace=False)
            ll[rng.integers(T), a] = nan
            ll[rng.integers(T), b] = inf
        elif k in (1, 2):
            ll[s2r[0, 0], 0] = nan if k == 1 else inf
        out.append((ll, s2r))
    return out


@functools.lru_cache(maxsize=None)
def reference(T, Cn):
    """The restatement on scans(T, Cn), computed once: acc after each of the first three calls, the schedule (with reset) after them, acc
    after the fourth call (made on the re-placed ladder), a second schedule without adaptation, and leg and restarts after each call."""
    beta = ladder(T, Cn)
    acc = pt.new_acc(T)
    leg, count = np.zeros((Cn, T), dtype=np.int32), np.zeros(Cn, dtype=np.int32)
    accs, legs, counts = [], [], []
    sched = None
    for k, (ll, s2r) in enumerate(scans(T, Cn)):
        if k == N_CALLS - 1:
            sched = pt.schedule(acc, beta, adapt=True, reset=True)
            acc, beta = sched["acc"], sched["beta"]             # the fourth call runs on the re-placed ladder
        acc = pt.stats(ll, s2r, beta, acc)
        pt.restarts(s2r, leg, count)
        accs.append(acc)
        legs.append(leg.copy())
        counts.append(count.copy())
    return dict(beta=ladder(T, Cn), accs=accs, legs=legs, counts=counts, schedule=sched, margin=pt.margins(accs[N_CALLS - 2]),
                last=pt.schedule(accs[-1], sched["beta"], adapt=False, reset=False))


# ---------------------------------------------------------------------------------------------------- 2. α against the swap kernel
SWAP_T, SWAP_CN, SWAP_STEPS, SWAP_SEED = 6, 512, 200, 77


def swap_inputs():
    """fixed ℓ [T][Cn] and a ladder on which the pairs' acceptance probabilities spread over (0, 1)"""
    rng = np.random.default_rng(606)
    return -100.0 + 3.0 * rng.standard_normal((SWAP_T, SWAP_CN)), pt.cubic_ladder(SWAP_T)


# ---------------------------------------------------------------------------------------------------- 3. exact tempered Gaussian draws
# Prior N(0, 1)^D, ℓ(x) = −‖x − μ‖²/(2σ²): the replica at β is N(βμ/(σ² + β), σ²/(σ² + β)) in every coordinate, drawn exactly, so the round
# loop is tested with a perfect explorer. log Z = D·(½ log(σ²/(1 + σ²)) − μ²/(2(1 + σ²))).
GAUSS_D, GAUSS_MU, GAUSS_SIGMA, GAUSS_T, GAUSS_CN, GAUSS_ROUNDS = 4, 3.0, 0.3, 8, 64, 8
GAUSS_LOGZ = GAUSS_D * (0.5 * math.log(GAUSS_SIGMA ** 2 / (1.0 + GAUSS_SIGMA ** 2)) - GAUSS_MU ** 2 / (2.0 * (1.0 + GAUSS_SIGMA ** 2)))      # −21.502
GAUSS_SEEDS = range(30)


def gauss_explorer(rng):
    """explore(β [T][Cn], scan) -> ℓ [T][Cn]: an exact draw of every replica at its β"""
    s2 = GAUSS_SIGMA ** 2

    def explore(beta, scan):
        x = beta[..., None] * GAUSS_MU / (s2 + beta[..., None]) + np.sqrt(s2 / (s2 + beta[..., None])) * rng.standard_normal(beta.shape + (GAUSS_D,))
        return -np.sum((x - GAUSS_MU) ** 2, axis=-1) / (2.0 * s2)
    return explore


def gauss_run(seed, adapt=True, stats_fn=pt.stats):
    rng = np.random.default_rng(seed)
    return pt.pigeons(gauss_explorer(rng), GAUSS_T, GAUSS_CN, GAUSS_ROUNDS, rng, adapt=adapt, stats_fn=stats_fn)


def spread(rej):
    return float(np.max(rej) - np.min(rej))


# Measured with the committed restatement over GAUSS_SEEDS (tests/test_pt_reference.py measures and prints them again):
#   Λ of the last round                       4.502 (4.494 … 4.512)
#   max_t r_t − min_t r_t, round 1            0.747 (0.694 … 0.796)
#   the same spread, round 8                  mean 0.0121, worst 0.0200
#   last-round forward error                  mean +0.004, sd 0.0313, worst |·| 0.097
#   last-round reverse error                  mean +0.008, sd 0.1006, worst |·| 0.250
#   last-round mean error                     mean +0.006, sd 0.0518, worst |·| 0.130
# The bars: 4 × the measured deviation for log Z, 1.5 × the measured worst spread.
GAUSS_FWD_SD, GAUSS_REV_SD, GAUSS_MEAN_SD, GAUSS_WORST_SPREAD = 0.0313, 0.1006, 0.0518, 0.0200
GAUSS_FWD_BAR, GAUSS_REV_BAR, GAUSS_MEAN_BAR = 4 * GAUSS_FWD_SD, 4 * GAUSS_REV_SD, 4 * GAUSS_MEAN_SD
GAUSS_SPREAD_BAR = 1.5 * GAUSS_WORST_SPREAD
GAUSS_BARRIER = (4.3, 4.7)      # Λ of the last round, every seed


# ---------------------------------------------------------------------------------------------------- 4. the driver on the suites' test model
# log Z of draws_device.hmc_model by prior importance sampling, log mean exp ℓ over 2^20 prior draws through the CPU oracle: seeds 31 (both
# windows of draws_cases.POST_FIRST), 32 and 7 gave −274.493, −274.514, −274.508, −274.509; ESS about 9 500 of 2^20, so se ≈ 0.010 each and
# ≈ 0.005 combined.
MODEL_LOGZ, MODEL_LOGZ_SE, MODEL_LOGZ_SE_ONE = -274.506, 0.005, 0.010
DRIVER_T, DRIVER_CN, DRIVER_ROUNDS, DRIVER_SEEDS = 8, 128, 8, (3, 4)
SLICE_ROUNDS = 4


def importance_logz(oracle, seed, first, n):
    """log mean exp ℓ over prior draws first … first + n − 1 of `seed`, and the effective sample size of the weights"""
    import draws_cases as cases
    import hmc_reference as ref
    obs, planets, priors, esrc, nsrc = cases.oracle_model(oracle)
    idx = np.uint64(first) + np.arange(n, dtype=np.uint64)
    _, tt = ref.prior_sample(cases.MODEL_PRIORS, seed, idx)
    lp, _ = oracle.oracle_model_logpost(obs, planets, priors, esrc, nsrc, tt, grad=False, n_threads=0)
    lpt, _ = ref.logprior_t(cases.MODEL_PRIORS, tt)
    with np.errstate(all="ignore"):
        ll = lp - lpt
        ll = np.where(np.isfinite(ll), ll, -np.inf)
        w = np.exp(ll - ll.max())
    return float(ll.max() + np.log(w.sum() / n)), float(w.sum() ** 2 / (w ** 2).sum())


# The sampler's own scatter of octofit_pigeons_device(explorer="hmc") at (DRIVER_T, DRIVER_CN, DRIVER_ROUNDS) = 510 scans, measured on the MI355X at
# seeds 1 … 8 (tools/pt_adapt_bench.py --scatter; profiles/pt_adapt_throughput.txt quotes the run), against MODEL_LOGZ:
#   fwd   mean −274.5035 (error +0.0025), sd 0.0129
#   rev   mean −274.4868 (error +0.0192), sd 0.0373
#   mean  mean −274.4952 (error +0.0108), sd 0.0226
# The bar is 4·√(se² + s²) on the statistic with the smallest s, the forward estimate: 4·√(0.005² + 0.0129²) = 0.0553. s is far below the 0.25
# at which the run would have to be lengthened.
DRIVER_STATISTIC, DRIVER_S = "fwd", 0.0129
DRIVER_BAR = 4.0 * math.hypot(MODEL_LOGZ_SE, DRIVER_S)
