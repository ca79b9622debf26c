"""
The inputs and bars of the variational reference's suites (tests/test_vref_reference.py on the CPU, tests/test_vref.py on the GPU): the tables
and exchanges the device calls are compared on, the exact tempered Gaussian of tests/pt_cases.py with a second, variational leg, and the
measured scatter the bars come from. A plain module, not a conftest and not a test module.
"""
import functools
import math

import numpy as np

import pt_cases as pc
import vref_reference as vr

# ---------------------------------------------------------------------------------------------------- 1. the table
TABLE_D = (1, 11, 64)


def table_inputs(D):
    """(μ [D], σ [D]): magnitudes over ten decades, both signs of μ"""
    rng = np.random.default_rng(500 + D)
    return rng.standard_normal(D) * 10.0 ** rng.integers(-3, 4, D), 10.0 ** rng.uniform(-5.0, 5.0, D)


def moments_inputs(D, n=37.0):
    """(count [1], mean [D], M2 [D]) of one group"""
    rng = np.random.default_rng(600 + D)
    return np.array([n]), rng.standard_normal(D) * 3.0, rng.uniform(0.1, 50.0, D) * n


# ---------------------------------------------------------------------------------------------------- 2. the exchange
# (Cn, T_a, T_b): a lone chain, a partial wave with unequal legs, a full wave, more than one block with the short leg second
EXCHANGE_SHAPES = [(1, 2, 2), (63, 3, 5), (64, 8, 8), (257, 5, 2)]
EXCHANGE_D = 5
EXCHANGE_PAD = 7      # ld = T·Cn + EXCHANGE_PAD, NaN beyond


@functools.lru_cache(maxsize=None)
def exchange_inputs(Cn, T_a, T_b):
    """Two legs of one shape: permuted slot2rep, θ_t [D][ld], ℓπ and ℓ [ld] with NaN beyond T·Cn, and the two reference fits. The target of leg A
    of chain 0 has ℓπ = −Inf; the target of leg B of the last chain has a NaN coordinate (the same chain where Cn = 1)."""
    rng = np.random.default_rng(7000 + 100 * Cn + 10 * T_a + T_b)
    D = EXCHANGE_D
    legs = []
    for T in (T_a, T_b):
        ld = T * Cn + EXCHANGE_PAD
        theta = np.full((D, ld), np.nan)
        theta[:, :T * Cn] = rng.standard_normal((D, T * Cn)) * 2.0
        lp, ll = np.full(ld, np.nan), np.full(ld, np.nan)
        lp[:T * Cn] = -300.0 + 30.0 * rng.standard_normal(T * Cn)
        ll[:T * Cn] = -200.0 + 30.0 * rng.standard_normal(T * Cn)
        s2r = np.stack([rng.permutation(T) for _ in range(Cn)]).astype(np.int32)
        legs.append(dict(T=T, slot2rep=s2r, theta=theta, lp=lp, ll=ll, mean=rng.standard_normal(D), sd=rng.uniform(0.5, 3.0, D)))
    a, b = legs
    a["lp"][a["slot2rep"][0, 0] * Cn + 0] = -np.inf
    b["theta"][2, b["slot2rep"][Cn - 1, 0] * Cn + Cn - 1] = np.nan
    for g in legs:
        g["priors"] = vr.normal_priors(g["mean"], g["sd"])
    return a, b


@functools.lru_cache(maxsize=None)
def exchange_reference(Cn, T_a, T_b):
    """the restatement on exchange_inputs, computed once"""
    a, b = exchange_inputs(Cn, T_a, T_b)
    return vr.exchange(Cn, a, b)


# ---------------------------------------------------------------------------------------------------- 3. the exact tempered Gaussian, two legs
# pt_cases' target (prior N(0, 1)^D, ℓ(x) = −‖x − μ‖²/(2σ²)) with a second leg annealed from q = N(m, s²) per coordinate: the replica at β of
# that leg is q^(1 − β)·π^β, a normal with precision (1 − β)/s² + β(1 + 1/σ²) and mean ((1 − β)m/s² + βμ/σ²)/precision, drawn exactly. The prior
# is the case m = 0, s = 1. Both legs' stepping stones estimate log Z = pt_cases.GAUSS_LOGZ: q is normalised.
GAUSS_TV, GAUSS_ROUNDS, GAUSS_FIRST_TUNING_ROUND = 8, 5, 3      # fits after rounds 2, 3 and 4: 8, 16 and 32 scans of 2·64 target draws


def gauss_explorer(rng):
    """explore(leg, β [T][Cn], scan, reference) -> (x [T][Cn][D], ℓπ [T][Cn]): an exact draw of every replica at its β under its reference"""
    s2, mu = pc.GAUSS_SIGMA ** 2, pc.GAUSS_MU

    def explore(leg, beta, scan, reference):
        m, s = (np.zeros(pc.GAUSS_D), np.ones(pc.GAUSS_D)) if reference is None else reference
        b = beta[..., None]
        prec = (1.0 - b) / s ** 2 + b * (1.0 + 1.0 / s2)
        x = ((1.0 - b) * m / s ** 2 + b * mu / s2) / prec + rng.standard_normal(beta.shape + (pc.GAUSS_D,)) / np.sqrt(prec)
        log_prior = -0.5 * np.sum(x ** 2, axis=-1) - 0.5 * pc.GAUSS_D * math.log(2.0 * math.pi)
        return x, log_prior - np.sum((x - mu) ** 2, axis=-1) / (2.0 * s2)
    return explore


def gauss_run(seed, fit_reference=True):
    rng = np.random.default_rng(seed)
    return vr.two_legs(gauss_explorer(rng), vr.normal_priors(np.zeros(pc.GAUSS_D), np.ones(pc.GAUSS_D)), pc.GAUSS_T, GAUSS_TV, pc.GAUSS_CN, GAUSS_ROUNDS, rng,
                       first_tuning_round=GAUSS_FIRST_TUNING_ROUND, fit_reference=fit_reference)


GAUSS_SEEDS = pc.GAUSS_SEEDS
GAUSS_POWER_SEEDS = range(3)      # the run with the fit skipped: the Λ assertion must fail on each

# Measured with the committed restatement over GAUSS_SEEDS (tests/test_vref_reference.py measures and prints them again), last round (5):
#                                   prior leg                                 variational leg
#   Λ                               4.501 (4.475 … 4.523)                     0.0334 (0.0162 … 0.0493); worst Λ_var/Λ_fixed 0.0110
#   forward error                   mean −0.024, sd 0.0998, worst |·| 0.192   mean +0.0002, sd 0.0006, worst |·| 0.0016
#   reverse error                   mean +0.093, sd 0.2228, worst |·| 0.597   mean +0.0001, sd 0.0006, worst |·| 0.0012
#   mean error                      mean +0.035, sd 0.1389, worst |·| 0.354   mean +0.0002, sd 0.0006, worst |·| 0.0014
# (The prior leg after 5 rounds scatters more than pt_cases' 8 rounds: 0.0313 / 0.1006 / 0.0518 there.) With the fit skipped the second leg
# is a second prior leg: Λ = 4.496, 4.523, 4.492 at seeds 0, 1, 2.
# The bars, as pt_cases sets them: 4 × the measured deviation for log Z, 1.5 × the measured worst Λ of the variational leg.
GAUSS_SD = dict(fixed=(0.0998, 0.2228, 0.1389), variational=(0.0006, 0.0006, 0.0006))      # fwd, rev, mean
GAUSS_BARS = {leg: tuple(4.0 * s for s in sds) for leg, sds in GAUSS_SD.items()}
GAUSS_WORST_BARRIER_VAR = 0.0493
GAUSS_BARRIER_VAR_BAR = 1.5 * GAUSS_WORST_BARRIER_VAR
GAUSS_BARRIER_RATIO = 0.25      # Λ_var < Λ_fixed/4 at every seed; measured: below 0.011


# ---------------------------------------------------------------------------------------------------- 4. the driver on the suites' test model
# octofit_pigeons_device(explorer="hmc", n_temps_variational=DRIVER_T, first_tuning_round=DRIVER_FIRST_TUNING_ROUND) at pt_cases' (DRIVER_T,
# DRIVER_CN, DRIVER_ROUNDS), seeds pt_cases.DRIVER_SEEDS: the reference is fitted after rounds 3 … 7.
DRIVER_FIRST_TUNING_ROUND = 4
# Measured on the MI355X at seeds 1 … 8 (tools/vref_bench.py --scatter; profiles/vref_throughput.txt quotes the run), against pt_cases.MODEL_LOGZ:
#                      prior leg (beside the variational one)            variational leg
#   fwd                mean −274.4975 (error +0.0085), sd 0.0120          mean −274.5048 (error +0.0012), sd 0.0087
#   rev                mean −274.4931 (error +0.0129), sd 0.0306          mean −274.5079 (error −0.0019), sd 0.0417
#   mean               mean −274.4953 (error +0.0107), sd 0.0178          mean −274.5064 (error −0.0004), sd 0.0215
#   Λ, last round      2.303 (2.298 … 2.307)                              2.185 (2.179 … 2.191)
#   restarts           6124                                               6791
# The bar on the variational leg's forward estimate is 4·√(se² + s_var²) = 4·√(0.005² + 0.0087²) = 0.0401; s_var is far below the 0.25 at which
# the run would have to be lengthened. The first leg keeps pt_cases.DRIVER_BAR.
DRIVER_S_VAR = 0.0087
DRIVER_VAR_BAR = 4.0 * math.hypot(pc.MODEL_LOGZ_SE, DRIVER_S_VAR)
# Λ_var < Λ_fixed held at all eight seeds, but the ratio Λ_var/Λ_fixed was 0.946 … 0.952: above the 0.8 a pass condition would need. A mean-field
# normal on θ_t takes 5 % off the barrier of this orbit model, not the factor the Gaussian target shows; it is recorded, not asserted.
DRIVER_BARRIER_RATIOS = (0.946, 0.952)
DRIVER_BARRIER_ASSERTED = False
