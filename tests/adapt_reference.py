"""
The warm-up statistics of include/octofitter_hip_draws.h ("Warm-up of the explorer"), restated in NumPy: the grouped cross-chain moments with
their Chan merge, the metric, dual averaging of the step size, the per-chain running moments and R̂, the windowed schedule, and the warm-up
loop of host/callers.py: hmc_warmup on top of hmc_reference.hmc_step. It imports nothing of the library. exact_moments is the same
statistic in rational arithmetic (fractions), rounded once at the end: what tests/test_adapt_reference.py holds the restatement to and
tests/test_adapt.py the device.

The restatement sums in NumPy's order, the device in its own; both are held to bars that any summation order meets.
"""
import math
from fractions import Fraction

import numpy as np

import hmc_reference as hmc

MAX_GROUPS = 64                      # OCTO_DRAWS_MAX_GROUPS
DELTA, GAMMA, T0, KAPPA = 0.8, 0.05, 10.0, 0.75      # Stan's constants


# ---------------------------------------------------------------------------------------------------- grouped moments
def included(x, group, G):
    """[W] bool: the chains that enter — an id inside 0 … G − 1 and every one of the K values finite."""
    x = np.asarray(x, dtype=np.float64)
    gid = np.zeros(x.shape[1], dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    return (gid >= 0) & (gid < G) & np.all(np.isfinite(x), axis=0), gid


def exact_moments(x, group=None, G=1):
    """(count [G], mean [G][K], m2 [G][K], amax [G][K]) in rational arithmetic, each rounded once to a double; amax = max |x| of the group's row
    (0 for an empty group), the scale of the bar on the mean."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    keep, gid = included(x, group, G)
    cnt, mean, m2, amax = np.zeros(G), np.zeros((G, K)), np.zeros((G, K)), np.zeros((G, K))
    for g in range(G):
        cols = np.nonzero(keep & (gid == g))[0]
        n = cols.size
        cnt[g] = n
        if n == 0:
            continue
        for k in range(K):
            ratios = [float(t).as_integer_ratio() for t in x[k, cols]]      # every denominator is a power of two
            den = max(q for _, q in ratios)
            v = [p * (den // q) for p, q in ratios]                          # the values as integers over one denominator
            s1, s2 = sum(v), sum(t * t for t in v)
            mean[g, k] = float(Fraction(s1, n * den))
            m2[g, k] = float(Fraction(n * s2 - s1 * s1, n * den * den))      # Σ(x − mean)² = (n·Σx² − (Σx)²)/n, exact in integers
            amax[g, k] = np.max(np.abs(x[k, cols]))
    return cnt, mean, m2, amax


def moments(x, group=None, G=1, held=None):
    """(count [G], mean [G][K], m2 [G][K]) of this block of chains; held = (count, mean, m2): Chan-merged into those (accumulate = 1), new arrays."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    keep, gid = included(x, group, G)
    cnt, mean, m2 = np.zeros(G), np.zeros((G, K)), np.zeros((G, K))
    for g in range(G):
        v = x[:, keep & (gid == g)]
        cnt[g] = v.shape[1]
        if v.shape[1]:
            mean[g] = v.sum(axis=1) / v.shape[1]
            m2[g] = ((v - mean[g][:, None]) ** 2).sum(axis=1)
    if held is None:
        return cnt, mean, m2
    ca, ma, sa = (np.array(t, dtype=np.float64) for t in held)
    for g in range(G):
        nb, na = cnt[g], ca[g]
        if nb == 0:
            continue
        if na == 0:
            ca[g], ma[g], sa[g] = nb, mean[g], m2[g]
            continue
        n = na + nb
        d = mean[g] - ma[g]
        ma[g] = ma[g] + d * nb / n
        sa[g] = sa[g] + m2[g] + d * d * na * nb / n
        ca[g] = n
    return ca, ma, sa


def metric(count, m2, inv_mass, regularize=True):
    """inv_mass with the entries the call writes replaced: n >= 2 and the (shrunk) variance finite and > 0."""
    n = float(count)
    out = np.array(inv_mass, dtype=np.float64)
    if not n >= 2:
        return out
    with np.errstate(all="ignore"):
        var = np.asarray(m2, dtype=np.float64) / (n - 1.0)
        v = (n / (n + 5.0)) * var + 1e-3 * 5.0 / (n + 5.0) if regularize else var
    ok = np.isfinite(v) & (v > 0)
    out[ok] = v[ok]
    return out


# ---------------------------------------------------------------------------------------------------- dual averaging
def adapt_init(eps0, G=1):
    e = np.broadcast_to(np.asarray(eps0, dtype=np.float64), (G,))
    return np.stack([np.log(e), np.log(e), np.zeros(G), np.log(10.0 * e)], axis=1)


def accept_prob(dH, accepted):
    dH = np.asarray(dH, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(dH), np.where(np.asarray(accepted) != 0, 1.0, 0.0), np.minimum(1.0, np.exp(dH)))


def adapt_step(state, dH, accepted, k, group=None, delta=DELTA, gamma=GAMMA, t0=T0, kappa=KAPPA):
    """Update number k: (the new state [G][4], a_g [G] — NaN for an empty group, whose state is kept)."""
    state = np.array(state, dtype=np.float64)
    G = state.shape[0]
    a = accept_prob(dH, accepted)
    cnt, mean, _ = moments(a[None, :], group, G)
    a_g = np.where(cnt > 0, mean[:, 0], np.nan)
    eta, w = 1.0 / (k + t0), float(k) ** -kappa
    for g in range(G):
        if cnt[g] == 0:
            continue
        x, xbar, Hbar, mu = state[g]
        Hbar = (1.0 - eta) * Hbar + eta * (delta - a_g[g])
        x = mu - (math.sqrt(k) / gamma) * Hbar
        state[g] = x, w * x + (1.0 - w) * xbar, Hbar, mu
    return state, a_g


def eps_of(state, group, W, use_average=False, held=None):
    """d_eps_w: exp(x) — or exp(x̄) — of every chain's group; excluded chains keep `held` (NaN without it)."""
    G = state.shape[0]
    gid = np.zeros(W, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    out = np.full(W, np.nan) if held is None else np.array(held, dtype=np.float64)
    ok = (gid >= 0) & (gid < G)
    out[ok] = np.exp(state[gid[ok], 1 if use_average else 0])
    return out


def learn_stepsize_stan(a_seq, eps0, delta=DELTA, gamma=GAMMA, t0=T0, kappa=KAPPA):
    """Stan's stepsize_adaptation::learn_stepsize on scalars, transcribed: the (ε, ε̄) after each acceptance statistic of a_seq."""
    mu, counter, s_bar, x_bar = math.log(10 * eps0), 0, 0.0, 0.0
    out = []
    for adapt_stat in a_seq:
        counter += 1
        adapt_stat = 1 if adapt_stat > 1 else adapt_stat
        eta = 1.0 / (counter + t0)
        s_bar = (1.0 - eta) * s_bar + eta * (delta - adapt_stat)
        x = mu - s_bar * math.sqrt(counter) / gamma
        x_eta = counter ** -kappa
        x_bar = (1.0 - x_eta) * x_bar + x_eta * x
        out.append((math.exp(x), math.exp(x_bar)))
    return out


# ---------------------------------------------------------------------------------------------------- per-chain moments, R̂
def chain_moments(x, k, cmean, cm2):
    x = np.asarray(x, dtype=np.float64)
    if k == 1:
        return x.copy(), np.zeros_like(x)
    with np.errstate(all="ignore"):
        d = x - cmean
        mean = cmean + d / k
        return mean, cm2 + d * (x - mean)


def rhat(cmean, cm2, n):
    """R̂ [K] by the identity of the header: two moments calls on the per-chain arrays."""
    cnt, _, m2b = moments(cmean)
    _, mw, _ = moments(cm2)
    b_over_n = m2b[0] / (cnt[0] - 1.0)
    wv = mw[0] / (n - 1.0)
    return np.sqrt(((n - 1.0) / n * wv + b_over_n) / wv)


def rhat_direct(samples):
    """R̂ [K] of stored draws [n][K][C] (chains with a non-finite draw left out): Gelman & Rubin's formula on the draws themselves."""
    s = np.asarray(samples, dtype=np.float64)
    s = s[:, :, np.all(np.isfinite(s), axis=(0, 1))]
    n = s.shape[0]
    wv = s.var(axis=0, ddof=1).mean(axis=1)
    b_over_n = s.mean(axis=0).var(axis=1, ddof=1)
    return np.sqrt(((n - 1.0) / n * wv + b_over_n) / wv)


# ---------------------------------------------------------------------------------------------------- the schedule and the loop
def warmup_windows(n):
    """(initial buffer, [slow windows], terminal buffer): Stan's 75 / 25·2^j / 50, or 15 % / the rest / 10 % when 150 rounds do not fit; a window
    takes all that is left in front of the terminal buffer unless a window of twice its length would still fit behind it."""
    if n < 20:
        return n, [], 0
    init, term, size = 75, 50, 25
    if n < init + size + term:
        init, term = int(15 * n / 100), int(10 * n / 100)
        size = n - init - term
    left, out = n - init - term, []
    while left > 0:
        take = size if left >= 3 * size else left
        out.append(take)
        left -= take
        size *= 2
    return init, out, term


def round_flags(n):
    """Per round r: (in a slow window, first of its window, last of its window)."""
    init, windows, _ = warmup_windows(n)
    flags = [(False, False, False)] * n
    at = init
    for length in windows:
        for r in range(at, at + length):
            flags[r] = (True, r == at, r == at + length - 1)
        at += length
    return flags


def hmc_warmup(priors, theta_t, n_warmup, n_leapfrog, eps, inv_mass, seed, step=0, chain0=0, logpost=None, delta=DELTA):
    """host/callers.py: hmc_warmup on hmc_reference.hmc_step. Returns dict(theta_t, eps, inv_mass, accept_stat [n], accepted [n][W], step)."""
    tt = np.array(theta_t, dtype=np.float64)
    im = np.array(inv_mass, dtype=np.float64)
    state = adapt_init(eps)
    e = float(np.exp(state[0, 0]))
    a_rec, acc_rec, mom, k = [], [], None, 0
    for r, (inside, first, last) in enumerate(round_flags(n_warmup)):
        s = hmc.hmc_step(priors, tt, None, e, n_leapfrog, im, seed, step + r, chain0=chain0, logpost=logpost)
        tt = s["theta_t"]
        k += 1
        state, a = adapt_step(state, s["dH"], s["accepted"], k, delta=delta)
        e = float(np.exp(state[0, 1 if r == n_warmup - 1 else 0]))
        a_rec.append(a[0])
        acc_rec.append(s["accepted"])
        if inside:
            mom = moments(tt, held=None if first else mom)
        if last:
            im = metric(mom[0][0], mom[2][0], im, regularize=True)
            state = adapt_init(np.exp(state[:, 1]))
            e, k = float(np.exp(state[0, 0])), 0
    return dict(theta_t=tt, eps=e, inv_mass=im, accept_stat=np.array(a_rec), accepted=np.array(acc_rec), step=step + n_warmup)
