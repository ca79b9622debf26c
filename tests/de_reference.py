"""
Differential evolution as include/octofitter_hip_draws.h states it (octo_draws_de_device), restated in NumPy on top of tests/hmc_reference.py
(the counter generator, the priors) and the evaluation rule of tests/nuts_reference.py (a linked x that rounds onto a bound of its support is
dead): purpose 12 of the generator, jDE's self-adapted (F, CR), parents from a ring neighbourhood, binomial crossover, the bound repair and
the synchronous selection. Vectorised over the individuals. It imports nothing of the library; `logpost` is the callable
hmc_reference.hmc_step takes (its gradient is never looked at), None: f = ℓprior_t.

    s = de_open(priors, theta_t, logpost=None, fcr=None)          # the state: X, f, ℓ, ℓprior_t, (F, CR), n_accept
    t = de_trial(s, seed, gen, radius, lo=None, hi=None)          # the trial points of generation gen and what made them
    s, g = de_generation(priors, s, seed, gen, radius, lo, hi, logpost)      # one generation: the new state and its record
    s, gens = de_run(priors, s, seed, gen0, n_gen, radius, lo, hi, logpost)

A generation's record holds the trial points `trial`, the parents' indices `parents` [3][W], `jrand`, the masks `cross` and `repaired` [D][W], (F′, CR′), whether
either was drawn anew, f′, `accepted`, and the selection MARGIN |f′ − f_i| / max(1, |f_i|) (Inf where either is −Inf: nothing to round). An
individual whose margin exceeds MARGIN = 1e-6 is DECIDED: a computation that differs in the last bits makes the same selection.
"""
import numpy as np

import hmc_reference as ref
import nuts_reference as nuts

PURPOSE_DE = 12
TAU_F, F_LOW, F_SPAN, TAU_CR, F0, CR0 = 0.1, 0.1, 0.9, 0.1, 0.5, 0.9
MARGIN = 1e-6


def de_words(seed, gen, idx, k):
    """the four uniforms of counter (i, k, 12, gen), one row per word"""
    words = ref.philox_vec((seed, ref.KEY1), np.asarray(idx, dtype=np.uint64), np.asarray(k, dtype=np.uint64), PURPOSE_DE, np.uint64(gen & ref.M64))
    return np.stack([ref.u01(w) for w in words])


def pick(u, n):
    """⌊u·n⌋, never n"""
    return np.minimum((u * float(n)).astype(np.int64), n - 1)


def neighbourhood_size(W, radius):
    return W - 1 if radius == 0 else min(max(2 * radius, 3), W - 1)


def member(i, k, n, W):
    h = n // 2
    return (i - h + k + (k >= h)) % W


def evaluate(priors, theta_t, logpost):
    """(f, ℓπ or 0, ℓprior_t) at the columns of theta_t: f = ℓπ, without a callback ℓprior_t; −Inf at a dead or non-finite point"""
    S = nuts._Setup(priors, theta_t, None, 1.0, None, 0, 0, 0, logpost)
    with np.errstate(all="ignore"):
        _E, _g, dead, lp, lpt = S.evaluate(S.theta_t, slice(None))
        f = lpt if logpost is None else lp
        dead = dead | ~np.isfinite(f)
    return np.where(dead, -np.inf, f), lp, lpt


def de_open(priors, theta_t, logpost=None, fcr=None):
    X = np.array(theta_t, dtype=np.float64)
    W = X.shape[1]
    f, _lp, lpt = evaluate(priors, X, logpost)
    F, CR = (np.full(W, F0), np.full(W, CR0)) if fcr is None else (np.array(fcr[0], dtype=np.float64), np.array(fcr[1], dtype=np.float64))
    return dict(theta_t=X, f=f, lpt=lpt, F=F, CR=CR, n_accept=np.zeros(W, dtype=np.int64))


def de_trial(s, seed, gen, radius, lo=None, hi=None):
    X = s["theta_t"]
    D, W = X.shape
    assert W >= 4 and radius >= 0 and (lo is None) == (hi is None)
    i = np.arange(W)
    n = neighbourhood_size(W, radius)
    u0, u1 = de_words(seed, gen, i, 0), de_words(seed, gen, i, 1)
    new_F, new_CR = u1[0] < TAU_F, u1[2] < TAU_CR
    Ft = np.where(new_F, F_LOW + F_SPAN * u1[1], s["F"])
    CRt = np.where(new_CR, u1[3], s["CR"])
    a = pick(u0[0], n)
    b = pick(u0[1], n - 1)
    b = b + (b >= a)
    c = pick(u0[2], n - 2)
    c = c + (c >= np.minimum(a, b))
    c = c + (c >= np.maximum(a, b))
    picks = np.stack([a, b, c])
    parents = member(i[None, :], picks, n, W)
    r1, r2, r3 = parents
    jrand = pick(u0[3], D)
    V = X.copy()
    cross = np.zeros((D, W), dtype=bool)
    repaired = np.zeros((D, W), dtype=bool)
    with np.errstate(all="ignore"):
        for d0 in range(0, D, 4):
            uc = de_words(seed, gen, i, 2 + d0 // 4)
            ub = de_words(seed, gen, i, 18 + d0 // 4)
            for q in range(min(4, D - d0)):
                d = d0 + q
                cr = (jrand == d) | (uc[q] < CRt)
                diff = X[d, r1] - X[d, r2]
                step = Ft * diff
                v = np.where(cr, X[d, r3] + step, X[d])
                if lo is not None:
                    low, high = cr & (v < lo[d]), cr & (v > hi[d])
                    v = np.where(low, lo[d] + ub[q] * (X[d] - lo[d]), v)
                    v = np.where(high, hi[d] - ub[q] * (hi[d] - X[d]), v)
                    repaired[d] = low | high
                V[d], cross[d] = v, cr
    return dict(trial=V, parents=parents, picks=picks, n=n, jrand=jrand, cross=cross, repaired=repaired, Ft=Ft, CRt=CRt, new_F=new_F, new_CR=new_CR)


def de_select(s, t, fp, lpt_p):
    """the synchronous selection of a generation from f′ and ℓprior_t of its trial points: the new state and the record"""
    f = s["f"]
    with np.errstate(all="ignore"):
        acc = (fp > -np.inf) & (fp >= f)
        margin = np.where(np.isfinite(fp) & np.isfinite(f), np.abs(fp - f) / np.maximum(1.0, np.abs(f)), np.inf)
    new = dict(theta_t=np.where(acc[None, :], t["trial"], s["theta_t"]), f=np.where(acc, fp, f), lpt=np.where(acc, lpt_p, s["lpt"]),
               F=np.where(acc, t["Ft"], s["F"]), CR=np.where(acc, t["CRt"], s["CR"]), n_accept=s["n_accept"] + acc)
    return new, dict(t, f_trial=fp, lpt_trial=lpt_p, accepted=acc, margin=margin)


def de_generation(priors, s, seed, gen, radius, lo=None, hi=None, logpost=None):
    t = de_trial(s, seed, gen, radius, lo, hi)
    fp, _lp, lpt_p = evaluate(priors, t["trial"], logpost)
    return de_select(s, t, fp, lpt_p)


def de_run(priors, s, seed, gen0, n_gen, radius, lo=None, hi=None, logpost=None):
    gens = []
    for g in range(n_gen):
        s, rec = de_generation(priors, s, seed, gen0 + g, radius, lo, hi, logpost)
        gens.append(rec)
    return s, gens


def loglike(s):
    with np.errstate(all="ignore"):
        ll = s["f"] - s["lpt"]
    return np.where(np.isfinite(ll), ll, -np.inf)


def best(s):
    """(index, f) of the highest finite f, ties to the lower index; (−1, −Inf) with none"""
    f = s["f"]
    if not np.any(f > -np.inf):
        return -1, -np.inf
    k = int(np.argmax(f))      # the first of the maxima
    return k, float(f[k])
