"""
The variational reference of a tempering leg (include/octofitter_hip_draws.h, "The variational reference of a tempering leg"), restated in NumPy:
the table rule of octo_draws_reference_set_device / _fit_device (table, fit), the exchange of two legs' target replicas
(octo_draws_reference_exchange_device: exchange, with ℓprior_t from hmc_reference.logprior_t on Normal priors), and the two-leg round loop of
host/callers.py: octofit_pigeons_device(n_temps_variational=…) on top of the pieces of pt_reference.pigeons (two_legs). It imports nothing of the
library.
"""
import numpy as np

import hmc_reference as ref
import pt_reference as pt

PRIOR_NC, IC_N, PRIOR_DOUBLES = 4, 4, 5      # the constants per prior of the density and of the quantile; sizeof(octo_prior)/8


def table_doubles(D):
    """octo_draws_reference_doubles: octo_prior [D] · pc [D][4] · ic [D][4] · μ [D] · σ [D]"""
    return (PRIOR_DOUBLES + PRIOR_NC + IC_N + 2) * D if D >= 1 else 0


def parts(D):
    """name -> (first double, doubles) of the table's parts, in order"""
    out, o = {}, 0
    for name, n in (("priors", PRIOR_DOUBLES * D), ("pc", PRIOR_NC * D), ("ic", IC_N * D), ("mean", D), ("sd", D)):
        out[name] = (o, n)
        o += n
    return out


def table(mean, sd, n=None):
    """The rule of k_vref_table for μ = mean, σ = sd (n: the fit's count, None for a set). Returns dict(bad [D] bool, priors: one
    hmc_reference.prior per coordinate (None where bad), pc [D][4], ic [D][4]); the rows of bad coordinates hold NaN here — the device keeps
    what the buffer held."""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    bad = ~np.isfinite(mean) | ~np.isfinite(sd) | ~(sd > 0.0)
    if n is not None and not n >= 2:
        bad[:] = True
    with np.errstate(all="ignore"):
        pc = np.stack([np.full(mean.shape, np.nan), np.zeros(mean.shape), -np.log(sd), 1.0 / sd], axis=1)
    pc[bad] = np.nan
    ic = np.zeros((mean.size, IC_N))
    ic[bad] = np.nan
    priors = [None if b else ref.prior(ref.NORMAL, m, s) for m, s, b in zip(mean, sd, bad)]
    return dict(bad=bad, priors=priors, pc=pc, ic=ic, mean=np.where(bad, np.nan, mean), sd=np.where(bad, np.nan, sd))


def fit(count, mean, m2, inflate=1.0):
    """(μ, σ, n) of octo_draws_reference_fit_device from one group's moments: σ = inflate·√(M2/(n − 1)), every operation rounded by itself"""
    n = float(np.asarray(count).reshape(-1)[0])
    with np.errstate(all="ignore"):
        sd = inflate * np.sqrt(np.asarray(m2, dtype=np.float64) / (n - 1.0))
    return np.asarray(mean, dtype=np.float64), sd, n


def normal_priors(mean, sd):
    return [ref.prior(ref.NORMAL, m, s) for m, s in zip(mean, sd)]


def log_q(priors, theta_t):
    """(ℓprior_t [W], healed [W]) of the points theta_t [D][W] under a table's priors"""
    lpt, _ = ref.logprior_t(priors, theta_t)
    return lpt, lpt == ref.HEALED


def potential(lp, lpt, healed):
    """the swap potential ℓπ − ℓprior_t: −Inf where it is not finite or the prior was healed (the rule of host/callers.py: _finite_or_neg_inf)"""
    with np.errstate(all="ignore"):
        v = lp - lpt
    return np.where(np.isfinite(v) & ~healed, v, -np.inf)


def exchange(Cn, leg_a, leg_b):
    """octo_draws_reference_exchange_device on copies. A leg is dict(T, slot2rep [Cn][T], theta [D][ld], lp [>= T·Cn], ll [>= T·Cn], priors: the
    reference's hmc_reference priors). Returns the two legs after the call."""
    a, b = ({k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in leg.items()} for leg in (leg_a, leg_b))
    c = np.arange(Cn)
    ra, rb = a["slot2rep"][:, 0], b["slot2rep"][:, 0]
    go = (ra >= 0) & (ra < a["T"]) & (rb >= 0) & (rb < b["T"])
    ca, cb = (ra * Cn + c)[go], (rb * Cn + c)[go]
    th_a, th_b = a["theta"][:, ca].copy(), b["theta"][:, cb].copy()
    lp_a, lp_b = a["lp"][ca].copy(), b["lp"][cb].copy()
    a["theta"][:, ca], b["theta"][:, cb] = th_b, th_a
    a["lp"][ca], b["lp"][cb] = lp_b, lp_a
    a["ll"][ca] = potential(lp_b, *log_q(a["priors"], th_b))
    b["ll"][cb] = potential(lp_a, *log_q(b["priors"], th_a))
    return a, b


def two_legs(explore, prior, T, Tv, Cn, n_rounds, rng, first_tuning_round=5, inflate=1.0, fit_reference=True):
    """The round loop of octofit_pigeons_device(n_temps_variational=Tv) around an explorer callback, from pt_reference.pigeons' pieces.
    explore(leg, β [Tl][Cn], scan, reference) -> (x [Tl][Cn][D], ℓπ [Tl][Cn]) explores leg 0 or 1 (the refresh of its β = 0 replicas included)
    under `reference` = None (the prior: `prior`, a list of hmc_reference priors on θ_t) or (μ [D], σ [D]). A scan: explore both legs; the swap
    potential ℓπ − log reference; the target replicas of both legs into the round's moments; the exchange; statistics, restarts and the swap per
    leg. At the end of round first_tuning_round − 1 <= r < n_rounds the normal is fitted to the round's target draws (fit_reference=False: never,
    the leg stays on the prior). Returns a list of two dicts as pt_reference.pigeons returns them, the second with mean_by_round, sd_by_round."""
    legs = []
    for Tl in (T, Tv):
        legs.append(dict(T=Tl, beta=pt.cubic_ladder(Tl), slot2rep=np.tile(np.arange(Tl), (Cn, 1)), leg=np.zeros((Cn, Tl), dtype=np.int64),
                         count=np.zeros(Cn, dtype=np.int64), acc=pt.new_acc(Tl), betas=[pt.cubic_ladder(Tl)], rej=[], lam=[], s=None, priors=prior))
    c = np.arange(Cn)
    active, scan = None, 0
    means, sds = [], []
    for r in range(1, n_rounds + 1):
        draws = []
        for _ in range(2 ** r):
            for k, g in enumerate(legs):
                rep2slot = np.empty_like(g["slot2rep"])
                rep2slot[c[:, None], g["slot2rep"]] = np.arange(g["T"])[None, :]
                x, lp = explore(k, g["beta"][rep2slot.T], scan, active if k == 1 else None)
                theta = x.reshape(g["T"] * Cn, -1).T.copy()
                g.update(theta=theta, lp=lp.reshape(-1).copy(), ll=potential(lp.reshape(-1), *log_q(g["priors"], theta)))
                draws.append(theta[:, g["slot2rep"][:, 0] * Cn + c])
            legs = list(exchange(Cn, *legs))
            for g in legs:
                ll = g["ll"].reshape(g["T"], Cn)
                g["acc"] = pt.stats(ll, g["slot2rep"], g["beta"], g["acc"])
                pt.restarts(g["slot2rep"], g["leg"], g["count"])
                g["slot2rep"], _ = pt.swap(ll, g["beta"], g["slot2rep"], scan % 2, 1.0 - rng.random((Cn, g["T"])))
            scan += 1
        if fit_reference and first_tuning_round - 1 <= r < n_rounds:
            x = np.concatenate(draws, axis=1)
            mu = x.mean(axis=1)
            mean, sd, n = fit(x.shape[1], mu, ((x - mu[:, None]) ** 2).sum(axis=1), inflate)
            if not table(mean, sd, n)["bad"].any():
                active = (mean, sd)
                legs[1]["priors"] = normal_priors(mean, sd)
        means.append(np.full(len(prior), np.nan) if active is None else active[0])
        sds.append(np.full(len(prior), np.nan) if active is None else active[1])
        for g in legs:
            g["s"] = pt.schedule(g["acc"], g["beta"], adapt=r < n_rounds, reset=True)
            g["beta"], g["acc"] = g["s"]["beta"], g["s"]["acc"]
            g["betas"].append(g["beta"].copy())
            g["rej"].append(g["s"]["rej"])
            g["lam"].append(g["s"]["summary"][pt.LAMBDA])
    out = [dict(betas_by_round=np.array(g["betas"]), rejection_by_round=np.array(g["rej"]), barrier_by_round=np.array(g["lam"]),
                log_evidence=tuple(g["s"]["summary"][1:]), restarts=g["count"], n_scans=scan, slot2rep=g["slot2rep"]) for g in legs]
    out[1].update(mean_by_round=np.array(means), sd_by_round=np.array(sds))
    return out
