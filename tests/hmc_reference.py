"""
The tempered HMC step of include/octofitter_hip_draws.h, restated in NumPy: the counter generator with its four purposes, the momenta,
Bijectors' invlink with logpdf_with_trans and its θ_t-derivative for the five prior kinds (analytic, in the reference's formulas), the
tempered target, the leapfrog and the decision. It imports nothing of the library: a prior is a dict(kind, p0, p1, lo, hi) with the kind
numbers of include/octofitter_hip.h, and the log-posterior is a callable the caller hands in (the oracle's callback in the tests).

    step = hmc_step(priors, theta_t, beta, eps, n_leapfrog, inv_mass, seed, step, chain0=0, logpost=None)
    step["theta_t"], step["proposal"], step["logpost"], step["loglike"], step["dH"], step["accepted"], step["log_u"]

Two deliberately broken variants serve the stationarity condition of tests/test_hmc_reference.py: always_accept=True skips the Metropolis
decision, mass_in_K=False sums K = ½ Σ p² without the inverse mass.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
PHILOX_W0, PHILOX_W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
KEY1 = 0x6F63746F64726177
PURPOSE_PRIOR, PURPOSE_UNIFORM, PURPOSE_MOMENTUM, PURPOSE_ACCEPT = 0, 1, 2, 3
UNIFORM, LOGUNIFORM, NORMAL, TRUNCNORMAL, SINE = 0, 1, 2, 3, 4
HEALED = -1.7976931348623157e308      # −floatmax: the value of a healed prior
EPS = 2.220446049250313e-16


# ---------------------------------------------------------------------------------------------------- the generator
def philox_int(key, ctr):
    """Philox4x64-10 on Python integers: key (k0, k1), counter (c0, c1, c2, c3) -> four 64-bit words."""
    k0, k1 = key
    c0, c1, c2, c3 = ctr
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 64) ^ c1 ^ k0, p1 & M64, (p0 >> 64) ^ c3 ^ k1, p0 & M64
        k0, k1 = (k0 + PHILOX_W0) & M64, (k1 + PHILOX_W1) & M64
    return c0, c1, c2, c3


def _mulhilo(a, b):
    a0, a1 = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    b0, b1 = b & m32, b >> s32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s32) + (p01 & m32) + (p10 & m32)
    return p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32), (mid << s32) | (p00 & m32)


def philox_vec(key, c0, c1, c2, c3):
    """The same rounds on uint64 arrays (one counter per element)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = key
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(PHILOX_M0, c0)
            hi1, lo1 = _mulhilo(PHILOX_M1, c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
            k0, k1 = (k0 + PHILOX_W0) & M64, (k1 + PHILOX_W1) & M64
    return c0, c1, c2, c3


def u01(x):
    """(2·(x >> 12) + 1)·2⁻⁵³"""
    return ((x >> np.uint64(12)) * np.uint64(2) + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def counter(purpose, i, d=0, step=0):
    """The counter of coordinate d of draw / chain i: (i, d // 4, purpose, step); purposes 0 and 1 have no step."""
    assert purpose in (PURPOSE_MOMENTUM, PURPOSE_ACCEPT) or step == 0
    return (int(i) & M64, d // 4, purpose, int(step) & M64)


def block_uniforms(seed, idx, D, purpose, step=0):
    """u[d][k] of index idx[k]: counter (i, d // 4, purpose, step), word d % 4."""
    idx = np.asarray(idx, dtype=np.uint64)
    out = np.empty((D, idx.size))
    for j in range((D + 3) // 4):
        words = philox_vec((seed, KEY1), idx, j, purpose, np.uint64(step))
        for q in range(4):
            if 4 * j + q < D:
                out[4 * j + q] = u01(words[q])
    return out


def prior_uniforms(seed, idx, D):
    return block_uniforms(seed, idx, D, PURPOSE_PRIOR)


def rejection_uniforms(seed, idx):
    return block_uniforms(seed, idx, 1, PURPOSE_UNIFORM)[0]


def chain_indices(chain0, W):
    return (np.uint64(chain0 & M64) + np.arange(W, dtype=np.uint64))      # wraps like the device's uint64


def momentum_uniforms(seed, step, chain0, W, D):
    return block_uniforms(seed, chain_indices(chain0, W), D, PURPOSE_MOMENTUM, step)


def momentum(seed, step, chain0, W, D, inv_mass=None):
    """p [D][W] = Φ⁻¹(u) / √inv_mass"""
    from scipy.special import ndtri
    z = ndtri(momentum_uniforms(seed, step, chain0, W, D))
    return z if inv_mass is None else z / np.sqrt(np.asarray(inv_mass, dtype=np.float64))[:, None]


def accept_uniforms(seed, step, chain0, W):
    return block_uniforms(seed, chain_indices(chain0, W), 1, PURPOSE_ACCEPT, step)[0]


# ---------------------------------------------------------------------------------------------------- the priors
def prior(kind, p0=0.0, p1=0.0, lo=-math.inf, hi=math.inf):
    return dict(kind=kind, p0=float(p0), p1=float(p1), lo=float(lo), hi=float(hi))


def support(pr):
    """The bounds the bijector is built on."""
    k = pr["kind"]
    if k in (UNIFORM, LOGUNIFORM):
        return pr["p0"], pr["p1"]
    if k == TRUNCNORMAL:
        return pr["lo"], pr["hi"]
    if k == SINE:
        return EPS, math.pi - EPS
    return -math.inf, math.inf


def scipy_dist(pr):
    """(cdf, ppf) of the prior in the natural domain."""
    import scipy.stats as ss
    k = pr["kind"]
    if k == UNIFORM:
        d = ss.uniform(pr["p0"], pr["p1"] - pr["p0"])
    elif k == LOGUNIFORM:
        d = ss.loguniform(pr["p0"], pr["p1"])
    elif k == NORMAL:
        d = ss.norm(pr["p0"], pr["p1"])
    elif k == TRUNCNORMAL:
        d = ss.truncnorm((pr["lo"] - pr["p0"]) / pr["p1"], (pr["hi"] - pr["p0"]) / pr["p1"], pr["p0"], pr["p1"])
    else:
        return (lambda x: (1 - np.cos(x)) / 2), (lambda u: np.arccos(1 - 2 * u))
    return d.cdf, d.ppf


def link(pr, x):
    """Bijectors.link of the support."""
    a, b = support(pr)
    if math.isfinite(a) and math.isfinite(b):
        u = (x - a) / (b - a)
        return np.log(u) - np.log1p(-u)
    if math.isfinite(a):
        return np.log(x - a)
    if math.isfinite(b):
        return np.log(b - x)
    return np.asarray(x, dtype=np.float64).copy()


def _sigmoid(y):
    em = np.exp(-np.abs(y))
    return np.where(y >= 0, 1.0 / (1.0 + em), em / (1.0 + em))


def invlink(pr, y):
    """(x, dx/dy)"""
    a, b = support(pr)
    if math.isfinite(a) and math.isfinite(b):
        sg = _sigmoid(y)
        return a + (b - a) * sg, (b - a) * sg * (1.0 - sg)
    if math.isfinite(a):
        return a + np.exp(y), np.exp(y)
    if math.isfinite(b):
        return b - np.exp(y), -np.exp(y)
    return np.asarray(y, dtype=np.float64).copy(), np.ones_like(y)


def prior_sample(priors, seed, idx):
    """(θ, θ_t) [D][n] of draws idx: the quantile of the restated uniform, moved one ulp inside a bound it rounds onto, then the link."""
    u = prior_uniforms(seed, idx, len(priors))
    th = np.empty_like(u)
    tt = np.empty_like(u)
    for d, pr in enumerate(priors):
        a, b = support(pr)
        x = scipy_dist(pr)[1](u[d])
        if math.isfinite(a):
            x = np.where(x > a, x, np.nextafter(a, math.inf))
        if math.isfinite(b):
            x = np.where(x < b, x, np.nextafter(b, -math.inf))
        th[d], tt[d] = x, link(pr, x)
    return th, tt


def logpdf_with_trans(pr, y):
    """(value, d/dθ_t) of logpdf(prior, x(θ_t)) + log|dx/dθ_t| at the linked value y. Outside the support: (−Inf, 0)."""
    from scipy.special import ndtr
    y = np.asarray(y, dtype=np.float64)
    k = pr["kind"]
    a, b = support(pr)
    x, dx = invlink(pr, y)
    with np.errstate(all="ignore"):
        if math.isfinite(a) and math.isfinite(b):
            ladj, ladj_d = np.log((x - a) * (b - x) / (b - a)), ((b - x) - (x - a)) / (b - a)      # d/dy log(σ(1 − σ)) = 1 − 2σ
        elif math.isfinite(a) or math.isfinite(b):
            ladj, ladj_d = y.copy(), np.ones_like(y)
        else:
            ladj, ladj_d = np.zeros_like(y), np.zeros_like(y)
        if k == UNIFORM:
            v, dv = np.full_like(y, -math.log(b - a)), np.zeros_like(y)
            inside = (x >= a) & (x <= b)
        elif k == LOGUNIFORM:
            v, dv = -np.log(x * math.log(b / a)), -1.0 / x
            inside = (x >= a) & (x <= b)
        elif k in (NORMAL, TRUNCNORMAL):
            z = (x - pr["p0"]) / pr["p1"]
            v, dv = -0.5 * (z * z + math.log(2 * math.pi)) - math.log(pr["p1"]), -z / pr["p1"]
            inside = np.ones(y.shape, dtype=bool)
            if k == TRUNCNORMAL:
                lo = ndtr((pr["lo"] - pr["p0"]) / pr["p1"]) if math.isfinite(pr["lo"]) else 0.0
                hi = ndtr((pr["hi"] - pr["p0"]) / pr["p1"]) if math.isfinite(pr["hi"]) else 1.0
                v = v - math.log(hi - lo)
                inside = (x >= pr["lo"]) & (x <= pr["hi"])
        else:
            v, dv = np.log(np.sin(x) / 2), np.cos(x) / np.sin(x)
            inside = (x > 0) & (x < math.pi)
        v = np.where(inside, v, -np.inf)
        dv = np.where(inside, dv, 0.0)
        return v + ladj, dv * dx + ladj_d


def logprior_t(priors, theta_t):
    """(ℓprior_t [W], ∇ℓprior_t [D][W]): the sum in declaration order; a non-finite term heals it — the sentinel, and a zero gradient."""
    theta_t = np.asarray(theta_t, dtype=np.float64)
    lpt = np.zeros(theta_t.shape[1])
    g = np.empty_like(theta_t)
    healed = np.zeros(theta_t.shape[1], dtype=bool)
    with np.errstate(all="ignore"):
        for d, pr in enumerate(priors):
            v, g[d] = logpdf_with_trans(pr, theta_t[d])
            healed |= ~np.isfinite(v)
            lpt = lpt + v
    return np.where(healed, HEALED, lpt), np.where(healed[None, :], 0.0, g)


# ---------------------------------------------------------------------------------------------------- the step
def tempered(priors, theta_t, beta, logpost):
    """(E, ∇E, dead, ℓπ, ℓprior_t) at theta_t. logpost(theta_t) -> (ℓπ [W], ∇ℓπ [D][W]); None: the prior alone (β = 0)."""
    lpt, gpr = logprior_t(priors, theta_t)
    W = theta_t.shape[1]
    if logpost is None:
        lp, glp = np.zeros(W), np.zeros_like(theta_t)
    else:
        lp, glp = logpost(theta_t)
    with np.errstate(all="ignore"):
        E = np.where(beta == 0.0, lpt, lpt + beta * (lp - lpt))
        gE = np.where(beta == 1.0, glp, np.where(beta == 0.0, gpr, beta * glp + (1.0 - beta) * gpr))
    dead = ~np.isfinite(E) | (lpt == HEALED) | ((beta > 0.0) & ~np.isfinite(lp))
    return E, gE, dead, lp, lpt


def hmc_step(priors, theta_t, beta, eps, n_leapfrog, inv_mass, seed, step, chain0=0, logpost=None, always_accept=False, mass_in_K=True):
    theta_t = np.array(theta_t, dtype=np.float64)
    D, W = theta_t.shape
    assert n_leapfrog >= 1 and D == len(priors)
    beta = np.zeros(W) if logpost is None else (np.ones(W) if beta is None else np.broadcast_to(np.asarray(beta, dtype=np.float64), (W,)))
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), (W,))
    im = np.ones(D) if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)
    imK = im if mass_in_K else np.ones(D)

    def kinetic(p):
        K = np.zeros(W)
        for d in range(D):
            K = K + imK[d] * p[d] * p[d]
        return 0.5 * K

    with np.errstate(all="ignore"):
        p = momentum(seed, step, chain0, W, D, inv_mass)
        E0, g, dead0, lp0, lpt0 = tempered(priors, theta_t, beta, logpost)
        H0 = -E0 + kinetic(p)
        q = theta_t.copy()
        p = p + 0.5 * eps * g
        for s in range(1, n_leapfrog + 1):
            q = q + eps * (im[:, None] * p)
            E1, g, dead1, lp1, lpt1 = tempered(priors, q, beta, logpost)
            p = p + (eps if s < n_leapfrog else 0.5 * eps) * g
        dH = H0 - (-E1 + kinetic(p))
        log_u = np.log(accept_uniforms(seed, step, chain0, W))
        acc = ~dead1 & (dead0 | (log_u < dH))
        if always_accept:
            acc = ~dead1
        out = np.where(acc[None, :], q, theta_t)
        lp = np.where(acc, lp1, lp0)
        ll = np.where(acc, lp1 - lpt1, lp0 - lpt0)
        ll = np.where(np.isfinite(ll), ll, -np.inf)
    return dict(theta_t=out, proposal=q, logpost=lp, loglike=ll, dH=dH, accepted=acc, log_u=log_u, E0=E0, E1=E1)
