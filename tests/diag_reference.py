"""
The NumPy restatement of the convergence diagnostics include/octofitter_hip_draws.h states ("Convergence diagnostics of stored draws"): the
split, the validity of a row, the type-7 quantiles, the average ranks and their normal scores, Stan's effective sample size with Geyer's
truncation written as Stan writes it, split-R̂, and the cross-chain sums in the order the header documents (a butterfly over the 64 lanes of a
wave, four waves in wave order, blocks of 256 split chains in block order). Plain loops and direct sums; scipy.special.ndtri for the normal
scores. dtype=np.longdouble runs the same statements in extended precision (the normal scores then come from mpmath, which only that run needs):
tools/diag_bench.py records the gap between the two runs, and the bars of tests/test_diag.py are written from it. A plain module, not a test module.

diagnose() also returns the DECISION MARGINS: the smallest |even + odd| any test of Geyer's loop met and the smallest gap of any comparison of
the monotone pass. A case whose margins are far above the arithmetic's error takes the same branches on every implementation. With them comes the
lag max_t at which each of Geyer's loops stopped: the suite pins by it which cases walk ρ_t beyond the lags the device keeps in LDS.
"""
import math

import numpy as np

RHAT, ESS_BULK, ESS_TAIL, RHAT_BASIC, ESS_BASIC, Q05, Q50, Q95, N_STATS = range(9)
NAMES = ("rhat", "ess_bulk", "ess_tail", "rhat_basic", "ess_basic", "q05", "q50", "q95")
SORT_BLOCK, LAG_BLOCK, CHAIN_BLOCK = 2048, 16, 256


def work_doubles(n, W, K):
    """octo_draws_diagnose_work_doubles: 2K(P + S) + 10KM + 4K·T·(nblk + 1) + 5K"""
    N, M = n // 2, 2 * W
    S = M * N
    P = SORT_BLOCK
    while P < S:
        P *= 2
    T, nblk = -(-N // LAG_BLOCK) * LAG_BLOCK, -(-M // CHAIN_BLOCK)
    return 2 * K * (P + S) + 10 * K * M + 4 * K * T * (nblk + 1) + 5 * K


def used(x):
    """[K, M, N] of x [n, K, W]: draw i of split chain m = h·W + w is sample h·(n − N) + i of chain w; n odd: the middle sample is unused"""
    x = np.asarray(x)
    n, K, W = x.shape
    N = n // 2
    return np.concatenate([x[:N], x[n - N:]], axis=2).transpose(1, 2, 0)      # [N, K, 2W] -> [K, M, N]


def unsplit(v, n, fill=np.nan):
    """the inverse of used(): [n, K, W] of v [K, M, N], the unused sample holding `fill`"""
    K, M, N = v.shape
    W = M // 2
    out = np.full((n, K, W), fill, dtype=v.dtype)
    out[:N] = v[:, :W].transpose(2, 0, 1)
    out[n - N:] = v[:, W:].transpose(2, 0, 1)
    return out


def quantile7(s, p):
    S = s.size
    h = s.dtype.type(S - 1) * s.dtype.type(p)
    lo = int(math.floor(h))
    return s[lo] + (h - s.dtype.type(lo)) * (s[min(lo + 1, S - 1)] - s[lo])


def average_ranks(v, s):
    """r(x) = #{s < x} + (#{s = x} + 1)/2 of every element of v among the sorted s; exact in a double"""
    lo, hi = np.searchsorted(s, v, "left"), np.searchsorted(s, v, "right")
    return lo + (hi - lo + 1) / 2.0


def ndtri(p):
    if p.dtype == np.float64:
        from scipy.special import ndtri as f
        return f(p)
    import mpmath
    mpmath.mp.prec = 80
    upper = p > 0.5                                     # z(1 − p) = −z(p): half as many evaluations
    u, inv = np.unique(np.where(upper, 1 - p, p), return_inverse=True)
    z = np.empty(u.size, dtype=np.longdouble)
    for k, t in enumerate(u):      # a long double is the exact sum of two doubles, in both directions
        hi = float(t)
        m = mpmath.sqrt(2) * mpmath.erfinv(2 * (mpmath.mpf(hi) + mpmath.mpf(float(t - np.longdouble(hi)))) - 1)
        hi = float(m)
        z[k] = np.longdouble(hi) + np.longdouble(float(m - mpmath.mpf(hi)))
    z = z[inv.reshape(p.shape)]
    return np.where(upper, -z, z)


def normal_scores(v, dtype=np.float64):
    """(r, z) of v [M, N] among its own S values: z = ndtri((r − 3/8)/(S + 1/4))"""
    r = average_ranks(v, np.sort(v, axis=None))
    S = v.size
    return r, ndtri((r.astype(dtype) - dtype(0.375)) / (dtype(S) + dtype(0.25)))


def chain_sum(v):
    """Σ over the last axis (the M split chains) in the documented order"""
    M = v.shape[-1]
    nblk = -(-M // CHAIN_BLOCK)
    a = np.zeros(v.shape[:-1] + (nblk * CHAIN_BLOCK,), dtype=v.dtype)
    a[..., :M] = v
    a = a.reshape(v.shape[:-1] + (nblk, CHAIN_BLOCK // 64, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    waves = a[..., 0]                                   # [..., nblk, 4]: the same bits in every lane
    total = np.zeros(v.shape[:-1], dtype=v.dtype)
    for b in range(nblk):
        t = np.zeros(v.shape[:-1], dtype=v.dtype)
        for u in range(CHAIN_BLOCK // 64):
            t = t + waves[..., b, u]
        total = total + t
    return total


def ordered_sum(a):
    """Σ over the last axis in index order"""
    return np.cumsum(a, axis=-1)[..., -1]


class Margins:
    """geyer, monotone: the margins. max_t: the lag at which Geyer's loop stopped, None where ess() is NaN before it: of one row a list in
    the order of the calls of ess() (QUANTITIES), of a cube a dict row -> that list (valid rows only)."""
    QUANTITIES = ("z", "x <= q05", "x <= q95", "x")

    def __init__(self):
        self.geyer, self.monotone = math.inf, math.inf
        self.max_t = []

    def merge(self, other):
        self.geyer, self.monotone = min(self.geyer, other.geyer), min(self.monotone, other.monotone)


def lag0(v):
    """(μ_m [M], centred draws [M, N], W̄, var⁺) of v [M, N]"""
    M, N = v.shape
    t = v.dtype.type
    mu = ordered_sum(v) / t(N)
    c = v - mu[:, None]
    var = ordered_sum(c * c) / t(N) * t(N) / t(N - 1)
    wbar = chain_sum(var) / t(M)
    mubar = chain_sum(mu) / t(M)
    d = mu - mubar
    varplus = wbar * t(N - 1) / t(N) + chain_sum(d * d) / t(M - 1)
    return mu, c, wbar, varplus


def rhat(v):
    _, _, wbar, varplus = lag0(v)
    with np.errstate(all="ignore"):
        return np.sqrt(varplus / wbar)


def ess(v, margins=None):
    """Stan's compute_effective_sample_size of v [M, N], Geyer's truncation as Stan writes it"""
    M, N = v.shape
    t_ = v.dtype.type
    S = M * N
    _, c, wbar, varplus = lag0(v)
    if not (np.isfinite(varplus) and varplus > 0):
        if margins is not None:
            margins.max_t.append(None)
        return t_(np.nan)
    cache = {}

    def rho(t):
        if t not in cache:
            acov = ordered_sum(c[:, :N - t] * c[:, t:]) / t_(N)
            cache[t] = t_(1) - (wbar - chain_sum(acov) / t_(M)) / varplus
        return cache[t]

    hat = np.zeros(N + 2, dtype=v.dtype)
    even, odd = t_(1), rho(1)
    hat[0], hat[1] = even, odd
    t = 1
    while t < N - 4:
        if margins is not None:
            margins.geyer = min(margins.geyer, abs(float(even + odd)))
        if not even + odd > 0:
            break
        even, odd = rho(t + 1), rho(t + 2)
        if margins is not None:
            margins.geyer = min(margins.geyer, abs(float(even + odd)))      # the test that stores the pair
        if even + odd >= 0:
            hat[t + 1], hat[t + 2] = even, odd
        t += 2
    max_t = t
    if margins is not None:
        margins.max_t.append(max_t)
    if even > 0:
        hat[max_t + 1] = even
    for t in range(1, max_t - 2, 2):
        before, after = hat[t - 1] + hat[t], hat[t + 1] + hat[t + 2]
        if margins is not None:
            margins.monotone = min(margins.monotone, abs(float(after - before)))
        if after > before:
            hat[t + 1] = before / t_(2)
            hat[t + 2] = hat[t + 1]
    s = t_(0)
    for t in range(max_t):
        s = s + hat[t]
    tau = t_(-1) + t_(2) * s + hat[max_t + 1]
    floor = t_(1) / np.log10(t_(S))
    return t_(S) / max(tau, floor)


def nan_max(a, b):
    return a if np.isnan(a) else b if np.isnan(b) else max(a, b)


def nan_min(a, b):
    return a if np.isnan(a) else b if np.isnan(b) else min(a, b)


def diagnose(x, dtype=np.float64):
    """x [n, K, W] (or [n, W]) float64. Returns dict(stats [N_STATS, K] of dtype, rank, z, rank_folded, z_folded [n, K, W] with NaN in the unused sample
    and in invalid rows, margins). The order statistics and the ranks are made of the float64 draws whatever dtype is; everything after them runs in dtype."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, None, :]
    n, K, W = x.shape
    v64 = used(x)
    _, M, N = v64.shape
    stats = np.full((N_STATS, K), np.nan, dtype=dtype)
    planes = {name: np.full((K, M, N), np.nan, dtype=np.float64 if name.startswith("rank") else dtype) for name in ("rank", "z", "rank_folded", "z_folded")}
    margins = Margins()
    margins.max_t = {}
    for k in range(K):
        row = v64[k]
        if not np.all(np.isfinite(row)) or row.min() == row.max():
            continue
        s = np.sort(row, axis=None)
        q05, q50, q95 = (quantile7(s, p) for p in (0.05, 0.5, 0.95))
        r, z = normal_scores(row, dtype)
        rf, zf = normal_scores(np.abs(row - q50), dtype)
        planes["rank"][k], planes["z"][k], planes["rank_folded"][k], planes["z_folded"][k] = r, z, rf, zf
        v = row.astype(dtype)
        m = Margins()
        stats[RHAT, k] = nan_max(rhat(z), rhat(zf))
        stats[ESS_BULK, k] = ess(z, m)
        stats[ESS_TAIL, k] = nan_min(ess((row <= q05).astype(dtype), m), ess((row <= q95).astype(dtype), m))
        stats[RHAT_BASIC, k] = rhat(v)
        stats[ESS_BASIC, k] = ess(v, m)
        stats[Q05, k], stats[Q50, k], stats[Q95, k] = q05, q50, q95
        margins.merge(m)
        margins.max_t[k] = m.max_t
    out = {name: unsplit(p, n) for name, p in planes.items()}
    out.update(stats=stats, margins=margins)
    return out
