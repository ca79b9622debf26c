"""Reference side of the PSIS tests (a helper, not a test; tools/psis_bench.py uses it too): the algorithm of include/octofitter_hip_psis.h
restated twice — psis_row in float64 NumPy (stable argsorts) and psis_row_mp in 40-digit mpmath — the Zhang–Stephens fit on its own
(gpdfit), the case generator of tests/test_psis.py and the comparison at its bars."""
import math

import numpy as np

EPS = 2.0 ** -52
LOG_TINY = float(np.log(np.finfo(np.float64).tiny))      # log(DBL_MIN) = −708.3964185322641
FIELDS = ("n", "tail_len", "pareto_k", "elpd_loo", "lppd", "ess")
MAX_TAIL = 4096


def tail_len(n):
    """M(n) = ceil(min(n/5, 3·√n)) in double arithmetic."""
    return 0 if n <= 0 else int(math.ceil(min(n / 5.0, 3.0 * math.sqrt(n))))


def _lse(a):
    m = np.max(a)
    return m + np.log(np.sum(np.exp(a - m)))


def gpdfit(y):
    """(k̂, σ) of the ascending sample y of a generalised Pareto distribution located at 0: Zhang & Stephens (2009) with the PSIS prior."""
    y = np.asarray(y, dtype=np.float64)
    tl = y.size
    m = 30 + math.isqrt(tl)
    j = np.arange(1, m + 1, dtype=np.float64)
    b = (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * y[int(math.floor(tl / 4.0 + 0.5)) - 1]) + 1.0 / y[tl - 1]
    k = np.log1p(-b[:, None] * y[None, :]).mean(axis=1)
    L = tl * (np.log(-b / k) - k - 1.0)
    with np.errstate(over="ignore"):      # exp(L_l − L_j) = +Inf for a hopeless grid point j: w_j = 0
        w = 1.0 / np.exp(L[None, :] - L[:, None]).sum(axis=1)
    w = np.where(w < 10.0 * EPS, 0.0, w)
    w = w / w.sum()
    bb = float(np.sum(w * b))
    kk = float(np.log1p(-bb * y).mean())
    return (tl * kk + 5.0) / (tl + 10.0), -kk / bb


def tail_order(ll):
    """The sample indices of a row's tail, ascending by (x, sample index), in float64; empty for n <= M."""
    ll = np.asarray(ll, dtype=np.float64)
    idx = np.nonzero(np.isfinite(ll))[0]
    n = idx.size
    M = tail_len(n)
    if n <= M:
        return idx[:0]
    x = -ll[idx] - np.max(-ll[idx])
    tail = np.nonzero(x > max(np.sort(x)[n - 1 - M], LOG_TINY))[0]
    return idx[tail[np.argsort(x[tail], kind="stable")]]


def psis_row(ll):
    """One row in float64: dict(n, tail_len, pareto_k, elpd_loo, lppd, ess, lw [S])."""
    ll = np.asarray(ll, dtype=np.float64)
    idx = np.nonzero(np.isfinite(ll))[0]
    v = ll[idx]
    n = v.size
    lw = np.full(ll.size, -np.inf)
    if n == 0:
        return dict(n=0.0, tail_len=np.nan, pareto_k=np.nan, elpd_loo=np.nan, lppd=np.nan, ess=np.nan, lw=lw)
    x = -v - np.max(-v)
    M = tail_len(n)
    khat, tl = np.inf, 0
    if n > M:
        xc = max(np.sort(x)[n - 1 - M], LOG_TINY)      # the (M+1)-th largest
        tail = np.nonzero(x > xc)[0]
        tl = tail.size
        if tl > 4:
            order = tail[np.argsort(x[tail], kind="stable")]      # ascending by (x, sample index): `tail` is in index order
            exc = np.exp(xc)
            khat, sigma = gpdfit(np.exp(x[order]) - exc)
            if np.isfinite(khat):
                l1 = np.log1p(-(np.arange(1, tl + 1) - 0.5) / tl)
                q = -sigma * l1 if khat == 0.0 else sigma * np.expm1(-khat * l1) / khat
                x = x.copy()
                x[order] = np.minimum(np.log(q + exc), 0.0)
    w = x - _lse(x)
    lw[idx] = w
    return dict(n=float(n), tail_len=float(tl), pareto_k=float(khat), elpd_loo=float(_lse(v + w)), lppd=float(_lse(v) - np.log(n)),
                ess=float(1.0 / np.sum(np.exp(2.0 * w))), lw=lw)


def psis_row_mp(ll, dps=52):
    """The same in `dps`-digit mpmath (52 working digits, so that at least 40 survive the log(1 − b·y) of the fit) on the exact values of the float64 input; the results rounded to float64 once, at the end."""
    import mpmath as mp
    ll = np.asarray(ll, dtype=np.float64)
    idx = np.nonzero(np.isfinite(ll))[0]
    n = idx.size
    lw = np.full(ll.size, -np.inf)
    if n == 0:
        return dict(n=0.0, tail_len=np.nan, pareto_k=np.nan, elpd_loo=np.nan, lppd=np.nan, ess=np.nan, lw=lw)
    with mp.workdps(dps):
        # x_s = −ll_s − max(−ll) is exact here, so x orders as −ll does: selection and sorting are made on the float64 values (exactly)
        vf = ll[idx]
        v = [mp.mpf(float(a)) for a in vf]
        mx = -mp.mpf(float(vf.min()))
        x = [-a - mx for a in v]
        M = tail_len(n)
        khat, tl, order = mp.inf, 0, []
        if n > M:
            vc = float(np.sort(vf)[M])      # the (M+1)-th smallest ll = the (M+1)-th largest x
            xc, log_tiny = -mp.mpf(vc) - mx, mp.log(mp.mpf(float(np.finfo(np.float64).tiny)))
            if xc >= log_tiny:
                tail = np.nonzero(vf < vc)[0]
            else:
                xc = log_tiny
                tail = np.array([i for i in range(n) if x[i] > xc], dtype=np.int64)
            tl = len(tail)
            if tl > 4:
                order = [int(i) for i in tail[np.lexsort((tail, -vf[tail]))]]      # ascending by (x, sample index)
                exc = mp.exp(xc)
                y = [mp.exp(x[i]) - exc for i in order]
                m = 30 + math.isqrt(tl)
                bs = [(1 - mp.sqrt(mp.mpf(m) / (j - mp.mpf(1) / 2))) / (3 * y[int(math.floor(tl / 4.0 + 0.5)) - 1]) + 1 / y[tl - 1] for j in range(1, m + 1)]
                ks = [mp.fsum(mp.log(1 - b * t) for t in y) / tl for b in bs]      # log, not log1p: |b·y| >= 1e-12 costs 12 of the digits
                Ls = [tl * (mp.log(-b / k) - k - 1) for b, k in zip(bs, ks)]
                ws = [1 / mp.fsum(mp.exp(Ll - Lj) for Ll in Ls) for Lj in Ls]
                ws = [w if w >= 10 * mp.mpf(2) ** -52 else mp.mpf(0) for w in ws]
                sw = mp.fsum(ws)
                bb = mp.fsum(w / sw * b for w, b in zip(ws, bs))
                kk = mp.fsum(mp.log(1 - bb * t) for t in y) / tl
                sigma = -kk / bb
                khat = (tl * kk + 5) / (tl + 10)
                if mp.isfinite(khat):
                    for r, i in enumerate(order, start=1):
                        l1 = mp.log1p(-(mp.mpf(r) - mp.mpf(1) / 2) / tl)
                        q = -sigma * l1 if khat == 0 else sigma * mp.expm1(-khat * l1) / khat
                        x[i] = min(mp.log(q + exc), mp.mpf(0))
        # Closing sums with ONE exponential per entry: an entry that kept its x has ll + x = −mx exactly and exp(ll) = exp(−mx)/exp(x)
        smoothed = set(order) if (tl > 4 and mp.isfinite(khat)) else set()
        ex = [mp.exp(a) for a in x]
        lse = mp.log(mp.fsum(ex))
        w = [a - lse for a in x]
        emx = mp.exp(-mx)
        kept = n - len(smoothed)
        elpd = mp.log(kept * mp.exp(-mx - lse) + mp.fsum(mp.exp(v[i] + w[i]) for i in smoothed))
        lppd = mp.log(emx * mp.fsum(1 / ex[i] for i in range(n) if i not in smoothed) + mp.fsum(mp.exp(v[i]) for i in smoothed)) - mp.log(n)
        ess = mp.exp(2 * lse) / mp.fsum(e * e for e in ex)
        lw[idx] = [float(a) for a in w]
        return dict(n=float(n), tail_len=float(tl), pareto_k=float(khat), elpd_loo=float(elpd), lppd=float(lppd), ess=float(ess), lw=lw)


def psis_matrix(LL, row_fn=psis_row):
    """row_fn over the rows of LL [R, S]: dict of [R] arrays and lw [R, S]."""
    rows = [row_fn(r) for r in np.asarray(LL, dtype=np.float64)]
    out = {k: np.array([r[k] for r in rows]) for k in FIELDS}
    out["lw"] = np.array([r["lw"] for r in rows]).reshape(np.asarray(LL).shape)
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
PARAMS = ((0.3, 30.0), (1.0, 5.0))      # (c, ν): ll = −½(c·t_ν)² − 3


def student_rows(S, R, c, nu, seed):
    rng = np.random.default_rng(seed)
    return -0.5 * (c * rng.standard_t(nu, size=(R, S))) ** 2 - 3.0


# name -> (S, R, (c, ν), seed), smallest first: n <= M; tail <= 4; the first fitted tail; wave and block edges; more than one pass of the
# block over a row; a tail wider than the block (1040 at S = 120 001); R = 1, 7, 70
CASES = {}
for _S in (1, 4, 5, 24, 25, 64, 65, 130, 257, 1000, 4103):
    for _p, (_c, _nu) in enumerate(PARAMS):
        CASES[f"S{_S}_c{_c}_nu{int(_nu)}"] = (_S, 1, (_c, _nu), 1000 + 2 * _S + _p)
CASES["S130_R7"] = (130, 7, PARAMS[1], 7)
CASES["S130_R70"] = (130, 70, PARAMS[0], 70)
CASES["S20011"] = (20011, 1, PARAMS[0], 20011)
CASES["S120001_R2"] = (120001, 2, PARAMS[0], 120001)
RESTATEMENT_CASES = [k for k in CASES if CASES[k][0] <= 4103]      # the cases of the CPU test (and of the gap that sets the k̂ / ess bars)

_cache = {}


def case(name):
    """(LL [R, S], the 40-digit reference of it), computed once per process. Asserts what the generator promises: the spread of ll stays
    below 600 (no case reaches the underflow clamp) and every fitted k̂ lies in [−0.5, 5]."""
    if name not in _cache:
        S, R, (c, nu), seed = CASES[name]
        LL = student_rows(S, R, c, nu, seed)
        assert np.all(LL.max(axis=1) - LL.min(axis=1) < 600.0), name
        ref = psis_matrix(LL, psis_row_mp)
        k = ref["pareto_k"][np.isfinite(ref["pareto_k"])]
        assert np.all((k >= -0.5) & (k <= 5.0)), (name, k)
        _cache[name] = (LL, ref)
    return _cache[name]


def gaps(got, ref):
    """Largest gaps of `got` to `ref`: k̂ absolute; ess, elpd, lppd and lw relative to max(1, |ref|). n and tail_len must be equal."""
    assert np.array_equal(got["n"], ref["n"]), (got["n"], ref["n"])
    assert np.array_equal(got["tail_len"], ref["tail_len"], equal_nan=True), (got["tail_len"], ref["tail_len"])
    out = {}
    for k in ("pareto_k", "ess", "elpd_loo", "lppd", "lw"):
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        assert a.shape == b.shape, k
        same = (a == b) | (np.isnan(a) & np.isnan(b))      # ±Inf and NaN must match exactly
        assert np.all(same | (np.isfinite(a) & np.isfinite(b))), (k, a[~same][:5], b[~same][:5])
        d = np.abs(a[~same] - b[~same])
        if k != "pareto_k":
            d = d / np.maximum(1.0, np.abs(b[~same]))
        out[k] = float(d.max()) if d.size else 0.0
    return out
