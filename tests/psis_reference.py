"""Reference side of the PSIS tests (a helper, not a test; tools/psis_bench.py uses it too): the algorithm of include/octofitter_hip_psis.h
restated twice — psis_row in float64 NumPy (stable argsorts) and psis_row_mp in 40-digit mpmath, with psis_row_hybrid for rows too long for
the latter — the Zhang–Stephens fit on its own (gpdfit), the case generator of tests/test_psis.py, the edge rows (EDGE_ROWS, with gather_pass:
where the kernel's select gathers) and the comparison at its bars."""
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


def psis_row(ll, dM=0):
    """One row in float64: dict(n, tail_len, pareto_k, elpd_loo, lppd, ess, lw [S]). dM moves the cut-off by that many entries (M + dM): what a
    select that is off by one would compute (cut_sensitivity)."""
    ll = np.asarray(ll, dtype=np.float64)
    idx = np.nonzero(np.isfinite(ll))[0]
    v = ll[idx]
    n = v.size
    lw = np.full(ll.size, -np.inf)
    if n == 0:
        return dict(n=0.0, tail_len=np.nan, pareto_k=np.nan, elpd_loo=np.nan, lppd=np.nan, ess=np.nan, lw=lw)
    x = -v - np.max(-v)
    M = tail_len(n) + dM
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


def _mp_tail(mp, xt, xc):
    """The fit and the smoothing of one tail in mpmath: xt the tail's x ascending (mpf), xc the cut-off. Returns (k̂, the smoothed x in the
    same order, or None where k̂ is not finite)."""
    tl = len(xt)
    exc = mp.exp(xc)
    y = [mp.exp(a) - exc for a in xt]
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
    if not mp.isfinite(khat):
        return khat, None
    xs = []
    for r in range(1, tl + 1):
        l1 = mp.log1p(-(mp.mpf(r) - mp.mpf(1) / 2) / tl)
        q = -sigma * l1 if khat == 0 else sigma * mp.expm1(-khat * l1) / khat
        xs.append(min(mp.log(q + exc), mp.mpf(0)))
    return khat, xs


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
        khat, tl, smoothed = mp.inf, 0, set()
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
                khat, xs = _mp_tail(mp, [x[i] for i in order], xc)
                if xs is not None:
                    smoothed = set(order)
                    for i, a in zip(order, xs):
                        x[i] = a
        # Closing sums with ONE exponential per entry: an entry that kept its x has ll + x = −mx exactly and exp(ll) = exp(−mx)/exp(x)
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


def _fsum_mp(mp, t):
    """Σ t of a long-double array as an mpf: the terms ascending, each split into a high and a low float64 half, the halves added with
    math.fsum (exact up to its one rounding), and the residual of that rounding added the same way."""
    t = np.sort(t)
    hi = t.astype(np.float64)
    halves = np.concatenate([hi, (t - hi).astype(np.float64)]).tolist()
    s1 = math.fsum(halves)
    return mp.mpf(s1) + mp.mpf(math.fsum(halves + [-s1]))


def psis_row_hybrid(ll, dps=52):
    """psis_row_mp for rows too long for it (about 55 µs an entry there): the selection, the fit and the smoothed tail (<= 4096 entries) in
    `dps`-digit mpmath exactly as psis_row_mp has them; the three sums over the entries that keep their x — Σ exp x, Σ exp 2x, Σ 1/exp x —
    and those entries' log-weights x − lse in np.longdouble (64-bit mantissa: each term within 2⁻⁶³, the sums by _fsum_mp). It is
    psis_row_mp itself where long double is no wider than float64, and for a row whose spread reaches 700 (the float64 halves of 1/exp x
    would overflow, and the cut-off could be the clamp)."""
    import mpmath as mp
    ll = np.asarray(ll, dtype=np.float64)
    idx = np.nonzero(np.isfinite(ll))[0]
    n = idx.size
    if not np.finfo(np.longdouble).eps < 1e-18 or n == 0 or np.ptp(ll[idx]) >= 700.0:
        return psis_row_mp(ll, dps)
    assert np.finfo(np.longdouble).eps < 1e-18
    lw = np.full(ll.size, -np.inf)
    with mp.workdps(dps):
        vf = ll[idx]
        vmin = float(vf.min())
        mx = -mp.mpf(vmin)
        xl = -(vf.astype(np.longdouble) - np.longdouble(vmin))
        M = tail_len(n)
        khat, tl, order, xs = mp.inf, 0, np.zeros(0, dtype=np.int64), None
        if n > M:
            vc = float(np.sort(vf)[M])
            xc = -mp.mpf(vc) - mx      # above log(DBL_MIN): the spread is below 700
            tail = np.nonzero(vf < vc)[0]
            tl = len(tail)
            if tl > 4:
                order = tail[np.lexsort((tail, -vf[tail]))]      # ascending by (x, sample index)
                khat, xs = _mp_tail(mp, [-mp.mpf(float(vf[i])) - mx for i in order], xc)
        bulk = np.ones(n, dtype=bool)
        if xs is None:
            order, xs = order[:0], []
        bulk[order] = False
        e = np.exp(xl[bulk])
        lse = mp.log(_fsum_mp(mp, e) + mp.fsum(mp.exp(a) for a in xs))
        vt = [mp.mpf(float(vf[i])) for i in order]
        wt = [a - lse for a in xs]
        elpd = mp.log(int(bulk.sum()) * mp.exp(-mx - lse) + mp.fsum(mp.exp(a + b) for a, b in zip(vt, wt)))
        lppd = mp.log(mp.exp(-mx) * _fsum_mp(mp, 1 / e) + mp.fsum(mp.exp(a) for a in vt)) - mp.log(n)
        ess = mp.exp(2 * lse) / (_fsum_mp(mp, e * e) + mp.fsum(mp.exp(2 * a) for a in xs))
        lse_hi = float(lse)
        w = np.empty(n)
        w[bulk] = (xl[bulk] - (np.longdouble(lse_hi) + np.longdouble(float(lse - lse_hi)))).astype(np.float64)
        w[order] = [float(a) for a in wt]
        lw[idx] = w
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


# ---- the edge rows: routes of the kernel's select and sort that no row of CASES takes -------------------------------------------------------
def gather_pass(row):
    """Where the kernel's radix select gathers its candidates into LDS, stated on the CPU with u = bits(v − min v) over the finite entries:
    "no select" for n <= M; 0 for n <= MAX_TAIL; else the first pass p in 1 … 7 at whose top at most MAX_TAIL entries share the top 8p bits
    with the (M+1)-th smallest u; "never" where even the top 56 bits are shared by more."""
    row = np.asarray(row, dtype=np.float64)
    v = row[np.isfinite(row)]
    n = v.size
    M = tail_len(n)
    if n <= M:
        return "no select"
    if n <= MAX_TAIL:
        return 0
    u = (v - v.min()).view(np.uint64)
    uc = np.partition(u, M)[M]
    for p in range(1, 8):
        sh = np.uint64(64 - 8 * p)
        if np.count_nonzero((u >> sh) == (uc >> sh)) <= MAX_TAIL:
            return p
    return "never"


def _one_low(seed, S, draw, low):
    """draw(rng, S) with one entry, at a position drawn after it, set to `low`."""
    rng = np.random.default_rng(seed)
    row = draw(rng, S)
    row[rng.integers(S)] = low
    return row


def _grid_row(seed, S, lsb):
    """−3 + k·2^lsb with S distinct integers k below 2¹⁶ and one entry set to −100: every v − min v is exact."""
    return _one_low(seed, S, lambda rng, n: -3.0 + rng.choice(2 ** 16, n, replace=False) * 2.0 ** lsb, -100.0)


def _tieblock(seed):
    rng = np.random.default_rng(seed)
    row = np.concatenate([-5.0 - 0.3 * rng.exponential(1.0, 100), np.full(6000, -5.0), rng.uniform(-4.0, -1.0, 5900)])
    return row[rng.permutation(row.size)]


def _near_tieblock(seed):
    """S = 12 000, M = 329: the minimum −6.5, 328 values in (−6.5, −4.6], then a block of 6 000 distinct values −4.5 + k·2⁻⁵⁰ (k < 2¹⁵: exact, as
    is every v − min v of the block) whose smallest is the cut, then 5 671 values above −4. The block shares the top 48 bits of u, so the select
    walks the row seven times; the tail lies at least 0.1 from the cut, so the fit is as well conditioned as a Student row's."""
    rng = np.random.default_rng(seed)
    row = np.concatenate([[-6.5], -4.6 - 0.3 * np.minimum(rng.exponential(1.0, 328), 6.0), -4.5 + rng.choice(2 ** 15, 6000, replace=False) * 2.0 ** -50,
                          rng.uniform(-4.0, -1.0, 5671)])
    return row[rng.permutation(row.size)]


def _two_scales(seed):
    """3 000 entries within 2 of the minimum (an exponential lower tail) and 17 000 more than 2 above it: the top byte of u splits them."""
    rng = np.random.default_rng(seed)
    row = np.concatenate([-6.5 - 0.2 * rng.exponential(1.0, 3000), rng.uniform(-5.5, -1.0, 17000)])
    return row[rng.permutation(row.size)]


def _scattered(seed, S, n_finite, student_seed, nan_every=0):
    """A row of −Inf with n_finite Student entries at random positions; NaN at every nan_every-th position, over whatever was there."""
    rng = np.random.default_rng(seed)
    row = np.full(S, -np.inf)
    row[rng.choice(S, n_finite, replace=False)] = student_rows(n_finite, 1, 0.3, 30.0, student_seed)[0]
    if nan_every:
        row[::nan_every] = np.nan
    return row


def _dup10():
    return np.repeat(student_rows(2000, 1, 0.3, 30.0, 9)[0], 10)


def _s20011():
    return student_rows(20011, 1, 0.3, 30.0, 20011)[0]


# name -> dict(make: () -> row [S]; ref: "mp" (psis_row_mp) or "hybrid" (psis_row_hybrid, S > 120 001); bars: "fixture" (the bars of the cases)
# or "row" (edge_bars: the fit is ill-conditioned by construction); gather: gather_pass of the row; tail_len: the reference's; k: the window
# of the reference's k̂, where it is pinned). Everything listed is asserted by edge_case on the CPU, before a device test sees the row.
EDGE_ROWS = {}
# sort edges: tails of 8, 64, 256 (no padding), 257, 1025 (most padding), 2048 (none at P = 2048), 2049 (P = 4096), 4096 (MAX_TAIL, m = MAX_GRID)
# (S, tail_len, gather_pass per PARAMS used). PARAMS[1] is left out where its row breaks what every row must promise: k̂ = 5.50 at S = 7282 and
# 6.60 at S = 116 509 (above 5), and above S = 116 509 its spread nears the clamp.
for _S, _tl, _gs in ((36, 8, (0, 0)), (40, 8, (0, 0)), (455, 64, (0, 0)), (7281, 256, (1, 2)), (7282, 257, (2,)), (116509, 1025, (2,)),
                     (466033, 2048, (2,)), (466034, 2049, (2,)), (1864135, 4096, (3,))):
    for _p, _g in enumerate(_gs):
        _c, _nu = PARAMS[_p]
        EDGE_ROWS[f"sort_S{_S}_c{_c}_nu{int(_nu)}"] = dict(make=lambda S=_S, c=_c, nu=_nu, p=_p: student_rows(S, 1, c, nu, 1000 + 2 * S + p)[0],
                                                          ref="mp" if _S <= 120001 else "hybrid", bars="fixture", gather=_g, tail_len=_tl)
LIMIT_ROW = "sort_S1864135_c0.3_nu30"
EDGE_ROWS.update({
    # select routes
    "gather1": dict(make=lambda: _two_scales(1), ref="mp", bars="row", gather=1, tail_len=425),
    "gather3": dict(make=lambda: _one_low(3, 20000, lambda rng, n: rng.normal(-3.0, 0.01, n), -100.0), ref="mp", bars="row", gather=3, tail_len=425),
    "gather4": dict(make=lambda: _one_low(4, 20000, lambda rng, n: rng.normal(-3.0, 0.03, n), -500.0), ref="mp", bars="row", gather=4, tail_len=425),
    "gather5": dict(make=lambda: _grid_row(5, 20000, -28), ref="mp", bars="row", gather=5, tail_len=425),
    "gather6": dict(make=lambda: _grid_row(6, 20000, -36), ref="mp", bars="row", gather=6, tail_len=425),
    # (−3 + k·2⁻⁴⁴ also gathers at pass 7, but there the restatement's own k̂ gap is 4.5e-7: 100 × it is above K_BAR_CAP)
    "gather7": dict(make=lambda: _near_tieblock(7), ref="mp", bars="row", gather=7, tail_len=329),
    "never_tieblock": dict(make=lambda: _tieblock(12), ref="mp", bars="fixture", gather="never", tail_len=100),
    "const_4096": dict(make=lambda: np.full(4096, -2.5), ref="mp", bars="fixture", gather=0, tail_len=0),
    "const_4097": dict(make=lambda: np.full(4097, -2.5), ref="mp", bars="fixture", gather="never", tail_len=0),
    "const_5000": dict(make=lambda: np.full(5000, -2.5), ref="mp", bars="fixture", gather="never", tail_len=0),
    # ties as a sampler produces them: every value ten times; the minimum's key equals the sort's padding key
    "dup10": dict(make=_dup10, ref="mp", bars="fixture", gather=2, tail_len=420),
    "dup10_perm": dict(make=lambda: _dup10()[np.random.default_rng(10).permutation(20000)], ref="mp", bars="fixture", gather=2, tail_len=420),
    # few finite entries in a long row
    "sparse": dict(make=lambda: _scattered(100, 100000, 3000, 4, nan_every=1001), ref="mp", bars="fixture", gather=0, tail_len=None),
    "finite_4096": dict(make=lambda: _scattered(4096, 20000, 4096, 4096), ref="mp", bars="fixture", gather=0, tail_len=192),
    "finite_4097": dict(make=lambda: _scattered(4097, 20000, 4097, 4097), ref="mp", bars="fixture", gather=1, tail_len=193),
    # values away from 0
    "offset_-1e6": dict(make=lambda: _s20011() - 1e6, ref="mp", bars="fixture", gather=2, tail_len=425),
    "offset_+20": dict(make=lambda: _s20011() + 20.0, ref="mp", bars="fixture", gather=2, tail_len=425),
})
ROUTE_ROWS = [k for k, e in EDGE_ROWS.items() if e["bars"] == "row"]

_edge_cache = {}


def edge_case(name):
    """(LL [1, S], its reference, gather_pass of the row), computed once per process, after asserting on the CPU what EDGE_ROWS lists for
    the row and what case() asserts: the route, the tail length (tail_len(n) where no tie at the cut is listed), spread < 600, k̂ in
    [−0.5, 5] where fitted — and that rounding v − min v makes no tie the exact values do not have, so that the reference (which selects on
    the exact values) and the device (which selects on u) choose the same tail."""
    if name not in _edge_cache:
        e = EDGE_ROWS[name]
        row = np.ascontiguousarray(e["make"](), dtype=np.float64)
        v = row[np.isfinite(row)]
        assert v.max() - v.min() < 600.0, name
        assert np.unique(v - v.min()).size == np.unique(v).size, name
        g = gather_pass(row)
        assert g == e["gather"], (name, g)
        ref = psis_matrix(row[None, :], psis_row_mp if e["ref"] == "mp" else psis_row_hybrid)
        want = tail_len(v.size) if e["tail_len"] is None else e["tail_len"]
        assert ref["n"][0] == v.size and ref["tail_len"][0] == want, (name, ref["n"], ref["tail_len"], want)
        if not name.startswith(("never", "const", "dup10")):
            assert want == tail_len(v.size), (name, want)
        k = ref["pareto_k"][0]
        assert (want <= 4 and k == np.inf) or -0.5 <= k <= 5.0, (name, k)
        _edge_cache[name] = (row[None, :], ref, g)
    return _edge_cache[name]


def restatement_bars():
    """The bars of the cases (tests/test_psis.py's `bars` fixture restated for the CPU suite and tools/psis_bench.py): k̂ and ess at 100 × the
    restatement's largest gap to the 40-digit reference over CASES, the rest at 1e-11."""
    worst = dict(pareto_k=0.0, ess=0.0)
    for name in CASES:
        LL, ref = case(name)
        g = gaps(psis_matrix(LL), ref)
        worst = {k: max(v, g[k]) for k, v in worst.items()}
    return dict(pareto_k=100.0 * worst["pareto_k"], ess=100.0 * worst["ess"], elpd_loo=1e-11, lppd=1e-11, lw=1e-11)


K_BAR_CAP = 1e-5


def edge_bars(name, base):
    """The bars of one edge row given the bars of the cases, `base`. A "fixture" row keeps them. A "row" row has its tail within 1e-2 … 1e-8 of
    the cut-off, so y = exp(x) − exp(x_c) cancels and the fit is ill-conditioned by construction: there a field's bar is the larger of base
    and 100 × the float64 restatement's own gap to the reference ON THAT ROW, the project's rule, with k̂'s capped at K_BAR_CAP. Nothing of
    the device enters. Returns (bars, the restatement's gaps)."""
    LL, ref, _ = edge_case(name)
    g = gaps(psis_matrix(LL), ref)
    if EDGE_ROWS[name]["bars"] != "row":
        return dict(base), g
    b = {k: max(base[k], 100.0 * g[k]) for k in base}
    b["pareto_k"] = min(b["pareto_k"], K_BAR_CAP)
    return b, g


def cut_sensitivity(name):
    """How far k̂ moves when the cut-off moves by one entry, in the float64 restatement: min over M − 1 and M + 1 of |k̂ − k̂(M)|. A bar a tenth
    of this cannot pass a tail that is wrong by one entry."""
    row = edge_case(name)[0][0]
    k0 = psis_row(row)["pareto_k"]
    return min(abs(psis_row(row, dM=d)["pareto_k"] - k0) for d in (-1, 1))
