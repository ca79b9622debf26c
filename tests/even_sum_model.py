"""Float64 restatement of the two ways k_main sums Σ_i Mb_i·(t_i − tp) over one wave's chunk of an EXACTLY even table (t_i = t_last − (n − 1 − i)·h, every
difference exact), lane = walker:

  parent_sum   the row's own FMA, g = fma(Mb_i, t_i − tp, g)                                   (octo_kernels.h: astrom_row, g[GT])
  prefix_sum   GM += Mb_i; GG += GM in the row, and behind the loop fma(−h, GG, ((t_last − tp) + h)·GM)   (astrom_row<…, WEVEN = 2>, even_gt_finish)
  reference    the same sum in long double

and their errors relative to Σ_i |Mb_i·(t_i − tp)|. The FMA is restated with error-free transformations (Veltkamp/Dekker product, Knuth sum): the product is exact
and the result is the float64 nearest to product + addend up to a second rounding of 2^-53 of it. No GPU, no device code: the rounding of the formula only."""
import numpy as np

_SPLIT = 134217729.0      # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ah = a * _SPLIT; ah = ah - (ah - a); al = a - ah
    bh = b * _SPLIT; bh = bh - (bh - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    p, e = _two_prod(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    s, es = _two_sum(p, np.asarray(c, dtype=np.float64))
    return s + (es + e)


def epochs(t_last, h, n):
    """the chunk's epochs; the caller picks t_last and h so that every product k·h and every difference is exact (asserted)"""
    t = t_last - h * np.arange(n - 1, -1, -1, dtype=np.float64)
    if n > 1:
        assert np.all(np.diff(t) == h)
        assert np.all(np.diff(t.astype(np.longdouble)) == np.longdouble(h))
    return t


def parent_sum(mb, t, tp):
    """mb: [lanes, n]; t: [n]; tp: [lanes]"""
    g = np.zeros(mb.shape[0])
    for i in range(t.size):
        g = fma(mb[:, i], t[i] - tp, g)
    return g


def prefix_sum(mb, t, tp):
    gm = np.zeros(mb.shape[0]); gg = np.zeros(mb.shape[0])
    for i in range(t.size):
        gm = gm + mb[:, i]
        gg = gg + gm
    h = t[-1] - t[-2] if t.size > 1 else 0.0      # the device takes the step from the chunk's last two records; a chunk of one row has none
    return fma(-h, gg, ((t[-1] - tp) + h) * gm)


MIN_ROWS = 5      # WARM_NEWTON_DEPTH + 1 (octo_device.h): the shortest chunk on which the history can fill and a Newton-only row can occur


def device_sum(mb, t, tp):
    """what k_main does on an exactly even task: the prefix form on chunks of at least MIN_ROWS rows, the parent's rows on shorter ones. (A shorter chunk has no
    Newton-only row to make cheaper, and on a chunk of TWO rows the prefix form is badly conditioned where the adjoints cancel and tp lies between the epochs: GM and GG
    round relative to |Mb|·h, the sum itself can be far smaller — 50 to 400 x the parent's error over 4 096 random lanes, against 12 x at three rows and 4-7 x from four on.)"""
    return prefix_sum(mb, t, tp) if t.size >= MIN_ROWS else parent_sum(mb, t, tp)


def reference(mb, t, tp):
    """(Σ Mb·dt, Σ |Mb·dt|) in long double"""
    dt = t.astype(np.longdouble)[None, :] - tp.astype(np.longdouble)[:, None]
    pr = mb.astype(np.longdouble) * dt
    return pr.sum(axis=1), np.abs(pr).sum(axis=1)


def errors(mb, t, tp, form=device_sum):
    """(worst error of `form`, worst error of the parent's form) over the lanes, relative to Σ |Mb·dt|"""
    ref, scale = reference(mb, t, tp)
    scale = np.maximum(scale, np.longdouble(1e-300))
    e_new = np.abs(form(mb, t, tp).astype(np.longdouble) - ref) / scale
    e_par = np.abs(parent_sum(mb, t, tp).astype(np.longdouble) - ref) / scale
    return float(e_new.max()), float(e_par.max())


def adjoints(kind, lanes, n, rng):
    """Mb of one chunk. smooth: one sign, slowly varying (a slow walker's Ē/D); sign: a smooth curve that changes sign inside the chunk (a sky-plane adjoint through a
    turning point); random: normal draws."""
    x = np.linspace(0.0, 1.0, n)[None, :]
    a = rng.uniform(0.5, 2.0, (lanes, 1)); b = rng.uniform(-1.0, 1.0, (lanes, 1)); c = rng.uniform(0.0, 1.0, (lanes, 1))
    if kind == "smooth":
        return a * (1.0 + 0.3 * b * x + 0.1 * np.sin(3.0 * x + 6.0 * c))
    if kind == "sign":
        return a * np.sin(2.0 * np.pi * (x * rng.uniform(0.5, 2.0, (lanes, 1)) + c))
    if kind == "random":
        return rng.normal(0.0, 1.0, (lanes, n))
    raise ValueError(kind)
