"""
The shapes of the Gaussian-process RV tests (tests/test_gp_reference.py on the CPU, tests/test_gp.py on the device) and their reference values. A plain
module, not a conftest and not a test module. Every reference evaluation is made once a session (lru_cache) and shared; nobody writes into it.

The smallest shapes at which the kernels can still go wrong, G = OCTO_DRAWS_GP_SEGMENT the rows between two checkpoints: n = 1, 2, G − 1, G, G + 1 and
3G + 5 (four segments, the last partial; seven row tasks); W = 1, 64, 65, 130; K = 0, 1, 2, 4; no jitter array, zeros, drawn; one REAL, one COMPLEX, an
SHO above ½, below ½ and with the lanes of one wave on both sides, four COMPLEX (R = 8) and REAL + COMPLEX + SHO (R = 5, padded to 8); one planet,
{RadialVelocityOrbit, KepOrbit, a planet without a mass, Visual{KepOrbit}} and eight planets; one table with a gap so long that φ is exactly 0. The dense
reference is kept affordable: wide batches on n <= 9, long tables on W <= 2. Ranges: a in [1, 25], c in [0.01, 0.5]/d, d in [0.05, 1], b in [0, ac/d],
S0 in [1, 30], Q in [0.05, 0.45] ∪ [0.6, 20], ω0 in [0.05, 1], σ in [0.5, 3], s in [0.1, 2]. Every drawn walker is valid.
"""
import functools

import numpy as np

import gp_reference as gref

G = gref.SEGMENT
V, RV, KEP = gref.VISUAL_KEP, gref.RADVEL, gref.KEP
RE, CO, SHO = gref.REAL, gref.COMPLEX, gref.SHO
# name: (W, n, planets [(orbit_kind, has_mass)], K, jitter: None = no array, 0.0 = zeros, "draw", terms, Q side of an SHO: "over", "under", "both", gap)
CASES = {
    "one":         (1, 1, [(RV, 1)], 0, None, [RE], None, False),
    "two_rows":    (64, 2, [(RV, 1)], 1, 0.0, [CO], None, False),
    "sho_over":    (65, 9, [(V, 1)], 2, "draw", [SHO], "over", False),
    "sho_under":   (64, 7, [(KEP, 1)], 1, "draw", [SHO], "under", False),
    "sho_both":    (130, 8, [(RV, 1)], 4, "draw", [SHO], "both", False),
    "g_minus_1":   (2, G - 1, [(RV, 1), (KEP, 1), (V, 0), (V, 1)], 2, "draw", [RE, CO, SHO], "both", False),
    "g":           (2, G, [(RV, 1)], 1, "draw", [CO, CO, CO, CO], None, False),
    "g_plus_1":    (2, G + 1, [(RV, 1)], 2, "draw", [SHO], "both", True),
    "four_segs":   (1, 3 * G + 5, [(RV, 1)] * 8, 4, "draw", [RE, CO, SHO], "under", False),
}


def draw_elements(rng, planets, W, t0=55000.0):
    rows = []
    for _kind, _ in planets:
        a, e = rng.uniform(0.3, 4.0, W), rng.uniform(0.0, 0.8, W)
        inc, om, Om = rng.uniform(0.3, np.pi - 0.3, W), rng.uniform(0, 2 * np.pi, W), rng.uniform(0, 2 * np.pi, W)
        M, plx, mass = rng.uniform(0.6, 1.8, W), rng.uniform(15.0, 80.0, W), rng.uniform(0.3, 10.0, W)
        tp = t0 - rng.uniform(0, 1, W) * 365.2568983840419 * np.sqrt(a ** 3 / M)
        rows.append(np.stack([a, e, inc, om, Om, tp, M, plx, mass]))
    return np.concatenate(rows)


def draw_hyper(rng, terms, W, side):
    h = []
    for kind in terms:
        if kind == RE:
            h += [rng.uniform(1, 25, W), rng.uniform(0.01, 0.5, W)]
        elif kind == CO:
            a, c, d = rng.uniform(1, 25, W), rng.uniform(0.01, 0.5, W), rng.uniform(0.05, 1, W)
            h += [a, rng.uniform(0, 1, W) * a * c / d, c, d]
        else:
            lo, hi = rng.uniform(0.05, 0.45, W), rng.uniform(0.6, 20, W)
            Q = hi if side == "over" else (lo if side == "under" else np.where(np.arange(W) % 2 == 0, hi, lo))
            h += [rng.uniform(1, 30, W), Q, rng.uniform(0.05, 1, W)]
    return np.array(h)


def draw_table(rng, n, K, gap):
    t = np.sort(rng.uniform(55000.0, 55000.0 + 4.0 * max(n, 2), n))
    if gap and n > 3:
        t[n // 2:] += 2.0e5      # c >= 0.01/d: φ = exp(−2000 …) is exactly 0
    dt = (t - t[0]) / 100.0
    cols = np.stack([np.ones(n), dt, dt * dt, rng.normal(size=n)])[:K]
    return gref.table(t, rng.normal(size=n) * 8.0, rng.uniform(0.5, 3.0, n), cols)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(tab, terms, planets, elems, hyper [H, W], beta [K, W], jitter [W] or None) of a case, drawn from its own seed"""
    W, n, planets, K, jit, terms, side, gap = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 19019)
    tab = draw_table(rng, n, K, gap)
    return dict(tab=tab, terms=list(terms), planets=planets, elems=draw_elements(rng, planets, W), hyper=draw_hyper(rng, terms, W, side),
                beta=rng.normal(size=(K, W)) * 2.0, jitter=None if jit is None else (np.zeros(W) if jit == 0.0 else rng.uniform(0.1, 2.0, W)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """gp_reference.dense of a case, with the gradient"""
    x = inputs(name)
    return gref.dense(x["tab"], x["terms"], x["planets"], x["elems"], x["hyper"], x["beta"], x["jitter"], grad=True)
