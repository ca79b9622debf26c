"""
The shapes of the dense Gaussian-process RV tests (tests/test_gpd_reference.py on the CPU, tests/test_gpd.py on the device) and their reference values. A
plain module, not a conftest and not a test module. Every reference evaluation is made once a session (lru_cache) and shared; nobody writes into it.

The smallest shapes at which the kernels can still go wrong: n = 1, 2, 3; 63, 64, 65 (the wave edge); OCTO_DRAWS_GP_DENSE_LDS_ROWS and one more (the last
table in LDS and the first in the work array); 257 (more rows than threads). W = 1, 2, 3, 65, 130, the wide batches on n <= 9. Each kind alone, QP +
Matérn-3/2, four QP (H = 16). K = 0, 1, 2, 4. No jitter array, zeros, drawn. One planet of each accepted orbit kind, a planet without a mass, eight planets.
Ranges: a in [1, 8], ℓ in [2, 40], P in [5, 60], r in [0.3, 2], σ in [0.5, 3], s in [0.1, 2], epochs about 4 days apart on average; cond(K) <= 1e6 on every
case is a condition on these inputs (tests/test_gpd_reference.py). Every drawn walker is valid.

The reference of a case with n <= MP_ROWS is the mpmath one; the longer tables are judged against the NumPy restatement, which the CPU suite holds to
mpmath at 1e-10 on every case it can afford.
"""
import functools

import numpy as np

import gp_cases as gc
import gp_reference as gref
import gpd_reference as dref

V, RV, KEP = gref.VISUAL_KEP, gref.RADVEL, gref.KEP
SE, M32, M52, PER, QP = dref.SE, dref.MATERN32, dref.MATERN52, dref.PERIODIC, dref.QUASIPERIODIC
L = dref.LDS_ROWS
MP_ROWS = 17
# name: (W, n, planets [(orbit_kind, has_mass)], K, jitter: None = no array, 0.0 = zeros, "draw", terms)
CASES = {
    "one":          (1, 1, [(RV, 1)], 0, None, [SE]),
    "two":          (2, 2, [(KEP, 1)], 1, 0.0, [M32]),
    "three":        (3, 3, [(V, 1)], 2, "draw", [M52]),
    "per_wide":     (65, 9, [(RV, 1)], 4, "draw", [PER]),
    "qp_wide":      (130, 7, [(RV, 1), (V, 0)], 1, "draw", [QP]),
    "qp_m32":       (2, 17, [(RV, 1), (KEP, 1), (V, 0), (V, 1)], 2, "draw", [QP, M32]),
    "four_qp":      (1, 16, [(RV, 1)] * 8, 4, "draw", [QP] * 4),
    "n63":          (1, 63, [(RV, 1)], 1, "draw", [QP]),
    "n64":          (2, 64, [(KEP, 1)], 0, "draw", [SE]),
    "n65":          (2, 65, [(RV, 1)], 2, 0.0, [QP, M32]),
    "lds_last":     (2, L, [(RV, 1)], 1, "draw", [QP]),
    "global_first": (2, L + 1, [(RV, 1)], 1, "draw", [QP]),
    "n257":         (1, 257, [(RV, 1)], 1, "draw", [M52, PER]),
}


def draw_hyper(rng, terms, W):
    h = []
    for kind in terms:
        a, ell, P, r = rng.uniform(1, 8, W), rng.uniform(2, 40, W), rng.uniform(5, 60, W), rng.uniform(0.3, 2, W)
        h += {SE: [a, ell], M32: [a, ell], M52: [a, ell], PER: [a, P, r], QP: [a, ell, P, r]}[kind]
    return np.array(h)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(tab, terms, planets, elems, hyper [H, W], beta [K, W], jitter [W] or None) of a case, drawn from its own seed"""
    W, n, planets, K, jit, terms = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20020)
    tab = gc.draw_table(rng, n, K, False)
    return dict(tab=tab, terms=list(terms), planets=planets, elems=gc.draw_elements(rng, planets, W), hyper=draw_hyper(rng, terms, W),
                beta=rng.normal(size=(K, W)) * 2.0, jitter=None if jit is None else (np.zeros(W) if jit == 0.0 else rng.uniform(0.1, 2.0, W)))


@functools.lru_cache(maxsize=None)
def numpy_reference(name):
    x = inputs(name)
    return dref.numpy_dense(x["tab"], x["terms"], x["planets"], x["elems"], x["hyper"], x["beta"], x["jitter"], grad=True)


@functools.lru_cache(maxsize=None)
def mp_reference(name):
    x = inputs(name)
    return dref.dense(x["tab"], x["terms"], x["planets"], x["elems"], x["hyper"], x["beta"], x["jitter"], grad=True)


def reference(name):
    """what the device is judged against: mpmath up to MP_ROWS rows, the NumPy restatement beyond"""
    return mp_reference(name) if CASES[name][1] <= MP_ROWS else numpy_reference(name)
