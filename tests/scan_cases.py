"""
The shapes of the along-scan astrometry tests (tests/test_scan_reference.py on the CPU, tests/test_scan.py on the device) and their restated values. A
plain module, not a conftest and not a test module. Every restated evaluation is made once a session (lru_cache) and shared; nobody writes into it.

The smallest shapes at which the kernels can still go wrong, R = OCTO_DRAWS_SCAN_ROWS = 8 the rows of a task: one row, fewer rows than a task, R − 1, R,
R + 1 and 3R + 5 (four tasks, the last partial); one lane, one full wave, one wave and a lane, two waves and two lanes; one, two, five and eight
planets, a ThieleInnesOrbit, a RadialVelocityOrbit (contributes nothing) and a planet without a mass (contributes nothing) among them; K = 0, 2, 5, 6;
no jitter array, s = 0 and s > 0. scan_set refuses a table whose design columns are rank deficient, so no case has n < K. All drawn walkers are valid
by construction: e in [0, 0.9], a, M, plx > 0, mass in [1, 80] M_jup.
"""
import functools

import numpy as np

import scan_reference as sref

R = 8
V, RV, TI = sref.VISUAL_KEP, sref.RADVEL, sref.THIELE_INNES
# name: (W, n, planets [(orbit_kind, has_mass)], K, jitter: None = no array, 0.0 = zeros, "draw" = positive)
CASES = {
    "one":        (1, 1, [(V, 1)], 0, None),
    "two_rows":   (64, 2, [(TI, 1), (V, 1)], 2, 0.0),
    "r_minus_1":  (65, R - 1, [(V, 1)], 5, "draw"),
    "r":          (130, R, [(V, 1)], 6, "draw"),
    "r_plus_1":   (65, R + 1, [(V, 1), (RV, 1), (V, 0), (TI, 1), (V, 1)], 5, "draw"),
    "four_tasks": (1, 3 * R + 5, [(V, 1)] * 8, 2, "draw"),
}


def draw_elements(rng, planets, W, t0=48500.0):
    """elems [P·9, W] of valid walkers; a ThieleInnesOrbit planet carries A, B, F, G [mas] of a drawn Campbell orbit"""
    rows = []
    for kind, _ in planets:
        a, e = rng.uniform(1.0, 12.0, W), rng.uniform(0.0, 0.9, W)
        inc, om, Om = rng.uniform(0.05, np.pi - 0.05, W), rng.uniform(0, 2 * np.pi, W), rng.uniform(0, 2 * np.pi, W)
        M, plx, mass = rng.uniform(0.6, 1.8, W), rng.uniform(15.0, 80.0, W), rng.uniform(1.0, 80.0, W)
        tp = t0 - rng.uniform(0, 1, W) * 365.2568983840419 * np.sqrt(a ** 3 / M)
        el = np.stack([a, e, inc, om, Om, tp, M, plx, mass])
        if kind == TI:
            al = a * plx
            sO, cO, sw, cw, ci = np.sin(Om), np.cos(Om), np.sin(om), np.cos(om), np.cos(inc)
            el[sref.TI_A] = al * (cO * cw - sO * sw * ci)
            el[sref.TI_B] = al * (sO * cw + cO * sw * ci)
            el[sref.TI_F] = al * (-cO * sw - sO * cw * ci)
            el[sref.TI_G] = al * (-sO * sw + cO * cw * ci)
        rows.append(el)
    return np.concatenate(rows)


def draw_table(rng, n, K):
    """a Hipparcos-like table: epochs over three years, random scan angles, the five astrometric columns and a sixth, y of the size of σ"""
    t = np.sort(rng.uniform(47900.0, 49050.0, n))
    psi = rng.uniform(0, 2 * np.pi, n)
    u, v = np.cos(psi), np.sin(psi)
    dt = (t - 48348.5625) / 365.25
    cols = np.stack([u, v, rng.uniform(-0.7, 0.7, n), u * dt, v * dt, rng.normal(size=n)])[:K]
    sigma = rng.uniform(0.5, 3.0, n)
    y = rng.normal(size=n) * 2.0
    return sref.table(t, u, v, y, sigma, cols)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(tab, planets, elems, beta [K, W], jitter [W] or None) of a case, drawn from its own seed"""
    W, n, planets, K, jit = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20260)
    tab = draw_table(rng, n, K)
    elems = draw_elements(rng, planets, W)
    beta = rng.normal(size=(K, W)) * 2.0
    jitter = None if jit is None else (np.zeros(W) if jit == 0.0 else rng.uniform(0.1, 2.0, W))
    return dict(tab=tab, planets=planets, elems=elems, beta=beta, jitter=jitter)


@functools.lru_cache(maxsize=None)
def restated(name, mode):
    """scan_reference.evaluate of a case in `mode`, with the gradient"""
    x = inputs(name)
    return sref.evaluate(x["tab"], x["planets"], x["elems"], x["beta"], x["jitter"], mode=mode, grad=True)
