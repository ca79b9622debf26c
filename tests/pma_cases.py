"""
The shapes of the catalogue proper-motion anomaly tests (tests/test_pma_reference.py on the CPU, tests/test_pma.py on the device) and their restated
values. A plain module, not a conftest and not a test module. Every restated evaluation is made once a session (lru_cache) and shared; nobody writes
into it.

The smallest shapes at which the kernels can still go wrong, R = OCTO_DRAWS_SCAN_ROWS = 8 the rows of a task: one row, fewer rows than a task, R − 1, R,
R + 1 and 3R + 5 (four tasks, the last partial); one lane, one full wave, one wave and a lane, two waves and two lanes; one, two, five and eight
planets, a ThieleInnesOrbit, a RadialVelocityOrbit (contributes nothing) and a planet without a mass (contributes nothing) among them; Q = 1, 6, 8;
K = 0, 2, 4. L is random and dense, d of z's size, Σ = A·Aᵀ + I, H random: the kernel knows nothing of fits. The walkers are scan_cases.draw_elements':
valid by construction.
"""
import functools

import numpy as np

import pma_reference as pref
import scan_cases as sc
from scan_cases import R, RV, TI, V

# name: (W, n, planets [(orbit_kind, has_mass)], Q, K)
CASES = {
    "one":        (1, 1, [(V, 1)], 1, 0),
    "two_rows":   (64, 2, [(TI, 1), (V, 1)], 6, 2),
    "r_minus_1":  (65, R - 1, [(V, 1)], 8, 4),
    "r":          (130, R, [(V, 1)], 6, 2),
    "r_plus_1":   (65, R + 1, [(V, 1), (RV, 1), (V, 0), (TI, 1), (V, 1)], 6, 2),
    "four_tasks": (1, 3 * R + 5, [(V, 1)] * 8, 8, 4),
}


def draw_table(rng, n, Q, K):
    """epochs over three years, random scan angles, a dense projector whose z is of the reflex's size, and a catalogue beside it"""
    t = np.sort(rng.uniform(47900.0, 49050.0, n))
    psi = rng.uniform(0, 2 * np.pi, n)
    L = rng.normal(size=(Q, n)) / np.sqrt(n)
    A = rng.normal(size=(Q, Q))
    cov = A @ A.T + np.eye(Q)
    return pref.table(t, np.cos(psi), np.sin(psi), L, rng.normal(size=Q) * 5.0, 0.5 * (cov + cov.T), rng.normal(size=(Q, K)) if K else None)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(tab, planets, elems, gamma [K, W]) of a case, drawn from its own seed"""
    W, n, planets, Q, K = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 20270)
    tab = draw_table(rng, n, Q, K)
    return dict(tab=tab, planets=planets, elems=sc.draw_elements(rng, planets, W), gamma=rng.normal(size=(K, W)) * 2.0)


@functools.lru_cache(maxsize=None)
def restated(name, mode):
    """pma_reference.evaluate of a case in `mode`, with the gradient"""
    x = inputs(name)
    return pref.evaluate(x["tab"], x["planets"], x["elems"], x["gamma"], mode=mode, grad=True)
