"""
The two restatements of the dense Gaussian-process RV likelihood (tests/gpd_reference.py) against each other, and the conditions on the drawn inputs
(tests/gpd_cases.py). CPU suite: no GPU.
"""
import mpmath as mp
import numpy as np
import pytest

import gp_reference as gref
import gpd_cases as dc
import gpd_reference as dref

KEYS = ("ll", "g_elems", "g_hyper", "g_beta", "g_jitter", "eta", "mu", "alpha")
SHORT = [name for name, case in dc.CASES.items() if case[1] <= dc.MP_ROWS]


def test_the_cases_cover_what_they_claim():
    ns = {case[1] for case in dc.CASES.values()}
    assert {1, 2, 3, 63, 64, 65, dref.LDS_ROWS, dref.LDS_ROWS + 1, 257} <= ns
    assert {case[0] for case in dc.CASES.values()} == {1, 2, 3, 65, 130} and all(case[1] <= 9 for case in dc.CASES.values() if case[0] > 3)
    assert {case[3] for case in dc.CASES.values()} == {0, 1, 2, 4} and {repr(case[4]) for case in dc.CASES.values()} == {"None", "0.0", "'draw'"}
    alone = {case[5][0] for case in dc.CASES.values() if len(case[5]) == 1}
    assert alone == set(dref.N_HYPER) and [dc.QP, dc.M32] in [c[5] for c in dc.CASES.values()] and [dc.QP] * 4 in [c[5] for c in dc.CASES.values()]
    planets = [p for case in dc.CASES.values() for p in case[2]]
    assert {(dc.RV, 1), (dc.KEP, 1), (dc.V, 1), (dc.V, 0)} <= set(planets) and any(len(case[2]) == 8 for case in dc.CASES.values())
    assert len(SHORT) >= 7 and set(SHORT) == {n for n, c in dc.CASES.items() if c[1] <= 17}


@pytest.mark.parametrize("name", list(dc.CASES))
def test_every_case_is_valid_and_well_conditioned(name):
    r = dc.numpy_reference(name)
    print(f"{name}: cond(K) max = {np.max(r['cond']):.3e}")
    assert np.all(np.isfinite(r["ll"])) and np.all(r["cond"] <= 1e6)      # a condition on the inputs, not a measurement


@pytest.mark.parametrize("name", SHORT)
def test_numpy_against_mpmath(name):
    r, m = dc.numpy_reference(name), dc.mp_reference(name)
    assert np.all(np.isfinite(m["ll"]))
    for k in KEYS:
        err = np.abs(r[k] - m[k]) / np.maximum(1.0, np.abs(m[k]))
        print(f"{name} {k}: {err.max() if err.size else 0.0:.3e}")
        assert np.all(err <= 1e-10), (name, k)


@pytest.mark.parametrize("kind", list(dref.N_HYPER))
def test_the_closed_form_derivatives_against_the_complex_step(kind):
    rng = np.random.default_rng(kind)
    for _ in range(6):
        h = dc.draw_hyper(rng, [kind], 1)[:, 0]
        tau = np.concatenate([[0.0], rng.uniform(0.0, 300.0, 7)])
        k, dk = dref.kernel_np(kind, h, tau)
        with mp.workdps(gref.DPS):
            for i, x in enumerate(tau):
                hm, xm = [mp.mpf(float(v)) for v in h], mp.mpf(float(x))
                assert abs(k[i] - float(dref.kernel_value(kind, hm, xm))) <= 1e-13 * max(1.0, abs(k[i]))
                for p in range(len(h)):
                    h1 = list(hm)
                    h1[p] = mp.mpc(h1[p], gref.STEP)
                    ref = float(mp.im(dref.kernel_value(kind, h1, xm)) / gref.STEP)
                    assert abs(dk[p][i] - ref) <= 1e-12 * max(1.0, abs(ref)), (kind, p, x, dk[p][i], ref)


def test_invalid_hyperparameters():
    h = np.array([2.0, 10.0, 25.0, 0.5])
    assert dref.valid_hyper([dref.QUASIPERIODIC], h)
    for p, bad in ((1, 0.0), (2, -3.0), (3, 0.0), (0, np.nan), (0, 1e200), (1, np.inf)):
        x = h.copy()
        x[p] = bad
        assert not dref.valid_hyper([dref.QUASIPERIODIC], x), (p, bad)
    x = h.copy()
    x[0] = -2.0      # a enters as a²
    assert dref.valid_hyper([dref.QUASIPERIODIC], x)
