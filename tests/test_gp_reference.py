"""
The two restatements of the Gaussian-process RV likelihood (tests/gp_reference.py) held to third parties and to each other. CPU suite.

  dense        against scipy.stats.multivariate_normal.logpdf on a covariance built in float64 from the celerite terms an SHO stands for, and the
               conditional mean against the textbook K_gp·(K_gp + N)⁻¹·r
  recursion    the float64 NumPy recursion and its reverse pass against the dense reference at the project's bar, 1e-8 relative to max(1, |ref|), on
               every case of tests/gp_cases.py: ℓ, α and every gradient the recursion forms (hyperparameters, jitter). The restatement takes the
               residuals as given: it forms no β or element adjoints (they are α against the design columns and the planets' sums), which the dense
               reference holds the device to in tests/test_gp.py.
"""
import numpy as np
import pytest
from scipy import stats

import gp_cases as gc
import gp_reference as gref

BAR = 1e-8


def close(x, ref, what):
    x, ref = np.asarray(x), np.asarray(ref)
    err = np.abs(x - ref) / np.maximum(1.0, np.abs(ref))
    print(f"{what}: max error relative to max(1, |ref|) = {err.max() if err.size else 0.0:.3e}")
    assert np.all(err <= BAR), (what, float(err.max()), np.unravel_index(np.argmax(err), err.shape))


def celerite_cov(t, terms, hyper):
    """Σ_terms k(|t_i − t_j|) in float64 from the REAL and COMPLEX forms of every term (an SHO through its celerite coefficients)"""
    tau = np.abs(t[:, None] - t[None, :])
    K, o = np.zeros_like(tau), 0
    for kind in terms:
        h = hyper[o:o + gref.N_HYPER[kind]]
        o += gref.N_HYPER[kind]
        if kind == gref.REAL:
            K += h[0] * np.exp(-h[1] * tau)
        elif kind == gref.COMPLEX:
            K += np.exp(-h[2] * tau) * (h[0] * np.cos(h[3] * tau) + h[1] * np.sin(h[3] * tau))
        else:
            S0, Q, w0 = h
            if Q > 0.5:
                f = np.sqrt(4 * Q * Q - 1)
                a, c = S0 * w0 * Q, w0 / (2 * Q)
                K += np.exp(-c * tau) * (a * np.cos(c * f * tau) + a / f * np.sin(c * f * tau))
            else:
                f = np.sqrt(1 - 4 * Q * Q)
                for sgn in (1.0, -1.0):
                    K += 0.5 * S0 * w0 * Q * (1 + sgn / f) * np.exp(-w0 / (2 * Q) * (1 - sgn * f) * tau)
    return K


@pytest.mark.parametrize("name", ["sho_both", "g_minus_1"])
def test_the_dense_reference_against_scipy_and_the_textbook_mean(name):
    x, r = gc.inputs(name), gc.reference(name)
    tab = x["tab"]
    for w in range(min(4, x["elems"].shape[1])):
        s = 0.0 if x["jitter"] is None else x["jitter"][w]
        Kgp = celerite_cov(tab["t"], x["terms"], x["hyper"][:, w])
        N = np.diag(tab["sigma"] ** 2 + s * s)
        res = tab["rv"] - r["eta"][:, w]
        ll = stats.multivariate_normal.logpdf(res, mean=np.zeros(res.size), cov=Kgp + N)
        assert abs(ll - r["ll"][w]) <= 1e-9 * max(1.0, abs(ll)), (w, ll, r["ll"][w])
        mu = Kgp @ np.linalg.solve(Kgp + N, res)
        assert np.all(np.abs(mu - r["mu"][:, w]) <= 1e-9 * np.maximum(1.0, np.abs(mu)))


@pytest.mark.parametrize("name", list(gc.CASES))
def test_the_recursion_against_the_dense_reference(name):
    x, r = gc.inputs(name), gc.reference(name)
    tab, W = x["tab"], x["elems"].shape[1]
    assert np.all(np.isfinite(r["ll"]))      # every drawn walker is valid
    s = np.zeros(W) if x["jitter"] is None else x["jitter"]
    o = gref.recursion(tab["t"], tab["rv"][:, None] - r["eta"], tab["sigma"], s, x["terms"], x["hyper"])
    print("smallest D:", float(o["D_min"].min()))
    close(o["ll"], r["ll"], "ll")
    close(o["alpha"], r["alpha"], "alpha")
    close(o["g_hyper"], r["g_hyper"], "g_hyper")
    close(o["g_jitter"], r["g_jitter"], "g_jitter")


def test_the_reference_calls_the_invalid_walkers_invalid():
    x = gc.inputs("sho_both")
    hy = x["hyper"][:, :4].copy()
    hy[1, 0] = 0.5            # Q = ½
    hy[2, 1] = -0.3           # ω0 < 0: a rate <= 0
    hy[0, 2] = np.nan
    hy[0, 3] = -40.0          # S0 < 0: the kernel is not positive definite
    r = gref.dense(x["tab"], x["terms"], x["planets"], x["elems"][:, :4], hy, x["beta"][:, :4], x["jitter"][:4], grad=False)
    assert np.all(r["ll"] == -np.inf)
    s = x["jitter"][:4]
    o = gref.recursion(x["tab"]["t"], np.ones((x["tab"]["t"].size, 4)), x["tab"]["sigma"], s, x["terms"], hy, grad=False)
    assert np.all(o["ll"] == -np.inf)
