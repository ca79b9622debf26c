"""NumPy restatement (float64) of k_main's warm Kepler step and of its a-priori bound (octo_device.h: warm_thr, kepler_warm_step,
kepler_correct<., FOURTH_ORDER>), with the device's polynomial orders — shared by tests/test_warm_bound.py, tools/kepler_warm_proto.py and
tools/warm_rates.py, so that the tools and the test can never calibrate against different bounds. No GPU, no package import.

The bound: a row starts warm when every lane's previous 1/D is below thr(e, |ΔM|).

    parent:  thr = (WARM_TOL/ΔM³)^(1/5)                      <=>  x³/D² < WARM_TOL,   x = ΔM/D
    now:     thr = max(parent, min(c(e), X_CAP)/ΔM)          <=>  … or  |x| < min(c(e), X_CAP)

c(e) = (6·WARM_C3/q_cap(e))^(1/3) from the predictor's third-order term (x³/6)(3β² − α) <= (x³/6) q(v), q(v) = 7v − 4 − 3(1 − e²)v², v = 1/D,
q_cap = max of q on [1, 1/(1 − e)]: 49/(12(1 − e²)) − 4 for e > 1/6, e/(1 − e) (the periastron itself) below. Above WARM_E_MAX the
eccentricity-aware term is dropped (the parent's bound alone): there the fourth-order term of the predictor, which grows like v³, is no
longer small against the third-order one the constant prices."""
import numpy as np

TWO_PI = 2 * np.pi
WARM_TOL = 1.0e-3
WARM_MIN_THR = 2.0
WARM_DM_VETO = 0.0314
WARM_C3 = 2.5e-4          # bound on the predictor's third-order term (octo_device.h: WARM_C3)
WARM_X_CAP = 0.06         # |x| = ΔM/D the rotation's polynomials are exact for (octo_device.h: WARM_X_CAP)
WARM_E_MAX = 0.99         # above: the parent's bound alone (octo_device.h: WARM_E_MAX)


def warm_thr_parent(dM):
    return (WARM_TOL / np.abs(dM) ** 3) ** 0.2


def q_cap(e):
    ome2 = 1.0 - e * e
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(e > 1.0 / 6.0, 49.0 / (12.0 * ome2) - 4.0, e / (1.0 - e))


def warm_thr(e, dM, c3=None, x_cap=None, e_max=None):
    """the lane's bound on the previous row's 1/D; float64 here, FP32 on the device (the tests leave 2 % between the two)"""
    c3 = WARM_C3 if c3 is None else c3
    x_cap = WARM_X_CAP if x_cap is None else x_cap
    e_max = WARM_E_MAX if e_max is None else e_max
    e = np.asarray(e, dtype=np.float64); dM = np.abs(np.asarray(dM, dtype=np.float64))
    old = warm_thr_parent(dM)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.cbrt(6.0 * c3 / q_cap(e))
    new = np.where((e >= 0.0) & (e < e_max), np.minimum(c, x_cap), 0.0) / dM
    return np.maximum(old, new)


def _rcp23(x, rng):
    """v_rcp_f64: good to ~2^-23"""
    return (1.0 / x) * (1 + rng.uniform(-1, 1, np.shape(x)) * 2.0 ** -23)


def warm_arm(sE, cE, invD, dM, e, rng):
    """kepler_warm_step: second-order predictor, rotation (sin to dE⁷, cos to dE⁸), f0 without E or M, fourth-order correction, rotation by δ4"""
    x = dM * invD
    z = x * invD
    dE = x - ((0.5 * e * sE) * z) * x
    u = dE * dE
    sr = dE * (1 + u * (-1 / 6 + u * (1 / 120 + u * (-1 / 5040))))
    cm1 = u * (-0.5 + u * (1 / 24 + u * (-1 / 720 + u / 40320)))
    ds = sE * cm1 + cE * sr
    s1 = sE + ds
    c1 = cE + (cE * cm1 - sE * sr)
    f0 = (dE - dM) - e * ds
    hf2 = 0.5 * e * s1; sf3 = e / 6 * c1; f1 = 1 - e * c1
    r3 = _rcp23(f1 * f1 - f0 * hf2, rng)
    r4 = f1 * r3; d3 = -f0 * r4
    den4 = f1 + d3 * (hf2 + d3 * sf3)
    d4 = d3 - r4 * (den4 * d3 + f0)
    dd = d4 * d4
    sd = d4 * (1 + dd * (-1 / 6)); cd = dd * (-0.5 + dd / 24)
    return s1 + (c1 * sd + s1 * cd), c1 + (-s1 * sd + c1 * cd)


def one_step_errors(e, E, dM, rng):
    """The previous row's exact state at E (rounded to float64), one warm step by dM; the D-weighted error of (sin E, cos E) against an
    80-bit Newton solve at M + ΔM, and the previous row's 1/D (what the bound is tested against)."""
    L = np.longdouble
    el, El = e.astype(L), E.astype(L)
    sE = np.sin(El).astype(np.float64); cE = np.cos(El).astype(np.float64)
    invD = (1 / (1 - el * np.cos(El))).astype(np.float64)
    s, c = warm_arm(sE, cE, invD, dM, e, rng)
    Mn = (El - el * np.sin(El)) + dM.astype(L)
    Et = El + dM.astype(L) * invD.astype(L)
    Et = np.where(np.abs(Et - El) > 0.5, El + np.sign(dM) * 0.5, Et)
    for _ in range(80):
        Et = Et - (Et - el * np.sin(Et) - Mn) / (1 - el * np.cos(Et))
    conv = np.abs(Et - el * np.sin(Et) - Mn) < 1e-17
    D = (1 - el * np.cos(Et)).astype(np.float64)
    err = np.maximum(np.abs(s - np.sin(Et).astype(np.float64)), np.abs(c - np.cos(Et).astype(np.float64))) * D
    return err, invD, conv


def draw_samples(rng, n):
    """(e, E, ΔM): e uniform on [0, 1) and log-dense towards 1 − 1e-9; every phase, half of the sample within |E| < 0.6 of periastron;
    ΔM log-uniform on [1e-7, WARM_DM_VETO], both signs"""
    h = n // 2
    e = np.concatenate([rng.uniform(0, 1, h), 1 - 10 ** rng.uniform(-9, -0.3, n - h)])
    E = np.concatenate([rng.uniform(-np.pi, np.pi, h), rng.uniform(-0.6, 0.6, n - h)])
    rng.shuffle(E)
    dM = 10 ** rng.uniform(-7, np.log10(WARM_DM_VETO), n) * rng.choice([-1.0, 1.0], n)
    return e, E, dM


def kepler_E(M, e):
    """E(M) by Newton in float64 (the bound needs 1/D to a few digits only)"""
    M = np.asarray(M, dtype=np.float64)
    Mr = M - TWO_PI * np.rint(M / TWO_PI)
    E = Mr + 0.85 * e * np.sign(np.sin(Mr))
    for _ in range(30):
        E = E - (E - e * np.sin(E) - Mr) / (1 - e * np.cos(E))
    return E


def cold_wave_row_share(elems, t, thr_fn, k_yr):
    """Share of the wave-rows (tiles of 64 walkers in the order given) that are solved cold: some lane's previous 1/D >= thr. Lanes whose ΔM
    vetoes the step bound make their whole tile cold. Returns (wave-row share, lane-row share over the lanes that do not veto)."""
    a, e, tp, Ms = elems[0], elems[1], elems[5], elems[6]
    P = k_yr * np.sqrt(a ** 3 / Ms)
    dM = TWO_PI * np.median(np.diff(t)) / P
    veto = dM > WARM_DM_VETO
    thr = thr_fn(e, dM)
    W = e.size
    fail = np.zeros((W, t.size), dtype=bool)
    for lo in range(0, W, 256):
        sl = slice(lo, min(lo + 256, W))
        Mm = TWO_PI * (t[None, :] - tp[sl, None]) / P[sl, None]
        Ee = kepler_E(Mm, e[sl, None])
        invD = 1.0 / (1.0 - e[sl, None] * np.cos(Ee))
        fail[sl, 1:] = invD[:, :-1] >= thr[sl, None]
    fail[veto, :] = True
    n_tiles = W // 64
    wave = fail[:n_tiles * 64].reshape(n_tiles, 64, -1).any(axis=1)[:, 1:].mean()
    return wave, (fail[~veto][:, 1:].mean() if (~veto).any() else 0.0)
