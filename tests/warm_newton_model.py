"""NumPy restatement (float64) of k_main's Newton-only warm row (octo_device.h: kepler_warm_newton), in the manner of warm_bound_model.py, which it
builds on — shared by tests/test_warm_newton_model.py and by whoever wants to re-price the candidates. No GPU, no package import.

On an evenly sampled table the gap between the true step of E and its second-order Taylor predictor,

    c_j = (E_j − E_{j−1}) − dE2_j,     dE2 = x − ½ (e sin E / D) x²,  x = ΔM / D,

is smooth in j, and its value for the rows behind is known: it is the correction that was applied. Extrapolated from the last rows — the polynomial
through the last four, c_pred = 4 (c₁ + c₃) − 6 c₂ − c₄ (FP32 on the device: the history only has to be good to ~1e-9) — the start dE2 + c_pred lies within ~1e-8 of the root for most
rows, and there ONE Newton step δ = −f0/f1 is exact to rounding: its truncation is δ² (e sin E)/(2D) <= ½ δ² β_max, β_max = e/√(1 − e²). A wave-row is

    cold           the a-priori bound rejects it (warm_bound_model.warm_thr), or some lane has |δ| > WARM_TOL — the history starts again;
    fourth order   otherwise, some lane has |δ| > τ(e) = min(√(WARM_NEWTON_TOL/β_max), WARM_NEWTON_CAP): the parent's correction from the same (s1, c1, f0);
    Newton-only    otherwise: sin E = s1 + c1 δ, cos E = c1 − s1 δ (δ²/2 < 1e-16), 1/D one Newton step from the reciprocal taken for δ.

c_pred is exactly 0 until `depth` consecutive rows have recorded a c. Every row is modelled from the EXACT previous state (80-bit Newton), as
warm_bound_model.one_step_errors does: what is priced is one step's error and the routing, not the chain's accumulated rounding."""
import numpy as np

import warm_bound_model as wbm

TWO_PI = 2 * np.pi
WARM_NEWTON_TOL = 4.0e-16      # octo_device.h: WARM_NEWTON_TOL — τ² β_max, twice the Newton step's truncation bound
WARM_NEWTON_CAP = 1.4e-8       # octo_device.h: WARM_NEWTON_CAP — τ <= this: δ²/2 < 1e-16 in the rotation, whatever e
L = np.longdouble
# c_pred from the last `depth` values, latest first: the polynomial through them, one step on (3: 3(c1 − c2) + c3, 4: 4(c1 + c3) − 6 c2 − c4)
EXTRAPOLATE = {2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1), 5: (5, -10, 10, -5, 1), 6: (6, -15, 20, -15, 6, -1)}


def tau(e):
    """the lane's bound on |δ| for a Newton-only row (FP32 on the device); an invalid e (>= 1, NaN) gives the cap"""
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.sqrt(WARM_NEWTON_TOL * np.sqrt(1.0 - e * e) / e)
    return np.where(np.isnan(t), WARM_NEWTON_CAP, np.minimum(t, WARM_NEWTON_CAP))


def predictor(sE, cE, invD, dM, e):
    x = dM * invD
    z = x * invD
    return x - ((0.5 * e * sE) * z) * x


def rotate_f0(sE, cE, dE, dM, e):
    """(sin, cos)(E + dE) by the device's polynomials and f0 = E1 − e sin E1 − M without E or M"""
    u = dE * dE
    sr = dE * (1 + u * (-1 / 6 + u * (1 / 120 + u * (-1 / 5040))))
    cm1 = u * (-0.5 + u * (1 / 24 + u * (-1 / 720 + u / 40320)))
    ds = sE * cm1 + cE * sr
    s1 = sE + ds
    c1 = cE + (cE * cm1 - sE * sr)
    f0 = (dE - dM) - e * ds
    return s1, c1, f0


def newton_head(c1, f0, e, rng):
    """f1, its reciprocal (v_rcp_f64 + one Newton step: 2^-46) and δ = −f0/f1"""
    f1 = 1 - e * c1
    r = wbm._rcp23(f1, rng)
    r1 = r + (1 - f1 * r) * r
    return r1, -f0 * r1


def newton_tail(s1, c1, r1, d, e):
    sE = s1 + c1 * d
    cE = c1 - s1 * d
    D = 1 - e * cE
    return sE, cE, r1 + (1 - D * r1) * r1


def fourth_order(s1, c1, f0, e, rng):
    """kepler_correct<., FOURTH_ORDER> from (s1, c1, f0): (sin E, cos E, δ4) — warm_bound_model.warm_arm's second half"""
    hf2 = 0.5 * e * s1; sf3 = e / 6 * c1; f1 = 1 - e * c1
    r3 = wbm._rcp23(f1 * f1 - f0 * hf2, rng)
    r4 = f1 * r3; d3 = -f0 * r4
    den4 = f1 + d3 * (hf2 + d3 * sf3)
    d4 = d3 - r4 * (den4 * d3 + f0)
    dd = d4 * d4
    sd = d4 * (1 + dd * (-1 / 6)); cd = dd * (-0.5 + dd / 24)
    return s1 + (c1 * sd + s1 * cd), c1 + (-s1 * sd + c1 * cd), d4


def exact_anomalies(elems, t, k_yr):
    """E of every (walker, row) to 80 bits, continuous along the rows (no 2π wrap), and ΔM of one row step"""
    a, e, tp, Ms = (elems[k].astype(L) for k in (0, 1, 5, 6))
    P = L(k_yr) * np.sqrt(a ** 3 / Ms)
    M = L(TWO_PI) * (t.astype(L)[None, :] - tp[:, None]) / P[:, None]
    k = np.rint(M[:, :1] / L(TWO_PI))
    M = M - L(TWO_PI) * k
    E = M + e[:, None] * np.sin(M)
    for _ in range(12):
        E = E - (E - e[:, None] * np.sin(E) - M) / (1 - e[:, None] * np.cos(E))
    for _ in range(60):      # (Newton from M + e sin M converges for every e < 1; the second loop polishes near-parabolic lanes)
        E = E - (E - e[:, None] * np.sin(E) - M) / (1 - e[:, None] * np.cos(E))
    assert np.all(np.abs(E - e[:, None] * np.sin(E) - M) < 1e-16)
    return E, (L(TWO_PI) * L(t[1] - t[0]) / P).astype(np.float64)


def simulate(elems, t, k_yr, rng, depth=4, taylor3=False, hist_dtype=np.float32):
    """One chain over the rows t (evenly spaced) for the walkers of elems [9, W], W a multiple of 64, tiles of 64 in the order given.
    depth: values of c kept (EXTRAPOLATE; the device keeps WARM_NEWTON_DEPTH = 4, in FP32). taylor3: the predictor carries the third-order term.
    Returns a dict: cls [tiles, rows] (0 cold, 1 fourth order, 2 Newton-only), per lane-row err_new / err_parent (D-weighted error of (sin E, cos E) of the
    arm the row took / of the parent's step, NaN in a cold row), invd_rel (Newton-only rows), delta (|δ| of the Newton head)."""
    e = elems[1].astype(np.float64)
    W, n = e.size, t.size
    assert W % 64 == 0
    E, dM = exact_anomalies(elems, t, k_yr)
    el = e.astype(L)[:, None]
    sE = np.sin(E).astype(np.float64); cE = np.cos(E).astype(np.float64)
    Dl = 1 - el * np.cos(E)
    invD = (1 / Dl).astype(np.float64); D = Dl.astype(np.float64)
    thr = wbm.warm_thr(e, dM * (1 + 2.0 ** -18))
    veto = (np.abs(dM) > wbm.WARM_DM_VETO).reshape(-1, 64).any(axis=1)
    tl = tau(e)
    T = W // 64
    cls = np.zeros((T, n), dtype=np.int8)
    err_new = np.full((W, n), np.nan); err_par = np.full((W, n), np.nan); invd_rel = np.full((W, n), np.nan); delta = np.full((W, n), np.nan)
    hist = np.zeros((depth, W), dtype=hist_dtype)
    cnt = np.zeros(T, dtype=np.int64)
    lane = lambda x: np.repeat(x, 64)
    for j in range(1, n):
        s0, c0, i0 = sE[:, j - 1], cE[:, j - 1], invD[:, j - 1]
        dE2 = predictor(s0, c0, i0, dM, e)
        if taylor3:
            x = dM * i0; be = e * s0 * i0; al = e * c0 * i0
            dE2 = dE2 + (x ** 3 / 6) * (3 * be * be - al)
        cp = sum(hist.dtype.type(k) * hist[i] for i, k in enumerate(EXTRAPOLATE[depth]))
        cp = np.where(lane(cnt >= depth), cp, 0.0).astype(np.float64)
        dE = dE2 + cp
        s1, c1, f0 = rotate_f0(s0, c0, dE, dM, e)
        r1, d = newton_head(c1, f0, e, rng)
        delta[:, j] = np.abs(d)
        apriori = ~((i0 >= thr).reshape(T, 64).any(axis=1)) & ~veto
        cold = ~apriori | (np.abs(d) > wbm.WARM_TOL).reshape(T, 64).any(axis=1)
        newton = ~cold & ~((np.abs(d) > tl).reshape(T, 64).any(axis=1))
        cls[:, j] = np.where(cold, 0, np.where(newton, 2, 1))
        sn, cn, rn = newton_tail(s1, c1, r1, d, e)
        s4, c4, _ = fourth_order(s1, c1, f0, e, rng)
        nl, cl = lane(newton), lane(cold)
        s = np.where(nl, sn, s4); c = np.where(nl, cn, c4)
        en = np.maximum(np.abs(s - sE[:, j]), np.abs(c - cE[:, j])) * D[:, j]
        err_new[:, j] = np.where(cl, np.nan, en)
        sp, cpar = wbm.warm_arm(s0, c0, i0, dM, e, rng)
        err_par[:, j] = np.where(cl, np.nan, np.maximum(np.abs(sp - sE[:, j]), np.abs(cpar - cE[:, j])) * D[:, j])
        invd_rel[:, j] = np.where(nl, np.abs(rn * D[:, j] - 1.0), np.nan)
        # the history: the correction that was applied, i.e. the true step less the Taylor predictor (the arms agree with it to rounding)
        ctrue = ((E[:, j] - E[:, j - 1]) - dE2.astype(L)).astype(hist_dtype)
        hist = np.where(cl[None, :], hist_dtype(0.0), np.concatenate([ctrue[None, :], hist[:-1]], axis=0))
        cnt = np.where(cold, 0, np.minimum(cnt + 1, depth))
    return dict(cls=cls, err_new=err_new, err_parent=err_par, invd_rel=invd_rel, delta=delta, tau=tl, lane_cls=np.repeat(cls, 64, axis=0))
