"""NumPy restatement (float64) of the MIDDLE arm of k_main's Newton-only warm row (octo_device.h: kepler_warm_newton), on top of warm_newton_model.py,
which it leaves as it is — shared by tests/test_warm_newton_mid_model.py and by whoever wants to re-price the bound. No GPU, no package import.

Most wave-rows that miss τ(e) miss it by little: their Newton δ is a few 1e-6, where the fourth-order correction (23 FP64 instructions and two
reciprocals) is far more than the start needs. Between τ and WARM_TOL a wave-row whose lanes all have |δ| <= τ₂(e) takes ONE Halley step instead, written
as a series in the Newton δ with the reciprocal r1 ≈ 1/f1 the Newton head has already taken:

    q  = (e/2 · s1) · r1                     f2/(2 f1)
    δh = δ − (q δ) δ                          its truncation is |a²/2 − b/6| |δ|³, a = e sin E/D, b = e cos E/D
    w  = −δh/2;  sin E = s1 + δh (c1 + w s1),  cos E = c1 + δh (−s1 + w c1)       (the dropped δh³/6 is below 1e-16 for |δh| <= 8.4e-6)
    D  = 1 − e cos E;  1/D by TWO Newton steps on r1 (off by a·δ <~ 5e-5 relative: ~1e-17 after two)

    τ₂(e) = min((WARM_NEWTON_MID_TOL/κ(e))^(1/3), WARM_NEWTON_MID_CAP),   κ(e) = β_max²/2 + e/(6(1 − e)),   β_max = e/√(1 − e²)

(a² <= β_max² and |b| <= e/(1 − e), so κ bounds |a²/2 − b/6|). The order of the exits: a-priori reject -> cold; every lane |δ| <= τ -> Newton-only;
every lane |δ| <= τ₂ -> middle; every lane |δ| <= WARM_TOL -> fourth order; else cold. simulate() below is warm_newton_model.simulate with that
extra class and the same draws of the reciprocal's error in the same order: with class 3 folded into class 1 it returns warm_newton_model's routing."""
import numpy as np

import warm_bound_model as wbm
import warm_newton_model as wnm

WARM_NEWTON_MID_TOL = 2.0e-16      # octo_device.h: WARM_NEWTON_MID_TOL — κ τ₂³, the bound on the Halley series' truncation
WARM_NEWTON_MID_CAP = 8.0e-6       # octo_device.h: WARM_NEWTON_MID_CAP — τ₂ <= this: δ³/6 < 1e-16 in the rotation, whatever e
L = np.longdouble
COLD, FOURTH, NEWTON, MIDDLE = 0, 1, 2, 3


def kappa(e):
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 0.5 * e * e / (1.0 - e * e) + e / (6.0 * (1.0 - e))


def tau2(e, tol=None, cap=None):
    """the lane's bound on |δ| for a middle row (FP32 on the device); e = 0 and an invalid e (> 1, NaN) give the cap"""
    tol = WARM_NEWTON_MID_TOL if tol is None else tol
    cap = WARM_NEWTON_MID_CAP if cap is None else cap
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.cbrt(tol / kappa(e))
        t = np.where(kappa(e) < 0.0, np.nan, t)      # (the device takes the cube root through a logarithm: a negative κ — e > 1 — is a NaN there)
    return np.where(np.isnan(t), cap, np.minimum(t, cap))


def middle_arm(s1, c1, r1, d, e):
    """the arm from the values live at the exit: (sin E, cos E, 1/D, δh)"""
    q = ((0.5 * e) * s1) * r1
    dh = d - (q * d) * d
    w = -0.5 * dh
    sE = s1 + dh * (c1 + w * s1)
    cE = c1 + dh * (-s1 + w * c1)
    D = 1 - e * cE
    r = r1 + (1 - D * r1) * r1
    return sE, cE, r + (1 - D * r) * r, dh


def simulate(elems, t, k_yr, rng, depth=4, tol=None, cap=None, hist_dtype=np.float32):
    """warm_newton_model.simulate with the middle class. Returns a dict: cls [tiles, rows] (COLD, FOURTH, NEWTON, MIDDLE) and lane_cls; per lane-row
    delta (|δ| of the Newton head), err_mid / err_fourth / err_parent (D-weighted error of (sin E, cos E) of the middle arm, of the fourth-order arm
    from the same start, of the parent's warm step; every non-cold row), invd_rel_mid (relative error of the middle arm's 1/D), tau, tau2."""
    e = elems[1].astype(np.float64)
    W, n = e.size, t.size
    assert W % 64 == 0
    E, dM = wnm.exact_anomalies(elems, t, k_yr)
    el = e.astype(L)[:, None]
    sE = np.sin(E).astype(np.float64); cE = np.cos(E).astype(np.float64)
    Dl = 1 - el * np.cos(E)
    invD = (1 / Dl).astype(np.float64); D = Dl.astype(np.float64)
    thr = wbm.warm_thr(e, dM * (1 + 2.0 ** -18))
    veto = (np.abs(dM) > wbm.WARM_DM_VETO).reshape(-1, 64).any(axis=1)
    tl, tl2 = wnm.tau(e), tau2(e, tol, cap)
    T = W // 64
    cls = np.zeros((T, n), dtype=np.int8)
    nan = lambda: np.full((W, n), np.nan)
    err_mid, err_4, err_par, invd_rel, delta = nan(), nan(), nan(), nan(), nan()
    hist = np.zeros((depth, W), dtype=hist_dtype)
    cnt = np.zeros(T, dtype=np.int64)
    lane = lambda x: np.repeat(x, 64)
    every = lambda m: ~(m.reshape(T, 64).any(axis=1))      # (a NaN lane passes, as on the device)
    derr = lambda s, c, j: np.maximum(np.abs(s - sE[:, j]), np.abs(c - cE[:, j])) * D[:, j]
    for j in range(1, n):
        s0, c0, i0 = sE[:, j - 1], cE[:, j - 1], invD[:, j - 1]
        dE2 = wnm.predictor(s0, c0, i0, dM, e)
        cp = sum(hist.dtype.type(k) * hist[i] for i, k in enumerate(wnm.EXTRAPOLATE[depth]))
        cp = np.where(lane(cnt >= depth), cp, 0.0).astype(np.float64)
        s1, c1, f0 = wnm.rotate_f0(s0, c0, dE2 + cp, dM, e)
        r1, d = wnm.newton_head(c1, f0, e, rng)
        delta[:, j] = np.abs(d)
        apriori = every(i0 >= thr) & ~veto
        cold = ~apriori | ~every(np.abs(d) > wbm.WARM_TOL)
        newton = ~cold & every(np.abs(d) > tl)
        middle = ~cold & ~newton & every(np.abs(d) > tl2)
        cls[:, j] = np.where(cold, COLD, np.where(newton, NEWTON, np.where(middle, MIDDLE, FOURTH)))
        s4, c4, _ = wnm.fourth_order(s1, c1, f0, e, rng)
        sp, cpar = wbm.warm_arm(s0, c0, i0, dM, e, rng)
        sm, cm, rm, _ = middle_arm(s1, c1, r1, d, e)
        cl = lane(cold)
        err_mid[:, j] = np.where(cl, np.nan, derr(sm, cm, j))
        err_4[:, j] = np.where(cl, np.nan, derr(s4, c4, j))
        err_par[:, j] = np.where(cl, np.nan, derr(sp, cpar, j))
        invd_rel[:, j] = np.where(cl, np.nan, np.abs(rm * D[:, j] - 1.0))
        ctrue = ((E[:, j] - E[:, j - 1]) - dE2.astype(L)).astype(hist_dtype)
        hist = np.where(cl[None, :], hist_dtype(0.0), np.concatenate([ctrue[None, :], hist[:-1]], axis=0))
        cnt = np.where(cold, 0, np.minimum(cnt + 1, depth))
    return dict(cls=cls, lane_cls=np.repeat(cls, 64, axis=0), delta=delta, err_mid=err_mid, err_fourth=err_4, err_parent=err_par,
                invd_rel_mid=invd_rel, tau=tl, tau2=tl2)
