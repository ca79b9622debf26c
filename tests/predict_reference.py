"""Reference side of the model-value tests (a helper, not a test): per-(walker, planet, epoch) primitives from the oracle's
octo_oracle_orbitsolve, the channel definitions of include/octofitter_hip_predict.h composed in NumPy, and a host-side Gaussian
log-likelihood of RADEC (with cor), SEPPA, RV_ABS and RV_REL tables FROM model values — the formulas of
oracle/octo_oracle_core.inc:377-405, 446-470. tests/test_predict_reference.py checks this file against oracle_eval alone, so that in the
GPU closure test the device is the only unknown."""
from __future__ import annotations

import numpy as np

import oracle_binding as ob

capi = ob.capi
predict = ob.pkg.predict
LOG2PI = float(np.log(2.0 * np.pi))
ASTROM_QUANTITIES = (predict.RAOFF, predict.DECOFF, predict.SEP, predict.PA)
COMPOSITE_QUANTITIES = (predict.ASTROM_RA, predict.ASTROM_DEC, predict.ASTROM_SEP, predict.ASTROM_PA)


def primitives(planets, elems, epochs, consts=None):
    """dict(ra, dec, rv: [P, T, W]; K, cart2angle: [P, W]) from one oracle call per (walker, planet, epoch)."""
    elems = np.asarray(elems, dtype=np.float64)
    epochs = np.asarray(epochs, dtype=np.float64)
    P, T, W = len(planets), epochs.size, elems.shape[1]
    out = dict(ra=np.empty((P, T, W)), dec=np.empty((P, T, W)), rv=np.empty((P, T, W)), K=np.empty((P, W)), cart2angle=np.empty((P, W)))
    for p, pl in enumerate(planets):
        for w in range(W):
            el = np.ascontiguousarray(elems[p * 9:(p + 1) * 9, w])
            for j, t in enumerate(epochs):
                s = ob.oracle_orbitsolve(el, t, orbit_kind=int(pl["orbit_kind"]), consts=consts)
                out["ra"][p, j, w], out["dec"][p, j, w], out["rv"][p, j, w] = s["raoff"], s["decoff"], s["radvel"]
            out["K"][p, w], out["cart2angle"][p, w] = s["K"], s["cart2angle"]
    return out


def mass_ratio(planets, elems, consts=None):
    """m_p / M_p [P, W]: 0 for a planet that declares no mass."""
    c = consts or ob.oracle_consts()
    return np.stack([(elems[p * 9 + capi.EL_MASS] * c.mjup2msol / elems[p * 9 + capi.EL_M]) if pl["has_mass"] else np.zeros(elems.shape[1])
                     for p, pl in enumerate(planets)])


def channel_values(planets, elems, epochs, channels, add0=None, add1=None, basis=None, consts=None, prims=None):
    """[C, T, W]: the channel table of the header, from the oracle's primitives."""
    elems = np.asarray(elems, dtype=np.float64)
    pr = prims or primitives(planets, elems, epochs, consts)
    P, T, W = pr["ra"].shape
    mu = mass_ratio(planets, elems, consts)
    sma = np.stack([elems[p * 9 + capi.EL_A] for p in range(P)])
    out = np.empty((len(channels), T, W))
    for c, (q, pl) in enumerate(channels):
        if q in (predict.RADVEL, predict.RV_STAR, predict.RV_REL):
            v = np.zeros((T, W))
            if add0 is not None:
                v = v + np.asarray(add0)[c][None, :]
            if add1 is not None and basis is not None:
                v = v + np.asarray(add1)[c][None, :] * np.asarray(basis)[:, None]
            if q == predict.RADVEL:
                v = v + pr["rv"][pl]
            elif q == predict.RV_STAR:
                for p in range(P):
                    v = v - mu[p][None, :] * pr["rv"][p]
            else:
                v = v + pr["rv"][pl]
                for p in range(P):
                    inner = (sma[p] < sma[pl]) & (p != pl)
                    v = v - np.where(inner, mu[p], 0.0)[None, :] * pr["rv"][p]
            out[c] = v
            continue
        x, y = pr["ra"][pl].copy(), pr["dec"][pl].copy()
        if q in COMPOSITE_QUANTITIES:
            for p in range(P):
                inner = (sma[p] < sma[pl]) & (p != pl)
                x = x + np.where(inner, mu[p], 0.0)[None, :] * pr["ra"][p]      # offset MINUS the reflex −m/M·raoff
                y = y + np.where(inner, mu[p], 0.0)[None, :] * pr["dec"][p]
        if q in (predict.RAOFF, predict.ASTROM_RA):
            out[c] = x
        elif q in (predict.DECOFF, predict.ASTROM_DEC):
            out[c] = y
        elif q in (predict.SEP, predict.ASTROM_SEP):
            out[c] = np.hypot(x, y)
        else:
            out[c] = np.arctan2(x, y)
    return out


def natural_scales(planets, elems, prims):
    """Per (planet, walker): a·plx·(1 + e) [mas] for offsets (a ThieleInnesOrbit: the size of its constants) and K·(1 + e) [m/s] for velocities."""
    P, W = len(planets), elems.shape[1]
    off, vel = np.empty((P, W)), np.empty((P, W))
    for p, pl in enumerate(planets):
        e = elems[p * 9 + capi.EL_E]
        if pl["orbit_kind"] == capi.ORBIT_THIELE_INNES:
            size = np.sqrt(sum(elems[p * 9 + k] ** 2 for k in (0, 2, 3, 4)))
        else:
            size = elems[p * 9 + capi.EL_A] * elems[p * 9 + capi.EL_PLX]
        off[p] = size * (1.0 + e)
        vel[p] = np.abs(prims["K"][p]) * (1.0 + e)
    return off, vel


def table_models(obs_tables, planets, elems, nuis=None, consts=None):
    """What callers.simulate_tables returns, from the oracle's primitives."""
    out = []
    for io, t in enumerate(obs_tables):
        kind, ip = int(t["kind"]), int(t["planet"])
        add0 = add1 = basis = None
        if kind in (capi.ASTROM_RADEC, capi.ONEIL_RADEC):
            names, ch = ("ra", "dec"), [(predict.ASTROM_RA, ip), (predict.ASTROM_DEC, ip)]
        elif kind in (capi.ASTROM_SEPPA, capi.ONEIL_SEPPA):
            names, ch = ("pa", "sep"), [(predict.ASTROM_PA, ip), (predict.ASTROM_SEP, ip)]
        else:
            names, ch = ("rv",), [(predict.RV_REL, ip) if kind == capi.RV_REL else (predict.RV_STAR, -1)]
            if nuis is not None:
                if kind != capi.RV_ABS_MARG:
                    add0 = nuis[io * 3 + capi.NU_RV_OFFSET][None, :]
                if t.get("extra") is not None:
                    add1, basis = nuis[io * 3 + capi.NU_RV_TREND][None, :], t["extra"]
        v = channel_values(planets, elems, t["epoch"], ch, add0, add1, basis, consts)
        out.append({n: v[k] for k, n in enumerate(names)})
    return out


def _logpdf_diag2(s1, s2, r1, r2):
    v1, v2 = s1 * s1, s2 * s2
    return -(np.log(v1) + np.log(v2) + 2.0 * LOG2PI) / 2.0 - (r1 * r1 / v1 + r2 * r2 / v2) / 2.0


def _logpdf_dense2(s1, s2, cor, r1, r2):
    S11, S22, S21 = s1 * s1, s2 * s2, s1 * cor * s2
    L11 = np.sqrt(S11)
    L21 = S21 / L11
    L22 = np.sqrt(S22 - L21 * L21)
    z1 = r1 / L11
    z2 = (r2 - L21 * z1) / L22
    return -(2.0 * (np.log(L11) + np.log(L22)) + 2.0 * LOG2PI) / 2.0 - (z1 * z1 + z2 * z2) / 2.0


def tables_loglike(obs_tables, models, nuis=None):
    """ll [W] of RADEC (+cor) / SEPPA / RV_ABS / RV_REL tables from their model values (`models`: table_models' or simulate_tables' lists)."""
    W = next(iter(models[0].values())).shape[1]
    ll = np.zeros(W)
    for io, (t, m) in enumerate(zip(obs_tables, models)):
        kind = int(t["kind"])
        nu = None if nuis is None else nuis[io * 3:(io + 1) * 3]
        col = lambda k: np.asarray(t[k], dtype=np.float64)[:, None]      # noqa: E731
        if kind in (capi.ASTROM_RADEC, capi.ASTROM_SEPPA):
            jitter = np.zeros(W) if nu is None else nu[capi.NU_JITTER]
            platescale = np.ones(W) if nu is None else nu[capi.NU_PLATESCALE]
            northangle = np.zeros(W) if nu is None else nu[capi.NU_NORTHANGLE]
            if kind == capi.ASTROM_SEPPA:
                pa_diff = np.fmod((col("y1") + northangle[None, :]) - m["pa"] + np.pi, 2.0 * np.pi) - np.pi
                r1 = np.where(pa_diff < -np.pi, pa_diff + 2.0 * np.pi, pa_diff)
                r2 = platescale[None, :] * col("y2") - m["sep"]
            else:
                pa_dat = np.arctan2(col("y2"), col("y1")) - northangle[None, :]
                sep_dat = platescale[None, :] * np.hypot(col("y2"), col("y1"))
                r1 = sep_dat * np.cos(pa_dat) - m["ra"]
                r2 = sep_dat * np.sin(pa_dat) - m["dec"]
            s1 = np.where(jitter[None, :] == 0.0, col("s1"), np.hypot(jitter[None, :], col("s1")))
            s2 = np.where(jitter[None, :] == 0.0, col("s2"), np.hypot(jitter[None, :], col("s2")))
            lp = _logpdf_dense2(s1, s2, col("cor"), r1, r2) if t.get("cor") is not None else _logpdf_diag2(s1, s2, r1, r2)
            ll = ll + lp.sum(axis=0)
        elif kind in (capi.RV_ABS, capi.RV_REL):
            jitter = np.zeros(W) if nu is None else nu[capi.NU_RV_JITTER]
            resid = col("y1") - m["rv"]
            var = jitter[None, :] ** 2 + col("s1") ** 2
            ll = ll + (-(np.log(var).sum(axis=0) + len(t["epoch"]) * LOG2PI) / 2.0 - (resid * resid / var).sum(axis=0) / 2.0)
        else:
            raise ValueError(f"tables_loglike: kind {kind} is not covered")
    return ll


def two_planet_system(seed=11, W=48, spread=None, noise=True):
    """Two Visual planets with masses and four tables: RADEC + cor on planet 1, SEPPA on planet 0, RV_ABS with the trend basis epoch − 57000,
    RV_REL on planet 1; every nuisance non-trivial. spread=None: W random walkers, e up to 0.95, either planet may be the inner one;
    spread=x: walkers within a relative x of the truth walker the data are drawn from (so that |ll| stays moderate).
    Returns (obs_tables, planets, elems [18, W], nuis [12, W], truth column)."""
    rng = np.random.default_rng(seed)
    planets = [dict(orbit_kind=capi.ORBIT_VISUAL_KEP, has_mass=1), dict(orbit_kind=capi.ORBIT_VISUAL_KEP, has_mass=1)]
    truth = np.array([5.0, 0.3, 1.0, 0.7, 2.1, 58100.0, 1.2, 45.0, 8.0,
                      9.0, 0.15, 1.05, 4.0, 2.0, 59900.0, 1.2, 45.0, 12.0])
    nu_truth = np.array([0.5, 1.002, 0.003, 0.3, 1.001, -0.002, 12.0, 3.0, 0.004, -7.0, 2.0, 0.002])
    ep = [np.sort(rng.uniform(57000, 60000, n)) for n in (12, 10, 25, 8)]
    tabs = [dict(kind=capi.ASTROM_RADEC, planet=1, epoch=ep[0], cor=rng.uniform(-0.5, 0.5, 12)),
            dict(kind=capi.ASTROM_SEPPA, planet=0, epoch=ep[1], cor=None),
            dict(kind=capi.RV_ABS, planet=-1, epoch=ep[2], cor=None, extra=ep[2] - 57000.0),
            dict(kind=capi.RV_REL, planet=1, epoch=ep[3], cor=None, extra=None)]
    for t in tabs:
        n = len(t["epoch"])
        t.update(y1=np.zeros(n), y2=np.zeros(n) if t["kind"] < 2 else None, s1=None, s2=None)
        t.setdefault("extra", None)
    tabs[0].update(s1=rng.uniform(1.0, 3.0, 12), s2=rng.uniform(1.0, 3.0, 12))
    tabs[1].update(s1=rng.uniform(0.002, 0.006, 10), s2=rng.uniform(1.0, 3.0, 10))
    tabs[2].update(s1=rng.uniform(3.0, 6.0, 25))
    tabs[3].update(s1=rng.uniform(20.0, 60.0, 8))
    m = table_models(tabs, planets, truth[:, None], nu_truth[:, None])
    z = (lambda n: rng.standard_normal(n)) if noise else (lambda n: np.zeros(n))
    # the DATA: the model with the platescale / northangle of the truth undone (they act on the data), plus noise
    ra, dec = m[0]["ra"][:, 0] + tabs[0]["s1"] * z(12), m[0]["dec"][:, 0] + tabs[0]["s2"] * z(12)
    pa_d, sep_d = np.arctan2(dec, ra) + nu_truth[2], np.hypot(ra, dec) / nu_truth[1]
    tabs[0].update(y1=sep_d * np.cos(pa_d), y2=sep_d * np.sin(pa_d))
    tabs[1].update(y1=m[1]["pa"][:, 0] - nu_truth[5] + tabs[1]["s1"] * z(10), y2=(m[1]["sep"][:, 0] + tabs[1]["s2"] * z(10)) / nu_truth[4])
    tabs[2].update(y1=m[2]["rv"][:, 0] + tabs[2]["s1"] * z(25))
    tabs[3].update(y1=m[3]["rv"][:, 0] + tabs[3]["s1"] * z(8))
    if spread is None:
        el = np.empty((18, W))
        for p in range(2):
            el[p * 9 + 0] = rng.uniform(3.0, 12.0, W); el[p * 9 + 1] = rng.uniform(0.0, 0.95, W); el[p * 9 + 2] = rng.uniform(0.1, 3.0, W)
            el[p * 9 + 3] = rng.uniform(-np.pi, 2 * np.pi, W); el[p * 9 + 4] = rng.uniform(0, 2 * np.pi, W); el[p * 9 + 5] = rng.uniform(56000, 61000, W)
            el[p * 9 + 8] = rng.uniform(1.0, 30.0, W)
        el[6] = el[15] = rng.uniform(0.8, 1.6, W); el[7] = el[16] = rng.uniform(20.0, 60.0, W)
        nu = nu_truth[:, None] * rng.uniform(0.5, 1.5, (12, W))
        nu[[1, 4]] = rng.uniform(0.99, 1.01, (2, W))
    else:
        el = truth[:, None] * (1.0 + spread * rng.uniform(-1.0, 1.0, (18, W)))
        el[15], el[16] = el[6], el[7]
        nu = nu_truth[:, None] * (1.0 + spread * rng.uniform(-1.0, 1.0, (12, W)))
        el[:, 0], nu[:, 0] = truth, nu_truth
    return tabs, planets, np.ascontiguousarray(el), np.ascontiguousarray(nu), truth


def channel_scales(planets, elems, channels, prims, consts=None):
    """[C, W]: the natural scale of each channel per walker — that of the channel's planet; for RV_STAR the sum of the reflex amplitudes."""
    off, vel = natural_scales(planets, elems, prims)
    mu = mass_ratio(planets, elems, consts)
    out = np.empty((len(channels), elems.shape[1]))
    for c, (q, pl) in enumerate(channels):
        if q == predict.RV_STAR:
            out[c] = (mu * vel).sum(axis=0)
        elif q in (predict.RADVEL, predict.RV_REL):
            out[c] = vel[pl]
        else:
            out[c] = off[pl]
    return out


def channel_errors(planets, elems, epochs, channels, cube, add0=None, add1=None, basis=None, consts=None):
    """{quantity name: max over (epoch, walker) of |cube - reference| / scale}; a position angle is compared as the angle difference wrapped
    into (-pi, pi], weighted by rho / scale. Returns (errors, reference cube)."""
    prims = primitives(planets, elems, epochs, consts)
    ref = channel_values(planets, elems, epochs, channels, add0, add1, basis, consts, prims)
    scale = channel_scales(planets, elems, channels, prims, consts)
    errs = {}
    for c, (q, pl) in enumerate(channels):
        d = np.asarray(cube[c]) - ref[c]
        if q in (predict.PA, predict.ASTROM_PA):
            sep_q = predict.SEP if q == predict.PA else predict.ASTROM_SEP
            rho = channel_values(planets, elems, epochs, [(sep_q, pl)], consts=consts, prims=prims)[0]
            d = (np.pi - np.mod(np.pi - d, 2.0 * np.pi)) * rho
        e = float(np.max(np.abs(d) / scale[c][None, :]))
        name = predict.QUANTITY_NAMES[q]
        errs[name] = max(errs.get(name, 0.0), e if np.isfinite(e) else np.inf)
    return errs, ref


def random_elements(planets, W, seed, e_max=0.999):
    """[P*9, W] valid element rows for any mix of orbit kinds; e spans 0 ... e_max with both ends present; M and plx shared by the planets."""
    rng = np.random.default_rng(seed)
    P = len(planets)
    el = np.empty((P * 9, W))
    Mt, plx = rng.uniform(0.6, 2.0, W), rng.uniform(10.0, 80.0, W)
    for p, pl in enumerate(planets):
        r = el[p * 9:(p + 1) * 9]
        r[0] = rng.uniform(1.0, 30.0, W); r[1] = rng.uniform(0.0, e_max, W); r[2] = rng.uniform(0.0, np.pi, W)
        r[3] = rng.uniform(-2 * np.pi, 2 * np.pi, W); r[4] = rng.uniform(-np.pi, 3 * np.pi, W); r[5] = rng.uniform(50000.0, 60000.0, W)
        r[6] = Mt; r[7] = plx; r[8] = rng.uniform(0.5, 40.0, W)
        r[1, 0] = 0.0
        if W > 1:
            r[1, 1] = e_max
        if pl["orbit_kind"] == capi.ORBIT_THIELE_INNES:
            for k in (0, 2, 3, 4):
                r[k] = rng.uniform(-300.0, 300.0, W)
    return np.ascontiguousarray(el)
