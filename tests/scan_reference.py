"""
An independent restatement of the along-scan absolute-astrometry likelihood of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, "The
seventeenth"; csrc/draws/octo_draws_scan.hip), in mpmath at 50 digits. A plain module, not a conftest and not a test module.

  Table    row i: t_i [MJD], (u_i, v_i), y_i [mas], σ_i > 0 [mas], c_i[0 … K − 1]
  Model    R_p(t) = f_p·(raoff_p(t), decoff_p(t)), f_p = −mass_p·mjup2msol/M_p (0 with has_mass = 0); visual planets only (Visual{KepOrbit} and
           ThieleInnesOrbit); η_i = Σ_k c_i[k]·β_k + Σ_p (u_i·R_p,α(t_i) + v_i·R_p,δ(t_i)); r_i = y_i − η_i; w_i = 1/(σ_i² + s²);
           ℓ = Σ_i (−½·w_i·r_i² + ½·log w_i − ½·log 2π)
  Marginal A = Σ w c cᵀ, b = Σ w c (y − reflex), β̂ = A⁻¹b, ℓ_marg = ℓ(β̂) + (K/2)·log 2π − ½·log det A

Written differently from the device: Kepler's equation by Newton's iteration to convergence (not Markley's starter and correction), the positions in
the textbook form X = cos E − e, Y = √(1 − e²)·sin E against the Thiele-Innes constants, a ThieleInnesOrbit's semi-major axis from the reference's
α² = u + √(u² − v²), and the gradient in FORWARD mode — ∂η_i/∂(every input) per row, then Σ_i w_i r_i·∂η_i — where the device runs reverse mode through
running sums. tests/test_scan_reference.py holds it to scipy and to mp central differences.
"""
import mpmath as mp
import numpy as np

DPS = 50      # every function here works at this precision whatever the caller's (mp.workdps): other modules of the suite set mpmath's global one

MAX_K = 6
SAMPLED, MARGINAL = 0, 1
VISUAL_KEP, RADVEL, THIELE_INNES, KEP = 0, 1, 2, 3
N_EL = 9
EL_A, EL_E, EL_I, EL_W, EL_O, EL_TP, EL_M, EL_PLX, EL_MASS = range(9)
TI_A, TI_B, TI_F, TI_G = 0, 2, 3, 4
# octo_consts_default
with mp.workdps(DPS):
    K_YR = mp.mpf("365.2568983840419")
    MAS_PER_AU_PER_PLX = mp.mpf(1)          # rad2as/pc2au
    MJUP2MSOL = mp.mpf("0.0009545942339693249")
    TWO_PI = 2 * mp.pi


def kepler_newton(MA, e):
    """E with E − e·sin E = MA (reduced to (−π, π]), Newton's iteration until the step is below 1e-45"""
    M = MA - TWO_PI * mp.nint(MA / TWO_PI)
    E = M + e * mp.sin(M) if e < mp.mpf("0.8") else (mp.pi if M >= 0 else -mp.pi)
    for _ in range(200):
        d = (E - e * mp.sin(E) - M) / (1 - e * mp.cos(E))
        E -= d
        if abs(d) < mp.mpf("1e-45"):
            return E
    raise RuntimeError("kepler_newton did not converge")


def contributes(planet):
    kind, has_mass = planet
    return kind in (VISUAL_KEP, THIELE_INNES) and bool(has_mass)


def valid_elements(el, planet):
    """the main library's element domain (setup_valid): every element the orbit kind reads finite, 0 <= e < 1, a > 0, M > 0, plx > 0"""
    kind, has_mass = planet
    radvel, ti, kep = kind == RADVEL, kind == THIELE_INNES, kind == KEP
    x = [el[EL_A], el[EL_E], el[EL_W], el[EL_TP], el[EL_M]]
    if not radvel:
        x += [el[EL_I], el[EL_O]]
    if not (radvel or kep):
        x.append(el[EL_PLX])
    if has_mass:
        x.append(el[EL_MASS])
    if not all(np.isfinite(float(v)) for v in x):
        return False
    plx = 1.0 if (radvel or kep) else float(el[EL_PLX])
    if ti:
        A, B, F, G = (float(el[k]) for k in (TI_A, TI_B, TI_F, TI_G))
        sma_ok = (A * A + B * B + F * F + G * G) > 0 and plx > 0
    else:
        sma_ok = float(el[EL_A]) > 0
    return 0.0 <= float(el[EL_E]) < 1.0 and sma_ok and float(el[EL_M]) > 0 and plx > 0


def reflex_row(el, planet, t, u, v, grad):
    """(u·R_α + v·R_δ at epoch t of one planet, its nine partials w.r.t. the planet's element rows or None), in mp"""
    kind, _ = planet
    el = [mp.mpf(float(x)) for x in el]
    e, tp, Mt, plx, mass = el[EL_E], el[EL_TP], el[EL_M], el[EL_PLX], el[EL_MASS]
    ti = kind == THIELE_INNES
    d_sma = [mp.mpf(0)] * N_EL      # ∂a/∂(element rows)
    if ti:
        A, B, F, G = el[TI_A], el[TI_B], el[TI_F], el[TI_G]
        uu, vv = (A * A + B * B + F * F + G * G) / 2, A * G - B * F
        root = mp.sqrt(uu * uu - vv * vv)
        alpha = mp.sqrt(uu + root)
        sma, T = alpha / plx, mp.mpf(1)
        if grad:
            # α² = u + √(u² − v²): dα = (du + (u·du − v·dv)/root)/(2α); at root = 0 (face-on, circular basis) the limit is du/(2α)
            du = {TI_A: A, TI_B: B, TI_F: F, TI_G: G}
            dv = {TI_A: G, TI_B: -F, TI_F: -B, TI_G: A}
            for k in (TI_A, TI_B, TI_F, TI_G):
                d_sma[k] = (du[k] + ((uu * du[k] - vv * dv[k]) / root if root != 0 else 0)) / (2 * alpha) / plx
            d_sma[EL_PLX] = -sma / plx
    else:
        sma, inc, om, Om = el[EL_A], el[EL_I], el[EL_W], el[EL_O]
        si, ci, sw, cw, sO, cO = mp.sin(inc), mp.cos(inc), mp.sin(om), mp.cos(om), mp.sin(Om), mp.cos(Om)
        A, B = cO * cw - sO * sw * ci, sO * cw + cO * sw * ci
        F, G = -cO * sw - sO * cw * ci, -sO * sw + cO * cw * ci
        T = sma * plx * MAS_PER_AU_PER_PLX
        d_sma[EL_A] = mp.mpf(1)
    P_d = K_YR * mp.sqrt(sma ** 3 / Mt)
    n_mot = TWO_PI / P_d
    MA = n_mot * (mp.mpf(float(t)) - tp)
    E = kepler_newton(MA, e)
    sE, cE, beta = mp.sin(E), mp.cos(E), mp.sqrt(1 - e * e)
    X, Y = cE - e, beta * sE
    u, v = mp.mpf(float(u)), mp.mpf(float(v))
    c1, c2 = u * B + v * A, u * G + v * F
    q = T * (c1 * X + c2 * Y)
    f = -mass * MJUP2MSOL / Mt
    if not grad:
        return f * q, None
    D = 1 - e * cE
    q_E = T * (-c1 * sE + c2 * beta * cE) / D      # ∂q/∂MA
    dq = [mp.mpf(0)] * N_EL
    # through the mean anomaly: MA = 2π(t − tp)/P_d, P_d ∝ a^{3/2}·M^{−1/2}
    for k in range(N_EL):
        dq[k] += q_E * (-mp.mpf(3) / 2 * MA / sma) * d_sma[k]
    dq[EL_M] += q_E * MA / (2 * Mt)
    dq[EL_TP] += -q_E * n_mot
    dq[EL_E] += q_E * sE + T * (-c1 - c2 * (e / beta) * sE)
    if ti:
        dq[TI_A] += v * X; dq[TI_B] += u * X; dq[TI_F] += v * Y; dq[TI_G] += u * Y
    else:
        dq[EL_A] += q / sma
        dq[EL_PLX] += q / plx
        dA = {EL_I: sO * sw * si, EL_W: F, EL_O: -B}
        dB = {EL_I: -cO * sw * si, EL_W: G, EL_O: A}
        dF = {EL_I: sO * cw * si, EL_W: -A, EL_O: -G}
        dG = {EL_I: -cO * cw * si, EL_W: -B, EL_O: F}
        for k in (EL_I, EL_W, EL_O):
            dq[k] += T * ((u * dB[k] + v * dA[k]) * X + (u * dG[k] + v * dF[k]) * Y)
    dR = [f * x for x in dq]
    dR[EL_MASS] += -MJUP2MSOL / Mt * q
    dR[EL_M] += -f / Mt * q
    return f * q, dR


def _walker(tab, planets, el, beta, s, mode, grad):
    """one walker in mp: dict(ll, eta [n], g_elems [P·9], g_beta [K], g_jitter, beta_hat [K]) of mp numbers (None where not formed)"""
    n, K, P = len(tab["t"]), tab["c"].shape[0], len(planets)
    refl = [mp.mpf(0)] * n
    drefl = [[mp.mpf(0)] * (P * N_EL) for _ in range(n)] if grad else None
    for p, pl in enumerate(planets):
        if not contributes(pl):
            continue
        for i in range(n):
            r, dr = reflex_row(el[p * N_EL:(p + 1) * N_EL], pl, tab["t"][i], tab["u"][i], tab["v"][i], grad)
            refl[i] += r
            if grad:
                drefl[i][p * N_EL:(p + 1) * N_EL] = dr
    s = mp.mpf(float(s))
    w = [1 / (mp.mpf(float(sg)) ** 2 + s * s) for sg in tab["sigma"]]
    c = [[mp.mpf(float(tab["c"][k, i])) for k in range(K)] for i in range(n)]
    y = [mp.mpf(float(x)) for x in tab["y"]]
    out = dict(beta_hat=None, g_beta=None)
    Ainv = None
    if mode == MARGINAL:
        A = mp.matrix(K, K)
        b = mp.matrix(K, 1)
        for i in range(n):
            for a_ in range(K):
                b[a_] += w[i] * c[i][a_] * (y[i] - refl[i])
                for b_ in range(K):
                    A[a_, b_] += w[i] * c[i][a_] * c[i][b_]
        bh = mp.lu_solve(A, b)
        beta = [bh[k] for k in range(K)]
        out["beta_hat"] = beta
        Ainv = A ** -1
    else:
        beta = [mp.mpf(float(x)) for x in beta]
    eta = [refl[i] + sum((c[i][k] * beta[k] for k in range(K)), mp.mpf(0)) for i in range(n)]
    r = [y[i] - eta[i] for i in range(n)]
    ll = sum((-w[i] * r[i] ** 2 / 2 + mp.log(w[i]) / 2 - mp.log(TWO_PI) / 2 for i in range(n)), mp.mpf(0))
    if mode == MARGINAL:
        ll += mp.mpf(K) / 2 * mp.log(TWO_PI) - mp.log(mp.det(A)) / 2
    out.update(ll=ll, eta=eta)
    if grad:
        out["g_elems"] = [sum((w[i] * r[i] * drefl[i][k] for i in range(n)), mp.mpf(0)) for k in range(P * N_EL)]
        gs = s * sum((w[i] ** 2 * r[i] ** 2 - w[i] for i in range(n)), mp.mpf(0))
        if mode == MARGINAL:
            gs += s * sum((w[i] ** 2 * (mp.matrix([c[i]]) * Ainv * mp.matrix([c[i]]).T)[0] for i in range(n)), mp.mpf(0))
        else:
            out["g_beta"] = [sum((w[i] * r[i] * c[i][k] for i in range(n)), mp.mpf(0)) for k in range(K)]
        out["g_jitter"] = gs
    return out


def table(t, u, v, y, sigma, columns=None):
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    c = np.zeros((0, t.size)) if columns is None else np.asarray(columns, dtype=np.float64).reshape(-1, t.size)
    return dict(t=t, u=np.asarray(u, dtype=np.float64), v=np.asarray(v, dtype=np.float64), y=np.asarray(y, dtype=np.float64),
                sigma=np.asarray(sigma, dtype=np.float64), c=c)


def evaluate(tab, planets, elems, beta=None, jitter=None, mode=SAMPLED, grad=True, mp_out=False):
    with mp.workdps(DPS):
        return _evaluate(tab, planets, elems, beta, jitter, mode, grad, mp_out)


def _evaluate(tab, planets, elems, beta, jitter, mode, grad, mp_out):
    """The restated function on W walkers: elems [P·9, W], beta [K, W] (sampled), jitter [W] or None = 0. Float64 arrays
    dict(ll [W], eta [n, W], g_elems [P·9, W], g_beta [K, W], g_jitter [W], beta_hat [K, W]); an invalid walker has ℓ = −Inf, a zero gradient
    and NaN η. mp_out: the mp numbers themselves, one dict a walker."""
    elems = np.asarray(elems, dtype=np.float64)
    P, K, n = len(planets), tab["c"].shape[0], tab["t"].size
    elems = elems.reshape(P * N_EL, -1)
    W = elems.shape[1]
    beta = np.zeros((K, W)) if beta is None else np.asarray(beta, dtype=np.float64).reshape(K, W)
    jitter = np.zeros(W) if jitter is None else np.asarray(jitter, dtype=np.float64).reshape(W)
    res = dict(ll=np.full(W, -np.inf), eta=np.full((n, W), np.nan), g_elems=np.zeros((P * N_EL, W)), g_beta=np.zeros((K, W)), g_jitter=np.zeros(W),
               beta_hat=np.full((K, W), np.nan))
    raw = []
    for w in range(W):
        el = elems[:, w]
        ok = np.isfinite(jitter[w]) and jitter[w] >= 0 and (mode == MARGINAL or np.all(np.isfinite(beta[:, w])))
        ok = ok and all(valid_elements(el[p * N_EL:(p + 1) * N_EL], planets[p]) for p in range(P))
        if not ok:
            raw.append(None)
            continue
        o = _walker(tab, planets, el, beta[:, w], jitter[w], mode, grad)
        raw.append(o)
        res["ll"][w] = float(o["ll"])
        res["eta"][:, w] = [float(x) for x in o["eta"]]
        if o["beta_hat"] is not None:
            res["beta_hat"][:, w] = [float(x) for x in o["beta_hat"]]
        if grad:
            res["g_elems"][:, w] = [float(x) for x in o["g_elems"]]
            res["g_jitter"][w] = float(o["g_jitter"])
            if o["g_beta"] is not None:
                res["g_beta"][:, w] = [float(x) for x in o["g_beta"]]
    return raw if mp_out else res


# ---- the column builders of host/observations.py, restated (the conventions are recalled: van Leeuwen 2007 IAD fields; Gaia's scan angle from north)
def hipparcos_columns(epoch_yr, parf, cpsi, spsi, res, plx, pmra, pmdec, ref_epoch=1991.25):
    """(t_mjd, u, v, y, columns [5, n]) of Hipparcos IAD rows: y = RES + PARF·ϖ + CPSI·Δt·μα* + SPSI·Δt·μδ, columns ↔ (Δα*, Δδ, ϖ, μα*, μδ)"""
    epoch_yr, parf, cpsi, spsi, res = (np.asarray(x, dtype=np.float64) for x in (epoch_yr, parf, cpsi, spsi, res))
    dt = epoch_yr - ref_epoch
    y = res + parf * plx + cpsi * dt * pmra + spsi * dt * pmdec
    t = (epoch_yr - 2000.0) * 365.25 + 51544.5
    return t, cpsi, spsi, y, np.stack([cpsi, spsi, parf, cpsi * dt, spsi * dt])
