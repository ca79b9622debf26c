"""
Two restatements of the Gaussian-process radial-velocity likelihood of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, "The nineteenth";
csrc/draws/octo_draws_gp.hip). A plain module, not a conftest and not a test module.

  dense        mpmath at 50 digits: the covariance K_ij = [i = j](σ_i² + s²) + Σ_terms k(|t_i − t_j|) written out from the kernels' closed forms
               in their OWN parameters (an SHO as the damped oscillator's cos/sin or cosh/sinh form, not as celerite terms), its Cholesky factor,
               ℓ = log N(r; 0, K), α = K⁻¹r, and the gradient ½αᵀ(∂K)α − ½tr(K⁻¹∂K). ∂K and ∂η come from complex steps of 1e-30 at 50 digits, the
               model values η from a Newton solve of Kepler's equation and the textbook radial velocity. It does not contain the recursion.
  recursion    float64 NumPy over the walkers: the semiseparable recursion and its reverse pass as the device runs them — per-slot coefficients
               (a, b, c, d, rot), the state (T, q) = (S + D·W·Wᵀ, f + W·z) handed from row to row, checkpoints of it every SEGMENT rows, the
               segment's states recomputed forward and walked backward. Nothing is divided by φ.

tests/test_gp_reference.py holds the first to scipy and the second to the first.
"""
import mpmath as mp
import numpy as np

import scan_reference as sref

DPS = 50
MAX_K, MAX_TERMS, MAX_SLOTS, SEGMENT, ROWS = 4, 4, 8, 16, 8      # OCTO_DRAWS_GP_MAX_K, _MAX_TERMS, _MAX_SLOTS, _SEGMENT; OCTO_DRAWS_SCAN_ROWS
REAL, COMPLEX, SHO = 0, 1, 2
N_HYPER = {REAL: 2, COMPLEX: 4, SHO: 3}
N_SLOTS = {REAL: 1, COMPLEX: 2, SHO: 2}
VISUAL_KEP, RADVEL, THIELE_INNES, KEP = sref.VISUAL_KEP, sref.RADVEL, sref.THIELE_INNES, sref.KEP
N_EL = 9
EL_A, EL_E, EL_I, EL_W, EL_O, EL_TP, EL_M, EL_PLX, EL_MASS = range(9)
LOG2PI = float(np.log(2 * np.pi))
with mp.workdps(DPS):
    # octo_consts_default: K = 2π·year2day·au2m·sec2year · a·sin i/(P_d·√(1 − e²)) [m/s]
    K_C = 2 * mp.pi * mp.mpf("365.25") * mp.mpf("1.495978707e11") * mp.mpf("3.168808781402895e-8")
    STEP = mp.mpf("1e-30")


def n_hyper(terms):
    return sum(N_HYPER[k] for k in terms)


def n_slots(terms):
    return sum(N_SLOTS[k] for k in terms)


def contributes(planet):
    kind, has_mass = planet
    return kind in (VISUAL_KEP, RADVEL, KEP) and bool(has_mass)


def table(t, rv, sigma, columns=None):
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    c = np.zeros((0, t.size)) if columns is None else np.asarray(columns, dtype=np.float64).reshape(-1, t.size)
    return dict(t=t, rv=np.asarray(rv, dtype=np.float64), sigma=np.asarray(sigma, dtype=np.float64), c=c)


# ---------------------------------------------------------------------------------------------------- the dense reference, mp
def _kepler(MA, e):
    """E with E − e·sin E = MA for mp real or complex arguments (a complex step rides along: the function is analytic)"""
    k = mp.nint(mp.re(MA) / sref.TWO_PI)
    M = MA - sref.TWO_PI * k
    E = M + e * mp.sin(M) if mp.re(e) < mp.mpf("0.8") else (mp.pi if mp.re(M) >= 0 else -mp.pi) + 0 * M
    for _ in range(300):
        d = (E - e * mp.sin(E) - M) / (1 - e * mp.cos(E))
        E -= d
        if abs(d) < mp.mpf("1e-47"):
            return E
    raise RuntimeError("_kepler did not converge")


def _star_rv(el, kind, t):
    """f·K·V(t) [m/s] of one planet with a mass: the star's reflex velocity, textbook form through the true anomaly"""
    a, e, inc, om, tp, Mt, mass = el[EL_A], el[EL_E], el[EL_I], el[EL_W], el[EL_TP], el[EL_M], el[EL_MASS]
    P_d = sref.K_YR * mp.sqrt(a ** 3 / Mt)
    E = _kepler(sref.TWO_PI * (t - tp) / P_d, e)
    nu = 2 * mp.atan(mp.sqrt((1 + e) / (1 - e)) * mp.tan(E / 2))
    sini = mp.mpf(1) if kind == RADVEL else mp.sin(inc)
    K = K_C * a * sini / (P_d * mp.sqrt(1 - e * e))
    return -(mass * sref.MJUP2MSOL / Mt) * K * (mp.cos(nu + om) + e * mp.cos(om))


def kernel_value(kind, h, tau):
    """k(τ) of one term in its own parameters, mp (real or complex h)"""
    if kind == REAL:
        return h[0] * mp.exp(-h[1] * tau)
    if kind == COMPLEX:
        return mp.exp(-h[2] * tau) * (h[0] * mp.cos(h[3] * tau) + h[1] * mp.sin(h[3] * tau))
    S0, Q, w0 = h
    pre = S0 * w0 * Q * mp.exp(-w0 * tau / (2 * Q))
    if mp.re(Q) > mp.mpf("0.5"):
        eta = mp.sqrt(1 - 1 / (4 * Q * Q))
        return pre * (mp.cos(eta * w0 * tau) + mp.sin(eta * w0 * tau) / (2 * eta * Q))
    eta = mp.sqrt(1 / (4 * Q * Q) - 1)
    return pre * (mp.cosh(eta * w0 * tau) + mp.sinh(eta * w0 * tau) / (2 * eta * Q))


def valid_hyper(terms, hyper):
    """finite, every rate > 0 (REAL, COMPLEX: c; SHO: ω0/(2Q), with Q > 0), and an SHO off Q = ½"""
    if not np.all(np.isfinite(hyper)):
        return False
    o = 0
    for kind in terms:
        h = hyper[o:o + N_HYPER[kind]]
        o += N_HYPER[kind]
        if kind == REAL and not h[1] > 0:
            return False
        if kind == COMPLEX and not h[2] > 0:
            return False
        if kind == SHO and not (h[1] > 0 and h[1] != 0.5 and h[2] > 0):
            return False
    return True


def _dense_walker(tab, terms, planets, el, hyper, beta, s, grad):
    n, K, P, H = tab["t"].size, tab["c"].shape[0], len(planets), n_hyper(terms)
    t = [mp.mpf(float(x)) for x in tab["t"]]
    elm = [mp.mpf(float(x)) for x in el]
    eta = [sum((mp.mpf(float(tab["c"][k, i])) * mp.mpf(float(beta[k])) for k in range(K)), mp.mpf(0)) for i in range(n)]
    deta = [[mp.mpf(0)] * (P * N_EL) for _ in range(n)]
    for p, pl in enumerate(planets):
        if not contributes(pl):
            continue
        e0 = elm[p * N_EL:(p + 1) * N_EL]
        for i in range(n):
            eta[i] += _star_rv(e0, pl[0], t[i])
            if grad:
                for k in (EL_A, EL_E, EL_I, EL_W, EL_TP, EL_M, EL_MASS):
                    if k == EL_I and pl[0] == RADVEL:
                        continue
                    e1 = list(e0)
                    e1[k] = mp.mpc(e0[k], STEP)
                    deta[i][p * N_EL + k] = mp.im(_star_rv(e1, pl[0], t[i])) / STEP
    s = mp.mpf(float(s))
    hm = [mp.mpf(float(x)) for x in hyper]
    r = mp.matrix([mp.mpf(float(tab["rv"][i])) - eta[i] for i in range(n)])
    white = [mp.mpf(float(sg)) ** 2 + s * s for sg in tab["sigma"]]
    Kd = mp.matrix(n, n)
    dK = [mp.matrix(n, n) for _ in range(H)] if grad else []
    for i in range(n):
        for j in range(i + 1):
            tau = t[i] - t[j]
            o, v = 0, mp.mpf(0)
            for kind in terms:
                nh = N_HYPER[kind]
                v += kernel_value(kind, hm[o:o + nh], tau)
                if grad:
                    for k in range(nh):
                        h1 = list(hm[o:o + nh])
                        h1[k] = mp.mpc(h1[k], STEP)
                        dK[o + k][i, j] = dK[o + k][j, i] = mp.im(kernel_value(kind, h1, tau)) / STEP
                o += nh
            Kd[i, j] = Kd[j, i] = v + (white[i] if i == j else 0)
    try:
        L = mp.cholesky(Kd)
    except (ValueError, ZeroDivisionError):
        return None      # not positive definite
    for i in range(n):
        if not (mp.im(L[i, i]) == 0 and mp.re(L[i, i]) > 0):
            return None
    y = mp.lu_solve(L, r) if n > 1 else mp.matrix([r[0] / L[0, 0]])
    alpha = mp.lu_solve(L.T, y) if n > 1 else mp.matrix([y[0] / L[0, 0]])
    ll = -sum((y[i] ** 2 for i in range(n)), mp.mpf(0)) / 2 - sum((mp.log(L[i, i]) for i in range(n)), mp.mpf(0)) - mp.mpf(n) / 2 * mp.log(sref.TWO_PI)
    out = dict(ll=ll, eta=eta, alpha=[alpha[i] for i in range(n)], mu=[r[i] - white[i] * alpha[i] for i in range(n)])
    if grad:
        Kinv = Kd ** -1
        out["g_hyper"] = [sum((alpha[i] * dK[h][i, j] * alpha[j] - Kinv[i, j] * dK[h][i, j] for i in range(n) for j in range(n)), mp.mpf(0)) / 2 for h in range(H)]
        out["g_jitter"] = s * (sum((alpha[i] ** 2 for i in range(n)), mp.mpf(0)) - sum((Kinv[i, i] for i in range(n)), mp.mpf(0)))
        out["g_beta"] = [sum((alpha[i] * mp.mpf(float(tab["c"][k, i])) for i in range(n)), mp.mpf(0)) for k in range(K)]
        out["g_elems"] = [sum((alpha[i] * deta[i][k] for i in range(n)), mp.mpf(0)) for k in range(P * N_EL)]
    return out


def dense(tab, terms, planets, elems, hyper, beta=None, jitter=None, grad=True):
    """The dense reference on W walkers: elems [P·9, W], hyper [H, W], beta [K, W], jitter [W] or None = 0. Float64 arrays dict(ll [W], eta, alpha,
    mu [n, W], g_elems [P·9, W], g_hyper [H, W], g_beta [K, W], g_jitter [W]); an invalid walker has ℓ = −Inf, zero gradients, NaN η, α, μ."""
    P, K, n, H = len(planets), tab["c"].shape[0], tab["t"].size, n_hyper(terms)
    elems = np.asarray(elems, dtype=np.float64).reshape(P * N_EL, -1)
    W = elems.shape[1]
    hyper = np.asarray(hyper, dtype=np.float64).reshape(H, W)
    beta = np.zeros((K, W)) if beta is None else np.asarray(beta, dtype=np.float64).reshape(K, W)
    jitter = np.zeros(W) if jitter is None else np.asarray(jitter, dtype=np.float64).reshape(W)
    res = dict(ll=np.full(W, -np.inf), eta=np.full((n, W), np.nan), alpha=np.full((n, W), np.nan), mu=np.full((n, W), np.nan),
               g_elems=np.zeros((P * N_EL, W)), g_hyper=np.zeros((H, W)), g_beta=np.zeros((K, W)), g_jitter=np.zeros(W))
    with mp.workdps(DPS):
        for w in range(W):
            ok = np.isfinite(jitter[w]) and jitter[w] >= 0 and np.all(np.isfinite(beta[:, w])) and valid_hyper(terms, hyper[:, w])
            ok = ok and all(sref.valid_elements(elems[p * N_EL:(p + 1) * N_EL, w], planets[p]) for p in range(P))
            o = _dense_walker(tab, terms, planets, elems[:, w], hyper[:, w], beta[:, w], jitter[w], grad) if ok else None
            if o is None:
                continue
            res["ll"][w] = float(o["ll"])
            for k in ("eta", "alpha", "mu"):
                res[k][:, w] = [float(x) for x in o[k]]
            if grad:
                for k in ("g_elems", "g_hyper", "g_beta"):
                    res[k][:, w] = [float(x) for x in o[k]]
                res["g_jitter"][w] = float(o["g_jitter"])
    return res


# ---------------------------------------------------------------------------------------------------- the recursion, float64 over the walkers
def coefficients(terms, hyper):
    """per slot (a, b, c, d) [R, W], rot [R, W] (the slot is the sine partner of a complex pair) and the walkers' validity. A slot's row values are
    x = d·(t_i − t_1), (cx, sx) = rot ? (sin x, −cos x) : (cos x, sin x), Ũ = a·cx + b·sx, Ṽ = cx, φ = exp(−c·(t_i − t_{i−1})); a slot with rot = 0
    adds its a to the diagonal. An SHO is a complex pair for Q > ½ and two real slots for Q < ½, walker by walker."""
    R, W = n_slots(terms), hyper.shape[1]
    a, b, c, d = (np.zeros((R, W)) for _ in range(4))
    rot = np.zeros((R, W), dtype=bool)
    ok = np.all(np.isfinite(hyper), axis=0)
    o = r = 0
    with np.errstate(all="ignore"):
        for kind in terms:
            h = hyper[o:o + N_HYPER[kind]]
            if kind == REAL:
                a[r], c[r] = h[0], h[1]
            elif kind == COMPLEX:
                a[r] = a[r + 1] = h[0]; b[r] = b[r + 1] = h[1]; c[r] = c[r + 1] = h[2]; d[r] = d[r + 1] = h[3]
                rot[r + 1] = True
            else:
                S0, Q, w0 = h
                over = Q > 0.5
                f = np.sqrt(np.where(over, 4 * Q * Q - 1, 1 - 4 * Q * Q))
                a0, c0 = S0 * w0 * Q, w0 / (2 * Q)
                a[r] = np.where(over, a0, 0.5 * a0 * (1 + 1 / f)); a[r + 1] = np.where(over, a0, 0.5 * a0 * (1 - 1 / f))
                b[r] = b[r + 1] = np.where(over, a0 / f, 0.0)
                c[r] = np.where(over, c0, c0 * (1 - f)); c[r + 1] = np.where(over, c0, c0 * (1 + f))
                d[r] = d[r + 1] = np.where(over, c0 * f, 0.0)
                rot[r + 1] = over
            o += N_HYPER[kind]
            r += N_SLOTS[kind]
        ok = ok & np.all(np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(d) & (c > 0), axis=0)
    return a, b, c, d, rot, ok


def coefficient_adjoints(terms, hyper, ga, gb, gc, gd):
    """the chain rule from the slots' coefficient adjoints [R, W] to the terms' own parameters [H, W]"""
    g = np.zeros_like(hyper)
    o = r = 0
    with np.errstate(all="ignore"):
        for kind in terms:
            if kind == REAL:
                g[o], g[o + 1] = ga[r], gc[r]
            elif kind == COMPLEX:
                g[o], g[o + 1], g[o + 2], g[o + 3] = ga[r] + ga[r + 1], gb[r] + gb[r + 1], gc[r] + gc[r + 1], gd[r] + gd[r + 1]
            else:
                S0, Q, w0 = hyper[o:o + 3]
                over = Q > 0.5
                f = np.sqrt(np.where(over, 4 * Q * Q - 1, 1 - 4 * Q * Q))
                a0, c0 = S0 * w0 * Q, w0 / (2 * Q)
                # Q > ½: a = a0, b = a0/f, c = c0, d = c0·f, f' = 4Q/f
                A, B, C, D = ga[r] + ga[r + 1], gb[r] + gb[r + 1], gc[r] + gc[r + 1], gd[r] + gd[r + 1]
                fp = 4 * Q / f
                ab = A + B / f      # adjoint of a0
                cb = C + D * f      # adjoint of c0
                fb = -B * a0 / (f * f) + D * c0
                gS_o, gQ_o, gw_o = ab * w0 * Q, ab * S0 * w0 - cb * c0 / Q + fb * fp, ab * S0 * Q + cb / (2 * Q)
                # Q < ½: a± = ½a0(1 ± 1/f), c± = c0(1 ∓ f), f' = −4Q/f; slot r is +, slot r + 1 is −
                ab = 0.5 * (ga[r] * (1 + 1 / f) + ga[r + 1] * (1 - 1 / f))
                cb = gc[r] * (1 - f) + gc[r + 1] * (1 + f)
                fb = 0.5 * a0 * (ga[r + 1] - ga[r]) / (f * f) + c0 * (gc[r + 1] - gc[r])
                fp = -4 * Q / f
                gS_u, gQ_u, gw_u = ab * w0 * Q, ab * S0 * w0 - cb * c0 / Q + fb * fp, ab * S0 * Q + cb / (2 * Q)
                g[o], g[o + 1], g[o + 2] = np.where(over, gS_o, gS_u), np.where(over, gQ_o, gQ_u), np.where(over, gw_o, gw_u)
            o += N_HYPER[kind]
            r += N_SLOTS[kind]
    return g


class _Rows:
    """the row values of every slot: (Ũ, Ṽ, φ, cx, sx) [R, W] and the diagonal A [W] at row i"""

    def __init__(self, t, sigma, s, coef):
        self.t, self.sigma, self.s = t, sigma, s
        self.a, self.b, self.c, self.d, self.rot, _ = coef
        self.asum = np.where(self.rot, 0.0, self.a).sum(axis=0)

    def at(self, i):
        tau, dt = self.t[i] - self.t[0], self.t[i] - self.t[max(i - 1, 0)]
        x = self.d * tau
        cx, sx = np.cos(x), np.sin(x)
        cx, sx = np.where(self.rot, sx, cx), np.where(self.rot, -cx, sx)
        return self.a * cx + self.b * sx, cx, np.exp(-self.c * dt), cx, sx, self.sigma[i] ** 2 + self.s * self.s + self.asum, tau, dt


def _step(T, q, U, V, phi, A, r):
    """one row of the recursion from the state (T, q) handed to it: S, f, SU, D, Wv, z and the state handed on"""
    S = phi[:, None] * phi[None, :] * T
    f = phi * q
    SU = np.einsum("abw,bw->aw", S, U)
    D = A - np.sum(U * SU, axis=0)
    Wv = (V - SU) / D
    z = r - np.sum(U * f, axis=0)
    return S, f, SU, D, Wv, z, S + D * Wv[:, None] * Wv[None, :], f + Wv * z


def recursion(t, r, sigma, s, terms, hyper, grad=True):
    """ℓ [W], α [n, W] and, with grad, ∂ℓ/∂hyper [H, W] and ∂ℓ/∂s [W] of the residuals r [n, W] by the recursion and its reverse pass; a walker whose
    coefficients are invalid or that meets a D_i that is not > 0 and finite has ℓ = −Inf, zero gradients and NaN α. Also D_min [W]."""
    t, r, sigma, s = np.asarray(t, float), np.asarray(r, float), np.asarray(sigma, float), np.asarray(s, float)
    n, W = r.shape
    R = n_slots(terms)
    coef = coefficients(terms, hyper)
    rows = _Rows(t, sigma, s, coef)
    with np.errstate(all="ignore"):
        T, q = np.zeros((R, R, W)), np.zeros((R, W))
        ll, ok, Dmin = np.zeros(W), coef[5].copy(), np.full(W, np.inf)
        check = []
        for i in range(n):
            if i % SEGMENT == 0:
                check.append((T, q))
            U, V, phi, _, _, A, _, _ = rows.at(i)
            _, _, _, D, _, z, T, q = _step(T, q, U, V, phi, A, r[i])
            ok &= np.isfinite(D) & (D > 0)
            Dmin = np.minimum(Dmin, D)
            ll += -0.5 * z * z / D - 0.5 * np.log(D) - 0.5 * LOG2PI
        ok &= np.isfinite(ll)
        out = dict(ll=np.where(ok, ll, -np.inf), D_min=Dmin, ok=ok)
        # the reverse walk, segment by segment from the last: bT, bq are the adjoints of the state a row hands on
        bT, bq = np.zeros((R, R, W)), np.zeros((R, W))
        ga, gb, gc, gd = (np.zeros((R, W)) for _ in range(4))
        gs, alpha = np.zeros(W), np.zeros((n, W))
        for seg in reversed(range(len(check))):
            i0, i1 = seg * SEGMENT, min(n, (seg + 1) * SEGMENT)
            T, q = check[seg]
            states = []
            for i in range(i0, i1):
                states.append((T, q))
                U, V, phi, _, _, A, _, _ = rows.at(i)
                T, q = _step(T, q, U, V, phi, A, r[i])[6:]
            for i in reversed(range(i0, i1)):
                T, q = states[i - i0]
                U, V, phi, cx, sx, A, tau, dt = rows.at(i)
                S, f, SU, D, Wv, z, _, _ = _step(T, q, U, V, phi, A, r[i])
                bz = -z / D + np.sum(Wv * bq, axis=0)
                alpha[i] = -bz
                y = np.einsum("abw,bw->aw", bT, Wv)
                bD = 0.5 * z * z / (D * D) - 0.5 / D + np.sum(Wv * y, axis=0)
                bW = 2 * D * y + bq * z
                bD = bD - np.sum(bW * Wv, axis=0) / D
                bV = bW / D
                bSU = -bV - bD * U
                bU = -bz * f - bD * SU + np.einsum("abw,bw->aw", S, bSU)
                bf = bq - bz * U
                bS = bT + 0.5 * (bSU[:, None] * U[None, :] + U[:, None] * bSU[None, :])
                bphi = 2 * np.einsum("abw,bw,abw->aw", bS, phi, T) + bf * q
                bT = phi[:, None] * phi[None, :] * bS
                bq = phi * bf
                if grad:
                    gs += 2 * s * bD
                    ga += bU * cx + np.where(rows.rot, 0.0, bD)
                    gb += bU * sx
                    gd += (bU * (rows.b * cx - rows.a * sx) - bV * sx) * tau
                    gc += bphi * (-dt * phi)
        out["alpha"] = np.where(ok, alpha, np.nan)
        if grad:
            out["g_hyper"] = np.where(ok, coefficient_adjoints(terms, hyper, ga, gb, gc, gd), 0.0)
            out["g_jitter"] = np.where(ok, gs, 0.0)
    return out
