"""
Two restatements of the Gaussian-process radial-velocity likelihood under DENSE kernels (include/octofitter_hip_draws.h, "The twentieth";
csrc/draws/octo_draws_gpd.hip). A plain module, not a conftest and not a test module.

  dense        mpmath at 50 digits, tests/gp_reference.py's dense normal with the five dense kinds: K written out from the kernels' formulas, its Cholesky
               factor, ℓ, α = K⁻¹r and ½αᵀ(∂K)α − ½tr(K⁻¹∂K), ∂K by complex steps of 1e-30. The model values η and ∂η/∂elements are gp_reference's
               (Newton's Kepler solve, the textbook radial velocity, complex steps).
  numpy_dense  float64 NumPy: the closed-form ∂k/∂h, a LAPACK Cholesky, K⁻¹ and the contraction with G = ααᵀ − K⁻¹. It takes η and ∂η/∂elements from the
               same mpmath helpers (rounded to float64), so it restates the linear algebra and the kernels' derivatives and nothing else. mpmath cannot
               afford K⁻¹ at n ≈ 200-260: the long tables are judged against this one, which tests/test_gpd_reference.py holds to the first at 1e-10.
"""
import mpmath as mp
import numpy as np

import gp_reference as gref
import scan_reference as sref

SE, MATERN32, MATERN52, PERIODIC, QUASIPERIODIC = 16, 17, 18, 19, 20
N_HYPER = {SE: 2, MATERN32: 2, MATERN52: 2, PERIODIC: 3, QUASIPERIODIC: 4}      # (a, ℓ) · (a, ℓ) · (a, ℓ) · (a, P, r) · (a, ℓ, P, r)
LDS_ROWS, MAX_N, MAX_TERMS = 192, 2048, 4      # OCTO_DRAWS_GP_DENSE_LDS_ROWS, _DENSE_MAX_N, OCTO_DRAWS_GP_MAX_TERMS
N_EL = gref.N_EL
STEPPED = (gref.EL_A, gref.EL_E, gref.EL_I, gref.EL_W, gref.EL_TP, gref.EL_M, gref.EL_MASS)


def n_hyper(terms):
    return sum(N_HYPER[k] for k in terms)


def kernel_value(kind, h, tau):
    """k(τ) of one term, mp (real or complex h): KernelFunctions.jl's definitions under ScaleTransform(1/ℓ) and ScaleTransform(1/P), times a²"""
    a2 = h[0] * h[0]
    if kind == SE:
        return a2 * mp.exp(-tau * tau / (2 * h[1] * h[1]))
    if kind == MATERN32:
        u = mp.sqrt(3) * tau / h[1]
        return a2 * (1 + u) * mp.exp(-u)
    if kind == MATERN52:
        u = mp.sqrt(5) * tau / h[1]
        return a2 * (1 + u + u * u / 3) * mp.exp(-u)
    if kind == PERIODIC:
        return a2 * mp.exp(-mp.sin(mp.pi * tau / h[1]) ** 2 / (2 * h[2] * h[2]))
    if kind == QUASIPERIODIC:
        return a2 * mp.exp(-tau * tau / (2 * h[1] * h[1]) - mp.sin(mp.pi * tau / h[2]) ** 2 / (2 * h[3] * h[3]))
    raise ValueError(kind)


def kernel_np(kind, h, tau):
    """(k, [∂k/∂h …]) of one term at τ (an array), float64, the closed forms of the header"""
    a, a2 = h[0], h[0] * h[0]
    if kind == SE:
        q = tau / h[1]
        E = np.exp(-0.5 * q * q)
        return a2 * E, [2 * a * E, a2 * E * q * q / h[1]]
    if kind == MATERN32:
        u = np.sqrt(3.0) * tau / h[1]
        e = np.exp(-u)
        return a2 * (1 + u) * e, [2 * a * (1 + u) * e, a2 * u * u * e / h[1]]
    if kind == MATERN52:
        u = np.sqrt(5.0) * tau / h[1]
        e = np.exp(-u)
        return a2 * (1 + u + u * u / 3) * e, [2 * a * (1 + u + u * u / 3) * e, a2 * u * u * (1 + u) * e / (3 * h[1])]
    if kind == PERIODIC:
        P, r = h[1], h[2]
        sn, cs = np.sin(np.pi * tau / P), np.cos(np.pi * tau / P)
        E = np.exp(-0.5 * (sn / r) ** 2)
        k = a2 * E
        return k, [2 * a * E, k * sn * cs * np.pi * tau / (P * P * r * r), k * sn * sn / r ** 3]
    if kind == QUASIPERIODIC:
        ell, P, r = h[1], h[2], h[3]
        sn, cs = np.sin(np.pi * tau / P), np.cos(np.pi * tau / P)
        q = tau / ell
        E = np.exp(-0.5 * (q * q + (sn / r) ** 2))
        k = a2 * E
        return k, [2 * a * E, k * q * q / ell, k * sn * cs * np.pi * tau / (P * P * r * r), k * sn * sn / r ** 3]
    raise ValueError(kind)


def valid_hyper(terms, hyper):
    """finite, a² finite, every length, period and width > 0"""
    if not np.all(np.isfinite(hyper)):
        return False
    o = 0
    for kind in terms:
        h = hyper[o:o + N_HYPER[kind]]
        o += N_HYPER[kind]
        with np.errstate(over="ignore"):
            if not np.isfinite(h[0] * h[0]) or not np.all(h[1:] > 0):
                return False
    return True


def valid_walker(tab, terms, planets, el, hyper, beta, s):
    ok = np.isfinite(s) and s >= 0 and np.all(np.isfinite(beta)) and valid_hyper(terms, hyper)
    return bool(ok and all(sref.valid_elements(el[p * N_EL:(p + 1) * N_EL], planets[p]) for p in range(len(planets))))


def model_values(tab, planets, el, beta, grad):
    """η [n] and ∂η/∂elements [n][P·9] of one walker, mp: gp_reference's helpers"""
    n, K, P = tab["t"].size, tab["c"].shape[0], len(planets)
    t = [mp.mpf(float(x)) for x in tab["t"]]
    elm = [mp.mpf(float(x)) for x in el]
    eta = [sum((mp.mpf(float(tab["c"][k, i])) * mp.mpf(float(beta[k])) for k in range(K)), mp.mpf(0)) for i in range(n)]
    deta = [[mp.mpf(0)] * (P * N_EL) for _ in range(n)]
    for p, pl in enumerate(planets):
        if not gref.contributes(pl):
            continue
        e0 = elm[p * N_EL:(p + 1) * N_EL]
        for i in range(n):
            eta[i] += gref._star_rv(e0, pl[0], t[i])
            if grad:
                for k in STEPPED:
                    if k == gref.EL_I and pl[0] == gref.RADVEL:
                        continue
                    e1 = list(e0)
                    e1[k] = mp.mpc(e0[k], gref.STEP)
                    deta[i][p * N_EL + k] = mp.im(gref._star_rv(e1, pl[0], t[i])) / gref.STEP
    return eta, deta


def _dense_walker(tab, terms, planets, el, hyper, beta, s, grad):
    n, K, P, H = tab["t"].size, tab["c"].shape[0], len(planets), n_hyper(terms)
    t = [mp.mpf(float(x)) for x in tab["t"]]
    eta, deta = model_values(tab, planets, el, beta, grad)
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
                        h1[k] = mp.mpc(h1[k], gref.STEP)
                        dK[o + k][i, j] = dK[o + k][j, i] = mp.im(kernel_value(kind, h1, tau)) / gref.STEP
                o += nh
            Kd[i, j] = Kd[j, i] = v + (white[i] if i == j else 0)
    try:
        L = mp.cholesky(Kd)
    except (ValueError, ZeroDivisionError):
        return None      # not positive definite
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


def _numpy_walker(tab, terms, planets, el, hyper, beta, s, grad):
    n, K, P, H = tab["t"].size, tab["c"].shape[0], len(planets), n_hyper(terms)
    eta_m, deta_m = model_values(tab, planets, el, beta, grad)
    eta = np.array([float(x) for x in eta_m])
    deta = np.array([[float(x) for x in row] for row in deta_m])
    r = tab["rv"] - eta
    white = tab["sigma"] ** 2 + s * s
    tau = np.abs(tab["t"][:, None] - tab["t"][None, :])
    Kd, dK, o = np.diag(white), [], 0
    for kind in terms:
        k, d = kernel_np(kind, hyper[o:o + N_HYPER[kind]], tau)
        Kd = Kd + k
        dK += d
        o += N_HYPER[kind]
    try:
        L = np.linalg.cholesky(Kd)
    except np.linalg.LinAlgError:
        return None
    y = np.linalg.solve(L, r)
    alpha = np.linalg.solve(L.T, y)
    out = dict(ll=-0.5 * y @ y - np.sum(np.log(np.diag(L))) - 0.5 * n * gref.LOG2PI, eta=eta, alpha=alpha, mu=r - white * alpha, cond=np.linalg.cond(Kd))
    if grad:
        Li = np.linalg.solve(L, np.eye(n))
        Kinv = Li.T @ Li
        G = np.outer(alpha, alpha) - Kinv
        out["g_hyper"] = [0.5 * np.sum(G * d) for d in dK]
        out["g_jitter"] = s * (alpha @ alpha - np.trace(Kinv))
        out["g_beta"] = tab["c"] @ alpha
        out["g_elems"] = deta.T @ alpha
    return out


def _over_walkers(walker, tab, terms, planets, elems, hyper, beta, jitter, grad):
    P, K, n, H = len(planets), tab["c"].shape[0], tab["t"].size, n_hyper(terms)
    elems = np.asarray(elems, dtype=np.float64).reshape(P * N_EL, -1)
    W = elems.shape[1]
    hyper = np.asarray(hyper, dtype=np.float64).reshape(H, W)
    beta = np.zeros((K, W)) if beta is None else np.asarray(beta, dtype=np.float64).reshape(K, W)
    jitter = np.zeros(W) if jitter is None else np.asarray(jitter, dtype=np.float64).reshape(W)
    res = dict(ll=np.full(W, -np.inf), eta=np.full((n, W), np.nan), alpha=np.full((n, W), np.nan), mu=np.full((n, W), np.nan), cond=np.full(W, np.nan),
               g_elems=np.zeros((P * N_EL, W)), g_hyper=np.zeros((H, W)), g_beta=np.zeros((K, W)), g_jitter=np.zeros(W))
    with mp.workdps(gref.DPS):
        for w in range(W):
            ok = valid_walker(tab, terms, planets, elems[:, w], hyper[:, w], beta[:, w], jitter[w])
            o = walker(tab, terms, planets, elems[:, w], hyper[:, w], beta[:, w], jitter[w], grad) if ok else None
            if o is None:
                continue
            res["ll"][w] = float(o["ll"])
            res["cond"][w] = float(o.get("cond", np.nan))
            for k in ("eta", "alpha", "mu"):
                res[k][:, w] = [float(x) for x in o[k]]
            if grad:
                for k in ("g_elems", "g_hyper", "g_beta"):
                    res[k][:, w] = [float(x) for x in o[k]]
                res["g_jitter"][w] = float(o["g_jitter"])
    return res


def dense(tab, terms, planets, elems, hyper, beta=None, jitter=None, grad=True):
    """The mpmath reference on W walkers: elems [P·9, W], hyper [H, W], beta [K, W], jitter [W] or None = 0. Float64 arrays dict(ll [W], eta, alpha, mu
    [n, W], g_elems [P·9, W], g_hyper [H, W], g_beta [K, W], g_jitter [W]); an invalid walker has ℓ = −Inf, zero gradients, NaN η, α, μ."""
    return _over_walkers(_dense_walker, tab, terms, planets, elems, hyper, beta, jitter, grad)


def numpy_dense(tab, terms, planets, elems, hyper, beta=None, jitter=None, grad=True):
    """The float64 restatement, the same dict and cond [W] = cond₂(K)."""
    return _over_walkers(_numpy_walker, tab, terms, planets, elems, hyper, beta, jitter, grad)
