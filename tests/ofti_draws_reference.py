"""
The OFTI rejection sampler of include/octofitter_hip_draws.h ("The sixteenth"), restated in NumPy on top of tests/hmc_reference.py's counter
generator (philox_vec, u01), prior draws (prior_sample) and rejection uniforms (rejection_uniforms). It imports nothing of the library: a table
is a dict(epochs, ra, dec, s_ra, s_dec, cor, sigma_abfg) of host arrays, k_yr the Kepler constant of the context.

    nl = nl_of(theta, tp_mode, t_ref, k_yr)                         # [5, n]: e, a, tp, M, plx
    s = solve(table, nl, k_yr)                                      # dict: ll [n] (−Inf where invalid), mu [4, n], S [n, 4, 4], chol [n, 4, 4]
    post = posterior(table, seed, index, nl, k_yr)                  # [16, n]: the rows of octo_draws_ofti_posterior_device
    r = rejection(table, priors, seed, first, N, tp_mode, t_ref, k_yr)      # the driver: index, n_accepted, max_logml, theta, nl, post, …

ℓ and μ are formed vectorised here (half a million draws a case); tests/test_ofti_draws_reference.py holds them to the oracle's restatement of
ofti_linear_solve (oracle_binding.oracle_ofti) at that function's own bar.
"""
import math

import numpy as np

import hmc_reference as ref

PURPOSE_OFTI = 13
N_OUT = 16
OUTPUTS = ("A", "B", "F", "G", "A_mean", "B_mean", "F_mean", "G_mean", "alpha", "a_ti", "i", "ω", "Ω", "P_d", "M_dyn", "logml")
CHUNK = 1 << 18
UNDECIDED = 1e-6      # a draw is undecided if |u − exp(ℓ − max)| <= UNDECIDED·exp(ℓ − max)
FACE_ON = 1e-6        # the angles of a draw with 1 − |cos i| below this are not compared


def period_days(k_yr, a, M):
    return k_yr * np.sqrt(a * a * a / M)


def nl_of(theta, tp_mode, t_ref, k_yr):
    """rows 0, 1, 3, 4 of θ as they are; row 2: tp itself (mode 0) or t_ref + τ·P_d (mode 1)"""
    nl = np.array(theta, dtype=np.float64, copy=True)
    if tp_mode:
        nl[2] = t_ref + theta[2] * period_days(k_yr, theta[1], theta[3])
    return nl


def kepler(M, e):
    """E of the mean anomaly M in [−π, π] (any shape, e broadcast): Markley's starter and fifth-order correction, then one Newton step."""
    pi2 = math.pi ** 2
    alpha = (3 * pi2 + 1.6 * math.pi * (math.pi - np.abs(M)) / (1 + e)) / (pi2 - 6)
    d = 3 * (1 - e) + alpha * e
    q = 2 * alpha * d * (1 - e) - M * M
    r = 3 * alpha * d * (d - 1 + e) * M + M ** 3
    w = (np.abs(r) + np.sqrt(q ** 3 + r * r)) ** (2.0 / 3.0)
    E = (2 * r * w / (w * w + w * q + q * q) + M) / d
    s, c = np.sin(E), np.cos(E)
    f0, f1, f2 = E - e * s - M, 1 - e * c, e * s
    f3, f4 = 1 - f1, -f2
    d3 = -f0 / (f1 - 0.5 * f0 * f2 / f1)
    d4 = -f0 / (f1 + 0.5 * d3 * f2 + d3 * d3 * f3 / 6)
    d5 = -f0 / (f1 + 0.5 * d4 * f2 + d4 * d4 * f3 / 6 + d4 ** 3 * f4 / 24)
    E = E + d5
    return E - (E - e * np.sin(E) - M) / (1 - e * np.cos(E))


def weights(tab):
    """(w_rr, w_dd, w_rd, p, q, dᵀWd, log det Σ_data) of the table: src/parameterizations.jl:359-366, 387-400"""
    sr, sd = np.asarray(tab["s_ra"], dtype=np.float64), np.asarray(tab["s_dec"], dtype=np.float64)
    rho = np.zeros_like(sr) if tab["cor"] is None else np.asarray(tab["cor"], dtype=np.float64)
    ra, dec = np.asarray(tab["ra"], dtype=np.float64), np.asarray(tab["dec"], dtype=np.float64)
    with np.errstate(all="ignore"):
        det = sr * sr * sd * sd * (1 - rho * rho)
        wrr, wdd, wrd = sd * sd / det, sr * sr / det, -rho * sr * sd / det
        p, q = wrr * ra + wrd * dec, wdd * dec + wrd * ra
        return wrr, wdd, wrd, p, q, float(np.sum(ra * p + dec * q)), float(np.sum(np.log(det)))


def design(tab, nl, k_yr):
    """x = cos E − e, y = √(1 − e²)·sin E at every (draw, epoch): [n, n_epochs] each"""
    e, a, tp, M = nl[0][:, None], nl[1][:, None], nl[2][:, None], nl[3][:, None]
    t = np.asarray(tab["epochs"], dtype=np.float64)[None, :]
    u = (t - tp) / period_days(k_yr, a, M)
    ma = 2 * math.pi * (u - np.rint(u))
    E = kepler(ma, e)
    return np.cos(E) - e, np.sqrt(1 - e * e) * np.sin(E)


def solve(tab, nl, k_yr, block=1 << 16):
    """ℓ, μ, S = DᵀWD + λI in the order (A, B, F, G) — dec = A·x + F·y, ra = B·x + G·y — and its lower Cholesky factor; ℓ = −Inf and μ = NaN for an
    element not finite, e outside [0, 1), a <= 0, M <= 0, S not positive definite or ℓ not finite (the rule of the device's finishing kernel)."""
    nl = np.asarray(nl, dtype=np.float64)
    n = nl.shape[1]
    wrr, wdd, wrd, p, q, data_quad, log_det_data = weights(tab)
    lam = 1.0 / tab["sigma_abfg"] ** 2
    n_ep = len(tab["epochs"])
    S, b = np.zeros((n, 4, 4)), np.zeros((n, 4))
    ok = np.all(np.isfinite(nl), axis=0) & (nl[0] >= 0) & (nl[0] < 1) & (nl[1] > 0) & (nl[3] > 0)
    safe = np.where(ok[None, :], nl, np.array([0.1, 1.0, 0.0, 1.0, 1.0])[:, None])
    with np.errstate(all="ignore"):
        for lo in range(0, n, block):
            sl = slice(lo, min(n, lo + block))
            x, y = design(tab, safe[:, sl], k_yr)
            xx, xy, yy = x * x, x * y, y * y
            s = S[sl]
            s[:, 0, 0], s[:, 0, 1], s[:, 0, 2], s[:, 0, 3] = xx @ wdd + lam, xx @ wrd, xy @ wdd, xy @ wrd
            s[:, 1, 1], s[:, 1, 2], s[:, 1, 3] = xx @ wrr + lam, xy @ wrd, xy @ wrr
            s[:, 2, 2], s[:, 2, 3] = yy @ wdd + lam, yy @ wrd
            s[:, 3, 3] = yy @ wrr + lam
            b[sl] = np.stack([x @ q, x @ p, y @ q, y @ p], axis=1)
        iu = np.triu_indices(4, 1)
        S[:, iu[1], iu[0]] = S[:, iu[0], iu[1]]
        good = ok & np.all(np.isfinite(S), axis=(1, 2)) & np.all(np.isfinite(b), axis=1)
        chol = np.full((n, 4, 4), np.nan)
        eye = np.eye(4)
        Sg = np.where(good[:, None, None], S, eye)
        try:
            chol_all = np.linalg.cholesky(Sg)
        except np.linalg.LinAlgError:      # some S is not positive definite: one at a time
            chol_all = np.full((n, 4, 4), np.nan)
            for k in np.nonzero(good)[0]:
                try:
                    chol_all[k] = np.linalg.cholesky(S[k])
                except np.linalg.LinAlgError:
                    good[k] = False
        chol[good] = chol_all[good]
        z = np.linalg.solve(np.where(good[:, None, None], chol_all, eye), b[:, :, None])
        mu = np.linalg.solve(np.transpose(np.where(good[:, None, None], chol_all, eye), (0, 2, 1)), z)[:, :, 0]
        post_quad = np.sum(z[:, :, 0] ** 2, axis=1)
        log_det_post_inv = 2 * np.sum(np.log(np.diagonal(np.where(good[:, None, None], chol_all, eye), axis1=1, axis2=2)), axis=1)
        ll = -0.5 * (data_quad - post_quad + log_det_post_inv - 4 * math.log(lam) + log_det_data) - n_ep * math.log(2 * math.pi)
        fin = good & np.isfinite(ll)
    return dict(ll=np.where(fin, ll, -np.inf), mu=np.where(fin[None, :], mu.T, np.nan), S=S, chol=chol, ok=fin)


def normals(seed, index):
    """z [4, n]: Φ⁻¹ of the uniforms of words 0 … 3 of counter (i, 0, 13, 0)"""
    from scipy.special import ndtri
    words = ref.philox_vec((seed, ref.KEY1), np.asarray(index, dtype=np.uint64), 0, PURPOSE_OFTI, 0)
    return ndtri(np.stack([ref.u01(w) for w in words]))


def fold_angles(wpo, wmo):
    """(ω, Ω) of ω + Ω and ω − Ω: Ω in [0, π), ω in [0, 2π)"""
    om, Om = 0.5 * (wpo + wmo), 0.5 * (wpo - wmo)
    neg, high = Om < 0, Om >= math.pi
    Om = np.where(neg, Om + math.pi, np.where(high, Om - math.pi, Om))
    om = np.where(neg, om + math.pi, np.where(high, om - math.pi, om))
    om = np.where(om < 0, om + 2 * math.pi, np.where(om >= 2 * math.pi, om - 2 * math.pi, om))
    return om, Om


def elements(x):
    """(α, cos i, i, ω, Ω) of Thiele-Innes constants x [4, n] = A, B, F, G"""
    A, B, F, G = x
    sp = np.sqrt(0.5 * ((A + G) ** 2 + (B - F) ** 2))      # √(u + v)
    sm = np.sqrt(0.5 * ((A - G) ** 2 + (B + F) ** 2))      # √(u − v)
    alpha = (sp + sm) / math.sqrt(2)
    cosi = (sp - sm) / (sp + sm)
    om, Om = fold_angles(np.arctan2(B - F, A + G), np.arctan2(-B - F, A - G))
    return alpha, cosi, np.arccos(cosi), om, Om


def thiele_innes(alpha, i, om, Om):
    """the textbook constants: what `elements` inverts"""
    cw, sw, cO, sO, ci = np.cos(om), np.sin(om), np.cos(Om), np.sin(Om), np.cos(i)
    return alpha * np.stack([cw * cO - sw * sO * ci, cw * sO + sw * cO * ci, -sw * cO - cw * sO * ci, -sw * sO + cw * cO * ci])


def draw_from(s, z):
    """x = μ + L⁻ᵀz [4, n] of solve's result and normals z [4, n]"""
    Lt = np.transpose(np.where(s["ok"][:, None, None], s["chol"], np.eye(4)), (0, 2, 1))
    y = np.linalg.solve(Lt, z.T[:, :, None])[:, :, 0]
    return s["mu"] + y.T


def posterior(tab, seed, index, nl, k_yr):
    nl = np.asarray(nl, dtype=np.float64)
    s = solve(tab, nl, k_yr)
    with np.errstate(all="ignore"):
        x = draw_from(s, normals(seed, index))
        alpha, cosi, inc, om, Om = elements(x)
        a_ti = alpha / nl[4]
        out = np.vstack([x, s["mu"], alpha, a_ti, inc, om, Om, period_days(k_yr, nl[1], nl[3]), nl[3] * (a_ti / nl[1]) ** 3, s["ll"]])
    out[:15, ~s["ok"]] = np.nan
    return out


def rejection(tab, priors, seed, first, N, tp_mode, t_ref, k_yr):
    """The driver: ℓ of draws first … first + N − 1 chunk by chunk, the accepted set, and the posterior rows of the accepted draws. Beside the
    outputs of the C call it reports what the cases' conditions are about: the undecided draws, cond(S) of the accepted, the near face-on count."""
    ll = np.empty(N)
    for lo in range(0, N, CHUNK):
        idx = np.uint64(first) + np.arange(lo, min(N, lo + CHUNK), dtype=np.uint64)
        theta, _ = ref.prior_sample(priors, seed, idx)
        ll[lo:lo + idx.size] = solve(tab, nl_of(theta, tp_mode, t_ref, k_yr), k_yr)["ll"]
    mx = float(np.max(ll))
    out = dict(ll=ll, max_logml=mx, n_accepted=0, index=np.zeros(0, dtype=np.uint64))
    if not math.isfinite(mx):
        return out
    idx_all = np.uint64(first) + np.arange(N, dtype=np.uint64)
    u = ref.rejection_uniforms(seed, idx_all)
    p = np.exp(ll - mx)
    acc = (ll != -np.inf) & (u < p)
    index = idx_all[acc]
    theta, _ = ref.prior_sample(priors, seed, index)
    nl = nl_of(theta, tp_mode, t_ref, k_yr)
    post = posterior(tab, seed, index, nl, k_yr)
    s = solve(tab, nl, k_yr)
    out.update(index=index, n_accepted=int(acc.sum()), theta=theta, nl=nl, post=post, undecided=int(np.sum(np.abs(u - p) <= UNDECIDED * p)),
               cond=np.linalg.cond(s["S"]), n_face_on=int(np.sum(1 - np.abs(np.cos(post[10])) < FACE_ON)))
    return out
