"""
An independent restatement of the catalogue proper-motion anomaly of liboctofitter_hip_draws.so (include/octofitter_hip_draws.h, "The eighteenth";
csrc/draws/octo_draws_pma.hip), in mpmath at scan_reference.DPS digits. A plain module, not a conftest and not a test module.

  Table     row i: t_i [MJD], (u_i, v_i); a projector L [Q, n]; catalogue values d [Q]; a covariance Σ [Q, Q]; a constant design H [Q, K]
  Model     ρ_i = Σ_p f_p·(u_i·raoff_p(t_i) + v_i·decoff_p(t_i)): scan_reference.reflex_row, valid_elements and contributes — the reflex rule is
            literally the scan part's; z = L·ρ, m = z + H·γ, r = d − m
  Sampled   ℓ = −½·rᵀΣ⁻¹r − ½·log det(2πΣ)
  Marginal  N = HᵀΣ⁻¹H, P_m = Σ⁻¹ − Σ⁻¹H·N⁻¹·HᵀΣ⁻¹, r = d − z, ℓ_marg = −½·rᵀP_m r − ½·log det(2πΣ) + (K/2)·log 2π − ½·log det N, γ̂ = N⁻¹HᵀΣ⁻¹r

Written differently from the device: the matrices by mp's LU inverse and determinant (not Cholesky factors), the reflex by scan_reference's Newton
iteration and textbook positions, and the gradient in FORWARD mode — ∂ρ_i/∂(every element) per row, pushed through L, then λᵀ·∂z — where the device
runs reverse mode through running sums. tests/test_pma_reference.py holds it to scipy and to mp central differences.
"""
import mpmath as mp
import numpy as np

import scan_reference as sref
from scan_reference import DPS, N_EL

MAX_Q, MAX_K = 8, 4
SAMPLED, MARGINAL = 0, 1


def table(t, u, v, L, d, cov, H=None):
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    L = np.asarray(L, dtype=np.float64).reshape(-1, t.size)
    Q = L.shape[0]
    H = np.zeros((Q, 0)) if H is None else np.asarray(H, dtype=np.float64).reshape(Q, -1)
    return dict(t=t, u=np.asarray(u, dtype=np.float64).reshape(-1), v=np.asarray(v, dtype=np.float64).reshape(-1), L=L,
                d=np.asarray(d, dtype=np.float64).reshape(Q), cov=np.asarray(cov, dtype=np.float64).reshape(Q, Q), H=H)


def _mat(a):
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a]) if a.size else mp.matrix(a.shape[0], a.shape[1])


def matrices(tab, mode):
    """(M, c, G) in mp: the mode's quadratic-form matrix, its constant, and N⁻¹HᵀΣ⁻¹ (marginal; None otherwise)"""
    Q, K = tab["H"].shape
    S = _mat(tab["cov"])
    Si = S ** -1
    c = -(Q * mp.log(2 * mp.pi) + mp.log(mp.det(S))) / 2
    if mode == SAMPLED:
        return Si, c, None
    H = _mat(tab["H"])
    N = H.T * Si * H
    G = (N ** -1) * H.T * Si
    return Si - Si * H * G, c + mp.mpf(K) / 2 * mp.log(2 * mp.pi) - mp.log(mp.det(N)) / 2, G


def _walker(tab, planets, el, gamma, mode, grad, mats):
    n, (Q, K), P = tab["t"].size, tab["H"].shape, len(planets)
    rho = [mp.mpf(0)] * n
    drho = [[mp.mpf(0)] * (P * N_EL) for _ in range(n)] if grad else None
    for p, pl in enumerate(planets):
        if not sref.contributes(pl):
            continue
        for i in range(n):
            r, dr = sref.reflex_row(el[p * N_EL:(p + 1) * N_EL], pl, tab["t"][i], tab["u"][i], tab["v"][i], grad)
            rho[i] += r
            if grad:
                drho[i][p * N_EL:(p + 1) * N_EL] = dr
    M, c, G = mats
    L = [[mp.mpf(float(x)) for x in row] for row in tab["L"]]
    z = [sum((L[q][i] * rho[i] for i in range(n)), mp.mpf(0)) for q in range(Q)]
    H = [[mp.mpf(float(x)) for x in row] for row in tab["H"]]
    g = [mp.mpf(float(x)) for x in gamma]
    m = [z[q] + sum((H[q][k] * g[k] for k in range(K)), mp.mpf(0)) for q in range(Q)]
    base = z if mode == MARGINAL else m
    r = mp.matrix([mp.mpf(float(tab["d"][q])) - base[q] for q in range(Q)])
    lam = M * r
    out = dict(ll=-(r.T * lam)[0] / 2 + c, z=z, m=m, gamma_hat=None, g_gamma=None, g_elems=None)
    if mode == MARGINAL:
        gh = G * r
        out["gamma_hat"] = [gh[k] for k in range(K)]
    else:
        out["g_gamma"] = [sum((H[q][k] * lam[q] for q in range(Q)), mp.mpf(0)) for k in range(K)]
    if grad:
        # ∂ℓ/∂x = −λᵀ·∂r/∂x … r = d − z − …, so ∂ℓ/∂x = +λᵀ·∂z/∂x = Σ_q λ_q Σ_i L[q][i]·∂ρ_i/∂x
        out["g_elems"] = [sum((lam[q] * sum((L[q][i] * drho[i][k] for i in range(n)), mp.mpf(0)) for q in range(Q)), mp.mpf(0)) for k in range(P * N_EL)]
    return out


def evaluate(tab, planets, elems, gamma=None, mode=SAMPLED, grad=True, mp_out=False):
    """The restated function on W walkers: elems [P·9, W], gamma [K, W] (sampled). Float64 arrays dict(ll [W], z, m [Q, W], g_elems [P·9, W],
    g_gamma [K, W], gamma_hat [K, W]); an invalid walker has ℓ = −Inf, a zero gradient and NaN z, m, γ̂. mp_out: the mp numbers, one dict a walker."""
    with mp.workdps(DPS):
        P, (Q, K) = len(planets), tab["H"].shape
        elems = np.asarray(elems, dtype=np.float64).reshape(P * N_EL, -1)
        W = elems.shape[1]
        gamma = np.zeros((K, W)) if gamma is None else np.asarray(gamma, dtype=np.float64).reshape(K, W)
        res = dict(ll=np.full(W, -np.inf), z=np.full((Q, W), np.nan), m=np.full((Q, W), np.nan), g_elems=np.zeros((P * N_EL, W)), g_gamma=np.zeros((K, W)),
                   gamma_hat=np.full((K, W), np.nan))
        mats = matrices(tab, mode)
        raw = []
        for w in range(W):
            el = elems[:, w]
            ok = (mode == MARGINAL or np.all(np.isfinite(gamma[:, w]))) and all(sref.valid_elements(el[p * N_EL:(p + 1) * N_EL], planets[p]) for p in range(P))
            if not ok:
                raw.append(None)
                continue
            o = _walker(tab, planets, el, gamma[:, w], mode, grad, mats)
            raw.append(o)
            res["ll"][w] = float(o["ll"])
            res["z"][:, w] = [float(x) for x in o["z"]]
            res["m"][:, w] = [float(x) for x in o["m"]]
            if o["gamma_hat"] is not None:
                res["gamma_hat"][:, w] = [float(x) for x in o["gamma_hat"]]
            if o["g_gamma"] is not None:
                res["g_gamma"][:, w] = [float(x) for x in o["g_gamma"]]
            if grad:
                res["g_elems"][:, w] = [float(x) for x in o["g_elems"]]
        return raw if mp_out else res


# ---- the builder of host/observations.py, restated by the normal equations (the host uses a pseudo-inverse)
def refit_operator(t_mjd, u, v, pf, sigma=None):
    """(F [5, n], t_ref): F = (CᵀWC)⁻¹CᵀW of C = [u, v, pf, u·τ, v·τ], τ = (t − t_ref)/365.25, t_ref the weighted mean epoch, w = 1/σ²"""
    t, u, v, pf = (np.asarray(x, dtype=np.float64) for x in (t_mjd, u, v, pf))
    w = np.ones_like(t) if sigma is None else 1.0 / np.asarray(sigma, dtype=np.float64) ** 2
    t_ref = np.sum(w * t) / np.sum(w)
    tau = (t - t_ref) / 365.25
    C = np.stack([u, v, pf, u * tau, v * tau], axis=1)
    return np.linalg.solve(C.T @ (w[:, None] * C), C.T * w[None, :]), t_ref
