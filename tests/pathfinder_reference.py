"""
NumPy restatement of Pathfinder on the L-BFGS paths, as include/octofitter_hip_draws.h states it (octo_draws_pathfinder_fit_device,
octo_draws_pathfinder_device, octo_draws_pathfinder_draw_device): the normal fit at an iterate from the chain's ring and Pathfinder diagonal,
the draw map, the ELBO and the selection. Built on lbfgs_reference (the state, slot_of, osum) and hmc_reference (the counter generator and the
u -> z map). A chain at a time: every sum over a coordinate or a pair in index order. A plain module.
"""
import math

import numpy as np

import hmc_reference as href
import lbfgs_reference as lref

MAX_D, MAX_ELBO_DRAWS = 64, 32
PURPOSE_ELBO, PURPOSE_PATHFINDER = 4, 5
LOG_2PI = math.log(2.0 * math.pi)


def pairs_of(cnt, head, S, Y, w):
    """the stored pairs of chain w, oldest first: pair k in slot (head − cnt + k) mod m"""
    m = S.shape[0]
    cnt, head = int(np.clip(cnt, 0, m)), int(head) % m
    return [(S[lref.slot_of(head, cnt - 1 - k, m), :, w], Y[lref.slot_of(head, cnt - 1 - k, m), :, w]) for k in range(cnt)]


def scaled_inverse_bfgs(pairs, alpha):
    """H̃ after the inverse-BFGS updates of I by the pairs (s/√α, y·√α), oldest first, each entry by the header's expression"""
    D, dt = len(alpha), alpha.dtype
    sa = np.sqrt(alpha)
    H = np.eye(D, dtype=dt)
    with np.errstate(all="ignore"):
        for s, y in pairs:
            st, yt = s / sa, y * sa
            w = np.zeros(D, dtype=dt)
            for j in range(D):
                w = w + H[:, j] * yt[j]
            sy, yw = lref.osum((st * yt)[:, None])[0], lref.osum((yt * w)[:, None])[0]
            rho = 1.0 / sy
            cc = rho * (1.0 + rho * yw)
            H = H - rho * (np.outer(st, w) + np.outer(w, st)) + cc * np.outer(st, st)
    return H


def cholesky(H):
    """(L̃ lower, ok): column by column, the pivot H_jj − Σ_{k<j} L_jk², the entries below (H_ij − Σ_{k<j} L_ik·L_jk)/L_jj; ok = every pivot
    finite and > 0"""
    D = H.shape[0]
    L = np.zeros_like(H)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(D):
            p = H[j, j]
            for k in range(j):
                p = p - L[j, k] * L[j, k]
            ok = ok and bool(np.isfinite(p) and p > 0)
            L[j, j] = np.sqrt(p)
            v = H[j + 1:, j].copy()
            for k in range(j):
                v = v - L[j + 1:, k] * L[j, k]
            L[j + 1:, j] = v / L[j, j]
    return L, ok


def fit_chain(pairs, x, g, alpha):
    """dict(mu, sqa, L, logdet, ok, H): N(μ, Σ) with Σ = diag(√α)·H̃·diag(√α) = T·Tᵀ, T = diag(√α)·L̃"""
    alpha = np.asarray(alpha)
    D = len(alpha)
    with np.errstate(all="ignore"):
        sa = np.sqrt(alpha)
        H = scaled_inverse_bfgs(pairs, alpha)
        t = sa * g
        u = np.zeros(D, dtype=alpha.dtype)
        for j in range(D):
            u = u + H[:, j] * t[j]
        mu = x - sa * u
        L, ok = cholesky(H)
        ok = ok and bool(np.all(np.isfinite(alpha) & (alpha > 0)))
        logdet = lref.osum(np.log(alpha)[:, None])[0] + 2.0 * lref.osum(np.log(np.diag(L))[:, None])[0]
    return dict(mu=mu, sqa=sa, L=L, logdet=logdet, ok=ok, H=H)


def sigma(f):
    return f["sqa"][:, None] * f["H"] * f["sqa"][None, :]


def pack(L):
    """L̃ packed row-major: L_ij (j <= i) at i(i+1)/2 + j"""
    return np.concatenate([L[i, :i + 1] for i in range(L.shape[0])])


def unpack(p, D):
    L = np.zeros((D, D), dtype=p.dtype)
    for i in range(D):
        L[i, :i + 1] = p[i * (i + 1) // 2: i * (i + 1) // 2 + i + 1]
    return L


def draw_map(mu, sqa, L, logdet, z):
    """(φ [D, n], log q [n]) of z [D, n]: φ = μ + √α ⊙ (L̃z), each row's sum from the left; zᵀz in index order"""
    D = len(mu)
    z = np.asarray(z).reshape(D, -1)
    Lz = np.zeros_like(z)
    for k in range(D):
        Lz = Lz + L[:, k][:, None] * z[k][None, :]      # L_ik = 0 for k > i: the terms of row i are added in index order
    zz = lref.osum(z * z)
    return mu[:, None] + sqa[:, None] * Lz, -0.5 * (D * LOG_2PI + logdet + zz)


def normals(seed, chain, D, purpose, t):
    """z [D, n] of counter (chain, d // 4, purpose, t[k]), word d % 4"""
    from scipy.special import ndtri
    t = np.atleast_1d(np.asarray(t, dtype=np.uint64))
    idx = np.full(t.shape, np.uint64(int(chain) & href.M64), dtype=np.uint64)
    return ndtri(href.block_uniforms(seed, idx, D, purpose, t))


def elbo_normals(seed, chain, D, iters, K):
    return normals(seed, chain, D, PURPOSE_ELBO, np.uint64(int(iters) * MAX_ELBO_DRAWS) + np.arange(K, dtype=np.uint64))


def final_normals(seed, chain, D, n):
    return normals(seed, chain, D, PURPOSE_PATHFINDER, np.arange(n, dtype=np.uint64))


class State:
    """What the handle holds between calls: the L-BFGS state and, per chain, the kept fit and its scalars."""

    def __init__(self, lb):
        W = lb.x.shape[1]
        self.lb = lb
        self.kept = [None] * W
        self.elbo = np.full(W, -np.inf)
        self.elbo_iter = np.full(W, -1, dtype=np.int32)
        self.n_fits = np.zeros(W, dtype=np.int32)
        self.history = [[] for _ in range(W)]      # (iters, ELBO) of every candidate, for the tests' margin


def pathfinder_round(logpost, ps, seed, chain0, n_elbo, gtol=1e-6, ftol=0.0):
    lb = ps.lb
    D, W = lb.x.shape
    before = lb.iters.copy()
    lref.lbfgs_round(logpost, lb, gtol, ftol)
    batch = np.repeat(lb.x[:, None, :], n_elbo, axis=1)      # [D, K, W]: a chain without a new fit sends its x
    logq = np.full((n_elbo, W), np.nan)
    cand = {}
    for w in np.nonzero(lb.iters != before)[0]:
        f = fit_chain(pairs_of(lb.cnt[w], lb.head[w], lb.S, lb.Y, w), lb.x[:, w], lb.g[:, w], lb.alpha[:, w])
        if not f["ok"]:
            continue
        z = elbo_normals(seed, (chain0 + int(w)) & href.M64, D, lb.iters[w], n_elbo)
        batch[:, :, w], logq[:, w] = draw_map(f["mu"], f["sqa"], f["L"], f["logdet"], z)
        cand[w] = f
    with np.errstate(all="ignore"):
        lp = logpost(np.ascontiguousarray(batch.reshape(D, n_elbo * W)))[0].reshape(n_elbo, W)      # column k·W + c
    for w, f in cand.items():
        e = lref.osum((lp[:, w] - logq[:, w])[:, None])[0] / n_elbo if np.all(np.isfinite(lp[:, w])) else -np.inf
        ps.n_fits[w] += 1
        ps.history[w].append((int(lb.iters[w]), float(e)))
        if e > ps.elbo[w]:      # strict: the earliest fit wins a tie, −Inf never wins
            ps.elbo[w], ps.elbo_iter[w], ps.kept[w] = e, lb.iters[w], f
    return ps


def result(ps):
    out = lref.result(ps.lb)
    out.update(elbo=ps.elbo.copy(), elbo_iter=ps.elbo_iter.copy(), n_fits=ps.n_fits.copy(), state=ps, margin_elbo=elbo_margin(ps))
    return out


def elbo_margin(ps):
    """per chain: the gap between its two best ELBOs relative to max(1, |best|) (Inf with fewer than two candidates, NaN without a fit)"""
    out = np.full(len(ps.history), np.nan)
    for w, hist in enumerate(ps.history):
        e = sorted((v for _, v in hist if np.isfinite(v)), reverse=True)
        if e:
            out[w] = np.inf if len(e) < 2 else (e[0] - e[1]) / max(1.0, abs(e[0]))
    return out


def pathfinder(logpost, x, v=None, m=6, n_rounds=50, gtol=1e-6, ftol=0.0, seed=0, chain0=0, n_elbo=5, state=None):
    """n_rounds rounds from x (state: go on from a previous result's state). Unlike lbfgs_reference.lbfgs it runs every round: a round
    without an active chain changes nothing."""
    assert 1 <= n_elbo <= MAX_ELBO_DRAWS and (state is not None or x.shape[0] <= MAX_D)
    ps = State(lref.lbfgs_open(logpost, x, v, m)) if state is None else state
    for _ in range(n_rounds):
        pathfinder_round(logpost, ps, seed, chain0, n_elbo, gtol, ftol)
    return result(ps)


def pathfinder_draw(logpost, ps, seed, chain0, n_draws):
    """(φ [D, n·W] column j·W + c, log q [n·W], ℓπ [n·W]); a chain without a fit: its x, NaN, −Inf"""
    D, W = ps.lb.x.shape
    phi = np.repeat(ps.lb.x[:, None, :], n_draws, axis=1)
    logq = np.full((n_draws, W), np.nan)
    for w, f in enumerate(ps.kept):
        if f is not None:
            phi[:, :, w], logq[:, w] = draw_map(f["mu"], f["sqa"], f["L"], f["logdet"], final_normals(seed, (chain0 + w) & href.M64, D, n_draws))
    phi = np.ascontiguousarray(phi.reshape(D, n_draws * W))
    with np.errstate(all="ignore"):
        lp = np.array(logpost(phi)[0]).reshape(n_draws, W)
    lp[:, [f is None for f in ps.kept]] = -np.inf
    return phi, logq.reshape(-1), lp.reshape(-1)


def compact_sigma(pairs, alpha):
    """The Pathfinder paper's compact form: diag(α) + [αY, S]·γ·[αY, S]ᵀ with γ = [[0, −R⁻¹], [−R⁻ᵀ, R⁻ᵀ(E + YᵀαY)R⁻¹]], R the upper
    triangle of SᵀY, E its diagonal (S, Y the pairs as columns, oldest first)."""
    alpha = np.asarray(alpha)
    D, J = len(alpha), len(pairs)
    if J == 0:
        return np.diag(alpha)
    S, Y = np.stack([p[0] for p in pairs], axis=1), np.stack([p[1] for p in pairs], axis=1)
    R = np.triu(S.T @ Y)
    Ri = np.linalg.inv(R.astype(np.float64)).astype(alpha.dtype) if alpha.dtype != np.float64 else np.linalg.inv(R)
    if alpha.dtype != np.float64:      # one Newton step in the wide type: inv() is float64 only
        Ri = Ri @ (2 * np.eye(J, dtype=alpha.dtype) - R @ Ri)
        Ri = Ri @ (2 * np.eye(J, dtype=alpha.dtype) - R @ Ri)
    E = np.diag(np.diag(R))
    aY = alpha[:, None] * Y
    gamma = np.block([[np.zeros((J, J), dtype=alpha.dtype), -Ri], [-Ri.T, Ri.T @ (E + Y.T @ aY) @ Ri]])
    B = np.concatenate([aY, S], axis=1)
    return np.diag(alpha) + B @ gamma @ B.T
