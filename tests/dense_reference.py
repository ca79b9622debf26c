"""
The dense metric of include/octofitter_hip_draws.h (the fourteenth part), restated in NumPy: the pooled co-moments in the block / Chan order of
octo_draws_cov_device and in rational arithmetic, the regularised Cholesky factor with its `info` rule, the two triangular products, and the
HMC step and the NUTS transition under M⁻¹ = Σ = L·Lᵀ.

The samplers are stated in the TEXTBOOK form — p₀ = L⁻ᵀz with z the null-metric normals of hmc_reference.momentum, K = ½pᵀΣp, drift Σp, turn
tests ρᵀΣp — not in the device's whitened form r = Lᵀp, so that a comparison with the device also proves the equivalence of the two.
form="whitened" states the device's form (r ~ N(0, I), kick Lᵀ∇E, drift L·r, identity products) for the CPU comparison of the two.
The tree logic is nuts_reference.nuts_transition's own: the metric enters that function through its _Setup alone, which is replaced for the
length of a call. It imports nothing of the library. Packed triangles: row i at i(i+1)/2.
"""
import contextlib
from fractions import Fraction

import numpy as np

import hmc_reference as ref
import nuts_reference as nuts

MAX_D = 64      # OCTO_DRAWS_DENSE_MAX_D
BLOCK = 256


# ---------------------------------------------------------------------------------------------------- packed triangles and the products
def pack(L):
    L = np.asarray(L, dtype=np.float64)
    return L[np.tril_indices(L.shape[0])].copy()


def unpack(packed, K):
    L = np.zeros((K, K))
    L[np.tril_indices(K)] = packed
    return L


def lower(L, x):
    """(L·x)_i, the sum over j = 0 … i in that order by fma — NumPy has none, so: plain products and sums, in that order"""
    K = L.shape[0]
    out = np.zeros_like(x)
    for i in range(K):
        s = np.zeros(x.shape[1:])
        for j in range(i + 1):
            s = s + L[i, j] * x[j]
        out[i] = s
    return out


def lower_t(L, x):
    """(Lᵀ·x)_j, the sum over i = j … K − 1 in that order"""
    K = L.shape[0]
    out = np.zeros_like(x)
    for j in range(K):
        s = np.zeros(x.shape[1:])
        for i in range(j, K):
            s = s + L[i, j] * x[i]
        out[j] = s
    return out


def product_scale(L, x, transpose):
    """Σ|terms| of each entry of the product: the scale of its rounding error"""
    A = np.abs(L.T if transpose else L)
    return A @ np.abs(x)


# ---------------------------------------------------------------------------------------------------- the pooled co-moments
def included(x):
    return np.all(np.isfinite(np.asarray(x, dtype=np.float64)), axis=0)


def exact_cov(x):
    """(count [1], mean [K], m2 [K(K+1)/2] packed, amax [K]) in rational arithmetic, each rounded once to a double (after
    adapt_reference.exact_moments): Σ(x_i − mean_i)(x_j − mean_j) = (n·Σx_i·x_j − Σx_i·Σx_j)/n, exact in integers."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    cols = np.nonzero(included(x))[0]
    n = cols.size
    mean, m2, amax = np.zeros(K), np.zeros(K * (K + 1) // 2), np.zeros(K)
    if n == 0:
        return np.array([0.0]), mean, m2, amax
    ints, dens = np.empty((K, n), dtype=object), []
    for k in range(K):
        ratios = [float(t).as_integer_ratio() for t in x[k, cols]]      # every denominator is a power of two
        den = max(q for _, q in ratios)
        ints[k] = [p * (den // q) for p, q in ratios]                   # the values as integers over one denominator
        dens.append(den)
        mean[k] = float(Fraction(sum(ints[k]), n * den))
        amax[k] = np.max(np.abs(x[k, cols]))
    sums = ints.sum(axis=1)
    cross = ints @ ints.T                                               # Python integers: exact
    for i in range(K):
        for j in range(i + 1):
            m2[i * (i + 1) // 2 + j] = float(Fraction(n * cross[i, j] - sums[i] * sums[j], n * dens[i] * dens[j]))
    return np.array([float(n)]), mean, m2, amax


def cov(x, held=None):
    """(count [1], mean [K], m2 [K(K+1)/2]) in the order of octo_draws_cov_device: blocks of 256 chains two-pass about the block's mean, merged in
    block order by Chan's formula (cross term d_i·d_j·n·n_b/(n + n_b)); held = (count, mean, m2): then merged into those (accumulate = 1), new arrays."""
    x = np.asarray(x, dtype=np.float64)
    K, W = x.shape
    keep = included(x)
    tri = np.tril_indices(K)
    n, s, m2 = 0.0, np.zeros(K), np.zeros(K * (K + 1) // 2)
    for b0 in range(0, W, BLOCK):
        v = x[:, b0:b0 + BLOCK][:, keep[b0:b0 + BLOCK]]
        nb = float(v.shape[1])
        if nb == 0:
            continue
        sb = v.sum(axis=1)
        dev = v - (sb / nb)[:, None]
        mb = (dev @ dev.T)[tri]
        if n == 0:
            n, s, m2 = nb, sb, mb
            continue
        d = sb / nb - s / n
        m2 = m2 + mb + np.outer(d, d)[tri] * n * nb / (n + nb)
        s = s + sb
        n = n + nb
    mean = s / n if n > 0 else np.zeros(K)
    if held is None:
        return np.array([n]), mean, m2
    ca, ma, sa = (np.array(t, dtype=np.float64) for t in held)
    if n == 0:
        return ca, ma, sa
    na = float(ca[0])
    if na == 0:
        return np.array([n]), mean, m2
    d = mean - ma
    return np.array([na + n]), ma + d * n / (na + n), sa + m2 + np.outer(d, d)[tri] * na * n / (na + n)


def factor(count, m2, chol, regularize=True):
    """(chol, info) of octo_draws_metric_dense_device: Σ = M2/(n − 1), with regularize (n/(n + 5))·Σ + 1e-3·(5/(n + 5))·I; the left-looking Cholesky
    with its sums in index order. info = 0 and the new packed factor, or info = j + 1 (pivot j not finite and > 0; n < 2: 1) and chol as it was."""
    n = float(np.asarray(count).reshape(-1)[0])
    chol = np.array(chol, dtype=np.float64)
    if not n >= 2:
        return chol, 1
    P = np.asarray(m2).size
    K = int(round((np.sqrt(8 * P + 1) - 1) / 2))
    with np.errstate(all="ignore"):
        A = unpack(np.asarray(m2, dtype=np.float64) / (n - 1.0), K)
        if regularize:
            A = (n / (n + 5.0)) * A
            A[np.diag_indices(K)] = A[np.diag_indices(K)] + 1e-3 * 5.0 / (n + 5.0)
        for j in range(K):
            s = A[j:, j].copy()
            for k in range(j):
                s = s - A[j:, k] * A[j, k]
            d = s[0]
            if not (np.isfinite(d) and d > 0):
                return chol, j + 1
            l = np.sqrt(d)
            A[j:, j] = s / l
            A[j, j] = l
    return pack(A), 0


# ---------------------------------------------------------------------------------------------------- the samplers
def null_momentum(seed, step, chain0, W, D):
    """z [D][W]: the standard normals octo_draws_momentum_device draws with a NULL metric"""
    return ref.momentum(seed, step, chain0, W, D, None)


def textbook_momentum(L, z):
    """p = L⁻ᵀz ~ N(0, Σ⁻¹), by back substitution"""
    K = L.shape[0]
    p = np.zeros_like(z)
    for j in range(K - 1, -1, -1):
        s = z[j].copy()
        for i in range(j + 1, K):
            s = s - L[i, j] * p[i]
        p[j] = s / L[j, j]
    return p


def hmc_step_dense(priors, theta_t, beta, eps, n_leapfrog, L, seed, step, chain0=0, logpost=None, form="textbook"):
    """hmc_reference.hmc_step under M⁻¹ = L·Lᵀ (L [D, D] lower). The same outputs."""
    assert form in ("textbook", "whitened")
    theta_t = np.array(theta_t, dtype=np.float64)
    D, W = theta_t.shape
    L = np.asarray(L, dtype=np.float64)
    assert n_leapfrog >= 1 and D == len(priors) and L.shape == (D, D)
    Sigma = L @ L.T
    beta = np.zeros(W) if logpost is None else (np.ones(W) if beta is None else np.broadcast_to(np.asarray(beta, dtype=np.float64), (W,)))
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), (W,))
    if form == "textbook":
        kinetic = lambda p: 0.5 * np.sum(p * (Sigma @ p), axis=0)      # noqa: E731
        velocity = lambda p: Sigma @ p                                 # noqa: E731
        force = lambda g: g                                            # noqa: E731
    else:
        kinetic = lambda r: 0.5 * np.sum(r * r, axis=0)                # noqa: E731
        velocity = lambda r: lower(L, r)                               # noqa: E731
        force = lambda g: lower_t(L, g)                                # noqa: E731
    with np.errstate(all="ignore"):
        z = null_momentum(seed, step, chain0, W, D)
        p = textbook_momentum(L, z) if form == "textbook" else z
        E0, g, dead0, lp0, lpt0 = ref.tempered(priors, theta_t, beta, logpost)
        H0 = -E0 + kinetic(p)
        q = theta_t.copy()
        p = p + 0.5 * eps * force(g)
        for s in range(1, n_leapfrog + 1):
            q = q + eps * velocity(p)
            E1, g, dead1, lp1, lpt1 = ref.tempered(priors, q, beta, logpost)
            p = p + (eps if s < n_leapfrog else 0.5 * eps) * force(g)
        dH = H0 - (-E1 + kinetic(p))
        log_u = np.log(ref.accept_uniforms(seed, step, chain0, W))
        acc = ~dead1 & (dead0 | (log_u < dH))
        out = np.where(acc[None, :], q, theta_t)
        lp = np.where(acc, lp1, lp0)
        ll = np.where(acc, lp1 - lpt1, lp0 - lpt0)
        ll = np.where(np.isfinite(ll), ll, -np.inf)
    return dict(theta_t=out, proposal=q, logpost=lp, loglike=ll, dH=dH, accepted=acc, log_u=log_u, E0=E0, E1=E1)


class _TextbookSetup(nuts._Setup):
    """nuts_reference._Setup with p ~ N(0, Σ⁻¹): every place the metric occurs takes Σ"""
    L = None

    def __init__(self, *a):
        super().__init__(*a)
        self.Sigma = self.L @ self.L.T

    def dot(self, x, y):
        return np.sum(x * (self.Sigma @ y), axis=0)

    def kinetic(self, p):
        return 0.5 * self.dot(p, p)

    def open(self):
        p0 = textbook_momentum(self.L, null_momentum(self.seed, self.step, self.chain0, self.W, self.D))
        E0, g0, dead0, lp0, lpt0 = self.evaluate(self.theta_t, slice(None))
        return p0, g0, dead0, lp0, lpt0, -E0 + self.kinetic(p0)

    def half_kick_and_drift(self, q, p, g, v, e):
        ph = p + (v * (0.5 * e)) * g
        return q + (v * e) * (self.Sigma @ ph), ph


class _WhitenedSetup(nuts._Setup):
    """the device's form: r = Lᵀp ~ N(0, I), the identity in K and in every product, Lᵀ on the gradient of a kick, L on the momentum of a drift"""
    L = None

    def open(self):
        r0 = null_momentum(self.seed, self.step, self.chain0, self.W, self.D)
        E0, g0, dead0, lp0, lpt0 = self.evaluate(self.theta_t, slice(None))
        return r0, g0, dead0, lp0, lpt0, -E0 + self.kinetic(r0)

    def half_kick_and_drift(self, q, p, g, v, e):
        ph = p + (v * (0.5 * e)) * lower_t(self.L, g)
        return q + (v * e) * lower(self.L, ph), ph

    def closing_half_kick(self, ph, g, v, e):
        return ph + (v * (0.5 * e)) * lower_t(self.L, g)


@contextlib.contextmanager
def _setup(cls, L):
    """nuts_reference builds its _Setup by that name: for the length of a call the name holds the dense one"""
    sub = type(cls.__name__, (cls,), dict(L=np.asarray(L, dtype=np.float64)))
    before = nuts._Setup
    nuts._Setup = sub
    try:
        yield
    finally:
        nuts._Setup = before


def nuts_transition_dense(priors, theta_t, beta, eps, L, max_depth, seed, step, chain0=0, logpost=None, form="textbook"):
    """nuts_reference.nuts_transition under M⁻¹ = L·Lᵀ (L [D, D] lower): its outputs, `margin` among them (the products of the turn tests relative to
    ‖p‖·‖ρ‖ in the metric of the form)."""
    assert form in ("textbook", "whitened")
    with _setup(_TextbookSetup if form == "textbook" else _WhitenedSetup, L):
        return nuts.nuts_transition(priors, theta_t, beta, eps, None, max_depth, seed, step, chain0=chain0, logpost=logpost)
