"""
NumPy restatement of the batched L-BFGS of include/octofitter_hip_draws.h (octo_draws_lbfgs_device, octo_draws_lbfgs_direction_device):
W chains in lockstep, one `logpost` call over all trial points a round. Arrays are [D, W] (the pair ring [m, D, W]); every sum over d runs in
index order, as the header states. `logpost(theta_t) -> (ℓπ [W], ∇ℓπ [D, W])` is the oracle's callback in the tests. A plain module.
"""
import numpy as np

ACTIVE, GTOL, FTOL, LINESEARCH, DEAD = 0, 1, 2, 3, 4
MAX_M = 8
C1, CURV, MAX_BACKTRACKS = 1e-4, 1e-10, 30


def osum(x):
    """Σ over axis 0 in index order (np.sum pairs its terms)."""
    acc = np.zeros(x.shape[1:], dtype=x.dtype)
    for row in x:
        acc = acc + row
    return acc


def slot_of(head, k, m):
    """the slot of the pair k steps back from the newest, head being the slot the next pair would take"""
    return (head - 1 - k) % m


def direction(cnt, head, S, Y, g, v=None, sy=None):
    """The two-loop recursion of every chain: d = −H·g, H the L-BFGS inverse Hessian of the chain's cnt newest pairs from H₀ = γ·diag(v).
    cnt, head: int [W]; S, Y: [m, D, W]; g: [D, W]; sy: sᵀy per slot [m, W] (summed from S and Y when None)."""
    m, D, W = S.shape
    v = np.ones(D, dtype=g.dtype) if v is None else np.asarray(v, dtype=g.dtype)
    cnt = np.clip(np.asarray(cnt), 0, m)
    head = np.asarray(head) % m
    lanes = np.arange(W)
    if sy is None:
        sy = np.stack([osum(S[k] * Y[k]) for k in range(m)])
    q = g.copy()
    coef = np.zeros((m, W), dtype=g.dtype)
    with np.errstate(all="ignore"):
        for k in range(m):
            on = k < cnt
            slot = slot_of(head, k, m)
            s, y = S[slot, :, lanes].T, Y[slot, :, lanes].T
            c = osum(s * q) / sy[slot, lanes]
            coef[k] = c
            q = np.where(on, q - c * y, q)
        newest = slot_of(head, 0, m)
        yn = Y[newest, :, lanes].T
        gamma = np.where(cnt > 0, sy[newest, lanes] / osum(yn * yn * v[:, None]), 1.0)
        r = q * (gamma * v[:, None])
        for k in range(m - 1, -1, -1):
            on = k < cnt
            slot = slot_of(head, k, m)
            s, y = S[slot, :, lanes].T, Y[slot, :, lanes].T
            c = coef[k] - osum(y * r) / sy[slot, lanes]
            r = np.where(on, r + c * s, r)
    return -r


def alpha_update(alpha, s, y):
    """The Pathfinder diagonal after the pair (s, y): the diagonal of the BFGS update of (a/b)·diag(1/α)."""
    a, b, c = osum(y * y * alpha), osum(s * y), osum(s * s / alpha)
    return 1.0 / (a / (b * alpha) + y * y / b - a * s * s / (b * c * alpha * alpha))


class State:
    """The chains' state between rounds (what the handle holds)."""

    def __init__(self, x, v, m):
        D, W = x.shape
        self.x, self.v, self.m = x.copy(), v, m
        self.S, self.Y, self.sy = np.zeros((m, D, W)), np.zeros((m, D, W)), np.zeros((m, W))
        self.cnt, self.head = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
        self.status, self.iters, self.evals, self.nbt = (np.zeros(W, dtype=np.int32) for _ in range(4))
        self.margin = np.full(W, np.inf)      # the smallest |f_t − (f + c1·t·gd)| / max(1, |f|) a decision of the chain had (with ftol > 0
                                              # also the smallest ||f_old − f| − ftol·max(1, |f|)| / max(1, |f|) of its ftol tests)
        self.decisions = []                   # per round: +1 accepted, −1 rejected, 0 frozen

    def steepest(self, on):
        d = -self.v[:, None] * self.g
        self.dir = np.where(on, d, self.dir)
        self.gd = np.where(on, osum(self.g * d), self.gd)


def lbfgs_open(logpost, x, v, m):
    D, W = x.shape
    v = np.ones(D) if v is None else np.asarray(v, dtype=np.float64)
    st = State(np.asarray(x, dtype=np.float64), v, m)
    with np.errstate(all="ignore"):
        lp, glp = logpost(st.x)
        st.f, st.g = -lp, -glp
        fin = np.isfinite(st.f) & np.all(np.isfinite(st.g), axis=0)
        st.status[:] = np.where(fin, ACTIVE, DEAD)
        st.evals[:] = 1
        st.alpha = np.repeat(v[:, None], W, axis=1)
        st.gn = np.where(fin, np.max(np.abs(st.g) * np.sqrt(v)[:, None], axis=0), np.nan)
        st.dir, st.gd = np.zeros((D, W)), np.zeros(W)
        st.steepest(fin)
        st.t = np.where(fin, np.minimum(1.0, 1.0 / np.sqrt(osum(v[:, None] * st.g * st.g))), 0.0)
        st.trial = np.where(fin, st.x + st.t * st.dir, st.x)
    return st


def lbfgs_round(logpost, st, gtol=1e-6, ftol=0.0):
    m, v, W = st.m, st.v, st.x.shape[1]
    lanes = np.arange(W)
    with np.errstate(all="ignore"):
        lp, glp = logpost(st.trial)
        ft, gt = -lp, -glp
        act = st.status == ACTIVE
        st.evals[act] += 1
        bound = st.f + C1 * st.t * st.gd
        fin = np.isfinite(ft) & np.all(np.isfinite(gt), axis=0)
        acc = act & fin & (ft <= bound)
        rej = act & ~acc
        mg = np.abs(ft - bound) / np.maximum(1.0, np.abs(st.f))
        st.margin = np.where(act & fin, np.minimum(st.margin, mg), st.margin)
        st.decisions.append(np.where(acc, 1, np.where(rej, -1, 0)))
        # accept
        s, y = st.trial - st.x, gt - st.g
        sy, ss, yy = osum(s * y), osum(s * s / v[:, None]), osum(y * y * v[:, None])
        store = acc & (sy > CURV * np.sqrt(ss * yy))
        new_alpha = alpha_update(st.alpha, s, y)
        for w in lanes[store]:
            st.S[st.head[w], :, w], st.Y[st.head[w], :, w], st.sy[st.head[w], w] = s[:, w], y[:, w], sy[w]
        st.alpha = np.where(store, new_alpha, st.alpha)
        st.head = np.where(store, (st.head + 1) % m, st.head)
        st.cnt = np.where(store, np.minimum(st.cnt + 1, m), st.cnt)
        f_old = st.f
        st.x, st.g, st.f = np.where(acc, st.trial, st.x), np.where(acc, gt, st.g), np.where(acc, ft, st.f)
        st.iters[acc] += 1
        st.nbt[acc] = 0
        gn = np.max(np.abs(st.g) * np.sqrt(v)[:, None], axis=0)
        st.gn = np.where(acc, gn, st.gn)
        conv_g = acc & (gn <= gtol)
        conv_f = acc & ~conv_g & (ftol > 0.0) & (np.abs(f_old - st.f) <= ftol * np.maximum(1.0, np.abs(st.f)))
        if ftol > 0.0:
            fm = np.abs(np.abs(f_old - st.f) / np.maximum(1.0, np.abs(st.f)) - ftol)
            st.margin = np.where(acc & ~conv_g, np.minimum(st.margin, fm), st.margin)
        st.status[conv_g], st.status[conv_f] = GTOL, FTOL
        go = acc & ~conv_g & ~conv_f
        d = direction(st.cnt, st.head, st.S, st.Y, st.g, v, sy=st.sy)
        st.dir = np.where(go, d, st.dir)
        st.gd = np.where(go, osum(st.g * st.dir), st.gd)
        back = go & ~(st.gd < 0.0)
        st.cnt, st.head = np.where(back, 0, st.cnt), np.where(back, 0, st.head)
        st.steepest(back)
        st.t = np.where(go, 1.0, st.t)
        # reject
        st.t = np.where(rej, 0.5 * st.t, st.t)
        st.nbt[rej] += 1
        st.status[rej & (st.nbt > MAX_BACKTRACKS)] = LINESEARCH
        moving = st.status == ACTIVE
        st.trial = np.where(moving, st.x + st.t * st.dir, st.x)
    return st


def result(st):
    return dict(theta_t=st.x.copy(), logpost=-st.f, gnorm=st.gn.copy(), status=st.status.copy(), iters=st.iters.copy(), evals=st.evals.copy(),
                inv_hess_diag=st.alpha.copy(), margin=st.margin.copy(), decisions=np.array(st.decisions).reshape(-1, st.x.shape[1]), state=st)


def lbfgs(logpost, x, v=None, m=6, n_rounds=50, gtol=1e-6, ftol=0.0, state=None):
    """n_rounds rounds from x (state: go on from a previous result's state instead). Stops early once no chain is active: the remaining
    rounds would change nothing."""
    st = lbfgs_open(logpost, x, v, m) if state is None else state
    for _ in range(n_rounds):
        if not np.any(st.status == ACTIVE):
            break
        lbfgs_round(logpost, st, gtol, ftol)
    return result(st)


def dense_inverse_bfgs(pairs, v, gamma):
    """H after the inverse-BFGS updates of H₀ = γ·diag(v) with the pairs (s, y), oldest first — what the two-loop recursion applies."""
    H = gamma * np.diag(v)
    I = np.eye(len(v), dtype=H.dtype)
    for s, y in pairs:
        rho = 1.0 / (s @ y)
        V = I - rho * np.outer(s, y)
        H = V @ H @ V.T + rho * np.outer(s, s)
    return H
