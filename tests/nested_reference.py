"""
Nested sampling of include/octofitter_hip_draws.h (octo_draws_cube_device, octo_draws_from_cube_device, octo_draws_nested_cull_device,
octo_draws_nested_move_device) and the driver on top of them (host/callers.py: octofit_nested_device), restated in NumPy on top of
tests/hmc_reference.py (the counter generator, the priors). It imports nothing of the library. The likelihood is any callable
loglike(u [D, n]) -> ℓ [n] on points of the unit cube; model_loglike builds the rejection driver's ℓ = ℓπ − ℓprior_t from a logpost callable.

    u = cube(seed, first, n, D)                                  the uniforms of purpose 0
    θ, θ_t, ℓprior_t = from_cube(priors, u)                      the hypercube transform; a column with a coordinate outside (0, 1) is NaN
    r = cull(u_live, ll_live, state, B, replace, seed, it)       one iteration's bookkeeping: r["u_live"], r["ll_live"], r["state"], r["slot"], r["src"],
                                                                 r["width"], r["dead_u"], r["dead_ll"], r["dead_logvol"], r["dead_logwt"]
    r = move(loglike, u_live, ll_live, floor, slot, w, …)        the constrained-prior transition in lockstep rounds, vectorised over the chains:
                                                                 r["u_live"], r["ll_live"], the counts, r["status"], r["margin"], r["rounds"]
    r = move_plain(…)                                            the same a second time, as plainly as it can be: chain by chain, nested loops
    r = run(loglike, D, …)                                       the driver: logz, logz_err, information, the weighted dead points, samples, …

margin: per chain the smallest |ℓ_trial − ℓ*| of any evaluation it made, relative to max(1, |ℓ*|). A chain whose margin exceeds MARGIN = 1e-6 is
DECIDED: a computation that differs in the last bits makes the same decisions.
"""
import math

import numpy as np

import hmc_reference as ref

PURPOSE_NESTED_SEED, PURPOSE_NESTED_MOVE = 10, 11
MAX_LIVE, MAX_STEPS, MAX_SHRINK, MAX_PASSES = 4096, 64, 64, 1024
ACTIVE, DONE = 0, 1
MARGIN = 1e-6
PH_L, PH_R, PH_X = range(3)
ST_EVAL, ST_NEXT, ST_OPEN, ST_LEFT, ST_RIGHT, ST_CLIP, ST_PROPOSE, ST_DONE = range(8)
STATE0 = (-math.inf, 0.0, -math.inf, -math.inf, math.inf, 0.0, 0.0, 0.0)      # logZ, logX, ℓ*, ℓmax, the remaining-evidence bound, dead so far, reserved
# the driver's defaults: the project's own
DEFAULTS = dict(n_live=1024, batch=256, n_passes=4, max_steps=8, max_shrink=64, dlogz=0.01, max_iter=2000, n_samples=4096)


# ---------------------------------------------------------------------------------------------------- the counters
def seed_counter(r, it):
    return (int(r), 0, PURPOSE_NESTED_SEED, int(it) & ref.M64)


def move_counter(c, j, i, it):
    """(c, j·128 + i, 11, iter): i = 0 the interval's position (word 1) and the split of the steps (word 2), i = 64 + s shrink proposal s (word 0)"""
    assert 0 <= i < 128
    return (int(c) & ref.M64, int(j) * 128 + int(i), PURPOSE_NESTED_MOVE, int(it) & ref.M64)


def _u01_int(x):
    return float(2 * (x >> 12) + 1) * 2.0 ** -53


def move_uniforms(seed, it, c, j, i):
    """(v, v′, v″) of words 0, 1, 2 of the counter (c, j·128 + i, 11, iter), one triple per chain"""
    words = ref.philox_vec((seed, ref.KEY1), np.asarray(c, dtype=np.uint64), np.asarray(j, dtype=np.uint64) * np.uint64(128) + np.asarray(i, dtype=np.uint64),
                           PURPOSE_NESTED_MOVE, np.uint64(it))
    return ref.u01(words[0]), ref.u01(words[1]), ref.u01(words[2])


# ---------------------------------------------------------------------------------------------------- 1. the cube
def cube(seed, first, n, D):
    return ref.prior_uniforms(seed, np.uint64(first) + np.arange(n, dtype=np.uint64), D)


def from_cube(priors, u):
    """(θ, θ_t [D][n], ℓprior_t [n]): hmc_reference.prior_sample's quantile, nudge and link on given uniforms; NaN where a column leaves (0, 1)"""
    u = np.asarray(u, dtype=np.float64)
    bad = ~np.all((u > 0.0) & (u < 1.0), axis=0)
    v = np.where(bad[None, :], 0.5, u)
    th, tt = np.empty_like(v), np.empty_like(v)
    for d, pr in enumerate(priors):
        a, b = ref.support(pr)
        x = ref.scipy_dist(pr)[1](v[d])
        if math.isfinite(a):
            x = np.where(x > a, x, np.nextafter(a, math.inf))
        if math.isfinite(b):
            x = np.where(x < b, x, np.nextafter(b, -math.inf))
        th[d], tt[d] = x, ref.link(pr, x)
    lpt = ref.logprior_t(priors, tt)[0]
    th[:, bad], tt[:, bad], lpt[bad] = np.nan, np.nan, np.nan
    return th, tt, lpt


def model_loglike(priors, logpost):
    """loglike(u) of the rejection driver on a model: ℓπ(θ_t(u)) − ℓprior_t(θ_t(u)), non-finite -> −Inf; logpost(θ_t) -> (ℓπ, anything)"""
    def loglike(u):
        _, tt, lpt = from_cube(priors, u)
        lp = np.asarray(logpost(np.ascontiguousarray(tt))[0], dtype=np.float64)
        with np.errstate(all="ignore"):
            ll = lp - lpt
        return np.where(np.isfinite(ll), ll, -np.inf)
    return loglike


# ---------------------------------------------------------------------------------------------------- 2. the cull
def key_of(ll):
    ll = np.asarray(ll, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(ll > -np.inf, ll, -np.inf)


def logaddexp(a, b):
    if a == -math.inf and b == -math.inf:
        return -math.inf
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def cull(u_live, ll_live, state, B, replace, seed=0, it=0):
    u, ll, st = np.array(u_live, dtype=np.float64), np.array(ll_live, dtype=np.float64), np.array(state, dtype=np.float64)
    D, K = u.shape
    assert 2 <= K <= MAX_LIVE and (1 <= B <= K - 1 if replace else B == K)
    key = key_of(ll)
    order = np.array(sorted(range(K), key=lambda i: (key[i], i)))
    logZ, logX = float(st[0]), float(st[1])
    logvol, logwt = np.empty(B), np.empty(B)
    for r in range(B):
        t = 1.0 / (K - r)
        logwt[r] = (key[order[r]] + logX) + math.log(-math.expm1(-t))
        logX -= t
        logZ = logaddexp(logZ, logwt[r])
        logvol[r] = logX
    lmax = float(key[order[K - 1]])
    st[:] = (logZ, logX, key[order[B - 1]], lmax, math.inf if logZ == -math.inf else logaddexp(logZ, lmax + logX) - logZ, st[5] + B, 0.0, 0.0)
    slot = order[:B].astype(np.int32)
    out = dict(state=st, slot=slot, dead_u=u[:, slot].copy(), dead_ll=key[slot].copy(), dead_logvol=logvol, dead_logwt=logwt, width=None, src=None, order=order)
    if replace:
        words = ref.philox_vec((seed, ref.KEY1), np.arange(B, dtype=np.uint64), 0, PURPOSE_NESTED_SEED, np.uint64(it))
        pick = np.minimum(K - B - 1, np.floor(ref.u01(words[0]) * (K - B)).astype(np.int64))
        src = order[B + pick]
        out["width"] = np.array([np.fmax.reduce(u[d]) - np.fmin.reduce(u[d]) for d in range(D)])
        u[:, slot] = u[:, src]
        ll[slot] = ll[src]
        out["src"] = src.astype(np.int32)
    out["u_live"], out["ll_live"] = u, ll
    return out


# ---------------------------------------------------------------------------------------------------- 3. the move
def _margin(ll, floor):
    with np.errstate(invalid="ignore"):
        m = np.abs(ll - floor) / max(1.0, abs(floor)) if math.isfinite(floor) else np.full(np.shape(ll), np.inf)
    return np.where(np.isfinite(ll), m, np.inf)


def move(loglike, u_live, ll_live, floor, slot, w, max_steps, n_passes, max_shrink, seed, it, max_rounds=None):
    """The lockstep restatement: a round is one loglike call at the trial points of the chains still active and one step of every such chain's
    state machine; between two evaluations a chain runs through the stages that need none. max_rounds: stop there (the chains stay ACTIVE)."""
    assert 1 <= max_steps <= MAX_STEPS and 1 <= max_shrink <= MAX_SHRINK and 1 <= n_passes <= MAX_PASSES
    u, ll_out = np.array(u_live, dtype=np.float64), np.array(ll_live, dtype=np.float64)
    D = u.shape[0]
    slot = np.asarray(slot, dtype=np.int64)
    B = slot.size
    widths = np.array(np.broadcast_to(np.asarray(w, dtype=np.float64), (D,)))
    n_updates = n_passes * D
    L, R, x, xp, y = (np.zeros(B) for _ in range(5))
    j = np.full(B, -1, dtype=np.int64)
    s, J, Kr, phase, n_eval, n_step, n_shrink, n_stuck = (np.zeros(B, dtype=np.int64) for _ in range(8))
    stage = np.full(B, ST_NEXT)
    status = np.full(B, ACTIVE)
    margin = np.full(B, np.inf)

    def advance(act):
        while True:
            act = act[(stage[act] != ST_EVAL) & (stage[act] != ST_DONE)]
            if not act.size:
                return
            m = act[stage[act] == ST_NEXT]
            fin = m[j[m] + 1 == n_updates]
            stage[fin], status[fin] = ST_DONE, DONE
            go = m[j[m] + 1 < n_updates]
            j[go] += 1
            stage[go] = ST_OPEN
            m = act[stage[act] == ST_OPEN]
            if m.size:
                d = j[m] % D
                _v, v1, v2 = move_uniforms(seed, it, slot[m], j[m], 0)
                x[m] = u[d, slot[m]]
                L[m] = x[m] - widths[d] * v1
                R[m] = L[m] + widths[d]
                J[m] = np.minimum(max_steps - 1, np.floor(max_steps * v2).astype(np.int64))
                Kr[m] = max_steps - 1 - J[m]
                s[m] = 0
                stage[m] = ST_LEFT
            m = act[stage[act] == ST_LEFT]
            ok = (J[m] > 0) & (L[m] > 0.0) & (L[m] < 1.0)
            y[m[ok]], phase[m[ok]], stage[m[ok]] = L[m[ok]], PH_L, ST_EVAL
            stage[m[~ok]] = ST_RIGHT
            m = act[stage[act] == ST_RIGHT]
            ok = (Kr[m] > 0) & (R[m] > 0.0) & (R[m] < 1.0)
            y[m[ok]], phase[m[ok]], stage[m[ok]] = R[m[ok]], PH_R, ST_EVAL
            stage[m[~ok]] = ST_CLIP
            m = act[stage[act] == ST_CLIP]
            L[m], R[m] = np.maximum(L[m], 0.0), np.minimum(R[m], 1.0)
            stage[m] = ST_PROPOSE
            m = act[stage[act] == ST_PROPOSE]
            stuck = m[s[m] == max_shrink]
            n_stuck[stuck] += 1
            stage[stuck] = ST_NEXT
            m = m[s[m] < max_shrink]
            if m.size:
                v0, _v1, _v2 = move_uniforms(seed, it, slot[m], j[m], 64 + s[m])
                xp[m] = L[m] + v0 * (R[m] - L[m])
                n_shrink[m] += 1
                ok = (xp[m] > 0.0) & (xp[m] < 1.0)
                y[m[ok]], phase[m[ok]], stage[m[ok]] = xp[m[ok]], PH_X, ST_EVAL
                out = m[~ok]
                left = xp[out] < x[out]
                L[out[left]] = xp[out[left]]
                R[out[~left]] = xp[out[~left]]
                s[out] += 1

    advance(np.arange(B))
    rounds = 0
    while (max_rounds is None or rounds < max_rounds) and np.any(status == ACTIVE):
        rounds += 1
        a = np.nonzero(status == ACTIVE)[0]
        d = j[a] % D
        pts = u[:, slot[a]].copy()
        pts[d, np.arange(a.size)] = y[a]
        with np.errstate(all="ignore"):
            ll = np.asarray(loglike(pts), dtype=np.float64)
        ll = np.where(np.isfinite(ll), ll, -np.inf)
        margin[a] = np.minimum(margin[a], _margin(ll, floor))
        inside = ll > floor
        n_eval[a] += 1
        ph = phase[a]
        m = a[(ph == PH_L) & inside]
        L[m] -= widths[j[m] % D]
        J[m] -= 1
        n_step[m] += 1
        stage[m] = ST_LEFT
        stage[a[(ph == PH_L) & ~inside]] = ST_RIGHT
        m = a[(ph == PH_R) & inside]
        R[m] += widths[j[m] % D]
        Kr[m] -= 1
        n_step[m] += 1
        stage[m] = ST_RIGHT
        stage[a[(ph == PH_R) & ~inside]] = ST_CLIP
        acc = (ph == PH_X) & inside
        m = a[acc]
        u[j[m] % D, slot[m]] = xp[m]
        ll_out[slot[m]] = ll[acc]
        stage[m] = ST_NEXT
        m = a[(ph == PH_X) & ~inside]
        left = xp[m] < x[m]
        L[m[left]] = xp[m[left]]
        R[m[~left]] = xp[m[~left]]
        s[m] += 1
        stage[m] = ST_PROPOSE
        advance(a)
    return dict(u_live=u, ll_live=ll_out, n_eval=n_eval, n_step=n_step, n_shrink=n_shrink, n_stuck=n_stuck, status=status, margin=margin, rounds=rounds)


def move_plain(loglike, u_live, ll_live, floor, slot, w, max_steps, n_passes, max_shrink, seed, it):
    """Chain by chain, update by update: Neal's stepping out and shrinkage as loops, every evaluation made where the figure makes it."""
    u, ll_out = np.array(u_live, dtype=np.float64), np.array(ll_live, dtype=np.float64)
    D = u.shape[0]
    widths = np.array(np.broadcast_to(np.asarray(w, dtype=np.float64), (D,)))
    B = len(slot)
    counts = {k: np.zeros(B, dtype=np.int64) for k in ("n_eval", "n_step", "n_shrink", "n_stuck")}
    for k, c in enumerate(int(v) for v in slot):
        def uniforms(j, i):
            words = ref.philox_int((seed, ref.KEY1), move_counter(c, j, i, it))
            return _u01_int(words[0]), _u01_int(words[1]), _u01_int(words[2])

        for j in range(n_passes * D):
            d = j % D
            wd, x = float(widths[d]), float(u[d, c])

            def inside(yv):
                if not 0.0 < yv < 1.0:
                    return False, None
                counts["n_eval"][k] += 1
                p = u[:, c:c + 1].copy()
                p[d, 0] = yv
                with np.errstate(all="ignore"):
                    v = float(np.asarray(loglike(p), dtype=np.float64)[0])
                v = v if math.isfinite(v) else -math.inf
                return v > floor, v

            _v, v1, v2 = uniforms(j, 0)
            L = x - wd * v1
            R = L + wd
            J = min(max_steps - 1, int(math.floor(max_steps * v2)))
            Kr = max_steps - 1 - J
            while J > 0 and inside(L)[0]:
                L, J = L - wd, J - 1
                counts["n_step"][k] += 1
            while Kr > 0 and inside(R)[0]:
                R, Kr = R + wd, Kr - 1
                counts["n_step"][k] += 1
            L, R = max(L, 0.0), min(R, 1.0)
            for s in range(max_shrink):
                xp = L + uniforms(j, 64 + s)[0] * (R - L)
                counts["n_shrink"][k] += 1
                ok, v = inside(xp)
                if ok:
                    u[d, c], ll_out[c] = xp, v
                    break
                if xp < x:
                    L = xp
                else:
                    R = xp
            else:
                counts["n_stuck"][k] += 1
    return dict(u_live=u, ll_live=ll_out, status=np.full(B, DONE), **counts)


# ---------------------------------------------------------------------------------------------------- the driver
def summarise(dead_ll, dead_logwt, K, logz):
    """From the run's logZ (the state's): the information H = Σ p(ℓ − logZ), √(H/K), the weights p = exp(logwt − logZ) and their effective sample size"""
    lw = np.asarray(dead_logwt, dtype=np.float64)
    p = np.exp(lw - logz)
    ok = p > 0
    H = float(np.sum(p[ok] * (np.asarray(dead_ll)[ok] - logz)))
    return dict(logz=float(logz), information=H, logz_err=math.sqrt(max(H, 0.0) / K), weights=p, ess=float(np.sum(p) ** 2 / np.sum(p * p)))


def systematic_resample(p, n, v):
    """n indices by systematic resampling on the weights p from the one uniform v"""
    cum = np.cumsum(p)
    return np.minimum(np.searchsorted(cum / cum[-1], (v + np.arange(n)) / n, side="left"), len(p) - 1)


def run(loglike, D, n_live=DEFAULTS["n_live"], batch=DEFAULTS["batch"], n_passes=DEFAULTS["n_passes"], max_steps=DEFAULTS["max_steps"],
        max_shrink=DEFAULTS["max_shrink"], dlogz=DEFAULTS["dlogz"], max_iter=DEFAULTS["max_iter"], n_samples=DEFAULTS["n_samples"], seed=0):
    """octofit_nested_device, restated: K prior points of the cube, cull + move until the remaining-evidence bound falls below dlogz, the flush."""
    K, B = n_live, batch
    u = cube(seed, 0, K, D)
    with np.errstate(all="ignore"):
        ll = np.asarray(loglike(u), dtype=np.float64)
    ll = np.where(np.isfinite(ll), ll, -np.inf)
    state = np.array(STATE0)
    dead = {k: [] for k in ("dead_u", "dead_ll", "dead_logvol", "dead_logwt")}
    n_iter = n_evals = n_stuck = 0
    while n_iter < max_iter:
        c = cull(u, ll, state, B, True, seed, n_iter)
        for k in dead:
            dead[k].append(c[k])
        state = c["state"]
        r = move(loglike, c["u_live"], c["ll_live"], state[2], c["slot"], c["width"], max_steps, n_passes, max_shrink, seed, n_iter)
        u, ll = r["u_live"], r["ll_live"]
        n_evals += int(r["n_eval"].sum())
        n_stuck += int(r["n_stuck"].sum())
        n_iter += 1
        if state[4] < dlogz:
            break
    c = cull(u, ll, state, K, False, seed, n_iter)
    for k in dead:
        dead[k].append(c[k])
    du, dl, dw = np.concatenate(dead["dead_u"], axis=1), np.concatenate(dead["dead_ll"]), np.concatenate(dead["dead_logwt"])
    out = summarise(dl, dw, K, float(c["state"][0]))
    out.update(u=du, loglike=dl, logwt=dw, logvol=np.concatenate(dead["dead_logvol"]), state=c["state"], n_iter=n_iter, n_evals=n_evals + K, n_stuck=n_stuck)
    out["samples_u"] = du[:, systematic_resample(out["weights"], n_samples, cube(seed, K, 1, D)[0, 0])]      # coordinate 0 of prior draw K
    return out
